"""CPU proof that the inputs of tests/test_mx4b_gpu.py are sharp, and the host-side presence of the feature.  On every case of
tests/mx4b_ref.py each plausible mistake of the batched MXFP4 kernel (the float64 "mutant" references there) changes the stored bits of the
y buffer (exact family) or moves an output by at least 10x the bound the GPU test applies (SwiGLU, toleranced); the arg-max cases are held
to their planted winners, exact ties, the penalised winner and the row without a finite logit.  Each test prints its mutants (pytest -s)."""
import os
import re

import pytest
import torch

import gemv_ref as G
import mx4b_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_mx4b_inputs_are_discriminating(case):
    ref = case.build().reference()
    assert float(case.load().max()) < 2.0 ** 23, case.id                      # every fp32 partial sum is exact in any order
    rows = [tuple(r.tolist()) for r in torch.nan_to_num(case.x, nan=123.0)]
    assert len(set(rows)) == case.B, case.id                                   # every row of X differs
    if case.epi == "argmax":
        toks = case.tokens()
        for b in range(case.B):
            if b == case.nan_row:
                assert toks[b] == -1 and not bool(torch.isfinite(ref[b]).any())
                continue
            top = ref[b].max()
            assert float(top) == 8.0 and sorted(torch.nonzero(ref[b] == top).flatten().tolist()) == sorted(case.tie_sets[b]), (case.id, b)
            if b == case.pen_row:                                              # the penalised winner loses to its tie partner
                assert len(case.tie_sets[b]) == 2 and toks[b] == case.tie_sets[b][1], (case.id, b, toks[b])
            else:
                assert toks[b] == min(case.tie_sets[b]), (case.id, b)
        multi = [b for b in range(case.B) if b not in (case.nan_row, case.pen_row) and len(case.tie_sets[b]) > 1]
        assert multi and all(case.tokens("tie_higher")[b] != toks[b] for b in multi), case.id
        assert len({case.tie_sets[b] for b in range(case.B)}) == case.B       # a different place for each env
        return
    if case.exact:
        assert bool(G.representable(ref, torch.bfloat16).all()), case.id      # every expected output is a bf16 value
        base = case.image()
        report = {m: int((case.image(m) != base).sum()) for m in case.mutants()}
        weak = {k: v for k, v in report.items() if v < 1}
    else:
        lo, hi = case.gate_span()
        assert lo <= -12 and hi >= 12, (case.id, lo, hi)
        report = {m: float(((case.reference(m) - ref).abs() / G.bound(ref, torch.bfloat16)).max()) for m in case.mutants() if m != "col_leak"}
        report["col_leak"] = float((case.image("col_leak") != case.image()).sum())
        weak = {k: v for k, v in report.items() if v < 10.0}
    print(f"{case.id}: " + ", ".join(f"{k} {round(v, 1)}" for k, v in report.items()))
    assert not weak, f"{case.id}: mutants the case cannot see: {weak} (all: {report})"


def test_case_list_reaches_every_launch_form():
    """both wave counts of EPI_NONE and EPI_SWIGLU, more than one grid-stride pass of the arg-max, the shapes and batch sizes asked for"""
    forms = {(c.epi, R.geometry(c.N, c.epi)[0]) for c in R.CASES}
    assert {("none", 16), ("none", 4), ("swiglu", 16), ("swiglu", 4), ("argmax", 4)} <= forms
    assert any(c.epi == "argmax" and R.geometry(c.N, c.epi)[2] > 1 for c in R.CASES)
    small = [c for c in R.CASES if c.epi == "none" and c.N <= 515]
    assert {(c.N, c.K) for c in small} == {(n, k) for n in (1, 7, 16, 17, 515) for k in (32, 96, 160, 4128)}
    for K in (32, 96, 160, 4128):
        assert {c.B for c in small if c.K == K} == {1, 2, 3, 5, 8}
    assert all(c.ldw == c.K + 64 and c.ldy > c.n_out for c in R.CASES)


def test_public_surface_names_the_batched_mxfp4_mode():
    """the switch and the op entry point exist in the header, in the ctypes stub and as the model method"""
    from streamvln_amd import _lib
    from streamvln_amd.model import StreamVLNForCausalLM
    header = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
    for name in ("svln_set_mxfp4_batched", "svln_op_gemv_mxfp4_batched"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["svln_op_gemv_mxfp4_batched"][1]) == 16
    assert callable(getattr(StreamVLNForCausalLM, "set_mxfp4_batched", None))
