"""CPU proof that the inputs of tests/test_gemv_gpu.py are sharp.  On every case of that file, in both engine types, each plausible
kernel mistake that applies to the case (the float64 "mutant" references of tests/gemv_ref.py) changes the stored bits of at least one
expected output (exact family), or moves the expected output by at least 10x the bound the GPU test applies (toleranced family; the
ratio tests/test_attention_inputs.py uses).  The exact cases are held to their precondition (sum |w x| of a row below 2^23 quanta:
every fp32 partial sum is exact in any order) and to at least 90 % of the rows being values of the engine type; the arg-max cases to
their intended winner and exact ties.  Each test prints its mutants with the rows changed / the ratio (pytest -s, or on failure)."""
import pytest
import torch

import gemv_ref as R


def _check(case, report):
    print(f"{case.id}: " + ", ".join(f"{k} {v if case.exact else round(v, 1)}" for k, v in report.items()))
    weak = {k: v for k, v in report.items() if not (v >= 1 if case.exact else v >= 10.0)}
    assert not weak, f"{case.id}: mutants the case cannot see: {weak} (all: {report})"


def _exact_conditions(case, ref):
    load = case.load()
    assert float(load.max()) < 2.0 ** 23, (case.id, float(load.max()))
    stored = torch.float32 if case.epi == "argmax" else case.dtype          # logits are compared in fp32 and never stored
    frac = float(R.representable(ref, stored).double().mean())
    print(f"{case.id}: max load {float(load.max()):.0f} quanta, {100 * frac:.2f} % of the outputs are {stored} values")
    assert frac >= 0.90, (case.id, frac)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_gemv_inputs_are_discriminating(case):
    ref = case.build().reference()
    assert case.kernel == ("ksplit" if case.epi == "none" and case.N <= 8192 else "rows")
    if case.exact or case.family == "wide-gate":
        _exact_conditions(case, case.accumulate() if case.family == "wide-gate" else ref)
    if case.family == "wide-gate":
        lo, hi = case.gate_span()
        assert lo <= -12 and hi >= 12, (case.id, lo, hi)
    if case.norm:
        ms = float((case.x * case.x).mean())
        assert (0.1 * R.EPS < ms < 10 * R.EPS) if case.family == "eps" else ms > 1e5 * R.EPS, (case.id, ms)
    if case.epi == "argmax":
        top = ref.max()
        assert float(top) == case.top and int(torch.argmax(ref)) == case.winner == min(case.tie_set)
        assert sorted(torch.nonzero(ref == top).flatten().tolist()) == sorted(case.tie_set), case.id
        if case.tie == "negative":
            assert float(ref.max()) < 0
        if case.tie in ("group", "iterations", "waves", "workgroups"):       # the placement is what its name says
            (wa, va, ia), (wb, vb, ib) = (R.owner(case.N, "argmax", n) for n in case.tie_set)
            same_group = case.tie_set[0] // 4 == case.tie_set[1] // 4
            assert {"group": same_group, "iterations": (wa, va) == (wb, vb) and ia != ib, "waves": wa == wb and va != vb and ia == ib,
                    "workgroups": wa != wb}[case.tie], case.id
    _check(case, R.mutant_report(case))


def test_grid_stride_regimes():
    """the shapes of the grid-stride cases reach the regimes of gemv_grid they are meant for"""
    assert R.gemv_grid(37888) == 1184 and R.iterations(37888, "swiglu") == 2          # divisor search
    assert R.gemv_grid(37891) == 1024 and R.iterations(37891, "none") == 3            # no divisor: 1024
    assert R.gemv_grid(152064) == R.gemv_grid(152063) == 1024                         # the cap
    assert R.iterations(152064, "argmax") == 10 and 152063 % 4 == 3
    assert R.gemv_grid(9001) == 563 and R.iterations(9001, "none") == 1               # one iteration per wave
    for fmt in R.FORMATS:                                                             # every branch of the K loops is taken
        roles = [R.chunk_roles(k // R.EPC[fmt], 1, True)[1] for k in R.k_ladder(fmt)]
        assert any(bool((r == 2).all()) for r in roles) and any(bool((r == 1).any() and (r == 2).any()) for r in roles), fmt
        assert any(len(r) == 192 and bool((r == 2).sum() == 64) for r in roles), fmt   # paired, then a tail chunk for every lane


@pytest.mark.parametrize("case", R.BATCHED_CASES, ids=lambda c: c.id)
def test_gemv_batched_inputs_are_discriminating(case):
    ref = case.build().reference()
    if case.exact or case.family == "wide-gate":
        load = case.load()
        assert float(load.max()) < 2.0 ** 23, (case.id, float(load.max()))
    if case.exact and case.epi == "none":
        frac = float(R.representable(ref, case.dtype).double().mean())
        print(f"{case.id}: {100 * frac:.2f} % of the outputs are {case.dtype} values")
        assert frac >= 0.90, (case.id, frac)
    if case.family == "wide-gate":
        lo, hi = case.gate_span()
        assert lo <= -12 and hi >= 12, (case.id, lo, hi)
    if case.epi == "argmax":
        places = set()
        for b in range(case.B):
            top = ref[b].max()
            assert float(top) > 0 and int(torch.argmax(ref[b])) == min(case.tie_sets[b])
            assert sorted(torch.nonzero(ref[b] == top).flatten().tolist()) == sorted(case.tie_sets[b]), (case.id, b)
            places.add(case.tie_sets[b])
        assert len(places) == case.B                                       # a different place for each env
        return                                                            # (a scaled or dropped share of K keeps a planted tie: the
                                                                          # K loop of this kernel is pinned by the cases above)
    report = {}
    refb = ref.to(case.dtype) if case.exact else None
    for m in case.mutants():
        mut = case.reference(m)
        report[m] = int((mut.to(case.dtype) != refb).any(1).sum()) if case.exact else float(((mut - ref).abs() / R.bound(ref, case.dtype)).max())
    _check(case, report)
