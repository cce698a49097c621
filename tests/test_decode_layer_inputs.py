"""CPU proof that the inputs of tests/test_decode_layer_gpu.py are sharp (tests/decode_layer_ref.py): every case is a shape the kernel
admits and hits what the case list promises; the exact family's expected values are values of the engine type; and every listed
kernel mistake moves a checked value -- bit-wise at the exact stages, by >= 10x the bound at the toleranced ones."""
import ctypes as C
import math

import pytest
import torch

import decode_layer_ref as R
from streamvln_amd import _lib

MUTANT_FACTOR = 10.0


def supported(dtype, H, I, qd, qkv_dim, cus):
    ok = C.c_int32(-1)
    _lib.check(_lib.load().svln_decode_layer_supported(R.DT_CODE[dtype], H, I, qd, qkv_dim, cus, C.byref(ok)))
    return bool(ok.value)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_case_is_supported_and_keeps_its_promises(case):
    assert supported(case.dtype, case.H, case.I, case.qd, case.qkv_dim, case.G)
    per, ops, pr = case.per(), case.ops(), case.promises
    assert per["A"] % case.vpg() == 0 and per["H"] % case.vpg() == 0 and per["I"] % case.vpg() == 0
    for k, v in pr.get("per", {}).items():
        assert per[k] == v, (k, per)
    for k, v in pr.get("bpr", {}).items():
        assert case.bpr(ops[k][0]) == v, (k, v)
    dealt = {k: [R.dealt(case.bpr(K), n, w) for w in range(R.NW)] for k, (K, n, _) in ops.items()}
    for k, v in pr.get("slots", {}).items():
        assert [R.slots(len(d)) for d in dealt[k]] == v, (k, v)
    for k, v in pr.get("padding", {}).items():
        assert sum(R.slots(len(d)) - len(d) for d in dealt[k]) == v, (k, v)
    if pr.get("idle_waves"):
        assert all(any(len(d) == 0 for d in dealt[k]) for k in ("o", "down", "qkv")) and 2 <= per["H"] <= 4 and 2 <= per["I"] <= 4
    if pr.get("straddle"):
        two = [(c * per["A"]) >> 7 != (c * per["A"] + per["A"] - 1) >> 7 for c in range(case.G)]
        assert any(two) and not all(two) and 128 % per["A"] != 0
    if "live" in pr:
        assert case.live == pr["live"]
    assert case.live >= 1 and case.masked_split < case.live and case.live <= case.nsplit


def test_case_list_covers_the_issue():
    ids = {(c.name, c.dtype) for c in R.CASES}
    bf, f32 = torch.bfloat16, torch.float32
    for need in (("tiny256", bf), ("tiny256", f32), ("caps", bf), ("caps", f32), ("rowmode15", bf), ("blockmode16", bf), ("rowmode15", f32),
                 ("blockmode16", f32), ("blockmode19", bf), ("hlimit", f32), ("straddle", bf), ("last", bf), ("last", f32), ("nobias", bf)):
        assert need in ids, need
    assert {c.live for c in R.CASES if c.name.startswith("splits")} == {1, 2, 4}
    assert {c.kv_len for c in R.CASES if c.name == "splits"} == {1, 64, 65, 64 * 4}
    assert any(c.live < c.nsplit for c in R.CASES) and {c.stale for c in R.CASES} == {True, False}
    assert {c.family for c in R.CASES} == {"exact", "eps", "outlier"}
    # one step past the H limit is refused: fp32 rows of 4096 values are 16 blocks, and [gate | up] pairs are dealt as whole rows
    assert not supported(f32, 4096, 1024, 256, 512, 256) and supported(f32, 3840, 1024, 256, 512, 256)
    # ... and so is everything past a per-workgroup cap, or a ragged share
    assert not supported(bf, 512, 1024, 512, 1024, 4) and not supported(bf, 512, 1024, 512, 1024, 7)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_expected_values_and_mutants(case):
    ref = case.reference()
    for st, v in ref.items():
        assert v is None or bool(torch.isfinite(v).all()), st
    if case.exact:
        # the merged output and x1 are values of the engine type before the final rounding (>= 90 %: the condition gemv_ref's exact cases
        # keep); x2 is built on the kernel's own edge 2, arbitrary T values: decode_layer_ref's docstring says why it is still exact
        a = _unrounded_merge(case)
        x1 = case.o_w @ ref["attn"] + case.x
        for name, v in (("attn", a), ("x1", x1)):
            frac = float(R.GR.representable(v, case.dtype).double().mean())
            assert frac >= 0.9, (name, frac)
        assert float((ref["attn"] != 0).double().mean()) > 0.5 and float((ref["x1"] != 0).double().mean()) > 0.5
    rep = R.mutant_report(case)
    assert set(rep) == set(case.mutants())
    for m, dev in rep.items():
        if case.exact_stage(case.mutants()[m]):
            assert dev > 0, (m, "no expected value moves")
        else:
            assert dev >= MUTANT_FACTOR, (m, dev)


def _unrounded_merge(case):
    keep, case.rt = case.rt, lambda t: t
    try:
        return case.merge()
    finally:
        case.rt = keep


def test_every_listed_mistake_is_caught_somewhere():
    seen = set()
    for c in R.CASES:
        seen |= set(c.mutants())
    assert seen == set(R.ALL_MUTANTS), set(R.ALL_MUTANTS) - seen
    # the dealing mistakes on both dealing modes of down_proj
    for m in ("drop_last_block", "padding_added", "partials_swapped"):
        modes = {c.bpr(c.I) > R.ROWMODE_MAX_BPR for c in R.CASES if m in c.mutants()}
        assert modes == {True, False}, m


def test_granule_prefill_is_poison():
    for case in R.CASES[:8]:
        for e in range(4):
            tags, vals = case.unpack(case.granule_prefill(e))
            assert bool(torch.isnan(vals).all())
            assert bool((tags == ((case.seq0 - 1) * 4 + e + 1 if case.stale else 0)).all())
            assert bool((tags != case.seq0 * 4 + e + 1).all())
    assert math.isnan(float(R._bits_to_f32(torch.tensor([0x7FC00000]))[0]))
