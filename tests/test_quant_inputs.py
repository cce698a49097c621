"""CPU proof that the inputs of tests/test_quant_gpu.py are sharp, and that the e4m3 encoder they are judged by is right.

  encoder   tests/quant_ref.py e4m3_encode (integer bit arithmetic) against torch.float8_e4m3fn (the encoder of the oracle's fp8 modes)
            on every bf16 bit pattern, its round trip through the decode table, and the parity of every tie.
  mutants   every mistake listed in quant_ref.MUTANTS changes a byte (after the fold) or a scale bit on every case written for it.
  coverage  the cases reach every code in both signs and hit every midpoint exactly.
  scheme    the properties of the scale floor and of the NaN rule, and the floor's threshold over all bf16 row maxima.
Each test prints what it counted (pytest -s, or on failure)."""
import numpy as np
import pytest
import torch

import quant_ref as R
from oracle import streamvln_oracle as O
from test_ops_gpu import _quant_ref

F32 = np.float32
BY_ID = {c.id: c for c in R.CASES}


def _torch_bytes(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def _all_bf16():
    return (np.arange(1 << 16, dtype=np.uint32) << 16).view(np.float32)


def test_encoder_equals_torch_on_every_bf16_pattern_and_on_the_tie_rows():
    v = _all_bf16()
    fin = np.isfinite(v)
    x = np.clip(v[fin], -448.0, 448.0).astype(np.float32)
    assert np.array_equal(R.e4m3_encode(x), _torch_bytes(x))                                  # signs included: no fold
    assert np.array_equal(R.fold(R.e4m3_encode(v[~fin & np.isnan(v)])), np.full(int(np.isnan(v).sum()), 0x7F, dtype=np.uint8))
    assert np.array_equal(R.fold(_torch_bytes(v[np.isnan(v)])), np.full(int(np.isnan(v).sum()), 0x7F, dtype=np.uint8))
    ties = R.scaled(BY_ID["ties"].W)
    assert np.isfinite(ties).all() and np.array_equal(R.e4m3_encode(ties), _torch_bytes(ties))
    # unclamped: both give the NaN byte from the first value that rounds above 448 on (the midpoint 464 still ties down to 448)
    big = np.array([464.0, 465.0, 480.0, 512.0, 1e30, np.inf], dtype=np.float32)
    assert R.e4m3_encode(big).tolist() == _torch_bytes(big).tolist() == [0x7E, 0x7F, 0x7F, 0x7F, 0x7F, 0x7F]
    # fp32 inputs that no bf16 value reaches: the sticky bits below bf16's 8 decide
    g = np.random.default_rng(5)
    r = (g.standard_normal(200000) * np.exp2(g.integers(-12, 9, 200000))).astype(np.float32)
    r = np.concatenate([np.clip(r, -448, 448), np.nextafter(R.MIDS.astype(np.float32), F32(0)), np.nextafter(R.MIDS.astype(np.float32), F32(1e9))])
    assert np.array_equal(R.e4m3_encode(r), _torch_bytes(r))


def test_round_trip_of_the_254_finite_codes():
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)
    assert len(codes) == 254
    v = R.e4m3_decode(codes)
    assert np.isfinite(v).all() and np.array_equal(R.e4m3_encode(v), codes)
    assert np.isnan(R.e4m3_decode(np.array([0x7F, 0xFF], dtype=np.uint8))).all()
    assert float(v.max()) == 448.0 and float(np.abs(v[v != 0]).min()) == 2.0 ** -9
    assert np.array_equal(v[:127].astype(np.float32), torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy())


def test_every_tie_goes_to_the_even_code():
    mids = R.MIDS.astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), R.MIDS) and len(mids) == 126
    for sign in (1.0, -1.0):
        got = R.e4m3_encode(F32(sign) * mids) & 0x7F
        lo = np.arange(126)
        exp = np.where(lo % 2 == 0, lo, lo + 1)                      # the midpoint of codes j, j + 1 goes to the even one
        assert np.array_equal(got, exp)
    assert np.array_equal(R.e4m3_encode(np.nextafter(mids, F32(0))), np.arange(126))
    assert np.array_equal(R.e4m3_encode(np.nextafter(mids, F32(1e9))), np.arange(1, 127))
    case = BY_ID["ties"]
    x = R.scaled(case.W)
    q, sc = R.quant_rows(case.W)
    assert sc.tolist() == [2.0 ** k for k in R.TIE_K]
    cols = case.info["mid_cols"]
    assert np.array_equal(np.abs(x[:, cols]), np.tile(np.concatenate([mids, mids]), (len(R.TIE_K), 1)))     # every midpoint is hit exactly
    assert not (q[:, cols] & 1).any()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_cases_catch_the_mutants_written_for_them(case):
    ref = R.quant_rows(case.W)
    report = {}
    for m in case.mutants:
        mut = R.quant_rows(case.W, m)
        report[m] = int((R.fold(mut[0]) != R.fold(ref[0])).sum()) + int((mut[1].view(np.uint32) != ref[1].view(np.uint32)).sum())
    print(f"{case.id} {tuple(case.W.shape)}: " + ", ".join(f"{k} {v}" for k, v in report.items()))
    assert all(v > 0 for v in report.values()), f"{case.id}: mutants the case cannot see: {[k for k, v in report.items() if v == 0]}"


def test_every_mutant_is_caught_somewhere():
    named = {m for c in R.CASES for m in c.mutants}
    assert named == set(R.MUTANTS), set(R.MUTANTS) ^ named
    for m in R.MUTANTS:
        assert any(not R.same(R.quant_rows(c.W, m), R.quant_rows(c.W)) for c in R.CASES), m


def test_placements_are_where_their_names_say():
    for cols in R.PLACE_COLS:
        case = BY_ID[f"placement-{cols}"]
        a = case.W.abs().numpy()
        scales = R.quant_rows(case.W)[1]
        assert all(scales[r] != scales[r - 1] for r in range(1, len(scales))), cols          # neighbouring rows differ in scale
        for r, (what, col, sign) in enumerate(case.info["spots"]):
            assert int(a[r].argmax()) == col and float(case.W[r, col]) * sign > 0 and (a[r] == a[r, col]).sum() == 1, (cols, what)
            chunk = col // 8
            if what.startswith("wave"):
                assert (chunk % R.BLOCK) // 64 == int(what[-1]) and chunk < R.BLOCK, (cols, what)
            if what == "iter2":
                assert R.BLOCK <= chunk < 2 * R.BLOCK
            if what == "iter3":
                assert chunk >= 2 * R.BLOCK
            if what == "negative":
                assert float(case.W[r].max()) < 32 * float(a[r, col]) / 448
    assert {w for w, _, _ in BY_ID["placement-2064"].info["spots"]} >= {"first", "last", "wave0", "wave1", "wave2", "wave3", "iter2", "negative"}
    assert [cols // 8 for cols in R.PLACE_COLS] == [2, 6, 66, 258, 514]


def test_cases_reach_every_code_in_both_signs_and_all_scale_classes():
    seen = set()
    for c in R.CASES:
        seen |= set(np.unique(R.quant_rows(c.W)[0]).tolist())
    missing = [hex(b) for b in list(range(0x01, 0x7F)) + list(range(0x81, 0xFF)) if b not in seen]
    assert not missing, missing
    picks = BY_ID["scales"].info["amax"]
    assert all(R.amax_class(a) == k for k, v in picks.items() for a in v) and sorted(picks) == [-1, 0, 1]
    # the measured aside of the scheme: the product amax * (1 / (amax / 448)) lands on, below or above 448 and encodes to 0x7E all the same
    v = _all_bf16()
    pos = v[(v > 0) & np.isfinite(v) & (v >= 448 * 2.0 ** -126)]
    p = pos * (F32(1) / (pos / F32(448)))
    assert float(p.min()) > 447.9999 and set(R.e4m3_encode(np.clip(p, -448, 448)).tolist()) == {0x7E}


def test_scheme_finite_rows_give_no_nan_byte_and_zeros_give_byte_zero():
    for c in R.CASES:
        q, sc = R.quant_rows(c.W)
        w = c.W.numpy()
        assert np.isfinite(sc[np.isfinite(w).all(1)]).all() and (sc >= R.FLOOR).all(), c.id
        fin_rows = np.isfinite(w).all(1)
        assert not (R.fold(q[fin_rows]) == 0x7F).any(), c.id
        assert (R.fold(q)[(w == 0) & fin_rows[:, None]] == 0).all(), c.id
    # every positive finite bf16 amax over a row of zeros, +-amax and +-amax / 2: no NaN byte, zeros stay 0, amax is 0x7E above the floor
    v = _all_bf16()
    amax = v[(v > 0) & np.isfinite(v)]
    assert len(amax) == 32639
    W = np.zeros((len(amax), 16), dtype=np.float32)
    W[:, 1], W[:, 6], W[:, 8], W[:, 15] = amax, -amax, amax / 2, -amax / 2
    q, sc = R.quant_rows(W)
    assert not (R.fold(q) == 0x7F).any() and (q[:, [0, 2, 7, 14]] == 0).all()
    above = amax >= F32(448 * 2.0 ** -126)
    assert (q[above, 1] == 0x7E).all() and (q[above, 6] == 0xFE).all() and (q[above, 8] == 0x76).all()
    # the floor touches no row at or above the threshold: same bits with and without it; below it the unfloored scheme is what breaks
    q0, sc0 = R.quant_rows(W, "no_floor")
    assert np.array_equal(q[above], q0[above]) and np.array_equal(sc[above].view(np.uint32), sc0[above].view(np.uint32))
    broken = (R.fold(q0) == 0x7F).any(1)
    print(f"{int((~above).sum())} bf16 maxima lie below 448 * 2^-126; without the floor {int(broken.sum())} of them turn zeros into NaN")
    assert int(broken.sum()) == 992 and not broken[above].any() and float(amax[broken].max()) < 1.3167e-36
    assert (sc[~above] == R.FLOOR).all() and (sc[above] > R.FLOOR).sum() == above.sum() - 1


def test_scheme_a_nan_element_changes_nothing_but_its_own_byte():
    for what in ("nan", "inf"):
        c = BY_ID[what]
        q, sc = R.quant_rows(c.W)
        qt, sct = R.quant_rows(c.info["twin"])
        hit = np.zeros(q.shape, dtype=bool)
        for r, col in c.info["spots"]:
            hit[r, col] = True
        assert (R.fold(q)[hit] == 0x7F).all(), what
        if what == "nan":
            assert np.array_equal(sc.view(np.uint32), sct.view(np.uint32)) and np.array_equal(R.fold(q)[~hit], R.fold(qt)[~hit])
            mut = R.quant_rows(c.W, "nan_to_448")[0]
            assert (mut[hit] == 0xFE).all()                              # what the clamp written with fmaxf / fminf alone makes of it
        else:
            assert np.isinf(sc).all() and (R.fold(q)[~hit] == 0).all()
    edges = BY_ID["edges"]
    q, sc = R.quant_rows(edges.W)
    assert sc[:2].tolist() == [1.0, 1.0] and not R.fold(q[:2]).any()
    q0 = R.quant_rows(edges.W, "no_floor")[0]
    for r in edges.info["tiny"]:                                        # the rows whose zeros the unfloored scheme turns into NaN
        assert (R.fold(q0[r])[edges.W[r].numpy() == 0] == 0x7F).all() and not (R.fold(q[r]) == 0x7F).any(), edges.info["names"][r]


def test_the_torch_references_agree_with_the_restatement():
    """_quant_ref of tests/test_ops_gpu.py and oracle.qdq_e4m3_rows (both on torch.float8_e4m3fn) against quant_rows, on every case"""
    for c in R.CASES:
        q, sc = R.quant_rows(c.W)
        qf, scale = _quant_ref(c.W)
        assert np.array_equal(scale.numpy().view(np.uint32), sc.view(np.uint32)), c.id
        assert np.array_equal(R.fold(qf.view(torch.uint8).numpy()), R.fold(q)), c.id
        with np.errstate(all="ignore"):
            deq = (R.e4m3_decode(q) * sc[:, None]).astype(np.float32)
        got = O.qdq_e4m3_rows(c.W).numpy()
        assert np.array_equal(np.isnan(got), np.isnan(deq)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(deq)), c.id
