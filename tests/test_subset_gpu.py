"""The allowed-token lm_head at op level (svln_set_allowed_tokens; gemv_subset.hip) through the test-only entry svln_op_subset_argmax, on
the exact cases of tests/subset_ref.py (tests/test_subset_inputs.py proves them sharp and that every case keeps its top-2 margin: no
case is skipped here), on the bf16 and the fp32 engine.

Cases: the returned y is BIT-EQUAL to the exact reference, the tokens equal the restatement's (= the float64 reference's),
|logprob - float64| <= 2e-5 and |allowed_logprobs - float64| <= 2e-5 (subset_ref.TOL, the bound of tests/test_scores_gpu.py for the same
merge), and the distribution's entry at the emitted id agrees with the score inside twice that bound.  Rows of W outside the list and
the ldw / ldx padding are NaN.
Invariance: on random (inexact) operands the value of a (weight row, activation row) pair is bit-equal for every B and for lists that
hold the id at different positions."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import subset_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
_engines = {}
WORST = {}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _i32(v):
    return (C.c_int32 * len(v))(*[int(q) for q in v])


def subset_op(m, dW, ldw, dx, ldx, V, K, B, ids, flags=None, pen_rows=None, pen=1.0, T=0.0, seed=0, streams=None, draws=None, rc_only=False,
              n=None):
    """svln_op_subset_argmax -> (tokens [B], logprobs [B], y [B][n], dist [B][n]); rc_only: the return code of a (malformed) call"""
    n = len(ids) if n is None else n
    ids_a = None if ids is None else np.ascontiguousarray(np.asarray(ids, dtype=np.int64))
    toks, lps = np.full(32, -7, dtype=np.int32), np.full(32, 123.0, dtype=np.float32)
    y, dist = np.full(32 * 256, 123.0, dtype=np.float32), np.full(32 * 256, 123.0, dtype=np.float32)
    pf = C.POINTER(C.c_float)
    rc = m._lib.svln_op_subset_argmax(m._h, ptr(dW), ldw, ptr(dx), ldx, V, K, B, None if ids_a is None else ids_a.ctypes.data_as(C.POINTER(C.c_int64)),
                                      n, ptr(flags), None if pen_rows is None else C.cast(ptr(pen_rows), C.POINTER(C.c_int32)), pen, T, seed,
                                      None if streams is None else _i32(streams), None if draws is None else _i32(draws),
                                      toks.ctypes.data_as(C.POINTER(C.c_int32)), lps.ctypes.data_as(pf), y.ctypes.data_as(pf), dist.ctypes.data_as(pf))
    if rc_only:
        return rc, (toks, lps, y, dist)
    _lib.check(rc)
    return list(toks[:B]), list(lps[:B]), y[: B * n].reshape(B, n), dist[: B * n].reshape(B, n)


def _run_case(case):
    dt = DT[case.fmt]
    m = engine(dt)
    W, x = case.operands()
    dW, dx = torch.from_numpy(W).to(dt).cuda(), torch.from_numpy(x).to(dt).cuda()
    _, flags = case.logits()
    df = None if flags is None else torch.from_numpy(flags).cuda()
    dr = None if flags is None else torch.tensor(case.pen_rows(), dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    return subset_op(m, dW, case.ldw, dx, case.ldx, R.V, case.K, case.B, case.ids(), df, dr, R.PEN if case.pen else 1.0, case.T, case.seed,
                     case.streams, case.draws)


@pytest.mark.parametrize("case", R.all_cases(), ids=lambda c: c.id)
def test_subset_case(case):
    toks, lps, y, dist = _run_case(case)
    rtoks, rscores, ry, rdist, _ = case.reference()
    assert np.array_equal(y.astype(np.float64), ry), (case.id, "y is not bit-equal to the exact reference")
    assert toks == case.restate()[0] == rtoks, (case.id, toks, rtoks)
    worst = 0.0
    for b in range(case.B):
        if rtoks[b] < 0:
            assert math.isnan(lps[b]), (case.id, b, lps[b])
            continue
        e = abs(float(lps[b]) - rscores[b])
        j = int(np.flatnonzero(case.ids() == toks[b])[0])
        worst = max(worst, e)
        assert e <= R.TOL, (case.id, b, lps[b], rscores[b])
        assert abs(float(dist[b, j]) - float(lps[b])) <= 2 * R.TOL, (case.id, b, dist[b, j], lps[b])
    with np.errstate(all="ignore"):
        d = np.abs(dist.astype(np.float64) - rdist)
    d = np.where((dist == rdist) | (np.isnan(dist) & np.isnan(rdist)), 0.0, d)          # (-inf entries and all--inf rows agree exactly)
    dw = float(np.nan_to_num(d, nan=np.inf).max())
    WORST["logprob"] = max(WORST.get("logprob", 0.0), worst)
    WORST["allowed_logprobs"] = max(WORST.get("allowed_logprobs", 0.0), dw)
    print(f"{case.id}: worst |logprob - ref| = {worst:.3e}, worst |allowed_logprobs - ref| = {dw:.3e}")
    assert dw <= R.TOL, (case.id, dw)


@pytest.mark.parametrize("fmt", ["fp32", "bf16"])
def test_pair_value_is_bit_equal_across_batch_sizes_and_list_positions(fmt):
    """random operands at the true width, where the summation order shows in the last bits: the value of (weight row a, activation row r)
    must not depend on B, on where r sits in the batch, on the list, or on a's place in it"""
    dt = DT[fmt]
    m = engine(dt)
    K, V, ldw, ldx = 3584, 1024, 3584 + 8, 3584 + 16
    g = torch.Generator().manual_seed(5)
    W = torch.full((V, ldw), float("nan"))
    x = torch.full((32, ldx), float("nan"))
    W[:, :K] = torch.randn((V, K), generator=g)
    x[:, :K] = torch.randn((32, K), generator=g)
    dW, dx = W.to(dt).cuda(), x.to(dt).cuda()
    torch.cuda.synchronize()
    a = [3, 500, 1023]
    wide = sorted(set(range(1, 1020, 4)) | set(a))[:255] + [1023]                                        # n = 256, the three ids far apart in it
    lists = [a, [0, 1, 2] + a, [3, 4, 5, 6, 7, 500, 777, 1023], sorted(set(wide))]
    assert all(set(a) <= set(l) and len(l) <= 256 for l in lists)
    base = None
    for ids in lists:
        pos = [ids.index(q) for q in a]
        for B in (1, 2, 3, 8, 32):
            _, _, y, _ = subset_op(m, dW, ldw, dx, ldx, V, K, B, ids)
            assert np.isfinite(y).all()
            got = y[:, pos].view(np.uint32)
            if base is None:
                assert B == 1
                full = subset_op(m, dW, ldw, dx, ldx, V, K, 32, ids)[2][:, pos].view(np.uint32)
                base = full
            assert np.array_equal(got, base[:B]), (fmt, len(ids), B)
    # a row's value does not depend on its place in the batch either: rows 5 .. 7 alone
    y = subset_op(m, dW, ldw, dx[5:8], ldx, V, K, 3, lists[1])[2][:, [lists[1].index(q) for q in a]].view(np.uint32)
    assert np.array_equal(y, base[5:8])
    # and it is the dot product of that pair: against float64, far inside what any other (weight row, activation row) pair would give
    ref = (x[:, :K].to(dt).double() @ W[a, :K].to(dt).double().T).numpy()
    assert np.abs(base.view(np.float32).astype(np.float64) - ref).max() <= 2e-3 * np.abs(ref).max() + 1e-2


@pytest.mark.parametrize("fmt", ["fp32", "bf16"])
def test_rows_without_a_finite_allowed_value(fmt):
    """a NaN entry among finite ones never wins and makes the row's score and distribution NaN; a row whose allowed entries are all NaN,
    or all -inf, gives token -1 and a NaN score; a -inf entry never wins and adds nothing to the sums"""
    dt = DT[fmt]
    m = engine(dt)
    K, V = 64, 1024
    ids = [0, 9, 511, 1023]
    vals = (1.0, 3.0, 2.0, -1.0)
    W = torch.full((V, K), float("nan"))
    W[ids] = 0.0
    W[ids, 0] = torch.tensor(vals)
    x = torch.zeros((2, K))
    x[0, 0], x[1, 0] = 1.0, 2.0
    dx = x.to(dt).cuda()

    def run(Wh, xd=dx, B=2):
        dW = Wh.to(dt).cuda()
        torch.cuda.synchronize()
        return subset_op(m, dW, K, xd, K, V, K, B, ids)

    toks, lps, y, dist = run(W)
    assert toks == [9, 9] and np.array_equal(y, np.array([vals, [2 * v for v in vals]], dtype=np.float32))
    assert abs(lps[0] - (3.0 - math.log(sum(math.exp(v) for v in vals)))) <= R.TOL
    Wn = W.clone()
    Wn[9, 4] = float("nan")                # NaN * 0 = NaN: id 9 is NaN for both rows
    toks, lps, y, dist = run(Wn)
    assert toks == [511, 511] and all(math.isnan(v) for v in lps) and np.isnan(dist).all() and np.isnan(y[:, 1]).all()
    toks, lps, y, dist = run(torch.full((V, K), float("nan")))
    assert toks == [-1, -1] and all(math.isnan(v) for v in lps) and np.isnan(dist).all()
    Wi = W.clone()
    Wi[ids, 5] = float("-inf")
    one = torch.zeros((1, K))
    one[0, 5] = 1.0
    d1 = one.to(dt).cuda()
    toks, lps, y, dist = run(Wi, d1, 1)
    assert toks == [-1] and math.isnan(lps[0]) and (y == -np.inf).all()
    Wi[511, 5] = 0.5
    toks, lps, y, dist = run(Wi, d1, 1)
    assert toks == [511] and abs(lps[0]) <= 1e-6 and dist[0, 2] == lps[0] and (np.delete(dist[0], 2) == -np.inf).all()


@pytest.mark.parametrize("fmt", ["fp32", "bf16"])
def test_malformed_calls_are_refused_before_any_launch(fmt):
    dt = DT[fmt]
    m = engine(dt)
    epc = R.EPC[fmt]
    K, V, B = 256, 64, 2
    W = torch.zeros((V, K), dtype=dt, device="cuda")
    x = torch.zeros((B, K), dtype=dt, device="cuda")
    fl = torch.zeros((B, V), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ids = [1, 5, 63]

    def call(W=W, x=x, ldw=K, ldx=K, V=V, K=K, B=B, ids=ids, n=None, T=0.0, streams=(0, 1), draws=(0, 0), flags=None, pen=1.0):
        rc, outs = subset_op(m, W, ldw, x, ldx, V, K, B, ids, flags, None, pen, T, 7, streams, draws, rc_only=True, n=n)
        if rc != 0:         # refused before any launch: nothing was written
            assert all((o == (-7 if o.dtype == np.int32 else 123.0)).all() for o in outs)
        return rc

    assert call() == 0 and call(T=1.0) == 0 and call(flags=fl, pen=2.0) == 0
    assert call(B=0) != 0 and call(B=33) != 0 and b"B" in m._lib.svln_last_error()
    assert call(K=K - epc // 2) != 0 and call(K=0) != 0
    assert call(ldw=K - epc) != 0 and call(ldx=K - epc) != 0
    assert call(W=None) != 0 and call(x=None) != 0
    assert call(ids=[1, 5, 64]) != 0 and b"vocabulary" in m._lib.svln_last_error()
    assert call(ids=[-1, 5]) != 0
    assert call(ids=[5, 5]) != 0 and b"ascending" in m._lib.svln_last_error()
    assert call(ids=[5, 1]) != 0
    assert call(ids=[], n=0) != 0 and call(ids=None, n=3) != 0
    assert call(V=1024, ids=list(range(257))) != 0 and b"256" in m._lib.svln_last_error()
    assert call(T=-1.0) != 0 and call(T=float("nan")) != 0 and call(T=float("inf")) != 0
    assert call(T=1.0, streams=None) != 0 and call(T=1.0, draws=(0, -1)) != 0
    assert call(flags=fl, pen=0.0) != 0


def test_zz_worst_error_report():
    """prints the worst errors of this run (the README records them); the bounds themselves are asserted per case"""
    for kind, w in sorted(WORST.items()):
        print(f"worst error, {kind}: {w:.3e}")
        assert w <= R.TOL
