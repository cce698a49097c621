"""The forced-turn head at op level (svln_generate_forced): the EPI_TARGET siblings of gemv_batched_kernel and of the MFMA arg-max
epilogue with target_final_batched_kernel, through the test-only entries svln_op_gemv_batched_target / svln_op_gemm_target on the exact
cases of tests/forced_ref.py (tests/test_forced_inputs.py proves them sharp on the CPU), in fp32 and bf16.

Every case asserts: greedy ids == the designed winners; |logprob - float64| <= 2e-5 and |greedy_logprob - float64| <= 2e-5
(forced_ref.TOL, the project's bound for these sums); the 32 capture slots hold the exact y of each named column and the canary
everywhere else (behind a -1 target, in the pad rows at and beyond M); a row whose target is its arg-max has the same bits in both scores;
and with inv_t = 1 the ids, greedy_logprobs and the three partial arrays are bit-equal to the svln_op_*_argmax_scores entry on the same
inputs."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import forced_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
_engines = {}
WORST = {}
PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _partials(m, rows, n):
    val, idx, s = np.zeros((rows, n), np.float32), np.zeros((rows, n), np.int32), np.zeros((rows, n), np.float32)
    _lib.check(m._lib.svln_op_read_argmax_partials(m._h, rows, n, val.ctypes.data_as(PF), idx.ctypes.data_as(PI), s.ctypes.data_as(PF)))
    return val.view(np.uint32), idx, s.view(np.uint32)


def _run(case):
    m = engine(case.dtype)
    dt = case.dtype
    x, W = case.operands()
    L, tgt = case.logits()
    pad = 16 if case.kind == "gemv" else 0
    xp = torch.full((case.B, case.K + pad), 3.0e4, dtype=torch.float64)
    xp[:, :case.K] = x
    dx, dW = xp.to(dt).cuda(), W.to(dt).cuda()
    torch.cuda.synchronize()
    B, N, K = case.B, case.N, case.K
    n_part = min((N + 3) // 4, 2048) if case.kind == "gemv" else (N + 127) // 128
    tg = (C.c_int32 * 32)(*(tgt + [-1] * (32 - B)))
    toks, glp, lp = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32)), (C.c_float * 32)(*([7.0] * 32))
    slots = np.full(32, R.CANARY, dtype=np.float32)
    if case.kind == "gemv":
        _lib.check(m._lib.svln_op_gemv_batched_target(m._h, ptr(dW), K, ptr(dx), K + pad, N, K, B, tg, case.inv_t, toks, glp, lp, slots.ctypes.data_as(PF)))
    else:
        _lib.check(m._lib.svln_op_gemm_target(m._h, ptr(dx), K, ptr(dW), K, B, N, K, tg, case.inv_t, toks, glp, lp, slots.ctypes.data_as(PF)))
    mine = _partials(m, B, n_part)
    toks, glp, lp = list(toks)[:B], np.asarray(list(glp)[:B], np.float32), np.asarray(list(lp)[:B], np.float32)

    ref_tok, ref_glp, ref_lp = case.reference()
    assert toks == [int(t) for t in ref_tok], (case.id, toks, ref_tok.tolist())
    assert np.array_equal(slots, case.expected_slots()), (case.id, slots, case.expected_slots())
    worst = 0.0
    for b in range(B):
        e = abs(float(glp[b]) - float(ref_glp[b]))
        assert e <= R.TOL, (case.id, b, "greedy", float(glp[b]), float(ref_glp[b]))
        worst = max(worst, e)
        if tgt[b] < 0:
            assert math.isnan(lp[b]), (case.id, b, lp[b])
            continue
        e = abs(float(lp[b]) - float(ref_lp[b]))
        worst = max(worst, e)
        assert e <= R.TOL, (case.id, b, float(lp[b]), float(ref_lp[b]), e)
        if tgt[b] == toks[b]:
            assert lp[b].tobytes() == glp[b].tobytes(), (case.id, b, lp[b], glp[b])
    WORST[case.kind] = max(WORST.get(case.kind, 0.0), worst)
    print(f"{case.id}: worst |logprob - ref| = {worst:.3e}")

    if case.inv_t == 1.0:          # the scored form on the same inputs: same ids, same scores, same partials, bit for bit
        st, sl = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32))
        if case.kind == "gemv":
            _lib.check(m._lib.svln_op_gemv_batched_argmax_scores(m._h, ptr(dW), K, ptr(dx), K + pad, None, 1e-6, N, K, B, None, None, 1.0, st, sl))
        else:
            _lib.check(m._lib.svln_op_gemm_argmax_scores(m._h, ptr(dx), K, ptr(dW), K, B, N, K, None, None, 1.0, st, sl))
        theirs = _partials(m, B, n_part)
        assert list(st)[:B] == toks, (case.id, list(st)[:B], toks)
        assert np.asarray(list(sl)[:B], np.float32).tobytes() == glp.tobytes(), (case.id, list(sl)[:B], glp)
        for a, b_, what in zip(mine, theirs, ("part_val", "part_idx", "part_sum")):
            assert np.array_equal(a, b_), (case.id, what)


@pytest.mark.parametrize("case", R.gemv_cases(), ids=lambda c: c.id)
def test_gemv_batched_target(case):
    _run(case)


@pytest.mark.parametrize("case", R.mfma_cases(), ids=lambda c: c.id)
def test_gemm_target(case):
    _run(case)


def test_nan_and_inf_target_logits():
    """a -inf target logit gives -inf, a NaN target logit NaN (and a NaN row), a row without a target NaN: none is an error"""
    m = engine(torch.float32)
    K, N, B = 96, 9, 2
    x = torch.zeros((B, K), dtype=torch.float32)
    x[:, 0] = 1.0
    W = torch.zeros((N, K), dtype=torch.float32)
    W[4, 0] = 2.0
    W[7, 0] = float("-inf")
    dW, dx = W.cuda(), x.cuda()
    torch.cuda.synchronize()
    toks, glp, lp = (C.c_int32 * 2)(), (C.c_float * 2)(), (C.c_float * 2)()

    def call(t0, t1):
        _lib.check(m._lib.svln_op_gemv_batched_target(m._h, ptr(dW), K, ptr(dx), K, N, K, B, (C.c_int32 * 2)(t0, t1), 1.0, toks, glp, lp, None))
        return list(toks), list(glp), list(lp)

    t, g, l = call(7, -1)
    assert t == [4, 4] and l[0] == float("-inf") and math.isnan(l[1]) and math.isfinite(g[0]) and g[0] == g[1]
    t, g, l = call(4, 0)
    assert l[0] == g[0] and abs(l[1] - (g[1] - 2.0)) <= 1e-6
    dW[7, 0] = float("nan")
    torch.cuda.synchronize()
    t, g, l = call(7, 4)
    assert math.isnan(l[0]) and math.isnan(l[1])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_malformed_calls_are_refused_before_any_launch(dt):
    m = engine(dt)
    epc = 4 if dt == torch.float32 else 8
    K, N, B = 256, 16, 2
    W = torch.zeros((N, K), dtype=dt, device="cuda")
    x = torch.zeros((4, K), dtype=dt, device="cuda")
    tok, g, lp = (C.c_int32 * 32)(), (C.c_float * 32)(), (C.c_float * 32)()
    tg = (C.c_int32 * 32)(*([0] * 32))
    torch.cuda.synchronize()
    Lb = m._lib

    def targets(*v):
        return (C.c_int32 * 32)(*(list(v) + [0] * (32 - len(v))))

    def bat(W=W, ldw=K, x=x, ldx=K, N=N, K=K, B=B, tg=tg, it=1.0, tok=tok, g=g, lp=lp):
        return Lb.svln_op_gemv_batched_target(m._h, ptr(W), ldw, ptr(x), ldx, N, K, B, tg, it, tok, g, lp, None)

    assert bat() == 0 and bat(B=4) == 0 and bat(tg=targets(-1, N - 1)) == 0
    assert bat(W=None) != 0 and bat(x=None) != 0 and bat(tok=None) != 0 and bat(g=None) != 0 and bat(lp=None) != 0 and bat(tg=None) != 0
    assert bat(B=1) != 0 and bat(B=3) != 0 and bat(B=0) != 0 and bat(B=16) != 0
    assert bat(N=0) != 0 and bat(K=K - epc // 2) != 0 and bat(ldw=K - epc) != 0 and bat(ldx=K - epc) != 0
    assert bat(tg=targets(0, N)) != 0 and bat(tg=targets(-2, 0)) != 0
    assert bat(it=0.0) != 0 and bat(it=-1.0) != 0 and bat(it=float("inf")) != 0 and bat(it=float("nan")) != 0

    def mfma(A=x, lda=K, W=W, ldw=K, M=4, N=N, K=K, tg=tg, it=1.0, tok=tok, g=g, lp=lp):
        return Lb.svln_op_gemm_target(m._h, ptr(A), lda, ptr(W), ldw, M, N, K, tg, it, tok, g, lp, None)

    assert mfma() == 0 and mfma(M=1) == 0 and mfma(tg=targets(-1, N - 1, 0, 0)) == 0
    assert mfma(A=None) != 0 and mfma(W=None) != 0 and mfma(tok=None) != 0 and mfma(g=None) != 0 and mfma(lp=None) != 0 and mfma(tg=None) != 0
    assert mfma(M=0) != 0 and mfma(M=33) != 0 and mfma(N=0) != 0 and mfma(N=128 * 2048 + 1) != 0
    assert mfma(K=K - epc // 2) != 0 and mfma(lda=K - epc) != 0 and mfma(ldw=K - epc) != 0 and mfma(A=x.view(-1)[epc // 2:]) != 0
    assert mfma(tg=targets(0, 0, 0, N)) != 0 and mfma(tg=targets(-2, 0, 0, 0)) != 0 and mfma(it=0.0) != 0 and mfma(it=float("nan")) != 0


def test_zz_worst_error_report():
    """prints the worst op-level error of this run per kernel shape (the README records it); the bound itself is asserted per case"""
    for kind, w in sorted(WORST.items()):
        print(f"worst |logprob - float64 reference| over the {kind} cases: {w:.3e}")
        assert w <= R.TOL
