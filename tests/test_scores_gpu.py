"""Token log-probabilities at op level (svln_set_token_scores): the EPI_ARGMAX_LSE siblings of gemv_rows_kernel (four weight policies),
gemv_batched_kernel and the MFMA arg-max epilogue, each with its final kernel, through the test-only entries svln_op_*_argmax_scores on
the exact cases of tests/scores_ref.py (tests/test_scores_inputs.py proves them sharp on the CPU).

Every case asserts: the tokens of the scored form are bit-equal to those of the plain EPI_ARGMAX call on the same inputs and to the
designed winner (lowest index on a planted tie), and |logprob - float64 reference| <= 2e-5 (scores_ref.TOL)."""
import ctypes as C
import math

import pytest
import torch

import scores_ref as S
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
_engines = {}
WORST = {}


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _check_case(case, plain, scored, lps, ref_tok, ref_lp):
    exp = [int(t) for t in ref_tok]
    assert plain == exp, (case.id, "plain tokens", plain, exp)
    assert scored == plain, (case.id, "scored tokens differ from the plain arg-max", scored, plain)
    errs = [abs(lps[b] - float(ref_lp[b])) for b in range(case.B)]
    worst = max(errs)
    WORST[case.kind] = max(WORST.get(case.kind, 0.0), worst if not math.isnan(worst) else float("inf"))
    print(f"{case.id}: worst |logprob - ref| = {worst:.3e}")
    assert all(e <= S.TOL for e in errs), (case.id, errs, lps, ref_lp.tolist())


def _flag_ops(case):
    _, flags, rows = case.logits()
    if flags is None:
        return None, None
    return flags.cuda(), torch.tensor(rows, dtype=torch.int32).cuda()


@pytest.mark.parametrize("case", S.rows_cases(), ids=lambda c: c.id)
def test_gemv_rows_scores(case):
    dt = case.dtype
    m = engine(dt)
    x, W = case.operands()
    ops = {k: v.cuda() for k, v in S.pack(case.fmt, W).items()}
    dx = x[0].to(dt).cuda()
    flags, rows = _flag_ops(case)
    fr = None if flags is None else flags[int(rows[0])].contiguous()
    torch.cuda.synchronize()

    def call(scored):
        tok, lp = C.c_int32(-7), C.c_float(float("nan"))
        _lib.check(m._lib.svln_op_gemv_argmax_scores(m._h, S.FMT_ID[case.fmt], ptr(ops["W"]), ptr(ops.get("aux")), case.K, ptr(dx), case.N, case.K,
                                                     ptr(fr), S.PEN, C.byref(tok), C.byref(lp) if scored else None))
        return [tok.value], [lp.value]

    plain, _ = call(False)
    scored, lps = call(True)
    _check_case(case, plain, scored, lps, *case.reference())


def _batched_inputs(case, ld_pad):
    dt = case.dtype
    x, W = case.operands()
    g, sc = None, torch.ones(case.B, dtype=torch.float64)
    if case.norm:                                   # g = +-1: g * (g * x) is the designed row, and the row factor is the only inexact step
        gen = torch.Generator().manual_seed(case.seed + 9)
        g = (torch.randint(0, 2, (case.K,), generator=gen) * 2 - 1).double()
        x = x * g
        sc = 1.0 / torch.sqrt((x * x).mean(1) + S.G.EPS)
    xp = torch.full((case.B, case.K + ld_pad), 3.0e4, dtype=torch.float64)
    xp[:, :case.K] = x
    return xp.to(dt).cuda(), W.to(dt).cuda(), (None if g is None else g.to(dt).cuda()), sc


@pytest.mark.parametrize("case", S.batched_cases(), ids=lambda c: c.id)
def test_gemv_batched_scores(case):
    m = engine(case.dtype)
    dx, dW, dg, sc = _batched_inputs(case, 16)
    flags, rows = _flag_ops(case)
    torch.cuda.synchronize()

    def call(scored):
        toks, lps = (C.c_int32 * 8)(*([-7] * 8)), (C.c_float * 8)(*([float("nan")] * 8))
        _lib.check(m._lib.svln_op_gemv_batched_argmax_scores(m._h, ptr(dW), case.K, ptr(dx), case.K + 16, ptr(dg), S.G.EPS, case.N, case.K, case.B,
                                                             ptr(flags), None if rows is None else C.cast(ptr(rows), C.POINTER(C.c_int32)), S.PEN,
                                                             toks, lps if scored else None))
        return list(toks)[:case.B], list(lps)[:case.B]

    plain, _ = call(False)
    scored, lps = call(True)
    _check_case(case, plain, scored, lps, *S.reference(case.processed() * sc[:, None]))


@pytest.mark.parametrize("case", S.mfma_cases(), ids=lambda c: c.id)
def test_gemm_argmax_scores(case):
    m = engine(case.dtype)
    dx, dW, _, _ = _batched_inputs(case, 0)
    flags, rows = _flag_ops(case)
    torch.cuda.synchronize()

    def call(scored):
        toks, lps = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32))
        _lib.check(m._lib.svln_op_gemm_argmax_scores(m._h, ptr(dx), case.K, ptr(dW), case.K, case.B, case.N, case.K, ptr(flags),
                                                     None if rows is None else C.cast(ptr(rows), C.POINTER(C.c_int32)), S.PEN, toks, lps if scored else None))
        return list(toks)[:case.B], list(lps)[:case.B]

    plain, _ = call(False)
    scored, lps = call(True)
    _check_case(case, plain, scored, lps, *case.reference())


def test_nan_logit_and_no_finite_logit():
    """a NaN logit makes the token's score NaN; a row without a finite logit gives token -1 and a NaN score: neither is an error"""
    m = engine(torch.float32)
    K, N = 96, 9
    x = torch.ones(K, dtype=torch.float32)
    W = torch.zeros((N, K), dtype=torch.float32)
    W[4, 0] = 2.0
    W[7, 1] = float("nan")
    tok, lp = C.c_int32(-7), C.c_float(0.0)
    dW, dx = W.cuda(), x.cuda()
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gemv_argmax_scores(m._h, 0, ptr(dW), None, K, ptr(dx), N, K, None, 1.0, C.byref(tok), C.byref(lp)))
    assert tok.value == 4 and math.isnan(lp.value)
    dW = torch.full((N, K), float("nan"), dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gemv_argmax_scores(m._h, 0, ptr(dW), None, K, ptr(dx), N, K, None, 1.0, C.byref(tok), C.byref(lp)))
    assert tok.value == -1 and math.isnan(lp.value)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_malformed_calls_are_refused_before_any_launch(dt):
    m = engine(dt)
    epc = 4 if dt == torch.float32 else 8
    K, N, B = 256, 16, 2
    W = torch.zeros((N, K), dtype=dt, device="cuda")
    x = torch.zeros((B, K), dtype=dt, device="cuda")
    fl = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
    rows = torch.zeros((B,), dtype=torch.int32, device="cuda")
    prow = C.cast(ptr(rows), C.POINTER(C.c_int32))
    tok, lp = (C.c_int32 * 32)(), (C.c_float * 32)()
    torch.cuda.synchronize()
    L = m._lib

    def gemv(fmt=0, W=W, aux=None, ldw=K, x=x, N=N, K=K, fl=None, pen=1.0, tok=tok):
        return L.svln_op_gemv_argmax_scores(m._h, fmt, ptr(W), ptr(aux), ldw, ptr(x), N, K, ptr(fl), pen, tok, lp)

    assert gemv() == 0 and gemv(fl=fl, pen=2.0) == 0
    assert gemv(W=None) != 0 and gemv(x=None) != 0 and gemv(tok=None) != 0 and gemv(fmt=3) != 0 and gemv(fmt=1) != 0 and gemv(fmt=2) != 0
    assert gemv(N=0) != 0 and gemv(K=0) != 0 and gemv(K=K - epc // 2) != 0 and gemv(ldw=K - epc) != 0 and gemv(fl=fl, pen=0.0) != 0
    big = (160 * 1024 // 4 // epc + 1) * epc
    assert gemv(K=big, ldw=big) != 0
    if dt == torch.float32:
        assert gemv(fmt=1, aux=x) != 0 and b"bf16" in L.svln_last_error()

    def bat(W=W, ldw=K, x=x, ldx=K, N=N, K=K, B=B, fl=None, rows=None, pen=1.0, tok=tok):
        return L.svln_op_gemv_batched_argmax_scores(m._h, ptr(W), ldw, ptr(x), ldx, None, 1e-6, N, K, B, ptr(fl), rows, pen, tok, lp)

    assert bat() == 0 and bat(fl=fl, rows=prow, pen=2.0) == 0
    assert bat(W=None) != 0 and bat(x=None) != 0 and bat(tok=None) != 0 and bat(B=3) != 0 and bat(B=0) != 0 and bat(B=16) != 0
    assert bat(N=0) != 0 and bat(K=K - epc // 2) != 0 and bat(ldw=K - epc) != 0 and bat(ldx=K - epc) != 0
    assert bat(fl=fl) != 0 and bat(fl=fl, rows=prow, pen=-1.0) != 0

    def mfma(A=x, lda=K, W=W, ldw=K, M=B, N=N, K=K, fl=None, rows=None, pen=1.0, tok=tok):
        return L.svln_op_gemm_argmax_scores(m._h, ptr(A), lda, ptr(W), ldw, M, N, K, ptr(fl), rows, pen, tok, lp)

    assert mfma() == 0 and mfma(fl=fl, rows=prow, pen=2.0) == 0
    assert mfma(A=None) != 0 and mfma(W=None) != 0 and mfma(tok=None) != 0 and mfma(M=0) != 0 and mfma(M=33) != 0
    assert mfma(N=0) != 0 and mfma(N=128 * 2048 + 1) != 0 and mfma(K=K - epc // 2) != 0 and mfma(lda=K - epc) != 0 and mfma(ldw=K - epc) != 0
    assert mfma(A=x.view(-1)[epc // 2:]) != 0 and mfma(fl=fl) != 0 and mfma(fl=fl, rows=prow, pen=0.0) != 0


def test_zz_worst_error_report():
    """prints the worst op-level error of this run per kernel shape (the README records it); the bound itself is asserted per case"""
    for kind, w in sorted(WORST.items()):
        print(f"worst |logprob - float64 reference| over the {kind} cases: {w:.3e}")
        assert w <= S.TOL
