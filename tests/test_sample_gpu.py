"""Temperature sampling at op level (svln_set_sampling): the noise as the kernels evaluate it (svln_op_gumbel) and the EPI_SAMPLE siblings of
gemv_rows_kernel (four weight policies), gemv_batched_kernel and the MFMA arg-max epilogue, each with its final kernel, through the
test-only entries svln_op_*_argmax_sample on the exact cases of tests/sample_ref.py (tests/test_sample_inputs.py proves them sharp, and
that every case keeps its perturbed top-2 margin: no case is skipped here).

Noise: |G - G64| <= 2^-18 max(1, |G|) -- two hardware logarithms of 1 ulp each plus the multiply chain, doubled -- over a full vocabulary
for three draws and over 72 + 72 (draw, column) pairs in the two tails (u > 1 - 2^-20, u < 2^-20: tests/golden/sample_tail_pairs.json,
found by a CPU search with the restated Philox).
Cases: the tokens equal the restatement's, |score - float64 log softmax(x / T)[token]| <= 2e-5 (sample_ref.TOL)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import sample_ref as R
import scores_ref as S
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import GOLD, ptr

pytestmark = pytest.mark.gpu
_engines = {}
WORST = {}
G_BOUND = 2.0 ** -18


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _gumbel(m, seed, stream, draw, n0, count):
    out = np.full(count, np.nan, dtype=np.float32)
    _lib.check(m._lib.svln_op_gumbel(m._h, seed, stream, draw, n0, count, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def _noise_err(got, ref):
    return np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))


def test_noise_over_a_full_vocabulary():
    m = engine(torch.float32)
    V, seed, stream = 152064, 0x5EED7A11, 1
    worst = 0.0
    for draw in (0, 1, 123456789):
        got = _gumbel(m, seed, stream, draw, 0, V)
        err = _noise_err(got, R.gumbel(seed, stream, draw, np.arange(V)))
        worst = max(worst, float(err.max()))
        assert np.isfinite(got).all() and err.max() <= G_BOUND, (draw, float(err.max()), int(err.argmax()))
    WORST["noise (vocabulary)"] = worst
    print(f"worst |G - G64| / max(1, |G|) over 3 x {V} columns: {worst:.3e} (bound {G_BOUND:.3e})")


def test_noise_in_both_tails():
    """u -> 1 (E -> 2^-24: the winners' tail, where E must be RELATIVELY accurate) and u -> 0"""
    m = engine(torch.float32)
    t = json.load(open(os.path.join(GOLD, "sample_tail_pairs.json")))
    for name in ("upper", "lower"):
        pairs = t[name]
        assert len(pairs) >= 64
        worst = 0.0
        for draw, col in pairs:
            ref = R.gumbel(t["seed"], t["stream"], draw, np.array([col]))
            u = R.uniform(R.noise_bits(t["seed"], t["stream"], draw, np.array([col])))[0]
            assert u > 1 - 2.0 ** -20 if name == "upper" else u < 2.0 ** -20
            err = float(_noise_err(_gumbel(m, t["seed"], t["stream"], draw, col, 1), ref)[0])
            worst = max(worst, err)
        WORST[f"noise ({name} tail)"] = worst
        print(f"worst |G - G64| / max(1, |G|) over {len(pairs)} {name}-tail pairs: {worst:.3e} (bound {G_BOUND:.3e})")
        assert worst <= G_BOUND, (name, worst)


def _check_case(case, toks, lps):
    ref = case.reference()
    exp = [r[0] for r in ref]
    assert toks == exp, (case.id, "tokens", toks, exp, [r[2] / r[3] if r[3] else None for r in ref])
    errs = [abs(lps[b] - ref[b][1]) for b in range(case.B)]
    worst = max(errs)
    WORST[case.kind] = max(WORST.get(case.kind, 0.0), worst if not math.isnan(worst) else float("inf"))
    print(f"{case.id}: seed {case.seed:#x}, worst |score - ref| = {worst:.3e}")
    assert all(e <= R.TOL for e in errs), (case.id, errs, lps, [r[1] for r in ref])


def _flag_ops(case):
    _, flags, rows = case.logits()
    if flags is None:
        return None, None
    return flags.cuda(), torch.tensor(rows, dtype=torch.int32).cuda()


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _rows_call(m, case, ops, dx, fr):
    tok, lp = C.c_int32(-7), C.c_float(float("nan"))
    _lib.check(m._lib.svln_op_gemv_argmax_sample(m._h, S.FMT_ID[case.fmt], ptr(ops["W"]), ptr(ops.get("aux")), case.K, ptr(dx), case.N, case.K,
                                                 ptr(fr), R.PEN, case.T, case.seed, case.streams[0], case.draws[0], C.byref(tok), C.byref(lp)))
    return [tok.value], [lp.value]


@pytest.mark.parametrize("case", R.rows_cases() + [R.u24_case()], ids=lambda c: c.id)
def test_gemv_rows_sample(case):
    dt = case.dtype
    m = engine(dt)
    x, W = case.operands()
    ops = {k: v.cuda() for k, v in S.pack(case.fmt, W).items()}
    dx = x[0].to(dt).cuda()
    flags, rows = _flag_ops(case)
    fr = None if flags is None else flags[int(rows[0])].contiguous()
    torch.cuda.synchronize()
    _check_case(case, *_rows_call(m, case, ops, dx, fr))


def _batched_inputs(case, ld_pad):
    dt = case.dtype
    x, W = case.operands()
    xp = torch.full((case.B, case.K + ld_pad), 3.0e4, dtype=torch.float64)
    xp[:, :case.K] = x
    return xp.to(dt).cuda(), W.to(dt).cuda()


def _batched_call(m, case, dW, dx, flags, rows, ldx):
    toks, lps = (C.c_int32 * 8)(*([-7] * 8)), (C.c_float * 8)(*([float("nan")] * 8))
    _lib.check(m._lib.svln_op_gemv_batched_argmax_sample(m._h, ptr(dW), case.K, ptr(dx), ldx, None, S.G.EPS, case.N, case.K, case.B, ptr(flags),
                                                         None if rows is None else C.cast(ptr(rows), C.POINTER(C.c_int32)), R.PEN, case.T,
                                                         case.seed, _i32(case.streams), _i32(case.draws), toks, lps))
    return list(toks)[:case.B], list(lps)[:case.B]


def _mfma_call(m, case, dW, dx, flags, rows):
    toks, lps = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32))
    _lib.check(m._lib.svln_op_gemm_argmax_sample(m._h, ptr(dx), case.K, ptr(dW), case.K, case.B, case.N, case.K, ptr(flags),
                                                 None if rows is None else C.cast(ptr(rows), C.POINTER(C.c_int32)), R.PEN, case.T, case.seed,
                                                 _i32(case.streams), _i32(case.draws), toks, lps))
    return list(toks)[:case.B], list(lps)[:case.B]


@pytest.mark.parametrize("case", R.batched_cases(), ids=lambda c: c.id)
def test_gemv_batched_sample(case):
    m = engine(case.dtype)
    dx, dW = _batched_inputs(case, 16)
    flags, rows = _flag_ops(case)
    torch.cuda.synchronize()
    _check_case(case, *_batched_call(m, case, dW, dx, flags, rows, case.K + 16))


@pytest.mark.parametrize("case", R.mfma_cases(), ids=lambda c: c.id)
def test_gemm_argmax_sample(case):
    m = engine(case.dtype)
    dx, dW = _batched_inputs(case, 0)
    flags, rows = _flag_ops(case)
    torch.cuda.synchronize()
    toks, lps = _mfma_call(m, case, dW, dx, flags, rows)
    _check_case(case, toks, lps)
    if case.B >= 2 and case.N == 645:   # rows 0 and 1 share their logits and differ in stream and draw only: they must sample differently
        assert toks[0] != toks[1], (case.id, toks[:2])      # (tests/test_sample_inputs.py: the reference does, in every such case)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_noise_identity_across_the_three_forms(dt):
    """the same logits, stream and draw through the rows kernel, the batched GEMV (B = 1 .. 8) and the MFMA tiles: the same token and the
    same score within the bound -- the noise does not depend on which kernel, tile, wave or batch row evaluates the column"""
    fmt = "plain-fp32" if dt == torch.float32 else "plain-bf16"
    m = engine(dt)
    base = R.Case("mfma", 645, 576, B=8, fmt=fmt, T=1.0, pen=True, seed=321)
    x, W = base.operands()
    dW = W.to(dt).cuda()
    dX = x.to(dt).cuda().contiguous()
    flags, rows = _flag_ops(base)
    torch.cuda.synchronize()
    ref = base.reference()
    mf_t, mf_s = _mfma_call(m, base, dW, dX, flags, rows)
    assert mf_t == [r[0] for r in ref]
    for B in (1, 2, 4, 8):
        sub = R.Case("batched", 645, 576, B=B, fmt=fmt, T=1.0, pen=True, seed=321)
        sub.forced, sub.streams, sub.draws = base.seed, base.streams[:B], base.draws[:B]
        t, s = _batched_call(m, sub, dW, dX, flags, rows, 576)
        assert t == mf_t[:B], (B, t, mf_t)
        assert all(abs(a - b) <= 2 * R.TOL for a, b in zip(s, mf_s))
    for b in range(8):
        one = R.Case("rows", 645, 576, fmt=fmt, T=1.0, pen=True, seed=321)
        one.forced, one.streams, one.draws = base.seed, [base.streams[b]], [base.draws[b]]
        t, s = _rows_call(m, one, {"W": dW}, dX[b].contiguous(), flags[int(rows[b])].contiguous())
        assert t == [mf_t[b]], (b, t, mf_t)
        assert abs(s[0] - mf_s[b]) <= 2 * R.TOL


def test_no_finite_logit_and_ninf_column():
    """a row without a finite logit gives token -1 and a NaN score; a -inf column never wins and adds nothing to the sum"""
    m = engine(torch.float32)
    K, N = 96, 9
    dx = torch.ones(K, dtype=torch.float32).cuda()
    dW = torch.full((N, K), float("nan"), dtype=torch.float32).cuda()
    tok, lp = C.c_int32(-7), C.c_float(0.0)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gemv_argmax_sample(m._h, 0, ptr(dW), None, K, ptr(dx), N, K, None, 1.0, 1.0, 1, 0, 0, C.byref(tok), C.byref(lp)))
    assert tok.value == -1 and math.isnan(lp.value)
    W = torch.zeros((N, K), dtype=torch.float32)
    W[:, 0] = float("-inf")
    W[3, 0] = 0.0
    dW = W.cuda()
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gemv_argmax_sample(m._h, 0, ptr(dW), None, K, ptr(dx), N, K, None, 1.0, 1.0, 1, 0, 0, C.byref(tok), C.byref(lp)))
    assert tok.value == 3 and abs(lp.value) <= 1e-6


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_malformed_calls_are_refused_before_any_launch(dt):
    m = engine(dt)
    epc = 4 if dt == torch.float32 else 8
    K, N, B = 256, 16, 2
    W = torch.zeros((N, K), dtype=dt, device="cuda")
    x = torch.zeros((B, K), dtype=dt, device="cuda")
    g = torch.ones((K,), dtype=dt, device="cuda")
    tok, lp = (C.c_int32 * 32)(), (C.c_float * 32)()
    st, dr, neg = _i32([0, 1]), _i32([0, 5]), _i32([0, -1])
    torch.cuda.synchronize()
    L = m._lib

    def gemv(W=W, x=x, N=N, K=K, T=1.0, stream=0, draw=0, tok=tok, lp=lp):
        return L.svln_op_gemv_argmax_sample(m._h, 0, ptr(W), None, K, ptr(x), N, K, None, 1.0, T, 7, stream, draw, tok, lp)

    assert gemv() == 0
    assert gemv(W=None) != 0 and gemv(x=None) != 0 and gemv(tok=None) != 0 and gemv(lp=None) != 0 and gemv(N=0) != 0 and gemv(K=K - epc // 2) != 0
    assert gemv(T=0.0) != 0 and gemv(T=-1.0) != 0 and gemv(T=float("nan")) != 0 and gemv(T=float("inf")) != 0 and gemv(T=1e-45) != 0
    assert gemv(stream=-1) != 0 and gemv(draw=-1) != 0

    def bat(norm=None, B=B, T=1.0, st=st, dr=dr, lp=lp):
        return L.svln_op_gemv_batched_argmax_sample(m._h, ptr(W), K, ptr(x), K, ptr(norm), 1e-6, N, K, B, None, None, 1.0, T, 7, st, dr, tok, lp)

    assert bat() == 0
    assert bat(norm=g) != 0 and b"norm" in L.svln_last_error()
    assert bat(B=3) != 0 and bat(T=0.0) != 0 and bat(st=None) != 0 and bat(dr=None) != 0 and bat(dr=neg) != 0 and bat(lp=None) != 0

    def mfma(M=B, T=1.0, st=st, dr=dr, lp=lp):
        return L.svln_op_gemm_argmax_sample(m._h, ptr(x), K, ptr(W), K, M, N, K, None, None, 1.0, T, 7, st, dr, tok, lp)

    assert mfma() == 0
    assert mfma(M=0) != 0 and mfma(M=33) != 0 and mfma(T=-2.0) != 0 and mfma(st=None) != 0 and mfma(st=neg) != 0 and mfma(lp=None) != 0
    out = (C.c_float * 4)()
    assert L.svln_op_gumbel(m._h, 1, 0, 0, 0, 4, out) == 0
    assert L.svln_op_gumbel(m._h, 1, 0, 0, 0, 0, out) != 0 and L.svln_op_gumbel(m._h, 1, 0, 0, 0, 4, None) != 0
    assert L.svln_op_gumbel(m._h, 1, -1, 0, 0, 4, out) != 0 and L.svln_op_gumbel(m._h, 1, 0, -1, 0, 4, out) != 0
    assert L.svln_op_gumbel(m._h, 1, 0, 0, -1, 4, out) != 0 and L.svln_op_gumbel(m._h, 1, 0, 0, 2 ** 31 - 2, 4, out) != 0


def test_zz_worst_error_report():
    """prints the worst errors of this run (the README records them); the bounds themselves are asserted per case"""
    for kind, w in sorted(WORST.items()):
        print(f"worst error, {kind}: {w:.3e}")
        assert w <= (G_BOUND if kind.startswith("noise") else R.TOL)
