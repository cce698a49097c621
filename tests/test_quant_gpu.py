"""The two e4m3 quantisers on designed inputs: quant_fp8_rows_kernel (csrc/gemv.hip) through svln_op_quant_fp8 and the e4m3 branch of
splitk_rownorm_kernel (csrc/gemm.hip) through svln_op_gemm_norm_q8, against tests/quant_ref.py: a float32 restatement of the kernels'
operation order with an e4m3 encoder written on integer bits (no torch.float8_e4m3fn).  tests/test_quant_inputs.py proves on the CPU that
every plausible mistake -- rounding mode, encoding, divisor, a share of the row missing from the maximum, a neighbour's scale, the NaN
rule, the scale floor -- changes a byte or a scale bit on these inputs.

Every comparison is bit equality: bytes after quant_ref.fold (-0 onto +0, 0xFF onto 0x7F), scales by their fp32 bits.  Outputs sit
between guard bands that must stay untouched.  The fused reduce is compared on the rows the device itself stored in norm_out, so the
product and the norm (held in tests/test_gemm_gpu.py) do not enter.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import quant_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr, q, rnd

pytestmark = pytest.mark.gpu
GUARD, FILL8, FILLS = 64, 0x55, -7.5
EPS = 1e-6
_engines = {}


def engine():
    if "m" not in _engines:
        _engines["m"] = StreamVLNForCausalLM(TINY, dtype=torch.bfloat16, max_envs=1, max_frames=3, max_positions=2048)
    return _engines["m"]


def _guarded(n, fill, dtype):
    return torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")


def _inner(buf, n, fill, what):
    """the n payload elements of a guarded buffer, after checking that both bands still hold `fill`"""
    b = buf.cpu()
    assert bool((b[:GUARD] == fill).all()) and bool((b[GUARD + n:] == fill).all()), f"{what}: a guard band was written"
    return b[GUARD:GUARD + n]


def _offset(buf):
    return C.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def _quant_op(m, W):
    """svln_op_quant_fp8 on fp32 values of bf16 -> (bytes [rows][cols], scale [rows]) as numpy"""
    rows, cols = W.shape
    dW = W.to(torch.bfloat16).cuda()
    w8, sc = _guarded(rows * cols, FILL8, torch.uint8), _guarded(rows, FILLS, torch.float32)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_quant_fp8(m._h, ptr(dW), rows, cols, _offset(w8), _offset(sc)))
    return _inner(w8, rows * cols, FILL8, "w8").reshape(rows, cols).numpy(), _inner(sc, rows, FILLS, "scale").numpy()


def _assert_same(got, exp, what):
    gs, es = np.asarray(got[1], dtype=np.float32).view(np.uint32), np.asarray(exp[1], dtype=np.float32).view(np.uint32)
    assert np.array_equal(gs, es), f"{what}: scales differ in rows {np.nonzero(gs != es)[0].tolist()[:8]}: {got[1][gs != es][:4]} != {exp[1][gs != es][:4]}"
    gb, eb = R.fold(got[0]), R.fold(exp[0])
    bad = np.argwhere(gb != eb)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {gb.size} bytes differ, first at {bad[:6].tolist()}: "
                           f"{[hex(gb[r, c]) for r, c in bad[:6]]} != {[hex(eb[r, c]) for r, c in bad[:6]]}")


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_quant_fp8_bytes_and_scales_equal_the_restatement(case):
    _assert_same(_quant_op(engine(), case.W), R.quant_rows(case.W), case.id)


# ----------------------------------------------------------------------------- the fused reduce
K_FUSED, SPLIT = 256, 2


def _steer_columns(N):
    """the columns whose norm weight is made large so that the row maximum falls there: in the first and the last quad of the row, and
    in every wave of the reduce (one thread = 4 columns, one wave = 256 columns)"""
    cols = {"first quad": 1, "last quad": N - 2}
    for w in range((N + 255) // 256):
        cols[f"wave {w}"] = min(256 * w + 77, N - 5) if N > 16 else 9
    return cols


def _fused(m, A, W, res, g):
    """one svln_op_gemm_norm_q8 call -> (norm_out rows as fp32 [M][N], (q8 bytes, scales))"""
    M, N = res.shape
    K = A.shape[1]
    dA, dW, dg = A.to(torch.bfloat16).cuda(), W.to(torch.bfloat16).cuda(), g.to(torch.bfloat16).cuda()
    x = res.to(torch.bfloat16).cuda()
    xn = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    q8, sc = _guarded(M * N, FILL8, torch.uint8), _guarded(M, FILLS, torch.float32)
    fused = C.c_int32(-1)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gemm_norm_q8(m._h, ptr(dA), K, ptr(dW), K, ptr(x), N, ptr(x), N, ptr(dg), ptr(xn), EPS, M, N, K, SPLIT, _offset(q8),
                                           _offset(sc), C.byref(fused)))
    torch.cuda.synchronize()
    assert fused.value == 1, (M, N, fused.value)
    return xn.float().cpu(), (_inner(q8, M * N, FILL8, "q8").reshape(M, N).numpy(), _inner(sc, M, FILLS, "q8 scale").numpy())


_operands = {}


def _fused_operands(N):
    if N not in _operands:
        _operands[N] = (q(rnd((37, K_FUSED), 71), torch.bfloat16), q(rnd((N, K_FUSED), 72, 1.0 / math.sqrt(K_FUSED)), torch.bfloat16),
                        q(rnd((37, N), 73), torch.bfloat16), q(1.0 + rnd((N,), 74, 0.2), torch.bfloat16))
    return _operands[N]


@pytest.mark.parametrize("M", [1, 3, 37])
@pytest.mark.parametrize("N", [16, 48, 272, 1024, 3584, 4096])
def test_fused_norm_quantisation_on_steered_rows(N, M):
    """N: 4 threads, a partial wave, 68 threads across a wave edge, 4 / 14 / 16 waves (the reduce's maximum).  Both quantisers are held to
    the restatement on the rows the reduce stored, and to each other."""
    m = engine()
    A, W, res, g = _fused_operands(N)
    A, res = A[:M], res[:M]
    for what, col in _steer_columns(N).items():
        gs, rs = g.clone(), res.clone()
        gs[col] = -48.0 if col % 2 else 48.0
        rs[:, col] = 3.0                                         # (the product's share of a column is about +-1: the column is not near 0)
        rows, got = _fused(m, A, W, rs, gs)
        assert bool((rows.abs().argmax(1) == col).all()), (N, M, what)
        exp = R.quant_rows(rows)
        _assert_same(got, exp, f"fused {M}x{N} maximum in the {what}")
        _assert_same(_quant_op(m, rows), got, f"quantise kernel against the fused reduce, {M}x{N} {what}")
    # a zero row (zero A row, zero residual): scale 1, bytes 0; a NaN through the residual: NaN bytes; beside untouched rows
    A2, res2 = A.clone(), res.clone()
    zero_row, nan_row = 0, M - 1
    if M > 1:
        A2[zero_row], res2[zero_row] = 0.0, 0.0
    res2[nan_row, N // 2] = float("nan")
    rows, got = _fused(m, A2, W, res2, g)
    _assert_same(got, R.quant_rows(rows), f"fused {M}x{N} zero and NaN rows")
    _assert_same(_quant_op(m, rows), got, f"quantise kernel against the fused reduce, {M}x{N} zero and NaN rows")
    assert bool(torch.isnan(rows[nan_row]).any()) and bool((R.fold(got[0][nan_row])[torch.isnan(rows[nan_row]).numpy()] == 0x7F).all())
    if M > 1:
        assert got[1][zero_row] == 1.0 and not R.fold(got[0][zero_row]).any()
    else:
        A2, res2 = torch.zeros_like(A), torch.zeros_like(res)
        rows, got = _fused(m, A2, W, res2, g)
        assert got[1][0] == 1.0 and not R.fold(got[0][0]).any() and not rows.any()
    if M > 2:
        assert bool(torch.isfinite(rows[1:M - 1]).all()) and not (R.fold(got[0][1:M - 1]) == 0x7F).any()
    # tiny rows with zeros in them (a norm weight of 2^-124, every seventh one 0): zeros stay byte 0 under the scale floor
    gt = torch.full((N,), 2.0 ** -124)
    gt[::7] = 0.0
    rows, got = _fused(m, A, W, res, gt)
    _assert_same(got, R.quant_rows(rows), f"fused {M}x{N} tiny rows")
    _assert_same(_quant_op(m, rows), got, f"quantise kernel against the fused reduce, {M}x{N} tiny rows")
    assert not (R.fold(got[0]) == 0x7F).any() and not R.fold(got[0])[:, ::7].any() and float(rows.abs().max()) < 1.3e-36


# ----------------------------------------------------------------------------- downstream and the entry's checks
def test_a_nan_byte_stays_nan_through_the_fp8_gemv_and_gemm():
    m = engine()
    dtype = torch.bfloat16
    N, K, M, bad = 128, 128, 8, 37
    W = q(rnd((N, K), 41, 1.0 / math.sqrt(K)), dtype)
    Wn = W.clone()
    Wn[bad, 77] = float("nan")
    (w8, sw), (w8n, swn) = _quant_op(m, W), _quant_op(m, Wn)
    assert R.fold(w8n)[bad, 77] == 0x7F and np.array_equal(np.delete(w8n, bad, 0), np.delete(w8, bad, 0)) and np.array_equal(sw, swn)
    x = q(rnd((K,), 42), dtype).to(dtype).cuda()
    A = q(rnd((M, K), 43), dtype)
    a8, sa = _quant_op(m, A)
    outs = []
    for b in (w8, w8n):
        d8, ds = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(sw.copy()).cuda()
        y = torch.zeros((N,), dtype=dtype, device="cuda")
        Y = torch.zeros((M, N), dtype=dtype, device="cuda")
        dA8, dsa = torch.from_numpy(a8.copy()).cuda(), torch.from_numpy(sa.copy()).cuda()
        torch.cuda.synchronize()
        _lib.check(m._lib.svln_op_gemv_fp8(m._h, ptr(d8), ptr(ds), K, ptr(x), None, EPS, None, None, ptr(y), N, K, _lib.EPI_NONE, None))
        _lib.check(m._lib.svln_op_gemm_fp8(m._h, ptr(dA8), ptr(dsa), K, ptr(d8), ptr(ds), K, ptr(Y), N, None, None, 0, M, N, K, _lib.EPI_NONE, 0, 0))
        torch.cuda.synchronize()
        outs.append((y.float().cpu(), Y.float().cpu()))
    (y0, Y0), (y1, Y1) = outs
    keep = torch.arange(N) != bad
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(Y0).all())
    assert bool(torch.isnan(y1[bad])) and torch.equal(y1[keep], y0[keep])
    assert bool(torch.isnan(Y1[:, bad]).all()) and torch.equal(Y1[:, keep], Y0[:, keep])


def test_quant_fp8_refuses_malformed_calls_before_any_launch():
    m = engine()
    rows, cols = 4, 64
    dW = q(rnd((rows, cols), 5), torch.bfloat16).to(torch.bfloat16).cuda()
    w8, sc = _guarded(rows * cols, FILL8, torch.uint8), _guarded(rows, FILLS, torch.float32)
    torch.cuda.synchronize()
    call = lambda w, r, c, o, s: m._lib.svln_op_quant_fp8(m._h, w, r, c, o, s)
    for what, args, msg in [("null input", (None, rows, cols, ptr(w8), ptr(sc)), "null pointer"),
                            ("null bytes", (ptr(dW), rows, cols, None, ptr(sc)), "null pointer"),
                            ("null scale", (ptr(dW), rows, cols, ptr(w8), None), "null pointer"),
                            ("rows < 0", (ptr(dW), -1, cols, ptr(w8), ptr(sc)), "rows must be >= 0"),
                            ("cols == 0", (ptr(dW), rows, 0, ptr(w8), ptr(sc)), "positive multiple of 16"),
                            ("cols < 0", (ptr(dW), rows, -16, ptr(w8), ptr(sc)), "positive multiple of 16"),
                            ("cols % 16", (ptr(dW), rows, 24, ptr(w8), ptr(sc)), "positive multiple of 16")]:
        rc = call(*args)
        assert rc != 0, what
        with pytest.raises(_lib.SvlnError, match=msg):
            _lib.check(rc)
    assert call(ptr(dW), 0, cols, ptr(w8), ptr(sc)) == 0                     # no rows: nothing to do, nothing launched
    torch.cuda.synchronize()
    assert bool((w8.cpu() == FILL8).all()) and bool((sc.cpu() == FILLS).all())       # none of the calls above wrote anything
    assert call(ptr(dW), rows, cols, _offset(w8), _offset(sc)) == 0
    got = (_inner(w8, rows * cols, FILL8, "w8").reshape(rows, cols).numpy(), _inner(sc, rows, FILLS, "scale").numpy())
    _assert_same(got, R.quant_rows(dW.float().cpu()), "after the refusals")
