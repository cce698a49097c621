"""The decode GEMVs (gemv.hip: gemv_rows_kernel, gemv_ksplit_kernel, gemv_batched_kernel) through svln_op_gemv / _fp8 / _mxfp4 / _batched
on the cases of tests/gemv_ref.py: inputs on which a subtly wrong kernel fails (tests/test_gemv_inputs.py proves that on the CPU).

  exact cases      dyadic values, power-of-two scales that change with every row / block: the un-normalised EPI_NONE output and the
                   arg-max winner are defined bit for bit -> torch.equal on the stored bits, the planted lowest index.
  toleranced cases (RMSNorm with eps-sized / outlier activations, SwiGLU over wide exact gate sums): float64 reference, util.assert_close.
Every output sits in a guard band that must stay untouched; with ldw > K the row padding holds poison."""
import ctypes as C

import pytest
import torch

import gemv_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import assert_close, ptr

pytestmark = pytest.mark.gpu
EPI = {"none": _lib.EPI_NONE, "swiglu": _lib.EPI_SWIGLU, "argmax": _lib.EPI_ARGMAX}
GUARD, FILL = 64, 777.0
_engines = {}


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _launch(m, case, ops, x, g, b, r, y):
    tok = C.c_int32(-7)
    tail = (case.W.ldw, ptr(x), ptr(g), R.EPS, ptr(b), ptr(r), ptr(y), case.N, case.K, EPI[case.epi], C.byref(tok))
    torch.cuda.synchronize()
    if case.fmt == "e4m3":
        rc = m._lib.svln_op_gemv_fp8(m._h, ptr(ops["w8"]), ptr(ops["scale"]), *tail)
    elif case.fmt == "mxfp4":
        rc = m._lib.svln_op_gemv_mxfp4(m._h, ptr(ops["q4"]), ptr(ops["e8"]), *tail)
    else:
        rc = m._lib.svln_op_gemv(m._h, ptr(ops["W"]), *tail)
    _lib.check(rc)
    return tok.value


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_gemv(case):
    case.build()
    dt = case.dtype
    m = engine(dt)
    dev = lambda t: None if t is None else t.to(dt).cuda()
    ops = {k: v.cuda() for k, v in case.W.ops.items()}
    buf = torch.full((case.n_out + 2 * GUARD,), FILL, dtype=dt, device="cuda")
    y = None if case.epi == "argmax" else buf[GUARD:GUARD + case.n_out]
    tok = _launch(m, case, ops, dev(case.x), dev(case.g), dev(case.bias), dev(case.res), y)
    out = buf.cpu()
    assert bool((out[:GUARD] == FILL).all()) and bool((out[GUARD + case.n_out:] == FILL).all()), f"{case.id}: guard band written"
    if case.epi == "argmax":
        assert tok == case.winner, (case.id, tok, case.winner, case.tie_set)
        return
    got = out[GUARD:GUARD + case.n_out]
    if case.exact:
        exp = case.reference().to(dt)
        bad = _bits(got) != _bits(exp)
        assert not bool(bad.any()), f"{case.id}: {int(bad.sum())} of {bad.numel()} outputs differ in their bits, first at {int(torch.nonzero(bad)[0])}"
    else:
        assert_close(got, case.reference(), dt, case.id)


@pytest.mark.parametrize("case", R.BATCHED_CASES, ids=lambda c: c.id)
def test_gemv_batched(case):
    case.build()
    dt, B, N, K, n_out = case.dtype, case.B, case.N, case.K, case.n_out
    m = engine(dt)
    ldx, ldy, ldr = K + 16, n_out + 24, N + 8
    x = torch.full((B, ldx), 3.0e4, dtype=torch.float64)
    x[:, :K] = case.x
    dx, dW = x.to(dt).cuda(), case.W.ops["W"].cuda()
    dg = None if case.g is None else case.g.to(dt).cuda()
    db = None if case.bias is None else case.bias.to(dt).cuda()
    dr = None
    if case.res is not None:
        r = torch.full((B, ldr), 3.0e4, dtype=torch.float64)
        r[:, :N] = case.res
        dr = r.to(dt).cuda()
    buf = torch.full((GUARD + B * ldy + GUARD,), FILL, dtype=dt, device="cuda")
    y = buf[GUARD:]
    toks = (C.c_int32 * 8)(*([-7] * 8))
    torch.cuda.synchronize()
    argmax = case.epi == "argmax"
    _lib.check(m._lib.svln_op_gemv_batched(m._h, ptr(dW), case.W.ldw, ptr(dx), ldx, ptr(dg), R.EPS, ptr(db), ptr(dr), ldr if dr is not None else 0,
                                           None if argmax else ptr(y), 0 if argmax else ldy, N, K, EPI[case.epi], B, toks))
    out = buf.cpu()
    rows = out[GUARD:GUARD + B * ldy].view(B, ldy)
    keep = n_out if not argmax else 0
    assert bool((out[:GUARD] == FILL).all()) and bool((out[GUARD + B * ldy:] == FILL).all()) and bool((rows[:, keep:] == FILL).all()), \
        f"{case.id}: guard band or row padding written"
    if argmax:
        assert [toks[b] for b in range(B)] == [min(s) for s in case.tie_sets], (case.id, list(toks), case.tie_sets)
        return
    got = rows[:, :n_out]
    if case.exact:
        exp = case.reference().to(dt)
        bad = _bits(got) != _bits(exp)
        assert not bool(bad.any()), f"{case.id}: {int(bad.sum())} of {bad.numel()} outputs differ in their bits"
    else:
        assert_close(got, case.reference(), dt, case.id)


@pytest.mark.parametrize("fmt", ["plain-fp32", "plain-bf16", "e4m3"])
def test_gemv_refusals(fmt):
    """svln_op_gemv and svln_op_gemv_fp8 refuse what svln_op_gemv_mxfp4 refuses, before anything is launched: null pointers, N < 1, K not a
    multiple of the format's chunk, ldw < K or unaligned for the 16-byte loads, and a K whose fp32 copy exceeds the LDS of the wave-per-rows
    kernel."""
    dt = R.DTYPE[fmt]
    m = engine(dt)
    epc, K, N = R.EPC[fmt], 256, 16
    W = torch.zeros((N, K + 64), dtype=torch.uint8 if fmt == "e4m3" else dt, device="cuda")
    sc = torch.ones((N,), dtype=torch.float32, device="cuda")
    x = torch.zeros((K,), dtype=dt, device="cuda")
    y = torch.zeros((N,), dtype=dt, device="cuda")
    torch.cuda.synchronize()

    def call(W=W, sc=sc, ldw=K, x=x, y=y, N=N, K=K, epi=_lib.EPI_NONE):
        tail = (ldw, ptr(x), None, R.EPS, None, None, ptr(y), N, K, epi, None)
        if fmt == "e4m3":
            return m._lib.svln_op_gemv_fp8(m._h, ptr(W), ptr(sc), *tail)
        return m._lib.svln_op_gemv(m._h, ptr(W), *tail)

    assert call() == 0 and call(ldw=K + 64) == 0
    assert call(W=None) != 0 and call(x=None) != 0 and call(y=None) != 0
    if fmt == "e4m3":
        assert call(sc=None) != 0
    assert call(N=0) != 0 and call(N=-4) != 0
    assert call(K=K - epc // 2) != 0 and call(K=0) != 0
    assert call(ldw=K - epc) != 0 and call(ldw=K + epc // 2) != 0
    assert call(epi=_lib.EPI_SWIGLU, N=N + 16) != 0                               # SwiGLU: whole [gate 32 | up 32] blocks
    big = (160 * 1024 // 4 // epc + 1) * epc                                      # K * 4 bytes past the LDS of the rows kernel
    assert call(K=big, ldw=big, N=9000) != 0 and call(K=big, ldw=big, N=64, epi=_lib.EPI_SWIGLU) != 0
    tok = C.c_int32(-7)
    tail = (big, ptr(x), None, R.EPS, None, None, None, 64, big, _lib.EPI_ARGMAX, C.byref(tok))
    assert (m._lib.svln_op_gemv_fp8(m._h, ptr(W), ptr(sc), *tail) if fmt == "e4m3" else m._lib.svln_op_gemv(m._h, ptr(W), *tail)) != 0
