"""The batched MXFP4 GEMV (gemv_mx4b.hip) through svln_op_gemv_mxfp4_batched on the cases of tests/mx4b_ref.py: inputs on which a subtly
wrong kernel fails (tests/test_mx4b_inputs.py proves that on the CPU).

  exact cases   sparse E2M1 codes, block scales that change with every row and block, dense x in {-1, 0, 1} different for every env:
                every expected output is a bf16 value -> torch.equal on the stored bits of the whole y buffer (guard bands and the row
                padding ldy > n_out included; poison in the ldw / ldx / ldr padding).
  SwiGLU        wide exact gate sums, float64 reference, util.assert_close.
  arg-max       planted exact ties per env at different places (one 16-row group, the two groups of a tile, two grid-stride passes, two
                workgroups), one env whose winner carries the penalty flag, one env without a finite logit.
  refusals      every malformed call returns non-zero and leaves y untouched."""
import ctypes as C

import pytest
import torch

import mx4b_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import assert_close, ptr

pytestmark = pytest.mark.gpu
EPI = {"none": _lib.EPI_NONE, "swiglu": _lib.EPI_SWIGLU, "argmax": _lib.EPI_ARGMAX}
_engines = {}


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_gemv_mxfp4_batched(case):
    case.build()
    dt = torch.bfloat16
    m = engine(dt)
    B, N, K = case.B, case.N, case.K
    dq, de = case.W.ops["q4"].cuda(), case.W.ops["e8"].cuda()
    dx = case.x_image().to(dt).cuda()
    db = None if case.bias is None else case.bias.to(dt).cuda()
    dr = None if case.res is None else case.res_image().to(dt).cuda()
    buf = torch.full((R.GUARD + B * case.ldy + R.GUARD,), R.FILL, dtype=dt, device="cuda")
    y = buf[R.GUARD:]
    toks = (C.c_int32 * 8)(*([-7] * 8))
    argmax = case.epi == "argmax"
    torch.cuda.synchronize()
    if argmax:
        flags = case.flags.cuda()
        rows = torch.arange(B, dtype=torch.int32).flip(0).contiguous()          # vector b uses flag row B - 1 - b: the table is followed
        dflags, drows = flags.flip(0).contiguous(), rows.cuda()
        torch.cuda.synchronize()
        _lib.check(m._lib.svln_op_gemv_mxfp4_batched_argmax_pen(m._h, ptr(dq), ptr(de), case.ldw, ptr(dx), case.ldx, N, K, B, ptr(dflags),
                                                                ptr(drows), case.pen, toks))
        assert [toks[b] for b in range(B)] == case.tokens(), (case.id, list(toks), case.tokens(), case.tie_sets)
        # without the flags the penalised env goes back to the lowest index of its tie
        _lib.check(m._lib.svln_op_gemv_mxfp4_batched(m._h, ptr(dq), ptr(de), case.ldw, ptr(dx), case.ldx, None, None, 0, None, 0, N, K,
                                                     EPI["argmax"], B, toks))
        exp = [-1 if b == case.nan_row else min(case.tie_sets[b]) for b in range(B)]
        assert [toks[b] for b in range(B)] == exp, (case.id, list(toks), exp)
        assert bool((buf == R.FILL).all())
        return
    _lib.check(m._lib.svln_op_gemv_mxfp4_batched(m._h, ptr(dq), ptr(de), case.ldw, ptr(dx), case.ldx, ptr(db), ptr(dr), case.ldr if dr is not None else 0,
                                                 ptr(y), case.ldy, N, K, EPI[case.epi], B, None))
    out = buf.cpu()
    if case.exact:
        exp = case.image()
        bad = _bits(out) != _bits(exp)
        assert not bool(bad.any()), f"{case.id}: {int(bad.sum())} of {bad.numel()} elements of the y buffer differ in their bits, first at {int(torch.nonzero(bad)[0])}"
        return
    rows = out[R.GUARD:R.GUARD + B * case.ldy].view(B, case.ldy)
    assert bool((out[:R.GUARD] == R.FILL).all()) and bool((out[R.GUARD + B * case.ldy:] == R.FILL).all()) and bool((rows[:, case.n_out:] == R.FILL).all()), \
        f"{case.id}: guard band or row padding written"
    assert_close(rows[:, :case.n_out], case.reference(), dt, case.id)


def test_gemv_mxfp4_batched_refusals():
    """refused before any launch, y untouched: an fp32 engine, null operands, B outside 1 .. 8, N < 1, K or ldw not a multiple of 32,
    ldw < K, ldx < K, SwiGLU with N not a multiple of 64"""
    dt = torch.bfloat16
    m, m32 = engine(dt), engine(torch.float32)
    K, N, B = 256, 64, 4
    q4 = torch.zeros((N, (K + 64) // 2), dtype=torch.uint8, device="cuda")
    e8 = torch.full((N, (K + 64) // 32), 127, dtype=torch.uint8, device="cuda")
    x = torch.ones((8, K + 16), dtype=dt, device="cuda")
    y = torch.full((8, N), R.FILL, dtype=dt, device="cuda")
    torch.cuda.synchronize()

    def call(eng=m, q4=q4, e8=e8, ldw=K + 64, x=x, ldx=K + 16, y=y, N=N, K=K, epi=_lib.EPI_NONE, B=B):
        return eng._lib.svln_op_gemv_mxfp4_batched(eng._h, ptr(q4), ptr(e8), ldw, ptr(x), ldx, None, None, 0, ptr(y), N, N, K, epi, B, None)

    bad = [call(eng=m32), call(q4=None), call(e8=None), call(x=None), call(y=None), call(B=0), call(B=9), call(B=-1), call(N=0), call(N=-3),
           call(K=K - 16), call(K=0), call(ldw=K + 16), call(ldw=K - 32), call(ldx=K - 8), call(epi=_lib.EPI_SWIGLU, N=32),
           call(epi=_lib.EPI_GELU_ERF)]
    assert all(rc != 0 for rc in bad), bad
    torch.cuda.synchronize()
    assert bool((y == R.FILL).all())                                              # nothing was launched
    assert call() == 0 and call(ldw=K) == 0 and call(epi=_lib.EPI_SWIGLU) == 0 and call(B=8) == 0 and call(B=1) == 0
    torch.cuda.synchronize()
    assert bool((y[:, :N] == 0).all())                                            # zero codes: the product ran and stored zeros
