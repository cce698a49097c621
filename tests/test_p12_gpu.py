"""The lossless 12-bit weight packing on the GPU (gemv.hip: WP12, p12_pack_rows_kernel) through svln_op_pack_rows, svln_op_unpack_rows and
svln_op_gemv_packed, on the inputs of tests/p12_ref.py (tests/test_p12_inputs.py proves them sharp on the CPU).

  encoder   equals the numpy restatement byte for byte (packed blocks, records, fallback count)
  decoder   gives back the input bits, on every bf16 pattern and on the designed rows
  GEMV      bit-equal to svln_op_gemv ON THE SAME ARGUMENTS (the decoded value is the original bit pattern and the lane -> chunk
            assignment is the bf16 policy's: same fmaf chain), every epilogue, fallback pattern and K geometry
  refusals  before any launch"""
import ctypes as C

import numpy as np
import pytest
import torch

import p12_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
EPI = {"none": _lib.EPI_NONE, "swiglu": _lib.EPI_SWIGLU, "argmax": _lib.EPI_ARGMAX}
GUARD, FILL = 64, 777.0
_engines = {}


def engine(dtype=torch.bfloat16):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def gpu_pack(m, bits, ld=None):
    """svln_op_pack_rows on bits [N][K] (row stride ld, the padding poisoned) -> packed, records (uint8, cpu), fallback count, device tensors"""
    N, K = bits.shape
    ld = ld or K
    w = torch.full((N, ld), 2.0 ** 60, dtype=torch.bfloat16)
    w[:, :K] = R.bf16_of(bits)
    dw = w.cuda()
    packed = torch.full((N * R.row_bytes(K) + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    rec = torch.full((N * 16 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    n_fb = C.c_int64(-1)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_pack_rows(m._h, ptr(dw), ld, N, K, ptr(packed), ptr(rec), C.byref(n_fb)))
    assert bool((packed[N * R.row_bytes(K):] == 0xAB).all()) and bool((rec[N * 16:] == 0xAB).all()), "guard band written"
    return packed[:N * R.row_bytes(K)].cpu().numpy().reshape(N, -1), rec[:N * 16].cpu().numpy().reshape(N, 16), n_fb.value, (dw, packed, rec)


def gpu_unpack(m, dev, N, K, ld):
    dw, packed, rec = dev
    out = torch.full((N * K + GUARD,), FILL, dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_unpack_rows(m._h, ptr(packed), ptr(rec), ptr(dw), ld, N, K, ptr(out)))
    assert bool((out[N * K:] == FILL).all()), "guard band written"
    return R.bits_of(out[:N * K].cpu()).reshape(N, K)


def _pack_inputs():
    out = {"all_patterns": np.arange(65536, dtype=np.uint16).reshape(128, 512)}
    for name, (bits, _, _) in R.designed_rows().items():
        out[name] = bits
    out["gaussian_3584"] = R.gaussian_bits(37, 3584, 3)
    out["ragged_131_chunks"] = R.designed_bits(5, 1048, "last", 4)
    out["one_chunk"] = R.gaussian_bits(3, 8, 5)
    out["specials"] = R.special_bits(9, 1048, 6)
    return out


@pytest.mark.parametrize("name", list(_pack_inputs()))
def test_pack_equals_the_restatement_and_unpack_the_input(name):
    bits = _pack_inputs()[name]
    m = engine()
    N, K = bits.shape
    for ld in (K, K + 64):
        packed, rec, n_fb, dev = gpu_pack(m, bits, ld)
        ep, er, ef = R.encode(bits)
        assert np.array_equal(rec, er), (name, ld, np.nonzero((rec != er).any(1))[0][:4])
        assert np.array_equal(packed, ep), (name, ld, np.argwhere(packed != ep)[:4])
        assert n_fb == ef
        assert np.array_equal(gpu_unpack(m, dev, N, K, ld), bits), (name, ld)


def _gemv(m, case, dev, packed_form, x, g, b, r):
    dw, packed, rec = dev
    buf = torch.full((case.n_out + 2 * GUARD,), FILL, dtype=torch.bfloat16, device="cuda")
    y = None if case.epi == "argmax" else buf[GUARD:GUARD + case.n_out]
    tok = C.c_int32(-7)
    tail = (ptr(dw), case.K + case.pad, ptr(x), ptr(g), 1e-6, ptr(b), ptr(r), ptr(y), case.N, case.K, EPI[case.epi], C.byref(tok))
    torch.cuda.synchronize()
    if packed_form:
        _lib.check(m._lib.svln_op_gemv_packed(m._h, ptr(packed), ptr(rec), *tail))
    else:
        _lib.check(m._lib.svln_op_gemv(m._h, *tail))
    out = buf.cpu()
    assert bool((out[:GUARD] == FILL).all()) and bool((out[GUARD + case.n_out:] == FILL).all()), f"{case.id}: guard band written"
    return tok.value, R.bits_of(out[GUARD:GUARD + case.n_out])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_packed_gemv_is_bit_equal_to_the_bf16_gemv(case):
    case.build()
    m = engine()
    packed, rec, n_fb, dev = gpu_pack(m, case.w, case.K + case.pad)
    assert np.array_equal(packed, case.packed) and np.array_equal(rec, case.rec) and n_fb == case.n_fb
    dv = lambda t: None if t is None else t.cuda()
    args = (dv(case.x), dv(case.g), dv(case.b), dv(case.r))
    tok_p, out_p = _gemv(m, case, dev, True, *args)
    tok_b, out_b = _gemv(m, case, dev, False, *args)
    if case.epi == "argmax":
        assert tok_p == tok_b == min(case.ties), (case.id, tok_p, tok_b)
        return
    bad = out_p != out_b
    assert not bad.any(), f"{case.id}: {int(bad.sum())} of {bad.size} outputs differ in their bits, first at {int(np.nonzero(bad)[0][0])}"
    if case.special:
        assert np.isnan(R.f32_of(out_p)).any()           # the NaNs really went through


@pytest.mark.parametrize("form", ["scored", "sampled"])
def test_scored_and_sampled_heads(form):
    """fmt 3 of the test heads (W = the bf16 original, aux = packed rows then records) against fmt 0: token and log-probability bits"""
    N, K = 1003, 1048
    m = engine()
    bits = R.designed_bits(N, K, "first", 31)
    packed, rec, _, (dw, dp, dr) = gpu_pack(m, bits)
    aux = torch.cat([dp[:N * R.row_bytes(K)], dr[:N * 16]]).contiguous()
    x = torch.randn((K,), generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).cuda()
    flags = torch.zeros((N,), dtype=torch.uint8, device="cuda")
    flags[::7] = 1
    got = []
    for fmt, W, a in ((0, dw, None), (3, dw, aux)):
        tok, lp = C.c_int32(-7), C.c_float(-7.0)
        torch.cuda.synchronize()
        if form == "scored":
            _lib.check(m._lib.svln_op_gemv_argmax_scores(m._h, fmt, ptr(W), ptr(a), K, ptr(x), N, K, ptr(flags), 1.3, C.byref(tok), C.byref(lp)))
        else:
            _lib.check(m._lib.svln_op_gemv_argmax_sample(m._h, fmt, ptr(W), ptr(a), K, ptr(x), N, K, ptr(flags), 1.3, 0.8, 1234, 0, 5, C.byref(tok),
                                                         C.byref(lp)))
        got.append((tok.value, np.float32(lp.value).view(np.uint32)))
    assert got[0] == got[1] and 0 <= got[0][0] < N, got


def test_refusals_before_any_launch():
    m = engine()
    N, K = 8, 512
    bits = R.designed_bits(N, K, "none", 1)
    _, _, _, (dw, dp, dr) = gpu_pack(m, bits)
    x = torch.ones((K,), dtype=torch.bfloat16, device="cuda")
    y = torch.full((N + GUARD,), FILL, dtype=torch.bfloat16, device="cuda")
    big = torch.zeros((40000,), dtype=torch.bfloat16, device="cuda")
    tok = C.c_int32()
    L, h = m._lib, m._h

    def gemv(packed, rec, W, ldw, k, eng=h):
        return L.svln_op_gemv_packed(eng, ptr(packed), ptr(rec), ptr(W), ldw, ptr(x), None, 1e-6, None, None, ptr(y), N, k, _lib.EPI_NONE, C.byref(tok))

    assert gemv(dp, dr, dw, K, K) == 0
    y.fill_(FILL)
    torch.cuda.synchronize()
    assert gemv(dp, dr, dw, K, K - 4) != 0 and b"multiple" in L.svln_last_error()
    assert gemv(dp, dr, big, 32776, 32776) != 0 and b"32768" in L.svln_last_error()
    for args in ((None, dr, dw), (dp, None, dw), (dp, dr, None)):
        assert gemv(*args, K, K) != 0 and b"null" in L.svln_last_error()
    n_fb = C.c_int64()
    assert L.svln_op_pack_rows(h, ptr(dw), K, N, K - 4, ptr(dp), ptr(dr), C.byref(n_fb)) != 0 and b"multiple" in L.svln_last_error()
    assert L.svln_op_pack_rows(h, ptr(big), 32776, 1, 32776, ptr(dp), ptr(dr), C.byref(n_fb)) != 0 and b"32768" in L.svln_last_error()
    assert L.svln_op_pack_rows(h, None, K, N, K, ptr(dp), ptr(dr), C.byref(n_fb)) != 0 and b"null" in L.svln_last_error()
    assert L.svln_op_pack_rows(h, ptr(dw), K - 8, N, K, ptr(dp), ptr(dr), C.byref(n_fb)) != 0
    assert L.svln_op_unpack_rows(h, ptr(dp), None, ptr(dw), K, N, K, ptr(y)) != 0 and b"null" in L.svln_last_error()
    # the fp32 engine has no packed form
    f = engine(torch.float32)
    assert gemv(dp, dr, dw, K, K, f._h) != 0 and b"bf16" in L.svln_last_error()
    assert L.svln_op_pack_rows(f._h, ptr(dw), K, N, K, ptr(dp), ptr(dr), C.byref(n_fb)) != 0 and b"bf16" in L.svln_last_error()
    assert L.svln_op_unpack_rows(f._h, ptr(dp), ptr(dr), ptr(dw), K, N, K, ptr(y)) != 0 and b"bf16" in L.svln_last_error()
    assert L.svln_set_packed_decode(f._h, 1) != 0 and b"bf16" in L.svln_last_error() and L.svln_set_packed_decode(f._h, 0) == 0
    assert bool((y == FILL).all()), "a refused call wrote its output"
