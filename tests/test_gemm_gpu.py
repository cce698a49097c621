"""The MFMA GEMMs (gemm.hip: gemm_glds_kernel over its tile configurations, the 8-phase schedule, the slab reduces, the tail-tile launch)
through svln_op_gemm / _gemm_norm / _gemm_norm_q8 / _gemm_fp8 on the cases of tests/gemm_ref.py: inputs on which a subtly wrong kernel fails
(tests/test_gemm_inputs.py proves that on the CPU).

  exact cases      signed powers of two with per-row exponents: product + bias + residual is defined bit for bit -> the stored bits.
  toleranced cases GELU / SwiGLU over the same exact accumulators, and the norm of the fused reduce (from the stored rows): float64
                   reference, util.assert_close.
lda, ldw > K with poison in the padding; C sits between guard rows with ldc > n_out, all filled with a sentinel that must survive; before a
K-split case a larger product leaves the fp32 slabs dirty; every launch runs twice on a refilled output and must give the same bits."""
import ctypes as C

import pytest
import torch

import gemm_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import assert_close, ptr

pytestmark = pytest.mark.gpu
EPI = {"none": _lib.EPI_NONE, "gelu_tanh": _lib.EPI_GELU_TANH, "gelu_erf": _lib.EPI_GELU_ERF, "swiglu": _lib.EPI_SWIGLU}
GUARD_ROWS, GUARD = 4, 64
_engines, _dirt = {}, {}


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _dirty_slabs(m, dtype):
    """16 K slices of a 256 x 4096 product of constants: every fp32 slab element a split case can use holds 8192 or 16384 afterwards"""
    K = 128 * R.EPC["bf16" if dtype == torch.bfloat16 else "fp32"]
    if dtype not in _dirt:
        _dirt[dtype] = (torch.full((256, K), 16.0, dtype=dtype, device="cuda"), torch.full((4096, K), 16.0, dtype=dtype, device="cuda"),
                        torch.empty((256, 4096), dtype=dtype, device="cuda"))
    A, W, out = _dirt[dtype]
    _lib.check(m._lib.svln_op_gemm(m._h, ptr(A), K, ptr(W), K, ptr(out), 4096, None, None, 0, 0, 256, 4096, K, _lib.EPI_NONE, 0, 16))


def _launch(m, c, d, Cp, res, ldr, Y, q8, q8s):
    fused = C.c_int32(-1)
    if c.entry == "fp8":
        rc = m._lib.svln_op_gemm_fp8(m._h, ptr(d["A"]), ptr(d["sa"]), c.lda, ptr(d["W"]), ptr(d["sw"]), c.ldw, Cp, c.ldc, ptr(d["bias"]), res, ldr,
                                     c.M, c.N, c.K, EPI[c.epi], c.force_cfg, c.force_split)
    elif c.entry == "norm":
        rc = m._lib.svln_op_gemm_norm(m._h, ptr(d["A"]), c.lda, ptr(d["W"]), c.ldw, Cp, c.ldc, ptr(d["bias"]), res, ldr, ptr(d["g"]), ptr(d["nb"]), ptr(Y),
                                      R.EPS, c.M, c.N, c.K, c.force_split, C.byref(fused))
    elif c.entry == "q8":
        rc = m._lib.svln_op_gemm_norm_q8(m._h, ptr(d["A"]), c.lda, ptr(d["W"]), c.ldw, Cp, c.ldc, res, ldr, ptr(d["g"]), ptr(Y), R.EPS, c.M, c.N, c.K,
                                         c.force_split, ptr(q8), ptr(q8s), C.byref(fused))
    else:
        rc = m._lib.svln_op_gemm(m._h, ptr(d["A"]), c.lda, ptr(d["W"]), c.ldw, Cp, c.ldc, ptr(d["bias"]), res, ldr, c.res_mod, c.M, c.N, c.K, EPI[c.epi],
                                 c.force_cfg, c.force_split)
    _lib.check(rc)
    torch.cuda.synchronize()
    return fused.value


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_gemm_cases(case):
    c = case.build()
    dt, M, N, n_out, ldc = c.dtype, c.M, c.N, c.n_out, c.ldc
    m = engine(dt)
    dev = lambda t: None if t is None else t.to(dt).cuda()
    d = {"A": c.Abuf.cuda(), "W": c.Wbuf.cuda(), "sa": c.a_scale.float().cuda(), "sw": c.w_scale.float().cuda(), "bias": dev(c.bias), "g": dev(c.g), "nb": dev(c.nb)}
    res_rows = None
    if c.res is not None:
        res_rows = torch.full((c.res.shape[0], c.ldr), R.POISON, dtype=torch.float64)
        res_rows[:, :N] = c.res
        res_rows = res_rows.to(dt)
    rows = GUARD_ROWS * 2 + M

    def run():
        buf = torch.full((rows, ldc), R.FILL, dtype=dt)
        if c.inplace:
            buf[GUARD_ROWS:GUARD_ROWS + M, :N] = c.res.to(dt)
        buf = buf.cuda()
        Cp = C.c_void_p(buf.data_ptr() + GUARD_ROWS * ldc * buf.element_size())
        res_dev = None if res_rows is None or c.inplace else res_rows.cuda()       # (held until the launch is over)
        res, ldr = (Cp, ldc) if c.inplace else (ptr(res_dev), c.ldr) if res_dev is not None else (None, 0)
        Y = torch.full((GUARD + M * N + GUARD,), R.FILL, dtype=dt, device="cuda") if c.norm else None
        q8 = torch.full((GUARD + M * N + GUARD,), 0x55, dtype=torch.uint8, device="cuda") if c.q8 else None
        q8s = torch.full((GUARD + M + GUARD,), R.FILL, dtype=torch.float32, device="cuda") if c.q8 else None
        torch.cuda.synchronize()
        if c.split_S > 1:
            _dirty_slabs(m, dt)
        fused = _launch(m, c, d, Cp, res, ldr, None if Y is None else Y[GUARD:], None if q8 is None else q8[GUARD:], None if q8s is None else q8s[GUARD:])
        return buf.cpu(), fused, *(None if t is None else t.cpu() for t in (Y, q8, q8s))

    out, fused, Y, q8, q8s = run()
    again = run()
    body = out[GUARD_ROWS:GUARD_ROWS + M]
    assert bool((out[:GUARD_ROWS] == R.FILL).all()) and bool((out[GUARD_ROWS + M:] == R.FILL).all()), f"{c.id}: guard rows written"
    assert bool((body[:, n_out:] == R.FILL).all()), f"{c.id}: ldc padding written"
    assert torch.equal(_bits(out), _bits(again[0])), f"{c.id}: two launches differ in {int((_bits(out) != _bits(again[0])).sum())} outputs"
    got = body[:, :n_out]
    ref = c.reference()
    if c.exact:
        exp = ref.to(dt)
        bad = _bits(got) != _bits(exp)
        if bool(bad.any()):
            at = torch.nonzero(bad)
            tiles = sorted({(int(i) // c.BM, int(j) // c.BN) for i, j in at.tolist()})
            i, j = at[0].tolist()
            raise AssertionError(f"{c.id}: {int(bad.sum())} of {bad.numel()} outputs differ in their bits; first ({i}, {j}) got {float(got[i, j])} expected "
                                 f"{float(exp[i, j])}; (row, column) tiles of {c.BM} x {c.BN}: {tiles[:12]}{' ...' if len(tiles) > 12 else ''}")
    else:
        assert_close(got, ref, dt, c.id)
    if c.norm:
        assert fused == 1, f"{c.id}: the reduce did not emit the norm"
        assert fused == int(c.geom["fused"]), f"{c.id}: the launch reports fused = {fused}, the plan {c.geom['fused']}"
        assert bool((Y[:GUARD] == R.FILL).all()) and bool((Y[GUARD + M * N:] == R.FILL).all()), f"{c.id}: guard band of norm_out written"
        assert torch.equal(_bits(Y), _bits(again[2])), f"{c.id}: two launches differ in norm_out"
        y = Y[GUARD:GUARD + M * N].view(M, N)
        assert_close(y, c.norm_reference(got), dt, c.id + " norm")
        if c.q8:
            assert bool((q8[:GUARD] == 0x55).all()) and bool((q8[GUARD + M * N:] == 0x55).all()) and bool((q8s[:GUARD] == R.FILL).all()) and \
                bool((q8s[GUARD + M:] == R.FILL).all()), f"{c.id}: guard band of the e4m3 copy written"
            # the e4m3 copy of the stored norm rows: scale = max |y| / 448 in fp32, values within half an e4m3 step (2^-4 relative, 2^-10 of
            # the scale below the normal range; twice that is allowed for the fp32 reciprocal)
            s = q8s[GUARD:GUARD + M]
            assert torch.equal(s, y.float().abs().amax(1) / 448.0), c.id + " e4m3 scale"
            deq = q8[GUARD:GUARD + M * N].view(torch.float8_e4m3fn).float().view(M, N) * s[:, None]
            assert bool(((deq - y.float()).abs() <= 2.0 ** -4 * y.float().abs() + 2.0 ** -9 * s[:, None]).all()), c.id + " e4m3 copy"


@pytest.mark.parametrize("entry", ["gemm", "norm", "q8", "fp8"])
def test_gemm_refusals(entry):
    """every svln_op_gemm* entry point refuses, with a message and before any launch: null A / W / C, negative extents, K or a row stride off
    the 16-byte chunk grid, lda / ldw below K, ldc below the output width, a residual with ldr below N, a negative res_mod, SwiGLU over
    N % 64 != 0 and an epilogue launch_gemm does not know (EPI_ARGMAX included)."""
    dt = torch.bfloat16 if entry in ("q8", "fp8") else torch.float32
    m = engine(dt)
    epc = 16 if entry == "fp8" else R.EPC["bf16" if dt == torch.bfloat16 else "fp32"]
    M, N, K = 16, 128, 8 * epc
    A = torch.zeros((M, K + 4 * epc), dtype=torch.uint8 if entry == "fp8" else dt, device="cuda")
    W = torch.zeros((N, K + 4 * epc), dtype=torch.uint8 if entry == "fp8" else dt, device="cuda")
    Cm = torch.full((M + 1, N + 8), 5.0, dtype=dt, device="cuda")
    res, g = torch.zeros((M, N + 8), dtype=dt, device="cuda"), torch.ones((N,), dtype=dt, device="cuda")
    Y, q8, q8s = torch.zeros((M, N), dtype=dt, device="cuda"), torch.zeros((M, N), dtype=torch.uint8, device="cuda"), torch.zeros((M,), device="cuda")
    sa, sw = torch.ones((M,), device="cuda"), torch.ones((N,), device="cuda")
    torch.cuda.synchronize()

    def call(A=A, W=W, Cm=Cm, lda=K, ldw=K, ldc=N, res=None, ldr=0, res_mod=0, M=M, N=N, K=K, epi=_lib.EPI_NONE, split=0):
        h, lib = m._h, m._lib
        if entry == "fp8":
            return lib.svln_op_gemm_fp8(h, ptr(A), ptr(sa), lda, ptr(W), ptr(sw), ldw, ptr(Cm), ldc, None, ptr(res), ldr, M, N, K, epi, 0, split)
        if entry == "norm":
            return lib.svln_op_gemm_norm(h, ptr(A), lda, ptr(W), ldw, ptr(Cm), ldc, None, ptr(res), ldr, ptr(g), None, ptr(Y), R.EPS, M, N, K, split, None)
        if entry == "q8":
            return lib.svln_op_gemm_norm_q8(h, ptr(A), lda, ptr(W), ldw, ptr(Cm), ldc, ptr(res), ldr, ptr(g), ptr(Y), R.EPS, M, N, K, split, ptr(q8), ptr(q8s), None)
        return lib.svln_op_gemm(h, ptr(A), lda, ptr(W), ldw, ptr(Cm), ldc, None, ptr(res), ldr, res_mod, M, N, K, epi, 0, split)

    def refused(**kw):
        rc = call(**kw)
        return rc != 0 and len(m._lib.svln_last_error()) > 0

    assert call() == 0 and call(lda=K + 4 * epc, ldw=K + 2 * epc, ldc=N + 8, res=res, ldr=N + 8) == 0
    Cm.fill_(5.0)
    torch.cuda.synchronize()
    assert refused(A=None) and refused(W=None) and refused(Cm=None)
    assert refused(M=-1) and refused(N=-4) and refused(K=-epc)
    assert refused(K=K - epc // 2) and refused(K=K + 1, lda=K + 4 * epc, ldw=K + 4 * epc)
    assert refused(lda=K - epc) and refused(ldw=K - epc) and refused(lda=K + epc // 2) and refused(ldw=K + epc // 2)
    assert refused(ldc=N - 1)
    assert refused(res=res, ldr=N - 1)
    if entry == "gemm":
        assert refused(res=res, ldr=N, res_mod=-3)
    if entry in ("gemm", "fp8"):
        assert refused(epi=_lib.EPI_SWIGLU, N=N - 32, ldc=N) and call(epi=_lib.EPI_SWIGLU) == 0
        assert refused(epi=_lib.EPI_ARGMAX) and refused(epi=5) and refused(epi=-1)
        Cm.fill_(5.0)
    torch.cuda.synchronize()
    assert bool((Cm == 5.0).all()), "a refused call wrote C"
