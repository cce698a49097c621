"""The row helpers of misc.hip (rmsnorm_kernel with its hidden tap and skip word, rmsnorm_indexed_kernel, layernorm_kernel,
gather_rows_kernel, gather_rows_ragged_kernel, frame_hash_kernel, mem_*_kernel, pool_kernel, patchify_kernel) through their operator entry
points, on the cases of tests/rows_ref.py: inputs on which a subtly wrong kernel fails (tests/test_rows_inputs.py proves that on the CPU).

  exact families      gathers, taps, patchify, the frame hash, the prune selection: compared bit for bit / for equality.
  toleranced families the norms, the prune scores, pool: float64 reference, the bound derived in rows_ref.py; every test prints its worst
                      error over bound.
Outputs sit between NaN canary rows that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import rows_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
_engines = {}
NAN = float("nan")


def engine(dtype):
    if dtype not in _engines:
        assert (TINY.hidden, TINY.v_hidden, TINY.vocab) == (R.HIDDEN, 144, R.VOCAB)
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=9, max_positions=2048)
    return _engines[dtype]


def i32(values):
    return (C.c_int32 * max(len(values), 1))(*[int(v) for v in values])


def dev(a, dtype):
    return R.to_t(a, dtype).cuda()


def canaried(rows, n, dtype):
    """(whole buffer of NaN, its rows 1 .. rows): one canary row before and one after"""
    buf = torch.full((rows + 2, n), NAN, dtype=dtype, device="cuda")
    return buf, buf[1:rows + 1]


def untouched(t):
    """rows that still hold the NaN fill, bit for bit"""
    fill = R.bits(torch.full((1,), NAN, dtype=t.dtype))[0]
    return (R.bits(t.cpu()) == fill).all(-1)


def within(got, ref, bound, what):
    err = np.abs(got.double().cpu().numpy() - ref)
    with np.errstate(all="ignore"):
        ratio = float(np.nanmax(err / bound))
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert np.isfinite(err).all() and (err <= bound).all(), f"{what}: worst error / bound {ratio:.3f}, {int((err > bound).sum())} of {err.size} outside"


def plain_rmsnorm(m, dx, dg, rows, n):
    y = torch.full((rows, n), NAN, dtype=dx.dtype, device="cuda")
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_rmsnorm(m._h, ptr(dx), ptr(dg), ptr(y), rows, n, R.EPS))
    return y.cpu()


# ---------------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("case", R.NORM_CASES, ids=lambda c: c.id)
def test_norm(case):
    case.build()
    dt, rows, n = case.dtype, case.rows, case.n
    m = engine(dt)
    dx, dg, db = dev(case.x, dt), dev(case.g, dt), dev(case.b, dt)
    buf, y = canaried(rows, n, dt)
    torch.cuda.synchronize()
    if case.op == "rms":
        _lib.check(m._lib.svln_op_rmsnorm(m._h, ptr(dx), ptr(dg), ptr(y), rows, n, R.EPS))
    else:
        _lib.check(m._lib.svln_op_layernorm(m._h, ptr(dx), ptr(dg), ptr(db), ptr(y), rows, n, R.EPS))
    assert bool(untouched(buf[[0, rows + 1]]).all()), f"{case.id}: canary row written"
    within(buf[1:rows + 1], case.reference(), case.bound(), case.id)


@pytest.mark.parametrize("case", R.TAP_CASES, ids=lambda c: c.id)
def test_rmsnorm_tap(case):
    """the launch of a graph-replayed decode step: device skip word, second copy at the device row *y2_row + r clamped to y2_cap - 1"""
    dt, rows, n, cap = case.dtype, case.rows, case.n, case.y2_cap
    m = engine(dt)
    src = R.tap_input(dt, n)
    dx, dg = dev(src.x[:rows], dt), dev(src.g, dt)
    plain = plain_rmsnorm(m, dx, dg, rows, n)
    ybuf, y = canaried(rows, n, dt)
    tbuf, tap = canaried(cap, n, dt)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_rmsnorm_tap(m._h, ptr(dx), ptr(dg), ptr(y), rows, n, R.EPS, case.skip, ptr(tap), case.y2_row, cap))
    written, tmap = case.maps()
    ycpu, tcpu = ybuf.cpu(), tbuf.cpu()
    assert bool(untouched(ycpu[[0, rows + 1]]).all()) and bool(untouched(tcpu[[0, cap + 1]]).all()), f"{case.id}: canary row written"
    if written:
        assert torch.equal(R.bits(ycpu[1:rows + 1]), R.bits(plain)), f"{case.id}: y differs from svln_op_rmsnorm on the same rows"
    else:
        assert bool(untouched(ycpu).all()), f"{case.id}: y written under skip"
    for t in range(cap):
        if tmap[t] < 0:
            assert bool(untouched(tcpu[1 + t])), f"{case.id}: tap row {t} written"
        else:
            assert torch.equal(R.bits(tcpu[1 + t]), R.bits(plain[tmap[t]])), f"{case.id}: tap row {t} is not y row {tmap[t]}"


@pytest.mark.parametrize("case", R.INDEXED_CASES, ids=lambda c: c.id)
def test_rmsnorm_indexed(case):
    """row r of y is bit-equal to what svln_op_rmsnorm stores for row src_rows[r] (the kernel comment's promise); the tap rows to y's"""
    dt, rows, n, cap = case.dtype, case.rows, case.n, case.tap_cap
    m = engine(dt)
    src = R.tap_input(dt, n, case.x_rows)
    dx, dg = dev(src.x, dt), dev(src.g, dt)
    plain = plain_rmsnorm(m, dx, dg, case.x_rows, n)
    within(plain, src.reference(), src.bound(), case.id + " (plain rows)")
    ybuf, y = canaried(rows, n, dt)
    tbuf, tap = canaried(cap, n, dt)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_rmsnorm_indexed(m._h, ptr(dx), case.x_rows, ptr(dg), ptr(y), i32(case.src), i32(case.tap_rows), ptr(tap), cap, rows, n, R.EPS))
    ymap, tmap = case.maps()
    ycpu, tcpu = ybuf.cpu(), tbuf.cpu()
    assert bool(untouched(ycpu[[0, rows + 1]]).all()) and bool(untouched(tcpu[[0, cap + 1]]).all()), f"{case.id}: canary row written"
    for r in range(rows):
        assert torch.equal(R.bits(ycpu[1 + r]), R.bits(plain[ymap[r]])), f"{case.id}: y row {r} is not the norm of x row {ymap[r]}"
    for t in range(cap):
        if tmap[t] < 0:
            assert bool(untouched(tcpu[1 + t])), f"{case.id}: tap row {t} written"
        else:
            assert torch.equal(R.bits(tcpu[1 + t]), R.bits(ycpu[1 + tmap[t]])), f"{case.id}: tap row {t} is not y row {tmap[t]}"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_norm_refusals(dtype):
    """the norm operators refuse, before anything is launched: null pointers, rows < 0, n <= 0 and an n that is not a multiple of the 16-byte
    chunk (n / EPC would drop the tail of every row and return status 0); the list forms also refuse entries outside their buffers"""
    m = engine(dtype)
    epc, n, rows = R.EPC[dtype], 64, 3
    x = torch.zeros((rows, n), dtype=dtype, device="cuda")
    g = torch.ones((n,), dtype=dtype, device="cuda")
    y = torch.zeros((rows, n), dtype=dtype, device="cuda")
    tap = torch.zeros((4, n), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    L = m._lib

    def refused(rc, text):
        assert rc != 0 and text in L.svln_last_error(), (rc, L.svln_last_error())

    rms = lambda x=x, g=g, y=y, rows=rows, n=n: L.svln_op_rmsnorm(m._h, ptr(x), ptr(g), ptr(y), rows, n, R.EPS)
    ln = lambda x=x, g=g, b=g, y=y, rows=rows, n=n: L.svln_op_layernorm(m._h, ptr(x), ptr(g), ptr(b), ptr(y), rows, n, R.EPS)
    tp = lambda x=x, y=y, y2=tap, rows=1, n=n, row=0, cap=4: L.svln_op_rmsnorm_tap(m._h, ptr(x), ptr(g), ptr(y), rows, n, R.EPS, 0, ptr(y2), row, cap)
    ix = lambda x=x, src=(2, 0), taps=(-1, 3), tap=tap, n=n, x_rows=rows, cap=4: \
        L.svln_op_rmsnorm_indexed(m._h, ptr(x), x_rows, ptr(g), ptr(y), i32(src), i32(taps), ptr(tap), cap, len(src), n, R.EPS)
    assert rms() == 0 and ln() == 0 and tp() == 0 and ix() == 0 and rms(rows=0) == 0 and ln(rows=0) == 0
    for call in (rms, ln, tp, ix):
        refused(call(x=None), b"null pointer")
        refused(call(n=n - epc // 2), b"multiple of the 16-byte chunk")
        refused(call(n=0), b"multiple of the 16-byte chunk")
    for call in (rms, ln):
        refused(call(g=None), b"null pointer")
        refused(call(y=None), b"null pointer")
        refused(call(rows=-1), b"rows must be >= 0")
    refused(ln(b=None), b"null pointer")
    refused(tp(y2=None), b"null pointer")
    refused(tp(cap=0), b"y2_cap")
    refused(tp(row=-1), b"y2_cap")
    refused(ix(src=(3, 0)), b"src_rows entry out of range")
    refused(ix(src=(-1, 0)), b"src_rows entry out of range")
    refused(ix(taps=(-1, 4)), b"tap_rows entry out of range")
    refused(ix(taps=(-2, 0)), b"tap_rows entry out of range")
    refused(ix(tap=None), b"null pointer")
    refused(tp(rows=-1), b"rows must be >= 0")
    refused(L.svln_op_rmsnorm_indexed(m._h, ptr(x), rows, ptr(g), ptr(y), i32(()), i32(()), ptr(tap), 4, -1, n, R.EPS), b"rows must be >= 0")
    refused(ix(x_rows=0), b"x_rows and tap_cap >= 1")
    refused(ix(cap=0), b"x_rows and tap_cap >= 1")


# ---------------------------------------------------------------------------------------------------------- gathers
_tables = {}


def tables(dtype):
    if dtype not in _tables:
        embed, feats = R.tables(dtype)
        _tables[dtype] = (embed, feats, dev(embed, dtype), dev(feats, dtype))
    return _tables[dtype]


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=lambda c: c.id)
def test_gather_rows(case):
    dt, rows, n = case.dtype, case.rows, R.GATHER_N
    m = engine(dt)
    embed, feats, de, df = tables(dt)
    buf, out = canaried(rows, n, dt)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gather_rows(m._h, i32(case.src), rows, ptr(de), R.VOCAB, ptr(df), R.FEAT_ROWS, ptr(out), n, case.skip))
    got = buf.cpu()
    ref = case.reference(embed, feats)
    if ref is None:
        assert bool(untouched(got).all()), f"{case.id}: out written under skip"
        return
    assert bool(untouched(got[[0, rows + 1]]).all()), f"{case.id}: canary row written"
    bad = (R.bits(got[1:rows + 1]) != R.bits(R.to_t(ref, dt))).any(1)
    assert not bool(bad.any()), f"{case.id}: {int(bad.sum())} of {rows} rows differ, first at {int(torch.nonzero(bad)[0])} (src {int(case.src[int(torch.nonzero(bad)[0])])})"


@pytest.mark.parametrize("case", R.RAGGED_CASES, ids=lambda c: c.id)
def test_gather_rows_ragged(case):
    dt, n, out_rows = case.dtype, R.GATHER_N, case.OUT_ROWS
    m = engine(dt)
    embed, _, de, _ = tables(dt)
    buf, out = canaried(out_rows, n, dt)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gather_rows_ragged(m._h, i32([v for p in case.pairs for v in p]), case.rows, ptr(de), R.VOCAB, ptr(out), out_rows, n))
    got = buf.cpu()
    ref = case.reference(embed)
    for d in range(-1, out_rows + 1):
        if d in ref:
            assert torch.equal(R.bits(got[1 + d]), R.bits(R.to_t(embed[ref[d]], dt))), f"{case.id}: row {d} is not embed row {ref[d]}"
        else:
            assert bool(untouched(got[1 + d])), f"{case.id}: row {d} written"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_gather_and_hash_refusals(dtype):
    m = engine(dtype)
    L, n = m._lib, R.GATHER_N
    _, _, de, df = tables(dtype)
    buf, out = canaried(4, n, dtype)
    words = torch.zeros((2, 100), dtype=torch.int32, device="cuda")
    keys = (C.c_uint64 * 4)()
    torch.cuda.synchronize()

    def refused(rc, text):
        assert rc != 0 and text in L.svln_last_error(), (rc, L.svln_last_error())

    ga = lambda src=(0, -1), e=de, f=df, o=out, n=n, rows=None, er=R.VOCAB, fr=R.FEAT_ROWS: \
        L.svln_op_gather_rows(m._h, i32(src), len(src) if rows is None else rows, ptr(e), er, ptr(f), fr, ptr(o), n, 0)
    rg = lambda lst=(3, 7, 0, 9), e=de, o=out, n=n, rows=None, er=R.VOCAB, orows=4: \
        L.svln_op_gather_rows_ragged(m._h, i32(lst), len(lst) // 2 if rows is None else rows, ptr(e), er, ptr(o), orows, n)
    fh = lambda p=words, F=2, w=100, k=keys: L.svln_op_frame_hash(m._h, ptr(p), F, w, k)
    assert ga() == 0 and rg() == 0 and fh() == 0
    refused(ga(src=(0, R.VOCAB)), b"src entry out of range")
    refused(ga(src=(-R.FEAT_ROWS - 1,)), b"src entry out of range")
    refused(ga(e=None), b"null pointer")
    refused(ga(f=None), b"null pointer")
    refused(ga(o=None), b"null pointer")
    refused(ga(n=n + 1), b"multiple of the 16-byte chunk")
    refused(rg(lst=(4, 7)), b"destination row out of range")
    refused(rg(lst=(-1, 7)), b"destination row out of range")
    refused(rg(lst=(0, R.VOCAB)), b"token id out of range")
    refused(rg(lst=(0, -1)), b"token id out of range")
    refused(rg(o=None), b"null pointer")
    refused(rg(n=n - 1), b"multiple of the 16-byte chunk")
    refused(fh(p=None), b"null pointer")
    refused(fh(k=None), b"null pointer")
    refused(fh(F=0), b"words_per_frame")
    refused(fh(w=0), b"words_per_frame")
    refused(fh(F=65536), b"words_per_frame")
    refused(fh(w=2 ** 32 + 1), b"words_per_frame")
    refused(ga(rows=-1), b"rows must be >= 0")
    refused(ga(er=0), b"embed_rows and feat_rows >= 1")
    refused(ga(fr=0), b"embed_rows and feat_rows >= 1")
    refused(rg(rows=-1), b"rows must be >= 0")
    refused(rg(er=0), b"embed_rows and out_rows >= 1")
    refused(rg(orows=0), b"embed_rows and out_rows >= 1")
    assert bool(untouched(buf.cpu()[[0, 5]]).all())


# ---------------------------------------------------------------------------------------------------------- frame hash
def gpu_keys(m, pix):
    """keys [F][2] uint64 of pix [F][words] uint32 (numpy)"""
    F, words = pix.shape
    d = torch.from_numpy(pix.view(np.int32)).cuda()
    keys = (C.c_uint64 * (2 * F))(*([0xDEAD] * (2 * F)))
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_frame_hash(m._h, ptr(d), F, words, keys))
    return np.array(list(keys), dtype=np.uint64).reshape(F, 2)


@pytest.mark.parametrize("F", R.HASH_FRAMES)
@pytest.mark.parametrize("words", R.HASH_WORDS)
def test_frame_hash(F, words):
    m = engine(torch.bfloat16)
    pix = R.hash_words(F, words)
    ref = R.frame_keys(pix)
    got = gpu_keys(m, pix)
    assert (got == ref).all(), f"F {F} words {words}: keys differ from the exact reference in frames {sorted(set(np.nonzero(got != ref)[0].tolist()))}"
    assert (gpu_keys(m, pix) == got).all()                              # the keys are zeroed before every launch
    if F > 1:                                                           # the same frame, the same key, whatever its batch slot
        moved = pix.copy()
        moved[F - 1] = pix[0]
        k = gpu_keys(m, moved)
        assert (k[F - 1] == got[0]).all() and (k[0] == got[0]).all()
    one = pix[:1].copy()
    i, j = 3, words - 2
    swapped, flipped = one.copy(), one.copy()
    swapped[0, [i, j]] = one[0, [j, i]]
    flipped[0, words // 2] ^= 1                                         # the lowest mantissa bit of one word
    for name, other in (("swapped", swapped), ("flipped", flipped)):
        k = gpu_keys(m, other)[0]
        assert k[0] != got[0, 0] and k[1] != got[0, 1], f"F {F} words {words}: {name} words leave a half of the key unchanged"
        assert (k == R.frame_keys(other)[0]).all()


def test_feature_cache_keys_hits_and_replacement():
    """the feature cache through the public calls: one bit of one word makes a miss; a hit returns the features of the miss bit for bit;
    identical frames in one call share features; with capacity 2 the least recently used entry is the one replaced"""
    cfg = TINY
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=1, max_frames=3, max_positions=2048)
    try:
        m.load_synthetic(5)
        m.set_feature_cache(2)
        g = np.random.default_rng(8)
        fr = lambda: (2 * g.random((1, 3, cfg.v_image, cfg.v_image)) - 1).astype(np.float32)
        A, B, Cc = fr(), fr(), fr()
        A1 = A.copy()
        A1.view(np.uint32)[0, 1, 200, 17] ^= 1                          # one bit of one word
        rows, H = cfg.pool_tokens, cfg.hidden

        def encode(*frames):
            pix = np.ascontiguousarray(np.concatenate(frames))
            _lib.check(m._lib.svln_encode_frames(m._h, C.c_void_p(pix.ctypes.data), len(frames), 0))
            out = np.zeros((len(frames) * rows, H), dtype=np.float32)
            _lib.check(m._lib.svln_get_frame_feats(m._h, 0, len(frames) * rows, out.ctypes.data_as(C.POINTER(C.c_float))))
            return out.reshape(len(frames), rows, H)

        stats = m.feature_cache_stats
        fa = encode(A)[0]
        assert stats() == (0, 1) and np.isfinite(fa).all() and float(np.abs(fa).max()) > 0
        assert np.array_equal(encode(A)[0].view(np.uint32), fa.view(np.uint32)) and stats() == (1, 1)         # hit == the miss, bit for bit
        fa1 = encode(A1)[0]
        assert stats() == (1, 2), "a frame that differs in one bit of one word must miss"
        # cache now: A (older), A1.  B replaces A, the least recently used
        encode(B)
        assert stats() == (1, 3)
        assert np.array_equal(encode(A1)[0].view(np.uint32), fa1.view(np.uint32)) and stats() == (2, 3)       # A1 survived ...
        encode(A)
        assert stats() == (2, 4)                                                                              # ... A did not; A now replaces B
        assert np.array_equal(encode(A1)[0].view(np.uint32), fa1.view(np.uint32)) and stats() == (3, 4)
        encode(B)
        assert stats() == (3, 5)                                                                              # B was the one replaced
        # two identical frames in one call: the same features, at most two misses
        h0, m0 = stats()
        two = encode(Cc, Cc)
        h1, m1 = stats()
        assert m1 - m0 <= 2 and (h1 - h0) + (m1 - m0) == 2
        print("identical frames in one call: max |difference|", float(np.abs(two[0] - two[1]).max()))
        assert np.array_equal(two[0].view(np.uint32), two[1].view(np.uint32))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------- memory prune
@pytest.mark.parametrize("case", R.PRUNE_CASES, ids=lambda c: c.id)
def test_memory_prune(case):
    """the kept set equals the reference's with no near-tie escape: the cases are built with a gap of >= 10 bounds at the cut, apart from
    exact ties of bit-identical rows (the lower index survives)"""
    case.build()
    dt, N, keep = case.dtype, case.N, case.keep
    m = engine(dt)
    dm = dev(case.mem, dt)
    out_idx = (C.c_int32 * keep)(*([-7] * keep))
    out_score = np.full(N, np.nan, dtype=np.float32)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_memory_prune(m._h, ptr(dm), N, keep, out_idx, out_score.ctypes.data_as(C.POINTER(C.c_float))))
    sel, s = case.reference()
    bound = case.score_bound()
    err = np.abs(out_score.astype(np.float64) - s)
    with np.errstate(all="ignore"):
        print(f"{case.id}: worst score error / bound {float(np.nanmax(err / bound)):.3f}")
    assert np.isfinite(out_score).all(), f"{case.id}: non-finite score"
    assert (err <= bound).all(), f"{case.id}: worst score error / bound {float((err / bound).max()):.3f}"
    assert list(out_idx) == sel, f"{case.id}: kept {[i for i in out_idx if i not in sel][:8]} instead of {[i for i in sel if i not in list(out_idx)][:8]}"
    if case.kind == "zero-row":
        assert out_score[5] == 0.0
    if case.kind == "identical":
        assert len(set(out_score.tolist())) == 1
    if case.pair:
        assert out_score[case.pair[0]] == out_score[case.pair[1]]


# ---------------------------------------------------------------------------------------------------------- pool and patchify
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
@pytest.mark.parametrize("kind", ["gradient", "one-hot"])
def test_pool(dtype, kind):
    m = engine(dtype)
    x = R.pool_input(dtype, kind)
    ref, bound = R.pool_ref(x, want_bound_for=dtype)
    din = dev(x, dtype)
    rows = R.POOL_F * R.OSIDE * R.OSIDE
    buf, out = canaried(rows, R.POOL_C, dtype)
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_pool(m._h, ptr(din), ptr(out), R.POOL_F))
    assert bool(untouched(buf[[0, rows + 1]]).all()), "pool: canary row written"
    within(buf[1:rows + 1], ref.reshape(rows, R.POOL_C), bound.reshape(rows, R.POOL_C), f"pool-{R.NAME[dtype]}-{kind}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_patchify_is_a_copy(dtype):
    """pixels that are values of the engine type come out bit for bit; the pad columns 588 .. 591 are zero over a buffer of ones"""
    m = engine(dtype)
    pix = R.pixels(dtype)
    ref = R.to_t(R.patchify_ref(pix), dtype)
    dpix = torch.from_numpy(pix.astype(np.float32)).cuda()
    out = torch.ones((ref.shape[0] + 2, R.KP), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_patchify(m._h, ptr(dpix), ptr(out[1:]), R.POOL_F))
    got = out.cpu()
    assert bool((got[[0, -1]] == 1).all()), "patchify: guard row written"
    bad = got[1:-1] != ref
    assert not bool(bad.any()), f"patchify: {int(bad.sum())} of {bad.numel()} values differ, first at {torch.nonzero(bad)[0].tolist()}"
    assert bool((got[1:-1, R.KREAL:] == 0).all())
