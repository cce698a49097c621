"""The engine's own LLM attention path on sharp inputs (tests/attn_ref.py), against a float64 reference:
  * decode: svln_op_attention_decode runs the engine's decode step attention (attn_decode_kernel: RoPE of q / k in the kernel, K / V
    append at the decoded position, split-KV partials, attn_combine_kernel), B = 1 through the single-env step and B = 2 / 4 / 8
    through the batched one, over scrambled page orders;
  * prefill: svln_op_attention_llm (causal, grid key split where the engine takes it) on needle / rising / falling inputs;
  * ViT: svln_op_attention_vit on sharp rows, and svln_op_vit_qkv_attention -- the tower's q|k|v product + attention, whose K / V^T pages
    come from one of three packers -- on selection weights.
The pools are filled with a finite sentinel before every op and the split-KV partials with NaN, so a read of an unwritten slot or of
a partial no workgroup wrote shows; K / V rows are read back through svln_op_kv_read / svln_op_vit_kv_read."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ref as R
from streamvln_amd import _lib
from streamvln_amd import weights as W
from streamvln_amd.config import CONFIGS
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
MAX_ENVS = 8
_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for m in _engines.values():
        m.close()
    _engines.clear()


def engine(cfg, dtype, max_positions=R.MAX_POSITIONS):
    key = (cfg.name, dtype, max_positions)
    if key not in _engines:
        _engines[key] = StreamVLNForCausalLM(cfg, dtype=dtype, max_envs=MAX_ENVS, max_frames=1, max_positions=max_positions)
    return _engines[key]


def chk(rc):
    _lib.check(rc)


def scrambled_pages(env, seed, max_positions):
    """a permutation of env's own block of pages in which no logical page is its physical page"""
    n = max_positions // R.PAGE
    perm = np.random.default_rng(seed).permutation(n)
    for i in range(n):
        if perm[i] == i:
            j = (i + 1) % n
            perm[i], perm[j] = perm[j], perm[i]
    return (env * n + perm).astype(np.int32)


def setup(m, envs, seed, max_positions=R.MAX_POSITIONS):
    """scrambled page orders for envs 0 .. envs-1, sentinel pools, NaN partials; returns the page lists"""
    pages = []
    for b in range(envs):
        pg = scrambled_pages(b, seed + b, max_positions)
        chk(m._lib.svln_op_set_pages(m._h, b, pg.ctypes.data_as(C.POINTER(C.c_int32)), len(pg)))
        pages.append(pg)
    chk(m._lib.svln_op_fill_attn_state(m._h, R.SENTINEL, 1))
    return pages


def kv_read(m, cfg, env, n):
    """K / V rows [n][kv_heads][128] of env's positions 0 .. n-1 (env = -1: the raw pools, position = page * 64 + slot)"""
    k = np.zeros((n, cfg.kv_heads, R.HD), np.float32)
    v = np.zeros_like(k)
    chk(m._lib.svln_op_kv_read(m._h, env, 0, n, k.ctypes.data_as(C.POINTER(C.c_float)), v.ctypes.data_as(C.POINTER(C.c_float))))
    return torch.from_numpy(k).double(), torch.from_numpy(v).double()


def check_untouched(m, cfg, dtype, max_positions, written, what):
    """every pool slot outside `written` (env b's positions [lo, hi) through its page list) still holds the sentinel: all pages of all
    envs and the pages no env holds"""
    n_slots = MAX_ENVS * max_positions
    K, V = kv_read(m, cfg, -1, n_slots)
    mask = np.zeros(n_slots, bool)
    for pages, lo, hi in written:
        p = np.arange(lo, hi)
        mask[pages[p // R.PAGE].astype(np.int64) * R.PAGE + p % R.PAGE] = True
    keep = torch.from_numpy(~mask)
    sent = float(torch.tensor(R.SENTINEL, dtype=dtype).double())
    bad = ((K[keep] != sent) | (V[keep] != sent)).flatten(1).any(1)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} pool slots outside the op's positions were written"


def check_pool(case, K, V, what, lo=0):
    """K / V rows of positions lo .. L-1 against the case: roped K within the RoPE bound, V bit-equal"""
    L = case.L
    kref, kb = R.roped_k_bound(case.k_in[lo:], torch.arange(lo, L), case.cfg.rope_theta, case.dtype)
    bad = (K[lo:L] - kref).abs() > kb
    assert not bool(bad.any()), f"{what}: roped K off at positions {sorted(set((lo + torch.nonzero(bad)[:, 0]).tolist()))[:8]}"
    vbad = V[lo:L] != case.v[lo:]
    assert not bool(vbad.any()), f"{what}: V rows not bit-equal at positions {sorted(set((lo + torch.nonzero(vbad)[:, 0]).tolist()))[:8]}"


def check_out(got, case, q, K, what, q_flips, device):
    exp = case.attend(q=q, k=K[:case.L], device=device)
    tol = case.tolerance(q=q, k=K[:case.L], q_flips=q_flips, device=device)
    err = (got.to(device) - exp).abs()
    ratio = float((err / tol).amax())
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert ratio <= 1.0, f"{what}: max err / tolerance {ratio:.3g} (max err {float(err.amax()):.3e})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,positions,max_positions", R.decode_cases())
def test_attention_decode(dtype, cfg, positions, max_positions):
    cfg = CONFIGS[cfg]
    m = engine(cfg, dtype, max_positions)
    B = len(positions)
    pages = setup(m, B, 100 + sum(positions), max_positions)
    cases = [R.decode_case(cfg, dtype, p, b, max_positions) for b, p in enumerate(positions)]
    ld = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD
    ctx_rows = max(max(positions), 1)
    ctx = torch.zeros((B, ctx_rows, ld), dtype=dtype)
    new = torch.zeros((B, ld), dtype=dtype)
    for b, (case, p) in enumerate(zip(cases, positions)):
        rows = case.qkv_rows()
        ctx[b, :p] = rows[:p].to(dtype)
        new[b] = rows[p].to(dtype)
    dctx, dnew = ctx.cuda(), new.cuda()
    out = torch.full((B, cfg.q_heads * R.HD), float("nan"), dtype=dtype, device="cuda")
    pos = np.asarray(positions, np.int32)
    torch.cuda.synchronize()
    chk(m._lib.svln_op_attention_decode(m._h, B, ptr(dctx), ld, ctx_rows, pos.ctypes.data_as(C.POINTER(C.c_int32)), ptr(dnew), ptr(out),
                                        cfg.q_heads * R.HD))
    got = out.double().cpu().view(B, cfg.q_heads, R.HD)
    for b, (case, p) in enumerate(zip(cases, positions)):
        K, V = kv_read(m, cfg, b, p + 1)
        what = f"decode {cfg.name} B{B} env {b} pos {p}"
        check_pool(case, K, V, what)
        check_out(got[b:b + 1], case, None, K, what, q_flips=True, device="cuda")
    check_untouched(m, cfg, dtype, max_positions, [(pages[b], 0, p + 1) for b, p in enumerate(positions)], f"decode {cfg.name} {positions}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,T,P", R.PREFILL_CASES)
def test_attention_prefill(dtype, cfg, T, P):
    cfg = CONFIGS[cfg]
    m = engine(cfg, dtype)
    pages = setup(m, 1, 200 + T + P)
    case = R.prefill_case(cfg, dtype, T, P)
    ld = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD
    rows = case.qkv_rows().to(dtype)
    dctx, dnew = rows[:max(P, 1)].clone().cuda(), rows[P:].clone().cuda()
    out = torch.full((T, cfg.q_heads * R.HD), float("nan"), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    chk(m._lib.svln_op_attention_llm(m._h, ptr(dnew), ld, T, P, ptr(dctx), P, ptr(out), cfg.q_heads * R.HD, 1))
    L = P + T
    K, V = kv_read(m, cfg, 0, L)
    what = f"prefill {cfg.name} T{T} P{P}"
    check_pool(case, K, V, what)
    check_untouched(m, cfg, dtype, R.MAX_POSITIONS, [(pages[0], 0, L)], what)
    # the op ropes q in place: the reference takes the kernel's own roped q (checked against the float64 RoPE first)
    q_rb = dnew[:, :cfg.q_heads * R.HD].double().cpu().view(T, cfg.q_heads, R.HD)
    qref, qb = R.roped_k_bound(case.q_in[P:], torch.arange(P, L), cfg.rope_theta, dtype)
    assert bool(((q_rb - qref).abs() <= qb).all()), f"{what}: roped q"
    check_out(out.double().cpu().view(T, cfg.q_heads, R.HD), case, q_rb, K, what, q_flips=False, device="cuda")


QKV_ROPE_CASES = [("tiny", 37, 300), ("tiny", 212, 800), ("tiny", 1952, 0), ("true_dims_1layer", 37, 300),
                  ("true_dims_1layer", 212, 800), ("true_dims_1layer", 1952, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_llm_qkv_rope(dtype):
    """the prefill q|k|v product of one env's turn with RoPE + KV append (svln_op_llm_qkv_rope: prefill_qkv / prefill_rope_append of the
    engine), element by element.  Selection weights: q head h and its kv head's k read the same 128 input coordinates scaled by 2 and
    1/2, v other coordinates: every product has one non-zero term and a power-of-two weight, so the q|k|v values before RoPE are exact
    in both dtypes and the stored rows only carry the RoPE rounding.  Both paths must run in each dtype: the split-K reduce with RoPE
    fused (steady turns) and the product followed by the separate RoPE + append kernel (the window-restart rows)."""
    paths = set()
    for name, T, P in QKV_ROPE_CASES:
        cfg = CONFIGS[name]
        m = engine(cfg, dtype)
        H, nq, nkv, G = cfg.hidden, cfg.q_heads, cfg.kv_heads, cfg.q_heads // cfg.kv_heads
        d = np.arange(R.HD)
        wq = np.zeros((nq * R.HD, H), np.float32)
        wk = np.zeros((nkv * R.HD, H), np.float32)
        wv = np.zeros((nkv * R.HD, H), np.float32)
        for h in range(nq):
            wq[h * R.HD + d, ((h // G) * R.HD + d) % H] = 2.0
        for kh in range(nkv):
            wk[kh * R.HD + d, (kh * R.HD + d) % H] = 0.5
            wv[kh * R.HD + d, ((nkv + kh) * R.HD + d) % H] = 1.0
        pre = "model.layers.0.self_attn."
        for part, w in (("q_proj", wq), ("k_proj", wk), ("v_proj", wv)):
            m.set_tensor(pre + part + ".weight", w)
            m.set_tensor(pre + part + ".bias", np.zeros(w.shape[0], np.float32))
        pages = setup(m, 1, 300 + T + P)
        g = torch.Generator().manual_seed(T + P)
        x = (torch.rand((T, H), generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
        dx = x.cuda()
        qout = torch.full((T, nq * R.HD), float("nan"), dtype=dtype, device="cuda")
        fused = C.c_int32(-1)
        torch.cuda.synchronize()
        chk(m._lib.svln_op_llm_qkv_rope(m._h, ptr(dx), T, P, ptr(qout), nq * R.HD, C.byref(fused)))
        assert fused.value in (0, 1)
        paths.add(fused.value)
        what = f"qkv_rope {name} T{T} P{P} fused={fused.value}"
        xd = x.double()
        cols = lambda kh: (kh * R.HD + d) % H
        q_pre = torch.stack([2.0 * xd[:, cols(h // G)] for h in range(nq)], 1)                 # [T, nq, 128]
        k_pre = torch.stack([0.5 * xd[:, cols(kh)] for kh in range(nkv)], 1)
        v_pre = torch.stack([xd[:, cols(nkv + kh)] for kh in range(nkv)], 1)
        pos = torch.arange(P, P + T)
        qref, qb = R.roped_k_bound(q_pre, pos, cfg.rope_theta, dtype)
        qbad = (qout.double().cpu().view(T, nq, R.HD) - qref).abs() > qb
        assert not bool(qbad.any()), f"{what}: roped q off at rows {sorted(set(torch.nonzero(qbad)[:, 0].tolist()))[:8]}"
        K, V = kv_read(m, cfg, 0, P + T)
        kref, kb = R.roped_k_bound(k_pre, pos, cfg.rope_theta, dtype)
        kbad = (K[P:] - kref).abs() > kb
        assert not bool(kbad.any()), f"{what}: roped K off at positions {sorted(set((P + torch.nonzero(kbad)[:, 0]).tolist()))[:8]}"
        assert torch.equal(V[P:], v_pre), f"{what}: V rows not bit-equal"
        check_untouched(m, cfg, dtype, R.MAX_POSITIONS, [(pages[0], P, P + T)], what)
    assert paths == {0, 1}, f"{dtype}: the fused RoPE path and the separate RoPE + append path must both run (saw {sorted(paths)})"


# ---------------------------------------------------------------------------------------------------------------- ViT
VIT_MAX_FRAMES = 9          # the window-restart batch


def vit_engine(cfg, dtype):
    key = (cfg.name, dtype, "vit")
    if key not in _engines:
        _engines[key] = StreamVLNForCausalLM(cfg, dtype=dtype, max_envs=1, max_frames=VIT_MAX_FRAMES, max_positions=R.MAX_POSITIONS)
    return _engines[key]


def vit_kv_read(m, cfg, dtype):
    """the raw ViT pools: K [page][64][HDP], V^T [page][96][64] over all key tiles * max_frames * heads pages"""
    pages = R.VTILES * VIT_MAX_FRAMES * cfg.v_heads
    K = np.zeros((pages, R.PAGE, R.vit_hdp(dtype)), np.float32)
    V = np.zeros((pages, R.VROWS, R.PAGE), np.float32)
    chk(m._lib.svln_op_vit_kv_read(m._h, K.ctypes.data_as(C.POINTER(C.c_float)), V.ctypes.data_as(C.POINTER(C.c_float))))
    return torch.from_numpy(K).double(), torch.from_numpy(V).double()


def check_vit_pools(m, case, pad, what):
    """K / V^T pages of the F-frame layout (page = tile * F * heads + frame * heads + head) against the case's k / v rows, bit-equal.
    pad: the values allowed in the pad channels, the V^T pad rows and the keys past 729 of the last tile (None: not checked), where
    pages past the layout must still hold the sentinel too.  Returns the layout's K pages [tiles, F, heads, 64, HDP]."""
    cfg, dtype, F, H = case.cfg, case.dtype, case.F, case.heads
    K, V = vit_kv_read(m, cfg, dtype)
    used, hdp, n = R.VTILES * F * H, R.vit_hdp(dtype), R.VTILES * R.PAGE
    Kl = K[:used].view(R.VTILES, F, H, R.PAGE, hdp)
    Vl = V[:used].view(R.VTILES, F, H, R.VROWS, R.PAGE)
    kx = torch.zeros((F, n, H, R.VHD), dtype=torch.float64)
    vx = torch.zeros_like(kx)
    kx[:, :R.VS], vx[:, :R.VS] = case.k, case.v
    kexp = kx.view(F, R.VTILES, R.PAGE, H, R.VHD).permute(1, 0, 3, 2, 4)            # [tiles, F, H, 64, 72]
    vexp = vx.view(F, R.VTILES, R.PAGE, H, R.VHD).permute(1, 0, 3, 4, 2)            # [tiles, F, H, 72, 64]
    valid = torch.arange(n) < R.VS
    kvalid = valid.view(R.VTILES, 1, 1, R.PAGE, 1).expand_as(kexp)
    vvalid = valid.view(R.VTILES, 1, 1, 1, R.PAGE).expand_as(vexp)
    for nm, got, exp, ok in (("K", Kl[..., :R.VHD], kexp, kvalid), ("V^T", Vl[:, :, :, :R.VHD], vexp, vvalid)):
        bad = (got != exp) & ok
        if bool(bad.any()):
            t, f, h, a, b = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} {nm} data slots differ from the rows (first: tile {t} frame {f} head {h} at "
                                 f"{a}, {b}: {float(got[t, f, h, a, b])} != {float(exp[t, f, h, a, b])})")
    if pad is None:
        return Kl
    allowed = lambda x: torch.stack([x == float(torch.tensor(p, dtype=dtype).double()) for p in pad]).any(0)
    sent = float(torch.tensor(R.SENTINEL, dtype=dtype).double())
    for nm, vals in (("K pad channels", Kl[..., R.VHD:]), ("K keys past 729", Kl[..., :R.VHD][~kvalid]),
                     ("V^T pad rows", Vl[:, :, :, R.VHD:]), ("V^T keys past 729", Vl[:, :, :, :R.VHD][~vvalid])):
        assert bool(allowed(vals).all()), f"{what}: {nm} hold values other than {pad}: {sorted(set(vals[~allowed(vals)].tolist()))[:6]}"
    assert bool((K[used:] == sent).all()) and bool((V[used:] == sent).all()), f"{what}: pages past the {F}-frame layout were written"
    return Kl


def check_vit_out(out, case, what):
    got = out.double().view(case.F, R.VS, case.heads, R.VHD)
    exp = case.attend(device="cuda")
    tol = case.tolerance(device="cuda")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - exp).abs()
    ratio = float((err / tol).amax())
    assert ratio <= 1.0, f"{what}: max err / tolerance {ratio:.3g} (max err {float(err.amax()):.3e})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,F", R.VIT_CASES)
def test_attention_vit_sharp(dtype, cfg, F):
    """svln_op_attention_vit (the standalone packer, then the key-group or plain kernel) on sharp rows (tests/attn_ref.py vit_case):
    every row of every head and frame against the float64 reference; the packer's pages bit-equal to the rows with zero padding, the
    pages past the F-frame layout untouched"""
    cfg = CONFIGS[cfg]
    m = vit_engine(cfg, dtype)
    chk(m._lib.svln_op_fill_vit_state(m._h, R.SENTINEL, 1))
    case = R.vit_case(cfg, dtype, F)
    Hv = cfg.v_hidden
    dq = case.qkv_rows().to(dtype).cuda()
    out = torch.full((F * R.VS, Hv), float("nan"), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    chk(m._lib.svln_op_attention_vit(m._h, ptr(dq), 3 * Hv, F, ptr(out), Hv))
    what = f"vit {cfg.name} F{F} KG{case.KG}"
    check_vit_pools(m, case, (0.0,), what)
    check_vit_out(out, case, what)


QW, KW = 4.0, 0.5           # selection weights of q and k (v: 1)


def set_vit_selection_weights(m, cfg, layer=0):
    """q and k channel (h, d) read input coordinate h * 72 + d (times QW / KW), v channel (h, d) reads head h + 1's coordinate; no bias:
    every q|k|v value is one product by a power of two, exact in both dtypes"""
    Hv, H = cfg.v_hidden, cfg.v_heads
    eye = np.eye(Hv, dtype=np.float32)
    perm = (np.arange(Hv) + R.VHD) % Hv
    pre = f"{W.VT}encoder.layers.{layer}.self_attn."
    for part, w in (("q_proj", QW * eye), ("k_proj", KW * eye), ("v_proj", eye[perm])):
        m.set_tensor(pre + part + ".weight", w)
        m.set_tensor(pre + part + ".bias", np.zeros(Hv, np.float32))


def run_vit_qkv(m, cfg, dtype, F, seed, force_split=0):
    """svln_op_vit_qkv_attention on random rows x: -> (case with the exact q / k / v, qkv_out, attn_out, packer)"""
    Hv, H = cfg.v_hidden, cfg.v_heads
    g = torch.Generator().manual_seed(seed)
    x = R.rnd_dtype(torch.rand((F * R.VS, Hv), generator=g, dtype=torch.float64) * 2 - 1, dtype)
    dx = x.to(dtype).cuda()
    qkv = torch.full((F * R.VS, 3 * Hv), float("nan"), dtype=dtype, device="cuda")
    out = torch.full((F * R.VS, Hv), float("nan"), dtype=dtype, device="cuda")
    packer = C.c_int32(-1)
    torch.cuda.synchronize()
    chk(m._lib.svln_op_vit_qkv_attention(m._h, 0, ptr(dx), F, ptr(qkv), ptr(out), Hv, force_split, C.byref(packer)))
    shape = (F, R.VS, H, R.VHD)
    case = R.VitCase(cfg, dtype, F, (QW * x).view(shape), (KW * x).view(shape), torch.roll(x, -R.VHD, 1).view(shape))
    return case, qkv, out, packer.value


def check_qkv_out(qkv, case, what):
    bad = qkv.double().cpu() != case.qkv_rows()
    if bool(bad.any()):
        r, c = torch.nonzero(bad)[0].tolist()
        parts = sorted({("q", "k", "v")[i // case.cfg.v_hidden] for i in torch.nonzero(bad)[:, 1].tolist()})
        raise AssertionError(f"{what}: qkv_out not bit-equal in parts {parts} ({int(bad.sum())} values; first row {r} col {c})")


# (cfg, F, force_split): the real shapes, then forced K splits.  At the real shapes fp32 reaches all three packers (TINY: the split-K
# reduce, TRUE1 F = 1: the tile epilogue, F >= 2: none), bf16 never the split-K reduce (TINY's K = 144 is too short to split, TRUE1 F = 1
# takes the tile epilogue): the forced cases run it on the TINY and TRUE1 one-frame shapes.
VIT_QKV_CASES = [(name, F, 0) for name, F in R.VIT_CASES] + [("tiny", 3, 2), ("true_dims_1layer", 1, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_vit_qkv_packers(dtype):
    """the tower's q|k|v product + attention (svln_op_vit_qkv_attention: vit_qkv_attention, as run_vit runs it) on selection weights:
    qkv_out bit-equal with all three parts, the K / V^T pages bit-equal to its k / v columns whichever packer wrote them -- the split-K
    reduce with the pack fused (1), the 128x128 tile epilogue (2) or, where the product packs nothing, the standalone packer (0) --
    padding zero (or still the sentinel: the tile epilogue never writes it), pages past the layout untouched, the attention within the
    reference tolerance.  Each dtype must see all three packers over the cases (bf16 sees the split-K reduce only where it is forced: see
    VIT_QKV_CASES)."""
    packers = {}
    for name, F, force in VIT_QKV_CASES:
        cfg = CONFIGS[name]
        m = vit_engine(cfg, dtype)
        set_vit_selection_weights(m, cfg)
        chk(m._lib.svln_op_fill_vit_state(m._h, R.SENTINEL, 1))
        case, qkv, out, pk = run_vit_qkv(m, cfg, dtype, F, 12000 + F + force, force)
        assert pk in (0, 1, 2)
        if force:
            assert pk == 1, f"{name} F{F}: a forced K split must take the split-K reduce's fused pack (packer {pk})"
        packers[(name, F, force)] = pk
        what = f"vit qkv {name} F{F} split {force} packer {pk}"
        check_qkv_out(qkv, case, what)
        check_vit_pools(m, case, (0.0, R.SENTINEL) if pk == 2 else (0.0,), what)
        check_vit_out(out, case, what)
    assert set(packers.values()) == {0, 1, 2}, f"{dtype}: all three packers must run (saw {packers})"


@pytest.mark.parametrize("dtype", DTYPES)
def test_vit_restart_then_steady(dtype):
    """production order on one engine: a nine-frame window restart, then a one-frame steady step without refilling the pools.  When the
    tile epilogue packs the one-frame step (it never writes padding), that layout's last tile still holds nine-frame data in its pad
    keys (asserted), which the attention must mask."""
    cfg = CONFIGS["true_dims_1layer"]
    m = vit_engine(cfg, dtype)
    set_vit_selection_weights(m, cfg)
    chk(m._lib.svln_op_fill_vit_state(m._h, R.SENTINEL, 1))
    run_vit_qkv(m, cfg, dtype, 9, 13009)
    case, qkv, out, pk = run_vit_qkv(m, cfg, dtype, 1, 13001)
    what = f"vit qkv restart -> steady, packer {pk}"
    check_qkv_out(qkv, case, what)
    Kl = check_vit_pools(m, case, None, what)
    stale = Kl[-1, :, :, R.VS - (R.VTILES - 1) * R.PAGE:, :R.VHD]
    sent = float(torch.tensor(R.SENTINEL, dtype=dtype).double())
    if pk == 2:
        assert bool(((stale != 0) & (stale != sent)).any()), f"{what}: the last tile's pad keys do not hold the nine-frame data"
    check_vit_out(out, case, what)
