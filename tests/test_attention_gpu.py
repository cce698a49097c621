"""The engine's own LLM attention path on sharp inputs (tests/attn_ref.py), against a float64 reference:
  * decode: svln_op_attention_decode runs the engine's decode step attention (attn_decode_kernel: RoPE of q / k in the kernel, K / V
    append at the decoded position, split-KV partials, attn_combine_kernel), B = 1 through the single-env step and B = 2 / 4 / 8
    through the batched one, over scrambled page orders;
  * prefill: svln_op_attention_llm (causal, grid key split where the engine takes it) on needle / rising / falling inputs.
The pools are filled with a finite sentinel before every op and the split-KV partials with NaN, so a read of an unwritten slot or of
a partial no workgroup wrote shows; K / V rows are read back through svln_op_kv_read."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ref as R
from streamvln_amd import _lib
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
