"""The mirror form of the RoPE + KV append launch (svln_op_rope_kv_mirror: rope_kv_kernel<T, true>) on poisoned layer-0 pools, fp32 and
bf16 engines.

The plain launch is the same op with an empty mirror list: that is the instantiation prefill_rope_append launches (the unfused leg of
svln_op_llm_qkv_rope), and it is pinned on its own here against the float64 RoPE of tests/attn_ref.py (the element bound of
test_attention_gpu.test_llm_qkv_rope).  Against it the mirror form must give
  * the q rows (roped in place) and the untouched k | v columns of the caller's rows, bit for bit;
  * every page of the env, bit for bit;
  * on each mirror page the cells of positions [max(P, 64 q0), L) equal to the env's page q0 = L / 64, in every kv head of K and V^T;
  * the poison in every other cell of the mirror pages and in every other page of the pool.
Shapes: T = 1, 3, 64, 70; L % 64 = 1, 61, 63 and 0 (a full last page: nothing lies in page L / 64, so nothing may be mirrored); rows that
cross from page q0 - 1 into q0; P inside page q0; 0, 1, 2 and 7 mirror pages, the first and the last page of the pool among them; a row
pitch wider than the q|k|v row.  Every malformed call is refused with the pools and the rows untouched."""
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
PI32, PF = C.POINTER(C.c_int32), C.POINTER(C.c_float)
MAX_ENVS, MAX_POSITIONS = 2, 512
N_PAGES = MAX_ENVS * MAX_POSITIONS // R.PAGE              # 16 pages in the pool
ENV_PAGES = [5, 9, 3]                                      # logical page i of env 0 -> physical page
LAST = N_PAGES - 1
#: (T, P, mirror pages, extra row pitch)
CASES = [
    (1, 64, [0], 0),                            # L = 65: one row, the first of page q0 = 1; the first page of the pool
    (1, 64, [], 0),
    (3, 62, [LAST, 0], 0),                      # L = 65: rows 62, 63 in page 0 (not mirrored), row 64 in page 1
    (3, 122, [7], 64),                          # L = 125: P inside page q0 = 1
    (64, 63, [1, 2], 0),                        # L = 127: crosses from page 0 into page 1
    (64, 63, [], 0),
    (70, 55, [0, 1, 2, 4, 6, 7, LAST], 0),      # L = 125: seven mirrors, crossing
    (70, 55, [], 64),
    (70, 119, [8, LAST], 0),                    # L = 189: q0 = 2, crosses from page 1, P inside page 1
    (64, 0, [], 0),                             # L = 64: a full page, the plain launch
    (70, 58, [], 0),                            # L = 128: full pages
    (70, 58, [0, LAST], 0),                     # L = 128 with a list: no row lies in page 2, nothing may be mirrored
    (1, 63, [4], 0),                            # L = 64: one row at the last slot of page 0, q0 = 1: nothing mirrored
]
_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for m in _engines.values():
        m.close()
    _engines.clear()


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(CONFIGS["tiny"], dtype=dtype, max_envs=MAX_ENVS, max_frames=1, max_positions=MAX_POSITIONS)
    return _engines[dtype]


def _sentinel(dtype):
    """the poison as the pools hold it: rounded to the engine dtype"""
    return np.float32(torch.tensor(R.SENTINEL).to(dtype).float().item())


def _pools(m):
    """the raw layer-0 pools: K, V as [page][slot][kv head][128] fp32"""
    n, nkv = N_PAGES * R.PAGE, m.cfg.kv_heads
    k, v = np.zeros((n, nkv, R.HD), np.float32), np.zeros((n, nkv, R.HD), np.float32)
    _lib.check(m._lib.svln_op_kv_read(m._h, -1, 0, n, k.ctypes.data_as(PF), v.ctypes.data_as(PF)))
    return k.reshape(N_PAGES, R.PAGE, nkv, R.HD), v.reshape(N_PAGES, R.PAGE, nkv, R.HD)


def _rows(cfg, dtype, T, P, pad):
    width = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD
    g = torch.Generator().manual_seed(1000 * T + P)
    rows = torch.full((T, width + pad), 7.0, dtype=dtype)
    rows[:, :width] = (torch.rand((T, width), generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    return rows


def _launch(m, rows, T, P, mirrors, env_pages=ENV_PAGES):
    """poison, fix env 0's pages, one svln_op_rope_kv_mirror call -> (rc, rows after the call, K pool, V pool)"""
    pg = np.asarray(env_pages, np.int32)
    _lib.check(m._lib.svln_op_set_pages(m._h, 0, pg.ctypes.data_as(PI32), len(pg)))
    _lib.check(m._lib.svln_op_fill_attn_state(m._h, R.SENTINEL, 0))
    d = rows.cuda()
    mp = np.asarray(list(mirrors) + [0], np.int32)
    torch.cuda.synchronize()
    rc = m._lib.svln_op_rope_kv_mirror(m._h, ptr(d), int(rows.shape[1]), T, P, mp.ctypes.data_as(PI32), len(mirrors))
    K, V = _pools(m)
    return rc, d.cpu(), K, V


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T,P,mirrors,pad", CASES, ids=[f"T{c[0]}-P{c[1]}-m{len(c[2])}{'-pitch' if c[3] else ''}" for c in CASES])
def test_mirror_pages_get_the_rows_of_page_q0_and_nothing_else(T, P, mirrors, pad, dtype):
    m = engine(dtype)
    cfg = m.cfg
    nq, nkv = cfg.q_heads, cfg.kv_heads
    L, q0 = P + T, (P + T) // R.PAGE
    rows = _rows(cfg, dtype, T, P, pad)
    rc, plain_rows, Kp, Vp = _launch(m, rows, T, P, [])
    assert rc == 0, m._lib.svln_last_error()
    # ---- the plain launch on its own: the float64 RoPE bound on q and K, V as fed, poison everywhere else
    pre = rows[:, : (nq + 2 * nkv) * R.HD].double().view(T, nq + 2 * nkv, R.HD)
    pos = torch.arange(P, L)
    got = plain_rows[:, : (nq + 2 * nkv) * R.HD].double().view(T, nq + 2 * nkv, R.HD)
    qref, qb = R.roped_k_bound(pre[:, :nq], pos, cfg.rope_theta, dtype)
    assert not bool(((got[:, :nq] - qref).abs() > qb).any()), "plain: roped q"
    assert torch.equal(got[:, nq:], pre[:, nq:]) and torch.equal(plain_rows[:, (nq + 2 * nkv) * R.HD:], rows[:, (nq + 2 * nkv) * R.HD:]), "plain: k | v columns / pitch"
    kref, kb = R.roped_k_bound(pre[:, nq:nq + nkv], pos, cfg.rope_theta, dtype)
    written = np.zeros((N_PAGES, R.PAGE), bool)
    for i, p in enumerate(range(P, L)):
        page, off = ENV_PAGES[p // R.PAGE], p % R.PAGE
        written[page, off] = True
        assert not bool(((torch.from_numpy(Kp[page, off]).double() - kref[i]).abs() > kb[i]).any()), ("plain: K", p)
        assert np.array_equal(Vp[page, off], pre[i, nq + nkv:].float().numpy()), ("plain: V", p)
    assert np.all(Kp[~written] == _sentinel(dtype)) and np.all(Vp[~written] == _sentinel(dtype)), "plain: a cell outside the rows was written"
    if not mirrors:
        return
    # ---- the mirror form against it
    rc, mir_rows, Km, Vm = _launch(m, rows, T, P, mirrors)
    assert rc == 0, m._lib.svln_last_error()
    assert torch.equal(mir_rows.view(torch.uint8), plain_rows.view(torch.uint8)), "the caller's rows (roped q, k | v, pitch) differ from the plain launch"
    lo = max(P, q0 * R.PAGE)
    expect_K, expect_V = Kp.copy(), Vp.copy()
    for mp in mirrors:
        for p in range(lo, L):                  # (empty when L % 64 == 0: no row lies in page q0)
            expect_K[mp, p % R.PAGE] = Kp[ENV_PAGES[q0], p % R.PAGE]
            expect_V[mp, p % R.PAGE] = Vp[ENV_PAGES[q0], p % R.PAGE]
    # the env's pages, the mirrored cells, and the poison of every other cell of every page, in every kv head: bit for bit
    assert Km.tobytes() == expect_K.tobytes(), [int(p) for p in np.unique(np.nonzero(Km != expect_K)[0])]
    assert Vm.tobytes() == expect_V.tobytes(), [int(p) for p in np.unique(np.nonzero(Vm != expect_V)[0])]
    if L % R.PAGE:
        assert all(np.all(Km[mp, lo % R.PAGE: L % R.PAGE] != _sentinel(dtype)) for mp in mirrors)       # (something was mirrored)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_malformed_calls_are_refused_with_the_pools_untouched(dtype):
    m = engine(dtype)
    T, P = 6, 60                                # L = 66, q0 = 1
    rows = _rows(m.cfg, dtype, T, P, 0)
    bad = [(dict(mirrors=[LAST, 0, 1, 2, 4, 6, 7, 8]), "0 .. 7"), (dict(mirrors=[N_PAGES]), "outside the pool"), (dict(mirrors=[-1]), "outside the pool"),
           (dict(mirrors=[ENV_PAGES[1]]), "page q0"), (dict(mirrors=[ENV_PAGES[0]]), "page of the env"), (dict(mirrors=[4, 7, 4]), "listed twice"),
           (dict(mirrors=[4], env_pages=ENV_PAGES[:1]), "beyond the env's pages"), (dict(mirrors=[], env_pages=ENV_PAGES[:1]), "beyond the env's pages"),
           (dict(mirrors=[4], P=MAX_POSITIONS - 3), "positions out of range"), (dict(mirrors=[4], env_pages=[]), "svln_op_set_pages")]
    for kw, match in bad:
        rc, after, K, V = _launch(m, rows, T, kw.get("P", P), kw["mirrors"], kw.get("env_pages", ENV_PAGES))
        err = m._lib.svln_last_error().decode()
        assert rc != 0 and match in err and "svln_op_rope_kv_mirror" in err, (kw, err)
        assert torch.equal(after.view(torch.uint8), rows.view(torch.uint8)), kw
        assert np.all(K == _sentinel(dtype)) and np.all(V == _sentinel(dtype)), kw
    n = np.zeros(1, np.int32)
    rc = m._lib.svln_op_rope_kv_mirror(m._h, ptr(rows.cuda()), int(rows.shape[1]), T, P, n.ctypes.data_as(PI32), -1)
    assert rc != 0 and "0 .. 7" in m._lib.svln_last_error().decode()
    rc = m._lib.svln_op_rope_kv_mirror(m._h, ptr(rows.cuda()), int(rows.shape[1]) - 1, T, P, n.ctypes.data_as(PI32), 0)
    assert rc != 0 and "row pitch" in m._lib.svln_last_error().decode()
    _lib.check(m._lib.svln_op_set_pages(m._h, 0, None, 0))
