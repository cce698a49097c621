"""The two kernels of a beam step at op level on a TINY engine.

beam_select_kernel (svln_op_beam_select) against tests/beam_ref.py: every designed case of beam_ref.cases() is walked step by step; at
every step the kernel gets the restatement's state and lists and must return its new set (ids, log-probabilities and scores bit for bit,
flags, page sets), fed tokens, parents, page pairs and record.

kv_page_gather_kernel (svln_op_beam_page_gather) on fp32 and bf16 engines: the pools carry the position-coded pattern of a 70-token prefill
over a poison fill (as tests/test_group_ops_gpu.py builds it); every page of every layer and both pools is read before and after each
launch: destinations bit-equal to their sources, every page not named unchanged; n = 1 and n = 2 W = 16, one source for two
destinations; every malformed call refused with the pools unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_ref as br
from scenarios import SEED
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM

pytestmark = pytest.mark.gpu
PAGE, POISON, N_TOKENS = 64, 6.5, 70
MAX_POSITIONS = 2048                  # 32 pages, one env
PI, PF = C.POINTER(C.c_int32), C.POINTER(C.c_float)
LEN_CAP = 64


def _pi(a):
    return a.ctypes.data_as(PI)


def _pf(a):
    return a.ctypes.data_as(PF)


@pytest.fixture(scope="module")
def engine():
    m = StreamVLNForCausalLM(TINY, dtype=torch.float32, max_envs=1, max_frames=1, max_positions=256)
    yield m
    m.close()


def _select(m, st, li, ll, W, limit, eos, n_cp, set_pages, B, tok_fill=-7):
    """one svln_op_beam_select call on the restatement's state -> (state, fed, pairs, rec) in beam_ref.step's form"""
    n = st["n"]
    hdr = np.zeros(25, dtype=np.int32)
    score = np.zeros(8, dtype=np.float32)
    ids, lps = np.full((8, LEN_CAP), -3, dtype=np.int32), np.full((8, LEN_CAP), 0.5, dtype=np.float32)
    hdr[0] = n
    for r in range(n):
        hdr[1 + r], hdr[9 + r], hdr[17 + r], score[r] = len(st["ids"][r]), int(st["fin"][r]), st["set_of"][r], st["score"][r]
        ids[r, : len(st["ids"][r])] = st["ids"][r]
        lps[r, : len(st["lps"][r])] = st["lps"][r]
    lid, llp = np.full((8, W), -1, dtype=np.int32), np.full((8, W), -np.inf, dtype=np.float32)
    for r in range(len(li)):
        lid[r], llp[r] = li[r], ll[r]
    eos_a = np.asarray(list(eos) + [0], dtype=np.int32)
    sp = np.ascontiguousarray(set_pages, dtype=np.int32) if n_cp else None
    hdr_o, score_o = np.zeros(25, dtype=np.int32), np.zeros(8, dtype=np.float32)
    ids_o, lps_o = np.full((8, LEN_CAP), -5, dtype=np.int32), np.full((8, LEN_CAP), 0.25, dtype=np.float32)
    tok = np.full(B, tok_fill, dtype=np.int32)
    ps, pd = np.full(8 * max(n_cp, 1), -9, dtype=np.int32), np.full(8 * max(n_cp, 1), -9, dtype=np.int32)
    rec = np.zeros(br.REC, dtype=np.int32)
    rc = m._lib.svln_op_beam_select(m._h, W, limit, B, n_cp, LEN_CAP, _pi(eos_a), len(eos), _pi(lid), _pf(llp), _pi(hdr), _pf(score), _pi(ids),
                                    _pf(lps), _pi(sp) if n_cp else None, _pi(hdr_o), _pf(score_o), _pi(ids_o), _pf(lps_o), _pi(tok), _pi(ps),
                                    _pi(pd), _pi(rec))
    assert rc == 0, m._lib.svln_last_error()
    nn = int(hdr_o[0])
    new = {"n": nn, "ids": [], "lps": [], "score": [], "fin": [], "set_of": []}
    for c in range(nn):
        k = int(hdr_o[1 + c])
        new["ids"].append(ids_o[c, :k].tolist()); new["lps"].append([np.float32(v) for v in lps_o[c, :k]])
        new["score"].append(np.float32(score_o[c])); new["fin"].append(bool(hdr_o[9 + c])); new["set_of"].append(int(hdr_o[17 + c]))
        assert (ids_o[c, k:] == -5).all() and (lps_o[c, k:] == 0.25).all()                # nothing written behind a row's end
    assert (ids_o[nn:] == -5).all() and (lps_o[nn:] == 0.25).all()                        # ... or into unused rows
    fed = [None if int(t) == tok_fill else int(t) for t in tok]
    pairs = list(zip(ps[: int(rec[3])].tolist(), pd[: int(rec[3])].tolist()))
    return new, fed, pairs, rec


def _same(a, b):
    return br.outputs(a) == br.outputs(b) and a["n"] == b["n"] and list(a["set_of"]) == list(b["set_of"])


CASES = br.cases()


@pytest.mark.parametrize("W", range(1, 9))
def test_select_equals_the_restatement_on_every_designed_case(engine, W):
    m = engine
    rng = np.random.RandomState(W)
    steps = 0
    for case in (c for c in CASES if c[1] == W):
        _, _, limit, eos, kw = case
        kw = dict(kw)
        provider = br.tree_provider(W, kw.pop("seed"), **kw)
        B = 2
        while B < W:
            B <<= 1
        st = br.root()
        for t in range(limit):
            if all(st["fin"][: st["n"]]):
                break
            li, ll = provider(t, st)
            n_cp = int(rng.randint(0, 3))
            set_pages = rng.permutation(1000)[: 16 * max(n_cp, 1)].reshape(16, max(n_cp, 1))
            want = br.step(st, li, ll, W, limit, eos, n_cp=n_cp, set_pages=set_pages, B=B)
            got = _select(m, st, li, ll, W, limit, eos, n_cp, set_pages, B)
            assert _same(got[0], want[0]), (case[0], t, got[0], want[0])
            assert got[1] == want[1], (case[0], t, "fed", got[1], want[1])
            assert got[2] == want[2], (case[0], t, "pairs", got[2], want[2])
            assert np.array_equal(got[3], want[3]), (case[0], t, "record", got[3], want[3])
            st = want[0]
            steps += 1
        assert br.outputs(st) == br.outputs(br.run_case(case)[0])       # the walk is the restatement's turn
    assert steps >= 8


def test_select_planted_ties_and_set_reuse(engine):
    m = engine
    h = np.float32(-0.5)
    # three hypotheses: rank 0 finished, ranks 1 and 2 live with equal scores, lists tying across and inside rows; sets out of order
    st = {"n": 3, "ids": [[9], [5, 1], [6, 1]], "lps": [[h], [h, h], [h, h]], "score": [np.float32(-0.5), np.float32(-1.0), np.float32(-1.0)],
          "fin": [True, False, False], "set_of": [4, 0, 7]}
    q, ninf = np.float32(-0.25), np.float32(-np.inf)
    li = [[0, 0, 0, 0], [3, 4, 8, -1], [3, 9, 1, 2]]
    ll = [[ninf] * 4, [q, q, np.float32(-0.75), ninf], [q, q, q, np.float32(-2.0)]]
    pages = np.arange(100, 132).reshape(16, 2)
    want = br.step(st, li, ll, 4, 5, [8], n_cp=2, set_pages=pages, B=4)
    got = _select(m, st, li, ll, 4, 5, [8], 2, pages, 4)
    assert want[0]["ids"] == [[9], [5, 1, 3], [5, 1, 4], [6, 1, 3]] and want[0]["set_of"] == [4, 0, 1, 7]
    assert want[2] == [(100, 102), (101, 103)] and want[1] == [3, 3, 4, 3]
    assert _same(got[0], want[0]) and got[1] == want[1] and got[2] == want[2] and np.array_equal(got[3], want[3])
    # the last entry of W = 8 lists and the EOS rule: every child of rank 0 finishes, nothing is fed
    st = br.root()
    li = [[10, 11, 12, 13, 14, 15, 16, 17]]
    ll = [[np.float32(-k / 4.0) for k in range(1, 9)]]
    want = br.step(st, li, ll, 8, 3, list(range(10, 18)), B=8)
    got = _select(m, st, li, ll, 8, 3, list(range(10, 18)), 0, None, 8)
    assert want[0]["n"] == 8 and all(want[0]["fin"]) and want[1] == [None] * 8
    assert _same(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[3], want[3])


def test_select_leaves_a_nan_score_out_of_the_pool(engine):
    nan, q = np.float32(np.nan), np.float32(-0.25)
    li, ll = [[4, 5, 6]], [[q, nan, np.float32(-0.5)]]
    want = br.step(br.root(), li, ll, 3, 5, [], B=4)
    got = _select(engine, br.root(), li, ll, 3, 5, [], 0, None, 4)
    assert want[0]["ids"] == [[4], [6]]
    assert _same(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[3], want[3])


def test_select_refuses_malformed_calls(engine):
    m = engine
    z25, z8f = np.zeros(25, dtype=np.int32), np.zeros(8, dtype=np.float32)
    rows_i, rows_f = np.zeros((8, LEN_CAP), dtype=np.int32), np.zeros((8, LEN_CAP), dtype=np.float32)
    lid, llp = np.zeros((8, 8), dtype=np.int32), np.zeros((8, 8), dtype=np.float32)
    out = dict(hdr=np.zeros(25, dtype=np.int32), sc=np.zeros(8, dtype=np.float32), ids=rows_i.copy(), lps=rows_f.copy(),
               tok=np.zeros(64, dtype=np.int32), ps=np.zeros(64, dtype=np.int32), pd=np.zeros(64, dtype=np.int32), rec=np.zeros(br.REC, dtype=np.int32))
    sets = np.arange(128, dtype=np.int32)
    eos = np.zeros(64, dtype=np.int32)

    def call(W=2, limit=5, B=2, n_cp=0, len_cap=LEN_CAP, n_eos=0, hdr=None, null=None):
        hdr = z25.copy() if hdr is None else hdr
        args = [W, limit, B, n_cp, len_cap, _pi(eos), n_eos, _pi(lid), _pf(llp), _pi(hdr), _pf(z8f), _pi(rows_i), _pf(rows_f), _pi(sets),
                _pi(out["hdr"]), _pf(out["sc"]), _pi(out["ids"]), _pf(out["lps"]), _pi(out["tok"]), _pi(out["ps"]), _pi(out["pd"]), _pi(out["rec"])]
        if null is not None:
            args[null] = None
        return m._lib.svln_op_beam_select(m._h, *args)

    def hdr(n, lens=(), fins=(), sets_=()):
        h = z25.copy()
        h[0] = n
        h[1: 1 + len(lens)], h[9: 9 + len(fins)], h[17: 17 + len(sets_)] = lens, fins, sets_
        return h

    ok = hdr(2, [1, 1], [0, 1], [0, 3])
    assert call(hdr=ok) == 0, m._lib.svln_last_error()
    bad = [dict(W=0), dict(W=9), dict(limit=0), dict(limit=LEN_CAP + 1), dict(len_cap=0), dict(len_cap=65), dict(B=0), dict(B=65), dict(n_cp=-1),
           dict(n_cp=9), dict(n_eos=-1), dict(n_eos=65), dict(hdr=hdr(-1)), dict(hdr=hdr(9)), dict(hdr=hdr(1, [1], [2], [0])),
           dict(hdr=hdr(1, [-1], [0], [0])), dict(hdr=hdr(1, [LEN_CAP + 1], [1], [0])), dict(hdr=hdr(1, [5], [0], [0])),
           dict(hdr=hdr(1, [1], [0], [16])), dict(hdr=hdr(1, [1], [0], [-1])), dict(hdr=hdr(2, [1, 1], [0, 0], [3, 3]))]
    bad += [dict(null=k) for k in (7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19, 20, 21)] + [dict(null=13, n_cp=1), dict(null=5, n_eos=1)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"svln_op_beam_select" in m._lib.svln_last_error(), kw
    assert call(hdr=hdr(1, [5], [1], [0])) == 0                   # a finished hypothesis may have reached the limit


# ---- the page hand-over ----------------------------------------------------------------------------------------------------------------
def _kv_engine(dtype):
    m = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=1, max_positions=MAX_POSITIONS)
    m.load_synthetic(SEED)
    assert m._lib.svln_op_fill_attn_state(m._h, POISON, 0) == 0
    ids = (np.arange(N_TOKENS, dtype=np.int64) * 37 + 11) % TINY.vocab
    assert m._lib.svln_append_turn(m._h, 0, ids.ctypes.data_as(C.POINTER(C.c_int64)), N_TOKENS, 0) == 0, m._lib.svln_last_error()
    out = np.zeros(1, dtype=np.int64)
    assert m._lib.svln_generate_fixed(m._h, 0, 1, out.ctypes.data_as(C.POINTER(C.c_int64))) == 0, m._lib.svln_last_error()
    return m


def _pools(m):
    """[layer][K | V][page][64 positions][kv_heads][128] of the whole pool, fp32 images of the engine dtype"""
    n = MAX_POSITIONS
    out = np.zeros((TINY.layers, 2, n, TINY.kv_heads, 128), dtype=np.float32)
    for layer in range(TINY.layers):
        assert m._lib.svln_op_kv_pool_read(m._h, layer, 0, n, _pf(out[layer, 0]), _pf(out[layer, 1])) == 0
    return out.reshape(TINY.layers, 2, n // PAGE, PAGE, TINY.kv_heads, 128)


def _gather(m, src, dst):
    s, d = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
    return m._lib.svln_op_beam_page_gather(m._h, _pi(s), _pi(d), len(dst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_page_gather_is_bit_exact_in_every_layer_and_touches_nothing_else(dtype):
    m = _kv_engine(dtype)
    last = MAX_POSITIONS // PAGE - 1
    before = _pools(m)
    assert not np.isnan(before).any()
    flat = before[:, :, :2].reshape(TINY.layers, 2, 2 * PAGE, -1)
    assert all(len({flat[l, kv, p].tobytes() for p in range(N_TOKENS)}) == N_TOKENS for l in range(TINY.layers) for kv in range(2))
    assert (before[0, :, 1, N_TOKENS - PAGE:] == POISON).all() and (before[0, :, 2:] == POISON).all()
    assert not np.array_equal(before[:, :, 0], before[:, :, 1])
    calls = [([1], [5]),                                                          # n = 1
             ([0, 1, 0], [7, last, 9]),                                           # one source for two destinations; the pool's last page
             ([0, 1] * 8, list(range(2, 18))),                                    # n = 2 W = 16
             ([5, last, 7], [20, 21, 2])]                                         # copies as sources, the last page among them
    for src, dst in calls:
        assert _gather(m, src, dst) == 0, m._lib.svln_last_error()
        after = _pools(m)
        for s, d in zip(src, dst):
            assert np.array_equal(after[:, :, d], before[:, :, s]), (s, d)
        rest = [p for p in range(last + 1) if p not in dst]
        assert np.array_equal(after[:, :, rest], before[:, :, rest]), (src, dst)
        before = after
    # every malformed call is refused before any launch: the pools do not change
    bad = [([], []), ([1] * 65, list(range(2, 32)) * 2 + list(range(2, 7))), ([-1], [3]), ([last + 1], [3]), ([1], [-1]), ([1], [last + 1]),
           ([1], [1]),                                                            # a destination equal to its source
           ([1, 3], [3, 4]),                                                      # overlapping sets: page 3 is read and written
           ([3, 1], [4, 3]),
           ([1, 1], [3, 3]),                                                      # a destination listed twice
           ([2], [0]), ([2, 2], [5, 1])]                                          # a destination held by the env
    for src, dst in bad:
        assert _gather(m, src, dst) != 0, (src, dst)
        assert b"svln_op_beam_page_gather" in m._lib.svln_last_error(), (src, dst)
    one = np.ones(1, dtype=np.int32)
    assert m._lib.svln_op_beam_page_gather(m._h, None, _pi(one), 1) != 0 and b"null" in m._lib.svln_last_error()
    assert m._lib.svln_op_beam_page_gather(m._h, _pi(one), None, 1) != 0 and b"null" in m._lib.svln_last_error()
    assert np.array_equal(_pools(m), before)
    assert m._lib.svln_reset_env(m._h, 0) == 0
    m.close()
