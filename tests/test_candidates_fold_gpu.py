"""The folded candidates call (generate(candidate_ids=..., fold_candidates=True) / svln_generate_candidates_folded) on the GPU.

The unfolded call is the twin: the same engine after a reset, on the same prompt and candidates (the engine is deterministic, so this
is what a second engine would compute).  No folded result is bit-equal to it -- the products' row count selects their plan -- so
(c) every score and greedy_logprob lies inside the a-priori bound of tests/test_candidates_e2e_gpu.py (2 gamma_K max_n sum_k |w_nk h_k|
    + 2e-5 of float64 log_softmax(lm_head . h)) computed from the call's OWN tap rows;
(t) against the twin: tap rows within 1e-3 (fp32; the bf16 engine inside its existing relative bound), scores within the sum of the two
    calls' bounds, greedy_ids equal wherever the float64 top-2 gap exceeds the bound (exempted share <= 10 %);
(s) after select_sequence(g), for every g, at L % 64 = 0, 1, 61, 63 and at a second turn whose history ends inside page q0
    (P > 64 q0: the one page copy before the pass): the next plain turn is the one that follows a forced turn on F_g (ids on fp32,
    hidden <= 1e-3, cache lengths), and the prompt's K / V rows [64 q0, L) the env then reads are the same bits whichever g was taken;
(i) a candidate's results do not depend on its neighbours' ids, bit for bit;
(f) lengths (6, 1, 6, 2, 6, 3, 5, 6) among the shapes (G = 8 on tiny: r = 4, a candidate of 6 ids folds 4 fed rows and leaves one for
    pass 1); all ones: the unfolded call bit for bit; sampling (inv_t applied, no
    draw consumed); an allowed list; twenty calls on an exactly full pool; every refusal; the agent attribute."""
import ctypes as C

import numpy as np
import pytest
import torch

import group_ref as GR
from scenarios import SCENARIOS, SEED, eos_ids
from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from test_candidates_e2e_gpu import SHAPES, _bounds, _cands, _cands_rc, _candidates_of, _check_against_float64, _select, _tap_rows, _taps
from test_e2e_gpu import BF16_HIDDEN_REL, HIDDEN_TOL
from test_forced_e2e_gpu import LSE_TOL, _append, _begin, _close_models, _fixed, _forced, _generate, _head, _other, _prompt, model  # noqa: F401
from test_group_e2e_gpu import _held
from util import load_golden

pytestmark = pytest.mark.gpu
PI64, PF, PI32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
#: the unfolded test's shapes, plus a second turn whose history ends inside page q0 = 1 (P = 70 > 64, L = 100)
FOLD_SHAPES = SHAPES + [("tiny_episode", 70, 30, (5, 2, 5, 3))]


def _fold_rc(m, Fs, eos=(), env=0):
    flat = np.ascontiguousarray(np.concatenate([np.asarray(f, np.int64).reshape(-1) for f in Fs]) if len(Fs) else np.zeros(0, np.int64))
    lens = np.asarray([len(f) for f in Fs], np.int32)
    e = np.ascontiguousarray(eos, dtype=np.int64)
    n = max(int(flat.size), 1)
    lp, glp, gid = np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32), np.full(n, -7, np.int64)
    rc = m._lib.svln_generate_candidates_folded(m._h, env, len(Fs), flat.ctypes.data_as(PI64), lens.ctypes.data_as(PI32),
                                                e.ctypes.data_as(PI64) if e.size else None, int(e.size), lp.ctypes.data_as(PF),
                                                gid.ctypes.data_as(PI64), glp.ctypes.data_as(PF))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    split = lambda a: [a[off[g]:off[g + 1]].copy() for g in range(len(Fs))]
    return rc, split(lp), [g.tolist() for g in split(gid)], split(glp)


def _fold(m, Fs, eos=()):
    rc, lp, gid, glp = _fold_rc(m, Fs, eos)
    _lib.check(rc)
    return lp, gid, glp


def _kv_rows(m, lo, hi):
    """layer 0's K / V rows of env 0 at positions [lo, hi), through the env's own table"""
    n = hi - lo
    K, V = np.zeros((max(n, 1), m.cfg.kv_heads, 128), np.float32), np.zeros((max(n, 1), m.cfg.kv_heads, 128), np.float32)
    if n > 0:
        _lib.check(m._lib.svln_op_kv_read(m._h, 0, lo, n, K.ctypes.data_as(PF), V.ctypes.data_as(PF)))
    return K[:n], V[:n]


# ------------------------------------------------------------------------------------------------------------ (c), (t), (s) on the shapes
_stats = {}


@DTYPES
@pytest.mark.parametrize("name,P,Tn,lens", FOLD_SHAPES, ids=[f"{s[0][:5]}-P{s[1]}-{'_'.join(map(str, s[3]))}" for s in FOLD_SHAPES])
def test_folded_scores_against_float64_the_unfolded_twin_and_the_continuation(name, P, Tn, lens, dtype):
    m = model(name, dtype)
    Fs = _candidates_of(m, P, Tn, lens)
    V, G, L, Wd = m.cfg.vocab, len(lens), P + Tn, _head(m)
    # the twin: the unfolded call
    _begin(m, P, Tn, 17)
    lp_u, gid_u, glp_u = _cands(m, Fs)
    hid_u = _taps(m, G)
    # the folded call
    _begin(m, P, Tn, 17)
    lp, gid, glp = _fold(m, Fs)
    hid = _taps(m, G)
    assert m.env_state(0) == (L, L)
    stats = dict(worst=0.0, rows=0, exempt=0, twin_rows=0, twin_exempt=0)
    for g in range(G):
        assert hid[g].shape[0] == min(lens[g], 8)
        _check_against_float64(Wd, Fs[g], lp[g], gid[g], glp[g], hid[g], 1.0, stats, (name, g))          # (c)
        assert all(float(lp[g][i]) <= float(glp[g][i]) + 1e-6 for i in range(lens[g]))
        b1, b2 = _bounds(Wd, hid[g], lens[g]), _bounds(Wd, hid_u[g], lens[g])
        for row, i in _tap_rows(lens[g]):                                                                 # (t)
            a, b = hid[g][row].astype(np.float64), hid_u[g][row].astype(np.float64)
            if dtype == torch.float32:
                assert float(np.abs(a - b).max()) <= HIDDEN_TOL, (name, g, i)
            else:
                assert float(np.linalg.norm(a - b) / np.linalg.norm(b)) < BF16_HIDDEN_REL[name], (name, g, i)
            if dtype == torch.float32 or i == 0:
                assert abs(float(lp[g][i]) - float(lp_u[g][i])) <= b1[i] + b2[i], (name, g, i, lp[g][i], lp_u[g][i])
            if dtype == torch.float32:
                # the two calls' logits of this row differ by at most delta = max_n |w_n . (a - b)| plus each call's own dot bound: where the
                # twin's float64 top-2 gap exceeds that on both sides, the two arg-maxes must agree; the rest is exempted and counted
                top = torch.topk(Wd @ torch.from_numpy(b), 2).values
                delta = float((Wd @ torch.from_numpy(a - b)).abs().max())
                stats["twin_rows"] += 1
                if float(top[0] - top[1]) > b1[i] + b2[i] + 2 * delta:
                    assert gid[g][i] == gid_u[g][i], (name, g, i)
                else:
                    stats["twin_exempt"] += 1
    _stats[(name, P, lens, dtype)] = stats
    # the group is the unfolded call's: svln_group_logprobs returns the same scores
    buf, k = np.zeros(32, np.float32), C.c_int32()
    for g in range(G):
        _lib.check(m._lib.svln_group_logprobs(m._h, g, buf.ctypes.data_as(PF), 32, C.byref(k)))
        assert k.value == lens[g] and buf[:lens[g]].tobytes() == lp[g].tobytes()
    # (s) the continuation after a select against the one after a forced turn
    nxt = _prompt(7, 5, V).tolist()
    for pick in sorted({0, G - 1}):
        if pick != 0:
            _begin(m, P, Tn, 17)
            _fold(m, Fs)
        assert _select(m, pick) == L + lens[pick] - 1 and m.env_state(0) == (L, L + lens[pick] - 1)
        _append(m, Fs[pick] + nxt)
        ids_c, hid_c, st_c = _fixed(m, 3), m.last_hidden(), m.env_state(0)
        _begin(m, P, Tn, 17)
        _forced(m, Fs[pick])
        _append(m, Fs[pick] + nxt)
        ids_t, hid_t, st_t = _fixed(m, 3), m.last_hidden(), m.env_state(0)
        assert st_c == st_t, (name, pick)
        if dtype == torch.float32:
            assert ids_c == ids_t and float(np.abs(hid_c - hid_t).max()) <= HIDDEN_TOL, (name, pick, ids_c, ids_t)
        else:
            rel = float(np.linalg.norm(hid_c[0] - hid_t[0]) / np.linalg.norm(hid_t[0]))
            assert rel < BF16_HIDDEN_REL[name], (name, pick, rel)
    print(f"folded candidates {name} P{P} {lens} [{dtype}]: worst |score - ref| / bound {stats['worst']:.3f}, exempt {stats['exempt']}/{stats['rows']}")


@DTYPES
def test_exempted_share_stays_under_a_tenth(dtype):
    """(c): over the rows of all shapes at most 10 % may fall under the exempted top-2 gap (the fixtures alone: test_candidates_host.py)"""
    rows = exempt = trows = texempt = 0
    for name, P, Tn, lens in FOLD_SHAPES:
        st = _stats.get((name, P, lens, dtype))
        if st is None:
            m = model(name, dtype)
            Fs = _candidates_of(m, P, Tn, lens)
            _begin(m, P, Tn, 17)
            lp, gid, glp = _fold(m, Fs)
            hid = _taps(m, len(lens))
            st = dict(worst=0.0, rows=0, exempt=0, twin_rows=0, twin_exempt=0)
            for g in range(len(lens)):
                _check_against_float64(_head(m), Fs[g], lp[g], gid[g], glp[g], hid[g], 1.0, st, (name, g))
            _select(m, 0)
        rows, exempt = rows + st["rows"], exempt + st["exempt"]
        trows, texempt = trows + st["twin_rows"], texempt + st["twin_exempt"]
    print(f"exempted rows, folded [{dtype}]: {exempt} of {rows} against float64, {texempt} of {trows} against the twin")
    assert rows >= 60 and exempt <= 0.10 * rows, (exempt, rows)
    assert texempt <= 0.10 * max(trows, 1), (texempt, trows)


# ------------------------------------------------------------------------------------------------------------ (s) every g, every residue
#: (history rows P, new rows Tn): L % 64 = 0, 1, 61, 63 on a first turn, and a second turn with P = 70 inside page q0 = 1 (L = 100)
SELECT_CASES = [(0, 128), (0, 129), (0, 189), (0, 191), (70, 30)]


@pytest.mark.parametrize("P,Tn", SELECT_CASES, ids=[f"P{p}-L{p + t}" for p, t in SELECT_CASES])
def test_every_selected_sequence_continues_as_its_forced_turn_and_reads_the_prompts_bits(P, Tn):
    m = model("tiny_episode", torch.float32)
    V, L, lens = m.cfg.vocab, P + Tn, (5, 1, 3, 6)
    q0 = L // 64
    Fs = [_prompt(n, 60 + g, V).tolist() for g, n in enumerate(lens)]
    nxt = _prompt(7, 5, V).tolist()
    rows = {}
    for g in range(len(lens)):
        _begin(m, P, Tn, 23)
        _fold(m, Fs)
        assert _select(m, g) == L + lens[g] - 1
        rows[g] = _kv_rows(m, q0 * 64, L)
        own = _kv_rows(m, L, L + lens[g] - 1)
        _append(m, Fs[g] + nxt)
        ids_c, hid_c, st_c = _fixed(m, 3), m.last_hidden(), m.env_state(0)
        _begin(m, P, Tn, 23)
        _forced(m, Fs[g])
        twin_own = _kv_rows(m, L, L + lens[g] - 1)
        _append(m, Fs[g] + nxt)
        ids_t, hid_t, st_t = _fixed(m, 3), m.last_hidden(), m.env_state(0)
        assert st_c == st_t and ids_c == ids_t, (P, Tn, g, ids_c, ids_t)
        assert float(np.abs(hid_c - hid_t).max()) <= HIDDEN_TOL, (P, Tn, g)
        # the branch's own rows are those of the forced turn up to rounding (layer 0: RoPE of the same q|k|v up to the products' plans)
        assert own[0].shape == twin_own[0].shape and float(np.abs(own[0] - twin_own[0]).max(initial=0.0)) <= HIDDEN_TOL
    for g in range(1, len(lens)):
        assert rows[g][0].tobytes() == rows[0][0].tobytes() and rows[g][1].tobytes() == rows[0][1].tobytes(), (P, Tn, g)
    assert rows[0][0].shape[0] == L - q0 * 64


# ------------------------------------------------------------------------------------------------------------ (i) independence
@DTYPES
def test_a_candidates_results_do_not_depend_on_its_neighbours(dtype):
    m = model("tiny_episode", dtype)
    V = m.cfg.vocab
    A, B, Cc, D = _prompt(5, 1, V).tolist(), _prompt(5, 2, V).tolist(), _prompt(3, 3, V).tolist(), _prompt(4, 4, V).tolist()
    _begin(m, 20, 42, 9)
    lp, gid, glp = _fold(m, [A, B, A])
    hid = _taps(m, 3)
    assert lp[0].tobytes() == lp[2].tobytes() and glp[0].tobytes() == glp[2].tobytes() and gid[0] == gid[2]
    assert np.array_equal(hid[0], hid[2]) and not np.array_equal(hid[0], hid[1]) and lp[0].tobytes() != lp[1].tobytes()
    _begin(m, 20, 42, 9)
    lp1, gid1, glp1 = _fold(m, [A, Cc, D])
    hid1 = _taps(m, 3)
    _begin(m, 20, 42, 9)
    lp2, gid2, glp2 = _fold(m, [D, Cc, A])
    hid2 = _taps(m, 3)
    _select(m, 2)
    for a, b in ((0, 2), (1, 1), (2, 0)):
        assert lp1[a].tobytes() == lp2[b].tobytes() and glp1[a].tobytes() == glp2[b].tobytes() and gid1[a] == gid2[b], (a, b)
        assert np.array_equal(hid1[a], hid2[b]), (a, b)
    assert lp1[0].tobytes() == lp[0].tobytes() and np.array_equal(hid1[0], hid[0])          # (other neighbours, the same bits)


# ------------------------------------------------------------------------------------------------------------ (f) shapes
@DTYPES
def test_all_ones_is_the_unfolded_call_bit_for_bit(dtype):
    m = model("tiny_episode", dtype)
    V = m.cfg.vocab
    Fs = [[int(t)] for t in _prompt(4, 77, V)]
    _begin(m, 20, 42, 9)
    lp_u, gid_u, glp_u = _cands(m, Fs)
    hid_u = _taps(m, 4)
    _begin(m, 20, 42, 9)
    lp, gid, glp = _fold(m, Fs)
    hid = _taps(m, 4)
    for g in range(4):
        assert lp[g].tobytes() == lp_u[g].tobytes() and glp[g].tobytes() == glp_u[g].tobytes() and gid[g] == gid_u[g]
        assert np.array_equal(hid[g], hid_u[g])
    assert _select(m, 3) == 62


@DTYPES
def test_sampling_scores_and_the_untouched_draw_counter(dtype):
    m = model("tiny_episode", dtype)
    T, seed, V, Wd = 0.5, 21, m.cfg.vocab, _head(m)
    inv_t = float(np.float32(1.0) / np.float32(T))
    Fs = [_prompt(5, 31, V).tolist(), _prompt(2, 32, V).tolist(), _prompt(5, 33, V).tolist()]
    nxt = _prompt(9, 8, V).tolist()
    m.set_sampling(T, seed)
    _begin(m, 0, 50, 7)
    lp, gid, glp = _fold(m, Fs)
    hid = _taps(m, 3)
    stats = dict(worst=0.0, rows=0, exempt=0)
    for g in range(3):
        _check_against_float64(Wd, Fs[g], lp[g], gid[g], glp[g], hid[g], inv_t, stats, ("sampling", g))
    _select(m, 2)
    _append(m, Fs[2] + nxt)
    ids2 = _generate(m, 5)
    # the twin ran no candidates call: a forced turn on F_2 (which consumes no draw), then the same sampled turn
    m.set_sampling(T, seed)
    _begin(m, 0, 50, 7)
    _forced(m, Fs[2])
    _append(m, Fs[2] + nxt)
    ids_t = _generate(m, 5)
    if dtype == torch.float32:
        assert ids_t == ids2
    assert len(ids_t) == len(ids2)
    m.set_sampling(None)
    _begin(m, 0, 50, 7)
    lp0, _, _ = _fold(m, Fs)
    _select(m, 0)
    assert lp0[0].tobytes() != lp[0].tobytes()


@DTYPES
def test_allowed_list(dtype):
    m = model("tiny_episode", dtype)
    V = m.cfg.vocab
    allowed = sorted(set(_prompt(40, 3, V).tolist()))
    Fs = [[allowed[3], allowed[17], allowed[0], allowed[-1], allowed[17]], [allowed[5]], [allowed[1], allowed[2]]]
    try:
        m.set_allowed_tokens(allowed, add_eos=False)
        _begin(m, 0, 50, 7)
        state = m.env_state(0)
        outside = next(t for t in range(5, V) if t not in allowed)
        rc = _fold_rc(m, [Fs[0], [allowed[1], outside]])[0]
        assert rc != 0 and b"allowed list" in m._lib.svln_last_error() and m.env_state(0) == state
        lp, gid, glp = _fold(m, Fs)
        for g, F in enumerate(Fs):
            buf, nr, nc = np.zeros(len(F) * len(allowed), np.float32), C.c_int32(), C.c_int32()
            _lib.check(m._lib.svln_group_dist(m._h, g, buf.ctypes.data_as(PF), len(F), C.byref(nr), C.byref(nc)))
            assert (nr.value, nc.value) == (len(F), len(allowed))
            alp = buf.reshape(len(F), len(allowed))
            for i, f in enumerate(F):
                assert lp[g][i].tobytes() == alp[i, allowed.index(f)].tobytes(), (g, i)
                assert gid[g][i] in allowed and gid[g][i] == allowed[int(np.argmax(alp[i]))]
                assert abs(float(glp[g][i]) - float(alp[i].max())) <= LSE_TOL
            assert abs(float(np.exp(alp.astype(np.float64)).sum(1).max()) - 1.0) <= 1e-4
        _select(m, 0)
    finally:
        m.set_allowed_tokens(None)


# ------------------------------------------------------------------------------------------------------------ (f) the pool
def test_twenty_calls_on_an_exactly_full_pool_leak_no_page():
    L, G, n, total = 64 + 63, 8, 5, 17                                # 3 own pages + 7 forks x 2 tail pages = the whole pool
    cfg = SCENARIOS["tiny_episode"]["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=1, max_frames=1, max_positions=total * 64)
    try:
        m.load_synthetic(SEED)
        pool = GR.Pool(total, 1)
        Fs = [_prompt(n, 90 + g, cfg.vocab).tolist() for g in range(G)]
        for it in range(20):
            _append(m, _prompt(L, 4, cfg.vocab))
            assert pool.can_fork(0, L, n, G)
            rc = _fold_rc(m, Fs)[0]
            assert rc == 0, (it, m._lib.svln_last_error())            # (a page lost by an earlier call would refuse this one)
            pool.fork(0, L, n, G)
            assert len(pool.free) == 0
            if it % 5 == 0:
                assert _held(m, total) == set(range(total))
            choice = (None, G - 1, 0, 3)[it % 4]
            if choice is None:
                m.reset(1)
                pool.reset_env(0)
                assert _held(m, total) == set()
                continue
            assert _select(m, choice) == L + n - 1
            pool.select(choice, [n] * G)
            assert len(pool.free) == total - 3 and pool.conserved()
            assert _held(m, total) == set(pool.env_pages[0]), (it, choice)
            m.reset(1)
            pool.reset_env(0)
        # a pool one page short refuses the call by name and keeps every page where it was
        _append(m, _prompt(L + 64, 4, cfg.vocab))
        rc = _fold_rc(m, Fs)[0]
        assert rc != 0 and b"free KV pages" in m._lib.svln_last_error() and m.env_state(0) == (L + 64, 0)
        assert _held(m, total) == set()
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_engine_as_the_unfolded_calls_do():
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.bfloat16, max_envs=2, max_frames=3, max_positions=256)
    try:
        m.load_synthetic(SEED)
        V = m.cfg.vocab
        A, B = [11, 12, 13], [21, 22]
        free = C.c_int32()

        def pages():
            _lib.check(m._lib.svln_kv_free_pages(m._h, C.byref(free)))
            return free.value

        def refused(Fs, match, eos=()):
            """the folded call is refused with `match`; ids, kv_len and the pages stay, no group is pending -- and the unfolded call is
            refused in the same state with the same reason"""
            state, held = m.env_state(0), pages()
            for call in (_fold_rc, _cands_rc):
                rc = call(m, Fs, eos)[0]
                err = m._lib.svln_last_error().decode()
                assert rc != 0 and match in err, (call.__name__, Fs, match, err)
                assert m.env_state(0) == state and pages() == held
                out, n_out = np.zeros(4, np.float32), C.c_int32()
                assert m._lib.svln_group_logprobs(m._h, 0, out.ctypes.data_as(PF), 4, C.byref(n_out)) != 0        # no group is pending

        m.reset(1)
        refused([A, B], "nothing to prefill")
        _begin(m, 0, 40, 1)
        refused([A], "2 .. 8")
        refused([A] * 9, "2 .. 8")
        refused([A, []], "1 .. 32")
        refused([A, list(range(5, 38))], "1 .. 32")
        refused([A, [11, V]], "outside the vocabulary")
        refused([A, [11, 12, 13]], "EOS", eos=(12,))
        _begin(m, 0, 240, 1)
        refused([B, list(range(5, 23))], "max_positions")                     # 240 + 18 - 1 > 256
        # the new refusal, by name: 236 new rows + 2 x 16 row slots > 256 rows of workspace; the unfolded call takes the same input
        _begin(m, 0, 236, 1)
        state, held = m.env_state(0), pages()
        rc = _fold_rc(m, [A, B])[0]
        err = m._lib.svln_last_error().decode()
        assert rc != 0 and "svln_generate_candidates_folded" in err and "row workspace" in err, err
        assert m.env_state(0) == state and pages() == held
        _cands(m, [A, B])
        assert _select(m, 0) == 238
        _begin(m, 0, 40, 1)
        _lib.check(m._lib.svln_set_repetition_penalty(m._h, 1.3))
        refused([A, B], "svln_set_repetition_penalty")
        _lib.check(m._lib.svln_set_repetition_penalty(m._h, 1.0))
        for sym, fn in {"svln_set_fp8_decode": m.set_fp8_decode, "svln_set_mxfp4_decode": m.set_mxfp4_decode, "svln_set_fp8_gemm": m.set_fp8_gemm,
                        "svln_set_decode_persistent": m.set_decode_persistent, "svln_set_mxfp4_batched": m.set_mxfp4_batched}.items():
            fn(True)
            refused([A, B], sym)
            fn(False)
        m.set_token_scores(True)
        m.set_top_logprobs(4)
        refused([A, B], "svln_top_logprobs")
        m.set_top_logprobs(0)
        m.set_token_scores(False)
        # a group already pending: the second call is refused
        m.reset(1)
        _begin(m, 0, 40, 1)
        _fold(m, [A, B])
        rc = _fold_rc(m, [A, B])[0]
        assert rc != 0 and "svln_group_select" in m._lib.svln_last_error().decode()
        ids = np.arange(10, 30, dtype=np.int64)
        assert m._lib.svln_append_turn(m._h, 0, ids.ctypes.data_as(PI64), 3, 0) != 0
        m.reset(1)
        # the armed-draft rule: the call consumes an armed draft, whether it runs or is refused after entry, as the unfolded call does
        m.set_prefill_draft(True)
        for call, Fs in ((_fold_rc, [A, B]), (_fold_rc, [A]), (_cands_rc, [A])):
            _begin(m, 0, 40, 1)
            d = np.asarray([21, 22, 23], np.int64)
            _lib.check(m._lib.svln_set_draft(m._h, 0, d.ctypes.data_as(PI64), 3))
            rc = call(m, Fs)[0]
            assert (rc == 0) == (len(Fs) == 2)
            if rc == 0:
                _select(m, 0)
                _append(m, A + [31, 32])
            _fixed(m, 2)
            assert m.prefill_draft_stats(reset=True) == (0, 0, 0), (call.__name__, Fs)
        m.set_prefill_draft(False)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------ the Python surface, the agent
def test_generate_and_the_agent_attribute():
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    m = model(name, torch.float32)

    def agent():
        m.reset(1)
        enc = SyntheticPromptEncoder(sc["cfg"], seed=7, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        return StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"],
                              max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=m.get_vision_tower().image_processor.preprocess_array,
                              device="cuda")

    F = list(gold[0])
    alt = F[:-1] + [_other(F[-1], sc)]
    calls = []
    for fold in (False, True):
        a = agent()
        assert a.fold_candidates is False
        a.fold_candidates = fold
        turn = m._lib.svln_turn_candidates_folded if fold else m._lib.svln_turn_candidates
        seen = []
        spy = lambda *args, _t=turn: (seen.append(1), _t(*args))[1]
        setattr(m._lib, "svln_turn_candidates_folded" if fold else "svln_turn_candidates", spy)
        try:
            a.act_candidates(synthetic_frame(0, 0), candidate_ids=[alt, F])
        finally:
            setattr(m._lib, "svln_turn_candidates_folded" if fold else "svln_turn_candidates", turn)
        assert seen == [1], fold                                          # the attribute chose the entry
        out = a.turn_log[-1]["out"]
        assert a.last_candidate_index == 1 and out.sequences[0].tolist() == F and a.last_greedy_ids[0].tolist() == F
        assert m.env_state(0)[1] == int(g["t0_cache_len"])
        calls.append(np.asarray(a.last_candidate_logprobs, dtype=np.float64))
    assert float(np.abs(calls[0] - calls[1]).max()) <= 1e-3
