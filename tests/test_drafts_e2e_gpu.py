"""Multi-draft turns (generate(draft_set=...) / svln_generate_drafts) on the GPU.

(a) every turn of the fixture episodes on the fp32 engine under ten kinds of draft set: the ids are the fixtures', the hidden rows within
    1e-3, the cache lengths the fixtures' across a window restart, and the eight counters are drafts_ref.simulate's;
(b) the bit pin against the folded candidates call on the same prompt with drafts equal to the candidates' fed ids, fp32 and bf16, at
    L % 64 = 0, 1, 61, 63 and with P > 64 q0: tap rows, emitted ids, layer-0 K / V rows [64 q0, kv_len) and the next plain turn;
(c) ignored hints: under every ignore condition ids, hidden rows and the env's layer-0 K / V rows are bit-identical to svln_generate;
(d) scores on: every log-probability inside the a-priori bound of float64 from the call's own tap rows, ids unchanged;
(e) the bf16 engine with right drafts under the bounds and the margin rule of test_bf16_mode_vs_golden;
(f) the pool: twenty calls on an exactly full pool, drafts dropped for pages and for rows, a prompt ending at max_positions - 2;
(g) the agent with draft_history = 4 acts as the plain agent."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ref as AR
import drafts_ref as R
from scenarios import SCENARIOS, SEED, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from test_candidates_e2e_gpu import _select
from test_candidates_fold_gpu import _fold, _kv_rows
from test_e2e_gpu import BF16_HIDDEN_REL, BF16_MARGIN, HIDDEN_TOL
from test_forced_e2e_gpu import MAX_POSITIONS, _append, _begin, _close_models, _fixed, _forced, _generate, _head, _prompt, _ref_scores, _token_scores, model  # noqa: F401
from test_prefill_draft_gpu import _other, variant
from util import load_golden

pytestmark = pytest.mark.gpu
PI64, PF, PI32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
POOL_PAGES = MAX_POSITIONS // 64                 # the page pool of the shared one-env engines


def _drafts_rc(m, drafts, max_new, eos=()):
    flat = np.ascontiguousarray(np.concatenate([np.asarray(d, np.int64).reshape(-1) for d in drafts] + [np.zeros(1, np.int64)]))
    lens = np.asarray([len(d) for d in drafts] + [0], np.int32)
    e = np.ascontiguousarray(eos, dtype=np.int64)
    out, n, win, ptok = np.full(max_new, -7, np.int64), C.c_int32(), C.c_int32(-9), C.c_int32(-9)
    rc = m._lib.svln_generate_drafts(m._h, 0, len(drafts), flat.ctypes.data_as(PI64), lens.ctypes.data_as(PI32), max_new,
                                     e.ctypes.data_as(PI64) if e.size else None, int(e.size), out.ctypes.data_as(PI64), max_new, C.byref(n),
                                     C.byref(win), C.byref(ptok))
    return rc, out[:max(n.value, 0)].tolist(), win.value, ptok.value


def _drafts(m, drafts, max_new, eos=()):
    rc, ids, win, ptok = _drafts_rc(m, drafts, max_new, eos)
    _lib.check(rc)
    return ids, win, ptok


def _delta(m, before):
    return tuple(a - b for a, b in zip(m.drafts_stats(), before))


def _free(m):
    n = C.c_int32()
    _lib.check(m._lib.svln_kv_free_pages(m._h, C.byref(n)))
    return n.value


def _oracle(gold):
    """the policy as a next-token function of the ids emitted so far (a row whose prefix is wrong is never read by the rule)"""
    return lambda pre: gold[len(pre)] if list(pre) == gold[:len(pre)] and len(pre) < len(gold) else -5


# ------------------------------------------------------------------------------------------------------------ (a) fixture episodes
def _sets(gold, sc):
    v = lambda kind: variant(kind, gold, sc)
    # right for two ids, then wrong
    two = gold[:2] + [_other(gold[2], sc)] + gold[3:] if len(gold) > 2 else v("wrong_at_last")
    return {
        "right_first": [v("right"), v("wrong_at_0"), v("short"), v("long")],
        "right_last": [v("wrong_at_0"), v("wrong_at_1"), v("eos_early"), v("right")],
        "none_right": [v("wrong_at_0"), v("wrong_at_0")[:1], v("wrong_at_0")[::-1]],
        "two_then_wrong": [v("wrong_at_0"), two],
        "short": [v("short"), gold[:1]],
        "long": [v("long") + v("long"), v("eos_missing")],
        "eos": [v("eos_early"), v("eos_missing"), v("wrong_at_0")],
        "oov": [v("oov_mid"), [sc["cfg"].vocab + 1] + gold[1:], [-1]],
        "duplicated": [v("right")] * 3 + [v("wrong_at_1")] * 2,
        "empty": [[], []],
        "eight": [v("wrong_at_0"), v("wrong_at_1"), v("short"), v("oov_mid"), v("eos_early"), [], v("wrong_at_last"), v("right")],
    }


class _WithSets:
    def __init__(self, m, sets):
        self._m, self._sets, self.turn = m, sets, 0

    def __getattr__(self, k):
        return getattr(self._m, k)

    def generate(self, *a, **kw):
        kw["draft_set"] = self._sets(self.turn)
        self.turn += 1
        # what the plan will see: a new window starts from an empty cache (its pages are back in the pool before the pass is planned)
        new_window = kw.get("past_key_values") is None
        held = 0 if new_window else POOL_PAGES - _free(self._m)
        self.pre = dict(P=0 if new_window else self._m.env_state(0)[1], env_pages=held, free_pages=POOL_PAGES - held)
        return self._m.generate(*a, **kw)


def _run(m, sc, sets, steps=None):
    taps, before = [], [m.drafts_stats()]
    wrapped = _WithSets(m, sets)

    def on_turn(t, rec):
        ne, kl = m.env_state(0)
        out = rec["out"]
        taps.append(dict(ids=out.sequences[0].tolist(), hidden=m.last_hidden(), cache_len=kl, n_embeds=ne, stats=_delta(m, before[0]),
                         winner=out.draft_index, pass_tokens=out.draft_tokens, **wrapped.pre))
        before[0] = m.drafts_stats()
    run_scenario(wrapped, sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda", steps=steps)
    return taps


KINDS = ["right_first", "right_last", "none_right", "two_then_wrong", "short", "long", "eos", "oov", "duplicated", "empty", "eight"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode"])
def test_fp32_fixture_draft_sets(name, kind):
    sc, g = SCENARIOS[name], load_golden(name)
    cfg = sc["cfg"]
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    sets = lambda t: _sets(gold[t], sc)[kind]
    m = model(name, torch.float32)
    taps = _run(m, sc, sets)
    assert len(taps) == len(gold)
    passes = 0
    for t, tap in enumerate(taps):
        assert tap["ids"] == gold[t], (name, kind, t, tap["ids"], gold[t])
        assert np.abs(tap["hidden"] - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, (name, kind, t, "hidden")
        assert tap["cache_len"] == int(g[f"t{t}_cache_len"]), (name, kind, t)
        L = tap["n_embeds"]
        want = R.simulate(_oracle(gold[t]), (), [list(d) for d in sets(t)], L, tap["P"], sc["max_new"], MAX_POSITIONS, cfg.vocab, set(eos_ids(sc)),
                          cfg.q_heads // cfg.kv_heads, free_pages=tap["free_pages"], env_pages=tap["env_pages"])
        assert want["ids"] == gold[t] and tap["stats"] == tuple(want["counters"][k] for k in R.COUNTERS), (name, kind, t, tap["stats"], want)
        assert (tap["winner"], tap["pass_tokens"]) == (want["winner"], want["pass_tokens"]), (name, kind, t)
        passes += tap["stats"][1]
    assert (passes == 0) if kind == "empty" else (passes >= 1), (name, kind, passes)
    if kind in ("right_first", "right_last"):
        # a right draft finishes the turn in the pass: no single step (r = 8 / 4 row slots hold the fixtures' turns) -- unless the plan
        # dropped it: the last turns of true1_episode's window and its restart leave too few free pages for three forks
        for t, tap in enumerate(taps):
            n = len(gold[t])
            G = R.plan([list(d) for d in sets(t)], tap["n_embeds"], tap["P"], sc["max_new"], MAX_POSITIONS, cfg.vocab, set(eos_ids(sc)),
                       cfg.q_heads // cfg.kv_heads, tap["free_pages"], tap["env_pages"])[0]
            assert G >= 2, (name, t, G)
            if n >= 2 and (G == 4 or kind == "right_first"):
                assert tap["stats"][1] == 1 and tap["stats"][2] == n and tap["stats"][4] == 1 and tap["stats"][7] == 0, (t, tap["stats"])


# ------------------------------------------------------------------------------------------------------------ (b) the bit pin
PIN_CASES = [(0, 128), (0, 129), (0, 189), (0, 191), (70, 30)]


@DTYPES
@pytest.mark.parametrize("P,Tn", PIN_CASES, ids=[f"P{p}-L{p + t}" for p, t in PIN_CASES])
def test_the_pass_is_the_folded_candidates_pass_bit_for_bit(P, Tn, dtype):
    m = model("tiny_episode", dtype)
    V, L = m.cfg.vocab, P + Tn
    q0 = L // 64
    _begin(m, P, Tn, 23)
    true = _fixed(m, 5)
    other = [t for t in _prompt(40, 61, V).tolist() if t not in true]
    # candidates of 5, 5, 3 and 2 ids; the drafts are the ids they feed (all but the last), max_new = 5: k_g = lens[g] - 1, the same rows
    Fs = [other[:5], list(true), true[:2] + other[5:6], other[6:8]]
    Ds = [f[:-1] for f in Fs]
    nxt = _prompt(7, 5, V).tolist()
    _begin(m, P, Tn, 23)
    _, gid, _ = _fold(m, Fs)
    group_taps = [m.last_hidden_group(g) for g in range(4)]
    _begin(m, P, Tn, 23)
    before = m.drafts_stats()
    ids, win, ptok = _drafts(m, Ds, 5)
    st = _delta(m, before)
    hid = m.last_hidden()
    assert st[1] == 1 and st[3] == 4 + 4 + 2 + 1 and ptok >= 1 and 0 <= win < 4, (st, win, ptok)
    # the emitted ids are the winner's greedy ids, and its tap rows are the group's, bit for bit
    assert ids[:ptok] == gid[win][:ptok], (ids, gid, win)
    assert hid[:ptok].tobytes() == group_taps[win][:ptok].tobytes(), (P, Tn, "tap rows")
    if dtype == torch.float32:
        assert (ids, win, ptok) == (true, 1, 5), (ids, true, win, ptok)
    if ptok == len(Fs[win]) and len(ids) == ptok:
        # the turn ended in the pass on the winner's own ids: the env is where select_sequence(winner) leaves the candidates call
        kv = m.env_state(0)[1]
        assert kv == L + ptok - 1
        rows_d = _kv_rows(m, q0 * 64, kv)
        _append(m, ids + nxt)
        ids_c, hid_c, st_c = _fixed(m, 3), m.last_hidden(), m.env_state(0)
        _begin(m, P, Tn, 23)
        _fold(m, Fs)
        assert _select(m, win) == kv
        rows_s = _kv_rows(m, q0 * 64, kv)
        assert rows_d[0].tobytes() == rows_s[0].tobytes() and rows_d[1].tobytes() == rows_s[1].tobytes(), (P, Tn, "K / V rows")
        # the next plain turn is the one that follows a forced turn on the emitted ids
        _begin(m, P, Tn, 23)
        _forced(m, ids)
        _append(m, ids + nxt)
        ids_t, hid_t, st_t = _fixed(m, 3), m.last_hidden(), m.env_state(0)
        assert st_c == st_t, (st_c, st_t)
        if dtype == torch.float32:
            assert ids_c == ids_t and float(np.abs(hid_c - hid_t).max()) <= HIDDEN_TOL, (P, Tn, ids_c, ids_t)
    else:
        assert dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------------------ (c) ignored hints
def _pool0(m):
    """layer 0's K / V rows of everything the env has cached, through its own page table"""
    K, V = _kv_rows(m, 0, m.env_state(0)[1])
    return K.tobytes() + V.tobytes()


def _penalty(m, p):
    m.generation_config.repetition_penalty = p
    m._sync_call_config()


IGNORE = {
    "sampling": (lambda m: m.set_sampling(0.8, seed=3), lambda m: m.set_sampling(None)),
    "penalty": (lambda m: _penalty(m, 1.3), lambda m: _penalty(m, 1.0)),
    "fp8_decode": (lambda m: m.set_fp8_decode(True), lambda m: m.set_fp8_decode(False)),
    "mxfp4_decode": (lambda m: m.set_mxfp4_decode(True), lambda m: m.set_mxfp4_decode(False)),
    "fp8_gemm": (lambda m: m.set_fp8_gemm(True), lambda m: m.set_fp8_gemm(False)),
    "persistent": (lambda m: m.set_decode_persistent(True), lambda m: m.set_decode_persistent(False)),
    "top_logprobs": (lambda m: (m.set_token_scores(True), m.set_top_logprobs(2)), lambda m: (m.set_top_logprobs(0), m.set_token_scores(False))),
    "entropy": (lambda m: (m.set_token_scores(True), m.set_token_entropy(True)), lambda m: (m.set_token_entropy(False), m.set_token_scores(False))),
    "scores_and_allowed": (lambda m: (m.set_allowed_tokens(list(range(10, 400, 3)), add_eos=False), m.set_token_scores(True)),
                           lambda m: (m.set_token_scores(False), m.set_allowed_tokens(None))),
    "no_usable_first_id": (lambda m: None, lambda m: None),
    "empty_set": (lambda m: None, lambda m: None),
}


@pytest.mark.parametrize("cond", list(IGNORE))
def test_ignored_hints_are_the_plain_call_bit_for_bit(cond):
    name = "true1_episode" if cond == "persistent" else "tiny_episode"          # (the persistent layer covers the true dimensions only)
    m = model(name, torch.bfloat16)
    V = m.cfg.vocab
    on, off = IGNORE[cond]
    on(m)
    try:
        m.reset(1)
        _lib.check(m._lib.svln_op_fill_attn_state(m._h, C.c_float(AR.SENTINEL), 0))
        _append(m, _prompt(100, 31, V))
        plain = _generate(m, 5)
        hid_p, st_p, pool_p = m.last_hidden(), m.env_state(0), _pool0(m)
        drafts = {"no_usable_first_id": [[V + 3, plain[1]], [], [-1]], "empty_set": []}.get(cond, [plain, plain[:2], [plain[0] + 1 if plain[0] + 1 < V else 5]])
        off(m); on(m)                                                            # (a sampled twin starts from the same draw counter)
        m.reset(1)
        _lib.check(m._lib.svln_op_fill_attn_state(m._h, C.c_float(AR.SENTINEL), 0))
        _append(m, _prompt(100, 31, V))
        before = m.drafts_stats()
        ids, win, ptok = _drafts(m, drafts, 5)
        st = _delta(m, before)
        assert ids == plain and (win, ptok) == (-1, 0), (cond, ids, plain, win, ptok)
        assert st == (1, 0, 0, 0, 0, 1, 0, len(plain) - 1), (cond, st)
        assert m.last_hidden().tobytes() == hid_p.tobytes() and m.env_state(0) == st_p and _pool0(m) == pool_p, cond
    finally:
        off(m)


# ------------------------------------------------------------------------------------------------------------ (d) scores on
@DTYPES
def test_scores_ride_the_pass_inside_the_bound(dtype):
    m = model("tiny_episode", dtype)
    V = m.cfg.vocab
    Wd = _head(m)
    _begin(m, 20, 80, 41)
    plain = _fixed(m, 5)
    wrong = [t for t in _prompt(20, 77, V).tolist() if t not in plain]
    m.set_token_scores(True)
    try:
        for drafts, pass_tokens in (([wrong[:3], plain], 5), ([plain[:2] + wrong[:2], wrong[3:5]], 3), ([plain[:3]], 4)):
            _begin(m, 20, 80, 41)
            ids, win, ptok = _drafts(m, drafts, 5)
            if dtype == torch.float32:
                assert ids == plain and ptok == pass_tokens, (ids, plain, ptok)
            lp, hid = _token_scores(m, len(ids)), m.last_hidden()
            for i, (want, arg, bound) in enumerate(_ref_scores(Wd, hid, ids)):
                print(f"multi-draft scores [{dtype}] token {i} ({'pass' if i < ptok else 'step'}): {lp[i]:.6f} vs float64 {want:.6f}, bound {bound:.2e}")
                assert abs(float(lp[i]) - want) <= bound, (drafts, i, lp[i], want, bound)
    finally:
        m.set_token_scores(False)
    _begin(m, 20, 80, 41)
    assert _drafts(m, [wrong[:3], plain], 5)[0] == plain or dtype == torch.bfloat16


def test_scores_with_an_allowed_list_alone_ride_too():
    m = model("tiny_episode", torch.float32)
    m.set_allowed_tokens(list(range(10, 400, 3)), add_eos=False)
    try:
        _begin(m, 0, 90, 43)
        plain = _fixed(m, 5)
        _begin(m, 0, 90, 43)
        ids, win, ptok = _drafts(m, [[11, 12], plain], 5)
        assert (ids, win, ptok) == (plain, 1, 5)
    finally:
        m.set_allowed_tokens(None)


# ------------------------------------------------------------------------------------------------------------ (e) bf16
@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode"])
def test_bf16_fixture_right_drafts(name):
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    m = model(name, torch.bfloat16)
    taps = _run(m, sc, lambda t: [variant("wrong_at_0", gold[t], sc), gold[t]])
    assert len(taps) == len(gold)
    rows = passes = 0
    diverged = False
    for t, tap in enumerate(taps):
        ids, margins = tap["ids"], g[f"t{t}_margins"]
        passes += tap["stats"][1]
        n = 0
        while n < min(len(ids), len(gold[t])) and ids[n] == gold[t][n]:
            n += 1
        if diverged:
            continue
        for j in range(min(n + 1, len(gold[t]), len(ids))):
            h, gh = tap["hidden"][j], g[f"t{t}_hidden"][j]
            rel = float(np.linalg.norm(h - gh) / np.linalg.norm(gh))
            print(f"bf16 multi-draft [{name}] turn {t} row {j}: rel L2 {rel:.3e}")
            rows += 1
            assert rel < BF16_HIDDEN_REL[name], (name, t, j, rel)
            if j < len(margins) and margins[j] > BF16_MARGIN:
                assert ids[j] == gold[t][j], (name, t, j, ids, gold[t], margins)
        diverged = n < len(gold[t])
    assert rows >= 1 and passes >= 1


# ------------------------------------------------------------------------------------------------------------ (f) pool and range
def test_twenty_calls_on_an_exactly_full_pool_and_dropped_drafts():
    L, total = 64 + 63, 17                                            # 3 own pages + 7 forks x 2 tail pages = the whole pool
    cfg = SCENARIOS["tiny_episode"]["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=1, max_frames=1, max_positions=total * 64)
    try:
        m.load_synthetic(SEED)
        V = cfg.vocab
        assert _free(m) == total
        _append(m, _prompt(L, 4, V))
        plain = _generate(m, 5)
        m.reset(1)
        junk = [t for t in _prompt(60, 9, V).tolist() if t not in plain]
        for it in range(20):
            w = it % 8
            drafts = [junk[4 * g:4 * g + 4] for g in range(8)]
            drafts[w] = plain[:4] if it % 3 else plain[:2] + junk[40:42]       # right (the turn ends in the pass), or right for two ids
            _append(m, _prompt(L, 4, V))
            want = R.plan(drafts, L, 0, 5, total * 64, V, set(), cfg.q_heads // cfg.kv_heads, total, 0)
            assert want == (8, 4, [4] * 8)
            before = m.drafts_stats()
            ids, win, ptok = _drafts(m, drafts, 5)
            st = _delta(m, before)
            assert ids == plain and win == w and ptok == (5 if it % 3 else 3), (it, ids, plain, win, ptok)
            assert st[1] == 1 and st[3] == 32 and st[6] == int(w >= 1), (it, st)
            assert _free(m) == total - 3, (it, _free(m))                        # every fork page and the displaced tail are back
            m.reset(1)
            assert _free(m) == total, it
        # one page more for the env: the last draft is dropped, the right one still rides; two right ones, the earlier wins
        drafts = [junk[4 * g:4 * g + 4] for g in range(8)]
        drafts[6] = drafts[7] = plain[:4]
        _append(m, _prompt(L + 64, 4, V))
        plain2 = _generate(m, 5)
        m.reset(1)
        drafts[6] = plain2[:4]
        drafts[7] = plain2[:4]
        _append(m, _prompt(L + 64, 4, V))
        assert R.plan(drafts, L + 64, 0, 5, total * 64, V, set(), cfg.q_heads // cfg.kv_heads, total, 0) == (7, 4, [4] * 7)
        before = m.drafts_stats()
        ids, win, ptok = _drafts(m, drafts, 5)
        assert (ids, win, ptok) == (plain2, 6, 5) and _delta(m, before)[3] == 28
        m.reset(1)
        assert _free(m) == total
    finally:
        m.close()


def test_row_workspace_drops_drafts_and_the_last_positions_stay_in_range():
    cfg = SCENARIOS["tiny_episode"]["cfg"]
    gq = cfg.q_heads // cfg.kv_heads
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=4, max_frames=1, max_positions=256)
    try:
        m.load_synthetic(SEED)
        V = cfg.vocab
        # 240 new rows: only one draft's 16 row slots fit the 256-row workspace
        _append(m, _prompt(240, 4, V))
        plain = _generate(m, 5)
        m.reset(1)
        junk = [t for t in _prompt(60, 9, V).tolist() if t not in plain]
        drafts = [plain[:4], junk[:4], junk[4:8]]
        _append(m, _prompt(240, 4, V))
        assert R.plan(drafts, 240, 0, 5, 256, V, set(), gq, 16, 0) == (1, 16, [4])
        before = m.drafts_stats()
        assert _drafts(m, drafts, 5) == (plain, 0, 5) and _delta(m, before)[3] == 4
        m.reset(1)
        _append(m, _prompt(240, 4, V))
        before = m.drafts_stats()
        assert _drafts(m, drafts[::-1], 5) == (plain, 0, 1) and _delta(m, before)[1:4] == (1, 1, 4)      # the right draft was dropped
        # a prompt that ends at max_positions - 2: two rows per draft at the most, nothing written outside the env's and the forks' pages
        m.reset(1)
        _lib.check(m._lib.svln_op_fill_attn_state(m._h, C.c_float(AR.SENTINEL), 0))
        _append(m, _prompt(200, 5, V))
        _fixed(m, 1)
        _append(m, _prompt(54, 6, V))
        assert m.env_state(0) == (254, 200)
        plain = _generate(m, 3)
        m.reset(1)
        _lib.check(m._lib.svln_op_fill_attn_state(m._h, C.c_float(AR.SENTINEL), 0))
        _append(m, _prompt(200, 5, V))
        _fixed(m, 1)
        _append(m, _prompt(54, 6, V))
        junk = [t for t in _prompt(80, 9, V).tolist() if t not in plain]
        drafts = [junk[6 * g:6 * g + 6] for g in range(7)] + [plain + junk[50:53]]
        assert R.plan(drafts, 254, 200, 3, 256, V, set(), gq, 12, 4) == (8, 4, [2] * 8)
        before = m.drafts_stats()
        assert _drafts(m, drafts, 3) == (plain, 7, 3) and _delta(m, before)[3] == 16 and m.env_state(0) == (254, 256)
        K = np.zeros((16 * 64, cfg.kv_heads, 128), np.float32)
        Vv = np.zeros_like(K)
        _lib.check(m._lib.svln_op_kv_read(m._h, -1, 0, 16 * 64, K.ctypes.data_as(PF), Vv.ctypes.data_as(PF)))
        written = (K != np.float32(AR.SENTINEL)).any((1, 2)) | (Vv != np.float32(AR.SENTINEL)).any((1, 2))
        pages = np.nonzero(written.reshape(-1, 64).any(1))[0]
        # the env's four pages and seven private copies of page 3 (rows 192 .. 255 each), no row anywhere else
        assert len(pages) == 11 and written.sum() == 256 + 7 * 64, (pages, written.sum())
        with pytest.raises(_lib.SvlnError, match="sequence exceeds max_positions"):
            m.reset(1)
            _append(m, _prompt(254, 5, V))
            _drafts(m, drafts, 6)
        m.reset(1)
        assert _free(m) == 16
    finally:
        m.close()


def test_malformed_calls_are_refused_by_name():
    m = model("tiny_episode", torch.float32)
    _begin(m, 0, 40, 3)
    free = _free(m)
    for drafts, words in (([[1]] * 9, "n_drafts must be 0 .. 8"), ([[1] * 33], "must be 0 .. 32")):
        rc, *_ = _drafts_rc(m, drafts, 4)
        assert rc != 0 and "svln_generate_drafts" in m._lib.svln_last_error().decode() and words in m._lib.svln_last_error().decode()
    out, n = np.zeros(4, np.int64), C.c_int32()
    lens = np.asarray([2], np.int32)
    assert m._lib.svln_generate_drafts(m._h, 0, 1, None, lens.ctypes.data_as(PI32), 4, None, 0, out.ctypes.data_as(PI64), 4, C.byref(n), None, None) != 0
    assert "null draft ids" in m._lib.svln_last_error().decode()
    assert m._lib.svln_generate_drafts(m._h, 0, 1, out.ctypes.data_as(PI64), lens.ctypes.data_as(PI32), 4, None, 0, None, 4, C.byref(n), None, None) != 0
    assert "null output pointer" in m._lib.svln_last_error().decode()
    assert m.env_state(0) == (40, 0) and _free(m) == free
    # what svln_generate refuses is refused the same way: nothing to prefill
    ids = _drafts(m, [[5, 6]], 3)[0]
    rc, *_ = _drafts_rc(m, [[5, 6]], 3)
    assert rc != 0 and "nothing to prefill" in m._lib.svln_last_error().decode() and len(ids) == 3


# ------------------------------------------------------------------------------------------------------------ (g) the agent
def test_agent_with_a_draft_history_acts_as_the_plain_agent():
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    m = model(name, torch.float32)
    cfg = sc["cfg"]
    acts = {}
    for G in (0, 4):
        m.reset(1)
        enc = SyntheticPromptEncoder(cfg, seed=sc.get("prompt_seed", 7), first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        agent = StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"],
                               max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc),
                               preprocess=m.get_vision_tower().image_processor.preprocess_array, device="cuda",
                               decode_actions=lambda ids: ([int(t) % 4 for t in ids.reshape(-1).tolist()] + [1] * sc["nfs"])[:sc["nfs"]])
        agent.draft_history = G
        before = m.drafts_stats()
        acts[G] = [agent.act(synthetic_frame(0, step)) for step in range(sc["steps"])]
        turns = [rec["out"].sequences[0].tolist() for rec in agent.turn_log]
        assert turns == [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))], G
        st = _delta(m, before)
        assert (st[0] == 0) if G == 0 else (st[0] == len(turns) and st[5] >= 1), (G, st)      # (the first turn has no history: ignored)
        assert len(agent.turn_history) <= 8 and (G == 0) == (agent.turn_history == [])
    assert acts[0] == acts[4]
