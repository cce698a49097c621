"""Drafts inside the prefill pass (svln_set_prefill_draft) on the GPU.  A ride is a prefill whose last k rows are the draft's first k
ids: (1) it must be, bit for bit, the plain prefill of the same rows spliced on by the caller -- probe buffers of the last layer, the
final-norm rows and the arg-max of every head row; (2) whole episodes with drafts armed reproduce the golden fixtures whatever the draft
says, with the counters of prefill_draft_ref.simulate; (3) capacity, top-2, refusals and the cases in which the mode must change nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import prefill_draft_ref as PR
import verify_ref as VR
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM
from test_e2e_gpu import BF16_HIDDEN_REL, BF16_MARGIN, HIDDEN_TOL, _note
from util import load_golden

pytestmark = pytest.mark.gpu
MAX_POSITIONS = 2048
PI64 = C.POINTER(C.c_int64)
_models = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def model(name, dtype):
    """one engine per (scenario knobs, dtype) for the module; every run starts from reset(1) with both draft modes off, counters at zero"""
    sc = SCENARIOS[name]
    key = (sc["cfg"].name, dtype, sc["num_history"], sc.get("tml"), sc.get("rep_penalty"))
    if key not in _models:
        m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=1, max_frames=1 + (sc["num_history"] or 0), max_positions=MAX_POSITIONS)
        m.load_synthetic(SEED)
        m.model.num_history = sc["num_history"]
        apply_knobs(m, sc)
        _models[key] = m
    m = _models[key]
    modes(m, False, 0)
    m.reset(1)
    return m


def modes(m, ride, rows):
    m.set_prefill_draft(ride)
    m.set_speculative(rows)
    m.draft_stats(reset=True)
    m.prefill_draft_stats(reset=True)


class Drafted:
    """the model with draft_ids added to generate: turn t of the episode is armed with drafts(t) (None = no draft)"""

    def __init__(self, m, drafts):
        self._m, self._drafts, self.turn = m, drafts, 0

    def __getattr__(self, k):
        return getattr(self._m, k)

    def generate(self, *a, **kw):
        d = self._drafts(self.turn)
        self.turn += 1
        if d is not None:
            kw["draft_ids"] = d
        return self._m.generate(*a, **kw)


def run(m, sc, drafts, steps=None):
    """the scenario with per-turn drafts -> per turn: ids, hidden rows, cache_len, n_embeds, the six counters of the turn"""
    taps = []

    def on_turn(t, rec):
        ne, kl = m.env_state(0)
        taps.append(dict(ids=rec["out"].sequences[0].tolist(), hidden=m.last_hidden(), cache_len=kl, n_embeds=ne,
                         stats=m.prefill_draft_stats(reset=True) + m.draft_stats(reset=True)))
    run_scenario(Drafted(m, drafts), sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda",
                 steps=steps)
    return taps


def check_fp32(tag, taps, g, sc, drafts, rows, max_positions=MAX_POSITIONS):
    assert len(taps) == int(g["n_turns"])
    for t, tap in enumerate(taps):
        gold = g[f"t{t}_ids"].tolist()
        assert tap["ids"] == gold, (tag, rows, t, tap["ids"], gold)
        assert np.abs(tap["hidden"] - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, (tag, rows, t, "hidden")
        assert tap["cache_len"] == int(g[f"t{t}_cache_len"]), (tag, rows, t)
        d = drafts(t)
        ids, stats = PR.simulate(gold, [] if d is None else d, sc["max_new"], eos_ids(sc), max_positions - tap["n_embeds"], rows, sc["cfg"].vocab)
        assert ids == gold and tap["stats"] == stats, (tag, rows, t, tap["stats"], stats)


# ------------------------------------------------------------------------------------------------------------ ride == spliced prompt
def _prompt(n, seed, vocab):
    return np.random.default_rng(seed).integers(5, vocab, size=n).astype(np.int64)


def _append(m, ids):
    a = np.ascontiguousarray(ids, dtype=np.int64)
    _lib.check(m._lib.svln_append_turn(m._h, 0, a.ctypes.data_as(PI64), int(a.size), 0))


def _fixed(m, n):
    out = np.zeros(n, np.int64)
    _lib.check(m._lib.svln_generate_fixed(m._h, 0, n, out.ctypes.data_as(PI64)))
    return out.tolist()


def _set_draft(m, d):
    a = np.ascontiguousarray(d, dtype=np.int64)
    _lib.check(m._lib.svln_set_draft(m._h, 0, a.ctypes.data_as(PI64), int(a.size)))


def _begin(m, P, Tn, seed):
    """a fresh env with P rows of history in the cache (one earlier turn) and Tn new prompt rows"""
    m.reset(1)
    V = m.cfg.vocab
    if P:
        _append(m, _prompt(P, seed, V))
        _fixed(m, 1)
    _append(m, _prompt(Tn, seed + 1, V))
    assert m.env_state(0) == (P + Tn, P)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


#: (history rows P, prompt rows Tn, fed draft rows k): draft rows across the first page boundary (positions 62 .. 66); Tn + k across 256,
#: the fused-norm limit of the product plans, and across the page boundary at 256; 3 head rows (padded to 4); 2 head rows (the batched
#: GEMV head); the most rows a ride feeds, across a page boundary behind a history
SPLICE_CASES = [(20, 42, 5), (0, 253, 5), (0, 62, 2), (0, 63, 1), (70, 55, 7)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ride_equals_spliced_prompt_bit_for_bit(dtype):
    m = model("tiny_episode", dtype)
    cfg = m.cfg
    last = cfg.layers - 1
    norm_w = torch.from_numpy(m.get_tensor("model.norm.weight")).to(dtype).cuda()
    lm_head = torch.from_numpy(m.get_tensor("lm_head.weight")).to(dtype).cuda()
    try:
        for P, Tn, k in SPLICE_CASES:
            n, M, seed = k + 1, Tn + k, 100 * P + Tn
            modes(m, False, 0)
            _begin(m, P, Tn, seed)
            true = _fixed(m, 8)                                  # the plain loop's ids: the draft
            d = true[:k]
            # run B: the caller splices the embeddings of d on; a plain prefill of the same M rows
            m.set_layer_taps(True, last)
            _begin(m, P, Tn, seed)
            _append(m, d)
            tok_b = _fixed(m, 1)
            qkv_b, x_b = m.layer_probe(7), m.layer_probe(1)
            assert qkv_b.shape[0] == x_b.shape[0] == M
            rows_b = torch.from_numpy(x_b[M - n:]).to(dtype).cuda().contiguous()
            B = 2 if n <= 2 else 4 if n <= 4 else 8             # the batched-row op takes 2, 4, 8 rows: pad with copies of the last row
            xn = torch.zeros((B, cfg.hidden), dtype=dtype, device="cuda")
            rows_p = torch.cat([rows_b, rows_b[-1:].expand(B - n, -1)]).contiguous()
            torch.cuda.synchronize()
            _lib.check(m._lib.svln_op_rmsnorm(m._h, _ptr(rows_p), _ptr(norm_w), _ptr(xn), B, cfg.hidden, C.c_float(cfg.rms_eps)))
            toks = (C.c_int32 * 8)()
            _lib.check(m._lib.svln_op_gemv_batched(m._h, _ptr(lm_head), cfg.hidden, _ptr(xn), cfg.hidden, None, C.c_float(cfg.rms_eps), None, None, 0,
                                                   None, 0, cfg.vocab, cfg.hidden, _lib.EPI_ARGMAX, B, toks))
            arg_b = [int(toks[i]) for i in range(n)]
            hid_b = xn[:n].float().cpu().numpy()
            # run A: the ride
            modes(m, True, 0)
            _begin(m, P, Tn, seed)
            _set_draft(m, d)
            ids_a = _fixed(m, n)
            rides, rtok, fed = m.prefill_draft_stats(reset=True)
            qkv_a, x_a, hid_a = m.layer_probe(7), m.layer_probe(1), m.last_hidden()
            m.set_layer_taps(False)
            assert (rides, fed) == (1, k), (P, Tn, k, rides, fed)
            assert qkv_a.shape == qkv_b.shape and np.array_equal(qkv_a, qkv_b), (P, Tn, k, "q|k|v after RoPE", float(np.abs(qkv_a - qkv_b).max()))
            assert x_a.shape == x_b.shape and np.array_equal(x_a, x_b), (P, Tn, k, "x leaving the last layer", float(np.abs(x_a - x_b).max()))
            # what the ride emits is the verify rule on run B's arg-maxes, and the final-norm rows are run B's
            _, _, want, _ = VR.verify_step([None] + d, arg_b, 0, n, set())
            assert rtok == len(want) and ids_a[:rtok] == want, (P, Tn, k, ids_a, rtok, arg_b, d)
            assert np.array_equal(hid_a[:rtok], hid_b[:rtok]), (P, Tn, k, "final-norm rows")
            print(f"ride vs splice [{dtype}] P={P} Tn={Tn} k={k}: {rtok}/{n} head rows emitted, plain ids {true[:n]}, row arg-maxes {arg_b}")
            if dtype == torch.float32:
                assert arg_b == true[:n] and ids_a == true[:n] and rtok == n, (P, Tn, k, arg_b, true)
                assert tok_b == true[k:k + 1]                   # (the plain head on run B's last row)
            assert m.env_state(0) == (P + Tn, P + Tn + n - 1)
    finally:
        m.set_layer_taps(False)
        modes(m, False, 0)


# ------------------------------------------------------------------------------------------------------------ fixture episodes
def _other(tok, sc, avoid=()):
    eos = set(eos_ids(sc))
    return next(t for t in range(5, sc["cfg"].vocab) if t != tok and t not in eos and t not in avoid)


def variant(kind, gold, sc):
    """a draft for a turn whose plain ids are `gold`"""
    eos = eos_ids(sc)
    d = list(gold)
    if kind == "right":
        return d
    if kind == "wrong_at_0":
        d[0] = _other(gold[0], sc)
    elif kind == "wrong_at_1":
        if len(d) > 1:
            d[1] = _other(gold[1], sc)
    elif kind == "wrong_at_last":
        d[-1] = _other(gold[-1], sc)
    elif kind == "short":
        d = d[:max(len(d) // 2, 1)]
    elif kind == "long":
        d = d + [_other(gold[-1], sc)] * 6
    elif kind == "eos_early":
        j = min(1, len(d) - 1)
        d[j] = next((t for t in eos if t != gold[j]), _other(gold[j], sc))
    elif kind == "eos_missing":
        if d[-1] in eos:
            d[-1] = _other(gold[-1], sc)
        d = d + [_other(gold[-1], sc)] * 2
    elif kind == "oov_mid":
        d[len(d) // 2] = sc["cfg"].vocab + 5
    else:
        raise KeyError(kind)
    return d


VARIANTS = ["right", "wrong_at_0", "wrong_at_1", "wrong_at_last", "short", "long", "eos_early", "eos_missing", "oov_mid"]


@pytest.mark.parametrize("kind", VARIANTS)
@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode"])
def test_fp32_fixture_drafts(name, kind):
    """every turn of the episode (true1_episode: through its window restart) armed with a variant of the fixture's own ids, once without
    and once with verify passes behind the ride: ids, hidden rows and cache lengths are the fixture's on every turn -- the turns after a
    partly rejected ride included, so kv_len is right and rejected K / V rows do not leak -- and all six counters are simulate's"""
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]

    def drafts(t):
        return variant(kind, gold[t], sc)
    for rows in (0, 4):
        m = model(name, torch.float32)
        modes(m, True, rows)
        taps = run(m, sc, drafts)
        check_fp32(f"{name}/{kind}", taps, g, sc, drafts, rows)
        assert sum(t["stats"][0] for t in taps) >= 1
        if kind == "right":
            # the whole turn comes from the ride: no verify pass, no single step (a one-token turn has nothing to ride)
            for i, t in enumerate(taps):
                n = len(gold[i])
                assert t["stats"] == ((1, n, n - 1, 0, 0, 0) if n >= 2 else (0, 0, 0, 0, 0, 0)), (i, t["stats"])
    modes(m, False, 0)


@pytest.mark.parametrize("rows", [0, 4])
def test_long_draft_under_generate_fixed(rows):
    """a right draft of 12 ids under svln_generate_fixed(12): the ride feeds 7 rows and emits 8 tokens, verify passes (or single steps)
    finish; a second turn on the same env gives what it gives after a plain first turn"""
    m = model("tiny_episode", torch.float32)
    V = m.cfg.vocab
    try:
        _begin(m, 0, 50, 7)
        true = _fixed(m, 12)
        _append(m, true + _prompt(9, 8, V).tolist())           # (the next turn's prompt repeats the answer: its last id is not in the cache)
        true2 = _fixed(m, 5)
        state = m.env_state(0)
        for draft in (true, true[:3] + [(true[3] + 1) % V] + true[4:]):
            modes(m, True, rows)
            _begin(m, 0, 50, 7)
            _set_draft(m, draft)
            assert _fixed(m, 12) == true
            want = PR.simulate(true, draft, 12, (), MAX_POSITIONS - 50, rows, V)
            assert want[0] == true and m.prefill_draft_stats(reset=True) + m.draft_stats(reset=True) == want[1], (draft, want)
            if draft == true:
                assert want[1] == ((1, 8, 7, 1, 4, 0) if rows else (1, 8, 7, 0, 0, 4))
            _append(m, true + _prompt(9, 8, V).tolist())
            assert _fixed(m, 5) == true2 and m.env_state(0) == state
    finally:
        modes(m, False, 0)


def test_draft_independence():
    """same prompt, every draft variant (and no draft, an empty one, a single id): identical ids, hidden rows within the bound of each other"""
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    gold0 = g["t0_ids"].tolist()
    m = model(name, torch.float32)
    modes(m, True, 0)
    base = None
    for d0 in [None, [], gold0[:1]] + [variant(k, gold0, sc) for k in VARIANTS]:
        m.reset(1)
        tap = run(m, sc, lambda t: d0, steps=1)[0]
        if base is None:
            base = tap
            assert tap["ids"] == gold0 and tap["stats"][:3] == (0, 0, 0)
        assert tap["ids"] == base["ids"] and tap["cache_len"] == base["cache_len"], (d0, tap["ids"])
        assert np.abs(tap["hidden"] - base["hidden"]).max() <= HIDDEN_TOL
    modes(m, False, 0)


# ------------------------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode"])
def test_bf16_fixture_drafts(name):
    """the bf16 engine, every turn armed with the fp32 fixture's ids: the bounds and the margin rule of test_bf16_mode_vs_golden; two runs
    are bit-identical to each other"""
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    runs = []
    for _ in range(2):
        m = model(name, torch.bfloat16)
        modes(m, True, 0)
        runs.append(run(m, sc, lambda t: gold[t]))
    modes(m, False, 0)
    a, b = runs
    assert len(a) == len(b) == int(g["n_turns"])
    for t, (x, y) in enumerate(zip(a, b)):
        assert x["ids"] == y["ids"] and x["cache_len"] == y["cache_len"] and np.array_equal(x["hidden"], y["hidden"]), (name, t)
    agree = total = rows = rides = 0
    worst = 0.0
    diverged = False
    for t, tap in enumerate(a):
        ids, margins = tap["ids"], g[f"t{t}_margins"]
        rides += tap["stats"][0]
        n = 0
        while n < min(len(ids), len(gold[t])) and ids[n] == gold[t][n]:
            n += 1
        k = min(n + 1, len(gold[t]), len(ids))
        if not diverged:
            for j in range(k):
                h, gh = tap["hidden"][j], g[f"t{t}_hidden"][j]
                rel = float(np.linalg.norm(h - gh) / np.linalg.norm(gh))
                print(f"bf16 ride [{name}] turn {t} row {j}: rel L2 {rel:.3e}")
                worst = max(worst, rel); rows += 1
                assert rel < BF16_HIDDEN_REL[name], (name, t, j, rel)
                if j < len(margins) and margins[j] > BF16_MARGIN:
                    assert ids[j] == gold[t][j], (name, t, j, ids, gold[t], margins)
            total += len(gold[t]); agree += n
            if n < len(gold[t]):
                diverged = True
    assert rows >= 1 and rides >= 1
    line = (f"bf16 rides vs fp32 fixture [{name}]: {rows} hidden rows compared, worst rel L2 error {worst:.2e}, "
            f"{agree}/{total} ids agree before the first divergence, {rides} rides")
    print(line)
    _note("bf16_ride_vs_fixture", line)


# ------------------------------------------------------------------------------------------------------------ nothing changes
def _same(a, b, tag):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x["ids"] == y["ids"] and x["cache_len"] == y["cache_len"], (tag, t, x["ids"], y["ids"])
        assert np.array_equal(x["hidden"], y["hidden"]), (tag, t, "hidden rows differ")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_no_draft_penalty_and_mode_off_are_the_plain_turn(dtype):
    """mode on without a draft, mode on under a repetition penalty with drafts, mode off with drafts armed: ids AND hidden rows
    bit-identical to the plain engine's, every ride counter zero, and the armed draft is consumed by the call"""
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    m = model(name, dtype)
    plain = run(m, sc, lambda t: None, steps=16)
    m.reset(1); modes(m, True, 0)
    on_no_draft = run(m, sc, lambda t: None, steps=16)
    m.reset(1); modes(m, False, 0)
    off_armed = run(m, sc, lambda t: gold[t], steps=16)
    _same(plain, on_no_draft, "mode on, no draft")
    _same(plain, off_armed, "mode off, draft armed")
    for tap in on_no_draft + off_armed:
        assert tap["stats"] == (0, 0, 0, 0, 0, len(tap["ids"]) - 1), tap["stats"]
    # the armed draft is consumed by the call that ignored it: the next call, with the mode on, has none
    m.reset(1); modes(m, False, 0)
    _begin(m, 0, 40, 3)
    true = _fixed(m, 4)
    _begin(m, 0, 40, 3)
    _set_draft(m, true)
    assert _fixed(m, 4) == true
    modes(m, True, 0)
    _append(m, true + _prompt(9, 4, m.cfg.vocab).tolist())
    _fixed(m, 4)
    assert m.prefill_draft_stats() == (0, 0, 0)
    modes(m, False, 0)
    # repetition penalty: drafts are ignored (and consumed)
    name = "tiny_penalty"
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    m = model(name, dtype)
    plain = run(m, sc, lambda t: None)
    m.reset(1); modes(m, True, 4)
    armed = run(m, sc, lambda t: gold[t])
    modes(m, False, 0)
    _same(plain, armed, "penalty")
    for tap in armed:
        assert tap["stats"] == (0, 0, 0, 0, 0, len(tap["ids"]) - 1), tap["stats"]
    if dtype == torch.float32:
        assert [t["ids"] for t in plain] == gold


# ------------------------------------------------------------------------------------------------------------ top-2
def test_get_top2_is_refused_after_a_ride_emitted_the_last_token():
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    m = model(name, torch.float32)
    modes(m, True, 0)
    gold0 = g["t0_ids"].tolist()
    out = np.zeros(2, np.float32)
    tap = run(m, sc, lambda t: gold0, steps=1)[0]
    assert tap["stats"][1] == len(gold0)
    assert m._lib.svln_get_top2(m._h, out.ctypes.data_as(C.POINTER(C.c_float))) != 0
    assert "svln_set_prefill_draft" in m._lib.svln_last_error().decode()
    m.reset(1)
    tap = run(m, sc, lambda t: variant("wrong_at_1", gold0, sc), steps=1)[0]      # the turn ends on single steps: their top-2 logits are current
    assert tap["stats"][5] >= 1
    _lib.check(m._lib.svln_get_top2(m._h, out.ctypes.data_as(C.POINTER(C.c_float))))
    modes(m, False, 0)


# ------------------------------------------------------------------------------------------------------------ capacity
def _written_pages(m, cfg, n_positions):
    import attn_ref as R
    K = np.zeros((n_positions, cfg.kv_heads, 128), np.float32)
    Vv = np.zeros_like(K)
    _lib.check(m._lib.svln_op_kv_read(m._h, -1, 0, n_positions, K.ctypes.data_as(C.POINTER(C.c_float)), Vv.ctypes.data_as(C.POINTER(C.c_float))))
    return (K != np.float32(R.SENTINEL)).any((1, 2)) | (Vv != np.float32(R.SENTINEL)).any((1, 2))


def test_capacity_no_row_reaches_max_positions():
    """TINY with max_positions = 256 and a first turn of L = 253 rows: a ride may feed three rows only (positions 253 .. 255) however
    long the draft.  max_new = 4 fits: same ids, hidden rows and cache_len as the plain run, with layer 0's pools set to the sentinel
    before the run nothing is written outside the env's four pages.  max_new = 6 does not: the plain run raises 'sequence exceeds
    max_positions', and so does the turn with a ride; the env is usable after reset_for_env."""
    import attn_ref as R
    sc4 = dict(SCENARIOS["tiny_episode"], lens=(58, 48, 16), max_new=4, eos_mod=0)
    sc6 = dict(sc4, max_new=6)
    cfg = sc4["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=2, max_frames=1 + sc4["num_history"], max_positions=256)
    try:
        m.load_synthetic(SEED)
        m.model.num_history = sc4["num_history"]
        m.reset(1)
        base = run(m, sc4, lambda t: None, steps=1)[0]
        assert base["n_embeds"] == 253 and len(base["ids"]) == 4 and base["cache_len"] == 256
        filler = next(t for t in range(9, cfg.vocab) if t not in base["ids"])
        right = base["ids"] + [filler] * 10
        wrong = base["ids"][:2] + [filler] * 10
        for draft in (right, wrong):
            m.reset(1)
            modes(m, True, 0)
            _lib.check(m._lib.svln_op_fill_attn_state(m._h, R.SENTINEL, 0))
            tap = run(m, sc4, lambda t: draft, steps=1)[0]
            want = PR.simulate(base["ids"], draft, 4, (), 256 - 253, 0, cfg.vocab)
            assert want[1][2] == 3 and tap["stats"] == want[1], (tap["stats"], want)
            assert tap["ids"] == base["ids"] and tap["cache_len"] == base["cache_len"], tap["ids"]
            assert np.abs(tap["hidden"] - base["hidden"]).max() <= HIDDEN_TOL
            written = _written_pages(m, cfg, 2 * 256)
            pages = np.nonzero(written.reshape(-1, 64).any(1))[0]
            assert len(pages) == 4 and written.sum() == 256, (pages, written.sum())      # the env's four pages, none of the other env's block
        # the turn that does not fit: the plain error, with and without a ride
        for ride, draft in ((False, None), (True, right), (True, wrong)):
            m.reset(1)
            modes(m, ride, 0)
            _lib.check(m._lib.svln_op_fill_attn_state(m._h, R.SENTINEL, 0))
            with pytest.raises(_lib.SvlnError, match="sequence exceeds max_positions"):
                run(m, sc6, lambda t: draft, steps=1)
            written = _written_pages(m, cfg, 2 * 256)
            assert len(np.nonzero(written.reshape(-1, 64).any(1))[0]) == 4 and written.sum() == 256
            m.reset_for_env(0)
            m.reset(1)
            modes(m, ride, 0)
            tap = run(m, sc4, lambda t: draft, steps=1)[0]
            assert tap["ids"] == base["ids"] and tap["cache_len"] == base["cache_len"]
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    sc = SCENARIOS["tiny_episode"]
    m7 = model("true1_episode", torch.float32)                 # G = 7: no rows * G <= 32 limit for rides
    m7.set_prefill_draft(True)
    m7.set_prefill_draft(False)
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.bfloat16, max_envs=2, max_frames=3, max_positions=MAX_POSITIONS)
    try:
        m.load_synthetic(SEED)
        m.reset(1)
        m.set_prefill_draft(True)
        m.set_prefill_draft(True)                              # a call that changes nothing
        m.set_speculative(4)                                   # the two draft modes are independent
        m.set_speculative(0)
        m.set_prefill_draft(False)
        switches = {"svln_set_fp8_decode": m.set_fp8_decode, "svln_set_mxfp4_decode": m.set_mxfp4_decode, "svln_set_fp8_gemm": m.set_fp8_gemm,
                    "svln_set_mxfp4_batched": m.set_mxfp4_batched, "svln_set_decode_persistent": m.set_decode_persistent}
        for sym, fn in switches.items():
            m.set_prefill_draft(True)
            with pytest.raises(_lib.SvlnError, match=sym + ".*svln_set_prefill_draft"):
                fn(True)
            fn(False)                                          # switching one off is always fine
            m.set_prefill_draft(False)
            fn(True)
            with pytest.raises(_lib.SvlnError, match=sym):
                m.set_prefill_draft(True)
            m.set_prefill_draft(False)                         # nothing changes
            fn(False)
        # a change while a scheduler turn is in flight, either way
        ids = np.arange(10, 30, dtype=np.int64)
        slot = C.c_int32(-1)
        _lib.check(m._lib.svln_append_turn(m._h, 0, ids.ctypes.data_as(PI64), len(ids), 0))
        _lib.check(m._lib.svln_batch_submit(m._h, 0, 4, None, 0, C.byref(slot)))
        with pytest.raises(_lib.SvlnError, match="in flight"):
            m.set_prefill_draft(True)
        m.set_prefill_draft(False)
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        m.set_prefill_draft(True)
        _lib.check(m._lib.svln_batch_submit(m._h, 0, 4, None, 0, C.byref(slot)))
        with pytest.raises(_lib.SvlnError, match="in flight"):
            m.set_prefill_draft(False)
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        m.set_prefill_draft(False)
    finally:
        m.close()
