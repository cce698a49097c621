"""Draft-verified greedy decode (svln_set_speculative) on the GPU: the verify step against its Python restatement, and whole episodes
with drafts armed against the golden fixtures -- the mode is lossless, so ids, hidden rows and cache lengths must be what the plain loop
gives whatever the draft says, and the counters must be those of verify_ref.simulate."""
import ctypes as C

import numpy as np
import pytest
import torch

import verify_ref as VR
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM
from test_e2e_gpu import BF16_HIDDEN_REL, BF16_MARGIN, HIDDEN_TOL, _note
from util import load_golden

pytestmark = pytest.mark.gpu
MAX_POSITIONS = 2048
_models = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def model(name, dtype):
    """one engine per (scenario knobs, dtype) for the module; every run starts from reset(1) with the mode off and the counters at zero"""
    sc = SCENARIOS[name]
    key = (sc["cfg"].name, dtype, sc["num_history"], sc.get("tml"), sc.get("rep_penalty"))
    if key not in _models:
        m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=1, max_frames=1 + (sc["num_history"] or 0), max_positions=MAX_POSITIONS)
        m.load_synthetic(SEED)
        m.model.num_history = sc["num_history"]
        apply_knobs(m, sc)
        _models[key] = m
    m = _models[key]
    m.set_speculative(0)
    m.reset(1)
    m.draft_stats(reset=True)
    return m


class Drafted:
    """the model with draft_ids added to generate: turn t of the episode is armed with drafts[t] (None = no draft)"""

    def __init__(self, m, drafts):
        self._m, self._drafts, self.turn = m, drafts, 0

    def __getattr__(self, k):
        return getattr(self._m, k)

    def generate(self, *a, **kw):
        d = self._drafts(self.turn) if callable(self._drafts) else self._drafts[self.turn]
        self.turn += 1
        if d is not None:
            kw["draft_ids"] = d
        return self._m.generate(*a, **kw)


def run(m, sc, drafts, steps=None):
    """the scenario with per-turn drafts -> per turn: ids, hidden rows, cache_len, n_embeds, counters of the turn"""
    taps = []
    dm = Drafted(m, drafts)

    def on_turn(t, rec):
        ne, kl = m.env_state(0)
        taps.append(dict(ids=rec["out"].sequences[0].tolist(), hidden=m.last_hidden(), cache_len=kl, n_embeds=ne,
                         stats=m.draft_stats(reset=True)))
    run_scenario(dm, sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda", steps=steps)
    return taps


def expect(sc, gold_ids, draft, rows, n_embeds, max_positions=MAX_POSITIONS):
    """simulate for one turn: the fixture's ids are what plain greedy decoding emits; the turn's rows end at n_embeds"""
    return VR.simulate(gold_ids, [] if draft is None else draft, rows, sc["max_new"], eos_ids(sc), max_positions - n_embeds, sc["cfg"].vocab)


def check_fp32(name, taps, g, sc, drafts, rows):
    assert len(taps) == int(g["n_turns"])
    for t, tap in enumerate(taps):
        gold = g[f"t{t}_ids"].tolist()
        assert tap["ids"] == gold, (name, rows, t, tap["ids"], gold)
        assert np.abs(tap["hidden"] - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, (name, rows, t, "hidden")
        assert tap["cache_len"] == int(g[f"t{t}_cache_len"]), (name, rows, t)
        d = drafts(t) if callable(drafts) else drafts[t]
        ids, passes, vtok, single = expect(sc, gold, d, rows, tap["n_embeds"])
        assert ids == gold and tap["stats"] == (passes, vtok, single), (name, rows, t, tap["stats"], (passes, vtok, single))


# ------------------------------------------------------------------------------------------------------------ the verify step
def test_verify_step_equals_the_rule_on_the_small_table():
    """svln_op_verify_step against verify_ref.verify_step (the step simulate is made of): rows x first mismatch index x EOS index x
    max_new cut, from count = 3; the rows behind a mismatch carry arg-maxes that would be wrong to emit"""
    m = model("tiny_episode", torch.float32)
    count, n = 3, 0
    for rows in (2, 4, 8):
        cand = [100 + i for i in range(rows)]
        for mism in list(range(1, rows)) + [None]:
            fed = [50] + cand[:-1]
            if mism is not None:
                fed[mism] = 499
            for e_idx in list(range(rows)) + [None]:
                eos = [7, cand[e_idx], 9] if e_idx is not None else [7, 9]
                for max_new in [count + k for k in range(1, rows + 1)] + [1000]:
                    exp = VR.verify_step(fed, cand, count, max_new, set(eos))
                    fa, ca = np.asarray(fed, np.int32), np.asarray(cand, np.int32)
                    ea, em = np.asarray(eos, np.int64), np.full(rows, -9, np.int64)
                    nc, dn, nt = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
                    _lib.check(m._lib.svln_op_verify_step(m._h, rows, fa.ctypes.data_as(C.POINTER(C.c_int32)), ca.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          count, max_new, ea.ctypes.data_as(C.POINTER(C.c_int64)), len(eos), C.byref(nc),
                                                          C.byref(dn), em.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nt)))
                    got = (nc.value, bool(dn.value), em[:nc.value - count].tolist(), nt.value)
                    assert got == exp and (em[nc.value - count:] == -3).all(), (rows, mism, e_idx, max_new, got, exp)
                    n += 1
    assert n == (2 * 3 * 3 + 4 * 5 * 5 + 8 * 9 * 9)
    # a non-finite arg-max (-1) stops like the plain step
    fa, ca = np.asarray([5, 6], np.int32), np.asarray([-1, 8], np.int32)
    ea, em = np.asarray([7], np.int64), np.zeros(2, np.int64)
    nc, dn, nt = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(m._lib.svln_op_verify_step(m._h, 2, fa.ctypes.data_as(C.POINTER(C.c_int32)), ca.ctypes.data_as(C.POINTER(C.c_int32)), 1, 100,
                                          ea.ctypes.data_as(C.POINTER(C.c_int64)), 1, C.byref(nc), C.byref(dn), em.ctypes.data_as(C.POINTER(C.c_int64)),
                                          C.byref(nt)))
    assert (nc.value, dn.value, em[0], nt.value) == (2, 1, -1, -1)


# ------------------------------------------------------------------------------------------------------------ fp32 episodes
@pytest.mark.parametrize("name,rows", [("tiny_episode", 2), ("tiny_episode", 4), ("tiny_episode", 8), ("true1_episode", 4),
                                       ("true1_episode", 2), ("true4_episode", 4)])
def test_fp32_fixture_drafts(name, rows):
    """every turn armed with the fixture's own ids: ids identical, hidden rows within 1e-3, cache_len identical, counters = simulate.
    tiny_episode turn 0 has 6 tokens: 3 / 2 / 1 verify passes at 2 / 4 / 8 rows and no single step."""
    sc, g = SCENARIOS[name], load_golden(name)
    m = model(name, torch.float32)
    m.set_speculative(rows)
    drafts = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    taps = run(m, sc, drafts)
    check_fp32(name, taps, g, sc, drafts, rows)
    if name == "tiny_episode":
        assert len(drafts[0]) == 6 and taps[0]["stats"] == ({2: 3, 4: 2, 8: 1}[rows], 5, 0)
    assert sum(t["stats"][0] for t in taps) >= 1 and all(t["stats"][2] == 0 for t in taps)         # right drafts: no single step at all
    m.set_speculative(0)


def _variants(gold0, sc):
    """drafts for turn 0 of tiny_episode that must not change what is emitted"""
    eos = eos_ids(sc)
    V = sc["cfg"].vocab
    out = {}
    for j in range(1, len(gold0)):
        d = list(gold0)
        d[j] = next(t for t in range(5, V) if t != gold0[j] and t not in eos)
        out[f"wrong_at_{j}"] = d
    out["empty"] = []
    out["length_1"] = gold0[:1]
    out["twice_too_long"] = gold0 + [next(t for t in range(9, V) if t not in eos)] * len(gold0)
    d = list(gold0)
    d[2] = next(t for t in eos if t != gold0[2])
    out["eos_at_2"] = d
    return out


@pytest.mark.parametrize("rows", [4, 8])
def test_draft_independence(rows):
    """whatever turn 0's draft says, the whole episode reproduces the fixture (K / V rows of rejected positions left behind by turn 0
    would show in the later turns, which run with the fixture's drafts) and the counters are simulate's"""
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    for vname, d0 in _variants(gold[0], sc).items():
        m = model(name, torch.float32)
        m.set_speculative(rows)
        drafts = [d0] + gold[1:]
        taps = run(m, sc, drafts)
        check_fp32(f"{name}/{vname}", taps, g, sc, drafts, rows)
    m.set_speculative(0)


def test_penalty_and_mode_off_ignore_drafts():
    for name, rows in (("tiny_penalty", 4), ("tiny_episode", 0)):
        sc, g = SCENARIOS[name], load_golden(name)
        m = model(name, torch.float32)
        m.set_speculative(rows)
        drafts = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
        taps = run(m, sc, drafts)
        for t, tap in enumerate(taps):
            gold = g[f"t{t}_ids"].tolist()
            assert tap["ids"] == gold and tap["cache_len"] == int(g[f"t{t}_cache_len"]), (name, t)
            assert np.abs(tap["hidden"] - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, (name, t)
            assert tap["stats"] == (0, 0, len(gold) - 1), (name, t, tap["stats"])
        m.set_speculative(0)


def test_get_top2_is_refused_after_a_verify_emitted_last_token():
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    m = model(name, torch.float32)
    m.set_speculative(4)
    gold0 = g["t0_ids"].tolist()
    out = np.zeros(2, np.float32)
    run(m, sc, [gold0], steps=1)
    assert m._lib.svln_get_top2(m._h, out.ctypes.data_as(C.POINTER(C.c_float))) != 0
    assert "verify" in m._lib.svln_last_error().decode()
    m.reset(1)
    bad = list(gold0)
    bad[1] = next(t for t in range(5, 99) if t != gold0[1] and t not in eos_ids(sc))
    run(m, sc, [bad], steps=1)                              # the turn ends on single steps: their top-2 logits are current
    _lib.check(m._lib.svln_get_top2(m._h, out.ctypes.data_as(C.POINTER(C.c_float))))
    m.set_speculative(0)


# ------------------------------------------------------------------------------------------------------------ capacity
def test_capacity_no_row_reaches_max_positions():
    """TINY with max_positions = 256: a first turn of 253 rows, max_new = 3, 8 rows per pass and a long right draft: the pass may carry
    two rows only (positions 253, 254).  Same ids, hidden rows and cache_len as the same engine with the mode off; with layer 0's pools
    set to the sentinel before the run, every slot from position 255 of the env's pages on, and every page no env holds, still holds it."""
    import attn_ref as R
    sc = dict(SCENARIOS["tiny_episode"], lens=(58, 48, 16), max_new=3, eos_mod=0)
    cfg = sc["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=2, max_frames=1 + sc["num_history"], max_positions=256)
    try:
        m.load_synthetic(SEED)
        m.model.num_history = sc["num_history"]
        m.reset(1)
        base = run(m, sc, [None], steps=1)[0]
        assert base["n_embeds"] == 253 and len(base["ids"]) == 3 and base["cache_len"] == 255
        filler = next(t for t in range(9, cfg.vocab) if t not in base["ids"])
        wrong = [base["ids"][0], filler] + [filler] * 10
        for draft, stats in ((base["ids"] + [filler] * 10, (1, 2, 0)), (wrong, (1, 1, 1))):
            m.reset(1)
            m.set_speculative(8)
            m.draft_stats(reset=True)
            _lib.check(m._lib.svln_op_fill_attn_state(m._h, R.SENTINEL, 0))
            tap = run(m, sc, [draft], steps=1)[0]
            m.set_speculative(0)
            assert tap["ids"] == base["ids"] and tap["cache_len"] == base["cache_len"] and tap["stats"] == stats, (tap["ids"], tap["stats"])
            assert np.abs(tap["hidden"] - base["hidden"]).max() <= HIDDEN_TOL
            n = 2 * 256
            K = np.zeros((n, cfg.kv_heads, 128), np.float32)
            Vv = np.zeros_like(K)
            _lib.check(m._lib.svln_op_kv_read(m._h, -1, 0, n, K.ctypes.data_as(C.POINTER(C.c_float)), Vv.ctypes.data_as(C.POINTER(C.c_float))))
            written = (K != np.float32(R.SENTINEL)).any((1, 2)) | (Vv != np.float32(R.SENTINEL)).any((1, 2))
            pages = np.nonzero(written.reshape(-1, 64).any(1))[0]
            assert len(pages) == 4, pages                              # the env's four pages, none of the other env's block
            order = np.argsort([int(np.nonzero(written[p * 64:(p + 1) * 64])[0].size) for p in pages])     # the partly written page is the last logical one
            last = pages[order[0]]
            assert written.sum() == 255 and written[last * 64:last * 64 + 63].all() and not written[last * 64 + 63], \
                "a K / V row was written at or beyond position 255"
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    m7 = model("true1_episode", torch.float32)                 # G = 7
    with pytest.raises(_lib.SvlnError, match="32"):
        m7.set_speculative(8)
    m7.set_speculative(4)
    m7.set_speculative(0)
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.bfloat16, max_envs=2, max_frames=3, max_positions=MAX_POSITIONS)
    try:
        m.load_synthetic(SEED)
        m.reset(1)
        for bad in (3, 1, 16, -2):
            with pytest.raises(_lib.SvlnError, match="rows"):
                m.set_speculative(bad)
        m.set_speculative(8)                                   # G = 2
        m.set_speculative(8)                                   # a call that changes nothing
        switches = {"svln_set_fp8_decode": m.set_fp8_decode, "svln_set_mxfp4_decode": m.set_mxfp4_decode, "svln_set_fp8_gemm": m.set_fp8_gemm,
                    "svln_set_mxfp4_batched": m.set_mxfp4_batched, "svln_set_decode_persistent": m.set_decode_persistent}
        for sym, fn in switches.items():
            m.set_speculative(4)
            with pytest.raises(_lib.SvlnError, match="svln_set_speculative"):
                fn(True)
            fn(False)                                          # switching one off is always fine
            m.set_speculative(0)
            fn(True)
            with pytest.raises(_lib.SvlnError, match="svln_set_speculative"):
                m.set_speculative(4)
            m.set_speculative(0)                               # nothing changes
            fn(False)
        # a change while a scheduler turn is in flight, either way
        ids = np.arange(10, 30, dtype=np.int64)
        slot = C.c_int32(-1)
        _lib.check(m._lib.svln_append_turn(m._h, 0, ids.ctypes.data_as(C.POINTER(C.c_int64)), len(ids), 0))
        _lib.check(m._lib.svln_batch_submit(m._h, 0, 4, None, 0, C.byref(slot)))
        with pytest.raises(_lib.SvlnError, match="in flight"):
            m.set_speculative(4)
        m.set_speculative(0)
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        m.set_speculative(4)
        _lib.check(m._lib.svln_batch_submit(m._h, 0, 4, None, 0, C.byref(slot)))
        with pytest.raises(_lib.SvlnError, match="in flight"):
            m.set_speculative(0)
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        m.set_speculative(0)
        # svln_set_draft: unknown env, negative or oversized length
        one = np.asarray([1], np.int64)
        p = one.ctypes.data_as(C.POINTER(C.c_int64))
        assert m._lib.svln_set_draft(m._h, 2, p, 1) != 0 and m._lib.svln_set_draft(m._h, -1, p, 1) != 0
        assert m._lib.svln_set_draft(m._h, 0, p, -1) != 0 and m._lib.svln_set_draft(m._h, 0, p, MAX_POSITIONS + 1) != 0
        _lib.check(m._lib.svln_set_draft(m._h, 0, p, 1))
        _lib.check(m._lib.svln_set_draft(m._h, 0, None, 0))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode", "true4_episode"])
def test_bf16_fixture_drafts(name):
    """the bf16 engine, 4 rows per pass, every turn armed with the fp32 fixture's ids: the bounds and the rule of test_bf16_mode_vs_golden
    (they cover bf16 storage error, not a summation order); two runs are bit-identical to each other"""
    sc, g = SCENARIOS[name], load_golden(name)
    drafts = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    runs = []
    for _ in range(2):
        m = model(name, torch.bfloat16)
        m.set_speculative(4)
        runs.append(run(m, sc, drafts))
        m.set_speculative(0)
    a, b = runs
    assert len(a) == len(b) == int(g["n_turns"])
    for t, (x, y) in enumerate(zip(a, b)):
        assert x["ids"] == y["ids"] and x["cache_len"] == y["cache_len"] and np.array_equal(x["hidden"], y["hidden"]), (name, t)
    agree = total = rows = passes = 0
    worst = 0.0
    diverged = False
    for t, tap in enumerate(a):
        ids, gold, margins = tap["ids"], g[f"t{t}_ids"].tolist(), g[f"t{t}_margins"]
        passes += tap["stats"][0]
        n = 0
        while n < min(len(ids), len(gold)) and ids[n] == gold[n]:
            n += 1
        k = min(n + 1, len(gold), len(ids))
        if not diverged:
            for j in range(k):
                h, gh = tap["hidden"][j], g[f"t{t}_hidden"][j]
                rel = float(np.linalg.norm(h - gh) / np.linalg.norm(gh))
                print(f"bf16 verify [{name}] turn {t} row {j}: rel L2 {rel:.3e}")
                worst = max(worst, rel); rows += 1
                assert rel < BF16_HIDDEN_REL[name], (name, t, j, rel)
                if j < len(margins) and margins[j] > BF16_MARGIN:
                    assert ids[j] == gold[j], (name, t, j, ids, gold, margins)
            total += len(gold); agree += n
            if n < len(gold):
                diverged = True
    assert rows >= 1 and passes >= 1
    line = (f"bf16 draft-verified (4 rows) vs fp32 fixture [{name}]: {rows} hidden rows compared, worst rel L2 error {worst:.2e}, "
            f"{agree}/{total} ids agree before the first divergence, {passes} verify passes")
    print(line)
    _note("bf16_verify_vs_fixture", line)
