"""Drafts in the scheduler's prefill pass (svln_set_batch_draft) on the GPU.  (1) an iteration with rides is, bit for bit, the mode-off
iteration whose callers spliced the same ids onto their prompts; (2) lockstep and (3) staggered envs reproduce the mode-off run whatever
the drafts say, with the counters of batch_draft_ref.simulate; (4) capacity; (5) the bf16 engine inside the bounds of the existing
lockstep test; (6) what the switch consumes, refuses and leaves alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_draft_ref as BR
from scenarios import SCENARIOS, SEED, eos_ids
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from test_e2e_gpu import HIDDEN_TOL
from test_prefill_draft_gpu import variant

pytestmark = pytest.mark.gpu
MAX_POSITIONS = 2048
PI64 = C.POINTER(C.c_int64)
PF32 = C.POINTER(C.c_float)
SC = SCENARIOS["tiny_episode"]
CFG = SC["cfg"]
_models = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def model(dtype):
    """one 8-env TINY engine per dtype for the module; every use starts from reset(8) with the switch off and the counters at zero"""
    if dtype not in _models:
        m = StreamVLNForCausalLM(CFG, dtype=dtype, max_envs=8, max_frames=24, max_positions=MAX_POSITIONS)
        m.load_synthetic(SEED)
        m.model.num_history = SC["num_history"]
        _models[dtype] = m
    m = _models[dtype]
    m.reset(8)
    switch(m, False)
    m.set_auto_draft(False)
    return m


def switch(m, on):
    m.set_batch_draft(on)
    m.batch_draft_stats(reset=True)


# ------------------------------------------------------------------------------------------------------------ the C ABI, env by slot
def _prompt(n, seed):
    return np.random.default_rng(seed).integers(5, CFG.vocab, size=n).astype(np.int64)


def _append(m, env, ids):
    a = np.ascontiguousarray(ids, dtype=np.int64)
    _lib.check(m._lib.svln_append_turn(m._h, env, a.ctypes.data_as(PI64), int(a.size), 0))


def _fixed(m, env, n):
    out = np.zeros(n, np.int64)
    _lib.check(m._lib.svln_generate_fixed(m._h, env, n, out.ctypes.data_as(PI64)))
    return out.tolist()


def _set_draft(m, env, d):
    a = np.ascontiguousarray(d, dtype=np.int64)
    _lib.check(m._lib.svln_set_draft(m._h, env, a.ctypes.data_as(PI64), int(a.size)))


def _state(m, env):
    ne, kl = C.c_int32(), C.c_int32()
    _lib.check(m._lib.svln_env_state(m._h, env, C.byref(ne), C.byref(kl)))
    return ne.value, kl.value


def _submit(m, env, max_new, eos=()):
    e = np.asarray(eos, dtype=np.int64)
    slot = C.c_int32(-1)
    _lib.check(m._lib.svln_batch_submit(m._h, env, max_new, e.ctypes.data_as(PI64) if len(e) else None, len(e), C.byref(slot)))
    return slot.value


def _step(m):
    running, nf = C.c_int32(), C.c_int32()
    fin = (C.c_int32 * 8)()
    _lib.check(m._lib.svln_batch_step(m._h, C.byref(running), fin, C.byref(nf)))
    return running.value, [fin[k] for k in range(nf.value)]


def _result(m, slot):
    out = np.zeros(64, np.int64)
    n, env = C.c_int32(), C.c_int32()
    _lib.check(m._lib.svln_batch_result(m._h, slot, C.byref(env), out.ctypes.data_as(PI64), 64, C.byref(n)))
    return env.value, out[: n.value].tolist()


def _kv(m, env, start, n):
    K = np.zeros((n, CFG.kv_heads, 128), np.float32)
    Vv = np.zeros_like(K)
    _lib.check(m._lib.svln_op_kv_read(m._h, env, start, n, K.ctypes.data_as(PF32), Vv.ctypes.data_as(PF32)))
    return K, Vv


def _begin(m, env, P, Tn, seed):
    """env with P rows of history in the cache (one earlier turn) and Tn new prompt rows"""
    _lib.check(m._lib.svln_reset_env(m._h, env))
    if P:
        _append(m, env, _prompt(P, seed))
        _fixed(m, env, 1)
    _append(m, env, _prompt(Tn, seed + 1))
    assert _state(m, env) == (P + Tn, P)


def _run(m, jobs, eos=(), max_iters=64):
    """submit (env, max_new) in order, iterate until all are done -> ({env: dict(ids, hidden, kv_len, slot)}, iterations run)"""
    slots = {_submit(m, env, max_new, eos): env for env, max_new in jobs}
    out, iters = {}, 0
    while slots:
        assert iters < max_iters
        _, fin = _step(m)
        iters += 1
        for s in fin:
            env, ids = _result(m, s)
            assert slots.pop(s) == env
            out[env] = dict(ids=ids, hidden=m.last_hidden_batch(s), kv_len=_state(m, env)[1], slot=s)
    return out, iters


# ------------------------------------------------------------------------------------------------------------ 1: ride == spliced prompts
#: (history rows P, prompt rows Tn, fed draft rows k) per env.  A: draft rows straddle (positions 62 .. 66) and end at (.. 63) a KV page
#: edge, the most rows a ride feeds behind a history; M = 173.  B: 8 envs, M = 308 rows, across the 256-row fused-norm limit of the
#: product plans; 48 head rows = two arg-max chunks, the second one partly filled
CASE_A = [(20, 42, 5), (0, 62, 2), (70, 55, 7)]
CASE_B = [(0, 30 + e, 5) for e in range(8)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [CASE_A, CASE_B], ids=["A", "B"])
def test_ride_iteration_equals_spliced_prompts_bit_for_bit(case, dtype):
    m = model(dtype)
    assert sum(Tn + k for _, Tn, k in case) == (173 if case is CASE_A else 308)

    def begin():
        for e, (P, Tn, k) in enumerate(case):
            _begin(m, e, P, Tn, 1000 * len(case) + 100 * e + Tn)
    # the plain run: its ids are the drafts
    begin()
    plain, _ = _run(m, [(e, k + 1) for e, (_, _, k) in enumerate(case)])
    true = {e: plain[e]["ids"] for e in plain}
    assert all(len(true[e]) == case[e][2] + 1 for e in true)
    # the callers splice the draft ids on as text: one mode-off iteration over the same segments
    begin()
    for e, (P, Tn, k) in enumerate(case):
        _append(m, e, true[e][:k])
    spliced, it_s = _run(m, [(e, 1) for e in range(len(case))])
    kv_s = {e: _kv(m, e, P, Tn + k) for e, (P, Tn, k) in enumerate(case)}
    # the ride
    switch(m, True)
    begin()
    for e, (P, Tn, k) in enumerate(case):
        _set_draft(m, e, true[e][:k])
    slots = {_submit(m, e, k + 1): e for e, (_, _, k) in enumerate(case)}
    _, fin = _step(m)
    kv_r = {e: _kv(m, e, P, Tn + k) for e, (P, Tn, k) in enumerate(case)}
    stats = m.batch_draft_stats()
    assert it_s == 1 and stats[0] == len(case) and stats[2:] == (sum(k for _, _, k in case), 1, 0), stats
    for e, (P, Tn, k) in enumerate(case):
        for a, b, what in zip(kv_r[e], kv_s[e], "KV"):
            assert np.array_equal(a, b), (e, what, "rows of positions P .. P + Tn + k - 1", float(np.abs(a - b).max()))
    assert sorted(fin) == sorted(slots), (fin, "every env's ride confirms its whole turn", stats)
    for s in fin:
        e, ids = _result(m, s)
        P, Tn, k = case[e]
        hid = m.last_hidden_batch(s)
        print(f"ride vs splice [{dtype}] env {e} P={P} Tn={Tn} k={k}: ride ids {ids}, plain ids {true[e]}, spliced token {spliced[e]['ids']}")
        assert len(ids) == k + 1 and hid.shape[0] == k + 1
        assert np.array_equal(hid[k], spliced[e]["hidden"][0]), (e, "final-norm row of the last head row")
        assert ids[k] == spliced[e]["ids"][0], (e, ids, spliced[e]["ids"])
        assert _state(m, e) == (P + Tn, P + Tn + k)
        if dtype == torch.float32:
            assert ids == true[e]
            assert np.abs(hid - plain[e]["hidden"]).max() <= HIDDEN_TOL, (e, float(np.abs(hid - plain[e]["hidden"]).max()))
    switch(m, False)


# ------------------------------------------------------------------------------------------------------------ agents with drafts
class Drafted:
    """the model with draft_ids added to generate_batch requests / submit: drafts(env_id, turn index, model) -> ids or None.  `turns`
    records every turn: dict(env, turn, draft, n_embeds, kv_len, at = the tick / call it was submitted in)."""

    def __init__(self, m, drafts):
        self._m, self._drafts, self.n, self.turns, self.at, self.calls = m, drafts, {}, [], 0, []

    def __getattr__(self, k):
        return getattr(self._m, k)

    def _draft(self, env_id):
        t = self.n.get(env_id, 0)
        self.n[env_id] = t + 1
        d = self._drafts(env_id, t, self._m)
        return t, (None if d is None else [int(x) for x in d])

    def generate_batch(self, reqs, **kw):
        reqs, recs = [dict(r) for r in reqs], []
        for r in reqs:
            t, d = self._draft(r["env_id"])
            armed = d
            if d is None and self._m._auto_draft and r["env_id"] in self._m._last_out:
                armed = self._m._last_out[r["env_id"]].tolist()
            if d is not None:
                r["draft_ids"] = d
            past = r["past_key_values"]
            recs.append(dict(env=r["env_id"], turn=t, draft=armed, kv_len=0 if past is None else past.get_seq_length(), at=0))
        outs = self._m.generate_batch(reqs, **kw)
        for rec in recs:
            rec["n_embeds"] = self._m.env_state(rec["env"])[0]
        self.calls.append((recs, self._m.batch_draft_stats(reset=True)))
        return outs

    def submit(self, **req):
        t, d = self._draft(req["env_id"])
        armed = d
        if d is None and self._m._auto_draft and req["env_id"] in self._m._last_out:
            armed = self._m._last_out[req["env_id"]].tolist()
        if d is not None:
            req["draft_ids"] = d
        ticket = self._m.submit(**req)
        ne, kl = self._m.env_state(req["env_id"])
        self.turns.append(dict(env=req["env_id"], turn=t, draft=armed, n_embeds=ne, kv_len=kl, at=self.at))
        return ticket


def _agents(mw, n_envs, seed0, lengths=None):
    proc = mw.get_vision_tower().image_processor
    agents = []
    for e in range(n_envs):
        enc = SyntheticPromptEncoder(CFG, seed=seed0(e), first_len=SC["lens"][0], memory_len=SC["lens"][1], later_len=SC["lens"][2])
        ag = StreamingAgent(mw, enc, num_frames=SC["num_frames"], num_future_steps=SC["nfs"], num_history=SC["num_history"], env_id=e,
                            device="cuda", max_new_tokens=SC["max_new"], eos_token_ids=eos_ids(SC), preprocess=proc.preprocess_array)
        if lengths is not None:
            ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
        agents.append(ag)
    return agents


def _sim(recs, true_of, switch_on=True):
    """batch_draft_ref.simulate on recorded turns; true_of(rec) = the ids the plain run emits for that turn"""
    turns = [BR.Turn(r["env"], list(true_of(r)) + [0] * 8, r["draft"], SC["max_new"], eos_ids(SC), r["n_embeds"], r["kv_len"], r["at"]) for r in recs]
    stats, log = BR.simulate(turns, MAX_POSITIONS, CFG.vocab, switch=switch_on)
    assert BR.broken_rules(turns, log, MAX_POSITIONS, drafts_usable=switch_on) == []
    return stats, log, turns


# ------------------------------------------------------------------------------------------------------------ 2: lockstep
MIXED = ["right", "wrong_at_1", "short", "long", "eos_early", "oov_mid", None, "right"]


def _lockstep(m, drafts, on, n_envs=8, steps=16, seed0=lambda e: 7 + 31 * e):
    m.reset(n_envs)
    switch(m, on)
    mw = Drafted(m, drafts)
    agents = _agents(mw, n_envs, seed0)
    group = BatchedAgents(agents)
    hidden = [[] for _ in range(n_envs)]
    for step in range(steps):
        n0 = len(agents[0].turn_log)
        group.act([synthetic_frame(e, step) for e in range(n_envs)])
        if len(agents[0].turn_log) > n0:
            for e in range(n_envs):
                hidden[e].append(m.last_hidden_batch(e))
    ids = [[t["out"].sequences[0].tolist() for t in a.turn_log] for a in agents]
    kv = [[t["out"].past_key_values.get_seq_length() for t in a.turn_log] for a in agents]
    assert any(t["memory"] for t in agents[0].turn_log)          # through a window restart
    return dict(ids=ids, hidden=hidden, kv=kv, calls=mw.calls)


def test_lockstep_eight_envs_equal_the_mode_off_run():
    """8 envs through generate_batch over a window restart.  The yardstick is the run with the switch off (held to the oracle by
    test_eight_env_lockstep_generate_batch_vs_oracle); every kind of draft must give its ids, hidden rows and cache lengths, and the five
    counters of every generate_batch call must be the restatement's."""
    m = model(torch.float32)
    base = _lockstep(m, lambda e, t, mm: None, False)
    gold = base["ids"]
    waits = 0
    for recs, stats in base["calls"]:
        want, log, turns = _sim(recs, lambda r: gold[r["env"]][r["turn"]], switch_on=False)
        assert stats == want and stats[:3] == (0, 0, 0), (stats, want)
        waits += any(t.first_iteration > 0 for t in turns)
    assert waits >= 1             # (the restart turns of 8 envs do not fit one pass: jobs wait, and keep their drafts)
    kinds = {"right": lambda e: "right", "wrong_at_0": lambda e: "wrong_at_0", "mixed": lambda e: MIXED[e]}
    for name, kind in kinds.items():
        def drafts(e, t, mm):
            return None if kind(e) is None else variant(kind(e), gold[e][t], SC)
        run = _lockstep(m, drafts, True)
        assert run["ids"] == gold, name
        assert run["kv"] == base["kv"], name
        for e in range(8):
            for t, (a, b) in enumerate(zip(run["hidden"][e], base["hidden"][e])):
                assert a.shape == b.shape and np.abs(a - b).max() <= HIDDEN_TOL, (name, e, t, float(np.abs(a - b).max()))
        rides = 0
        for c, (recs, stats) in enumerate(run["calls"]):
            want, log, turns = _sim(recs, lambda r: gold[r["env"]][r["turn"]])
            print(f"lockstep [{name}] call {c}: counters {stats}, restatement {want}")
            assert stats == want, (name, c, stats, want)
            rides += stats[0]
            if name == "right":
                # every turn takes exactly one iteration and no decode row is fed; the call is one iteration unless jobs had to wait
                assert stats[4] == 0 and all(t.first_iteration == t.last_iteration for t in turns), (c, stats)
                assert stats[3] == 1 + max(t.first_iteration for t in turns), (c, stats)
        assert rides >= 1, name
    switch(m, False)


# ------------------------------------------------------------------------------------------------------------ 3: staggered
def _ragged(m, drafts, on, auto, ticks):
    N = 8
    m.reset(N)
    switch(m, on)
    m.set_auto_draft(auto)
    mw = Drafted(m, drafts)
    lengths = lambda e, t: 2 if (e + t) % 2 == 0 else 4
    agents = _agents(mw, N, lambda e: 7 + 31 * e, lengths)
    hidden = [[] for _ in range(N)]
    group = AsyncBatchedAgents(agents, on_result=lambda i, ticket, out: hidden[i].append(m.last_hidden_batch(ticket.slot)))
    tick = 0
    while tick < ticks or group.waiting:                       # (after the last tick no env steps: the turns in flight run to their end)
        assert tick < ticks + 8
        mw.at = tick
        active = {i for i in range(N) if tick >= i} if tick < ticks else set()
        group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active=active)
        tick += 1
    stats = m.batch_draft_stats(reset=True)
    m.set_auto_draft(False)
    ids = [[t["out"].sequences[0].tolist() for t in a.turn_log] for a in agents]
    kv = [[t["out"].past_key_values.get_seq_length() for t in a.turn_log] for a in agents]
    return dict(ids=ids, hidden=hidden, kv=kv, turns=mw.turns, stats=stats, ticks=tick)


def test_ragged_scheduler_equals_the_mode_off_run():
    """8 envs with staggered starts through submit / step_batch, 24 ticks: rides share iterations with other envs' decode rows.  One run
    under set_auto_draft, one with explicit right drafts, one with long drafts wrong at index 0; ids, hidden rows and cache lengths are the
    mode-off run's, turn by turn, the counters the restatement's, and at least 4 iterations carried a ride beside decode rows."""
    m = model(torch.float32)
    # (a run with rides gets further in 24 ticks than the plain one: the mode-off run is given the ticks to reach those turns as well)
    base = _ragged(m, lambda e, t, mm: None, False, False, 64)
    gold = base["ids"]
    # (most turns of this episode are a single EOS token: with right drafts nothing is left to decode, so no ride can share its iteration
    #  with a decode row, and auto-drafts ride once per window.  A third run arms every turn with a long draft that is wrong at index 0:
    #  every turn rides five rows, beside the decode rows of the envs whose first turn is still running.)
    def wrong_long(e, t, mm):
        return variant("long", variant("wrong_at_0", gold[e][t], SC), SC) if t < len(gold[e]) else None
    runs = {"auto": _ragged(m, lambda e, t, mm: None, True, True, 24),
            "right": _ragged(m, lambda e, t, mm: gold[e][t] if t < len(gold[e]) else None, True, False, 24),
            "wrong_long": _ragged(m, wrong_long, True, False, 24)}
    mixed_total = 0
    for name, run in runs.items():
        for e in range(8):
            n = len(run["ids"][e])
            assert 2 <= n <= len(gold[e]) and run["ids"][e] == gold[e][:n], (name, e, run["ids"][e], gold[e][:n])
            assert run["kv"][e] == base["kv"][e][:n], (name, e)
            for t in range(n):
                a, b = run["hidden"][e][t], base["hidden"][e][t]
                assert a.shape == b.shape and np.abs(a - b).max() <= HIDDEN_TOL, (name, e, t)
        want, log, _ = _sim(run["turns"], lambda r: gold[r["env"]][r["turn"]])
        mixed = sum(1 for rec in log if rec["rides"] and rec["decode_rows"])
        print(f"ragged [{name}]: counters {run['stats']}, restatement {want}, {mixed} mixed iterations with a ride")
        assert run["stats"] == want, (name, run["stats"], want)
        assert run["stats"][0] >= 1, (name, run["stats"])
        mixed_total += mixed
    assert mixed_total >= 4, mixed_total
    switch(m, False)


# ------------------------------------------------------------------------------------------------------------ 4: capacity
def _written(m, n_positions):
    import attn_ref as R
    K, Vv = _kv(m, -1, 0, n_positions)
    return (K != np.float32(R.SENTINEL)).any((1, 2)) | (Vv != np.float32(R.SENTINEL)).any((1, 2))


def test_capacity_workspace_cut_and_last_positions():
    """max_positions = 256.  Two envs, max_new = 4, right drafts: env 0 (120 rows) rides 3 rows, so env 1's k is cut to 256 - 123 - Tn:
    2 at Tn = 131, 0 at 133; at Tn = 134 it waits for the next iteration and rides there.  A prompt that ends at max_positions - 2 rides
    two rows only.  Ids, hidden rows and kv_len are the mode-off run's, the counters the restatement's, and with layer 0's pools set to
    a sentinel before the run nothing is written outside the pages of the rows the iteration prepared."""
    import attn_ref as R
    MP = 256
    m = StreamVLNForCausalLM(CFG, dtype=torch.float32, max_envs=2, max_frames=3, max_positions=MP)
    try:
        m.load_synthetic(SEED)
        m.reset(2)
        # a turn the plain loop cannot finish inside max_positions: the plain error, with and without a ride
        for on in (False, True):
            switch(m, on)
            _begin(m, 0, 0, 253, 77)
            _set_draft(m, 0, [7] * 9)
            with pytest.raises(_lib.SvlnError, match="sequence exceeds max_positions"):
                _run(m, [(0, 6)])
        _lib.check(m._lib.svln_set_draft(m._h, 0, None, 0))
        layouts = [([120, 131], 4, (3, 2)), ([120, 133], 4, (3, 0)), ([120, 134], 4, (3, 3)), ([254], 3, (2,))]
        for lens, max_new, ks in layouts:
            def begin():
                for e, Tn in enumerate(lens):
                    _begin(m, e, 0, Tn, 50 * Tn + e)
            switch(m, False)
            begin()
            base, _ = _run(m, [(e, max_new) for e in range(len(lens))])
            switch(m, True)
            begin()
            _lib.check(m._lib.svln_op_fill_attn_state(m._h, R.SENTINEL, 0))
            for e in base:
                _set_draft(m, e, base[e]["ids"] + [9] * 6)
            run, iters = _run(m, [(e, max_new) for e in range(len(lens))])
            stats = m.batch_draft_stats(reset=True)
            turns = [BR.Turn(e, base[e]["ids"] + [0] * 8, base[e]["ids"] + [9] * 6, max_new, (), Tn, 0) for e, Tn in enumerate(lens)]
            want, log = BR.simulate(turns, MP, CFG.vocab)
            assert BR.broken_rules(turns, log, MP) == [] and tuple(t.k for t in turns) == ks, (lens, [t.k for t in turns])
            assert stats == want and iters == want[3], (lens, stats, want)
            for e in base:
                assert run[e]["ids"] == base[e]["ids"] and run[e]["kv_len"] == base[e]["kv_len"], (lens, e, run[e]["ids"], base[e]["ids"])
                assert np.abs(run[e]["hidden"] - base[e]["hidden"]).max() <= HIDDEN_TOL, (lens, e)
            written = _written(m, 2 * MP)
            rows = sum(Tn + max_new - 1 for Tn in lens)                       # prompt rows + every fed token (the drafts are right)
            pages = sum((Tn + max_new - 1 + 63) // 64 for Tn in lens)
            assert written.sum() == rows and len(np.nonzero(written.reshape(-1, 64).any(1))[0]) == pages, (lens, written.sum(), rows)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------ 5: bf16
def test_bf16_lockstep_five_envs_with_right_drafts():
    """the set-up of test_batched_lockstep_envs_equal_solo_runs (5 envs x 4 turns, bf16) with the mode-off run's ids as drafts, against
    that mode-off run, inside that test's bounds: first hidden row of every turn rel L2 < 3e-2, first-token agreement >= total - 2.  The
    counters are the restatement's on the ids the ride run itself emitted."""
    m = model(torch.bfloat16)
    seed0 = lambda e: 100 + e
    base = _lockstep(m, lambda e, t, mm: None, False, n_envs=5, seed0=seed0)
    gold = base["ids"]
    run = _lockstep(m, lambda e, t, mm: gold[e][t] if t < len(gold[e]) else None, True, n_envs=5, seed0=seed0)
    agree = total = 0
    worst = 0.0
    for e in range(5):
        assert len(run["ids"][e]) == len(gold[e]) == 4
        for t in range(4):
            total += 1
            agree += int(run["ids"][e][t][0] == gold[e][t][0])
            a, b = run["hidden"][e][t][0], base["hidden"][e][t][0]
            rel = float(np.linalg.norm(a - b) / np.linalg.norm(b))
            worst = max(worst, rel)
            print(f"bf16 batch ride env {e} turn {t}: rel L2 {rel:.3e}, ids {run['ids'][e][t]} vs mode off {gold[e][t]}")
            assert rel < 3e-2, (e, t, rel)
    print(f"bf16 batch rides: first-token agreement {agree}/{total}, worst rel L2 of a turn's first hidden row {worst:.2e}")
    assert agree >= total - 2, (agree, total)
    rides = 0
    for c, (recs, stats) in enumerate(run["calls"]):
        want, _, _ = _sim(recs, lambda r: run["ids"][r["env"]][r["turn"]])
        assert stats == want, (c, stats, want)
        rides += stats[0]
    assert rides >= 1
    switch(m, False)


# ------------------------------------------------------------------------------------------------------------ 6: the switch
def _three(m, max_new=5):
    for e, Tn in enumerate((33, 47, 64)):
        _begin(m, e, 0, Tn, 400 + e)
    return _run(m, [(e, max_new) for e in range(3)])[0]


def test_switch_off_leaves_the_draft_armed_and_on_consumes_it():
    m = model(torch.float32)
    try:
        plain = _three(m)
        # off: the scheduler neither reads nor disarms an armed draft; the next generate uses it
        _set_draft(m, 0, plain[0]["ids"])
        assert {e: r["ids"] for e, r in _three(m).items()} == {e: r["ids"] for e, r in plain.items()}
        assert m.batch_draft_stats()[:3] == (0, 0, 0)
        m.set_prefill_draft(True)
        m.prefill_draft_stats(reset=True)
        _begin(m, 0, 0, 33, 400)
        assert _fixed(m, 0, 5) == plain[0]["ids"] and m.prefill_draft_stats(reset=True)[0] == 1
        # off: a draft_ids key in a request arms nothing
        m.reset(8)
        ag = _agents(m, 1, lambda e: 7)[0]
        ag.observe(synthetic_frame(0, 0))
        req = ag._build_request("")
        out = m.generate_batch([dict(req, draft_ids=[5, 6, 7])])[0].sequences[0].tolist()
        m.reset(8)
        ag = _agents(m, 1, lambda e: 7)[0]
        ag.observe(synthetic_frame(0, 0))
        assert m.generate(**ag._build_request("")).sequences[0].tolist() == out and m.prefill_draft_stats(reset=True)[0] == 0
        m.set_prefill_draft(False)
        # on, no drafts: bit-identical to off
        m.reset(8)
        switch(m, True)
        on = _three(m)
        for e in plain:
            assert on[e]["ids"] == plain[e]["ids"] and on[e]["kv_len"] == plain[e]["kv_len"] and np.array_equal(on[e]["hidden"], plain[e]["hidden"]), e
        assert m.batch_draft_stats(reset=True)[:3] == (0, 0, 0)
        # on: the submit consumes the draft -- the ride happens, and the next generate has no draft
        _set_draft(m, 0, plain[0]["ids"])
        on = _three(m)
        assert [on[e]["ids"] for e in range(3)] == [plain[e]["ids"] for e in range(3)]
        assert m.batch_draft_stats(reset=True)[:3] == (1, 5, 4)
        m.set_prefill_draft(True)
        _begin(m, 0, 0, 33, 400)
        assert _fixed(m, 0, 5) == plain[0]["ids"] and m.prefill_draft_stats(reset=True)[0] == 0
        # on, under a repetition penalty: consumed and ignored, the turn is the plain penalised one
        switch(m, False)
        m.generation_config.repetition_penalty = 1.3
        m._sync_call_config()
        pen = _three(m)
        switch(m, True)
        _set_draft(m, 0, pen[0]["ids"])
        got = _three(m)
        for e in pen:
            assert got[e]["ids"] == pen[e]["ids"] and np.array_equal(got[e]["hidden"], pen[e]["hidden"]), e
        assert m.batch_draft_stats(reset=True)[:3] == (0, 0, 0)
        m.generation_config.repetition_penalty = 1.0
        m._sync_call_config()
        _begin(m, 0, 0, 33, 400)
        assert _fixed(m, 0, 5) == plain[0]["ids"] and m.prefill_draft_stats(reset=True)[0] == 0
        m.set_prefill_draft(False)
        # reset / reset_for_env / cancel drop a job's draft with the job
        for how in ("cancel", "reset_env", "reset"):
            _begin(m, 0, 0, 33, 400)
            _set_draft(m, 0, plain[0]["ids"])
            slot = _submit(m, 0, 5)
            if how == "cancel":
                _lib.check(m._lib.svln_batch_cancel(m._h, slot))
            elif how == "reset_env":
                _lib.check(m._lib.svln_reset_env(m._h, 0))
                _append(m, 0, _prompt(33, 401))
            else:
                m.reset(8)
                _append(m, 0, _prompt(33, 401))
            got, _ = _run(m, [(0, 5)])
            assert got[0]["ids"] == plain[0]["ids"] and m.batch_draft_stats(reset=True)[:3] == (0, 0, 0), how
    finally:
        m.generation_config.repetition_penalty = 1.0
        m._sync_call_config()
        m.set_prefill_draft(False)
        switch(m, False)


def test_refusals():
    m = StreamVLNForCausalLM(CFG, dtype=torch.bfloat16, max_envs=2, max_frames=3, max_positions=MAX_POSITIONS)
    try:
        m.load_synthetic(SEED)
        m.reset(1)
        m.set_batch_draft(True)
        m.set_batch_draft(True)                                # a call that changes nothing
        m.set_speculative(4)                                   # the three draft switches are independent
        m.set_prefill_draft(True)
        m.set_prefill_draft(False)
        m.set_speculative(0)
        m.set_batch_draft(False)
        switches = {"svln_set_fp8_decode": m.set_fp8_decode, "svln_set_mxfp4_decode": m.set_mxfp4_decode, "svln_set_fp8_gemm": m.set_fp8_gemm,
                    "svln_set_mxfp4_batched": m.set_mxfp4_batched, "svln_set_decode_persistent": m.set_decode_persistent}
        for sym, fn in switches.items():
            m.set_batch_draft(True)
            with pytest.raises(_lib.SvlnError, match=sym + ".*svln_set_batch_draft"):
                fn(True)
            fn(False)                                          # switching one off is always fine
            m.set_batch_draft(False)
            fn(True)
            with pytest.raises(_lib.SvlnError, match="svln_set_batch_draft.*" + sym):
                m.set_batch_draft(True)
            m.set_batch_draft(False)                           # nothing changes
            fn(False)
        # a change while a scheduler turn is in flight, either way
        _append(m, 0, np.arange(10, 30))
        _submit(m, 0, 4)
        with pytest.raises(_lib.SvlnError, match="in flight"):
            m.set_batch_draft(True)
        m.set_batch_draft(False)
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        m.set_batch_draft(True)
        _submit(m, 0, 4)
        with pytest.raises(_lib.SvlnError, match="in flight"):
            m.set_batch_draft(False)
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        m.set_batch_draft(False)
    finally:
        m.close()
