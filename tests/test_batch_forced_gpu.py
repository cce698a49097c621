"""Forced jobs in the multi-env scheduler (svln_batch_submit_forced / submit_forced / generate_batch_forced) on the GPU.

(1) Bit for bit: an iteration with forced jobs is the iteration whose callers spliced F[:-1] onto their prompts and submitted plain jobs
with max_new = 1 (layer 0's K / V rows of every env, the final-norm rows, the neighbours' tokens, greedy_ids[n - 1]); the counters are the
restatement's (tests/batch_forced_ref.py).  (2) The head: every chunk's outputs are the bits of svln_op_gemm_target /
svln_op_gemv_batched_target on the jobs' own final-norm rows, and on the fp32 engine every score lies inside the a-priori bound of
tests/test_forced_e2e_gpu.py.  (3) The fixtures (tiny_episode, true4_episode) as 8 lockstep envs and through the staggered scheduler with
every turn a forced job on the fixture's ids; a DAgger mix against the teacher-forced oracle; a plain run after forced runs against a
never-forced engine.  (4) Edges: the last position, an allowed list, sampling.  (5) Every refusal, the wrong kind of slot, the agents."""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_forced_ref as BF
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd import weights as Wt
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from test_e2e_gpu import BF16_HIDDEN_REL, HIDDEN_TOL
from test_forced_e2e_gpu import _check_scores, _head, _other
from util import load_golden

pytestmark = pytest.mark.gpu
MAX_POSITIONS = 2048
PI64, PF32, PI32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
SC = SCENARIOS["tiny_episode"]
CFG = SC["cfg"]
_models = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def model(dtype, name="tiny_episode"):
    """one 8-env engine per (configuration, dtype) for the module; every use starts from reset(8) with every switch off and the counters at 0"""
    sc = SCENARIOS[name]
    key = (name, dtype)
    if key not in _models:
        m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=8, max_frames=24, max_positions=MAX_POSITIONS)
        m.load_synthetic(SEED)
        _models[key] = m
    m = _models[key]
    m.model.num_history = sc["num_history"]
    m.reset(8)
    m.set_batch_draft(False); m.set_auto_draft(False)
    m.set_sampling(None); m.set_allowed_tokens(None); m.set_token_scores(False)
    m.batch_forced_stats(reset=True)
    return m


# ------------------------------------------------------------------------------------------------------------ the C ABI, env by slot
def _prompt(n, seed, vocab=None):
    return np.random.default_rng(seed).integers(5, vocab or CFG.vocab, size=n).astype(np.int64)


def _append(m, env, ids):
    a = np.ascontiguousarray(ids, dtype=np.int64)
    _lib.check(m._lib.svln_append_turn(m._h, env, a.ctypes.data_as(PI64), int(a.size), 0))


def _fixed(m, env, n):
    out = np.zeros(n, np.int64)
    _lib.check(m._lib.svln_generate_fixed(m._h, env, n, out.ctypes.data_as(PI64)))
    return out.tolist()


def _state(m, env):
    ne, kl = C.c_int32(), C.c_int32()
    _lib.check(m._lib.svln_env_state(m._h, env, C.byref(ne), C.byref(kl)))
    return ne.value, kl.value


def _submit(m, env, max_new, eos=()):
    e = np.asarray(eos, dtype=np.int64)
    slot = C.c_int32(-1)
    _lib.check(m._lib.svln_batch_submit(m._h, env, max_new, e.ctypes.data_as(PI64) if len(e) else None, len(e), C.byref(slot)))
    return slot.value


def _submit_forced_rc(m, env, F, eos=()):
    f = np.ascontiguousarray(F, dtype=np.int64)
    e = np.ascontiguousarray(eos, dtype=np.int64)
    slot = C.c_int32(-1)
    rc = m._lib.svln_batch_submit_forced(m._h, env, f.ctypes.data_as(PI64), int(f.size), e.ctypes.data_as(PI64) if e.size else None, int(e.size),
                                         C.byref(slot))
    return rc, slot.value


def _submit_forced(m, env, F, eos=()):
    rc, slot = _submit_forced_rc(m, env, F, eos)
    _lib.check(rc)
    return slot


def _step(m):
    running, nf = C.c_int32(), C.c_int32()
    fin = (C.c_int32 * 8)()
    _lib.check(m._lib.svln_batch_step(m._h, C.byref(running), fin, C.byref(nf)))
    return running.value, [fin[k] for k in range(nf.value)]


def _forced_out(m, slot, cap=32):
    lp, glp, gid, n = np.full(cap, 7.0, np.float32), np.full(cap, 7.0, np.float32), np.full(cap, -7, np.int64), C.c_int32(-1)
    _lib.check(m._lib.svln_batch_forced(m._h, slot, lp.ctypes.data_as(PF32), gid.ctypes.data_as(PI64), glp.ctypes.data_as(PF32), cap, C.byref(n)))
    return lp[: n.value], gid[: n.value].tolist(), glp[: n.value]


def _scores(m, slot, cap=64):
    buf, n = np.zeros(cap, np.float32), C.c_int32(-1)
    _lib.check(m._lib.svln_batch_scores(m._h, slot, buf.ctypes.data_as(PF32), cap, C.byref(n)))
    return buf[: n.value]


def _result(m, slot):
    out = np.zeros(64, np.int64)
    n, env = C.c_int32(), C.c_int32()
    _lib.check(m._lib.svln_batch_result(m._h, slot, C.byref(env), out.ctypes.data_as(PI64), 64, C.byref(n)))
    return env.value, out[: n.value].tolist()


def _kv(m, env, start, n, cfg=CFG):
    K = np.zeros((n, cfg.kv_heads, 128), np.float32)
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


def _collect(m, slots, fin, out, forced=()):
    """results of the finished slots `fin` (slots: slot -> env) into out[env]"""
    for s in fin:
        rec = dict(hidden=m.last_hidden_batch(s), slot=s)
        if s in forced:
            rec["lp"], rec["gid"], rec["glp"] = _forced_out(m, s)
            assert np.array_equal(_scores(m, s), rec["lp"])           # svln_batch_scores: the forced log-probabilities, whatever the switch says
        env, ids = _result(m, s)
        assert slots.pop(s) == env
        out[env] = dict(rec, ids=ids, kv_len=_state(m, env)[1])


def _run(m, jobs, eos=(), max_iters=64):
    """submit (env, max_new) in order, iterate until all are done -> ({env: dict(ids, hidden, kv_len, slot)}, iterations run)"""
    slots = {_submit(m, env, max_new, eos): env for env, max_new in jobs}
    out, iters = {}, 0
    while slots:
        assert iters < max_iters
        _, fin = _step(m)
        iters += 1
        _collect(m, slots, fin, out)
    return out, iters


# ------------------------------------------------------------------------------------------------------------ 1: forced == spliced prompts
#: per env (history rows P, prompt rows Tn, n).  small: n of 1, 2, 3, 5, 8 behind page edges and histories (19 head rows: one MFMA chunk).
#: page: n = 12 with the fed rows across a KV page edge (positions 58 .. 68).  n32: Tn + n - 1 = 271 rows across the 256-row fused-norm
#: limit of the product plans and the page edge at 256.  rows33: 8 + 8 + 8 + 8 + 1 = 33 head rows, so the second chunk holds one row.
CASES = {"small": [(20, 42, 1), (0, 62, 2), (70, 55, 3), (0, 30, 5), (0, 60, 8)],
         "page": [(0, 58, 12)],
         "n32": [(0, 240, 32)],
         "rows33": [(0, 30, 8), (10, 31, 8), (0, 59, 8), (0, 33, 8), (0, 34, 1)]}


@DTYPES
@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_forced_iteration_equals_spliced_prompts_bit_for_bit(case, dtype):
    m = model(dtype)
    envs = CASES[case]
    F = {e: _prompt(n, 900 + 10 * e + n).tolist() for e, (_, _, n) in enumerate(envs)}          # ids the policy did not choose

    def begin():
        for e, (P, Tn, n) in enumerate(envs):
            _begin(m, e, P, Tn, 1000 * len(envs) + 100 * e + Tn)
    # the callers splice F[:-1] on as text and submit plain jobs with max_new = 1: one iteration over the same segments
    begin()
    for e, (P, Tn, n) in enumerate(envs):
        if n > 1:
            _append(m, e, F[e][:-1])
    spliced, it_s = _run(m, [(e, 1) for e in range(len(envs))])
    kv_s = {e: _kv(m, e, P, Tn + n - 1) for e, (P, Tn, n) in enumerate(envs)}
    # the forced jobs
    begin()
    slots = {_submit_forced(m, e, F[e]): e for e in range(len(envs))}
    forced_slots = set(slots)
    running, fin = _step(m)
    kv_f = {e: _kv(m, e, P, Tn + n - 1) for e, (P, Tn, n) in enumerate(envs)}
    assert it_s == 1 and running == 0 and sorted(fin) == sorted(slots), (fin, "every forced job finishes in the iteration that prefills it")
    got = {}
    _collect(m, dict(slots), fin, got, forced=forced_slots)
    turns = [BF.Turn(e, P + Tn, P, F[e]) for e, (P, Tn, n) in enumerate(envs)]
    want, log = BF.simulate(turns, MAX_POSITIONS)
    stats = m.batch_forced_stats(reset=True)
    assert BF.broken_rules(turns, log, MAX_POSITIONS) == [] and tuple(stats.values()) == want, (stats, want)
    for e, (P, Tn, n) in enumerate(envs):
        for a, b, what in zip(kv_f[e], kv_s[e], "KV"):
            assert np.array_equal(a, b), (e, what, "rows of positions P .. P + Tn + n - 2", float(np.abs(a - b).max()))
        r = got[e]
        print(f"forced vs splice [{dtype}] {case} env {e} P={P} Tn={Tn} n={n}: greedy {r['gid']}, spliced token {spliced[e]['ids']}")
        assert r["ids"] == F[e] and r["kv_len"] == P + Tn + n - 1 and _state(m, e) == (P + Tn, P + Tn + n - 1)
        assert r["hidden"].shape[0] == min(n, 8)
        assert np.array_equal(r["hidden"][min(n, 8) - 1], spliced[e]["hidden"][0]), (e, "final-norm row of the last head row")
        assert r["gid"][n - 1] == spliced[e]["ids"][0], (e, r["gid"], spliced[e]["ids"])
        assert len(r["lp"]) == n and all(float(r["lp"][i]) <= float(r["glp"][i]) for i in range(n))
        for i in range(n):
            if r["gid"][i] == F[e][i]:
                assert r["lp"][i].tobytes() == r["glp"][i].tobytes(), (e, i)


@DTYPES
def test_mixed_iteration_equals_spliced_prompts_bit_for_bit(dtype):
    """two forced jobs, one plain prefill and two decode rows in ONE iteration: envs 3 and 4 prefill first and decode; then envs 0 (forced,
    n = 5), 1 (plain) and 2 (forced, n = 3) join.  Against the run whose callers spliced F[:-1] on: every env's layer-0 K / V rows, the
    final-norm rows, the neighbours' tokens to the end of their turns, greedy_ids[n - 1]."""
    m = model(dtype)
    lay = {0: (20, 42, 5), 1: (0, 37, 0), 2: (0, 62, 3), 3: (0, 33, 0), 4: (8, 25, 0)}
    F = {e: _prompt(n, 700 + e).tolist() for e, (_, _, n) in lay.items() if n}

    def run(forced):
        for e, (P, Tn, n) in lay.items():
            _begin(m, e, P, Tn, 4000 + 100 * e + Tn)
        slots = {_submit(m, e, 4): e for e in (3, 4)}
        running, fin = _step(m)
        assert running == 2 and fin == []
        fslots = set()
        for e in (0, 1, 2):
            if e in F and forced:
                s = _submit_forced(m, e, F[e])
                fslots.add(s)
            else:
                if e in F:
                    _append(m, e, F[e][:-1])
                s = _submit(m, e, 1 if e in F else 4)
            slots[s] = e
        out = {}
        running, fin = _step(m)                                 # the mixed iteration
        kv = {e: _kv(m, e, P, Tn + max(n - 1, 0) + (1 if e in (3, 4) else 0)) for e, (P, Tn, n) in lay.items()}
        assert running == 3 and sorted(slots[s] for s in fin) == [0, 2], (running, fin)
        _collect(m, slots, fin, out, forced=fslots)
        iters = 2
        while slots:
            assert iters < 16
            _, fin = _step(m)
            iters += 1
            _collect(m, slots, fin, out)
        return out, kv, iters

    spliced, kv_s, it_s = run(False)
    got, kv_f, it_f = run(True)
    stats = m.batch_forced_stats(reset=True)
    assert it_s == it_f and tuple(stats.values()) == (2, 6, 1), stats
    for e, (P, Tn, n) in lay.items():
        for a, b, what in zip(kv_f[e], kv_s[e], "KV"):
            assert np.array_equal(a, b), (e, what, float(np.abs(a - b).max()))
        if n:
            assert got[e]["ids"] == F[e] and got[e]["gid"][n - 1] == spliced[e]["ids"][0], (e, got[e]["gid"], spliced[e]["ids"])
            assert np.array_equal(got[e]["hidden"][n - 1], spliced[e]["hidden"][0]), e
            assert got[e]["kv_len"] == P + Tn + n - 1
        else:
            assert got[e]["ids"] == spliced[e]["ids"] and got[e]["kv_len"] == spliced[e]["kv_len"], (e, got[e]["ids"], spliced[e]["ids"])
            assert np.array_equal(got[e]["hidden"], spliced[e]["hidden"]), (e, "a neighbour's final-norm rows")


# ------------------------------------------------------------------------------------------------------------ 2: the head
def _ptr(t):
    return C.c_void_p(t.data_ptr())


#: n of the jobs of one iteration (slot order).  one chunk of 32 and one of a single row; a job that straddles the chunk edge (31 + 3 rows);
#: r = 2 (the batched GEMV); r = 3 (the MFMA tiles, padded to 4); r = 1
HEAD_CASES = [(8, 8, 8, 8, 1), (8, 8, 8, 7, 3), (2,), (3,), (1,), (5, 3)]


@DTYPES
def test_head_chunks_equal_the_target_ops_on_the_same_rows(dtype):
    m = model(dtype)
    cfg = m.cfg
    lm_head = torch.from_numpy(m.get_tensor("lm_head.weight")).to(dtype).cuda()
    Wd = _head(m)
    for ns in HEAD_CASES:
        F = {e: _prompt(n, 300 + 7 * e + n).tolist() for e, n in enumerate(ns)}
        for e, n in enumerate(ns):
            _begin(m, e, 0, 30 + 3 * e, 6000 + e)
        slots = {_submit_forced(m, e, F[e]): e for e in range(len(ns))}
        _, fin = _step(m)
        got = {}
        _collect(m, dict(slots), fin, got, forced=set(slots))
        # the head list: slot order, a job's n rows consecutive (n <= 8: every row has a tap row of its own)
        rows = np.concatenate([got[e]["hidden"] for e in range(len(ns))])
        tgt = [t for e in range(len(ns)) for t in F[e]]
        lp = np.concatenate([got[e]["lp"] for e in range(len(ns))])
        glp = np.concatenate([got[e]["glp"] for e in range(len(ns))])
        gid = [t for e in range(len(ns)) for t in got[e]["gid"]]
        assert rows.shape[0] == len(tgt) == sum(ns)
        stats = m.batch_forced_stats(reset=True)
        assert stats["head_launches"] == len(BF.chunks_of(len(tgt))), stats
        for r0, r in BF.chunks_of(len(tgt)):
            launched, form = BF.head_route(r)
            x = torch.from_numpy(np.concatenate([rows[r0:r0 + r], np.repeat(rows[r0:r0 + 1], launched - r, 0)])).to(dtype).cuda().contiguous()
            tg = (C.c_int32 * 32)(*(tgt[r0:r0 + r] + [-1] * (launched - r)))
            toks, og, ol = (C.c_int32 * 32)(), (C.c_float * 32)(), (C.c_float * 32)()
            torch.cuda.synchronize()
            if form == "gemv":
                _lib.check(m._lib.svln_op_gemv_batched_target(m._h, _ptr(lm_head), cfg.hidden, _ptr(x), cfg.hidden, cfg.vocab, cfg.hidden, launched, tg,
                                                              1.0, toks, og, ol, None))
            else:
                _lib.check(m._lib.svln_op_gemm_target(m._h, _ptr(x), cfg.hidden, _ptr(lm_head), cfg.hidden, launched, cfg.vocab, cfg.hidden, tg, 1.0, toks,
                                                      og, ol, None))
            assert gid[r0:r0 + r] == [int(toks[k]) for k in range(r)], (ns, r0, r)
            assert glp[r0:r0 + r].tobytes() == np.asarray([og[k] for k in range(r)], np.float32).tobytes(), (ns, r0, r, "greedy_logprobs")
            assert lp[r0:r0 + r].tobytes() == np.asarray([ol[k] for k in range(r)], np.float32).tobytes(), (ns, r0, r, "logprobs")
        for e, n in enumerate(ns):
            for i in range(n):
                if got[e]["gid"][i] == F[e][i]:
                    assert got[e]["lp"][i].tobytes() == got[e]["glp"][i].tobytes(), (ns, e, i)
            if dtype == torch.float32:
                worst = _check_scores(Wd, got[e]["lp"], got[e]["hidden"], F[e], what=(ns, e))
                print(f"head {ns} env {e}: worst |score - ref| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------ 3: the fixtures
def _agents(m, name, n_envs):
    """n_envs agents that each run the fixture's own episode (its prompt seed, env 0's frame stream)"""
    sc = SCENARIOS[name]
    proc = m.get_vision_tower().image_processor
    out = []
    for e in range(n_envs):
        enc = SyntheticPromptEncoder(sc["cfg"], seed=sc.get("prompt_seed", 7), first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        out.append(StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                                  device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=proc.preprocess_array))
    return out


def _gold(name):
    g = load_golden(name)
    return g, [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]


def _check_fixture_turn(name, dtype, g, gold, t, out, hid, e):
    n = len(gold[t])
    assert out.sequences[0].tolist() == gold[t] and out.past_key_values.get_seq_length() == int(g[f"t{t}_cache_len"]), (name, e, t)
    assert tuple(out.token_logprobs.shape) == (1, n) and tuple(out.greedy_ids.shape) == (1, n) and tuple(out.greedy_logprobs.shape) == (1, n)
    hf = g[f"t{t}_hidden"]
    k = min(n, 8, hid.shape[0])
    assert hid.shape[0] == min(n, 8)
    if dtype == torch.float32:
        assert float(np.abs(hid[:k] - hf[:k]).max()) <= HIDDEN_TOL, (name, e, t)
        assert out.greedy_ids[0].tolist() == gold[t], (name, e, t, out.greedy_ids[0].tolist(), gold[t])
        assert out.token_logprobs.numpy().tobytes() == out.greedy_logprobs.numpy().tobytes(), (name, e, t)
    else:
        for j in range(k):
            rel = float(np.linalg.norm(hid[j] - hf[j]) / np.linalg.norm(hf[j]))
            assert rel < BF16_HIDDEN_REL[name], (name, e, t, j, rel)


@DTYPES
@pytest.mark.parametrize("name", ["tiny_episode", "true4_episode"])
def test_lockstep_envs_forced_onto_the_fixtures_ids_reproduce_the_fixtures(name, dtype):
    """8 envs in lockstep through BatchedAgents.act(forced_ids=...), every turn a forced job on the fixture's ids (tiny_episode: through two
    window restarts, whose segments do not fit one pass, so jobs wait)"""
    sc = SCENARIOS[name]
    g, gold = _gold(name)
    m = model(dtype, name)
    N = 8
    agents = _agents(m, name, N)
    group = BatchedAgents(agents)
    hidden = [[] for _ in range(N)]
    iters0 = m.batch_draft_stats(reset=True)
    for step in range(sc["steps"]):
        t = len(agents[0].turn_log)
        due = len(agents[0].action_seq) == 0
        if not due:
            with pytest.raises(ValueError, match="no model turn"):
                group.act([synthetic_frame(0, step)] * N, forced_ids={3: gold[0]})
        group.act([synthetic_frame(0, step)] * N, forced_ids=[gold[t]] * N if due else None)
        if due:
            for e in range(N):
                hidden[e].append(m.last_hidden_batch(e))
    stats, iters = m.batch_forced_stats(reset=True), m.batch_draft_stats(reset=True)[3]
    assert [len(a.turn_log) for a in agents] == [len(gold)] * N
    assert stats["jobs"] == N * len(gold) and stats["rows_fed"] == N * sum(len(x) - 1 for x in gold), stats
    if name == "tiny_episode":
        assert any(r["memory"] for r in agents[0].turn_log) and iters > len(gold), (iters, "a restart turn of 8 envs takes more than one pass: jobs wait")
    for e, a in enumerate(agents):
        for t, rec in enumerate(a.turn_log):
            _check_fixture_turn(name, dtype, g, gold, t, rec["out"], hidden[e][t], e)
        assert a.last_greedy_ids is not None and a.last_token_logprobs is not None
        assert abs(a.last_turn_logprob - float(a.turn_log[-1]["out"].token_logprobs.sum())) <= 1e-6


@DTYPES
def test_staggered_scheduler_forced_onto_the_fixtures_ids_reproduces_the_fixture(dtype):
    """8 envs with staggered starts through AsyncBatchedAgents.tick(forced_ids=...): every env runs tiny_episode, every turn is a forced job
    on the fixture's ids and finishes in the tick that submits it"""
    name = "tiny_episode"
    sc = SCENARIOS[name]
    g, gold = _gold(name)
    m = model(dtype, name)
    N = 8
    agents = _agents(m, name, N)
    hidden = [[] for _ in range(N)]
    group = AsyncBatchedAgents(agents, on_result=lambda i, ticket, out: hidden[i].append(m.last_hidden_batch(ticket.slot)))
    tick = 0
    while min(len(a.turn_log) for a in agents) < len(gold):
        assert tick < 4 * sc["steps"]
        active = {i for i in range(N) if tick >= i and len(agents[i].turn_log) + (not agents[i].pending_turn and not agents[i].action_seq) <= len(gold)}
        busy = set(group.waiting.values())
        forced = {i: gold[len(agents[i].turn_log)] for i in active if i not in busy and not agents[i].pending_turn and not agents[i].action_seq}
        if tick == 1:
            with pytest.raises(ValueError, match="submits no model turn"):
                group.tick([synthetic_frame(0, a.step_id) for a in agents], active=active, forced_ids={7: gold[0]})
        group.tick([synthetic_frame(0, a.step_id) for a in agents], active=active, forced_ids=forced)
        tick += 1
    assert not group.waiting
    stats = m.batch_forced_stats(reset=True)
    assert stats["jobs"] == N * len(gold), stats
    assert any(r["memory"] for r in agents[0].turn_log)
    for e, a in enumerate(agents):
        assert len(a.turn_log) == len(gold) == len(hidden[e])
        for t, rec in enumerate(a.turn_log):
            _check_fixture_turn(name, dtype, g, gold, t, rec["out"], hidden[e][t], e)


@DTYPES
def test_dagger_mix_forced_envs_follow_the_oracle_and_plain_envs_the_fixture(dtype):
    """6 lockstep envs on tiny_episode, two turns.  Turn 0: envs 0, 2, 4 are forced onto the fixture's ids with one id replaced (at index 0,
    1, last) by an id that is neither the policy's nor in the EOS set, envs 1, 3, 5 run plain; turn 1 is plain for all.  The forced envs
    against the oracle teacher-forced on the same ids (their next plain turn too); the plain envs against the fixture inside the bounds
    of test_batched_lockstep_envs_equal_solo_runs (fp32: ids equal, hidden <= 1e-3; bf16: first row rel L2 < 3e-2, first ids agree but 2)."""
    name = "tiny_episode"
    sc = SCENARIOS[name]
    g, gold = _gold(name)
    m = model(dtype, name)
    N, steps = 6, 2 * sc["nfs"]
    where = {0: 0, 2: 1, 4: len(gold[0]) - 1}
    F = {}
    for e, j in where.items():
        F[e] = list(gold[0])
        F[e][j] = _other(gold[0][j], sc)
    agents = _agents(m, name, N)
    group = BatchedAgents(agents)
    hidden = [[] for _ in range(N)]
    for step in range(steps):
        due = len(agents[0].action_seq) == 0
        first = len(agents[0].turn_log) == 0
        group.act([synthetic_frame(0, step)] * N, forced_ids=F if due and first else None)
        if due:
            for e in range(N):
                hidden[e].append(m.last_hidden_batch(e))
    assert m.batch_forced_stats(reset=True)["jobs"] == 3
    agree = total = 0
    for e, a in enumerate(agents):
        assert len(a.turn_log) == 2
        o0, o1 = a.turn_log[0]["out"], a.turn_log[1]["out"]
        if e in F:
            orc = O.OracleStreamVLN(sc["cfg"], Wt.synth_state_dict(sc["cfg"], SEED), num_history=sc["num_history"])
            orc.teacher_tokens = [list(F[e])]
            log_o = run_scenario(orc, sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, steps=steps)
            r0, r1 = log_o[0]["out"], log_o[1]["out"]
            assert o0.sequences[0].tolist() == F[e] == r0.sequences[0].tolist() and o0.past_key_values.get_seq_length() == r0.cache_len, e
            gid = o0.greedy_ids[0].tolist()
            j = where[e]
            assert gid[j] != F[e][j] and float(o0.token_logprobs[0, j]) < float(o0.greedy_logprobs[0, j]), (e, gid)
            assert "greedy_ids" not in o1 and "token_logprobs" not in o1
            if dtype == torch.float32:
                assert float(np.abs(hidden[e][0] - r0.hidden.numpy()).max()) <= HIDDEN_TOL and gid == r0.own_picks, (e, gid, r0.own_picks)
                assert o1.sequences[0].tolist() == r1.sequences[0].tolist() and o1.past_key_values.get_seq_length() == r1.cache_len, e
                k = min(len(hidden[e][1]), r1.hidden.shape[0])
                assert float(np.abs(hidden[e][1][:k] - r1.hidden.numpy()[:k]).max()) <= HIDDEN_TOL, e
            else:
                for r in range(len(F[e])):
                    rel = float(np.linalg.norm(hidden[e][0][r] - r0.hidden.numpy()[r]) / np.linalg.norm(r0.hidden.numpy()[r]))
                    assert rel < BF16_HIDDEN_REL[name], (e, r, rel)
                rel = float(np.linalg.norm(hidden[e][1][0] - r1.hidden.numpy()[0]) / np.linalg.norm(r1.hidden.numpy()[0]))
                assert rel < BF16_HIDDEN_REL[name], (e, rel)
        else:
            for t, out in enumerate((o0, o1)):
                hf = g[f"t{t}_hidden"]
                if dtype == torch.float32:
                    assert out.sequences[0].tolist() == gold[t], (e, t)
                    k = min(len(hidden[e][t]), hf.shape[0])
                    assert float(np.abs(hidden[e][t][:k] - hf[:k]).max()) <= HIDDEN_TOL, (e, t)
                else:
                    total += 1
                    agree += int(out.sequences[0, 0].item() == gold[t][0])
                    rel = float(np.linalg.norm(hidden[e][t][0] - hf[0]) / np.linalg.norm(hf[0]))
                    assert rel < 3e-2, (e, t, rel)
    assert dtype == torch.float32 or agree >= total - 2, (agree, total)


def _three(m, max_new=5):
    for e, Tn in enumerate((33, 47, 64)):
        _begin(m, e, 0, Tn, 400 + e)
    return _run(m, [(e, max_new) for e in range(3)])[0]


@DTYPES
def test_plain_run_after_forced_runs_equals_a_never_forced_engine_bit_for_bit(dtype):
    fresh = StreamVLNForCausalLM(CFG, dtype=dtype, max_envs=8, max_frames=24, max_positions=MAX_POSITIONS)
    try:
        fresh.load_synthetic(SEED)
        fresh.reset(8)
        want = _three(fresh)
    finally:
        fresh.close()
    m = model(dtype)
    for ns in ((32, 32, 8), (1,), (5, 3)):
        for e, n in enumerate(ns):
            _begin(m, e, 0, 40 + e, 70 + e)
        slots = {_submit_forced(m, e, _prompt(n, 50 + e).tolist()): e for e, n in enumerate(ns)}
        _, fin = _step(m)
        for s in fin:
            _result(m, s)
    assert m.batch_forced_stats(reset=True)["jobs"] == 6
    got = _three(m)
    for e in want:
        assert got[e]["ids"] == want[e]["ids"] and got[e]["kv_len"] == want[e]["kv_len"] and np.array_equal(got[e]["hidden"], want[e]["hidden"]), e


# ------------------------------------------------------------------------------------------------------------ 4: edges
def _written(m, n_positions, cfg=CFG):
    import attn_ref as R
    K, Vv = _kv(m, -1, 0, n_positions, cfg)
    return (K != np.float32(R.SENTINEL)).any((1, 2)) | (Vv != np.float32(R.SENTINEL)).any((1, 2))


def test_last_position_waiting_jobs_and_the_prepared_pages():
    """max_positions = 256.  n_embeds + n - 1 == 256 is accepted and one more id refused; with layer 0's pools set to a sentinel before
    the run nothing is written outside the pages of the rows the iteration prepared.  Two jobs whose segments do not fit one pass: the
    second waits, whole, and runs in the next iteration; a job that does not fit beside two decode rows runs once they have left."""
    import attn_ref as R
    MP = 256
    m = StreamVLNForCausalLM(CFG, dtype=torch.float32, max_envs=3, max_frames=3, max_positions=MP)
    try:
        m.load_synthetic(SEED)
        m.reset(3)
        _begin(m, 0, 0, 240, 1)
        rc, _ = _submit_forced_rc(m, 0, list(range(5, 23)))                 # 240 + 18 - 1 > 256
        assert rc != 0 and "max_positions" in m._lib.svln_last_error().decode() and _state(m, 0) == (240, 0)
        _lib.check(m._lib.svln_op_fill_attn_state(m._h, R.SENTINEL, 0))
        F = list(range(5, 22))
        slot = _submit_forced(m, 0, F)                                      # 240 + 17 - 1 == 256
        running, fin = _step(m)
        assert running == 0 and fin == [slot] and _state(m, 0) == (240, 256)
        written = _written(m, 3 * MP)
        assert written.sum() == 256 and len(np.nonzero(written.reshape(-1, 64).any(1))[0]) == 4, written.sum()
        assert _result(m, slot) == (0, F)
        # two segments of 150 + 4 rows: the second job waits whole and runs alone
        m.batch_forced_stats(reset=True)
        for e in (0, 1):
            _begin(m, e, 0, 150, 10 + e)
        F5 = {e: _prompt(5, 20 + e).tolist() for e in (0, 1)}
        slots = {_submit_forced(m, e, F5[e]): e for e in (0, 1)}
        first = _step(m)
        second = _step(m)
        assert first[0] == 1 and [slots[s] for s in first[1]] == [0] and second[0] == 0 and [slots[s] for s in second[1]] == [1], (first, second)
        lone = {}
        for s in list(slots):
            lp, gid, glp = _forced_out(m, s)
            lone[slots[s]] = (lp.copy(), gid, glp.copy())
            assert _result(m, s) == (slots[s], F5[slots[s]])
        turns = [BF.Turn(e, 150, 0, F5[e]) for e in (0, 1)]
        want, log = BF.simulate(turns, MP)
        assert tuple(m.batch_forced_stats(reset=True).values()) == want == (2, 8, 2) and [t.first_iteration for t in turns] == [0, 1]
        # the waiting job computed what it computes alone
        _begin(m, 1, 0, 150, 11)
        s = _submit_forced(m, 1, F5[1])
        _step(m)
        lp, gid, glp = _forced_out(m, s)
        _result(m, s)
        assert np.array_equal(lp, lone[1][0]) and gid == lone[1][1] and np.array_equal(glp, lone[1][2])
        # a job of 250 + 5 rows beside two decode rows: it waits until they have left
        for e, Tn in ((0, 20), (1, 21), (2, 250)):
            _begin(m, e, 0, Tn, 30 + e)
        slots = {_submit(m, 0, 3): 0, _submit(m, 1, 3): 1}
        assert _step(m) == (2, [])
        F6 = _prompt(6, 44).tolist()
        fs = _submit_forced(m, 2, F6)
        slots[fs] = 2
        seen = []
        while slots:
            running, fin = _step(m)
            seen.append(sorted(slots[s] for s in fin))
            for s in fin:
                assert _result(m, s)[0] == slots.pop(s)
            assert len(seen) < 8
        assert seen == [[], [0, 1], [2]] and _state(m, 2) == (250, 255), seen
    finally:
        m.close()


@DTYPES
def test_allowed_list(dtype):
    """the head is the subset product: the score of F[i] is the bits of row i of svln_batch_allowed_logprobs at F[i]'s list position, the
    rows are those of the single-env forced turn on the same prompt, greedy ids lie in the list; an id outside the list is refused"""
    m = model(dtype)
    V = CFG.vocab
    allowed = sorted(set(_prompt(40, 3, V).tolist()))
    Fs = {0: [allowed[3], allowed[17], allowed[0], allowed[-1], allowed[17]], 1: [allowed[5]], 2: [allowed[2], allowed[9], allowed[9]]}
    try:
        m.set_allowed_tokens(allowed, add_eos=False)
        for T in (None, 0.5):
            m.set_sampling(T, 5) if T else m.set_sampling(None)
            solo = {}
            for e, F in Fs.items():                             # the single-env forced turn: its rows are the yardstick
                _begin(m, e, 0, 50 + e, 7 + e)
                f = np.ascontiguousarray(F, dtype=np.int64)
                n = len(F)
                lp, glp, gid, kv = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64), C.c_int32()
                _lib.check(m._lib.svln_generate_forced(m._h, e, f.ctypes.data_as(PI64), n, None, 0, lp.ctypes.data_as(PF32), gid.ctypes.data_as(PI64),
                                                       glp.ctypes.data_as(PF32), C.byref(kv)))
                buf, nt, ni = np.zeros(n * len(allowed), np.float32), C.c_int32(), C.c_int32()
                _lib.check(m._lib.svln_get_allowed_logprobs(m._h, buf.ctypes.data_as(PF32), int(buf.size), C.byref(nt), C.byref(ni)))
                solo[e] = buf.reshape(n, len(allowed)).copy()
            # one job alone in its iteration runs the single-env turn's launches on the same rows: the same rows bit for bit
            _begin(m, 0, 0, 50, 7)
            s = _submit_forced(m, 0, Fs[0])
            assert _step(m) == (0, [s])
            buf, nt, ni = np.zeros(len(Fs[0]) * len(allowed), np.float32), C.c_int32(), C.c_int32()
            _lib.check(m._lib.svln_batch_allowed_logprobs(m._h, s, buf.ctypes.data_as(PF32), int(buf.size), C.byref(nt), C.byref(ni)))
            assert np.array_equal(buf.reshape(len(Fs[0]), len(allowed)), solo[0]), (T, "rows of a job alone vs the single-env forced turn")
            _result(m, s)
            for e in Fs:
                _begin(m, e, 0, 50 + e, 7 + e)
            state = _state(m, 0)
            outside = next(t for t in range(5, V) if t not in allowed)
            rc, _ = _submit_forced_rc(m, 0, [allowed[1], outside, allowed[2]])
            assert rc != 0 and "allowed list" in m._lib.svln_last_error().decode() and _state(m, 0) == state
            slots = {_submit_forced(m, e, F): e for e, F in Fs.items()}
            _, fin = _step(m)
            assert sorted(fin) == sorted(slots)
            for s in fin:
                e = slots[s]
                F = Fs[e]
                lp, gid, glp = _forced_out(m, s)
                buf, nt, ni = np.zeros(len(F) * len(allowed), np.float32), C.c_int32(), C.c_int32()
                _lib.check(m._lib.svln_batch_allowed_logprobs(m._h, s, buf.ctypes.data_as(PF32), int(buf.size), C.byref(nt), C.byref(ni)))
                assert (nt.value, ni.value) == (len(F), len(allowed))
                alp = buf.reshape(len(F), len(allowed))
                for i, f in enumerate(F):
                    assert lp[i].tobytes() == alp[i, allowed.index(f)].tobytes(), (T, e, i)
                    assert gid[i] in allowed and gid[i] == allowed[int(np.argmax(alp[i]))]
                    assert abs(float(glp[i]) - float(alp[i].max())) <= 2e-5
                assert abs(float(np.exp(alp.astype(np.float64)).sum(1).max()) - 1.0) <= 1e-4
                # (beside neighbours the prefill products take other tile plans than alone: reported, not asserted)
                print(f"allowed list [{dtype}] T={T} env {e}: max |row - single-env row| = {float(np.abs(alp.astype(np.float64) - solo[e]).max()):.3e}")
                _result(m, s)
    finally:
        m.set_sampling(None)
        m.set_allowed_tokens(None)


@DTYPES
def test_sampling_scores_and_the_untouched_draw_counters(dtype):
    """T = 1/2: the forced scores are of softmax(logits / T) (inside the a-priori bound, scaled by 1 / T, of float64 from the job's own tap
    rows; different numbers from the run with sampling off); no draw counter moves: the next sampled turn of every env equals the one of a
    twin whose counters were restarted after its forced jobs"""
    m = model(dtype)
    T, seed = 0.5, 21
    inv_t = float(np.float32(1.0) / np.float32(T))
    Wd = _head(m)
    lay = {0: (50, 5), 1: (41, 2), 2: (33, 8)}
    F = {e: _prompt(n, 80 + e).tolist() for e, (_, n) in lay.items()}
    nxt = {e: _prompt(9, 8 + e).tolist() for e in lay}

    def forced_jobs():
        for e, (Tn, n) in lay.items():
            _begin(m, e, 0, Tn, 7 + e)
        slots = {_submit_forced(m, e, F[e]): e for e in lay}
        _, fin = _step(m)
        out = {}
        _collect(m, slots, fin, out, forced=set(fin))
        return out

    def sampled_turns(prev):
        for e in lay:
            _append(m, e, list(prev[e]) + nxt[e])              # (the caller's next inputs: the last turn's ids, then the new prompt)
        return {e: r["ids"] for e, r in _run(m, [(e, 5) for e in lay])[0].items()}
    try:
        m.set_sampling(T, seed)
        hot = forced_jobs()
        for e in lay:
            worst = _check_scores(Wd, hot[e]["lp"], hot[e]["hidden"], F[e], inv_t, what=("sampling", e, str(dtype)))
            print(f"sampling [{dtype}] env {e}: worst |score - ref| / bound = {worst:.3f}")
        ids_hot = sampled_turns(F)
        # the twin: its forced jobs ran with sampling off; the counters start when the switch goes on
        m.set_sampling(None)
        cold = forced_jobs()
        assert all(not np.array_equal(cold[e]["lp"], hot[e]["lp"]) for e in lay)
        m.set_sampling(T, seed)
        ids_twin = sampled_turns(F)
        assert ids_hot == ids_twin, (ids_hot, ids_twin)
        # turns sampled with draws that HAVE moved differ
        moved = sampled_turns(ids_twin)
        assert moved != ids_hot
    finally:
        m.set_sampling(None)


# ------------------------------------------------------------------------------------------------------------ 5: rules
def test_refusals_leave_everything_as_found():
    m = StreamVLNForCausalLM(CFG, dtype=torch.bfloat16, max_envs=8, max_frames=3, max_positions=256)
    try:
        m.load_synthetic(SEED)
        V = CFG.vocab
        F = [11, 12, 13]
        draft = np.asarray([21, 22, 23, 24], np.int64)

        def refused(ids, match, eos=(), env=0):
            state = _state(m, env)
            rc, _ = _submit_forced_rc(m, env, ids, eos)
            err = m._lib.svln_last_error().decode()
            assert rc != 0 and match in err, (ids, match, err)
            assert _state(m, env) == state
            # the dry run (slot == NULL) gives the same answer for every refusal that needs no rows of the env
            if match not in ("nothing to prefill", "max_positions"):
                f, e = np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(eos, dtype=np.int64)
                assert m._lib.svln_batch_submit_forced(m._h, env, f.ctypes.data_as(PI64), int(f.size), e.ctypes.data_as(PI64) if e.size else None,
                                                       int(e.size), None) != 0 and match in m._lib.svln_last_error().decode()

        m.reset(8)
        _lib.check(m._lib.svln_set_draft(m._h, 0, draft.ctypes.data_as(PI64), 4))      # armed throughout: no refusal may consume it
        refused(F, "nothing to prefill")
        _begin(m, 0, 0, 40, 1)
        refused([], "1 .. 32")
        refused(list(range(5, 38)), "1 .. 32")
        refused([11, V, 13], "outside the vocabulary")
        refused([11, -1, 13], "outside the vocabulary")
        refused([11, 12, 13], "EOS", eos=(12,))
        _begin(m, 0, 0, 240, 1)
        refused(list(range(5, 23)), "max_positions")
        _begin(m, 0, 0, 40, 1)
        _lib.check(m._lib.svln_set_repetition_penalty(m._h, 1.3))
        refused(F, "svln_set_repetition_penalty")
        _lib.check(m._lib.svln_set_repetition_penalty(m._h, 1.0))
        for sym, fn in {"svln_set_fp8_decode": m.set_fp8_decode, "svln_set_mxfp4_decode": m.set_mxfp4_decode, "svln_set_fp8_gemm": m.set_fp8_gemm,
                        "svln_set_mxfp4_batched": m.set_mxfp4_batched, "svln_set_decode_persistent": m.set_decode_persistent}.items():
            fn(True)
            refused(F, sym)
            fn(False)
        allowed = sorted(set(_prompt(20, 3).tolist()) - {11, 12, 13})
        m.set_allowed_tokens(allowed, add_eos=False)
        refused(F, "allowed list")
        m.set_allowed_tokens(None)
        # the job table is as found: no turn is in flight ...
        assert _step(m) == (0, [])
        # ... and the draft is still armed: with svln_set_batch_draft on a plain submit rides it
        m.set_batch_draft(True)
        m.batch_draft_stats(reset=True)
        _begin(m, 0, 0, 40, 1)
        _run(m, [(0, 3)])
        assert m.batch_draft_stats(reset=True)[0] == 1
        m.set_batch_draft(False)
        # a pending group
        m.set_sampling(1.0, 3)
        _begin(m, 0, 0, 40, 1)
        out, n_out = np.zeros((2, 3), np.int64), np.zeros(2, np.int32)
        _lib.check(m._lib.svln_generate_group(m._h, 0, 2, 3, None, 0, out.ctypes.data_as(PI64), 3, n_out.ctypes.data_as(PI32)))
        rc, _ = _submit_forced_rc(m, 0, F)
        assert rc != 0 and "svln_group_select" in m._lib.svln_last_error().decode()
        _lib.check(m._lib.svln_group_select(m._h, 0, 0, None))
        m.set_sampling(None)
        # an env with a turn in flight (the other slots are free: the slot a later submit gets is the lowest free one, as before)
        for e in range(3):
            _begin(m, e, 0, 20 + e, 60 + e)
        assert _submit(m, 0, 2) == 0
        refused(F, "already has a turn in flight")
        assert _submit_forced(m, 1, F) == 1 and _submit(m, 2, 2) == 2
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        # the armed draft: consumed by an accepted forced submit iff svln_set_batch_draft is on, and never read
        for on in (True, False):
            m.set_batch_draft(on)
            m.batch_draft_stats(reset=True)
            _begin(m, 0, 0, 40, 1)
            _lib.check(m._lib.svln_set_draft(m._h, 0, draft.ctypes.data_as(PI64), 4))
            s = _submit_forced(m, 0, F)
            assert _step(m) == (0, [s]) and _result(m, s) == (0, F)
            m.set_batch_draft(True)
            _append(m, 0, F + _prompt(9, 5).tolist())
            _run(m, [(0, 3)])
            assert m.batch_draft_stats(reset=True)[0] == (0 if on else 1), on
        m.set_batch_draft(False)
        # svln_generate_forced keeps its idle-scheduler refusal while a forced job is in flight on another env
        _begin(m, 0, 0, 40, 1)
        _begin(m, 1, 0, 30, 2)
        _submit_forced(m, 1, F)
        f = np.asarray(F, np.int64)
        lp, glp, gid = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.int64)
        assert m._lib.svln_generate_forced(m._h, 0, f.ctypes.data_as(PI64), 3, None, 0, lp.ctypes.data_as(PF32), gid.ctypes.data_as(PI64),
                                           glp.ctypes.data_as(PF32), None) != 0 and "in flight" in m._lib.svln_last_error().decode()
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
    finally:
        m.close()


def test_getters_on_the_wrong_kind_of_slot():
    m = model(torch.bfloat16)
    m.set_token_scores(True)
    m.set_top_logprobs(3)
    try:
        _begin(m, 0, 0, 30, 1)
        _begin(m, 1, 0, 31, 2)
        F = [11, 12, 13]
        sf, sp = _submit_forced(m, 0, F), _submit(m, 1, 1)
        running, fin = _step(m)
        assert running == 0 and sorted(fin) == sorted([sf, sp])
        ids, lps, nr, nk = np.zeros(8 * 3, np.int32), np.zeros(8 * 3, np.float32), C.c_int32(), C.c_int32()
        args = (ids.ctypes.data_as(PI32), lps.ctypes.data_as(PF32), 8, C.byref(nr), C.byref(nk))
        assert m._lib.svln_batch_topk(m._h, sf, *args) != 0
        err = m._lib.svln_last_error().decode()
        assert "svln_batch_topk" in err and "forced" in err, err
        _lib.check(m._lib.svln_batch_topk(m._h, sp, *args))
        assert (nr.value, nk.value) == (1, 3)
        lp, glp, gid, n = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.int64), C.c_int32()
        assert m._lib.svln_batch_forced(m._h, sp, lp.ctypes.data_as(PF32), gid.ctypes.data_as(PI64), glp.ctypes.data_as(PF32), 8, C.byref(n)) != 0
        err = m._lib.svln_last_error().decode()
        assert "svln_batch_forced" in err and "plain" in err, err
        assert len(_forced_out(m, sf)[0]) == 3 and m.last_hidden_batch(sf).shape[0] == 3
        assert _result(m, sf) == (0, F) and _result(m, sp)[0] == 1
        # freed: the forced getters are refused as on any empty slot
        assert m._lib.svln_batch_forced(m._h, sf, lp.ctypes.data_as(PF32), gid.ctypes.data_as(PI64), glp.ctypes.data_as(PF32), 8, C.byref(n)) != 0
    finally:
        m.set_top_logprobs(0)
        m.set_token_scores(False)


def test_python_requests_mix_forced_and_plain_and_refuse_before_anything_changes():
    """generate_batch_forced: forced and plain requests in one call, results in request order with the keys of generate(forced_ids=...);
    submit / generate_batch still raise NotImplementedError; a refused submit_forced leaves the env, curr_t and the tickets as found"""
    name = "tiny_episode"
    g, gold = _gold(name)
    m = model(torch.float32, name)
    m.set_token_scores(True)
    try:
        agents = _agents(m, name, 3)
        for a in agents:
            a.observe(synthetic_frame(0, 0))
        reqs = [a._build_request("") for a in agents]
        with pytest.raises(NotImplementedError, match="forced_ids"):
            m.submit(**dict(reqs[0], forced_ids=gold[0]))
        with pytest.raises(NotImplementedError, match="forced_ids"):
            m.generate_batch([dict(reqs[0], forced_ids=gold[0])])
        before = (m.env_state(1), list(m.curr_t), dict(m._tickets))
        for bad, match in (([6] * 33, "1 .. 32"), ([6, CFG.vocab], "vocabulary"), ([eos_ids(SC)[0], 6], "EOS")):
            with pytest.raises((ValueError, _lib.SvlnError), match=match):
                m.submit_forced(**dict(reqs[1], forced_ids=bad))
            assert (m.env_state(1), list(m.curr_t), dict(m._tickets)) == before, bad
        outs = m.generate_batch_forced([dict(reqs[0], forced_ids=gold[0]), reqs[1], dict(reqs[2], forced_ids=gold[0][:1])])
        assert [o.sequences[0].tolist() for o in outs] == [gold[0], gold[0], gold[0][:1]]
        assert "greedy_ids" in outs[0] and "greedy_ids" not in outs[1] and tuple(outs[2].greedy_ids.shape) == (1, 1)
        assert tuple(outs[1].token_logprobs.shape) == (1, len(gold[0]))      # (set_token_scores is on: the plain request is scored as before)
        assert outs[0].greedy_ids[0].tolist() == gold[0] and outs[2].greedy_ids[0].tolist() == gold[0][:1]
        assert outs[0].past_key_values.get_seq_length() == int(g["t0_cache_len"]) == outs[1].past_key_values.get_seq_length()
        assert not m._tickets and not m._forced_tickets
        assert m.batch_forced_stats() == {"jobs": 2, "rows_fed": len(gold[0]) - 1, "head_launches": 1}
    finally:
        m.set_token_scores(False)
