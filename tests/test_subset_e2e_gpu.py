"""Allowed-token decode end to end (set_allowed_tokens / svln_set_allowed_tokens) on the GPU, on the committed fixtures.

(1) Containment, fp32 engine: with A = every id the fixture emits, ids, hidden rows (<= 1e-3) and cache lengths are the fixture's -- a
    restricted arg-max equals the unrestricted one when the winner is allowed -- and off after on is bit-identical to the run before the
    switch was ever on.  true4_episode: one turn at the full vocabulary (152 064 rows, hidden 3584).
(2) Exclusion: with one emitted id removed from A, every token equals the float64 restatement argmax_{a in A} lm_head[a] . h from the
    engine's OWN tap row h, the first one that differs from the fixture included.  Every compared token's margin exceeds the a-priori dot
    bound 2 gamma_K max_a sum_k |w_ak h_k| (gamma_K = K 2^-24) of tests/test_scores_e2e_gpu.py (tests/test_subset_inputs.py proves it from
    the fixtures up to the first difference); every score and every allowed_logprobs row lies inside that file's bound,
    2 gamma_K max_a sum_k |w_ak h_k| + 2e-5.
(3) generate, generate_batch at 8 and 2 envs and the staggered scheduler agree per env (fp32: identical ids; bf16: the bounds of
    test_batched_lockstep_envs_equal_solo_runs).
(4) Sampling: seeds reproduce, T = 2^-14 reproduces the restricted greedy run, at T = 1 tokens equal the restatement wherever the
    perturbed margin exceeds the bound.
(5) Composition, bf16: rides with right and wrong drafts (counters of prefill_draft_ref.simulate), set_speculative(2), set_fp8_decode,
    set_mxfp4_batched.
(6) Refusals of svln_set_allowed_tokens and the getters' failure modes."""
import ctypes as C

import numpy as np
import pytest
import torch

import prefill_draft_ref as PR
import sample_ref as SR
import subset_ref as R
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from util import load_golden

pytestmark = pytest.mark.gpu
LSE_TOL = 2e-5
HIDDEN_TOL = 1e-3
REMOVED, PATHS_A, fixture_ids, allowed_set, restricted_rows = R.REMOVED, R.PATHS_A, R.fixture_ids, R.allowed_set, R.restricted_rows


def _model(sc, dtype, envs=1, frames=None):
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=envs, max_frames=frames or 1 + (sc["num_history"] or 0), max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    apply_knobs(m, sc)
    return m


def _episode(m, sc, steps=None, model=None):
    taps = []

    def on_turn(t, rec):
        ne, kl = m.env_state(0)
        taps.append(dict(hidden=m.last_hidden(), cache_len=kl, n_embeds=ne))
    log = run_scenario(model or m, sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda", steps=steps)
    return log, taps


def _ids(log):
    return [r["out"].sequences[0].tolist() for r in log]


def _head(m):
    return torch.from_numpy(m.get_tensor("lm_head.weight")).double()


def check_turn(Wd, A, out, hidden, penalty=1.0, strict=True, stats=None, what=""):
    """greedy turn against the float64 restatement over A: tokens (strict: every margin must exceed the bound), scores and allowed_logprobs"""
    ids = out.sequences[0].tolist()
    A = list(A)
    lp, alp = out.get("token_logprobs"), out.get("allowed_logprobs")
    if alp is not None:
        assert alp.dtype == torch.float32 and tuple(alp.shape) == (1, len(ids), len(A)) and alp.device == out.sequences.device, (what, alp.shape)
        assert out.allowed_token_ids.dtype == torch.int64 and out.allowed_token_ids.tolist() == A
    for k, (y, dot) in enumerate(restricted_rows(Wd, A, hidden, ids, penalty)):
        assert ids[k] in A, (what, k, ids[k])
        top = np.sort(y)[::-1]
        margin = float(top[0] - top[1]) if len(A) > 1 else float("inf")
        if stats is not None:
            stats["tokens"] = stats.get("tokens", 0) + 1
            stats["min_margin_over_bound"] = min(stats.get("min_margin_over_bound", float("inf")), margin / dot)
        if strict:
            assert margin > dot, (what, k, "margin under the a-priori bound", margin, dot)
        if margin > dot:
            assert ids[k] == A[int(np.argmax(y))], (what, k, ids[k], A[int(np.argmax(y))], margin, dot)
        ref = y - (y.max() + np.log(np.exp(y - y.max()).sum()))
        if lp is not None:
            assert abs(float(lp[0, k]) - ref[A.index(ids[k])]) <= dot + LSE_TOL, (what, k, float(lp[0, k]), ref[A.index(ids[k])], dot)
        if alp is not None:
            err = float(np.abs(alp[0, k].cpu().numpy().astype(np.float64) - ref).max())
            assert err <= dot + LSE_TOL, (what, k, err, dot)
            assert abs(float(alp[0, k, A.index(ids[k])]) - float(lp[0, k])) <= 2 * LSE_TOL


# ------------------------------------------------------------------------------------------------------------ (1) containment
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_containment_equals_the_fixture_and_off_after_on_is_untouched(name):
    sc, g = SCENARIOS[name], load_golden(name)
    A = allowed_set(name)
    m = _model(sc, torch.float32)
    log0, taps0 = _episode(m, sc)                             # the switch has never been on
    assert _ids(log0) == fixture_ids(name) and m.allowed_token_ids is None
    m.set_token_scores(True)
    m.set_allowed_tokens(A, add_eos=False)
    assert m.allowed_token_ids == tuple(A)
    m.reset(1)
    log1, taps1 = _episode(m, sc)
    Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
    assert _ids(log1) == fixture_ids(name)
    for t, (r, tp) in enumerate(zip(log1, taps1)):
        n = len(r["out"].sequences[0])
        assert np.abs(tp["hidden"][:n] - g[f"t{t}_hidden"][:n]).max() <= HIDDEN_TOL and tp["cache_len"] == int(g[f"t{t}_cache_len"]), t
        assert np.array_equal(tp["hidden"], taps0[t]["hidden"])           # the layers never see the switch
        check_turn(Wd, A, r["out"], tp["hidden"], pen, strict=False, what=(name, t))
    m.set_allowed_tokens(None)
    m.set_token_scores(False)
    assert m.allowed_token_ids is None
    m.reset(1)
    log2, taps2 = _episode(m, sc)
    assert _ids(log2) == _ids(log0) and all("allowed_logprobs" not in r["out"] and "token_logprobs" not in r["out"] for r in log2)
    for a, b in zip(taps0, taps2):
        assert np.array_equal(a["hidden"], b["hidden"]) and a["cache_len"] == b["cache_len"]
    m.close()


def test_containment_one_turn_at_the_full_vocabulary():
    sc, g = SCENARIOS["true4_episode"], load_golden("true4_episode")
    A = sorted(set(g["t0_ids"].tolist()))
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    m.set_allowed_tokens(A, add_eos=False)
    log, taps = _episode(m, sc, steps=1)
    ids = _ids(log)[0]
    assert len(log) == 1 and ids == g["t0_ids"].tolist() and taps[0]["cache_len"] == int(g["t0_cache_len"])
    assert np.abs(taps[0]["hidden"][:len(ids)] - g["t0_hidden"][:len(ids)]).max() <= HIDDEN_TOL
    check_turn(_head(m), A, log[0]["out"], taps[0]["hidden"], strict=False, what="true4")
    m.close()


# ------------------------------------------------------------------------------------------------------------ (2) exclusion
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_exclusion_equals_the_restatement_from_the_engines_own_rows(name):
    sc = SCENARIOS[name]
    A = [a for a in allowed_set(name) if a != REMOVED[name]]
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    m.set_allowed_tokens(A, add_eos=False)
    log, taps = _episode(m, sc)
    Wd, stats = _head(m), {}
    got, fix = _ids(log), fixture_ids(name)
    assert got != fix[:len(got)] and all(REMOVED[name] not in t for t in got)
    first = next(t for t, ids in enumerate(got) if ids != fix[t])
    assert REMOVED[name] in fix[first]                       # the first difference is where the fixture emits the removed id
    for t, (r, tp) in enumerate(zip(log, taps)):
        check_turn(Wd, A, r["out"], tp["hidden"], sc.get("rep_penalty", 1.0), strict=True, stats=stats, what=(name, t))
    print(f"{name}: {stats}")
    m.close()


# ------------------------------------------------------------------------------------------------------------ (3) paths agree
def _agent(m, sc, e, T=None, fixed=False):
    """fixed: every turn yields four actions whatever its ids say, so that every path runs the same turns at the same env steps"""
    enc = SyntheticPromptEncoder(sc["cfg"], seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
    ag = StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                          device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc),
                          preprocess=m.get_vision_tower().image_processor.preprocess_array, do_sample=T is not None, temperature=T)
    if fixed:
        ag.decode_actions = lambda ids: [1] * 4
    return ag


def _solo(m, sc, e, steps, T=None, fixed=False):
    ag, hid = _agent(m, sc, e, T, fixed), []
    for s in range(steps):
        n0 = len(ag.turn_log)
        ag.act(synthetic_frame(e, s))
        if len(ag.turn_log) > n0:
            hid.append(m.last_hidden())
    return ag, hid


def _lockstep(m, sc, N, steps, fixed=False):
    m.reset(N)
    agents = [_agent(m, sc, e, fixed=fixed) for e in range(N)]
    group = BatchedAgents(agents)
    hid = [[] for _ in range(N)]
    for s in range(steps):
        n0 = len(agents[0].turn_log)
        group.act([synthetic_frame(e, s) for e in range(N)])
        if len(agents[0].turn_log) > n0:
            for e in range(N):
                hid[e].append(m.last_hidden_batch(e))
    return agents, hid


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_paths_agree_per_env(dtype):
    sc, steps, N = SCENARIOS["tiny_episode"], 16, 8
    A = list(PATHS_A)
    m = _model(sc, dtype, envs=N, frames=3 * N)
    m.set_token_scores(True)
    m.set_allowed_tokens(A, add_eos=False)
    solo = []
    for e in range(N):
        m.reset(N)
        solo.append(_solo(m, sc, e, steps, fixed=True))
    runs = {"batch8": _lockstep(m, sc, 8, steps, fixed=True), "batch2": _lockstep(m, sc, 2, steps, fixed=True)}
    # the staggered scheduler: env i joins at tick i
    m.reset(4)
    agents = [_agent(m, sc, e, fixed=True) for e in range(4)]
    hid = [[] for _ in range(4)]
    group = AsyncBatchedAgents(agents, on_result=lambda i, ticket, out: hid[i].append(m.last_hidden_batch(ticket.slot)))
    tick = 0
    while any(ag.step_id < steps for ag in agents):
        assert tick < 50 * steps
        act = {i for i in range(4) if tick >= i and agents[i].step_id < steps}
        group.tick([synthetic_frame(i, agents[i].step_id) for i in range(4)], active=act)
        tick += 1
    assert group.stats["mixed_iterations"] >= 1, group.stats
    runs["scheduler"] = (agents, hid)
    Wd = _head(m)
    agree = total = 0
    for path, (ags, hids) in runs.items():
        for e, ag in enumerate(ags):
            ref_ag, ref_hid = solo[e]
            got, want = _ids(ag.turn_log), _ids(ref_ag.turn_log)
            assert len(got) == len(want) == 4, (path, e, len(got), len(want))
            for t, r in enumerate(ag.turn_log):
                assert set(got[t]) <= set(A) and r["out"].allowed_logprobs.shape == (1, len(got[t]), len(A))
                if dtype == torch.float32:
                    assert got[t] == want[t], (path, e, t, got[t], want[t])
                    assert np.abs(hids[e][t][:len(got[t])] - ref_hid[t][:len(got[t])]).max() <= HIDDEN_TOL
                    check_turn(Wd, A, r["out"], hids[e][t], strict=False, what=(path, e, t))
                else:
                    total += 1
                    agree += int(got[t][0] == want[t][0])
                    rel = np.linalg.norm(hids[e][t][0] - ref_hid[t][0]) / np.linalg.norm(ref_hid[t][0])
                    assert rel < 3e-2, (path, e, t, rel)
            assert ag.last_allowed_logprobs is not None and torch.equal(ag.last_allowed_logprobs, ag.turn_log[-1]["out"].allowed_logprobs)
    assert dtype == torch.float32 or agree >= total - 2, (agree, total)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (4) sampling
def _sampled(m, sc, steps, T, seed):
    m.reset(1)
    m.sampling_seed = seed
    m.set_sampling(T, seed)
    return _solo(m, sc, 0, steps, T)


def test_sampling_over_the_allowed_set():
    sc, steps = SCENARIOS["tiny_episode"], 16
    A = list(PATHS_A)
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    m.set_allowed_tokens(A, add_eos=False)
    greedy, _ = _solo(m, sc, 0, steps)
    a, hid_a = _sampled(m, sc, steps, 1.0, 11)
    b, _ = _sampled(m, sc, steps, 1.0, 11)
    c, _ = _sampled(m, sc, steps, 1.0, 12)
    assert _ids(a.turn_log) == _ids(b.turn_log) and _ids(a.turn_log) != _ids(c.turn_log)
    assert all(torch.equal(p["out"].allowed_logprobs, q["out"].allowed_logprobs) for p, q in zip(a.turn_log, b.turn_log))
    cold, _ = _sampled(m, sc, steps, 2.0 ** -14, 5)
    assert _ids(cold.turn_log) == _ids(greedy.turn_log)
    # T = 1: the full-vocabulary sampled turn conditioned on A -- noise column = the vocabulary id, stream = env slot 0, draw = tokens so far
    Wd, draw, under, total = _head(m), 0, 0, 0
    for t, r in enumerate(a.turn_log):
        ids = r["out"].sequences[0].tolist()
        for k, (y, dot) in enumerate(restricted_rows(Wd, A, hid_a[t], ids)):
            g = SR.gumbel(11, 0, draw + k, np.array(A))
            z = np.sort(y + g)[::-1]
            tol = 2.0 ** -17 * max(1.0, float(np.abs(g).max())) + 2.0 ** -22 * float(np.abs(y + g).max())
            total += 1
            if z[0] - z[1] > dot + tol:
                assert ids[k] == A[int(np.argmax(y + g))], (t, k, ids[k], float(z[0] - z[1]))
            else:
                under += 1
            ref = y - (y.max() + np.log(np.exp(y - y.max()).sum()))
            assert float(np.abs(r["out"].allowed_logprobs[0, k].cpu().numpy() - ref).max()) <= dot + LSE_TOL
            assert abs(float(r["out"].token_logprobs[0, k]) - ref[A.index(ids[k])]) <= dot + LSE_TOL
        draw += len(ids)
    assert under <= total // 4, (under, total)
    m.set_sampling(None)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (5) composition, bf16
class _Drafted:
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


def test_composition_with_drafts_and_reduced_precision_modes():
    sc, steps = SCENARIOS["tiny_episode"], 16
    A = list(PATHS_A)
    m = _model(sc, torch.bfloat16, envs=2, frames=6)
    m.set_allowed_tokens(A, add_eos=False)
    base, _ = _episode(m, sc, steps)
    want = _ids(base)
    assert all(set(t) <= set(A) for t in want) and len(want) >= 3
    Wd = _head(m)

    def drafts(t):                                            # right, wrong from id 1 on, wrong at once, none
        d = list(want[t]) if t < len(want) else [A[0]]
        other = lambda tok: next(a for a in A if a != tok and a not in eos_ids(sc))
        return [d, d[:1] + [other(x) for x in d[1:]] + [A[0]], [other(d[0])] + d[1:], None][t % 4]

    for ride, rows in ((True, 0), (True, 2), (False, 2)):
        m.set_prefill_draft(ride)
        m.set_speculative(rows)
        m.prefill_draft_stats(reset=True), m.draft_stats(reset=True)
        m.reset(1)
        per_turn = []

        def on_turn(t, rec):
            per_turn.append((rec["out"].sequences[0].tolist(), m.env_state(0)[0], m.prefill_draft_stats(reset=True) + m.draft_stats(reset=True)))
        run_scenario(_Drafted(m, drafts), sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda",
                     steps=steps)
        assert len(per_turn) == len(want)
        for t, (ids, n_embeds, stats) in enumerate(per_turn):
            assert set(ids) <= set(A), (ride, rows, t, ids)
            d = drafts(t)
            sim_ids, sim_stats = PR.simulate(ids, [] if d is None else d, sc["max_new"], eos_ids(sc), 2048 - n_embeds, rows, sc["cfg"].vocab) \
                if ride else (ids, None)
            assert sim_ids == ids and (sim_stats is None or stats == sim_stats), (ride, rows, t, stats, sim_stats)
        assert sum(s[2][0] for s in per_turn) >= (2 if ride else 0)
    m.set_prefill_draft(False)
    m.set_speculative(0)
    # the reduced-precision modes: the head stays the bf16 lm_head over A, so every token is the restatement's where the margin allows
    m.set_fp8_decode(True)
    m.reset(1)
    log, taps = _episode(m, sc, steps)
    for t, (r, tp) in enumerate(zip(log, taps)):
        check_turn(Wd, A, r["out"], tp["hidden"], strict=False, what=("fp8_decode", t))
    m.set_fp8_decode(False)
    m.set_mxfp4_batched(True)
    agents, hid = _lockstep(m, sc, 2, steps)
    for e, ag in enumerate(agents):
        assert len(ag.turn_log) >= 3
        for t, r in enumerate(ag.turn_log):
            check_turn(Wd, A, r["out"], hid[e][t], strict=False, what=("mxfp4_batched", e, t))
    m.set_mxfp4_batched(False)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (6) refusals, getters
def test_refusals_and_getters():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16, envs=2, frames=6)
    L, V = m._lib, sc["cfg"].vocab
    P64 = C.POINTER(C.c_int64)

    def raw(ids, n=None):
        arr = None if ids is None else np.asarray(ids, dtype=np.int64)
        return L.svln_set_allowed_tokens(m._h, None if arr is None else arr.ctypes.data_as(P64), len(ids) if n is None else n)

    assert raw(list(range(257))) != 0 and b"256" in L.svln_last_error()
    assert raw([1, V]) != 0 and b"vocabulary" in L.svln_last_error()
    assert raw([-1, 3]) != 0 and b"vocabulary" in L.svln_last_error()
    assert raw([3, 3]) != 0 and b"ascending" in L.svln_last_error()
    assert raw([5, 3]) != 0 and b"ascending" in L.svln_last_error()
    assert raw(None, 3) != 0 and b"null" in L.svln_last_error()
    assert raw([1], -1) != 0
    assert raw([1, 2, 3]) == 0 and raw([1, 2, 3]) == 0 and raw(None, 0) == 0 and raw(None, 0) == 0
    # the Python method: sorted, de-duplicated, EOS added by default (the generation config's ids inside the vocabulary)
    m.generation_config.eos_token_id = [7, 151645]
    m.set_allowed_tokens([9, 3, 9, 5])
    assert m.allowed_token_ids == (3, 5, 7, 9)
    m.set_allowed_tokens([9, 3], add_eos=False)
    assert m.allowed_token_ids == (3, 9)
    m.set_allowed_tokens([])
    assert m.allowed_token_ids is None
    with pytest.raises(_lib.SvlnError, match="vocabulary"):
        m.set_allowed_tokens([V + 1])
    assert m.allowed_token_ids is None
    # getters: off for that turn -> refused by name
    buf, nt, ni = (C.c_float * 4096)(), C.c_int32(), C.c_int32()
    agents = [_agent(m, sc, e) for e in range(2)]
    agents[0].act(synthetic_frame(0, 0))
    assert agents[0].last_allowed_logprobs is None
    assert L.svln_get_allowed_logprobs(m._h, buf, 4096, C.byref(nt), C.byref(ni)) != 0 and b"svln_set_allowed_tokens" in L.svln_last_error()
    m.set_allowed_tokens(list(PATHS_A), add_eos=False)       # the list alone: still no distribution
    m.reset(2)
    agents = [_agent(m, sc, e) for e in range(2)]
    agents[0].act(synthetic_frame(0, 0))
    assert "allowed_logprobs" not in agents[0].turn_log[-1]["out"] and set(_ids(agents[0].turn_log)[0]) <= set(PATHS_A)
    assert L.svln_get_allowed_logprobs(m._h, buf, 4096, C.byref(nt), C.byref(ni)) != 0
    m.set_token_scores(True)
    m.reset(2)
    agents = [_agent(m, sc, e) for e in range(2)]
    agents[0].act(synthetic_frame(0, 0))
    out = agents[0].turn_log[-1]["out"]
    assert L.svln_get_allowed_logprobs(m._h, buf, 4096, C.byref(nt), C.byref(ni)) == 0
    assert (nt.value, ni.value) == (out.sequences.shape[1], len(PATHS_A))
    assert [buf[k] for k in range(nt.value * ni.value)] == out.allowed_logprobs.flatten().tolist()
    assert L.svln_get_allowed_logprobs(m._h, None, 0, C.byref(nt), C.byref(ni)) != 0
    assert agents[0].last_allowed_logprobs is not None
    agents[0].reset_memory()
    assert agents[0].last_allowed_logprobs is None
    # no change while scheduler turns are in flight, not even to the same list; the slot getter's lifetime
    agents[1].observe(synthetic_frame(1, 0))
    ticket = m.submit(**agents[1]._build_request(""))
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_allowed_tokens(None)
    assert raw(list(PATHS_A)) != 0 and b"in flight" in L.svln_last_error()
    assert L.svln_batch_allowed_logprobs(m._h, ticket.slot, buf, 4096, C.byref(nt), C.byref(ni)) != 0          # not finished yet
    fin, _ = m.step_batch()
    while not fin:
        fin, _ = m.step_batch()
    assert fin[0][1].allowed_logprobs.shape == (1, fin[0][1].sequences.shape[1], len(PATHS_A))
    assert L.svln_batch_allowed_logprobs(m._h, ticket.slot, buf, 4096, C.byref(nt), C.byref(ni)) != 0          # svln_batch_result freed the slot
    assert L.svln_generate_batch_allowed_logprobs(m._h, 0, buf, 4096, C.byref(nt), C.byref(ni)) != 0           # no svln_generate_batch has run
    m.close()
