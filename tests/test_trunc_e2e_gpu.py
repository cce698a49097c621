"""Truncated sampling end to end (set_sampling_truncation / svln_sampling_truncation) on the GPU, TINY fixtures, a few turns.

(1) top_k = 1 (any T, any seed) and (8, 2^-20) keep one id, the best: the greedy fixtures' ids, hidden rows and cache lengths are
    reproduced (fp32 against the fixtures; fp32 and bf16 bit for bit against the engine's own greedy episode).  Fails without the feature.
(2) Off after on is bit-identical to a sampled engine that never had it on: ids and scores, decode graphs on and off.
(3) fp32 engine: every token equals the float64 restatement (tests/trunc_e2e.py) from the engine's OWN tap rows wherever the three gaps
    exceed the a-priori dot bound; at most 10 % of a setting's tokens are exempt (tests/test_trunc_inputs.py proves the oracle alone
    stays inside that on the fixtures).  Every score is within bound + 2e-5 of the float64 log-softmax over the kept set, wherever the
    two gaps that decide the kept SET are clear (elsewhere float64 itself cannot say which set the score is normalised over).
(4) generate, generate_batch at 8 (MFMA tiles) and 2 envs (batched GEMV), the staggered scheduler and sequence 0 of a group turn agree per
    env; seeds reproduce.
(5) With an allowed list of n <= 8 ids at (8, 1) the ids equal the untruncated allowed run's exactly.
(6) With set_top_logprobs(8) the lists are over the kept set, padded with (-1, -inf), and the emitted id's entry is the score's bits.
(7) Every row of tests/switches_ref.py's table switched on together with truncation (the stand-in for the pair-table row this attribute
    of svln_set_sampling cannot have); top_k = 1 makes the attribute visible: every score is exactly 0.
(8) Every row of the header's table: the refusals, cleared by svln_set_sampling(h, 0, ..), kept by svln_set_sampling(h, 1, ..), forced
    turns unchanged."""

import numpy as np
import pytest
import torch

import switch_probe as SP
import switches_ref as SW
import trunc_e2e as E
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from util import load_golden

pytestmark = pytest.mark.gpu
SHARE = {}


def _model(sc, dtype, envs=1, frames=None):
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=envs, max_frames=frames or 1 + (sc["num_history"] or 0), max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    apply_knobs(m, sc)
    return m


def _agent(m, sc, e=0, T=None, cls=StreamingAgent):
    enc = SyntheticPromptEncoder(sc["cfg"], seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
    return cls(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
               device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc),
               preprocess=m.get_vision_tower().image_processor.preprocess_array, do_sample=T is not None, temperature=T)


def _sample(m, T, seed, k=None, p=None):
    m.sampling_seed = seed
    m.set_sampling_truncation(k, p)              # held on the model ...
    m.set_sampling(T, seed)                      # ... and applied after the switch


def _episode(m, sc, steps, T=None, seed=0, k=None, p=None):
    """one env through `steps` env steps; T: sampled at that temperature with `seed` (the counters restart) under (k, p)"""
    m.reset(1)
    if T is not None:
        _sample(m, T, seed, k, p)
    ag = _agent(m, sc, 0, T)
    taps = []
    for step in range(steps):
        n0 = len(ag.turn_log)
        ag.act(synthetic_frame(0, step))
        if len(ag.turn_log) > n0:
            taps.append(dict(hidden=m.last_hidden(), cache_len=m.env_state(0)[1]))
    return ag.turn_log, taps


def _ids(log):
    return [r["out"].sequences[0].tolist() for r in log]


def _scores(log):
    return [r["out"].token_logprobs.cpu().numpy().view(np.uint32).tolist() for r in log]


# ------------------------------------------------------------------------------------------------------------ (1)
@pytest.mark.parametrize("k,p,T,seed", [(1, None, 1.0, 5), (1, 0.3, 0.7, 6), (8, 2.0 ** -20, 1.0, 7)])
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_one_kept_id_reproduces_the_greedy_fixtures(name, k, p, T, seed):
    sc, g = SCENARIOS[name], load_golden(name)
    m = _model(sc, torch.float32)
    assert m.sampling_truncation is None
    log, taps = _episode(m, sc, 16, T=T, seed=seed, k=k, p=p)
    assert m.sampling_truncation == (k, 1.0 if p is None else p) and m._sampling == (T, seed)
    assert len(log) >= 4
    for t, (r, tp) in enumerate(zip(log, taps)):
        assert r["out"].sequences[0].tolist() == g[f"t{t}_ids"].tolist(), (name, t)
        assert tp["cache_len"] == int(g[f"t{t}_cache_len"]), (name, t)
        hid = np.asarray(g[f"t{t}_hidden"])
        assert float(np.abs(tp["hidden"][:len(hid)] - hid).max()) <= 1e-3, (name, t)
    m.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_kept_id_is_the_engines_own_greedy_episode_bit_for_bit(dtype):
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, dtype)
    log0, taps0 = _episode(m, sc, 16)
    for (k, p, T) in ((1, None, 1.0), (8, 2.0 ** -20, 1.0)):
        log1, taps1 = _episode(m, sc, 16, T=T, seed=3, k=k, p=p)
        assert _ids(log1) == _ids(log0)
        for x, y in zip(taps0, taps1):
            assert np.array_equal(x["hidden"], y["hidden"]) and x["cache_len"] == y["cache_len"]
    # a greedy call afterwards needs no new step: set_sampling(off) clears the truncation in the engine, the pair stays on the model
    log2, _ = _episode(m, sc, 4)
    assert m._sampling is None and m.sampling_truncation == (8, 2.0 ** -20) and _ids(log2) == _ids(log0)[:len(log2)]
    m.close()


# ------------------------------------------------------------------------------------------------------------ (2)
@pytest.mark.parametrize("graph", [True, False], ids=["graphs", "launches"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_off_after_on_is_the_untouched_sampled_path(dtype, graph):
    sc, steps = SCENARIOS["tiny_episode"], 12
    ref = _model(sc, dtype)                                   # never on
    ref.set_decode_graph(graph)
    ref.set_token_scores(True)
    a, _ = _episode(ref, sc, steps, T=1.0, seed=11)
    ref.close()
    m = _model(sc, dtype)
    m.set_decode_graph(graph)
    m.set_token_scores(True)
    on1, _ = _episode(m, sc, steps, T=1.0, seed=11, k=4, p=0.9)
    on2, _ = _episode(m, sc, steps, T=1.0, seed=11, k=4, p=0.9)
    assert _ids(on1) == _ids(on2) and _scores(on1) == _scores(on2)            # reproducible, graphs replayed or not
    assert _ids(on1) != _ids(a)
    b, _ = _episode(m, sc, steps, T=1.0, seed=11)             # set_sampling_truncation(None, None): off
    assert m.sampling_truncation is None
    assert _ids(b) == _ids(a) and _scores(b) == _scores(a)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (3)
@pytest.mark.parametrize("setting", E.SETTINGS, ids=lambda s: f"k{s[0]}-p{s[1]}-T{s[2]}")
@pytest.mark.parametrize("name", E.FIXTURES)
def test_every_token_is_the_restated_truncated_sample_of_its_own_tap_row(name, setting):
    k, p, T, seeds = setting
    sc = SCENARIOS[name]
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    Wd, pen = torch.from_numpy(m.get_tensor("lm_head.weight")).double(), sc.get("rep_penalty", 1.0)
    stats = dict(tokens=0, under=0, score=0.0, scored=0)
    for seed in seeds:
        log, taps = _episode(m, sc, sc["steps"] if name == "tiny_episode" else 16, T=T, seed=seed, k=k, p=p)
        draw = 0
        for t, (r, tp) in enumerate(zip(log, taps)):
            ids, lp = r["out"].sequences[0].tolist(), r["out"].token_logprobs
            for j, tok in enumerate(ids[:len(tp["hidden"])]):
                want, cols, lps, dot, set_ok = E.restate_token(Wd, tp["hidden"][j], ids[:j], pen, k, p, T, seed, 0, draw + j, stats)
                if want is not None:
                    assert tok == want, (name, setting, seed, t, j, tok, want, cols)
                if set_ok:
                    assert tok in cols, (name, setting, seed, t, j, tok, cols)
                    err = abs(float(lp[0, j]) - float(lps[cols.index(tok)]))
                    stats["score"], stats["scored"] = max(stats["score"], err / (dot + E.LSE_TOL)), stats["scored"] + 1
                    assert err <= dot + E.LSE_TOL, (name, setting, seed, t, j, float(lp[0, j]), float(lps[cols.index(tok)]), dot)
            draw += len(ids)
    SHARE[(name,) + tuple(setting[:3])] = stats
    print(f"{name} {setting[:3]}: {stats['under']} of {stats['tokens']} tokens under the bound; worst |score - ref| / bound = {stats['score']:.3f}")
    assert stats["tokens"] >= 36 and stats["under"] <= 0.10 * stats["tokens"], stats
    m.close()


# ------------------------------------------------------------------------------------------------------------ (4)
TRUNC = (5, 0.5, 2.0)         # (top_k, top_p, T): the nucleus drops entries on every row (tests/trunc_e2e.py)


def _solo(m, sc, N, ticks, seed, lengths=None):
    k, p, T = TRUNC
    m.reset(N)
    _sample(m, T, seed, k, p)
    out = []
    for e in range(N):
        ag = _agent(m, sc, e, T)
        if lengths:
            ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
        for _ in range(ticks(e)):
            ag.act(synthetic_frame(e, ag.step_id))
        out.append(_ids(ag.turn_log))
    return out


@pytest.mark.parametrize("N,name", [(8, "tiny_episode"), (2, "tiny_penalty")])
def test_generate_batch_samples_what_generate_samples(N, name):
    sc, seed, steps = SCENARIOS[name], 2024, 16
    k, p, T = TRUNC
    m = _model(sc, torch.float32, envs=N, frames=3 * N)
    solo = _solo(m, sc, N, lambda e: steps, seed)
    assert _solo(m, sc, N, lambda e: steps, seed) == solo and _solo(m, sc, N, lambda e: steps, seed + 1) != solo       # seeds reproduce
    m.reset(N)
    _sample(m, T, seed, k, p)
    agents = [_agent(m, sc, e, T) for e in range(N)]
    group = BatchedAgents(agents)
    for step in range(steps):
        group.act([synthetic_frame(e, step) for e in range(N)])
    for e in range(N):
        assert _ids(agents[e].turn_log) == solo[e], (N, name, e)
    assert len({str(s) for s in solo}) == N
    # the untruncated episode of the same seed differs: the truncation was in force
    m.reset(N)
    _sample(m, T, seed)
    ag = _agent(m, sc, 0, T)
    for step in range(steps):
        ag.act(synthetic_frame(0, step))
    assert _ids(ag.turn_log) != solo[0]
    m.close()


def test_scheduler_samples_what_generate_samples():
    sc, N, seed = SCENARIOS["tiny_episode"], 4, 2025
    k, p, T = TRUNC
    m = _model(sc, torch.float32, envs=N, frames=3)
    lengths = lambda e, t: 2 if (e + t) % 2 == 0 else 4
    m.reset(N)
    _sample(m, T, seed, k, p)
    agents = [_agent(m, sc, e, T) for e in range(N)]
    for e, ag in enumerate(agents):
        ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
    group = AsyncBatchedAgents(agents)
    for tick in range(24):
        group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active={i for i in range(N) if tick >= i})
    assert group.stats["mixed_iterations"] >= 2, group.stats
    sched = [_ids(a.turn_log) for a in agents]
    m.cancel()
    steps_taken = [a.step_id for a in agents]
    solo = _solo(m, sc, N, lambda e: steps_taken[e], seed, lengths)
    for e in range(N):
        n = min(len(sched[e]), len(solo[e]))
        assert n >= 3 and sched[e][:n] == solo[e][:n], (e, sched[e], solo[e])
    m.close()


def test_sequence_0_of_a_group_turn_is_the_plain_truncated_turn():
    sc, seed = SCENARIOS["tiny_episode"], 99
    k, p, T = TRUNC
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    _sample(m, T, seed, k, p)
    ag = _agent(m, sc, 0, T)
    ag.observe(synthetic_frame(0, 0))
    req = ag._build_request("")
    plain = m.generate(**req)
    m.reset(1)
    _sample(m, T, seed, k, p)
    ag = _agent(m, sc, 0, T)
    ag.observe(synthetic_frame(0, 0))
    out = m.generate(**dict(ag._build_request(""), num_return_sequences=4))
    assert m.sampling_truncation == (k, p)
    n0 = int(out.sequence_lengths[0])
    assert out.sequences[0, :n0].tolist() == plain.sequences[0].tolist()
    assert np.abs(out.token_logprobs[0, :n0].cpu().numpy() - plain.token_logprobs[0].cpu().numpy()).max() <= 2 * E.LSE_TOL
    assert len({tuple(out.sequences[g, :int(out.sequence_lengths[g])].tolist()) for g in range(4)}) > 1
    m.select_sequence(0)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (5), (6)
def test_allowed_list_of_at_most_8_ids_at_8_1_is_the_untruncated_allowed_run():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.float32)
    base = sorted({i for r in _episode(m, sc, 4)[0] for i in r["out"].sequences[0].tolist()})
    allowed = sorted(set(base) | {1, 2, 3, 5})[:7]
    m.set_allowed_tokens(allowed, add_eos=False)
    m.set_token_scores(True)
    a, _ = _episode(m, sc, 12, T=1.0, seed=21)
    b, _ = _episode(m, sc, 12, T=1.0, seed=21, k=8, p=1.0)
    assert _ids(a) == _ids(b) and {i for s in _ids(b) for i in s} <= set(allowed)
    for x, y in zip(a, b):
        assert np.abs(x["out"].token_logprobs.cpu().numpy() - y["out"].token_logprobs.cpu().numpy()).max() <= 2 * E.LSE_TOL
        assert torch.equal(x["out"].allowed_logprobs, y["out"].allowed_logprobs)     # the rows stay the untruncated log-softmax over the list
    c, _ = _episode(m, sc, 12, T=1.0, seed=21, k=1)
    assert all(float(r["out"].token_logprobs.abs().max()) == 0.0 for r in c)
    m.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lists_are_over_the_kept_set(dtype):
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, dtype)
    m.set_token_scores(True)
    m.set_top_logprobs(8)
    log, _ = _episode(m, sc, 12, T=2.0, seed=31, k=4, p=0.64)
    kept_counts = set()
    for r in log:
        o = r["out"]
        ids, lps = o.top_token_ids[0].cpu().numpy(), o.top_logprobs[0].cpu().numpy()
        for j, tok in enumerate(o.sequences[0].tolist()):
            n = int((ids[j] >= 0).sum())
            kept_counts.add(n)
            assert 1 <= n <= 4 and bool((ids[j, n:] == -1).all()) and bool(np.isneginf(lps[j, n:]).all()) and bool(np.isfinite(lps[j, :n]).all())
            assert bool((np.diff(lps[j, :n]) <= 0).all())
            assert abs(float(np.exp(lps[j, :n].astype(np.float64)).sum()) - 1.0) <= 1e-4            # a distribution over the kept set
            assert tok in ids[j, :n].tolist()
            q = ids[j].tolist().index(tok)
            assert lps[j, q:q + 1].view(np.uint32).tolist() == o.token_logprobs[0, j:j + 1].cpu().numpy().view(np.uint32).tolist()
    assert kept_counts & {2, 3}, kept_counts                   # the nucleus dropped entries
    m.close()


# ------------------------------------------------------------------------------------------------------------ (7)
@pytest.mark.parametrize("row", SW.ROWS, ids=lambda r: r.name)
def test_every_switch_row_with_truncation_on(row):
    m = SP.make_model()                                     # the pair test's own engine: bf16, 4 envs, the probe's sampling seed
    T, seed = SW.SAMPLING
    ag = SP._agent(m, 0, sampled=True)
    ag.observe(synthetic_frame(0, 0))
    req = ag._build_request("")
    if row.name in SW.PLAIN_HEAD:
        # unreachable together: sampling refuses the row both ways, and truncation needs sampling
        row.on(m)
        m.set_sampling_truncation(4, 0.9)                   # sampling is off: held on the model only
        with pytest.raises(_lib.SvlnError, match=row.c_name):
            m.set_sampling(T, seed)
        assert m._lib.svln_sampling_truncation(m._h, 4, 0.9) != 0 and b"svln_set_sampling" in m._lib.svln_last_error()
        row.off(m)
        m.set_sampling(T, seed)
        with pytest.raises(_lib.SvlnError, match="svln_set_sampling"):
            row.on(m)
    elif row.name == "sampling":
        m.set_token_scores(True)
        m.set_sampling_truncation(1)
        row.on(m)                                           # Python's set_sampling applies the pair the model holds
        assert m.sampling_truncation == (1, 1.0) and m._sampling == SW.SAMPLING
        _lib.check(m._lib.svln_set_sampling(m._h, 1, T, seed))             # the C switch, on again: the truncation is kept
        assert float(m.generate(**req).token_logprobs.abs().max()) == 0.0
        m.set_sampling_truncation()                         # while sampling is on: off at once
        assert m.sampling_truncation is None and m._sampling == SW.SAMPLING
        m.reset(SP.N_ENVS)
        assert float(m.generate(**req).token_logprobs.abs().max()) > 0.0
        m.set_sampling_truncation(1)                        # ... and on at once
        m.reset(SP.N_ENVS)
        assert float(m.generate(**req).token_logprobs.abs().max()) == 0.0
        row.off(m)                                          # cleared: a greedy call works, and the C switch on again starts untruncated
        m.reset(SP.N_ENVS)
        g = m.generate(**dict(req, do_sample=False))
        _lib.check(m._lib.svln_set_sampling(m._h, 1, T, seed))
        m.sampling_truncation = None
        m._sampling = SW.SAMPLING
        m.reset(SP.N_ENVS)
        assert g.sequences.shape[1] >= 1 and float(m.generate(**req).token_logprobs.abs().max()) > 0.0
    elif row.name == "generate_group":
        m.set_sampling_truncation(4, 0.9)
        m.set_sampling(T, seed)
        out = m.generate(**dict(req, num_return_sequences=2))
        assert out.sequences.shape[0] == 2 and m.sampling_truncation == (4, 0.9)
        with pytest.raises(_lib.SvlnError, match="group"):  # a group pending
            m.set_sampling_truncation(2)
        assert m.sampling_truncation == (4, 0.9)
        m.select_sequence(0)
        _lib.check(m._lib.svln_sampling_truncation(m._h, 2, 1.0))
    elif row.name == "generate_forced":
        m.set_token_scores(True)
        m.set_sampling(T, seed)
        f0 = m.generate(**req, forced_ids=list(SW.FORCED_IDS))
        m.reset(SP.N_ENVS)
        m.set_sampling_truncation(2, 0.5)
        m.set_sampling(T, seed)
        f1 = m.generate(**req, forced_ids=list(SW.FORCED_IDS))
        assert f1.sequences[0].tolist() == list(SW.FORCED_IDS) and torch.equal(f0.token_logprobs, f1.token_logprobs)      # untruncated softmax(x / T)
    else:
        # composes: both stay in force -- the row switches on in either order and top_k = 1 shows in every score
        row.on(m)
        m.set_token_scores(True)
        m.set_sampling_truncation(1)
        m.set_sampling(T, seed)
        if row.name != "token_scores":
            row.off(m)
            row.on(m)
        o = m.generate(**req)
        assert o.sequences.shape[1] >= 1 and float(o.token_logprobs.abs().max()) == 0.0, row.name
        assert m.sampling_truncation == (1, 1.0) and m._sampling == SW.SAMPLING
        if row.name == "allowed_tokens":
            assert set(o.sequences.reshape(-1).tolist()) <= set(SW.ALLOWED_IDS)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (8)
def test_refusals_and_what_clears_and_keeps_it():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.float32, envs=2, frames=6)
    m.sampling_seed = 3
    L, h = m._lib, m._h

    def refused(k, p, word):
        assert L.svln_sampling_truncation(h, k, p) != 0, (k, p)
        assert word in L.svln_last_error(), (k, p, L.svln_last_error())

    # sampling off: the off setting changes nothing and succeeds, anything else names svln_set_sampling
    assert L.svln_sampling_truncation(h, 0, 1.0) == 0
    refused(4, 1.0, b"svln_set_sampling")
    with pytest.raises(ValueError, match="top_k"):
        m.set_sampling_truncation(top_p=0.9)
    for bad in ((9, None), (-1, None), (4, 0.0), (4, float("nan"))):
        with pytest.raises(ValueError):
            m.set_sampling_truncation(*bad)
    assert m._sampling is None and m.sampling_truncation is None
    m.set_token_scores(True)
    m.set_sampling(1.0, 3)
    for k in (-1, 9, 100):
        refused(k, 1.0, b"top_k")
    for p in (0.0, -0.5, 1.0001, float("nan"), float("inf")):
        refused(4, p, b"top_p")
    refused(0, 0.9, b"top_k")
    ag = _agent(m, sc, 0, 1.0)
    ag.observe(synthetic_frame(0, 0))
    req = ag._build_request("")
    base = m.generate(**req)                                # the refused calls changed nothing: still the untruncated sample
    assert float(base.token_logprobs.abs().max()) > 0.0
    _lib.check(L.svln_sampling_truncation(h, 1, 1.0))
    m.reset(2)
    assert float(m.generate(**req).token_logprobs.abs().max()) == 0.0
    _lib.check(L.svln_set_sampling(h, 1, 1.0, 3))           # kept by an "on" call
    m.reset(2)
    assert float(m.generate(**req).token_logprobs.abs().max()) == 0.0
    _lib.check(L.svln_set_sampling(h, 0, 1.0, 0))           # cleared by "off" ...
    _lib.check(L.svln_set_sampling(h, 1, 1.0, 3))
    m.reset(2)
    again = m.generate(**req)                               # ... so the next sampled turn is the untruncated one, draw for draw
    assert again.sequences.tolist() == base.sequences.tolist() and torch.equal(again.token_logprobs, base.token_logprobs)
    # in flight
    agents = [_agent(m, sc, e, 1.0) for e in range(2)]
    for e, a in enumerate(agents):
        a.observe(synthetic_frame(e, 0))
    m.reset(2)
    m.submit(**agents[0]._build_request(""))
    refused(4, 0.9, b"in flight")
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_sampling_truncation(4, 0.9)
    assert m.sampling_truncation is None
    m.cancel()
    _lib.check(L.svln_sampling_truncation(h, 4, 0.9))
    # the per-call keys stay refused
    m.reset(2)
    for kw, key in ((dict(top_k=5), "top_k"), (dict(top_p=0.9), "top_p")):
        with pytest.raises(NotImplementedError, match=key):
            m.generate(**dict(req, **kw))
    # the automatic flip of do_sample=True applies the pair the model holds
    m.set_sampling(None)
    m.sampling_truncation = (1, 1.0)
    m.sampling_seed = 3
    out = m.generate(**dict(req, temperature=1.0))
    assert m._sampling == (1.0, 3) and float(out.token_logprobs.abs().max()) == 0.0
    m.close()


def test_zz_share_report():
    for key, st in sorted(SHARE.items()):
        print(f"{key}: {st['under']} of {st['tokens']} tokens under the bound ({100.0 * st['under'] / max(st['tokens'], 1):.1f} %), "
              f"{st['scored']} scores checked, worst |score - ref| / bound {st['score']:.3f}")
