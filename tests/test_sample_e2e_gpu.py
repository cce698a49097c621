"""Temperature sampling end to end (set_sampling / svln_set_sampling, generate(do_sample=True)) on the GPU, TINY fixtures, a few turns.

(1) Off after on: ids, hidden rows and cache lengths are bit-identical to an engine that never had the switch on (fp32 and bf16).
(2) The same seed twice gives the same ids; another seed gives another episode.
(3) fp32 engine at T = 2^-14: the greedy fixtures' ids are reproduced (tests/test_sample_inputs.py asserts that the recorded margins,
    scaled by 2^14, exceed the largest noise gap).
(4) fp32 engine at T = 1: every emitted token equals argmax(float64(lm_head . h) / T + G64) computed from the engine's OWN tap row h,
    wherever the restated top-2 margin of the perturbed values exceeds  2 * (2 gamma_K max_n sum_k |w_nk h_k|) / T + tol_G  -- the a-priori
    dot bound of tests/test_scores_e2e_gpu.py on both candidates plus the noise tolerance of tests/sample_ref.py.  At most 5 % of the
    tokens may fall under it (asserted).  With set_token_scores on, every score lies within that file's bound (scaled by 1 / T) of float64
    log_softmax(l / T)[token].
(5) generate, generate_batch (8 envs: the MFMA head; 2 envs: the batched GEMV) and the staggered scheduler with the same seed on the fp32
    engine emit identical ids per env: the noise depends on (seed, env slot, draw, column) alone.
(6) The repetition penalty (tiny_penalty), the bf16 engine, the e4m3 / MXFP4 heads; the refusal matrix in both orders, the in-flight
    refusal, svln_get_top2, the do_sample kwargs and the agents."""
import ctypes as C

import numpy as np
import pytest
import torch

import mxfp4_ref as MX
import sample_ref as R
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from util import load_golden

pytestmark = pytest.mark.gpu
LSE_TOL = 2e-5
SHARE = {}


def _model(sc, dtype, envs=1, frames=None):
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=envs, max_frames=frames or 1 + (sc["num_history"] or 0), max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    apply_knobs(m, sc)
    return m


def _agent(m, sc, e=0, T=None):
    enc = SyntheticPromptEncoder(sc["cfg"], seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
    return StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                          device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc),
                          preprocess=m.get_vision_tower().image_processor.preprocess_array, do_sample=T is not None, temperature=T)


def _episode(m, sc, steps, T=None, seed=0):
    """one env through `steps` env steps; T: sampled at that temperature with `seed` (the counters restart), None: the greedy call"""
    m.reset(1)
    if T is not None:
        m.sampling_seed = seed
        m.set_sampling(T, seed)
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


def _head(m, mode=None):
    w = torch.from_numpy(m.get_tensor("lm_head.weight")).float()
    if mode == "fp8":
        w = O.qdq_e4m3_rows(w)
    elif mode == "mxfp4":
        w = MX.qdq_mxfp4(w).float()
    return w.double()


def _check_turn(Wd, out, hidden, T, seed, stream, draw0, penalty, stats, what):
    """tokens (where the margin allows) and scores (when present) of one sampled turn against float64 from the tap rows"""
    ids = out.sequences[0].tolist()
    K, V = Wd.shape[1], Wd.shape[0]
    gamma, inv_t = K * 2.0 ** -24, float(np.float32(1.0) / np.float32(T))
    lp = out.get("token_logprobs")
    for k, tok in enumerate(ids[:len(hidden)]):
        h = torch.from_numpy(np.asarray(hidden[k], dtype=np.float64))
        l = Wd @ h
        if penalty != 1.0 and k:
            seen = torch.tensor(sorted(set(ids[:k])), dtype=torch.long)
            l[seen] = torch.where(l[seen] < 0, l[seen] * penalty, l[seen] / penalty)
        y = l.numpy() * inv_t
        dot = 2 * gamma * float((Wd.abs() @ h.abs()).max()) * inv_t
        g = R.gumbel(seed, stream, draw0 + k, np.arange(V))
        z = y + g
        a = int(np.argmax(z))
        zb = np.delete(z, a)
        b = int(np.argmax(zb))
        tol = 2.0 ** -17 * max(1.0, abs(g[a]), abs(np.delete(g, a)[b])) + 2.0 ** -22 * float(np.abs(z).max())
        stats["tokens"] += 1
        if z[a] - zb[b] > 2 * dot + tol:
            assert tok == a, (what, k, tok, a, float(z[a] - zb[b]), dot, tol)
        else:
            stats["under"] += 1
        if lp is not None:
            ref = float(y[tok] - (y.max() + np.log(np.exp(y - y.max()).sum())))
            err = abs(float(lp[0, k]) - ref)
            stats["score"] = max(stats["score"], err / (dot + LSE_TOL))
            assert err <= dot + LSE_TOL, (what, k, float(lp[0, k]), ref, dot)
    return len(ids)


# ------------------------------------------------------------------------------------------------------------ single env
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_off_after_on_is_the_untouched_greedy_path_and_seeds_reproduce(dtype):
    sc, steps = SCENARIOS["tiny_episode"], 16
    ref = _model(sc, dtype)                                   # never on
    log0, taps0 = _episode(ref, sc, steps)
    ref.close()
    m = _model(sc, dtype)
    m.set_token_scores(True)
    a, _ = _episode(m, sc, steps, T=1.0, seed=11)
    b, _ = _episode(m, sc, steps, T=1.0, seed=11)
    c, _ = _episode(m, sc, steps, T=1.0, seed=12)
    assert _ids(a) == _ids(b) and _ids(a) != _ids(c)
    assert all(torch.equal(x["out"].token_logprobs, y["out"].token_logprobs) for x, y in zip(a, b))
    assert _ids(a) != _ids(log0)                              # (T = 1 on random-initialised weights: the samples leave the greedy path)
    # svln_get_top2 after a sampled turn: refused by name
    buf = (C.c_float * 2)()
    assert m._lib.svln_get_top2(m._h, buf) != 0 and b"svln_set_sampling" in m._lib.svln_last_error()
    m.set_token_scores(False)
    m.set_sampling(None)
    log1, taps1 = _episode(m, sc, steps)                      # the agent's do_sample=False call
    assert _ids(log1) == _ids(log0)
    for x, y in zip(taps0, taps1):
        assert np.array_equal(x["hidden"], y["hidden"]) and x["cache_len"] == y["cache_len"]
    assert m._lib.svln_get_top2(m._h, buf) == 0
    # a greedy call flips a switch that generate(do_sample=True) left on
    a2, _ = _episode(m, sc, 4, T=1.0, seed=11)
    assert m._sampling == (1.0, 11) and _ids(a2) == _ids(a)[:len(a2)]
    log2, _ = _episode(m, sc, 4)
    assert m._sampling is None and _ids(log2) == _ids(log0)[:len(log2)]
    m.close()


@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_cold_temperature_reproduces_the_greedy_fixtures(name):
    sc, g = SCENARIOS[name], load_golden(name)
    m = _model(sc, torch.float32)
    log, _ = _episode(m, sc, 16, T=2.0 ** -14, seed=5)
    assert len(log) >= 4
    for t, r in enumerate(log):
        assert r["out"].sequences[0].tolist() == g[f"t{t}_ids"].tolist(), (name, t)
    m.close()


@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_every_token_is_the_restated_sample_of_its_own_tap_row(name):
    sc, seed = SCENARIOS[name], 0xC0FFEE1234
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    log, taps = _episode(m, sc, 36 if name == "tiny_episode" else 16, T=1.0, seed=seed)
    Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
    stats, draw = dict(tokens=0, under=0, score=0.0), 0
    for t, (r, tp) in enumerate(zip(log, taps)):
        assert tuple(r["out"].token_logprobs.shape) == tuple(r["out"].sequences.shape)
        draw += _check_turn(Wd, r["out"], tp["hidden"], 1.0, seed, 0, draw, pen, stats, (name, t))
    SHARE[name] = stats
    print(f"{name}: {stats['under']} of {stats['tokens']} tokens under the margin; worst |score - ref| / bound = {stats['score']:.3f}")
    assert stats["tokens"] >= 12 and stats["under"] <= 0.05 * stats["tokens"], stats
    m.close()


@pytest.mark.parametrize("mode", ["bf16", "fp8", "mxfp4"])
def test_bf16_engine_and_quantised_heads_sample_deterministically_and_score_their_own_logits(mode):
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    m = _model(sc, torch.bfloat16)
    if mode != "bf16":
        (m.set_fp8_decode if mode == "fp8" else m.set_mxfp4_decode)(True)
    m.set_token_scores(True)
    seed = 77
    a, taps = _episode(m, sc, 12, T=0.5, seed=seed)
    b, _ = _episode(m, sc, 12, T=0.5, seed=seed)
    assert _ids(a) == _ids(b) and all(torch.equal(x["out"].token_logprobs, y["out"].token_logprobs) for x, y in zip(a, b))
    Wd = _head(m, None if mode == "bf16" else mode)
    stats, draw = dict(tokens=0, under=0, score=0.0), 0
    for t, (r, tp) in enumerate(zip(a, taps)):
        draw += _check_turn(Wd, r["out"], tp["hidden"], 0.5, seed, 0, draw, 1.0, stats, (mode, t))
    print(f"{mode}: {stats['under']} of {stats['tokens']} tokens under the margin; worst |score - ref| / bound = {stats['score']:.3f}")
    m.close()


# ------------------------------------------------------------------------------------------------------------ several envs
def _solo(m, sc, N, ticks, T, seed, lengths=None):
    """every env on its own through generate, `ticks(e)` env steps each"""
    m.reset(N)
    m.sampling_seed = seed
    m.set_sampling(T, seed)
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
    sc, T, seed, steps = SCENARIOS[name], 1.0, 2024, 16
    m = _model(sc, torch.float32, envs=N, frames=3 * N)
    solo = _solo(m, sc, N, lambda e: steps, T, seed)
    m.reset(N)
    m.set_sampling(T, seed)
    agents = [_agent(m, sc, e, T) for e in range(N)]
    group = BatchedAgents(agents)
    for step in range(steps):
        group.act([synthetic_frame(e, step) for e in range(N)])
    for e in range(N):
        assert _ids(agents[e].turn_log) == solo[e], (N, name, e)
    assert len({str(s) for s in solo}) == N                   # the envs' streams differ
    m.close()


def test_scheduler_samples_what_generate_samples():
    sc, N, T, seed = SCENARIOS["tiny_episode"], 4, 1.0, 2025
    m = _model(sc, torch.float32, envs=N, frames=3)
    lengths = lambda e, t: 2 if (e + t) % 2 == 0 else 4
    m.reset(N)
    m.sampling_seed = seed
    m.set_sampling(T, seed)
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
    solo = _solo(m, sc, N, lambda e: steps_taken[e], T, seed, lengths)
    for e in range(N):
        n = min(len(sched[e]), len(solo[e]))
        assert n >= 3 and sched[e][:n] == solo[e][:n], (e, sched[e], solo[e])
    m.close()


# ------------------------------------------------------------------------------------------------------------ surface
def test_refusal_matrix_in_flight_and_kwargs():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16, envs=2, frames=6)
    others = [("svln_set_speculative", lambda on: m.set_speculative(2 if on else 0)), ("svln_set_prefill_draft", m.set_prefill_draft),
              ("svln_set_batch_draft", m.set_batch_draft), ("svln_set_decode_persistent", m.set_decode_persistent),
              ("svln_set_mxfp4_batched", m.set_mxfp4_batched)]
    for name, switch in others:
        switch(True)
        with pytest.raises(_lib.SvlnError, match=name):
            m.set_sampling(1.0, 1)
        switch(False)
        m.set_sampling(1.0, 1)
        with pytest.raises(_lib.SvlnError, match="svln_set_sampling"):
            switch(True)
        switch(False)                                       # off is always allowed
        m.set_sampling(None)
    for allowed in (m.set_fp8_decode, m.set_mxfp4_decode, m.set_fp8_gemm, m.set_fp8_scaled_mfma, m.set_token_scores):
        m.set_sampling(0.7, 3)
        allowed(True)
        m.set_sampling(None)
        m.set_sampling(0.7, 3)
        allowed(False)
        m.set_sampling(None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            m.set_sampling(bad, 0)
        assert m._lib.svln_set_sampling(m._h, 1, bad, 0) != 0
    assert m._sampling is None
    # in flight: every call is refused, on or off
    agents = [_agent(m, sc, e) for e in range(2)]
    for e, ag in enumerate(agents):
        ag.observe(synthetic_frame(e, 0))
    req = agents[0]._build_request("")
    m.submit(**req)
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_sampling(1.0, 0)
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_sampling(None)
    with pytest.raises(_lib.SvlnError, match="in flight"):     # a sampled turn beside a greedy one in flight
        m.submit(**dict(agents[1]._build_request(""), do_sample=True))
    m.cancel()
    # kwargs
    m.reset(2)
    ag = _agent(m, sc, 0)
    ag.observe(synthetic_frame(0, 0))
    req = ag._build_request("")
    for kw, key in ((dict(top_k=50), "top_k"), (dict(top_p=0.9), "top_p"), (dict(num_beams=2), "num_beams")):
        with pytest.raises(NotImplementedError, match=key):
            m.generate(**dict(req, do_sample=True, **kw))
    assert m._sampling is None
    m.generation_config.temperature = 0.5
    m.sampling_seed = 9
    out = m.generate(**dict(req, do_sample=True, top_k=0, top_p=1.0))
    assert m._sampling == (0.5, 9) and out.sequences.shape[1] >= 1
    m.reset(2)
    m.generate(**dict(req, do_sample=True, temperature=2.0))
    assert m._sampling == (2.0, 9)
    m.reset(2)
    m.generate(**req)                                       # the harness's do_sample=False
    assert m._sampling is None
    m.close()


def test_zz_share_report():
    for name, st in sorted(SHARE.items()):
        print(f"{name}: {st['under']} of {st['tokens']} tokens under the margin ({100.0 * st['under'] / max(st['tokens'], 1):.1f} %), "
              f"worst |score - ref| / bound {st['score']:.3f}")
