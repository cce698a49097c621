"""Token log-probabilities end to end (set_token_scores / svln_set_token_scores) on the GPU.

(1) The switch changes nothing else: ids, hidden rows and cache lengths are bit-identical to the switch off (fp32 and bf16 engines;
generate, generate_batch at 8 lockstep envs -- the MFMA head -- and at 2 envs -- the batched GEMV head -- and the staggered scheduler).
(2) Every emitted token's score is checked against float64 log_softmax(lm_head . h) computed from the engine's OWN tap row h and the
loaded lm_head (the dequantised copy under set_fp8_decode / set_mxfp4_decode), penalty over the ids generated so far, inside
    2 * max_n gamma_K sum_k |w_nk h_k| + 2e-5,     gamma_K = K * 2^-24
-- the a-priori bound of an fp32 dot product in any summation order (bf16 x bf16 products are exact in fp32) on either side of the
softmax, plus the op-level log-sum-exp bound (tests/test_scores_gpu.py).  The bound is computed per token, not chosen.
(3) On the fp32 engine the scores also sit within 2 * max_n |w_n|_1 * |h_engine - h_fixture|_inf + 2e-5 of those computed from the golden
fixtures' hidden rows.
(4) The refusal matrix, both orders; the getters when the switch was off; the agents' last_token_logprobs / last_turn_logprob."""
import ctypes as C

import numpy as np
import pytest
import torch

import mxfp4_ref as MX
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from util import load_golden

pytestmark = pytest.mark.gpu
LSE_TOL = 2e-5
PF32 = C.POINTER(C.c_float)


def _model(sc, dtype, envs=1, frames=None):
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=envs, max_frames=frames or 1 + (sc["num_history"] or 0), max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    apply_knobs(m, sc)
    return m


def _episode(m, sc, steps=None):
    taps = []

    def on_turn(t, rec):
        taps.append(dict(hidden=m.last_hidden(), cache_len=m.env_state(0)[1]))
    log = run_scenario(m, sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda", steps=steps)
    return log, taps


def _head(m, mode=None):
    """float64 lm_head the engine multiplies by: the loaded tensor in the engine's type, or its dequantised e4m3 / MXFP4 copy"""
    w = torch.from_numpy(m.get_tensor("lm_head.weight")).float()
    if mode == "fp8":
        w = O.qdq_e4m3_rows(w)
    elif mode == "mxfp4":
        w = MX.qdq_mxfp4(w).float()
    return w.double()


def _ref(Wd, hidden, ids, penalty=1.0):
    """float64 (log-probability, bound) of every emitted id from the tap rows: penalty over the ids generated so far in the turn"""
    K = Wd.shape[1]
    gamma = K * 2.0 ** -24
    lps, bounds = [], []
    for k, tok in enumerate(ids):
        h = torch.from_numpy(np.asarray(hidden[k], dtype=np.float64))
        l = Wd @ h
        if penalty != 1.0 and k:
            seen = torch.tensor(sorted(set(ids[:k])), dtype=torch.long)
            l[seen] = torch.where(l[seen] < 0, l[seen] * penalty, l[seen] / penalty)
        lps.append(float(l[tok] - torch.logsumexp(l, 0)))
        bounds.append(2 * gamma * float((Wd.abs() @ h.abs()).max()) + LSE_TOL)
    return lps, bounds


def _check_scores(Wd, out, hidden, penalty=1.0, what=""):
    ids = out.sequences[0].tolist()
    lp = out.token_logprobs
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (1, len(ids)) and lp.device == out.sequences.device, (what, lp.shape)
    n = min(len(ids), len(hidden))                          # (the taps hold a bounded number of rows)
    ref, bound = _ref(Wd, hidden[:n], ids[:n], penalty)
    got = lp[0].tolist()
    assert all(g <= 0.0 for g in got), (what, got)
    worst = 0.0
    for k in range(n):
        err = abs(got[k] - ref[k])
        worst = max(worst, err / bound[k])
        assert err <= bound[k], (what, k, got[k], ref[k], err, bound[k])
    return worst


def _ids(log):
    return [r["out"].sequences[0].tolist() for r in log]


# ------------------------------------------------------------------------------------------------------------ single env
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_generate_switch_on_equals_off_and_scores_match_the_head(name, dtype):
    """nine turns through two window restarts (tiny_episode: turns end by EOS) / four turns under the repetition penalty (they end by
    max_new_tokens): the run with the switch on is bit-identical, and every token -- token 0 of a turn comes from the prefill head -- has the score
    of the head's own hidden row"""
    sc = SCENARIOS[name]
    m = _model(sc, dtype)
    log0, taps0 = _episode(m, sc)
    assert all("token_logprobs" not in r["out"] for r in log0)
    m.set_token_scores(True)
    m.reset(1)
    log1, taps1 = _episode(m, sc)
    assert _ids(log1) == _ids(log0)
    for a, b in zip(taps0, taps1):
        assert np.array_equal(a["hidden"], b["hidden"]) and a["cache_len"] == b["cache_len"]
    Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
    worst = max(_check_scores(Wd, r["out"], tp["hidden"], pen, (name, t)) for t, (r, tp) in enumerate(zip(log1, taps1)))
    # tiny_episode's turns end by EOS (at varying lengths), tiny_penalty's by max_new_tokens; both run through a <memory> turn
    eos = set(eos_ids(sc))
    ends = {("eos" if r["out"].sequences[0, -1].item() in eos else "max_new") for r in log1}
    assert ends == ({"eos"} if name == "tiny_episode" else {"max_new"}), ends
    assert any(r["memory"] for r in log1) and len({r["out"].sequences.shape[1] for r in log1}) > (1 if name == "tiny_episode" else 0)
    if dtype == torch.float32:                              # against the fixtures' hidden rows
        g = load_golden(name)
        for t, (r, tp) in enumerate(zip(log1, taps1)):
            ids = r["out"].sequences[0].tolist()
            assert ids == g[f"t{t}_ids"].tolist()
            hf = g[f"t{t}_hidden"]
            ref, _ = _ref(Wd, hf, ids, pen)
            dh = np.abs(tp["hidden"][:len(ids)].astype(np.float64) - hf[:len(ids)]).max(1)
            w1 = float(Wd.abs().sum(1).max())
            for k, lp in enumerate(r["out"].token_logprobs[0].tolist()):
                assert abs(lp - ref[k]) <= 2 * w1 * float(dh[k]) + LSE_TOL, (name, t, k, lp, ref[k], float(dh[k]))
    # the switch off again: the key is gone and the getter is refused
    m.set_token_scores(False)
    m.reset(1)
    log2, _ = _episode(m, sc, steps=4)
    assert _ids(log2) == _ids(log0)[:len(log2)] and "token_logprobs" not in log2[0]["out"]
    buf, n = (C.c_float * 8)(), C.c_int32()
    assert m._lib.svln_get_token_scores(m._h, buf, 8, C.byref(n)) != 0 and b"svln_set_token_scores" in m._lib.svln_last_error()
    print(f"{name} {dtype}: worst |score - ref| / bound = {worst:.3f}")
    m.close()


def test_true_width_turns_through_the_memory_turn_vs_fixture():
    """true1_episode (hidden 3584, one layer) on the fp32 engine with the switch on: ids equal the fixture's (the switch-off reference) and
    the scores obey both bounds; the last turn carries the 1568-row <memory> block"""
    sc, g = SCENARIOS["true1_episode"], load_golden("true1_episode")
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    log, taps = _episode(m, sc)
    assert any(r["memory"] for r in log)
    Wd = _head(m)
    w1 = float(Wd.abs().sum(1).max())
    for t, (r, tp) in enumerate(zip(log, taps)):
        ids = r["out"].sequences[0].tolist()
        assert ids == g[f"t{t}_ids"].tolist() and tp["cache_len"] == int(g[f"t{t}_cache_len"]), t
        _check_scores(Wd, r["out"], tp["hidden"], 1.0, ("true1", t))
        ref, _ = _ref(Wd, g[f"t{t}_hidden"], ids)
        dh = np.abs(tp["hidden"][:len(ids)].astype(np.float64) - g[f"t{t}_hidden"][:len(ids)]).max(1)
        for k, lp in enumerate(r["out"].token_logprobs[0].tolist()):
            assert abs(lp - ref[k]) <= 2 * w1 * float(dh[k]) + LSE_TOL, (t, k, lp, ref[k])
    m.close()


@pytest.mark.parametrize("mode", ["fp8", "mxfp4"])
def test_quantised_lm_heads_score_their_own_logits(mode):
    """set_fp8_decode / set_mxfp4_decode: the weight policy is a template parameter of the scored kernel, so the quantised lm_head comes
    with it -- reference: the dequantised copy; ids equal the same mode with the switch off"""
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    m = _model(sc, torch.bfloat16)
    (m.set_fp8_decode if mode == "fp8" else m.set_mxfp4_decode)(True)
    log0, taps0 = _episode(m, sc, steps=12)
    m.set_token_scores(True)
    m.reset(1)
    log1, taps1 = _episode(m, sc, steps=12)
    assert _ids(log1) == _ids(log0) and all(np.array_equal(a["hidden"], b["hidden"]) for a, b in zip(taps0, taps1))
    Wd = _head(m, mode)
    for t, (r, tp) in enumerate(zip(log1, taps1)):
        _check_scores(Wd, r["out"], tp["hidden"], 1.0, (mode, t))
    m.close()


# ------------------------------------------------------------------------------------------------------------ several envs
def _agents(m, sc, N):
    proc = m.get_vision_tower().image_processor
    out = []
    for e in range(N):
        enc = SyntheticPromptEncoder(sc["cfg"], seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        out.append(StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                                  device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=proc.preprocess_array))
    return out


def _lockstep(m, sc, N, steps):
    m.reset(N)
    agents = _agents(m, sc, N)
    group = BatchedAgents(agents)
    hidden, conf = [[] for _ in range(N)], [[] for _ in range(N)]
    for step in range(steps):
        n0 = len(agents[0].turn_log)
        group.act([synthetic_frame(e, step) for e in range(N)])
        if len(agents[0].turn_log) > n0:
            for e in range(N):
                hidden[e].append(m.last_hidden_batch(e))
                conf[e].append((agents[e].last_token_logprobs, agents[e].last_turn_logprob))
    return agents, hidden, conf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,name", [(8, "tiny_episode"), (2, "tiny_penalty")])
def test_generate_batch_switch_on_equals_off_and_scores_match_the_head(N, name, dtype):
    """8 lockstep envs go through the MFMA head, 2 envs through the batched GEMV (there with the repetition penalty: row b's own flag row);
    through a window restart; BatchedAgents keep the confidence of every env"""
    sc = SCENARIOS[name]
    m = _model(sc, dtype, envs=N, frames=3 * N)
    steps = 16
    a0, h0, c0 = _lockstep(m, sc, N, steps)
    assert all(c == (None, None) for e in range(N) for c in c0[e])
    m.set_token_scores(True)
    a1, h1, c1 = _lockstep(m, sc, N, steps)
    Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
    assert any(r["memory"] for r in a1[0].turn_log)
    for e in range(N):
        assert _ids(a1[e].turn_log) == _ids(a0[e].turn_log), e
        for t, (r0, r1) in enumerate(zip(a0[e].turn_log, a1[e].turn_log)):
            assert np.array_equal(h0[e][t], h1[e][t]) and r0["out"].past_key_values.get_seq_length() == r1["out"].past_key_values.get_seq_length()
            assert "token_logprobs" not in r0["out"]
            _check_scores(Wd, r1["out"], h1[e][t], pen, (N, name, e, t))
            lp, joint = c1[e][t]
            assert torch.equal(lp, r1["out"].token_logprobs) and joint == pytest.approx(float(r1["out"].token_logprobs.sum()))
    m.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_scheduler_switch_on_equals_off_and_scores_match_the_head(dtype):
    """4 envs whose turns fall due at different times (submit / step_batch through AsyncBatchedAgents): prefilling and decoding envs share
    passes, the head rows of an iteration change in number from pass to pass"""
    sc, N = SCENARIOS["tiny_episode"], 4
    m = _model(sc, dtype, envs=N, frames=3)
    lengths = lambda e, t: 2 if (e + t) % 2 == 0 else 4

    def run():
        m.reset(N)
        agents = _agents(m, sc, N)
        for e, ag in enumerate(agents):
            ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
        hidden, conf = [[] for _ in range(N)], [[] for _ in range(N)]

        def on_result(i, ticket, out):
            hidden[i].append(m.last_hidden_batch(ticket.slot))
            conf[i].append(out.get("token_logprobs"))
        group = AsyncBatchedAgents(agents, on_result=on_result)
        for tick in range(24):
            group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active={i for i in range(N) if tick >= i})
        return agents, hidden, conf, group.stats

    a0, h0, c0, _ = run()
    m.set_token_scores(True)
    a1, h1, c1, st = run()
    assert st["mixed_iterations"] >= 2, st
    Wd = _head(m)
    for e in range(N):
        assert _ids(a1[e].turn_log) == _ids(a0[e].turn_log) and len(a1[e].turn_log) >= 3, e
        for t, (r0, r1) in enumerate(zip(a0[e].turn_log, a1[e].turn_log)):
            assert np.array_equal(h0[e][t], h1[e][t]) and c0[e][t] is None
            assert r0["out"].past_key_values.get_seq_length() == r1["out"].past_key_values.get_seq_length()
            _check_scores(Wd, r1["out"], h1[e][t], 1.0, ("scheduler", e, t))
        assert torch.equal(a1[e].last_token_logprobs, a1[e].turn_log[-1]["out"].token_logprobs)
        assert a1[e].last_turn_logprob == pytest.approx(float(a1[e].turn_log[-1]["out"].token_logprobs.sum()))
    m.close()


def test_fp8_gemm_products_keep_the_bf16_head_scored():
    """set_fp8_gemm / set_fp8_scaled_mfma are allowed: the lm_head stays bf16 there, and its scores are those of its own hidden rows"""
    sc, N = SCENARIOS["tiny_episode"], 4
    m = _model(sc, torch.bfloat16, envs=N, frames=3 * N)
    m.set_fp8_gemm(True)
    m.set_fp8_scaled_mfma(True)
    m.set_token_scores(True)
    agents, hidden, _ = _lockstep(m, sc, N, 8)
    Wd = _head(m)
    for e in range(N):
        for t, r in enumerate(agents[e].turn_log):
            _check_scores(Wd, r["out"], hidden[e][t], 1.0, ("fp8 gemm", e, t))
    m.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusal_matrix_and_getters():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16, envs=2, frames=6)
    others = [("svln_set_speculative", lambda on: m.set_speculative(2 if on else 0)), ("svln_set_prefill_draft", m.set_prefill_draft),
              ("svln_set_batch_draft", m.set_batch_draft), ("svln_set_decode_persistent", m.set_decode_persistent),
              ("svln_set_mxfp4_batched", m.set_mxfp4_batched)]
    for name, switch in others:
        switch(True)
        with pytest.raises(_lib.SvlnError, match=name):
            m.set_token_scores(True)
        switch(False)
        m.set_token_scores(True)
        m.set_token_scores(True)                            # a call that changes nothing always succeeds
        with pytest.raises(_lib.SvlnError, match="svln_set_token_scores"):
            switch(True)
        switch(False)                                       # off is always allowed
        m.set_token_scores(False)
    for allowed in (m.set_fp8_decode, m.set_mxfp4_decode, m.set_fp8_gemm, m.set_fp8_scaled_mfma):
        m.set_token_scores(True)
        allowed(True)
        m.set_token_scores(False)
        m.set_token_scores(True)
        allowed(False)
        m.set_token_scores(False)
    # a change while scheduler turns are in flight; the getters of turns that ran with the switch off
    agents = _agents(m, sc, 2)
    for e, ag in enumerate(agents):
        ag.observe(synthetic_frame(e, 0))
    ticket = m.submit(**agents[0]._build_request(""))
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_token_scores(True)
    buf, n = (C.c_float * 16)(), C.c_int32()
    done = []
    while not done:
        running, nf, fin = C.c_int32(), C.c_int32(), (C.c_int32 * 8)()
        _lib.check(m._lib.svln_batch_step(m._h, C.byref(running), fin, C.byref(nf)))
        done = [fin[k] for k in range(nf.value)]
    assert done == [ticket.slot]
    assert m._lib.svln_batch_scores(m._h, ticket.slot, buf, 16, C.byref(n)) != 0 and b"svln_set_token_scores" in m._lib.svln_last_error()
    m.cancel()
    m.set_token_scores(True)
    t1 = m.submit(**agents[1]._build_request(""))
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_token_scores(False)
    assert m._lib.svln_batch_scores(m._h, t1.slot, buf, 16, C.byref(n)) != 0            # not finished yet
    fin, running = m.step_batch()
    while not fin:
        fin, running = m.step_batch()
    assert fin[0][1].token_logprobs.shape == fin[0][1].sequences.shape
    assert m._lib.svln_batch_scores(m._h, t1.slot, buf, 16, C.byref(n)) != 0            # svln_batch_result freed the slot
    assert m._lib.svln_generate_batch_scores(m._h, 0, buf, 16, C.byref(n)) != 0         # no svln_generate_batch has run at all
    # a generate_batch that ran with the switch off: its getter is refused by name; one that ran with it on serves every listed env
    m.cancel()
    m.reset(2)
    ag = _agents(m, sc, 2)

    def batch():
        for e, a in enumerate(ag):
            a.reset_memory()
            a.observe(synthetic_frame(e, 0))
        return m.generate_batch([a._build_request("") for a in ag])
    m.set_token_scores(False)
    outs = batch()
    assert all("token_logprobs" not in o for o in outs)
    assert m._lib.svln_generate_batch_scores(m._h, 0, buf, 16, C.byref(n)) != 0 and b"svln_set_token_scores" in m._lib.svln_last_error()
    m.set_token_scores(True)
    outs = batch()
    for e, o in enumerate(outs):
        assert m._lib.svln_generate_batch_scores(m._h, e, buf, 16, C.byref(n)) == 0 and n.value == o.sequences.shape[1]
        assert [buf[k] for k in range(n.value)] == o.token_logprobs[0].tolist()
    assert m._lib.svln_generate_batch_scores(m._h, 2, buf, 16, C.byref(n)) != 0         # no such env index
    assert m._lib.svln_get_token_scores(m._h, None, 16, C.byref(n)) != 0 and m._lib.svln_get_token_scores(m._h, buf, 16, None) != 0
    m.close()
