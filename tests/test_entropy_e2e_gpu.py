"""Token entropies end to end (set_token_entropy / svln_token_entropy) on the GPU, fixtures tiny_episode / tiny_penalty.

(1) The switch changes nothing else: ids, hidden rows, cache lengths and token_logprobs are bit-identical to the switch off (fp32 and bf16
engines; generate with the decode graphs on and off, generate_batch at 8 lockstep envs -- the MFMA head -- and at 2 envs -- the batched
GEMV head, with the repetition penalty -- and the staggered scheduler); off after on equals never on.
(2) Every entropy is checked against float64 softmax(lm_head . h) computed from the engine's OWN tap row h and the loaded lm_head (the
dequantised copy under set_fp8_decode / set_mxfp4_decode), penalty over the ids generated so far, times 1 / T under sampling.  The bound is
derived and evaluated per row in float64; no row is exempt (an entropy has no ties).  With
    delta = 2 gamma_K max_n sum_k |w_nk h_k|,  gamma_K = K 2^-24
the a-priori bound of an fp32 dot product in any summation order on either side (tests/test_scores_e2e_gpu.py), the processed value y_n is
off by at most  dy = (delta max(pen, 1 / pen) + u max|x|) / T + u max|y|  (u = 2^-24: the penalty's and the temperature's roundings).
H = log Z - sum p_n y_n has the gradient dH / dy_n = -p_n (log p_n + H), hence the first-order term  dy * A,  A = sum_n p_n |log p_n + H|
(at most 2 H).  Its Hessian is  -p_n (d_nm - p_m) c_n - p_n d_nm + p_n p_m (1 + c_m)  with c_n = y_n - sum p y = log p_n + H; the sum of
the absolute values of its entries is at most 2 + 3 A, and at any point of the dy-ball p_n grows by at most e^(2 dy) and |c_n| by 2 dy, so
the second-order remainder is at most  1/2 dy^2 e^(4 dy) (2 + 3 (A + 2 dy)).  Plus the op tolerance entropy_ref.TOL (derived there).
(3) Under an allowed list the entropy equals that of the distribution `allowed_logprobs` carries, within the op tolerance.
(4) The refusal matrix, the three getters, the agents' last_token_entropies / last_turn_entropy."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import entropy_ref as E
import mxfp4_ref as MX
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
WORST = {}


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
    """one env through `steps` env steps (T: sampled at that temperature, the counters restart) -> (turn log, taps, agent)"""
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
            taps.append(dict(hidden=m.last_hidden(), cache_len=m.env_state(0)[1], ent=ag.last_token_entropies, mean=ag.last_turn_entropy))
    return ag.turn_log, taps, ag


def _ids(log):
    return [r["out"].sequences[0].tolist() for r in log]


def _head(m, mode=None):
    w = torch.from_numpy(m.get_tensor("lm_head.weight")).float()
    if mode == "fp8":
        w = O.qdq_e4m3_rows(w)
    elif mode == "mxfp4":
        w = MX.qdq_mxfp4(w).float()
    return w.double()


def _ref(Wd, hidden, ids, penalty=1.0, T=1.0):
    """float64 (entropy, bound) of every emitted id's distribution from the tap rows (the derivation is in the module docstring)"""
    K = Wd.shape[1]
    gamma = K * 2.0 ** -24
    inv_t = float(np.float32(1.0) / np.float32(T))
    out = []
    for k in range(len(ids)):
        h = torch.from_numpy(np.asarray(hidden[k], dtype=np.float64))
        x = Wd @ h
        if penalty != 1.0 and k:
            seen = torch.tensor(sorted(set(ids[:k])), dtype=torch.long)
            x[seen] = torch.where(x[seen] < 0, x[seen] * penalty, x[seen] / penalty)
        y = (x * inv_t).numpy()
        delta = 2 * gamma * float((Wd.abs() @ h.abs()).max())
        dy = (delta * max(penalty, 1.0 / penalty) + U * float(x.abs().max())) * inv_t + U * float(np.abs(y).max())
        lse = float(torch.logsumexp(torch.from_numpy(y), 0))
        logp = y - lse
        p = np.exp(logp)
        H = float(-(p * logp).sum())
        A = float((p * np.abs(logp + H)).sum())
        bound = dy * A + 0.5 * dy * dy * math.exp(4 * dy) * (2 + 3 * (A + 2 * dy)) + E.TOL
        out.append((H, bound))
    return out


def _check(Wd, out, hidden, penalty=1.0, T=1.0, what=""):
    ids = out.sequences[0].tolist()
    ent = out.token_entropies
    assert ent.dtype == torch.float32 and tuple(ent.shape) == (1, len(ids)) and ent.device == out.sequences.device, (what, ent.shape)
    n = min(len(ids), len(hidden))                          # (the taps hold a bounded number of rows)
    got = ent[0].tolist()
    assert all(g >= 0.0 for g in got), (what, got)
    for k, (H, bound) in enumerate(_ref(Wd, hidden[:n], ids[:n], penalty, T)):
        err = abs(got[k] - H)
        WORST[what[0]] = max(WORST.get(what[0], 0.0), err / bound)
        assert err <= bound, (what, k, got[k], H, err, bound)


def _same(log0, taps0, log1, taps1):
    assert _ids(log1) == _ids(log0)
    for a, b in zip(taps0, taps1):
        assert np.array_equal(a["hidden"], b["hidden"]) and a["cache_len"] == b["cache_len"]
    for r0, r1 in zip(log0, log1):
        assert torch.equal(r0["out"].token_logprobs, r1["out"].token_logprobs)
        assert r0["out"].token_logprobs.view(torch.int32).tolist() == r1["out"].token_logprobs.view(torch.int32).tolist()


# ------------------------------------------------------------------------------------------------------------ single env
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_generate_switch_on_equals_off_and_entropies_match_the_head(name, dtype, graph):
    sc = SCENARIOS[name]
    m = _model(sc, dtype)
    m.set_decode_graph(graph)
    m.set_token_scores(True)
    steps = sc["steps"] if graph else 8
    log0, taps0, ag0 = _episode(m, sc, steps)
    assert all("token_entropies" not in r["out"] and r["out"].token_entropies is None for r in log0)
    assert ag0.last_token_entropies is None and ag0.last_turn_entropy is None
    m.set_token_entropy(True)
    m.set_token_entropy(True)                               # a call that changes nothing succeeds
    log1, taps1, ag1 = _episode(m, sc, steps)
    _same(log0, taps0, log1, taps1)
    assert any(r["memory"] for r in log1) or not graph
    if dtype == torch.float32:
        Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
        for t, (r, tp) in enumerate(zip(log1, taps1)):
            _check(Wd, r["out"], tp["hidden"], pen, 1.0, ("generate " + name, t))
    for r, tp in zip(log1, taps1):
        assert torch.equal(tp["ent"], r["out"].token_entropies) and tp["mean"] == pytest.approx(float(r["out"].token_entropies.mean()))
    ag1.reset_memory()
    assert ag1.last_token_entropies is None and ag1.last_turn_entropy is None
    # off after on equals never on; the getter is refused by name
    m.set_token_entropy(False)
    log2, taps2, _ = _episode(m, sc, 8)
    _same(log0[:len(log2)], taps0[:len(log2)], log2, taps2)
    assert "token_entropies" not in log2[0]["out"]
    buf, n = (C.c_float * 8)(), C.c_int32()
    assert m._lib.svln_get_token_entropy(m._h, buf, 8, C.byref(n)) != 0 and b"svln_token_entropy" in m._lib.svln_last_error()
    m.close()


@pytest.mark.parametrize("T", [0.5, 2.0])
def test_sampled_entropy_is_that_of_the_tempered_softmax(T):
    sc = SCENARIOS["tiny_penalty"]
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    log0, taps0, _ = _episode(m, sc, 8, T, 11)
    m.set_token_entropy(True)
    log1, taps1, _ = _episode(m, sc, 8, T, 11)
    _same(log0, taps0, log1, taps1)
    Wd = _head(m)
    for t, (r, tp) in enumerate(zip(log1, taps1)):
        _check(Wd, r["out"], tp["hidden"], sc["rep_penalty"], T, (f"sampled T={T}", t))
    m.close()


def test_allowed_list_entropy_is_over_the_allowed_set():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    m.set_allowed_tokens(list(range(3, 200, 7)))
    for T in (None, 2.0):
        m.set_token_entropy(False)
        log0, taps0, _ = _episode(m, sc, 8, T, 5)
        m.set_token_entropy(True)
        log1, taps1, _ = _episode(m, sc, 8, T, 5)
        _same(log0, taps0, log1, taps1)
        for r in log1:
            alp = r["out"].allowed_logprobs[0].double().cpu().numpy()           # [n_new][n_allowed]
            ref = [-float((np.exp(a[a > -np.inf]) * a[a > -np.inf]).sum()) for a in alp]
            got = r["out"].token_entropies[0].tolist()
            assert len(got) == len(ref) and max(abs(a - b) for a, b in zip(got, ref)) <= E.TOL, (T, got, ref)
            assert max(got) <= math.log(len(m.allowed_token_ids)) + E.TOL
    m.close()


@pytest.mark.parametrize("mode", ["fp8", "mxfp4", "packed"])
def test_quantised_and_packed_lm_heads_give_the_entropy_of_their_own_logits(mode):
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    m = _model(sc, torch.bfloat16)
    {"fp8": m.set_fp8_decode, "mxfp4": m.set_mxfp4_decode, "packed": m.set_packed_decode}[mode](True)
    m.set_token_scores(True)
    log0, taps0, _ = _episode(m, sc, 8)
    m.set_token_entropy(True)
    log1, taps1, _ = _episode(m, sc, 8)
    _same(log0, taps0, log1, taps1)
    Wd = _head(m, mode)
    for t, (r, tp) in enumerate(zip(log1, taps1)):
        _check(Wd, r["out"], tp["hidden"], 1.0, 1.0, (mode, t))
    m.close()


# ------------------------------------------------------------------------------------------------------------ several envs
def _agents(m, sc, N):
    return [_agent(m, sc, e) for e in range(N)]


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
                conf[e].append((agents[e].last_token_entropies, agents[e].last_turn_entropy))
    return agents, hidden, conf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,name", [(8, "tiny_episode"), (2, "tiny_penalty")])
def test_generate_batch_switch_on_equals_off_and_entropies_match_the_head(N, name, dtype):
    sc = SCENARIOS[name]
    m = _model(sc, dtype, envs=N, frames=3 * N)
    m.set_token_scores(True)
    steps = 16
    a0, h0, c0 = _lockstep(m, sc, N, steps)
    assert all(c == (None, None) for e in range(N) for c in c0[e])
    m.set_token_entropy(True)
    a1, h1, c1 = _lockstep(m, sc, N, steps)
    Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
    for e in range(N):
        assert _ids(a1[e].turn_log) == _ids(a0[e].turn_log), e
        for t, (r0, r1) in enumerate(zip(a0[e].turn_log, a1[e].turn_log)):
            assert np.array_equal(h0[e][t], h1[e][t]) and r0["out"].past_key_values.get_seq_length() == r1["out"].past_key_values.get_seq_length()
            assert r0["out"].token_logprobs.view(torch.int32).tolist() == r1["out"].token_logprobs.view(torch.int32).tolist()
            assert "token_entropies" not in r0["out"]
            if dtype == torch.float32:
                _check(Wd, r1["out"], h1[e][t], pen, 1.0, (f"generate_batch N={N}", e, t))
            ent, mean = c1[e][t]
            assert torch.equal(ent, r1["out"].token_entropies) and mean == pytest.approx(float(r1["out"].token_entropies.mean()))
    # the getter of every listed env; a batch that ran with the switch off is refused by name
    buf, n = (C.c_float * 16)(), C.c_int32()
    last = [a.turn_log[-1]["out"] for a in a1]
    for e, o in enumerate(last):
        assert m._lib.svln_generate_batch_entropy(m._h, e, buf, 16, C.byref(n)) == 0 and n.value == o.sequences.shape[1]
        assert [buf[k] for k in range(n.value)] == o.token_entropies[0].tolist()
    assert m._lib.svln_generate_batch_entropy(m._h, N, buf, 16, C.byref(n)) != 0
    m.set_token_entropy(False)
    _lockstep(m, sc, N, 1)
    assert m._lib.svln_generate_batch_entropy(m._h, 0, buf, 16, C.byref(n)) != 0 and b"svln_token_entropy" in m._lib.svln_last_error()
    m.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_scheduler_switch_on_equals_off_and_entropies_match_the_head(dtype):
    sc, N = SCENARIOS["tiny_episode"], 4
    m = _model(sc, dtype, envs=N, frames=3)
    m.set_token_scores(True)
    lengths = lambda e, t: 2 if (e + t) % 2 == 0 else 4

    def run():
        m.reset(N)
        agents = _agents(m, sc, N)
        for e, ag in enumerate(agents):
            ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
        hidden = [[] for _ in range(N)]

        def on_result(i, ticket, out):
            hidden[i].append(m.last_hidden_batch(ticket.slot))
        group = AsyncBatchedAgents(agents, on_result=on_result)
        for tick in range(24):
            group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active={i for i in range(N) if tick >= i})
        return agents, hidden, group.stats

    a0, h0, _ = run()
    m.set_token_entropy(True)
    a1, h1, st = run()
    assert st["mixed_iterations"] >= 2, st
    Wd = _head(m)
    for e in range(N):
        assert _ids(a1[e].turn_log) == _ids(a0[e].turn_log) and len(a1[e].turn_log) >= 3, e
        for t, (r0, r1) in enumerate(zip(a0[e].turn_log, a1[e].turn_log)):
            assert np.array_equal(h0[e][t], h1[e][t]) and "token_entropies" not in r0["out"]
            assert r0["out"].past_key_values.get_seq_length() == r1["out"].past_key_values.get_seq_length()
            assert r0["out"].token_logprobs.view(torch.int32).tolist() == r1["out"].token_logprobs.view(torch.int32).tolist()
            if dtype == torch.float32:
                _check(Wd, r1["out"], h1[e][t], 1.0, 1.0, ("scheduler", e, t))
        assert torch.equal(a1[e].last_token_entropies, a1[e].turn_log[-1]["out"].token_entropies)
        assert a1[e].last_turn_entropy == pytest.approx(float(a1[e].turn_log[-1]["out"].token_entropies.mean()))
    m.close()


def test_fp8_gemm_products_keep_the_bf16_head():
    sc, N = SCENARIOS["tiny_episode"], 4
    m = _model(sc, torch.bfloat16, envs=N, frames=3 * N)
    m.set_fp8_gemm(True)
    m.set_fp8_scaled_mfma(True)
    m.set_token_scores(True)
    m.set_token_entropy(True)
    agents, hidden, _ = _lockstep(m, sc, N, 8)
    Wd = _head(m)
    for e in range(N):
        for t, r in enumerate(agents[e].turn_log):
            _check(Wd, r["out"], hidden[e][t], 1.0, 1.0, ("fp8 gemm", e, t))
    m.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusal_matrix_and_getters():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16, envs=2, frames=6)
    L, h = m._lib, m._h
    # needs the scores first, and keeps them on
    with pytest.raises(_lib.SvlnError, match="svln_set_token_scores"):
        m.set_token_entropy(True)
    m.set_token_entropy(False)                              # off while off changes nothing
    m.set_token_scores(True)
    m.set_token_entropy(True)
    with pytest.raises(_lib.SvlnError, match="svln_token_entropy"):
        m.set_token_scores(False)
    # the candidate siblings, both ways
    with pytest.raises(_lib.SvlnError, match="svln_token_entropy"):
        m.set_top_logprobs(4)
    m.set_token_entropy(False)
    m.set_top_logprobs(4)
    with pytest.raises(_lib.SvlnError, match="svln_top_logprobs"):
        m.set_token_entropy(True)
    m.set_top_logprobs(0)
    m.set_sampling(1.0, 3)
    m.set_token_entropy(True)                               # sampling without truncation composes
    assert L.svln_sampling_truncation(h, 4, 0.9) != 0 and b"svln_token_entropy" in L.svln_last_error()
    m.set_token_entropy(False)
    _lib.check(L.svln_sampling_truncation(h, 4, 0.9))
    with pytest.raises(_lib.SvlnError, match="svln_sampling_truncation"):
        m.set_token_entropy(True)
    _lib.check(L.svln_sampling_truncation(h, 0, 1.0))
    m.set_token_entropy(True)
    # the turn forms that carry no entropies, refused while on (and naming the switch)
    ids = (C.c_int64 * 4)(5, 6, 7, 8)
    eos = (C.c_int64 * 1)(1)
    out64, n32, f32 = (C.c_int64 * 64)(), (C.c_int32 * 8)(), (C.c_float * 64)()
    lens = (C.c_int32 * 2)(2, 2)
    slot = C.c_int32()
    assert L.svln_generate_group(h, 0, 2, 4, eos, 1, out64, 8, n32) != 0 and b"svln_token_entropy" in L.svln_last_error()
    m.set_sampling(None)
    assert L.svln_generate_beams(h, 0, 2, 4, eos, 1, out64, 8, n32, f32) != 0 and b"svln_token_entropy" in L.svln_last_error()
    assert L.svln_generate_forced(h, 0, ids, 4, eos, 1, f32, out64, f32, None) != 0 and b"svln_token_entropy" in L.svln_last_error()
    assert L.svln_generate_candidates(h, 0, 2, ids, lens, eos, 1, f32, out64, f32) != 0 and b"svln_token_entropy" in L.svln_last_error()
    assert L.svln_batch_submit_forced(h, 0, ids, 4, eos, 1, C.byref(slot)) != 0 and b"svln_token_entropy" in L.svln_last_error()
    # the allowed modes
    m.set_token_entropy(False)
    for allowed in (m.set_fp8_decode, m.set_mxfp4_decode, m.set_packed_decode, m.set_fp8_gemm, m.set_fp8_scaled_mfma):
        m.set_token_entropy(True)
        allowed(True)
        m.set_token_entropy(False)
        m.set_token_entropy(True)
        allowed(False)
        m.set_token_entropy(False)
    # a change while scheduler turns are in flight; the getter of a turn that ran with the switch off, and of one that ran with it on
    agents = _agents(m, sc, 2)
    for e, ag in enumerate(agents):
        ag.observe(synthetic_frame(e, 0))
    buf, n = (C.c_float * 16)(), C.c_int32()
    ticket = m.submit(**agents[0]._build_request(""))
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_token_entropy(True)
    done = []
    while not done:
        running, nf, fin = C.c_int32(), C.c_int32(), (C.c_int32 * 8)()
        _lib.check(L.svln_batch_step(h, C.byref(running), fin, C.byref(nf)))
        done = [fin[k] for k in range(nf.value)]
    assert L.svln_batch_entropy(h, ticket.slot, buf, 16, C.byref(n)) != 0 and b"svln_token_entropy" in L.svln_last_error()
    m.cancel()
    m.set_token_entropy(True)
    t1 = m.submit(**agents[1]._build_request(""))
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_token_entropy(False)
    assert L.svln_batch_entropy(h, t1.slot, buf, 16, C.byref(n)) != 0                   # not finished yet
    fin, running = m.step_batch()
    while not fin:
        fin, running = m.step_batch()
    res = fin[0][1]
    assert res.token_entropies.shape == res.sequences.shape and res.token_entropies.dtype == torch.float32
    assert L.svln_batch_entropy(h, t1.slot, buf, 16, C.byref(n)) != 0                   # svln_batch_result freed the slot
    assert L.svln_get_token_entropy(h, None, 16, C.byref(n)) != 0 and L.svln_get_token_entropy(h, buf, 16, None) != 0
    assert L.svln_get_token_entropy(h, buf, 16, C.byref(n)) != 0                        # no single-env turn has run with the switch on
    m.close()


def test_report_worst():
    print("worst |H - float64| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
