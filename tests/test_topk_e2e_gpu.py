"""Top-k log-probabilities end to end (set_top_logprobs / svln_top_logprobs) on the GPU: generate, generate_batch at 8 envs (the MFMA head) and at
2 envs (the batched GEMV head), and the staggered scheduler.

(1) k on changes nothing else: ids, hidden rows, cache lengths and token_logprobs are bit-identical to k = 0 with the scores on (fp32 and
    bf16 engines -- the bf16 one streams the 12-bit packing --, decode graphs on and off); off after on equals never on.
(2) top_token_ids[..., 0] == sequences and top_logprobs[..., 0] is token_logprobs bit for bit (greedy); under set_sampling the emitted
    id's entry, when listed, is.
(3) fp32 engine, k = 8, tiny_episode and tiny_penalty: every list against the float64 restatement from the engine's OWN tap rows.  No
    comparison is dropped: an adjacent pair whose float64 gap is at or under the a-priori bound 2 gamma_K max_n sum_k |w_nk h_k| may come
    in either order, a rank-8 / 9 gap at or under it lets the last id be either of the two, every other id and position must match, every
    log-probability lies inside bound + 2e-5, and the share of exempted pairs stays <= 10 % (the fixtures sit at 0 % and 3.1 %:
    tests/test_topk_inputs.py).
(4) Allowed lists with k above (padding) and below n_allowed; the e4m3 and MXFP4 heads against their own dequantised logits under the
    bound tests/test_scores_e2e_gpu.py uses; the agents' last_top_*; the switch rules.
(5) Switch pairs: tests/switches_ref.py may not change here, so svln_top_logprobs has no row in its pair table.  As the stand-in every
    existing row is switched on together with k = 4 on a tiny engine and the documented outcome asserted: the refusal by name, or both
    in force."""
import ctypes as C

import numpy as np
import pytest
import torch

import mxfp4_ref as MX
import switch_probe as SP
import switches_ref as SW
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame

pytestmark = pytest.mark.gpu
LSE_TOL = 2e-5


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
    w = torch.from_numpy(m.get_tensor("lm_head.weight")).float()
    if mode == "fp8":
        w = O.qdq_e4m3_rows(w)
    elif mode == "mxfp4":
        w = MX.qdq_mxfp4(w).float()
    return w.double()


def _ids(log):
    return [r["out"].sequences[0].tolist() for r in log]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _shape_and_entry0(out, k, greedy=True):
    seq, lp = out.sequences, out.token_logprobs
    ti, tl = out.top_token_ids, out.top_logprobs
    n = seq.shape[1]
    assert ti.dtype == torch.int64 and tl.dtype == torch.float32 and tuple(ti.shape) == (1, n, k) == tuple(tl.shape)
    assert ti.device == seq.device and tl.device == seq.device
    if greedy:
        assert torch.equal(ti[..., 0], seq), (ti[..., 0], seq)
        assert torch.equal(_bits(tl[..., 0]), _bits(lp)), (tl[..., 0], lp)
    else:
        for j in range(n):
            hit = (ti[0, j] == seq[0, j]).nonzero()
            if len(hit):
                assert torch.equal(_bits(tl[0, j, hit[0, 0]]), _bits(lp[0, j])), (j, tl[0, j], lp[0, j])
    # order: log-probability descending, then id ascending; padding (-1, -inf) last
    for j in range(n):
        ids, lps = ti[0, j].tolist(), tl[0, j].tolist()
        live = [x for x in ids if x >= 0]
        assert ids == live + [-1] * (k - len(live)) and all(v == float("-inf") for v in lps[len(live):]) and len(set(live)) == len(live)
        assert all(a > b or (a == b and i < i2) for a, b, i, i2 in zip(lps, lps[1:len(live)], ids, ids[1:len(live)])), (j, ids, lps)


def _check_lists(Wd, out, hidden, penalty, k, what, stats):
    """(3) of the module docstring on one turn"""
    ids = out.sequences[0].tolist()
    K = Wd.shape[1]
    gamma = K * 2.0 ** -24
    for j, tok in enumerate(ids[:len(hidden)]):
        h = torch.from_numpy(np.asarray(hidden[j], dtype=np.float64))
        y = Wd @ h
        if penalty != 1.0 and j:
            seen = torch.tensor(sorted(set(ids[:j])), dtype=torch.long)
            y[seen] = torch.where(y[seen] < 0, y[seen] * penalty, y[seen] / penalty)
        bound = 2 * gamma * float((Wd.abs() @ h.abs()).max())
        lse = float(torch.logsumexp(y, 0))
        order = sorted(range(y.numel()), key=lambda n: (-float(y[n]), n))[:k + 1]
        gaps = [float(y[a] - y[b]) for a, b in zip(order, order[1:])]
        got_i, got_l = out.top_token_ids[0, j].tolist(), out.top_logprobs[0, j].tolist()
        # positions joined by gaps at or under the bound form runs inside which any order is allowed; the last run may reach rank k + 1
        stats["pairs"] += k
        stats["exempt"] += sum(g <= bound for g in gaps)
        p = 0
        while p < k:
            q = p
            while q < k and gaps[q] <= bound:
                q += 1
            run = set(order[p:q + 1])                       # ranks p .. q (q == k: the run crosses the list's end)
            got = got_i[p:min(q + 1, k)]
            assert set(got) <= run and len(set(got)) == len(got), (what, j, p, q, got_i, order, gaps, bound)
            if q < k:
                assert set(got) == run, (what, j, p, q, got_i, order)
            p = q + 1
        for n, lp in zip(got_i, got_l):
            assert abs(lp - (float(y[n]) - lse)) <= bound + LSE_TOL, (what, j, n, lp, float(y[n]) - lse, bound)


# ------------------------------------------------------------------------------------------------------------ (1) (2) (3)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_generate_k_on_equals_k_off_and_lists_match_the_head(name, dtype):
    sc = SCENARIOS[name]
    m = _model(sc, dtype)
    m.set_token_scores(True)
    log0, taps0 = _episode(m, sc)
    assert all(r["out"].top_token_ids is None and r["out"].top_logprobs is None and "top_logprobs" not in r["out"] for r in log0)
    Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
    stats = {"pairs": 0, "exempt": 0}
    for k, graph in ((8, True), (4, False), (1, True)):
        m.set_decode_graph(graph)
        m.set_top_logprobs(k)
        assert m.top_logprobs_k == k
        m.reset(1)
        log1, taps1 = _episode(m, sc)
        assert _ids(log1) == _ids(log0), k
        for a, b, r0, r1 in zip(taps0, taps1, log0, log1):
            assert np.array_equal(a["hidden"], b["hidden"]) and a["cache_len"] == b["cache_len"]
            assert torch.equal(_bits(r0["out"].token_logprobs), _bits(r1["out"].token_logprobs))
            _shape_and_entry0(r1["out"], k)
        if k == 8 and dtype == torch.float32:
            for t, (r, tp) in enumerate(zip(log1, taps1)):
                _check_lists(Wd, r["out"], tp["hidden"], pen, k, (name, t), stats)
            share = stats["exempt"] / stats["pairs"]
            print(f"{name}: {stats['exempt']} of {stats['pairs']} adjacent pairs at or under the a-priori bound ({100 * share:.1f} %)")
            assert share <= 0.10, stats
    # off after on: the run never-on, and the getter is refused
    m.set_decode_graph(True)
    m.set_top_logprobs(0)
    m.reset(1)
    log2, taps2 = _episode(m, sc)
    assert _ids(log2) == _ids(log0) and all(r["out"].top_token_ids is None for r in log2)
    for a, b, r0, r2 in zip(taps0, taps2, log0, log2):
        assert np.array_equal(a["hidden"], b["hidden"]) and torch.equal(_bits(r0["out"].token_logprobs), _bits(r2["out"].token_logprobs))
    ids, lps, nr, nk = (C.c_int32 * 64)(), (C.c_float * 64)(), C.c_int32(), C.c_int32()
    assert m._lib.svln_get_topk(m._h, ids, lps, 8, C.byref(nr), C.byref(nk)) != 0 and b"svln_top_logprobs" in m._lib.svln_last_error()
    m.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sampled_turns_list_the_unperturbed_distribution(dtype):
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, dtype)
    m.set_token_scores(True)
    m.set_sampling(0.8, 77)
    log0, taps0 = _episode(m, sc, steps=8)
    m.set_top_logprobs(5)
    m.set_sampling(0.8, 77)                                 # (restarts the draw counters: the same noise again)
    m.reset(1)
    log1, taps1 = _episode(m, sc, steps=8)
    assert _ids(log1) == _ids(log0)
    listed = differs = 0
    for a, b, r0, r1 in zip(taps0, taps1, log0, log1):
        assert np.array_equal(a["hidden"], b["hidden"]) and torch.equal(_bits(r0["out"].token_logprobs), _bits(r1["out"].token_logprobs))
        _shape_and_entry0(r1["out"], 5, greedy=False)
        o = r1["out"]
        listed += int((o.top_token_ids[0] == o.sequences[0][:, None]).any(1).sum())
        differs += int((o.top_token_ids[0, :, 0] != o.sequences[0]).sum())
    print(f"sampled {dtype}: {listed} emitted ids listed, {differs} differ from entry 0")
    assert listed >= 1
    m.close()


def test_allowed_list_pads_and_truncates():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.float32)
    m.set_token_scores(True)
    base = sorted({i for r in _episode(m, sc, steps=4)[0] for i in r["out"].sequences[0].tolist()})
    allowed = sorted(set(base) | {1, 2, 3})[:6]
    m.set_allowed_tokens(allowed, add_eos=False)
    for k in (8, 3):
        m.set_top_logprobs(k)
        m.reset(1)
        log, _ = _episode(m, sc, steps=4)
        for r in log:
            o = r["out"]
            _shape_and_entry0(o, k)
            n_live = min(k, len(allowed))
            assert bool((o.top_token_ids[0, :, :n_live] >= 0).all()) and bool((o.top_token_ids[0, :, n_live:] == -1).all())
            assert set(o.top_token_ids[0, :, :n_live].reshape(-1).tolist()) <= set(allowed)
            # the list is the allowed distribution's own top: same bits as allowed_logprobs at the listed ids
            alp, aid = o.allowed_logprobs[0], o.allowed_token_ids.tolist()
            for j in range(o.sequences.shape[1]):
                want = sorted(range(len(aid)), key=lambda q: (-float(alp[j, q]), aid[q]))[:n_live]
                assert o.top_token_ids[0, j, :n_live].tolist() == [aid[q] for q in want]
                assert np.allclose(o.top_logprobs[0, j, :n_live].cpu().numpy(), alp[j, want].cpu().numpy(), atol=LSE_TOL, rtol=0)
    m.close()


@pytest.mark.parametrize("mode", ["fp8", "mxfp4"])
def test_quantised_lm_heads_list_their_own_logits(mode):
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    m = _model(sc, torch.bfloat16)
    (m.set_fp8_decode if mode == "fp8" else m.set_mxfp4_decode)(True)
    m.set_token_scores(True)
    log0, taps0 = _episode(m, sc, steps=8)
    m.set_top_logprobs(8)
    m.reset(1)
    log1, taps1 = _episode(m, sc, steps=8)
    assert _ids(log1) == _ids(log0)
    Wd = _head(m, mode)
    gamma = Wd.shape[1] * 2.0 ** -24
    for r0, r1, tp in zip(log0, log1, taps1):
        o = r1["out"]
        assert torch.equal(_bits(r0["out"].token_logprobs), _bits(o.token_logprobs))
        _shape_and_entry0(o, 8)
        for j in range(min(o.sequences.shape[1], len(tp["hidden"]))):
            h = torch.from_numpy(np.asarray(tp["hidden"][j], dtype=np.float64))
            y = Wd @ h
            bound = 2 * gamma * float((Wd.abs() @ h.abs()).max()) + LSE_TOL
            lse = float(torch.logsumexp(y, 0))
            for n, lp in zip(o.top_token_ids[0, j].tolist(), o.top_logprobs[0, j].tolist()):
                assert abs(lp - (float(y[n]) - lse)) <= bound, (mode, j, n, lp, float(y[n]) - lse, bound)
    m.close()


# ------------------------------------------------------------------------------------------------------------ agents, switch rules
def _agent(m, sc, e=0):
    enc = SyntheticPromptEncoder(sc["cfg"], seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
    return StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                          device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc),
                          preprocess=m.get_vision_tower().image_processor.preprocess_array)


def test_agent_keeps_the_last_lists():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16)
    ag = _agent(m, sc)
    ag.act(synthetic_frame(0, 0))
    assert ag.last_top_token_ids is None and ag.last_top_logprobs is None
    m.set_token_scores(True)
    m.set_top_logprobs(3)
    ag.reset_memory()
    step = 0
    while not ag.turn_log or "top_logprobs" not in ag.turn_log[-1]["out"]:
        ag.act(synthetic_frame(0, step))
        step += 1
    out = ag.turn_log[-1]["out"]
    assert torch.equal(ag.last_top_token_ids, out.top_token_ids) and torch.equal(ag.last_top_logprobs, out.top_logprobs)
    assert tuple(ag.last_top_logprobs.shape) == (1, out.sequences.shape[1], 3)
    ag.reset_memory()
    assert ag.last_top_token_ids is None and ag.last_top_logprobs is None
    m.close()


def test_switch_rules():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16, envs=2, frames=6)
    L, h = m._lib, m._h
    err = lambda: L.svln_last_error()
    # needs the scores, which then stay on
    with pytest.raises(_lib.SvlnError, match="svln_set_token_scores"):
        m.set_top_logprobs(4)
    m.set_top_logprobs(0)                                   # a call that changes nothing succeeds
    m.set_token_scores(True)
    for k in (-1, 9):
        with pytest.raises(_lib.SvlnError, match=r"\.\. 8"):
            m.set_top_logprobs(k)
    m.set_top_logprobs(4)
    m.set_top_logprobs(4)
    with pytest.raises(_lib.SvlnError, match="svln_top_logprobs"):
        m.set_token_scores(False)
    m.set_token_scores(True)                                # nothing changes: succeeds
    # group turns carry no lists: refused by name, before any state change
    ags = [_agent(m, sc, e) for e in range(2)]
    for e, a in enumerate(ags):
        a.observe(synthetic_frame(e, 0))
    reqs = [a._build_request("") for a in ags]
    state = [m.env_state(e) for e in range(2)]
    eos, out = (C.c_int64 * 1)(2), (C.c_int64 * 16)()
    assert L.svln_generate_group(h, 0, 2, 4, eos, 1, out, 8, (C.c_int32 * 2)()) != 0 and b"svln_top_logprobs" in err()
    assert [m.env_state(e) for e in range(2)] == state
    # a single-env turn, then a forced turn: it runs as before, carries no lists, and the getter is refused after it
    o = m.generate(**reqs[0])
    _shape_and_entry0(o, 4)
    ids, lps, nr, nk = (C.c_int32 * 256)(), (C.c_float * 256)(), C.c_int32(), C.c_int32()
    assert L.svln_get_topk(h, ids, lps, 32, C.byref(nr), C.byref(nk)) == 0 and (nr.value, nk.value) == (o.sequences.shape[1], 4)
    assert [ids[j] for j in range(nr.value * 4)] == o.top_token_ids.reshape(-1).tolist()
    assert L.svln_get_topk(h, None, lps, 32, C.byref(nr), C.byref(nk)) != 0 and L.svln_get_topk(h, ids, lps, 32, None, C.byref(nk)) != 0
    ags[0]._consume(o)
    ags[0].observe(synthetic_frame(0, 1))
    f = m.generate(**ags[0]._build_request(""), forced_ids=list(SW.FORCED_IDS))
    assert f.top_token_ids is None and "top_logprobs" not in f
    assert L.svln_get_topk(h, ids, lps, 32, C.byref(nr), C.byref(nk)) != 0 and b"forced" in err()
    # a change while scheduler turns are in flight; the batched getters of turns that ran with k = 0
    m.set_top_logprobs(0)
    ticket = m.submit(**reqs[1])
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_top_logprobs(4)
    fin, _ = m.step_batch()
    while not fin:
        fin, _ = m.step_batch()
    assert fin[0][1].top_token_ids is None
    assert L.svln_generate_batch_topk(h, 0, ids, lps, 32, C.byref(nr), C.byref(nk)) != 0 and b"svln_top_logprobs" in err()
    m.set_top_logprobs(4)
    ags[1]._consume(fin[0][1])
    ags[1].observe(synthetic_frame(1, 1))
    t1 = m.submit(**ags[1]._build_request(""))
    assert L.svln_batch_topk(h, t1.slot, ids, lps, 32, C.byref(nr), C.byref(nk)) != 0            # not finished yet
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_top_logprobs(0)
    fin, _ = m.step_batch()
    while not fin:
        fin, _ = m.step_batch()
    _shape_and_entry0(fin[0][1], 4)
    assert L.svln_batch_topk(h, t1.slot, ids, lps, 32, C.byref(nr), C.byref(nk)) != 0            # svln_batch_result freed the slot
    m.close()


# ------------------------------------------------------------------------------------------------------------ several envs
def _agents(m, sc, N):
    return [_agent(m, sc, e) for e in range(N)]


def _lockstep(m, sc, N, steps):
    m.reset(N)
    agents = _agents(m, sc, N)
    group = BatchedAgents(agents)
    hidden, tops = [[] for _ in range(N)], [[] for _ in range(N)]
    for step in range(steps):
        n0 = len(agents[0].turn_log)
        group.act([synthetic_frame(e, step) for e in range(N)])
        if len(agents[0].turn_log) > n0:
            for e in range(N):
                hidden[e].append(m.last_hidden_batch(e))
                tops[e].append((agents[e].last_top_token_ids, agents[e].last_top_logprobs))
    return agents, hidden, tops


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,name", [(8, "tiny_episode"), (2, "tiny_penalty")])
def test_generate_batch_k_on_equals_k_off(N, name, dtype):
    """8 lockstep envs go through the MFMA head, 2 envs through the batched GEMV (there with the repetition penalty: row b's own flag
    row); through a window restart; BatchedAgents keep every env's lists; on the fp32 engine every list is checked against float64"""
    sc = SCENARIOS[name]
    m = _model(sc, dtype, envs=N, frames=3 * N)
    m.set_token_scores(True)
    steps = 16
    a0, h0, t0 = _lockstep(m, sc, N, steps)
    assert all(t == (None, None) for e in range(N) for t in t0[e])
    m.set_top_logprobs(8)
    a1, h1, t1 = _lockstep(m, sc, N, steps)
    Wd, pen = _head(m), sc.get("rep_penalty", 1.0)
    stats = {"pairs": 0, "exempt": 0}
    assert any(r["memory"] for r in a1[0].turn_log)
    for e in range(N):
        assert _ids(a1[e].turn_log) == _ids(a0[e].turn_log), e
        for t, (r0, r1) in enumerate(zip(a0[e].turn_log, a1[e].turn_log)):
            assert np.array_equal(h0[e][t], h1[e][t]) and r0["out"].past_key_values.get_seq_length() == r1["out"].past_key_values.get_seq_length()
            assert torch.equal(_bits(r0["out"].token_logprobs), _bits(r1["out"].token_logprobs)) and r0["out"].top_token_ids is None
            _shape_and_entry0(r1["out"], 8)
            assert torch.equal(t1[e][t][0], r1["out"].top_token_ids) and torch.equal(t1[e][t][1], r1["out"].top_logprobs)
            if dtype == torch.float32:
                _check_lists(Wd, r1["out"], h1[e][t], pen, 8, (N, name, e, t), stats)
    if dtype == torch.float32:
        assert stats["exempt"] <= 0.10 * stats["pairs"], stats
    # the getter of the last svln_generate_batch serves every listed env
    ids, lps, nr, nk = (C.c_int32 * 512)(), (C.c_float * 512)(), C.c_int32(), C.c_int32()
    for e in range(N):
        o = a1[e].turn_log[-1]["out"]
        assert m._lib.svln_generate_batch_topk(m._h, e, ids, lps, 64, C.byref(nr), C.byref(nk)) == 0 and (nr.value, nk.value) == (o.sequences.shape[1], 8)
        assert [ids[j] for j in range(nr.value * 8)] == o.top_token_ids.reshape(-1).tolist()
    assert m._lib.svln_generate_batch_topk(m._h, N, ids, lps, 64, C.byref(nr), C.byref(nk)) != 0
    m.set_top_logprobs(0)
    a2, h2, _ = _lockstep(m, sc, N, 8)
    for e in range(N):
        assert _ids(a2[e].turn_log) == _ids(a0[e].turn_log)[:len(a2[e].turn_log)] and all(r["out"].top_token_ids is None for r in a2[e].turn_log)
    m.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_scheduler_k_on_equals_k_off(dtype):
    """4 envs whose turns fall due at different times: prefilling and decoding envs share passes, the head rows of an iteration change
    in number from pass to pass (row tok0 + b of the lists beside the scores)"""
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
        group = AsyncBatchedAgents(agents, on_result=lambda i, ticket, out: hidden[i].append(m.last_hidden_batch(ticket.slot)))
        for tick in range(24):
            group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active={i for i in range(N) if tick >= i})
        return agents, hidden, group.stats

    a0, h0, _ = run()
    m.set_top_logprobs(5)
    a1, h1, st = run()
    assert st["mixed_iterations"] >= 2, st
    Wd = _head(m)
    stats = {"pairs": 0, "exempt": 0}
    for e in range(N):
        assert _ids(a1[e].turn_log) == _ids(a0[e].turn_log) and len(a1[e].turn_log) >= 3, e
        for t, (r0, r1) in enumerate(zip(a0[e].turn_log, a1[e].turn_log)):
            assert np.array_equal(h0[e][t], h1[e][t]) and torch.equal(_bits(r0["out"].token_logprobs), _bits(r1["out"].token_logprobs))
            assert r0["out"].past_key_values.get_seq_length() == r1["out"].past_key_values.get_seq_length()
            _shape_and_entry0(r1["out"], 5)
            if dtype == torch.float32:
                _check_lists(Wd, r1["out"], h1[e][t], 1.0, 5, ("scheduler", e, t), stats)
        assert torch.equal(a1[e].last_top_token_ids, a1[e].turn_log[-1]["out"].top_token_ids)
    m.close()


@pytest.mark.parametrize("row", SW.ROWS, ids=lambda r: r.name)
def test_every_switch_row_with_k_on(row):
    """the stand-in for the pair-table row this switch cannot have (module docstring, (5))"""
    m = SP.make_model()                                     # the pair test's own engine: bf16, 4 envs, the probe's sampling seed
    ag = SP._agent(m, 0, sampled=row.name == "sampling")
    ag.observe(synthetic_frame(0, 0))
    req = ag._build_request("")
    refused_by_scores = row.name in SW.PLAIN_HEAD
    if row.name == "token_scores":
        row.on(m)
        m.set_top_logprobs(4)
        with pytest.raises(_lib.SvlnError, match="svln_top_logprobs"):
            row.off(m)
    elif refused_by_scores:
        # unreachable together: the scores refuse the row both ways, and k > 0 needs the scores
        row.on(m)
        with pytest.raises(_lib.SvlnError, match=row.c_name):
            m.set_token_scores(True)
        with pytest.raises(_lib.SvlnError, match="svln_set_token_scores"):
            m.set_top_logprobs(4)
        row.off(m)
        m.set_token_scores(True)
        m.set_top_logprobs(4)
        with pytest.raises(_lib.SvlnError, match="svln_set_token_scores"):
            row.on(m)
    elif row.name == "generate_group":
        m.set_token_scores(True)
        m.set_top_logprobs(4)
        with pytest.raises(_lib.SvlnError, match="svln_top_logprobs"):
            m.generate(**dict(req, do_sample=True, num_return_sequences=2))
    elif row.name == "generate_forced":
        m.set_token_scores(True)
        m.set_top_logprobs(4)
        f = m.generate(**req, forced_ids=list(SW.FORCED_IDS))
        assert f.sequences[0].tolist() == list(SW.FORCED_IDS) and f.top_token_ids is None
    else:
        # composes: both stay in force -- the row switches on in either order and a turn carries its lists
        row.on(m)
        m.set_token_scores(True)
        m.set_top_logprobs(4)
        row.off(m)
        row.on(m)
        o = m.generate(**req)
        _shape_and_entry0(o, 4, greedy=row.name != "sampling")
        if row.name == "allowed_tokens":
            assert set(o.top_token_ids.reshape(-1).tolist()) <= set(SW.ALLOWED_IDS)
        if row.name == "sampling":
            assert m._sampling == SW.SAMPLING
    m.close()
