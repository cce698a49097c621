"""Group sampling end to end on the GPU (svln_generate_group / svln_turn_group / svln_group_select; generate(do_sample=True,
num_return_sequences=G) + select_sequence), TINY engines, fp32 unless said.

(a) prompt rows: after a group turn, and after a select of the last index, every K / V row of the positions < L is bit-equal -- in every
    layer -- to a twin engine's after a plain sampled svln_generate of the same turn; L % 64 = 0, 1, 61, 63 at max_new = 5.
(b) near-greedy temperature 2^-14: all G sequences are the greedy fixture's ids; after select_sequence(G - 1) the episode continues on
    the fork's pages through the fixture's turns: ids, hidden rows (<= 1e-3), cache lengths.  G = 2, 4, 8 and 3 (padded to 4).
(c) T = 1: every token of every sequence equals the float64 restatement argmax_n(l_n + G(seed, stream_g, draw, n)) from the engine's own
    tap row wherever the perturbed margin exceeds the a-priori dot bound of tests/test_sample_e2e_gpu.py; at most 10 % of the compared
    tokens may sit under it.  Every turn of the episode is a group turn, so the draws of turn n + 1 start where the longest sequence of
    turn n ended (f: no (stream, draw) pair repeats -- a wrong counter would restate other tokens).  Sequence 0 is checked with the env's
    own stream, as a twin engine's plain sampled generate of the same turn is.
(d) scores: every token_logprobs entry within dot + 2e-5 (the bound of tests/test_scores_e2e_gpu.py) of float64 log softmax from the tap
    row; with a list set, every allowed_logprobs row too.
(e) after a T = 1 group turn and select_sequence(g), g = 0 and G - 1, the oracle is teacher-forced with the selected ids; the next two
    greedy turns give the oracle's ids and hidden rows within 1e-3.
(f) the same seed reproduces all G sequences, another seed changes some.
(g) pool accounting on a pool the G = 8 fork fills to the last page: 20 consecutive group turns (select / drop by reset) leak nothing -- a
    lost page would refuse the next turn -- and which pages are held follows tests/group_ref.py.
(h) bf16 engine, G = 8 at T = 2^-14 against the greedy run inside the bounds of test_batched_lockstep_envs_equal_solo_runs.
(i) every refusal; each leaves the engine usable and no group pending."""
import ctypes as C

import numpy as np
import pytest
import torch

import group_ref as GR
import sample_ref as R
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, eos_ids
from streamvln_amd import _lib
from streamvln_amd import weights as W
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.config import TINY
from streamvln_amd.model import GenerateOutput, StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from util import load_golden

pytestmark = pytest.mark.gpu
LSE_TOL, HIDDEN_TOL = 2e-5, 1e-3
PI32, PI64, PF = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)


def _model(dtype=torch.float32, envs=1, max_positions=2048):
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=envs, max_frames=1 + sc["num_history"], max_positions=max_positions)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    return m


class GroupAgent(StreamingAgent):
    """a StreamingAgent whose turn t runs as a group turn when plan(t) gives (G, temperature, picked index); the agent goes on with the
    picked sequence.  group_log[t] keeps the whole result, the tap rows of every sequence and the env's cache length after the select."""

    def __init__(self, *a, plan=None, **k):
        self.plan, self.group_log = plan or (lambda t: None), {}
        super().__init__(*a, **k)

    def _turn(self, instruction, env_id=None):
        t = len(self.turn_log)
        spec = self.plan(t)
        if spec is None:
            return super()._turn(instruction, env_id)
        G, T, pick = spec
        m = self.model
        out = m.generate(**dict(self._build_request(instruction, env_id), do_sample=True, temperature=T, num_return_sequences=G))
        taps = [m.last_hidden_group(g) for g in range(G)]
        n = int(out.sequence_lengths[pick])
        kv = m.select_sequence(pick, self.env_id)
        self.group_log[t] = dict(out=out, taps=taps, cache_len=m.env_state(self.env_id)[1])
        return self._consume(GenerateOutput(sequences=out.sequences[pick:pick + 1, :n].clone(), past_key_values=kv))


def _agent(m, plan=None, cls=GroupAgent, device="cuda", preprocess=None):
    sc = SCENARIOS["tiny_episode"]
    enc = SyntheticPromptEncoder(sc["cfg"], seed=7, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
    kw = dict(plan=plan) if cls is GroupAgent else {}
    return cls(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=0, device=device,
               max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc),
               preprocess=preprocess or m.get_vision_tower().image_processor.preprocess_array, **kw)


def _run(ag, m, steps):
    """env steps; after every model turn: (hidden rows of a plain turn or None, cache length)"""
    seen = []
    for step in range(steps):
        n0 = len(ag.turn_log)
        ag.act(synthetic_frame(0, step))
        if len(ag.turn_log) > n0:
            t = n0
            seen.append((None if t in ag.group_log else m.last_hidden(), m.env_state(0)[1]))
    return seen


def _restate(Wd, ids, hidden, T, seed, stream, draw0, stats, what, logprobs=None, allowed=None, dist=None):
    """tokens (where the margin allows) and scores of one sampled sequence against float64 from its tap rows (the rule of
    tests/test_sample_e2e_gpu.py::_check_turn; `allowed`: the ids of the set the head ran over)"""
    K = Wd.shape[1]
    cols = np.arange(Wd.shape[0]) if allowed is None else np.asarray(allowed)
    Ws = Wd[cols]
    gamma, inv_t = K * 2.0 ** -24, float(np.float32(1.0) / np.float32(T))
    for k, tok in enumerate(ids[:len(hidden)]):
        h = np.asarray(hidden[k], dtype=np.float64)
        y = (Ws @ h) * inv_t
        dot = 2 * gamma * float((np.abs(Ws) @ np.abs(h)).max()) * inv_t
        g = R.gumbel(seed, stream, draw0 + k, cols)
        z = y + g
        a = int(np.argmax(z))
        zb, gb = np.delete(z, a), np.delete(g, a)
        b = int(np.argmax(zb))
        tol = 2.0 ** -17 * max(1.0, abs(g[a]), abs(gb[b])) + 2.0 ** -22 * float(np.abs(z).max())
        stats["tokens"] += 1
        if z[a] - zb[b] > 2 * dot + tol:
            assert tok == int(cols[a]), (what, k, tok, int(cols[a]), float(z[a] - zb[b]), dot, tol)
        else:
            stats["under"] += 1
        lsm = y - (y.max() + np.log(np.exp(y - y.max()).sum()))
        if logprobs is not None:
            assert tok in cols, (what, k, tok)
            err = abs(float(logprobs[k]) - float(lsm[int(np.searchsorted(cols, tok))]))
            stats["score"] = max(stats["score"], err / (dot + LSE_TOL))
            assert err <= dot + LSE_TOL, (what, k, float(logprobs[k]), dot)
        if dist is not None:
            err = float(np.abs(np.asarray(dist[k], dtype=np.float64) - lsm).max())
            stats["dist"] = max(stats.get("dist", 0.0), err / (dot + LSE_TOL))
            assert err <= dot + LSE_TOL, (what, k, err, dot)


# ------------------------------------------------------------------------------------------------------------ (a) prompt rows, (g), (i): C entry points
def _text_turn(m, L, env=0):
    ids = (np.arange(L, dtype=np.int64) * 37 + 11) % TINY.vocab
    assert m._lib.svln_append_turn(m._h, env, ids.ctypes.data_as(PI64), L, 0) == 0, m._lib.svln_last_error()


def _group(m, G, max_new, env=0, eos=()):
    out, n = np.zeros((G, max_new), dtype=np.int64), np.zeros(8, dtype=np.int32)
    e = np.asarray(eos, dtype=np.int64)
    rc = m._lib.svln_generate_group(m._h, env, G, max_new, e.ctypes.data_as(PI64), len(eos), out.ctypes.data_as(PI64), max_new, n.ctypes.data_as(PI32))
    return rc, out, n[:G]


def _plain(m, max_new, env=0):
    out, n = np.zeros(max_new, dtype=np.int64), C.c_int32()
    rc = m._lib.svln_generate(m._h, env, max_new, None, 0, out.ctypes.data_as(PI64), max_new, C.byref(n))
    return rc, out[:n.value]


def _pool_rows(m, layer, pages, n):
    """K / V rows of the first n positions of a sequence whose table is `pages`, from the raw pools of `layer`"""
    k, v = np.zeros((len(pages) * 64, TINY.kv_heads, 128), np.float32), np.zeros((len(pages) * 64, TINY.kv_heads, 128), np.float32)
    for i, p in enumerate(pages):
        assert m._lib.svln_op_kv_pool_read(m._h, layer, p * 64, 64, k[i * 64:].ctypes.data_as(PF), v[i * 64:].ctypes.data_as(PF)) == 0
    return k[:n], v[:n]


@pytest.mark.parametrize("residue", [0, 1, 61, 63])
def test_prompt_rows_are_the_plain_turns_bits_before_and_after_a_select(residue):
    L, G, max_new, seed = 128 + residue, 4, 5, 99
    twin, m = _model(max_positions=1024), _model(max_positions=1024)
    for e in (twin, m):
        assert e._lib.svln_set_sampling(e._h, 1, 1.0, seed) == 0
        _text_turn(e, L)
    rc, ids_plain = _plain(twin, max_new)
    assert rc == 0 and len(ids_plain) == max_new
    pool = GR.Pool(1024 // 64, 1)
    tabs = [list(t) for t in pool.fork(0, L, max_new, G)]
    want = [_pool_rows(twin, layer, tabs[0], L) for layer in range(TINY.layers)]       # (the twin took the same pages: page 0 first)
    rc, out, n = _group(m, G, max_new)
    assert rc == 0 and n.tolist() == [max_new] * G, m._lib.svln_last_error()
    assert len({tuple(r) for r in out.tolist()}) > 1                                     # (T = 1 on random weights: the sequences differ)
    for g in range(G):                                                                   # every sequence's table sees the prompt's bits
        for layer in range(TINY.layers):
            k, v = _pool_rows(m, layer, tabs[g], L)
            assert np.array_equal(k, want[layer][0]) and np.array_equal(v, want[layer][1]), (residue, g, layer)
    kv = C.c_int32()
    assert m._lib.svln_group_select(m._h, 0, G - 1, C.byref(kv)) == 0 and kv.value == L + max_new - 1
    pool.select(G - 1, [max_new] * G)
    assert pool.env_pages[0] == tabs[G - 1]                                              # the env now reads through the fork's private pages
    for layer in range(TINY.layers):
        k, v = _pool_rows(m, layer, pool.env_pages[0], L)
        assert np.array_equal(k, want[layer][0]) and np.array_equal(v, want[layer][1]), (residue, "selected", layer)
    # the engine's own view of the env (layer 0 through its page table) agrees with the restated table
    k0, v0 = np.zeros((L, TINY.kv_heads, 128), np.float32), np.zeros((L, TINY.kv_heads, 128), np.float32)
    assert m._lib.svln_op_kv_read(m._h, 0, 0, L, k0.ctypes.data_as(PF), v0.ctypes.data_as(PF)) == 0
    assert np.array_equal(k0, want[0][0]) and np.array_equal(v0, want[0][1])
    ne, kl = C.c_int32(), C.c_int32()
    assert m._lib.svln_env_state(m._h, 0, C.byref(ne), C.byref(kl)) == 0 and (ne.value, kl.value) == (L, L + max_new - 1)
    twin.close()
    m.close()


# ------------------------------------------------------------------------------------------------------------ (b) near-greedy
@pytest.mark.parametrize("G", [2, 4, 8, 3])
def test_cold_group_reproduces_the_greedy_fixture_and_the_episode_continues_on_the_fork(G):
    g = load_golden("tiny_episode")
    m = _model()
    m.sampling_seed = 5
    steps = 36 if G == 8 else 20
    group_turns = {0: G, 2: G, 4: 2}                                   # turn 0 decodes five tokens; later turns continue on forked pages
    ag = _agent(m, plan=lambda t: (group_turns[t], 2.0 ** -14, group_turns[t] - 1) if t in group_turns else None)
    seen = _run(ag, m, steps)
    assert len(ag.turn_log) == steps // 4 and sorted(ag.group_log) == sorted(group_turns)
    for t, (r, (hid, cache_len)) in enumerate(zip(ag.turn_log, seen)):
        want = g[f"t{t}_ids"].tolist()
        assert r["out"].sequences[0].tolist() == want, (G, t)
        assert cache_len == int(g[f"t{t}_cache_len"]), (G, t)
        if t in ag.group_log:
            gl = ag.group_log[t]
            assert gl["out"].sequence_lengths.tolist() == [len(want)] * group_turns[t] and gl["out"].past_key_values is None
            for s in range(group_turns[t]):
                assert gl["out"].sequences[s].tolist() == want, (G, t, s)
                assert np.abs(gl["taps"][s] - g[f"t{t}_hidden"][:8]).max() <= HIDDEN_TOL, (G, t, s)
        else:
            assert np.abs(hid - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, (G, t)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (c) (d) (f) restatement at T = 1
def _sampled_episode(m, G, seed, steps, pick=lambda t, G: G - 1):
    m.reset(1)
    m.sampling_seed = seed
    m.set_sampling(1.0, seed)                                           # (restarts the draw counters)
    ag = _agent(m, plan=lambda t: (G, 1.0, pick(t, G)))
    _run(ag, m, steps)
    return ag


@pytest.mark.parametrize("G,allowed", [(8, False), (3, False), (4, True)], ids=["G8", "G3", "G4-allowed"])
def test_every_token_of_every_sequence_is_the_restated_sample_of_its_own_tap_row(G, allowed):
    seed, steps = GR.E2E_SEED, 24
    m = _model()
    m.set_token_scores(True)
    ids_set = None
    if allowed:
        m.generation_config.eos_token_id = list(eos_ids(SCENARIOS["tiny_episode"]))[:40]
        m.set_allowed_tokens(list(range(3, 4096, 41)))                 # 100 ids plus 40 EOS ids
        ids_set = list(m.allowed_token_ids)
    ag = _sampled_episode(m, G, seed, steps)
    Wd = m.get_tensor("lm_head.weight").astype(np.float64)
    stats, draw = dict(tokens=0, under=0, score=0.0), 0
    assert len(ag.group_log) == steps // 4
    for t in sorted(ag.group_log):
        out, taps = ag.group_log[t]["out"], ag.group_log[t]["taps"]
        lens = out.sequence_lengths.tolist()
        assert tuple(out.token_logprobs.shape) == tuple(out.sequences.shape) == (G, max(lens))
        for s in range(G):
            n = lens[s]
            assert len(taps[s]) == min(n, 8)
            assert float(out.token_logprobs[s, n:].abs().sum()) == 0.0           # padded with 0: the row sum is the joint log-probability
            _restate(Wd, out.sequences[s, :n].tolist(), taps[s], 1.0, seed, s * m.max_envs, draw, stats, (G, t, s),
                     logprobs=out.token_logprobs[s, :n].tolist(), allowed=ids_set,
                     dist=out.allowed_logprobs[s, :n].numpy() if allowed else None)
        if allowed:
            assert out.allowed_token_ids.tolist() == ids_set and tuple(out.allowed_logprobs.shape) == (G, max(lens), len(ids_set))
        else:
            assert "allowed_logprobs" not in out
        draw += max(lens)                                               # the engine's rule: the counter clears the longest sequence
    print(f"G={G} allowed={allowed}: {stats['under']} of {stats['tokens']} tokens under the margin; worst |score - ref| / bound = {stats['score']:.3f}"
          + (f", worst |dist - ref| / bound = {stats['dist']:.3f}" if allowed else ""))
    assert stats["tokens"] >= 6 * G and stats["under"] <= 0.10 * stats["tokens"], stats
    m.close()


def test_sequence_0_draws_from_the_envs_own_stream_like_a_plain_sampled_turn():
    """turn 0 of the episode on a twin engine through the plain sampled generate and as a group turn: both restate with stream 0, draws
    0 ..; where every margin of both is clear the ids are equal as a consequence"""
    seed = GR.E2E_SEED
    stats = dict(tokens=0, under=0, score=0.0)
    twin = _model()
    twin.sampling_seed = seed
    a = _agent(twin, cls=StreamingAgent)
    a.do_sample, a.temperature = True, 1.0
    a.act(synthetic_frame(0, 0))
    ids_plain, hid_plain = a.turn_log[0]["out"].sequences[0].tolist(), twin.last_hidden()
    Wd = twin.get_tensor("lm_head.weight").astype(np.float64)
    _restate(Wd, ids_plain, hid_plain, 1.0, seed, 0, 0, stats, "plain")
    twin.close()
    m = _model()
    ag = _sampled_episode(m, 4, seed, 1, pick=lambda t, G: 0)
    out = ag.group_log[0]["out"]
    ids0 = out.sequences[0, :int(out.sequence_lengths[0])].tolist()
    _restate(Wd, ids0, ag.group_log[0]["taps"][0], 1.0, seed, 0, 0, stats, "group seq 0")
    print(f"plain {ids_plain} group sequence 0 {ids0}; {stats['under']} of {stats['tokens']} under the margin")
    if stats["under"] == 0:
        assert ids0 == ids_plain
    m.close()


def test_seeds_reproduce_and_differ():
    m = _model()
    runs = [[ag.group_log[t]["out"].sequences.tolist() for t in sorted(ag.group_log)]
            for ag in (_sampled_episode(m, 8, sd, 12) for sd in (41, 41, 42))]
    assert runs[0] == runs[1] and runs[0] != runs[2]
    assert all(len({tuple(r) for r in turn}) > 1 for turn in runs[0])   # the streams of one turn are independent samples
    m.close()


# ------------------------------------------------------------------------------------------------------------ (e) the oracle goes on from the selected ids
@pytest.mark.parametrize("pick", ["first", "last"])
def test_selected_continuation_matches_the_teacher_forced_oracle(pick):
    sc, G, seed = SCENARIOS["tiny_episode"], 4, 321
    m = _model()
    m.sampling_seed = seed
    idx = 0 if pick == "first" else G - 1
    ag = _agent(m, plan=lambda t: (G, 1.0, idx) if t == 0 else None)
    seen = _run(ag, m, 12)                                             # the group turn, then two greedy turns
    gl = ag.group_log[0]
    chosen = ag.turn_log[0]["out"].sequences[0].tolist()
    assert chosen == gl["out"].sequences[idx, :len(chosen)].tolist() and len(ag.turn_log) == 3
    orc = O.OracleStreamVLN(sc["cfg"], W.synth_state_dict(sc["cfg"], SEED), num_history=sc["num_history"])
    orc.teacher_tokens = [chosen]
    pre = m.get_vision_tower().image_processor.preprocess_array
    oa = _agent(orc, cls=StreamingAgent, device="cpu", preprocess=lambda rgb: pre(rgb).cpu())
    cache_lens = []                                                     # (the oracle's cache object grows in place: read it turn by turn)
    for step in range(12):
        n0 = len(oa.turn_log)
        oa.act(synthetic_frame(0, step))
        if len(oa.turn_log) > n0:
            cache_lens.append(len(oa.turn_log[-1]["out"].past_key_values))
    assert oa.turn_log[0]["out"].sequences[0].tolist() == chosen
    assert np.abs(gl["taps"][idx] - oa.turn_log[0]["out"].hidden.numpy()[:8]).max() <= HIDDEN_TOL
    assert gl["cache_len"] == cache_lens[0]
    for t in (1, 2):
        assert ag.turn_log[t]["out"].sequences[0].tolist() == oa.turn_log[t]["out"].sequences[0].tolist(), (pick, t)
        assert np.abs(seen[t][0] - oa.turn_log[t]["out"].hidden.numpy()).max() <= HIDDEN_TOL, (pick, t)
        assert seen[t][1] == cache_lens[t], (pick, t)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (g) pool accounting
def _held(m, total):
    """pages an env or a pending group holds: svln_op_kv_page_copy refuses exactly those as a destination"""
    held = set()
    for p in range(total):
        dst = np.asarray([p], dtype=np.int32)
        if m._lib.svln_op_kv_page_copy(m._h, (p + 1) % total, dst.ctypes.data_as(PI32), 1) != 0:
            assert b"held by" in m._lib.svln_last_error()
            held.add(p)
    return held


def test_twenty_group_turns_on_an_exactly_full_pool_leak_no_page():
    L, G, max_new, total = 64 + 63, 8, 5, 17                            # 3 own pages + 7 forks x 2 tail pages = the whole pool
    m = _model(max_positions=total * 64)
    pool = GR.Pool(total, 1)
    assert m._lib.svln_set_sampling(m._h, 1, 1.0, 7) == 0
    ne, kl = C.c_int32(), C.c_int32()
    for it in range(20):
        _text_turn(m, L)
        assert pool.can_fork(0, L, max_new, G) and not pool.can_fork(0, L + 64, max_new, G)
        rc, out, n = _group(m, G, max_new, eos=eos_ids(SCENARIOS["tiny_episode"]))
        assert rc == 0, (it, m._lib.svln_last_error())                  # (a page lost by an earlier turn would refuse this one)
        pool.fork(0, L, max_new, G)
        assert len(pool.free) == 0
        if it % 5 == 0:
            assert _held(m, total) == set(range(total))
        choice = (None, G - 1, 0, 3)[it % 4]
        if choice is None:                                              # drop by reset
            assert m._lib.svln_reset_env(m._h, 0) == 0
            pool.reset_env(0)
            assert _held(m, total) == set() and len(pool.free) == total
            continue
        assert m._lib.svln_group_select(m._h, 0, choice, C.byref(kl)) == 0 and kl.value == L + int(n[choice]) - 1
        pool.select(choice, n.tolist())
        assert len(pool.free) == total - 3 and pool.conserved()
        assert _held(m, total) == set(pool.env_pages[0]), (it, choice)
        assert m._lib.svln_env_state(m._h, 0, C.byref(ne), C.byref(kl)) == 0 and (ne.value, kl.value) == (L, pool.kv_len[0])
        assert m._lib.svln_reset_env(m._h, 0) == 0
        pool.reset_env(0)
    # one position more needs an 18th page: refused before anything changes, as the restatement predicts
    _text_turn(m, L + 64)
    rc, _, _ = _group(m, G, max_new)
    assert rc != 0 and b"free KV pages" in m._lib.svln_last_error()
    rc, _, n = _group(m, G - 1, max_new)                                # 4 own + 6 x 2 = 16 pages fit
    assert rc == 0 and pool.can_fork(0, L + 64, max_new, G - 1)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (h) bf16
def test_bf16_cold_group_of_8_stays_inside_the_lockstep_bounds():
    m = _model(dtype=torch.bfloat16)
    greedy = _agent(m)
    ref = _run(greedy, m, 16)
    ref_ids = [r["out"].sequences[0].tolist() for r in greedy.turn_log]
    m.reset(1)
    m.sampling_seed = 5
    ag = _agent(m, plan=lambda t: (8, 2.0 ** -14, 7))
    _run(ag, m, 16)
    agree = total = 0
    for t in sorted(ag.group_log):
        if [r["out"].sequences[0].tolist() for r in ag.turn_log[:t]] != ref_ids[:t]:
            break                                                       # (a near-tie fell the other way: the later prompts differ)
        for s in range(8):
            total += 1
            agree += int(int(ag.group_log[t]["out"].sequences[s, 0]) == ref_ids[t][0])
            a, b = ag.group_log[t]["taps"][s][0], ref[t][0][0]
            assert np.linalg.norm(a - b) / np.linalg.norm(b) < 3e-2, (t, s)
    assert total >= 8 and agree >= total - 2, (agree, total)
    m.close()


# ------------------------------------------------------------------------------------------------------------ (i) refusals
def test_every_refusal_leaves_the_engine_usable_and_no_group_pending():
    m = _model(envs=2, max_positions=512)                               # 16 pages
    lib, h = m._lib, m._h
    err = lambda: lib.svln_last_error()
    buf, n, n2 = np.zeros(8 * 512, dtype=np.float32), C.c_int32(), C.c_int32()

    def no_group():
        assert lib.svln_group_select(h, 0, 0, None) != 0 and b"no group turn is pending" in err()
    _text_turn(m, 100)
    # sampling off; the group sizes; a penalty; positions; the pool
    rc, _, _ = _group(m, 4, 5)
    assert rc != 0 and b"svln_set_sampling" in err()
    assert lib.svln_set_sampling(h, 1, 1.0, 3) == 0
    for G in (1, 9, 0, -2):
        out = np.zeros((9, 5), dtype=np.int64)
        assert lib.svln_generate_group(h, 0, G, 5, None, 0, out.ctypes.data_as(PI64), 5, buf.ctypes.data_as(PI32)) != 0 and b"2 .. 8" in err()
    assert lib.svln_set_repetition_penalty(h, 1.3) == 0
    rc, _, _ = _group(m, 4, 5)
    assert rc != 0 and b"repetition penalty" in err()
    assert lib.svln_set_repetition_penalty(h, 1.0) == 0
    rc, _, _ = _group(m, 2, 414)                                        # 100 + 414 - 1 = 513 > 512
    assert rc != 0 and b"max_positions" in err()
    rc, _, _ = _group(m, 8, 200)                                        # tail of 3 pages x 7 forks + 5 own > 16
    assert rc != 0 and b"free KV pages" in err()
    no_group()
    # scheduler turns in flight
    _text_turn(m, 30, env=1)
    slot = C.c_int32()
    assert lib.svln_batch_submit(h, 1, 3, None, 0, C.byref(slot)) == 0
    rc, _, _ = _group(m, 4, 5)
    assert rc != 0 and b"in flight" in err()
    assert lib.svln_batch_cancel(h, -1) == 0
    no_group()
    ne, kl = C.c_int32(), C.c_int32()
    assert lib.svln_env_state(h, 0, C.byref(ne), C.byref(kl)) == 0 and (ne.value, kl.value) == (100, 0)      # nothing changed so far
    # a group turn, scores off: the score getters are refused, the tap is not
    rc, out, n_out = _group(m, 3, 5)
    assert rc == 0, err()
    assert lib.svln_group_logprobs(h, 0, buf.ctypes.data_as(PF), 8, C.byref(n)) != 0 and b"svln_set_token_scores" in err()
    assert lib.svln_group_dist(h, 0, buf.ctypes.data_as(PF), 8, C.byref(n), C.byref(n2)) != 0 and b"svln_set_allowed_tokens" in err()
    assert lib.svln_get_hidden_group(h, 2, buf.ctypes.data_as(PF), 8, C.byref(n)) == 0 and n.value == min(int(n_out[2]), 8)
    assert lib.svln_get_hidden_group(h, 3, buf.ctypes.data_as(PF), 8, C.byref(n)) != 0
    # while it is pending: every entry that would move the env is refused by name, the three switches too
    ids = np.asarray([5, 6, 7], dtype=np.int64)
    o64 = np.zeros(8, dtype=np.int64)
    calls = [lambda: lib.svln_append_turn(h, 0, ids.ctypes.data_as(PI64), 3, 0),
             lambda: lib.svln_append_turn_at(h, 0, ids.ctypes.data_as(PI64), 3, 0, 0),
             lambda: lib.svln_generate(h, 0, 4, None, 0, o64.ctypes.data_as(PI64), 8, C.byref(n)),
             lambda: lib.svln_generate_fixed(h, 0, 2, o64.ctypes.data_as(PI64)),
             lambda: lib.svln_batch_submit(h, 0, 3, None, 0, C.byref(slot)),
             lambda: lib.svln_generate_batch(h, np.asarray([0], dtype=np.int32).ctypes.data_as(PI32), 1, 3, None, 0, o64.ctypes.data_as(PI64), 8, C.byref(n)),
             lambda: lib.svln_generate_group(h, 0, 2, 3, None, 0, o64.ctypes.data_as(PI64), 4, buf.ctypes.data_as(PI32)),
             lambda: lib.svln_generate_group(h, 1, 2, 3, None, 0, o64.ctypes.data_as(PI64), 4, buf.ctypes.data_as(PI32))]
    for k, call in enumerate(calls):
        assert call() != 0 and b"svln_group_select" in err(), (k, err())
    ta = _lib.SvlnTurnArgs()
    ta.env, ta.ids, ta.n_ids, ta.max_new_tokens = 0, ids.ctypes.data, 3, 3
    assert lib.svln_turn(h, C.byref(ta), o64.ctypes.data_as(PI64), 8, C.byref(n), None) != 0 and b"svln_group_select" in err()
    assert lib.svln_turn_group(h, C.byref(ta), 2, o64.ctypes.data_as(PI64), 4, buf.ctypes.data_as(PI32)) != 0 and b"svln_group_select" in err()
    assert lib.svln_set_sampling(h, 0, 1.0, 0) != 0 and b"group turn is pending" in err()
    assert lib.svln_set_token_scores(h, 1) != 0 and b"group turn is pending" in err()
    assert lib.svln_set_allowed_tokens(h, ids.ctypes.data_as(PI64), 3) != 0 and b"group turn is pending" in err()
    assert lib.svln_group_select(h, 1, 0, None) != 0 and lib.svln_group_select(h, 0, 3, None) != 0 and lib.svln_group_select(h, 0, -1, None) != 0
    assert lib.svln_group_select(h, 0, 2, C.byref(kl)) == 0 and kl.value == 100 + int(n_out[2]) - 1
    no_group()
    # the env goes on: the next plain turn, then a group dropped by svln_kv_reset
    more = np.arange(int(n_out[2]) + 3, dtype=np.int64) + 20           # (the next prompt carries the chosen ids and new text)
    assert lib.svln_append_turn(h, 0, more.ctypes.data_as(PI64), len(more), 0) == 0 and calls[2]() == 0 and n.value >= 1, err()
    assert lib.svln_append_turn(h, 0, more.ctypes.data_as(PI64), 6, 0) == 0           # (more rows than the plain turn's 4 ids fed)
    rc, _, _ = _group(m, 2, 3)
    assert rc == 0, err()
    assert lib.svln_kv_reset(h, 0) == 0
    no_group()
    assert lib.svln_reset_env(h, 0) == 0 and lib.svln_reset_env(h, 1) == 0 and _held(m, 16) == set()
    # the Python surface
    m.reset(2)
    m.set_sampling(None)
    ag = _agent(m)
    ag.observe(synthetic_frame(0, 0))
    req = ag._build_request("")
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(**dict(req, do_sample=True, num_return_sequences=9))
    for call in (lambda r: m.generate_batch([r]), lambda r: m.submit(**r)):
        with pytest.raises(NotImplementedError, match="num_return_sequences"):
            call(dict(req, do_sample=True, num_return_sequences=2))
    assert m.env_state(0) == (0, 0)
    plain = m.generate(**dict(req, do_sample=False, num_return_sequences=4))           # greedy: the key stays unread
    assert tuple(plain.sequences.shape)[0] == 1 and "sequence_lengths" not in plain
    m.reset(2)
    out = m.generate(**dict(req, do_sample=True, num_return_sequences=2))
    assert tuple(out.sequences.shape)[0] == 2 and out.past_key_values is None
    with pytest.raises(RuntimeError, match="select_sequence"):
        m.generate(**req)
    m.reset_for_env(0)                                                  # drops the group
    with pytest.raises(RuntimeError, match="no group turn is pending"):
        m.select_sequence(0)
    out = m.generate(**dict(req, do_sample=True, num_return_sequences=2))
    kv = m.select_sequence(1)
    assert kv.get_seq_length() == m.env_state(0)[1] == m.env_state(0)[0] + int(out.sequence_lengths[1]) - 1
    m.close()
