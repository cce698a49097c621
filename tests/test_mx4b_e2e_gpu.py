"""svln_set_mxfp4_batched end to end (TINY; NO reference counterpart: the reference is bf16 only): the envs that generate_batch and the
scheduler carry, against the CPU restatement of the scheme (tests/mxfp4_ref.py Mxfp4Emu: prefill bf16, decode projections and every
lm_head product on the MXFP4 quantise -> dequantise of the weights).  Weight-only, so engine and emulation see the same operands:
every hidden row is held at the bf16 engine's own bound (test_fp8_gpu.W8_REL), ids wherever the emulation's top-2 margin exceeds
test_fp8_gpu.MARGIN.  Teacher-forced on the token level as tests/test_mxfp4_gpu.py: the engine runs first, each env's emulation then
decodes that env's ENGINE tokens, alone."""
import gc

import numpy as np
import pytest
import torch

import mxfp4_ref as R
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from test_e2e_gpu import _note
from test_fp8_gpu import MARGIN, W8_REL, _rel
from util import synth_weights

pytestmark = pytest.mark.gpu


def _model(sc, n_envs, dtype=torch.bfloat16):
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=n_envs, max_frames=3 * n_envs, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    apply_knobs(m, sc)
    return m


def _agents(model, sc, n_envs, preprocess, device):
    out = []
    for e in range(n_envs):
        enc = SyntheticPromptEncoder(sc["cfg"], seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        out.append(StreamingAgent(model, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                                  device=device, max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=preprocess))
    return out


def _lockstep(m, sc, n_envs, steps):
    """n_envs envs through generate_batch for `steps` env steps -> (ids [env][turn], hidden [env][turn])"""
    agents = _agents(m, sc, n_envs, m.get_vision_tower().image_processor.preprocess_array, "cuda")
    group = BatchedAgents(agents)
    hidden = [[] for _ in range(n_envs)]
    for step in range(steps):
        n0 = len(agents[0].turn_log)
        group.act([synthetic_frame(e, step) for e in range(n_envs)])
        if len(agents[0].turn_log) > n0:
            for e in range(n_envs):
                hidden[e].append(m.last_hidden_batch(e))
    ids = [[r["out"].sequences[0].tolist() for r in a.turn_log] for a in agents]
    return ids, hidden


def _emulate(sc, ids, lengths=None, knobs=False):
    """every env alone on Mxfp4Emu, decoding the engine's tokens of that env: [env][turn] -> (hidden, margins, own picks, cache_len)"""
    from concurrent.futures import ThreadPoolExecutor
    cfg = sc["cfg"]
    sd = synth_weights(cfg, SEED)
    shared = {}

    def solo(e):
        emu = R.Mxfp4Emu()
        emu._dq = shared
        orc = O.OracleStreamVLN(cfg, sd, num_history=sc["num_history"], fp8=emu)
        if knobs:
            apply_knobs(orc, sc)
        orc.teacher_tokens = [list(t) for t in ids[e]]
        enc = SyntheticPromptEncoder(cfg, seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        ag = StreamingAgent(orc, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"],
                            max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb)))
        if lengths is not None:
            ag.decode_actions = lambda _ids, ag=ag: [1] * lengths(e, len(ag.turn_log) - 1)
        while len(ag.turn_log) < len(ids[e]):
            ag.act(synthetic_frame(e, ag.step_id))
        assert not orc.teacher_tokens
        return [(r["out"].hidden.numpy().copy(), list(r["out"].margins), list(r["out"].own_picks), r["out"].cache_len) for r in ag.turn_log]
    with ThreadPoolExecutor(max_workers=min(len(ids), 8)) as ex:
        out = list(ex.map(solo, range(len(ids))))
    del shared
    gc.collect()
    return out


def _compare(what, cfg, ids, hidden, emu, bound):
    """every tapped row of every turn of every env under `bound`; ids wherever the emulation's margin exceeds MARGIN.
    -> decode rows compared per env"""
    worst, asserted, dec = 0.0, 0, [0] * len(ids)
    for e in range(len(ids)):
        for t, (gh, margins, picks, _) in enumerate(emu[e]):
            assert len(picks) == len(ids[e][t]), (what, e, t)
            for j in range(min(len(picks), len(hidden[e][t]))):
                rel = _rel(hidden[e][t][j], gh[j])
                worst = max(worst, rel)
                print(f"{what} env {e} turn {t} row {j}: rel L2 {rel:.5f} margin {margins[j]:.4f} engine id {ids[e][t][j]} emulation pick {picks[j]}")
                assert rel < bound, (what, e, t, j, rel, bound)
                dec[e] += j > 0
                if margins[j] > MARGIN:
                    assert ids[e][t][j] == picks[j], (what, e, t, j, ids[e][t], picks, margins)
                    asserted += 1
    line = (f"{cfg.name} batched MXFP4 weights [{what}] vs the emulating oracle (teacher-forced per env): decode rows per env {dec}, all rows < {bound}, "
            f"worst rel L2 {worst:.4f}; {asserted} ids with emulation margin > {MARGIN} asserted equal")
    print(line)
    _note("mxfp4_batched_vs_emulation", line)
    return dec


def test_eight_env_lockstep_vs_emulating_oracle():
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    m = _model(sc, 8)
    m.set_mxfp4_batched(True)
    ids, hidden = _lockstep(m, sc, 8, 12)
    m.close()
    assert [len(t) for t in ids] == [3] * 8
    dec = _compare("lockstep x8", sc["cfg"], ids, hidden, _emulate(sc, ids), W8_REL[sc["cfg"].name])
    assert min(dec) >= 8, dec


def test_ragged_scheduler_vs_emulating_oracle():
    """3 envs whose turns fall due in different iterations: with the switch on, an iteration that holds decode rows and prefill rows is
    split (decode rows on the MXFP4 step, prefill segments on a bf16 pass), and every env still computes what it computes alone"""
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    N = 3
    m = _model(sc, N)
    m.set_mxfp4_batched(True)
    lengths = lambda e, t: 2 if (e + t) % 2 == 0 else 4
    agents = _agents(m, sc, N, m.get_vision_tower().image_processor.preprocess_array, "cuda")
    for e, ag in enumerate(agents):
        ag.decode_actions = lambda _ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
    hidden = [[] for _ in range(N)]
    group = AsyncBatchedAgents(agents, on_result=lambda i, ticket, out: hidden[i].append(m.last_hidden_batch(ticket.slot)))
    for tick in range(40):
        group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active={i for i in range(N) if tick >= 2 * i})
        if tick == 0:                                            # env 0's turn is in flight: the mode cannot change under it, either way
            assert group.waiting
            with pytest.raises(_lib.SvlnError, match="in flight"):
                m.set_mxfp4_batched(False)
            m.set_mxfp4_batched(True)                            # (a call that changes nothing is accepted)
    st = group.stats
    m.close()
    assert st["mixed_iterations"] >= 1 and st["max_in_flight"] >= 2, st          # prefill and decode rows met in one iteration
    ids = [[r["out"].sequences[0].tolist() for r in a.turn_log] for a in agents]
    assert min(len(t) for t in ids) >= 2, [len(t) for t in ids]
    emu = _emulate(sc, ids, lengths)
    for e in range(N):
        for t, rec in enumerate(agents[e].turn_log):
            assert rec["out"].past_key_values.get_seq_length() == emu[e][t][3], (e, t)
    dec = _compare(f"ragged x{N} {st}", sc["cfg"], ids, hidden, emu, W8_REL[sc["cfg"].name])
    assert min(dec) >= 8, dec


def test_switch_semantics_exclusive_modes_and_bit_exact_return_to_bf16():
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    N = 4
    m = _model(sc, N)
    m.set_decode_graph(True)
    ids0, hid0 = _lockstep(m, sc, N, 8)                          # bf16, batched decode graph on, before the mode was ever enabled
    # mutual refusal with the two fp8 switches, each way round, with a message
    m.set_fp8_decode(True)
    with pytest.raises(_lib.SvlnError, match="svln_set_fp8_decode"):
        m.set_mxfp4_batched(True)
    m.set_fp8_decode(False)
    m.set_fp8_gemm(True)
    with pytest.raises(_lib.SvlnError, match="svln_set_fp8_gemm"):
        m.set_mxfp4_batched(True)
    m.set_fp8_gemm(False)
    m.set_mxfp4_batched(True)
    with pytest.raises(_lib.SvlnError, match="svln_set_mxfp4_batched"):
        m.set_fp8_decode(True)
    with pytest.raises(_lib.SvlnError, match="svln_set_mxfp4_batched"):
        m.set_fp8_gemm(True)
    m.set_mxfp4_decode(True)                                     # independent of the single-env switch: both may be on
    m.set_mxfp4_decode(False)
    m.set_mxfp4_batched(True)                                    # enabling twice is fine
    m.reset(N)
    ids1, hid1 = _lockstep(m, sc, N, 8)
    # the mode does something: decode rows differ from bf16 (row 0 of a turn is the prefill's last row through the bf16 products)
    assert any(not np.array_equal(a[1:], b[1:]) for e in range(N) for a, b in zip(hid0[e], hid1[e]) if len(a) == len(b))
    assert all(np.array_equal(hid0[e][0][0], hid1[e][0][0]) for e in range(N))   # ... and the first turn's prefill row does not
    m.set_mxfp4_batched(False)
    m.set_mxfp4_batched(False)                                   # and so is disabling twice
    m.reset(N)
    ids2, hid2 = _lockstep(m, sc, N, 8)
    assert ids2 == ids0
    for e in range(N):
        assert len(hid2[e]) == len(hid0[e]) == 2
        for a, b in zip(hid0[e], hid2[e]):
            assert np.array_equal(a, b)                          # bit for bit: the default path is unchanged, no stale graph is replayed
    m.close()
    m32 = _model(sc, 1, torch.float32)
    with pytest.raises(_lib.SvlnError, match="bf16"):
        m32.set_mxfp4_batched(True)
    m32.close()


def test_repetition_penalty_rides_on_the_batched_mxfp4_lm_head():
    """tiny_penalty (generation_config.repetition_penalty = 1.3) through generate_batch with the switch on: the flags are applied in the
    arg-max epilogue of gemv_mx4b_kernel; against Mxfp4Emu with the same knob, teacher-forced per env"""
    sc = SCENARIOS["tiny_penalty"]
    N = 2
    m = _model(sc, N)
    m.set_mxfp4_batched(True)
    ids, hidden = _lockstep(m, sc, N, sc["steps"])
    m.close()
    dec = _compare("tiny_penalty x2", sc["cfg"], ids, hidden, _emulate(sc, ids, knobs=True), W8_REL[sc["cfg"].name])
    assert min(dec) >= 8, dec
