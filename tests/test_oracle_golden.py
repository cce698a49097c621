"""CPU: the oracle (fp32 restatement) reproduces the fixtures generated from the REFERENCE's own modules
(oracle/make_golden.py).  tiny_episode is replayed in full; true1_episode (true dimensions) for its first turn; true2_restart (true
dimensions, 2 + 2 layers) in full, its restart turn and the turn behind it row by row (tests/restart_ref.py)."""
import numpy as np
import pytest
import torch

import restart_ref as RR
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, run_scenario
from streamvln_amd import weights as W
from streamvln_amd.synthetic import synthetic_frame
from util import load_golden


def _replay(name, steps=None, on_turn=None, tap_rows=False):
    sc, g = SCENARIOS[name], load_golden(name)
    cfg = sc["cfg"]
    orc = O.OracleStreamVLN(cfg, W.synth_state_dict(cfg, SEED), num_history=sc["num_history"])
    orc.tap_rows = tap_rows
    apply_knobs(orc, sc)
    log = run_scenario(orc, sc, preprocess=lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb)), steps=steps, on_turn=on_turn)
    for t, rec in enumerate(log):
        out = rec["out"]
        assert out.sequences[0].tolist() == g[f"t{t}_ids"].tolist()
        assert out.cache_len == int(g[f"t{t}_cache_len"])
        assert np.abs(out.hidden.numpy() - g[f"t{t}_hidden"]).max() <= 2e-4 * (1 + np.abs(g[f"t{t}_hidden"]).max())
        assert rec["views"] == int(g[f"t{t}_views"]) and rec["memory"] == bool(g[f"t{t}_memory"])
    return len(log)


def test_tiny_episode_matches_reference_fixture():
    assert _replay("tiny_episode") == 9


def test_truncated_turns_match_reference_fixture():
    """config.tokenizer_model_max_length = 150 through the reference's own prepare_inputs_labels_for_multimodal (stream_video_vln.py:241-244)"""
    assert _replay("tiny_truncate") == 3
    g = load_golden("tiny_truncate")
    assert [int(g[f"t{t}_embeds_rows"]) for t in range(3)] == [150, 150, 150]


def test_repetition_penalty_matches_reference_fixture_and_transformers():
    """generation_config.repetition_penalty = 1.3: the fixture was produced with transformers' own RepetitionPenaltyLogitsProcessor inside
    the restated greedy loop (oracle/ref_harness.py); the oracle's formula equals that class on random logits, negative values included."""
    assert _replay("tiny_penalty") == 4
    from transformers import RepetitionPenaltyLogitsProcessor
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(500, generator=g) * 3
    gen = [7, 7, 13, 499, 0, 250]
    exp = RepetitionPenaltyLogitsProcessor(penalty=1.3)(torch.tensor([gen]), logits[None].clone())[0]
    got = O.repetition_penalty(logits, gen, 1.3)
    assert torch.equal(got, exp) and not torch.equal(got, logits)
    assert torch.equal(O.repetition_penalty(logits, gen, 1.0), logits) and torch.equal(O.repetition_penalty(logits, [], 1.3), logits)


def test_true_dims_first_turn_matches_reference_fixture():
    assert _replay("true1_episode", steps=1) == 1


@pytest.fixture(scope="module")
def restart_taps():
    """true2_restart once through the oracle (ids, hidden, cache lengths against the fixture as for every replay), keeping for the tapped
    turns every layer's output on all prefill rows and layer 1's post-RoPE K rows: {turn: (rows per layer, K [T, kv_dim])}.  Read-only."""
    sc = SCENARIOS["true2_restart"]
    taps = {}

    def keep(t, rec):
        if t in sc["row_taps"]:
            out = rec["out"]
            P, T = out.prefill_span[0], out.row_taps[0].shape[0]
            k1 = out.past_key_values.k[1][:, P:P + T].transpose(0, 1).reshape(T, -1).numpy().copy()
            taps[t] = ([x.numpy() for x in out.row_taps], k1)
    assert _replay("true2_restart", on_turn=keep, tap_rows=True) == 4
    for rows, k1 in taps.values():
        for a in rows + [k1]:
            a.setflags(write=False)
    return taps


def test_restart_prefill_rows_match_reference_fixture(restart_taps):
    """Every row of the T = 1952 restart prefill and of the steady turn behind it, after each of the two decoder layers, against the rows
    and sign projections recorded from the reference's own decoder layers: pins the oracle row by row, and shows that a correct
    implementation stays inside the helper's bounds."""
    sc, g = SCENARIOS["true2_restart"], load_golden("true2_restart")
    assert sorted(restart_taps) == list(sc["row_taps"]) == [2, 3]
    assert restart_taps[2][0][0].shape == (1952, sc["cfg"].hidden) and restart_taps[3][0][0].shape == (212, sc["cfg"].hidden)
    assert g["t2_L0_rows_idx"].tolist()[:6] == [0, 255, 256, 1791, 1792, 1951]
    for t, (rows, k1) in restart_taps.items():
        for l, x in enumerate(rows):
            r = RR.compare_rows(g, t, l, x)
            print(f"oracle turn {t} layer {l}: selected rows {r['sel_err']:.2e}, projections {r['proj_err']:.2e} (bound {r['proj_bound']:.2e})")
        RR.compare_k_rows(g, t, 1, k1[g[f"t{t}_L1_rows_idx"]])


def _planted(x, kind, idx):
    """a copy of `x` with one defect a kernel could produce, away from the selected rows `idx` so that only the projections can see it"""
    y = np.array(x, dtype=np.float32)
    free = [r for r in range(y.shape[0]) if r not in set(int(i) for i in idx)]
    if kind == "row":                                   # (a) one row x (1 + 1e-3)
        y[free[len(free) // 3]] *= np.float32(1 + 1e-3)
    elif kind == "tile":                                # (b) a 32-row x 128-column tile x (1 + 2^-8), inside one 256-row tile
        r0 = next(r for r in range(32, y.shape[0] - 32, 32) if not set(range(r, r + 32)) & set(int(i) for i in idx))
        y[r0:r0 + 32, 1280:1408] *= np.float32(1 + 2.0 ** -8)
    elif kind == "swap":                                # (c) two neighbouring rows swapped
        a = free[len(free) // 2]
        b = a + 1 if a + 1 in free else a - 1
        y[[a, b]] = y[[b, a]]
    return y


@pytest.mark.parametrize("kind", ["row", "tile", "swap"])
def test_restart_row_helper_rejects_planted_defects(restart_taps, kind):
    """Self-check of tests/restart_ref.compare_rows: the oracle's tensors pass; the same tensors with (a) one row scaled by 1 + 1e-3,
    (b) a 32 x 128 tile scaled by 1 + 2^-8, (c) two rows swapped -- each planted away from the 8 full-width rows -- must FAIL, on both
    layers of both tapped turns.  A bound that lets one of them through is not acceptable."""
    g = load_golden("true2_restart")
    for t, (rows, _) in restart_taps.items():
        for l, x in enumerate(rows):
            idx = g[f"t{t}_L{l}_rows_idx"]
            clean = RR.compare_rows(g, t, l, x)
            bad = _planted(x, kind, idx)
            assert np.array_equal(bad[idx], x[idx]) and not np.array_equal(bad, x)
            err = float(np.abs(RR.project(bad) - g[f"t{t}_L{l}_proj"]).max(1).max())
            print(f"planted {kind} turn {t} layer {l}: projection error {err:.3e} = {err / clean['proj_bound']:.1f} x bound")
            with pytest.raises(AssertionError, match="projection of row"):
                RR.compare_rows(g, t, l, bad)


def test_preprocess_matches_reference_fixture():
    g = load_golden("preprocess")
    pv = O.siglip_preprocess(synthetic_frame(0, 0))
    assert pv.shape == (3, 384, 384) and pv.dtype == np.float32
    assert np.array_equal(pv.reshape(-1)[g["flat_idx"]], g["values"])
    assert abs(float(pv.astype(np.float64).sum()) - float(g["sum"])) < 1e-6


def test_cache_bookkeeping_and_incremental_equals_one_shot():
    """a-9: after a turn cache_len = L_total + n_new - 1; next turn prefill starts at the previous EOS embed;
    the incremental first-token of a later turn equals an uncached forward over all embeds."""
    sc = SCENARIOS["tiny_episode"]
    cfg = sc["cfg"]
    w = W.synth_state_dict(cfg, SEED)
    orc = O.OracleStreamVLN(cfg, w, num_history=2)
    img = torch.from_numpy(O.siglip_preprocess(synthetic_frame(0, 0)))[None, None]
    o1 = orc.generate(np.array([[11, 12, -200, 13]]), img, env_id=0, time_ids=[[0]], max_new_tokens=3)
    L1 = orc.cache[0]["inputs_embeds"].shape[0]
    assert L1 == 3 + 196 and o1.cache_len == L1 + 3 - 1
    ids2 = o1.sequences[0].tolist() + [21, -200, 22]
    o2 = orc.generate(np.array([ids2]), img, env_id=0, time_ids=[[0, 1, 2, 3, 4]], past_key_values=o1.past_key_values, max_new_tokens=1)
    E = orc.cache[0]["inputs_embeds"]
    assert E.shape[0] == L1 + 3 + 2 + 196
    h = O.qwen2_forward(orc.w, cfg, E, 0, O.KVCache(cfg.layers))[-1]
    tok, _ = O.greedy_pick(O.lm_logits(orc.w, h))
    assert tok == int(o2.sequences[0, 0])
    assert np.abs(h.numpy() - o2.hidden[0].numpy()).max() < 1e-4


def test_pool_restatement_equals_interpolate():
    from streamvln_amd.config import TINY
    x = torch.rand(2, 729, 16)
    ref = torch.nn.functional.interpolate(x.view(2, 27, 27, 16).permute(0, 3, 1, 2), size=[14, 14], mode="bilinear")
    assert torch.allclose(O.pool_bilinear(TINY, x), ref.permute(0, 2, 3, 1).reshape(2, 196, 16), atol=1e-5)


def test_memory_prune_extension_definition():
    """prune_memory_tokens (opt-in extension; the reference has no counterpart, SURVEY a-13): keeps the `keep` tokens least similar to
    the mean token, in order, ties to the lower index; the oracle's memory turns shrink accordingly."""
    g = torch.Generator().manual_seed(5)
    mem = torch.randn(50, 16, generator=g) + 2.0
    mem[7] = -mem[7]                      # the most atypical token
    mem[20] = mem[10]                     # an exact tie
    idx, score = O.prune_memory_tokens(mem, 5)
    assert idx.tolist() == sorted(idx.tolist()) and len(idx) == 5 and 7 in idx.tolist()
    ref = torch.nn.functional.cosine_similarity(mem, mem.mean(0, keepdim=True), dim=1)
    assert torch.allclose(score, ref, atol=1e-6)
    assert set(idx.tolist()) == set(sorted(range(50), key=lambda i: (float(ref[i]), i))[:5])
    full, _ = O.prune_memory_tokens(mem, 50)
    assert full.tolist() == list(range(50))
    k = [i for i in range(50) if float(score[i]) <= float(score[10])]
    idx2, _ = O.prune_memory_tokens(mem, len(k) - 1)     # cut between the tied pair: 10 stays, 20 goes
    assert 10 in idx2.tolist() and 20 not in idx2.tolist()


def test_fp8_emulation_arithmetic_and_neutral_mode():
    """oracle.Fp8Emu (extension, no reference counterpart): the per-row e4m3 quantise -> dequantise restates gemv.hip quant_fp8_rows_kernel
    (scale = amax / 448, 1 for a zero row, RNE, idempotent on its own output, every value a multiple of an e4m3 step of its row);
    with both modes off the oracle's arithmetic -- hence the reference-pinned fixture -- is untouched; with them on it changes."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 64, generator=g) * torch.tensor([1e-3, 1.0, 50.0, 3e4, 1.0, 1.0])[:, None]
    x[4] = 0.0
    x[5, 0] = 1000.0                                      # an outlier sets the row's scale
    y = O.qdq_e4m3_rows(x)
    assert torch.equal(O.qdq_e4m3_rows(y), y)             # idempotent
    assert torch.equal(y[4], torch.zeros(64)) and float(y[5, 0]) == 1000.0
    sc = x.abs().amax(-1, keepdim=True) / 448.0
    sc[4] = 1.0
    q = y / sc
    assert torch.allclose(q, q.to(torch.float8_e4m3fn).float(), rtol=1e-6, atol=0)   # every dequantised value sits on the e4m3 grid of its row
    rel = ((y - x).norm(dim=1) / x.norm(dim=1).clamp(min=1e-30))[:4]
    assert float(rel.max()) < 0.04 and float(rel.min()) > 0.01         # 3 mantissa bits: ~2.5 % per element
    assert float((y - x).abs().max() / x.abs().max()) <= 2.0 ** -4
    # the emulation object: weight cache, activation rounding to bf16 first
    emu = O.Fp8Emu(decode=True, gemm=True)
    w = {"a.weight": torch.randn(8, 32, generator=g)}
    assert emu.weight(w, "a.weight") is emu.weight(w, "a.weight")
    a = torch.randn(3, 32, generator=g)
    assert torch.equal(emu.act(a), O.qdq_e4m3_rows(a.bfloat16().float()))
    assert torch.equal(emu.lin(w, "a.weight", a, None, "decode"), a @ emu.weight(w, "a.weight").t())
    assert torch.equal(emu.lin(w, "a.weight", a, None, "prefill"), emu.act(a) @ emu.weight(w, "a.weight").t())
    off = O.Fp8Emu()
    assert torch.equal(off.lin(w, "a.weight", a, None, "prefill"), a @ w["a.weight"].t())
    # end to end on the tiny episode's first turns: neutral emulation == plain oracle bit for bit; the modes change the hidden rows
    sc_t = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    cfg = sc_t["cfg"]
    sd = W.synth_state_dict(cfg, SEED)
    pre = lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb))
    runs = {}
    for key, fp8 in (("plain", None), ("neutral", O.Fp8Emu()), ("decode", O.Fp8Emu(decode=True)), ("gemm", O.Fp8Emu(gemm=True))):
        orc = O.OracleStreamVLN(cfg, sd, num_history=sc_t["num_history"], fp8=fp8)
        log = run_scenario(orc, sc_t, preprocess=pre, steps=5)
        runs[key] = [(r["out"].sequences[0].tolist(), r["out"].hidden.numpy()) for r in log]
        assert len(orc.layer_taps) == cfg.layers
    assert runs["plain"][0][0] == runs["neutral"][0][0] and np.array_equal(runs["plain"][0][1], runs["neutral"][0][1])
    h0 = runs["plain"][0][1]
    assert np.array_equal(runs["decode"][0][1][0], h0[0])              # weight-only decode mode: the prefill row is untouched ...
    d = np.linalg.norm(runs["decode"][0][1][1] - h0[1]) / np.linalg.norm(h0[1])
    assert (0.0 < d < 0.3) or runs["decode"][0][0][0] != runs["plain"][0][0][0]     # ... the decode rows move (unless the e4m3 lm_head already changed the fed token)
    gmm = np.linalg.norm(runs["gemm"][0][1][0] - h0[0]) / np.linalg.norm(h0[0])
    assert 0.005 < gmm < 0.3, gmm


def test_teacher_tokens_mode_keeps_the_models_own_picks():
    """OracleStreamVLN.teacher_tokens (test mode): a turn decodes the given tokens; with the model's own tokens nothing changes, with a
    changed second token the first row, the first pick and its margin stay and the sequence is the forced one."""
    sc = SCENARIOS["tiny_episode"]
    cfg = sc["cfg"]
    pre = lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb))
    sd = W.synth_state_dict(cfg, SEED)
    free = run_scenario(O.OracleStreamVLN(cfg, sd, num_history=sc["num_history"]), sc, preprocess=pre, steps=1)[0]["out"]
    ids = free.sequences[0].tolist()
    assert len(ids) >= 2
    orc = O.OracleStreamVLN(cfg, sd, num_history=sc["num_history"])
    orc.teacher_tokens = [list(ids)]
    same = run_scenario(orc, sc, preprocess=pre, steps=1)[0]["out"]
    assert same.sequences[0].tolist() == ids and orc.own_picks == ids and orc.teacher_tokens == []
    assert torch.equal(same.hidden, free.hidden) and same.margins == free.margins and same.cache_len == free.cache_len
    forced = [ids[0], (ids[1] + 1) % cfg.vocab] + ids[2:]
    orc = O.OracleStreamVLN(cfg, sd, num_history=sc["num_history"])
    orc.teacher_tokens = [forced]
    other = run_scenario(orc, sc, preprocess=pre, steps=1)[0]["out"]
    assert other.sequences[0].tolist() == forced and orc.own_picks[:2] == ids[:2]
    assert torch.equal(other.hidden[:2], free.hidden[:2]) and other.margins[:2] == free.margins[:2]
    assert len(forced) < 3 or not torch.equal(other.hidden[2], free.hidden[2])
