"""End-to-end parity of the HIP path (through the C ABI and the Python operator surface) against the
golden fixtures produced from the reference, and against the CPU oracle run live on the GPU box.

North-star bar: action-token ids bit-identical, hidden states within 1e-3 (fp32 parity mode).
bf16 shipping mode is additionally checked with a bf16-sized bound and id agreement wherever the
oracle's top-2 logit margin exceeds the bf16 noise floor."""
import numpy as np
import pytest
import torch

from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids, run_scenario
from streamvln_amd.model import StreamVLNForCausalLM
import util
from util import load_golden

pytestmark = pytest.mark.gpu
HIDDEN_TOL = 1e-3          # north_star: hidden states within 1e-3 (fp32)


def _note(name, line):
    """measured values of a test (the numbers DESIGN.md quotes) -> gpurun_out/<name>.txt on the GPU box; never fails the test"""
    import os
    try:
        d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _model(sc, dtype):
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=1, max_frames=1 + (sc["num_history"] or 0),
                             max_positions=sc.get("max_positions", 2048))
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    apply_knobs(m, sc)
    return m


def _run(m, sc, device="cuda"):
    taps = []

    def on_turn(t, rec):
        ne, kl = m.env_state(0)
        taps.append(dict(hidden=m.last_hidden(), cache_len=kl, n_embeds=ne))
    proc = m.get_vision_tower().image_processor
    log = run_scenario(m, sc, preprocess=proc.preprocess_array, on_turn=on_turn, device=device)
    return log, taps


@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode", "true4_episode", "tiny_truncate", "tiny_penalty", "true2_restart"])
def test_fp32_parity_vs_reference_golden(name):
    """true1_episode runs through the window restart at true width (9-frame ViT batch, 1568-row <memory> block, T = 1952);
    true4_episode has 4 ViT + 4 LLM layers at true width and the full 152 064-entry vocabulary (fused inter-layer norms, lm_head);
    true2_restart runs the same restart shape at depth 2 + 2 after two turns (a window of 8 frames) and the steady turn behind it: the
    embeds taps of its restart turn pin the 9-frame ViT batch through two ViT layers (the fc2 -> layer_norm1 hand-off at 6561 rows);
    what its prefill rows hold is checked by test_restart_prefill_rows_vs_reference_golden;
    tiny_truncate: config.tokenizer_model_max_length = 150 cuts every turn's spliced rows (stream_video_vln.py:241-244);
    tiny_penalty: generation_config.repetition_penalty = 1.3 (transformers' RepetitionPenaltyLogitsProcessor in the greedy loop)."""
    sc, g = SCENARIOS[name], load_golden(name)
    m = _model(sc, torch.float32)
    embeds = []
    seen = [0]

    def grab(t, rec):
        ne, _ = m.env_state(0)
        if m.curr_t[0] == 1:
            seen[0] = 0
        embeds.append(m.get_embeds(0, seen[0], ne - seen[0]))
        seen[0] = ne
    taps = []

    def on_turn(t, rec):
        grab(t, rec)
        taps.append(dict(hidden=m.last_hidden(), cache_len=m.env_state(0)[1]))
    proc = m.get_vision_tower().image_processor
    log = run_scenario(m, sc, preprocess=proc.preprocess_array, on_turn=on_turn, device="cuda")
    assert len(log) == int(g["n_turns"])
    for t, rec in enumerate(log):
        ids = rec["out"].sequences[0].tolist()
        assert rec["views"] == int(g[f"t{t}_views"]) and rec["n_inputs"] == int(g[f"t{t}_n_inputs"])
        # vision + splice: this turn's inputs_embeds rows
        e = embeds[t]
        assert e.shape[0] == int(g[f"t{t}_embeds_rows"])
        cols = [0, 1, e.shape[1] // 2, e.shape[1] - 1]
        assert np.abs(e[:, cols] - g[f"t{t}_embeds_cols"]).max() <= HIDDEN_TOL, (name, t, "embeds cols")
        assert np.abs(e[[0, e.shape[0] // 2, e.shape[0] - 1]] - g[f"t{t}_embeds_sel"]).max() <= HIDDEN_TOL, (name, t, "embeds rows")
        assert np.abs(e.sum(1) - g[f"t{t}_embeds_rowsum"]).max() <= 1e-2, (name, t, "embeds rowsum")
        # token ids bit-identical, hidden states within 1e-3, cache bookkeeping identical
        assert ids == g[f"t{t}_ids"].tolist(), (name, t, ids, g[f"t{t}_ids"].tolist())
        assert np.abs(taps[t]["hidden"] - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, (name, t, "hidden")
        assert taps[t]["cache_len"] == int(g[f"t{t}_cache_len"])
        assert rec["out"].past_key_values.get_seq_length() == int(g[f"t{t}_cache_len"])
    m.close()


# bf16 shipping mode against the fp32 reference fixture.  The hidden state is a unit-RMS vector after the final norm; with bf16
# storage of activations between ~10 kernels per layer its error grows like sqrt(depth) * 2^-9.  BF16_HIDDEN_REL bounds the relative
# L2 error of EVERY comparable hidden row (rows of a turn up to and including the first token that differs from the fixture: they saw
# identical inputs); measured values are printed.  Token ids must agree wherever the fixture's top-2 logit margin exceeds
# BF16_MARGIN (logit error of a bf16 run ~ |h| * |w| * 2^-8 ~ 0.02 here).  A window-restart turn starts from an empty cache and a prompt that
# carries no generated id, so it is comparable again whatever an earlier turn picked: the comparison resumes there.
# true2_restart: the value of four layers at the same width -- under the sqrt(depth) growth two layers cannot legitimately need more.
BF16_HIDDEN_REL = {"tiny_episode": 1.2e-2, "true1_episode": 8e-3, "true4_episode": 1.2e-2, "true2_restart": 1.2e-2}
BF16_MARGIN = 0.05


def test_bf16_episode_through_the_restart_is_bit_reproducible():
    """true1_episode twice on one bf16 engine: first turn, seven steady turns and the window restart (9-frame ViT batch, T = 1952 prefill on
    the 8-phase GEMM with its counted LDS-DMA waits, the two-slice down_proj, the column-tiles-fastest fc2).  No kernel on the path uses
    atomics or an order-dependent reduction, so ids and final-norm hidden rows must repeat BIT FOR BIT; a staging race under the real
    load of a turn (which an isolated op test may not provoke) would show here as a differing row."""
    sc = SCENARIOS["true1_episode"]
    m = _model(sc, torch.bfloat16)
    log_a, taps_a = _run(m, sc)
    m.reset(1)
    log_b, taps_b = _run(m, sc)
    assert len(log_a) == len(log_b) == 9
    for t, (a, b) in enumerate(zip(log_a, log_b)):
        assert a["out"].sequences[0].tolist() == b["out"].sequences[0].tolist(), t
    for t, (a, b) in enumerate(zip(taps_a, taps_b)):
        assert a["cache_len"] == b["cache_len"] and np.array_equal(a["hidden"], b["hidden"]), t
    m.close()


@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode", "true4_episode", "true2_restart"])
def test_bf16_mode_vs_golden(name):
    sc, g = SCENARIOS[name], load_golden(name)
    m = _model(sc, torch.bfloat16)
    log, taps = _run(m, sc)
    agree = total = rows = 0
    worst = 0.0
    diverged = False
    for t, rec in enumerate(log):
        ids = rec["out"].sequences[0].tolist()
        gold = g[f"t{t}_ids"].tolist()
        margins = g[f"t{t}_margins"]
        n = 0
        while n < min(len(ids), len(gold)) and ids[n] == gold[n]:
            n += 1
        k = min(n + 1, len(gold), len(ids))                 # comparable rows of this turn
        if bool(g[f"t{t}_memory"]):
            diverged = False                                  # a restart turn depends on no earlier id
        if not diverged:
            for j in range(k):
                h, gh = taps[t]["hidden"][j], g[f"t{t}_hidden"][j]
                rel = float(np.linalg.norm(h - gh) / np.linalg.norm(gh))
                worst = max(worst, rel); rows += 1
                assert rel < BF16_HIDDEN_REL[name], (name, t, j, rel)
                if j < len(margins) and margins[j] > BF16_MARGIN:
                    assert ids[j] == gold[j], (name, t, j, ids, gold, margins)
            total += len(gold); agree += n
            if n < len(gold):
                diverged = True                               # later turns start from different generated ids: not comparable
    assert rows >= 1
    line = (f"bf16 vs fp32 fixture [{name}]: {rows} hidden rows compared, worst rel L2 error {worst:.2e}, "
            f"{agree}/{total} ids agree before the first divergence")
    print(line)
    _note("bf16_vs_fixture", line)
    m.close()


def _cached_k_rows(m, layer, positions, pool_pages):
    """post-RoPE K rows [len(positions), kv_dim] of env 0 as `layer`'s paged cache holds them (what the RoPE + append launch wrote and
    the attention reads; the k columns of the q|k|v buffer are never rotated).  The C ABI reads an env's pages on layer 0 and the raw
    pools of any layer; every layer shares the env's page table, so the physical page of a logical page is the one page of the layer-0
    pool whose K rows equal the env's bit for bit (one page exactly, on an engine that has not run the same turn before)."""
    import ctypes as C
    from streamvln_amd import _lib
    PF = C.POINTER(C.c_float)
    nkv = m.cfg.kv_heads
    raw0, raw0_v = np.zeros((pool_pages * 64, nkv, 128), np.float32), np.zeros((pool_pages * 64, nkv, 128), np.float32)
    _lib.check(m._lib.svln_op_kv_pool_read(m._h, 0, 0, pool_pages * 64, raw0.ctypes.data_as(PF), raw0_v.ctypes.data_as(PF)))
    k, v = np.zeros((64, nkv, 128), np.float32), np.zeros((64, nkv, 128), np.float32)
    phys, out = {}, []
    for p in (int(p) for p in positions):
        lp = p // 64
        if lp not in phys:
            _lib.check(m._lib.svln_op_kv_read(m._h, 0, lp * 64, 64, k.ctypes.data_as(PF), v.ctypes.data_as(PF)))
            match = [q for q in range(pool_pages) if np.array_equal(raw0[q * 64:(q + 1) * 64], k)]
            assert len(match) == 1, (lp, match)
            phys[lp] = match[0]
        _lib.check(m._lib.svln_op_kv_pool_read(m._h, layer, phys[lp] * 64, 64, k.ctypes.data_as(PF), v.ctypes.data_as(PF)))
        out.append(k[p % 64].reshape(-1).copy())
    return np.stack(out)


def _run_probed(m, sc, g, with_k=False):
    """true2_restart with the layer-1 probe on: after each tapped turn, probes 0 (x entering layer 1 = everything layer 0 produced) and
    1 (x leaving layer 1) of all its prefill rows; with_k: layer 1's cached K rows of the fixture's selected rows as well ("k1")"""
    probes = {}
    taps = []

    def on_turn(t, rec):
        taps.append(dict(hidden=m.last_hidden(), cache_len=m.env_state(0)[1]))
        if t in sc["row_taps"]:
            T = g[f"t{t}_L0_proj"].shape[0]
            probes[t] = {w: m.layer_probe(w, max_rows=1952) for w in (0, 1)}
            assert all(p.shape[0] == T for p in probes[t].values()), (t, T, [p.shape for p in probes[t].values()])
            if with_k:
                P = taps[-1]["cache_len"] - (rec["out"].sequences.shape[1] - 1) - T          # cached positions before this prefill
                probes[t]["k1"] = _cached_k_rows(m, 1, P + g[f"t{t}_L1_rows_idx"], sc["max_positions"] // 64)
    proc = m.get_vision_tower().image_processor
    log = run_scenario(m, sc, preprocess=proc.preprocess_array, on_turn=on_turn, device="cuda")
    return log, taps, probes


def test_restart_prefill_rows_vs_reference_golden():
    """The window-restart turn at depth, EVERY prefill row against the reference (tests/restart_ref.py; DESIGN.md parity section).  Ids and
    the final hidden of a turn read its last row only, and a wrong row among 1952 keys moves them by ~1e-6; so after the restart turn
    (T = 1952: the 8-phase 256 x 256 GEMM on a ragged last row tile, the unfused norms of M > 256, the separate RoPE + append launch,
    31 key tiles) and the steady turn behind it (T = 212 on 1954 cached positions) the layer-1 probe gives what layer 0 produced and
    what layer 1 produced on all rows, held against 8 (4) full-width reference rows within 1e-3 and, for every row, 16 sign projections
    within 32 x the recorded oracle-vs-reference noise; layer 1's post-RoPE K rows, read from the paged cache, within 1e-3.  The probed
    pass must equal an unprobed pass of the same engine bit for bit (the tap stays a tap).
    Measured on an MI355X (every run writes its own figures through _note("restart_rows", ...)), fp32 engine, error / bound:
      turn 2 (T = 1952)  layer 0: selected rows 7.75e-06 / 1e-3, worst projection 3.27e-04 (row 881) / 3.35e-03 = 0.098
                         layer 1: selected rows 9.72e-06 / 1e-3, worst projection 5.52e-04 (row 41)  / 5.62e-03 = 0.098;  K rows 1.17e-05 / 1e-3
      turn 3 (T = 212)   layer 0: selected rows 3.22e-06 / 1e-3, worst projection 1.61e-04 (row 199) / 2.43e-03 = 0.066
                         layer 1: selected rows 4.35e-06 / 1e-3, worst projection 2.77e-04 (row 129) / 4.35e-03 = 0.064;  K rows 4.65e-06 / 1e-3
    (the engine sits ~3 x the oracle-vs-reference noise away from the reference, a tenth of the bound; the planted defects of
    tests/test_oracle_golden.py sit 10 to 25 x above it).
    bf16 engine: relative L2 error of each selected row of both probes under BF16_HIDDEN_REL (no projection bound: none is measured);
    measured 7.20e-03 / 8.50e-03 (turn 2, layers 0 / 1, both at row 256) and 4.46e-03 / 5.13e-03 (turn 3) under 1.2e-2."""
    import restart_ref as RR
    name = "true2_restart"
    sc, g = SCENARIOS[name], load_golden(name)
    m = _model(sc, torch.float32)
    m.set_layer_taps(True, 1)                                 # the probed pass first: no page of the pool holds an earlier pass' rows yet
    log1, taps1, probes = _run_probed(m, sc, g, with_k=True)
    m.set_layer_taps(False)
    m.reset(1)
    log0, taps0 = _run(m, sc)                                 # unprobed
    assert len(log0) == len(log1) == int(g["n_turns"]) and sorted(probes) == list(sc["row_taps"])
    for t, (a, b) in enumerate(zip(log0, log1)):
        ids = b["out"].sequences[0].tolist()
        assert ids == g[f"t{t}_ids"].tolist(), (t, ids)
        assert np.abs(taps1[t]["hidden"] - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, (t, "hidden")
        assert taps1[t]["cache_len"] == int(g[f"t{t}_cache_len"])
        assert a["out"].sequences[0].tolist() == ids and np.array_equal(taps0[t]["hidden"], taps1[t]["hidden"]), (t, "probed != unprobed")
    failures = []
    for t in sc["row_taps"]:
        for layer in (0, 1):
            try:
                r = RR.compare_rows(g, t, layer, probes[t][layer])
                line = (f"fp32 engine vs reference rows [{name}] turn {t} layer {layer}: {probes[t][layer].shape[0]} rows, selected rows "
                        f"|err| {r['sel_err']:.2e} (bound {HIDDEN_TOL:.0e}), worst projection |err| {r['proj_err']:.2e} at row {r['proj_row']} "
                        f"(bound {r['proj_bound']:.2e}, ratio {r['proj_ratio']:.3f})")
            except AssertionError as e:
                failures.append(e.args[0] if e.args else e)
                line = f"fp32 engine vs reference rows [{name}] turn {t} layer {layer}: FAILED {e.args[0] if e.args else e}"
            print(line)
            _note("restart_rows", line)
        # layer 1's K rows: the q|k|v buffer (probe 7) holds q rotated and k as the product left it -- the rotated k goes to the pages
        # only -- so the rows of the paged cache are what is held against the reference's cache
        idx = g[f"t{t}_L1_rows_idx"]
        ref_k = g[f"t{t}_K1_rows"].astype(np.float64)
        err = float(np.abs(probes[t]["k1"] - ref_k).max())
        line = (f"fp32 engine vs reference K rows [{name}] turn {t} layer 1: {len(idx)} post-RoPE rows of the paged cache, "
                f"|err| {err:.2e} (bound {HIDDEN_TOL:.0e})")
        print(line)
        _note("restart_rows", line)
        if err > HIDDEN_TOL:
            failures.append((f"t{t}_K1_rows", err))
    assert not failures, failures
    m.close()

    # bf16 leg.  The restart turn depends on no earlier id; the turn behind it is comparable if the restart turn's ids are the fixture's
    # (their margins, 0.23, are above BF16_MARGIN, so they must be)
    m = _model(sc, torch.bfloat16)
    m.set_layer_taps(True, 1)
    log, _, probes = _run_probed(m, sc, g)
    m.set_layer_taps(False)
    ids2, gold2 = log[2]["out"].sequences[0].tolist(), g["t2_ids"].tolist()
    assert all(ids2[j] == gold2[j] for j in range(len(gold2)) if g["t2_margins"][j] > BF16_MARGIN), (ids2, gold2)
    for t in sc["row_taps"] if ids2 == gold2 else sc["row_taps"][:1]:
        for layer in (0, 1):
            idx, ref = g[f"t{t}_L{layer}_rows_idx"], g[f"t{t}_L{layer}_rows"].astype(np.float64)
            got = probes[t][layer][idx].astype(np.float64)
            rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
            line = (f"bf16 engine vs reference rows [{name}] turn {t} layer {layer}: {len(idx)} selected rows, worst rel L2 error "
                    f"{rel.max():.2e} at row {int(idx[rel.argmax()])} (bound {BF16_HIDDEN_REL[name]:.1e})")
            print(line)
            _note("restart_rows", line)
            assert rel.max() < BF16_HIDDEN_REL[name], (t, layer, rel.tolist())
    m.close()


@pytest.mark.parametrize("name", ["tiny_episode", "true4_episode", "tiny_penalty"])
def test_persistent_decode_layer_vs_reference_golden(name):
    """svln_set_decode_persistent: every decode step runs, per layer, the attention launch + ONE persistent launch (LDS-DMA weight ring,
    granule all-gathers between the products; decode_layer.hip).  Same bar as the launched path against the reference-generated
    fixtures: fp32 engine ids identical and hidden <= 1e-3 on every generated token (tiny: 9 turns through two restarts; true4: true
    width, full vocabulary; tiny_penalty: the repetition penalty rides on the same steps); bf16 engine under the bf16 bound, ids
    wherever the fixture margin allows.  With hipGraph replay and without; switching it off restores the launched path bit for bit."""
    sc, g = SCENARIOS[name], load_golden(name)
    m = _model(sc, torch.float32)
    m.set_decode_persistent(True)
    for graph in (True, False):
        m.set_decode_graph(graph)
        m.reset(1)
        log, taps = _run(m, sc)
        assert len(log) == int(g["n_turns"])
        worst = 0.0
        for t, rec in enumerate(log):
            assert rec["out"].sequences[0].tolist() == g[f"t{t}_ids"].tolist(), (name, graph, t, rec["out"].sequences[0].tolist(), g[f"t{t}_ids"].tolist())
            err = float(np.abs(taps[t]["hidden"] - g[f"t{t}_hidden"]).max())
            worst = max(worst, err)
            assert err <= HIDDEN_TOL, (name, graph, t, err)
            assert taps[t]["cache_len"] == int(g[f"t{t}_cache_len"])
    _note("persistent_decode", f"fp32 engine, persistent decode layer vs reference fixture [{name}]: ids identical, worst |hidden err| {worst:.2e}")
    m.close()
    if name == "tiny_penalty":
        return
    m = _model(sc, torch.bfloat16)
    log0, taps0 = _run(m, sc)                                # launched path
    m.set_decode_persistent(True)
    m.reset(1)
    log1, taps1 = _run(m, sc)
    worst = worst_pair = 0.0
    for t, rec in enumerate(log1):
        ids, gold, margins = rec["out"].sequences[0].tolist(), g[f"t{t}_ids"].tolist(), g[f"t{t}_margins"]
        n = 0
        while n < min(len(ids), len(gold)) and ids[n] == gold[n]:
            n += 1
        for j in range(min(n + 1, len(gold), len(ids))):
            gh = g[f"t{t}_hidden"][j]
            rel = float(np.linalg.norm(taps1[t]["hidden"][j] - gh) / np.linalg.norm(gh))
            worst = max(worst, rel)
            assert rel < BF16_HIDDEN_REL[name], (name, t, j, rel)
            if margins[j] > BF16_MARGIN:
                assert ids[j] == gold[j], (name, t, j, ids, gold, margins)
            if log0[t]["out"].sequences[0].tolist()[:j] == ids[:j] and j < len(taps0[t]["hidden"]):
                h0 = taps0[t]["hidden"][j]
                worst_pair = max(worst_pair, float(np.linalg.norm(taps1[t]["hidden"][j] - h0) / np.linalg.norm(h0)))
        if n < len(gold):
            break
    _note("persistent_decode", f"bf16 engine, persistent decode layer [{name}]: worst rel L2 vs fp32 fixture {worst:.2e}, vs the launched path {worst_pair:.2e}")
    m.set_decode_persistent(False)
    m.reset(1)
    log2, taps2 = _run(m, sc)
    assert [r["out"].sequences[0].tolist() for r in log2] == [r["out"].sequences[0].tolist() for r in log0]
    for a, b in zip(taps0, taps2):
        assert np.array_equal(a["hidden"], b["hidden"])
    m.close()


def test_feature_cache_keeps_parity_and_skips_history_reencode():
    """opt-in memoisation of pooled frame features: same ids / hidden as the reference fixture, history frames hit"""
    sc, g = SCENARIOS["tiny_episode"], load_golden("tiny_episode")
    m = _model(sc, torch.float32)
    m.set_feature_cache(32)
    log, taps = _run(m, sc)
    for t, rec in enumerate(log):
        assert rec["out"].sequences[0].tolist() == g[f"t{t}_ids"].tolist(), t
        assert np.abs(taps[t]["hidden"] - g[f"t{t}_hidden"]).max() <= HIDDEN_TOL, t
    hits, misses = m.feature_cache_stats()
    # frames seen: 9 turn frames + history {0, 6} at step 12 and {0, 12} at step 24 -> 13 lookups; 0, 0 and 12 are hits
    assert hits == 3 and misses == 10, (hits, misses)
    m.set_feature_cache(0)
    m.close()


def test_graph_replay_equals_plain_launches():
    sc = SCENARIOS["tiny_episode"]
    outs = []
    for graph in (False, True):
        m = _model(sc, torch.bfloat16)
        m.set_decode_graph(graph)
        sc2 = dict(sc, eos_mod=0)                      # never stop early: 6 decode steps per turn
        log, taps = _run(m, sc2)
        outs.append(([r["out"].sequences[0].tolist() for r in log], [tp["hidden"] for tp in taps]))
        m.close()
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, b)


def test_one_call_turn_equals_the_five_call_sequence_and_stream_adoption():
    """svln_turn (what `generate` uses: ONE crossing per model turn) against the five entry points it stands for (svln_encode_frames,
    svln_kv_reset / svln_reset_env, svln_append_turn, svln_generate) driven by hand through the same episode incl. both <memory> restarts:
    ids, hidden taps, cache lengths and embeds counts bit-identical.  The same episode once more with torch running on the engine's own
    stream (`model.torch_stream`: no cross-stream ordering calls) and with the frames in the engine's pinned ring."""
    import ctypes as C
    from streamvln_amd import _lib
    from streamvln_amd.synthetic import synthetic_frame
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16)
    log1, taps1 = _run(m, sc)
    ref = [(r["out"].sequences[0].tolist(), tp["hidden"], tp["cache_len"], tp["n_embeds"]) for r, tp in zip(log1, taps1)]

    class FiveCalls:
        """the pre-round-4 body of StreamVLNForCausalLM.generate"""
        def __init__(self, m):
            self.m = m

        def __getattr__(self, k):
            return getattr(self.m, k)

        def generate(self, inputs=None, images=None, **kwargs):
            m = self.m
            ids, pix, V, n_memory, env_id, past, max_new, eos = m._parse_call(inputs, images, kwargs)
            m._order_engine_after(pix)
            _lib.check(m._lib.svln_encode_frames(m._h, pix.data_ptr(), V, 1))
            m._order_torch_after(pix)
            m._begin_turn(env_id, past)
            ids_np = np.ascontiguousarray(ids.numpy())
            _lib.check(m._lib.svln_append_turn(m._h, m._slot(env_id), ids_np.ctypes.data_as(C.POINTER(C.c_int64)), ids_np.size, n_memory))
            cap = min(max_new, m.cfg.max_positions)
            out = np.zeros(cap, dtype=np.int64)
            n_out = C.c_int32()
            eos_np = np.asarray(eos, dtype=np.int64)
            _lib.check(m._lib.svln_generate(m._h, m._slot(env_id), max_new, eos_np.ctypes.data_as(C.POINTER(C.c_int64)), eos_np.size,
                                            out.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n_out)))
            return m._result(env_id, out[: n_out.value], inputs)
    m.reset(1)
    taps = []
    proc = m.get_vision_tower().image_processor
    log5 = run_scenario(FiveCalls(m), sc, preprocess=proc.preprocess_array, device="cuda",
                        on_turn=lambda t, rec: taps.append((m.last_hidden(),) + m.env_state(0)[::-1]))
    assert len(log5) == len(ref)
    for t, (rec, (h, kl, ne)) in enumerate(zip(log5, taps)):
        assert rec["out"].sequences[0].tolist() == ref[t][0], t
        assert np.array_equal(h, ref[t][1]) and kl == ref[t][2] and ne == ref[t][3], t
        assert rec["out"].past_key_values.length == kl
    # torch on the engine's stream + frames in the pinned ring
    m.reset(1)
    ring = m.frame_ring(sc["steps"], 480, 640)
    for s_ in range(sc["steps"]):
        ring[s_][...] = synthetic_frame(0, s_)
    slot_of = {synthetic_frame(0, s_).tobytes()[:64]: s_ for s_ in range(sc["steps"])}
    with torch.cuda.stream(m.torch_stream):
        log2, taps2 = [], []
        log2 = run_scenario(m, sc, preprocess=lambda rgb: proc.preprocess_array(ring[slot_of[rgb.tobytes()[:64]]]), device="cuda",
                            on_turn=lambda t, rec: taps2.append(m.last_hidden()))
    for t, rec in enumerate(log2):
        assert rec["out"].sequences[0].tolist() == ref[t][0], t
        assert np.array_equal(taps2[t], ref[t][1]), t
    # a stale handle is still refused before anything reaches the engine, and a refused turn does not count
    ids, img = _first_turn_inputs(m, sc)
    m.reset(1)
    out = m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=2, eos_token_ids=[])
    m.reset_for_env(0)
    with pytest.raises(ValueError, match="past_key_values"):
        m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=2, eos_token_ids=[], past_key_values=out.past_key_values)
    assert m.curr_t[0] == 0
    m.close()


def test_fp8_decode_weights_opt_in():
    """SURVEY 8f-2 extension (no reference oracle: the reference is bf16 only).  With e4m3 decode weights the prefill is untouched
    (bf16), so every turn's first hidden row is bit-identical; decode-step hidden states stay within the e4m3 error level; graph
    replay equals plain launches; switching it off restores the bf16 results exactly; fp32 engines refuse it."""
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)          # never stop early: several decode steps per turn
    m = _model(sc, torch.bfloat16)
    log0, taps0 = _run(m, sc)
    m.set_fp8_decode(True)
    runs = []
    for graph in (True, False):
        m.set_decode_graph(graph)
        m.reset(1)
        log, taps = _run(m, sc)
        runs.append(([r["out"].sequences[0].tolist() for r in log], [tp["hidden"] for tp in taps], [tp["cache_len"] for tp in taps]))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)
    assert runs[0][2] == [tp["cache_len"] for tp in taps0]                       # same protocol bookkeeping
    agree, total, worst = 0, 0, 0.0
    for t, (h8, tp0, r0) in enumerate(zip(runs[0][1], taps0, log0)):
        if t == 0:
            assert np.array_equal(h8[0], tp0["hidden"][0])                       # first turn, first token: prefill only (bf16 in both modes)
        ids0, ids8 = r0["out"].sequences[0].tolist(), runs[0][0][t]
        n = 0
        while n < len(ids0) and ids0[n] == ids8[n]:
            n += 1
        agree += n; total += len(ids0)
        k = min(n + 1, len(ids0))            # rows up to and including the first divergent token saw identical inputs
        ref = tp0["hidden"][:k].astype(np.float64)
        worst = max(worst, float(np.linalg.norm(h8[:k] - ref) / np.linalg.norm(ref)))
        if n < len(ids0):
            break                             # later turns start from different tokens: not comparable
    assert worst < 0.08, worst
    assert total > 0
    print(f"fp8 decode weights: {agree}/{total} token ids agree with bf16 before the first divergence, hidden rel err {worst:.4f}")
    m.set_fp8_decode(False)
    m.set_decode_graph(True)
    m.reset(1)
    log1, taps1 = _run(m, sc)
    assert [r["out"].sequences[0].tolist() for r in log1] == [r["out"].sequences[0].tolist() for r in log0]
    for a, b in zip(taps0, taps1):
        assert np.array_equal(a["hidden"], b["hidden"])
    m.close()
    m32 = _model(SCENARIOS["tiny_episode"], torch.float32)
    with pytest.raises(Exception, match="bf16"):
        m32.set_fp8_decode(True)
    m32.close()


def test_reference_harness_env_ids_map_onto_engine_slots():
    """The reference harness calls model.reset(world_size) and drives env_id = rank (streamvln_eval.py:225,324,542,553) in a process
    that owns ONE env: an engine with max_envs = 1 must accept reset(8) + generate(env_id=7), and refuse a second live env."""
    sc, g = SCENARIOS["tiny_episode"], load_golden("tiny_episode")
    m = _model(sc, torch.float32)
    m.reset(8)
    proc = m.get_vision_tower().image_processor
    from scenarios import run_scenario as rs
    from streamvln_amd.agent import StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    enc = SyntheticPromptEncoder(sc["cfg"], seed=7, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
    ag = StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=7,
                        max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=proc.preprocess_array, device="cuda")
    for step in range(16):                                    # 4 turns incl. the first window restart, all as env 7
        ag.act(synthetic_frame(0, step))
    for t, rec in enumerate(ag.turn_log):
        assert rec["out"].sequences[0].tolist() == g[f"t{t}_ids"].tolist(), t
        assert rec["out"].past_key_values.env_id == 7
    img = torch.zeros(1, 1, 3, 384, 384)
    with pytest.raises(ValueError, match="slots"):
        m.generate(inputs=torch.tensor([[5, 6, -200, 7]]), images=img, env_id=3, time_ids=[[0]], max_new_tokens=1)   # a second live env
    with pytest.raises(IndexError):
        m.generate(inputs=torch.tensor([[5, 6, -200, 7]]), images=img, env_id=8, time_ids=[[0]], max_new_tokens=1)
    m.reset(2)                                               # a new reset frees the binding
    out = m.generate(inputs=torch.tensor([[5, 6, -200, 7]]), images=img, env_id=1, time_ids=[[0]], max_new_tokens=1, eos_token_ids=[])
    assert out.sequences.shape == (1, 1)
    m.close()


def test_fp8_mfma_gemms_opt_in():
    """SURVEY 8f-2 / BASELINE configs[4] (no reference oracle: the reference is bf16 only): with svln_set_fp8_gemm the LLM's prefill
    products -- and, in generate_batch with >= 4 envs, the decode-step products -- are e4m3 MFMA products.  Reported: id agreement
    with the bf16 run before the first divergence and the relative error of the hidden states; switching it off restores bf16 exactly."""
    from streamvln_amd.synthetic import synthetic_frame
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    m = _model(sc, torch.bfloat16)
    log0, taps0 = _run(m, sc)
    m.set_fp8_gemm(True)
    m.reset(1)
    log8, taps8 = _run(m, sc)
    assert [tp["cache_len"] for tp in taps8] == [tp["cache_len"] for tp in taps0]
    agree = total = 0
    worst = 0.0
    for t, (r0, r8) in enumerate(zip(log0, log8)):
        ids0, ids8 = r0["out"].sequences[0].tolist(), r8["out"].sequences[0].tolist()
        n = 0
        while n < len(ids0) and ids0[n] == ids8[n]:
            n += 1
        agree += n; total += len(ids0)
        k = min(n + 1, len(ids0))
        ref = taps0[t]["hidden"][:k].astype(np.float64)
        worst = max(worst, float(np.linalg.norm(taps8[t]["hidden"][:k] - ref) / np.linalg.norm(ref)))
        if n < len(ids0):
            break
    line = f"fp8 MFMA GEMMs (TINY): {agree}/{total} token ids agree with bf16 before the first divergence, hidden rel err {worst:.4f}"
    print(line)
    _note("fp8_true_width", line)
    # (TINY's top-2 margins are ~0.01: the id-agreement floor is asserted at true width, test_fp8_opt_ins_true_width_vs_bf16_and_fixture)
    assert worst < 0.10 and agree >= 1, (worst, agree, total)
    # 8 envs through generate_batch: prefill rows and the batched decode steps (32-row tiles) take the fp8 MFMA path
    m.close()
    NE = 8                                                   # configs[4]: 8 concurrent envs + fp8 MFMA products
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.bfloat16, max_envs=NE, max_frames=NE, max_positions=1024)
    m.load_synthetic(SEED)
    m.model.num_history = 2
    m.set_fp8_gemm(True)
    reqs = []
    for e in range(NE):
        ids, img = _first_turn_inputs(m, sc, step=e, seed=20 + e)
        reqs.append(dict(inputs=ids, images=img, env_id=e, time_ids=[[0]]))
    outs = m.generate_batch(reqs, max_new_tokens=4, eos_token_ids=[])
    hb = [m.last_hidden_batch(e) for e in range(NE)]
    m.set_fp8_gemm(False)
    m.reset(NE)
    outs16 = m.generate_batch(reqs, max_new_tokens=4, eos_token_ids=[])
    for e in range(NE):
        h16 = m.last_hidden_batch(e)
        assert outs[e].sequences.shape == (1, 4)
        rel = float(np.linalg.norm(hb[e][0] - h16[0]) / np.linalg.norm(h16[0]))      # first token: prefill only
        assert rel < 0.10, (e, rel)
    m.close()
    m32 = _model(SCENARIOS["tiny_episode"], torch.float32)
    with pytest.raises(Exception, match="bf16"):
        m32.set_fp8_gemm(True)
    m32.close()


def test_operator_surface_errors():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.bfloat16)
    img = torch.zeros(1, 1, 3, 384, 384)
    ids = torch.tensor([[5, 6, -200, 7]])
    with pytest.raises(NotImplementedError):
        m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], inputs_embeds=torch.zeros(1))
    with pytest.raises(NotImplementedError):
        m.generate(inputs=torch.tensor([[5]]), images=img, env_id=0, time_ids=[[0]])
    with pytest.raises(Exception):
        m.generate(inputs=torch.tensor([[5, -300, -200]]), images=img, env_id=0, time_ids=[[0]], max_new_tokens=1)   # <memory> without frames
    out = m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=2, eos_token_ids=[])
    assert out.sequences.shape == (1, 2)
    assert out.past_key_values.get_seq_length() == 3 + 196 + 2 - 1
    m.reset_for_env(0)
    with pytest.raises(ValueError):
        m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], past_key_values=out.past_key_values)   # stale handle
    m.close()


def _first_turn_inputs(m, sc, step=0, n_text=24, seed=3):
    from streamvln_amd.synthetic import synthetic_frame
    rng = np.random.default_rng(seed)
    ids = [int(t) for t in rng.integers(10, sc["cfg"].vocab, n_text)]
    ids.insert(n_text - 2, -200)
    img = m.get_vision_tower().image_processor.preprocess_array(synthetic_frame(0, step))[None, None].cuda()
    return torch.tensor([ids]), img


def test_ragged_turns_vs_live_oracle():
    """Ragged inputs of the splice (stream_video_vln.py:102-291), fp32 engine against the CPU oracle on the same inputs:
    (a) three frames and three <image> sentinels in ONE turn without memory (V != 1, time_ids[0][0] == 0: every view is an image);
    (b) a follow-up turn whose only new text is a single token before <image>; (c) a memory turn whose <memory> sentinel comes
    AFTER its <image>; (d) eos on the very first generated token (one new id, EOS kept, cache length L_total)."""
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    from streamvln_amd.synthetic import synthetic_frame
    sc = SCENARIOS["tiny_episode"]
    cfg = sc["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=1, max_frames=3, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = 2
    orc = O.OracleStreamVLN(cfg, util.synth_weights(cfg, SEED), num_history=2)
    pre = m.get_vision_tower().image_processor.preprocess_array
    frames = torch.stack([pre(synthetic_frame(0, s)) for s in range(5)])               # [5,3,384,384]

    def both(ids, imgs, time_ids, pkv_g, pkv_o, eos=()):
        g = m.generate(inputs=torch.tensor([ids]), images=imgs[None].cuda(), env_id=0, time_ids=time_ids, max_new_tokens=4, eos_token_ids=list(eos),
                       past_key_values=pkv_g)
        hg = m.last_hidden()
        o = orc.generate(inputs=np.array([ids]), images=imgs[None].cpu().numpy(), env_id=0, time_ids=time_ids, max_new_tokens=4, eos_token_ids=list(eos),
                         past_key_values=pkv_o)
        assert g.sequences[0].tolist() == o.sequences[0].tolist()
        assert np.abs(hg - o.hidden.numpy()).max() <= HIDDEN_TOL
        assert g.past_key_values.get_seq_length() == o.cache_len
        return g, o

    # (a) three images, no memory
    ids_a = [11, 12, -200, 13, -200, -200, 14, 15]
    g, o = both(ids_a, frames[:3], [[0, 1, 2]], None, None)
    assert g.past_key_values.get_seq_length() == 5 + 3 * 196 + 4 - 1
    # (b) single text token + image on top of the previous output
    ids_b = g.sequences[0].tolist() + [21, -200]
    g, o = both(ids_b, frames[3:4], [[0, 1, 2, 3]], g.past_key_values, o.past_key_values)
    # (c) window restart with history: <image> first, <memory> after it
    m.reset_for_env(0); orc.reset_for_env(0)
    ids_c = [31, -200, 32, -300, 33]
    g, o = both(ids_c, frames[[0, 2, 4]], [[4]], None, None)
    assert g.past_key_values.get_seq_length() == 3 + 196 + 2 * 196 + 4 - 1
    # (d) EOS on the first generated token
    first = g.sequences[0].tolist()[0]
    m.reset_for_env(0); orc.reset_for_env(0)
    g, o = both(ids_c, frames[[0, 2, 4]], [[4]], None, None, eos=(first,))
    assert g.sequences[0].tolist() == [first] and g.past_key_values.get_seq_length() == 3 + 3 * 196
    m.close()


def test_two_envs_are_isolated():
    """per-env state (embeds, KV pages): interleaving two envs gives each the outputs it has alone"""
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.float32, max_envs=2, max_frames=3, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = 2
    ids_a, img_a = _first_turn_inputs(m, sc, step=0, seed=3)
    ids_b, img_b = _first_turn_inputs(m, sc, step=5, seed=4)

    def two_turns(env, ids, img):
        o1 = m.generate(inputs=ids, images=img, env_id=env, time_ids=[[0]], max_new_tokens=3, eos_token_ids=[])
        ids2 = torch.cat([o1.sequences.cpu(), torch.tensor([[7, 8, -200, 9]])], 1)
        o2 = m.generate(inputs=ids2, images=img, env_id=env, time_ids=[[0, 1, 2, 3, 4]], max_new_tokens=3, eos_token_ids=[],
                        past_key_values=o1.past_key_values)
        return o1.sequences[0].tolist() + o2.sequences[0].tolist(), m.last_hidden()
    alone_a = two_turns(0, ids_a, img_a)
    m.reset_for_env(0)
    alone_b = two_turns(0, ids_b, img_b)
    m.reset(2)
    a1 = m.generate(inputs=ids_a, images=img_a, env_id=0, time_ids=[[0]], max_new_tokens=3, eos_token_ids=[])
    b1 = m.generate(inputs=ids_b, images=img_b, env_id=1, time_ids=[[0]], max_new_tokens=3, eos_token_ids=[])
    tail = torch.tensor([[7, 8, -200, 9]])
    a2 = m.generate(inputs=torch.cat([a1.sequences.cpu(), tail], 1), images=img_a, env_id=0, time_ids=[[0, 1, 2, 3, 4]], max_new_tokens=3,
                    eos_token_ids=[], past_key_values=a1.past_key_values)
    ha = m.last_hidden()
    b2 = m.generate(inputs=torch.cat([b1.sequences.cpu(), tail], 1), images=img_b, env_id=1, time_ids=[[0, 1, 2, 3, 4]], max_new_tokens=3,
                    eos_token_ids=[], past_key_values=b1.past_key_values)
    hb = m.last_hidden()
    assert a1.sequences[0].tolist() + a2.sequences[0].tolist() == alone_a[0]
    assert b1.sequences[0].tolist() + b2.sequences[0].tolist() == alone_b[0]
    assert np.array_equal(ha, alone_a[1]) and np.array_equal(hb, alone_b[1])
    with pytest.raises(ValueError):
        m.generate(inputs=ids_a, images=img_a, env_id=1, time_ids=[[0]], past_key_values=a2.past_key_values)   # handle of another env
    m.close()


def test_sequence_limit_is_an_error_not_a_fault():
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.bfloat16, max_envs=1, max_frames=3, max_positions=256)
    m.load_synthetic(SEED)
    ids, img = _first_turn_inputs(m, sc)
    out = m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=2, eos_token_ids=[])      # 24 + 196 rows fit
    from streamvln_amd._lib import SvlnError
    with pytest.raises(SvlnError):                                                                            # + 196 more do not
        m.generate(inputs=torch.cat([out.sequences.cpu(), ids], 1), images=img, env_id=0, time_ids=[[0, 1, 2, 3, 4]], max_new_tokens=2,
                   eos_token_ids=[], past_key_values=out.past_key_values)
    m.reset_for_env(0)
    out2 = m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=2, eos_token_ids=[])     # engine still usable
    assert out2.sequences.tolist() == out.sequences.tolist()
    m.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decode_path_equals_prefill_path(dtype):
    """size-independent property at true dimensions: tokens produced by the decode path (GEMV + split-KV attention with the
    fused RoPE/KV append, hipGraph replay) are reproduced by ONE prefill (MFMA GEMM + causal attention) over the same
    embeddings: teacher-forced arg-max at the last position == last generated token; kv_reset re-prefill == first token."""
    from streamvln_amd.config import TRUE1
    import ctypes as C
    sc = dict(SCENARIOS["true1_episode"])
    m = StreamVLNForCausalLM(TRUE1, dtype=dtype, max_envs=1, max_frames=9, max_positions=4096)
    m.load_synthetic(SEED)
    m.model.num_history = 8
    m.set_decode_graph(True)
    ids, img = _first_turn_inputs(m, sc, n_text=180)
    out = m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=5, eos_token_ids=[])
    toks = out.sequences[0].tolist()
    h_dec = m.last_hidden()
    assert out.past_key_values.get_seq_length() == 180 + 196 + 5 - 1
    lib, h = m._lib, m._h
    from streamvln_amd import _lib

    def regen(n_new):
        o = np.zeros(n_new, dtype=np.int64)
        n = C.c_int32()
        _lib.check(lib.svln_generate(h, 0, n_new, None, 0, o.ctypes.data_as(C.POINTER(C.c_int64)), n_new, C.byref(n)))
        return o[: n.value].tolist()
    _lib.check(lib.svln_kv_reset(h, 0))                         # past_key_values=None: re-prefill everything accumulated
    assert regen(1) == toks[:1]
    fed = np.asarray(toks[:4], dtype=np.int64)                  # teacher forcing: embeds of t0..t3 appended, one prefill of L+4 rows
    _lib.check(lib.svln_append_turn(h, 0, fed.ctypes.data_as(C.POINTER(C.c_int64)), 4, 0))
    _lib.check(lib.svln_kv_reset(h, 0))
    last = regen(1)
    h_pre = m.last_hidden()[0]
    rel = np.linalg.norm(h_pre - h_dec[4]) / np.linalg.norm(h_dec[4])
    if dtype == torch.float32:
        assert last == toks[4:5] and rel < 1e-4, (last, toks, rel)
    else:
        assert rel < 3e-2, rel
    m.close()


def test_full_size_determinism_and_graph_equivalence():
    """BASELINE full size (SigLIP-so400m + Qwen2-7B, bf16): two runs of the same turns agree bit for bit, with and without
    hipGraph replay of the decode step; KV pages recycled by reset_for_env give the same result as fresh ones."""
    from streamvln_amd.config import TRUE
    sc = dict(SCENARIOS["true1_episode"], cfg=TRUE)
    m = StreamVLNForCausalLM(TRUE, dtype=torch.bfloat16, max_envs=1, max_frames=9, max_positions=4096)
    m.load_synthetic(SEED)
    m.model.num_history = 8
    runs = []
    for graph in (True, False, True):
        m.set_decode_graph(graph)
        m.reset_for_env(0)
        ids, img = _first_turn_inputs(m, sc, n_text=180)
        o1 = m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=5, eos_token_ids=[])
        h1 = m.last_hidden()
        ids2 = torch.cat([o1.sequences.cpu(), torch.tensor([[11, 12, 13, -200, 14]])], 1)
        o2 = m.generate(inputs=ids2, images=img, env_id=0, time_ids=[[0, 1, 2, 3, 4]], max_new_tokens=5, eos_token_ids=[],
                        past_key_values=o1.past_key_values)
        runs.append((o1.sequences[0].tolist(), o2.sequences[0].tolist(), h1, m.last_hidden()))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1]
        assert np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3])
    assert np.isfinite(runs[0][3]).all()
    m.close()


def test_long_horizon_single_window_vs_live_oracle():
    """BASELINE configs[3] shape (64-step dialogue in ONE window = 16 turns, KV growing to ~3.4k positions) on the TINY model,
    fp32 engine against the CPU oracle run live on the same inputs: ids identical, hidden <= 1e-3 at every turn."""
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    from scenarios import run_scenario
    sc = dict(SCENARIOS["tiny_episode"], steps=64, num_frames=64, num_history=8, max_new=5, eos_mod=0, lens=(40, 48, 16))
    cfg = sc["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=1, max_frames=9, max_positions=4096)
    m.load_synthetic(SEED)
    m.model.num_history = 8
    hid = []
    pre = m.get_vision_tower().image_processor.preprocess_array
    log_g = run_scenario(m, sc, preprocess=pre, device="cuda", on_turn=lambda t, r: hid.append(m.last_hidden()))
    orc = O.OracleStreamVLN(cfg, util.synth_weights(cfg, SEED), num_history=8)
    log_o = run_scenario(orc, sc, preprocess=pre)
    assert len(log_g) == len(log_o) == 16
    for t, (a, b) in enumerate(zip(log_g, log_o)):
        assert a["out"].sequences[0].tolist() == b["out"].sequences[0].tolist(), t
        assert np.abs(hid[t] - b["out"].hidden.numpy()).max() <= HIDDEN_TOL, t
        assert a["out"].past_key_values.get_seq_length() == b["out"].cache_len
    # first turn 39 text + 196 image rows; every later turn 5 previous tokens + 15 text + 196 image rows; last EOS is not fed
    assert log_g[-1]["out"].past_key_values.get_seq_length() == 39 + 196 + 15 * (5 + 15 + 196) + 5 - 1
    m.close()


def test_memory_prune_extension_vs_live_oracle():
    """Opt-in slow-memory pruning (BASELINE configs[3]; NO reference counterpart, SURVEY a-13: parity unpinned -- pinned here against
    the project's own CPU restatement).  Tiny episode with two window restarts, `<memory>` = 40 of the 2 x 196 history tokens: the
    fp32 engine reproduces the oracle's ids / hidden / cache lengths, the memory turns shrink by exactly 392 - 40 rows, and
    keep = 0 restores the reference behaviour."""
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    from scenarios import run_scenario
    sc = SCENARIOS["tiny_episode"]
    cfg, keep = sc["cfg"], 40
    m = _model(sc, torch.float32)
    m.set_memory_prune(keep)
    hid = []
    pre = m.get_vision_tower().image_processor.preprocess_array
    log_g = run_scenario(m, sc, preprocess=pre, device="cuda", on_turn=lambda t, r: hid.append(m.last_hidden()))
    orc = O.OracleStreamVLN(cfg, util.synth_weights(cfg, SEED), num_history=sc["num_history"], memory_keep=keep)
    log_o = run_scenario(orc, sc, preprocess=pre)
    assert len(log_g) == len(log_o)
    mem_turns = 0
    for t, (a, b) in enumerate(zip(log_g, log_o)):
        assert a["out"].sequences[0].tolist() == b["out"].sequences[0].tolist(), t
        assert np.abs(hid[t] - b["out"].hidden.numpy()).max() <= HIDDEN_TOL, t
        assert a["out"].past_key_values.get_seq_length() == b["out"].cache_len, t
        mem_turns += int(a["memory"])
    assert mem_turns == 2
    # same episode without pruning: every memory turn is 2*196 - keep rows longer
    m.set_memory_prune(0)
    m.reset(1)
    log_full = run_scenario(m, sc, preprocess=pre, device="cuda")
    for a, f in zip(log_g, log_full):
        if a["memory"]:
            n_a, n_f = len(a["out"].sequences[0]), len(f["out"].sequences[0])
            assert f["out"].past_key_values.get_seq_length() - n_f == a["out"].past_key_values.get_seq_length() - n_a + 2 * 196 - keep
    m.close()


def test_config3_long_window_with_pruned_memory_vs_live_oracle():
    """BASELINE configs[3] in one piece ("64-step horizon, 16-frame window, 32-token pruned slow memory") on the TINY model: num_frames 64
    (a 16-turn window), num_history 8, `<memory>` pruned to 32 tokens, 72 env steps = the full first window (KV to ~3.4k positions), the
    window restart at step 64 (9 views, 8 x 196 memory tokens pruned to 32) and one turn after it.  fp32 engine vs the CPU oracle run live
    with the same extension (the prune rule has no reference counterpart): ids identical, hidden <= 1e-3, cache lengths equal."""
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    from scenarios import run_scenario
    sc = dict(SCENARIOS["tiny_episode"], steps=72, num_frames=64, num_history=8, max_new=5, eos_mod=0, lens=(40, 48, 16))
    cfg, keep = sc["cfg"], 32
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=1, max_frames=9, max_positions=4096)
    m.load_synthetic(SEED)
    m.model.num_history = 8
    m.set_memory_prune(keep)
    hid = []
    pre = m.get_vision_tower().image_processor.preprocess_array
    log_g = run_scenario(m, sc, preprocess=pre, device="cuda", on_turn=lambda t, r: hid.append(m.last_hidden()))
    orc = O.OracleStreamVLN(cfg, util.synth_weights(cfg, SEED), num_history=8, memory_keep=keep)
    log_o = run_scenario(orc, sc, preprocess=pre)
    assert len(log_g) == len(log_o) == 18
    for t, (a, b) in enumerate(zip(log_g, log_o)):
        assert a["out"].sequences[0].tolist() == b["out"].sequences[0].tolist(), t
        assert np.abs(hid[t] - b["out"].hidden.numpy()).max() <= HIDDEN_TOL, t
        assert a["out"].past_key_values.get_seq_length() == b["out"].cache_len, t
    restart = log_g[16]
    assert restart["memory"] and restart["views"] == 9 and restart["step_id"] == 64
    assert restart["out"].past_key_values.get_seq_length() == (48 - 2) + keep + 196 + 5 - 1        # 46 text + 32 pruned memory + 196 image rows
    m.close()


def test_eight_envs_round_robin_equal_their_solo_runs():
    """BASELINE configs[4] shape (8 concurrent envs on one GPU): turns of 8 envs interleaved round-robin; every env reproduces
    the token ids it produces when it runs alone (per-env semantics = the batch-1 path)."""
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.bfloat16, max_envs=8, max_frames=3, max_positions=1024)
    m.load_synthetic(SEED)
    m.model.num_history = 2
    tail = torch.tensor([[7, 8, -200, 9]])
    inputs = [_first_turn_inputs(m, sc, step=e, seed=10 + e) for e in range(8)]
    solo = []
    for e in range(8):
        m.reset_for_env(0)
        ids, img = inputs[e]
        o1 = m.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=3, eos_token_ids=[])
        o2 = m.generate(inputs=torch.cat([o1.sequences.cpu(), tail], 1), images=img, env_id=0, time_ids=[[0, 1, 2, 3, 4]],
                        max_new_tokens=3, eos_token_ids=[], past_key_values=o1.past_key_values)
        solo.append(o1.sequences[0].tolist() + o2.sequences[0].tolist())
    m.reset(8)
    first = [m.generate(inputs=inputs[e][0], images=inputs[e][1], env_id=e, time_ids=[[0]], max_new_tokens=3, eos_token_ids=[])
             for e in range(8)]
    second = [m.generate(inputs=torch.cat([first[e].sequences.cpu(), tail], 1), images=inputs[e][1], env_id=e,
                         time_ids=[[0, 1, 2, 3, 4]], max_new_tokens=3, eos_token_ids=[], past_key_values=first[e].past_key_values)
              for e in range(8)]
    for e in range(8):
        assert first[e].sequences[0].tolist() + second[e].sequences[0].tolist() == solo[e], e
    m.close()


def test_from_pretrained_safetensors_equals_synthetic(tmp_path):
    """checkpoint ingestion (HF state-dict names, bf16 safetensors shards) gives the same engine as on-device synthesis"""
    from safetensors.torch import save_file
    from streamvln_amd import weights as W
    sc = SCENARIOS["tiny_episode"]
    cfg = sc["cfg"]
    sd = {k: torch.from_numpy(v).to(torch.bfloat16) for k, v in util.synth_weights(cfg, SEED).items()}
    names = sorted(sd)
    save_file({k: sd[k] for k in names[: len(names) // 2]}, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file({k: sd[k] for k in names[len(names) // 2:]}, str(tmp_path / "model-00002-of-00002.safetensors"))
    a = StreamVLNForCausalLM.from_pretrained(str(tmp_path), config=cfg, torch_dtype=torch.bfloat16, max_frames=3, max_positions=1024)
    b = _model(sc, torch.bfloat16)
    for n in ("model.layers.1.mlp.up_proj.weight", "model.layers.0.self_attn.k_proj.bias", "lm_head.weight"):
        assert np.array_equal(a.get_tensor(n), b.get_tensor(n)), n
    ids, img = _first_turn_inputs(a, sc)
    oa = a.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=4, eos_token_ids=[])
    ob = b.generate(inputs=ids, images=img, env_id=0, time_ids=[[0]], max_new_tokens=4, eos_token_ids=[])
    assert oa.sequences.tolist() == ob.sequences.tolist() and np.array_equal(a.last_hidden(), b.last_hidden())
    with pytest.raises(Exception):
        StreamVLNForCausalLM.from_pretrained(str(tmp_path / "missing"), config=cfg)
    a.close(); b.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batched_lockstep_envs_equal_solo_runs(dtype):
    """BASELINE configs[4] (concurrent envs on one GPU, build-side extension): 5 envs stepped in lockstep through
    `generate_batch` (batched prefill rows, batched decode steps, padded to 8 slots, grouped frame encodes incl. a <memory>
    window restart) reproduce the ids every env gets from the batch-1 path; fp32: hidden within 1e-3."""
    from streamvln_amd.agent import BatchedAgents, StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    sc = SCENARIOS["tiny_episode"]
    cfg, n_env, steps = sc["cfg"], 5, 16
    m = StreamVLNForCausalLM(cfg, dtype=dtype, max_envs=n_env, max_frames=7, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    pre = m.get_vision_tower().image_processor.preprocess_array
    eos = eos_ids(sc)

    def make(e):
        enc = SyntheticPromptEncoder(cfg, seed=100 + e, first_len=40, memory_len=48, later_len=16)
        return StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=4, num_history=sc["num_history"], env_id=e,
                              device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos, preprocess=pre)
    solo, solo_hid = [], []
    for e in range(n_env):
        ag, hid = make(e), []
        for s in range(steps):
            n0 = len(ag.turn_log)
            ag.act(synthetic_frame(e, s))
            if len(ag.turn_log) > n0:
                hid.append(m.last_hidden())
        solo.append([t["out"].sequences[0].tolist() for t in ag.turn_log])
        solo_hid.append(hid)
    m.reset(n_env)
    agents = [make(e) for e in range(n_env)]
    batch = BatchedAgents(agents)
    bat_hid = [[] for _ in range(n_env)]
    for s in range(steps):
        n0 = len(agents[0].turn_log)
        batch.act([synthetic_frame(e, s) for e in range(n_env)])
        if len(agents[0].turn_log) > n0:
            for e in range(n_env):
                bat_hid[e].append(m.last_hidden_batch(e))
    agree = total = 0
    for e in range(n_env):
        got = [t["out"].sequences[0].tolist() for t in agents[e].turn_log]
        assert len(got) == len(solo[e]) == 4 and [t["views"] for t in agents[e].turn_log] == [1, 1, 1, 3]
        for t in range(4):
            if dtype == torch.float32:
                assert got[t] == solo[e][t], (e, t, got[t], solo[e][t])
                assert np.abs(bat_hid[e][t] - solo_hid[e][t]).max() <= HIDDEN_TOL, (e, t)
            else:
                total += 1
                agree += int(got[t][0] == solo[e][t][0])
                rel = np.linalg.norm(bat_hid[e][t][0] - solo_hid[e][t][0]) / np.linalg.norm(solo_hid[e][t][0])
                assert rel < 3e-2, (e, t, rel)
    assert dtype == torch.float32 or agree >= total - 2, (agree, total)
    with pytest.raises(ValueError):
        req = agents[0]._build_request("")
        m.generate_batch([req, dict(req)])                      # duplicate env
    m.close()


# ----------------------------------------------------------------------------------------------- multi-env turns vs the ORACLE
def _oracle_env_logs(sc, n_envs, lengths, n_turns, env_steps=None):
    """every env alone on the CPU oracle: same prompts (seed 7 + 31 e), same frames (env e's stream), same action-count rule"""
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    from streamvln_amd.agent import StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    cfg = sc["cfg"]
    sd = util.synth_weights(cfg, SEED)
    def solo(e):
        orc = O.OracleStreamVLN(cfg, sd, num_history=sc["num_history"])
        enc = SyntheticPromptEncoder(cfg, seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        ag = StreamingAgent(orc, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"],
                            max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb)))
        ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
        while len(ag.turn_log) < n_turns[e]:
            ag.act(synthetic_frame(e, ag.step_id))
        return ag.turn_log
    # the envs are independent CPU jobs (the box has 128 host threads; torch releases the GIL inside its operators)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(n_envs, 8)) as ex:
        logs = list(ex.map(solo, range(n_envs)))
    return logs


def test_ragged_multi_env_scheduler_vs_oracle():
    """SURVEY 8f-1 / streamvln_dagger.py:232-313: 8 envs on one GPU whose model turns fall due at different times (staggered starts,
    2 or 4 env steps per turn depending on env and turn), driven through submit / step_batch: envs prefill a new turn (incl. window
    restarts with a <memory> block) in the same weight pass in which others decode.  Every env must reproduce what it produces ALONE
    on the fp32 CPU oracle: ids identical, hidden <= 1e-3, cache lengths equal."""
    from streamvln_amd.agent import AsyncBatchedAgents, StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    sc = SCENARIOS["tiny_episode"]
    cfg, N = sc["cfg"], 8
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=N, max_frames=3, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    proc = m.get_vision_tower().image_processor
    lengths = lambda e, t: 2 if (e + t) % 2 == 0 else 4            # env steps until env e's next model turn: keeps 12 | turn steps
    agents = []
    for e in range(N):
        enc = SyntheticPromptEncoder(cfg, seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        ag = StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                            device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=proc.preprocess_array)
        ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
        agents.append(ag)
    hidden = [[] for _ in range(N)]

    def on_result(i, ticket, out):
        hidden[i].append(m.last_hidden_batch(ticket.slot))
    group = AsyncBatchedAgents(agents, on_result=on_result)
    for tick in range(64):
        active = {i for i in range(N) if tick >= i}               # env i starts one tick after env i-1
        group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active=active)
    n_turns = [len(a.turn_log) for a in agents]
    st = group.stats
    assert min(n_turns) >= 4 and any(r["memory"] for a in agents for r in a.turn_log), n_turns      # window restarts happened
    assert st["max_in_flight"] >= 4 and st["mixed_iterations"] >= 8, st              # prefilling and decoding envs shared weight passes
    logs_o = _oracle_env_logs(sc, N, lengths, n_turns)
    worst = 0.0
    for e in range(N):
        for t, (g, o) in enumerate(zip(agents[e].turn_log, logs_o[e])):
            assert g["step_id"] == o["step_id"] and g["views"] == o["views"] and g["memory"] == o["memory"], (e, t)
            assert g["out"].sequences[0].tolist() == o["out"].sequences[0].tolist(), (e, t)
            assert g["out"].past_key_values.get_seq_length() == o["out"].cache_len, (e, t)
            ho = o["out"].hidden.numpy()
            hg = hidden[e][t]
            k = min(len(hg), len(ho))
            err = float(np.abs(hg[:k] - ho[:k]).max())
            worst = max(worst, err)
            assert err <= HIDDEN_TOL, (e, t, err)
    print(f"ragged scheduler: {sum(n_turns)} turns of {N} envs vs the oracle, ids identical, worst hidden err {worst:.2e}, {st}")
    m.close()


def test_eight_env_lockstep_generate_batch_vs_oracle():
    """BASELINE configs[4] shape: 8 envs stepped in lockstep through generate_batch (what bench.py's batched pass runs), fp32 TINY,
    against 8 solo oracle envs: ids identical, hidden <= 1e-3 -- through two window restarts."""
    from streamvln_amd.agent import BatchedAgents, StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    sc = SCENARIOS["tiny_episode"]
    cfg, N = sc["cfg"], 8
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=N, max_frames=3 * N, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    proc = m.get_vision_tower().image_processor
    agents = []
    for e in range(N):
        enc = SyntheticPromptEncoder(cfg, seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        agents.append(StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                                     device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=proc.preprocess_array))
    group = BatchedAgents(agents)
    hidden = [[] for _ in range(N)]
    for step in range(28):
        n0 = len(agents[0].turn_log)
        group.act([synthetic_frame(e, step) for e in range(N)])
        if len(agents[0].turn_log) > n0:
            for e in range(N):
                hidden[e].append(m.last_hidden_batch(e))
    n_turns = [len(a.turn_log) for a in agents]
    assert n_turns == [7] * N
    logs_o = _oracle_env_logs(sc, N, lambda e, t: 4, n_turns)
    for e in range(N):
        for t, (g, o) in enumerate(zip(agents[e].turn_log, logs_o[e])):
            assert g["out"].sequences[0].tolist() == o["out"].sequences[0].tolist(), (e, t)
            ho, hg = o["out"].hidden.numpy(), hidden[e][t]
            k = min(len(hg), len(ho))
            assert np.abs(hg[:k] - ho[:k]).max() <= HIDDEN_TOL, (e, t)
            assert g["out"].past_key_values.get_seq_length() == o["out"].cache_len, (e, t)
    m.close()


# ----------------------------------------------------------------------------------------------- boundary edges (round 3)
def test_repetition_penalty_solo_batch_and_scheduler_agree_with_oracle():
    """generation_config.repetition_penalty through all three execution paths -- svln_generate (device-side greedy loop, graph replay on
    and off), generate_batch and submit / step_batch -- against the CPU oracle (transformers' formula, pinned in tiny_penalty.npz):
    ids identical.  Switching the penalty back to 1 restores the unpenalised fixture."""
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    sc = SCENARIOS["tiny_episode"]
    cfg, NE, pen = sc["cfg"], 4, 1.3
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=NE, max_frames=NE, max_positions=1024)
    m.load_synthetic(SEED)
    m.model.num_history = 2
    m.generation_config.repetition_penalty = pen
    orc = O.OracleStreamVLN(cfg, util.synth_weights(cfg, SEED), num_history=2)
    orc.generation_config.repetition_penalty = pen
    reqs, exp = [], []
    for e in range(NE):
        ids, img = _first_turn_inputs(m, sc, step=e, seed=40 + e)
        reqs.append(dict(inputs=ids, images=img, env_id=e, time_ids=[[0]]))
        orc.reset(1)
        exp.append(orc.generate(inputs=ids.numpy(), images=img.cpu().numpy(), env_id=0, time_ids=[[0]], max_new_tokens=6).sequences[0].tolist())
    assert any(len(set(x)) == len(x) for x in exp)
    for graph in (True, False):
        m.set_decode_graph(graph)
        m.reset(NE)
        for e in range(NE):
            got = m.generate(max_new_tokens=6, eos_token_ids=[], **reqs[e]).sequences[0].tolist()
            assert got == exp[e], ("solo", graph, e, got, exp[e])
    m.reset(NE)
    outs = m.generate_batch(reqs, max_new_tokens=6, eos_token_ids=[])
    for e in range(NE):
        assert outs[e].sequences[0].tolist() == exp[e], ("batch", e)
    m.reset(NE)
    tickets = [m.submit(max_new_tokens=6, eos_token_ids=[], **reqs[e]) for e in range(2)]          # two envs start ...
    done, running = m.step_batch()
    tickets += [m.submit(max_new_tokens=6, eos_token_ids=[], **reqs[e]) for e in range(2, NE)]    # ... two join while they decode
    res = {}
    while True:
        done, running = m.step_batch()
        for tk, out in done:
            res[tk.env_id] = out.sequences[0].tolist()
        if running == 0:
            break
    assert [res[e] for e in range(NE)] == exp
    # penalty off again: the unpenalised ids of the same request differ and repeat
    m.generation_config.repetition_penalty = 1.0
    m.reset(NE)
    orc.generation_config.repetition_penalty = 1.0
    orc.reset(1)
    plain = orc.generate(inputs=reqs[0]["inputs"].numpy(), images=reqs[0]["images"].cpu().numpy(), env_id=0, time_ids=[[0]], max_new_tokens=6).sequences[0].tolist()
    assert m.generate(max_new_tokens=6, eos_token_ids=[], **reqs[0]).sequences[0].tolist() == plain
    # ... and ON again (P -> 1 -> P): the unpenalised generate above rewrote the engine's id ring without touching the flags
    # of the last penalised turn; those flags must not leak into this one.  Solo (graph on / off) and scheduler paths vs the oracle.
    m.generation_config.repetition_penalty = pen
    for graph in (True, False):
        m.set_decode_graph(graph)
        m.reset(NE)
        for e in (1, 0):
            got = m.generate(max_new_tokens=6, eos_token_ids=[], **reqs[e]).sequences[0].tolist()
            assert got == exp[e], ("solo, penalty off -> on", graph, e, got, exp[e])
    m.reset(NE)
    outs = m.generate_batch(reqs, max_new_tokens=6, eos_token_ids=[])
    for e in range(NE):
        assert outs[e].sequences[0].tolist() == exp[e], ("batch, penalty off -> on", e)
    # a penalty change while scheduler turns are in flight is refused, not ignored; the row limit may change at any call
    m.reset(NE)
    tk = m.submit(max_new_tokens=6, eos_token_ids=[], **reqs[0])
    m.generation_config.repetition_penalty = 1.0
    with pytest.raises(RuntimeError, match="in flight"):
        m.submit(max_new_tokens=6, eos_token_ids=[], **reqs[1])
    m.generation_config.repetition_penalty = pen
    m.config.tokenizer_model_max_length = 0
    with pytest.raises(ValueError, match="tokenizer_model_max_length"):
        m.submit(max_new_tokens=6, eos_token_ids=[], **reqs[1])
    m.config.tokenizer_model_max_length = None
    m.cancel(tk)
    m.close()


def test_scheduler_survives_resets_cancels_and_failed_steps():
    """an env reset with a turn in flight, a failing iteration and a refused submit must leave the engine usable and the
    envs unchanged: (a) reset_for_env drops the env's submitted turn; (b) a refused submit (env already in flight) leaves curr_t and
    the env's rows untouched; (c) cancel() frees the slots; (d) a prefill of exactly max_positions rows runs through generate_batch."""
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.float32, max_envs=3, max_frames=3, max_positions=512)
    m.load_synthetic(SEED)
    m.model.num_history = 2
    reqs = []
    for e in range(3):
        ids, img = _first_turn_inputs(m, sc, step=e, seed=60 + e)
        reqs.append(dict(inputs=ids, images=img, env_id=e, time_ids=[[0]], max_new_tokens=3, eos_token_ids=[]))
    solo = []
    for e in range(3):
        solo.append(m.generate(**reqs[e]).sequences[0].tolist())
    m.reset(3)
    # (a) env 0 submitted, then reset before any step: the scheduler must not run it; envs 1, 2 finish normally
    t0 = m.submit(**reqs[0])
    m.reset_for_env(0)
    t1, t2 = m.submit(**reqs[1]), m.submit(**reqs[2])
    res = {}
    for _ in range(8):
        done, running = m.step_batch()
        for tk, out in done:
            res[tk.env_id] = out.sequences[0].tolist()
        if running == 0:
            break
    assert res == {1: solo[1], 2: solo[2]}
    # (b) a second submit for an env in flight is refused before the env changes
    m.reset(3)
    tk = m.submit(**reqs[0])
    before = (m.curr_t[0], m.env_state(0))
    with pytest.raises(RuntimeError, match="in flight"):
        m.submit(**reqs[0])
    assert (m.curr_t[0], m.env_state(0)) == before
    # (c) cancel frees the slot; the env is reset and runs again alone
    m.cancel(tk)
    m.reset_for_env(0)
    assert m.generate(**reqs[0]).sequences[0].tolist() == solo[0]
    # generate_batch refuses while a submitted turn is pending, and works after cancel()
    m.reset(3)
    m.submit(**reqs[1])
    with pytest.raises(RuntimeError, match="idle scheduler"):
        m.generate_batch([reqs[0], reqs[2]])
    m.cancel()
    m.reset(3)
    outs = m.generate_batch([dict(r) for r in reqs])
    assert [o.sequences[0].tolist() for o in outs] == solo
    # (d) a turn that fills the engine to max_positions exactly: 512 = 316 text + 196 image rows (generate_batch used to stop at 504)
    m.reset(3)
    rng = np.random.default_rng(5)
    ids = [int(t) for t in rng.integers(10, sc["cfg"].vocab, 316)]
    ids.insert(300, -200)
    big = dict(inputs=torch.tensor([ids]), images=reqs[0]["images"], env_id=0, time_ids=[[0]], max_new_tokens=1, eos_token_ids=[])
    a = m.generate_batch([dict(big)])[0].sequences[0].tolist()
    m.reset(3)
    b = m.generate(**big).sequences[0].tolist()
    assert a == b and m.env_state(0)[0] == 512
    m.close()


def test_generation_config_keys(tmp_path):
    """from_pretrained: eos ids and repetition_penalty of generation_config.json are honoured, sampling knobs (inert under the
    harness's do_sample=False) are ignored, anything else that changes greedy decoding raises; config.json's
    tokenizer_model_max_length becomes the per-turn row limit."""
    import json
    from safetensors.torch import save_file
    from streamvln_amd import weights as W
    sc = SCENARIOS["tiny_episode"]
    cfg = sc["cfg"]
    sd = {k: torch.from_numpy(v).to(torch.bfloat16) for k, v in util.synth_weights(cfg, SEED).items()}
    save_file(sd, str(tmp_path / "model.safetensors"))
    json.dump({"do_sample": True, "temperature": 0.7, "top_p": 0.8, "top_k": 20, "repetition_penalty": 1.05, "eos_token_id": [7, 9],
               "bos_token_id": 1, "pad_token_id": 1}, open(tmp_path / "generation_config.json", "w"))
    m = StreamVLNForCausalLM.from_pretrained(str(tmp_path), config=cfg, torch_dtype=torch.bfloat16, max_frames=3, max_positions=1024)
    assert m.generation_config.eos_token_id == [7, 9] and m.generation_config.repetition_penalty == 1.05
    m.close()
    json.dump({"no_repeat_ngram_size": 3, "eos_token_id": 7}, open(tmp_path / "generation_config.json", "w"))
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        StreamVLNForCausalLM.from_pretrained(str(tmp_path), config=cfg, torch_dtype=torch.bfloat16, max_frames=3, max_positions=1024)


def test_config0_window_16_4_4_vs_live_oracle():
    """BASELINE configs[0]'s window (num_frames 16 / num_future_steps 4 / num_history 4: the reference's CPU-runnable plumbing case) on the
    TINY model: 40 env steps = 10 turns, window restarts at steps 16 and 32 with a 4-frame <memory> block (5 views).  fp32 engine vs the
    CPU oracle run live: ids identical, hidden <= 1e-3, cache lengths equal."""
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    sc = dict(SCENARIOS["tiny_episode"], steps=40, num_frames=16, nfs=4, num_history=4, max_new=5, eos_mod=3)
    cfg = sc["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=1, max_frames=5, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = 4
    hid = []
    pre = m.get_vision_tower().image_processor.preprocess_array
    log_g = run_scenario(m, sc, preprocess=pre, device="cuda", on_turn=lambda t, r: hid.append(m.last_hidden()))
    orc = O.OracleStreamVLN(cfg, util.synth_weights(cfg, SEED), num_history=4)
    log_o = run_scenario(orc, sc, preprocess=pre)
    assert len(log_g) == len(log_o) == 10
    assert [r["views"] for r in log_g] == [1, 1, 1, 1, 5, 1, 1, 1, 5, 1] and [bool(r["memory"]) for r in log_g] == [v == 5 for v in [1, 1, 1, 1, 5, 1, 1, 1, 5, 1]]
    for t, (a, b) in enumerate(zip(log_g, log_o)):
        assert a["out"].sequences[0].tolist() == b["out"].sequences[0].tolist(), t
        assert np.abs(hid[t] - b["out"].hidden.numpy()).max() <= HIDDEN_TOL, t
        assert a["out"].past_key_values.get_seq_length() == b["out"].cache_len, t
    m.close()


# bf16 relative L2 bound of the final-norm hidden rows at the benchmarked depth (26 ViT + 28 LLM layers); measured value printed and
# recorded in DESIGN.md section 6
BF16_FULL_DEPTH_REL = 3e-2


def test_full_depth_true_size_vs_live_oracle():
    """The benchmarked instantiation itself (SigLIP 26 layers + Qwen2 28 layers at true width, vocabulary 152 064) against the fp32 CPU
    oracle run live on the box: first turn (T = 376) + one steady turn (T = 214), 3 tokens each.  fp32 engine: ids identical, hidden
    <= 1e-3 (the north-star bar); bf16 engine (what bench.py measures): every comparable hidden row under BF16_FULL_DEPTH_REL and ids
    equal wherever the oracle's top-2 margin exceeds BF16_MARGIN.  (stream_video_vln.py:353-407 + the Qwen2 equations of SURVEY a-10.)"""
    import time
    from oracle import streamvln_oracle as O
    from streamvln_amd import weights as W
    from streamvln_amd.config import TRUE
    sc = dict(SCENARIOS["true4_episode"], cfg=TRUE, steps=8, max_new=3)
    t0 = time.time()
    from util import synth_weights
    sd = synth_weights(TRUE, SEED)                     # (kept for the session: tests/test_fp8_gpu.py runs the emulating oracle on the same weights)
    t_w = time.time() - t0
    orc = O.OracleStreamVLN(TRUE, sd, num_history=8)
    pre_cpu = lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb))
    t0 = time.time()
    log_o = run_scenario(orc, sc, preprocess=pre_cpu)
    t_o = time.time() - t0
    exp = [(r["out"].sequences[0].tolist(), r["out"].hidden.numpy().copy(), list(r["out"].margins), r["out"].cache_len) for r in log_o]
    del orc, sd, log_o
    import gc
    gc.collect()
    assert len(exp) == 2
    report = {}
    for dtype in (torch.float32, torch.bfloat16):
        m = StreamVLNForCausalLM(TRUE, dtype=dtype, max_envs=1, max_frames=9, max_positions=4096)
        m.load_synthetic(SEED)
        m.model.num_history = 8
        log, taps = _run(m, sc)
        worst_abs = worst_rel = 0.0
        for t, rec in enumerate(log):
            ids, (gold, gh, margins, clen) = rec["out"].sequences[0].tolist(), exp[t]
            h = taps[t]["hidden"]
            if dtype == torch.float32:
                assert ids == gold, (t, ids, gold, margins)
                err = float(np.abs(h - gh).max())
                worst_abs = max(worst_abs, err)
                assert err <= HIDDEN_TOL, (t, err)
                assert taps[t]["cache_len"] == clen
            else:
                n = 0
                while n < min(len(ids), len(gold)) and ids[n] == gold[n]:
                    n += 1
                for j in range(min(n + 1, len(gold), len(ids))):
                    rel = float(np.linalg.norm(h[j] - gh[j]) / np.linalg.norm(gh[j]))
                    worst_rel = max(worst_rel, rel)
                    assert rel < BF16_FULL_DEPTH_REL, (t, j, rel)
                    if margins[j] > BF16_MARGIN:
                        assert ids[j] == gold[j], (t, j, ids, gold, margins)
                if n < len(gold):
                    break
        report[str(dtype)] = worst_abs if dtype == torch.float32 else worst_rel
        m.close()
    line = (f"full depth (26 + 28 layers, true width) vs the live CPU oracle: fp32 worst |hidden err| {report['torch.float32']:.2e}, "
            f"bf16 worst rel L2 {report['torch.bfloat16']:.2e}; oracle ids {[e[0] for e in exp]}, margins {[[round(x, 3) for x in e[2]] for e in exp]}; "
            f"weights {t_w:.0f} s, oracle {t_o:.0f} s")
    print(line)
    _note("full_depth_parity", line)


def test_full_depth_restart_turn_bf16_vs_fp32_engine():
    """The window-restart turn of the benchmarked instantiation (26 + 28 layers, true width; 9-frame ViT batch, 1568-row <memory> block,
    T = 1952) is too slow for the CPU oracle, but the fp32 engine is oracle-verified at depth 28 (T = 376 / 214, the test above) and at
    T = 1952 (true1_episode, depth 1), and it runs different GEMM kernels (stage ring, fp32 MFMA) from the bf16 engine (8-phase 256x256
    schedule on 16x16x32 MFMAs, two K slices for down_proj, 128x128 tiles for o_proj).  Here both engines run the same 9 turns through
    the restart on identical inputs: the fp32 engine's calls are recorded and replayed on the bf16 engine, one token per turn so that
    no generated token is ever fed (a low-margin flip of the bf16 arg-max cannot put the two caches on different tokens).  Every turn's
    hidden row within BF16_FULL_DEPTH_REL of the fp32 engine's, ids equal wherever the fp32 top-2 logit margin (lm_head applied on the
    host to the fp32 hidden row) exceeds BF16_MARGIN."""
    from streamvln_amd import weights as W
    from streamvln_amd.config import TRUE
    sc = dict(SCENARIOS["true1_episode"], cfg=TRUE, steps=36, max_new=1, eos_mod=0)
    calls = []

    class Recorder:
        def __init__(self, m):
            self.m = m

        def __getattr__(self, k):
            return getattr(self.m, k)

        def reset_for_env(self, i):
            calls.append(("reset", i))
            return self.m.reset_for_env(i)

        def generate(self, **kw):
            out = self.m.generate(**kw)
            calls.append(("generate", {k: kw[k] for k in ("inputs", "images", "env_id", "time_ids", "max_new_tokens", "eos_token_ids")},
                          kw["past_key_values"] is None, out.sequences[0].tolist(), self.m.last_hidden()[0].copy()))
            return out
    m32 = StreamVLNForCausalLM(TRUE, dtype=torch.float32, max_envs=1, max_frames=9, max_positions=4096)
    m32.load_synthetic(SEED)
    m32.model.num_history = 8
    log = run_scenario(Recorder(m32), sc, preprocess=m32.get_vision_tower().image_processor.preprocess_array, device="cuda")
    assert len(log) == 9 and log[8]["views"] == 9 and log[8]["memory"]
    m32.close()
    lm_head = torch.from_numpy(W.synth_state_dict(TRUE, SEED, only=["lm_head.weight"], workers=16)["lm_head.weight"])
    m16 = StreamVLNForCausalLM(TRUE, dtype=torch.bfloat16, max_envs=1, max_frames=9, max_positions=4096)
    m16.load_synthetic(SEED)
    m16.model.num_history = 8
    past, t, worst, asserted, rels = None, 0, 0.0, 0, []
    for c in calls:
        if c[0] == "reset":
            m16.reset_for_env(c[1])
            past = None
            continue
        _, kw, fresh, ids32, h32 = c
        out = m16.generate(past_key_values=None if fresh else past, **kw)
        past = out.past_key_values
        h16 = m16.last_hidden()[0]
        rel = float(np.linalg.norm(h16 - h32) / np.linalg.norm(h32))
        rels.append(round(rel, 4))
        worst = max(worst, rel)
        assert rel < BF16_FULL_DEPTH_REL, (t, rel)
        top2 = torch.topk(lm_head @ torch.from_numpy(h32), 2)
        assert int(top2.indices[0]) == ids32[0], (t, "host lm_head disagrees with the fp32 engine", ids32, top2)
        if float(top2.values[0] - top2.values[1]) > BF16_MARGIN:
            assert out.sequences[0].tolist() == ids32, (t, out.sequences[0].tolist(), ids32, float(top2.values[0] - top2.values[1]))
            asserted += 1
        t += 1
    assert t == 9
    ne, kl = m16.env_state(0)
    assert ne == kl and ne >= 1952                               # the restart turn's rows are in the env; one token per turn: nothing fed beyond them
    m16.close()
    line = (f"full depth, 9 turns through the window restart (T = 1952, 9-frame ViT), bf16 engine vs fp32 engine on identical inputs: hidden rel L2 per turn "
            f"{rels} (restart turn last), worst {worst:.4f} < {BF16_FULL_DEPTH_REL}; {asserted} of 9 ids had fp32 margin > {BF16_MARGIN} and agree")
    print(line)
    _note("full_depth_parity", line)


# ----------------------------------------------------------------------------------------------- f-1 / f-2 at TRUE width (round 3)
def _true1_multi():
    """TRUE1 (true widths, 1 ViT + 1 LLM layer) with a short window so that a <memory> restart happens within three turns"""
    from streamvln_amd.config import TRUE1
    return dict(cfg=TRUE1, steps=12, num_frames=8, nfs=4, num_history=2, max_new=3, eos_mod=0, lens=(60, 70, 16))


def test_eight_env_lockstep_true_width_vs_oracle():
    """f-1 at H = 3584 (bench.py's batched pass runs at this width): 8 envs stepped in lockstep through generate_batch on the fp32
    engine, every env against its own solo CPU-oracle run: ids identical, hidden <= 1e-3, through a window restart with a 2-frame
    <memory> block (batched prefill rows of 8 envs: 256x256 tiles; 32-row MFMA decode products; batched lm_head)."""
    from streamvln_amd.agent import BatchedAgents, StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    sc = _true1_multi()
    cfg, N = sc["cfg"], 8
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=N, max_frames=3 * N, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    proc = m.get_vision_tower().image_processor
    agents = []
    for e in range(N):
        enc = SyntheticPromptEncoder(cfg, seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        agents.append(StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                                     device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=(), preprocess=proc.preprocess_array))
    group = BatchedAgents(agents)
    hidden = [[] for _ in range(N)]
    for step in range(sc["steps"]):
        n0 = len(agents[0].turn_log)
        group.act([synthetic_frame(e, step) for e in range(N)])
        if len(agents[0].turn_log) > n0:
            for e in range(N):
                hidden[e].append(m.last_hidden_batch(e))
    n_turns = [len(a.turn_log) for a in agents]
    assert n_turns == [3] * N and all(a.turn_log[2]["memory"] and a.turn_log[2]["views"] == 3 for a in agents)
    logs_o = _oracle_env_logs(sc, N, lambda e, t: 4, n_turns)
    worst = 0.0
    for e in range(N):
        for t, (g, o) in enumerate(zip(agents[e].turn_log, logs_o[e])):
            assert g["out"].sequences[0].tolist() == o["out"].sequences[0].tolist(), (e, t)
            ho, hg = o["out"].hidden.numpy(), hidden[e][t]
            k = min(len(hg), len(ho))
            worst = max(worst, float(np.abs(hg[:k] - ho[:k]).max()))
            assert np.abs(hg[:k] - ho[:k]).max() <= HIDDEN_TOL, (e, t)
            assert g["out"].past_key_values.get_seq_length() == o["out"].cache_len, (e, t)
    _note("multi_env_true_width", f"8-env lockstep at true width (TRUE1, fp32) vs solo oracle envs: ids identical, worst hidden err {worst:.2e}")
    m.close()


def test_ragged_scheduler_true_width_vs_oracle():
    """f-1 at H = 3584, ragged: 4 envs with staggered starts and 2- or 4-step turn cadences through submit / step_batch (prefilling envs
    share weight passes with decoding ones), each against its solo CPU-oracle run: ids identical, hidden <= 1e-3."""
    from streamvln_amd.agent import AsyncBatchedAgents, StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    sc = _true1_multi()
    cfg, N = sc["cfg"], 4
    m = StreamVLNForCausalLM(cfg, dtype=torch.float32, max_envs=N, max_frames=3, max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    proc = m.get_vision_tower().image_processor
    lengths = lambda e, t: (2, 2, 4)[(e + t) % 3]                  # env steps until the env's next turn: every 8th step (the window) is a turn step
    agents = []
    for e in range(N):
        enc = SyntheticPromptEncoder(cfg, seed=7 + 31 * e, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        ag = StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=e,
                            device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=(), preprocess=proc.preprocess_array)
        ag.decode_actions = lambda ids, ag=ag, e=e: [1] * lengths(e, len(ag.turn_log) - 1)
        agents.append(ag)
    hidden = [[] for _ in range(N)]
    group = AsyncBatchedAgents(agents, on_result=lambda i, ticket, out: hidden[i].append(m.last_hidden_batch(ticket.slot)))
    for tick in range(36):
        group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active={i for i in range(N) if tick >= 2 * i})
    n_turns = [len(a.turn_log) for a in agents]
    st = group.stats
    assert min(n_turns) >= 3 and any(r["memory"] for a in agents for r in a.turn_log), n_turns
    assert st["mixed_iterations"] >= 3, st
    logs_o = _oracle_env_logs(sc, N, lengths, n_turns)
    worst = 0.0
    for e in range(N):
        for t, (g, o) in enumerate(zip(agents[e].turn_log, logs_o[e])):
            assert g["step_id"] == o["step_id"] and g["views"] == o["views"] and g["memory"] == o["memory"], (e, t)
            assert g["out"].sequences[0].tolist() == o["out"].sequences[0].tolist(), (e, t)
            assert g["out"].past_key_values.get_seq_length() == o["out"].cache_len, (e, t)
            ho, hg = o["out"].hidden.numpy(), hidden[e][t]
            k = min(len(hg), len(ho))
            err = float(np.abs(hg[:k] - ho[:k]).max())
            worst = max(worst, err)
            assert err <= HIDDEN_TOL, (e, t, err)
    _note("multi_env_true_width", f"ragged scheduler at true width (TRUE1, fp32), {sum(n_turns)} turns of {N} envs vs solo oracle envs: ids identical, "
                                  f"worst hidden err {worst:.2e}, {st}")
    m.close()


# (the fp8 opt-ins at true width and at full depth are checked against the quantisation-emulating oracle in tests/test_fp8_gpu.py)
