"""The packed-decode switch end to end (set_packed_decode / svln_set_packed_decode) on the tiny fixtures, bf16 engine: the decode step's
gate/up and down_proj GEMVs and the lm_head GEMV read the lossless 12-bit packing of their weights, so ids, hidden tap rows and cache
lengths are BIT-identical with the switch on and off -- with and without decode graphs, after a set_tensor, and under every mode the
switch composes with."""
import numpy as np
import pytest
import torch

import p12_ref as R
from scenarios import SCENARIOS, SEED, apply_knobs, run_scenario
from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM

pytestmark = pytest.mark.gpu


def _model(sc, dtype=torch.bfloat16):
    m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=1, max_frames=1 + (sc["num_history"] or 0), max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    apply_knobs(m, sc)
    return m


def _episode(m, sc, steps=None):
    m.reset(1)
    taps = []

    def on_turn(t, rec):
        taps.append((m.last_hidden(), m.env_state(0)))
    log = run_scenario(m, sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda", steps=steps)
    ids = [r["out"].sequences[0].tolist() for r in log]
    lps = [r["out"].token_logprobs.cpu().numpy().view(np.uint32).tolist() for r in log if "token_logprobs" in r["out"]]
    return ids, taps, lps


def _same(a, b):
    assert a[0] == b[0] and len(a[1]) == len(b[1]) and a[2] == b[2], (a[0], b[0])
    for (ha, sa), (hb, sb) in zip(a[1], b[1]):
        assert sa == sb and np.array_equal(ha.view(np.uint32), hb.view(np.uint32))


@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graphs"])
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_on_is_bit_identical_to_off(name, graph):
    sc = SCENARIOS[name]
    m = _model(sc)
    m.set_decode_graph(graph)
    m.set_packed_decode(False)
    never = _episode(m, sc)                         # no run has used the packed weights yet
    assert len(never[0]) >= 4 and any(len(t) >= 3 for t in never[0])       # decode steps did run
    m.set_packed_decode(True)
    on = _episode(m, sc)
    _same(on, never)
    st, cfg = m.packed_stats(), sc["cfg"]
    shapes = [(2 * cfg.inter, cfg.hidden), (cfg.hidden, cfg.inter)] * cfg.layers + [(cfg.vocab, cfg.hidden)]      # gate/up, down_proj per layer; lm_head
    assert st["bf16_bytes"] == sum(2 * n * k for n, k in shapes) and st["blocks"] == sum(n * -(-k // 512) for n, k in shapes)
    assert st["packed_bytes"] == sum(n * (R.row_bytes(k) + 16) for n, k in shapes) and st["fallback_blocks"] <= st["blocks"] // 50
    m.set_packed_decode(False)
    _same(_episode(m, sc), never)                   # off after on
    m.set_packed_decode(True)
    m.set_packed_decode(True)                       # a call that changes nothing
    _same(_episode(m, sc), never)
    m.close()


def test_set_tensor_is_picked_up_and_stats_agree_with_the_restatement():
    sc = SCENARIOS["tiny_episode"]
    cfg = sc["cfg"]
    name = "model.layers.1.mlp.down_proj.weight"
    new = R.bf16_of(R.designed_bits(cfg.hidden, cfg.inter, "last", 77))           # every row's last block falls back
    lm = R.bf16_of(R.gaussian_bits(cfg.vocab, cfg.hidden, 78, sigma=0.03))
    m = _model(sc)
    before = _episode(m, sc, steps=12)
    m.set_tensor(name, new)                         # after creation, after the first encoding, after graphs may have been captured
    m.set_tensor("lm_head.weight", lm)
    on = _episode(m, sc, steps=12)
    assert on[0] != before[0]
    fresh = _model(sc)
    fresh.set_packed_decode(False)
    fresh.set_tensor(name, new)
    fresh.set_tensor("lm_head.weight", lm)
    _same(on, _episode(fresh, sc, steps=12))
    fresh.close()
    # the counts of the restatement over the packed matrices: gate / up rows, down_proj, lm_head
    packed = bf16 = blocks = fb = 0
    mats = [f"model.layers.{i}.mlp.{p}_proj.weight" for i in range(cfg.layers) for p in ("gate", "up", "down")] + ["lm_head.weight"]
    for t in mats:
        bits = R.bits_of(torch.from_numpy(m.get_tensor(t)).to(torch.bfloat16))
        p, r, f = R.encode(bits)
        packed += p.size + r.size
        bf16 += bits.size * 2
        blocks += bits.shape[0] * -(-bits.shape[1] // 512)
        fb += f
    st = m.packed_stats()
    assert st == dict(packed_bytes=packed, bf16_bytes=bf16, blocks=blocks, fallback_blocks=fb), (st, packed, bf16, blocks, fb)
    assert fb >= cfg.hidden
    m.close()


def test_composes_with_the_other_modes():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc)
    m.set_decode_graph(True)
    m.set_auto_draft(True)
    allowed = sorted({t for ids in _episode(m, sc)[0] for t in ids})
    modes = {"speculative": (lambda on: m.set_speculative(2 if on else 0)), "prefill_draft": m.set_prefill_draft,
             "token_scores": m.set_token_scores, "allowed_tokens": (lambda on: m.set_allowed_tokens(allowed if on else None, add_eos=False))}
    for what, switch in modes.items():
        switch(True)
        m.set_packed_decode(False)
        off = _episode(m, sc)
        m.set_packed_decode(True)
        on = _episode(m, sc)
        _same(on, off)
        assert (what == "token_scores") == bool(on[2]), what
        switch(False)
    m.close()


def test_fp32_engine_refuses_the_switch():
    sc = SCENARIOS["tiny_episode"]
    m = _model(sc, torch.float32)
    with pytest.raises(_lib.SvlnError, match="bf16"):
        m.set_packed_decode(True)
    m.set_packed_decode(False)
    assert m.packed_stats() == dict(packed_bytes=0, bf16_bytes=0, blocks=0, fallback_blocks=0)
    ids, _, _ = _episode(m, sc, steps=8)
    assert ids
    m.close()
