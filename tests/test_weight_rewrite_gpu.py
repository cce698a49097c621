"""Weight writes under every mode that keeps state derived from the weights (TINY, bf16, decode graphs on).

Engine E1 loads seed 1234, enables the mode and runs the probe (tests/switch_probe.py) -- so the quantised copies are built, the decode
graphs captured, the feature cache filled -- then has weights rewritten and runs the probe again.  Engine E2 is fresh: the rewritten
weights first, then the mode.  The two runs must be BIT-equal: ids, hidden rows, scores, env_state.  A copy, graph or cache entry that
still belongs to the old weights shows as a difference, because the new values are chosen so that more than half of the rows of every
rewritten LLM matrix quantise to other e4m3 / MXFP4 bytes (asserted on the CPU before any GPU call).

Also: a weight write while scheduler turns are in flight, or while a group turn is pending, is refused by name and changes nothing."""
import numpy as np
import pytest
import torch

import mxfp4_ref as MX
import p12_ref as R
import switch_probe as P
from oracle import streamvln_oracle as O
from scenarios import SEED
from streamvln_amd import weights as W
from util import synth_weights

pytestmark = pytest.mark.gpu

CFG = P.SC["cfg"]
SEED2 = 4321
VT = "model.vision_tower.vision_tower.vision_model."
LLM_TENSORS = ["lm_head.weight",
               "model.layers.1.mlp.gate_proj.weight",           # the interleaved RowMap{32, 2, 0} slot: the up rows must stay
               "model.layers.0.self_attn.k_proj.weight"]        # inside the fused q | k | v
VISION_TENSORS = [VT + "encoder.layers.1.mlp.fc1.weight", VT + "embeddings.patch_embedding.weight"]
TENSORS = LLM_TENSORS + VISION_TENSORS

MODES = {
    "packed": lambda m: None,                                   # the default: the 12-bit packed copies
    "fp8_decode": lambda m: m.set_fp8_decode(True),
    "mxfp4_decode": lambda m: m.set_mxfp4_decode(True),
    "mxfp4_batched": lambda m: m.set_mxfp4_batched(True),
    "fp8_gemm": lambda m: m.set_fp8_gemm(True),
    "fp8_gemm_scaled": lambda m: (m.set_fp8_gemm(True), m.set_fp8_scaled_mfma(True)),
    "feature_cache": lambda m: m.set_feature_cache(16),         # (never emptied by the probe here: E1's second run meets what its first run cached)
    "speculative": lambda m: m.set_speculative(2),              # with the auto-draft of the probe's base state
}


def _spec(name):
    return {s.name: s for s in W.tensor_specs(CFG)}[name]


def new_values(name):
    """Gaussian bf16 values of the tensor's shape at the scale of its synthetic ones (fp32 numpy, exactly representable in bf16)"""
    spec = _spec(name)
    rows, cols = spec.shape[0], int(np.prod(spec.shape[1:]))
    sigma = spec.half_width / 3.0 ** 0.5                        # the uniform distribution's standard deviation
    bits = R.gaussian_bits(rows, cols, 1000 + TENSORS.index(name), sigma=sigma)
    return R.f32_of(bits).reshape(spec.shape)


def _rows_that_requantise(old, new):
    """fraction of the rows whose e4m3 copy (bytes or row scale: the dequantised row) / MXFP4 copy (codes or block scales) differs"""
    old, new = torch.from_numpy(old.reshape(old.shape[0], -1).copy()), torch.from_numpy(new.reshape(new.shape[0], -1).copy())
    co, eo = MX.quant_mxfp4(old)
    cn, en = MX.quant_mxfp4(new)
    mx = ((MX.fold_zero(co) != MX.fold_zero(cn)).any(1) | (eo != en).any(1)).float().mean().item()
    f8 = (O.Fp8Emu().weight({"w": old}, "w") != O.Fp8Emu().weight({"w": new}, "w")).any(1).float().mean().item()
    return f8, mx


@pytest.fixture(scope="module")
def rewrites():
    """what each rewrite writes, checked on the CPU: {tensor: fp32 array}; 'synthetic' = the whole model of seed 4321"""
    old = synth_weights(CFG, SEED)
    out = {name: new_values(name) for name in TENSORS}
    whole = synth_weights(CFG, SEED2)
    for name in LLM_TENSORS:
        for what, new in (("single", out[name]), ("synthetic", whole[name])):
            f8, mx = _rows_that_requantise(old[name], new)
            print(f"{name} [{what}]: {f8:.3f} of the rows change their e4m3 copy, {mx:.3f} their MXFP4 copy")
            assert f8 > 0.5 and mx > 0.5, (name, what, f8, mx)
    for name in VISION_TENSORS:
        changed = (old[name].reshape(old[name].shape[0], -1) != out[name].reshape(out[name].shape[0], -1)).any(1).mean()
        assert changed > 0.5, (name, changed)
    return out


def _same(a, b):
    """bit equality of everything two runs returned; the counters stay out (E1's feature cache is warm where E2's is cold)"""
    strip = lambda run: {k: v for k, v in run.items() if k != "stats"}
    return P.same(strip(a), strip(b))


def _engine(seed):
    m = P.make_model(torch.bfloat16, seed)
    m.probe_on = []
    P.base_state(m)
    return m


_FRESH = {}


def _fresh_run(mode, what, write):
    """E2: a fresh engine, the rewritten weights first, then the mode; one run per (mode, rewrite), shared by the upload variants"""
    key = (mode, what)
    if key not in _FRESH:
        m = _engine(SEED)
        write(m)
        MODES[mode](m)
        _FRESH[key] = P.probe(m)
        m.close()
    return _FRESH[key]


def _rewritten_run(mode, write):
    """E1: seed 1234, the mode, a run (copies built, graphs captured, cache filled), the rewrite, a run"""
    m = _engine(SEED)
    MODES[mode](m)
    before = P.probe(m)
    write(m)
    after = P.probe(m)
    m.close()
    return before, after


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_model_reload(mode, rewrites):
    write = lambda m: m.load_synthetic(SEED2)
    before, after = _rewritten_run(mode, write)
    assert P.results_of(after) != P.results_of(before)
    _same(after, _fresh_run(mode, "synthetic", write))


@pytest.mark.parametrize("name", TENSORS, ids=[t.replace(VT, "vit.").replace("model.", "") for t in TENSORS])
@pytest.mark.parametrize("mode", list(MODES))
def test_single_tensor(mode, name, rewrites):
    value = rewrites[name]
    host = lambda m: m.set_tensor(name, value)                                                   # a host fp32 array
    device = lambda m: m.set_tensor(name, torch.from_numpy(value).to("cuda", torch.bfloat16))    # a device bf16 tensor
    fresh = _fresh_run(mode, name, host)
    for what, write in (("host fp32", host), ("device bf16", device)):
        before, after = _rewritten_run(mode, write)
        assert P.results_of(after) != P.results_of(before), (mode, name, what)
        try:
            _same(after, fresh)
        except AssertionError as err:
            raise AssertionError(f"{mode}, {name} from a {what} source: {err}") from None


def test_single_tensor_write_keeps_its_neighbours():
    """gate_proj shares an interleaved matrix with up_proj, k_proj a fused one with q and v: a write of one leaves the others' values"""
    m = _engine(SEED)
    old = synth_weights(CFG, SEED)
    for name, others in ((LLM_TENSORS[1], ["model.layers.1.mlp.up_proj.weight"]),
                         (LLM_TENSORS[2], ["model.layers.0.self_attn.q_proj.weight", "model.layers.0.self_attn.v_proj.weight"])):
        new = new_values(name)
        m.set_tensor(name, new)
        assert np.array_equal(m.get_tensor(name), new)
        for o in others:
            assert np.array_equal(m.get_tensor(o), old[o]), o
    m.close()


def _first_request(m, env=0, **kw):
    ag = P._agent(m, env, bool(kw.get("do_sample")))
    ag.observe(P.synthetic_frame(env, 0))
    req = ag._build_request("")
    req.update(kw)
    return req


def test_write_refused_while_scheduler_turns_are_in_flight(rewrites):
    name = LLM_TENSORS[0]
    m = _engine(SEED)
    m.set_fp8_decode(True)                                      # so that a write would have copies to rebuild
    control = P.probe(m)
    m.reset(P.N_ENVS)
    weights, stats = m.get_tensor(name), m.packed_stats()
    m.submit(**_first_request(m))
    with pytest.raises(RuntimeError, match="svln_set_tensor cannot change while scheduler turns are in flight"):
        m.set_tensor(name, rewrites[name])
    with pytest.raises(RuntimeError, match="svln_synth_tensor cannot change while scheduler turns are in flight"):
        m.load_synthetic(SEED2)
    done = []
    while not done:
        done, _ = m.step_batch()                                # the turn in flight finishes
    assert np.array_equal(m.get_tensor(name), weights) and m.packed_stats() == stats
    P.same(P.probe(m), control)                                 # ... and nothing else moved
    m.close()


def test_write_refused_while_a_group_is_pending(rewrites):
    name = LLM_TENSORS[0]
    m = _engine(SEED)
    m.set_fp8_decode(True)
    control = P.probe(m)
    m.reset(P.N_ENVS)
    weights, stats = m.get_tensor(name), m.packed_stats()
    out = m.generate(**_first_request(m, do_sample=True, temperature=0.8, num_return_sequences=2))
    state = m.env_state(0)
    with pytest.raises(RuntimeError, match="svln_set_tensor cannot change while a group turn is pending"):
        m.set_tensor(name, rewrites[name])
    with pytest.raises(RuntimeError, match="svln_synth_tensor cannot change while a group turn is pending"):
        m.load_synthetic(SEED2)
    assert m.env_state(0) == state and np.array_equal(m.get_tensor(name), weights) and m.packed_stats() == stats
    kv = m.select_sequence(1, env_id=0)                         # the group is whole
    assert kv.get_seq_length() == state[0] + int(out.sequence_lengths[1]) - 1
    m.set_tensor(name, weights)                                 # accepted again once the group is resolved
    m.set_sampling(None)
    P.same(P.probe(m), control)
    m.close()
