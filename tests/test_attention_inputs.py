"""CPU proof that the attention tests' inputs are sharp: on every case of tests/test_attention_gpu.py, each plausible kernel mistake
(float64 "mutant" references of tests/attn_ref.py) moves the expected output by at least 10x the tolerance the GPU test applies.
(The current random +-1 inputs of test_attention_llm give logits of standard deviation ~0.33: a dropped newest key stays inside the
bf16 bound there.)"""
import numpy as np
import pytest
import torch

import attn_ref as R
from streamvln_amd.config import CONFIGS

DTYPES = [torch.float32, torch.bfloat16]


def _check(ratios, what):
    weak = {k: round(v, 1) for k, v in ratios.items() if not v >= 10.0}
    assert not weak, f"{what}: mutants within 10x the tolerance: {weak} (all: { {k: round(v, 1) for k, v in ratios.items()} })"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,positions,max_positions", R.decode_cases())
def test_attention_inputs_are_discriminating_decode(dtype, cfg, positions, max_positions):
    """one case = one launch over the B envs: each mutant must move the output of some env of the launch"""
    c = CONFIGS[cfg]
    ratios = {}
    for b, p in enumerate(positions):
        case = R.decode_case(c, dtype, p, b, max_positions)
        for k, v in R.mutant_ratios(case, R.decode_mutants(p), q_flips=True).items():
            ratios[k] = max(ratios.get(k, 0.0), v)
    _check(ratios, f"decode {cfg} positions {positions}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,T,P", R.PREFILL_CASES)
def test_attention_inputs_are_discriminating_prefill(dtype, cfg, T, P):
    c = CONFIGS[cfg]
    ns, tps = R.prefill_split(c, T, P + T)
    # a subset of the query rows (a mutant that moves these rows moves the full output as much): the first and last rows, rows at
    # key-tile and split edges
    rows = {P, P + 1, P + 2, P + T - 3, P + T - 2, P + T - 1}
    for t in range(P, P + T):
        if t % R.PAGE in (0, 63) or t % (tps * R.PAGE) in (0, tps * R.PAGE - 1):
            rows.add(t)
    rows = sorted(rows)[:48] + sorted(rows)[-8:]
    case = R.prefill_case(c, dtype, T, P, rows=sorted(set(rows)))
    _check(R.mutant_ratios(case, R.prefill_mutants(c, T, P), q_flips=False), f"prefill {cfg} T{T} P{P}")


def test_reference_is_rope_consistent():
    """the generator's roped-space design survives un-rope -> dtype rounding -> RoPE: a needle row puts ~all its weight on its key"""
    c = CONFIGS["tiny"]
    case = R.decode_case(c, torch.float32, 700, 0)
    s = torch.einsum("hd,shd->hs", case.q[0], case.k.repeat_interleave(case.G, 1)) * case.scale
    p = torch.softmax(s, -1)
    assert float(p[0, 700]) > 0.999           # head 0: "newest"
    assert float(p[1, 0]) > 0.999             # head 1: "sink"
    assert float(p[2, 640]) > 0.999           # head 2: "tile_first" (700 // 64 * 64)
    assert int(p[3].argmax()) == 700          # head 3: "rising": the max is the newest key


# ViT: the first and last rows, the rows around the key-tile edge 64 and the partial tile (every pattern of every head and frame occurs)
VIT_ROWS = list(range(0, 40)) + list(range(60, 70)) + list(range(R.VS - 29, R.VS))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,F", R.VIT_CASES)
def test_attention_inputs_are_discriminating_vit(dtype, cfg, F):
    case = R.vit_case(CONFIGS[cfg], dtype, F, rows=VIT_ROWS)
    _check(R.vit_mutant_ratios(case), f"vit {cfg} F{F}")


def test_vit_reference_is_sharp():
    """needle rows put ~all their weight on their key, "two" splits it between keys 0 and 728, the ramps peak at their ends"""
    c = CONFIGS["true_dims_1layer"]
    case = R.vit_case(c, torch.bfloat16, 2, rows=list(range(10)))
    s = torch.einsum("rhd,shd->rhs", case.q[1, :10], case.k[1]) * case.scale
    p = torch.softmax(s, -1)[:, 0]                    # frame 1, head 0: row r takes VIT_PATTERNS[(r + 3) % 10]
    last = R.VS - 1
    for r, key in ((1, 64), (2, 703), (4, 0), (5, last), (7, 0), (8, 8), (9, 63)):       # key64 key703 group_first key728 key0 self key63
        assert float(p[r, key]) > 0.999, (r, key, float(p[r, key]))
    # rising, falling (steps of 60 / 728 logits: bf16 rounding may reorder neighbouring keys)
    assert int(p[0].argmax()) >= last - 3 and int(p[6].argmax()) <= 3
    assert float(p[3, 0] + p[3, last]) > 0.999 and min(float(p[3, 0]), float(p[3, last])) > 0.2     # two
