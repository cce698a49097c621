"""CPU checks of the P12 restatement (tests/p12_ref.py) and of the inputs tests/test_p12_gpu.py runs: the format round-trips every bf16
pattern, the table rule and the mask hold on designed rows, the stored-byte ratio on the project's synthetic weights is the recorded
one, the in-flight depth does not reorder a lane's elements, and every GEMV case is sharp against every decoder mistake it can show."""
import numpy as np
import pytest

import p12_ref as R
from streamvln_amd import weights as W

# stored bytes / bf16 bytes of 3584-wide rows of the synthetic distribution (uniform, a = sqrt(3 / 3584)): packed blocks + 16-byte records
# + the bf16 bytes of the fallback blocks (streamed instead of the packed ones).  Measured with this restatement: 0.7525 at 0.2 % fallback
# blocks (0.75 + 16 / 7168 for the records = 0.7522 without them); the issue's reference encoder gave 0.7506.
RATIO_ISSUE, RATIO_TOL = 0.7506, 0.005


def test_every_bf16_pattern_round_trips():
    allp = np.arange(65536, dtype=np.uint16).reshape(128, 512)
    packed, rec, n_fb = R.encode(allp)
    assert packed.shape == (128, 768) and rec.shape == (128, 16)
    assert np.array_equal(R.decode(packed, rec, allp), allp)
    # row r holds the 512 patterns of the high bytes 2r and 2r + 1, 256 each: two table entries (the lower first), the second repeated
    assert n_fb == 0 and all(list(rec[r, :8]) == [2 * r & 0x7F] + [(2 * r + 1) & 0x7F] * 7 for r in range(128))
    # without the original (zeros in its place) the packed bytes alone give it back: nothing was read from the fallback source
    assert np.array_equal(R.decode(packed, rec, np.zeros_like(allp)), allp)


@pytest.mark.parametrize("name", list(R.designed_rows()))
def test_table_rule_and_mask_on_designed_rows(name):
    bits, table, mask = R.designed_rows()[name]
    packed, rec, n_fb = R.encode(bits)
    assert list(rec[0, :8]) == table, (name, list(rec[0, :8]))
    assert R.masks_of(rec)[0] == mask and n_fb == bin(mask).count("1")
    blocks = packed.reshape(-1, R.BLOCK_BYTES)
    for k in range(len(blocks)):
        assert (not blocks[k].any()) == bool(mask >> k & 1) or not bits[0, k * 512:(k + 1) * 512].any(), (name, k)
    assert np.array_equal(R.decode(packed, rec, bits), bits)


def test_ragged_block_is_zero_padded_and_row_stride():
    bits = R.designed_bits(3, 520, "none", 5)
    packed, rec, n_fb = R.encode(bits)
    assert packed.shape[1] == 2 * 768 == R.row_bytes(520) and n_fb == 0
    last = packed[:, 768:]
    assert not last[:, 8:512].any() and not last[:, 512 + 4:].any() and last[:, :8].any()
    assert R.row_bytes(512) == 768 and R.row_bytes(8) == 768 and R.row_bytes(32768) == 64 * 768


def test_stored_byte_ratio_on_the_synthetic_distribution():
    rows, K = 96, 3584
    v = W.synth_flat(W.tensor_seed(0, "model.layers.0.mlp.gate_proj.weight"), 0, rows * K, (3.0 / K) ** 0.5, 0.0)
    bits = W.to_bf16_bits(v).reshape(rows, K)
    packed, rec, n_fb = R.encode(bits)
    stored = packed.size + rec.size + n_fb * 1024
    ratio = stored / (rows * K * 2)
    print(f"stored-byte ratio {ratio:.4f}, fallback blocks {n_fb} of {rows * 7}")
    assert abs(ratio - RATIO_ISSUE) <= RATIO_TOL, ratio
    assert abs(ratio - 0.7525) <= 0.001 and n_fb <= 0.01 * rows * 7, (ratio, n_fb)      # the figure recorded above
    assert np.array_equal(R.decode(packed, rec, bits), bits)


@pytest.mark.parametrize("nch,kw", [(8, 4), (63, 4), (64, 4), (65, 4), (131, 4), (576, 4), (448, 1), (131, 1), (2368, 4)])
def test_depth_does_not_reorder_a_lane(nch, kw):
    two, one = R.lane_chunks(nch, kw, 2), R.lane_chunks(nch, kw, 1)
    seen = []
    for key in two:
        a, b = [c for c, _ in two[key]], [c for c, _ in one[key]]
        assert a == b == sorted(a) and all(c % 64 == key[1] and (c // 64) % kw == key[0] for c in a), key
        seen += a
    assert sorted(seen) == list(range(nch))                                  # every chunk once
    for depth, seqs in ((2, two), (1, one)):                                # the lanes of one load step share the block: ci >> 6 is wave-uniform
        for kwi in range(kw):
            steps = {}
            for lane in range(64):
                for pos, (c, step) in enumerate(seqs[(kwi, lane)]):
                    steps.setdefault((step, pos), set()).add(c >> 6)
            assert all(len(v) == 1 for v in steps.values()), (depth, kwi)


def test_case_list_reaches_what_it_names():
    ks = {c.K for c in R.CASES}
    assert {64, 504, 512, 520, 1048, 4608} <= ks
    assert {1, 2, 3, 7, 8, 9} <= {c.N for c in R.CASES if c.kernel == "ksplit"}
    assert any(c.epi == "swiglu" and c.N == 128 for c in R.CASES) and any(c.kernel == "rows" and c.epi == "none" and c.N > 8192 and c.K == 512 for c in R.CASES)
    assert any(c.norm for c in R.CASES) and any(c.bias and c.res for c in R.CASES) and any(c.pad for c in R.CASES) and any(c.special for c in R.CASES)
    for c in R.CASES:
        c.build()
        nblk = -(-c.K // 512)
        masks = R.masks_of(c.rec)
        if c.special or c.ties:
            continue
        want = {"none": 0, "first": 1, "last": 1 << (nblk - 1), "all": (1 << nblk) - 1}[c.fb]
        assert all(m == want for m in masks), (c.id, masks[:4], want)
    # fallback: none, first, last, ragged last, all
    assert any(c.fb == "last" and c.K % 512 for c in R.CASES) and any(c.fb == "last" and c.K % 512 == 0 for c in R.CASES)
    tie = next(c for c in R.CASES if c.ties)
    logits = tie.outputs().view(np.float32)
    assert logits[tie.ties[0]] == logits[tie.ties[1]] == logits.max() and (logits == logits.max()).sum() == 2


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_gemv_case_is_sharp(case):
    """each decoder mistake the case can show changes at least one stored output bit (emulated in the kernels' summation order)"""
    case.build()
    ref = case.outputs()
    for m in case.mutants():
        assert (case.outputs(m) != ref).any(), (case.id, m)


def test_every_mutant_is_shown_by_some_case():
    shown = set()
    for c in R.CASES:
        shown |= set(c.mutants())
    assert shown == set(R.MUTANTS)
