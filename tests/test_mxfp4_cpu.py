"""The CPU restatement of the MXFP4 weight scheme (tests/mxfp4_ref.py) against hand-written cases, and the scheme's quantisation noise on
the op-test inputs under a cap.  The GPU quantiser is held to this restatement byte for byte (tests/test_mxfp4_gpu.py), so it inherits
every check made here."""
import math

import pytest
import torch

import mxfp4_ref as R
from util import q, rnd


def _block(vals, fill=0.0):
    """one row of one 32-element block beginning with `vals`"""
    row = torch.full((1, 32), float(fill))
    row[0, :len(vals)] = torch.tensor([float(v) for v in vals])
    return row


def _nibbles(codes):
    return torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(codes.shape[0], -1)


def test_grid_values_are_fixed_points_with_their_codes():
    # amax = 6 -> floor(log2 6) - 2 = 0: the scale is 1 and every grid value is its own code
    row = _block(list(R.GRID) + [-g for g in R.GRID])
    codes, e8 = R.quant_mxfp4(row)
    assert e8.tolist() == [[127]]
    nib = _nibbles(codes)[0].tolist()
    assert nib[:8] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert nib[9:16] == [9, 10, 11, 12, 13, 14, 15] and nib[8] in (0, 8)         # -0 == +0
    assert torch.equal(R.dequant_mxfp4(codes, e8), row)


def test_every_tie_rounds_to_the_even_code_and_values_above_six_saturate():
    ties = [(5.0, 4.0), (3.5, 4.0), (2.5, 2.0), (1.75, 2.0), (1.25, 1.0), (0.75, 1.0), (0.25, 0.0), (7.0, 6.0)]
    # the block holds a 6 (scale 1) for the proper ties, and 7 alone defines amax in its own block (floor(log2 7) - 2 = 0 as well)
    for sign in (1.0, -1.0):
        row = _block([6.0] + [sign * a for a, _ in ties[:-1]])
        out = R.dequant_mxfp4(*R.quant_mxfp4(row))[0]
        assert out[1:8].tolist() == [sign * b for _, b in ties[:-1]]              # (-0.0 == 0.0)
        row7 = _block([sign * 7.0])
        codes, e8 = R.quant_mxfp4(row7)
        assert e8.tolist() == [[127]] and R.dequant_mxfp4(codes, e8)[0, 0] == sign * 6.0
    # just beside the ties: nearest wins
    row = _block([6.0, 5.0 + 2 ** -10, 5.0 - 2 ** -10, 0.25 + 2 ** -12, 0.25 - 2 ** -12, 2.5 + 2 ** -10, 3.5 - 2 ** -10])
    assert R.dequant_mxfp4(*R.quant_mxfp4(row))[0, :7].tolist() == [6.0, 6.0, 4.0, 0.5, 0.0, 3.0, 3.0]
    # the same ties under other block scales: the element is w / 2^e, exactly
    for k in (-20, -7, 3, 11):
        row = _block([6.0] + [a for a, _ in ties[:-1]]) * 2.0 ** k
        codes, e8 = R.quant_mxfp4(row)
        assert e8.tolist() == [[127 + k]]
        assert R.dequant_mxfp4(codes, e8)[0, :8].tolist() == [6.0 * 2.0 ** k] + [b * 2.0 ** k for _, b in ties[:-1]]


def test_all_zero_block_and_power_of_two_amax():
    codes, e8 = R.quant_mxfp4(torch.zeros(2, 64))
    assert e8.tolist() == [[127, 127], [127, 127]] and int(codes.max()) == 0          # e = 0, bytes 0
    # amax = 2^k exactly: e = k - 2, the largest element is code 6 (value 4), nothing saturates
    for k in (-9, 0, 1, 5):
        row = _block([2.0 ** k, -(2.0 ** k), 2.0 ** (k - 1), 2.0 ** (k - 3), 2.0 ** (k - 4)])
        codes, e8 = R.quant_mxfp4(row)
        assert e8.tolist() == [[127 + k - 2]]
        assert _nibbles(codes)[0, :5].tolist() == [6, 14, 4, 1, 0]                     # 4, -4, 2, 0.5, 0.25 -> 0 (tie to even)
    # just below a power of two the exponent is one less and the element saturates at 6 (7.97 / 1 -> 6)
    row = _block([q(torch.tensor(7.97), torch.bfloat16).item()])
    codes, e8 = R.quant_mxfp4(row)
    assert e8.tolist() == [[127]] and _nibbles(codes)[0, 0] == 7


def test_nibble_order_and_layout():
    W = torch.zeros(2, 64)
    W[0, 0], W[0, 1], W[0, 2], W[0, 3] = 1.0, -6.0, 0.5, 3.0          # block 0 of row 0: scale 1
    W[1, 32], W[1, 35] = 8.0, -2.0                                    # block 1 of row 1: amax 8 -> e = 1
    codes, e8 = R.quant_mxfp4(W)
    assert codes.shape == (2, 32) and e8.shape == (2, 2) and codes.dtype == e8.dtype == torch.uint8
    assert codes[0, 0] == (2 | (15 << 4)) and codes[0, 1] == (1 | (5 << 4))           # element 2j low nibble, 2j + 1 high nibble
    assert e8.tolist() == [[127, 127], [127, 128]]
    assert codes[1, 16] == 6 and codes[1, 17] == (10 << 4)                            # 8 / 2 = 4 -> code 6; -2 / 2 = -1 -> code 2 | 8, element 3
    exp = torch.zeros(2, 64)
    exp[0, :4] = torch.tensor([1.0, -6.0, 0.5, 3.0])
    exp[1, 32], exp[1, 35] = 8.0, -2.0
    assert torch.equal(R.dequant_mxfp4(codes, e8), exp)


@pytest.mark.parametrize("rows,cols,sd,seed", [(37, 512, 0.02, 3), (5, 18944, 0.5, 4), (3, 32, 1.0, 5)])
def test_exponent_formula_idempotence_and_error_bound(rows, cols, sd, seed):
    W = q(rnd((rows, cols), seed, sd), torch.bfloat16)
    W[0] = 0.0
    codes, e8 = R.quant_mxfp4(W)
    amax = W.reshape(rows, -1, 32).abs().amax(-1)
    for r in range(rows):
        for b in range(cols // 32):
            a = float(amax[r, b])
            assert int(e8[r, b]) == (127 if a == 0 else math.floor(math.log2(a)) + 125), (r, b, a)
    D = R.dequant_mxfp4(codes, e8)
    c2, e2 = R.quant_mxfp4(D)
    assert torch.equal(R.fold_zero(c2), R.fold_zero(codes)) and torch.equal(e2, e8)    # quant(dequant(quant(W))) == quant(W)
    # an element is at most half a grid step from its value (the widest step is 2, between 4 and 6), or saturated from below 8 to 6
    scale = torch.ldexp(torch.ones_like(amax), e8.to(torch.int32) - 127)
    err = (D - W).reshape(rows, -1, 32).abs() / scale[..., None]
    assert float(err.max()) <= 2.0


# the code of every member of mxfp4_ref.TIE_VALS, written out by hand (value in units of the block scale -> magnitude code)
HAND_CODE = {0.0: 0, 0.125: 0, 0.25: 0, 0.375: 1, 0.5: 1, 0.625: 1, 0.75: 2, 0.875: 2, 1.0: 2, 1.25: 2, 1.5: 3, 1.75: 4, 2.0: 4, 2.25: 4,
             2.5: 4, 2.75: 5, 3.0: 5, 3.5: 6, 4.0: 6, 4.5: 6, 5.0: 6, 5.5: 7, 6.0: 7, 7.0: 7, 7.5: 7}


def _hand_nibbles(block, k):
    """the 32 nibbles of a block whose scale is 2^k, from HAND_CODE"""
    out = []
    for w in block.double().tolist():
        v = w / 2.0 ** k
        out.append(HAND_CODE[abs(v)] | (8 if v < 0 and HAND_CODE[abs(v)] else 0))
    return out


def _fold_nibbles(codes):
    return _nibbles(R.fold_zero(codes))


def test_ties_where_the_block_exponent_clamps():
    W, e8_exp = R.clamp_tie_matrix()
    assert set(R.TIE_VALS) == set(HAND_CODE) and all(HAND_CODE[t] % 2 == 0 for t in R.TIES)      # every tie goes to an even code
    codes, e8 = R.quant_mxfp4(W)
    assert e8.tolist() == e8_exp
    nib = _fold_nibbles(codes)
    amax = W.reshape(len(W), 2, 32).abs().amax(-1)
    assert float(amax[0, 0]) == 3 * 2.0 ** -127 and 2.0 ** -126 <= float(amax[0, 0]) < 2.0 ** -125       # floor(log2) - 2 = -128: clamped
    assert 0 < float(amax[1, 0]) < 2.0 ** -126                                                          # a bf16 subnormal
    assert float(amax[1, 1]) == 1.75 * 2.0 ** 127
    for r in range(len(W)):
        for b in range(2):
            blk = W[r, 32 * b:32 * b + 32]
            got = [n if n != 8 else 0 for n in nib[r, 32 * b:32 * b + 32].tolist()]
            assert got == _hand_nibbles(blk, int(e8[r, b]) - 127), (r, b)
            assert sum(1 for w in blk.tolist() if abs(w) / 2.0 ** (int(e8[r, b]) - 127) in R.TIES) >= 3, (r, b)      # ties are present
    assert torch.equal(R.dequant_mxfp4(codes, e8)[:, 31], W[:, 31])                                      # each block-0 amax (3, 1.5, 6) is a grid value


def test_ties_at_the_edge_of_the_second_loop_iteration():
    W = R.wide_tie_matrix()
    assert W.shape == (2, 8256) and {255, 256, 257} <= {b for b, _ in R.WIDE_BLOCKS}
    codes, e8 = R.quant_mxfp4(W)
    exp_e8 = torch.full((2, 258), 127, dtype=torch.uint8)
    for b, k in R.WIDE_BLOCKS:
        exp_e8[:, b] = 127 + k
    assert torch.equal(e8, exp_e8)
    assert all(exp_e8[0, b] != exp_e8[0, b + 1] for b in (254, 255, 256))                                # neighbours differ in exponent
    nib = _fold_nibbles(codes)
    for r in range(2):
        for b, k in R.WIDE_BLOCKS:
            assert nib[r, 32 * b:32 * b + 32].tolist() == _hand_nibbles(W[r, 32 * b:32 * b + 32], k), (r, b)
    live = torch.zeros(258, dtype=torch.bool)
    live[[b for b, _ in R.WIDE_BLOCKS]] = True
    assert int(codes.reshape(2, 258, 16)[:, ~live].max()) == 0


def test_a_block_with_a_nan_or_an_infinity_gets_the_scale_byte_0xff():
    for what, W, twin, bad in R.nonfinite_matrices():
        codes, e8 = R.quant_mxfp4(W)
        ct, et = R.quant_mxfp4(twin)
        is_bad = torch.zeros_like(e8, dtype=torch.bool)
        for r, b in bad:
            is_bad[r, b] = True
        assert torch.equal(e8 == R.E8_NAN, is_bad), what                                                 # exactly the blocks that hold one
        assert not bool((et == R.E8_NAN).any()) and torch.equal(e8[~is_bad], et[~is_bad]), what
        keep = (~is_bad).repeat_interleave(16, dim=1)
        assert torch.equal(codes[keep], ct[keep]), what                                                  # the other blocks are unchanged
        assert torch.equal(R.mask_nonfinite(codes, e8)[keep], codes[keep]) and int(R.mask_nonfinite(codes, e8)[~keep].max()) == 0
        ex = et.int() - 127
        assert bool((ex[:, 1:] != ex[:, :-1]).float().mean() > 0.8), what                                # neighbouring exponents differ


def _differs(ref, mut):
    """what the device comparison sees: the scale bytes, and the code bytes outside the reference's 0xFF blocks (-0 folded)"""
    return not torch.equal(ref[1], mut[1]) or not torch.equal(R.fold_zero(R.mask_nonfinite(ref[0], ref[1])), R.fold_zero(R.mask_nonfinite(mut[0], ref[1])))


def test_the_designed_inputs_see_the_two_mutants():
    """nan_code0 = the kernel before the 0xFF rule; iter2 = a thread's second loop iteration dropped.  Each is caught on every input
    written for it, by a scale byte or (outside 0xFF blocks) a code byte; the narrow finite inputs cannot see iter2 and say so."""
    nonfinite = R.nonfinite_matrices()
    wide = [R.wide_tie_matrix()] + [W for what, W, _, _ in nonfinite if what == "wide"]
    report = {}
    for i, (what, W, _, bad) in enumerate(nonfinite):
        ref, mut = R.quant_mxfp4(W), R.quant_mxfp4(W, "nan_code0")
        report[f"nan_code0/{what}"] = int((ref[1] != mut[1]).sum())
        assert report[f"nan_code0/{what}"] == len(bad) and _differs(ref, mut)
    for i, W in enumerate(wide):
        ref, mut = R.quant_mxfp4(W), R.quant_mxfp4(W, "iter2")
        report[f"iter2/wide{i}"] = int((ref[1] != mut[1]).sum())
        assert report[f"iter2/wide{i}"] >= 2 and _differs(ref, mut)
    Wc, _ = R.clamp_tie_matrix()
    assert not _differs(R.quant_mxfp4(Wc), R.quant_mxfp4(Wc, "iter2")) and not _differs(R.quant_mxfp4(Wc), R.quant_mxfp4(Wc, "nan_code0"))
    print(report)


# relative L2 distance between the product over the dequantised weights and the unquantised product on the inputs of the GEMV op tests
# (util.rnd((N, K), 41, 1 / sqrt(K)) weights, rnd((K,), 42) x, both rounded to bf16).  `expected` = the figures stated with the scheme
# (computed from its definition; re-measured with this restatement: 0.0971 / 0.1160 / 0.1220 / 0.1688 / 0.0972); the cap is 1.5 x expected.  A block exponent one
# too small gives 0.228 / 0.462 / 0.322 / 0.464 / 0.228, at least 2.3 x expected, so it cannot pass; an exponent one too large is NOT
# visible here (0.112 / 0.107 / 0.131 / 0.111 / 0.111) and is pinned by the hand-written e8 cases above instead.
NOISE = [
    (4608, 3584, 0.097),
    (3584, 18944, 0.116),
    (515, 512, 0.122),
    (7, 64, 0.169),
    (9000, 3584, 0.097),
]


def product_noise(N, K):
    Wt, x = q(rnd((N, K), 41, 1.0 / math.sqrt(K)), torch.bfloat16), q(rnd((K,), 42), torch.bfloat16)
    full = Wt.double() @ x.double()
    deq = R.qdq_mxfp4(Wt).double() @ x.double()
    return float((deq - full).norm() / full.norm())


@pytest.mark.parametrize("N,K,expected", NOISE)
def test_quantisation_noise_of_the_scheme_is_4bit_sized(N, K, expected):
    rel = product_noise(N, K)
    print(f"MXFP4 product noise {N} x {K}: rel L2 {rel:.4f} (stated {expected}, cap {1.5 * expected:.4f})")
    assert rel < 1.5 * expected, (N, K, rel)
