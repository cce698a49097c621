"""CPU restatement of the engine's MXFP4 weight scheme (test infrastructure; DESIGN.md section 6, include/streamvln_hip.h
svln_op_quant_mxfp4).  This is the OCP MX conversion, nothing project-specific:

  * every run of 32 consecutive elements of a row is one block; amax = max |w|; e = floor(log2(amax)) - 2 (2 = E2M1's largest
    exponent) clamped to [-127, 127], 0 for an all-zero block; the stored scale byte is e + 127 (E8M0), the scale 2^e exactly;
  * element code = E2M1 of w / 2^e (exact in fp32) on the grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, round to nearest, ties to the code with
    an even mantissa bit (5 -> 4, 3.5 -> 4, 2.5 -> 2, 1.75 -> 2, 1.25 -> 1, 0.75 -> 1, 0.25 -> 0), saturating at 6; sign in bit 3;
  * element 2j in the low nibble, 2j + 1 in the high nibble of byte j;
  * a block that holds a NaN or an infinity gets the scale byte 0xFF (E8M0 NaN) and unspecified codes; the other blocks of its row are
    what they are without it.  How the GEMVs consume a scale byte 0xFF (or 0) is out of scope here.

The designed quantiser inputs (tie_matrix, clamp_tie_matrix, wide_tie_matrix, nonfinite_matrices) live here so that the CPU proof
(tests/test_mxfp4_cpu.py) and the device comparison (tests/test_mxfp4_gpu.py) read the same bytes.
"""
import torch

from oracle import streamvln_oracle as O

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32


def block_exponent(amax: torch.Tensor) -> torch.Tensor:
    """e of a block from its amax (fp32, >= 0): floor(log2(amax)) - 2 clamped to [-127, 127]; 0 where amax == 0"""
    _, ex = torch.frexp(amax.to(torch.float32))               # amax = m * 2^ex, 0.5 <= m < 1  ->  floor(log2(amax)) = ex - 1
    e = (ex.to(torch.int32) - 1 - 2).clamp(-127, 127)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def e2m1_codes(v: torch.Tensor) -> torch.Tensor:
    """4-bit codes (uint8, sign in bit 3) of fp32 values: round to nearest even on GRID, saturating at 6.  The seven comparisons are the
    midpoints of neighbouring grid values; a tie goes to the neighbour whose code is even (mantissa bit 0)."""
    a = v.abs()
    mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
           + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    return mag | ((v < 0).to(torch.uint8) << 3)


E8_NAN = 0xFF
MUTANTS = ("nan_code0", "iter2")


def quant_mxfp4(W: torch.Tensor, mutant=None):
    """W [rows][cols] (cols % 32 == 0; fp32 or bf16) -> (codes uint8 [rows][cols / 2], e8 uint8 [rows][cols / 32]).  A block that holds
    a NaN or an infinity gets the scale byte 0xFF; its codes are unspecified (here: those of the block with the element set to 0), so
    comparisons mask them (mask_nonfinite).  How a GEMV reads a scale byte 0xFF is outside this restatement.
    mutant (tests/test_mxfp4_cpu.py proves the designed inputs see them):
      nan_code0   the kernel before the 0xFF rule: a NaN is left out of amax and becomes code 0 under the block's finite scale; an
                  infinity sets e = 126 (e8 = 253), saturates to code 7 and zeroes the rest of its block
      iter2       a thread's second loop iteration is dropped: blocks 256 .. of a row are never written (left 0)"""
    assert mutant is None or mutant in MUTANTS, mutant
    W = W.detach().to(torch.float32)
    rows, cols = W.shape
    assert cols % BLOCK == 0, cols
    blk = W.reshape(rows, cols // BLOCK, BLOCK)
    bad = ~torch.isfinite(blk).all(-1)
    if mutant == "nan_code0":
        blk = torch.where(torch.isnan(blk), torch.zeros_like(blk), blk)
        amax = blk.abs().amax(-1)
        inf = torch.isinf(amax)
        e = torch.where(inf, torch.full_like(amax, 126, dtype=torch.int32), block_exponent(torch.where(inf, torch.ones_like(amax), amax)))
    else:
        blk = torch.where(torch.isfinite(blk), blk, torch.zeros_like(blk))
        e = block_exponent(blk.abs().amax(-1))
    scaled = torch.ldexp(blk, -e[..., None])                   # w / 2^e, exact
    c = e2m1_codes(scaled).reshape(rows, cols // 2, 2)
    codes = c[..., 0] | (c[..., 1] << 4)
    e8 = (e + 127).to(torch.uint8)
    if mutant != "nan_code0":
        e8 = torch.where(bad, torch.full_like(e8, E8_NAN), e8)
    if mutant == "iter2":
        e8[:, 256:] = 0
        codes[:, 256 * (BLOCK // 2):] = 0
    return codes.contiguous(), e8.contiguous()


def mask_nonfinite(codes: torch.Tensor, e8: torch.Tensor) -> torch.Tensor:
    """codes with the 16 bytes of every block whose scale byte is 0xFF set to 0 (they are unspecified)"""
    keep = (e8 != E8_NAN).repeat_interleave(BLOCK // 2, dim=1)
    return torch.where(keep, codes, torch.zeros_like(codes))


def dequant_mxfp4(codes: torch.Tensor, e8: torch.Tensor) -> torch.Tensor:
    """(codes [rows][cols / 2], e8 [rows][cols / 32]) -> fp32 [rows][cols]"""
    rows, half = codes.shape
    c = torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(rows, half * 2).to(torch.int64)
    grid = torch.tensor(GRID, dtype=torch.float32)
    v = grid[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0)
    e = e8.to(torch.int32) - 127
    return torch.ldexp(v.reshape(rows, -1, BLOCK), e[..., None]).reshape(rows, half * 2)


def fold_zero(codes: torch.Tensor) -> torch.Tensor:
    """-0 (nibble 8) and +0 (nibble 0) are the same value: map every -0 nibble to +0 before comparing bytes"""
    lo, hi = codes & 0xF, codes >> 4
    lo = torch.where(lo == 8, torch.zeros_like(lo), lo)
    hi = torch.where(hi == 8, torch.zeros_like(hi), hi)
    return lo | (hi << 4)


def qdq_mxfp4(W: torch.Tensor) -> torch.Tensor:
    return dequant_mxfp4(*quant_mxfp4(W))


# ----------------------------------------------------------------------------- designed quantiser inputs
# every tie of the element grid, the grid itself and values beside the ties (units of the block scale)
TIE_VALS = (5.0, 3.5, 2.5, 1.75, 1.25, 0.75, 0.25, 7.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 5.5, 4.5, 0.125, 0.375, 7.5, 2.25, 2.75, 0.625, 0.875)
TIES = (5.0, 3.5, 2.5, 1.75, 1.25, 0.75, 0.25)
WIDE_COLS = 8256                       # 258 blocks: blocks 256 and 257 are a thread's second loop iteration
WIDE_BLOCKS = ((255, -3), (256, 4), (257, -9), (0, 2), (1, -6), (130, 11))      # (block, k): ties at scale 2^k


def _is_bf16(W):
    return torch.equal(W.to(torch.bfloat16).to(torch.float32), W)


def _tie_block(sign, k, top=6.0):
    """32 values: the members of TIE_VALS up to `top` times sign, and +top last so that the block's amax is top; all times 2^k"""
    vals = [v for v in TIE_VALS if v <= top]
    b = torch.zeros(32, dtype=torch.float64)
    b[:len(vals)] = torch.tensor(vals, dtype=torch.float64) * sign
    b[31] = top
    return b * 2.0 ** k


def clamp_tie_matrix():
    """The ties where the block exponent clamps, beside blocks of another exponent (64 columns, both signs):
         amax 3 * 2^-127 in [2^-126, 2^-125): floor(log2) - 2 = -128 clamps to -127, e8 = 0, the elements are w * 2^127;
         amax 1.5 * 2^-127, a bf16 subnormal: its exponent field reads -129 and clamps, e8 = 0;
         amax 6 * 2^-127 in [2^-125, 2^-124): e = -127 without the clamp, e8 = 0;
         amax 7 * 2^125 = 1.75 * 2^127: e = 125, e8 = 252, the largest scale byte a bf16 block can have.
    -> (W, expected e8 per row)"""
    rows, e8 = [], []
    for sign in (1.0, -1.0):
        rows.append(torch.cat([_tie_block(sign, -127, 3.0), _tie_block(-sign, -120)]))
        e8.append([0, 7])
        rows.append(torch.cat([_tie_block(sign, -127, 1.5), _tie_block(-sign, 125, 7.0)]))
        e8.append([0, 252])
        rows.append(torch.cat([_tie_block(sign, -127), _tie_block(sign, 125, 7.0)]))
        e8.append([0, 252])
    W = torch.stack(rows).to(torch.float32)
    assert _is_bf16(W) and torch.equal(W.double(), torch.stack(rows))
    return W, e8


def wide_tie_matrix():
    """two rows (one per sign) of WIDE_COLS columns: tie blocks at WIDE_BLOCKS, each under its own exponent, zeros elsewhere"""
    W = torch.zeros(2, WIDE_COLS, dtype=torch.float64)
    for r, sign in enumerate((1.0, -1.0)):
        for b, k in WIDE_BLOCKS:
            W[r, 32 * b:32 * b + 32] = _tie_block(sign, k)
    W = W.to(torch.float32)
    assert _is_bf16(W)
    return W


def nonfinite_matrices():
    """[(what, W, twin, bad)]: W holds NaN / inf elements at chosen places, twin is W with them set to 0, bad = {(row, block)} of the
    blocks that hold one.  Neighbouring blocks differ in exponent, so a scale taken from the wrong block shows."""
    g = torch.Generator().manual_seed(77)
    out = []
    for what, cols, spots in (("narrow", 128, [(0, 37, float("nan")), (1, 64, float("inf")), (2, 31, float("-inf")), (2, 100, float("nan")),
                                                (3, 5, float("nan")), (3, 6, float("inf"))]),
                              ("wide", WIDE_COLS, [(0, 32 * 257 + 9, float("nan")), (0, 32 * 255, float("inf")), (1, 32 * 256 + 31, float("-inf"))])):
        rows = 1 + max(r for r, _, _ in spots)
        k = torch.randint(-8, 9, (rows, cols // 32), generator=g)
        twin = (torch.randn((rows, cols), generator=g) * torch.exp2(k.float()).repeat_interleave(32, dim=1)).to(torch.bfloat16).to(torch.float32)
        W = twin.clone()
        for r, c, v in spots:
            W[r, c], twin[r, c] = v, 0.0
        out.append((what, W, twin, {(r, c // 32) for r, c, _ in spots}))
    return out


class Mxfp4Emu(O.Fp8Emu):
    """svln_set_mxfp4_decode as a CPU restatement: the decode step's four projections and every lm_head product read the MXFP4
    quantise -> dequantise of the weights; activations stay in the engine dtype (weight-only).  Blocks lie inside rows, so the engine's
    fused q|k|v matrix gives the same values as q / k / v quantised apart."""

    def __init__(self):
        super().__init__(decode=True, gemm=False)

    def weight(self, w, name):
        t = self._dq.get(name)
        if t is None:
            with O._DQ_LOCK:
                t = self._dq.get(name)
                if t is None:
                    t = self._dq[name] = qdq_mxfp4(w[name])
        return t
