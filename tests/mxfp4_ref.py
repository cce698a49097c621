"""CPU restatement of the engine's MXFP4 weight scheme (test infrastructure; DESIGN.md section 6, include/streamvln_hip.h
svln_op_quant_mxfp4).  This is the OCP MX conversion, nothing project-specific:

  * every run of 32 consecutive elements of a row is one block; amax = max |w|; e = floor(log2(amax)) - 2 (2 = E2M1's largest
    exponent) clamped to [-127, 127], 0 for an all-zero block; the stored scale byte is e + 127 (E8M0), the scale 2^e exactly;
  * element code = E2M1 of w / 2^e (exact in fp32) on the grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, round to nearest, ties to the code with
    an even mantissa bit (5 -> 4, 3.5 -> 4, 2.5 -> 2, 1.75 -> 2, 1.25 -> 1, 0.75 -> 1, 0.25 -> 0), saturating at 6; sign in bit 3;
  * element 2j in the low nibble, 2j + 1 in the high nibble of byte j.
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


def quant_mxfp4(W: torch.Tensor):
    """W [rows][cols] (cols % 32 == 0; fp32 or bf16) -> (codes uint8 [rows][cols / 2], e8 uint8 [rows][cols / 32])"""
    W = W.detach().to(torch.float32)
    rows, cols = W.shape
    assert cols % BLOCK == 0, cols
    blk = W.reshape(rows, cols // BLOCK, BLOCK)
    e = block_exponent(blk.abs().amax(-1))
    scaled = torch.ldexp(blk, -e[..., None])                   # w / 2^e, exact
    c = e2m1_codes(scaled).reshape(rows, cols // 2, 2)
    codes = c[..., 0] | (c[..., 1] << 4)
    return codes.contiguous(), (e + 127).to(torch.uint8).contiguous()


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
