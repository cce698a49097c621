"""CPU case builder and float64 reference of the MFMA GEMMs (streamvln_amd/csrc/gemm.hip) behind svln_op_gemm / _gemm_norm / _gemm_norm_q8 /
_gemm_fp8, and "mutant" references (plausible kernel mistakes) that prove the inputs sharp.  Test infrastructure, modelled on
tests/gemv_ref.py.

The exact family.  Every operand is a signed power of two whose exponent changes with every row,
    A[m][k] = +-2^ea[m],  ea[m] = (3 m mod 5) - 2        W[n][k] = +-2^ew[n],  ew[n] = (5 n mod 7) - 3
with seeded-random signs, so no product is zero, every product of output (m, n) is +-2^(ea[m] + ew[n]) and an output is that quantum times
a small integer (a sum of K signs: |sum| stays far below 256, so one dropped or doubled product changes the stored bf16 bits).  e4m3 cases
store +-1 bytes and carry 2^ea / 2^ew as the per-row a_scale / w_scale.  Bias and residual are small integers times 2^ew[n].  While
sum |a w| (+ |bias| + |res|) of an output stays below 2^23 quanta every fp32 partial sum is exact in any order -- across MFMA steps, K
slices (fp32 slabs) and in-workgroup K groups -- so the expected stored bits are the float64 value rounded ONCE to the engine type, and
the GPU test compares bits.  Planted columns (bf16 cases with bias and residual): bias 2^(ew + 9), residual -2^(ew + 9): acc + bias needs
more than 8 significant bits and the residual cancels it, so a kernel that rounds to the engine type before the residual add differs.

The toleranced family (float64 reference, util.assert_close): GELU-tanh, GELU-erf and SwiGLU over the same exact accumulators with a
narrower exponent spread (ea in -1 .. 1, ew in -2 .. 0; SwiGLU gates span at least [-12, 12]); and the norm the fused split-K reduce emits,
taken from the stored (bit-compared) rows.

Strides and poison.  lda, ldw > K with padding that holds 2^60 (e4m3: byte 0x7E = 448); ldc > n_out; the GPU test puts C between guard
rows filled with a sentinel.
"""
import math

import torch

from oracle import streamvln_oracle as O
from streamvln_amd import _lib

EPS = 1e-6
EPC = {"fp32": 4, "bf16": 8, "e4m3": 16}             # operand values per 16-byte chunk
LADDER = (1, 8, 9, 16, 17, 24, 25, 57)               # K in chunks: a ragged single stage, one stage, ring depths 2 / 3 (/ 6: 48 + 9) and one past
POISON = 2.0 ** 60
FILL = 777.0                                         # sentinel of the output buffers (guard rows, ldc padding)
WS_ELEMS = 8 * 3 * 729 * 1024                        # split-K workspace of the TINY engine the GPU test creates (max_frames 3), fp32 elements
DIRTY = 16384.0                                      # what the slabs hold before a split case (the GPU test runs a product that leaves it)
# what the reference needs of a tile configuration of gemm.hip and the plan does not report: (ring depth | "p8", K groups)
CFGS = {"skinny": (3, 1), "c64": (6, 1), "c128": (2, 1), "c128L": (2, 1), "c128K2": (2, 2), "c256": (3, 1), "c256n64": (3, 1), "big": (2, 1),
        "p8": ("p8", 1), "p8_32": ("p8", 1)}
EPI_ID = {"none": 0, "gelu_tanh": 1, "gelu_erf": 2, "swiglu": 3}


def cdiv(a, b):
    return -(-a // b)


def representable(v, dtype):
    return v.to(dtype).to(torch.float64) == v


# ---------------------------------------------------------------------------------------------------------- the dispatcher's plan
def plan(bf16, fp8, M, N, K, epi, force_cfg=0, force_split=0, norm=False, res=False):
    """what the dispatcher itself (gemm_plan.h through svln_gemm_plan; no GPU) does with a product issued by the op entry points of the GPU
    test's engine: {cfg, BM, BN, S (K slices of the main launch), tail (None | (first tile, S of the tail launch)), fused (the reduce emits
    the norm)}.  It places the cases (coverage, which mutants apply); no expected value depends on it."""
    g = _lib.gemm_plan(dtype=_lib.SVLN_BF16 if bf16 else _lib.SVLN_F32, epi=EPI_ID[epi], M=M, N=N, K=K, fp8=int(fp8), has_ws=1, ws_elems=WS_ELEMS,
                       has_zeros=1, norm_out=int(norm), norm_w=int(norm), res=int(res), force_cfg=force_cfg, force_split=force_split)
    main, tail = g.launch[0], g.launch[1] if g.n_launches == 2 else None
    return {"cfg": _lib.GEMM_TILES[main.tile], "BM": main.bm, "BN": main.bn, "S": main.nsplit, "tail": (tail.tile_base, tail.nsplit) if tail else None,
            "fused": bool(g.fused)}


def k_slices(stages, S):
    """[begin, end) in stages of every K slice: stages_per = ceil(stages / S); a slice past the end is empty"""
    per = cdiv(stages, S)
    return [(min(s * per, stages), min(stages, (s + 1) * per)) for s in range(S)]


# ---------------------------------------------------------------------------------------------------------- cases
class Case:
    """One call of svln_op_gemm (entry "gemm"), svln_op_gemm_norm ("norm"), svln_op_gemm_norm_q8 ("q8") or svln_op_gemm_fp8 ("fp8").
    kc       K in 16-byte chunks of the operand format;   epi "none" | "gelu_tanh" | "gelu_erf" | "swiglu"
    pads     (lda - K, ldw - K) in chunks, ldc - n_out in elements;   inplace: C == res, ldr == ldc;   norm None | "rms" | "ln" """

    def __init__(self, dtype, M, N, kc, cfg=0, split=0, epi="none", bias=False, res=False, res_mod=0, fp8=False, pad=(2, 3), padc=9,
                 inplace=False, norm=None, q8=False, seed=0, note=""):
        self.dtype, self.M, self.N, self.kc, self.force_cfg, self.force_split, self.epi = dtype, M, N, kc, cfg, split, epi
        self.bias_on, self.res_on, self.res_mod, self.fp8, self.inplace, self.norm, self.q8, self.seed = bias, res or inplace, res_mod, fp8, inplace, norm, q8, seed
        self.bf16 = dtype == torch.bfloat16
        self.fmt = "e4m3" if fp8 else "bf16" if self.bf16 else "fp32"
        self.epc = EPC[self.fmt]
        self.K = kc * self.epc
        self.lda, self.ldw = self.K + pad[0] * self.epc, self.K + pad[1] * self.epc
        self.n_out = N // 2 if epi == "swiglu" else N
        self.ldc = self.n_out + padc
        self.ldr = self.ldc if inplace else N + 5
        self.entry = "fp8" if fp8 else "q8" if q8 else "norm" if norm else "gemm"
        self.exact = epi == "none"
        assert not (inplace and (res_mod or epi == "swiglu")) and not (fp8 and not self.bf16) and not (norm and (cfg or epi != "none" or res_mod))
        self.geom = plan(self.bf16, fp8, M, N, self.K, epi, cfg, split, norm is not None, self.res_on)
        self.BM, self.BN = self.geom["BM"], self.geom["BN"]
        self.ring, self.KG = CFGS[self.geom["cfg"]]
        self.stages = cdiv(kc, 8)
        S, tail = self.geom["S"], self.geom["tail"]
        self.split_S = tail[1] if tail else S                                   # K slices of the split launch (1: none)
        self.split_col0 = tail[0] * 128 if tail else 0                          # first weight row (column of the product) the split launch covers
        # the 8-phase kernel stores through LDS when the rows of C are 16-byte aligned (the GPU test aligns C itself to 16 bytes)
        self.staged = self.geom["cfg"] == "p8" and S == 1 and self.ldc % 8 == 0 and not cfg & 0x20000
        self.id = f"{self.fmt}-{self.geom['cfg']}-{M}x{N}x{kc}c-{epi}" + (f"-cfg{cfg:#x}" if cfg else "") + (f"-split{split}" if split else "") + \
                  ("-bias" if bias else "") + ("-res" if self.res_on else "") + (f"-mod{res_mod}" if res_mod else "") + ("-inplace" if inplace else "") + \
                  (f"-{norm}" if norm else "") + ("-q8" if q8 else "") + ("" if pad != (0, 0) else "-dense") + (f"-{note}" if note else "")
        self._built = False

    # ------------------------------------------------------------------------------------------------------ operands
    def build(self):
        if self._built:
            return self
        self._built = True
        M, N, K = self.M, self.N, self.K
        g = torch.Generator().manual_seed(4000 + self.seed)
        sign = lambda *shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
        m, n = torch.arange(M), torch.arange(N)
        if self.exact:
            self.ea, self.ew = ((3 * m) % 5 - 2).double(), ((5 * n) % 7 - 3).double()
        else:
            self.ea, self.ew = (m % 3 - 1).double(), (n % 3 - 2).double()
        if self.epi == "swiglu":       # a gate row and its up row (32 further) share the exponent pattern of their block position
            self.ew = ((n % 32) % 3 - 1).double()
        sa, sw = sign(M, K), sign(N, K)
        self.a_scale, self.w_scale = torch.exp2(self.ea), torch.exp2(self.ew)
        if self.fp8:
            Abuf = torch.full((M, self.lda), 0x7E, dtype=torch.uint8)
            Wbuf = torch.full((N, self.ldw), 0x7E, dtype=torch.uint8)
            Abuf[:, :K] = sa.float().to(torch.float8_e4m3fn).view(torch.uint8)
            Wbuf[:, :K] = sw.float().to(torch.float8_e4m3fn).view(torch.uint8)
        else:
            Abuf = torch.full((M, self.lda), POISON, dtype=torch.float64)
            Wbuf = torch.full((N, self.ldw), POISON, dtype=torch.float64)
            Abuf[:, :K] = sa * self.a_scale[:, None]
            Wbuf[:, :K] = sw * self.w_scale[:, None]
            Abuf, Wbuf = Abuf.to(self.dtype), Wbuf.to(self.dtype)
        self.Abuf, self.Wbuf = Abuf, Wbuf
        self.bias = torch.randint(-2, 3, (N,), generator=g).double() * self.w_scale if self.bias_on else None
        self.res = None
        if self.res_on:
            rows = self.res_mod if self.res_mod else M
            self.res = torch.randint(-3, 4, (rows, N), generator=g).double() * self.w_scale[None]
        self.planted = ()
        if self.exact and self.bf16 and self.bias_on and self.res_on:
            self.planted = tuple(sorted({3, N - 2, min(self.BN + 1, N - 1)}))
            for c in self.planted:
                self.bias[c] = 2.0 ** (float(self.ew[c]) + 9)
                self.res[:, c] = -self.bias[c]
        self.g = self.nb = None
        if self.norm:
            self.g = ((0.5 + torch.rand((N,), generator=g).double()) * sign(N)).to(self.dtype).double()
            if self.norm == "ln":
                self.nb = (torch.rand((N,), generator=g).double() - 0.5).to(self.dtype).double()
        return self

    def _operand(self, buf, ld, scale, width):
        """float64 [rows][width] of what a kernel that reads `width` values per row finds in memory (past K: the padding, then the next row)"""
        flat = buf.reshape(-1)
        if width > self.K:
            flat = torch.cat([flat, flat[-1:].expand(width)])
        v = flat.as_strided((buf.shape[0], width), (ld, 1)).clone()
        v = v.view(torch.float8_e4m3fn).float().double() if self.fp8 else v.double()
        return v                                            # (e4m3 scales are applied to the accumulator, as the kernel does)

    # ------------------------------------------------------------------------------------------------------ mutants
    def groups(self):
        """[begin, end) in stages of the two in-workgroup K groups (Cfg128K2) of an unsplit launch"""
        per = cdiv(self.stages, 2)
        return [(0, min(per, self.stages)), (min(per, self.stages), min(self.stages, 2 * per))]

    def mutants(self):
        self.build()
        m, S = [], self.split_S
        if self.exact:
            if self.kc % 8:
                m += ["drop_ragged_stage", "read_past_K"]
            if S > 1:
                m.append("drop_last_slice")
                if self.stages > cdiv(self.stages, S):
                    m.append("double_boundary_stage")
                if self.ldc != self.N and not self.geom["tail"]:
                    m.append("slab_ldc")
            if self.KG == 2 and self.groups()[1][1] > self.groups()[1][0]:
                m += ["drop_second_kgroup", "double_boundary_stage"]
            if self.planted:
                m.append("round_before_res")
        if self.bias_on and self.N > self.BN:
            m.append("bias_tile_col")
        if self.res_on and self.epi != "swiglu":
            if self.res_mod and self.M > self.res_mod:
                m.append("res_ignores_mod")
            if self.M > self.BM and (self.res_mod == 0 or self.BM % self.res_mod):
                m.append("res_mod_tile")
            if self.epi.startswith("gelu"):
                m.append("res_before_act")
        if self.epi == "swiglu":
            m += ["gate_up_swapped", "gate_up_neighbour_block"]
        if self.geom["tail"]:
            m.append("tail_begin_off_by_one")
        if self.fp8:
            m += ["a_scale_by_column", "w_scale_by_row"] + (["scale_twice_per_slab"] if S > 1 else [])
        return m

    def _k_weight(self, mutant, width):
        """how often every K position is summed under the mutant (1 everywhere for the kernel as written)"""
        per_stage = 8 * self.epc
        w = torch.ones(width, dtype=torch.float64)
        stage = lambda s: slice(s * per_stage, (s + 1) * per_stage)
        if mutant == "drop_ragged_stage":
            w[stage(self.stages - 1)] = 0
        elif mutant == "drop_last_slice":
            b, e = [sl for sl in k_slices(self.stages, self.split_S) if sl[1] > sl[0]][-1]
            w[b * per_stage:e * per_stage] = 0
        elif mutant == "drop_second_kgroup":
            b, e = self.groups()[1]
            w[b * per_stage:e * per_stage] = 0
        elif mutant == "double_boundary_stage":
            w[stage(self.groups()[1][0] if self.KG == 2 else cdiv(self.stages, self.split_S))] = 2
        return w

    def accumulate(self, mutant=None):
        """float64 A . W^T [M][N] (e4m3: times the scales) as the fp32 accumulators / summed slabs hold it, under `mutant`"""
        self.build()
        M, N = self.M, self.N
        width = self.stages * 8 * self.epc if mutant == "read_past_K" else self.K
        A, W = self._operand(self.Abuf, self.lda, self.a_scale, width), self._operand(self.Wbuf, self.ldw, self.w_scale, width)
        acc = A @ W.t()
        if mutant in ("drop_ragged_stage", "drop_last_slice", "drop_second_kgroup", "double_boundary_stage"):
            mut = (A * self._k_weight(mutant, width)[None]) @ W.t()
            if mutant in ("drop_last_slice", "double_boundary_stage") and self.KG == 1:
                acc[:, self.split_col0:] = mut[:, self.split_col0:]            # (a tail launch: only its columns are K-split)
            else:
                acc = mut
        if self.fp8:
            sa = self.a_scale[:, None].expand(M, N)
            sw = self.w_scale[None].expand(M, N)
            if mutant == "a_scale_by_column":
                sa = self.a_scale[torch.arange(N).clamp(max=M - 1)][None].expand(M, N)
            if mutant == "w_scale_by_row":
                sw = self.w_scale[torch.arange(M).clamp(max=N - 1)][:, None].expand(M, N)
            acc = acc * sa * sw
            if mutant == "scale_twice_per_slab":
                acc = acc * sa * sw
        if mutant == "slab_ldc":       # the slices write slab[m * ldc + n], the reduce reads slab[m * N + n]: what it finds there
            f = torch.arange(M)[:, None] * N + torch.arange(N)[None]
            mm, nn = f // self.ldc, f % self.ldc
            acc = torch.where(nn < N, acc[mm.clamp(max=M - 1), nn.clamp(max=N - 1)], torch.full_like(acc, DIRTY * self.split_S))
        return acc

    def reference(self, mutant=None):
        """float64 C [M][n_out] before the one rounding to the engine type (round_before_res: with its extra rounding applied)"""
        acc = self.accumulate(mutant)
        M, N = self.M, self.N
        if self.epi == "swiglu":
            j = torch.arange(self.n_out)
            gate = (j // 32) * 64 + j % 32
            up = gate + 32
            if mutant == "gate_up_swapped":
                gate, up = up, gate
            if mutant == "gate_up_neighbour_block":
                up = (up + 64) % N
            out = O.silu(acc[:, gate]) * acc[:, up]
        else:
            n = torch.arange(N)
            if self.bias is not None:
                acc = acc + self.bias[n % self.BN if mutant == "bias_tile_col" else n][None]
            r = None
            if self.res is not None:
                m = torch.arange(M)
                rr = m % self.res_mod if self.res_mod else m
                if mutant == "res_ignores_mod":
                    rr = m.clamp(max=self.res.shape[0] - 1)
                if mutant == "res_mod_tile":
                    rr = (m % self.BM) % self.res_mod if self.res_mod else m % self.BM
                r = self.res[rr]
            if mutant == "res_before_act" and r is not None:
                acc, r = acc + r, None
            out = O.gelu_tanh(acc) if self.epi == "gelu_tanh" else O.gelu_erf(acc) if self.epi == "gelu_erf" else acc
            if mutant == "round_before_res":
                out = out.to(self.dtype).double()
            if r is not None:
                out = out + r
        if mutant == "tail_begin_off_by_one":       # the reduce of the tail launch starts one column tile late: that tile keeps the sentinel
            c0 = self.split_col0 // (2 if self.epi == "swiglu" else 1)
            out[:, c0:c0 + (64 if self.epi == "swiglu" else 128)] = FILL
        return out

    def norm_reference(self, stored):
        """float64 norm of the STORED rows (engine type), as splitk_rownorm_kernel takes it"""
        x = stored.double()
        if self.norm == "ln":
            mu = x.mean(1, keepdim=True)
            var = ((x - mu) ** 2).mean(1, keepdim=True)
            return (x - mu) / torch.sqrt(var + EPS) * self.g[None] + self.nb[None]
        return self.g[None] * (x / torch.sqrt((x * x).mean(1, keepdim=True) + EPS))

    def load(self):
        """sum |a w| (+ |bias| + |res|) of every output in quanta 2^(ea + ew): below 2^23 every fp32 partial sum is exact"""
        self.build()
        q = self.a_scale[:, None] * self.w_scale[None]
        s = torch.full((self.M, self.N), float(self.K), dtype=torch.float64)
        if self.bias is not None:
            s = s + self.bias.abs()[None] / q
        if self.res is not None:
            s = s + self.res.abs().max(0).values[None] / q
        return s

    def gate_span(self):
        acc = self.accumulate()
        j = torch.arange(self.n_out)
        gate = acc[:, (j // 32) * 64 + j % 32]
        return float(gate.min()), float(gate.max())


def bound(exp, dtype):
    """the per-element bound util.assert_close applies to an expected output"""
    from util import tol
    rt, at = tol(dtype)
    exp = exp.float().double()
    return at * max(1.0, float(exp.abs().max())) + rt * exp.abs()


def mutant_report(case):
    """{mutant: outputs whose stored bits change} (exact cases) or {mutant: max |mutant - reference| / bound} (toleranced cases)"""
    ref = case.reference()
    out = {}
    for m in case.mutants():
        mut = case.reference(m)
        if case.exact:
            out[m] = int((mut.to(case.dtype) != ref.to(case.dtype)).sum())
        else:
            out[m] = float(((mut - ref).abs() / bound(ref, case.dtype)).max())
    return out


# ---------------------------------------------------------------------------------------------------------- the case list
F32, BF16 = torch.float32, torch.bfloat16
P8_32, RING, DIRECT, BNFAST = 0x8000, 0x4000, 0x20000, 0x10000


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, seed=len(out), **k))
    dt = lambda i: (F32, BF16)[i % 2]
    epis = ("none", "none", "gelu_tanh", "none", "gelu_erf", "none", "none", "swiglu")
    # ---- forced configurations, unsplit: every rung of the ladder for every ring depth, dtypes alternating, epilogues rotating
    for i, kc in enumerate(LADDER):
        epi = epis[i]
        glu = epi == "swiglu"
        br = dict(bias=not glu, res=not glu and i % 2 == 0)
        # ring depth 3: 32x128 tiles (M = 19) and 256x128 tiles (force_split 1: M = 70 / 256, one row tile)
        add(dt(i), 19, 128 + (64 if glu else 75), kc, cfg=32, split=1, epi=epi, **br)
        add(dt(i + 1), (70, 256)[i % 2], 128 + (64 if glu else 75), kc, split=1, epi=epi, bias=not glu, res=not glu, res_mod=0 if glu else 50)
        # ring depth 6: 64x64 tiles
        add(dt(i), 64 + 37, 64 + (64 if glu else 75), kc, cfg=64, epi=epi, **br)
        # ring depth 2: 128x128 tiles, the same with two K groups, 256x256 tiles on the stage ring
        add(dt(i + 1), 128 + 37, 128 + (64 if glu else 75), kc, cfg=128 | (BNFAST if i == 3 else 0), epi=epi, inplace=i in (1, 5), **(br if i not in (1, 5) else dict(bias=True)))
        add(dt(i), 128 + 37, 128 + (64 if glu else 75), kc, cfg=129, epi=epi, bias=not glu, res=not glu, res_mod=0 if glu else 100)
        add(dt(i + 1), 256 + 37, 256 + (64 if glu else 75), kc, cfg=256 | RING, epi=epi, **br)
        # the 8-phase kernel (bf16): LDS-staged stores (ldc % 8 == 0) and direct ones (odd ldc, or | 0x20000) in turn
        n_out = (256 + 64) // 2 if glu else 256 + 75
        add(BF16, 256 + 37, 256 + (64 if glu else 75), kc, cfg=256 | (DIRECT if i == 5 else 0), epi=epi, padc=(8 - n_out % 8) % 8 + 8 if i % 2 == 0 or i == 5 else 9,
            bias=not glu, res=not glu, res_mod=0 if glu or i % 4 else 100)
    add(BF16, 256 + 37, 256 + 75, 9, cfg=256 | P8_32, bias=True, res=True)
    add(BF16, 256 + 37, 256 + 75, 16, cfg=256 | P8_32, epi="gelu_tanh", bias=True)
    add(F32, 256 + 37, 256 + 75, 17, cfg=256, bias=True, res=True)                                  # fp32: force_cfg 256 is the stage ring
    # ---- 256x64 tiles (force_cfg 264), unsplit and split (the launcher caps the slices at stages / 2)
    for i, kc in enumerate((1, 9, 17, 25)):
        add(dt(i), 256 + 37, 64 + 75, kc, cfg=264, epi=("none", "gelu_tanh")[i % 2], bias=True, res=i % 2 == 0)
    add(F32, 256 + 37, 64 + 76, 57, cfg=264, split=3, bias=True, res=True, res_mod=100)
    add(BF16, 256 + 37, 64 + 76, 57, cfg=264, split=2, bias=True, res=True)
    add(BF16, 70, 64 + 76, 41, cfg=264, split=2, inplace=True)
    # ---- split-K: {2, 3, 5} slices on 256x128 and 32x128 tiles; more slices than stages (empty slices); SwiGLU through the slabs
    for i, (kc, S) in enumerate(((9, 2), (17, 3), (57, 5), (16, 5), (8, 3), (25, 2), (24, 3))):
        add(dt(i), (70, 256, 256 + 37)[i % 3], 128 + 76, kc, split=S, bias=True, res=True, res_mod=(0, 50)[i % 2])
        add(dt(i + 1), 19, 128 + 76, kc, cfg=32, split=S, bias=i % 2 == 0, res=True)
    add(BF16, 70, 128 + 64, 17, split=2, epi="swiglu")
    add(F32, 19, 128 + 64, 25, cfg=32, split=3, epi="swiglu")
    add(BF16, 256, 128 + 76, 24, split=2, epi="gelu_erf", bias=True, res=True)
    add(F32, 70, 128 + 76, 9, split=3, inplace=True, bias=True)
    # ---- two K slices on the 8-phase kernel (force_cfg 258): one K tile (the second slice is empty), odd and even tile counts, ragged
    for i, kc in enumerate((8, 9, 16, 17, 24, 25, 57)):
        add(BF16, 256 + 37, 256 + 76, kc, cfg=258, bias=True, res=i % 2 == 0, res_mod=(0, 100)[i % 4 == 0])
    add(BF16, 256 + 37, 256 + 64, 17, cfg=258, epi="swiglu")
    # ---- default heuristics: one row tile (K split by the launcher; N % 4 != 0: unsplit), dense operands (lda == ldw == K)
    add(BF16, 70, 128 + 76, 57, bias=True, res=True)
    add(F32, 256, 128 + 75, 25, bias=True, res=True, res_mod=50)
    add(BF16, 256 + 37, 128 + 75, 17, bias=True, pad=(0, 0))
    add(F32, 70, 128 + 76, 25, bias=True, res=True, pad=(0, 0))
    add(BF16, 19, 128 + 76, 57, bias=True, res=True)
    # ---- more than one round of 128x128 tiles (Cfg128L) at a short K
    add(BF16, 1300, 3400, 17, cfg=128, bias=True, res=True, res_mod=729)
    add(F32, 1300, 3400, 17, cfg=128, epi="gelu_tanh", bias=True)
    # ---- tail-tile launch: one row tile, 296 column tiles: 256 unsplit + 40 K-split
    add(BF16, 70, 2 * 18944, 25, bias=True, res=True)
    add(F32, 70, 2 * 18944, 25, epi="swiglu")
    # ---- e4m3 operands (svln_op_gemm_fp8): per-row power-of-two scales
    for i, (kc, kw) in enumerate(((1, dict(cfg=32, M=19)), (9, dict(cfg=64, M=101)), (17, dict(cfg=128, M=165)), (25, dict(cfg=129, M=165)),
                                  (16, dict(split=1, M=70)), (57, dict(cfg=256, M=293)), (24, dict(cfg=128, M=165)), (8, dict(cfg=64, M=101)))):
        M = kw.pop("M")
        add(BF16, M, plan(True, True, M, 1024, kc * 16, "none", kw.get("cfg", 0), kw.get("split", 0))["BN"] + 75, kc, fp8=True, bias=True, res=i % 2 == 0, **kw)
    add(BF16, 70, 128 + 76, 17, split=3, fp8=True, bias=True, res=True)
    add(BF16, 19, 128 + 76, 25, cfg=32, split=5, fp8=True, bias=True)
    add(BF16, 165, 128 + 64, 9, cfg=128, fp8=True, epi="swiglu")
    add(BF16, 70, 128 + 64, 57, split=2, fp8=True, epi="swiglu")
    # ---- the norm emitted by the fused reduce (svln_op_gemm_norm / _q8): forced splits, the steady-prefill 256x64 route, the vit64 route
    add(BF16, 70, 128 + 76, 17, split=2, bias=True, res=True, norm="rms")
    add(F32, 256, 128 + 76, 57, split=5, bias=True, inplace=True, norm="ln")
    add(F32, 70, 1024 + 76, 257, res=True, norm="rms", note="n64")
    add(BF16, 70, 1024 + 76, 129, inplace=True, norm="rms", note="n64")
    add(BF16, 513, 64 + 76, 57, bias=True, res=True, norm="ln", note="vit64")
    add(F32, 513, 64 + 76, 57, bias=True, inplace=True, norm="rms", note="vit64")
    add(BF16, 70, 128 + 76, 25, split=3, res=True, norm="rms", q8=True)
    add(BF16, 256, 1024 + 76, 129, inplace=True, norm="rms", q8=True, note="n64")
    return out


CASES = cases()
