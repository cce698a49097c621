"""CPU case builder, float64 reference and mutant references of the e4m3 products on the block-scaled MFMAs (svln_op_gemm_fp8 with
force_cfg | 0x40000; gemm.hip: the fp8s_t rows of the variant table).  Test infrastructure built on tests/gemm_ref.py: a ScaledCase is a
gemm_ref.Case (same operand layout, poison, strides, plan lookup, scale / split / epilogue mutants) with the flag set and more mutants.

Two exact families, both compared bit for bit by the GPU test:
  sign      the +-1 bytes of gemm_ref with power-of-two per-row scales: every product is one quantum, a dropped, doubled or mispaired
            product changes the sum.  It never exercises the instruction's decode: 0x38 / 0xB8 are the only bytes.
  alphabet  rows of A rotate over three bands of e4m3 bytes, each with its own quantum (m % 3):
              normal     significands 8 .. 15 over 8, exponents -1 .. 1 (and +-0)            quantum 2^-4
              subnormal  bytes 0x01 .. 0x0F, either sign (k 2^-9: 0x01 .. 0x07 are subnormal)  quantum 2^-9
              top        bytes 0x78 .. 0x7E, either sign (256 .. 448)                          quantum 2^5
            W columns alternate between the normal band (even n, with +-0) and +-{1, 1.5} (odd n).  NaN codes (0x7F / 0xFF) never occur.
Exactness: every term of output (m, n) -- the products times the scales, the bias, the residual -- is a multiple of the power-of-two
quantum q0(m, n) = min(quantum of A row m x quantum of W row n x a_scale[m] x w_scale[n], quantum of bias / residual), and
load() = (sum |a w| + |bias| + |res|) / q0 stays below 2^23, so every fp32 partial sum is exact in any order and the expected stored bits
are the float64 value rounded once to bf16.  tests/test_fp8_scaled_inputs.py asserts the condition for every case.

Mutants of the scaled form (float64, on the same bytes):
  decode_e5m2 / decode_fnuz   the format selector wrong: bytes read as e5m2 / as e4m3fnuz (bias 8; 0x80 is its NaN)
  flush_subnormals            bytes with a zero exponent field read as 0
  block_scale_126             E8M0 126 = 0.5 on one operand
  drop_upper_16               the second 16-byte chunk of a lane's 32-byte fragment never fed
  chunk_pairing               A feeds chunks (4t + h, 4t + 2 + h) to lane half h, W feeds (4t + 2h, 4t + 2h + 1)
                              (8-phase: (g, 4 + g) against (2g, 2g + 1) for lane group g)
  step_twice / drop_ragged_step   the first MFMA step summed twice; a last step that is not full (chunks past K are zeros) left out
"""
import torch

import gemm_ref as R
from streamvln_amd import _lib

SCALED = _lib.GEMM_FORCE_FP8_SCALED
LADDER = (1, 2, 3, 5, 7, 8, 9, 12, 16, 17, 25, 57)      # K in chunks: ragged inside a 4-chunk MFMA step, inside a stage, ring depths 2 / 3 / 6 and one past
BF16 = torch.bfloat16
NEW_MUTANTS = ("decode_e5m2", "decode_fnuz", "flush_subnormals", "block_scale_126", "drop_upper_16", "chunk_pairing", "step_twice", "drop_ragged_step")
# byte alphabets (positive codes; the sign bit is drawn separately)
NORMAL = [(e << 3) | mant for e in (6, 7, 8) for mant in range(8)]        # exponent field 6 .. 8 = 2^-1 .. 2^1
SUBNORMAL = list(range(0x01, 0x10))
TOP = list(range(0x78, 0x7F))
ONE_ONEHALF = [0x38, 0x3C]
QA = (2.0 ** -4, 2.0 ** -9, 2.0 ** 5)          # quantum of an A row by band (m % 3)
QW = (2.0 ** -4, 2.0 ** -1)                   # quantum of a W row (n % 2)


def decode(b, how="e4m3fn"):
    """float64 values of e4m3 bytes under a decode"""
    if how == "e4m3fn":
        return b.view(torch.float8_e4m3fn).float().double()
    if how == "e5m2":
        return b.view(torch.float8_e5m2).float().double()
    if how == "fnuz":
        return b.view(torch.float8_e4m3fnuz).float().double()
    assert how == "flush"
    return torch.where((b & 0x78) == 0, torch.zeros((), dtype=torch.float64), b.view(torch.float8_e4m3fn).float().double())


class ScaledCase(R.Case):
    def __init__(self, M, N, kc, family="sign", cfg=0, **kw):
        self.family = family
        super().__init__(BF16, M, N, kc, cfg=cfg | SCALED, fp8=True, **kw)
        assert family in ("sign", "alphabet") and (family == "sign" or self.epi == "none")
        self.p8 = self.geom["cfg"] == "p8"
        self.step_chunks = 8 if self.p8 else 4                       # 16-byte chunks of K per MFMA
        self.id = f"{family}-" + self.id

    def build(self):
        if self._built:
            return self
        super().build()
        if self.family == "alphabet":
            M, N, K = self.M, self.N, self.K
            g = torch.Generator().manual_seed(9000 + self.seed)
            pick = lambda codes, *shape: torch.tensor(codes, dtype=torch.uint8)[torch.randint(0, len(codes), shape, generator=g)]
            sgn = lambda *shape: (torch.randint(0, 2, shape, generator=g) * 0x80).to(torch.uint8)
            bands = [pick(NORMAL + [0x00], M, K), pick(SUBNORMAL, M, K), pick(TOP, M, K)]
            m = torch.arange(M)
            A = torch.where((m % 3 == 0)[:, None], bands[0], torch.where((m % 3 == 1)[:, None], bands[1], bands[2])) | sgn(M, K)
            n = torch.arange(N)
            W = torch.where((n % 2 == 0)[:, None], pick(NORMAL + [0x00], N, K), pick(ONE_ONEHALF, N, K)) | sgn(N, K)
            self.Abuf[:, :K], self.Wbuf[:, :K] = A, W
            self.planted = ()
            if self.bias is not None:
                self.bias = torch.randint(-2, 3, (N,), generator=g).double() * 8 * self.w_scale
            if self.res is not None:
                self.res = torch.randint(-3, 4, (self.res.shape[0], N), generator=g).double() * 8 * self.w_scale[None]
        return self

    # ---------------------------------------------------------------------------------------------------------- exactness
    def quantum(self):
        """q0 [M][N]: the power of two every term of an output is a multiple of"""
        self.build()
        m, n = torch.arange(self.M), torch.arange(self.N)
        if self.family == "sign":
            q = (self.a_scale[:, None] * self.w_scale[None]).clone()
            other = self.w_scale                                     # bias / residual: integers times 2^ew
        else:
            qa, qw = torch.tensor(QA, dtype=torch.float64)[m % 3], torch.tensor(QW, dtype=torch.float64)[n % 2]
            q = (qa * self.a_scale)[:, None] * (qw * self.w_scale)[None]
            other = 8 * self.w_scale
        if self.bias is not None or self.res is not None:
            q = torch.minimum(q, other[None].expand_as(q))
        return q

    def load(self):
        self.build()
        A, W = decode(self.Abuf[:, :self.K]).abs(), decode(self.Wbuf[:, :self.K]).abs()
        s = (A @ W.t()) * self.a_scale[:, None] * self.w_scale[None]
        if self.bias is not None:
            s = s + self.bias.abs()[None]
        if self.res is not None:
            s = s + self.res.abs().max(0).values[None]
        return s / self.quantum()

    def terms_on_quantum(self):
        """every term is a multiple of q0 (the products by construction of the bands: checked on the values themselves)"""
        self.build()
        q = self.quantum()
        whole = lambda v: bool((v == v.round()).all())
        qa = (q / (self.a_scale[:, None] * self.w_scale[None]))      # what a_scale w_scale (a w) has to be a multiple of, per output
        A, W = decode(self.Abuf[:, :self.K]), decode(self.Wbuf[:, :self.K])
        # a w is a multiple of (row quantum of A) x (row quantum of W), itself a multiple of qa
        if self.family == "sign":
            ra, rw = torch.ones(self.M, dtype=torch.float64), torch.ones(self.N, dtype=torch.float64)
        else:
            ra = torch.tensor(QA, dtype=torch.float64)[torch.arange(self.M) % 3]
            rw = torch.tensor(QW, dtype=torch.float64)[torch.arange(self.N) % 2]
        ok = whole(A / ra[:, None]) and whole(W / rw[:, None]) and whole(ra[:, None] * rw[None] / qa)
        if self.bias is not None:
            ok = ok and whole(self.bias[None] / q)
        if self.res is not None:
            ok = ok and whole(self.res.abs().max(0).values[None] / q) and whole(self.res[:1] / q[:1])
        return ok

    # ---------------------------------------------------------------------------------------------------------- mutants
    def steps(self):
        return R.cdiv(self.kc, self.step_chunks)

    def mutants(self):
        m = super().mutants()
        if not self.exact:
            return m
        self.build()
        body = torch.cat([self.Abuf[:, :self.K].reshape(-1), self.Wbuf[:, :self.K].reshape(-1)])
        m += ["decode_e5m2", "decode_fnuz", "block_scale_126", "step_twice"]
        if bool((((body & 0x78) == 0) & ((body & 0x07) != 0)).any()):
            m.append("flush_subnormals")
        sc = self.step_chunks
        if any(c % sc >= sc // 2 for c in range(self.kc)):
            m.append("drop_upper_16")
        if self.kc >= 2:
            m.append("chunk_pairing")
        if self.kc % sc:
            m.append("drop_ragged_step")
        return m

    def accumulate(self, mutant=None):
        if mutant not in NEW_MUTANTS:
            return super().accumulate(mutant)
        self.build()
        K, sc = self.K, self.step_chunks
        how = {"decode_e5m2": "e5m2", "decode_fnuz": "fnuz", "flush_subnormals": "flush"}.get(mutant, "e4m3fn")
        A, W = decode(self.Abuf[:, :K].contiguous(), how), decode(self.Wbuf[:, :K].contiguous(), how)
        chunk = torch.arange(K) // 16
        if mutant == "block_scale_126":
            W = W * 0.5
        elif mutant == "drop_upper_16":
            A = A * (chunk % sc < sc // 2).double()[None]
        elif mutant == "step_twice":
            A = A * torch.where(chunk < sc, 2.0, 1.0).double()[None]
        elif mutant == "drop_ragged_step":
            A = A * (chunk < (self.kc // sc) * sc).double()[None]
        elif mutant == "chunk_pairing":
            # A chunk c of a step meets W chunk pair[c] of it (chunks past K: zeros, as staged from the zero line)
            pair = (0, 2, 1, 3) if sc == 4 else (0, 2, 4, 6, 1, 3, 5, 7)
            full = self.steps() * sc
            Wp = torch.zeros((self.N, full, 16), dtype=torch.float64)
            Wp[:, :self.kc] = W.view(self.N, self.kc, 16)
            c = torch.arange(full)
            W = Wp[:, (c // sc) * sc + torch.tensor(pair)[c % sc]][:, :self.kc].reshape(self.N, K)
        return (A @ W.t()) * self.a_scale[:, None] * self.w_scale[None]


# -------------------------------------------------------------------------------------------------------------- the case list
P8, RING, DIRECT = 256, 256 | R.RING, 256 | R.DIRECT


def cases():
    out = []

    def add(*a, **k):
        out.append(ScaledCase(*a, seed=len(out), **k))

    bn_of = lambda M, **kw: R.plan(True, True, M, 1024, 256, kw.get("epi", "none"), kw.get("cfg", 0) | SCALED, kw.get("split", 0))["BN"]
    # ---- every tile of the scaled form, unsplit, over the chunk ladder; the families alternate and each tile sees both
    tiles = (dict(cfg=32, M=19, split=1), dict(cfg=64, M=70), dict(cfg=128, M=165), dict(cfg=129, M=165), dict(M=70, split=1),
             dict(cfg=RING, M=293), dict(cfg=P8, M=293))
    for i, kc in enumerate(LADDER):
        for j, t in enumerate(tiles):
            kw = dict(t)
            M = kw.pop("M")
            fam = ("sign", "alphabet")[(i + j) % 2]
            p8 = kw.get("cfg") == P8
            N = bn_of(M, **kw) + 75
            # the 8-phase kernel: LDS-staged stores (ldc % 8 == 0) and direct ones (odd ldc, or | 0x20000) in turn
            padc = (8 - N % 8) % 8 + 8 if p8 and i % 2 == 0 else 9
            if p8 and i % 4 == 3:
                kw["cfg"] = DIRECT
                padc = (8 - N % 8) % 8 + 8
            add(M, N, kc, family=fam, bias=True, res=(i + j) % 3 != 0, padc=padc, **kw)
    # ---- K-split launches: 2, 3, 5 slices, one of them empty (16 chunks = 2 stages in 5 slices is capped; 17 = 3 stages in 5)
    for i, (kc, S) in enumerate(((9, 2), (17, 3), (57, 5), (17, 5), (25, 2), (12, 3))):
        add(70, 128 + 76, kc, family=("alphabet", "sign")[i % 2], split=S, bias=True, res=True)
        add(19, 128 + 76, kc, family=("sign", "alphabet")[i % 2], cfg=32, split=S, bias=i % 2 == 0, res=True)
    # ---- SwiGLU (toleranced over exact accumulators, as in gemm_ref): every tile, and through the slabs
    for kc, t in zip((5, 9, 12, 17, 7, 25, 16, 57), tiles + (dict(cfg=P8, M=293),)):
        kw = dict(t)
        M = kw.pop("M")
        add(M, bn_of(M, epi="swiglu", **kw) + 64, kc, epi="swiglu", padc=8 if kc == 57 else 9, **kw)      # (kc 57: the 8-phase kernel's staged stores)
    add(70, 128 + 64, 57, split=2, epi="swiglu")
    add(19, 128 + 64, 25, cfg=32, split=3, epi="swiglu")
    # ---- more than one round of 128x128 tiles (the 128L rows), dense operands
    add(1300, 3400, 17, family="alphabet", cfg=128, bias=True, res=True, pad=(0, 0))
    add(1300, 3392, 9, cfg=128, epi="swiglu")
    # ---- the heuristics with the flag alone: one row tile (K split by the planner), several row tiles
    add(70, 128 + 76, 57, family="alphabet", bias=True, res=True)
    add(293, 128 + 75, 17, family="alphabet", bias=True, pad=(0, 0))
    return out


CASES = cases()
