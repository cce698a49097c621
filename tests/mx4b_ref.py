"""CPU case builder and float64 reference of the batched MXFP4 GEMV (streamvln_amd/csrc/gemv_mx4b.hip, svln_op_gemv_mxfp4_batched), and
"mutant" references (plausible kernel mistakes) that prove the inputs sharp.  Test infrastructure in the manner of tests/gemv_ref.py,
whose helpers it imports.

The exact family.  Sparse E2M1 codes as in gemv_ref (a dense row would mix seven block scales and need more significant bits than bf16
keeps), e8[n][blk] = 127 + ((3 n + 5 blk) mod 7 - 3), dense x in {-1, 0, 1} with every one of the B rows different, small-integer bias
and residual.  A weight row keeps its second non-zero code only where all B outputs stay bf16 values, so EVERY expected output is a
bf16 value and the GPU test compares stored bits.  Poison: code byte 0x77 and scale byte 140 in the ldw padding of the weights, 3e4 in
the ldx / ldr padding of x and the residual.

What a case compares is the IMAGE of the y buffer: guard band | B rows of stride ldy > n_out | guard band, FILL wherever the kernel must
not write.  A mutant is the image a mistaken kernel would leave:
  nibbles_swapped        element 2j read from the high nibble
  scale_blk+1            a block taking its neighbour's scale byte
  k_perm_w_only          the in-super-step permutation of K (lane (r, g) spends block 4 s + g over four MFMAs, so MFMA j sums over
                         128 s + 32 g + 8 j + 0..7) applied to the weights while x is read in the natural order 128 s + 32 j + 8 g + 0..7
  drop_partial_superstep the blocks after the last whole 128-element super-step dropped           (K % 128 != 0)
  read_past_K            the last super-step read to its end: what lies after K in the memory of the weight rows and of x
  x_rows_swapped         rows 0 and 1 of X exchanged                                               (B >= 2)
  col_leak               the store not limited to b < B: the tile's columns B .. 15 stored as further rows of y
  up_16_apart            up rows paired 16 after their gate rows instead of 32                     (SwiGLU)
  tie_higher             an arg-max tie going to the higher index                                  (arg-max)
"""
import torch

import gemv_ref as G
import mxfp4_ref as MX
from oracle import streamvln_oracle as O

GUARD, FILL = 64, 777.0
PAD_W = 64
POISON_X = 3.0e4
NAN = float("nan")


def tiles(N, epi):
    """restatement of gemv_mx4b.hip mx4b_tiles"""
    return (N + 15) // 16 if epi == "none" else N // 32 if epi == "swiglu" else (N + 31) // 32


def geometry(N, epi):
    """(waves on K, workgroups, grid-stride passes) of a launch: restates launch_gemv_mx4b / gemv_mx4b_grid"""
    t = tiles(N, epi)
    kw = 4 if epi == "argmax" or t >= 512 else 16
    grid = max(1, min(t, 1024 if epi == "argmax" else 2048))
    return kw, grid, (t + grid - 1) // grid


def _superstep_perm(K128):
    """index k of the weights -> index of x that the `k_perm_w_only` mistake pairs it with"""
    k = torch.arange(K128)
    s, g, j, e = k // 128, (k % 128) // 32, (k % 32) // 8, k % 8
    return 128 * s + 32 * j + 8 * g + e


class Case:
    """one launch of svln_op_gemv_mxfp4_batched: epi "none" | "swiglu" | "argmax"; family "exact" (none, argmax) | "wide-gate" (swiglu)"""

    def __init__(self, B, epi, N, K, bias=False, res=False, seed=0, nan_row=None, pen_row=None):
        self.B, self.epi, self.N, self.K, self.bias_on, self.res_on, self.seed = B, epi, N, K, bias, res, seed
        self.nan_row, self.pen_row = nan_row, pen_row
        self.n_out = N // 2 if epi == "swiglu" else N
        self.exact = epi != "swiglu"
        self.ldw, self.ldx, self.ldr, self.ldy = K + PAD_W, K + 16, N + 8, self.n_out + 24
        self.id = f"mx4b-B{B}-{epi}-N{N}-K{K}" + ("-bias" if bias else "") + ("-res" if res else "")
        self._built = False

    # ------------------------------------------------------------------------------------------------------ construction
    def build(self):
        if self._built:
            return self
        self._built = True
        B, N, K = self.B, self.N, self.K
        g = torch.Generator().manual_seed(9000 + self.seed)
        self.W = G.Weights("mxfp4", N, K, 277 + self.seed)
        self.bias = self.res = None
        self.pen = 1.0
        if self.epi == "argmax":
            self._build_argmax(g)
        else:
            x = torch.randint(-1, 2, (B, K), generator=g).double()
            x[:, 0] = -1.0
            # row 0 of the weights always has a code at K - 1 (the high nibble of the last byte of the last block): the rows of X
            # alternate in sign there and are 0 at K - 2, so that code alone tells a swapped nibble and two exchanged rows of X
            x[:, K - 1] = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).double()
            x[:, K - 2] = 0.0
            for b in range(1, B):                               # every row differs from every other in at least its first block
                x[b, 1 + b] = -x[0, 1 + b] if x[0, 1 + b] != 0 else 1.0
            self.x = x
            if self.bias_on:
                self.bias = torch.randint(-2, 3, (N,), generator=g).double()
            if self.res_on:
                self.res = torch.randint(-3, 4, (B, N), generator=g).double()
            if self.epi == "none":
                self.W.vals[0, :K - 1] = 0.0                    # row 0: that code alone (no second code can cancel it)
                self._make_representable()
        self.W.pack(self.ldw)
        return self

    def _make_representable(self):
        """a row whose outputs are not all bf16 values keeps only its LAST non-zero code (the one planted in the last block of every
        fourth row); one scaled code plus two small integers always is a bf16 value"""
        bad = ~G.representable(self._outputs(self.W.dense()), torch.bfloat16).all(0)
        for n in torch.nonzero(bad).flatten().tolist():
            nz = torch.nonzero(self.W.vals[n]).flatten()
            self.W.vals[n, nz[:-1]] = 0.0
        assert bool(G.representable(self._outputs(self.W.dense()), torch.bfloat16).all()), self.id

    def _build_argmax(self, g):
        """as gemv_ref.BatchedCase: common signs, the first half of K in stripes private to one env (k % 8 == b).  A row against the common
        signs has a logit <= 0 in every env; env b's planted rows are coherent on its private positions (exactly 8 for env b, 0 for
        the others).  The ties of env b sit in the same 16-row group, in the two groups of one tile, in two tiles of one workgroup
        (grid-stride passes) or in two workgroups, by b."""
        B, N, K = self.B, self.N, self.K
        kw, grid, passes = geometry(N, "argmax")
        sig = torch.randint(0, 2, (K,), generator=g).double() * 2 - 1
        k = torch.arange(K)
        mask = torch.stack([torch.where(k < K // 2, (k % 8 == b).double(), (torch.rand((K,), generator=g) < 0.75).double()) for b in range(B)])
        self.x = mask * sig[None]
        self.W.vals = -self.W.vals.abs() * sig[None]
        T = tiles(N, "argmax")
        self.tie_sets = []
        for b in range(B):
            t0 = (T // 3 + 5 * b) % max(T - 1, 1)
            kind = b % 4
            if kind == 0:
                rows = (32 * t0 + 3, 32 * t0 + 9)                               # one 16-row group
            elif kind == 1:
                rows = (32 * t0 + 14, 32 * t0 + 17)                             # the two groups of a tile
            elif kind == 2 and passes > 1:
                t0 = t0 % (T - grid)
                rows = (32 * t0 + 30, 32 * (t0 + grid) + 1)                     # two passes of one workgroup
            else:
                rows = (32 * t0 + 21, N - 1 - b)                                # two workgroups; the last rows of the matrix
            rows = tuple(sorted(set(min(n, N - 1) for n in rows)))
            priv = k[(k < K // 2) & (k % 8 == b)]
            for n in rows:
                self.W.vals[n] = self.W.coherent_row(n, self.x[b], 8.0, priv[torch.randperm(len(priv), generator=g)])
            self.tie_sets.append(rows)
        self.flags = None
        if self.pen_row is not None:
            # the penalty (1.5) on the winner of env pen_row moves its logit 8 below the untouched tie partner, which then wins; the
            # flags of every other env mark only rows with a logit <= 0, which cannot win
            self.pen = 1.5
            self.flags = torch.zeros((B, N), dtype=torch.uint8)
            self.flags[self.pen_row, self.tie_sets[self.pen_row][0]] = 1
            for b in range(B):
                if b != self.pen_row:
                    others = [n for n in range(0, N, 97) if n not in self.tie_sets[b]]
                    self.flags[b, others] = 1
        if self.nan_row is not None:
            self.x[self.nan_row] = NAN

    # ------------------------------------------------------------------------------------------------------ reference
    def _outputs(self, Wd, x=None, up_offset=32):
        """float64 [B][n_out] (arg-max: the logits [B][N])"""
        x = self.x if x is None else x
        acc = x @ Wd.t()
        if self.epi == "swiglu":
            gate, _ = G.swiglu_rows(self.n_out)
            return O.silu(acc[:, gate]) * acc[:, gate + up_offset]
        if self.bias is not None:
            acc = acc + self.bias[None]
        if self.res is not None:
            acc = acc + self.res
        return acc

    def _beyond_K(self):
        """(weights, x) of the whole last super-step as the memory holds them: what follows K in every weight row (its ldw padding, then
        the next row) and in every row of x (its ldx padding, then the next row)"""
        K, K128 = self.K, (self.K + 127) // 128 * 128
        q4, e8 = self.W.ops["q4"], self.W.ops["e8"]
        fq = torch.cat([q4.reshape(-1), torch.full((K128,), 0x77, dtype=torch.uint8)])
        fe = torch.cat([e8.reshape(-1), torch.full((K128,), 140, dtype=torch.uint8)])
        Wq = fq.as_strided((self.N, K128 // 2), (self.ldw // 2, 1)).clone()
        We = fe.as_strided((self.N, K128 // 32), (self.ldw // 32, 1)).clone()
        fx = torch.cat([self.x_image().reshape(-1), torch.full((K128,), POISON_X, dtype=torch.float64)])
        return MX.dequant_mxfp4(Wq, We).double(), fx.as_strided((self.B, K128), (self.ldx, 1)).clone()

    def x_image(self):
        x = torch.full((self.B, self.ldx), POISON_X, dtype=torch.float64)
        x[:, :self.K] = self.x
        return x

    def res_image(self):
        if self.res is None:
            return None
        r = torch.full((self.B, self.ldr), POISON_X, dtype=torch.float64)
        r[:, :self.N] = self.res
        return r

    def mutants(self):
        m = ["nibbles_swapped", "scale_blk+1", "k_perm_w_only", "col_leak"]
        if self.K % 128:
            m += ["drop_partial_superstep", "read_past_K"]
        if self.B >= 2:
            m.append("x_rows_swapped")
        if self.epi == "swiglu":
            m.append("up_16_apart")
        return m

    def reference(self, mutant=None):
        self.build()
        K, K128 = self.K, (self.K + 127) // 128 * 128
        if mutant in ("nibbles_swapped", "scale_blk+1"):
            return self._outputs(self.W.dequant(mutant))
        Wd = self.W.dequant()
        if mutant == "k_perm_w_only":
            Wp, xp = torch.zeros((self.N, K128), dtype=torch.float64), torch.zeros((self.B, K128), dtype=torch.float64)
            Wp[:, :K], xp[:, :K] = Wd, self.x
            return self._outputs(Wp, xp[:, _superstep_perm(K128)])
        if mutant == "drop_partial_superstep":
            keep = (torch.arange(K) < K // 128 * 128).double()
            return self._outputs(Wd * keep[None])
        if mutant == "read_past_K":
            return self._outputs(*self._beyond_K())
        if mutant == "x_rows_swapped":
            perm = list(range(self.B))
            perm[0], perm[1] = 1, 0
            out = self._outputs(Wd, self.x[perm])
            if self.res is not None:                            # (the residual rows stay where they are)
                out = out - self.res[perm] + self.res
            return out
        if mutant == "up_16_apart":
            return self._outputs(Wd, up_offset=16)
        return self._outputs(Wd)

    def image(self, mutant=None, dtype=torch.bfloat16):
        """the y buffer after the launch, as the stored type would hold it: [GUARD + B * ldy + GUARD]"""
        out = self.reference(None if mutant == "col_leak" else mutant)
        img = torch.full((GUARD + self.B * self.ldy + GUARD,), FILL, dtype=torch.float64)
        rows = self.B
        if mutant == "col_leak":                                # columns B .. 15 of the tile (zero activations: bias only) stored too
            pad = torch.zeros((16 - self.B, self.n_out), dtype=torch.float64)
            if self.bias is not None:
                pad = pad + self.bias[None]
            out, rows = torch.cat([out, pad]), 16
        for b in range(rows):
            lo = GUARD + b * self.ldy
            n = max(0, min(self.n_out, img.numel() - lo))
            img[lo:lo + n] = out[b, :n]
        return img.to(dtype)

    def tokens(self, mutant=None):
        """arg-max: the token of every env (lowest index of the maximum after the penalty; -1 for a row without a finite logit)"""
        logits = self.reference()
        if self.flags is not None:
            logits = torch.where(self.flags.bool(), torch.where(logits < 0, logits * self.pen, logits / self.pen), logits)
        toks = []
        for b in range(self.B):
            row = logits[b]
            fin = torch.isfinite(row)
            if not bool(fin.any()):
                toks.append(-1)
                continue
            top = row[fin].max()
            idx = torch.nonzero(row == top).flatten()
            toks.append(int(idx.max() if mutant == "tie_higher" else idx.min()))
        return toks

    def load(self):
        """sum |w x| (+ |bias| + |res|) per output in quanta of 2^-4: below 2^23 every fp32 partial sum is exact in any order"""
        self.build()
        s = torch.nan_to_num(self.x, nan=0.0).abs() @ self.W.dense().abs().t()
        if self.bias is not None:
            s = s + self.bias.abs()[None]
        if self.res is not None:
            s = s + self.res.abs()
        return s / G.QUANTUM["mxfp4"]

    def gate_span(self):
        acc = self.x @ self.W.dense().t()
        gate, _ = G.swiglu_rows(self.n_out)
        return float(acc[:, gate].min()), float(acc[:, gate].max())


def cases():
    out = []
    # exact: K below one super-step, partial last super-steps (96, 160), many super-steps with a partial last one (4128 = 32 * 128 + 32)
    # against N below / at / above one tile and ragged; B walks 1, 2, 3, 5, 8 along the list
    Bs = (1, 2, 3, 5, 8)
    c = 0
    for K in (32, 96, 160, 4128):
        for N in (1, 7, 16, 17, 515):
            out.append(Case(Bs[(3 * c) % 5], "none", N, K, bias=c % 2 == 0, res=c % 3 != 1, seed=c))      # (3 is coprime to 5: each K meets every B)
            c += 1
    out.append(Case(8, "none", 8200, 96, bias=True, res=True, seed=70))               # 513 tiles: the 4-wave form of EPI_NONE
    out.append(Case(8, "none", 3584, 18944, res=True, seed=71))                       # down_proj
    out.append(Case(4, "none", 4608, 3584, bias=True, seed=72))                       # q|k|v
    for I in (96, 1024):
        for B in (3, 8):
            out.append(Case(B, "swiglu", 2 * I, 512, seed=80 + B))
    out.append(Case(5, "swiglu", 2 * 16416, 128, seed=90))                            # 513 tiles: the 4-wave form of EPI_SWIGLU
    out.append(Case(8, "argmax", 5000, 512, seed=100, pen_row=2, nan_row=5))
    out.append(Case(5, "argmax", 40000, 256, seed=101, pen_row=0, nan_row=3))         # 1250 tiles on 1024 workgroups: two passes
    return out


CASES = cases()
