"""CPU case builder and float64 reference of the decode GEMVs (streamvln_amd/csrc/gemv.hip), and "mutant" references (plausible kernel
mistakes) that prove the inputs sharp.  Test infrastructure, modelled on tests/attn_ref.py.

Formats: plain-fp32, plain-bf16 (weights in the engine type), e4m3 (bytes + one fp32 scale per row), mxfp4 (E2M1 codes + one E8M0 byte per
block of 32).  The quantised operands are BUILT, not quantised: the GEMV ops take bytes and scales as arguments, and the quantisers are
pinned byte for byte elsewhere.

The exact family.  Every value is a small dyadic number: plain weights and e4m3 values in {-1, -1/2, 0, 1/2, 1}, MXFP4 weights on the
E2M1 grid, x in {-1, 0, 1}, bias and residual small integers.  The scales are powers of two that change with the index,
    e4m3   scale[n]    = 2^((5 n mod 7) - 3)
    mxfp4  e8[n][blk]  = 127 + ((3 n + 5 blk) mod 7 - 3)
so neighbouring rows and neighbouring blocks never share one.  While sum |w x| of a row stays below 2^23 quanta (the smallest unit a
term can have) every fp32 partial sum is exact in any order: the un-normalised EPI_NONE output and every logit are defined bit for
bit, the expected output is the float64 sum rounded once to the engine type, and the GPU test compares with torch.equal.
    An MXFP4 row that mixed its seven block scales over a dense row would need 10+ significant bits, and bf16 keeps 8: the exact MXFP4
weights are therefore sparse (MX_NZ non-zero codes per row at random positions, the rest code 0), so that >= 90 % of the rows are bf16
values exactly (the condition every exact case is held to).  Over thousands of rows the non-zero codes still visit every chunk position
and every block scale many times; x stays dense.

The toleranced family (float64 reference, util.assert_close): `eps` (|x| ~ 1e-3: mean(x^2) is of the size of eps), `outlier` (a few
channels of |x| ~ 200 among 0.1), both with norm weights spread over 0.05 .. 4 in magnitude with both signs; `wide-gate` (SwiGLU over
exact gate / up sums whose gate spans at least [-12, 12]).

Poison.  With ldw > K the padding of every row holds large finite weights (plain: 2^60, e4m3: byte 0x7E = 448), code byte 0x77 and
scale byte 140 (MXFP4): a kernel that strays into it is far off.
"""
import functools
import math

import torch

import mxfp4_ref as MX
from oracle import streamvln_oracle as O

EPS = 1e-6
FORMATS = ("plain-fp32", "plain-bf16", "e4m3", "mxfp4")
DTYPE = {"plain-fp32": torch.float32, "plain-bf16": torch.bfloat16, "e4m3": torch.bfloat16, "mxfp4": torch.bfloat16}
EPC = {"plain-fp32": 4, "plain-bf16": 8, "e4m3": 16, "mxfp4": 32}               # weights per 16-byte chunk
KS_R = {"plain-fp32": 2, "plain-bf16": 2, "e4m3": 4, "mxfp4": 4}                # K-split kernel: rows per row group
KS_KW_NARROW = {"plain-fp32": 4, "plain-bf16": 4, "e4m3": 4, "mxfp4": 2}        # ... waves on K when K <= 4096 (4 above)
QUANTUM = {"plain-fp32": 0.5, "plain-bf16": 0.5, "e4m3": 0.5, "mxfp4": 2.0 ** -4}   # smallest unit of a term of the fp32 sum
MX_NZ = 2
POISON = 2.0 ** 60
WAVES = 4


def plain_fmt(dtype):
    return "plain-fp32" if dtype == torch.float32 else "plain-bf16"


def swiglu_rows(I):
    """weight rows of gate j and up j (j < I) in the [gate 32 | up 32] packing"""
    j = torch.arange(I)
    gate = (j // 32) * 64 + j % 32
    return gate, gate + 32


def representable(v, dtype):
    """which float64 values are values of the dtype"""
    return v.to(dtype).to(torch.float64) == v


# ---------------------------------------------------------------------------------------------------------- ownership map
def gemv_grid(N):
    """restatement of gemv.hip gemv_grid: workgroups of the wave-per-rows kernel for N weight rows"""
    groups = (N + 3) // 4
    wg = (groups + WAVES - 1) // WAVES
    if wg <= 1280:
        return max(wg, 1)
    if wg > 4 * 1280:
        return 1024
    if groups % WAVES == 0:
        for g in range(1280, 639, -1):
            if wg % g == 0:
                return g
    return 1024


def owner(N, epi, n):
    """(workgroup, wave, iteration) of the wave-per-rows kernel that produces output n of a launch over N weight rows.  A restatement of
    gemv_grid, OUTS (4 outputs per group; 2 with SwiGLU) and the grid-stride loop `n0 = gw * OUTS; n0 += nw * OUTS`.  It only PLACES the
    arg-max ties: if it drifts from the kernel a tie merely lands somewhere less pointed; no assertion becomes wrong."""
    outs = 2 if epi == "swiglu" else 4
    nw = gemv_grid(N) * WAVES
    group = n // outs
    return (group % nw) // WAVES, (group % nw) % WAVES, group // nw


def iterations(N, epi):
    n_out = N // 2 if epi == "swiglu" else N
    return owner(N, epi, n_out - 1)[2] + 1


TIES = ("group", "iterations", "waves", "workgroups", "ragged", "last", "negative")


def tie_rows(V, where, kernel="rows", shift=0):
    """rows that hold the (equal) maximum of an arg-max case over V rows; the lowest must win.  kernel "rows": the wave-per-rows kernel
    (a wave owns groups of 4 rows, 4 waves per workgroup, grid gemv_grid(V)); "batched": gemv_batched_kernel (a workgroup owns units of 4
    rows, grid min(units, 2048): "waves" does not exist there).  "last": a unique maximum at row V - 1; "negative": a unique maximum
    below zero.  shift moves a placement by that many groups (several envs of a batched case, each with rows of its own)."""
    G = (V + 3) // 4
    nw = gemv_grid(V) * WAVES if kernel == "rows" else min(G, 2048)
    if where == "group":
        g = G // 2 + shift
        return (4 * g + 1, 4 * g + 3)
    if where == "iterations":
        assert G > nw, (V, "one iteration per wave")
        g = (G - nw) // 2 + shift
        return (4 * g + 3, 4 * (g + nw))
    if where == "waves":
        assert kernel == "rows"
        wg = min(nw, G) // WAVES // 2
        return (4 * (WAVES * wg) + 2, 4 * (WAVES * wg + 2) + 1)
    if where == "workgroups":
        a, b = (min(nw, G) // 3, min(nw, G) - 1) if kernel == "batched" else (WAVES * (min(nw, G) // WAVES // 3) + 1, WAVES * (min(nw, G) // WAVES - 1) + 3)
        return (4 * (a + shift), 4 * b + 2 - 8 * shift)
    if where == "ragged":
        assert V % 4 >= 2, V
        return (4 * (G - 1), V - 1)
    if where == "last":
        return (V - 1,)
    assert where == "negative", where
    return (4 * (G // 3) + 2,)


# ---------------------------------------------------------------------------------------------------------- chunk ownership along K
def chunk_roles(nch, kw_count, paired):
    """role of every 16-byte chunk position of a row: (wave on K, role), role 0 = first chunk of a paired iteration, 1 = second
    in-flight chunk, 2 = tail loop; an un-paired loop gives role 0 throughout.  Restates dot_accum (c0 = kw * 64, stride 64 * KW) and the
    un-paired loops of gemv_ksplit_kernel / gemv_batched_kernel."""
    wave = torch.zeros(nch, dtype=torch.int64)
    role = torch.zeros(nch, dtype=torch.int64)
    stride = 64 * kw_count
    for kw in range(kw_count):
        for lane in range(64):
            ci = kw * 64 + lane
            if paired:
                while ci + stride < nch:
                    wave[ci], wave[ci + stride] = kw, kw
                    role[ci + stride] = 1
                    ci += 2 * stride
            while ci < nch:
                wave[ci] = kw
                role[ci] = 2 if paired else 0
                ci += stride
    return wave, role


# ---------------------------------------------------------------------------------------------------------- weights
def _e4m3_scale(N):
    return torch.exp2(((5 * torch.arange(N)) % 7 - 3).double())


def _mx_exponent(N, nblk):
    return ((3 * torch.arange(N)[:, None] + 5 * torch.arange(nblk)[None]) % 7 - 3)


@functools.lru_cache(maxsize=4)
def _random_values(fmt, N, K, seed):
    """unscaled values [N][K] float64: {-1 .. 1} in halves, or E2M1 grid values (MX_NZ non-zero per row)"""
    g = torch.Generator().manual_seed(seed)
    if fmt != "mxfp4":
        return torch.randint(-2, 3, (N, K), generator=g).double() / 2
    v = torch.zeros((N, K), dtype=torch.float64)
    pos = torch.randint(0, K, (N, MX_NZ), generator=g)
    last = K - 32 + torch.randint(0, 32, (N,), generator=g)          # every fourth row has a code in the last chunk: a small N sees it too
    last[0] = K - 1                                                  # (x[K - 1] is never zero)
    pos[:, 0] = torch.where(torch.arange(N) % 4 == 0, last, pos[:, 0])
    mag = torch.tensor(MX.GRID, dtype=torch.float64)[torch.randint(1, 8, (N, MX_NZ), generator=g)]
    sgn = torch.randint(0, 2, (N, MX_NZ), generator=g).double() * 2 - 1
    v.scatter_(1, pos, mag * sgn)
    return v


class Weights:
    """one weight matrix [N][K]: unscaled values (editable row by row until pack()), then the device operands with row stride ldw and
    their float64 dequantisation, read back from the packed buffers so that stride mistakes see what the memory holds"""

    def __init__(self, fmt, N, K, seed):
        self.fmt, self.N, self.K = fmt, N, K
        self.vals = _random_values(fmt, N, K, seed).clone()
        self.scale = _e4m3_scale(N) if fmt == "e4m3" else None
        self.exp = _mx_exponent(N, K // 32) if fmt == "mxfp4" else None

    def elem_scale(self):
        """[N][K] (or broadcastable) float64 factor of every unscaled value"""
        if self.fmt == "e4m3":
            return self.scale[:, None]
        if self.fmt == "mxfp4":
            return torch.exp2(self.exp.double()).repeat_interleave(32, 1)
        return torch.ones((1, 1), dtype=torch.float64)

    def dense(self):
        return self.vals * self.elem_scale()

    def pack(self, ldw):
        fmt, N, K = self.fmt, self.N, self.K
        assert ldw >= K and ldw % EPC[fmt] == 0
        self.ldw = ldw
        if fmt.startswith("plain"):
            buf = torch.full((N, ldw), POISON, dtype=torch.float64)
            buf[:, :K] = self.vals
            self.ops = {"W": buf.to(DTYPE[fmt])}
        elif fmt == "e4m3":
            buf = torch.full((N, ldw), 0x7E, dtype=torch.uint8)
            buf[:, :K] = self.vals.float().to(torch.float8_e4m3fn).view(torch.uint8)
            self.ops = {"w8": buf, "scale": self.scale.float()}
        else:
            a = self.vals.abs()
            code = sum((a > m).to(torch.uint8) for m in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)) | ((self.vals < 0).to(torch.uint8) << 3)
            q4 = torch.full((N, ldw // 2), 0x77, dtype=torch.uint8)
            q4[:, :K // 2] = code[:, 0::2] | (code[:, 1::2] << 4)
            e8 = torch.full((N, ldw // 32), 140, dtype=torch.uint8)
            e8[:, :K // 32] = (self.exp + 127).to(torch.uint8)
            self.ops = {"q4": q4, "e8": e8}
        assert torch.equal(self.dequant(), self.dense()), "packed operands do not hold the designed values"
        return self

    @staticmethod
    def _rows(buf, stride, width, shift=0):
        if stride == buf.shape[1] and shift == 0:
            return buf[:, :width]
        flat = buf.reshape(-1)
        flat = torch.cat([flat[:1], flat, flat[-1:]])         # (a shift of one element past either end reads the end element)
        return flat.as_strided((buf.shape[0], width), (stride, 1), 1 + shift).clone()

    def dequant(self, mutant=None, scale_index=None):
        """float64 [N][K] of what a kernel reads.  mutants: ldw_as_K (plain / e4m3 row stride), ldw_as_K_q4, ldw_as_K_e8 (the MXFP4 code /
        scale-byte row strides ldw / 2, ldw / 32), scale_blk+1 / scale_blk-1 (the scale byte of the neighbouring block position in
        memory), nibbles_swapped.  scale_index [N]: the row whose e4m3 scale each row takes (default: its own)."""
        fmt, N, K, ldw = self.fmt, self.N, self.K, self.ldw
        if fmt.startswith("plain"):
            return self._rows(self.ops["W"], K if mutant == "ldw_as_K" else ldw, K).double()
        if fmt == "e4m3":
            v = self._rows(self.ops["w8"], K if mutant == "ldw_as_K" else ldw, K).contiguous().view(torch.float8_e4m3fn).float().double()
            s = self.scale if scale_index is None else self.scale[scale_index]
            return v * s[:, None]
        q4 = self._rows(self.ops["q4"], (K if mutant == "ldw_as_K_q4" else ldw) // 2, K // 2)
        if mutant == "nibbles_swapped":
            q4 = (q4 >> 4) | ((q4 & 0xF) << 4)
        shift = {"scale_blk+1": 1, "scale_blk-1": -1}.get(mutant, 0)
        e8 = self._rows(self.ops["e8"], (K if mutant == "ldw_as_K_e8" else ldw) // 32, K // 32, shift)
        return MX.dequant_mxfp4(q4, e8).double()

    # -------------------------------------------------------------------------------------------------- planted rows (arg-max)
    def coherent_row(self, n, x, T, order):
        """unscaled values of a row whose product with x is exactly T > 0: greedy over the positions `order`, each taking the largest
        value v of the format with v * scale <= what is left, signed like x"""
        row = torch.zeros(self.K, dtype=torch.float64)
        grid = (1.0, 0.5) if self.fmt != "mxfp4" else tuple(reversed(MX.GRID[1:]))
        left = float(T)
        for k in order.tolist():
            if left == 0:
                break
            if x[k] == 0:
                continue
            s = float(self.scale[n]) if self.fmt == "e4m3" else 2.0 ** int(self.exp[n, k // 32]) if self.fmt == "mxfp4" else 1.0
            for v in grid:
                if v * s <= left:
                    row[k] = v * float(x[k])
                    left -= v * s
                    break
        assert left == 0, (self.fmt, n, T, left)
        return row


# ---------------------------------------------------------------------------------------------------------- cases
class Case:
    """One launch of svln_op_gemv / _fp8 / _mxfp4.
    kernel   "rows" | "ksplit" (what launch_gemv_fmt picks for N, epi; asserted)
    epi      "none" | "swiglu" | "argmax";   family "exact" | "eps" | "outlier" | "wide-gate"
    pad      ldw - K;   tie: one of TIES (arg-max)"""

    def __init__(self, fmt, epi, N, K, family="exact", norm=False, bias=False, res=False, pad=0, tie=None, seed=0):
        self.fmt, self.epi, self.N, self.K, self.family, self.norm = fmt, epi, N, K, family, norm
        self.bias_on, self.res_on, self.pad, self.tie, self.seed = bias, res, pad, tie, seed
        self.dtype = DTYPE[fmt]
        self.kernel = "ksplit" if epi == "none" and N <= 8192 else "rows"
        self.n_out = N // 2 if epi == "swiglu" else N
        assert (family in ("eps", "outlier")) == norm and (family == "wide-gate") == (epi == "swiglu" and not norm)
        self.exact = family == "exact" and not norm and epi != "swiglu"
        self.id = f"{fmt}-{self.kernel}-{epi}-N{N}-K{K}-{family}" + ("-norm" if norm else "") + ("-bias" if bias else "") + \
                  ("-res" if res else "") + (f"-pad{pad}" if pad else "") + (f"-tie_{tie}" if tie else "")
        self._built = False

    # geometry of the K loop the case runs
    def k_loop(self):
        if self.kernel == "rows":
            return 1, True
        kw = WAVES if self.K > 4096 else KS_KW_NARROW[self.fmt]
        return kw, self.fmt.startswith("plain") and not self.norm

    def group_rows(self):
        return 4 if self.kernel == "rows" else KS_R[self.fmt]

    def build(self):
        if self._built:
            return self
        self._built = True
        fmt, N, K, dt = self.fmt, self.N, self.K, self.dtype
        g = torch.Generator().manual_seed(1000 + self.seed)
        rt = lambda t: t.to(dt).double()
        if self.family in ("exact", "wide-gate"):
            x = torch.randint(-1, 2, (K,), generator=g).double()
            if K > 8192 and fmt != "mxfp4":
                x = x * (torch.rand((K,), generator=g) < 0.5)               # thinned at the largest K: >= 90 % of the sums stay bf16 values
            x[0], x[K - 1] = -1.0, 1.0
            if self.epi == "argmax":
                x = torch.where(x == 0, torch.ones_like(x), x)              # dense: a planted row may need every position
        elif self.family == "eps":
            x = rt(1e-3 * (0.5 + torch.rand((K,), generator=g).double()) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1))
        else:
            x = 0.1 * (torch.rand((K,), generator=g).double() * 2 - 1)
            hot = torch.tensor([3, K // 2 + 1, K - 2, K - 1 - 5 * EPC[fmt] // 4])
            x[hot] = torch.tensor([200.0, -190.0, 210.0, -205.0], dtype=torch.float64)
            x = rt(x)
        self.x = x
        self.g = None
        if self.norm:
            mag = 0.05 * torch.exp(torch.rand((K,), generator=g).double() * math.log(4 / 0.05))
            self.g = rt(mag * (torch.randint(0, 2, (K,), generator=g) * 2 - 1))
        self.bias = torch.randint(-2, 3, (N,), generator=g).double() if self.bias_on else None
        self.res = torch.randint(-3, 4, (N,), generator=g).double() if self.res_on else None
        self.W = Weights(fmt, N, K, 77 + self.seed)
        self.winner = None
        if self.epi == "argmax":
            self._plant(g)
        self.W.pack(K + self.pad)
        return self

    def _plant(self, g):
        """the arg-max rows: every other row's logit ends below the planted maximum (a row with a positive logit is negated; below a
        negative maximum, rows too close to zero become a fully coherent negative row)"""
        W, x, K = self.W, self.x, self.K
        rows = tie_rows(self.N, self.tie)
        T = -4.0 if self.tie == "negative" else 8.0
        logits = (W.dense() @ x)
        W.vals[logits > 0] *= -1
        logits = -logits.abs()
        if T < 0:
            W.vals[logits >= T] = -x[None]
        for n in rows:
            W.vals[n] = W.coherent_row(n, x, abs(T), torch.randperm(K, generator=g)) * (1 if T > 0 else -1)
        self.tie_set, self.winner, self.top = rows, min(rows), T

    # -------------------------------------------------------------------------------------------------- reference
    def mutants(self):
        fmt, N, K = self.fmt, self.N, self.K
        nch = K // EPC[fmt]
        kw, paired = self.k_loop()
        wave, role = chunk_roles(nch, kw, paired)
        m = []
        if not self.norm:       # shares of K: on exact sums only (under a norm one chunk is 1 / nch of a toleranced sum; the exact cases
                                # run the same loops)
            m.append("drop_last_chunk")
            if paired and bool((role == 2).any()):
                m.append("drop_tail_loop")
            if paired and bool((role == 1).any()):
                m.append("drop_second_inflight")
            if kw > 1 and bool((wave == kw - 1).any()):
                m.append("drop_last_wave_share")
        if fmt == "e4m3":
            m += ["scale_row+1", "scale_row-1"]
            if self.epi == "swiglu":
                m.append("swiglu_scale_unpermuted")
            if self.epi != "swiglu" and N % self.group_rows() >= 2:
                m.append("scale_clamped_row")
        if fmt == "mxfp4":
            m += ["scale_blk+1", "scale_blk-1", "nibbles_swapped"]
        if self.pad:
            m += ["ldw_as_K_q4", "ldw_as_K_e8"] if fmt == "mxfp4" else ["ldw_as_K"]
        if self.norm:       # eps shows where mean(x^2) is of its size -- and there it hides the norm weights' share of the radicand
            m += ["eps_omitted", "eps_outside_root"] if self.family == "eps" else ["rstd_from_gx"]
        if self.epi == "swiglu":
            m.append("gate_up_swapped")
        return m

    def _scale_index(self, mutant):
        n = torch.arange(self.N)
        if mutant == "scale_row+1":
            return (n + 1).clamp(max=self.N - 1)
        if mutant == "scale_row-1":
            return (n - 1).clamp(min=0)
        if mutant == "scale_clamped_row":           # every row of the ragged last group takes the scale of the row the clamp substitutes
            R = self.group_rows()
            return torch.where(n >= (self.N // R) * R, torch.full_like(n, self.N - 1), n)
        if mutant == "swiglu_scale_unpermuted":     # row r of the group of outputs (n0, n0 + 1) takes scale[n0 + r], not scale[rn[r]]
            gate, up = swiglu_rows(self.n_out)
            j = torch.arange(self.n_out)
            idx = n.clone()
            idx[gate] = (j - j % 2) + 2 * (j % 2)
            idx[up] = (j - j % 2) + 2 * (j % 2) + 1
            return idx
        return None

    def accumulate(self, mutant=None):
        """float64 W . x' per weight row (before bias / residual / SwiGLU), under `mutant`"""
        self.build()
        fmt, K = self.fmt, self.K
        Wd = self.W.dequant(mutant, self._scale_index(mutant))
        if mutant and mutant.startswith("drop_"):
            kw, paired = self.k_loop()
            wave, role = chunk_roles(K // EPC[fmt], kw, paired)
            nch = K // EPC[fmt]
            drop = {"drop_last_chunk": torch.arange(nch) == nch - 1, "drop_tail_loop": role == 2, "drop_second_inflight": role == 1,
                    "drop_last_wave_share": wave == kw - 1}[mutant]
            Wd = Wd * (~drop).double().repeat_interleave(EPC[fmt])[None]
        x = self.x
        if not self.norm:
            return Wd @ x
        gx = self.g * x
        ms = (x * x).mean()
        if mutant == "rstd_from_gx":
            ms = (gx * gx).mean()
        rstd = 1 / torch.sqrt(ms) if mutant == "eps_omitted" else 1 / (torch.sqrt(ms) + EPS) if mutant == "eps_outside_root" else 1 / torch.sqrt(ms + EPS)
        return (Wd @ gx) * rstd

    def reference(self, mutant=None):
        """float64 output [n_out] (arg-max: the logits [N])"""
        acc = self.accumulate(mutant)
        if self.epi == "swiglu":
            gate, up = swiglu_rows(self.n_out)
            if mutant == "gate_up_swapped":
                gate, up = up, gate
            return O.silu(acc[gate]) * acc[up]
        if self.bias is not None:
            acc = acc + self.bias
        if self.res is not None:
            acc = acc + self.res
        return acc

    def load(self):
        """sum |w x| (+ |bias| + |res|) per weight row in quanta: below 2^23 every fp32 partial sum is exact"""
        self.build()
        s = self.W.dense().abs() @ self.x.abs()
        for t in (self.bias, self.res):
            if t is not None:
                s = s + t.abs()
        return s / QUANTUM[self.fmt]

    def gate_span(self):
        acc = self.accumulate()
        gate, _ = swiglu_rows(self.n_out)
        return float(acc[gate].min()), float(acc[gate].max())


def bound(exp, dtype):
    """the per-element bound util.assert_close applies to an expected output"""
    from util import tol
    rt, at = tol(dtype)
    exp = exp.float().double()
    return at * max(1.0, float(exp.abs().max())) + rt * exp.abs()


def mutant_report(case):
    """{mutant: rows whose stored bits change} (exact cases) or {mutant: max |mutant - reference| / bound} (toleranced cases)"""
    ref = case.reference()
    out = {}
    for m in case.mutants():
        mut = case.reference(m)
        if case.exact:
            stored = torch.float32 if case.epi == "argmax" else case.dtype          # logits are compared in fp32, never stored
            out[m] = int((mut.to(stored) != ref.to(stored)).sum())
        else:
            out[m] = float(((mut - ref).abs() / bound(ref, case.dtype)).max())
    return out


# ---------------------------------------------------------------------------------------------------------- the case lists
def k_ladder(fmt):
    """K by chunks per row nch = K / EPC: some lanes idle (24); 64; some lanes paired, the rest tail-only (112: MXFP4's true K); paired
    plus tail for every lane (192); the true 3584"""
    return sorted({n * EPC[fmt] for n in (24, 64, 112, 192)} | {3584})


def cases():
    out = []
    for f, fmt in enumerate(FORMATS):
        ks = k_ladder(fmt)
        # rows kernel, EPI_NONE (N > 8192), ragged against the 4-row group
        for i, (K, N) in enumerate(zip(ks, (8193, 8999, 9001, 8202, 8195))):
            out.append(Case(fmt, "none", N, K, bias=i % 2 == 0, res=i % 3 == 0, seed=i))
        out.append(Case(fmt, "none", 8197, ks[1], pad=64, bias=True, seed=6))
        out.append(Case(fmt, "none", 8194, ks[2], family="eps", norm=True, seed=7))
        out.append(Case(fmt, "none", 8201, 3584, family="outlier", norm=True, res=True, pad=64, seed=8))
        # rows kernel, SwiGLU
        for i, (K, I) in enumerate(zip(ks, (1056, 544, 1024, 288, 1120))):
            out.append(Case(fmt, "swiglu", 2 * I, K, family="wide-gate", seed=10 + i))
        out.append(Case(fmt, "swiglu", 2 * 544, ks[2], family="wide-gate", pad=64, seed=16))
        out.append(Case(fmt, "swiglu", 2 * 1056, ks[3], family="eps", norm=True, seed=17))
        out.append(Case(fmt, "swiglu", 2 * 544, 3584, family="outlier", norm=True, pad=64, seed=18))
        # rows kernel, arg-max: one placement per case, K walks the ladder
        for i, (tie, V) in enumerate((("group", 5001), ("waves", 5000), ("workgroups", 5003), ("ragged", 5002), ("last", 5001), ("negative", 5003))):
            out.append(Case(fmt, "argmax", V, ks[i % len(ks)], tie=tie, pad=64 if tie == "waves" else 0, seed=20 + i))
        # K-split kernel, narrow and wide, ragged against KS_R x row groups
        for i, (K, N) in enumerate(zip(ks + [18944], (515, 7, 257, 130, 513, 515))):
            out.append(Case(fmt, "none", N, K, bias=i % 2 == 1, res=i % 3 != 1, seed=30 + i))
        out.append(Case(fmt, "none", 514, ks[2], pad=64, res=True, seed=37))
        out.append(Case(fmt, "none", 259, 18944, pad=64, bias=True, seed=38))
        out.append(Case(fmt, "none", 515, ks[0], family="eps", norm=True, seed=39))
        out.append(Case(fmt, "none", 258, 3584, family="outlier", norm=True, bias=True, pad=64, seed=40))
        out.append(Case(fmt, "none", 131, 18944, family="eps", norm=True, res=True, seed=41))
        out.append(Case(fmt, "none", 35, 18944, family="outlier", norm=True, pad=64, seed=42))
        # grid-stride regimes of gemv_grid at the smallest K
        K = 128 if fmt == "mxfp4" else 64
        out.append(Case(fmt, "swiglu", 37888, K, family="wide-gate", seed=50))              # divisor search: 1184 workgroups x 2 iterations
        out.append(Case(fmt, "none", 37891, K, bias=True, seed=51))                         # no divisor (ragged): 1024 workgroups x 3
        for i, (V, tie) in enumerate(((152064, "iterations"), (152064, "last"), (152063, "ragged"), (152063, "negative"))):
            out.append(Case(fmt, "argmax", V, K, tie=tie, seed=52 + i))                     # the 1024-workgroup cap
    return out


CASES = cases()


# ---------------------------------------------------------------------------------------------------------- batched kernel
class BatchedCase:
    """gemv_batched_kernel (plain weights, B environments): the exact family with a different x per env, row strides ldx > K, ldy > n_out,
    ldr > N, ragged N; SwiGLU wide-gate; a per-env arg-max whose exact tie sits in a different place for each env."""
    BTIES = (("group", 0), ("workgroups", 0), ("iterations", 0), ("last", 0), ("group", 5), ("workgroups", 7), ("iterations", 9), ("group", 11))

    def __init__(self, dtype, B, epi, N, K, family="exact", norm=False, seed=0):
        self.dtype, self.B, self.epi, self.N, self.K, self.family, self.norm, self.seed = dtype, B, epi, N, K, family, norm, seed
        self.fmt = plain_fmt(dtype)
        self.n_out = N // 2 if epi == "swiglu" else N
        self.exact = family == "exact" and not norm and epi != "swiglu"
        self.id = f"{self.fmt}-batched-B{B}-{epi}-N{N}-K{K}-{family}" + ("-norm" if norm else "")
        self._built = False

    def build(self):
        if self._built:
            return self
        self._built = True
        B, N, K, dt = self.B, self.N, self.K, self.dtype
        g = torch.Generator().manual_seed(5000 + self.seed)
        rt = lambda t: t.to(dt).double()
        self.W = Weights(self.fmt, N, K, 177 + self.seed)
        self.g = self.bias = self.res = None
        if self.epi == "argmax":
            # every env shares the signs of x and differs in which positions are non-zero: the first half of K in stripes private to one
            # env (k % 8 == b), the second half at random.  A row against the common signs has a logit <= 0 in every env; env b's
            # planted rows are 8 coherent ones on its private positions: the logit 8 for env b, 0 for every other env.
            sig = torch.randint(0, 2, (K,), generator=g).double() * 2 - 1
            k = torch.arange(K)
            mask = torch.stack([torch.where(k < K // 2, (k % 8 == b).double(), (torch.rand((K,), generator=g) < 0.75).double()) for b in range(B)])
            self.x = mask * sig[None]
            self.W.vals = -self.W.vals.abs() * sig[None]
            self.tie_sets = []
            for b in range(B):
                rows = tie_rows(N, self.BTIES[b][0], "batched", self.BTIES[b][1])
                priv = k[(k < K // 2) & (k % 8 == b)]
                for n in rows:
                    self.W.vals[n] = 0
                    self.W.vals[n, priv[torch.randperm(len(priv), generator=g)[:8]]] = 1.0
                    self.W.vals[n] *= sig
                self.tie_sets.append(rows)
            if self.norm:       # positive powers of two (1 on the private stripes): every sign and every planted sum stays as it is, and
                                # rstd > 0 differs per env but scales that env's logits alike
                self.g = torch.where(k < K // 2, torch.ones(K, dtype=torch.float64), torch.exp2(torch.randint(-1, 2, (K,), generator=g).double()))
        elif self.family in ("exact", "wide-gate"):
            self.x = torch.randint(-1, 2, (B, K), generator=g).double()
            self.x[:, 0], self.x[:, K - 1] = -1.0, 1.0
            if self.family == "exact":
                self.bias = torch.randint(-2, 3, (N,), generator=g).double()
                self.res = torch.randint(-3, 4, (B, N), generator=g).double()
        else:
            x = 0.1 * (torch.rand((B, K), generator=g).double() * 2 - 1)
            x[:, [3, K - 2]] = torch.tensor([200.0, -210.0], dtype=torch.float64)
            if self.family == "eps":
                x = 1e-3 * (0.5 + torch.rand((B, K), generator=g).double()) * (torch.randint(0, 2, (B, K), generator=g) * 2 - 1)
            self.x = rt(x)
            mag = 0.05 * torch.exp(torch.rand((K,), generator=g).double() * math.log(4 / 0.05))
            self.g = rt(mag * (torch.randint(0, 2, (K,), generator=g) * 2 - 1))
        self.W.pack(K + 64)
        return self

    def mutants(self):
        wave, _ = chunk_roles(self.K // EPC[self.fmt], WAVES, False)
        m = ["ldw_as_K"]
        if not self.norm:
            m += ["drop_last_chunk"] + (["drop_last_wave_share"] if bool((wave == WAVES - 1).any()) else [])
        else:
            m += ["eps_omitted", "eps_outside_root"] if self.family == "eps" else ["rstd_from_gx"]
        if self.epi == "swiglu":
            m.append("gate_up_swapped")
        return m

    def reference(self, mutant=None):
        """float64 [B][n_out] (arg-max: the logits [B][N])"""
        self.build()
        fmt, K = self.fmt, self.K
        Wd = self.W.dequant(mutant)
        if mutant and mutant.startswith("drop_"):
            nch = K // EPC[fmt]
            wave, _ = chunk_roles(nch, WAVES, False)
            drop = torch.arange(nch) == nch - 1 if mutant == "drop_last_chunk" else wave == WAVES - 1
            Wd = Wd * (~drop).double().repeat_interleave(EPC[fmt])[None]
        x = self.x
        if self.g is not None:
            gx = self.g[None] * x
            ms = ((gx * gx) if mutant == "rstd_from_gx" else (x * x)).mean(1, keepdim=True)
            rstd = 1 / torch.sqrt(ms) if mutant == "eps_omitted" else 1 / (torch.sqrt(ms) + EPS) if mutant == "eps_outside_root" else 1 / torch.sqrt(ms + EPS)
            acc = (gx @ Wd.t()) * rstd
        else:
            acc = x @ Wd.t()
        if self.epi == "swiglu":
            gate, up = swiglu_rows(self.n_out)
            if mutant == "gate_up_swapped":
                gate, up = up, gate
            return O.silu(acc[:, gate]) * acc[:, up]
        if self.bias is not None:
            acc = acc + self.bias[None] + self.res
        return acc

    def load(self):
        self.build()
        s = self.x.abs() @ self.W.dense().abs().t()
        if self.bias is not None:
            s = s + self.bias.abs()[None] + self.res.abs()
        return s / QUANTUM[self.fmt]

    def gate_span(self):
        acc = self.x @ self.W.dense().t()
        gate, _ = swiglu_rows(self.n_out)
        return float(acc[:, gate].min()), float(acc[:, gate].max())


def batched_cases():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        epc = EPC[plain_fmt(dtype)]
        for i, B in enumerate((1, 2, 4, 8)):
            # chunks per row against the 256 chunk positions of one pass of the four waves: below, across, and the true width
            K = (40 * epc, 3584, 300 * epc, 200 * epc)[i]
            out.append(BatchedCase(dtype, B, "none", 1031 + i, K, seed=i))
            out.append(BatchedCase(dtype, B, "none", 517 + i, K, family=("eps", "outlier")[i % 2], norm=True, seed=10 + i))
            out.append(BatchedCase(dtype, B, "swiglu", 2 * 544, K, family="wide-gate", seed=20 + i))
            out.append(BatchedCase(dtype, B, "argmax", 9001 + i, 256, seed=30 + i))                       # un-normed: argmax_rows
            out.append(BatchedCase(dtype, B, "argmax", 8999 - i, 256, norm=True, seed=40 + i))            # normed: gemv_batched_kernel
    return out


BATCHED_CASES = batched_cases()
