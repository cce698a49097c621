"""CPU case builder, float64 reference and "mutant" references (plausible kernel mistakes) of the persistent decode layer
(streamvln_amd/csrc/decode_layer.hip), plus a restatement of how the kernel deals weight blocks to its waves.  Test infrastructure,
modelled on tests/gemv_ref.py.

One launch = merge of the split-KV partials (edge 0), o_proj + residual (edge 1, x1), RMSNorm + gate/up + SwiGLU (edge 2), down_proj +
residual (edge 3 and x, x2), the next layer's RMSNorm + q|k|v (+ bias) (qkv_out).  The reference returns every stage separately and
computes each from a GIVEN previous stage, so that the GPU test can feed it the kernel's own previous edge: errors do not compound.
Rounding points are the kernel's: every stored value is rounded once to T; the merge output is rounded to T before o_proj; RMSNorm is
rstd * (W . (g * x)).

The exact family.  Partials with integer m (log2 domain), dyadic l whose weighted sum is a power of two, outputs in halves; o_proj and
down_proj are selection rows (at most one non-zero, a power of two, per row; the hot columns walk over every 1 KiB block position of a
row); x small integers.  Then the merged output, x1, and x2 GIVEN the kernel's edge 2 are defined bit for bit and are compared with
torch.equal: the merged output and x1 are exact fp32 values before the one rounding to T; x2 = (power of two) * h + x1 over arbitrary T
values h, x1 is one exact product and ONE fp32 add -- for fp32 that add is the rounding to T; for bf16 the fp32 sum of two bf16 values is
inexact only when one is below 2^-16 of the other, where both roundings return the larger.  Gate/up and q|k|v are dense in both families and
always toleranced.
The toleranced family: dense weights ~ N(0, 1/K); norm weights 0.05 .. 4 in magnitude with both signs; `eps` (|x| ~ 1e-3: mean(x^2)
is of the size of eps) and `outlier` (a few channels of |x| ~ 200 among 0.1) activations, gemv_ref's families.  Compared per stage with
gemv_ref.bound.

Poison.  Partials of splits at or past the live count, rows of q heads that do not exist and the pad columns hold NaN; one live split
of one head is fully masked, (m, l) = (-inf, 0) (with one live split that head has nothing left: the all-masked guard); weight rows
outside the matrix proper hold 2^60 (the GPU test adds them); granule buffers start with NaN payloads under the previous epoch's tags
(odd seeds) or zero tags (even seeds).
"""
import math

import numpy as np
import torch

import gemv_ref as GR
from oracle import streamvln_oracle as O

EPS = 1e-6
BLK, NW, PF, ROWMODE_MAX_BPR = 1024, 8, 16, 15
POISON = 2.0 ** 60
PART_LD = 132                      # 128 outputs, m, l, 2 pad
ES = {torch.bfloat16: 2, torch.float32: 4}
DT_CODE = {torch.bfloat16: 0, torch.float32: 1}


# ------------------------------------------------------------------------------------------------- the dealing, restated
def swiglu_gate_row(j):
    return (j >> 5) * 64 + (j & 31)


def op_row(first, pair, j):
    """matrix row of stream row j"""
    return first + j if not pair else swiglu_gate_row(first + (j >> 1)) + (j & 1) * 32


def dealt(bpr, nrows, w):
    """[(stream row, block of the row)] wave w computes, in order: whole rows w, w + 8, ... when a row has at most 15 blocks; otherwise
    blocks w, w + 8, ... of the share's nrows * bpr blocks taken as one contiguous run"""
    if bpr <= ROWMODE_MAX_BPR:
        r = np.arange(w, nrows, NW)
        return list(zip(np.repeat(r, bpr).tolist(), np.tile(np.arange(bpr), len(r)).tolist()))
    gb = np.arange(w, nrows * bpr, NW)
    return list(zip((gb // bpr).tolist(), (gb % bpr).tolist()))


def slots(n_dealt):
    """slots of a wave that is dealt n_dealt blocks: whole groups of PF, at least one"""
    return max(PF, -(-n_dealt // PF) * PF)


def matrix_rows(nrows, pair, first):
    """rows of the smallest matrix that holds the share [first, first + nrows) -- the share of the LAST workgroup, the tightest bound.
    pair: outputs first .. first + nrows / 2 of a [gate 32 | up 32] packing, which comes in whole 64-row blocks.  A share without rows
    still loads (every wave walks at least one group of padding slots, which re-read the row at `first`): one row is granted; the
    kernel never walks such an op."""
    if pair:
        return 2 * (-(-(first + max(nrows // 2, 1)) // 32) * 32)
    return first + max(nrows, 1)


# ------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, dtype, H, I, nq, nkv, G, family, has_next=True, bias=True, kv_len=100, nsplit=4, tps=1, seed=0, promises=None):
        self.name, self.dtype, self.H, self.I, self.nq, self.nkv, self.G, self.family = name, dtype, H, I, nq, nkv, G, family
        self.has_next, self.bias_on, self.kv_len, self.nsplit, self.tps, self.seed = has_next, bias and has_next, kv_len, nsplit, tps, seed
        self.qd, self.qkv_dim, self.Gq = nq * 128, (nq + 2 * nkv) * 128, nq // nkv
        self.exact = family == "exact"
        self.stale = seed % 2 == 1
        self.seq0 = 7 if self.stale else 0
        self.promises = promises or {}
        self.live = min(nsplit, 64, -(-((kv_len + 63) // 64) // tps))
        self.masked_head = (seed + 1) % nq
        self.masked_split = (seed // 2) % self.live
        self.id = f"{name}-{'bf16' if dtype == torch.bfloat16 else 'fp32'}-{family}-kv{kv_len}" + ("" if has_next else "-last") + \
                  ("" if self.bias_on or not has_next else "-nobias") + ("-stale" if self.stale else "-zerotags")
        self._built = False

    # geometry
    def per(self):
        G = self.G
        return {"A": self.qd // G, "H": self.H // G, "I": self.I // G, "Q": self.qkv_dim // G if self.has_next else 0}

    def ops(self):
        """{product: (K, stream rows per workgroup, pair)}"""
        p = self.per()
        d = {"o": (self.qd, p["H"], 0), "gu": (self.H, 2 * p["I"], 1), "down": (self.I, p["H"], 0)}
        if self.has_next:
            d["qkv"] = (self.H, p["Q"], 0)
        return d

    def bpr(self, K):
        return K * ES[self.dtype] // BLK

    def vpg(self):
        return 2 if self.dtype == torch.bfloat16 else 1

    def rt(self, t):
        return t.to(self.dtype).double()

    def build(self):
        if self._built:
            return self
        self._built = True
        H, I, qd, dt = self.H, self.I, self.qd, self.dtype
        g = torch.Generator().manual_seed(9000 + self.seed)
        rt = self.rt
        randn = lambda *s: torch.randn(s, generator=g, dtype=torch.float32).double()
        # ---- partials [nsplit][nkv][32][132]
        part = torch.full((self.nsplit, self.nkv, 32, PART_LD), float("nan"), dtype=torch.float64)
        L = self.live
        for hq in range(self.nq):
            kh, rho = divmod(hq, self.Gq)
            if self.exact:
                m = torch.randint(-2, 1, (L,), generator=g).double() + float(torch.randint(-3, 4, (1,), generator=g))
                o = torch.randint(-2, 3, (L, 128), generator=g).double() / 2
                l = torch.exp2(torch.randint(0, 3, (L,), generator=g).double())
            else:
                m = (torch.rand((L,), generator=g).double() * 8 - 4).float().double()
                l = (0.5 + 63.5 * torch.rand((L,), generator=g).double()).float().double()
                o = (randn(L, 128) * l[:, None] * (1e-3 if self.family == "eps" else 1.0)).float().double()
            if hq == self.masked_head:
                m[self.masked_split], l[self.masked_split], o[self.masked_split] = -math.inf, 0.0, 7.0
            if self.exact and bool((m > -math.inf).any()):
                top = int(torch.argmax(m))                       # its weight is 1: its l makes the weighted sum of l a power of two
                w = torch.where(m == -math.inf, torch.zeros_like(m), torch.exp2(m - m[top]))
                rest = float((w * l).sum() - l[top])
                l[top] = 2.0 ** math.ceil(math.log2(2 * rest + 1)) - rest
            part[:L, kh, rho, :128], part[:L, kh, rho, 128], part[:L, kh, rho, 129] = o, m, l
        self.part = part
        # ---- activations and norms
        if self.exact:
            x = torch.randint(-3, 4, (H,), generator=g).double()
        elif self.family == "eps":
            x = 1e-3 * (0.5 + torch.rand((H,), generator=g).double()) * (torch.randint(0, 2, (H,), generator=g) * 2 - 1)
        else:
            x = 0.1 * (torch.rand((H,), generator=g).double() * 2 - 1)
            x[torch.tensor([3, H // 2 + 1, H - 2, H - 7])] = torch.tensor([200.0, -190.0, 210.0, -205.0], dtype=torch.float64)
        self.x = rt(x)
        norm_w = lambda: rt(0.05 * torch.exp(torch.rand((H,), generator=g).double() * math.log(4 / 0.05)) * (torch.randint(0, 2, (H,), generator=g) * 2 - 1))
        self.post_norm, self.next_norm = norm_w(), norm_w()
        # ---- weights
        dense = lambda N, K: rt(randn(N, K) * K ** -0.5)
        self.o_w = self._selection(H, qd) if self.exact else dense(H, qd)
        self.down_w = self._selection(H, I) if self.exact else dense(H, I)
        gate, up = GR.swiglu_rows(I)
        self.gu_w = torch.empty((2 * I, H), dtype=torch.float64)
        self.gu_w[gate], self.gu_w[up] = dense(I, H), dense(I, H)
        self.qkv_w = dense(self.qkv_dim, H)
        self.qkv_b = rt(randn(self.qkv_dim)) if self.bias_on else None
        return self

    def _selection(self, N, K):
        """selection rows: row n has one power of two at a column of 1 KiB block n mod bpr (every 11th row has none)"""
        bs = BLK // ES[self.dtype]
        n = torch.arange(N)
        col = (n % (K // bs)) * bs + (n * 37 + 11) % bs
        val = torch.tensor([1.0, -1.0, 2.0, -0.5], dtype=torch.float64)[n % 4] * (n % 11 != 5)
        W = torch.zeros((N, K), dtype=torch.float64)
        W[n, col] = val
        return W

    # ---------------------------------------------------------------------------------------------- granules
    def granule_prefill(self, e):
        """int64 [n_e / VPG] initial granules of edge e: NaN payloads, the previous epoch's tag or tag 0"""
        n = (self.qd, self.H, self.I, self.H)[e] // self.vpg()
        tag = (self.seq0 - 1) * 4 + e + 1 if self.stale else 0
        payload = 0x7FC07FC0 if self.dtype == torch.bfloat16 else 0x7FC00000
        return torch.full((n,), (tag << 32) | payload, dtype=torch.int64)

    def unpack(self, gran):
        """(tags int64 [n / VPG], values float64 [n]) of raw granules"""
        tags, pay = gran >> 32 & 0xFFFFFFFF, gran & 0xFFFFFFFF
        if self.dtype == torch.float32:
            return tags, _bits_to_f32(pay).double()
        lo, hi = pay & 0xFFFF, pay >> 16
        v = torch.stack([_bits_to_f32(lo << 16), _bits_to_f32(hi << 16)], 1).reshape(-1)
        return tags, v.double()

    # ---------------------------------------------------------------------------------------------- reference stages
    def merge(self, mutant=None):
        """edge 0: float64 [qd], rounded to T"""
        self.build()
        part, L = self.part, self.live
        if mutant == "merge_split+1":
            L += 1
        if mutant == "merge_split-1":
            L -= 1

        def head(hq):
            kh, rho = divmod(hq, self.Gq)
            rows = part[:L, kh, rho]
            m, l, o = rows[:, 128], rows[:, 129], rows[:, :128]
            ms = m.max() if L else torch.tensor(-math.inf, dtype=torch.float64)
            w = torch.exp2(m - ms)                                                   # NaN where both are -inf
            if mutant != "merge_no_inf_guard":
                w = torch.where(m == -math.inf, torch.zeros_like(w), w)
            s = (w * l).sum()
            inv = 1.0 / s if s > 0 else torch.zeros((), dtype=torch.float64)         # (NaN > 0 is false)
            return w, o, inv

        out = torch.empty(self.qd, dtype=torch.float64)
        perA = self.per()["A"]
        for hq in range(self.nq):
            w, o, inv = head(hq)
            out[hq * 128:(hq + 1) * 128] = (w[:, None] * o).sum(0) * inv if len(w) else 0.0
        if mutant == "merge_head_mix":              # a workgroup whose slice straddles two heads treats all of it as the first head's
            for c in range(self.G):
                n0 = c * perA
                hqA, hqB = n0 >> 7, (n0 + perA - 1) >> 7
                if hqA != hqB:
                    w, o, inv = head(hqA)
                    d = torch.arange(hqB * 128, n0 + perA) & 127
                    out[hqB * 128:n0 + perA] = (w[:, None] * o[:, d]).sum(0) * inv
        return self.rt(out)

    def _block_partials(self, W, x, shift=0):
        """[N][bpr]: the dot product of every 1 KiB block of every row with its block of x (block b + shift with the off-by-one mutant)"""
        bs = BLK // ES[self.dtype]
        N, K = W.shape
        xb = x.view(K // bs, bs)
        if shift:
            xb = xb.roll(-shift, 0)
        return (W.view(N, K // bs, bs) * xb[None]).sum(2)

    def _product(self, W, x, mutant):
        """float64 W . x per output row of o_proj / down_proj under a dealing mutant"""
        N, K = W.shape
        bpr, per = self.bpr(K), N // self.G
        if mutant is None:
            return W @ x
        P = self._block_partials(W, x, 1 if mutant == "block_off_by_one" else 0)
        if mutant == "block_off_by_one":
            return P.sum(1)
        out = P.sum(1)
        for c in range(self.G):
            r0 = c * per
            if mutant == "drop_last_block":                    # every wave loses its last block of every row it has a part of
                for w in range(NW):
                    d = dealt(bpr, per, w)
                    for i, (r, b) in enumerate(d):
                        if i + 1 == len(d) or d[i + 1][0] != r:
                            out[r0 + r] -= P[r0 + r, b]
            elif mutant == "padding_added":                    # a padding slot (it re-read the share's first block) lands in the last row
                out[r0 + per - 1] += P[r0, 0]
            elif mutant == "partials_swapped":                 # part[r][w] and part[r + 1][w] exchanged for one wave w
                if per < 2:
                    continue
                if bpr > ROWMODE_MAX_BPR:                      # block mode: one wave's partials of the share's rows 0 and 1 (the wave that
                    w = (r0 % bpr) % NW                        # has row 0's hot block, where the row is a selection row)
                    pw = [sum(P[r0 + r, b] for (r, b) in dealt(bpr, per, w) if r == rr) for rr in (0, 1)]
                else:                                          # row mode: a row has one partial
                    pw = [out[r0].clone(), out[r0 + 1].clone()]
                out[r0] += pw[1] - pw[0]
                out[r0 + 1] += pw[0] - pw[1]
        return out

    def x1(self, attn, mutant=None):
        """edge 1 from a given edge 0: float64 [H], rounded to T"""
        self.build()
        acc = self._product(self.o_w, attn, mutant if mutant in ROW_MUTANTS else None)
        return self.rt(acc if mutant == "no_residual_o" else acc + self.x)

    def rstd(self, x):
        return 1 / torch.sqrt((x * x).mean() + EPS)

    def swiglu(self, x1, mutant=None):
        """edge 2 from a given edge 1: float64 [I], rounded to T"""
        self.build()
        gx = x1 if mutant == "g_not_folded" else self.post_norm * x1
        acc = (self.gu_w @ gx) * self.rstd(x1)
        gate, up = GR.swiglu_rows(self.I)
        if mutant == "gate_up_swapped":
            gate, up = up, gate
        if mutant == "op_row_no_pair":              # stream row j of workgroup c read at matrix row c * perI + j
            pI = self.per()["I"]
            j = torch.arange(self.I)
            gate = (j // pI) * pI + 2 * (j % pI)
            up = gate + 1
        return self.rt(O.silu(acc[gate]) * acc[up])

    def x2(self, h, x1, mutant=None):
        """edge 3 (and x) from given edges 2 and 1: float64 [H], rounded to T"""
        self.build()
        acc = self._product(self.down_w, h, mutant if mutant in ROW_MUTANTS else None)
        return self.rt(acc if mutant == "no_residual_down" else acc + x1)

    def qkv(self, x2, x1=None, mutant=None):
        """qkv_out from a given edge 3: float64 [qkv_dim], rounded to T"""
        self.build()
        rstd = self.rstd(x1) if mutant == "rstd1_at_edge3" else self.rstd(x2)
        acc = (self.qkv_w @ (self.next_norm * x2)) * rstd
        if self.qkv_b is not None and mutant != "bias_missing":
            acc = acc + self.qkv_b
        return self.rt(acc)

    def without_wg1(self, v, e):
        """edge e with workgroup 1's granules never arriving: what the buffer held before the launch (NaN payloads)"""
        n = len(v) // self.G
        v = v.clone()
        v[n:2 * n] = float("nan")
        return v

    def reference(self):
        """every stage from the previous REFERENCE stage"""
        a = self.merge()
        x1 = self.x1(a)
        h = self.swiglu(x1)
        x2 = self.x2(h, x1)
        return {"attn": a, "x1": x1, "h": h, "x2": x2, "qkv": self.qkv(x2) if self.has_next else None}

    # ---------------------------------------------------------------------------------------------- mutants
    def mutants(self):
        """{mutant: stage it shows at}: the mistakes this case is built to catch.  Shares of K (a dropped / shifted / added block, a
        swapped partial) on exact sums only: under dense weights one block is 1 / bpr of a toleranced sum; the exact cases run the same
        loops."""
        m = {"gate_up_swapped": "h", "op_row_no_pair": "h", "g_not_folded": "h", "stale_granule": "x1"}
        if self.exact:                              # (under random m the last live split may weigh next to nothing)
            m["merge_split-1"] = "attn"
        if self.family != "eps":                    # (a residual of 1e-3 is below the absolute term of the bound)
            m.update({"no_residual_o": "x1", "no_residual_down": "x2"})
        if self.live < self.nsplit:
            m["merge_split+1"] = "attn"
        if self.live == 1:
            m["merge_no_inf_guard"] = "attn"
        perA = self.per()["A"]
        if any((c * perA) >> 7 != (c * perA + perA - 1) >> 7 for c in range(self.G)):
            m["merge_head_mix"] = "attn"
        if self.exact:
            m.update({"drop_last_block": "x2", "padding_added": "x2"})
            if self.per()["H"] >= 2:
                m["partials_swapped"] = "x2"
            if self.bpr(self.I) > ROWMODE_MAX_BPR:
                m["block_off_by_one"] = "x2"
        if self.has_next:
            if self.bias_on:
                m["bias_missing"] = "qkv"
            if self.family == "eps":
                m["rstd1_at_edge3"] = "qkv"
        return m

    def exact_stage(self, stage):
        return self.exact and stage in ("attn", "x1", "x2")

    def mutant_stage(self, mutant, ref):
        """the stage `mutant` shows at, computed like the reference from the reference's previous stages"""
        st = self.mutants()[mutant]
        if st == "attn":
            return self.merge(mutant)
        if mutant == "stale_granule":
            return self.x1(self.without_wg1(ref["attn"], 0))
        if st == "x1":
            return self.x1(ref["attn"], mutant)
        if st == "h":
            return self.swiglu(ref["x1"], mutant)
        if st == "x2":
            return self.x2(ref["h"], ref["x1"], mutant)
        return self.qkv(ref["x2"], ref["x1"], mutant)


ROW_MUTANTS = ("drop_last_block", "block_off_by_one", "padding_added", "partials_swapped")
ALL_MUTANTS = ROW_MUTANTS + ("gate_up_swapped", "op_row_no_pair", "no_residual_o", "no_residual_down", "rstd1_at_edge3", "g_not_folded",
                             "bias_missing", "merge_no_inf_guard", "merge_split+1", "merge_split-1", "merge_head_mix", "stale_granule")


def _bits_to_f32(u):
    """int64 holding 32-bit patterns -> float32"""
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32)


def deviation(case, stage, got, exp):
    """how far `got` is from `exp` at a stage: exact stages -> number of values that differ (NaN differs); toleranced -> max |err| / bound
    (inf where got is not finite)"""
    if case.exact_stage(stage):
        return int((~(got == exp)).sum())
    err = (got - exp).abs() / GR.bound(exp, case.dtype)
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    return float(err.max())


def mutant_report(case):
    ref = case.reference()
    return {m: deviation(case, st, case.mutant_stage(m, ref), ref[st]) for m, st in case.mutants().items()}


# ------------------------------------------------------------------------------------------------- the case list
def cases():
    bf, f32 = torch.bfloat16, torch.float32
    out = []
    seed = [0]

    def add(name, dt, H, I, nq, nkv, G, fams=("exact", None), **kw):
        for fam in fams:
            seed[0] += 1
            fam = fam or ("eps", "outlier")[seed[0] // 2 % 2]
            out.append(Case(name, dt, H, I, nq, nkv, G, fam, seed=seed[0], **kw))

    for dt in (bf, f32):
        # 1: the engine's TINY launch: 2 to 4 rows per workgroup, waves without work
        add("tiny256", dt, 512, 1024, 4, 2, 256, promises={"idle_waves": True})
        # 2: the per-workgroup caps exactly; two (bf16) / four (fp32) slot groups per wave in gate / up
        add("caps", dt, 512, 1024, 4, 2, 8, promises={"per": {"A": 64, "H": 64, "I": 128, "Q": 128}, "slots": {"gu": [32 * ES[dt] // 2] * 8}})
    # 3: the row / block mode boundary of down_proj
    add("rowmode15", bf, 512, 7680, 4, 2, 64, promises={"bpr": {"down": 15}})
    add("blockmode16", bf, 512, 8192, 4, 2, 64, promises={"bpr": {"down": 16}, "slots": {"down": [16] * 8}, "padding": {"down": 0}})
    add("rowmode15", f32, 512, 3840, 4, 2, 64, promises={"bpr": {"down": 15}})
    add("blockmode16", f32, 512, 4096, 4, 2, 64, promises={"bpr": {"down": 16}, "slots": {"down": [16] * 8}, "padding": {"down": 0}})
    # 4: block mode, odd blocks per row, a ragged share of more than one group
    add("blockmode19", bf, 1024, 9728, 4, 2, 128, promises={"bpr": {"down": 19}, "slots": {"down": [32] * 8}, "padding": {"down": 13 * 8}})
    # 5: H at its limit (fp32: 15 blocks per row)
    add("hlimit", f32, 3840, 1024, 2, 1, 256, promises={"bpr": {"gu": 15, "qkv": 15}})
    # 6: merge slices that straddle two q heads (and slices inside one): 24 outputs per workgroup do not divide the 128 of a head (rows
    # of whole KiB need qd in multiples of 512 / 256 values, so 3 q heads are not a shape the kernel admits; 12 are)
    for dt in (bf, f32):
        add("straddle", dt, 512, 1024, 12, 4, 64, promises={"straddle": True, "per": {"A": 24}})
    # 7: live split counts 1, 1 (a full tile), 2, all
    for i, kv in enumerate((1, 64, 65, 256)):
        add("splits", (bf, f32)[i % 2], 512, 1024, 4, 2, 64, fams=("exact",) if i % 2 else (None,), kv_len=kv, promises={"live": (1, 1, 2, 4)[i]})
    add("splits-tps2", bf, 512, 1024, 4, 2, 64, fams=("exact",), kv_len=129, tps=2, promises={"live": 2})
    # 8: last layer; middle layer without bias
    for dt in (bf, f32):
        add("last", dt, 512, 1024, 4, 2, 64, has_next=False)
        add("nobias", dt, 512, 1024, 4, 2, 64, fams=(None,), bias=False)
    return out


CASES = cases()
