"""CPU case builder, float64 reference and fp32 restatement of the token log-probabilities (svln_set_token_scores): the EPI_ARGMAX_LSE
siblings of the lm_head kernels (gemv.hip gemv_rows_kernel / gemv_batched_kernel, the 32 x 128 MFMA arg-max epilogue of gemm.hip) and the
final kernels that merge their partials.  Test infrastructure, modelled on tests/gemv_ref.py.

    logprob = l_t - logsumexp_j(l_j),  t = argmax_j l_j (lowest index on ties), over the PROCESSED logits (after the repetition penalty)

Exact inputs.  Weights and activations come from {0, +-1/2, +-1, +-2} and every logit is DESIGNED: activation row b owns a block of 16
columns (x = 2 in eight of them, 1 in three) in which weight row n spells its logit L[b][n], a multiple of 1/2 with |L| <= 35; every other
column pair holds (w, -w) against equal activations and cancels exactly.  All products and partial sums are small dyadic numbers, so the
fp32 logit is L[b][n] bit for bit in any summation order, on the FMA chain, the packed dot products and the MFMAs alike; with penalty 2
the processed logits are exact too.  What is left to tolerance is the log-sum-exp alone.

Sharp placement.  One dropped row of weight exp(0) among 152 064 moves the result by 7e-6, below any tolerance, so a case keeps its
background 20 .. 30 below the row's top value and plants HEAVY rows (top, top - 1, a tie) where a mistake would look: in the ragged tail,
late in a wave's order, in another wave / workgroup / tile, in the last valid column, in a flagged penalty row.  Odd rows of a batch
have a negative top, so that a counted column beyond N (logit 0) is heavy there.

Mutants: the restatement with one plausible kernel mistake each; tests/test_scores_inputs.py proves that every one moves some case by
>= 100 x the op tolerance while the correct restatement stays inside it.
"""
import functools

import numpy as np
import torch

import gemv_ref as G

TOL = 2e-5                  # op-level bound on |logprob - float64 reference| (fp32 sums of a few dozen sequential terms, 1-ulp exp / log on
                            # arguments bounded by 30; the margin is for the hardware transcendentals)
PEN = 2.0                   # repetition penalty of the penalised cases: halving / doubling is exact
BLOCK = 16                  # designed columns per activation row
VALUES = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
MUTANTS = ("no_rescale", "ragged_twice", "cols_ge_N", "rows_ge_M", "pen_compare_only", "wrong_flag_row", "merge_no_rescale",
           "winner_partial_only", "empty_wave_nan", "row0_max")
F = np.float32
NEG = F(-np.inf)


# ---------------------------------------------------------------------------------------------------------- designed operands
def design_x(B, K, seed):
    """activations [B][K] float64: row b = (2 x 8, 1 x 3, 1/2 x 5) in its own block b, zero in the other blocks, and pairs of equal
    non-zero values in the cancelling columns from B * BLOCK on"""
    assert K >= B * BLOCK + 2 and (K - B * BLOCK) % 2 == 0, (B, K)
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((B, K), dtype=torch.float64)
    blk = torch.tensor([2.0] * 8 + [1.0] * 3 + [0.5] * 5, dtype=torch.float64)
    for b in range(B):
        x[b, b * BLOCK:(b + 1) * BLOCK] = blk
    nz = torch.tensor(VALUES[1:], dtype=torch.float64)
    pairs = nz[torch.randint(0, len(nz), (B, (K - B * BLOCK) // 2), generator=g)]
    x[:, B * BLOCK:] = pairs.repeat_interleave(2, 1)
    return x


def design_w(L, K, seed, dtype=torch.float32):
    """weights [N][K] in `dtype` (every value is exact in bf16) with W . x_b = L[b] exactly for x = design_x(B, K, .); L [B][N] multiples
    of 1/2, |L| <= 35.5"""
    B, N = L.shape
    assert float(L.abs().max()) <= 35.5 and bool((L * 2 == (L * 2).round()).all())
    g = torch.Generator().manual_seed(seed + 1)
    W = torch.zeros((N, K), dtype=dtype)
    for b in range(B):
        a, sg = L[b].abs(), torch.sign(L[b])
        n4 = torch.floor(a / 4)
        rem = a - 4 * n4
        blk = torch.zeros((N, BLOCK), dtype=torch.float64)
        blk[:, :8] = (torch.arange(8)[None] < n4[:, None]).double() * 2
        for slot, unit, w in ((8, 2.0, 2.0), (9, 1.0, 1.0), (10, 0.5, 0.5)):
            take = rem >= unit
            blk[:, slot] = take.double() * w
            rem = rem - take.double() * unit
        assert float(rem.abs().max()) == 0
        W[:, b * BLOCK:(b + 1) * BLOCK] = (blk * sg[:, None]).to(dtype)
    vals = torch.tensor(VALUES, dtype=dtype)
    half = vals[torch.randint(0, len(vals), (N, (K - B * BLOCK) // 2), generator=g)]
    W[:, B * BLOCK::2] = half
    W[:, B * BLOCK + 1::2] = -half
    return W


def pack(fmt, W):
    """device operands of weight format fmt for the exact values W [N][K] (unit scales: the scale handling is pinned by tests/gemv_ref.py)"""
    N, K = W.shape
    if fmt.startswith("plain"):
        return {"W": W.to(G.DTYPE[fmt])}
    if fmt == "e4m3":
        return {"W": W.float().to(torch.float8_e4m3fn).view(torch.uint8), "aux": torch.ones(N, dtype=torch.float32)}
    a = W.float().abs()
    code = sum((a > m).to(torch.uint8) for m in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)) | ((W.float() < 0).to(torch.uint8) << 3)
    return {"W": (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous(), "aux": torch.full((N, K // 32), 127, dtype=torch.uint8)}


FMT_ID = {"plain-fp32": 0, "plain-bf16": 0, "e4m3": 1, "mxfp4": 2}


# ---------------------------------------------------------------------------------------------------------- logits
def background(B, N, tops, seed):
    g = torch.Generator().manual_seed(seed + 2)
    L = -torch.randint(40, 61, (B, N), generator=g).double() / 2            # 20 .. 30 below the top, in halves
    return L + torch.tensor(tops, dtype=torch.float64)[:, None]


def processed(L, flags, pen_rows, pen):
    """float64 processed logits [B][N]: HF's RepetitionPenaltyLogitsProcessor through row b's flag row"""
    if flags is None:
        return L.clone()
    f = flags[torch.as_tensor(pen_rows, dtype=torch.long)].bool()
    return torch.where(f, torch.where(L < 0, L * pen, L / pen), L)


def reference(Lp):
    """(tokens [B], float64 log-probabilities [B]) of processed logits Lp [B][N]; lowest index on ties"""
    Lp = Lp.double()
    tok = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in Lp])
    return tok, Lp.gather(1, tok[:, None])[:, 0] - torch.logsumexp(Lp, 1)


# ---------------------------------------------------------------------------------------------------------- fp32 restatement
def _exp(d):
    return np.exp(F(d), dtype=F)


def _add(v, m, s, mut):
    """lse_add of common.h: logit v joins the running (m, s)"""
    if v > m:
        s = (s if mut == "no_rescale" else s * _exp(m - v)) + F(1)
        return v, F(s)
    return m, F(s + (F(0) if v == NEG else _exp(v - m)))


def _rescale(s, m, V):
    """lse_rescale of common.h: the empty partial (-inf, 0) merges as 0"""
    return F(0) if s == 0 else F(s * _exp(m - V))


def _merge(parts, mut):
    """[(m, s, lowest index)] of one level -> (V, S, index): greatest m, lowest index on ties, S = sum s_k exp(m_k - V).
    Mutants: merge_no_rescale (plain sum), winner_partial_only, empty_wave_nan (pairwise online merge without the empty guard)."""
    V, I = NEG, 0x7FFFFFFF
    for m, _, i in parts:
        if m > V or (m == V and i < I):
            V, I = m, i
    if mut == "empty_wave_nan":
        lvl = [(m, s) for m, s, _ in parts]
        while len(lvl) > 1:
            nxt = []
            for k in range(0, len(lvl) - 1, 2):
                (ma, sa), (mb, sb) = lvl[k], lvl[k + 1]
                mm = max(ma, mb)
                nxt.append((mm, F(sa * _exp(ma - mm) + sb * _exp(mb - mm))))
            if len(lvl) % 2:
                nxt.append(lvl[-1])
            lvl = nxt
        return V, lvl[0][1], I
    if mut == "winner_partial_only":
        return V, next(s for m, s, i in parts if m == V and i == I), I
    S = F(0)
    for m, s, _ in parts:
        S = F(S + (s if mut == "merge_no_rescale" else _rescale(s, m, V)))
    return V, S, I


def _final(parts, mut, V_override=None):
    """argmax_final_*: thread t sums the rescaled partials k = t, t + 256, ..; fixed tree over the 256 threads"""
    V, _, I = _merge(parts, None)
    Vn = V if V_override is None else V_override
    if mut in ("merge_no_rescale", "winner_partial_only", "empty_wave_nan"):
        S = _merge(parts, mut)[1]
    else:
        mine = [F(0)] * 256
        for k, (m, s, _) in enumerate(parts):
            mine[k % 256] = F(mine[k % 256] + _rescale(s, m, Vn))
        w = 128
        while w:
            for t in range(w):
                mine[t] = F(mine[t] + mine[t + w])
            w //= 2
        S = mine[0]
    tok = -1 if I == 0x7FFFFFFF else I
    return tok, (float("nan") if tok < 0 else float(-np.log(S, dtype=F)))


def _vals(L, flags_row, pen, mut):
    """(compared, summed) fp32 logits of one activation row"""
    raw = L.numpy().astype(F)
    if flags_row is None:
        return raw, raw
    f = flags_row.numpy().astype(bool)
    p = np.where(f, np.where(raw < 0, raw * F(pen), raw / F(pen)), raw).astype(F)
    return p, (raw if mut == "pen_compare_only" else p)


def restate_rows(L, flags=None, pen=PEN, mut=None):
    """gemv_rows_kernel<P, EPI_ARGMAX_LSE> + argmax_final_kernel<true> on the logits L [N] (float64 tensor): wave gw of gemv_grid(N) x 4
    takes the 4-row groups gw, gw + nw, ..; a ragged last group repeats row N - 1 (mutant ragged_twice counts the repeats)"""
    N = L.numel()
    cmp_, sum_ = _vals(L, flags, pen, mut)
    grid = G.gemv_grid(N)
    nw = grid * G.WAVES
    parts = []
    with np.errstate(all="ignore"):
        for wg in range(grid):
            waves = []
            for w in range(G.WAVES):
                m, s, best, bi = NEG, F(0), NEG, 0x7FFFFFFF
                for n0 in range((wg * G.WAVES + w) * 4, N, nw * 4):
                    for r in range(4):
                        n = n0 + r
                        if n >= N and mut != "ragged_twice":
                            continue
                        j = min(n, N - 1)
                        if n < N and cmp_[j] > best:
                            best, bi = cmp_[j], j
                        m, s = _add(sum_[j], m, s, mut)
                waves.append((best if mut == "pen_compare_only" else m, s, bi))
            parts.append(_merge(waves, mut))
        parts = [(V, S, I) for V, S, I in parts]
        return _final(parts, mut)


def restate_batched(L, flags=None, pen_rows=None, pen=PEN, mut=None):
    """gemv_batched_kernel<.., EPI_ARGMAX_LSE, .., B> + argmax_final_batched_kernel<true> on L [B][N]: workgroup k of min(units, 2048)
    takes the 4-row units k, k + grid, ..; thread b keeps row b's (max, sum) and reads the flag row pen_rows[b]"""
    B, N = L.shape
    units = (N + 3) // 4
    grid = min(units, 2048)
    out = []
    with np.errstate(all="ignore"):
        V0 = None
        for b in range(B):
            fr = None if flags is None else flags[pen_rows[0 if mut == "wrong_flag_row" else b]]
            cmp_, sum_ = _vals(L[b], fr, pen, mut)                 # (wrong_flag_row: the compare takes the wrong row too -- the mistake is the pointer)
            parts = []
            for k in range(grid):
                m, s, best, bi = NEG, F(0), NEG, 0x7FFFFFFF
                for u in range(k, units, grid):
                    for r in range(4):
                        n = 4 * u + r
                        if n >= N and mut != "ragged_twice":
                            continue
                        j = min(n, N - 1)
                        if n < N and cmp_[j] > best:
                            best, bi = cmp_[j], j
                        m, s = _add(sum_[j], m, s, mut)
                parts.append((best if mut == "pen_compare_only" else m, s, bi))
            if b == 0:
                V0 = _merge(parts, None)[0]
            out.append(_final(parts, mut, V0 if mut == "row0_max" else None))
    return out


def restate_mfma(L, flags=None, pen_rows=None, pen=PEN, mut=None):
    """the EPI_ARGMAX_LSE epilogue of the 32 x 128 tiles (2 waves x 64 columns; lane r32 holds columns j * 32 + r32, j < 2) +
    argmax_final_batched_kernel<true> on L [M][N].  Mutants: cols_ge_N (the zero logits of the columns beyond N are counted), rows_ge_M
    (the tile rows beyond M, which clamp to row M - 1, are counted into it), empty_wave_nan (exp(-inf - -inf) for the columns beyond N of
    a wave that has no column below N)."""
    M, N = L.shape
    tiles = (N + 127) // 128
    out = []
    with np.errstate(all="ignore"):
        V0 = None
        for b in range(M):
            fr = None if flags is None else flags[pen_rows[0 if mut == "wrong_flag_row" else b]]
            cmp_, sum_ = _vals(L[b], fr, pen, mut)
            parts = []
            for t in range(tiles):
                waves = []
                for w in range(2):
                    cols = [t * 128 + w * 64 + j * 32 + r for r in range(32) for j in range(2)]       # lane-major
                    v, vi = NEG, 0x7FFFFFFF
                    for n in cols:
                        if n < N and (cmp_[n] > v or (cmp_[n] == v and n < vi)):
                            v, vi = cmp_[n], n
                    lane = []
                    for r in range(32):
                        a = F(0)
                        for j in range(2):
                            n = t * 128 + w * 64 + j * 32 + r
                            if n < N:
                                a = F(a + (F(0) if sum_[n] == NEG else _exp(sum_[n] - v)))
                            elif mut == "cols_ge_N":
                                a = F(a + _exp(F(0) - v))
                            elif mut == "empty_wave_nan":      # the unguarded -inf column of a wave whose maximum is -inf too
                                a = F(a + _exp(NEG - v))
                        lane.append(a)
                    o = 1
                    while o < 32:                              # the xor-shuffle tree
                        lane = [F(lane[r] + lane[r ^ o]) for r in range(32)]
                        o *= 2
                    waves.append((v, lane[0], vi))
                parts.append(_merge(waves, mut))
            if mut == "rows_ge_M" and b == M - 1:
                parts = [(V, F(S * F(32 - M + 1)), I) for V, S, I in parts]
            if b == 0:
                V0 = _merge(parts, None)[0]
            out.append(_final(parts, mut, V0 if mut == "row0_max" else None))
    return out


# ---------------------------------------------------------------------------------------------------------- cases
class Case:
    """kind "rows" (B = 1), "batched" (B = 1, 2, 4, 8) or "mfma" (M = B <= 32).  L [B][N]: designed raw logits; flags [8 or B][N] uint8 +
    pen_rows [B], or None.  tie: two rows share the top, the lowest index must win."""

    def __init__(self, kind, N, K, B=1, fmt="plain-fp32", pen=False, tie=False, norm=False, seed=0):
        self.kind, self.N, self.K, self.B, self.fmt, self.pen, self.tie, self.norm, self.seed = kind, N, K, B, fmt, pen, tie, norm, seed
        self.id = f"{kind}-{fmt}-B{B}-N{N}-K{K}" + ("-pen" if pen else "") + ("-tie" if tie else "") + ("-norm" if norm else "")

    @property
    def dtype(self):
        return G.DTYPE[self.fmt]

    def tops(self):
        # odd rows of a batch sit below zero (whole numbers: their halved penalty rows stay multiples of 1/2): a counted logit 0 (a column
        # beyond N) is heavy there; neighbouring rows never share a top
        return [(12.0 - 0.5 * ((b // 2) % 8)) if b % 2 == 0 else (-1.0 - ((b // 2) % 4)) for b in range(self.B)]

    def heavy_rows(self, b):
        """where row b's top, its runner-up (top - 1) and, with a penalty, the flagged row that would win un-penalised sit"""
        N, kind = self.N, self.kind
        if N == 1:
            return {"top": 0}
        if kind == "rows":
            nw = G.gemv_grid(N) * G.WAVES
            groups = (N + 3) // 4
            if groups > nw:                                   # some waves loop twice: runner-up first, the top in the wave's second group
                g0 = (groups - nw) // 2
                h = {"up": 4 * g0 + 1, "top": min(4 * (g0 + nw) + 2, N - 1)}
            else:                                             # the same group: the top comes after the runner-up in the wave's order
                g0 = groups // 3
                h = {"up": 4 * g0, "top": min(4 * g0 + 2, N - 2)}
            h["tail"] = N - 1                                 # the ragged tail / last row, in another workgroup when there is one
        else:
            last_tile = 128 * ((N - 1) // 128)
            h = {"up": min(5 + b, N - 2), "top": min(last_tile // 2 + 7 + 4 * b, N - 2) if N > 130 else max(N - 2 - b % 3, 1), "tail": N - 1}
            if h["up"] == h["top"]:
                h["up"] = 0
        return h

    @functools.lru_cache(maxsize=None)
    def logits(self):
        B, N = self.B, self.N
        tops = self.tops()
        L = background(B, N, tops, self.seed)
        flags = torch.zeros((8 if self.kind != "mfma" else B, N), dtype=torch.uint8) if self.pen else None
        rows = [(3 * b + 1) % (8 if self.kind != "mfma" else B) for b in range(B)] if self.pen else None
        g = torch.Generator().manual_seed(self.seed + 3)
        for b in range(B):
            h = self.heavy_rows(b)
            T = tops[b]
            L[b, h["top"]] = T
            if "up" in h and h["up"] != h["top"]:
                L[b, h["up"]] = T - 1
            if "tail" in h and h["tail"] not in (h["top"], h.get("up")):
                L[b, h["tail"]] = T - 1 if not self.tie else T
            if self.tie and N > 1 and "tail" in h and h["tail"] == h["top"]:
                L[b, 0] = T
            if self.pen:
                fr = flags[rows[b]]
                fr[torch.randint(0, N, (max(N // 16, 1),), generator=g)] = 1
                fr[h["top"]] = 0                              # (the winner is found among the processed values: keep it designed)
                n = next((n for n in list(range(N // 2, N)) + list(range(N // 2)) if n not in h.values()), None)
                if n is not None:                             # a flagged row that carries weight exp(-1) after the penalty, far more before
                    fr[n] = 1
                    L[b, n] = (T - 1) * PEN if T - 1 >= 0 else (T - 1) / PEN
        if self.pen:                                          # the heavy rows of b must not be flagged through another row's placement
            for b in range(B):
                h = self.heavy_rows(b)
                for key in ("up", "tail"):
                    if key in h and float(L[b, h[key]]) >= self.tops()[b] - 1:
                        flags[rows[b], h[key]] = 0
        return L, flags, rows

    def processed(self):
        L, flags, rows = self.logits()
        return processed(L, flags, rows, PEN)

    def reference(self):
        return reference(self.processed())

    def restate(self, mut=None):
        L, flags, rows = self.logits()
        if self.kind == "rows":
            return [restate_rows(L[0], None if flags is None else flags[rows[0]], PEN, mut)]
        return (restate_batched if self.kind == "batched" else restate_mfma)(L, flags, rows, PEN, mut)

    def operands(self):
        """(x [B][K] float64, W [N][K] exact values in fp32 / bf16)"""
        L, _, _ = self.logits()
        return design_x(self.B, self.K, self.seed), design_w(L, self.K, self.seed, torch.float32 if self.fmt == "plain-fp32" else torch.bfloat16)


def rows_cases(big=True):
    out = []
    for f, fmt in enumerate(G.FORMATS):
        ks = G.k_ladder(fmt)[:2]
        for i, N in enumerate((1, 3, 5, 4 * 4 * 7 + 1, 20497)):
            for j, K in enumerate(ks):
                out.append(Case("rows", N, K, fmt=fmt, pen=(i + j) % 2 == 1, tie=N in (5, 113) and j == 0, seed=10 * f + i))
                if N in (5, 113):                              # both penalty settings where the tail and the penalty meet
                    out.append(Case("rows", N, K, fmt=fmt, pen=(i + j) % 2 == 0, seed=10 * f + i + 5))
    if big:
        out.append(Case("rows", 152064, G.k_ladder("plain-bf16")[0], fmt="plain-bf16", pen=True, seed=77))
    return out


def batched_cases():
    out = []
    for d, fmt in enumerate(("plain-fp32", "plain-bf16")):
        for i, B in enumerate((1, 2, 4, 8)):
            for j, N in enumerate((1, 5, 8193)):
                out.append(Case("batched", N, 192 if (i + j) % 2 else 512, B=B, fmt=fmt, pen=(i + j + d) % 2 == 0, norm=(i + d) % 2 == 1,
                                tie=N == 5 and i % 2 == 0, seed=100 + 10 * i + j))
                out.append(Case("batched", N, 512 if (i + j) % 2 else 192, B=B, fmt=fmt, pen=(i + j + d) % 2 == 1, norm=(i + d) % 2 == 0, seed=150 + 10 * i + j))
    return out


def mfma_cases():
    out = []
    for d, fmt in enumerate(("plain-fp32", "plain-bf16")):
        for i, M in enumerate((4, 5, 31, 32)):
            for j, N in enumerate((1, 127, 128, 129, 16385)):
                out.append(Case("mfma", N, 576 if (i + j + d) % 2 else 1024, B=M, fmt=fmt, pen=(i + j) % 2 == 0, tie=j == 3, seed=200 + 10 * i + j))
    return out


def cpu_cases():
    """the cases the CPU proof walks: every kernel shape and size class, without the sizes that only repeat a class at Python-loop cost"""
    rows = [c for c in rows_cases(big=False) if c.fmt == "plain-fp32"]
    bat = [c for c in batched_cases() if c.fmt == "plain-fp32" and (c.N < 8193 or c.B == 2)]
    mf = [c for c in mfma_cases() if c.fmt == "plain-fp32" and (c.N < 16385 or c.B == 5)]
    return rows + bat + mf


KIND_MUTANTS = {
    "rows": ("no_rescale", "ragged_twice", "pen_compare_only", "merge_no_rescale", "winner_partial_only", "empty_wave_nan"),
    "batched": ("no_rescale", "ragged_twice", "pen_compare_only", "wrong_flag_row", "merge_no_rescale", "winner_partial_only", "row0_max"),
    "mfma": ("cols_ge_N", "rows_ge_M", "pen_compare_only", "wrong_flag_row", "merge_no_rescale", "winner_partial_only",
             "empty_wave_nan", "row0_max"),
}
