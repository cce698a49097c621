"""CPU case builder, float64 reference and restatement of temperature sampling (svln_set_sampling): the EPI_SAMPLE siblings of the lm_head
kernels (gemv.hip gemv_rows_kernel / gemv_batched_kernel, the 32 x 128 MFMA arg-max epilogue of gemm.hip) and the final kernels that merge
their partials.  Test infrastructure, modelled on tests/scores_ref.py, whose exact-logit designs (design_x / design_w / pack) it reuses.

    token = argmax_n ( fl(x_n * invT) + G(seed, stream, draw, n) ),  lowest column on ties; x = the PROCESSED logit (after the penalty)
    score = log softmax(x * invT)[token]

Noise.  Philox4x32-10 on counter (column, draw, stream, 0) and key (seed lo, seed hi), output word 0 = w; u = ((w >> 9) + 0.5) * 2^-23;
E = -ln u; G = -ln E.  Restated here in numpy integers and float64.

Exact inputs.  The raw logits are multiples of 1/2 with |L| <= 35.5, spelled exactly by design_w against design_x; the penalty is 2 and
T is 1, 1/2 or 2, so y = fl(x * invT) is exact as well.  What is left to tolerance is the noise (two hardware logarithms) and the
log-sum-exp.  Unlike the cases of scores_ref, the logits of a row lie within a few units of each other, so the noise decides the winner
and the sampled token is usually NOT the greedy one.

Margins.  A case is usable on the GPU when the two best perturbed values of every row lie >= 100 tolerances apart,
tol = 2^-17 max(1, |G_a|, |G_b|) + 2^-22 max|z| (the noise bound of tests/test_sample_gpu.py, doubled, plus the rounding of y + G); the
case's seed is the first one from its base for which every row does (find_seed: deterministic, checked by tests/test_sample_inputs.py).

Mutants: the restatement with one plausible kernel mistake each; tests/test_sample_inputs.py proves that every one changes some case's
token or moves its score by >= 100 tolerances.
"""
import functools

import numpy as np
import torch

import gemv_ref as G
import scores_ref as S

TOL = S.TOL                 # op-level bound on |score - float64 reference|
PEN = S.PEN
F = np.float32
NEG = F(-np.inf)
NONE = 0x7FFFFFFF
M32 = np.uint64(0xFFFFFFFF)
TEMPS = (1.0, 0.5, 2.0)
MUTANTS = ("local_column", "row_as_stream", "draw_stuck", "pen_after_noise", "lse_on_z", "score_from_max_y", "ragged_twice", "cols_ge_N",
           "rows_ge_M", "u24", "empty_poison")


# ---------------------------------------------------------------------------------------------------------- noise
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """output word 0 of Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11); array counters"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def noise_bits(seed, stream, draw, cols):
    return philox4x32_10(cols, draw, stream, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def uniform(w):
    """u in [2^-24, 1 - 2^-24], exact in fp32 and float64"""
    return ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def uniform24_fp32(w):
    """the 24-bit mistake in fp32: 16777215.5 rounds to 2^24, u = 1"""
    return (((w >> np.uint64(8)).astype(F) + F(0.5)) * F(2.0 ** -24)).astype(np.float64)


def gumbel(seed, stream, draw, cols, u24=False):
    """float64 standard Gumbel noise of the columns `cols`; E = -log u through log1p next to u = 1"""
    w = noise_bits(seed, stream, draw, cols)
    u = uniform24_fp32(w) if u24 else uniform(w)
    with np.errstate(divide="ignore"):
        E = np.where(u >= 0.5, -np.log1p(-(1.0 - u)), -np.log(u))
        return -np.log(E)


# ---------------------------------------------------------------------------------------------------------- partial layout
def layout(kind, N):
    """(sub, part, local, subs_per_part, n_parts, padded) of the columns 0 .. padded - 1: the wave (sub-partial) and the workgroup / tile
    (partial) that own column n, its index inside the producer's smallest unit, and the columns up to `padded` that the producer's
    last unit touches beyond N (clamped rows of a ragged group / the tile's zero columns)"""
    if kind == "rows":
        grid = G.gemv_grid(N)
        padded = 4 * ((N + 3) // 4)
        n = np.arange(padded)
        gw = (n // 4) % (grid * G.WAVES)
        return gw, gw // G.WAVES, n % 4, G.WAVES, grid, padded
    if kind == "batched":
        units = (N + 3) // 4
        grid = min(units, 2048)
        padded = 4 * units
        n = np.arange(padded)
        p = (n // 4) % grid
        return p, p, n % 4, 1, grid, padded
    tiles = (N + 127) // 128
    n = np.arange(tiles * 128)
    return n // 64, n // 128, n % 128, 2, tiles, tiles * 128


def _exp(d):
    return np.exp(F(d), dtype=F)


def _rescale(s, m, V):
    return F(0) if s == 0 else F(s * _exp(m - V))


def _merge(subs, mut):
    """[(z, idx, raw, max y, sum)] -> one such tuple: the winner on (z, idx), V = max of the maxima, S = sum of the rescaled sums.
    empty_poison: a pairwise online merge without the guard for two empty partials (exp(-inf - -inf))"""
    z, i, raw = NEG, NONE, NEG
    for sz, si, sr, _, _ in subs:
        if sz > z or (sz == z and si < i):
            z, i, raw = sz, si, sr
    if mut == "empty_poison":
        lvl = [(m, s) for _, _, _, m, s in subs]
        while len(lvl) > 1:
            nxt = []
            for k in range(0, len(lvl) - 1, 2):
                (ma, sa), (mb, sb) = lvl[k], lvl[k + 1]
                mm = max(ma, mb)
                nxt.append((mm, F(sa * _exp(ma - mm) + sb * _exp(mb - mm))))
            if len(lvl) % 2:
                nxt.append(lvl[-1])
            lvl = nxt
        return z, i, raw, lvl[0][0], lvl[0][1]
    V = max([m for _, _, _, m, _ in subs] + [NEG])
    S_ = F(0)
    for _, _, _, m, s in subs:
        S_ = F(S_ + _rescale(s, m, V))
    return z, i, raw, V, S_


def restate_row(kind, x, flags_row, pen, inv_t, seed, stream, draw, mut=None, M_pad=1):
    """one activation row through producer `kind` and its final kernel: (token, score).  x [N] float64 raw logits (exact in fp32).
    M_pad (mutant rows_ge_M, last row of an MFMA case): how many tile rows compute this row, itself included"""
    N = x.size
    sub, part, local, spp, n_parts, padded = layout(kind, N)
    cols = np.arange(padded)
    # a ragged group repeats the last row; a tile's extra columns are zeros
    raw = np.where(cols < N, x[np.minimum(cols, N - 1)], x[N - 1] if kind != "mfma" else 0.0).astype(F)
    fl = np.zeros(padded, dtype=bool)
    if flags_row is not None:
        fl[:N] = flags_row.astype(bool)
        if kind != "mfma":
            fl[N:] = fl[N - 1]

    def penal(v):
        return np.where(fl, np.where(v < 0, v * F(pen), v / F(pen)), v).astype(F)

    with np.errstate(all="ignore"):
        g = gumbel(seed, stream, draw, local if mut == "local_column" else cols, u24=mut == "u24").astype(F)
        if mut == "pen_after_noise":
            y = (raw * F(inv_t)).astype(F)
            z = penal((y + g).astype(F))
        else:
            y = (penal(raw) * F(inv_t)).astype(F)
            z = (y + g).astype(F)
        live = cols < N
        joins_max = live | (mut == "cols_ge_N")
        joins_sum = live | (mut in ("cols_ge_N", "ragged_twice"))
        t = z if mut == "lse_on_z" else y
        order = np.lexsort((cols, sub))
        bounds = np.flatnonzero(np.diff(sub[order])) + 1
        groups = dict((int(sub[o[0]]), o) for o in np.split(order, bounds))
        parts = []
        for p in range(n_parts):
            subs = []
            for s in range(spp):
                o = groups.get(p * spp + s if spp > 1 else p)
                if o is None:
                    subs.append((NEG, NONE, NEG, NEG, F(0)))
                    continue
                om, os_ = o[joins_max[o]], o[joins_sum[o]]
                bz, bi, br = NEG, NONE, NEG
                if om.size:
                    zz = z[om]
                    zz = np.where(np.isnan(zz), NEG, zz)
                    k = int(np.argmax(zz))                          # columns ascend inside a sub-partial: the first maximum is the lowest
                    if zz[k] > NEG:
                        bz, bi, br = zz[k], int(om[k]), y[om[k]]
                m, sm = NEG, F(0)
                if os_.size:
                    m = F(t[os_].max())
                    if m > NEG:
                        sm = F(np.exp((t[os_] - m).astype(np.float64))[t[os_] > NEG].sum())
                subs.append((bz, bi, br, m, sm))
            if mut == "rows_ge_M":       # the tile rows at or beyond M, which compute row M - 1 again (clamped), join its reduction
                subs = subs * M_pad
            parts.append(_merge(subs, mut))
        z_, i_, raw_, V, S_ = _merge(parts, None if mut == "empty_poison" else mut)
        if mut == "score_from_max_y":
            raw_ = next(r for _, _, r, m, _ in parts if m == V)
        tok = -1 if i_ == NONE else i_
        return tok, (float("nan") if tok < 0 else float(F(F(raw_ - V) - np.log(S_, dtype=F))))


def reference_row(x, flags_row, pen, inv_t, seed, stream, draw):
    """float64: (token, score, margin of the two best perturbed values, tolerance of that margin)"""
    x = x.astype(np.float64)
    p = x if flags_row is None else np.where(flags_row.astype(bool), np.where(x < 0, x * pen, x / pen), x)
    y = p * float(F(inv_t))
    g = gumbel(seed, stream, draw, np.arange(x.size))
    z = y + g
    z = np.where(np.isnan(z), -np.inf, z)
    a = int(np.argmax(z))
    if not z[a] > -np.inf:
        return -1, float("nan"), float("inf"), 0.0
    rest = np.delete(z, a)
    b = int(np.argmax(rest)) if rest.size else None
    fin = y[y > -np.inf]
    lse = fin.max() + np.log(np.exp(fin - fin.max()).sum())
    if b is None or not rest[b] > -np.inf:
        return a, float(y[a] - lse), float("inf"), 0.0
    gb = np.delete(g, a)[b]
    tol = 2.0 ** -17 * max(1.0, abs(g[a]), abs(gb)) + 2.0 ** -22 * float(np.abs(z[z > -np.inf]).max())
    return a, float(y[a] - lse), float(z[a] - rest[b]), tol


# ---------------------------------------------------------------------------------------------------------- cases
class Case:
    """kind "rows" (B = 1), "batched" (B = 1, 2, 4, 8) or "mfma" (M = B <= 32).  Row b uses streams[b], draws[b]; rows 2k and 2k + 1 share
    their logits and differ in stream and draw only.  ninf: column N // 2 of row 0 holds -inf (plain formats, B = 1)."""

    def __init__(self, kind, N, K, B=1, fmt="plain-fp32", T=1.0, pen=False, ninf=False, seed=0):
        self.kind, self.N, self.K, self.B, self.fmt, self.T, self.pen, self.ninf, self.base = kind, N, K, B, fmt, T, pen, ninf, seed
        self.id = f"{kind}-{fmt}-B{B}-N{N}-K{K}-T{T}" + ("-pen" if pen else "") + ("-ninf" if ninf else "")
        self.streams = [(5 * b + 3) % 8 for b in range(B)]
        self.draws = [7 + 3 * b + (1000003 if b == 1 else 0) for b in range(B)]
        self.forced = None
        self.low = None            # a column of row 0 whose logit sits 30 lower: it loses under any finite noise

    @property
    def dtype(self):
        return G.DTYPE[self.fmt]

    @property
    def inv_t(self):
        return float(F(1.0) / F(self.T))

    @functools.lru_cache(maxsize=None)
    def logits(self):
        """L [B][N] raw logits in halves within 6 of the row's top (even rows above zero, odd rows below: a counted zero column is heavy
        there), flags [B or 8][N] + pen_rows, or None"""
        B, N = self.B, self.N
        g = torch.Generator().manual_seed(1000 + self.base)
        L = torch.zeros((B, N), dtype=torch.float64)
        for b in range(0, B, 2):
            top = 3.0 - 0.5 * (b % 4)
            row = top - torch.randint(0, 13, (N,), generator=g).double() / 2
            L[b] = row
            if b + 1 < B:
                L[b + 1] = row if (b // 2) % 2 == 0 else row - 8.0      # (pairs with the same logits; every other pair below zero)
        if self.low is not None:
            L[0, self.low] -= 30.0
        flags = rows = None
        if self.pen:
            R = B if self.kind == "mfma" else 8
            flags = torch.zeros((R, N), dtype=torch.uint8)
            rows = [(3 * b + 1) % R for b in range(B)]
            for b in range(B):
                flags[rows[b]][torch.randint(0, N, (max(N // 3, 1),), generator=g)] = 1
        return L, flags, rows

    def row_inputs(self, b):
        L, flags, rows = self.logits()
        x = L[b].numpy().copy()
        if self.ninf and b == 0:
            x[self.N // 2] = -np.inf
        return x, (None if flags is None else flags[rows[b]].numpy())

    def margins_ok(self, seed):
        for b in range(self.B):
            x, fr = self.row_inputs(b)
            _, _, margin, tol = reference_row(x, fr, PEN, self.inv_t, seed, self.streams[b], self.draws[b])
            if margin < 100 * tol:
                return False
        return True

    @property
    @functools.lru_cache(maxsize=None)
    def seed(self):
        if self.forced is not None:
            return self.forced
        s = 0x5EED0000 + 97 * self.base
        while not self.margins_ok(s):
            s += 1
        return s

    def reference(self):
        return [reference_row(*self.row_inputs(b), PEN, self.inv_t, self.seed, self.streams[b], self.draws[b]) for b in range(self.B)]

    def restate(self, mut=None):
        out = []
        for b in range(self.B):
            x, fr = self.row_inputs(b)
            st = b if mut == "row_as_stream" else self.streams[b]
            dr = self.draws[0] if mut == "draw_stuck" else self.draws[b]
            pad = 32 - self.B + 1 if (mut == "rows_ge_M" and b == self.B - 1) else 1
            out.append(restate_row(self.kind, x, fr, PEN, self.inv_t, self.seed, st, dr, mut, pad))
        return out

    def operands(self):
        """(x [B][K] float64, W [N][K] exact values); the -inf column is spelled by one -inf weight against x = 2"""
        L, _, _ = self.logits()
        W = S.design_w(L, self.K, self.base, torch.float32 if self.fmt == "plain-fp32" else torch.bfloat16)
        if self.ninf:
            assert self.B == 1 and self.fmt.startswith("plain")
            W[self.N // 2, 0] = float("-inf")
        return S.design_x(self.B, self.K, self.base), W


def rows_cases():
    """N = 1, N no multiple of the wave's 4-row group (5, 113), and 20497: 1281 workgroups' worth of groups on a grid of 1024, so some
    workgroups loop twice; all four formats; the three temperatures; both penalty settings"""
    out = []
    for f, fmt in enumerate(G.FORMATS):
        K = G.k_ladder(fmt)[0]
        for i, N in enumerate((1, 5, 113, 20497)):
            out.append(Case("rows", N, K, fmt=fmt, T=TEMPS[(i + f) % 3], pen=(i + f) % 2 == 1, seed=10 * f + i))
        out.append(Case("rows", 113, K, fmt=fmt, T=TEMPS[(f + 1) % 3], pen=f % 2 == 0, seed=10 * f + 5))
    for f, fmt in enumerate(("plain-fp32", "plain-bf16")):
        out.append(Case("rows", 113, G.k_ladder(fmt)[0], fmt=fmt, T=1.0, ninf=True, seed=90 + f))
    return out


def batched_cases():
    """B = 1, 2, 4, 8; N = 5 (one ragged unit) and 8197 (2050 units on 2048 workgroups: two loop twice)"""
    out = []
    for d, fmt in enumerate(("plain-fp32", "plain-bf16")):
        for i, B in enumerate((1, 2, 4, 8)):
            for j, N in enumerate((5, 8197)):
                out.append(Case("batched", N, 192 if (i + j) % 2 else 512, B=B, fmt=fmt, T=TEMPS[(i + j + d) % 3], pen=(i + j + d) % 2 == 0,
                                seed=100 + 10 * i + j))
    return out


def mfma_cases():
    """M = 1, 5, 17, 32; N = 129 (a tile with one live column, its second wave empty) and 128 * 5 + 5; K = 576: 4.5 stages of 128 elements,
    a ragged count of 16-byte chunks per stage in both engine types"""
    out = []
    for d, fmt in enumerate(("plain-fp32", "plain-bf16")):
        for i, M in enumerate((1, 5, 17, 32)):
            for j, N in enumerate((129, 645)):
                out.append(Case("mfma", N, 576, B=M, fmt=fmt, T=TEMPS[(i + j + d) % 3], pen=(i + j) % 2 == 0, seed=200 + 10 * i + j))
    return out


def all_cases():
    return rows_cases() + batched_cases() + mfma_cases()


def cpu_cases():
    """the cases the CPU proof walks through the restatement: the fp32 forms (the formats share the epilogue)"""
    return [c for c in all_cases() if c.fmt == "plain-fp32"]


def u24_case():
    """a rows case whose (seed, draw) puts a column on w >> 8 = 2^24 - 1: the 24-bit form makes u = 1 and G = +inf there, so the column
    wins although its logit lies 30 below the others (its correct noise, the largest possible 16.64, cannot lift it).  Found by a
    search over draws with the restated Philox (tests/test_sample_inputs.py checks the hit)"""
    c = Case("rows", 20497, G.k_ladder("plain-fp32")[0], fmt="plain-fp32", T=1.0, seed=3)
    c.forced, c.draws, c.low = U24_SEED, [U24_DRAW], U24_COLUMN
    c.id += "-u24"
    return c


U24_SEED, U24_DRAW, U24_COLUMN = 0x5EED0123, 1054, 13381        # found by the search below (python tests/sample_ref.py)

KIND_MUTANTS = {
    "rows": ("local_column", "pen_after_noise", "lse_on_z", "score_from_max_y", "ragged_twice", "empty_poison"),
    "batched": ("local_column", "row_as_stream", "draw_stuck", "pen_after_noise", "lse_on_z", "score_from_max_y", "ragged_twice"),
    "mfma": ("local_column", "row_as_stream", "draw_stuck", "pen_after_noise", "lse_on_z", "score_from_max_y", "cols_ge_N", "rows_ge_M"),
}


def search_tail_pairs(seed=0x5EED7A11, stream=1, V=152064, want=72):
    """the search that produced tests/golden/sample_tail_pairs.json: the first `want` (draw, column) pairs over a full vocabulary, draws
    ascending, with u > 1 - 2^-20 (k >= 2^23 - 8) and with u < 2^-20 (k < 8), k = w >> 9"""
    cols = np.arange(V)
    hi, lo, d = [], [], 0
    while len(hi) < want or len(lo) < want:
        k = noise_bits(seed, stream, np.arange(d, d + 8)[:, None], cols[None]) >> np.uint64(9)
        for arr, out in ((np.argwhere(k >= (1 << 23) - 8), hi), (np.argwhere(k < 8), lo)):
            out.extend([d + int(a), int(b)] for a, b in arr)
        d += 8
    return {"seed": seed, "stream": stream, "upper": hi[:want], "lower": lo[:want]}


if __name__ == "__main__":                 # the search that produced U24_DRAW (python tests/sample_ref.py tail: the tail pairs, as JSON)
    import json
    import sys
    if sys.argv[1:] == ["tail"]:
        print(json.dumps(search_tail_pairs()))
        sys.exit(0)
    cols = np.arange(20497)
    for d0 in range(0, 1 << 20, 256):
        w = noise_bits(U24_SEED, 3, np.arange(d0, d0 + 256)[:, None], cols[None])
        hit = np.argwhere((w >> np.uint64(8)) == np.uint64(0xFFFFFF))
        if hit.size:
            print("draw", d0 + int(hit[0][0]), "column", int(hit[0][1]))
            break
