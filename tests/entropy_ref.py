"""CPU case builder, float64 reference and fp32 restatement of the token entropies (svln_token_entropy): the EPI_ARGMAX_LSE_ENT /
EPI_SAMPLE_ENT siblings of the lm_head kernels (gemv.hip gemv_rows_kernel / gemv_batched_kernel, the 32 x 128 MFMA arg-max epilogue of
gemm.hip) and entropy_merge_kernel (misc.hip), which merges their partials.  Test infrastructure; the case machinery (exact operands,
case tables, partial layout, noise) is that of tests/scores_ref.py and tests/sample_ref.py.

    H = log S - T / S,   S = sum_n exp(y_n - V),  T = sum_n (y_n - V) exp(y_n - V),  V = max_n y_n        (nats)

y_n is the PROCESSED logit (after the repetition penalty), times 1 / T under sampling -- never the perturbed z.

Sharp placement.  A far background contributes nothing visible to an entropy, so every row carries HEAVY entries at gaps 0 (ties), 1/2, 1
and 5/2 below its top, planted where a mistake would look: in the ragged tail, late in a wave's order, in another wave / workgroup /
tile, in the last valid column, in a flagged penalty row.  Odd rows of a batch have a negative top, so that a counted column beyond N
(logit 0) is heavy there.  The raw logits are multiples of 1/2 with |L| <= 35.5, spelled exactly by scores_ref.design_w against
design_x; the penalty is 2 and T is 1/2 or 2, so y is exact in fp32 and every difference y - m is exact: what is left to tolerance is
the exponentials, the sums and the logarithm.

Tolerance (derived from the operation order, not from a run).  u = 2^-24.  With d_n = y_n - V <= 0 every summand of S is positive and
every summand of T non-positive, also after any rescale to an intermediate maximum (t_k <= 0, (m_k - V) s_k <= 0): no sum cancels, so
relative errors of summands carry over to the sums.
  * one exponential exp(d) = v_exp_f32(fl(log2e * d)): 1 ulp of the instruction (<= 2 u relative) + the rounded product and the rounded
    constant in the argument (<= 2 |d| u relative): <= (2 + 2 |d|) u;
  * the rescales on a summand's way to V shift by (m - V) in steps whose lengths add up to at most |d_n|: again <= 2 |d_n| u, and each
    of the R steps adds 5 roundings (the exponential's 2 u, two products, the shift's add, the fma): <= 5 R u;
  * L additions lie between a summand and its total (sequential adds of a wave or thread, the shuffle / LDS / block trees): <= L u;
  * the product d * exp(d) is one more rounding.
So  |dS| / S <= u (2 + L + 5 R + 4 a)  and  |dT| / S <= u ((3 + L + 5 R) a + 4 q)  with  a = sum_n p_n |d_n|  and  q = sum_n p_n d_n^2,
and with log S on v_log_f32 (1 ulp, <= 2 u relative) times fl(ln 2), the division and the subtraction:
    |dH| <= u ( (2 + L + 5 R + 4 a)(1 + a) + (3 + L + 5 R) a + 4 q + 3 log S + 2 (a + H) ).
Operation counts: the longest chain is the full vocabulary on the wave-per-rows kernel -- 152064 rows in groups of 4 on 4096 waves: 10
groups = 40 sequential joins, each of which may rescale (R <= 40 + the wave merge + the final merge = 42), then 4 waves, at most 4
partials per merge thread and the 8-level block tree: L <= 40 + 4 + 4 + 8 = 56.  The batched GEMV (8 joins, 8 + 8 tree) and the MFMA
tiles (2 + 5 + 2 joins, 2 rescales, 8 + 8 tree) lie below both.  Design bounds of the cases, asserted in float64 by
tests/test_entropy_inputs.py for every case and temperature: a <= A_MAX, q <= Q_MAX, log S <= LOGS_MAX, H <= H_MAX.
|d exp(d)| <= 1 / e bounds every single summand of T, which is why a and q stay this small whatever the background is.

Mutants: the restatement with one plausible kernel mistake each; tests/test_entropy_inputs.py proves that every one moves some case
written for it by >= 100 x the tolerance (or to NaN) while the correct restatement stays inside it.
"""
import functools
import math

import numpy as np
import torch

import gemv_ref as G
import sample_ref as SM
import scores_ref as S

U = 2.0 ** -24
L_MAX, R_MAX = 56, 42
A_MAX, Q_MAX, LOGS_MAX, H_MAX = 4.0, 40.0, 2.5, 5.0
TOL = U * ((2 + L_MAX + 5 * R_MAX + 4 * A_MAX) * (1 + A_MAX) + (3 + L_MAX + 5 * R_MAX) * A_MAX + 4 * Q_MAX + 3 * LOGS_MAX + 2 * (A_MAX + H_MAX))
PEN = S.PEN
TEMPS = (0.5, 2.0)          # of the sampled forms: 1 / T and x / T are exact
F = np.float32
NEG = F(-np.inf)
NONE = 0x7FFFFFFF
MUTANTS = ("t_no_shift", "merge_no_shift", "empty_nan", "neginf_nan", "ragged_twice", "cols_ge_N", "rows_ge_M", "pen_compare_only",
           "wrong_flag_row", "winner_partial_sum", "row0_VS", "t_on_z", "log_sign")


# ---------------------------------------------------------------------------------------------------------- float64 reference
def reference(y):
    """float64 entropies [B] of the rows of y [B][N] (numpy or tensor): -inf columns carry no mass; a row without a finite value or with
    a NaN gives NaN"""
    y = np.asarray(y, dtype=np.float64)
    out = []
    with np.errstate(all="ignore"):
        for r in y:
            if np.isnan(r).any() or not (r > -np.inf).any():
                out.append(float("nan"))
                continue
            f = r[r > -np.inf]
            d = f - f.max()
            e = np.exp(d)
            out.append(float(np.log(e.sum()) - (d * e).sum() / e.sum()))
    return out


def moments(y):
    """(a, q, log S, H) of one row in float64: the quantities the tolerance is stated in"""
    f = np.asarray(y, dtype=np.float64)
    f = f[f > -np.inf]
    d = f - f.max()
    e = np.exp(d)
    Ssum = e.sum()
    return float((-d * e).sum() / Ssum), float((d * d * e).sum() / Ssum), float(np.log(Ssum)), reference(f[None])[0]


# ---------------------------------------------------------------------------------------------------------- fp32 restatement
def _exp(d):
    return np.exp(F(d), dtype=F)


def _term(v, m, mut=None):
    """ent_term of common.h: one logit's share of t seen from m"""
    if v == NEG and mut != "neginf_nan":
        return F(0)
    d = F(v - m)
    return F(d * _exp(d))


def _add(v, m, s, t, mut=None):
    """ent_add of common.h: logit v joins the running (m, s, t)"""
    if v > m:
        f = _exp(m - v)
        if mut == "t_no_shift":
            t = F(t * f)
        elif s == 0 and mut != "empty_nan":
            t = F(0)
        else:
            t = F(F(t + F(F(m - v) * s)) * f)
        return v, F(F(s * f) + F(1)), t
    return m, F(s + (F(0) if v == NEG else _exp(v - m))), F(t + _term(v, m, mut))


def _rescale_s(s, m, V):
    return F(0) if s == 0 else F(s * _exp(m - V))


def _rescale_t(t, s, m, V, mut=None):
    """ent_rescale of common.h: the partial (m, s, t) seen from V"""
    if s == 0 and mut != "empty_nan":
        return F(0)
    if mut == "merge_no_shift":
        return F(t * _exp(m - V))
    return F(F(t + F(F(m - V) * s)) * _exp(m - V))


def _merge_waves(subs, mut):
    """the sub-partials (m, s, t) of one workgroup / tile -> its partial: V = max, the sums rescaled and added in wave order"""
    V = NEG
    for m, _, _ in subs:
        V = m if m > V else V
    Ssum, T = F(0), F(0)
    for m, s, t in subs:
        Ssum = F(Ssum + _rescale_s(s, m, V))
        T = F(T + _rescale_t(t, s, m, V, mut))
    return V, Ssum, T


def _tree256(mine):
    w = 128
    while w:
        for k in range(w):
            mine[k] = F(mine[k] + mine[k + w])
        w //= 2
    return mine[0]


def merge(parts, mut=None, VS=None):
    """entropy_merge_kernel on one row's partials [(m, s, t)]: thread k % 256 adds the rescaled partials k, k + 256, ..; fixed trees.
    VS: (V, S) forced from outside (mutant row0_VS)"""
    with np.errstate(all="ignore"):
        V = NEG
        for m, _, _ in parts:
            V = m if m > V else V
        if VS is not None:
            V = VS[0]
        ms, mt = [F(0)] * 256, [F(0)] * 256
        for k, (m, s, t) in enumerate(parts):
            ms[k % 256] = F(ms[k % 256] + _rescale_s(s, m, V))
            mt[k % 256] = F(mt[k % 256] + _rescale_t(t, s, m, V, mut))
        Ssum, T = _tree256(ms), _tree256(mt)
        if VS is not None:
            Ssum = VS[1]
        if not V > NEG:
            return float("nan"), (V, Ssum, T)
        Sdiv = Ssum
        if mut == "winner_partial_sum":
            Sdiv = next(_rescale_s(s, m, V) for m, s, _ in parts if m == V)
        logS = F(np.log(Ssum, dtype=F))
        H = F((-logS if mut == "log_sign" else logS) - F(T / Sdiv))
        return float(H), (V, Ssum, T)


def produce(kind, y, mut=None, cmp_max=None, z=None, M_pad=1):
    """one activation row through producer `kind`: the partials [(m, s, t)] it writes.  y [N] fp32: the summed values; cmp_max (mutant
    pen_compare_only): the values the maxima are taken on; z (mutant t_on_z): the perturbed values"""
    N = y.size
    sub, part, _, spp, n_parts, padded = SM.layout(kind, N)
    cols = np.arange(padded)
    pad_val = F(0) if kind == "mfma" else y[N - 1]
    yy = np.where(cols < N, y[np.minimum(cols, N - 1)], pad_val).astype(F)
    tt = yy if z is None else np.where(cols < N, z[np.minimum(cols, N - 1)], pad_val).astype(F)
    counted = (cols < N) | (mut == "ragged_twice" and kind != "mfma") | (mut == "cols_ge_N" and kind == "mfma")
    order = np.lexsort((cols, sub))
    bounds = np.flatnonzero(np.diff(sub[order])) + 1
    groups = dict((int(sub[o[0]]), o) for o in np.split(order, bounds))
    parts = []
    with np.errstate(all="ignore"):
        for p in range(n_parts):
            subs = []
            for w in range(spp):
                o = groups.get(p * spp + w if spp > 1 else p)
                if kind != "mfma":
                    m, s, t = NEG, F(0), F(0)
                    for n in ([] if o is None else o):
                        if not counted[n]:
                            continue
                        if z is None:
                            m, s, t = _add(yy[n], m, s, t, mut)
                        else:                                  # t_on_z: the sums on y as they should be, every term of t on the perturbed value
                            v = yy[n]
                            if v > m:
                                t = F(0) if s == 0 else F(F(t + F(F(m - v) * s)) * _exp(m - v))
                            m, s, _ = _add(v, m, s, F(0))
                            t = F(t + _term(tt[n], m))
                    if cmp_max is not None and o is not None:
                        live = [n for n in o if n < N]
                        m = F(max([cmp_max[n] for n in live] + [NEG]))
                    subs.append((m, s, t))
                    continue
                # MFMA wave: the maximum first (compares and the shuffle tree), then per lane the NJ = 2 columns j * 32 + r32, the xor tree
                live = [] if o is None else [n for n in o if n < N or mut == "cols_ge_N"]
                src = yy if cmp_max is None else np.where(cols < N, np.concatenate([cmp_max, np.zeros(padded - N, F)])[cols], pad_val).astype(F)
                v = F(max([src[n] for n in live] + [NEG]))
                base = (p * spp + w) * 64
                ls, lt = [], []
                for r in range(32):
                    a, b = F(0), F(0)
                    for j in range(2):
                        n = base + j * 32 + r
                        c = yy[n] if counted[n] else NEG
                        ct = tt[n] if counted[n] else NEG
                        a = F(a + (F(0) if c == NEG else _exp(c - v)))
                        b = F(b + _term(ct, v, mut))
                    ls.append(a)
                    lt.append(b)
                k = 1
                while k < 32:
                    ls = [F(ls[r] + ls[r ^ k]) for r in range(32)]
                    lt = [F(lt[r] + lt[r ^ k]) for r in range(32)]
                    k *= 2
                subs.append((v, ls[0], lt[0]))
            if mut == "rows_ge_M":       # the tile rows at or beyond M, which compute row M - 1 again (clamped), join its sums
                subs = [(m, F(s * F(M_pad)), F(t * F(M_pad))) for m, s, t in subs]
            parts.append(subs[0] if spp == 1 else _merge_waves(subs, mut))
    return parts


# ---------------------------------------------------------------------------------------------------------- cases
class Case(S.Case):
    """scores_ref.Case with the logit design of this file: heavy entries at gaps 0 (tie), 1/2, 1 and 5/2 below the row's top"""

    def __init__(self, base):
        super().__init__(base.kind, base.N, base.K, B=base.B, fmt=base.fmt, pen=base.pen, tie=base.tie, norm=False, seed=base.seed)
        self.id = self.id.replace("-norm", "")
        self.T = TEMPS[self.seed % 2]                          # of the sampled form of this case
        self.smp_seed = 0x5EED0000 + 31 * self.seed
        self.streams = [(5 * b + 3) % 8 for b in range(self.B)]
        self.draws = [7 + 3 * b for b in range(self.B)]

    @property
    def inv_t(self):
        return float(F(1.0) / F(self.T))

    def heavy_rows(self, b):
        h = dict(super().heavy_rows(b))
        N = self.N
        if N < 8:
            return h
        used = set(h.values())
        if self.kind == "rows":
            start = 4 * ((h["up"] // 4) + 1)                   # the next group: the next wave of the workgroup
        else:
            start = 64 + b if N > 70 else 1                    # the second wave of tile 0 / another unit
        n = next((n for n in list(range(start, N)) + list(range(start)) if n not in used), None)
        if n is not None:
            h["deep"] = n
            used.add(n)
        n = next((n for n in range(N - 2, -1, -1) if n not in used), None)      # beside the last valid column
        if n is not None:
            h["half"] = n
        return h

    @functools.lru_cache(maxsize=None)
    def logits(self):
        B, N = self.B, self.N
        tops = self.tops()
        L = S.background(B, N, tops, self.seed)
        flags = torch.zeros((8 if self.kind != "mfma" else B, N), dtype=torch.uint8) if self.pen else None
        rows = [(3 * b + 1) % (8 if self.kind != "mfma" else B) for b in range(B)] if self.pen else None
        g = torch.Generator().manual_seed(self.seed + 3)
        heavy = []
        for b in range(B):
            h = self.heavy_rows(b)
            T = tops[b]
            L[b, h["top"]] = T
            if "up" in h and h["up"] != h["top"]:
                L[b, h["up"]] = T - 0.5
            if "tail" in h and h["tail"] not in (h["top"], h.get("up")):
                L[b, h["tail"]] = T - 1 if not self.tie else T
            if self.tie and N > 1 and "tail" in h and h["tail"] == h["top"]:
                L[b, 0] = T
            if "deep" in h:
                L[b, h["deep"]] = T - 2.5
            if "half" in h:
                L[b, h["half"]] = T - 0.5
            keep = set(h.values()) | ({0} if self.tie else set())
            if self.pen:
                fr = flags[rows[b]]
                fr[torch.randint(0, N, (max(N // 16, 1),), generator=g)] = 1
                n = next((n for n in list(range(N // 2, N)) + list(range(N // 2)) if n not in keep), None)
                if n is not None:                             # a flagged row that carries weight exp(-1) after the penalty, far more before
                    fr[n] = 1
                    L[b, n] = (T - 1) * PEN if T - 1 >= 0 else (T - 1) / PEN
            heavy.append(keep)
        if self.pen:                                          # the designed heavy rows of b are not flagged, through whichever row's placement
            for b in range(B):
                for n in heavy[b]:
                    flags[rows[b], n] = 0
        return L, flags, rows

    # ---- y of the greedy (sampled = False) and the sampled form, float64 [B][N]
    def y(self, sampled):
        p = self.processed()
        return (p * self.inv_t if sampled else p).numpy()

    def reference_entropy(self, sampled):
        return reference(self.y(sampled))

    def noise(self, b):
        return SM.gumbel(self.smp_seed, self.streams[b], self.draws[b], np.arange(self.N)).astype(F)

    def restate(self, sampled=False, mut=None):
        """[(H, partials)] per row through the case's producer and the merge"""
        L, flags, rows = self.logits()
        out, VS0 = [], None
        for b in range(self.B):
            fr = None if flags is None else flags[rows[0 if mut == "wrong_flag_row" else b]]
            cmp_, sum_ = S._vals(L[b], fr, PEN, mut)
            sc = F(self.inv_t) if sampled else F(1)
            ys, yc = (sum_ * sc).astype(F), (cmp_ * sc).astype(F)
            z = (ys + self.noise(b)).astype(F) if mut == "t_on_z" else None
            pad = 32 - self.B + 1 if (mut == "rows_ge_M" and b == self.B - 1) else 1
            parts = produce(self.kind, ys, mut, yc if mut == "pen_compare_only" else None, z, pad)
            H, vst = merge(parts, mut, VS0 if (mut == "row0_VS" and b > 0) else None)
            if b == 0:
                VS0 = vst[:2]
            out.append((H, parts))
        return out


def rows_cases(big=True):
    return [Case(c) for c in S.rows_cases(big)]


def batched_cases():
    seen, out = set(), []
    for c in S.batched_cases():                                # (the fused-norm variants of scores_ref repeat a shape: the entropy forms have none)
        e = Case(c)
        if e.id not in seen:
            seen.add(e.id)
            out.append(e)
    return out


def mfma_cases():
    return [Case(c) for c in S.mfma_cases()]


def cpu_cases():
    return [Case(c) for c in S.cpu_cases()]


KIND_MUTANTS = {
    "rows": ("t_no_shift", "merge_no_shift", "empty_nan", "ragged_twice", "pen_compare_only", "winner_partial_sum", "t_on_z", "log_sign"),
    "batched": ("t_no_shift", "merge_no_shift", "empty_nan", "ragged_twice", "pen_compare_only", "wrong_flag_row", "winner_partial_sum", "row0_VS",
                "t_on_z", "log_sign"),
    "mfma": ("merge_no_shift", "empty_nan", "neginf_nan", "cols_ge_N", "rows_ge_M", "pen_compare_only", "wrong_flag_row", "winner_partial_sum",
             "row0_VS", "t_on_z", "log_sign"),
}


def moved(a, b):
    """|a - b|, infinite when exactly one of the two is NaN"""
    if math.isnan(a) or math.isnan(b):
        return 0.0 if math.isnan(a) and math.isnan(b) else float("inf")
    return abs(a - b)
