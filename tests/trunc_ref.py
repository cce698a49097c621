"""CPU case builder, float64 reference and fp32 restatement of truncated sampling (svln_sampling_truncation): truncate_partials_kernel of
misc.hip followed by the sampled final kernel on the 8-entry partial row it writes.  Test infrastructure, modelled on tests/topk_ref.py and
tests/sample_ref.py, whose Philox / Gumbel restatement it reuses.

The rule, for one head row with candidates (y, column) [n_part][c]  (c = 8: the lists of the EPI_SAMPLE_TOPK epilogues; c = 1: one
candidate per partial, as under an allowed list):

    1. the k' = min(top_k, listable) best pairs, y descending then column ascending (NaN, -inf and 0x7FFFFFFF are never listed);
    2. e_j = exp(y_j - y_0), c_j = c_{j-1} + e_j serially in fp32, total = c_{k'-1}; entry 0 is kept, entry j >= 1 iff top_p >= 1 or
       c_{j-1} < fl(top_p * total);
    3. token = argmax over the kept j of fl(y_j + G(seed, stream, draw + count, column_j)), lowest column on ties;
    4. score = log-softmax over the kept set at the token.

Exact inputs.  A test gives the kernel its candidates, so y is exact; the designed values are multiples of 1/8.  What is left to tolerance
is the noise (two hardware logarithms), the hardware exponentials of the prefix and the log-sum-exp.

Decisive gaps (tests/test_trunc_inputs.py asserts them for every case, so the GPU test skips nothing), each >= 100 x its GPU tolerance:
    * the two best perturbed values among the kept: tol_z = 2^-17 max(1, |G_a|, |G_b|) + 2^-22 max|z| (tests/sample_ref.py);
    * |c_{j-1} - top_p * total| for every j >= 1: tol_c = 2^-20 total -- eight exponentials of ~1 ulp (2^-23 relative) each and seven
      fp32 additions (2^-24 each) stay below 8 * 2^-23 = 2^-20 relative.  One planted EQUALITY is exempt: y_0 == y_1 with top_p = 1/2 and
      top_k = 2, where e = (1, 1), total = 2 and top_p * total = 1 are exact on any hardware (exp2(0) = 1): it is what tells `<` from `<=`;
    * y_{k-1} - y_k (the k-th against the (k+1)-th listable value): the candidates are given, so the GPU tolerance is 0 and any two
      different fp32 values are decisive; the cases keep >= 1/8 unless the tie is planted (then the lower column is listed).

Mutants: the restatement with one plausible kernel mistake each; tests/test_trunc_inputs.py proves that every one changes some case's
token or kept set or moves its score by >= 100 tolerances.  `score_all8` and `excluded_sum1` move the same scores by construction (the
first normalises over every selected entry in the final expression, the second leaves (part_max = y, part_sum = 1) on the excluded
entries of the partial row); an excluded entry whose part_max is -inf merges as 0 whatever its part_sum, so that spelling alone is
invisible in the outputs.
"""
import functools

import numpy as np

import sample_ref as SR

C = 8                       # entries of the truncated partial row (TOPK_C of kernels.h)
F = np.float32
NEG = F(-np.inf)
NONE = 0x7FFFFFFF
TOL = 2e-5                  # op-level bound on |logprob - float64| on the GPU (the project's bound for scored ops)
TOL_CPU = 2e-6              # the restatement against float64
G_BOUND = 2.0 ** -18        # |G - G64| <= G_BOUND max(1, |G|): the tested noise bound of tests/test_sample_gpu.py
KS = (1, 2, 5, 8)
PS = (1.0, 0.55, 2.0 ** -20)
N_PARTS = (1, 2, 5, 1024, 1025, 2048)
BS = (1, 2, 8, 32)
MUTANTS = ("k_plus_1", "k_minus_1", "ties_high", "nucleus_le", "mass_incl", "no_shortcut", "full_row_mass", "noise_by_position",
           "row0_stream", "count_ignored", "score_all8", "excluded_sum1", "stale_beyond")
LOG2E = F(1.4426950408889634)
LN2 = F(0.6931471805599453)
# what an earlier call left in the eight entries (mutant stale_beyond): a kept row whose perturbed values beat every case's
STALE = dict(pv=np.full(C, 100.0, F), pi=np.arange(7, 7 + C, dtype=np.int64), pr=np.full(C, 100.0, F), pm=np.full(C, 100.0, F), ps=np.ones(C, F))


def lse_exp(d):
    """lse_exp of common.h in fp32: exp2(fl(log2 e * d))"""
    return F(np.exp2(F(LOG2E * F(d))))


def listable(cv, ci):
    cv, ci = np.asarray(cv, dtype=F).reshape(-1), np.asarray(ci, dtype=np.int64).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (cv > NEG) & (ci != NONE)
    return cv[ok], ci[ok]


def select(cv, ci, k, ties_high=False):
    """the winners of the selection rounds: [(y, column)] of the k best listable pairs"""
    v, i = listable(cv, ci)
    order = np.lexsort((-i if ties_high else i, -v.astype(np.float64)))
    return [(F(v[o]), int(i[o])) for o in order[:k]]


# ---------------------------------------------------------------------------------------------------------- float64 reference
def reference_row(cv, ci, k, p, seed, stream, draw):
    """top-k, then top-p over the top-k set, then the renormalised softmax, from the definitions in float64.  Returns (kept columns,
    token, log-probability of the token, dict of the decisive gaps)"""
    top = select(cv, ci, k)
    if not top:
        return [], -1, float("nan"), dict(z=np.inf, c=np.inf, tol_c=0.0, tol_z=0.0, yk=np.inf)
    y = np.array([float(v) for v, _ in top])
    cols = np.array([i for _, i in top])
    e = np.exp(y - y[0])
    cum = np.cumsum(e)
    total = cum[-1]
    keep = [0] + [j for j in range(1, len(top)) if p >= 1.0 or cum[j - 1] < p * total]
    gap_c = min([abs(cum[j - 1] - p * total) for j in range(1, len(top))] + [np.inf]) if p < 1.0 else np.inf
    yk, ck = y[keep], cols[keep]
    g = SR.gumbel(seed, stream, draw, ck)
    z = yk + g
    order = np.lexsort((ck, -z))
    a = int(order[0])
    if len(keep) > 1:
        b = int(order[1])
        gap_z = float(z[a] - z[b])
        tol_z = 2.0 ** -17 * max(1.0, abs(g[a]), abs(g[b])) + 2.0 ** -22 * float(np.abs(z).max())
    else:
        gap_z, tol_z = np.inf, 0.0
    lp = float(yk[a] - (yk.max() + np.log(np.exp(yk - yk.max()).sum())))
    v_all, _ = listable(cv, ci)
    rest = np.sort(v_all.astype(np.float64))[::-1]
    gap_y = float(rest[k - 1] - rest[k]) if len(rest) > k else np.inf
    return [int(c) for c in ck], int(ck[a]), lp, dict(z=gap_z, tol_z=tol_z, c=float(gap_c), tol_c=2.0 ** -20 * float(total), yk=gap_y)


# ---------------------------------------------------------------------------------------------------------- fp32 restatement
def _tree_sum8(v):
    """block_sum_256 over entries in threads 0 .. 7 (zeros elsewhere): the fixed tree of the final kernels"""
    r = [F(x) for x in v]
    for s in (4, 2, 1):
        for t in range(s):
            r[t] = F(r[t] + r[t + s])
    return r[0]


def restate_row(cv, ci, k, p, seed, stream, draw, count=0, mut=None, row0=None, prev=None):
    """truncate_partials_kernel + the sampled final kernel for one row, in fp32.  row0 = (stream, draw) of row 0 (mutant row0_stream);
    prev: the five arrays an earlier call left in the row's eight entries (mutant stale_beyond; default STALE).  Returns a dict: kept
    [(y, column)], the partial row pv / pi / pr / pm / ps, the noise g (float64, per entry), token, score (fp32 as float)"""
    kk = k + 1 if mut == "k_plus_1" else k - 1 if mut == "k_minus_1" else k
    top = select(cv, ci, min(kk, C), ties_high=mut == "ties_high")
    n = len(top)
    kept = 0
    p32 = F(p)
    if n:
        e = [lse_exp(F(v - top[0][0])) for v, _ in top]
        cs, acc = [], F(0)
        for x in e:
            acc = F(acc + x)
            cs.append(acc)
        total = cs[-1]
        if mut == "full_row_mass":                       # the row's (V, S) instead of the top-k set's
            v_all, _ = listable(cv, ci)
            total = np.exp2((LOG2E * (v_all - top[0][0]).astype(F)).astype(F)).astype(F).sum(dtype=F)
        bound = F(p32 * total)
        kept = 1
        for j in range(1, n):
            before = cs[j] if mut == "mass_incl" else cs[j - 1]
            short = p32 >= F(1) and mut != "no_shortcut"
            if not (short or (before <= bound if mut == "nucleus_le" else before < bound)):
                break
            kept = j + 1
    if mut == "row0_stream" and row0 is not None:
        stream, draw = row0
    d = draw + (0 if mut == "count_ignored" else count)
    prev = prev or STALE
    pv, pi, pr, pm, ps = np.full(C, NEG, F), np.full(C, NONE, np.int64), np.zeros(C, F), np.full(C, NEG, F), np.zeros(C, F)
    g = np.zeros(C)
    for j in range(C):
        if j < kept:
            y, col = top[j]
            g[j] = float(SR.gumbel(seed, stream, d, np.array([j if mut == "noise_by_position" else col]))[0])
            pv[j], pi[j], pr[j], pm[j], ps[j] = F(y + F(g[j])), col, y, y, F(1)
        elif j < n and mut == "excluded_sum1":
            pm[j], ps[j] = top[j][0], F(1)
        elif j >= n and mut == "stale_beyond":
            pv[j], pi[j], pr[j], pm[j], ps[j] = prev["pv"][j], prev["pi"][j], prev["pr"][j], prev["pm"][j], prev["ps"][j]
    # the sampled final kernel on the eight partials
    tok, zbest, raw = NONE, NEG, F(0)
    for j in range(C):
        if pv[j] > zbest or (pv[j] == zbest and pi[j] < tok):
            zbest, tok, raw = pv[j], int(pi[j]), pr[j]
    if tok == NONE:
        token, score = -1, float("nan")
    else:
        V = F(np.max(pm))
        terms = [F(0) if ps[j] == 0 else F(ps[j] * lse_exp(F(pm[j] - V))) for j in range(C)]
        if mut == "score_all8":
            terms = [lse_exp(F(top[j][0] - V)) if j < n else F(0) for j in range(C)]
        S = _tree_sum8(terms)
        with np.errstate(divide="ignore"):
            score = float(F(F(raw - V) + F(-LN2 * F(np.log2(S)))))
        token = tok
    return dict(kept=top[:kept], pv=pv, pi=pi, pr=pr, pm=pm, ps=ps, g=g, token=token, score=score)


# ---------------------------------------------------------------------------------------------------------- cases
TOP = 12.0


class Case:
    """B rows of candidates [B][n_part][c] with one (top_k, top_p).  Row b uses streams[b], draws[b] (+ count: the op entry has no count,
    the GPU test passes draws + count); the seed is the first from the case's base for which every row keeps its decisive margin."""

    def __init__(self, name, cv, ci, k, p, base, count=0, planted_tie=False, planted_equality=False):
        self.name, self.k, self.p, self.base, self.count = name, k, float(p), base, count
        self.cv, self.ci = np.asarray(cv, dtype=F), np.asarray(ci, dtype=np.int32)
        self.B, self.n_part, self.c = self.cv.shape
        self.streams = [(5 * b + 3) % 8 for b in range(self.B)]
        self.draws = [7 + 3 * b + base % 5 for b in range(self.B)]
        self.planted_tie, self.planted_equality = planted_tie, planted_equality
        self.id = f"{name}-B{self.B}-n{self.n_part}-c{self.c}-k{k}-p{p:.3g}"

    def reference(self, seed=None):
        s = self.seed if seed is None else seed
        return [reference_row(self.cv[b], self.ci[b], self.k, self.p, s, self.streams[b], self.draws[b] + self.count) for b in range(self.B)]

    @property
    @functools.lru_cache(maxsize=None)
    def seed(self):
        s = 0x7C0000 + 977 * self.base
        while True:
            if all(g["z"] >= 100 * g["tol_z"] for _, _, _, g in self.reference(s)):
                return s
            s += 1

    def restate(self, mut=None):
        row0 = (self.streams[0], self.draws[0])
        return [restate_row(self.cv[b], self.ci[b], self.k, self.p, self.seed, self.streams[b], self.draws[b], self.count, mut, row0)
                for b in range(self.B)]


def design_row(n_part, c, values, rng, n_background=None, specials=0):
    """one row [n_part][c]: the designed `values` (descending list of y, duplicates = planted ties) on distinct random columns, a background
    20 .. 30 below the top, per-partial lists ordered as the epilogues write them and padded with (-inf, none); `specials` unlistable
    entries (NaN, -inf with no column) where there is room.  Fewer slots than values: the best ones stay (a one-partial row)."""
    slots = n_part * c
    cols = rng.permutation(3 * slots + 64)[:slots].astype(np.int64)
    n_bg = min(slots - min(len(values), slots), slots // 2 if n_background is None else n_background)
    vals = np.array(list(values)[:slots] + list(TOP - rng.integers(160, 241, size=n_bg) / 8.0), dtype=np.float64)
    n = len(vals)
    part = rng.permutation(slots)[:n] // c                  # distinct slots: no partial gets more than c
    order = np.lexsort((cols[:n], -vals, part))             # by partial, then y descending, then column ascending
    part, vals, ids = part[order], vals[order], cols[:n][order]
    first = np.searchsorted(part, part, side="left")        # rank inside the partial
    rank = np.arange(n) - first
    cv, ci = np.full((n_part, c), NEG, F), np.full((n_part, c), NONE, np.int32)
    cv[part, rank] = vals
    ci[part, rank] = ids
    used = np.bincount(part, minlength=n_part)
    for s in range(specials):                              # unlistable entries in the first free slot of random partials with room
        free = np.flatnonzero(used < c)
        if not len(free):
            break
        q = int(free[int(rng.integers(len(free)))])
        cv[q, used[q]] = F(np.nan) if s % 2 == 0 else NEG
        used[q] += 1
    return cv, ci


def _ladder(step, n=9, top=TOP):
    return [top - step * j for j in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    steps = (0.5, 0.25, 1.0, 2.0, 0.125)
    idx = 0
    for a, n_part in enumerate(N_PARTS):
        for c in (1, C):
            for i, k in enumerate(KS):
                for j, p in enumerate(PS):
                    B = BS[(a + i + j + (c == 1)) % 4]
                    rng = np.random.default_rng(1000 + idx)
                    rows = [design_row(n_part, c, _ladder(steps[(idx + b) % 5], top=TOP - (b % 3)), rng, specials=(idx + b) % 3) for b in range(B)]
                    out.append(Case("grid", [r[0] for r in rows], [r[1] for r in rows], k, p, idx, count=(idx % 4) * 2))
                    idx += 1
    rng = np.random.default_rng(7)
    # a planted tie on the k-th value (the lower column is listed), k = 1, 2, 5; the tied pair also heads the row
    for k in (1, 2, 5):
        vals = _ladder(0.5)
        vals[k] = vals[k - 1]
        rows = [design_row(5, C, vals, rng) for _ in range(2)]
        out.append(Case("tie-on-kth", [r[0] for r in rows], [r[1] for r in rows], k, 1.0, 900 + k, planted_tie=True))
    # the planted equality c_0 == top_p * total: y_0 == y_1, top_k = 2, top_p = 1/2 -> `<` keeps one entry, `<=` two
    rows = [design_row(5, C, [TOP, TOP] + _ladder(0.5, 7, TOP - 1), rng) for _ in range(2)]
    out.append(Case("equality", [r[0] for r in rows], [r[1] for r in rows], 2, 0.5, 910, planted_equality=True))
    # the absorbed tail: y_7 = y_0 - 40 adds nothing to c_6 in fp32; top_p = 1 keeps it all the same
    rows = [design_row(n, C, _ladder(0.5, 7) + [TOP - 40.0], rng, n_background=0) for n in (2, 1024)]
    out.append(Case("absorbed-tail", [rows[0][0]], [rows[0][1]], 8, 1.0, 920))
    out.append(Case("absorbed-tail", [rows[1][0]], [rows[1][1]], 8, 1.0, 921))
    # close values: the mass outside the top-k set is most of the row's (full_row_mass), k + 1 / k - 1 change the nucleus
    for k, p in ((2, 0.55), (5, 0.55), (5, 0.9), (8, 0.9), (2, 0.9)):
        rows = [design_row(5, C, _ladder(0.125, 12), rng) for _ in range(2)]
        out.append(Case("close", [r[0] for r in rows], [r[1] for r in rows], k, p, 930 + 10 * k + int(10 * p)))
    # fewer listable candidates than k (1, 3 and 0 of them), c of 1 and 8; all-NaN and all-padding rows
    for c in (1, C):
        r1 = design_row(5, c, [TOP], rng, n_background=0, specials=3)
        r3 = design_row(5, c, _ladder(0.5, 3), rng, n_background=0, specials=2)
        r0 = (np.full((5, c), np.nan, F), np.full((5, c), NONE, np.int32))
        rp = (np.full((5, c), NEG, F), np.full((5, c), NONE, np.int32))
        for k, p in ((8, 1.0), (5, 0.55), (2, 1.0)):
            out.append(Case("short", [r1[0], r3[0], r0[0], rp[0]], [r1[1], r3[1], r0[1], rp[1]], k, p, 950 + k + c))
    return out


# ---------------------------------------------------------------------------------------------------------- distribution
def sample_many(y, cols, k, p, seed, stream, n_draws):
    """the restated pick, vectorised over draws 0 .. n_draws - 1, for one row of listable (y, column) pairs -> (kept columns, counts)"""
    r = restate_row(np.asarray(y, dtype=F).reshape(1, -1), np.asarray(cols).reshape(1, -1), k, p, seed, stream, 0)
    ky = np.array([v for v, _ in r["kept"]], dtype=F)
    kc = np.array([i for _, i in r["kept"]], dtype=np.int64)
    draws = np.arange(n_draws, dtype=np.int64)[:, None]
    g = SR.gumbel(seed, stream, draws, kc[None, :])
    z = (ky[None, :] + g.astype(F)).astype(F)
    order = np.argsort(kc)                                   # lowest column on ties: argmax over columns ascending takes the first
    win = order[np.argmax(z[:, order], axis=1)]
    return kc, np.bincount(win, minlength=len(kc))
