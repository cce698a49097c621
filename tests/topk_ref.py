"""CPU case builder, float64 reference and fp32 restatement of the top-k log-probabilities (svln_top_logprobs): the EPI_ARGMAX_LSE_TOPK /
EPI_SAMPLE_TOPK siblings of gemv_rows_kernel (gemv.hip), the subset form (one candidate per allowed id) and topk_merge_kernel (misc.hip).
Test infrastructure, modelled on tests/scores_ref.py and tests/sample_ref.py, whose designed operands, partial layout and noise it reuses.

    y_n = x_n (greedy) or fl(x_n * inv_t) (sampled; never y + G), x_n the processed fp32 logit (after the repetition penalty)
    list = the k columns with the largest y, y descending then column ascending; NaN and -inf never listed; padding (-1, -inf)
    logprob_j = (y_j - V) - log S, (V, S) the merge of the scored kernels

Exact inputs.  Every logit is DESIGNED (scores_ref.design_x / design_w): a multiple of 1/2 that the fp32 dot product gives bit for bit in
any summation order; penalty 2 and inv_t of 1, 1/2, 2 keep it exact.  So ids and the order of a list are exact, planted ties are exactly
0 apart and every other gap a case relies on is >= 1/8 (>= 100 x TOL); what is left to tolerance is log S alone.

Scheme restated.  Wave (sub-partial) lists by INSERTION in the wave's column order -- the kernel's one compare against entry 7, the
shift of the displaced entries -- then the workgroup's list by rank among the waves' entries, then the merge by k rounds of "best pair
strictly behind the previous winner".  Mutants: one plausible mistake each; tests/test_topk_inputs.py proves that every one changes an id
or moves a value by >= 100 x TOL on some case while the correct restatement equals the float64 reference.
"""
import functools

import numpy as np
import torch

import gemv_ref as G
import sample_ref as R
import scores_ref as S

TOL = S.TOL                 # op-level bound on |logprob - float64 reference| on the GPU (the project's bound for scored ops)
TOL_CPU = 2e-6              # the restatement against float64 (the bound tests/test_scores_inputs.py uses)
PEN = S.PEN
C = 8                       # candidates per partial (TOPK_C of kernels.h)
F = np.float32
NEG = F(-np.inf)
NONE = 0x7FFFFFFF
KS = (1, 2, 5, 8)
MUTANTS = ("best_only", "ties_high", "drop_displaced", "ragged_twice", "cols_ge_N", "rows_ge_M", "raw_listed", "z_listed", "merge_first_parts",
           "stale_beyond", "logS_winner_partial", "row0_cand", "row0_VS", "nan_listed", "ninf_listed", "k_minus_1", "k_plus_1")


# ---------------------------------------------------------------------------------------------------------- float64 reference
def processed64(x, flags_row, pen):
    x = x.astype(np.float64)
    return x if flags_row is None else np.where(flags_row.astype(bool), np.where(x < 0, x * pen, x / pen), x)


def reference(x, flags_row, pen, inv_t, k, allowed=None):
    """(ids [k] (-1 padding), float64 log-probabilities [k] (-inf padding; NaN when the row holds a NaN), gaps): x [N] raw logits; with
    `allowed` the list is over those columns only.  gaps: the adjacent differences of the k + 1 best y (those the order relies on)"""
    y = processed64(x, flags_row, pen) * float(F(inv_t))
    cols = np.arange(x.size) if allowed is None else np.asarray(allowed)
    yy = y[cols]
    ok = np.isfinite(yy) | (yy == np.inf)
    order = sorted((int(c) for c, o in zip(cols, ok) if o), key=lambda c: (-y[c], c))
    fin = yy[yy > -np.inf]
    if np.isnan(yy).any():
        lse = float("nan")
    elif fin.size == 0:
        lse = float("nan")
    else:
        lse = float(fin.max() + np.log(np.exp(fin - fin.max()).sum()))
    ids = order[:k] + [-1] * (k - len(order[:k]))
    lps = [float(y[c] - lse) if c >= 0 else float("-inf") for c in ids]
    best = [y[c] for c in order[:k + 1]]
    return ids, lps, [a - b for a, b in zip(best, best[1:])]


# ---------------------------------------------------------------------------------------------------------- fp32 restatement
def _insert(lst, v, i, mut):
    """tk_insert of gemv_rows_kernel: v joins the wave's list `lst` of C (value, column) pairs when it beats entry C - 1"""
    thr = lst[C - 1][0]
    if mut == "nan_listed" and np.isnan(v):
        pos = 0
    elif mut == "ninf_listed" and v == NEG and lst[C - 1][1] == NONE:
        pos = next(p for p in range(C) if lst[p][1] == NONE)
    elif mut == "ties_high":
        if not v >= thr or v == NEG:
            return
        pos = sum(1 for a, _ in lst if a > v)
    else:
        if not v > thr:
            return
        pos = sum(1 for a, _ in lst if a >= v)
    if mut == "drop_displaced":
        lst[pos] = (v, i)
    else:
        lst.insert(pos, (v, i))
        lst.pop()


def _key(mut):
    return (lambda e: (-e[0] if not np.isnan(e[0]) else -np.inf, -e[1])) if mut == "ties_high" else \
           (lambda e: (-e[0] if not np.isnan(e[0]) else -np.inf, e[1]))


def _row_values(kind, x, flags_row, pen, inv_t, sampled, seed, stream, draw, mut):
    """(y listed, y summed, z compared, live, layout) over the padded columns of producer `kind`"""
    N = x.size
    sub, part, local, spp, n_parts, padded = R.layout(kind, N)
    cols = np.arange(padded)
    raw = np.where(cols < N, x[np.minimum(cols, N - 1)], x[N - 1] if kind != "mfma" else 0.0).astype(F)
    fl = np.zeros(padded, dtype=bool)
    if flags_row is not None:
        fl[:N] = flags_row.astype(bool)
        if kind != "mfma":
            fl[N:] = fl[N - 1]
    with np.errstate(all="ignore"):
        p = np.where(fl, np.where(raw < 0, raw * F(pen), raw / F(pen)), raw).astype(F)
        y = (p * F(inv_t)).astype(F) if sampled else p
        z = (y + R.gumbel(seed, stream, draw, cols).astype(F)).astype(F) if sampled else y
        listed = y
        if mut == "raw_listed":
            listed = (raw * F(inv_t)).astype(F) if sampled else raw
        if mut == "z_listed":
            listed = z
    return listed, y, z, cols < N, (sub, part, spp, n_parts, padded)


def _lse_parts(y, z, live, sub, spp, n_parts):
    """the scored / sampled partials [(best z, its column, its y, max y, sum exp(y - max))] per workgroup, as sample_ref.restate_row
    builds them (the greedy form is the same with z = y)"""
    order = np.lexsort((np.arange(sub.size), sub))
    bounds = np.flatnonzero(np.diff(sub[order])) + 1
    groups = dict((int(sub[o[0]]), o) for o in np.split(order, bounds))
    parts = []
    with np.errstate(all="ignore"):
        for p in range(n_parts):
            subs = []
            for s in range(spp):
                o = groups.get(p * spp + s if spp > 1 else p)
                o = None if o is None else o[live[o]]
                if o is None or not o.size:
                    subs.append((NEG, NONE, NEG, NEG, F(0)))
                    continue
                zz = np.where(np.isnan(z[o]), NEG, z[o])
                j = int(np.argmax(zz))
                bz, bi, br = (zz[j], int(o[j]), y[o[j]]) if zz[j] > NEG else (NEG, NONE, NEG)
                m = F(np.fmax.reduce(y[o]))
                sm = F(np.exp((y[o] - m).astype(np.float64))[~(y[o] == NEG)].sum()) if m > NEG else F(0)
                if np.isnan(y[o]).any():
                    sm = F(np.nan)
                subs.append((bz, bi, br, m, sm))
            parts.append(R._merge(subs, None))
    return parts


def _final_sum(parts, V):
    """S of the final kernels (block_sum_256): thread t adds the rescaled sums of partials t, t + 256, ..; a fixed tree over the threads"""
    mine = [F(0)] * 256
    with np.errstate(all="ignore"):
        for j, (_, _, _, m, s) in enumerate(parts):
            mine[j % 256] = F(mine[j % 256] + R._rescale(s, m, V))
        w = 128
        while w:
            for t in range(w):
                mine[t] = F(mine[t] + mine[t + w])
            w //= 2
    return mine[0]


def _merge_lists(cands, n_read, k, mut):
    """topk_merge_kernel's k rounds over the first n_read partials' candidates -> [(value, column)] of length k (padding (-inf, NONE))"""
    pool = [e for part in cands[:n_read] for e in part]
    if mut not in ("nan_listed", "ninf_listed"):
        pool = [e for e in pool if e[0] > NEG and e[1] != NONE]
    else:
        pool = [e for e in pool if e[1] != NONE]
    pool.sort(key=_key(mut))
    out = pool[:k]
    return out + [(NEG, NONE)] * (k - len(out))


def _finish(winners, V, S_, sampled, k, mut):
    with np.errstate(all="ignore"):
        lp = F(-np.log(S_, dtype=F))
        ids, lps = [], []
        for v, i in winners:
            if i == NONE:
                ids.append(-1); lps.append(float("-inf"))
            else:
                ids.append(int(i))
                lps.append(float(F(F(v - V) + lp)) if sampled else float(-F(F(-lp) - F(v - V))))
    n = k - 1 if mut == "k_minus_1" else k
    return ids[:n] + [-7] * (k - n), lps[:n] + [float("nan")] * (k - n)


def restate(kind, x, flags_row=None, pen=PEN, inv_t=1.0, sampled=False, seed=0, stream=0, draw=0, k=C, mut=None, pad_rows=0, VS=None):
    """one activation row through producer `kind` ("rows", "batched", "mfma"), its final kernel and the merge.  pad_rows (mutant rows_ge_M,
    the last row of an MFMA case): the tile rows beyond M, which compute this row again; VS (mutant row0_VS): another row's (V, S).  Returns a dict: token, score (fp32 as float),
    cand [n_parts][C] (value, column), ids [k], logprobs [k], n_parts"""
    N = x.size
    listed, y, z, live, (sub, part, spp, n_parts, padded) = _row_values(kind, x, flags_row, pen, inv_t, sampled, seed, stream, draw, mut)
    parts = _lse_parts(y, z, live, sub, spp, n_parts)
    tz, ti, traw, V, _ = R._merge(parts, None)
    S_ = _final_sum(parts, V)
    # ---- candidates: wave lists by insertion in the wave's column order, the workgroup's list by rank
    waves = {}
    for n in range(padded):
        if n >= N and not (mut == "ragged_twice" and kind != "mfma") and not (mut == "cols_ge_N" and kind == "mfma"):
            continue
        lst = waves.setdefault(int(sub[n]), [(NEG, NONE)] * C)
        for _ in range(1 + (pad_rows if mut == "rows_ge_M" else 0)):
            _insert(lst, listed[n], n if kind == "mfma" else min(n, N - 1), mut)
    cands = []
    for p in range(n_parts):
        ent = [e for s in range(spp) for e in waves.get(p * spp + s if spp > 1 else p, [(NEG, NONE)] * C)]
        ent.sort(key=_key(mut))
        ent = ent[:C]
        if mut == "best_only":
            ent = ent[:1] + [(NEG, NONE)] * (C - 1)
        cands.append(ent)
    n_read = n_parts
    if mut == "merge_first_parts":
        n_read = max(n_parts - 1, 1) if n_parts <= 256 else 256
    if mut == "stale_beyond":              # one partial more than the launch wrote: what an earlier, larger launch left there
        cands = cands + [[(F(V + F(1)), 0)] + [(NEG, NONE)] * (C - 1)]
        n_read = n_parts + 1
    if mut == "logS_winner_partial":
        S_ = next(s for _, _, _, m, s in parts if m == V)
    kk = k + 1 if mut == "k_plus_1" else k
    winners = _merge_lists(cands, n_read, kk, mut)
    Vf, Sf = VS if VS is not None else (V, S_)
    ids, lps = _finish(winners, Vf, Sf, sampled, kk, mut)
    with np.errstate(all="ignore"):
        lp0 = F(-np.log(S_, dtype=F))            # the greedy score is -log S itself (-0 when S == 1), the sampled one (raw - V) + it
        score = float("nan") if ti == NONE else float(F(F(traw - V) + lp0)) if sampled else float(lp0)
    return {"token": -1 if ti == NONE else int(ti), "score": score, "cand": cands[:n_parts], "ids": ids, "logprobs": lps, "n_parts": n_parts,
            "VS": (V, S_), "part_val": [F(q[0]) for q in parts], "part_idx": [int(q[1]) for q in parts], "part_max": [F(q[3]) for q in parts]}


def restate_subset(x, allowed, flags_row=None, pen=PEN, inv_t=1.0, sampled=False, seed=0, stream=0, draw=0, k=C, mut=None):
    """the subset form: partial j is allowed id a_j alone -- (y, a_j), or (., NONE) for a NaN / -inf value -- and the merge runs with one
    candidate per partial"""
    allowed = list(allowed)
    with np.errstate(all="ignore"):
        raw = x[allowed].astype(F)
        fl = np.zeros(len(allowed), dtype=bool) if flags_row is None else flags_row[allowed].astype(bool)
        p = np.where(fl, np.where(raw < 0, raw * F(pen), raw / F(pen)), raw).astype(F)
        y = (p * F(inv_t)).astype(F) if sampled else p
        z = (y + R.gumbel(seed, stream, draw, np.asarray(allowed)).astype(F)).astype(F) if sampled else y
        listed = z if mut == "z_listed" else ((raw * F(inv_t)).astype(F) if sampled else raw) if mut == "raw_listed" else y
        own = [a if (v > NEG) else NONE for a, v in zip(allowed, z)]
        if mut in ("nan_listed", "ninf_listed"):
            own = list(allowed)
        V = F(np.fmax.reduce(y)) if len(allowed) else NEG
        S_ = F(np.exp((y - V).astype(np.float64))[~(y == NEG)].sum())
        if np.isnan(y).any():
            S_ = F(np.nan)
    cands = [[(v, o)] for v, o in zip(listed, own)]
    n_read = len(cands)
    if mut == "merge_first_parts":
        n_read = max(n_read - 1, 1)
    if mut == "stale_beyond":
        cands = cands + [[(F(V + F(1)), 0)]]
        n_read += 1
    if mut == "logS_winner_partial":
        S_ = F(1)
    kk = k + 1 if mut == "k_plus_1" else k
    winners = _merge_lists(cands, n_read, kk, mut)
    ids, lps = _finish(winners, V, S_, sampled, kk, mut)
    return {"cand": cands[:len(allowed)], "ids": ids, "logprobs": lps, "n_parts": len(allowed)}


# ---------------------------------------------------------------------------------------------------------- cases
TOP = 12.0


def _background(N, seed):
    g = torch.Generator().manual_seed(seed + 2)
    return (TOP - torch.randint(40, 61, (N,), generator=g).double() / 2).numpy()       # 20 .. 30 below the top, in halves


class Case:
    """One head row of N columns.  plant: {column: logit} over the background; flags: columns with the penalty flag; special:
    {column: nan / -inf}.  sampled cases carry T and search a seed whose sampled id differs from entry 0 (want_differ)."""

    def __init__(self, name, N, plant, K=192, fmt="plain-fp32", flags=(), special=None, T=None, k=C, seed=0, kind="rows", allowed=None,
                 want_differ=False):
        self.name, self.N, self.K, self.fmt, self.k, self.base, self.kind = name, N, K, fmt, k, seed, kind
        self.plant, self.flag_cols, self.special, self.T, self.allowed, self.want_differ = dict(plant), tuple(flags), dict(special or {}), T, allowed, want_differ
        self.id = f"{kind}-{name}-{fmt}-N{N}-K{K}-k{k}" + (f"-T{T}" if T else "")
        self.stream, self.draw = 3, 7 + seed

    @property
    def dtype(self):
        return G.DTYPE[self.fmt]

    @property
    def sampled(self):
        return self.T is not None

    @property
    def inv_t(self):
        return float(F(1.0) / F(self.T)) if self.sampled else 1.0

    @functools.lru_cache(maxsize=None)
    def logits(self):
        """(designed raw logits [N] float64 -- what the weights spell --, the logits the kernel sees (NaN / -inf planted), flag row)"""
        L = _background(self.N, self.base)
        for c, v in self.plant.items():
            L[c] = v
        x = L.copy()
        for c, v in self.special.items():
            x[c] = v
        fr = None
        if self.flag_cols:
            fr = np.zeros(self.N, dtype=np.uint8)
            fr[list(self.flag_cols)] = 1
        return L, x, fr

    def operands(self):
        """(x [1][K] float64, W [N][K] exact values); a special column is spelled by one NaN / -inf weight against x = 2"""
        L, _, _ = self.logits()
        W = S.design_w(torch.from_numpy(L)[None], self.K, self.base, torch.float32 if self.fmt == "plain-fp32" else torch.bfloat16)
        for c, v in self.special.items():
            assert self.fmt.startswith("plain")
            W[c, 0] = float(v)
        return S.design_x(1, self.K, self.base), W

    def _sampled_token(self, seed):
        _, x, fr = self.logits()
        xs = x if self.allowed is None else np.where(np.isin(np.arange(self.N), self.allowed), x, -np.inf)
        return R.reference_row(xs, fr, PEN, self.inv_t, seed, self.stream, self.draw)

    @property
    @functools.lru_cache(maxsize=None)
    def seed(self):
        if not self.sampled:
            return 0
        s = 0x70B50000 + 131 * self.base
        first = self.reference()[0][0]
        while True:
            tok, _, margin, tol = self._sampled_token(s)
            if margin >= 100 * tol and (not self.want_differ or tok != first):
                return s
            s += 1

    def reference(self, k=None):
        _, x, fr = self.logits()
        return reference(x, fr, PEN, self.inv_t, k or self.k, self.allowed)

    def restate(self, mut=None, k=None):
        _, x, fr = self.logits()
        kw = dict(flags_row=fr, pen=PEN, inv_t=self.inv_t, sampled=self.sampled, seed=self.seed, stream=self.stream, draw=self.draw,
                  k=k or self.k, mut=mut)
        if self.allowed is not None:
            return restate_subset(x, self.allowed, **kw)
        return restate(self.kind, x, **kw)


def _wave_cols(N, wave, count):
    """the first `count` columns of wave `wave` of the rows kernel, in the wave's order"""
    sub = R.layout("rows", N)[0]
    return [int(n) for n in np.flatnonzero(sub[:N] == wave)[:count]]


def _desc(cols, top=TOP, step=0.5):
    return {c: top - step * j for j, c in enumerate(cols)}


def rows_cases():
    out = []
    BIG = 20497                  # gemv_grid = 1024: waves 0 .. 1028 take two groups (8 columns; wave 1028's second group is the ragged tail)
    w8 = _wave_cols(BIG, 17, 8)
    # all 8 winners (and a ninth just below) inside one wave, arriving in descending, ascending and mixed order
    out.append(Case("one-wave-desc", BIG, _desc(w8), seed=1))
    out.append(Case("one-wave-asc", BIG, _desc(w8[::-1]), seed=2, fmt="plain-bf16"))
    out.append(Case("one-wave-mixed", BIG, _desc([w8[k] for k in (3, 0, 6, 1, 7, 2, 5, 4)]), seed=3, k=5))
    # nine good columns in one wave of 8 .. 12: the ninth must not displace, the displaced entries must move down
    w12 = _wave_cols(50000, 5, 12)
    out.append(Case("one-wave-nine", 50000, _desc([w12[k] for k in (8, 2, 10, 0, 4, 6, 1, 9, 3)]), seed=4))
    # one winner per workgroup (wave 0 of workgroups 3, 6, ..) and per wave of one workgroup
    out.append(Case("one-per-partial", BIG, _desc([_wave_cols(BIG, 4 * (3 * j + 3), 1)[0] for j in range(9)]), seed=5))
    out.append(Case("one-per-wave", BIG, _desc([_wave_cols(BIG, 40 + (j % 4), 2)[j // 4] for j in range(8)]), seed=6, fmt="plain-bf16"))
    # ties: inside a wave, across waves of a workgroup, across workgroups -- the lowest id first; the last listed entry is a tie too
    tie = {w8[5]: TOP, w8[1]: TOP, _wave_cols(BIG, 18, 1)[0]: TOP, _wave_cols(BIG, 400, 1)[0]: TOP, 3: TOP - 1, 20000: TOP - 1,
           w8[7]: TOP - 1, w8[0]: TOP - 1, 9000: TOP - 1, 9001: TOP - 1}
    for k in KS:
        out.append(Case("ties", BIG, tie, seed=7, k=k))
    # ragged tails, N % 4 of 0 .. 3, partials with fewer than 8 columns, waves without a column, fewer than k listable
    for N in (1, 2, 3, 4, 5, 7, 13, 16, 113, 114, 115, 116):
        plant = _desc(list(dict.fromkeys(c for c in (N - 1, 0, N // 2, N - 2, 1, N // 3) if 0 <= c < N)))
        out.append(Case("ragged", N, plant, seed=10 + N, fmt="plain-bf16" if N % 2 else "plain-fp32", k=8 if N < 16 else 5))
    out.append(Case("ragged-tail-top", BIG, {BIG - 1: TOP, BIG - 2: TOP - 0.5, 0: TOP - 1}, seed=30, k=2))
    # penalty flags that reorder the list (12 -> 6, -4 -> -8), flags on the ragged tail
    out.append(Case("penalty", 115, {3: 12.0, 40: 11.0, 77: 10.0, 114: 9.0, 5: 8.0, 6: 5.5, 90: -4.0}, flags=(3, 77, 114, 90, 10, 11), seed=31))
    out.append(Case("penalty-big", BIG, _desc(w8), flags=(w8[0], w8[3], BIG - 1, 100), seed=32, fmt="plain-bf16", k=5))
    # NaN and -inf logits: never listed, even when the row has fewer than k others
    out.append(Case("ninf", 7, {0: 12.0, 3: 11.0}, special={2: -np.inf, 6: -np.inf}, seed=33))
    out.append(Case("nan", 7, {0: 12.0, 3: 11.0}, special={5: np.nan}, seed=34, k=8))
    out.append(Case("ninf-big", BIG, _desc(w8), special={w8[2]: -np.inf}, seed=35))
    # the weight formats of the single-env head
    for fmt in ("e4m3", "mxfp4"):
        out.append(Case("formats", 1301, _desc([1300, 7, 640, 641, 3, 1299, 100, 99, 650]), K=G.k_ladder(fmt)[0], fmt=fmt, seed=36, k=8))
    # sampled: inv_t of 1, 1/2, 2; the sampled id differs from entry 0
    for j, T in enumerate((1.0, 2.0, 0.5)):
        out.append(Case("sampled", 115, _desc([114, 3, 40, 77, 5, 6, 90, 91, 20], step=0.5), T=T, seed=40 + j, want_differ=True,
                        flags=(3, 40) if j == 1 else ()))
        out.append(Case("sampled-big", BIG, _desc(w8), T=T, seed=45 + j, want_differ=True, fmt="plain-bf16", k=5))
    return out


def subset_cases():
    """the subset form: n_allowed of 1, 3, 8, 9, 256 in a vocabulary of 1301; k above and below n_allowed; a -inf member"""
    out = []
    N = 1301
    g = np.random.default_rng(5)
    for j, n in enumerate((1, 3, 8, 9, 256)):
        allowed = sorted(int(a) for a in g.choice(N, size=n, replace=False))
        plant = _desc(allowed[::-1][:9] if j % 2 else allowed[:9])
        plant[next(c for c in range(N) if c not in allowed)] = TOP + 5             # the best column of the vocabulary is not allowed
        for k in (8, 2):
            out.append(Case("subset", N, plant, seed=60 + j, allowed=allowed, k=k, kind="subset", fmt="plain-bf16" if j % 2 else "plain-fp32"))
    allowed = [5, 9, 700, 1300]
    out.append(Case("subset-ninf", N, kind="subset", plant= {5: 12.0, 9: 11.0, 1300: 12.0}, special={700: -np.inf}, seed=70, allowed=allowed, k=8))
    out.append(Case("subset-sampled", N, kind="subset", plant= _desc([5, 9, 700, 1300]), seed=71, allowed=allowed, k=3, T=2.0, want_differ=True))
    out.append(Case("subset-penalty", N, kind="subset", plant= {5: 12.0, 9: 11.0, 700: 10.0, 1300: 9.0}, flags=(5, 700), seed=72, allowed=allowed, k=4))
    return out


class BatchCase:
    """B head rows of one product through producer `kind` ("batched": B of 1, 2, 4, 8; "mfma": M = B <= 32).  Row b is a Case of its own
    (its plant, flag row pen_rows[b] = B - 1 - b, stream and draw); the operands spell all rows at once."""

    def __init__(self, kind, rows, name):
        self.kind, self.rows, self.B, self.name = kind, rows, len(rows), name
        c = rows[0]
        self.N, self.K, self.fmt, self.k, self.base, self.T = c.N, c.K, c.fmt, c.k, c.base, c.T
        self.id = f"{kind}-{name}-{c.fmt}-B{self.B}-N{c.N}-K{c.K}-k{c.k}" + (f"-T{c.T}" if c.T else "")
        self.streams = [(5 * b + 3) % 8 for b in range(self.B)]
        self.draws = [7 + 3 * b for b in range(self.B)]
        for b, r in enumerate(rows):
            r.stream, r.draw = self.streams[b], self.draws[b]
            r.seed_of = self
        self.pen_rows = [self.B - 1 - b for b in range(self.B)]
        self.special = rows[0].special

    dtype = property(lambda self: G.DTYPE[self.fmt])
    sampled = property(lambda self: self.T is not None)

    @property
    @functools.lru_cache(maxsize=None)
    def seed(self):
        """one seed for the product: every row's sampled id keeps its margin, and row 0's differs from its entry 0"""
        if not self.sampled:
            return 0
        s = 0x70B60000 + 131 * self.base
        first = self.rows[0].reference()[0][0]
        while True:
            toks = [r._sampled_token(s) for r in self.rows]
            if all(m >= 100 * t for _, _, m, t in toks) and toks[0][0] != first:
                return s
            s += 1

    def flags(self):
        """(flags [B][N] uint8 with row pen_rows[b] = row b's flags, pen_rows) or (None, None)"""
        if not any(r.flag_cols for r in self.rows):
            return None, None
        f = np.zeros((self.B, self.N), dtype=np.uint8)
        for b, r in enumerate(self.rows):
            f[self.pen_rows[b], list(r.flag_cols)] = 1
        return f, self.pen_rows

    def operands(self):
        L = np.stack([r.logits()[0] for r in self.rows])
        W = S.design_w(torch.from_numpy(L), self.K, self.base, torch.float32 if self.fmt == "plain-fp32" else torch.bfloat16)
        for c, v in self.special.items():
            assert self.B == 1
            W[c, 0] = float(v)
        return S.design_x(self.B, self.K, self.base), W

    def reference(self, k=None):
        return [r.reference(k) for r in self.rows]

    def restate(self, mut=None, k=None):
        out = []
        for b, r in enumerate(self.rows):
            _, x, fr = r.logits()
            kw = dict(flags_row=fr, pen=PEN, inv_t=r.inv_t, sampled=self.sampled, seed=self.seed, stream=self.streams[b], draw=self.draws[b],
                      k=k or self.k, mut=mut)
            if mut == "rows_ge_M" and b == self.B - 1:
                kw["pad_rows"] = 1
            if mut == "row0_VS" and b:
                kw["VS"] = out[0]["VS"]
            out.append(out[0] if (mut == "row0_cand" and b) else restate(self.kind, x, **kw))
        return out


def _batch_rows(kind, N, B, K, fmt, k, seed, T=None, pen=False, special=None):
    """row b's nine planted columns: a tile's first and last column, the next tile's first, N - 1 and others, rotated by b"""
    cols = list(dict.fromkeys(c for c in (0, 127, 128, N - 1, N // 2, 255, 256, N - 2, 5, 64, 63, N // 3, 1) if 0 <= c < N))[:9]
    rows = []
    for b in range(B):
        rot = cols[b % len(cols):] + cols[:b % len(cols)]
        plant = _desc(rot, top=TOP - (b % 3))
        if b % 4 == 3 and len(rot) > 2:
            plant[rot[1]] = plant[rot[0]]                     # a planted tie: the lowest id first
        flags = (rot[0], rot[min(2, len(rot) - 1)]) if pen and b % 2 == 0 else ()
        rows.append(Case(f"r{b}", N, plant, K=K, fmt=fmt, flags=flags, special=special if b == 0 else None, T=T, k=k, seed=seed + b, kind=kind))
    return rows


def batched_cases():
    out = []
    for i, B in enumerate((1, 2, 4, 8)):
        for j, N in enumerate((5, 115, 8193 + i)):             # one unit per workgroup; 2049 .. units over 2048 workgroups: some loop twice
            fmt = "plain-bf16" if (i + j) % 2 else "plain-fp32"
            out.append(BatchCase("batched", _batch_rows("batched", N, B, 192, fmt, (8, 5, 2, 1)[(i + j) % 4], 200 + 10 * i + j, pen=j == 1), "greedy"))
        out.append(BatchCase("batched", _batch_rows("batched", 115, B, 192, "plain-fp32", 8, 260 + i, T=(1.0, 2.0, 0.5, 2.0)[i], pen=i == 2), "sampled"))
    out.append(BatchCase("batched", _batch_rows("batched", 7, 1, 192, "plain-fp32", 8, 280, special={3: -np.inf, 6: np.nan}), "special"))
    return out


def mfma_cases():
    out = []
    for i, M in enumerate((3, 4, 5, 8, 17, 32)):
        for j, N in enumerate((127, 128, 129, 257, 391)):
            if (i + j) % 2 and M not in (3, 32):                # every M x two or three N, every N x three or more M
                continue
            fmt = "plain-bf16" if (i + j) % 3 == 0 else "plain-fp32"
            out.append(BatchCase("mfma", _batch_rows("mfma", N, M, 576, fmt, (8, 5, 2, 1)[(i + j) % 4], 300 + 10 * i + j, pen=j in (1, 3)), "greedy"))
    for i, (M, N) in enumerate(((3, 129), (8, 391), (32, 257))):
        out.append(BatchCase("mfma", _batch_rows("mfma", N, M, 576, "plain-fp32", 8, 380 + i, T=(1.0, 0.5, 2.0)[i], pen=i == 1), "sampled"))
    out.append(BatchCase("mfma", _batch_rows("mfma", 130, 1, 576, "plain-fp32", 8, 390, special={3: -np.inf, 129: np.nan}), "special"))
    out.append(BatchCase("mfma", _batch_rows("mfma", 7, 1, 576, "plain-fp32", 8, 392, special={2: -np.inf, 5: -np.inf}), "special"))
    rows = _batch_rows("mfma", 129, 4, 576, "plain-fp32", 8, 395)         # three winners only: ranks 4 .. 8 are background below zero, where
    for r in rows:                                                        # a counted pad column (logit 0) of the last tile would be listed
        r.plant = dict(list(r.plant.items())[:3])
    out.append(BatchCase("mfma", rows, "below-zero"))
    return out


def all_cases():
    return rows_cases() + subset_cases()


def all_batch_cases():
    return batched_cases() + mfma_cases()


KIND_MUTANTS = {
    "rows": ("best_only", "ties_high", "drop_displaced", "ragged_twice", "raw_listed", "z_listed", "merge_first_parts", "stale_beyond",
             "logS_winner_partial", "nan_listed", "ninf_listed", "k_minus_1", "k_plus_1"),
    "batched": ("best_only", "ties_high", "drop_displaced", "ragged_twice", "raw_listed", "z_listed", "merge_first_parts", "stale_beyond",
                "logS_winner_partial", "row0_cand", "row0_VS", "nan_listed", "ninf_listed", "k_minus_1", "k_plus_1"),
    "mfma": ("best_only", "ties_high", "cols_ge_N", "rows_ge_M", "raw_listed", "z_listed", "merge_first_parts", "stale_beyond",
             "logS_winner_partial", "row0_cand", "row0_VS", "nan_listed", "ninf_listed", "k_minus_1", "k_plus_1"),
    "subset": ("ties_high", "raw_listed", "z_listed", "merge_first_parts", "stale_beyond", "logS_winner_partial", "nan_listed",
               "ninf_listed", "k_minus_1", "k_plus_1"),
}
