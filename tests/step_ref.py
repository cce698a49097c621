"""Plain Python restatement and exact cases of the greedy loop's step kernel (launch_argmax_step / launch_argmax_final: argmax_final_kernel of
gemv.hip with and without GenCtl), written from the contract in kernels.h.  Test infrastructure, modelled on tests/verify_ref.py.

Arg-max over one set of n partials (part_val, part_idx): the greatest value wins, an equal value goes to the lowest part_idx wherever the
partial stands; NaN never wins; a partial with index 0x7FFFFFFF owns nothing; no winner gives token -1.  out_top = (best value, second
largest partial value counted with multiplicity; NaN ignored; -inf for n = 1).

Step on GenCtl (pos, kv_len, done, count, max_new): done on entry -> nothing at all is written.  Otherwise out_ids[count] = tok and
scores[count] are written before the count advances, the flag byte `tok` is set for tok >= 0 only, count += 1, done is set on an EOS hit,
on tok < 0 or on count == max_new; otherwise pos and kv_len advance by one (an EOS is appended, never fed).

Scores in float64: greedy -log sum_k part_sum[k] exp(part_val[k] - V); sampled part_raw(owner) - V - log S on (part_max, part_sum).

Exact inputs: every finite value is a multiple of 1/4 of small magnitude, so each compare of the kernel is decided exactly and no two
candidates for the winner are closer than an exact tie (tests/test_step_inputs.py asserts it); the background sits 20 .. 30 below the top,
so the fp32 sums of the two score merges stay inside scores_ref.TOL / sample_ref.TOL, the bound those merges already carry.

Mutants: the restatement with one plausible mistake each; tests/test_step_inputs.py proves every one is rejected by some case.
"""
import math

import numpy as np

import sample_ref
import scores_ref

assert sample_ref.TOL == scores_ref.TOL
TOL = scores_ref.TOL        # |score - float64| of the greedy and of the sampled merge (derived in scores_ref.py / sample_ref.py)
NONE = 0x7FFFFFFF
F = np.float32
NEG = float("-inf")
SENT_ID, SENT_FLAG = -7, 0x5A                       # what svln_op_argmax_step fills ids / flag bytes with (floats: NaN)
NS = (1, 2, 8, 255, 256, 257, 1024, 2048)           # truncated row, allowed-token head (<= 256), gemv_grid of a full vocabulary, largest lm_head grid
N_EOS = (0, 1, 2, 256, 257, 300)
FORMS = ("plain", "lse", "smp")
FLAG_BYTES = 4352                                   # above every part_idx a case uses
MUTANTS = ("tie_highest_index", "tie_first_partial", "eos_fed", "stop_before_increment", "flag_for_minus_one", "score_at_next_row",
           "runner_up_distinct", "eos_scan_256", "works_when_done")
TOP = 12.0


# ---------------------------------------------------------------------------------------------------------- restatement
def argmax(pv, pi, mut=None):
    """(token, best value, runner-up value) of one partial set"""
    live = [(float(v), int(i), k) for k, (v, i) in enumerate(zip(pv, pi)) if not math.isnan(v) and int(i) != NONE]
    vals = sorted((float(v) for v in pv if not math.isnan(v)), reverse=True)
    best = vals[0] if vals else NEG
    if not live:
        tok = -1
    else:
        top = max(v for v, _, _ in live)
        tied = [(i, k) for v, i, k in live if v == top]
        if mut == "tie_highest_index":
            tok = max(i for i, _ in tied)
        elif mut == "tie_first_partial":
            tok = min(tied, key=lambda t: t[1])[0]
        else:
            tok = min(i for i, _ in tied)
    if mut == "runner_up_distinct":
        rest = [v for v in vals if v < best]
        second = rest[0] if rest else NEG
    else:
        second = vals[1] if len(vals) > 1 else NEG
    return tok, best, second


def _lse(m, s):
    """(V, log S) in float64 over the partials with a non-zero sum"""
    with np.errstate(all="ignore"):
        m, s = np.asarray(m, np.float64), np.asarray(s, np.float64)
        fin = m[~np.isnan(m)]
        V = float(fin.max()) if fin.size else NEG
        keep = s != 0
        return V, float(np.log(np.sum(s[keep] * np.exp(m[keep] - V))))


def score(case, s, tok):
    """float64 score of launch s's token (None: the form writes no score)"""
    if case.form == "plain":
        return None
    if tok < 0:
        return float("nan")
    if case.form == "lse":
        return -_lse(case.pv[s], case.ps[s])[1]
    V, logS = _lse(case.pm[s], case.ps[s])
    owner = [k for k in range(case.n) if int(case.pi[s][k]) == tok]
    assert len(owner) == 1, (case.name, s, tok)
    return float(case.pr[s][owner[0]]) - V - logS


class Outcome:
    """what the entry must return: ctl (pos, kv_len, done, count, max_new), out_ids [rows], last_token, out_top (None: untouched),
    scores [rows] (None: untouched, else float64, NaN included), flags (bytes)"""

    def key(self):
        sc = tuple(None if v is None else ("nan" if math.isnan(v) else v) for v in self.scores)
        return (tuple(self.ctl), tuple(self.out_ids), self.last_token, self.out_top, sc, bytes(self.flags))


def run(case, mut=None):
    """the `steps` launches of launch_argmax_step on the case, back to back"""
    o = Outcome()
    pos, kv_len, done, count, max_new = case.pos, case.kv_len, case.done, case.count, case.max_new
    o.out_ids, o.scores, o.flags = [SENT_ID] * case.rows, [None] * case.rows, bytearray([SENT_FLAG]) * case.flag_bytes
    o.last_token, o.out_top = SENT_ID, None
    for s in range(case.steps):
        if done and mut != "works_when_done":
            continue
        tok, best, second = argmax(case.pv[s], case.pi[s], mut)
        o.last_token, o.out_top = tok, (best, second)
        c = count
        sc = score(case, s, tok)
        if sc is not None:
            o.scores[c + 1 if mut == "score_at_next_row" else c] = sc
        o.out_ids[c] = tok
        if case.flag_bytes and (tok >= 0 or mut == "flag_for_minus_one"):
            o.flags[tok] = 1
        count = c + 1
        eos = case.eos[:256] if mut == "eos_scan_256" else case.eos
        hit = tok in eos
        stop = (c == max_new) if mut == "stop_before_increment" else (count == max_new)
        if hit or tok < 0 or stop:
            done = 1
        if not (tok < 0 or stop or (hit and mut != "eos_fed")):
            pos, kv_len = pos + 1, kv_len + 1
    o.ctl = (pos, kv_len, done, count, max_new)
    return o


def run_final(case):
    """launch_argmax_final on set 0: (token, out_top, score or None)"""
    tok, best, second = argmax(case.pv[0], case.pi[0])
    return tok, (best, second), score(case, 0, tok)


# ---------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, sets, form="plain", pos=40, done=0, count=0, max_new=100, eos=(), flags=False, rows=None):
        """sets: [(pv [n], pi [n])] per launch; the score arrays of `form` are derived from them (see _score_arrays)"""
        self.name, self.form = f"{name}-{form}" + ("-flags" if flags else ""), form
        self.pv = np.stack([np.asarray(v, F) for v, _ in sets])
        self.pi = np.stack([np.asarray(i, np.int32) for _, i in sets])
        self.steps, self.n = self.pv.shape
        self.pos, self.kv_len, self.done, self.count, self.max_new = pos, pos + 1, done, count, max_new
        self.eos, self.flag_bytes = tuple(int(e) for e in eos), FLAG_BYTES if flags else 0
        self.rows = rows if rows is not None else count + self.steps + 2
        self.ps = self.pr = self.pm = None
        if form != "plain":
            self.ps, self.pr, self.pm = _score_arrays(self.pv, self.pi, form)
        if form == "lse":
            self.pr = self.pm = None


def _score_arrays(pv, pi, form):
    """part_sum in {1, 1.25, 1.5, 1.75} (0 for a partial that owns nothing); sampled: part_max 20 .. 30 below TOP but one heavy partial at
    TOP, which need not be the winner's (V comes from part_max, the winner from part_val), part_raw = part_max - {0, 1/2, 1}"""
    steps, n = pv.shape
    k = np.arange(n)
    ps = np.tile((1 + (k % 4) / 4).astype(F), (steps, 1))
    pm = np.tile((TOP - 20 - ((k * 11) % 21) / 2).astype(F), (steps, 1))
    pm[:, (2 * n) // 3] = TOP
    pr = (pm - ((k % 3) / 2).astype(F)[None]).astype(F)
    empty = pi == NONE
    ps[empty], pm[empty], pr[empty] = 0, -np.inf, 0
    if form == "smp" and bool(empty[:, (2 * n) // 3].any()):
        for s in range(steps):                        # keep one heavy live partial
            j = int(np.nonzero(~empty[s])[0][0]) if (~empty[s]).any() else None
            if j is not None:
                pm[s, j], pr[s, j] = TOP, TOP - 1
    return ps, pr, pm


def base(n, top_at=None, seed=0, top=TOP):
    """background 20 .. 30 below `top` in halves, part_idx = 5 + 2 k, the top planted at partial top_at (default: late in the row)"""
    k = np.arange(n)
    pv = (top - 20 - ((k * 7 + seed) % 21) / 2).astype(F)
    pi = (5 + 2 * k).astype(np.int32)
    pv[(n * 3) // 4 if top_at is None else top_at] = top
    return pv, pi


def tie(n, a, b, low_in_b, seed=0):
    """the top value in partials a < b; the lower index stands in b when low_in_b"""
    pv, pi = base(n, a, seed)
    pv[b] = TOP
    pi[a], pi[b] = (4300, 3) if low_in_b else (3, 4300)
    return pv, pi


def empty_set(n):
    return np.full(n, -np.inf, F), np.full(n, NONE, np.int32)


def winner(n, tok, seed=0):
    """a set whose decided winner is token `tok`"""
    pv, pi = base(n, None, seed)
    pi[(n * 3) // 4] = tok
    return pv, pi


def level_pairs(n):
    """(a, b): partials of threads t = s - 1 and t + s, the two halves of reduction level s, for every level the row reaches"""
    return [(s - 1, 2 * s - 1) for s in (128, 64, 32, 16, 8, 4, 2, 1) if 2 * s - 1 < n]


def argmax_cases():
    out = []
    for n in NS:
        for form in FORMS:
            out.append(Case(f"base-n{n}", [base(n, None, n)], form, flags=True))
            out.append(Case(f"first-n{n}", [base(n, 0, n)], form))
            out.append(Case(f"last-n{n}", [base(n, n - 1, n)], form, flags=True))
            for a, b in level_pairs(n):
                for low_in_b in (False, True):
                    out.append(Case(f"level{b - a}-{'hi' if low_in_b else 'lo'}-n{n}", [tie(n, a, b, low_in_b, n)], form))
            for k in (0, 3, 255):                     # the same thread on two trips (and on three, where the row has them)
                if k + 256 < n:
                    for low_in_b in (False, True):
                        out.append(Case(f"trips{k}-{'hi' if low_in_b else 'lo'}-n{n}", [tie(n, k, k + 256, low_in_b, n)], form))
                    if k + 512 < n:
                        out.append(Case(f"trips3-{k}-n{n}", [tie(n, k + 256, k + 512, True, n)], form))
            if n >= 3:                                # a three-way tie: the runner-up is the top value itself
                pv, pi = tie(n, 0, n - 1, True, n)
                pv[n // 2], pi[n // 2] = TOP, 4200
                out.append(Case(f"three-way-n{n}", [(pv, pi)], form, flags=True))
                pv, pi = base(n, n // 2, n)           # owns-nothing partials between live ones, first and last included
                for k in {0, n // 2 - 1, n - 1} - {n // 2}:
                    pv[k], pi[k] = -np.inf, NONE
                out.append(Case(f"holes-n{n}", [(pv, pi)], form))
            out.append(Case(f"all-empty-n{n}", [empty_set(n)], form, flags=True, pos=7, count=3))
        for form in ("plain", "smp"):                 # NaN / +inf values: the greedy sum over them has no decided value
            pv, pi = base(n, n - 1, n)
            pv[0], pi[0] = np.nan, 0                  # the lowest index of all: it must not win, nor count as a runner-up
            if n >= 3:
                pv[n // 2] = np.nan
            out.append(Case(f"nan-n{n}", [(pv, pi)], form, flags=True))
            pv, pi = base(n, n - 1, n)
            pv[n // 3] = np.inf
            if n >= 3:
                pv[0], pi[0] = np.nan, NONE
            out.append(Case(f"inf-n{n}", [(pv, pi)], form))
            if n >= 2:                                # two +inf: the tie rule and the runner-up hold at infinity too
                pv, pi = tie(n, 0, n - 1, True, n)
                pv[0] = pv[n - 1] = np.inf
                out.append(Case(f"inf-tie-n{n}", [(pv, pi)], form))
        pv = np.full(n, np.nan, F)                    # nothing but NaN
        out.append(Case(f"all-nan-n{n}", [(pv, np.full(n, NONE, np.int32))], "plain", flags=True))
    return out


def _eos_list(n_eos, hit_at, tok):
    e = [100000 + j for j in range(n_eos)]
    if hit_at is not None:
        e[hit_at] = tok
    return e


def step_cases():
    out = []
    n, tok = 257, 76                               # (the background owns the odd indices: planted tokens are even)
    for form in FORMS:
        for n_eos in N_EOS:
            out.append(Case(f"eos{n_eos}-miss", [winner(n, tok)], form, eos=_eos_list(n_eos, None, tok), flags=True))
            for hit_at in sorted({0, n_eos - 1, 256} & set(range(n_eos))):
                out.append(Case(f"eos{n_eos}-hit{hit_at}", [winner(n, tok)], form, eos=_eos_list(n_eos, hit_at, tok), flags=True, count=2))
        # the max_new edge from both sides, max_new = 1, EOS and max_new at once
        out.append(Case("max_new-reached", [winner(n, tok)], form, count=4, max_new=5, flags=True))
        out.append(Case("max_new-one-short", [winner(n, tok)], form, count=3, max_new=5))
        out.append(Case("max_new-1", [winner(n, tok)], form, count=0, max_new=1))
        out.append(Case("eos-and-max_new", [winner(n, tok)], form, count=4, max_new=5, eos=[tok], flags=True))
        # done on entry: every output keeps its sentinel, GenCtl its values
        out.append(Case("done-on-entry", [winner(n, tok)], form, done=1, count=2, eos=[tok], flags=True))
        out.append(Case("done-on-entry-x3", [winner(n, tok + 2 * s, s) for s in range(3)], form, done=1, count=0, max_new=1, flags=True))
        # sequences that end in the middle; every launch has its own token
        for steps in (2, 3, 4, 5, 6):
            sets = [winner(n, 200 + 4 * s, s) for s in range(steps)]
            for end in range(steps - 1):
                out.append(Case(f"seq{steps}-eos-at{end}", sets, form, count=1, eos=[9, 200 + 4 * end], flags=True))
                out.append(Case(f"seq{steps}-max_new-at{end}", sets, form, count=1, max_new=end + 2, flags=True))
            out.append(Case(f"seq{steps}-runs-on", sets, form, count=1, eos=[9], flags=True))
        sets = [winner(n, 300, 0), empty_set(n), winner(n, 302, 1)]             # an empty row ends the turn in the middle
        out.append(Case("emptyrow-in-seq3-at1", sets, form, flags=True))
        sets = [winner(8, 310, 0), winner(8, 310, 1), winner(8, 312, 2)]         # the same token twice, then EOS (truncated-row size)
        out.append(Case("repeat-in-seq3", sets, form, eos=[312], flags=True))
    return out


def all_cases():
    return argmax_cases() + step_cases()


def check_decided(case):
    """every finite value is a multiple of 1/4 with |v| <= 64 (exact in fp32, so every compare is decided and a tie is exact), a partial
    that owns nothing holds -inf or NaN, the live indices fit the flag array and are unique but for none (the owner of a token is one
    partial)"""
    for s in range(case.steps):
        for arr in (case.pv, case.ps, case.pr, case.pm):
            if arr is None:
                continue
            v = arr[s][np.isfinite(arr[s])].astype(np.float64)
            assert np.all(v * 4 == np.round(v * 4)) and (v.size == 0 or np.abs(v).max() <= 64), case.name
        none = case.pi[s] == NONE
        assert np.all(np.isnan(case.pv[s][none]) | (case.pv[s][none] == -np.inf)), case.name
        live = case.pi[s][~none]
        assert live.size == np.unique(live).size and (live.size == 0 or (live.min() >= 0 and live.max() < FLAG_BYTES)), case.name
        assert not np.any((case.pv[s] == -np.inf) & ~none), case.name      # (-inf with a live index is no producer's output)
    assert case.count + case.steps <= case.rows
