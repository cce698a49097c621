"""Restatement of a beam turn (svln_generate_beams) in plain Python / numpy fp32: the rule of one select step (`step`), the loop around it
(`run`) and designed list providers with dyadic log-probabilities, on which fp32 sums are exact and planted ties are real.

State of the hypothesis set (rank = index):
    n        hypotheses in the set (<= W)
    ids      [n] lists of ids;  lps  [n] lists of fp32 log-probabilities;  score [n] fp32;  fin [n] bool
    set_of   [n] the page set (0 .. 2 W - 1) that holds the hypothesis' private tail pages
Step 0 starts from `root()`: one live hypothesis without ids, score 0, on set 0 (fl(0 + lp) = lp).

One step (`step`): row r of `list_ids` / `list_lps` ([rows][W], rows indexed by rank; rows of finished ranks are not read) is the list of
live hypothesis r: entries by log-probability descending, -1 / -inf behind the listable ones.
    pool    = every finished hypothesis (item (r, 0), score unchanged) + every (r, j) of a live one with id >= 0, score fl(score_r + lp_rj);
              an item whose score is NaN is left out (the engine's lists hold none; the rule keeps the order total)
    new set = the best W of the pool by score descending, then r ascending, then j ascending; a live hypothesis survives in its children only
    finished: the appended id is in the EOS set, or the length equals `limit`
    pages   : new rank c in order takes the set of its parent if no earlier new rank took it (no copy), else the lowest set that no
              hypothesis of the OLD set holds and no earlier new rank took, and copies the parent's first n_cp tail pages into it
              (pairs (src, dst)); sources are held by the old set, destinations are not: the two sides never meet
    fed     : row k < B of the next step feeds the last id of rank k if it is live, else of the first live rank (untouched if none is live)
    record  : [n_new, n_live, n_rows (live before), n_pairs, parent[8], j[8], set[8]] (int32, unused entries -1)
"""
import numpy as np

MAXW = 8
REC = 4 + 3 * MAXW

MUTANTS = ("drop_finished", "extend_finished", "tie_high_j", "tie_high_rank", "parent_survives", "feed_eos", "score_last_lp",
           "keep_w_minus_1", "keep_w_plus_1", "parent_off_by_one", "limit_not_finishing", "take_pad")


def root():
    return {"n": 1, "ids": [[]], "lps": [[]], "score": [np.float32(0.0)], "fin": [False], "set_of": [0]}


def step(state, list_ids, list_lps, W, limit, eos, n_cp=0, set_pages=None, B=None, mutant=None):
    """-> (new state, fed [B] or None entries where untouched, pairs [(src, dst)], record int32 [REC])"""
    n = state["n"]
    eos = set(int(e) for e in eos)
    pool = []
    for r in range(n):
        if state["fin"][r] and mutant != "extend_finished":
            if mutant != "drop_finished":
                pool.append((state["score"][r], r, 0, True))
            continue
        if mutant == "parent_survives" and not state["fin"][r] and state["ids"][r]:
            pool.append((state["score"][r], r, 0, True))
        for j in range(W):
            tid = int(list_ids[r][j])
            if tid < 0 and mutant != "take_pad":
                continue
            lp = np.float32(list_lps[r][j])
            s = lp if mutant == "score_last_lp" else np.float32(state["score"][r] + lp)
            if s != s:                   # a NaN score has no place in an order: the item is not in the pool
                continue
            pool.append((s, r, j, False))
    if mutant == "tie_high_j":
        key = lambda it: (-float(it[0]), it[1], -it[2])
    elif mutant == "tie_high_rank":
        key = lambda it: (-float(it[0]), -it[1], it[2])
    else:
        key = lambda it: (-float(it[0]), it[1], it[2])
    pool.sort(key=key)
    keep = W - 1 if mutant == "keep_w_minus_1" else W + 1 if mutant == "keep_w_plus_1" else W
    pool = pool[:keep]
    new = {"n": len(pool), "ids": [], "lps": [], "score": [], "fin": [], "set_of": []}
    rec = np.full(REC, -1, dtype=np.int32)
    held = set(state["set_of"][:n])
    free = [s for s in range(2 * MAXW) if s not in held]
    claimed, pairs = set(), []
    for c, (s, r, j, carried) in enumerate(pool):
        src_r = r
        if mutant == "parent_off_by_one" and not carried:
            src_r = (r + 1) % n
        if carried:
            ids, lps, fin = list(state["ids"][r]), list(state["lps"][r]), bool(state["fin"][r])
        else:
            tid = int(list_ids[r][j])
            ids = list(state["ids"][src_r]) + [tid]
            lps = list(state["lps"][src_r]) + [np.float32(list_lps[r][j])]
            fin = tid in eos or (len(ids) >= limit and mutant != "limit_not_finishing")
        new["ids"].append(ids); new["lps"].append(lps); new["score"].append(np.float32(s)); new["fin"].append(fin)
        src = state["set_of"][src_r]
        if src not in claimed:
            dst = src
        else:
            dst = free.pop(0)
            if set_pages is not None:
                pairs += [(int(set_pages[src][i]), int(set_pages[dst][i])) for i in range(n_cp)]
            else:
                pairs += [(src, dst)] * n_cp
        claimed.add(dst)
        new["set_of"].append(dst)
        if c < MAXW:
            rec[4 + c], rec[4 + MAXW + c], rec[4 + 2 * MAXW + c] = r, j, dst
    live = [c for c in range(new["n"]) if not new["fin"][c]]
    if B is None:
        B = 2
        while B < W:
            B <<= 1
    fed = [None] * B
    for k in range(B):
        if not live:
            break
        own = k < new["n"] and (not new["fin"][k] or mutant == "feed_eos")
        fed[k] = new["ids"][k if own else live[0]][-1]
    rec[0], rec[1], rec[2], rec[3] = new["n"], len(live), sum(1 for r in range(n) if not state["fin"][r]), len(pairs)
    return new, fed, pairs, rec


def run(W, limit, eos, provider, mutant=None, max_steps=64):
    """the whole turn: provider(t, state) -> (list_ids [rows][W], list_lps [rows][W]) for the set BEFORE step t's select (rows by rank).
    -> (final state, per-step records, per-step fed lists)"""
    st = root()
    recs, feds = [], []
    for t in range(max_steps):
        if all(st["fin"][: st["n"]]):          # (an empty set is finished as well)
            break
        li, ll = provider(t, st)
        st, fed, _, rec = step(st, li, ll, W, limit, eos, mutant=mutant)
        recs.append(rec); feds.append(fed)
        if st["n"] == 0:
            break
    return st, recs, feds


def outputs(st):
    """what a caller sees: (ids, lps as bit patterns, scores as bit patterns, fin) in rank order"""
    return ([list(x) for x in st["ids"]],
            [[int(np.float32(v).view(np.uint32)) for v in x] for x in st["lps"]],
            [int(np.float32(v).view(np.uint32)) for v in st["score"]],
            [bool(f) for f in st["fin"]])


# ---- designed lists ------------------------------------------------------------------------------------------------------------------
def _mix(*vals):
    h = 0x9E3779B97F4A7C15
    for v in vals:
        h ^= (int(v) + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
        h = (h * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 29
    return h


def tree_lists(prefix, W, seed, alphabet=12, pad=False, eos_top=None, all_eos=None):
    """the list of the hypothesis with ids `prefix`: W entries, distinct ids of 0 .. alphabet - 1, log-probabilities -m / 8 with small
    integer steps (0 plants a tie; ties list the lower id first, as the engine's lists do).  pad: the list ends in 1 .. 2 entries (-1, -inf)
    when W > 2.  eos_top: that id is entry 0.  all_eos: every listable entry is this id's neighbourhood (ids all_eos, all_eos + 1, ...)."""
    h = _mix(seed, len(prefix), *prefix)
    n_list = W
    if pad and W > 2:
        n_list = W - 1 - (h >> 7) % 2
    ids = sorted(range(alphabet), key=lambda c: _mix(h, c))[:n_list]
    if all_eos is not None:
        ids = [all_eos + i for i in range(n_list)]
    elif eos_top is not None:
        ids = [eos_top] + [i for i in ids if i != eos_top][: n_list - 1]
    lps, m, g = [], 1 + (h >> 3) % 3, h >> 17
    for i in range(n_list):
        lps.append(np.float32(-m / 8.0))
        m += g % 3                       # 0: a tie with the next entry
        g = g // 3 + 0x2545F
    # ties list the lower id first
    i = 0
    while i < n_list:
        j = i
        while j + 1 < n_list and lps[j + 1] == lps[i]:
            j += 1
        ids[i: j + 1] = sorted(ids[i: j + 1])
        i = j + 1
    ids += [-1] * (W - n_list)
    lps += [np.float32(-np.inf)] * (W - n_list)
    return ids, lps


def tree_provider(W, seed, **kw):
    eos_step0 = kw.pop("eos_step0", None)
    all_eos_at = kw.pop("all_eos_at", None)
    all_eos = kw.pop("all_eos", None)

    def provider(t, st):
        li, ll = [], []
        for r in range(st["n"]):
            a, b = tree_lists(st["ids"][r], W, seed, eos_top=eos_step0 if t == 0 else None,
                              all_eos=all_eos if (all_eos_at is not None and t == all_eos_at) else None, **kw)
            li.append(a); ll.append(b)
        return li, ll
    return provider


def cases():
    """(name, W, limit, eos, provider kwargs) of the designed cases: every W, EOS at step 0 / mid-turn / never, limit 1 and 2, -1 padding,
    all hypotheses finishing in one step"""
    out = []
    for W in range(1, MAXW + 1):
        for seed in (1, 2, 3):
            out.append((f"never-W{W}-s{seed}", W, 5, [], dict(seed=seed)))
            out.append((f"mid-W{W}-s{seed}", W, 5, [2, 7], dict(seed=seed)))
            out.append((f"pad-W{W}-s{seed}", W, 5, [2], dict(seed=seed, pad=True)))
        out.append((f"eos0-W{W}", W, 5, [3], dict(seed=4, eos_step0=3)))
        out.append((f"limit1-W{W}", W, 1, [2], dict(seed=5)))
        out.append((f"limit2-W{W}", W, 2, [2], dict(seed=6)))
        out.append((f"allfin-W{W}", W, 5, list(range(20, 20 + MAXW)), dict(seed=7, all_eos_at=2, all_eos=20)))
        out.append((f"small-W{W}", W, 4, [1], dict(seed=8, alphabet=max(W, 3))))
    return out


def run_case(case, mutant=None):
    _, W, limit, eos, kw = case
    kw = dict(kw)
    return run(W, limit, eos, tree_provider(W, kw.pop("seed"), **kw), mutant=mutant)
