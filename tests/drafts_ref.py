"""Restatement of the multi-draft turn (svln_generate_drafts) in plain Python: the plan (which drafts ride the prefill pass and how many
ids each feeds), the select step (draft_select_kernel: the verify rule on every branch, the winner) and a whole turn against an arbitrary
next-token function, with the eight counters of svln_drafts_stats.  `mutant` names one deliberate mistake of the select step; the tests
show that every one of them is caught."""

PAGE = 64
COUNTERS = ("calls", "passes", "pass_tokens", "rows_fed", "finished_in_pass", "ignored", "handovers", "single_steps")
MUTANTS = ("tie_high", "rows_of_0", "cmp_fed_i", "past_stop", "other_tokens", "stop_adv_e", "skip_row0", "k_wrong_seq", "tap_wrong_row")


def rows_per_pass(G, gq):
    """row slots of a draft: the candidates call's rule (gq = q_heads / kv_heads)"""
    return min(32 // gq, 32 // G)


def fork_tail_pages(L, limit):
    return 0 if limit == 1 else (L + limit - 1 + PAGE - 1) // PAGE - L // PAGE


def plan(drafts, L, P, limit, max_positions, vocab, eos, gq, free_pages, env_pages):
    """-> (G, r, [k_g]): the drafts that ride and the ids each feeds; G = 0: the plain turn"""
    Tn = L - P
    if Tn < 1 or limit < 1:
        return 0, 0, []
    for G in range(len(drafts), 0, -1):
        r = rows_per_pass(G, gq)
        ks, need = [], 0
        for g in range(G):
            D = drafts[g]
            k = max(min(len(D), r, limit - 1, max_positions - L), 0)
            for j in range(k):
                if not (0 <= D[j] < vocab) or D[j] in eos:
                    k = j
                    break
            ks.append(k)
            need += max((L + k + PAGE - 1) // PAGE - env_pages, 0) if g == 0 else fork_tail_pages(L, k + 1)
        if Tn + G * r > max_positions or need > free_pages:
            continue
        if sum(ks) == 0:
            return 0, 0, []
        return G, r, ks
    return 0, 0, []


def select(cand, fed, ks, r, count, max_new, eos, mutant=None):
    """cand: the head rows' arg-maxes (row 0 = the prompt's last row, then the rows of draft 0, 1, ...); fed[g * r + j] = the id row slot j
    of draft g was fed.  -> dict(winner, e, stop, ids, rows = the head row of every emitted token, nh, adv = what pos / kv_len advance by)"""
    G, nh = len(ks), 1 + sum(ks)
    bases, b = [], 1
    for g in range(G):
        bases.append(b)
        b += ks[g]
    best = dict(winner=-1, e=0, stop=0, rows=[])
    for g in range(G):
        kg = ks[(g + 1) % G] if mutant == "k_wrong_seq" else ks[g]
        base = 1 if mutant == "rows_of_0" else bases[g]
        rows, stop, prev = [], 0, None
        for i in range(kg + 1):
            if stop and mutant != "past_stop":
                break
            if mutant == "skip_row0":
                row = base + i
            else:
                row = 0 if i == 0 else base + i - 1
            if row >= nh:
                break
            if i > 0:
                j = i if mutant == "cmp_fed_i" else i - 1
                if j >= r or prev != fed[g * r + j]:
                    break
            prev = cand[row]
            rows.append(row)
            stop = stop or int(prev < 0 or count + len(rows) >= max_new or prev in eos)
        better = len(rows) >= best["e"] if mutant == "tie_high" else len(rows) > best["e"]
        if better and rows:
            best = dict(winner=g, e=len(rows), stop=stop, rows=rows)
    e, rows = best["e"], list(best["rows"])
    if mutant == "other_tokens" and G > 1:
        o = (best["winner"] + 1) % G
        rows = [0 if i == 0 else min(bases[o] + i - 1, nh - 1) for i in range(e)]
    ids = [cand[q] for q in rows]
    if mutant == "tap_wrong_row":
        rows = [0 if i == 0 else min(i, nh - 1) for i in range(e)]
    adv = e if (not best["stop"] or mutant == "stop_adv_e") else e - 1
    return dict(winner=best["winner"], e=e, stop=best["stop"], ids=ids, rows=rows, nh=nh, adv=adv)


def plain_turn(next_token, prefix, L, max_new, max_positions, eos):
    """the greedy loop of svln_generate: -> (ids, kv_len) or None when the sequence would pass max_positions"""
    ids = []
    while True:
        t = next_token(tuple(prefix) + tuple(ids))
        ids.append(t)
        if t < 0 or t in eos or len(ids) >= max_new:
            return ids, L + len(ids) - 1
        if L + len(ids) - 1 >= max_positions:          # the next step would feed a position the cache does not have
            return None


def simulate(next_token, prefix, drafts, L, P, max_new, max_positions, vocab, eos, gq, free_pages=10 ** 6, env_pages=0, ignore=False,
             mutant=None):
    """One svln_generate_drafts call.  -> dict(ids, kv_len, counters, winner, pass_tokens, fed = [(position, id)] of every row the pass
    fed, tap_prefix = per emitted pass token the ids its head row had been fed behind the prompt) or None (max_positions)."""
    c = dict.fromkeys(COUNTERS, 0)
    c["calls"] = 1
    G, r, ks = (0, 0, []) if ignore else plan(drafts, L, P, max_new, max_positions, vocab, eos, gq, free_pages, env_pages)
    if G == 0:
        c["ignored"] = 1
        out = plain_turn(next_token, prefix, L, max_new, max_positions, eos)
        if out is None:
            return None
        c["single_steps"] = len(out[0]) - 1
        return dict(ids=out[0], kv_len=out[1], counters=c, winner=-1, pass_tokens=0, fed=[], tap_prefix=[])
    cand, fed, fed_rows, row_prefix = [next_token(tuple(prefix))], [0] * (G * r), [], [()]
    for g in range(G):
        for j in range(ks[g]):
            fed[g * r + j] = drafts[g][j]
            fed_rows.append((L + j, drafts[g][j]))
            row_prefix.append(tuple(drafts[g][: j + 1]))
            cand.append(next_token(tuple(prefix) + tuple(drafts[g][: j + 1])))
    s = select(cand, fed, ks, r, 0, max_new, eos, mutant)
    ids, kv = list(s["ids"]), L + s["adv"]
    c.update(passes=1, pass_tokens=s["e"], rows_fed=sum(ks), finished_in_pass=int(bool(s["stop"])), handovers=int(s["winner"] >= 1))
    done = bool(s["stop"])
    while not done:
        if L + len(ids) - 1 >= max_positions:
            return None
        t = next_token(tuple(prefix) + tuple(ids))
        ids.append(t)
        c["single_steps"] += 1
        done = t < 0 or t in eos or len(ids) >= max_new
        if not done:
            kv += 1
    return dict(ids=ids, kv_len=kv, counters=c, winner=s["winner"], pass_tokens=s["e"], fed=fed_rows,
                tap_prefix=[row_prefix[q] for q in s["rows"]])
