"""The multi-draft turn on paper (no GPU): on an exhaustive small table the simulated turn of drafts_ref equals the plain greedy loop
whatever the drafts say, every listed mistake of the select step is caught by some case of that table, and the rule that drops trailing
drafts holds against the row workspace and against the page pool."""
import itertools

import pytest

import drafts_ref as R

EOS, VOCAB = 3, 4                  # alphabet 0, 1, 2 and the EOS id; 4 and -1 are outside the vocabulary
MAXP = 200


def _policy(seed):
    """a toy deterministic next-token function of the whole prefix (ids 0 .. 3, 3 = EOS)"""
    def f(prefix):
        h = seed
        for i, t in enumerate(prefix):
            h = (h * 31 + (t + 2) * (i + 7)) % 1009
        return h % 4 if h % 5 else h % 3
    return f


def _truth(f, prefix, n):
    ids = []
    for _ in range(n):
        ids.append(f(tuple(prefix) + tuple(ids)))
    return ids


def _draft_pool(f, prefix):
    """drafts built around what the policy will emit: right, right then wrong at every index, EOS-carrying, out of vocabulary, empty"""
    t = _truth(f, prefix, 5)
    pool = [tuple(t), tuple(t[:2]), ()]
    for i in range(4):
        pool.append(tuple(t[:i] + [(t[i] + 1) % 3] + t[i + 1:]))
    pool += [tuple(t[:1] + [EOS] + t[2:]), tuple(t[:2] + [VOCAB] + t[3:]), (-1,) + tuple(t[1:]), tuple(reversed(t))]
    return list(dict.fromkeys(pool))


def _cases():
    """(policy, prefix, drafts, L, P, max_new): every draft of up to 3 ids alone, every set of up to 3 drafts of the pool, every max_new
    from 1 to 6, L in the open and next to max_positions"""
    for seed in (1, 2):
        f = _policy(seed)
        prefix = (seed, 2, 0)
        sets = [()] + [(d,) for n in range(1, 4) for d in itertools.product(range(4), repeat=n)]
        pool = _draft_pool(f, prefix)
        sets += [s for n in (1, 2, 3) for s in itertools.product(pool, repeat=n)]
        for L in (70, 127, MAXP - 6, MAXP - 2, MAXP - 1):
            for max_new in range(1, 7):
                for drafts in sets:
                    yield f, prefix, drafts, L, L - 3, max_new


def _check(case, mutant=None):
    """None when the simulated turn is the plain one and keeps every promise, else what went wrong"""
    f, prefix, drafts, L, P, max_new = case
    want = R.plain_turn(f, prefix, L, max_new, MAXP, {EOS})
    got = R.simulate(f, prefix, drafts, L, P, max_new, MAXP, VOCAB, {EOS}, gq=7, mutant=mutant)
    if want is None or got is None:
        return None if want is None and got is None else "max_positions"
    if got["ids"] != want[0]:
        return "ids"
    if got["kv_len"] != want[1]:
        return "kv_len"
    if any(t == EOS or not (0 <= t < VOCAB) for _, t in got["fed"]):
        return "fed an EOS / foreign id"
    if any(p >= MAXP for p, _ in got["fed"]):
        return "row at max_positions"
    if any(tuple(pre) != tuple(want[0][:i]) for i, pre in enumerate(got["tap_prefix"])):
        return "tap row"
    c = got["counters"]
    if got["winner"] >= 0:
        # the winner is the LOWEST draft that carried the pass's tokens: no page changes hands when an earlier draft is as good
        G, r, ks = R.plan(drafts, L, P, max_new, MAXP, VOCAB, {EOS}, 7, 10 ** 6, 0)
        e = got["pass_tokens"]
        good = [g for g in range(G) if ks[g] >= e - 1 and tuple(drafts[g][:e - 1]) == tuple(want[0][:e - 1])]
        if not good or got["winner"] != good[0] or c["handovers"] != int(good[0] >= 1):
            return "winner"
    if c["pass_tokens"] + c["single_steps"] + c["ignored"] != len(want[0]):
        return "counters"
    return None


def _check_select(case, mutant=None):
    """the select step alone on rows the plan would have cut (a held draft longer than max_new allows: the kernel stops by itself)"""
    f, prefix, drafts, L, P, max_new = case
    want = R.plain_turn(f, prefix, L, max_new, 10 ** 6, {EOS})[0]
    r = 5
    ks = [next((j for j, t in enumerate(D) if not (0 <= t < VOCAB) or t == EOS), len(D)) for D in drafts]
    cand, fed = [f(tuple(prefix))], [0] * (len(drafts) * r)
    for g, D in enumerate(drafts):
        for j in range(ks[g]):
            fed[g * r + j] = D[j]
            cand.append(f(tuple(prefix) + tuple(D[: j + 1])))
    s = R.select(cand, fed, ks, r, 0, max_new, {EOS}, mutant)
    e = s["e"]
    if not (1 <= e <= len(want)) or s["ids"] != want[:e]:
        return "ids"
    if bool(s["stop"]) != (e == len(want)) or s["adv"] != (e - 1 if e == len(want) else e):
        return "stop"
    return None


CASES = None


def _all_cases():
    global CASES
    if CASES is None:
        CASES = list(_cases())
    return CASES


def test_simulated_turn_is_the_plain_greedy_loop():
    n_pass = n_handover = 0
    for case in _all_cases():
        bad = _check(case)
        assert bad is None, (bad, case[2:], R.simulate(*case[:2], case[2], case[3], case[4], case[5], MAXP, VOCAB, {EOS}, gq=7))
    for case in _all_cases():
        if case[3] == 70 and case[2]:
            assert _check_select(case) is None, (_check_select(case), case[2:])
    for f, prefix, drafts, L, P, max_new in _all_cases()[::97]:
        got = R.simulate(f, prefix, drafts, L, P, max_new, MAXP, VOCAB, {EOS}, gq=7)
        if got is not None:
            n_pass += got["counters"]["passes"]
            n_handover += got["counters"]["handovers"]
    assert n_pass > 50 and n_handover > 5            # (the table is not a table of ignored hints)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught(mutant):
    assert any(_check(case, mutant) is not None or (case[3] == 70 and case[2] and _check_select(case, mutant) is not None)
               for case in _all_cases()), mutant


def test_select_tie_goes_to_the_lowest_draft():
    # two drafts equally right: no page changes hands
    s = R.select([5, 6, 7, 6, 7], [5, 6, 0, 0, 5, 6, 0, 0], [2, 2], 4, 0, 10, set())
    assert (s["winner"], s["e"], s["stop"], s["ids"], s["rows"], s["adv"]) == (0, 3, 0, [5, 6, 7], [0, 1, 2], 3)
    s = R.select([5, 9, 6, 7], [4, 0, 5, 6], [1, 2], 2, 0, 10, {7})
    assert (s["winner"], s["e"], s["stop"], s["ids"], s["rows"], s["adv"]) == (1, 3, 1, [5, 6, 7], [0, 2, 3], 2)


def test_trailing_drafts_are_dropped_against_both_limits():
    D = [(1, 1, 1, 1), (2, 2, 2, 2), (0, 1, 2, 0)]
    kw = dict(L=100, P=90, limit=6, vocab=VOCAB, eos={EOS}, gq=7)
    # plenty of both: all three ride, r = 4
    assert R.plan(D, max_positions=400, free_pages=10, env_pages=2, **kw) == (3, 4, [4, 4, 4])
    # positions 100 .. 103 lie in page 1, which the env holds: every fork takes one private page, the env none
    assert R.plan(D, max_positions=400, free_pages=2, env_pages=2, **kw) == (3, 4, [4, 4, 4])
    assert R.plan(D, max_positions=400, free_pages=1, env_pages=2, **kw) == (2, 4, [4, 4])
    assert R.plan(D, max_positions=400, free_pages=0, env_pages=2, **kw) == (1, 4, [4])
    # the env itself lacks page 1: one page goes to it first, and with none free no draft rides
    assert R.plan(D, max_positions=400, free_pages=1, env_pages=1, **kw) == (1, 4, [4])
    assert R.plan(D, max_positions=400, free_pages=0, env_pages=1, **kw) == (0, 0, [])
    # a fork whose rows cross into the next page takes two
    kw2 = dict(kw, L=126, P=120)
    assert R.plan(D, max_positions=400, free_pages=4, env_pages=3, **kw2) == (3, 4, [4, 4, 4])
    assert R.plan(D, max_positions=400, free_pages=3, env_pages=3, **kw2) == (2, 4, [4, 4])
    # the row workspace: Tn + G r rows within max_positions (Tn = 10); k is cut by max_positions - L as well
    assert R.plan(D, max_positions=104, free_pages=10, env_pages=2, **kw) == (3, 4, [4, 4, 4])
    kw3 = dict(kw, L=20, P=10)
    assert R.plan(D, max_positions=22, free_pages=10, env_pages=1, **kw3) == (3, 4, [2, 2, 2])
    assert R.plan(D, max_positions=21, free_pages=10, env_pages=1, **kw3) == (2, 4, [1, 1])
    assert R.plan(D, max_positions=23, free_pages=10, env_pages=1, **dict(kw, L=20, P=0)) == (0, 0, [])      # 20 + 1 x 4 rows > 23
    assert R.plan(D, max_positions=24, free_pages=10, env_pages=1, **dict(kw, L=20, P=0)) == (1, 4, [4])
    # a draft with k = 0 takes no page; drafts that all open with an unusable id are no drafts
    assert R.plan([(1, 1), (EOS, 1), (2,)], max_positions=400, free_pages=1, env_pages=2, **kw) == (3, 4, [2, 0, 1])
    assert R.plan([(EOS,), (VOCAB, 1), ()], max_positions=400, free_pages=9, env_pages=2, **kw) == (0, 0, [])
    # limit - 1 ids at the most, cut at the first EOS / foreign id
    assert R.plan([(1, 1, 1, 1)], max_positions=400, free_pages=9, env_pages=2, **dict(kw, limit=3)) == (1, 4, [2])
    assert R.plan([(1, 1, EOS, 1), (1, -1, 1)], max_positions=400, free_pages=9, env_pages=2, **kw) == (2, 4, [2, 1])
    assert R.plan([(1, 1)], max_positions=400, free_pages=9, env_pages=2, **dict(kw, limit=1)) == (0, 0, [])
