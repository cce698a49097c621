"""The restatement of a beam turn (tests/beam_ref.py) on designed lists: properties that follow from the rule alone, and every mutant of
the rule shown to change an output on some designed case (a mutant no case notices would mean the cases check nothing there)."""
import numpy as np
import pytest

import beam_ref as br

CASES = br.cases()


def _everything(res):
    st, recs, feds = res
    return br.outputs(st), [r.tolist() for r in recs], feds, list(st["set_of"])


def test_cases_cover_the_issue():
    names = [c[0] for c in CASES]
    assert {c[1] for c in CASES} == set(range(1, 9))
    assert {c[2] for c in CASES} >= {1, 2, 5}
    for kind in ("never", "mid", "pad", "eos0", "limit1", "limit2", "allfin"):
        assert any(n.startswith(kind) for n in names)
    # the kinds do what their names say
    for c in CASES:
        st, recs, _ = br.run_case(c)
        kind = c[0].split("-")[0]
        if kind == "never":
            assert all(len(x) == c[2] for x in st["ids"])
        if kind == "eos0":
            assert any(len(x) == 1 and x[0] in c[3] for x in st["ids"]) and (c[1] == 1 or any(len(x) > 1 for x in st["ids"]))
        if kind == "mid":
            assert any(x[-1] in c[3] for x in st["ids"]) or all(len(x) == c[2] for x in st["ids"])
        if kind == "allfin":
            assert all(len(x) == 3 and x[-1] in c[3] for x in st["ids"]) and len(recs) == 3
        if kind == "limit1":
            assert len(recs) == 1 and all(len(x) == 1 for x in st["ids"])
        if kind == "limit2":
            assert all(len(x) <= 2 for x in st["ids"])
    assert any(len({len(x) for x in br.run_case(c)[0]["ids"]}) >= 2 for c in CASES if c[0].startswith("mid"))
    assert any(-1 in br.tree_lists((), c[1], c[4]["seed"], pad=True)[0] for c in CASES if c[0].startswith("pad"))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_invariants(case):
    _, W, limit, eos, _ = case
    st, recs, feds = br.run_case(case)
    assert 1 <= st["n"] <= W and all(st["fin"])
    sc = [float(s) for s in st["score"]]
    assert sc == sorted(sc, reverse=True)                        # rank order
    assert len(set(map(tuple, st["ids"]))) == st["n"]            # distinct ids in a list -> distinct hypotheses
    assert len(set(st["set_of"])) == st["n"]                     # one page set each
    for g in range(st["n"]):
        ids, lps = st["ids"][g], st["lps"][g]
        assert 1 <= len(ids) <= limit and len(lps) == len(ids)
        assert all(t not in eos for t in ids[:-1]) and (ids[-1] in eos or len(ids) == limit)
        acc = np.float32(0.0)
        for v in lps:
            acc = np.float32(acc + v)
        assert acc.view(np.uint32) == np.float32(st["score"][g]).view(np.uint32)
        assert float(acc) == float(sum(float(v) for v in lps))   # dyadic: the fp32 sum is the exact sum
    for rec, fed in zip(recs, feds):
        n_new, n_live = int(rec[0]), int(rec[1])
        assert n_new <= W and n_live <= n_new
        assert (n_live == 0) == all(f is None for f in fed)


def test_width_one_is_greedy():
    for case in (c for c in CASES if c[1] == 1):
        _, W, limit, eos, kw = case
        kw = dict(kw)
        seed = kw.pop("seed")
        eos0, all_at, all_id = kw.pop("eos_step0", None), kw.pop("all_eos_at", None), kw.pop("all_eos", None)
        ids = []
        while True:
            li, _ = br.tree_lists(ids, 1, seed, eos_top=eos0 if not ids else None, all_eos=all_id if all_at == len(ids) else None, **kw)
            ids.append(li[0])
            if li[0] in eos or len(ids) == limit:
                break
        assert br.run_case(case)[0]["ids"] == [ids]


def test_a_planted_tie_is_real_and_broken_by_rank_then_entry():
    # two live hypotheses with equal scores and lists that tie across and inside rows
    st = {"n": 2, "ids": [[5], [6]], "lps": [[np.float32(-0.5)], [np.float32(-0.5)]], "score": [np.float32(-0.5)] * 2, "fin": [False] * 2,
          "set_of": [0, 1]}
    li = [[3, 4, -1], [3, 9, 1]]
    ll = [[np.float32(-0.25), np.float32(-0.25), np.float32(-np.inf)], [np.float32(-0.25), np.float32(-0.25), np.float32(-0.25)]]
    new, fed, pairs, rec = br.step(st, li, ll, 3, 5, [], n_cp=1)
    assert new["ids"] == [[5, 3], [5, 4], [6, 3]]
    assert rec[4:7].tolist() == [0, 0, 1] and rec[12:15].tolist() == [0, 1, 0]
    assert new["set_of"] == [0, 2, 1] and pairs == [(0, 2)]       # rank 1 is the second child of set 0: the lowest unheld set, one copy
    assert fed == [3, 4, 3, 3]


def test_a_nan_score_is_left_out_of_the_pool():
    nan, q = np.float32(np.nan), np.float32(-0.25)
    new, fed, _, rec = br.step(br.root(), [[4, 5, 6]], [[q, nan, np.float32(-0.5)]], 3, 5, [])
    assert new["ids"] == [[4], [6]] and rec[0] == 2 and rec[12:14].tolist() == [0, 2] and fed == [4, 6, 4, 4]


@pytest.mark.parametrize("mutant", br.MUTANTS)
def test_every_mutant_changes_an_output(mutant):
    hit = [c[0] for c in CASES if _everything(br.run_case(c, mutant=mutant)) != _everything(br.run_case(c))]
    assert hit, f"no designed case notices the mutant {mutant!r}"
