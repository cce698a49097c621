"""Truncated sampling on the CPU (svln_sampling_truncation): the cases of tests/trunc_ref.py are sharp and its restatement is right.

  * the fp32 restatement against the float64 reference: the kept set and the token are equal, |logprob - float64| <= 2e-6;
  * every case keeps >= 100 x the GPU tolerance on the perturbed top-2 margin among the kept, on the distance of every c_{j-1} from
    top_p * total and on the gap between the k-th and the (k+1)-th y (planted ties and the one planted equality excepted: trunc_ref's
    docstring), so tests/test_trunc_gpu.py skips nothing;
  * the kept sets against transformers' TopKLogitsWarper + TopPLogitsWarper on the tie-free rows;
  * a chi-square test of 2^18 restated draws against the float64 truncated distribution;
  * every mutant of trunc_ref.MUTANTS changes a token or a kept set or moves a score by >= 100 x tolerance on some case;
  * the end-to-end oracle: for the (top_k, top_p, T, seed) tests/test_trunc_e2e_gpu.py uses, the float64 restatement of the fixtures'
    own hidden rows exempts at most 10 % of the tokens (trunc_e2e_settings).
"""
import math

import numpy as np
import pytest
import torch

import trunc_ref as R
from util import load_golden

CASES = R.cases()
SMALL = [c for c in CASES if c.n_part <= 5]


def test_the_grid_covers_what_the_issue_lists():
    grid = [c for c in CASES if c.name == "grid"]
    assert {c.n_part for c in grid} == set(R.N_PARTS) and {c.c for c in grid} == {1, 8} and {c.B for c in grid} == set(R.BS)
    assert {(c.k, c.p) for c in grid} == {(k, p) for k in R.KS for p in R.PS}
    assert {(c.n_part, c.c, c.k, c.p) for c in grid} == {(n, c, k, p) for n in R.N_PARTS for c in (1, 8) for k in R.KS for p in R.PS}
    for n in R.N_PARTS:
        assert {c.B for c in grid if c.n_part == n} == set(R.BS), n
    kept = {len(e["kept"]) for c in CASES for e in c.restate()}
    assert kept >= {0, 1, 2, 3, 5, 8}, kept
    assert any(c.count for c in CASES) and len(CASES) < 200


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_restatement_against_float64_and_decisive_gaps(case):
    for b, ((kept, tok, lp, gaps), e) in enumerate(zip(case.reference(), case.restate())):
        assert [i for _, i in e["kept"]] == kept and e["token"] == tok, (case.id, b, kept, e["kept"], tok, e["token"])
        if tok < 0:
            assert math.isnan(lp) and math.isnan(e["score"]) and not kept
            continue
        assert abs(e["score"] - lp) <= R.TOL_CPU, (case.id, b, e["score"], lp)
        assert gaps["z"] >= 100 * gaps["tol_z"], (case.id, b, gaps)
        if not case.planted_equality:
            assert gaps["c"] >= 100 * gaps["tol_c"], (case.id, b, gaps)
        if not (case.planted_tie or case.planted_equality):
            assert gaps["yk"] >= 0.125, (case.id, b, gaps)
        # the partial row: kept entries first, the owns-nothing partial behind them
        n = len(kept)
        assert e["pi"][:n].tolist() == kept and e["pi"][n:].tolist() == [R.NONE] * (R.C - n)
        assert e["ps"].tolist() == [1.0] * n + [0.0] * (R.C - n) and bool(np.isneginf(e["pm"][n:]).all()) and bool(np.isneginf(e["pv"][n:]).all())
        assert e["pr"][:n].tolist() == e["pm"][:n].tolist() and e["pr"][n:].tolist() == [0.0] * (R.C - n)
    if case.planted_tie:
        for b in range(case.B):
            top = R.select(case.cv[b], case.ci[b], case.k + 1)
            assert top[case.k - 1][0] == top[case.k][0] and top[case.k - 1][1] < top[case.k][1]
    if case.planted_equality:
        assert all(len(e["kept"]) == 1 for e in case.restate()) and all(len(e["kept"]) == 2 for e in case.restate("nucleus_le"))


def test_kept_sets_against_the_transformers_warpers():
    tf = pytest.importorskip("transformers")
    from transformers.generation.logits_process import TopKLogitsWarper, TopPLogitsWarper
    checked = 0
    for case in SMALL:
        if case.planted_tie or case.planted_equality or case.name == "absorbed-tail":
            continue
        for b, e in enumerate(case.restate()):
            v, i = R.listable(case.cv[b], case.ci[b])
            if len(v) == 0:
                continue
            row = torch.full((1, int(i.max()) + 1), -float("inf"))
            row[0, torch.from_numpy(i)] = torch.from_numpy(v)
            out = TopKLogitsWarper(top_k=case.k)(None, row.clone())
            if case.p < 1.0:
                out = TopPLogitsWarper(top_p=case.p)(None, out)
            hf = sorted(torch.nonzero(torch.isfinite(out[0])).reshape(-1).tolist())
            assert hf == sorted(c for _, c in e["kept"]), (case.id, b, hf, e["kept"])
            checked += 1
    assert checked >= 100 and tf is not None


def _chi2_critical(df, z=4.7534):
    """Wilson-Hilferty quantile of chi-square(df) at the upper tail 1e-6 (z = the normal quantile)"""
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


@pytest.mark.parametrize("k,p", [(8, 1.0), (4, 1.0), (8, 0.55)])
@pytest.mark.parametrize("T", [1.0, 0.5])
def test_restated_draws_follow_the_truncated_distribution(k, p, T):
    n = 1 << 18
    x = np.array([12.0, 11.75, 11.5, 11.0, 10.75, 10.25, 10.0, 9.5, 9.25, 9.0, 3.0, 2.0], dtype=np.float64)
    cols = np.array([901, 17, 4000, 3, 77, 5, 1300, 256, 255, 9, 11, 12])
    y = (x.astype(np.float32) * np.float32(1.0 / T)).astype(np.float32)
    kept, counts = R.sample_many(y, cols, k, p, seed=0xD157 + k, stream=2, n_draws=n)
    # float64 truncated distribution from the definitions
    order = np.lexsort((cols, -y.astype(np.float64)))[:k]
    yy = y.astype(np.float64)[order]
    cum = np.cumsum(np.exp(yy - yy[0]))
    keep = [0] + [j for j in range(1, k) if p >= 1.0 or cum[j - 1] < p * cum[-1]]
    assert cols[order][keep].tolist() == kept.tolist()
    prob = np.exp(yy[keep] - yy[0])
    prob /= prob.sum()
    assert len(keep) >= 2 and counts.sum() == n
    chi2 = float((((counts - n * prob) ** 2) / (n * prob)).sum())
    assert chi2 <= _chi2_critical(len(keep) - 1), (k, p, T, chi2, counts.tolist(), (n * prob).tolist())


def _differs(case, mut):
    """does the mutant change a token or a kept set, or move a score by >= 100 x tolerance, on some row of the case?"""
    for a, b in zip(case.restate(), case.restate(mut)):
        if a["token"] != b["token"] or [i for _, i in a["kept"]] != [i for _, i in b["kept"]]:
            return True
        if not math.isnan(a["score"]) and not abs(a["score"] - b["score"]) < 100 * R.TOL:
            return True
    return False


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_caught(mut):
    hits = [c.id for c in SMALL if _differs(c, mut)]
    assert hits, mut
    if mut == "no_shortcut":
        assert any("absorbed-tail" in h for h in hits)


def test_absorbed_tail_is_absorbed():
    case = next(c for c in CASES if c.name == "absorbed-tail")
    e = case.restate()[0]
    y = [v for v, _ in e["kept"]]
    assert len(y) == 8 and y[7] == y[0] - 40
    acc = np.float32(0)
    for v in y[:7]:
        acc = np.float32(acc + R.lse_exp(v - y[0]))
    assert np.float32(acc + R.lse_exp(y[7] - y[0])) == acc


# ------------------------------------------------------------------------------------------------------------ the end-to-end oracle
def test_e2e_settings_exempt_at_most_a_tenth_of_the_fixture_tokens():
    """tests/test_trunc_e2e_gpu.py compares every token with the float64 restatement of the engine's own tap row wherever the three gaps
    exceed the a-priori dot bound.  Here the same count on the fixtures' recorded hidden rows (the oracle's, which the fp32 engine meets
    to 1e-3): the chosen settings leave at most 10 % of the tokens under the bound."""
    import trunc_e2e as E
    from scenarios import SCENARIOS
    for name in E.FIXTURES:
        g, Wd, pen = load_golden(name), E.fixture_head(name), SCENARIOS[name].get("rep_penalty", 1.0)
        for (k, p, T, seeds) in E.SETTINGS:
            stats, kept = dict(tokens=0, under=0), set()
            for seed in seeds:
                t = draw = 0
                while f"t{t}_hidden" in g:
                    hid, ids = np.asarray(g[f"t{t}_hidden"], dtype=np.float64), g[f"t{t}_ids"].tolist()
                    for r in range(hid.shape[0]):
                        _, cols, _, _, _ = E.restate_token(Wd, hid[r], ids[:r], pen, k, p, T, seed, 0, draw, stats)
                        kept.add(len(cols))
                        draw += 1
                    t += 1
            assert stats["tokens"] >= 36 and stats["under"] <= 0.10 * stats["tokens"], (name, k, p, T, stats)
            assert p >= 1.0 or T < 1.0 or max(kept) < k, (name, k, p, T, kept)        # the nucleus bites where it is meant to
