"""CPU proof of the inputs of tests/test_topk_gpu.py / tests/test_topk_e2e_gpu.py (svln_top_logprobs; tests/topk_ref.py):

  * the fp32 restatement of the candidate scheme and the merge equals the float64 reference on every case and k: ids equal,
    |logprob - float64| <= 2e-6 (the bound tests/test_scores_inputs.py uses);
  * every adjacent gap among a case's k + 1 best values is exactly 0 (a planted tie) or >= 100 x the GPU tolerance;
  * every mutant changes an id or moves a value by >= 100 x the tolerance on some case;
  * entry 0 of a greedy list is the token and its log-probability the score's bits; under sampling the emitted id's entry is, and some
    case's sampled id differs from entry 0;
  * fixture precondition of the end-to-end test: on tiny_episode and tiny_penalty at most 5 % of the adjacent pairs among ranks 1 .. 9 of
    the float64 logits lie at or under the a-priori bound 2 gamma_K max_n sum_k |w_nk h_k| of the fp32 dot product.
"""
import math

import numpy as np
import pytest
import torch

import subset_ref as SR
import topk_ref as R
from scenarios import SCENARIOS, SEED
from util import load_golden, synth_weights

CASES = R.all_cases()
BATCH_CASES = R.all_batch_cases()


def _same(a, b, tol):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_restatement_equals_float64(case):
    ks = R.KS if case.name in ("ties", "ragged", "subset") else (case.k,)
    for k in ks:
        ids, lps, gaps = case.reference(k)
        got = case.restate(k=k)
        assert got["ids"] == ids, (case.id, k, got["ids"], ids)
        worst = max([abs(a - b) for a, b in zip(got["logprobs"], lps) if math.isfinite(a) and math.isfinite(b)] + [0.0])
        assert all(_same(a, b, R.TOL_CPU) for a, b in zip(got["logprobs"], lps)), (case.id, k, worst, got["logprobs"], lps)
        assert all(g == 0.0 or g >= 100 * R.TOL for g in gaps), (case.id, k, gaps)
        # padding is (-1, -inf) and sits behind every listed entry
        n = sum(i >= 0 for i in ids)
        assert ids[n:] == [-1] * (k - n) and all(v == float("-inf") for v in got["logprobs"][n:])


@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: c.id)
def test_batch_restatement_equals_float64(case):
    """the batched GEMV (thread b's list over the workgroup's units) and the MFMA tiles (per-wave lists of 64 columns, merged per tile), row
    by row; entry 0 / the sampled id's entry is the score"""
    for k in (R.KS if case.name == "greedy" and case.N in (115, 129) else (case.k,)):
        for b, ((ids, lps, gaps), got) in enumerate(zip(case.reference(k), case.restate(k=k))):
            assert got["ids"] == ids, (case.id, b, k, got["ids"], ids)
            assert all(_same(a, r, R.TOL_CPU) for a, r in zip(got["logprobs"], lps)), (case.id, b, k, got["logprobs"], lps)
            assert all(g == 0.0 or g >= 100 * R.TOL for g in gaps), (case.id, b, gaps)
            if math.isnan(got["score"]):
                continue
            if not case.sampled:
                assert got["ids"][0] == got["token"] and np.float32(got["logprobs"][0]).tobytes() == np.float32(got["score"]).tobytes()
            elif got["token"] in got["ids"]:
                j = got["ids"].index(got["token"])
                assert np.float32(got["logprobs"][j]).tobytes() == np.float32(got["score"]).tobytes()
    if case.sampled:
        r0 = case.restate()[0]
        assert r0["token"] != r0["ids"][0], case.id


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "rows"], ids=lambda c: c.id)
def test_candidates_are_each_partials_best(case):
    """exactness: a partial's list is the C best (y, column) pairs of the columns it owns, in order, padded -- so a column of the row's
    top k is in the top k of the partial that owns it"""
    _, x, fr = case.logits()
    got = case.restate()
    y = R.processed64(x, fr, R.PEN) * case.inv_t
    part = R.R.layout("rows", case.N)[1][:case.N]
    for p, ent in enumerate(got["cand"]):
        own = [int(c) for c in np.flatnonzero(part == p) if y[c] > -np.inf]
        exp = sorted(own, key=lambda c: (-y[c], c))[:R.C]
        assert [i for _, i in ent] == exp + [R.NONE] * (R.C - len(exp)), (case.id, p)
        assert [float(v) for v, i in ent if i != R.NONE] == [float(y[c]) for c in exp]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_emitted_id_entry_is_the_score(case):
    if case.allowed is not None:
        return
    got = case.restate()
    if math.isnan(got["score"]):
        return
    if not case.sampled:
        assert got["ids"][0] == got["token"]
        assert np.float32(got["logprobs"][0]).tobytes() == np.float32(got["score"]).tobytes()
    elif got["token"] in got["ids"]:
        j = got["ids"].index(got["token"])
        assert np.float32(got["logprobs"][j]).tobytes() == np.float32(got["score"]).tobytes()


def test_some_sampled_id_differs_from_entry_0():
    hit = [c.id for c in CASES if c.sampled and c.allowed is None and c.restate()["token"] != c.restate()["ids"][0]]
    listed = [c.id for c in CASES if c.sampled and c.allowed is None and c.restate()["token"] in c.restate()["ids"][1:]]
    assert len(hit) >= 3 and listed, (hit, listed)


def _moved(a, b):
    if a["ids"] != b["ids"]:
        return True
    for u, v in zip(a["logprobs"], b["logprobs"]):
        if math.isnan(u) != math.isnan(v):
            return True
        if math.isnan(u):
            continue
        if math.isinf(u) or math.isinf(v):
            if u != v:
                return True
        elif abs(u - v) >= 100 * R.TOL:
            return True
    return False


@pytest.mark.parametrize("kind", sorted(R.KIND_MUTANTS))
def test_every_mutant_is_caught(kind):
    if kind in ("batched", "mfma"):
        cases = [c for c in BATCH_CASES if c.kind == kind]
        good = {c.id: c.restate() for c in cases}
        moved = lambda c, mut: any(_moved(a, b) for a, b in zip(c.restate(mut=mut), good[c.id]))
    else:
        cases = [c for c in CASES if c.kind == kind]
        good = {c.id: c.restate() for c in cases}
        moved = lambda c, mut: _moved(c.restate(mut=mut), good[c.id])
    for mut in R.KIND_MUTANTS[kind]:
        caught = [c.id for c in cases if moved(c, mut)]
        assert caught, (kind, mut)
    assert set(m for ms in R.KIND_MUTANTS.values() for m in ms) == set(R.MUTANTS)


def test_case_coverage():
    rows = [c for c in CASES if c.kind == "rows"]
    assert {c.N % 4 for c in rows} == {0, 1, 2, 3}
    assert {c.k for c in CASES} >= set(R.KS)
    assert {c.T for c in rows if c.sampled} == {1.0, 0.5, 2.0}
    assert {c.fmt for c in rows} == {"plain-fp32", "plain-bf16", "e4m3", "mxfp4"}
    assert {len(c.allowed) for c in CASES if c.allowed is not None} >= {1, 3, 8, 9, 256}
    assert any(c.N < 16 and c.k == 8 for c in rows)                                   # fewer than k listable, waves without a column
    assert any(np.isnan(list(c.special.values())).any() for c in rows if c.special) and any(-np.inf in c.special.values() for c in rows)
    bat = [c for c in BATCH_CASES if c.kind == "batched"]
    mf = [c for c in BATCH_CASES if c.kind == "mfma"]
    assert {c.B for c in bat} == {1, 2, 4, 8} and {c.T for c in bat if c.sampled} == {1.0, 0.5, 2.0}
    assert {c.B for c in mf} >= {3, 4, 5, 8, 17, 32} and {c.N for c in mf} >= {127, 128, 129, 257, 391}
    assert {c.T for c in mf if c.sampled} == {1.0, 0.5, 2.0} and any(c.special for c in bat) and any(c.special for c in mf)
    for c in mf:                                                    # winners at a tile's first and last column and at N - 1
        planted = set(c.rows[0].plant)
        assert {0, c.N - 1} <= planted and (c.N <= 128 or {127, 128} <= planted), c.id


# ---------------------------------------------------------------------------------------------------------- end-to-end precondition
def fixture_pairs(name, hidden_of=None, k=8):
    """per emitted token of fixture `name`: (float64 logits [V], a-priori bound, the adjacent gaps among ranks 1 .. k + 1) from the
    fixture's (or the given) final-norm rows"""
    sc, g = SCENARIOS[name], load_golden(name)
    Wd = torch.from_numpy(np.asarray(synth_weights(sc["cfg"], SEED)["lm_head.weight"])).double()
    pen = sc.get("rep_penalty", 1.0)
    A = list(range(sc["cfg"].vocab))
    out = []
    for t, ids in enumerate(SR.fixture_ids(name)):
        hidden = g[f"t{t}_hidden"] if hidden_of is None else hidden_of(t)
        for y, bound in SR.restricted_rows(Wd, A, hidden, ids, pen):
            top = np.sort(y)[::-1][:k + 1]
            out.append((y, bound, top[:-1] - top[1:]))
    return out


@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_e2e_preconditions_hold_on_the_fixtures(name):
    rows = fixture_pairs(name)
    pairs = sum(len(g) for _, _, g in rows)
    close = sum(int((g <= b).sum()) for _, b, g in rows)
    print(f"{name}: {close} of {pairs} adjacent pairs among ranks 1 .. 9 at or under the bound "
          f"(smallest gap / bound {min(float((g / b).min()) for _, b, g in rows):.2f})")
    assert pairs >= 100 and close <= 0.05 * pairs, (name, close, pairs)
