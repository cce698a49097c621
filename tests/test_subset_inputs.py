"""CPU proof that the inputs of tests/test_subset_gpu.py and tests/test_subset_e2e_gpu.py are sharp, before any GPU sees them
(tests/subset_ref.py): the correct fp32 restatement reproduces the float64 reference (tokens equal, values inside TOL, exact cases exact),
every case keeps its top-2 margin >= 100 x TOL (planted ties are exact), every mutant changes a token or moves a value by >= 100 x TOL on
at least one case, and the end-to-end preconditions hold on the committed fixtures."""
import math

import numpy as np
import pytest

import torch

import subset_ref as R
from scenarios import SCENARIOS, SEED
from util import load_golden, synth_weights

CASES = R.all_cases()


def _moved(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, np.where((a == b), 0.0, d))     # (equal infinities have not moved)
    return float(np.nan_to_num(d, nan=np.inf).max()) if d.size else 0.0


def test_case_table_covers_the_ladders():
    for fmt in ("fp32", "bf16"):
        cs = [c for c in CASES if c.fmt == fmt]
        assert {c.K for c in cs} == set(R.k_ladder(fmt))
        assert {c.n for c in cs} >= set(R.N_LADDER) and {c.B for c in cs} == set(R.B_LADDER)
        assert any(c.T for c in cs) and any(c.pen and not c.T for c in cs) and any(c.pen and c.T for c in cs) and any(c.tie for c in cs)
        assert all(0 in c.ids() or c.n == 1 for c in cs) and all(R.V - 1 in c.ids() or c.n == 1 for c in cs)
        assert any(c.n == 1 and c.ids()[0] == 0 for c in cs) and any(c.n == 1 and c.ids()[0] == R.V - 1 for c in cs)
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_is_exact_sharp_and_restated(case):
    W, x = case.operands()
    ids = case.ids()
    assert (np.diff(ids) > 0).all() and 0 <= ids[0] and ids[-1] < R.V and 1 <= case.n <= 256
    inside = np.concatenate([W[ids, :case.K].ravel(), x[:, :case.K].ravel()])
    fin = inside[np.isfinite(inside)]
    assert (fin == np.round(fin)).all() and np.abs(fin).max() <= 4          # integers of [-4, 4]: partial sums < 2^24 at K <= 3584
    assert case.K * 16 < 2 ** 24
    assert np.isnan(W[:, case.K:]).all() and np.isnan(x[:, case.K:]).all()
    assert np.isnan(np.delete(W, ids, axis=0)).all()
    toks, scores, y, dist, margins = case.reference()
    # the designed logits are what the operands spell, in float64 and (bit for bit) in the fp32 restatement
    with np.errstate(all="ignore"):
        dots = x[:, :case.K] @ W[ids, :case.K].T
    raw = case.raw()
    assert np.array_equal(dots, raw)
    rt, rs, ry, rd = case.restate()
    assert np.array_equal(ry.astype(np.float64), y), case.id
    assert rt == toks, (case.id, rt, toks)
    for b in range(case.B):
        tie_ok = case.tie and not case.T and margins[b] == 0.0
        assert margins[b] >= 100 * R.TOL or tie_ok, (case.id, b, margins[b])
        if toks[b] < 0:
            assert math.isnan(rs[b])
        else:
            assert abs(rs[b] - scores[b]) <= R.TOL, (case.id, b, rs[b], scores[b])
    if case.tie and not case.T:
        assert any(m == 0.0 for m in margins)
    assert _moved(rd, dist) <= R.TOL, (case.id, _moved(rd, dist))


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_caught(mut):
    killed = []
    for case in CASES:
        toks, scores, y, dist, _ = case.reference()
        mt, ms, my, md = case.restate(mut)
        if mt != toks or _moved(my, y) >= 100 * R.TOL or _moved(md, dist) >= 100 * R.TOL or \
                _moved([s for s, t in zip(ms, toks) if t >= 0], [s for s, t in zip(scores, toks) if t >= 0]) >= 100 * R.TOL:
            killed.append(case.id)
    assert killed, mut
    print(f"{mut}: caught by {len(killed)} of {len(CASES)} cases")


# ---------------------------------------------------------------------------------------------------------- end-to-end preconditions
@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_e2e_preconditions_hold_on_the_fixtures(name):
    """containment: the allowed set holds every emitted id and fits the list; exclusion: up to and including the first token at which the
    fixture emits the removed id -- the rows the restricted run shares with the fixture -- every restricted top-2 margin exceeds the
    a-priori dot bound, and the restricted winner differs from the fixture's id exactly there"""
    sc, g = SCENARIOS[name], load_golden(name)
    A = R.allowed_set(name)
    assert 1 <= len(A) <= 256 and all(0 <= a < sc["cfg"].vocab for a in A) and R.REMOVED[name] in A
    assert set(R.PATHS_A) <= set(R.allowed_set("tiny_episode")) | set(R.allowed_set("tiny_penalty")) and list(R.PATHS_A) == sorted(R.PATHS_A)
    Wd = torch.from_numpy(np.asarray(synth_weights(sc["cfg"], SEED)["lm_head.weight"])).double()
    pen = sc.get("rep_penalty", 1.0)
    Ax = [a for a in A if a != R.REMOVED[name]]
    hit = False
    for t, ids in enumerate(R.fixture_ids(name)):
        full = R.restricted_rows(Wd, A, g[f"t{t}_hidden"], ids, pen)
        for k, (y, dot) in enumerate(full):                 # containment: the fixture's id is the restricted winner, by a margin above the bound
            top = np.sort(y)[::-1]
            assert A[int(np.argmax(y))] == ids[k] and top[0] - top[1] > dot, (name, t, k)
        cut = ids.index(R.REMOVED[name]) if R.REMOVED[name] in ids else len(ids) - 1
        for k, (y, dot) in enumerate(R.restricted_rows(Wd, Ax, g[f"t{t}_hidden"], ids[:cut + 1], pen)):
            top = np.sort(y)[::-1]
            assert top[0] - top[1] > dot, (name, t, k, float(top[0] - top[1]), dot)
            assert (Ax[int(np.argmax(y))] != ids[k]) == (ids[k] == R.REMOVED[name])
        if R.REMOVED[name] in ids:
            hit = True
            break
    assert hit
