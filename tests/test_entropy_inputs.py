"""CPU proof that the cases of tests/entropy_ref.py are sharp (svln_token_entropy; no GPU):

  * the fp32 restatement of the three producers and of the merge, in the kernels' operation order, stays inside the derived tolerance
    against float64 on every CPU case, greedy and sampled; the N = 1 cases give exactly 0;
  * the design bounds the tolerance is stated in (a, q, log S, H) hold for every case of the GPU tables, in float64;
  * every mutant of KIND_MUTANTS moves some case of its kind by >= 100 x the tolerance (or to NaN);
  * the merge's edge rules on hand-made partials: empty partials between live ones, a -inf-only row, a NaN partial, n equal single-id
    partials.
"""
import math

import numpy as np
import pytest

import entropy_ref as E

F = np.float32
_BASE = {}


def _base(c, sampled):
    key = (c.id, sampled)
    if key not in _BASE:
        _BASE[key] = [h for h, _ in c.restate(sampled)]
    return _BASE[key]


def test_tolerance_is_the_derived_one():
    u, L, R, a, q, ls, H = 2.0 ** -24, 56, 42, E.A_MAX, E.Q_MAX, E.LOGS_MAX, E.H_MAX
    assert (E.L_MAX, E.R_MAX) == (L, R)
    assert E.TOL == u * ((2 + L + 5 * R + 4 * a) * (1 + a) + (3 + L + 5 * R) * a + 4 * q + 3 * ls + 2 * (a + H))
    assert 1e-4 < E.TOL < 2e-4


def test_design_bounds_hold_for_every_case():
    for c in E.rows_cases() + E.batched_cases() + E.mfma_cases():
        for sampled in (False, True):
            y = c.y(sampled)
            for b in range(c.B):
                a, q, ls, H = E.moments(y[b])
                assert a <= E.A_MAX and q <= E.Q_MAX and ls <= E.LOGS_MAX and H <= E.H_MAX, (c.id, sampled, b, a, q, ls, H)


@pytest.mark.parametrize("case", E.cpu_cases(), ids=lambda c: c.id)
def test_restatement_is_inside_the_tolerance(case):
    for sampled in (False, True):
        ref = case.reference_entropy(sampled)
        got = _base(case, sampled)
        for b in range(case.B):
            assert E.moved(got[b], ref[b]) <= E.TOL, (case.id, sampled, b, got[b], ref[b])
            if case.N == 1:
                assert got[b] == 0.0 and ref[b] == 0.0, (case.id, sampled, b, got[b])


@pytest.mark.parametrize("kind,mut", [(k, m) for k in ("rows", "batched", "mfma") for m in E.KIND_MUTANTS[k]])
def test_every_mutant_moves_a_case(kind, mut):
    assert mut in E.MUTANTS
    best = 0.0
    for c in E.cpu_cases():
        if c.kind != kind or c.N > 9000:
            continue
        for sampled in ((True,) if mut == "t_on_z" else (False, True)):
            got = [h for h, _ in c.restate(sampled, mut)]
            best = max(best, max(E.moved(a, b) for a, b in zip(got, _base(c, sampled))))
        if best >= 100 * E.TOL:
            return
    assert best >= 100 * E.TOL, (kind, mut, best)


def test_every_mutant_is_assigned_to_a_kind():
    assert set(E.MUTANTS) == set(m for k in E.KIND_MUTANTS.values() for m in k)


def test_merge_edge_rules():
    NEG = E.NEG
    live = (F(3.0), F(1.5), F(-0.25))
    empty = (NEG, F(0), F(0))
    h0, _ = E.merge([live, (F(2.0), F(1.0), F(0.0))])
    h1, _ = E.merge([empty, live, empty, empty, (F(2.0), F(1.0), F(0.0)), empty])
    assert h0 == h1 and not math.isnan(h0)
    assert math.isnan(E.merge([empty, empty])[0])                       # a -inf-only row
    assert math.isnan(E.merge([live, (F(1.0), F(np.nan), F(np.nan))])[0])
    assert math.isnan(E.merge([empty, live], "empty_nan")[0])           # (the guard is what keeps the empty partial out)
    for n in (1, 2, 255, 256, 257, 2048):
        h, _ = E.merge([(F(1.25), F(1), F(0))] * n)
        assert abs(h - math.log(n)) <= E.TOL, (n, h)
    assert E.merge([(F(1.25), F(1), F(0))])[0] == 0.0
