"""The inputs of tests/test_forced_gpu.py are sharp (no GPU): on the cases of tests/forced_ref.py the fp32 restatement of the partial /
capture / merge scheme of both EPI_TARGET forms stays within 2e-6 of float64 on every case, a row whose target is its own arg-max gets
the same bits for both scores, the capture array is exact (the canary everywhere no column was named), and every mutant -- one plausible
kernel mistake each -- moves a log-probability or a capture slot of at least one case by >= 100 x the GPU tolerance."""
import math

import numpy as np
import pytest
import torch

import forced_ref as R

CASES = R.cpu_cases()


def _moved(got, ref):
    if math.isnan(ref):
        return not math.isnan(got)
    return not abs(got - ref) < 100 * R.TOL            # (NaN / inf count as moved)


@pytest.fixture(scope="module")
def refs():
    return {c.id: c.reference() for c in CASES}


def test_designed_operands_give_the_designed_logits():
    """W . x_b is L[b] exactly with fp32 and with bf16 operands; y = l * inv_t and y_t - V are exact in fp32"""
    for c in [c for c in R.mfma_cases() if c.N == 129] + [c for c in R.gemv_cases() if c.N in (5, 7)]:
        x, W = c.operands()
        L, tgt = c.logits()
        assert torch.equal(W.double(), W.to(torch.bfloat16).double()) and torch.equal(x, x.to(torch.bfloat16).double()), c.id
        assert torch.equal((x.float() @ W.float().T).double(), L), c.id
        y = L * c.inv_t
        assert torch.equal(y.float().double(), y) and float(L.abs().max()) <= 35.5, c.id
        assert bool((L * 2 == (L * 2).round()).all()) and float((y.max(1).values[:, None] - y).max()) <= 150, c.id


def test_cases_cover_the_named_places():
    mf, gv = R.mfma_cases(), R.gemv_cases()
    assert len({c.id for c in mf + gv}) == len(mf + gv), "duplicate case ids"
    for fmt in ("plain-fp32", "plain-bf16"):
        mine = [c for c in mf if c.fmt == fmt]
        assert {(c.B, c.live, c.N) for c in mine} >= {(M, l, N) for M, l in ((3, 3), (4, 3), (4, 4), (5, 5), (8, 8), (17, 17), (32, 32)) for N in R.MFMA_N}
        assert {c.inv_t for c in mine} == set(R.INV_TS) and max(R.MFMA_N) > 3 * 128 - 1
        named = set()
        for c in mine:
            if c.N == 391:
                named |= {t for t in c.logits()[1] if t >= 0}
        assert named >= set(R.mfma_places(391)), sorted(set(R.mfma_places(391)) - named)
        assert {0, 127, 128, 390} <= named
        # both lane halves, r32 of 0 and 31 and both j are someone's target row / column; a -1 sits in front of a canary
        assert any(R.acc_row(r, 32) == b for c in mine for b, t in enumerate(c.logits()[1]) if t >= 0 for r in range(16))
        assert any(-1 in c.logits()[1][:c.live] for c in mine) and any(c.live < c.B for c in mine)
        assert any(t >= 0 and t == int(torch.argmax(c.logits()[0][b])) for c in mine for b, t in enumerate(c.logits()[1]))
        g = [c for c in gv if c.fmt == fmt]
        assert {(c.B, c.N % 4) for c in g} == {(B, q) for B in (2, 4, 8) for q in range(4)} and {c.inv_t for c in g} == set(R.INV_TS)
        for N in (8196, 8197, 8198, 8199):          # the grid strides: workgroup 0 visits unit 0 and unit 2048
            assert (N + 3) // 4 > 2048
            named = set()
            for c in g:
                if c.N == N:
                    named |= {t for t in c.logits()[1] if t >= 0}
            assert named & {8192 + r for r in range(4)} and (N - 1) in named, (N, sorted(named))
        named = set()
        for c in g:
            named |= {t % 4 for t in c.logits()[1] if t >= 0}
        assert named == {0, 1, 2, 3}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_restatement_matches_the_reference(case, refs):
    tok, glp, lp = refs[case.id]
    got, slots = case.restate()
    L, tgt = case.logits()
    assert np.array_equal(slots, case.expected_slots()), (case.id, slots, case.expected_slots())
    for b in range(case.B):
        g_tok, g_glp, g_lp = got[b]
        assert g_tok == int(tok[b]), (case.id, b, g_tok, int(tok[b]))
        assert abs(g_glp - float(glp[b])) <= 2e-6, (case.id, b, g_glp, float(glp[b]))
        if tgt[b] < 0:
            assert math.isnan(g_lp), (case.id, b, g_lp)
            continue
        assert abs(g_lp - float(lp[b])) <= 2e-6, (case.id, b, g_lp, float(lp[b]))
        if tgt[b] == g_tok:                            # target == arg-max: the two scores are the same bits
            assert np.float32(g_lp).tobytes() == np.float32(g_glp).tobytes(), (case.id, b, g_lp, g_glp)


@pytest.mark.parametrize("kind", sorted(R.KIND_MUTANTS))
def test_every_mutant_moves_a_case(kind, refs):
    mine = [c for c in CASES if c.kind == kind]
    for mut in R.KIND_MUTANTS[kind]:
        hit = []
        for c in mine:
            _, _, lp = refs[c.id]
            got, slots = c.restate(mut)
            exp = c.expected_slots()
            if any(_moved(got[b][2], float(lp[b])) for b in range(c.B)) or any(_moved(float(a), float(e)) for a, e in zip(slots, exp)):
                hit.append(c.id)
                break                                  # one witness is the claim
        assert hit, f"{kind}: no case notices the mutant {mut}"
    assert set().union(*R.KIND_MUTANTS.values()) == set(R.MUTANTS)


def test_nan_and_inf_targets():
    """a NaN target logit gives NaN, a -inf target logit gives -inf, a row without a target NaN: none is an error"""
    L = torch.tensor([[1.0, float("-inf"), 0.5, -3.0, 2.0], [1.0, 0.0, 0.5, -3.0, 2.0]], dtype=torch.float64)
    got, _ = R.restate_gemv(L, [1, -1], 1.0)
    assert got[0][0] == 4 and got[0][2] == float("-inf") and math.isfinite(got[0][1])
    assert got[1][0] == 4 and math.isnan(got[1][2]) and math.isfinite(got[1][1])
    L[0, 1] = float("nan")
    got, _ = R.restate_gemv(L, [1, 4], 1.0)
    assert math.isnan(got[0][2]) and got[1][2] == got[1][1]
