"""The inputs of tests/test_scores_gpu.py are sharp (no GPU): on the cases of tests/scores_ref.py the fp32 restatement of the partial / merge
decomposition stays inside the op tolerance of the float64 reference on every case, and every mutant -- one plausible kernel mistake
each -- moves the expected log-probability of at least one case by >= 100 x that tolerance."""
import math

import pytest
import torch

import scores_ref as S

CASES = S.cpu_cases()


def _moved(got, ref):
    d = abs(got - ref)
    return not d < 100 * S.TOL            # (NaN / inf count as moved)


@pytest.fixture(scope="module")
def refs():
    return {c.id: c.reference() for c in CASES}


def test_designed_operands_give_the_designed_logits():
    """W . x_b is L[b] exactly, in fp32 and with every product rounded to bf16 operands, for every weight format's packing"""
    for c in [c for c in S.rows_cases(big=False) if c.N in (5, 113)] + [c for c in S.batched_cases() if c.N == 5] + [c for c in S.mfma_cases() if c.N == 129]:
        x, W = c.operands()
        L = c.logits()[0]
        assert torch.equal(W.double(), W.to(torch.bfloat16).double()) and torch.equal(x, x.to(torch.bfloat16).double()), c.id
        assert torch.equal((x.float() @ W.float().T).double(), L), c.id
        ops = S.pack(c.fmt, W)
        if c.fmt == "e4m3":
            assert torch.equal(ops["W"].view(torch.float8_e4m3fn).float(), W.float()), c.id
        if c.fmt == "mxfp4":
            import mxfp4_ref as MX
            assert torch.equal(MX.dequant_mxfp4(ops["W"], ops["aux"]).float(), W.float()), c.id
        Lp = c.processed()
        assert float((Lp.max(1).values[:, None] - Lp).max()) <= 80 and bool((Lp * 4 == (Lp * 4).round()).all()), c.id


def test_cases_cover_the_named_places():
    ids = {c.id for c in S.rows_cases() + S.batched_cases() + S.mfma_cases()}
    assert len(ids) == len(S.rows_cases() + S.batched_cases() + S.mfma_cases()), "duplicate case ids"
    rows = S.rows_cases()
    for fmt in S.G.FORMATS:
        mine = [c for c in rows if c.fmt == fmt]
        assert {c.N for c in mine} >= {1, 3, 5, 113, 20497} and len({c.K for c in mine}) == 2, fmt
        assert {c.pen for c in mine} == {True, False} and any(c.tie for c in mine), fmt
    assert sum(c.N == 152064 for c in rows) == 1
    assert S.G.iterations(20497, "argmax") == 2 and S.G.gemv_grid(20497) * 4 * 4 < 20497 < 2 * S.G.gemv_grid(20497) * 4 * 4
    bat = S.batched_cases()
    assert {(c.B, c.N) for c in bat} == {(B, N) for B in (1, 2, 4, 8) for N in (1, 5, 8193)}
    assert {(c.B, c.norm) for c in bat} == {(B, n) for B in (1, 2, 4, 8) for n in (True, False)} and {c.pen for c in bat} == {True, False}
    mf = S.mfma_cases()
    assert {(c.B, c.N) for c in mf} == {(M, N) for M in (4, 5, 31, 32) for N in (1, 127, 128, 129, 16385)} and {c.K for c in mf} == {576, 1024}
    for c in bat + mf:                       # distinct penalty rows per activation row
        if c.pen:
            rows_ = c.logits()[2]
            assert len(set(rows_)) == c.B, c.id


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_restatement_matches_the_reference(case, refs):
    tok, lp = refs[case.id]
    got = case.restate()
    for b in range(case.B):
        assert got[b][0] == int(tok[b]), (case.id, b, got[b][0], int(tok[b]))
        err = abs(got[b][1] - float(lp[b]))
        assert err <= S.TOL, (case.id, b, got[b][1], float(lp[b]), err)
        assert err <= 2e-6, (case.id, b, err)      # what the decomposition itself costs in fp32 with libm exp / log, far below the bound


@pytest.mark.parametrize("kind", sorted(S.KIND_MUTANTS))
def test_every_mutant_moves_a_case(kind, refs):
    mine = [c for c in CASES if c.kind == kind]
    for mut in S.KIND_MUTANTS[kind]:
        hit = []
        for c in mine:
            _, lp = refs[c.id]
            got = c.restate(mut)
            if any(_moved(got[b][1], float(lp[b])) for b in range(c.B)):
                hit.append(c.id)
        assert hit, f"{kind}: no case notices the mutant {mut}"
    assert set().union(*S.KIND_MUTANTS.values()) == set(S.MUTANTS)


def test_nan_and_no_finite_logit():
    """a NaN logit makes the score NaN; a row without a finite logit gives token -1 and NaN"""
    L = torch.tensor([1.0, float("nan"), 0.5, -3.0, 2.0], dtype=torch.float64)
    tok, lp = S.restate_rows(L)
    assert tok == 4 and math.isnan(lp)
    tok, lp = S.restate_rows(torch.full((7,), float("-inf"), dtype=torch.float64))
    assert tok == -1 and math.isnan(lp)
