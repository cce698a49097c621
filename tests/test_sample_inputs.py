"""CPU proof of the sampling test inputs (svln_set_sampling, tests/sample_ref.py): the restated noise is Philox4x32-10, the restated
sampler draws from softmax(l / T), every op-level case keeps its two best perturbed values >= 100 tolerances apart (so the GPU test skips
none), the correct restatement reproduces the float64 reference, and every mutant is caught by some case.

One mutant of the issue's list cannot exist: "the penalty applied after the temperature".  HF's penalty (x < 0 ? x * p : x / p) is
positively homogeneous and 1 / T > 0, so pen(x) / T = pen(x / T) in exact arithmetic; on these exact inputs (penalty 2, T a power of two)
the two orders agree bit for bit, which test_penalty_commutes_with_the_temperature asserts.  The ordering mistake that does change the
distribution, the penalty applied after the NOISE, stands in for it (mutant pen_after_noise)."""
import math

import numpy as np
import pytest

import sample_ref as R
from util import load_golden


# ------------------------------------------------------------------------------------------------ (a) the noise
def _philox_ints(c, k):
    """an independent straight-line Philox4x32-10 on Python ints: all four output words"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


# the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors: counter, key -> output)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))


def test_philox_known_answers_and_independent_restatement():
    for c, k, out in KAT:
        assert tuple(_philox_ints(c, k)) == out
        assert int(R.philox4x32_10(*c, *k)) == out[0]
    rng = np.random.default_rng(5)
    for _ in range(200):
        c = [int(v) for v in rng.integers(0, 1 << 32, 4)]
        k = [int(v) for v in rng.integers(0, 1 << 32, 2)]
        assert int(R.philox4x32_10(*c, *k)) == _philox_ints(c, k)[0]
    cols = np.arange(1000)
    w = R.noise_bits(0x0123456789ABCDEF, 5, 77, cols)
    assert [int(v) for v in w[:50]] == [_philox_ints((n, 77, 5, 0), (0x89ABCDEF, 0x01234567))[0] for n in range(50)]


def test_uniform_is_exact_in_fp32_and_open():
    w = np.array([0, 0x1FF, 0x200, 0xFFFFFFFF, 0xFFFFFE00, 0x80000000], dtype=np.uint64)
    u = R.uniform(w)
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24
    g = R.gumbel(1, 0, 0, np.arange(4096))
    assert np.isfinite(g).all() and g.max() < 16.7 and g.min() > -2.9          # G in [-ln(24 ln 2), -ln(2^-24 (1 + ..))]
    assert R.uniform24_fp32(np.array([0xFFFFFFFF], dtype=np.uint64))[0] == 1.0   # the 24-bit mistake


# ------------------------------------------------------------------------------------------------ (b) the distribution
@pytest.mark.parametrize("T", R.TEMPS)
def test_restated_sampler_draws_from_the_softmax(T):
    """2^20 restated draws at N = 16, seed 0x5EED, stream 2: chi-square of the token histogram against softmax(l / T), p >= 0.01
    (15 degrees of freedom: the 99th percentile is 30.58)"""
    N, draws = 16, 1 << 20
    l = np.array([0.0, -0.5, 1.0, 2.5, -3.0, 0.5, 1.5, -1.0, 2.0, 0.0, -2.0, 3.0, 1.0, -0.5, 0.5, -1.5])
    y = (l.astype(np.float32) * np.float32(1.0 / T)).astype(np.float64)
    g = R.gumbel(0x5EED, 2, np.arange(draws)[:, None], np.arange(N)[None])
    tok = np.argmax(y[None] + g, axis=1)
    hist = np.bincount(tok, minlength=N)
    p = np.exp(y - y.max())
    p /= p.sum()
    chi2 = float(((hist - draws * p) ** 2 / (draws * p)).sum())
    print(f"T = {T}: chi-square {chi2:.2f} on 15 degrees of freedom")
    assert chi2 <= 30.58


# ------------------------------------------------------------------------------------------------ (c) margins, (d) mutants
CASES = R.all_cases()


def test_every_case_keeps_its_margin():
    """the top-2 perturbed margin of every row of every op-level case is >= 100 x its tolerance at the case's seed: no GPU case skips"""
    for c in CASES + [R.u24_case()]:
        worst = min(m / t if t > 0 else float("inf") for _, _, m, t in c.reference())
        assert worst >= 100, (c.id, worst)
    assert len({c.id for c in CASES}) == len(CASES)


def test_sampled_tokens_are_not_the_greedy_ones():
    """the noise decides: in most rows the sampled token differs from the arg-max of the processed logits, and the two rows of a pair
    (same logits, another stream and draw) sample differently somewhere"""
    greedy = sampled = pairs = differ = 0
    for c in CASES:
        ref = c.reference()
        for b in range(c.B):
            x, fr = c.row_inputs(b)
            p = x if fr is None else np.where(fr.astype(bool), np.where(x < 0, x * R.PEN, x / R.PEN), x)
            sampled += 1
            greedy += ref[b][0] == int(np.argmax(p))
        for b in range(0, c.B - 1, 2):
            if c.N > 1:
                pairs += 1
                differ += ref[b][0] != ref[b + 1][0]
    assert greedy < sampled / 2 and differ > pairs / 2, (greedy, sampled, differ, pairs)


def test_rows_that_share_their_logits_sample_differently():
    """rows 0 and 1 of every MFMA case with M >= 2 and N = 645 hold the same logits and the same penalty-free or penalised values up to their flag
    rows; stream and draw differ.  The reference tokens differ in every such case: the GPU test asserts it on the kernel's tokens."""
    n = 0
    for c in R.mfma_cases():
        if c.B >= 2 and c.N == 645:
            L, _, _ = c.logits()
            assert bool((L[0] == L[1]).all()) and (c.streams[0], c.draws[0]) != (c.streams[1], c.draws[1])
            ref = c.reference()
            assert ref[0][0] != ref[1][0], c.id
            n += 1
    assert n >= 6


def test_committed_tail_pairs_are_what_the_search_finds():
    """tests/golden/sample_tail_pairs.json against a re-run of the first draws of the committed search (sample_ref.search_tail_pairs)"""
    import json
    import os
    from util import GOLD
    t = json.load(open(os.path.join(GOLD, "sample_tail_pairs.json")))
    got = R.search_tail_pairs(t["seed"], t["stream"], want=2)
    assert got["upper"] == t["upper"][:2] and got["lower"] == t["lower"][:2]
    for name, test in (("upper", lambda u: u > 1 - 2.0 ** -20), ("lower", lambda u: u < 2.0 ** -20)):
        assert len(t[name]) == 72
        for draw, col in t[name]:
            assert test(R.uniform(R.noise_bits(t["seed"], t["stream"], draw, np.array([col])))[0])


@pytest.mark.parametrize("case", R.cpu_cases(), ids=lambda c: c.id)
def test_restatement_matches_the_reference(case):
    for (tok, lp), (rt, rl, _, _) in zip(case.restate(), case.reference()):
        assert tok == rt, (case.id, tok, rt)
        assert (math.isnan(lp) and math.isnan(rl)) or abs(lp - rl) <= R.TOL, (case.id, lp, rl)


def _moved(case, mut):
    """does mutant `mut` change a token of `case`, or move a score by >= 100 tolerances (a NaN counts)"""
    for (tok, lp), (rt, rl, _, _) in zip(case.restate(mut), case.reference()):
        if tok != rt or math.isnan(lp) != math.isnan(rl) or abs(lp - rl) >= 100 * R.TOL:
            return True
    return False


@pytest.mark.parametrize("kind", sorted(R.KIND_MUTANTS))
def test_every_mutant_is_caught(kind):
    cases = [c for c in R.cpu_cases() if c.kind == kind]
    for mut in R.KIND_MUTANTS[kind]:
        caught = [c.id for c in cases if _moved(c, mut)]
        print(f"{kind} / {mut}: caught by {len(caught)} of {len(cases)} cases")
        assert caught, (kind, mut)
    assert set(m for ms in R.KIND_MUTANTS.values() for m in ms) | {"u24"} == set(R.MUTANTS)


def test_u24_mutant_is_caught():
    """24 random bits: the column the search found has w >> 8 = 2^24 - 1, so fp32 rounds u to 1 and G to +inf: that column wins"""
    c = R.u24_case()
    w = R.noise_bits(c.seed, c.streams[0], c.draws[0], np.array([R.U24_COLUMN]))
    assert int(w[0]) >> 8 == 0xFFFFFF
    assert c.restate()[0][0] == c.reference()[0][0]
    assert c.restate("u24")[0][0] == R.U24_COLUMN != c.reference()[0][0]


def test_penalty_commutes_with_the_temperature():
    """pen(x) * invT == pen(x * invT) bit for bit on the exact inputs: the order cannot be told apart (see the module docstring)"""
    for c in R.cpu_cases():
        if not c.pen:
            continue
        for b in range(c.B):
            x, fr = c.row_inputs(b)
            x, f, it = x.astype(np.float32), fr.astype(bool), np.float32(c.inv_t)
            pen = lambda v: np.where(f, np.where(v < 0, v * np.float32(R.PEN), v / np.float32(R.PEN)), v).astype(np.float32)
            assert (pen(x) * it == pen(x * it)).all()


# ------------------------------------------------------------------------------------------------ the greedy limit (e2e test, T = 2^-14)
def test_recorded_greedy_margins_dwarf_the_noise_at_T_2_pow_minus_14():
    """tests/test_sample_e2e_gpu.py reproduces the greedy fixtures at T = 2^-14: the fixtures' recorded top-2 logit margins, scaled by
    2^14, must exceed the largest possible noise gap max G - min G = -ln(2^-24 ..) + ln(24 ln 2) < 19.5"""
    gap = -math.log(-math.log1p(-2.0 ** -24)) + math.log(-math.log(2.0 ** -24))
    assert gap < 19.5
    for name in ("tiny_episode", "tiny_penalty"):
        g = load_golden(name)
        margins = np.concatenate([g[f"t{t}_margins"] for t in range(int(g["n_turns"]))])
        print(f"{name}: smallest recorded top-2 margin {margins.min():.4f} -> {margins.min() * 2.0 ** 14:.1f} at T = 2^-14, noise gap < {gap:.2f}")
        assert margins.min() * 2.0 ** 14 > gap, (name, margins.min())
