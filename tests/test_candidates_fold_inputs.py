"""The bookkeeping of the folded candidates call, restated cell by cell (tests/candidates_fold_ref.py; no GPU): over L % 64 in
{0, 1, 61, 63}, P on both sides of 64 q0, G = 2 .. 8 and every length vector in 1 .. 6 at G = 2 and 3, every fork's page q0 ends holding
the env's rows [64 q0, L) followed by its own branch rows, no branch writes a shared page, the env's pages are written by the prompt and
sequence 0 only, pages are conserved, and the head-row list maps F_g[i] to the row that was fed F_g[i - 1].  Each mutant -- a way to get
the fold wrong -- breaks an invariant on some input of the same sweep."""
import itertools

import pytest

import candidates_fold_ref as F

RESIDUES = (0, 1, 61, 63)


def _histories(L):
    """P on both sides of 64 q0 (and on it), below L"""
    q0 = L // F.PAGE
    return sorted({p for p in (0, q0 * F.PAGE - 5, q0 * F.PAGE, q0 * F.PAGE + 1, q0 * F.PAGE + 40) if 0 <= p < L})


def _length_vectors():
    for G in (2, 3):
        yield from itertools.product(range(1, 7), repeat=G)
    for G in range(4, 9):
        yield tuple(1 + (3 * g + G) % 6 for g in range(G))            # ragged, ones among them
        yield (6,) * G
        yield (2,) + (1,) * (G - 2) + (6,)


def _inputs():
    for res in RESIDUES:
        L = 128 + res
        for P in _histories(L):
            for lens in _length_vectors():
                if max(lens) >= 2:                                    # (all ones: nothing is fed, the unfolded call runs)
                    # q heads per kv head: 2 (r = 16, 10, 8, ...) everywhere; 7 (r = 4: fold + a remaining pass) where a candidate has 6 ids
                    for q_per_kv in ((2, 7) if max(lens) == 6 and (len(lens) > 3 or min(lens) >= 5) else (2,)):
                        yield L, P, lens, q_per_kv


def test_the_sweep_covers_what_it_claims():
    seen = list(_inputs())
    assert {L % 64 for L, *_ in seen} == set(RESIDUES)
    assert {len(lens) for _, _, lens, _ in seen} == set(range(2, 9))
    assert sum(1 for L, P, lens, q in seen if (L, P, q) == (189, 0, 2) and len(lens) == 3) == 6 ** 3 - 1
    for L in (129, 189, 191):                                         # (L = 129: page q0 holds one row, so no history ends inside it)
        q0 = L // 64
        assert any(P > q0 * 64 for l, P, *_ in seen if l == L) == (L != 129) and any(0 < P < q0 * 64 for l, P, *_ in seen if l == L)
        assert any(P == q0 * 64 for l, P, *_ in seen if l == L)
    assert F.rows_per_pass(8, 2) == 4 and F.rows_per_pass(3, 2) == 10 and F.rows_per_pass(2, 7) == 4      # a candidate of 6 ids: fold + one pass


def test_invariants_hold_on_every_input():
    n = 0
    for L, P, lens, q in _inputs():
        s = F.simulate(L, P, lens, q_per_kv=q)
        assert F.check(s), (L, P, lens, q)
        # the mirror list is empty on a full last page, and the one copy runs only behind a history that ends inside page q0
        mirrors = [w for w in s.log if w[0] == "mirror"]
        copies = [w for w in s.log if w[0] == "copy"]
        assert bool(mirrors) == (L % 64 != 0 and bool(s.tails)), (L, P, lens)
        assert bool(copies) == (L % 64 != 0 and bool(s.tails) and P > s.q0 * 64), (L, P, lens)
        assert all(s.q0 * 64 <= w[3][1] < L for w in mirrors)
        n += 1
    assert n > 4000, n


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_every_mutant_breaks_an_invariant(mutant):
    caught = clean = 0
    for L, P, lens, q in _inputs():
        try:
            F.check(F.simulate(L, P, lens, q_per_kv=q, mutant=mutant))
            clean += 1
        except AssertionError:
            caught += 1
    assert caught > 0, f"{mutant}: no input of the sweep shows it"
    print(f"{mutant}: caught on {caught} inputs, invisible on {clean}")


def test_where_each_mutant_shows():
    """the inputs that need each part of the rule"""
    bad = lambda **kw: pytest.raises(AssertionError, lambda: F.check(F.simulate(**kw)))
    ok = lambda **kw: F.check(F.simulate(**kw))
    # the copy matters only behind a history that ends inside page q0
    bad(L=189, P=168, lens=(3, 3), mutant="no_precopy")
    ok(L=189, P=128, lens=(3, 3), mutant="no_precopy")
    bad(L=189, P=168, lens=(3, 3), mutant="precopy_after")
    # rows of page q0 - 1 must not reach the forks' pages
    bad(L=189, P=100, lens=(3, 3), mutant="mirror_below_q0")
    ok(L=189, P=128, lens=(3, 3), mutant="mirror_below_q0")
    bad(L=128, P=0, lens=(3, 3), mutant="mirror_full_page")
    ok(L=129, P=0, lens=(3, 3), mutant="mirror_full_page")
    bad(L=189, P=0, lens=(1, 2), mutant="slot_pos_plus_1")
    bad(L=189, P=0, lens=(1, 2), mutant="src_rows_not_offset")
