"""The group turn's host rules on an exhaustive small table (no GPU): tests/group_ref.py restates the page bookkeeping (fork, decode writes,
select, drop) and the stream / draw rule; here every invariant is checked for L % 64 in {0, 1, 61, 63} at limit = 5 (61 and 63 cross a page
edge inside the turn, 0 needs no copy), every group size 2 .. 8, EVERY vector of sequence lengths in 1 .. 5, every selected index and a drop
instead of a select -- and every mutant of group_ref.MUTANTS must break an invariant on some case.  The end-to-end precondition of
tests/test_group_e2e_gpu.py (which token-0 samples of the fixtures sit under the a-priori margin bound) is proved at the end."""
import numpy as np
import pytest

import group_ref as GR
from scenarios import SCENARIOS, SEED
from util import load_golden, synth_weights

LIMIT = 5
RESIDUES = (0, 1, 61, 63)
PAGES_PER_ENV, MAX_ENVS = 8, 3          # 24 pages: env 1 holds a turn of its own beside the group of env 0
BASE = 2 * GR.PAGE                      # two full prompt pages below the partly filled one


def _violations(mutant, residues=RESIDUES, sizes=range(2, 9)):
    """names of the invariants that fail somewhere on the table"""
    bad = set()
    for r in residues:
        L = BASE + r
        for G in sizes:
            lengths = GR.length_vectors(G, LIMIT)
            # ---- fork
            pool = GR.Pool(PAGES_PER_ENV, MAX_ENVS, mutant)
            pool.ensure_pages(1, 100)                          # another env's pages
            other = set(pool.env_pages[1])
            free0 = len(pool.free)
            tabs = pool.fork(0, L, LIMIT, G)
            q0, nt = L // GR.PAGE, GR.n_tail_of(L, LIMIT)
            if pool.copy_launches != int(r != 0 and nt > 0):
                bad.add("one copy launch iff the prompt ends inside a page")
            if not pool.conserved():
                bad.add("no page has two owners")
            # every position a sequence may write (L .. L + limit - 2) maps to a page no other sequence and no other env can read
            for g in range(G):
                for pos in range(L, L + LIMIT - 1):
                    pg = tabs[g][pos // GR.PAGE]
                    if pg in other or any(pg in tabs[k] for k in range(G) if k != g):
                        bad.add("a written page is private to its sequence")
                    if pos // GR.PAGE < q0:
                        bad.add("no shared page is in a written slot")
            for g in range(1, G):                              # the shared prefix is the env's
                if tabs[g][:q0] != tabs[0][:q0]:
                    bad.add("forks share the prompt's full pages")
            # ---- decode rows, for every length vector at once
            W = GR.written(lengths, LIMIT, mutant)
            want = np.stack([lengths > t + 1 for t in range(LIMIT - 1)], -1)       # sequence g feeds its token t at position L + t iff it is live
            if not np.array_equal(W, want):
                bad.add("a sequence's table is written exactly at the positions of the tokens it fed")
            # ---- draws: the next turn's counter clears every stream of this one
            nxt = GR.advance(7, lengths, mutant)
            if not bool((nxt[:, None] >= 7 + lengths).all()):
                bad.add("no (stream, draw) pair is used twice")
            # ---- select every index / drop
            prompt = list(tabs[0][:q0])
            for choice in list(range(G)) + ["drop"]:
                p2 = GR.Pool(PAGES_PER_ENV, MAX_ENVS, mutant)
                p2.ensure_pages(1, 100)
                t2 = p2.fork(0, L, LIMIT, G)
                tail = list(t2[0][q0:q0 + nt]) if choice in (0, "drop") else list(p2.group["tails"][choice])
                if choice == "drop":
                    p2.drop()
                else:
                    p2.select(choice, [LIMIT] * G)
                if not p2.conserved():
                    bad.add("after select or drop no page has two owners and none is lost")
                if len(p2.free) != free0 - -(-(L + LIMIT - 1) // GR.PAGE):
                    bad.add("after select or drop the free count is the pool minus the env's own pages")
                if p2.env_pages[0][:q0] != prompt or p2.env_pages[0][q0:q0 + nt] != tail:
                    bad.add("the env's table maps the prompt pages plus the selected tail")
                if choice != "drop":
                    for n in range(1, LIMIT + 1):
                        p3 = GR.Pool(PAGES_PER_ENV, MAX_ENVS, mutant)
                        p3.fork(0, L, LIMIT, G)
                        p3.select(choice, [n] * G)
                        if p3.kv_len[0] != L + n - 1 or -(-p3.kv_len[0] // GR.PAGE) > len(p3.env_pages[0]):
                            bad.add("kv_len = L + n_out[index] - 1 lies inside the env's pages")
    # ---- streams and draws across sequences, turns and envs
    turns = [(0, [3, 5, 1, 2]), (1, [4]), (0, [2, 2, 5]), (2, [1, 5]), (1, [5, 1, 1, 1, 1, 1, 1, 1]), (0, [6]), (2, [3])]
    pairs = GR.noise_pairs(turns, MAX_ENVS, mutant)
    if len(set(pairs)) != len(pairs):
        bad.add("no (stream, draw) pair is used twice")
    if GR.stream_of(0, 0, MAX_ENVS, mutant) != 0 or GR.stream_of(2, 0, MAX_ENVS, mutant) != 2:
        bad.add("sequence 0 draws from the env's own stream")
    return bad


def test_every_invariant_holds_on_the_exhaustive_table():
    assert _violations(None) == set()


@pytest.mark.parametrize("mutant", GR.MUTANTS)
def test_every_mutant_breaks_an_invariant(mutant):
    bad = _violations(mutant, sizes=(2, 3, 5))
    print(f"{mutant}: {sorted(bad)}")
    assert bad, mutant


def test_refusal_rule_counts_the_envs_own_pages_and_the_forks():
    """can_fork: the free pool must hold the env's missing pages plus (n_seq - 1) * n_tail; max_positions bounds L + limit - 1"""
    pool = GR.Pool(4, 1)                                        # 4 pages in all
    assert GR.n_tail_of(63, 5) == 2 and GR.n_tail_of(64, 5) == 1 and GR.n_tail_of(64, 1) == 0 and GR.n_tail_of(65, 1) == 0
    assert pool.can_fork(0, 63, 5, 2) and not pool.can_fork(0, 63, 5, 3)        # 2 own + 2 / 4 fork pages
    assert pool.can_fork(0, 64, 5, 3) and not pool.can_fork(0, 64, 5, 4)        # 2 own + 2 / 3
    assert pool.can_fork(0, 252, 5, 2) is False                                 # 256 positions: L + limit - 1 fits, the pool does not
    assert not pool.can_fork(0, 253, 5, 2)                                      # past max_positions
    assert pool.can_fork(0, 256, 1, 8)                                          # limit 1: no fork at all


@pytest.mark.parametrize("name", ["tiny_episode", "tiny_penalty"])
def test_token0_margins_of_the_fixtures(name):
    """which (turn, stream) token-0 samples at T = 1, draw 0, seed E2E_SEED sit under the a-priori dot bound: exactly group_ref.TOKEN0_UNDER"""
    sc, g = SCENARIOS[name], load_golden(name)
    Wd = np.asarray(synth_weights(sc["cfg"], SEED)["lm_head.weight"], dtype=np.float64)
    rows = [g[f"t{t}_hidden"][0] for t in range(int(g["n_turns"]))]
    m = GR.token0_margins(Wd, rows, GR.E2E_SEED)
    under = sorted([list(k) for k, (margin, bound, _) in m.items() if margin <= bound])
    worst = min(v[0] / v[1] for v in m.values())
    print(f"{name}: {len(m)} (turn, stream) pairs, {len(under)} under the bound {under}; smallest margin / bound = {worst:.1f}")
    assert under == GR.TOKEN0_UNDER[name]
    # the streams are independent samples: the 8 sequences of a turn do not all agree on every turn
    assert any(len({m[(t, s)][2] for s in range(8)}) > 1 for t in range(len(rows)))
