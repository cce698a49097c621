"""prefill_draft_ref.simulate (the host policy of svln_set_prefill_draft) on a small exhaustive table (no GPU): whatever the draft says the
emitted ids are the plain loop's, the counters add up, the ride never breaks a rule, the row count is the formula's at each cap in turn,
and leaving any one cap out is caught by some entry of the table."""
import itertools

import pytest

import prefill_draft_ref as PR
import verify_ref as VR

EOS = {2}
VOCAB = 3


def turns():
    """every turn of <= 6 tokens over the alphabet {0, 1, EOS = 2}: <= 5 free tokens, then the EOS; ids behind the stop are never read"""
    for n in range(6):
        for s in itertools.product((0, 1), repeat=n):
            yield list(s) + [2]


def drafts_for(turn):
    """every draft of <= 3 ids over the alphabet, and drafts of up to 9 ids made from the turn: the turn itself, one id changed at each
    index, too short, too long, without the EOS, an EOS early, an id outside the vocabulary in the middle"""
    out = [list(d) for n in range(4) for d in itertools.product((0, 1, 2), repeat=n)]
    out.append(list(turn))
    for j in range(len(turn)):
        d = list(turn)
        d[j] = (d[j] + 1) % 3
        out.append((d + [1] * 9)[:9])
    out.append(turn[:-1])
    out.append((turn + [1] * 9)[:9])
    out.append((turn[:-1] + [1] * 9)[:9])
    out.append((turn[:-1] + [0] * 9)[:9])
    out.append(turn[:1] + [2] + turn[1:])
    out.append(turn[:2] + [3] + turn[2:])
    return out


def plain(true_ids, max_new):
    out = []
    for t in true_ids:
        out.append(t)
        if t in EOS or len(out) >= max_new:
            break
    return out


def table():
    for turn in turns():
        true_ids = turn + [0] * 12
        for max_new in (1, 2, 4, 16):
            want = plain(true_ids, max_new)
            for room in (len(want) - 1, 16):
                for d in drafts_for(turn):
                    yield true_ids, want, d, max_new, room


def test_simulate_emits_the_plain_ids_and_the_counters_add_up():
    n = n_rides = n_clean = 0
    for true_ids, want, d, max_new, room in table():
        D = VR.usable_draft(d, VOCAB)
        k = PR.ride_rows(D, max_new, EOS, room)
        assert PR.broken_rules(k, D, max_new, EOS, room) == [], (d, max_new, room, k)
        for rows in (0, 2, 4):
            ids, (rides, rtok, fed, passes, vtok, single) = PR.simulate(true_ids, d, max_new, EOS, room, rows, VOCAB)
            assert ids == want, (true_ids, d, max_new, room, rows, ids)
            assert (rides, fed) == (int(k > 0), k)
            if rides:
                assert 1 <= rtok <= k + 1 and rtok + vtok + single == len(ids)
                n_rides += 1
            else:
                assert rtok == 0 and 1 + vtok + single == len(ids)
                assert (ids, passes, vtok, single) == VR.simulate(true_ids, d, rows, max_new, EOS, room, VOCAB)
            if rows == 0:
                assert passes == vtok == 0
            # a right draft that fits one ride: the whole turn comes from it, no decode pass of either kind
            if d[:len(want)] == want and len(want) >= 2 and room >= len(want) - 1:
                assert (rides, rtok, fed, passes, vtok, single) == (1, len(want), len(want) - 1, 0, 0, 0), (d, want, max_new, room)
                n_clean += 1
            n += 1
    assert n > 50000 and n_rides > n // 4 and n_clean > 1000, (n, n_rides, n_clean)


@pytest.mark.parametrize("what,D,max_new,room,k", [
    ("dlen", [0, 1, 0], 16, 16, 3),
    ("dlen = 1 is enough", [0], 16, 16, 1),
    ("7 rows", [0, 1] * 5, 16, 16, 7),
    ("max_new - 1", [0, 1, 0, 1, 0, 1], 4, 16, 3),
    ("max_new = 1: plain", [0, 1], 1, 16, 0),
    ("room", [0, 1, 0, 1, 0, 1], 16, 2, 2),
    ("room = 0: plain", [0, 1], 16, 0, 0),
    ("room < 0: plain (the plain turn raises)", [0, 1], 16, -3, 0),
    ("first EOS", [0, 1, 2, 1, 0], 16, 16, 2),
    ("EOS at 0: plain", [2, 1, 0], 16, 16, 0),
    ("EOS behind the other caps", [0, 1, 0, 2], 3, 16, 2),
    ("empty", [], 16, 16, 0),
])
def test_row_count_at_each_cap(what, D, max_new, room, k):
    assert PR.ride_rows(D, max_new, EOS, room) == k, what
    assert PR.broken_rules(k, D, max_new, EOS, room) == []
    true_ids = [0, 1, 0, 1, 0, 1, 0, 1, 0, 2]
    if room >= 0:
        want = plain(true_ids, max_new)
        if room >= len(want) - 1:
            ids, st = PR.simulate(true_ids, D, max_new, EOS, room, 0, VOCAB)
            assert ids == want and st[2] == k and st[0] == int(k > 0), (what, st)


@pytest.mark.parametrize("mutant", PR.MUTANTS)
def test_each_cap_is_needed(mutant):
    """a ride_rows with one cap left out breaks a rule on some entry of the table; the real one on none (asserted above)"""
    caught = 0
    for true_ids, want, d, max_new, room in table():
        D = VR.usable_draft(d, VOCAB)
        k = PR.ride_rows(D, max_new, EOS, room, mutant)
        if PR.broken_rules(k, D, max_new, EOS, room):
            caught += 1
    assert caught >= 1, mutant


def test_out_of_vocabulary_id_ends_the_draft():
    true_ids = [0, 1, 0, 1, 2] + [0] * 8
    ids, st = PR.simulate(true_ids, [0, 1, 7, 1, 2], 16, EOS, 16, 0, VOCAB)
    assert ids == [0, 1, 0, 1, 2] and st == (1, 3, 2, 0, 0, 2)
    ids, st = PR.simulate(true_ids, [0, 1, 7, 1, 2], 16, EOS, 16, 4, VOCAB)            # verify passes need a guess beyond the emitted ids
    assert ids == [0, 1, 0, 1, 2] and st == (1, 3, 2, 0, 0, 2)
    ids, st = PR.simulate(true_ids, [5, 1], 16, EOS, 16, 4, VOCAB)
    assert st[:3] == (0, 0, 0)


def test_ride_then_verify_passes():
    """a right draft longer than one ride: 8 tokens from the ride, the rest from verify passes (or single steps with the mode off)"""
    true_ids = [0, 1] * 5 + [2] + [0] * 8
    d = true_ids[:11]
    ids, st = PR.simulate(true_ids, d, 16, EOS, 16, 4, VOCAB)
    assert ids == d and st == (1, 8, 7, 1, 3, 0)
    ids, st = PR.simulate(true_ids, d, 16, EOS, 16, 0, VOCAB)
    assert ids == d and st == (1, 8, 7, 0, 0, 3)
    wrong = list(d)
    wrong[3] = 0
    ids, st = PR.simulate(true_ids, wrong, 16, EOS, 16, 4, VOCAB)                      # the ride emits ids 0 .. 3; id 3 differs from the draft: single steps
    assert ids == d and st == (1, 4, 7, 0, 0, 7)
