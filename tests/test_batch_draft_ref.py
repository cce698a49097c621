"""batch_draft_ref.simulate (the host policy of svln_set_batch_draft) on a small exhaustive table (no GPU): whatever the drafts say every
env's ids and kv_len are the plain loop's, no row reaches max_positions, no iteration overfills the row workspace, no EOS id is fed, the
counters add up -- and every listed mutant of the policy is caught by some entry of the table."""
import itertools

import pytest

import batch_draft_ref as BR
import prefill_draft_ref as PR

EOS = {2}
VOCAB = 3
MP = 20                    # max_positions of the table: two segments of 8 rows leave 4 rows for drafts, a third one waits

TURNS = [[2], [0, 2], [0, 1, 2], [1, 1, 0, 2], [1, 0, 0, 1, 1, 0, 1, 0, 2]]


def drafts_for(turn):
    """no draft, an empty one, the turn itself, an id changed at 0 / at 1, too short, too long, an EOS early, an id outside the vocabulary"""
    out = [None, [], list(turn)]
    for j in (0, 1):
        if j < len(turn):
            d = list(turn)
            d[j] = (d[j] + 1) % 3
            out.append((d + [1] * 9)[:9])
    out.append(turn[:max(len(turn) // 2, 1)])
    out.append((turn[:-1] + [1] * 9)[:9])
    out.append(turn[:1] + [2] + turn[1:])
    out.append(turn[:1] + [3] + turn[1:])
    return out


#: env layouts: (n_embeds, kv_len, submitted before iteration) per turn, in submit order; the env is the index unless given
LAYOUTS = {
    "solo": [(12, 0, 0)],
    "solo_last_rows": [(MP - 2, 10, 0)],                        # two positions left: k <= 2
    "two_lockstep": [(8, 0, 0), (8, 0, 0)],                     # the second segment's k is cut by the workspace
    "three_lockstep": [(8, 0, 0), (8, 0, 0), (8, 0, 0)],        # the third segment waits for the next iteration, beside decode rows
    "staggered": [(9, 0, 0), (7, 2, 1), (11, 3, 2)],            # rides beside other envs' decode rows
}


def schedule(layout, turn_ix, draft_ix, max_new):
    turns = []
    for e, (ne, kl, at) in enumerate(LAYOUTS[layout]):
        turn = TURNS[turn_ix[e]]
        turns.append(BR.Turn(e, turn + [0] * 12, drafts_for(turn)[draft_ix[e]], max_new, EOS, ne, kl, at))
    return turns


def table():
    for layout, rows in LAYOUTS.items():
        n = len(rows)
        turn_sets = itertools.product(range(len(TURNS)), repeat=n) if n == 1 else itertools.product((1, 3, 4), repeat=n)
        for turn_ix in turn_sets:
            nd = [len(drafts_for(TURNS[i])) for i in turn_ix]
            picks = itertools.product(*[range(x) for x in nd]) if n <= 2 else itertools.product(*[(0, 2, 3, 6) for _ in nd])
            for draft_ix in picks:
                for max_new in (1, 2, 16):
                    # (a turn the plain loop cannot finish inside max_positions is an error with and without drafts)
                    if all(ne + min(len(TURNS[i]), max_new) - 1 <= MP for i, (ne, _, _) in zip(turn_ix, rows)):
                        yield layout, turn_ix, draft_ix, max_new
    # a second turn of the same env with no draft of its own, after a turn whose draft was used
    for d0 in range(len(drafts_for(TURNS[2]))):
        yield "second_turn", (2, 1), (d0, 0), 16


def build(layout, turn_ix, draft_ix, max_new):
    if layout != "second_turn":
        return schedule(layout, turn_ix, draft_ix, max_new)
    t0, t1 = TURNS[turn_ix[0]], TURNS[turn_ix[1]]
    return [BR.Turn(0, t0 + [0] * 12, drafts_for(t0)[draft_ix[0]], max_new, EOS, 8, 0, 0),
            BR.Turn(0, t1 + [0] * 12, None, max_new, EOS, 8 + len(t0) + 3, 8 + len(t0) - 1, 10)]


def test_every_schedule_emits_the_plain_ids_and_the_counters_add_up():
    n = n_rides = n_cut = n_wait = n_mixed = 0
    for case in table():
        turns = build(*case)
        (rides, rtok, rfed, iters, single), log = BR.simulate(turns, MP, VOCAB)
        assert BR.broken_rules(turns, log, MP) == [], case
        assert iters == len(log) and single == sum(r["decode_rows"] for r in log) == sum(t.decode_rows for t in turns)
        assert rides == sum(1 for t in turns if t.k) == sum(r["rides"] for r in log) and rfed == sum(t.k for t in turns)
        assert rtok == sum(t.ride_tokens for t in turns)
        assert sum(len(t.out) for t in turns) == rtok + single + sum(1 for t in turns if not t.k), case
        for t in turns:
            D = [] if t.draft is None else BR.VR.usable_draft(t.draft, VOCAB)
            assert t.k <= PR.ride_rows(D, t.max_new, EOS, MP - t.n_embeds)
            assert 0 <= t.ride_tokens <= t.k + 1 and len(t.out) == max(t.ride_tokens, 1) + t.decode_rows
        n += 1
        n_rides += rides
        n_cut += any(t.k < PR.ride_rows([] if t.draft is None else BR.VR.usable_draft(t.draft, VOCAB), t.max_new, EOS, MP - t.n_embeds)
                     for t in turns)
        n_wait += any(t.first_iteration > t.at for t in turns)
        n_mixed += any(r["rides"] and r["decode_rows"] for r in log)
    print(f"{n} schedules, {n_rides} rides, {n_cut} with a workspace cut, {n_wait} with a waiting job, {n_mixed} with a ride beside decode rows")
    assert n > 3000 and n_rides > n and n_cut > 50 and n_wait > 50 and n_mixed > 50


def test_right_drafts_take_one_iteration():
    """lockstep envs whose drafts are all right: one iteration per turn, no decode row -- while the workspace holds every draft row"""
    for n_envs in (1, 2, 5, 8):
        for ti in range(len(TURNS)):
            turn = TURNS[ti]
            turns = [BR.Turn(e, turn + [0] * 12, list(turn), 16, EOS, 40 + e, 0) for e in range(n_envs)]
            stats, log = BR.simulate(turns, 2048, VOCAB)
            k = min(len(turn) - 1, PR.RIDE_MAX_ROWS)
            done = len(turn) <= 8
            assert BR.broken_rules(turns, log, 2048) == []
            if done:
                assert stats == (n_envs * (k > 0), n_envs * len(turn) * (k > 0), n_envs * k, 1, 0), (n_envs, turn, stats)
                assert log[0]["head_rows"] == n_envs * (k + 1) <= BR.HEAD_ROWS
            else:
                assert stats == (n_envs, n_envs * 8, n_envs * 7, 1 + len(turn) - 8, n_envs * (len(turn) - 8)), (n_envs, turn, stats)


def test_switch_off_and_penalty_ride_nothing():
    for switch, penalty in ((False, 1.0), (True, 1.3)):
        for case in itertools.islice(table(), 0, None, 7):
            turns = build(*case)
            stats, log = BR.simulate(turns, MP, VOCAB, penalty=penalty, switch=switch)
            assert stats[:3] == (0, 0, 0) and BR.broken_rules(turns, log, MP, drafts_usable=False) == [], case
            assert stats[4] == sum(len(t.out) - 1 for t in turns)


@pytest.mark.parametrize("mutant", BR.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = 0
    for case in table():
        turns = build(*case)
        try:
            _, log = BR.simulate(turns, MP, VOCAB, mutant=mutant)
        except (AssertionError, IndexError):
            caught += 1
            continue
        caught += bool(BR.broken_rules(turns, log, MP))
    print(f"{mutant}: caught by {caught} schedules")
    assert caught >= 1, mutant
