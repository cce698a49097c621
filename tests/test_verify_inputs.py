"""CPU proofs for the draft-verify tests: the verify attention cases of tests/test_verify_attn_gpu.py are sharp (every plausible mistake
of a multi-row pass -- float64 "mutant" references of tests/attn_ref.py and tests/verify_ref.py -- moves the expected output by at least
10x the tolerance the GPU test applies, the factor of test_attention_inputs.py), and the Python restatement of the verify rule and host
policy (verify_ref.simulate) gives the hand-written outcomes.  (P = 127 with (tiny, 8 rows, bf16) is not sharp -- stale_k moves it only
2.7x -- and is not a case.)"""
import pytest
import torch

import verify_ref as VR
from streamvln_amd.config import CONFIGS

DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,rows,P", VR.all_cases())
def test_verify_attention_inputs_are_discriminating(dtype, cfg, rows, P):
    case = VR.verify_case(CONFIGS[cfg], dtype, P, rows)
    ratios = VR.mutant_ratios(case)
    assert set(VR.VERIFY_MUTANTS) <= set(ratios) and ("drop_split" in ratios) == (P + rows > 64)
    weak = {k: round(v, 1) for k, v in ratios.items() if not v >= 10.0}
    assert not weak, f"verify {cfg} rows {rows} P {P}: mutants within 10x the tolerance: {weak}"


# ------------------------------------------------------------------------------------------------------------ simulate
TRUE = [11, 12, 13, 14, 15, 2, 99, 98]        # plain greedy ids of a turn; 2 is the EOS id, so the turn is TRUE[:6]
EOS = (2,)
TURN = TRUE[:6]


def sim(draft, rows, max_new=16, room=100, true=TRUE, eos=EOS, vocab=1000):
    return VR.simulate(true, draft, rows, max_new, eos, room, vocab)


def test_simulate_perfect_draft():
    assert sim(TURN, 2) == (TURN, 3, 5, 0)
    assert sim(TURN, 4) == (TURN, 2, 5, 0)
    assert sim(TURN, 8) == (TURN, 1, 5, 0)
    assert sim(TURN, 0) == (TURN, 0, 0, 5)                # mode off
    assert sim([777] + TURN[1:], 4) == (TURN, 2, 5, 0)    # D[0] is never needed


@pytest.mark.parametrize("rows", [2, 4, 8])
@pytest.mark.parametrize("j", [1, 2, 3, 4, 5])
def test_simulate_draft_wrong_at_each_index(rows, j):
    draft = list(TURN)
    draft[j] = 500
    ids, passes, vtok, single = sim(draft, rows)
    assert ids == TURN and vtok + single == 5
    # a pass runs while the draft has a guess for the next token and has held so far; the pass that is fed the wrong guess (or whose
    # first row replaces it) emits up to and including the token that replaces it, and single steps finish the turn
    exp_passes, c = 0, 1
    while c < 6:
        r = min(rows, 6 - c + 1)
        exp_passes += 1
        if c <= j < c + r:
            c = j + 1
            break
        c += r
    assert passes == exp_passes and vtok == c - 1 and single == 6 - c


def test_simulate_hand_cases():
    # wrong at index 1, rows 4: one pass emits one token, four single steps
    assert sim([11, 500, 13, 14, 15, 2], 4) == (TURN, 1, 1, 4)
    # wrong at index 3, rows 4: the pass emits 12, 13, 14 (row 2's arg-max 14 replaces the guess 500); then two single steps
    assert sim([11, 12, 13, 500, 15, 2], 4) == (TURN, 1, 3, 2)
    # wrong at index 5 (the EOS), rows 4: pass 1 emits 4 tokens, pass 2 (2 rows) emits the EOS from row 0
    assert sim([11, 12, 13, 14, 15, 500], 4) == (TURN, 2, 5, 0)


def test_simulate_draft_shorter_or_longer_than_the_turn():
    assert sim([], 4) == (TURN, 0, 0, 5)
    assert sim([11], 4) == (TURN, 0, 0, 5)                         # no guess beyond index 0
    assert sim([11, 12], 4) == (TURN, 1, 2, 3)                     # one guessed row: 2 rows -> 12, 13; the draft is spent
    assert sim([11, 12, 13, 14], 4) == (TURN, 1, 4, 1)             # 4 rows -> 12 .. 15; the EOS by a single step
    assert sim(TURN + [7, 7, 7, 7, 7, 7], 4) == (TURN, 2, 5, 0)    # twice too long: pass 2 stops at the EOS in row 0
    assert sim(TURN + [7, 7, 7, 7, 7, 7], 8) == (TURN, 1, 5, 0)
    assert sim([11, 12, -1, 14, 15, 2], 4) == (TURN, 1, 2, 3)      # an id outside the vocabulary ends the usable draft
    assert sim([11, 12, 5000, 14, 15, 2], 4) == (TURN, 1, 2, 3)


def test_simulate_eos_inside_the_draft_where_the_model_emits_none():
    # the guess at index 2 is an EOS id: it is fed like any token, row 1's arg-max 13 != 2 rejects it
    assert sim([11, 12, 2, 14, 15, 2], 4) == (TURN, 1, 2, 3)
    assert sim([11, 12, 2, 14, 15, 2], 8) == (TURN, 1, 2, 3)


def test_simulate_max_new_cuts_a_pass():
    assert sim(TURN, 4, max_new=3) == (TURN[:3], 1, 2, 0)          # room for two tokens: a 2-row pass
    assert sim(TURN, 4, max_new=2) == (TURN[:2], 1, 1, 0)          # room for one: a one-row pass
    assert sim(TURN, 4, max_new=1) == (TURN[:1], 0, 0, 0)
    assert sim(TURN, 2, max_new=4) == (TURN[:4], 2, 3, 0)          # 12, 13 by pass 1; pass 2 carries one row
    assert sim(TURN, 2, max_new=6) == (TURN, 3, 5, 0)              # the turn's own length: the third pass carries one row and emits the EOS
    assert sim(TURN, 4, max_new=6) == (TURN, 2, 5, 0)
    assert sim(TURN, 8, max_new=5) == (TURN[:5], 1, 4, 0)


def test_simulate_room_cuts_a_pass():
    # room = positions left for fed tokens: token k (k >= 0) is fed at position L + k, so room 3 lets tokens 0, 1, 2 be fed
    assert sim(TURN, 4, max_new=4, room=3) == (TURN[:4], 1, 3, 0)  # rows at L, L+1, L+2
    assert sim(TURN, 8, max_new=3, room=2) == (TURN[:3], 1, 2, 0)
    assert sim(TURN, 4, max_new=2, room=1) == (TURN[:2], 1, 1, 0)  # one position: a one-row pass
    assert sim(TURN, 2, max_new=4, room=3) == (TURN[:4], 2, 3, 0)  # pass 2 has one position left
    with pytest.raises(AssertionError):
        sim(TURN, 4, max_new=6, room=2)                             # the turn does not fit: the engine reports it too


def test_verify_step_rule():
    assert VR.verify_step([11, 12, 13, 14], [12, 13, 14, 15], 1, 16, EOS) == (5, False, [12, 13, 14, 15], 15)
    assert VR.verify_step([11, 12, 500, 14], [12, 13, 77, 78], 1, 16, EOS) == (3, False, [12, 13], 13)
    assert VR.verify_step([11, 12, 13, 14], [12, 2, 14, 15], 1, 16, EOS) == (3, True, [12, 2], 2)          # EOS appended, stop
    assert VR.verify_step([11, 12, 13, 14], [12, 13, 14, 15], 1, 3, EOS) == (3, True, [12, 13], 13)        # max_new
    assert VR.verify_step([11, 12, 13, 14], [-1, 13, 14, 15], 1, 16, EOS) == (2, True, [-1], -1)           # non-finite arg-max
