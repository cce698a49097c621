"""The restated policy of forced jobs in the scheduler (tests/batch_forced_ref.py) on an exhaustive small table: 1 .. 3 forced envs with n
of 1 .. 4 and 32, prompts and workspaces small enough that jobs wait, with and without the decode rows of a plain neighbour.  The
restatement breaks none of the rules; every mutant breaks at least one somewhere on the table."""
import itertools

import pytest

import batch_forced_ref as BF

NS = (1, 2, 3, 4, 32)
EOS = (2,)


def _F(env, n):
    """ids of a forced job: distinct per position (a target taken from the wrong position shows), the EOS id last for even envs"""
    ids = [100 * (env + 1) + i for i in range(n)]
    if env % 2 == 0:
        ids[-1] = EOS[0]
    return ids


def table():
    """(turns factory, max_positions, label): every combination of 1 .. 3 forced envs x n, at two prompt lengths, in a workspace that
    holds everything, one that makes the later jobs wait for the earlier ones, and -- with a plain neighbour that prefills first and then
    decodes three more rows -- one that makes a job wait until the decode rows have left"""
    out = []
    for n_envs in (1, 2, 3):
        for ns in itertools.product(NS, repeat=n_envs):
            for Tn in (3, 9):
                need = [Tn + n - 1 for n in ns]
                # the smallest workspace every submit accepts: env 1 has 4 rows of history, so its last position is 4 + Tn + n - 2; the
                # neighbour decodes up to position 8.  At `most` the longest job fits alone only: one decode row makes it wait.
                most = max(max(r + (4 if e == 1 else 0) for e, r in enumerate(need)), 9)
                for mp in sorted({2048, most, most + 2, max(sum(need), most)}):
                    for neighbour in (False, True):
                        def make(ns=ns, Tn=Tn, neighbour=neighbour):
                            turns = []
                            if neighbour:     # env 7: a plain job submitted first; it decodes while the forced jobs prefill
                                turns.append(BF.Turn(7, 5, 0, None, true_ids=[11, 12, 13, 14], max_new=4, eos=EOS, at=0))
                            for e, n in enumerate(ns):
                                turns.append(BF.Turn(e, (4 if e == 1 else 0) + Tn, 4 if e == 1 else 0, _F(e, n), eos=EOS, at=1 if neighbour else 0))
                            return turns
                        out.append((make, mp, f"ns={ns} Tn={Tn} mp={mp} neighbour={neighbour}"))
    return out


TABLE = table()


def test_table_is_what_it_claims():
    assert len(TABLE) > 1000
    waited = decode_shared = straddle = waited_for_decode = 0
    for make, mp, label in TABLE:
        turns = make()
        _, log = BF.simulate(turns, mp)
        waited += any(t.waited for t in turns)
        decode_shared += any(r["decode_rows"] and r["forced_rows"] for r in log)
        straddle += any(len(r["chunks"]) > 1 for r in log)
        # a job that could not run beside the decode rows and ran once they had left
        waited_for_decode += any(t.forced is not None and t.waited and log[[r["iteration"] for r in log].index(t.first_iteration)]["decode_rows"] == 0
                                 and any(log[[r["iteration"] for r in log].index(it)]["decode_rows"] > 0 for it, _ in t.waited) for t in turns)
    assert waited > 100 and decode_shared > 100 and straddle > 10 and waited_for_decode > 10, (waited, decode_shared, straddle, waited_for_decode)


def test_restatement_respects_every_rule():
    for make, mp, label in TABLE:
        turns = make()
        stats, log = BF.simulate(turns, mp)
        assert BF.broken_rules(turns, log, mp) == [], label
        forced = [t for t in turns if t.forced is not None]
        assert stats[0] == len(forced) and stats[1] == sum(len(t.forced) - 1 for t in forced), (label, stats)
        assert stats[2] == sum((r["forced_rows"] + 31) // 32 for r in log), (label, stats)
        for t in forced:
            assert t.out == t.forced and t.kv_len == t.n_embeds + len(t.forced) - 1 and t.done, label
            assert all(pos < mp for pos, _ in t.fed) and all(tok not in EOS for _, tok in t.fed), label
            assert (t.n_embeds + len(t.forced) - 1, t.forced[-1]) not in t.fed, label
        for r in log:
            assert r["rows"] <= mp, label


@pytest.mark.parametrize("mutant", BF.MUTANTS)
def test_every_mutant_breaks_a_rule(mutant):
    assert len(BF.MUTANTS) >= 6
    broken = 0
    for make, mp, label in TABLE:
        turns = make()
        _, log = BF.simulate(turns, mp, mutant=mutant)
        broken += bool(BF.broken_rules(turns, log, mp))
    print(f"mutant {mutant}: breaks a rule on {broken} of {len(TABLE)} schedules")
    assert broken >= 1, mutant


def test_chunk_table():
    assert [BF.head_route(r) for r in (1, 2, 3, 4, 5, 31, 32)] == [(2, "gemv"), (2, "gemv"), (4, "mfma"), (4, "mfma"), (5, "mfma"), (31, "mfma"),
                                                                   (32, "mfma")]
    assert BF.chunks_of(33) == [(0, 32), (32, 1)] and BF.chunks_of(32) == [(0, 32)] and BF.chunks_of(256) == [(32 * k, 32) for k in range(8)]
    assert BF.chunks_of(1) == [(0, 1)] and BF.chunks_of(0) == []


def test_submit_rules():
    ok = dict(F=[5, 6, 2], eos=EOS, n_embeds=40, kv_len=0, max_positions=256, vocab=100)
    assert BF.submit_refusal(**ok) is None
    assert BF.submit_refusal(**dict(ok, F=[])) == "n must be 1 .. 32" == BF.submit_refusal(**dict(ok, F=[5] * 33))
    assert BF.submit_refusal(**dict(ok, F=[5, 100, 6])) == "outside the vocabulary" == BF.submit_refusal(**dict(ok, F=[-1]))
    assert BF.submit_refusal(**dict(ok, F=[5, 2, 6])) == "EOS"
    assert BF.submit_refusal(**dict(ok, penalty=1.3)) == "svln_set_repetition_penalty"
    for s in ("svln_set_fp8_decode", "svln_set_mxfp4_decode", "svln_set_fp8_gemm", "svln_set_mxfp4_batched", "svln_set_decode_persistent"):
        assert BF.submit_refusal(**dict(ok, switches=(s,))) == s
    assert BF.submit_refusal(**dict(ok, allowed={5, 6})) == "allowed list" and BF.submit_refusal(**dict(ok, allowed={2, 5, 6})) is None
    assert BF.submit_refusal(**dict(ok, kv_len=40)) == "nothing to prefill"
    assert BF.submit_refusal(**dict(ok, n_embeds=254)) is None and BF.submit_refusal(**dict(ok, n_embeds=255)) == "max_positions"
    assert BF.submit_refusal(**dict(ok, in_flight=True)) == "already has a turn in flight"
    assert BF.submit_refusal(**dict(ok, free_slots=0)) == "at most 8 turns in flight"
