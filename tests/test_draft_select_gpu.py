"""draft_select_kernel through svln_op_draft_select against drafts_ref.select, on sentinel-filled outputs: G = 1, 2, 3, 8 at r = 1 and 4
(and the 33-row limit), ragged row counts including 0, an EOS arg-max at the first, a middle and the last row, a -1 arg-max, max_new cutting
a held draft, planted ties, a start count > 0.  Everything is compared bit for bit: ids, GenCtl, the last token, the result record, the
counters, the tap rows (copies of distinct final-norm rows), the score rows; nothing is written past the emitted count; a launch with
done set changes no byte; malformed calls are refused before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import drafts_ref as R
from scenarios import SCENARIOS, SEED
from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM

pytestmark = pytest.mark.gpu
ROWS, TAP_ROWS = 48, 64
EOS = (7, 11, 4000)


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def engine(request):
    cfg = SCENARIOS["tiny_episode"]["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=request.param, max_envs=1, max_frames=1, max_positions=256)
    m.load_synthetic(SEED)
    yield m
    m.close()


def _p(a, t):
    return C.cast(a.ctypes.data_as(C.POINTER(t)), C.c_void_p) if a is not None else None


def run_op(m, ks, fed, cand, r, count, max_new, eos=EOS, done=0, scores=None, stats=(3, 40), pos=99, raw=False):
    G = len(ks)
    k = np.asarray(ks, np.int32)
    f = np.asarray(fed, np.int32)
    c = np.asarray(cand, np.int32)
    e = np.asarray(eos, np.int64)
    sc_in = None if scores is None else np.asarray(scores, np.float32)
    out = dict(ctl=np.full(8, -9, np.int32), ids=np.full(ROWS, -9, np.int32), tok=np.full(1, -9, np.int32), rec=np.full(4, -9, np.int32),
               stats=np.asarray(stats, np.int32).copy(), scores=np.full(ROWS, 5.0, np.float32) if scores is not None else None,
               taps=np.zeros((TAP_ROWS, m.cfg.hidden), np.float32))
    op = _lib.SvlnDraftSelectOp(k=_p(k, C.c_int32), fed=_p(f, C.c_int32), cand=_p(c, C.c_int32), cand_score=_p(sc_in, C.c_float),
                                eos=_p(e, C.c_int64) if e.size else None, ctl_out=_p(out["ctl"], C.c_int32), out_ids=_p(out["ids"], C.c_int32),
                                last_token=_p(out["tok"], C.c_int32), scores=_p(out["scores"], C.c_float), rec=_p(out["rec"], C.c_int32),
                                stats=_p(out["stats"], C.c_int32), taps=_p(out["taps"], C.c_float), G=G, r=r, pos=pos, kv_len=pos + 1, done=done,
                                count=count, max_new=max_new, n_eos=int(e.size), rows=ROWS, tap_rows=TAP_ROWS)
    rc = m._lib.svln_op_draft_select(m._h, C.byref(op))
    if raw:
        return rc, m._lib.svln_last_error().decode()
    _lib.check(rc)
    return out


def xn_row(q, H):
    return (q + 1 + (np.arange(H) % 4) * 0.25).astype(np.float32)


def check(m, ks, fed, cand, r, count, max_new, scored, tag):
    H = m.cfg.hidden
    nh = 1 + sum(ks)
    scores = [-(0.5 + q) / 8 for q in range(nh)] if scored else None
    want = R.select(list(cand), list(fed), list(ks), r, count, max_new, set(EOS))
    got = run_op(m, ks, fed, cand, r, count, max_new, scores=scores)
    e, stop = want["e"], want["stop"]
    assert got["rec"].tolist() == [want["winner"], e, stop, nh], (tag, got["rec"], want)
    assert got["ctl"].tolist() == [99 + want["adv"], 100 + want["adv"], stop, count + e, max_new, len(EOS), 0, 0], (tag, got["ctl"], want)
    ids = [-7] * ROWS
    ids[count:count + e] = want["ids"]
    assert got["ids"].tolist() == ids, (tag, got["ids"], want)                        # (nothing is written past e)
    assert got["tok"][0] == want["ids"][-1] and got["stats"].tolist() == [4, 40 + e], (tag, got["tok"], got["stats"])
    taps = np.full((TAP_ROWS, H), -1.0, np.float32)
    for i, q in enumerate(want["rows"]):
        taps[min(count + i, TAP_ROWS - 1)] = xn_row(q, H)
    assert np.array_equal(got["taps"], taps), (tag, "tap rows", np.nonzero((got["taps"] != taps).any(1))[0])
    if scored:
        sc = np.full(ROWS, np.nan, np.float32)
        for i, q in enumerate(want["rows"]):
            sc[count + i] = np.float32(scores[q])
        assert np.array_equal(np.isnan(got["scores"]), np.isnan(sc)), (tag, got["scores"])
        assert np.array_equal(got["scores"][count:count + e], sc[count:count + e]), (tag, got["scores"], sc)
    return want


def build(rng, G, r, truth, ks, held):
    """drafts around `truth` (the policy's ids t_0, t_1, ...): draft g repeats t_0 .. t_{held[g] - 1} and is wrong from there on; a fed row
    whose prefix is right has the next true id as its arg-max, any other row junk"""
    fed, cand = [0] * (G * r), [truth[0]]
    for g in range(G):
        for j in range(ks[g]):
            fed[g * r + j] = truth[j] if j < held[g] else 3000 + 10 * g + j
            cand.append(truth[j + 1] if j < held[g] else int(rng.integers(100, 2000)))
    return fed, cand


def test_select_matches_the_restatement(engine):
    m = engine
    rng = np.random.default_rng(5)
    n = wins = ties = stops = 0
    for G in (1, 2, 3, 8):
        for r in (1, 4):
            for trial in range(14):
                truth = [int(t) for t in rng.choice(np.arange(20, 2000), size=r + 1, replace=False)]
                special = trial % 7
                if special == 1:
                    truth[0] = EOS[0]                               # an EOS arg-max at the first row
                elif special == 2:
                    truth[r // 2] = EOS[1]                          # ... a middle row
                elif special == 3:
                    truth[r] = EOS[2]                               # ... the last row
                elif special == 4:
                    truth[int(rng.integers(0, r + 1))] = -1         # a non-finite arg-max
                ks = [int(rng.integers(0, r + 1)) for _ in range(G)]
                held = [int(rng.integers(0, r + 1)) for _ in range(G)]
                if trial >= 7:                                      # a fully held draft somewhere, and a planted tie with it
                    g = int(rng.integers(0, G))
                    ks[g] = held[g] = r
                    if G > 1:
                        o = (g + 1 + int(rng.integers(0, G - 1))) % G
                        ks[o], held[o] = r, r
                        ties += 1
                fed, cand = build(rng, G, r, truth, ks, held)
                max_new = [10, 10, 10, 10, 10, max(r, 1), 1][special] if trial < 7 else [10, r + 1, r, 2, 10, 3, 1][special]
                count = 0 if trial % 3 else int(rng.integers(1, 20))
                want = check(m, ks, fed, cand, r, count, count + max_new, scored=bool(trial % 2), tag=(G, r, trial))
                n += 1
                wins += want["winner"] >= 1
                stops += want["stop"]
    assert n == 112 and wins >= 10 and ties >= 30 and stops >= 30, (n, wins, ties, stops)


def test_thirty_three_rows_and_ragged_zero(engine):
    m = engine
    rng = np.random.default_rng(9)
    truth = [int(t) for t in rng.choice(np.arange(20, 2000), size=17, replace=False)]
    # G = 2, r = 16: 33 head rows, the second draft holds to the end
    fed, cand = build(rng, 2, 16, truth, [16, 16], [3, 16])
    want = check(m, [16, 16], fed, cand, 16, 0, 40, scored=True, tag="33 rows")
    assert (want["winner"], want["e"], want["stop"]) == (1, 17, 0)
    want = check(m, [16, 16], fed, cand, 16, 0, 9, scored=False, tag="33 rows, max_new cuts the held draft")
    assert (want["winner"], want["e"], want["stop"]) == (1, 9, 1)
    # G = 8, r = 4 with most drafts empty: only the prompt's row and draft 5's
    ks = [0, 0, 0, 0, 0, 3, 0, 0]
    fed, cand = build(rng, 8, 4, truth, ks, [0] * 5 + [3, 0, 0])
    want = check(m, ks, fed, cand, 4, 2, 12, scored=True, tag="ragged")
    assert (want["winner"], want["e"]) == (5, 4)
    # nothing fed at all: token 0 alone, winner 0
    want = check(m, [0, 0, 0], [0] * 12, [truth[0]], 4, 0, 5, scored=False, tag="nothing fed")
    assert (want["winner"], want["e"], want["stop"]) == (0, 1, 0)
    # equal drafts: the lowest one wins
    fed, cand = build(rng, 3, 4, truth, [2, 2, 2], [2, 2, 2])
    assert check(m, [2, 2, 2], fed, cand, 4, 0, 9, scored=False, tag="tie")["winner"] == 0


def test_done_changes_no_byte(engine):
    m = engine
    rng = np.random.default_rng(2)
    truth = [int(t) for t in rng.choice(np.arange(20, 2000), size=5, replace=False)]
    fed, cand = build(rng, 2, 4, truth, [4, 4], [4, 2])
    got = run_op(m, [4, 4], fed, cand, 4, 2, 9, done=1, scores=[0.0] * 9)
    assert got["ctl"].tolist() == [99, 100, 1, 2, 9, len(EOS), 0, 0]
    assert (got["ids"] == -7).all() and got["tok"][0] == -7 and (got["rec"] == -7).all() and got["stats"].tolist() == [3, 40]
    assert (got["taps"] == -1.0).all() and np.isnan(got["scores"]).all()


def test_malformed_calls_are_refused(engine):
    m = engine
    ok = dict(ks=[1, 1], fed=[5, 0, 6, 0], cand=[5, 6, 7], r=2, count=0, max_new=5)
    bad = [(dict(ks=[1] * 9, fed=[0] * 18), "G must be 1 .. 8"), (dict(ks=[]), "G must be 1 .. 8"), (dict(r=0), "head rows"),
           (dict(ks=[1] * 8, fed=[0] * 40, cand=[0] * 9, r=5), "head rows"), (dict(ks=[3, 1]), "outside 0 .. r"), (dict(ks=[-1, 1]), "outside 0 .. r"),
           (dict(count=-1), "count leaves no room"), (dict(count=ROWS - 2), "count leaves no room"), (dict(eos=list(range(5000))), "eos list")]
    for change, words in bad:
        rc, err = run_op(m, raw=True, **dict(ok, **change))
        assert rc != 0 and "op_draft_select" in err and words in err, (change, err)
    assert run_op(m, **ok)["rec"].tolist() == [0, 2, 0, 3]
