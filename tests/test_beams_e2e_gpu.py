"""Beam turns end to end on the GPU (svln_generate_beams / svln_beam_trace / svln_group_select), TINY fp32 engines unless said.  Prompts
are plain id turns (svln_append_turn), L % 64 = 0, 1, 61, 63 at max_new = 6, so that turns start on a fresh page, inside one, and cross a
page edge.

(a) n_beams = 1: every id is the arg-max a twin engine's forced turn reports for the same prefix; where the twin prefers another id, its
    margin must be covered by the two routes' bounds (derived in the test).  The strict form runs in (j).
(b) W = 2, 4, 8: the call's trace (the list of every head row of every step) replayed through tests/beam_ref.py gives the returned set
    bit for bit: ids, log-probabilities, scores, and the records of every step.
(c) every token's log-probability lies within the bound of tests/test_scores_e2e_gpu.py (2 K 2^-24 max|W||h| + 2e-5) of float64
    log_softmax from the call's own tap row (svln_get_hidden_group).
(d) every returned hypothesis is rerun as a forced turn on a twin engine.  The ids are accepted; the twin's log-probabilities lie within
    the same bound of float64 from the TWIN's own tap rows; the rows of the two engines agree within the suite's 1e-3; and the two sides
    differ by no more than their two bounds plus the float64 difference that the rows themselves explain.  A wrong KV hand-over moves a
    row by O(1).
(e) after svln_group_select(g) the env's cache length is L + n_g - 1 and its next greedy turn equals the twin's after the forced turn:
    ids identical, tap rows within 1e-3.
(f) EOS sets taken from a dry run's lists make hypotheses finish at different steps; the replay still holds.
(g) 20 calls at W = 4 with selects and resets on a tight pool: svln_kv_free_pages is back where it started after every one.
(h) one bf16 run at W = 8 under the bounds of the bf16 group test: tap rows of beam and forced twin, and of the turn after the select,
    within 3e-2 in relative norm; the next turn's first ids equal but for two near-ties of eight; the replay bit for bit.
(i) every refusal on a bf16 engine with two envs (the five switches, turns in flight, the pool), each leaving the engine usable, no
    page taken and no group pending.
(j) the agent on the tiny_episode scenario: act_beams(beam_width=1) walks the episode with the ids of a plain greedy agent on a twin model
    (turn by turn; hidden rows of the plain turns are not compared), and act_beams(beam_width=4, select=1) keeps its last_beam_* fields
    and goes on."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_ref as br
from scenarios import SEED
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM

pytestmark = pytest.mark.gpu
LSE_TOL, HIDDEN_TOL = 2e-5, 1e-3
PI32, PI64, PF = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
MAX_NEW = 6


def _engine(dtype=torch.float32, max_positions=2048, envs=1):
    m = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=envs, max_frames=1, max_positions=max_positions)
    m.load_synthetic(SEED)
    return m


@pytest.fixture(scope="module")
def pair():
    a, b = _engine(), _engine()
    yield a, b
    a.close(); b.close()


def _ok(m, rc):
    assert rc == 0, m._lib.svln_last_error()


def _prompt(L, salt=0):
    return ((np.arange(L, dtype=np.int64) * 37 + 11 + 101 * salt) % TINY.vocab).astype(np.int64)


def _start(m, L, salt=0):
    _ok(m, m._lib.svln_reset_env(m._h, 0))
    p = _prompt(L, salt)
    _ok(m, m._lib.svln_append_turn(m._h, 0, p.ctypes.data_as(PI64), L, 0))


def _beams(m, W, eos=(), max_new=MAX_NEW):
    e = np.asarray(list(eos) + [0], dtype=np.int64)
    out, n_out, sc = np.zeros((W, max_new), dtype=np.int64), np.zeros(W, dtype=np.int32), np.zeros(W, dtype=np.float32)
    rc = m._lib.svln_generate_beams(m._h, 0, W, max_new, e.ctypes.data_as(PI64), len(eos), out.ctypes.data_as(PI64), max_new,
                                    n_out.ctypes.data_as(PI32), sc.ctypes.data_as(PF))
    if rc != 0:
        return rc, None
    n = int((n_out > 0).sum())
    hyps = []
    for g in range(n):
        buf, k = np.zeros(max_new, dtype=np.float32), C.c_int32()
        _ok(m, m._lib.svln_group_logprobs(m._h, g, buf.ctypes.data_as(PF), max_new, C.byref(k)))
        assert k.value == n_out[g]
        hyps.append(dict(ids=out[g, : n_out[g]].tolist(), lps=buf[: n_out[g]].copy(), score=np.float32(sc[g])))
    return 0, hyps


def _replay(m, W, limit, eos):
    """the trace of the last call through beam_ref -> (final state, the engine's records)"""
    w, li, ll, rec = m.beam_trace()
    assert w == W
    st, recs, _ = br.run(W, limit, eos, lambda t, s: (li[t, :, :W], ll[t, :, :W]))
    assert len(recs) == len(rec), (len(recs), len(rec))
    for t, r in enumerate(recs):
        assert np.array_equal(r[:3], rec[t][:3]) and np.array_equal(r[4:20], rec[t][4:20]), (t, r, rec[t])      # (pairs / sets: the engine's page counts)
    return st


def _check_replay(m, hyps, W, limit, eos):
    st = _replay(m, W, limit, eos)
    assert st["n"] == len(hyps)
    for g, h in enumerate(hyps):
        assert st["ids"][g] == h["ids"], (g, st["ids"][g], h["ids"])
        assert [np.float32(v).view(np.uint32) for v in st["lps"][g]] == [np.float32(v).view(np.uint32) for v in h["lps"]], g
        assert np.float32(st["score"][g]).view(np.uint32) == h["score"].view(np.uint32), g
        assert h["ids"][-1] in eos or len(h["ids"]) == limit
    sc = [float(h["score"]) for h in hyps]
    assert sc == sorted(sc, reverse=True)


def _hidden_group(m, g):
    buf, n = np.zeros((8, TINY.hidden), dtype=np.float32), C.c_int32()
    _ok(m, m._lib.svln_get_hidden_group(m._h, g, buf.ctypes.data_as(PF), 8, C.byref(n)))
    return buf[: n.value].copy()


def _ref_logprobs(Wd, hidden, ids):
    """float64 (log-probability, bound) of every id from its tap row: the rule of tests/test_scores_e2e_gpu.py"""
    gamma = Wd.shape[1] * 2.0 ** -24
    lps, bounds = [], []
    for k, tok in enumerate(ids[: len(hidden)]):
        h = torch.from_numpy(np.asarray(hidden[k], dtype=np.float64))
        l = Wd @ h
        lps.append(float(l[tok] - torch.logsumexp(l, 0)))
        bounds.append(2 * gamma * float((Wd.abs() @ h.abs()).max()) + LSE_TOL)
    return lps, bounds


def _hidden(m):
    buf, k = np.zeros((8, TINY.hidden), dtype=np.float32), C.c_int32()
    _ok(m, m._lib.svln_get_hidden(m._h, buf.ctypes.data_as(PF), 8, C.byref(k)))
    return buf[: k.value].copy()


def _free_pages(m):
    n = C.c_int32()
    _ok(m, m._lib.svln_kv_free_pages(m._h, C.byref(n)))
    return n.value


def _both_sides(Wd, ids, lp_a, hid_a, lp_b, hid_b, what):
    """two kernel routes gave log-probabilities lp_a / lp_b of `ids` from the rows hid_a / hid_b: each side lies within the scores' bound
    of float64 on its OWN rows; the rows agree within the suite's 1e-3; and so the two sides differ by no more than the two bounds plus
    what float64 itself makes of the difference of the rows (the triangle inequality, no further slack)"""
    n = min(len(ids), len(hid_a), len(hid_b))
    ref_a, bd_a = _ref_logprobs(Wd, hid_a[:n], ids[:n])
    ref_b, bd_b = _ref_logprobs(Wd, hid_b[:n], ids[:n])
    assert n >= 1 and float(np.abs(hid_a[:n] - hid_b[:n]).max()) <= HIDDEN_TOL, (what, float(np.abs(hid_a[:n] - hid_b[:n]).max()))
    worst = 0.0
    for k in range(n):
        ea, eb = abs(float(lp_a[k]) - ref_a[k]), abs(float(lp_b[k]) - ref_b[k])
        assert ea <= bd_a[k] and eb <= bd_b[k], (what, k, ea, bd_a[k], eb, bd_b[k])
        assert abs(float(lp_a[k]) - float(lp_b[k])) <= bd_a[k] + bd_b[k] + abs(ref_a[k] - ref_b[k]), (what, k, float(lp_a[k]), float(lp_b[k]))
        worst = max(worst, ea / bd_a[k], eb / bd_b[k])
    return worst


def _forced(m, ids):
    f = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    lp, glp, gid, kv = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64), C.c_int32()
    _ok(m, m._lib.svln_generate_forced(m._h, 0, f.ctypes.data_as(PI64), n, None, 0, lp.ctypes.data_as(PF), gid.ctypes.data_as(PI64),
                                       glp.ctypes.data_as(PF), C.byref(kv)))
    return lp, kv.value, gid, glp


def _greedy(m, max_new=MAX_NEW, eos=()):
    e = np.asarray(list(eos) + [0], dtype=np.int64)
    out, n = np.zeros(max_new, dtype=np.int64), C.c_int32()
    _ok(m, m._lib.svln_generate(m._h, 0, max_new, e.ctypes.data_as(PI64), len(eos), out.ctypes.data_as(PI64), max_new, C.byref(n)))
    buf, k = np.zeros((8, TINY.hidden), dtype=np.float32), C.c_int32()
    _ok(m, m._lib.svln_get_hidden(m._h, buf.ctypes.data_as(PF), 8, C.byref(k)))
    return out[: n.value].tolist(), buf[: k.value].copy()


@pytest.mark.parametrize("L", [64, 65, 61, 63])
def test_width_one_is_the_greedy_turn(pair, L):
    m, twin = pair
    _start(m, L); _start(twin, L)
    Wd = torch.from_numpy(m.get_tensor("lm_head.weight")).double()
    rc, hyps = _beams(m, 1)
    _ok(m, rc)
    assert len(hyps) == 1
    ids = hyps[0]["ids"]
    _check_replay(m, hyps, 1, MAX_NEW, [])
    # every id is the twin's own arg-max given the same prefix (the forced turn's greedy ids).  The two engines reach a row by different
    # kernels (batched step / prefill rows), so where the twin prefers another id g its margin over the beam's id a must be explained by
    # the routes: lp_t(g) - lp_t(a) <= D(g) + D(a), D(x) = the two scores' bounds + |float64 on the beam's row - float64 on the twin's| for
    # id x (the beam's own list put a first).  The strict form of the check is test_agent_act_beams on tiny_episode.
    hid_a = _hidden_group(m, 0)
    lp, _, gid, glp = _forced(twin, ids)
    hid_b = _hidden(twin)
    _both_sides(Wd, ids, hyps[0]["lps"], hid_a, lp, hid_b, ("W = 1", L))
    assert ids[0] == int(gid[0])                               # (one prefill, one row: the same kernel on both engines)
    for k in range(min(len(ids), len(hid_a), len(hid_b))):
        if ids[k] == int(gid[k]):
            continue
        D = 0.0
        for x in (ids[k], int(gid[k])):
            ra, ba = _ref_logprobs(Wd, hid_a[k:k + 1], [x])
            rb, bb = _ref_logprobs(Wd, hid_b[k:k + 1], [x])
            D += ba[0] + bb[0] + abs(ra[0] - rb[0])
        assert float(glp[k]) - float(lp[k]) <= D, (k, ids, gid, float(glp[k]), float(lp[k]), D)
    kv = C.c_int32()
    _ok(m, m._lib.svln_group_select(m._h, 0, 0, C.byref(kv)))
    assert kv.value == L + len(ids) - 1


@pytest.mark.parametrize("L,W", [(64, 4), (65, 4), (61, 2), (61, 4), (61, 8), (63, 4), (63, 8)])
def test_beams_replay_scores_forced_rerun_and_select(pair, L, W):
    m, twin = pair
    Wd = torch.from_numpy(m.get_tensor("lm_head.weight")).double()
    # a dry run's lists give EOS ids that finish hypotheses at different steps
    _start(m, L)
    rc, dry = _beams(m, W)
    _ok(m, rc)
    _check_replay(m, dry, W, MAX_NEW, [])
    eos = sorted({dry[0]["ids"][1], dry[-1]["ids"][3]})
    _start(m, L)
    rc, hyps = _beams(m, W, eos)
    _ok(m, rc)
    _check_replay(m, hyps, W, MAX_NEW, eos)
    assert len(hyps) == W and len({tuple(h["ids"]) for h in hyps}) == W
    assert len({len(h["ids"]) for h in hyps}) >= 2, [h["ids"] for h in hyps]          # staggered finishes
    worst = 0.0
    for g, h in enumerate(hyps):
        _start(twin, L)
        lp, kv, _, _ = _forced(twin, h["ids"])                  # the ids are accepted
        assert kv == L + len(h["ids"]) - 1
        worst = max(worst, _both_sides(Wd, h["ids"], h["lps"], _hidden_group(m, g), lp, _hidden(twin), (L, W, g)))
    print(f"L {L} W {W}: worst error / bound on either side {worst:.3f}")
    # select the last rank (its pages were handed over most often), then one more greedy turn on both engines
    g = len(hyps) - 1
    kv = C.c_int32()
    _ok(m, m._lib.svln_group_select(m._h, 0, g, C.byref(kv)))
    assert kv.value == L + len(hyps[g]["ids"]) - 1              # (the twin stands after the forced turn of that same rank)
    nxt = _prompt(9, salt=3)
    for e in (m, twin):
        _ok(e, e._lib.svln_append_turn(e._h, 0, nxt.ctypes.data_as(PI64), 9, 0))
    ids_a, hid_a = _greedy(m)
    ids_b, hid_b = _greedy(twin)
    assert ids_a == ids_b and float(np.abs(hid_a - hid_b).max()) <= HIDDEN_TOL


def test_pool_accounting_over_twenty_calls():
    # 12 pages: the env's 2 + 15 tail pages of W = 8 do not fit; W = 4 needs 2 + 7 = 9: a leak of one page per call refuses call 4
    m = _engine(max_positions=768)
    _start(m, 70)
    free0 = _free_pages(m)
    assert free0 == 12
    for i in range(20):
        _start(m, 70, salt=i)
        assert _free_pages(m) == free0, i                       # back where it started: nothing lost, nothing returned twice
        rc, hyps = _beams(m, 4)
        _ok(m, rc)
        if i % 3 != 2:
            _ok(m, m._lib.svln_group_select(m._h, 0, i % len(hyps), None))
            ids, _ = _greedy_after(m)
            assert len(ids) >= 1
    _start(m, 70)
    rc, _ = _beams(m, 8)
    assert rc != 0 and b"free KV pages" in m._lib.svln_last_error()
    rc, hyps = _beams(m, 4)
    _ok(m, rc)
    assert _free_pages(m) == free0 - 2 - (len(hyps) - 1)        # the env's two pages and one tail page per further rank
    _ok(m, m._lib.svln_reset_env(m._h, 0))
    assert _free_pages(m) == free0
    m.close()


def _greedy_after(m):
    nxt = _prompt(9, salt=9)               # (longer than the turn the cache already holds)
    _ok(m, m._lib.svln_append_turn(m._h, 0, nxt.ctypes.data_as(PI64), 9, 0))
    return _greedy(m, 3)


def test_bf16_run():
    """the bounds of the bf16 group test (tests/test_group_e2e_gpu.py (h)): tap rows of the two routes within 3e-2 in relative norm,
    first ids of the next turn equal but for two near-ties of eight"""
    m, twin = _engine(torch.bfloat16), _engine(torch.bfloat16)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    agree = total = 0
    for g in range(8):
        _start(m, 61); _start(twin, 61)
        rc, hyps = _beams(m, 8)
        _ok(m, rc)
        _check_replay(m, hyps, 8, MAX_NEW, [])
        assert len(hyps) == 8
        taps = _hidden_group(m, g)
        lp, kv, _, _ = _forced(twin, hyps[g]["ids"])            # the ids are accepted
        assert kv == 61 + len(hyps[g]["ids"]) - 1
        rows = _hidden(twin)
        n = min(len(taps), len(rows))
        assert n >= MAX_NEW
        for k in range(n):
            assert rel(taps[k], rows[k]) < 3e-2, (g, k, rel(taps[k], rows[k]))
        kvs = C.c_int32()
        _ok(m, m._lib.svln_group_select(m._h, 0, g, C.byref(kvs)))
        assert kvs.value == kv
        nxt = _prompt(9, salt=3)
        for e in (m, twin):
            _ok(e, e._lib.svln_append_turn(e._h, 0, nxt.ctypes.data_as(PI64), 9, 0))
        ids_a, hid_a = _greedy(m)
        ids_b, hid_b = _greedy(twin)
        assert rel(hid_a[0], hid_b[0]) < 3e-2, (g, rel(hid_a[0], hid_b[0]))
        total += 1
        agree += int(ids_a[0] == ids_b[0])
    assert total == 8 and agree >= total - 2, (agree, total)
    m.close(); twin.close()


def test_refusals():
    """a bf16 engine with two envs: it takes every reduced-precision switch, and env 1 holds the scheduler turn of the in-flight case"""
    m = _engine(torch.bfloat16, max_positions=2048, envs=2)
    lib, h = m._lib, m._h
    _start(m, 61)

    def refused(needle, W=2, max_new=MAX_NEW):
        free = _free_pages(m)
        rc, _ = _beams(m, W, max_new=max_new)
        assert rc != 0 and needle in lib.svln_last_error(), (needle, lib.svln_last_error())
        ne, kl = C.c_int32(), C.c_int32()
        _ok(m, lib.svln_env_state(h, 0, C.byref(ne), C.byref(kl)))
        assert (ne.value, kl.value) == (61, 0) and _free_pages(m) == free          # nothing was prefilled, no page taken
        assert lib.svln_group_select(h, 0, 0, None) != 0        # no group is pending

    refused(b"n_beams must be 1 .. 8", W=0)
    refused(b"n_beams must be 1 .. 8", W=9)
    _ok(m, lib.svln_set_sampling(h, 1, 1.0, 1)); refused(b"svln_set_sampling"); _ok(m, lib.svln_set_sampling(h, 0, 1.0, 1))
    _ok(m, lib.svln_set_repetition_penalty(h, 1.5)); refused(b"repetition penalty"); _ok(m, lib.svln_set_repetition_penalty(h, 1.0))
    for name, fn in (("svln_set_fp8_decode", m.set_fp8_decode), ("svln_set_mxfp4_decode", m.set_mxfp4_decode), ("svln_set_fp8_gemm", m.set_fp8_gemm),
                     ("svln_set_decode_persistent", m.set_decode_persistent), ("svln_set_mxfp4_batched", m.set_mxfp4_batched)):
        fn(True); refused(name.encode()); fn(False)
    # scheduler turns in flight (on the other env)
    ids = np.arange(10, 30, dtype=np.int64)
    slot = C.c_int32(-1)
    _ok(m, lib.svln_append_turn(h, 1, ids.ctypes.data_as(PI64), len(ids), 0))
    _ok(m, lib.svln_batch_submit(h, 1, 4, None, 0, C.byref(slot)))
    refused(b"turns are in flight")
    _ok(m, lib.svln_batch_cancel(h, -1))
    _ok(m, lib.svln_reset_env(h, 1))
    # a pool that cannot hold the tails: 64 pages; a turn of 451 ids behind 61 rows has 8 tail pages: 8 + 15 x 8 = 128
    assert _free_pages(m) == 64
    refused(b"free KV pages", W=8, max_new=451)
    allow = np.asarray([3, 5, 9], dtype=np.int64)
    _ok(m, lib.svln_set_allowed_tokens(h, allow.ctypes.data_as(PI64), 3)); refused(b"shorter than n_beams", W=4)
    rc, hyps = _beams(m, 3)                                     # a list of 3 serves 3 beams: every id is of the list
    _ok(m, rc)
    assert all(t in (3, 5, 9) for hy in hyps for t in hy["ids"])
    _check_replay(m, hyps, 3, MAX_NEW, [])
    rc, _ = _beams(m, 2)
    assert rc != 0 and b"pending" in lib.svln_last_error()      # a group pending
    _ok(m, lib.svln_group_select(h, 0, 1, None))
    _ok(m, lib.svln_set_allowed_tokens(h, None, 0))
    rc, _ = _beams(m, 2)
    assert rc != 0 and b"nothing to prefill" in lib.svln_last_error()
    _start(m, 61)
    refused(b"exceeds max_positions", max_new=2048)
    rc, hyps = _beams(m, 2)                                     # the engine is usable after all of it
    _ok(m, rc)
    _check_replay(m, hyps, 2, MAX_NEW, [])
    _ok(m, lib.svln_reset_env(h, 0))
    m.close()


def test_agent_act_beams():
    from scenarios import SCENARIOS, eos_ids
    from streamvln_amd.agent import StreamingAgent
    from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
    sc = SCENARIOS["tiny_episode"]

    def model():
        m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.float32, max_envs=1, max_frames=1 + sc["num_history"], max_positions=2048)
        m.load_synthetic(SEED)
        m.model.num_history = sc["num_history"]
        return m

    def agent(m):
        enc = SyntheticPromptEncoder(sc["cfg"], seed=7, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
        return StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"], env_id=0,
                              device="cuda", max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc),
                              preprocess=m.get_vision_tower().image_processor.preprocess_array)

    ma, mb = model(), model()
    a, b = agent(ma), agent(mb)
    for step in range(8):
        frame = synthetic_frame(0, step)
        if len(a.action_seq) == 0:
            assert a.act_beams(frame, beam_width=1) == b.act(frame)
            assert a.last_beam_index == 0 and len(a.last_beam_ids) == 1
        else:
            with pytest.raises(ValueError, match="no model turn runs"):
                a.act_beams(frame, beam_width=2)
            assert a.act(frame) == b.act(frame)
    assert len(a.turn_log) >= 2
    assert [r["out"].sequences[0].tolist() for r in a.turn_log] == [r["out"].sequences[0].tolist() for r in b.turn_log]
    with pytest.raises(NotImplementedError, match="beam_width together with forced_ids"):
        ma.generate(**dict(a._build_request(""), beam_width=2, forced_ids=[1, 2]))
    # a wider turn with a chosen hypothesis, then the episode goes on
    step = 8
    while len(a.action_seq) != 0:
        a.act(synthetic_frame(0, step)); step += 1
    a.act_beams(synthetic_frame(0, step), beam_width=4, select=1)
    assert a.last_beam_index == 1 and 2 <= len(a.last_beam_ids) <= 4 and tuple(a.last_beam_scores.shape) == (len(a.last_beam_ids),)
    sc_l = a.last_beam_scores.tolist()
    assert sc_l == sorted(sc_l, reverse=True)
    assert a.turn_log[-1]["out"].sequences[0].tolist() == a.last_beam_ids[1]
    for k in range(6):
        a.act(synthetic_frame(0, step + 1 + k))
    ma.close(); mb.close()
