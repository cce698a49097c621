"""Forced turns end to end (generate(forced_ids=...) / svln_generate_forced / svln_turn_forced) on the GPU, fp32 and bf16 engines.

(1) Bit for bit: a forced turn on F computes what a ride with the draft D = F computes (q | k | v rows after RoPE and the residual rows
of the last layer, layer 0's cached K / V rows, the final-norm tap rows, the arg-max of every head row), and for n = 12 (forced rows
across a KV page edge) and n = 32 (Tn + n - 1 across 256 rows) what a plain prefill computes whose caller spliced the same embeddings on
-- there also greedy_logprobs are the bits of the scored MFMA head on the spliced run's rows.
(2) With F = the fixtures' own ids (tiny_episode, true4_episode) the episode IS the fixtures' episode: ids, hidden rows (<= 1e-3 on the
fp32 engine), cache lengths; greedy_ids == F and token_logprobs is bit-equal to greedy_logprobs.
(3) With F differing from the policy's choice at index 0, 1 or last: tap rows within 1e-3 of the oracle teacher-forced on the same ids,
every score inside the a-priori bound 2 gamma_K max_n sum|w h| + 2e-5 of float64 log_softmax from the engine's own tap rows
(tests/test_scores_e2e_gpu.py), and the next plain turn agrees with the oracle continued from F.
(4) Sampling at T = 1/2 with F = a sampled turn's ids; an allowed list; the agent; every row of the refusal / allowed table."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, eos_ids, run_scenario
from streamvln_amd import _lib
from streamvln_amd import weights as Wt
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
from test_e2e_gpu import BF16_HIDDEN_REL, HIDDEN_TOL
from util import load_golden

pytestmark = pytest.mark.gpu
LSE_TOL = 2e-5
MAX_POSITIONS = 2048
PI64, PF, PI32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
_models = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def model(name, dtype):
    """one engine per (configuration, dtype) for the module; every test starts from reset(1) with every switch off"""
    sc = SCENARIOS[name]
    key = (sc["cfg"].name, dtype)
    if key not in _models:
        m = StreamVLNForCausalLM(sc["cfg"], dtype=dtype, max_envs=1, max_frames=1 + (sc["num_history"] or 0), max_positions=MAX_POSITIONS)
        m.load_synthetic(SEED)
        _models[key] = m
    m = _models[key]
    m.model.num_history = sc["num_history"]
    m.set_prefill_draft(False); m.set_speculative(0); m.set_batch_draft(False)
    m.set_sampling(None); m.set_allowed_tokens(None); m.set_token_scores(False)
    m.generation_config.repetition_penalty = 1.0
    m._sync_call_config()
    m.reset(1)
    return m


# ------------------------------------------------------------------------------------------------------------ low-level helpers
def _prompt(n, seed, vocab):
    return np.random.default_rng(seed).integers(5, vocab, size=n).astype(np.int64)


def _append(m, ids):
    a = np.ascontiguousarray(ids, dtype=np.int64)
    _lib.check(m._lib.svln_append_turn(m._h, 0, a.ctypes.data_as(PI64), int(a.size), 0))


def _fixed(m, n):
    out = np.zeros(n, np.int64)
    _lib.check(m._lib.svln_generate_fixed(m._h, 0, n, out.ctypes.data_as(PI64)))
    return out.tolist()


def _begin(m, P, Tn, seed):
    """a fresh env with P rows of history in the cache (one earlier turn) and Tn new prompt rows"""
    m.reset(1)
    V = m.cfg.vocab
    if P:
        _append(m, _prompt(P, seed, V))
        _fixed(m, 1)
    _append(m, _prompt(Tn, seed + 1, V))
    assert m.env_state(0) == (P + Tn, P)


def _forced_rc(m, F, eos=()):
    f = np.ascontiguousarray(F, dtype=np.int64)
    e = np.ascontiguousarray(eos, dtype=np.int64)
    n = max(int(f.size), 1)
    lp, glp, gid, kv = np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32), np.full(n, -7, np.int64), C.c_int32(-1)
    rc = m._lib.svln_generate_forced(m._h, 0, f.ctypes.data_as(PI64), int(f.size), e.ctypes.data_as(PI64) if e.size else None, int(e.size),
                                     lp.ctypes.data_as(PF), gid.ctypes.data_as(PI64), glp.ctypes.data_as(PF), C.byref(kv))
    return rc, lp, gid.tolist(), glp, kv.value


def _forced(m, F, eos=()):
    rc, lp, gid, glp, kv = _forced_rc(m, F, eos)
    _lib.check(rc)
    return lp, gid, glp, kv


def _kv0(m, n):
    """layer 0's cached K / V rows of env 0, positions [0, n)"""
    K = np.zeros((n, m.cfg.kv_heads, 128), np.float32)
    V = np.zeros_like(K)
    _lib.check(m._lib.svln_op_kv_read(m._h, 0, 0, n, K.ctypes.data_as(PF), V.ctypes.data_as(PF)))
    return K, V


def _head(m):
    return torch.from_numpy(m.get_tensor("lm_head.weight")).double()


def _ref_scores(Wd, hidden, ids, inv_t=1.0):
    """float64 (log-probability of ids[k], arg-max, bound) per tap row: log_softmax(inv_t * W h); bound = the a-priori fp32 dot bound on
    either side of the softmax, scaled by inv_t, plus the op-level log-sum-exp bound"""
    gamma = Wd.shape[1] * 2.0 ** -24
    out = []
    for k, tok in enumerate(ids):
        h = torch.from_numpy(np.asarray(hidden[k], dtype=np.float64))
        y = (Wd @ h) * inv_t
        out.append((float(y[tok] - torch.logsumexp(y, 0)), int(torch.argmax(y)), 2 * gamma * float((Wd.abs() @ h.abs()).max()) * inv_t + LSE_TOL))
    return out


def _check_scores(Wd, lp, hidden, F, inv_t=1.0, what=""):
    worst = 0.0
    for k, (ref, _, bound) in enumerate(_ref_scores(Wd, hidden, F, inv_t)):
        err = abs(float(lp[k]) - ref)
        worst = max(worst, err / bound)
        assert err <= bound, (what, k, float(lp[k]), ref, err, bound)
    return worst


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------ (1) bit for bit
#: (history rows P, prompt rows Tn, ids n): fed rows across the first page edge (positions 62 .. 66); n = 3 (MFMA head, padded to 4);
#: n = 2 (the batched GEMV head); the most a ride feeds, across a page edge behind a history; n = 1 (nothing is fed)
RIDE_CASES = [(20, 42, 6), (0, 62, 3), (0, 63, 2), (70, 55, 8), (0, 40, 1)]


@DTYPES
def test_forced_turn_equals_the_ride_with_the_right_draft_bit_for_bit(dtype):
    m = model("tiny_episode", dtype)
    last = m.cfg.layers - 1
    try:
        for P, Tn, n in RIDE_CASES:
            seed, k, L = 100 * P + Tn, n - 1, P + Tn
            _begin(m, P, Tn, seed)
            F = _fixed(m, n)                                   # the plain loop's ids
            # the ride with the draft D = F
            m.set_prefill_draft(True)
            m.set_layer_taps(True, last)
            _begin(m, P, Tn, seed)
            d = np.ascontiguousarray(F, dtype=np.int64)
            _lib.check(m._lib.svln_set_draft(m._h, 0, d.ctypes.data_as(PI64), n))
            ids_r = _fixed(m, n)
            qkv_r, x_r, hid_r, kv_r = m.layer_probe(7), m.layer_probe(1), m.last_hidden(), _kv0(m, L + k)
            fed = m.prefill_draft_stats(reset=True)[2]
            m.set_prefill_draft(False)
            assert fed == k and qkv_r.shape[0] == Tn + k, (P, Tn, n, fed)
            # the forced turn
            _begin(m, P, Tn, seed)
            lp, gid, glp, kv = _forced(m, F)
            qkv_f, x_f, hid_f, kv_f = m.layer_probe(7), m.layer_probe(1), m.last_hidden(), _kv0(m, L + k)
            m.set_layer_taps(False)
            assert m.env_state(0) == (L, L + n - 1) and kv == L + n - 1
            assert np.array_equal(qkv_f, qkv_r) and np.array_equal(x_f, x_r), (P, Tn, n, "last layer's rows")
            assert np.array_equal(kv_f[0], kv_r[0]) and np.array_equal(kv_f[1], kv_r[1]), (P, Tn, n, "layer 0's cached K / V rows")
            # the ride emits while its head rows' arg-maxes equal the draft: every id it emitted is that row's arg-max
            rtok = 1
            while rtok < n and ids_r[rtok - 1] == F[rtok - 1]:
                rtok += 1
            assert hid_f.shape[0] == n and np.array_equal(hid_f[:rtok], hid_r[:rtok]), (P, Tn, n, "final-norm rows")
            assert gid[:rtok] == ids_r[:rtok], (P, Tn, n, gid, ids_r)
            if dtype == torch.float32:
                assert ids_r == F and gid == F and rtok == n, (P, Tn, n, gid, ids_r, F)
            for i in range(n):
                if gid[i] == F[i]:
                    assert lp[i].tobytes() == glp[i].tobytes(), (P, Tn, n, i, lp[i], glp[i])
            print(f"forced vs ride [{dtype}] P={P} Tn={Tn} n={n}: {rtok}/{n} ride rows, greedy {gid}, F {F}")
    finally:
        m.set_layer_taps(False)
        m.set_prefill_draft(False)


#: n = 12 with the forced rows across a KV page edge (positions 58 .. 68); n = 32 with Tn + n - 1 = 271 across 256 (the fused-norm limit of
#: the product plans) and across the page edge at 256
SPLICE_CASES = [(0, 58, 12), (0, 240, 32)]


@DTYPES
def test_forced_turn_equals_the_spliced_prefill_bit_for_bit(dtype):
    m = model("tiny_episode", dtype)
    cfg = m.cfg
    last = cfg.layers - 1
    norm_w = torch.from_numpy(m.get_tensor("model.norm.weight")).to(dtype).cuda()
    lm_head = torch.from_numpy(m.get_tensor("lm_head.weight")).to(dtype).cuda()
    Wd = _head(m)
    try:
        for P, Tn, n in SPLICE_CASES:
            seed, k, L = 100 * P + Tn, n - 1, P + Tn
            F = _prompt(n, seed + 2, cfg.vocab).tolist()        # ids the policy did not choose
            m.set_layer_taps(True, last)
            # run B: the caller splices the embeddings of F[:-1] on; a plain prefill of the same Tn + n - 1 rows
            _begin(m, P, Tn, seed)
            _append(m, F[:k])
            _fixed(m, 1)
            qkv_b, x_b = m.layer_probe(7, max_rows=320), m.layer_probe(1, max_rows=320)
            assert x_b.shape[0] == Tn + k
            rows = torch.from_numpy(x_b[Tn + k - n:]).to(dtype).cuda().contiguous()
            xn = torch.zeros((n, cfg.hidden), dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            _lib.check(m._lib.svln_op_rmsnorm(m._h, _ptr(rows), _ptr(norm_w), _ptr(xn), n, cfg.hidden, C.c_float(cfg.rms_eps)))
            toks, lps = (C.c_int32 * 32)(), (C.c_float * 32)()
            _lib.check(m._lib.svln_op_gemm_argmax_scores(m._h, _ptr(xn), cfg.hidden, _ptr(lm_head), cfg.hidden, n, cfg.vocab, cfg.hidden, None, None,
                                                         1.0, toks, lps))
            hid_b = xn.float().cpu().numpy()
            # run A: the forced turn
            _begin(m, P, Tn, seed)
            lp, gid, glp, kv = _forced(m, F)
            qkv_a, x_a, hid_a = m.layer_probe(7, max_rows=320), m.layer_probe(1, max_rows=320), m.last_hidden()
            m.set_layer_taps(False)
            assert np.array_equal(qkv_a, qkv_b) and np.array_equal(x_a, x_b), (P, Tn, n, "last layer's rows")
            assert hid_a.shape == hid_b.shape and np.array_equal(hid_a, hid_b), (P, Tn, n, "final-norm rows")
            assert gid == [int(toks[i]) for i in range(n)], (P, Tn, n, gid)
            assert glp.tobytes() == np.asarray([lps[i] for i in range(n)], np.float32).tobytes(), (P, Tn, n, "greedy_logprobs")
            assert m.env_state(0) == (L, L + n - 1) and kv == L + n - 1
            worst = _check_scores(Wd, lp, hid_a, F, what=(P, Tn, n))
            assert all(float(lp[i]) <= float(glp[i]) for i in range(n))
            print(f"forced vs splice [{dtype}] Tn={Tn} n={n}: worst |score - ref| / bound = {worst:.3f}")
    finally:
        m.set_layer_taps(False)


# ------------------------------------------------------------------------------------------------------------ episodes through the agent
class Forced:
    """the model with forced_ids added to generate: turn t of the episode is forced to ids(t) (None = a plain turn)"""

    def __init__(self, m, ids):
        self._m, self._ids, self.turn = m, ids, 0

    def __getattr__(self, k):
        return getattr(self._m, k)

    def generate(self, *a, **kw):
        f = self._ids(self.turn)
        self.turn += 1
        if f is not None:
            kw["forced_ids"] = f
        return self._m.generate(*a, **kw)


def _episode(m, sc, ids, steps=None):
    taps = []

    def on_turn(t, rec):
        taps.append(dict(out=rec["out"], hidden=m.last_hidden(), cache_len=m.env_state(0)[1]))
    run_scenario(Forced(m, ids), sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, on_turn=on_turn, device="cuda", steps=steps)
    return taps


@DTYPES
@pytest.mark.parametrize("name", ["tiny_episode", "true4_episode"])
def test_the_fixtures_own_ids_reproduce_the_fixtures(name, dtype):
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    m = model(name, dtype)
    taps = _episode(m, sc, lambda t: gold[t])
    assert len(taps) == len(gold)
    for t, tap in enumerate(taps):
        out, n = tap["out"], len(gold[t])
        assert out.sequences[0].tolist() == gold[t] and tap["cache_len"] == int(g[f"t{t}_cache_len"]), (name, t)
        assert tuple(out.token_logprobs.shape) == (1, n) and out.token_logprobs.dtype == torch.float32
        assert tuple(out.greedy_ids.shape) == (1, n) and out.greedy_ids.dtype == torch.int64 and tuple(out.greedy_logprobs.shape) == (1, n)
        gid, hf = out.greedy_ids[0].tolist(), g[f"t{t}_hidden"]
        if dtype == torch.float32:
            assert float(np.abs(tap["hidden"] - hf[:n]).max()) <= HIDDEN_TOL, (name, t)
            assert gid == gold[t], (name, t, gid, gold[t])
            assert torch.equal(out.token_logprobs, out.greedy_logprobs) and out.token_logprobs.numpy().tobytes() == out.greedy_logprobs.numpy().tobytes()
        else:
            for j in range(n):          # the rows are forced onto the fixture's ids: every one is compared (no divergence to stop at)
                rel = float(np.linalg.norm(tap["hidden"][j] - hf[j]) / np.linalg.norm(hf[j]))
                assert rel < BF16_HIDDEN_REL[name], (name, t, j, rel)
            for j in range(n):
                if gid[j] == gold[t][j]:
                    assert out.token_logprobs[0, j].numpy().tobytes() == out.greedy_logprobs[0, j].numpy().tobytes(), (name, t, j)
                else:
                    assert float(out.token_logprobs[0, j]) <= float(out.greedy_logprobs[0, j]), (name, t, j)


def _other(tok, sc, avoid=()):
    eos = set(eos_ids(sc))
    return next(t for t in range(5, sc["cfg"].vocab) if t != tok and t not in eos and t not in avoid)


@DTYPES
@pytest.mark.parametrize("where", ["index0", "index1", "last"])
def test_ids_the_policy_did_not_choose(where, dtype):
    """turn 0 of tiny_episode forced onto the fixture's ids with one id replaced by an id that is neither the arg-max nor in the EOS set;
    turn 1 plain.  The oracle runs the same two turns teacher-forced on the same ids."""
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    gold0 = g["t0_ids"].tolist()
    assert len(gold0) >= 2
    j = {"index0": 0, "index1": 1, "last": len(gold0) - 1}[where]
    F = list(gold0)
    F[j] = _other(gold0[j], sc)
    m = model(name, dtype)
    taps = _episode(m, sc, lambda t: F if t == 0 else None, steps=2 * sc["nfs"])
    assert len(taps) == 2
    orc = O.OracleStreamVLN(sc["cfg"], Wt.synth_state_dict(sc["cfg"], SEED), num_history=sc["num_history"])
    orc.teacher_tokens = [list(F)]
    log_o = run_scenario(orc, sc, preprocess=m.get_vision_tower().image_processor.preprocess_array, steps=2 * sc["nfs"])
    o0, o1 = log_o[0]["out"], log_o[1]["out"]
    out0, out1 = taps[0]["out"], taps[1]["out"]
    assert out0.sequences[0].tolist() == F == o0.sequences[0].tolist() and taps[0]["cache_len"] == o0.cache_len
    gid = out0.greedy_ids[0].tolist()
    worst = _check_scores(_head(m), out0.token_logprobs[0].tolist(), taps[0]["hidden"], F, what=(where, str(dtype)))
    assert float(out0.token_logprobs[0, j]) < float(out0.greedy_logprobs[0, j]) and gid[j] != F[j]
    if dtype == torch.float32:
        assert float(np.abs(taps[0]["hidden"] - o0.hidden.numpy()).max()) <= HIDDEN_TOL, where
        assert gid == o0.own_picks, (where, gid, o0.own_picks)
        # the next plain turn continues from F, as the oracle's does
        assert out1.sequences[0].tolist() == o1.sequences[0].tolist() and taps[1]["cache_len"] == o1.cache_len, where
        assert float(np.abs(taps[1]["hidden"] - o1.hidden.numpy()).max()) <= HIDDEN_TOL, where
    else:
        for r in range(len(F)):
            rel = float(np.linalg.norm(taps[0]["hidden"][r] - o0.hidden.numpy()[r]) / np.linalg.norm(o0.hidden.numpy()[r]))
            assert rel < BF16_HIDDEN_REL[name], (where, r, rel)
        n1 = min(len(out1.sequences[0]), o1.hidden.shape[0])
        rel = float(np.linalg.norm(taps[1]["hidden"][0] - o1.hidden.numpy()[0]) / np.linalg.norm(o1.hidden.numpy()[0]))
        assert n1 >= 1 and rel < BF16_HIDDEN_REL[name], (where, rel)
        if o1.margins[0] > 0.05:                               # (BF16_MARGIN of test_e2e_gpu.py: above it the first id must agree)
            assert int(out1.sequences[0, 0]) == int(o1.sequences[0, 0]), where
    print(f"F differs at {where} [{dtype}]: worst |score - ref| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------ sampling, allowed list
def _generate(m, max_new):
    out, n = np.zeros(max_new, np.int64), C.c_int32()
    _lib.check(m._lib.svln_generate(m._h, 0, max_new, None, 0, out.ctypes.data_as(PI64), max_new, C.byref(n)))
    return out[:n.value].tolist()


def _token_scores(m, n):
    buf, k = np.zeros(n, np.float32), C.c_int32()
    _lib.check(m._lib.svln_get_token_scores(m._h, buf.ctypes.data_as(PF), n, C.byref(k)))
    assert k.value == n
    return buf


@DTYPES
def test_sampling_scores_and_the_untouched_draw_counter(dtype):
    """T = 1/2: F = the ids of a sampled turn.  The forced scores are those of softmax(logits / T), as the sampled turn reports them.  The
    two turns' tap rows are not the same rows -- the sampled turn's ids 1 .. n - 1 come from decode steps, whose bf16 rows differ from the
    prefill's by a rounding of the row (measured |score difference| there 0.9 .. 1.8e-2 against 2.1e-3 for the a-priori bound; 2e-6 on the
    fp32 engine) -- so the claim is made in three parts, each against a figure fixed beforehand: (a) every forced score inside the bound
    (scaled by 1 / T) of float64 from the forced turn's own tap rows; (b) every score of the sampled turn inside the same bound of float64
    from ITS own tap rows; (c) the two sets of rows within the project's row tolerances of each other (fp32: 1e-3 absolute, HIDDEN_TOL;
    bf16: relative L2 below BF16_HIDDEN_REL; measured 3.1e-6 absolute and 8.0 .. 8.7e-3 relative).  Where the rows agree to fp32 rounding (the fp32 engine; id 0, the prefill's row, on both) the
    bound is asserted between the two turns' scores directly.  No draw is consumed: the next sampled turn repeats the one of a twin whose
    counters were restarted after its forced turn, and differs from the one that follows a turn that did consume draws."""
    m = model("tiny_episode", dtype)
    T, seed, n = 0.5, 21, 5
    V, Wd = m.cfg.vocab, _head(m)
    inv_t = float(np.float32(1.0) / np.float32(T))
    nxt = _prompt(9, 8, V).tolist()
    m.set_token_scores(True)
    m.set_sampling(T, seed)
    _begin(m, 0, 50, 7)
    S = _generate(m, n)
    lp_s, hid_s = _token_scores(m, n), m.last_hidden()
    assert len(S) == n
    # the forced turn on S, then a sampled turn
    m.set_sampling(T, seed)                                    # (restarts the draw counters)
    _begin(m, 0, 50, 7)
    lp, gid, glp, kv = _forced(m, S)
    hid_f = m.last_hidden()
    worst = _check_scores(Wd, lp, hid_f, S, inv_t, what=("sampling, forced", str(dtype)))                      # (a)
    worst_s = _check_scores(Wd, lp_s, hid_s, S, inv_t, what=("sampling, sampled", str(dtype)))                  # (b)
    refs = _ref_scores(Wd, hid_f, S, inv_t)
    assert hid_f.shape == hid_s.shape == (n, m.cfg.hidden)
    for i in range(n):                                                                                          # (c)
        dh = float(np.abs(hid_f[i].astype(np.float64) - hid_s[i]).max())
        rel = float(np.linalg.norm(hid_f[i].astype(np.float64) - hid_s[i]) / np.linalg.norm(hid_s[i].astype(np.float64)))
        print(f"sampling [{dtype}] id {i}: forced {lp[i]:.6f} sampled {lp_s[i]:.6f} |diff| {abs(lp[i] - lp_s[i]):.3e} bound {refs[i][2]:.3e}; "
              f"rows: max |diff| {dh:.3e}, rel L2 {rel:.3e}")
        if dtype == torch.float32:
            assert dh <= HIDDEN_TOL, (i, dh)
        else:
            assert rel < BF16_HIDDEN_REL["tiny_episode"], (i, rel)
        if dtype == torch.float32 or i == 0:
            assert abs(float(lp[i]) - float(lp_s[i])) <= refs[i][2], (i, lp[i], lp_s[i], refs[i][2])
    _append(m, S + nxt)
    ids2 = _generate(m, n)
    # the twin: its forced turn ran with sampling off; the counters start when the switch goes on
    m.set_sampling(None)
    _begin(m, 0, 50, 7)
    lp_g, _, _, _ = _forced(m, S)
    m.set_sampling(T, seed)
    _append(m, S + nxt)
    ids2_twin = _generate(m, n)
    assert ids2 == ids2_twin, (ids2, ids2_twin)
    # with sampling off the same call scores softmax(logits): different numbers
    assert not np.array_equal(lp_g, lp)
    # a turn sampled with draws that HAVE moved differs (T = 1/2 on random-initialised weights leaves the greedy path)
    m.set_sampling(T, seed)
    _begin(m, 0, 50, 7)
    assert _generate(m, n) == S
    _append(m, S + nxt)
    moved = _generate(m, n)
    assert moved != ids2, (moved, ids2)
    print(f"sampling [{dtype}]: worst |score - ref| / bound = {worst:.3f} (forced), {worst_s:.3f} (sampled); next turn {ids2}, after a sampled turn "
          f"(draws moved) {moved}")
    m.set_sampling(None)
    m.set_token_scores(False)


@DTYPES
def test_allowed_list(dtype):
    """the head is the subset product: logprobs[i] is bit-equal to allowed_logprobs[i, pos(F[i])], greedy ids lie in the list, an id
    outside the list is refused before anything changes"""
    m = model("tiny_episode", dtype)
    V = m.cfg.vocab
    allowed = sorted(set(_prompt(40, 3, V).tolist()))
    F = [allowed[3], allowed[17], allowed[0], allowed[-1], allowed[17]]
    try:
        m.set_allowed_tokens(allowed, add_eos=False)
        for T in (None, 0.5):
            m.set_sampling(T, 5) if T else m.set_sampling(None)
            _begin(m, 0, 50, 7)
            state = m.env_state(0)
            outside = next(t for t in range(5, V) if t not in allowed)
            rc = _forced_rc(m, [allowed[1], outside, allowed[2]])[0]
            assert rc != 0 and b"allowed list" in m._lib.svln_last_error() and m.env_state(0) == state
            lp, gid, glp, kv = _forced(m, F)
            buf, nt, ni = np.zeros(len(F) * len(allowed), np.float32), C.c_int32(), C.c_int32()
            _lib.check(m._lib.svln_get_allowed_logprobs(m._h, buf.ctypes.data_as(PF), int(buf.size), C.byref(nt), C.byref(ni)))
            assert (nt.value, ni.value) == (len(F), len(allowed))
            alp = buf.reshape(len(F), len(allowed))
            for i, f in enumerate(F):
                assert lp[i].tobytes() == alp[i, allowed.index(f)].tobytes(), (T, i, lp[i], alp[i, allowed.index(f)])
                assert gid[i] in allowed and gid[i] == allowed[int(np.argmax(alp[i]))]
                assert abs(float(glp[i]) - float(alp[i].max())) <= LSE_TOL
            assert abs(float(np.exp(alp.astype(np.float64)).sum(1).max()) - 1.0) <= 1e-4
        m.set_sampling(None)
    finally:
        m.set_sampling(None)
        m.set_allowed_tokens(None)


# ------------------------------------------------------------------------------------------------------------ the agent
def test_agent_path():
    name = "tiny_episode"
    sc, g = SCENARIOS[name], load_golden(name)
    gold = [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]
    m = model(name, torch.float32)
    enc = SyntheticPromptEncoder(sc["cfg"], seed=7, first_len=sc["lens"][0], memory_len=sc["lens"][1], later_len=sc["lens"][2])
    agent = StreamingAgent(m, enc, num_frames=sc["num_frames"], num_future_steps=sc["nfs"], num_history=sc["num_history"],
                           max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=m.get_vision_tower().image_processor.preprocess_array,
                           device="cuda")
    assert agent.last_greedy_ids is None
    F = list(gold[0])
    F[0] = _other(gold[0][0], sc)
    agent.act(synthetic_frame(0, 0), forced_ids=F)
    out = agent.turn_log[-1]["out"]
    assert out.sequences[0].tolist() == F and agent.output_ids[0].tolist() == F
    assert torch.equal(agent.last_token_logprobs, out.token_logprobs) and tuple(agent.last_token_logprobs.shape) == (1, len(F))
    assert abs(agent.last_turn_logprob - float(out.token_logprobs.sum())) <= 1e-6
    assert agent.last_greedy_ids[0].tolist() == out.greedy_ids[0].tolist() and agent.last_greedy_ids[0, 0].item() == gold[0][0]
    # no model turn runs at the next step: the argument raises before anything changes
    state, step_id, frames = m.env_state(0), agent.step_id, len(agent.rgb_list)
    with pytest.raises(ValueError, match="no model turn"):
        agent.act(synthetic_frame(0, 1), forced_ids=F)
    assert (m.env_state(0), agent.step_id, len(agent.rgb_list)) == (state, step_id, frames)
    for step in range(1, sc["nfs"]):
        agent.act(synthetic_frame(0, step))
    agent.act(synthetic_frame(0, sc["nfs"]))                   # a plain turn follows a forced one with nothing special
    assert len(agent.turn_log) == 2 and agent.last_greedy_ids is None and agent.last_token_logprobs is None
    agent.reset_memory()
    assert agent.last_greedy_ids is None


# ------------------------------------------------------------------------------------------------------------ rules
def test_refusals_and_what_is_allowed():
    sc = SCENARIOS["tiny_episode"]
    m = StreamVLNForCausalLM(sc["cfg"], dtype=torch.bfloat16, max_envs=2, max_frames=3, max_positions=256)
    try:
        m.load_synthetic(SEED)
        V = m.cfg.vocab
        F = [11, 12, 13]

        def refused(ids, match, eos=()):
            state = m.env_state(0)
            rc = _forced_rc(m, ids, eos)[0]
            err = m._lib.svln_last_error().decode()
            assert rc != 0 and match in err, (ids, match, err)
            assert m.env_state(0) == state

        m.reset(1)
        refused(F, "nothing to prefill")
        _begin(m, 0, 40, 1)
        refused([], "1 .. 32")
        refused(list(range(5, 38)), "1 .. 32")
        refused([11, V, 13], "outside the vocabulary")
        refused([11, -1, 13], "outside the vocabulary")
        refused([11, 12, 13], "EOS", eos=(12,))
        assert _forced_rc(m, [11, 13, 12], eos=(12,))[0] == 0               # an EOS id last is a turn that ended by EOS
        assert m.env_state(0) == (40, 42)
        _begin(m, 0, 240, 1)
        refused(list(range(5, 23)), "max_positions")                        # 240 + 18 - 1 > 256
        assert _forced_rc(m, list(range(5, 22)))[0] == 0 and m.env_state(0) == (240, 256)
        _begin(m, 0, 40, 1)
        _lib.check(m._lib.svln_set_repetition_penalty(m._h, 1.3))
        refused(F, "svln_set_repetition_penalty")
        _lib.check(m._lib.svln_set_repetition_penalty(m._h, 1.0))
        for sym, fn in {"svln_set_fp8_decode": m.set_fp8_decode, "svln_set_mxfp4_decode": m.set_mxfp4_decode, "svln_set_fp8_gemm": m.set_fp8_gemm,
                        "svln_set_decode_persistent": m.set_decode_persistent}.items():
            fn(True)
            refused(F, sym)
            fn(False)
        # scheduler turns in flight (on the other env)
        m.reset(2)
        ids = np.arange(10, 30, dtype=np.int64)
        slot = C.c_int32(-1)
        _lib.check(m._lib.svln_append_turn(m._h, 1, ids.ctypes.data_as(PI64), len(ids), 0))
        _lib.check(m._lib.svln_batch_submit(m._h, 1, 4, None, 0, C.byref(slot)))
        _lib.check(m._lib.svln_append_turn(m._h, 0, ids.ctypes.data_as(PI64), len(ids), 0))
        refused(F, "in flight")
        _lib.check(m._lib.svln_batch_cancel(m._h, -1))
        # a pending group
        m.reset(1)
        m.set_sampling(1.0, 3)
        _begin(m, 0, 40, 1)
        out, n_out = np.zeros((2, 3), np.int64), np.zeros(2, np.int32)
        _lib.check(m._lib.svln_generate_group(m._h, 0, 2, 3, None, 0, out.ctypes.data_as(PI64), 3, n_out.ctypes.data_as(PI32)))
        rc = _forced_rc(m, F)[0]
        assert rc != 0 and "svln_group_select" in m._lib.svln_last_error().decode()
        _lib.check(m._lib.svln_group_select(m._h, 0, 0, None))
        m.set_sampling(None)
        # allowed: the draft switches (an armed draft is consumed), the scores either way, the batched MXFP4 weights
        base = None
        for setup in ("plain", "speculative", "prefill_draft", "batch_draft", "token_scores", "mxfp4_batched"):
            m.set_speculative(4 if setup == "speculative" else 0)
            m.set_prefill_draft(setup == "prefill_draft")
            m.set_batch_draft(setup == "batch_draft")
            m.set_token_scores(setup == "token_scores")
            m.set_mxfp4_batched(setup == "mxfp4_batched")
            _begin(m, 0, 40, 1)
            if setup in ("speculative", "prefill_draft"):
                d = np.asarray([21, 22, 23], np.int64)
                _lib.check(m._lib.svln_set_draft(m._h, 0, d.ctypes.data_as(PI64), 3))
            lp, gid, glp, kv = _forced(m, F)
            if base is None:
                base = (lp.copy(), gid, glp.copy(), kv)
            assert np.array_equal(lp, base[0]) and gid == base[1] and np.array_equal(glp, base[2]) and kv == base[3] == 42, setup
            if setup == "prefill_draft":                        # the draft was consumed: the next plain turn rides nothing
                _append(m, F + [31, 32])
                _fixed(m, 2)
                assert m.prefill_draft_stats(reset=True) == (0, 0, 0)
            top = np.zeros(2, np.float32)
            if setup == "plain":
                assert m._lib.svln_get_top2(m._h, top.ctypes.data_as(PF)) != 0
        m.set_speculative(0); m.set_prefill_draft(False); m.set_batch_draft(False); m.set_token_scores(False); m.set_mxfp4_batched(False)
    finally:
        m.close()
