"""Dead decode steps on the GPU: the launches a run-ahead batch enqueues behind the end of a generation (engine.hip decode_steps; every
launch of a step is a no-op once GenCtl.done is set).  TINY config, max_envs = 1, text-only prompts through the public calls.

(1) test_dead_step_writes_nothing: the test-only entry svln_op_dead_step replays ONE step (decode_ops over the whole step + head, the
    captured one-step graph when the graph is on) behind a finished generation with done = 1 and compares every buffer a step may touch
    with a host snapshot: the K / V^T pools of every layer, the split-KV partials, x / qkv / attn / hbuf / head_xn / hid_tap, every
    partial, candidate and truncation array, d_token, d_out_ids, d_scores, d_topi, d_topl, d_ent, d_alp, pen_flags, d_top2, the granule
    and sequence words of the persistent layer and GenCtl.  Nothing may change; SCRATCH_EXCLUSIONS (pure scratch that the next live step
    overwrites before reading) is empty.  With done = 0 on the same engine the step is live: the K / V^T slot of GenCtl.pos (and only
    that slot of the pools), d_out_ids and GenCtl change, so the probe cannot pass vacuously.

(2) test_early_end_inside_a_batch_equals_an_end_with_no_dead_step: per configuration, on fresh engines (the pools are zeroed at engine
    creation and fresh engines hand out pages in the same order, so the raw pools are comparable and no fill control is needed): a free
    run of 9 tokens g; then for every t in 1 .. 6 turn A ends at token t by the EOS list {g[t - 1]} with max_new = 9 -- RUN_AHEAD = 4
    leaves 4, 3, 2, 1, 0, 3 dead steps behind it -- and turn B ends at the same token by max_new = t, where the host never enqueues a
    step past the end.  A and B must agree bit for bit on the ids, the svln_get_hidden rows, the scores / lists / entropies / allowed
    log-probabilities where the head is on, svln_get_top2, svln_env_state and the raw K / V^T pools of every layer, and again after a
    second turn (the first turn's own ids, then new text) of 3 tokens: a leaked penalty flag or a rewritten KV slot shows there.  The prompt seed of every configuration is in
    SEEDS; g[0 .. 6) pairwise distinct is asserted, so that a change of weights fails loudly instead of dropping a t.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from scenarios import SEED
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM

pytestmark = pytest.mark.gpu
PI64, PI32, PF = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)
F32, BF16 = torch.float32, torch.bfloat16
MAX_POS = 256
PROMPT_LEN, TURN2_LEN = 21, 5
ALLOWED = tuple(range(7, 4096, 64))                    # 64 ids for the allowed-token head
SMP_SEED = 0x5EED

# a buffer a dead step may write: pure scratch that the next live step overwrites before reading -- name -> reason.  Pools, flags,
# output rows, d_token and GenCtl may never be listed.
SCRATCH_EXCLUSIONS = {}
NEVER_EXCLUDED = ("kpool", "vpool", "pen_flags", "d_out_ids", "d_scores", "d_topi", "d_topl", "d_ent", "d_alp", "d_token", "d_top2", "ctl", "hid_tap")


def _scores(L, h):
    _lib.check(L.svln_set_token_scores(h, 1))


def _sampling(L, h):
    _scores(L, h)
    _lib.check(L.svln_set_sampling(h, 1, 1.0, SMP_SEED))


def _trunc(L, h):
    _sampling(L, h)
    _lib.check(L.svln_sampling_truncation(h, 5, 0.9))


def _topk(L, h):
    _scores(L, h)
    _lib.check(L.svln_top_logprobs(h, 5))


def _entropy(L, h):
    _scores(L, h)
    _lib.check(L.svln_token_entropy(h, 1))


def _allowed(L, h):
    ids = np.asarray(ALLOWED, dtype=np.int64)
    _lib.check(L.svln_set_allowed_tokens(h, ids.ctypes.data_as(PI64), ids.size))
    _scores(L, h)


# name -> (engine dtype, hipGraph replay, switches).  Speculative, ride and batch drafts stay off: they have their own step kernel.
CONFIGS = {
    "fp32": (F32, True, None),
    "fp32-nograph": (F32, False, None),
    "bf16-packed": (BF16, True, lambda L, h: _lib.check(L.svln_set_packed_decode(h, 1))),        # (the bf16 default)
    "bf16-unpacked": (BF16, True, lambda L, h: _lib.check(L.svln_set_packed_decode(h, 0))),
    "bf16-e4m3": (BF16, True, lambda L, h: _lib.check(L.svln_set_fp8_decode(h, 1))),
    "bf16-mxfp4": (BF16, True, lambda L, h: _lib.check(L.svln_set_mxfp4_decode(h, 1))),
    "bf16-persistent": (BF16, True, lambda L, h: _lib.check(L.svln_set_decode_persistent(h, 1))),
    "bf16-scores": (BF16, True, _scores),
    "bf16-sampling": (BF16, True, _sampling),
    "bf16-sampling-trunc": (BF16, True, _trunc),
    "bf16-top-logprobs": (BF16, True, _topk),
    "bf16-entropy": (BF16, True, _entropy),
    "bf16-allowed-scores": (BF16, True, _allowed),
    "bf16-penalty": (BF16, True, lambda L, h: _lib.check(L.svln_set_repetition_penalty(h, 1.3))),
}
# prompt seed per configuration: the first for which the free run's g[0 .. 6) are pairwise distinct (asserted below)
SEEDS = {name: 0 for name in CONFIGS}
SEEDS["bf16-allowed-scores"] = 2


def prompt(seed, n=PROMPT_LEN):
    return np.random.default_rng(1000 + seed).integers(0, TINY.vocab, n).astype(np.int64)


def fresh(name):
    dtype, graph, switches = CONFIGS[name]
    m = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=1, max_positions=MAX_POS)
    m.load_synthetic(SEED)
    _lib.check(m._lib.svln_set_decode_graph(m._h, int(graph)))
    if switches:
        switches(m._lib, m._h)
    return m


def append(m, ids):
    _lib.check(m._lib.svln_append_turn(m._h, 0, ids.ctypes.data_as(PI64), ids.size, 0))


def generate(m, max_new, eos=()):
    out, n, e = np.zeros(max_new, dtype=np.int64), C.c_int32(), np.asarray(eos, dtype=np.int64)
    _lib.check(m._lib.svln_generate(m._h, 0, max_new, e.ctypes.data_as(PI64) if e.size else None, e.size, out.ctypes.data_as(PI64), max_new, C.byref(n)))
    return out[:n.value].tolist()


def observe(m, name, ids):
    """everything the public getters and the raw-pool read return after a turn, as bytes"""
    L, h, n, k = m._lib, m._h, C.c_int32(), C.c_int32()
    obs = {"ids": tuple(ids), "env_state": m.env_state(0)}
    hid = np.zeros((64, TINY.hidden), np.float32)
    _lib.check(L.svln_get_hidden(h, hid.ctypes.data_as(PF), 64, C.byref(n)))
    assert n.value == len(ids)
    obs["hidden"] = hid[:n.value].tobytes()
    top2 = np.zeros(2, np.float32)
    rc = L.svln_get_top2(h, top2.ctypes.data_as(PF))           # (refused after a sampled turn: the refusal itself must agree)
    obs["top2"] = (rc, top2.tobytes() if rc == 0 else None)
    if name not in ("fp32", "fp32-nograph", "bf16-packed", "bf16-unpacked", "bf16-e4m3", "bf16-mxfp4", "bf16-persistent", "bf16-penalty"):
        sc = np.zeros(16, np.float32)
        _lib.check(L.svln_get_token_scores(h, sc.ctypes.data_as(PF), 16, C.byref(n)))
        assert n.value == len(ids)
        obs["scores"] = sc[:n.value].tobytes()
    if name == "bf16-top-logprobs":
        ti, tl = np.zeros((16, 8), np.int32), np.zeros((16, 8), np.float32)
        _lib.check(L.svln_get_topk(h, ti.ctypes.data_as(PI32), tl.ctypes.data_as(PF), 16, C.byref(n), C.byref(k)))
        assert n.value == len(ids) and k.value == 5
        obs["topk"] = (ti.reshape(-1)[:n.value * 5].tobytes(), tl.reshape(-1)[:n.value * 5].tobytes())
    if name == "bf16-entropy":
        en = np.zeros(16, np.float32)
        _lib.check(L.svln_get_token_entropy(h, en.ctypes.data_as(PF), 16, C.byref(n)))
        assert n.value == len(ids)
        obs["entropy"] = en[:n.value].tobytes()
    if name == "bf16-allowed-scores":
        al = np.zeros(16 * len(ALLOWED), np.float32)
        _lib.check(L.svln_get_allowed_logprobs(h, al.ctypes.data_as(PF), al.size, C.byref(n), C.byref(k)))
        assert n.value == len(ids) and k.value == len(ALLOWED)
        obs["allowed"] = al[:n.value * k.value].tobytes()
    rows = MAX_POS                                             # max_envs = 1: the pool holds MAX_POS / 64 pages
    for layer in range(TINY.layers):
        kk, vv = np.zeros((rows, TINY.kv_heads, 128), np.float32), np.zeros((rows, TINY.kv_heads, 128), np.float32)
        _lib.check(L.svln_op_kv_pool_read(h, layer, 0, rows, kk.ctypes.data_as(PF), vv.ctypes.data_as(PF)))
        obs[f"kpool.{layer}"], obs[f"vpool.{layer}"] = kk.tobytes(), vv.tobytes()
    return obs


def _differs(a, b):
    return [key for key in a if a[key] != b.get(key)] + [key for key in b if key not in a]


# ------------------------------------------------------------------------------------------------------------ (2) differential, end to end
def _turn_pair(name, seed, max_new, eos):
    """fresh engine: the turn, what it left, a second turn of 3 tokens, what that left"""
    m = fresh(name)
    append(m, prompt(seed))
    ids = generate(m, max_new, eos)
    first = observe(m, name, ids)
    append(m, np.concatenate([np.asarray(ids, dtype=np.int64), prompt(seed + 500, TURN2_LEN)]))      # the turn's own ids, then new text
    ids2 = generate(m, 3)
    second = observe(m, name, ids2)
    m.close()
    return first, second


@pytest.mark.parametrize("name", list(CONFIGS))
def test_early_end_inside_a_batch_equals_an_end_with_no_dead_step(name):
    seed = SEEDS[name]
    m = fresh(name)
    assert m.env_state(0) == (0, 0)
    append(m, prompt(seed))
    g = generate(m, 9)
    m.close()
    assert len(g) == 9 and len(set(g[:6])) == 6, (name, seed, g)           # the condition on the inputs: every t in 1 .. 6 is a case
    for t in range(1, 7):
        a1, a2 = _turn_pair(name, seed, 9, [g[t - 1]])                     # ends at token t by EOS: dead steps behind it
        b1, b2 = _turn_pair(name, seed, t, [])                             # ends at token t by max_new: no step past it
        assert a1["ids"] == tuple(g[:t]) == b1["ids"], (name, t, a1["ids"], b1["ids"], g)
        assert a1["env_state"] == (PROMPT_LEN, PROMPT_LEN + t - 1)
        assert not _differs(a1, b1), (name, t, "after the turn", _differs(a1, b1))
        assert len(a2["ids"]) == 3 and not _differs(a2, b2), (name, t, "after the second turn", _differs(a2, b2), a2["ids"], b2["ids"])
    if name in ("fp32", "bf16-scores"):                                    # the pools are what the turn wrote: not all zero, and zero behind it
        k0 = np.frombuffer(b1["kpool.0"], np.float32).reshape(MAX_POS, -1)
        assert np.count_nonzero(np.abs(k0).sum(1)) == PROMPT_LEN + 5, np.nonzero(np.abs(k0).sum(1))[0].tolist()


# ------------------------------------------------------------------------------------------------------------ (1) a dead step writes nothing
def dead_step(m, done):
    buf, n = C.create_string_buffer(1 << 14), C.c_int32()
    _lib.check(m._lib.svln_op_dead_step(m._h, done, buf, len(buf), C.byref(n)))
    rep = {}
    for line in buf.value.decode().splitlines():
        nm, size, changed, first, last = line.split()
        rep[nm] = (int(size), int(changed), int(first), int(last))
    assert sum(1 for v in rep.values() if v[1]) == n.value
    return rep


@pytest.mark.parametrize("name", list(CONFIGS))
def test_dead_step_writes_nothing(name):
    assert not any(k.startswith(NEVER_EXCLUDED) for k in SCRATCH_EXCLUSIONS)
    m = fresh(name)
    es = 4 if CONFIGS[name][0] == F32 else 2
    append(m, prompt(SEEDS[name]))
    g = generate(m, 2)                                                      # prefill head + one decode step; GenCtl.pos = PROMPT_LEN
    assert len(g) == 2 and g[0] != g[1], g
    rep = dead_step(m, 1)
    want = {f"{p}.{i}" for p in ("kpool", "vpool") for i in range(TINY.layers)} | {
        "attn_part", "x", "qkv", "attn", "hbuf", "head_xn", "hid_tap", "part_val", "part_idx", "part_sum", "part_raw", "part_max", "d_token",
        "d_out_ids", "d_scores", "d_top2", "ctl"}
    want |= {"bf16-sampling-trunc": {"tr_val", "tr_idx", "tr_sum", "tr_raw", "tr_max", "cand_val", "cand_idx"},
             "bf16-top-logprobs": {"cand_val", "cand_idx", "d_topi", "d_topl"}, "bf16-entropy": {"part_ent", "d_ent"}, "bf16-allowed-scores": {"d_alp"},
             "bf16-penalty": {"pen_flags"}, "bf16-persistent": {"dl_seq"} | {f"dl_gran.{k}" for k in range(4)}}.get(name, set())
    assert want <= set(rep), (name, sorted(want - set(rep)))
    wrote = {k: v for k, v in rep.items() if v[1] and k not in SCRATCH_EXCLUSIONS}
    assert not wrote, (name, "a dead step wrote", wrote)
    # the same step, live: the KV slot of pos in every layer (and nothing else of the pools), d_out_ids and GenCtl change
    live = dead_step(m, 0)
    pos, page_k = PROMPT_LEN, TINY.kv_heads * 64 * 128 * es
    for i in range(TINY.layers):
        size, changed, first, last = live[f"kpool.{i}"]                    # K [page][kv head][64][128]: row pos of every head of one page
        assert 0 < changed <= TINY.kv_heads * 128 * es and first // page_k == last // page_k, (name, i, live[f"kpool.{i}"])
        lo, hi = first % page_k, last % page_k
        assert lo >= pos * 128 * es and hi < ((TINY.kv_heads - 1) * 64 + pos + 1) * 128 * es, (name, i, lo, hi)
        assert (lo // (128 * es)) % 64 == pos and (hi // (128 * es)) % 64 == pos, (name, i, lo, hi)
        size, changed, first, last = live[f"vpool.{i}"]                    # V^T [page][kv head][128][64]: column pos
        assert 0 < changed <= TINY.kv_heads * 128 * es and first // page_k == last // page_k, (name, i, live[f"vpool.{i}"])
        assert (first // es) % 64 == pos and (last // es) % 64 == pos, (name, i, first, last)
    assert live["d_out_ids"][1] and live["d_out_ids"][2] // 4 == 2 and live["d_out_ids"][3] // 4 == 2, live["d_out_ids"]      # row count = 2
    assert live["ctl"][1], live["ctl"]
    assert live["x"][1] and live["qkv"][1] and live["part_val"][1]
    m.close()
