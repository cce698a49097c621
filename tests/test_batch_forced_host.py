"""Host surface of forced jobs in the scheduler (no GPU): the header declares the three entries, the ctypes table binds them with the
declared argument counts and types, the library exports them; no new svln_set_* switch; submit / generate_batch still refuse a forced_ids
key; the result a forced ticket gets from step_batch and the order of generate_batch_forced's results, on a fake library; the agents'
argument."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import switches_ref
from streamvln_amd import _lib
from streamvln_amd.agent import AsyncBatchedAgents, BatchedAgents, _forced_map
from streamvln_amd.model import GenerateOutput, KVHandle, StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_batch_submit_forced": 7, "svln_batch_forced": 7, "svln_batch_forced_stats": 5}


def _prototypes():
    header = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
    return header, {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(svln_\w+)\s*\(([^;]*)\);", header, flags=re.M)}


def test_header_declares_the_entries():
    header, protos = _prototypes()
    for name, n_args in ENTRIES.items():
        assert name in protos, f"{name} is not declared"
        assert protos[name].count(",") + 1 == n_args, (name, protos[name])
    assert {p for p in protos if p.startswith("svln_batch_") and "forced" in p} == set(ENTRIES)
    for word in ("all or nothing", "never fed", "slot order", "chunks of <= 32", "pad rows carry target", "consumed iff svln_set_batch_draft", "refused by name",
                 "svln_set_mxfp4_batched on", "no draw counter moves"):
        assert word in header, word


def test_signatures_match_the_header():
    p, i = C.c_void_p, C.c_int
    pi32, pi64, pf = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_batch_submit_forced"][1] == [p, i, pi64, i, pi64, i, pi32]
    assert _lib.SIGNATURES["svln_batch_forced"][1] == [p, i, pf, pi64, pf, i, pi32]
    assert _lib.SIGNATURES["svln_batch_forced_stats"][1] == [p, pi64, pi64, pi64, i]
    # the forced submit takes what the plain submit takes, with (ids, n) in place of max_new_tokens
    plain = _lib.SIGNATURES["svln_batch_submit"][1]
    assert plain == [p, i, i, pi64, i, pi32]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_no_new_switch():
    _, protos = _prototypes()
    setters = {p for p in protos if p.startswith("svln_set_")}
    rows = {r.c_name for r in switches_ref.ROWS} | set(switches_ref.NOT_SWITCHES)
    assert setters <= rows, setters - rows
    assert not any(name.startswith("svln_set_") for name in ENTRIES)


def test_plain_entries_still_refuse_a_forced_ids_key():
    for fn in (StreamVLNForCausalLM.generate_batch, StreamVLNForCausalLM.submit):
        assert "_reject_group_request" in inspect.getsource(fn), fn.__name__
    m = SimpleNamespace(_reject_group_request=StreamVLNForCausalLM._reject_group_request)
    with pytest.raises(NotImplementedError, match="forced_ids in a generate_batch request"):
        StreamVLNForCausalLM.generate_batch(m, [dict(forced_ids=[3, 4], inputs=None, images=None)])
    with pytest.raises(NotImplementedError, match="forced_ids in a submit request"):
        StreamVLNForCausalLM.submit(m, forced_ids=[3, 4])
    for name in ("submit_forced", "generate_batch_forced", "batch_forced_stats"):
        assert callable(getattr(StreamVLNForCausalLM, name))
    sig = inspect.signature(StreamVLNForCausalLM.submit_forced)
    assert list(sig.parameters)[:4] == ["self", "inputs", "images", "forced_ids"]


class _FakeLib:
    """the getters of a finished forced slot answering from fixed rows; records the order of the calls"""

    def __init__(self, F, n_ids=0):
        self.F, self.n_ids, self.calls = list(F), n_ids, []

    def svln_batch_forced(self, h, slot, lp, gid, glp, cap, n):
        self.calls.append("forced")
        for k in range(min(cap, len(self.F))):
            lp[k], gid[k], glp[k] = -1.5 - k, 900 + k, -0.25 * k
        n._obj.value = len(self.F)
        return 0

    def svln_batch_allowed_logprobs(self, h, slot, out, cap, nt, ni):
        self.calls.append("allowed")
        for k in range(min(cap, len(self.F) * self.n_ids)):
            out[k] = -float(k)
        nt._obj.value, ni._obj.value = len(self.F), self.n_ids
        return 0

    def svln_batch_result(self, h, slot, env, out, cap, n):
        self.calls.append("result")
        for k in range(min(cap, len(self.F))):
            out[k] = self.F[k]
        env._obj.value, n._obj.value = 2, len(self.F)
        return 0

    def svln_env_state(self, h, slot, ne, kl):
        ne._obj.value, kl._obj.value = 80, 77
        return 0


def _fake(F, allowed=None):
    m = SimpleNamespace(_lib=_FakeLib(F, len(allowed or ())), _h=None, allowed_token_ids=allowed, _slot=lambda e: e, _epoch={2: 4}, _auto_draft=True,
                        _last_out={}, _tickets={5: (2, torch.tensor([[1, 2, 3]]))})
    m._result = lambda env_id, tokens, inputs: StreamVLNForCausalLM._result(m, env_id, tokens, inputs)
    m._batch_result = lambda env_id, tokens, inputs, scores=None: StreamVLNForCausalLM._batch_result(m, env_id, tokens, inputs, scores)
    return m


def test_forced_ticket_result_shapes():
    F = [31, 7, 9, 12]
    m = _fake(F)
    ticket, res = StreamVLNForCausalLM._forced_batch_result(m, 5, np.asarray(F, np.int64))
    assert (ticket.env_id, ticket.slot, ticket.forced) == (2, 5, True) and not m._tickets
    assert res.sequences.dtype == torch.int64 and res.sequences.tolist() == [F]
    assert res.token_logprobs.dtype == torch.float32 and res.token_logprobs.tolist() == [[-1.5, -2.5, -3.5, -4.5]]
    assert res.greedy_ids.dtype == torch.int64 and res.greedy_ids.tolist() == [[900, 901, 902, 903]]
    assert res.greedy_logprobs.dtype == torch.float32 and res.greedy_logprobs.tolist() == [[0.0, -0.25, -0.5, -0.75]]
    assert isinstance(res.past_key_values, KVHandle) and (res.past_key_values.env_id, res.past_key_values.epoch, res.past_key_values.length) == (2, 4, 77)
    assert "allowed_logprobs" not in res and m._last_out[2].tolist() == F
    assert m._lib.calls == ["forced", "result"]                  # the getters come before svln_batch_result frees the slot
    m = _fake(F, allowed=(4, 7, 9, 12, 31))
    _, res = StreamVLNForCausalLM._forced_batch_result(m, 5, np.asarray(F, np.int64))
    assert tuple(res.allowed_logprobs.shape) == (1, 4, 5) and res.allowed_logprobs[0, 1, 2].item() == -7.0
    assert res.allowed_token_ids.tolist() == [4, 7, 9, 12, 31] and m._lib.calls == ["forced", "allowed", "result"]


def test_generate_batch_forced_submits_by_kind_and_returns_in_request_order():
    """on a fake library: the dry-run refusals come before the one grouped frame encode, the submits follow in request order by kind, and
    the results come back in request order whatever order the jobs finish in"""
    log = []

    class Lib:
        def svln_batch_submit_forced(self, h, env, ids, n, eos, n_eos, slot):
            log.append(("dry" if slot is None else "forced", env, [ids[k] for k in range(n)], [eos[k] for k in range(n_eos)]))
            if slot is not None:
                slot._obj.value = env + 1
            return 0

        def svln_batch_submit(self, h, env, max_new, eos, n_eos, slot):
            log.append(("plain", env, max_new, [eos[k] for k in range(n_eos)]))
            slot._obj.value = env + 1
            return 0

        def svln_encode_frames(self, h, pix, frames, on_dev):
            log.append(("encode", frames))
            return 0

        def svln_append_turn_at(self, h, env, ids, n, base, n_memory):
            log.append(("append", env, base))
            return 0
    # the job of the LAST request finishes first, the first request's waits an iteration
    steps = [([(SimpleNamespace(slot=3), GenerateOutput(sequences=torch.tensor([[8]])))], 2), ([], 2),
             ([(SimpleNamespace(slot=1), GenerateOutput(sequences=torch.tensor([[5, 6]]))), (SimpleNamespace(slot=2), GenerateOutput(sequences=torch.tensor([[7]])))], 0)]
    m = SimpleNamespace(_lib=Lib(), _h=None, _tickets={}, _forced_tickets={}, _sampling=None, max_frames=8, cfg=SimpleNamespace(max_positions=2048),
                        _slot=lambda e: e, _sync_call_config=lambda: None, _sync_sampling=lambda kw: None, _begin_turn=lambda e, past: log.append(("begin", e)),
                        _arm_batch_draft=lambda e, d: None, step_batch=lambda: steps.pop(0), cancel=lambda: None)
    m._forced_array = lambda f: StreamVLNForCausalLM._forced_array(m, f)
    m._forced_precheck = lambda e, f, eos: StreamVLNForCausalLM._forced_precheck(m, e, f, eos)
    m._parse_call = lambda inputs, images, kw: (torch.tensor([1, 2, 3]), torch.zeros((1, 3, 2, 2)), 1, 0, kw["env_id"], None, kw["max_new_tokens"], list(kw["eos_token_ids"]))
    outs = StreamVLNForCausalLM.generate_batch_forced(m, [dict(env_id=0, forced_ids=[5, 6]), dict(env_id=1, forced_ids=None), dict(env_id=2, forced_ids=[8], max_new_tokens=6)],
                                                      max_new_tokens=4, eos_token_ids=[9])
    assert [o.sequences.tolist() for o in outs] == [[[5, 6]], [[7]], [[8]]] and not steps
    assert log == [("dry", 0, [5, 6], [9]), ("dry", 2, [8], [9]), ("encode", 3), ("begin", 0), ("append", 0, 0), ("begin", 1), ("append", 1, 1), ("begin", 2),
                   ("append", 2, 2), ("forced", 0, [5, 6], [9]), ("plain", 1, 4, [9]), ("forced", 2, [8], [9])], log
    assert sorted(m._forced_tickets) == [1, 3] and sorted(m._tickets) == [1, 2, 3]       # (step_batch, faked here, is what pops them)
    m._tickets.clear()
    for bad, exc, match in (([], ValueError, "1..8"), ([dict(env_id=0)] * 2, ValueError, "duplicate"), ([dict(env_id=k) for k in range(9)], ValueError, "1..8"),
                            ([dict(env_id=0, forced_ids=[5] * 33)], ValueError, "1 .. 32"),
                            ([dict(env_id=0, forced_ids=[5], do_sample=True, num_return_sequences=2)], NotImplementedError, "num_return_sequences")):
        n_log = len(log)
        with pytest.raises(exc, match=match):
            StreamVLNForCausalLM.generate_batch_forced(m, bad, eos_token_ids=[9])
        assert len(log) == n_log                                 # refused before the engine is called
    m._tickets = {0: (0, None)}
    with pytest.raises(RuntimeError, match="idle scheduler"):
        StreamVLNForCausalLM.generate_batch_forced(m, [dict(env_id=0)], eos_token_ids=[9])


def test_agents_argument():
    assert _forced_map(None, 3) == {} and _forced_map([None, [4], None], 3) == {1: [4]} and _forced_map({2: [5], 0: None}, 3) == {2: [5]}
    with pytest.raises(ValueError, match="entries"):
        _forced_map([[4]], 3)
    with pytest.raises(ValueError, match="names agent"):
        _forced_map({3: [4]}, 3)
    for fn in (BatchedAgents.act, AsyncBatchedAgents.tick):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[-1] == "forced_ids" and sig.parameters["forced_ids"].default is None
    # no model turn is due: ValueError before anything is observed
    idle = lambda: SimpleNamespace(action_seq=[1, 2], step_id=5, pending_turn=False, model=None, observe=lambda rgb: pytest.fail("observed"))
    group = BatchedAgents([idle(), idle()])
    with pytest.raises(ValueError, match="no model turn"):
        group.act([None, None], forced_ids={1: [3]})
    group = AsyncBatchedAgents([idle(), idle()])
    with pytest.raises(ValueError, match="submits no model turn"):
        group.tick([None, None], forced_ids=[None, [3]])
    # forced_ids=None: the calls of before
    calls = []
    model = SimpleNamespace(generate_batch=lambda reqs, **kw: calls.append(("generate_batch", len(reqs), sorted(kw))) or [SimpleNamespace()] * len(reqs),
                            generate_batch_forced=lambda reqs, **kw: pytest.fail("generate_batch_forced without forced_ids"))
    due = lambda: SimpleNamespace(model=model, observe=lambda rgb: True, _build_request=lambda ins: dict(max_new_tokens=4, eos_token_ids=(9,)),
                                  _consume=lambda out: [1], finish_step=lambda: 1, action_seq=[])
    assert BatchedAgents([due(), due()]).act([None, None]) == [1, 1]
    assert calls == [("generate_batch", 2, ["eos_token_ids", "max_new_tokens"])]
