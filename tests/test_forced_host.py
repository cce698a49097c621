"""Host surface of forced turns (no GPU): the header declares the entries, the ctypes table binds them with the declared argument counts
and types, the library exports them; generate(forced_ids=...) on a fake library -- the output keys, shapes and dtypes -- and the
NotImplementedError of generate_batch / submit requests; StreamingAgent.act's argument."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import KVHandle, StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_generate_forced": 10, "svln_turn_forced": 8, "svln_op_gemv_batched_target": 14, "svln_op_gemm_target": 14,
           "svln_op_read_argmax_partials": 6}


def test_header_declares_the_entries():
    header = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    assert set(re.findall(r"\bint (svln_[a-z0-9_]*(?:forced|target|partials))\s*\(", header)) == set(ENTRIES)
    for word in ("EPI_TARGET", "1 <= n <= 32", "svln_get_top2 is refused", "a repetition penalty != 1", "never fed"):
        assert word in header, word


def test_signatures_match_the_header():
    p, i, f = C.c_void_p, C.c_int, C.c_float
    pi32, pi64, pf = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_generate_forced"][1] == [p, i, pi64, i, pi64, i, pf, pi64, pf, pi32]
    assert _lib.SIGNATURES["svln_turn_forced"][1] == [p, C.POINTER(_lib.SvlnTurnArgs), pi64, i, pf, pi64, pf, pi32]
    assert _lib.SIGNATURES["svln_op_gemv_batched_target"][1] == [p, p, i, p, i, i, i, i, pi32, f, pi32, pf, pf, pf]
    assert _lib.SIGNATURES["svln_op_gemm_target"][1] == [p, p, i, p, i, i, i, i, pi32, f, pi32, pf, pf, pf]
    assert _lib.SIGNATURES["svln_op_read_argmax_partials"][1] == [p, i, i, pf, pi32, pf]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


class _FakeLib:
    """svln_turn_forced and svln_get_allowed_logprobs answering from fixed rows; records what it was given"""

    def __init__(self, n_ids=0):
        self.n_ids, self.calls = n_ids, []

    def svln_turn_forced(self, h, a, ids, n, lp, gid, glp, kv):
        a = a._obj
        self.calls.append(dict(ids=[ids[k] for k in range(n)], n=n, max_new=a.max_new_tokens, n_eos=a.n_eos, new_window=a.new_window,
                               new_episode=a.new_episode, n_prompt=a.n_ids))
        for k in range(n):
            lp[k], gid[k], glp[k] = -1.5 - k, 900 + k, -0.25 * k
        kv._obj.value = 77
        return 0

    def svln_get_allowed_logprobs(self, h, out, cap, nt, ni):
        n = self.calls[-1]["n"]
        for k in range(min(cap, n * self.n_ids)):
            out[k] = -float(k)
        nt._obj.value, ni._obj.value = n, self.n_ids
        return 0


def _fake(allowed=None, curr_t=0):
    return SimpleNamespace(_lib=_FakeLib(len(allowed or ())), _h=None, allowed_token_ids=allowed, _slot=lambda e: e, _epoch={2: 4}, curr_t=[0, 0, curr_t],
                           _auto_draft=True, _last_out={})


def test_generate_forced_output_shapes():
    F = [31, 7, 9, 12]
    pix = torch.zeros((1, 3, 4, 4))
    m = _fake()
    res = StreamVLNForCausalLM._generate_forced(m, torch.tensor(F), torch.tensor([[1, 2, 3]]), torch.tensor([1, 2, 3]), pix, 1, 0, 2, None, [7, 9])
    assert res.sequences.dtype == torch.int64 and res.sequences.tolist() == [F]
    assert res.token_logprobs.dtype == torch.float32 and res.token_logprobs.tolist() == [[-1.5, -2.5, -3.5, -4.5]]
    assert res.greedy_ids.dtype == torch.int64 and res.greedy_ids.tolist() == [[900, 901, 902, 903]]
    assert res.greedy_logprobs.dtype == torch.float32 and res.greedy_logprobs.tolist() == [[0.0, -0.25, -0.5, -0.75]]
    assert isinstance(res.past_key_values, KVHandle) and (res.past_key_values.env_id, res.past_key_values.epoch, res.past_key_values.length) == (2, 4, 77)
    assert "allowed_logprobs" not in res and "allowed_token_ids" not in res
    call = m._lib.calls[0]
    assert call["ids"] == F and call["n_eos"] == 2 and call["n_prompt"] == 3 and (call["new_window"], call["new_episode"]) == (1, 1)
    assert m.curr_t[2] == 1 and m._last_out[2].tolist() == F          # the next turn's automatic draft is what the env went on with
    # an allowed list: the rows come with the result, whatever set_token_scores says
    m = _fake(allowed=(4, 7, 9, 12, 31), curr_t=3)
    res = StreamVLNForCausalLM._generate_forced(m, F, torch.tensor([[1, 2, 3]]), torch.tensor([1, 2, 3]), pix, 1, 0, 2, KVHandle(2, 4, 10), [7])
    assert tuple(res.allowed_logprobs.shape) == (1, 4, 5) and res.allowed_logprobs.dtype == torch.float32 and res.allowed_logprobs[0, 1, 2].item() == -7.0
    assert res.allowed_token_ids.tolist() == [4, 7, 9, 12, 31] and (m._lib.calls[0]["new_window"], m._lib.calls[0]["new_episode"]) == (0, 0)
    # n outside 1 .. 32 and a foreign KV handle are refused before the engine is called
    for bad in ([], list(range(33))):
        with pytest.raises(ValueError, match="1 .. 32"):
            StreamVLNForCausalLM._generate_forced(_fake(), bad, None, torch.tensor([1, 2]), pix, 1, 0, 2, None, [7])
    with pytest.raises(ValueError, match="past_key_values"):
        StreamVLNForCausalLM._generate_forced(_fake(), F, None, torch.tensor([1, 2]), pix, 1, 0, 2, KVHandle(2, 3, 10), [7])


def test_python_surface():
    sig = inspect.signature(StreamVLNForCausalLM.generate)
    assert "forced_ids" in sig.parameters and sig.parameters["forced_ids"].default is None
    assert "forced_ids" in StreamVLNForCausalLM.generate.__doc__ and "max_new_tokens" in StreamVLNForCausalLM.generate.__doc__
    for fn in (StreamVLNForCausalLM.generate_batch, StreamVLNForCausalLM.submit):
        assert "_reject_group_request" in inspect.getsource(fn), fn.__name__
    for who in ("generate_batch", "submit"):
        with pytest.raises(NotImplementedError, match="forced_ids"):
            StreamVLNForCausalLM._reject_group_request(dict(forced_ids=[1, 2]), who)
    StreamVLNForCausalLM._reject_group_request(dict(forced_ids=None), "submit")
    sig = inspect.signature(StreamingAgent.act)
    assert list(sig.parameters) == ["self", "rgb", "instruction", "forced_ids"] and sig.parameters["forced_ids"].default is None
    assert "last_greedy_ids" in inspect.getsource(StreamingAgent.reset_memory)


def test_batch_requests_with_forced_ids_raise_before_anything_is_parsed():
    m = SimpleNamespace(_reject_group_request=StreamVLNForCausalLM._reject_group_request)
    with pytest.raises(NotImplementedError, match="forced_ids in a generate_batch request"):
        StreamVLNForCausalLM.generate_batch(m, [dict(forced_ids=[3, 4], inputs=None, images=None)])
    with pytest.raises(NotImplementedError, match="forced_ids in a submit request"):
        StreamVLNForCausalLM.submit(m, forced_ids=[3, 4])


def test_agent_argument_raises_when_no_model_turn_runs():
    a = SimpleNamespace(action_seq=[1, 2], step_id=5, observe=lambda rgb: pytest.fail("observed"))
    with pytest.raises(ValueError, match="no model turn"):
        StreamingAgent.act(a, None, "", forced_ids=[3])
