"""Host surface of the allowed-token decode (no GPU): the header declares the entries, the ctypes table binds them with the declared argument
counts and types, the library exports them, the Python signatures, what set_allowed_tokens sends to the engine (sorting, de-duplication,
add_eos), and the agent's last_allowed_logprobs."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import torch

from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import GenerateOutput, StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_set_allowed_tokens": 3, "svln_get_allowed_logprobs": 5, "svln_batch_allowed_logprobs": 6,
           "svln_generate_batch_allowed_logprobs": 6, "svln_op_subset_argmax": 21}


def test_header_declares_the_entries():
    header = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    assert set(re.findall(r"\bint (svln_[a-z0-9_]*allowed[a-z0-9_]*|svln_op_subset[a-z0-9_]*)\s*\(", header)) == set(ENTRIES)
    assert not any(name.endswith("scores") for name in ENTRIES)


def test_signatures_match_the_header():
    p, i, f, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
    pi32, pi64, pf = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_set_allowed_tokens"][1] == [p, pi64, i]
    assert _lib.SIGNATURES["svln_get_allowed_logprobs"][1] == [p, pf, i, pi32, pi32]
    assert _lib.SIGNATURES["svln_batch_allowed_logprobs"][1] == _lib.SIGNATURES["svln_generate_batch_allowed_logprobs"][1] == [p, i, pf, i, pi32, pi32]
    assert _lib.SIGNATURES["svln_op_subset_argmax"][1] == [p, p, i, p, i, i, i, i, pi64, i, p, p, f, f, u64, pi32, pi32, pi32, pf, pf, pf]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_surface():
    assert list(inspect.signature(StreamVLNForCausalLM.set_allowed_tokens).parameters) == ["self", "ids", "add_eos"]
    assert inspect.signature(StreamVLNForCausalLM.set_allowed_tokens).parameters["add_eos"].default is True
    doc = StreamVLNForCausalLM.set_allowed_tokens.__doc__
    assert "allowed_logprobs" in doc and "allowed_token_ids" in doc and "add_eos" in doc
    for fn in (StreamVLNForCausalLM.generate, StreamVLNForCausalLM.generate_batch, StreamVLNForCausalLM.step_batch):
        assert "allowed" in inspect.getsource(fn), fn.__name__
    assert "last_allowed_logprobs" in inspect.getsource(StreamingAgent)


class _FakeLib:
    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def svln_set_allowed_tokens(self, h, ids, n):
        self.calls.append(None if n == 0 else [ids[k] for k in range(n)])
        return self.rc

    def svln_last_error(self):
        return b"refused"


def _fake(eos, vocab=4096, rc=0):
    return SimpleNamespace(_lib=_FakeLib(rc), _h=None, allowed_token_ids=None, cfg=SimpleNamespace(vocab=vocab),
                           generation_config=SimpleNamespace(eos_token_id=eos))


def test_set_allowed_tokens_sorts_dedups_and_adds_eos():
    m = _fake([151645, 7])
    StreamVLNForCausalLM.set_allowed_tokens(m, [9, 3, 9, 5])
    assert m._lib.calls[-1] == [3, 5, 7, 9] and m.allowed_token_ids == (3, 5, 7, 9)          # the EOS id outside the vocabulary can never be emitted
    StreamVLNForCausalLM.set_allowed_tokens(m, torch.tensor([9, 3]), add_eos=False)
    assert m._lib.calls[-1] == [3, 9] and m.allowed_token_ids == (3, 9)
    StreamVLNForCausalLM.set_allowed_tokens(m, None)
    assert m._lib.calls[-1] is None and m.allowed_token_ids is None
    StreamVLNForCausalLM.set_allowed_tokens(m, [4])
    StreamVLNForCausalLM.set_allowed_tokens(m, [])
    assert m._lib.calls[-1] is None and m.allowed_token_ids is None
    m = _fake(5)                                              # a single EOS id, not a list
    StreamVLNForCausalLM.set_allowed_tokens(m, (8,))
    assert m.allowed_token_ids == (5, 8)


def test_a_refused_list_leaves_the_model_state_alone(monkeypatch):
    import streamvln_amd.model as M
    m = _fake([7], rc=-1)
    m.allowed_token_ids = (1, 2)

    def check(rc):
        if rc != 0:
            raise _lib.SvlnError("refused")
    monkeypatch.setattr(M, "_check", check)
    try:
        StreamVLNForCausalLM.set_allowed_tokens(m, [99999])
        raise AssertionError("not refused")
    except _lib.SvlnError:
        pass
    assert m.allowed_token_ids == (1, 2)


def test_agent_keeps_and_clears_the_distribution():
    class _Model:
        def reset_for_env(self, env):
            pass

    ag = StreamingAgent(_Model(), lambda *a: [1, 2, 3], preprocess=lambda rgb: rgb)
    assert ag.last_allowed_logprobs is None
    ag._pending = {}
    alp = torch.zeros((1, 3, 4))
    ag._consume(GenerateOutput(sequences=torch.tensor([[4, 5, 6]]), past_key_values=None, token_logprobs=torch.zeros((1, 3)), allowed_logprobs=alp,
                               allowed_token_ids=torch.tensor([4, 5, 6, 7])))
    assert ag.last_allowed_logprobs is alp
    ag._consume(GenerateOutput(sequences=torch.tensor([[4]]), past_key_values=None))
    assert ag.last_allowed_logprobs is None
    ag.last_allowed_logprobs = alp
    ag.reset_memory()
    assert ag.last_allowed_logprobs is None
