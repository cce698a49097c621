"""Host surface of the token log-probabilities (no GPU): the header declares the entries, the ctypes table binds them with the declared
argument counts and types, the library exports them, and the Python model / agent surface exists."""
import inspect
import os
import re
import subprocess

from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_set_token_scores": 2, "svln_get_token_scores": 4, "svln_batch_scores": 5, "svln_generate_batch_scores": 5,
           "svln_op_gemv_argmax_scores": 12, "svln_op_gemv_batched_argmax_scores": 15, "svln_op_gemm_argmax_scores": 13}


def _header():
    return open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()


def test_header_declares_the_entries():
    header = _header()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    assert set(re.findall(r"\bint (svln_[a-z0-9_]*scores)\s*\(", header)) == set(ENTRIES)


def test_signatures_match_the_header():
    c = _lib.C
    p, i, f, pi32, pf = c.c_void_p, c.c_int, c.c_float, c.POINTER(c.c_int32), c.POINTER(c.c_float)
    for name, n_args in ENTRIES.items():
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is c.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_set_token_scores"][1] == [p, i]
    assert _lib.SIGNATURES["svln_get_token_scores"][1] == [p, pf, i, pi32]
    assert _lib.SIGNATURES["svln_batch_scores"][1] == _lib.SIGNATURES["svln_generate_batch_scores"][1] == [p, i, pf, i, pi32]
    assert _lib.SIGNATURES["svln_op_gemv_argmax_scores"][1] == [p, i, p, p, i, p, i, i, p, f, pi32, pf]
    assert _lib.SIGNATURES["svln_op_gemv_batched_argmax_scores"][1] == [p, p, i, p, i, p, f, i, i, i, p, p, f, pi32, pf]
    assert _lib.SIGNATURES["svln_op_gemm_argmax_scores"][1] == [p, p, i, p, i, i, i, i, p, p, f, pi32, pf]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_surface():
    assert list(inspect.signature(StreamVLNForCausalLM.set_token_scores).parameters) == ["self", "enable"]
    doc = StreamVLNForCausalLM.set_token_scores.__doc__ + StreamVLNForCausalLM.generate.__doc__
    assert "output_scores" in doc and "token_logprobs" in doc
    for fn in (StreamVLNForCausalLM.generate, StreamVLNForCausalLM.generate_batch, StreamVLNForCausalLM.step_batch):
        assert "_token_scores" in inspect.getsource(fn), fn.__name__
    src = inspect.getsource(StreamingAgent)
    assert "last_token_logprobs" in src and "last_turn_logprob" in src


def test_agent_confidence_follows_the_output():
    """the agent keeps what the model's output carries, and None when it carries nothing (a model without scores, the CPU oracle)"""
    import torch

    class _Model:
        def reset_for_env(self, env):
            pass

    ag = StreamingAgent(_Model(), lambda *a: [1, 2, 3], preprocess=lambda rgb: rgb)
    assert ag.last_token_logprobs is None and ag.last_turn_logprob is None
    from streamvln_amd.model import GenerateOutput
    ag._pending = {}
    lp = torch.tensor([[-0.5, -0.25, -1.0]])
    ag._consume(GenerateOutput(sequences=torch.tensor([[4, 5, 6]]), past_key_values=None, token_logprobs=lp))
    assert ag.last_token_logprobs is lp and ag.last_turn_logprob == -1.75
    ag._consume(GenerateOutput(sequences=torch.tensor([[4]]), past_key_values=None))
    assert ag.last_token_logprobs is None and ag.last_turn_logprob is None
    ag.last_token_logprobs = lp
    ag.reset_memory()
    assert ag.last_token_logprobs is None
