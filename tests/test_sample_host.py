"""Host surface of temperature sampling (no GPU): the header declares the entries, the ctypes table binds them with the declared argument
counts and types, the library exports them, and the Python model / agent surface exists and refuses what it does not implement."""
import inspect
import os
import re
import subprocess

import pytest

from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_set_sampling": 4, "svln_op_gumbel": 7, "svln_op_gemv_argmax_sample": 16, "svln_op_gemv_batched_argmax_sample": 19,
           "svln_op_gemm_argmax_sample": 17}


def test_header_declares_the_entries():
    header = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    assert "int svln_set_sampling(svln_engine* h, int enable, float temperature, uint64_t seed);" in header


def test_signatures_match_the_header():
    c = _lib.C
    p, i, f, u64, pi32, pf = c.c_void_p, c.c_int, c.c_float, c.c_uint64, c.POINTER(c.c_int32), c.POINTER(c.c_float)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is c.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_set_sampling"][1] == [p, i, f, u64]
    assert _lib.SIGNATURES["svln_op_gumbel"][1] == [p, u64, i, i, i, i, pf]
    assert _lib.SIGNATURES["svln_op_gemv_argmax_sample"][1] == [p, i, p, p, i, p, i, i, p, f, f, u64, i, i, pi32, pf]
    assert _lib.SIGNATURES["svln_op_gemv_batched_argmax_sample"][1] == [p, p, i, p, i, p, f, i, i, i, p, p, f, f, u64, pi32, pi32, pi32, pf]
    assert _lib.SIGNATURES["svln_op_gemm_argmax_sample"][1] == [p, p, i, p, i, i, i, i, p, p, f, f, u64, pi32, pi32, pi32, pf]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_surface():
    assert list(inspect.signature(StreamVLNForCausalLM.set_sampling).parameters) == ["self", "temperature", "seed"]
    sig = inspect.signature(StreamVLNForCausalLM.set_sampling)
    assert sig.parameters["temperature"].default == 1.0 and sig.parameters["seed"].default == 0
    for fn in (StreamVLNForCausalLM.generate, StreamVLNForCausalLM.generate_batch, StreamVLNForCausalLM.submit):
        assert "_sync_sampling" in inspect.getsource(fn), fn.__name__
    sig = inspect.signature(StreamingAgent.__init__)
    assert sig.parameters["do_sample"].default is False and sig.parameters["temperature"].default is None


class _Model:
    def reset_for_env(self, env):
        pass


def test_agent_passes_the_sampling_kwargs_through():
    import torch
    kw = dict(preprocess=lambda rgb: torch.zeros(3, 4, 4), num_frames=8, num_history=2)
    ag = StreamingAgent(_Model(), lambda *a: [1, 2, 3], **kw)
    ag.observe(0)
    req = ag._build_request("")
    assert req["do_sample"] is False and "temperature" not in req            # the reference's greedy call, unchanged
    ag = StreamingAgent(_Model(), lambda *a: [1, 2, 3], do_sample=True, temperature=0.7, **kw)
    ag.observe(0)
    req = ag._build_request("")
    assert req["do_sample"] is True and req["temperature"] == 0.7
    ag = StreamingAgent(_Model(), lambda *a: [1, 2, 3], do_sample=True, **kw)
    ag.observe(0)
    assert "temperature" not in ag._build_request("")                        # the model's generation_config decides


def test_truncated_sampling_is_refused_by_key():
    """_parse_call refuses before anything else happens (no engine needed: the checks come first)"""
    parse = StreamVLNForCausalLM._parse_call
    for kw, key in ((dict(do_sample=True, top_k=5), "top_k"), (dict(do_sample=True, top_p=0.5), "top_p"), (dict(do_sample=True, num_beams=4), "num_beams"),
                    (dict(num_beams=4), "num_beams")):
        with pytest.raises(NotImplementedError, match=key):
            parse(None, None, None, kw)
