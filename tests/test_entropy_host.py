"""Host-side checks of the token entropies (svln_token_entropy; no GPU): the header, the ctypes table and the library's exports agree on
the new names and arities; no new prototype is a svln_set_* (the switch-pair table of tests/switches_ref.py lists those) or matches a name
pattern another host test claims; the header says why; GenerateOutput and the agent default to None."""
import os
import re
import subprocess
from types import SimpleNamespace

from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import GenerateOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
NEW = {"svln_token_entropy": 2, "svln_get_token_entropy": 4, "svln_batch_entropy": 5, "svln_generate_batch_entropy": 5,
       "svln_op_gemv_argmax_entropy": 25, "svln_op_gemv_batched_argmax_entropy": 26, "svln_op_gemm_argmax_entropy": 26,
       "svln_op_entropy_merge": 9}


def _prototype(name):
    m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\);", HEADER, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_ctypes_and_exports_agree():
    _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    for name, arity in NEW.items():
        args = _prototype(name)
        assert len(args) == arity, (name, len(args))
        assert args[0] == "svln_engine* h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.C.c_int and len(argtypes) == arity, (name, len(argtypes))
        assert name in exported, name
    every = set(re.findall(r"\b(svln_[a-z0-9_]*entropy[a-z0-9_]*)\s*\(", HEADER))
    assert every == set(NEW), every ^ set(NEW)


def test_names_fall_into_no_claimed_pattern():
    for name in NEW:
        assert not name.startswith("svln_set_"), name
        assert not name.endswith(("scores", "forced", "target", "partials", "candidates", "verify_multi")), name
        assert not any(s in name for s in ("pack", "allowed", "group", "svln_op_subset", "svln_op_kv_p")), name


def test_header_says_why_the_switch_is_no_set_function():
    doc = HEADER[:HEADER.index("int svln_token_entropy(")]
    doc = doc[doc.rindex("/*"):]
    assert "deliberately not svln_set_*" in doc and "svln_set_token_scores" in doc and "switch-pair" in doc
    for other in ("svln_top_logprobs", "svln_sampling_truncation", "svln_batch_submit_forced", "svln_set_allowed_tokens"):
        assert other in doc, other


def test_generate_output_and_agent_defaults():
    out = GenerateOutput(sequences=None, past_key_values=None)
    assert out.token_entropies is None and "token_entropies" not in out
    out["token_entropies"] = 1
    assert out.token_entropies == 1
    assert "token_entropies" in GenerateOutput._OPTIONAL
    ag = StreamingAgent.__new__(StreamingAgent)
    ag.model, ag.env_id = SimpleNamespace(reset_for_env=lambda env: None), 0
    ag.last_token_entropies, ag.last_turn_entropy = 1, 1.0
    StreamingAgent.reset_memory(ag)
    assert ag.last_token_entropies is None and ag.last_turn_entropy is None
