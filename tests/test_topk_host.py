"""Host-side checks of the top-k log-probabilities (svln_top_logprobs), no GPU: the C ABI entries exist in the header, the ctypes table
and the library's exports and agree; no new prototype is an `svln_set_*` (tests/switches_ref.py keeps a row for each of those, and this
switch is tied to svln_set_token_scores instead); GenerateOutput's defaults; the restatement's output shapes and padding."""
import os
import re
import subprocess

import torch

import topk_ref as R
from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import GenerateOutput, StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svln_top_logprobs", "svln_get_topk", "svln_batch_topk", "svln_generate_batch_topk", "svln_op_gemv_argmax_topk",
       "svln_op_gemv_batched_argmax_topk", "svln_op_gemm_argmax_topk")
# patterns other host tests own (they scan the header for names like these)
FORBIDDEN_END = ("scores", "forced", "target", "partials")
FORBIDDEN_IN = ("pack", "allowed", "group", "svln_op_subset", "svln_op_kv_p")


def _header():
    return open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()


def test_entries_in_header_ctypes_table_and_exports():
    declared = set(re.findall(r"\b(svln_[a-z0-9_]+)\s*\(", _header()))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
        assert not name.startswith("svln_set_"), name
        assert not name.endswith(FORBIDDEN_END) and not any(p in name for p in FORBIDDEN_IN), name
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)


def test_prototype_arity_matches_the_ctypes_table():
    text = _header()
    for name in NEW:
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name


def test_header_says_why_the_switch_is_not_a_set_prototype():
    text = " ".join(_header().split())
    assert "deliberately not svln_set_*" in text and "svln_top_logprobs" in text


def test_generate_output_defaults():
    out = GenerateOutput(sequences=torch.zeros((1, 2), dtype=torch.int64), past_key_values=None)
    assert out.top_token_ids is None and out.top_logprobs is None
    assert "top_token_ids" not in out and "top_logprobs" not in out
    out["top_logprobs"] = torch.zeros((1, 2, 3))
    assert tuple(out.top_logprobs.shape) == (1, 2, 3)
    try:
        out.no_such_entry
    except AttributeError:
        pass
    else:
        raise AssertionError("an unknown entry must stay an AttributeError")
    assert callable(StreamVLNForCausalLM.set_top_logprobs)
    src = open(os.path.join(ROOT, "streamvln_amd", "agent.py")).read()
    assert src.count("self.last_top_token_ids = None") == 1 and src.count("self.last_top_logprobs = None") == 1
    assert hasattr(StreamingAgent, "reset_memory")


def test_output_shapes_and_padding():
    """k entries whatever the row holds; padding is (-1, -inf) and only at the end"""
    case = next(c for c in R.rows_cases() if c.name == "ragged" and c.N == 3)
    for k in R.KS:
        got = case.restate(k=k)
        assert len(got["ids"]) == k == len(got["logprobs"])
        live = min(k, 3)
        assert all(i >= 0 for i in got["ids"][:live]) and got["ids"][live:] == [-1] * (k - live)
        assert all(v == float("-inf") for v in got["logprobs"][live:])
        assert all(len(p) == R.C for p in got["cand"])
    sub = next(c for c in R.subset_cases() if c.allowed is not None and len(c.allowed) == 3 and c.k == 8)
    got = sub.restate()
    assert sorted(got["ids"][:3]) == sorted(sub.allowed) and got["ids"][3:] == [-1] * 5
