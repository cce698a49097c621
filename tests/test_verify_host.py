"""Host surface of draft-verified greedy decode (no GPU): the header declares the three product entries and the two op entries, the ctypes
table binds them with the declared argument counts, the library exports them and the Python model surface has the operator methods."""
import inspect
import os
import re
import subprocess

from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_set_speculative": 2, "svln_set_draft": 4, "svln_draft_stats": 5, "svln_op_attention_verify": 8, "svln_op_verify_step": 12}


def _header():
    return open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()


def test_header_declares_the_entries():
    header = _header()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))


def test_signatures_match_the_header():
    for name, n_args in ENTRIES.items():
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == n_args, (name, len(args))
    declared = set(re.findall(r"\b(svln_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_surface():
    for name in ("set_speculative", "set_auto_draft", "draft_stats"):
        assert callable(getattr(StreamVLNForCausalLM, name)), name
    par = inspect.signature(StreamVLNForCausalLM.generate).parameters
    assert "draft_ids" in par and par["draft_ids"].default is None
    assert list(inspect.signature(StreamVLNForCausalLM.set_speculative).parameters) == ["self", "rows"]
    assert inspect.signature(StreamVLNForCausalLM.draft_stats).parameters["reset"].default is False
