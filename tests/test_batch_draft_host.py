"""Host surface of drafts in the scheduler's prefill pass (no GPU): the header declares the two entries, the ctypes table binds them with the
declared argument counts, the library exports them and the Python model surface has the operator methods."""
import inspect
import os
import re
import subprocess

from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_set_batch_draft": 2, "svln_batch_draft_stats": 7}


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
    assert _lib.SIGNATURES["svln_set_batch_draft"][1] == [_lib.C.c_void_p, _lib.C.c_int]
    p64 = _lib.C.POINTER(_lib.C.c_int64)
    assert _lib.SIGNATURES["svln_batch_draft_stats"][1] == [_lib.C.c_void_p, p64, p64, p64, p64, p64, _lib.C.c_int]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_surface():
    for name in ("set_batch_draft", "batch_draft_stats"):
        assert callable(getattr(StreamVLNForCausalLM, name, None)), name
    assert list(inspect.signature(StreamVLNForCausalLM.set_batch_draft).parameters) == ["self", "enable"]
    assert inspect.signature(StreamVLNForCausalLM.batch_draft_stats).parameters["reset"].default is False
    src = inspect.getsource(StreamVLNForCausalLM.submit) + inspect.getsource(StreamVLNForCausalLM.generate_batch)
    assert src.count("draft_ids") >= 2 and src.count("_arm_batch_draft") == 2
