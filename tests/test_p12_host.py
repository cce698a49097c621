"""Host surface of the packed-decode feature (no GPU): the header declares the entries, the ctypes table binds them with the declared
argument counts and types, the library exports them, and the Python methods exist."""
import ctypes as C
import inspect
import os
import re
import subprocess

from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_set_packed_decode": 2, "svln_packed_stats": 5, "svln_op_pack_rows": 8, "svln_op_unpack_rows": 8, "svln_op_gemv_packed": 15}


def test_header_declares_the_entries():
    header = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    assert set(re.findall(r"\bint (svln_[a-z0-9_]*pack[a-z0-9_]*)\s*\(", header)) == set(ENTRIES)


def test_signatures_match_the_header():
    p, i, f, i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
    pi32, pi64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_set_packed_decode"][1] == [p, i]
    assert _lib.SIGNATURES["svln_packed_stats"][1] == [p, pi64, pi64, pi64, pi64]
    assert _lib.SIGNATURES["svln_op_pack_rows"][1] == [p, p, i, i64, i, p, p, pi64]
    assert _lib.SIGNATURES["svln_op_unpack_rows"][1] == [p, p, p, p, i, i64, i, p]
    assert _lib.SIGNATURES["svln_op_gemv_packed"][1] == [p, p, p] + _lib.SIGNATURES["svln_op_gemv"][1][1:]
    assert _lib.SIGNATURES["svln_op_gemv"][1][-1] == pi32 and f in _lib.SIGNATURES["svln_op_gemv_packed"][1]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_surface():
    assert list(inspect.signature(StreamVLNForCausalLM.set_packed_decode).parameters) == ["self", "enable"]
    assert "bit-identical" in StreamVLNForCausalLM.set_packed_decode.__doc__
    assert list(inspect.signature(StreamVLNForCausalLM.packed_stats).parameters) == ["self"]
    assert "svln_packed_stats" in inspect.getsource(StreamVLNForCausalLM.packed_stats)
