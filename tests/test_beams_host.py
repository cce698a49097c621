"""Host-side agreement for the beam ops: the header, the ctypes table and the library's exports name the same two test entries with the
same number of arguments, and the beam work adds no engine switch (no svln_set_* name)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import beam_ref as br
from streamvln_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
NAMES = ("svln_op_beam_select", "svln_op_beam_page_gather", "svln_generate_beams", "svln_turn_beams", "svln_beam_trace")


def _declared_args(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, re.S)
    assert m, f"{name} is not declared in the header"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_ctypes_and_exports_agree():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        args = _declared_args(name)
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib._I and len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert args[0] == "svln_engine* h" and argtypes[0] is _lib._P
        for decl, ty in zip(args[1:], argtypes[1:]):
            want = (_lib._PF if "float*" in decl else _lib._PI32 if "int32_t*" in decl else _lib._PI64 if "int64_t*" in decl
                    else C.POINTER(_lib.SvlnTurnArgs) if "svln_turn_args*" in decl else _lib._I)
            assert ty is want or ty == want, (name, decl, ty)
        assert re.search(r" T " + name + r"\b", nm), f"{name} is not exported"
        assert getattr(lib, name).argtypes == argtypes


def test_the_beam_ops_add_no_engine_switch():
    setters = set(re.findall(r"\b(svln_set_[a-z0-9_]+)\s*\(", HEADER))
    assert setters and not [s for s in setters if "beam" in s]
    assert all(not n.startswith("svln_set_") for n in NAMES)


def test_record_layout_matches_the_kernel_header():
    kh = open(os.path.join(ROOT, "streamvln_amd", "csrc", "kernels.h")).read()
    m = re.search(r"BEAM_MAX_W = (\d+), BEAM_CP_MAX = (\d+), BEAM_REC = 4 \+ 3 \* BEAM_MAX_W", kh)
    assert m and int(m.group(1)) == br.MAXW and br.REC == 4 + 3 * br.MAXW


def test_python_refusals_fire_without_a_gpu():
    from streamvln_amd.model import StreamVLNForCausalLM as M
    assert M._beam_request(None, None, None, {}) == 0 and M._beam_request(4, None, None, {"do_sample": False}) == 4
    for bad in (0, 9):
        with pytest.raises(ValueError, match="beam_width"):
            M._beam_request(bad, None, None, {})
    for args, needle in (((2, [1, 2], None, {}), "forced_ids"), ((2, None, [[1], [2]], {}), "candidate_ids"),
                         ((2, None, None, {"do_sample": True}), "do_sample"), ((2, None, None, {"num_return_sequences": 2}), "num_return_sequences")):
        with pytest.raises(NotImplementedError, match="beam_width together with " + needle):
            M._beam_request(*args)
    for who in ("generate_batch", "submit"):
        with pytest.raises(NotImplementedError, match=f"beam_width in a {who} request"):
            M._reject_group_request({"beam_width": 2}, who)
    M._reject_group_request({}, "submit")
    src = open(os.path.join(ROOT, "streamvln_amd", "model.py")).read()
    assert "beam_width in a submit_forced request" in src
