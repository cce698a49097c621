"""Host-side checks of truncated sampling (svln_sampling_truncation), no GPU: the two C ABI entries exist in the header, the ctypes table
and the library's exports and agree; neither is an `svln_set_*` (tests/switches_ref.py keeps a row for each of those, and truncation is
an attribute of svln_set_sampling); set_sampling_truncation, model.sampling_truncation and the Python-side refusals; the per-call
`top_k=` / `top_p=` keys of generate stay refused by name."""
import inspect
import os
import re
import subprocess

import pytest

import switches_ref
from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svln_sampling_truncation", "svln_op_truncate")


def _header():
    return open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()


def test_entries_in_header_ctypes_table_and_exports():
    declared = set(re.findall(r"\b(svln_[a-z0-9_]+)\s*\(", _header()))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
        assert not name.startswith("svln_set_"), name
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    p, i, f, u64 = _lib._P, _lib._I, _lib._F, _lib._U64
    pf, pi32 = _lib._PF, _lib._PI32
    assert _lib.SIGNATURES["svln_sampling_truncation"][1] == [p, i, f]
    assert _lib.SIGNATURES["svln_op_truncate"][1] == [p, pf, pi32, i, i, i, pi32, pi32, u64, f, i, f, pf, pi32, pf, pf, pf, pi32, pf]


def test_prototype_arity_matches_the_ctypes_table():
    text = _header()
    for name in NEW:
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"int svln_sampling_truncation\(svln_engine\* h, int32_t top_k, float top_p\);", text)


def test_no_new_set_prototype_and_the_header_says_why():
    text = " ".join(_header().split())
    assert "attribute of svln_set_sampling" in text and text.count("deliberately not svln_set_*") >= 2
    src = inspect.getsource(switches_ref)
    assert "truncation" not in src                      # the switch-pair table has no row for it
    sets = set(re.findall(r"\bint (svln_set_[a-z0-9_]+)\s*\(", _header()))
    assert not any("trunc" in s or "top_k" in s or "top_p" in s for s in sets)


def test_python_surface():
    # set_sampling keeps its parameters (tests/test_sample_host.py pins them): the truncation has a setter of its own
    assert list(inspect.signature(StreamVLNForCausalLM.set_sampling).parameters) == ["self", "temperature", "seed"]
    sig = inspect.signature(StreamVLNForCausalLM.set_sampling_truncation)
    assert list(sig.parameters) == ["self", "top_k", "top_p"]
    assert sig.parameters["top_k"].default is None and sig.parameters["top_p"].default is None
    assert "self.sampling_truncation = None" in inspect.getsource(StreamVLNForCausalLM.__init__)
    # every switch-on from Python -- set_sampling and the automatic flip of do_sample=True -- applies the held pair after the switch
    assert "_switch_sampling_on" in inspect.getsource(StreamVLNForCausalLM._sync_sampling)
    assert "_switch_sampling_on" in inspect.getsource(StreamVLNForCausalLM.set_sampling)
    src = inspect.getsource(StreamVLNForCausalLM._switch_sampling_on)
    assert src.index("svln_set_sampling") < src.index("svln_sampling_truncation")
    chk = StreamVLNForCausalLM._check_truncation
    assert chk(None, None) is None and chk(0, 1.0) is None and chk(0, None) is None
    assert chk(8, None) == (8, 1.0) and chk(4, 0.9) == (4, 0.9) and chk(1, 2.0 ** -20) == (1, 2.0 ** -20)
    for bad in ((9, None), (-1, None), (4, 0.0), (4, 1.5), (4, float("nan")), (4, -0.1)):
        with pytest.raises(ValueError):
            chk(*bad)
    with pytest.raises(ValueError, match="top_k"):
        chk(None, 0.9)
    with pytest.raises(ValueError, match="top_k"):
        chk(0, 0.5)


def test_the_kwargs_stay_refused_by_key():
    parse = StreamVLNForCausalLM._parse_call
    for kw, key in ((dict(do_sample=True, top_k=5), "top_k"), (dict(do_sample=True, top_p=0.5), "top_p")):
        with pytest.raises(NotImplementedError, match=key) as ei:
            parse(None, None, None, dict(kw))
        assert "set_sampling_truncation" in str(ei.value)
