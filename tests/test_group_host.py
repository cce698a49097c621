"""Host surface of group sampling (no GPU): the header declares the entries, the ctypes table binds them with the declared argument counts and
types, the library exports them; the Python surface (generate's num_return_sequences, select_sequence, the output keys); padding and
sequence_lengths of a group result on a fake library."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from streamvln_amd import _lib
from streamvln_amd.model import KVHandle, StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_generate_group": 9, "svln_turn_group": 6, "svln_group_select": 4, "svln_group_logprobs": 5, "svln_group_dist": 6,
           "svln_get_hidden_group": 5, "svln_op_kv_page_copy": 4, "svln_op_kv_pool_read": 6}


def test_header_declares_the_entries():
    header = open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    assert set(re.findall(r"\bint (svln_[a-z0-9_]*group[a-z0-9_]*|svln_op_kv_p[a-z0-9_]*)\s*\(", header)) == set(ENTRIES)
    # the name rules of the neighbouring host tests: theirs are the entries that end in "scores" / contain "allowed"
    assert not any(name.endswith("scores") or "allowed" in name for name in ENTRIES)


def test_signatures_match_the_header():
    p, i = C.c_void_p, C.c_int
    pi32, pi64, pf = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_generate_group"][1] == [p, i, i, i, pi64, i, pi64, i, pi32]
    assert _lib.SIGNATURES["svln_turn_group"][1] == [p, C.POINTER(_lib.SvlnTurnArgs), i, pi64, i, pi32]
    assert _lib.SIGNATURES["svln_group_select"][1] == [p, i, i, pi32]
    assert _lib.SIGNATURES["svln_group_logprobs"][1] == _lib.SIGNATURES["svln_get_hidden_group"][1] == [p, i, pf, i, pi32]
    assert _lib.SIGNATURES["svln_group_dist"][1] == [p, i, pf, i, pi32, pi32]
    assert _lib.SIGNATURES["svln_op_kv_page_copy"][1] == [p, i, pi32, i]
    assert _lib.SIGNATURES["svln_op_kv_pool_read"][1] == [p, i, i, i, pf, pf]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_surface():
    sig = inspect.signature(StreamVLNForCausalLM.select_sequence)
    assert list(sig.parameters) == ["self", "index", "env_id"] and sig.parameters["env_id"].default == 0
    assert sig.return_annotation in (KVHandle, "KVHandle")
    assert "num_return_sequences" in StreamVLNForCausalLM.generate.__doc__
    for key in ("sequences", "sequence_lengths", "token_logprobs", "allowed_logprobs", "allowed_token_ids", "past_key_values"):
        assert key in inspect.getsource(StreamVLNForCausalLM._group_result), key
    for fn in (StreamVLNForCausalLM.generate_batch, StreamVLNForCausalLM.submit):
        assert "_reject_group_request" in inspect.getsource(fn), fn.__name__
    for fn in (StreamVLNForCausalLM.reset, StreamVLNForCausalLM.reset_for_env):
        assert "_group_pending" in inspect.getsource(fn), fn.__name__
    nrs = StreamVLNForCausalLM._num_return_sequences
    assert nrs(dict(do_sample=True, num_return_sequences=4)) == 4 and nrs(dict(do_sample=True)) == 1 and nrs(dict(do_sample=True, num_return_sequences=1)) == 1
    assert nrs(dict(do_sample=False, num_return_sequences=99)) == 1 and nrs(dict(num_return_sequences=99)) == 1      # a greedy call leaves the key unread
    for bad in (9, 0, -1):
        with pytest.raises(ValueError, match="num_return_sequences"):
            nrs(dict(do_sample=True, num_return_sequences=bad))
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        StreamVLNForCausalLM._reject_group_request(dict(num_return_sequences=2), "submit")
    StreamVLNForCausalLM._reject_group_request(dict(num_return_sequences=1), "submit")
    StreamVLNForCausalLM._reject_group_request(dict(), "submit")


class _FakeLib:
    """the three calls a group result makes, answering from fixed rows"""

    def __init__(self, lens, n_ids):
        self.lens, self.n_ids, self.selected = lens, n_ids, []

    def svln_group_logprobs(self, h, index, out, cap, n):
        for k in range(min(self.lens[index], cap)):
            out[k] = -(index + 1) - 0.25 * k
        n._obj.value = self.lens[index]
        return 0

    def svln_group_dist(self, h, index, out, cap_rows, n_rows, n_cols):
        for k in range(min(self.lens[index], cap_rows) * self.n_ids):
            out[k] = -(100 * index + k)
        n_rows._obj.value, n_cols._obj.value = self.lens[index], self.n_ids
        return 0

    def svln_group_select(self, h, env, index, kv):
        self.selected.append((env, index))
        kv._obj.value = 40 + index
        return 0


def _fake(lens, scores, allowed, pad=None):
    return SimpleNamespace(_lib=_FakeLib(lens, len(allowed or ())), _h=None, _token_scores=scores, allowed_token_ids=allowed,
                           generation_config=SimpleNamespace(eos_token_id=[7, 9], **({} if pad is None else {"pad_token_id": pad})),
                           _group_pending={3: len(lens)}, _slot=lambda e: 0, _epoch={3: 5})


def test_group_result_pads_and_reports_lengths():
    lens = [3, 1, 4]
    out = np.arange(30, dtype=np.int64).reshape(3, 10) + 100
    m = _fake(lens, False, None)
    res = StreamVLNForCausalLM._group_result(m, out, np.asarray(lens, dtype=np.int32), [7, 9])
    assert res.sequences.dtype == torch.int64 and res.sequences.tolist() == [[100, 101, 102, 7], [110, 7, 7, 7], [120, 121, 122, 123]]
    assert res.sequence_lengths.dtype == torch.int64 and res.sequence_lengths.tolist() == lens
    assert res.past_key_values is None and "token_logprobs" not in res and "allowed_logprobs" not in res
    # pad_token_id wins over the first EOS id; no EOS at all pads with 0
    assert StreamVLNForCausalLM._group_result(_fake(lens, False, None, pad=55), out, lens, [7])["sequences"][1].tolist() == [110, 55, 55, 55]
    assert StreamVLNForCausalLM._group_result(m, out, lens, [])["sequences"][1].tolist() == [110, 0, 0, 0]
    # scores: padded with 0, so that a row sum is the joint log-probability of the sequence
    res = StreamVLNForCausalLM._group_result(_fake(lens, True, None), out, lens, [7, 9])
    lp = res.token_logprobs
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (3, 4) and "allowed_logprobs" not in res
    assert lp[1].tolist() == [-2.0, 0.0, 0.0, 0.0] and lp[0].tolist() == [-1.0, -1.25, -1.5, 0.0]
    assert float(lp[2].sum()) == pytest.approx(-3.0 * 4 - 0.25 * 6)
    # ... and the rows over the allowed set
    res = StreamVLNForCausalLM._group_result(_fake(lens, True, (4, 7, 9)), out, lens, [7, 9])
    alp = res.allowed_logprobs
    assert tuple(alp.shape) == (3, 4, 3) and res.allowed_token_ids.tolist() == [4, 7, 9]
    assert alp[1, 0].tolist() == [-100.0, -101.0, -102.0] and float(alp[1, 1:].abs().sum()) == 0.0 and alp[2, 3].tolist() == [-209.0, -210.0, -211.0]
    # an allowed list without the scores carries neither key
    assert "allowed_logprobs" not in StreamVLNForCausalLM._group_result(_fake(lens, False, (4, 7, 9)), out, lens, [7, 9])


def test_select_sequence_returns_the_envs_handle_and_clears_the_pending_group():
    m = _fake([2, 2], False, None)
    with pytest.raises(RuntimeError, match="no group turn is pending"):
        StreamVLNForCausalLM.select_sequence(m, 0, env_id=1)
    kv = StreamVLNForCausalLM.select_sequence(m, 1, env_id=3)
    assert isinstance(kv, KVHandle) and (kv.env_id, kv.epoch, kv.length) == (3, 5, 41)
    assert m._lib.selected == [(0, 1)] and m._group_pending == {}
