"""Host surface of the folded candidates call (no GPU): the header declares the entries and documents them, the ctypes table binds them
with the signatures of the unfolded pair, the library exports them; no new svln_set_* switch; the names stay outside the patterns the
neighbouring host tests pin; generate's fold_candidates, its refusals and the result on a fake library; the agent's attribute."""
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
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_generate_candidates_folded": 10, "svln_turn_candidates_folded": 8, "svln_op_rope_kv_mirror": 7}


def _header():
    return open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()


def test_header_declares_and_documents_the_entries():
    header = _header()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    proto = lambda name: re.sub(r"\s+", " ", re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header).group(1))
    assert proto("svln_generate_candidates_folded") == proto("svln_generate_candidates")
    assert proto("svln_turn_candidates_folded") == proto("svln_turn_candidates")
    doc = header[header.index("FOLDED into the prefill pass"):header.index("int svln_generate_candidates_folded")]
    for words in ("mirror", "bit-equal", "svln_set_prefill_draft", "L % 64", "Tn + n_seq r", "row workspace"):
        assert words in doc, words
    # the name rules of the neighbouring host tests
    for name in ENTRIES:
        assert not any(k in name for k in ("group", "allowed", "pack", "entropy")), name
        assert not name.endswith(("candidates", "verify_multi", "scores", "forced", "target", "partials")) and not name.startswith("svln_set_"), name
        assert not name.startswith("svln_op_kv_p"), name


def test_no_new_switch():
    sets = set(re.findall(r"^int\s+(svln_set_[a-z0-9_]+)\s*\(", _header(), flags=re.M))
    assert not any("fold" in s or "mirror" in s or "candidate" in s for s in sets), sets
    assert not any(k.startswith("svln_set_") and ("fold" in k or "mirror" in k) for k in _lib.SIGNATURES)
    assert not any(n.startswith("set_") and ("fold" in n or "mirror" in n) for n in dir(StreamVLNForCausalLM))
    assert {k for k in _lib.SIGNATURES if k.startswith("svln_set_")} == sets


def test_signatures_match_the_header():
    p, i = C.c_void_p, C.c_int
    pi32 = C.POINTER(C.c_int32)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_generate_candidates_folded"][1] == _lib.SIGNATURES["svln_generate_candidates"][1]
    assert _lib.SIGNATURES["svln_turn_candidates_folded"][1] == _lib.SIGNATURES["svln_turn_candidates"][1]
    assert _lib.SIGNATURES["svln_op_rope_kv_mirror"][1] == [p, p, i, i, i, pi32, i]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_the_kernel_has_a_mirror_sibling_and_the_product_is_untouched():
    misc = open(os.path.join(ROOT, "streamvln_amd", "csrc", "misc.hip")).read()
    assert "template <typename T, bool MIRROR = false>" in misc and "rope_kv_kernel<T, true>" in misc and "if constexpr (MIRROR)" in misc
    kh = open(os.path.join(ROOT, "streamvln_amd", "csrc", "kernels.h")).read()
    for field in ("mirror_page", "mirror_dst", "n_mirror"):
        assert re.search(r"\b" + field + r"\b", kh[kh.index("struct RopeKvArgs {"):kh.index("void launch_rope_kv")]), field
    gemm = open(os.path.join(ROOT, "streamvln_amd", "csrc", "gemm.hip")).read()
    assert "mirror" not in gemm


# ------------------------------------------------------------------------------------------------------------ the Python surface
class _FakeLib:
    """the engine calls a candidates turn makes, on canned numbers; the folded entry scores 0.25 lower, so the result shows which ran"""

    def __init__(self):
        self.calls = []

    def _turn(self, who, shift, G, ids, lens, lp, gid, glp):
        self.calls.append((who, G))
        k = 0
        for g in range(G):
            for i in range(lens[g]):
                lp[k], gid[k], glp[k] = -(g + 1) - i / 10 - shift, 1000 + ids[k], -0.5 - g
                k += 1
        return 0

    def svln_turn_candidates(self, h, a, G, ids, lens, lp, gid, glp):
        return self._turn("unfolded", 0.0, G, ids, lens, lp, gid, glp)

    def svln_turn_candidates_folded(self, h, a, G, ids, lens, lp, gid, glp):
        return self._turn("folded", 0.25, G, ids, lens, lp, gid, glp)

    def svln_group_select(self, h, env, index, kv):
        self.calls.append(("select", index))
        kv._obj.value = 100 + index
        return 0


def _fake_model():
    m = StreamVLNForCausalLM.__new__(StreamVLNForCausalLM)
    m._lib, m._h = _FakeLib(), None
    m.curr_t, m._epoch, m._group_pending, m._env_slot = [0], [0], {}, {0: 0}
    m._slot = lambda env_id: 0
    m.generation_config = SimpleNamespace(pad_token_id=None, eos_token_id=2)
    m.allowed_token_ids = []
    m._sync_call_config = lambda: None
    m._sampling = None
    return m


def _call(m, **kw):
    pix = torch.zeros((1, 1, 3, 4, 4))
    return m.generate(inputs=torch.arange(6), images=pix, env_id=0, eos_token_ids=[2], **kw)


def test_generate_takes_fold_candidates_and_keeps_the_result_layout():
    sig = inspect.signature(StreamVLNForCausalLM.generate)
    assert sig.parameters["fold_candidates"].default is False and "fold_candidates" in StreamVLNForCausalLM.generate.__doc__
    sig = inspect.signature(StreamVLNForCausalLM._generate_candidates)
    assert list(sig.parameters)[:10] == ["self", "cands", "inputs", "ids", "pix", "V", "n_memory", "env_id", "past", "eos"]
    assert sig.parameters["fold"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["fold"].default is False
    cands = [[11, 12, 13, 14, 15], [21], [31, 32]]
    outs = {}
    for fold in (False, True):
        m = _fake_model()
        out = _call(m, candidate_ids=cands, fold_candidates=fold)
        assert m._lib.calls == [("folded" if fold else "unfolded", 3)]
        assert out.sequences.tolist() == [[11, 12, 13, 14, 15], [21, 2, 2, 2, 2], [31, 32, 2, 2, 2]] and out.sequence_lengths.tolist() == [5, 1, 2]
        assert tuple(out.token_logprobs.shape) == (3, 5) and out.past_key_values is None and out.greedy_ids.tolist()[1] == [1021, 2, 2, 2, 2]
        assert m._group_pending == {0: 3} and m.curr_t == [1]
        assert m.select_sequence(2, 0).get_seq_length() == 102
        outs[fold] = out
    assert np.allclose(outs[True].token_logprobs[0].numpy(), outs[False].token_logprobs[0].numpy() - 0.25)
    assert float(outs[True].token_logprobs[1, 1:].abs().sum()) == 0.0                  # pads stay 0
    # the default and a plain False take the unfolded entry
    m = _fake_model()
    _call(m, candidate_ids=cands)
    assert m._lib.calls == [("unfolded", 3)]


def test_python_level_refusals():
    m = _fake_model()
    C2 = [[1, 2], [3]]
    with pytest.raises(ValueError, match="fold_candidates without candidate_ids"):
        _call(m, fold_candidates=True)
    with pytest.raises(ValueError, match="fold_candidates without candidate_ids"):
        _call(m, fold_candidates=True, forced_ids=[1, 2])
    with pytest.raises(NotImplementedError, match="candidate_ids together with forced_ids"):
        _call(m, candidate_ids=C2, forced_ids=[1, 2], fold_candidates=True)
    with pytest.raises(ValueError, match="2 .. 8"):
        _call(m, candidate_ids=[[1, 2]], fold_candidates=True)
    assert m._lib.calls == [] and m._group_pending == {} and m.curr_t == [0]
    req = dict(inputs=torch.arange(6), images=torch.zeros((1, 1, 3, 4, 4)), env_id=0, fold_candidates=True)
    for fn, who in ((m.generate_batch, "generate_batch"), (m.generate_batch_forced, "generate_batch_forced")):
        with pytest.raises(NotImplementedError, match=f"fold_candidates in a {who} request"):
            fn([dict(req)])
    with pytest.raises(NotImplementedError, match="fold_candidates in a submit request"):
        m.submit(**req)
    with pytest.raises(NotImplementedError, match="fold_candidates in a submit_forced request"):
        m.submit_forced(forced_ids=[1], **req)
    assert m._lib.calls == []
    # a pending folded call blocks the env's next turn by name, as the unfolded one does
    _call(m, candidate_ids=C2, fold_candidates=True)
    with pytest.raises(RuntimeError, match="select_sequence"):
        _call(m, candidate_ids=C2, fold_candidates=True)


def test_agent_attribute():
    assert list(inspect.signature(StreamingAgent.act_candidates).parameters) == ["self", "rgb", "instruction", "candidate_ids", "select"]
    assert "fold_candidates" not in inspect.signature(StreamingAgent.__init__).parameters
    assert "self.fold_candidates = False" in inspect.getsource(StreamingAgent.__init__)
    src = inspect.getsource(StreamingAgent._turn_candidates)
    assert "fold_candidates" in src and "select_sequence" in src
    # _turn_candidates passes the attribute on, and leaves the key out when it is off
    for fold in (False, True):
        seen = {}

        def generate(**req):
            seen.update(req)
            raise KeyboardInterrupt                                   # (stop at the model call: the rest is the unfolded turn's)

        a = SimpleNamespace(fold_candidates=fold, model=SimpleNamespace(generate=generate),
                            _build_request=lambda instruction, env_id: dict(inputs=None, env_id=0, do_sample=True, temperature=0.5))
        with pytest.raises(KeyboardInterrupt):
            StreamingAgent._turn_candidates(a, "", [[1], [2]])
        assert seen.get("candidate_ids") == [[1], [2]] and ("fold_candidates" in seen) == fold and "do_sample" not in seen
