"""Host surface of candidate scoring (no GPU): the header declares the entries, the ctypes table binds them with the declared argument
counts and types, the library exports them; no new svln_set_* switch exists and the names stay outside the patterns the neighbouring host
tests pin; the Python surface (generate's candidate_ids, the refusals that need no engine, shapes and padding of a result on a fake
library, the agent's arguments); and the fixtures alone leave at most 10 % of their rows under the top-2 gap the GPU test exempts."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from scenarios import SCENARIOS, SEED
from streamvln_amd import _lib
from streamvln_amd import weights as W
from streamvln_amd.agent import StreamingAgent
from streamvln_amd.model import StreamVLNForCausalLM
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_generate_candidates": 10, "svln_turn_candidates": 8, "svln_op_attention_verify_multi": 12}


def _header():
    return open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()


def test_header_declares_the_entries():
    header = _header()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    assert set(re.findall(r"\bint (svln_[a-z0-9_]*(?:candidates|verify_multi))\s*\(", header)) == set(ENTRIES)
    # the name rules of the neighbouring host tests
    for name in ENTRIES:
        assert not any(k in name for k in ("group", "allowed", "pack")), name
        assert not name.endswith(("forced", "target", "partials", "scores")) and not name.startswith("svln_set_"), name


def test_no_new_switch():
    # the switches of the parent commit: candidate scoring is a call, not a mode
    sets = set(re.findall(r"\bint (svln_set_[a-z0-9_]+)\s*\(", _header()))
    assert not any("candidate" in s or "verify_multi" in s for s in sets)
    assert not any(k.startswith("svln_set_") and ("candidate" in k or "multi" in k) for k in _lib.SIGNATURES)
    assert not any("candidate" in n and n.startswith("set_") for n in dir(StreamVLNForCausalLM))


def test_signatures_match_the_header():
    p, i = C.c_void_p, C.c_int
    pi32, pi64, pf = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_generate_candidates"][1] == [p, i, i, pi64, pi32, pi64, i, pf, pi64, pf]
    assert _lib.SIGNATURES["svln_turn_candidates"][1] == [p, C.POINTER(_lib.SvlnTurnArgs), i, pi64, pi32, pf, pi64, pf]
    assert _lib.SIGNATURES["svln_op_attention_verify_multi"][1] == [p, i, i, p, i, i, pi32, p, pi32, i, p, i]


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


# ------------------------------------------------------------------------------------------------------------ the Python surface
def test_candidate_arrays():
    ca = StreamVLNForCausalLM._candidate_arrays
    flat, lens = ca([[1, 2, 3], [4], torch.tensor([5, 6])])
    assert flat.dtype == np.int64 and flat.tolist() == [1, 2, 3, 4, 5, 6] and lens.dtype == np.int32 and lens.tolist() == [3, 1, 2]
    flat, lens = ca(torch.tensor([[1, 2], [3, 4]]))
    assert flat.tolist() == [1, 2, 3, 4] and lens.tolist() == [2, 2]
    for bad, match in (([[1, 2]], "2 .. 8"), ([[1]] * 9, "2 .. 8"), ([[1], []], "1 .. 32"), ([[1], list(range(33))], "1 .. 32")):
        with pytest.raises(ValueError, match=match):
            ca(bad)
    with pytest.raises(ValueError, match="list of id sequences"):
        ca(torch.tensor([1, 2, 3]))


class _FakeLib:
    """the two engine calls a candidates turn makes, on canned numbers: score of id t at position i of sequence g = -(g + 1) - i / 10"""

    def __init__(self, n_allowed=0):
        self.calls, self.n_allowed = [], n_allowed

    def svln_turn_candidates(self, h, a, G, ids, lens, lp, gid, glp):
        self.calls.append(("turn", G))
        k = 0
        for g in range(G):
            for i in range(lens[g]):
                lp[k], gid[k], glp[k] = -(g + 1) - i / 10, 1000 + ids[k], -0.5 - g
                k += 1
        return 0

    def svln_group_dist(self, h, g, buf, cap_rows, nr, nc):
        n = self.lens[g]
        for q in range(n * self.n_allowed):
            buf[q] = -float(g) - q
        nr._obj.value, nc._obj.value = n, self.n_allowed
        return 0

    def svln_group_select(self, h, env, index, kv):
        self.calls.append(("select", index))
        kv._obj.value = 100 + index
        return 0


def _fake_model(n_allowed=0):
    m = StreamVLNForCausalLM.__new__(StreamVLNForCausalLM)
    m._lib, m._h = _FakeLib(n_allowed), None
    m.curr_t, m._epoch, m._group_pending, m._env_slot = [0], [0], {}, {0: 0}
    m._slot = lambda env_id: 0
    m.generation_config = SimpleNamespace(pad_token_id=None, eos_token_id=2)
    m.allowed_token_ids = list(range(50, 50 + n_allowed))
    return m


def test_result_shapes_and_padding():
    m = _fake_model()
    cands = [[11, 12, 13, 14, 15], [21], [31, 32]]
    pix, ids = torch.zeros((1, 3, 4, 4)), torch.arange(6)
    out = m._generate_candidates(cands, ids, ids, pix, 1, 0, 0, None, [2])
    assert out.sequences.tolist() == [[11, 12, 13, 14, 15], [21, 2, 2, 2, 2], [31, 32, 2, 2, 2]] and out.sequences.dtype == torch.int64
    assert out.sequence_lengths.tolist() == [5, 1, 2] and out.past_key_values is None
    assert tuple(out.token_logprobs.shape) == (3, 5) and out.token_logprobs.dtype == torch.float32
    assert np.allclose(out.token_logprobs[0].numpy(), [-1, -1.1, -1.2, -1.3, -1.4]) and out.token_logprobs[1].tolist()[1:] == [0.0] * 4
    assert abs(float(out.token_logprobs[2].sum()) - (-3 - 3.1)) < 1e-6                       # a row sum is the joint log-probability
    assert out.greedy_ids.tolist()[1] == [1021, 2, 2, 2, 2] and out.greedy_ids.dtype == torch.int64
    assert out.greedy_logprobs[2].tolist() == [-2.5, -2.5, 0.0, 0.0, 0.0]
    assert "allowed_logprobs" not in out
    assert m._group_pending == {0: 3} and m.curr_t == [1]
    kv = m.select_sequence(2, 0)
    assert kv.get_seq_length() == 102 and m._group_pending == {} and m._lib.calls == [("turn", 3), ("select", 2)]
    # with an allowed list
    m = _fake_model(n_allowed=4)
    m._lib.lens = [5, 1, 2]
    out = m._generate_candidates(cands, ids, ids, pix, 1, 0, 0, None, [2])
    assert tuple(out.allowed_logprobs.shape) == (3, 5, 4) and out.allowed_token_ids.tolist() == [50, 51, 52, 53]
    assert out.allowed_logprobs[1, 0].tolist() == [-1.0, -2.0, -3.0, -4.0] and float(out.allowed_logprobs[1, 1:].abs().sum()) == 0.0


def _call(m, **kw):
    pix = torch.zeros((1, 1, 3, 4, 4))
    return m.generate(inputs=torch.arange(6), images=pix, env_id=0, eos_token_ids=[2], **kw)


def test_python_level_refusals():
    m = _fake_model()
    m._sync_call_config = lambda: None
    m._sampling = None
    C2 = [[1, 2], [3]]
    with pytest.raises(NotImplementedError, match="candidate_ids together with forced_ids"):
        _call(m, candidate_ids=C2, forced_ids=[1, 2])
    with pytest.raises(NotImplementedError, match="candidate_ids with num_return_sequences"):
        _call(m, candidate_ids=C2, do_sample=True, num_return_sequences=2)
    with pytest.raises(ValueError, match="2 .. 8"):
        _call(m, candidate_ids=[[1, 2]])
    assert m._lib.calls == [] and m._group_pending == {} and m.curr_t == [0]
    for fn, who in ((m.generate_batch, "generate_batch"), (m.generate_batch_forced, "generate_batch_forced")):
        with pytest.raises(NotImplementedError, match=f"candidate_ids in a {who} request"):
            fn([dict(inputs=torch.arange(6), images=torch.zeros((1, 1, 3, 4, 4)), env_id=0, candidate_ids=C2)])
    with pytest.raises(NotImplementedError, match="candidate_ids in a submit request"):
        m.submit(inputs=torch.arange(6), images=torch.zeros((1, 1, 3, 4, 4)), env_id=0, candidate_ids=C2)
    with pytest.raises(NotImplementedError, match="candidate_ids in a submit_forced request"):
        m.submit_forced(inputs=torch.arange(6), images=torch.zeros((1, 1, 3, 4, 4)), env_id=0, forced_ids=[1], candidate_ids=C2)
    # a pending candidates call blocks the env's next turn by name, as a group turn does
    _call(m, candidate_ids=C2)
    with pytest.raises(RuntimeError, match="select_sequence"):
        _call(m, candidate_ids=C2)


def test_agent_arguments():
    sig = inspect.signature(StreamingAgent.act_candidates)
    assert list(sig.parameters) == ["self", "rgb", "instruction", "candidate_ids", "select"] and sig.parameters["select"].default is None
    assert list(inspect.signature(StreamingAgent.act).parameters) == ["self", "rgb", "instruction", "forced_ids"]      # (act keeps its list)
    a = SimpleNamespace(action_seq=[1, 2], step_id=5, observe=lambda rgb: pytest.fail("observed"))
    with pytest.raises(ValueError, match="no model turn"):
        StreamingAgent.act_candidates(a, None, "", candidate_ids=[[1], [2]])
    a.action_seq = []
    with pytest.raises(ValueError, match="select=2"):
        StreamingAgent.act_candidates(a, None, "", candidate_ids=[[1], [2]], select=2)
    src = inspect.getsource(StreamingAgent._turn_candidates)
    assert "select_sequence" in src and "last_candidate_logprobs" in src and "argmax" in src
    assert "candidate_ids" in StreamVLNForCausalLM.generate.__doc__


# ------------------------------------------------------------------------------------------------------------ the fixtures' margins
@pytest.mark.parametrize("name", ["tiny_episode", "true1_episode"])
def test_fixture_rows_leave_at_most_a_tenth_under_the_exempted_gap(name):
    """the GPU test exempts greedy_ids where the float64 top-2 gap of a row is within 2 gamma_K max_n sum_k |w_nk h_k| + 2e-5; on the
    fixtures' own final-norm rows that share must stay <= 10 %"""
    sc, g = SCENARIOS[name], load_golden(name)
    Wd = torch.as_tensor(np.asarray(W.synth_state_dict(sc["cfg"], SEED)["lm_head.weight"], dtype=np.float64))
    gamma = Wd.shape[1] * 2.0 ** -24
    rows = exempt = 0
    for t in range(int(g["n_turns"])):
        for h in g[f"t{t}_hidden"]:
            h = torch.from_numpy(np.asarray(h, dtype=np.float64))
            top = torch.topk(Wd @ h, 2).values
            rows += 1
            exempt += float(top[0] - top[1]) <= 2 * gamma * float((Wd.abs() @ h.abs()).max()) + 2e-5
    assert rows > 0 and exempt <= 0.10 * rows, (name, exempt, rows)
