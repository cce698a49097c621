"""Host surface of the multi-draft turn (no GPU): the header declares and documents the four entries, the ctypes table binds them, the
library exports them; none is a switch and modes.h holds no rule for them; generate's draft_set, its conflicts and the result on a fake
library; the agent's draft history."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from streamvln_amd import _lib
from streamvln_amd.agent import StreamingAgent, update_draft_history
from streamvln_amd.model import GenerateOutput, StreamVLNForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svln_generate_drafts": 13, "svln_turn_drafts": 11, "svln_drafts_stats": 2, "svln_op_draft_select": 2}


def _header():
    return open(os.path.join(ROOT, "include", "streamvln_hip.h")).read()


def test_header_declares_and_documents_the_entries():
    header = _header()
    for name, n_args in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert m.group(1).count(",") + 1 == n_args, (name, m.group(1))
    doc = header[header.index("MULTI-DRAFT turns"):header.index("int svln_generate_drafts")]
    for words in ("IGNORED", "never a refusal", "launch for launch", "tie goes to the lowest g", "never fed", "svln_set_sampling",
                  "svln_set_decode_persistent", "svln_top_logprobs", "svln_token_entropy", "svln_set_allowed_tokens", "n_drafts outside 0 .. 8",
                  "outside 0 .. 32", "svln_generate_candidates_folded", "-1 when no pass ran"):
        assert words in doc, words
    fields = re.search(r"typedef struct svln_draft_select_op \{(.*?)\} svln_draft_select_op;", header, flags=re.S).group(1)
    names = re.findall(r"[\*\s,](\w+)(?=[;,])", fields)
    assert names == [n for n, _ in _lib.SvlnDraftSelectOp._fields_], names


def test_no_switch_and_no_mode_rule():
    sets = set(re.findall(r"^int\s+(svln_set_[a-z0-9_]+)\s*\(", _header(), flags=re.M))
    assert {k for k in _lib.SIGNATURES if k.startswith("svln_set_")} == sets
    assert not any(s.endswith("drafts") or "draft_select" in s or "multi" in s for s in sets), sets
    assert not any(n.startswith("set_") and ("drafts" in n or "draft_set" in n) for n in dir(StreamVLNForCausalLM))
    modes = open(os.path.join(ROOT, "streamvln_amd", "csrc", "modes.h")).read()
    assert "GENERATE_DRAFTS" not in modes and "svln_generate_drafts" not in modes and "svln_turn_drafts" not in modes


def test_signatures_match_the_header():
    p, i = C.c_void_p, C.c_int
    p64, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    for name, n_args in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, (name, len(args))
    assert _lib.SIGNATURES["svln_generate_drafts"][1] == [p, i, i, p64, p32, i, p64, i, p64, i, p32, p32, p32]
    assert _lib.SIGNATURES["svln_turn_drafts"][1] == [p, C.POINTER(_lib.SvlnTurnArgs), i, p64, p32, p64, i, p32, p32, p32, p32]
    assert _lib.SIGNATURES["svln_drafts_stats"][1] == [p, p64]
    assert _lib.SIGNATURES["svln_op_draft_select"][1] == [p, C.POINTER(_lib.SvlnDraftSelectOp)]
    assert C.sizeof(_lib.SvlnDraftSelectOp) == 12 * C.sizeof(C.c_void_p) + 10 * 4


def test_library_exports_the_entries():
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (svln_[a-z0-9_]+)", nm))
    assert set(ENTRIES) <= exported, set(ENTRIES) - exported
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_the_select_kernel_sits_beside_the_verify_step():
    misc = open(os.path.join(ROOT, "streamvln_amd", "csrc", "misc.hip")).read()
    assert misc.index("void verify_step_kernel(") < misc.index("void draft_select_kernel(") < misc.index("slow-memory token pruning")
    assert "__launch_bounds__(256) void draft_select_kernel" in misc and "asm" not in misc[misc.index("void draft_select_kernel("):misc.index("slow-memory token pruning")]


# ------------------------------------------------------------------------------------------------------------ the Python surface
class _FakeLib:
    """the engine calls of a turn on canned numbers: the plain entry emits 7, 8, 2; the multi-draft one the same, and reports a winner"""

    def __init__(self):
        self.calls = []

    def _emit(self, out, n_out, kv):
        for k, t in enumerate((7, 8, 2)):
            out[k] = t
        n_out._obj.value, kv._obj.value = 3, 40
        return 0

    def svln_turn(self, h, a, out, cap, n_out, kv):
        self.calls.append(("plain",))
        return self._emit(out, n_out, kv)

    def svln_turn_drafts(self, h, a, G, ids, lens, out, cap, n_out, kv, win, ptok):
        L = [lens[g] for g in range(G)]
        self.calls.append(("drafts", G, L, [ids[k] for k in range(sum(L))]))
        win._obj.value, ptok._obj.value = (G - 1, 2) if sum(L) else (-1, 0)
        return self._emit(out, n_out, kv)

    def svln_set_draft(self, h, slot, ids, n):
        self.calls.append(("set_draft", n))
        return 0


def _fake_model():
    m = StreamVLNForCausalLM.__new__(StreamVLNForCausalLM)
    m._lib, m._h = _FakeLib(), None
    m.curr_t, m._epoch, m._group_pending, m._env_slot = [0], [0], {}, {0: 0}
    m._slot = lambda env_id: 0
    m.cfg = SimpleNamespace(max_positions=64)
    m.generation_config = SimpleNamespace(pad_token_id=None, eos_token_id=2)
    m.allowed_token_ids = []
    m._sync_call_config = lambda: None
    m._sampling = None
    m._auto_draft, m._last_out = True, {0: torch.tensor([9, 9])}
    m._token_scores, m.top_logprobs_k, m._token_entropy = False, 0, False
    m._turn_bufs = {}
    return m


def _call(m, **kw):
    pix = torch.zeros((1, 1, 3, 4, 4))
    return m.generate(inputs=torch.arange(6), images=pix, env_id=0, eos_token_ids=[2], max_new_tokens=8, **kw)


def test_generate_takes_draft_set():
    sig = inspect.signature(StreamVLNForCausalLM.generate)
    assert sig.parameters["draft_set"].default is None and "draft_set" in StreamVLNForCausalLM.generate.__doc__
    m = _fake_model()
    out = _call(m, draft_set=[[7, 8, 2], [], torch.tensor([5])])
    # the auto draft is not armed for a multi-draft turn; the flat ids and the lengths reach the engine as given
    assert m._lib.calls == [("drafts", 3, [3, 0, 1], [7, 8, 2, 5])]
    assert out.sequences.tolist() == [[7, 8, 2]] and out.draft_index == 2 and out.draft_tokens == 2
    assert out.past_key_values.get_seq_length() == 40
    out = _call(m, draft_set=[])
    assert m._lib.calls[-1] == ("drafts", 0, [], []) and out.draft_index == -1 and out.draft_tokens == 0
    out = _call(m)
    assert m._lib.calls[-2:] == [("set_draft", 3), ("plain",)] and "draft_index" not in out and out.draft_index is None


def test_kwarg_conflicts_raise_by_name():
    m = _fake_model()
    for name, v in (("draft_ids", [1]), ("forced_ids", [1, 2]), ("candidate_ids", [[1], [2]]), ("beam_width", 2)):
        with pytest.raises(NotImplementedError, match=f"draft_set together with {name}"):
            _call(m, draft_set=[[1]], **{name: v})
    with pytest.raises(NotImplementedError, match="draft_set together with num_return_sequences > 1"):
        _call(m, draft_set=[[1]], do_sample=True, num_return_sequences=2)
    with pytest.raises(ValueError, match="holds 9 drafts"):
        _call(m, draft_set=[[1]] * 9)
    with pytest.raises(ValueError, match=r"draft_set\[1\] holds 33 ids"):
        _call(m, draft_set=[[1], [1] * 33])
    assert m._lib.calls == [] and m.curr_t == [0]
    req = dict(inputs=torch.arange(6), images=torch.zeros((1, 1, 3, 4, 4)), env_id=0, draft_set=[[1]])
    for fn, who in ((m.generate_batch, "generate_batch"), (m.generate_batch_forced, "generate_batch_forced")):
        with pytest.raises(NotImplementedError, match=f"draft_set in a {who} request"):
            fn([dict(req)])
    with pytest.raises(NotImplementedError, match="draft_set in a submit request"):
        m.submit(**req)
    with pytest.raises(NotImplementedError, match="draft_set in a submit_forced request"):
        m.submit_forced(forced_ids=[1], **req)
    assert m._lib.calls == []


def test_generate_output_defaults():
    out = GenerateOutput(sequences=torch.zeros((1, 1)))
    assert out.draft_index is None and out.draft_tokens is None and "draft_index" not in out
    assert out.top_token_ids is None and out.token_entropies is None
    with pytest.raises(AttributeError):
        out.no_such_entry
    out["draft_index"] = -1
    assert out.draft_index == -1
    assert inspect.signature(StreamVLNForCausalLM.drafts_stats).parameters.keys() == {"self"}


def test_agent_history_function():
    h = []
    h = update_draft_history(h, [1, 2, 3])
    h = update_draft_history(h, [4, 5])
    assert h == [[4, 5], [1, 2, 3]]
    h2 = update_draft_history(h, [1, 2, 3])                   # a repeated output moves to the front, once
    assert h2 == [[1, 2, 3], [4, 5]] and h == [[4, 5], [1, 2, 3]]      # (pure: the argument is unchanged)
    assert update_draft_history(h2, []) == h2
    for k in range(10):
        h2 = update_draft_history(h2, [100 + k])
    assert len(h2) == 8 and h2[0] == [109] and h2[-1] == [102]
    assert update_draft_history([[1]], torch.tensor([2, 3]).tolist(), cap=1) == [[2, 3]]


def test_agent_passes_its_history_and_is_off_by_default():
    assert "draft_history" not in inspect.signature(StreamingAgent.__init__).parameters
    assert "self.draft_history = 0" in inspect.getsource(StreamingAgent.__init__)
    assert "self.turn_history" in inspect.getsource(StreamingAgent.reset_memory)
    seen = []

    def generate(**req):
        seen.append(req)
        return GenerateOutput(sequences=torch.tensor([[10 + len(seen), 2]]))

    for G in (0, 2):
        seen.clear()
        a = SimpleNamespace(draft_history=G, turn_history=[[5], [6], [7]], model=SimpleNamespace(generate=generate),
                            _build_request=lambda instruction, env_id: dict(inputs=None, env_id=0), _consume=lambda out: out)
        StreamingAgent._turn(a, "")
        StreamingAgent._turn(a, "", forced_ids=[3])
        if G == 0:
            assert all("draft_set" not in r for r in seen) and a.turn_history == [[5], [6], [7]]
        else:
            assert seen[0]["draft_set"] == [[5], [6]] and "draft_set" not in seen[1] and seen[1]["forced_ids"] == [3]
            assert a.turn_history == [[12, 2], [11, 2], [5], [6], [7]]
