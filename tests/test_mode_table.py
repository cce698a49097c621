"""The engine's mode rule table (csrc/modes.h, asked through svln_mode_refusal / svln_mode_rule: no GPU) against

  the record   tests/golden/mode_refusals.json: what the engine answered, on an MI355X, to every setter, weight write and turn form under
               every reachable mode state BEFORE the table existed (tests/mode_refusals_ref.py, tools/record_mode_refusals.py).  Every row:
               same outcome, identical message.  Every rule of the table is the first violated rule of some row, or is named with its
               reason in DESIGN.md ("Rules the record cannot reach")
  the matrix   tests/switches_ref.py: every REFUSED pair is refused in both orders with a message that names the switch that is on,
               every COMPOSES / NO_EFFECT pair is accepted in both orders
  itself       a message that names a mode's C function names the one of the violated bit
"""
import ctypes as C
import json
import os
import re

import pytest

import mode_refusals_ref as R
import switches_ref as S
from streamvln_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "mode_refusals.json")

# the observer's mode names -> the setter's callers (None: the setter reads no rule)
SETTER = {"decode_graph": None, "packed": None, "persistent": "set_decode_persistent", "fp8_decode": "set_fp8_decode",
          "mxfp4_decode": "set_mxfp4_decode", "mxfp4_batched": "set_mxfp4_batched", "fp8_gemm": "set_fp8_gemm", "fp8_scaled": "set_fp8_scaled_mfma",
          "speculative": "set_speculative", "prefill_draft": "set_prefill_draft", "batch_draft": "set_batch_draft", "scores": "set_token_scores",
          "topk": "top_logprobs", "entropy": "token_entropy", "sampling": "set_sampling", "truncation": "sampling_truncation",
          "allowed": "set_allowed_tokens", "penalty": "set_repetition_penalty"}
# the C function a message names for a violated bit (jobs: none)
BIT_FN = {"persistent": "svln_set_decode_persistent", "fp8_decode": "svln_set_fp8_decode", "mxfp4_decode": "svln_set_mxfp4_decode",
          "mxfp4_batched": "svln_set_mxfp4_batched", "fp8_gemm": "svln_set_fp8_gemm", "speculative": "svln_set_speculative",
          "prefill_draft": "svln_set_prefill_draft", "batch_draft": "svln_set_batch_draft", "scores": "svln_set_token_scores",
          "topk": "svln_top_logprobs", "entropy": "svln_token_entropy", "sampling": "svln_set_sampling", "truncation": "svln_sampling_truncation",
          "penalty": "svln_set_repetition_penalty", "group": "svln_group_select", "jobs": None}
# switches_ref's row names -> the observer's mode names (rows without an entry have no rule in the table)
ROW_MODE = {"decode_graph": "decode_graph", "packed_decode": "packed", "fp8_decode": "fp8_decode", "mxfp4_decode": "mxfp4_decode",
            "mxfp4_batched": "mxfp4_batched", "fp8_gemm": "fp8_gemm", "fp8_scaled_mfma": "fp8_scaled", "decode_persistent": "persistent",
            "token_scores": "scores", "sampling": "sampling", "allowed_tokens": "allowed", "repetition_penalty": "penalty",
            "speculative": "speculative", "prefill_draft": "prefill_draft", "batch_draft": "batch_draft"}


@pytest.fixture(scope="module")
def record():
    return json.load(open(RECORD))


@pytest.fixture(scope="module")
def rules():
    return _lib.mode_rules()


def steps_of(attempt, state):
    """an attempt of the record -> the table queries the engine makes for it, in order: [(caller, who, no_change)]"""
    if ":" in attempt:
        mode, d = attempt.split(":")
        base = SETTER[mode]
        if base is None:
            return []
        name = base if base in _lib.MODE_CALLERS else f"{base}:{d}"
        return [(name, None, (d == "on") == (mode in state))]
    if attempt == R.WEIGHT_WRITE:
        return [("weight_write", attempt, False)]
    form = attempt[len("svln_"):]
    if form.startswith("generate_candidates"):           # their own rules, then the forced rules under their own name
        return [("generate_candidates", attempt, False), ("generate_forced", attempt, False)]
    return [(form, None, False)]


def table_answer(attempt, state):
    bits = [b for b in state if b in _lib.MODE_BITS]
    for caller, who, same in steps_of(attempt, state):
        msg = _lib.mode_refusal(caller, on=bits, no_change=same, who=who, group_env=R.BUSY_ENV)
        if msg is not None:
            return msg
    return R.ACCEPTED


def first_violated(rules, attempt, state):
    """index of the rule that refuses the attempt (the lookup of modes.h restated over the walked table), or None"""
    for caller, _, same in steps_of(attempt, state):
        ci = _lib.MODE_CALLERS.index(caller)
        for i, r in enumerate(rules):
            if r["caller"] == ci and (r["on_no_change"] or not same) and (r["bit"] in state) != r["must_be_on"]:
                return i
    return None


def test_record_is_complete(record):
    assert record["attempts"] == list(R.ATTEMPTS)
    assert record["messages"][0] == R.ACCEPTED
    states = [tuple(s) for s in record["states"]]
    assert len(set(states)) == len(states) and set(states) <= set(R.states())
    assert () in states and (R.JOBS,) in states and ("sampling", R.GROUP) in states
    assert all((m,) in states for m in R.MODES if m not in R.PREREQ)
    # one row per state and attempt, in order
    assert [r[:2] for r in record["rows"]] == [[s, a] for s in range(len(states)) for a in range(len(R.ATTEMPTS))]
    assert os.path.getsize(RECORD) < 1 << 20


def test_table_answers_what_the_engine_answered(record):
    diff = []
    for s, a, m in record["rows"]:
        state, attempt, want = record["states"][s], record["attempts"][a], record["messages"][m]
        got = table_answer(attempt, state)
        if got != want:
            diff.append((state, attempt, want, got))
    assert not diff, f"{len(diff)} of {len(record['rows'])} rows differ; first: under {diff[0][0]} {diff[0][1]} -> recorded {diff[0][2]!r}, table {diff[0][3]!r}"


def unreachable_in_design():
    """DESIGN.md, "Rules the record cannot reach": lines "- `caller` / `bit`: reason" -> {(caller, bit): reason}"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text.split("Rules the record cannot reach", 1)[1].split("\n#", 1)[0]
    return {(c, b): why.strip() for c, b, why in re.findall(r"^- `([\w:]+)` / `(\w+)`:(.+)$", sec, flags=re.M)}


def test_every_rule_is_reached_by_the_record_or_listed(record, rules):
    hit = set()
    for s, a, m in record["rows"]:
        state, attempt = record["states"][s], record["attempts"][a]
        i = first_violated(rules, attempt, state)
        assert (i is None) == (m == 0), (state, attempt)
        if i is not None:
            r = rules[i]
            who = r["caller_name"] if ":" in attempt else attempt
            assert record["messages"][m] == who + r["text"].replace("{env}", str(R.BUSY_ENV)), (state, attempt, i)
            hit.add(i)
    missed = {(_lib.MODE_CALLERS[r["caller"]], r["bit"]) for i, r in enumerate(rules) if i not in hit}
    listed = unreachable_in_design()
    assert missed == set(listed), f"unreached and not listed: {sorted(missed - set(listed))}; listed but reached: {sorted(set(listed) - missed)}"
    assert all(listed.values()) and len(listed) <= 3          # each with its reason; not a way to thin the record


def test_callers_and_names(rules):
    seen = {}
    for r in rules:
        seen.setdefault(r["caller"], r["caller_name"])
    assert sorted(seen) == list(range(len(_lib.MODE_CALLERS)))            # every caller has rules
    for ci, name in seen.items():
        base = _lib.MODE_CALLERS[ci].split(":")[0]
        want = {"set_repetition_penalty": "repetition_penalty", "weight_write": "svln_set_tensor", "op_gemv_batched_argmax": "svln_op_gemv_batched"}
        assert name == want.get(base, "svln_" + base), (ci, name)
    # the rows of a caller stand together, its parts in ascending order
    order = [(r["caller"], r["part"]) for r in rules]
    assert order == sorted(order)


def _pair_state(row):
    """the bits a switches_ref row leaves on (call-time rows: none)"""
    return [ROW_MODE[row]] if row in ROW_MODE else []


def _ask(row, state):
    """switching `row` on (or making the call) under `state` -> the table's message or None"""
    if row == "generate_group":                           # the Python surface switches sampling on for the call
        return _lib.mode_refusal("generate_group", on=state + ["sampling"])
    if row == "generate_forced":
        return _lib.mode_refusal("generate_forced", on=state)
    if row not in ROW_MODE:
        return None
    att = ROW_MODE[row] + ":on"
    for caller, who, same in steps_of(att, state):
        msg = _lib.mode_refusal(caller, on=state, no_change=same, who=who)
        if msg is not None:
            return msg
    return None


def test_switch_matrix_agrees_with_the_table():
    for a, b in S.pairs():
        e = S.entry(a, b)
        if {a, b} == {"generate_group", "generate_forced"}:
            continue                                      # the per-env refuse_while_group_on of the forced call: it reads the env, not a mode
        orders = [(x, y) for x, y in ((a, b), (b, a)) if not S.BY_NAME[x].call_time]        # x on, then y
        assert orders, (a, b)
        for first, second in orders:
            msg = _ask(second, _pair_state(first))
            if e.kind == S.REFUSED:
                assert msg is not None and e.names[first] in msg, (first, second, msg)
            else:
                assert msg is None, (first, second, msg)


def test_shared_texts_name_the_violated_bit(rules):
    for r in rules:
        named = re.findall(r"svln_\w+", r["text"])
        fn = BIT_FN[r["bit"]]
        if fn is None:
            assert not named, r
        else:
            assert fn in named, r
            assert set(named) - {fn} <= set(BIT_FN.values()) | {"svln_op_gemv_batched_argmax_sample"}, r
        if fn is not None and r["bit"] != "group":        # the sentence states the side of the bit that is violated
            assert (re.search(r"\b(is|are) off \(", r["text"]) is not None) == r["must_be_on"], r
            assert (re.search(r"\b(is|are) (on|set) \(", r["text"]) is not None) != r["must_be_on"], r


def test_bad_queries_are_refused():
    lib = _lib.load()
    with pytest.raises(_lib.SvlnError, match="unknown caller"):
        _lib.mode_refusal(len(_lib.MODE_CALLERS))
    with pytest.raises(_lib.SvlnError, match="unknown caller"):
        _lib.mode_refusal(-1)
    buf, refused = C.create_string_buffer(64), C.c_int32()
    assert lib.svln_mode_refusal(0, None, None, 0, buf, len(buf), C.byref(refused)) != 0
    assert b"null" in lib.svln_last_error()
    st = _lib.SvlnModeState(jobs=1)
    assert lib.svln_mode_refusal(0, None, C.byref(st), 0, buf, 8, C.byref(refused)) != 0 and b"fit" in lib.svln_last_error()
    assert lib.svln_mode_rule(0, None) != 0 and lib.svln_last_error()
    n = len(_lib.mode_rules())
    assert lib.svln_mode_rule(n, C.byref(_lib.SvlnModeRule())) != 0 and b"no such rule" in lib.svln_last_error()
    assert lib.svln_mode_rule_count(None, None, None) != 0 and lib.svln_last_error()
