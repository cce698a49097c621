"""The switch table of tests/switches_ref.py against include/streamvln_hip.h (no GPU): every `svln_set_*` prototype has a row, the pair
matrix is symmetric and total, every refusal names a function that exists, every precedence and exclusion says why."""
import os
import re

import switches_ref as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "streamvln_hip.h")


def _prototypes():
    text = open(HEADER).read()
    return set(re.findall(r"^int\s+(svln_\w+)\s*\(", text, flags=re.M))


def test_every_set_prototype_of_the_header_has_a_row():
    protos = _prototypes()
    setters = {p for p in protos if p.startswith("svln_set_")}
    assert len(setters) >= 21, sorted(setters)                # the parser found them (21 at the time of writing)
    rows = {r.c_name for r in S.ROWS}
    assert len(rows) == len(S.ROWS) == len(set(S.NAMES))      # one row per function, one name per row
    missing = setters - rows - set(S.NOT_SWITCHES)
    assert not missing, f"switches without a row in tests/switches_ref.py: {sorted(missing)}"
    assert not (set(S.NOT_SWITCHES) & rows)
    for name, why in S.NOT_SWITCHES.items():
        assert name in protos and why.strip(), name
    unknown = rows - protos
    assert not unknown, f"rows that name no function of the header: {sorted(unknown)}"
    for r in S.ROWS:                                          # the call-time rows are the only ones that are not setters
        assert r.call_time == (not r.c_name.startswith("svln_set_")), r.name


def test_rows_are_complete():
    for r in S.ROWS:
        assert r.cls in ("lossless", "scheme", "output", "draft"), r.name
        assert r.dtypes and set(r.dtypes) <= set(S.BOTH) and S.BF16 in r.dtypes, r.name
        assert callable(r.on) and callable(r.off) and r.setter, r.name
        assert r.effect is not None or r.note.strip(), f"{r.name}: no effect probe and no reason"
        if r.effect is not None:
            assert r.effect[0] in ("stat", "key", "subset", "differs", "call"), r.name
    classes = {c: {r.name for r in S.ROWS if r.cls == c} for c in ("lossless", "scheme", "output", "draft")}
    assert classes["lossless"] == {"decode_graph", "packed_decode", "feature_cache", "layer_taps"}
    assert classes["scheme"] == {"fp8_decode", "mxfp4_decode", "mxfp4_batched", "fp8_gemm", "fp8_scaled_mfma", "decode_persistent", "memory_prune",
                                 "turn_row_limit"}
    assert classes["output"] == {"token_scores", "sampling", "allowed_tokens", "repetition_penalty", "generate_group", "generate_forced"}
    assert classes["draft"] == {"speculative", "prefill_draft", "batch_draft", "draft"}
    # restore() reaches every row: each is either switched off in the fixed order or part of the probe's base state
    assert sorted(S.RESTORE_ORDER + S.BASE_ON) == sorted(S.NAMES)


def test_matrix_is_total_and_symmetric():
    n = len(S.NAMES)
    assert len(S.PAIRS) == n * (n - 1) // 2 == len(S.pairs())
    for a in S.NAMES:
        for b in S.NAMES:
            if a == b:
                continue
            e = S.entry(a, b)
            assert e is S.entry(b, a)                         # one entry per unordered pair, whichever way it is asked
            assert e.kind in (S.REFUSED, S.COMPOSES, S.NO_EFFECT)
    c = S.counts()
    assert c[S.REFUSED] + c[S.COMPOSES] + c[S.NO_EFFECT] == len(S.PAIRS)


def test_refusals_name_functions_of_the_header():
    protos = _prototypes()
    for (a, b) in S.pairs():
        e = S.entry(a, b)
        if e.kind != S.REFUSED:
            assert e.names is None
            continue
        assert set(e.names) == {a, b}, (a, b)                 # both orders
        for on_first, fn in e.names.items():
            assert fn in protos, (a, b, fn)
            # a setter that is on is named by its own function; a pending group by the call that resolves it
            assert fn == S.BY_NAME[on_first].c_name or (S.BY_NAME[on_first].call_time and fn == "svln_group_select"), (a, b, fn)
    # the lists the engine shares between its setters (engine.hip: spec_exclusive_on, refuse_while_plain_head_only, single_scheme_on)
    for d in S.DRAFT3:
        for s in S.SCHEME5 + ("token_scores", "sampling"):
            assert S.entry(d, s).kind == S.REFUSED, (d, s)
    for p in S.PLAIN_HEAD:
        for o in ("token_scores", "sampling", "generate_group"):
            assert S.entry(p, o).kind == S.REFUSED, (p, o)
    for s in S.SINGLE_SCHEME:
        assert S.entry("generate_forced", s).kind == S.REFUSED, s
    assert S.entry("generate_forced", "mxfp4_batched").kind == S.COMPOSES     # scheduler paths only: the header says so


def test_precedence_and_exclusions_carry_a_reason():
    excluded = 0
    for (a, b) in S.pairs():
        e = S.entry(a, b)
        if e.kind == S.NO_EFFECT:
            assert e.inert in (a, b) and e.reason.strip(), (a, b)
            assert re.search(r"svln_\w+", e.reason), (a, b)   # the reason points at the header entry that documents it
        else:
            assert e.inert is None
        if e.excluded is not None:
            excluded += 1
            assert e.excluded.strip(), (a, b)
            other = a if b == "decode_persistent" else b
            assert "decode_persistent" in (a, b) and other not in S.PERSISTENT_RUNS, (a, b)       # the cap on what the run part may leave out
        elif "decode_persistent" in (a, b):
            assert (a if b == "decode_persistent" else b) in S.PERSISTENT_RUNS
    assert excluded == len(S.NAMES) - 1 - len(S.PERSISTENT_RUNS) == S.counts()["excluded"]


def test_header_documents_the_decisions():
    """the decisions this table rests on are stated where a caller reads them"""
    text = " ".join(re.sub(r"\n\s*\*\s", " ", open(HEADER).read()).split())          # comment text without its line breaks
    for phrase in ("svln_set_tensor / svln_synth_tensor",                      # the weight-write hook
                   "whatever svln_set_fp8_decode or svln_set_mxfp4_decode says",  # a group under the single-env decode switches
                   "cannot change while scheduler turns are in flight"):
        assert phrase in text, phrase
