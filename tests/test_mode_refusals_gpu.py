"""The engine answers every setter, weight write and turn form under every reachable mode state as tests/golden/mode_refusals.json
records it (tests/mode_refusals_ref.py; recorded before the rules moved into csrc/modes.h): the engine really asks the table, with the
state it is in.  tests/test_mode_table.py holds the table itself against the same record without a GPU."""
import json
import os

import pytest

import mode_refusals_ref as R
import switch_probe as P

pytestmark = pytest.mark.gpu

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mode_refusals.json")


def test_engine_answers_as_recorded():
    want = json.load(open(RECORD))
    m = P.make_model()
    try:
        got = R.observe(m)
    finally:
        m.close()
    assert got["attempts"] == want["attempts"]
    assert got["states"] == want["states"], "the reachable states differ"
    diff = [(g, w) for g, w in zip(got["rows"], want["rows"]) if (g[:2], got["messages"][g[2]]) != (w[:2], want["messages"][w[2]])]
    if diff:
        g, w = diff[0]
        raise AssertionError(f"{len(diff)} of {len(want['rows'])} rows differ; first: under {want['states'][w[0]]} {want['attempts'][w[1]]} -> "
                             f"recorded {want['messages'][w[2]]!r}, engine {got['messages'][g[2]]!r}")
    assert len(got["rows"]) == len(want["rows"])
