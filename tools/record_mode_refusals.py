#!/usr/bin/env python3
"""Record what the engine answers to every mode switch and turn form under every reachable mode state (tests/mode_refusals_ref.py) as
tests/golden/mode_refusals.json.  Needs a GPU.  The record is the yardstick of tests/test_mode_table.py and
tests/test_mode_refusals_gpu.py, so it is made from the commit BEFORE a change to the rules, never from the code under test:

    python tools/record_mode_refusals.py --commit <hash of the tree it runs on> [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the engine was built from (stored in the header)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mode_refusals.json"))
    a = ap.parse_args()
    import mode_refusals_ref as R
    import switch_probe as P
    m = P.make_model()
    t0 = time.perf_counter()
    rec = R.observe(m)
    dt = time.perf_counter() - t0
    m.close()
    doc = {"header": {"recorded_from": a.commit, "engine": "bf16 TINY (tests/switch_probe.make_model)",
                      "columns": ["state: index into states (the modes that are on, prerequisites included; jobs / group last)",
                                  "attempt: index into attempts (<mode>:on / <mode>:off = its setter, else the C function called)",
                                  "message: index into messages (0 = accepted, else the complete refusal text)"]},
           "states": rec["states"], "attempts": rec["attempts"], "messages": rec["messages"]}
    text = json.dumps(doc, indent=1)[:-2] + ',\n "rows": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rec["rows"]) + "\n ]\n}\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(f"{len(rec['states'])} states x {len(rec['attempts'])} attempts = {len(rec['rows'])} rows, {len(rec['messages'])} distinct messages, "
          f"observe() took {dt:.2f} s -> {a.out} ({len(text)} bytes)")


if __name__ == "__main__":
    main()
