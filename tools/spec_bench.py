#!/usr/bin/env python
"""Draft-verified greedy decode (svln_set_speculative) and drafts inside the prefill pass (svln_set_prefill_draft) next to the plain bf16
decode loop on the headline workload (bench.Runner: frames in, action ids out, 8-frame window, decode graph on), one box, one process
per build:

    python tools/spec_bench.py [--steps 20 --warmup 5] [--rows 4] [--ref-lib build_ab/libA.so] [--rounds 2]
    python tools/spec_bench.py --passes bf16,ride_oracle,ride_wrong0,ride_auto,ride_spec_oracle --ref-passes bf16,spec_oracle --ref-lib ...

Passes of this build, every one over the SAME seeded episode (agent memory, frame stream and prompt encoder are reset between passes):
  bf16          the mode off (must equal the --ref-lib build inside the box-to-box spread);
  spec_oracle   every turn armed with the ids a first plain run of the episode recorded for it: the acceptance rate is 1 by construction,
                so this is the ceiling of the mode;
  spec_wrong    the recorded ids with index 1 replaced: the worst case, one verify pass that emits one token, then single steps;
  spec_auto     set_auto_draft: the env's previous turn output is the draft.  The weights are random-initialised and the prompt stream synthetic, so how
                often turns repeat here says nothing about a real checkpoint.
  ride_oracle   svln_set_prefill_draft on, verify passes off, the recorded ids as drafts: the whole turn comes out of the prefill pass;
  ride_wrong0   the recorded ids with index 0 replaced: the worst case of a ride, k extra prefill rows and one extra synchronisation
                that emit what the plain prefill emits, then single steps;
  ride_auto     rides with set_auto_draft;
  ride_spec_oracle   rides AND verify passes on, recorded ids (the turns of this workload fit one ride, so no verify pass is expected).
Per pass: action-steps/s, phase_ms_per_turn (svln_phase_times), the counters of svln_draft_stats over the timed turns, the share of
decode tokens that verify passes emitted, and whether each timed turn's ids equal the plain run's.

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its passes (--ref-passes, default bf16; a build that has svln_set_speculative can also run the spec_* passes) run in a child process of its own, alternating with this build's passes `--rounds` times.  The parent process
never opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/spec_decode.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/spec_bench.py --child --passes spec_oracle --steps 10 --warmup 3
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "SPEC_BENCH_CHILD "


def child(a):
    import torch
    from streamvln_amd import _lib
    if os.environ.get("SVLN_LIB"):
        # an older build does not export the entry points this change adds: this tool (only) drops them from its copy of the table
        lib0 = C.CDLL(_lib.LIB_PATH)
        for name in list(_lib.SIGNATURES):
            if not hasattr(lib0, name):
                _lib.SIGNATURES.pop(name)
    import bench
    from streamvln_amd.config import CONFIGS
    from streamvln_amd.model import StreamVLNForCausalLM
    cfg = CONFIGS[a.config]
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=1, max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h
    plain_generate = model.generate
    armed = {"drafts": None, "turn": 0}

    def generate(*args, **kw):              # turn t of the pass is armed with drafts[t]
        if armed["drafts"] is not None:
            kw["draft_ids"] = armed["drafts"][armed["turn"]]
        armed["turn"] += 1
        return plain_generate(*args, **kw)
    model.generate = generate

    def restart(drafts=None):
        run.agent.reset_memory(); run.step = 0
        run.agent.prompt_encoder.reset()          # every pass sees the same prompt stream
        armed["drafts"], armed["turn"] = drafts, 0

    def turn_ids():
        run.turn()
        return run.agent.turn_log[-1]["out"].sequences[0].tolist()

    total = a.warmup + a.steps
    restart()
    plain = [turn_ids() for _ in range(total)]     # the recording run (also the process's warm-up: graphs captured, caches warm)
    vocab = cfg.vocab
    res = {}
    for mode in a.passes.split(","):
        drafts = None
        if mode == "spec_oracle":
            drafts = plain
        elif mode == "spec_wrong":
            drafts = [ids[:1] + [(ids[1] + 1) % vocab] + ids[2:] if len(ids) > 1 else ids for ids in plain]
        elif mode in ("ride_oracle", "ride_spec_oracle"):
            drafts = plain
        elif mode == "ride_wrong0":
            drafts = [[(ids[0] + 1) % vocab] + ids[1:] for ids in plain]
        ride = mode.startswith("ride_")
        if mode != "bf16":
            model.set_speculative(0 if ride and mode != "ride_spec_oracle" else a.rows)
            model.set_auto_draft(mode.endswith("_auto"))
        if ride:
            model.set_prefill_draft(True)
            model.prefill_draft_stats(reset=True)
        restart(drafts)
        got = [turn_ids() for _ in range(a.warmup)]
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        if mode != "bf16":
            model.draft_stats(reset=True)
        if ride:
            model.prefill_draft_stats(reset=True)
        dt = bench.timed_pass(model, lambda: got.append(turn_ids()), a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        r = {"action_steps_per_s": round(bench.NUM_FUTURE * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
             "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)},
             "ids_equal_plain_run_per_timed_turn": [g == p for g, p in zip(got[a.warmup:], plain[a.warmup:])]}
        if mode != "bf16":
            passes, vtok, single = model.draft_stats(reset=True)
            r["rows"] = 0 if ride and mode != "ride_spec_oracle" else a.rows
            r["counters_timed_turns"] = {"verify_passes": passes, "tokens_from_verify": vtok, "single_steps": single}
            r["share_of_decode_tokens_from_verify"] = round(vtok / max(vtok + single, 1), 4)
            if ride:
                rides, rtok, fed = model.prefill_draft_stats(reset=True)
                r["ride_counters_timed_turns"] = {"rides": rides, "tokens_from_rides": rtok, "rows_fed": fed}
                r["share_of_turn_tokens_from_rides"] = round(rtok / max(rtok + vtok + single, 1), 4)
                model.set_prefill_draft(False)
            model.set_auto_draft(False)
            model.set_speculative(0)
        res[mode] = r
    model.close()
    print(TAG + json.dumps(res), flush=True)


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--config", a.config, "--rows", str(a.rows)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)      # a fresh process per build, under its own limit
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child ({lib or 'this build'}) ended with status {p.returncode}: nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)][-1]
    sys.stderr.write(f"child ({lib or 'this build'}: {passes}) done\n"); sys.stderr.flush()
    return json.loads(line[len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4, help="rows per verify pass (2, 4, 8; rows * q_heads / kv_heads <= 32)")
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick for the bf16 pass")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="bf16,spec_oracle,spec_wrong,spec_auto")
    ap.add_argument("--ref-passes", default="bf16", help="passes the --ref-lib build runs (it must know the modes they switch on)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"bench.Runner headline workload, --steps {a.steps} --warmup {a.warmup}, 8-frame window, decode graph on, {a.rows} rows per "
                       f"verify pass, one box, builds alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, a.ref_passes)
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)

    def col(build, mode, f):
        v = [f(r[build][mode]) for r in out["rounds"] if mode in r.get(build, {})]
        return v or None
    yard = "parent_build" if a.ref_lib else "this_build"
    modes = [("bf16", yard)] + [(m, "parent_build") for m in (a.ref_passes.split(",") if a.ref_lib else []) if m != "bf16"] \
        + [(m, "this_build") for m in a.passes.split(",")]
    out["summary"] = {
        "action_steps_per_s_best": {f"{m} ({b})": max(col(b, m, lambda r: r["action_steps_per_s"]) or [0]) for m, b in modes},
        "decode_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["decode"]) or [0]) for m, b in modes},
        "prefill_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["prefill"]) or [0]) for m, b in modes},
        "ids_equal_plain_run_every_timed_turn": {m: all(all(x) for x in (col("this_build", m, lambda r: r["ids_equal_plain_run_per_timed_turn"]) or []))
                                                 for m in a.passes.split(",")}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
