#!/usr/bin/env python
"""Multi-draft turns (generate(draft_set=...) / svln_turn_drafts) next to the plain bf16 decode loop and to the single-draft ride of
svln_set_prefill_draft on the headline workload (bench.Runner: frames in, action ids out, 8-frame window, decode graph on), one box, one
process per build:

    python tools/drafts_bench.py [--steps 20 --warmup 5] --ref-lib build_ab/libA.so [--rounds 2]

Passes, every one over the SAME seeded episode (agent memory, frame stream and prompt encoder are reset between passes):
  bf16          the plain loop: no draft_set (this build: the feature unused; must equal the --ref-lib build inside the box-to-box spread);
  ride_oracle   (the --ref-lib build) svln_set_prefill_draft with the ids a first plain run recorded: the yardstick for the best case;
  g4_first      four drafts, the recorded ids at index 0, the others wrong at id 0;
  g4_last       four drafts, the recorded ids at index 3: the winner's pages change hands;
  g4_wrong      four drafts, every one wrong at id 0: the worst case, G r extra rows and one extra synchronisation that emit token 0 alone;
  g8_wrong      the same with eight drafts;
  history       StreamingAgent.draft_history = 4: the env's four most recent distinct turn outputs.  The weights are random-initialised and
                the prompt stream synthetic, so how often turns repeat here says nothing about a real checkpoint.
Per pass: action-steps/s, phase_ms_per_turn (svln_phase_times), the eight counters of svln_drafts_stats over the timed turns, and whether
each timed turn's ids equal the plain run's.

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick; its passes run in a child process of its own, alternating with this build's passes `--rounds` times.  The parent process never
opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/multi_draft.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/drafts_bench.py --child --passes g4_last --steps 10 --warmup 3
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "DRAFTS_BENCH_CHILD "
COUNTERS = ("calls", "passes", "pass_tokens", "rows_fed", "finished_in_pass", "ignored", "handovers", "single_steps")


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
    has_drafts = hasattr(lib, "svln_drafts_stats")
    plain_generate = model.generate
    armed = {"sets": None, "ride": None, "turn": 0}

    def generate(*args, **kw):              # turn t of the pass carries sets[t] (or the single draft ride[t])
        if armed["sets"] is not None:
            kw["draft_set"] = armed["sets"][armed["turn"]]
        if armed["ride"] is not None:
            kw["draft_ids"] = armed["ride"][armed["turn"]]
        armed["turn"] += 1
        return plain_generate(*args, **kw)
    model.generate = generate

    def restart(sets=None, ride=None, history=0):
        run.agent.reset_memory(); run.step = 0
        run.agent.prompt_encoder.reset()          # every pass sees the same prompt stream
        run.agent.draft_history = history
        armed["sets"], armed["ride"], armed["turn"] = sets, ride, 0

    def turn_ids():
        run.turn()
        return run.agent.turn_log[-1]["out"].sequences[0].tolist()

    total = a.warmup + a.steps
    restart()
    plain = [turn_ids() for _ in range(total)]     # the recording run (also the process's warm-up: graphs captured, caches warm)
    vocab = cfg.vocab
    wrong = lambda ids, g: [(ids[0] + 1 + g) % vocab] + ids[1:]
    res = {}
    for mode in a.passes.split(","):
        sets = ride = None
        history = 0
        if mode == "g4_first":
            sets = [[ids] + [wrong(ids, g) for g in range(3)] for ids in plain]
        elif mode == "g4_last":
            sets = [[wrong(ids, g) for g in range(3)] + [ids] for ids in plain]
        elif mode in ("g4_wrong", "g8_wrong"):
            sets = [[wrong(ids, g) for g in range(int(mode[1]))] for ids in plain]
        elif mode == "history":
            history = 4
        elif mode == "ride_oracle":
            ride = plain
            model.set_prefill_draft(True)
        elif mode != "bf16":
            raise SystemExit(f"unknown pass {mode}")
        restart(sets, ride, history)
        got = [turn_ids() for _ in range(a.warmup)]
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        before = model.drafts_stats() if has_drafts else None
        dt = bench.timed_pass(model, lambda: got.append(turn_ids()), a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        r = {"action_steps_per_s": round(bench.NUM_FUTURE * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
             "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)},
             "ids_equal_plain_run_per_timed_turn": [g == p for g, p in zip(got[a.warmup:], plain[a.warmup:])]}
        if has_drafts:
            r["counters_timed_turns"] = dict(zip(COUNTERS, (x - y for x, y in zip(model.drafts_stats(), before))))
        if mode == "ride_oracle":
            model.set_prefill_draft(False)
        res[mode] = r
    model.close()
    print(TAG + json.dumps(res), flush=True)


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--config", a.config]
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
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="bf16,g4_first,g4_last,g4_wrong,g8_wrong,history")
    ap.add_argument("--ref-passes", default="bf16,ride_oracle", help="passes the --ref-lib build runs")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"bench.Runner headline workload, --steps {a.steps} --warmup {a.warmup}, 8-frame window, decode graph on, one box, builds "
                       f"alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, a.ref_passes)
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)

    def col(build, mode, f):
        v = [f(r[build][mode]) for r in out["rounds"] if mode in r.get(build, {})]
        return v or None
    modes = [(m, "parent_build") for m in (a.ref_passes.split(",") if a.ref_lib else [])] + [(m, "this_build") for m in a.passes.split(",")]
    out["summary"] = {
        "action_steps_per_s_best": {f"{m} ({b})": max(col(b, m, lambda r: r["action_steps_per_s"]) or [0]) for m, b in modes},
        "decode_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["decode"]) or [0]) for m, b in modes},
        "prefill_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["prefill"]) or [0]) for m, b in modes},
        "ids_equal_plain_run_every_timed_turn": {m: all(all(x) for x in (col("this_build", m, lambda r: r["ids_equal_plain_run_per_timed_turn"]) or []))
                                                 for m in a.passes.split(",")}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
