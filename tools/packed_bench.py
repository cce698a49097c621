#!/usr/bin/env python
"""Packed-decode weights (svln_set_packed_decode) next to the bf16 decode GEMVs on the headline workload (bench.Runner: frames in, action
ids out, 8-frame window, decode graph on), one box, a fresh process per build:

    python tools/packed_bench.py [--steps 20 --warmup 5] [--ref-lib build_ab/libA.so] [--rounds 2]

Passes of this build, every one over the SAME seeded episode: `on` (the default of a bf16 engine) and `off`; the --ref-lib build (another
commit, tools/build_ref_lib.sh: the code under test is not its own yardstick) runs its plain pass in a child process of its own,
alternating with this build's child `--rounds` times.  Per pass: action-steps/s, phase_ms_per_turn (svln_phase_times), the probed layer-0
gate/up launch (svln_probe_read: mean us, bytes, TB/s) and the ids of every timed turn.  The tool FAILS unless every pass of every round
emitted the same ids in every timed turn.  The parent process never opens the GPU; every child runs under its own time limit, and nothing
is started after a child that failed.  Prints ONE JSON line (committed as profiles/packed_decode.json)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "PACKED_BENCH_CHILD "


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
    has_switch = "svln_set_packed_decode" in _lib.SIGNATURES

    def restart():
        run.agent.reset_memory(); run.step = 0
        run.agent.prompt_encoder.reset()          # every pass sees the same prompt stream

    def turn_ids():
        run.turn()
        return run.agent.turn_log[-1]["out"].sequences[0].tolist()

    res = {}
    if has_switch:
        res["packed_stats"] = model.packed_stats()
    for mode in a.passes.split(","):
        if mode in ("on", "off"):
            model.set_packed_decode(mode == "on")
        restart()
        for _ in range(a.warmup + (a.steps if not res.get("warm") else 0)):      # the first pass of a process also runs the episode once untimed
            turn_ids()
        res["warm"] = True
        restart()
        got = [turn_ids() for _ in range(a.warmup)]
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        _lib.check(lib.svln_probe_reset(h))
        dt = bench.timed_pass(model, lambda: got.append(turn_ids()), a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(lib.svln_probe_read(h, C.byref(ms), C.byref(n), C.byref(by)))
        us = ms.value / max(n.value, 1) * 1e3
        res[mode] = {"action_steps_per_s": round(bench.NUM_FUTURE * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
                     "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)},
                     "gate_up_probe": {"launches": n.value, "mean_us": round(us, 2), "bytes": by.value, "TB_per_s": round(by.value / max(us, 1e-9) / 1e6, 3)},
                     "ids": got[a.warmup:]}
    res.pop("warm")
    model.close()
    print(TAG + json.dumps(res), flush=True)


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup), "--config", a.config]
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
    ap.add_argument("--ref-lib", default=None, help="library of the parent commit (tools/build_ref_lib.sh): the yardstick")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="on,off")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"bench.Runner headline workload, --steps {a.steps} --warmup {a.warmup}, 8-frame window, decode graph on, one box, builds "
                       f"alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box, "rounds": []}
    ids = None
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, "plain")
        rnd["this_build"] = spawn(a, None, a.passes)
        for build, passes in rnd.items():
            for mode, r in passes.items():
                if mode == "packed_stats":
                    continue
                got = r.pop("ids")
                ids = ids or got
                if got != ids:
                    raise SystemExit(f"{build} / {mode}: the ids of the timed turns differ from the first pass's")
        out["rounds"].append(rnd)
    out["ids_equal_in_every_timed_turn_of_every_pass"] = True
    out["ids_of_the_first_timed_turns"] = ids[:3]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
