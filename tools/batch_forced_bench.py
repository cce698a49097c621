#!/usr/bin/env python
"""Forced jobs in the multi-env scheduler (svln_batch_submit_forced / generate_batch_forced) next to the only way that existed before them,
on the lockstep workload of bench.py's batched pass (N envs stepped together, bf16, 8-frame window, 5-id turns), one box, one process per
build:

    python tools/batch_forced_bench.py [--envs 2,4,8] [--steps 10 --warmup 3] [--ref-lib build_ab/libA.so] [--rounds 2]

Every pass runs the SAME seeded episode (agent memories, frame streams and prompt encoders are reset between passes); the forced ids of
turn t of env e are the ids a first plain run of the episode recorded for it, so every pass leaves the envs where the plain run does.
  plain          the feature unused: generate_batch (both builds: must agree inside the box-to-box spread -- the launches are the same);
  single         the feature unused: bench.py's single-env turn (both builds);
  forced_solo    every env's turn as generate(forced_ids=...), one env after another: the yardstick, what a collector had to do before
                 (both builds; the parent's figure is the one to beat);
  forced_batch   every env's turn as a forced job of ONE generate_batch_forced call (this build);
  half_solo      envs 0, 2, 4, .. forced singly, then generate_batch for the rest: the yardstick of the mix (both builds);
  half_batch     the same mix as one generate_batch_forced call (this build).
Per pass and env count: action-steps/s, ms per lockstep turn, phase_ms_per_turn (svln_phase_times), and for this build the three counters of
svln_batch_forced_stats over the timed turns.

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its passes run in a child process of their own, alternating with this build's `--rounds` times.  The parent process never
opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/batch_forced.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/batch_forced_bench.py --child --passes forced_batch --envs 8
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "BATCH_FORCED_BENCH_CHILD "
BOTH = ("plain", "single", "forced_solo", "half_solo")
NEW = ("forced_batch", "half_batch")


def child(a):
    import torch
    from streamvln_amd import _lib
    ref = bool(os.environ.get("SVLN_LIB"))
    if ref:
        # an older build does not export the entry points this change adds: this tool (only) drops them from its copy of the table
        lib0 = C.CDLL(_lib.LIB_PATH)
        for name in list(_lib.SIGNATURES):
            if not hasattr(lib0, name):
                _lib.SIGNATURES.pop(name)
    import bench
    from streamvln_amd.agent import BatchedAgents, StreamingAgent
    from streamvln_amd.config import CONFIGS
    from streamvln_amd.model import StreamVLNForCausalLM
    from streamvln_amd.synthetic import SyntheticPromptEncoder
    cfg = CONFIGS[a.config]
    env_counts = [int(x) for x in a.envs.split(",")]
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=max(env_counts), max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h
    plain_generate_batch = model.generate_batch
    st = {"mode": "plain", "forced": None, "turn": 0}

    def generate_batch(reqs, **kw):          # lockstep turn t of the pass: env e is forced onto forced[t][e] as the pass says
        mode, t = st["mode"], st["turn"]
        st["turn"] += 1
        if mode == "plain":
            return plain_generate_batch(reqs, **kw)
        F = st["forced"][t]
        half = mode.startswith("half_")
        is_forced = [(not half) or e % 2 == 0 for e in range(len(reqs))]
        if mode.endswith("_batch"):
            return model.generate_batch_forced([dict(r, forced_ids=F[e]) if is_forced[e] else r for e, r in enumerate(reqs)], **kw)
        outs = [None] * len(reqs)
        for e, r in enumerate(reqs):             # the way of before: the forced turns one env after another on an idle scheduler ...
            if is_forced[e]:
                outs[e] = model.generate(**dict(r, forced_ids=F[e]))
        rest = [e for e in range(len(reqs)) if not is_forced[e]]
        if rest:                                 # ... then the plain turns of the others together
            for e, o in zip(rest, plain_generate_batch([reqs[e] for e in rest], **kw)):
                outs[e] = o
        return outs
    model.generate_batch = generate_batch
    passes = a.passes.split(",")
    res = {}

    def measure(turn_fn, per_turn_actions):
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        if not ref:
            model.batch_forced_stats(reset=True)
        dt = bench.timed_pass(model, turn_fn, a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        r = {"action_steps_per_s": round(per_turn_actions * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
             "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)}}
        if not ref:
            r["counters_timed_turns"] = model.batch_forced_stats(reset=True)
        return r
    if "single" in passes:
        model.reset(1)
        for _ in range(a.warmup):
            run.turn()
        res["1"] = {"single": measure(run.turn, bench.NUM_FUTURE)}
    for n in env_counts:
        model.reset(n)
        agents = [StreamingAgent(model, SyntheticPromptEncoder(cfg, seed=7 + 31 * e), num_frames=bench.NUM_FRAMES,
                                 num_future_steps=bench.NUM_FUTURE, num_history=bench.NUM_HISTORY, env_id=e, device="cuda",
                                 max_new_tokens=bench.DECODE_TOKENS, eos_token_ids=(), preprocess=run.preprocess) for e in range(n)]
        group = BatchedAgents(agents)
        bstep = [0]

        def restart(mode, forced=None):
            for ag in agents:
                ag.reset_memory()
                ag.prompt_encoder.reset()          # every pass sees the same prompt streams
            bstep[0] = 0
            st["mode"], st["forced"], st["turn"] = mode, forced, 0

        def lockstep_turn():                       # bench.py's batched pass: env e sees the stream shifted by 7e frames
            n0 = len(agents[0].turn_log)
            while len(agents[0].turn_log) == n0:
                if bstep[0] == bench.EP_STEPS:
                    for ag in agents:
                        ag.reset_memory()
                    bstep[0] = 0
                group.act([(bstep[0] + 7 * e) % bench.EP_STEPS for e in range(n)])
                bstep[0] += 1
            ids = [ag.turn_log[-1]["out"].sequences[0].tolist() for ag in agents]
            for ag in agents:
                ag.turn_log[:] = ag.turn_log[-1:]
            return ids
        total = a.warmup + a.steps
        restart("plain")
        plain = [lockstep_turn() for _ in range(total)]      # the recording run (also the warm-up: graphs captured, caches warm)
        res[str(n)] = {}
        for mode in passes:
            if mode == "single" or (mode.startswith("half_") and n != max(env_counts)):
                continue
            restart(mode, plain)
            got = [lockstep_turn() for _ in range(a.warmup)]
            r = measure(lambda: got.append(lockstep_turn()), bench.NUM_FUTURE * n)
            r["ids_equal_plain_run_per_timed_turn"] = [g == p for g, p in zip(got[a.warmup:], plain[a.warmup:])]
            res[str(n)][mode] = r
    model.close()
    print(TAG + json.dumps(res), flush=True)


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--config", a.config, "--envs", a.envs]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)      # a fresh process per build, under its own limit
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child ({lib or 'this build'}) ended with status {p.returncode}: nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)][-1]
    sys.stderr.write(f"child ({lib or 'this build'}: {passes}) done\n"); sys.stderr.flush()
    return json.loads(line[len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", default="2,4,8", help="env counts of the lockstep workload")
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default=",".join(BOTH + NEW))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"the lockstep workload of bench.py's batched pass (bf16, 8-frame window, 5-id turns), --steps {a.steps} --warmup {a.warmup}, "
                       f"one box, builds alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box, "rounds": []}
    both = ",".join(p for p in a.passes.split(",") if p in BOTH)
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib and both:
            rnd["parent_build"] = spawn(a, a.ref_lib, both)
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)
    summary = {}
    for n in ["1"] + a.envs.split(","):
        row = {}
        for build in ("parent_build", "this_build"):
            for mode in a.passes.split(","):
                col = [r[build][n][mode] for r in out["rounds"] if mode in r.get(build, {}).get(n, {})]
                if col:
                    best = max(col, key=lambda r: r["action_steps_per_s"])
                    row[f"{mode} ({build})"] = {"action_steps_per_s_best": best["action_steps_per_s"], "ms_per_turn_best": best["ms_per_turn"],
                                                "phase_ms_per_turn": best["phase_ms_per_turn"], "counters_timed_turns": best.get("counters_timed_turns")}
        if row:
            summary[n] = row
    out["summary"] = summary
    print(json.dumps(out))


if __name__ == "__main__":
    main()
