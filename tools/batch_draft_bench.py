#!/usr/bin/env python
"""Drafts in the scheduler's prefill pass (svln_set_batch_draft) next to the plain lockstep workload of bench.py's batched pass (N envs
stepped together through generate_batch, bf16, 8-frame window), one box, one process per build:

    python tools/batch_draft_bench.py [--envs 2,4,8] [--steps 10 --warmup 3] [--ref-lib build_ab/libA.so] [--rounds 2]

Passes of this build, every one over the SAME seeded episode (agent memories, frame streams and prompt encoders are reset between passes):
  off           the switch off (must equal the --ref-lib build's bf16 pass inside the box-to-box spread);
  ride_oracle   every env's turn armed with the ids a first plain run of the episode recorded for it: every draft is right, so a lockstep
                turn is one scheduler iteration -- the ceiling of the mode;
  ride_wrong0   the recorded ids with index 0 replaced: the worst case, k extra prefill rows per env that emit what the plain prefill emits,
                then the plain decode iterations;
  ride_auto     set_auto_draft: each env's previous turn output is its draft.  The weights are random-initialised and the prompt stream
                synthetic, so how often turns repeat here says nothing about a real checkpoint.
Per pass and env count: action-steps/s, ms per lockstep turn, phase_ms_per_turn (svln_phase_times), the five counters of
svln_batch_draft_stats over the timed turns, and whether every timed turn's ids equal the plain run's.

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its bf16 pass runs in a child process of its own, alternating with this build's passes `--rounds` times.  The parent process
never opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/batch_draft.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/batch_draft_bench.py --child --passes ride_oracle --envs 8
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "BATCH_DRAFT_BENCH_CHILD "
COUNTERS = ("rides", "tokens_from_rides", "rows_fed", "iterations", "single_rows")


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
    armed = {"drafts": None, "turn": 0}

    def generate_batch(reqs, **kw):          # lockstep turn t of the pass: env e is armed with drafts[t][e]
        if armed["drafts"] is not None:
            reqs = [dict(r, draft_ids=d) for r, d in zip(reqs, armed["drafts"][armed["turn"]])]
        armed["turn"] += 1
        return plain_generate_batch(reqs, **kw)
    model.generate_batch = generate_batch
    res = {}
    for n in env_counts:
        model.reset(n)
        agents = [StreamingAgent(model, SyntheticPromptEncoder(cfg, seed=7 + 31 * e), num_frames=bench.NUM_FRAMES,
                                 num_future_steps=bench.NUM_FUTURE, num_history=bench.NUM_HISTORY, env_id=e, device="cuda",
                                 max_new_tokens=bench.DECODE_TOKENS, eos_token_ids=(), preprocess=run.preprocess) for e in range(n)]
        group = BatchedAgents(agents)
        bstep = [0]

        def restart(drafts=None):
            for ag in agents:
                ag.reset_memory()
                ag.prompt_encoder.reset()          # every pass sees the same prompt streams
            bstep[0] = 0
            armed["drafts"], armed["turn"] = drafts, 0

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
        restart()
        plain = [lockstep_turn() for _ in range(total)]      # the recording run (also the warm-up: graphs captured, caches warm)
        res[str(n)] = {}
        for mode in a.passes.split(","):
            drafts = None
            if mode == "ride_oracle":
                drafts = plain
            elif mode == "ride_wrong0":
                drafts = [[[(ids[0] + 1) % cfg.vocab] + ids[1:] for ids in turn] for turn in plain]
            ride = mode.startswith("ride_")
            if ride:
                model.set_batch_draft(True)
                model.set_auto_draft(mode.endswith("_auto"))
            restart(drafts)
            got = [lockstep_turn() for _ in range(a.warmup)]
            d3 = [C.c_double() for _ in range(3)]
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
            if not ref:
                model.batch_draft_stats(reset=True)
            dt = bench.timed_pass(model, lambda: got.append(lockstep_turn()), a.steps, 0, 1)
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
            r = {"action_steps_per_s": round(bench.NUM_FUTURE * n * a.steps / dt, 2), "ms_per_lockstep_turn": round(dt / a.steps * 1e3, 3),
                 "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)},
                 "ids_equal_plain_run_per_timed_turn": [g == p for g, p in zip(got[a.warmup:], plain[a.warmup:])]}
            if not ref:
                r["counters_timed_turns"] = dict(zip(COUNTERS, model.batch_draft_stats(reset=True)))
            if ride:
                model.set_auto_draft(False)
                model.set_batch_draft(False)
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
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick for the switch-off pass")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="off,ride_oracle,ride_wrong0,ride_auto")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"the lockstep workload of bench.py's batched pass (generate_batch, bf16, 8-frame window), --steps {a.steps} --warmup "
                       f"{a.warmup}, one box, builds alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box,
           "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, "bf16")
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)
    modes = ([("bf16", "parent_build")] if a.ref_lib else []) + [(m, "this_build") for m in a.passes.split(",")]
    summary = {}
    for n in a.envs.split(","):
        def col(build, mode, f):
            return [f(r[build][n][mode]) for r in out["rounds"] if mode in r.get(build, {}).get(n, {})]
        summary[n] = {
            "action_steps_per_s_best": {f"{m} ({b})": max(col(b, m, lambda r: r["action_steps_per_s"])) for m, b in modes},
            "prefill_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["prefill"])) for m, b in modes},
            "decode_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["decode"])) for m, b in modes},
            "ids_equal_plain_run_every_timed_turn": {m: all(all(all(t) if isinstance(t, list) else t for t in x)
                                                            for x in col("this_build", m, lambda r: r["ids_equal_plain_run_per_timed_turn"]))
                                                     for m in a.passes.split(",")}}
    out["summary"] = summary
    print(json.dumps(out))


if __name__ == "__main__":
    main()
