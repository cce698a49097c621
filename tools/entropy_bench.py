#!/usr/bin/env python
"""What token entropies (svln_token_entropy) cost, on the headline workload (bench.Runner: frames in, action ids out, 8-frame window,
decode graph on, bf16, single env) and on the lockstep workload of bench.py's batched pass (N envs through generate_batch: the MFMA head
at 8 envs), one box, one process per build:

    python tools/entropy_bench.py [--steps 12 --warmup 3] [--envs 8] [--ref-lib build_ab/libA.so] [--rounds 2]

Passes of this build, every one over the SAME seeded episode (agent memories, frame streams and prompt encoders are reset between passes):
  off      every switch off;
  scores   svln_set_token_scores on, entropies off: must equal the --ref-lib build's scored pass inside the box-to-box spread (the
           launched kernels are the previous instantiations);
  entropy  scores on and svln_token_entropy on: the EPI_*_ENT sibling of the lm_head product plus entropy_merge_kernel per head pass.
Per pass: action-steps/s, ms per turn, phase_ms_per_turn (svln_phase_times), whether every timed turn's ids equal the plain run's, and
for `entropy` whether every turn carries one finite entropy >= 0 per id and the bits of token_logprobs the scored pass gave.

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its passes (off, scores) run in a child process of their own, alternating with this build's passes `--rounds` times.  The
parent process never opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/token_entropy.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats -M --output-format csv -d out -- python tools/entropy_bench.py --child --passes entropy --steps 10 --warmup 3
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "ENTROPY_BENCH_CHILD "


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
    from streamvln_amd.agent import BatchedAgents, StreamingAgent
    from streamvln_amd.config import CONFIGS
    from streamvln_amd.model import StreamVLNForCausalLM
    from streamvln_amd.synthetic import SyntheticPromptEncoder
    cfg = CONFIGS[a.config]
    env_counts = [int(x) for x in a.envs.split(",") if x]
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=max(env_counts + [1]), max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h

    def measure(restart, turn, per_turn_actions, modes):
        total = a.warmup + a.steps
        restart()
        plain = [turn()[0] for _ in range(total)]          # the recording run (also the warm-up: graphs captured, caches warm)
        out = {}
        scored = [None]
        for mode in modes:
            if mode != "off":
                model.set_token_scores(True)
            if mode == "entropy":
                model.set_token_entropy(True)
            restart()
            got = [turn() for _ in range(a.warmup)]
            d3 = [C.c_double() for _ in range(3)]
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
            dt = bench.timed_pass(model, lambda: got.append(turn()), a.steps, 0, 1)
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
            timed = got[a.warmup:]
            r = {"action_steps_per_s": round(per_turn_actions * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
                 "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)},
                 "ids_equal_plain_run_per_timed_turn": [g[0] == p for g, p in zip(timed, plain[a.warmup:])]}
            if mode == "scores":
                scored[0] = [[o.token_logprobs.view(torch.int32).tolist() for o in g[1]] for g in timed]
            if mode == "entropy":
                r["every_id_has_a_finite_entropy"] = all(
                    o.token_entropies is not None and tuple(o.token_entropies.shape) == tuple(o.sequences.shape)
                    and bool(torch.isfinite(o.token_entropies).all()) and bool((o.token_entropies >= 0).all()) for g in timed for o in g[1])
                r["mean_entropy_nats"] = round(float(torch.cat([o.token_entropies.reshape(-1).cpu() for g in timed for o in g[1]]).mean()), 4)
                if scored[0] is not None:
                    r["token_logprobs_bits_equal_scored_pass"] = scored[0] == [[o.token_logprobs.view(torch.int32).tolist() for o in g[1]] for g in timed]
                model.set_token_entropy(False)
            if mode != "off":
                model.set_token_scores(False)
            out[mode] = r
        return out

    res = {}
    passes = a.passes.split(",")
    if a.single:
        def restart1():
            run.agent.reset_memory(); run.step = 0
            run.agent.prompt_encoder.reset()

        def turn1():
            run.turn()
            o = run.agent.turn_log[-1]["out"]
            return [o.sequences[0].tolist()], [o]
        res["1"] = measure(restart1, turn1, bench.NUM_FUTURE, passes)
    for n in env_counts:
        model.reset(n)
        agents = [StreamingAgent(model, SyntheticPromptEncoder(cfg, seed=7 + 31 * e), num_frames=bench.NUM_FRAMES,
                                 num_future_steps=bench.NUM_FUTURE, num_history=bench.NUM_HISTORY, env_id=e, device="cuda",
                                 max_new_tokens=bench.DECODE_TOKENS, eos_token_ids=(), preprocess=run.preprocess) for e in range(n)]
        group = BatchedAgents(agents)
        bstep = [0]

        def restart():
            for ag in agents:
                ag.reset_memory()
                ag.prompt_encoder.reset()          # every pass sees the same prompt streams
            bstep[0] = 0

        def lockstep_turn():                       # bench.py's batched pass: env e sees the stream shifted by 7e frames
            n0 = len(agents[0].turn_log)
            while len(agents[0].turn_log) == n0:
                if bstep[0] == bench.EP_STEPS:
                    for ag in agents:
                        ag.reset_memory()
                    bstep[0] = 0
                group.act([(bstep[0] + 7 * e) % bench.EP_STEPS for e in range(n)])
                bstep[0] += 1
            outs = [ag.turn_log[-1]["out"] for ag in agents]
            for ag in agents:
                ag.turn_log[:] = ag.turn_log[-1:]
            return [o.sequences[0].tolist() for o in outs], outs
        res[f"{n} lockstep"] = measure(restart, lockstep_turn, bench.NUM_FUTURE * n, passes)
    model.close()
    print(TAG + json.dumps(res), flush=True)


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--config", a.config, "--envs", a.envs] + ([] if a.single else ["--no-single"])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)      # a fresh process per build, under its own limit
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child ({lib or 'this build'}) ended with status {p.returncode}: nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)][-1]
    sys.stderr.write(f"child ({lib or 'this build'}: {passes}) done\n"); sys.stderr.flush()
    return json.loads(line[len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", default="8", help="env counts of the lockstep workload (comma separated; empty = none)")
    ap.add_argument("--no-single", dest="single", action="store_false", help="skip the single-env workload")
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick for the switch-off pass")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="off,scores,entropy")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"bench.Runner (single env) and the lockstep workload of bench.py's batched pass (generate_batch), bf16, 8-frame window, "
                       f"--steps {a.steps} --warmup {a.warmup}, one box, builds alternating {a.rounds}x, a fresh process per build",
           "config": a.config, "box": a.box, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, "off,scores")
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)
    modes = ([("off", "parent_build"), ("scores", "parent_build")] if a.ref_lib else []) + [(m, "this_build") for m in a.passes.split(",")]
    summary = {}
    for w in out["rounds"][0]["this_build"]:
        def col(build, mode, f):
            return [f(r[build][w][mode]) for r in out["rounds"] if mode in r.get(build, {}).get(w, {})]
        best = {f"{m} ({b})": max(col(b, m, lambda r: r["action_steps_per_s"])) for m, b in modes if col(b, m, lambda r: 0)}
        base, sbase = best.get("off (parent_build)"), best.get("scores (parent_build)")
        summary[w] = {
            "action_steps_per_s_best": best,
            "vs_parent_off_percent": {k: round(100.0 * (v / base - 1.0), 2) for k, v in best.items()} if base else None,
            "vs_parent_scores_percent": {k: round(100.0 * (v / sbase - 1.0), 2) for k, v in best.items() if not k.startswith("off")} if sbase else None,
            "decode_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["decode"])) for m, b in modes
                                              if col(b, m, lambda r: 0)},
            "ids_equal_plain_run_every_timed_turn": {m: all(all(x) for x in col("this_build", m, lambda r: r["ids_equal_plain_run_per_timed_turn"]))
                                                     for m in a.passes.split(",") if col("this_build", m, lambda r: 0)},
            "entropies_ok": all(col("this_build", "entropy", lambda r: r["every_id_has_a_finite_entropy"] and r.get("token_logprobs_bits_equal_scored_pass", True)))}
    out["summary"] = summary
    print(json.dumps(out))


if __name__ == "__main__":
    main()
