#!/usr/bin/env python
"""What truncated sampling (svln_sampling_truncation: top-k / top-p over the lm_head's candidate lists) costs, on the headline workload
(bench.Runner: frames in, action ids out, 8-frame window, decode graph on, bf16, single env) and on the lockstep workload of bench.py's
batched pass (N envs through generate_batch: the MFMA head at 8 envs), one box, one process per build:

    python tools/trunc_bench.py [--steps 20 --warmup 5] [--envs 8] [--ref-lib build_ab/libA.so] [--rounds 2] [--temperature 1.0]

Passes, every one over the SAME seeded episode (agent memories, frame streams, prompt encoders and the draw counters are reset between
passes; turns have a fixed length, so every pass does the same number of head passes):
  sampled   generate(do_sample=True), truncation off.  The --ref-lib build runs this pass too: it is the yardstick, and this build's pass
            must sit inside the box-to-box spread of it (the launches are the same);
  k8p1      set_sampling_truncation(8, 1.0): the EPI_SAMPLE_TOPK form of every lm_head product, truncate_partials_kernel, the final
            kernel on 8 partials;
  k4p09     set_sampling_truncation(4, 0.9).
A pass is run twice over the episode (the recording run and the timed run): its ids must repeat.
Per pass, for the single env and for each env count: action-steps/s, ms per turn, phase_ms_per_turn (svln_phase_times).

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its pass runs in a child process of its own, alternating with this build's passes `--rounds` times.  The parent process never
opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/truncated_sampling.json).  Per-launch kernel times come from a run of two passes under the profiler:
    rocprofv3 --kernel-trace --stats -M --output-format csv -d out -- python tools/trunc_bench.py --child --passes sampled,k8p1 --steps 10 --warmup 3
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "TRUNC_BENCH_CHILD "
TRUNC = {"sampled": (None, None), "k8p1": (8, 1.0), "k4p09": (4, 0.9)}
SEED = 20261019


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
    env_counts = [int(x) for x in a.envs.split(",") if x]
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=max(env_counts + [1]), max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h
    if ref and not hasattr(lib, "svln_sampling_truncation"):
        lib.svln_sampling_truncation = lambda *args: 0            # the parent build: the off setting is all this tool asks of it

    def measure(agents, restart, turn, per_turn_actions):
        """-> {pass: result}; turn() returns (ids per env, token_logprobs per env or None)"""
        total = a.warmup + a.steps
        out = {}
        for mode in a.passes.split(","):
            for ag in agents:
                ag.do_sample, ag.temperature = True, a.temperature
            model.sampling_seed = SEED
            k, p = TRUNC[mode]

            def begin():
                restart()
                model.set_sampling_truncation(k, p)
                model.set_sampling(a.temperature, SEED)        # (restarts the draw counters: the passes see the same noise)
            begin()
            plain = [turn()[0] for _ in range(total)]      # the recording run (also the warm-up: graphs captured, caches warm)
            begin()
            got = [turn() for _ in range(a.warmup)]
            d3 = [C.c_double() for _ in range(3)]
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
            dt = bench.timed_pass(model, lambda: got.append(turn()), a.steps, 0, 1)
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
            timed = got[a.warmup:]
            r = {"action_steps_per_s": round(per_turn_actions * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
                 "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)},
                 "ids_repeat_the_recording_run_per_timed_turn": [g[0] == p for g, p in zip(timed, plain[a.warmup:])]}
            out[mode] = r
        model.set_sampling(None)
        model.set_sampling_truncation()
        return out

    res = {}
    if a.single:
        def restart1():
            run.agent.reset_memory(); run.step = 0
            run.agent.prompt_encoder.reset()

        def turn1():
            run.turn()
            o = run.agent.turn_log[-1]["out"]
            return [o.sequences[0].tolist()], [o.get("token_logprobs")]
        res["1"] = measure([run.agent], restart1, turn1, bench.NUM_FUTURE)
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
            return [o.sequences[0].tolist() for o in outs], [o.get("token_logprobs") for o in outs]
        res[f"{n} lockstep"] = measure(agents, restart, lockstep_turn, bench.NUM_FUTURE * n)
    model.close()
    print(TAG + json.dumps(res), flush=True)


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--config", a.config, "--envs", a.envs, "--temperature", str(a.temperature)] + ([] if a.single else ["--no-single"])
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
    ap.add_argument("--envs", default="8", help="env counts of the lockstep workload (comma separated; empty = none)")
    ap.add_argument("--no-single", dest="single", action="store_false", help="skip the single-env workload")
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick for the switch-off pass")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="sampled,k8p1,k4p09")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"bench.Runner (single env) and the lockstep workload of bench.py's batched pass (generate_batch), bf16, 8-frame window, "
                       f"--steps {a.steps} --warmup {a.warmup}, temperature {a.temperature}, one box, builds alternating {a.rounds}x, a fresh process per build",
           "config": a.config, "box": a.box, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, "sampled")
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)
    modes = ([("sampled", "parent_build")] if a.ref_lib else []) + [(m, "this_build") for m in a.passes.split(",")]
    summary = {}
    for w in out["rounds"][0]["this_build"]:
        def col(build, mode, f):
            return [f(r[build][w][mode]) for r in out["rounds"] if mode in r.get(build, {}).get(w, {})]
        best = {f"{m} ({b})": max(col(b, m, lambda r: r["action_steps_per_s"])) for m, b in modes}
        base = best.get("sampled (parent_build)")
        summary[w] = {
            "action_steps_per_s_best": best,
            "vs_parent_sampled_percent": {k: round(100.0 * (v / base - 1.0), 2) for k, v in best.items()} if base else None,
            "decode_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["decode"])) for m, b in modes},
            "prefill_phase_ms_per_turn_best": {f"{m} ({b})": min(col(b, m, lambda r: r["phase_ms_per_turn"]["prefill"])) for m, b in modes},
            "ids_repeat_the_recording_run_every_timed_turn": {m: all(all(x) for x in col("this_build", m, lambda r: r["ids_repeat_the_recording_run_per_timed_turn"]))
                                                     for m in a.passes.split(",")}}
    out["summary"] = summary
    print(json.dumps(out))


if __name__ == "__main__":
    main()
