#!/usr/bin/env python
"""Candidate scoring (generate(candidate_ids=...) / svln_turn_candidates) next to the only way that existed before it, on bench.py's
workload (bf16, 8-frame window, 5-id turns), one box, one process per build:

    python tools/candidates_bench.py [--groups 2,4,8] [--steps 10 --warmup 3] [--ref-lib build_ab/libA.so] [--rounds 2]

Every pass runs the SAME seeded episode (agent memories, frame streams and prompt encoders are reset between passes).  Candidate 0 of turn
t is what a first plain run of the episode emitted at turn t, candidate g >= 1 the same ids with the last one replaced; the env goes on
with candidate 0, so every pass leaves it where the plain run does.
  single         the feature unused: bench.py's single-env turn (both builds: must agree inside the box-to-box spread);
  plain8         the feature unused: generate_batch on 8 envs (both builds);
  replicated     G envs fed the same frames and the same prompt, env g forced onto candidate g by ONE generate_batch_forced call: the
                 yardstick, the vision tower and the prefill G times (both builds; the parent's figure is the one to beat);
  candidates     ONE candidates call on ONE env (both builds, where the build exports it: the parent's figure is the one `folded` is
                 held against);
  folded         the same call with fold_candidates (svln_turn_candidates_folded; this build): the candidates' rows ride the prefill.
Per pass and G: scored sequences/s, ms per model turn, phase_ms_per_turn (svln_phase_times; a candidates call books its prefill under
`prefill` and its scoring passes + head under `decode`).

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its passes run in a child process of their own, alternating with this build's `--rounds` times.  The parent process never
opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/candidates.json; the run with the folded pass as profiles/candidates_fold.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/candidates_bench.py --child --passes folded --groups 8
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "CANDIDATES_BENCH_CHILD "
BOTH = ("single", "plain8", "replicated", "candidates")
NEW = ("folded",)


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
    groups = [int(x) for x in a.groups.split(",")]
    passes = a.passes.split(",")
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=8, max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h
    res = {}

    def measure(turn_fn, sequences_per_turn):
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        dt = bench.timed_pass(model, turn_fn, a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        return {"sequences_per_s": round(sequences_per_turn * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
                "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)}}

    def make_agents(n, same):
        return [StreamingAgent(model, SyntheticPromptEncoder(cfg, seed=7 if same else 7 + 31 * e), num_frames=bench.NUM_FRAMES,
                               num_future_steps=bench.NUM_FUTURE, num_history=bench.NUM_HISTORY, env_id=e, device="cuda",
                               max_new_tokens=bench.DECODE_TOKENS, eos_token_ids=(), preprocess=run.preprocess) for e in range(n)]

    def driver(agents, step_fn, shift):
        """bench.py's loop for `agents` stepped together: step_fn(frames, turn index) runs one env step of all of them"""
        state = {"step": 0, "turn": 0}

        def restart():
            for ag in agents:
                ag.reset_memory()
                ag.prompt_encoder.reset()
            state["step"], state["turn"] = 0, 0

        def turn():
            n0 = len(agents[0].turn_log)
            while len(agents[0].turn_log) == n0:
                if state["step"] == bench.EP_STEPS:
                    for ag in agents:
                        ag.reset_memory()
                    state["step"] = 0
                step_fn([(state["step"] + shift * e) % bench.EP_STEPS for e in range(len(agents))], state["turn"])
                state["step"] += 1
            state["turn"] += 1
            ids = [ag.turn_log[-1]["out"].sequences[0].tolist() for ag in agents]
            for ag in agents:
                ag.turn_log[:] = ag.turn_log[-1:]
            return ids
        return restart, turn

    total = a.warmup + a.steps
    # the recording run: one env, plain turns (also the warm-up of the process)
    model.reset(1)
    one = make_agents(1, True)
    restart, turn = driver(one, lambda frames, t: one[0].act(frames[0]), 0)
    restart()
    plain = [turn()[0] for _ in range(total)]

    def cands(t, G):
        F = plain[t]
        return [F] + [F[:-1] + [(F[-1] + 17 * g) % cfg.vocab] for g in range(1, G)]

    if "single" in passes:
        restart()
        for _ in range(a.warmup):
            turn()
        res["single"] = measure(turn, 1)
    if "plain8" in passes:
        model.reset(8)
        ags = make_agents(8, False)
        grp = BatchedAgents(ags)
        restart8, turn8 = driver(ags, lambda frames, t: grp.act(frames), 7)
        restart8()
        for _ in range(a.warmup):
            turn8()
        res["plain8"] = measure(turn8, 8)
    for G in groups:
        res[str(G)] = {}
        if "replicated" in passes:
            model.reset(G)
            ags = make_agents(G, True)
            grp = BatchedAgents(ags)

            def step_rep(frames, t, ags=ags, grp=grp, G=G):
                due = len(ags[0].action_seq) == 0
                grp.act(frames, forced_ids=cands(t, G) if due else None)
            restart_r, turn_r = driver(ags, step_rep, 0)
            restart_r()
            got = [turn_r() for _ in range(a.warmup)]
            r = measure(lambda: got.append(turn_r()), G)
            r["ids_are_the_candidates_per_timed_turn"] = [g == cands(a.warmup + k, G) for k, g in enumerate(got[a.warmup:])]
            res[str(G)]["replicated"] = r
        for mode, fold in (("candidates", False), ("folded", True)):
            if mode not in passes or (fold and ref) or not hasattr(lib, "svln_turn_candidates"):
                continue
            model.reset(1)
            ags = make_agents(1, True)
            ags[0].fold_candidates = fold

            def step_cand(frames, t, ag=ags[0], G=G):
                if len(ag.action_seq) == 0:
                    ag.act_candidates(frames[0], candidate_ids=cands(t, G), select=0)
                else:
                    ag.act(frames[0])
            restart_c, turn_c = driver(ags, step_cand, 0)
            restart_c()
            got = [turn_c() for _ in range(a.warmup)]
            r = measure(lambda: got.append(turn_c()), G)
            r["ids_equal_plain_run_per_timed_turn"] = [g[0] == plain[a.warmup + k] for k, g in enumerate(got[a.warmup:])]
            res[str(G)][mode] = r
    model.close()
    print(TAG + json.dumps(res), flush=True)


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--config", a.config, "--groups", a.groups]
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
    ap.add_argument("--groups", default="2,4,8", help="candidates per call / replicated envs")
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
    out = {"workload": f"bench.py's workload (bf16, 8-frame window, 5-id turns), --steps {a.steps} --warmup {a.warmup}, one box, builds "
                       f"alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box, "rounds": []}
    both = ",".join(p for p in a.passes.split(",") if p in BOTH)
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib and both:
            rnd["parent_build"] = spawn(a, a.ref_lib, both)
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)
    best = lambda col: max(col, key=lambda r: r["sequences_per_s"])
    summary = {}
    for build in ("parent_build", "this_build"):
        for key in ("single", "plain8"):
            col = [r[build][key] for r in out["rounds"] if key in r.get(build, {})]
            if col:
                summary[f"{key} ({build})"] = best(col)
        for G in a.groups.split(","):
            for mode in ("replicated", "candidates", "folded"):
                col = [r[build][G][mode] for r in out["rounds"] if mode in r.get(build, {}).get(G, {})]
                if col:
                    summary[f"G={G} {mode} ({build})"] = best(col)
    out["summary"] = summary
    print(json.dumps(out))


if __name__ == "__main__":
    main()
