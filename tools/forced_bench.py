#!/usr/bin/env python
"""What a forced turn (generate(forced_ids=F): log-probabilities of given ids in one prefill pass, no decode phase) costs, on the headline
workload (bench.Runner: frames in, action ids out, 8-frame window, decode graph on, bf16, one env), one box, one process per build:

    python tools/forced_bench.py [--steps 20 --warmup 5] [--ref-lib build_ab/libA.so] [--rounds 2]

Passes (every turn has bench.DECODE_TOKENS = 5 ids; the same seeded episode in all of them):
  plain      greedy turns, every opt-in switch off                          -- regression yardstick: this build against --ref-lib
  scored     greedy turns with set_token_scores on                          -- the cheapest existing way to get n log-probabilities out of a
                                                                               turn; the yardstick of the gain, on both builds
  forced     forced turns with F = the ids the scored pass recorded         -- this build only
Per pass: turns/s, action-steps/s (bench.NUM_FUTURE per turn), ms per turn, phase_ms_per_turn (svln_phase_times: vision / prefill /
decode; a forced turn's prefill phase includes its head, and it has no decode phase).

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its passes run in a child process of their own, alternating with this build's `--rounds` times; the best round counts.  The
parent process never opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/forced_turn.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats -M --output-format csv -d out -- python tools/forced_bench.py --child --passes scored,forced --steps 10 --warmup 3
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "FORCED_BENCH_CHILD "


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
    from streamvln_amd.agent import StreamingAgent
    from streamvln_amd.config import CONFIGS
    from streamvln_amd.model import StreamVLNForCausalLM
    from streamvln_amd.synthetic import SyntheticPromptEncoder
    cfg = CONFIGS[a.config]
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=1, max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h
    recorded = []

    class ForcedAgent(StreamingAgent):
        """turn k of the pass is forced onto the ids turn k of the scored pass emitted"""
        turn_no = 0

        def _turn(self, instruction, env_id=None, forced_ids=None):
            req = dict(self._build_request(instruction, env_id), forced_ids=recorded[self.turn_no])
            self.turn_no += 1
            return self._consume(self.model.generate(**req))

    def agent(cls=StreamingAgent):
        return cls(model, SyntheticPromptEncoder(cfg, seed=7), num_frames=bench.NUM_FRAMES, num_future_steps=bench.NUM_FUTURE,
                   num_history=bench.NUM_HISTORY, env_id=0, device="cuda", max_new_tokens=bench.DECODE_TOKENS, eos_token_ids=(),
                   preprocess=run.preprocess)

    def measure(ag, record):
        """one pass over the seeded episode: warm-up turns (graphs captured, caches warm), then the timed turns"""
        ag.reset_memory()
        ag.prompt_encoder.reset()
        step = [0]

        def turn():
            n0 = len(ag.turn_log)
            while len(ag.turn_log) == n0:
                if step[0] == bench.EP_STEPS:
                    ag.reset_memory()
                    step[0] = 0
                ag.act(step[0])
                step[0] += 1
            if record:
                recorded.append(ag.turn_log[-1]["out"].sequences[0].tolist())
            ag.turn_log[:] = ag.turn_log[-1:]
        for _ in range(a.warmup):
            turn()
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        dt = bench.timed_pass(model, turn, a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        return {"turns_per_s": round(a.steps / dt, 3), "action_steps_per_s": round(bench.NUM_FUTURE * a.steps / dt, 2),
                "ms_per_turn": round(dt / a.steps * 1e3, 3),
                "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)}}

    res = {}
    for name in a.passes.split(","):
        model.reset(1)
        model.set_token_scores(name == "scored")
        if name in ("plain", "scored"):
            del recorded[:]
            res[name] = measure(agent(), name == "scored")
        elif name == "forced":
            if not recorded:
                raise SystemExit("the forced pass follows the scored pass of the same child: it replays its ids")
            ag = agent(ForcedAgent)
            res[name] = measure(ag, False)
            out = ag.turn_log[-1]["out"]
            res[name]["greedy_equals_forced_in_the_last_turn"] = bool(out.greedy_ids.tolist() == out.sequences.tolist())
            res[name]["last_turn_logprob"] = round(float(out.token_logprobs.sum()), 4)
        else:
            raise SystemExit(f"unknown pass {name!r}")
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
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick of the passes it can run")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default=None, help="(child) comma separated pass names")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    import bench
    out = {"workload": f"bench.Runner frames and prompts, one env, bf16, 8-frame window, decode graph on, {a.steps} timed turns after {a.warmup}, "
                       f"{bench.DECODE_TOKENS} ids per turn, one box, builds alternating {a.rounds}x, a fresh process per build, best round counts",
           "config": a.config, "box": a.box, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, "plain,scored")
        rnd["this_build"] = spawn(a, None, "plain,scored,forced")
        out["rounds"].append(rnd)

    def best(build, name):
        rows = [r[build][name] for r in out["rounds"] if name in r.get(build, {})]
        return max(rows, key=lambda r: r["turns_per_s"]) if rows else None

    summary = {}
    for name in ("plain", "scored"):
        mine, par = best("this_build", name), best("parent_build", name)
        summary[f"{name}_unused_vs_parent"] = {"this_build": mine, "parent_build": par,
                                               "percent": round(100.0 * (mine["turns_per_s"] / par["turns_per_s"] - 1.0), 2) if par else None}
    forced = best("this_build", "forced")
    yard = max((r for r in (best("parent_build", "scored"), best("this_build", "scored")) if r), key=lambda r: r["turns_per_s"])
    summary["forced_vs_best_scored"] = {"forced": forced, "scored_yardstick": yard,
                                        "percent": round(100.0 * (forced["turns_per_s"] / yard["turns_per_s"] - 1.0), 1)}
    out["summary"] = summary
    print(json.dumps(out))


if __name__ == "__main__":
    main()
