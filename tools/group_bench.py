#!/usr/bin/env python
"""What a group turn (generate(do_sample=True, num_return_sequences=G) + select_sequence) costs and gains, on the headline workload
(bench.Runner: frames in, action ids out, 8-frame window, decode graph on, bf16), one box, one process per build:

    python tools/group_bench.py [--steps 20 --warmup 5] [--groups 2,4,8] [--ref-lib build_ab/libA.so] [--rounds 2] [--temperature 1.0]

Passes (every turn emits bench.DECODE_TOKENS ids per sequence; sampling on in all of them):
  single         one env, plain sampled turns                                    -- regression yardstick: this build against --ref-lib
  lockstep8      8 envs with their own frames and prompts through generate_batch -- regression yardstick
  replicated G   G envs fed the SAME frames and the SAME prompt through generate_batch: the only way to get G samples of a turn without
                 this change (vision and prefill are paid G times)               -- gain yardstick, on both builds
  group G        one env, one group turn of G sequences, then select_sequence(0) -- this build only
Per pass: turns/s, sequences/s (G x turns/s), ms per turn, phase_ms_per_turn (svln_phase_times: vision / prefill / decode; a group turn's
prefill phase includes its batched token-0 head and the page fork).

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its passes run in a child process of their own, alternating with this build's `--rounds` times.  The parent process never opens
the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/group_sampling.json).  Per-launch kernel times come from a run of one pass under the profiler:
    rocprofv3 --kernel-trace --stats -M --output-format csv -d out -- python tools/group_bench.py --child --passes group8 --steps 10 --warmup 3
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "GROUP_BENCH_CHILD "
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
    from streamvln_amd.model import GenerateOutput, StreamVLNForCausalLM
    from streamvln_amd.synthetic import SyntheticPromptEncoder
    cfg = CONFIGS[a.config]
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=8, max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h

    class GroupAgent(StreamingAgent):
        """every turn is a group turn of n_seq sequences; the env goes on with sequence 0"""
        n_seq = 2

        def _turn(self, instruction, env_id=None):
            out = self.model.generate(**dict(self._build_request(instruction, env_id), num_return_sequences=self.n_seq))
            n = int(out.sequence_lengths[0])
            kv = self.model.select_sequence(0, self.env_id)
            self.group_ids = out.sequences
            return self._consume(GenerateOutput(sequences=out.sequences[:1, :n], past_key_values=kv))

    def agent(e, seed, cls=StreamingAgent):
        return cls(model, SyntheticPromptEncoder(cfg, seed=seed), num_frames=bench.NUM_FRAMES, num_future_steps=bench.NUM_FUTURE,
                   num_history=bench.NUM_HISTORY, env_id=e, device="cuda", max_new_tokens=bench.DECODE_TOKENS, eos_token_ids=(),
                   preprocess=run.preprocess, do_sample=True, temperature=a.temperature)

    def measure(agents, frame_of, n_seq_total, batched):
        """one pass over the seeded episode: warm-up turns (graphs captured, caches warm), then the timed turns"""
        for ag in agents:
            ag.reset_memory()
            ag.prompt_encoder.reset()
        model.sampling_seed = SEED
        model.set_sampling(a.temperature, SEED)            # (restarts the draw counters: every pass sees the same noise)
        group = BatchedAgents(agents) if batched else None
        step = [0]

        def turn():
            n0 = len(agents[0].turn_log)
            while len(agents[0].turn_log) == n0:
                if step[0] == bench.EP_STEPS:
                    for ag in agents:
                        ag.reset_memory()
                    step[0] = 0
                if batched:
                    group.act([frame_of(e, step[0]) for e in range(len(agents))])
                else:
                    agents[0].act(frame_of(0, step[0]))
                step[0] += 1
            for ag in agents:
                ag.turn_log[:] = ag.turn_log[-1:]
        for _ in range(a.warmup):
            turn()
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        dt = bench.timed_pass(model, turn, a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        return {"turns_per_s": round(a.steps / dt, 3), "sequences_per_s": round(n_seq_total * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
                "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)}}

    res = {}
    for name in a.passes.split(","):
        model.reset(8)
        if name == "single":
            res[name] = measure([agent(0, 7)], lambda e, s: s, 1, False)
        elif name == "lockstep8":          # bench.py's batched pass: env e sees the stream shifted by 7 e frames, its own prompts
            res[name] = measure([agent(e, 7 + 31 * e) for e in range(8)], lambda e, s: (s + 7 * e) % bench.EP_STEPS, 8, True)
        elif name.startswith("replicated"):
            g = int(name[len("replicated"):])
            res[name] = measure([agent(e, 7) for e in range(g)], lambda e, s: s, g, True)
        elif name.startswith("group"):
            g = int(name[len("group"):])
            ag = agent(0, 7, GroupAgent)
            ag.n_seq = g
            res[name] = measure([ag], lambda e, s: s, g, False)
            res[name]["distinct_sequences_in_the_last_turn"] = len({tuple(r) for r in ag.group_ids.tolist()})
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
           "--config", a.config, "--temperature", str(a.temperature)]
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
    ap.add_argument("--groups", default="2,4,8")
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick of the passes it can run")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default=None, help="(child) comma separated pass names")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    groups = [int(x) for x in a.groups.split(",") if x]
    common = ["single", "lockstep8"] + [f"replicated{g}" for g in groups]
    mine = common + [f"group{g}" for g in groups]
    out = {"workload": f"bench.Runner frames and prompts, bf16, 8-frame window, decode graph on, {a.steps} timed turns after {a.warmup}, temperature "
                       f"{a.temperature}, {__import__('bench').DECODE_TOKENS} ids per sequence, one box, builds alternating {a.rounds}x, a fresh process per build",
           "config": a.config, "box": a.box, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, ",".join(common))
        rnd["this_build"] = spawn(a, None, ",".join(mine))
        out["rounds"].append(rnd)

    def best(build, name, key, pick=max):
        vals = [r[build][name][key] for r in out["rounds"] if name in r.get(build, {})]
        return pick(vals) if vals else None

    def phases(build, name):
        rows = [r[build][name]["phase_ms_per_turn"] for r in out["rounds"] if name in r.get(build, {})]
        return {k: min(x[k] for x in rows) for k in rows[0]} if rows else None
    summary = {"regression_vs_parent_percent": {}, "groups": {}}
    for name in common:
        mine_v, par = best("this_build", name, "sequences_per_s"), best("parent_build", name, "sequences_per_s")
        summary["regression_vs_parent_percent"][name] = {"this_build": mine_v, "parent_build": par,
                                                          "percent": round(100.0 * (mine_v / par - 1.0), 2) if par else None}
    for g in groups:
        grp, rep, rep_par = (best("this_build", f"group{g}", "sequences_per_s"), best("this_build", f"replicated{g}", "sequences_per_s"),
                             best("parent_build", f"replicated{g}", "sequences_per_s"))
        yard = max(v for v in (rep, rep_par) if v is not None)
        summary["groups"][str(g)] = {
            "group_sequences_per_s": grp, "replicated_sequences_per_s": {"this_build": rep, "parent_build": rep_par},
            "group_vs_best_replicated_percent": round(100.0 * (grp / yard - 1.0), 1),
            "ms_per_turn": {"group": best("this_build", f"group{g}", "ms_per_turn", min), "replicated": best("this_build", f"replicated{g}", "ms_per_turn", min),
                            "single": best("this_build", "single", "ms_per_turn", min)},
            "phase_ms_per_turn": {"group": phases("this_build", f"group{g}"), "replicated": phases("this_build", f"replicated{g}"),
                                  "single": phases("this_build", "single")}}
    out["summary"] = summary
    print(json.dumps(out))


if __name__ == "__main__":
    main()
