#!/usr/bin/env python
"""The MXFP4 decode mode next to bf16 and the e4m3 decode mode on the headline workload (bench.Runner: frames in, action ids out, 8-frame
window, decode graph on), one box, one process per build:

    python tools/mxfp4_bench.py [--steps 20 --warmup 5] [--ref-lib build_ab/libA.so] [--rounds 2]

Per mode (bf16, svln_set_fp8_decode, svln_set_mxfp4_decode) a pass reports action-steps/s, phase_ms_per_turn (svln_phase_times), the
layer-0 gate/up GEMV's time and weight bytes per launch (svln_probe_read; the kernel's own begin / end timestamps) and, from a 3-turn
episode on the SAME prompt stream as the bf16 pass (the prompt encoder is reset between passes), the relative L2 of the hidden rows that
saw identical inputs.

--ref-lib: the library of ANOTHER build of the engine (tools/build_ref_lib.sh <commit>), so that the code under test is not its own
yardstick: its passes (--ref-passes, default bf16,fp8: the parent of the MXFP4 change had no third mode) run in a child process of their own, alternating with this build's passes `--rounds` times.  The
parent process never opens the GPU; every child runs under its own time limit, and nothing is started after a child that failed.
Prints ONE JSON line (committed as profiles/mxfp4_decode.json).

    python tools/mxfp4_bench.py --batched 2,4,8 [--steps 10 --warmup 3] [--ref-lib build_ab/libA.so] [--rounds 2]

The lockstep multi-env workload instead (bench.py's batched pass: that many envs through generate_batch, 8-frame window, batched decode
graph on): per env count a pass with bf16 weights, one with svln_set_mxfp4_batched and one with svln_set_fp8_gemm, reporting
action-steps/s and phase_ms_per_turn; the --ref-lib build runs its bf16 and fp8_gemm passes as the yardstick, alternating as above.
--gate-up-trace FILE adds the per-launch time of the gate/up product from the kernel statistics of one `rocprofv3 --kernel-trace --stats`
run of `--batched 8 --rounds 1` (its *_kernel_stats.csv).  Committed as profiles/mxfp4_batched.json.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8000.0          # GB/s, MI355X specification


def child(a):
    import numpy as np
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
    I, H = cfg.inter, cfg.hidden
    weight_bytes = {"bf16": 2.0 * I * H * 2, "fp8": 2.0 * I * H + 2.0 * I * 4, "mxfp4": 2.0 * I * (H // 2) + 2.0 * I * (H // 32)}
    setters = {"bf16": lambda on: None, "fp8": model.set_fp8_decode, "mxfp4": getattr(model, "set_mxfp4_decode", None)}

    def restart():
        run.agent.reset_memory(); run.step = 0
        run.agent.prompt_encoder.reset()          # every pass sees the same prompt stream

    def short_episode(n=3):
        restart()
        out = []
        for _ in range(n):
            run.turn()
            out.append((run.agent.turn_log[-1]["out"].sequences[0].tolist(), model.last_hidden()))
        return out

    res, ref = {}, None
    for mode in a.passes.split(","):
        setters[mode](True)
        restart()
        for _ in range(a.warmup):
            run.turn()
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
        _lib.check(lib.svln_probe_reset(h))
        dt = bench.timed_pass(model, run.turn, a.steps, 0, 1)
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(lib.svln_probe_read(h, C.byref(ms), C.byref(n), C.byref(by)))
        r = {"action_steps_per_s": round(bench.NUM_FUTURE * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
             "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)}}
        if n.value:
            us = ms.value / n.value * 1e3
            gbs = weight_bytes[mode] / (us * 1e-6) / 1e9
            r["gate_up_gemv"] = {"avg_us": round(us, 2), "launches_timed": n.value, "weight_bytes_per_launch": weight_bytes[mode],
                                 "engine_probe_bytes": by.value, "GB_per_s": round(gbs, 1), "frac_of_8TBps": round(gbs / HBM_PEAK, 4)}
        ep = short_episode()
        if mode == "bf16":
            ref = ep
        elif ref is not None:
            per_turn, agree, total = [], 0, 0
            for (ia, ha), (ib, hb) in zip(ref, ep):
                k = 0
                while k < min(len(ia), len(ib)) and ia[k] == ib[k]:
                    k += 1
                agree += k; total += len(ia)
                rows = min(k + 1, len(ha), len(hb))        # rows 0 .. k saw identical inputs
                per_turn.append([round(float(np.linalg.norm(hb[j] - ha[j]) / np.linalg.norm(ha[j])), 4) for j in range(rows)])
                if k < len(ia):
                    break                                  # later turns carry a different token history
            r["vs_bf16_same_prompts"] = {"hidden_rel_l2_rows_with_identical_inputs": per_turn, "ids_equal_before_first_divergence": f"{agree}/{total}"}
        setters[mode](False)
        res[mode] = r
    model.close()
    print("MXFP4_BENCH_CHILD " + json.dumps(res), flush=True)


def child_batched(a):
    """the lockstep multi-env workload of bench.py's batched pass, per env count and mode"""
    import torch
    from streamvln_amd import _lib
    if os.environ.get("SVLN_LIB"):
        lib0 = C.CDLL(_lib.LIB_PATH)
        for name in list(_lib.SIGNATURES):
            if not hasattr(lib0, name):           # an older build lacks the entry points added since: this tool (only) drops them
                _lib.SIGNATURES.pop(name)
    import bench
    from streamvln_amd.agent import BatchedAgents, StreamingAgent
    from streamvln_amd.config import CONFIGS
    from streamvln_amd.model import StreamVLNForCausalLM
    from streamvln_amd.synthetic import SyntheticPromptEncoder
    cfg = CONFIGS[a.config]
    counts = [int(x) for x in a.batched.split(",")]
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=max(counts), max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h
    setters = {"bf16": lambda on: None, "mxfp4_batched": getattr(model, "set_mxfp4_batched", None), "fp8_gemm": model.set_fp8_gemm}
    res = {}
    for n in counts:
        for mode in a.passes.split(","):
            setters[mode](True)
            model.reset(n)
            agents = [StreamingAgent(model, SyntheticPromptEncoder(cfg, seed=7 + 31 * e), num_frames=bench.NUM_FRAMES, num_future_steps=bench.NUM_FUTURE,
                                     num_history=bench.NUM_HISTORY, env_id=e, device="cuda", max_new_tokens=bench.DECODE_TOKENS, eos_token_ids=(),
                                     preprocess=run.preprocess) for e in range(n)]
            group = BatchedAgents(agents)
            bstep = [0]

            def lockstep_turn():
                n0 = len(agents[0].turn_log)
                while len(agents[0].turn_log) == n0:
                    if bstep[0] == bench.EP_STEPS:
                        for ag in agents:
                            ag.reset_memory()
                        bstep[0] = 0
                    group.act([(bstep[0] + 7 * e) % bench.EP_STEPS for e in range(n)])
                    bstep[0] += 1
                for ag in agents:
                    ag.turn_log[:] = ag.turn_log[-1:]
            for _ in range(a.warmup):
                lockstep_turn()
            d3 = [C.c_double() for _ in range(3)]
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1))
            dt = bench.timed_pass(model, lockstep_turn, a.steps, 0, 1)
            _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0))
            res[f"{mode}@{n}"] = {"action_steps_per_s": round(bench.NUM_FUTURE * n * a.steps / dt, 2), "ms_per_lockstep_turn": round(dt / a.steps * 1e3, 3),
                                  "phase_ms_per_turn": {k: round(v.value / a.steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)}}
            setters[mode](False)
    model.close()
    print("MXFP4_BENCH_CHILD " + json.dumps(res), flush=True)


def gate_up_from_trace(path, cfg_name):
    """per-launch time of the batched gate/up product (gemv_mx4b_kernel, EPI_SWIGLU = 3, 4 waves on K) from a rocprofv3 kernel-stats CSV"""
    import csv
    from streamvln_amd.config import CONFIGS
    cfg = CONFIGS[cfg_name]
    out = {"weight_bytes_per_launch": 2.0 * cfg.inter * (cfg.hidden // 2) + 2.0 * cfg.inter * (cfg.hidden // 32), "source": os.path.basename(path)}
    with open(path) as f:
        for row in csv.DictReader(f):
            if any(t in row.get("Name", "") for t in ("gemv_mx4b_kernel<3, 4>", "gemv_mx4b_kernelILi3ELi4E")):
                us = float(row["AverageNs"]) / 1e3
                out.update({"kernel": row["Name"], "calls": int(row["Calls"]), "avg_us": round(us, 2),
                            "GB_per_s": round(out["weight_bytes_per_launch"] / (us * 1e-6) / 1e9, 1)})
    return out


def spawn(a, lib, passes):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--config", a.config] + (["--batched", a.batched] if a.batched else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)      # a fresh process per build, under its own limit
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child ({lib or 'this build'}) ended with status {p.returncode}: nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("MXFP4_BENCH_CHILD ")][-1]
    sys.stderr.write(f"child ({lib or 'this build'}: {passes}) done\n"); sys.stderr.flush()
    return json.loads(line[len("MXFP4_BENCH_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of another build (tools/build_ref_lib.sh): the yardstick for bf16 and e4m3")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="bf16,fp8,mxfp4")
    ap.add_argument("--ref-passes", default="bf16,fp8", help="passes of the --ref-lib build (a build older than the MXFP4 mode has only bf16,fp8)")
    ap.add_argument("--batched", default=None, help="env counts, e.g. 2,4,8: measure the lockstep multi-env workload instead (see above)")
    ap.add_argument("--gate-up-trace", default=None, help="a rocprofv3 *_kernel_stats.csv of a --batched 8 run: adds the gate/up product's per-launch time")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.batched and a.passes == "bf16,fp8,mxfp4":
        a.passes, a.ref_passes = "bf16,mxfp4_batched,fp8_gemm", "bf16,fp8_gemm"
    if a.child:
        return child_batched(a) if a.batched else child(a)
    if a.batched:
        out = {"workload": f"bench.py's batched pass: N envs in lockstep through generate_batch, --steps {a.steps} --warmup {a.warmup}, 8-frame window, "
                           f"batched decode graph on, one box, builds alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box,
               "rounds": []}
        for _ in range(a.rounds):
            rnd = {}
            if a.ref_lib:
                rnd["parent_build"] = spawn(a, a.ref_lib, a.ref_passes)
            rnd["this_build"] = spawn(a, None, a.passes)
            out["rounds"].append(rnd)
        keys = sorted({k for r in out["rounds"] for b in r.values() for k in b})
        out["summary_action_steps_per_s_best"] = {f"{k} ({b})": max(r[b][k]["action_steps_per_s"] for r in out["rounds"] if k in r.get(b, {}))
                                                  for k in keys for b in ("parent_build", "this_build") if any(k in r.get(b, {}) for r in out["rounds"])}
        if a.gate_up_trace:
            out["gate_up_B8_kernel_trace"] = gate_up_from_trace(a.gate_up_trace, a.config)
        print(json.dumps(out))
        return
    out = {"workload": f"bench.Runner headline workload, --steps {a.steps} --warmup {a.warmup}, 8-frame window, decode graph on, one box, "
                       f"builds alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box, "rounds": []}
    for _ in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, a.ref_passes)
        rnd["this_build"] = spawn(a, None, a.passes)
        out["rounds"].append(rnd)

    def best(build, mode, key):
        v = [r[build][mode][key] for r in out["rounds"] if build in r and mode in r[build]]
        return max(v) if v else None
    def decode_ms(build, mode):
        v = [r[build][mode]["phase_ms_per_turn"]["decode"] for r in out["rounds"] if build in r and mode in r[build]]
        return min(v) if v else None
    yard = "parent_build" if a.ref_lib else "this_build"
    out["summary"] = {
        "action_steps_per_s_best": {"bf16 (" + yard + ")": best(yard, "bf16", "action_steps_per_s"), "e4m3 (" + yard + ")": best(yard, "fp8", "action_steps_per_s"),
                                    "bf16 (this_build)": best("this_build", "bf16", "action_steps_per_s"),
                                    "e4m3 (this_build)": best("this_build", "fp8", "action_steps_per_s"),
                                    "mxfp4 (this_build)": best("this_build", "mxfp4", "action_steps_per_s")},
        "decode_phase_ms_per_turn_best": {"bf16 (" + yard + ")": decode_ms(yard, "bf16"), "e4m3 (" + yard + ")": decode_ms(yard, "fp8"),
                                          "mxfp4 (this_build)": decode_ms("this_build", "mxfp4")}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
