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
        for name in ("svln_set_mxfp4_decode", "svln_op_quant_mxfp4", "svln_op_gemv_mxfp4"):
            if not hasattr(lib0, name):
                _lib.SIGNATURES.pop(name, None)
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
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("MXFP4_BENCH_CHILD ")][-1]
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
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
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
