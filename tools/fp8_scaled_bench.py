#!/usr/bin/env python
"""The block-scaled e4m3 MFMA form (svln_set_fp8_scaled_mfma) next to the unscaled e4m3 products of svln_set_fp8_gemm, one box, one fresh
process per build:

    python tools/fp8_scaled_bench.py --ref-lib build_ab/libA.so [--rounds 2] [--batched 8,4] [--box NAME]

Yardstick = the library of the PARENT commit (tools/build_ref_lib.sh <commit>): its fp8_gemm passes are the baseline; the builds alternate
`--rounds` times.  The parent process never opens the GPU; every child runs under its own time limit and nothing is started after a child
that failed.  A child (one engine at full size, decode graph on) runs
  * bench.py's batched pass -- N envs in lockstep through generate_batch, --batched-steps 10 --batched-warmup 3 -- with fp8_gemm and, on this
    build, fp8_gemm + the scaled form: action-steps/s and phase_ms_per_turn;
  * the single-env headline workload (bench.Runner, --steps 20 --warmup 5) in the same modes: action-steps/s, phase_ms_per_turn and the
    turn_ms of the window-restart turns (T = 1952);
  * this build only: isolated launches of gate/up (SwiGLU, N = 37888, K = 3584) and down_proj (N = 3584, K = 18944) at M = 1696 and 1952 through
    svln_op_gemm_fp8 in five forms -- the planner's choice unscaled / scaled, and the 256x256 tile as stage ring unscaled, stage ring
    scaled and 8-phase scaled -- rotating over enough weight copies to miss the infinity cache; times are stream events around launch + sync
    (the host gap between the sync and the closing event, ~10 us, is in every form alike), median of --kernel-reps.
Prints ONE JSON line (committed as profiles/fp8_scaled.json).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = "FP8_SCALED_BENCH_CHILD "
SCALED, RING = 0x40000, 0x4000


def child(a):
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
    counts = [int(x) for x in a.batched.split(",")] if a.batched else []
    model = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, device=0, max_envs=max(counts + [1]), max_frames=1 + bench.NUM_HISTORY)
    model.load_synthetic(1234)
    model.model.num_history = bench.NUM_HISTORY
    model.set_decode_graph(True)
    run = bench.Runner(model, cfg, 0)
    torch.cuda.set_stream(model.torch_stream)
    lib, h = model._lib, model._h
    has_switch = "svln_set_fp8_scaled_mfma" in _lib.SIGNATURES

    def set_mode(mode, on):
        model.set_fp8_gemm(on)
        if mode == "fp8_gemm_scaled":
            model.set_fp8_scaled_mfma(on)

    def phases(steps, reset):
        d3 = [C.c_double() for _ in range(3)]
        _lib.check(lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), int(reset)))
        return {k: round(v.value / steps, 3) for k, v in zip(("vision", "prefill", "decode"), d3)}

    modes = [m for m in a.passes.split(",") if m != "fp8_gemm_scaled" or has_switch]
    res = {}
    for n in counts:
        for mode in modes:
            set_mode(mode, True)
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
            for _ in range(a.batched_warmup):
                lockstep_turn()
            phases(1, True)
            dt = bench.timed_pass(model, lockstep_turn, a.batched_steps, 0, 1)
            res[f"{mode}@{n}"] = {"action_steps_per_s": round(bench.NUM_FUTURE * n * a.batched_steps / dt, 2),
                                  "ms_per_lockstep_turn": round(dt / a.batched_steps * 1e3, 3), "phase_ms_per_turn": phases(a.batched_steps, False)}
            set_mode(mode, False)
    if a.steps > 0:
        model.reset(1)
        for mode in modes:
            set_mode(mode, True)
            run.agent.reset_memory(); run.step = 0
            run.agent.prompt_encoder.reset()          # every pass sees the same prompt stream
            for _ in range(a.warmup):
                run.turn()
            phases(1, True)
            lat = []
            dt = bench.timed_pass(model, run.turn, a.steps, 0, 1, lat)
            per_episode = bench.EP_STEPS // bench.NUM_FUTURE
            restart = [round(x * 1e3, 2) for i, x in enumerate(lat) if (a.warmup + i) % per_episode == per_episode // 2]
            res[f"{mode}@single"] = {"action_steps_per_s": round(bench.NUM_FUTURE * a.steps / dt, 2), "ms_per_turn": round(dt / a.steps * 1e3, 3),
                                     "phase_ms_per_turn": phases(a.steps, False), "turn_ms_window_restart": restart}
            set_mode(mode, False)
    if a.kernels and has_switch:
        res["kernels_us"] = kernels(a, model, torch, _lib)
    model.close()
    print(TAG + json.dumps(res), flush=True)


def kernels(a, model, torch, _lib):
    lib, h = model._lib, model._h
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    forms = {"planner_unscaled": 0, "planner_scaled": SCALED, "ring256_unscaled": 256, "ring256_scaled": 256 | RING | SCALED, "p8_scaled": 256 | SCALED}
    out = {}
    g = torch.Generator(device="cuda").manual_seed(5)
    rand8 = lambda r, c: torch.randint(0, 0x7E, (r, c), dtype=torch.uint8, device="cuda", generator=g) | (torch.randint(0, 2, (r, c), dtype=torch.uint8, device="cuda", generator=g) << 7)
    for name, N, K, epi in (("gate_up", 37888, 3584, _lib.EPI_SWIGLU), ("down_proj", 3584, 18944, _lib.EPI_NONE)):
        nw = max(1, min(8, -(-768 * 2 ** 20 // (N * K))))
        Ws = [rand8(N, K) for _ in range(nw)]
        sw = torch.rand(N, device="cuda") * 1e-4 + 1e-5
        for M in (1696, 1952):
            A, sa = rand8(M, K), torch.rand(M, device="cuda") * 1e-4 + 1e-5
            Cn = N // 2 if epi == _lib.EPI_SWIGLU else N
            Cm = torch.zeros(M, Cn, device="cuda", dtype=torch.bfloat16)
            for form, fc in forms.items():
                tile = _lib.GEMM_TILES[_lib.gemm_plan(dtype=_lib.SVLN_BF16, epi=epi, M=M, N=N, K=K, fp8=1, has_ws=1, ws_elems=1 << 30, has_zeros=1, force_cfg=fc).launch[0].tile]
                us = []
                for i in range(a.kernel_reps + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    _lib.check(lib.svln_op_gemm_fp8(h, ptr(A), ptr(sa), K, ptr(Ws[i % nw]), ptr(sw), K, ptr(Cm), Cn, None, None, 0, M, N, K, epi, fc, 0))
                    e1.record()
                    e1.synchronize()
                    if i >= 2:
                        us.append(e0.elapsed_time(e1) * 1e3)
                out[f"{name}@M{M}/{form}"] = {"tile": tile, "median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1),
                                             "TFLOPs_at_median": round(2.0 * M * N * K / statistics.median(us) / 1e6, 1)}
        del Ws
    return out


def spawn(a, lib, passes, kernels_on):
    env = dict(os.environ)
    env.pop("SVLN_LIB", None)
    if lib:
        env["SVLN_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--passes", passes, "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--batched-steps", str(a.batched_steps), "--batched-warmup", str(a.batched_warmup), "--config", a.config, "--batched", a.batched,
           "--kernel-reps", str(a.kernel_reps)] + (["--kernels"] if kernels_on else [])
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
    ap.add_argument("--batched", default="8,4")
    ap.add_argument("--batched-steps", type=int, default=10)
    ap.add_argument("--batched-warmup", type=int, default=3)
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--ref-lib", default=None, help="library of the parent commit (tools/build_ref_lib.sh): the baseline")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--passes", default="fp8_gemm,fp8_gemm_scaled")
    ap.add_argument("--kernels", action="store_true", help="(child) also time the isolated launches")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--box", default=None, help="free text naming the box the run was made on")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"workload": f"fp8_gemm with the e4m3 MFMA form off / on: bench.py's batched pass ({a.batched} envs in lockstep, --steps {a.batched_steps} --warmup "
                       f"{a.batched_warmup}) and the single-env headline workload (--steps {a.steps} --warmup {a.warmup}), 8-frame window, decode graph on, one box, "
                       f"builds alternating {a.rounds}x, a fresh process per build", "config": a.config, "box": a.box,
           "baseline": "parent_build fp8_gemm (the parent commit's library)", "rounds": []}
    for r in range(a.rounds):
        rnd = {}
        if a.ref_lib:
            rnd["parent_build"] = spawn(a, a.ref_lib, "fp8_gemm", False)
        rnd["this_build"] = spawn(a, None, a.passes, r == 0 and not a.no_kernels)
        out["rounds"].append(rnd)
    keys = sorted({k for r in out["rounds"] for b in r.values() for k in b if k != "kernels_us"})
    out["summary_action_steps_per_s_best"] = {f"{k} ({b})": max(r[b][k]["action_steps_per_s"] for r in out["rounds"] if k in r.get(b, {}))
                                              for k in keys for b in ("parent_build", "this_build") if any(k in r.get(b, {}) for r in out["rounds"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
