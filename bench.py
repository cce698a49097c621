#!/usr/bin/env python
"""bench.py -- action-steps/s of the StreamVLN streaming-inference hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W
  N > 1 either under a launcher (python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...: RANK /
  LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment), or as the plain command above: without RANK in the environment
  bench.py starts that launcher itself as a CHILD process (before anything here has touched the GPU), relays rank 0's JSON line and
  exits with the child's return code -- the reference's `torchrun --nproc_per_node=8 streamvln/streamvln_eval.py`
  (scripts/streamvln_eval_multi_gpu.sh:7) as one command.

Workload (BASELINE.json configs[1]): StreamVLN-Qwen-1.5 = SigLIP-so400m + Qwen2-7B at true
size, bf16, seeded random-init weights, synthetic 640x480 RGB stream, 8-frame window
(num_frames 32 / num_future_steps 4 / num_history 8), one env per GPU.  A "step" = one model turn
(new frame in -> 4 action tokens + EOS out = 4 environment actions): vision encode of the new frame
(9 frames at a window restart), splice, LLM prefill of the turn's tokens over the retained KV window, 5 greedy
decode steps.  Turns cycle through 64-env-step episodes: turn 0 = episode start (T=376), turns 1-7 steady
(T=212), turn 8 = window restart with the 8-frame <memory> block (T=1952, 9 ViT frames), turns 9-15 steady.
Frames enter as uint8 640x480 host arrays; every env step preprocesses its frame (upload + HIP bicubic resize, bit-exact with the
reference's PIL path) INSIDE the timed region, as the reference loop does (streamvln_eval.py:271-274); `value` = 4 * turns / time
over all ranks (frame in -> action ids out).  `generate_boundary` is the same run with the image-processor time taken out.

A plain run sets up, warms up, times the K steps and prints the JSON line.  `--full` adds everything else (their objects are null
without it):
  roofline      the gate/up SwiGLU GEMV of the decode step (largest single weight stream: 2*I*H*2 B = 271.6 MB per
                launch, HBM-bound); `achieved` = those bytes / its mean duration, measured live with HIP events
                on the engine's stream around the layer-0 launch of the first decode step of every turn in the timed region.
  with_feature_cache / fp8_decode_weights / memory_prune_32 / batched_envs
                the opt-in modes, each timed in a pass of its own after the headline pass.
  metric_allreduce_check
                the 5-scalar metric all-reduce of the eval loop on synthetic metrics.
  cpu_baseline  the CPU oracle (fp32 port of the reference path, torch CPU, all host threads) on a bounded sample of
                the same steady turn (rank 0, N = 1 only).
The --no-* options switch single parts of `--full` off.

--dump-outputs DIR writes what the last timed step returned (rank 0): DIR/sequences.npy (the turn's generated token ids, float64)
and DIR/hidden.npy (the final-norm hidden rows of those tokens, float32).  Weights, frames and prompts are seeded, so the same
arguments give the same inputs in every run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--config", default="streamvln_qwen2_7b")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-probe", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-feature-cache-pass", action="store_true")
    ap.add_argument("--no-batched-pass", action="store_true")
    ap.add_argument("--no-fp8-pass", action="store_true")
    ap.add_argument("--no-prune-pass", action="store_true")
    ap.add_argument("--batched-envs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--backend", default=None, help="torch.distributed backend (default nccl = RCCL); gloo for rehearsals")
    ap.add_argument("--single-device", action="store_true", help="rehearsal: every rank uses GPU 0 (needs --backend gloo)")
    ap.add_argument("--persistent-decode", action="store_true", help="decode step as attention + ONE persistent launch per layer (svln_set_decode_persistent; "
                    "measured slower than the six launches at this size, DESIGN.md 4.1: A/B only)")
    ap.add_argument("--pageable-frames", action="store_true", help="camera frames in ordinary numpy arrays instead of the engine's pinned frame ring")
    ap.add_argument("--own-torch-stream", action="store_true", help="leave torch on its default stream (cross-stream ordering per frame / turn) instead of the engine's")
    ap.add_argument("--full", action="store_true", help="also the roofline probes, the opt-in passes, the metric all-reduce check and the CPU "
                    "baseline (a plain run measures the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned as DIR/<name>.npy")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


def self_launch(a):
    """`bench.py --gpus N` (N > 1) started without a launcher: run `python -m torch.distributed.run ... bench.py <same args>` as a child
    process, one rank per GPU, and pass its output and return code through.  Nothing in this process has initialised the GPU (no HIP
    call, no torch.cuda query) and nothing is exec'd: the child is an ordinary subprocess."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // a.gpus)))
    r = subprocess.run(cmd, env=env, cwd=ROOT)          # the ranks inherit stdout / stderr: rank 0 prints the ONE JSON line
    return r.returncode


if __name__ == "__main__":
    # N > 1 without a launcher: hand over to the child launcher BEFORE importing torch (nothing here has touched the GPU)
    _a = parse()
    if _a.gpus > 1 and ("RANK" not in os.environ or "WORLD_SIZE" not in os.environ):
        sys.exit(self_launch(_a))

import numpy as np
import torch


NUM_FRAMES, NUM_FUTURE, NUM_HISTORY, EP_STEPS, DECODE_TOKENS = 32, 4, 8, 64, 5


class Runner:
    """Drives the agent turn by turn from raw uint8 640x480 camera frames (host memory), exactly as the reference loop does:
    every env step preprocesses its frame (streamvln_eval.py:271-274 -> here upload + HIP bicubic kernel), every 4th step runs a
    model turn."""

    def __init__(self, model, cfg, rank, frame_ring=True):
        from streamvln_amd.agent import StreamingAgent
        from streamvln_amd.synthetic import SyntheticPromptEncoder, synthetic_frame
        self.proc = model.get_vision_tower().image_processor
        assert self.proc.backend == "hip"
        # the camera side of the loop: uint8 [480,640,3] frames in host memory.  With the engine's pinned frame ring (default) the
        # "camera" writes each frame into a ring slot, which the image processor then reads in place; --pageable-frames keeps them in
        # ordinary numpy arrays (one 921 KB staging copy per frame inside the processor, as in rounds 1-3).
        if frame_ring:
            ring = model.frame_ring(EP_STEPS, 480, 640)
            for s in range(EP_STEPS):
                ring[s][...] = synthetic_frame(rank, s)
            self.raw = [ring[s] for s in range(EP_STEPS)]
        else:
            self.raw = [synthetic_frame(rank, s) for s in range(EP_STEPS)]
        self.pre_s = 0.0                                                        # wall seconds inside the image processor
        self.agent = StreamingAgent(model, SyntheticPromptEncoder(cfg), num_frames=NUM_FRAMES, num_future_steps=NUM_FUTURE,
                                    num_history=NUM_HISTORY, device="cuda", max_new_tokens=DECODE_TOKENS, eos_token_ids=(),
                                    preprocess=self.preprocess)
        self.step = 0
        self.actions = 0
        self.model = model
        self.cache_frames = 0

    def preprocess(self, idx):
        t = time.perf_counter()
        out = self.proc.preprocess_array(self.raw[idx])
        self.pre_s += time.perf_counter() - t
        return out

    def turn(self):
        """run env steps until one model turn has happened"""
        n0 = len(self.agent.turn_log)
        while len(self.agent.turn_log) == n0:
            if self.step == EP_STEPS:                       # next episode
                self.agent.reset_memory()
                self.step = 0
                if self.cache_frames:                       # a new episode brings new frames: start from an empty cache
                    self.model.set_feature_cache(self.cache_frames)
            self.agent.act(self.step)
            self.step += 1
            self.actions += 1
        self.agent.turn_log[:] = self.agent.turn_log[-1:]


def timed_pass(model, turn, steps, warmup, world, lat=None):
    """W untimed turns, then exactly K turns bracketed by barrier + synchronize; returns the MAX-over-ranks seconds."""
    import torch.distributed as dist
    for _ in range(warmup):
        turn()
    grouped = dist.is_initialized()      # (a 1-rank group still runs the barrier / all-reduce: the RCCL branch on a one-GPU box)
    model.sync(); torch.cuda.synchronize()
    if grouped:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        turn()
        if lat is not None:
            lat.append(time.perf_counter() - t1)
    model.sync(); torch.cuda.synchronize()
    if grouped:
        dist.barrier()
    dt = time.perf_counter() - t0
    if grouped:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    return dt


def dump_outputs(d, run, model):
    """--dump-outputs: what the last timed turn returned to its caller (generate's `sequences`, exact in float64) and the final-norm
    hidden rows of the tokens it generated (float32); read after the clock stopped"""
    os.makedirs(d, exist_ok=True)
    seq = run.agent.turn_log[-1]["out"].sequences
    np.save(os.path.join(d, "sequences.npy"), seq.cpu().numpy().astype(np.float64))
    np.save(os.path.join(d, "hidden.npy"), model.last_hidden().astype(np.float32))


def cpu_baseline(cfg_true):
    """The CPU oracle (fp32 torch-CPU port of the reference path) on a bounded sample of the same workload: ONE steady turn at the
    true size, measured end to end (26-layer ViT on 1 frame, projector + pool, 28-layer prefill of T=212 rows over a C=1676 context,
    4 decode steps, 5 lm_head + arg-max) when the host has the memory for the 32 GB of fp32 weights; otherwise the round-1
    extrapolation from single layers (labelled).  Weight VALUES do not affect the timing: they are uniform random here (no 30 GB
    synthesis), and the context K/V are random tensors instead of a 1676-row prefill."""
    try:
        import psutil
        avail = psutil.virtual_memory().available
    except Exception:
        avail = 0
    if avail >= 56 << 30:
        try:
            return cpu_baseline_measured(cfg_true)
        except (MemoryError, RuntimeError) as e:          # out of memory on the host: fall back
            print(f"cpu_baseline: measured turn failed ({type(e).__name__}), falling back to the extrapolation", file=sys.stderr)
    return cpu_baseline_extrapolated(cfg_true)


def cpu_baseline_measured(cfg):
    from oracle import streamvln_oracle as O
    from streamvln_amd.weights import tensor_specs
    threads = torch.get_num_threads()
    t0 = time.perf_counter()
    w = {}
    for s in tensor_specs(cfg):
        w[s.name] = torch.empty(s.shape, dtype=torch.float32).uniform_(-s.half_width, s.half_width)
        if s.base:
            w[s.name] += s.base
    t_build = time.perf_counter() - t0
    T, C, H = 212, 1676, cfg.hidden
    g = torch.Generator().manual_seed(0)
    pix = torch.rand(1, 1, 3, cfg.v_image, cfg.v_image, generator=g) * 2 - 1
    ids = [int(t) for t in torch.randint(1000, 150000, (15,), generator=g)]
    cache = O.KVCache(cfg.layers)
    for i in range(cfg.layers):                            # the retained window: random K/V of the right shape
        cache.k[i] = torch.rand(cfg.kv_heads, C, cfg.head_dim, generator=g) - 0.5
        cache.v[i] = torch.rand(cfg.kv_heads, C, cfg.head_dim, generator=g) - 0.5
    with torch.no_grad():
        t0 = time.perf_counter()
        img, _ = O.encode_rgbd(w, cfg, pix, [[40]], None)                                   # vision: ViT + projector + pool
        rows = O.splice_embeds(w, ids[:13] + [O.IMAGE_TOKEN_INDEX] + ids[13:], img, None)    # 15 text + 196 image rows
        rows = torch.cat((w["model.embed_tokens.weight"][ids[0]][None], rows), 0)           # + the previous turn's EOS row = 212
        assert rows.shape[0] == T
        t_vis = time.perf_counter() - t0
        t0 = time.perf_counter()
        h = O.qwen2_forward(w, cfg, rows, C, cache)[-1]
        tok, _ = O.greedy_pick(O.lm_logits(w, h))
        t_pre = time.perf_counter() - t0
        t0 = time.perf_counter()
        for _ in range(DECODE_TOKENS - 1):
            x = w["model.embed_tokens.weight"][tok][None]
            h = O.qwen2_forward(w, cfg, x, len(cache), cache)[-1]
            tok, _ = O.greedy_pick(O.lm_logits(w, h))
        t_dec = time.perf_counter() - t0
    turn_s = t_vis + t_pre + t_dec
    return {"value": NUM_FUTURE / turn_s, "unit": "action-steps/s", "cores": threads, "kind": "port",
            "sample": f"n = 1: ONE measured steady turn at true size (fp32 torch-CPU oracle, all {cfg.v_layers} ViT + {cfg.layers} LLM layers, vocab "
                      f"{cfg.vocab}): vision {t_vis:.2f} s + prefill T={T} over C={C} {t_pre:.2f} s + {DECODE_TOKENS - 1} decode steps "
                      f"{t_dec:.2f} s = {turn_s:.2f} s (random weights built in {t_build:.1f} s, not timed)"}


def cpu_baseline_extrapolated(cfg_true):
    """Fallback when the host cannot hold the fp32 model: 1 ViT layer (1 frame) x26, projector + pool, 1 LLM layer prefill T=212 over
    C=1676 and 5 decode steps x28, lm_head x6, timed and scaled."""
    from dataclasses import replace
    from oracle import streamvln_oracle as O
    cfg = replace(cfg_true, v_layers=1, layers=1)
    torch.manual_seed(0)
    from streamvln_amd.weights import tensor_specs
    w = {s.name: (torch.rand(s.shape) * 2 - 1) * s.half_width + s.base for s in tensor_specs(cfg)}
    threads = torch.get_num_threads()
    T, C, H = 212, 1676, cfg.hidden

    def timed(fn, reps=2):
        best = 1e9
        for _ in range(reps):
            t = time.perf_counter(); fn(); best = min(best, time.perf_counter() - t)
        return best
    pix = torch.rand(1, 3, cfg.v_image, cfg.v_image) * 2 - 1
    x0 = O.siglip_embeddings(w, cfg, pix)
    t_vit_layer = timed(lambda: O.siglip_layer(w, cfg, 0, x0))
    t_embed = timed(lambda: O.siglip_embeddings(w, cfg, pix))
    t_proj = timed(lambda: O.pool_bilinear(cfg, O.mm_projector(w, x0)), reps=1)
    cache = O.KVCache(1)
    O.qwen2_layer(w, cfg, 0, torch.rand(C, H) - 0.5, torch.arange(C), cache)
    xs = torch.rand(T, H) - 0.5

    def prefill():
        c2 = O.KVCache(1); c2.k[0], c2.v[0] = cache.k[0], cache.v[0]
        O.qwen2_layer(w, cfg, 0, xs, torch.arange(C, C + T), c2)
    t_prefill_layer = timed(prefill)

    def decode():
        c2 = O.KVCache(1); c2.k[0], c2.v[0] = cache.k[0], cache.v[0]
        O.qwen2_layer(w, cfg, 0, xs[:1], torch.arange(C, C + 1), c2)
    t_decode_layer = timed(decode, reps=3)
    t_head = timed(lambda: O.lm_logits(w, xs[0]), reps=3)
    turn_s = (t_embed + 26 * t_vit_layer + t_proj + 28 * t_prefill_layer + (DECODE_TOKENS - 1) * 28 * t_decode_layer
              + DECODE_TOKENS * t_head)
    return {"value": NUM_FUTURE / turn_s, "unit": "action-steps/s", "cores": threads, "kind": "port",
            "sample": "EXTRAPOLATED (host memory too small for the fp32 model): one steady turn (1 frame, prefill T=212 over C=1676, 5 "
                      "tokens) at true dims, fp32 torch-CPU oracle: 1 ViT layer, projector+pool, 1 LLM layer prefill/decode and lm_head "
                      f"timed and scaled to 26/28 layers (turn = {turn_s:.2f} s)"}


def main():
    a = parse()
    from streamvln_amd.config import CONFIGS
    from streamvln_amd.dist import init_distributed_mode
    from streamvln_amd.model import StreamVLNForCausalLM
    from streamvln_amd.eval_harness import reduce_metrics
    import torch.distributed as dist

    if not a.full:              # a plain run: the headline pass only (the batched pass is skipped below; --batched-envs still sizes the engine)
        a.no_probe = a.no_cpu_baseline = a.no_feature_cache_pass = a.no_fp8_pass = a.no_prune_pass = True
    rank, world, local = init_distributed_mode(backend=a.backend)
    if a.single_device:
        local = 0
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE {world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP engine has no CPU fallback)"
    torch.cuda.set_device(local)
    cfg = CONFIGS[a.config]
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    n_benv = 1 if a.no_batched_pass else a.batched_envs
    model = StreamVLNForCausalLM(cfg, dtype=dtype, device=local, max_envs=n_benv, max_frames=1 + NUM_HISTORY)
    model.load_synthetic(a.seed)
    model.model.num_history = NUM_HISTORY
    model.set_decode_graph(not a.no_graph)
    if a.persistent_decode:
        model.set_decode_persistent(True)
    run = Runner(model, cfg, rank, frame_ring=not a.pageable_frames)
    if not a.own_torch_stream:
        torch.cuda.set_stream(model.torch_stream)       # the harness's own tensor ops (stack / to) run on the engine's stream: no cross-stream ordering
    lib, h = model._lib, model._h
    import ctypes as C

    def finish_episode():
        while run.step <= EP_STEPS - NUM_FUTURE:    # so the next pass starts on an episode boundary
            run.turn()                              # (after the last turn of an episode run.step == EP_STEPS - NUM_FUTURE + 1)

    # ---- headline pass: frame in (uint8, host) -> action ids out, everything inside the timed region
    for _ in range(a.warmup):
        run.turn()
    d3 = [C.c_double() for _ in range(3)]
    lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 1)
    model.preprocess_time(reset=True)
    run.pre_s = 0.0
    if not a.no_probe:
        lib.svln_probe_reset(h)
    lat = []
    dt = timed_pass(model, run.turn, a.steps, 0, world, lat)
    pre_wall_s = run.pre_s
    pre_gpu_ms, pre_frames = model.preprocess_time(reset=True)
    lib.svln_phase_times(h, C.byref(d3[0]), C.byref(d3[1]), C.byref(d3[2]), 0)
    roof = None
    if not a.no_probe:
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        lib.svln_probe_read(h, C.byref(ms), C.byref(n), C.byref(by))
        if n.value:
            avg_s = ms.value / n.value / 1e3
            ach = by.value / avg_s / 1e9
            # HBM bytes/launch: NOT measured in this run -- PMC counters need their own rocprofv3 --pmc passes (tools/make_profiles.sh);
            # the value is read from the latest committed pass of this kernel (gfx950 FETCH_SIZE x2 correction) and its file is named
            traffic = traffic_src = None
            import glob
            pmcs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemv_swiglu_pmc.json")))
            if pmcs and a.config == "streamvln_qwen2_7b" and a.dtype == "bf16" and not a.persistent_decode:
                traffic = json.load(open(pmcs[-1]))["traffic_bytes_per_launch"]
                traffic_src = os.path.relpath(pmcs[-1], ROOT)
            kern = ("decode_layer_kernel<bf16> (persistent layer: o_proj + gate/up + down_proj + next q|k|v)" if a.persistent_decode
                    else "gemv_kernel<bf16, EPI_SWIGLU> (decode gate/up projection)")
            roof = {"bound": "hbm", "kernel": kern, "achieved": round(ach, 1),
                    "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4), "traffic": traffic, "traffic_source": traffic_src,
                    "bytes_per_launch": by.value, "avg_us": round(avg_s * 1e6, 2), "launches_timed": n.value}

    roof2 = None
    if not a.no_probe:
        ms2, n2 = C.c_double(), C.c_int64()
        rows2, fl2, wb2 = C.c_double(), C.c_double(), C.c_double()
        lib.svln_probe_read_prefill(h, C.byref(ms2), C.byref(n2), C.byref(rows2), C.byref(fl2), C.byref(wb2))
        if n2.value:
            t2 = ms2.value / n2.value / 1e3
            # the steady prefill's largest product sits between both roofs (intensity ~ 2 * rows flop/B ~ the ridge): report both
            roof2 = {"bound": "mfma", "kernel": "gemm_glds_kernel<bf16, EPI_SWIGLU, 256x128 tiles> + K-split tail + reduce (prefill gate/up, layer 0 "
                                               "of every steady turn, HIP events on the engine's stream)",
                     "achieved": round(fl2.value / t2 / 1e12, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(fl2.value / t2 / 2.5e15, 4),
                     "traffic": None, "rows": round(rows2.value, 1), "flops_per_launch": fl2.value, "avg_us": round(t2 * 1e6, 2),
                     "launches_timed": n2.value,
                     "weight_stream": {"bound": "hbm", "achieved": round(wb2.value / t2 / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                                       "frac": round(wb2.value / t2 / 8e12, 4), "bytes_per_launch": wb2.value}}
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, run, model)

    def extra_pass(setup, teardown):
        setup()
        finish_episode()
        t = timed_pass(model, run.turn, a.steps, a.warmup, world)
        teardown()
        return {"value": round(NUM_FUTURE * a.steps * world / t, 2), "ms_per_step": round(t / a.steps * 1e3, 3)}

    # opt-in frame-feature memoisation.  Reported separately; `value` above re-encodes the history frames at every
    # window restart exactly as the reference does.
    cached = None
    if not a.no_feature_cache_pass:
        def on():
            run.cache_frames = 96
            model.set_feature_cache(96)

        def off():
            run.cache_frames = 0
        cached = extra_pass(on, off)
        hits, misses = model.feature_cache_stats()
        model.set_feature_cache(0)
        cached.update(hits=hits, misses=misses,
                      note="opt-in: pooled features of frames already encoded in the episode are reused (content hash) instead of "
                           "re-running the ViT on the 8 <memory> frames; not the headline value")
    # opt-in fp8 (e4m3) LLM weights (no reference counterpart): decode GEMVs + lm_head stream the e4m3 copies, the prefill
    # products run as e4m3 x e4m3 MFMA GEMMs with per-row activation scales.  Reduced precision -> never the headline value.
    fp8 = None
    if not a.no_fp8_pass and a.dtype == "bf16":
        def fp8_on():
            model.set_fp8_decode(True)
            model.set_fp8_gemm(True)

        def fp8_off():
            model.set_fp8_decode(False)
            model.set_fp8_gemm(False)
        fp8 = extra_pass(fp8_on, fp8_off)
        fp8.update(dtype="bf16 activations / e4m3 LLM weights (per-row scales); prefill GEMMs e4m3 x e4m3 MFMA with fp32 accumulate",
                   note="opt-in: decode-step GEMVs and lm_head stream per-row-scaled e4m3 copies of the LLM weights (half the HBM bytes per "
                        "token), prefill QKV / o / gate-up / down run as fp8 MFMA products; vision, attention and norms stay bf16; "
                        "reduced precision, not the headline value")
    if fp8 is not None:
        # what the reduced precision does to the outputs, at the benchmarked size: the first 3 turns of an episode in bf16 and with both
        # e4m3 modes on the same inputs -- ids equal before the first divergence, and the relative L2 error of the final-norm hidden rows
        # that saw identical inputs (random-init weights have top-2 margins of the size of the e4m3 logit error: see DESIGN.md 6)
        def short_episode():
            run.agent.reset_memory(); run.step = 0
            run.agent.prompt_encoder.reset()      # the SAME prompts in both runs (round 3 compared runs with different prompt streams: its
            out = []                              # "0/5 ids, rel L2 1.25" was the distance between two unrelated prompts, not an fp8 error)
            for _ in range(3):
                run.turn()
                out.append((run.agent.turn_log[-1]["out"].sequences[0].tolist(), model.last_hidden()))
            return out
        ref = short_episode()
        fp8_on()
        got = short_episode()
        fp8_off()
        run.agent.reset_memory(); run.step = 0              # the next pass starts on an episode boundary
        agree = total = 0
        worst = 0.0
        for (ia, ha), (ib, hb) in zip(ref, got):
            n = 0
            while n < len(ia) and ia[n] == ib[n]:
                n += 1
            agree += n; total += len(ia)
            for j in range(min(n + 1, len(ia))):
                worst = max(worst, float(np.linalg.norm(hb[j] - ha[j]) / np.linalg.norm(ha[j])))
            if n < len(ia):
                break
        fp8["vs_bf16"] = {"ids_agree_before_first_divergence": f"{agree}/{total}", "hidden_rel_l2_worst": round(worst, 4),
                          "sample": "first 3 turns of an episode, 5 tokens each, same frames and prompts (the distance to bf16 is the e4m3 scheme's own "
                                    "noise on random-init weights, not an error bound: DESIGN.md 6)"}
        # engine vs the SAME numeric scheme restated on the CPU (oracle Fp8Emu): measured by tests/test_fp8_gpu.py on the GPU box and committed;
        # bench.py does not run the oracle for this (only its cpu_baseline leg may)
        import glob
        emu = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_fp8_vs_emulation.json")))
        if emu and a.config == "streamvln_qwen2_7b":
            e = json.load(open(emu[-1]))
            fp8["vs_emulation"] = {"source": os.path.relpath(emu[-1], ROOT),
                                   "decode_weights_full_depth": e.get("streamvln_qwen2_7b/decode"),
                                   "mfma_products_full_depth": {k: v for k, v in (e.get("streamvln_qwen2_7b/gemm") or {}).items() if k != "depth_curve_vs_bf16_engine"}}
    # opt-in slow-memory pruning (BASELINE configs[3] "32 pruned slow-memory tokens"; no reference counterpart, SURVEY a-13).
    pruned = None
    if not a.no_prune_pass:
        pruned = extra_pass(lambda: model.set_memory_prune(32), lambda: model.set_memory_prune(0))
        pruned.update(keep_tokens=32,
                      note="opt-in extension (no reference counterpart): <memory> = the 32 history tokens least similar to the mean "
                           "history token instead of all 8 x 196 (HIP selection kernels, checked against the project's own CPU "
                           "restatement); changes the model input, not the headline value")
    # BASELINE configs[4]-style concurrent envs on this GPU through generate_batch (build-side extension).
    batched = None
    if a.full and not a.no_batched_pass and n_benv > 1:
        from streamvln_amd.agent import BatchedAgents, StreamingAgent
        from streamvln_amd.synthetic import SyntheticPromptEncoder
        model.reset(n_benv)
        agents = [StreamingAgent(model, SyntheticPromptEncoder(cfg, seed=7 + 31 * e), num_frames=NUM_FRAMES, num_future_steps=NUM_FUTURE,
                                 num_history=NUM_HISTORY, env_id=e, device="cuda", max_new_tokens=DECODE_TOKENS, eos_token_ids=(),
                                 preprocess=run.preprocess) for e in range(n_benv)]
        group = BatchedAgents(agents)
        bstep = [0]

        def lockstep_turn():
            n0 = len(agents[0].turn_log)
            while len(agents[0].turn_log) == n0:
                if bstep[0] == EP_STEPS:
                    for ag in agents:
                        ag.reset_memory()
                    bstep[0] = 0
                group.act([(bstep[0] + 7 * e) % EP_STEPS for e in range(n_benv)])       # env e sees the stream shifted by 7e frames
                bstep[0] += 1
            for ag in agents:
                ag.turn_log[:] = ag.turn_log[-1:]
        dtb = timed_pass(model, lockstep_turn, a.steps, a.warmup, world)
        batched = {"envs_per_gpu": n_benv, "value": round(NUM_FUTURE * n_benv * a.steps * world / dtb, 2), "unit": "action-steps/s",
                   "per_gpu": round(NUM_FUTURE * n_benv * a.steps / dtb, 2), "ms_per_lockstep_turn": round(dtb / a.steps * 1e3, 3),
                   "dtype": "bf16",
                   "note": "BASELINE configs[4]-style: envs_per_gpu concurrent envs stepped in lockstep (batched prefill rows + batched "
                           "decode steps, bf16); not the headline value"}
        if a.dtype == "bf16" and not a.no_fp8_pass:
            # configs[4] as BASELINE.json words it: batch of concurrent envs + fp8 MFMA on the QKV / MLP GEMMs (prefill rows and the
            # 32-row decode-step products of the batch); opt-in, reduced precision
            model.set_fp8_gemm(True)
            while bstep[0] <= EP_STEPS - NUM_FUTURE:        # finish the episode (after its last turn bstep == EP_STEPS - NUM_FUTURE + 1)
                lockstep_turn()
            dt8 = timed_pass(model, lockstep_turn, a.steps, a.warmup, world)
            model.set_fp8_gemm(False)
            batched["fp8_mfma"] = {"value": round(NUM_FUTURE * n_benv * a.steps * world / dt8, 2), "unit": "action-steps/s",
                                   "ms_per_lockstep_turn": round(dt8 / a.steps * 1e3, 3),
                                   "dtype": "bf16 activations / e4m3 x e4m3 MFMA for the LLM's QKV, o, gate-up and down products (per-row "
                                            "weight and activation scales, fp32 accumulate, bf16 out); lm_head, attention, vision bf16",
                                   "note": "opt-in extension, no reference counterpart; reduced precision, never the headline"}
    # the one exchange of the path: per-episode metrics -> 5-scalar RCCL all-reduce (synthetic metrics here)
    summary = None
    if a.full:
        summary = reduce_metrics([{"success": 1.0, "spl": 0.5, "os": 1.0, "ne": float(rank)}],
                                 device="cuda" if (dist.is_initialized() and dist.get_backend() == "nccl") else "cpu")
    turns_total = a.steps * world
    value = NUM_FUTURE * turns_total / dt
    if rank == 0:
        out = {
            "metric": "action-steps/sec (8-frame window, StreamVLN-Qwen-1.5)", "value": round(value, 2), "unit": "action-steps/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": "configs[1]: StreamVLN-Qwen-1.5 (SigLIP-so400m + Qwen2-7B, random-init), synthetic uint8 640x480 stream, "
                                   "8-frame window (num_frames 32 / future 4 / history 8), 5 decode tokens/turn, 1 env per GPU; "
                                   "step = one model turn = 4 env steps, each preprocessing its frame (upload + HIP bicubic) inside "
                                   "the timed region", "model_config": a.config, "envs_per_gpu": 1,
                       "decode_graph": not a.no_graph, "decode_step": "attention + 1 persistent launch per layer" if a.persistent_decode else "6 launches per layer (hipGraph)",
                       "frames": "pageable host arrays" if a.pageable_frames else "engine's pinned frame ring (host)",
                       "parallelism": f"episode-parallel x{world}",
                       "dist_backend": dist.get_backend() if dist.is_initialized() else None},
            "per_gpu": round(value / world, 2),
            "p50_ms_per_turn": round(float(np.median(lat)) * 1e3, 3),
            "turn_ms": [round(x * 1e3, 2) for x in lat],
            # preprocess = wall time inside the image processor (host memcpy to pinned staging + H2D + kernel + sync), 4 frames per turn;
            # preprocess_gpu = the device part of it (HIP events); vision / prefill / decode = HIP events on the engine's stream
            "phase_ms_per_turn": {"preprocess": round(pre_wall_s / a.steps * 1e3, 3), "preprocess_gpu": round(pre_gpu_ms / a.steps, 3),
                                  "vision": round(d3[0].value / a.steps, 3), "prefill": round(d3[1].value / a.steps, 3),
                                  "decode": round(d3[2].value / a.steps, 3)},
            "preprocess_frames_per_turn": round(pre_frames / a.steps, 2),
            # the same run with the image-processor time taken out: the rate at the generate() boundary (frames already preprocessed
            # and resident, as round 1 reported it)
            "generate_boundary": {"value": round(NUM_FUTURE * turns_total / max(dt - pre_wall_s, 1e-9), 2), "unit": "action-steps/s",
                                  "ms_per_step": round((dt - pre_wall_s) / a.steps * 1e3, 3)},
            "metric_allreduce_check": summary,
            "roofline": roof,
            "roofline_prefill_gemm": roof2,
            "with_feature_cache": cached,
            "fp8_decode_weights": fp8,
            "memory_prune_32": pruned,
            "batched_envs": batched,
        }
        if world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(CONFIGS["streamvln_qwen2_7b"])
        print(json.dumps(out), flush=True)
    model.close()
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
