"""The GEMM dispatcher (gemm_plan.h through svln_gemm_plan: no GPU) on e4m3 products in the block-scaled MFMA form (svln_gemm_problem.fp8 = 2,
or force_cfg | 0x40000 on an e4m3 product): every launch is marked scaled, the large-tile products of a window restart / a batched-env
prefill go to the 8-phase 256x256 schedule on the conditions bf16 products do, and nothing else moves against fp8 = 1, over the shapes of
the recorded table (tests/golden/gemm_plan_table.json).  fp8 = 1 never reaches the 8-phase schedule.  The switch is part of the C surface."""
import json
import os
import re

from streamvln_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
_FILE = json.load(open(os.path.join(HERE, "golden", "gemm_plan_table.json")))
PROBLEMS = [{**_FILE["problem_defaults"], **problem} for _, problem, _, _, _ in _FILE["rows"]]
BF16_E4M3 = [p for p in PROBLEMS if p.get("dtype", _lib.SVLN_BF16) == _lib.SVLN_BF16 and p.get("epi", 0) in (_lib.EPI_NONE, _lib.EPI_SWIGLU)]
P8, BIG = _lib.GEMM_TILES.index("p8"), _lib.GEMM_TILES.index("big")
LAUNCH_FIELDS = [n for n, _ in _lib.SvlnGemmLaunch._fields_]


def plan(p, **kw):
    g = _lib.gemm_plan(**{**p, **kw})
    ls = [{f: (list(getattr(l, f)) if f == "reducer_grid" else getattr(l, f)) for f in LAUNCH_FIELDS} for l in g.launch[:g.n_launches]]
    return dict(nt_w=g.nt_w, bn_fast=g.bn_fast, fused=g.fused, vit_packer=g.vit_packer), ls


def test_fp8_2_marks_every_launch_scaled_and_moves_nothing_but_the_8_phase_route():
    assert len(BF16_E4M3) >= 100
    moved = 0
    for p in BF16_E4M3:
        h1, l1 = plan(p, fp8=1)
        h2, l2 = plan(p, fp8=2)
        assert h1 == h2 and len(l1) == len(l2), p
        for a, b in zip(l1, l2):
            assert a["fp8"] == 1 and b["fp8"] == 2, (p, a, b)
            assert a["tile"] != P8, p                                # fp8 = 1 never reports the 8-phase tile
            if b["tile"] == P8:
                moved += 1
                assert a["tile"] == BIG and not b["splitk"], (p, a, b)
                a = {**a, "tile": P8}
            assert {**a, "fp8": 2} == b, (p, a, b)
        # the op-level flag is the same request
        assert plan(p, fp8=1, force_cfg=p.get("force_cfg", 0) | _lib.GEMM_FORCE_FP8_SCALED)[1] == \
            [{**l} for l in plan(p, fp8=2, force_cfg=p.get("force_cfg", 0) | _lib.GEMM_FORCE_FP8_SCALED)[1]], p
    assert moved >= 2, moved


def test_fp8_2_sends_the_restart_and_batched_prefill_products_to_the_8_phase_tile():
    base = dict(dtype=_lib.SVLN_BF16, has_ws=1, ws_elems=1 << 28, has_zeros=1)
    for M in (1696, 1952):
        for epi in (_lib.EPI_SWIGLU, _lib.EPI_NONE):
            _, (l,) = plan(base, M=M, N=37888, K=3584, epi=epi, fp8=2)
            assert l["tile"] == P8 and l["fp8"] == 2 and not l["splitk"] and l["block"] == 512 and l["lds_bytes"] == 131072, (M, l)
            assert l["grid"] == -(-M // 256) * (37888 // 256)
            _, (l1,) = plan(base, M=M, N=37888, K=3584, epi=epi, fp8=1)
            assert l1["tile"] == BIG and l1["fp8"] == 1
    _, (l,) = plan(base, M=293, N=331, K=912, fp8=2, force_cfg=256)
    assert l["tile"] == P8 and l["fp8"] == 2
    _, (l,) = plan(base, M=293, N=331, K=912, fp8=2, force_cfg=256 | 0x4000)          # the stage ring stays reachable
    assert l["tile"] == BIG and l["fp8"] == 2
    _, (l,) = plan(base, M=293, N=331, K=912, fp8=1, force_cfg=256)
    assert l["tile"] == BIG and l["fp8"] == 1
    # without the zero line (the K-tail source of the schedule) or below the thresholds: as fp8 = 1
    _, (l,) = plan({**base, "has_zeros": 0}, M=1952, N=37888, K=3584, fp8=2)
    assert l["tile"] != P8
    _, (l,) = plan(base, M=512, N=37888, K=3584, fp8=2)
    assert l["tile"] != P8
    # the two-K-slice 8-phase form stays bf16-only: an e4m3 down_proj of a window restart plans as fp8 = 1 does
    for fc in (0, 258):
        t1 = [l["tile"] for l in plan(base, M=1952, N=3584, K=18944, fp8=1, force_cfg=fc)[1]]
        t2 = [l["tile"] for l in plan(base, M=1952, N=3584, K=18944, fp8=2, force_cfg=fc)[1]]
        assert t1 == t2 and P8 not in t2, (fc, t1, t2)


def test_fp8_0_and_the_float_engine_ignore_the_form():
    for p in PROBLEMS[::7]:
        if p.get("fp8"):
            continue
        assert plan(p) == plan(p, force_cfg=p.get("force_cfg", 0) | _lib.GEMM_FORCE_FP8_SCALED), p
    _, ls = plan(dict(dtype=_lib.SVLN_F32, has_ws=1, ws_elems=1 << 28, has_zeros=1), M=1952, N=37888, K=3584, fp8=2)
    assert all(l["fp8"] == 0 and l["tile"] != P8 for l in ls)                         # (no e4m3 kernels for the fp32 engine: as fp8 = 1 there)


def test_the_switch_is_declared_bound_and_documented():
    header = open(os.path.join(HERE, "..", "include", "streamvln_hip.h")).read()
    assert re.search(r"\bint svln_set_fp8_scaled_mfma\(svln_engine\* h, int enable\);", header)
    assert "svln_set_fp8_scaled_mfma" in _lib.SIGNATURES and _lib.SIGNATURES["svln_set_fp8_scaled_mfma"] == _lib.SIGNATURES["svln_set_fp8_gemm"]
    assert hasattr(_lib.load(), "svln_set_fp8_scaled_mfma")
    assert "0x40000" in header and _lib.GEMM_FORCE_FP8_SCALED == 0x40000
    from streamvln_amd.model import StreamVLNForCausalLM
    assert callable(getattr(StreamVLNForCausalLM, "set_fp8_scaled_mfma"))
