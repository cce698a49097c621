"""CPU proof that the inputs of tests/test_gemm_gpu.py are sharp.  On every case of that file each plausible kernel mistake that applies
to the case (the float64 "mutant" references of tests/gemm_ref.py) changes the stored bits of at least one expected output (exact family),
or moves the expected output by at least 10x the bound the GPU test applies (toleranced family; the ratio tests/test_gemv_inputs.py uses).
The exact cases are held to their precondition (sum |a w| + |bias| + |res| of an output below 2^23 quanta: every fp32 partial sum is exact
in any order, across slabs and K groups) and to at least 90 % of the expected outputs being values of the engine type.  One test asserts
that the case list reaches every tile configuration, every rung of the K ladder for every ring depth, empty K slices, an empty K group and
both epilogues of the 8-phase kernel.  Each test prints its mutants with the outputs changed / the ratio (pytest -s, or on failure)."""
import pytest
import torch

import gemm_ref as R


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_gemm_inputs_are_discriminating(case):
    ref = case.build().reference()
    if case.exact or case.epi == "swiglu":
        load = case.load()
        assert float(load.max()) < 2.0 ** 23, (case.id, float(load.max()))
    if case.exact:
        frac = float(R.representable(ref, case.dtype).double().mean())
        print(f"{case.id}: max load {float(load.max()):.0f} quanta, {100 * frac:.2f} % of the outputs are {case.dtype} values")
        assert frac >= 0.90, (case.id, frac)
        for buf in (case.Abuf, case.Wbuf):                                # no operand is zero: no product is
            assert bool((buf != 0).all()), case.id
    if case.epi == "swiglu":
        lo, hi = case.gate_span()
        assert lo <= -12 and hi >= 12, (case.id, lo, hi)
    report = R.mutant_report(case)
    print(f"{case.id}: " + ", ".join(f"{k} {v if case.exact else round(v, 1)}" for k, v in report.items()))
    weak = {k: v for k, v in report.items() if not (v >= 1 if case.exact else v >= 10.0)}
    assert not weak, f"{case.id}: mutants the case cannot see: {weak} (all: {report})"


def test_gemm_case_coverage():
    """the case list reaches what it is named for (R.plan asks the dispatcher itself, svln_gemm_plan; k_slices / groups restate the stage and slice arithmetic)"""
    by_cfg = {}
    for c in R.CASES:
        by_cfg.setdefault(c.geom["cfg"], []).append(c)
    # every tile configuration, in both engine types where it exists (the 8-phase schedule takes bf16 operands only)
    for cfg in R.CFGS:
        fmts = {c.fmt for c in by_cfg.get(cfg, [])}
        assert fmts >= ({"bf16"} if cfg.startswith("p8") else {"bf16", "fp32"}), (cfg, fmts)
    forced = {c.force_cfg for c in R.CASES}
    assert forced >= {0, 32, 64, 128, 129, 256, 256 | 0x4000, 256 | 0x8000, 256 | 0x20000, 258, 264} and any(f & 0x10000 for f in forced)
    assert {c.force_split for c in R.CASES} >= {0, 1, 2, 3, 5}
    for entry in ("gemm", "norm", "q8", "fp8"):
        assert any(c.entry == entry for c in R.CASES), entry
    # each rung of the ladder on an unsplit K loop of every ring depth (2, 3, 6 stage buffers; the 8-phase kernel's two tiles per iteration)
    for depth in (2, 3, 6, "p8"):
        rungs = {c.kc for c in R.CASES if c.ring == depth and c.split_S == 1 and c.KG == 1 and not c.geom["tail"]}
        assert rungs >= set(R.LADDER), (depth, sorted(set(R.LADDER) - rungs))
    assert {c.kc for c in by_cfg["c128K2"]} >= set(R.LADDER)
    # empty K slices (more slices than stages; the second slice of the two-slice 8-phase launch at one K tile) and an empty K group
    empty = lambda c: any(b == e for b, e in R.k_slices(c.stages, c.split_S))
    assert any(empty(c) and c.geom["cfg"] == "c256" for c in R.CASES) and any(empty(c) and c.geom["cfg"] == "skinny" for c in R.CASES)
    assert any(empty(c) and c.geom["cfg"] == "p8" and c.stages == 1 for c in R.CASES)
    assert any(c.KG == 2 and c.groups()[1][0] == c.groups()[1][1] for c in R.CASES)
    assert any(c.KG == 2 and c.stages % 2 == 1 and c.stages > 1 for c in R.CASES)               # the second group one stage short
    for c in R.CASES:                                                                          # a forced split count is the one that runs
        if c.force_split > 1 and c.geom["cfg"] != "c256n64":
            assert c.split_S == c.force_split, c.id
    # the 8-phase kernel: LDS-staged and direct stores, with and without a ragged last 16-byte chunk, odd and even K tile counts
    p8 = [c for c in by_cfg["p8"] if c.split_S == 1]
    assert any(c.staged and c.n_out % 8 for c in p8) and any(not c.staged and c.ldc % 8 for c in p8) and any(c.force_cfg & 0x20000 for c in p8)
    assert {c.stages % 2 for c in p8 if c.staged} == {0, 1} and {c.stages % 2 for c in p8 if not c.staged} == {0, 1}
    # the regimes the big shapes are named for
    assert any(c.geom["cfg"] == "c128L" and R.cdiv(c.M, 128) * R.cdiv(c.N, 128) > 256 for c in R.CASES)
    tails = [c for c in R.CASES if c.geom["tail"]]
    assert {c.epi for c in tails} >= {"none", "swiglu"} and all(c.geom["tail"][1] > 1 and c.M <= 256 for c in tails)
    n64 = [c for c in R.CASES if c.geom["cfg"] == "c256n64" and c.force_cfg == 0 and c.M <= 256]
    vit64 = [c for c in R.CASES if c.geom["cfg"] == "c256n64" and c.force_cfg == 0 and c.M > 512]
    assert {c.fmt for c in n64} == {"bf16", "fp32"} and {c.fmt for c in vit64} == {"bf16", "fp32"}
    assert all(c.geom["fused"] and c.split_S > 1 for c in n64 + vit64) and all(c.split_S == 3 for c in vit64)
    assert all(c.geom["fused"] for c in R.CASES if c.norm), "a norm case whose reduce does not emit the norm"
    # shapes: ragged against the tile in both directions, at least two column tiles, split launches on N % 4 == 0 but not % 8
    for c in R.CASES:
        assert c.N > c.BN and (c.N % c.BN or c.geom["tail"] or c.epi == "swiglu"), c.id
        assert c.M % 32 or c.M in (256,), c.id
        if c.split_S > 1 and c.epi != "swiglu" and not c.geom["tail"]:
            assert c.N % 4 == 0 and c.N % 8, c.id
        assert c.split_S * c.M * c.N <= 16 * 256 * 4096, c.id           # inside what the GPU test dirties before a split case
    assert any(c.inplace for c in R.CASES) and any(c.lda == c.K for c in R.CASES) and any(c.res_mod for c in R.CASES)
