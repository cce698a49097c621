"""CPU proof that the inputs of tests/test_fp8_scaled_gpu.py are sharp (the cases of tests/fp8s_ref.py: e4m3 products on the block-scaled
MFMAs).  Every exact case is held to its exactness condition -- every term a multiple of the output's quantum and sum |a w| + |bias| +
|res| below 2^23 quanta, so the expected bits are the float64 value rounded once to bf16 -- and on every case each mutant that applies
changes the stored bits of at least one output (exact cases) or moves the output by at least 10x the bound of the GPU test (SwiGLU, the
ratio of tests/test_gemm_inputs.py).  One test asserts that each mutant is seen by some case of each kernel form and that the case list
reaches every (tile, split / unsplit, epilogue) the variant table of gemm.hip instantiates for the scaled form."""
import re
import os

import pytest
import torch

import fp8s_ref as S
import gemm_ref as R


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_scaled_inputs_are_discriminating(case):
    case.build()
    assert case.geom["cfg"] in R.CFGS and case.force_cfg & S.SCALED
    load = case.load()
    assert float(load.max()) < 2.0 ** 23, (case.id, float(load.max()))
    assert case.terms_on_quantum(), case.id
    body = torch.cat([case.Abuf[:, :case.K].reshape(-1), case.Wbuf[:, :case.K].reshape(-1)])
    assert not bool(((body & 0x7F) == 0x7F).any()), f"{case.id}: a NaN code among the operands"
    if case.family == "alphabet":                 # all three bands, and both zeros, in every case
        codes = {b & 0x7F for b in set(body.tolist())}
        assert codes & set(S.NORMAL) and codes & set(range(1, 8)) and codes & set(S.TOP) and {0x00, 0x80} <= set(body.tolist()), case.id
    report = R.mutant_report(case)
    print(f"{case.id}: max load {float(load.max()):.0f} quanta; " + ", ".join(f"{k} {v if case.exact else round(v, 1)}" for k, v in report.items()))
    weak = {k: v for k, v in report.items() if not (v >= 1 if case.exact else v >= 10.0)}
    assert not weak, f"{case.id}: mutants the case cannot see: {weak} (all: {report})"


def _instantiated_scaled_variants():
    """(tile, splitk) of the rows with operand column 2 in SVLN_GEMM_VARIANTS, read from gemm.hip"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "streamvln_amd", "csrc", "gemm.hip")).read()
    src = src.replace("\\\n", " ")
    macros = dict(re.findall(r"#define (SVLN_GEMM_ROWS\w+)\(X, tile, C\)\s+(.*)", src))
    body = re.search(r"#define SVLN_GEMM_VARIANTS\(X\)\s+(.*)", src).group(1)
    for name, text in macros.items():
        body = re.sub(name + r"\(X, (\w+), (\w+)\)", lambda m: text.replace("tile", m.group(1)).replace(" C,", f" {m.group(2)},"), body)
    rows = re.findall(r"X\((TILE_\w+), \w+, (true|false), (\d), (true|false), (true|false)\)", body)
    assert len(rows) >= 50, len(rows)
    names = {"TILE_SKINNY": "skinny", "TILE_C64": "c64", "TILE_C128": "c128", "TILE_C128L": "c128L", "TILE_C128K2": "c128K2", "TILE_C256": "c256",
             "TILE_C256N64": "c256n64", "TILE_BIG": "big", "TILE_P8": "p8", "TILE_P8_32": "p8_32"}
    return {(names[t], sk == "true") for t, sk, op, ntw, vp in rows if op == "2"}


def test_scaled_case_coverage():
    variants = _instantiated_scaled_variants()
    assert {t for t, _ in variants} == {"skinny", "c64", "c128", "c128L", "c128K2", "c256", "big", "p8"}, variants
    hit = {(c.geom["cfg"], c.split_S > 1 and not c.geom["tail"], c.epi) for c in S.CASES}
    for tile, splitk in sorted(variants):
        for epi in ("none", "swiglu"):              # the epilogues an e4m3 kernel exists for
            assert (tile, splitk, epi) in hit, (tile, splitk, epi)
    # the ladder on an unsplit loop of every tile, in both families for the exact ones
    for tile in {t for t, _ in variants} - {"c128L"}:
        for fam in ("sign", "alphabet"):
            rungs = {c.kc for c in S.CASES if c.geom["cfg"] == tile and c.split_S == 1 and c.family == fam and c.exact}
            assert len(rungs) >= len(S.LADDER) // 2, (tile, fam, rungs)
        assert {c.kc for c in S.CASES if c.geom["cfg"] == tile and c.split_S == 1 and c.exact} >= set(S.LADDER), tile
    # split launches: 2, 3 and 5 slices, an empty slice; the 8-phase kernel: odd and even K tile counts, staged and direct stores
    splits = [c for c in S.CASES if c.split_S > 1]
    assert {c.split_S for c in splits} >= {2, 3, 5} and any(b == e for c in splits for b, e in R.k_slices(c.stages, c.split_S))
    p8 = [c for c in S.CASES if c.geom["cfg"] == "p8"]
    assert {c.stages % 2 for c in p8 if c.staged} == {0, 1} and {c.stages % 2 for c in p8 if not c.staged} == {0, 1}
    assert any(c.force_cfg & 0x20000 for c in p8) and any(c.epi == "swiglu" and c.staged for c in p8) and any(c.epi == "swiglu" and not c.staged for c in p8)
    assert any(c.geom["cfg"] == "big" and c.force_cfg & 0x4000 for c in S.CASES)
    # every mutant is seen (changes bits) by cases of the stage ring and of the 8-phase kernel; the scale mutants by every case they apply to
    for form in (False, True):
        seen = {}
        for c in S.CASES:
            if c.exact and c.p8 == form:
                for k in c.mutants():
                    seen.setdefault(k, 0)
                    seen[k] += 1
        need = set(S.NEW_MUTANTS) | {"a_scale_by_column", "w_scale_by_row", "drop_ragged_stage"} | (set() if form else {"scale_twice_per_slab"})
        assert set(seen) >= need, (form, need - set(seen))
    for c in S.CASES:
        assert c.N > c.BN and c.M % 32 and c.K % 16 == 0, c.id
        assert c.split_S * c.M * c.N <= 16 * 256 * 4096, c.id
