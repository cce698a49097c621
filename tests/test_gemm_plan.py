"""The GEMM dispatcher (streamvln_amd/csrc/gemm_plan.h, asked through svln_gemm_plan: no GPU) against a characterisation table.

tests/golden/gemm_plan_table.json was recorded from launch_epi as it stood BEFORE the planner was split out of it (DESIGN.md 4.1 says
how): per problem, every launch that reached the stream -- kernel instantiation, grid, block, dynamic LDS, the launcher-filled GemmArgs
fields [nsplit, tile_base, launch_tiles, nt_w, bn_fast, vp_on], the reducer and its grid -- and what launch_gemm returned; the file's
head names the columns.  The rows are every product the engine issues at true size in bf16, float and e4m3, every case of
gemm_ref.CASES, both sides of every threshold of the dispatcher (in bf16) and one row for each kernel variant those leave out.  A
deliberate change of a heuristic re-records the rows it moves; a refactor moves none."""
import json
import os

import pytest

from streamvln_amd import _lib

_FILE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_table.json")))
TABLE = [dict(what=what, problem={**_FILE["problem_defaults"], **problem}, launches=[list(l) for l in ls], fused=fused, vit_packer=vp)
         for what, problem, ls, fused, vp in _FILE["rows"]]
REDUCER_KERNELS = {"epilogue": "epilogue", "rownorm": "rownorm", "qkv_rope": "qkv_rope", "vitpack": "qkv_vitpack"}   # splitk_*_kernel


def launches(problem):
    """the plan of `problem` in the form of a table row"""
    g = _lib.gemm_plan(**problem)
    T = "float" if problem.get("dtype", _lib.SVLN_BF16) == _lib.SVLN_F32 else "bf16"
    out = []
    for l in g.launch[:g.n_launches]:
        kernel = f"{T},epi{problem.get('epi', 0)},{_lib.GEMM_TILES[l.tile]},{'e4m3' if l.fp8 else T}" + \
                 ",splitk" * l.splitk + ",ntw" * l.ntw + ",vp" * l.vp
        red = _lib.GEMM_REDUCERS[l.reducer]
        assert not l.reduce_too_large
        out.append([kernel, l.grid, l.block, l.lds_bytes, [l.nsplit, l.tile_base, l.launch_tiles, g.nt_w, g.bn_fast, l.vp]] +
                   ([REDUCER_KERNELS[red], list(l.reducer_grid), l.reducer_block] if red else []))
    return {"launches": out, "fused": g.fused, "vit_packer": g.vit_packer}


def test_plan_reproduces_the_recorded_dispatch():
    assert len(TABLE) >= 300 and len({json.dumps(r["problem"], sort_keys=True) for r in TABLE}) == len(TABLE)
    wrong = []
    for row in TABLE:
        got = launches(row["problem"])
        exp = {k: row[k] for k in ("launches", "fused", "vit_packer")}
        if got != exp:
            wrong.append((row["what"], row["problem"], exp, got))
    assert not wrong, f"{len(wrong)} of {len(TABLE)} rows differ; the first: {wrong[0]}"


def test_table_reaches_every_route():
    """every tile, every reducer, the tail launch, both engine types and e4m3 operands occur in the recorded rows"""
    kernels = {l[0] + ">" for r in TABLE for l in r["launches"]}
    for T in ("bf16", "float"):
        for tile in _lib.GEMM_TILES:
            if T == "float" and tile.startswith("p8"):
                continue
            assert any(k.startswith(f"{T},") and f",{tile}," in k for k in kernels), (T, tile)
    assert any(",e4m3" in k for k in kernels) and any(k.endswith(",vp>") for k in kernels)
    assert {l[5] for r in TABLE for l in r["launches"] if len(l) > 5} == set(REDUCER_KERNELS.values())
    assert any(len(r["launches"]) == 2 and r["launches"][1][4][1] == 256 for r in TABLE)
    assert any(not r["launches"] for r in TABLE)
    assert {r["vit_packer"] for r in TABLE} == {0, 1, 2}


def test_plan_refuses_unknown_dtype_and_epilogue():
    for bad in (dict(dtype=2), dict(dtype=-1), dict(epi=_lib.EPI_ARGMAX), dict(epi=5), dict(epi=-1), dict(M=1 << 31)):
        with pytest.raises(_lib.SvlnError):
            _lib.gemm_plan(**{"M": 64, "N": 64, "K": 64, **bad})
    lib = _lib.load()
    assert lib.svln_gemm_plan(None, None) != 0 and len(lib.svln_last_error()) > 0
