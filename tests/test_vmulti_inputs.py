"""CPU proofs for tests/test_vmulti_gpu.py: the scenarios of tests/vmulti_ref.py show every mistake only a several-sequence verify launch
can make.  Each mutant of vmulti_ref.MUTANTS must move some output of some scenario by at least 100x the tolerance the GPU test applies,
or an appended K / V row, or the set of pool slots the launch writes (the untouched-slot check of the GPU test).  The sequences that use
all their row slots are also sharp in the single-sequence sense of tests/test_verify_inputs.py (10x, its factor)."""
import pytest
import torch

import attn_ref as R
import verify_ref as VR
import vmulti_ref as VM

DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def effects():
    return {(name, dtype, mu): VM.mutant_effect(name, dtype, mu) for name in VM.SCENARIOS for dtype in DTYPES for mu in VM.MUTANTS}


def test_scenarios_cover_the_shapes():
    sc = VM.SCENARIOS.values()
    assert {len(s[3]) for s in sc} >= {1, 2, 3, 8}
    assert {s[0] for s in sc} == {"tiny", "true_dims_1layer"} and {s[2] for s in sc} == {"disjoint", "fork"}
    assert {p for s in sc for p, _ in s[3]} >= {0, 61, 63, 64, 130}
    for cfg, T, layout, seqs in sc:
        assert all(r in (0, 1, T) for _, r in seqs) and seqs[0][1] > 0
        assert layout == "disjoint" or len({p for p, _ in seqs}) == 1
    assert any({r for _, r in s[3]} == {0, 1, s[1]} for s in sc)
    assert 130 // R.PAGE >= 2 * R.decode_split(None, R.MAX_POSITIONS)         # position 130 lies past the first key split


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", VM.MUTANTS)
def test_every_mutant_shows(effects, dtype, mutant):
    hits = {}
    for name in VM.SCENARIOS:
        o, k, v, w = effects[(name, dtype, mutant)]
        if o >= 100.0 or k >= 100.0 or v > 0 or w > 0:
            hits[name] = (o, k, v, w)
    assert hits, f"{mutant}: no scenario moves by 100x the tolerance, an appended row or the written slots"


@pytest.mark.parametrize("dtype", DTYPES)
def test_output_mutants_move_outputs(effects, dtype):
    """the mutants that misroute what a sequence READS must show in the outputs themselves, not only in the pool"""
    for mutant in ("table0", "pos0", "q0", "part0"):
        best = max(effects[(name, dtype, mutant)][0] for name in VM.SCENARIOS)
        assert best >= 100.0, (mutant, best)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_mutants_change_the_written_slots(effects, dtype):
    for mutant in ("zero_rows_append", "append_all_slots", "append_shared", "rows0"):
        assert max(effects[(name, dtype, mutant)][3] for name in VM.SCENARIOS) > 0, mutant


def test_the_model_without_a_mutant_is_the_single_sequence_reference():
    for name in VM.SCENARIOS:
        out, K, V, W = VM.launch(name, torch.bfloat16)
        for z, (P, Rz) in enumerate(VM.SCENARIOS[name][3]):
            assert bool(torch.isnan(out[z, Rz:]).all())
            if Rz:
                ref, tol = VM.reference(name, torch.bfloat16, z)
                assert float(((out[z, :Rz] - ref).abs() / tol).amax()) <= 1e-6, (name, z)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(VM.SCENARIOS))
def test_full_sequences_are_sharp_alone(name, dtype):
    cfg, T, layout, seqs = VM.SCENARIOS[name]
    for z, (P, Rz) in enumerate(seqs):
        if Rz != T:
            continue
        ratios = VR.mutant_ratios(VM.cases(name, dtype)[z])
        weak = {k: round(v, 1) for k, v in ratios.items() if not v >= 10.0}
        assert not weak, f"{name} sequence {z}: mutants within 10x the tolerance: {weak}"
