"""CPU proof that the step-kernel cases of tests/step_ref.py are sharp (no GPU): every case has a decided outcome, the case list covers what
it claims, and each mutant of the restatement is rejected by at least one case, on an output that tests/test_step_gpu.py compares bit for
bit (never on a score value alone)."""
import math

import numpy as np
import pytest

import step_ref as R

CASES = R.all_cases()


def test_every_case_has_a_decided_outcome():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    for c in CASES:
        R.check_decided(c)
        for s in range(c.steps):
            # no two candidates for the winner closer than an exact tie: the live values are multiples of 1/4, so the gap below the top is
            # 0 (a planted tie, decided by the index) or at least 1/4
            live = c.pv[s][(c.pi[s] != R.NONE) & ~np.isnan(c.pv[s])].astype(np.float64)
            fin = live[np.isfinite(live)]
            if fin.size > 1:
                d = fin.max() - fin
                assert np.all((d == 0) | (d >= 0.25)), c.name
        o = R.run(c)
        assert o.ctl[3] - c.count <= c.steps and o.ctl[3] <= c.rows
        for v in o.scores:                                   # a score is NaN only for token -1
            if v is not None and math.isnan(v):
                assert -1 in o.out_ids, c.name


def test_case_list_covers_the_sizes_and_edges():
    by = lambda pred: [c for c in CASES if pred(c)]
    assert {c.n for c in CASES} >= set(R.NS)
    for n in R.NS:
        for form in R.FORMS:
            assert by(lambda c: c.n == n and c.form == form and c.steps == 1), (n, form)
    # ties across the two halves of each of the eight reduction levels, both placements of the lower index
    for n in (256, 257, 1024, 2048):
        for s in (128, 64, 32, 16, 8, 4, 2, 1):
            for side in ("hi", "lo"):
                assert by(lambda c: c.name.startswith(f"level{s}-{side}-n{n}-")), (n, s, side)
    assert by(lambda c: c.name.startswith("trips0-hi-n257")) and by(lambda c: c.name.startswith("trips255-hi-n1024"))
    assert by(lambda c: c.name.startswith("trips3-"))
    # all-empty rows: token -1, done, count + 1, no flag, no advance, NaN score
    for c in by(lambda c: c.name.startswith("all-empty")):
        o = R.run(c)
        assert o.ctl == (c.pos, c.kv_len, 1, c.count + 1, c.max_new) and o.out_ids[c.count] == -1 and o.last_token == -1
        assert bytes(o.flags) == bytes([R.SENT_FLAG]) * c.flag_bytes and c.flag_bytes
        assert c.form == "plain" or math.isnan(o.scores[c.count])
    # EOS list lengths and hit positions: index 0, the last index, index 256 (the second trip of the 256-thread loop)
    assert {len(c.eos) for c in CASES} >= set(R.N_EOS)
    for n_eos in (257, 300):
        for hit in (0, 256, n_eos - 1):
            assert by(lambda c: c.name.startswith(f"eos{n_eos}-hit{hit}-")), (n_eos, hit)
    for c in by(lambda c: "-hit" in c.name):
        o = R.run(c)
        assert o.ctl == (c.pos, c.kv_len, 1, c.count + 1, c.max_new), c.name            # appended, never fed
    for c in by(lambda c: "-miss" in c.name or c.name.startswith("max_new-one-short")):
        o = R.run(c)
        assert o.ctl == (c.pos + 1, c.kv_len + 1, 0, c.count + 1, c.max_new), c.name
    # done on entry: every output keeps its sentinel
    for c in by(lambda c: c.name.startswith("done-on-entry")):
        o = R.run(c)
        assert o.ctl == (c.pos, c.kv_len, 1, c.count, c.max_new) and set(o.out_ids) == {R.SENT_ID} and o.last_token == R.SENT_ID
        assert o.out_top is None and set(o.scores) == {None} and set(o.flags) == {R.SENT_FLAG}
    # sequences of 2 .. 6 launches that end in the middle: the launches behind the end are no-ops
    for steps in (2, 3, 4, 5, 6):
        ended = by(lambda c: c.steps == steps and c.name.startswith(f"seq{steps}-") and "runs-on" not in c.name)
        assert {R.run(c).ctl[3] - c.count for c in ended} == set(range(1, steps)), steps
        for c in ended:
            o = R.run(c)
            assert o.ctl[2] == 1 and all(v == R.SENT_ID for v in o.out_ids[o.ctl[3]:]) and all(v is None for v in o.scores[o.ctl[3]:])


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_rejected(mut):
    """on the bit-exact outputs alone: the scores enter the key as values of the same float64 function, so they differ only by their row"""
    killers = [c.name for c in CASES if R.run(c, mut).key() != R.run(c).key()]
    assert killers, mut
    print(f"{mut}: rejected by {len(killers)} of {len(CASES)} cases, e.g. {killers[0]}")


def test_fp32_prompt_seed_gives_six_distinct_tokens_on_the_cpu_oracle():
    """the condition on the inputs of tests/test_dead_step_gpu.py (2), checked without a GPU for the fp32 greedy base: the free run's
    first six ids are pairwise distinct, each by a top-2 margin far above the fp32 engine's error"""
    import torch

    import test_dead_step_gpu as D
    from oracle import streamvln_oracle as O
    from scenarios import SEED
    from streamvln_amd import weights as W
    from streamvln_amd.config import TINY

    w = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in W.synth_state_dict(TINY, SEED).items()}
    assert D.SEEDS["fp32"] == D.SEEDS["fp32-nograph"]
    emb = w["model.embed_tokens.weight"]
    cache = O.KVCache(TINY.layers)
    with torch.no_grad():
        h = O.qwen2_forward(w, TINY, emb[torch.from_numpy(D.prompt(D.SEEDS["fp32"]))], 0, cache)[-1]
        out, margins = [], []
        for _ in range(9):
            tok, margin = O.greedy_pick(O.lm_logits(w, h))
            out.append(tok)
            margins.append(margin)
            h = O.qwen2_forward(w, TINY, emb[tok][None], len(cache), cache, None, "decode")[-1]
    print("oracle free run", out, "margins", [f"{x:.3g}" for x in margins])
    assert len(set(out[:6])) == 6, out
    assert min(margins[:6]) > 1e-3, margins


def test_host_surface_of_the_two_entries():
    """the header declares both test-only entries, the ctypes table binds them with the declared argument counts, the library exports
    them, and the ctypes mirror of svln_argmax_step_op names the header's fields in the header's order"""
    import os
    import re
    import subprocess

    from streamvln_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "streamvln_hip.h")).read()
    for name, n_args in {"svln_op_argmax_step": 2, "svln_op_dead_step": 5}.items():
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", header)
        assert m and m.group(1).count(",") + 1 == n_args, name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == n_args, name
    body = re.search(r"typedef struct svln_argmax_step_op \{(.*?)\} svln_argmax_step_op;", header, re.S).group(1)
    fields = [re.sub(r"[\s*]", "", f.split()[-1]) for decl in body.split(";") for f in decl.split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.SvlnArgmaxStepOp._fields_], fields
    ptrs = [n for n, t in _lib.SvlnArgmaxStepOp._fields_ if t is _lib.C.c_void_p]
    assert ptrs == fields[:len(ptrs)] and all(t is _lib.C.c_int32 for _, t in _lib.SvlnArgmaxStepOp._fields_[len(ptrs):])
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"svln_op_argmax_step", "svln_op_dead_step"} <= set(re.findall(r" T (svln_[a-z0-9_]+)", nm))


def test_mutants_named_by_the_issue_are_all_there():
    want = {"tie_highest_index", "tie_first_partial", "eos_fed", "stop_before_increment", "flag_for_minus_one", "score_at_next_row",
            "runner_up_distinct", "eos_scan_256", "works_when_done"}
    assert set(R.MUTANTS) == want
