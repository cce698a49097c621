"""The greedy loop's step kernel at op level (launch_argmax_step / launch_argmax_final: argmax_final_kernel with and without GenCtl), through
the test-only entry svln_op_argmax_step, on the exact cases of tests/step_ref.py (tests/test_step_inputs.py proves them sharp on the CPU;
no case is skipped here).  Every case runs in the plain, the scored and the sampled form of the kernel.

  * the final GenCtl, out_ids, the last token, out_top, the flag bytes and WHICH score rows were written are the restatement's bit for
    bit; an output the restatement leaves alone keeps the entry's sentinel (-7, NaN, 0x5A);
  * a written score lies within step_ref.TOL (= scores_ref.TOL = sample_ref.TOL, the bound those merges carry) of float64, NaN for
    token -1, and is bit-equal to what launch_argmax_final (use_ctl = 0) returns on the same partial set, as are token and out_top;
  * every malformed call is refused before any launch, and the engine's own generation state is what it was afterwards.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import step_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM

pytestmark = pytest.mark.gpu
F = np.float32
_engines = {}
WORST = {}


def engine(dtype=torch.float32):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def call(m, case, use_ctl=1, sets=None, rc_only=False, **over):
    """svln_op_argmax_step on the case (sets: the launches to keep, default all) -> dict of everything it returns"""
    sel = list(range(case.steps)) if sets is None else sets
    arr = {k: (None if getattr(case, k) is None else np.ascontiguousarray(getattr(case, k)[sel])) for k in ("pv", "pi", "ps", "pr", "pm")}
    eos = np.asarray(case.eos, dtype=np.int64)
    rows = over.get("rows", case.rows)
    out = {"ctl": np.full(8, -7, np.int32), "ids": np.full(max(rows, 1), -99, np.int32), "tok": np.full(1, -99, np.int32),
           "top": np.zeros(2, F), "scores": np.zeros(max(rows, 1), F), "flags": np.zeros(max(case.flag_bytes, 1), np.uint8)}
    op = _lib.SvlnArgmaxStepOp(part_val=_p(arr["pv"]), part_idx=_p(arr["pi"]), part_sum=_p(arr["ps"]), part_raw=_p(arr["pr"]), part_max=_p(arr["pm"]),
                               eos=_p(eos) if len(eos) else None, ctl_out=_p(out["ctl"]), out_ids=_p(out["ids"]), last_token=_p(out["tok"]),
                               out_top=_p(out["top"]), scores=_p(out["scores"]), flags=_p(out["flags"]) if case.flag_bytes else None,
                               n=case.n, steps=len(sel), use_ctl=use_ctl, pos=case.pos, kv_len=case.kv_len, done=case.done, count=case.count,
                               max_new=case.max_new, n_eos=len(eos), flag_bytes=case.flag_bytes, rows=rows)
    for k, v in over.items():
        setattr(op, k, v)
    rc = m._lib.svln_op_argmax_step(m._h, C.byref(op))
    if rc_only:
        return rc
    _lib.check(rc)
    return out


def _bits(v):
    return np.asarray(v, F).view(np.uint32).tolist()


def _check(m, case):
    want = R.run(case)
    got = call(m, case)
    assert tuple(got["ctl"][:5].tolist()) == want.ctl and got["ctl"][5] == len(case.eos), (case.name, got["ctl"].tolist(), want.ctl)
    assert got["ids"].tolist() == want.out_ids, (case.name, got["ids"].tolist(), want.out_ids)
    assert int(got["tok"][0]) == want.last_token, (case.name, int(got["tok"][0]), want.last_token)
    if want.out_top is None:
        assert np.isnan(got["top"]).all(), (case.name, got["top"])
    else:
        assert _bits(got["top"]) == _bits(want.out_top), (case.name, got["top"].tolist(), want.out_top)
    if case.flag_bytes:
        assert got["flags"].tobytes() == bytes(want.flags), (case.name, np.nonzero(got["flags"] != R.SENT_FLAG)[0].tolist())
    live = [(s, case.count + s) for s in range(want.ctl[3] - case.count)]      # (launch, row) of every launch that did its work
    assert not (case.done and live)
    for row, ref in enumerate(want.scores):
        g = float(got["scores"][row])
        if ref is None or math.isnan(ref):
            assert math.isnan(g), (case.name, row, g, ref)
        else:
            err = abs(g - ref)
            WORST[case.form] = max(WORST.get(case.form, 0.0), err)
            assert err <= R.TOL, (case.name, row, g, ref, err)
    # the same bits as launch_argmax_final on every live launch's own partial set
    for s, row in live:
        fin = call(m, case, use_ctl=0, sets=[s])
        tok, top, sc = R.run_final(R.Case("x", [(case.pv[s], case.pi[s])], case.form))
        assert int(fin["tok"][0]) == tok == want.out_ids[row], (case.name, s)
        assert _bits(fin["top"]) == _bits(top), (case.name, s)
        assert fin["ids"].tolist() == [R.SENT_ID] * case.rows, (case.name, s)
        assert not case.flag_bytes or (fin["flags"] == R.SENT_FLAG).all(), (case.name, s)
        assert tuple(fin["ctl"][:5].tolist()) == (case.pos, case.kv_len, case.done, case.count, case.max_new), (case.name, s)    # no GenCtl: untouched
        if case.form != "plain":
            assert _bits(fin["scores"][0]) == _bits(got["scores"][row]), (case.name, s, float(fin["scores"][0]), float(got["scores"][row]))
            assert np.isnan(fin["scores"][1:]).all()
        else:
            assert np.isnan(fin["scores"]).all()
        if s == live[-1][0]:
            assert _bits(fin["top"]) == _bits(got["top"]) and int(fin["tok"][0]) == int(got["tok"][0])


@pytest.mark.parametrize("n", R.NS)
def test_argmax_cases(n):
    """ties within a thread's trips and across the halves of every reduction level, the lower index in the higher partial, three-way ties,
    owns-nothing partials, NaN, +inf and all-empty rows, at every partial count an lm_head hands the kernel"""
    m = engine()
    cases = [c for c in R.argmax_cases() if c.n == n]
    assert cases
    for c in cases:
        _check(m, c)
    print(f"n = {n}: {len(cases)} cases; worst |score - float64| so far {WORST}")


@pytest.mark.parametrize("form", R.FORMS)
def test_step_cases(form):
    """EOS lists of 0 .. 300 ids with the hit at index 0, at the last index and at 256, the max_new edge from both sides, done on entry,
    and sequences of 2 .. 6 launches that end in the middle: the later launches are no-ops"""
    m = engine()
    cases = [c for c in R.step_cases() if c.form == form]
    assert cases
    for c in cases:
        _check(m, c)
    print(f"{form}: {len(cases)} cases; worst |score - float64| so far {WORST}")


def test_bf16_engine_runs_the_same_kernel():
    """the step kernel has no engine-dtype parameter: a sample of the cases on the bf16 engine"""
    m = engine(torch.bfloat16)
    for c in R.all_cases()[::17]:
        _check(m, c)


def test_malformed_calls_are_refused_and_the_engine_state_is_kept():
    m = engine()
    c = next(c for c in R.step_cases() if c.name.startswith("seq3-eos-at0-smp"))
    state = lambda: (m.env_state(0), )
    s0 = state()
    assert call(m, c, rc_only=True) == 0
    bad = [dict(n=0), dict(n=2049), dict(steps=0), dict(steps=9), dict(count=-1), dict(count=c.rows), dict(count=c.rows - c.steps + 1),
           dict(rows=0), dict(rows=2048 + 9), dict(part_val=None), dict(part_idx=None), dict(part_max=None), dict(part_raw=None),
           dict(part_sum=None), dict(ctl_out=None), dict(out_ids=None), dict(last_token=None), dict(out_top=None), dict(scores=None),
           dict(flags=None), dict(eos=None), dict(n_eos=-1), dict(n_eos=1 << 20), dict(flag_bytes=-1), dict(flag_bytes=100)]
    for over in bad:
        assert call(m, c, rc_only=True, **over) != 0, over
        assert b"op_argmax_step" in m._lib.svln_last_error() or b"null" in m._lib.svln_last_error(), (over, m._lib.svln_last_error())
    assert m._lib.svln_op_argmax_step(m._h, None) != 0
    assert call(m, c, rc_only=True) == 0 and state() == s0
