"""The packed GEMVs' deeper stream (gemv.hip: WP12::DEPTH, deep_step) on the GPU: svln_op_gemv_packed is bit-equal to svln_op_gemv ON THE
SAME ARGUMENTS -- the comparison of tests/test_p12_gpu.py -- at every load-step geometry of the two kernels (blocks per wave from one to
two steps and a remainder, ragged last blocks) with fallback blocks planted at every slot of a step, in the remainder, across a step
boundary, over a whole row, in the ragged block and nowhere, on one row of a row group and on all of them, and with NaN / -0 / denormal
weights in the packed blocks next to a fallback (tests/p12_depth_ref.py; tests/test_p12_depth_inputs.py proves the plans on the CPU).
Every case first shows that the GPU encoder produces the planted records."""
import numpy as np
import pytest

import p12_depth_ref as D
import p12_ref as R
from test_p12_gpu import _gemv, engine, gpu_pack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.id)
def test_packed_gemv_is_bit_equal_to_the_bf16_gemv_at_depth(case):
    case.build()                                    # (asserts on the CPU that the encoder's masks and fallback count are the plan)
    m = engine()
    packed, rec, n_fb, dev = gpu_pack(m, case.w)
    assert np.array_equal(rec, case.rec) and np.array_equal(packed, case.packed) and n_fb == case.n_fb
    dv = lambda t: None if t is None else t.cuda()
    args = (dv(case.x), dv(case.g), dv(case.b), dv(case.r))
    tok_p, out_p = _gemv(m, case, dev, True, *args)
    tok_b, out_b = _gemv(m, case, dev, False, *args)
    if case.epi == "argmax":
        assert tok_p == tok_b == min(case.ties), (case.id, tok_p, tok_b)
        return
    bad = out_p != out_b
    assert not bad.any(), f"{case.id}: {int(bad.sum())} of {bad.size} outputs differ in their bits, first at {int(np.nonzero(bad)[0][0])}"
    if "special_nan" in case.patterns_present and -(-case.K // R.BLOCK) > 1:
        assert np.isnan(R.f32_of(out_p)).any()       # the NaNs really went through
