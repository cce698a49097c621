"""The opt-in MXFP4 decode weights (svln_set_mxfp4_decode; NO reference counterpart: the reference is bf16 only) against the same
numeric scheme restated on the CPU (tests/mxfp4_ref.py): OCP MX blocks of 32 E2M1 elements with one E8M0 scale byte.

  quantiser   bytes and scale bytes EQUAL to the restatement (-0 folded onto +0), also where the block exponent clamps, in a thread's
              second loop iteration, and with NaN / inf elements: such a block gets the scale byte 0xFF and its codes are masked.  How the
              GEMVs consume a scale byte 0xFF is out of scope here.
  GEMV        against the fp32 product over the DEQUANTISED weights: both sides multiply identical values, so what is left is fp32
              summation order and one bf16 rounding -- the bound util.assert_close is defined for.
  end to end  weight-only, so engine and emulation (mxfp4_ref.Mxfp4Emu) see the same quantised operands: every comparable hidden row --
              decode rows included -- is held at the bf16 engine's own bound (test_fp8_gpu.W8_REL), ids wherever the emulation's top-2
              margin exceeds test_fp8_gpu.MARGIN.  Teacher-forced on the token level exactly as tests/test_fp8_gpu.py: the engine runs
              first, the emulation then decodes the ENGINE'S tokens.
"""
import ctypes as C
import gc
import math
import time

import numpy as np
import pytest
import torch

import mxfp4_ref as R
from oracle import streamvln_oracle as O
from scenarios import SCENARIOS, SEED, apply_knobs, run_scenario
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from test_e2e_gpu import _model, _note, _run
from test_fp8_gpu import MARGIN, W8_REL, _rel
from util import assert_close, ptr, q, rnd, synth_weights

pytestmark = pytest.mark.gpu
_engines = {}


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def chk(rc):
    _lib.check(rc)


def _gpu_quant(m, W):
    rows, cols = W.shape
    dW = W.to(torch.bfloat16).cuda()
    q4 = torch.full((rows, cols // 2), 0xAA, dtype=torch.uint8, device="cuda")
    e8 = torch.full((rows, cols // 32), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    chk(m._lib.svln_op_quant_mxfp4(m._h, ptr(dW), rows, cols, ptr(q4), ptr(e8)))
    return q4.cpu(), e8.cpu()


def _tie_matrix():
    """every tie of the scheme (and its neighbours) times assorted powers of two, positive and negative; each block also holds a 6 * 2^k
    so that its scale is 2^k and the ties are ties of the element grid"""
    vals = [5.0, 3.5, 2.5, 1.75, 1.25, 0.75, 0.25, 7.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 5.5, 4.5, 0.125, 0.375, 7.5, 2.25, 2.75, 0.625, 0.875]
    rows = []
    for k in (-30, -14, -9, -1, 0, 1, 6, 17):
        for sign in (1.0, -1.0):
            row = torch.zeros(64)
            row[:len(vals)] = torch.tensor(vals) * sign
            row[31] = 6.0
            row[32:32 + len(vals)] = torch.tensor(vals) * -sign          # second block: no 6, amax 7.5 (same exponent)
            rows.append(row * 2.0 ** k)
    W = torch.stack(rows)
    assert torch.equal(q(W, torch.bfloat16), W)                          # every value is a bf16 value
    return W


def test_quantiser_bytes_equal_the_cpu_restatement():
    m = engine(torch.bfloat16)
    cases = [(f"{r}x{c} sd {sd}", q(rnd((r, c), 31, sd), torch.bfloat16)) for r, c, sd in [(515, 3584, 0.02), (64, 18944, 0.5), (3, 32, 1.0)]]
    Wz = q(rnd((9, 256), 32, 0.1), torch.bfloat16)
    Wz[4] = 0.0                                                          # all-zero row: e8 = 127, bytes 0
    Wz[6, 32:64] = 0.0                                                   # and an all-zero block inside a row
    cases += [("all-zero row", Wz), ("ties", _tie_matrix())]
    for what, W in cases:
        codes, e8 = R.quant_mxfp4(W)
        gq, ge = _gpu_quant(m, W)
        assert torch.equal(ge, e8), f"{what}: {int((ge != e8).sum())} of {e8.numel()} scale bytes differ"
        got, exp = R.fold_zero(gq), R.fold_zero(codes)
        assert torch.equal(got, exp), f"{what}: {int((got != exp).sum())} of {exp.numel()} bytes differ"
    gq, ge = _gpu_quant(m, Wz)
    assert int(gq[4].max()) == 0 and ge[4].tolist() == [127] * 8 and int(ge[6, 1]) == 127


def test_quantiser_at_the_exponent_clamps_and_in_the_second_loop_iteration():
    """the ties of the element grid where the block exponent clamps (e8 = 0 from an amax in [2^-126, 2^-125) and from a bf16-subnormal
    amax; e8 = 252 from amax = 1.75 * 2^127) and in blocks 255, 256, 257 of a row of 8256 columns, neighbouring blocks under different
    exponents; tests/test_mxfp4_cpu.py holds the expected bytes to hand-written codes"""
    m = engine(torch.bfloat16)
    Wc, e8_exp = R.clamp_tie_matrix()
    for what, W in (("clamps", Wc), ("wide", R.wide_tie_matrix())):
        codes, e8 = R.quant_mxfp4(W)
        gq, ge = _gpu_quant(m, W)
        assert torch.equal(ge, e8), f"{what}: scale bytes differ at {torch.nonzero(ge != e8).tolist()[:8]}"
        got, exp = R.fold_zero(gq), R.fold_zero(codes)
        assert torch.equal(got, exp), f"{what}: {int((got != exp).sum())} of {exp.numel()} bytes differ, first at {torch.nonzero(got != exp).tolist()[:8]}"
    assert _gpu_quant(m, Wc)[1].tolist() == e8_exp


def test_quantiser_marks_a_block_with_a_nan_or_an_infinity_with_scale_byte_0xff():
    """a block that holds a non-finite element gets E8M0 NaN (0xFF) and unspecified codes (masked); every other block of the row is
    what the restatement makes of it, in a thread's first and second loop iteration"""
    m = engine(torch.bfloat16)
    for what, W, twin, bad in R.nonfinite_matrices():
        codes, e8 = R.quant_mxfp4(W)
        assert {tuple(x) for x in torch.nonzero(e8 == R.E8_NAN).tolist()} == bad
        gq, ge = _gpu_quant(m, W)
        assert torch.equal(ge, e8), f"{what}: scale bytes differ at {torch.nonzero(ge != e8).tolist()[:8]}"
        got, exp = R.fold_zero(R.mask_nonfinite(gq, e8)), R.fold_zero(R.mask_nonfinite(codes, e8))
        assert torch.equal(got, exp), f"{what}: {int((got != exp).sum())} of {exp.numel()} bytes differ"


def _dev(t, dtype=torch.bfloat16):
    return t.to(dtype).cuda() if t is not None else None


@pytest.mark.parametrize("N,K,norm,bias,res", [(4608, 3584, True, True, False), (3584, 18944, False, False, True),
                                               (515, 512, True, False, True), (7, 64, False, True, False), (9000, 3584, False, False, False)])
def test_gemv_mxfp4_weights(N, K, norm, bias, res):
    """MXFP4 weight-only GEMV == the same product over the dequantised weights (fp32 accumulate both sides); shapes and norm / bias /
    residual combinations of test_ops_gpu.py::test_gemv_fp8_weights.  The bytes come from the CPU restatement (the device quantiser is held
    to it byte for byte in the test above); the size of the quantisation error itself is capped in tests/test_mxfp4_cpu.py."""
    dtype = torch.bfloat16
    m = engine(dtype)
    Wt, x = q(rnd((N, K), 41, 1.0 / math.sqrt(K)), dtype), q(rnd((K,), 42), dtype)
    g = q(1 + rnd((K,), 43, 0.1), dtype) if norm else None
    b = q(rnd((N,), 44, 0.1), dtype) if bias else None
    r = q(rnd((N,), 45), dtype) if res else None
    codes, e8 = R.quant_mxfp4(Wt)
    Wd = R.dequant_mxfp4(codes, e8)
    xe = O.rms_norm(x, g, 1e-6) if norm else x
    exp = Wd @ xe
    if b is not None:
        exp = exp + b
    if r is not None:
        exp = exp + r
    dx, dg, db, dr = _dev(x), _dev(g), _dev(b), _dev(r)
    dq, de = codes.cuda(), e8.cuda()
    y = torch.zeros((N,), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    chk(m._lib.svln_op_gemv_mxfp4(m._h, ptr(dq), ptr(de), K, ptr(dx), ptr(dg), 1e-6, ptr(db), ptr(dr), ptr(y), N, K, _lib.EPI_NONE, None))
    assert_close(y, exp, dtype, f"gemv mxfp4 {N}x{K}")


def test_gemv_mxfp4_swiglu_argmax_and_fp32_refusal():
    dtype = torch.bfloat16
    m = engine(dtype)
    I, K = 1024, 512
    x = q(rnd((K,), 46), dtype)
    g = q(1 + rnd((K,), 47, 0.1), dtype)
    gate, up = q(rnd((I, K), 48, 0.08), dtype), q(rnd((I, K), 49, 0.08), dtype)
    packed = torch.zeros((2 * I, K))
    idx = torch.arange(I)
    packed[(idx // 32) * 64 + idx % 32] = gate                   # the [gate 32 | up 32] row packing of the engine's gate/up matrix
    packed[(idx // 32) * 64 + 32 + idx % 32] = up
    codes, e8 = R.quant_mxfp4(packed)
    Wd = R.dequant_mxfp4(codes, e8)
    xe = O.rms_norm(x, g, 1e-6)
    gd, ud = Wd[(idx // 32) * 64 + idx % 32], Wd[(idx // 32) * 64 + 32 + idx % 32]
    exp = O.silu(gd @ xe) * (ud @ xe)
    y = torch.zeros((I,), dtype=dtype, device="cuda")
    dq, de, dx, dg = codes.cuda(), e8.cuda(), _dev(x), _dev(g)
    torch.cuda.synchronize()
    chk(m._lib.svln_op_gemv_mxfp4(m._h, ptr(dq), ptr(de), K, ptr(dx), ptr(dg), 1e-6, None, None, ptr(y), 2 * I, K, _lib.EPI_SWIGLU, None))
    assert_close(y, exp, dtype, "gemv mxfp4 swiglu")
    # arg-max with a planted row (lowest index on ties is torch.argmax's rule; the planted row wins by a wide margin)
    V = 5000
    Wv = q(rnd((V, K), 50, 0.05), dtype)
    Wv[77] = q(x * 0.02, dtype)
    cv, ev = R.quant_mxfp4(Wv)
    logits = R.dequant_mxfp4(cv, ev) @ x
    tok = C.c_int32(-1)
    dcv, dev_ = cv.cuda(), ev.cuda()
    torch.cuda.synchronize()
    chk(m._lib.svln_op_gemv_mxfp4(m._h, ptr(dcv), ptr(dev_), K, ptr(dx), None, 1e-6, None, None, None, V, K, _lib.EPI_ARGMAX, C.byref(tok)))
    assert tok.value == int(torch.argmax(logits)) == 77, tok.value
    # fp32 engines refuse MXFP4 weights, the product and the quantiser alike
    m32 = engine(torch.float32)
    rc = m32._lib.svln_op_gemv_mxfp4(m32._h, ptr(dq), ptr(de), K, ptr(dx), None, 1e-6, None, None, ptr(y), 2 * I, K, _lib.EPI_NONE, None)
    assert rc != 0
    dW = packed.to(torch.bfloat16).cuda()
    rc = m32._lib.svln_op_quant_mxfp4(m32._h, ptr(dW), 2 * I, K, ptr(dq), ptr(de))
    assert rc != 0
    # malformed extents are refused, not run
    rc = m._lib.svln_op_gemv_mxfp4(m._h, ptr(dq), ptr(de), K, ptr(dx), None, 1e-6, None, None, ptr(y), 2 * I, K - 16, _lib.EPI_NONE, None)
    assert rc != 0


def _emulate(cfg, sc, engine_ids, knobs=False):
    """{seed: [(hidden [n, H], margins, own picks, cache_len) per turn]} from Mxfp4Emu decoding the ENGINE'S tokens (`engine_ids`:
    {seed: [ids per turn]}); the episodes run on a thread pool over one shared cache of dequantised copies (as test_fp8_gpu.py)"""
    from concurrent.futures import ThreadPoolExecutor
    sd = synth_weights(cfg, SEED)
    pre = lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb))
    shared = {}

    def episode(seed):
        emu = R.Mxfp4Emu()
        emu._dq = shared
        orc = O.OracleStreamVLN(cfg, sd, num_history=sc["num_history"], fp8=emu)
        if knobs:
            apply_knobs(orc, sc)
        orc.teacher_tokens = [list(t) for t in engine_ids[seed]]
        log = run_scenario(orc, dict(sc, prompt_seed=seed), preprocess=pre)
        assert not orc.teacher_tokens and len(log) == len(engine_ids[seed]), (seed, len(log))
        return seed, [(r["out"].hidden.numpy().copy(), list(r["out"].margins), list(r["out"].own_picks), r["out"].cache_len) for r in log]
    with ThreadPoolExecutor(max_workers=min(len(engine_ids), 6)) as ex:
        out = dict(ex.map(episode, list(engine_ids)))
    del shared
    gc.collect()
    return out


def _compare(what, cfg, eng, emu, bound):
    """every row of every turn under `bound`; ids wherever the emulation's margin exceeds MARGIN.  -> (rows, decode rows, asserted, worst)"""
    rows = dec_rows = asserted = 0
    worst = 0.0
    for seed, (ids_t, taps) in eng.items():
        for t, (gh, margins, picks, clen) in enumerate(emu[seed]):
            assert len(picks) == len(ids_t[t]) == len(gh) and taps[t]["cache_len"] == clen, (what, seed, t)
            for j in range(len(picks)):
                rel = _rel(taps[t]["hidden"][j], gh[j])
                worst = max(worst, rel)
                print(f"{what} seed {seed} turn {t} row {j}: rel L2 {rel:.5f} margin {margins[j]:.4f} engine id {ids_t[t][j]} emulation pick {picks[j]}")
                assert rel < bound, (what, seed, t, j, rel, bound)
                rows += 1
                dec_rows += j > 0
                if margins[j] > MARGIN:
                    assert ids_t[t][j] == picks[j], (what, seed, t, j, ids_t[t], picks, margins)
                    asserted += 1
    line = (f"{cfg.name} MXFP4 decode weights [{what}] vs the emulating oracle (teacher-forced on the engine's tokens): {rows} hidden rows "
            f"({dec_rows} decode rows) all < {bound}, worst rel L2 {worst:.4f}; {asserted} ids with emulation margin > {MARGIN} asserted equal")
    print(line)
    _note("mxfp4_vs_emulation", line)
    return rows, dec_rows, asserted, worst


def test_repetition_penalty_rides_on_the_mxfp4_lm_head():
    """tiny_penalty (generation_config.repetition_penalty = 1.3) with the mode on: the penalty flags are applied inside gemv_rows_kernel<WMxfp4, EPI_ARGMAX>'s
    arg-max epilogue; against Mxfp4Emu with the same knob, teacher-forced."""
    sc = SCENARIOS["tiny_penalty"]
    cfg = sc["cfg"]
    m = _model(sc, torch.bfloat16)
    m.set_mxfp4_decode(True)
    log, taps = _run(m, sc)
    ids = [rec["out"].sequences[0].tolist() for rec in log]
    m.set_mxfp4_decode(False)
    m.close()
    emu = _emulate(cfg, sc, {7: ids}, knobs=True)
    rows, dec_rows, asserted, _ = _compare("tiny_penalty", cfg, {7: (ids, taps)}, emu, W8_REL[cfg.name])
    assert rows >= 16 and dec_rows >= 8, (rows, dec_rows)


def test_switch_semantics_exclusive_modes_and_bit_exact_return_to_bf16():
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    m = _model(sc, torch.bfloat16)
    m.set_decode_graph(True)
    log0, taps0 = _run(m, sc)                                    # bf16, decode graph on, before the mode was ever enabled
    ids0 = [r["out"].sequences[0].tolist() for r in log0]
    # mutually exclusive, refused with a message
    m.set_fp8_decode(True)
    with pytest.raises(_lib.SvlnError, match="e4m3 decode weights are on"):
        m.set_mxfp4_decode(True)
    m.set_fp8_decode(False)
    m.set_mxfp4_decode(True)
    with pytest.raises(_lib.SvlnError, match="MXFP4 decode weights are on"):
        m.set_fp8_decode(True)
    m.set_mxfp4_decode(True)                                     # enabling twice is fine
    m.reset(1)
    log1, taps1 = _run(m, sc)
    # the mode does something: decode rows differ from bf16 (first rows of a turn are prefill rows through the bf16 products)
    assert any(not np.array_equal(a["hidden"][1:], b["hidden"][1:]) for a, b in zip(taps0, taps1) if len(a["hidden"]) == len(b["hidden"]))
    m.set_mxfp4_decode(False)
    m.set_mxfp4_decode(False)                                    # and so is disabling twice
    m.reset(1)
    log2, taps2 = _run(m, sc)
    assert [r["out"].sequences[0].tolist() for r in log2] == ids0
    assert len(taps2) == len(taps0)
    for a, b in zip(taps0, taps2):
        assert np.array_equal(a["hidden"], b["hidden"])          # bit for bit: the default path is unchanged, no stale graph is replayed
    m.close()
    m32 = _model(sc, torch.float32)
    with pytest.raises(_lib.SvlnError):
        m32.set_mxfp4_decode(True)
    m32.close()


@pytest.mark.parametrize("name", ["tiny_episode", "true4_episode"])
def test_mxfp4_decode_vs_emulating_oracle(name):
    """TINY (9 turns through two <memory> restarts, seed 7) and TRUE4 (true width, 4 + 4 layers, vocabulary 152 064, seeds 7 and 11):
    EVERY row of every turn (prefill rows and decode rows) within the bf16 engine's own bound W8_REL, and the engine's token equal to the
    emulation's pick wherever the emulation's top-2 margin exceeds MARGIN."""
    sc = dict(SCENARIOS[name], eos_mod=0)
    cfg = sc["cfg"]
    seeds = (7,) if name == "tiny_episode" else (7, 11)
    m = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, max_envs=1, max_frames=1 + sc["num_history"], max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    m.set_mxfp4_decode(True)
    eng = {}
    for seed in seeds:
        m.reset(1)
        log, taps = _run(m, dict(sc, prompt_seed=seed))
        eng[seed] = ([rec["out"].sequences[0].tolist() for rec in log], taps)
    m.set_mxfp4_decode(False)
    m.close()
    emu = _emulate(cfg, sc, {k: v[0] for k, v in eng.items()})
    rows, dec_rows, asserted, worst = _compare(name, cfg, eng, emu, W8_REL[cfg.name])
    assert dec_rows >= 1 and rows > dec_rows, (rows, dec_rows)            # decode rows were compared
    assert rows >= (16 if name == "tiny_episode" else 12) and dec_rows >= (8 if name == "tiny_episode" else 9), (rows, dec_rows)


def test_mxfp4_full_depth_decode_weights_vs_emulating_oracle():
    """The benchmarked instantiation (26 + 28 layers, true width) with MXFP4 decode weights against the emulation run live: the first turn
    (T = 376) with 6 tokens, 5 of the 6 rows decode rows, teacher-forced on the engine's tokens; same form and bound as
    test_fp8_gpu.py::test_fp8_full_depth_decode_weights_vs_emulating_oracle."""
    from streamvln_amd.config import TRUE
    sc = dict(SCENARIOS["true4_episode"], cfg=TRUE, steps=4, max_new=6, eos_mod=0)
    m = StreamVLNForCausalLM(TRUE, dtype=torch.bfloat16, max_envs=1, max_frames=9, max_positions=4096)
    m.load_synthetic(SEED)
    m.model.num_history = 8
    m.set_mxfp4_decode(True)
    log, taps = _run(m, dict(sc, prompt_seed=7))
    m.close()
    assert len(log) == 1
    ids = log[0]["out"].sequences[0].tolist()
    t0 = time.time()
    orc = O.OracleStreamVLN(TRUE, synth_weights(TRUE, SEED), num_history=sc["num_history"], fp8=R.Mxfp4Emu())
    orc.teacher_tokens = [list(ids)]
    olog = run_scenario(orc, dict(sc, prompt_seed=7), preprocess=lambda rgb: torch.from_numpy(O.siglip_preprocess(rgb)))
    t_o = time.time() - t0
    gh, margins, picks = olog[0]["out"].hidden.numpy(), list(olog[0]["out"].margins), list(orc.own_picks)
    assert olog[0]["out"].sequences[0].tolist() == ids and len(picks) == len(ids) == 6
    assert taps[0]["cache_len"] == olog[0]["out"].cache_len
    del orc, olog
    gc.collect()
    worst, asserted = 0.0, 0
    for j in range(len(ids)):
        rel = _rel(taps[0]["hidden"][j], gh[j])
        worst = max(worst, rel)
        print(f"full depth row {j}: rel L2 {rel:.5f} margin {margins[j]:.4f} engine id {ids[j]} emulation pick {picks[j]}")
        assert rel < W8_REL[TRUE.name], (j, rel)
        if margins[j] > MARGIN:
            assert ids[j] == picks[j], (j, ids, picks, margins)
            asserted += 1
    line = (f"full depth, MXFP4 decode weights vs the emulating oracle (teacher-forced on the engine's tokens): {len(ids)} rows ({len(ids) - 1} decode rows) < "
            f"{W8_REL[TRUE.name]}, worst rel L2 {worst:.4f}; {asserted} ids with margin > {MARGIN} equal; margins {[round(x, 3) for x in margins]}; oracle {t_o:.0f} s")
    print(line)
    _note("mxfp4_vs_emulation", line)
