"""The e4m3 products on the block-scaled MFMAs (svln_set_fp8_scaled_mfma; svln_op_gemm_fp8 with force_cfg | 0x40000): the stage-ring
kernels on v_mfma_scale_f32_32x32x64_f8f6f4 and the 8-phase 256x256 schedule on v_mfma_scale_f32_16x16x128_f8f6f4, neutral block scales.

  exact cases   tests/fp8s_ref.py (tests/test_fp8_scaled_inputs.py proves them sharp on the CPU): the stored bits, between guard rows, over
                poisoned padding and dirty slabs, twice -- the harness of tests/test_gemm_gpu.py.  The instruction's operand lane map is
                not documented: the sign family pins which bytes meet which, the alphabet family the decode.
  one random product at K = 3584 per form against float64 of the same bytes, under gemm_ref.bound.
  engine level  TINY, mode `gemm` with the switch on, teacher-forced against the emulating oracle exactly as
                test_fp8_gpu.test_fp8_modes_vs_emulating_oracle (the numeric scheme is unchanged, so are the oracle and the bounds); four
                envs in lockstep with the decode graph on, in both forms in turn: each form replays its own captured graph.
  the switch    refused on an fp32 engine, refused while turns are in flight, a call that changes nothing always succeeds."""

import numpy as np
import pytest
import torch

import fp8s_ref as S
import gemm_ref as R
import test_gemm_gpu as G
from scenarios import SCENARIOS, SEED
from streamvln_amd import _lib
from streamvln_amd.model import StreamVLNForCausalLM
from test_e2e_gpu import _note, _run
from test_fp8_gpu import MARGIN_W8A8, W8A8_REL, _emulate_teacher_forced, _rel
from util import ptr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_scaled_gemm_cases(case):
    assert case.force_cfg & S.SCALED
    G.test_gemm_cases(case)


@pytest.mark.parametrize("form", ["ring", "p8", "heuristic"])
def test_scaled_random_product_k3584(form):
    """random e4m3 operands (normal draws scaled to the format's range, per-row scales) at the K of the LLM's q|k|v / o / gate|up products"""
    M, N, K = 293, 331, 3584
    cfg = {"ring": 256 | R.RING, "p8": 256, "heuristic": 0}[form] | S.SCALED
    tile = R.plan(True, True, M, N, K, "none", cfg)["cfg"]
    assert tile == {"ring": "big", "p8": "p8", "heuristic": "c256"}[form]
    g = torch.Generator().manual_seed(3584)
    A8 = (torch.randn((M, K), generator=g) * 64).clamp(-448, 448).to(torch.float8_e4m3fn)
    W8 = (torch.randn((N, K), generator=g) * 64).clamp(-448, 448).to(torch.float8_e4m3fn)
    sa, sw = torch.rand((M,), generator=g) * 0.01 + 0.002, torch.rand((N,), generator=g) * 0.01 + 0.002
    bias = torch.randn((N,), generator=g).to(torch.bfloat16)
    exp = (A8.float().double() @ W8.float().double().t()) * sa.double()[:, None] * sw.double()[None] + bias.double()[None]
    m = G.engine(torch.bfloat16)
    out = torch.full((M, N), R.FILL, dtype=torch.bfloat16, device="cuda")
    d = [t.cuda() for t in (A8.view(torch.uint8), sa, W8.view(torch.uint8), sw, bias)]
    torch.cuda.synchronize()
    _lib.check(m._lib.svln_op_gemm_fp8(m._h, ptr(d[0]), ptr(d[1]), K, ptr(d[2]), ptr(d[3]), K, ptr(out), N, ptr(d[4]), None, 0, M, N, K, _lib.EPI_NONE, cfg, 0))
    torch.cuda.synchronize()
    err = (out.cpu().double() - exp).abs()
    bound = R.bound(exp, torch.bfloat16)
    print(f"scaled e4m3 product {M} x {N} x {K} on {tile}: max err / bound {float((err / bound).max()):.3f}, |exp| max {float(exp.abs().max()):.3f}")
    assert bool((err <= bound).all()), (form, float((err / bound).max()))


def test_scaled_form_vs_emulating_oracle():
    """test_fp8_modes_vs_emulating_oracle's `gemm` mode on TINY (seed 7) with the scaled form on: every row of every turn under W8A8_REL, ids
    wherever the emulation's margin exceeds MARGIN_W8A8"""
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    cfg = sc["cfg"]
    m = StreamVLNForCausalLM(cfg, dtype=torch.bfloat16, max_envs=1, max_frames=1 + sc["num_history"], max_positions=2048)
    m.load_synthetic(SEED)
    m.model.num_history = sc["num_history"]
    m.set_fp8_scaled_mfma(True)                       # (before the mode: no effect until svln_set_fp8_gemm is on)
    m.set_fp8_gemm(True)
    log, taps = _run(m, dict(sc, prompt_seed=7))
    m.set_fp8_gemm(False)
    m.set_fp8_scaled_mfma(False)
    m.close()
    ids_t = [rec["out"].sequences[0].tolist() for rec in log]
    emu = _emulate_teacher_forced(cfg, sc, {("gemm", 7): ids_t})[("gemm", 7)]
    rows = dec_rows = asserted = 0
    worst = 0.0
    for t, (gh, margins, picks, clen) in enumerate(emu):
        assert len(picks) == len(ids_t[t]) == len(gh) and taps[t]["cache_len"] == clen, t
        for j in range(len(picks)):
            rel = _rel(taps[t]["hidden"][j], gh[j])
            worst = max(worst, rel)
            assert rel < W8A8_REL[cfg.name], (t, j, rel)
            rows += 1
            dec_rows += j > 0
            if margins[j] > MARGIN_W8A8:
                assert ids_t[t][j] == picks[j], (t, j, ids_t[t], picks, margins)
                asserted += 1
    line = (f"{cfg.name} fp8 mode 'gemm' on the block-scaled MFMAs vs the emulating oracle: {rows} hidden rows ({dec_rows} decode rows) all < "
            f"{W8A8_REL[cfg.name]}, worst rel L2 {worst:.4f}; {asserted} ids with emulation margin > {MARGIN_W8A8} asserted equal")
    print(line)
    _note("fp8_scaled_vs_emulation", line)
    assert rows >= 16 and dec_rows >= 8, (rows, dec_rows)


def test_scaled_form_batched_graphs_and_switch():
    """four envs in lockstep (decode steps on the 32x128 tile, decode graph on) with svln_set_fp8_gemm: unscaled, scaled, unscaled, scaled.
    A form gives the same bits every time it runs -- the graph captured in the other form is never replayed for it -- and the two forms,
    the same sums in another order, stay within the scheme's own bound of each other.  Then the switch's refusals."""
    from test_mx4b_e2e_gpu import _agents, _lockstep, _model
    from streamvln_amd.agent import AsyncBatchedAgents
    from streamvln_amd.synthetic import synthetic_frame
    sc = dict(SCENARIOS["tiny_episode"], eos_mod=0)
    N = 4
    m = _model(sc, N)
    m.set_decode_graph(True)
    m.set_fp8_gemm(True)
    runs = []
    for on in (False, True, False, True):
        m.set_fp8_scaled_mfma(on)
        m.set_fp8_scaled_mfma(on)                                    # twice is fine
        m.reset(N)
        runs.append(_lockstep(m, sc, N, 8))
    for a, b in ((0, 2), (1, 3)):
        assert runs[a][0] == runs[b][0], (a, b)
        for e in range(N):
            assert len(runs[a][1][e]) == len(runs[b][1][e]) == 2
            for x, y in zip(runs[a][1][e], runs[b][1][e]):
                assert np.array_equal(x, y), (a, b, e)
    worst = 0.0
    for e in range(N):                  # rows are comparable while both forms fed the same tokens: always the first row of the first turn
        same = True
        for t, (x, y) in enumerate(zip(runs[0][1][e], runs[1][1][e])):
            ia, ib = runs[0][0][e][t], runs[1][0][e][t]
            for j in range(min(len(x), len(y))):
                if same:
                    worst = max(worst, _rel(x[j], y[j].astype(np.float64)))
                same = same and j < len(ia) and j < len(ib) and ia[j] == ib[j]
    print(f"four envs in lockstep, scaled against unscaled e4m3 form: worst rel L2 of a hidden row {worst:.5f}")
    assert worst < W8A8_REL[sc["cfg"].name], worst
    # refused while a turn is in flight, either way; a call that changes nothing is accepted
    m.set_fp8_scaled_mfma(False)
    m.reset(N)
    agents = _agents(m, sc, N, m.get_vision_tower().image_processor.preprocess_array, "cuda")
    group = AsyncBatchedAgents(agents)
    group.tick([synthetic_frame(i, agents[i].step_id) for i in range(N)], active={0})      # env 0 submits its first turn
    assert group.waiting
    with pytest.raises(_lib.SvlnError, match="in flight"):
        m.set_fp8_scaled_mfma(True)
    m.set_fp8_scaled_mfma(False)
    m.cancel()
    m.set_fp8_scaled_mfma(True)                                      # idle again: accepted
    m.close()
    m32 = _model(sc, 1, torch.float32)
    with pytest.raises(_lib.SvlnError, match="bf16"):
        m32.set_fp8_scaled_mfma(True)
    m32.set_fp8_scaled_mfma(False)                                   # changes nothing: accepted
    m32.close()
