"""Truncated sampling at op level (svln_sampling_truncation): truncate_partials_kernel and the batched sampled final kernel through the
test-only entry svln_op_truncate, on the cases of tests/trunc_ref.py (tests/test_trunc_inputs.py proves them sharp on the CPU; no case
is skipped here): n_part of 1, 2, 5, 1024, 1025, 2048 (the <32> / <64> register forms on both sides of 8192 candidates), c of 1 and 8,
B of 1, 2, 8, 32, top_k of 1, 2, 5, 8, top_p of 1, 0.55, 2^-20.

  * the partial rows: part_idx, part_raw, part_max and part_sum bit-equal to the restatement, part_val within 2^-18 max(1, |G|) of
    y + G64; tokens equal; |logprob - float64| <= 2e-5 (the worst observed is printed);
  * rows with fewer than k listable candidates, all-NaN and all-padding rows (token -1, score NaN);
  * the chain: candidates and sampled tokens of svln_op_gemv_argmax_topk, svln_op_gemv_batched_argmax_topk and svln_op_gemm_argmax_topk
    in their sampled form, fed to svln_op_truncate at (8, 1): the truncated token is the untruncated one whenever that is among the row's
    8 best, otherwise the restatement's -- exactly;
  * every malformed call is refused before any launch.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import scores_ref as S
import topk_ref as TK
import trunc_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
_engines = {}
WORST = dict(logprob=0.0, noise=0.0)
PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def engine(dtype=torch.float32):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def truncate(m, cv, ci, streams, draws, seed, k, p, T=1.0, rc_only=False, B=None, n_part=None, c=None):
    """svln_op_truncate -> dict of everything it returns (or the return code and the untouched outputs)"""
    cv, ci = np.ascontiguousarray(cv, dtype=np.float32), np.ascontiguousarray(ci, dtype=np.int32)
    Bs, n, cc = cv.shape
    B, n_part, c = Bs if B is None else B, n if n_part is None else n_part, cc if c is None else c
    o = {key: np.full(32 * R.C, np.nan, np.float32) for key in ("pv", "pr", "pm", "ps")}
    o["pi"] = np.full(32 * R.C, -7, np.int32)
    toks, lps = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32))
    rc = m._lib.svln_op_truncate(m._h, cv.ctypes.data_as(PF), ci.ctypes.data_as(PI), B, n_part, c, streams, draws, seed, T, k, p,
                                 o["pv"].ctypes.data_as(PF), o["pi"].ctypes.data_as(PI), o["pr"].ctypes.data_as(PF), o["pm"].ctypes.data_as(PF),
                                 o["ps"].ctypes.data_as(PF), toks, lps)
    o.update(tokens=list(toks), scores=list(lps))
    if rc_only:
        return rc, o
    _lib.check(rc)
    return o


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def _check(case, got):
    exp, ref = case.restate(), case.reference()
    B = case.B
    assert got["tokens"][B:] == [-7] * (32 - B) and bool((got["pi"][B * R.C:] == -7).all()), "rows beyond B written"
    for b in range(B):
        e, (kept, tok, lp, _) = exp[b], ref[b]
        sl = slice(b * R.C, (b + 1) * R.C)
        assert got["pi"][sl].tolist() == e["pi"].tolist(), (case.id, b, "part_idx", got["pi"][sl], e["pi"])
        for key in ("pr", "pm", "ps"):
            assert _bits(got[key][sl]) == _bits(e[key]), (case.id, b, key, got[key][sl], e[key])
        n = len(kept)
        assert bool(np.isneginf(got["pv"][sl][n:]).all()), (case.id, b, "part_val beyond the kept")
        for j in range(n):
            g = e["g"][j]
            err = abs(float(got["pv"][sl][j]) - (float(e["pr"][j]) + g))
            WORST["noise"] = max(WORST["noise"], err / (R.G_BOUND * max(1.0, abs(g))))
            assert err <= R.G_BOUND * max(1.0, abs(g)), (case.id, b, j, got["pv"][sl][j], e["pr"][j], g)
        assert got["tokens"][b] == e["token"] == tok, (case.id, b, got["tokens"][b], e["token"], tok)
        if tok < 0:
            assert math.isnan(got["scores"][b])
        else:
            err = abs(got["scores"][b] - lp)
            WORST["logprob"] = max(WORST["logprob"], err)
            assert err <= R.TOL, (case.id, b, got["scores"][b], lp)


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c.id)
def test_truncate_partials(case):
    m = engine()
    draws = [d + case.count for d in case.draws]                # (the op entry has no GenCtl.count: the draw carries it)
    _check(case, truncate(m, case.cv, case.ci, _i32(case.streams), _i32(draws), case.seed, case.k, case.p))


def test_a_short_row_after_a_full_one_reads_nothing_stale():
    """the eight entries of a row are rewritten by every launch: a row with one listable candidate after a call that kept eight"""
    m = engine()
    full = next(c for c in R.cases() if c.name == "grid" and c.k == 8 and c.p == 1.0 and c.c == 8 and c.n_part == 5)
    short = next(c for c in R.cases() if c.name == "short" and c.k == 8)
    truncate(m, full.cv, full.ci, _i32(full.streams), _i32(full.draws), full.seed, 8, 1.0)
    _check(short, truncate(m, short.cv, short.ci, _i32(short.streams), _i32([d + short.count for d in short.draws]), short.seed, short.k, short.p))


# ------------------------------------------------------------------------------------------------------------ the chain
def _chain_check(m, cv, ci, n_part, rows, toks, top_ids, seed, what):
    """candidates [B][n_part][8] and sampled tokens of a producer -> svln_op_truncate at (8, 1)"""
    B = len(rows)
    cv, ci = cv[:B * n_part * R.C].reshape(B, n_part, R.C), ci[:B * n_part * R.C].reshape(B, n_part, R.C)
    streams, draws = [r[0] for r in rows], [r[1] for r in rows]
    got = truncate(m, cv, ci, _i32(streams), _i32(draws), seed, 8, 1.0)
    same = 0
    for b in range(B):
        best = [i for _, i in R.select(cv[b], ci[b], 8)]
        assert best == [i for i in top_ids[b] if i >= 0], (what, b, best, top_ids[b])
        if toks[b] in best:
            assert got["tokens"][b] == toks[b], (what, b, got["tokens"][b], toks[b], best)
            same += 1
        else:
            e = R.restate_row(cv[b], ci[b], 8, 1.0, seed, streams[b], draws[b])
            assert got["tokens"][b] == e["token"], (what, b, got["tokens"][b], e["token"])
    return same


def test_chain_from_the_rows_gemv():
    import test_topk_gpu as TG
    same = 0
    for case in [c for c in TK.rows_cases() if c.sampled and c.N <= 391]:
        m = TG.engine(case.dtype)
        ops, dx, flags, smp = TG._device_case(case)
        torch.cuda.synchronize()
        got = TG.call(m, S.FMT_ID[case.fmt], ops["W"], ops.get("aux"), case.K, dx, case.N, case.K, flags, 8, smp)
        same += _chain_check(m, got["cv"], got["ci"], got["n_part"], [(case.stream, case.draw)], [got["token"]], [got["ids"].tolist()],
                             case.seed, case.id)
    assert same >= 1


@pytest.mark.parametrize("kind", ["batched", "mfma"])
def test_chain_from_the_batched_gemv_and_the_mfma_tiles(kind):
    import test_topk_gpu as TG
    same = rows = 0
    for case in [c for c in TK.all_batch_cases() if c.kind == kind and c.sampled and c.N <= 391]:
        m = TG.engine(case.dtype)
        got = TG._batch_call(m, case, True, 8)
        ids = [got["ids"][b * 8:(b + 1) * 8].tolist() for b in range(case.B)]
        same += _chain_check(m, got["cv"], got["ci"], got["n_part"], list(zip(case.streams, case.draws)), got["tokens"], ids, case.seed, case.id)
        rows += case.B
    assert rows >= 8 and same >= rows // 2, (kind, same, rows)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_malformed_calls_are_refused_before_any_launch():
    m = engine()
    cv, ci = np.zeros((2, 5, 8), np.float32), np.arange(80, dtype=np.int32).reshape(2, 5, 8)
    st, dr = _i32([0, 1]), _i32([0, 0])
    L = m._lib

    def refused(what, *a, **kw):
        rc, o = truncate(m, *a, rc_only=True, **kw)
        assert rc != 0, what
        assert bool((o["pi"] == -7).all()) and o["tokens"] == [-7] * 32 and all(math.isnan(x) for x in o["scores"]) and bool(np.isnan(o["pv"]).all()), \
            (what, "a refused call wrote its output")
        return L.svln_last_error()

    assert truncate(m, cv, ci, st, dr, 1, 8, 1.0, rc_only=True)[0] == 0
    assert b"top_k" in refused("top_k = 0", cv, ci, st, dr, 1, 0, 1.0)
    assert b"top_k" in refused("top_k = 9", cv, ci, st, dr, 1, 9, 1.0)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        assert b"top_p" in refused(f"top_p = {bad}", cv, ci, st, dr, 1, 4, bad)
    refused("B = 0", cv, ci, st, dr, 1, 4, 1.0, B=0)
    refused("B = 33", cv, ci, st, dr, 1, 4, 1.0, B=33)
    refused("n_part = 0", cv, ci, st, dr, 1, 4, 1.0, n_part=0)
    refused("c = 4", cv, ci, st, dr, 1, 4, 1.0, c=4)
    refused("n_part x c > 16384", cv, ci, st, dr, 1, 4, 1.0, n_part=2049)
    refused("n_part x c > 16384 (c = 1)", cv, ci, st, dr, 1, 4, 1.0, n_part=16385, c=1)
    assert b"temperature" in refused("T = 0", cv, ci, st, dr, 1, 4, 1.0, T=0.0)
    refused("negative stream", cv, ci, _i32([0, -1]), dr, 1, 4, 1.0)
    refused("negative draw", cv, ci, st, _i32([-1, 0]), 1, 4, 1.0)
    refused("no streams", cv, ci, None, dr, 1, 4, 1.0)
    neg = ci.copy()
    neg[1, 2, 3] = -1
    refused("negative column", cv, neg, st, dr, 1, 4, 1.0)
    toks, lps = (C.c_int32 * 32)(), (C.c_float * 32)()
    buf = np.zeros(16, np.float32)
    assert L.svln_op_truncate(m._h, None, ci.ctypes.data_as(PI), 2, 5, 8, st, dr, 1, 1.0, 4, 1.0, buf.ctypes.data_as(PF), ci.ctypes.data_as(PI),
                              buf.ctypes.data_as(PF), buf.ctypes.data_as(PF), buf.ctypes.data_as(PF), toks, lps) != 0
    assert b"null" in L.svln_last_error()


def test_zz_report_worst():
    print(f"worst |logprob - float64| = {WORST['logprob']:.3e} (bound {R.TOL:.0e}); worst noise error / bound = {WORST['noise']:.3f}")
