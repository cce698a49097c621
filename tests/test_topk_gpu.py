"""Top-k log-probabilities at op level (svln_top_logprobs): the EPI_ARGMAX_LSE_TOPK / EPI_SAMPLE_TOPK siblings of gemv_rows_kernel (engine
dtype, e4m3, MXFP4, the 12-bit packing), the final kernel and topk_merge_kernel through the test-only entry svln_op_gemv_argmax_topk, on
the exact cases of tests/topk_ref.py (tests/test_topk_inputs.py proves them sharp on the CPU; no case is skipped here).

  * the candidate arrays, part_val / part_idx and the merged ids are bit-equal to the restatement;
  * the batched GEMV (B = 1, 2, 4, 8) and the 32 x 128 MFMA tiles through svln_op_gemv_batched_argmax_topk / svln_op_gemm_argmax_topk on
    the multi-row cases: the same assertions per row, and tokens, scores, part_val / part_idx / part_sum bit-equal to the existing
    svln_op_*_argmax_scores / _sample entries on the same arguments (svln_op_read_argmax_partials);
  * the three forms give the same list for the same operands;
  * token and score are the bits svln_op_gemv_argmax_scores / svln_op_gemv_argmax_sample return on the same arguments;
  * |logprob - float64| <= 2e-5 (topk_ref.TOL, the project's op-level bound); the worst observed is printed;
  * entry 0 (greedy) and the sampled id's entry (when listed) are the score's bits;
  * the 12-bit packing gives the bf16 form's outputs bit for bit; one case runs at the true K = 3584;
  * every malformed call is refused before any launch.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import p12_ref
import scores_ref as S
import topk_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
_engines = {}
WORST = {}
MAXP = 1280
PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def call(m, fmt_id, W, aux, ldw, x, N, K, flags, k, case_like, rc_only=False, outs=None):
    """svln_op_gemv_argmax_topk -> dict of everything it returns (or the return code)"""
    o = outs or {
        "pv": np.full(MAXP, np.nan, np.float32), "pi": np.full(MAXP, -7, np.int32), "ps": np.full(MAXP, np.nan, np.float32),
        "pr": np.full(MAXP, np.nan, np.float32), "pm": np.full(MAXP, np.nan, np.float32),
        "cv": np.full(MAXP * R.C, np.nan, np.float32), "ci": np.full(MAXP * R.C, -7, np.int32),
        "ids": np.full(R.C, -7, np.int32), "lps": np.full(R.C, np.nan, np.float32)}
    tok, lp, npart = C.c_int32(-7), C.c_float(float("nan")), C.c_int32(-7)
    sampled, T, seed, stream, draw = case_like
    rc = m._lib.svln_op_gemv_argmax_topk(
        m._h, fmt_id, ptr(W), ptr(aux), ldw, ptr(x), N, K, ptr(flags), R.PEN, k, int(sampled), T, seed, stream, draw, C.byref(tok), C.byref(lp),
        o["pv"].ctypes.data_as(PF), o["pi"].ctypes.data_as(PI), o["ps"].ctypes.data_as(PF), o["pr"].ctypes.data_as(PF), o["pm"].ctypes.data_as(PF),
        o["cv"].ctypes.data_as(PF), o["ci"].ctypes.data_as(PI), o["ids"].ctypes.data_as(PI), o["lps"].ctypes.data_as(PF), C.byref(npart))
    if rc_only:
        return rc, o
    _lib.check(rc)
    o.update(token=tok.value, score=lp.value, n_part=npart.value)
    return o


def _device_case(case):
    dt = case.dtype
    x, W = case.operands()
    ops = {k: v.cuda() for k, v in S.pack(case.fmt, W).items()}
    _, _, fr = case.logits()
    flags = None if fr is None else torch.from_numpy(fr).cuda()
    return ops, x[0].to(dt).cuda(), flags, (case.sampled, case.T or 1.0, case.seed, case.stream, case.draw)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def _check(case, got, k):
    exp = case.restate(k=k)
    ids, lps, _ = case.reference(k)
    n = exp["n_parts"]
    assert got["n_part"] == n
    ev = np.array([[v for v, _ in part] for part in exp["cand"]], dtype=np.float32)
    ei = np.array([[i for _, i in part] for part in exp["cand"]], dtype=np.int32)
    assert got["ci"][:n * R.C].tolist() == ei.reshape(-1).tolist(), (case.id, "candidate columns")
    assert _bits(got["cv"][:n * R.C]) == _bits(ev.reshape(-1)), (case.id, "candidate values")
    assert bool((got["ci"][n * R.C:] == -7).all()), "candidates written beyond the partials"
    assert got["ids"][:k].tolist() == ids and got["ids"][k:].tolist() == [-7] * (R.C - k), (case.id, got["ids"], ids)
    assert bool(np.isnan(got["lps"][k:]).all()), "more than k entries written"
    assert got["token"] == exp["token"], (case.id, got["token"], exp["token"])
    if "pv" in got:                                       # the rows form returns its partials: the arg-max partials are exact
        pv = got["pm"] if case.sampled else got["pv"]     # (sampled: part_val holds z, whose noise is rounded; part_max is the exact max y)
        assert _bits(pv[:n]) == _bits(exp["part_max" if case.sampled else "part_val"]), (case.id, "partial maxima")
        if not case.sampled:
            assert got["pi"][:n].tolist() == exp["part_idx"], (case.id, "part_idx")
    errs = []
    for a, b in zip(got["lps"][:k].tolist(), lps):
        if math.isnan(b) or math.isinf(b):
            assert (math.isnan(a) and math.isnan(b)) or a == b, (case.id, a, b)
        else:
            errs.append(abs(a - b))
    worst = max(errs + [0.0])
    WORST[case.fmt] = max(WORST.get(case.fmt, 0.0), worst)
    print(f"{case.id}: worst |logprob - float64| = {worst:.3e} (bound {R.TOL:.0e})")
    assert worst <= R.TOL, (case.id, worst)
    if not math.isnan(got["score"]):
        if not case.sampled:
            assert got["ids"][0] == got["token"] and _bits(got["lps"][:1]) == _bits([got["score"]]), (case.id, got["lps"][0], got["score"])
        elif got["token"] in ids:
            j = ids.index(got["token"])
            assert _bits(got["lps"][j:j + 1]) == _bits([got["score"]]), (case.id, j, got["lps"][j], got["score"])


def _existing(m, case, ops, dx, flags):
    """token and score of the non-top-k sibling on the same arguments"""
    tok, lp = C.c_int32(-7), C.c_float(float("nan"))
    if case.sampled:
        _lib.check(m._lib.svln_op_gemv_argmax_sample(m._h, S.FMT_ID[case.fmt], ptr(ops["W"]), ptr(ops.get("aux")), case.K, ptr(dx), case.N, case.K,
                                                     ptr(flags), R.PEN, case.T, case.seed, case.stream, case.draw, C.byref(tok), C.byref(lp)))
    else:
        _lib.check(m._lib.svln_op_gemv_argmax_scores(m._h, S.FMT_ID[case.fmt], ptr(ops["W"]), ptr(ops.get("aux")), case.K, ptr(dx), case.N, case.K,
                                                     ptr(flags), R.PEN, C.byref(tok), C.byref(lp)))
    return tok.value, lp.value


def _pack12(m, W):
    """device (bf16 original, packed rows followed by the row records) of W [N][K] bf16"""
    N, K = W.shape
    dw = W.cuda().contiguous()
    aux = torch.zeros(N * p12_ref.row_bytes(K) + N * 16, dtype=torch.uint8, device="cuda")
    n_fb = C.c_int64(0)
    _lib.check(m._lib.svln_op_pack_rows(m._h, ptr(dw), K, N, K, ptr(aux), ptr(aux[N * p12_ref.row_bytes(K):]), C.byref(n_fb)))
    return dw, aux


@pytest.mark.parametrize("case", R.rows_cases(), ids=lambda c: c.id)
def test_gemv_rows_topk(case):
    m = engine(case.dtype)
    ops, dx, flags, smp = _device_case(case)
    torch.cuda.synchronize()
    ks = R.KS if case.name in ("ties", "ragged") else (case.k,)
    first = None
    for k in ks:
        got = call(m, S.FMT_ID[case.fmt], ops["W"], ops.get("aux"), case.K, dx, case.N, case.K, flags, k, smp)
        _check(case, got, k)
        first = first or got
    tok, lp = _existing(m, case, ops, dx, flags)
    assert tok == first["token"] and _bits([lp]) == _bits([first["score"]]), (case.id, tok, lp, first["token"], first["score"])
    if case.fmt == "plain-bf16" and not case.special:
        # the 12-bit packing: the bf16 form's outputs bit for bit (it is the default lm_head stream of a bf16 engine)
        dw, aux = _pack12(m, case.operands()[1])
        torch.cuda.synchronize()
        p = call(m, 3, dw, aux, case.K, dx, case.N, case.K, flags, ks[0], smp)
        g0 = call(m, 0, ops["W"], None, case.K, dx, case.N, case.K, flags, ks[0], smp)
        for key in ("pv", "pi", "ps", "cv", "ci", "ids", "lps") + (("pr", "pm") if case.sampled else ()):
            assert p[key].view(np.uint32).tolist() == g0[key].view(np.uint32).tolist(), (case.id, "packed", key)
        assert p["token"] == g0["token"] and _bits([p["score"]]) == _bits([g0["score"]])


@pytest.mark.parametrize("fmt", ["plain-fp32", "plain-bf16"])
def test_true_k_chunk_loop(fmt):
    """K = 3584: every lane walks several chunks per row (the paired loop and its tail)"""
    case = R.Case("true-K", 1301, R._desc([1300, 7, 640, 641, 3, 1299, 100, 99, 650]), K=3584, fmt=fmt, seed=90, k=8)
    m = engine(case.dtype)
    ops, dx, flags, smp = _device_case(case)
    torch.cuda.synchronize()
    _check(case, call(m, 0, ops["W"], None, case.K, dx, case.N, case.K, flags, 8, smp), 8)


def test_malformed_calls_are_refused_before_any_launch():
    m = engine(torch.float32)
    N, K = 16, 64
    W = torch.zeros((N, K), dtype=torch.float32, device="cuda")
    x = torch.zeros(K, dtype=torch.float32, device="cuda")
    greedy = (False, 1.0, 0, 0, 0)
    L = m._lib

    def refused(what, *a, smp=greedy, **kw):
        rc, o = call(m, *a, smp, rc_only=True, **kw)
        assert rc != 0, what
        assert bool((o["ci"] == -7).all()) and bool((o["ids"] == -7).all()) and bool(np.isnan(o["lps"]).all()), (what, "a refused call wrote its output")
        return L.svln_last_error()

    assert b"k must be" in refused("k = 0", 0, W, None, K, x, N, K, None, 0)
    assert b"k must be" in refused("k = 9", 0, W, None, K, x, N, K, None, 9)
    assert b"null" in refused("no weights", 0, None, None, K, x, N, K, None, 4)
    assert b"null" in refused("no activations", 0, W, None, K, None, N, K, None, 4)
    refused("K not a chunk multiple", 0, W, None, K, x, N, K - 2, None, 4)
    refused("ldw below K", 0, W, None, K - 4, x, N, K, None, 4)
    refused("N = 0", 0, W, None, K, x, 0, K, None, 4)
    assert b"fmt" in refused("fmt 4", 4, W, None, K, x, N, K, None, 4)
    assert b"bf16" in refused("e4m3 on fp32", 1, W, x, K, x, N, K, None, 4)
    assert b"bf16" in refused("packed on fp32", 3, W, W, K, x, N, K, None, 4)
    assert b"temperature" in refused("T = 0", 0, W, None, K, x, N, K, None, 4, smp=(True, 0.0, 0, 0, 0))
    refused("negative draw", 0, W, None, K, x, N, K, None, 4, smp=(True, 1.0, 0, 0, -1))


# ------------------------------------------------------------------------------------------------------------ batched GEMV, MFMA tiles
def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _batch_call(m, case, topk, k=None):
    """the top-k entry (topk) or the existing scored / sampled entry of the case's kind on the same device operands -> dict"""
    dt = case.dtype
    x, W = case.operands()
    dx, dW = x.to(dt).cuda().contiguous(), W.to(dt).cuda().contiguous()
    fl, rows = case.flags()
    dfl = None if fl is None else torch.from_numpy(fl).cuda()
    drows = None if rows is None else torch.tensor(rows, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    B, N, K = case.B, case.N, case.K
    n_max = 2048
    toks, lps = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32))
    o = {"cv": np.full(B * n_max * R.C, np.nan, np.float32), "ci": np.full(B * n_max * R.C, -7, np.int32),
         "ids": np.full(B * R.C, -7, np.int32), "lps": np.full(B * R.C, np.nan, np.float32)}
    npart = C.c_int32(-7)
    L, h = m._lib, m._h
    T, seed = case.T or 1.0, case.seed
    if topk:
        tail = (k, int(case.sampled), T, seed, _i32(case.streams), _i32(case.draws), toks, lps, o["cv"].ctypes.data_as(PF), o["ci"].ctypes.data_as(PI),
                o["ids"].ctypes.data_as(PI), o["lps"].ctypes.data_as(PF), C.byref(npart))
        if case.kind == "batched":
            _lib.check(L.svln_op_gemv_batched_argmax_topk(h, ptr(dW), K, ptr(dx), K, N, K, B, ptr(dfl), ptr(drows), R.PEN, *tail))
        else:
            _lib.check(L.svln_op_gemm_argmax_topk(h, ptr(dx), K, ptr(dW), K, B, N, K, ptr(dfl), ptr(drows), R.PEN, *tail))
    elif case.kind == "batched":
        if case.sampled:
            _lib.check(L.svln_op_gemv_batched_argmax_sample(h, ptr(dW), K, ptr(dx), K, None, S.G.EPS, N, K, B, ptr(dfl), ptr(drows), R.PEN, T, seed,
                                                            _i32(case.streams), _i32(case.draws), toks, lps))
        else:
            _lib.check(L.svln_op_gemv_batched_argmax_scores(h, ptr(dW), K, ptr(dx), K, None, S.G.EPS, N, K, B, ptr(dfl), ptr(drows), R.PEN, toks, lps))
    elif case.sampled:
        _lib.check(L.svln_op_gemm_argmax_sample(h, ptr(dx), K, ptr(dW), K, B, N, K, ptr(dfl), ptr(drows), R.PEN, T, seed, _i32(case.streams),
                                                _i32(case.draws), toks, lps))
    else:
        _lib.check(L.svln_op_gemm_argmax_scores(h, ptr(dx), K, ptr(dW), K, B, N, K, ptr(dfl), ptr(drows), R.PEN, toks, lps))
    n = case.restate()[0]["n_parts"]
    pv, pi, ps = np.full(B * n, np.nan, np.float32), np.full(B * n, -7, np.int32), np.full(B * n, np.nan, np.float32)
    _lib.check(L.svln_op_read_argmax_partials(h, B, n, pv.ctypes.data_as(PF), pi.ctypes.data_as(PI), ps.ctypes.data_as(PF)))
    o.update(tokens=list(toks)[:B], scores=np.array(list(lps)[:B], dtype=np.float32), pv=pv, pi=pi, ps=ps, n_part=npart.value, n=n)
    return o


def _check_batch(case, got, k):
    exp, ref = case.restate(k=k), case.reference(k)
    n, B = exp[0]["n_parts"], case.B
    assert got["n_part"] == n
    ev = np.array([[[v for v, _ in part] for part in e["cand"]] for e in exp], dtype=np.float32)
    ei = np.array([[[i for _, i in part] for part in e["cand"]] for e in exp], dtype=np.int32)
    assert got["ci"][:B * n * R.C].tolist() == ei.reshape(-1).tolist(), (case.id, "candidate columns")
    assert _bits(got["cv"][:B * n * R.C]) == _bits(ev.reshape(-1)), (case.id, "candidate values")
    assert bool((got["ci"][B * n * R.C:] == -7).all()) and bool((got["ids"][B * k:] == -7).all()) and bool(np.isnan(got["lps"][B * k:]).all())
    worst = 0.0
    for b in range(B):
        ids, lps, _ = ref[b]
        gi, gl = got["ids"][b * k:(b + 1) * k].tolist(), got["lps"][b * k:(b + 1) * k]
        assert gi == ids and got["tokens"][b] == exp[b]["token"], (case.id, b, gi, ids, got["tokens"][b], exp[b]["token"])
        for a, r in zip(gl.tolist(), lps):
            if math.isnan(r) or math.isinf(r):
                assert (math.isnan(a) and math.isnan(r)) or a == r, (case.id, b, a, r)
            else:
                worst = max(worst, abs(a - r))
        sc = got["scores"][b:b + 1]
        if not math.isnan(float(sc[0])):
            if not case.sampled:
                assert gi[0] == got["tokens"][b] and _bits(gl[:1]) == _bits(sc), (case.id, b, gl[0], sc)
            elif got["tokens"][b] in gi:
                j = gi.index(got["tokens"][b])
                assert _bits(gl[j:j + 1]) == _bits(sc), (case.id, b, j, gl[j], sc)
    WORST[case.kind] = max(WORST.get(case.kind, 0.0), worst)
    print(f"{case.id}: worst |logprob - float64| = {worst:.3e} (bound {R.TOL:.0e})")
    assert worst <= R.TOL, (case.id, worst)


@pytest.mark.parametrize("case", R.all_batch_cases(), ids=lambda c: c.id)
def test_batched_and_mfma_topk(case):
    m = engine(case.dtype)
    first = None
    for k in (R.KS if case.name == "greedy" and case.N in (115, 129) else (case.k,)):
        got = _batch_call(m, case, True, k)
        _check_batch(case, got, k)
        first = first or got
    sib = _batch_call(m, case, False)
    assert sib["tokens"] == first["tokens"] and _bits(sib["scores"]) == _bits(first["scores"]), (case.id, sib["tokens"], first["tokens"])
    for key in ("pv", "pi", "ps"):
        assert sib[key].view(np.uint32).tolist() == first[key].view(np.uint32).tolist(), (case.id, "partials differ from the sibling entry", key)


@pytest.mark.parametrize("B", [1, 4])
def test_three_forms_give_the_same_list(B):
    """the same operands through the batched GEMV and the MFMA tiles (and, row by row, the wave-per-rows GEMV): exact logits, so the ids
    agree and the log-probabilities differ by the summation order of log S alone"""
    rows = R._batch_rows("batched", 391, B, 576, "plain-fp32", 8, 500, pen=True)
    cb, cm = R.BatchCase("batched", rows, "forms"), R.BatchCase("mfma", R._batch_rows("mfma", 391, B, 576, "plain-fp32", 8, 500, pen=True), "forms")
    m = engine(torch.float32)
    gb, gm = _batch_call(m, cb, True, 8), _batch_call(m, cm, True, 8)
    assert gb["ids"][:B * 8].tolist() == gm["ids"][:B * 8].tolist()
    assert np.abs(gb["lps"][:B * 8] - gm["lps"][:B * 8]).max() <= R.TOL
    x, W = cb.operands()
    fl, prow = cb.flags()
    for b in range(B):
        fr = None if fl is None else torch.from_numpy(fl[prow[b]]).cuda()
        g = call(m, 0, W.cuda(), None, 576, x[b].float().cuda(), 391, 576, fr, 8, (False, 1.0, 0, 0, 0))
        assert g["ids"].tolist() == gb["ids"][b * 8:(b + 1) * 8].tolist(), b
        assert np.abs(g["lps"] - gb["lps"][b * 8:(b + 1) * 8]).max() <= R.TOL


def test_report_worst():
    print("worst |logprob - float64| per format: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(WORST.items())))
