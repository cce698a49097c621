"""Token entropies at op level (svln_token_entropy): the EPI_ARGMAX_LSE_ENT / EPI_SAMPLE_ENT siblings of gemv_rows_kernel (engine dtype,
e4m3, MXFP4, the 12-bit packing), of gemv_batched_kernel and of the 32 x 128 MFMA arg-max epilogue, and entropy_merge_kernel, through
the test-only entries svln_op_gemv_argmax_entropy / svln_op_gemv_batched_argmax_entropy / svln_op_gemm_argmax_entropy /
svln_op_entropy_merge, on the exact cases of tests/entropy_ref.py (tests/test_entropy_inputs.py proves them sharp on the CPU; no case is
skipped here).  Every case runs greedy and sampled.

  * |H - float64| <= entropy_ref.TOL, the bound derived there from the operation order; the worst observed is printed per form;
  * tokens and log-probabilities are the bits svln_op_*_argmax_scores / _sample return on the same arguments; part_val / part_idx /
    part_sum are the bits those entries leave (svln_op_read_argmax_partials for the batched forms; for the single-env GEMV, whose scored
    entries return no partials, the five arrays of svln_op_gemv_argmax_topk, which the top-k tests pin to the scored form bit for bit);
    part_raw / part_max of the batched forms, which no existing entry returns, are checked against the exact values (designed logits:
    the maximum of a partial and the y of its winner are exact);
  * the 12-bit packing gives the bf16 form's outputs bit for bit;
  * the three forms agree on the same operands within the tolerance;
  * the merge on hand-made partials: null part_ent equals explicit zeros bit for bit, empty partials between live ones change nothing, a
    -inf-only row and a NaN partial give NaN, n equal single-id partials give log n (n = 1, 255, 256, 257, 2048: the largest grid an
    lm_head launches), one partial gives exactly 0;
  * every malformed call is refused before any launch.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import entropy_ref as E
import p12_ref
import scores_ref as S
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from util import ptr

pytestmark = pytest.mark.gpu
_engines = {}
WORST = {}
NMAX = 2048
PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int32)
F = np.float32


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def _outs(rows):
    return {"pv": np.full(rows * NMAX, np.nan, F), "pi": np.full(rows * NMAX, -7, np.int32), "ps": np.full(rows * NMAX, np.nan, F),
            "pr": np.full(rows * NMAX, np.nan, F), "pm": np.full(rows * NMAX, np.nan, F), "pe": np.full(rows * NMAX, np.nan, F),
            "ent": np.full(max(rows, 1), np.nan, F)}


def _tail(o, npart):
    return (o["ent"].ctypes.data_as(PF), o["pv"].ctypes.data_as(PF), o["pi"].ctypes.data_as(PI), o["ps"].ctypes.data_as(PF),
            o["pr"].ctypes.data_as(PF), o["pm"].ctypes.data_as(PF), o["pe"].ctypes.data_as(PF), C.byref(npart))


def rows_call(m, fmt_id, W, aux, ldw, x, N, K, flags, smp, rc_only=False):
    """svln_op_gemv_argmax_entropy -> dict of everything it returns (or the return code); smp = (sampled, T, seed, stream, draw)"""
    o = _outs(1)
    tok, lp, npart = C.c_int32(-7), C.c_float(float("nan")), C.c_int32(-7)
    sampled, T, seed, stream, draw = smp
    rc = m._lib.svln_op_gemv_argmax_entropy(m._h, fmt_id, ptr(W), ptr(aux), ldw, ptr(x), N, K, ptr(flags), E.PEN, int(sampled), T, seed, stream, draw,
                                            C.byref(tok), C.byref(lp), *_tail(o, npart))
    if rc_only:
        return rc, o
    _lib.check(rc)
    o.update(token=tok.value, score=lp.value, n=npart.value)
    return o


def _smp(case, sampled, b=0):
    return (sampled, case.T if sampled else 1.0, case.smp_seed, case.streams[b], case.draws[b])


def _rows_existing(m, case, ops, dx, fr, sampled):
    """token and score of the scored / sampled entry, and the five partial arrays of the top-k entry, on the same arguments"""
    L, h = m._lib, m._h
    tok, lp = C.c_int32(-7), C.c_float(float("nan"))
    head = (h, S.FMT_ID[case.fmt], ptr(ops["W"]), ptr(ops.get("aux")), case.K, ptr(dx), case.N, case.K, ptr(fr), E.PEN)
    if sampled:
        _lib.check(L.svln_op_gemv_argmax_sample(*head, case.T, case.smp_seed, case.streams[0], case.draws[0], C.byref(tok), C.byref(lp)))
    else:
        _lib.check(L.svln_op_gemv_argmax_scores(*head, C.byref(tok), C.byref(lp)))
    o = _outs(1)
    cv, ci = np.zeros(NMAX * 8, F), np.zeros(NMAX * 8, np.int32)
    ti, tl = np.zeros(8, np.int32), np.zeros(8, F)
    t2, l2, npart = C.c_int32(-7), C.c_float(float("nan")), C.c_int32(-7)
    _lib.check(L.svln_op_gemv_argmax_topk(*head, 1, int(sampled), case.T if sampled else 1.0, case.smp_seed, case.streams[0], case.draws[0],
                                          C.byref(t2), C.byref(l2), o["pv"].ctypes.data_as(PF), o["pi"].ctypes.data_as(PI), o["ps"].ctypes.data_as(PF),
                                          o["pr"].ctypes.data_as(PF), o["pm"].ctypes.data_as(PF), cv.ctypes.data_as(PF), ci.ctypes.data_as(PI),
                                          ti.ctypes.data_as(PI), tl.ctypes.data_as(PF), C.byref(npart)))
    o.update(token=tok.value, score=lp.value, n=npart.value)
    return o


def _note(key, worst):
    WORST[key] = max(WORST.get(key, 0.0), worst)


def _check_entropy(case, sampled, ent, form):
    ref = case.reference_entropy(sampled)
    worst = 0.0
    for b in range(case.B):
        if math.isnan(ref[b]):
            assert math.isnan(float(ent[b])), (case.id, b)
            continue
        err = abs(float(ent[b]) - ref[b])
        worst = max(worst, err)
        if case.N == 1:
            assert float(ent[b]) == 0.0, (case.id, sampled, b, float(ent[b]))
    _note(form, worst)
    print(f"{case.id}{' sampled' if sampled else ''}: worst |H - float64| = {worst:.3e} (bound {E.TOL:.3e})")
    assert worst <= E.TOL, (case.id, sampled, worst)


@pytest.mark.parametrize("case", E.rows_cases(), ids=lambda c: c.id)
def test_gemv_rows_entropy(case):
    dt = case.dtype
    m = engine(dt)
    x, W = case.operands()
    ops = {k: v.cuda() for k, v in S.pack(case.fmt, W).items()}
    dx = x[0].to(dt).cuda()
    _, flags, rows = case.logits()
    fr = None if flags is None else flags[rows[0]].contiguous().cuda()
    torch.cuda.synchronize()
    for sampled in (False, True):
        got = rows_call(m, S.FMT_ID[case.fmt], ops["W"], ops.get("aux"), case.K, dx, case.N, case.K, fr, _smp(case, sampled))
        n = S.G.gemv_grid(case.N)
        assert got["n"] == n
        _check_entropy(case, sampled, got["ent"], "rows-" + case.fmt)
        old = _rows_existing(m, case, ops, dx, fr, sampled)
        assert old["n"] == n and got["token"] == old["token"] and _bits([got["score"]]) == _bits([old["score"]]), (case.id, sampled, got["token"], old["token"])
        for key in ("pv", "pi", "ps") + (("pr", "pm") if sampled else ()):
            assert got[key][:n].view(np.uint32).tolist() == old[key][:n].view(np.uint32).tolist(), (case.id, sampled, "partials differ from the sibling", key)
        for key in ("pv", "ps", "pe"):
            assert bool(np.isnan(got[key][n:]).all()), (case.id, "written beyond the partials", key)
        if case.fmt == "plain-bf16" and case.N <= 20497:
            # the 12-bit packing: the bf16 form's outputs bit for bit
            dw = W.cuda().contiguous()
            aux = torch.zeros(case.N * p12_ref.row_bytes(case.K) + case.N * 16, dtype=torch.uint8, device="cuda")
            n_fb = C.c_int64(0)
            _lib.check(m._lib.svln_op_pack_rows(m._h, ptr(dw), case.K, case.N, case.K, ptr(aux), ptr(aux[case.N * p12_ref.row_bytes(case.K):]), C.byref(n_fb)))
            torch.cuda.synchronize()
            p = rows_call(m, 3, dw, aux, case.K, dx, case.N, case.K, fr, _smp(case, sampled))
            for key in ("pv", "pi", "ps", "pe", "ent") + (("pr", "pm") if sampled else ()):
                assert p[key].view(np.uint32).tolist() == got[key].view(np.uint32).tolist(), (case.id, sampled, "packed", key)
            assert p["token"] == got["token"] and _bits([p["score"]]) == _bits([got["score"]])


# ------------------------------------------------------------------------------------------------------------ batched GEMV, MFMA tiles
def multi_call(m, case, sampled, entry, kind=None, rc_only=False):
    """entry "entropy": the new entry of `kind` (default: the case's); "existing": the scored / sampled entry -> dict"""
    kind = kind or case.kind
    dt = case.dtype
    x, W = case.operands()
    dx, dW = x.to(dt).cuda().contiguous(), W.to(dt).cuda().contiguous()
    _, flags, rows = case.logits()
    dfl = None if flags is None else flags.cuda()
    drows = None if rows is None else torch.tensor(rows, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    B, N, K = case.B, case.N, case.K
    toks, lps = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32))
    o = _outs(B)
    npart = C.c_int32(-7)
    L, h = m._lib, m._h
    T, seed = (case.T if sampled else 1.0), case.smp_seed
    st, dr = _i32(case.streams), _i32(case.draws)
    n = min((N + 3) // 4, 2048) if kind == "batched" else (N + 127) // 128
    if entry == "entropy":
        if kind == "batched":
            rc = L.svln_op_gemv_batched_argmax_entropy(h, ptr(dW), K, ptr(dx), K, N, K, B, ptr(dfl), ptr(drows), E.PEN, int(sampled), T, seed, st, dr,
                                                       toks, lps, *_tail(o, npart))
        else:
            rc = L.svln_op_gemm_argmax_entropy(h, ptr(dx), K, ptr(dW), K, B, N, K, ptr(dfl), ptr(drows), E.PEN, int(sampled), T, seed, st, dr, toks, lps,
                                               *_tail(o, npart))
        if rc_only:
            return rc, o
        _lib.check(rc)
        assert npart.value == n
    else:
        if kind == "batched" and sampled:
            _lib.check(L.svln_op_gemv_batched_argmax_sample(h, ptr(dW), K, ptr(dx), K, None, S.G.EPS, N, K, B, ptr(dfl), ptr(drows), E.PEN, T, seed, st, dr, toks, lps))
        elif kind == "batched":
            _lib.check(L.svln_op_gemv_batched_argmax_scores(h, ptr(dW), K, ptr(dx), K, None, S.G.EPS, N, K, B, ptr(dfl), ptr(drows), E.PEN, toks, lps))
        elif sampled:
            _lib.check(L.svln_op_gemm_argmax_sample(h, ptr(dx), K, ptr(dW), K, B, N, K, ptr(dfl), ptr(drows), E.PEN, T, seed, st, dr, toks, lps))
        else:
            _lib.check(L.svln_op_gemm_argmax_scores(h, ptr(dx), K, ptr(dW), K, B, N, K, ptr(dfl), ptr(drows), E.PEN, toks, lps))
        pv, pi, ps = np.full(B * n, np.nan, F), np.full(B * n, -7, np.int32), np.full(B * n, np.nan, F)
        _lib.check(L.svln_op_read_argmax_partials(h, B, n, pv.ctypes.data_as(PF), pi.ctypes.data_as(PI), ps.ctypes.data_as(PF)))
        o.update(pv=pv, pi=pi, ps=ps)
    o.update(tokens=list(toks)[:B], scores=np.array(list(lps)[:B], dtype=F), n=n)
    return o


def _check_multi(case, sampled, kind=None):
    m = engine(case.dtype)
    got = multi_call(m, case, sampled, "entropy", kind)
    B, n = case.B, got["n"]
    _check_entropy(case, sampled, got["ent"], (kind or case.kind) + "-" + case.fmt)
    old = multi_call(m, case, sampled, "existing", kind)
    assert got["tokens"] == old["tokens"] and _bits(got["scores"]) == _bits(old["scores"]), (case.id, sampled, got["tokens"], old["tokens"])
    for key in ("pv", "pi", "ps"):
        assert got[key][:B * n].view(np.uint32).tolist() == old[key].view(np.uint32).tolist(), (case.id, sampled, "partials differ from the sibling", key)
    for key in ("pv", "ps", "pe"):
        assert bool(np.isnan(got[key][B * n:]).all()), (case.id, "written beyond the partials", key)
    if sampled:
        # part_max / part_raw against the exact values: the maximum y of the columns a partial owns and the y of its winner
        y = case.y(True).astype(F)
        _, part, _, _, n_parts, _ = E.SM.layout(kind or case.kind, case.N)
        assert n_parts == n
        for b in range(B):
            pm, pr, pi = got["pm"][b * n:(b + 1) * n], got["pr"][b * n:(b + 1) * n], got["pi"][b * n:(b + 1) * n]
            exp_m = np.full(n, -np.inf, F)
            np.maximum.at(exp_m, part[:case.N], y[b])
            assert _bits(pm) == _bits(exp_m), (case.id, b, "part_max")
            own = pi != 0x7FFFFFFF
            assert bool(own.all()) and _bits(pr) == _bits(y[b][pi]), (case.id, b, "part_raw")
    return got


@pytest.mark.parametrize("case", E.batched_cases(), ids=lambda c: c.id)
def test_gemv_batched_entropy(case):
    for sampled in (False, True):
        _check_multi(case, sampled)


@pytest.mark.parametrize("case", E.mfma_cases(), ids=lambda c: c.id)
def test_gemm_argmax_entropy(case):
    for sampled in (False, True):
        _check_multi(case, sampled)


@pytest.mark.parametrize("B", [1, 4])
def test_three_forms_agree(B):
    """the same operands and flags through the batched GEMV, the MFMA tiles and, row by row, the wave-per-rows GEMV: exact logits, so
    the entropies differ by the summation order alone"""
    case = E.Case(S.Case("batched", 391, 576, B=B, fmt="plain-fp32", pen=True, seed=500))
    m = engine(torch.float32)
    x, W = case.operands()
    _, flags, rows = case.logits()
    for sampled in (False, True):
        gb = _check_multi(case, sampled)
        gm = _check_multi(case, sampled, "mfma")
        assert float(np.abs(gb["ent"][:B] - gm["ent"][:B]).max()) <= E.TOL
        for b in range(B):
            g = rows_call(m, 0, W.cuda(), None, 576, x[b].float().cuda(), 391, 576, flags[rows[b]].contiguous().cuda(), _smp(case, sampled, b))
            assert abs(float(g["ent"][0]) - float(gb["ent"][b])) <= E.TOL, (sampled, b)
            assert abs(float(g["ent"][0]) - case.reference_entropy(sampled)[b]) <= E.TOL, (sampled, b)


# ------------------------------------------------------------------------------------------------------------ the merge
def merge_call(m, pv, pi, ps, pm=None, pe=None, B=None, n=None, rc_only=False):
    pv, pi, ps = np.ascontiguousarray(pv, F), np.ascontiguousarray(pi, np.int32), np.ascontiguousarray(ps, F)
    B = pv.shape[0] if B is None else B
    n = pv.shape[1] if n is None else n
    out = np.full(max(B, 1), np.nan, F)
    pm = None if pm is None else np.ascontiguousarray(pm, F)
    pe = None if pe is None else np.ascontiguousarray(pe, F)
    rc = m._lib.svln_op_entropy_merge(m._h, pv.ctypes.data_as(PF), pi.ctypes.data_as(PI), ps.ctypes.data_as(PF),
                                      None if pm is None else pm.ctypes.data_as(PF), None if pe is None else pe.ctypes.data_as(PF), B, n,
                                      out.ctypes.data_as(PF))
    if rc_only:
        return rc, out
    _lib.check(rc)
    return out


def test_merge_on_hand_made_partials():
    m = engine(torch.float32)
    ninf, nan, none = -np.inf, np.nan, 0x7FFFFFFF
    # n equal single-id partials: log n; one partial: exactly 0
    for n in (1, 255, 256, 257, 2048):
        pv, pi, ps = np.full((2, n), 1.25, F), np.arange(2 * n, dtype=np.int32).reshape(2, n), np.ones((2, n), F)
        a = merge_call(m, pv, pi, ps)
        b = merge_call(m, pv, pi, ps, pe=np.zeros((2, n), F))
        assert _bits(a) == _bits(b), (n, "null part_ent differs from explicit zeros")
        s = merge_call(m, pv + 3, pi, ps, pm=pv)            # sampled form: part_val holds z, the sums are relative to part_max
        assert _bits(s) == _bits(a), n
        assert float(np.abs(a - math.log(n)).max()) <= E.TOL, (n, a)
        if n == 1:
            assert a.tolist() == [0.0, 0.0]
    # live partials with t, empty partials between them: nothing changes; against the restatement and float64
    live = [(3.0, 1.5, -0.25), (2.0, 1.0, 0.0), (3.0, 2.25, -0.5), (-1.0, 1.0, 0.0)]
    empty = (ninf, 0.0, 0.0)
    rows = [live, [empty, live[0], empty, empty, live[1], live[2], empty, live[3]]]
    outs = []
    for r in rows:
        pv = np.array([[p[0] for p in r]], F)
        ps = np.array([[p[1] for p in r]], F)
        pe = np.array([[p[2] for p in r]], F)
        pi = np.array([[none if p[1] == 0 else 7 * k for k, p in enumerate(r)]], np.int32)
        outs.append(merge_call(m, pv, pi, ps, pe=pe))
        assert _bits(merge_call(m, pv + 1, pi, ps, pm=pv, pe=pe)) == _bits(outs[-1])
    assert _bits(outs[0]) == _bits(outs[1])
    exp, _ = E.merge([(F(a), F(b), F(c)) for a, b, c in live])
    assert abs(float(outs[0][0]) - exp) <= E.TOL
    # a -inf-only row gives NaN, a NaN partial gives NaN, the row beside them is untouched
    pv = np.array([[ninf, ninf, ninf], [1.0, nan, 0.5], [1.0, 0.5, 0.0]], F)
    pi = np.array([[none, none, none], [0, none, 2], [0, 1, 2]], np.int32)
    ps = np.array([[0, 0, 0], [1, nan, 1], [1, 1, 1]], F)
    pe = np.array([[0, 0, 0], [0, nan, 0], [0, 0, 0]], F)
    for pm in (None, pv):
        got = merge_call(m, pv, pi, ps, pm=pm, pe=pe)
        assert math.isnan(float(got[0])) and math.isnan(float(got[1])), got
        assert abs(float(got[2]) - E.reference(np.array([[1.0, 0.5, 0.0]]))[0]) <= E.TOL


def test_malformed_calls_are_refused_before_any_launch():
    m = engine(torch.float32)
    L = m._lib
    N, K = 16, 64
    W = torch.zeros((N, K), dtype=torch.float32, device="cuda")
    x = torch.zeros((4, K), dtype=torch.float32, device="cuda")
    greedy = (False, 1.0, 0, 0, 0)

    def refused(what, *a, smp=greedy):
        rc, o = rows_call(m, *a, smp, rc_only=True)
        assert rc != 0, what
        assert bool(np.isnan(o["ent"]).all()) and bool(np.isnan(o["pe"]).all()) and bool((o["pi"] == -7).all()), (what, "a refused call wrote its output")
        return L.svln_last_error()

    assert b"null" in refused("no weights", 0, None, None, K, x, N, K, None)
    assert b"null" in refused("no activations", 0, W, None, K, None, N, K, None)
    refused("K not a chunk multiple", 0, W, None, K, x, N, K - 2, None)
    refused("ldw below K", 0, W, None, K - 4, x, N, K, None)
    refused("N = 0", 0, W, None, K, x, 0, K, None)
    assert b"fmt" in refused("fmt 4", 4, W, None, K, x, N, K, None)
    assert b"bf16" in refused("e4m3 on fp32", 1, W, x, K, x, N, K, None)
    assert b"bf16" in refused("packed on fp32", 3, W, W, K, x, N, K, None)
    assert b"temperature" in refused("T = 0", 0, W, None, K, x, N, K, None, smp=(True, 0.0, 0, 0, 0))
    refused("negative draw", 0, W, None, K, x, N, K, None, smp=(True, 1.0, 0, 0, -1))
    # null outputs of the three product entries
    tok, lp, npart = C.c_int32(-7), C.c_float(float("nan")), C.c_int32(-7)
    o = _outs(4)
    t = list(_tail(o, npart))
    t[6] = None                                               # part_ent
    assert L.svln_op_gemv_argmax_entropy(m._h, 0, ptr(W), None, K, ptr(x), N, K, None, 2.0, 0, 1.0, 0, 0, 0, C.byref(tok), C.byref(lp), *t) != 0
    assert b"null" in L.svln_last_error()
    toks, lps = (C.c_int32 * 32)(*([-7] * 32)), (C.c_float * 32)(*([float("nan")] * 32))
    st = _i32([0] * 32)
    assert L.svln_op_gemv_batched_argmax_entropy(m._h, ptr(W), K, ptr(x), K, N, K, 4, None, None, 2.0, 0, 1.0, 0, st, st, toks, lps, *t) != 0
    assert L.svln_op_gemm_argmax_entropy(m._h, ptr(x), K, ptr(W), K, 4, N, K, None, None, 2.0, 0, 1.0, 0, st, st, toks, lps, *t) != 0
    full = _tail(o, npart)
    assert L.svln_op_gemv_batched_argmax_entropy(m._h, ptr(W), K, ptr(x), K, N, K, 3, None, None, 2.0, 0, 1.0, 0, st, st, toks, lps, *full) != 0
    assert b"B must be" in L.svln_last_error()
    assert L.svln_op_gemm_argmax_entropy(m._h, ptr(x), K, ptr(W), K, 33, N, K, None, None, 2.0, 0, 1.0, 0, st, st, toks, lps, *full) != 0
    assert L.svln_op_gemm_argmax_entropy(m._h, ptr(x), K, ptr(W), K, 4, N, K, ptr(W), None, 2.0, 0, 1.0, 0, st, st, toks, lps, *full) != 0      # flags without rows
    assert list(toks) == [-7] * 32 and bool(np.isnan(o["ent"]).all()) and bool(np.isnan(o["pe"]).all())
    # the merge: the bounds come first
    one = np.ones((1, 4), F)
    idx = np.zeros((1, 4), np.int32)
    for B, n in ((0, 4), (33, 4), (1, 0), (1, 2049)):
        rc, out = merge_call(m, one, idx, one, B=B, n=n, rc_only=True)
        assert rc != 0 and bool(np.isnan(out).all()), (B, n)
        assert (b"rows" in L.svln_last_error()) if B in (0, 33) else (b"n_part" in L.svln_last_error())
    out = np.full(1, np.nan, F)
    assert L.svln_op_entropy_merge(m._h, None, idx.ctypes.data_as(PI), one.ctypes.data_as(PF), None, None, 0, 4, out.ctypes.data_as(PF)) != 0
    assert b"rows" in L.svln_last_error()                      # (B is checked before the pointers)
    assert L.svln_op_entropy_merge(m._h, None, idx.ctypes.data_as(PI), one.ctypes.data_as(PF), None, None, 1, 4, out.ctypes.data_as(PF)) != 0
    assert b"null" in L.svln_last_error() and math.isnan(float(out[0]))


def test_report_worst():
    print("worst |H - float64| per form (bound %.3e): " % E.TOL + ", ".join(f"{k} {v:.3e}" for k, v in sorted(WORST.items())))
