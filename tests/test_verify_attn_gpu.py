"""The verify attention of a draft-verify pass (svln_op_attention_verify: attn_verify_kernel + the verify form of attn_combine_kernel) on
the sharp cases of tests/verify_ref.py, against the float64 reference: `rows` un-roped q|k|v rows verified at positions P .. P + rows - 1
behind P context rows, on scrambled page tables, the pools filled with the finite sentinel and the split-KV partials with NaN (a row with
no visible key in the split a straddling pass opens must still write its partial).  Output within Case.tolerance(q_flips=True), every
appended K row within roped_k_bound, V rows exact, every other pool slot untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ref as R
import verify_ref as VR
from streamvln_amd.config import CONFIGS
from test_attention_gpu import check_out, check_pool, check_untouched, chk, engine, kv_read, setup, _close_engines  # noqa: F401
from util import ptr

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def run_verify(m, cfg, dtype, case, P, rows):
    """the case through svln_op_attention_verify -> output [rows, q_heads, 128] (float64, host)"""
    ld = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD
    allrows = case.qkv_rows().to(dtype)
    dctx, dnew = allrows[:max(P, 1)].clone().cuda(), allrows[P:].clone().cuda()
    out = torch.full((rows, cfg.q_heads * R.HD), float("nan"), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    chk(m._lib.svln_op_attention_verify(m._h, rows, ptr(dctx), ld, P, ptr(dnew), ptr(out), cfg.q_heads * R.HD))
    return out.double().cpu().view(rows, cfg.q_heads, R.HD)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg,rows,P", VR.all_cases())
def test_attention_verify(dtype, cfg, rows, P):
    cfg = CONFIGS[cfg]
    m = engine(cfg, dtype)
    pages = setup(m, 1, 500 + 31 * P + rows)
    case = VR.verify_case(cfg, dtype, P, rows)
    got = run_verify(m, cfg, dtype, case, P, rows)
    L = P + rows
    K, V = kv_read(m, cfg, 0, L)
    what = f"verify {cfg.name} rows {rows} P {P}"
    check_pool(case, K, V, what)                     # the context rows and every row the pass appended
    check_out(got, case, None, K, what, q_flips=True, device="cuda")
    check_untouched(m, cfg, dtype, R.MAX_POSITIONS, [(pages[0], 0, L)], what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_verify_pass_then_decode_step_on_the_same_pages(dtype):
    """a verify pass at P = 61 (4 rows: 61 .. 64, over the page boundary), then ONE decode step (svln_op_attention_decode, B = 1) at
    position 65 on the same pages WITHOUT re-appending anything (null context rows: env 0 stays as the verify op left it).  The step
    must see the rows the pass appended: its needles sit on key 64 (written by the pass), the newest key and key 0, and one head ramps
    over all 66 keys, so a row the pass had not stored (the pools hold the sentinel) moves the output far past the tolerance.  The pool
    rows 0 .. 64 must be bit for bit what the pass left."""
    cfg = CONFIGS["tiny"]
    P, rows = 61, 4
    m = engine(cfg, dtype)
    pages = setup(m, 1, 4242)
    full = R.Case(cfg, dtype, P + rows + 1, [P + rows], R.DECODE_PATTERNS, seed=4242, tps=R.decode_split(cfg, R.MAX_POSITIONS),
                  nsplit=R.MAX_POSITIONS // R.PAGE)
    assert {"tile_first", "newest", "rising"} <= {full.pattern(h, 0) for h in range(cfg.q_heads)}
    ld = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD
    allrows = full.qkv_rows().to(dtype)
    out_v = torch.full((rows, cfg.q_heads * R.HD), float("nan"), dtype=dtype, device="cuda")
    dctx, dnew = allrows[:P].clone().cuda(), allrows[P:P + rows].clone().cuda()
    torch.cuda.synchronize()
    chk(m._lib.svln_op_attention_verify(m._h, rows, ptr(dctx), ld, P, ptr(dnew), ptr(out_v), cfg.q_heads * R.HD))
    Kv, Vv = kv_read(m, cfg, 0, P + rows)
    assert torch.isfinite(out_v.float()).all()
    kref, kb = R.roped_k_bound(full.k_in[:P + rows], torch.arange(P + rows), cfg.rope_theta, dtype)
    assert bool(((Kv - kref).abs() <= kb).all()) and torch.equal(Vv, full.v[:P + rows]), "rows appended by the verify pass"
    check_untouched(m, cfg, dtype, R.MAX_POSITIONS, [(pages[0], 0, P + rows)], "verify pass at 61")
    # the decode step at P + rows on env 0 as it stands: no context rows are handed over
    pos = np.asarray([P + rows], np.int32)
    dnew2 = allrows[P + rows:].clone().cuda()
    out_d = torch.full((1, cfg.q_heads * R.HD), float("nan"), dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    chk(m._lib.svln_op_attention_decode(m._h, 1, C.c_void_p(0), ld, 0, pos.ctypes.data_as(C.POINTER(C.c_int32)), ptr(dnew2), ptr(out_d),
                                        cfg.q_heads * R.HD))
    Kd, Vd = kv_read(m, cfg, 0, P + rows + 1)
    assert torch.equal(Kd[:P + rows], Kv) and torch.equal(Vd[:P + rows], Vv), "the step rewrote rows the verify pass had appended"
    what = "decode step after the verify pass"
    check_pool(full, Kd, Vd, what)
    check_out(out_d.double().cpu().view(1, cfg.q_heads, R.HD), full, None, Kd, what, q_flips=True, device="cuda")
    check_untouched(m, cfg, dtype, R.MAX_POSITIONS, [(pages[0], 0, P + rows + 1)], what)
    # a position in a page env 0 does not hold is refused, not written
    far = np.asarray([500], np.int32)
    assert m._lib.svln_op_attention_decode(m._h, 1, C.c_void_p(0), ld, 0, far.ctypes.data_as(C.POINTER(C.c_int32)), ptr(dnew2), ptr(out_d),
                                           cfg.q_heads * R.HD) != 0


def test_attention_verify_refusals():
    m = engine(CONFIGS["true_dims_1layer"], torch.bfloat16)
    cfg = CONFIGS["true_dims_1layer"]
    ld = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD
    buf = torch.zeros((8, ld), dtype=torch.bfloat16, device="cuda")
    out = torch.zeros((8, cfg.q_heads * R.HD), dtype=torch.bfloat16, device="cuda")
    for rows, ctx_rows in ((8, 0), (0, 0), (4, R.MAX_POSITIONS - 3)):          # rows * G > 32; no rows; past max_positions
        rc = m._lib.svln_op_attention_verify(m._h, rows, ptr(buf), ld, ctx_rows, ptr(buf), ptr(out), cfg.q_heads * R.HD)
        assert rc != 0, (rows, ctx_rows)
