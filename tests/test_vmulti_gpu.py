"""The batched verify attention (svln_op_attention_verify_multi: attn_verify_multi_kernel + the multi form of the verify merge) on the
scenarios of tests/vmulti_ref.py: S sequences in one launch, each on its own page table (scrambled), at its own position, with its own
row count, on disjoint tables and on the fork layout.  The pools are filled with the finite sentinel, the partials with NaN, the outputs
with a NaN canary (the setup of tests/test_verify_attn_gpu.py).  Per sequence: the outputs and the appended K / V rows are BIT-EQUAL to
svln_op_attention_verify on that sequence alone; the outputs are within Case.tolerance(q_flips=True) of float64, the appended K within
roped_k_bound, V exact; every other pool slot (the shared pages of a fork included) is untouched; the rows of a 0-row sequence and the row
slots beyond R_z still hold the canary."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ref as R
import vmulti_ref as VM
from streamvln_amd.config import CONFIGS
from test_attention_gpu import check_untouched, chk, engine, kv_read, setup, _close_engines  # noqa: F401
from util import ptr

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
PI32 = C.POINTER(C.c_int32)


def i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(PI32)


def run_multi(m, cfg, dtype, name, share):
    """the scenario through svln_op_attention_verify_multi -> raw output [S, T, q_heads * 128] (engine dtype, host; NaN canary)"""
    _, T, _, seqs = VM.SCENARIOS[name]
    cs = VM.cases(name, dtype)
    S, ld, od = len(seqs), (cfg.q_heads + 2 * cfg.kv_heads) * R.HD, cfg.q_heads * R.HD
    ctx_rows = max(max(p for p, _ in seqs), 1)
    ctx = torch.zeros((S, ctx_rows, ld), dtype=dtype)
    new = torch.zeros((S, T, ld), dtype=dtype)
    for z, (P, _) in enumerate(seqs):
        rows = cs[z].qkv_rows().to(dtype)
        ctx[z, :P], new[z] = rows[:P], rows[P:]
    dctx, dnew = ctx.cuda(), new.cuda()
    out = torch.full((S * T, od), float("nan"), dtype=dtype, device="cuda")
    cl, clp = i32([p for p, _ in seqs])
    rw, rwp = i32([r for _, r in seqs])
    torch.cuda.synchronize()
    chk(m._lib.svln_op_attention_verify_multi(m._h, S, T, ptr(dctx), ld, ctx_rows, clp, ptr(dnew), rwp, int(share), ptr(out), od))
    return out.cpu().view(S, T, od)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(VM.SCENARIOS))
def test_attention_verify_multi(name, dtype):
    cfg_name, T, layout, seqs = VM.SCENARIOS[name]
    cfg = CONFIGS[cfg_name]
    m = engine(cfg, dtype)
    S, od, share = len(seqs), cfg.q_heads * R.HD, layout == "fork"
    pages = setup(m, S, 900 + 7 * sorted(VM.SCENARIOS).index(name))
    cs = VM.cases(name, dtype)
    got = run_multi(m, cfg, dtype, name, share)
    q0 = seqs[0][0] // R.PAGE if share else 0
    written, kv = [], []
    for z, (P, Rz) in enumerate(seqs):
        lo = q0 * R.PAGE if share and z > 0 else 0
        hi = P + Rz
        # a fork sequence reads its shared positions through sequence 0's pages, the rest through its own
        K, V = kv_read(m, cfg, z, hi) if hi > 0 else (torch.zeros(0, cfg.kv_heads, R.HD, dtype=torch.float64),) * 2
        if share and z > 0 and lo > 0:
            K0, V0 = kv_read(m, cfg, 0, lo)
            K, V = torch.cat([K0, K[lo:]]), torch.cat([V0, V[lo:]])
        kv.append((K, V))
        if hi > lo:
            written.append((pages[z], lo, hi))
    check_untouched(m, cfg, dtype, R.MAX_POSITIONS, written, f"multi {name}")
    for z, (P, Rz) in enumerate(seqs):
        what = f"multi {name} sequence {z} (P {P}, rows {Rz})"
        assert bool(torch.isnan(got[z, Rz:].float()).all()), f"{what}: a row slot beyond the sequence's rows was written"
        K, V = kv[z]
        c, hi = cs[z], P + Rz
        if hi:
            kref, kb = R.roped_k_bound(c.k_in[:hi], torch.arange(hi), cfg.rope_theta, dtype)
            assert bool(((K - kref).abs() <= kb).all()), f"{what}: roped K"
            assert torch.equal(V, c.v[:hi]), f"{what}: V rows not bit-equal"
        if Rz == 0:
            continue
        o = got[z, :Rz].double().view(Rz, cfg.q_heads, R.HD)
        assert torch.isfinite(o).all(), f"{what}: non-finite output"
        Kfull = torch.cat([K, c.k[hi:]])              # (the row slots the launch did not append are masked for every row it computed)
        exp = c.attend(k=Kfull, device="cuda")[:Rz]
        tol = c.tolerance(k=Kfull, q_flips=True, device="cuda")[:Rz]
        ratio = float(((o.cuda() - exp).abs() / tol).amax())
        assert ratio <= 1.0, f"{what}: max err / tolerance {ratio:.3g}"
    # the single-sequence launch on every sequence alone (env 0, its own scrambled pages): bit-equal outputs and appended rows
    ld = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD
    for z, (P, Rz) in enumerate(seqs):
        if Rz == 0:
            continue
        rows = cs[z].qkv_rows().to(dtype)
        dctx, dnew = rows[:max(P, 1)].clone().cuda(), rows[P:P + Rz].clone().cuda()
        one = torch.full((Rz, od), float("nan"), dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        chk(m._lib.svln_op_attention_verify(m._h, Rz, ptr(dctx), ld, P, ptr(dnew), ptr(one), od))
        K1, V1 = kv_read(m, cfg, 0, P + Rz)
        what = f"multi {name} sequence {z} against the single-sequence launch"
        assert torch.equal(one.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           got[z, :Rz].contiguous().view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), f"{what}: outputs differ"
        assert torch.equal(K1[P:], kv[z][0][P:]) and torch.equal(V1[P:], kv[z][1][P:]), f"{what}: appended rows differ"


def test_attention_verify_multi_refusals():
    cfg = CONFIGS["true_dims_1layer"]
    m = engine(cfg, torch.bfloat16)
    setup(m, 8, 31)
    ld, od = (cfg.q_heads + 2 * cfg.kv_heads) * R.HD, cfg.q_heads * R.HD
    buf = torch.zeros((8 * 8, ld), dtype=torch.bfloat16, device="cuda")
    out = torch.zeros((8 * 8, od), dtype=torch.bfloat16, device="cuda")

    def call(S, T, ctx_len, rows, share=0):
        cl, clp = i32(ctx_len)
        rw, rwp = i32(rows)
        return m._lib.svln_op_attention_verify_multi(m._h, S, T, ptr(buf), ld, 8, clp, ptr(buf), rwp, share, ptr(out), od)

    assert call(2, 4, [2, 3], [4, 1]) == 0
    assert call(0, 4, [0], [1]) != 0                                   # S outside 1 .. 8
    assert call(9, 4, [0] * 9, [1] * 9) != 0
    assert call(2, 5, [0, 0], [1, 1]) != 0                             # T * (q_heads / kv_heads) > 32
    assert call(2, 4, [0, 0], [5, 1]) != 0                             # a row count past T
    assert call(2, 4, [0, 0], [1, -1]) != 0
    assert call(2, 4, [1, 2], [1, 1], share=1) != 0                    # a fork needs equal context lengths
    # a position at or past max_positions (the context length itself is refused past the context rows handed over)
    big = torch.zeros((2 * R.MAX_POSITIONS, ld), dtype=torch.bfloat16, device="cuda")
    cl, clp = i32([R.MAX_POSITIONS - 2, 0])
    rw, rwp = i32([4, 1])
    assert m._lib.svln_op_attention_verify_multi(m._h, 2, 4, ptr(big), ld, R.MAX_POSITIONS, clp, ptr(buf), rwp, 0, ptr(out), od) != 0
    # a page the sequence does not hold: its list covers one page, the pass crosses into the second
    one_page = np.asarray([5], np.int32)
    chk(m._lib.svln_op_set_pages(m._h, 1, one_page.ctypes.data_as(PI32), 1))
    cl, clp = i32([0, 62])
    rw, rwp = i32([1, 4])
    assert m._lib.svln_op_attention_verify_multi(m._h, 2, 4, ptr(big), ld, R.MAX_POSITIONS, clp, ptr(buf), rwp, 0, ptr(out), od) != 0
    assert "does not hold" in m._lib.svln_last_error().decode()
    setup(m, 8, 31)
    assert call(2, 4, [2, 3], [4, 1]) == 0
