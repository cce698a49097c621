"""CPU restatement, designed inputs and mutants of the engine's per-row e4m3 quantisers (test infrastructure): quant_fp8_rows_kernel in
csrc/gemv.hip behind svln_op_quant_fp8, and the same arithmetic in the e4m3 branch of splitk_rownorm_kernel in csrc/gemm.hip behind
svln_op_gemm_norm_q8.

  encoder   e4m3_encode is OCP e4m3fn (bias 7, no infinity, NaN = 0x7F, largest finite 448 = 0x7E), round to nearest even, written on the
            integer bits of the fp32 value.  It does not use torch.float8_e4m3fn; tests/test_quant_inputs.py holds the two against each
            other, which also checks the encoder of the oracle's fp8 modes (oracle.qdq_e4m3_rows).
  rows      quant_rows restates the kernels' operation order in float32:
              amax = max |w| over the row, a NaN ignored (fmaxf);
              sc = max(amax / 448, 2^-126), 1 for amax == 0       (the floor keeps 1 / sc finite and normal)
              inv = fl(1 / sc);  x = fl(w * inv);  x = x if x != x else min(max(x, -448), 448);  byte = e4m3_encode(x).
            A NaN element gives a NaN byte and changes nothing else.  An infinite element makes the scale infinite: the finite elements
            become 0 and the infinite one NaN (inf * 0).
  fold      -0 (0x80) and +0, and the two NaN bytes (0xFF, 0x7F), are the same value: fold() maps them onto 0x00 / 0x7F before bytes are
            compared.  Every comparison is bit equality after the fold, scales by their fp32 bits.
  cases     CASES: small bf16 matrices (cols % 16 == 0) on which a subtly wrong quantiser fails; each names the mutants it is written to
            catch.  MUTANTS: quant_rows with one such mistake.  tests/test_quant_inputs.py proves every pairing on the CPU.
"""
from collections import namedtuple

import numpy as np
import torch

F32 = np.float32
E4M3_MAX = F32(448.0)
FLOOR = F32(2.0 ** -126)               # the smallest normal fp32: 1 / FLOOR = 2^126 is finite
BLOCK = 256                            # threads of quant_fp8_rows_kernel: thread t reads the 8-element chunks t, t + 256, ...


# ----------------------------------------------------------------------------- encoder / decoder
def e4m3_encode(x, rnd="even", bias=7, top=0x7E, over=0x7F, nan=0x7F, flush_sub=False):
    """fp32 -> e4m3 byte (numpy uint8).  Defaults = OCP e4m3fn with round to nearest even; a magnitude that rounds above 448 and an
    infinity give the NaN byte (as torch does: the kernels clamp first, so they never get there).  The other arguments exist for the
    mutants: rnd "trunc" / "away", the fnuz layout (bias 8, top 0x7F, NaN 0x80), subnormal codes flushed to 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.int64)
    sign, a = (b >> 31) & 1, b & 0x7FFFFFFF
    e, man = (a >> 23) - 127, a & 0x7FFFFF
    sig = np.where(e == -127, man, man | 0x800000)              # |x| = sig * 2^(ee - 23)
    ee = np.maximum(e, -126)
    emin = 1 - bias                                             # exponent of the smallest normal of the target
    shift = np.minimum(20 + np.maximum(emin - ee, 0), 40)       # low bits that go: 20 for a normal result, more below emin
    qv, rem, half = sig >> shift, sig & (np.left_shift(1, shift) - 1), np.left_shift(1, shift - 1)
    if rnd == "even":
        up = (rem > half) | ((rem == half) & ((qv & 1) == 1))
    elif rnd == "away":
        up = rem >= half
    else:
        assert rnd == "trunc", rnd
        up = np.zeros_like(qv, dtype=bool)
    qv = qv + up
    # normal result: qv in [8, 16] counts eighths of 2^ee; subnormal result: qv in [0, 8] counts 2^(emin - 3); one formula serves both
    code = (np.maximum(ee - emin, 0) << 3) + qv
    if flush_sub:
        code = np.where(code < 8, 0, code)
    code = np.where(code > top, over, code) | (sign << 7)
    code = np.where(a > 0x7F800000, nan, code)
    return code.astype(np.uint8)


def _decode_table():
    t = np.empty(256, dtype=np.float32)
    for c in range(128):
        e, m = c >> 3, c & 7
        v = m * 2.0 ** -9 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c], t[c + 128] = v, -v
    t[0x7F] = t[0xFF] = np.nan
    return t


DECODE = _decode_table()


def e4m3_decode(byte):
    return DECODE[np.asarray(byte, dtype=np.uint8)]


def fold(b):
    b = np.asarray(b, dtype=np.uint8)
    return np.where(b == 0x80, 0x00, np.where(b == 0xFF, 0x7F, b)).astype(np.uint8)


# ----------------------------------------------------------------------------- the rows
def _f32(W):
    if isinstance(W, torch.Tensor):
        W = W.detach().to(torch.float32).cpu().numpy()
    W = np.ascontiguousarray(W, dtype=np.float32)
    assert W.ndim == 2 and W.shape[1] % 16 == 0, W.shape
    return W


def _left_out(mutant, cols):
    """columns a mutant leaves out of the row maximum (None: none)"""
    chunk = np.arange(cols) // 8
    if mutant == "drop_last_chunk":
        return chunk == cols // 8 - 1
    if mutant in ("drop_wave0", "drop_wave1", "drop_wave2", "drop_wave3"):
        return (chunk % BLOCK) // 64 == int(mutant[-1])
    if mutant in ("iter2_max", "iter2_bytes"):
        return chunk >= BLOCK
    return None


MUTANTS = ("trunc", "ties_away", "fnuz", "amax_240", "max_no_abs", "drop_last_chunk", "drop_wave0", "drop_wave1", "drop_wave2",
           "drop_wave3", "iter2_max", "iter2_bytes", "div_by_scale", "prev_row_scale", "flush_sub", "nan_to_448", "no_floor")


def quant_rows(W, mutant=None):
    """bf16 values [rows][cols] (torch or numpy) -> (bytes uint8 [rows][cols], scale float32 [rows]).  mutant: one of MUTANTS.
       nan_to_448   the clamp written as fminf(fmaxf(x, -448), 448): a NaN becomes -448
       no_floor     no scale floor: 1 / sc overflows for amax <= 1.3166e-36 and the row's zeros become 0 * inf = NaN
    (the two together are the kernels before the floor and the NaN rule were added)."""
    assert mutant is None or mutant in MUTANTS, mutant
    w = _f32(W)
    cols = w.shape[1]
    a = w.copy() if mutant == "max_no_abs" else np.abs(w)
    out = _left_out(mutant, cols)
    if out is not None:
        a = np.where(out[None, :], F32(0), a)
    amax = np.fmax.reduce(a, axis=1, initial=F32(0))            # fmax: a NaN operand is ignored
    with np.errstate(all="ignore"):
        sc = np.where(amax > 0, amax / (F32(240.0) if mutant == "amax_240" else E4M3_MAX), F32(1)).astype(np.float32)
        if mutant != "no_floor":
            sc = np.maximum(sc, FLOOR)
        if mutant == "prev_row_scale":
            sc = np.roll(sc, 1)
        inv = (F32(1) / sc).astype(np.float32)
        x = (w / sc[:, None] if mutant == "div_by_scale" else w * inv[:, None]).astype(np.float32)
        if mutant == "nan_to_448":
            x = np.fmin(np.fmax(x, -E4M3_MAX), E4M3_MAX)
        else:
            x = np.minimum(np.maximum(x, -E4M3_MAX), E4M3_MAX)  # (numpy's maximum / minimum keep a NaN)
    kw = {"trunc": dict(rnd="trunc"), "ties_away": dict(rnd="away"), "fnuz": dict(bias=8, top=0x7F, over=0x7F, nan=0x80),
          "flush_sub": dict(flush_sub=True)}.get(mutant, {})
    q = e4m3_encode(x, **kw)
    if mutant == "iter2_bytes":
        q = np.where(out[None, :], np.uint8(0), q)
    return q, sc


def scaled(W):
    """fl(w * inv) of quant_rows before the clamp (the coverage checks read it)"""
    w = _f32(W)
    _, sc = quant_rows(w)
    with np.errstate(all="ignore"):
        return (w * (F32(1) / sc)[:, None]).astype(np.float32)


def same(got, exp):
    """(bytes, scale) pairs equal: bytes after the fold, scales by their bits"""
    return bool(np.array_equal(fold(got[0]), fold(exp[0]))) and bool(np.array_equal(np.asarray(got[1], dtype=np.float32).view(np.uint32),
                                                                                   np.asarray(exp[1], dtype=np.float32).view(np.uint32)))


# ----------------------------------------------------------------------------- cases
# id; W: fp32 tensor of bf16 values; mutants: the mutants the case is written to catch;
# finite: no NaN / inf in W; info: what the builder wants checked about itself
Case = namedtuple("Case", "id W mutants finite info")

GRID = DECODE[:0x7F].astype(np.float64)                         # the 127 non-negative finite values, codes 0x00 .. 0x7E
MIDS = (GRID[:-1] + GRID[1:]) / 2                               # the 126 midpoints, 2^-10 (between 0 and 2^-9) first
TIE_K = (-20, -3, 0, 5, 60)


def _bf16_step(v, d):
    """the bf16 value d steps from the positive bf16 value v"""
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    assert not (b & 0xFFFF).any()
    return ((((b >> 16).astype(np.int64) + d) << 16).astype(np.uint32)).view(np.float32).astype(np.float64)


def _as_case(cid, W, mutants, finite=True, **info):
    W = torch.as_tensor(np.asarray(W, dtype=np.float32))
    fin = torch.isfinite(W)
    Wb = W.to(torch.bfloat16).to(torch.float32)
    assert torch.equal(Wb[fin], W[fin]) and W.shape[1] % 16 == 0, cid       # every value is a bf16 value
    assert bool(fin.all()) == finite, cid
    return Case(cid, W, tuple(mutants), finite, info)


def _tie_case():
    """one row per k of TIE_K with amax = 448 * 2^k: every grid value, every midpoint and the midpoint's two bf16 neighbours, in both
    signs (1010 values, zero padded to 1024 columns).  sc = 2^k and inv = 2^-k exactly, so fl(w * inv) is the value itself."""
    pos = np.concatenate([GRID, MIDS, _bf16_step(MIDS, -1), _bf16_step(MIDS, +1)])
    row = np.concatenate([pos, -pos, np.zeros(1024 - 2 * len(pos))])
    W = np.stack([row * 2.0 ** k for k in TIE_K])
    mid_cols = np.concatenate([len(GRID) + np.arange(len(MIDS)), len(pos) + len(GRID) + np.arange(len(MIDS))])
    return _as_case("ties", W, ("trunc", "ties_away", "fnuz", "amax_240", "flush_sub", "prev_row_scale"), mid_cols=mid_cols)


def amax_class(a):
    """-1 / 0 / +1: fl(amax * fl(1 / fl(amax / 448))) below / equal to / above 448"""
    a = F32(a)
    p = a * (F32(1) / (a / E4M3_MAX))
    return int(p > E4M3_MAX) - int(p < E4M3_MAX)


def _bf16_rand(shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(torch.float32).numpy()


def _scale_cases():
    """amax values whose scale is no power of two, three of each class of amax_class, each over 62 random values below it and
    amax / 2; and rows on which fl(w * inv) and fl(w / sc) encode differently (found by search)."""
    picks = {-1: [], 0: [], 1: []}
    for m in range(1, 128):                                     # bf16 values 1 + m / 128 times assorted exponents
        for k in (-9, 0, 4):
            a = (1.0 + m / 128.0) * 2.0 ** k
            c = amax_class(a)
            if len(picks[c]) < 3:
                picks[c].append(a)
    assert all(len(v) == 3 for v in picks.values()), picks
    rows = []
    for i, a in enumerate(picks[0] + picks[-1] + picks[1]):
        r = _bf16_rand((64,), 100 + i, 0.3) * F32(a)
        r = np.clip(r.astype(np.float32), -a / 2, a / 2)
        r = torch.tensor(r).to(torch.bfloat16).to(torch.float32).numpy()
        r[i % 64], r[(i + 7) % 64] = (a if i % 2 else -a), a / 2
        rows.append(r)
    out = [_as_case("scales", np.stack(rows), ("amax_240", "prev_row_scale", "trunc"), amax=picks)]
    found = []
    for seed in range(400):
        W = _bf16_rand((1, 512), 1000 + seed, 0.02)
        if not np.array_equal(fold(quant_rows(W)[0]), fold(quant_rows(W, "div_by_scale")[0])):
            found.append(W[0])
            if len(found) == 2:
                break
    assert len(found) == 2, "no row separates w * (1 / sc) from w / sc"
    out.append(_as_case("mul-vs-div", np.stack(found), ("div_by_scale",)))
    return out


PLACE_COLS = (16, 48, 528, 2064, 4096 + 16)
_PLACE_K = (-3, 2, -7, 5, 0, -12, 9, 4, -1, 7)


def placements(cols):
    """[(what, column, sign)]: where the row maximum is planted for a row of `cols` columns"""
    out = [("first", 0, 1), ("last", cols - 1, 1)]
    out += [(f"wave{w}", min(512 * w + 13, cols - 3), 1) for w in range(4) if 512 * w < cols]
    if cols > 2048:
        out.append(("iter2", min(2048 + 5, cols - 2), 1))
    if cols > 4096:
        out.append(("iter3", cols - 11, 1))
    out.append(("negative", cols // 2, -1))
    return out


def _placement_case(cols):
    """row r: values below 32 * 2^k and one +-448 * 2^k planted at a chosen column, k different from row to row.  A maximum that misses
    the planted column gives another scale."""
    rows, spots = [], placements(cols)
    for r, (what, col, sign) in enumerate(spots):
        row = np.clip(_bf16_rand((cols,), 300 + cols + r, 8.0), -31.0, 31.0).astype(np.float64)
        if sign < 0:
            row = np.abs(row)                                   # every positive value is small: a maximum without abs sees no -448
        row[col] = sign * 448.0
        rows.append(row * 2.0 ** _PLACE_K[r])
    muts = ["max_no_abs", "drop_last_chunk", "prev_row_scale", "amax_240"] + [f"drop_wave{w}" for w in range(4) if 512 * w < cols]
    if cols > 2048:
        muts += ["iter2_max", "iter2_bytes"]
    return _as_case(f"placement-{cols}", np.stack(rows), muts, spots=spots)


def _bf16_amax_overflowing():
    """the largest bf16 amax for which fl(1 / fl(amax / 448)) is infinite (1.3166e-36), and the bf16 value after it"""
    b = np.arange(1, 0x7F80, dtype=np.uint32) << 16             # every positive finite bf16 value, ascending
    v = b.view(np.float32)
    with np.errstate(all="ignore"):
        bad = np.isinf(F32(1) / (v / E4M3_MAX))
    n = int(bad.sum())
    assert bad[:n].all() and not bad[n:].any() and n == 992, n
    return float(v[n - 1]), float(v[n])


def _edge_row(amax, cols=32):
    row = np.zeros(cols)
    row[3], row[9], row[17], row[30] = amax, -amax / 2, amax / 2, -amax
    return row


def _edge_cases():
    t, t_next = _bf16_amax_overflowing()
    sub = np.zeros(32)
    sub[2], sub[5], sub[11], sub[31] = 2.0 ** -130, -3 * 2.0 ** -133, 2.0 ** -133, -(2.0 ** -127)       # bf16 subnormals
    bmax = float(torch.finfo(torch.bfloat16).max)
    big = _edge_row(bmax)
    big[20], big[21] = 1.0, -bmax / 256
    rows = [np.zeros(32), -np.zeros(32), sub, _edge_row(2.0 ** -126), _edge_row(t), _edge_row(t_next), _edge_row(448 * 2.0 ** -126), big]
    names = ["zero", "minus-zero", "subnormals", "2^-126", "1.3166e-36", "above-1.3166e-36", "448*2^-126", "bf16-max"]
    out = [_as_case("edges", np.stack(rows), ("no_floor",), names=names, tiny=(2, 3, 4))]
    base = np.stack([np.clip(_bf16_rand((48,), 500 + r, 1.0), -3, 3) for r in range(3)]).astype(np.float64)
    base[0, 5], base[1, 40], base[2, 0] = 3.5, -3.5, 3.5                                                # each row's maximum
    spots = [(0, 17), (1, 47), (2, 1)]
    for what, v in (("nan", np.nan), ("inf", np.inf)):
        W = base.copy()
        for r, c in spots:
            W[r, c] = v
        twin = base.copy()
        for r, c in spots:
            twin[r, c] = 0.0
        out.append(_as_case(what, W, ("nan_to_448",) if what == "nan" else (), finite=False, spots=spots, twin=torch.as_tensor(twin.astype(np.float32))))
    return out


def _build():
    return [_tie_case()] + _scale_cases() + [_placement_case(c) for c in PLACE_COLS] + _edge_cases()


CASES = _build()
