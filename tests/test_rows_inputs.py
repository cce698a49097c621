"""CPU proof that the inputs of tests/test_rows_gpu.py are sharp.  On every case of tests/rows_ref.py each plausible kernel mistake that
applies to the case (the "mutant" references of that module) changes a stored bit of the expected output (exact families: taps, gathers,
frame hash, prune selection, patchify), or moves it by at least 10x the bound the GPU test applies (toleranced families: norms, prune
scores, pool; the ratio tests/test_gemv_inputs.py uses).  Every toleranced bound is checked from both sides: the float64 reference
rounded to the engine type lies within it, and a plain fp32 restatement that sums in the kernel's order lies within half of it.  Each test
prints its mutants with the bits changed / the ratio (pytest -s, or on failure)."""
import numpy as np
import pytest
import torch

import rows_ref as R


def _check(cid, report, exact):
    print(f"{cid}: " + ", ".join(f"{k} {v if exact else round(v, 1)}" for k, v in report.items()))
    weak = {k: v for k, v in report.items() if not (v >= 1 if exact else v >= R.RATIO)}
    assert not weak, f"{cid}: mutants the case cannot see: {weak} (all: {report})"


def _two_sided(cid, ref, bound, restated, dtype):
    """the bound is neither below what the number format forces nor far above what fp32 in the kernel's order needs"""
    rounding = np.abs(R.rt(ref, dtype) - ref)
    assert (rounding <= bound).all(), (cid, float((rounding / bound).max()))
    fp32 = np.abs(restated - ref)
    assert (fp32 <= 0.5 * bound).all(), (cid, float((fp32 / bound).max()))
    print(f"{cid}: rounding / bound {float((rounding / bound).max()):.3f}, fp32 restatement / bound {float((fp32 / bound).max()):.3f}")


# ---------------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("case", R.NORM_CASES, ids=lambda c: c.id)
def test_norm_inputs_are_discriminating(case):
    case.build()
    ref, bound = case.reference(), case.bound()
    assert (R.rt(case.x, case.dtype) == case.x).all() and np.isfinite(ref).all()
    sg, sb = np.sign(case.g), np.sign(case.b)
    assert (sg != sg[::-1]).any() and (sg != -sg[::-1]).any() and (sb != sb[::-1]).any()       # (d) no symmetry under reversal
    if case.family == "eps":
        ms = (case.x ** 2).mean(1)
        assert ((0.1 * R.EPS < ms) & (ms < 10 * R.EPS)).all(), (case.id, ms)
    if case.family == "offset":
        spread = case.x.std(1) / np.abs(case.x.mean(1))
        assert (spread < 2.0 ** -4).all(), (case.id, spread)
    for ci in case.hot_chunks():                                        # the distinctive values sit where the family says, and only there
        assert (np.abs(case.x[:, ci * case.epc:(ci + 1) * case.epc]) >= 2).all()
    if case.hot_chunks():
        assert int((np.abs(case.x) >= 2).sum()) == case.rows * case.epc * len(case.hot_chunks())
    _two_sided(case.id, ref, bound, case.kernel_order(), case.dtype)
    muts = {m: case.reference(m) for m in case.mutants()}
    if case.cancel is not None:                                         # the constructed column carries the unbiased-variance mutant by itself
        c0 = case.cancel
        assert abs(ref[0, c0]) <= 2.0 ** -7 * abs(case.b[c0])
        alone = abs(muts["unbiased_var"][0, c0] - ref[0, c0]) / bound[0, c0]
        print(f"{case.id}: unbiased_var at the cancelling column alone {alone:.1f}")
        assert alone >= R.RATIO, (case.id, alone)
    if case.family == "offset" and case.dtype == torch.bfloat16:
        assert ((case.x == 256) | (case.x == 258)).all() and ((case.x == 258).sum(1) == 1).all()
        assert ("one_pass_var" in muts) == (case.n > 1024)
    _check(case.id, R.toleranced_report(ref, bound, muts), exact=False)


def test_norm_case_list_covers_the_lane_striding():
    """every width in both engine types, every row count, the families wherever the width has the chunk they need"""
    seen = {(c.op, c.dtype, c.n, c.family) for c in R.NORM_CASES}
    for op in ("rms", "ln"):
        for dt in R.DTYPES:
            for n in R.WIDTHS:
                assert n % R.EPC[dt] == 0
                for fam in R.NORM_FAMILIES:
                    assert ((op, dt, n, fam) in seen) == R.NormCase.exists(op, dt, n, fam)
            assert {c.rows for c in R.NORM_CASES if c.op == op and c.dtype == dt} == set(R.ROWS)
    nch = {(R.NAME[dt], n): n // R.EPC[dt] for dt in R.DTYPES for n in R.WIDTHS}
    assert nch[("bf16", 144)] == 18 and nch[("bf16", 512)] == 64 and nch[("bf16", 520)] == 65 and nch[("fp32", 512)] == 128 and nch[("fp32", 520)] == 130
    every = {m for c in R.NORM_CASES for m in c.mutants()}
    assert every == {"gain_shifted", "bias_dropped", "unbiased_var", "divisor_rounded", "drop_last_chunk", "drop_past_first_sweep", "lane63_skipped",
                     "eps_dropped", "eps_outside_root", "one_pass_var"}


# ---------------------------------------------------------------------------------------------------------- tap and indexed norm
def _distinct_rows(dtype, n):
    y = R.bits(R.to_t(R.tap_input(dtype, n).reference(), dtype))
    assert len({tuple(r.tolist()) for r in y}) == y.shape[0]            # a row in the wrong place is a changed bit


@pytest.mark.parametrize("case", R.TAP_CASES, ids=lambda c: c.id)
def test_tap_inputs_are_discriminating(case):
    _distinct_rows(case.dtype, case.n)
    ref = case.maps()
    assert ref[0] == (not case.skip) and ref[1][case.y2_cap] == -1      # the canary row after the tap is never a target
    if not case.skip:
        assert sorted(t for t in ref[1] if t >= 0) == list(range(case.rows)) or case.y2_row + case.rows > case.y2_cap
        first = min(case.y2_row, case.y2_cap - 1)
        assert ref[1][first] == 0
    _check(case.id, {m: int(case.maps(m) != ref) for m in case.mutants()}, exact=True)


def test_tap_case_list():
    for dt in R.DTYPES:
        for n in R.WIDTHS:
            cs = [c for c in R.TAP_CASES if c.dtype == dt and c.n == n]
            assert any(c.y2_row == 0 for c in cs) and any(c.y2_row == c.y2_cap - 1 for c in cs) and any(c.y2_row >= c.y2_cap for c in cs)
            assert any(c.skip for c in cs) and any(c.rows >= 4 for c in cs)
    assert {m for c in R.TAP_CASES for m in c.mutants()} == {"skip_ignored", "no_offset", "clamp_to_cap"}


@pytest.mark.parametrize("case", R.INDEXED_CASES, ids=lambda c: c.id)
def test_indexed_inputs_are_discriminating(case):
    _distinct_rows(case.dtype, case.n)
    ref = case.maps()
    assert case.src != list(range(case.rows)) and max(case.src) < case.x_rows
    if case.rows > 1:
        assert len(set(case.src)) < case.rows                           # a repeated source
        assert {-1, 0, case.tap_cap - 1} <= set(case.tap_rows)
    _check(case.id, {m: int(case.maps(m) != ref) for m in case.mutants()}, exact=True)


# ---------------------------------------------------------------------------------------------------------- gathers
@pytest.mark.parametrize("case", R.GATHER_CASES + R.RAGGED_CASES, ids=lambda c: c.id)
def test_gather_inputs_are_discriminating(case):
    embed, feats = R.tables(case.dtype)
    both = np.concatenate([embed, feats])
    assert len({r.tobytes() for r in both}) == both.shape[0]            # distinct per-row patterns
    if isinstance(case, R.RaggedCase):
        ref = case.reference(embed)
        dests = [d for d, _ in case.pairs]
        assert len(set(dests)) == len(dests) and max(dests) < case.OUT_ROWS
        if case.rows > 1:
            assert dests != sorted(dests) and len(dests) < max(dests) + 1           # out of order, with gaps
        _check(case.id, {m: int(case.reference(embed, m) != ref) for m in case.mutants()}, exact=True)
        return
    ref = case.reference(embed, feats)
    if case.rows > 1:
        assert {0, R.VOCAB - 1, -1, -R.FEAT_ROWS} <= set(case.src.tolist())
    report = {}
    for m in case.mutants():
        mut = case.reference(embed, feats, m)
        report[m] = int(mut is not None) if ref is None else int((mut != ref).any(1).sum())
    _check(case.id, report, exact=True)


def test_gather_case_list():
    assert {c.rows for c in R.GATHER_CASES} == {1, 300}
    assert {m for c in R.GATHER_CASES + R.RAGGED_CASES for m in c.mutants()} == {"neg_without_plus1", "zero_to_feats", "skip_ignored", "pair_swapped"}


# ---------------------------------------------------------------------------------------------------------- frame hash
@pytest.mark.parametrize("F", R.HASH_FRAMES)
@pytest.mark.parametrize("words", R.HASH_WORDS)
def test_hash_inputs_are_discriminating(F, words):
    pix = R.hash_words(F, words)
    ref = R.frame_keys(pix)
    assert len({tuple(k) for k in ref.tolist()}) == F
    report = {m: int((R.frame_keys(pix, m) != ref).sum()) for m in R.hash_mutants(F, words)}
    _check(f"hash-F{F}-w{words}", report, exact=True)
    # the properties the GPU test asserts hold for the reference: order matters, one bit matters, the batch slot does not
    one = pix[:1].copy()
    i, j = 3, words - 2
    assert one[0, i] != one[0, j]
    swapped = one.copy()
    swapped[0, [i, j]] = one[0, [j, i]]
    flipped = one.copy()
    flipped[0, words // 2] ^= 1
    base = R.frame_keys(one)[0]
    for other in (swapped, flipped):
        k = R.frame_keys(other)[0]
        assert k[0] != base[0] and k[1] != base[1]
    assert (R.frame_keys(swapped, "index_left_out")[0] == R.frame_keys(one, "index_left_out")[0]).all()      # the order-blind key
    if F > 1:
        moved = pix.copy()
        moved[F - 1] = pix[0]
        assert (R.frame_keys(moved)[F - 1] == ref[0]).all()


def test_hash_constants_are_the_project_s():
    import os
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "streamvln_amd", "csrc")
    text = open(os.path.join(src, "common.h")).read() + open(os.path.join(src, "misc.hip")).read()
    for c in (R._C1, R._C2, R._KA, R._KM, R._KB):
        assert f"0x{int(c):016X}ull" in text, hex(int(c))
    assert R.ENGINE_WORDS % (64 * 256) == 0 and R.HASH_WORDS[1] % (64 * 256) == 5 and R.HASH_WORDS[2] < 256


# ---------------------------------------------------------------------------------------------------------- memory prune
@pytest.mark.parametrize("case", R.PRUNE_CASES, ids=lambda c: c.id)
def test_prune_inputs_are_discriminating(case):
    case.build()
    sel, s = case.reference()
    bound = case.score_bound()
    assert np.isfinite(s).all() and len(sel) == case.keep == len(set(sel))
    assert (R.rt(case.mem, case.dtype) == case.mem).all()
    gap = case.cut_gap()
    if case.kind == "identical":
        assert gap == 0.0 and sel == list(range(case.keep)) and len(set(s.tolist())) <= 2
    elif case.pair:                                                     # the only tie is the built one, exactly at the cut
        p, q = case.pair
        assert (case.mem[p] == case.mem[q]).all() and gap == 0.0 and p in sel and q not in sel
        order = np.sort(s)
        lo = order[case.keep - 1] - order[case.keep - 2] if case.keep >= 2 else np.inf
        hi = order[case.keep + 1] - order[case.keep] if case.keep + 1 < case.N else np.inf
        print(f"{case.id}: gaps beside the tie {lo:.3e} / {hi:.3e}, bound {bound.max():.3e}")
        assert min(lo, hi) >= R.RATIO * bound.max(), (case.id, lo, hi, float(bound.max()))
    else:
        assert gap >= R.RATIO * bound.max(), (case.id, gap, float(bound.max()))
    if case.kind == "graded" and case.keep > 8:                         # survivors on both sides of every boundary the size has
        for a in (63, 1023, 1087):
            if a + 1 < case.N:
                assert a in sel and a + 1 in sel, (case.id, a)
        if case.N > 1088:
            assert {1023, 1024, 1087, 1088} <= set(sel)
    if case.kind == "zero-row":
        assert s[5] == 0.0 and 5 in sel
    if case.kind == "clamp-edge":
        den = np.linalg.norm(case.mem, axis=1) * np.linalg.norm(case.mem.mean(0))
        assert (den > 1.2e-20).all() and (den < 1.9e-20).all(), (float(den.min()), float(den.max()))
    # fp32 in the kernel's order: 64-row blocks, block sums, fmaf chains per lane (restated without the fused rounding), the wave tree
    f = np.float32
    m32 = case.mem.astype(f)
    blocks = [m32[r0:r0 + 64] for r0 in range(0, case.N, 64)]
    part = []
    for blk in blocks:
        acc = np.zeros(R.HIDDEN, dtype=f)
        for r in blk:
            acc = acc + r
        part.append(acc)
    mu = np.zeros(R.HIDDEN, dtype=f)
    for pt in part:
        mu = mu + pt
    mu = mu / f(case.N)
    epc = R.EPC[case.dtype]
    dot, nn, mm = (R.lane_sum32(t, epc) for t in (m32 * mu[None], m32 * m32, np.broadcast_to(mu * mu, m32.shape).copy()))
    restated = (dot / np.maximum(np.sqrt(nn) * np.sqrt(mm), f(1e-20))).astype(np.float64)
    err = np.abs(restated - s)
    assert (err <= 0.5 * bound).all(), (case.id, float((err / bound).max()))
    report = {}
    for mname in case.mutants():
        msel, ms = case.reference(mname)
        moved = R.toleranced_report(s, bound, {mname: ms})[mname]
        report[mname] = int(msel != sel) or int(moved >= R.RATIO)
    _check(case.id, report, exact=True)


def test_prune_case_list_and_the_scaled_mean():
    assert {c.N for c in R.PRUNE_CASES} == set(R.PRUNE_N)
    for N in R.PRUNE_N:
        assert {c.keep for c in R.PRUNE_CASES if c.N == N and c.kind == "graded"} == {1, max(N // 2, 1), N}
    assert {m for c in R.PRUNE_CASES for m in c.mutants()} == {"largest_kept", "ties_to_higher", "base_not_carried", "unclamped", "mean_divisor_rounded"}
    # away from the clamp a scaled mean cannot be seen: the cosine ignores it (why the mutant is listed for the clamp-edge case only)
    for c in R.PRUNE_CASES:
        if c.kind == "graded" and c.N % 64:
            assert np.abs(c.scores("mean_divisor_rounded") - c.scores()).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------- pool and patchify
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
@pytest.mark.parametrize("kind", ["gradient", "one-hot"])
def test_pool_inputs_are_discriminating(dtype, kind):
    x = R.pool_input(dtype, kind)
    assert (R.rt(x, dtype) == x).all() and (x[0] != x[1]).any()
    ref, bound = R.pool_ref(x, want_bound_for=dtype)
    f = np.float32
    x32 = x.astype(f).reshape(R.POOL_F, R.SIDE, R.SIDE, R.POOL_C)
    taps = R.pool_taps()
    restated = np.empty_like(ref)
    for oy, (y0, y1, wy0, wy1) in enumerate(taps):
        for ox, (x0, x1, wx0, wx1) in enumerate(taps):
            restated[:, oy * R.OSIDE + ox] = f(wy0) * (f(wx0) * x32[:, y0, x0] + f(wx1) * x32[:, y0, x1]) + f(wy1) * (f(wx0) * x32[:, y1, x0] + f(wx1) * x32[:, y1, x1])
    _two_sided(f"pool-{R.NAME[dtype]}-{kind}", ref, bound, restated, dtype)
    if kind == "gradient":
        grid = x.reshape(R.POOL_F, R.SIDE, R.SIDE, -1)
        for f in range(R.POOL_F):                                       # different gradients in y and x, in each frame
            assert abs(np.diff(grid[f], axis=0).mean() - np.diff(grid[f], axis=1).mean()) > 0.1
    _check(f"pool-{R.NAME[dtype]}-{kind}", R.toleranced_report(ref, bound, {m: R.pool_ref(x, m) for m in R.POOL_MUTANTS}), exact=False)


def test_pool_taps_never_reach_the_border():
    """why "border tap not clamped" has no case: no tap of the 27 -> 14 geometry needs the clamp, and every input row and column is read"""
    taps = R.pool_taps()
    assert all(i0 + 1 == i1 <= R.SIDE - 1 for i0, i1, _, _ in taps) and all((d + 0.5) * R.SIDE / R.OSIDE - 0.5 > 0 for d in range(R.OSIDE))
    assert max(i1 for _, i1, _, _ in taps) == R.SIDE - 1 and min(i0 for i0, _, _, _ in taps) == 0


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_patchify_inputs_are_discriminating(dtype):
    pix = R.pixels(dtype)
    assert (R.rt(pix, dtype) == pix).all()
    ref = R.patchify_ref(pix)
    assert ref.shape == (R.POOL_F * R.SIDE * R.SIDE, R.KP) and (ref[:, R.KREAL:] == 0).all()
    assert ref[R.SIDE + 2, 14 * 14 + 3 * 14 + 5] == pix[0, 1, 14 + 3, 2 * 14 + 5]
    _check(f"patchify-{R.NAME[dtype]}", {m: int((R.patchify_ref(pix, m) != ref).sum()) for m in R.PATCHIFY_MUTANTS}, exact=True)
