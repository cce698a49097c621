"""Inputs of tests/test_p12_depth_gpu.py: P12 weights with fallback blocks planted at chosen places of a wave's load steps.  Built on
tests/p12_ref.py (encoder, designed weights), which can only plant the first, the last or every block.  Test infrastructure.

The packed GEMVs (gemv.hip: WP12, deep_step) stream DEPTH chunk positions per row and step: a wave that owns the blocks b_0 < b_1 < ... of
a row (all of them in the row kernel; every fourth one, from its own index, in the K-split kernel) takes them in steps of DEPTH, then
the remainder one by one, and one wave-uniform branch per step picks the plain decode or the form that fetches fallback blocks from the
bf16 original.  A pattern names own-block indices; a row group gets one pattern, on one of its rows or on all of them, so that clean
steps, mixed steps and steps with several fallback rows all occur in one launch."""
import functools

import numpy as np
import torch

import p12_ref as R

ROWS_DEPTH, KS_DEPTH, KS_KW = 3, 3, 4            # WP12::DEPTH, WP12::KS_DEPTH, the K-split kernel's waves on K (gemv.hip)
PATTERNS = ("none", "first", "middle", "last", "remainder", "adjacent", "row", "ragged", "special", "special_nan")
MAIN_H = (58, 59, 60, 61)                        # hi7 classes of a special row beside 0 (-0, denormals) and 127 (NaN)


def own_blocks(nblk, kernel, kw):
    return list(range(nblk)) if kernel == "rows" else list(range(kw, nblk, KS_KW))


def pattern_blocks(pattern, nblk, kernel, kw, depth):
    """the fallback blocks (row-global indices) of `pattern` for the wave `kw` whose steps are `depth` deep"""
    own = own_blocks(nblk, kernel, kw)
    if pattern == "none" or not own:
        return []
    if pattern == "row":
        return list(range(nblk))
    if pattern == "ragged":
        return [nblk - 1]
    n, full = len(own), len(own) // depth
    idx = {"first": [0], "middle": [min(depth // 2, n - 1)] if full else [min(1, n - 1)], "last": [depth - 1] if full else [n - 1],
           "remainder": [full * depth] if full * depth < n else [n - 1],
           "adjacent": [depth - 1, depth] if n > depth else ([0, 1] if n > 1 else [0]),
           "special": [min(1, n - 1)] if n > 1 else [], "special_nan": [min(1, n - 1)] if n > 1 else []}[pattern]
    return sorted({own[i] for i in idx})


def group_of_row(n, epi, kernel):
    """the wave's row group that weight row n belongs to: 4 consecutive rows, the (gate, up) rows of 2 consecutive outputs, or the K-split
    kernel's 2 consecutive rows; and the row's place in it"""
    if kernel == "ksplit":
        return n // 2, n % 2
    if epi == "swiglu":
        j, side = (n // 64) * 32 + n % 32, (n % 64) // 32
        return j // 2, 2 * (j % 2) + side
    return n // 4, n % 4


def special_row(K, blocks, seed, nan):
    """one row of six frequent hi7 classes -- four ordinary ones, 0 (-0 and denormals) and, with `nan`, 127 (NaN payloads of both signs)
    -- whose specials sit in the blocks next to `blocks`, and the eight rare outliers of p12_ref planted in `blocks`: those fall back,
    the blocks with the specials stay packed"""
    g = np.random.default_rng(seed)
    nblk = -(-K // R.BLOCK)
    w = ((g.integers(0, 2, K) << 15) | (g.choice(MAIN_H, K) << 8) | g.integers(0, 256, K)).astype(np.uint16)
    near = sorted({b + d for b in blocks for d in (-1, 1) if 0 <= b + d < nblk and b + d not in blocks}) if blocks else [0]
    spread = [b for b in range(nblk) if b not in blocks]           # the classes are frequent over the row, and dense next to the fallback
    for b in spread:
        lo, hi = b * R.BLOCK, min((b + 1) * R.BLOCK, K)
        step = 3 if b in near else 29
        pos = np.arange(lo + 8, hi, step)
        kinds = np.arange(len(pos)) % (3 if nan else 2)
        w[pos[kinds == 0]] = 0x8000
        w[pos[kinds == 1]] = (1 + g.integers(0, 0x7F, int((kinds == 1).sum()))).astype(np.uint16)
        w[pos[kinds == 2]] = np.where(g.integers(0, 2, int((kinds == 2).sum())) == 1, 0x7FC1, 0xFFC5).astype(np.uint16) + g.integers(0, 50, int((kinds == 2).sum())).astype(np.uint16)
    for k in blocks:
        for i, e in enumerate(R.OUTLIER_E):
            w[k * R.BLOCK + i] = (w[k * R.BLOCK + i] & 0x807F) | np.uint16(e << 7)
    return w


def plantable(w):
    """the first eight elements of every block -- where the outliers go -- moved into the row's most frequent hi7 class, and any class
    that this leaves with fewer than three elements too: planting then takes elements from the most frequent class only, so no ordinary
    class can fall behind an outlier (at most one copy per block, ties to the lower value) and out of the table"""
    w = w.copy()
    N, K = w.shape
    first8 = (np.arange(K) % R.BLOCK) < 8
    for n in range(N):
        h = (w[n] >> 8) & 0x7F
        top = int(np.argmax(np.bincount(h, minlength=128)))
        h[first8] = top
        cnt = np.bincount(h, minlength=128)
        h[cnt[h] < 3] = top
        w[n] = (w[n] & 0x80FF) | (h.astype(np.uint16) << 8)
    return w


class DepthCase:
    """one packed launch against the bf16 launch on the same arguments; `period` distinct rows, repeated down the matrix (the encoder
    works row by row, so the CPU encodes the distinct rows once)"""

    def __init__(self, N, K, epi="none", norm=False, bias=False, res=False, ties=None, seed=0):
        self.N, self.K, self.epi, self.norm, self.bias, self.res, self.ties, self.seed = N, K, epi, norm, bias, res, ties, seed
        self.kernel = "ksplit" if epi == "none" and N <= 8192 else "rows"
        self.depth = 1 if self.kernel == "ksplit" and norm else (ROWS_DEPTH if self.kernel == "rows" else KS_DEPTH)
        self.n_out = N // 2 if epi == "swiglu" else N
        self.pad, self.special = 0, False
        self.id = f"{self.kernel}-{epi}-N{N}-K{K}" + ("-norm" if norm else "") + ("-bias" if bias else "") + ("-res" if res else "") + ("-ties" if ties else "") + f"-s{seed}"

    def plan_of_row(self, n):
        """(pattern, fallback blocks) of weight row n"""
        g, place = group_of_row(n, self.epi, self.kernel)
        size = 2 if self.kernel == "ksplit" else 4
        pat = PATTERNS[(g + self.seed) % len(PATTERNS)]
        variant = (g // len(PATTERNS) + g + self.seed) % (size + 1)          # one row of the group or, last, all of them; every pattern meets every variant
        if variant < size and place != variant:
            pat = "none"
        nblk = -(-self.K // R.BLOCK)
        return pat, pattern_blocks(pat, nblk, self.kernel, g % KS_KW, self.depth)

    @functools.lru_cache(maxsize=None)
    def build(self):
        N, K = self.N, self.K
        size = 2 if self.kernel == "ksplit" else 4
        # (the SwiGLU groups interleave the rows of a 64-row block: the plan repeats after whole blocks)
        self.period = min(N, (64 if self.epi == "swiglu" else size) * len(PATTERNS) * (size + 1))
        P = self.period
        base = plantable(R.designed_bits(P, K, "none", 70 + self.seed))
        plan = [self.plan_of_row(n) for n in range(P)]
        for n, (pat, blocks) in enumerate(plan):
            if pat.startswith("special"):
                base[n] = special_row(K, blocks, 1000 * self.seed + n, pat == "special_nan")
            else:
                for k in blocks:
                    for i, e in enumerate(R.OUTLIER_E):
                        base[n, k * R.BLOCK + i] = (base[n, k * R.BLOCK + i] & 0x807F) | np.uint16(e << 7)
        g = torch.Generator().manual_seed(900 + self.seed)
        self.x = torch.randn((K,), generator=g).to(torch.bfloat16)
        self.x[min(9, K - 1)], self.x[K - 3] = 8.0, -8.0
        reps = -(-N // P)
        assert all(self.plan_of_row(n) == plan[n % P] for n in range(0, N, 7))
        self.w = np.tile(base, (reps, 1))[:N].copy()
        tie_rows = {}
        if self.ties:                                   # two equal rows that beat every other logit: the lower index wins
            x = R.f32_of(R.bits_of(self.x))
            row = R.bits_of(torch.from_numpy(np.sign(x) * 0.25).to(torch.bfloat16))
            for n in self.ties:
                self.w[n] = row
                tie_rows[n] = row
        # the CPU's word on the plan: the encoder's masks and fallback count are the planted ones
        packed, rec, n_fb = R.encode(base)
        want = [sum(1 << k for k in blocks) for _, blocks in plan]
        assert R.masks_of(rec) == want, (self.id, [(n, hex(a), hex(b)) for n, (a, b) in enumerate(zip(R.masks_of(rec), want)) if a != b][:4])
        assert n_fb == sum(len(b) for _, b in plan)
        self.patterns_present = sorted({pat for pat, blocks in plan if blocks or pat == "none"})
        self.packed = np.tile(packed, (reps, 1))[:N].copy()
        self.rec = np.tile(rec, (reps, 1))[:N].copy()
        self.n_fb = sum(len(plan[n % P][1]) for n in range(N))
        for n, row in tie_rows.items():
            tp, tr, tf = R.encode(row[None])
            assert tf == 0
            self.n_fb -= len(plan[n % P][1])
            self.packed[n], self.rec[n] = tp[0], tr[0]
        self.g = (1 + 0.5 * torch.randn((K,), generator=g)).to(torch.bfloat16) if self.norm else None
        self.b = torch.randn((N,), generator=g).to(torch.bfloat16) if self.bias else None
        self.r = torch.randn((N,), generator=g).to(torch.bfloat16) if self.res else None
        return self


ROWS_K = (512, 1024, 1536, 2048, 2560, 3584, 3592, 4104)      # blocks 1, 2, 3, 4, 5, 7 (3 + 3 + 1), ragged behind a remainder of 0 and of 1
# blocks of wave 0: 1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 7 (= 2 KS_DEPTH + 1), 10 (down_proj's row); the last K is ragged (10 blocks, one chunk in the last)
KSPLIT_K = tuple(512 * b for b in (1, 4, 5, 8, 9, 12, 13, 16, 17, 21, 25, 37)) + (512 * 9 + 8,)


def cases():
    out = []
    for i, K in enumerate(ROWS_K):
        out.append(DepthCase(8195, K, bias=i % 2 == 0, res=i % 2 == 1, seed=i))
        out.append(DepthCase(8195, K, epi="argmax", ties=(402 + 4 * i, 7935 - 8 * i), seed=10 + i))
        out.append(DepthCase(128, K, epi="swiglu", norm=i % 2 == 0, seed=20 + i))
    for i, K in enumerate(KSPLIT_K):
        for norm in (False, True):                  # (nine rows are five row groups: two launches, five patterns each)
            for half in (0, 5):
                out.append(DepthCase(9, K, norm=norm, bias=(i + norm) % 2 == 0, res=(i + norm) % 2 == 1, seed=40 + i + half))
    return out


CASES = cases()
