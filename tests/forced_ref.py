"""CPU case builder, float64 reference and fp32 restatement of the forced-turn head (svln_generate_forced): the EPI_TARGET siblings of
gemv_batched_kernel (gemv.hip) and of the 32 x 128 MFMA arg-max epilogue (gemm.hip), and target_final_batched_kernel that merges their
partials.  Test infrastructure, beside tests/scores_ref.py, whose designed operands and log-sum-exp pieces it reuses.

    y_j = fl(l_j * inv_t);  greedy = argmax_j y_j (lowest index on ties);  greedy_logprob = y_greedy - logsumexp_j y_j
    logprob = y_t - logsumexp_j y_j for the NAMED column t of the row (t = -1: NaN, nothing is captured)

Exact inputs.  Logits are designed multiples of 1/2 with |l| <= 35.5 (scores_ref.design_w / design_x: W . x_b is l bit for bit in any
summation order) and inv_t is 1, 1/2 or 2, so y, the captured y_t and y_t - V are exact; what is left to tolerance is log S alone.  The
background sits 20 .. 30 below the row's top: at inv_t = 1/2 that is 10 .. 15 in y, a sum of a few thousand terms of <= 5e-5 beside the
heavy ones, which fp32 carries to ~1e-7 -- the 2e-6 margin of test_forced_inputs.py is what limits the span from below; at inv_t = 2 the
span is 71 * 2 < 150, far from fp32 exp underflow mattering (such terms are 0 in float64 too at 2e-6).

Capture placement.  The MFMA restatement walks the accumulator registers as the kernel does -- tile, wave (64 columns), lane (r32 = lane
& 31 holds columns j * 32 + r32, half = lane >> 5 holds rows acc_row(r, lane) = (r & 3) + 8 (r >> 2) + 4 half), register r < 16, j < 2 -- and
stores into a 32-row array that starts as a canary, so that a store from a pad register, through a tile-local column, from the wrong j or
with the other half's row is a different array.  The GEMV restatement walks units of 4 columns per workgroup (grid min(units, 2048)),
thread b keeping row b.

Mutants: the restatement with one plausible kernel mistake each; tests/test_forced_inputs.py proves that every one moves a log-probability
or a capture slot of some case by >= 100 x the GPU tolerance.
"""
import functools

import numpy as np
import torch

import scores_ref as S

TOL = S.TOL                 # 2e-5: the project's op-level bound for these sums
F = np.float32
NEG = F(-np.inf)
CANARY = 12345.0            # what every capture slot holds before the launch
INV_TS = (1.0, 0.5, 2.0)
MFMA_MUTANTS = ("clamped_pad_row", "tile_local_col", "wrong_j", "half1_takes_half0_target")
GEMV_MUTANTS = ("env0_target",)
SHARED_MUTANTS = ("temp_target_only", "temp_sums_only", "no_log_s", "own_partial_max", "row0_V", "neg1_is_a_column")
MUTANTS = MFMA_MUTANTS + GEMV_MUTANTS + SHARED_MUTANTS


def acc_row(r, lane):
    return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)


# ---------------------------------------------------------------------------------------------------------- reference
def reference(L, tgt, inv_t):
    """float64: (greedy ids [B], greedy log-probabilities [B], target log-probabilities [B] (NaN for -1)) of raw logits L [B][N]"""
    y = L.double() * inv_t
    lse = torch.logsumexp(y, 1)
    tok = torch.tensor([int(torch.nonzero(r == r.max())[0]) for r in y])
    glp = y.gather(1, tok[:, None])[:, 0] - lse
    lp = torch.tensor([float("nan") if t < 0 else float(y[b, t] - lse[b]) for b, t in enumerate(tgt)], dtype=torch.float64)
    return tok, glp, lp


# ---------------------------------------------------------------------------------------------------------- fp32 restatement
def _values(Lrow, inv_t, mut):
    """(summed / compared, captured) fp32 values of one row: y = fl(l * inv_t) for both, but for the two temperature mutants"""
    raw = Lrow.numpy().astype(F)
    y = (raw * F(inv_t)).astype(F)
    return (raw if mut == "temp_target_only" else y), (raw if mut == "temp_sums_only" else y)


def _final(parts, tv, t, own_m, mut, V0=None):
    """target_final_batched_kernel on one row: parts [(m, s, index)], tv the captured value (the canary when nothing was captured), t the
    target, own_m the maximum of the partial that owns column t -> (greedy id, greedy logprob, target logprob), fp32 arithmetic"""
    V, _, I = S._merge(parts, None)
    Vn = V0 if mut == "row0_V" and V0 is not None else V
    mine = [F(0)] * 256
    for k, (m, s, _) in enumerate(parts):
        mine[k % 256] = F(mine[k % 256] + S._rescale(s, m, Vn))
    w = 128
    while w:
        for q in range(w):
            mine[q] = F(mine[q] + mine[q + w])
        w //= 2
    tok = -1 if I == 0x7FFFFFFF else I
    glp = F(-np.log(mine[0], dtype=F))
    if tok < 0:
        return tok, float("nan"), float("nan")
    if t < 0 and mut != "neg1_is_a_column":
        return tok, float(glp), float("nan")
    # (row0_V: the sum loop rescales to row 0's maximum while the difference takes the row's own -- a consistent shift of both would cancel)
    base = own_m if mut == "own_partial_max" and t >= 0 else V
    d = F(F(tv) - base)
    return tok, float(glp), float(d if mut == "no_log_s" else -F(F(-glp) - d))       # (with d == 0 this is glp to the sign of a zero)


def restate_gemv(L, tgt, inv_t, mut=None):
    """gemv_batched_kernel<T, EPI_TARGET, false, B> + target_final_batched_kernel on L [B][N] -> ([(greedy, glp, lp)] per row, slots [32])"""
    B, N = L.shape
    units = (N + 3) // 4
    grid = min(units, 2048)
    slots = np.full(32, CANARY, dtype=F)
    out, V0 = [], None
    with np.errstate(all="ignore"):
        for b in range(B):
            sum_, cap_ = _values(L[b], inv_t, mut)
            tg = tgt[0] if mut == "env0_target" else tgt[b]
            parts, own_m = [], NEG
            for k in range(grid):
                m, s, best, bi, mine = NEG, F(0), NEG, 0x7FFFFFFF, False
                for u in range(k, units, grid):
                    for r in range(4):
                        n = 4 * u + r
                        if n >= N:
                            continue
                        if n == tg:
                            slots[b] = cap_[n]
                            mine = True
                        if sum_[n] > best:
                            best, bi = sum_[n], n
                        m, s = S._add(sum_[n], m, s, None)
                parts.append((m, s, bi))
                if mine:
                    own_m = m
            if b == 0:
                V0 = S._merge(parts, None)[0]
            out.append(_final(parts, slots[b], tgt[b], own_m, mut, V0))
    return out, slots


def restate_mfma(L, tgt, inv_t, mut=None):
    """the EPI_TARGET epilogue of the 32 x 128 tiles + target_final_batched_kernel on L [M][N] -> ([(greedy, glp, lp)] per row, slots [32])"""
    M, N = L.shape
    tiles = (N + 127) // 128
    slots = np.full(32, CANARY, dtype=F)
    vals = [_values(L[b], inv_t, mut) for b in range(M)]
    own = [NEG] * M
    all_parts = []
    with np.errstate(all="ignore"):
        # the capture, register by register
        for t in range(tiles):
            for w in range(2):
                for lane in range(64):
                    r32 = lane & 31
                    for r in range(16):
                        m_own = acc_row(r, lane)
                        m = min(m_own, M - 1)                              # the clamp that serves the loads (pad registers hold row M - 1's logits)
                        if mut == "clamped_pad_row":
                            tg = tgt[m]
                        elif mut == "half1_takes_half0_target":
                            tg = tgt[acc_row(r, 0)] if acc_row(r, 0) < M and m_own < M else -1
                        else:
                            tg = tgt[m_own] if m_own < M else -1
                        for j in range(2):
                            nn = t * 128 + w * 64 + j * 32 + r32
                            col = nn - t * 128 if mut == "tile_local_col" else nn
                            if nn < N and col == tg:
                                src = t * 128 + w * 64 + (1 - j) * 32 + r32 if mut == "wrong_j" else nn
                                slots[m_own] = vals[m][1][src] if src < N else F(0)        # (a column beyond N holds the product with no weight row: 0)
        # the partials, as scores_ref.restate_mfma without a penalty
        for b in range(M):
            sum_ = vals[b][0]
            parts = []
            for t in range(tiles):
                waves = []
                for w in range(2):
                    v, vi = NEG, 0x7FFFFFFF
                    for r in range(32):
                        for j in range(2):
                            n = t * 128 + w * 64 + j * 32 + r
                            if n < N and (sum_[n] > v or (sum_[n] == v and n < vi)):
                                v, vi = sum_[n], n
                    lane = []
                    for r in range(32):
                        a = F(0)
                        for j in range(2):
                            n = t * 128 + w * 64 + j * 32 + r
                            if n < N:
                                a = F(a + (F(0) if sum_[n] == NEG else S._exp(sum_[n] - v)))
                        lane.append(a)
                    o = 1
                    while o < 32:
                        lane = [F(lane[r] + lane[r ^ o]) for r in range(32)]
                        o *= 2
                    waves.append((v, lane[0], vi))
                parts.append(S._merge(waves, None))
                if 0 <= tgt[b] < N and tgt[b] // 128 == t:
                    own[b] = parts[-1][0]
            all_parts.append(parts)
        V0 = S._merge(all_parts[0], None)[0]
        out = [_final(all_parts[b], slots[b], tgt[b], own[b], mut, V0) for b in range(M)]
    return out, slots


# ---------------------------------------------------------------------------------------------------------- cases
def mfma_places(N):
    """the named columns of an MFMA case: 0, N - 1, 127 / 128, and in every wave's 64-column range its first and last column, both j
    (offsets 0 .. 31 and 32 .. 63) at r32 = 0 and 31"""
    cols = {0, N - 1, 127, 128}
    for w0 in range(0, N, 64):
        cols |= {w0, w0 + 31, w0 + 32, w0 + 63}
    return sorted(c for c in cols if 0 <= c < N)


def gemv_places(N):
    """the named columns of a GEMV case: every r of a unit (the first and a middle one), the ragged last unit, and -- where the grid
    strides (more than 2048 units) -- every r of the second unit workgroup 0 visits"""
    u_mid = ((N + 3) // 4) // 2
    cols = {0, 1, 2, 3, N - 1, 4 * ((N - 1) // 4)} | {4 * u_mid + r for r in range(4)}
    if (N + 3) // 4 > 2048:
        cols |= {4 * 2048 + r for r in range(4)}
    return sorted(c for c in cols if 0 <= c < N)


class Case:
    """kind "gemv" (B = 2, 4, 8 rows) or "mfma" (M rows passed to the kernel, the first `live` of them with a target; M = 4, live = 3 is
    the engine's padding of n = 3).  L [M][N] designed raw logits, tgt [M] (-1: none), inv_t."""

    def __init__(self, kind, M, N, K, inv_t=1.0, fmt="plain-fp32", live=None, shift=0, seed=0):
        self.kind, self.B, self.N, self.K, self.inv_t, self.fmt, self.shift, self.seed = kind, M, N, K, inv_t, fmt, shift, seed
        self.live = M if live is None else live
        self.id = f"{kind}-{fmt}-M{M}" + (f"of{self.live}" if self.live != M else "") + f"-N{N}-K{K}-it{inv_t:g}-s{shift}"

    @property
    def dtype(self):
        return S.G.DTYPE[self.fmt]

    def tops(self):
        return [(12.0 - 0.5 * ((b // 2) % 8)) if b % 2 == 0 else (-1.0 - ((b // 2) % 4)) for b in range(self.B)]

    @functools.lru_cache(maxsize=None)
    def logits(self):
        """(L [M][N], tgt [M]): row b's top at a column spread over the tiles, a runner-up one below it, and its target -- one of the named
        places, rotated by row and by the case's shift -- at top - 3 - (b % 4) unless it falls on the top (rows b % 5 == 2 aim at it on
        purpose: target == arg-max) ; one live row of every case with >= 4 live rows names no column (-1)"""
        B, N = self.B, self.N
        tops = self.tops()
        L = S.background(B, N, tops, self.seed)
        places = mfma_places(N) if self.kind == "mfma" else gemv_places(N)
        tgt = []
        for b in range(B):
            top_col = (37 * b + 11 + 64 * b) % N
            up_col = (top_col + 5) % N
            L[b, top_col] = tops[b]
            if up_col != top_col:
                L[b, up_col] = tops[b] - 1
            if b >= self.live or (self.live >= 4 and b == (self.shift + 1) % self.live):
                tgt.append(-1)
                continue
            t = top_col if b % 5 == 2 else places[(b + self.shift) % len(places)]
            if t not in (top_col, up_col):
                L[b, t] = tops[b] - 3 - (b % 4)
            tgt.append(int(t))
        return L, tgt

    def reference(self):
        L, tgt = self.logits()
        return reference(L, tgt, self.inv_t)

    def restate(self, mut=None):
        L, tgt = self.logits()
        return (restate_gemv if self.kind == "gemv" else restate_mfma)(L, tgt, self.inv_t, mut)

    def expected_slots(self):
        """the capture array after a correct launch: y_t in the rows that name a column, the canary everywhere else"""
        L, tgt = self.logits()
        s = np.full(32, CANARY, dtype=F)
        for b, t in enumerate(tgt):
            if t >= 0:
                s[b] = F(F(float(L[b, t])) * F(self.inv_t))
        return s

    def operands(self):
        """(x [M][K] float64, W [N][K] exact values in fp32 / bf16)"""
        L, _ = self.logits()
        return S.design_x(self.B, self.K, self.seed), S.design_w(L, self.K, self.seed, torch.float32 if self.fmt == "plain-fp32" else torch.bfloat16)


MFMA_N = (127, 128, 129, 257, 391)


def mfma_cases():
    out = []
    for d, fmt in enumerate(("plain-fp32", "plain-bf16")):
        # (3, 3): the kernel launched with M = 3 itself; (4, 3): the engine's padding of n = 3 to four rows, the last with target -1
        for i, (M, live) in enumerate(((3, 3), (4, 3), (4, 4), (5, 5), (8, 8), (17, 17), (32, 32))):
            for j, N in enumerate(MFMA_N):
                # every (M, N) at the temperature the walk assigns it; the places rotate with the shift
                out.append(Case("mfma", M, N, 576 if (i + j + d) % 2 else 1024, inv_t=INV_TS[(i + j) % 3], fmt=fmt, live=live, shift=3 * i + 5 * j,
                                seed=300 + 10 * i + j))
        for k, it in enumerate(INV_TS):      # one shape at every temperature, more shifts: every named place is some row's target
            for sh in range(0, 24, 4):
                out.append(Case("mfma", 8, 391, 576, inv_t=it, fmt=fmt, shift=sh + k, seed=390 + sh + k))
    return out


GEMV_N = (5, 6, 7, 8, 8196, 8197, 8198, 8199)


def gemv_cases():
    out = []
    for d, fmt in enumerate(("plain-fp32", "plain-bf16")):
        for i, B in enumerate((2, 4, 8)):
            for j, N in enumerate(GEMV_N):
                for sh in (0, 6):
                    out.append(Case("gemv", B, N, 192 if (i + j) % 2 else 512, inv_t=INV_TS[(i + j + sh) % 3], fmt=fmt, shift=sh + i, seed=500 + 10 * i + j + sh))
    return out


def cpu_cases():
    """the cases the CPU proof walks: every shape, without the repeats that only cost Python-loop time (the stride sizes at B = 2 only)"""
    mf = [c for c in mfma_cases() if c.fmt == "plain-fp32"]
    gv = [c for c in gemv_cases() if c.fmt == "plain-fp32" and (c.N < 8196 or c.B == 2)]
    return mf + gv


KIND_MUTANTS = {"mfma": MFMA_MUTANTS + SHARED_MUTANTS, "gemv": GEMV_MUTANTS + SHARED_MUTANTS}
