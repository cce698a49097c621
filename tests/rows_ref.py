"""CPU case builder, float64 / exact-integer references, derived bounds and "mutant" references (plausible kernel mistakes) of the
bandwidth-bound row helpers of streamvln_amd/csrc/misc.hip: the norms (rmsnorm_kernel with its hidden tap and skip word,
rmsnorm_indexed_kernel, layernorm_kernel), the gathers (gather_rows_kernel, gather_rows_ragged_kernel), frame_hash_kernel, the memory
prune (mem_*_kernel), pool_kernel and patchify_kernel.  Test infrastructure, modelled on tests/gemv_ref.py.

Exact families (compared bit for bit): gathers, taps, patchify, the frame hash, the prune selection.
Toleranced families: the norms, the prune scores, pool.  Their bounds are DERIVED here from the kernels' own operation order; nothing in
them is fitted to what the GPU returns.  u = 2^-24 is the unit roundoff of fp32, hu(v) half an ulp of v in the engine type.

  One wave owns a row; lane l takes the 16-byte chunks l, l + 64, ... (EPC = 8 bf16 / 4 fp32 values each), so a lane adds
  m = ceil(nch / 64) * EPC terms one after the other, and the butterfly wave_sum adds 6 more levels: a sum of S terms t_i carries at most
  (m + 5) u sum|t_i| of rounding error, plus u |t_i| for each product that forms a term.  The hardware reciprocal square root is good to
  one ulp = 2 u.

  RMSNorm   ss = sum x^2: relative error (m + 6) u; / n and + eps: 2 u more; sc = rsqrt(.): half of that plus 2 u; x * sc and g * (.): 2 u.
            |y - ref| <= |ref| * (0.5 (m + 8) + 4) u + hu(ref)
  LayerNorm mu = sum x / n: |mu - ref| <= dmu = (m + 6) u mean|x|.  d = x - mu: dmu + u |d|.  v = sum d^2: relative (m + 9) u, plus
            dmu^2 / var for the shifted mean (sum d = 0 about the true mean, so the shift enters squared); / n, + eps: 2 u;
            dsc = 0.5 ((m + 11) u + dmu^2 / var) + 2 u.  d * sc * g: 2 u; + b: u of the result.
            |y - ref| <= |g| sc dmu + |g d sc| (dsc + 3 u) + u |ref| + hu(ref)
  Pool      r = wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d), weights exact fp32 values: at most 4 roundings on every path, so a correct
            fp32 evaluation errs by up to 4 u S, S = wy0 (wx0 |a| + wx1 |b|) + wy1 (wx0 |c| + wx1 |d|) -- and with four terms it comes
            close to that.  The bound doubles it, so that a correct evaluation in ANY association stays within half the bound:
            |r - ref| <= 8 u S + hu(ref)
  Prune     mean_c = (blocks of 64 rows summed in order, then the nb block sums in order) / N:
            |mean_c - ref| <= L u a_c, a_c = mean_r |M_rc|, L = min(N, 64) + nb + 1.
            score = dot / max(sqrt(nn) sqrt(mm), 1e-20), the three sums by fmaf over m terms and the wave tree; with D = |f| |mu|:
            |score - ref| <= u [ (m + 7) sum|f mu| / D + L sum|f| a / D + ((m + 11) + L |a| / |mu|) |ref| ]
            (dot's own rounding; the mean's error through dot; the two norms, their roots, the product and the division; the mean's
            error through |mu|).  The score is stored as fp32 in both engines.

Mutants that cannot be seen, with the reason (tests/test_rows_inputs.py proves each):
  * prune "mean divided by N rounded up to 64": the cosine does not change when the mean is scaled, EXCEPT through the clamp of the
    denominator; the `clamp-edge` case puts sqrt(nn) sqrt(mm) just above 1e-20 so that the smaller mean falls below it.
  * pool "border tap not clamped": the 27 -> 14 geometry of every configuration never produces a tap at the border (the largest source
    coordinate is 25.54), so the clamp is dead code for the shapes the engine can run; the test asserts that instead.
  * LayerNorm "variance in one pass" on the bf16 engine at n <= 1024.  The bf16 offset rows are 256 everywhere with one entry per row at
    258 (one bf16 ulp away: var / mean^2 ~ 2^-14 / n).  At n = 1152 and 3584 the fp32 sum of squares (multiples of 4 near n 2^16) leaves
    the exact range 2^26 and E[x^2] - mu^2 is far off; up to n = 520 every partial sum is an exact integer and the mutant differs only by
    the single roundings of E[x^2], mu and mu^2, whose size is the luck of the row (seen at some widths, not at others): not listed there.
    The fp32 engine's offset rows (mean 256, spread 2^-4) see it at every width.
  * LayerNorm "unbiased variance" on the offset rows: there the bound is the error of the mean itself, far above 1 / (2 n).
"""
import math

import numpy as np
import torch

from oracle import streamvln_oracle as O

U = 2.0 ** -24
EPS = 1e-6
RATIO = 10.0
DTYPES = (torch.float32, torch.bfloat16)
EPC = {torch.float32: 4, torch.bfloat16: 8}
PREC = {torch.float32: 24, torch.bfloat16: 8}              # significant bits
NAME = {torch.float32: "fp32", torch.bfloat16: "bf16"}
HIDDEN, VOCAB = 512, 4096                                   # TINY


def rt(a, dtype):
    """float64 array rounded to the engine type, as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).double().numpy()


def to_t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype)


def half_ulp(v, dtype):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - PREC[dtype])


def bits(t):
    """stored bits of a tensor of an engine type"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def lanes_m(n, dtype):
    """terms one lane adds in a row sum over n values"""
    nch = n // EPC[dtype]
    return -(-nch // 64) * EPC[dtype]


# ---------------------------------------------------------------------------------------------------------- fp32 in the kernel's order
def wave_tree(acc):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ o]
    return acc[:, 0]


def lane_sum32(t, epc):
    """fp32 sum of the terms t [rows][n] the way a wave forms it: lane l adds its chunks l, l + 64, ... element by element, then the
    butterfly tree (missing chunks add an exact 0)"""
    assert t.dtype == np.float32
    rows, n = t.shape
    sweeps = -(-(n // epc) // 64)
    pad = np.zeros((rows, sweeps * 64 * epc), dtype=np.float32)
    pad[:, :n] = t
    v = pad.reshape(rows, sweeps, 64, epc)
    acc = np.zeros((rows, 64), dtype=np.float32)
    for s in range(sweeps):
        for e in range(epc):
            acc = acc + v[:, s, :, e]
    return wave_tree(acc)


# ---------------------------------------------------------------------------------------------------------- norms
WIDTHS = (144, 512, 520, 1152, 3584)
ROWS = (1, 4, 5, 7)
NORM_FAMILIES = ("last", "chunk64", "lane63", "eps", "offset")


def _gain(n, dtype, seed):
    """gains and biases of magnitude 0.5 .. 2 / 0 .. 1 whose sign pattern is not symmetric under reversal (asserted by the CPU test)"""
    g = np.random.default_rng(seed)
    gain = (0.5 + 1.5 * g.random(n)) * np.where(g.random(n) < 0.4, -1.0, 1.0)
    bias = g.random(n) * np.where(g.random(n) < 0.6, -1.0, 1.0)
    return rt(gain, dtype), rt(bias, dtype)


class NormCase:
    """rows x n values through svln_op_rmsnorm (op "rms") or svln_op_layernorm ("ln").
    family  last / chunk64 / lane63: |x| <= 1/8 everywhere except the last chunk / chunk 64 / lane 63's chunks, which hold |x| in 2 .. 4;
            eps: |x| ~ 1e-3 (mean square ~ eps);  offset (ln): a large common offset (fp32: 256 + 2^-4 [-1, 1]; bf16: 256, one entry per
            row at 258)"""

    def __init__(self, op, dtype, n, rows, family, seed):
        self.op, self.dtype, self.n, self.rows, self.family, self.seed = op, dtype, n, rows, family, seed
        self.epc = EPC[dtype]
        self.nch = n // self.epc
        self.id = f"{op}-{NAME[dtype]}-n{n}-r{rows}-{family}"
        self._built = False

    @staticmethod
    def exists(op, dtype, n, family):
        nch = n // EPC[dtype]
        return {"last": True, "chunk64": nch > 64, "lane63": nch >= 64, "eps": True, "offset": op == "ln"}[family]

    def hot_chunks(self):
        return {"last": [self.nch - 1], "chunk64": [64], "lane63": list(range(63, self.nch, 64))}.get(self.family, [])

    def build(self):
        if self._built:
            return self
        self._built = True
        g = np.random.default_rng(9000 + self.seed)
        rows, n, epc = self.rows, self.n, self.epc
        sign = lambda shape: np.where(g.random(shape) < 0.5, -1.0, 1.0)
        if self.family == "eps":
            x = 1e-3 * (0.5 + g.random((rows, n))) * sign((rows, n))
        elif self.family == "offset":
            if self.dtype == torch.float32:
                x = 256.0 + 2.0 ** -4 * (2 * g.random((rows, n)) - 1)
            else:                                                    # bf16: 256 everywhere, ONE entry per row a bf16 ulp above it
                x = np.full((rows, n), 256.0)
                x[np.arange(rows), g.integers(0, n, rows)] = 258.0
        else:
            x = 0.125 * (2 * g.random((rows, n)) - 1)
            for ci in self.hot_chunks():
                x[:, ci * epc:(ci + 1) * epc] = (2 + 2 * g.random((rows, epc))) * sign((rows, epc))
        self.x = rt(x, self.dtype)
        self.g, self.b = _gain(n, self.dtype, 77 + n)
        self.cancel = None
        if self.op == "ln" and self.family != "offset":
            # one constructed column where (x - mu) sc g and b cancel in row 0 up to b's own rounding: the output there is tiny, so is its
            # ulp, and a relative change of sc (the unbiased variance: 1 / 2n) shows against the fp32 terms of the bound alone.  The
            # column of row 0's largest |x - mu|, where the error of the mean weighs least.
            d = self.x[0] - self.x[0].mean()
            want = -self.g * d / math.sqrt((d * d).mean() + EPS)
            top = np.argsort(-np.abs(d))[:16]                        # ... and among the 16 largest, where b's rounding leaves the least
            c0 = int(top[np.argmin(np.abs(rt(want[top], self.dtype) - want[top]) / np.abs(want[top]))])
            self.b = self.b.copy()
            self.b[c0] = float(rt(want[c0:c0 + 1], self.dtype)[0])
            self.cancel = c0
        return self

    def mutants(self):
        m = ["gain_shifted"]
        if self.op == "ln":
            m.append("bias_dropped")
            if self.family != "offset":        # (offset rows: the bound is the mean's own error, far above 1 / 2n.  Elsewhere the bf16 engine
                m.append("unbiased_var")       # sees it too, on the column build() makes (x - mu) sc g and b cancel in: a tiny output, a tiny ulp)
        if self.n % (64 * self.epc):
            m.append("divisor_rounded")
        if self.family == "last":
            m.append("drop_last_chunk")
        if (self.family == "last" and self.nch > 64) or self.family == "chunk64" or (self.family == "lane63" and self.nch >= 128):
            m.append("drop_past_first_sweep")
        if self.family == "lane63":
            m.append("lane63_skipped")
        if self.family == "eps":
            m += ["eps_dropped", "eps_outside_root"]
        if self.family == "offset" and (self.dtype == torch.float32 or self.n * 2 ** 16 > 2 ** 26):
            m.append("one_pass_var")       # (bf16: where sum x^2, multiples of 4 near n 2^16, leaves the exact range of fp32; module docstring)
        return m

    def reference(self, mutant=None):
        """float64 [rows][n]"""
        self.build()
        x, g, b, n, epc = self.x, self.g, self.b, self.n, self.epc
        keep = np.ones(self.nch, dtype=bool)
        if mutant == "drop_last_chunk":
            keep[-1] = False
        elif mutant == "drop_past_first_sweep":
            keep[64:] = False
        elif mutant == "lane63_skipped":
            keep[63::64] = False
        w = np.repeat(keep, epc).astype(np.float64)[None]
        div = float(-(-n // (64 * epc)) * 64 * epc) if mutant == "divisor_rounded" else float(n)
        if mutant == "gain_shifted":
            g = np.roll(g, -epc)                                     # column c takes the gain of column c + EPC
        root = lambda ms: 1 / np.sqrt(ms) if mutant == "eps_dropped" else 1 / (np.sqrt(ms) + EPS) if mutant == "eps_outside_root" else 1 / np.sqrt(ms + EPS)
        with np.errstate(all="ignore"):
            if self.op == "rms":
                sc = root((x * x * w).sum(1) / div)
                return g[None] * (x * sc[:, None])
            mu = (x * w).sum(1) / div
            d = x - mu[:, None]
            if mutant == "one_pass_var":                             # E[x^2] - mu^2, formed in fp32 the way the kernel would
                x32 = x.astype(np.float32)
                mu32 = lane_sum32(x32, epc) / np.float32(n)
                var = (lane_sum32(x32 * x32, epc) / np.float32(n) - mu32 * mu32).astype(np.float64)
            else:
                var = (d * d * w).sum(1) / (div - 1 if mutant == "unbiased_var" else div)
            sc = root(var)
            return d * sc[:, None] * g[None] + (0.0 if mutant == "bias_dropped" else b[None])

    def bound(self):
        """the derived bound [rows][n] (module docstring)"""
        ref = self.reference()
        m = lanes_m(self.n, self.dtype)
        if self.op == "rms":
            return np.abs(ref) * (0.5 * (m + 8) + 4) * U + half_ulp(ref, self.dtype)
        x, g = self.x, self.g
        mu = x.mean(1, keepdims=True)
        d = x - mu
        var = (d * d).mean(1, keepdims=True)
        sc = 1 / np.sqrt(var + EPS)
        dmu = (m + 6) * U * np.abs(x).mean(1, keepdims=True)
        dsc = 0.5 * ((m + 11) * U + dmu * dmu / var) + 2 * U
        return np.abs(g)[None] * sc * dmu + np.abs(g[None] * d * sc) * (dsc + 3 * U) + U * np.abs(ref) + half_ulp(ref, self.dtype)

    def kernel_order(self):
        """plain fp32 restatement in the kernel's order, BEFORE the rounding to the engine type, as float64"""
        self.build()
        f = np.float32
        x, g, b, n = self.x.astype(f), self.g.astype(f), self.b.astype(f), f(self.n)
        if self.op == "rms":
            sc = f(1) / np.sqrt(lane_sum32(x * x, self.epc) / n + f(EPS))
            return (g[None] * (x * sc[:, None])).astype(np.float64)
        mu = lane_sum32(x, self.epc) / n
        d = x - mu[:, None]
        sc = f(1) / np.sqrt(lane_sum32(d * d, self.epc) / n + f(EPS))
        return (d * sc[:, None] * g[None] + b[None]).astype(np.float64)


def norm_cases():
    out, i = [], 0
    for dtype in DTYPES:
        for op in ("rms", "ln"):
            for n in WIDTHS:
                for fam in NORM_FAMILIES:
                    if NormCase.exists(op, dtype, n, fam):
                        out.append(NormCase(op, dtype, n, ROWS[i % 4], fam, i))
                        i += 1
    return out


NORM_CASES = norm_cases()


def toleranced_report(ref, bound, mutant_outputs):
    """{mutant: max |mutant - ref| / bound}; a non-finite mutant output counts as infinitely far"""
    out = {}
    for k, mut in mutant_outputs.items():
        with np.errstate(all="ignore"):
            r = np.abs(mut - ref) / bound
        out[k] = float("inf") if not np.isfinite(mut).all() else float(r.max())
    return out


# ---------------------------------------------------------------------------------------------------------- tap and indexed norm
class TapCase:
    """svln_op_rmsnorm_tap: rows rows; the tap holds y2_cap rows between two canary rows.  The expectation is a MAP: tap row t (0 ..
    y2_cap, the last being the canary after the buffer) <- row of y, or -1 = untouched; y itself is written unless skip."""

    def __init__(self, dtype, n, rows, y2_row, y2_cap, skip=0):
        self.dtype, self.n, self.rows, self.y2_row, self.y2_cap, self.skip = dtype, n, rows, y2_row, y2_cap, skip
        self.id = f"tap-{NAME[dtype]}-n{n}-r{rows}-row{y2_row}of{y2_cap}" + ("-skip" if skip else "")
        assert rows == 1 or y2_row + rows <= y2_cap, "several rows clamped to one tap row would race"

    def mutants(self):
        m = ["skip_ignored"] if self.skip else []
        if not self.skip and self.y2_row > 0:
            m.append("no_offset")
        if not self.skip and self.y2_row + self.rows > self.y2_cap:
            m.append("clamp_to_cap")
        return m

    def maps(self, mutant=None):
        """(y written?, tap map [y2_cap + 1])"""
        tap = [-1] * (self.y2_cap + 1)
        if self.skip and mutant != "skip_ignored":
            return False, tap
        for r in range(self.rows):
            t = r if mutant == "no_offset" else self.y2_row + r
            tap[min(t, self.y2_cap if mutant == "clamp_to_cap" else self.y2_cap - 1)] = r
        return True, tap


class IndexedCase:
    """svln_op_rmsnorm_indexed: y[r] = norm(x[src[r]]), tap[tap_rows[r]] = y[r] unless -1.  maps(): (source row of every y row, tap map)"""

    def __init__(self, dtype, n, x_rows, src, tap_rows, tap_cap):
        self.dtype, self.n, self.x_rows, self.src, self.tap_rows, self.tap_cap = dtype, n, x_rows, list(src), list(tap_rows), tap_cap
        self.rows = len(self.src)
        self.id = f"indexed-{NAME[dtype]}-n{n}-r{self.rows}"
        live = [t for t in self.tap_rows if t >= 0]
        assert len(live) == len(set(live)), "two rows into one tap row would race"

    def mutants(self):
        return ["src_ignored"] + (["tap_gt0"] if 0 in self.tap_rows else [])

    def maps(self, mutant=None):
        ymap = [r if mutant == "src_ignored" else s for r, s in enumerate(self.src)]
        tap = [-1] * self.tap_cap
        for r, t in enumerate(self.tap_rows):
            if (t > 0) if mutant == "tap_gt0" else (t >= 0):
                tap[t] = r
        return ymap, tap


def tap_cases():
    out = []
    for dtype in DTYPES:
        for i, n in enumerate(WIDTHS):
            cap = 6
            out += [TapCase(dtype, n, 1, 0, cap), TapCase(dtype, n, 1, cap - 1, cap), TapCase(dtype, n, 1, cap + 3, cap),
                    TapCase(dtype, n, 1, 2, cap, skip=1), TapCase(dtype, n, ROWS[1 + i % 3], 0, 8), TapCase(dtype, n, ROWS[1 + (i + 1) % 3], 1, 8)]
    return out


def indexed_cases():
    out = []
    for dtype in DTYPES:
        for n in WIDTHS:
            out.append(IndexedCase(dtype, n, 7, [6], [0], 5))
            out.append(IndexedCase(dtype, n, 7, [3, 0, 3, 6], [-1, 0, 4, -1], 5))
            out.append(IndexedCase(dtype, n, 7, [2, 2, 0, 5, 1], [4, -1, 0, -1, 2], 5))
            out.append(IndexedCase(dtype, n, 7, [6, 4, 4, 0, 1, 3, 5], [-1, 4, -1, 0, -1, 1, -1], 5))
    return out


TAP_CASES, INDEXED_CASES = tap_cases(), indexed_cases()


def tap_input(dtype, n, rows=7):
    """the rows the tap / indexed cases normalise: distinct rows of the `last` family"""
    return NormCase("rms", dtype, n, rows, "last", 4000 + n).build()


# ---------------------------------------------------------------------------------------------------------- gathers
FEAT_ROWS, GATHER_N = 392, HIDDEN
SENTINEL = -999.0


def tables(dtype):
    """embed [VOCAB][n] of integers, feats [FEAT_ROWS][n] of half-integers: values of both engine types, no row equal to another"""
    g = np.random.default_rng(31)
    embed = g.integers(-128, 128, (VOCAB, GATHER_N)).astype(np.float64)
    feats = g.integers(-127, 127, (FEAT_ROWS, GATHER_N)) + 0.5
    assert (rt(embed, dtype) == embed).all() and (rt(feats, dtype) == feats).all()
    return embed, feats


class GatherCase:
    def __init__(self, dtype, src, skip=0, tag=""):
        self.dtype, self.src, self.skip = dtype, np.asarray(src, dtype=np.int32), skip
        self.rows = len(self.src)
        self.id = f"gather-{NAME[dtype]}-r{self.rows}{tag}" + ("-skip" if skip else "")

    def mutants(self):
        if self.skip:
            return ["skip_ignored"]
        return (["neg_without_plus1"] if (self.src < 0).any() else []) + (["zero_to_feats"] if (self.src == 0).any() else [])

    def reference(self, embed, feats, mutant=None):
        """[rows][n] float64, or None = out untouched.  A row the mutant would fetch from outside a table reads SENTINEL."""
        if self.skip and mutant != "skip_ignored":
            return None
        bad = np.full((1, GATHER_N), SENTINEL)
        fe = np.concatenate([feats, bad, bad])                    # [FEAT_ROWS] = one past the end, [FEAT_ROWS + 1] stands for row -1
        out = np.empty((self.rows, GATHER_N))
        for r, s in enumerate(self.src.tolist()):
            if mutant == "zero_to_feats" and s == 0:
                out[r] = fe[FEAT_ROWS + 1]
            elif s >= 0:
                out[r] = embed[s]
            else:
                out[r] = fe[-s if mutant == "neg_without_plus1" else -(s + 1)]
        return out


class RaggedCase:
    OUT_ROWS = 40

    def __init__(self, dtype, pairs):
        self.dtype, self.pairs = dtype, list(pairs)
        self.rows = len(self.pairs)
        self.id = f"ragged-{NAME[dtype]}-r{self.rows}"

    def mutants(self):
        return ["pair_swapped"]

    def reference(self, embed, mutant=None):
        """{row of out: source row of embed}; rows not named stay untouched"""
        return {(t if mutant == "pair_swapped" else d): (d if mutant == "pair_swapped" else t) for d, t in self.pairs}


def gather_cases():
    out = []
    g = np.random.default_rng(5)
    for dtype in DTYPES:
        out.append(GatherCase(dtype, [0], tag="-zero"))
        out.append(GatherCase(dtype, [-FEAT_ROWS], tag="-lastfeat"))
        edge = [0, VOCAB - 1, -1, -FEAT_ROWS]
        src = np.concatenate([edge, g.integers(-FEAT_ROWS, VOCAB, 300 - 2 * len(edge)), edge[::-1]])
        out.append(GatherCase(dtype, src))
        out.append(GatherCase(dtype, src, skip=1))
    return out


def ragged_cases():
    pairs = [(17, 0), (3, VOCAB - 1), (30, 77), (4, 2048), (39, 1), (0, 4094), (22, 3)]
    return [RaggedCase(dtype, p) for dtype in DTYPES for p in (pairs[:1], pairs)]


GATHER_CASES, RAGGED_CASES = gather_cases(), ragged_cases()


# ---------------------------------------------------------------------------------------------------------- frame hash
_C1, _C2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)                 # common.h: splitmix64
_KA, _KM, _KB = np.uint64(0x243F6A8885A308D3), np.uint64(0x9E3779B97F4A7C15), np.uint64(0x13198A2E03707344)   # misc.hip: frame_hash_kernel
ENGINE_WORDS = 3 * 384 * 384
HASH_WORDS = (ENGINE_WORDS, 2 * 16384 + 5, 100)
HASH_FRAMES = (1, 9)


def splitmix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _C1
        z = (z ^ (z >> np.uint64(27))) * _C2
        return z ^ (z >> np.uint64(31))


def hash_words(F, words, seed=0):
    """[F][words] uint32: random words; every frame differs"""
    return np.random.default_rng(600 + seed).integers(0, 2 ** 32, (F, words), dtype=np.uint64).astype(np.uint32)


def hash_mutants(F, words):
    return ["index_left_out", "one_half_only"] + (["index_16_bits"] if words > 65536 else []) + (["frame_offset_short"] if F > 1 else [])


def frame_keys(pix, mutant=None):
    """exact keys [F][2] uint64 of pix [F][words] uint32: two sums mod 2^64 over splitmix64 of (word | index << 32)"""
    F, words = pix.shape
    flat = pix.reshape(-1)
    i = np.arange(words, dtype=np.uint64)
    if mutant == "index_left_out":
        i = i * np.uint64(0)
    elif mutant == "index_16_bits":
        i = i & np.uint64(0xFFFF)
    out = np.zeros((F, 2), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for f in range(F):
            off = f * (words - 1) if mutant == "frame_offset_short" else f * words
            v = flat[off:off + words].astype(np.uint64) | (i << np.uint64(32))
            out[f, 0] = splitmix64(v ^ _KA).sum(dtype=np.uint64)
            out[f, 1] = out[f, 0] if mutant == "one_half_only" else splitmix64(v * _KM + _KB).sum(dtype=np.uint64)
    return out


# ---------------------------------------------------------------------------------------------------------- memory prune
PRUNE_N = (1, 64, 65, 1024, 1025, 1568)
EDGES = (1024, 1023, 1088, 1087, 64, 63, 0)


class PruneCase:
    """svln_op_memory_prune on N rows of HIDDEN values.
    kind  graded     row i = c + beta_i w_i: beta in 2 .. 3 for the rows meant to survive (both sides of 63|64, 1023|1024, 1087|1088 and the
                     last row first, then random ones), 0.3 .. 0.6 for the rest, and ONE pair of bit-identical rows (beta 1.2, rows 1
                     and N / 2) whose scores rank keep - 1 and keep: an exact tie at the cut, the lower index survives
          identical  every row the same: every score tied, the first `keep` indices survive
          zero-row   graded, with row 5 all zero: its score is exactly 0 through the clamped denominator
          clamp-edge graded rows scaled down until sqrt(nn) sqrt(mm) ~ 1.5e-20, just above the clamp"""

    def __init__(self, dtype, N, keep, kind="graded", seed=0):
        self.dtype, self.N, self.keep, self.kind, self.seed = dtype, N, keep, kind, seed
        self.id = f"prune-{NAME[dtype]}-N{N}-keep{keep}-{kind}"
        self._built = False

    def build(self):
        if self._built:
            return self
        self._built = True
        N, keep, H = self.N, self.keep, HIDDEN
        g = np.random.default_rng(7000 + self.seed)
        c = (0.5 + 0.5 * g.random(H)) * np.where(g.random(H) < 0.5, -1.0, 1.0)
        if self.kind == "identical":
            self.pair = None
            self.mem = rt(np.tile(c + 0.3 * (2 * g.random(H) - 1), (N, 1)), self.dtype)
            return self
        w = 2 * g.random((N, H)) - 1
        w *= np.linalg.norm(c) / np.linalg.norm(w, axis=1, keepdims=True)
        beta = 0.3 + 0.3 * g.random(N)
        self.pair = None if keep == N or N < 4 else (1, N // 2)
        rest = [i for i in range(N) if not self.pair or i not in self.pair]
        first = [i for i in EDGES + (N - 1,) if i in rest]
        first = list(dict.fromkeys(([5] if self.kind == "zero-row" else []) + first))
        others = [i for i in rest if i not in first]
        g.shuffle(others)
        n_hi = keep - (1 if self.pair else 0)
        hi = (first + others)[:n_hi]
        beta[hi] = 2.0 + g.random(len(hi))
        mem = c[None] + beta[:, None] * w
        if self.pair:
            mem[self.pair[0]] = mem[self.pair[1]] = c + 1.2 * w[self.pair[0]]
        if self.kind == "clamp-edge":
            mem /= np.linalg.norm(mem, axis=1, keepdims=True)
            mem *= math.sqrt(1.5e-20 / np.linalg.norm(mem.mean(0)))
        else:
            mem *= (0.5 + 1.5 * g.random((N, 1)))                    # the cosine ignores a row's length
            if self.pair:
                mem[self.pair[1]] = mem[self.pair[0]]
        if self.kind == "zero-row":
            mem[5] = 0.0
        self.mem = rt(mem, self.dtype)
        return self

    def mutants(self):
        sel, _ = self.reference()
        m = []
        if self.keep < self.N:
            if self.kind != "identical":                              # (all scores tied: either end of the order is the first `keep` rows)
                m.append("largest_kept")
            if self.pair or self.kind == "identical":
                m.append("ties_to_higher")
        if self.N > 1024 and max(sel) >= 1024:
            m.append("base_not_carried")
        if self.kind == "zero-row":
            m.append("unclamped")
        if self.kind == "clamp-edge" and self.N % 64:
            m.append("mean_divisor_rounded")
        return m

    def scores(self, mutant=None):
        self.build()
        mem = self.mem
        div = -(-self.N // 64) * 64 if mutant == "mean_divisor_rounded" else self.N
        mu = mem.sum(0) / div
        den = np.sqrt((mem * mem).sum(1)) * np.linalg.norm(mu)        # (row by row: bit-identical rows get bit-identical scores)
        with np.errstate(all="ignore"):
            return (mem * mu[None]).sum(1) / (den if mutant == "unclamped" else np.maximum(den, 1e-20))

    def reference(self, mutant=None):
        """(selected indices as the op returns them [keep], float64 scores [N])"""
        s = self.scores(mutant)
        N, keep = self.N, self.keep
        key = [(-s[i] if mutant == "largest_kept" else s[i], -i if mutant == "ties_to_higher" else i) for i in range(N)]
        sel = sorted(sorted(range(N), key=lambda i: key[i])[:keep])
        if mutant == "base_not_carried":                              # the second pass of the compaction writes from slot 0 again
            a, b = [i for i in sel if i < 1024], [i for i in sel if i >= 1024]
            sel = (b + a[len(b):] + [-1] * keep)[:keep] if len(b) <= len(a) else (b + [-1] * keep)[:keep]
        return sel, s

    def score_bound(self):
        self.build()
        mem, N = self.mem, self.N
        m = lanes_m(HIDDEN, self.dtype)
        L = min(N, 64) + -(-N // 64) + 1
        mu, a = mem.mean(0), np.abs(mem).mean(0)
        D = np.maximum(np.linalg.norm(mem, axis=1) * np.linalg.norm(mu), 1e-20)
        _, s = self.reference()
        return U * ((m + 7) * (np.abs(mem) @ np.abs(mu)) / D + L * (np.abs(mem) @ a) / D + ((m + 11) + L * np.linalg.norm(a) / np.linalg.norm(mu)) * np.abs(s))

    def cut_gap(self):
        """gap between the scores ranked keep - 1 and keep (inf when keep == N)"""
        s = np.sort(self.scores())
        return float("inf") if self.keep == self.N else float(s[self.keep] - s[self.keep - 1])


def prune_cases():
    out, i = [], 0
    for dtype in DTYPES:
        for N in PRUNE_N:
            for keep in sorted({1, max(N // 2, 1), N}):
                out.append(PruneCase(dtype, N, keep, seed=i))
                i += 1
        out.append(PruneCase(dtype, 1025, 512, "identical", seed=i))
        out.append(PruneCase(dtype, 65, 8, "zero-row", seed=i + 1))
        out.append(PruneCase(dtype, 65, 8, "clamp-edge", seed=i + 2))
        i += 3
    return out


PRUNE_CASES = prune_cases()


# ---------------------------------------------------------------------------------------------------------- pool and patchify
SIDE, OSIDE, POOL_C, POOL_F = 27, 14, HIDDEN, 2
IMAGE, PATCH, KP, KREAL = 384, 14, 592, 588
POOL_MUTANTS = ("align_corners", "xy_exchanged", "frame_stride_short")
PATCHIFY_MUTANTS = ("kykx_exchanged", "patch_major")


def pool_taps(mutant=None):
    if mutant != "align_corners":
        return O.bilinear_taps(SIDE, OSIDE)
    taps = []
    for d in range(OSIDE):
        src = d * (SIDE - 1) / (OSIDE - 1)
        i0 = min(int(math.floor(src)), SIDE - 1)
        l1 = np.float32(src - i0)
        taps.append((i0, min(i0 + 1, SIDE - 1), np.float32(1.0) - l1, l1))
    return taps


def pool_input(dtype, kind):
    """[F][729][C] float64 values of the engine type.  `gradient`: noise on a plane that rises 0.5 per row and falls 0.3 per column, the
    second frame offset and negated; `one-hot`: channel c of frame f is 1 at position (217 f + c) and 0 elsewhere, so output (o, c) IS
    the weight output o gives that position: the tap table read back."""
    S = SIDE * SIDE
    if kind == "one-hot":
        x = np.zeros((POOL_F, S, POOL_C))
        for f in range(POOL_F):
            x[f, 217 * f + np.arange(POOL_C), np.arange(POOL_C)] = 1.0
        return x
    g = np.random.default_rng(51)
    yy, xx = np.divmod(np.arange(S), SIDE)
    plane = (0.5 * yy - 0.3 * xx)[None, :, None] / 4
    x = plane + (2 * g.random((POOL_F, S, POOL_C)) - 1)
    x[1] = 1.5 - x[1]
    return rt(x, dtype)


def pool_ref(x, mutant=None, want_bound_for=None):
    """float64 [F][196][C]; with want_bound_for = dtype: (reference, bound)"""
    taps = pool_taps(mutant)
    F, S, Cn = x.shape
    flat = np.concatenate([x.reshape(F * S, Cn), np.full((S, Cn), SENTINEL)])
    out = np.empty((F, OSIDE * OSIDE, Cn))
    mag = np.empty_like(out)
    for f in range(F):
        base = f * (S - 1) if mutant == "frame_stride_short" else f * S
        for oy in range(OSIDE):
            for ox in range(OSIDE):
                (y0, y1, wy0, wy1), (x0, x1, wx0, wx1) = (taps[ox], taps[oy]) if mutant == "xy_exchanged" else (taps[oy], taps[ox])
                wy0, wy1, wx0, wx1 = float(wy0), float(wy1), float(wx0), float(wx1)
                a, b, c, d = (flat[base + yy * SIDE + xx] for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
                out[f, oy * OSIDE + ox] = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d)
                mag[f, oy * OSIDE + ox] = wy0 * (wx0 * abs(a) + wx1 * abs(b)) + wy1 * (wx0 * abs(c) + wx1 * abs(d))
    if want_bound_for is None:
        return out
    return out, 8 * U * mag + half_ulp(out, want_bound_for)


def pixels(dtype):
    """[F][3][384][384] float64 values of the engine type"""
    return rt(2 * np.random.default_rng(52).random((POOL_F, 3, IMAGE, IMAGE)) - 1, dtype)


def patchify_ref(pix, mutant=None):
    """[F * 27 * 27][592]: column k = (c, ky, kx) of the patch, columns 588 .. 591 zero"""
    F = pix.shape[0]
    p = pix[:, :, :SIDE * PATCH, :SIDE * PATCH].reshape(F, 3, SIDE, PATCH, SIDE, PATCH)          # f c py ky px kx
    order = {None: (0, 2, 4, 1, 3, 5), "kykx_exchanged": (0, 2, 4, 1, 5, 3), "patch_major": (0, 2, 4, 3, 5, 1)}[mutant]
    e = p.transpose(order).reshape(F * SIDE * SIDE, KREAL)
    return np.concatenate([e, np.zeros((e.shape[0], KP - KREAL))], 1)
