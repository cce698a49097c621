"""numpy restatement of the lossless 12-bit weight packing "P12" (streamvln_amd/csrc/gemv.hip: WP12, p12_pack_rows_kernel): encoder,
decoder, the per-lane element order of the two GEMV kernels, the GEMV cases of tests/test_p12_gpu.py and the "mutants" (plausible
decoder mistakes) that tests/test_p12_inputs.py uses to prove those cases sharp.  Test infrastructure.

Format.  For bf16 bits b: lo = b & 0xFF, hi7 = (b >> 8) & 0x7F, s = b >> 15.
  record [16 bytes per row]: T[0..7] = the row's eight most frequent hi7 values, most frequent first, ties to the lower value; a row with
      fewer distinct values repeats its last entry; then the 64-bit little-endian mask, bit k = block k falls back.
  block  [768 bytes per 512 elements = 64 chunks of 8]: 512 low bytes (chunk l's eight at 8 l), then 256 code bytes: chunk l's dword at
      512 + 4 l, byte k of it = code(element k) | code(element k + 4) << 4, code = s << 3 | j, j = the lowest index with T[j] == hi7.
  A block with a hi7 outside T is a fallback block: mask bit set, packed bytes zero, read from the bf16 original.  A ragged last block is
  zero padded.  decode = s << 15 | T[j] << 8 | lo.

Element order.  In both kernels a lane takes the chunks ci = c0 + lane + 64 * KW * k (k = 0, 1, ...) of a row in ascending order and the
eight elements of a chunk in ascending order, one fmaf chain per (row, lane); the in-flight depth only groups the loads.  ci >> 6 is the
same for every lane of a step: the fallback decision is wave-uniform."""
import functools

import numpy as np
import torch

BLOCK, BLOCK_BYTES, MAX_K, WAVES = 512, 768, 32768, 4
MUTANTS = ("swap_elements", "table_j+1", "sign_other_nibble", "lo_lane+1", "mask_blk+1", "fallback_from_packed", "drop_ragged_block", "record_row+1")


def row_bytes(K):
    return -(-K // BLOCK) * BLOCK_BYTES


def bits_of(t):
    """uint16 bit patterns of a bf16 tensor"""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def bf16_of(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def f32_of(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------ encoder / decoder
def table_of(hi7_row):
    """T[0..7] of one row and the number of distinct values it holds"""
    hist = np.bincount(hi7_row, minlength=128)
    order = sorted((v for v in range(128) if hist[v] > 0), key=lambda v: (-hist[v], v))[:8]
    return order + [order[-1]] * (8 - len(order)), len(order)


def encode(w):
    """w [N][K] uint16 -> packed [N][row_bytes(K)] uint8, records [N][16] uint8, number of fallback blocks"""
    N, K = w.shape
    assert K % 8 == 0 and 8 <= K <= MAX_K
    nblk = -(-K // BLOCK)
    packed = np.zeros((N, nblk, BLOCK_BYTES), dtype=np.uint8)
    rec = np.zeros((N, 16), dtype=np.uint8)
    pad = np.zeros((N, nblk * BLOCK), dtype=np.uint16)
    pad[:, :K] = w
    lo, hi7, s = (pad & 0xFF).astype(np.uint8), ((pad >> 8) & 0x7F).astype(np.int64), (pad >> 15).astype(np.uint8)
    n_fb = 0
    for n in range(N):
        T, _ = table_of(hi7[n, :K])
        code = np.full(128, 0xFF, dtype=np.uint8)
        for j in range(7, -1, -1):
            code[T[j]] = j
        c = code[hi7[n]]
        miss = (c == 0xFF)
        miss[K:] = False                                               # padding never misses
        c = ((s[n] << 3) | (c & 7)).astype(np.uint8)
        c[K:] = 0                                                      # a ragged last block is zero padded
        c = c.reshape(nblk, 64, 8)
        fb = miss.reshape(nblk, BLOCK).any(1)
        packed[n, :, :512] = lo[n].reshape(nblk, 512)
        packed[n, :, 512:] = (c[:, :, :4] | (c[:, :, 4:] << 4)).reshape(nblk, 256)
        packed[n, fb] = 0
        rec[n, :8] = T
        mask = sum(1 << k for k in range(nblk) if fb[k])
        rec[n, 8:] = np.frombuffer(int(mask).to_bytes(8, "little"), dtype=np.uint8)
        n_fb += int(fb.sum())
    return packed.reshape(N, nblk * BLOCK_BYTES), rec, n_fb


def masks_of(rec):
    return [int.from_bytes(bytes(r[8:]), "little") for r in rec]


def decode(packed, rec, w, mutant=None):
    """[N][K] uint16 of what a GEMV over (packed, records, bf16 original w) multiplies, under `mutant`:
      swap_elements         elements 0 and 1 of every packed chunk change places
      table_j+1             code j reads T[(j + 1) % 8]
      sign_other_nibble     the sign comes from the other nibble of the code byte (element k <-> k + 4)
      lo_lane+1             a lane reads the low bytes of the next lane of its block (63 -> 0)
      mask_blk+1            block k tests mask bit k + 1
      fallback_from_packed  the mask is ignored: a fallback block is decoded from its (zero) packed bytes
      drop_ragged_block     the ragged last block contributes nothing
      record_row+1          row n uses the record of row n + 1 (the last row its own)"""
    N, K = w.shape
    nblk = -(-K // BLOCK)
    blocks = packed.reshape(N, nblk, BLOCK_BYTES)
    if mutant == "record_row+1":
        rec = rec[np.minimum(np.arange(N) + 1, N - 1)]
    out = np.zeros((N, nblk * BLOCK), dtype=np.uint16)
    orig = np.zeros((N, nblk * BLOCK), dtype=np.uint16)
    orig[:, :K] = w
    masks = masks_of(rec)
    for n in range(N):
        T = rec[n, :8].astype(np.uint16)
        lo = blocks[n, :, :512].reshape(nblk, 64, 8).astype(np.uint16)
        cb = blocks[n, :, 512:].reshape(nblk, 64, 4)
        code = np.concatenate([cb & 0xF, cb >> 4], axis=2).astype(np.uint16)          # elements 0 .. 3 low nibbles, 4 .. 7 high nibbles
        j, s = code & 7, code >> 3
        if mutant == "table_j+1":
            j = (j + 1) % 8
        if mutant == "sign_other_nibble":
            s = np.concatenate([s[:, :, 4:], s[:, :, :4]], axis=2)
        if mutant == "lo_lane+1":
            lo = np.roll(lo, -1, axis=1)
        val = (s << 15) | (T[j] << 8) | lo
        if mutant == "swap_elements":
            val = val[:, :, [1, 0, 2, 3, 4, 5, 6, 7]]
        val = val.reshape(nblk, BLOCK)
        for k in range(nblk):
            bit = (masks[n] >> (k + 1 if mutant == "mask_blk+1" else k)) & 1
            if mutant == "fallback_from_packed":
                bit = 0
            out[n, k * BLOCK:(k + 1) * BLOCK] = orig[n, k * BLOCK:(k + 1) * BLOCK] if bit else val[k]
        if mutant == "drop_ragged_block" and K % BLOCK:
            out[n, (nblk - 1) * BLOCK:] = 0
    return out[:, :K]


# ------------------------------------------------------------------------------------------------------------------ lane order
def lane_chunks(nch, kw_count, depth):
    """{(wave on K, lane): [(chunk index, step)]}: the chunks a lane consumes, in order, and the load step each belongs to.  Restates
    dot_accum: groups of `depth` chunk positions in flight (the kernels: 2; the K-split kernel's fused-norm loop: 1), then singles."""
    out = {}
    stride = 64 * kw_count
    for kw in range(kw_count):
        for lane in range(64):
            seq, ci, step = [], kw * 64 + lane, 0
            for d in (depth, 1):
                while ci + (d - 1) * stride < nch:
                    seq += [(ci + i * stride, step) for i in range(d)]
                    ci += d * stride
                    step += 1
            out[(kw, lane)] = seq
    return out


def kw_of(kernel, K, norm):
    return 1 if kernel == "rows" else 4            # (KS_KW_NARROW = 4 and K > 4096 -> 4: the bf16 policy's values, which WP12 repeats)


# ------------------------------------------------------------------------------------------------------------------ GEMV emulation
def _fma(a, b, c):
    """fl32(a * b + c) for fp32 arrays whose product is exact in float64 (bf16 x bf16-or-fp32 operands); the float64 sum is rounded once
    more to fp32 -- a double rounding that can differ from fmaf only on a 2^-29 tie, the same way for a case and its mutants"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gemv_sums(wbits, xs, kw_count):
    """fp32 [N]: the reduced dot products of rows wbits [N][K] (uint16) with the staged activations xs [K] (fp32), in the kernels' order:
    per (wave on K, lane) one fmaf chain over its chunks ascending, the xor butterfly over the 64 lanes, then the waves on K in order"""
    with np.errstate(invalid="ignore", over="ignore"):          # (NaN / Inf weights are cases too)
        return _gemv_sums(wbits, xs, kw_count)


def _gemv_sums(wbits, xs, kw_count):
    N, K = wbits.shape
    nch = K // 8
    wf = f32_of(wbits).reshape(N, nch, 8)
    xc = xs.astype(np.float32).reshape(nch, 8)
    acc = np.zeros((N, kw_count, 64), dtype=np.float32)
    stride = 64 * kw_count
    for kw in range(kw_count):
        for k in range(-(-nch // stride)):
            c0 = kw * 64 + k * stride
            n_l = min(64, nch - c0)
            if n_l <= 0:
                break
            for e in range(8):
                acc[:, kw, :n_l] = _fma(wf[:, c0:c0 + n_l, e], xc[None, c0:c0 + n_l, e], acc[:, kw, :n_l])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ o]
    tot = acc[:, 0, 0].copy()
    for kw in range(1, kw_count):
        tot = tot + acc[:, kw, 0]
    return tot


# ------------------------------------------------------------------------------------------------------------------ designed weights
MAIN_E = (112, 128)            # biased exponents of the "main" values: hi7 56 .. 63, eight values
OUTLIER_E = tuple(range(80, 64, -2))      # eight tiny outliers (2^-47 .. 2^-61): hi7 40, 39, ..., 33


def gaussian_bits(N, K, seed, sigma=0.05):
    g = torch.Generator().manual_seed(seed)
    return bits_of((torch.randn((N, K), generator=g) * sigma).to(torch.bfloat16))


def designed_bits(N, K, fb, seed):
    """Gaussian bf16 weights (sigma 0.05) shaped so that the fallback blocks are exactly the named ones: exponents clamped into the 16
    binades of MAIN_E (eight hi7 values); classes that a row holds fewer than three times join its most frequent one; row n is scaled by
    4^-(n mod 3), so that neighbouring rows have different tables; then the eight
    OUTLIER_E values are planted once each in the first 8 elements of every block of `fb` ("none", "first", "last", "all"; "last" of a
    K % 512 != 0 is the ragged block).  With every main class at >= 3 and every outlier at <= nblk copies, the table keeps every main class
    that beats the outliers and at least one outlier stays outside it: the planted blocks fall back, the others do not."""
    w = gaussian_bits(N, K, seed)
    E = ((w >> 7) & 0xFF).astype(np.int64)
    E = np.clip(E, MAIN_E[0], MAIN_E[1] - 1)
    for n in range(N):
        h = E[n] >> 1
        cnt = np.bincount(h, minlength=128)
        top = int(np.argmax(cnt))
        rare = (cnt[h] < 3) & (h != top)
        E[n, rare] = 2 * top
    E -= 2 * (np.arange(N)[:, None] % 3)           # neighbouring rows have different tables
    w = (w & 0x807F) | (E.astype(np.uint16) << 7)
    nblk = -(-K // BLOCK)
    where = {"none": [], "first": [0], "last": [nblk - 1], "all": list(range(nblk))}[fb]
    for k in where:
        for i, e in enumerate(OUTLIER_E):
            w[:, k * BLOCK + i] = (w[:, k * BLOCK + i] & 0x807F) | np.uint16(e << 7)
    return w


def special_bits(N, K, seed):
    """weights with NaN, +-Inf, -0 and denormals: rows 0 mod 3 hold so many infinities that hi7 = 127 enters the table (the packed path
    carries them), rows 1 mod 3 hold NaNs with payloads likewise plus -0 / denormals, rows 2 mod 3 a single NaN (a fallback block)"""
    w = designed_bits(N, K, "none", seed)
    g = np.random.default_rng(seed)
    for n in range(N):
        if n % 3 == 0:
            pos = g.choice(K, max(3, K // 8), replace=False)
            w[n, pos] = np.where(g.integers(0, 2, len(pos)) == 1, 0x7F80, 0xFF80).astype(np.uint16)
        elif n % 3 == 1:
            pos = g.choice(K, max(6, K // 4), replace=False)
            third = len(pos) // 3
            w[n, pos[:third]] = (0x7FC1 + g.integers(0, 60, third)).astype(np.uint16)
            w[n, pos[third:2 * third]] = 0x8000
            w[n, pos[2 * third:]] = (0x0001 + g.integers(0, 100, len(pos) - 2 * third)).astype(np.uint16)
        else:
            w[n, g.integers(0, K)] = 0xFFC5
    return w


# ------------------------------------------------------------------------------------------------------------------ the GEMV cases
class Case:
    """one P12 GEMV launch compared bit for bit with the bf16 launch on the same arguments"""

    def __init__(self, N, K, epi="none", norm=False, bias=False, res=False, fb="none", pad=0, special=False, ties=None, seed=0):
        self.N, self.K, self.epi, self.norm, self.bias, self.res, self.fb, self.pad, self.special, self.ties, self.seed = \
            N, K, epi, norm, bias, res, fb, pad, special, ties, seed
        self.kernel = "ksplit" if epi == "none" and N <= 8192 else "rows"
        self.n_out = N // 2 if epi == "swiglu" else N
        self.id = f"{self.kernel}-{epi}-N{N}-K{K}-fb_{fb}" + ("-norm" if norm else "") + ("-bias" if bias else "") + ("-res" if res else "") + \
                  (f"-pad{pad}" if pad else "") + ("-special" if special else "") + ("-ties" if ties else "")

    @functools.lru_cache(maxsize=None)
    def build(self):
        N, K = self.N, self.K
        g = torch.Generator().manual_seed(900 + self.seed)
        self.w = special_bits(N, K, 40 + self.seed) if self.special else designed_bits(N, K, self.fb, 40 + self.seed)
        self.x = (torch.randn((K,), generator=g)).to(torch.bfloat16)
        self.x[min(9, K - 1)], self.x[K - 3] = 8.0, -8.0          # one loud activation in the first and in the last block: a single output row shows a block-sized mistake
        self.g = (1 + 0.5 * torch.randn((K,), generator=g)).to(torch.bfloat16) if self.norm else None
        self.b = torch.randn((N,), generator=g).to(torch.bfloat16) if self.bias else None
        self.r = torch.randn((N,), generator=g).to(torch.bfloat16) if self.res else None
        if self.ties:                               # two equal rows that beat every other logit: the lower index wins
            x = f32_of(bits_of(self.x))
            row = bits_of(torch.from_numpy(np.sign(x) * 0.25).to(torch.bfloat16))
            for n in self.ties:
                self.w[n] = row
        self.packed, self.rec, self.n_fb = encode(self.w)
        return self

    def W(self):
        """the bf16 original with its row stride K + pad, the padding poisoned (2^60)"""
        t = torch.full((self.N, self.K + self.pad), 2.0 ** 60, dtype=torch.bfloat16)
        t[:, :self.K] = bf16_of(self.w)
        return t

    def staged_x(self):
        x = f32_of(bits_of(self.x))
        return x * f32_of(bits_of(self.g)) if self.norm else x          # (g * x is exact in fp32; the norm's row factor multiplies a case and its mutants alike)

    def outputs(self, mutant=None):
        """what the launch stores, from the emulated sums under `mutant`: bf16 bits [n_out] (EPI_NONE / SwiGLU; the fused norm's positive
        row factor left out) or the fp32 logits' bits (arg-max)"""
        self.build()
        sums = gemv_sums(decode(self.packed, self.rec, self.w, mutant), self.staged_x(), kw_of(self.kernel, self.K, self.norm))
        if self.epi == "argmax":
            return sums.view(np.uint32)
        if self.epi == "swiglu":
            j = np.arange(self.n_out)
            gate = (j // 32) * 64 + j % 32
            a, u = sums[gate].astype(np.float64), sums[gate + 32].astype(np.float64)
            sums = (a / (1 + np.exp(-a)) * u).astype(np.float32)
        else:
            if self.b is not None:
                sums = sums + f32_of(bits_of(self.b))
            if self.r is not None:
                sums = sums + f32_of(bits_of(self.r))
        return bits_of(torch.from_numpy(sums).to(torch.bfloat16))

    def mutants(self):
        """the mutants that can show on this case: the decoder ones need a packed block, the mask ones a fallback block, the ragged one a
        ragged block, the record one a second row"""
        self.build()
        m = []
        all_fb = self.n_fb == self.N * -(-self.K // BLOCK)
        if not all_fb:                              # (with every block on the bf16 original nothing is decoded)
            m += ["swap_elements", "table_j+1", "sign_other_nibble", "lo_lane+1"]
        if self.n_fb and (not all_fb or self.K <= BLOCK):
            m.append("mask_blk+1")
        if self.n_fb:
            m.append("fallback_from_packed")
        if self.K % BLOCK:
            m.append("drop_ragged_block")
        if self.N >= 2 and not self.ties and not all_fb:
            m.append("record_row+1")
        if self.special:                            # NaN outputs hide everything else in their rows; the values are checked bit for bit on the GPU
            m = []
        return m


def cases():
    out = []
    # K ladder (chunks per row: 8, 63, 64, 65, 131, and K = 4608 for the K > 4096 geometry) on the K-split kernel, fallback patterns walking along
    for i, (K, fb) in enumerate(((64, "first"), (504, "none"), (512, "all"), (520, "none"), (1048, "first"), (4608, "last"), (1048, "none"), (1048, "all"))):
        out.append(Case(9, K, fb=fb, bias=i % 2 == 0, res=i % 3 == 0, seed=i))
    # N ladder at 131 chunks; fused norm on every other one
    for i, N in enumerate((1, 2, 3, 7, 8)):
        out.append(Case(N, 1048, norm=i % 2 == 0, fb=("last", "none", "first", "all", "last")[i], seed=10 + i))
    out.append(Case(9, 4608, norm=True, fb="first", seed=16))
    # SwiGLU [gate 32 | up 32] on the rows kernel
    out.append(Case(128, 1048, epi="swiglu", norm=True, fb="last", seed=20))
    out.append(Case(128, 520, epi="swiglu", fb="first", seed=21))
    # rows kernel with EPI_NONE (N > 8192) at one block
    out.append(Case(8195, 512, bias=True, res=True, fb="none", seed=22))
    # arg-max with two planted ties (different groups and workgroups)
    out.append(Case(1003, 1048, epi="argmax", fb="first", ties=(402, 935), seed=23))
    # NaN / Inf / -0 / denormal weights; a padded ldw over poison
    out.append(Case(9, 1048, special=True, seed=24))
    out.append(Case(12, 520, epi="none", special=True, norm=True, seed=25))
    out.append(Case(7, 1048, fb="last", pad=64, res=True, seed=26))
    out.append(Case(128, 1048, epi="swiglu", fb="all", pad=64, seed=27))
    return out


CASES = cases()


# ------------------------------------------------------------------------------------------------------------------ designed rows
def designed_rows():
    """{name: (bits [1][K], expected table, expected mask)} for the table rule and the mask (K = 1536: three blocks)"""
    K = 1536
    val = lambda h, n: np.full(n, h << 8 | 0x3C, dtype=np.uint16)
    out = {}
    # exactly 8 distinct values, frequencies 8 > 7 > ... except a tie between 70 and 66 (the lower first)
    counts = {60: 400, 61: 300, 62: 250, 63: 200, 70: 150, 66: 150, 64: 50, 65: 36}
    row = np.concatenate([val(h, c) for h, c in counts.items()])
    assert len(row) == K
    out["eight"] = (row[None], [60, 61, 62, 63, 66, 70, 64, 65], 0)
    # 9 distinct: the least frequent (hi7 5, twice, in block 1) stays outside
    row9 = row.copy()
    row9[700], row9[701] = 5 << 8, 5 << 8 | 1
    t9, _ = table_of((row9 >> 8) & 0x7F)
    out["nine"] = (row9[None], t9, 0b010)
    out["one"] = (val(33, K)[None], [33] * 8, 0)
    lane0 = row.copy()
    lane0[0] = 2 << 8
    out["outlier_lane0_first"] = (lane0[None], out["eight"][1], 0b001)
    lane63 = row.copy()
    lane63[K - 1] = 0x8000 | 2 << 8
    out["outlier_lane63_last"] = (lane63[None], out["eight"][1], 0b100)
    esc = row.copy()
    for k in range(3):
        esc[k * BLOCK + 100 + k] = 3 << 8
    out["every_block"] = (esc[None], out["eight"][1], 0b111)
    return out
