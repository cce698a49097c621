"""Float64 reference of the LLM attention path (RoPE, paged causal / decode attention, split-KV merge), sharp inputs for it, the
tolerance of a kernel against it, and "mutant" references (plausible kernel mistakes) that prove the inputs sharp.

Inputs are designed in roped space and un-roped to give the kernel's q|k|v rows:
  * keys k_r[s] = a_s * u + n_s per kv head: u is a unit sign vector, n_s unit sign vectors with their u component removed, a_s = s / S0.
    Query q_r = c * n_j makes key j a needle (logit ~ +60, the others ~ N(0, 5.3)); q_r = +-c * u gives logits rising / falling by
    60 / S0 per key along the whole sequence (the running max moves at every key tile, by large factors; or sits in the first tile and
    the later tiles underflow in exp2).
  * V rows are distinct per key (uniform in +-1).
  * "next" puts the needle on the first masked key (the key after the row's diagonal): a kernel that admits it is far off.
Each q head of each query row takes one pattern of the case (head h of the row at position t: patterns[(h + t) % n]; the one row of a
decode step: patterns[h]).
"""
import math

import numpy as np
import torch

from oracle import streamvln_oracle as O

HD = 128
PAGE = 64
LOGIT = 60.0            # needle / ramp logit magnitude (natural units, after the 1/sqrt(128) scale)
SENTINEL = 1.0e4        # value of every pool slot an op has not written (finite: masked keys meet stale data in production)
EPS = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}       # unit roundoff of the engine dtype


def rnd_dtype(x, dtype):
    """round a float64 tensor to the engine dtype and come back"""
    return x.to(dtype).to(torch.float64)


def rope(x, pos, theta, inverse=False):
    """x [n, heads, 128] float64 at positions pos [n]: Qwen2 RoPE with the oracle's fp32 angles, the rest in float64"""
    cos, sin = O.rope_cos_sin(torch.as_tensor(pos), HD, theta)
    cos, sin = cos.double()[:, None], sin.double()[:, None]
    return x * cos - O.rotate_half(x) * sin if inverse else x * cos + O.rotate_half(x) * sin


def prefill_split(cfg, T, kv_len, prefill_split_rows=2048):
    """(nsplit, tiles_per_split) of llm_attn_args for a prefill of T rows over kv_len keys"""
    G = cfg.q_heads // cfg.kv_heads
    rows, tiles = T * G, (kv_len + PAGE - 1) // PAGE
    wgs = ((rows + 127) // 128) * cfg.kv_heads
    if rows <= prefill_split_rows and wgs < 128 and tiles >= 4:
        ns = min((256 + wgs - 1) // wgs, 8, tiles // 2)
        if ns > 1:
            return ns, (tiles + ns - 1) // ns
    return 1, max(tiles, 1)


def decode_split(cfg, max_positions):
    """tiles_per_split of the engine's decode attention (one 64-key page per split while there are <= 64 pages)"""
    pages = max_positions // PAGE
    tps = 1
    while (pages + tps - 1) // tps > 64:
        tps += 1
    return tps


class Case:
    """One attention launch: L keys (positions 0 .. L-1), query rows at positions qpos (the last T positions, or one decode position)."""

    def __init__(self, cfg, dtype, L, qpos, patterns, seed, tps, nsplit, S0=None):
        self.cfg, self.dtype, self.L, self.seed = cfg, dtype, L, seed
        self.qpos = np.asarray(qpos)
        self.patterns, self.tps, self.nsplit = patterns, tps, nsplit
        self.S0 = S0 or max(L, 128)
        self.G = cfg.q_heads // cfg.kv_heads
        self.scale = HD ** -0.5
        self._build()

    def pattern(self, h, t):
        return self.patterns[(h + t) % len(self.patterns)]

    def needle(self, pat, t):
        """key index of a needle pattern for the query at position t"""
        split_keys = self.tps * PAGE
        z = t // split_keys
        return {"newest": t, "next": min(t + 1, self.L - 1), "sink": 0, "key63": min(63, t), "key64": min(64, t),
                "tile_first": (t // PAGE) * PAGE, "tile_last": max((t // PAGE) * PAGE - 1, 0),
                "split_first": z * split_keys, "split_last": max(z * split_keys - 1, 0)}[pat]

    def _build(self):
        cfg, L, dtype = self.cfg, self.L, self.dtype
        nq, nkv = cfg.q_heads, cfg.kv_heads
        g = torch.Generator().manual_seed(self.seed)
        sign = lambda *s: (torch.randint(0, 2, s, generator=g).double() * 2 - 1) / math.sqrt(HD)
        u = sign(nkv, HD)
        n = sign(L, nkv, HD)
        n = n - (n * u[None]).sum(-1, keepdim=True) * u[None]
        a = torch.arange(L, dtype=torch.float64) / self.S0
        k_r = a[:, None, None] * u[None] + n
        v = torch.rand((L, nkv, HD), generator=g, dtype=torch.float64) * 2 - 1
        c = LOGIT / self.scale
        R = len(self.qpos)
        q_r = torch.zeros((R, nq, HD), dtype=torch.float64)
        for i, t in enumerate(self.qpos.tolist()):
            for h in range(nq):
                kh, pat = h // self.G, self.pattern(h, 0 if len(self.qpos) == 1 else t)
                if pat == "rising":
                    q_r[i, h] = c * u[kh]
                elif pat == "falling":
                    q_r[i, h] = -c * u[kh]
                elif pat == "two":         # the newest key and the last key of the split before t's split (key 0 while t is in the
                                           # first split): two competing needles in different splits
                    j = self.needle("split_last", t) if t >= self.tps * PAGE else 0
                    q_r[i, h] = c * (n[t, kh] + n[j, kh])
                else:
                    q_r[i, h] = c * n[self.needle(pat, t), kh]
        # kernel inputs: un-roped, rounded to the engine dtype; every position has a q|k|v row (q of the non-query rows: random)
        pos = torch.arange(L)
        self.k_in = rnd_dtype(rope(k_r, pos, cfg.rope_theta, inverse=True), dtype)
        self.v = rnd_dtype(v, dtype)
        q_all = torch.rand((L, nq, HD), generator=g, dtype=torch.float64) * 2 - 1
        q_all[torch.as_tensor(self.qpos)] = rope(q_r, self.qpos, cfg.rope_theta, inverse=True)
        self.q_in = rnd_dtype(q_all, dtype)
        # what the kernel stores: roped q / k rounded to the engine dtype (a kernel's own fp32 RoPE may round a value the other way:
        # tests replace these by read-back rows where the op makes them visible)
        self.k = rnd_dtype(rope(self.k_in, pos, cfg.rope_theta), dtype)
        self.q = rnd_dtype(rope(self.q_in[torch.as_tensor(self.qpos)], self.qpos, cfg.rope_theta), dtype)

    def qkv_rows(self):
        """[L, (nq + 2 nkv) * 128] float64 q|k|v rows of positions 0 .. L-1"""
        L = self.L
        return torch.cat([self.q_in.reshape(L, -1), self.k_in.reshape(L, -1), self.v.reshape(L, -1)], 1)

    # ------------------------------------------------------------------------------------------------------ reference
    def attend(self, q=None, k=None, v=None, mutant=None, device="cpu"):
        """float64 attention of the query rows -> [R, nq, 128].  mutant: None or one of MUTANTS."""
        q = (self.q if q is None else q).to(device)
        k = (self.k if k is None else k).to(device)
        v = (self.v if v is None else v).to(device)
        L, G = self.L, self.G
        qpos = torch.as_tensor(self.qpos, device=device)
        keys = torch.arange(L + 1, device=device)
        # one extra key slot past kv_len holds the sentinel: a kernel that admits it reads stale pool data
        k = torch.cat([k, torch.full_like(k[:1], SENTINEL)], 0)
        v = torch.cat([v, torch.full_like(v[:1], SENTINEL)], 0)
        allowed = (keys[None] <= qpos[:, None]) & (keys[None] < L)
        if mutant == "drop_newest":
            allowed &= keys[None] != qpos[:, None]
        elif mutant == "admit_masked":             # the first key past the diagonal (past kv_len on the last row: a stale slot)
            allowed |= keys[None] == (qpos[:, None] + 1)
        elif mutant == "diag_shift":               # causal diagonal one key too far where that key exists
            allowed |= (keys[None] == (qpos[:, None] + 1)) & (keys[None] < L)
        elif mutant == "rope_off":                 # q roped at the next position
            q = rnd_dtype(rope(self.q_in[torch.as_tensor(self.qpos)], self.qpos + 1, self.cfg.rope_theta), self.dtype).to(device)
        elif mutant == "page_swap":                # logical page 0 and the last (partial) page read each other's physical page
            lp = (L - 1) // PAGE
            n_pad = max((lp + 1) * PAGE, L + 1)
            kp = torch.full((n_pad,) + k.shape[1:], SENTINEL, dtype=k.dtype, device=device)
            vp = kp.clone()
            kp[:L], vp[:L] = k[:L], v[:L]
            a, b = slice(0, PAGE), slice(lp * PAGE, (lp + 1) * PAGE)
            kp[a], kp[b] = kp[b].clone(), kp[a].clone()
            vp[a], vp[b] = vp[b].clone(), vp[a].clone()
            k, v = kp[:L + 1], vp[:L + 1]
        elif mutant == "stale_k":                  # the newest key's K slot not written (stale pool data) -> the last query row
            k = k.clone()
            k[L - 1] = SENTINEL
        elif mutant == "drop_split":               # split 0's partial left out of the merge (only when there are splits)
            allowed &= keys[None] >= self.tps * PAGE
        kk = k.repeat_interleave(G, 1)             # [L+1, nq, 128]
        vv = v.repeat_interleave(G, 1)
        s = torch.einsum("rhd,shd->rhs", q, kk) * self.scale
        s = s.masked_fill(~allowed[:, None, :], float("-inf"))
        if mutant == "no_rescale":
            return self._no_rescale(s, vv)
        p = torch.softmax(s, -1)
        p = torch.nan_to_num(p)
        return torch.einsum("rhs,shd->rhd", p, vv)

    def _no_rescale(self, s, vv):
        """online softmax whose O accumulator is never rescaled when the running max moves (l is), per split, splits merged right"""
        R, H, S = s.shape
        ntiles = (S + PAGE - 1) // PAGE
        Os, ms, ls = [], [], []
        for z0 in range(0, ntiles, self.tps):
            m = torch.full((R, H), float("-inf"), dtype=s.dtype, device=s.device)
            o = torch.zeros((R, H, HD), dtype=s.dtype, device=s.device)
            ssum = []
            for t in range(z0, min(z0 + self.tps, ntiles)):
                st = s[:, :, t * PAGE:(t + 1) * PAGE]
                m = torch.maximum(m, st.amax(-1))
                pe = torch.nan_to_num(torch.exp(st - m[..., None]))
                o = o + torch.einsum("rhs,shd->rhd", pe, vv[t * PAGE:(t + 1) * PAGE])
                ssum.append(st)
            l = torch.nan_to_num(torch.exp(torch.cat(ssum, -1) - m[..., None])).sum(-1)
            Os.append(o), ms.append(m), ls.append(l)
        M = torch.stack(ms).amax(0)
        w = [torch.nan_to_num(torch.exp(m - M)) for m in ms]
        num = sum(wz[..., None] * oz for wz, oz in zip(w, Os))
        den = sum(wz * lz for wz, lz in zip(w, ls))
        return num / den.clamp_min(1e-300)[..., None]

    # ------------------------------------------------------------------------------------------------------ tolerance
    def tolerance(self, q=None, k=None, q_flips=True, device="cpu"):
        """per-element bound [R, nq, 1] of |kernel - reference|, relative to mv = max |V| of the head's keys (the output's natural
        scale: every output is a convex combination of V rows).  From the kernel's rounding points, with u = unit roundoff of the dtype
        and e = 2^-24 (fp32 accumulation):
          * P rounded to the dtype as the B operand of the P.V product (bf16: the fp32 instantiation keeps P in fp32):      u * mv
          * the output stored in the dtype (one rounding of an fp32 value of magnitude <= mv):                              u * mv
          * the logits: a 128-term fp32 dot product (worst case 128 e A, A = max over keys of scale * sum_d |q_d k_d|), the
            fp32 fma with the log2 scale and v_exp_f32 (a few ulp): a relative error d of every p, numerator and l  -> 2 d mv
          * fp32 sums over L keys of p v and of p (worst case L e each)                                               -> 2 L e mv
          * q_flips (decode: the kernel ropes q in registers in fp32, the reference rounds a float64 RoPE: an element can round
            the other way).  Assumed at most 2 elements per row, each 2u relative; a logit error ds moves out_d by at most
            ds * sum_j p_j |v_jd - out_d| to first order, taken twice.  fp32: every element may differ by 2 e, and by
            the kernel's cos / sin table (roped_k_bound): ds = 8 e A.
        The read-back K rows are used for the keys (no flips there); q of a prefill is read back too (q_flips=False)."""
        q = (self.q if q is None else q).to(device)
        k = (self.k if k is None else k).to(device)
        u, e = EPS[self.dtype], 2.0 ** -24
        kk = k.repeat_interleave(self.G, 1)
        qpos = torch.as_tensor(self.qpos, device=device)
        vis = (torch.arange(self.L, device=device)[None] <= qpos[:, None]).double()     # [R, L]
        mv = self.v.to(device).abs().amax(-1).amax(0).repeat_interleave(self.G)          # [nq]
        tol = rounding_tolerance(q, kk, vis, self.scale, mv, self.dtype, self.L)
        A = (torch.einsum("rhd,shd->rhs", q.abs(), kk.abs()) * self.scale * vis[:, None]).amax(-1)
        if q_flips:
            if self.dtype == torch.bfloat16:
                term = (q.abs()[:, :, None, :] * kk.abs().permute(1, 0, 2)[None]).amax(-1) * self.scale     # [R, nq, L]
                ds = 2 * (2 * u) * (term * vis[:, None]).amax(-1)
            else:           # rounding (2 e A) and the kernel's cos / sin table (roped_k_bound: 2^-22 (|x1| + |x2|) per element,
                ds = 8 * e * A  # |x1| + |x2| <= sqrt(2) |(q1, q2)|: at most ~6 e A more)
            # first order: logits moved by at most ds move out_d by at most ds * sum_j p_j |v_jd - out_d|; twice that
            s = torch.einsum("rhd,shd->rhs", q, kk) * self.scale
            p = torch.nan_to_num(torch.softmax(s.masked_fill(vis[:, None] == 0, float("-inf")), -1))
            vv = self.v.to(device).repeat_interleave(self.G, 1)
            out = torch.einsum("rhs,shd->rhd", p, vv)
            sens = torch.einsum("rhs,rhsd->rhd", p, (vv.permute(1, 0, 2)[None] - out[:, :, None]).abs())
            tol = tol + 2 * ds[..., None] * sens
        return tol


def rounding_tolerance(q, kk, vis, scale, mv, dtype, L, hd=HD):
    """the part of Case.tolerance without q flips (see there), for hd-term dot products: q [R, H, hd], keys kk [L, H, hd], vis [R, L]
    (1 = visible key), mv [H] = max |V| of the head's keys -> [R, H, 1]"""
    u, e = EPS[dtype], 2.0 ** -24
    A = (torch.einsum("rhd,shd->rhs", q.abs(), kk.abs()) * scale * vis[:, None]).amax(-1)         # [R, H]
    coef = 2 * u + 2 * (hd * e * A + 8 * e) + 2 * L * e
    return (coef * mv[None])[..., None]


MUTANTS = ["drop_newest", "admit_masked", "diag_shift", "rope_off", "no_rescale", "page_swap", "stale_k", "drop_split"]


def mutant_ratios(case, mutants, q_flips=True, device="cpu"):
    """{mutant: max over elements of |mutant - reference| / tolerance} on the case's own reference"""
    ref = case.attend(device=device)
    tol = case.tolerance(q_flips=q_flips, device=device)
    return {mname: float(((case.attend(mutant=mname, device=device) - ref).abs() / tol).amax()) for mname in mutants}


def roped_k_bound(k_in, pos, theta, dtype):
    """bound of |stored roped K - reference| per element: one ulp of the dtype (the kernel rounds its fp32 RoPE, the reference its
    float64 one), plus the kernel's fp32 arithmetic (two products and a sum: 4 fp32 roundings of |x1 c| + |x2 s|, which matters where
    the sum cancels), plus its cos / sin table: the engine takes the inverse frequencies from the host's powf, which can differ from the
    oracle's fp32 pow by one ulp (theta = 1e6: one of the 64 frequencies), so at large positions an entry can differ by 2^-23 absolute
    (seen on a host emulation of the table; the fp32 decode at positions > 3400 went past the bound without this term); taken twice:
    2^-22 (|x1| + |x2|)"""
    cos, sin = O.rope_cos_sin(torch.as_tensor(pos), HD, theta)
    cos, sin = cos.double()[:, None], sin.double()[:, None]
    ref = rnd_dtype(rope(k_in, pos, theta), dtype)
    mag = k_in.abs() * cos.abs() + O.rotate_half(k_in).abs() * sin.abs()
    tab = 2.0 ** -22 * (k_in.abs() + O.rotate_half(k_in).abs())
    mant = 7 if dtype == torch.bfloat16 else 23
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - mant)
    return ref, ulp + 4 * 2.0 ** -24 * mag + tab


# ---------------------------------------------------------------------------------------------------------- the cases
DECODE_PATTERNS = ["newest", "sink", "tile_first", "rising", "tile_last", "two", "falling", "key63"]
PREFILL_PATTERNS = ["newest", "rising", "next", "sink", "split_first", "falling", "two", "key64", "split_last"]
MAX_POSITIONS = 2048        # of the test engine: 32 pages of 64 keys per env, one page per decode split
WIDE_POSITIONS = 4096       # the production capacity: 64 decode splits, the widest merge attn_combine_kernel runs


def decode_cases():
    """(cfg name, positions of the B envs, max_positions of the engine)"""
    out = []
    for cfg, far in (("tiny", 777), ("true_dims_1layer", 1500)):
        for p in (0, 63, 64, 128, far, MAX_POSITIONS - 1):
            out.append((cfg, (p,), MAX_POSITIONS))
        out += [(cfg, (300, 64), MAX_POSITIONS), (cfg, (0, 63, far, MAX_POSITIONS - 1), MAX_POSITIONS),
                (cfg, (5, 64, 127, 128, 700, far, MAX_POSITIONS - 1, 63), MAX_POSITIONS)]
        out += [(cfg, (WIDE_POSITIONS - 1,), WIDE_POSITIONS), (cfg, (4000, 2100), WIDE_POSITIONS)]
    return out


PREFILL_CASES = [("tiny", 212, 0), ("tiny", 37, 300), ("true_dims_1layer", 1952, 0), ("true_dims_1layer", 212, 800),
                 ("true_dims_1layer", 212, 1740)]


def decode_case(cfg, dtype, pos, b, max_positions=MAX_POSITIONS):
    return Case(cfg, dtype, pos + 1, [pos], DECODE_PATTERNS, seed=7000 + 31 * pos + b, tps=decode_split(cfg, max_positions),
                nsplit=max_positions // PAGE)


def prefill_case(cfg, dtype, T, P, rows=None):
    ns, tps = prefill_split(cfg, T, P + T)
    qpos = np.arange(P, P + T) if rows is None else np.asarray(rows)
    return Case(cfg, dtype, P + T, qpos, PREFILL_PATTERNS, seed=9000 + T + P, tps=tps, nsplit=ns)


def decode_mutants(pos):
    m = ["drop_newest", "admit_masked"]
    if pos > 0:             # (one visible key: the output is its V whatever its logit)
        m += ["rope_off", "stale_k"]
    if pos >= PAGE:
        m.append("drop_split")
        if (pos + 1) % PAGE:    # (two full pages swapped only permute the keys: the K / V read-back checks the page mapping there)
            m.append("page_swap")
    return m


def prefill_mutants(cfg, T, P):
    ns, tps = prefill_split(cfg, T, P + T)
    m = ["drop_newest", "admit_masked", "diag_shift", "rope_off", "stale_k", "page_swap"]
    if tps > 1:
        m.append("no_rescale")
    if ns > 1:
        m.append("drop_split")
    return m


# ---------------------------------------------------------------------------------------------------------- ViT
# SigLIP attention (siglip_encoder.py:197-232): per frame and head, 729 query rows against the frame's 729 keys, non-causal, head_dim 72,
# no RoPE.  The engine packs K into pages [tile][F * heads][64][HDP] and V^T into [tile][F * heads][96][64] (12 key tiles, the last one
# holding 25 keys), then runs either the plain 4-wave kernel over all 12 tiles or, when that would be too few workgroups, key groups:
# group g of KG walks tiles g, g + KG, ... and the groups' (m, l, O) are merged through LDS with exp2(m_g - M).
VHD = 72
VS = 729
VTILES = (VS + PAGE - 1) // PAGE
VROWS = 96
VIT_PATTERNS = ["key0", "self", "key63", "rising", "key64", "key703", "two", "group_first", "key728", "falling"]
VIT_CASES = [("tiny", 1), ("tiny", 3), ("true_dims_1layer", 1), ("true_dims_1layer", 2), ("true_dims_1layer", 9)]


def vit_hdp(dtype):
    """padded K row of the ViT pools: 72 rounded to an even number of 16-byte chunks"""
    epc = 8 if dtype == torch.bfloat16 else 4
    return ((((VHD + epc - 1) // epc) + 1) & ~1) * epc


def vit_key_groups(cfg, F, dtype):
    """KG of the engine's ViT attention (vit_attn_args): key groups when the plain kernel would have fewer than 192 workgroups
    (attn_key_groups: 4 for bf16, 3 for fp32), else 1 (the plain kernel)"""
    if ((VS + 127) // 128) * F * cfg.v_heads < 192:
        return 4 if dtype == torch.bfloat16 else 3
    return 1


class VitCase:
    """F frames of ViT q / k / v [F, 729, heads, 72] (float64 holding dtype values) and their float64 attention, tolerance and mutants.
    rows: the query rows evaluated (all 729 by default)."""

    def __init__(self, cfg, dtype, F, q, k, v, rows=None):
        self.cfg, self.dtype, self.F = cfg, dtype, F
        self.heads = cfg.v_heads
        self.KG = vit_key_groups(cfg, F, dtype)
        self.q, self.k, self.v = q, k, v
        self.rows = torch.arange(VS) if rows is None else torch.as_tensor(rows)
        self.scale = VHD ** -0.5

    def qkv_rows(self):
        """[F * 729, 3 * heads * 72] q | k | v rows as the engine's qkv buffer holds them"""
        n = self.F * VS
        return torch.cat([self.q.reshape(n, -1), self.k.reshape(n, -1), self.v.reshape(n, -1)], 1)

    def mutants(self):
        m = ["drop_last_tile", "admit_pad", "no_rescale", "wrong_frame", "vt_swap"]
        if self.KG > 1:
            m += [f"drop_group{g}" for g in range(self.KG)] + ["merge_no_rescale"]
        else:
            m += ["drop_tile1"]
        return m

    def attend(self, mutant=None, device="cpu"):
        """float64 attention of the evaluated rows -> [F, R, heads, 72].  mutant: None or one of self.mutants():
          drop_last_tile  the partial tile (keys 704 .. 728) left out
          admit_pad       keys 729 .. 767 of the last tile admitted (the packers zero them)
          drop_group<g>   key group g's tiles left out of the merge; drop_tile1: tile 1 left out (plain kernel)
          no_rescale      online softmax whose O is never rescaled when the running max moves (per key group; merge right)
          merge_no_rescale  key groups right, merged without exp2(m_g - M)
          wrong_frame     frame f reads frame f + 1's pages (F >= 2), or head h reads head h + 1's (F = 1)
          vt_swap         V^T keys swapped between the two halves of every tile"""
        keys = torch.arange(VTILES * PAGE, device=device)
        allowed = keys < VS
        tile = keys // PAGE
        if mutant == "drop_last_tile":
            allowed = keys < (VTILES - 1) * PAGE
        elif mutant == "admit_pad":
            allowed = torch.ones_like(allowed)
        elif mutant is not None and mutant.startswith("drop_group"):
            allowed = allowed & (tile % self.KG != int(mutant[len("drop_group"):]))
        elif mutant == "drop_tile1":
            allowed = allowed & (tile != 1)
        out = []
        for f in range(self.F):
            q = self.q[f, self.rows].to(device)                                   # [R, H, 72]
            k, v = self.k[f].to(device), self.v[f].to(device)                     # [729, H, 72]
            if mutant == "wrong_frame":
                k, v = (self.k[(f + 1) % self.F].to(device), self.v[(f + 1) % self.F].to(device)) if self.F > 1 else \
                       (torch.roll(k, -1, 1), torch.roll(v, -1, 1))
            pad = torch.zeros((VTILES * PAGE - VS,) + k.shape[1:], dtype=k.dtype, device=device)
            k, v = torch.cat([k, pad]), torch.cat([v, pad])
            if mutant == "vt_swap":
                v = v[keys ^ 32]
            s = torch.einsum("rhd,shd->rhs", q, k) * self.scale
            s = s.masked_fill(~allowed[None, None], float("-inf"))
            if mutant in ("no_rescale", "merge_no_rescale"):
                out.append(self._grouped(s, v, online_rescale=mutant != "no_rescale", merge_rescale=mutant != "merge_no_rescale"))
            else:
                out.append(torch.einsum("rhs,shd->rhd", torch.nan_to_num(torch.softmax(s, -1)), v))
        return torch.stack(out)

    def _grouped(self, s, v, online_rescale, merge_rescale):
        """the kernel's schedule: key group g walks tiles g, g + KG, ... with an online softmax, the groups are merged at the end"""
        os_, ms, ls = [], [], []
        for g in range(self.KG):
            idx = torch.cat([torch.arange(t * PAGE, (t + 1) * PAGE) for t in range(g, VTILES, self.KG)]).to(s.device)
            sg = s[..., idx]
            m = torch.full(s.shape[:2], float("-inf"), dtype=s.dtype, device=s.device)
            o = torch.zeros(s.shape[:2] + (VHD,), dtype=s.dtype, device=s.device)
            for t0 in range(0, idx.numel(), PAGE):
                st = sg[..., t0:t0 + PAGE]
                mnew = torch.maximum(m, st.amax(-1))
                if online_rescale:
                    o = o * torch.nan_to_num(torch.exp(m - mnew))[..., None]
                m = mnew
                o = o + torch.einsum("rhs,shd->rhd", torch.nan_to_num(torch.exp(st - m[..., None])), v[idx[t0:t0 + PAGE]])
            os_.append(o), ms.append(m), ls.append(torch.nan_to_num(torch.exp(sg - m[..., None])).sum(-1))
        M = torch.stack(ms).amax(0)
        w = [torch.nan_to_num(torch.exp(m - M)) if merge_rescale else torch.ones_like(M) for m in ms]
        num = sum(wg[..., None] * og for wg, og in zip(w, os_))
        den = sum(wg * lg for wg, lg in zip(w, ls))
        return num / den.clamp_min(1e-300)[..., None]

    def tolerance(self, device="cpu"):
        """[F, R, heads, 1]: rounding_tolerance over the frame's 729 keys (no q flips: q is read as stored)"""
        vis = torch.ones((len(self.rows), VS), dtype=torch.float64, device=device)
        tol = []
        for f in range(self.F):
            mv = self.v[f].to(device).abs().amax(-1).amax(0)                  # [H]
            tol.append(rounding_tolerance(self.q[f, self.rows].to(device), self.k[f].to(device), vis, self.scale, mv,
                                          self.dtype, VS, hd=VHD))
        return torch.stack(tol)


def vit_case(cfg, dtype, F, rows=None):
    """sharp ViT inputs, the LLM design in 72 dimensions (no RoPE): keys k[s] = a_s u + n_s per (frame, head) with sign vectors u, n_s
    (u removed from n_s) and a_s = s / 728; V rows distinct (uniform in +-1).  Query row s of head h in frame f takes pattern
    VIT_PATTERNS[(s + h + 3 f) % 10] (needle placements move from frame to frame):
      key0 / key63 / key64 / key703 / key728 (the last valid key, in the partial tile) / self: q = c n_j, a needle of logit ~60 at key j;
      group_first: the first key of key group g's first tile (key 64 g, g = (s // 10) % KG, KG = 4 for the plain kernel);
      two: equal needles at keys 0 and 728 (different key groups);  rising / falling: q = +-c u, logits +-60 a_s over all 729 keys."""
    seed = 11000 + 97 * F + (1 if dtype == torch.bfloat16 else 0) + (500 if cfg.name != "tiny" else 0)
    g = torch.Generator().manual_seed(seed)
    H = cfg.v_heads
    sign = lambda *s: (torch.randint(0, 2, s, generator=g).double() * 2 - 1) / math.sqrt(VHD)
    u = sign(F, 1, H, VHD)
    n = sign(F, VS, H, VHD)
    n = n - (n * u).sum(-1, keepdim=True) * u
    a = torch.arange(VS, dtype=torch.float64) / (VS - 1)
    k = a[None, :, None, None] * u + n
    v = torch.rand((F, VS, H, VHD), generator=g, dtype=torch.float64) * 2 - 1
    c = LOGIT * math.sqrt(VHD)
    kg = vit_key_groups(cfg, F, dtype)
    kg = kg if kg > 1 else 4
    q = torch.zeros((F, VS, H, VHD), dtype=torch.float64)
    fixed = {"key0": 0, "key63": 63, "key64": 64, "key703": 703, "key728": VS - 1}
    for f in range(F):
        for s in range(VS):
            for h in range(H):
                pat = VIT_PATTERNS[(s + h + 3 * f) % len(VIT_PATTERNS)]
                if pat == "rising":
                    q[f, s, h] = c * u[f, 0, h]
                elif pat == "falling":
                    q[f, s, h] = -c * u[f, 0, h]
                elif pat == "two":
                    q[f, s, h] = c * (n[f, 0, h] + n[f, VS - 1, h])
                else:
                    j = fixed.get(pat, s if pat == "self" else PAGE * ((s // len(VIT_PATTERNS)) % kg))
                    q[f, s, h] = c * n[f, j, h]
    return VitCase(cfg, dtype, F, rnd_dtype(q, dtype), rnd_dtype(k, dtype), rnd_dtype(v, dtype), rows=rows)


def vit_mutant_ratios(case, device="cpu"):
    """{mutant: max over elements of |mutant - reference| / tolerance}"""
    ref = case.attend(device=device)
    tol = case.tolerance(device=device)
    return {mname: float(((case.attend(mutant=mname, device=device) - ref).abs() / tol).amax()) for mname in case.mutants()}
