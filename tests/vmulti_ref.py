"""Reference for the batched verify attention (svln_op_attention_verify_multi: attn_verify_multi_kernel + the multi form of the verify
merge), on top of tests/attn_ref.py and tests/verify_ref.py.

A scenario is ONE launch: S sequences, sequence z with P_z context rows, R_z (0 .. T) of its T row slots verified at positions P_z ...,
on disjoint page tables or on the fork layout (every sequence shares sequence 0's context: the pages below q0 = P / 64 are sequence 0's,
the page of P is a private copy).  Each sequence is an attn_ref.Case of its own (its own needles, ramps, K and V rows); the sequences of a
fork scenario share the key direction u and the context rows and differ in everything they bring themselves.

`launch` is a float64 model of the launch on a physical pool (sentinel-filled, page tables per sequence): the appended rows, the output
rows (NaN where the launch writes nothing) and, through the pool, every slot it leaves alone.  Its mutants are the mistakes only a
several-sequence launch can make (see MUTANTS); tests/test_vmulti_inputs.py proves that the scenarios show each of them."""
import math

import numpy as np
import torch

import attn_ref as R
import verify_ref as VR

NP = R.MAX_POSITIONS // R.PAGE          # pages of one sequence's table
#: name -> (cfg, T, layout, [(P_z, R_z)]).  Start positions 0, 61 (four rows cross the page edge), 63, 64, 130 (past the first key split:
#: one page per split at 2048 positions); row counts over {0, 1, T}; S = 1, 2, 3, 8; both layouts; both head ratios (2 and 7).
SCENARIOS = {
    "tiny_s1": ("tiny", 4, "disjoint", [(61, 4)]),
    "tiny_s2": ("tiny", 4, "disjoint", [(0, 4), (63, 1)]),
    "tiny_s3": ("tiny", 4, "disjoint", [(64, 4), (61, 0), (130, 4)]),
    "tiny_s8": ("tiny", 8, "disjoint", [(0, 8), (61, 1), (63, 0), (64, 8), (130, 1), (61, 8), (5, 0), (200, 8)]),
    "tiny_fork3": ("tiny", 4, "fork", [(61, 4), (61, 1), (61, 4)]),
    "tiny_fork8": ("tiny", 4, "fork", [(130, 4), (130, 0), (130, 1), (130, 4), (130, 4), (130, 1), (130, 0), (130, 4)]),
    "tiny_fork_edge": ("tiny", 4, "fork", [(64, 4), (64, 4)]),
    "tiny_fork_63": ("tiny", 4, "fork", [(63, 4), (63, 4), (63, 0)]),
    "tiny_fork_0": ("tiny", 4, "fork", [(0, 4), (0, 1)]),
    "true_s3": ("true_dims_1layer", 4, "disjoint", [(61, 4), (0, 1), (64, 0)]),
    "true_s2": ("true_dims_1layer", 4, "disjoint", [(63, 4), (130, 4)]),
    "true_fork8": ("true_dims_1layer", 4, "fork", [(61, 4), (61, 1), (61, 0), (61, 4), (61, 4), (61, 4), (61, 1), (61, 4)]),
}
MUTANTS = ["table0", "pos0", "rows0", "q0", "part0", "append_shared", "zero_rows_append", "append_all_slots"]


class SeqCase(R.Case):
    """attn_ref.Case whose key direction u and first `shared` positions (K, V, the random q rows) come from `shared_seed`, the rest from
    the case's own seed: the sequences of a fork scenario"""

    def __init__(self, cfg, dtype, L, qpos, patterns, seed, tps, nsplit, shared, shared_seed):
        self.shared, self.shared_seed = shared, shared_seed
        super().__init__(cfg, dtype, L, qpos, patterns, seed, tps, nsplit)

    def _build(self):
        cfg, L, dtype, P = self.cfg, self.L, self.dtype, self.shared
        nq, nkv = cfg.q_heads, cfg.kv_heads
        gs, g = torch.Generator().manual_seed(self.shared_seed), torch.Generator().manual_seed(self.seed)
        sign = lambda gen, *s: (torch.randint(0, 2, s, generator=gen).double() * 2 - 1) / math.sqrt(R.HD)
        uni = lambda gen, *s: torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1
        u = sign(gs, nkv, R.HD)
        n = torch.cat([sign(gs, P, nkv, R.HD), sign(g, L - P, nkv, R.HD)], 0)
        n = n - (n * u[None]).sum(-1, keepdim=True) * u[None]
        a = torch.arange(L, dtype=torch.float64) / self.S0
        k_r = a[:, None, None] * u[None] + n
        v = torch.cat([uni(gs, P, nkv, R.HD), uni(g, L - P, nkv, R.HD)], 0)
        c = R.LOGIT / self.scale
        q_r = torch.zeros((len(self.qpos), nq, R.HD), dtype=torch.float64)
        for i, t in enumerate(self.qpos.tolist()):
            for h in range(nq):
                kh, pat = h // self.G, self.pattern(h, t)
                if pat == "rising":
                    q_r[i, h] = c * u[kh]
                elif pat == "falling":
                    q_r[i, h] = -c * u[kh]
                elif pat == "two":
                    j = self.needle("split_last", t) if t >= self.tps * R.PAGE else 0
                    q_r[i, h] = c * (n[t, kh] + n[j, kh])
                else:
                    q_r[i, h] = c * n[self.needle(pat, t), kh]
        pos = torch.arange(L)
        self.k_in = R.rnd_dtype(R.rope(k_r, pos, cfg.rope_theta, inverse=True), dtype)
        self.v = R.rnd_dtype(v, dtype)
        q_all = torch.cat([uni(gs, P, nq, R.HD), uni(g, L - P, nq, R.HD)], 0)
        q_all[torch.as_tensor(self.qpos)] = R.rope(q_r, self.qpos, cfg.rope_theta, inverse=True)
        self.q_in = R.rnd_dtype(q_all, dtype)
        self.k = R.rnd_dtype(R.rope(self.k_in, pos, cfg.rope_theta), dtype)
        self.q = R.rnd_dtype(R.rope(self.q_in[torch.as_tensor(self.qpos)], self.qpos, cfg.rope_theta), dtype)


_cache = {}


def cases(name, dtype):
    """the scenario's Case per sequence: L = P_z + T positions (every row slot holds data; the launch uses the first R_z)"""
    from streamvln_amd.config import CONFIGS
    key = (name, dtype)
    if key not in _cache:
        cfg_name, T, layout, seqs = SCENARIOS[name]
        cfg = CONFIGS[cfg_name]
        tps, ns = R.decode_split(cfg, R.MAX_POSITIONS), R.MAX_POSITIONS // R.PAGE
        base = 21000 + 97 * sorted(SCENARIOS).index(name)
        out = []
        for z, (P, _) in enumerate(seqs):
            # pattern lists rotated per sequence: the same head takes another pattern in every sequence
            pats = VR.PATTERNS[z % len(VR.PATTERNS):] + VR.PATTERNS[:z % len(VR.PATTERNS)]
            shared = P if layout == "fork" else 0
            out.append(SeqCase(cfg, dtype, P + T, np.arange(P, P + T), pats, base + 1 + z, tps, ns, shared, base))
        _cache[key] = out
    return _cache[key]


def tables(name):
    """page table per sequence in the model's pool (sequence z's own pages: z * NP + i)"""
    _, _, layout, seqs = SCENARIOS[name]
    tabs = [np.arange(z * NP, (z + 1) * NP) for z in range(len(seqs))]
    if layout == "fork":
        q0 = seqs[0][0] // R.PAGE
        for z in range(1, len(seqs)):
            tabs[z][:q0] = tabs[0][:q0]
    return tabs


def _slots(tab, pos):
    pos = np.asarray(pos)
    return torch.as_tensor(tab[pos // R.PAGE] * R.PAGE + pos % R.PAGE)


def _attend(q, qpos, k, v, G, scale):
    """float64 attention of rows q [r, nq, 128] at positions qpos over keys k / v [L, nkv, 128], causal per row"""
    allowed = torch.arange(k.shape[0])[None] <= torch.as_tensor(qpos)[:, None]
    s = torch.einsum("rhd,shd->rhs", q, k.repeat_interleave(G, 1)) * scale
    s = s.masked_fill(~allowed[:, None, :], float("-inf"))
    return torch.einsum("rhs,shd->rhd", torch.nan_to_num(torch.softmax(s, -1)), v.repeat_interleave(G, 1))


def launch(name, dtype, mutant=None):
    """(out [S, T, nq, 128] with NaN in every row the launch does not write, K pool, V pool [S * NP * 64, nkv, 128], written [slots] bool)
    after the context rows, the fork copy and ONE launch.  mutant: None or one of MUTANTS
      table0            sequence z reads and appends through sequence 0's page table
      pos0              sequence z starts at sequence 0's position
      rows0             sequence z takes sequence 0's row count
      q0                sequence z reads sequence 0's q|k|v rows
      part0             the partial stride of z is ignored: every sequence writes sequence 0's partials, and every merge reads them (the
                        last sequence's, in launch order)
      append_shared     the append of a fork sequence goes through sequence 0's table (the shared page)
      zero_rows_append  a sequence with 0 rows appends its first row slot
      append_all_slots  the row slots beyond R_z are appended too"""
    cfg_name, T, layout, seqs = SCENARIOS[name]
    cs, tabs = cases(name, dtype), tables(name)
    cfg = cs[0].cfg
    S, nkv, nq, G = len(seqs), cfg.kv_heads, cfg.q_heads, cfg.q_heads // cfg.kv_heads
    K = torch.full((S * NP * R.PAGE, nkv, R.HD), float(torch.tensor(R.SENTINEL, dtype=dtype).double()), dtype=torch.float64)
    V = K.clone()
    written = torch.zeros(S * NP * R.PAGE, dtype=torch.bool)
    # context: every sequence's own rows (disjoint) or sequence 0's + the copy of the partly filled page (fork)
    for z, (P, _) in enumerate(seqs):
        if P == 0:
            continue
        if layout == "disjoint" or z == 0:
            sl = _slots(tabs[z], np.arange(P))
            K[sl], V[sl], written[sl] = cs[z].k[:P], cs[z].v[:P], True
        elif P % R.PAGE:
            q0 = P // R.PAGE
            pos = np.arange(q0 * R.PAGE, P)
            src, dst = _slots(tabs[0], pos), _slots(tabs[z], pos)
            K[dst], V[dst], written[dst] = K[src], V[src], True
    out = torch.full((S, T, nq, R.HD), float("nan"), dtype=torch.float64)
    use = []
    for z, (P, Rz) in enumerate(seqs):
        src = 0 if mutant == "q0" else z
        pos0 = seqs[0][0] if mutant == "pos0" else P
        rows = seqs[0][1] if mutant == "rows0" else Rz
        tab = tabs[0] if mutant == "table0" else tabs[z]
        use.append((src, pos0, rows, tab))
        app = rows
        if mutant == "zero_rows_append" and rows == 0:
            app = 1
        if mutant == "append_all_slots":
            app = T
        app = min(app, R.MAX_POSITIONS - pos0)
        if app:
            pos = np.arange(pos0, pos0 + app)
            kin = cs[src].k_in[cs[src].qpos[0]:cs[src].qpos[0] + app]
            vin = cs[src].v[cs[src].qpos[0]:cs[src].qpos[0] + app]
            sl = _slots(tabs[0] if mutant == "append_shared" and layout == "fork" else tab, pos)
            K[sl], V[sl], written[sl] = R.rnd_dtype(R.rope(kin, pos, cfg.rope_theta), dtype), vin, True
    for z, (src, pos0, rows, tab) in enumerate(use):
        if rows == 0:
            continue
        qpos = np.arange(pos0, pos0 + rows)
        p0 = int(cs[src].qpos[0])
        q = R.rnd_dtype(R.rope(cs[src].q_in[p0:p0 + rows], qpos, cfg.rope_theta), dtype)
        sl = _slots(tab, np.arange(pos0 + rows))
        out[z, :rows] = _attend(q, qpos, K[sl], V[sl], G, cs[0].scale)
    if mutant == "part0":
        last = max(z for z, u_ in enumerate(use) if u_[2] > 0)
        for z, u_ in enumerate(use):
            if u_[2] > 0:
                out[z, :u_[2]] = out[last, :u_[2]]        # (rows the last sequence did not write: the NaN of the workspace)
    return out, K, V, written


def reference(name, dtype, z):
    """sequence z alone: (out [R_z, nq, 128], tolerance [R_z, nq, 1]) of its Case -- what launch_attention_verify gives for it"""
    Rz = SCENARIOS[name][3][z][1]
    c = cases(name, dtype)[z]
    return c.attend()[:Rz], c.tolerance(q_flips=True)[:Rz]


def mutant_effect(name, dtype, mutant):
    """how far the mutant moves the scenario: (max |out - ref| / tolerance over the written rows (inf where a row appears, vanishes or
    turns NaN), max |K - ref| / roped_k_bound over the slots both write, V rows that differ, slots written by one of the two only)"""
    ref_o, ref_k, ref_v, ref_w = launch(name, dtype)
    out, K, V, W = launch(name, dtype, mutant)
    cfg_name, T, layout, seqs = SCENARIOS[name]
    cs = cases(name, dtype)
    o_ratio = 0.0
    for z, (P, Rz) in enumerate(seqs):
        a, b = out[z], ref_o[z]
        if bool((torch.isnan(a) != torch.isnan(b)).any()):
            o_ratio = float("inf")
            continue
        if Rz:
            tol = cs[z].tolerance(q_flips=True)[:Rz]
            o_ratio = max(o_ratio, float(((a[:Rz] - b[:Rz]).abs() / tol).amax()))
    both = ref_w & W
    eps = R.EPS[dtype]
    k_ratio = float(((K[both] - ref_k[both]).abs() / (ref_k[both].abs() * 2 * eps + 1e-30)).amax()) if bool(both.any()) else 0.0
    v_diff = int((V[both] != ref_v[both]).flatten(1).any(1).sum()) if bool(both.any()) else 0
    return o_ratio, k_ratio, v_diff, int((ref_w != W).sum())
