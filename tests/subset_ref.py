"""CPU case builder, float64 reference and fp32 restatement of the allowed-token lm_head (svln_set_allowed_tokens): gemv_subset_kernel and
subset_logprobs_kernel of streamvln_amd/csrc/gemv_subset.hip behind the unchanged final kernels, as svln_op_subset_argmax runs them.  Test
infrastructure, modelled on tests/scores_ref.py and tests/sample_ref.py, whose merge and Philox noise it reuses.

    x_{a_j}(b) = W[a_j, :] . x[b, :]           (fp32; one wave per listed id, lane l owns the chunks l, l + 64, ..; wave_sum butterfly)
    y = penalty(x) [* invT]                     (flag of the VOCABULARY id a_j, in the flag row pen_rows[b])
    token = argmax_j (y_j [+ G(seed, stream_b, draw_b, a_j)]), lowest id on ties, -1 when nothing is finite
    dist[b][j] = y_j - logsumexp_i y_i,  score = dist[b][token]

Exact inputs.  Every element of W and x is an integer of [-4, 4] (exact in bf16), so every product and every partial sum is an integer
below 2^24 at K <= 3584 and the fp32 logit is exact in ANY summation order.  Every logit is DESIGNED: activation row b owns the two
columns K - 2B + 2b, + 1 (x = 4 and 1 there, 0 in the other rows' pairs), in which weight row a spells L[b][a] = 4 w0 + w1, |L| <= 20; the
columns before them hold (w, -w) against equal activations and cancel exactly.  The designed columns are the LAST of the row, so the
last iteration of the lanes carries them.  Weight rows outside the list, and the ldw / ldx padding, are NaN: nothing of them may show.
What is left to tolerance is the log-sum-exp alone (TOL, the bound of tests/test_scores_gpu.py for the same merge).

Sharp placement.  Greedy cases: the top T sits mid-list, the runner-up T - 1 at the LAST list position (a dropped tail id changes the
sums by e^-1), the background 2 .. 8 below.  Penalised cases flag (a) the vocabulary id of an entry that would win un-penalised and
carries e^-1 penalised, (b) the vocabulary id EQUAL TO the top's list position: a kernel that indexes the flags by position halves the
top.  Sampled cases are flat (background 0 .. 3 below the top) so that the noise decides, and every row has its own stream and draw.

Mutants: the restatement with one plausible kernel mistake each; tests/test_subset_inputs.py proves each changes a token or moves a value
by >= 100 x TOL on at least one case, while the correct restatement stays inside TOL.
"""
import functools

import numpy as np
import torch

import sample_ref as R
import scores_ref as S
from util import load_golden

TOL = S.TOL                 # |logprob - float64| and |allowed_logprobs - float64| (tests/test_scores_gpu.py's bound for the same merge)
PEN = 2.0
V = 1024
F = np.float32
NEG = F(-np.inf)
NONE = 0x7FFFFFFF
WAVES = 4                   # listed ids per workgroup (GEMV_SUBSET_WAVES)
EPC = {"fp32": 4, "bf16": 8}
MUTANTS = ("w_row_j", "noise_col_j", "flag_j", "tie_highest", "drop_last_k_iter", "drop_tail_ids", "ldx_ignored", "ldw_ignored", "x_row0",
           "stream_row0", "stale_partials", "ninf_wins", "dist_on_z")


def k_ladder(fmt):
    """one lane, one lane idle, a full wave, one lane in a second iteration (all in chunks), and the true width"""
    e = EPC[fmt]
    return (e, 63 * e, 64 * e, 65 * e, 3584)


class Case:
    """B activation rows against the list `ids` (n of V = 1024).  T = 0: greedy; else sampled at temperature T with streams / draws [B].
    special: None, "ninf_all" (every allowed logit of the only row is -inf) or "ninf_one" (one allowed logit is -inf)."""

    def __init__(self, fmt, K, n, B, pen=False, tie=False, T=0.0, seed=0, special=None, pad=(16, 24)):
        assert K >= 2 * B and K % EPC[fmt] == 0, (K, B)
        self.fmt, self.K, self.n, self.B, self.pen, self.tie, self.T, self.seed, self.special = fmt, K, n, B, pen, tie, float(T), seed, special
        self.ldw, self.ldx = K + pad[0], K + pad[1]
        self.inv_t = F(1.0) / F(T) if T else F(1.0)
        self.streams = [(3 * b + 1) % 8 for b in range(B)]
        self.draws = [(7 * b + seed) % 1000 for b in range(B)]
        self.id = (f"{fmt}-K{K}-n{n}-B{B}" + ("-pen" if pen else "") + ("-tie" if tie else "") + (f"-T{T:g}" if T else "") +
                   (f"-{special}" if special else ""))

    @functools.lru_cache(maxsize=None)
    def ids(self):
        g = np.random.default_rng(1000 + self.seed)
        if self.n == 1:
            return np.array([V - 1 if self.T else 0], dtype=np.int64)
        mid = g.choice(np.arange(1, V - 1), size=self.n - 2, replace=False)
        return np.sort(np.concatenate([[0, V - 1], mid])).astype(np.int64)

    def pen_rows(self):
        return [(5 * b + 1) % self.B for b in range(self.B)] if self.pen else None

    def tops(self):
        return [4 + (b % 7) for b in range(self.B)]

    def heavy(self, b):
        """list positions of row b's top, runner-up (last position) and penalised heavy entry"""
        n = self.n
        if n == 1:
            return {"top": 0}
        h = {"top": (n // 2 + b) % (n - 1), "up": n - 1}
        if n >= 3:
            h["pen"] = (h["top"] + 1) % (n - 1)
        return h

    @functools.lru_cache(maxsize=None)
    def logits(self):
        """(L [B][n] float64 raw designed logits, flags [B][V] uint8 or None)"""
        g = np.random.default_rng(2000 + self.seed)
        B, n = self.B, self.n
        tops = np.array(self.tops(), dtype=np.float64)
        if self.T:
            L = tops[:, None] - g.integers(0, 4, size=(B, n)).astype(np.float64)
        else:
            L = tops[:, None] - 2 - g.integers(0, 7, size=(B, n)).astype(np.float64)
        flags = np.zeros((B, V), dtype=np.uint8) if self.pen else None
        ids, rows = self.ids(), self.pen_rows()
        for b in range(B):
            h = self.heavy(b)
            if not self.T:
                L[b, h["top"]] = tops[b]
                if "up" in h:
                    L[b, h["up"]] = tops[b] if self.tie else tops[b] - 1
            if self.pen:
                fr = flags[rows[b]]
                fr[g.choice(V, size=8, replace=False)] = 1                      # mostly ids outside the list: nothing may come of them
                fr[ids] = 0
                if h["top"] not in ids:                                         # (b) the top's list position as a vocabulary id
                    fr[h["top"]] = 1
                if "pen" in h and not self.T:                                   # (a) wins un-penalised, e^-1 penalised
                    fr[ids[h["pen"]]] = 1
                    L[b, h["pen"]] = 2 * (tops[b] - 1)
                elif "pen" in h:
                    fr[ids[h["pen"]]] = 1
        assert np.abs(L).max() <= 20
        return L, flags

    @functools.lru_cache(maxsize=None)
    def operands(self):
        """(W [V][ldw], x [B][ldx]) float64 holding exact values; NaN in the rows outside the list and in the padding"""
        g = np.random.default_rng(3000 + self.seed)
        L, _ = self.logits()
        B, n, K = self.B, self.n, self.K
        ids = self.ids()
        nf = K - 2 * B
        x = np.full((B, self.ldx), np.nan)
        W = np.full((V, self.ldw), np.nan)
        x[:, :K] = 0.0
        pairs = g.choice([-4, -3, -2, -1, 1, 2, 3, 4], size=(B, nf // 2)).astype(np.float64)
        x[:, :nf] = np.repeat(pairs, 2, axis=1)
        half = g.integers(-4, 5, size=(n, nf // 2)).astype(np.float64)
        Wl = np.zeros((n, K))
        Wl[:, 0:nf:2] = half
        Wl[:, 1:nf:2] = -half
        for b in range(B):
            x[b, nf + 2 * b], x[b, nf + 2 * b + 1] = 4.0, 1.0
            w0 = np.round(L[b] / 4)
            Wl[:, nf + 2 * b], Wl[:, nf + 2 * b + 1] = w0, L[b] - 4 * w0
        assert np.abs(Wl).max() <= 4
        if self.special == "ninf_all":
            Wl[:, nf] = -np.inf
        elif self.special == "ninf_one":
            Wl[n // 2, nf] = -np.inf
        W[ids, :K] = Wl
        return W, x

    def raw(self):
        """float64 raw logits incl. the special -inf entries"""
        L = self.logits()[0].copy()
        if self.special == "ninf_all":
            L[0, :] = -np.inf
        elif self.special == "ninf_one":
            L[0, self.n // 2] = -np.inf
        return L

    # ------------------------------------------------------------------------------------------------ float64 reference
    def noise64(self):
        ids = self.ids()
        return np.stack([R.gumbel(self.seed, self.streams[b], self.draws[b], ids) for b in range(self.B)])

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """(tokens [B], scores [B], y [B][n], dist [B][n], margins [B]) in float64; margin = top-2 gap of the compared values (inf for n = 1)"""
        L, (_, flags) = self.raw(), self.logits()
        ids = self.ids()
        y = L.copy()
        if flags is not None:
            f = flags[self.pen_rows()][:, ids].astype(bool)
            y = np.where(f, np.where(L < 0, L * PEN, L / PEN), L)
        y = y * float(self.inv_t)
        z = y + self.noise64() if self.T else y
        toks, scores, margins = [], [], []
        with np.errstate(all="ignore"):
            m = y.max(1, keepdims=True)
            lse = m + np.log(np.exp(y - m).sum(1, keepdims=True))
            dist = y - lse
        for b in range(self.B):
            zz = z[b]
            if not (zz > -np.inf).any():
                toks.append(-1); scores.append(float("nan")); margins.append(float("inf"))
                continue
            j = int(np.flatnonzero(zz == zz.max())[0])
            rest = np.delete(zz, j)
            toks.append(int(ids[j])); scores.append(float(dist[b, j]))
            margins.append(float(zz[j] - rest.max()) if rest.size else float("inf"))
        return toks, scores, y, dist, margins

    # ------------------------------------------------------------------------------------------------ fp32 restatement
    def restate(self, mut=None):
        """(tokens, scores, y [B][n] fp32, dist [B][n] fp32) as the kernels compute them, with the mistake `mut`"""
        W, x = self.operands()
        B, n, K, e = self.B, self.n, self.K, EPC[self.fmt]
        ids = self.ids()
        Wf, xf = W.astype(F).ravel(), x.astype(F).ravel()
        sw = K if mut == "ldw_ignored" else self.ldw
        sx = K if mut == "ldx_ignored" else self.ldx
        rows = np.arange(n) if mut == "w_row_j" else ids
        Wl = np.stack([Wf[r * sw: r * sw + K] for r in rows])
        X = np.stack([xf[(0 if mut == "x_row0" else b) * sx: (0 if mut == "x_row0" else b) * sx + K] for b in range(B)])
        nch = K // e
        iters = (nch + 63) // 64
        Wp = np.zeros((n, iters * 64 * e), dtype=F); Wp[:, :K] = Wl
        Xp = np.zeros((B, iters * 64 * e), dtype=F); Xp[:, :K] = X
        Wp, Xp = Wp.reshape(n, iters, 64, e), Xp.reshape(B, iters, 64, e)
        with np.errstate(all="ignore"):
            acc = np.zeros((B, n, 64), dtype=F)
            for it in range(iters):
                if mut == "drop_last_k_iter" and it == iters - 1:
                    continue
                live = (it * 64 + np.arange(64)) < nch                          # lanes past the row's last chunk do not run the iteration
                for q in range(e):
                    prod = (Xp[:, it, :, q][:, None, :] * Wp[:, it, :, q][None, :, :]).astype(F)
                    acc = np.where(live[None, None, :], (acc + prod).astype(F), acc)
            o = 32
            while o:                                                            # wave_sum: v += shfl_xor(v, o)
                acc = (acc + acc[:, :, np.arange(64) ^ o]).astype(F)
                o //= 2
            v = acc[:, :, 0]
            _, flags = self.logits()
            if flags is not None:
                fcol = np.arange(n) if mut == "flag_j" else ids
                f = flags[self.pen_rows()][:, fcol].astype(bool)
                v = np.where(f, np.where(v < 0, v * F(PEN), v / F(PEN)), v).astype(F)
            y = (v * self.inv_t).astype(F) if self.T else v
            if self.T:
                ncol = np.arange(n) if mut == "noise_col_j" else ids
                g = np.stack([R.gumbel(self.seed, self.streams[0 if mut == "stream_row0" else b], self.draws[0 if mut == "stream_row0" else b], ncol)
                              for b in range(B)]).astype(F)
                z = (y + g).astype(F)
            else:
                z = y
            toks, scores = [], []
            keep = n - n % WAVES if mut == "drop_tail_ids" and n > WAVES else n
            for b in range(B):
                parts = []
                for j in range(keep):
                    val, yy = z[b, j], y[b, j]
                    own = val > NEG or (mut == "ninf_wins" and val == NEG)
                    idx = int(ids[j]) if own else NONE
                    if mut == "tie_highest" and own:
                        idx = 2 * V - idx                                       # the merge keeps the lowest index: mirror the ids to invert the tie rule
                    s = F(0) if yy == NEG else (yy if np.isnan(yy) else F(1))
                    parts.append((val, idx, yy, yy, s))
                if mut == "stale_partials" and n % WAVES:
                    parts.append((F(100), 5, F(100), F(100), F(1)))
                if self.T:
                    z_, i_, raw_, Vm, S_ = R._merge(parts, None)
                    tok = -1 if i_ == NONE else i_
                    sc = float("nan") if tok < 0 else float(F(F(raw_ - Vm) - np.log(S_, dtype=F)))
                else:
                    tok, sc = S._final([(p[0], p[4], p[1]) for p in parts], None)
                if mut == "tie_highest" and tok >= 0:
                    tok = 2 * V - tok
                toks.append(tok); scores.append(sc)
            t = z if mut == "dist_on_z" else y
            m = np.max(np.where(np.isnan(t), NEG, t), axis=1, keepdims=True)
            s = np.where(t == NEG, F(0), np.exp((t - m).astype(F), dtype=F)).astype(F).sum(1, keepdims=True, dtype=F)
            dist = (t - (m + np.log(s, dtype=F)).astype(F)).astype(F)
        return toks, scores, y, dist


N_LADDER = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256)
B_LADDER = (1, 2, 3, 8, 32)


def cases(fmt):
    """every K of the ladder, every n, every B at least once; greedy plain / tie / penalty and the three temperatures"""
    ks = k_ladder(fmt)
    out = []
    for i, n in enumerate(N_LADDER):
        K = ks[i % len(ks)]
        Bs = [b for b in B_LADDER if 2 * b <= K]
        B = Bs[(i * 2 + 1) % len(Bs)]
        out.append(Case(fmt, K, n, B, pen=i % 2 == 1 and n >= 3, tie=i % 3 == 0 and n >= 2, seed=10 + i))
        K2 = ks[(i + 2) % len(ks)]
        Bs2 = [b for b in B_LADDER if 2 * b <= K2]
        out.append(Case(fmt, K2, n, Bs2[(i + 2) % len(Bs2)], pen=i % 2 == 0 and n >= 3, T=R.TEMPS[i % 3], seed=40 + i))
    for j, K in enumerate(ks):                                                  # every K with the largest B it holds, n off the workgroup multiple
        Bs = [b for b in B_LADDER if 2 * b <= K]
        out.append(Case(fmt, K, 7 if j % 2 else 9, Bs[-1], pen=True, seed=70 + j))
        out.append(Case(fmt, K, 5, Bs[-1], T=1.0, pen=j % 2 == 0, seed=80 + j))
    out.append(Case(fmt, ks[1], 6, 1, seed=90, special="ninf_all"))
    out.append(Case(fmt, ks[3], 6, 1, seed=91, special="ninf_one"))
    out.append(Case(fmt, ks[3], 6, 1, T=1.0, seed=92, special="ninf_one"))
    return out


def all_cases():
    return cases("fp32") + cases("bf16")


# ---------------------------------------------------------------------------------------------------------- end-to-end inputs
REMOVED = {"tiny_episode": 153, "tiny_penalty": 1507}          # the emitted id taken out of the allowed set in the exclusion runs
PATHS_A = (153, 1025, 1507, 1687, 2693, 2731, 3912, 4003)      # a constant list of ids the two tiny fixtures emit; 1025 and 2693 are EOS ids of tiny_episode


def fixture_ids(name):
    g = load_golden(name)
    return [g[f"t{t}_ids"].tolist() for t in range(int(g["n_turns"]))]


def allowed_set(name):
    """the sorted set of every id the fixture emits"""
    return sorted({i for t in fixture_ids(name) for i in t})


def restricted_rows(Wd, A, hidden, ids, penalty=1.0):
    """float64, per emitted token: (y [n] processed logits over the list A, dot bound 2 gamma_K max_a sum_k |w_ak h_k|) from the final-norm
    rows `hidden`; penalty over the ids generated so far in the turn.  Wd: the lm_head [V][K] as a float64 tensor."""
    A = list(A)
    WA = Wd[torch.tensor(A, dtype=torch.long)]
    gamma = Wd.shape[1] * 2.0 ** -24
    out = []
    for k in range(min(len(ids), len(hidden))):
        h = torch.from_numpy(np.asarray(hidden[k], dtype=np.float64))
        y = WA @ h
        if penalty != 1.0 and k:
            seen = torch.tensor(sorted({A.index(i) for i in ids[:k] if i in A}), dtype=torch.long)
            y[seen] = torch.where(y[seen] < 0, y[seen] * penalty, y[seen] / penalty)
        out.append((y.numpy(), 2 * gamma * float((WA.abs() @ h.abs()).max())))
    return out
