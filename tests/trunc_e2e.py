"""The end-to-end oracle of truncated sampling, shared by tests/test_trunc_e2e_gpu.py (on the engine's own tap rows) and
tests/test_trunc_inputs.py (on the fixtures' recorded hidden rows: the proof that the settings below exempt at most 10 % of the tokens).
Test infrastructure.

restate_token: float64 logits l = W h of one hidden row, the penalty, y = l / T, top-k, top-p over the top-k set, the pick with the
float64 noise, the renormalised log-softmax.  A token is checked only where three gaps exceed the a-priori error of the engine's fp32
dot products, dot = 2 gamma_K max_n sum_k |w_nk h_k| / T with gamma_K = K 2^-24 (the bound of tests/test_scores_e2e_gpu.py):

    * the two best perturbed values among the kept:   z_a - z_b          > 2 dot + tol_z   (tol_z: tests/sample_ref.py);
    * the k-th against the (k+1)-th value:            y_{k-1} - y_k      > 2 dot;
    * every prefix against the nucleus bound:         |c_{j-1} - p total| > 2 dot (c_{j-1} + p total) + 2^-20 total
      (e_i = exp(y_i - y_0) moves by at most a factor exp(+-2 dot), i.e. 2 dot e_i to first order; 2^-20 total: tests/trunc_ref.py).

SETTINGS: (top_k, top_p, T, seeds); the share of exempted tokens is taken over the setting's three seeds together.  These heads are
random-initialised, so a row's best logits lie close together (the 8th and the 9th of 4096 often closer than 2 dot ~ 2e-3): top_k = 8
and top_p = 0.55 over 8 exempt 2 to 6 of a fixture's 14 / 24 rows whatever the seed, measured on the fixtures' own rows, and are left to
the op-level tests and to the path-agreement tests, which need no oracle.  Chosen: (5, 1) the top-k cut alone; (5, 0.5) at T = 2, where
e ~ (1, .99, .98, .97, .96) and the bound 0.5 x 4.9 = 2.45 lies between c_1 ~ 1.99 and c_2 ~ 2.97: the nucleus drops two entries on
every row, decisively; (4, 0.64) at T = 2 likewise drops one; (2, 0.9) at T = 1/2 keeps both."""
import numpy as np
import torch

import sample_ref as SR
from scenarios import SCENARIOS, SEED
from util import synth_weights

FIXTURES = ("tiny_episode", "tiny_penalty")
SETTINGS = ((5, 1.0, 1.0, (0xC0FFEE70, 0xC0FFEE71, 0xC0FFEE72)), (5, 0.5, 2.0, (0xC0FFEE73, 0xC0FFEE74, 0xC0FFEE75)),
            (4, 0.64, 2.0, (0xC0FFEE76, 0xC0FFEE77, 0xC0FFEE78)), (2, 0.9, 0.5, (0xC0FFEE79, 0xC0FFEE7A, 0xC0FFEE7B)))
LSE_TOL = 2e-5


def fixture_head(name):
    """float64 lm_head of the fixture's synthetic model"""
    sd = synth_weights(SCENARIOS[name]["cfg"], SEED)
    return torch.from_numpy(np.asarray(sd["lm_head.weight"])).double()


def restate_token(Wd, h, seen, penalty, k, p, T, seed, stream, draw, stats):
    """-> (token or None when a gap is under the bound, the kept columns in list order, float64 log-probabilities of the kept, dot,
    whether the two gaps that decide the kept SET are clear).  stats["tokens"] / stats["under"] count."""
    K = Wd.shape[1]
    h = torch.from_numpy(np.asarray(h, dtype=np.float64))
    l = Wd @ h
    if penalty != 1.0 and len(seen):
        s = torch.tensor(sorted(set(seen)), dtype=torch.long)
        l[s] = torch.where(l[s] < 0, l[s] * penalty, l[s] / penalty)
    inv_t = float(np.float32(1.0) / np.float32(T))
    y = l.numpy() * inv_t
    dot = 2 * (K * 2.0 ** -24) * float((Wd.abs() @ h.abs()).max()) * inv_t
    order = np.lexsort((np.arange(len(y)), -y))[:k + 1]
    top, nxt = order[:k], order[k]
    yt = y[top]
    e = np.exp(yt - yt[0])
    cum = np.cumsum(e)
    total = cum[-1]
    keep = [0] + [j for j in range(1, k) if p >= 1.0 or cum[j - 1] < p * total]
    ok = yt[-1] - y[nxt] > 2 * dot
    if p < 1.0:
        ok = ok and all(abs(cum[j - 1] - p * total) > 2 * dot * (cum[j - 1] + p * total) + 2.0 ** -20 * total for j in range(1, k))
    set_ok = bool(ok)
    cols = top[keep]
    g = SR.gumbel(seed, stream, draw, cols)
    z = yt[keep] + g
    o = np.lexsort((cols, -z))
    a = int(o[0])
    if len(keep) > 1:
        b = int(o[1])
        tol = 2.0 ** -17 * max(1.0, abs(g[a]), abs(g[b])) + 2.0 ** -22 * float(np.abs(z).max())
        ok = ok and z[a] - z[b] > 2 * dot + tol
    yk = yt[keep]
    lps = yk - (yk.max() + np.log(np.exp(yk - yk.max()).sum()))
    stats["tokens"] += 1
    if not ok:
        stats["under"] += 1
    return (int(cols[a]) if ok else None), [int(c) for c in cols], lps, dot, set_ok
