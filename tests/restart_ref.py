"""Row-by-row reference of a prefill: what `tests/golden/true2_restart.npz` records for its tapped turns and the ONE comparison
every leg uses (the CPU oracle, the planted-defect self-check, the fp32 engine; test infrastructure).

Why rows.  Ids and the final-norm hidden of a turn come from its last row; every other row of a T = 1952 prefill reaches them only
through the softmax over 1952 keys, which dilutes a wrong row to ~1e-6 of the hidden (parity section).  So the fixture
keeps, for each tapped turn t and each decoder layer l (the layer's OUTPUT, all T rows of the prefill call):

  t{t}_L{l}_rows_idx / _rows   full-width fp32 rows.  Restart turn: 8 (tile edges 255 | 256 and 1791 | 1792, first / last row, the
                               first row of the <memory> block, the last row of the image block).  Steady turn: 4 (first, last and 2
                               drawn by seed; 8 would put the file over the 1 MB a fixture may have, and the projections stay whole)
  t{t}_L{l}_proj               fp32 [T, 16]: X.double() @ S with S a [hidden, 16] matrix of +-1, for EVERY row.  Each element of each
                               row enters 16 sums with weight +-1, so a wrong row, column tile or epilogue lane cannot cancel out of
                               all of them.  The signs come from the project's own counter-based generator (no library RNG stream).
  t{t}_L{l}_proj_noise         max |oracle - reference| over that projection, measured by the generator: the scale of legitimate fp32
                               re-ordering between two correct implementations.
  t{t}_K1_rows                 post-RoPE K rows of layer 1 for the selected rows, from the reference's cache object, [rows, kv_dim]

Bounds.  Selected rows: elementwise HIDDEN_TOL = 1e-3, the project's fp32 bar; unscaled it is meaningful here (row RMS of these
tensors 0.29 - 0.83, largest element 3.1, oracle - reference <= 4.1e-6).  Projections: every row within PROJ_FACTOR x proj_noise.
PROJ_FACTOR = 32: the fp32 engine sums in yet another order than either CPU implementation (split-K, MFMA blocks); its record
against the reference is <= 1.3e-5 on the hidden at depth 28, a few times what the two CPU implementations differ by here
(<= 4.1e-6).  With proj_noise 1.05e-4 (layer 0) and 1.76e-4 (layer 1) the bounds are ~3.4e-3 and ~5.6e-3; one row scaled by
1 + 1e-3 moves its projections by 0.053 / 0.074 and a 32-row x 128-column tile scaled by 1 + 2^-8 by 0.026 / 0.049: 7 to 13 times the
bound (tests/test_oracle_golden.py plants them, and a row swap, and requires the helper to reject each)."""
import numpy as np

from streamvln_amd import weights as Wt

HIDDEN_TOL = 1e-3
PROJ_FACTOR = 32
N_PROJ = 16
N_SEL_RESTART, N_SEL_STEADY = 8, 4
IMAGE_TOKEN_INDEX, MEMORY_TOKEN_INDEX = -200, -300

_signs = {}


def sign_matrix(hidden):
    """S [hidden, 16] of +-1 (float64): the sign of the project's counter-based stream `probe.signs` under seed 99"""
    s = _signs.get(hidden)
    if s is None:
        v = Wt.synth_flat(Wt.tensor_seed(99, "probe.signs"), 0, hidden * N_PROJ, 1.0, 0.0)
        s = _signs[hidden] = np.where(v >= 0, 1.0, -1.0).reshape(hidden, N_PROJ)
    return s


def project(x):
    """fp32 [T, hidden] -> [T, 16] in float64"""
    x = np.asarray(x, dtype=np.float64)
    return x @ sign_matrix(x.shape[1])


def block_rows(input_ids, pool_tokens, memory_rows):
    """(first row of the <memory> block or None, last row of the last image block or None, row count) of a turn's spliced rows"""
    row, mem0, img_last = 0, None, None
    for t in input_ids:
        t = int(t)
        if t == IMAGE_TOKEN_INDEX:
            row += pool_tokens
            img_last = row - 1
        elif t == MEMORY_TOKEN_INDEX:
            mem0 = row
            row += memory_rows
        else:
            row += 1
    return mem0, img_last, row


def select_rows(T, input_ids, pool_tokens, memory_rows, seed):
    """the rows a tapped turn keeps at full width (generator side; the fixture records the choice in `_rows_idx`)"""
    mem0, img_last, rows = block_rows(input_ids, pool_tokens, memory_rows)
    skip = rows - T                         # a steady turn's first ids were fed by the previous turn's decode steps: not prefill rows
    assert 0 <= skip < 8, (rows, T)
    if mem0 is not None:                    # the restart turn: tile edges of the 256-row tiling, ragged last tile included
        sel = [0, 255, 256, T - 161, T - 160, T - 1, mem0 - skip, img_last - skip]
        assert (T - 160) % 256 == 0 and len(set(sel)) == N_SEL_RESTART, sel
    else:
        rng = np.random.default_rng(seed)
        sel = [0, T - 1] + sorted(int(i) for i in rng.choice(np.arange(1, T - 1), N_SEL_STEADY - 2, replace=False))
    return np.asarray(sel, dtype=np.int64)


def compare_rows(g, t, layer, got):
    """`got` (fp32 [T, hidden], the output of decoder layer `layer` on all rows of turn t's prefill) against the fixture `g`.
    Returns the measured figures; raises AssertionError naming the worst row where a bound is missed."""
    key = f"t{t}_L{layer}_"
    got = np.asarray(got, dtype=np.float32)
    ref_proj = g[key + "proj"]
    assert got.shape[0] == ref_proj.shape[0], (key, "rows", got.shape, ref_proj.shape)
    idx = g[key + "rows_idx"]
    sel_err = np.abs(got[idx].astype(np.float64) - g[key + "rows"].astype(np.float64)).max(1)
    row_err = np.abs(project(got) - ref_proj.astype(np.float64)).max(1)
    bound = PROJ_FACTOR * float(g[key + "proj_noise"])
    worst = int(row_err.argmax())
    out = dict(sel_err=float(sel_err.max()), proj_err=float(row_err.max()), proj_bound=bound, proj_row=worst,
               proj_ratio=float(row_err.max()) / bound, bad_rows=int((row_err > bound).sum()))
    assert np.isfinite(got).all(), (key, "non-finite values")
    assert out["sel_err"] <= HIDDEN_TOL, (key, "selected row", int(idx[sel_err.argmax()]), out["sel_err"])
    assert out["proj_err"] <= bound, (key, "projection of row", worst, out["proj_err"], "bound", bound, "rows over", out["bad_rows"])
    return out


def compare_k_rows(g, t, layer, got_k, tol=HIDDEN_TOL):
    """post-RoPE K rows of the selected rows ([rows, kv_dim]) against `t{t}_K{layer}_rows`; returns the largest error"""
    ref = g[f"t{t}_K{layer}_rows"]
    err = float(np.abs(np.asarray(got_k, dtype=np.float64) - ref.astype(np.float64)).max())
    assert err <= tol, (f"t{t}_K{layer}_rows", err)
    return err
