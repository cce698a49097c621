"""References for draft-verified greedy decode (svln_set_speculative), on top of tests/attn_ref.py:
  * the verify attention: one env, `rows` consecutive query positions P .. P + rows - 1 whose K / V rows the launch appends itself, each
    row roped and masked at its own position, through the decode split-KV scheme.  Cases are attn_ref.Case objects; four mutants beside
    attn_ref's describe the mistakes only a multi-row pass can make;
  * the verify rule and the host policy, restated in Python: verify_step (one pass on given row tokens / arg-maxes) and simulate (a whole
    turn: emitted ids and the three counters of svln_draft_stats)."""
import numpy as np
import torch

import attn_ref as R

PATTERNS = ["newest", "next", "rising", "sink", "tile_last", "falling", "two", "tile_first"]
#: (cfg name, rows per pass): TINY has G = 2 (rows <= 8 ... 16 query rows), the true width G = 7 (rows <= 4 ... 28 of the 32 rows)
CASES = [("tiny", 8), ("tiny", 4), ("true_dims_1layer", 4), ("true_dims_1layer", 2)]
VERIFY_MUTANTS = ["shared_pos", "all_visible", "stale_mid", "last_row_only"]


def positions(rows, max_positions=R.MAX_POSITIONS):
    """first positions P of the verify cases: the start, every way of straddling the first page boundary, a far page, the last rows"""
    return [0, 1, 60, 61, 62, 63, 64, 700, max_positions - rows]


def all_cases():
    return [(cfg, rows, P) for cfg, rows in CASES for P in positions(rows)]


def verify_case(cfg, dtype, P, rows, max_positions=R.MAX_POSITIONS):
    return R.Case(cfg, dtype, P + rows, np.arange(P, P + rows), PATTERNS, seed=11000 + 31 * P + rows,
                  tps=R.decode_split(cfg, max_positions), nsplit=max_positions // R.PAGE)


def mutants(case):
    """the mutants that apply to a verify case (rows >= 2, so the last row always sees an earlier key)"""
    m = ["drop_newest", "admit_masked", "diag_shift", "rope_off", "stale_k"]
    if case.L > case.tps * R.PAGE:            # a second split exists
        m.append("drop_split")
    return m + VERIFY_MUTANTS


def attend(case, mutant=None, device="cpu"):
    """Case.attend for attn_ref's mutants; the verify-specific ones:
      shared_pos      every row roped and masked at the first position P (the decode kernel's one position for all rows)
      all_visible     no causal mask among the new rows: every row sees all P + rows keys
      stale_mid       the K row of the second new position not appended (stale pool data)
      last_row_only   only the last new row's K / V appended (the single-step append)"""
    if mutant not in VERIFY_MUTANTS:
        return case.attend(mutant=mutant, device=device)
    L, G = case.L, case.G
    qpos = torch.as_tensor(case.qpos)
    P = int(case.qpos[0])
    q, k, v = case.q, case.k.clone(), case.v.clone()
    keys = torch.arange(L)
    allowed = keys[None] <= qpos[:, None]
    if mutant == "shared_pos":
        q = R.rnd_dtype(R.rope(case.q_in[qpos], np.full(len(case.qpos), P), case.cfg.rope_theta), case.dtype)
        allowed = (keys[None] <= P).expand(len(case.qpos), L)
    elif mutant == "all_visible":
        allowed = torch.ones((len(case.qpos), L), dtype=torch.bool)
    elif mutant == "stale_mid":
        k[P + 1] = R.SENTINEL
    elif mutant == "last_row_only":
        k[P:L - 1] = R.SENTINEL
        v[P:L - 1] = R.SENTINEL
    q, k, v, allowed = q.to(device), k.to(device), v.to(device), allowed.to(device)
    s = torch.einsum("rhd,shd->rhs", q, k.repeat_interleave(G, 1)) * case.scale
    s = s.masked_fill(~allowed[:, None, :], float("-inf"))
    return torch.einsum("rhs,shd->rhd", torch.nan_to_num(torch.softmax(s, -1)), v.repeat_interleave(G, 1))


def mutant_ratios(case, device="cpu"):
    """{mutant: max over elements of |mutant - reference| / tolerance} with the tolerance the GPU test applies (q_flips: the kernel ropes
    q in registers)"""
    ref = case.attend(device=device)
    tol = case.tolerance(q_flips=True, device=device)
    return {m: float(((attend(case, m, device) - ref).abs() / tol).amax()) for m in mutants(case)}


# ------------------------------------------------------------------------------------------------------------ the rule
def usable_draft(draft, vocab=None):
    """the draft up to the first id outside [0, vocab)"""
    out = []
    for t in draft:
        if t < 0 or (vocab is not None and t >= vocab):
            break
        out.append(int(t))
    return out


def pass_rows(rows, dlen, c, max_new, room):
    """rows a verify pass carries with c tokens emitted: row 0 feeds the last token at position L + c - 1, row i the guess D[c + i - 1]
    at L + c - 1 + i.  Fewer than `rows` when the draft (dlen usable ids) runs out, when max_new leaves room for fewer tokens, or when a
    row would reach max_positions (room = max_positions - L positions are left for fed tokens)."""
    return max(min(rows, max(dlen - c + 1, 1), max_new - c, room - (c - 1)), 0)


def verify_step(fed, cand, count, max_new, eos):
    """one verify step on the rows' fed tokens and arg-maxes -> (new count, done, emitted ids, next token or None).  cand[0] is always
    emitted; cand[i] iff every earlier row was emitted without stopping and cand[i - 1] == fed[i].  Stops: an EOS id (appended), the
    max_new-th token, a non-finite arg-max (-1)."""
    emitted, done = [], False
    for i, tok in enumerate(cand):
        if i > 0 and cand[i - 1] != fed[i]:
            break
        emitted.append(int(tok))
        if tok < 0 or count + len(emitted) >= max_new or tok in eos:
            done = True
            break
    return count + len(emitted), done, emitted, (emitted[-1] if emitted else None)


def simulate(true_ids, draft, rows, max_new, eos, room, vocab=None):
    """A whole turn under the verify rule and the host policy.  true_ids: what plain greedy decoding emits (at least as many ids as the
    turn needs; a row fed the true prefix has the true next id as its arg-max, any other row's arg-max is never used).  draft: the
    caller's guess of the turn's ids (index 0 included), rows: 0 = mode off.  Returns (ids, verify_passes, tokens_from_verify,
    single_steps).  Policy: after the prefill's token, a verify pass runs while the draft has a guess for the next token (c < len(D)) and
    a position is left, even where max_new or room cut it to one row; after each the next one follows only if every emitted id from
    index 1 on equals the draft; otherwise single steps finish the turn."""
    eos = set(eos)
    D = usable_draft(draft, vocab)
    out = [int(true_ids[0])]
    done = out[0] < 0 or 1 >= max_new or out[0] in eos
    passes = vtok = single = 0
    if rows and len(D) >= 2:
        while not done:
            c = len(out)
            r = pass_rows(rows, len(D), c, max_new, room)
            if c >= len(D) or r < 1:
                break
            fed = [out[-1]] + [D[c + i - 1] for i in range(1, r)]
            cand, ok = [], True
            for i in range(r):                      # arg-max of row i: the true id while every fed token so far is the true one
                ok = ok and (i == 0 or fed[i] == true_ids[c + i - 1])
                cand.append(int(true_ids[c + i]) if ok and c + i < len(true_ids) else -7)       # (rows past the turn's end are never used)
            _, done, emitted, _ = verify_step(fed, cand, c, max_new, eos)
            assert -7 not in emitted
            out += emitted
            passes += 1
            vtok += len(emitted)
            if not all(out[k] == D[k] for k in range(1, min(len(out), len(D)))):
                break
    while not done:
        c = len(out)
        assert room - (c - 1) > 0, "sequence exceeds max_positions during decode"
        tok = int(true_ids[c])
        out.append(tok)
        single += 1
        done = tok < 0 or len(out) >= max_new or tok in eos
    return out, passes, vtok, single
