"""The host policy of drafts inside the prefill pass (svln_set_prefill_draft), restated in Python on top of verify_ref: how many draft
rows a ride feeds, what the ride emits (verify_ref.verify_step from zero emitted tokens), and how the turn goes on -- verify passes
while the draft holds (svln_set_speculative), single steps otherwise.  simulate gives the emitted ids and the counters of
svln_prefill_draft_stats followed by those of svln_draft_stats."""
import verify_ref as VR

RIDE_MAX_ROWS = 7          # fed draft rows per ride: the verify step holds 8 head rows
#: one mistake per cap of ride_rows: the cap is left out
MUTANTS = ["no_dlen_cap", "no_head_cap", "no_max_new_cap", "no_room_cap", "no_eos_cut"]


def ride_rows(D, max_new, eos, room, mutant=None):
    """k, the draft rows a ride feeds: D = the usable draft, max_new = the tokens the call may emit, room = max_positions - L positions
    left for fed tokens.  k = min(len(D), 7, max_new - 1, room), cut at the first draft id in the EOS set (an EOS is appended, never
    fed).  k = 0: a plain turn."""
    caps = []
    if mutant != "no_dlen_cap":
        caps.append(len(D))
    if mutant != "no_head_cap":
        caps.append(RIDE_MAX_ROWS)
    if mutant != "no_max_new_cap":
        caps.append(max_new - 1)
    if mutant != "no_room_cap":
        caps.append(room)
    k = max(min(caps), 0)
    if mutant != "no_eos_cut":
        for j in range(min(k, len(D))):
            if D[j] in eos:
                return j
    return k


def broken_rules(k, D, max_new, eos, room):
    """what a ride of k fed rows must respect whatever formula gave k, as a list of the rules it breaks (empty = fine): every fed row has
    a draft id, the head rows fit the verify step, no row's arg-max lies beyond max_new, no row reaches max_positions, no EOS id is fed"""
    bad = []
    if k > len(D):
        bad.append("a fed row without a draft id")
    if k + 1 > 8:
        bad.append("more than 8 head rows")
    if k >= 1 and k + 1 > max_new:
        bad.append("a row whose arg-max could never be emitted")
    if k > max(room, 0):
        bad.append("a row at or beyond max_positions")
    if any(t in eos for t in D[:k]):
        bad.append("an EOS id is fed")
    return bad


def simulate(true_ids, draft, max_new, eos, room, spec_rows, vocab=None, mutant=None):
    """A whole turn with the ride mode on.  true_ids: what plain greedy decoding emits (a row fed the true prefix has the true next id as
    its arg-max; any other row's arg-max is never used), draft: the caller's guess of the turn's ids, room = max_positions - L,
    spec_rows: rows per verify pass (0 = svln_set_speculative off).  Returns (ids, (rides, tokens_from_rides, rows_fed, verify_passes,
    tokens_from_verify, single_steps)); the ride's tokens include token 0, which counts in none of the last three."""
    eos = set(eos)
    D = VR.usable_draft(draft, vocab)
    k = ride_rows(D, max_new, eos, room, mutant)
    if k == 0:
        ids, passes, vtok, single = VR.simulate(true_ids, draft, spec_rows, max_new, eos, room, vocab)
        return ids, (0, 0, 0, passes, vtok, single)
    fed = [None] + [D[i] if i < len(D) else -5 for i in range(k)]          # (-5: only a mutant feeds a row the draft does not have)
    cand, ok = [], True
    for i in range(k + 1):
        ok = ok and (i == 0 or fed[i] == true_ids[i - 1])
        cand.append(int(true_ids[i]) if ok and i < len(true_ids) else -7)
    _, done, out, _ = VR.verify_step(fed, cand, 0, max_new, eos)
    assert -7 not in out
    rtok = len(out)
    held = all(out[j] == D[j] for j in range(min(len(out), len(D))))
    passes = vtok = single = 0
    if spec_rows and len(D) >= 2 and held:
        while not done:                                                 # verify_ref.simulate's loop, entered with len(out) tokens emitted
            c = len(out)
            r = VR.pass_rows(spec_rows, len(D), c, max_new, room)
            if c >= len(D) or r < 1:
                break
            vfed = [out[-1]] + [D[c + i - 1] for i in range(1, r)]
            vc, ok = [], True
            for i in range(r):
                ok = ok and (i == 0 or vfed[i] == true_ids[c + i - 1])
                vc.append(int(true_ids[c + i]) if ok and c + i < len(true_ids) else -7)
            _, done, emitted, _ = VR.verify_step(vfed, vc, c, max_new, eos)
            assert -7 not in emitted
            out += emitted
            passes += 1
            vtok += len(emitted)
            if not all(out[j] == D[j] for j in range(1, min(len(out), len(D)))):
                break
    while not done:
        c = len(out)
        assert room - (c - 1) > 0, "sequence exceeds max_positions during decode"
        tok = int(true_ids[c])
        out.append(tok)
        single += 1
        done = tok < 0 or len(out) >= max_new or tok in eos
    return out, (1, rtok, k, passes, vtok, single)
