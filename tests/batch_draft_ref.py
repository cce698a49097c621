"""The host policy of drafts in the scheduler's prefill pass (svln_set_batch_draft), restated in Python on top of prefill_draft_ref.ride_rows
and verify_ref.verify_step: what a submit does with the env's armed draft, how an iteration packs its prefill segments (slot order, the
workspace cut of k, jobs that wait), what each job emits from its k + 1 head rows, the kv_len / count bookkeeping, and the five counters of
svln_batch_draft_stats.  simulate runs a whole schedule -- lockstep (every turn submitted before iteration 0) or staggered."""
import prefill_draft_ref as PR
import verify_ref as VR

MAXB = 8                   # scheduler slots
HEAD_ROWS = 64             # head rows of one iteration: MAXB x (RIDE_MAX_ROWS + 1)
#: one mistake each: k not cut to the rows the workspace still holds; kv_len = n_embeds + e after a stop (the stopping token counted as
#: fed); the env's draft left armed by the submit that used it; a job that waits for the next iteration forgets its draft; the
#: acceptance goes on behind a row whose arg-max differs from the draft
MUTANTS = ["no_workspace_cut", "kv_len_after_stop", "draft_kept", "waiting_draft_lost", "accept_past_mismatch"]


class Turn:
    """one env's turn.  true_ids: what plain greedy decoding emits (a row fed the true prefix has the true next id as its arg-max; ids
    behind the stop are never read); draft: the ids armed for the env before the submit (None: nothing is armed); at: the scheduler
    iteration before which the turn is submitted; n_embeds / kv_len: the env's rows and cached rows at the submit."""

    def __init__(self, env, true_ids, draft, max_new, eos, n_embeds, kv_len, at=0):
        self.env, self.true_ids, self.draft, self.max_new, self.eos = env, [int(t) for t in true_ids], draft, max_new, set(eos)
        self.n_embeds, self.kv_len0, self.at = n_embeds, kv_len, at
        # filled in by simulate
        self.slot, self.D, self.k, self.out, self.kv_len, self.prefill, self.done = None, [], None, [], kv_len, True, False
        self.ride_tokens, self.decode_rows, self.first_iteration, self.first_log, self.last_iteration = 0, 0, None, None, None
        self.fed = []                     # (position, token) of every row the turn fed behind its prompt, rides and decode rows alike

    @property
    def Tn(self):
        return self.n_embeds - self.kv_len0


def pack(pre, n_dec, max_positions, mutant=None):
    """the prefill segments of one iteration: `pre` = the prefilling turns in slot order, n_dec = decode rows in front of them.  Returns
    (segments [(turn, k, first row)], rows M).  A turn whose Tn rows do not fit waits (and keeps its draft); k is ride_rows, cut to
    max_positions - M - Tn."""
    segs, M = [], n_dec
    for t in pre:
        if M + t.Tn > max_positions:
            if mutant == "waiting_draft_lost":
                t.D = []
            continue
        k = 0
        if t.D:
            k = PR.ride_rows(t.D, t.max_new, t.eos, max_positions - t.n_embeds)
            if mutant != "no_workspace_cut":
                k = min(k, max_positions - M - t.Tn)
        segs.append((t, k, M))
        M += t.Tn + k
    return segs, M


def accept(cand, D, max_new, eos, mutant=None):
    """the verify rule from zero emitted tokens on a job's k + 1 arg-maxes: row 0's is always emitted, row i's iff every earlier one was
    emitted without stopping and cand[i - 1] == D[i - 1] -> (emitted ids, stopped)"""
    if mutant == "accept_past_mismatch":
        fed = [None] + list(cand[:-1])
    else:
        fed = [None] + list(D[:len(cand) - 1])
    _, done, emitted, _ = VR.verify_step(fed, cand, 0, max_new, eos)
    return emitted, done


def _cand(t, k):
    """arg-max of head row i of a segment: the true id while every fed draft id so far is the true one (-7: never to be emitted)"""
    out, ok = [], True
    for i in range(k + 1):
        ok = ok and (i == 0 or t.D[i - 1] == t.true_ids[i - 1])
        out.append(t.true_ids[i] if ok and i < len(t.true_ids) else -7)
    return out


def simulate(turns, max_positions, vocab=None, penalty=1.0, switch=True, mutant=None):
    """Runs the schedule: before iteration i the turns with at == i are submitted in list order (lowest free slot; the env's armed draft
    is consumed when the switch is on, usable if penalty == 1, up to the first id outside the vocabulary); an iteration runs if a turn
    is in flight; a finished turn's slot is free for the next iteration.  Returns (rides, tokens_from_rides, rows_fed, iterations,
    single_rows) and a log: per iteration a dict(rows=M, head_rows, rides, decode_rows).  The turns carry their results."""
    armed = {}
    slots = [None] * MAXB
    rides = rtok = rfed = iters = single = 0
    log = []
    pending = sorted(turns, key=lambda t: t.at)
    it = 0
    while pending or any(s is not None for s in slots):
        for t in [t for t in pending if t.at <= it]:
            pending.remove(t)
            if t.draft is not None:
                armed[t.env] = list(t.draft)          # svln_set_draft (n = 0 clears)
                if not t.draft:
                    armed.pop(t.env)
            assert all(s is None or s.env != t.env for s in slots), "this env already has a turn in flight"
            t.slot = next(k for k in range(MAXB) if slots[k] is None)
            slots[t.slot] = t
            if switch and t.env in armed:
                d = armed[t.env] if mutant == "draft_kept" else armed.pop(t.env)
                t.D = VR.usable_draft(d, vocab) if penalty == 1.0 else []
        live = [s for s in slots if s is not None]
        if not live:
            it += 1
            continue
        dec = [t for t in live if not t.prefill]
        segs, M = pack([t for t in live if t.prefill], len(dec), max_positions, mutant)
        head = len(dec) + sum(k + 1 for _, k, _ in segs)
        log.append(dict(rows=M, head_rows=head, rides=sum(k > 0 for _, k, _ in segs), decode_rows=len(dec)))
        iters += 1
        single += len(dec)
        for t in dec:
            assert t.kv_len + 1 <= max_positions, "sequence exceeds max_positions during decode"
            t.fed.append((t.kv_len, t.out[-1]))
            tok = t.true_ids[len(t.out)]
            t.out.append(tok)
            t.kv_len += 1
            t.decode_rows += 1
            t.done = tok < 0 or len(t.out) >= t.max_new or tok in t.eos
        for t, k, _ in segs:
            t.k, t.first_iteration, t.first_log = k, it, len(log) - 1
            t.fed += [(t.n_embeds + i, t.D[i]) for i in range(k)]
            emitted, t.done = accept(_cand(t, k), t.D, t.max_new, t.eos, mutant)
            t.out += emitted
            e = len(emitted)
            t.kv_len = t.n_embeds + e - 1
            if mutant == "kv_len_after_stop" and t.done:
                t.kv_len += 1
            t.prefill = False
            if k > 0:
                rides += 1; rtok += e; rfed += k
                t.ride_tokens = e
            t.D = []                                  # the draft is dropped after its ride
        for t in live:
            if t.done:
                t.last_iteration = it
                slots[t.slot] = None
        it += 1
    return (rides, rtok, rfed, iters, single), log


def broken_rules(turns, log, max_positions, drafts_usable=True):
    """what a finished schedule must respect whatever policy produced it, as a list of the rules it breaks (empty = fine);
    drafts_usable: the switch is on and there is no repetition penalty"""
    bad = []
    for i, rec in enumerate(log):
        if rec["rows"] > max_positions:
            bad.append(f"iteration {i}: {rec['rows']} rows in a workspace of {max_positions}")
        if rec["head_rows"] > HEAD_ROWS:
            bad.append(f"iteration {i}: {rec['head_rows']} head rows")
    for t in turns:
        want = []
        for tok in t.true_ids:
            want.append(tok)
            if tok in t.eos or len(want) >= t.max_new:
                break
        if t.out != want:
            bad.append(f"env {t.env}: ids {t.out}, the plain loop's are {want}")
        if t.kv_len != t.n_embeds + len(want) - 1:
            bad.append(f"env {t.env}: kv_len {t.kv_len}, the plain loop's is {t.n_embeds + len(want) - 1}")
        if any(pos >= max_positions for pos, _ in t.fed):
            bad.append(f"env {t.env}: a row at or beyond max_positions")
        if any(tok in t.eos for _, tok in t.fed):
            bad.append(f"env {t.env}: an EOS id is fed")
        if t.draft is None and t.k:
            bad.append(f"env {t.env}: a turn without a draft of its own fed {t.k} draft rows")
        # a right draft that no cap cuts (the turn has <= 8 tokens, its positions fit, the workspace of its prefill iteration had room
        # for 7 more rows) leaves nothing to decode
        if drafts_usable and t.draft is not None and list(t.draft[:len(want)]) == want and len(want) <= PR.RIDE_MAX_ROWS + 1 and \
                t.n_embeds + len(want) - 1 <= max_positions and log[t.first_log]["rows"] + PR.RIDE_MAX_ROWS <= max_positions and t.decode_rows:
            bad.append(f"env {t.env}: a right draft, yet {t.decode_rows} decode rows")
    return bad
