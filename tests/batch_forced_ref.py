"""The host policy of forced jobs in the multi-env scheduler (svln_batch_submit_forced), restated in Python in the style of
batch_draft_ref.py: what a forced submit refuses, how an iteration packs its segments (slot order, all or nothing, jobs that wait), which
rows a forced segment feeds, the head list behind the plain head rows and its chunk table, the kv_len bookkeeping and the three counters
of svln_batch_forced_stats.  Plain jobs here are the scheduler's plain jobs without rides (batch_draft_ref.py owns those): one arg-max per
iteration.  simulate runs a whole schedule; broken_rules states what every finished schedule must respect whatever policy produced it."""
MAXB = 8                   # scheduler slots
FORCED_MAX = 32            # ids of one forced job
CHUNK = 32                 # head rows of one EPI_TARGET launch
MFMA_MIN = 4               # rows from which the lm_head product is the 32-row MFMA tiles
#: one mistake each: the last id is fed too; kv_len = n_embeds + n; a segment that does not fit is cut to the rows left, like a draft; the
#: row at a chunk edge is dropped (chunks of 32 taken every 33 rows) / repeated (every 31); row i's target is F[i + 1]; the tap row is
#: taken from the row's index in its chunk; the plain head rows are listed behind the forced ones
MUTANTS = ["last_id_fed", "kv_len_off_by_one", "segment_cut", "chunk_edge_dropped", "chunk_edge_repeated", "target_next", "tap_from_chunk_row",
           "plain_rows_shifted"]


def head_route(r):
    """(rows the product is launched with, its form) for a chunk of r live rows: the routing of svln_generate_forced for n = r"""
    if r <= 2:
        return 2, "gemv"
    return (4 if r == 3 else r), "mfma"


def submit_refusal(F, eos, n_embeds, kv_len, max_positions, vocab, penalty=1.0, allowed=None, switches=(), in_flight=False, free_slots=8):
    """the reason a forced submit is refused, or None.  Nothing changes before a refusal."""
    if not (1 <= len(F) <= FORCED_MAX):
        return "n must be 1 .. 32"
    for k, t in enumerate(F):
        if not (0 <= t < vocab):
            return "outside the vocabulary"
        if k + 1 < len(F) and t in eos:
            return "EOS"
    if penalty != 1.0:
        return "svln_set_repetition_penalty"
    for s in ("svln_set_fp8_decode", "svln_set_mxfp4_decode", "svln_set_fp8_gemm", "svln_set_mxfp4_batched", "svln_set_decode_persistent"):
        if s in switches:
            return s
    if allowed is not None and any(t not in allowed for t in F):
        return "allowed list"
    if in_flight:
        return "already has a turn in flight"
    if free_slots < 1:
        return "at most 8 turns in flight"
    if n_embeds - kv_len < 1:
        return "nothing to prefill"
    if n_embeds + len(F) - 1 > max_positions:
        return "max_positions"
    return None


class Turn:
    """one env's turn.  forced: the ids F of a forced job, or None for a plain job, which emits true_ids one per iteration until max_new or
    an EOS id; at: the scheduler iteration before which the turn is submitted; n_embeds / kv_len: the env's rows at the submit."""

    def __init__(self, env, n_embeds, kv_len, forced=None, true_ids=(), max_new=1, eos=(), at=0):
        self.env, self.n_embeds, self.kv_len0, self.at = env, n_embeds, kv_len, at
        self.forced = None if forced is None else [int(t) for t in forced]
        self.true_ids, self.max_new, self.eos = [int(t) for t in true_ids], max_new, set(eos)
        # filled in by simulate
        self.slot, self.out, self.kv_len, self.prefill, self.done = None, [], kv_len, True, False
        self.first_iteration, self.last_iteration, self.waited = None, None, []
        self.fed = []                     # (position, token) of every row the turn fed behind its prompt
        self.head = []                    # forced: per head row dict(i, src, tap, target, list_index, iteration)

    @property
    def Tn(self):
        return self.n_embeds - self.kv_len0


def tap_row(i, n, slot):
    """the parity tap row head row i of a job of n ids is copied to: min(i, 7) of the job's slot; of the rows that share tap row 7 the
    last one is kept (what a sequence of copies leaves there), the others are not copied (-1)"""
    return (min(i, 7) * MAXB + slot) if (i < 7 or i == n - 1) else -1


def chunks_of(nf, mutant=None):
    """[(first list row, live rows)] of the chunks of nf forced head rows"""
    step = CHUNK + 1 if mutant == "chunk_edge_dropped" else CHUNK - 1 if mutant == "chunk_edge_repeated" else CHUNK
    return [(r0, min(nf - r0, CHUNK)) for r0 in range(0, nf, step)]


def simulate(turns, max_positions, mutant=None):
    """Runs the schedule: before iteration i the turns with at == i are submitted in list order (lowest free slot); an iteration runs
    while a turn is in flight; a finished turn's slot is free for the next iteration.  Returns (jobs, rows_fed, head_launches) and a log:
    per iteration dict(iteration, rows, decode_rows, plain_head [(slot, head index)], forced_rows, chunks [(r0, r, launched rows, form, targets)],
    gathered [(workspace row, id)])."""
    slots = [None] * MAXB
    jobs = rows_fed = launches = 0
    log = []
    pending = sorted(turns, key=lambda t: t.at)
    it = 0
    while pending or any(s is not None for s in slots):
        for t in [t for t in pending if t.at <= it]:
            pending.remove(t)
            assert all(s is None or s.env != t.env for s in slots), "this env already has a turn in flight"
            t.slot = next(k for k in range(MAXB) if slots[k] is None)
            slots[t.slot] = t
        live = [s for s in slots if s is not None]
        if not live:
            it += 1
            continue
        dec = [t for t in live if not t.prefill]
        M = len(dec)
        segs, gathered = [], []
        for t in [t for t in live if t.prefill]:
            nfed = 0 if t.forced is None else len(t.forced) - (0 if mutant == "last_id_fed" else 1)
            if M + t.Tn + nfed > max_positions:
                if mutant == "segment_cut" and t.forced is not None and M + t.Tn <= max_positions:
                    nfed = max_positions - M - t.Tn
                else:
                    t.waited.append((it, M))
                    continue
            for q in range(nfed):
                gathered.append((M + t.Tn + q, t.forced[q]))
                t.fed.append((t.n_embeds + q, t.forced[q]))
            segs.append((t, M, t.Tn + nfed))
            M += t.Tn + nfed
        if not dec and not segs:          # nothing can run: a policy that never fits a job it accepted (broken_rules names the job)
            break
        # the plain head rows: decode rows first, then the last row of every plain segment -- the indices of an iteration without forced jobs
        plain = [t for t in dec] + [t for t, _, _ in segs if t.forced is None]
        forced_rows = []
        for t, off, rows in segs:
            if t.forced is None:
                continue
            n = len(t.forced)
            for i in range(n):
                tgt = t.forced[i + 1] if mutant == "target_next" and i + 1 < n else t.forced[i]
                forced_rows.append(dict(turn=t, i=i, src=off + rows - n + i, target=tgt))
        shift = len(forced_rows) if mutant == "plain_rows_shifted" else 0
        plain_head = [(t.slot, shift + k) for k, t in enumerate(plain)]
        chunks = []
        for r0, r in chunks_of(len(forced_rows), mutant):
            launched, form = head_route(r)
            chunks.append((r0, r, launched, form, [forced_rows[r0 + k]["target"] if k < r else -1 for k in range(launched)]))
            launches += 1
        for li, row in enumerate(forced_rows):
            t, i = row["turn"], row["i"]
            ti = li % CHUNK if mutant == "tap_from_chunk_row" else i
            t.head.append(dict(i=i, src=row["src"], tap=tap_row(ti, len(t.forced), t.slot), target=row["target"], list_index=li, iteration=it))
        log.append(dict(iteration=it, rows=M, decode_rows=len(dec), plain_head=plain_head, forced_rows=len(forced_rows), chunks=chunks, gathered=gathered))
        for t in dec:
            assert t.kv_len + 1 <= max_positions, "sequence exceeds max_positions during decode"
            t.fed.append((t.kv_len, t.out[-1]))
            t.out.append(t.true_ids[len(t.out)])
            t.kv_len += 1
        for t, _, rows in segs:
            t.first_iteration, t.prefill = it, False
            if t.forced is None:
                t.out.append(t.true_ids[0])
                t.kv_len = t.n_embeds
            else:
                n = len(t.forced)
                t.out = list(t.forced)
                t.kv_len = t.n_embeds + n - (0 if mutant == "kv_len_off_by_one" else 1)
                t.done = True
                jobs += 1
                rows_fed += rows - t.Tn
        for t in live:
            if t.forced is None and not t.prefill:
                t.done = len(t.out) >= t.max_new or t.out[-1] in t.eos
            if t.done:
                t.last_iteration = it
                slots[t.slot] = None
        it += 1
    return (jobs, rows_fed, launches), log


def broken_rules(turns, log, max_positions):
    """what a finished schedule must respect, as a list of the rules it breaks (empty = fine)"""
    bad = []
    for i, rec in enumerate(log):
        if rec["rows"] > max_positions:
            bad.append(f"iteration {i}: {rec['rows']} rows in a workspace of {max_positions}")
        if any(row >= max_positions for row, _ in rec["gathered"]):
            bad.append(f"iteration {i}: a gathered row at or beyond the workspace")
        # plain head rows keep the indices of an iteration without forced jobs: 0 .. count - 1 in slot-of-kind order
        if [h for _, h in rec["plain_head"]] != list(range(len(rec["plain_head"]))):
            bad.append(f"iteration {i}: plain head rows at {[h for _, h in rec['plain_head']]}")
        # every forced head row lies in exactly one chunk; pad rows carry -1; the launch follows the route table
        cover = [0] * rec["forced_rows"]
        for r0, r, launched, form, targets in rec["chunks"]:
            for k in range(r0, min(r0 + r, rec["forced_rows"])):
                cover[k] += 1
            if r0 + r > rec["forced_rows"] or not (1 <= r <= CHUNK) or (launched, form) != head_route(r):
                bad.append(f"iteration {i}: chunk ({r0}, {r}) launched as {launched} rows of {form}")
            if any(t != -1 for t in targets[r:]):
                bad.append(f"iteration {i}: a pad row with a target")
        if any(c != 1 for c in cover):
            bad.append(f"iteration {i}: forced head rows covered {cover} times")
    for t in turns:
        if t.forced is None:
            want = []
            for tok in t.true_ids:
                want.append(tok)
                if tok in t.eos or len(want) >= t.max_new:
                    break
            if t.out != want or t.kv_len != t.n_embeds + len(want) - 1:
                bad.append(f"env {t.env}: a plain turn with ids {t.out} / kv_len {t.kv_len}")
            continue
        F, n = t.forced, len(t.forced)
        if not t.done:
            bad.append(f"env {t.env}: an accepted forced job that never ran")
            continue
        if t.out != F:
            bad.append(f"env {t.env}: out {t.out} != F")
        if t.kv_len != t.n_embeds + n - 1:
            bad.append(f"env {t.env}: kv_len {t.kv_len}, not n_embeds + n - 1 = {t.n_embeds + n - 1}")
        if t.fed != [(t.n_embeds + q, F[q]) for q in range(n - 1)]:
            bad.append(f"env {t.env}: fed {t.fed}, not F[:-1] at n_embeds ..")
        if any(pos >= max_positions for pos, _ in t.fed):
            bad.append(f"env {t.env}: a row at or beyond max_positions")
        if any(tok in t.eos for _, tok in t.fed):
            bad.append(f"env {t.env}: an EOS id is fed")
        if t.first_iteration != t.last_iteration:
            bad.append(f"env {t.env}: a forced job that took a decode iteration")
        if [h["i"] for h in t.head] != list(range(n)) or [h["list_index"] for h in t.head] != list(range(t.head[0]["list_index"], t.head[0]["list_index"] + n)):
            bad.append(f"env {t.env}: its head rows are not n consecutive rows of the list")
        for h in t.head:
            if h["target"] != F[h["i"]]:
                bad.append(f"env {t.env}: head row {h['i']} scores id {h['target']}, not F[i]")
            if h["tap"] != tap_row(h["i"], n, t.slot):
                bad.append(f"env {t.env}: head row {h['i']} goes to tap row {h['tap']}")
        # head row i is the row that precedes F[i]: the last prompt row for i = 0, the row that fed F[i - 1] behind it
        rec = log_of(log, t)
        if rec is not None:
            fed_rows = [row for row, tok in rec["gathered"]]
            for h in t.head[1:]:
                if h["src"] not in fed_rows or h["src"] != t.head[0]["src"] + h["i"]:
                    bad.append(f"env {t.env}: head row {h['i']} reads workspace row {h['src']}")
        # a job waits only while its whole segment does not fit behind the rows packed before it
        for it, M in t.waited:
            if M + t.Tn + n - 1 <= max_positions:
                bad.append(f"env {t.env}: waited in iteration {it} with room for its segment")
    return bad


def log_of(log, t):
    """the log record of the iteration that prefilled turn t (an iteration without a live turn is not logged)"""
    if not t.head:
        return None
    for rec in log:
        if rec["iteration"] == t.head[0]["iteration"]:
            return rec
    return None
