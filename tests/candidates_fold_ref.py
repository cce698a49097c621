"""Cell-level restatement of the folded candidates call (svln_generate_candidates_folded): who writes which (page, slot) cell of ONE
layer's K / V pool, and which row of which pass scores which id.  Every layer does the same, so one layer is the model.

A cell holds a tag: ("row", pos) for a row of the env's own sequence (an earlier turn's or the prompt's), ("br", g, j) for the row that
sequence g fed F_g[j] at position L + j.  The call, in stream order:

  1. the env gets its pages up to position L + n_0 - 2; every sequence g >= 1 with n_g >= 2 gets a table = the env's pages below
     q0 = L / 64 + fresh pages from q0 on (fork_tail_pages);
  2. PRE-COPY, iff L % 64 != 0, a fork exists and P > 64 q0: the env's page q0 -- rows [64 q0, P) of earlier turns and whatever else it
     holds -- is copied whole to every fork's first page;
  3. PROMPT: row pos in [P, L) goes to the env's page pos / 64; if pos / 64 == q0 and L % 64 != 0, also to every fork's first page at
     the same slot (the mirror list; empty when L % 64 == 0);
  4. BRANCH: sequence g writes ("br", g, j) at position L + j, j < n_g - 1, through its own table (g = 0: the env's).  Rows j < r ride the
     prefill pass as rows Tn + g r + j; rows of pass p >= 1 are rows g r + (j - p r) of that pass.

simulate() returns the final state and a log of every write; check() raises AssertionError on the first broken invariant.  MUTANTS are
wrong variants, each of which check() must catch on some input (tests/test_candidates_fold_inputs.py)."""
PAGE = 64
MUTANTS = ("no_precopy", "precopy_after", "mirror_below_q0", "mirror_full_page", "slot_pos_plus_1", "src_rows_not_offset")


def rows_per_pass(n_seq, q_per_kv):
    return min(32 // q_per_kv, 32 // n_seq)


def fork_tail_pages(L, n):
    return 0 if n == 1 else (L + n - 1 + PAGE - 1) // PAGE - L // PAGE


class Sim:
    def __init__(self, n_pages):
        self.free = list(range(n_pages - 1, -1, -1))        # pages are taken from the back, as the engine's free list
        self.n_pages = n_pages
        self.cells = {}                                     # (page, slot) -> tag
        self.log = []                                       # (who, page, slot, tag); who: "hist", "copy", "prompt", "mirror", ("branch", g)
        self.env = []                                       # the env's table
        self.tables = {}                                    # g >= 1 -> table (shared entries below q0, private from q0 on)
        self.tails = {}                                     # g >= 1 -> private pages
        self.fed = {}                                       # (pass, row) -> (g, j): the row was fed F_g[j]; pass 0 = the folded prefill pass
        self.head = {}                                      # (g, i) -> (pass, row): the row whose final norm scores F_g[i]

    def take(self):
        assert self.free, "pool exhausted"
        return self.free.pop()

    def write(self, who, page, slot, tag):
        self.cells[(page, slot)] = tag
        self.log.append((who, page, slot, tag))


def simulate(L, P, lens, q_per_kv=2, n_pages=64, mutant=None):
    """the folded call on a prompt of L rows of which P are cached, candidates of lens[g] ids"""
    assert mutant is None or mutant in MUTANTS
    G, n_max, Tn, q0 = len(lens), max(lens), L - P, L // PAGE
    assert 2 <= G <= 8 and 0 <= P < L and n_max >= 2
    r = rows_per_pass(G, q_per_kv)
    s = Sim(n_pages)
    # the earlier turns' rows
    while len(s.env) * PAGE < P:
        s.env.append(s.take())
    for pos in range(P):
        s.write("hist", s.env[pos // PAGE], pos % PAGE, ("row", pos))
    # 1. pages and tables
    while len(s.env) * PAGE < L + lens[0] - 1:
        s.env.append(s.take())
    for g in range(1, G):
        n_tail = fork_tail_pages(L, lens[g])
        if n_tail:
            s.tails[g] = [s.take() for _ in range(n_tail)]
            s.tables[g] = s.env[:q0] + s.tails[g]
    firsts = [s.tails[g][0] for g in sorted(s.tails)]

    def precopy():
        src = s.env[q0]
        for dst in firsts:
            for slot in range(PAGE):
                if (src, slot) in s.cells:
                    s.write("copy", dst, slot, s.cells[(src, slot)])

    # 2. pre-copy
    copy_due = L % PAGE != 0 and firsts and P > q0 * PAGE
    if copy_due and mutant not in ("no_precopy", "precopy_after"):
        precopy()
    # 3. prompt rows, mirrored
    mirror_on = L % PAGE != 0 or mutant == "mirror_full_page"
    mirror_page = (L - 1) // PAGE if mutant == "mirror_full_page" and L % PAGE == 0 else q0
    for pos in range(P, L):
        s.write("prompt", s.env[pos // PAGE], pos % PAGE, ("row", pos))
        hit = pos // PAGE <= mirror_page if mutant == "mirror_below_q0" else pos // PAGE == mirror_page
        if mirror_on and hit:
            for dst in firsts:
                s.write("mirror", dst, pos % PAGE, ("row", pos))
    # 4. branch rows: pass 0 rides the prefill (rows Tn + g r + j), the later passes are scoring passes (rows g r + j)
    shift = 1 if mutant == "slot_pos_plus_1" else 0
    passes = (n_max - 1 + r - 1) // r
    for p in range(passes):
        for g in range(G):
            table = s.env if g == 0 else s.tables.get(g)
            for j in range(p * r, min((p + 1) * r, lens[g] - 1)):
                pos = L + j + shift
                assert pos // PAGE < len(table), ("a branch row beyond the pages of its sequence", g, pos)
                s.write(("branch", g), table[pos // PAGE], pos % PAGE, ("br", g, j))
                s.fed[(p, (Tn if p == 0 else 0) + g * r + (j - p * r))] = (g, j)
    if copy_due and mutant == "precopy_after":
        precopy()
    # head rows: F_g[0] <- the prompt's last row; F_g[i] <- the row that was fed F_g[i - 1]
    for g in range(G):
        s.head[(g, 0)] = (0, Tn - 1)
        for i in range(1, lens[g]):
            p, j = (i - 1) // r, (i - 1) % r
            base = Tn if p == 0 and mutant != "src_rows_not_offset" else 0
            s.head[(g, i)] = (p, base + g * r + j)
    s.L, s.P, s.lens, s.q0, s.Tn, s.r = L, P, tuple(lens), q0, Tn, r
    return s


def check(s):
    """the invariants of the folded call on a simulated state"""
    L, P, lens, q0, Tn = s.L, s.P, s.lens, s.q0, s.Tn
    # pages are conserved: the free list, the env's table and the forks' private pages partition the pool
    held = list(s.free) + list(s.env) + [p for t in s.tails.values() for p in t]
    assert sorted(held) == list(range(s.n_pages)), "pages are not conserved"
    logical = {p: i for i, p in enumerate(s.env)}
    for g, tail in s.tails.items():
        logical.update({p: q0 + i for i, p in enumerate(tail)})
    shared = set(s.env[:q0])
    for who, page, slot, tag in s.log:
        # a cell only ever receives the row of its own position: logical page x 64 + slot
        pos = tag[1] if tag[0] == "row" else L + tag[2]
        assert page in logical and logical[page] * PAGE + slot == pos, ("a row was stored at another position's cell", who, page, slot, tag)
        if isinstance(who, tuple):
            assert page not in shared, ("a branch wrote a shared page", who, page)
            if who[1] != 0:
                assert page not in s.env, ("a fork wrote a page of the env", who, page)
        if page in s.env:
            assert who in ("hist", "prompt", ("branch", 0)), ("the env's page was written by", who, page)
    # the env reads its own rows, then sequence 0's
    for pos in range(L + lens[0] - 1):
        want = ("row", pos) if pos < L else ("br", 0, pos - L)
        assert s.cells.get((s.env[pos // PAGE], pos % PAGE)) == want, ("env", pos)
    # every fork reads the env's rows up to L through its table -- in its own page q0 from 64 q0 on -- then its own branch rows
    for g, table in s.tables.items():
        assert table[:q0] == s.env[:q0] and not set(table[q0:]) & set(s.env)
        for pos in range(L + lens[g] - 1):
            want = ("row", pos) if pos < L else ("br", g, pos - L)
            assert s.cells.get((table[pos // PAGE], pos % PAGE)) == want, ("fork", g, pos, s.cells.get((table[pos // PAGE], pos % PAGE)))
    # the head-row list: F_g[0] is scored by the prompt's last row, F_g[i] by the row that was fed F_g[i - 1]
    for (g, i), (p, row) in s.head.items():
        if i == 0:
            assert (p, row) == (0, Tn - 1) and (p, row) not in s.fed, ("head row of F_g[0]", g)
        else:
            assert s.fed.get((p, row)) == (g, i - 1), ("head row", g, i, p, row, s.fed.get((p, row)))
    assert len(s.head) == sum(lens)
    return True
