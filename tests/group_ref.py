"""Host restatement of the group turn (svln_generate_group / svln_group_select): the page bookkeeping of the fork, which rows the batched decode
step carries and what they write, the select and the drop, and the stream / draw rule of the sampling noise.  No GPU, no engine: plain
Python lists for the pool and numpy over whole tables of length vectors.

The engine's rules, restated (engine.hip, "group sampling"):
  pool      free_pages is a stack, initially [total - 1 .. 0]: pages are taken from the back (page 0 first) and freed pages are pushed back.
  fork      L = n_embeds, limit = min(max_new, cap), q0 = L // 64, n_tail = ceil((L + limit - 1) / 64) - q0 (0 when limit == 1).  The env's
            own table is grown to cover L + limit - 1 positions; sequence g >= 1 gets a table = the env's entries [0, q0) + n_tail fresh
            pages; if L % 64 != 0 ONE copy launch duplicates the env's page q0 into the fresh q0 pages, else nothing is launched.
  decode    iteration t (0 <= t < limit - 1) runs while a sequence is live (has emitted t + 1 tokens and not stopped); row k of the
            B = next power of two >= n_seq rows is sequence k when that is live, else the FIRST LIVE sequence; a row writes position L + t
            of its sequence's table.
  select    index >= 1: the env's entries [q0, q0 + n_tail) and that sequence's private pages change places; then every fork page (the
            env's former tail included) is freed.  kv_len = L + n_out[index] - 1.
  drop      every fork page is freed (a reset then frees the env's own).
  noise     sequence g of env e draws from stream e + g * max_envs; token t of a turn uses draw c_e + t, c_e the env's counter, which
            then advances by max_g n_out[g].
Each MUTANTS entry changes one of these rules; tests/test_group_ref.py shows that each breaks an invariant on some case."""
import numpy as np

PAGE = 64
MUTANTS = ("share_q0", "copy_when_aligned", "select_keeps_env_tail", "select_swaps_q0_only", "forks_not_freed", "draws_by_seq0", "stream_env_plus_g",
           "pad_replays_row0")


def n_tail_of(L, limit):
    return 0 if limit == 1 else -(-(L + limit - 1) // PAGE) - L // PAGE


class Pool:
    """the engine's page pool and env tables (Engine::ensure_pages / release_pages), plus the pending group"""

    def __init__(self, pages_per_env, max_envs, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.pages_per_env, self.max_envs, self.mutant = pages_per_env, max_envs, mutant
        self.total = pages_per_env * max_envs
        self.free = list(range(self.total - 1, -1, -1))
        self.env_pages = [[] for _ in range(max_envs)]
        self.kv_len = [0] * max_envs
        self.group = None
        self.copy_launches = 0

    # ---- the plain engine
    def ensure_pages(self, env, positions):
        need = -(-positions // PAGE)
        assert need <= self.pages_per_env
        while len(self.env_pages[env]) < need:
            self.env_pages[env].append(self.free.pop())

    def reset_env(self, env):
        if self.group and self.group["env"] == env:
            self.drop()
        self.free.extend(self.env_pages[env])
        self.env_pages[env] = []
        self.kv_len[env] = 0

    # ---- the group turn
    def can_fork(self, env, L, limit, n_seq):
        nt = n_tail_of(L, limit)
        own = max((-(-L // PAGE) if limit == 1 else L // PAGE + nt) - len(self.env_pages[env]), 0)
        return L + limit - 1 <= self.pages_per_env * PAGE and len(self.free) >= own + (n_seq - 1) * nt

    def fork(self, env, L, limit, n_seq):
        """prefill pages, the env's tail, the forks' tables; returns the tables (index 0 = the env's own list object)"""
        assert self.group is None and 2 <= n_seq <= 8 and self.can_fork(env, L, limit, n_seq)
        q0, nt = L // PAGE, n_tail_of(L, limit)
        self.ensure_pages(env, L)
        if limit > 1:
            self.ensure_pages(env, L + limit - 1)
        own = self.env_pages[env]
        tails = [None] + [[] for _ in range(1, n_seq)]
        for g in range(1, n_seq):
            for i in range(nt):
                if self.mutant == "share_q0" and i == 0 and L % PAGE:
                    tails[g].append(own[q0])                       # MUTANT: the partly filled page is shared instead of copied
                else:
                    tails[g].append(self.free.pop())
        copy = bool(L % PAGE) and nt > 0
        if self.mutant == "copy_when_aligned" and nt > 0:
            copy = True
        if self.mutant == "share_q0":
            copy = False
        self.copy_launches += int(copy)
        self.group = dict(env=env, L=L, q0=q0, n_tail=nt, n_seq=n_seq, tails=tails, copied=copy, limit=limit)
        self.kv_len[env] = L
        return [own] + [own[:q0] + tails[g] for g in range(1, n_seq)]

    def tables(self):
        g, own = self.group, self.env_pages[self.group["env"]]
        return [own] + [own[:g["q0"]] + g["tails"][k] for k in range(1, g["n_seq"])]

    def select(self, index, n_out):
        g = self.group
        assert g is not None and 0 <= index < g["n_seq"]
        own, q0, nt = self.env_pages[g["env"]], g["q0"], g["n_tail"]
        if index >= 1 and nt > 0:
            swap = 1 if self.mutant == "select_swaps_q0_only" else nt
            for i in range(swap):
                own[q0 + i], g["tails"][index][i] = g["tails"][index][i], own[q0 + i]
            if self.mutant == "select_keeps_env_tail":
                g["tails"][index] = []                             # MUTANT: the env's former tail is forgotten, not freed
        self._free_forks()
        self.kv_len[g["env"]] = g["L"] + n_out[index] - 1
        self.group = None

    def drop(self):
        self._free_forks()
        self.group = None

    def _free_forks(self):
        g = self.group
        for k in range(1, g["n_seq"]):
            if self.mutant == "forks_not_freed" and k >= 2:
                continue                                           # MUTANT: only the first fork's pages go back
            self.free.extend(g["tails"][k])

    # ---- what the invariants look at
    def owners(self):
        """page -> list of owners ('free', ('env', e), ('fork', g))"""
        out = {}
        for p in self.free:
            out.setdefault(p, []).append("free")
        for e, pages in enumerate(self.env_pages):
            for p in pages:
                out.setdefault(p, []).append(("env", e))
        if self.group:
            for k in range(1, self.group["n_seq"]):
                for p in self.group["tails"][k]:
                    out.setdefault(p, []).append(("fork", k))
        return out

    def conserved(self):
        """every page of the pool has exactly one owner"""
        o = self.owners()
        return len(o) == self.total and all(len(v) == 1 for v in o.values())


# ------------------------------------------------------------------------------------------------ decode rows over whole tables of lengths
def length_vectors(n_seq, limit):
    """every vector of sequence lengths in 1 .. limit: int8 [limit ** n_seq, n_seq]"""
    return np.stack(np.meshgrid(*[np.arange(1, limit + 1, dtype=np.int8)] * n_seq, indexing="ij"), -1).reshape(-1, n_seq)


def row_sources(lengths, t, mutant=None):
    """iteration t of the decode loop for every length vector: (ran [N], src [N, B]) -- src[n, k] = the sequence row k carries"""
    N, G = lengths.shape
    B = 2
    while B < G:
        B *= 2
    live = lengths > t + 1                                         # sequence g has emitted t + 1 tokens without stopping
    ran = live.any(1)
    first = np.argmax(live, 1)
    if mutant == "pad_replays_row0":
        first = np.zeros(N, dtype=np.int64)                        # MUTANT: the scheduler's "slot 0" rule, after sequence 0 may have finished
    src = np.empty((N, B), dtype=np.int64)
    for k in range(B):
        src[:, k] = np.where(live[:, k], k, first) if k < G else first
    return ran, src


def written(lengths, limit, mutant=None):
    """W [N, G, limit - 1]: does iteration t write position L + t of sequence g's table"""
    N, G = lengths.shape
    W = np.zeros((N, G, max(limit - 1, 0)), dtype=bool)
    for t in range(limit - 1):
        ran, src = row_sources(lengths, t, mutant)
        for g in range(G):
            W[:, g, t] = ran & (src == g).any(1)
    return W


# ------------------------------------------------------------------------------------------------ streams and draws
def stream_of(env, g, max_envs, mutant=None):
    return env + g if mutant == "stream_env_plus_g" else env + g * max_envs


def advance(counter, lengths, mutant=None):
    """the env's draw counter after a group turn, for every length vector: [N]"""
    return counter + (lengths[:, 0] if mutant == "draws_by_seq0" else lengths.max(1)).astype(np.int64)


def noise_pairs(turns, max_envs, mutant=None):
    """turns: list of (env, lengths of its sequences; one entry = a plain sampled turn).  Returns every (stream, draw) pair used, in order."""
    counter, pairs = [0] * max_envs, []
    for env, lens in turns:
        for g, n in enumerate(lens):
            pairs += [(stream_of(env, g, max_envs, mutant), counter[env] + t) for t in range(n)]
        counter[env] += lens[0] if mutant == "draws_by_seq0" else max(lens)
    return pairs


# ------------------------------------------------------------------------------------------------ the end-to-end precondition
#: (turn, stream) pairs of the fixtures whose token-0 perturbed top-2 margin at T = 1, seed E2E_SEED, draw 0 falls under the a-priori dot
#: bound of tests/test_sample_e2e_gpu.py: proved by tests/test_group_ref.py from the fixtures' hidden rows, excluded by the GPU test
E2E_SEED = 0x6A0FF1CE5EED
TOKEN0_UNDER = {"tiny_episode": [], "tiny_penalty": []}


def token0_margins(Wd, hidden_rows, seed, n_streams=8, T=1.0):
    """for each fixture turn (its token-0 final-norm row) and stream g < n_streams at draw 0: (margin, bound, arg-max) in float64 -- the
    margin of the two largest perturbed logits against 2 * dot + tol, as tests/test_sample_e2e_gpu.py::_check_turn computes them"""
    import sample_ref as R
    V, K = Wd.shape
    gamma, inv_t = K * 2.0 ** -24, float(np.float32(1.0) / np.float32(T))
    out = {}
    for t, h in enumerate(hidden_rows):
        h = np.asarray(h, dtype=np.float64)
        y = (Wd @ h) * inv_t
        dot = 2 * gamma * float((np.abs(Wd) @ np.abs(h)).max()) * inv_t
        for s in range(n_streams):
            g = R.gumbel(seed, s, 0, np.arange(V))
            z = y + g
            a = int(np.argmax(z))
            zb, gb = np.delete(z, a), np.delete(g, a)
            b = int(np.argmax(zb))
            tol = 2.0 ** -17 * max(1.0, abs(g[a]), abs(gb[b])) + 2.0 ** -22 * float(np.abs(z).max())
            out[(t, s)] = (float(z[a] - zb[b]), 2 * dot + tol, a)
    return out
