"""What the engine answers to every mode switch and turn form under every reachable mode state (test infrastructure).

`observe(model)` works on one bf16 TINY engine (tests/switch_probe.make_model) through the ctypes surface only, so the same file runs on
any build of the engine.  tools/record_mode_refusals.py stores its result as tests/golden/mode_refusals.json; tests/test_mode_table.py
compares that record with the rule table of csrc/modes.h on a machine without a GPU, tests/test_mode_refusals_gpu.py with the engine.

  states    every set of at most two modes that can be switched on together (prerequisites -- the scores under top-k lists and entropies,
            sampling under its truncation -- do not count towards the two), the empty set, and two further ones: "jobs" (one
            svln_batch_submit on an env with an appended turn, never stepped, then svln_batch_cancel) and "group" (one svln_generate_group
            turn with sampling on), each alone and with every single mode that can be switched on before it
  attempts  every setter in both directions (on while on / off while off are the no-change calls), one weight write, and every turn form
            on an env with NOTHING TO PREFILL: every form reaches that check only after its refusals, so an accepted attempt ends in
            the "nothing to prefill" message and launches nothing; that text is stored as "accepted"

Apart from the one group turn no turn runs and no scheduler is stepped: in particular no decode step ever runs with
svln_set_decode_persistent on (the setter allocates and checks only; see switches_ref.py on untried persistent combinations).
"""
import ctypes as C
import itertools

import numpy as np

import switches_ref as S
from scenarios import SEED
from streamvln_amd.weights import tensor_seed, tensor_specs

ACCEPTED = "accepted"
JOBS, GROUP = "jobs", "group"
# the modes the rules read, in the order a state switches them on (svln_mode_state's field order)
MODES = ("decode_graph", "persistent", "fp8_decode", "mxfp4_decode", "mxfp4_batched", "fp8_gemm", "fp8_scaled", "packed",
         "speculative", "prefill_draft", "batch_draft", "scores", "topk", "entropy", "sampling", "truncation", "allowed", "penalty")
PREREQ = {"topk": "scores", "entropy": "scores", "truncation": "sampling"}
OFF_ORDER = ("truncation", "entropy", "topk") + tuple(m for m in MODES if m not in ("truncation", "entropy", "topk"))
TURN_FORMS = ("svln_generate_group", "svln_generate_beams", "svln_generate_forced", "svln_batch_submit_forced", "svln_generate_candidates",
              "svln_generate_candidates_folded", "svln_generate_batch")
WEIGHT_WRITE = "svln_synth_tensor"
ATTEMPTS = tuple(f"{m}:{d}" for m in MODES for d in ("on", "off")) + (WEIGHT_WRITE,) + TURN_FORMS
IDLE_ENV, BUSY_ENV = 0, 1          # nothing to prefill / the env of the submitted job and of the pending group
TOPK_K, TRUNC = 4, (4, 0.9)
PI64, PI32, PF = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)


def full_state(modes):
    """the modes with their prerequisites, in MODES order (then jobs / group)"""
    want = set(modes)
    want |= {PREREQ[m] for m in want if m in PREREQ}
    return tuple(m for m in MODES + (JOBS, GROUP) if m in want)


class _Engine:
    def __init__(self, model):
        self.lib, self.h = model._lib, model._h
        self.allowed = np.asarray(S.ALLOWED_IDS, dtype=np.int64)
        self.forced = np.asarray(S.FORCED_IDS, dtype=np.int64)                 # ids inside the vocabulary and the allowed list
        self.cand = np.asarray(S.FORCED_IDS[:2] + S.FORCED_IDS[:1], dtype=np.int64)
        self.cand_lens = np.asarray([2, 1], dtype=np.int32)
        self.eos = np.asarray([S.FORCED_IDS[-1] + 17], dtype=np.int64)          # an allowed id no attempt's list holds
        self.out = np.zeros(8 * 64, dtype=np.int64)
        self.n_out = np.zeros(8, dtype=np.int32)
        self.f32 = np.zeros(3 * 64, dtype=np.float32)
        self.envs = np.asarray([IDLE_ENV], dtype=np.int32)
        spec = {s.name: s for s in tensor_specs(model.cfg)}["model.norm.weight"]
        self.synth = (spec.name.encode(), tensor_seed(SEED, spec.name), spec.half_width, spec.base)    # rewrites the bits it holds
        self.slot = None

    def _p(self, a, t):
        return a.ctypes.data_as(t)

    def result(self, rc):
        if rc == 0:
            return ACCEPTED
        msg = self.lib.svln_last_error().decode("utf-8", "replace")
        return ACCEPTED if "nothing to prefill" in msg else msg

    def must(self, rc):
        if rc != 0:
            raise RuntimeError("mode_refusals_ref: " + self.lib.svln_last_error().decode("utf-8", "replace"))

    def switch(self, mode, on):
        """the setter call of `mode` -> its return code"""
        lib, h, v = self.lib, self.h, int(on)
        if mode == "decode_graph":
            return lib.svln_set_decode_graph(h, v)
        if mode == "persistent":
            return lib.svln_set_decode_persistent(h, v)
        if mode == "fp8_decode":
            return lib.svln_set_fp8_decode(h, v)
        if mode == "mxfp4_decode":
            return lib.svln_set_mxfp4_decode(h, v)
        if mode == "mxfp4_batched":
            return lib.svln_set_mxfp4_batched(h, v)
        if mode == "fp8_gemm":
            return lib.svln_set_fp8_gemm(h, v)
        if mode == "fp8_scaled":
            return lib.svln_set_fp8_scaled_mfma(h, v)
        if mode == "packed":
            return lib.svln_set_packed_decode(h, v)
        if mode == "speculative":
            return lib.svln_set_speculative(h, 2 * v)
        if mode == "prefill_draft":
            return lib.svln_set_prefill_draft(h, v)
        if mode == "batch_draft":
            return lib.svln_set_batch_draft(h, v)
        if mode == "scores":
            return lib.svln_set_token_scores(h, v)
        if mode == "topk":
            return lib.svln_top_logprobs(h, TOPK_K * v)
        if mode == "entropy":
            return lib.svln_token_entropy(h, v)
        if mode == "sampling":
            return lib.svln_set_sampling(h, 1, S.SAMPLING[0], S.SAMPLING[1]) if on else lib.svln_set_sampling(h, 0, 0.0, 0)
        if mode == "truncation":
            return lib.svln_sampling_truncation(h, *TRUNC) if on else lib.svln_sampling_truncation(h, 0, 1.0)
        if mode == "allowed":
            return lib.svln_set_allowed_tokens(h, self._p(self.allowed, PI64), len(self.allowed)) if on else lib.svln_set_allowed_tokens(h, None, 0)
        if mode == "penalty":
            return lib.svln_set_repetition_penalty(h, S.PENALTY if on else 1.0)
        raise KeyError(mode)

    def call(self, name):
        """a weight write, or a turn form on the env that has nothing to prefill -> its return code"""
        lib, h, p = self.lib, self.h, self._p
        if name == WEIGHT_WRITE:
            return lib.svln_synth_tensor(h, *self.synth)
        if name == "svln_generate_group":
            return lib.svln_generate_group(h, IDLE_ENV, 2, 2, p(self.eos, PI64), 1, p(self.out, PI64), 64, p(self.n_out, PI32))
        if name == "svln_generate_beams":
            return lib.svln_generate_beams(h, IDLE_ENV, 2, 2, p(self.eos, PI64), 1, p(self.out, PI64), 64, p(self.n_out, PI32), p(self.f32, PF))
        if name == "svln_generate_forced":
            return lib.svln_generate_forced(h, IDLE_ENV, p(self.forced, PI64), len(self.forced), p(self.eos, PI64), 1, p(self.f32, PF),
                                            p(self.out, PI64), p(self.f32[64:], PF), None)
        if name == "svln_batch_submit_forced":         # the dry run: a null slot queues nothing
            return lib.svln_batch_submit_forced(h, IDLE_ENV, p(self.forced, PI64), len(self.forced), p(self.eos, PI64), 1, None)
        if name in ("svln_generate_candidates", "svln_generate_candidates_folded"):
            return getattr(lib, name)(h, IDLE_ENV, 2, p(self.cand, PI64), p(self.cand_lens, PI32), p(self.eos, PI64), 1, p(self.f32, PF),
                                      p(self.out, PI64), p(self.f32[64:], PF))
        if name == "svln_generate_batch":
            return lib.svln_generate_batch(h, p(self.envs, PI32), 1, 2, p(self.eos, PI64), 1, p(self.out, PI64), 64, p(self.n_out, PI32))
        raise KeyError(name)

    # ---- states
    def all_off(self):
        if self.slot is not None:
            self.must(self.lib.svln_batch_cancel(self.h, self.slot))
            self.slot = None
        for env in (IDLE_ENV, BUSY_ENV):               # (drops a pending group, a job and the appended rows)
            self.must(self.lib.svln_reset_env(self.h, env))
        for m in OFF_ORDER:
            self.must(self.switch(m, False))

    def establish(self, state):
        """from all-off: the state's switches in MODES order, then its job / group; False (and all-off again) if a step is refused"""
        for m in state:
            if m in (JOBS, GROUP):
                ids = np.asarray([5, 6, 7, 8, 9], dtype=np.int64)
                self.must(self.lib.svln_append_turn(self.h, BUSY_ENV, self._p(ids, PI64), len(ids), 0))
                if m == JOBS:
                    slot = C.c_int32(-1)
                    self.must(self.lib.svln_batch_submit(self.h, BUSY_ENV, 2, None, 0, C.byref(slot)))
                    self.slot = slot.value
                    continue
                rc = self.lib.svln_generate_group(self.h, BUSY_ENV, 2, 2, None, 0, self._p(self.out, PI64), 64, self._p(self.n_out, PI32))
            else:
                rc = self.switch(m, True)
            if rc != 0:
                self.all_off()
                return False
        return True

    def restore(self, mode, state):
        """after an accepted setter attempt: the switch (and what hangs on it) back to what `state` says"""
        self.must(self.switch(mode, mode in state))
        if mode == "sampling" and "truncation" in state:        # (sampling off clears its truncation)
            self.must(self.switch("truncation", True))


def states():
    """every candidate state, as full_state tuples in a fixed order (unreachable ones are dropped by observe)"""
    out = [()]
    for n in (1, 2):
        out += [full_state(c) for c in itertools.combinations(MODES, n)]
    for extra in (JOBS, GROUP):
        base = ("sampling",) if extra == GROUP else ()
        out += [full_state(base + c + (extra,)) for c in [()] + [(m,) for m in MODES]]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def observe(model):
    """-> {"states": [...], "attempts": [...], "messages": [...], "rows": [[state, attempt, message], ...]} (indices into the three lists)"""
    e = _Engine(model)
    e.all_off()
    for m in ("fp8_decode", "mxfp4_decode", "fp8_gemm", "persistent"):       # the e4m3 / MXFP4 copies and the layer's buffers: built once
        e.must(e.switch(m, True))
        e.must(e.switch(m, False))
    reached, rows, messages = [], [], {ACCEPTED: 0}
    for state in states():
        if not e.establish(state):
            continue
        si = len(reached)
        reached.append(list(state))
        for ai, att in enumerate(ATTEMPTS):
            if ":" in att:
                mode, d = att.split(":")
                res = e.result(e.switch(mode, d == "on"))
                if res == ACCEPTED:
                    e.restore(mode, state)
            else:
                res = e.result(e.call(att))
            rows.append([si, ai, messages.setdefault(res, len(messages))])
        e.all_off()
    e.must(e.switch("packed", True))                   # the engine's default on bf16
    return {"states": reached, "attempts": list(ATTEMPTS), "messages": list(messages), "rows": rows}
