"""The engine's switches as one table, and the expected outcome of every unordered pair of them (test infrastructure; the spec that
tests/test_switches_inputs.py checks against include/streamvln_hip.h and tests/test_switch_pairs_gpu.py against the engine).

A row is one `svln_set_*` switch of the C ABI, or one call-time mode (`svln_generate_group`, `svln_generate_forced`: their "on" is the
call).  The matrix is DERIVED from the header text and the rule table of csrc/modes.h -- the rule that produces an entry stands beside it;
tests/test_mode_table.py compares the two without a GPU -- and is total: PAIRS holds every unordered pair of rows exactly once.

  REFUSED   with A on, switching B on (or making the call B) raises, and the message names A's C function; the same with the roles
            swapped.  Call-time modes leave nothing switched on behind them, so a pair with one is refused in the one order that exists
            (switch on, then the call); group x forced is the forced call on an env whose group is pending.
  COMPOSES  both are honoured in one run.
  NO_EFFECT documented precedence: under the other row, switching `inert` on changes no bit of any result.  `reason` says why.

`excluded` (a reason string) marks the pairs whose RUN part test_switch_pairs_gpu.py leaves out; their setter outcomes are still
checked.  Only pairs with svln_set_decode_persistent may be excluded, and not those with decode_graph, packed_decode,
repetition_penalty and layer_taps (which tests/test_e2e_gpu.py already runs or which are trivially lossless): the persistent kernel
spins on inter-workgroup flags, and a combination nobody has run is not something to try first on a shared machine.
"""
from collections import namedtuple

BF16, F32 = "bf16", "fp32"
BOTH = (BF16, F32)

REFUSED, COMPOSES, NO_EFFECT = "REFUSED", "COMPOSES", "NO_EFFECT"

# ---------------------------------------------------------------------------------------------------------------------------- the probe's constants
ALLOWED_IDS = tuple(range(0, 4096, 17))          # 241 ids of the TINY vocabulary; a third of them are in tiny_episode's EOS set (id % 3 == 2)
FORCED_IDS = (34, 51, 68)                      # a forced turn's ids, all in ALLOWED_IDS; only the last one is an EOS id of tiny_episode
SAMPLING = (0.8, 77)                             # temperature, seed
PRUNE_KEEP = 100                                 # of the 2 x 196 memory tokens of tiny_episode's restart turn
ROW_LIMIT = 150                                  # tiny_truncate's value: cuts every turn inside its image block
PENALTY = 1.3                                    # tiny_penalty's value
CACHE_FRAMES = 16

# Row.on / Row.off: callables on the Python model (streamvln_amd.model.StreamVLNForCausalLM).  Row.setter: the Python name (a method, or an
# attribute the model pushes to the engine at call time).  Row.effect: how a probe run shows that the switch was honoured:
#   ("stat", key)        the run's stats delta `key` is > 0
#   ("key", name)        every solo turn's result carries `name`
#   ("subset",)          every emitted id is in ALLOWED_IDS
#   ("differs", part)    the run's `part` ("solo", "lock" or "any") differs from the all-off run in ids or hidden bits
#   ("call",)            the call itself is the effect (a group result has several sequences; a forced turn returns its ids)
#   None                 nothing public shows it (`why` in the row says so); the class assertions still hold
Row = namedtuple("Row", "name c_name setter on off dtypes cls effect call_time note")


def _attr(obj_name, attr, value):
    return lambda m: setattr(getattr(m, obj_name), attr, value)


def _mode(key, value):
    """call-time modes are flags of the probe driver (m.probe_modes), read when it issues the solo turns"""
    return lambda m: m.probe_modes.__setitem__(key, value)


ROWS = [
    # ---- lossless: results are bit-identical to off
    Row("decode_graph", "svln_set_decode_graph", "set_decode_graph", lambda m: m.set_decode_graph(True), lambda m: m.set_decode_graph(False),
        BOTH, "lossless", None, False, "no public counter: a replayed step is the launched step"),
    Row("packed_decode", "svln_set_packed_decode", "set_packed_decode", lambda m: m.set_packed_decode(True), lambda m: m.set_packed_decode(False),
        (BF16,), "lossless", ("stat", "packed_blocks"), False, ""),
    Row("feature_cache", "svln_set_feature_cache", "set_feature_cache", lambda m: m.set_feature_cache(CACHE_FRAMES), lambda m: m.set_feature_cache(0),
        BOTH, "lossless", ("stat", "cache_hits"), False, ""),
    Row("layer_taps", "svln_set_layer_taps", "set_layer_taps", lambda m: m.set_layer_taps(True), lambda m: m.set_layer_taps(False),
        BOTH, "lossless", ("stat", "layer_taps"), False, ""),
    # ---- scheme: changes numerics
    Row("fp8_decode", "svln_set_fp8_decode", "set_fp8_decode", lambda m: m.set_fp8_decode(True), lambda m: m.set_fp8_decode(False),
        (BF16,), "scheme", ("differs", "solo"), False, ""),
    Row("mxfp4_decode", "svln_set_mxfp4_decode", "set_mxfp4_decode", lambda m: m.set_mxfp4_decode(True), lambda m: m.set_mxfp4_decode(False),
        (BF16,), "scheme", ("differs", "solo"), False, ""),
    Row("mxfp4_batched", "svln_set_mxfp4_batched", "set_mxfp4_batched", lambda m: m.set_mxfp4_batched(True), lambda m: m.set_mxfp4_batched(False),
        (BF16,), "scheme", ("differs", "lock"), False, ""),
    Row("fp8_gemm", "svln_set_fp8_gemm", "set_fp8_gemm", lambda m: m.set_fp8_gemm(True), lambda m: m.set_fp8_gemm(False),
        (BF16,), "scheme", ("differs", "any"), False, ""),
    Row("fp8_scaled_mfma", "svln_set_fp8_scaled_mfma", "set_fp8_scaled_mfma", lambda m: m.set_fp8_scaled_mfma(True), lambda m: m.set_fp8_scaled_mfma(False),
        (BF16,), "scheme", None, False, "the same e4m3 bytes, scales and fp32 sums on another instruction: no result has to move, and no counter exists"),
    Row("decode_persistent", "svln_set_decode_persistent", "set_decode_persistent", lambda m: m.set_decode_persistent(True),
        lambda m: m.set_decode_persistent(False), BOTH, "scheme", ("differs", "solo"), False, ""),
    Row("memory_prune", "svln_set_memory_prune", "set_memory_prune", lambda m: m.set_memory_prune(PRUNE_KEEP), lambda m: m.set_memory_prune(0),
        BOTH, "scheme", ("differs", "solo"), False, ""),
    Row("turn_row_limit", "svln_set_turn_row_limit", "config.tokenizer_model_max_length", _attr("config", "tokenizer_model_max_length", ROW_LIMIT),
        _attr("config", "tokenizer_model_max_length", None), BOTH, "scheme", ("differs", "any"), False, ""),
    # ---- output: changes or adds outputs
    Row("token_scores", "svln_set_token_scores", "set_token_scores", lambda m: m.set_token_scores(True), lambda m: m.set_token_scores(False),
        BOTH, "output", ("key", "token_logprobs"), False, ""),
    Row("sampling", "svln_set_sampling", "set_sampling", lambda m: m.set_sampling(*SAMPLING), lambda m: m.set_sampling(None),
        BOTH, "output", ("differs", "any"), False, ""),
    Row("allowed_tokens", "svln_set_allowed_tokens", "set_allowed_tokens", lambda m: m.set_allowed_tokens(ALLOWED_IDS, add_eos=False),
        lambda m: m.set_allowed_tokens(None), BOTH, "output", ("subset",), False, ""),
    Row("repetition_penalty", "svln_set_repetition_penalty", "generation_config.repetition_penalty", _attr("generation_config", "repetition_penalty", PENALTY),
        _attr("generation_config", "repetition_penalty", 1.0), BOTH, "output", ("differs", "any"), False, ""),
    # ---- draft
    Row("speculative", "svln_set_speculative", "set_speculative", lambda m: m.set_speculative(2), lambda m: m.set_speculative(0),
        BOTH, "draft", ("stat", "verify_passes"), False, ""),
    Row("prefill_draft", "svln_set_prefill_draft", "set_prefill_draft", lambda m: m.set_prefill_draft(True), lambda m: m.set_prefill_draft(False),
        BOTH, "draft", ("stat", "rides"), False, ""),
    Row("batch_draft", "svln_set_batch_draft", "set_batch_draft", lambda m: m.set_batch_draft(True), lambda m: m.set_batch_draft(False),
        BOTH, "draft", ("stat", "batch_rides"), False, ""),
    Row("draft", "svln_set_draft", "set_auto_draft", lambda m: m.set_auto_draft(True), lambda m: m.set_auto_draft(False),
        BOTH, "draft", None, False, "arms a guess; only a draft switch reads it (their counters are their effect, not this row's)"),
    # ---- call-time modes: the "on" is the call
    Row("generate_group", "svln_generate_group", "generate(do_sample=True, num_return_sequences=2)", _mode("group", True), _mode("group", False),
        BOTH, "output", ("call",), True, ""),
    Row("generate_forced", "svln_generate_forced", "generate(forced_ids=...)", _mode("forced", True), _mode("forced", False),
        BOTH, "output", ("call",), True, ""),
]
BY_NAME = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]

# every other `svln_set_*` prototype of the header, and why it has no row
NOT_SWITCHES = {
    "svln_set_tensor": "a weight write, not a switch: tests/test_weight_rewrite_gpu.py covers it under every mode",
}

# the state restore() returns to, in this fixed order: everything off, then the probe's base (decode graphs on, auto-draft armed)
RESTORE_ORDER = ["generate_group", "generate_forced", "speculative", "prefill_draft", "batch_draft", "token_scores", "sampling", "allowed_tokens",
                 "repetition_penalty", "turn_row_limit", "memory_prune", "feature_cache", "layer_taps", "fp8_scaled_mfma", "fp8_gemm", "mxfp4_batched",
                 "mxfp4_decode", "fp8_decode", "decode_persistent"]
BASE_ON = ["packed_decode", "decode_graph", "draft"]          # packed_decode: the engine's default on bf16

# ---------------------------------------------------------------------------------------------------------------------------- the matrix
Entry = namedtuple("Entry", "kind names inert reason excluded")     # names: REFUSED -> {row on first: C function the message must name}

DRAFT3 = ("speculative", "prefill_draft", "batch_draft")
SCHEME5 = ("fp8_decode", "mxfp4_decode", "fp8_gemm", "mxfp4_batched", "decode_persistent")      # csrc/modes.h SVLN_SCHEME5
PLAIN_HEAD = DRAFT3 + ("decode_persistent", "mxfp4_batched")                                     # csrc/modes.h SVLN_PLAIN_HEAD_ONLY
SINGLE_SCHEME = ("fp8_decode", "mxfp4_decode", "fp8_gemm", "decode_persistent")                  # csrc/modes.h SVLN_SCHEME4
PERSISTENT_RUNS = ("decode_graph", "packed_decode", "repetition_penalty", "layer_taps")
EXCLUDED_WHY = ("the persistent layer spins on inter-workgroup flags: a combination no test has run before is not tried first on a shared "
                "machine (setter outcomes are still checked)")


def _key(a, b):
    return frozenset((a, b))


def _refused(a, b):
    return Entry(REFUSED, {a: BY_NAME[a].c_name, b: BY_NAME[b].c_name}, None, "", None)


def _build():
    refused, inert = {}, {}

    def refuse(a, b):
        refused[_key(a, b)] = _refused(a, b)

    def no_effect(other, who, reason):
        inert.setdefault(_key(other, who), Entry(NO_EFFECT, None, who, reason, None))

    # -- refusals between setters (each holds in both orders: each setter's "on" caller has a row for the other's bit)
    for d in DRAFT3:
        for s in SCHEME5:                # a verify pass / ridden row must be computed in the scheme of the step it replaces
            refuse(d, s)
        for o in ("token_scores", "sampling"):       # their tokens leave the verify step: no scores, a greedy rule
            refuse(d, o)
    for o in ("token_scores", "sampling"):           # no scored / sampled form of the persistent layer's head or of gemv_mx4b_kernel
        refuse(o, "decode_persistent")
        refuse(o, "mxfp4_batched")
    refuse("fp8_decode", "mxfp4_decode")             # one weight format per decode step
    refuse("fp8_decode", "mxfp4_batched")
    refuse("fp8_gemm", "mxfp4_batched")
    # -- refusals of the call-time modes
    refuse("generate_group", "repetition_penalty")   # a group does not support it
    for p in PLAIN_HEAD:                             # a group is sampled by definition
        refuse("generate_group", p)
    refuse("generate_forced", "repetition_penalty")  # its flags change row by row
    for s in SINGLE_SCHEME:                          # a forced row must be computed in the scheme of the step it stands in for
        refuse("generate_forced", s)
    refused[_key("generate_group", "generate_forced")] = Entry(
        REFUSED, {"generate_group": "svln_group_select", "generate_forced": "svln_group_select"}, None,
        "both are calls: the pair is a forced turn on an env whose group is pending", None)
    # -- documented precedence
    for r in NAMES:
        if r not in ("fp8_gemm", "fp8_scaled_mfma"):
            no_effect(r, "fp8_scaled_mfma", "svln_set_fp8_scaled_mfma: no effect while svln_set_fp8_gemm is off")
    for s in ("fp8_decode", "mxfp4_decode"):
        no_effect(s, "packed_decode", "svln_set_packed_decode: the e4m3 / MXFP4 decode weights read their own copies and take precedence")
        no_effect(s, "decode_persistent", "svln_set_decode_persistent: with the e4m3 / MXFP4 decode weights on, the launched GEMVs are kept")
        no_effect("generate_group", s, "svln_generate_group runs the scheduler's batched lm_head and decode step, which the single-env decode "
                                       "switches never reach (a group computes what svln_generate_batch would)")
    for r in NAMES:
        if r not in DRAFT3 + ("draft",):
            no_effect(r, "draft", "svln_set_draft: ignored while no draft switch is on")
    for d in DRAFT3:
        no_effect("repetition_penalty", d, "svln_set_draft: a draft is ignored while a repetition penalty != 1 is set")
    for d in ("speculative", "prefill_draft"):
        no_effect("generate_forced", d, "svln_generate_forced: the draft switches may be on, no verify rule runs (the armed draft is consumed); "
                                        "the scheduler ignores these two")
    out = {}
    for i, a in enumerate(NAMES):
        for b in NAMES[i + 1:]:
            k = _key(a, b)
            e = refused.get(k) or inert.get(k) or Entry(COMPOSES, None, None, "", None)
            if "decode_persistent" in k and not (k & set(PERSISTENT_RUNS)):
                e = e._replace(excluded=EXCLUDED_WHY)
            out[k] = e
    return out


PAIRS = _build()


def entry(a, b):
    return PAIRS[_key(a, b)]


def pairs():
    """every unordered pair once, in table order"""
    return [(a, b) for i, a in enumerate(NAMES) for b in NAMES[i + 1:]]


def counts():
    c = {REFUSED: 0, COMPOSES: 0, NO_EFFECT: 0, "excluded": 0}
    for e in PAIRS.values():
        c[e.kind] += 1
        c["excluded"] += e.excluded is not None
    return c
