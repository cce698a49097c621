// Which of the engine's modes may be on together, and which turn forms run under them: ONE ordered rule table, as a pure host function.
// Plain C++17, no HIP.  Every setter and turn form of engine.hip asks mode_refusal() (through Engine::refuse) and holds no rule of its
// own; svln_mode_refusal / svln_mode_rule (engine.hip) answer without a device; tests/test_mode_table.py pins the table to a record of
// what the engine answered before the table existed (tests/golden/mode_refusals.json).
//
// A new mode adds: its bit to ModeBit (and the field to svln_mode_state, in the same place), its term to Engine::modes_now(), one
// sentence to mode_text, the Caller value(s) of its setter with their rows, and one row to every caller that cannot run under
// it -- the rows of a refused PAIR are two: each setter's "on" caller holds the other's bit.  DESIGN.md ("The mode table") has the rest.
#pragma once
#include <cstdint>
#include <string>

namespace svln {

// one bit per mode the rules read (the order of svln_mode_state's fields), then the two pieces of engine state they also refuse on
enum ModeBit : int {
    M_DECODE_GRAPH, M_PERSISTENT, M_FP8_DECODE, M_MXFP4_DECODE, M_MXFP4_BATCHED, M_FP8_GEMM, M_FP8_SCALED, M_PACKED,
    M_SPECULATIVE, M_PREFILL_DRAFT, M_BATCH_DRAFT,
    M_SCORES, M_TOPK, M_ENTROPY, M_SAMPLING, M_TRUNCATION, M_ALLOWED,
    M_PENALTY,          // rep_penalty != 1
    M_JOBS,             // scheduler turns in flight
    M_GROUP,            // a group turn is pending (on env ModeState::group_env)
    M_COUNT
};
struct ModeState {
    uint32_t bits = 0;
    int group_env = 0;
    bool on(ModeBit b) const { return (bits >> b) & 1u; }
    void set(ModeBit b, bool v) { if (v) bits |= 1u << b; }
};

// one value per thing that can be refused: a setter per direction (their rows differ), the weight write, the turn forms
enum Caller : int {
    C_SET_DECODE_PERSISTENT_ON, C_SET_DECODE_PERSISTENT_OFF,
    C_SET_FP8_DECODE_ON, C_SET_FP8_DECODE_OFF,
    C_SET_MXFP4_DECODE_ON, C_SET_MXFP4_DECODE_OFF,
    C_SET_MXFP4_BATCHED_ON, C_SET_MXFP4_BATCHED_OFF,
    C_SET_FP8_GEMM_ON, C_SET_FP8_GEMM_OFF,
    C_SET_FP8_SCALED_MFMA,
    C_SET_SPECULATIVE_ON, C_SET_SPECULATIVE_OFF,
    C_SET_PREFILL_DRAFT_ON, C_SET_PREFILL_DRAFT_OFF,
    C_SET_BATCH_DRAFT_ON, C_SET_BATCH_DRAFT_OFF,
    C_SET_TOKEN_SCORES_ON, C_SET_TOKEN_SCORES_OFF,
    C_TOP_LOGPROBS_ON, C_TOP_LOGPROBS_OFF,                    // k > 0, k = 0
    C_TOKEN_ENTROPY_ON, C_TOKEN_ENTROPY_OFF,
    C_SET_SAMPLING_ON, C_SET_SAMPLING_OFF,
    C_SAMPLING_TRUNCATION_ON, C_SAMPLING_TRUNCATION_OFF,      // top_k > 0, top_k = 0 (top_p < 1 needs a top_k)
    C_SET_ALLOWED_TOKENS,
    C_SET_REPETITION_PENALTY,
    C_WEIGHT_WRITE,                                           // svln_set_tensor, svln_synth_tensor
    C_GENERATE_BATCH, C_GENERATE_GROUP, C_GENERATE_BEAMS,
    C_GENERATE_FORCED, C_BATCH_SUBMIT_FORCED,                 // (the candidates forms run C_GENERATE_FORCED's rows under their own name)
    C_GENERATE_CANDIDATES,
    C_OP_GEMV_BATCHED_ARGMAX,                                 // the test op's plain arg-max form (epi = EPI_ARGMAX, no norm)
    C_COUNT
};
// the name a caller's messages begin with, unless the call passes another (svln_synth_tensor, the candidates forms, svln_turn_*)
constexpr const char* CALLER_NAME[C_COUNT] = {
    "svln_set_decode_persistent", "svln_set_decode_persistent", "svln_set_fp8_decode", "svln_set_fp8_decode",
    "svln_set_mxfp4_decode", "svln_set_mxfp4_decode", "svln_set_mxfp4_batched", "svln_set_mxfp4_batched",
    "svln_set_fp8_gemm", "svln_set_fp8_gemm", "svln_set_fp8_scaled_mfma",
    "svln_set_speculative", "svln_set_speculative", "svln_set_prefill_draft", "svln_set_prefill_draft",
    "svln_set_batch_draft", "svln_set_batch_draft", "svln_set_token_scores", "svln_set_token_scores",
    "svln_top_logprobs", "svln_top_logprobs", "svln_token_entropy", "svln_token_entropy",
    "svln_set_sampling", "svln_set_sampling", "svln_sampling_truncation", "svln_sampling_truncation",
    "svln_set_allowed_tokens",
    "repetition_penalty",                                     // (its one message never named the C function)
    "svln_set_tensor",
    "svln_generate_batch", "svln_generate_group", "svln_generate_beams", "svln_generate_forced", "svln_batch_submit_forced",
    "svln_generate_candidates", "svln_op_gemv_batched",
};

// ---- the sentences, once each.  A message is <caller's name> + what + tail; "{env}" in a sentence stands for ModeState::group_env.
namespace mode_text {
constexpr const char* JOBS = " cannot change while scheduler turns are in flight";
constexpr const char* JOBS_PENALTY = " cannot change while turns are in flight";
constexpr const char* BUSY = " needs an idle scheduler (turns are in flight)";
constexpr const char* GROUP = " cannot change while a group turn is pending (svln_group_select)";
constexpr const char* ANY_GROUP = ": a group turn is pending on env {env}; choose its continuation with svln_group_select first";
constexpr const char* PERSISTENT = ": the persistent decode layer is on (svln_set_decode_persistent)";
constexpr const char* FP8_DECODE = ": the e4m3 decode weights are on (svln_set_fp8_decode)";
constexpr const char* MXFP4_DECODE = ": the MXFP4 decode weights are on (svln_set_mxfp4_decode)";
constexpr const char* MXFP4_BATCHED = ": the batched MXFP4 weights are on (svln_set_mxfp4_batched)";
constexpr const char* FP8_GEMM = ": the e4m3 MFMA products are on (svln_set_fp8_gemm)";
constexpr const char* FP8_GEMM_BEAMS = ": the fp8 MFMA products are on (svln_set_fp8_gemm)";
constexpr const char* SPECULATIVE = ": draft-verified decode is on (svln_set_speculative)";
constexpr const char* PREFILL_DRAFT = ": drafts inside the prefill pass are on (svln_set_prefill_draft)";
constexpr const char* BATCH_DRAFT = ": drafts in the scheduler's prefill pass are on (svln_set_batch_draft)";
constexpr const char* SCORES = ": token log-probabilities are on (svln_set_token_scores)";
constexpr const char* SCORES_OFF = ": token log-probabilities are off (svln_set_token_scores)";
constexpr const char* TOPK = ": top-k log-probabilities are on (svln_top_logprobs)";
constexpr const char* ENTROPY = ": token entropies are on (svln_token_entropy)";
constexpr const char* SAMPLING = ": temperature sampling is on (svln_set_sampling)";
constexpr const char* SAMPLING_OFF = ": temperature sampling is off (svln_set_sampling)";
constexpr const char* TRUNCATION = ": truncated sampling is on (svln_sampling_truncation)";
constexpr const char* PENALTY = ": a repetition penalty != 1 is set (svln_set_repetition_penalty)";
// the switches that change the numeric scheme or the execution form of a step.  SCHEME4: those the single-env paths read (svln_generate's
// decode step and prefill) -- a forced turn, which runs on those paths only, refuses them.  SCHEME5 adds svln_set_mxfp4_batched, which the
// scheduler paths alone read: the three draft switches and the scheduler's forced submit refuse all five.  One row per bit, one sentence.
constexpr const char* SCHEME5 = ": a reduced-precision or persistent decode mode is on (svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm, "
                                "svln_set_mxfp4_batched, svln_set_decode_persistent)";
constexpr const char* SCHEME4 = ": a reduced-precision or persistent decode mode is on (svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm, "
                                "svln_set_decode_persistent)";
// the tails
constexpr const char* NONE = "";
constexpr const char* IT_OFF = "; switch it off first";
constexpr const char* THEM_OFF = "; switch them off first";
constexpr const char* IT_ON = "; switch it on first";
constexpr const char* THEM_ON = "; switch them on first";
constexpr const char* NO_CANDIDATE_FORM = ", whose epilogue has no candidate form; switch them off first";
constexpr const char* NO_ENTROPY_FORM_THEM = ", whose epilogue has no entropy form; switch them off first";
constexpr const char* NO_ENTROPY_FORM_IT = ", whose epilogue has no entropy form; switch it off first";
constexpr const char* NOT_IN_GROUPS = ", which group turns do not carry; switch them off first";
constexpr const char* NOT_IN_THIS_FORM = ", which this turn form does not carry; switch them off first";
constexpr const char* GREEDY_IDENTICAL = ": greedy sequences would be identical";
constexpr const char* BEAMS_GREEDY = "; beams are greedy: switch it off first";
constexpr const char* GROUP_NO_PENALTY = "; a group does not support it";
constexpr const char* BEAMS_NO_PENALTY = "; beams do not support it";
constexpr const char* FLAGS_PER_ROW = "; its flags change row by row";
constexpr const char* OR_SAMPLE_OP = "; switch it off first, or use svln_op_gemv_batched_argmax_sample";
constexpr const char* BATCHED_STEP = ": a scoring pass runs the batched step; switch them off first";
}  // namespace mode_text

// A rule: `caller` is refused while `bit` is on (must_be_on: while it is OFF).  part: a caller whose run of rules is interrupted by a
// check that is no mode rule (an argument, a shape) makes one call per part, so that no message changes precedence.  on_no_change: the
// rule also holds for a call that would change nothing (setters return early in that case, at different places).
struct ModeRule { Caller caller; int part; ModeBit bit; bool must_be_on; bool on_no_change; const char* what; const char* tail; };

namespace mode_rows {
using namespace mode_text;
// the runs several callers share, in the order they always had
#define SVLN_DRAFTS(c, p)                                                                                                              \
    {c, p, M_SPECULATIVE, false, false, SPECULATIVE, IT_OFF}, {c, p, M_PREFILL_DRAFT, false, false, PREFILL_DRAFT, THEM_OFF},          \
    {c, p, M_BATCH_DRAFT, false, false, BATCH_DRAFT, THEM_OFF}
// the modes whose tokens come out of neither a scored nor a sampled arg-max: the three draft switches (their tokens leave the verify
// step, whose rule is written for greedy rows), the persistent decode layer and the batched MXFP4 weights (gemv_mx4b_kernel has the
// plain arg-max only).  svln_set_sampling, svln_set_token_scores and svln_generate_group (sampled by definition) share the list.
#define SVLN_PLAIN_HEAD_ONLY(c, p)                                                                                                     \
    SVLN_DRAFTS(c, p), {c, p, M_PERSISTENT, false, false, PERSISTENT, IT_OFF}, {c, p, M_MXFP4_BATCHED, false, false, MXFP4_BATCHED, THEM_OFF}
#define SVLN_SCHEME4(c, p, text)                                                                                                       \
    {c, p, M_FP8_DECODE, false, false, text, IT_OFF}, {c, p, M_MXFP4_DECODE, false, false, text, IT_OFF},                              \
    {c, p, M_FP8_GEMM, false, false, text, IT_OFF}, {c, p, M_PERSISTENT, false, false, text, IT_OFF}
#define SVLN_SCHEME5(c, p) SVLN_SCHEME4(c, p, SCHEME5), {c, p, M_MXFP4_BATCHED, false, false, SCHEME5, IT_OFF}
// a draft switch: off needs no turns in flight; on also greedy unscored tokens and the numeric scheme of the step a row replaces
#define SVLN_DRAFT_SETTER(on, off, p_scheme)                                                                                           \
    {on, 0, M_JOBS, false, false, JOBS, NONE}, {on, 0, M_SCORES, false, false, SCORES, THEM_OFF},                                      \
    {on, 0, M_SAMPLING, false, false, SAMPLING, IT_OFF}, SVLN_SCHEME5(on, p_scheme), {off, 0, M_JOBS, false, false, JOBS, NONE}

constexpr ModeRule RULES[] = {
    {C_SET_DECODE_PERSISTENT_ON, 0, M_JOBS, false, false, JOBS, NONE},
    SVLN_DRAFTS(C_SET_DECODE_PERSISTENT_ON, 0),
    {C_SET_DECODE_PERSISTENT_ON, 0, M_SCORES, false, false, SCORES, THEM_OFF},
    {C_SET_DECODE_PERSISTENT_ON, 0, M_SAMPLING, false, false, SAMPLING, IT_OFF},
    {C_SET_DECODE_PERSISTENT_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    {C_SET_FP8_DECODE_ON, 0, M_JOBS, false, false, JOBS, NONE},
    SVLN_DRAFTS(C_SET_FP8_DECODE_ON, 0),
    {C_SET_FP8_DECODE_ON, 0, M_MXFP4_DECODE, false, false, MXFP4_DECODE, THEM_OFF},           // one weight format per decode step
    {C_SET_FP8_DECODE_ON, 0, M_MXFP4_BATCHED, false, false, MXFP4_BATCHED, THEM_OFF},
    {C_SET_FP8_DECODE_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    {C_SET_MXFP4_DECODE_ON, 0, M_JOBS, false, false, JOBS, NONE},
    SVLN_DRAFTS(C_SET_MXFP4_DECODE_ON, 0),
    {C_SET_MXFP4_DECODE_ON, 0, M_FP8_DECODE, false, false, FP8_DECODE, THEM_OFF},
    {C_SET_MXFP4_DECODE_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    // part 1 follows the bf16 check
    {C_SET_MXFP4_BATCHED_ON, 0, M_JOBS, false, false, JOBS, NONE},
    SVLN_DRAFTS(C_SET_MXFP4_BATCHED_ON, 0),
    {C_SET_MXFP4_BATCHED_ON, 0, M_SCORES, false, false, SCORES, THEM_OFF},
    {C_SET_MXFP4_BATCHED_ON, 0, M_SAMPLING, false, false, SAMPLING, IT_OFF},
    {C_SET_MXFP4_BATCHED_ON, 1, M_FP8_DECODE, false, false, FP8_DECODE, THEM_OFF},
    {C_SET_MXFP4_BATCHED_ON, 1, M_FP8_GEMM, false, false, FP8_GEMM, THEM_OFF},
    {C_SET_MXFP4_BATCHED_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    {C_SET_FP8_GEMM_ON, 0, M_JOBS, false, false, JOBS, NONE},
    SVLN_DRAFTS(C_SET_FP8_GEMM_ON, 0),
    {C_SET_FP8_GEMM_ON, 0, M_MXFP4_BATCHED, false, false, MXFP4_BATCHED, THEM_OFF},
    {C_SET_FP8_GEMM_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    {C_SET_FP8_SCALED_MFMA, 0, M_JOBS, false, false, JOBS, NONE},

    // svln_set_speculative's part 1 follows its rows x heads check; the other two have one run
    SVLN_DRAFT_SETTER(C_SET_SPECULATIVE_ON, C_SET_SPECULATIVE_OFF, 1),
    SVLN_DRAFT_SETTER(C_SET_PREFILL_DRAFT_ON, C_SET_PREFILL_DRAFT_OFF, 0),
    SVLN_DRAFT_SETTER(C_SET_BATCH_DRAFT_ON, C_SET_BATCH_DRAFT_OFF, 0),

    // the lists and entropies ride on the scored partials: the scores stay on under them
    {C_SET_TOKEN_SCORES_ON, 0, M_GROUP, false, true, GROUP, NONE},
    {C_SET_TOKEN_SCORES_ON, 0, M_JOBS, false, false, JOBS, NONE},
    SVLN_PLAIN_HEAD_ONLY(C_SET_TOKEN_SCORES_ON, 0),
    {C_SET_TOKEN_SCORES_OFF, 0, M_GROUP, false, true, GROUP, NONE},
    {C_SET_TOKEN_SCORES_OFF, 0, M_TOPK, false, false, TOPK, THEM_OFF},
    {C_SET_TOKEN_SCORES_OFF, 0, M_ENTROPY, false, false, ENTROPY, THEM_OFF},
    {C_SET_TOKEN_SCORES_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    {C_TOP_LOGPROBS_ON, 0, M_GROUP, false, true, GROUP, NONE},
    {C_TOP_LOGPROBS_ON, 0, M_JOBS, false, false, JOBS, NONE},
    {C_TOP_LOGPROBS_ON, 0, M_SCORES, true, false, SCORES_OFF, THEM_ON},
    {C_TOP_LOGPROBS_ON, 0, M_ENTROPY, false, false, ENTROPY, NO_CANDIDATE_FORM},
    {C_TOP_LOGPROBS_OFF, 0, M_GROUP, false, true, GROUP, NONE},
    {C_TOP_LOGPROBS_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    {C_TOKEN_ENTROPY_ON, 0, M_GROUP, false, true, GROUP, NONE},
    {C_TOKEN_ENTROPY_ON, 0, M_JOBS, false, false, JOBS, NONE},
    {C_TOKEN_ENTROPY_ON, 0, M_SCORES, true, false, SCORES_OFF, THEM_ON},
    {C_TOKEN_ENTROPY_ON, 0, M_TOPK, false, false, TOPK, NO_ENTROPY_FORM_THEM},
    {C_TOKEN_ENTROPY_ON, 0, M_TRUNCATION, false, false, TRUNCATION, NO_ENTROPY_FORM_IT},
    {C_TOKEN_ENTROPY_OFF, 0, M_GROUP, false, true, GROUP, NONE},
    {C_TOKEN_ENTROPY_OFF, 0, M_JOBS, false, false, JOBS, NONE},

    // svln_set_sampling has no no-change case; part 1 follows its temperature checks
    {C_SET_SAMPLING_ON, 0, M_JOBS, false, true, JOBS, NONE},
    {C_SET_SAMPLING_ON, 0, M_GROUP, false, true, GROUP, NONE},
    SVLN_PLAIN_HEAD_ONLY(C_SET_SAMPLING_ON, 1),
    {C_SET_SAMPLING_OFF, 0, M_JOBS, false, true, JOBS, NONE},
    {C_SET_SAMPLING_OFF, 0, M_GROUP, false, true, GROUP, NONE},

    // (off stays off whatever the switches are; a truncation that is on has sampling on, so "off" needs no sampling row)
    {C_SAMPLING_TRUNCATION_ON, 0, M_ENTROPY, false, true, ENTROPY, NO_CANDIDATE_FORM},
    {C_SAMPLING_TRUNCATION_ON, 0, M_GROUP, false, true, GROUP, NONE},
    {C_SAMPLING_TRUNCATION_ON, 0, M_JOBS, false, true, JOBS, NONE},
    {C_SAMPLING_TRUNCATION_ON, 0, M_SAMPLING, true, false, SAMPLING_OFF, IT_ON},
    {C_SAMPLING_TRUNCATION_OFF, 0, M_GROUP, false, true, GROUP, NONE},
    {C_SAMPLING_TRUNCATION_OFF, 0, M_JOBS, false, true, JOBS, NONE},

    // only the lm_head product is swapped: no rule against another switch
    {C_SET_ALLOWED_TOKENS, 0, M_JOBS, false, true, JOBS, NONE},
    {C_SET_ALLOWED_TOKENS, 0, M_GROUP, false, true, GROUP, NONE},

    {C_SET_REPETITION_PENALTY, 0, M_JOBS, false, true, JOBS_PENALTY, NONE},

    // a turn in flight or a pending group was computed partly with the old weights
    {C_WEIGHT_WRITE, 0, M_JOBS, false, true, JOBS, NONE},
    {C_WEIGHT_WRITE, 0, M_GROUP, false, true, GROUP, NONE},

    // the turn forms that run the scheduler's batched step themselves need it idle
    {C_GENERATE_BATCH, 0, M_JOBS, false, true, BUSY, NONE},

    {C_GENERATE_GROUP, 0, M_TOPK, false, true, TOPK, NOT_IN_GROUPS},
    {C_GENERATE_GROUP, 0, M_ENTROPY, false, true, ENTROPY, NOT_IN_THIS_FORM},
    SVLN_PLAIN_HEAD_ONLY(C_GENERATE_GROUP, 0),                 // (svln_set_sampling is refused under each of them: name the cause)
    {C_GENERATE_GROUP, 0, M_SAMPLING, true, true, SAMPLING_OFF, GREEDY_IDENTICAL},
    {C_GENERATE_GROUP, 0, M_PENALTY, false, true, PENALTY, GROUP_NO_PENALTY},
    {C_GENERATE_GROUP, 0, M_JOBS, false, true, BUSY, NONE},
    {C_GENERATE_GROUP, 0, M_GROUP, false, true, ANY_GROUP, NONE},

    // part 1 follows the check of the allowed list's length, part 2 the LDS bound of the candidate head
    {C_GENERATE_BEAMS, 0, M_ENTROPY, false, true, ENTROPY, NOT_IN_THIS_FORM},
    {C_GENERATE_BEAMS, 0, M_SAMPLING, false, true, SAMPLING, BEAMS_GREEDY},
    {C_GENERATE_BEAMS, 1, M_PENALTY, false, true, PENALTY, BEAMS_NO_PENALTY},
    {C_GENERATE_BEAMS, 1, M_FP8_DECODE, false, true, FP8_DECODE, THEM_OFF},
    {C_GENERATE_BEAMS, 1, M_MXFP4_DECODE, false, true, MXFP4_DECODE, THEM_OFF},
    {C_GENERATE_BEAMS, 1, M_FP8_GEMM, false, true, FP8_GEMM_BEAMS, THEM_OFF},
    {C_GENERATE_BEAMS, 1, M_PERSISTENT, false, true, PERSISTENT, IT_OFF},
    {C_GENERATE_BEAMS, 1, M_MXFP4_BATCHED, false, true, MXFP4_BATCHED, THEM_OFF},
    {C_GENERATE_BEAMS, 2, M_JOBS, false, true, BUSY, NONE},
    {C_GENERATE_BEAMS, 2, M_GROUP, false, true, ANY_GROUP, NONE},

    // a forced row must be computed in the numeric scheme of the step it stands in for.  The scheduler's forced submit needs no idle
    // scheduler, and refuses svln_set_mxfp4_batched too: the decode rows a forced row stands in for would run MXFP4 products there
    {C_GENERATE_FORCED, 0, M_PENALTY, false, true, PENALTY, FLAGS_PER_ROW},
    {C_GENERATE_FORCED, 0, M_ENTROPY, false, true, ENTROPY, NOT_IN_THIS_FORM},
    SVLN_SCHEME4(C_GENERATE_FORCED, 0, SCHEME4),
    {C_GENERATE_FORCED, 0, M_JOBS, false, true, BUSY, NONE},
    {C_BATCH_SUBMIT_FORCED, 0, M_PENALTY, false, true, PENALTY, FLAGS_PER_ROW},
    {C_BATCH_SUBMIT_FORCED, 0, M_ENTROPY, false, true, ENTROPY, NOT_IN_THIS_FORM},
    SVLN_SCHEME5(C_BATCH_SUBMIT_FORCED, 0),

    // the candidates forms: these rows, then C_GENERATE_FORCED's under the form's own name
    {C_GENERATE_CANDIDATES, 0, M_TOPK, false, true, TOPK, NOT_IN_GROUPS},
    {C_GENERATE_CANDIDATES, 0, M_MXFP4_BATCHED, false, true, MXFP4_BATCHED, BATCHED_STEP},
    {C_GENERATE_CANDIDATES, 0, M_GROUP, false, true, ANY_GROUP, NONE},

    // (argmax_rows follows the engine's switches: under svln_set_sampling it would sample on whatever rows the last call staged)
    {C_OP_GEMV_BATCHED_ARGMAX, 0, M_SAMPLING, false, true, SAMPLING, OR_SAMPLE_OP},
};
#undef SVLN_DRAFTS
#undef SVLN_PLAIN_HEAD_ONLY
#undef SVLN_SCHEME4
#undef SVLN_SCHEME5
#undef SVLN_DRAFT_SETTER
constexpr int N_RULES = (int)(sizeof(RULES) / sizeof(RULES[0]));
}  // namespace mode_rows

constexpr int MODE_ALL_PARTS = -1;

// The message of the first rule of `caller` (of its part `part`, or of every part in order) that `s` violates, beginning with `who`;
// empty: the call is accepted.  no_change: the call would change nothing -- only the rules marked on_no_change hold.
inline std::string mode_refusal(Caller caller, const ModeState& s, const char* who, bool no_change = false, int part = MODE_ALL_PARTS) {
    for (const ModeRule& r : mode_rows::RULES) {
        if (r.caller != caller || (part != MODE_ALL_PARTS && r.part != part) || (no_change && !r.on_no_change)) continue;
        if (s.on(r.bit) != r.must_be_on) {
            std::string m = std::string(who) + r.what + r.tail;
            const size_t at = m.find("{env}");
            if (at != std::string::npos) m.replace(at, 5, std::to_string(s.group_env));
            return m;
        }
    }
    return std::string();
}

}  // namespace svln
