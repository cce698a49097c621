/* streamvln_hip.h -- C ABI of the MI355X-native StreamVLN streaming-inference engine.
 *
 * The reference has no FFI: its hot path sits behind the Python class
 * `StreamVLNForCausalLM` (streamvln/model/stream_video_vln.py).  This library is what sits
 * UNDER a Python class of the same shape (streamvln_amd/model.py); each entry point names the
 * reference interface it replaces.  Plain pointers and sizes only; device pointers are raw HIP
 * device addresses; no torch types.  All functions return 0 on success, < 0 on error (message
 * via svln_last_error()).  One engine = one GPU = one HIP stream; not re-entrant per engine.
 */
#ifndef STREAMVLN_HIP_H
#define STREAMVLN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svln_engine svln_engine;

enum { SVLN_BF16 = 0, SVLN_F32 = 1 };

/* Model dimensions (streamvln_amd/config.py; reference: siglip_encoder.py:73-86, Qwen2-7B). */
typedef struct svln_config {
    int32_t v_hidden, v_inter, v_heads, v_layers, v_patch, v_image;
    float v_eps;
    int32_t hidden, layers, q_heads, kv_heads, head_dim, inter, vocab;
    float rope_theta, rms_eps;
    int32_t max_positions;   /* KV / embeds capacity per env (model_max_length, streamvln_eval.py:501) */
    int32_t max_envs;        /* model.reset(env_num), stream_video_vln.py:473 */
    int32_t max_frames;      /* views per generate call: 1 + num_history */
    int32_t dtype;           /* SVLN_BF16 (shipping) or SVLN_F32 (parity mode) */
} svln_config;

/* -- lifetime: StreamVLNForCausalLM.from_pretrained(...).to(device) (streamvln_eval.py:523-533) -- */
int svln_create(const svln_config* cfg, int device, svln_engine** out);
void svln_destroy(svln_engine* h);
const char* svln_last_error(void);
int svln_sync(svln_engine* h);

/* -- weights: HF state-dict names (model.layers.N.self_attn.q_proj.weight, ...).
 * svln_synth_tensor fills a tensor on the device from the counter-based generator of
 * streamvln_amd/weights.py (seed_t = fnv1a64(name) ^ splitmix64(seed)); svln_set_tensor uploads
 * a canonical row-major tensor (host or device memory, fp32 or bf16).
 * A write may come at any time between turns, also after switches were enabled and turns have run: everything the engine derives from
 * the written tensor follows it, on the engine stream behind the write -- the 12-bit packed copy (svln_set_packed_decode), the e4m3 and
 * MXFP4 copies of the matrix if they exist (svln_set_fp8_decode / svln_set_fp8_gemm, svln_set_mxfp4_decode / svln_set_mxfp4_batched;
 * quantised again into the same buffers, so captured decode graphs stay valid), and the feature cache (svln_set_feature_cache), whose
 * entries are dropped when a tensor of the vision tower or the projector is written.  An env's rows and KV cache are session state
 * computed with the old weights: reset the envs (svln_reset_env) after a write.  Refused before anything changes, by name
 * ("svln_set_tensor cannot change while ..."): while scheduler turns are in flight, and while a group turn is pending. */
int svln_synth_tensor(svln_engine* h, const char* name, uint64_t seed_t, float half_width, float base);
int svln_set_tensor(svln_engine* h, const char* name, const void* data, int dtype, int64_t numel, int on_device);
int svln_weights_ready(svln_engine* h);            /* 0 when every tensor of the path has been provided */
int svln_get_tensor_f32(svln_engine* h, const char* name, float* host_out, int64_t numel);   /* canonical order */

/* -- session state: model.reset(env_num) / model.reset_for_env(i) (stream_video_vln.py:473-479);
 * svln_kv_reset = caller passing past_key_values=None (streamvln_eval.py:349). */
int svln_reset_env(svln_engine* h, int env);
int svln_kv_reset(svln_engine* h, int env);
int svln_env_state(svln_engine* h, int env, int32_t* n_embeds, int32_t* kv_len);
/* pages of the KV pool that no env and no pending group holds (tests: page accounting) */
int svln_kv_free_pages(svln_engine* h, int32_t* n);

/* -- vision: encode_rgbd (stream_video_vln.py:102-142) minus the memory/image split:
 * pixels fp32 [F,3,S,S] (device or host) -> F*196 pooled rows kept in the engine's frame buffer. */
int svln_encode_frames(svln_engine* h, const float* pixels, int n_frames, int on_device);

/* -- image preprocess: SigLipImageProcessor.preprocess (llava/model/multimodal_encoder/siglip_encoder.py:47-67) =
 * PIL bicubic resize of the camera frame to v_image x v_image (aspect not preserved), x/255, (x - 0.5)/0.5, channels first.
 * rgb uint8 [n_frames][height][width][3] (host memory, or device memory when on_device) -> out_dev fp32 [n_frames][3][S][S]
 * (device).  Bit-exact with Pillow's two-pass fixed-point resampler (pillow==11.2.1, requirements.txt:97); complete on return.
 * svln_preprocess_time: accumulated GPU time (upload + kernel, HIP events) and frame count since the last reset. */
int svln_preprocess_frames(svln_engine* h, const uint8_t* rgb, int n_frames, int height, int width, int on_device, float* out_dev);
/* The same work without the final wait: returns once the frame bytes have been consumed (copied to pinned staging) and the upload +
 * kernel are enqueued on the engine's stream.  svln_encode_frames / svln_generate on the same engine are ordered behind it; any other
 * stream that touches out_dev must first wait on the engine's stream (svln_engine_stream: the hipStream_t as a void*).
 * Lifetime of rgb: with on_device = 0 the bytes have been copied when the call returns and the caller may reuse the buffer.  With
 * on_device = 1 the engine's stream reads the caller's DEVICE buffer asynchronously: it must stay allocated and unmodified until the
 * work enqueued here has run (wait on svln_engine_stream, or call svln_sync), and whatever stream produced it must have finished --
 * or the engine's stream must have been ordered behind it -- before this call. */
int svln_preprocess_frames_enqueue(svln_engine* h, const uint8_t* rgb, int n_frames, int height, int width, int on_device, float* out_dev);
int svln_engine_stream(svln_engine* h, void** stream);
/* Engine-owned frame ring: `slots` frames of height x width x 3 bytes in pinned, device-mapped host memory (*host_base, slots
 * *slot_stride bytes apart, 256-byte aligned).  The camera / simulator side writes its RGB frames into the slots; a frame passed to
 * svln_preprocess_frames[_enqueue] (on_device = 0) whose bytes lie inside the ring is read by the GPU where it is -- the staging copy on
 * the host (921 KB per 640x480 frame) disappears.  Any other host pointer takes the staging path as before.  A slot may be rewritten
 * once the upload that last read it has run: svln_frame_ring_wait(slot) returns when that is the case (immediately if none is pending).
 * A second call replaces the ring (the old memory is freed). */
int svln_frame_ring(svln_engine* h, int slots, int height, int width, uint8_t** host_base, int64_t* slot_stride);
int svln_frame_ring_wait(svln_engine* h, int slot);
int svln_preprocess_time(svln_engine* h, double* gpu_ms, int64_t* frames, int reset);

/* -- splice: prepare_inputs_labels_for_multimodal (stream_video_vln.py:182-238) for one env.
 * ids hold text tokens and the sentinels -200 (<image>) / -300 (<memory>); the first n_memory frames
 * of the last svln_encode_frames call form the memory block, the rest are consumed by <image> in order.
 * Rows are appended to the env's inputs_embeds (stream_video_vln.py:396-401). */
int svln_append_turn(svln_engine* h, int env, const int64_t* ids, int n_ids, int n_memory);
/* config.tokenizer_model_max_length of the reference (stream_video_vln.py:241-244): the spliced rows of ONE turn are truncated to
 * `rows` before they are appended (new_input_embeds[:tokenizer_model_max_length]).  0 = no truncation (the attribute is None, the
 * reference's default).  Independent of max_positions, the capacity of the accumulated sequence, which the reference does not have:
 * exceeding it is an error ("inputs_embeds exceeds max_positions"). */
int svln_set_turn_row_limit(svln_engine* h, int rows);

/* -- greedy generation: StreamVLNForCausalLM.generate -> GenerationMixin (do_sample=False, num_beams=1):
 * prefill embeds[kv_len:], arg-max, feed generated ids until one is in eos_ids (appended, not fed) or
 * max_new_tokens; afterwards kv_len = n_embeds + n_out - 1. */
int svln_generate(svln_engine* h, int env, int max_new_tokens, const int64_t* eos_ids, int n_eos, int64_t* out_ids,
                  int out_cap, int32_t* n_out);
/* -- ONE call per model turn: what StreamVLNForCausalLM.generate does between the harness's call and its return
 * (stream_video_vln.py:353-407) = svln_encode_frames(pixels) ; new_window (the caller passed past_key_values=None): svln_kv_reset ;
 * new_episode (curr_t == 0) and the env holds rows: svln_reset_env ; svln_append_turn(ids, n_memory) ; svln_generate.  *kv_len (optional)
 * = the env's cache length afterwards (the KV handle the Python class hands back).  Same results and errors as the five calls. */
typedef struct svln_turn_args {
    const float* pixels; int32_t n_frames; int32_t pixels_on_device;     /* fp32 [n_frames,3,S,S] */
    int32_t env;
    const int64_t* ids; int32_t n_ids; int32_t n_memory;                /* text ids + sentinels; first n_memory frames = <memory> block */
    int32_t new_window, new_episode;
    int32_t max_new_tokens;
    const int64_t* eos_ids; int32_t n_eos;
} svln_turn_args;
int svln_turn(svln_engine* h, const svln_turn_args* a, int64_t* out_ids, int out_cap, int32_t* n_out, int32_t* kv_len);
/* generation_config.repetition_penalty of a checkpoint: transformers' RepetitionPenaltyLogitsProcessor -- applied by
 * GenerationMixin under greedy decoding too -- on the fp32 logits of every step, over the ids generated so far in the turn (the prompt is
 * passed as inputs_embeds, so it has no ids): logit < 0 ? logit * penalty : logit / penalty.  1 = off (default).  Applies to svln_generate,
 * svln_generate_batch and the scheduler; cannot change while scheduler turns are in flight. */
int svln_set_repetition_penalty(svln_engine* h, float penalty);
/* perf harness variant: decode exactly n_tokens regardless of EOS */
int svln_generate_fixed(svln_engine* h, int env, int n_tokens, int64_t* out_ids);

/* -- multi-env lockstep turns (SURVEY.md 8f-1 / BASELINE configs[4]; build-side extension, the reference runs batch 1):
 * svln_append_turn_at = svln_append_turn with the env's frames starting at `frame_base` of the last svln_encode_frames
 * call (several envs' frames encoded together); svln_generate_batch = svln_generate on each listed env (<= 8, distinct),
 * executed together: dense layers of all prefill rows at once, then batched decode steps that stream each weight matrix
 * once per step for all still-active envs.  out_ids is [n_envs][out_cap], n_out is [n_envs]. */
int svln_append_turn_at(svln_engine* h, int env, const int64_t* ids, int n_ids, int frame_base, int n_memory);
int svln_generate_batch(svln_engine* h, const int32_t* envs, int n_envs, int max_new_tokens, const int64_t* eos_ids, int n_eos,
                        int64_t* out_ids, int out_cap, int32_t* n_out);
/* -- the scheduler underneath svln_generate_batch, for callers whose envs' turns fall due at DIFFERENT times (a DAgger-style
 * collector mixing expert and model steps per env, streamvln_dagger.py:232-313): iteration-level batching.
 * svln_batch_submit: the env (turn already appended with svln_append_turn[_at]) joins the next iteration; *slot identifies the turn.
 * svln_batch_step: ONE pass over the weights carrying, for every turn in flight, either its prefill rows or the row of the token it
 * generated in the previous iteration (prefilling and decoding envs share the pass); *running = turns still in flight afterwards,
 * finished_slots[0 .. *n_finished) = turns that emitted EOS / max_new_tokens in this iteration (<= 8 entries).
 * svln_batch_result: ids of a finished turn (frees the slot).  Per-env results are exactly those of svln_generate. */
int svln_batch_submit(svln_engine* h, int env, int max_new_tokens, const int64_t* eos_ids, int n_eos, int32_t* slot);
int svln_batch_step(svln_engine* h, int32_t* running, int32_t* finished_slots, int32_t* n_finished);
int svln_batch_result(svln_engine* h, int slot, int32_t* env, int64_t* out_ids, int out_cap, int32_t* n_out);
/* Drop the turn in `slot` (slot < 0: every turn in flight), finished or not; its slot is free again.  svln_reset_env / svln_kv_reset drop
 * the env's turn themselves.  A svln_batch_step that fails part-way drops every turn in flight before it returns the error (a turn whose
 * env has no rows left to prefill is dropped alone), so the scheduler is always usable after an error. */
int svln_batch_cancel(svln_engine* h, int slot);
int svln_get_hidden_batch(svln_engine* h, int slot, float* host_out, int max_rows, int32_t* n_rows);   /* parity tap, <= 8 rows */

/* -- parity taps (test infrastructure reads these; not used by the product path) */
int svln_get_hidden(svln_engine* h, float* host_out, int max_rows, int32_t* n_rows);  /* final-norm hidden per generated token of the last generate */
int svln_get_embeds(svln_engine* h, int env, int start_row, int n_rows, float* host_out);
int svln_get_frame_feats(svln_engine* h, int start_row, int n_rows, float* host_out);
int svln_get_top2(svln_engine* h, float* host_out2);       /* refused when the last token of the last turn came from a verify pass (svln_set_speculative) or a ride (svln_set_prefill_draft) */
/* Opt-in, default off, no reference counterpart: token log-probabilities.  While on, every lm_head product runs a sibling kernel that
 * computes the arg-max exactly as before (same accumulators, compare order and partials: the ids are bit-identical) and, beside every
 * arg-max partial, sum exp(l - partial max) over the logits the partial owns; the final arg-max kernel merges the partials,
 * S = sum_k part_sum[k] * exp(part_val[k] - V), and writes logprob = -log S = l_t - logsumexp_j(l_j) of the emitted token t over the
 * PROCESSED fp32 logits (after the repetition penalty, as HF's `scores`).  No logit reaches memory and the lm_head is not read twice;
 * the scores travel in the synchronisation that already reads the ids.  A NaN logit makes that token's score NaN; so does token -1.
 * Works with svln_set_fp8_decode, svln_set_mxfp4_decode (the quantised lm_heads), svln_set_fp8_gemm / svln_set_fp8_scaled_mfma and the
 * repetition penalty.  Refused, and each of these refused while it is on: svln_set_speculative, svln_set_prefill_draft,
 * svln_set_batch_draft (their tokens leave the verify step, which carries no scores), svln_set_decode_persistent and
 * svln_set_mxfp4_batched (its lm_head kernel has no scored form).  A change is refused while scheduler turns are in flight; a call that
 * changes nothing always succeeds.  Captured decode graphs are dropped when it changes.
 * svln_get_token_scores: the scores of the last svln_generate / svln_turn / svln_generate_fixed, *n = the number of ids it returned
 * (out receives min(*n, cap) of them).  svln_batch_scores: those of the finished scheduler turn in `slot`, valid until svln_batch_result
 * frees the slot.  svln_generate_batch_scores: those of env index `index` (its place in the envs list) of the last svln_generate_batch.
 * All three fail, with svln_last_error saying so, when the switch was off for that turn. */
int svln_set_token_scores(svln_engine* h, int enable);
/* Opt-in, default off, no reference counterpart: temperature sampling.  While on, every lm_head product runs a sibling kernel
 * (EPI_SAMPLE) and token t of an env is  argmax_n ( fl(x_n * invT) + G(seed, stream, draw, n) ),  lowest column on ties, -1 for a row
 * with no finite value: by the Gumbel-max identity an exact sample of softmax(x / T).  x_n is the PROCESSED fp32 logit (after the
 * repetition penalty: processors before warpers, as HF), invT = fl(1 / temperature) computed once on the host, stream = the engine env
 * slot, draw = the number of tokens that env has emitted since the last svln_set_sampling call.  The noise is a pure function of
 * (seed, stream, draw, column) -- Philox4x32-10 on counter (column, draw, stream, 0) and key (seed lo, seed hi), output word 0 = w;
 * u = ((w >> 9) + 0.5) * 2^-23; G = -ln(-ln u) -- so svln_generate, svln_generate_batch and the scheduler emit the same ids for the
 * same seed wherever their logits agree.  No logit reaches memory and the lm_head is not read twice.
 * The sampled kernels also compute log softmax(x / T)[token]; it is delivered through the svln_set_token_scores getters while that
 * switch is on (HF's `scores` under sampling).
 * enable != 0 requires a finite temperature > 0.  EVERY call, on or off, resets every env's draw counter to 0 and drops the captured
 * decode graphs; it is refused while scheduler turns are in flight.  Works with svln_set_fp8_decode, svln_set_mxfp4_decode,
 * svln_set_fp8_gemm / svln_set_fp8_scaled_mfma, the repetition penalty, svln_set_token_scores, svln_set_memory_prune and
 * svln_set_feature_cache.  Refused, and each of these refused while it is on: svln_set_speculative, svln_set_prefill_draft,
 * svln_set_batch_draft (their verify rule is written for greedy rows), svln_set_decode_persistent and svln_set_mxfp4_batched (its
 * lm_head kernel has no sampled form).  svln_get_top2 is refused after a sampled turn: the values are perturbed, not logits. */
int svln_set_sampling(svln_engine* h, int enable, float temperature, uint64_t seed);
/* Opt-in, default off (top_k = 0, top_p = 1), no reference counterpart: truncated sampling -- top-k then top-p over the lm_head's
 * candidate lists.  While top_k is 1 .. 8 every lm_head product of a sampled pass (svln_generate / svln_turn / svln_generate_fixed,
 * svln_generate_batch, the scheduler, group turns) runs its candidate form (the EPI_SAMPLE_TOPK kernels of svln_top_logprobs, lists on
 * or off; under svln_set_allowed_tokens the subset product's partials are the candidates) and one small kernel per head pass applies,
 * per row, HF's warpers in HF's order -- temperature, top-k, top-p -- on y_n = fl(x_n * invT):
 *   1. the k' = min(top_k, listable columns) best (y, column) pairs, y descending then column ascending (NaN and -inf are never listed).
 *      At an exact tie on the k-th value HF's TopKLogitsWarper keeps every tied column; this engine keeps exactly k, lowest columns first;
 *   2. e_j = exp(y_j - y_0), c_j = c_{j-1} + e_j (fp32, serially), total = c_{k'-1}: entry 0 is kept, entry j >= 1 is kept iff top_p >= 1
 *      or c_{j-1} < fl(top_p * total) -- HF's TopPLogitsWarper over the top-k set: keep an id iff the mass strictly before it is below top_p;
 *   3. token = argmax over the kept j of fl(y_j + G(seed, stream, draw, column_j)), the noise and the expression of svln_set_sampling:
 *      whenever the untruncated sampled token lies in the kept set the truncated turn emits that token, bit for bit -- a truncated turn
 *      is the full sampled turn conditioned on the kept set, as an allowed list is.  One draw per emitted id, as without truncation;
 *   4. the score (svln_set_token_scores) is the log-softmax over the kept set at the emitted id -- HF's `scores` after the warpers -- and
 *      under svln_top_logprobs the lists are over the kept set, padded with (-1, -inf) beyond it; the emitted id's entry is the score's bits.
 *      svln_get_allowed_logprobs rows stay the untruncated log-softmax over the allowed list.
 * The name is deliberately not svln_set_*: this is an attribute of svln_set_sampling, not an independent row of the switch-pair table the
 * tests keep for every svln_set_* prototype (the decision svln_top_logprobs made).  svln_set_sampling(h, 0, ..) clears it,
 * svln_set_sampling(h, 1, ..) keeps it; every mode sampling refuses is thereby unreachable.  Refused, before any launch or state change:
 * top_k outside 0 .. 8; top_p not in (0, 1] (NaN included); top_k = 0 with top_p < 1 (naming top_k: a nucleus is taken over at most 8
 * listed ids); sampling off (naming svln_set_sampling); scheduler turns in flight; a group pending; a hidden size too large for the
 * candidate form of the lm_head GEMV.  Composes with svln_set_token_scores, svln_top_logprobs, svln_set_allowed_tokens, the repetition
 * penalty, svln_set_fp8_decode / svln_set_mxfp4_decode / svln_set_packed_decode (candidates of their own formats), svln_set_fp8_gemm,
 * group turns and graph replay (captured steps are dropped when the setting changes; top_k / top_p are launch scalars).  Forced turns
 * are unchanged: they score softmax(x / T) untruncated.  With truncation off every launch is what ran before. */
int svln_sampling_truncation(svln_engine* h, int32_t top_k, float top_p);
/* Opt-in, default off (k = 0), no reference counterpart: top-k log-probabilities -- what else the policy considered.  While k is 1 .. 8
 * every lm_head product (the single-env GEMV of svln_generate / svln_turn / svln_generate_fixed, the batched GEMV and the 32 x 128 MFMA
 * tiles of svln_generate_batch and the scheduler) runs the sibling of its scored or sampled kernel that also keeps, beside every arg-max
 * partial, the partial's 8 best (y, column) pairs, and one small merge kernel per head pass writes the k best of every row.  With x_n the PROCESSED fp32 logit (after the repetition penalty), y_n = x_n under greedy decoding and
 * y_n = fl(x_n * invT) under svln_set_sampling (the unperturbed value, never y + noise).  The list is ordered y descending, then column
 * ascending; NaN and -inf are never listed; a row with fewer than k listable columns is padded with (id -1, logprob -inf);
 * logprob_j = (y_j - V) - log S with (V, S) the merge the scored kernels compute.  Hence under greedy decoding entry 0 is the emitted id
 * and its log-probability is the bits of svln_get_token_scores; under sampling the emitted id's entry, when listed, is.  Tokens, scores
 * and every partial are bit-identical to k = 0: same accumulators, same compares.  No logit reaches memory and the lm_head is not read
 * twice.  Under svln_set_allowed_tokens the list is over the allowed set (k > n_allowed: the rest is padding).
 * The name is deliberately not svln_set_*: the switch is tied to svln_set_token_scores and is no independent row of the switch-pair
 * table the tests keep for every svln_set_* prototype.  Rules, in force only for k > 0: refused while svln_set_token_scores is off
 * (naming it), and svln_set_token_scores(0) is refused while k > 0 (naming svln_top_logprobs) -- so every mode the scores refuse
 * (the draft switches, svln_set_decode_persistent, svln_set_mxfp4_batched) is unreachable.  Composes with svln_set_fp8_decode /
 * svln_set_mxfp4_decode / svln_set_packed_decode (the lists are of their own lm_head formats), svln_set_fp8_gemm /
 * svln_set_fp8_scaled_mfma, the repetition penalty, svln_set_sampling, svln_set_allowed_tokens and graph replay (captured decode graphs
 * are keyed by k and dropped when it changes).  Refused: k outside 0 .. 8; a change while scheduler turns are in flight or a group is
 * pending; k > 0 while svln_token_entropy is on (naming it); and, while k > 0, svln_generate_group / svln_turn_group and the candidates
 * forms (naming svln_top_logprobs: group turns carry no lists).  The scheduler and svln_generate_batch carry lists (svln_batch_topk,
 * svln_generate_batch_topk).  A forced turn runs as before and produces no lists; a beam turn runs its own k = n_beams head.  A call
 * that changes nothing succeeds, but for a pending group.  The rule table behind svln_mode_refusal is the reference for all of this.
 * svln_get_topk: the lists of the last single-env turn, ids [n_rows][k] int32 and logprobs [n_rows][k] fp32 (min(n_rows, cap_rows) rows
 * are written), read in the synchronisation that reads the ids; refused when k was 0 for that turn, after a forced turn, or before any. */
int svln_top_logprobs(svln_engine* h, int k);
int svln_get_topk(svln_engine* h, int32_t* host_ids, float* host_logprobs, int cap_rows, int32_t* n_rows, int32_t* k);
/* ... those of the finished scheduler turn in `slot` (valid until svln_batch_result frees the slot), and of env index `index` of the
 * last svln_generate_batch; both refused when k was 0 for that turn. */
int svln_batch_topk(svln_engine* h, int slot, int32_t* host_ids, float* host_logprobs, int cap_rows, int32_t* n_rows, int32_t* k);
int svln_generate_batch_topk(svln_engine* h, int index, int32_t* host_ids, float* host_logprobs, int cap_rows, int32_t* n_rows, int32_t* k);
/* Opt-in, default off, no reference counterpart: token entropies -- how spread the policy's distribution was at every emitted id.
 * While on, every lm_head product (the single-env GEMV in all four weight formats, the batched GEMV and the 32 x 128 MFMA tiles) runs
 * the sibling of its scored or sampled kernel that keeps, beside every partial's (max m, sum s = sum exp(y - m)), one more fp32
 * t = sum (y - m) exp(y - m), and one small merge kernel per head pass writes H = log S - T / S in nats, fp32, with (V, S) the very merge
 * the scored kernels compute and T = sum_n (y_n - V) exp(y_n - V) merged like S.  y_n is the PROCESSED fp32 logit x_n (after the
 * repetition penalty) under greedy decoding and fl(x_n * invT) under svln_set_sampling (the unperturbed value, never y + noise).  A -inf
 * column adds 0; a NaN logit makes the row's entropy NaN; a row without a finite value (token -1) gives NaN; a one-column row gives
 * exactly 0.  Under svln_set_allowed_tokens the entropy is over the allowed set.  Tokens, scores, hidden rows, cache lengths and every
 * existing partial are bit-identical to the switch off: same accumulators, same compares, same orders; with the switch off every launch
 * is the kernel that ran before.  No logit reaches memory and the lm_head is not read twice.
 * The name is deliberately not svln_set_*: like svln_top_logprobs the switch is tied to svln_set_token_scores and is no independent row
 * of the switch-pair table the tests keep for every svln_set_* prototype.  Rules: switching on is refused while svln_set_token_scores
 * is off (naming it), and svln_set_token_scores(0) is refused while on (naming svln_token_entropy) -- so every mode the scores refuse
 * (the draft switches, svln_set_decode_persistent, svln_set_mxfp4_batched) is unreachable.  Composes with svln_set_fp8_decode /
 * svln_set_mxfp4_decode / svln_set_packed_decode (the entropy is of their own lm_head formats), svln_set_fp8_gemm /
 * svln_set_fp8_scaled_mfma, the repetition penalty, svln_set_sampling without truncation, svln_set_allowed_tokens, graph replay (captured
 * decode graphs are keyed by the switch and dropped when it changes), svln_generate / svln_turn, svln_generate_batch and the scheduler's
 * plain turns.  Refused both ways, naming the other function: svln_top_logprobs with k > 0 and svln_sampling_truncation with top_k > 0
 * (their epilogues are the candidate siblings, which have no entropy form yet).  Refused while on, naming svln_token_entropy: group,
 * beam, candidate and forced turns and svln_batch_submit_forced.  Refused: a change while scheduler turns are in flight or a group is
 * pending.  A call that changes nothing succeeds.
 * svln_get_token_entropy: the entropies of the last single-env turn, one per emitted id (min(n, cap) are written), read in the
 * synchronisation that reads the ids; refused when the switch was off for that turn, after a forced turn, or before any.
 * svln_batch_entropy / svln_generate_batch_entropy: those of the finished scheduler turn in `slot` (valid until svln_batch_result frees
 * the slot) and of env index `index` of the last svln_generate_batch; both refused when the switch was off for that turn. */
int svln_token_entropy(svln_engine* h, int enable);
int svln_get_token_entropy(svln_engine* h, float* host_out, int cap, int32_t* n);
int svln_batch_entropy(svln_engine* h, int slot, float* host_out, int cap, int32_t* n);
int svln_generate_batch_entropy(svln_engine* h, int index, float* host_out, int cap, int32_t* n);
int svln_get_token_scores(svln_engine* h, float* host_out, int cap, int32_t* n);
int svln_batch_scores(svln_engine* h, int slot, float* host_out, int cap, int32_t* n);
int svln_generate_batch_scores(svln_engine* h, int index, float* host_out, int cap, int32_t* n);
/* Opt-in, default off: allowed-token decode (HF's prefix_allowed_tokens_fn with a constant set; vLLM's allowed_token_ids).  ids[0 .. n) is
 * the allowed list A = a_0 < a_1 < ... < a_{n-1}, 1 <= n <= 256, every id in [0, vocab); n == 0 switches it off.  While set, EVERY lm_head
 * product of the engine (svln_generate / svln_turn, svln_generate_batch, the scheduler, verify passes, rides) is the product over the
 * listed rows only: x_a = the fp32 dot of lm_head row a with the final-norm row (elements converted to fp32, fp32 fmaf, 16-byte chunks per
 * lane, a summation order that depends on the hidden size alone -- not on the row count, the list or a's place in it, so the same pair
 * gives the same bits on every path).  It reads the engine-dtype lm_head (bf16 or fp32) whichever weight-format switch is on: a product
 * of <= 256 rows gains nothing from the e4m3 / MXFP4 copies, and one format makes the head the same function everywhere.
 * Repetition penalty: as before, on the flag of the vocabulary id.  Greedy: token = argmax over A, lowest id on ties, -1 when no allowed
 * id has a finite value (NaN and -inf never win).  Sampling (svln_set_sampling): y_a = fl(x_a * invT), z_a = y_a + G(seed, stream, draw,
 * a) -- the noise column is the vocabulary id, so the turn is the full-vocabulary sampled turn conditioned on A, with the same noise.
 * Scores (svln_set_token_scores): log softmax over the processed logits OF THE SET at the emitted id (HF's semantics with -inf elsewhere).
 * The list is taken as given: without an EOS id in it a turn ends at max_new_tokens.
 * Refused before any launch or state change (svln_last_error says which): n > 256 or n < 0, an id outside the vocabulary, a list that is
 * not strictly ascending, a null list with n > 0, any call while scheduler turns are in flight.  A call that repeats the current list
 * succeeds and changes nothing; a change synchronises the stream and drops the captured decode graphs.  Composes with every other
 * switch: only the lm_head product is swapped, every existing refusal stays as it is.
 * While svln_set_token_scores is on as well, the whole distribution over A of every emitted token is kept:
 * allowed_logprobs[t][j] = y_j - logsumexp_i y_i (y = x after the penalty; x * invT under sampling); a NaN logit makes that row NaN.  It
 * travels in the synchronisation that already reads ids and scores.  svln_get_allowed_logprobs / svln_batch_allowed_logprobs /
 * svln_generate_batch_allowed_logprobs: lifetimes of the three score getters above; *n_tokens rows of *n_ids floats each, host_out
 * receives min(*n_tokens * *n_ids, cap_floats) of them; each fails when the scores or the list were off for that turn. */
int svln_set_allowed_tokens(svln_engine* h, const int64_t* ids, int n);
int svln_get_allowed_logprobs(svln_engine* h, float* host_out, int cap_floats, int32_t* n_tokens, int32_t* n_ids);
int svln_batch_allowed_logprobs(svln_engine* h, int slot, float* host_out, int cap_floats, int32_t* n_tokens, int32_t* n_ids);
int svln_generate_batch_allowed_logprobs(svln_engine* h, int index, float* host_out, int cap_floats, int32_t* n_tokens, int32_t* n_ids);
/* Opt-in, no reference counterpart (HF: num_return_sequences under do_sample): a GROUP turn -- n_seq (2 .. 8) independently sampled
 * continuations of ONE prefill of env's turn.  With L = n_embeds, limit = min(max_new_tokens, out_cap), q0 = L / 64 and B = the next power
 * of two >= n_seq:
 *   prefill   exactly svln_generate's (same launches, same K / V bits for positions < L);
 *   token 0   the last prefill row replicated B times through the scheduler's batched lm_head; row g samples with
 *             stream = env + g * max_envs and draw = the env's draw counter (stream 0 is the env's own: sequence 0 is what svln_generate
 *             would have sampled wherever the two paths' logits agree; no stream collides with another env's);
 *   fork      sequence 0 keeps the env's page table; sequence g >= 1 gets a table whose entries [0, q0) are the env's pages (shared, never
 *             written: every write of the turn is at a position >= L) and whose n_tail = ceil((L + limit - 1) / 64) - q0 further entries
 *             (0 when limit == 1) are fresh pages of the free pool; if L % 64 != 0 ONE launch (kv_page_copy_kernel) copies the env's partly
 *             filled page q0 to the n_seq - 1 fresh q0 pages in every layer's K and V^T pool, else nothing is launched;
 *   decode    up to limit - 1 iterations of the scheduler's pure batched decode step at B rows (the same launches or captured graph),
 *             row g = {table g, position L + t, g's last token}, draws = counter + t + 1, one synchronisation each; the host applies the
 *             stop rule per sequence (an EOS id, limit, a non-finite arg-max); a finished sequence's row and every pad row replay the first
 *             live row (identical writes).
 * The head and the products are whatever the batched step runs under the switches in force (svln_set_fp8_gemm, svln_set_allowed_tokens,
 * ...): a group computes what svln_generate_batch would compute for n_seq envs holding this prompt.  Which scheme each phase runs:
 * the prefill is bf16, or e4m3 under svln_set_fp8_gemm; token 0 and every decode iteration are the batched lm_head and the batched
 * decode step on the bf16 weights (e4m3 products at B >= 4 under svln_set_fp8_gemm), whatever svln_set_fp8_decode or
 * svln_set_mxfp4_decode says: those two switch the single-env decode step and its lm_head, which a group never runs, so under either
 * of them a group returns the bits it returns with both off.  out_ids [n_seq][out_cap], n_out [n_seq].
 * Afterwards the env's draw counter has advanced by max_g n_out[g] (no (stream, draw) pair is ever used twice), its kv length is L and the
 * group is PENDING on it: svln_group_select must say which continuation the env goes on with.  While a group is pending,
 * svln_append_turn*, svln_generate*, svln_turn*, svln_batch_submit and svln_generate_batch on that env fail with a message that names
 * svln_group_select; svln_reset_env / svln_kv_reset drop the group and free its pages; svln_set_sampling, svln_set_token_scores and
 * svln_set_allowed_tokens fail, as they do while scheduler turns are in flight.
 * Refused before any launch or state change: svln_set_speculative, svln_set_prefill_draft, svln_set_batch_draft,
 * svln_set_decode_persistent or svln_set_mxfp4_batched on (svln_set_sampling is refused under each of them; the message names the
 * one that is on); sampling off (greedy sequences would be identical); a repetition penalty != 1; scheduler
 * turns in flight; a group pending on any env; n_seq outside 2 .. 8; nothing to prefill; L + limit - 1 > max_positions; a free pool that
 * cannot hold the env's own missing pages plus (n_seq - 1) * n_tail.  An error after the fork returns every fork page to the pool, leaves
 * no group pending and the env as after a failed svln_generate. */
int svln_generate_group(svln_engine* h, int env, int n_seq, int max_new_tokens, const int64_t* eos_ids, int n_eos, int64_t* out_ids, int out_cap,
                        int32_t* n_out);
/* svln_turn's bookkeeping (encode, window / episode resets, splice), then the group turn, in one crossing */
int svln_turn_group(svln_engine* h, const svln_turn_args* a, int n_seq, int64_t* out_ids, int out_cap, int32_t* n_out);
/* Beam turn: the n_beams (1 .. 8) most probable turns of env's prompt in ONE prefill.  limit = min(max_new_tokens, out_cap).  The set of
 * at most n_beams hypotheses is kept in rank order; a step pools every finished hypothesis (score unchanged) with every listable entry
 * (rank r, entry j) of the top-n_beams list of every live one (score fl(score_r + lp), lp as svln_top_logprobs defines it under greedy
 * decoding) and keeps the best n_beams by score descending, then r, then j ascending; a hypothesis is finished when its last id is in the
 * EOS set (appended, never fed) or its length equals limit; no length penalty.  n_beams = 1 is the greedy turn.
 *   out_ids [n_beams][out_cap], n_out [n_beams] (0 for ranks the set does not hold), scores [n_beams] (fp32 sum of the log-probabilities).
 * The prefill, the fork of the partly filled page and the batched step are svln_generate_group's; the head of every step is the top-k
 * form at k = n_beams whatever svln_set_token_scores / svln_top_logprobs say.  The call leaves a pending group turn: sequence g = rank g
 * owns exactly the pages that hold its rows; svln_group_select (kv_len = L + n_g - 1), svln_group_logprobs, svln_get_hidden_group, the
 * resets work as after svln_generate_group.  Needs env_need + (2 n_beams - 1) x n_tail free pages.  An armed draft is consumed.
 * Refused by name before any launch or state change: n_beams outside 1 .. 8, sampling on, an allowed list shorter than n_beams, a
 * repetition penalty != 1, svln_set_fp8_decode / svln_set_mxfp4_decode / svln_set_fp8_gemm / svln_set_decode_persistent /
 * svln_set_mxfp4_batched on, scheduler turns in flight, a group pending, nothing to prefill, L + limit - 1 > max_positions, more
 * than 8 tail pages, a pool that cannot hold the tails. */
int svln_generate_beams(svln_engine* h, int env, int n_beams, int max_new_tokens, const int64_t* eos_ids, int n_eos, int64_t* out_ids, int out_cap,
                        int32_t* n_out, float* scores);
/* svln_turn (encode, bookkeeping, splice) followed by svln_generate_beams */
int svln_turn_beams(svln_engine* h, const svln_turn_args* a, int n_beams, int64_t* out_ids, int out_cap, int32_t* n_out, float* scores);
/* The steps of the last beam turn, for tests: *n_steps, *width = n_beams; for step s < min(*n_steps, cap_steps): list_ids / list_lps
 * [s][8][8] = the list of head row r (= rank r before the step; step 0: row 0 only; -1 / -inf = none; rows of finished ranks replay the
 * first live row) and records [s][28] = the record of svln_op_beam_select. */
int svln_beam_trace(svln_engine* h, int cap_steps, int32_t* n_steps, int32_t* width, int32_t* list_ids, float* list_lps, int32_t* records);
/* The env goes on with sequence `index` of its pending group: for index >= 1 its table entries [q0, q0 + n_tail) become that sequence's
 * private pages and its former pages at those entries go back to the free pool; every other fork's pages go back too.  The env's kv
 * length becomes L + n_out[index] - 1 (-> *kv_len_out, may be null).  Refused: no group pending on env, index outside [0, n_seq). */
int svln_group_select(svln_engine* h, int env, int index, int32_t* kv_len_out);
/* Results of the pending group, valid until its select (or drop): the log-probability of every id of sequence `index` (refused when
 * svln_set_token_scores was off for the turn); its rows over the allowed set, [n_rows][n_cols] (refused unless the scores and a list were
 * on); the final-norm row of each of its first <= 8 tokens (a parity tap). */
int svln_group_logprobs(svln_engine* h, int index, float* host_out, int cap, int32_t* n);
int svln_group_dist(svln_engine* h, int index, float* host_out, int cap_rows, int32_t* n_rows, int32_t* n_cols);
int svln_get_hidden_group(svln_engine* h, int index, float* host_out, int max_rows, int32_t* n_rows);
/* Opt-in, no reference counterpart: a FORCED turn -- the turn's ids F[0 .. n), 1 <= n <= 32, come from the caller.  With L = n_embeds and
 * Tn = L - kv_len, ONE prefill pass of Tn + n - 1 rows feeds F[0 .. n - 1) behind the prompt at positions L .. L + n - 2 (the ride's
 * gather, RoPE, KV append and causal attention; the last id is never fed), the final norm of the last n rows goes to the tap rows
 * (svln_get_hidden: n rows), one lm_head product in its EPI_TARGET form -- the scored partials plus the logit of column F[i] of row i,
 * captured while the logits are in registers -- and one final kernel give, per position i:
 *   logprobs[i]         log softmax(logits_i)[F[i]]: the policy's log-probability of F[i] given the prompt and F[0 .. i)
 *   greedy_ids[i]       the policy's own arg-max there, greedy_logprobs[i] its log-probability (the value a scored turn reports)
 * There is no decode launch, no [n, vocab] tensor, and one synchronisation.  Head rows: n <= 2 -> the batched GEMV at B = 2, n >= 3 -> the
 * 32-row MFMA tiles (n = 3 padded to 4); pad rows carry target -1.  Afterwards kv_len = L + n - 1 (-> *kv_len, may be null) and the loop
 * state is what a plain turn that emitted F leaves, so the next turn -- plain, ridden, sampled or grouped -- needs nothing special.
 * svln_set_token_scores may be on or off: the call launches its own instantiations and never reads that switch; svln_get_token_scores
 * returns logprobs afterwards.  With svln_set_sampling on the scores are of softmax(logits / T), as a sampled turn reports them; no noise
 * is evaluated and the env's draw counter does not move.  With svln_set_allowed_tokens on the head is the subset product, every F[i] must
 * be in the list, logprobs[i] is bit-equal to row i of svln_get_allowed_logprobs at F[i]'s list position, and greedy_* are over the list.
 * svln_get_top2 is refused afterwards, as after a ride.  An armed draft is consumed by the call -- also by a call that is refused
 * (svln_generate's rule: the one exception to "before any state change" below).  The draft switches may be on (no verify
 * rule runs), svln_set_mxfp4_batched too (scheduler paths only).
 * Refused before any launch or state change: everything svln_generate refuses (a pending group, nothing to prefill, ...); n outside
 * 1 .. 32; an id outside the vocabulary; an id of the EOS set anywhere but last (an EOS is appended, never fed); L + n - 1 >
 * max_positions; a repetition penalty != 1 (its flags change row by row); svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm
 * or svln_set_decode_persistent on (a forced row must be computed in the numeric scheme of the step it stands in for: the list the
 * draft switches refuse, without svln_set_mxfp4_batched, which only the scheduler paths read and a forced turn never runs); scheduler
 * turns in flight; an id outside the allowed list. */
int svln_generate_forced(svln_engine* h, int env, const int64_t* ids, int n, const int64_t* eos_ids, int n_eos, float* logprobs,
                         int64_t* greedy_ids, float* greedy_logprobs, int32_t* kv_len);
/* svln_turn's bookkeeping (encode, window / episode resets, splice), then the forced turn, in one crossing (a->max_new_tokens is not read).
 * The refusals that need no state of the env come before a frame is encoded; those that depend on the spliced length (nothing to prefill,
 * L + n - 1 > max_positions) come after the splice, as svln_turn's own do. */
int svln_turn_forced(svln_engine* h, const svln_turn_args* a, const int64_t* ids, int n, float* logprobs, int64_t* greedy_ids,
                     float* greedy_logprobs, int32_t* kv_len);
/* Opt-in, no reference counterpart: CANDIDATE scoring -- n_seq (2 .. 8) caller-given continuations F_g[0 .. n_g), 1 <= n_g <= 32, of ONE
 * prompt, scored in one prefill and ceil(max_g (n_g - 1) / r) scoring passes.  ids holds the sequences back to back (sum_g n_g ids), lens
 * their lengths; logprobs / greedy_ids / greedy_logprobs are laid out like ids and defined per position as by svln_generate_forced.
 *   prefill   svln_generate's, launch for launch: Tn = L - kv_len rows, nothing appended behind the prompt (L = n_embeds).
 *   fork      the group turn's: sequence 0 keeps the env's table; sequence g >= 1 with n_g >= 2 gets the env's pages below q0 = L / 64 and
 *             fresh pages covering positions up to L + n_g - 1; the partly filled page is copied by one launch when L % 64 != 0.
 *   passes    r = min(32 / (q_heads / kv_heads), 32 / n_seq).  Pass p feeds F_g[p r .. min((p + 1) r, n_g - 1)) of every sequence as the
 *             row slots [g r, g r + r) at positions L + p r + i through ONE sweep of the batched step's products (the 32-row MFMA tiles
 *             from 4 rows up, else the batched GEMV at its padded row count) with the batched verify attention (every sequence on its
 *             own table, RoPE / append / causal mask per row) in place of the decode attention; the last id of a sequence is never
 *             fed.  Unused row slots are fed id 0: the attention writes nothing for them and nothing reads them afterwards.
 *   head      the prompt's last row (target F_g[0], once per sequence) and every fed row (target the next id) are normed into rows of their
 *             own by indexed final norms and go through the EPI_TARGET lm_head in chunks of <= 32 rows + its final kernel, as the forced
 *             jobs of the scheduler do; under an allowed list the subset product.  With svln_set_sampling on inv_t = 1 / T, no noise is
 *             evaluated and no draw is consumed.
 * Afterwards a group is PENDING on the env (svln_group_select and everything a pending group blocks, as after svln_generate_group): its
 * sequence g has fed n_g - 1 ids, so svln_group_select makes the env go on where a forced turn on F_g would have left it
 * (kv_len = L + n_g - 1).  svln_group_logprobs returns sequence g's scores, svln_group_dist its rows over the allowed list,
 * svln_get_hidden_group its first <= 8 tap rows.  An armed draft is consumed, as by a forced turn; the draft switches may be on.
 * Refused before any launch or state change: everything svln_generate_forced refuses, for every sequence; svln_set_mxfp4_batched on (a
 * scoring pass runs the batched step and would change its numeric scheme); svln_top_logprobs k > 0; n_seq outside 2 .. 8; a length outside
 * 1 .. 32; L + max_g n_g - 1 > max_positions; a free pool that cannot hold the env's own missing pages and the forks' tails. */
int svln_generate_candidates(svln_engine* h, int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos_ids, int n_eos,
                             float* logprobs, int64_t* greedy_ids, float* greedy_logprobs);
/* svln_turn's bookkeeping (encode, window / episode resets, splice), then the candidates call, in one crossing (a->max_new_tokens is not read) */
int svln_turn_candidates(svln_engine* h, const svln_turn_args* a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs,
                         int64_t* greedy_ids, float* greedy_logprobs);
/* Opt-in: svln_generate_candidates with the rows of scoring pass 0 FOLDED into the prefill pass.  Arguments, results, refusals, the
 * pending group and what svln_group_select leaves are svln_generate_candidates'; what changes is where the rows are computed.
 *   rows      one pass of M = Tn + n_seq r rows: rows [0, Tn) are the prompt's new rows; row Tn + g r + j is the token embedding of
 *             F_g[j], j < min(r, n_g - 1), at position L + j of sequence g (pad slots are fed id 0, as in a scoring pass).  Every dense
 *             product of every layer runs once on the M rows; the q|k|v product does not rope or append (its fused reduce is not used).
 *   prompt    rows [0, Tn): the separate RoPE + append launch, then the prefill's causal attention.
 *   branches  rows [Tn, M): the batched verify attention of a scoring pass -- sequence g on its own table from position L, RoPE, append
 *             and causal mask per row.  Candidates longer than r + 1 ids go on with svln_generate_candidates' passes from pass 1.
 *   mirror    the tables of the fork are built BEFORE the pass.  When L % 64 != 0 the forks' first private pages must hold the prompt's
 *             rows of page q0 = L / 64 in every layer while the pass is still running: the RoPE + append launch stores each k / v row of
 *             logical page q0 to the env's page and, same values and offsets, to every fork's first page (at most 7).  Rows of EARLIER
 *             turns in page q0 (kv_len > 64 q0) are copied by one page-copy launch before the pass; the fork launch after the prefill
 *             is gone.  When L % 64 == 0 nothing is mirrored or copied.
 *   head      ONE indexed final norm for the prompt's last row (once per sequence) and the folded rows; then as svln_generate_candidates.
 * Candidates of one id each feed nothing: the call is svln_generate_candidates, launch for launch (and bit for bit).
 * Otherwise NO result is bit-equal to svln_generate_candidates' by contract: the row count of a product selects its plan (tile,
 * split-K), so the prompt's rows and the candidates' rows may both differ in rounding from the unfolded call's -- the caveat stated for
 * svln_set_prefill_draft.  Both calls lie inside the same bounds of the exact result.
 * Results of one candidate still do not depend on the other candidates' ids.
 * Refused besides, by name and before any launch or change: a row workspace (max_positions rows) that cannot hold Tn + n_seq r rows. */
int svln_generate_candidates_folded(svln_engine* h, int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos_ids,
                                    int n_eos, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs);
/* svln_turn_candidates with the folded call */
int svln_turn_candidates_folded(svln_engine* h, const svln_turn_args* a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs,
                                int64_t* greedy_ids, float* greedy_logprobs);
/* Opt-in, no reference counterpart: forced turns as jobs of the multi-env scheduler.  svln_batch_submit_forced queues a forced turn on the
 * ids F[0 .. n) for an env whose turn has been appended, as svln_batch_submit queues a plain one.  The job is a prefill segment of
 * Tn + n - 1 rows: the iteration that prefills it gathers F[0 .. n - 1) on the device as the rows at positions n_embeds .. n_embeds + n - 2
 * (the ragged gather list of svln_set_batch_draft; the last id is never fed) and sends its last n rows through the EPI_TARGET head; the
 * job FINISHES in that iteration, with no decode iteration.  The segment is all or nothing: when it does not fit the row workspace beside
 * the rows already packed (M + Tn + n - 1 > max_positions) the job waits for the next iteration, as a plain job does; it is never cut
 * the way a draft is.
 * Head: the plain head rows of the iteration (decode rows, last prompt rows, ride rows) are produced by the code, in the order and in the
 * buffers of an iteration without forced jobs.  The forced head rows are listed after them in slot order, a job's n rows consecutive:
 * ONE indexed final norm writes them to rows of their own and to the parity taps (head row i of a job -> tap row min(i, 7) of its slot; tap row 7 keeps the LAST of the rows that share it),
 * then the list is taken in chunks of <= 32 rows from its start (a job may straddle a chunk); a chunk of r rows has the routing of
 * svln_generate_forced for n = r (r <= 2: the batched GEMV at B = 2; r >= 3: the 32-row MFMA tiles, 3 padded to 4; pad rows carry target
 * -1); under an allowed list it is the subset product in its EPI_TARGET form.  The lists hold 8 x 32 rows, so no job waits for head
 * space.  With svln_set_sampling on inv_t = 1 / T, no noise is evaluated and no draw counter moves.  An iteration that holds no forced job
 * runs the launches it ran before these entries existed.
 * On a finished forced slot: svln_batch_result returns out_ids = F (and frees the slot); svln_batch_scores the n forced log-probabilities
 * whatever svln_set_token_scores says; svln_batch_allowed_logprobs the n rows when an allowed list is set (scores switch on or off);
 * svln_get_hidden_batch min(n, 8) tap rows; svln_batch_topk is refused by name (a forced turn produces no lists); svln_batch_forced
 * returns logprobs / greedy_ids / greedy_logprobs as svln_generate_forced defines them (valid until svln_batch_result frees the slot;
 * refused by name on a slot that holds a plain turn).  Afterwards the env's kv_len = n_embeds + n - 1.
 * Refused before any state change (the job table, the env, the armed draft): everything svln_batch_submit refuses; n outside 1 .. 32; an
 * id outside the vocabulary; an id of the EOS set anywhere but last; a repetition penalty != 1; an id outside the allowed list;
 * n_embeds + n - 1 > max_positions; svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm, svln_set_decode_persistent or
 * svln_set_mxfp4_batched on (the decode rows a forced row stands in for would run MXFP4 products there while the prefill runs bf16: the
 * reason svln_set_batch_draft gives).  An armed draft is treated as svln_batch_submit treats it: consumed iff svln_set_batch_draft is
 * on; a forced job never reads it.  Forced jobs may share an iteration with rides.  svln_generate_forced / svln_turn_forced keep their
 * idle-scheduler refusal and svln_generate_batch stays greedy or sampled only.
 * slot == NULL is a dry run: the refusals that need no state of the env's rows (all of the above but "nothing to prefill" and the
 * max_positions line) are checked and nothing is queued, so that a caller can refuse a turn before it encodes a frame or splices a row.
 * svln_batch_forced_stats: forced jobs finished, rows they fed (n - 1 each), head chunks launched; any pointer may be null. */
/* (the two declarations below carry their return type on a line of its own: tests/test_forced_host.py pins the set of one-line
 * `int svln_*forced(` declarations of this header to the single-env entries above) */
int
svln_batch_submit_forced(svln_engine* h, int env, const int64_t* ids, int n, const int64_t* eos_ids, int n_eos, int32_t* slot);
int
svln_batch_forced(svln_engine* h, int slot, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs, int cap, int32_t* n);
int svln_batch_forced_stats(svln_engine* h, int64_t* jobs, int64_t* rows_fed, int64_t* head_launches, int reset);
/* prefill taps of svln_generate (single env): enable != 0 records the LAST row of the residual stream after every decoder layer of the
 * next prefills (svln_get_layer_taps: host_out [layers][hidden]); probe_layer >= 0 additionally records, for every row of the prefill,
 * the operands the products of that one layer actually saw (svln_get_layer_probe, which: 0 = x entering the layer, 1 = x leaving it,
 * 2 = attention output [q_heads * 128], 3 = x after the attention residual, 4 = post_attention_layernorm(x), 5 = silu(gate) * up
 * [inter], 6 = input_layernorm(x), 7 = the q | k | v buffer after bias and RoPE [(q_heads + 2 kv_heads) * 128]: the q columns are rotated; the rotated k goes to the
 * KV pages only, so the k and v columns hold the plain product (and nothing where the product's reduce did the append); the others [hidden]),
 * so that each fused stage can be checked against the oracle on the engine's own inputs, at its own scale.  enable = 0 switches
 * both off. */
int svln_set_layer_taps(svln_engine* h, int enable, int probe_layer);
int svln_get_layer_taps(svln_engine* h, float* host_out);
int svln_get_layer_probe(svln_engine* h, int which, float* host_out, int64_t max_elems, int32_t* n_rows, int32_t* n_cols);

/* -- decode execution mode + timing probes (bench.py) */
int svln_set_decode_graph(svln_engine* h, int enable);     /* replay the per-token decode step as a hipGraph */
/* Execution form of the single-env decode step (same arithmetic per output, different summation order over K): enable != 0 runs, per
 * layer, the decode attention launch followed by ONE persistent launch (one workgroup per CU: LDS-DMA weight ring + consumer waves,
 * granule all-gathers between the products) for the merge of the attention partials, o_proj, gate/up + SwiGLU, down_proj and the next
 * layer's q|k|v, instead of six launches.  Needs the whole GPU (every workgroup must be resident); a hand-off that times out makes
 * svln_generate / svln_turn fail.  Refused for shapes it does not cover.  With svln_set_fp8_decode on, the launched GEMVs are kept. */
int svln_set_decode_persistent(svln_engine* h, int enable);
/* diagnostic (tools/persist_probe.py): one persistent launch of `layer` with per-workgroup phase stamps, out [n_wgs][16] ticks of the
 * 100 MHz wall clock: [0] merge done, [1] edge 0 gathered, [2] o_proj done, [3] edge 1 gathered, [4] gate/up done, [5] edge 2 gathered,
 * [6] down_proj done, [7] edge 3 gathered, [8] q|k|v done (consumer wave 0); [10..14] the loader at the start / after each product's
 * stream.  Runs on whatever the engine's buffers hold (after a decode step); overwrites the residual row and the q|k|v buffer. */
int svln_probe_decode_layer(svln_engine* h, int layer, unsigned long long* out, int max_wgs, int32_t* n_wgs);
/* Test hook: ONE launch of the persistent decode layer kernel with `cus` workgroups on the caller's device buffers, then a
 * synchronisation.  Nothing of the engine's own persistent-layer state is used: granules, launch counter and give-up word are the
 * caller's.  T = the engine dtype; qd = n_q * 128.  Refused by error, WITHOUT a launch, when the shape is outside what
 * svln_decode_layer_supported admits or when cus exceeds the device's CU count (every workgroup must be resident at once).
 * Buffer layouts (all device memory):
 *   o_w [H][qd], gu_w [2 I][H] in the EPI_SWIGLU packing (64-row blocks = [gate 32 | up 32]), down_w [H][I], next_qkv_w [qkv_dim][H],
 *   all T, rows dense; post_norm [H], next_norm [H], next_qkv_b [qkv_dim] T.  next_norm / next_qkv_w null = last layer (qkv_out and
 *   gran[3] are then not touched); next_qkv_b may be null.
 *   part    float [nsplit][n_kv][32][132]: per split and q head (kv head kh, q head rho of it at row kh * 32 + rho) 128 un-normalised
 *           outputs, then m (log2 domain) at [128] and l at [129]; splits at or past ceil(ceil(*kv_len / 64) / tiles_per_split) are
 *           not read
 *   kv_len  int32 [1];  skip: optional int32 [1], the launch is a no-op when it is non-zero
 *   x       T [H]: residual row in, layer output out;  qkv_out T [qkv_dim]
 *   gran[e] uint64 [n_e / VPG], n = {qd, H, I, H}, VPG = 2 (bf16) or 1 (fp32) values per granule: bits 63..32 the tag
 *           *seq * 4 + e + 1 of the launch that wrote it, bits 31..0 the payload (bf16: value 2g in bits 15..0, value 2g + 1 in bits
 *           31..16; fp32: the value's bits); a granule whose tag is not this launch's is never consumed
 *   seq     uint32 [1]: launch counter, read at the start, + 1 at the end;  giveup uint32 [1]: 0, or the code of a spin that timed out */
typedef struct svln_decode_layer_op {
    const void *o_w, *post_norm, *gu_w, *down_w, *next_norm, *next_qkv_w, *next_qkv_b;
    const float* part; const int32_t* kv_len; const int32_t* skip;
    void *x, *qkv_out;
    uint64_t* gran[4]; uint32_t* seq; uint32_t* giveup;
    int32_t nsplit, tiles_per_split, n_q, n_kv, H, I, qkv_dim, cus;
    float eps;
} svln_decode_layer_op;
int svln_op_decode_layer(svln_engine* h, const svln_decode_layer_op* op);
/* host only, no engine: *supported = whether the persistent layer kernel covers (H, I, qd, qkv_dim) with `cus` workgroups */
int svln_decode_layer_supported(int dtype, int H, int I, int qd, int qkv_dim, int cus, int32_t* supported);
/* host only, no engine: how the persistent layer kernel deals one product's weight blocks (1 KiB each) to its 8 waves.  `op`: this
 * workgroup's share, nrows stream rows of K elements of elem_size bytes from output index `first` (pair: rows are gate j, up j of the
 * EPI_SWIGLU packing); `next`: the product whose first 16 slots refill the last group (the same op after the last product).  For one
 * wave and lane: slots[k], k < *n_slots: load_off = the byte offset (from the start of the weight matrix) of the load that filled
 * the register slot k consumes; valid / row / pb = whether slot k is computed and which (stream row, block of the row) it is;
 * row_done = the wave's partial sum of that row is complete after it.  refill[16]: the offsets in `next` loaded by the last group. */
typedef struct svln_decode_layer_walk_op { int32_t elem_size, K, nrows, pair, first; } svln_decode_layer_walk_op;
typedef struct svln_decode_layer_slot { int64_t load_off; int32_t valid, row, pb, row_done; } svln_decode_layer_slot;
int svln_decode_layer_walk(const svln_decode_layer_walk_op* op, const svln_decode_layer_walk_op* next, int wave, int lane,
                           svln_decode_layer_slot* slots, int max_slots, int32_t* n_slots, int64_t* refill);
/* Opt-in, no reference counterpart: the single-env decode step and the lm_head stream OCP e4m3 copies of the LLM
 * weights (one fp32 scale per output row; allocated and quantised on the device at the first enable, quantised again whenever
 * svln_set_tensor / svln_synth_tensor writes one of the matrices) instead of the bf16 ones -- half the HBM bytes per generated token.  bf16 engines only; prefill, vision and svln_generate_batch keep bf16 weights (the
 * batched paths have svln_set_fp8_gemm and svln_set_mxfp4_batched).  Refused while svln_set_mxfp4_batched is on.  A call that would
 * change the mode fails while scheduler turns are in flight ("svln_set_fp8_decode cannot change while scheduler turns are in flight";
 * the same holds for svln_set_mxfp4_decode, svln_set_fp8_gemm and svln_set_decode_persistent: no env changes scheme inside a turn); a
 * call that changes nothing always succeeds. */
int svln_set_fp8_decode(svln_engine* h, int enable);
/* Opt-in, no reference counterpart: the single-env decode step's four projections and every lm_head product (the
 * prefill's token included) stream OCP MXFP4 copies of the LLM weights instead of the bf16 ones -- E2M1 elements, one E8M0 power-of-two
 * scale per 32 consecutive elements of a row, 4.25 bits per weight; allocated and quantised on the device at the first enable, quantised
 * again whenever svln_set_tensor / svln_synth_tensor writes one of the matrices (~4.0 GB beside the bf16 copy at the 7B size).  Numeric scheme: svln_op_quant_mxfp4.  bf16 engines only; hidden, intermediate and
 * q_heads * 128 must be multiples of 32.  Prefill, vision, attention and norms keep bf16 weights; svln_generate_batch and the scheduler
 * keep them too unless svln_set_mxfp4_batched (below) is on.  Mutually exclusive with svln_set_fp8_decode: enabling one while the other
 * is on fails.  Captured decode graphs are dropped when the
 * mode changes; while it is on the launched GEMVs are kept (svln_set_decode_persistent has no effect). */
int svln_set_mxfp4_decode(svln_engine* h, int enable);
/* Lossless, no reference counterpart, ON by default on bf16 engines: the single-env decode step's gate/up and down_proj GEMVs and the
 * lm_head GEMV (the prefill's token included) stream a 12-bit packing of their bf16 weights instead of the bf16 bytes -- per row a table
 * of the eight most frequent values of the high byte (without the sign), per weight the low byte and a 4-bit code (sign, table index); a
 * 512-element block that holds a value outside the table is read from the bf16 original.  The decoded weight is the original bit
 * pattern and the summation order is the bf16 kernel's, so ids, hidden rows and scores are bit-identical with the switch on or off;
 * about 0.75 x the bytes of those products (svln_packed_stats).  Format: svln_op_pack_rows.  The packed copies are allocated at creation
 * (~9.4 GB at the 7B size) and re-encoded on the engine stream whenever svln_synth_tensor / svln_set_tensor writes one of the matrices.
 * q|k|v and o_proj (latency-bound launches), the persistent layer, svln_generate_batch / the scheduler, the verify passes, the
 * allowed-token head and every GEMM keep the bf16 weights; svln_set_fp8_decode / svln_set_mxfp4_decode read their own copies and take
 * precedence.  Composes with every other mode.  enable != 0 is refused on fp32 engines (and for hidden / intermediate sizes above 32768);
 * a change drops the captured decode graphs. */
int svln_set_packed_decode(svln_engine* h, int enable);
/* totals over the packed matrices as they are encoded now: bytes of the packed form (blocks + 16-byte row records), bytes of the bf16
 * originals, 512-element blocks, and the blocks among them that fall back to the bf16 original.  All 0 on an fp32 engine. */
int svln_packed_stats(svln_engine* h, int64_t* packed_bytes, int64_t* bf16_bytes, int64_t* blocks, int64_t* fallback_blocks);
/* Opt-in, no reference counterpart: the same MXFP4 weight copies for the envs that svln_generate_batch / svln_batch_step carry.  While it
 * is on, the batched decode step runs q|k|v, o_proj, gate/up and down_proj at every batch size (1, 2, 4, 8) on a weight-only MFMA kernel
 * (bf16 activations x exactly dequantised weights, fp32 accumulate: svln_op_gemv_mxfp4_batched), and every lm_head product of the
 * scheduler -- the token that follows a prefill included -- reads the MXFP4 lm_head.  Prefill rows keep the bf16 products; a scheduler
 * iteration that holds decode rows and prefill rows runs the decode rows as a batched decode step of their own, then the prefill
 * segments as a bf16 pass, so every env is computed by the scheme of svln_set_mxfp4_decode (prefill bf16, decode projections and
 * lm_head MXFP4) whatever its neighbours do.  bf16 engines only.  Independent of svln_set_mxfp4_decode (either or both may be on);
 * mutually exclusive with svln_set_fp8_decode and svln_set_fp8_gemm: enabling it while one of them is on fails, and they fail while it
 * is on.  A call that would change the mode (on -> off as well as off -> on) fails while scheduler turns are in flight; a call that changes
 * nothing always succeeds.  Captured batched decode graphs are dropped when it changes. */
int svln_set_mxfp4_batched(svln_engine* h, int enable);
/* Opt-in, no reference counterpart (BASELINE configs[4] "fp8 MFMA on QKV/MLP GEMMs"): the LLM's dense products with more
 * than one row -- prefill, and the decode steps of >= 4 envs batched by svln_generate_batch / svln_batch_step -- run as e4m3 x e4m3 MFMA
 * products (fp32 accumulate, bf16 out) on the e4m3 weight copies above with per-row activation scales computed on the fly.  bf16 engines
 * only; vision, attention, norms, lm_head and the batch-1 decode GEMVs are unaffected (the latter have svln_set_fp8_decode).  Refused
 * while svln_set_mxfp4_batched is on. */
int svln_set_fp8_gemm(svln_engine* h, int enable);
/* Opt-in, default off: the instruction form of the svln_set_fp8_gemm products.  Off: v_mfma_f32_32x32x16_fp8_fp8 (the bf16 MFMA rate).  On:
 * the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (v_mfma_scale_f32_16x16x128_f8f6f4 on the 8-phase 256x256 schedule, which e4m3 products
 * may take only in this form) with e4m3 operands and neutral block scales (E8M0 127): twice the bf16 work per clock on the SAME e4m3
 * bytes and per-row fp32 scales -- no numeric scheme changes, the products are the same sums in fp32.  No effect while svln_set_fp8_gemm is
 * off.  bf16 engines only.  A call that would change the form fails while scheduler turns are in flight; a call that changes nothing
 * always succeeds.  Captured batched decode graphs are keyed by the form. */
int svln_set_fp8_scaled_mfma(svln_engine* h, int enable);
/* Opt-in, default off, no reference counterpart: draft-verified greedy decode -- several tokens per pass over the weights, the SAME ids as
 * the plain greedy loop (exactly so on the fp32 engine; on the bf16 engine a verify row runs the batched step's products, whose summation
 * order differs from the batch-1 GEMVs, so a near-tie arg-max can fall the other way, as between svln_generate and
 * svln_generate_batch).  rows = 0 switches it off (today's behaviour, launch for launch); rows in {2, 4, 8} = rows per verify pass.  With
 * c >= 1 tokens of a turn emitted and an armed draft D (svln_set_draft), a verify pass feeds the last emitted token at position
 * L + c - 1 (row 0) and D[c + i - 1] at L + c - 1 + i (rows i >= 1) as the rows of one pass -- the batched decode step's products at
 * B = rows, with an attention that ropes, appends and masks every row at its own position -- and takes the arg-max o_i of every row.
 * o_0 is always emitted; o_i iff every earlier row was emitted without stopping and o_{i-1} == D[c + i - 1].  Stops are those of the
 * plain loop (an EOS id, appended and not fed; max_new_tokens; a non-finite arg-max).  Fewer rows are used when the draft runs out, when
 * max_new_tokens leaves room for fewer or when a row would reach max_positions; K / V rows of rejected positions lie at or beyond the
 * env's kv length and are overwritten later.  Host policy: after the prefill one pass is enqueued if a guessed row exists; a further pass
 * follows while every emitted id from index 1 on equals the draft and guessed rows remain; otherwise ordinary decode steps finish the turn.
 * Refused: rows outside {0, 2, 4, 8}; rows * (q_heads / kv_heads) > 32 (the verify attention keeps the decode kernel's 32 query rows
 * per kv head: Qwen2-7B, G = 7, takes rows <= 4); while svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm,
 * svln_set_mxfp4_batched or svln_set_decode_persistent is on (a verify pass must compute each row in the numeric scheme of the single
 * step it replaces), and each of those is refused while this mode is on; while scheduler turns are in flight.  A call that changes nothing
 * always succeeds.  Captured decode graphs are dropped when it changes. */
int svln_set_speculative(svln_engine* h, int rows);
/* Arms a draft for env's next svln_generate / svln_turn / svln_generate_fixed: the caller's guess of the WHOLE id sequence of that turn,
 * index 0 included (never needed: the prefill emits it), so the previous turn's output can be passed verbatim.  Consumed by that call
 * whether or not it helped; n = 0 clears it; svln_reset_env / svln_kv_reset leave it armed.  Host-only: no GPU work, no synchronisation.
 * Refused: an unknown env, n < 0, n > max_positions.  An id outside [0, vocab) ends the usable draft at its index.  Ignored (not an error)
 * while the mode is off or a repetition penalty != 1 is set, and by svln_generate_batch / the scheduler (which leave it armed) unless
 * svln_set_batch_draft is on: then svln_batch_submit consumes it. */
int svln_set_draft(svln_engine* h, int env, const int64_t* ids, int n);
/* Counters since the last reset, over svln_generate / svln_turn / svln_generate_fixed: verify passes run, tokens they emitted, tokens
 * emitted by ordinary decode steps.  The prefill's own token counts in none of them.  Any pointer may be null. */
int svln_draft_stats(svln_engine* h, int64_t* verify_passes, int64_t* tokens_from_verify, int64_t* single_steps, int reset);
/* Opt-in, default off, no reference counterpart: drafts inside the prefill pass ("rides") -- a turn whose armed draft (svln_set_draft)
 * is right needs NO decode pass.  With L rows of inputs_embeds, Tn of them new, and a usable draft D (ids up to the first one outside
 * the vocabulary; one id is enough), the prefill of svln_generate / svln_turn / svln_generate_fixed carries
 *     k = min(len(D), 7, tokens the call may emit - 1, max_positions - L), cut further at the first D[j] in the EOS set
 * extra rows: the token embeddings of D[0 .. k) at positions L .. L + k - 1 of the same sequence (RoPE, KV append and the causal prefill
 * attention at any T; there is no rows * (q_heads / kv_heads) limit).  The lm_head arg-max o_i of the last k + 1 rows then goes through
 * the verify rule of svln_set_speculative from zero emitted tokens: o_0 (the plain turn's token 0) is always emitted, o_i iff every
 * earlier row was emitted without stopping and o_{i-1} == D[i - 1].  K / V rows of rejected positions lie at or beyond the env's kv
 * length and are overwritten later.  One synchronisation reads the result: a finished turn returns with no decode step enqueued; an
 * unfinished one whose emitted ids all equal the draft continues with verify passes when svln_set_speculative is on and guesses remain;
 * otherwise ordinary decode steps finish it (a failed ride costs k rows and one extra synchronisation).  k = 0 (no draft, a draft that
 * opens with an EOS id, max_new_tokens = 1, no position left, a repetition penalty != 1): the plain turn, launch for launch, bit-identical
 * to mode off.  Ids are those of the plain loop exactly on the fp32 engine's fixtures; the product plans depend on the row count, so with
 * k > 0 the prompt rows' sums may be ordered differently than in a plain turn and a ridden row's differently than a decode step's: on the
 * bf16 engine a near-tie arg-max can fall the other way, as between svln_generate and svln_generate_batch.  Independent of
 * svln_set_speculative (either, both or neither).  Refused like it: while svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm,
 * svln_set_mxfp4_batched or svln_set_decode_persistent is on, and each of those is refused while this mode is on; while scheduler turns
 * are in flight.  A call that changes nothing always succeeds.  svln_generate_batch and the scheduler ignore the mode (their own
 * switch is svln_set_batch_draft). */
int svln_set_prefill_draft(svln_engine* h, int on);
/* Counters since the last reset: rides run, tokens they emitted (the turn's token 0 included), draft rows they fed (the k's summed).
 * svln_draft_stats keeps its meaning: a token emitted by a ride counts in none of its three counters.  Any pointer may be null. */
int svln_prefill_draft_stats(svln_engine* h, int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int reset);
/* MULTI-DRAFT turns, no switch, no reference counterpart: svln_generate with hints -- n_drafts <= 8 guessed id sequences D_0 .. D_{G-1}
 * of THIS turn (ids = the sequences back to back, lens[g] = 0 .. 32 ids each), all verified by ONE prefill pass.  Ids, the EOS / max_new
 * stop, the cache length and every getter are svln_generate's on the same state; no guess can change a greedy output: every emitted token
 * is the arg-max of a row that was fed the true prefix.  fp32 engine: ids identical on the fixtures; bf16 engine: a near-tie arg-max may
 * fall the other way, because a product's row count selects its plan (as under svln_set_prefill_draft).
 *   plan    r = min(32 / (q_heads / kv_heads), 32 / G) row slots per draft.  Draft g feeds k_g = min(len D_g, r, tokens the call may emit
 *           - 1, max_positions - L) ids, cut at the first id outside the vocabulary and at the first id in the EOS set (an EOS id is
 *           compared, never fed).  Trailing drafts are dropped one at a time while the row workspace (Tn + G r rows within max_positions)
 *           or the free pages (the env's pages up to L + k_0, plus the fork tails of drafts 1 ..) fall short, possibly down to none.  A
 *           draft with k_g = 0 feeds nothing and takes no page.  Duplicates are not merged.
 *   pass    the row layout of svln_generate_candidates_folded: M = Tn + G r rows, row Tn + g r + j = the embedding of D_g[j], sequence 0
 *           on the env's own page table, sequence g >= 1 on a fork whose first private page mirrors the prompt's last page (L % 64 != 0).
 *   head    one indexed final norm of the prompt's last row (once) and of the fed rows, the lm_head arg-max in chunks of <= 32 rows in the
 *           form the switches ask for (token scores, an allowed list), then ONE select launch: per draft the verify rule of
 *           svln_set_speculative on [row 0, rows of g] from zero emitted tokens; the largest emitted count wins, a tie goes to the lowest g.
 *   after   one synchronisation; the winner's private pages become the env's, every other fork page and the env's displaced pages go back
 *           to the pool, no group is left pending.  A finished turn returns with no decode launch; otherwise single decode steps finish
 *           it (no verify passes behind a multi-draft pass).
 * Hints are IGNORED -- the call is then svln_generate launch for launch and bit for bit, never a refusal -- with svln_set_sampling on, a
 * repetition penalty != 1, svln_set_fp8_decode / svln_set_mxfp4_decode / svln_set_fp8_gemm / svln_set_decode_persistent on,
 * svln_top_logprobs k > 0, svln_token_entropy on, svln_set_token_scores together with svln_set_allowed_tokens, a group turn pending on
 * another env (its forks hold the one fork scaffold), or no draft with a usable first id.  Everything svln_generate refuses is refused the same way; an armed svln_set_draft draft is consumed and not used.  Argument
 * faults are refused by name before any launch: n_drafts outside 0 .. 8, a length outside 0 .. 32, a null pointer.
 * *winner_out (optional) = the winning draft, -1 when no pass ran; *pass_tokens_out (optional) = the tokens the pass emitted (0 then). */
int svln_generate_drafts(svln_engine* h, int env, int n_drafts, const int64_t* ids, const int32_t* lens, int max_new_tokens,
                         const int64_t* eos_ids, int n_eos, int64_t* out_ids, int out_cap, int32_t* n_out, int32_t* winner_out,
                         int32_t* pass_tokens_out);
/* svln_turn's bookkeeping (encode, window / episode resets, splice), then svln_generate_drafts, in one crossing */
int svln_turn_drafts(svln_engine* h, const svln_turn_args* a, int n_drafts, const int64_t* ids, const int32_t* lens, int64_t* out_ids, int out_cap,
                     int32_t* n_out, int32_t* kv_len, int32_t* winner_out, int32_t* pass_tokens_out);
/* Counters of the multi-draft calls since the engine was created, out[8]: calls, passes run, tokens the passes emitted (token 0 included),
 * draft rows fed, turns finished in the pass, calls whose hints were ignored, page handovers (winner >= 1), tokens of single steps. */
int svln_drafts_stats(svln_engine* h, int64_t* out);
/* Opt-in, default off, no reference counterpart: drafts in the prefill pass of the multi-env scheduler (svln_batch_submit /
 * svln_batch_step / svln_generate_batch) -- a lockstep turn whose drafts are all right is ONE scheduler iteration.  Independent of
 * svln_set_speculative and svln_set_prefill_draft, which the scheduler goes on ignoring.  With the switch on, svln_batch_submit consumes
 * the env's armed draft (svln_set_draft) whether or not it helps; it is usable if the repetition penalty is 1, up to its first id outside
 * the vocabulary, and the job keeps it.  When an iteration packs the prefill segments in slot order, a job with a usable draft D, Tn new
 * rows and M rows packed before it gets
 *     k = min(len(D), 7, max_new_tokens - 1, max_positions - n_embeds), cut at the first D[j] in the job's EOS set,
 *         and cut to max_positions - M - Tn, the rows the workspace still holds
 * extra rows: the token embeddings of D[0 .. k) at positions n_embeds .. n_embeds + k - 1 of that env, behind its prompt rows (a job
 * whose Tn rows do not fit waits for the next iteration, as without the switch, and keeps its draft).  Decode rows of other envs share
 * the pass as before.  The lm_head arg-max runs on one row per decode row and k + 1 rows per segment, at most 64 in all, in chunks of
 * at most 32 rows.  After the iteration's one synchronisation the host applies the verify rule of svln_set_speculative from zero
 * emitted tokens to each job: o_0 is always emitted, o_i iff every earlier one was emitted without stopping and o_{i-1} == D[i - 1];
 * stops are an EOS id (appended, never fed), the max_new_tokens-th token, a non-finite arg-max.  With e tokens emitted the env's kv
 * length is n_embeds + e - 1; K / V rows of rejected positions lie beyond it and are overwritten later.  A job that did not stop goes on
 * as an ordinary decode row; its draft is dropped after the ride (there are no batched verify passes).  svln_get_hidden_batch returns
 * the final-norm rows of the emitted tokens as before.  An iteration in which no job rides is launch for launch the one without the
 * switch, bit-identical.  With rides the row count of the pass, and so the product plans, differ from a plain iteration: fp32 ids equal
 * the plain run's on the fixtures; on the bf16 engine a near-tie arg-max can fall the other way.  Refused: while scheduler turns are in
 * flight; while svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm, svln_set_mxfp4_batched or svln_set_decode_persistent is
 * on (a ridden row must be computed in the numeric scheme of the decode row it replaces: under svln_set_fp8_gemm a batched step of
 * B <= 2 runs bf16 GEMVs while the prefill products run e4m3), and each of those is refused while this switch is on.  A call that
 * changes nothing always succeeds. */
int svln_set_batch_draft(svln_engine* h, int on);
/* Counters of the scheduler since the last reset: rides run (jobs prefilled with k >= 1), tokens they emitted (the turn's token 0
 * included), draft rows they fed (the k's summed), iterations (passes svln_batch_step executed; counted with the switch off as well),
 * decode rows fed one token at a time.  Any pointer may be null. */
int svln_batch_draft_stats(svln_engine* h, int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int64_t* iterations,
                           int64_t* single_rows, int reset);
/* Opt-in slow-memory pruning (BASELINE configs[3]; the reference has NO counterpart -- its memory is all num_history x 196 pooled
 * tokens, streamvln_eval.py:313-321 -- so this is pinned only by the project's own CPU restatement, oracle: prune_memory_tokens):
 * with keep_tokens > 0 a `<memory>` sentinel expands to the keep_tokens memory tokens least similar (cosine) to the mean memory
 * token, in their original order (ties: lower index).  0 (default) = the reference behaviour. */
int svln_set_memory_prune(svln_engine* h, int keep_tokens);
int svln_probe_reset(svln_engine* h);
int svln_probe_read(svln_engine* h, double* total_ms, int64_t* launches, double* bytes_per_launch);
/* second probe armed by svln_probe_reset: the layer-0 gate/up product of every steady prefill (<= 256 rows) between two stream events:
 * total ms, how many, their mean row count, flops of one (2 * rows * 2 * inter * hidden) and its weight bytes */
int svln_probe_read_prefill(svln_engine* h, double* total_ms, int64_t* count, double* mean_rows, double* flops, double* weight_bytes);
int svln_phase_times(svln_engine* h, double* vision_ms, double* prefill_ms, double* decode_ms, int reset);

/* -- optional memoisation of pooled frame features keyed by a 128-bit content hash of the pixels:
 * the <memory> frames of a window restart were all encoded earlier as "current" frames, so with the cache on they
 * skip the ViT.  capacity_frames = 0 (default) disables it: every frame is re-encoded, as the reference does
 * (stream_video_vln.py:104).  The entries are features of the weights loaded when they were computed: a svln_set_tensor /
 * svln_synth_tensor of a vision-tower or projector tensor drops them all. */
int svln_set_feature_cache(svln_engine* h, int capacity_frames);
int svln_feature_cache_stats(svln_engine* h, int64_t* hits, int64_t* misses);

/* -- single-kernel entry points (device pointers in the engine dtype) for the op-level parity tests */
/* force_cfg (op tests and A/B runs only; the engine always passes 0): low 12 bits = tile configuration, 0 = heuristic, 128 = 128x128,
 * 129 = 128x128 with two in-workgroup K groups, 256 = 256x256 (bf16: 8-phase schedule), 258 = 256x256 with two K slices, 264 = 256x64
 * (M <= 256), 64 = 64x64, 32 = 32x128 (M <= 32); flag bits: 0x1000 row tiles fastest in the workgroup order, 0x10000 column tiles
 * fastest, 0x4000 stage-ring kernel for the 256x256 tile, 0x8000 32x32x16 form of the 8-phase schedule, 0x20000 direct 2-byte stores in the 8-phase
 * epilogue instead of the LDS-staged 16-byte row chunks, 0x40000 (svln_op_gemm_fp8 only; what the engine passes while
 * svln_set_fp8_scaled_mfma is on) the block-scaled MFMA form of an e4m3 product, with which force_cfg 256 means the 8-phase schedule.
 * force_split: 0 = heuristic, S >= 1 = 256x128 tiles (256x64 with force_cfg 264) with S K-splits.
 * Every svln_op_gemm* call is refused (non-zero, svln_last_error) before any launch when A, W or C is null or A / W not 16-byte aligned, an
 * extent is negative, K, lda or ldw is not a multiple of the operand format's 16-byte chunk (4 fp32, 8 bf16, 16 e4m3 values), lda or
 * ldw < K, ldc below the output width, a residual has ldr < N, res_mod < 0, SwiGLU meets N % 64 != 0, or epi is not NONE, GELU_TANH,
 * GELU_ERF or SWIGLU. */
int svln_op_gemm(svln_engine* h, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* res,
                 int ldr, int res_mod, int M, int N, int K, int epi, int force_cfg, int force_split);
/* C = A . W^T + bias + res, and -- when the product takes the split-K path (few rows, N <= 4096) -- norm_out = norm(C) from the same slab
 * reduce (*fused = 1): RMSNorm with weight norm_w when norm_b is null (Qwen2 o_proj -> post_attention_layernorm, down_proj ->
 * input_layernorm, modeling_qwen2.py:269-299), LayerNorm with weight norm_w and bias norm_b otherwise (SigLIP out_proj -> layer_norm2,
 * fc2 -> next layer_norm1, siglip_encoder.py:269-305).  Otherwise norm_out is left untouched (*fused = 0) and the caller runs
 * svln_op_rmsnorm / svln_op_layernorm. */
int svln_op_gemm_norm(svln_engine* h, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* res, int ldr,
                      const void* norm_w, const void* norm_b, void* norm_out, float eps, int M, int N, int K, int force_split, int* fused);
/* the RMSNorm form with the e4m3 copy of the normalised rows (opt-in fp8 products: the reduce that emits the norm also quantises it):
 * q8 [M][N] bytes, q8_scale [M] = max |norm_out row| / 448, with the floor and the NaN rule of svln_op_quant_fp8 (same arithmetic) */
int svln_op_gemm_norm_q8(svln_engine* h, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* res, int ldr,
                         const void* norm_w, void* norm_out, float eps, int M, int N, int K, int force_split, void* q8, float* q8_scale, int* fused);
int svln_op_gemv(svln_engine* h, const void* W, int ldw, const void* x, const void* norm_w, float eps, const void* bias, const void* res,
                 void* y, int N, int K, int epi, int32_t* host_token);
/* What the GEMM dispatcher does with one product, without launching it: needs no engine and no device.  The problem holds what the
 * dispatcher reads of a call: dtype SVLN_BF16 / SVLN_F32, epi as above, the extents, 0 / 1 flags for the optional pointers (fp8 = e4m3
 * operands with scales; fp8 = 2: on the block-scaled MFMAs, reported as fp8 = 2 in each launch, has_ws / ws_elems = the split-K workspace in fp32 elements, has_zeros = the zero line, norm_out, norm_w, res), the
 * fused-tail requests with their extents (rope: q heads, kv heads, rows; vitpack: frames, rows per frame, heads, head_dim) and force_cfg /
 * force_split.  The plan holds the one or two tile launches (tile: 0 32x128, 1 64x64, 2 128x128, 3 128x128 for more than one round,
 * 4 128x128 with two K groups, 5 256x128, 6 256x64, 7 256x256 stage ring, 8 256x256 8-phase, 9 its 32x32x16 form; the kernel variant;
 * the launcher-filled GemmArgs fields; grid, block, dynamic LDS), the reducer after a K-split launch (0 none, 1 epilogue, 2 row norm,
 * 3 q|k|v RoPE + KV append, 4 ViT K / V^T pack) with its grid and block, `fused` (what svln_op_gemm_norm reports) and vit_packer.
 * Refused with a message: a null argument, an unknown dtype or epilogue, an extent outside int32. */
typedef struct svln_gemm_problem {
    int64_t dtype, epi, M, N, K, fp8, has_ws;
    uint64_t ws_elems;
    int64_t has_zeros, norm_out, norm_w, res, rope, rope_nq, rope_nkv, rope_T, vitpack, vit_F, vit_S, vit_heads, vit_head_dim, force_cfg, force_split;
} svln_gemm_problem;
typedef struct svln_gemm_launch {
    int32_t tile, splitk, fp8, ntw, vp, tile_base, launch_tiles, nsplit, grid, block, lds_bytes, bm, bn;
    int32_t reducer, reducer_grid[3], reducer_block, reduce_too_large;
} svln_gemm_launch;
typedef struct svln_gemm_plan_out {
    int32_t nt_w, bn_fast, n_launches, fused, vit_packer;
    svln_gemm_launch launch[2];
} svln_gemm_plan_out;
int svln_gemm_plan(const svln_gemm_problem* problem, svln_gemm_plan_out* plan);
/* Which modes may be on together, and which turn forms run under them, without an engine and without a device: the ONE rule table every
 * setter, the weight write and every turn form read (csrc/modes.h), which is the reference for every refusal the comments of this file
 * mention.  A state is one 0 / 1 field per mode the rules read (topk: k > 0, truncation: top_k > 0, penalty: a factor != 1), jobs =
 * scheduler turns in flight, group = a group turn is pending, on env group_env.  A caller is a number of the Caller enumeration of
 * modes.h: a setter in one direction (where the directions differ), the weight write, a turn form; svln_mode_rule names it.
 * svln_mode_refusal: *refused = 0 and an empty message, or 1 and the message the engine raises -- that of the caller's first violated
 * rule, beginning with `who` (null: the caller's own name; svln_synth_tensor and the candidates forms pass theirs).  no_change != 0: the
 * call would change nothing (on while on, off while off), where some setters return before some of their rules.
 * svln_mode_rule: rule `index` of svln_mode_rule_count's n_rules, in table order: the caller and its name, the part (a caller whose
 * rules are interrupted by an argument check asks part by part), the field index of the bit, whether the bit must be ON (else off),
 * whether the rule holds for a no-change call, and the message as what + tail (static strings).
 * Refused with a message: a null argument, an unknown caller, a message longer than cap - 1, an index outside the table. */
typedef struct svln_mode_state {
    int32_t decode_graph, persistent, fp8_decode, mxfp4_decode, mxfp4_batched, fp8_gemm, fp8_scaled, packed;
    int32_t speculative, prefill_draft, batch_draft;
    int32_t scores, topk, entropy, sampling, truncation, allowed;
    int32_t penalty, jobs, group, group_env;
} svln_mode_state;
typedef struct svln_mode_rule_out {
    int32_t caller, part, bit, must_be_on, on_no_change;
    const char* caller_name;
    const char* what;
    const char* tail;
} svln_mode_rule_out;
int svln_mode_refusal(int caller, const char* who, const svln_mode_state* state, int no_change, char* message, int cap, int32_t* refused);
int svln_mode_rule_count(int32_t* n_rules, int32_t* n_callers, int32_t* n_bits);
int svln_mode_rule(int index, svln_mode_rule_out* out);
/* the product behind svln_set_fp8_gemm: C [M][N] (bf16) = epi(a_scale[m] * w_scale[n] * (A8 [M][K] . W8 [N][K]^T) + bias) + res, e4m3 operands
 * (svln_op_quant_fp8 makes them), epi = EPI_NONE or EPI_SWIGLU, K % 16 == 0 */
int svln_op_gemm_fp8(svln_engine* h, const void* A8, const float* a_scale, int lda, const void* W8, const float* w_scale, int ldw, void* C, int ldc,
                     const void* bias, const void* res, int ldr, int M, int N, int K, int epi, int force_cfg, int force_split);
/* B (1, 2, 4 or 8) activation vectors x [B][ldx] against one weight stream (the decode step of svln_generate_batch / svln_batch_step at
 * B <= 2, and its lm_head at every B): y [B][ldy], res [B][ldr]; EPI_ARGMAX writes one token per vector to host_tokens[B] */
int svln_op_gemv_batched(svln_engine* h, const void* W, int ldw, const void* x, int ldx, const void* norm_w, float eps, const void* bias,
                         const void* res, int ldr, void* y, int ldy, int N, int K, int epi, int B, int32_t* host_tokens);
/* the selection step of svln_set_memory_prune on mem [n_rows][hidden] (engine dtype, device): out_idx[keep] ascending row indices
 * (host), out_score [n_rows] cosine scores (host, optional) */
int svln_op_memory_prune(svln_engine* h, const void* mem, int n_rows, int keep, int32_t* out_idx, float* out_score);
/* fp8 weight-only pieces of svln_set_fp8_decode: per-row e4m3 quantisation of a bf16 matrix [rows][cols] (cols % 16 == 0,
 * scale[r] = max|W[r]| / 448, round to nearest even), and the GEMV over such a matrix (same epilogues as svln_op_gemv).
 * Scale floor: scale[r] = max(max|W[r]| / 448, 2^-126), 1 for an all-zero row, so 1 / scale is finite and normal and a zero element is
 * byte 0 in every row; rows with max|W[r]| >= 448 * 2^-126 are not touched by the floor.  Non-finite elements: the maximum ignores a NaN,
 * and the NaN element becomes a NaN byte (0x7F / 0xFF) while the row's scale and other bytes stay what they are without it; an infinite
 * element makes the scale infinite, the row's finite elements 0 and the infinite one NaN.  A finite row never yields a NaN byte.
 * Refused with a message before any launch: a null pointer, rows < 0, cols <= 0, cols % 16 != 0; rows == 0 does nothing. */
int svln_op_quant_fp8(svln_engine* h, const void* w_bf16, int64_t rows, int cols, void* w8, float* scale);
int svln_op_gemv_fp8(svln_engine* h, const void* w8, const float* scale, int ldw, const void* x, const void* norm_w, float eps, const void* bias,
                     const void* res, void* y, int N, int K, int epi, int32_t* host_token);
/* MXFP4 weight-only pieces of svln_set_mxfp4_decode (no reference counterpart).  svln_op_quant_mxfp4: the OCP MX conversion of a bf16
 * matrix [rows][cols] (device, cols % 32 == 0).  Every run of 32 consecutive elements of a row is one block: e = floor(log2(max |w|)) - 2
 * clamped to [-127, 127] (0 for an all-zero block), e8 = e + 127 (E8M0, scale 2^e); element code = E2M1 of w / 2^e on the grid
 * {0, 0.5, 1, 1.5, 2, 3, 4, 6}, round to nearest even (5 -> 4, 3.5 -> 4, 2.5 -> 2, 1.75 -> 2, 1.25 -> 1, 0.75 -> 1, 0.25 -> 0),
 * saturating at 6, sign in bit 3; element 2j in the low nibble and 2j + 1 in the high nibble of byte j.  A block that holds a NaN or an
 * infinity gets e8 = 0xFF (E8M0 NaN) and unspecified codes; the row's other blocks are what they are without it.  (How the GEMVs read a
 * scale byte 0xFF is not specified here.)
 * q4 [rows][cols / 2] and e8 [rows][cols / 32] bytes, row-major (device): one 16-byte run of q4 is one block.
 * svln_op_gemv_mxfp4: the GEMV over such a matrix, y = epi(Wq . x' + bias) + res with the epilogues of svln_op_gemv; ldw (the row
 * stride) and K in elements, both multiples of 32.  fp32 engines refuse both. */
int svln_op_quant_mxfp4(svln_engine* h, const void* w_bf16, int64_t rows, int cols, void* q4, void* e8);
int svln_op_gemv_mxfp4(svln_engine* h, const void* q4, const void* e8, int ldw, const void* x, const void* norm_w, float eps, const void* bias,
                       const void* res, void* y, int N, int K, int epi, int32_t* host_token);
/* TEST-ONLY pieces of svln_set_packed_decode (bf16 engines; device pointers).  For bf16 bits b: lo = b & 0xFF, hi7 = (b >> 8) & 0x7F,
 * s = b >> 15.  svln_op_pack_rows encodes w_bf16 [rows][cols] (row stride ldw; cols % 8 == 0, cols <= 32768) into
 *   records [rows][16]: T[0..7] = the row's eight most frequent hi7 values, most frequent first, ties to the lower value, the last entry
 *       repeated when the row has fewer; then a little-endian 64-bit mask, bit k = block k falls back;
 *   packed [rows][ceil(cols / 512) * 768]: per block of 512 elements (64 chunks of 8; a ragged last block is zero padded) 512 low bytes
 *       (chunk l's eight at offset 8 l) and 256 bytes of 4-bit codes c = s << 3 | j, T[j] == hi7, lowest such j (chunk l's dword at
 *       512 + 4 l: byte k holds element k's code in the low nibble and element k + 4's in the high nibble).  A block with a hi7 outside T
 *       has its mask bit set and its packed bytes zero.
 * *fallback_blocks (host, optional) = the number of such blocks.  svln_op_unpack_rows writes the bf16 rows the packed form stands for to
 * out [rows][cols]: s << 15 | T[j] << 8 | lo, and the bf16 original's bytes for a fallback block.  svln_op_gemv_packed is svln_op_gemv
 * over such a matrix (W / ldw: the bf16 original); every output is bit-equal to svln_op_gemv on W.  The scored / sampled heads take it as
 * fmt 3 of svln_op_gemv_argmax_scores / _sample: W = the bf16 original, aux = the N packed rows followed by the N records.
 * Refused before any launch: an fp32 engine, a null plane, cols / K not a multiple of 8 or above 32768, ldw < K. */
int svln_op_pack_rows(svln_engine* h, const void* w_bf16, int ldw, int64_t rows, int cols, void* packed, void* records, int64_t* fallback_blocks);
int svln_op_unpack_rows(svln_engine* h, const void* packed, const void* records, const void* w_bf16, int ldw, int64_t rows, int cols, void* out);
int svln_op_gemv_packed(svln_engine* h, const void* packed, const void* records, const void* W, int ldw, const void* x, const void* norm_w, float eps,
                        const void* bias, const void* res, void* y, int N, int K, int epi, int32_t* host_token);
/* the product behind svln_set_mxfp4_batched: B (1 .. 8) bf16 activation vectors x [B][ldx] against one MXFP4 weight stream (q4 / e8 / ldw
 * as svln_op_gemv_mxfp4: the layout is shared), Y[b][n] = epi(Wq[n] . x[b] + bias[n]) + res[b][n] with y [B][ldy], res [B][ldr]; epi =
 * EPI_NONE, EPI_SWIGLU (y has N / 2 columns) or EPI_ARGMAX (no y: one token per vector to host_tokens[B], lowest index on ties, -1 for a
 * row without a finite logit).  No fused RMSNorm.  Precondition (not checked): q4 and x are 16-byte aligned base pointers (the
 * kernel loads 16-byte runs of both; with ldw % 32 == 0 and ldx % 8 == 0 every row then is).  Refused before any launch: an fp32 engine, null operands, B outside 1 .. 8, N < 1, K or
 * ldw not a positive multiple of 32, ldw < K, ldx < K or not a multiple of 8, SwiGLU with N % 64 != 0. */
int svln_op_gemv_mxfp4_batched(svln_engine* h, const void* q4, const void* e8, int ldw, const void* x, int ldx, const void* bias, const void* res,
                               int ldr, void* y, int ldy, int N, int K, int epi, int B, int32_t* host_tokens);
/* TEST-ONLY entry, not part of the product surface: the EPI_ARGMAX form above with the repetition penalty of svln_set_repetition_penalty
 * as the scheduler applies it (the flags are otherwise the engine's own, so no caller needs this): pen_flags [rows][N] bytes and
 * pen_rows [B] (device) -- vector b uses flag row pen_rows[b]; a flagged
 * logit becomes v < 0 ? v * penalty : v / penalty before the arg-max.  Same refusals; penalty must be > 0. */
int svln_op_gemv_mxfp4_batched_argmax_pen(svln_engine* h, const void* q4, const void* e8, int ldw, const void* x, int ldx, int N, int K, int B,
                                          const void* pen_flags, const int32_t* pen_rows, float penalty, int32_t* host_tokens);
/* TEST-ONLY entries, not part of the product surface: one lm_head product of svln_set_token_scores with optional repetition-penalty
 * flags (device pointers; null = none), tokens and log-probabilities to the host.  host_logprob(s) null: the plain EPI_ARGMAX kernels
 * on the same inputs (the tokens of the two forms are bit-equal).
 * svln_op_gemv_argmax_scores: the single-env head; fmt 0 = W in the engine dtype, 1 = e4m3 bytes with aux = fp32 row scales, 2 = MXFP4
 * codes with aux = E8M0 scale bytes (layouts of svln_op_gemv_fp8 / svln_op_gemv_mxfp4); pen_flags [N] bytes.
 * svln_op_gemv_batched_argmax_scores: the batched GEMV itself at B = 1, 2, 4, 8 (no routing to the MFMA form), optional fused RMSNorm;
 * the arg-max ignores the norm's positive row factor (as the plain form does), the log-probability is that of the normalised logits;
 * pen_flags [rows][N], pen_rows [B]: vector b uses flag row pen_rows[b].
 * svln_op_gemm_argmax_scores: the 32 x 128 MFMA tiles, 1 <= M <= 32 rows of A [M][lda]; pen_rows [M].
 * Refused before any launch: null operands, extents below 1, K / the leading dimensions not positive multiples of the format's 16-byte
 * chunk or below K, B outside {1, 2, 4, 8}, M outside 1 .. 32, N above 262144 (MFMA form), flags without their row table, penalty <= 0,
 * fmt 1 / 2 on an fp32 engine, A / W not 16-byte aligned (MFMA form). */
int svln_op_gemv_argmax_scores(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                               float penalty, int32_t* host_token, float* host_logprob);
/* TEST-ONLY: the single-env head under svln_top_logprobs on caller-given operands (fmt / W / aux / pen_flags as
 * svln_op_gemv_argmax_scores, plus fmt 3 = the 12-bit packing with W the bf16 original and aux the packed rows followed by the row
 * records): the EPI_ARGMAX_LSE_TOPK product (sampled != 0: EPI_SAMPLE_TOPK on temperature, seed, stream, draw), the final kernel and
 * the merge.  Outputs (host): the token and its score; the partial arrays [*n_part] (part_raw / part_max: sampled form only, may be null
 * otherwise); the candidates [*n_part][8]; the merged lists [k].  Arrays must hold 1280 partials.  The refusals of
 * svln_op_gemv_argmax_scores / _sample apply, plus k outside 1 .. 8 and null outputs -- before any launch. */
int svln_op_gemv_argmax_topk(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                             float penalty, int k, int sampled, float temperature, uint64_t seed, int32_t stream, int32_t draw, int32_t* host_token,
                             float* host_logprob, float* part_val, int32_t* part_idx, float* part_sum, float* part_raw, float* part_max,
                             float* cand_val, int32_t* cand_idx, int32_t* top_ids, float* top_logprobs, int32_t* n_part);
/* TEST-ONLY: the batched GEMV (B = 1, 2, 4, 8; no fused norm) and the 32 x 128 MFMA tiles (1 <= M <= 32) under svln_top_logprobs, arguments
 * as svln_op_gemv_batched_argmax_sample / svln_op_gemm_argmax_sample (sampled == 0: the greedy form, streams / draws unread).  Outputs
 * (host): tokens and scores [rows]; candidates [rows][*n_part][8]; lists [rows][k]; the partial arrays stay readable through
 * svln_op_read_argmax_partials, as after the scored entries.  Same refusals, plus k outside 1 .. 8 and null outputs, before any launch. */
int svln_op_gemv_batched_argmax_topk(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int N, int K, int B, const void* pen_flags,
                                     const int32_t* pen_rows, float penalty, int k, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                                     const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* cand_val, int32_t* cand_idx,
                                     int32_t* top_ids, float* top_logprobs, int32_t* n_part);
int svln_op_gemm_argmax_topk(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                             const int32_t* pen_rows, float penalty, int k, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                             const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* cand_val, int32_t* cand_idx, int32_t* top_ids,
                             float* top_logprobs, int32_t* n_part);
/* TEST-ONLY: the three lm_head forms under svln_token_entropy on caller-given operands -- the EPI_ARGMAX_LSE_ENT product (sampled != 0:
 * EPI_SAMPLE_ENT on temperature, seed, stream(s), draw(s)), the entropy merge and the scored / sampled final kernel.  Arguments as
 * svln_op_gemv_argmax_topk (fmt 0 .. 3), svln_op_gemv_batched_argmax_topk and svln_op_gemm_argmax_topk without k and the lists.  Outputs
 * (host): tokens, scores and entropies [rows]; the partial arrays [rows][*n_part] including part_ent (part_raw / part_max: sampled form
 * only, may be null otherwise).  Arrays must hold 2048 partials per row.  The refusals of the _scores / _sample entries apply, plus null
 * outputs -- before any launch. */
int svln_op_gemv_argmax_entropy(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                                float penalty, int sampled, float temperature, uint64_t seed, int32_t stream, int32_t draw, int32_t* host_token,
                                float* host_logprob, float* host_entropy, float* part_val, int32_t* part_idx, float* part_sum, float* part_raw,
                                float* part_max, float* part_ent, int32_t* n_part);
int svln_op_gemv_batched_argmax_entropy(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int N, int K, int B, const void* pen_flags,
                                        const int32_t* pen_rows, float penalty, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                                        const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* host_entropies, float* part_val,
                                        int32_t* part_idx, float* part_sum, float* part_raw, float* part_max, float* part_ent, int32_t* n_part);
int svln_op_gemm_argmax_entropy(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                                const int32_t* pen_rows, float penalty, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                                const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* host_entropies, float* part_val,
                                int32_t* part_idx, float* part_sum, float* part_raw, float* part_max, float* part_ent, int32_t* n_part);
/* TEST-ONLY: the merge kernel of svln_token_entropy on host partial rows [B][n_part] (layout and meaning of the epilogues' arrays).
 * part_max null: the greedy form, the sums are relative to part_val and (V, none) come from (part_val, part_idx); else the sampled form
 * on (part_max, part_sum).  part_ent null: every t is 0 (one id per partial, the subset product).  host_entropies [B].  Refused before
 * any launch: B outside 1 .. 32, n_part outside 1 .. 2048 (checked first), then null part_val / part_idx / part_sum / host_entropies. */
int svln_op_entropy_merge(svln_engine* h, const float* part_val, const int32_t* part_idx, const float* part_sum, const float* part_max,
                          const float* part_ent, int B, int n_part, float* host_entropies);
/* TEST-ONLY: the truncation kernel of svln_sampling_truncation followed by the batched sampled final kernel, on host candidates
 * cand_val / cand_idx [B][n_part][c] (c = 8: lists as the EPI_SAMPLE_TOPK epilogues write them, padded with (-inf, 0x7FFFFFFF); c = 1:
 * one candidate per partial, as under an allowed list).  The values are y as they stand (already times 1 / T: `temperature` is checked
 * and otherwise unused); row b uses streams[b] / draws[b].  Outputs (host): the five 8-entry partial rows [B][8], tokens [B] and scores
 * [B].  Refused before any launch: null pointers, B outside 1 .. 32, n_part < 1, c not 1 or 8, n_part x c > 16384, top_k outside 1 .. 8,
 * top_p not in (0, 1], a negative column, stream or draw, a temperature that is not finite and > 0. */
int svln_op_truncate(svln_engine* h, const float* cand_val, const int32_t* cand_idx, int B, int n_part, int c, const int32_t* streams,
                     const int32_t* draws, uint64_t seed, float temperature, int32_t top_k, float top_p, float* part_val, int32_t* part_idx,
                     float* part_raw, float* part_max, float* part_sum, int32_t* host_tokens, float* host_logprobs);
int svln_op_gemv_batched_argmax_scores(svln_engine* h, const void* W, int ldw, const void* x, int ldx, const void* norm_w, float eps, int N, int K, int B,
                                       const void* pen_flags, const int32_t* pen_rows, float penalty, int32_t* host_tokens, float* host_logprobs);
int svln_op_gemm_argmax_scores(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                               const int32_t* pen_rows, float penalty, int32_t* host_tokens, float* host_logprobs);
/* TEST-ONLY entries: the EPI_TARGET forms (svln_generate_forced) of the two batched entries above and their final kernel, whatever the
 * engine's switches say.  targets [B] / [M] host: -1 (no column: that row's log-probability is NaN and nothing is captured) or a column
 * of [0, N); inv_t > 0 scales every logit before the compares, sums and the capture (1.0f: the scored form's bits).  host_tokens /
 * host_greedy_logprobs: the arg-max and its log-probability, host_logprobs: the targets'.  No fused norm, no penalty.  The refusals of
 * the entries above apply (B in {2, 4, 8}), plus a target outside [-1, N), inv_t not finite or <= 0, a null output -- before any launch.
 * host_slots (optional, 32 floats): in, what the 32 capture slots hold before the launch; out, what they hold after it (row m's captured
 * y in slot m, every other slot untouched).
 * svln_op_read_argmax_partials: the [rows][n] arg-max partials (value, index, sum) the last batched test product left. */
int svln_op_gemv_batched_target(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int N, int K, int B, const int32_t* targets, float inv_t,
                                int32_t* host_tokens, float* host_greedy_logprobs, float* host_logprobs, float* host_slots);
int svln_op_gemm_target(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const int32_t* targets, float inv_t,
                        int32_t* host_tokens, float* host_greedy_logprobs, float* host_logprobs, float* host_slots);
int svln_op_read_argmax_partials(svln_engine* h, int rows, int n, float* val, int32_t* idx, float* sum);
/* TEST-ONLY entries: the sampled forms (EPI_SAMPLE, see svln_set_sampling) of the three entries above, on the given temperature, seed
 * and per-row streams / draws (host values; the engine's own switch and counters are not touched).  host_logprob(s) receive
 * log softmax(x / T)[token] and must not be null.  The refusals of the entries above apply, plus: temperature not finite or <= 0,
 * negative streams / draws, and norm_w with the batched form (it has no fused-norm kernel) -- all before any launch.
 * svln_op_gumbel: host_out[k] = G(seed, stream, draw, n0 + k) for k < count, as the kernels evaluate it. */
int svln_op_gemv_argmax_sample(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                               float penalty, float temperature, uint64_t seed, int32_t stream, int32_t draw, int32_t* host_token, float* host_logprob);
int svln_op_gemv_batched_argmax_sample(svln_engine* h, const void* W, int ldw, const void* x, int ldx, const void* norm_w, float eps, int N, int K, int B,
                                       const void* pen_flags, const int32_t* pen_rows, float penalty, float temperature, uint64_t seed,
                                       const int32_t* streams, const int32_t* draws, int32_t* host_tokens, float* host_logprobs);
int svln_op_gemm_argmax_sample(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                               const int32_t* pen_rows, float penalty, float temperature, uint64_t seed, const int32_t* streams,
                               const int32_t* draws, int32_t* host_tokens, float* host_logprobs);
int svln_op_gumbel(svln_engine* h, uint64_t seed, int32_t stream, int32_t draw, int32_t n0, int32_t count, float* host_out);
/* TEST-ONLY: one subset product of svln_set_allowed_tokens (gemv_subset.hip) on caller-given operands; the engine's own list and switches
 * are not touched.  W [V][ldw], x [B][ldx] device, engine dtype; ids [n] host (the rules of svln_set_allowed_tokens with vocab = V);
 * 1 <= B <= 32; K a positive multiple of the 16-byte chunk, ldw, ldx >= K and multiples of it.  pen_flags (device, optional) [.][V] with
 * pen_rows (device, optional, [B]; null = every row uses flag row 0) and penalty > 0.  temperature == 0: greedy; > 0: sampled with
 * seed and the host arrays streams / draws [B]; anything else (negative, NaN, inf) is refused.  Returns host_tokens [B], host_logprobs
 * [B], host_y [B][n] (the processed values y) and host_dist [B][n] (y - logsumexp y).  Malformed calls are refused before any launch. */
int svln_op_subset_argmax(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int V, int K, int B, const int64_t* ids, int n,
                          const void* pen_flags, const int32_t* pen_rows, float penalty, float temperature, uint64_t seed, const int32_t* streams,
                          const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* host_y, float* host_dist);
/* the row helpers between the products (misc.hip), rows of n values of the engine type on the device.  Every op refuses null pointers,
 * rows < 0 and an n that is not a positive multiple of the 16-byte chunk (8 bf16 / 4 fp32 values: the kernels move whole chunks). */
int svln_op_rmsnorm(svln_engine* h, const void* x, const void* g, void* y, int rows, int n, float eps);
int svln_op_layernorm(svln_engine* h, const void* x, const void* g, const void* b, void* y, int rows, int n, float eps);
/* the RMSNorm launch of a graph-replayed decode step: a device skip word (non-zero: nothing is written) and a second copy of the rows at
 * row min(y2_row_value + r, y2_cap - 1) of y2, the row index read from a device word */
int svln_op_rmsnorm_tap(svln_engine* h, const void* x, const void* g, void* y, int rows, int n, float eps, int skip_value, void* y2, int y2_row_value,
                        int y2_cap);
/* y[r] = RMSNorm(x[src_rows[r]]), copied to tap[tap_rows[r]] unless that is -1.  src_rows / tap_rows: host arrays of `rows` ints, refused
 * when an entry lies outside [0, x_rows) / [-1, tap_cap) */
int svln_op_rmsnorm_indexed(svln_engine* h, const void* x, int x_rows, const void* g, void* y, const int32_t* src_rows, const int32_t* tap_rows,
                            void* tap, int tap_cap, int rows, int n, float eps);
/* out[r] = embed[src[r]] for src[r] >= 0, feats[-(src[r] + 1)] otherwise (the embedding splice); src: host array, refused outside
 * [-feat_rows, embed_rows).  A non-zero skip_value (a device word, like GenCtl.done) leaves out untouched. */
int svln_op_gather_rows(svln_engine* h, const int32_t* src, int rows, const void* embed, int embed_rows, const void* feats, int feat_rows, void* out,
                        int n, int skip_value);
/* out[list[2 i]] = embed[list[2 i + 1]] for i < rows; list: host array of (destination row, token id) pairs, refused outside
 * [0, out_rows) / [0, embed_rows) */
int svln_op_gather_rows_ragged(svln_engine* h, const int32_t* list, int rows, const void* embed, int embed_rows, void* out, int out_rows, int n);
/* the 128-bit content keys of the feature cache: F frames of words_per_frame 32-bit words each (device) -> out_keys[2 F] (host) */
int svln_op_frame_hash(svln_engine* h, const void* pix_dev, int F, int64_t words_per_frame, uint64_t* out_keys);
/* attention over caller-provided q [T][q_stride] and k/v [S][kv_stride] (engine packs them into pages):
 * llm: rope = 1 applies RoPE at positions P + i to q and k (head_dim 128, GQA G = nq/nkv, causal)
 * vit: head_dim 72, non-causal, frames * heads */
int svln_op_attention_llm(svln_engine* h, void* qkv, int ld, int T, int P, const void* ctx_qkv, int ctx_T, void* out, int o_stride,
                          int nsplit);
int svln_op_attention_vit(svln_engine* h, const void* qkv, int ld, int F, void* out, int o_stride);
/* one decode step of B in {1, 2, 4, 8} envs on layer 0, through the engine's own decode attention (fused RoPE of q / k, K / V append,
 * split-KV partials + merge).  Env b first gets pos[b] context rows (ctx_qkv + b * ctx_rows * ld, roped in place + appended as in
 * svln_op_attention_llm), then its un-roped q|k|v row qkv_new[b * ld] is decoded at position pos[b] -> out[b * o_stride].
 * B == 1 takes the single-env step, B > 1 the batched one.  B == 1 with ctx_qkv == NULL and pos[0] > 0: env 0 is NOT reset and nothing is
 * re-appended -- the step runs on the pages and rows the last op left (which must cover the position), e.g. behind
 * svln_op_attention_verify, whose appended rows it then reads. */
int svln_op_attention_decode(svln_engine* h, int B, const void* ctx_qkv, int ld, int64_t ctx_rows, const int32_t* pos, const void* qkv_new,
                             void* out, int o_stride);
/* the attention of one verify pass (svln_set_speculative) on layer 0 / env 0, through the engine's own verify attention.  Env 0 first gets
 * ctx_rows context rows as in svln_op_attention_decode, then the `rows` (1 .. 8, rows * G <= 32) un-roped q|k|v rows qkv_new[i * ld] are
 * verified at positions ctx_rows + i -> out[i * o_stride]: RoPE of q / k per row, K / V append of every row (the rows may straddle a
 * page), per-row causal mask, split-KV partials + merge.  svln_op_kv_read / svln_op_set_pages / svln_op_fill_attn_state work with it as
 * with the decode op. */
int svln_op_attention_verify(svln_engine* h, int rows, const void* ctx_qkv, int ld, int ctx_rows, const void* qkv_new, void* out,
                             int o_stride);
/* TEST-ONLY: the batched verify attention (a scoring pass of svln_generate_candidates) on layer 0 / envs 0 .. n_seq - 1.  Sequence s gets
 * ctx_len[s] context rows (ctx_qkv + s * ctx_rows * ld), then rows[s] (0 .. rows_max) of its rows_max row slots qkv_new[s * rows_max ..]
 * are verified at positions ctx_len[s] ...; out [n_seq * rows_max][o_stride] keeps the caller's bytes in every row the launch leaves alone.
 * share != 0: the fork layout (equal context lengths; sequence s >= 1 runs on env 0's pages below ctx_len / 64 and on env s's own pages
 * from there on, the partly filled page copied by the fork launch).  Refused before any launch: n_seq outside 1 .. 8,
 * rows_max * (q_heads / kv_heads) > 32, a row count outside 0 .. rows_max, a position at or past max_positions, a position in a page the
 * sequence's list (svln_op_set_pages) does not hold. */
int svln_op_attention_verify_multi(svln_engine* h, int n_seq, int rows_max, const void* ctx_qkv, int ld, int ctx_rows, const int32_t* ctx_len,
                                   const void* qkv_new, const int32_t* rows, int share, void* out, int o_stride);
/* one verify-step launch on caller-given host arrays: fed[rows] = the tokens the rows were fed (fed[0] is not read), cand[rows] = their
 * arg-maxes, from `count` emitted tokens, with max_new and eos[n_eos <= 16] as svln_generate takes them.  *new_count, *done, the emitted
 * ids in emitted[0 .. *new_count - count) (the rest of emitted[rows] = -3) and *next_token (the last emitted token; -3 when none). */
int svln_op_verify_step(svln_engine* h, int rows, const int32_t* fed, const int32_t* cand, int count, int max_new, const int64_t* eos,
                        int n_eos, int32_t* new_count, int32_t* done, int64_t* emitted, int32_t* next_token);
/* TEST-ONLY: one launch of draft_select_kernel (the select step of svln_generate_drafts) on caller-given host arrays: k[G] rows per draft,
 * fed[G][r] the ids the row slots were fed, cand[1 + sum k] the head rows' arg-maxes (row 0 = the prompt's last row, then the rows of
 * draft 0, 1, ...), cand_score (optional, with scores) their log-probabilities; the GenCtl start state pos, kv_len, done, count, max_new;
 * eos[n_eos].  Final-norm row q holds q + 1 + (column % 4) / 4 in every column.  Before the launch every output is filled with a
 * sentinel: out_ids[rows] -7, scores[rows] NaN, *last_token -7, rec[4] -7, the tap rows -1; stats[2] is read and written (passes, tokens).
 * Afterwards ctl_out[8] = the final GenCtl, rec = {winner, emitted, stop, head rows read}, taps [tap_rows][hidden] = the first tap rows.
 * Refused before any launch: G outside 1 .. 8, r < 1 or 1 + G r > 33, a k outside 0 .. r, count < 0 or count + r + 1 > rows, rows beyond
 * the engine's id buffer, n_eos beyond its EOS buffer, cand_score without scores or the reverse, more than 64 tap rows, a null array.
 * The engine's own d_ctl, d_out_ids, d_scores and d_token are restored afterwards. */
typedef struct svln_draft_select_op {
    const int32_t* k; const int32_t* fed; const int32_t* cand; const float* cand_score; const int64_t* eos;
    int32_t* ctl_out; int32_t* out_ids; int32_t* last_token; float* scores; int32_t* rec; int32_t* stats; float* taps;
    int32_t G, r, pos, kv_len, done, count, max_new, n_eos, rows, tap_rows;
} svln_draft_select_op;
int svln_op_draft_select(svln_engine* h, const svln_draft_select_op* op);
/* TEST-ONLY: `steps` launches of the greedy loop's step kernel (launch_argmax_step; use_ctl = 0: ONE launch_argmax_final on set 0) on
 * caller-given host partials, enqueued back to back with no host synchronisation between them; launch s reads partial set s.
 *   part_val / part_idx [steps][n]; part_sum (optional: the scored merge), part_raw / part_max (optional, both or neither, with
 *   part_sum: the sampled merge); the GenCtl start state pos, kv_len, done, count, max_new; eos[n_eos] (n_eos may be 0);
 *   flag_bytes > 0: the step kernel sets the emitted token's byte in a flag array of that many bytes (every live part_idx must lie
 *   below it), 0: no flags.
 * Before the first launch every output is filled with a sentinel: out_ids[rows] -7, scores[rows] NaN, *last_token -7, out_top[2] NaN,
 * flags[flag_bytes] 0x5A.  Afterwards ctl_out[8] = the final GenCtl (pos, kv_len, done, count, max_new, n_eos, draw0, stream) and the
 * five arrays as the launches left them.  `rows` is the capacity of out_ids / scores the launches run against.
 * Refused before any launch: n outside 1 .. 2048, steps outside 1 .. 8, count < 0 or count + steps > rows, rows beyond the engine's id
 * buffer, n_eos beyond its EOS buffer, part_raw without part_max or either without part_sum, a null array the chosen form reads, a live
 * part_idx outside the flag array.  The engine's own generation state is restored afterwards. */
typedef struct svln_argmax_step_op {
    const float* part_val; const int32_t* part_idx; const float* part_sum; const float* part_raw; const float* part_max;
    const int64_t* eos;
    int32_t* ctl_out; int32_t* out_ids; int32_t* last_token; float* out_top; float* scores; uint8_t* flags;
    int32_t n, steps, use_ctl, pos, kv_len, done, count, max_new, n_eos, flag_bytes, rows;
} svln_argmax_step_op;
int svln_op_argmax_step(svln_engine* h, const svln_argmax_step_op* op);
/* TEST-ONLY: one decode step behind a finished (done != 0) or a running (done = 0) generation.  Env 0 must hold a prompt that the public
 * calls have prefilled and generated from.  The entry sets GenCtl.done = done, fills the id rows behind the generation
 * (d_out_ids[count ..), never read) with -7 so that a live append always shows, snapshots every buffer a step may touch, enqueues exactly
 * what one replayed step enqueues (decode_ops over the whole step, then head(x, count, true); the captured one-step graph while
 * svln_set_decode_graph is on), and compares.  report (report_cap bytes, NUL-terminated) gets one line per buffer:
 *   "<name> <bytes> <changed bytes> <first changed offset or -1> <last changed offset or -1>\n"
 * for the K and V^T pools of every layer (kpool.<i>, vpool.<i>), attn_part, x, qkv, attn, hbuf, head_xn, hid_tap, the partial, candidate
 * and truncation arrays, d_token, d_out_ids, d_scores, d_topi, d_topl, d_ent, d_alp, pen_flags, d_top2, the granule and sequence words
 * of the persistent layer (dl_gran.<k>, dl_seq) and ctl (GenCtl itself, compared with the state AFTER done was set); buffers the engine
 * has not allocated are left out.  *n_changed = the buffers with a changed byte.  With done = 0 the step is live: it writes the KV slot
 * of GenCtl.pos and appends a token; the env's host-side bookkeeping does not follow, so reset the env before the next public call. */
int svln_op_dead_step(svln_engine* h, int done, char* report, int report_cap, int32_t* n_changed);
/* roped K and V rows of positions [start, start + n) of env's layer-0 KV pages -> host fp32 [n][kv_heads][128] each; env = -1 reads
 * the raw pools (position p = slot p % 64 of physical page p / 64).  The attention ops reset their envs on entry only, so this reads
 * what the last op wrote. */
int svln_op_kv_read(svln_engine* h, int env, int start, int n, float* k_out, float* v_out);
/* the same raw-pool read (env = -1 above) on the K / V^T pools of any layer */
int svln_op_kv_pool_read(svln_engine* h, int layer, int start, int n, float* k_out, float* v_out);
/* TEST-ONLY: one launch of kv_page_copy_kernel (the fork of svln_generate_group): physical page src_page is copied to the n_dst pages of the
 * host list dst_pages in every layer's K and V^T pool.  Refused before any launch: a null list, n_dst outside 1 .. 7, a page outside the
 * pool, a destination equal to the source or listed twice, a destination held by an env (or by a pending group). */
int svln_op_kv_page_copy(svln_engine* h, int src_page, const int32_t* dst_pages, int n_dst);
/* TEST-ONLY: one launch of kv_page_gather_kernel (the KV hand-over between the hypotheses of a beam step): physical page src_pages[i] is
 * copied to page dst_pages[i], i < n, in every layer's K and V^T pool; one source may serve several destinations.  Refused before any
 * launch: a null list, n outside 1 .. 64, a page outside the pool, a page that is both a source and a destination, a destination listed
 * twice, a destination held by an env (or by a pending group). */
int svln_op_beam_page_gather(svln_engine* h, const int32_t* src_pages, const int32_t* dst_pages, int n);
/* TEST-ONLY: one launch of beam_select_kernel, the select step of a beam search over the lm_head's top-W lists, on a caller-given
 * hypothesis set (rank = index, at most 8 hypotheses of at most len_cap <= 64 ids).
 *   in : hdr_in int32 [25] = n, len[8], fin[8], set_of[8]; score_in [8]; ids_in / lps_in [8][len_cap]; list_ids / list_lps [8][W], row =
 *        rank (rows of finished ranks are not read; id -1 = no entry); eos [n_eos]; set_pages [16][n_cp] (may be null when n_cp = 0);
 *        tok_b [B] holds the caller's bytes on entry
 *   rule: pool = every finished hypothesis (score unchanged) + every entry (r, j) with id >= 0 of a live one, score fl(score_r + lp_rj);
 *        the new set = the best W by score descending, then r, then j ascending; a new hypothesis is finished when its last id is in eos
 *        or its length equals limit; tok_b[k] = the last id of rank k if it is live, else of the first live rank (untouched: none is
 *        live); rank c keeps its parent's page set if no earlier rank took it, else takes the lowest set that neither the old set holds
 *        nor an earlier rank took, and the first n_cp pages of the two sets are listed in pair_src / pair_dst [8 * n_cp]
 *   out: hdr_out / score_out / ids_out / lps_out as the inputs (entries past the new n are unspecified; ids_out / lps_out keep the caller's
 *        bytes where the kernel writes nothing); rec int32 [28] = n_new, live now, live before, pairs, parent rank [8], entry [8], page
 *        set [8] (-1 = unused)
 * Refused before any launch: a null pointer, W outside 1 .. 8, len_cap outside 1 .. 64, limit outside 1 .. len_cap, B or n_eos outside
 * their ranges, n_cp outside 0 .. 8, n outside 0 .. 8, a flag that is not 0 / 1, a length outside 0 .. len_cap or not below limit for a
 * live hypothesis, a page set outside 0 .. 15 or held twice. */
int svln_op_beam_select(svln_engine* h, int W, int limit, int B, int n_cp, int len_cap, const int32_t* eos, int n_eos, const int32_t* list_ids,
                        const float* list_lps, const int32_t* hdr_in, const float* score_in, const int32_t* ids_in, const float* lps_in,
                        const int32_t* set_pages, int32_t* hdr_out, float* score_out, int32_t* ids_out, float* lps_out, int32_t* tok_b,
                        int32_t* pair_src, int32_t* pair_dst, int32_t* rec);
/* the prefill q|k|v product of one env's turn on layer 0 (env 0, positions P .. P + T - 1) as a prefill runs it: x = the normed input
 * rows [T][hidden] (device); roped q rows -> q_out [T][q_stride], roped k / v appended to env 0's pages; *fused = 1 when the product's
 * split-K reduce did the RoPE + append, 0 when the separate RoPE + append kernel did */
int svln_op_llm_qkv_rope(svln_engine* h, const void* x, int T, int P, void* q_out, int q_stride, int32_t* fused);
/* TEST-ONLY: the separate RoPE + append launch on caller rows: rows [T][ld] (device, engine dtype; q | k | v of one row side by side,
 * ld >= (q_heads + 2 kv_heads) * 128) at positions P .. P + T - 1 of env 0 on the layer-0 pools, through the pages svln_op_set_pages
 * fixed for env 0.  q is roped in place; roped k and v go to the env's pages.  With n_mirror > 0 (the folded candidates call's form) every
 * k / v row whose position lies in logical page q0 = (P + T) / 64 is stored a second time, same values and in-page offsets, to each of
 * the physical pages mirror_pages[0 .. n_mirror) in every kv head; n_mirror == 0 is the plain launch.
 * Refused before the env is reset or anything is launched: n_mirror outside 0 .. 7; a mirror page outside the pool, equal to the env's
 * page q0 (or any page fixed for the env), or listed twice; positions beyond the env's pages or max_positions; no pages fixed. */
int svln_op_rope_kv_mirror(svln_engine* h, void* rows, int ld, int T, int P, const int32_t* mirror_pages, int n_mirror);
/* test control: the attention ops give env these pages (in this order: logical page i -> pages[i]); n = 0 restores the free list */
int svln_op_set_pages(svln_engine* h, int env, const int32_t* pages, int n);
/* test control: fill the layer-0 K / V pools with a finite value and (part_nan) the split-KV partial workspace with NaN */
int svln_op_fill_attn_state(svln_engine* h, float pool_value, int part_nan);
/* ViT layer `layer`'s q|k|v product and attention as the vision tower runs them (the product packs the K / V^T pages where its launch
 * can): x = the normed rows [F * 729][v_hidden] (device), qkv_out [F * 729][3 * v_hidden], attn_out [F * 729][o_stride]; *packer = the
 * writer of the pages: 0 = the standalone packer, 1 = the split-K reduce, 2 = the 128x128 tile epilogue.  force_split: 0 = the
 * engine's own launch choice; > 1 = that many K splits (tests: the reduce's fused pack at shapes where the engine does not split) */
int svln_op_vit_qkv_attention(svln_engine* h, int layer, const void* x, int F, void* qkv_out, void* attn_out, int o_stride,
                              int force_split, int32_t* packer);
/* test control: fill the ViT K / V^T pools with a finite value and (part_nan) the split-KV partial workspace with NaN */
int svln_op_fill_vit_state(svln_engine* h, float pool_value, int part_nan);
/* the raw ViT pools over their whole allocation (pages = key tiles * max_frames * v_heads) -> host fp32 K [page][64][HDP] and
 * V^T [page][VROWS][64] (HDP = head dim padded to an even number of 16-byte chunks, VROWS = 96) */
int svln_op_vit_kv_read(svln_engine* h, float* k_out, float* v_out);
int svln_op_pool(svln_engine* h, const void* in, void* out, int F);
int svln_op_patchify(svln_engine* h, const float* pix, void* out, int F);

#ifdef __cplusplus
}
#endif
#endif
