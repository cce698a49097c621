// Host-side launch interface of the hand-written gfx950 kernels.  One launcher per kernel,
// each instantiated for T = bf16 (shipping) and T = float (parity mode).  Launchers only
// enqueue on `stream` (no allocation, no sync) so a caller may capture them in a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>
#include <vector>

namespace svln {

enum Epi : int { EPI_NONE = 0, EPI_GELU_TANH = 1, EPI_GELU_ERF = 2, EPI_SWIGLU = 3, EPI_ARGMAX = 4, EPI_ARGMAX_LSE = 5, EPI_SAMPLE = 6, EPI_TARGET = 7,
                 EPI_ARGMAX_LSE_TOPK = 8, EPI_SAMPLE_TOPK = 9, EPI_ARGMAX_LSE_ENT = 10, EPI_SAMPLE_ENT = 11 };
// EPI_ARGMAX_LSE (svln_set_token_scores): EPI_ARGMAX -- same accumulators, same compares, same partials, hence the same tokens -- plus one
// fp32 per partial, part_sum[k] = sum exp(l_j - part_val[k]) over the (penalised) logits partial k owns.  The final kernels merge them,
// S = sum_k part_sum[k] * exp(part_val[k] - V) with V the winning value, and write the token's log-probability -log S.  A partial that
// owns no logit has (max -inf, sum 0) and merges as 0.
// EPI_SAMPLE (svln_set_sampling): temperature sampling as an arg-max (Gumbel-max).  With x the processed fp32 logit of column n (after the
// repetition penalty), y = fl(x * inv_t) and z = y + G(seed, stream, draw, n) (gumbel_noise, common.h: a pure function of those four), the
// token is argmax_n z, lowest column on ties.  A partial carries five values: part_val = its best z, part_idx, part_raw = the y of that
// winner, part_max = max y, part_sum = sum exp(y - part_max) over the logits it owns (-inf, 0 for none).  The final kernels pick the token
// on (part_val, part_idx), take the part_raw of the partial that owns it (a column belongs to one partial), V = max_k part_max[k],
// S = sum_k part_sum[k] * exp(part_max[k] - V), and write the token's log-probability under softmax(x * inv_t): part_raw - V - log S.
// EPI_TARGET (svln_generate_forced): the EPI_ARGMAX_LSE partials on y = fl(x * inv_t) -- no penalty, no noise; inv_t is exactly 1.0f with
// sampling off, so tokens and partials are then the scored form's bit for bit -- plus the capture of ONE named column per row: the lane
// that holds column tgt[m] of a live row m stores tgt_val[m] = y (one plain store per row in the whole grid; -1 names no column).  The
// final kernel (launch_target_final_batched) writes the arg-max, its log-probability -log S and the target's, (tgt_val - V) - log S.
// EPI_ARGMAX_LSE_TOPK / EPI_SAMPLE_TOPK (svln_top_logprobs; every lm_head form: wave-per-rows GEMV, batched GEMV, 32 x 128 MFMA tiles): EPI_ARGMAX_LSE / EPI_SAMPLE -- the same accumulators,
// compares and partials, hence the same tokens, scores and partial arrays bit for bit -- and beside every arg-max partial its TOPK_C best
// (y, column) pairs among the columns it owns, y descending then column ascending, padded with (-inf, 0x7FFFFFFF): cand_val / cand_idx
// [partials][TOPK_C].  y is the processed logit (after the penalty), times inv_t under sampling -- never the perturbed z.  NaN and -inf are
// never listed.  A column of the row's top k <= TOPK_C is in the top k of the partial that owns it, so launch_topk_merge is exact.
// EPI_ARGMAX_LSE_ENT / EPI_SAMPLE_ENT (svln_token_entropy; every lm_head form): EPI_ARGMAX_LSE / EPI_SAMPLE -- the same accumulators, compares
// and partials, hence the same tokens, scores and partial arrays bit for bit -- plus one more fp32 per partial, part_ent[k] = sum (y_j -
// m_k) exp(y_j - m_k) over the columns partial k owns, m_k the maximum part_sum[k] is relative to (part_val when greedy, smp.part_max when
// sampled); y as in the _TOPK forms, never the perturbed z.  A -inf column adds 0, the partial that owns nothing has 0.
// launch_entropy_merge turns them into the row's entropy log S - T / S.
constexpr int TOPK_C = 8;
// The lm_head form: the five facts every EPI_* arg-max sibling is made of.  ONE table, read by the kernels (constexpr HeadForm F =
// head_form(EPI)), the launchers (with_head_epi) and the engine (which builds a form from its switches and asks head_epi for the kernel).
//   lse   part_sum is kept relative to part_val (the greedy scored sums).  EPI_TARGET carries it too: where a kernel body says LSE it means
//         F.lse, forced form included (batched GEMV, MFMA epilogue, subset product; the wave-per-rows GEMV has no forced sibling)
//   smp   Gumbel-max sampling: part_sum is relative to smp.part_max, beside smp.part_raw; never together with lse
//   tgt   the capture of one named column per row (with lse, nothing else)
//   topk  TOPK_C candidates beside every partial (cand_val / cand_idx);  ent: part_ent beside every partial sum (never with topk)
struct HeadForm { bool lse, smp, tgt, topk, ent; };
constexpr bool operator==(HeadForm a, HeadForm b) { return a.lse == b.lse && a.smp == b.smp && a.tgt == b.tgt && a.topk == b.topk && a.ent == b.ent; }
constexpr int HEAD_EPIS[] = {EPI_TARGET, EPI_SAMPLE_TOPK, EPI_ARGMAX_LSE_TOPK, EPI_SAMPLE_ENT, EPI_ARGMAX_LSE_ENT, EPI_SAMPLE, EPI_ARGMAX_LSE, EPI_ARGMAX};      // all eight
constexpr HeadForm head_form(int epi) {      // (an epilogue that is no arg-max form has no fact)
    return HeadForm{epi == EPI_ARGMAX_LSE || epi == EPI_TARGET || epi == EPI_ARGMAX_LSE_TOPK || epi == EPI_ARGMAX_LSE_ENT,
                    epi == EPI_SAMPLE || epi == EPI_SAMPLE_TOPK || epi == EPI_SAMPLE_ENT, epi == EPI_TARGET,
                    epi == EPI_ARGMAX_LSE_TOPK || epi == EPI_SAMPLE_TOPK, epi == EPI_ARGMAX_LSE_ENT || epi == EPI_SAMPLE_ENT};
}
constexpr int head_epi(HeadForm f) {         // -1: a combination nobody has built a kernel for
    for (int e : HEAD_EPIS) if (head_form(e) == f) return e;
    return -1;
}
constexpr bool epi_is_argmax(int epi) { return head_epi(head_form(epi)) == epi; }
constexpr bool head_round_trip() { for (int e : HEAD_EPIS) if (!epi_is_argmax(e)) return false; return true; }
static_assert(sizeof(HEAD_EPIS) / sizeof(int) == 8 && head_round_trip() && !epi_is_argmax(EPI_NONE) && !epi_is_argmax(EPI_SWIGLU), "head_form / head_epi: the eight arg-max forms round-trip");
static_assert(head_epi({true, false, false, true, true}) == -1 && head_epi({false, true, false, true, true}) == -1, "no entropy form with candidates");
static_assert(head_epi({false, false, true, false, false}) == -1 && head_epi({true, true, true, false, false}) == -1 && head_epi({true, false, true, true, false}) == -1 &&
              head_epi({true, false, true, false, true}) == -1 && head_epi({true, true, false, false, false}) == -1, "tgt rides on lse alone; lse and smp exclude each other");
// Which siblings each product form is instantiated for: the 32 x 128 MFMA epilogue has all of HEAD_EPIS, gemv_mx4b has EPI_ARGMAX only.
// ONE dispatcher (with_head_epi<LIST>) turns a run-time epi into a kernel and for_each_head_epi<LIST> visits the same set for the attributes.
// The ORDER of a list (HEAD_EPIS too) is the order in which the product's kernels stand in the code object, kept so that it stays byte for byte.
constexpr int GEMV_ROWS_EPIS[] = {EPI_ARGMAX, EPI_ARGMAX_LSE, EPI_SAMPLE, EPI_ARGMAX_LSE_TOPK, EPI_SAMPLE_TOPK, EPI_ARGMAX_LSE_ENT, EPI_SAMPLE_ENT};      // wave-per-rows GEMV: no forced form
constexpr int GEMV_BATCHED_EPIS[] = {EPI_ARGMAX, EPI_ARGMAX_LSE, EPI_SAMPLE, EPI_SAMPLE_TOPK, EPI_ARGMAX_LSE_TOPK, EPI_SAMPLE_ENT, EPI_ARGMAX_LSE_ENT, EPI_TARGET};
constexpr bool gemv_batched_norm_has(int epi) { return epi == EPI_ARGMAX || epi == EPI_ARGMAX_LSE; }    // ... of which the fused-norm variant exists for two
constexpr int GEMV_SUBSET_EPIS[] = {EPI_ARGMAX, EPI_ARGMAX_LSE, EPI_SAMPLE, EPI_TARGET};                // subset product: one id per partial, so no lists and t = 0
// f(std::integral_constant<int, EPI_...>{}) for the form `epi` names if list L has it, else false (L backwards: a fold's kernels are emitted last first)
template <auto& L, class F, size_t... I> bool with_head_epi_at(int epi, F&& f, std::index_sequence<I...>) {
    return ((epi == L[sizeof...(I) - 1 - I] ? (f(std::integral_constant<int, L[sizeof...(I) - 1 - I]>{}), true) : false) || ...);
}
template <auto& L, class F> bool with_head_epi(int epi, F&& f) { return with_head_epi_at<L>(epi, f, std::make_index_sequence<sizeof(L) / sizeof(int)>{}); }
template <auto& L, class F> void for_each_head_epi(F&& f) { for (int e : L) with_head_epi<L>(e, f); }
// Inputs of EPI_TARGET: tgt [rows] device ids (-1: none), tgt_val [rows] the captured y
struct TargetArgs { const int* tgt = nullptr; float* tgt_val = nullptr; float inv_t = 1.0f; };
// Inputs of EPI_SAMPLE.  stream / draw are device arrays indexed by the row of the product (row 0 of a GEMV), read by the kernel: nothing a
// captured launch would freeze.  count (GEMV only, optional): a device scalar added to draw[0] (GenCtl::count: the tokens of this turn).
struct SampleArgs {
    const int* stream = nullptr; const int* draw = nullptr; const int* count = nullptr;
    float inv_t = 1.0f; uint32_t seed_lo = 0, seed_hi = 0;
    float* part_raw = nullptr; float* part_max = nullptr;      // beside part_val / part_sum, same shape
};

struct RopeKvArgs;
// K / V^T pools of the ViT attention (layout of launch_vit_kv_pack): the fused tail of the SigLIP QKV product
struct VitPackArgs { void* Kpool; void* Vpool; int F, S, heads, head_dim; };
// C[M,N] = epi(A[M,K] . W[N,K]^T + bias[N]) + res[row % res_mod or row][N]      (all T, fp32 accumulate)
// K, lda, ldw multiples of one 16-byte chunk; EPI_SWIGLU: W rows are 32-row blocks
// [gate 32 | up 32] and C is [M, N/2] = silu(gate) * up.
struct GemmArgs {
    const void* A; int lda;
    const void* W; int ldw;
    void* C; int ldc;
    const void* bias;
    const void* res; int ldr; int res_mod;
    int M, N, K;
    int epi;
    float* ws; size_t ws_elems;   // split-K slab workspace (fp32) or null
    int nsplit, tile_base, launch_tiles;   // filled by the launcher (K splits; first column tile and tile count of this launch)
    int nt_w;                              // filled by the launcher: stage the weight tile with non-temporal loads (weights read once)
    int bn_fast;                           // filled by the launcher: consecutive workgroups walk the COLUMN tiles of one row tile (activations larger than weights)
    const void* zeros;            // >= 16 B of zeros in device memory: the K-tail source of the LDS-DMA staging (required)
    // optional fused RMSNorm of the finished output rows (o_proj -> post_attention_layernorm, down_proj -> next input_layernorm):
    // when the product takes the split-K path with N <= 4096 the slab reduce also writes norm_out = rmsnorm(C) * norm_w and
    // launch_gemm returns true; otherwise norm_out is untouched (false) and the caller runs launch_rmsnorm itself
    const void* norm_w; void* norm_out; float norm_eps;
    // optional fused tail of the QKV product of a prefill (Qwen2Attention: bias, RoPE on q / k, KV append): when the product takes the
    // split-K path the slab reduce also applies RoPE and appends k / v^T to the paged cache (rope->qkv must be C) and launch_gemm
    // returns true; otherwise C holds the plain product + bias and the caller runs launch_rope_kv itself
    const RopeKvArgs* rope;
    // optional fused tail of the SigLIP QKV product (siglip_encoder.py:197-232): when the product takes the split-K path the slab reduce
    // (sum + bias, rounded to T) also writes the K pages and the transposed V pages of the ViT attention -- splitk_epilogue followed by
    // vit_kv_pack in one pass -- and launch_gemm returns true; otherwise the caller runs launch_vit_kv_pack itself
    const VitPackArgs* vitpack;
    // optional with norm_out (bf16 engine, opt-in fp8 products): the fused reduce also writes the e4m3 copy of the normalised row and its
    // scale (max |y| / 448), exactly what launch_quant_fp8_rows produces from norm_out -- the A operand of the next product
    void* norm_q8 = nullptr; float* norm_q8_scale = nullptr;
    const void* norm_b;           // non-null: LayerNorm (mean/variance, weight norm_w, bias norm_b) instead of RMSNorm -- the ViT's ln1 / ln2
    // opt-in fp8 (OCP e4m3) operands (bf16 engine): when a_scale is set, A [M][K] and W [N][K] are e4m3 bytes (lda / ldw in
    // elements), C = a_scale[m] * w_scale[n] * (A . W^T) then the usual epilogue in bf16; K % 16 == 0
    const float* a_scale; const float* w_scale;
    // The arg-max forms (launch_gemm_argmax; epi = one of the eight of head_form; M <= 32 rows, 32x128 tiles, no K split: the lm_head of
    // several envs decoded together): no C; row m's (max, lowest index) over the 128 columns of tile t goes to part_val / part_idx
    // [m][tiles], reduced by launch_argmax_final_batched.  Optional repetition penalty as in GemvBatchArgs.  The arrays below are read
    // by the forms that carry the fact, ignored by the others.
    float* part_val = nullptr; int* part_idx = nullptr;
    const uint8_t* pen_flags = nullptr; const int* pen_rows = nullptr; float pen = 1.0f;
    float* part_sum = nullptr;    // lse / smp: [m][tiles] beside part_val
    SampleArgs smp;               // smp (smp.part_raw / part_max beside part_sum)
    TargetArgs tg;                // tgt (no penalty flags)
    float* cand_val = nullptr; int* cand_idx = nullptr;       // topk: [m][tiles][TOPK_C]
    float* part_ent = nullptr;    // ent: [m][tiles] beside part_sum
    VitPackArgs vp; int vp_on;    // filled by the launcher: device-side copy of *vitpack for the unsplit kernels that pack in their epilogue
    int force_cfg, force_split;   // tests: 0 = heuristic; force_cfg 129 -> 128x128 tiles with two in-workgroup K groups; force_cfg low bits 128 -> 128x128 tiles, 264 -> 256x64 tiles; force_split S -> 256x128 tiles, S splits
};
// true: a.norm_out was produced, or the K / V^T pages of a.vitpack were.  vit_packer (host, optional): the writer of those pages --
// 0 = none (the caller runs launch_vit_kv_pack), 1 = the split-K reduce (splitk_qkv_vitpack_kernel), 2 = the 128x128 tile epilogue
template <typename T> bool launch_gemm(hipStream_t s, const GemmArgs& a, int* vit_packer = nullptr);
template <typename T> int launch_gemm_argmax(hipStream_t s, GemmArgs a);    // the arg-max form a.epi names (M <= 32); throws on a form whose arrays are null; returns the partials per row

// y[N] = epi(W[N,K] . x'[K] + bias) + res,  x' = x or rmsnorm(x) * norm_w (fused prologue).
// EPI_SWIGLU as above (y has N/2 entries).  EPI_ARGMAX: no y; per-workgroup (max, lowest index)
// partials go to part_val/part_idx, reduced by launch_argmax_final.
struct GemvArgs {
    const void* W; int ldw;
    const void* x;
    const void* norm_w; float eps;
    const void* bias;
    const void* res;
    void* y;
    int N, K;
    int epi;
    float* part_val; int* part_idx;
    // optional fp8 (OCP e4m3) weight-only path (bf16 engine, opt-in): w8 [N][K] bytes, one fp32 scale per row,
    // W[n][k] ~= scale[n] * e4m3(w8[n][k]); when set, W is ignored
    const void* w8; const float* scale;
    // optional MXFP4 weight-only path (bf16 engine, opt-in): w4 [N][ldw / 2] bytes (two E2M1 codes per byte, element 2j in the low
    // nibble), e8 [N][ldw / 32] E8M0 scale bytes, W[n][k] = 2^(e8[n][k / 32] - 127) * e2m1(code); ldw in elements, a multiple of 32;
    // when set, W and w8 are ignored
    const void* w4 = nullptr; const uint8_t* e8 = nullptr;
    // optional lossless 12-bit packing of the bf16 weights (bf16 engine; svln_set_packed_decode, format in gemv.hip): wp [N][p12_row_bytes(K)]
    // packed blocks, prec [N][16] row records; W / ldw stay the bf16 original, which the blocks a record marks as fallback are read from.
    // K <= 32768.  The outputs are bit-equal to the call without wp.  Ignored when w4 or w8 is set.
    const void* wp = nullptr; const void* prec = nullptr;
    const int* skip;              // optional device flag: the launch is a no-op when *skip != 0 (generation finished: run-ahead decode steps)
    // EPI_ARGMAX only, optional: HF RepetitionPenaltyLogitsProcessor on the fp32 logits before the arg-max (a checkpoint's
    // generation_config.json `repetition_penalty`): pen_flags[n] != 0 marks token n as already generated in this turn;
    // its logit becomes v < 0 ? v * pen : v / pen.  null = no penalty.
    const uint8_t* pen_flags = nullptr; float pen = 1.0f;
    float* part_sum = nullptr;    // EPI_ARGMAX_LSE / EPI_SAMPLE: [gemv_grid(N)] beside part_val
    SampleArgs smp;               // EPI_SAMPLE only
    float* cand_val = nullptr; int* cand_idx = nullptr;       // EPI_*_TOPK: [gemv_grid(N)][TOPK_C]
    float* part_ent = nullptr;    // EPI_*_ENT: [gemv_grid(N)] beside part_sum
};
template <typename T> void launch_gemv(hipStream_t s, const GemvArgs& a);
// per-row e4m3 quantisation of a bf16 matrix [rows][cols] (cols % 16 == 0): scale[r] = max|W[r]| / 448
void launch_quant_fp8_rows(hipStream_t s, const void* w_bf16, int ld, void* w8, float* scale, int64_t rows, int cols);
// OCP MXFP4 quantisation of a bf16 matrix [rows][cols] (cols % 32 == 0): q4 [rows][cols / 2], e8 [rows][cols / 32] (see GemvArgs)
void launch_quant_mxfp4_rows(hipStream_t s, const void* w_bf16, int ld, void* q4, uint8_t* e8, int64_t rows, int cols);
// P12 (see GemvArgs::wp): bytes of one packed row; the encoder of a bf16 matrix [rows][cols] (row stride ld; cols % 8 == 0, cols <= 32768;
// *fb_count, optional, is incremented by the fallback blocks); and, TEST-ONLY, the decoder back to bf16 rows out [rows][ldo]
constexpr int P12_MAX_K = 32768;
__host__ __device__ constexpr size_t p12_row_bytes(int K) { return (size_t)((K + 511) / 512) * 768; }
void launch_p12_pack_rows(hipStream_t s, const void* w_bf16, int ld, void* packed, void* rec, unsigned* fb_count, int64_t rows, int cols);
void launch_p12_unpack_rows(hipStream_t s, const void* packed, const void* rec, const void* w_bf16, int ld, void* out, int ldo, int64_t rows, int cols);
template <typename T> void launch_gemv_timed(hipStream_t s, const GemvArgs& a, hipEvent_t start, hipEvent_t stop);   // events get the kernel's own begin/end
int gemv_grid(int N);                       // workgroups launch_gemv uses for N rows
constexpr int GEMV_ROWS_MAX_LDS = 160 * 1024 - 256;    // dynamic LDS the wave-per-rows kernel may ask for (K fp32 activations): N > 8192 or an epilogue
constexpr int GEMV_ROWS_TOPK_MAX_LDS = GEMV_ROWS_MAX_LDS - 256;   // the EPI_*_TOPK forms keep the four waves' lists (256 bytes) in static LDS

// B (1, 2, 4 or 8) activation vectors against one weight stream: x [B][ldx], y [B][ldy], res [B][ldr].
// EPI_ARGMAX: part_val / part_idx are [B][gemv_batched_grid(N, epi, B)]; launch_argmax_final_batched reduces them to B tokens.
struct GemvBatchArgs {
    const void* W; int ldw;
    const void* x; int ldx;
    const void* norm_w; float eps;
    const void* bias;
    const void* res; int ldr;
    void* y; int ldy;
    int N, K, epi, B;
    float* part_val; int* part_idx;
    // EPI_ARGMAX only, optional repetition penalty (see GemvArgs): row b of the batch uses the flag row pen_rows[b] of pen_flags [.][N]
    const uint8_t* pen_flags = nullptr; const int* pen_rows = nullptr; float pen = 1.0f;
    float* part_sum = nullptr;    // EPI_ARGMAX_LSE / EPI_SAMPLE: [B][grid] beside part_val
    SampleArgs smp;               // EPI_SAMPLE only (no fused norm: launch_gemv_batched throws)
    TargetArgs tg;                // EPI_TARGET only (no fused norm, no penalty flags: launch_gemv_batched throws)
    float* row_scale = nullptr;   // EPI_ARGMAX_LSE with norm_w only: [B], the norm's row factor (the arg-max ignores it, the sums are taken on the scaled logits)
    float* cand_val = nullptr; int* cand_idx = nullptr;       // EPI_*_TOPK (no fused norm: launch_gemv_batched throws): [B][grid][TOPK_C]
    float* part_ent = nullptr;    // EPI_*_ENT (no fused norm: launch_gemv_batched throws): [B][grid] beside part_sum
};
template <typename T> void launch_gemv_batched(hipStream_t s, const GemvBatchArgs& a);
int gemv_batched_grid(int N, int epi, int B);
// part_sum / scores (both or neither): the EPI_ARGMAX_LSE merge, scores[b] = log-probability of out_tokens[b] (NaN for token -1);
// row_scale (optional, [B]): GemvBatchArgs::row_scale of the producer
// part_raw / part_max (both or neither, with part_sum / scores): the EPI_SAMPLE merge instead (see there)
void launch_argmax_final_batched(hipStream_t s, const float* part_val, const int* part_idx, int n, int B, int* out_tokens,
                                 const float* part_sum = nullptr, float* scores = nullptr, const float* row_scale = nullptr,
                                 const float* part_raw = nullptr, const float* part_max = nullptr);
// the EPI_TARGET merge: row b's partials -> greedy_ids[b] (-1: no finite logit), greedy_logprobs[b] = -log S (the scored form's value)
// and logprobs[b] = (tgt_val[b] - V) - log S; a row with tgt[b] < 0 gets NaN and tgt_val[b] is not read
void launch_target_final_batched(hipStream_t s, const float* part_val, const int* part_idx, const float* part_sum, int n, int B, const int* tgt,
                                 const float* tgt_val, int* greedy_ids, float* greedy_logprobs, float* logprobs);
// B (1 .. 8) bf16 activation vectors against one MXFP4 weight stream on v_mfma_f32_16x16x32_bf16 (gemv_mx4b.hip; bf16 engine, opt-in):
// q4 / e8 / ldw as GemvArgs::w4 / e8 / ldw (the layout of the batch-1 GEMVs), x [B][ldx], y [B][ldy], res [B][ldr]; K, ldw multiples of 32,
// ldx a multiple of 8.  No fused RMSNorm.  EPI_SWIGLU as above.  EPI_ARGMAX: part_val / part_idx are [B][gemv_mx4b_grid(N, epi)], reduced
// by launch_argmax_final_batched; optional repetition penalty as in GemvBatchArgs.
struct GemvMx4BatchArgs {
    const void* q4; const uint8_t* e8; int ldw;
    const void* x; int ldx;
    const void* bias;
    const void* res; int ldr;
    void* y; int ldy;
    int N, K, epi, B;
    float* part_val; int* part_idx;
    const uint8_t* pen_flags = nullptr; const int* pen_rows = nullptr; float pen = 1.0f;
};
void launch_gemv_mx4b(hipStream_t s, const GemvMx4BatchArgs& a);
int gemv_mx4b_grid(int N, int epi);
// part_sum / scores (both or neither): the EPI_ARGMAX_LSE merge; the token's log-probability goes to scores[0]
void launch_argmax_final(hipStream_t s, const float* part_val, const int* part_idx, int n, int* out_token,
                         float* out_top /*[2]: best, runner-up of partial maxima (diagnostic)*/, const float* part_sum = nullptr,
                         float* scores = nullptr, const float* part_raw = nullptr, const float* part_max = nullptr);
// Device-side state of one greedy generation (GenerationMixin._sample: append the arg-max, stop on EOS or max_new_tokens), so that
// decode steps can be enqueued ahead of the host: every kernel of a step is a no-op once `done` is set.
struct GenCtl {
    int pos;        // position of the token the next decode step feeds (read by the attention kernel: RoPE, KV append)
    int kv_len;     // keys visible to that step (= pos + 1)
    int done;       // set by the arg-max step that emitted EOS / the max_new-th token / a non-finite arg-max (-1)
    int count;      // tokens emitted so far (out_ids[0 .. count))
    int max_new, n_eos;
    int draw0, stream;  // EPI_SAMPLE (svln_set_sampling): the env's draw counter at the start of the turn (token t draws draw0 + count) and its noise stream
};
// launch_argmax_final + the bookkeeping above: out_ids[count++] = token; done |= token in eos[0 .. n_eos) || count == max_new || token < 0;
// otherwise pos / kv_len advance by one.  No-op when ctl->done is already set.
// pen_flags (optional): the emitted token's byte is set (repetition penalty of the following steps)
// part_sum / scores (both or neither): the EPI_ARGMAX_LSE merge; scores[count] = the token's log-probability, written before count advances
// part_raw / part_max (both or neither, with part_sum / scores): the EPI_SAMPLE merge instead
void launch_argmax_step(hipStream_t s, const float* part_val, const int* part_idx, int n, int* out_token, float* out_top, GenCtl* ctl,
                        const int* eos, int* out_ids, uint8_t* pen_flags = nullptr, const float* part_sum = nullptr, float* scores = nullptr,
                        const float* part_raw = nullptr, const float* part_max = nullptr);
// Allowed-token lm_head (svln_set_allowed_tokens; gemv_subset.hip): the product over the n <= 256 listed rows ids[0] < ... < ids[n - 1] of
// W [V][ldw] for B <= 32 activation rows x [B][ldx], fp32 accumulate in an order that depends on K alone.  ONE arg-max partial per listed
// id, row stride n: part_val[b][j] = the processed value (after the penalty; z under EPI_SAMPLE), part_idx[b][j] = ids[j], or 0x7FFFFFFF
// (owns nothing) when the value is NaN or -inf, part_sum[b][j] = 1 (0 for -inf, NaN for NaN; EPI_ARGMAX_LSE / EPI_SAMPLE), and under
// EPI_SAMPLE smp.part_max = smp.part_raw = y.  launch_argmax_step / launch_argmax_final / launch_argmax_final_batched reduce them with
// n partials.  Penalty flags are indexed by the vocabulary id: pen_flags[(pen_rows ? pen_rows[b] : 0) * V + ids[j]].  EPI_SAMPLE: row b
// uses smp.stream[b], smp.draw[b] (+ *smp.count), and the noise column is the vocabulary id.
struct GemvSubsetArgs {
    const int* ids = nullptr; int n = 0;          // device list
    const void* W = nullptr; int ldw = 0;
    const void* x = nullptr; int ldx = 0;
    int V = 0, K = 0, B = 0, epi = EPI_ARGMAX;    // EPI_ARGMAX, EPI_ARGMAX_LSE, EPI_SAMPLE or EPI_TARGET (the LSE partials on y = v * tg_inv_t: a forced turn under sampling)
    float tg_inv_t = 1.0f;
    float* part_val = nullptr; int* part_idx = nullptr; float* part_sum = nullptr;
    const uint8_t* pen_flags = nullptr; const int* pen_rows = nullptr; float pen = 1.0f;
    SampleArgs smp;
    const int* skip = nullptr;                    // optional device flag: no-op when *skip != 0
};
template <typename T> void launch_gemv_subset(hipStream_t s, const GemvSubsetArgs& a);
// out[row][j] = y_j - logsumexp_i y_i for the B partial rows src [B][n] (part_val under greedy decoding, part_max under sampling);
// row = *row_dev when given (B = 1: GenCtl::count, launched before the step kernel advances it), else b.  out rows have stride n.
void launch_subset_logprobs(hipStream_t s, const float* src, int n, int B, float* out, const int* row_dev = nullptr, const int* skip = nullptr);
// svln_top_logprobs (misc.hip): the k <= TOPK_C best of the n_part x c candidates (cand_val, cand_idx) [B][n_part][c] of every row -- c =
// TOPK_C from the EPI_*_TOPK epilogues, c = 1 for the subset product, whose partials are candidates as they stand (part_val, or part_max
// under sampling, with part_idx) -- y descending then column ascending; entries that are NaN, -inf or own nothing (0x7FFFFFFF) are never
// listed.  (V, S) of the row come from the device functions the scored final kernels use, on the same partials: part_max == nullptr is
// the greedy merge on (part_val, part_idx, part_sum), else the sampled one on (part_max, part_sum).  top_ids[row][k] (-1: padding) and
// top_logprobs[row][k] = (y - V) - log S (-inf: padding); row = *row_dev when given (B = 1: GenCtl::count, launched before the step kernel
// advances it), else b.  Under greedy decoding entry 0 is the token's score bit for bit; under sampling the emitted id's entry is.
void launch_topk_merge(hipStream_t s, const float* cand_val, const int* cand_idx, int n_part, int c, int B, int k, const float* part_val,
                       const int* part_idx, const float* part_sum, const float* part_max, int* top_ids, float* top_logprobs,
                       const int* row_dev = nullptr, const int* skip = nullptr);
// svln_token_entropy (misc.hip): the entropy of every row's distribution from its n_part partials [B][n_part]: (V, S) through the device
// functions the scored final kernels use, on the same partials -- part_max == nullptr is the greedy merge on (part_val, part_idx,
// part_sum), else the sampled one on (part_max, part_sum) -- T = sum_k ent_rescale(part_ent[k], part_sum[k], m_k, V) on the same fixed
// tree, out[row] = log S - T / S in nats (NaN for a row without a finite value).  part_ent == nullptr: every t_k is 0 (the subset product:
// one id per partial).  row = *row_dev when given (B = 1: GenCtl::count, launched before the step kernel advances it), else b.
void launch_entropy_merge(hipStream_t s, const float* part_val, const int* part_idx, const float* part_sum, const float* part_max,
                          const float* part_ent, int n_part, int B, float* out, const int* row_dev = nullptr, const int* skip = nullptr);
// svln_sampling_truncation (misc.hip): top-k then top-p over one row's candidates, as an 8-entry partial row the sampled final kernels
// (launch_argmax_step / launch_argmax_final / launch_argmax_final_batched with n = TOPK_C) reduce unchanged.  Candidates as in
// launch_topk_merge ([B][n_part][c], c = TOPK_C or 1; n_part x c <= 16384).  Rule per row, one 256-thread workgroup each:
//   1. the k' = min(top_k, listable candidates) winners of launch_topk_merge's rounds, (y_j, col_j), y descending then column ascending;
//   2. e_j = lse_exp(y_j - y_0), c_j = c_{j-1} + e_j serially in fp32, total = c_{k'-1}; entry 0 is kept, entry j >= 1 iff
//      top_p >= 1 or c_{j-1} < fl(top_p * total) -- a prefix of the list (HF's TopPLogitsWarper over the top-k set: temperature, top-k,
//      top-p).  At an exact tie on the k-th value HF's TopKLogitsWarper keeps every tied column; this rule keeps exactly k, lowest columns;
//   3. a kept entry becomes the partial (part_val = fl(y_j + G(seed, stream[b], draw[b] + *count, col_j)), part_idx = col_j, part_raw =
//      part_max = y_j, part_sum = 1): the noise and the sum of the untruncated epilogues, so whenever the untruncated sampled token is
//      kept the truncated turn emits it; every other entry of the eight is the owns-nothing partial (-inf, 0x7FFFFFFF, 0, -inf, 0).
// The final kernel's score is then the log-softmax over the kept set at the emitted id; a row with nothing listable gives token -1.
// smp: stream / draw / count / seed as the producer's; smp.part_raw / smp.part_max are the OUTPUT rows [B][TOPK_C] beside tr_val / tr_idx /
// tr_sum (never the producer's partial arrays: launch_topk_merge and the tests still read those); smp.inv_t is not used (y is scaled).
void launch_truncate_partials(hipStream_t s, const float* cand_val, const int* cand_idx, int n_part, int c, int B, int top_k, float top_p,
                              const SampleArgs& smp, float* tr_val, int* tr_idx, float* tr_sum, const int* skip = nullptr);
// TEST-ONLY: out[k] = gumbel_noise(seed, stream, draw, n0 + k) for k < count
void launch_gumbel(hipStream_t s, uint32_t seed_lo, uint32_t seed_hi, int stream, int draw, int n0, int count, float* out);
// Draft-verified greedy decode (svln_set_speculative; misc.hip).  launch_verify_feed builds the rows of the next verify pass from GenCtl,
// the last token and the device copy of the draft: fed[0 .. rows) and vctl[1] = rows used (vctl[0] = usable draft length, set by the
// host).  launch_verify_step applies the verify rule to the rows' arg-maxes `cand`: appends the accepted tokens to out_ids, advances
// GenCtl as that many launch_argmax_step calls would, sets *out_token, copies the final-norm rows xn[i] of the emitted tokens to
// hid_tap[min(token index, tap_cap - 1)] and adds to stats[0] (passes run) / stats[1] (tokens emitted).  Both are no-ops once done is set.
void launch_verify_feed(hipStream_t s, const GenCtl* ctl, const int* token, const int* draft, int* vctl, int* fed, int rows, int max_positions);
template <typename T> void launch_verify_step(hipStream_t s, const int* fed, const int* cand, const int* n_rows, int max_rows, GenCtl* ctl,
                                              const int* eos, int* out_ids, int* out_token, const void* xn, void* hid_tap, int H, int tap_cap,
                                              int* stats);
// Several drafts of one turn verified by one prefill pass (svln_generate_drafts; misc.hip).  cand [1 + sum k_g]: the arg-maxes of the head
// rows -- row 0 = the prompt's last row, then the rows draft g fed, sequence by sequence; cand_score: their log-probabilities (null: not
// scored); fed [G][r]: the ids the row slots were fed (the folded candidates call's layout); k [G]: rows draft g fed (clamped to 0 .. r).
// The verify rule of launch_verify_step runs for every g on [row 0, rows of g]; the largest emitted count wins, a tie goes to the lowest
// g.  The winner's tokens go to out_ids / *out_token / GenCtl as launch_verify_step leaves them, the final-norm rows xn[row] of its
// emitted tokens to hid_tap[min(token index, tap_cap - 1)], scores[index] when scored; rec = {winner, emitted, stop, head rows read},
// stats[0] += 1, stats[1] += emitted.  No-op once done is set.  G <= 8, 1 + G r <= DRAFT_SELECT_ROWS.
constexpr int DRAFT_SELECT_ROWS = 33;
struct DraftSelectArgs {
    const int* cand; const float* cand_score; const int* fed; const int* k; int G, r;
    GenCtl* ctl; const int* eos; int* out_ids; int* out_token; const void* xn; void* hid_tap; int H, tap_cap; float* scores; int* rec; int* stats;
};
template <typename T> void launch_draft_select(hipStream_t s, const DraftSelectArgs& a);
// flags[ids[k]] = value for k < *count (count: device scalar) or k < n_host when count is null; ids < 0 are skipped
void launch_set_flags(hipStream_t s, uint8_t* flags, const int* ids, const int* count, int n_host, int value);

// Flash-style attention over paged K / V^T tiles (64 keys per page).
//   pools:  K  [page][n_kv_total][64][HDP]        HDP = head dim padded to an even chunk count
//           Vt [page][n_kv_total][DT*32][64]      DT = ceil(HD/32); transposed so keys are contiguous
//   rows of one "kv head" kh: rho = i*G + g  (query position i, q-head g of the group)
//   Q/O element (frame, i, head, d) at  ((frame*T + i) * stride) + head*HD + d, head = (kh % hpf)*G + g
// one environment of a batched decode step
struct DecodeSlot { const int* page_table; int pos; int pad; };

constexpr int ATTN_PART_PAD = 4;    // floats after the HD partial outputs of a row: m, l, 2 unused
struct AttnArgs {
    const void* Q; int q_stride;
    void* O; int o_stride;
    const void* Kpool; const void* Vpool;
    const int* page_table;        // device [tiles]; null = identity
    int n_kv_total, hpf, G, T;
    int P;                        // absolute position of query 0 (causal mask: key <= P + i)
    int kv_len;
    const int* dyn_kv_len;        // device scalar overriding kv_len (P = kv_len - T); for hipGraph replay
    float scale;
    int causal;
    int nsplit, tiles_per_split;  // split-KV: gridDim.z = nsplit, partials in `part`
    float* part;                  // [nsplit][n_kv_total][rows_pad][HD + ATTN_PART_PAD] fp32 (O unnormalised, m, l, 2 pad: rows stay 16-byte aligned)
    int rows_pad;
    // decode fusion (T == 1, head_dim 128, one wave per workgroup): Q points at the UN-roped qkv row
    // [(nq + 2 nkv) * 128]; the kernel applies RoPE to q in registers, and the workgroup that owns the page of
    // position *dyn_pos ropes k, appends k / v to the pools (global) and patches its LDS tiles.
    int fuse_rope_append;
    const float* rope_tab;        // [max_positions][128]: cos[64] | sin[64]
    const int* dyn_pos;
    int nq_heads;
    // batched decode (gridDim.z = environments): per-env page table / position; Q, O and the partials advance by
    // q_stride, o_stride and part_bstride per environment
    const DecodeSlot* slots;
    size_t part_bstride;
    int batch;
    const int* skip;              // optional device flag: decode attention / combine are no-ops when *skip != 0
    int key_groups;               // > 1: split-KV inside the workgroup (64 query rows x key groups, merged through LDS); nsplit > 1 on top: the merge writes the split's partial row
    const int* dyn_rows;          // verify pass only (launch_attention_verify): device scalar, query positions of this pass (<= T)
};
template <typename T> void launch_attention(hipStream_t s, const AttnArgs& a, int head_dim, int waves);
// Draft-verify pass of ONE env (svln_set_speculative): min(*dyn_rows, T) query positions from *dyn_pos on, Q = their un-roped q|k|v rows
// [T][q_stride]; RoPE at each row's own position, K / V^T append of every row, per-row causal mask, decode split-KV partials + merge
// -> O [T][o_stride].  T * G <= 32; a no-op when *skip != 0 or *dyn_rows <= 0.  The caller owns the pages of every position written.
template <typename T> void launch_attention_verify(hipStream_t s, const AttnArgs& a);
// the same for a.batch <= 8 sequences at once: a.slots[s] = {page table, start position, pad = rows of the sequence (0 .. a.T)}, its q|k|v /
// output rows [s * a.T, (s + 1) * a.T), its partials at a.part + s * a.part_bstride; per sequence bit for bit launch_attention_verify
template <typename T> void launch_attention_verify_multi(hipStream_t s, const AttnArgs& a);
template <typename T> void launch_attention_combine(hipStream_t s, const AttnArgs& a, int head_dim);
template <typename T> int attn_key_groups(int head_dim);       // the key-group count launch_attention<T> is built for at this head dim (AttnArgs::key_groups)

// Persistent batch-1 decode layer (decode_layer.hip): merge of this layer's split-KV attention partials, o_proj + residual,
// post_attention_layernorm, gate/up + SwiGLU, down_proj + residual, and the NEXT layer's input_layernorm + q|k|v projection, as ONE launch
// of one workgroup per CU (LDS-DMA loader ring + consumer waves, data-tagged granule all-gathers between the products).
struct DecodeLayerArgs {
    const float* part; int nsplit, tiles_per_split; const int* dyn_kv_len; int n_kv, Gq;      // attn_decode_kernel's partials [split][n_kv][32][132]
    const void *o_w, *post_norm, *gu_w, *down_w;                                            // this layer (engine dtype, packed as the engine holds them)
    const void *next_norm, *next_qkv_w, *next_qkv_b;                                        // next layer's input_layernorm / q|k|v; null for the last layer
    void* x;                      // residual stream [H]: read at the start, rewritten with the layer's output
    void* qkv_out;                // [qkv_dim]: the next layer's q | k | v rows (bias added, un-roped)
    int H, I, qd, qkv_dim; float eps;
    unsigned long long* gran[4];  // granule buffers of the four all-gather edges (qd, H, I, H values)
    unsigned* seq;                // launch counter (device): the epoch of the launch's granule tags
    unsigned* giveup;             // != 0: a bounded spin timed out (code); results are invalid
    const int* skip;              // optional device flag: no-op when *skip != 0 (run-ahead steps past the end of the generation)
    unsigned long long* dbg;      // optional [workgroups][16] phase stamps (100 MHz clock): svln_probe_decode_layer
};
template <typename T> bool decode_layer_supported(const DecodeLayerArgs& a, int cus);
template <typename T> void launch_decode_layer(hipStream_t s, const DecodeLayerArgs& a, int cus, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
void decode_layer_init_attrs();
// Host only (svln_decode_layer_walk): the slot sequence of one wave and lane through one op, as `prefetch` + `product` order it.
struct DecodeLayerWalkOp { int elem_size, K, nrows, pair, first; };
struct DecodeLayerWalkSlot { int64_t load_off; int32_t valid, row, pb, row_done; };      // = svln_decode_layer_slot
// Returns the slot count ns (out[0 .. ns) filled, refill[0 .. PF) = offsets in `next` loaded by the last group); -ns if ns > max_slots.
int decode_layer_walk(const DecodeLayerWalkOp& op, const DecodeLayerWalkOp& next, int wave, int lane, DecodeLayerWalkSlot* out, int max_slots,
                      int64_t* refill);

// RMSNorm / LayerNorm over rows of length n (T in, T out).
// y2 / y2_row / y2_cap: optional second copy of the rows at row *y2_row (device scalar) of y2, clamped to y2_cap rows
template <typename T> void launch_rmsnorm(hipStream_t s, const void* x, const void* g, void* y, int rows, int n, float eps, const int* skip = nullptr,
                                          void* y2 = nullptr, const int* y2_row = nullptr, int y2_cap = 0);
// indexed form: y[r] = rmsnorm(x[src_rows[r]]) * g for r < rows, bit-equal to launch_rmsnorm on that row; the row also goes to
// tap[tap_rows[r]] unless tap_rows[r] < 0.  src_rows / tap_rows: device arrays of `rows` ints.
template <typename T> void launch_rmsnorm_indexed(hipStream_t s, const void* x, const void* g, void* y, const int* src_rows, const int* tap_rows,
                                                  void* tap, int rows, int n, float eps);
template <typename T> void launch_layernorm(hipStream_t s, const void* x, const void* g, const void* b, void* y, int rows, int n, float eps);

// RoPE on q,k (in place on q) + append roped k and v to the paged cache.
// qkv: [T][(nq + 2 nkv) * 128]; positions P + i (P = *dyn_pos if given).
struct RopeKvArgs {
    void* qkv; int ld;
    void* Kpool; void* Vpool;
    const int* page_table;
    const float* rope_tab;        // [max_positions][128]: cos[64] | sin[64]  (launch_rope_table)
    int T, nq, nkv, P;
    const int* dyn_pos;
    // mirror form (n_mirror > 0; the folded candidates call): a k / v row whose position lies in LOGICAL page mirror_page is also stored,
    // same values and in-page offsets, to the n_mirror <= ROPE_MIRROR_MAX PHYSICAL pages mirror_dst lists (a device array), in every kv
    // head.  n_mirror == 0 launches the plain instantiation, which reads none of the three.
    int mirror_page = 0;
    const int* mirror_dst = nullptr;
    int n_mirror = 0;
};
constexpr int ROPE_MIRROR_MAX = 7;
template <typename T> void launch_rope_kv(hipStream_t s, const RopeKvArgs& a);
void launch_rope_table(hipStream_t s, float* tab, const float* inv_freq, int positions);
// out[2f], out[2f+1] += 128-bit content key of frame f (caller zeroes `out` first)
void launch_frame_hash(hipStream_t s, const float* pix, int F, size_t words_per_frame, unsigned long long* out);

// ViT: qkv [F*S][3*Hv] -> K pages [page][F*heads][64][HDP], Vt pages [page][F*heads][96][64]
template <typename T> void launch_vit_kv_pack(hipStream_t s, const void* qkv, int ld, void* Kpool, void* Vpool, int F, int S,
                                             int heads, int head_dim);

// pixels [F,3,S,S] (fp32) -> patches [F*side*side][kp] (T), k = c*p*p + ky*p + kx, zero padded to kp
template <typename T> void launch_patchify(hipStream_t s, const float* pix, void* out, int F, int image, int patch, int kp);

// bilinear 2-D pooling of token grids: in [F][side*side][C] -> out [F][out*out][C]
// taps: device int2/float2 tables [out] (i0,i1) and (w0,w1), shared by both axes.
template <typename T> void launch_pool(hipStream_t s, const void* in, void* out, const int* tap_idx, const float* tap_w, int F,
                                       int side, int out_side, int C);

// out[r][:] = src[r] >= 0 ? embed[src[r]][:] : feats[-(src[r]+1)][:]
// opt-in slow-memory pruning (misc.hip): sel[0..keep) = ascending indices of the `keep` rows of m [n_rows][H] least similar (cosine) to the mean row
template <typename T> void launch_memory_prune(hipStream_t s, const void* m, int n_rows, int H, int keep, float* partial, float* mean, float* score,
                                               int* sel);
template <typename T> void launch_gather_rows(hipStream_t s, const int* src, const void* embed, const void* feats, void* out,
                                              int rows, int n, const int* skip = nullptr);
// ragged form: out[list[2 i]][:] = embed[list[2 i + 1]][:] for i < rows (list: device array of (destination row, token id) pairs)
template <typename T> void launch_gather_rows_ragged(hipStream_t s, const int* list, const void* embed, void* out, int rows, int n);

// Fork of a KV page (svln_generate_group; kv_fork.hip): in each of the n_pools pools of `pools` (device table of pool bases: every layer's
// K pool and V^T pool) page src_page is copied to the n_dst pages of the device list dst_pages, in 16-byte chunks, each chunk loaded once
// and stored n_dst times.  page_elems = elements of T per page of one pool.  The caller guarantees: every page inside the pools, the
// destinations distinct and different from the source.
template <typename T> void launch_kv_page_copy(hipStream_t s, void* const* pools, int n_pools, int src_page, const int* dst_pages, int n_dst,
                                               int64_t page_elems);

// Hand-over of KV pages between the hypotheses of a beam turn (kv_fork.hip): kv_page_copy with one source per destination.  In each of the
// n_pools pools, page src_pages[i] is copied to page dst_pages[i] for i < n (device lists), in 16-byte chunks, all pairs in one launch.
// The caller guarantees: every page inside the pools, the destinations distinct, no page both a source and a destination (so the order
// of the pairs does not matter and nothing is permuted in place).  One source may serve several destinations.
template <typename T> void launch_kv_page_gather(hipStream_t s, void* const* pools, int n_pools, const int* src_pages, const int* dst_pages, int n,
                                                 int64_t page_elems);

// One select step of a beam turn (misc.hip, beam_select_kernel; one workgroup).  The hypothesis set lives in device memory: a BeamHdr and
// the rows ids / lps [BEAM_MAX_W][len_cap]; rank = index.  `in` is the set before the step, `out` the set after it (two different
// states: children copy their parents' rows).  list_ids / list_lps [rank][W]: the lm_head list of every live hypothesis (the layout of
// the batched heads' top-k lists at k = W; rows of finished ranks are not read; -1 = no entry).  Rule:
//   pool    = every finished hypothesis (item (r, 0), score unchanged) + every (r, j) of a live one with id >= 0, score fl(score_r + lp_rj)
//   new set = the best W of the pool by score descending, then r, then j ascending; finished = id in eos[0 .. n_eos) or length == limit
//   tok_b   : row k < B of the next step feeds the last id of rank k if it is live, else of the first live rank (untouched: none live)
//   pages   : rank c in order keeps its parent's page set if no earlier rank took it, else takes the lowest of the 16 sets that neither
//             the old set holds nor an earlier rank took and lists (src, dst) for the first n_cp pages of the two sets
//             (set_pages[set * set_stride + i]) in pair_src / pair_dst (room for BEAM_MAX_W * n_cp pairs)
//   rec     : int [BEAM_REC]: n_new, n_live, live hypotheses before, pairs, then parent rank [8], chosen entry [8], page set [8] (-1 unused)
// The caller guarantees: in->n <= 8, every length <= len_cap and < limit for a live hypothesis, limit <= len_cap, in->set_of distinct
// values of 0 .. 15.
constexpr int BEAM_MAX_W = 8, BEAM_CP_MAX = 8, BEAM_REC = 4 + 3 * BEAM_MAX_W;
struct BeamHdr { int n; int len[BEAM_MAX_W]; int fin[BEAM_MAX_W]; int set_of[BEAM_MAX_W]; float score[BEAM_MAX_W]; };
struct BeamSelectArgs {
    const int* list_ids = nullptr; const float* list_lps = nullptr;
    const BeamHdr* in = nullptr; const int* in_ids = nullptr; const float* in_lps = nullptr;
    BeamHdr* out = nullptr; int* out_ids = nullptr; float* out_lps = nullptr;
    int len_cap = 0, W = 0, limit = 0, n_eos = 0, B = 0, n_cp = 0, set_stride = 0;
    const int* eos = nullptr; const int* set_pages = nullptr;
    int *tok_b = nullptr, *pair_src = nullptr, *pair_dst = nullptr, *rec = nullptr;
};
void launch_beam_select(hipStream_t s, const BeamSelectArgs& a);

// weights: synthesize (see weights.py) or convert canonical rows into packed rows
// dst row = (r / blk) * blk * nint + phase * blk + r % blk ; cols copied to [0, cols), dst_ld >= cols
struct RowMap { int blk, nint, phase; };
template <typename T> void launch_synth(hipStream_t s, void* dst, int dst_ld, int64_t rows, int cols, RowMap m, uint64_t seed_t,
                                        float half_width, float base);
template <typename T> void launch_convert(hipStream_t s, void* dst, int dst_ld, int64_t rows, int cols, RowMap m, const void* src,
                                          int src_is_f32);
template <typename T> void launch_to_f32(hipStream_t s, const void* src, float* dst, int64_t n);
template <typename T> void launch_from_f32(hipStream_t s, const float* src, void* dst, int64_t n);

// a-1 on the GPU (preprocess.hip): Pillow's two-pass fixed-point bicubic resize + rescale / normalise, bit-exact.
// ResampleAxis = the host-built coefficient table of one axis (precompute_coeffs + normalize_coeffs_8bpc of Pillow's Resample.c):
// for output index i, source taps xmin[i] .. xmin[i]+cnt[i]-1 with 22-bit fixed-point weights k[i*ksize ..].
struct ResampleAxis { int ksize = 0; std::vector<int> xmin, cnt, k; };
struct ResampleDev { const int *hmin, *hcnt, *hk, *vmin, *vcnt, *vk; int ks_h, ks_v; };   // device copies (h = along the width, v = along the height)
void build_resample_table(int in_size, int out_size, ResampleAxis& ax);
void build_normalize_lut(float* lut256, float mean, float std);
size_t preprocess_lds_bytes(int W, int S, int ks_v, int ks_h);
// rgb uint8 [n][H][W][3] (device, readable up to 16 bytes past its end) -> out fp32 [n][3][S][S]
void launch_preprocess(hipStream_t s, const uint8_t* rgb, float* out, int n_frames, int H, int W, int S, const ResampleDev& t, const float* lut);
void launch_upload(hipStream_t s, const void* src_dev_visible, void* dst, size_t bytes);    // 16-byte granules; src may be pinned host memory
void preprocess_init_attrs();

// raise the dynamic-LDS limit of the kernels that may ask for more than 64 KiB (call once, outside capture).  A refused attribute would
// only show up later as a failed launch of that one kernel: the first refusal is kept and returned by init_kernel_attributes().
inline hipError_t& attr_status() { static hipError_t e = hipSuccess; return e; }
// threads > 0: also check, on the host, that the code object accepts a block of that size (its max flat workgroup size comes from
// __launch_bounds__): a launch above it -- or above the dynamic-LDS attribute -- is not reported by hipLaunchKernel; the packet
// processor rejects the packet and the runtime aborts the process from its queue-error callback, with no message at the default log
// level (the round-2 test_gemm abort).
inline void set_max_lds(const void* fn, int bytes, int threads = 0) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && threads > 0) {
        hipFuncAttributes at;
        e = hipFuncGetAttributes(&at, fn);
        if (e == hipSuccess && (at.maxThreadsPerBlock < threads || bytes > 160 * 1024)) e = hipErrorInvalidConfiguration;
    }
    if (e != hipSuccess && attr_status() == hipSuccess) attr_status() = e;
}
void gemm_init_attrs();
void gemv_init_attrs();
void attention_init_attrs();
inline hipError_t init_kernel_attributes() {
    attr_status() = hipSuccess;
    gemm_init_attrs(); gemv_init_attrs(); attention_init_attrs(); preprocess_init_attrs(); decode_layer_init_attrs();
    return attr_status();
}

}  // namespace svln
