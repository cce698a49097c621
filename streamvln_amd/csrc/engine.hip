// StreamVLN streaming-inference engine: weights, workspaces, paged KV cache, per-env session state,
// the vision / prefill / decode schedules, and the C ABI of include/streamvln_hip.h.
//
// Replaces (reference file:line under /root/reference):
//   encode_rgbd + vision tower + projector + get_2dPool   streamvln/model/stream_video_vln.py:53-142
//   prepare_inputs_labels_for_multimodal (splice)         stream_video_vln.py:144-291
//   generate / prepare_inputs_for_generation / reset*     stream_video_vln.py:353-479
//   Qwen2 decoder stack + DynamicCache + greedy _sample   transformers 4.45.1 (requirements.txt:140)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/streamvln_hip.h"
#include "common.h"
#include "gemm_plan.h"
#include "modes.h"
#include "kernels.h"

namespace svln {

static thread_local std::string g_err;

#define HIP_CHECK(x)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess)                                                                          \
            throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
    } while (0)
#define REQUIRE(c, msg)                                          \
    do {                                                         \
        if (!(c)) throw std::runtime_error(std::string(msg));    \
    } while (0)

// The engine's buffers, stream and launches belong to ONE device; every API call runs with that device current and restores the
// caller's (torch's) current device on the way out.
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) HIP_CHECK(hipSetDevice(dev));
    }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};
// launches are asynchronous: a bad configuration (LDS size, grid) only shows up in hipGetLastError
#define LAUNCH_CHECK(what)                                                                              \
    do {                                                                                               \
        hipError_t e_ = hipGetLastError();                                                             \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(what) + ": kernel launch failed: " + hipGetErrorString(e_)); \
    } while (0)

constexpr int IMAGE_TOKEN = -200, MEMORY_TOKEN = -300;   // streamvln/utils/utils.py:9,15
constexpr int PAGE = 64;                                 // keys per KV page
constexpr int HID_TAP_ROWS = 64;
constexpr int PREFILL_SPLIT_ROWS = 2048;                 // split-KV prefill only when T * G fits this many rows

struct Slot {            // canonical tensor -> where its rows live in the packed device layout
    void* dst; int ld; int64_t rows; int cols; RowMap map; bool filled;
    bool vision;         // a tensor of the vision tower or the projector: the cached frame features depend on it
};

// the sampled form of a test-only lm_head op (svln_op_*_argmax_sample): streams / draws are host arrays, one entry per row of the product
struct OpSample { float temperature; uint64_t seed; const int32_t* streams; const int32_t* draws; };
// the outputs of the batched test entries under svln_top_logprobs (null: the scored / sampled entries): k, candidates [rows][n][8], lists [rows][k]
struct OpTopkRows { int k; float* cv; int32_t* ci; int32_t* top_ids; float* top_lp; int32_t* n_part; };
// the outputs of the test entries under svln_token_entropy (null: the scored / sampled entries): the entropies [rows], every partial array
// [rows][n] (pr / pm: the sampled form only) and n
struct OpEntOut { float* ent; float* pv; int32_t* pi; float *ps, *pr, *pm, *pe; int32_t* n_part; };
struct EngineBase {
    virtual ~EngineBase() {}
    virtual void synth_tensor(const char* name, uint64_t seed_t, float hw, float base) = 0;
    virtual void set_tensor(const char* name, const void* data, int dtype, int64_t numel, int on_device) = 0;
    virtual int weights_missing() = 0;
    virtual void get_tensor_f32(const char* name, float* out, int64_t numel) = 0;
    virtual void reset_env(int env) = 0;
    virtual void kv_reset(int env) = 0;
    virtual void env_state(int env, int32_t* n_embeds, int32_t* kv_len) = 0;
    virtual int kv_free_pages() = 0;
    virtual void encode_frames(const float* pixels, int F, int on_device) = 0;
    virtual void preprocess_frames(const uint8_t* rgb, int n, int height, int width, int on_device, float* out_dev, bool wait) = 0;
    virtual void* stream_handle() = 0;
    virtual void frame_ring(int slots, int height, int width, uint8_t** base, int64_t* stride) = 0;
    virtual void frame_ring_wait(int slot) = 0;
    virtual void turn(const svln_turn_args& a, int64_t* out, int cap, int32_t* n_out, int32_t* kv_len) = 0;
    virtual void preprocess_time(double* ms, int64_t* frames, int reset) = 0;
    virtual int device_id() const = 0;
    virtual void append_turn(int env, const int64_t* ids, int n, int frame_base, int n_memory) = 0;
    virtual void generate(int env, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out, bool fixed) = 0;
    virtual void generate_batch(const int32_t* envs, int n_envs, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out) = 0;
    virtual int batch_submit(int env, int max_new, const int64_t* eos, int n_eos) = 0;
    virtual int batch_step(int32_t* finished_slots, int32_t* n_finished) = 0;
    virtual void batch_result(int slot, int32_t* env, int64_t* out, int cap, int32_t* n_out) = 0;
    virtual void batch_cancel(int slot) = 0;
    virtual void set_turn_row_limit(int rows) = 0;
    virtual void set_repetition_penalty(float penalty) = 0;
    virtual void get_hidden_batch(int slot, float* out, int max_rows, int32_t* n_rows) = 0;
    virtual void get_hidden(float* out, int max_rows, int32_t* n_rows) = 0;
    virtual void set_layer_taps(int enable, int probe_layer) = 0;
    virtual void get_layer_taps(float* out) = 0;
    virtual void get_layer_probe(int which, float* out, int64_t max_elems, int32_t* n_rows, int32_t* n_cols) = 0;
    virtual void get_embeds(int env, int start, int n, float* out) = 0;
    virtual void get_feats(int start, int n, float* out) = 0;
    virtual void get_top2(float* out) = 0;
    virtual void set_token_scores(int enable) = 0;
    virtual void top_logprobs(int k) = 0;
    virtual void get_topk(int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) = 0;
    virtual void batch_topk(int slot, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) = 0;
    virtual void generate_batch_topk(int index, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) = 0;
    virtual void op_gemv_topk(GemvArgs a, int k, const OpSample* smp, int32_t* host_token, float* host_logprob, float* pv, int32_t* pi, float* ps,
                              float* pr, float* pm, float* cv, int32_t* ci, int32_t* top_ids, float* top_lp, int32_t* n_part) = 0;
    virtual void get_token_scores(float* out, int cap, int32_t* n) = 0;
    virtual void batch_scores(int slot, float* out, int cap, int32_t* n) = 0;
    virtual void generate_batch_scores(int index, float* out, int cap, int32_t* n) = 0;
    virtual void op_gemv_scores(GemvArgs a, int32_t* host_token, float* host_logprob, const OpSample* smp, const OpEntOut* en = nullptr) = 0;
    virtual void op_gemv_batched_scores(GemvBatchArgs a, int32_t* host_tokens, float* host_logprobs, const OpSample* smp, const OpTopkRows* tk = nullptr,
                                        const OpEntOut* en = nullptr) = 0;
    virtual void op_gemm_argmax_scores(GemmArgs a, int32_t* host_tokens, float* host_logprobs, const OpSample* smp, const OpTopkRows* tk = nullptr,
                                       const OpEntOut* en = nullptr) = 0;
    virtual void token_entropy(int enable) = 0;
    virtual void get_token_entropy(float* out, int cap, int32_t* n) = 0;
    virtual void batch_entropy(int slot, float* out, int cap, int32_t* n) = 0;
    virtual void generate_batch_entropy(int index, float* out, int cap, int32_t* n) = 0;
    virtual void op_entropy_merge(const float* pv, const int32_t* pi, const float* ps, const float* pm, const float* pe, int B, int n_part, float* out) = 0;
    virtual void set_sampling(int enable, float temperature, uint64_t seed) = 0;
    virtual void sampling_truncation(int top_k, float top_p) = 0;
    virtual void op_truncate(const float* cv, const int32_t* ci, int B, int n_part, int cc, const OpSample* q, int top_k, float top_p, float* pv,
                             int32_t* pi, float* pr, float* pm, float* ps, int32_t* host_tokens, float* host_logprobs) = 0;
    virtual void set_allowed_tokens(const int64_t* ids, int n) = 0;
    virtual void get_allowed_logprobs(float* out, int cap, int32_t* n_tokens, int32_t* n_ids) = 0;
    virtual void batch_allowed_logprobs(int slot, float* out, int cap, int32_t* n_tokens, int32_t* n_ids) = 0;
    virtual void generate_batch_allowed_logprobs(int index, float* out, int cap, int32_t* n_tokens, int32_t* n_ids) = 0;
    virtual void op_subset_argmax(GemvSubsetArgs a, const int64_t* ids, const OpSample& smp, int32_t* host_tokens, float* host_logprobs, float* host_y,
                                  float* host_dist) = 0;
    virtual void op_gumbel(uint64_t seed, int stream, int draw, int n0, int count, float* out) = 0;
    virtual void generate_group(int env, int n_seq, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out) = 0;
    virtual void turn_group(const svln_turn_args& a, int n_seq, int64_t* out, int cap, int32_t* n_out) = 0;
    virtual void generate_beams(int env, int W, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out, float* scores) = 0;
    virtual void turn_beams(const svln_turn_args& a, int W, int64_t* out, int cap, int32_t* n_out, float* scores) = 0;
    virtual void beam_trace(int cap_steps, int32_t* n_steps, int32_t* width, int32_t* list_ids, float* list_lps, int32_t* records) = 0;
    virtual void generate_forced(int env, const int64_t* ids, int n, const int64_t* eos, int n_eos, float* logprobs, int64_t* greedy_ids,
                                 float* greedy_logprobs, int32_t* kv_len) = 0;
    virtual void turn_forced(const svln_turn_args& a, const int64_t* ids, int n, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs,
                             int32_t* kv_len) = 0;
    virtual void generate_candidates(int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos, int n_eos, float* logprobs,
                                     int64_t* greedy_ids, float* greedy_logprobs) = 0;
    virtual void generate_candidates_folded(int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos, int n_eos, float* logprobs,
                                            int64_t* greedy_ids, float* greedy_logprobs) = 0;
    virtual void turn_candidates_folded(const svln_turn_args& a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs,
                                        int64_t* greedy_ids, float* greedy_logprobs) = 0;
    virtual void op_rope_kv_mirror(void* rows, int ld, int Tn, int P, const int32_t* mirror_pages, int n_mirror) = 0;
    virtual void turn_candidates(const svln_turn_args& a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs, int64_t* greedy_ids,
                                 float* greedy_logprobs) = 0;
    virtual int batch_submit_forced(int env, const int64_t* ids, int n, const int64_t* eos, int n_eos) = 0;
    virtual void batch_forced_check(int env, const int64_t* ids, int n, const int64_t* eos, int n_eos) = 0;
    virtual void batch_forced(int slot, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs, int cap, int32_t* n) = 0;
    virtual void batch_forced_stats(int64_t* jobs, int64_t* rows_fed, int64_t* head_launches, int reset) = 0;
    virtual void op_gemv_batched_target(GemvBatchArgs a, const int32_t* targets, float inv_t, int32_t* host_tokens, float* host_greedy,
                                        float* host_logprobs, float* host_slots) = 0;
    virtual void op_gemm_target(GemmArgs a, const int32_t* targets, float inv_t, int32_t* host_tokens, float* host_greedy, float* host_logprobs,
                                float* host_slots) = 0;
    virtual void op_read_argmax_partials(int rows, int n, float* val, int32_t* idx, float* sum) = 0;
    virtual void group_select(int env, int index, int32_t* kv_len) = 0;
    virtual void group_logprobs(int index, float* out, int cap, int32_t* n) = 0;
    virtual void group_dist(int index, float* out, int cap_rows, int32_t* n_rows, int32_t* n_cols) = 0;
    virtual void get_hidden_group(int index, float* out, int max_rows, int32_t* n_rows) = 0;
    virtual void op_kv_page_copy(int src_page, const int32_t* dst_pages, int n_dst) = 0;
    virtual void op_beam_page_gather(const int32_t* src_pages, const int32_t* dst_pages, int n) = 0;
    virtual void op_beam_select(int W, int limit, int B, int n_cp, int len_cap, const int32_t* eos, int n_eos, const int32_t* list_ids,
                                const float* list_lps, const int32_t* hdr_in, const float* score_in, const int32_t* ids_in, const float* lps_in,
                                const int32_t* set_pages, int32_t* hdr_out, float* score_out, int32_t* ids_out, float* lps_out, int32_t* tok_b,
                                int32_t* pair_src, int32_t* pair_dst, int32_t* rec) = 0;
    virtual void op_kv_pool_read(int layer, int start, int n, float* k_out, float* v_out) = 0;
    virtual void sync() = 0;
    virtual void set_graph(int enable) = 0;
    virtual void set_decode_persistent(int enable) = 0;
    virtual void probe_decode_layer(int layer, unsigned long long* out, int max_wgs, int32_t* n_wgs) = 0;
    virtual void op_decode_layer(const svln_decode_layer_op& q) = 0;
    virtual void set_fp8_decode(int enable) = 0;
    virtual void set_fp8_gemm(int enable) = 0;
    virtual void set_fp8_scaled_mfma(int enable) = 0;
    virtual void set_mxfp4_decode(int enable) = 0;
    virtual void set_mxfp4_batched(int enable) = 0;
    virtual void set_speculative(int rows) = 0;
    virtual void set_draft(int env, const int64_t* ids, int n) = 0;
    virtual void draft_stats(int64_t* verify_passes, int64_t* tokens_from_verify, int64_t* single_steps, int reset) = 0;
    virtual void set_prefill_draft(int on) = 0;
    virtual void prefill_draft_stats(int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int reset) = 0;
    virtual void set_batch_draft(int on) = 0;
    virtual void batch_draft_stats(int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int64_t* iterations, int64_t* single_rows, int reset) = 0;
    virtual void op_attention_verify(int rows, const void* ctx, int ld, int ctx_rows, const void* qkv_new, void* out, int o_stride) = 0;
    virtual void op_attention_verify_multi(int S, int T, const void* ctx, int ld, int ctx_rows, const int32_t* ctx_len, const void* qkv_new,
                                           const int32_t* rows, int share, void* out, int o_stride) = 0;
    virtual void op_verify_step(int rows, const int32_t* fed, const int32_t* cand, int count, int max_new, const int64_t* eos, int n_eos,
                                int32_t* new_count, int32_t* done, int64_t* emitted, int32_t* next_token) = 0;
    virtual void op_argmax_step(const svln_argmax_step_op& q) = 0;
    virtual void generate_drafts(int env, int n_drafts, const int64_t* ids, const int32_t* lens, int max_new, const int64_t* eos, int n_eos,
                                 int64_t* out, int cap, int32_t* n_out, int32_t* winner_out, int32_t* pass_tokens_out) = 0;
    virtual void turn_drafts(const svln_turn_args& a, int n_drafts, const int64_t* ids, const int32_t* lens, int64_t* out, int cap,
                             int32_t* n_out, int32_t* kv_len, int32_t* winner_out, int32_t* pass_tokens_out) = 0;
    virtual void drafts_stats(int64_t* out8) = 0;
    virtual void op_draft_select(const svln_draft_select_op& q) = 0;
    virtual void op_dead_step(int done, char* report, int report_cap, int32_t* n_changed) = 0;
    virtual bool op_gemm_fp8(const GemmArgs& a) = 0;
    virtual void set_memory_prune(int keep) = 0;
    virtual void op_memory_prune(const void* m, int n_rows, int keep, int32_t* out_idx, float* out_score) = 0;
    virtual void probe_reset() = 0;
    virtual void probe_read(double* ms, int64_t* launches, double* bytes) = 0;
    virtual void phase_times(double* v, double* p, double* d, int reset) = 0;
    virtual void probe_read_prefill(double* ms, int64_t* n, double* rows, double* flops, double* wbytes) = 0;
    virtual void set_feature_cache(int cap) = 0;
    virtual void feature_cache_stats(int64_t* hits, int64_t* misses) = 0;
    virtual bool op_gemm(const GemmArgs& a) = 0;
    virtual void op_gemv(GemvArgs a, int32_t* host_token) = 0;
    virtual void op_gemv_batched(GemvBatchArgs a, int32_t* host_tokens) = 0;
    virtual void op_gemv_mxfp4_batched(GemvMx4BatchArgs a, int32_t* host_tokens) = 0;
    virtual void op_quant_fp8(const void* w, int64_t rows, int cols, void* w8, float* scale) = 0;
    virtual void set_packed_decode(int enable) = 0;
    virtual void packed_stats(int64_t* packed_bytes, int64_t* bf16_bytes, int64_t* blocks, int64_t* fallback_blocks) = 0;
    virtual void op_pack_rows(const void* w, int ldw, int64_t rows, int cols, void* packed, void* rec, int64_t* fallback_blocks) = 0;
    virtual void op_unpack_rows(const void* packed, const void* rec, const void* w, int ldw, int64_t rows, int cols, void* out) = 0;
    virtual void op_quant_mxfp4(const void* w, int64_t rows, int cols, void* q4, uint8_t* e8) = 0;
    virtual void op_rmsnorm(const void* x, const void* g, void* y, int rows, int n, float eps) = 0;
    virtual void op_layernorm(const void* x, const void* g, const void* b, void* y, int rows, int n, float eps) = 0;
    virtual void op_rmsnorm_tap(const void* x, const void* g, void* y, int rows, int n, float eps, int skip_value, void* y2, int y2_row_value,
                                int y2_cap) = 0;
    virtual void op_rmsnorm_indexed(const void* x, int x_rows, const void* g, void* y, const int32_t* src_rows, const int32_t* tap_rows, void* tap,
                                    int tap_cap, int rows, int n, float eps) = 0;
    virtual void op_gather_rows(const int32_t* src, int rows, const void* embed, int embed_rows, const void* feats, int feat_rows, void* out, int n,
                                int skip_value) = 0;
    virtual void op_gather_rows_ragged(const int32_t* list, int rows, const void* embed, int embed_rows, void* out, int out_rows, int n) = 0;
    virtual void op_frame_hash(const void* pix, int F, int64_t words_per_frame, uint64_t* out_keys) = 0;
    virtual void op_attention_llm(void* qkv, int ld, int T, int P, const void* ctx, int ctx_T, void* out, int o_stride, int nsplit) = 0;
    virtual void op_attention_vit(const void* qkv, int ld, int F, void* out, int o_stride) = 0;
    virtual void op_attention_decode(int B, const void* ctx, int ld, int64_t ctx_rows, const int32_t* pos, const void* qkv_new, void* out,
                                     int o_stride) = 0;
    virtual void op_kv_read(int env, int start, int n, float* k_out, float* v_out) = 0;
    virtual void op_llm_qkv_rope(const void* x, int T, int P, void* q_out, int q_stride, int32_t* fused) = 0;
    virtual void op_set_pages(int env, const int32_t* pages, int n) = 0;
    virtual void op_fill_attn_state(float pool_value, int part_nan) = 0;
    virtual void op_vit_qkv_attention(int layer, const void* x, int F, void* qkv_out, void* attn_out, int o_stride, int force_split,
                                      int32_t* packer) = 0;
    virtual void op_fill_vit_state(float pool_value, int part_nan) = 0;
    virtual void op_vit_kv_read(float* k_out, float* v_out) = 0;
    virtual void op_pool(const void* in, void* out, int F) = 0;
    virtual void op_patchify(const float* pix, void* out, int F) = 0;
};

template <typename T>
class Engine : public EngineBase {
public:
    svln_config c;
    int device;
    hipStream_t st = nullptr;
    std::vector<void*> allocs;
    std::unordered_map<std::string, Slot> slots;

    // derived dims
    int Hv, Iv, vheads, vhd, side, S, kp, oside, otok, H, I, nq, nkv, qkv_dim, V;
    int vhdp, vvrows, vtiles;         // ViT attention geometry
    int pages_per_env, pages_total;

    struct VLayer { T *ln1_w, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b; };
    struct Q8 { uint8_t* q = nullptr; float* s = nullptr; };      // fp8 (e4m3) copy of a weight matrix + per-row scales (opt-in decode mode)
    struct Q4 { uint8_t* q = nullptr; uint8_t* e8 = nullptr; };   // MXFP4 copy of a weight matrix: E2M1 code pairs + one E8M0 scale byte per 32 (opt-in decode mode)
    // lossless 12-bit packing of a bf16 weight matrix (svln_set_packed_decode; format: WP12 in gemv.hip): packed blocks, row records, and
    // the device counter of the blocks that fall back to the bf16 original.  Only the products that gain are packed: gate/up, down_proj
    // and the lm_head (q|k|v and o_proj are one-latency-round launches: DESIGN.md 4.1).
    struct P12 { uint8_t* pk = nullptr; uint8_t* rec = nullptr; unsigned* fb = nullptr; const T* w = nullptr; int64_t rows = 0; int cols = 0; };
    struct LLayer { T *in_norm, *qkv_w, *qkv_b, *o_w, *post_norm, *gu_w, *down_w, *kpool, *vpool; Q8 qkv8, o8, gu8, down8; Q4 qkv4, o4, gu4, down4; P12 gu12, down12; };
    P12 lm_head12; bool p12_on = false;
    std::unordered_map<const void*, P12*> p12_of;      // bf16 matrix -> its packed copy: a write of the matrix (synth / set_tensor) re-encodes it
    Q8 lm_head8; bool fp8_on = false, fp8_built = false;
    Q4 lm_head4; bool mx4_on = false, mx4_built = false;
    bool mx4b_on = false;            // opt-in MXFP4 weights in the batched (multi-env) decode step and the scheduler's lm_head: svln_set_mxfp4_batched
    bool fp8_scaled_on = false;         // the e4m3 products run on the block-scaled MFMAs (svln_set_fp8_scaled_mfma)
    bool fp8_gemm_on = false; uint8_t* act8 = nullptr; float* act8_scale = nullptr;      // opt-in fp8 MFMA products: quantised activation rows
    T *patch_w, *patch_b, *pos_emb, *proj0_w, *proj0_b, *proj2_w, *proj2_b, *embed, *final_norm, *lm_head;
    std::vector<VLayer> vl;
    std::vector<LLayer> ll;

    // vision workspaces
    float* pix = nullptr;
    T *patches, *vx, *vn, *vqkv, *vattn, *vh, *vkpool, *vvpool, *proj_h, *proj_o, *feats;
    int n_feat_frames = 0;
    int* tap_idx; float* tap_w;
    // llm workspaces
    T *x, *xn, *qkv, *attn, *hbuf, *hid_tap, *head_xn;
    float* gemm_ws = nullptr; size_t gemm_ws_elems = 0; void* zero_line = nullptr;
    float* inv_freq; float* rope_tab;
    float* attn_part; size_t attn_part_elems = 0; int nsplit_max, tiles_per_split;
    float* part_val; int* part_idx; int* d_token; float* d_top2;
    GenCtl* d_ctl;               // device-side generation state (position / kv length of the next decode step, done flag, emitted count)
    GenCtl* h_ctl = nullptr;     // pinned
    int *d_eos = nullptr, *d_out_ids = nullptr, *h_out_ids = nullptr; std::vector<int> eos_cached; bool eos_valid = false;
    static constexpr int RUN_AHEAD = 4;     // decode steps enqueued per host synchronisation (a typical turn: 4 action tokens + EOS)
    // batched (multi-env lockstep) decode
    static constexpr int MAXB = 8;
    static constexpr int batched_mfma_min = 4;    // measured at B = 8: 340 vs 319 action-steps/s (gate/up 58 vs 97 us per launch)
    DecodeSlot* d_slots = nullptr; DecodeSlot* h_slots = nullptr; int* d_tok_b = nullptr; int* h_tok_b = nullptr;
    float* part_val_b = nullptr; int* part_idx_b = nullptr; T* last_rows = nullptr; int n_generated_b[MAXB] = {0};
    int* d_src; int* h_src;      // splice descriptors
    // opt-in slow-memory pruning (no reference counterpart): `<memory>` expands to the prune_keep least-average tokens
    int prune_keep = 0; float *prune_partial = nullptr, *prune_mean = nullptr, *prune_score = nullptr; int *d_sel = nullptr, *h_sel = nullptr;
    int* h_token;                // pinned
    float* h_top2;
    // Opt-in token log-probabilities (svln_set_token_scores; no reference counterpart): every lm_head product runs its EPI_ARGMAX_LSE
    // sibling (kernels.h) -- the same tokens, plus log softmax of the emitted token over the processed fp32 logits.  Partial sums beside
    // part_val / part_val_b; the scores of a single-env turn in d_scores[0 .. count) beside d_out_ids, those of a scheduler iteration in
    // d_score_b beside d_tok_b: both are read in the synchronisation that reads the ids.
    bool scores_on = false;
    float *part_sum = nullptr, *part_sum_b = nullptr, *d_scores = nullptr, *h_scores = nullptr, *d_score_b = nullptr, *h_score_b = nullptr;
    float* row_scale_b = nullptr;            // [MAXB]: the row factors of a scored batched GEMV with a fused norm (svln_op_gemv_batched_argmax_scores only)
    // Opt-in top-k log-probabilities (svln_top_logprobs; single-env turns): while topk > 0 head() runs the EPI_*_TOPK sibling of its scored
    // or sampled lm_head GEMV (cand_val / cand_idx: TOPK_C candidates beside every partial; under an allowed list the subset product's
    // partials are the candidates) and topk_merge_kernel writes d_topi / d_topl [count][topk] beside d_scores[count].
    int topk = 0;
    float *cand_val = nullptr, *d_topl = nullptr, *h_topl = nullptr; int *cand_idx = nullptr, *d_topi = nullptr, *h_topi = nullptr;
    std::vector<int32_t> last_topi; std::vector<float> last_topl; int last_topk = 0; bool last_topk_valid = false;
    // ... and of the batched heads (argmax_rows): candidates [rows][partials][TOPK_C], lists d_topi_b / d_topl_b [tok0 + b][topk] beside d_score_b
    float *cand_val_b = nullptr, *d_topl_b = nullptr, *h_topl_b = nullptr; int *cand_idx_b = nullptr, *d_topi_b = nullptr, *h_topi_b = nullptr;
    std::vector<std::vector<int32_t>> gb_topi; std::vector<std::vector<float>> gb_topl; int gb_topk = 0; bool gb_topk_valid = false;
    void ensure_topk_buffers() {
        if (cand_val) return;
        const size_t rows = (size_t)c.max_positions + 8;
        cand_val = dalloc<float>((size_t)2048 * TOPK_C); cand_idx = dalloc<int>((size_t)2048 * TOPK_C);
        d_topi = dalloc<int>(rows * TOPK_C, true); d_topl = dalloc<float>(rows * TOPK_C, true);
        HIP_CHECK(hipHostMalloc((void**)&h_topi, rows * TOPK_C * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_topl, rows * TOPK_C * sizeof(float)));
        cand_val_b = dalloc<float>((size_t)HEAD_ROWS * 2048 * TOPK_C); cand_idx_b = dalloc<int>((size_t)HEAD_ROWS * 2048 * TOPK_C);
        d_topi_b = dalloc<int>((size_t)(HEAD_ROWS + MAXB) * TOPK_C, true); d_topl_b = dalloc<float>((size_t)(HEAD_ROWS + MAXB) * TOPK_C, true);
        HIP_CHECK(hipHostMalloc((void**)&h_topi_b, (size_t)(HEAD_ROWS + MAXB) * TOPK_C * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_topl_b, (size_t)(HEAD_ROWS + MAXB) * TOPK_C * sizeof(float)));
    }
    std::vector<float> last_scores; bool last_scores_valid = false;           // of the last svln_generate / svln_turn / svln_generate_fixed
    // Opt-in token entropies (svln_token_entropy; tied to svln_set_token_scores as svln_top_logprobs is): while ent_on every lm_head product
    // runs the EPI_*_ENT sibling of its scored or sampled form (part_ent / part_ent_b: one more fp32 beside every partial sum; the subset
    // product of an allowed list stays as it is: one id per partial, t = 0) and entropy_merge_kernel writes d_ent[count] beside
    // d_scores[count], d_ent_b[tok0 + b] beside d_score_b.  The final / step kernels are untouched.
    bool ent_on = false;
    float *part_ent = nullptr, *part_ent_b = nullptr, *d_ent = nullptr, *h_ent = nullptr, *d_ent_b = nullptr, *h_ent_b = nullptr;
    std::vector<float> last_ent; bool last_ent_valid = false;
    std::vector<std::vector<float>> gb_ent; bool gb_ent_valid = false;
    void ensure_ent_buffers() {
        if (part_ent) return;
        const size_t rows = (size_t)c.max_positions + 8;
        part_ent = dalloc<float>(2048); part_ent_b = dalloc<float>((size_t)HEAD_ROWS * 2048);
        d_ent = dalloc<float>(rows, true); d_ent_b = dalloc<float>(HEAD_ROWS + MAXB, true);
        HIP_CHECK(hipHostMalloc((void**)&h_ent, rows * sizeof(float)));
        HIP_CHECK(hipHostMalloc((void**)&h_ent_b, (HEAD_ROWS + MAXB) * sizeof(float)));
    }
    // Opt-in temperature sampling (svln_set_sampling; no reference counterpart): every lm_head product runs its EPI_SAMPLE sibling
    // (kernels.h): token = argmax_n (fl(x_n * inv_t) + G(seed, stream, draw, n)), an exact sample of softmax(x / T).  stream = the env slot,
    // draw = env_draws[env] + the tokens of this turn.  A single-env turn carries both in GenCtl (draw0, stream); the scheduler uploads
    // d_smp[0 .. rows) = streams, d_smp[SMP_ROWS .. + rows) = draws per iteration.  The sampled kernels always compute the token's
    // log-probability under softmax(x / T) (d_scores / d_score_b); it is delivered only while svln_set_token_scores is on.
    static constexpr int SMP_ROWS = 64 + 8;  // HEAD_ROWS + MAXB
    bool smp_on = false; float smp_inv_t = 1.0f; uint64_t smp_seed = 0;
    float *part_raw = nullptr, *part_max = nullptr, *part_raw_b = nullptr, *part_max_b = nullptr;
    int *d_smp = nullptr, *h_smp = nullptr;
    std::vector<int> env_draws;              // tokens every env has emitted since the last svln_set_sampling
    // Opt-in truncated sampling (svln_sampling_truncation; an attribute of svln_set_sampling): while trunc_k > 0 every lm_head product of a
    // sampled pass runs its EPI_SAMPLE_TOPK form (the candidates of ensure_topk_buffers, lists on or off), truncate_partials_kernel
    // (kernels.h, launch_truncate_partials) turns them into an 8-entry partial row -- tr_* [1][TOPK_C] for head(), tr_*_b
    // [SMP_ROWS][TOPK_C] for argmax_rows() -- and the unchanged final / step kernel reduces that row.  top_k / top_p are launch scalars.
    int trunc_k = 0; float trunc_p = 1.0f;
    float *tr_val = nullptr, *tr_raw = nullptr, *tr_max = nullptr, *tr_sum = nullptr, *tr_val_b = nullptr, *tr_raw_b = nullptr, *tr_max_b = nullptr, *tr_sum_b = nullptr;
    int *tr_idx = nullptr, *tr_idx_b = nullptr;
    void ensure_trunc_buffers() {
        ensure_topk_buffers();
        if (tr_val) return;
        tr_val = dalloc<float>(TOPK_C); tr_raw = dalloc<float>(TOPK_C); tr_max = dalloc<float>(TOPK_C); tr_sum = dalloc<float>(TOPK_C); tr_idx = dalloc<int>(TOPK_C);
        const size_t nb = (size_t)SMP_ROWS * TOPK_C;
        tr_val_b = dalloc<float>(nb); tr_raw_b = dalloc<float>(nb); tr_max_b = dalloc<float>(nb); tr_sum_b = dalloc<float>(nb); tr_idx_b = dalloc<int>(nb);
    }
    bool top2_sampled = false;               // the last turn was sampled: d_top2 holds perturbed values, not logits
    // an op-level override of the engine's own switch (svln_op_*_argmax_sample): the product's SampleArgs scalars
    SampleArgs smp_args(const int* stream, const int* draw, const int* count, float* raw, float* mx) const {
        SampleArgs q; q.stream = stream; q.draw = draw; q.count = count; q.inv_t = smp_inv_t;
        q.seed_lo = (uint32_t)smp_seed; q.seed_hi = (uint32_t)(smp_seed >> 32); q.part_raw = raw; q.part_max = mx; return q;
    }
    std::vector<std::vector<float>> gb_scores; bool gb_scores_valid = false;  // of the last svln_generate_batch, per listed env
    // Opt-in allowed-token decode (svln_set_allowed_tokens; HF's prefix_allowed_tokens_fn with a constant set): while a list is set every
    // lm_head product of the engine -- head(), argmax_rows() on lm_head, the MXFP4 branch of head_batched() -- is the subset product
    // (gemv_subset.hip) on the engine-dtype lm_head, whichever weight-format switch is on: n <= 256 rows gain nothing from an e4m3 or
    // MXFP4 copy, and one format makes the head the same function on every path.  One arg-max partial per listed id; the merge kernels
    // run unchanged on allow_n partials.  While svln_set_token_scores is on too, subset_logprobs_kernel writes the whole normalised row
    // of every emitted token: d_alp[count][allow_n] beside d_scores, d_alp_b[tok0 + b][allow_n] beside d_score_b.
    static constexpr int ALLOW_MAX = 256;
    bool allow_on = false; int allow_n = 0; std::vector<int> allow_ids;
    int *d_allow = nullptr, *d_op_allow = nullptr;   // the engine's list / the list of svln_op_subset_argmax, ALLOW_MAX ints each
    float *d_alp = nullptr, *h_alp = nullptr, *d_alp_b = nullptr, *h_alp_b = nullptr;
    std::vector<float> last_alp; int last_alp_n = 0; bool last_alp_valid = false;           // of the last single-env turn
    std::vector<std::vector<float>> gb_alp; int gb_alp_n = 0; bool gb_alp_valid = false;    // of the last svln_generate_batch

    // Opt-in group sampling (svln_generate_group; HF's num_return_sequences): n_seq sampled continuations of one prefill.  Sequence 0 decodes
    // on the env's own page table; sequence g >= 1 on fork_tab[g]: the env's pages below q0 = L / 64 (shared, never written: every write
    // of the turn is at a position >= L) and private pages from q0 on (Group::tail[g]); the partly filled page q0 is copied by ONE launch
    // of kv_page_copy_kernel over d_pool_tab (every layer's K and V^T pool base).  The group stays pending on its env until
    // svln_group_select picks the continuation (or a reset drops it).
    static constexpr int FORK_MAX_DST = MAXB - 1;
    void** d_pool_tab = nullptr;                         // [2 * layers]: kpool, vpool per layer
    int* fork_tab[MAXB] = {nullptr};                     // device page tables of sequences 1 .. 7 (allocated on first use)
    int *d_fork_dst = nullptr, *h_fork_dst = nullptr;    // destination pages of the fork launch (device / pinned)
    struct Group {
        bool pending = false, scored = false;
        int env = -1, n_seq = 0, L = 0, q0 = 0, n_tail = 0, alp_n = 0;
        int n_out[MAXB] = {0};
        std::vector<int> tail[MAXB];                     // private pages of sequence g >= 1: its table entries [q0, q0 + n_tail)
        std::vector<float> scores[MAXB], alp[MAXB];
    };
    Group grp;

    struct Env {
        T* embeds = nullptr; int n_embeds = 0; int kv_len = 0;
        int* d_pages = nullptr; std::vector<int> pages; int n_pages = 0;
    };
    std::vector<Env> envs;
    std::vector<int> free_pages;
    int n_generated = 0;
    // Opt-in draft-verified greedy decode (svln_set_speculative; no reference counterpart: the emitted ids are those of the plain greedy
    // loop).  A verify pass feeds the last emitted token and up to spec_rows - 1 guessed tokens as the rows of ONE pass over the weights
    // (the batched step's products at B = spec_rows, the verify attention, the verify step) and keeps the longest confirmed prefix.
    int spec_rows = 0;                       // 0 = off, else rows per verify pass (2, 4, 8)
    std::vector<std::vector<int64_t>> drafts; std::vector<char> draft_armed;     // per env: the caller's guess of the next turn's ids (svln_set_draft)
    int *d_draft = nullptr, *h_draft = nullptr;      // the armed draft of the running turn (device copy / pinned staging)
    int *d_vctl = nullptr, *h_vctl = nullptr;        // [0] usable draft length, [1] rows of the pass, [2] passes, [3] tokens of the turn; d_vctl[8 ..] = fed rows
    int64_t st_passes = 0, st_vtokens = 0, st_single = 0;
    bool top2_stale = false;                 // the last token of the last turn came from a verify pass or a ride (which keep no top-2 logits)
    // Opt-in drafts inside the prefill pass (svln_set_prefill_draft; no reference counterpart, same ids as the plain loop).  A "ride" is a
    // prefill whose last k rows are the embeddings of the draft's first k ids at positions L .. L + k - 1: the lm_head arg-max of its
    // last k + 1 rows goes through the verify step from count = 0, so a confirmed turn needs no decode pass at all.  Ride state in
    // d_vctl: [4] rides run, [5] tokens they emitted, [6] head rows of the ride (k + 1).
    bool ride_on = false;
    static constexpr int RIDE_MAX_ROWS = 7;  // fed draft rows per ride: the verify step holds 8 head rows
    int64_t st_rides = 0, st_rtokens = 0, st_rrows = 0;
    // Opt-in drafts in the scheduler's prefill pass (svln_set_batch_draft; independent of the two switches above).  A job keeps the usable
    // part of the draft its env had armed at the submit; the iteration that prefills the job appends k of its ids as rows of the job's
    // segment and the host applies the verify rule to the k + 1 arg-maxes of that job.  Head rows of such an iteration: one per decode
    // row, k + 1 per segment, at most HEAD_ROWS; the lists of the indexed norm and of the ragged gather are staged in pinned memory.
    bool bdraft_on = false;
    static constexpr int HEAD_ROWS = 64;     // MAXB jobs x (RIDE_MAX_ROWS + 1) head rows
    // the ragged gather list holds the draft rows of every ride (MAXB x RIDE_MAX_ROWS pairs) and the fed rows of every forced job
    // (svln_batch_submit_forced: MAXB x (BFORCED_MAX - 1) pairs) of one iteration
    static constexpr int BFORCED_MAX = 32;                       // ids of one forced job (= FORCED_MAX)
    static constexpr int BFORCED_ROWS = MAXB * BFORCED_MAX;      // forced head rows of one iteration
    static constexpr int RIDE_PAIRS = MAXB * RIDE_MAX_ROWS + MAXB * (BFORCED_MAX - 1);
    int *d_head_src = nullptr, *d_head_tap = nullptr, *d_ride_list = nullptr;       // device lists: [HEAD_ROWS], [HEAD_ROWS], [RIDE_PAIRS] pairs
    int *h_head_src = nullptr, *h_head_tap = nullptr, *h_ride_list = nullptr;       // pinned
    int64_t st_brides = 0, st_btokens = 0, st_brows = 0, st_biters = 0, st_bsingle = 0;
    // Forced jobs of the scheduler (svln_batch_submit_forced): their head rows are normed into bf_xn, rows of their own beside xn, and go
    // through the EPI_TARGET lm_head in chunks of <= 32; every list is sized for MAXB jobs of BFORCED_MAX ids (+ 8: the pad rows of the last
    // chunk's row count), so no job waits for head space.  Allocated by the first forced submit.
    T* bf_xn = nullptr;
    // the lists of the target head, BFORCED_ROWS + 8 entries each, cut from one int and one float block: source row, tap row, target id,
    // greedy id / capture slot, greedy log-probability, target log-probability
    struct HeadLists {
        static constexpr int R = BFORCED_ROWS + 8;
        int *src = nullptr, *tap = nullptr, *tgt = nullptr, *tok = nullptr; float *val = nullptr, *score = nullptr, *lp = nullptr;
        void cut(int* i, float* f) { src = i; tap = i + R; tgt = i + 2 * R; tok = i + 3 * R; val = f; score = f + R; lp = f + 2 * R; }
    };
    HeadLists bf_dev, bf_host;                                   // device / pinned (bf_host.src and bf_host.val own the pinned blocks)
    float *bf_dev_alp = nullptr, *bf_host_alp = nullptr;         // [BFORCED_ROWS][ALLOW_MAX], with the first forced submit under an allowed list
    int64_t st_fjobs = 0, st_frows = 0, st_fhead = 0;

    // decode graph + probes.  The step graph holds the env's page-table pointer, so there is one set per env (a round-robin over several
    // envs through svln_generate replays instead of re-capturing); [0] = the whole step, [1] / [2] = the halves around the probed launch
    // (captured only while the roofline probe is on); a run-ahead batch of several steps is one graph.
    bool use_graph = false;
    struct GraphSet { std::unordered_map<int, hipGraphExec_t> ex; };     // key: steps (whole batch) | 1000 (head of a probed step) | 2000 + steps (its tail) | 3000 + rows (verify pass); + head_graph_key() (10000 with svln_set_token_scores, 20000 with svln_set_sampling, 100000 k with svln_top_logprobs(k), 1000000 with svln_token_entropy) + 40000 with svln_set_packed_decode
    std::vector<GraphSet> graphs;
    std::unordered_map<int, hipGraphExec_t> bgraphs;          // batched decode step: key = B | penalty << 8 | fp8 gemm << 9 | MXFP4 batched << 10 | scaled fp8 form << 11 | token scores << 12
    // per-turn truncation of the spliced rows (the reference's config.tokenizer_model_max_length, stream_video_vln.py:241-244); 0 = none
    int turn_row_limit = 0;
    // HF repetition penalty of the checkpoint's generation_config (1 = off): flags of the tokens generated in the current turn
    float rep_penalty = 1.0f; uint8_t* pen_flags = nullptr; uint8_t* pen_flags_b = nullptr; int* d_pen_rows = nullptr; int* h_pen_rows = nullptr;
    int* d_pen_ids = nullptr; int* h_pen_ids = nullptr;
    std::vector<hipEvent_t> probe_ev; size_t probe_used = 0; bool probe_on = false; double probe_bytes = 0;
    // second probe: the layer-0 gate/up product of every steady prefill (M <= 256 rows: main launch + K-split tail + reduce) between two events
    std::vector<hipEvent_t> pprobe_ev; size_t pprobe_used = 0; double pprobe_rows = 0;
    hipEvent_t ph_ev[5]; double ph_ms[3] = {0, 0, 0}; bool vision_pending = false;   // v0 v1 p0 p1 d1

    template <typename U> U* dalloc(size_t n, bool zero = false) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, n * sizeof(U) + 256));
        if (zero) HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(U), st));
        allocs.push_back(p);
        return (U*)p;
    }
    void add_slot(const std::string& name, void* dst, int ld, int64_t rows, int cols, RowMap m = RowMap{1 << 30, 1, 0}) {
        const bool vision = name.rfind("model.vision_tower.", 0) == 0 || name.rfind("model.mm_projector.", 0) == 0;
        slots[name] = Slot{dst, ld, rows, cols, m, false, vision};
    }
    void add_linear(const std::string& name, T* w, T* b, int out_f, int in_f) {
        add_slot(name + ".weight", w, in_f, out_f, in_f);
        if (b) add_slot(name + ".bias", b, out_f, 1, out_f);
    }

    int device_id() const override { return device; }

    Engine(const svln_config& cfg, int dev) : c(cfg), device(dev) {
        DeviceGuard guard(dev);
        HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        Hv = c.v_hidden; Iv = c.v_inter; vheads = c.v_heads; vhd = Hv / vheads; side = c.v_image / c.v_patch; S = side * side;
        kp = ((3 * c.v_patch * c.v_patch + 7) / 8) * 8;
        oside = (side + 1) / 2; otok = oside * oside;
        H = c.hidden; I = c.inter; nq = c.q_heads; nkv = c.kv_heads; qkv_dim = (nq + 2 * nkv) * c.head_dim; V = c.vocab;
        REQUIRE(c.head_dim == 128, "LLM head_dim must be 128");
        REQUIRE(vhd == 72, "vision head_dim must be 72");
        REQUIRE(nq % nkv == 0, "q_heads must be a multiple of kv_heads");
        REQUIRE(nq / nkv <= 32, "at most 32 q heads per kv head (decode attention keeps one GQA group in a 32-row tile)");
        REQUIRE(H % 8 == 0 && I % 32 == 0 && Hv % 8 == 0 && Iv % 8 == 0, "dims must be multiples of 8 (inter of 32)");
        REQUIRE(c.max_positions % PAGE == 0, "max_positions must be a multiple of 64");
        constexpr int EPC = Elt<T>::PER_CHUNK;
        vhdp = ((((vhd + EPC - 1) / EPC) + 1) & ~1) * EPC;
        vvrows = ((vhd + 31) / 32) * 32;
        vtiles = (S + PAGE - 1) / PAGE;

        const std::string VT = "model.vision_tower.vision_tower.vision_model.";
        patch_w = dalloc<T>((size_t)Hv * kp, true); patch_b = dalloc<T>(Hv); pos_emb = dalloc<T>((size_t)S * Hv);
        add_slot(VT + "embeddings.patch_embedding.weight", patch_w, kp, Hv, 3 * c.v_patch * c.v_patch);
        add_slot(VT + "embeddings.patch_embedding.bias", patch_b, Hv, 1, Hv);
        add_slot(VT + "embeddings.position_embedding.weight", pos_emb, Hv, S, Hv);
        vl.resize(c.v_layers);
        for (int i = 0; i < c.v_layers; ++i) {
            VLayer& L = vl[i];
            const std::string P = VT + "encoder.layers." + std::to_string(i) + ".";
            L.ln1_w = dalloc<T>(Hv); L.ln1_b = dalloc<T>(Hv); L.ln2_w = dalloc<T>(Hv); L.ln2_b = dalloc<T>(Hv);
            L.qkv_w = dalloc<T>((size_t)3 * Hv * Hv); L.qkv_b = dalloc<T>(3 * Hv);
            L.out_w = dalloc<T>((size_t)Hv * Hv); L.out_b = dalloc<T>(Hv);
            L.fc1_w = dalloc<T>((size_t)Iv * Hv); L.fc1_b = dalloc<T>(Iv);
            L.fc2_w = dalloc<T>((size_t)Hv * Iv); L.fc2_b = dalloc<T>(Hv);
            add_slot(P + "layer_norm1.weight", L.ln1_w, Hv, 1, Hv); add_slot(P + "layer_norm1.bias", L.ln1_b, Hv, 1, Hv);
            add_slot(P + "layer_norm2.weight", L.ln2_w, Hv, 1, Hv); add_slot(P + "layer_norm2.bias", L.ln2_b, Hv, 1, Hv);
            add_linear(P + "self_attn.q_proj", L.qkv_w, L.qkv_b, Hv, Hv);
            add_linear(P + "self_attn.k_proj", L.qkv_w + (size_t)Hv * Hv, L.qkv_b + Hv, Hv, Hv);
            add_linear(P + "self_attn.v_proj", L.qkv_w + (size_t)2 * Hv * Hv, L.qkv_b + 2 * Hv, Hv, Hv);
            add_linear(P + "self_attn.out_proj", L.out_w, L.out_b, Hv, Hv);
            add_linear(P + "mlp.fc1", L.fc1_w, L.fc1_b, Iv, Hv);
            add_linear(P + "mlp.fc2", L.fc2_w, L.fc2_b, Hv, Iv);
        }
        proj0_w = dalloc<T>((size_t)H * Hv); proj0_b = dalloc<T>(H); proj2_w = dalloc<T>((size_t)H * H); proj2_b = dalloc<T>(H);
        add_linear("model.mm_projector.0", proj0_w, proj0_b, H, Hv);
        add_linear("model.mm_projector.2", proj2_w, proj2_b, H, H);
        embed = dalloc<T>((size_t)V * H);
        add_slot("model.embed_tokens.weight", embed, H, V, H);

        pages_per_env = c.max_positions / PAGE;
        pages_total = pages_per_env * c.max_envs;
        ll.resize(c.layers);
        const int qd = nq * 128, kd = nkv * 128;
        for (int i = 0; i < c.layers; ++i) {
            LLayer& L = ll[i];
            const std::string P = "model.layers." + std::to_string(i) + ".";
            L.in_norm = dalloc<T>(H); L.post_norm = dalloc<T>(H);
            L.qkv_w = dalloc<T>((size_t)qkv_dim * H); L.qkv_b = dalloc<T>(qkv_dim);
            L.o_w = dalloc<T>((size_t)H * qd); L.gu_w = dalloc<T>((size_t)2 * I * H); L.down_w = dalloc<T>((size_t)H * I);
            L.kpool = dalloc<T>((size_t)pages_total * nkv * PAGE * 128, true);
            L.vpool = dalloc<T>((size_t)pages_total * nkv * 128 * PAGE, true);
            add_slot(P + "input_layernorm.weight", L.in_norm, H, 1, H);
            add_slot(P + "post_attention_layernorm.weight", L.post_norm, H, 1, H);
            add_linear(P + "self_attn.q_proj", L.qkv_w, L.qkv_b, qd, H);
            add_linear(P + "self_attn.k_proj", L.qkv_w + (size_t)qd * H, L.qkv_b + qd, kd, H);
            add_linear(P + "self_attn.v_proj", L.qkv_w + (size_t)(qd + kd) * H, L.qkv_b + qd + kd, kd, H);
            add_linear(P + "self_attn.o_proj", L.o_w, nullptr, H, qd);
            add_slot(P + "mlp.gate_proj.weight", L.gu_w, H, I, H, RowMap{32, 2, 0});
            add_slot(P + "mlp.up_proj.weight", L.gu_w, H, I, H, RowMap{32, 2, 1});
            add_linear(P + "mlp.down_proj", L.down_w, nullptr, H, I);
        }
        {   // base of every layer's K and V^T pool, for the one-launch page fork (kv_fork.hip)
            std::vector<void*> tab;
            for (const LLayer& L : ll) { tab.push_back(L.kpool); tab.push_back(L.vpool); }
            d_pool_tab = dalloc<void*>(tab.size());
            HIP_CHECK(hipMemcpy(d_pool_tab, tab.data(), tab.size() * sizeof(void*), hipMemcpyHostToDevice));
            d_fork_dst = dalloc<int>(MAXB, true);
            HIP_CHECK(hipHostMalloc((void**)&h_fork_dst, MAXB * sizeof(int)));
        }
        final_norm = dalloc<T>(H); lm_head = dalloc<T>((size_t)V * H);
        add_slot("model.norm.weight", final_norm, H, 1, H);
        add_slot("lm_head.weight", lm_head, H, V, H);
        for (auto& L : ll) {        // what build_fp8_weights / build_mxfp4_weights copy (ll is never resized again: the pointers stay)
            qmats.push_back(QMat{L.qkv_w, qkv_dim, H, &L.qkv8, &L.qkv4}); qmats.push_back(QMat{L.o_w, H, qd, &L.o8, &L.o4});
            qmats.push_back(QMat{L.gu_w, 2 * (int64_t)I, H, &L.gu8, &L.gu4}); qmats.push_back(QMat{L.down_w, H, I, &L.down8, &L.down4});
        }
        qmats.push_back(QMat{lm_head, V, H, &lm_head8, &lm_head4});
        if (sizeof(T) == 2 && H <= P12_MAX_K && I <= P12_MAX_K) {      // packed copies of the decode GEMVs' big weight streams; on by default
            unsigned* counters = dalloc<unsigned>(2 * (size_t)c.layers + 1, true);
            auto make = [&](P12& m, const T* w, int64_t rows, int cols) {
                m.pk = dalloc<uint8_t>((size_t)rows * p12_row_bytes(cols)); m.rec = dalloc<uint8_t>((size_t)rows * 16);
                m.fb = counters++; m.w = w; m.rows = rows; m.cols = cols;
                p12_of[w] = &m;
            };
            for (auto& L : ll) { make(L.gu12, L.gu_w, 2 * (int64_t)I, H); make(L.down12, L.down_w, H, I); }
            make(lm_head12, lm_head, V, H);
            p12_on = true;
        }

        // vision workspaces
        const size_t rv = (size_t)c.max_frames * S;
        pix = dalloc<float>((size_t)c.max_frames * 3 * c.v_image * c.v_image);
        patches = dalloc<T>(rv * kp); vx = dalloc<T>(rv * Hv); vn = dalloc<T>(rv * Hv); vqkv = dalloc<T>(rv * 3 * Hv);
        vattn = dalloc<T>(rv * Hv); vh = dalloc<T>(rv * Iv);
        vkpool = dalloc<T>((size_t)vtiles * c.max_frames * vheads * PAGE * vhdp, true);
        vvpool = dalloc<T>((size_t)vtiles * c.max_frames * vheads * vvrows * PAGE, true);
        proj_h = dalloc<T>(rv * H); proj_o = dalloc<T>(rv * H);
        feats = dalloc<T>((size_t)c.max_frames * otok * H);
        {   // bilinear taps: F.interpolate(align_corners=False), scale = side/oside  (stream_video_vln.py:64-67)
            std::vector<int> ti(2 * oside); std::vector<float> tw(2 * oside);
            const double scale = (double)side / (double)oside;
            for (int d = 0; d < oside; ++d) {
                double src = (d + 0.5) * scale - 0.5; if (src < 0) src = 0;
                int i0 = (int)std::floor(src); if (i0 > side - 1) i0 = side - 1;
                int i1 = i0 + 1 < side ? i0 + 1 : side - 1;
                float l1 = (float)(src - i0);
                ti[2 * d] = i0; ti[2 * d + 1] = i1; tw[2 * d] = 1.0f - l1; tw[2 * d + 1] = l1;
            }
            tap_idx = dalloc<int>(2 * oside); tap_w = dalloc<float>(2 * oside);
            HIP_CHECK(hipMemcpy(tap_idx, ti.data(), ti.size() * sizeof(int), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(tap_w, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        // llm workspaces
        const size_t rt = (size_t)c.max_positions;
        x = dalloc<T>(rt * H); xn = dalloc<T>(rt * H); qkv = dalloc<T>(rt * qkv_dim); attn = dalloc<T>(rt * qd); hbuf = dalloc<T>(rt * I);
        hid_tap = dalloc<T>((size_t)HID_TAP_ROWS * H);
        head_xn = dalloc<T>((size_t)H);
        {   // split-K slabs: enough for 8 splits of the widest skinny product (rows of one ViT frame batch or a 512-row prefill)
            size_t widest = (size_t)(qkv_dim > 3 * Hv ? qkv_dim : 3 * Hv);
            if ((size_t)Iv > widest) widest = Iv;
            size_t rows = (size_t)c.max_frames * S > 768 ? (size_t)c.max_frames * S : 768;
            gemm_ws_elems = 8 * rows * widest;
            if (gemm_ws_elems > (size_t)64 << 20) gemm_ws_elems = (size_t)64 << 20;
            gemm_ws = dalloc<float>(gemm_ws_elems);
            zero_line = dalloc<char>(256, true);
        }
        {
            std::vector<float> f(64);
            for (int j = 0; j < 64; ++j) f[j] = 1.0f / powf(c.rope_theta, (float)(2 * j) / 128.0f);     // modeling_qwen2.py:115
            inv_freq = dalloc<float>(64);
            HIP_CHECK(hipMemcpy(inv_freq, f.data(), 64 * sizeof(float), hipMemcpyHostToDevice));
            rope_tab = dalloc<float>((size_t)c.max_positions * 128);
            launch_rope_table(st, rope_tab, inv_freq, c.max_positions);
        }
        tiles_per_split = 1;                       // decode: one 64-key page per workgroup, <= 64 splits
        while ((pages_per_env + tiles_per_split - 1) / tiles_per_split > 64) ++tiles_per_split;
        nsplit_max = (pages_per_env + tiles_per_split - 1) / tiles_per_split;
        {   // partials: decode [nsplit_max][nkv][32][132], prefill split-KV [<= 8][nkv][PREFILL_SPLIT_ROWS][132]
            constexpr int PW = 128 + ATTN_PART_PAD;
            const size_t dec = (size_t)MAXB * nsplit_max * nkv * 32 * PW, pre = (size_t)8 * nkv * PREFILL_SPLIT_ROWS * PW;
            attn_part_elems = dec > pre ? dec : pre;
            attn_part = dalloc<float>(attn_part_elems);
        }
        part_val = dalloc<float>(2048); part_idx = dalloc<int>(2048); part_sum = dalloc<float>(2048);
        d_scores = dalloc<float>((size_t)c.max_positions + 8, true); d_score_b = dalloc<float>(HEAD_ROWS + MAXB, true);
        part_sum_b = dalloc<float>((size_t)HEAD_ROWS * 2048); row_scale_b = dalloc<float>(MAXB, true);
        static_assert(SMP_ROWS == HEAD_ROWS + MAXB, "SMP_ROWS");
        part_raw = dalloc<float>(2048); part_max = dalloc<float>(2048);
        part_raw_b = dalloc<float>((size_t)HEAD_ROWS * 2048); part_max_b = dalloc<float>((size_t)HEAD_ROWS * 2048);
        d_smp = dalloc<int>(2 * SMP_ROWS, true);
        HIP_CHECK(hipHostMalloc((void**)&h_smp, 2 * SMP_ROWS * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_scores, ((size_t)c.max_positions + 8) * sizeof(float)));
        HIP_CHECK(hipHostMalloc((void**)&h_score_b, (HEAD_ROWS + MAXB) * sizeof(float)));
        d_token = dalloc<int>(4, true); d_top2 = dalloc<float>(4, true);
        d_ctl = (GenCtl*)dalloc<int>(sizeof(GenCtl) / sizeof(int), true);
        d_eos = dalloc<int>((size_t)(V > 16 ? V : 16)); d_out_ids = dalloc<int>((size_t)c.max_positions + 8);
        HIP_CHECK(hipHostMalloc((void**)&h_ctl, sizeof(GenCtl)));
        HIP_CHECK(hipHostMalloc((void**)&h_out_ids, ((size_t)c.max_positions + 8) * sizeof(int)));
        d_slots = dalloc<DecodeSlot>(MAXB, true); d_tok_b = dalloc<int>(HEAD_ROWS + MAXB, true);
        part_val_b = dalloc<float>((size_t)HEAD_ROWS * 2048); part_idx_b = dalloc<int>((size_t)HEAD_ROWS * 2048);
        last_rows = dalloc<T>((size_t)HEAD_ROWS * H);
        HIP_CHECK(hipHostMalloc((void**)&h_slots, MAXB * sizeof(DecodeSlot)));
        HIP_CHECK(hipHostMalloc((void**)&h_tok_b, (HEAD_ROWS + MAXB) * sizeof(int)));
        d_head_src = dalloc<int>(2 * HEAD_ROWS + 2 * RIDE_PAIRS, true); d_head_tap = d_head_src + HEAD_ROWS; d_ride_list = d_head_src + 2 * HEAD_ROWS;
        HIP_CHECK(hipHostMalloc((void**)&h_head_src, (2 * HEAD_ROWS + 2 * RIDE_PAIRS) * sizeof(int)));
        h_head_tap = h_head_src + HEAD_ROWS; h_ride_list = h_head_src + 2 * HEAD_ROWS;
        d_src = dalloc<int>(rt);
        HIP_CHECK(hipHostMalloc((void**)&h_src, rt * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_token, 16));
        HIP_CHECK(hipHostMalloc((void**)&h_top2, 16));
        envs.resize(c.max_envs);
        env_draws.assign(c.max_envs, 0);
        graphs.resize(c.max_envs);
        for (auto& e : envs) {
            e.embeds = dalloc<T>(rt * H);
            e.d_pages = dalloc<int>(pages_per_env, true);
            e.pages.assign(pages_per_env, 0);
        }
        for (int p = pages_total - 1; p >= 0; --p) free_pages.push_back(p);
        for (int i = 0; i < 5; ++i) HIP_CHECK(hipEventCreate(&ph_ev[i]));
        HIP_CHECK(init_kernel_attributes());
        HIP_CHECK(hipStreamSynchronize(st));
    }

    ~Engine() override {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
        drop_graphs();
        if (d_rgb) (void)hipFree(d_rgb);
        for (auto& t : rs_tabs) for (void* p : t.bufs) (void)hipFree(p);
        for (int i = 0; i < 2; ++i) {
            if (h_rgb[i]) (void)hipHostFree(h_rgb[i]);
            if (h2d_ev[i]) (void)hipEventDestroy(h2d_ev[i]);
        }
        for (auto& pr : pp_ring) { if (pr.a) (void)hipEventDestroy(pr.a); if (pr.b) (void)hipEventDestroy(pr.b); }
        if (src_ev) (void)hipEventDestroy(src_ev);
        for (auto ev : ring_ev) (void)hipEventDestroy(ev);
        if (ring_host) (void)hipHostFree(ring_host);
        for (auto e : probe_ev) (void)hipEventDestroy(e);
        for (auto e : pprobe_ev) (void)hipEventDestroy(e);
        for (int i = 0; i < 5; ++i) (void)hipEventDestroy(ph_ev[i]);
        (void)hipHostFree(h_ctl); (void)hipHostFree(h_out_ids); (void)hipHostFree(h_scores); (void)hipHostFree(h_score_b);
        if (h_topi) (void)hipHostFree(h_topi);
        if (h_topl) (void)hipHostFree(h_topl);
        if (h_topi_b) (void)hipHostFree(h_topi_b);
        if (h_topl_b) (void)hipHostFree(h_topl_b);
        if (h_ent) (void)hipHostFree(h_ent);
        if (h_ent_b) (void)hipHostFree(h_ent_b);
        if (h_smp) (void)hipHostFree(h_smp);
        if (h_fork_dst) (void)hipHostFree(h_fork_dst);
        if (h_alp) (void)hipHostFree(h_alp);
        if (h_alp_b) (void)hipHostFree(h_alp_b);
        if (h_giveup) (void)hipHostFree(h_giveup);
        if (h_hash) (void)hipHostFree(h_hash);
        for (void* p : allocs) (void)hipFree(p);
        (void)hipHostFree(h_src); (void)hipHostFree(h_token); (void)hipHostFree(h_top2);
        if (h_sel) (void)hipHostFree(h_sel);
        (void)hipHostFree(h_slots); (void)hipHostFree(h_tok_b);
        if (h_head_src) (void)hipHostFree(h_head_src);
        if (bf_host.src) (void)hipHostFree(bf_host.src);
        if (h_cfeed) (void)hipHostFree(h_cfeed);
        if (h_cslots) (void)hipHostFree(h_cslots);
        if (bf_host.val) (void)hipHostFree(bf_host.val);
        if (bf_host_alp) (void)hipHostFree(bf_host_alp);
        if (h_draft) (void)hipHostFree(h_draft);
        if (h_vctl) (void)hipHostFree(h_vctl);
        if (h_pen_rows) (void)hipHostFree(h_pen_rows);
        if (h_pen_ids) (void)hipHostFree(h_pen_ids);
        (void)hipStreamDestroy(st);
        if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    }

    // ------------------------------------------------------------------------------- weights
    Slot& slot(const char* name) {
        auto it = slots.find(name);
        REQUIRE(it != slots.end(), std::string("unknown tensor: ") + name);
        return it->second;
    }
    void synth_tensor(const char* name, uint64_t seed_t, float hw, float base) override {
        Slot& s = slot(name);
        before_weight_write("svln_synth_tensor");
        launch_synth<T>(st, s.dst, s.ld, s.rows, s.cols, s.map, seed_t, hw, base);
        s.filled = true;
        after_weight_write(s);
    }
    // The two hooks of every weight write (svln_synth_tensor, svln_set_tensor).  Before: a turn in flight or a pending group was computed
    // partly with the old weights, so the write is refused by name before anything changes.  After: everything the engine derives from
    // the written tensor follows it, on the engine stream behind the write -- the 12-bit packed copy, the e4m3 / MXFP4 copies of the
    // matrix if they are built (into the same buffers: the pointers stay, so captured graphs stay valid), and the feature cache, whose
    // entries are features of the old vision tower / projector.  Nothing on a turn's launch path reads a flag set here.
    void before_weight_write(const char* who) { refuse(C_WEIGHT_WRITE, who); }
    void after_weight_write(const Slot& s) {
        p12_encode(s.dst);
        requantise(s.dst);
        if (s.vision) for (auto& e : fc_entries) e.used = false;
    }
    // the LLM matrices that svln_set_fp8_decode / svln_set_fp8_gemm (Q8) and svln_set_mxfp4_decode / svln_set_mxfp4_batched (Q4) copy; a
    // canonical tensor is a row range of one of them (q | k | v fused, gate / up interleaved), and the row scales / block scales are per
    // row, so the whole matrix is quantised again: the bytes of the untouched rows come out as they were
    struct QMat { const T* w; int64_t rows; int cols; Q8* q8; Q4* q4; };
    std::vector<QMat> qmats;
    void requantise(const void* dst) {
        if (!fp8_built && !mx4_built) return;
        for (const QMat& m : qmats) {
            const char* lo = (const char*)m.w; const char* hi = lo + (size_t)m.rows * m.cols * sizeof(T);
            if ((const char*)dst < lo || (const char*)dst >= hi) continue;
            if (fp8_built) launch_quant_fp8_rows(st, m.w, m.cols, m.q8->q, m.q8->s, m.rows, m.cols);
            if (mx4_built) launch_quant_mxfp4_rows(st, m.w, m.cols, m.q4->q, m.q4->e8, m.rows, m.cols);
        }
    }
    // re-encode the packed copy of the matrix at `dst`, if it has one, on the engine stream (behind the write): the pointers stay, so
    // captured graphs stay valid
    void p12_encode(const void* dst) {
        auto it = p12_of.find(dst);
        if (it == p12_of.end()) return;
        const P12& m = *it->second;
        HIP_CHECK(hipMemsetAsync(m.fb, 0, sizeof(unsigned), st));
        launch_p12_pack_rows(st, m.w, m.cols, m.pk, m.rec, m.fb, m.rows, m.cols);
    }
    void set_tensor(const char* name, const void* data, int dtype, int64_t numel, int on_device) override {
        Slot& s = slot(name);
        REQUIRE(numel == s.rows * s.cols, std::string("size mismatch for ") + name);
        before_weight_write("svln_set_tensor");
        const size_t bytes = (size_t)numel * (dtype == SVLN_F32 ? 4 : 2);
        const void* src = data;
        void* tmp = nullptr;
        if (!on_device) {
            HIP_CHECK(hipMalloc(&tmp, bytes));
            HIP_CHECK(hipMemcpyAsync(tmp, data, bytes, hipMemcpyHostToDevice, st));
            src = tmp;
        }
        launch_convert<T>(st, s.dst, s.ld, s.rows, s.cols, s.map, src, dtype == SVLN_F32);
        after_weight_write(s);
        HIP_CHECK(hipStreamSynchronize(st));
        if (tmp) HIP_CHECK(hipFree(tmp));
        s.filled = true;
    }
    int weights_missing() override {
        int n = 0;
        for (auto& kv : slots) if (!kv.second.filled) { if (!n) g_err = "missing tensor: " + kv.first; ++n; }
        return n;
    }
    void get_tensor_f32(const char* name, float* out, int64_t numel) override {
        Slot& s = slot(name);
        REQUIRE(numel == s.rows * s.cols, "size mismatch");
        std::vector<T> row(s.cols);
        for (int64_t r = 0; r < s.rows; ++r) {
            const int64_t dr = (r / s.map.blk) * (int64_t)s.map.blk * s.map.nint + (int64_t)s.map.phase * s.map.blk + r % s.map.blk;
            HIP_CHECK(hipMemcpy(row.data(), (const T*)s.dst + dr * s.ld, s.cols * sizeof(T), hipMemcpyDeviceToHost));
            for (int k = 0; k < s.cols; ++k) out[r * s.cols + k] = host_to_f32(row[k]);
        }
    }
    static float host_to_f32(float v) { return v; }
    static float host_to_f32(bf16 v) {
        unsigned short b; std::memcpy(&b, &v, 2);
        uint32_t u = (uint32_t)b << 16; float f; std::memcpy(&f, &u, 4); return f;
    }

    // ------------------------------------------------------------------------------- session
    Env& env_at(int env) { REQUIRE(env >= 0 && env < (int)envs.size(), "env out of range"); return envs[env]; }
    void release_pages(Env& e) {
        for (int i = 0; i < e.n_pages; ++i) free_pages.push_back(e.pages[i]);
        e.n_pages = 0;
    }
    // A reset drops the env's turn in the multi-env scheduler, if it has one (submitted, running or finished but not collected): its rows
    // and KV pages are gone, so the job must not reach another batch_step.
    // ... and its pending group (svln_generate_group), whose fork pages go back to the pool
    void reset_env(int env) override { Env& e = env_at(env); cancel_jobs_of(env); drop_group_of(env); release_pages(e); e.n_embeds = 0; e.kv_len = 0; }
    void kv_reset(int env) override { Env& e = env_at(env); cancel_jobs_of(env); drop_group_of(env); release_pages(e); e.kv_len = 0; }
    void drop_group() {
        for (int g = 1; g < MAXB; ++g) {
            for (int p : grp.tail[g]) free_pages.push_back(p);
            grp.tail[g].clear();
        }
        grp.pending = false;
    }
    void drop_group_of(int env) { if (grp.pending && grp.env == env) drop_group(); }
    void refuse_while_group_on(int env, const char* who) {
        REQUIRE(!(grp.pending && grp.env == env), std::string(who) + ": a group turn is pending on this env; choose its continuation with svln_group_select first");
    }
    // Which modes may be on together and which turn forms run under them is ONE table (modes.h): every setter, the weight write and every
    // turn form ask it here, with the state the engine is in, and hold no such rule themselves.  The hot paths keep reading the flags.
    ModeState modes_now() const {
        ModeState s;
        s.set(M_DECODE_GRAPH, use_graph); s.set(M_PERSISTENT, persistent_on); s.set(M_FP8_DECODE, fp8_on); s.set(M_MXFP4_DECODE, mx4_on);
        s.set(M_MXFP4_BATCHED, mx4b_on); s.set(M_FP8_GEMM, fp8_gemm_on); s.set(M_FP8_SCALED, fp8_scaled_on); s.set(M_PACKED, p12_on);
        s.set(M_SPECULATIVE, spec_rows > 0); s.set(M_PREFILL_DRAFT, ride_on); s.set(M_BATCH_DRAFT, bdraft_on);
        s.set(M_SCORES, scores_on); s.set(M_TOPK, topk > 0); s.set(M_ENTROPY, ent_on); s.set(M_SAMPLING, smp_on); s.set(M_TRUNCATION, trunc_k > 0);
        s.set(M_ALLOWED, allow_on); s.set(M_PENALTY, rep_penalty != 1.0f);
        for (int k = 0; k < MAXB; ++k) s.set(M_JOBS, jobs[k].used);
        s.set(M_GROUP, grp.pending); s.group_env = grp.env;
        return s;
    }
    // who: the name the message begins with, where it is not the caller's own; part: see ModeRule
    void refuse(Caller caller, const char* who = nullptr, bool no_change = false, int part = MODE_ALL_PARTS) const {
        const std::string m = mode_refusal(caller, modes_now(), who ? who : CALLER_NAME[caller], no_change, part);
        REQUIRE(m.empty(), m);
    }
    // the small lines every turn form shares: the results of the last single-env turn, the phase timers (events v0 v1 p0 p1 d1 of ph_ev,
    // read after a synchronisation), the check of the ids a synchronisation read
    void invalidate_last_results() { last_scores_valid = false; last_alp_valid = false; last_topk_valid = false; last_ent_valid = false; }
    void add_phase(int k, int ev_from, int ev_to) { float t = 0.f; HIP_CHECK(hipEventElapsedTime(&t, ph_ev[ev_from], ph_ev[ev_to])); ph_ms[k] += t; }
    void settle_vision() { if (vision_pending) { add_phase(0, 0, 1); vision_pending = false; } }
    void require_finite_tokens(const int* tok, int n) {
        for (int k = 0; k < n; ++k)
            REQUIRE(tok[k] >= 0 && tok[k] < V, "non-finite logits: the arg-max found no finite value (check the weights / fp8 scales)");
    }
    int kv_free_pages() override { return (int)free_pages.size(); }
    void env_state(int env, int32_t* n_embeds, int32_t* kv_len) override { Env& e = env_at(env); *n_embeds = e.n_embeds; *kv_len = e.kv_len; }
    void ensure_pages(Env& e, int positions) {      // pages covering [0, positions)
        const int need = (positions + PAGE - 1) / PAGE;
        REQUIRE(need <= pages_per_env, "sequence exceeds max_positions");
        if (need <= e.n_pages) return;
        const int first = e.n_pages;
        while (e.n_pages < need) {
            REQUIRE(!free_pages.empty(), "KV page pool exhausted");
            e.pages[e.n_pages++] = free_pages.back();
            free_pages.pop_back();
        }
        HIP_CHECK(hipMemcpyAsync(e.d_pages + first, e.pages.data() + first, (e.n_pages - first) * sizeof(int), hipMemcpyHostToDevice, st));
    }

    // ------------------------------------------------------------------------------- vision
    GemmArgs gemm_args(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* res, int ldr,
                       int res_mod, int M, int N, int K, int epi) {
        GemmArgs a; a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.bias = bias; a.res = res; a.ldr = ldr;
        a.res_mod = res_mod; a.M = M; a.N = N; a.K = K; a.epi = epi; a.ws = gemm_ws; a.ws_elems = gemm_ws_elems; a.nsplit = 1;
        a.zeros = zero_line; a.force_cfg = 0; a.force_split = 0; a.norm_w = nullptr; a.norm_out = nullptr; a.norm_eps = 0.0f; a.norm_b = nullptr;
        a.a_scale = nullptr; a.w_scale = nullptr; a.rope = nullptr; a.vitpack = nullptr; return a;
    }
    AttnArgs vit_attn_args(const void* q, int ld, int F, void* out, int o_stride) {
        AttnArgs a; std::memset(&a, 0, sizeof(a));
        a.Q = q; a.q_stride = ld; a.O = out; a.o_stride = o_stride; a.Kpool = vkpool; a.Vpool = vvpool; a.page_table = nullptr;
        a.n_kv_total = F * vheads; a.hpf = vheads; a.G = 1; a.T = S; a.P = 0; a.kv_len = S; a.dyn_kv_len = nullptr;
        a.scale = 1.0f / sqrtf((float)vhd); a.causal = 0; a.nsplit = 1; a.tiles_per_split = vtiles; a.part = attn_part; a.rows_pad = 0;
        // one frame = 6 row blocks x 16 heads = 96 workgroups of the plain kernel: too few to fill the chip
        const int wgs = ((S + 127) / 128) * F * vheads, rows_pad = ((S + 127) / 128) * 128;
        // (measured: 6 splits are slower than 3 -- the fp32 partials double -- and unsplit is 35 us against 18 + 8 for split + combine)
        // one frame, head_dim 72: the key split stays inside the workgroup (key groups merged through LDS): 14.3 us against 15.6 + 7.4
        if (wgs < 192 && vtiles >= 6 && vhd == 72) { a.key_groups = attn_key_groups<T>(72); return a; }
        // (other head dims)
        if (wgs < 192 && vtiles >= 6 && (size_t)3 * F * vheads * rows_pad * (vhd + ATTN_PART_PAD) <= attn_part_elems) {
            a.nsplit = 3; a.tiles_per_split = (vtiles + 2) / 3; a.rows_pad = rows_pad;
        }
        return a;
    }
    void vit_attention(const void* qkv_buf, int ld, int F, void* out, int o_stride, bool packed = false) {
        if (!packed) launch_vit_kv_pack<T>(st, qkv_buf, ld, vkpool, vvpool, F, S, vheads, vhd);
        AttnArgs a = vit_attn_args(qkv_buf, ld, F, out, o_stride);
        launch_attention<T>(st, a, vhd, 4);
        if (a.nsplit > 1) launch_attention_combine<T>(st, a, vhd);
    }
    // q|k|v product of one SigLIP layer on the normed rows x [F*S][Hv] -> qkv_out [F*S][3 Hv] and its attention -> attn_out [F*S][o_stride]
    // (siglip_encoder.py:197-232).  The product also packs the K / V^T pages where its launch can (one frame: the split-K reduce or the
    // tile epilogue), else vit_attention packs them.  Returns the writer of the pages (launch_gemm's vit_packer: 0, 1 or 2).
    // run_vit and op_vit_qkv_attention run this member; force_split (tests, GemmArgs::force_split) is 0 on the engine's path.
    int vit_qkv_attention(const VLayer& L, const T* x, int F, T* qkv_out, T* attn_out, int o_stride, int force_split = 0) {
        GemmArgs aq = gemm_args(x, Hv, L.qkv_w, Hv, qkv_out, 3 * Hv, L.qkv_b, nullptr, 0, 0, F * S, 3 * Hv, Hv, EPI_NONE);
        aq.force_split = force_split;
        const VitPackArgs vpk{vkpool, vvpool, F, S, vheads, vhd};
        aq.vitpack = &vpk;
        int packer = 0;
        const bool packed = launch_gemm<T>(st, aq, &packer);
        vit_attention(qkv_out, 3 * Hv, F, attn_out, o_stride, packed);
        return packer;
    }
    // SigLIP tower + projector + pool on F frames of `pixbuf` (fp32 [F,3,S,S]) -> dst [F*otok][H]
    void run_vit(const float* pixbuf, int F, T* dst) {
        const int M = F * S;
        // SigLipVisionEmbeddings (siglip_encoder.py:169-174): patch GEMM + bias + position embedding
        launch_patchify<T>(st, pixbuf, patches, F, c.v_image, c.v_patch, kp);
        launch_gemm<T>(st, gemm_args(patches, kp, patch_w, kp, vx, Hv, patch_b, pos_emb, Hv, S, M, Hv, kp, EPI_NONE));
        bool vn_ready = false;                      // vn already holds ln1(vx) (written by the previous layer's fc2 epilogue)
        for (int i = 0; i < c.v_layers; ++i) {      // SigLipEncoderLayer (siglip_encoder.py:269-305)
            const VLayer& L = vl[i];
            if (!vn_ready) launch_layernorm<T>(st, vx, L.ln1_w, L.ln1_b, vn, M, Hv, c.v_eps);
            vit_qkv_attention(L, vn, F, vqkv, vattn, Hv);
            // out_proj / fc2 run split-K at one frame: their slab reduce also emits the following LayerNorm
            GemmArgs ao = gemm_args(vattn, Hv, L.out_w, Hv, vx, Hv, L.out_b, vx, Hv, 0, M, Hv, Hv, EPI_NONE);
            ao.norm_w = L.ln2_w; ao.norm_b = L.ln2_b; ao.norm_out = vn; ao.norm_eps = c.v_eps;
            if (!launch_gemm<T>(st, ao)) launch_layernorm<T>(st, vx, L.ln2_w, L.ln2_b, vn, M, Hv, c.v_eps);
            launch_gemm<T>(st, gemm_args(vn, Hv, L.fc1_w, Hv, vh, Iv, L.fc1_b, nullptr, 0, 0, M, Iv, Hv, EPI_GELU_TANH));
            GemmArgs a2 = gemm_args(vh, Iv, L.fc2_w, Iv, vx, Hv, L.fc2_b, vx, Hv, 0, M, Hv, Iv, EPI_NONE);
            if (i + 1 < c.v_layers) { a2.norm_w = vl[i + 1].ln1_w; a2.norm_b = vl[i + 1].ln1_b; a2.norm_out = vn; a2.norm_eps = c.v_eps; }
            vn_ready = launch_gemm<T>(st, a2);
        }
        // mm_projector (builder.py:41-48) then get_2dPool bilinear 27x27 -> 14x14 (stream_video_vln.py:53-73)
        launch_gemm<T>(st, gemm_args(vx, Hv, proj0_w, Hv, proj_h, H, proj0_b, nullptr, 0, 0, M, H, Hv, EPI_GELU_ERF));
        launch_gemm<T>(st, gemm_args(proj_h, H, proj2_w, H, proj_o, H, proj2_b, nullptr, 0, 0, M, H, H, EPI_NONE));
        launch_pool<T>(st, proj_o, dst, tap_idx, tap_w, F, side, oside, H);
    }

    // Optional memoisation of pooled frame features: the reference re-encodes the
    // num_history memory frames through the ViT at every window restart (stream_video_vln.py:104); the same pixels through
    // the same frozen weights give the same features, so frames are keyed by a 128-bit content hash and reused.  OFF by
    // default (svln_set_feature_cache).
    struct CacheEntry { unsigned long long a, b; uint64_t stamp; bool used; };
    int fc_cap = 0; T* fc_store = nullptr; std::vector<CacheEntry> fc_entries; uint64_t fc_clock = 0;
    int64_t fc_hits = 0, fc_misses = 0;
    float* pix2 = nullptr; T* feats_stage = nullptr; unsigned long long* d_hash = nullptr; unsigned long long* h_hash = nullptr;
    void set_feature_cache(int cap) override {
        REQUIRE(cap >= 0, "capacity must be >= 0");
        if (cap > 0 && cap != (int)fc_entries.size()) {
            REQUIRE(fc_store == nullptr, "feature cache capacity can be set once");
            fc_store = dalloc<T>((size_t)cap * otok * H);
            fc_entries.assign(cap, CacheEntry{0, 0, 0, false});
            pix2 = dalloc<float>((size_t)c.max_frames * 3 * c.v_image * c.v_image);
            feats_stage = dalloc<T>((size_t)c.max_frames * otok * H);
            d_hash = dalloc<unsigned long long>(2 * c.max_frames);
            HIP_CHECK(hipHostMalloc((void**)&h_hash, 2 * c.max_frames * sizeof(unsigned long long)));
        }
        fc_cap = cap;
        for (auto& e : fc_entries) e.used = false;
    }
    void feature_cache_stats(int64_t* hits, int64_t* misses) override { *hits = fc_hits; *misses = fc_misses; }

    void encode_frames(const float* pixels, int F, int on_device) override {
        REQUIRE(F >= 1 && F <= c.max_frames, "n_frames out of range");
        REQUIRE(weights_missing() == 0, g_err);
        const size_t fwords = (size_t)3 * c.v_image * c.v_image;
        HIP_CHECK(hipEventRecord(ph_ev[0], st));
        HIP_CHECK(hipMemcpyAsync(pix, pixels, F * fwords * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (fc_cap <= 0) {
            run_vit(pix, F, feats);
        } else {
            HIP_CHECK(hipMemsetAsync(d_hash, 0, 2 * F * sizeof(unsigned long long), st));
            launch_frame_hash(st, pix, F, fwords, d_hash);
            HIP_CHECK(hipMemcpyAsync(h_hash, d_hash, 2 * F * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            std::vector<int> slot(F, -1), miss;
            for (int f = 0; f < F; ++f) {
                for (int k = 0; k < fc_cap; ++k)
                    if (fc_entries[k].used && fc_entries[k].a == h_hash[2 * f] && fc_entries[k].b == h_hash[2 * f + 1]) { slot[f] = k; break; }
                if (slot[f] >= 0) { fc_entries[slot[f]].stamp = ++fc_clock; ++fc_hits; }
                else { miss.push_back(f); ++fc_misses; }
            }
            const size_t fbytes = (size_t)otok * H * sizeof(T);
            if (!miss.empty()) {
                for (size_t j = 0; j < miss.size(); ++j)
                    HIP_CHECK(hipMemcpyAsync(pix2 + j * fwords, pix + (size_t)miss[j] * fwords, fwords * sizeof(float), hipMemcpyDeviceToDevice, st));
                run_vit(pix2, (int)miss.size(), feats_stage);
                for (size_t j = 0; j < miss.size(); ++j) {
                    const int f = miss[j];
                    int victim = -1;                                           // free slot, else least recently used
                    for (int k = 0; k < fc_cap; ++k) {
                        bool taken = false;
                        for (int g = 0; g < F; ++g) taken |= slot[g] == k;     // never evict a slot this call still needs
                        if (taken) continue;
                        if (!fc_entries[k].used) { victim = k; break; }
                        if (victim < 0 || fc_entries[k].stamp < fc_entries[victim].stamp) victim = k;
                    }
                    HIP_CHECK(hipMemcpyAsync((char*)feats + (size_t)f * fbytes, (char*)feats_stage + j * fbytes, fbytes, hipMemcpyDeviceToDevice, st));
                    if (victim >= 0) {
                        HIP_CHECK(hipMemcpyAsync((char*)fc_store + (size_t)victim * fbytes, (char*)feats_stage + j * fbytes, fbytes, hipMemcpyDeviceToDevice, st));
                        fc_entries[victim] = CacheEntry{h_hash[2 * f], h_hash[2 * f + 1], ++fc_clock, true};
                        slot[f] = victim;
                    }
                }
            }
            for (int f = 0; f < F; ++f) {
                bool was_miss = false;
                for (int g : miss) was_miss |= g == f;
                if (!was_miss)
                    HIP_CHECK(hipMemcpyAsync((char*)feats + (size_t)f * fbytes, (char*)fc_store + (size_t)slot[f] * fbytes, fbytes, hipMemcpyDeviceToDevice, st));
            }
        }
        HIP_CHECK(hipEventRecord(ph_ev[1], st));
        vision_pending = true;
        n_feat_frames = F;
    }

    // ------------------------------------------------------------------------------- a-1: image preprocess on the GPU
    // SigLipImageProcessor.preprocess (siglip_encoder.py:47-67), bit-exact with Pillow's bicubic (preprocess.hip).  Coefficient tables
    // are built on the host per frame geometry (double precision, Pillow's operation order) and cached on the device.
    struct ResampleTabs { int H, W; ResampleDev dev; uint64_t stamp = 0; std::vector<void*> bufs; };
    std::vector<ResampleTabs> rs_tabs;
    uint8_t* d_rgb = nullptr; size_t d_rgb_cap = 0; float* d_lut = nullptr;
    // pinned staging, double-buffered: call i + 1 copies its frame in while the DMA of call i may still be reading the other buffer
    uint8_t* h_rgb[2] = {nullptr, nullptr}; uint8_t* h_rgb_dev[2] = {nullptr, nullptr}; size_t h_rgb_cap[2] = {0, 0}; hipEvent_t h2d_ev[2] = {nullptr, nullptr}; int h_cur = 0;
    // GPU time of the preprocess calls: a fixed ring of (begin, end) event pairs created with the first call and read back lazily (when the
    // ring wraps, or when the totals are asked for), so that an enqueue-only call neither waits nor creates events -- event creation on
    // the hot path stalls for milliseconds whenever the runtime grows its signal pool
    static constexpr int PP_RING = 16;
    struct EvPair { hipEvent_t a = nullptr, b = nullptr; int frames = 0; };
    EvPair pp_ring[PP_RING]; size_t pp_head = 0, pp_tail = 0;      // pairs [pp_tail, pp_head) are pending
    double pp_ms = 0; int64_t pp_frames = 0;
    void pp_resolve_oldest() {
        EvPair& pr = pp_ring[pp_tail++ % PP_RING];
        float t = 0.f;
        HIP_CHECK(hipEventSynchronize(pr.b));
        HIP_CHECK(hipEventElapsedTime(&t, pr.a, pr.b));
        pp_ms += t; pp_frames += pr.frames;
    }
    void pp_collect() { while (pp_tail < pp_head) pp_resolve_oldest(); }
    void* stream_handle() override { return (void*)st; }
    // Coefficient tables per frame geometry: at most RS_CACHE geometries stay on the device (least recently used one evicted, its buffers
    // reused by hipFree after a stream sync), and a geometry the kernel cannot take is rejected BEFORE anything is uploaded.
    static constexpr int RS_CACHE = 4;
    uint64_t rs_clock = 0;
    const ResampleDev& resample_tabs(int Hh, int Ww) {
        for (auto& t : rs_tabs) if (t.H == Hh && t.W == Ww) { t.stamp = ++rs_clock; return t.dev; }
        const int Sx = c.v_image;
        ResampleAxis ah, av;
        build_resample_table(Ww, Sx, ah);
        build_resample_table(Hh, Sx, av);
        REQUIRE(av.ksize <= 40, "frame too large for the GPU preprocess kernel (more than 40 source rows per output row)");
        REQUIRE(preprocess_lds_bytes(Ww, Sx, av.ksize, ah.ksize) <= (size_t)160 * 1024,
                "frame too large for the GPU preprocess kernel (its source rows of one output row must fit the 160 KiB LDS)");
        if ((int)rs_tabs.size() >= RS_CACHE) {
            HIP_CHECK(hipStreamSynchronize(st));       // no launch may still be reading the evicted tables
            size_t v = 0;
            for (size_t k = 1; k < rs_tabs.size(); ++k) if (rs_tabs[k].stamp < rs_tabs[v].stamp) v = k;
            for (void* p : rs_tabs[v].bufs) (void)hipFree(p);
            rs_tabs.erase(rs_tabs.begin() + v);
        }
        ResampleTabs t; t.H = Hh; t.W = Ww; t.stamp = ++rs_clock;
        auto up = [&](const std::vector<int>& v) {
            int* d = nullptr;
            HIP_CHECK(hipMalloc((void**)&d, v.size() * sizeof(int) + 256));
            t.bufs.push_back(d);
            HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, st));
            return d;
        };
        t.dev.hmin = up(ah.xmin); t.dev.hcnt = up(ah.cnt); t.dev.hk = up(ah.k); t.dev.ks_h = ah.ksize;
        t.dev.vmin = up(av.xmin); t.dev.vcnt = up(av.cnt); t.dev.vk = up(av.k); t.dev.ks_v = av.ksize;
        HIP_CHECK(hipStreamSynchronize(st));          // the host vectors go out of scope
        rs_tabs.push_back(t);
        return rs_tabs.back().dev;
    }
    // Engine-owned pinned frame ring (svln_frame_ring): `slots` frames of height x width x 3 bytes in pinned, device-mapped host memory.
    // A frame handed to svln_preprocess_frames* that lies INSIDE the ring is read by the upload kernel where it is -- no staging copy on
    // the host (921 KB per 640x480 frame).  The camera / simulator side writes frames into the slots; a slot may be rewritten once the
    // upload that last read it has run (svln_frame_ring_wait).
    uint8_t *ring_host = nullptr, *ring_dev = nullptr; size_t ring_stride = 0, ring_frame_bytes = 0; int ring_slots = 0;
    std::vector<hipEvent_t> ring_ev; std::vector<char> ring_pending;
    void frame_ring(int slots, int height, int width, uint8_t** base, int64_t* stride) override {
        REQUIRE(slots >= 1 && height >= 1 && width >= 1, "frame ring: bad geometry");
        REQUIRE(base && stride, "null output pointer");
        HIP_CHECK(hipStreamSynchronize(st));
        for (auto ev : ring_ev) (void)hipEventDestroy(ev);
        ring_ev.clear(); ring_pending.clear();
        if (ring_host) { (void)hipHostFree(ring_host); ring_host = nullptr; ring_dev = nullptr; }
        ring_frame_bytes = (size_t)height * width * 3;
        ring_stride = (ring_frame_bytes + 255) / 256 * 256;            // slots start 256-byte aligned (the upload kernel moves 16-byte granules)
        ring_slots = slots;
        HIP_CHECK(hipHostMalloc((void**)&ring_host, ring_stride * slots + 256));
        HIP_CHECK(hipHostGetDevicePointer((void**)&ring_dev, ring_host, 0));
        ring_ev.resize(slots); ring_pending.assign(slots, 0);
        for (auto& ev : ring_ev) HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        *base = ring_host; *stride = (int64_t)ring_stride;
    }
    void frame_ring_wait(int slot) override {
        REQUIRE(slot >= 0 && slot < ring_slots, "frame ring: no such slot");
        if (ring_pending[slot]) { HIP_CHECK(hipEventSynchronize(ring_ev[slot])); ring_pending[slot] = 0; }
    }
    // device-visible address of a host frame batch that lies inside the ring (16-byte aligned, contiguous), else null
    const uint8_t* ring_lookup(const uint8_t* rgb, size_t bytes, int n) const {
        if (!ring_host || rgb < ring_host || rgb + bytes > ring_host + ring_stride * ring_slots) return nullptr;
        const size_t off = (size_t)(rgb - ring_host);
        if (off % 16 != 0) return nullptr;
        if (n > 1 && ring_stride != ring_frame_bytes) return nullptr;      // padded slots: a multi-frame batch is not contiguous
        return ring_dev + off;
    }
    void ring_mark(const uint8_t* rgb, size_t bytes) {                      // the slots this upload reads: busy until the event fires
        const int s0 = (int)((size_t)(rgb - ring_host) / ring_stride), s1 = (int)((size_t)(rgb - ring_host + bytes - 1) / ring_stride);
        for (int k = s0; k <= s1 && k < ring_slots; ++k) { HIP_CHECK(hipEventRecord(ring_ev[k], st)); ring_pending[k] = 1; }
    }
    // One model turn behind ONE call (SURVEY.md 8b `svln_turn`): encode_rgbd + the KV / embeds bookkeeping of StreamVLNForCausalLM.generate +
    // splice + greedy generation -- svln_encode_frames, svln_kv_reset / svln_reset_env, svln_append_turn, svln_generate in that order.
    // The shared body of every svln_turn_*, up to the generate call (a.env is in range: the caller checked).  `checks` = the form's
    // argument check and refusals, run inside the guard: a refusal of svln_turn, svln_turn_forced or svln_turn_candidates consumes the
    // armed draft.  svln_turn_group and svln_turn_beams refuse BEFORE they call this and pass nothing: their refusals leave the draft armed.
    template <typename Checks>
    void begin_turn(const svln_turn_args& a, Checks checks) {
        try {
            checks();
            encode_frames(a.pixels, a.n_frames, a.pixels_on_device);
            if (a.new_window) kv_reset(a.env);                                  // past_key_values = None (streamvln_eval.py:349)
            if (a.new_episode && envs[a.env].n_embeds != 0) reset_env(a.env);   // curr_t == 0: the env's inputs_embeds start over (stream_video_vln.py:396-401)
            append_turn(a.env, a.ids, a.n_ids, 0, a.n_memory);
        } catch (...) {
            disarm_draft(a.env);          // an armed draft (svln_set_draft) is consumed by this call even when it fails before generating
            throw;
        }
    }
    void begin_turn(const svln_turn_args& a) { begin_turn(a, [] {}); }
    void turn(const svln_turn_args& a, int64_t* out, int cap, int32_t* n_out, int32_t* kv_len) override {
        Env& e = env_at(a.env);
        refuse_while_group_on(a.env, "svln_turn");
        begin_turn(a, [&] { REQUIRE(a.ids && a.n_ids >= 1 && out && n_out, "svln_turn: null / empty argument"); });
        generate(a.env, a.max_new_tokens, a.eos_ids, a.n_eos, out, cap, n_out, false);
        if (kv_len) *kv_len = e.kv_len;
    }
    void preprocess_frames(const uint8_t* rgb, int n, int Hh, int Ww, int on_device, float* out_dev, bool wait) override {
        REQUIRE(rgb && out_dev, "null frame / output pointer");
        REQUIRE(n >= 1 && Hh >= 1 && Ww >= 1, "bad frame geometry");
        REQUIRE((long long)Hh <= 100ll * Ww, "frames taller than 100 x their width are not supported (Pillow >= 12 resizes them vertical-first)");
        const int Sx = c.v_image;
        const size_t bytes = (size_t)n * Hh * Ww * 3;
        if (!d_lut) {
            float lut[256];
            build_normalize_lut(lut, 0.5f, 0.5f);      // image_mean = image_std = 0.5 (siglip_encoder.py:35)
            d_lut = dalloc<float>(256);
            HIP_CHECK(hipMemcpy(d_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
            for (int i = 0; i < 2; ++i) HIP_CHECK(hipEventCreate(&h2d_ev[i]));
            for (auto& pr : pp_ring) { HIP_CHECK(hipEventCreate(&pr.a)); HIP_CHECK(hipEventCreate(&pr.b)); }
        }
        const ResampleDev tabs = resample_tabs(Hh, Ww);       // (by value: a later geometry may evict the cache entry)
        if (d_rgb_cap < bytes + 64) {
            HIP_CHECK(hipStreamSynchronize(st));
            if (d_rgb) HIP_CHECK(hipFree(d_rgb));
            d_rgb = nullptr; d_rgb_cap = 0;
            HIP_CHECK(hipMalloc((void**)&d_rgb, bytes + 256));
            d_rgb_cap = bytes + 256;
        }
        if (pp_head - pp_tail == PP_RING) pp_resolve_oldest();      // 16 calls old: finished long ago
        EvPair& pr = pp_ring[pp_head++ % PP_RING];
        pr.frames = n;
        HIP_CHECK(hipEventRecord(pr.a, st));
        if (on_device) {
            HIP_CHECK(hipMemcpyAsync(d_rgb, rgb, bytes, hipMemcpyDeviceToDevice, st));
        } else if (const uint8_t* rd = ring_lookup(rgb, bytes, n)) {
            launch_upload(st, rd, d_rgb, bytes);             // the frame sits in the engine's pinned ring: read it where it is
            ring_mark(rgb, bytes);
        } else {
            const int b = h_cur; h_cur ^= 1;
            if (h_rgb_cap[b] < bytes) {
                HIP_CHECK(hipStreamSynchronize(st));
                if (h_rgb[b]) HIP_CHECK(hipHostFree(h_rgb[b]));
                h_rgb[b] = nullptr; h_rgb_cap[b] = 0;
                HIP_CHECK(hipHostMalloc((void**)&h_rgb[b], bytes + 16));
                HIP_CHECK(hipHostGetDevicePointer((void**)&h_rgb_dev[b], h_rgb[b], 0));
                h_rgb_cap[b] = bytes;
            }
            HIP_CHECK(hipEventSynchronize(h2d_ev[b]));   // the DMA that last read this staging buffer (two calls ago) has finished
            std::memcpy(h_rgb[b], rgb, bytes);           // pinned, device-mapped staging: the upload below is one kernel reading it over PCIe
            launch_upload(st, h_rgb_dev[b], d_rgb, bytes);
            HIP_CHECK(hipEventRecord(h2d_ev[b], st));
        }
        launch_preprocess(st, d_rgb, out_dev, n, Hh, Ww, Sx, tabs, d_lut);
        LAUNCH_CHECK("preprocess");
        HIP_CHECK(hipEventRecord(pr.b, st));
        // wait: out_dev (the caller's tensor) is complete on return.  Otherwise the work is only enqueued on the engine's stream (the
        // frame bytes have been consumed): svln_encode_frames on the same engine is ordered behind it, any other stream must wait on
        // svln_engine_stream() itself.
        if (wait) HIP_CHECK(hipEventSynchronize(pr.b));
    }
    void preprocess_time(double* ms, int64_t* frames, int reset) override {
        pp_collect();
        *ms = pp_ms; *frames = pp_frames;
        if (reset) { pp_ms = 0; pp_frames = 0; }
    }

    // ------------------------------------------------------------------------------- splice
    hipEvent_t src_ev = nullptr; bool src_pending = false;      // h_src (pinned splice descriptor) is still being read by the last upload
    void append_turn(int env, const int64_t* ids, int n, int frame_base, int n_memory) override {
        Env& e = env_at(env);
        refuse_while_group_on(env, "svln_append_turn");
        if (src_pending) { HIP_CHECK(hipEventSynchronize(src_ev)); src_pending = false; }
        REQUIRE(frame_base >= 0 && n_memory >= 0 && frame_base + n_memory <= n_feat_frames, "n_memory exceeds encoded frames");
        // rows of this turn, then the reference's per-turn truncation (new_input_embeds[:tokenizer_model_max_length], stream_video_vln.py:241-244),
        // then the capacity check of the accumulated sequence (max_positions is this engine's buffer size; the reference has no such cap)
        int img = frame_base + n_memory, mem_used = 0;
        const int cap = c.max_positions - e.n_embeds;
        const size_t lim = turn_row_limit > 0 ? (size_t)turn_row_limit : (size_t)1 << 30;
        std::vector<int> src;
        for (int k = 0; k < n && src.size() < lim; ++k) {
            const int64_t t = ids[k];
            if (t == IMAGE_TOKEN) {
                REQUIRE(img < n_feat_frames, "more <image> tokens than encoded frames");
                for (int j = 0; j < otok; ++j) src.push_back(-(1 + img * otok + j));
                ++img;
            } else if (t == MEMORY_TOKEN) {
                REQUIRE(n_memory > 0 && mem_used == 0, "<memory> token without (or with repeated) memory frames");
                const int nm = n_memory * otok;
                if (prune_keep > 0 && prune_keep < nm) {          // opt-in: keep the prune_keep least-average memory tokens, in order
                    run_memory_prune(feats + (size_t)frame_base * otok * H, nm, prune_keep);
                    for (int j = 0; j < prune_keep; ++j) src.push_back(-(1 + frame_base * otok + h_sel[j]));
                } else {
                    for (int j = 0; j < nm; ++j) src.push_back(-(1 + frame_base * otok + j));
                }
                mem_used = 1;
            } else {
                REQUIRE(t >= 0 && t < V, "token id out of range");
                src.push_back((int)t);
            }
        }
        if (src.size() > lim) src.resize(lim);
        REQUIRE((int)src.size() <= cap, "inputs_embeds exceeds max_positions");
        const int rows = (int)src.size();
        std::memcpy(h_src, src.data(), (size_t)rows * sizeof(int));
        HIP_CHECK(hipMemcpyAsync(d_src, h_src, rows * sizeof(int), hipMemcpyHostToDevice, st));
        launch_gather_rows<T>(st, d_src, embed, feats, e.embeds + (size_t)e.n_embeds * H, rows, H);
        if (!src_ev) HIP_CHECK(hipEventCreateWithFlags(&src_ev, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(src_ev, st));       // no stream synchronisation on the hot path: the next call waits for this upload only
        src_pending = true;
        e.n_embeds += rows;
    }

    // ------------------------------------------------------------------------------- LLM
    AttnArgs llm_attn_args(const LLayer& L, const Env& e, const void* q, int ld, void* out, int o_stride, int Tn, int P, int kv_len,
                           bool decode) {
        AttnArgs a; std::memset(&a, 0, sizeof(a));
        a.Q = q; a.q_stride = ld; a.O = out; a.o_stride = o_stride; a.Kpool = L.kpool; a.Vpool = L.vpool; a.page_table = e.d_pages;
        a.n_kv_total = nkv; a.hpf = nkv; a.G = nq / nkv; a.T = Tn; a.P = P; a.kv_len = kv_len; a.scale = 1.0f / sqrtf(128.0f);
        a.part = attn_part; a.rows_pad = 32;
        if (decode) {
            a.causal = 0; a.dyn_kv_len = &d_ctl->kv_len; a.nsplit = nsplit_max; a.tiles_per_split = tiles_per_split;
            a.fuse_rope_append = 1; a.rope_tab = rope_tab; a.dyn_pos = &d_ctl->pos; a.nq_heads = nq; a.skip = &d_ctl->done;
        } else {
            a.causal = 1; a.dyn_kv_len = nullptr; a.nsplit = 1; a.tiles_per_split = pages_per_env;
            // few row blocks (steady turn: 12 x nkv workgroups): split the keys as well so the chip is filled
            const int rows = Tn * a.G, wgs = ((rows + 127) / 128) * nkv, tiles = (kv_len + PAGE - 1) / PAGE;
            // (the ViT's in-workgroup key groups were tried here as well -- 96 workgroups of 4 groups x 2 waves under a 2-way grid split, K
            //  prefetched in registers: steady prefill 9.00 against 9.01-9.03 ms per turn in two alternating rounds, +0.15-0.19 without the
            //  grid split; not kept)
            if (rows <= PREFILL_SPLIT_ROWS && wgs < 128 && tiles >= 4) {
                int ns = (256 + wgs - 1) / wgs;
                if (ns > 8) ns = 8;
                if (ns > tiles / 2) ns = tiles / 2;
                if (ns > 1) { a.nsplit = ns; a.tiles_per_split = (tiles + ns - 1) / ns; a.rows_pad = PREFILL_SPLIT_ROWS; }
            }
        }
        return a;
    }

    // rows [off, off + Tn) of the prefill batch belong to env e at positions P..; the last n_draft of them are draft rows (a ride)
    struct Seg { Env* e; int P, Tn, off; int n_draft = 0; };
    RopeKvArgs rope_kv_args(const LLayer& L, const Seg& g) {
        RopeKvArgs r; r.qkv = qkv + (size_t)g.off * qkv_dim; r.ld = qkv_dim; r.Kpool = L.kpool; r.Vpool = L.vpool; r.rope_tab = rope_tab;
        r.nq = nq; r.nkv = nkv; r.dyn_pos = nullptr; r.page_table = g.e->d_pages; r.T = g.Tn; r.P = g.P;
        return r;
    }
    // q|k|v product of the M prefill rows (xn -> qkv) of layer L.  One env's turn alone in the batch (`single`): the product's split-K
    // reduce also ropes q / k and appends k / v to the env's pages -- returns true when it did; otherwise every segment is roped and
    // appended by prefill_rope_append.  op_llm_qkv_rope runs these same two members.
    bool prefill_qkv(const LLayer& L, int M, const Seg* single) {
        GemmArgs aq = gemm_args(xn, H, L.qkv_w, H, qkv, qkv_dim, L.qkv_b, nullptr, 0, 0, M, qkv_dim, H, EPI_NONE);
        RopeKvArgs r0;
        if (single) { r0 = rope_kv_args(L, *single); aq.rope = &r0; }
        return llm_gemm(aq, L.qkv8);
    }
    // The candidate rows folded into a prefill (svln_generate_candidates_folded): the last S * rows rows of the batch are S sequences x
    // `rows` row slots that branch off the ONE segment's last position, fed the ids `feed` (slot g rows + j = F_g[j], pad slots id 0);
    // slots[g] = {table g, first position, row count}, kv_max as a scoring pass's.  The segment's k / v rows of logical page mirror_page
    // also go to the n_mirror physical pages mirror_dst lists (a device array): the forks' private copies of the prompt's last page.
    struct Fold { const int* feed; const DecodeSlot* slots; int S, rows, kv_max, mirror_page; const int* mirror_dst; int n_mirror; };
    void prefill_rope_append(const LLayer& L, const Seg& g, const Fold* fold = nullptr) {
        RopeKvArgs r = rope_kv_args(L, g);
        if (fold) { r.mirror_page = fold->mirror_page; r.mirror_dst = fold->mirror_dst; r.n_mirror = fold->n_mirror; }
        launch_rope_kv<T>(st, r);
    }
    // Qwen2DecoderLayer stack (modeling_qwen2.py:269-299) over the concatenated new rows of one or several envs:
    // the dense products run once on all rows; RoPE + KV append and attention run per env (own pages / positions).
    // n_dec > 0 (mixed iteration of the multi-env scheduler): rows [0, n_dec) are single-token decode rows of n_dec other envs
    // (x already holds their token embeddings, d_slots their page tables / positions); they share every dense product with the
    // prefill rows and run the batched decode attention (fused RoPE + KV append) instead of the per-segment prefill attention.
    // Seg.n_draft > 0 (a ride): the segment's last n_draft rows are not rows of the env's embeds but token embeddings of draft ids, gathered
    // here; RoPE, KV append and the causal attention treat them as the next positions of the same sequence.  n_ragged = 0
    // (svln_set_prefill_draft; one env alone in the batch): the ids are d_draft[0 .. n_draft).  n_ragged > 0 (svln_set_batch_draft): the
    // draft rows of all segments are the n_ragged (row, id) pairs of d_ride_list, written by one launch.
    // fold != null (one segment at row 0, no decode rows): rows [M - S rows, M) are the Fold's candidate rows.  They share every dense
    // product; the q|k|v product leaves RoPE and append to launch_rope_kv (mirror form) for the segment and to the batched verify
    // attention for the candidate rows, which reads q|k|v and writes its output Tn rows into the buffers.
    void prefill_rows(const std::vector<Seg>& segs, int M, int n_dec = 0, int n_ragged = 0, const Fold* fold = nullptr) {
        const int qd = nq * 128;
        const int row0 = fold ? M - fold->S * fold->rows : M;        // the first candidate row
        REQUIRE(!fold || (segs.size() == 1 && n_dec == 0 && n_ragged == 0 && segs[0].off == 0 && segs[0].Tn == row0), "prefill_rows: a fold rides one segment");
        for (const Seg& g : segs) {
            HIP_CHECK(hipMemcpyAsync(x + (size_t)g.off * H, g.e->embeds + (size_t)g.P * H, (size_t)(g.Tn - g.n_draft) * H * sizeof(T), hipMemcpyDeviceToDevice, st));
            if (g.n_draft > 0 && n_ragged == 0)
                launch_gather_rows<T>(st, d_draft, embed, feats, x + (size_t)(g.off + g.Tn - g.n_draft) * H, g.n_draft, H);
        }
        launch_gather_rows_ragged<T>(st, d_ride_list, embed, x, n_ragged, H);
        if (fold) launch_gather_rows<T>(st, fold->feed, embed, feats, x + (size_t)row0 * H, M - row0, H);
        bool xn_ready = false;        // xn already holds rmsnorm(x) * in_norm (written by the previous layer's down_proj epilogue)
        const bool taps = layer_taps_on && segs.size() == 1 && n_dec == 0;
        for (int i = 0; i < c.layers; ++i) {
            const LLayer& L = ll[i];
            const bool probing = taps && i == probe_layer;
            if (probing) { probe_copy(0, x, M); probe_rows = M; }
            if (!xn_ready) launch_rmsnorm<T>(st, x, L.in_norm, xn, M, H, c.rms_eps);
            if (probing) probe_copy(6, xn, M);
            const bool roped = prefill_qkv(L, M, segs.size() == 1 && n_dec == 0 && !fold ? &segs[0] : nullptr);
            if (n_dec > 0) decode_attention(batched_decode_attn_args(L, n_dec));
            for (const Seg& g : segs) {
                T* q_g = qkv + (size_t)g.off * qkv_dim;
                if (!roped) prefill_rope_append(L, g, fold);
                AttnArgs a = llm_attn_args(L, *g.e, q_g, qkv_dim, attn + (size_t)g.off * qd, qd, g.Tn, g.P, g.P + g.Tn, false);
                launch_attention<T>(st, a, 128, 4);
                if (a.nsplit > 1) launch_attention_combine<T>(st, a, 128);
            }
            if (fold) {
                AttnArgs a = verify_multi_attn_args(L, fold->S, fold->rows, fold->kv_max, fold->slots);
                a.Q = qkv + (size_t)row0 * qkv_dim; a.O = attn + (size_t)row0 * qd;
                launch_attention_verify_multi<T>(st, a);
            }
            // the split-K reduce of o_proj / down_proj also emits the following RMSNorm when it can (T <= 256 rows)
            GemmArgs ao = gemm_args(attn, qd, L.o_w, qd, x, H, nullptr, x, H, 0, M, H, qd, EPI_NONE);
            ao.norm_w = L.post_norm; ao.norm_out = xn; ao.norm_eps = c.rms_eps;
            if (probing) { probe_copy(2, attn, M); probe_copy(7, qkv, M); }
            if (!llm_gemm(ao, L.o8)) launch_rmsnorm<T>(st, x, L.post_norm, xn, M, H, c.rms_eps);
            if (probing) { probe_copy(3, x, M); probe_copy(4, xn, M); }
            const bool pp = i == 0 && probe_on && M <= 256 && n_dec == 0 && pprobe_used + 2 <= pprobe_ev.size();
            if (pp) HIP_CHECK(hipEventRecord(pprobe_ev[pprobe_used], st));
            llm_gemm(gemm_args(xn, H, L.gu_w, H, hbuf, I, nullptr, nullptr, 0, 0, M, 2 * I, H, EPI_SWIGLU), L.gu8);
            if (pp) { HIP_CHECK(hipEventRecord(pprobe_ev[pprobe_used + 1], st)); pprobe_used += 2; pprobe_rows += M; }
            if (probing) probe_copy(5, hbuf, M);
            GemmArgs ad = gemm_args(hbuf, I, L.down_w, I, x, H, nullptr, x, H, 0, M, H, I, EPI_NONE);
            if (i + 1 < c.layers) { ad.norm_w = ll[i + 1].in_norm; ad.norm_out = xn; ad.norm_eps = c.rms_eps; }
            xn_ready = llm_gemm(ad, L.down8);
            if (taps) {
                HIP_CHECK(hipMemcpyAsync(layer_tap + (size_t)i * H, x + (size_t)(row0 - 1) * H, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
                if (probing) probe_copy(1, x, M);
            }
        }
    }
    // decode-step attention of layer L: one env (its page table, position / kv length in d_ctl) or B envs of the batched step (d_slots).
    // q|k|v rows in qkv (un-roped; RoPE of q / k and the append of k / v^T are fused), output rows in attn.  op_attention_decode runs
    // these same builders and launches.
    AttnArgs decode_attn_args(const LLayer& L, const Env& e) { return llm_attn_args(L, e, qkv, qkv_dim, attn, nq * 128, 1, 0, 0, true); }
    AttnArgs batched_decode_attn_args(const LLayer& L, int B) {
        AttnArgs a = decode_attn_args(L, envs[0]);
        a.page_table = nullptr; a.dyn_kv_len = nullptr; a.dyn_pos = nullptr; a.skip = nullptr;
        a.slots = d_slots; a.batch = B; a.part_bstride = (size_t)nsplit_max * nkv * 32 * (128 + ATTN_PART_PAD);
        return a;
    }
    // verify pass: `rows` = the most query positions a pass carries; this pass's count is d_vctl[1], its first position GenCtl.pos
    AttnArgs verify_attn_args(const LLayer& L, const Env& e, int rows) {
        AttnArgs a = decode_attn_args(L, e);
        a.T = rows; a.dyn_rows = d_vctl + 1;
        return a;
    }
    // a scoring pass of svln_generate_candidates: S sequences of up to `rows` row slots each, d_slots[s] = {table, first position, row count}
    // kv_max: the most keys any sequence of the pass reaches (known on the host: the pass is not captured) -- the grid covers the key
    // splits below it only; the partial layout and the merge do not depend on the number of splits launched
    AttnArgs verify_multi_attn_args(const LLayer& L, int S, int rows, int kv_max, const DecodeSlot* slots = nullptr) {
        AttnArgs a = batched_decode_attn_args(L, S);
        a.T = rows;
        const int tiles = (kv_max + PAGE - 1) / PAGE;
        a.nsplit = std::max(1, std::min(nsplit_max, (tiles + tiles_per_split - 1) / tiles_per_split));
        if (slots) a.slots = slots;
        return a;
    }
    void decode_attention(const AttnArgs& a) {
        launch_attention<T>(st, a, 128, 1);
        launch_attention_combine<T>(st, a, 128);
    }
    void prefill(Env& e, int P, int Tn, int n_draft = 0) {        // Tn rows in all, the last n_draft of them draft rows
        std::vector<Seg> segs{Seg{&e, P, Tn, 0, n_draft}};
        prefill_rows(segs, Tn);
    }

    GemvArgs gemv_args(const void* W, int ldw, const void* xin, const void* norm_w, const void* bias, const void* res, void* y, int N, int K,
                       int epi) {
        GemvArgs a; a.W = W; a.ldw = ldw; a.x = xin; a.norm_w = norm_w; a.eps = c.rms_eps; a.bias = bias; a.res = res; a.y = y; a.N = N; a.K = K;
        a.epi = epi; a.part_val = part_val; a.part_idx = part_idx; a.w8 = nullptr; a.scale = nullptr; a.skip = nullptr; return a;
    }
    GemvArgs with8(GemvArgs a, const Q8& q) { if (fp8_on) { a.w8 = q.q; a.scale = q.s; } return a; }
    GemvArgs with4(GemvArgs a, const Q4& q) { if (mx4_on) { a.w4 = q.q; a.e8 = q.e8; } return a; }
    // the losslessly packed copy (same outputs bit for bit); the e4m3 / MXFP4 modes read their own copies and take precedence
    GemvArgs with12(GemvArgs a, const P12& m) { if (p12_on && !fp8_on && !mx4_on && m.pk) { a.wp = m.pk; a.prec = m.rec; } return a; }
    GemvArgs guarded(GemvArgs a) { a.skip = &d_ctl->done; return a; }      // decode-step launch: no-op once the generation is done
    // ------------------------------------------------------------------------------- the lm_head ("Anatomy of the lm_head")
    // The form the switches ask for.  The setters keep: topk > 0 and ent_on only while scores_on, trunc_k only while smp_on, ent_on with
    // neither -- so head_epi(form) names a kernel (aim refuses otherwise).  A truncated pass runs the candidate form, lists on or off.
    HeadForm head_form_now() const { return HeadForm{scores_on && !smp_on, smp_on, false, topk > 0 || trunc_k > 0, ent_on}; }
    // the head's share of the decode-graph key (GraphSet): the captured launches differ with every term
    int head_graph_key() const { return (scores_on ? 10000 : 0) + (smp_on ? 20000 : 0) + 100000 * topk + (ent_on ? 1000000 : 0); }
    // A view of one set of partial arrays, read when called (the ensure_*_buffers allocate lazily): the single-env set [partials], the
    // batched set [rows][partials], and the 8-entry rows launch_truncate_partials writes ([1][TOPK_C], [SMP_ROWS][TOPK_C])
    struct HeadParts { float* val; int* idx; float* sum; float* raw; float* max; float* cand_val; int* cand_idx; float* ent; };
    HeadParts parts() const { return {part_val, part_idx, part_sum, part_raw, part_max, cand_val, cand_idx, part_ent}; }
    HeadParts parts_b() const { return {part_val_b, part_idx_b, part_sum_b, part_raw_b, part_max_b, cand_val_b, cand_idx_b, part_ent_b}; }
    HeadParts trunc_parts() const { return {tr_val, tr_idx, tr_sum, tr_raw, tr_max, nullptr, nullptr, nullptr}; }
    HeadParts trunc_parts_b() const { return {tr_val_b, tr_idx_b, tr_sum_b, tr_raw_b, tr_max_b, nullptr, nullptr, nullptr}; }
    // where a sampled product of the engine's own switch reads its stream, its draw counter and (optional) the tokens of this turn
    struct Draws { const int *stream, *draw, *count; };
    // aim a product at a set of partials in form f: epi and every array pointer (a kernel reads the arrays of its form only); dr: the
    // sampling scalars are the engine's own too (a test entry has set its own before)
    template <class A> void aim(A& a, const HeadParts& p, HeadForm f, const Draws* dr = nullptr) {
        constexpr bool subset = std::is_same<A, GemvSubsetArgs>::value;
        if (subset) f.topk = f.ent = false;      // one id per partial: the partials are the candidates as they stand, and t = 0
        a.epi = head_epi(f);
        REQUIRE(a.epi >= 0, "lm_head: no kernel carries this combination of scores, sampling, targets, lists and entropies");
        if (dr && f.smp) a.smp = smp_args(dr->stream, dr->draw, dr->count, nullptr, nullptr);
        a.part_val = p.val; a.part_idx = p.idx; a.part_sum = p.sum; a.smp.part_raw = p.raw; a.smp.part_max = p.max;
        if constexpr (!subset) { a.cand_val = p.cand_val; a.cand_idx = p.cand_idx; a.part_ent = p.ent; }
    }
    // the repetition penalty of a generating turn: the single-env flags, or the flag row d_pen_rows[b] of every batch row
    void with_penalty(GemvArgs& a, bool on) { if (on) { a.pen_flags = pen_flags; a.pen = rep_penalty; } }
    template <class A> void with_penalty(A& a, bool on, bool rows) {
        if (on) { a.pen_flags = rows ? pen_flags_b : pen_flags; a.pen_rows = rows ? d_pen_rows : nullptr; a.pen = rep_penalty; }
    }
    // the routing of a head of several rows: one pass of 32-row MFMA tiles from batched_mfma_min rows, else the batched GEMV
    static bool mfma_head_fits(int rows, int N, int K) { return rows >= batched_mfma_min && K % Elt<T>::PER_CHUNK == 0 && (N + 127) / 128 <= 2048; }
    // Where a merge writes.  single: launch_argmax_final on one row (gen: launch_argmax_step, guarded by the done flag; lists and entropy go
    // to row GenCtl::count, the token's penalty flag is set in step_flags); else launch_argmax_final_batched (row_scale: the producer's).  k = 0: no lists.
    struct HeadOut { bool single, gen; int* tok; float* score; int k; int* top_ids; float* top_lp; float* ent; uint8_t* step_flags = nullptr; const float* row_scale = nullptr; };
    HeadOut out_single(bool gen, bool pen, int k) { return {true, gen, d_token, d_scores, k, d_topi, d_topl, d_ent, pen ? pen_flags : nullptr}; }
    HeadOut out_rows(int tok0, int k) { return {false, false, d_tok_b + tok0, d_score_b + tok0, k, d_topi_b + (size_t)tok0 * k, d_topl_b + (size_t)tok0 * k, d_ent_b + tok0}; }
    // What follows every product: the lists' merge (k > 0), the entropy merge (f.ent), then the step / final kernel -- in this order: the
    // step kernel advances GenCtl::count, which the merges index by.  n_part partials per row with c candidates each; c == 1: the partials
    // are the candidates as they stand (the subset product, a truncated row) and there is no part_ent (t = 0).
    void merge_head(const HeadParts& p, int n_part, int c, int rows, HeadForm f, const HeadOut& o) {
        const float *ps = f.lse || f.smp ? p.sum : nullptr, *pr = f.smp ? p.raw : nullptr, *pm = f.smp ? p.max : nullptr;
        const int *row = o.gen ? &d_ctl->count : nullptr, *skip = o.gen ? &d_ctl->done : nullptr;
        if (o.k) launch_topk_merge(st, c == 1 ? (f.smp ? p.max : p.val) : p.cand_val, c == 1 ? p.idx : p.cand_idx, n_part, c, rows, o.k, p.val, p.idx, p.sum, pm, o.top_ids, o.top_lp, row, skip);
        if (f.ent) launch_entropy_merge(st, p.val, p.idx, p.sum, pm, c == 1 ? nullptr : p.ent, n_part, rows, o.ent, row, skip);
        if (o.gen) launch_argmax_step(st, p.val, p.idx, n_part, o.tok, d_top2, d_ctl, d_eos, d_out_ids, o.step_flags, ps, o.score, pr, pm);
        else if (o.single) launch_argmax_final(st, p.val, p.idx, n_part, o.tok, d_top2, ps, o.score, pr, pm);
        else launch_argmax_final_batched(st, p.val, p.idx, n_part, rows, o.tok, ps, o.score, o.row_scale, pr, pm);
    }
    // svln_sampling_truncation, in front of the merge: the product's candidates -> the 8-entry row(s) tr_*, which the final kernel and the
    // lists' merge then read in place of the product's partials (n_part and c become those of the row)
    HeadParts truncate(const HeadParts& p, const HeadParts& tr, int& n_part, int& c, int rows, const Draws& dr, const int* skip) {
        launch_truncate_partials(st, c == 1 ? p.max : p.cand_val, c == 1 ? p.idx : p.cand_idx, n_part, c, rows, trunc_k, trunc_p,
                                 smp_args(dr.stream, dr.draw, dr.count, tr.raw, tr.max), tr.val, tr.idx, tr.sum, skip);
        n_part = TOPK_C; c = 1;
        return tr;
    }
    // the subset product of the engine's own list on its lm_head for B rows (svln_set_allowed_tokens), aimed at p in form f
    GemvSubsetArgs subset_args(const void* xrows, int ldx, int B, const HeadParts& p, HeadForm f, const Draws* dr = nullptr) {
        GemvSubsetArgs a; a.ids = d_allow; a.n = allow_n; a.W = lm_head; a.ldw = H; a.x = xrows; a.ldx = ldx; a.V = V; a.K = H; a.B = B;
        aim(a, p, f, dr); return a;
    }
    // final norm -> hidden tap row -> lm_head arg-max -> d_token  (lm_head on the LAST position only).
    // `gen`: the arg-max also runs one step of the greedy loop on the device (GenCtl: append, EOS / max_new stop, advance the position)
    // and every launch is guarded by the done flag.
    // With `gen` the tap row is GenCtl.count on the device (= tap_row on the host: tokens emitted so far), so the three launches are the
    // same for every decode step and sit at the end of the captured step graph.
    void head(const T* xrow, int tap_row, bool gen) {
        T* tap = hid_tap + (size_t)(tap_row < HID_TAP_ROWS ? tap_row : HID_TAP_ROWS - 1) * H;
        const int* skip = gen ? &d_ctl->done : nullptr;
        if (gen) {
            launch_rmsnorm<T>(st, xrow, final_norm, head_xn, 1, H, c.rms_eps, skip, hid_tap, &d_ctl->count, HID_TAP_ROWS);
            tap = head_xn;
        } else {
            launch_rmsnorm<T>(st, xrow, final_norm, tap, 1, H, c.rms_eps, skip);
        }
        const HeadForm f = head_form_now();
        HeadParts p = parts();
        const bool pen = gen && rep_penalty != 1.0f;
        // svln_set_sampling: stream and draw come from GenCtl on the device (the turn wrote them), so a captured step stays valid
        const Draws dr{&d_ctl->stream, &d_ctl->draw0, &d_ctl->count};
        int n_part = gemv_grid(V), cc = TOPK_C;
        if (allow_on) {
            // svln_set_allowed_tokens: the subset product on the engine-dtype lm_head, one partial per listed id; with the scores on, the
            // normalised row goes to d_alp[count] before the step kernel advances the count
            GemvSubsetArgs sa = subset_args(tap, H, 1, p, f, &dr);
            sa.skip = skip;
            with_penalty(sa, pen, false);
            launch_gemv_subset<T>(st, sa);
            if (scores_on) launch_subset_logprobs(st, f.smp ? p.max : p.val, allow_n, 1, d_alp, gen ? &d_ctl->count : nullptr, skip);
            n_part = allow_n; cc = 1;
        } else {
            GemvArgs a = with12(with4(with8(gemv_args(lm_head, H, tap, nullptr, nullptr, nullptr, nullptr, V, H, EPI_ARGMAX), lm_head8), lm_head4), lm_head12);
            a.skip = skip;
            aim(a, p, f, &dr);
            with_penalty(a, pen);
            launch_gemv<T>(st, a);
        }
        if (trunc_k) p = truncate(p, trunc_parts(), n_part, cc, 1, dr, skip);
        // svln_top_logprobs / svln_token_entropy: the lists / the entropy of this token -> d_topi / d_topl / d_ent [count]
        merge_head(p, n_part, cc, 1, f, out_single(gen, pen, topk));
    }
    // One decode step as a fixed op sequence; every run-time scalar is read from device memory (d_ctl,
    // d_token) so any sub-range [lo, hi) of the sequence can be captured once and graph-replayed.
    // Op ids: 0 = embedding gather, then 6 per layer (qkv GEMV, attention with fused RoPE + KV append, combine, o GEMV,
    // gate/up GEMV, down GEMV); the layer-0 gate/up GEMV is op probe_op().
    static constexpr int OPS_PER_LAYER = 6;
    // Persistent decode layer (svln_set_decode_persistent; decode_layer.hip): per layer the attention launch + ONE launch for everything
    // behind it (merge of the partials, o_proj, gate/up, down_proj, the next layer's q|k|v), instead of six launches.
    bool persistent_on = false; int n_cus = 0;
    unsigned long long* dl_gran[4] = {nullptr, nullptr, nullptr, nullptr}; unsigned* dl_seq = nullptr; unsigned* dl_giveup = nullptr; unsigned* h_giveup = nullptr;
    DecodeLayerArgs layer_args(int i) {
        const LLayer& L = ll[i];
        DecodeLayerArgs a; std::memset(&a, 0, sizeof(a));
        a.part = attn_part; a.nsplit = nsplit_max; a.tiles_per_split = tiles_per_split; a.dyn_kv_len = &d_ctl->kv_len; a.n_kv = nkv; a.Gq = nq / nkv;
        a.o_w = L.o_w; a.post_norm = L.post_norm; a.gu_w = L.gu_w; a.down_w = L.down_w;
        if (i + 1 < c.layers) { a.next_norm = ll[i + 1].in_norm; a.next_qkv_w = ll[i + 1].qkv_w; a.next_qkv_b = ll[i + 1].qkv_b; }
        a.x = x; a.qkv_out = qkv; a.H = H; a.I = I; a.qd = nq * 128; a.qkv_dim = qkv_dim; a.eps = c.rms_eps;
        for (int k = 0; k < 4; ++k) a.gran[k] = dl_gran[k];
        a.seq = dl_seq; a.giveup = dl_giveup; a.skip = &d_ctl->done;
        return a;
    }
    void set_decode_persistent(int enable) override {
        if ((enable != 0) == persistent_on) return;        // nothing changes
        refuse(enable ? C_SET_DECODE_PERSISTENT_ON : C_SET_DECODE_PERSISTENT_OFF);
        HIP_CHECK(hipStreamSynchronize(st));
        if (!enable) { drop_graphs(); persistent_on = false; return; }
        if (!n_cus) { hipDeviceProp_t pr; HIP_CHECK(hipGetDeviceProperties(&pr, device)); n_cus = pr.multiProcessorCount; }
        DecodeLayerArgs a = layer_args(0);
        REQUIRE(decode_layer_supported<T>(a, n_cus), "persistent decode layer: this configuration is not supported (per-CU slices of hidden / inter / q|k|v "
                                                   "must be whole, rows whole KiB, LDS <= 160 KiB)");
        if (!dl_seq) {
            const size_t ng[4] = {(size_t)nq * 128, (size_t)H, (size_t)I, (size_t)H};
            for (int k = 0; k < 4; ++k) dl_gran[k] = dalloc<unsigned long long>(ng[k], true);
            dl_seq = dalloc<unsigned>(64, true);          // [0] = launch counter, [16] = give-up word (own cache lines)
            dl_giveup = dl_seq + 16;
            HIP_CHECK(hipHostMalloc((void**)&h_giveup, 64));
            h_giveup[0] = 0;
            HIP_CHECK(hipStreamSynchronize(st));
        }
        drop_graphs();
        persistent_on = true;
    }
    // diagnostic: ONE persistent launch of `layer` on whatever the buffers hold after the last decode step, with phase stamps per workgroup
    void probe_decode_layer(int layer, unsigned long long* out, int max_wgs, int32_t* n_wgs) override {
        REQUIRE(persistent_on && layer >= 0 && layer < c.layers, "persistent decode layer is off / no such layer");
        unsigned long long* d = nullptr;
        HIP_CHECK(hipMalloc((void**)&d, (size_t)n_cus * 16 * 8));
        HIP_CHECK(hipMemsetAsync(d, 0, (size_t)n_cus * 16 * 8, st));
        DecodeLayerArgs a = layer_args(layer);
        a.skip = nullptr; a.dbg = d;
        launch_decode_layer<T>(st, a, n_cus);
        const int n = n_cus < max_wgs ? n_cus : max_wgs;
        HIP_CHECK(hipMemcpyAsync(out, d, (size_t)n * 16 * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipFree(d));
        *n_wgs = n;
    }
    // svln_op_decode_layer: ONE persistent launch on the caller's buffers (granules, seq and give-up word included: not the engine's)
    void op_decode_layer(const svln_decode_layer_op& q) override {
        REQUIRE(q.o_w && q.post_norm && q.gu_w && q.down_w && q.part && q.kv_len && q.x && q.seq && q.giveup, "null pointer");
        for (int k = 0; k < 4; ++k) REQUIRE(q.gran[k] != nullptr, "null granule buffer");
        const bool has_next = q.next_qkv_w != nullptr;
        REQUIRE(has_next == (q.next_norm != nullptr) && (has_next || !q.next_qkv_b), "next_norm / next_qkv_w come together; a bias needs them");
        REQUIRE(!has_next || q.qkv_out, "null pointer");
        REQUIRE(q.n_q >= 1 && q.n_kv >= 1 && q.n_q % q.n_kv == 0 && q.n_q / q.n_kv <= 32, "heads: n_q a multiple of n_kv, at most 32 q heads per kv head");
        REQUIRE(q.nsplit >= 1 && q.tiles_per_split >= 1 && q.H >= 1 && q.I >= 1 && q.qkv_dim >= 1, "extent");
        DecodeLayerArgs a; std::memset(&a, 0, sizeof(a));
        a.part = q.part; a.nsplit = q.nsplit; a.tiles_per_split = q.tiles_per_split; a.dyn_kv_len = q.kv_len; a.n_kv = q.n_kv; a.Gq = q.n_q / q.n_kv;
        a.o_w = q.o_w; a.post_norm = q.post_norm; a.gu_w = q.gu_w; a.down_w = q.down_w;
        a.next_norm = q.next_norm; a.next_qkv_w = q.next_qkv_w; a.next_qkv_b = q.next_qkv_b;
        a.x = q.x; a.qkv_out = q.qkv_out; a.H = q.H; a.I = q.I; a.qd = q.n_q * 128; a.qkv_dim = q.qkv_dim; a.eps = q.eps;
        for (int k = 0; k < 4; ++k) a.gran[k] = (unsigned long long*)q.gran[k];
        a.seq = q.seq; a.giveup = q.giveup; a.skip = q.skip;
        REQUIRE(q.cus >= 1 && decode_layer_supported<T>(a, q.cus), "persistent decode layer: this configuration is not supported");
        hipDeviceProp_t pr; HIP_CHECK(hipGetDeviceProperties(&pr, device));
        REQUIRE(q.cus <= pr.multiProcessorCount, "persistent decode layer: more workgroups than CUs (all of them must be resident)");
        launch_decode_layer<T>(st, a, q.cus);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    bool persistent_active() const { return persistent_on && !fp8_on && !mx4_on; }       // (the e4m3 / MXFP4 decode weights keep the launched GEMVs)
    int probe_op() const { return persistent_active() ? 3 : 1 + 4; }          // the launch the roofline probe times (layer 0)
    int total_ops() const { return persistent_active() ? 2 + 2 * c.layers : 1 + c.layers * OPS_PER_LAYER; }
    void decode_ops(Env& e, int lo, int hi) {
        const int qd = nq * 128;
        int op = 0;
        auto on = [&](void) { const bool r = op >= lo && op < hi; ++op; return r; };
        if (on()) launch_gather_rows<T>(st, d_token, embed, feats, x, 1, H, &d_ctl->done);
        if (persistent_active()) {
            // op 1: layer 0's q|k|v rows; then per layer: decode attention (RoPE, KV append, per-page partials), the persistent layer
            if (on()) launch_gemv<T>(st, guarded(gemv_args(ll[0].qkv_w, H, x, ll[0].in_norm, ll[0].qkv_b, nullptr, qkv, qkv_dim, H, EPI_NONE)));
            for (int i = 0; i < c.layers; ++i) {
                if (on()) launch_attention<T>(st, decode_attn_args(ll[i], e), 128, 1);
                if (on()) launch_decode_layer<T>(st, layer_args(i), n_cus);
            }
            return;
        }
        for (int i = 0; i < c.layers; ++i) {
            const LLayer& L = ll[i];
            if (on()) launch_gemv<T>(st, guarded(with4(with8(gemv_args(L.qkv_w, H, x, L.in_norm, L.qkv_b, nullptr, qkv, qkv_dim, H, EPI_NONE), L.qkv8), L.qkv4)));
            const AttnArgs a = decode_attn_args(L, e);
            if (on()) launch_attention<T>(st, a, 128, 1);
            if (on()) launch_attention_combine<T>(st, a, 128);
            if (on()) launch_gemv<T>(st, guarded(with4(with8(gemv_args(L.o_w, qd, attn, nullptr, nullptr, x, x, H, qd, EPI_NONE), L.o8), L.o4)));
            if (on()) launch_gemv<T>(st, guarded(with12(with4(with8(gemv_args(L.gu_w, H, x, L.post_norm, nullptr, nullptr, hbuf, 2 * I, H, EPI_SWIGLU), L.gu8), L.gu4), L.gu12)));
            if (on()) launch_gemv<T>(st, guarded(with12(with4(with8(gemv_args(L.down_w, I, hbuf, nullptr, nullptr, x, x, H, I, EPI_NONE), L.down8), L.down4), L.down12)));
        }
    }

    // layer-0 gate/up SwiGLU GEMV with the kernel's own begin/end timestamps
    void probe_launch(Env&) {
        const LLayer& L = ll[0];
        if (persistent_active()) launch_decode_layer<T>(st, layer_args(0), n_cus, probe_ev[probe_used], probe_ev[probe_used + 1]);
        else launch_gemv_timed<T>(st, guarded(with12(with4(with8(gemv_args(L.gu_w, H, x, L.post_norm, nullptr, nullptr, hbuf, 2 * I, H, EPI_SWIGLU), L.gu8), L.gu4), L.gu12)),
                                  probe_ev[probe_used], probe_ev[probe_used + 1]);
        probe_used += 2;
    }
    // graph of: ops [lo, hi) of one decode step (+ the head when hi is the end of the step), then `more` further whole steps
    hipGraphExec_t capture(Env& e, int lo, int hi, int more = 0) {
        return capture_graph([&] {
            decode_ops(e, lo, hi);
            if (hi == total_ops()) head(x, 0, true);       // (the tap row comes from the device)
            for (int k = 0; k < more; ++k) { decode_ops(e, 0, total_ops()); head(x, 0, true); }
        });
    }
    // Capture `body` (launches on `st` only) into an executable graph.  An exception thrown inside the capture (REQUIRE / HIP_CHECK /
    // LAUNCH_CHECK of a launcher) must not leave the stream in capture mode: the capture is ended, the partial graph destroyed and the
    // host-side state a captured product may have left behind (act8_src) reset before the exception travels on.
    template <typename F> hipGraphExec_t capture_graph(F&& body) {
        hipGraph_t g = nullptr; hipGraphExec_t ex = nullptr;
        HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        try {
            body();
        } catch (...) {
            (void)hipStreamEndCapture(st, &g);
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            act8_src = nullptr;
            throw;
        }
        HIP_CHECK(hipStreamEndCapture(st, &g));
        const hipError_t inst = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIP_CHECK(inst);
        return ex;
    }
    void drop_graphs() {
        for (auto& gs : graphs) {
            for (auto& kv : gs.ex) if (kv.second) (void)hipGraphExecDestroy(kv.second);
            gs.ex.clear();
        }
        for (auto& kv : bgraphs) if (kv.second) (void)hipGraphExecDestroy(kv.second);
        bgraphs.clear();
    }
    // Enqueue `steps` decode steps (position, kv length and the fed token live in device memory: GenCtl / d_token); nothing here waits
    // for the GPU.  With hipGraph replay the whole run-ahead batch is ONE graph launch (every launch of a ~175-node graph left a
    // 50-70 us bubble in the kernel trace of round 2: four launches per turn).  The roofline probe times the layer-0 gate/up GEMV of
    // the FIRST decode step of every turn: that step is split around one plain timed launch (same kernel, grid and bytes as the other
    // layers' gate/up GEMVs inside the graph), the remaining steps ride in the second graph.
    void decode_steps(Env& e, int env, int first_tap_row, int steps) {
        if (steps <= 0) return;
        const int n_ops = total_ops();
        const bool probing = probe_on && first_tap_row == 1 && probe_used + 2 <= probe_ev.size();
        if (use_graph) {
            GraphSet& gs = graphs[env];
            const int sk = head_graph_key() + (p12_on ? 40000 : 0);      // the captured head is the plain, the scored or the sampled one; the GEMVs read the packed weights or not
            auto get = [&](int key, int lo, int hi, int more) {
                auto it = gs.ex.find(key);
                if (it == gs.ex.end()) it = gs.ex.emplace(key, capture(e, lo, hi, more)).first;
                return it->second;
            };
            if (!probing) {
                HIP_CHECK(hipGraphLaunch(get(sk + steps, 0, n_ops, steps - 1), st));
            } else {
                HIP_CHECK(hipGraphLaunch(get(sk + 1000, 0, probe_op(), 0), st));
                probe_launch(e);
                HIP_CHECK(hipGraphLaunch(get(sk + 2000 + steps, probe_op() + 1, n_ops, steps - 1), st));
            }
            return;
        }
        for (int k = 0; k < steps; ++k) {
            if (!(probing && k == 0)) {
                decode_ops(e, 0, n_ops);
            } else {
                decode_ops(e, 0, probe_op());
                probe_launch(e);
                decode_ops(e, probe_op() + 1, n_ops);
            }
            head(x, first_tap_row + k, true);
        }
    }

    // ------------------------------------------------------------------------------- multi-env lockstep
    GemvBatchArgs gemvb_args(const void* W, int ldw, const void* xin, int ldx, const void* norm_w, const void* bias, const void* res, int ldr,
                             void* y, int ldy, int N, int K, int epi, int B) {
        GemvBatchArgs a; a.W = W; a.ldw = ldw; a.x = xin; a.ldx = ldx; a.norm_w = norm_w; a.eps = c.rms_eps; a.bias = bias; a.res = res; a.ldr = ldr;
        a.y = y; a.ldy = ldy; a.N = N; a.K = K; a.epi = epi; a.B = B; a.part_val = part_val_b; a.part_idx = part_idx_b; return a;
    }
    // arg-max over W [N][K] . x_b for B rows -> d_tok_b.  B >= 4: one pass of 32-row MFMA tiles with the arg-max in the epilogue (the
    // batched GEMV is dot-product-issue bound from B = 4: 386 us at B = 8 on the full vocabulary); B <= 2: the batched GEMV.
    // pen: the repetition penalty is on and d_pen_rows[0..B) holds the job slot (= flag row) of every batch row
    // svln_set_token_scores: the EPI_ARGMAX_LSE siblings, row b's log-probability -> d_score_b[tok0 + b]
    void argmax_rows(const void* W, int ldw, const T* xrows, int ldx, int N, int K, int B, bool pen, int tok0 = 0) {       // -> d_tok_b[tok0 ..)
        const HeadForm f = head_form_now();
        HeadParts p = parts_b();
        // svln_set_sampling: the EPI_SAMPLE siblings; row b's stream / draw are d_smp[tok0 + b] / d_smp[SMP_ROWS + tok0 + b]
        const Draws dr{d_smp + tok0, d_smp + SMP_ROWS + tok0, nullptr};
        int n = allow_n, cc = TOPK_C;
        if (allow_on && W == (const void*)lm_head) {
            // svln_set_allowed_tokens: the subset product whatever the row count; row b's normalised row -> d_alp_b[tok0 + b]
            GemvSubsetArgs su = subset_args(xrows, ldx, B, p, f, &dr);
            with_penalty(su, pen, true);
            launch_gemv_subset<T>(st, su);
            if (scores_on) launch_subset_logprobs(st, f.smp ? p.max : p.val, allow_n, B, d_alp_b + (size_t)tok0 * allow_n);
            cc = 1;
        } else if (mfma_head_fits(B, N, K)) {
            GemmArgs a = gemm_args(xrows, ldx, W, ldw, nullptr, 0, nullptr, nullptr, 0, 0, B, N, K, EPI_ARGMAX);
            aim(a, p, f, &dr);
            with_penalty(a, pen, true);
            n = launch_gemm_argmax<T>(st, a);
        } else {
            GemvBatchArgs hb = gemvb_args(W, ldw, xrows, ldx, nullptr, nullptr, nullptr, 0, nullptr, 0, N, K, EPI_ARGMAX, B);
            aim(hb, p, f, &dr);
            with_penalty(hb, pen, true);
            launch_gemv_batched<T>(st, hb);
            n = gemv_batched_grid(N, EPI_ARGMAX, B);
        }
        if (trunc_k) p = truncate(p, trunc_parts_b(), n, cc, B, dr, nullptr);
        merge_head(p, n, cc, B, f, out_rows(tok0, topk));
    }
    void head_batched(const T* rows, int B, bool pen = false) {
        launch_rmsnorm<T>(st, rows, final_norm, xn, B, H, c.rms_eps);
        if (mx4b_on && !allow_on) {      // (an allowed list reads the engine-dtype lm_head on every path)
            GemvMx4BatchArgs hb = gemvb4_args(lm_head4, H, xn, H, nullptr, nullptr, 0, nullptr, 0, V, H, EPI_ARGMAX, B);
            with_penalty(hb, pen, true);
            launch_gemv_mx4b(st, hb);
            merge_head(parts_b(), gemv_mx4b_grid(V, EPI_ARGMAX), TOPK_C, B, head_form(EPI_ARGMAX), out_rows(0, 0));
            return;
        }
        argmax_rows(lm_head, H, xn, H, V, H, B, pen);
    }
    // rows argmax_rows is given for n >= 2 head rows of a ride: the 32-row MFMA tiles take any row count from batched_mfma_min up, the
    // batched GEMV 2, 4 or 8 (the pad rows are stale rows of xn: readable, their arg-maxes never read)
    int ride_head_rows(int n) const {
        if (mfma_head_fits(n, V, H)) return n;
        return n <= 2 ? 2 : n <= 4 ? 4 : 8;
    }
    // head of a ride: final norm of the last n rows of the M prefill rows -> xn[0 .. n), lm_head arg-max of every row -> d_tok_b, then
    // the verify step from count = 0 on fed = d_vctl + 8 (fed[i] = draft[i - 1]); its counters are d_vctl[4], [5]
    void ride_head(int M, int n) {
        launch_rmsnorm<T>(st, x + (size_t)(M - n) * H, final_norm, xn, n, H, c.rms_eps);
        argmax_rows(lm_head, H, xn, H, V, H, ride_head_rows(n), false);
        launch_verify_step<T>(st, d_vctl + 8, d_tok_b, d_vctl + 6, n, d_ctl, d_eos, d_out_ids, d_token, xn, hid_tap, H, HID_TAP_ROWS, d_vctl + 4);
    }
    // svln_set_mxfp4_batched: one product of the batched step on the MXFP4 copy `q` of a weight matrix (gemv_mx4b.hip)
    GemvMx4BatchArgs gemvb4_args(const Q4& q, int ldw, const void* xin, int ldx, const void* bias, const void* res, int ldr, void* y, int ldy,
                                 int N, int K, int epi, int B) {
        GemvMx4BatchArgs a; a.q4 = q.q; a.e8 = q.e8; a.ldw = ldw; a.x = xin; a.ldx = ldx; a.bias = bias; a.res = res; a.ldr = ldr; a.y = y; a.ldy = ldy;
        a.N = N; a.K = K; a.epi = epi; a.B = B; a.part_val = part_val_b; a.part_idx = part_idx_b; return a;
    }
    // the batched step with svln_set_mxfp4_batched on: every B takes the same five launches per layer beside the attention (RMSNorm as
    // its own launch, the four projections on gemv_mx4b_kernel), then the MXFP4 lm_head
    void decode_ops_batched_mx4(int B, bool pen) {
        const int qd = nq * 128;
        launch_gather_rows<T>(st, d_tok_b, embed, feats, x, B, H);
        for (int i = 0; i < c.layers; ++i) {
            const LLayer& L = ll[i];
            launch_rmsnorm<T>(st, x, L.in_norm, xn, B, H, c.rms_eps);
            launch_gemv_mx4b(st, gemvb4_args(L.qkv4, H, xn, H, L.qkv_b, nullptr, 0, qkv, qkv_dim, qkv_dim, H, EPI_NONE, B));
            decode_attention(batched_decode_attn_args(L, B));
            launch_gemv_mx4b(st, gemvb4_args(L.o4, qd, attn, qd, nullptr, x, H, x, H, H, qd, EPI_NONE, B));
            launch_rmsnorm<T>(st, x, L.post_norm, xn, B, H, c.rms_eps);
            launch_gemv_mx4b(st, gemvb4_args(L.gu4, H, xn, H, nullptr, nullptr, 0, hbuf, I, 2 * I, H, EPI_SWIGLU, B));
            launch_gemv_mx4b(st, gemvb4_args(L.down4, I, hbuf, I, nullptr, x, H, x, H, H, I, EPI_NONE, B));
        }
        head_batched(x, B, pen);
    }
    // One decode step for B envs (B in {1,2,4,8}; d_slots / d_tok_b already set): every weight matrix is streamed once.
    // B >= 4: the projections run as 32-row MFMA products (gemm.hip CfgSkinny: the weight stream goes through LDS-DMA, the B rows
    // ride along; the batched GEMV is dot-product-issue bound from B = 4 up) and the split-K reduce of o_proj / down_proj also emits
    // the following RMSNorm.  B <= 2: the batched GEMV (HBM-bound there).
    // verify != null (a verify pass of svln_set_speculative, B = spec_rows): the rows are one env's fed tokens (d_vctl + 8) at consecutive
    // positions and the attention is the verify attention on that env's pages; the dense products and the lm_head are the same launches.
    // A pass that uses fewer than B rows (d_vctl[1]) still carries B rows through the products: the unused rows are fed row 0's token,
    // the verify attention writes no output for them, so from o_proj on they hold stale buffer contents -- the products are independent
    // per row and the verify step never reads their arg-maxes.
    // multi != null (a scoring pass of svln_generate_candidates): the rows are multi->S sequences x multi->rows row slots, fed the ids
    // multi->tok; the attention is the batched verify attention on multi->slots; the sweep ends before the head (the caller norms the
    // rows it keeps).
    struct MultiPass { const int* tok; const DecodeSlot* slots; int S; int rows; int kv_max; };
    void decode_ops_batched(int B, bool pen = false, const Env* verify = nullptr, const MultiPass* multi = nullptr) {
        if (mx4b_on) { decode_ops_batched_mx4(B, pen); return; }
        const int qd = nq * 128;
        const bool mfma = B >= batched_mfma_min;
        if (verify) launch_gather_rows<T>(st, d_vctl + 8, embed, feats, x, B, H, &d_ctl->done);
        else launch_gather_rows<T>(st, multi ? multi->tok : d_tok_b, embed, feats, x, B, H);
        bool xn_ready = false;
        for (int i = 0; i < c.layers; ++i) {
            const LLayer& L = ll[i];
            // RMSNorm as its own tiny launch in the batched step (amortised over B envs)
            if (!xn_ready) launch_rmsnorm<T>(st, x, L.in_norm, xn, B, H, c.rms_eps);
            if (mfma) llm_gemm(gemm_args(xn, H, L.qkv_w, H, qkv, qkv_dim, L.qkv_b, nullptr, 0, 0, B, qkv_dim, H, EPI_NONE), L.qkv8);
            else launch_gemv_batched<T>(st, gemvb_args(L.qkv_w, H, xn, H, nullptr, L.qkv_b, nullptr, 0, qkv, qkv_dim, qkv_dim, H, EPI_NONE, B));
            if (verify) launch_attention_verify<T>(st, verify_attn_args(L, *verify, B));
            else if (multi) launch_attention_verify_multi<T>(st, verify_multi_attn_args(L, multi->S, multi->rows, multi->kv_max, multi->slots));
            else decode_attention(batched_decode_attn_args(L, B));
            if (mfma) {
                GemmArgs ao = gemm_args(attn, qd, L.o_w, qd, x, H, nullptr, x, H, 0, B, H, qd, EPI_NONE);
                ao.norm_w = L.post_norm; ao.norm_out = xn; ao.norm_eps = c.rms_eps;
                if (!llm_gemm(ao, L.o8)) launch_rmsnorm<T>(st, x, L.post_norm, xn, B, H, c.rms_eps);
                llm_gemm(gemm_args(xn, H, L.gu_w, H, hbuf, I, nullptr, nullptr, 0, 0, B, 2 * I, H, EPI_SWIGLU), L.gu8);
                GemmArgs ad = gemm_args(hbuf, I, L.down_w, I, x, H, nullptr, x, H, 0, B, H, I, EPI_NONE);
                if (i + 1 < c.layers) { ad.norm_w = ll[i + 1].in_norm; ad.norm_out = xn; ad.norm_eps = c.rms_eps; }
                xn_ready = llm_gemm(ad, L.down8);
            } else {
                launch_gemv_batched<T>(st, gemvb_args(L.o_w, qd, attn, qd, nullptr, nullptr, x, H, x, H, H, qd, EPI_NONE, B));
                launch_rmsnorm<T>(st, x, L.post_norm, xn, B, H, c.rms_eps);
                launch_gemv_batched<T>(st, gemvb_args(L.gu_w, H, xn, H, nullptr, nullptr, nullptr, 0, hbuf, I, 2 * I, H, EPI_SWIGLU, B));
                launch_gemv_batched<T>(st, gemvb_args(L.down_w, I, hbuf, I, nullptr, nullptr, x, H, x, H, H, I, EPI_NONE, B));
            }
        }
        if (multi) return;
        head_batched(x, B, pen);
    }
    // One verify pass of env e, enqueued only (GenCtl, the fed token and the draft live in device memory, so the pass is one fixed launch
    // sequence per (env, rows) and replays as a graph): feed rows -> the batched step's products with the verify attention -> lm_head
    // arg-max of every row (d_tok_b) -> verify step.  Every launch that writes state a later step reads is a no-op once done is set.
    void verify_pass_ops(const Env& e) {
        launch_verify_feed(st, d_ctl, d_token, d_draft, d_vctl, d_vctl + 8, spec_rows, c.max_positions);
        decode_ops_batched(spec_rows, false, &e);           // (its head leaves the final-norm rows in xn)
        launch_verify_step<T>(st, d_vctl + 8, d_tok_b, d_vctl + 1, spec_rows, d_ctl, d_eos, d_out_ids, d_token, xn, hid_tap, H, HID_TAP_ROWS, d_vctl + 2);
    }
    void verify_pass(const Env& e, int env) {
        if (!use_graph) { verify_pass_ops(e); return; }
        GraphSet& gs = graphs[env];
        const int key = 3000 + spec_rows;
        auto it = gs.ex.find(key);
        if (it == gs.ex.end()) it = gs.ex.emplace(key, capture_graph([&] { verify_pass_ops(e); })).first;
        HIP_CHECK(hipGraphLaunch(it->second, st));
    }
    void set_speculative_buffers() {
        if (d_draft) return;
        d_draft = dalloc<int>((size_t)c.max_positions + 8, true);
        d_vctl = dalloc<int>(16, true);
        HIP_CHECK(hipHostMalloc((void**)&h_draft, ((size_t)c.max_positions + 8) * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_vctl, 16 * sizeof(int)));
        for (int k = 0; k < 16; ++k) h_vctl[k] = 0;
        HIP_CHECK(hipStreamSynchronize(st));
    }
    void set_speculative(int rows) override {
        if (rows == spec_rows) return;         // nothing changes
        REQUIRE(rows == 0 || rows == 2 || rows == 4 || rows == 8, "svln_set_speculative: rows must be 0 (off), 2, 4 or 8");
        refuse(rows > 0 ? C_SET_SPECULATIVE_ON : C_SET_SPECULATIVE_OFF, nullptr, false, 0);
        if (rows > 0) {
            REQUIRE(rows * (nq / nkv) <= 32, "svln_set_speculative: rows * (q_heads / kv_heads) must be <= 32 (the verify attention keeps 32 query rows per kv head)");
            refuse(C_SET_SPECULATIVE_ON, nullptr, false, 1);       // a verify pass must compute each row in the numeric scheme of the single step it replaces
            set_speculative_buffers();
        }
        HIP_CHECK(hipStreamSynchronize(st));
        drop_graphs();
        spec_rows = rows;
    }
    bool disarm_draft(int env) {
        if (env < 0 || env >= (int)draft_armed.size() || !draft_armed[env]) return false;
        draft_armed[env] = 0;
        return true;
    }
    // svln_set_sampling.  Refused with the modes whose tokens do not come out of a sampled arg-max (modes.h: SVLN_PLAIN_HEAD_ONLY).
    // Every call, on or off, restarts the draw counters and drops the captured steps (seed and 1 / T are launch scalars).
    void set_sampling(int enable, float temperature, uint64_t seed) override {
        const bool want = enable != 0;
        refuse(want ? C_SET_SAMPLING_ON : C_SET_SAMPLING_OFF, nullptr, false, 0);
        float inv_t = 1.0f;
        if (want) {
            REQUIRE(std::isfinite(temperature) && temperature > 0.0f, "svln_set_sampling: the temperature must be finite and > 0");
            inv_t = 1.0f / temperature;
            REQUIRE(std::isfinite(inv_t), "svln_set_sampling: 1 / temperature overflows fp32");
            refuse(C_SET_SAMPLING_ON, nullptr, false, 1);
        }
        HIP_CHECK(hipStreamSynchronize(st));
        drop_graphs();
        smp_on = want; smp_inv_t = inv_t; smp_seed = want ? seed : 0;
        if (!want) { trunc_k = 0; trunc_p = 1.0f; }      // svln_sampling_truncation is an attribute of the sampling: kept by an "on" call, cleared by "off"
        std::fill(env_draws.begin(), env_draws.end(), 0);
    }
    // svln_sampling_truncation.  An attribute of svln_set_sampling (every mode sampling refuses is thereby unreachable); every refusal
    // comes before any launch or state change.  The draw counters are not touched: one draw per emitted id, truncated or not.
    void sampling_truncation(int top_k, float top_p) override {
        REQUIRE(top_k >= 0 && top_k <= TOPK_C, "svln_sampling_truncation: top_k must be 0 (off) .. 8");
        REQUIRE(top_p > 0.0f && top_p <= 1.0f, "svln_sampling_truncation: top_p must lie in (0, 1]");
        REQUIRE(top_k > 0 || top_p >= 1.0f, "svln_sampling_truncation: top_p < 1 needs top_k = 1 .. 8 (the nucleus is taken over at most 8 listed ids)");
        const bool same = top_k == trunc_k && top_p == trunc_p;
        refuse(top_k ? C_SAMPLING_TRUNCATION_ON : C_SAMPLING_TRUNCATION_OFF, nullptr, same);
        if (same) return;                                      // nothing changes (off stays off whatever the switches are)
        REQUIRE((size_t)H * sizeof(float) <= (size_t)GEMV_ROWS_TOPK_MAX_LDS, "svln_sampling_truncation: the hidden size is too large for the candidate form of the lm_head GEMV");
        HIP_CHECK(hipStreamSynchronize(st));
        if (top_k) ensure_trunc_buffers();
        drop_graphs();           // the captured head is the truncated or the plain sampled one; top_k / top_p are launch scalars
        trunc_k = top_k; trunc_p = top_k ? top_p : 1.0f;
    }
    // TEST-ONLY: truncate_partials_kernel + launch_argmax_final_batched on host candidate rows [B][n_part][c]
    void op_truncate(const float* cv, const int32_t* ci, int B, int n_part, int cc, const OpSample* q, int top_k, float top_p, float* pv,
                     int32_t* pi, float* pr, float* pm, float* ps, int32_t* host_tokens, float* host_logprobs) override {
        REQUIRE(cv && ci && q && pv && pi && pr && pm && ps && host_tokens && host_logprobs, "svln_op_truncate: null pointer");
        REQUIRE(B >= 1 && B <= 32, "svln_op_truncate: 1 <= B <= 32 rows");
        REQUIRE(n_part >= 1 && (cc == 1 || cc == TOPK_C) && (size_t)n_part * cc <= (size_t)2048 * TOPK_C, "svln_op_truncate: n_part >= 1, c = 1 or 8, n_part x c <= 16384");
        REQUIRE(top_k >= 1 && top_k <= TOPK_C, "svln_op_truncate: top_k must be 1 .. 8");
        REQUIRE(top_p > 0.0f && top_p <= 1.0f, "svln_op_truncate: top_p must lie in (0, 1]");
        const size_t nc = (size_t)B * n_part * cc;
        for (size_t i = 0; i < nc; ++i) REQUIRE(ci[i] >= 0, "svln_op_truncate: candidate columns must be >= 0 (0x7FFFFFFF: none)");
        ensure_trunc_buffers();
        SampleArgs sa = op_sample_args(*q, B, tr_raw_b, tr_max_b, true);
        HIP_CHECK(hipMemcpyAsync(cand_val_b, cv, nc * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(cand_idx_b, ci, nc * sizeof(int), hipMemcpyHostToDevice, st));
        launch_truncate_partials(st, cand_val_b, cand_idx_b, n_part, cc, B, top_k, top_p, sa, tr_val_b, tr_idx_b, tr_sum_b);
        merge_head(trunc_parts_b(), TOPK_C, 1, B, head_form(EPI_SAMPLE), out_rows(0, 0));
        const size_t nb = (size_t)B * TOPK_C;
        HIP_CHECK(hipMemcpyAsync(pv, tr_val_b, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(pi, tr_idx_b, nb * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(pr, tr_raw_b, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(pm, tr_max_b, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(ps, tr_sum_b, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        batched_scores_out(B, host_tokens, host_logprobs, "op_truncate");
    }
    // rows [0, n) of the next sampled lm_head pass: job slot order[k] per row (rows beyond n_jobs replay row 0)
    void upload_sample_rows(const int* job_of_row, int n_jobs, int n) {
        for (int k = 0; k < n; ++k) {
            const int env = jobs[job_of_row[k < n_jobs ? k : 0]].env;
            h_smp[k] = env; h_smp[SMP_ROWS + k] = env_draws[env];
        }
        HIP_CHECK(hipMemcpyAsync(d_smp, h_smp, n * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_smp + SMP_ROWS, h_smp + SMP_ROWS, n * sizeof(int), hipMemcpyHostToDevice, st));
    }
    void op_gumbel(uint64_t seed, int stream, int draw, int n0, int count, float* out) override {
        REQUIRE(out && count >= 1 && n0 >= 0 && (int64_t)n0 + count <= (int64_t)1 << 31, "svln_op_gumbel: out, count >= 1, 0 <= n0, n0 + count <= 2^31");
        REQUIRE(stream >= 0 && draw >= 0, "svln_op_gumbel: stream and draw must be >= 0");
        float* d = nullptr;
        HIP_CHECK(hipMalloc((void**)&d, (size_t)count * sizeof(float)));
        launch_gumbel(st, (uint32_t)seed, (uint32_t)(seed >> 32), stream, draw, n0, count, d);
        const hipError_t err = hipMemcpyAsync(out, d, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, st);
        const hipError_t err2 = hipStreamSynchronize(st);
        (void)hipFree(d);
        HIP_CHECK(err); HIP_CHECK(err2);
        LAUNCH_CHECK("op_gumbel");
    }
    // stage the rows of a sampled test op and return its SampleArgs
    SampleArgs op_sample_args(const OpSample& q, int rows, float* raw, float* mx, bool want_logprob) {
        REQUIRE(want_logprob, "the sampled form writes log-probabilities: host_logprob(s) must not be null");
        REQUIRE(q.streams && q.draws, "null pointer");
        REQUIRE(std::isfinite(q.temperature) && q.temperature > 0.0f && std::isfinite(1.0f / q.temperature), "the temperature must be finite and > 0");
        REQUIRE(rows >= 1 && rows <= SMP_ROWS, "rows");
        for (int k = 0; k < rows; ++k) REQUIRE(q.streams[k] >= 0 && q.draws[k] >= 0, "streams and draws must be >= 0");
        HIP_CHECK(hipStreamSynchronize(st));       // (h_smp of an earlier call is no longer being read)
        for (int k = 0; k < rows; ++k) { h_smp[k] = q.streams[k]; h_smp[SMP_ROWS + k] = q.draws[k]; }
        HIP_CHECK(hipMemcpyAsync(d_smp, h_smp, rows * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_smp + SMP_ROWS, h_smp + SMP_ROWS, rows * sizeof(int), hipMemcpyHostToDevice, st));
        SampleArgs a; a.stream = d_smp; a.draw = d_smp + SMP_ROWS; a.count = nullptr; a.inv_t = 1.0f / q.temperature;
        a.seed_lo = (uint32_t)q.seed; a.seed_hi = (uint32_t)(q.seed >> 32); a.part_raw = raw; a.part_max = mx;
        return a;
    }
    // svln_set_token_scores.  Refused with the modes whose tokens do not come out of a scored arg-max (modes.h: SVLN_PLAIN_HEAD_ONLY);
    // off is refused under the top-k lists and the entropies, which ride on the scored partials.
    void set_token_scores(int enable) override {
        const bool want = enable != 0;
        refuse(want ? C_SET_TOKEN_SCORES_ON : C_SET_TOKEN_SCORES_OFF, nullptr, want == scores_on);
        if (want == scores_on) return;         // nothing changes
        HIP_CHECK(hipStreamSynchronize(st));
        drop_graphs();           // the captured lm_head / arg-max launches are the plain or the scored kernels
        scores_on = want;
    }
    // svln_top_logprobs.  The lists ride on the scored kernels' partials, so the scores must be on (and stay on): every mode the scores
    // refuse is thereby unreachable.  Single-env turns, the scheduler's jobs (Job::topk) and svln_generate_batch carry lists; group and
    // candidates turns refuse while k > 0, beam and forced turns run their own head and ignore k (modes.h).
    void top_logprobs(int k) override {
        REQUIRE(k >= 0 && k <= TOPK_C, "svln_top_logprobs: k must be 0 (off) .. 8");
        refuse(k ? C_TOP_LOGPROBS_ON : C_TOP_LOGPROBS_OFF, nullptr, k == topk);
        if (k == topk) return;                 // nothing changes
        REQUIRE(k == 0 || (size_t)H * sizeof(float) <= (size_t)GEMV_ROWS_TOPK_MAX_LDS, "svln_top_logprobs: the hidden size is too large for the candidate form of the lm_head GEMV");
        HIP_CHECK(hipStreamSynchronize(st));
        if (k) ensure_topk_buffers();
        drop_graphs();           // the captured lm_head launch is the sibling with or without candidates; the merge holds k
        topk = k;
    }
    void get_topk(int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) override {
        REQUIRE(last_topk_valid, "svln_get_topk: top-k log-probabilities were off for the last turn (svln_top_logprobs), the last turn was forced, or no turn has run");
        topk_out(last_topi, last_topl, last_topk, ids, logprobs, cap_rows, n_rows, k);
    }
    static void topk_out(const std::vector<int32_t>& ti, const std::vector<float>& tl, int kk, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) {
        const int m = (int)ti.size() / kk;
        for (int q = 0; q < (m < cap_rows ? m : cap_rows) * kk; ++q) { ids[q] = ti[q]; logprobs[q] = tl[q]; }
        *n_rows = m; *k = kk;
    }
    void batch_topk(int slot, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) override {
        REQUIRE(slot >= 0 && slot < MAXB && jobs[slot].used && jobs[slot].finished, "no finished turn in this slot");
        const Job& j = jobs[slot];
        REQUIRE(!j.forced, "svln_batch_topk: this slot holds a forced turn (svln_batch_submit_forced), which produces no lists");
        REQUIRE(j.topk > 0, "svln_batch_topk: top-k log-probabilities were off for this turn (svln_top_logprobs)");
        topk_out(j.topi, j.topl, j.topk, ids, logprobs, cap_rows, n_rows, k);
    }
    void generate_batch_topk(int index, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) override {
        REQUIRE(gb_topk_valid, "svln_generate_batch_topk: top-k log-probabilities were off for the last svln_generate_batch (svln_top_logprobs), or none has run");
        REQUIRE(index >= 0 && index < (int)gb_topi.size(), "svln_generate_batch_topk: no such env index in the last batch");
        topk_out(gb_topi[index], gb_topl[index], gb_topk, ids, logprobs, cap_rows, n_rows, k);
    }
    // svln_token_entropy.  The entropies ride on the scored / sampled kernels' partials, so the scores must be on (and stay on): every
    // mode the scores refuse is thereby unreachable.  The _TOPK epilogues (svln_top_logprobs, svln_sampling_truncation) have no entropy
    // form: refused both ways.  Group, beam, candidate and forced turns carry no entropies: refused while on.
    void token_entropy(int enable) override {
        const bool want = enable != 0;
        refuse(want ? C_TOKEN_ENTROPY_ON : C_TOKEN_ENTROPY_OFF, nullptr, want == ent_on);
        if (want == ent_on) return;            // nothing changes
        HIP_CHECK(hipStreamSynchronize(st));
        if (want) ensure_ent_buffers();
        drop_graphs();           // the captured lm_head launch is the sibling with or without t; the merge is in the graph or not
        ent_on = want;
    }
    static void floats_out(const std::vector<float>& v, float* out, int cap, int32_t* n) {
        const int m = (int)v.size();
        for (int k = 0; k < m && k < cap; ++k) out[k] = v[k];
        *n = m;
    }
    void get_token_entropy(float* out, int cap, int32_t* n) override {
        REQUIRE(last_ent_valid, "svln_get_token_entropy: token entropies were off for the last turn (svln_token_entropy), the last turn was forced, or no turn has run");
        floats_out(last_ent, out, cap, n);
    }
    void batch_entropy(int slot, float* out, int cap, int32_t* n) override {
        REQUIRE(slot >= 0 && slot < MAXB && jobs[slot].used && jobs[slot].finished, "no finished turn in this slot");
        REQUIRE(jobs[slot].ent_on, "svln_batch_entropy: token entropies were off for this turn (svln_token_entropy)");
        floats_out(jobs[slot].ent, out, cap, n);
    }
    void generate_batch_entropy(int index, float* out, int cap, int32_t* n) override {
        REQUIRE(gb_ent_valid, "svln_generate_batch_entropy: token entropies were off for the last svln_generate_batch (svln_token_entropy), or none has run");
        REQUIRE(index >= 0 && index < (int)gb_ent.size(), "svln_generate_batch_entropy: no such env index in the last batch");
        floats_out(gb_ent[index], out, cap, n);
    }
    // TEST-ONLY: entropy_merge_kernel on host partial rows [B][n_part]; pm null: the greedy form, pe null: every t = 0
    void op_entropy_merge(const float* pv, const int32_t* pi, const float* ps, const float* pm, const float* pe, int B, int n_part, float* out) override {
        REQUIRE(B >= 1 && B <= 32, "svln_op_entropy_merge: 1 <= B <= 32 rows");
        REQUIRE(n_part >= 1 && n_part <= 2048, "svln_op_entropy_merge: 1 <= n_part <= 2048 partials per row");
        REQUIRE(pv && pi && ps && out, "svln_op_entropy_merge: null pointer");
        ensure_ent_buffers();
        const size_t nb = (size_t)B * n_part;
        HIP_CHECK(hipMemcpyAsync(part_val_b, pv, nb * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(part_idx_b, pi, nb * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(part_sum_b, ps, nb * sizeof(float), hipMemcpyHostToDevice, st));
        if (pm) HIP_CHECK(hipMemcpyAsync(part_max_b, pm, nb * sizeof(float), hipMemcpyHostToDevice, st));
        if (pe) HIP_CHECK(hipMemcpyAsync(part_ent_b, pe, nb * sizeof(float), hipMemcpyHostToDevice, st));
        launch_entropy_merge(st, part_val_b, part_idx_b, part_sum_b, pm ? part_max_b : nullptr, pe ? part_ent_b : nullptr, n_part, B, d_ent_b);
        HIP_CHECK(hipMemcpyAsync(h_ent_b, d_ent_b, B * sizeof(float), hipMemcpyDeviceToHost, st));
        sync();
        LAUNCH_CHECK("op_entropy_merge");
        for (int b = 0; b < B; ++b) out[b] = h_ent_b[b];
    }
    void get_token_scores(float* out, int cap, int32_t* n) override {
        REQUIRE(last_scores_valid, "svln_get_token_scores: token log-probabilities were off for the last turn (svln_set_token_scores), or no turn has run");
        const int m = (int)last_scores.size();
        for (int k = 0; k < m && k < cap; ++k) out[k] = last_scores[k];
        *n = m;
    }
    void batch_scores(int slot, float* out, int cap, int32_t* n) override {
        REQUIRE(slot >= 0 && slot < MAXB && jobs[slot].used && jobs[slot].finished, "no finished turn in this slot");
        const Job& j = jobs[slot];
        REQUIRE(j.scored, "svln_batch_scores: token log-probabilities were off for this turn (svln_set_token_scores)");
        const int m = (int)j.scores.size();
        for (int k = 0; k < m && k < cap; ++k) out[k] = j.scores[k];
        *n = m;
    }
    void generate_batch_scores(int index, float* out, int cap, int32_t* n) override {
        REQUIRE(gb_scores_valid, "svln_generate_batch_scores: token log-probabilities were off for the last svln_generate_batch (svln_set_token_scores), or none has run");
        REQUIRE(index >= 0 && index < (int)gb_scores.size(), "svln_generate_batch_scores: no such env index in the last batch");
        const int m = (int)gb_scores[index].size();
        for (int k = 0; k < m && k < cap; ++k) out[k] = gb_scores[index][k];
        *n = m;
    }
    // ---- svln_set_allowed_tokens
    void ensure_allow_buffers() {
        if (d_allow) return;
        d_allow = dalloc<int>(ALLOW_MAX, true); d_op_allow = dalloc<int>(ALLOW_MAX, true);
        const size_t rows = (size_t)c.max_positions + 8, rows_b = HEAD_ROWS + MAXB;
        d_alp = dalloc<float>(rows * ALLOW_MAX, true); d_alp_b = dalloc<float>(rows_b * ALLOW_MAX, true);
        HIP_CHECK(hipHostMalloc((void**)&h_alp, rows * ALLOW_MAX * sizeof(float)));
        HIP_CHECK(hipHostMalloc((void**)&h_alp_b, rows_b * ALLOW_MAX * sizeof(float)));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // a list is 1 .. 256 strictly ascending ids of [0, vocab)
    static void check_allowed_list(const std::string& who, const int64_t* ids, int n, int vocab) {
        REQUIRE(n >= 1 && n <= ALLOW_MAX, who + ": the list holds 1 .. 256 ids");
        REQUIRE(ids, who + ": null id list");
        for (int k = 0; k < n; ++k) {
            REQUIRE(ids[k] >= 0 && ids[k] < vocab, who + ": id " + std::to_string((long long)ids[k]) + " is outside the vocabulary");
            REQUIRE(k == 0 || ids[k] > ids[k - 1], who + ": the ids must be strictly ascending (sorted, no duplicates)");
        }
    }
    // Every refusal comes before any launch or state change.  The switch needs no refusal of its own against the other switches: only the
    // lm_head product is swapped, the merge kernels, the verify rule, rides, penalty, sampling and scores see partials as before.
    void set_allowed_tokens(const int64_t* ids, int n) override {
        REQUIRE(n >= 0, "svln_set_allowed_tokens: n must be >= 0 (0 = off)");
        REQUIRE(n <= ALLOW_MAX, "svln_set_allowed_tokens: at most 256 ids");
        REQUIRE(n == 0 || ids, "svln_set_allowed_tokens: null id list with n > 0");
        if (n > 0) check_allowed_list("svln_set_allowed_tokens", ids, n, V);
        refuse(C_SET_ALLOWED_TOKENS);
        std::vector<int> want(n);
        for (int k = 0; k < n; ++k) want[k] = (int)ids[k];
        if (want == allow_ids) return;         // the current list (or off while off): nothing changes
        HIP_CHECK(hipStreamSynchronize(st));
        if (n > 0) {
            ensure_allow_buffers();
            HIP_CHECK(hipMemcpy(d_allow, want.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        }
        drop_graphs();           // the captured lm_head launches hold the list length and the kernel choice
        allow_ids.swap(want); allow_n = n; allow_on = n > 0;
    }
    static void alp_out(const std::vector<float>& v, int n_ids, float* out, int cap, int32_t* n_tokens, int32_t* n_ids_out) {
        const size_t m = v.size();
        for (size_t k = 0; k < m && k < (size_t)cap; ++k) out[k] = v[k];
        *n_tokens = n_ids > 0 ? (int32_t)(m / (size_t)n_ids) : 0; *n_ids_out = n_ids;
    }
    void get_allowed_logprobs(float* out, int cap, int32_t* n_tokens, int32_t* n_ids) override {
        REQUIRE(last_alp_valid, "svln_get_allowed_logprobs: token log-probabilities (svln_set_token_scores) or the allowed list (svln_set_allowed_tokens) were off for the last turn, or no turn has run");
        alp_out(last_alp, last_alp_n, out, cap, n_tokens, n_ids);
    }
    void batch_allowed_logprobs(int slot, float* out, int cap, int32_t* n_tokens, int32_t* n_ids) override {
        REQUIRE(slot >= 0 && slot < MAXB && jobs[slot].used && jobs[slot].finished, "no finished turn in this slot");
        const Job& j = jobs[slot];
        REQUIRE(j.alp_n > 0, "svln_batch_allowed_logprobs: token log-probabilities (svln_set_token_scores) or the allowed list (svln_set_allowed_tokens) were off for this turn");
        alp_out(j.alp, j.alp_n, out, cap, n_tokens, n_ids);
    }
    void generate_batch_allowed_logprobs(int index, float* out, int cap, int32_t* n_tokens, int32_t* n_ids) override {
        REQUIRE(gb_alp_valid, "svln_generate_batch_allowed_logprobs: token log-probabilities (svln_set_token_scores) or the allowed list (svln_set_allowed_tokens) were off for the last svln_generate_batch, or none has run");
        REQUIRE(index >= 0 && index < (int)gb_alp.size(), "svln_generate_batch_allowed_logprobs: no such env index in the last batch");
        alp_out(gb_alp[index], gb_alp_n, out, cap, n_tokens, n_ids);
    }
    // TEST-ONLY: one subset product (scored; sampled when smp.temperature > 0) on caller-given operands and list; the engine's own switches
    // and list are not touched
    void op_subset_argmax(GemvSubsetArgs a, const int64_t* ids, const OpSample& smp, int32_t* host_tokens, float* host_logprobs, float* host_y,
                          float* host_dist) override {
        constexpr int chunk = Elt<T>::PER_CHUNK;
        REQUIRE(a.W && a.x && host_tokens && host_logprobs && host_y && host_dist, "svln_op_subset_argmax: null pointer");
        REQUIRE(a.B >= 1 && a.B <= 32, "svln_op_subset_argmax: B must be 1 .. 32");
        REQUIRE(a.V >= 1, "svln_op_subset_argmax: V must be >= 1");
        REQUIRE(a.K >= chunk && a.K % chunk == 0, "svln_op_subset_argmax: K must be a positive multiple of the 16-byte chunk");
        REQUIRE(a.ldw >= a.K && a.ldx >= a.K, "svln_op_subset_argmax: ldw and ldx must be >= K");
        REQUIRE(a.ldw % chunk == 0 && a.ldx % chunk == 0 && ((size_t)a.W & 15) == 0 && ((size_t)a.x & 15) == 0,
                "svln_op_subset_argmax: ldw, ldx multiples of the 16-byte chunk, W and x 16-byte aligned (aligned row loads)");
        check_allowed_list("svln_op_subset_argmax", ids, a.n, a.V);
        REQUIRE(!a.pen_flags || a.pen > 0.0f, "svln_op_subset_argmax: penalty flags need a factor > 0");
        REQUIRE(std::isfinite(smp.temperature) && smp.temperature >= 0.0f, "svln_op_subset_argmax: the temperature must be finite and >= 0 (0 = greedy)");
        const bool sampled = smp.temperature > 0.0f;
        ensure_allow_buffers();
        const int n = a.n, B = a.B;
        const HeadForm f = head_form(sampled ? EPI_SAMPLE : EPI_ARGMAX_LSE);
        a.ids = d_op_allow; a.skip = nullptr;
        if (sampled) a.smp = op_sample_args(smp, B, part_raw_b, part_max_b, true);
        aim(a, parts_b(), f);
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<int> l(n);
        for (int k = 0; k < n; ++k) l[k] = (int)ids[k];
        HIP_CHECK(hipMemcpy(d_op_allow, l.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        const float* ysrc = sampled ? part_max_b : part_val_b;
        launch_gemv_subset<T>(st, a);
        launch_subset_logprobs(st, ysrc, n, B, d_alp_b);
        merge_head(parts_b(), n, 1, B, f, out_rows(0, 0));
        HIP_CHECK(hipMemcpyAsync(h_alp_b, d_alp_b, (size_t)B * n * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(host_y, ysrc, (size_t)B * n * sizeof(float), hipMemcpyDeviceToHost, st));
        batched_scores_out(B, host_tokens, host_logprobs, "op_subset_argmax");
        std::memcpy(host_dist, h_alp_b, (size_t)B * n * sizeof(float));
    }
    void set_batch_draft(int on) override {
        const bool want = on != 0;
        if (want == bdraft_on) return;         // nothing changes
        refuse(want ? C_SET_BATCH_DRAFT_ON : C_SET_BATCH_DRAFT_OFF);      // a ridden row must be computed in the numeric scheme of the decode row it replaces
        if (want) {
            REQUIRE(c.max_positions >= HEAD_ROWS + MAXB, "svln_set_batch_draft: max_positions too small");
        }
        HIP_CHECK(hipStreamSynchronize(st));
        bdraft_on = want;
    }
    void batch_draft_stats(int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int64_t* iterations, int64_t* single_rows, int reset) override {
        if (rides) *rides = st_brides;
        if (tokens_from_rides) *tokens_from_rides = st_btokens;
        if (rows_fed) *rows_fed = st_brows;
        if (iterations) *iterations = st_biters;
        if (single_rows) *single_rows = st_bsingle;
        if (reset) st_brides = st_btokens = st_brows = st_biters = st_bsingle = 0;
    }
    void set_prefill_draft(int on) override {
        const bool want = on != 0;
        if (want == ride_on) return;           // nothing changes
        refuse(want ? C_SET_PREFILL_DRAFT_ON : C_SET_PREFILL_DRAFT_OFF);      // a ridden row must be computed in the numeric scheme of the pass it replaces
        if (want) {
            REQUIRE(c.max_positions >= MAXB, "svln_set_prefill_draft: max_positions too small");
            set_speculative_buffers();
        }
        HIP_CHECK(hipStreamSynchronize(st));
        ride_on = want;
    }
    void prefill_draft_stats(int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int reset) override {
        if (rides) *rides = st_rides;
        if (tokens_from_rides) *tokens_from_rides = st_rtokens;
        if (rows_fed) *rows_fed = st_rrows;
        if (reset) st_rides = st_rtokens = st_rrows = 0;
    }
    void set_draft(int env, const int64_t* ids, int n) override {
        env_at(env);
        REQUIRE(n >= 0 && n <= c.max_positions, "svln_set_draft: 0 <= n <= max_positions");
        REQUIRE(n == 0 || ids, "svln_set_draft: null ids");
        if (drafts.empty()) { drafts.resize(envs.size()); draft_armed.assign(envs.size(), 0); }
        drafts[env].assign(ids, ids + n);
        draft_armed[env] = n > 0;
    }
    void draft_stats(int64_t* verify_passes, int64_t* tokens_from_verify, int64_t* single_steps, int reset) override {
        if (verify_passes) *verify_passes = st_passes;
        if (tokens_from_verify) *tokens_from_verify = st_vtokens;
        if (single_steps) *single_steps = st_single;
        if (reset) st_passes = st_vtokens = st_single = 0;
    }
    bool taps_on = true;
    void tap_copy(const T* row, int token_idx, int slot) {       // parity tap: hid_tap[min(token,7)][slot]
        if (!taps_on) return;
        const int t = token_idx < 8 ? token_idx : 7;
        HIP_CHECK(hipMemcpyAsync(hid_tap + (size_t)(t * MAXB + slot) * H, row, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
    }

    // ---- multi-env scheduler (caller = a DAgger-style collector whose envs mix expert and model steps, so their model
    // turns fall due at different times: streamvln_dagger.py:232-313).  Per-env semantics are those of svln_generate; execution is
    // iteration-level batching: every iteration is ONE pass over the weights that carries, for each active env, either the rows of
    // its new turn (prefill) or the single row of the token it generated in the previous iteration (decode).  Envs join at any
    // iteration (svln_batch_submit) and leave when they emit EOS / max_new_tokens, so prefilling and decoding envs share passes.
    struct Job {
        bool used = false, finished = false, prefill = true;
        int env = -1, max_new = 0, count = 0, last_tok = -1;
        std::vector<int64_t> out, eos;
        std::vector<float> scores; bool scored = false;      // svln_set_token_scores: log-probability of every id of `out`
        std::vector<int32_t> topi; std::vector<float> topl; int topk = 0;      // svln_top_logprobs: the [topk] lists of every id of `out`
        std::vector<float> ent; bool ent_on = false;         // svln_token_entropy: the entropy of the distribution every id of `out` was taken from
        std::vector<float> alp; int alp_n = 0;               // with svln_set_allowed_tokens too: the normalised row [alp_n] of every id of `out`
        std::vector<int> draft;      // svln_set_batch_draft: the usable draft the submit consumed, kept until the job's prefill iteration
        // svln_batch_submit_forced: the turn's ids are `fids`; the job ends in the iteration that prefills it with out = fids, `scores` their
        // log-probabilities (scored whatever svln_set_token_scores says) and the policy's own arg-max / its log-probability of every position
        bool forced = false;
        std::vector<int> fids; std::vector<int64_t> greedy; std::vector<float> greedy_lp;
    };
    Job jobs[MAXB];
    // forget a job: its slot becomes free, its repetition-penalty flags are cleared (the stream is idle between scheduler calls)
    void drop_job(int k) {
        Job& j = jobs[k];
        if (!j.used) return;
        if (pen_flags_b && !j.out.empty()) {
            const int n = (int)j.out.size() < c.max_positions ? (int)j.out.size() : c.max_positions;
            for (int q = 0; q < n; ++q) h_pen_ids[q] = (int)j.out[q];
            (void)hipMemcpyAsync(d_pen_ids, h_pen_ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st);
            launch_set_flags(st, pen_flags_b + (size_t)k * V, d_pen_ids, nullptr, n, 0);
            (void)hipStreamSynchronize(st);          // h_pen_ids is reused by the next drop
        }
        j = Job();
    }
    void cancel_jobs_of(int env) {
        for (int k = 0; k < MAXB; ++k) if (jobs[k].used && jobs[k].env == env) drop_job(k);
    }
    // svln_batch_cancel: slot >= 0 drops that turn, slot < 0 every turn in flight.  The envs keep whatever rows / KV the dropped turns
    // had already written (a cancelled prefill leaves kv_len behind n_embeds: reset the env, or submit it again to finish the prefill).
    void batch_cancel(int slot) override {
        REQUIRE(slot < MAXB, "no such scheduler slot");
        HIP_CHECK(hipStreamSynchronize(st));
        if (slot >= 0) drop_job(slot);
        else for (int k = 0; k < MAXB; ++k) drop_job(k);
    }
    void ensure_pen_buffers() {
        if (pen_flags) return;
        pen_flags = dalloc<uint8_t>((size_t)V, true);
        pen_flags_b = dalloc<uint8_t>((size_t)MAXB * V, true);
        d_pen_rows = dalloc<int>(MAXB, true);
        d_pen_ids = dalloc<int>((size_t)c.max_positions + 8);
        HIP_CHECK(hipHostMalloc((void**)&h_pen_rows, 2 * MAXB * sizeof(int)));      // [MAXB ..): the second upload of a split iteration
        HIP_CHECK(hipHostMalloc((void**)&h_pen_ids, ((size_t)c.max_positions + 8) * sizeof(int)));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // generation_config.repetition_penalty of a checkpoint (HF RepetitionPenaltyLogitsProcessor over the tokens generated in the turn;
    // transformers 4.45.1 applies it under greedy decoding too).  1 = off (the default: no kernel sees a flag pointer).
    void set_repetition_penalty(float penalty) override {
        REQUIRE(penalty > 0.0f, "repetition_penalty must be > 0");
        refuse(C_SET_REPETITION_PENALTY);
        HIP_CHECK(hipStreamSynchronize(st));
        if (penalty != 1.0f) ensure_pen_buffers();
        if (penalty != rep_penalty) {
            drop_graphs();           // the captured lm_head launch holds the flag pointer and the factor
            // flags of the last penalised turn must not survive a change of the factor: an unpenalised generate() in between rewrites
            // d_out_ids / GenCtl.count without touching them, so the next penalised turn would clear the wrong ids (P -> 1 -> P)
            if (pen_flags) {
                HIP_CHECK(hipMemsetAsync(pen_flags, 0, (size_t)V, st));
                HIP_CHECK(hipMemsetAsync(pen_flags_b, 0, (size_t)MAXB * V, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
        }
        rep_penalty = penalty;
    }
    void set_turn_row_limit(int rows) override { REQUIRE(rows >= 0, "row limit must be >= 0 (0 = none)"); turn_row_limit = rows; }
    int batch_submit(int env, int max_new, const int64_t* eos, int n_eos) override {
        Env& e = env_at(env);
        refuse_while_group_on(env, "svln_batch_submit");
        REQUIRE(weights_missing() == 0, g_err);
        REQUIRE(max_new >= 1, "max_new_tokens must be >= 1");
        REQUIRE(e.n_embeds - e.kv_len >= 1, "nothing to prefill for this env (append its turn first)");
        int slot = -1;
        for (int k = 0; k < MAXB; ++k) {
            REQUIRE(!(jobs[k].used && jobs[k].env == env), "this env already has a turn in flight");
            if (slot < 0 && !jobs[k].used) slot = k;
        }
        REQUIRE(slot >= 0, "at most 8 turns in flight");
        Job& j = jobs[slot];
        j = Job();
        j.used = true; j.env = env; j.max_new = max_new < c.max_positions ? max_new : c.max_positions;
        j.eos.assign(eos, eos + n_eos);
        j.scored = scores_on; j.topk = topk; j.ent_on = ent_on;
        j.alp_n = scores_on && allow_on ? allow_n : 0;
        n_generated_b[slot] = 0;
        // svln_set_batch_draft: the env's armed draft is consumed by the submit whether or not it helps (the rule of svln_generate); usable:
        // no repetition penalty, ids in the vocabulary (the first one outside ends the draft)
        if (bdraft_on && disarm_draft(env) && rep_penalty == 1.0f)
            for (int64_t id : drafts[env]) { if (id < 0 || id >= V) break; j.draft.push_back((int)id); }
        return slot;
    }
    // svln_batch_submit_forced: a forced turn (svln_generate_forced) as a job of the scheduler.  The job is a prefill segment that also
    // feeds F[0 .. n - 1) and sends its last n rows through the EPI_TARGET head; it finishes in the iteration that prefills it.  Every
    // refusal of svln_batch_submit and of forced_refusals (but the idle-scheduler line) comes before any state change: the job table, the
    // env, the armed draft.  The armed draft is treated as svln_batch_submit treats it -- consumed iff svln_set_batch_draft is on -- and
    // never read.
    void ensure_bforced_buffers() {
        constexpr int R = HeadLists::R;
        if (bf_xn && (bf_dev_alp || !allow_on)) return;      // (the hot path: no allocation, no synchronisation)
        if (!bf_xn) {
            bf_xn = dalloc<T>((size_t)R * H, true);
            int* di = dalloc<int>(4 * R, true); float* df = dalloc<float>(3 * R, true);
            bf_dev.cut(di, df);
            HIP_CHECK(hipHostMalloc((void**)&bf_host.src, 4 * R * sizeof(int)));
            HIP_CHECK(hipHostMalloc((void**)&bf_host.val, 3 * R * sizeof(float)));
            bf_host.cut(bf_host.src, bf_host.val);
        }
        if (allow_on && !bf_dev_alp) {
            bf_dev_alp = dalloc<float>((size_t)BFORCED_ROWS * ALLOW_MAX, true);
            HIP_CHECK(hipHostMalloc((void**)&bf_host_alp, (size_t)BFORCED_ROWS * ALLOW_MAX * sizeof(float)));
        }
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // the refusals of a forced submit that need no state of the env's rows (a caller checks them before it encodes a frame or splices a turn)
    void batch_forced_check(int env, const int64_t* ids, int n, const int64_t* eos, int n_eos) override {
        env_at(env);
        refuse_while_group_on(env, "svln_batch_submit_forced");
        REQUIRE(weights_missing() == 0, g_err);
        forced_refusals(env, ids, n, eos, n_eos, "svln_batch_submit_forced", true);
        int free_slots = 0;
        for (int k = 0; k < MAXB; ++k) {
            REQUIRE(!(jobs[k].used && jobs[k].env == env), "this env already has a turn in flight");
            free_slots += !jobs[k].used;
        }
        REQUIRE(free_slots > 0, "at most 8 turns in flight");
    }
    int batch_submit_forced(int env, const int64_t* ids, int n, const int64_t* eos, int n_eos) override {
        Env& e = env_at(env);
        batch_forced_check(env, ids, n, eos, n_eos);
        REQUIRE(e.n_embeds - e.kv_len >= 1, "nothing to prefill for this env (append its turn first)");
        REQUIRE((int64_t)e.n_embeds + n - 1 <= c.max_positions, "svln_batch_submit_forced: n_embeds + n - 1 exceeds max_positions");
        int slot = -1;
        for (int k = 0; k < MAXB; ++k) {
            REQUIRE(!(jobs[k].used && jobs[k].env == env), "this env already has a turn in flight");
            if (slot < 0 && !jobs[k].used) slot = k;
        }
        REQUIRE(slot >= 0, "at most 8 turns in flight");
        ensure_bforced_buffers();       // (a failed allocation leaves the job table, the env and the draft as they were)
        // ---- nothing was changed up to here
        Job& j = jobs[slot];
        j = Job();
        j.used = true; j.env = env; j.max_new = n; j.forced = true;
        j.eos.assign(eos, eos + n_eos);
        j.fids.assign(ids, ids + n);
        j.scored = true;
        j.alp_n = allow_on ? allow_n : 0;
        n_generated_b[slot] = 0;
        if (bdraft_on) disarm_draft(env);
        return slot;
    }
    void batch_forced(int slot, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs, int cap, int32_t* n) override {
        REQUIRE(slot >= 0 && slot < MAXB && jobs[slot].used && jobs[slot].finished, "no finished turn in this slot");
        const Job& j = jobs[slot];
        REQUIRE(j.forced, "svln_batch_forced: this slot holds a plain turn (svln_batch_submit), not a forced one");
        const int m = (int)j.fids.size();
        for (int k = 0; k < m && k < cap; ++k) { logprobs[k] = j.scores[k]; greedy_ids[k] = j.greedy[k]; greedy_logprobs[k] = j.greedy_lp[k]; }
        *n = m;
    }
    void batch_forced_stats(int64_t* jobs_run, int64_t* rows_fed, int64_t* head_launches, int reset) override {
        if (jobs_run) *jobs_run = st_fjobs;
        if (rows_fed) *rows_fed = st_frows;
        if (head_launches) *head_launches = st_fhead;
        if (reset) st_fjobs = st_frows = st_fhead = 0;
    }
    // Head of the forced jobs of an iteration, after the plain head rows (which keep their code, order and buffers): the forced head rows
    // are listed in slot order, a job's n rows consecutive (row i = the segment's row that precedes F[i]); ONE indexed final norm writes
    // them to bf_xn and to the parity taps (row i -> tap row min(i, 7) of the job's slot, tap row 7 keeping the last); the list goes through the EPI_TARGET lm_head in
    // chunks of <= 32 rows from its start (a job may straddle a chunk), each chunk of r rows with the routing svln_generate_forced has for
    // n = r; pad rows carry target -1.  Under an allowed list: the subset product in its EPI_TARGET form, subset_logprobs and the final
    // kernel.  With sampling on inv_t = smp_inv_t, no noise is evaluated and no draw counter moves.  Returns the number of head rows.
    int head_forced(const std::vector<Seg>& segs, const std::vector<int>& pre_now) {
        const HeadLists& h = bf_host;
        int nf = 0;
        for (size_t q = 0; q < segs.size(); ++q) {
            const Job& j = jobs[pre_now[q]];
            if (!j.forced) continue;
            const int n = (int)j.fids.size();
            for (int i = 0; i < n; ++i) {
                h.src[nf] = segs[q].off + segs[q].Tn - n + i;
                // tap row min(i, 7); of the rows that share tap row 7 only the last is written (what tap_copy's sequence leaves there:
                // one launch must not write one tap row from two head rows)
                h.tap[nf] = taps_on && (i < 7 || i == n - 1) ? (i < 7 ? i : 7) * MAXB + pre_now[q] : -1;
                h.tgt[nf] = j.fids[i];
                ++nf;
            }
        }
        REQUIRE(nf >= 1 && nf <= BFORCED_ROWS, "batch_step: more forced head rows than the workspace holds");
        // (the pinned lists were last read by copies of an iteration that ended in a synchronisation)
        upload_head_lists(nf);
        launch_rmsnorm_indexed<T>(st, x, final_norm, bf_xn, bf_dev.src, bf_dev.tap, hid_tap, nf, H, c.rms_eps);
        head_target_chunks(nf);
        return nf;
    }
    // the source, tap and target lists of nf head rows -> the device (8 pad targets of -1 behind them: the last chunk's row count)
    void upload_head_lists(int nf) {
        const HeadLists &h = bf_host, &d = bf_dev;
        for (int k = nf; k < nf + 8; ++k) h.tgt[k] = -1;
        HIP_CHECK(hipMemcpyAsync(d.src, h.src, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d.tap, h.tap, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d.tgt, h.tgt, (size_t)(nf + 8) * sizeof(int), hipMemcpyHostToDevice, st));
    }
    // rows [0, nf) of bf_xn (targets bf_dev.tgt) through the EPI_TARGET head in chunks of <= 32 rows; the results are copied to the
    // pinned lists (the caller synchronises).  Shared by the forced jobs of an iteration and by svln_generate_candidates.
    void head_target_chunks(int nf) {
        const HeadLists &h = bf_host, &d = bf_dev;
        const float inv_t = smp_on ? smp_inv_t : 1.0f;
        for (int r0 = 0; r0 < nf; r0 += 32) {
            const int r = std::min(nf - r0, 32);
            const T* rows_x = bf_xn + (size_t)r0 * H;
            if (allow_on) {
                target_subset_rows(rows_x, r, inv_t, bf_dev_alp + (size_t)r0 * allow_n, d.tok + r0, d.score + r0);
            } else {
                const TargetOut o{d.tgt + r0, d.val + r0, d.tok + r0, d.score + r0, d.lp + r0};
                target_rows(lm_head, H, rows_x, H, V, H, ride_head_rows(r), r, inv_t, &o);
            }
            st_fhead += 1;
        }
        HIP_CHECK(hipMemcpyAsync(h.tok, d.tok, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h.score, d.score, (size_t)nf * sizeof(float), hipMemcpyDeviceToHost, st));
        if (allow_on) HIP_CHECK(hipMemcpyAsync(bf_host_alp, bf_dev_alp, (size_t)nf * allow_n * sizeof(float), hipMemcpyDeviceToHost, st));
        else HIP_CHECK(hipMemcpyAsync(h.lp, d.lp, (size_t)nf * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    // the log-probability of forced id `id` on head row `row`: the row's entry of the target list, or under an allowed list the id's entry
    // of the row's normalised allowed-list row (the same bits svln_get_allowed_logprobs returns)
    float forced_score(int row, int id, const float* lp_rows, const float* alp_rows) const {
        if (!allow_on) return lp_rows[row];
        const int pos = (int)(std::lower_bound(allow_ids.begin(), allow_ids.end(), id) - allow_ids.begin());
        return alp_rows[(size_t)row * allow_n + pos];
    }
    // one iteration; returns the number of jobs still running afterwards, finished_slots = jobs that completed in this iteration
    int batch_step(int32_t* finished_slots, int32_t* n_finished) override {
        *n_finished = 0;
        // a turn whose env has nothing left to prefill (its rows were reset or already consumed) is dropped alone, with an error that
        // names it; the other turns stay valid for the next call
        for (int k = 0; k < MAXB; ++k) {
            Job& j = jobs[k];
            if (!j.used || j.finished || !j.prefill) continue;
            const Env& e = envs[j.env];
            if (e.n_embeds - e.kv_len < 1) {
                const int env = j.env;
                drop_job(k);
                REQUIRE(false, "batch_step: env " + std::to_string(env) + " has no rows to prefill (reset after submit?); its turn was dropped");
            }
        }
        try {
            return batch_step_run(finished_slots, n_finished);
        } catch (...) {
            // the iteration failed part-way (page pool exhausted, non-finite logits, a HIP error): which jobs advanced is unknown, so every
            // turn in flight is dropped and the scheduler is idle again; the envs keep their rows (reset them or submit again)
            (void)hipStreamSynchronize(st);
            for (int k = 0; k < MAXB; ++k) drop_job(k);
            *n_finished = 0;
            throw;
        }
    }
    // Head of an iteration with rides (svln_set_batch_draft): a fixed number of launches whatever the row count.  Head rows = the nrow decode
    // rows, then the last prompt row and the draft rows of every segment; one indexed final norm writes them to xn[0 .. nh) and to their
    // parity taps (head row i of a segment -> tap row i of its job), the arg-max product takes them in chunks of <= 32 rows into
    // d_tok_b[0 .. nh) (the pad rows of a chunk's row count are stale rows of xn: readable, their arg-maxes never read).  Returns nh.
    int head_with_rides(const std::vector<int>& dec, int nrow, const std::vector<Seg>& segs, const std::vector<int>& pre_now, std::vector<int>& order) {
        int nh = 0;
        auto head_row = [&](int src, int tap_idx, int slot) {
            h_head_src[nh] = src;
            h_head_tap[nh] = taps_on ? (tap_idx < 8 ? tap_idx : 7) * MAXB + slot : -1;
            ++nh;
        };
        for (int k = 0; k < nrow; ++k) head_row(k, jobs[dec[k]].count, dec[k]);
        for (size_t q = 0; q < segs.size(); ++q) {
            const Seg& g = segs[q];
            if (jobs[pre_now[q]].forced) continue;      // (its head rows follow in head_forced)
            for (int i = 0; i <= g.n_draft; ++i) head_row(g.off + g.Tn - 1 - g.n_draft + i, i, pre_now[q]);
            order.push_back(pre_now[q]);
        }
        REQUIRE(nh <= HEAD_ROWS, "batch_step: more head rows than the workspace holds");
        HIP_CHECK(hipMemcpyAsync(d_head_src, h_head_src, (size_t)nh * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_head_tap, h_head_tap, (size_t)nh * sizeof(int), hipMemcpyHostToDevice, st));
        launch_rmsnorm_indexed<T>(st, x, final_norm, xn, d_head_src, d_head_tap, hid_tap, nh, H, c.rms_eps);
        for (int r0 = 0; r0 < nh; r0 += 32) {
            const int n = std::min(nh - r0, 32);
            argmax_rows(lm_head, H, xn + (size_t)r0 * H, H, V, H, n == 1 ? 1 : ride_head_rows(n), false, r0);
        }
        return nh;
    }
    // the pure batched decode step for B rows (d_slots / d_tok_b / d_smp set): the launches, or their captured graph
    void batched_step(int B, bool pen) {
        if (use_graph) {
            const int key = B | (pen ? 256 : 0) | (fp8_gemm_on ? 512 : 0) | (mx4b_on ? 1024 : 0) | (fp8_gemm_on && fp8_scaled_on ? 2048 : 0) | (scores_on ? 4096 : 0) | (smp_on ? 8192 : 0) | (topk << 16) | (ent_on ? 1 << 24 : 0);
            auto it = bgraphs.find(key);
            if (it == bgraphs.end())      // (a failed capture leaves no entry behind)
                it = bgraphs.emplace(key, capture_graph([&] { decode_ops_batched(B, pen); })).first;
            HIP_CHECK(hipGraphLaunch(it->second, st));
        } else {
            decode_ops_batched(B, pen);
        }
    }
    int batch_step_run(int32_t* finished_slots, int32_t* n_finished) {
        std::vector<int> dec, pre;                      // job slots decoding / prefilling in this iteration
        for (int k = 0; k < MAXB; ++k)
            if (jobs[k].used && !jobs[k].finished) (jobs[k].prefill ? pre : dec).push_back(k);
        if (dec.empty() && pre.empty()) return 0;
        const int nd = (int)dec.size();
        const bool pen = rep_penalty != 1.0f;
        // prefill jobs that fit the row workspaces next to the decode rows (the rest wait for the next iteration; a turn of up to
        // max_positions rows runs as soon as no decode row shares the pass)
        // svln_set_mxfp4_batched: decode rows never ride through the bf16 prefill products.  An iteration that holds both kinds is split:
        // the decode rows run as a pure batched decode step on the MXFP4 weights, then the prefill segments as a bf16 pass of their own
        // (rows from 0) with one lm_head for their last rows -- every env keeps the scheme of the solo mode whatever its neighbours do.
        const bool split_mixed = mx4b_on;
        std::vector<Seg> segs;
        std::vector<int> pre_now;
        int n_ride = 0;                                 // draft rows of this iteration: (row, id) pairs in h_ride_list
        int n_fed = 0, n_forced = 0, n_plain = 0;       // fed rows of forced jobs (pairs of the same list, after the n_ride counted so far) / forced / plain segments
        int ride_kd[MAXB] = {0};                        // draft rows of each plain job's segment, by slot
        int M = split_mixed ? 0 : nd;
        for (int k : pre) {
            Env& e = envs[jobs[k].env];
            const int Tn = e.n_embeds - e.kv_len;
            REQUIRE(Tn >= 1 && Tn <= c.max_positions, "prefill length out of range");
            if (jobs[k].forced) {
                // a forced job's segment: its Tn rows and the ids F[0 .. n - 1) at the next positions, gathered on the device through the
                // ragged list; the last id is never fed.  All or nothing: a segment that does not fit waits, it is never cut like a draft.
                const Job& j = jobs[k];
                const int nfed = (int)j.fids.size() - 1;
                if (M + Tn + nfed > c.max_positions) continue;
                // (the submit checked this; rows appended to the env since then must not push a fed row past the last position)
                REQUIRE(e.n_embeds + nfed <= c.max_positions, "batch_step: a forced turn's n_embeds + n - 1 exceeds max_positions (rows appended after the submit?)");
                ensure_pages(e, e.n_embeds + nfed);
                for (int q = 0; q < nfed; ++q) { h_ride_list[2 * (n_ride + n_fed)] = M + Tn + q; h_ride_list[2 * (n_ride + n_fed) + 1] = j.fids[q]; ++n_fed; }
                segs.push_back(Seg{&e, e.kv_len, Tn + nfed, M, nfed});
                pre_now.push_back(k);
                M += Tn + nfed;
                ++n_forced;
                continue;
            }
            if (M + Tn > c.max_positions) continue;          // (a waiting job keeps its draft)
            // svln_set_batch_draft: k ids of the job's draft ride as the segment's last rows -- the rule of the single-env ride (k of
            // svln_set_prefill_draft), cut further to the rows the workspace still holds.  The draft is dropped with its ride.
            int kd = 0;
            Job& j = jobs[k];
            if (!j.draft.empty()) {
                kd = std::max(std::min(std::min((int)j.draft.size(), RIDE_MAX_ROWS), std::min(j.max_new - 1, c.max_positions - e.n_embeds)), 0);
                for (int q = 0; q < kd; ++q)
                    if (std::find(j.eos.begin(), j.eos.end(), (int64_t)j.draft[q]) != j.eos.end()) { kd = q; break; }
                kd = std::min(kd, c.max_positions - M - Tn);
                for (int q = 0; q < kd; ++q) { h_ride_list[2 * (n_ride + n_fed)] = M + Tn + q; h_ride_list[2 * (n_ride + n_fed) + 1] = j.draft[q]; ++n_ride; }
            }
            ensure_pages(e, e.n_embeds + kd);
            segs.push_back(Seg{&e, e.kv_len, Tn + kd, M, kd});
            pre_now.push_back(k);
            ride_kd[k] = kd;
            M += Tn + kd;
            ++n_plain;
        }
        const bool rides = n_ride > 0;                  // (never under a repetition penalty or svln_set_mxfp4_batched: no draft is usable / the switch excludes it)
        const int n_ragged = n_ride + n_fed;            // rows the ragged gather writes: the rides' draft rows and the forced jobs' fed rows
        REQUIRE(n_ragged <= RIDE_PAIRS, "batch_step: more gathered rows than the list holds");
        if (n_ragged > 0) HIP_CHECK(hipMemcpyAsync(d_ride_list, h_ride_list, (size_t)n_ragged * 2 * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(ph_ev[2], st));
        std::vector<int> order;                         // job slot of each output token of this iteration
        if (nd > 0) {
            int B = nd;
            const bool pure = segs.empty() || split_mixed;
            if (pure) { B = 1; while (B < nd) B <<= 1; }              // the pure decode kernels come in power-of-two batch sizes
            for (int k = 0; k < B; ++k) {
                const int kk = k < nd ? k : 0;                          // padding slots replay slot 0 (same writes, ignored outputs)
                Env& e = envs[jobs[dec[kk]].env];
                REQUIRE(e.kv_len + 1 <= c.max_positions, "sequence exceeds max_positions during decode");
                if (k < nd) ensure_pages(e, e.kv_len + 1);
                h_slots[k].page_table = e.d_pages; h_slots[k].pos = e.kv_len; h_slots[k].pad = 0;
                h_tok_b[k] = jobs[dec[kk]].last_tok;
                if (pen) h_pen_rows[k] = dec[kk];
            }
            HIP_CHECK(hipMemcpyAsync(d_slots, h_slots, B * sizeof(DecodeSlot), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d_tok_b, h_tok_b, B * sizeof(int), hipMemcpyHostToDevice, st));
            if (pure) {
                if (pen) HIP_CHECK(hipMemcpyAsync(d_pen_rows, h_pen_rows, B * sizeof(int), hipMemcpyHostToDevice, st));
                if (smp_on) upload_sample_rows(dec.data(), nd, B);
                // gather + 28 layers + head for B decode rows -> d_tok_b, xn = final-norm rows.  With hipGraph replay on, the step of each
                // (B, fp8, penalty) combination is captured once: every run-time value (page tables, positions, fed tokens) is in d_slots / d_tok_b.
                batched_step(B, pen);
            } else {
                launch_gather_rows<T>(st, d_tok_b, embed, feats, x, nd, H);
            }
            for (int k = 0; k < nd; ++k) order.push_back(dec[k]);
        }
        // a split iteration: the decode step above is complete (d_tok_b, xn = its final-norm rows); its taps and tokens are taken
        // before the prefill pass reuses xn / d_tok_b, and ph_ev[4] divides the iteration's time between the two phase timers
        const bool split = split_mixed && nd > 0 && !segs.empty();
        const int head0 = split ? nd : 0;               // first entry of `order` that the lm_head pass below produces
        int n_head = 0;                                 // arg-maxes the lm_head pass below leaves in d_tok_b
        if (split) {
            for (int q = 0; q < nd; ++q) tap_copy(xn + (size_t)q * H, jobs[order[q]].count, order[q]);
            HIP_CHECK(hipMemcpyAsync(h_tok_b, d_tok_b, nd * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipEventRecord(ph_ev[4], st));
        }
        if (!segs.empty()) {
            const int nrow = split_mixed ? 0 : nd;      // decode rows that share the prefill pass
            prefill_rows(segs, M, nrow, n_ragged);
            if (rides) {
                n_head = head_with_rides(dec, nrow, segs, pre_now, order);
            } else if (nrow + n_plain > 0) {            // (== 0: every segment of the pass is a forced job's)
                // last row of every plain job of this pass -> one lm_head pass
                const int nj = nrow + n_plain;
                for (int k = 0; k < nrow; ++k)
                    HIP_CHECK(hipMemcpyAsync(last_rows + (size_t)k * H, x + (size_t)k * H, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
                for (size_t q = 0, qp = 0; q < segs.size(); ++q) {
                    if (jobs[pre_now[q]].forced) continue;
                    const T* last = x + (size_t)(segs[q].off + segs[q].Tn - 1) * H;
                    HIP_CHECK(hipMemcpyAsync(last_rows + (size_t)(nrow + qp) * H, last, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
                    order.push_back(pre_now[q]);
                    ++qp;
                }
                int Bp = 1; while (Bp < nj) Bp <<= 1;
                for (int k = nj; k < Bp; ++k)
                    HIP_CHECK(hipMemcpyAsync(last_rows + (size_t)k * H, last_rows, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
                if (pen) {
                    int* hp = h_pen_rows + (split ? MAXB : 0);      // (the decode step's upload may still be pending on the first half)
                    for (int k = 0; k < Bp; ++k) hp[k] = order[head0 + (k < nj ? k : 0)];
                    HIP_CHECK(hipMemcpyAsync(d_pen_rows, hp, Bp * sizeof(int), hipMemcpyHostToDevice, st));
                }
                if (smp_on) upload_sample_rows(order.data() + head0, nj, Bp);
                head_batched(last_rows, Bp, pen);
            }
        }
        const int nj = (int)order.size();
        if (!rides) {
            for (int q = head0; q < nj; ++q) tap_copy(xn + (size_t)(q - head0) * H, jobs[order[q]].count, order[q]);
            n_head = nj - head0;
        }
        const int n_fhead = n_forced > 0 ? head_forced(segs, pre_now) : 0;      // (bf_xn and lists of its own: the plain rows above are untouched)
        HIP_CHECK(hipEventRecord(ph_ev[3], st));
        if (n_head > 0) HIP_CHECK(hipMemcpyAsync(h_tok_b + head0, d_tok_b, n_head * sizeof(int), hipMemcpyDeviceToHost, st));
        if (scores_on) HIP_CHECK(hipMemcpyAsync(h_score_b + head0, d_score_b, n_head * sizeof(float), hipMemcpyDeviceToHost, st));      // (never split: the switches exclude each other)
        if (scores_on && allow_on) HIP_CHECK(hipMemcpyAsync(h_alp_b + (size_t)head0 * allow_n, d_alp_b, (size_t)n_head * allow_n * sizeof(float), hipMemcpyDeviceToHost, st));
        if (ent_on) HIP_CHECK(hipMemcpyAsync(h_ent_b + head0, d_ent_b, n_head * sizeof(float), hipMemcpyDeviceToHost, st));
        if (topk) {
            HIP_CHECK(hipMemcpyAsync(h_topi_b + (size_t)head0 * topk, d_topi_b, (size_t)n_head * topk * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(h_topl_b + (size_t)head0 * topk, d_topl_b, (size_t)n_head * topk * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        LAUNCH_CHECK("batch_step");
        if (split) { add_phase(2, 2, 4); add_phase(1, 4, 3); }
        else add_phase(segs.empty() ? 2 : 1, 2, 3);
        settle_vision();
        st_biters += 1;
        st_bsingle += nd;
        int hq = 0;                                     // head row of h_tok_b the next job starts at
        for (int q = 0; q < nj; ++q) {
            Job& j = jobs[order[q]];
            Env& e = envs[j.env];
            // a job's k + 1 arg-maxes (k = 0 without a ride) under the verify rule from zero emitted tokens: row 0's is always emitted,
            // row i's iff every earlier one was emitted without stopping and equals the draft id row i was fed; a stopping token is
            // appended, never fed.  K / V rows of rejected positions lie beyond kv_len and are overwritten later.
            const int kd = j.prefill && rides ? ride_kd[order[q]] : 0;
            int tok = -1, emitted = 0;
            bool stop = false;
            for (int i = 0; i <= kd && !stop; ++i) {
                if (i > 0 && tok != j.draft[i - 1]) break;
                tok = h_tok_b[hq + i];
                require_finite_tokens(&tok, 1);
                j.out.push_back(tok);
                if (j.scored) j.scores.push_back(h_score_b[hq + i]);
                if (j.ent_on) j.ent.push_back(h_ent_b[hq + i]);
                if (j.topk) {
                    j.topi.insert(j.topi.end(), h_topi_b + (size_t)(hq + i) * j.topk, h_topi_b + (size_t)(hq + i + 1) * j.topk);
                    j.topl.insert(j.topl.end(), h_topl_b + (size_t)(hq + i) * j.topk, h_topl_b + (size_t)(hq + i + 1) * j.topk);
                }
                if (j.alp_n > 0) j.alp.insert(j.alp.end(), h_alp_b + (size_t)(hq + i) * j.alp_n, h_alp_b + (size_t)(hq + i + 1) * j.alp_n);
                if (smp_on) env_draws[j.env] += 1;
                j.count += 1;
                ++emitted;
                stop = j.count >= j.max_new;
                for (int64_t id : j.eos) stop |= id == tok;
            }
            hq += kd + 1;
            if (j.prefill) {                                                  // this iteration prefilled the turn
                e.kv_len = e.n_embeds + emitted - 1;
                j.prefill = false;
                if (kd > 0) { st_brides += 1; st_btokens += emitted; st_brows += kd; }
                std::vector<int>().swap(j.draft);
            } else {
                e.kv_len += 1;                                                // ... or fed the previous token
            }
            j.last_tok = tok;
            if (pen && !stop) {                                               // the token counts as generated for this job's next arg-max
                h_pen_ids[q] = tok;
                HIP_CHECK(hipMemcpyAsync(d_pen_ids + q, h_pen_ids + q, sizeof(int), hipMemcpyHostToDevice, st));
                launch_set_flags(st, pen_flags_b + (size_t)order[q] * V, d_pen_ids + q, nullptr, 1, 1);
            }
            if (stop) {
                j.finished = true;
                n_generated_b[order[q]] = j.count;
                finished_slots[(*n_finished)++] = order[q];
            }
        }
        if (pen) HIP_CHECK(hipStreamSynchronize(st));                         // h_pen_ids is rewritten by the next iteration
        // the forced jobs of the iteration, in the order head_forced listed them: each ends here with out = F, where a plain turn that
        // emitted F leaves the env (the last id appended, not fed); no draw counter moves
        if (n_fhead > 0) {
            const HeadLists& h = bf_host;
            require_finite_tokens(h.tok, n_fhead);
            int fq = 0;
            for (size_t q = 0; q < segs.size(); ++q) {
                Job& j = jobs[pre_now[q]];
                if (!j.forced) continue;
                Env& e = envs[j.env];
                const int n = (int)j.fids.size();
                j.out.assign(j.fids.begin(), j.fids.end());
                for (int i = 0; i < n; ++i) {
                    j.greedy.push_back(h.tok[fq + i]);
                    j.greedy_lp.push_back(h.score[fq + i]);
                    j.scores.push_back(forced_score(fq + i, j.fids[i], h.lp, bf_host_alp));
                }
                if (allow_on) { j.alp.assign(bf_host_alp + (size_t)fq * allow_n, bf_host_alp + (size_t)(fq + n) * allow_n); j.alp_n = allow_n; }
                fq += n;
                e.kv_len = e.n_embeds + n - 1;
                j.prefill = false; j.count = n; j.last_tok = j.fids[n - 1];
                j.finished = true;
                n_generated_b[pre_now[q]] = n;
                finished_slots[(*n_finished)++] = pre_now[q];
                st_fjobs += 1; st_frows += n - 1;
            }
        }
        int running = 0;
        for (int k = 0; k < MAXB; ++k) running += jobs[k].used && !jobs[k].finished;
        return running;
    }
    void batch_result(int slot, int32_t* env, int64_t* out, int cap, int32_t* n_out) override {
        REQUIRE(slot >= 0 && slot < MAXB && jobs[slot].used && jobs[slot].finished, "no finished turn in this slot");
        Job& j = jobs[slot];
        const int n = (int)j.out.size();
        for (int k = 0; k < n && k < cap; ++k) out[k] = j.out[k];
        *n_out = n; *env = j.env;
        drop_job(slot);
    }
    // svln_generate on each listed env, executed together: submit all, iterate until all are done (all envs prefill in the first
    // iteration and decode in lockstep afterwards: the special case of the scheduler in which every turn falls due at once)
    void generate_batch(const int32_t* env_ids, int n_envs, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap,
                        int32_t* n_out) override {
        REQUIRE(n_envs >= 1 && n_envs <= MAXB, "1..8 envs per batch");
        REQUIRE(max_new >= 1 && cap >= 1, "max_new_tokens must be >= 1");
        refuse(C_GENERATE_BATCH);
        for (int s = 0; s < n_envs; ++s)
            for (int t = 0; t < s; ++t) REQUIRE(env_ids[t] != env_ids[s], "duplicate env in batch");
        for (int s = 0; s < n_envs; ++s) refuse_while_group_on(env_ids[s], "svln_generate_batch");
        std::vector<int> slots(n_envs);
        gb_scores_valid = false; gb_alp_valid = false; gb_topk_valid = false; gb_ent_valid = false;
        try {
            for (int s = 0; s < n_envs; ++s) slots[s] = batch_submit(env_ids[s], max_new < cap ? max_new : cap, eos, n_eos);
            int32_t fin[MAXB], nf = 0;
            while (batch_step(fin, &nf) > 0) {}
        } catch (...) {
            for (int k = 0; k < MAXB; ++k) drop_job(k);
            throw;
        }
        gb_scores.assign(n_envs, std::vector<float>());
        gb_topi.assign(n_envs, std::vector<int32_t>()); gb_topl.assign(n_envs, std::vector<float>());
        gb_alp.assign(n_envs, std::vector<float>());
        gb_ent.assign(n_envs, std::vector<float>());
        for (int s = 0; s < n_envs; ++s) {
            int32_t env = 0;
            if (scores_on) gb_scores[s] = jobs[slots[s]].scores;
            if (topk) { gb_topi[s] = jobs[slots[s]].topi; gb_topl[s] = jobs[slots[s]].topl; }
            if (scores_on && allow_on) gb_alp[s] = jobs[slots[s]].alp;
            if (ent_on) gb_ent[s] = jobs[slots[s]].ent;
            batch_result(slots[s], &env, out + (size_t)s * cap, cap, &n_out[s]);
        }
        gb_scores_valid = scores_on;          // (only once every env's scores are in place)
        gb_topk = topk; gb_topk_valid = topk > 0;
        gb_ent_valid = ent_on;
        gb_alp_n = allow_n; gb_alp_valid = scores_on && allow_on;
    }
    void get_hidden_batch(int slot, float* out, int max_rows, int32_t* n_rows) override {
        REQUIRE(slot >= 0 && slot < MAXB, "slot");
        int n = n_generated_b[slot] < 8 ? n_generated_b[slot] : 8;
        if (n > max_rows) n = max_rows;
        for (int t = 0; t < n; ++t) read_rows_f32(hid_tap + (size_t)(t * MAXB + slot) * H, (size_t)H, out + (size_t)t * H);
        *n_rows = n;
    }

    int read_token() {
        HIP_CHECK(hipMemcpyAsync(h_token, d_token, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_top2, d_top2, 2 * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return h_token[0];
    }

    // StreamVLNForCausalLM.generate -> GenerationMixin._sample (greedy): prefill embeds[kv_len:], then feed each generated id until
    // one is in the EOS set (appended, not fed) or max_new_tokens.  The loop state lives on the device (GenCtl): the prefill, its
    // arg-max and RUN_AHEAD decode steps are enqueued back to back, then ONE synchronisation reads the ids emitted so far; steps
    // enqueued past the end of the generation are no-ops (every kernel checks the done flag).
    // What svln_generate and svln_generate_drafts do before their first launch: the refusals, the armed draft (consumed by the call whether
    // it helps, is ignored or the call fails) and the EOS set on the device.  limit = the tokens the call may emit.
    struct GenBegin { bool had_draft; int P, L, Tn, limit; };
    GenBegin gen_begin(int env, int max_new, const int64_t* eos, int n_eos, int cap) {
        Env& e = env_at(env);
        refuse_while_group_on(env, "svln_generate");
        invalidate_last_results();
        GenBegin b;
        b.had_draft = disarm_draft(env);
        REQUIRE(weights_missing() == 0, g_err);
        b.P = e.kv_len; b.L = e.n_embeds; b.Tn = b.L - b.P;
        REQUIRE(b.Tn >= 1, "nothing to prefill: inputs_embeds not longer than the KV cache");
        REQUIRE(max_new >= 1 && cap >= 1, "max_new_tokens must be >= 1");
        REQUIRE(n_eos >= 0 && n_eos <= (V > 16 ? V : 16), "too many eos ids");
        b.limit = max_new < cap ? max_new : cap;
        {   // EOS set -> device (cached across calls: the harness passes the same list every turn)
            std::vector<int> ev(n_eos);
            for (int k = 0; k < n_eos; ++k) ev[k] = eos[k] >= 0 && eos[k] < V ? (int)eos[k] : -2;      // ids outside the vocabulary never match
            if (!eos_valid || ev != eos_cached) {
                HIP_CHECK(hipStreamSynchronize(st));
                eos_cached.swap(ev);
                if (n_eos) HIP_CHECK(hipMemcpy(d_eos, eos_cached.data(), (size_t)n_eos * sizeof(int), hipMemcpyHostToDevice));
                eos_valid = true;
            }
        }
        return b;
    }
    // the loop state of a turn that has emitted nothing: the first decode step feeds token 0 at position L (pos / kv_len advance when the
    // arg-max step appends without stopping); the penalty flags of the previous turn's tokens are cleared first
    void gen_ctl_start(int env, int L, int limit, int n_eos) {
        h_ctl->pos = L - 1; h_ctl->kv_len = L; h_ctl->done = 0; h_ctl->count = 0; h_ctl->max_new = limit; h_ctl->n_eos = n_eos;
        h_ctl->draw0 = smp_on ? env_draws[env] : 0; h_ctl->stream = smp_on ? env : 0;
        if (rep_penalty != 1.0f)      // tokens of the previous generate (still listed in d_out_ids[0 .. d_ctl.count)) no longer count
            launch_set_flags(st, pen_flags, d_out_ids, &d_ctl->count, 0, 0);
        HIP_CHECK(hipMemcpyAsync(d_ctl, h_ctl, sizeof(GenCtl), hipMemcpyHostToDevice, st));
    }
    void generate(int env, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out, bool fixed) override {
        Env& e = env_at(env);
        if (fixed) n_eos = 0;
        const GenBegin gb = gen_begin(env, max_new, eos, n_eos, cap);
        const bool had_draft = gb.had_draft;
        const int P = gb.P, L = gb.L, Tn = gb.Tn, limit = gb.limit;
        // the env's armed draft is consumed by this call whether or not it helps; usable: a draft mode is on, no repetition penalty (its
        // flags change the logits token by token), ids in the vocabulary (the first one outside ends the draft); verify passes need a guess
        // beyond index 0, a ride is served by index 0 alone
        int dlen = 0;
        if (had_draft) {
            if ((spec_rows > 0 || ride_on) && rep_penalty == 1.0f) {
                const std::vector<int64_t>& D = drafts[env];
                while (dlen < (int)D.size() && D[dlen] >= 0 && D[dlen] < V) { h_draft[dlen] = (int)D[dlen]; ++dlen; }
            }
        }
        const bool spec = spec_rows > 0 && dlen >= 2;
        // Ride (svln_set_prefill_draft): draft ids 0 .. k - 1 are fed as k more prefill rows at positions L .. L + k - 1; k is cut by the
        // verify step's 8 head rows, by the tokens the call may emit (a row's arg-max beyond them is useless), by max_positions and at
        // the first draft id in the EOS set (an EOS is appended, never fed).  k = 0: the plain turn, launch for launch.
        int k_ride = 0;
        if (ride_on && dlen >= 1) {
            k_ride = std::max(std::min(std::min(dlen, RIDE_MAX_ROWS), std::min(limit - 1, c.max_positions - L)), 0);
            for (int j = 0; j < k_ride; ++j)
                if (std::find(eos_cached.begin(), eos_cached.end(), h_draft[j]) != eos_cached.end()) { k_ride = j; break; }
        }
        const bool ride = k_ride >= 1;
        const int n_head = k_ride + 1;
        ensure_pages(e, L + k_ride);
        if (spec || ride) {
            h_vctl[0] = dlen;
            for (int j = 1; j < 16; ++j) h_vctl[j] = 0;
            if (ride) {
                h_vctl[6] = n_head;
                for (int i = 1; i < n_head; ++i) h_vctl[8 + i] = h_draft[i - 1];       // fed[i]: the token row Tn + i - 1 was given
            }
            HIP_CHECK(hipMemcpyAsync(d_draft, h_draft, (size_t)dlen * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d_vctl, h_vctl, 16 * sizeof(int), hipMemcpyHostToDevice, st));
        }
        gen_ctl_start(env, L, limit, n_eos);
        HIP_CHECK(hipEventRecord(ph_ev[2], st));
        if (ride) {
            prefill(e, P, Tn + k_ride, k_ride);
            ride_head(Tn + k_ride, n_head);
        } else {
            prefill(e, P, Tn);
            head(x + (size_t)(Tn - 1) * H, 0, true);
        }
        e.kv_len = L;
        HIP_CHECK(hipEventRecord(ph_ev[3], st));
        int enq = 1;                      // tokens whose arg-max step has been enqueued
        int n = 0;
        bool done = false, decoded = false;
        int vtokens = 0;                  // tokens of this turn that verify passes emitted
        int rtokens = 0;                  // tokens of this turn that the ride emitted (token 0 included)
        bool ride_held = true;            // every id the ride emitted equals the draft
        if (ride) {
            // one synchronisation reads what the ride emitted: a finished turn returns with no decode pass enqueued; otherwise verify
            // passes continue while the draft holds (svln_set_speculative on and guesses left), else single steps finish the turn
            HIP_CHECK(hipMemcpyAsync(h_ctl, d_ctl, sizeof(GenCtl), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(h_out_ids, d_out_ids, (size_t)n_head * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(h_vctl, d_vctl, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            LAUNCH_CHECK("generate (ride)");
            n = h_ctl->count;
            done = h_ctl->done != 0;
            REQUIRE(n >= 1 && n <= n_head, "generation state out of range");
            require_finite_tokens(h_out_ids, n);
            for (int k = 0; k < n && k < dlen; ++k) ride_held = ride_held && h_out_ids[k] == h_draft[k];
            rtokens = h_vctl[5];
            st_rides += h_vctl[4]; st_rtokens += rtokens; st_rrows += k_ride;
            enq = n;
        }
        if (spec && ride_held && !done) {
            // Verify passes while the draft holds: with cnt tokens emitted a pass carries rows_at(cnt) rows (verify_feed_kernel computes the
            // same number on the device); one is enqueued while the draft has a guess for the next token (cnt < dlen), even where max_new
            // or max_positions cut it to one row.  After each the host reads the ids: a further pass follows only if every id from index 1
            // on equals the draft, else the single steps below take over.
            auto rows_at = [&](int cnt) {
                int r = spec_rows;
                r = std::min(r, std::max(dlen - cnt + 1, 1));
                r = std::min(r, limit - cnt);
                r = std::min(r, c.max_positions - (L + cnt - 1));
                return r;
            };
            int cnt = enq;
            while (!done && cnt < dlen && rows_at(cnt) >= 1) {
                const int r = rows_at(cnt);
                ensure_pages(e, L + cnt - 1 + r);              // row i writes position L + cnt - 1 + i
                verify_pass(e, env);
                decoded = true;
                HIP_CHECK(hipEventRecord(ph_ev[4], st));
                HIP_CHECK(hipMemcpyAsync(h_ctl, d_ctl, sizeof(GenCtl), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipMemcpyAsync(h_out_ids, d_out_ids, (size_t)(cnt + r) * sizeof(int), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipMemcpyAsync(h_vctl, d_vctl, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                LAUNCH_CHECK("generate (verify pass)");
                n = h_ctl->count;
                done = h_ctl->done != 0;
                REQUIRE(n >= cnt && n <= cnt + r, "generation state out of range");
                require_finite_tokens(h_out_ids, n);
                bool held = n > cnt;
                for (int k = 1; k < n && k < dlen; ++k) held = held && h_out_ids[k] == h_draft[k];
                cnt = n;
                if (!held) break;
            }
            enq = cnt;
            vtokens = h_vctl[3];
            st_passes += h_vctl[2];
        }
        finish_turn(e, env, L, limit, enq, n, done, decoded, vtokens, ride ? rtokens : 1, ride, out, n_out);
    }
    // The rest of a single-env turn, shared by svln_generate and svln_generate_drafts: single decode steps until the turn is done (enq =
    // tokens whose arg-max step has been enqueued, n / done = what the last synchronisation read, if any), then the results: ids, scores,
    // lists, e.kv_len, the phase timers, n_generated, the draft counters and top2_stale.  vtokens: tokens of verify passes; head_tokens:
    // tokens the prefill pass itself emitted (1 without a draft); drafted: the pass carried draft rows.  Returns the single-step tokens.
    int finish_turn(Env& e, int env, int L, int limit, int enq, int n, bool done, bool decoded, int vtokens, int head_tokens, bool drafted,
                    int64_t* out, int32_t* n_out) {
        while (!done) {
            int steps = limit - enq;
            if (steps > RUN_AHEAD) steps = RUN_AHEAD;
            if (steps > c.max_positions - (L + enq - 1)) steps = c.max_positions - (L + enq - 1);       // step k feeds position L + enq - 1
            if (steps > 0) {
                ensure_pages(e, L + enq + steps - 1);          // pages of every position the batch may write, before it is enqueued
                decode_steps(e, env, enq, steps);
                enq += steps;
                decoded = true;
            }
            if (decoded) HIP_CHECK(hipEventRecord(ph_ev[4], st));
            HIP_CHECK(hipMemcpyAsync(h_ctl, d_ctl, sizeof(GenCtl), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(h_out_ids, d_out_ids, (size_t)enq * sizeof(int), hipMemcpyDeviceToHost, st));
            if (scores_on) HIP_CHECK(hipMemcpyAsync(h_scores, d_scores, (size_t)enq * sizeof(float), hipMemcpyDeviceToHost, st));
            if (scores_on && allow_on) HIP_CHECK(hipMemcpyAsync(h_alp, d_alp, (size_t)enq * allow_n * sizeof(float), hipMemcpyDeviceToHost, st));
            if (ent_on) HIP_CHECK(hipMemcpyAsync(h_ent, d_ent, (size_t)enq * sizeof(float), hipMemcpyDeviceToHost, st));
            if (topk) {
                HIP_CHECK(hipMemcpyAsync(h_topi, d_topi, (size_t)enq * topk * sizeof(int), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipMemcpyAsync(h_topl, d_topl, (size_t)enq * topk * sizeof(float), hipMemcpyDeviceToHost, st));
            }
            HIP_CHECK(hipMemcpyAsync(h_top2, d_top2, 2 * sizeof(float), hipMemcpyDeviceToHost, st));
            if (persistent_on) HIP_CHECK(hipMemcpyAsync(h_giveup, dl_giveup, sizeof(unsigned), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            LAUNCH_CHECK("generate");
            if (persistent_on && h_giveup[0]) {
                const unsigned code = h_giveup[0];
                h_giveup[0] = 0;
                HIP_CHECK(hipMemsetAsync(dl_giveup, 0, sizeof(unsigned), st));
                char msg[200];
                snprintf(msg, sizeof(msg), "persistent decode layer: a hand-off wait timed out (code 0x%x); the turn's results are invalid (is another process using the GPU?)", code);
                REQUIRE(false, msg);
            }
            n = h_ctl->count;
            done = h_ctl->done != 0;
            REQUIRE(n >= 1 && n <= enq, "generation state out of range");
            require_finite_tokens(h_out_ids, n);
            if (done) break;
            REQUIRE(steps > 0, "sequence exceeds max_positions during decode");
        }
        for (int k = 0; k < n; ++k) out[k] = h_out_ids[k];
        if (scores_on) { last_scores.assign(h_scores, h_scores + n); last_scores_valid = true; }      // (the draft modes are off: every id left the scored arg-max step)
        if (scores_on && allow_on) { last_alp.assign(h_alp, h_alp + (size_t)n * allow_n); last_alp_n = allow_n; last_alp_valid = true; }
        if (ent_on) { last_ent.assign(h_ent, h_ent + n); last_ent_valid = true; }
        if (topk) {
            last_topi.assign(h_topi, h_topi + (size_t)n * topk); last_topl.assign(h_topl, h_topl + (size_t)n * topk);
            last_topk = topk; last_topk_valid = true;
        }
        e.kv_len = L + n - 1;             // EOS (or the last token) is appended to the ids but never fed
        add_phase(1, 2, 3);
        settle_vision();
        if (decoded) add_phase(2, 3, 4);
        n_generated = n;
        const int singles = n - vtokens - head_tokens;      // (the prefill's own token counts in none of the draft counters)
        st_vtokens += vtokens; st_single += singles;
        top2_stale = (vtokens > 0 || drafted) && singles == 0;
        top2_sampled = smp_on;
        if (smp_on) env_draws[env] += n;
        *n_out = n;
        return singles;
    }

    // ------------------------------------------------------------------------------- group sampling (svln_generate_group)
    // the refusals of a group turn that need no state of the env (svln_turn_group checks them before it encodes a frame)
    void group_refusals(int env, int n_seq) {
        env_at(env);
        REQUIRE(n_seq >= 2 && n_seq <= MAXB, "svln_generate_group: n_seq must be 2 .. 8");
        refuse(C_GENERATE_GROUP);
    }
    // The plan of a turn form that shares one prefill: P cached rows, L rows in all, Tn = L - P rows to prefill, limit = min(max_new, cap)
    // ids after them (emitted or fed; the last one is never fed), q0 = the page L falls in, n_tail = the private pages of a fork from q0
    // on, env_need = the pages the env itself still lacks.  Issues the refusals the forms share, in the order they always had; arg_fault
    // (the form's own argument fault, if it found one: the text after `who`) is reported in its old place.  Nothing is launched or changed.
    struct TurnPlan { int P, L, Tn, limit, q0, n_tail, env_need; };
    static int fork_tail_pages(int L, int limit) { return limit == 1 ? 0 : (L + limit - 1 + PAGE - 1) / PAGE - L / PAGE; }
    TurnPlan plan_turn(const Env& e, const char* who, int max_new, int cap, const char* limit_text, const char* arg_fault = nullptr) {
        REQUIRE(weights_missing() == 0, g_err);
        TurnPlan p;
        p.P = e.kv_len; p.L = e.n_embeds; p.Tn = p.L - p.P; p.limit = max_new < cap ? max_new : cap;
        REQUIRE(p.Tn >= 1, "nothing to prefill: inputs_embeds not longer than the KV cache");
        REQUIRE(max_new >= 1 && cap >= 1, "max_new_tokens must be >= 1");
        REQUIRE(!arg_fault, std::string(who) + arg_fault);
        REQUIRE((int64_t)p.L + p.limit - 1 <= c.max_positions, std::string(who) + ": n_embeds + " + limit_text + " - 1 exceeds max_positions");
        p.q0 = p.L / PAGE;
        p.n_tail = fork_tail_pages(p.L, p.limit);
        p.env_need = std::max((p.limit == 1 ? (p.L + PAGE - 1) / PAGE : p.q0 + p.n_tail) - e.n_pages, 0);
        return p;
    }
    std::vector<int> fork_host[MAXB];            // host copies of fork_tab (kept: an upload reads them after the call that wrote them)
    void ensure_fork_tab(int g) { if (!fork_tab[g]) { fork_tab[g] = dalloc<int>(pages_per_env, true); fork_host[g].assign(pages_per_env, 0); } }
    void upload_fork_dst(int n_dst) { HIP_CHECK(hipMemcpyAsync(d_fork_dst, h_fork_dst, (size_t)n_dst * sizeof(int), hipMemcpyHostToDevice, st)); }
    // h_fork_dst[0 .. n_dst) -> the device, then the ONE fork launch: page src_page of every layer's K and V^T pool to each listed page
    void fork_page_copy(int src_page, int n_dst) {
        upload_fork_dst(n_dst);
        launch_kv_page_copy<T>(st, d_pool_tab, 2 * c.layers, src_page, d_fork_dst, n_dst, (int64_t)nkv * PAGE * 128);
    }
    // The fork of the pending group grp (its L set): per sequence g >= 1 with tail_n[g] > 0 a table = the env's pages below q0 + tail_n[g]
    // private pages from q0 on (grp.tail[g]), uploaded to fork_tab[g]; then the partly filled page q0, if the prompt ends inside one.
    // fork_tables is the table half: it returns the number of forks, whose first private pages it leaves in h_fork_dst.
    void fork_tails(Env& e, int q0, const int* tail_n, int n_seq) {
        const int n_dst = fork_tables(e, q0, tail_n, n_seq);
        if (grp.L % PAGE != 0 && n_dst > 0) fork_page_copy(e.pages[q0], n_dst);      // one launch for every layer, both pools, all forks
    }
    int fork_tables(Env& e, int q0, const int* tail_n, int n_seq) {
        int n_dst = 0;
        for (int g = 1; g < n_seq; ++g) {
            if (tail_n[g] == 0) continue;
            std::vector<int>& tab = fork_host[g];
            for (int i = 0; i < q0; ++i) tab[i] = e.pages[i];
            for (int i = 0; i < tail_n[g]; ++i) {
                REQUIRE(!free_pages.empty(), "KV page pool exhausted");
                grp.tail[g].push_back(free_pages.back());
                free_pages.pop_back();
                tab[q0 + i] = grp.tail[g][i];
            }
            HIP_CHECK(hipMemcpyAsync(fork_tab[g], tab.data(), (size_t)(q0 + tail_n[g]) * sizeof(int), hipMemcpyHostToDevice, st));
            h_fork_dst[n_dst++] = grp.tail[g][0];
        }
        return n_dst;
    }
    void generate_group(int env, int n_seq, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out) override {
        group_refusals(env, n_seq);
        Env& e = envs[env];
        REQUIRE(out && n_out, "svln_generate_group: null output pointer");
        const TurnPlan pl = plan_turn(e, "svln_generate_group", max_new, cap, "min(max_new_tokens, out_cap)",
                                      n_eos >= 0 && (n_eos == 0 || eos) ? nullptr : ": null eos list");
        const int P = pl.P, L = pl.L, Tn = pl.Tn, limit = pl.limit, q0 = pl.q0, n_tail = pl.n_tail;      // limit: tokens each sequence may emit
        REQUIRE((int64_t)free_pages.size() >= (int64_t)pl.env_need + (int64_t)(n_seq - 1) * n_tail,
                "svln_generate_group: the free KV pages cannot hold the env's own pages and (n_seq - 1) x the tail pages of the fork");
        // ---- nothing was launched or changed up to here
        disarm_draft(env);
        invalidate_last_results();
        int B = 2; while (B < n_seq) B <<= 1;
        for (int g = 1; g < n_seq; ++g) ensure_fork_tab(g);
        grp = Group();
        grp.env = env; grp.n_seq = n_seq; grp.L = L; grp.q0 = q0; grp.n_tail = n_tail;
        grp.scored = scores_on; grp.alp_n = scores_on && allow_on ? allow_n : 0;
        std::vector<std::vector<int64_t>> ids(n_seq);
        bool stopped[MAXB] = {false}; int last_tok[MAXB] = {0};
        // the host's stop rule on head row `row` of sequence g: EOS id (appended, never fed), limit, a non-finite arg-max
        auto accept = [&](int g, int row) {
            const int tok = h_tok_b[row];
            require_finite_tokens(&tok, 1);
            ids[g].push_back(tok);
            if (grp.scored) grp.scores[g].push_back(h_score_b[row]);
            if (grp.alp_n > 0) grp.alp[g].insert(grp.alp[g].end(), h_alp_b + (size_t)row * grp.alp_n, h_alp_b + (size_t)(row + 1) * grp.alp_n);
            last_tok[g] = tok;
            bool stop = (int)ids[g].size() >= limit;
            for (int k = 0; k < n_eos; ++k) stop |= eos[k] == tok;
            stopped[g] = stop;
        };
        // the one synchronisation of a pass: ids (and scores) of its B head rows, then the phase timer
        auto read_rows = [&](int phase) {
            HIP_CHECK(hipEventRecord(ph_ev[3], st));
            HIP_CHECK(hipMemcpyAsync(h_tok_b, d_tok_b, B * sizeof(int), hipMemcpyDeviceToHost, st));
            if (scores_on) HIP_CHECK(hipMemcpyAsync(h_score_b, d_score_b, B * sizeof(float), hipMemcpyDeviceToHost, st));
            if (scores_on && allow_on) HIP_CHECK(hipMemcpyAsync(h_alp_b, d_alp_b, (size_t)B * allow_n * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            LAUNCH_CHECK("generate_group");
            add_phase(phase, 2, 3);
            settle_vision();
        };
        auto upload_streams = [&]() {
            HIP_CHECK(hipMemcpyAsync(d_smp, h_smp, B * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d_smp + SMP_ROWS, h_smp + SMP_ROWS, B * sizeof(int), hipMemcpyHostToDevice, st));
        };
        try {
            // prefill: svln_generate's, launch for launch
            ensure_pages(e, L);
            HIP_CHECK(hipEventRecord(ph_ev[2], st));
            prefill(e, P, Tn);
            e.kv_len = L;
            // token 0: the last prefill row B times through the scheduler's head; row g draws from stream env + g * max_envs (pad rows replay row 0)
            const T* last = x + (size_t)(Tn - 1) * H;
            for (int k = 0; k < B; ++k)
                HIP_CHECK(hipMemcpyAsync(last_rows + (size_t)k * H, last, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
            for (int k = 0; k < B; ++k) { h_smp[k] = env + (k < n_seq ? k : 0) * c.max_envs; h_smp[SMP_ROWS + k] = env_draws[env]; }
            upload_streams();
            head_batched(last_rows, B);
            for (int g = 0; g < n_seq; ++g) tap_copy(xn + (size_t)g * H, 0, g);
            // fork: the env's own tail pages, then per sequence g >= 1 a table = the env's pages below q0 + private pages from q0 on
            if (limit > 1) ensure_pages(e, L + limit - 1);
            int tail_n[MAXB];
            std::fill(tail_n, tail_n + MAXB, n_tail);
            fork_tails(e, q0, tail_n, n_seq);
            read_rows(1);
            for (int g = 0; g < n_seq; ++g) accept(g, g);
            // decode: the scheduler's pure batched step; a finished sequence's row and every pad row replay the first live row
            for (int t = 0; t + 1 < limit; ++t) {
                int first = -1;
                for (int g = n_seq - 1; g >= 0; --g) if (!stopped[g]) first = g;
                if (first < 0) break;
                for (int k = 0; k < B; ++k) {
                    const int g = k < n_seq && !stopped[k] ? k : first;
                    h_slots[k].page_table = g == 0 ? e.d_pages : fork_tab[g]; h_slots[k].pos = L + t; h_slots[k].pad = 0;
                    h_tok_b[k] = last_tok[g];
                    h_smp[k] = env + g * c.max_envs; h_smp[SMP_ROWS + k] = env_draws[env] + t + 1;
                }
                HIP_CHECK(hipEventRecord(ph_ev[2], st));
                HIP_CHECK(hipMemcpyAsync(d_slots, h_slots, B * sizeof(DecodeSlot), hipMemcpyHostToDevice, st));
                HIP_CHECK(hipMemcpyAsync(d_tok_b, h_tok_b, B * sizeof(int), hipMemcpyHostToDevice, st));
                upload_streams();
                batched_step(B, false);
                for (int g = 0; g < n_seq; ++g) if (!stopped[g]) tap_copy(xn + (size_t)g * H, t + 1, g);
                read_rows(2);
                for (int g = 0; g < n_seq; ++g) if (!stopped[g]) accept(g, g);
            }
        } catch (...) {
            // every fork page goes back to the pool, no group is pending; the env is as after a failed svln_generate
            (void)hipStreamSynchronize(st);
            drop_group();
            throw;
        }
        int longest = 0;
        for (int g = 0; g < n_seq; ++g) {
            const int n = (int)ids[g].size();
            for (int k = 0; k < n; ++k) out[(size_t)g * cap + k] = ids[g][k];
            n_out[g] = grp.n_out[g] = n;
            longest = std::max(longest, n);
        }
        env_draws[env] += longest;        // every stream of the group has used draws [counter, counter + its length): none is used twice
        e.kv_len = L;                     // until svln_group_select
        n_generated = 0;                  // (the single-env tap rows were overwritten)
        top2_sampled = true;
        grp.pending = true;
    }
    void turn_group(const svln_turn_args& a, int n_seq, int64_t* out, int cap, int32_t* n_out) override {
        group_refusals(a.env, n_seq);
        REQUIRE(a.ids && a.n_ids >= 1 && out && n_out, "svln_turn_group: null / empty argument");
        begin_turn(a);                    // (the refusals above came first: they leave an armed draft in place)
        generate_group(a.env, n_seq, a.max_new_tokens, a.eos_ids, a.n_eos, out, cap, n_out);
    }
    // ------------------------------------------------------------------------------- beam turns (svln_generate_beams)
    // The W most probable turns of one prompt.  The prefill, the fork of the partly filled page and the batched step are the group turn's;
    // the head of every step is the EPI_ARGMAX_LSE_TOPK form at k = W (scores_on / topk / trunc_k are overridden for the call), whose
    // lists d_topi_b / d_topl_b [row = rank][W] feed beam_select_kernel.  The hypothesis set lives in bm_hdr / bm_ids / bm_lps (two
    // states, swapped every step).  Pages: 2 W sets of n_tail tail pages (set 0 = the env's own), each with a device page table
    // beam_tab[s] = the env's pages below q0 + the set's pages; the select kernel hands the sets out and lists the (src, dst) pages of
    // every child that cannot keep its parent's set, kv_page_gather_kernel copies them.  Sources are held by the old set, destinations
    // are not, so nothing is permuted in place.  One synchronisation per step reads the record, the new header and the lists.
    int* beam_tab[2 * BEAM_MAX_W] = {nullptr};
    std::vector<int> beam_set[2 * BEAM_MAX_W];               // the tail pages of every set during a call (set 0: the env's own)
    struct BeamTrace { int W = 0; std::vector<int32_t> list_ids, rec; std::vector<float> list_lps; int steps = 0; };
    BeamTrace beam_trace_last;
    void beam_refusals(int env, int W) {
        const char* who = "svln_generate_beams";
        env_at(env);
        REQUIRE(W >= 1 && W <= BEAM_MAX_W, std::string(who) + ": n_beams must be 1 .. 8");
        refuse(C_GENERATE_BEAMS, who, false, 0);
        REQUIRE(!allow_on || allow_n >= W, std::string(who) + ": the allowed list (svln_set_allowed_tokens) is shorter than n_beams");
        refuse(C_GENERATE_BEAMS, who, false, 1);
        REQUIRE((size_t)H * sizeof(float) <= (size_t)GEMV_ROWS_TOPK_MAX_LDS, std::string(who) + ": the hidden size is too large for the candidate form of the lm_head GEMV");
        refuse(C_GENERATE_BEAMS, who, false, 2);
    }
    void generate_beams(int env, int W, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out, float* scores) override {
        const char* who = "svln_generate_beams";
        beam_refusals(env, W);
        Env& e = envs[env];
        REQUIRE(out && n_out && scores, std::string(who) + ": null output pointer");
        const TurnPlan pl = plan_turn(e, who, max_new, cap, "min(max_new_tokens, out_cap)",
                                      n_eos >= 0 && n_eos <= std::max(V, 64) && (n_eos == 0 || eos) ? nullptr : ": null eos list / too many eos ids");
        const int P = pl.P, L = pl.L, Tn = pl.Tn, limit = pl.limit, q0 = pl.q0, n_tail = pl.n_tail;
        REQUIRE(n_tail <= BEAM_CP_MAX, std::string(who) + ": a turn of more than 8 tail pages does not fit the page lists of a beam step");
        REQUIRE((int64_t)free_pages.size() >= (int64_t)pl.env_need + (int64_t)(2 * W - 1) * n_tail,
                std::string(who) + ": the free KV pages cannot hold the env's own pages and (2 n_beams - 1) x the tail pages of the hypotheses");
        // ---- nothing was launched or changed up to here
        disarm_draft(env);
        invalidate_last_results();
        ensure_topk_buffers();
        ensure_beam_buffers();
        int B = 2; while (B < W) B <<= 1;
        const int n_sets = 2 * W;
        // the head of the call: restored however the call ends (the step graphs are keyed on these three)
        struct HeadOverride {
            bool& scores; int &topk, &trunc; const bool scores0; const int topk0, trunc0;
            ~HeadOverride() { scores = scores0; topk = topk0; trunc = trunc0; }
        } held{scores_on, topk, trunc_k, scores_on, topk, trunc_k};
        scores_on = true; topk = W; trunc_k = 0;
        BeamTrace tr; tr.W = W;
        BeamHdr hh;
        std::vector<int> anc[BEAM_MAX_W];                 // per hypothesis: the head row that gave each of its ids (parity taps)
        int rec[BEAM_REC];
        int cur = 0;
        auto read_step = [&](int rows, int phase) {
            HIP_CHECK(hipEventRecord(ph_ev[3], st));
            HIP_CHECK(hipStreamSynchronize(st));
            LAUNCH_CHECK("generate_beams");
            HIP_CHECK(hipMemcpy(rec, bm_rec, sizeof(rec), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(&hh, bm_hdr[cur], sizeof(BeamHdr), hipMemcpyDeviceToHost));
            const size_t o = tr.list_ids.size();
            tr.list_ids.resize(o + BEAM_MAX_W * BEAM_MAX_W, -1); tr.list_lps.resize(o + BEAM_MAX_W * BEAM_MAX_W, -INFINITY);
            std::vector<int> li((size_t)rows * W); std::vector<float> ll((size_t)rows * W);
            HIP_CHECK(hipMemcpy(li.data(), d_topi_b, li.size() * sizeof(int), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(ll.data(), d_topl_b, ll.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (int r = 0; r < rows; ++r)
                for (int j = 0; j < W; ++j) { tr.list_ids[o + r * BEAM_MAX_W + j] = li[(size_t)r * W + j]; tr.list_lps[o + r * BEAM_MAX_W + j] = ll[(size_t)r * W + j]; }
            tr.rec.insert(tr.rec.end(), rec, rec + BEAM_REC);
            ++tr.steps;
            add_phase(phase, 2, 3);
            settle_vision();
            REQUIRE(hh.n >= 0 && hh.n <= W && rec[0] == hh.n && rec[3] >= 0 && rec[3] <= BEAM_MAX_W * BEAM_CP_MAX, "beam state out of range");
            for (int q = 0; q < hh.n; ++q) REQUIRE(hh.set_of[q] >= 0 && hh.set_of[q] < n_sets && rec[4 + q] >= 0 && rec[4 + q] < BEAM_MAX_W, "beam state out of range");
        };
        auto select = [&](int n_cp) {
            BeamSelectArgs a;
            a.list_ids = d_topi_b; a.list_lps = d_topl_b; a.in = bm_hdr[cur]; a.in_ids = bm_ids[cur]; a.in_lps = bm_lps[cur];
            a.out = bm_hdr[cur ^ 1]; a.out_ids = bm_ids[cur ^ 1]; a.out_lps = bm_lps[cur ^ 1];
            a.len_cap = bm_len_cap; a.W = W; a.limit = limit; a.n_eos = n_eos; a.B = B; a.n_cp = n_cp; a.set_stride = BEAM_CP_MAX;
            a.eos = bm_eos; a.set_pages = bm_sets; a.tok_b = d_tok_b; a.pair_src = bm_pair_src; a.pair_dst = bm_pair_dst; a.rec = bm_rec;
            launch_beam_select(st, a);
            cur ^= 1;
        };
        // the ancestry of the new set from the record: child c's rows are its parent's, plus the row that listed its last id
        auto follow = [&](int row_of_parent_is_rank) {
            std::vector<int> next[BEAM_MAX_W];
            for (int q = 0; q < hh.n; ++q) {
                const int pr = rec[4 + q];
                next[q] = anc[pr];
                if ((int)next[q].size() < hh.len[q]) next[q].push_back(row_of_parent_is_rank ? pr : 0);
            }
            for (int q = 0; q < BEAM_MAX_W; ++q) anc[q].swap(next[q]);
        };
        try {
            HIP_CHECK(hipStreamSynchronize(st));
            {   // the root of step 0, the EOS list, the page sets
                BeamHdr root; std::memset(&root, 0, sizeof(root)); root.n = 1;
                HIP_CHECK(hipMemcpy(bm_hdr[0], &root, sizeof(BeamHdr), hipMemcpyHostToDevice));
                std::vector<int> ev(n_eos);
                for (int k = 0; k < n_eos; ++k) ev[k] = eos[k] >= 0 && eos[k] < V ? (int)eos[k] : -2;      // ids outside the vocabulary never match
                if (n_eos) HIP_CHECK(hipMemcpy(bm_eos, ev.data(), (size_t)n_eos * sizeof(int), hipMemcpyHostToDevice));
            }
            // prefill: svln_generate's, launch for launch
            ensure_pages(e, L);
            HIP_CHECK(hipEventRecord(ph_ev[2], st));
            prefill(e, P, Tn);
            e.kv_len = L;
            const T* last = x + (size_t)(Tn - 1) * H;
            for (int k = 0; k < B; ++k)
                HIP_CHECK(hipMemcpyAsync(last_rows + (size_t)k * H, last, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
            head_batched(last_rows, B);
            tap_copy(xn, 0, 0);
            // the page sets: set 0 = the env's own tail, the others fresh pages; one device table each
            if (limit > 1) ensure_pages(e, L + limit - 1);
            if (n_tail > 0) {
                std::vector<int> flat((size_t)2 * BEAM_MAX_W * BEAM_CP_MAX, 0), tab(pages_per_env, 0);
                for (int s = 0; s < n_sets; ++s) {
                    beam_set[s].clear();
                    for (int i = 0; i < n_tail; ++i) {
                        if (s == 0) { beam_set[s].push_back(e.pages[q0 + i]); continue; }
                        REQUIRE(!free_pages.empty(), "KV page pool exhausted");
                        beam_set[s].push_back(free_pages.back());
                        free_pages.pop_back();
                    }
                    if (!beam_tab[s]) beam_tab[s] = dalloc<int>(pages_per_env);       // (not zeroed: the stream's memset would land after the blocking upload below)
                    for (int i = 0; i < q0; ++i) tab[i] = e.pages[i];
                    for (int i = 0; i < n_tail; ++i) { tab[q0 + i] = beam_set[s][i]; flat[(size_t)s * BEAM_CP_MAX + i] = beam_set[s][i]; }
                    HIP_CHECK(hipMemcpy(beam_tab[s], tab.data(), (size_t)(q0 + n_tail) * sizeof(int), hipMemcpyHostToDevice));
                }
                HIP_CHECK(hipMemcpy(bm_sets, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
                if (L % PAGE != 0 && W > 1) {       // the partly filled page: the group turn's fork, to the sets the step-0 children take
                    for (int s = 1; s < W; ++s) h_fork_dst[s - 1] = beam_set[s][0];
                    fork_page_copy(e.pages[q0], W - 1);
                }
            }
            select(0);
            read_step(1, 1);
            REQUIRE(hh.n >= 1, "non-finite logits: the arg-max found no finite value (check the weights / fp8 scales)");
            follow(0);
            for (int t = 0; rec[1] > 0; ++t) {
                REQUIRE(t + 1 < limit && n_tail > 0, "beam state out of range");
                int first = -1;
                for (int q = hh.n - 1; q >= 0; --q) if (!hh.fin[q]) first = q;
                REQUIRE(first >= 0, "beam state out of range");
                for (int k = 0; k < B; ++k) {
                    const int q = k < hh.n && !hh.fin[k] ? k : first;
                    h_slots[k].page_table = beam_tab[hh.set_of[q]]; h_slots[k].pos = L + t; h_slots[k].pad = 0;
                }
                HIP_CHECK(hipEventRecord(ph_ev[2], st));
                HIP_CHECK(hipMemcpyAsync(d_slots, h_slots, B * sizeof(DecodeSlot), hipMemcpyHostToDevice, st));
                batched_step(B, false);
                // (tokens 0 .. 7 are tapped, as svln_get_hidden_group reads them: a later step would overwrite tap row 7 with a row the
                // rank reorder below cannot place)
                for (int q = 0; q < hh.n && t + 1 < 8; ++q) if (!hh.fin[q]) tap_copy(xn + (size_t)q * H, t + 1, q);
                select((L + t) / PAGE - q0 + 1);
                read_step(hh.n, 2);          // (hh still holds the old set while the argument is evaluated)
                follow(1);
                if (rec[3] > 0) launch_kv_page_gather<T>(st, d_pool_tab, 2 * c.layers, bm_pair_src, bm_pair_dst, rec[3], (int64_t)nkv * PAGE * 128);
            }
            HIP_CHECK(hipStreamSynchronize(st));
            LAUNCH_CHECK("generate_beams");
            // the result: ids, log-probabilities and scores of the final set, in rank order
            std::vector<int> ids((size_t)BEAM_MAX_W * bm_len_cap); std::vector<float> lps((size_t)BEAM_MAX_W * bm_len_cap);
            HIP_CHECK(hipMemcpy(ids.data(), bm_ids[cur], ids.size() * sizeof(int), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(lps.data(), bm_lps[cur], lps.size() * sizeof(float), hipMemcpyDeviceToHost));
            grp = Group();
            grp.env = env; grp.n_seq = hh.n; grp.L = L; grp.q0 = q0; grp.n_tail = n_tail; grp.scored = true; grp.alp_n = 0;
            for (int g = 0; g < W; ++g) { n_out[g] = 0; scores[g] = -INFINITY; }
            for (int g = 0; g < hh.n; ++g) {
                const int n = hh.len[g];
                REQUIRE(n >= 1 && n <= limit && hh.fin[g], "beam state out of range");
                for (int k = 0; k < n; ++k) {
                    const int tok = ids[(size_t)g * bm_len_cap + k];
                    REQUIRE(tok >= 0 && tok < V, "beam state out of range");
                    out[(size_t)g * cap + k] = tok;
                    grp.scores[g].push_back(lps[(size_t)g * bm_len_cap + k]);
                }
                n_out[g] = grp.n_out[g] = n; scores[g] = hh.score[g];
            }
            // pages: rank 0's set becomes the env's tail, rank g's set the group's tail[g], every other set goes back to the pool
            if (n_tail > 0) {
                bool used[2 * BEAM_MAX_W] = {false};
                for (int g = 0; g < hh.n; ++g) used[hh.set_of[g]] = true;
                for (int i = 0; i < n_tail; ++i) e.pages[q0 + i] = beam_set[hh.set_of[0]][i];
                HIP_CHECK(hipMemcpyAsync(e.d_pages + q0, e.pages.data() + q0, (size_t)n_tail * sizeof(int), hipMemcpyHostToDevice, st));
                for (int g = 1; g < hh.n; ++g) grp.tail[g] = beam_set[hh.set_of[g]];
                for (int s = 0; s < n_sets; ++s) {
                    if (!used[s]) for (int p : beam_set[s]) free_pages.push_back(p);
                    beam_set[s].clear();
                }
            }
            if (taps_on) {      // the parity taps in rank order: token i of rank g left head row anc[g][i] of step i
                const size_t n_tap = (size_t)8 * MAXB * H;
                if (!bm_tap) bm_tap = dalloc<T>(n_tap);
                HIP_CHECK(hipMemcpyAsync(bm_tap, hid_tap, n_tap * sizeof(T), hipMemcpyDeviceToDevice, st));
                for (int g = 0; g < hh.n; ++g)
                    for (int i = 0; i < (int)anc[g].size() && i < 8; ++i)
                        HIP_CHECK(hipMemcpyAsync(hid_tap + (size_t)(i * MAXB + g) * H, bm_tap + (size_t)(i * MAXB + anc[g][i]) * H, (size_t)H * sizeof(T), hipMemcpyDeviceToDevice, st));
            }
            HIP_CHECK(hipStreamSynchronize(st));
        } catch (...) {
            // every page of sets 1 .. goes back to the pool, no group is pending; the env is as after a failed svln_generate
            (void)hipStreamSynchronize(st);
            for (int s = 1; s < 2 * BEAM_MAX_W; ++s) { for (int p : beam_set[s]) free_pages.push_back(p); beam_set[s].clear(); }
            beam_set[0].clear();
            grp = Group();
            throw;
        }
        beam_trace_last = std::move(tr);
        e.kv_len = L;                     // until svln_group_select
        n_generated = 0;                  // (the single-env tap rows were overwritten)
        top2_stale = true;
        top2_sampled = false;
        grp.pending = true;
    }
    void turn_beams(const svln_turn_args& a, int W, int64_t* out, int cap, int32_t* n_out, float* scores) override {
        beam_refusals(a.env, W);
        REQUIRE(a.ids && a.n_ids >= 1 && out && n_out && scores, "svln_turn_beams: null / empty argument");
        begin_turn(a);                    // (the refusals above came first: they leave an armed draft in place)
        generate_beams(a.env, W, a.max_new_tokens, a.eos_ids, a.n_eos, out, cap, n_out, scores);
    }
    void beam_trace(int cap_steps, int32_t* n_steps, int32_t* width, int32_t* list_ids, float* list_lps, int32_t* records) override {
        const BeamTrace& tr = beam_trace_last;
        REQUIRE(tr.steps > 0, "svln_beam_trace: no beam turn has run");
        const int m = std::min(tr.steps, cap_steps);
        for (int q = 0; q < m * BEAM_MAX_W * BEAM_MAX_W; ++q) { list_ids[q] = tr.list_ids[q]; list_lps[q] = tr.list_lps[q]; }
        for (int q = 0; q < m * BEAM_REC; ++q) records[q] = tr.rec[q];
        *n_steps = tr.steps; *width = tr.W;
    }
    // ------------------------------------------------------------------------------- candidate scoring (svln_generate_candidates)
    // n_seq caller-given continuations of ONE prompt: the prompt is prefilled once (svln_generate's prefill), forked as a group turn forks
    // it, and the fed ids of all sequences go through the batched step's products in passes of n_seq x r row slots with the batched verify
    // attention; the head rows (the prompt's last row once per sequence, every fed row) are normed into bf_xn and scored by the
    // EPI_TARGET head of the scheduler's forced jobs.  The result is a pending group whose sequence g has fed n_g - 1 ids.
    static constexpr int CAND_PASSES = BFORCED_MAX - 1, CAND_FEED = CAND_PASSES * 32;
    int *d_cfeed = nullptr, *h_cfeed = nullptr;                   // fed ids of every pass: [pass][B]
    DecodeSlot *d_cslots = nullptr, *h_cslots = nullptr;          // slots of every pass: [pass][MAXB]
    void ensure_cand_buffers() {
        if (d_cfeed) return;
        d_cfeed = dalloc<int>(CAND_FEED, true); d_cslots = dalloc<DecodeSlot>((size_t)CAND_PASSES * MAXB, true);
        HIP_CHECK(hipHostMalloc((void**)&h_cfeed, CAND_FEED * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_cslots, (size_t)CAND_PASSES * MAXB * sizeof(DecodeSlot)));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // rows of a sequence per scoring pass
    int cand_rows_per_pass(int n_seq) const { return std::min(32 / (nq / nkv), 32 / n_seq); }
    // every refusal that needs no state of the env's rows (svln_turn_candidates checks them before it encodes a frame)
    void cand_refusals(int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos, int n_eos,
                       const char* who = "svln_generate_candidates") {
        env_at(env);
        REQUIRE(n_seq >= 2 && n_seq <= MAXB, std::string(who) + ": n_seq must be 2 .. 8");
        REQUIRE(ids && lens, std::string(who) + ": null id list / lengths");
        for (int g = 0; g < n_seq; ++g) REQUIRE(lens[g] >= 1 && lens[g] <= FORCED_MAX, std::string(who) + ": a sequence length (lens) must be 1 .. 32");
        refuse(C_GENERATE_CANDIDATES, who);
        int off = 0;
        for (int g = 0; g < n_seq; ++g) { forced_refusals(env, ids + off, lens[g], eos, n_eos, who); off += lens[g]; }
    }
    void generate_candidates(int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos, int n_eos, float* logprobs,
                             int64_t* greedy_ids, float* greedy_logprobs) override {
        candidates_call(env, n_seq, ids, lens, eos, n_eos, logprobs, greedy_ids, greedy_logprobs, false);
    }
    // svln_generate_candidates_folded: the same call with the rows of scoring pass 0 folded into the prefill pass (Fold, prefill_rows):
    // the tables of the fork are built BEFORE the prefill, every layer's launch_rope_kv mirrors the prompt's rows of page q0 into the
    // forks' first private pages (rows of earlier turns in that page: ONE fork_page_copy before the prefill), and the fork launch after
    // the prefill is gone.  Passes 1 .. are unchanged.  Candidates of one id each feed nothing: the unfolded call, launch for launch.
    void generate_candidates_folded(int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos, int n_eos, float* logprobs,
                                    int64_t* greedy_ids, float* greedy_logprobs) override {
        candidates_call(env, n_seq, ids, lens, eos, n_eos, logprobs, greedy_ids, greedy_logprobs, true);
    }
    void candidates_call(int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos, int n_eos, float* logprobs,
                         int64_t* greedy_ids, float* greedy_logprobs, bool folded) {
        const char* who = folded ? "svln_generate_candidates_folded" : "svln_generate_candidates";
        Env& e = env_at(env);
        disarm_draft(env);              // consumed by this call, as svln_generate_forced consumes it
        REQUIRE(logprobs && greedy_ids && greedy_logprobs, std::string(who) + ": null output pointer");
        cand_refusals(env, n_seq, ids, lens, eos, n_eos, who);
        int n_max = 0, nf = 0, off[MAXB + 1] = {0};
        for (int g = 0; g < n_seq; ++g) { n_max = std::max(n_max, (int)lens[g]); off[g + 1] = off[g] + lens[g]; }
        nf = off[n_seq];
        const TurnPlan pl = plan_turn(e, who, n_max, n_max, "max(lens)");
        const int P = pl.P, L = pl.L, Tn = pl.Tn, q0 = pl.q0;
        // (the plan's page counts are those of the longest sequence: here the env feeds lens[0] ids and every fork its own)
        int tail_n[MAXB] = {0};
        int64_t need = std::max((L + lens[0] - 1 + PAGE - 1) / PAGE - e.n_pages, 0);
        for (int g = 1; g < n_seq; ++g) { tail_n[g] = fork_tail_pages(L, lens[g]); need += tail_n[g]; }
        REQUIRE((int64_t)free_pages.size() >= need,
                std::string(who) + ": the free KV pages cannot hold the env's own pages and the tail pages of the fork");
        const int r = cand_rows_per_pass(n_seq);
        const int passes = (n_max - 1 + r - 1) / r;
        const int Bu = n_seq * r, B = Bu >= batched_mfma_min ? Bu : (Bu <= 2 ? 2 : 4);
        REQUIRE(passes <= CAND_PASSES && passes * B <= CAND_FEED && nf <= BFORCED_ROWS && B <= c.max_positions, std::string(who) + ": workspace");
        const bool fold = folded && n_max >= 2;        // (nothing is fed otherwise)
        const int row0 = fold ? Tn : 0;                // the row of x that slot 0 of pass 0 is
        REQUIRE(!fold || (int64_t)Tn + Bu <= c.max_positions,
                std::string(who) + ": the row workspace (max_positions rows) cannot hold the prompt's new rows and n_seq x r candidate rows");
        ensure_bforced_buffers();
        ensure_cand_buffers();
        // ---- nothing was launched or changed up to here (but the armed draft)
        invalidate_last_results();
        for (int g = 1; g < n_seq; ++g) ensure_fork_tab(g);
        grp = Group();
        grp.env = env; grp.n_seq = n_seq; grp.L = L; grp.q0 = q0; grp.scored = true; grp.alp_n = allow_on ? allow_n : 0;
        for (int g = 1; g < n_seq; ++g) grp.n_tail = std::max(grp.n_tail, tail_n[g]);
        // head row lists.  Block 0: the prompt's last row once per sequence (target F_g[0]); block p + 1: the rows pass p fed, sequence by
        // sequence (row slot g r + j fed F_g[p r + j], target F_g[p r + j + 1]).  hrow[off[g] + i] = the head row that scores F_g[i].
        const HeadLists &h = bf_host, &d = bf_dev;
        std::vector<int> hrow(nf), base(passes + 2, 0);
        HIP_CHECK(hipStreamSynchronize(st));       // (the pinned lists of an earlier call are no longer being read)
        int k = 0;
        for (int g = 0; g < n_seq; ++g) { h.src[k] = Tn - 1; h.tap[k] = taps_on ? g : -1; h.tgt[k] = (int)ids[off[g]]; hrow[off[g]] = k; ++k; }
        base[1] = k;
        for (int p = 0; p < passes; ++p) {
            for (int q = 0; q < B; ++q) h_cfeed[p * B + q] = 0;
            for (int g = 0; g < n_seq; ++g) {
                const int lo = p * r, hi = std::min((p + 1) * r, (int)lens[g] - 1), cnt = std::max(hi - lo, 0);
                DecodeSlot& sl = h_cslots[p * MAXB + g];
                sl.page_table = g == 0 ? e.d_pages : fork_tab[g]; sl.pos = L + lo; sl.pad = cnt;
                for (int j = 0; j < cnt; ++j) {
                    const int i = lo + j + 1;       // the position of the turn this row scores
                    h_cfeed[p * B + g * r + j] = (int)ids[off[g] + lo + j];
                    h.src[k] = (p == 0 ? row0 : 0) + g * r + j;
                    // tap row min(i, 7); of the rows of one launch that share tap row 7 only the last is written (later passes overwrite it)
                    h.tap[k] = taps_on && (i < 7 || j == cnt - 1) ? (i < 7 ? i : 7) * MAXB + g : -1;
                    h.tgt[k] = (int)ids[off[g] + i];
                    hrow[off[g] + i] = k;
                    ++k;
                }
            }
            base[p + 2] = k;
        }
        REQUIRE(k == nf, std::string(who) + ": head row count");
        try {
            upload_head_lists(nf);
            if (passes > 0) {
                HIP_CHECK(hipMemcpyAsync(d_cfeed, h_cfeed, (size_t)passes * B * sizeof(int), hipMemcpyHostToDevice, st));
                HIP_CHECK(hipMemcpyAsync(d_cslots, h_cslots, (size_t)passes * MAXB * sizeof(DecodeSlot), hipMemcpyHostToDevice, st));
            }
            if (fold) {
                // the tables of the fork first; the prompt's rows of page q0 reach the forks' first pages layer by layer (the mirror list),
                // rows of earlier turns in that page by one copy now -- what it copies at positions >= P the stream overwrites
                HIP_CHECK(hipEventRecord(ph_ev[2], st));
                ensure_pages(e, L + lens[0] - 1);
                const int n_dst = fork_tables(e, q0, tail_n, n_seq);
                const int n_mirror = L % PAGE != 0 ? n_dst : 0;
                if (n_mirror > 0) { if (P > q0 * PAGE) fork_page_copy(e.pages[q0], n_dst); else upload_fork_dst(n_dst); }
                const Fold f{d_cfeed, d_cslots, n_seq, r, L + std::min(r, n_max - 1), q0, d_fork_dst, n_mirror};
                std::vector<Seg> segs{Seg{&e, P, Tn, 0}};
                prefill_rows(segs, Tn + Bu, 0, 0, &f);
                e.kv_len = L;
                // block 0 and the folded rows in one launch
                launch_rmsnorm_indexed<T>(st, x, final_norm, bf_xn, d.src, d.tap, hid_tap, base[2], H, c.rms_eps);
                HIP_CHECK(hipEventRecord(ph_ev[3], st));
            } else {
                // prefill: svln_generate's, launch for launch
                ensure_pages(e, L);
                HIP_CHECK(hipEventRecord(ph_ev[2], st));
                prefill(e, P, Tn);
                e.kv_len = L;
                launch_rmsnorm_indexed<T>(st, x, final_norm, bf_xn, d.src, d.tap, hid_tap, n_seq, H, c.rms_eps);
                HIP_CHECK(hipEventRecord(ph_ev[3], st));
                // fork: the env's own tail pages, then per sequence g >= 1 a table = the env's pages below q0 + private pages from q0 on
                ensure_pages(e, L + lens[0] - 1);
                fork_tails(e, q0, tail_n, n_seq);
            }
            // scoring passes: one sweep of the batched step's products each, then the final norm of the rows it fed
            for (int p = fold ? 1 : 0; p < passes; ++p) {
                const MultiPass mp{d_cfeed + p * B, d_cslots + (size_t)p * MAXB, n_seq, r, std::min(L + (p + 1) * r, L + n_max - 1)};
                decode_ops_batched(B, false, nullptr, &mp);
                const int cnt = base[p + 2] - base[p + 1];
                launch_rmsnorm_indexed<T>(st, x, final_norm, bf_xn + (size_t)base[p + 1] * H, d.src + base[p + 1], d.tap + base[p + 1], hid_tap, cnt, H, c.rms_eps);
            }
            head_target_chunks(nf);
            HIP_CHECK(hipEventRecord(ph_ev[4], st));
            HIP_CHECK(hipStreamSynchronize(st));
            LAUNCH_CHECK(folded ? "generate_candidates_folded" : "generate_candidates");
            require_finite_tokens(h.tok, nf);
            for (int g = 0; g < n_seq; ++g) {
                for (int i = 0; i < lens[g]; ++i) {
                    const int q = hrow[off[g] + i], o = off[g] + i;
                    greedy_ids[o] = h.tok[q]; greedy_logprobs[o] = h.score[q];
                    logprobs[o] = forced_score(q, (int)ids[o], h.lp, bf_host_alp);
                    if (allow_on) grp.alp[g].insert(grp.alp[g].end(), bf_host_alp + (size_t)q * allow_n, bf_host_alp + (size_t)(q + 1) * allow_n);
                    grp.scores[g].push_back(logprobs[o]);
                }
                grp.n_out[g] = lens[g];
            }
        } catch (...) {
            // every fork page goes back to the pool, no group is pending; the env is as after a failed svln_generate
            (void)hipStreamSynchronize(st);
            drop_group();
            throw;
        }
        add_phase(1, 2, 3);
        add_phase(2, 3, 4);
        settle_vision();
        e.kv_len = L;                     // until svln_group_select
        n_generated = 0;                  // (the single-env tap rows were overwritten)
        top2_stale = true;
        top2_sampled = false;
        grp.pending = true;
    }
    void turn_candidates(const svln_turn_args& a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs, int64_t* greedy_ids,
                         float* greedy_logprobs) override {
        env_at(a.env);
        begin_turn(a, [&] {
            REQUIRE(a.ids && a.n_ids >= 1 && logprobs && greedy_ids && greedy_logprobs, "svln_turn_candidates: null / empty argument");
            cand_refusals(a.env, n_seq, ids, lens, a.eos_ids, a.n_eos);
        });
        generate_candidates(a.env, n_seq, ids, lens, a.eos_ids, a.n_eos, logprobs, greedy_ids, greedy_logprobs);
    }
    void turn_candidates_folded(const svln_turn_args& a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs, int64_t* greedy_ids,
                                float* greedy_logprobs) override {
        env_at(a.env);
        begin_turn(a, [&] {
            REQUIRE(a.ids && a.n_ids >= 1 && logprobs && greedy_ids && greedy_logprobs, "svln_turn_candidates_folded: null / empty argument");
            cand_refusals(a.env, n_seq, ids, lens, a.eos_ids, a.n_eos, "svln_turn_candidates_folded");
        });
        generate_candidates_folded(a.env, n_seq, ids, lens, a.eos_ids, a.n_eos, logprobs, greedy_ids, greedy_logprobs);
    }
    // ------------------------------------------------------------------------------- multi-draft turns (svln_generate_drafts)
    // svln_generate with hints: up to 8 guessed id sequences of this turn ride ONE prefill pass in the folded candidates call's row layout
    // (Fold: sequence g on its own page table, page q0 mirrored into the forks), one indexed final norm and the arg-max head score the
    // prompt's last row and every fed row, draft_select_kernel applies the verify rule to every branch and picks the winner, the host
    // hands the winner's pages to the env and the single-step loop of svln_generate finishes the turn.  Every emitted token is the arg-max
    // of a row that was fed the true prefix, so no guess changes a greedy output.  Hints that cannot be used are ignored: the call is then
    // svln_generate itself.
    static constexpr int DRAFTS_MAX = MAXB, DRAFT_LEN_MAX = 32;
    int* d_dsel = nullptr; int* h_dsel = nullptr;      // [0 .. 8) k_g, [8 .. 12) the result record, [12], [13] passes / tokens (device counters)
    // calls, passes, tokens from passes, rows fed, turns finished in the pass, calls ignored, page handovers (winner >= 1), single steps
    int64_t st_drafts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void ensure_dsel_buffers() {
        if (d_dsel) return;
        d_dsel = dalloc<int>(16, true);
        HIP_CHECK(hipHostMalloc((void**)&h_dsel, 16 * sizeof(int)));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // The plan: how many of the drafts ride (G, trailing ones dropped while the row workspace or the free pages fall short, possibly to 0 =
    // the plain turn) and how many ids k[g] each feeds.  A pure function of the arguments and the env's counts; nothing is changed.
    struct DraftPlan { int G = 0, r = 0, k[DRAFTS_MAX] = {0}; };
    DraftPlan plan_drafts(const Env& e, int n_drafts, const int64_t* ids, const int32_t* lens, int limit, const int64_t* eos, int n_eos) const {
        DraftPlan p;
        const int L = e.n_embeds, Tn = L - e.kv_len;
        if (Tn < 1 || limit < 1) return p;            // (svln_generate refuses the call)
        for (int G = n_drafts; G >= 1; --G) {
            const int r = cand_rows_per_pass(G);
            int k[DRAFTS_MAX] = {0}, off = 0;
            int64_t need = 0;
            for (int g = 0; g < G; ++g) {
                int kg = std::max(std::min(std::min((int)lens[g], r), std::min(limit - 1, c.max_positions - L)), 0);
                for (int j = 0; j < kg; ++j) {
                    const int64_t id = ids[off + j];
                    bool cut = id < 0 || id >= V;                       // an id outside the vocabulary ends the draft
                    for (int q = 0; q < n_eos && !cut; ++q) cut = eos[q] == id;      // an EOS id is compared, never fed
                    if (cut) { kg = j; break; }
                }
                k[g] = kg; off += lens[g];
                need += g == 0 ? std::max((L + kg + PAGE - 1) / PAGE - e.n_pages, 0) : fork_tail_pages(L, kg + 1);
            }
            if ((int64_t)Tn + (int64_t)G * r > c.max_positions || need > (int64_t)free_pages.size()) continue;
            p.G = G; p.r = r;
            for (int g = 0; g < G; ++g) p.k[g] = k[g];
            break;
        }
        int fed = 0;
        for (int g = 0; g < p.G; ++g) fed += p.k[g];
        if (fed == 0) p.G = 0;                        // no draft with a usable first id
        return p;
    }
    void drafts_arg_check(const char* who_c, int n_drafts, const int64_t* ids, const int32_t* lens, const int64_t* out, const int32_t* n_out) {
        const std::string who(who_c);
        REQUIRE(n_drafts >= 0 && n_drafts <= DRAFTS_MAX, who + ": n_drafts must be 0 .. 8");
        REQUIRE(out && n_out, who + ": null output pointer");
        REQUIRE(n_drafts == 0 || lens, who + ": null draft lengths");
        int total = 0;
        for (int g = 0; g < n_drafts; ++g) {
            REQUIRE(lens[g] >= 0 && lens[g] <= DRAFT_LEN_MAX, who + ": a draft length (lens) must be 0 .. 32");
            total += lens[g];
        }
        REQUIRE(total == 0 || ids, who + ": null draft ids");
    }
    void generate_drafts(int env, int n_drafts, const int64_t* ids, const int32_t* lens, int max_new, const int64_t* eos, int n_eos, int64_t* out,
                         int cap, int32_t* n_out, int32_t* winner_out, int32_t* pass_tokens_out) override {
        const char* who = "svln_generate_drafts";
        Env& e = env_at(env);
        drafts_arg_check(who, n_drafts, ids, lens, out, n_out);
        REQUIRE(n_eos >= 0 && (n_eos == 0 || eos), std::string(who) + ": null eos list");
        if (winner_out) *winner_out = -1;
        if (pass_tokens_out) *pass_tokens_out = 0;
        // a ridden row must be in the numeric scheme and the head form of the step it replaces; the select kernel carries ids, scores and
        // final-norm rows, not lists, entropies, noise or penalty flags
        const bool usable = !smp_on && rep_penalty == 1.0f && !fp8_on && !mx4_on && !fp8_gemm_on && !persistent_on && topk == 0 && !ent_on &&
                            !(scores_on && allow_on) && !grp.pending;      // (one fork scaffold: a group pending on another env keeps it)
        DraftPlan pl;
        if (usable && max_new >= 1 && cap >= 1) pl = plan_drafts(e, n_drafts, ids, lens, max_new < cap ? max_new : cap, eos, n_eos);
        st_drafts[0] += 1;
        if (pl.G == 0) {                              // hints ignored: svln_generate, launch for launch
            st_drafts[5] += 1;
            generate(env, max_new, eos, n_eos, out, cap, n_out, false);
            st_drafts[7] += *n_out - 1;
            return;
        }
        const GenBegin gb = gen_begin(env, max_new, eos, n_eos, cap);      // (an armed svln_set_draft draft is consumed and not used)
        const int P = gb.P, L = gb.L, Tn = gb.Tn, limit = gb.limit, G = pl.G, r = pl.r, q0 = L / PAGE;
        ensure_bforced_buffers();
        ensure_cand_buffers();
        ensure_dsel_buffers();
        for (int g = 1; g < G; ++g) ensure_fork_tab(g);
        // ---- nothing was launched up to here
        int tail_n[MAXB] = {0}, k_max = 0, nh = 1, off = 0;
        const HeadLists &h = bf_host, &d = bf_dev;
        // (the pinned staging was last read by copies of calls that ended in a synchronisation)
        for (int q = 0; q < G * r; ++q) h_cfeed[q] = 0;
        h.src[0] = Tn - 1; h.tap[0] = -1;
        for (int g = 0; g < G; ++g) {
            const int kg = pl.k[g];
            if (g >= 1) tail_n[g] = fork_tail_pages(L, kg + 1);
            DecodeSlot& sl = h_cslots[g];
            sl.page_table = g == 0 ? e.d_pages : fork_tab[g]; sl.pos = L; sl.pad = kg;
            for (int j = 0; j < kg; ++j) { h_cfeed[g * r + j] = (int)ids[off + j]; h.src[nh] = Tn + g * r + j; h.tap[nh] = -1; ++nh; }
            h_dsel[g] = kg;
            k_max = std::max(k_max, kg); off += lens[g];
        }
        for (int g = G; g < 16; ++g) h_dsel[g] = 0;
        grp = Group();
        grp.env = env; grp.n_seq = G; grp.L = L; grp.q0 = q0;
        for (int g = 1; g < G; ++g) grp.n_tail = std::max(grp.n_tail, tail_n[g]);
        int n = 0, winner = 0;
        bool done = false;
        try {
            HIP_CHECK(hipMemcpyAsync(d.src, h.src, (size_t)nh * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d.tap, h.tap, (size_t)nh * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d_cfeed, h_cfeed, (size_t)G * r * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d_cslots, h_cslots, (size_t)G * sizeof(DecodeSlot), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d_dsel, h_dsel, 16 * sizeof(int), hipMemcpyHostToDevice, st));
            gen_ctl_start(env, L, limit, n_eos);
            HIP_CHECK(hipEventRecord(ph_ev[2], st));
            // the folded candidates call's pass: the tables of the fork first, rows of earlier turns in page q0 by one copy, the prompt's rows
            // of that page layer by layer through the mirror list
            ensure_pages(e, L + pl.k[0]);
            const int n_dst = fork_tables(e, q0, tail_n, G);
            const int n_mirror = L % PAGE != 0 ? n_dst : 0;
            if (n_mirror > 0) { if (P > q0 * PAGE) fork_page_copy(e.pages[q0], n_dst); else upload_fork_dst(n_dst); }
            const Fold f{d_cfeed, d_cslots, G, r, L + k_max, q0, d_fork_dst, n_mirror};
            std::vector<Seg> segs{Seg{&e, P, Tn, 0}};
            prefill_rows(segs, Tn + G * r, 0, 0, &f);
            e.kv_len = L;
            // head: the prompt's last row once, then the fed rows sequence by sequence; no tap scatter (the select kernel copies the winner's)
            launch_rmsnorm_indexed<T>(st, x, final_norm, bf_xn, d.src, d.tap, hid_tap, nh, H, c.rms_eps);
            for (int r0 = 0; r0 < nh; r0 += 32) {
                const int m = std::min(nh - r0, 32);
                argmax_rows(lm_head, H, bf_xn + (size_t)r0 * H, H, V, H, m == 1 ? 1 : ride_head_rows(m), false, r0);
            }
            DraftSelectArgs a;
            a.cand = d_tok_b; a.cand_score = scores_on ? d_score_b : nullptr; a.fed = d_cfeed; a.k = d_dsel; a.G = G; a.r = r;
            a.ctl = d_ctl; a.eos = d_eos; a.out_ids = d_out_ids; a.out_token = d_token; a.xn = bf_xn; a.hid_tap = hid_tap; a.H = H;
            a.tap_cap = HID_TAP_ROWS; a.scores = d_scores; a.rec = d_dsel + 8; a.stats = d_dsel + 12;
            launch_draft_select<T>(st, a);
            HIP_CHECK(hipEventRecord(ph_ev[3], st));
            // ONE synchronisation reads the loop state, the ids and the result record
            HIP_CHECK(hipMemcpyAsync(h_ctl, d_ctl, sizeof(GenCtl), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(h_out_ids, d_out_ids, (size_t)(k_max + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(h_dsel, d_dsel, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
            if (scores_on) HIP_CHECK(hipMemcpyAsync(h_scores, d_scores, (size_t)(k_max + 1) * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            LAUNCH_CHECK("generate_drafts");
            n = h_ctl->count; done = h_ctl->done != 0; winner = h_dsel[8];
            REQUIRE(n >= 1 && n <= k_max + 1 && n == h_dsel[9] && winner >= 0 && winner < G && n <= pl.k[winner] + 1, "generation state out of range");
            require_finite_tokens(h_out_ids, n);
        } catch (...) {
            // every fork page goes back to the pool, no group is pending; the env is as after a failed svln_generate
            (void)hipStreamSynchronize(st);
            drop_group();
            throw;
        }
        // the winner's private tail becomes the env's; the other forks' pages and the env's displaced tail go back to the pool
        promote_fork(e, winner, h_ctl->kv_len);
        if (!done) ensure_pages(e, L + n);            // the next step writes position L + n - 1
        st_drafts[1] += 1; st_drafts[2] += n; st_drafts[3] += nh - 1; st_drafts[4] += done ? 1 : 0; st_drafts[6] += winner >= 1 ? 1 : 0;
        if (winner_out) *winner_out = winner;
        if (pass_tokens_out) *pass_tokens_out = n;
        st_drafts[7] += finish_turn(e, env, L, limit, n, n, done, false, 0, n, true, out, n_out);
    }
    void turn_drafts(const svln_turn_args& a, int n_drafts, const int64_t* ids, const int32_t* lens, int64_t* out, int cap, int32_t* n_out,
                     int32_t* kv_len, int32_t* winner_out, int32_t* pass_tokens_out) override {
        Env& e = env_at(a.env);
        refuse_while_group_on(a.env, "svln_turn_drafts");
        begin_turn(a, [&] {
            REQUIRE(a.ids && a.n_ids >= 1, "svln_turn_drafts: null / empty argument");
            drafts_arg_check("svln_turn_drafts", n_drafts, ids, lens, out, n_out);
        });
        generate_drafts(a.env, n_drafts, ids, lens, a.max_new_tokens, a.eos_ids, a.n_eos, out, cap, n_out, winner_out, pass_tokens_out);
        if (kv_len) *kv_len = e.kv_len;
    }
    void drafts_stats(int64_t* out8) override { for (int q = 0; q < 8; ++q) out8[q] = st_drafts[q]; }
    // ------------------------------------------------------------------------------- forced turns (svln_generate_forced)
    // A turn on the CALLER's ids F[0 .. n): ids F[0 .. n - 1) ride the prefill pass as n - 1 more rows (the ride's gather, RoPE, KV append
    // and causal attention), the final norm of the last n rows goes to xn and the tap rows, ONE lm_head product in its EPI_TARGET form
    // keeps row i's logit of column F[i] beside the scored partials, and one final kernel writes the policy's arg-max, its log-probability
    // and F[i]'s.  No decode launch, one synchronisation.  The env and the loop state end where a plain turn that emitted F leaves them.
    static constexpr int FORCED_MAX = 32;
    int* d_ftgt = nullptr; int* h_ftgt = nullptr; float* d_fval = nullptr; float* d_flp = nullptr; float* h_flp = nullptr;
    void ensure_forced_buffers() {
        if (d_ftgt) return;
        d_ftgt = dalloc<int>(FORCED_MAX, true); d_fval = dalloc<float>(FORCED_MAX, true); d_flp = dalloc<float>(FORCED_MAX, true);
        HIP_CHECK(hipHostMalloc((void**)&h_ftgt, FORCED_MAX * sizeof(int)));
        HIP_CHECK(hipHostMalloc((void**)&h_flp, FORCED_MAX * sizeof(float)));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // targets of `rows` head rows -> d_ftgt (pad rows: -1)
    void upload_targets(const int32_t* tg, int n, int rows) {
        HIP_CHECK(hipStreamSynchronize(st));       // (h_ftgt of an earlier call is no longer being read)
        for (int k = 0; k < rows; ++k) h_ftgt[k] = k < n ? tg[k] : -1;
        HIP_CHECK(hipMemcpyAsync(d_ftgt, h_ftgt, rows * sizeof(int), hipMemcpyHostToDevice, st));
    }
    TargetArgs target_args(float inv_t) { TargetArgs t; t.tgt = d_ftgt; t.tgt_val = d_fval; t.inv_t = inv_t; return t; }
    // the EPI_TARGET lm_head over `rows` rows of xrows (the first n of them live) and its final kernel: greedy ids -> d_tok_b, their
    // log-probabilities -> d_score_b, the targets' -> d_flp.  The routing is argmax_rows' own: MFMA tiles from batched_mfma_min rows.
    // `to` (a head chunk of the scheduler's forced jobs): the chunk's own targets, capture slots and outputs in place of those five buffers
    struct TargetOut { const int* tgt; float* val; int* tok; float* score; float* lp; };
    void target_rows(const void* W, int ldw, const T* xrows, int ldx, int N, int K, int rows, int n, float inv_t, const TargetOut* to = nullptr) {
        const TargetOut o = to ? *to : TargetOut{d_ftgt, d_fval, d_tok_b, d_score_b, d_flp};
        TargetArgs tg; tg.tgt = o.tgt; tg.tgt_val = o.val; tg.inv_t = inv_t;
        const HeadParts p = parts_b();
        int np;
        if (mfma_head_fits(rows, N, K)) {        // (the callers take the subset product themselves: target_subset_rows)
            GemmArgs a = gemm_args(xrows, ldx, W, ldw, nullptr, 0, nullptr, nullptr, 0, 0, rows, N, K, EPI_ARGMAX);
            aim(a, p, head_form(EPI_TARGET)); a.tg = tg;
            np = launch_gemm_argmax<T>(st, a);
        } else {
            GemvBatchArgs hb = gemvb_args(W, ldw, xrows, ldx, nullptr, nullptr, nullptr, 0, nullptr, 0, N, K, EPI_ARGMAX, rows);
            aim(hb, p, head_form(EPI_TARGET)); hb.tg = tg;
            launch_gemv_batched<T>(st, hb);
            np = gemv_batched_grid(N, EPI_ARGMAX, rows);
        }
        // (its own final kernel, with the targets' outputs: not merge_head's)
        launch_target_final_batched(st, p.val, p.idx, p.sum, np, n, o.tgt, o.val, o.tok, o.score, o.lp);
    }
    // the same head under an allowed list: the subset product in its forced form on n rows, row i's normalised row -> alp[i] (the score of
    // a forced id is that row's entry at the id's list position), the greedy ids and their scores through the scored final kernel
    void target_subset_rows(const T* xrows, int n, float inv_t, float* alp, int* tok, float* score) {
        const HeadForm f = head_form(EPI_TARGET);
        GemvSubsetArgs su = subset_args(xrows, H, n, parts_b(), f);
        su.tg_inv_t = inv_t;
        launch_gemv_subset<T>(st, su);
        launch_subset_logprobs(st, part_val_b, allow_n, n, alp);
        HeadOut o = out_rows(0, 0); o.tok = tok; o.score = score;
        merge_head(parts_b(), allow_n, 1, n, f, o);
    }
    // every refusal of a forced turn that needs no state of the env (svln_turn_forced checks them before it encodes a frame).  sched: the
    // forced submit of the scheduler (svln_batch_submit_forced), whose mode rules are its own (modes.h: C_BATCH_SUBMIT_FORCED)
    void forced_refusals(int env, const int64_t* ids, int n, const int64_t* eos, int n_eos, const char* who_c = "svln_generate_forced", bool sched = false) {
        const std::string who(who_c);
        env_at(env);
        REQUIRE(ids, who + ": null id list");
        REQUIRE(n >= 1 && n <= FORCED_MAX, who + ": n must be 1 .. 32");
        REQUIRE(n_eos >= 0 && n_eos <= (V > 16 ? V : 16) && (n_eos == 0 || eos), who + ": bad eos list");
        for (int k = 0; k < n; ++k) {
            REQUIRE(ids[k] >= 0 && ids[k] < V, who + ": id " + std::to_string((long long)ids[k]) + " is outside the vocabulary");
            if (k + 1 < n)
                for (int q = 0; q < n_eos; ++q)
                    REQUIRE(eos[q] != ids[k], who + ": an id of the EOS set may only be the last one (an EOS is appended, never fed)");
        }
        refuse(sched ? C_BATCH_SUBMIT_FORCED : C_GENERATE_FORCED, who_c);
        if (allow_on)
            for (int k = 0; k < n; ++k)
                REQUIRE(std::binary_search(allow_ids.begin(), allow_ids.end(), (int)ids[k]),
                        who + ": id " + std::to_string((long long)ids[k]) + " is not in the allowed list (svln_set_allowed_tokens)");
        // (a head chunk of the scheduler holds up to 32 rows of several jobs, whatever n is)
        REQUIRE(allow_on || ride_head_rows(sched ? FORCED_MAX : n) >= (sched ? FORCED_MAX : n), who + ": this vocabulary / hidden size has no lm_head form for more than 8 rows");
    }
    void generate_forced(int env, const int64_t* ids, int n, const int64_t* eos, int n_eos, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs,
                         int32_t* kv_len) override {
        Env& e = env_at(env);
        refuse_while_group_on(env, "svln_generate_forced");
        disarm_draft(env);              // consumed by this call, as svln_generate consumes it
        REQUIRE(logprobs && greedy_ids && greedy_logprobs, "svln_generate_forced: null output pointer");
        forced_refusals(env, ids, n, eos, n_eos);
        const TurnPlan pl = plan_turn(e, "svln_generate_forced", n, n, "n");
        const int P = pl.P, L = pl.L, Tn = pl.Tn;
        // ---- nothing was launched or changed up to here (but the armed draft)
        invalidate_last_results();
        set_speculative_buffers();      // d_draft / h_draft: the fed ids
        ensure_forced_buffers();
        ensure_pages(e, L + n - 1);
        const int k = n - 1;            // fed rows: the last id is never fed
        const int M = Tn + k;
        const int rows = allow_on ? n : ride_head_rows(n);
        const float inv_t = smp_on ? smp_inv_t : 1.0f;
        // (the pinned staging was last read by copies of calls that ended in a synchronisation)
        for (int i = 0; i < n; ++i) h_draft[i] = (int)ids[i];
        for (int i = 0; i < rows; ++i) h_ftgt[i] = i < n ? (int)ids[i] : -1;
        HIP_CHECK(hipMemcpyAsync(d_draft, h_draft, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_ftgt, h_ftgt, (size_t)rows * sizeof(int), hipMemcpyHostToDevice, st));
        // the loop state a plain turn that emitted F leaves: n ids listed, the last one appended and not fed
        HIP_CHECK(hipMemcpyAsync(d_out_ids, h_draft, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        h_ctl->pos = L - 1 + k; h_ctl->kv_len = L + k; h_ctl->done = 1; h_ctl->count = n; h_ctl->max_new = n; h_ctl->n_eos = n_eos;
        h_ctl->draw0 = smp_on ? env_draws[env] : 0; h_ctl->stream = smp_on ? env : 0;
        HIP_CHECK(hipMemcpyAsync(d_ctl, h_ctl, sizeof(GenCtl), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipEventRecord(ph_ev[2], st));
        prefill(e, P, M, k);
        e.kv_len = L;
        launch_rmsnorm<T>(st, x + (size_t)(M - n) * H, final_norm, xn, n, H, c.rms_eps);
        HIP_CHECK(hipMemcpyAsync(hid_tap, xn, (size_t)n * H * sizeof(T), hipMemcpyDeviceToDevice, st));
        if (allow_on) {
            // the subset product as on every other path: one partial per listed id on y; row i's normalised row -> d_alp_b[i], and the
            // score of F[i] is that row's entry at the id's list position (the same bits svln_get_allowed_logprobs returns)
            target_subset_rows(xn, n, inv_t, d_alp_b, d_tok_b, d_score_b);
        } else {
            target_rows(lm_head, H, xn, H, V, H, rows, n, inv_t);
        }
        HIP_CHECK(hipEventRecord(ph_ev[3], st));
        HIP_CHECK(hipMemcpyAsync(h_tok_b, d_tok_b, n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_score_b, d_score_b, n * sizeof(float), hipMemcpyDeviceToHost, st));
        if (allow_on) HIP_CHECK(hipMemcpyAsync(h_alp_b, d_alp_b, (size_t)n * allow_n * sizeof(float), hipMemcpyDeviceToHost, st));
        else HIP_CHECK(hipMemcpyAsync(h_flp, d_flp, n * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        LAUNCH_CHECK("generate_forced");
        require_finite_tokens(h_tok_b, n);
        for (int i = 0; i < n; ++i) {
            greedy_ids[i] = h_tok_b[i]; greedy_logprobs[i] = h_score_b[i];
            logprobs[i] = forced_score(i, (int)ids[i], h_flp, h_alp_b);
        }
        last_scores.assign(logprobs, logprobs + n); last_scores_valid = true;
        if (allow_on) { last_alp.assign(h_alp_b, h_alp_b + (size_t)n * allow_n); last_alp_n = allow_n; last_alp_valid = true; }
        e.kv_len = L + n - 1;
        add_phase(1, 2, 3);
        settle_vision();
        n_generated = n;
        top2_stale = true;              // no top-2 logits were kept, as after a ride
        top2_sampled = false;
        if (kv_len) *kv_len = e.kv_len;
    }
    void turn_forced(const svln_turn_args& a, const int64_t* ids, int n, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs,
                     int32_t* kv_len) override {
        env_at(a.env);
        refuse_while_group_on(a.env, "svln_turn_forced");
        begin_turn(a, [&] {
            REQUIRE(a.ids && a.n_ids >= 1 && logprobs && greedy_ids && greedy_logprobs, "svln_turn_forced: null / empty argument");
            forced_refusals(a.env, ids, n, a.eos_ids, a.n_eos);
        });
        generate_forced(a.env, ids, n, a.eos_ids, a.n_eos, logprobs, greedy_ids, greedy_logprobs, kv_len);
    }
    // TEST-ONLY: one EPI_TARGET product and its final kernel on caller-given device operands, whatever the engine's switches say
    // host_slots (optional, [32]): in, what the capture slots hold before the launch; out, what they hold after it
    void slots_in(const float* host_slots) {
        if (host_slots) HIP_CHECK(hipMemcpy(d_fval, host_slots, FORCED_MAX * sizeof(float), hipMemcpyHostToDevice));
    }
    void target_out(int n, int32_t* host_tokens, float* host_greedy, float* host_logprobs, float* host_slots, const char* who) {
        if (host_slots) HIP_CHECK(hipMemcpyAsync(host_slots, d_fval, FORCED_MAX * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_tok_b, d_tok_b, n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_score_b, d_score_b, n * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_flp, d_flp, n * sizeof(float), hipMemcpyDeviceToHost, st));
        sync();
        LAUNCH_CHECK(who);
        for (int b = 0; b < n; ++b) { host_tokens[b] = h_tok_b[b]; host_greedy[b] = h_score_b[b]; host_logprobs[b] = h_flp[b]; }
    }
    void target_op_refusals(const int32_t* targets, int rows, int N, float inv_t, const void* o0, const void* o1, const void* o2) {
        REQUIRE(targets && o0 && o1 && o2, "null pointer");
        REQUIRE(std::isfinite(inv_t) && inv_t > 0.0f, "inv_t must be finite and > 0");
        for (int k = 0; k < rows; ++k) REQUIRE(targets[k] >= -1 && targets[k] < N, "targets: -1 (none) or a column of [0, N)");
    }
    void op_gemv_batched_target(GemvBatchArgs a, const int32_t* targets, float inv_t, int32_t* host_tokens, float* host_greedy,
                                float* host_logprobs, float* host_slots) override {
        REQUIRE(a.W && a.x, "null pointer");
        REQUIRE(a.B == 2 || a.B == 4 || a.B == 8, "B must be 2, 4 or 8");
        REQUIRE(a.N >= 1 && a.K >= Elt<T>::PER_CHUNK && a.K % Elt<T>::PER_CHUNK == 0, "N >= 1, K a positive multiple of the 16-byte chunk");
        REQUIRE(a.ldw >= a.K && a.ldw % Elt<T>::PER_CHUNK == 0 && a.ldx >= a.K && a.ldx % Elt<T>::PER_CHUNK == 0, "ldw, ldx >= K, multiples of the 16-byte chunk");
        target_op_refusals(targets, a.B, a.N, inv_t, host_tokens, host_greedy, host_logprobs);
        ensure_forced_buffers();
        upload_targets(targets, a.B, a.B);
        slots_in(host_slots);
        a.norm_w = nullptr; a.pen_flags = nullptr; a.tg = target_args(inv_t);
        aim(a, parts_b(), head_form(EPI_TARGET));
        launch_gemv_batched<T>(st, a);
        launch_target_final_batched(st, part_val_b, part_idx_b, part_sum_b, gemv_batched_grid(a.N, EPI_ARGMAX, a.B), a.B, d_ftgt, d_fval, d_tok_b, d_score_b, d_flp);
        target_out(a.B, host_tokens, host_greedy, host_logprobs, host_slots, "op_gemv_batched_target");
    }
    void op_gemm_target(GemmArgs a, const int32_t* targets, float inv_t, int32_t* host_tokens, float* host_greedy, float* host_logprobs,
                        float* host_slots) override {
        constexpr int chunk = Elt<T>::PER_CHUNK;
        REQUIRE(a.A && a.W, "null pointer");
        REQUIRE(a.M >= 1 && a.M <= 32 && a.N >= 1 && (a.N + 127) / 128 <= 2048, "1 <= M <= 32 rows, 1 <= N <= 262144");
        REQUIRE(a.K >= chunk && a.K % chunk == 0 && a.lda >= a.K && a.ldw >= a.K && a.lda % chunk == 0 && a.ldw % chunk == 0,
                "K a positive multiple of the 16-byte chunk; lda, ldw >= K, multiples of it (aligned LDS-DMA)");
        REQUIRE(((size_t)a.A & 15) == 0 && ((size_t)a.W & 15) == 0, "A and W must be 16-byte aligned (LDS-DMA)");
        target_op_refusals(targets, a.M, a.N, inv_t, host_tokens, host_greedy, host_logprobs);
        ensure_forced_buffers();
        upload_targets(targets, a.M, a.M);
        slots_in(host_slots);
        a.zeros = zero_line; a.pen_flags = nullptr; a.tg = target_args(inv_t);
        aim(a, parts_b(), head_form(EPI_TARGET));
        const int np = launch_gemm_argmax<T>(st, a);
        launch_target_final_batched(st, part_val_b, part_idx_b, part_sum_b, np, a.M, d_ftgt, d_fval, d_tok_b, d_score_b, d_flp);
        target_out(a.M, host_tokens, host_greedy, host_logprobs, host_slots, "op_gemm_target");
    }
    // TEST-ONLY: the batched arg-max partials [rows][n] the last lm_head product of a test op left (part_val, part_idx, part_sum)
    void op_read_argmax_partials(int rows, int n, float* val, int32_t* idx, float* sum) override {
        REQUIRE(val && idx && sum, "null pointer");
        REQUIRE(rows >= 1 && rows <= HEAD_ROWS && n >= 1 && n <= 2048, "1 <= rows <= 64, 1 <= n <= 2048");
        sync();
        const size_t m = (size_t)rows * n;
        HIP_CHECK(hipMemcpy(val, part_val_b, m * sizeof(float), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(idx, part_idx_b, m * sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(sum, part_sum_b, m * sizeof(float), hipMemcpyDeviceToHost));
    }
    void group_select(int env, int index, int32_t* kv_len) override {
        env_at(env);
        REQUIRE(grp.pending && grp.env == env, "svln_group_select: no group turn is pending on this env");
        REQUIRE(index >= 0 && index < grp.n_seq, "svln_group_select: index outside the group's sequences");
        promote_fork(envs[env], index, grp.L + grp.n_out[index] - 1);
        if (kv_len) *kv_len = envs[env].kv_len;
    }
    // The page handover of a fork turn: the env goes on with sequence `index` of the group at kv length kv_final.  The group is dropped:
    // every other fork page and the env's displaced tail go back to the pool exactly once, no group is left pending.
    void promote_fork(Env& e, int index, int kv_final) {
        if (index >= 1 && !grp.tail[index].empty()) {
            // the env goes on with sequence `index`: its private tail becomes the env's, the env's former tail is freed with the other forks'
            // (a group turn's tails all have n_tail pages, as has the env; the candidates of svln_generate_candidates are ragged: a page the
            // env does not hold yet is handed over)
            std::vector<int>& tl = grp.tail[index];
            const int nt = (int)tl.size();
            std::vector<int> back;
            for (int i = 0; i < nt; ++i) {
                if (grp.q0 + i < e.n_pages) { back.push_back(e.pages[grp.q0 + i]); e.pages[grp.q0 + i] = tl[i]; }
                else e.pages[e.n_pages++] = tl[i];
            }
            tl = back;
            HIP_CHECK(hipMemcpyAsync(e.d_pages + grp.q0, e.pages.data() + grp.q0, (size_t)nt * sizeof(int), hipMemcpyHostToDevice, st));
        }
        drop_group();
        e.kv_len = kv_final;
    }
    void group_logprobs(int index, float* out, int cap, int32_t* n) override {
        REQUIRE(grp.pending && index >= 0 && index < grp.n_seq, "svln_group_logprobs: no pending group turn / no such sequence");
        REQUIRE(grp.scored, "svln_group_logprobs: token log-probabilities were off for this turn (svln_set_token_scores)");
        const int m = (int)grp.scores[index].size();
        for (int k = 0; k < m && k < cap; ++k) out[k] = grp.scores[index][k];
        *n = m;
    }
    void group_dist(int index, float* out, int cap_rows, int32_t* n_rows, int32_t* n_cols) override {
        REQUIRE(grp.pending && index >= 0 && index < grp.n_seq, "svln_group_dist: no pending group turn / no such sequence");
        REQUIRE(grp.alp_n > 0, "svln_group_dist: token log-probabilities (svln_set_token_scores) or the allowed list (svln_set_allowed_tokens) were off for this turn");
        const size_t m = grp.alp[index].size(), lim = (size_t)cap_rows * grp.alp_n;
        for (size_t k = 0; k < m && k < lim; ++k) out[k] = grp.alp[index][k];
        *n_rows = (int32_t)(m / (size_t)grp.alp_n); *n_cols = grp.alp_n;
    }
    void get_hidden_group(int index, float* out, int max_rows, int32_t* n_rows) override {
        REQUIRE(grp.pending && index >= 0 && index < grp.n_seq, "svln_get_hidden_group: no pending group turn / no such sequence");
        int n = grp.n_out[index] < 8 ? grp.n_out[index] : 8;
        if (n > max_rows) n = max_rows;
        for (int t = 0; t < n; ++t) read_rows_f32(hid_tap + (size_t)(t * MAXB + index) * H, (size_t)H, out + (size_t)t * H);
        *n_rows = n;
    }

    // ------------------------------------------------------------------------------- taps
    // Parity taps of the single-env prefill (test infrastructure, off by default): the LAST row of the residual stream after every
    // decoder layer (error-versus-depth curves), and every row entering / leaving ONE probed layer (a fused layer checked against
    // the oracle at its own scale, on the engine's own inputs: a whole-stack tolerance would hide an O(1)-wrong stage).
    // probe buffers of the probed layer: 0 = x entering the layer, 1 = x leaving it, 2 = attention output (the A operand of o_proj),
    // 3 = x after the attention residual, 4 = post_attention_layernorm(x) (A of gate/up), 5 = silu(gate) * up (A of down_proj)
    // 6 = input_layernorm(x) (A of the q/k/v product), 7 = the q | k | v buffer after bias and RoPE (q columns rotated; k / v columns: the plain product, the rotated k is in the pages)
    static constexpr int N_PROBE = 8;
    bool layer_taps_on = false; int probe_layer = -1; int probe_rows = 0;
    T* layer_tap = nullptr; T* probe_buf[N_PROBE] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int probe_cols(int which) const { return which == 2 ? nq * 128 : which == 5 ? I : which == 7 ? qkv_dim : H; }
    void set_layer_taps(int enable, int layer) override {
        REQUIRE(layer < c.layers, "probe layer out of range");
        HIP_CHECK(hipStreamSynchronize(st));
        layer_taps_on = enable != 0;
        probe_layer = layer_taps_on ? layer : -1;
        probe_rows = 0;
        if (layer_taps_on && !layer_tap) layer_tap = dalloc<T>((size_t)c.layers * H, true);
        if (probe_layer >= 0 && !probe_buf[0])
            for (int k = 0; k < N_PROBE; ++k) probe_buf[k] = dalloc<T>((size_t)c.max_positions * probe_cols(k));
    }
    void probe_copy(int which, const T* src, int M) {
        HIP_CHECK(hipMemcpyAsync(probe_buf[which], src, (size_t)M * probe_cols(which) * sizeof(T), hipMemcpyDeviceToDevice, st));
    }
    void get_layer_taps(float* out) override {
        REQUIRE(layer_tap != nullptr, "layer taps were never enabled");
        read_rows_f32(layer_tap, (size_t)c.layers * H, out);
    }
    void get_layer_probe(int which, float* out, int64_t max_elems, int32_t* n_rows, int32_t* n_cols) override {
        REQUIRE(probe_buf[0] != nullptr && which >= 0 && which < N_PROBE, "no such layer probe");
        const int cols = probe_cols(which);
        REQUIRE((int64_t)probe_rows * cols <= max_elems, "layer probe: output buffer too small");
        if (probe_rows > 0) read_rows_f32(probe_buf[which], (size_t)probe_rows * cols, out);
        *n_rows = probe_rows; *n_cols = cols;
    }
    void read_rows_f32(const T* src, size_t n, float* out) {
        float* tmp = nullptr;
        HIP_CHECK(hipMalloc((void**)&tmp, n * sizeof(float)));
        launch_to_f32<T>(st, src, tmp, (int64_t)n);
        HIP_CHECK(hipMemcpyAsync(out, tmp, n * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipFree(tmp));
    }
    void get_hidden(float* out, int max_rows, int32_t* n_rows) override {
        int n = n_generated < HID_TAP_ROWS ? n_generated : HID_TAP_ROWS;
        if (n > max_rows) n = max_rows;
        read_rows_f32(hid_tap, (size_t)n * H, out);
        *n_rows = n;
    }
    void get_embeds(int env, int start, int n, float* out) override {
        Env& e = env_at(env);
        REQUIRE(start >= 0 && n >= 0 && start + n <= e.n_embeds, "embeds range");
        read_rows_f32(e.embeds + (size_t)start * H, (size_t)n * H, out);
    }
    void get_feats(int start, int n, float* out) override {
        REQUIRE(start >= 0 && n >= 0 && start + n <= n_feat_frames * otok, "feats range");
        read_rows_f32(feats + (size_t)start * H, (size_t)n * H, out);
    }
    void get_top2(float* out) override {
        REQUIRE(!top2_sampled, "svln_get_top2: the last turn was sampled (svln_set_sampling): the top-2 values of its last arg-max are perturbed by the noise, not logits");
        REQUIRE(!top2_stale, "svln_get_top2: the last token of the last turn came from a verify pass (svln_set_speculative) or a ride "
                             "(svln_set_prefill_draft), which keep no top-2 logits");
        out[0] = h_top2[0]; out[1] = h_top2[1];
    }
    void sync() override { HIP_CHECK(hipStreamSynchronize(st)); }
    void set_graph(int enable) override { use_graph = enable != 0; if (!use_graph) drop_graphs(); }
    void ensure_prune_scratch() {
        if (prune_partial) return;
        const int nmax = c.max_frames * otok;
        prune_partial = dalloc<float>((size_t)((nmax + 63) / 64) * H);
        prune_mean = dalloc<float>(H);
        prune_score = dalloc<float>(nmax);
        d_sel = dalloc<int>(nmax);
        HIP_CHECK(hipHostMalloc((void**)&h_sel, nmax * sizeof(int)));
    }
    void set_memory_prune(int keep) override {
        REQUIRE(keep >= 0, "keep must be >= 0 (0 = the reference behaviour: all num_history x 196 memory tokens)");
        if (keep > 0) ensure_prune_scratch();
        prune_keep = keep;
    }
    // indices (ascending) of the `keep` rows of m [n_rows][H] (engine dtype, device) that survive; h_sel holds them on return
    void run_memory_prune(const T* m, int n_rows, int keep) {
        ensure_prune_scratch();
        REQUIRE(n_rows >= 1 && n_rows <= c.max_frames * otok && keep >= 1 && keep <= n_rows, "memory prune: bad sizes");
        launch_memory_prune<T>(st, m, n_rows, H, keep, prune_partial, prune_mean, prune_score, d_sel);
        HIP_CHECK(hipMemcpyAsync(h_sel, d_sel, keep * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    void op_memory_prune(const void* m, int n_rows, int keep, int32_t* out_idx, float* out_score) override {
        run_memory_prune((const T*)m, n_rows, keep);
        for (int j = 0; j < keep; ++j) out_idx[j] = h_sel[j];
        if (out_score) HIP_CHECK(hipMemcpy(out_score, prune_score, n_rows * sizeof(float), hipMemcpyDeviceToHost));
    }
    // Opt-in (no reference counterpart): the single-env decode step and the lm_head read e4m3 copies of the LLM
    // weights (per-row scale) instead of the bf16 ones; prefill, vision and the lockstep multi-env path keep bf16.  Both copies stay
    // resident (15.2 + 7.6 GB of 288).  Allocated and quantised at the first enable; a later svln_set_tensor / svln_synth_tensor quantises the
    // written matrix again (after_weight_write), so the copies are always those of the weights loaded now.
    void build_fp8_weights() {
        REQUIRE(sizeof(T) == 2, "fp8 weights need the bf16 engine");
        REQUIRE(weights_missing() == 0, g_err);
        REQUIRE(H % 16 == 0 && I % 16 == 0, "fp8 weights need hidden and intermediate sizes that are multiples of 16");
        if (fp8_built) return;
        for (const QMat& m : qmats) {
            m.q8->q = dalloc<uint8_t>((size_t)m.rows * m.cols);
            m.q8->s = dalloc<float>((size_t)m.rows);
            launch_quant_fp8_rows(st, m.w, m.cols, m.q8->q, m.q8->s, m.rows, m.cols);
        }
        HIP_CHECK(hipStreamSynchronize(st));
        fp8_built = true;
    }
    void set_fp8_decode(int enable) override {
        if ((enable != 0) == fp8_on) return;       // nothing changes
        refuse(enable ? C_SET_FP8_DECODE_ON : C_SET_FP8_DECODE_OFF);
        if (!enable) { drop_graphs(); fp8_on = false; return; }
        build_fp8_weights();
        drop_graphs();
        fp8_on = true;
    }
    // Opt-in (no reference counterpart): the single-env decode step's four projections and every lm_head product read
    // OCP MXFP4 copies of the LLM weights (E2M1 elements, one E8M0 scale per 32 elements of a row: 4.25 bits per weight) instead of the
    // bf16 ones; prefill, vision, attention and norms keep bf16, and so does the lockstep multi-env path unless svln_set_mxfp4_batched is on.
    // Both copies stay resident (15.2 + 4.0 GB).
    // Allocated and quantised at the first enable, and kept in step with later weight writes as the e4m3 copies are (after_weight_write).
    void build_mxfp4_weights() {
        REQUIRE(sizeof(T) == 2, "MXFP4 weights need the bf16 engine");
        REQUIRE(weights_missing() == 0, g_err);
        REQUIRE(H % 32 == 0 && I % 32 == 0 && (nq * 128) % 32 == 0, "MXFP4 weights need hidden, intermediate and q sizes that are multiples of 32");
        if (mx4_built) return;
        for (const QMat& m : qmats) {
            m.q4->q = dalloc<uint8_t>((size_t)m.rows * (m.cols / 2));
            m.q4->e8 = dalloc<uint8_t>((size_t)m.rows * (m.cols / 32));
            launch_quant_mxfp4_rows(st, m.w, m.cols, m.q4->q, m.q4->e8, m.rows, m.cols);
        }
        HIP_CHECK(hipStreamSynchronize(st));
        LAUNCH_CHECK("build_mxfp4_weights");
        mx4_built = true;
    }
    void set_mxfp4_decode(int enable) override {
        if ((enable != 0) == mx4_on) return;       // nothing changes
        refuse(enable ? C_SET_MXFP4_DECODE_ON : C_SET_MXFP4_DECODE_OFF);
        if (!enable) { drop_graphs(); mx4_on = false; return; }
        build_mxfp4_weights();
        drop_graphs();
        mx4_on = true;
    }
    // Lossless (no reference counterpart; same ids and hidden rows bit for bit): the single-env decode step's gate/up and down_proj GEMVs and
    // head()'s lm_head GEMV stream the 12-bit packing of their bf16 weights (gemv.hip, WP12) -- about 0.75 x the bytes.  The copies are
    // allocated at creation and encoded whenever a matrix is written.  On by default on the bf16 engine; the e4m3 / MXFP4 decode modes take
    // precedence, and the persistent layer, the batched and verify passes, the subset head and every GEMM keep the bf16 weights.
    void set_packed_decode(int enable) override {
        const bool want = enable != 0;
        REQUIRE(!want || sizeof(T) == 2, "svln_set_packed_decode: the packed weights are a bf16 format; the fp32 engine has none");
        REQUIRE(!want || lm_head12.pk, "svln_set_packed_decode: hidden or intermediate size above 32768: no packed copies exist");
        if (want == p12_on) return;
        drop_graphs();
        p12_on = want;
    }
    void packed_stats(int64_t* packed_bytes, int64_t* bf16_bytes, int64_t* blocks, int64_t* fallback_blocks) override {
        HIP_CHECK(hipStreamSynchronize(st));
        int64_t pb = 0, bb = 0, nb = 0, fb = 0;
        for (auto& kv : p12_of) {
            const P12& m = *kv.second;
            unsigned f = 0;
            HIP_CHECK(hipMemcpy(&f, m.fb, sizeof(unsigned), hipMemcpyDeviceToHost));
            pb += m.rows * (int64_t)(p12_row_bytes(m.cols) + 16); bb += m.rows * (int64_t)m.cols * 2; nb += m.rows * (int64_t)((m.cols + 511) / 512); fb += f;
        }
        *packed_bytes = pb; *bf16_bytes = bb; *blocks = nb; *fallback_blocks = fb;
    }
    // Opt-in (no reference counterpart): the batched decode step of svln_generate_batch / svln_batch_step (q|k|v, o_proj, gate/up and
    // down_proj at every B) and every lm_head product of the scheduler read the MXFP4 copies above through gemv_mx4b_kernel (weight-only:
    // bf16 activations on the MFMA path); prefill rows keep the bf16 products, and an iteration that holds decode rows and prefill rows is
    // split so that no decode row rides through them (batch_step_run).  Independent of svln_set_mxfp4_decode (the single-env step).
    void set_mxfp4_batched(int enable) override {
        if ((enable != 0) == mx4b_on) return;      // nothing changes
        // an env must not change scheme in the middle of a turn, in either direction
        refuse(enable ? C_SET_MXFP4_BATCHED_ON : C_SET_MXFP4_BATCHED_OFF, nullptr, false, 0);
        if (!enable) { drop_graphs(); mx4b_on = false; return; }
        REQUIRE(sizeof(T) == 2, "svln_set_mxfp4_batched: MXFP4 weights need the bf16 engine");
        refuse(C_SET_MXFP4_BATCHED_ON, nullptr, false, 1);
        build_mxfp4_weights();
        drop_graphs();
        mx4b_on = true;
    }
    // Opt-in (no reference counterpart): the LLM's dense products with more than one row -- prefill (svln_generate,
    // the scheduler) and the decode steps of >= 4 lockstep envs -- run as e4m3 x e4m3 MFMA products (v_mfma_f32_32x32x16_fp8_fp8, fp32
    // accumulate, bf16 out): per-row weight scales (the copies of svln_set_fp8_decode), per-row activation scales computed on the fly.
    // Half the operand bytes per k through HBM / L2 / LDS.  Vision, attention, norms and the lm_head stay bf16.
    void set_fp8_gemm(int enable) override {
        if ((enable != 0) == fp8_gemm_on) return;  // nothing changes
        refuse(enable ? C_SET_FP8_GEMM_ON : C_SET_FP8_GEMM_OFF);
        if (!enable) { fp8_gemm_on = false; return; }
        build_fp8_weights();
        if (!act8) {
            const size_t widest = (size_t)(I > nq * 128 ? I : nq * 128);
            act8 = dalloc<uint8_t>((size_t)c.max_positions * (widest > (size_t)H ? widest : (size_t)H));
            act8_scale = dalloc<float>((size_t)c.max_positions);
        }
        fp8_gemm_on = true;
    }
    // Opt-in: the instruction form of those products.  On: v_mfma_scale_f32_32x32x64_f8f6f4 (v_mfma_scale_f32_16x16x128_f8f6f4 on the 8-phase
    // 256x256 tile) with neutral block scales -- the same e4m3 bytes, per-row scales and fp32 accumulation at twice the MFMA rate -- and
    // the large-tile products may take the 8-phase schedule as bf16 ones do.  No effect while svln_set_fp8_gemm is off.
    void set_fp8_scaled_mfma(int enable) override {
        if ((enable != 0) == fp8_scaled_on) return;
        REQUIRE(sizeof(T) == 2, "svln_set_fp8_scaled_mfma: the e4m3 products need the bf16 engine");
        refuse(C_SET_FP8_SCALED_MFMA);
        fp8_scaled_on = enable != 0;
    }
    // C = A . W^T (+ epilogue) for an LLM linear: bf16 operands, or -- with svln_set_fp8_gemm -- the rows of A quantised on the fly
    // against the e4m3 copy of W
    // act8_src: the rows whose e4m3 copy act8 currently holds because the reduce that produced them also quantised them (the normalised
    // rows handed from o_proj to gate/up and from down_proj to the next layer's qkv: two of the four quantise launches of a layer)
    const void* act8_src = nullptr; int act8_rows = 0;
    bool llm_gemm(GemmArgs a, const Q8& q) {
        if (fp8_gemm_on && q.q) {
            if (!(act8_src == a.A && act8_rows == a.M && a.lda == a.K)) launch_quant_fp8_rows(st, a.A, a.lda, act8, act8_scale, a.M, a.K);
            act8_src = nullptr;
            if (a.norm_out && a.norm_w && !a.norm_b && (size_t)a.N <= (size_t)H) { a.norm_q8 = act8; a.norm_q8_scale = act8_scale; }
            const void* nout = a.norm_out; const int rows = a.M;
            a.A = act8; a.lda = a.K; a.W = q.q; a.ldw = a.K; a.a_scale = act8_scale; a.w_scale = q.s;
            if (fp8_scaled_on) a.force_cfg |= GEMM_FORCE_FP8_SCALED;
            const bool fused = launch_gemm<T>(st, a);
            if (fused && a.norm_q8) { act8_src = nout; act8_rows = rows; }      // the reduce ran after the product had consumed act8
            return fused;
        }
        act8_src = nullptr;
        return launch_gemm<T>(st, a);
    }
    bool op_gemm_fp8(const GemmArgs& a0) override {
        REQUIRE(sizeof(T) == 2, "fp8 products need the bf16 engine");
        GemmArgs a = a0; a.ws = gemm_ws; a.ws_elems = gemm_ws_elems; a.zeros = zero_line;
        REQUIRE(a.a_scale && a.w_scale, "missing scales");
        REQUIRE(a.epi == EPI_NONE || a.epi == EPI_SWIGLU, "fp8 products: plain or SwiGLU epilogue");
        gemm_refusals(a, 16);
        const bool fused = launch_gemm<T>(st, a);
        sync();
        LAUNCH_CHECK("op_gemm_fp8");
        return fused;
    }
    void probe_reset() override {
        if (probe_ev.empty()) { probe_ev.resize(4096); for (auto& ev : probe_ev) HIP_CHECK(hipEventCreate(&ev)); }
        if (pprobe_ev.empty()) { pprobe_ev.resize(512); for (auto& ev : pprobe_ev) HIP_CHECK(hipEventCreate(&ev)); }
        probe_used = 0; probe_on = true; pprobe_used = 0; pprobe_rows = 0;
        probe_bytes = (double)2 * I * H * sizeof(T);
        if (mx4_on) probe_bytes = (double)2 * I * (H / 2) + (double)2 * I * (H / 32);                // E2M1 code pairs + E8M0 scale bytes
        else if (!fp8_on && p12_on && ll[0].gu12.pk) {      // what the probed launch streams: packed blocks + records + the fallback blocks' bf16 bytes
            unsigned f = 0;
            HIP_CHECK(hipStreamSynchronize(st));
            HIP_CHECK(hipMemcpy(&f, ll[0].gu12.fb, sizeof(unsigned), hipMemcpyDeviceToHost));
            probe_bytes = (double)2 * I * (double)(p12_row_bytes(H) + 16) + (double)f * 1024.0;
        }
        // persistent layer: the four products one launch streams (o, gate/up, down, the next layer's q|k|v)
        if (persistent_active()) probe_bytes = ((double)H * nq * 128 + (double)2 * I * H + (double)H * I + (double)qkv_dim * H) * sizeof(T);
    }
    void probe_read(double* ms, int64_t* launches, double* bytes) override {
        HIP_CHECK(hipStreamSynchronize(st));
        double tot = 0;
        for (size_t k = 0; k + 1 < probe_used; k += 2) { float t = 0; HIP_CHECK(hipEventElapsedTime(&t, probe_ev[k], probe_ev[k + 1])); tot += t; }
        *ms = tot; *launches = (int64_t)(probe_used / 2); *bytes = probe_bytes;
        probe_on = false;
    }
    // steady-prefill gate/up products timed since probe_reset: total ms, count, mean rows, flops of one (2 * rows * 2I * H) and its weight bytes
    void probe_read_prefill(double* ms, int64_t* n, double* rows, double* flops, double* wbytes) override {
        HIP_CHECK(hipStreamSynchronize(st));
        double tot = 0;
        for (size_t k = 0; k + 1 < pprobe_used; k += 2) { float t = 0; HIP_CHECK(hipEventElapsedTime(&t, pprobe_ev[k], pprobe_ev[k + 1])); tot += t; }
        const int64_t cnt = (int64_t)(pprobe_used / 2);
        *ms = tot; *n = cnt; *rows = cnt ? pprobe_rows / cnt : 0;
        *flops = 2.0 * (*rows) * 2.0 * I * H; *wbytes = (double)2 * I * H * sizeof(T);
    }
    void phase_times(double* v, double* p, double* d, int reset) override {
        HIP_CHECK(hipStreamSynchronize(st));
        settle_vision();
        *v = ph_ms[0]; *p = ph_ms[1]; *d = ph_ms[2];
        if (reset) ph_ms[0] = ph_ms[1] = ph_ms[2] = 0;
    }

    // ------------------------------------------------------------------------------- op-level entry points
    // refusals of svln_op_gemm* before any launch: `chunk` = operand values per 16-byte LDS-DMA piece (the kernels index K in chunks and
    // stage whole chunks: a K or a row stride off that grid would be truncated or misalign the DMA); launch_gemm knows four epilogues
    void gemm_refusals(const GemmArgs& a, int chunk) {
        REQUIRE(a.A && a.W && a.C, "null pointer");
        REQUIRE(a.M >= 0 && a.N >= 0 && a.K >= 0, "negative GEMM extent");
        REQUIRE(a.epi == EPI_NONE || a.epi == EPI_GELU_TANH || a.epi == EPI_GELU_ERF || a.epi == EPI_SWIGLU,
                "epilogue: EPI_NONE, EPI_GELU_TANH, EPI_GELU_ERF or EPI_SWIGLU");
        REQUIRE(a.K % chunk == 0, "K must be a multiple of the format's 16-byte chunk");
        REQUIRE(a.lda >= a.K && a.ldw >= a.K && a.lda % chunk == 0 && a.ldw % chunk == 0,
                "lda, ldw >= K, multiples of the format's 16-byte chunk (aligned LDS-DMA)");
        REQUIRE(((size_t)a.A & 15) == 0 && ((size_t)a.W & 15) == 0, "A and W must be 16-byte aligned (LDS-DMA)");
        REQUIRE(a.epi != EPI_SWIGLU || a.N % 64 == 0, "SwiGLU needs N % 64 == 0 (32-row gate / up blocks)");
        REQUIRE(a.ldc >= (a.epi == EPI_SWIGLU ? a.N / 2 : a.N), "ldc below the output width");
        REQUIRE(!a.res || a.ldr >= a.N, "residual: ldr below N");
        REQUIRE(a.res_mod >= 0, "negative res_mod");
        REQUIRE(!a.norm_out || a.norm_w, "norm_out without norm_w");
        if (a.force_split > 1) {
            REQUIRE((size_t)a.force_split * a.M * a.N <= gemm_ws_elems, "force_split: S * M * N exceeds the split-K workspace");
            REQUIRE(a.N % 4 == 0, "force_split: N must be a multiple of 4");
        }
    }
    bool op_gemm(const GemmArgs& a0) override {
        GemmArgs a = a0; a.ws = gemm_ws; a.ws_elems = gemm_ws_elems; a.zeros = zero_line;
        gemm_refusals(a, Elt<T>::PER_CHUNK);
        const bool fused = launch_gemm<T>(st, a);
        sync();
        LAUNCH_CHECK("op_gemm");
        return fused;
    }
    // the packed (P12) form of a test GEMV: both planes and the bf16 original, the bf16 engine, K inside the 64-block mask
    void p12_refusals(const GemvArgs& a) {
        if (!a.wp && !a.prec) return;
        REQUIRE(sizeof(T) == 2, "packed weights need the bf16 engine");
        REQUIRE(a.wp && a.prec && a.W, "null pointer (packed blocks, row records and the bf16 original are all needed)");
        REQUIRE(!a.w4 && !a.w8, "one weight format per call");
        REQUIRE(a.K % 8 == 0, "K must be a multiple of 8");
        REQUIRE(a.K <= P12_MAX_K, "packed weights: K above 32768 (64 blocks of 512 per row)");
    }
    void op_pack_rows(const void* w, int ldw, int64_t rows, int cols, void* packed, void* rec, int64_t* fallback_blocks) override {
        REQUIRE(sizeof(T) == 2, "packed weights need the bf16 engine");
        REQUIRE(w && packed && rec, "null pointer");
        REQUIRE(rows >= 0 && rows <= 0x7FFFFFFF && cols >= 8 && cols % 8 == 0, "cols must be a positive multiple of 8");
        REQUIRE(cols <= P12_MAX_K, "packed weights: more than 32768 columns (64 blocks of 512 per row)");
        REQUIRE(ldw >= cols && ldw % 8 == 0, "ldw >= cols, a multiple of 8 (aligned row loads)");
        unsigned* cnt = nullptr;
        HIP_CHECK(hipMalloc((void**)&cnt, sizeof(unsigned)));
        HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned), st));
        if (rows > 0) launch_p12_pack_rows(st, w, ldw, packed, rec, cnt, rows, cols);
        unsigned f = 0;
        HIP_CHECK(hipMemcpyAsync(&f, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        sync();
        HIP_CHECK(hipFree(cnt));
        LAUNCH_CHECK("op_pack_rows");
        if (fallback_blocks) *fallback_blocks = f;
    }
    void op_unpack_rows(const void* packed, const void* rec, const void* w, int ldw, int64_t rows, int cols, void* out) override {
        REQUIRE(sizeof(T) == 2, "packed weights need the bf16 engine");
        REQUIRE(w && packed && rec && out, "null pointer");
        REQUIRE(rows >= 0 && rows <= 0x7FFFFFFF && cols >= 8 && cols % 8 == 0 && cols <= P12_MAX_K, "cols: a positive multiple of 8, at most 32768");
        REQUIRE(ldw >= cols && ldw % 8 == 0, "ldw >= cols, a multiple of 8 (aligned row loads)");
        if (rows > 0) launch_p12_unpack_rows(st, packed, rec, w, ldw, out, cols, rows, cols);
        sync();
        LAUNCH_CHECK("op_unpack_rows");
    }
    void op_gemv(GemvArgs a, int32_t* host_token) override {
        REQUIRE(a.w8 == nullptr || sizeof(T) == 2, "fp8 weights need the bf16 engine");
        REQUIRE(a.w4 == nullptr || sizeof(T) == 2, "MXFP4 weights need the bf16 engine");
        p12_refusals(a);
        // refusals before launch, the same for every weight format: `chunk` = weights per 16-byte load of the format
        const int chunk = a.w4 ? 32 : a.w8 ? 16 : Elt<T>::PER_CHUNK;
        REQUIRE(a.x && (a.w4 ? a.e8 != nullptr : a.w8 ? a.scale != nullptr : a.W != nullptr), "null pointer");
        REQUIRE(a.N >= 1 && a.K >= chunk && a.K % chunk == 0, "N >= 1, K a positive multiple of the format's 16-byte chunk");
        REQUIRE(a.ldw >= a.K && a.ldw % chunk == 0, "ldw >= K, a multiple of the format's 16-byte chunk (aligned row loads)");
        REQUIRE(a.epi == EPI_NONE || a.epi == EPI_SWIGLU || a.epi == EPI_ARGMAX, "epilogue: EPI_NONE, EPI_SWIGLU or EPI_ARGMAX");
        REQUIRE(a.epi != EPI_SWIGLU || a.N % 64 == 0, "SwiGLU needs N % 64 == 0 (32-row gate / up blocks)");
        REQUIRE(a.epi == EPI_ARGMAX || a.y, "null output pointer");
        REQUIRE((a.epi == EPI_NONE && a.N <= 8192) || (size_t)a.K * sizeof(float) <= (size_t)GEMV_ROWS_MAX_LDS,
                "the wave-per-rows kernel stages K fp32 activations in LDS: K too large");
        a.part_val = part_val; a.part_idx = part_idx;
        launch_gemv<T>(st, a);
        if (a.epi == EPI_ARGMAX) {
            merge_head(parts(), gemv_grid(a.N), TOPK_C, 1, head_form(EPI_ARGMAX), out_single(false, false, 0));
            const int t = read_token();
            if (host_token) *host_token = t;
        }
        sync();
    }
    // TEST-ONLY: one lm_head product in its plain (host_logprob null: EPI_ARGMAX) or scored (EPI_ARGMAX_LSE) form with optional penalty flags
    // smp: the sampled form (EPI_SAMPLE) on the given temperature, seed, streams and draws, whatever the engine's own switch says
    // the refusals the single-env head's test entries share (max_lds: the dynamic LDS the instantiation may ask for)
    void head_op_refusals(const GemvArgs& a, const int32_t* host_token, int max_lds) {
        REQUIRE(a.w8 == nullptr || sizeof(T) == 2, "fp8 weights need the bf16 engine");
        REQUIRE(a.w4 == nullptr || sizeof(T) == 2, "MXFP4 weights need the bf16 engine");
        p12_refusals(a);
        const int chunk = a.w4 ? 32 : a.w8 ? 16 : Elt<T>::PER_CHUNK;
        REQUIRE(a.x && host_token && (a.w4 ? a.e8 != nullptr : a.w8 ? a.scale != nullptr : a.W != nullptr), "null pointer");
        REQUIRE(a.N >= 1 && a.K >= chunk && a.K % chunk == 0, "N >= 1, K a positive multiple of the format's 16-byte chunk");
        REQUIRE(a.ldw >= a.K && a.ldw % chunk == 0, "ldw >= K, a multiple of the format's 16-byte chunk (aligned row loads)");
        REQUIRE((size_t)a.K * sizeof(float) <= (size_t)max_lds, "the wave-per-rows kernel stages K fp32 activations in LDS: K too large");
        REQUIRE(!a.pen_flags || a.pen > 0.0f, "penalty flags need a factor > 0");
    }
    // en: the single-env head with svln_token_entropy on -- the EPI_*_ENT product, entropy_merge_kernel and the scored (or, with smp,
    // sampled) final kernel; everything the three launches wrote goes to the host
    void op_ent_refusals(const OpEntOut* en, const float* host_logprobs, bool sampled) {
        if (!en) return;
        REQUIRE(host_logprobs && en->ent && en->pv && en->pi && en->ps && en->pe && en->n_part && (!sampled || (en->pr && en->pm)), "null output pointer");
    }
    // after merge_head: the copies of `rows` rows of n partials each (the arrays of p; the entropies de) to the host, on the stream
    void op_ent_out(const OpEntOut& en, int rows, int n, const HeadParts& p, bool sampled, const float* de) {
        const size_t nb = (size_t)rows * n;
        HIP_CHECK(hipMemcpyAsync(en.ent, de, rows * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(en.pv, p.val, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(en.pi, p.idx, nb * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(en.ps, p.sum, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(en.pe, p.ent, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        if (sampled) {
            HIP_CHECK(hipMemcpyAsync(en.pr, p.raw, nb * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(en.pm, p.max, nb * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        *en.n_part = n;
    }
    // the form a test entry asks for with its arguments, whatever the engine's switches say
    static HeadForm op_form(bool scored, bool sampled, bool lists, bool ent) { return HeadForm{scored && !sampled, sampled, false, lists, ent}; }
    void op_gemv_scores(GemvArgs a, int32_t* host_token, float* host_logprob, const OpSample* smp, const OpEntOut* en) override {
        head_op_refusals(a, host_token, GEMV_ROWS_MAX_LDS);
        op_ent_refusals(en, host_logprob, smp != nullptr);
        if (en) ensure_ent_buffers();
        const HeadForm f = op_form(host_logprob, smp, false, en);
        if (smp) a.smp = op_sample_args(*smp, 1, part_raw, part_max, host_logprob != nullptr);
        aim(a, parts(), f);
        launch_gemv<T>(st, a);
        merge_head(parts(), gemv_grid(a.N), TOPK_C, 1, f, out_single(false, false, 0));
        if (en) op_ent_out(*en, 1, gemv_grid(a.N), parts(), f.smp, d_ent);
        if (host_logprob) HIP_CHECK(hipMemcpyAsync(h_scores, d_scores, sizeof(float), hipMemcpyDeviceToHost, st));
        *host_token = read_token();
        if (host_logprob) *host_logprob = h_scores[0];
        LAUNCH_CHECK("op_gemv_scores");
    }
    // TEST-ONLY: the single-env head with svln_top_logprobs on -- the EPI_*_TOPK product, the scored (or, with smp, sampled) final kernel
    // and topk_merge_kernel -- on caller-given operands; everything the three launches wrote goes to the host
    void op_gemv_topk(GemvArgs a, int k, const OpSample* smp, int32_t* host_token, float* host_logprob, float* pv, int32_t* pi, float* ps,
                      float* pr, float* pm, float* cv, int32_t* ci, int32_t* top_ids, float* top_lp, int32_t* n_part) override {
        head_op_refusals(a, host_token, GEMV_ROWS_TOPK_MAX_LDS);
        REQUIRE(host_logprob && pv && pi && ps && cv && ci && top_ids && top_lp && n_part && (!smp || (pr && pm)), "null output pointer");
        REQUIRE(k >= 1 && k <= TOPK_C, "k must be 1 .. 8");
        const int np = gemv_grid(a.N);
        ensure_topk_buffers();
        float* d_cv = cand_val_b; int *d_ci = cand_idx_b, *d_ti = d_topi_b; float* d_tl = d_topl_b;      // (the batched heads' buffers: idle in a test entry)
        const HeadForm f = op_form(true, smp, true, false);
        HeadParts p = parts(); p.cand_val = d_cv; p.cand_idx = d_ci;
        HeadOut o = out_single(false, false, k); o.top_ids = d_ti; o.top_lp = d_tl;
        if (smp) a.smp = op_sample_args(*smp, 1, part_raw, part_max, true);
        aim(a, p, f);
        launch_gemv<T>(st, a);
        merge_head(p, np, TOPK_C, 1, f, o);
        hipError_t err = hipMemcpyAsync(h_scores, d_scores, sizeof(float), hipMemcpyDeviceToHost, st);
        auto back = [&](void* dst, const void* src, size_t bytes) { if (err == hipSuccess) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); };
        back(pv, part_val, np * sizeof(float)); back(pi, part_idx, np * sizeof(int)); back(ps, part_sum, np * sizeof(float));
        if (smp) { back(pr, part_raw, np * sizeof(float)); back(pm, part_max, np * sizeof(float)); }
        back(cv, d_cv, (size_t)np * TOPK_C * sizeof(float)); back(ci, d_ci, (size_t)np * TOPK_C * sizeof(int));
        back(top_ids, d_ti, k * sizeof(int)); back(top_lp, d_tl, k * sizeof(float));
        back(h_token, d_token, sizeof(int));
        const hipError_t err2 = hipStreamSynchronize(st);
        HIP_CHECK(err); HIP_CHECK(err2);
        *host_token = h_token[0]; *host_logprob = h_scores[0]; *n_part = np;
        LAUNCH_CHECK("op_gemv_topk");
    }
    void batched_scores_out(int B, int32_t* host_tokens, float* host_logprobs, const char* who) {
        HIP_CHECK(hipMemcpyAsync(h_tok_b, d_tok_b, B * sizeof(int), hipMemcpyDeviceToHost, st));
        if (host_logprobs) HIP_CHECK(hipMemcpyAsync(h_score_b, d_score_b, B * sizeof(float), hipMemcpyDeviceToHost, st));
        sync();
        LAUNCH_CHECK(who);
        for (int b = 0; b < B; ++b) { host_tokens[b] = h_tok_b[b]; if (host_logprobs) host_logprobs[b] = h_score_b[b]; }
    }
    // the batched test entries under svln_top_logprobs: stage the candidate form (before the launch) ...
    void op_topk_rows_refusals(const OpTopkRows* tk, const float* host_logprobs) {
        if (!tk) return;
        REQUIRE(host_logprobs && tk->cv && tk->ci && tk->top_ids && tk->top_lp && tk->n_part, "null output pointer");
        REQUIRE(tk->k >= 1 && tk->k <= TOPK_C, "k must be 1 .. 8");
    }
    // ... and read candidates and lists back (after merge_head)
    void op_topk_rows_out(const OpTopkRows& tk, int rows, int n) {
        const size_t nc = (size_t)rows * n * TOPK_C;
        HIP_CHECK(hipMemcpyAsync(tk.cv, cand_val_b, nc * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(tk.ci, cand_idx_b, nc * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(tk.top_ids, d_topi_b, (size_t)rows * tk.k * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(tk.top_lp, d_topl_b, (size_t)rows * tk.k * sizeof(float), hipMemcpyDeviceToHost, st));
        *tk.n_part = n;
    }
    void op_gemv_batched_scores(GemvBatchArgs a, int32_t* host_tokens, float* host_logprobs, const OpSample* smp, const OpTopkRows* tk,
                                const OpEntOut* en) override {
        REQUIRE(a.W && a.x && host_tokens, "null pointer");
        REQUIRE(a.B == 1 || a.B == 2 || a.B == 4 || a.B == 8, "B must be 1, 2, 4 or 8");
        REQUIRE(a.N >= 1 && a.K >= Elt<T>::PER_CHUNK && a.K % Elt<T>::PER_CHUNK == 0, "N >= 1, K a positive multiple of the 16-byte chunk");
        REQUIRE(a.ldw >= a.K && a.ldw % Elt<T>::PER_CHUNK == 0 && a.ldx >= a.K && a.ldx % Elt<T>::PER_CHUNK == 0, "ldw, ldx >= K, multiples of the 16-byte chunk");
        REQUIRE(!a.pen_flags || (a.pen_rows && a.pen > 0.0f), "penalty flags come with their row table and a factor > 0");
        REQUIRE(!smp || !a.norm_w, "the sampled batched GEMV has no fused-norm form");
        REQUIRE(!tk || !a.norm_w, "the candidate form of the batched GEMV has no fused-norm form");
        REQUIRE(!en || (!a.norm_w && !tk), "the entropy form of the batched GEMV has no fused-norm form and no candidates");
        op_topk_rows_refusals(tk, host_logprobs);
        op_ent_refusals(en, host_logprobs, smp != nullptr);
        if (tk) ensure_topk_buffers();
        if (en) ensure_ent_buffers();
        const HeadForm f = op_form(host_logprobs, smp, tk, en);
        const int n = gemv_batched_grid(a.N, EPI_ARGMAX, a.B);
        HeadOut o = out_rows(0, tk ? tk->k : 0);
        a.row_scale = row_scale_b;
        if (host_logprobs && a.norm_w) o.row_scale = row_scale_b;
        if (smp) a.smp = op_sample_args(*smp, a.B, part_raw_b, part_max_b, host_logprobs != nullptr);
        aim(a, parts_b(), f);
        launch_gemv_batched<T>(st, a);
        merge_head(parts_b(), n, TOPK_C, a.B, f, o);
        if (tk) op_topk_rows_out(*tk, a.B, n);
        if (en) op_ent_out(*en, a.B, n, parts_b(), f.smp, d_ent_b);
        batched_scores_out(a.B, host_tokens, host_logprobs, "op_gemv_batched_scores");
    }
    void op_gemm_argmax_scores(GemmArgs a, int32_t* host_tokens, float* host_logprobs, const OpSample* smp, const OpTopkRows* tk,
                               const OpEntOut* en) override {
        constexpr int chunk = Elt<T>::PER_CHUNK;
        REQUIRE(a.A && a.W && host_tokens, "null pointer");
        REQUIRE(a.M >= 1 && a.M <= 32 && a.N >= 1 && (a.N + 127) / 128 <= 2048, "1 <= M <= 32 rows, 1 <= N <= 262144");
        REQUIRE(a.K >= chunk && a.K % chunk == 0 && a.lda >= a.K && a.ldw >= a.K && a.lda % chunk == 0 && a.ldw % chunk == 0,
                "K a positive multiple of the 16-byte chunk; lda, ldw >= K, multiples of it (aligned LDS-DMA)");
        REQUIRE(((size_t)a.A & 15) == 0 && ((size_t)a.W & 15) == 0, "A and W must be 16-byte aligned (LDS-DMA)");
        REQUIRE(!a.pen_flags || (a.pen_rows && a.pen > 0.0f), "penalty flags come with their row table and a factor > 0");
        REQUIRE(!en || !tk, "the entropy form has no candidates");
        op_topk_rows_refusals(tk, host_logprobs);
        op_ent_refusals(en, host_logprobs, smp != nullptr);
        if (tk) ensure_topk_buffers();
        if (en) ensure_ent_buffers();
        const HeadForm f = op_form(host_logprobs, smp, tk, en);
        a.zeros = zero_line;
        if (smp) a.smp = op_sample_args(*smp, a.M, part_raw_b, part_max_b, host_logprobs != nullptr);
        aim(a, parts_b(), f);
        const int n = launch_gemm_argmax<T>(st, a);
        merge_head(parts_b(), n, TOPK_C, a.M, f, out_rows(0, tk ? tk->k : 0));
        if (tk) op_topk_rows_out(*tk, a.M, n);
        if (en) op_ent_out(*en, a.M, n, parts_b(), f.smp, d_ent_b);
        batched_scores_out(a.M, host_tokens, host_logprobs, "op_gemm_argmax_scores");
    }
    void op_gemv_batched(GemvBatchArgs a, int32_t* host_tokens) override {
        REQUIRE(a.B == 1 || a.B == 2 || a.B == 4 || a.B == 8, "B must be 1, 2, 4 or 8");
        REQUIRE(a.K % Elt<T>::PER_CHUNK == 0 && a.N >= 1, "bad GEMV extents");
        REQUIRE(a.epi != EPI_SWIGLU || a.N % 64 == 0, "SwiGLU needs N % 64 == 0 (32-row gate / up blocks)");
        a.part_val = part_val_b; a.part_idx = part_idx_b;
        // (argmax_rows follows the engine's switches: under svln_set_sampling it would sample on whatever rows d_smp last held)
        if (a.epi == EPI_ARGMAX && !a.norm_w) refuse(C_OP_GEMV_BATCHED_ARGMAX);
        if (a.epi == EPI_ARGMAX && !a.norm_w) argmax_rows(a.W, a.ldw, (const T*)a.x, a.ldx, a.N, a.K, a.B, false);      // the engine's own routing (MFMA tiles from B = 4)
        else launch_gemv_batched<T>(st, a);
        if (a.epi == EPI_ARGMAX) {
            if (a.norm_w) merge_head(parts_b(), gemv_batched_grid(a.N, EPI_ARGMAX, a.B), TOPK_C, a.B, head_form(EPI_ARGMAX), out_rows(0, 0));
            HIP_CHECK(hipMemcpyAsync(h_tok_b, d_tok_b, a.B * sizeof(int), hipMemcpyDeviceToHost, st));
            sync();
            if (host_tokens) for (int b = 0; b < a.B; ++b) host_tokens[b] = h_tok_b[b];
        }
        sync();
        LAUNCH_CHECK("op_gemv_batched");
    }
    void op_gemv_mxfp4_batched(GemvMx4BatchArgs a, int32_t* host_tokens) override {
        // refusals before any launch
        REQUIRE(sizeof(T) == 2, "MXFP4 weights need the bf16 engine");
        REQUIRE(a.q4 && a.e8 && a.x, "null pointer");
        REQUIRE(a.B >= 1 && a.B <= MAXB, "B must be 1 .. 8");
        REQUIRE(a.N >= 1 && a.K >= 32 && a.K % 32 == 0, "N >= 1, K a positive multiple of 32");
        REQUIRE(a.ldw >= a.K && a.ldw % 32 == 0, "ldw >= K, a multiple of 32");
        REQUIRE(a.ldx >= a.K && a.ldx % 8 == 0, "ldx >= K, a multiple of 8 (aligned 16-byte loads)");
        REQUIRE(a.epi == EPI_NONE || a.epi == EPI_SWIGLU || a.epi == EPI_ARGMAX, "epilogue: EPI_NONE, EPI_SWIGLU or EPI_ARGMAX");
        REQUIRE(a.epi != EPI_SWIGLU || a.N % 64 == 0, "SwiGLU needs N % 64 == 0 (32-row gate / up blocks)");
        REQUIRE(a.epi == EPI_ARGMAX || a.y, "null output pointer");
        REQUIRE(!a.pen_flags || (a.epi == EPI_ARGMAX && a.pen_rows && a.pen > 0.0f), "penalty flags: arg-max only, with their row table and a factor > 0");
        a.part_val = part_val_b; a.part_idx = part_idx_b;
        launch_gemv_mx4b(st, a);
        if (a.epi == EPI_ARGMAX) {
            merge_head(parts_b(), gemv_mx4b_grid(a.N, EPI_ARGMAX), TOPK_C, a.B, head_form(EPI_ARGMAX), out_rows(0, 0));
            HIP_CHECK(hipMemcpyAsync(h_tok_b, d_tok_b, a.B * sizeof(int), hipMemcpyDeviceToHost, st));
            sync();
            if (host_tokens) for (int b = 0; b < a.B; ++b) host_tokens[b] = h_tok_b[b];
        }
        sync();
        LAUNCH_CHECK("op_gemv_mxfp4_batched");
    }
    void op_quant_fp8(const void* w, int64_t rows, int cols, void* w8, float* scale) override {
        REQUIRE(sizeof(T) == 2, "fp8 quantisation reads bf16 weights");
        REQUIRE(w && w8 && scale, "null pointer");
        REQUIRE(rows >= 0 && rows <= INT32_MAX && cols > 0 && cols % 16 == 0, "rows must be >= 0 and cols a positive multiple of 16");
        if (rows > 0) launch_quant_fp8_rows(st, w, cols, w8, scale, rows, cols);
        sync();
        LAUNCH_CHECK("op_quant_fp8");
    }
    void op_quant_mxfp4(const void* w, int64_t rows, int cols, void* q4, uint8_t* e8) override {
        REQUIRE(sizeof(T) == 2, "MXFP4 quantisation reads bf16 weights");
        REQUIRE(w && q4 && e8, "null pointer");
        REQUIRE(rows >= 0 && cols > 0 && cols % 32 == 0, "cols must be a positive multiple of 32");
        if (rows > 0) launch_quant_mxfp4_rows(st, w, cols, q4, e8, rows, cols);
        sync();
        LAUNCH_CHECK("op_quant_mxfp4");
    }
    // ---- row helpers (misc.hip).  The ops check what the engine's own callers guarantee; lists arrive on the host, are range-checked and
    // go to a device buffer that lives for the call.  Test surface only, not for a hot path: every call allocates and frees device memory
    // (hipFree synchronises the device) and ends with a stream sync.
    void require_row_width(int n) {
        constexpr int EPC = Elt<T>::PER_CHUNK;
        REQUIRE(n > 0 && n % EPC == 0,
                std::string("n must be a positive multiple of the 16-byte chunk (") + std::to_string(EPC) + " values of the engine type)");
    }
    struct OpInts {          // `count` ints on the device for the length of one op
        int* d = nullptr;
        OpInts(const int32_t* host, size_t count) {
            HIP_CHECK(hipMalloc((void**)&d, (count ? count : 1) * sizeof(int)));
            if (count && hipMemcpy(d, host, count * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipFree(d);
                REQUIRE(false, "op: list upload failed");
            }
        }
        ~OpInts() { (void)hipFree(d); }
        OpInts(const OpInts&) = delete;
        OpInts& operator=(const OpInts&) = delete;
    };
    void op_rmsnorm(const void* xi, const void* g, void* y, int rows, int n, float eps) override {
        REQUIRE(xi && g && y, "null pointer");
        REQUIRE(rows >= 0, "rows must be >= 0");
        require_row_width(n);
        launch_rmsnorm<T>(st, xi, g, y, rows, n, eps);
        sync();
        LAUNCH_CHECK("op_rmsnorm");
    }
    void op_layernorm(const void* xi, const void* g, const void* b, void* y, int rows, int n, float eps) override {
        REQUIRE(xi && g && b && y, "null pointer");
        REQUIRE(rows >= 0, "rows must be >= 0");
        require_row_width(n);
        launch_layernorm<T>(st, xi, g, b, y, rows, n, eps);
        sync();
        LAUNCH_CHECK("op_layernorm");
    }
    void op_rmsnorm_tap(const void* xi, const void* g, void* y, int rows, int n, float eps, int skip_value, void* y2, int y2_row_value,
                        int y2_cap) override {
        REQUIRE(xi && g && y && y2, "null pointer");
        REQUIRE(rows >= 0, "rows must be >= 0");
        require_row_width(n);
        REQUIRE(y2_cap >= 1 && y2_row_value >= 0, "y2_cap must be >= 1 and y2_row >= 0");
        const int32_t words[2] = {skip_value, y2_row_value};
        OpInts d(words, 2);
        launch_rmsnorm<T>(st, xi, g, y, rows, n, eps, d.d, y2, d.d + 1, y2_cap);
        sync();
        LAUNCH_CHECK("op_rmsnorm_tap");
    }
    void op_rmsnorm_indexed(const void* xi, int x_rows, const void* g, void* y, const int32_t* src_rows, const int32_t* tap_rows, void* tap,
                            int tap_cap, int rows, int n, float eps) override {
        REQUIRE(xi && g && y && src_rows && tap_rows && tap, "null pointer");
        REQUIRE(rows >= 0 && x_rows >= 1 && tap_cap >= 1, "rows must be >= 0, x_rows and tap_cap >= 1");
        require_row_width(n);
        for (int r = 0; r < rows; ++r) {
            REQUIRE(src_rows[r] >= 0 && src_rows[r] < x_rows, "src_rows entry out of range");
            REQUIRE(tap_rows[r] >= -1 && tap_rows[r] < tap_cap, "tap_rows entry out of range");
        }
        std::vector<int32_t> both(src_rows, src_rows + rows);
        both.insert(both.end(), tap_rows, tap_rows + rows);
        OpInts d(both.data(), both.size());
        launch_rmsnorm_indexed<T>(st, xi, g, y, d.d, d.d + rows, tap, rows, n, eps);
        sync();
        LAUNCH_CHECK("op_rmsnorm_indexed");
    }
    void op_gather_rows(const int32_t* src, int rows, const void* emb, int embed_rows, const void* ft, int feat_rows, void* out, int n,
                        int skip_value) override {
        REQUIRE(src && emb && ft && out, "null pointer");
        REQUIRE(rows >= 0 && embed_rows >= 1 && feat_rows >= 1, "rows must be >= 0, embed_rows and feat_rows >= 1");
        require_row_width(n);
        for (int r = 0; r < rows; ++r) REQUIRE(src[r] < embed_rows && src[r] >= -feat_rows, "src entry out of range");
        std::vector<int32_t> h(src, src + rows);
        h.push_back(skip_value);
        OpInts d(h.data(), h.size());
        launch_gather_rows<T>(st, d.d, emb, ft, out, rows, n, d.d + rows);
        sync();
        LAUNCH_CHECK("op_gather_rows");
    }
    void op_gather_rows_ragged(const int32_t* list, int rows, const void* emb, int embed_rows, void* out, int out_rows, int n) override {
        REQUIRE(list && emb && out, "null pointer");
        REQUIRE(rows >= 0 && embed_rows >= 1 && out_rows >= 1, "rows must be >= 0, embed_rows and out_rows >= 1");
        require_row_width(n);
        for (int r = 0; r < rows; ++r) {
            REQUIRE(list[2 * r] >= 0 && list[2 * r] < out_rows, "destination row out of range");
            REQUIRE(list[2 * r + 1] >= 0 && list[2 * r + 1] < embed_rows, "token id out of range");
        }
        OpInts d(list, (size_t)2 * rows);
        launch_gather_rows_ragged<T>(st, d.d, emb, out, rows, n);
        sync();
        LAUNCH_CHECK("op_gather_rows_ragged");
    }
    void op_frame_hash(const void* p, int F, int64_t words_per_frame, uint64_t* out_keys) override {
        REQUIRE(p && out_keys, "null pointer");
        REQUIRE(F >= 1 && F <= 65535 && words_per_frame >= 1 && words_per_frame <= ((int64_t)1 << 32),
                "F must be 1 .. 65535, words_per_frame 1 .. 2^32");
        unsigned long long* dk = nullptr;
        HIP_CHECK(hipMalloc((void**)&dk, (size_t)2 * F * sizeof(unsigned long long)));
        hipError_t e = hipMemsetAsync(dk, 0, (size_t)2 * F * sizeof(unsigned long long), st);
        if (e == hipSuccess) {
            launch_frame_hash(st, (const float*)p, F, (size_t)words_per_frame, dk);
            e = hipStreamSynchronize(st);
        }
        if (e == hipSuccess) e = hipMemcpy(out_keys, dk, (size_t)2 * F * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        (void)hipFree(dk);
        HIP_CHECK(e);
        LAUNCH_CHECK("op_frame_hash");
    }
    // ---- attention ops.  An op resets the envs it uses on entry (never on exit: svln_op_kv_read sees what the op wrote) and gives each
    // the pages op_set_pages fixed for it, in that order, or else pages from the free list.
    std::vector<std::vector<int>> op_pages;
    void op_env_begin(int env, int positions) {
        Env& e = env_at(env);
        reset_env(env);
        const std::vector<int> want = env < (int)op_pages.size() ? op_pages[env] : std::vector<int>();
        if (want.empty()) { ensure_pages(e, positions); return; }
        const int need = (positions + PAGE - 1) / PAGE;
        REQUIRE(need <= (int)want.size(), "op_set_pages: fewer pages than the op's positions need");
        for (int i = 0; i < need; ++i) {
            auto it = std::find(free_pages.begin(), free_pages.end(), want[i]);
            REQUIRE(it != free_pages.end(), "op_set_pages: page is held by another env");
            free_pages.erase(it);
            e.pages[e.n_pages++] = want[i];
        }
        HIP_CHECK(hipMemcpyAsync(e.d_pages, e.pages.data(), need * sizeof(int), hipMemcpyHostToDevice, st));
    }
    void op_set_pages(int env, const int32_t* pages, int n) override {
        env_at(env);
        REQUIRE(n >= 0 && n <= pages_per_env && (n == 0 || pages), "op_set_pages: 0 .. pages_per_env pages");
        std::vector<int> v(pages, pages + n);
        for (int p : v) REQUIRE(p >= 0 && p < pages_total, "op_set_pages: page out of range");
        if ((int)op_pages.size() < c.max_envs) op_pages.resize(c.max_envs);
        op_pages[env] = v;
    }
    static void host_from_f32(float v, float& out) { out = v; }
    static void host_from_f32(float v, bf16& out) {       // round to nearest even (finite values)
        uint32_t u; std::memcpy(&u, &v, 4);
        const unsigned short b = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        std::memcpy(&out, &b, 2);
    }
    // layer-0 K / V^T pools := pool_value (rounded to the engine dtype; finite: masked keys meet stale data in production too),
    // split-KV partials := NaN (part_nan): a slot an op leaves unwritten, or a partial the merge reads without a workgroup having
    // written it, then shows in the output
    void op_fill_attn_state(float pool_value, int part_nan) override {
        REQUIRE(std::isfinite(pool_value), "the pool value must be finite");
        const LLayer& L = ll[0];
        const size_t n = (size_t)pages_total * nkv * PAGE * 128;
        T v; host_from_f32(pool_value, v);
        std::vector<T> h(n, v);
        sync();
        HIP_CHECK(hipMemcpy(L.kpool, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(L.vpool, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
        if (part_nan) HIP_CHECK(hipMemsetAsync(attn_part, 0xff, attn_part_elems * sizeof(float), st));
        sync();
    }
    // roped K and V rows of positions [start, start + n) of env's layer-0 pages -> fp32 [n][nkv][128] each.  env = -1: the raw pools,
    // position p = slot p % 64 of physical page p / 64 (every page, whoever holds it)
    void op_kv_read(int env, int start, int n, float* k_out, float* v_out) override { kv_read(ll[0], env, start, n, k_out, v_out); }
    void op_kv_pool_read(int layer, int start, int n, float* k_out, float* v_out) override {
        REQUIRE(layer >= 0 && layer < c.layers, "op_kv_pool_read: no such layer");
        kv_read(ll[layer], -1, start, n, k_out, v_out);
    }
    // TEST-ONLY: the fork launch of svln_generate_group on caller-given pages; every refusal comes before the launch
    void op_kv_page_copy(int src_page, const int32_t* dst_pages, int n_dst) override {
        REQUIRE(dst_pages, "svln_op_kv_page_copy: null page list");
        REQUIRE(n_dst >= 1 && n_dst <= FORK_MAX_DST, "svln_op_kv_page_copy: n_dst must be 1 .. 7");
        REQUIRE(src_page >= 0 && src_page < pages_total, "svln_op_kv_page_copy: source page outside the pool");
        for (int d = 0; d < n_dst; ++d) {
            const int p = dst_pages[d];
            REQUIRE(p >= 0 && p < pages_total, "svln_op_kv_page_copy: destination page outside the pool");
            REQUIRE(p != src_page, "svln_op_kv_page_copy: a destination equals the source");
            for (int q = 0; q < d; ++q) REQUIRE(dst_pages[q] != p, "svln_op_kv_page_copy: a destination is listed twice");
            for (const Env& e : envs)
                for (int i = 0; i < e.n_pages; ++i) REQUIRE(e.pages[i] != p, "svln_op_kv_page_copy: a destination is held by an env");
            for (int g = 1; g < MAXB; ++g)
                for (int t : grp.tail[g]) REQUIRE(t != p, "svln_op_kv_page_copy: a destination is held by a pending group");
        }
        sync();
        for (int d = 0; d < n_dst; ++d) h_fork_dst[d] = dst_pages[d];
        fork_page_copy(src_page, n_dst);
        sync();
        LAUNCH_CHECK("op_kv_page_copy");
    }
    // the device workspace of the beam ops (allocated on first use): two hypothesis states of BEAM_OP_LEN ids per row, the lists of 8 rows,
    // the page sets, the pair lists, the record, the EOS list and the fed tokens
    static constexpr int BEAM_OP_LEN = 64, BEAM_OP_PAIRS = BEAM_MAX_W * BEAM_CP_MAX;
    BeamHdr* bm_hdr[2] = {nullptr, nullptr};
    int *bm_ids[2] = {nullptr, nullptr}, *bm_list_ids = nullptr, *bm_sets = nullptr, *bm_pair_src = nullptr, *bm_pair_dst = nullptr, *bm_rec = nullptr,
        *bm_eos = nullptr, *bm_tok = nullptr;
    float *bm_lps[2] = {nullptr, nullptr}, *bm_list_lps = nullptr;
    int bm_len_cap = 0;                              // ids per row of the two states: what a beam turn can emit
    T* bm_tap = nullptr;                             // copy of the parity taps while a beam turn reorders them by rank
    void ensure_beam_buffers() {
        if (bm_hdr[0]) return;
        bm_len_cap = std::min(std::max(BEAM_OP_LEN, c.max_positions), BEAM_CP_MAX * PAGE + 64);     // (a turn of <= 8 tail pages emits <= 513 ids)
        for (int k = 0; k < 2; ++k) {
            bm_hdr[k] = dalloc<BeamHdr>(1, true);
            bm_ids[k] = dalloc<int>((size_t)BEAM_MAX_W * bm_len_cap, true); bm_lps[k] = dalloc<float>((size_t)BEAM_MAX_W * bm_len_cap, true);
        }
        bm_list_ids = dalloc<int>(BEAM_MAX_W * BEAM_MAX_W, true); bm_list_lps = dalloc<float>(BEAM_MAX_W * BEAM_MAX_W, true);
        bm_sets = dalloc<int>(2 * BEAM_MAX_W * BEAM_CP_MAX, true);
        bm_pair_src = dalloc<int>(BEAM_OP_PAIRS, true); bm_pair_dst = dalloc<int>(BEAM_OP_PAIRS, true);
        bm_rec = dalloc<int>(BEAM_REC, true); bm_eos = dalloc<int>((size_t)std::max(V, 64), true); bm_tok = dalloc<int>(64, true);
    }
    // TEST-ONLY: one launch of kv_page_gather_kernel on caller-given pairs; every refusal comes before the launch
    void op_beam_page_gather(const int32_t* src_pages, const int32_t* dst_pages, int n) override {
        const char* who = "svln_op_beam_page_gather";
        REQUIRE(src_pages && dst_pages, std::string(who) + ": null page list");
        REQUIRE(n >= 1 && n <= BEAM_OP_PAIRS, std::string(who) + ": n must be 1 .. 64");
        for (int i = 0; i < n; ++i) {
            const int s = src_pages[i], p = dst_pages[i];
            REQUIRE(s >= 0 && s < pages_total, std::string(who) + ": source page outside the pool");
            REQUIRE(p >= 0 && p < pages_total, std::string(who) + ": destination page outside the pool");
            for (int q = 0; q < n; ++q) REQUIRE(src_pages[q] != p, std::string(who) + ": a page is both a source and a destination");
            for (int q = 0; q < i; ++q) REQUIRE(dst_pages[q] != p, std::string(who) + ": a destination is listed twice");
            for (const Env& e : envs)
                for (int k = 0; k < e.n_pages; ++k) REQUIRE(e.pages[k] != p, std::string(who) + ": a destination is held by an env");
            for (int g = 1; g < MAXB; ++g)
                for (int t : grp.tail[g]) REQUIRE(t != p, std::string(who) + ": a destination is held by a pending group");
        }
        ensure_beam_buffers();
        sync();
        HIP_CHECK(hipMemcpy(bm_pair_src, src_pages, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(bm_pair_dst, dst_pages, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        launch_kv_page_gather<T>(st, d_pool_tab, 2 * c.layers, bm_pair_src, bm_pair_dst, n, (int64_t)nkv * PAGE * 128);
        sync();
        LAUNCH_CHECK("op_beam_page_gather");
    }
    // TEST-ONLY: one launch of beam_select_kernel on a caller-given hypothesis set and lists; every refusal comes before the launch.
    // hdr = int32 [25]: n, len[8], fin[8], set_of[8]
    void op_beam_select(int W, int limit, int B, int n_cp, int len_cap, const int32_t* eos, int n_eos, const int32_t* list_ids, const float* list_lps,
                        const int32_t* hdr_in, const float* score_in, const int32_t* ids_in, const float* lps_in, const int32_t* set_pages,
                        int32_t* hdr_out, float* score_out, int32_t* ids_out, float* lps_out, int32_t* tok_b, int32_t* pair_src, int32_t* pair_dst,
                        int32_t* rec) override {
        const char* who = "svln_op_beam_select";
        REQUIRE(list_ids && list_lps && hdr_in && score_in && ids_in && lps_in && hdr_out && score_out && ids_out && lps_out && tok_b && pair_src &&
                    pair_dst && rec, std::string(who) + ": null pointer");
        REQUIRE(W >= 1 && W <= BEAM_MAX_W, std::string(who) + ": W must be 1 .. 8");
        REQUIRE(len_cap >= 1 && len_cap <= BEAM_OP_LEN, std::string(who) + ": len_cap must be 1 .. 64");
        REQUIRE(limit >= 1 && limit <= len_cap, std::string(who) + ": limit must be 1 .. len_cap");
        REQUIRE(B >= 1 && B <= 64, std::string(who) + ": B must be 1 .. 64");
        REQUIRE(n_cp >= 0 && n_cp <= BEAM_CP_MAX && (n_cp == 0 || set_pages), std::string(who) + ": n_cp must be 0 .. 8 (with the page sets)");
        REQUIRE(n_eos >= 0 && n_eos <= 64 && (n_eos == 0 || eos), std::string(who) + ": n_eos must be 0 .. 64 (with the list)");
        BeamHdr hi;
        hi.n = hdr_in[0];
        REQUIRE(hi.n >= 0 && hi.n <= BEAM_MAX_W, std::string(who) + ": the set holds 0 .. 8 hypotheses");
        for (int r = 0; r < BEAM_MAX_W; ++r) {
            hi.len[r] = hdr_in[1 + r]; hi.fin[r] = hdr_in[1 + BEAM_MAX_W + r]; hi.set_of[r] = hdr_in[1 + 2 * BEAM_MAX_W + r]; hi.score[r] = score_in[r];
            if (r >= hi.n) continue;
            REQUIRE(hi.fin[r] == 0 || hi.fin[r] == 1, std::string(who) + ": a finished flag must be 0 or 1");
            REQUIRE(hi.len[r] >= 0 && hi.len[r] <= len_cap && (hi.fin[r] || hi.len[r] < limit), std::string(who) + ": a length must be 0 .. len_cap, below limit for a live hypothesis");
            REQUIRE(hi.set_of[r] >= 0 && hi.set_of[r] < 2 * BEAM_MAX_W, std::string(who) + ": a page set must be 0 .. 15");
            for (int q = 0; q < r; ++q) REQUIRE(hi.set_of[q] != hi.set_of[r], std::string(who) + ": two hypotheses hold one page set");
        }
        ensure_beam_buffers();
        sync();
        const size_t rows = (size_t)BEAM_MAX_W * len_cap;
        HIP_CHECK(hipMemcpy(bm_hdr[0], &hi, sizeof(BeamHdr), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemsetAsync(bm_hdr[1], 0xff, sizeof(BeamHdr), st));
        HIP_CHECK(hipMemcpy(bm_ids[0], ids_in, rows * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(bm_lps[0], lps_in, rows * sizeof(float), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(bm_ids[1], ids_out, rows * sizeof(int), hipMemcpyHostToDevice));        // (what the kernel leaves alone keeps the caller's bytes)
        HIP_CHECK(hipMemcpy(bm_lps[1], lps_out, rows * sizeof(float), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(bm_list_ids, list_ids, (size_t)BEAM_MAX_W * W * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(bm_list_lps, list_lps, (size_t)BEAM_MAX_W * W * sizeof(float), hipMemcpyHostToDevice));
        if (n_cp) HIP_CHECK(hipMemcpy(bm_sets, set_pages, (size_t)2 * BEAM_MAX_W * n_cp * sizeof(int), hipMemcpyHostToDevice));
        if (n_eos) HIP_CHECK(hipMemcpy(bm_eos, eos, (size_t)n_eos * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(bm_tok, tok_b, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemsetAsync(bm_pair_src, 0xff, BEAM_OP_PAIRS * sizeof(int), st));
        HIP_CHECK(hipMemsetAsync(bm_pair_dst, 0xff, BEAM_OP_PAIRS * sizeof(int), st));
        BeamSelectArgs a;
        a.list_ids = bm_list_ids; a.list_lps = bm_list_lps; a.in = bm_hdr[0]; a.in_ids = bm_ids[0]; a.in_lps = bm_lps[0];
        a.out = bm_hdr[1]; a.out_ids = bm_ids[1]; a.out_lps = bm_lps[1];
        a.len_cap = len_cap; a.W = W; a.limit = limit; a.n_eos = n_eos; a.B = B; a.n_cp = n_cp; a.set_stride = n_cp;
        a.eos = bm_eos; a.set_pages = bm_sets; a.tok_b = bm_tok; a.pair_src = bm_pair_src; a.pair_dst = bm_pair_dst; a.rec = bm_rec;
        launch_beam_select(st, a);
        sync();
        LAUNCH_CHECK("op_beam_select");
        BeamHdr ho;
        HIP_CHECK(hipMemcpy(&ho, bm_hdr[1], sizeof(BeamHdr), hipMemcpyDeviceToHost));
        hdr_out[0] = ho.n;
        for (int r = 0; r < BEAM_MAX_W; ++r) {
            hdr_out[1 + r] = ho.len[r]; hdr_out[1 + BEAM_MAX_W + r] = ho.fin[r]; hdr_out[1 + 2 * BEAM_MAX_W + r] = ho.set_of[r]; score_out[r] = ho.score[r];
        }
        HIP_CHECK(hipMemcpy(ids_out, bm_ids[1], rows * sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(lps_out, bm_lps[1], rows * sizeof(float), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(tok_b, bm_tok, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        if (n_cp) {
            HIP_CHECK(hipMemcpy(pair_src, bm_pair_src, (size_t)BEAM_MAX_W * n_cp * sizeof(int), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(pair_dst, bm_pair_dst, (size_t)BEAM_MAX_W * n_cp * sizeof(int), hipMemcpyDeviceToHost));
        }
        HIP_CHECK(hipMemcpy(rec, bm_rec, BEAM_REC * sizeof(int), hipMemcpyDeviceToHost));
    }
    void kv_read(const LLayer& L, int env, int start, int n, float* k_out, float* v_out) {
        REQUIRE(k_out && v_out, "null output pointer");
        const int limit = env < 0 ? pages_total * PAGE : env_at(env).n_pages * PAGE;
        REQUIRE(start >= 0 && n >= 0 && start + n <= limit, "op_kv_read: positions outside the env's pages");
        const size_t page_elems = (size_t)nkv * PAGE * 128;
        std::vector<T> kp(page_elems), vp(page_elems);
        sync();
        for (int pg = start / PAGE; pg * PAGE < start + n; ++pg) {
            const int phys = env < 0 ? pg : envs[env].pages[pg];
            HIP_CHECK(hipMemcpy(kp.data(), L.kpool + (size_t)phys * page_elems, page_elems * sizeof(T), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(vp.data(), L.vpool + (size_t)phys * page_elems, page_elems * sizeof(T), hipMemcpyDeviceToHost));
            for (int off = 0; off < PAGE; ++off) {
                const int p = pg * PAGE + off;
                if (p < start || p >= start + n) continue;
                for (int kh = 0; kh < nkv; ++kh)
                    for (int d = 0; d < 128; ++d) {
                        const size_t o = ((size_t)(p - start) * nkv + kh) * 128 + d;
                        k_out[o] = host_to_f32(kp[((size_t)kh * PAGE + off) * 128 + d]);
                        v_out[o] = host_to_f32(vp[((size_t)kh * 128 + d) * PAGE + off]);
                    }
            }
        }
    }
    // the prefill q|k|v product of one env's turn on layer 0 (env 0, positions P .. P + T - 1) through prefill_qkv / prefill_rope_append,
    // as prefill_rows runs it: x = the normed input rows [T][hidden]; the roped q rows -> q_out, k / v in the env's pages;
    // *fused = 1 when the product's split-K reduce did the RoPE + append, 0 when launch_rope_kv did
    void op_llm_qkv_rope(const void* xin, int Tn, int P, void* q_out, int q_stride, int32_t* fused) override {
        REQUIRE(xin && q_out && fused, "null pointer");
        REQUIRE(Tn >= 1 && P >= 0 && P + Tn <= c.max_positions, "positions out of range");
        REQUIRE(q_stride >= nq * 128, "q_stride");
        Env& e = env_at(0);
        op_env_begin(0, P + Tn);
        const LLayer& L = ll[0];
        HIP_CHECK(hipMemcpyAsync(xn, xin, (size_t)Tn * H * sizeof(T), hipMemcpyDeviceToDevice, st));
        const Seg g{&e, P, Tn, 0};
        const bool roped = prefill_qkv(L, Tn, &g);
        if (!roped) prefill_rope_append(L, g);
        HIP_CHECK(hipMemcpy2DAsync(q_out, (size_t)q_stride * sizeof(T), qkv, (size_t)qkv_dim * sizeof(T), (size_t)nq * 128 * sizeof(T), Tn,
                                   hipMemcpyDeviceToDevice, st));
        sync();
        LAUNCH_CHECK("op_llm_qkv_rope");
        *fused = roped ? 1 : 0;
    }
    // TEST-ONLY: launch_rope_kv on caller rows [Tn][ld] (q|k|v, q roped in place) at positions P .. of env 0 on the layer-0 pools, through
    // the pages svln_op_set_pages fixed for it, with the mirror list of the folded candidates call: mirror_page = (P + Tn) / 64, the
    // page a fork's branch would open.  n_mirror == 0 is the plain launch.  Every refusal comes before the env is reset or a launch is made.
    void op_rope_kv_mirror(void* rows, int ld, int Tn, int P, const int32_t* mirror_pages, int n_mirror) override {
        const char* who = "svln_op_rope_kv_mirror";
        REQUIRE(rows && ld >= qkv_dim, std::string(who) + ": null rows / a row pitch below (q_heads + 2 kv_heads) * 128");
        REQUIRE(n_mirror >= 0 && n_mirror <= ROPE_MIRROR_MAX && (n_mirror == 0 || mirror_pages), std::string(who) + ": n_mirror must be 0 .. 7");
        REQUIRE(Tn >= 1 && P >= 0 && (int64_t)P + Tn <= c.max_positions, std::string(who) + ": positions out of range");
        const int L = P + Tn, need = (L + PAGE - 1) / PAGE, q0 = L / PAGE;
        REQUIRE(!op_pages.empty() && !op_pages[0].empty(), std::string(who) + ": fix the pages of env 0 with svln_op_set_pages first");
        const std::vector<int>& want = op_pages[0];
        REQUIRE(need <= (int)want.size() && need <= pages_per_env, std::string(who) + ": positions beyond the env's pages");
        for (int d = 0; d < n_mirror; ++d) {
            const int p = mirror_pages[d];
            REQUIRE(p >= 0 && p < pages_total, std::string(who) + ": a mirror page outside the pool");
            for (int i = 0; i < (int)want.size(); ++i)
                REQUIRE(want[i] != p, std::string(who) + (i == q0 ? ": a mirror page equals the env's page q0" : ": a mirror page is a page of the env"));
            for (int q = 0; q < d; ++q) REQUIRE(mirror_pages[q] != p, std::string(who) + ": a mirror page is listed twice");
        }
        Env& e = env_at(0);
        sync();
        op_env_begin(0, L);
        RopeKvArgs r = rope_kv_args(ll[0], Seg{&e, P, Tn, 0});
        r.qkv = rows; r.ld = ld;
        if (n_mirror > 0) {
            for (int d = 0; d < n_mirror; ++d) h_fork_dst[d] = mirror_pages[d];
            upload_fork_dst(n_mirror);
            r.mirror_page = q0; r.mirror_dst = d_fork_dst; r.n_mirror = n_mirror;
        }
        launch_rope_kv<T>(st, r);
        sync();
        LAUNCH_CHECK("op_rope_kv_mirror");
    }
    void op_rope_append(Env& e, const LLayer& L, void* rows, int ld, int Tn, int P) {
        RopeKvArgs r; r.Kpool = L.kpool; r.Vpool = L.vpool; r.page_table = e.d_pages; r.rope_tab = rope_tab; r.nq = nq; r.nkv = nkv; r.dyn_pos = nullptr;
        r.ld = ld; r.qkv = rows; r.T = Tn; r.P = P;
        launch_rope_kv<T>(st, r);
    }
    // LLM attention on layer-0 pools / env 0: context rows (ctx_T positions from 0) are roped + appended first, then the T new rows
    void op_attention_llm(void* qkv_new, int ld, int Tn, int P, const void* ctx, int ctx_T, void* out, int o_stride, int nsplit) override {
        Env& e = env_at(0);
        REQUIRE(ctx_T == P, "context length must equal P");
        op_env_begin(0, P + Tn);
        const LLayer& L = ll[0];
        if (ctx_T > 0) op_rope_append(e, L, const_cast<void*>(ctx), ld, ctx_T, 0);
        op_rope_append(e, L, qkv_new, ld, Tn, P);
        AttnArgs a = llm_attn_args(L, e, qkv_new, ld, out, o_stride, Tn, P, P + Tn, false);
        if (nsplit > 1) {
            // split-KV with one wave per kv head and key page: attn_kernel<T, 128, 1>, which the engine itself never launches (its decode
            // steps take attn_decode_kernel through decode_attn_args, with fused RoPE + append: op_attention_decode tests that one)
            REQUIRE(Tn * (nq / nkv) <= 32, "split-KV path takes at most 32 rows per kv head");
            a.nsplit = nsplit_max; a.tiles_per_split = tiles_per_split; a.rows_pad = 32;
            launch_attention<T>(st, a, 128, 1);
            launch_attention_combine<T>(st, a, 128);
        } else {                    // prefill: engine heuristic (may split the keys for few row blocks)
            launch_attention<T>(st, a, 128, 4);
            if (a.nsplit > 1) launch_attention_combine<T>(st, a, 128);
        }
        sync();
    }
    // one decode step of B envs on layer 0, through the engine's own decode attention (decode_attn_args / batched_decode_attn_args +
    // decode_attention).  Env b first gets pos[b] context rows (ctx + b * ctx_rows * ld, roped in place + appended like
    // op_attention_llm); then its un-roped q|k|v row qkv_new[b] is decoded at position pos[b] (RoPE, K / V append, attention, merge).
    // B == 1 takes the single-env step (d_ctl), B > 1 the batched step (d_slots).
    void op_attention_decode(int B, const void* ctx, int ld, int64_t ctx_rows, const int32_t* pos, const void* qkv_new, void* out,
                             int o_stride) override {
        REQUIRE(B == 1 || B == 2 || B == 4 || B == 8, "B must be 1, 2, 4 or 8");
        REQUIRE(B <= c.max_envs, "B exceeds max_envs");
        REQUIRE(pos && qkv_new && out, "null pointer");
        REQUIRE(ld >= qkv_dim && o_stride >= nq * 128, "row strides");
        const LLayer& L = ll[0];
        // B == 1 with null context rows and pos > 0: the step runs on env 0 AS THE LAST OP LEFT IT (no reset, nothing re-appended): its
        // pages must already cover the position.  So a step can follow a verify pass and read the rows that pass appended.
        const bool keep = B == 1 && !ctx && pos[0] > 0;
        for (int b = 0; b < B; ++b) {
            REQUIRE(pos[b] >= 0 && pos[b] < c.max_positions && (keep || pos[b] <= ctx_rows), "decode position out of range");
            REQUIRE(pos[b] == 0 || ctx || keep, "null context rows");
            if (!keep) reset_env(b);
        }
        if (keep) REQUIRE(pos[0] < env_at(0).n_pages * PAGE, "null context rows: env 0 holds no page for this position (run the op that fills it first)");
        for (int b = 0; b < B && !keep; ++b) {
            Env& e = env_at(b);
            op_env_begin(b, pos[b] + 1);
            if (pos[b] > 0) op_rope_append(e, L, (char*)const_cast<void*>(ctx) + (size_t)b * ctx_rows * ld * sizeof(T), ld, pos[b], 0);
        }
        HIP_CHECK(hipMemcpy2DAsync(qkv, (size_t)qkv_dim * sizeof(T), qkv_new, (size_t)ld * sizeof(T), (size_t)qkv_dim * sizeof(T), B,
                                   hipMemcpyDeviceToDevice, st));
        if (B == 1) {
            h_ctl->pos = pos[0]; h_ctl->kv_len = pos[0] + 1; h_ctl->done = 0; h_ctl->count = 0; h_ctl->max_new = 0; h_ctl->n_eos = 0;
            h_ctl->draw0 = h_ctl->stream = 0;
            HIP_CHECK(hipMemcpyAsync(d_ctl, h_ctl, sizeof(GenCtl), hipMemcpyHostToDevice, st));
            decode_attention(decode_attn_args(L, env_at(0)));
        } else {
            for (int b = 0; b < B; ++b) { h_slots[b].page_table = envs[b].d_pages; h_slots[b].pos = pos[b]; h_slots[b].pad = 0; }
            HIP_CHECK(hipMemcpyAsync(d_slots, h_slots, B * sizeof(DecodeSlot), hipMemcpyHostToDevice, st));
            decode_attention(batched_decode_attn_args(L, B));
        }
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)o_stride * sizeof(T), attn, (size_t)nq * 128 * sizeof(T), (size_t)nq * 128 * sizeof(T), B,
                                   hipMemcpyDeviceToDevice, st));
        sync();
        LAUNCH_CHECK("op_attention_decode");
    }
    // one verify pass's attention on layer 0 / env 0 through verify_attn_args + launch_attention_verify, as a verify pass runs it: env 0
    // first gets ctx_rows context rows (roped in place + appended like op_attention_llm), then the `rows` un-roped q|k|v rows qkv_new are
    // verified at positions ctx_rows .. ctx_rows + rows - 1 (RoPE per row, K / V append of every row, per-row mask, merge)
    void op_attention_verify(int rows, const void* ctx, int ld, int ctx_rows, const void* qkv_new, void* out, int o_stride) override {
        REQUIRE(rows >= 1 && rows <= MAXB && rows * (nq / nkv) <= 32, "rows must be 1 .. 8 with rows * (q_heads / kv_heads) <= 32");
        REQUIRE(qkv_new && out, "null pointer");
        REQUIRE(ld >= qkv_dim && o_stride >= nq * 128, "row strides");
        REQUIRE(ctx_rows >= 0 && ctx_rows + rows <= c.max_positions, "verify positions out of range");
        REQUIRE(ctx_rows == 0 || ctx, "null context rows");
        set_speculative_buffers();
        const LLayer& L = ll[0];
        Env& e = env_at(0);
        op_env_begin(0, ctx_rows + rows);
        if (ctx_rows > 0) op_rope_append(e, L, const_cast<void*>(ctx), ld, ctx_rows, 0);
        HIP_CHECK(hipMemcpy2DAsync(qkv, (size_t)qkv_dim * sizeof(T), qkv_new, (size_t)ld * sizeof(T), (size_t)qkv_dim * sizeof(T), rows,
                                   hipMemcpyDeviceToDevice, st));
        h_ctl->pos = ctx_rows; h_ctl->kv_len = ctx_rows + 1; h_ctl->done = 0; h_ctl->count = 0; h_ctl->max_new = 0; h_ctl->n_eos = 0;
        h_ctl->draw0 = h_ctl->stream = 0;
        HIP_CHECK(hipMemcpyAsync(d_ctl, h_ctl, sizeof(GenCtl), hipMemcpyHostToDevice, st));
        h_vctl[0] = 0; h_vctl[1] = rows; h_vctl[2] = h_vctl[3] = 0;
        HIP_CHECK(hipMemcpyAsync(d_vctl, h_vctl, 4 * sizeof(int), hipMemcpyHostToDevice, st));
        launch_attention_verify<T>(st, verify_attn_args(L, e, rows));
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)o_stride * sizeof(T), attn, (size_t)nq * 128 * sizeof(T), (size_t)nq * 128 * sizeof(T), rows,
                                   hipMemcpyDeviceToDevice, st));
        sync();
        LAUNCH_CHECK("op_attention_verify");
    }
    // the batched verify attention (verify_multi_attn_args + launch_attention_verify_multi, as a scoring pass of svln_generate_candidates
    // runs it) on layer 0 / envs 0 .. S - 1.  Sequence s: ctx_len[s] context rows (ctx + s * ctx_rows * ld; roped + appended like
    // op_attention_llm), then rows[s] (0 .. T) of its T un-roped q|k|v row slots qkv_new[s * T ..] verified at positions ctx_len[s] ...
    // share != 0: the fork layout -- every ctx_len equals ctx_len[0], only env 0 gets the context, and sequence s >= 1 runs on a table of
    // env 0's pages below q0 = ctx_len / 64 followed by env s's own pages from q0 on (the partly filled page copied by the fork launch);
    // env s's pages below q0 stay unused.  Every refusal comes before the first launch.
    void op_attention_verify_multi(int S, int Tm, const void* ctx, int ld, int ctx_rows, const int32_t* ctx_len, const void* qkv_new,
                                   const int32_t* rows, int share, void* out, int o_stride) override {
        REQUIRE(S >= 1 && S <= MAXB, "svln_op_attention_verify_multi: 1 .. 8 sequences");
        REQUIRE(S <= c.max_envs, "svln_op_attention_verify_multi: more sequences than max_envs");
        REQUIRE(Tm >= 1 && Tm * (nq / nkv) <= 32, "svln_op_attention_verify_multi: T * (q_heads / kv_heads) must be 1 .. 32");
        REQUIRE(ctx_len && rows && qkv_new && out, "null pointer");
        REQUIRE(S * Tm <= c.max_positions, "svln_op_attention_verify_multi: more row slots than the row buffers hold");
        REQUIRE(ld >= qkv_dim && o_stride >= nq * 128, "row strides");
        int q0 = 0;
        for (int s = 0; s < S; ++s) {
            REQUIRE(rows[s] >= 0 && rows[s] <= Tm, "svln_op_attention_verify_multi: a row count outside 0 .. T");
            REQUIRE(ctx_len[s] >= 0 && ctx_len[s] <= ctx_rows && (int64_t)ctx_len[s] + rows[s] <= c.max_positions,
                    "svln_op_attention_verify_multi: a position at or past max_positions (or more context than context rows)");
            REQUIRE(ctx_len[s] == 0 || ctx, "null context rows");
            REQUIRE(!share || ctx_len[s] == ctx_len[0], "svln_op_attention_verify_multi: shared context needs equal context lengths");
            // a page the sequence does not hold: the caller's page list (svln_op_set_pages) must cover every position the pass touches
            const int need = (ctx_len[s] + rows[s] + PAGE - 1) / PAGE;
            if (s < (int)op_pages.size() && !op_pages[s].empty())
                REQUIRE(need <= (int)op_pages[s].size(), "svln_op_attention_verify_multi: a sequence's position lies in a page it does not hold");
        }
        if (share) q0 = ctx_len[0] / PAGE;
        set_speculative_buffers();
        const LLayer& L = ll[0];
        for (int s = 0; s < S; ++s) reset_env(s);
        for (int s = 0; s < S; ++s) {
            Env& e = env_at(s);
            op_env_begin(s, ctx_len[s] + rows[s]);
            if (ctx_len[s] > 0 && (!share || s == 0))
                op_rope_append(e, L, (char*)const_cast<void*>(ctx) + (size_t)s * ctx_rows * ld * sizeof(T), ld, ctx_len[s], 0);
        }
        int n_dst = 0;
        for (int s = 0; s < S; ++s) {
            h_slots[s].pos = ctx_len[s]; h_slots[s].pad = rows[s];
            if (!share || s == 0) { h_slots[s].page_table = envs[s].d_pages; continue; }
            ensure_fork_tab(s);
            std::vector<int>& tab = fork_host[s];
            for (int i = 0; i < q0; ++i) tab[i] = envs[0].pages[i];
            for (int i = q0; i < envs[s].n_pages; ++i) tab[i] = envs[s].pages[i];
            HIP_CHECK(hipMemcpyAsync(fork_tab[s], tab.data(), (size_t)pages_per_env * sizeof(int), hipMemcpyHostToDevice, st));
            h_slots[s].page_table = fork_tab[s];
            if (ctx_len[0] % PAGE != 0 && envs[s].n_pages > q0) h_fork_dst[n_dst++] = envs[s].pages[q0];
        }
        if (n_dst > 0) fork_page_copy(envs[0].pages[q0], n_dst);
        HIP_CHECK(hipMemcpyAsync(d_slots, h_slots, S * sizeof(DecodeSlot), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpy2DAsync(qkv, (size_t)qkv_dim * sizeof(T), qkv_new, (size_t)ld * sizeof(T), (size_t)qkv_dim * sizeof(T), (size_t)S * Tm,
                                   hipMemcpyDeviceToDevice, st));
        // the output rows the launch leaves alone keep the caller's bytes: attn := out first
        HIP_CHECK(hipMemcpy2DAsync(attn, (size_t)nq * 128 * sizeof(T), out, (size_t)o_stride * sizeof(T), (size_t)nq * 128 * sizeof(T), (size_t)S * Tm,
                                   hipMemcpyDeviceToDevice, st));
        int kv_max = 1;
        for (int s = 0; s < S; ++s) kv_max = std::max(kv_max, (int)(ctx_len[s] + rows[s]));
        launch_attention_verify_multi<T>(st, verify_multi_attn_args(L, S, Tm, kv_max));
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)o_stride * sizeof(T), attn, (size_t)nq * 128 * sizeof(T), (size_t)nq * 128 * sizeof(T), (size_t)S * Tm,
                                   hipMemcpyDeviceToDevice, st));
        sync();
        LAUNCH_CHECK("op_attention_verify_multi");
    }
    // one verify-step launch on caller-given row tokens and arg-maxes, from `count` emitted tokens (host arrays)
    void op_verify_step(int rows, const int32_t* fed, const int32_t* cand, int count, int max_new, const int64_t* eos, int n_eos,
                        int32_t* new_count, int32_t* done, int64_t* emitted, int32_t* next_token) override {
        REQUIRE(rows >= 1 && rows <= MAXB, "rows must be 1 .. 8");
        REQUIRE(fed && cand && new_count && done && emitted && next_token, "null pointer");
        REQUIRE(count >= 0 && count + rows <= c.max_positions, "count out of range");
        REQUIRE(n_eos >= 0 && n_eos <= 16 && (n_eos == 0 || eos), "0 .. 16 eos ids");
        set_speculative_buffers();
        sync();
        eos_valid = false;                 // d_eos is rewritten here
        int he[16];
        for (int k = 0; k < n_eos; ++k) he[k] = eos[k] >= 0 && eos[k] < V ? (int)eos[k] : -2;
        if (n_eos) HIP_CHECK(hipMemcpy(d_eos, he, (size_t)n_eos * sizeof(int), hipMemcpyHostToDevice));
        int hv[16] = {0};
        hv[1] = rows;
        for (int i = 0; i < rows; ++i) hv[8 + i] = fed[i];
        HIP_CHECK(hipMemcpy(d_vctl, hv, sizeof(hv), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_tok_b, cand, (size_t)rows * sizeof(int), hipMemcpyHostToDevice));
        const int tok0 = -3;
        HIP_CHECK(hipMemcpy(d_token, &tok0, sizeof(int), hipMemcpyHostToDevice));
        GenCtl g; g.pos = count; g.kv_len = count + 1; g.done = 0; g.count = count; g.max_new = max_new; g.n_eos = n_eos; g.draw0 = g.stream = 0;
        HIP_CHECK(hipMemcpy(d_ctl, &g, sizeof(g), hipMemcpyHostToDevice));
        launch_verify_step<T>(st, d_vctl + 8, d_tok_b, d_vctl + 1, rows, d_ctl, d_eos, d_out_ids, d_token, xn, hid_tap, H, HID_TAP_ROWS, d_vctl + 2);
        sync();
        LAUNCH_CHECK("op_verify_step");
        HIP_CHECK(hipMemcpy(&g, d_ctl, sizeof(g), hipMemcpyDeviceToHost));
        REQUIRE(g.count >= count && g.count <= count + rows, "verify step: count out of range");
        std::vector<int> ids(rows, -3);
        if (g.count > count) HIP_CHECK(hipMemcpy(ids.data(), d_out_ids + count, (size_t)(g.count - count) * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < rows; ++i) emitted[i] = i < g.count - count ? ids[i] : -3;
        int tk = 0;
        HIP_CHECK(hipMemcpy(&tk, d_token, sizeof(int), hipMemcpyDeviceToHost));
        *new_count = g.count; *done = g.done; *next_token = tk;
    }
    // TEST-ONLY: `steps` step-kernel launches back to back on caller-given partial sets (use_ctl = 0: one launch_argmax_final on set 0),
    // on the engine's own d_ctl / d_eos / d_out_ids / d_scores / d_token / d_top2, which are saved before and restored afterwards
    void op_argmax_step(const svln_argmax_step_op& q) override {
        const size_t cap = (size_t)c.max_positions + 8, eos_cap = (size_t)(V > 16 ? V : 16);
        REQUIRE(q.n >= 1 && q.n <= 2048, "op_argmax_step: n must be 1 .. 2048");
        REQUIRE(q.steps >= 1 && q.steps <= 8, "op_argmax_step: steps must be 1 .. 8");
        REQUIRE(q.rows >= 1 && (size_t)q.rows <= cap, "op_argmax_step: rows beyond the id buffer");
        REQUIRE(q.count >= 0 && q.count + q.steps <= q.rows, "op_argmax_step: count leaves no room in out_ids");
        REQUIRE(q.n_eos >= 0 && (size_t)q.n_eos <= eos_cap && (q.n_eos == 0 || q.eos), "op_argmax_step: eos list");
        REQUIRE(q.part_val && q.part_idx && q.ctl_out && q.out_ids && q.last_token && q.out_top && q.scores, "op_argmax_step: null pointer");
        REQUIRE((q.part_raw != nullptr) == (q.part_max != nullptr) && (!q.part_raw || q.part_sum), "op_argmax_step: part_raw / part_max come together, with part_sum");
        REQUIRE(q.flag_bytes >= 0 && q.flag_bytes <= (1 << 24) && (q.flag_bytes == 0 || q.flags), "op_argmax_step: flag array");
        const size_t np = (size_t)q.steps * q.n;
        if (q.flag_bytes)
            for (size_t k = 0; k < np; ++k)
                REQUIRE(q.part_idx[k] == 0x7FFFFFFF || (q.part_idx[k] >= 0 && q.part_idx[k] < q.flag_bytes), "op_argmax_step: a part_idx outside the flag array");
        sync();
        eos_valid = false;                 // d_eos is rewritten here
        std::vector<int> he(q.n_eos);
        for (int k = 0; k < q.n_eos; ++k) he[k] = q.eos[k] >= 0 && q.eos[k] < 0x7FFFFFFF ? (int)q.eos[k] : -2;
        // the engine's own state, restored at the end
        GenCtl g0; int tok0[4]; float top0[4];
        std::vector<int> ids0(q.rows); std::vector<float> sc0(q.rows);
        HIP_CHECK(hipMemcpy(&g0, d_ctl, sizeof(g0), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(tok0, d_token, sizeof(tok0), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(top0, d_top2, sizeof(top0), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ids0.data(), d_out_ids, ids0.size() * sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(sc0.data(), d_scores, sc0.size() * sizeof(float), hipMemcpyDeviceToHost));
        float *pv = nullptr, *ps = nullptr, *pr = nullptr, *pm = nullptr; int* pi = nullptr; uint8_t* fl = nullptr;
        auto up = [&](auto*& dst, const void* src, size_t bytes) {
            HIP_CHECK(hipMalloc((void**)&dst, bytes));
            HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        };
        auto cleanup = [&] {
            for (void* p : {(void*)pv, (void*)ps, (void*)pr, (void*)pm, (void*)pi, (void*)fl}) if (p) (void)hipFree(p);
        };
        try {
            up(pv, q.part_val, np * 4); up(pi, q.part_idx, np * 4);
            if (q.part_sum) up(ps, q.part_sum, np * 4);
            if (q.part_raw) { up(pr, q.part_raw, np * 4); up(pm, q.part_max, np * 4); }
            if (q.flag_bytes) { HIP_CHECK(hipMalloc((void**)&fl, (size_t)q.flag_bytes)); HIP_CHECK(hipMemset(fl, 0x5A, (size_t)q.flag_bytes)); }
            if (q.n_eos) HIP_CHECK(hipMemcpy(d_eos, he.data(), (size_t)q.n_eos * sizeof(int), hipMemcpyHostToDevice));
            const float nanv = __builtin_nanf("");
            std::vector<int> ids(q.rows, -7); std::vector<float> sc(q.rows, nanv);
            const int tk[4] = {-7, -7, -7, -7}; const float tp[4] = {nanv, nanv, nanv, nanv};
            HIP_CHECK(hipMemcpy(d_out_ids, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_scores, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_token, tk, sizeof(tk), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_top2, tp, sizeof(tp), hipMemcpyHostToDevice));
            GenCtl g; g.pos = q.pos; g.kv_len = q.kv_len; g.done = q.done; g.count = q.count; g.max_new = q.max_new; g.n_eos = q.n_eos; g.draw0 = g.stream = 0;
            HIP_CHECK(hipMemcpy(d_ctl, &g, sizeof(g), hipMemcpyHostToDevice));
            if (q.use_ctl) {
                for (int s = 0; s < q.steps; ++s) {
                    const size_t o = (size_t)s * q.n;
                    launch_argmax_step(st, pv + o, pi + o, q.n, d_token, d_top2, d_ctl, d_eos, d_out_ids, fl, ps ? ps + o : nullptr, ps ? d_scores : nullptr,
                                       pr ? pr + o : nullptr, pm ? pm + o : nullptr);
                }
            } else {
                launch_argmax_final(st, pv, pi, q.n, d_token, d_top2, ps, ps ? d_scores : nullptr, pr, pm);
            }
            sync();
            LAUNCH_CHECK("op_argmax_step");
            HIP_CHECK(hipMemcpy(&g, d_ctl, sizeof(g), hipMemcpyDeviceToHost));
            static_assert(sizeof(GenCtl) == 8 * sizeof(int), "GenCtl: eight ints");
            std::memcpy(q.ctl_out, &g, sizeof(g));
            HIP_CHECK(hipMemcpy(q.out_ids, d_out_ids, (size_t)q.rows * sizeof(int), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(q.scores, d_scores, (size_t)q.rows * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(q.last_token, d_token, sizeof(int), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(q.out_top, d_top2, 2 * sizeof(float), hipMemcpyDeviceToHost));
            if (q.flag_bytes) HIP_CHECK(hipMemcpy(q.flags, fl, (size_t)q.flag_bytes, hipMemcpyDeviceToHost));
        } catch (...) {
            cleanup();
            throw;
        }
        cleanup();
        HIP_CHECK(hipMemcpy(d_ctl, &g0, sizeof(g0), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_token, tok0, sizeof(tok0), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_top2, top0, sizeof(top0), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_out_ids, ids0.data(), ids0.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_scores, sc0.data(), sc0.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // TEST-ONLY: one draft_select_kernel launch on caller-given host arrays, on the engine's own d_ctl / d_out_ids / d_scores / d_token, which
    // are saved before and restored afterwards.  Final-norm row q holds q + 1 + (column % 4) / 4, the tap rows start at -1.
    void op_draft_select(const svln_draft_select_op& q) override {
        const size_t cap = (size_t)c.max_positions + 8, eos_cap = (size_t)(V > 16 ? V : 16);
        REQUIRE(q.G >= 1 && q.G <= DRAFTS_MAX, "op_draft_select: G must be 1 .. 8");
        REQUIRE(q.r >= 1 && 1 + q.G * q.r <= DRAFT_SELECT_ROWS, "op_draft_select: 1 + G r head rows must be <= 33");
        REQUIRE(q.k && q.fed && q.cand && q.ctl_out && q.out_ids && q.last_token && q.rec && q.stats, "op_draft_select: null pointer");
        REQUIRE(!q.cand_score == !q.scores, "op_draft_select: cand_score and scores come together");
        for (int g = 0; g < q.G; ++g) REQUIRE(q.k[g] >= 0 && q.k[g] <= q.r, "op_draft_select: a row count (k) outside 0 .. r");
        REQUIRE(q.rows >= 1 && (size_t)q.rows <= cap, "op_draft_select: rows beyond the id buffer");
        REQUIRE(q.count >= 0 && q.count + q.r + 1 <= q.rows, "op_draft_select: count leaves no room in out_ids");
        REQUIRE(q.n_eos >= 0 && (size_t)q.n_eos <= eos_cap && (q.n_eos == 0 || q.eos), "op_draft_select: eos list");
        REQUIRE(q.tap_rows >= 0 && q.tap_rows <= HID_TAP_ROWS && (q.tap_rows == 0 || q.taps), "op_draft_select: tap rows");
        ensure_bforced_buffers();
        ensure_cand_buffers();
        ensure_dsel_buffers();
        sync();
        eos_valid = false;                 // d_eos is rewritten here
        int nh = 1;
        for (int g = 0; g < q.G; ++g) nh += q.k[g];
        std::vector<int> he(q.n_eos);
        for (int k = 0; k < q.n_eos; ++k) he[k] = q.eos[k] >= 0 && q.eos[k] < 0x7FFFFFFF ? (int)q.eos[k] : -2;
        // the engine's own state, restored at the end
        GenCtl g0; int tok0 = 0;
        std::vector<int> ids0(q.rows); std::vector<float> sc0(q.rows);
        HIP_CHECK(hipMemcpy(&g0, d_ctl, sizeof(g0), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&tok0, d_token, sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ids0.data(), d_out_ids, ids0.size() * sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(sc0.data(), d_scores, sc0.size() * sizeof(float), hipMemcpyDeviceToHost));
        auto restore = [&] {
            (void)hipMemcpy(d_ctl, &g0, sizeof(g0), hipMemcpyHostToDevice);
            (void)hipMemcpy(d_token, &tok0, sizeof(int), hipMemcpyHostToDevice);
            (void)hipMemcpy(d_out_ids, ids0.data(), ids0.size() * sizeof(int), hipMemcpyHostToDevice);
            (void)hipMemcpy(d_scores, sc0.data(), sc0.size() * sizeof(float), hipMemcpyHostToDevice);
        };
        try {
            if (q.n_eos) HIP_CHECK(hipMemcpy(d_eos, he.data(), (size_t)q.n_eos * sizeof(int), hipMemcpyHostToDevice));
            const float nanv = __builtin_nanf("");
            std::vector<int> ids(q.rows, -7); std::vector<float> sc(q.rows, nanv);
            const int tk = -7;
            HIP_CHECK(hipMemcpy(d_out_ids, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_scores, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_token, &tk, sizeof(int), hipMemcpyHostToDevice));
            int sel[16] = {0};
            for (int g = 0; g < q.G; ++g) sel[g] = q.k[g];
            for (int j = 0; j < 4; ++j) sel[8 + j] = -7;
            sel[12] = q.stats[0]; sel[13] = q.stats[1];
            HIP_CHECK(hipMemcpy(d_dsel, sel, sizeof(sel), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_cfeed, q.fed, (size_t)q.G * q.r * sizeof(int), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_tok_b, q.cand, (size_t)nh * sizeof(int), hipMemcpyHostToDevice));
            if (q.cand_score) HIP_CHECK(hipMemcpy(d_score_b, q.cand_score, (size_t)nh * sizeof(float), hipMemcpyHostToDevice));
            std::vector<T> rows_x((size_t)DRAFT_SELECT_ROWS * H), rows_t((size_t)HID_TAP_ROWS * H);
            for (int row = 0; row < DRAFT_SELECT_ROWS; ++row)
                for (int col = 0; col < H; ++col) host_from_f32((float)(row + 1) + (float)(col % 4) * 0.25f, rows_x[(size_t)row * H + col]);
            for (size_t j = 0; j < rows_t.size(); ++j) host_from_f32(-1.0f, rows_t[j]);
            HIP_CHECK(hipMemcpy(bf_xn, rows_x.data(), rows_x.size() * sizeof(T), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(hid_tap, rows_t.data(), rows_t.size() * sizeof(T), hipMemcpyHostToDevice));
            GenCtl g; g.pos = q.pos; g.kv_len = q.kv_len; g.done = q.done; g.count = q.count; g.max_new = q.max_new; g.n_eos = q.n_eos; g.draw0 = g.stream = 0;
            HIP_CHECK(hipMemcpy(d_ctl, &g, sizeof(g), hipMemcpyHostToDevice));
            DraftSelectArgs a;
            a.cand = d_tok_b; a.cand_score = q.cand_score ? d_score_b : nullptr; a.fed = d_cfeed; a.k = d_dsel; a.G = q.G; a.r = q.r;
            a.ctl = d_ctl; a.eos = d_eos; a.out_ids = d_out_ids; a.out_token = d_token; a.xn = bf_xn; a.hid_tap = hid_tap; a.H = H;
            a.tap_cap = HID_TAP_ROWS; a.scores = d_scores; a.rec = d_dsel + 8; a.stats = d_dsel + 12;
            launch_draft_select<T>(st, a);
            sync();
            LAUNCH_CHECK("op_draft_select");
            HIP_CHECK(hipMemcpy(&g, d_ctl, sizeof(g), hipMemcpyDeviceToHost));
            std::memcpy(q.ctl_out, &g, sizeof(g));
            HIP_CHECK(hipMemcpy(q.out_ids, d_out_ids, (size_t)q.rows * sizeof(int), hipMemcpyDeviceToHost));
            if (q.scores) HIP_CHECK(hipMemcpy(q.scores, d_scores, (size_t)q.rows * sizeof(float), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(q.last_token, d_token, sizeof(int), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(sel, d_dsel, sizeof(sel), hipMemcpyDeviceToHost));
            for (int j = 0; j < 4; ++j) q.rec[j] = sel[8 + j];
            q.stats[0] = sel[12]; q.stats[1] = sel[13];
            if (q.tap_rows) read_rows_f32(hid_tap, (size_t)q.tap_rows * H, q.taps);
        } catch (...) {
            restore();
            throw;
        }
        restore();
    }
    // TEST-ONLY: one decode step on env 0 with GenCtl.done forced to `done`, every buffer a step may touch compared with a host snapshot
    void op_dead_step(int done, char* report, int report_cap, int32_t* n_changed) override {
        REQUIRE(report && report_cap >= 1 && n_changed, "op_dead_step: null pointer");
        Env& e = env_at(0);
        REQUIRE(e.n_embeds >= 1 && e.kv_len >= 1 && e.n_pages >= 1, "op_dead_step: env 0 holds no prefilled prompt");
        for (int k = 0; k < MAXB; ++k) REQUIRE(!jobs[k].used, "op_dead_step: scheduler turns are in flight");
        REQUIRE(!probe_on, "op_dead_step: the roofline probe is on");
        REQUIRE(spec_rows == 0 && !ride_on, "op_dead_step: the draft modes have their own step");
        sync();
        GenCtl g;
        HIP_CHECK(hipMemcpy(&g, d_ctl, sizeof(g), hipMemcpyDeviceToHost));
        REQUIRE(g.pos >= 0 && g.pos < c.max_positions && g.kv_len == g.pos + 1, "op_dead_step: GenCtl holds no generation");
        REQUIRE(g.count >= 1 && g.count < c.max_positions, "op_dead_step: GenCtl holds no generation");
        if (!done) ensure_pages(e, g.pos + 1);
        g.done = done ? 1 : 0;
        HIP_CHECK(hipMemcpy(d_ctl, &g, sizeof(g), hipMemcpyHostToDevice));
        {   // the id rows behind the generation hold whatever the allocation held: a sentinel, so that a live step's append always shows
            std::vector<int> fill((size_t)c.max_positions + 8 - g.count, -7);
            HIP_CHECK(hipMemcpy(d_out_ids + g.count, fill.data(), fill.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        struct Buf { std::string name; const void* p; size_t bytes; };
        std::vector<Buf> bufs;
        auto add = [&](const std::string& name, const void* p, size_t bytes) { if (p && bytes) bufs.push_back({name, p, bytes}); };
        const size_t rt = (size_t)c.max_positions, rows = rt + 8, pool = (size_t)pages_total * nkv * PAGE * 128 * sizeof(T);
        for (int i = 0; i < c.layers; ++i) { add("kpool." + std::to_string(i), ll[i].kpool, pool); add("vpool." + std::to_string(i), ll[i].vpool, pool); }
        add("attn_part", attn_part, attn_part_elems * sizeof(float));
        add("x", x, rt * H * sizeof(T)); add("qkv", qkv, rt * qkv_dim * sizeof(T)); add("attn", attn, rt * nq * 128 * sizeof(T));
        add("hbuf", hbuf, rt * I * sizeof(T)); add("head_xn", head_xn, (size_t)H * sizeof(T)); add("hid_tap", hid_tap, (size_t)HID_TAP_ROWS * H * sizeof(T));
        add("part_val", part_val, 2048 * 4); add("part_idx", part_idx, 2048 * 4); add("part_sum", part_sum, 2048 * 4);
        add("part_raw", part_raw, 2048 * 4); add("part_max", part_max, 2048 * 4); add("part_ent", part_ent, 2048 * 4);
        add("cand_val", cand_val, (size_t)2048 * TOPK_C * 4); add("cand_idx", cand_idx, (size_t)2048 * TOPK_C * 4);
        add("tr_val", tr_val, TOPK_C * 4); add("tr_idx", tr_idx, TOPK_C * 4); add("tr_sum", tr_sum, TOPK_C * 4);
        add("tr_raw", tr_raw, TOPK_C * 4); add("tr_max", tr_max, TOPK_C * 4);
        add("d_token", d_token, 4 * sizeof(int)); add("d_out_ids", d_out_ids, rows * sizeof(int)); add("d_scores", d_scores, rows * sizeof(float));
        add("d_topi", d_topi, rows * TOPK_C * sizeof(int)); add("d_topl", d_topl, rows * TOPK_C * sizeof(float));
        add("d_ent", d_ent, rows * sizeof(float)); add("d_alp", d_alp, rows * ALLOW_MAX * sizeof(float));
        add("pen_flags", pen_flags, (size_t)V); add("d_top2", d_top2, 4 * sizeof(float));
        if (dl_seq) {
            const size_t ng[4] = {(size_t)nq * 128, (size_t)H, (size_t)I, (size_t)H};
            for (int k = 0; k < 4; ++k) add("dl_gran." + std::to_string(k), dl_gran[k], ng[k] * sizeof(unsigned long long));
            add("dl_seq", dl_seq, 64 * sizeof(unsigned));
        }
        add("ctl", d_ctl, sizeof(GenCtl));
        std::vector<std::vector<uint8_t>> before(bufs.size());
        for (size_t b = 0; b < bufs.size(); ++b) {
            before[b].resize(bufs[b].bytes);
            HIP_CHECK(hipMemcpy(before[b].data(), bufs[b].p, bufs[b].bytes, hipMemcpyDeviceToHost));
        }
        decode_steps(e, 0, g.count, 1);
        sync();
        LAUNCH_CHECK("op_dead_step");
        std::string out;
        int changed = 0;
        std::vector<uint8_t> after;
        for (size_t b = 0; b < bufs.size(); ++b) {
            after.resize(bufs[b].bytes);
            HIP_CHECK(hipMemcpy(after.data(), bufs[b].p, bufs[b].bytes, hipMemcpyDeviceToHost));
            long long n = 0, first = -1, last = -1;
            if (std::memcmp(after.data(), before[b].data(), bufs[b].bytes) != 0)
                for (size_t k = 0; k < bufs[b].bytes; ++k)
                    if (after[k] != before[b][k]) { if (first < 0) first = (long long)k; last = (long long)k; ++n; }
            changed += n != 0;
            out += bufs[b].name + " " + std::to_string(bufs[b].bytes) + " " + std::to_string(n) + " " + std::to_string(first) + " " + std::to_string(last) + "\n";
        }
        REQUIRE(out.size() + 1 <= (size_t)report_cap, "op_dead_step: the report does not fit");
        std::memcpy(report, out.c_str(), out.size() + 1);
        *n_changed = changed;
    }
    void op_attention_vit(const void* qkv_buf, int ld, int F, void* out, int o_stride) override {
        REQUIRE(F >= 1 && F <= c.max_frames, "frames");
        vit_attention(qkv_buf, ld, F, out, o_stride); sync();
    }
    // ViT layer `layer`'s q|k|v product + attention through vit_qkv_attention, as run_vit runs it, on caller buffers: x [F*S][Hv] (the
    // normed rows), qkv_out [F*S][3 Hv], attn_out [F*S][o_stride]; *packer = the writer of the K / V^T pages (0 = launch_vit_kv_pack,
    // 1 = the split-K reduce, 2 = the tile epilogue).  force_split > 1: the product takes that many K splits (GemmArgs::force_split; the
    // reduce's fused pack is reached this way where no real shape of the dtype takes it), 0 = the engine's choice
    void op_vit_qkv_attention(int layer, const void* x, int F, void* qkv_out, void* attn_out, int o_stride, int force_split,
                              int32_t* packer) override {
        REQUIRE(layer >= 0 && layer < c.v_layers, "layer out of range");
        REQUIRE(F >= 1 && F <= c.max_frames, "frames");
        REQUIRE(force_split == 0 || force_split > 1, "force_split: 0 or > 1");
        REQUIRE(x && qkv_out && attn_out && packer, "null pointer");
        REQUIRE(o_stride >= Hv, "o_stride");
        const int pk = vit_qkv_attention(vl[layer], (const T*)x, F, (T*)qkv_out, (T*)attn_out, o_stride, force_split);
        sync();
        LAUNCH_CHECK("op_vit_qkv_attention");
        *packer = pk;
    }
    // ViT K / V^T pools := pool_value (rounded to the engine dtype), split-KV partials := NaN (part_nan): see op_fill_attn_state
    void op_fill_vit_state(float pool_value, int part_nan) override {
        REQUIRE(std::isfinite(pool_value), "the pool value must be finite");
        const size_t pages = (size_t)vtiles * c.max_frames * vheads, nk = pages * PAGE * vhdp, nv = pages * vvrows * PAGE;
        T v; host_from_f32(pool_value, v);
        std::vector<T> h(nk > nv ? nk : nv, v);
        sync();
        HIP_CHECK(hipMemcpy(vkpool, h.data(), nk * sizeof(T), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(vvpool, h.data(), nv * sizeof(T), hipMemcpyHostToDevice));
        if (part_nan) HIP_CHECK(hipMemsetAsync(attn_part, 0xff, attn_part_elems * sizeof(float), st));
        sync();
    }
    // the raw ViT pools over the whole allocation (vtiles * max_frames * heads pages) -> fp32 k_out [page][64][HDP], v_out [page][VROWS][64]
    void op_vit_kv_read(float* k_out, float* v_out) override {
        REQUIRE(k_out && v_out, "null output pointer");
        const size_t pages = (size_t)vtiles * c.max_frames * vheads, nk = pages * PAGE * vhdp, nv = pages * vvrows * PAGE;
        std::vector<T> h(nk > nv ? nk : nv);
        sync();
        HIP_CHECK(hipMemcpy(h.data(), vkpool, nk * sizeof(T), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nk; ++i) k_out[i] = host_to_f32(h[i]);
        HIP_CHECK(hipMemcpy(h.data(), vvpool, nv * sizeof(T), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nv; ++i) v_out[i] = host_to_f32(h[i]);
    }
    void op_pool(const void* in, void* out, int F) override { launch_pool<T>(st, in, out, tap_idx, tap_w, F, side, oside, H); sync(); }
    void op_patchify(const float* p, void* out, int F) override { launch_patchify<T>(st, p, out, F, c.v_image, c.v_patch, kp); sync(); }
};

}  // namespace svln

// =================================================================================== C ABI
using namespace svln;
struct svln_engine { EngineBase* impl; };

#define API_BEGIN try {
#define API_BEGIN_H try { REQUIRE(h && h->impl, "null engine handle"); DeviceGuard guard_(h->impl->device_id());
#define API_END                                   \
    return 0;                                     \
    }                                             \
    catch (const std::exception& ex) {            \
        g_err = ex.what();                        \
        return -1;                                \
    }

extern "C" {

const char* svln_last_error(void) { return g_err.c_str(); }

int svln_create(const svln_config* cfg, int device, svln_engine** out) {
    API_BEGIN
    REQUIRE(cfg && out, "null argument");
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    REQUIRE(n > 0 && device < n, "no such HIP device");
    svln_engine* h = new svln_engine;
    if (cfg->dtype == SVLN_F32) h->impl = new Engine<float>(*cfg, device);
    else h->impl = new Engine<bf16>(*cfg, device);
    *out = h;
    API_END
}
void svln_destroy(svln_engine* h) { if (h) { delete h->impl; delete h; } }       /* ~Engine switches to its device and back */
int svln_sync(svln_engine* h) { API_BEGIN_H h->impl->sync(); API_END }
int svln_synth_tensor(svln_engine* h, const char* name, uint64_t seed_t, float hw, float base) { API_BEGIN_H h->impl->synth_tensor(name, seed_t, hw, base); API_END }
int svln_set_tensor(svln_engine* h, const char* name, const void* data, int dtype, int64_t numel, int on_device) {
    API_BEGIN_H h->impl->set_tensor(name, data, dtype, numel, on_device); API_END
}
int svln_weights_ready(svln_engine* h) { API_BEGIN_H if (h->impl->weights_missing()) return -2; API_END }
int svln_get_tensor_f32(svln_engine* h, const char* name, float* out, int64_t numel) { API_BEGIN_H h->impl->get_tensor_f32(name, out, numel); API_END }
int svln_reset_env(svln_engine* h, int env) { API_BEGIN_H h->impl->reset_env(env); API_END }
int svln_kv_reset(svln_engine* h, int env) { API_BEGIN_H h->impl->kv_reset(env); API_END }
int svln_kv_free_pages(svln_engine* h, int32_t* n) { API_BEGIN_H REQUIRE(n, "null output pointer"); *n = h->impl->kv_free_pages(); API_END }
int svln_env_state(svln_engine* h, int env, int32_t* n_embeds, int32_t* kv_len) { API_BEGIN_H h->impl->env_state(env, n_embeds, kv_len); API_END }
int svln_encode_frames(svln_engine* h, const float* pixels, int n_frames, int on_device) { API_BEGIN_H h->impl->encode_frames(pixels, n_frames, on_device); API_END }
int svln_preprocess_frames(svln_engine* h, const uint8_t* rgb, int n_frames, int height, int width, int on_device, float* out_dev) {
    API_BEGIN_H h->impl->preprocess_frames(rgb, n_frames, height, width, on_device, out_dev, true); API_END
}
int svln_preprocess_frames_enqueue(svln_engine* h, const uint8_t* rgb, int n_frames, int height, int width, int on_device, float* out_dev) {
    API_BEGIN_H h->impl->preprocess_frames(rgb, n_frames, height, width, on_device, out_dev, false); API_END
}
int svln_frame_ring(svln_engine* h, int slots, int height, int width, uint8_t** host_base, int64_t* slot_stride) {
    API_BEGIN_H h->impl->frame_ring(slots, height, width, host_base, slot_stride); API_END
}
int svln_frame_ring_wait(svln_engine* h, int slot) { API_BEGIN_H h->impl->frame_ring_wait(slot); API_END }
int svln_turn(svln_engine* h, const svln_turn_args* a, int64_t* out_ids, int out_cap, int32_t* n_out, int32_t* kv_len) {
    API_BEGIN_H REQUIRE(a, "null argument"); h->impl->turn(*a, out_ids, out_cap, n_out, kv_len); API_END
}
int svln_engine_stream(svln_engine* h, void** stream) { API_BEGIN_H REQUIRE(stream, "null output pointer"); *stream = h->impl->stream_handle(); API_END }
int svln_preprocess_time(svln_engine* h, double* gpu_ms, int64_t* frames, int reset) { API_BEGIN_H h->impl->preprocess_time(gpu_ms, frames, reset); API_END }
int svln_append_turn(svln_engine* h, int env, const int64_t* ids, int n_ids, int n_memory) { API_BEGIN_H h->impl->append_turn(env, ids, n_ids, 0, n_memory); API_END }
int svln_append_turn_at(svln_engine* h, int env, const int64_t* ids, int n_ids, int frame_base, int n_memory) {
    API_BEGIN_H h->impl->append_turn(env, ids, n_ids, frame_base, n_memory); API_END
}
int svln_generate_batch(svln_engine* h, const int32_t* envs, int n_envs, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap,
                        int32_t* n_out) {
    API_BEGIN_H h->impl->generate_batch(envs, n_envs, max_new, eos, n_eos, out, cap, n_out); API_END
}
int svln_batch_submit(svln_engine* h, int env, int max_new_tokens, const int64_t* eos_ids, int n_eos, int32_t* slot) {
    API_BEGIN_H
    REQUIRE(slot, "null slot pointer");
    *slot = h->impl->batch_submit(env, max_new_tokens, eos_ids, n_eos);
    API_END
}
int svln_batch_step(svln_engine* h, int32_t* running, int32_t* finished_slots, int32_t* n_finished) {
    API_BEGIN_H
    REQUIRE(running && finished_slots && n_finished, "null output pointer");
    *running = h->impl->batch_step(finished_slots, n_finished);
    API_END
}
int svln_batch_result(svln_engine* h, int slot, int32_t* env, int64_t* out_ids, int out_cap, int32_t* n_out) {
    API_BEGIN_H h->impl->batch_result(slot, env, out_ids, out_cap, n_out); API_END
}
int svln_batch_cancel(svln_engine* h, int slot) { API_BEGIN_H h->impl->batch_cancel(slot); API_END }
int svln_batch_submit_forced(svln_engine* h, int env, const int64_t* ids, int n, const int64_t* eos_ids, int n_eos, int32_t* slot) {
    API_BEGIN_H
    REQUIRE((eos_ids || n_eos == 0) && n_eos >= 0, "null argument");
    if (!slot) h->impl->batch_forced_check(env, ids, n, eos_ids, n_eos);      // a dry run: nothing is queued
    else *slot = h->impl->batch_submit_forced(env, ids, n, eos_ids, n_eos);
    API_END
}
int svln_batch_forced(svln_engine* h, int slot, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs, int cap, int32_t* n) {
    API_BEGIN_H
    REQUIRE(logprobs && greedy_ids && greedy_logprobs && n && cap >= 0, "null output pointer");
    h->impl->batch_forced(slot, logprobs, greedy_ids, greedy_logprobs, cap, n);
    API_END
}
int svln_batch_forced_stats(svln_engine* h, int64_t* jobs, int64_t* rows_fed, int64_t* head_launches, int reset) {
    API_BEGIN_H h->impl->batch_forced_stats(jobs, rows_fed, head_launches, reset); API_END
}
int svln_set_turn_row_limit(svln_engine* h, int rows) { API_BEGIN_H h->impl->set_turn_row_limit(rows); API_END }
int svln_set_repetition_penalty(svln_engine* h, float penalty) { API_BEGIN_H h->impl->set_repetition_penalty(penalty); API_END }
int svln_get_hidden_batch(svln_engine* h, int slot, float* out, int max_rows, int32_t* n_rows) { API_BEGIN_H h->impl->get_hidden_batch(slot, out, max_rows, n_rows); API_END }
int svln_generate(svln_engine* h, int env, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out) {
    API_BEGIN_H h->impl->generate(env, max_new, eos, n_eos, out, cap, n_out, false); API_END
}
int svln_generate_fixed(svln_engine* h, int env, int n_tokens, int64_t* out) {
    API_BEGIN_H int32_t n = 0; h->impl->generate(env, n_tokens, nullptr, 0, out, n_tokens, &n, true); API_END
}
int svln_get_hidden(svln_engine* h, float* out, int max_rows, int32_t* n_rows) { API_BEGIN_H h->impl->get_hidden(out, max_rows, n_rows); API_END }
int svln_set_layer_taps(svln_engine* h, int enable, int probe_layer) { API_BEGIN_H h->impl->set_layer_taps(enable, probe_layer); API_END }
int svln_get_layer_taps(svln_engine* h, float* out) { API_BEGIN_H REQUIRE(out, "null output pointer"); h->impl->get_layer_taps(out); API_END }
int svln_get_layer_probe(svln_engine* h, int which, float* out, int64_t max_elems, int32_t* n_rows, int32_t* n_cols) {
    API_BEGIN_H REQUIRE(out && n_rows && n_cols, "null output pointer"); h->impl->get_layer_probe(which, out, max_elems, n_rows, n_cols); API_END
}
int svln_get_embeds(svln_engine* h, int env, int start, int n, float* out) { API_BEGIN_H h->impl->get_embeds(env, start, n, out); API_END }
int svln_get_frame_feats(svln_engine* h, int start, int n, float* out) { API_BEGIN_H h->impl->get_feats(start, n, out); API_END }
int svln_get_top2(svln_engine* h, float* out) { API_BEGIN_H h->impl->get_top2(out); API_END }
int svln_set_token_scores(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_token_scores(enable); API_END }
int svln_top_logprobs(svln_engine* h, int k) { API_BEGIN_H h->impl->top_logprobs(k); API_END }
int svln_get_topk(svln_engine* h, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) {
    API_BEGIN_H REQUIRE(ids && logprobs && n_rows && k && cap_rows >= 0, "null output pointer"); h->impl->get_topk(ids, logprobs, cap_rows, n_rows, k); API_END
}
int svln_get_token_scores(svln_engine* h, float* out, int cap, int32_t* n) {
    API_BEGIN_H REQUIRE(out && n && cap >= 0, "null output pointer"); h->impl->get_token_scores(out, cap, n); API_END
}
int svln_batch_scores(svln_engine* h, int slot, float* out, int cap, int32_t* n) {
    API_BEGIN_H REQUIRE(out && n && cap >= 0, "null output pointer"); h->impl->batch_scores(slot, out, cap, n); API_END
}
int svln_generate_batch_scores(svln_engine* h, int index, float* out, int cap, int32_t* n) {
    API_BEGIN_H REQUIRE(out && n && cap >= 0, "null output pointer"); h->impl->generate_batch_scores(index, out, cap, n); API_END
}
// the outputs of svln_op_gemv_argmax_topk beyond token and score (null: the scored / sampled entries)
struct OpTopkOut { int k; float* pv; int32_t* pi; float *ps, *pr, *pm, *cv; int32_t *ci, *top_ids; float* top_lp; int32_t* n_part; };
static int op_gemv_argmax_any(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                              float penalty, int32_t* host_token, float* host_logprob, const OpSample* smp, const OpTopkOut* tk = nullptr,
                              const OpEntOut* en = nullptr) {
    API_BEGIN_H
    REQUIRE(fmt >= 0 && fmt <= 3, "fmt: 0 = engine dtype, 1 = e4m3 + row scales, 2 = MXFP4, 3 = 12-bit packing");
    GemvArgs a; a.W = nullptr; a.ldw = ldw; a.x = x; a.norm_w = nullptr; a.eps = 0.0f; a.bias = nullptr; a.res = nullptr; a.y = nullptr; a.N = N; a.K = K;
    a.epi = EPI_ARGMAX; a.part_val = nullptr; a.part_idx = nullptr; a.w8 = nullptr; a.scale = nullptr; a.skip = nullptr;
    if (fmt == 0) a.W = W;
    else if (fmt == 1) { a.w8 = W; a.scale = (const float*)aux; }
    else if (fmt == 2) { a.w4 = W; a.e8 = (const uint8_t*)aux; }
    else {      // W = the bf16 original, aux = the N packed rows followed by the N row records
        REQUIRE(aux && K >= 0 && N >= 0, "null pointer");
        a.W = W; a.wp = aux; a.prec = (const uint8_t*)aux + (size_t)N * p12_row_bytes(K);
    }
    REQUIRE(W, "null pointer");
    a.pen_flags = (const uint8_t*)pen_flags; a.pen = penalty;
    if (tk) h->impl->op_gemv_topk(a, tk->k, smp, host_token, host_logprob, tk->pv, tk->pi, tk->ps, tk->pr, tk->pm, tk->cv, tk->ci, tk->top_ids, tk->top_lp, tk->n_part);
    else h->impl->op_gemv_scores(a, host_token, host_logprob, smp, en);
    API_END
}
int svln_op_gemv_argmax_scores(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                               float penalty, int32_t* host_token, float* host_logprob) {
    return op_gemv_argmax_any(h, fmt, W, aux, ldw, x, N, K, pen_flags, penalty, host_token, host_logprob, nullptr);
}
int svln_op_gemv_argmax_sample(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                               float penalty, float temperature, uint64_t seed, int32_t stream, int32_t draw, int32_t* host_token, float* host_logprob) {
    const OpSample q{temperature, seed, &stream, &draw};
    return op_gemv_argmax_any(h, fmt, W, aux, ldw, x, N, K, pen_flags, penalty, host_token, host_logprob, &q);
}
int svln_op_gemv_argmax_topk(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                             float penalty, int k, int sampled, float temperature, uint64_t seed, int32_t stream, int32_t draw, int32_t* host_token,
                             float* host_logprob, float* part_val, int32_t* part_idx, float* part_sum, float* part_raw, float* part_max,
                             float* cand_val, int32_t* cand_idx, int32_t* top_ids, float* top_logprobs, int32_t* n_part) {
    const OpSample q{temperature, seed, &stream, &draw};
    const OpTopkOut tk{k, part_val, part_idx, part_sum, part_raw, part_max, cand_val, cand_idx, top_ids, top_logprobs, n_part};
    return op_gemv_argmax_any(h, fmt, W, aux, ldw, x, N, K, pen_flags, penalty, host_token, host_logprob, sampled ? &q : nullptr, &tk);
}
static int op_gemv_batched_argmax_any(svln_engine* h, const void* W, int ldw, const void* x, int ldx, const void* norm_w, float eps, int N, int K, int B,
                                      const void* pen_flags, const int32_t* pen_rows, float penalty, int32_t* host_tokens, float* host_logprobs,
                                      const OpSample* smp, const OpTopkRows* tk = nullptr, const OpEntOut* en = nullptr) {
    API_BEGIN_H
    GemvBatchArgs a; a.W = W; a.ldw = ldw; a.x = x; a.ldx = ldx; a.norm_w = norm_w; a.eps = eps; a.bias = nullptr; a.res = nullptr; a.ldr = 0;
    a.y = nullptr; a.ldy = 0; a.N = N; a.K = K; a.epi = EPI_ARGMAX; a.B = B; a.part_val = nullptr; a.part_idx = nullptr;
    a.pen_flags = (const uint8_t*)pen_flags; a.pen_rows = pen_rows; a.pen = penalty;
    h->impl->op_gemv_batched_scores(a, host_tokens, host_logprobs, smp, tk, en);
    API_END
}
int svln_op_gemv_batched_argmax_scores(svln_engine* h, const void* W, int ldw, const void* x, int ldx, const void* norm_w, float eps, int N, int K, int B,
                                       const void* pen_flags, const int32_t* pen_rows, float penalty, int32_t* host_tokens, float* host_logprobs) {
    return op_gemv_batched_argmax_any(h, W, ldw, x, ldx, norm_w, eps, N, K, B, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, nullptr);
}
int svln_op_gemv_batched_argmax_sample(svln_engine* h, const void* W, int ldw, const void* x, int ldx, const void* norm_w, float eps, int N, int K, int B,
                                       const void* pen_flags, const int32_t* pen_rows, float penalty, float temperature, uint64_t seed,
                                       const int32_t* streams, const int32_t* draws, int32_t* host_tokens, float* host_logprobs) {
    const OpSample q{temperature, seed, streams, draws};
    return op_gemv_batched_argmax_any(h, W, ldw, x, ldx, norm_w, eps, N, K, B, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, &q);
}
static int op_gemm_argmax_any(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                              const int32_t* pen_rows, float penalty, int32_t* host_tokens, float* host_logprobs, const OpSample* smp,
                              const OpTopkRows* tk = nullptr, const OpEntOut* en = nullptr) {
    API_BEGIN_H
    GemmArgs a; std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.epi = EPI_ARGMAX; a.nsplit = 1;
    a.pen_flags = (const uint8_t*)pen_flags; a.pen_rows = pen_rows; a.pen = penalty;
    h->impl->op_gemm_argmax_scores(a, host_tokens, host_logprobs, smp, tk, en);
    API_END
}
int svln_op_gemm_argmax_scores(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                               const int32_t* pen_rows, float penalty, int32_t* host_tokens, float* host_logprobs) {
    return op_gemm_argmax_any(h, A, lda, W, ldw, M, N, K, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, nullptr);
}
int svln_op_gemm_argmax_sample(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                               const int32_t* pen_rows, float penalty, float temperature, uint64_t seed, const int32_t* streams,
                               const int32_t* draws, int32_t* host_tokens, float* host_logprobs) {
    const OpSample q{temperature, seed, streams, draws};
    return op_gemm_argmax_any(h, A, lda, W, ldw, M, N, K, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, &q);
}
int svln_op_gemv_batched_argmax_topk(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int N, int K, int B, const void* pen_flags,
                                     const int32_t* pen_rows, float penalty, int k, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                                     const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* cand_val, int32_t* cand_idx,
                                     int32_t* top_ids, float* top_logprobs, int32_t* n_part) {
    const OpSample q{temperature, seed, streams, draws};
    const OpTopkRows tk{k, cand_val, cand_idx, top_ids, top_logprobs, n_part};
    return op_gemv_batched_argmax_any(h, W, ldw, x, ldx, nullptr, 0.0f, N, K, B, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, sampled ? &q : nullptr, &tk);
}
int svln_op_gemm_argmax_topk(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                             const int32_t* pen_rows, float penalty, int k, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                             const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* cand_val, int32_t* cand_idx, int32_t* top_ids,
                             float* top_logprobs, int32_t* n_part) {
    const OpSample q{temperature, seed, streams, draws};
    const OpTopkRows tk{k, cand_val, cand_idx, top_ids, top_logprobs, n_part};
    return op_gemm_argmax_any(h, A, lda, W, ldw, M, N, K, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, sampled ? &q : nullptr, &tk);
}
int svln_token_entropy(svln_engine* h, int enable) { API_BEGIN_H h->impl->token_entropy(enable); API_END }
int svln_get_token_entropy(svln_engine* h, float* out, int cap, int32_t* n) {
    API_BEGIN_H REQUIRE(out && n && cap >= 0, "null output pointer"); h->impl->get_token_entropy(out, cap, n); API_END
}
int svln_batch_entropy(svln_engine* h, int slot, float* out, int cap, int32_t* n) {
    API_BEGIN_H REQUIRE(out && n && cap >= 0, "null output pointer"); h->impl->batch_entropy(slot, out, cap, n); API_END
}
int svln_generate_batch_entropy(svln_engine* h, int index, float* out, int cap, int32_t* n) {
    API_BEGIN_H REQUIRE(out && n && cap >= 0, "null output pointer"); h->impl->generate_batch_entropy(index, out, cap, n); API_END
}
int svln_op_gemv_argmax_entropy(svln_engine* h, int fmt, const void* W, const void* aux, int ldw, const void* x, int N, int K, const void* pen_flags,
                                float penalty, int sampled, float temperature, uint64_t seed, int32_t stream, int32_t draw, int32_t* host_token,
                                float* host_logprob, float* host_entropy, float* part_val, int32_t* part_idx, float* part_sum, float* part_raw,
                                float* part_max, float* part_ent, int32_t* n_part) {
    const OpSample q{temperature, seed, &stream, &draw};
    const OpEntOut en{host_entropy, part_val, part_idx, part_sum, part_raw, part_max, part_ent, n_part};
    return op_gemv_argmax_any(h, fmt, W, aux, ldw, x, N, K, pen_flags, penalty, host_token, host_logprob, sampled ? &q : nullptr, nullptr, &en);
}
int svln_op_gemv_batched_argmax_entropy(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int N, int K, int B, const void* pen_flags,
                                        const int32_t* pen_rows, float penalty, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                                        const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* host_entropies, float* part_val,
                                        int32_t* part_idx, float* part_sum, float* part_raw, float* part_max, float* part_ent, int32_t* n_part) {
    const OpSample q{temperature, seed, streams, draws};
    const OpEntOut en{host_entropies, part_val, part_idx, part_sum, part_raw, part_max, part_ent, n_part};
    return op_gemv_batched_argmax_any(h, W, ldw, x, ldx, nullptr, 0.0f, N, K, B, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, sampled ? &q : nullptr, nullptr, &en);
}
int svln_op_gemm_argmax_entropy(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const void* pen_flags,
                                const int32_t* pen_rows, float penalty, int sampled, float temperature, uint64_t seed, const int32_t* streams,
                                const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* host_entropies, float* part_val,
                                int32_t* part_idx, float* part_sum, float* part_raw, float* part_max, float* part_ent, int32_t* n_part) {
    const OpSample q{temperature, seed, streams, draws};
    const OpEntOut en{host_entropies, part_val, part_idx, part_sum, part_raw, part_max, part_ent, n_part};
    return op_gemm_argmax_any(h, A, lda, W, ldw, M, N, K, pen_flags, pen_rows, penalty, host_tokens, host_logprobs, sampled ? &q : nullptr, nullptr, &en);
}
int svln_op_entropy_merge(svln_engine* h, const float* part_val, const int32_t* part_idx, const float* part_sum, const float* part_max,
                          const float* part_ent, int B, int n_part, float* host_entropies) {
    API_BEGIN_H h->impl->op_entropy_merge(part_val, part_idx, part_sum, part_max, part_ent, B, n_part, host_entropies); API_END
}
int svln_batch_topk(svln_engine* h, int slot, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) {
    API_BEGIN_H REQUIRE(ids && logprobs && n_rows && k && cap_rows >= 0, "null output pointer"); h->impl->batch_topk(slot, ids, logprobs, cap_rows, n_rows, k); API_END
}
int svln_generate_batch_topk(svln_engine* h, int index, int32_t* ids, float* logprobs, int cap_rows, int32_t* n_rows, int32_t* k) {
    API_BEGIN_H REQUIRE(ids && logprobs && n_rows && k && cap_rows >= 0, "null output pointer"); h->impl->generate_batch_topk(index, ids, logprobs, cap_rows, n_rows, k); API_END
}
int svln_set_sampling(svln_engine* h, int enable, float temperature, uint64_t seed) { API_BEGIN_H h->impl->set_sampling(enable, temperature, seed); API_END }
int svln_sampling_truncation(svln_engine* h, int32_t top_k, float top_p) { API_BEGIN_H h->impl->sampling_truncation(top_k, top_p); API_END }
int svln_op_truncate(svln_engine* h, const float* cand_val, const int32_t* cand_idx, int B, int n_part, int c, const int32_t* streams,
                     const int32_t* draws, uint64_t seed, float temperature, int32_t top_k, float top_p, float* part_val, int32_t* part_idx,
                     float* part_raw, float* part_max, float* part_sum, int32_t* host_tokens, float* host_logprobs) {
    API_BEGIN_H
    const OpSample q{temperature, seed, streams, draws};
    h->impl->op_truncate(cand_val, cand_idx, B, n_part, c, &q, top_k, top_p, part_val, part_idx, part_raw, part_max, part_sum, host_tokens, host_logprobs);
    API_END
}
int svln_set_allowed_tokens(svln_engine* h, const int64_t* ids, int n) { API_BEGIN_H h->impl->set_allowed_tokens(ids, n); API_END }
int svln_get_allowed_logprobs(svln_engine* h, float* out, int cap_floats, int32_t* n_tokens, int32_t* n_ids) {
    API_BEGIN_H REQUIRE(out && n_tokens && n_ids && cap_floats >= 0, "null output pointer"); h->impl->get_allowed_logprobs(out, cap_floats, n_tokens, n_ids); API_END
}
int svln_batch_allowed_logprobs(svln_engine* h, int slot, float* out, int cap_floats, int32_t* n_tokens, int32_t* n_ids) {
    API_BEGIN_H REQUIRE(out && n_tokens && n_ids && cap_floats >= 0, "null output pointer"); h->impl->batch_allowed_logprobs(slot, out, cap_floats, n_tokens, n_ids); API_END
}
int svln_generate_batch_allowed_logprobs(svln_engine* h, int index, float* out, int cap_floats, int32_t* n_tokens, int32_t* n_ids) {
    API_BEGIN_H REQUIRE(out && n_tokens && n_ids && cap_floats >= 0, "null output pointer"); h->impl->generate_batch_allowed_logprobs(index, out, cap_floats, n_tokens, n_ids); API_END
}
int svln_generate_group(svln_engine* h, int env, int n_seq, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out) {
    API_BEGIN_H h->impl->generate_group(env, n_seq, max_new, eos, n_eos, out, cap, n_out); API_END
}
int svln_generate_beams(svln_engine* h, int env, int n_beams, int max_new, const int64_t* eos, int n_eos, int64_t* out, int cap, int32_t* n_out, float* scores) {
    API_BEGIN_H h->impl->generate_beams(env, n_beams, max_new, eos, n_eos, out, cap, n_out, scores); API_END
}
int svln_turn_beams(svln_engine* h, const svln_turn_args* a, int n_beams, int64_t* out_ids, int out_cap, int32_t* n_out, float* scores) {
    API_BEGIN_H REQUIRE(a, "null argument"); h->impl->turn_beams(*a, n_beams, out_ids, out_cap, n_out, scores); API_END
}
int svln_beam_trace(svln_engine* h, int cap_steps, int32_t* n_steps, int32_t* width, int32_t* list_ids, float* list_lps, int32_t* records) {
    API_BEGIN_H REQUIRE(cap_steps >= 0 && n_steps && width && list_ids && list_lps && records, "null output pointer");
    h->impl->beam_trace(cap_steps, n_steps, width, list_ids, list_lps, records); API_END
}
int svln_turn_group(svln_engine* h, const svln_turn_args* a, int n_seq, int64_t* out_ids, int out_cap, int32_t* n_out) {
    API_BEGIN_H REQUIRE(a, "null argument"); h->impl->turn_group(*a, n_seq, out_ids, out_cap, n_out); API_END
}
int svln_generate_forced(svln_engine* h, int env, const int64_t* ids, int n, const int64_t* eos_ids, int n_eos, float* logprobs, int64_t* greedy_ids,
                         float* greedy_logprobs, int32_t* kv_len) {
    API_BEGIN_H h->impl->generate_forced(env, ids, n, eos_ids, n_eos, logprobs, greedy_ids, greedy_logprobs, kv_len); API_END
}
int svln_generate_candidates(svln_engine* h, int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos_ids, int n_eos,
                             float* logprobs, int64_t* greedy_ids, float* greedy_logprobs) {
    API_BEGIN_H h->impl->generate_candidates(env, n_seq, ids, lens, eos_ids, n_eos, logprobs, greedy_ids, greedy_logprobs); API_END
}
int svln_turn_candidates(svln_engine* h, const svln_turn_args* a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs,
                         int64_t* greedy_ids, float* greedy_logprobs) {
    API_BEGIN_H REQUIRE(a, "null turn args"); h->impl->turn_candidates(*a, n_seq, ids, lens, logprobs, greedy_ids, greedy_logprobs); API_END
}
int svln_generate_candidates_folded(svln_engine* h, int env, int n_seq, const int64_t* ids, const int32_t* lens, const int64_t* eos_ids,
                                    int n_eos, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs) {
    API_BEGIN_H h->impl->generate_candidates_folded(env, n_seq, ids, lens, eos_ids, n_eos, logprobs, greedy_ids, greedy_logprobs); API_END
}
int svln_turn_candidates_folded(svln_engine* h, const svln_turn_args* a, int n_seq, const int64_t* ids, const int32_t* lens, float* logprobs,
                                int64_t* greedy_ids, float* greedy_logprobs) {
    API_BEGIN_H REQUIRE(a, "null turn args"); h->impl->turn_candidates_folded(*a, n_seq, ids, lens, logprobs, greedy_ids, greedy_logprobs); API_END
}
int svln_op_rope_kv_mirror(svln_engine* h, void* rows, int ld, int T, int P, const int32_t* mirror_pages, int n_mirror) {
    API_BEGIN_H h->impl->op_rope_kv_mirror(rows, ld, T, P, mirror_pages, n_mirror); API_END
}
int svln_turn_forced(svln_engine* h, const svln_turn_args* a, const int64_t* ids, int n, float* logprobs, int64_t* greedy_ids, float* greedy_logprobs,
                     int32_t* kv_len) {
    API_BEGIN_H REQUIRE(a, "null argument"); h->impl->turn_forced(*a, ids, n, logprobs, greedy_ids, greedy_logprobs, kv_len); API_END
}
int svln_op_gemv_batched_target(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int N, int K, int B, const int32_t* targets, float inv_t,
                                int32_t* host_tokens, float* host_greedy_logprobs, float* host_logprobs, float* host_slots) {
    API_BEGIN_H
    GemvBatchArgs a; a.W = W; a.ldw = ldw; a.x = x; a.ldx = ldx; a.norm_w = nullptr; a.eps = 0.0f; a.bias = nullptr; a.res = nullptr; a.ldr = 0;
    a.y = nullptr; a.ldy = 0; a.N = N; a.K = K; a.epi = EPI_TARGET; a.B = B; a.part_val = nullptr; a.part_idx = nullptr;
    h->impl->op_gemv_batched_target(a, targets, inv_t, host_tokens, host_greedy_logprobs, host_logprobs, host_slots);
    API_END
}
int svln_op_gemm_target(svln_engine* h, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const int32_t* targets, float inv_t,
                        int32_t* host_tokens, float* host_greedy_logprobs, float* host_logprobs, float* host_slots) {
    API_BEGIN_H
    GemmArgs a; std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.epi = EPI_ARGMAX; a.nsplit = 1; a.pen = 1.0f; a.smp.inv_t = 1.0f; a.tg.inv_t = 1.0f;
    h->impl->op_gemm_target(a, targets, inv_t, host_tokens, host_greedy_logprobs, host_logprobs, host_slots);
    API_END
}
int svln_op_read_argmax_partials(svln_engine* h, int rows, int n, float* val, int32_t* idx, float* sum) {
    API_BEGIN_H h->impl->op_read_argmax_partials(rows, n, val, idx, sum); API_END
}
int svln_group_select(svln_engine* h, int env, int index, int32_t* kv_len_out) { API_BEGIN_H h->impl->group_select(env, index, kv_len_out); API_END }
int svln_group_logprobs(svln_engine* h, int index, float* out, int cap, int32_t* n) {
    API_BEGIN_H REQUIRE(out && n && cap >= 0, "null output pointer"); h->impl->group_logprobs(index, out, cap, n); API_END
}
int svln_group_dist(svln_engine* h, int index, float* out, int cap_rows, int32_t* n_rows, int32_t* n_cols) {
    API_BEGIN_H REQUIRE(out && n_rows && n_cols && cap_rows >= 0, "null output pointer"); h->impl->group_dist(index, out, cap_rows, n_rows, n_cols); API_END
}
int svln_get_hidden_group(svln_engine* h, int index, float* out, int max_rows, int32_t* n_rows) {
    API_BEGIN_H REQUIRE(out && n_rows, "null output pointer"); h->impl->get_hidden_group(index, out, max_rows, n_rows); API_END
}
int svln_op_kv_page_copy(svln_engine* h, int src_page, const int32_t* dst_pages, int n_dst) { API_BEGIN_H h->impl->op_kv_page_copy(src_page, dst_pages, n_dst); API_END }
int svln_op_beam_page_gather(svln_engine* h, const int32_t* src_pages, const int32_t* dst_pages, int n) { API_BEGIN_H h->impl->op_beam_page_gather(src_pages, dst_pages, n); API_END }
int svln_op_beam_select(svln_engine* h, int W, int limit, int B, int n_cp, int len_cap, const int32_t* eos, int n_eos, const int32_t* list_ids,
                        const float* list_lps, const int32_t* hdr_in, const float* score_in, const int32_t* ids_in, const float* lps_in,
                        const int32_t* set_pages, int32_t* hdr_out, float* score_out, int32_t* ids_out, float* lps_out, int32_t* tok_b,
                        int32_t* pair_src, int32_t* pair_dst, int32_t* rec) {
    API_BEGIN_H h->impl->op_beam_select(W, limit, B, n_cp, len_cap, eos, n_eos, list_ids, list_lps, hdr_in, score_in, ids_in, lps_in, set_pages, hdr_out,
                                        score_out, ids_out, lps_out, tok_b, pair_src, pair_dst, rec); API_END
}
int svln_op_kv_pool_read(svln_engine* h, int layer, int start, int n, float* k_out, float* v_out) { API_BEGIN_H h->impl->op_kv_pool_read(layer, start, n, k_out, v_out); API_END }
int svln_op_subset_argmax(svln_engine* h, const void* W, int ldw, const void* x, int ldx, int V, int K, int B, const int64_t* ids, int n,
                          const void* pen_flags, const int32_t* pen_rows, float penalty, float temperature, uint64_t seed, const int32_t* streams,
                          const int32_t* draws, int32_t* host_tokens, float* host_logprobs, float* host_y, float* host_dist) {
    API_BEGIN_H
    GemvSubsetArgs a; a.W = W; a.ldw = ldw; a.x = x; a.ldx = ldx; a.V = V; a.K = K; a.B = B; a.n = n;
    a.pen_flags = (const uint8_t*)pen_flags; a.pen_rows = pen_rows; a.pen = penalty;
    const OpSample q{temperature, seed, streams, draws};
    h->impl->op_subset_argmax(a, ids, q, host_tokens, host_logprobs, host_y, host_dist);
    API_END
}
int svln_op_gumbel(svln_engine* h, uint64_t seed, int32_t stream, int32_t draw, int32_t n0, int32_t count, float* host_out) {
    API_BEGIN_H h->impl->op_gumbel(seed, stream, draw, n0, count, host_out); API_END
}
int svln_set_decode_graph(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_graph(enable); API_END }
int svln_set_decode_persistent(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_decode_persistent(enable); API_END }
int svln_probe_decode_layer(svln_engine* h, int layer, unsigned long long* out, int max_wgs, int32_t* n_wgs) {
    API_BEGIN_H REQUIRE(out && n_wgs, "null output pointer"); h->impl->probe_decode_layer(layer, out, max_wgs, n_wgs); API_END
}
int svln_set_fp8_decode(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_fp8_decode(enable); API_END }
int svln_set_fp8_gemm(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_fp8_gemm(enable); API_END }
int svln_set_fp8_scaled_mfma(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_fp8_scaled_mfma(enable); API_END }
int svln_set_mxfp4_decode(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_mxfp4_decode(enable); API_END }
int svln_set_packed_decode(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_packed_decode(enable); API_END }
int svln_packed_stats(svln_engine* h, int64_t* packed_bytes, int64_t* bf16_bytes, int64_t* blocks, int64_t* fallback_blocks) {
    API_BEGIN_H
    REQUIRE(packed_bytes && bf16_bytes && blocks && fallback_blocks, "null output pointer");
    h->impl->packed_stats(packed_bytes, bf16_bytes, blocks, fallback_blocks);
    API_END
}
int svln_op_pack_rows(svln_engine* h, const void* w_bf16, int ldw, int64_t rows, int cols, void* packed, void* records, int64_t* fallback_blocks) {
    API_BEGIN_H h->impl->op_pack_rows(w_bf16, ldw, rows, cols, packed, records, fallback_blocks); API_END
}
int svln_op_unpack_rows(svln_engine* h, const void* packed, const void* records, const void* w_bf16, int ldw, int64_t rows, int cols, void* out) {
    API_BEGIN_H h->impl->op_unpack_rows(packed, records, w_bf16, ldw, rows, cols, out); API_END
}
int svln_op_gemv_packed(svln_engine* h, const void* packed, const void* records, const void* W, int ldw, const void* x, const void* norm_w, float eps,
                        const void* bias, const void* res, void* y, int N, int K, int epi, int32_t* host_token) {
    API_BEGIN_H
    if (!packed || !records || !W) throw std::runtime_error("null pointer (packed blocks, row records and the bf16 original are all needed)");
    GemvArgs a; a.W = W; a.ldw = ldw; a.x = x; a.norm_w = norm_w; a.eps = eps; a.bias = bias; a.res = res; a.y = y; a.N = N; a.K = K; a.epi = epi;
    a.part_val = nullptr; a.part_idx = nullptr; a.w8 = nullptr; a.scale = nullptr; a.skip = nullptr; a.wp = packed; a.prec = records;
    h->impl->op_gemv(a, host_token);
    API_END
}
int svln_set_mxfp4_batched(svln_engine* h, int enable) { API_BEGIN_H h->impl->set_mxfp4_batched(enable); API_END }
int svln_set_speculative(svln_engine* h, int rows) { API_BEGIN_H h->impl->set_speculative(rows); API_END }
int svln_set_draft(svln_engine* h, int env, const int64_t* ids, int n) { API_BEGIN_H h->impl->set_draft(env, ids, n); API_END }
int svln_draft_stats(svln_engine* h, int64_t* verify_passes, int64_t* tokens_from_verify, int64_t* single_steps, int reset) {
    API_BEGIN_H h->impl->draft_stats(verify_passes, tokens_from_verify, single_steps, reset); API_END
}
int svln_set_prefill_draft(svln_engine* h, int on) { API_BEGIN_H h->impl->set_prefill_draft(on); API_END }
int svln_prefill_draft_stats(svln_engine* h, int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int reset) {
    API_BEGIN_H h->impl->prefill_draft_stats(rides, tokens_from_rides, rows_fed, reset); API_END
}
int svln_set_batch_draft(svln_engine* h, int on) { API_BEGIN_H h->impl->set_batch_draft(on); API_END }
int svln_batch_draft_stats(svln_engine* h, int64_t* rides, int64_t* tokens_from_rides, int64_t* rows_fed, int64_t* iterations, int64_t* single_rows,
                           int reset) {
    API_BEGIN_H h->impl->batch_draft_stats(rides, tokens_from_rides, rows_fed, iterations, single_rows, reset); API_END
}
int svln_set_memory_prune(svln_engine* h, int keep_tokens) { API_BEGIN_H h->impl->set_memory_prune(keep_tokens); API_END }
int svln_op_memory_prune(svln_engine* h, const void* mem, int n_rows, int keep, int32_t* out_idx, float* out_score) {
    API_BEGIN_H h->impl->op_memory_prune(mem, n_rows, keep, out_idx, out_score); API_END
}
int svln_probe_reset(svln_engine* h) { API_BEGIN_H h->impl->probe_reset(); API_END }
int svln_probe_read(svln_engine* h, double* ms, int64_t* launches, double* bytes) { API_BEGIN_H h->impl->probe_read(ms, launches, bytes); API_END }
int svln_probe_read_prefill(svln_engine* h, double* ms, int64_t* n, double* rows, double* flops, double* wbytes) {
    API_BEGIN_H h->impl->probe_read_prefill(ms, n, rows, flops, wbytes); API_END
}
int svln_phase_times(svln_engine* h, double* v, double* p, double* d, int reset) { API_BEGIN_H h->impl->phase_times(v, p, d, reset); API_END }
int svln_set_feature_cache(svln_engine* h, int capacity_frames) { API_BEGIN_H h->impl->set_feature_cache(capacity_frames); API_END }
int svln_feature_cache_stats(svln_engine* h, int64_t* hits, int64_t* misses) { API_BEGIN_H h->impl->feature_cache_stats(hits, misses); API_END }

int svln_op_gemm(svln_engine* h, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* res, int ldr,
                 int res_mod, int M, int N, int K, int epi, int force_cfg, int force_split) {
    API_BEGIN_H
    GemmArgs a; std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.bias = bias; a.res = res; a.ldr = ldr; a.res_mod = res_mod;
    a.M = M; a.N = N; a.K = K; a.epi = epi; a.nsplit = 1; a.force_cfg = force_cfg; a.force_split = force_split;
    h->impl->op_gemm(a);
    API_END
}
int svln_op_gemm_norm(svln_engine* h, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* res, int ldr,
                      const void* norm_w, const void* norm_b, void* norm_out, float eps, int M, int N, int K, int force_split, int* fused) {
    API_BEGIN_H
    GemmArgs a; std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.bias = bias; a.res = res; a.ldr = ldr; a.norm_b = norm_b;
    a.M = M; a.N = N; a.K = K; a.epi = EPI_NONE; a.nsplit = 1; a.force_split = force_split; a.norm_w = norm_w; a.norm_out = norm_out; a.norm_eps = eps;
    const bool f = h->impl->op_gemm(a);
    if (fused) *fused = f ? 1 : 0;
    API_END
}
int svln_op_gemm_norm_q8(svln_engine* h, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* res, int ldr,
                         const void* norm_w, void* norm_out, float eps, int M, int N, int K, int force_split, void* q8, float* q8_scale, int* fused) {
    API_BEGIN_H
    GemmArgs a; std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.res = res; a.ldr = ldr;
    a.M = M; a.N = N; a.K = K; a.epi = EPI_NONE; a.nsplit = 1; a.force_split = force_split; a.norm_w = norm_w; a.norm_out = norm_out; a.norm_eps = eps;
    a.norm_q8 = q8; a.norm_q8_scale = q8_scale; a.pen = 1.0f;
    const bool f = h->impl->op_gemm(a);
    if (fused) *fused = f ? 1 : 0;
    API_END
}
int svln_op_decode_layer(svln_engine* h, const svln_decode_layer_op* op) {
    API_BEGIN_H REQUIRE(op, "null argument"); h->impl->op_decode_layer(*op); API_END
}
int svln_decode_layer_supported(int dtype, int H, int I, int qd, int qkv_dim, int cus, int32_t* supported) {
    API_BEGIN
    REQUIRE(supported, "null argument");
    REQUIRE(dtype == SVLN_BF16 || dtype == SVLN_F32, "dtype: SVLN_BF16 or SVLN_F32");
    DecodeLayerArgs a; std::memset(&a, 0, sizeof(a));
    a.H = H; a.I = I; a.qd = qd; a.qkv_dim = qkv_dim;
    *supported = (dtype == SVLN_BF16 ? decode_layer_supported<bf16>(a, cus) : decode_layer_supported<float>(a, cus)) ? 1 : 0;
    API_END
}
int svln_decode_layer_walk(const svln_decode_layer_walk_op* op, const svln_decode_layer_walk_op* next, int wave, int lane,
                           svln_decode_layer_slot* slots, int max_slots, int32_t* n_slots, int64_t* refill) {
    API_BEGIN
    REQUIRE(op && next && slots && n_slots && refill, "null argument");
    static_assert(sizeof(svln_decode_layer_slot) == sizeof(DecodeLayerWalkSlot), "slot layout");
    for (const svln_decode_layer_walk_op* d : {op, next}) {
        REQUIRE(d->elem_size == 2 || d->elem_size == 4, "element size: 2 or 4");
        REQUIRE(d->K >= 1 && d->K <= (1 << 24) && (int64_t)d->K * d->elem_size % 1024 == 0, "rows must be whole KiB");
        REQUIRE(d->nrows >= 0 && d->nrows <= (1 << 16) && d->first >= 0 && d->first <= (1 << 24), "nrows / first out of range");
        const int64_t bpr = (int64_t)d->K * d->elem_size / 1024;
        REQUIRE(d->pair == 0 || (d->pair == 1 && d->nrows % 2 == 0 && bpr <= 15), "pair: 0, or 1 on an even number of whole-row-dealt rows");
    }
    REQUIRE(wave >= 0 && wave < 8 && lane >= 0 && lane < 64, "wave < 8, lane < 64");
    const DecodeLayerWalkOp o{op->elem_size, op->K, op->nrows, op->pair, op->first}, r{next->elem_size, next->K, next->nrows, next->pair, next->first};
    const int ns = decode_layer_walk(o, r, wave, lane, (DecodeLayerWalkSlot*)slots, max_slots, refill);
    REQUIRE(ns > 0, "max_slots too small");
    *n_slots = ns;
    API_END
}
int svln_gemm_plan(const svln_gemm_problem* q, svln_gemm_plan_out* out) {
    API_BEGIN
    REQUIRE(q && out, "null argument");
    REQUIRE(q->dtype == SVLN_BF16 || q->dtype == SVLN_F32, "dtype: SVLN_BF16 or SVLN_F32");
    REQUIRE(q->epi == EPI_NONE || q->epi == EPI_GELU_TANH || q->epi == EPI_GELU_ERF || q->epi == EPI_SWIGLU,
            "epilogue: EPI_NONE, EPI_GELU_TANH, EPI_GELU_ERF or EPI_SWIGLU");
    for (int64_t v : {q->M, q->N, q->K, q->rope_nq, q->rope_nkv, q->rope_T, q->vit_F, q->vit_S, q->vit_heads, q->vit_head_dim, q->force_cfg, q->force_split})
        REQUIRE(v >= INT32_MIN && v <= INT32_MAX, "extent outside int32");
    GemmProblem p;
    p.elt_bytes = q->dtype == SVLN_F32 ? 4 : 2; p.epi = (int)q->epi; p.M = (int)q->M; p.N = (int)q->N; p.K = (int)q->K;
    p.fp8 = q->fp8 != 0; p.fp8_scaled = q->fp8 == 2 || (p.fp8 && (q->force_cfg & GEMM_FORCE_FP8_SCALED)); p.has_ws = q->has_ws != 0; p.ws_elems = (size_t)q->ws_elems; p.has_zeros = q->has_zeros != 0;
    p.norm_out = q->norm_out != 0; p.norm_w = q->norm_w != 0; p.res = q->res != 0;
    p.rope = q->rope != 0; p.rope_nq = (int)q->rope_nq; p.rope_nkv = (int)q->rope_nkv; p.rope_T = (int)q->rope_T;
    p.vitpack = q->vitpack != 0; p.vit_F = (int)q->vit_F; p.vit_S = (int)q->vit_S; p.vit_heads = (int)q->vit_heads; p.vit_head_dim = (int)q->vit_head_dim;
    p.force_cfg = (int)q->force_cfg; p.force_split = (int)q->force_split;
    const GemmPlan g = plan_gemm(p);
    std::memset(out, 0, sizeof(*out));
    out->nt_w = g.nt_w; out->bn_fast = g.bn_fast; out->n_launches = g.n_launches; out->fused = g.fused ? 1 : 0; out->vit_packer = g.vit_packer;
    for (int i = 0; i < g.n_launches; ++i) {
        const GemmLaunch& l = g.launch[i];
        const TileGeom& t = TILE_GEOM[l.tile];
        svln_gemm_launch& o = out->launch[i];
        o.tile = l.tile; o.splitk = l.splitk; o.fp8 = l.fp8 ? (l.scaled ? 2 : 1) : 0; o.ntw = l.ntw; o.vp = l.vp;
        o.tile_base = l.tile_base; o.launch_tiles = l.launch_tiles; o.nsplit = l.nsplit; o.grid = l.wgs;
        o.block = t.threads; o.lds_bytes = t.lds_bytes; o.bm = t.bm; o.bn = t.bn;
        o.reducer = l.reducer; o.reducer_block = l.rblock; o.reduce_too_large = l.reduce_too_large;
        for (int j = 0; j < 3; ++j) o.reducer_grid[j] = (int32_t)l.rgrid[j];
    }
    API_END
}
// the fields of svln_mode_state are the bits of ModeBit, in order, then group_env
static_assert(sizeof(svln_mode_state) == (M_COUNT + 1) * sizeof(int32_t), "svln_mode_state: one int32 per ModeBit, then group_env");
int svln_mode_refusal(int caller, const char* who, const svln_mode_state* state, int no_change, char* message, int cap, int32_t* refused) {
    API_BEGIN
    REQUIRE(state && message && refused && cap >= 1, "svln_mode_refusal: null argument");
    REQUIRE(caller >= 0 && caller < C_COUNT, "svln_mode_refusal: unknown caller");
    const int32_t* f = &state->decode_graph;
    ModeState s;
    for (int b = 0; b < M_COUNT; ++b) s.set((ModeBit)b, f[b] != 0);
    s.group_env = state->group_env;
    const std::string m = mode_refusal((Caller)caller, s, who ? who : CALLER_NAME[caller], no_change != 0);
    REQUIRE((int)m.size() < cap, "svln_mode_refusal: the message does not fit");
    std::memcpy(message, m.c_str(), m.size() + 1);
    *refused = !m.empty();
    API_END
}
int svln_mode_rule_count(int32_t* n_rules, int32_t* n_callers, int32_t* n_bits) {
    API_BEGIN
    REQUIRE(n_rules && n_callers && n_bits, "svln_mode_rule_count: null argument");
    *n_rules = mode_rows::N_RULES; *n_callers = C_COUNT; *n_bits = M_COUNT;
    API_END
}
int svln_mode_rule(int index, svln_mode_rule_out* out) {
    API_BEGIN
    REQUIRE(out, "svln_mode_rule: null argument");
    REQUIRE(index >= 0 && index < mode_rows::N_RULES, "svln_mode_rule: no such rule");
    const ModeRule& r = mode_rows::RULES[index];
    out->caller = r.caller; out->part = r.part; out->bit = r.bit; out->must_be_on = r.must_be_on; out->on_no_change = r.on_no_change;
    out->caller_name = CALLER_NAME[r.caller]; out->what = r.what; out->tail = r.tail;
    API_END
}
int svln_op_gemv(svln_engine* h, const void* W, int ldw, const void* x, const void* norm_w, float eps, const void* bias, const void* res, void* y,
                 int N, int K, int epi, int32_t* host_token) {
    API_BEGIN_H
    GemvArgs a; a.W = W; a.ldw = ldw; a.x = x; a.norm_w = norm_w; a.eps = eps; a.bias = bias; a.res = res; a.y = y; a.N = N; a.K = K; a.epi = epi;
    a.part_val = nullptr; a.part_idx = nullptr; a.w8 = nullptr; a.scale = nullptr; a.skip = nullptr;
    h->impl->op_gemv(a, host_token);
    API_END
}
int svln_op_gemm_fp8(svln_engine* h, const void* A8, const float* a_scale, int lda, const void* W8, const float* w_scale, int ldw, void* C, int ldc,
                     const void* bias, const void* res, int ldr, int M, int N, int K, int epi, int force_cfg, int force_split) {
    API_BEGIN_H
    GemmArgs a; std::memset(&a, 0, sizeof(a));
    a.A = A8; a.lda = lda; a.W = W8; a.ldw = ldw; a.C = C; a.ldc = ldc; a.bias = bias; a.res = res; a.ldr = ldr; a.a_scale = a_scale; a.w_scale = w_scale;
    a.M = M; a.N = N; a.K = K; a.epi = epi; a.nsplit = 1; a.force_cfg = force_cfg; a.force_split = force_split;
    h->impl->op_gemm_fp8(a);
    API_END
}
int svln_op_gemv_batched(svln_engine* h, const void* W, int ldw, const void* x, int ldx, const void* norm_w, float eps, const void* bias,
                         const void* res, int ldr, void* y, int ldy, int N, int K, int epi, int B, int32_t* host_tokens) {
    API_BEGIN_H
    GemvBatchArgs a; a.W = W; a.ldw = ldw; a.x = x; a.ldx = ldx; a.norm_w = norm_w; a.eps = eps; a.bias = bias; a.res = res; a.ldr = ldr;
    a.y = y; a.ldy = ldy; a.N = N; a.K = K; a.epi = epi; a.B = B; a.part_val = nullptr; a.part_idx = nullptr;
    h->impl->op_gemv_batched(a, host_tokens);
    API_END
}
int svln_op_quant_fp8(svln_engine* h, const void* w_bf16, int64_t rows, int cols, void* w8, float* scale) {
    API_BEGIN_H h->impl->op_quant_fp8(w_bf16, rows, cols, w8, scale); API_END
}
int svln_op_gemv_fp8(svln_engine* h, const void* w8, const float* scale, int ldw, const void* x, const void* norm_w, float eps, const void* bias,
                     const void* res, void* y, int N, int K, int epi, int32_t* host_token) {
    API_BEGIN_H
    if (K % 16 != 0) throw std::runtime_error("K must be a multiple of 16");
    GemvArgs a; a.W = nullptr; a.ldw = ldw; a.x = x; a.norm_w = norm_w; a.eps = eps; a.bias = bias; a.res = res; a.y = y; a.N = N; a.K = K; a.epi = epi;
    a.part_val = nullptr; a.part_idx = nullptr; a.w8 = w8; a.scale = scale; a.skip = nullptr;
    h->impl->op_gemv(a, host_token);
    API_END
}
int svln_op_quant_mxfp4(svln_engine* h, const void* w_bf16, int64_t rows, int cols, void* q4, void* e8) {
    API_BEGIN_H h->impl->op_quant_mxfp4(w_bf16, rows, cols, q4, (uint8_t*)e8); API_END
}
int svln_op_gemv_mxfp4(svln_engine* h, const void* q4, const void* e8, int ldw, const void* x, const void* norm_w, float eps, const void* bias,
                       const void* res, void* y, int N, int K, int epi, int32_t* host_token) {
    API_BEGIN_H
    if (!q4 || !e8 || !x) throw std::runtime_error("null pointer");
    if (N < 1 || K < 32 || K % 32 != 0 || ldw % 32 != 0 || ldw < K) throw std::runtime_error("K and ldw must be multiples of 32, ldw >= K, N >= 1");
    if (epi != EPI_NONE && epi != EPI_SWIGLU && epi != EPI_ARGMAX) throw std::runtime_error("epilogue: EPI_NONE, EPI_SWIGLU or EPI_ARGMAX");
    if (epi == EPI_SWIGLU && N % 64 != 0) throw std::runtime_error("SwiGLU needs N % 64 == 0 (32-row gate / up blocks)");
    if (epi != EPI_ARGMAX && !y) throw std::runtime_error("null output pointer");
    GemvArgs a; a.W = nullptr; a.ldw = ldw; a.x = x; a.norm_w = norm_w; a.eps = eps; a.bias = bias; a.res = res; a.y = y; a.N = N; a.K = K; a.epi = epi;
    a.part_val = nullptr; a.part_idx = nullptr; a.w8 = nullptr; a.scale = nullptr; a.skip = nullptr; a.w4 = q4; a.e8 = (const uint8_t*)e8;
    h->impl->op_gemv(a, host_token);
    API_END
}
int svln_op_gemv_mxfp4_batched(svln_engine* h, const void* q4, const void* e8, int ldw, const void* x, int ldx, const void* bias, const void* res,
                               int ldr, void* y, int ldy, int N, int K, int epi, int B, int32_t* host_tokens) {
    API_BEGIN_H
    GemvMx4BatchArgs a; a.q4 = q4; a.e8 = (const uint8_t*)e8; a.ldw = ldw; a.x = x; a.ldx = ldx; a.bias = bias; a.res = res; a.ldr = ldr;
    a.y = y; a.ldy = ldy; a.N = N; a.K = K; a.epi = epi; a.B = B; a.part_val = nullptr; a.part_idx = nullptr;
    h->impl->op_gemv_mxfp4_batched(a, host_tokens);
    API_END
}
int svln_op_gemv_mxfp4_batched_argmax_pen(svln_engine* h, const void* q4, const void* e8, int ldw, const void* x, int ldx, int N, int K, int B,
                                          const void* pen_flags, const int32_t* pen_rows, float penalty, int32_t* host_tokens) {
    API_BEGIN_H
    if (!pen_flags || !pen_rows) throw std::runtime_error("null pointer");
    GemvMx4BatchArgs a; a.q4 = q4; a.e8 = (const uint8_t*)e8; a.ldw = ldw; a.x = x; a.ldx = ldx; a.bias = nullptr; a.res = nullptr; a.ldr = 0;
    a.y = nullptr; a.ldy = 0; a.N = N; a.K = K; a.epi = EPI_ARGMAX; a.B = B; a.part_val = nullptr; a.part_idx = nullptr;
    a.pen_flags = (const uint8_t*)pen_flags; a.pen_rows = pen_rows; a.pen = penalty;
    h->impl->op_gemv_mxfp4_batched(a, host_tokens);
    API_END
}
int svln_op_rmsnorm(svln_engine* h, const void* x, const void* g, void* y, int rows, int n, float eps) { API_BEGIN_H h->impl->op_rmsnorm(x, g, y, rows, n, eps); API_END }
int svln_op_layernorm(svln_engine* h, const void* x, const void* g, const void* b, void* y, int rows, int n, float eps) {
    API_BEGIN_H h->impl->op_layernorm(x, g, b, y, rows, n, eps); API_END
}
int svln_op_rmsnorm_tap(svln_engine* h, const void* x, const void* g, void* y, int rows, int n, float eps, int skip_value, void* y2, int y2_row_value,
                        int y2_cap) {
    API_BEGIN_H h->impl->op_rmsnorm_tap(x, g, y, rows, n, eps, skip_value, y2, y2_row_value, y2_cap); API_END
}
int svln_op_rmsnorm_indexed(svln_engine* h, const void* x, int x_rows, const void* g, void* y, const int32_t* src_rows, const int32_t* tap_rows,
                            void* tap, int tap_cap, int rows, int n, float eps) {
    API_BEGIN_H h->impl->op_rmsnorm_indexed(x, x_rows, g, y, src_rows, tap_rows, tap, tap_cap, rows, n, eps); API_END
}
int svln_op_gather_rows(svln_engine* h, const int32_t* src, int rows, const void* embed, int embed_rows, const void* feats, int feat_rows, void* out,
                        int n, int skip_value) {
    API_BEGIN_H h->impl->op_gather_rows(src, rows, embed, embed_rows, feats, feat_rows, out, n, skip_value); API_END
}
int svln_op_gather_rows_ragged(svln_engine* h, const int32_t* list, int rows, const void* embed, int embed_rows, void* out, int out_rows, int n) {
    API_BEGIN_H h->impl->op_gather_rows_ragged(list, rows, embed, embed_rows, out, out_rows, n); API_END
}
int svln_op_frame_hash(svln_engine* h, const void* pix_dev, int F, int64_t words_per_frame, uint64_t* out_keys) {
    API_BEGIN_H h->impl->op_frame_hash(pix_dev, F, words_per_frame, out_keys); API_END
}
int svln_op_attention_llm(svln_engine* h, void* qkv, int ld, int T, int P, const void* ctx, int ctx_T, void* out, int o_stride, int nsplit) {
    API_BEGIN_H h->impl->op_attention_llm(qkv, ld, T, P, ctx, ctx_T, out, o_stride, nsplit); API_END
}
int svln_op_attention_vit(svln_engine* h, const void* qkv, int ld, int F, void* out, int o_stride) { API_BEGIN_H h->impl->op_attention_vit(qkv, ld, F, out, o_stride); API_END }
int svln_op_attention_decode(svln_engine* h, int B, const void* ctx_qkv, int ld, int64_t ctx_rows, const int32_t* pos, const void* qkv_new, void* out,
                             int o_stride) {
    API_BEGIN_H h->impl->op_attention_decode(B, ctx_qkv, ld, ctx_rows, pos, qkv_new, out, o_stride); API_END
}
int svln_op_attention_verify(svln_engine* h, int rows, const void* ctx_qkv, int ld, int ctx_rows, const void* qkv_new, void* out, int o_stride) {
    API_BEGIN_H h->impl->op_attention_verify(rows, ctx_qkv, ld, ctx_rows, qkv_new, out, o_stride); API_END
}
int svln_op_attention_verify_multi(svln_engine* h, int n_seq, int rows_max, const void* ctx_qkv, int ld, int ctx_rows, const int32_t* ctx_len, const void* qkv_new, const int32_t* rows, int share, void* out, int o_stride) {
    API_BEGIN_H h->impl->op_attention_verify_multi(n_seq, rows_max, ctx_qkv, ld, ctx_rows, ctx_len, qkv_new, rows, share, out, o_stride); API_END
}
int svln_op_verify_step(svln_engine* h, int rows, const int32_t* fed, const int32_t* cand, int count, int max_new, const int64_t* eos, int n_eos,
                        int32_t* new_count, int32_t* done, int64_t* emitted, int32_t* next_token) {
    API_BEGIN_H h->impl->op_verify_step(rows, fed, cand, count, max_new, eos, n_eos, new_count, done, emitted, next_token); API_END
}
int svln_generate_drafts(svln_engine* h, int env, int n_drafts, const int64_t* ids, const int32_t* lens, int max_new_tokens, const int64_t* eos_ids,
                         int n_eos, int64_t* out_ids, int out_cap, int32_t* n_out, int32_t* winner_out, int32_t* pass_tokens_out) {
    API_BEGIN_H h->impl->generate_drafts(env, n_drafts, ids, lens, max_new_tokens, eos_ids, n_eos, out_ids, out_cap, n_out, winner_out, pass_tokens_out); API_END
}
int svln_turn_drafts(svln_engine* h, const svln_turn_args* a, int n_drafts, const int64_t* ids, const int32_t* lens, int64_t* out_ids, int out_cap,
                     int32_t* n_out, int32_t* kv_len, int32_t* winner_out, int32_t* pass_tokens_out) {
    API_BEGIN_H REQUIRE(a, "svln_turn_drafts: null argument"); h->impl->turn_drafts(*a, n_drafts, ids, lens, out_ids, out_cap, n_out, kv_len, winner_out, pass_tokens_out); API_END
}
int svln_drafts_stats(svln_engine* h, int64_t* out) { API_BEGIN_H REQUIRE(out, "svln_drafts_stats: null output pointer"); h->impl->drafts_stats(out); API_END }
int svln_op_draft_select(svln_engine* h, const svln_draft_select_op* op) {
    API_BEGIN_H
    REQUIRE(op, "svln_op_draft_select: null pointer");
    h->impl->op_draft_select(*op);
    API_END
}
int svln_op_argmax_step(svln_engine* h, const svln_argmax_step_op* op) {
    API_BEGIN_H
    if (!op) throw std::runtime_error("null pointer");
    h->impl->op_argmax_step(*op);
    API_END
}
int svln_op_dead_step(svln_engine* h, int done, char* report, int report_cap, int32_t* n_changed) {
    API_BEGIN_H h->impl->op_dead_step(done, report, report_cap, n_changed); API_END
}
int svln_op_kv_read(svln_engine* h, int env, int start, int n, float* k_out, float* v_out) { API_BEGIN_H h->impl->op_kv_read(env, start, n, k_out, v_out); API_END }
int svln_op_llm_qkv_rope(svln_engine* h, const void* x, int T, int P, void* q_out, int q_stride, int32_t* fused) {
    API_BEGIN_H h->impl->op_llm_qkv_rope(x, T, P, q_out, q_stride, fused); API_END
}
int svln_op_set_pages(svln_engine* h, int env, const int32_t* pages, int n) { API_BEGIN_H h->impl->op_set_pages(env, pages, n); API_END }
int svln_op_fill_attn_state(svln_engine* h, float pool_value, int part_nan) { API_BEGIN_H h->impl->op_fill_attn_state(pool_value, part_nan); API_END }
int svln_op_vit_qkv_attention(svln_engine* h, int layer, const void* x, int F, void* qkv_out, void* attn_out, int o_stride, int force_split,
                              int32_t* packer) {
    API_BEGIN_H h->impl->op_vit_qkv_attention(layer, x, F, qkv_out, attn_out, o_stride, force_split, packer); API_END
}
int svln_op_fill_vit_state(svln_engine* h, float pool_value, int part_nan) { API_BEGIN_H h->impl->op_fill_vit_state(pool_value, part_nan); API_END }
int svln_op_vit_kv_read(svln_engine* h, float* k_out, float* v_out) { API_BEGIN_H h->impl->op_vit_kv_read(k_out, v_out); API_END }
int svln_op_pool(svln_engine* h, const void* in, void* out, int F) { API_BEGIN_H h->impl->op_pool(in, out, F); API_END }
int svln_op_patchify(svln_engine* h, const float* pix, void* out, int F) { API_BEGIN_H h->impl->op_patchify(pix, out, F); API_END }

}  // extern "C"
