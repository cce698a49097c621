// Decode-path GEMV  y[N] = epi(W[N,K] . x'[K] + bias) + res  -- the HBM-bound weight stream that
// dominates a batch-1 action-token decode (14.1 GB of bf16 weights per token).
//
// Two kernels, each written once over a WEIGHT-FORMAT POLICY (WPlain<T>, WE4m3, WMxfp4, WP12 below):
//   gemv_rows_kernel<P, EPI>         256-thread workgroups; the activation vector is staged ONCE per workgroup into LDS as fp32 (with a
//       fused RMSNorm the copy holds g * x and rsqrt(mean x^2 + eps) is applied once per output in the epilogue: one pass over x, one
//       barrier), then every wave streams whole weight rows straight HBM -> VGPR with 16-byte loads (lane i takes chunks i, i+64, ... of
//       the row: each wave instruction reads 1 KiB contiguous), 4 rows per wave and two chunks per row in flight (WP12: three) for
//       memory-level parallelism, wave-shuffle reduction, fused epilogue (bias / residual / SwiGLU / arg-max).  No LDS round trip for weights (each
//       byte is used once).
//   gemv_ksplit_kernel<P, NORM, KW>  small N (qkv / o / down of a decode step): a workgroup owns a few rows and its waves split K.
// A policy says what a weight format is and nothing else: elements per 16-byte chunk (hence the LDS planes of the staged activations),
// the per-row handle and the loads of one chunk position, the accumulator and the chunk . x step, the per-row scale after the
// reduction, and the K-split geometry that was measured best for the format.  Staging, the row loop and its clamp, the SwiGLU row
// mapping, the arg-max, the bias / residual / store epilogue, the skip flag and the dispatch exist once, outside the policies.
// gemv_batched_kernel (B environments in lockstep, bf16 / fp32 weights only) is a separate kernel further down.
//
// Roofline: HBM.  Algorithmic bytes per launch = the weight matrix in its format (+ x, y: negligible).
#include <hip/hip_ext.h>

#include <cstdlib>
#include <stdexcept>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace svln {

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int GEMV_THREADS = 256;
constexpr int GEMV_WAVES = GEMV_THREADS / 64;

// ------------------------------------------------------------------------------------------------ weight-format policies
// Common shape of a policy P:
//   X                activation / bias / residual / output type
//   EPC              weights per 16-byte chunk; the staged activations have EPC / 4 LDS planes
//   Row, row(p, n)   handle of weight row n built from GemvArgs;  Chunk, load(row, ci): what chunk position ci of a row needs
//   Acc, zero(), fma(chunk, x2, acc), sum(acc)   the accumulator and the chunk . x step (x2[k]: activations 2k, 2k + 1 under the chunk, fp32)
//   row_scale(p, n)  factor applied to row n's dot product after the reduction
//   X_LATE           row kernel: load the second chunk's activations only after the first chunk's products
//   DEPTH, KS_DEPTH, ROWS_RESIDENT, KS_RESIDENT   (optional; WP12 only) chunks per row in flight in the row / K-split kernel instead of
//                    two (dot_accum_deep instead of dot_accum), and the workgroups per CU the registers must leave room for
//   ROWS_GRID_CAP    row kernel without arg-max: most workgroups of a launch (0: gemv_grid alone decides)
//   KS_R, KS_KW_NARROW, KS_PAIRED   K-split kernel: rows per row group; waves on K when K <= 4096 (4 above: see launch_gemv_fmt);
//                    two chunks per row in flight in the un-normalised form
// The per-format values of the last four are measured choices, not noise: keep them when touching a policy.

// bf16 / fp32 weights in the engine's storage type: one fp32 fmaf chain per row.
template <typename T> struct WPlain {
    using X = T;
    static constexpr int EPC = Elt<T>::PER_CHUNK;
    struct Row { const T* w; };
    using Chunk = uint4;
    using Acc = float;
    static constexpr bool X_LATE = false;
    static constexpr int ROWS_GRID_CAP = 0;
    static constexpr int KS_R = 2;                  // (R = 4 / 8 measured slower at N <= 8192)
    static constexpr int KS_KW_NARROW = 4;
    static constexpr bool KS_PAIRED = true;         // two chunks per row in flight without the norm, one with it: both as measured
    SVLN_DEV static Row row(const GemvArgs& p, size_t n) { return {(const T*)p.W + n * p.ldw}; }
    SVLN_DEV static Chunk load(const Row& r, int ci) { return load_nt(r.w + (size_t)ci * EPC); }
    SVLN_DEV static Acc zero() { return 0.0f; }
    SVLN_DEV static void fma(const Chunk& w, const f32x2* x2, Acc& acc) {
        float f[EPC];
        chunk_to_f32<T>(w, f);
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc = fmaf(f[e], x2[e / 2][e % 2], acc);
    }
    SVLN_DEV static float sum(Acc a) { return a; }
    SVLN_DEV static float row_scale(const GemvArgs&, size_t) { return 1.0f; }
};

// e4m3 and MXFP4 accumulate in two lanes of packed fp32 FMAs (v_pk_fma_f32: the conversions deliver pairs), summed before the wave
// reduction.  Both are opt-in modes of the bf16 engine (the engine refuses to enable them otherwise): X = bf16.
struct WPacked {
    using X = bf16;
    using Acc = f32x2;
    SVLN_DEV static Acc zero() { return f32x2{0.0f, 0.0f}; }
    SVLN_DEV static float sum(Acc a) { return a[0] + a[1]; }
};

// Opt-in decode mode: OCP e4m3 bytes with one fp32 scale per output row, applied once after the wave reduction.
// 16 weights per chunk (v_cvt_pk_f32_fp8: 2 weights per instruction).  Halves the HBM bytes of a decode step; VALU work per byte
// doubles but stays far below the issue limit.
struct WE4m3 : WPacked {
    static constexpr int EPC = 16;
    struct Row { const uint8_t* w; };
    using Chunk = uint4;
    static constexpr bool X_LATE = false;
    static constexpr int ROWS_GRID_CAP = 0;
    static constexpr int KS_R = 4;
    static constexpr int KS_KW_NARROW = 4;
    static constexpr bool KS_PAIRED = false;
    SVLN_DEV static Row row(const GemvArgs& p, size_t n) { return {(const uint8_t*)p.w8 + n * p.ldw}; }
    SVLN_DEV static Chunk load(const Row& r, int ci) { return load_nt(r.w + (size_t)ci * 16); }
    SVLN_DEV static void fma(const Chunk& w, const f32x2* x2, Acc& acc) {
        const unsigned d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[q], false);
            const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[q], true);
            acc = __builtin_elementwise_fma(lo, x2[2 * q], acc);
            acc = __builtin_elementwise_fma(hi, x2[2 * q + 1], acc);
        }
    }
    SVLN_DEV static float row_scale(const GemvArgs& p, size_t n) { return p.scale[n]; }
};

// Opt-in decode mode (svln_set_mxfp4_decode): OCP MXFP4 -- E2M1 elements on the grid {0, 0.5, 1, 1.5, 2, 3, 4, 6} with the sign in
// bit 3, element 2j in the low nibble and 2j + 1 in the high nibble of byte j, and one E8M0 scale byte (2^(byte - 127)) per block of 32
// consecutive elements of a row: q4 [N][K/2] bytes, e8 [N][K/32] bytes, 4.25 bits per weight.  One 16-byte chunk is one MX block; its
// scale byte is shifted into a float's exponent field and sixteen v_cvt_scalef32_pk_f32_fp4 (one byte -> two scaled fp32 values each)
// feed v_pk_fma_f32 against 32 activations.  There is no per-row scale: the block scale is applied by the conversion.
struct WMxfp4 : WPacked {
    static constexpr int EPC = 32;
    struct Row { const uint8_t* q; const uint8_t* s; };
    struct Chunk { uint4 q; unsigned s; };
    static constexpr bool X_LATE = true;            // register pressure: the row kernels sit at 163-179 VGPRs
    static constexpr int ROWS_GRID_CAP = 0;
    static constexpr int KS_R = 4;
    static constexpr int KS_KW_NARROW = 2;          // a row of K = 3584 is only 112 blocks, fewer than two waves' worth of lanes
    static constexpr bool KS_PAIRED = false;
    SVLN_DEV static Row row(const GemvArgs& p, size_t n) {      // row strides of q4 / e8 in bytes: ldw / 2, ldw / 32
        return {(const uint8_t*)p.w4 + n * ((size_t)p.ldw / 2), p.e8 + n * ((size_t)p.ldw / 32)};
    }
    SVLN_DEV static Chunk load(const Row& r, int ci) { return {load_nt(r.q + (size_t)ci * 16), r.s[ci]}; }
    SVLN_DEV static void fma(const Chunk& w, const f32x2* x2, Acc& acc) {
        const unsigned d[4] = {w.q.x, w.q.y, w.q.z, w.q.w};
        const float sc = __uint_as_float(w.s << 23);            // E8M0 -> fp32
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_elementwise_fma((f32x2)__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d[q], sc, 0), x2[4 * q], acc);
            acc = __builtin_elementwise_fma((f32x2)__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d[q], sc, 1), x2[4 * q + 1], acc);
            acc = __builtin_elementwise_fma((f32x2)__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d[q], sc, 2), x2[4 * q + 2], acc);
            acc = __builtin_elementwise_fma((f32x2)__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(d[q], sc, 3), x2[4 * q + 3], acc);
        }
    }
    SVLN_DEV static float row_scale(const GemvArgs&, size_t) { return 1.0f; }
};

// Lossless 12-bit packing of bf16 weights ("P12", svln_set_packed_decode; on by default for the products listed there).  The high
// byte of a bf16 weight (sign, top seven exponent bits) takes few values within one row; the low byte is incompressible.  For bits
// b = s | E[7:0] | m[6:0]:  lo = b & 0xFF, hi7 = (b >> 8) & 0x7F, s = b >> 15.
//   row record, 16 bytes:  T[0..7] -- the row's eight most frequent hi7 values, most frequent first, ties to the lower value, a row with
//       fewer distinct values repeats its last entry -- then a 64-bit mask, bit k = block k of the row "falls back" (K <= 32768).
//   block = 512 consecutive elements = the 64 chunks one wave instruction covers in both kernels; 768 contiguous bytes:
//       [0, 512)    low bytes: lane l's elements 8 l .. 8 l + 7 at offset 8 l
//       [512, 768)  4-bit codes c = s << 3 | j with T[j] == hi7 (the lowest such j): lane l's dword at offset 512 + 4 l; byte k of that
//                   dword holds element k's code in its LOW nibble and element k + 4's in its HIGH nibble (k = 0 .. 3), so that
//                   x & 0x07070707 and (x >> 4) & 0x07070707 are the v_perm_b32 selectors of elements 0 .. 3 and 4 .. 7 into T.
//   A block with an element whose hi7 is not in T has its mask bit set and packed bytes zero; it is read from the bf16 original
//   (W / ldw, resident for prefill anyway).  The packed bytes of EVERY block are loaded without a look at the record (zeros inside the
//   fixed row stride for a fallback block); the record is looked at when a step's chunks are consumed, and only then a fallback block
//   is fetched from the original (WP12 below, consume()).
//   A ragged last block (K % 512 != 0) is zero padded; the packed row stride is ceil(K / 512) * 768 bytes.
// Decoding is s << 15 | T[j] << 8 | lo: the original bit pattern, whatever it means (NaN, Inf, -0, denormals).  The lane -> chunk
// assignment, EPC and the fmaf chain are WPlain<bf16>'s, so every output is bit-equal to the bf16 kernel's.
// v_perm_b32(hi, lo, sel): selector bytes 0 .. 3 pick bytes of `lo`, 4 .. 7 of `hi`, 12 is 0x00.
// The high bytes s << 7 | T[j] of elements 0 .. 3 (ha) and 4 .. 7 (hb) of a chunk from its code dword and the table t0 = T[0..3], t1 = T[4..7]
SVLN_DEV void p12_high_bytes(unsigned c, unsigned t0, unsigned t1, unsigned& ha, unsigned& hb) {
    ha = __builtin_amdgcn_perm(t1, t0, c & 0x07070707u) | ((c << 4) & 0x80808080u);
    hb = __builtin_amdgcn_perm(t1, t0, (c >> 4) & 0x07070707u) | (c & 0x80808080u);
}
// the chunk as 8 bf16 (TEST-ONLY decoder) ...
SVLN_DEV uint4 p12_decode(unsigned lo0, unsigned lo1, unsigned c, unsigned t0, unsigned t1) {
    unsigned ha, hb;
    p12_high_bytes(c, t0, t1, ha, hb);
    return make_uint4(__builtin_amdgcn_perm(ha, lo0, 0x05010400u), __builtin_amdgcn_perm(ha, lo0, 0x07030602u),
                      __builtin_amdgcn_perm(hb, lo1, 0x05010400u), __builtin_amdgcn_perm(hb, lo1, 0x07030602u));
}
// ... and as the 8 floats chunk_to_f32<bf16> makes of those (bits hi << 24 | lo << 16): one v_perm_b32 per weight, no conversion
SVLN_DEV void p12_decode_f32(unsigned lo0, unsigned lo1, unsigned c, unsigned t0, unsigned t1, float* f) {
    unsigned ha, hb;
    p12_high_bytes(c, t0, t1, ha, hb);
    f[0] = __uint_as_float(__builtin_amdgcn_perm(ha, lo0, 0x04000C0Cu)); f[1] = __uint_as_float(__builtin_amdgcn_perm(ha, lo0, 0x05010C0Cu));
    f[2] = __uint_as_float(__builtin_amdgcn_perm(ha, lo0, 0x06020C0Cu)); f[3] = __uint_as_float(__builtin_amdgcn_perm(ha, lo0, 0x07030C0Cu));
    f[4] = __uint_as_float(__builtin_amdgcn_perm(hb, lo1, 0x04000C0Cu)); f[5] = __uint_as_float(__builtin_amdgcn_perm(hb, lo1, 0x05010C0Cu));
    f[6] = __uint_as_float(__builtin_amdgcn_perm(hb, lo1, 0x06020C0Cu)); f[7] = __uint_as_float(__builtin_amdgcn_perm(hb, lo1, 0x07030C0Cu));
}
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((address_space(4))) const u32x4 p12_record_t;
struct WP12 {
    using X = bf16;
    static constexpr int EPC = 8;
    // The record is needed to DECODE a chunk, not to load it: table and mask come in with one uniform-address scalar load per row (SGPRs,
    // counted on lgkmcnt, so vmcnt stays exact for the stream), issued in front of the row group's weight loads and first looked at behind
    // the loads of the group's first step (consume()).  No load address depends on it.
    struct Row { const uint8_t* pk; const bf16* W; unsigned ldw, n, t0, t1, m0, m1; };      // (W, ldw: the launch's, one copy for all rows)
    // A chunk in flight is 12 bytes in 3 VGPRs: the 8 low bytes and the lane's own code dword, loaded UNCONDITIONALLY at addresses the
    // record has no part in.  In bounds for every block of every row: the packed row stride p12_row_bytes(K) covers ceil(K / 512) whole
    // blocks -- a fallback block's bytes are zeros, a ragged last block is zero padded -- and blk < ceil(K / 512) whenever a lane of it is
    // active.  (blk: the wave-uniform block index, a scalar.)
    struct Chunk { u32x2 a; unsigned c; int blk; };
    using Acc = float;
    // Chunks per row in flight (a CU streams bytes in flight / ~4.5-5 us of loaded HBM latency: profiles/r04_stream_layout_bench.txt).
    // Row kernels: 3 -> 4 rows x 3 x 768 B = 9 KB per wave, 100-121 VGPRs, 4 waves per SIMD as at depth 2: 144 KB per CU instead of 96.
    // K-split (down_proj): 3 -> 2 rows x 3 x 768 B = 4.5 KB per wave at 70 VGPRs, its 7 workgroups per CU still resident: 126 KB
    // instead of 84; depth 4 takes 84 VGPRs (5 waves per SIMD: 120 KB) or, held to 72, spills.  Measured: DESIGN.md 4.1.
    static constexpr int DEPTH = 3, KS_DEPTH = 3;
    // ... and the workgroups per CU (= waves per SIMD) the register allocation is held to in the row kernels, so that no epilogue pays
    // for the depth in waves (without it EPI_SAMPLE_TOPK took 133 VGPRs); the K-split kernel fits on its own (1: no bound)
    static constexpr int ROWS_RESIDENT = 4, KS_RESIDENT = 1;
    // four workgroups per CU are resident, at depth 3 as at depth 2.  With gate/up's 1184 workgroups the last 160 ran as a second round of
    // a kernel that is not bandwidth-bound (depth 2: 41.3 us per launch; 1024: 39.0 us alone, 40.5 against 43.3 in the decode step: DESIGN.md 4.1)
    static constexpr int ROWS_GRID_CAP = 1024;
    static constexpr int KS_R = 2;                  // the bf16 policy's K-split geometry: the lane -> chunk assignment is part of the bit-equality contract
    static constexpr int KS_KW_NARROW = 4;
    static constexpr bool KS_PAIRED = true;
    // a wave-uniform byte offset, said so (scalar base + lane offset addressing).  The offset, not the pointer: a pointer rebuilt from
    // integers loses its address space, and every load through it becomes a flat load that also counts as an LDS operation
    SVLN_DEV static size_t uniform(size_t v) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
        return ((size_t)hi << 32) | lo;
    }
    SVLN_DEV static Row row(const GemvArgs& p, size_t n) {
        // (the records are read-only for the whole launch and the address is wave-uniform: the constant address space makes it a scalar load)
        const u32x4 rec = *(p12_record_t*)((size_t)p.prec + uniform(n * 16));
        return {(const uint8_t*)p.wp + uniform(n * p12_row_bytes(p.K)), (const bf16*)p.W, (unsigned)p.ldw, (unsigned)__builtin_amdgcn_readfirstlane((int)n), rec.x, rec.y, rec.z,
                rec.w};
    }
    SVLN_DEV static Chunk load(const Row& r, int ci) {          // (ci = lane + a multiple of 64 in both kernels: the block is wave-uniform)
        Chunk c;
        c.blk = __builtin_amdgcn_readfirstlane(ci >> 6);
        const unsigned l = (unsigned)ci & 63u;
        const uint8_t* pb = r.pk + (size_t)c.blk * 768;
        c.a = __builtin_nontemporal_load((const u32x2*)(pb + (l << 3)));
        c.c = __builtin_nontemporal_load((const unsigned*)(pb + 512 + (l << 2)));
        return c;
    }
    SVLN_DEV static Acc zero() { return 0.0f; }
    SVLN_DEV static bool falls_back(const Row& r, int blk) { return (((blk & 32) ? r.m1 : r.m0) >> (blk & 31)) & 1u; }
    // does no row of the group fall back on a block of `blocks` (bit k = block k)?  One scalar AND per row.
    template <int R> SVLN_DEV static bool all_packed(const Row (&rows)[R], unsigned long long blocks) {
        // (the empty asm keeps the look at the masks HERE, behind the step's loads: the union of the rows' masks does not change from step to
        // step, and formed in front of the loop it makes the wave wait for the records before its first weight load)
        unsigned long long hit = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            unsigned long long m = ((unsigned long long)rows[r].m1 << 32) | rows[r].m0;
            asm volatile("" : "+s"(m));
            hit |= m & blocks;
        }
        return hit == 0;
    }
    SVLN_DEV static void chain(const float* f, const f32x2* x2, Acc& acc) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc = fmaf(f[e], x2[e / 2][e % 2], acc);
    }
    // the step of a group without a fallback block: decode and multiply, nothing else
    SVLN_DEV static void fma(const Row& r, const Chunk& w, const f32x2* x2, Acc& acc) {
        float f[EPC];
        p12_decode_f32(w.a.x, w.a.y, w.c, r.t0, r.t1, f);
        chain(f, x2, acc);
    }
    // ... and of a group with one (0.2 % of the blocks of real weights, so this path may drain the stream).  A fallback block (a scalar
    // branch) is fetched HERE, when the row's chain reaches it, from the bf16 original -- lane l's 16 bytes at element blk * 512 + 8 l
    // of the row, below K for every active lane exactly as in WPlain -- and waited for at once; its zero packed bytes are never decoded.
    // (the empty asm pins each chunk's products where they stand: left alone, the compiler moves every chain of the group behind the
    // last branch and keeps all the decoded values in registers until then)
    SVLN_DEV static void fma_checked(const Row& r, int ci, const Chunk& w, const f32x2* x2, Acc& acc) {
        float f[EPC];
        if (falls_back(r, w.blk)) {
            unsigned off = ((unsigned)ci & 63u) << 4;
            asm volatile("" : "+v"(off));           // (the address is formed here: hoisted, it is two registers per row held through the whole kernel)
            chunk_to_f32<bf16>(load_nt((const uint8_t*)(r.W + (size_t)r.n * r.ldw) + (size_t)w.blk * 1024 + off), f);
        } else p12_decode_f32(w.a.x, w.a.y, w.c, r.t0, r.t1, f);
        chain(f, x2, acc);
        asm volatile("" : "+v"(acc));
    }
    SVLN_DEV static float sum(Acc a) { return a; }
    SVLN_DEV static float row_scale(const GemvArgs&, size_t) { return 1.0f; }
};
// chunks per row in flight: two, unless the policy says otherwise (WP12: a chunk in flight is 3 registers, not 4)
template <typename P, typename = void> struct StreamDepth { static constexpr bool OWN = false; static constexpr int ROWS = 2, KSPLIT = 2, ROWS_WG = 1, KS_WG = 1; };
template <typename P> struct StreamDepth<P, decltype((void)P::DEPTH)> {
    static constexpr bool OWN = true;
    static constexpr int ROWS = P::DEPTH, KSPLIT = P::KS_DEPTH, ROWS_WG = P::ROWS_RESIDENT, KS_WG = P::KS_RESIDENT;
};
// acc[r] += w[d][r] . x[d] for the D chunk positions ci, ci + stride, ... of R rows, every row's chunks in ascending order.  WP12: all
// loads of the step have been issued; only now the records are looked at (sched_barrier: the scalar test, and with it the wait for the
// records, stays behind the loads), ONE wave-uniform branch per step: no fallback block among the D x R -> the plain decode, a basic
// block of its own whose waits on the loads are counted; otherwise the checked form.  Every load of w is used on both sides, so none can
// sink behind the branch.
template <typename P, int R, int D>
SVLN_DEV void consume(const typename P::Row (&rows)[R], int ci, int stride, const typename P::Chunk (&w)[D][R], const f32x2 (&x)[D][P::EPC / 2],
                      typename P::Acc (&acc)[R]) {
    if constexpr (std::is_same<P, WP12>::value) {
        unsigned long long blocks = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) blocks |= 1ull << w[d][0].blk;
        __builtin_amdgcn_sched_barrier(0);
        if (P::all_packed(rows, blocks)) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int d = 0; d < D; ++d) P::fma(rows[r], w[d][r], x[d], acc[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int d = 0; d < D; ++d) P::fma_checked(rows[r], ci + d * stride, w[d][r], x[d], acc[r]);
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int d = 0; d < D; ++d) P::fma(w[d][r], x[d], acc[r]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ shared pieces
// x in LDS as fp32, split in PLANES 16-byte planes per weight chunk so that consecutive lanes read consecutive 16 B (conflict-free):
// element 4 * q + e of the activations under weight chunk cj lives at xs[q * nch * 4 + cj * 4 + e]  (nch = weight chunks per row).
// With a fused RMSNorm the LDS copy holds g * x (one pass over x, one barrier) and the function returns rsqrt(mean(x^2) + eps):
// y = rstd * (W . (g * x)) -- the scale is applied once per output in the epilogue (same folding as gemv_ksplit_kernel).
template <typename X, int PLANES>
SVLN_DEV float stage_x(float* xs, const GemvArgs& p, int nch) {
    constexpr int XEPC = Elt<X>::PER_CHUNK;         // one activation chunk fills XP planes; XPW of them lie under one weight chunk
    constexpr int XP = XEPC / 4, XPW = PLANES / XP;
    __shared__ float red[GEMV_WAVES];
    const X* x = (const X*)p.x;
    const X* g = (const X*)p.norm_w;
    const int tid = threadIdx.x, nxch = p.K / XEPC;
    float ss = 0.0f;
    for (int ci = tid; ci < nxch; ci += GEMV_THREADS) {
        float f[XEPC];
        chunk_to_f32<X>(*(const uint4*)(x + (size_t)ci * XEPC), f);
        if (g) {
            float gf[XEPC];
            chunk_to_f32<X>(*(const uint4*)(g + (size_t)ci * XEPC), gf);
#pragma unroll
            for (int e = 0; e < XEPC; ++e) { ss = fmaf(f[e], f[e], ss); f[e] *= gf[e]; }
        }
        const int cj = ci / XPW, p0 = (ci % XPW) * XP;
#pragma unroll
        for (int q = 0; q < XP; ++q)
            *(float4*)(xs + (size_t)(p0 + q) * nch * 4 + (size_t)cj * 4) = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
    }
    if (g) {
        ss = wave_sum(ss);
        if ((tid & 63) == 0) red[tid >> 6] = ss;
    }
    __syncthreads();
    if (!g) return 1.0f;
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < GEMV_WAVES; ++w) tot += red[w];
    return rsqrtf(tot / (float)p.K + p.eps);
}

// the activations under weight chunk ci as fp32 pairs (x2[k] = activations 2k, 2k + 1): from the staged LDS copy, or straight from
// global memory (L2-resident, 7-37 KB)
template <int PLANES>
SVLN_DEV void load_x(const float* xs, int nch, int ci, f32x2* x2) {
#pragma unroll
    for (int q = 0; q < PLANES; ++q) {
        const float4 v = *(const float4*)(xs + (size_t)q * nch * 4 + (size_t)ci * 4);
        x2[2 * q] = f32x2{v.x, v.y};
        x2[2 * q + 1] = f32x2{v.z, v.w};
    }
}
// (global form) NORM: x2 holds g * x, and the squares of x are added to ss in element order; returns the new ss
template <typename P, bool NORM>
SVLN_DEV float load_xg(const typename P::X* xg, const typename P::X* gg, int ci, f32x2* x2, float ss) {
    using X = typename P::X;
    constexpr int XEPC = Elt<X>::PER_CHUNK;
#pragma unroll
    for (int h = 0; h < P::EPC / XEPC; ++h) {
        float fh[XEPC];
        chunk_to_f32<X>(*(const uint4*)(xg + (size_t)ci * P::EPC + h * XEPC), fh);
        if (NORM) {
            float gf[XEPC];
            chunk_to_f32<X>(*(const uint4*)(gg + (size_t)ci * P::EPC + h * XEPC), gf);
#pragma unroll
            for (int e = 0; e < XEPC; ++e) { ss = fmaf(fh[e], fh[e], ss); fh[e] *= gf[e]; }
        }
#pragma unroll
        for (int e = 0; e < XEPC / 2; ++e) x2[h * (XEPC / 2) + e] = f32x2{fh[2 * e], fh[2 * e + 1]};
    }
    return ss;
}

// acc[r] += row r . x over the chunks ci = c0 + lane + 64*k*cstep (k = 0, 1, ...) below nch, two chunks per row in flight
// (2R x 1 KiB per wave).  XLDS: x comes from the workgroup's LDS copy (possibly RMS-normalised); otherwise each lane reads the
// x chunk it needs from global memory next to its weight chunks.
template <typename P, int R, bool XLDS>
SVLN_DEV void dot_accum(const typename P::Row (&rows)[R], const float* xs, const typename P::X* xg, int nch, int c0, int cstep, int lane,
                        typename P::Acc (&acc)[R]) {
    constexpr int EPC = P::EPC;
    auto get_x = [&](int ci, f32x2* x2) {
        if (XLDS) load_x<EPC / 4>(xs, nch, ci, x2);
        else load_xg<P, false>(xg, nullptr, ci, x2, 0.0f);
    };
    const int stride = 64 * cstep;
    int ci = c0 + lane;
    for (; ci + stride < nch; ci += 2 * stride) {
        typename P::Chunk w0[R], w1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            w0[r] = P::load(rows[r], ci);
            w1[r] = P::load(rows[r], ci + stride);
        }
        f32x2 x0[EPC / 2];
        get_x(ci, x0);
        if (P::X_LATE) {
#pragma unroll
            for (int r = 0; r < R; ++r) P::fma(w0[r], x0, acc[r]);
            get_x(ci + stride, x0);
#pragma unroll
            for (int r = 0; r < R; ++r) P::fma(w1[r], x0, acc[r]);
        } else {
            f32x2 x1[EPC / 2];
            get_x(ci + stride, x1);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                P::fma(w0[r], x0, acc[r]);
                P::fma(w1[r], x1, acc[r]);
            }
        }
    }
    for (; ci < nch; ci += stride) {
        typename P::Chunk w0[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w0[r] = P::load(rows[r], ci);
        f32x2 x0[EPC / 2];
        get_x(ci, x0);
#pragma unroll
        for (int r = 0; r < R; ++r) P::fma(w0[r], x0, acc[r]);
    }
}

// the same over D chunks per row in flight (StreamDepth<P>: a policy with its own DEPTH), in the same ascending chunk order: a main loop
// of D positions, then the remainders one by one.  The two-deep form above stays as it is for the policies that were tuned on it.
// A step issues its loads and nothing else (sched_barrier) -- without LDS the raw activation chunks first: they are the oldest loads, so
// unpacking them waits for them alone -- and only then turns to the activations and the products.
template <typename P, int R, bool XLDS, int D>
SVLN_DEV void deep_step(const typename P::Row (&rows)[R], const float* xs, const typename P::X* xg, int nch, int ci, int stride,
                        typename P::Acc (&acc)[R]) {
    using X = typename P::X;
    constexpr int EPC = P::EPC, XEPC = Elt<X>::PER_CHUNK, XH = EPC / XEPC;
    [[maybe_unused]] uint4 raw[D][XH];
    if constexpr (!XLDS) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int h = 0; h < XH; ++h) raw[d][h] = *(const uint4*)(xg + (size_t)(ci + d * stride) * EPC + h * XEPC);
        }
    }
    typename P::Chunk w[D][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int d = 0; d < D; ++d) w[d][r] = P::load(rows[r], ci + d * stride);
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x2 x[D][EPC / 2];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if constexpr (XLDS) {
            load_x<EPC / 4>(xs, nch, ci + d * stride, x[d]);
        } else {
#pragma unroll
            for (int h = 0; h < XH; ++h) {
                float fh[XEPC];
                chunk_to_f32<X>(raw[d][h], fh);
#pragma unroll
                for (int e = 0; e < XEPC / 2; ++e) x[d][h * (XEPC / 2) + e] = f32x2{fh[2 * e], fh[2 * e + 1]};
            }
        }
    }
    consume<P, R, D>(rows, ci, stride, w, x, acc);
}
template <typename P, int R, bool XLDS, int D>
SVLN_DEV void dot_accum_deep(const typename P::Row (&rows)[R], const float* xs, const typename P::X* xg, int nch, int c0, int cstep, int lane,
                             typename P::Acc (&acc)[R]) {
    const int stride = 64 * cstep;
    int ci = c0 + lane;
    for (; ci + (D - 1) * stride < nch; ci += D * stride) deep_step<P, R, XLDS, D>(rows, xs, xg, nch, ci, stride, acc);
    for (; ci < nch; ci += stride) deep_step<P, R, XLDS, 1>(rows, xs, xg, nch, ci, stride, acc);
}

// bias / residual / store of output n
template <typename X>
SVLN_DEV void store_out(const GemvArgs& p, int n, float v) {
    if (p.bias) v += to_f32(((const X*)p.bias)[n]);
    if (p.res) v += to_f32(((const X*)p.res)[n]);
    ((X*)p.y)[n] = from_f32<X>(v);
}

// ------------------------------------------------------------------------------------------------ wave-per-rows kernel
// A wave takes groups of R = 4 weight rows: R consecutive outputs, or with EPI_SWIGLU the (gate, up) rows of 2 consecutive outputs.
template <typename P, int EPI>
__global__ __launch_bounds__(GEMV_THREADS, StreamDepth<P>::ROWS_WG) void gemv_rows_kernel(GemvArgs p) {
    using X = typename P::X;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* xs = (float*)smem_raw;
    const int skip = p.skip ? *p.skip : 0;        // checked after the activation staging, so the flag's load latency hides behind it
    constexpr int R = 4, OUTS = EPI == EPI_SWIGLU ? R / 2 : R;     // rows / outputs per group
    const int nch = p.K / P::EPC;
    const float xscale = stage_x<X, P::EPC / 4>(xs, p, nch);
    if (skip) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * GEMV_WAVES + wave, nw = gridDim.x * GEMV_WAVES;
    const int n_out = EPI == EPI_SWIGLU ? p.N >> 1 : p.N;

    constexpr HeadForm F = head_form(EPI);
    constexpr bool AMAX = epi_is_argmax(EPI), TOPK = F.topk, ENT = F.ent, LSE = F.lse, SMP = F.smp;
    static_assert(!F.tgt, "the wave-per-rows GEMV has no forced form");
    // EPI_*_TOPK: the wave's TOPK_C best (y, column) pairs, entry l in lane l < TOPK_C, y descending then column ascending; a logit is
    // wave-uniform, so is tk_thr = entry TOPK_C - 1, and the common case of a column costs one scalar compare against it
    [[maybe_unused]] float tk_v = -INFINITY, tk_thr = -INFINITY;
    [[maybe_unused]] int tk_i = 0x7FFFFFFF;
    [[maybe_unused]] auto tk_insert = [&](float y, int col) {
        if (!(y > tk_thr)) return;                // NaN, -inf, or not above the last entry (columns ascend: an equal value stays behind)
        const float up_v = __shfl_up(tk_v, 1, 64);
        const int up_i = __shfl_up(tk_i, 1, 64);
        if (!(tk_v >= y)) {                       // entries at or above y stay; y lands behind them and the rest moves down one lane
            const bool here = lane == 0 || up_v >= y;
            tk_v = here ? y : up_v;
            tk_i = here ? col : up_i;
        }
        tk_thr = __shfl(tk_v, TOPK_C - 1, 64);
    };
    float best = -INFINITY;                       // EPI_ARGMAX (EPI_SAMPLE: the best perturbed value z)
    int best_i = 0x7FFFFFFF;
    float lm = -INFINITY, ls = 0.0f;              // EPI_ARGMAX_LSE: wave-uniform (max, sum exp(l - max)) over the wave's rows (EPI_SAMPLE: over y)
    [[maybe_unused]] float lt = 0.0f;             // EPI_*_ENT: sum (l - max) exp(l - max) beside ls
    [[maybe_unused]] float best_raw = -INFINITY;  // EPI_SAMPLE: the y of the best z
    [[maybe_unused]] int smp_stream = 0, smp_draw = 0;
    if constexpr (SMP) { smp_stream = p.smp.stream[0]; smp_draw = p.smp.draw[0] + (p.smp.count ? *p.smp.count : 0); }
    for (int n0 = gw * OUTS; n0 < n_out; n0 += nw * OUTS) {
        size_t rn[R];                             // the group's weight rows; a ragged last group repeats the last output's rows
#pragma unroll
        for (int u = 0; u < OUTS; ++u) {
            const int j = min(n0 + u, n_out - 1);
            if (EPI == EPI_SWIGLU) { rn[2 * u] = swiglu_gate_row(j); rn[2 * u + 1] = rn[2 * u] + 32; }
            else rn[u] = (size_t)j;
        }
        typename P::Row rows[R];
        typename P::Acc a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { rows[r] = P::row(p, rn[r]); a[r] = P::zero(); }
        if constexpr (!StreamDepth<P>::OWN) dot_accum<P, R, true>(rows, xs, nullptr, nch, 0, 1, lane, a);
        else dot_accum_deep<P, R, true, StreamDepth<P>::ROWS>(rows, xs, nullptr, nch, 0, 1, lane, a);
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = wave_sum(P::sum(a[r])) * (P::row_scale(p, rn[r]) * xscale);
        if (EPI == EPI_SWIGLU) {
            if (lane < OUTS && n0 + lane < n_out) {
                const float gt = lane == 0 ? acc[0] : acc[2], up = lane == 0 ? acc[1] : acc[3];
                ((X*)p.y)[n0 + lane] = from_f32<X>(silu_f(gt) * up);
            }
        } else if (AMAX) {
            if (p.pen_flags) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (n0 + r < p.N && p.pen_flags[n0 + r]) acc[r] = acc[r] < 0.0f ? acc[r] * p.pen : acc[r] / p.pen;
            }
            if constexpr (SMP) {
                // lane l evaluates the noise of column n0 + (l & 3) -- one Philox per group, not four -- and the wave reads lanes 0 .. 3
                const float gq = gumbel_noise(p.smp.seed_lo, p.smp.seed_hi, smp_stream, smp_draw, n0 + (lane & 3));
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float y = acc[r] * p.smp.inv_t, z = __fadd_rn(y, __shfl(gq, r, 64));       // (fl(y + G), never fma(acc, inv_t, G): truncate_partials_kernel adds the same G to the stored y)
                    if (n0 + r < p.N) {
                        if (z > best) { best = z; best_i = n0 + r; best_raw = y; }         // rows ascend: first max wins
                        if constexpr (ENT) ent_add(y, lm, ls, lt); else lse_add(y, lm, ls);
                        if constexpr (TOPK) tk_insert(y, n0 + r);
                    }
                }
            } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (n0 + r < p.N && acc[r] > best) { best = acc[r]; best_i = n0 + r; }     // rows ascend: first max wins
            }
            if (LSE) {                            // the penalised values; the repeated rows of a ragged last group (n0 + r >= N) count once
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (n0 + r < p.N) {
                        if constexpr (ENT) ent_add(acc[r], lm, ls, lt); else lse_add(acc[r], lm, ls);
                        if constexpr (TOPK) tk_insert(acc[r], n0 + r);
                    }
            }
        } else if (lane < R && n0 + lane < p.N) {
            store_out<X>(p, n0 + lane, lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3]);
        }
    }
    if (AMAX) {
        __shared__ float bv[GEMV_WAVES];
        __shared__ int bi[GEMV_WAVES];
        if constexpr (TOPK) {
            // the four waves' lists -> the workgroup's: candidate t is entry t % TOPK_C of wave t / TOPK_C; its place is the number of
            // candidates before it in (y descending, column ascending) order -- padding, all alike, keeps its own order -- so the places
            // are a permutation and the first TOPK_C of them are the partial's list
            __shared__ float cv[GEMV_WAVES * TOPK_C];
            __shared__ int ci[GEMV_WAVES * TOPK_C];
            if (lane < TOPK_C) { cv[wave * TOPK_C + lane] = tk_v; ci[wave * TOPK_C + lane] = tk_i; }
            __syncthreads();
            if (threadIdx.x < GEMV_WAVES * TOPK_C) {
                const int t = threadIdx.x;
                const float v = cv[t];
                const int i = ci[t];
                int place = 0;
#pragma unroll
                for (int o = 0; o < GEMV_WAVES * TOPK_C; ++o)
                    place += cv[o] > v || (cv[o] == v && (ci[o] < i || (ci[o] == i && o < t)));
                if (place < TOPK_C) {
                    p.cand_val[(size_t)blockIdx.x * TOPK_C + place] = v;
                    p.cand_idx[(size_t)blockIdx.x * TOPK_C + place] = i;
                }
            }
        }
        if (lane == 0) { bv[wave] = best; bi[wave] = best_i; }
        if constexpr (SMP) {
            __shared__ float bs[GEMV_WAVES], bm[GEMV_WAVES], br[GEMV_WAVES];
            if (lane == 0) { bs[wave] = ls; bm[wave] = lm; br[wave] = best_raw; }
            __syncthreads();
            if (threadIdx.x == 0) {               // a wave without a row is (-inf, 0) and adds 0
                float v = bv[0], m = bm[0], raw = br[0]; int i = bi[0];
#pragma unroll
                for (int w = 1; w < GEMV_WAVES; ++w) {
                    if (bv[w] > v || (bv[w] == v && bi[w] < i)) { v = bv[w]; i = bi[w]; raw = br[w]; }
                    m = bm[w] > m ? bm[w] : m;
                }
                float sum = 0.0f;
#pragma unroll
                for (int w = 0; w < GEMV_WAVES; ++w) sum += lse_rescale(bs[w], bm[w], m);
                p.part_val[blockIdx.x] = v; p.part_idx[blockIdx.x] = i; p.smp.part_raw[blockIdx.x] = raw;
                p.smp.part_max[blockIdx.x] = m; p.part_sum[blockIdx.x] = sum;
            }
            if constexpr (ENT) {                  // the four waves' t, each seen from the workgroup's maximum (bs / bm are unchanged)
                __shared__ float bt[GEMV_WAVES];
                if (lane == 0) bt[wave] = lt;
                __syncthreads();
                if (threadIdx.x == 0) {
                    float m = bm[0];
#pragma unroll
                    for (int w = 1; w < GEMV_WAVES; ++w) m = bm[w] > m ? bm[w] : m;
                    float te = 0.0f;
#pragma unroll
                    for (int w = 0; w < GEMV_WAVES; ++w) te += ent_rescale(bt[w], bs[w], bm[w], m);
                    p.part_ent[blockIdx.x] = te;
                }
            }
            return;
        }
        if constexpr (LSE) {
            __shared__ float bs[GEMV_WAVES];
            [[maybe_unused]] __shared__ float bt[ENT ? GEMV_WAVES : 1];
            if (lane == 0) bs[wave] = ls;         // (lm == best: the same compares in the same order)
            if constexpr (ENT) if (lane == 0) bt[wave] = lt;
            __syncthreads();
            if (threadIdx.x == 0) {               // a wave without a row is (-inf, 0) and adds 0
                float v = bv[0];
#pragma unroll
                for (int w = 1; w < GEMV_WAVES; ++w) v = bv[w] > v ? bv[w] : v;
                float sum = 0.0f;
#pragma unroll
                for (int w = 0; w < GEMV_WAVES; ++w) sum += lse_rescale(bs[w], bv[w], v);
                p.part_sum[blockIdx.x] = sum;
                if constexpr (ENT) {
                    float te = 0.0f;
#pragma unroll
                    for (int w = 0; w < GEMV_WAVES; ++w) te += ent_rescale(bt[w], bs[w], bv[w], v);
                    p.part_ent[blockIdx.x] = te;
                }
            }
        } else {
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            float v = bv[0]; int i = bi[0];
#pragma unroll
            for (int w = 1; w < GEMV_WAVES; ++w)
                if (bv[w] > v || (bv[w] == v && bi[w] < i)) { v = bv[w]; i = bi[w]; }
            p.part_val[blockIdx.x] = v;
            p.part_idx[blockIdx.x] = i;
        }
    }
}

// ------------------------------------------------------------------------------------------------ K-split kernel
// Small-N variant (qkv / o / down projections of a decode step: N <= 8192 rows is only 224-288 workgroups of the wave-per-rows kernel,
// i.e. < 1 per CU).  KW of the workgroup's 4 waves split K (interleaved 1 KiB blocks) and the 4 / KW groups of KW waves take
// R = P::KS_R rows each, so N / (R * 4 / KW) workgroups exist (3.5-4.5 per CU) and their prologues overlap other workgroups' streams.
// RMSNorm is folded into the product, no prologue:  y = rsqrt(mean(x^2) + eps) * sum_i W[n][i] * (g[i] * x[i]); every wave reads its
// K share of x and g from global memory next to its weight chunks (L2-resident, 7 KB each).  No staging to hide the skip flag's load
// behind: the kernel returns at once.
template <typename P, bool NORM, int KW>
__global__ __launch_bounds__(GEMV_THREADS, StreamDepth<P>::KS_WG) void gemv_ksplit_kernel(GemvArgs p) {
    using X = typename P::X;
    constexpr int R = P::KS_R, EPC = P::EPC;
    constexpr int RG = GEMV_WAVES / KW;             // row groups per workgroup
    __shared__ float part[GEMV_WAVES][R + 1];       // [.][R] = the wave's share of sum(x^2) when NORM
    if (p.skip && *p.skip) return;
    const int nch = p.K / EPC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kw = RG == 1 ? wave : wave % KW, rg = RG == 1 ? 0 : wave / KW;      // (rg spelled out as 0: the row index stays scalar)
    const X* xg = (const X*)p.x;
    const X* gg = (const X*)p.norm_w;
    for (int b0 = blockIdx.x * RG * R; b0 < p.N; b0 += gridDim.x * RG * R) {
        const int n0 = b0 + rg * R;                 // (may lie beyond N for the last workgroup: rows clamp, nothing is written)
        typename P::Row rows[R];
        typename P::Acc a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { rows[r] = P::row(p, (size_t)min(n0 + r, p.N - 1)); a[r] = P::zero(); }
        float ss = 0.0f;
        if (!NORM && P::KS_PAIRED) {
            if constexpr (!StreamDepth<P>::OWN) dot_accum<P, R, false>(rows, nullptr, xg, nch, kw * 64, KW, lane, a);
            else dot_accum_deep<P, R, false, StreamDepth<P>::KSPLIT>(rows, nullptr, xg, nch, kw * 64, KW, lane, a);
        } else {
            for (int ci = kw * 64 + lane; ci < nch; ci += 64 * KW) {
                typename P::Chunk w[1][R];
#pragma unroll
                for (int r = 0; r < R; ++r) w[0][r] = P::load(rows[r], ci);
                // all R weight loads are issued before anything else of the iteration: left alone, the scheduler sinks some of them
                // below the norm arithmetic and waits for each in turn (seen in the e4m3 NORM form)
                __builtin_amdgcn_sched_barrier(0);
                f32x2 xf[1][EPC / 2];
                ss = load_xg<P, NORM>(xg, gg, ci, xf[0], ss);
                consume<P, R, 1>(rows, ci, 64 * KW, w, xf, a);
            }
        }
        // the accumulators stay R separate values: without this the SLP vectoriser, seeded by the R horizontal sums below, fuses the
        // rows' packed FMAs of the e4m3 NORM form into <8 x float> operations (88 VGPRs instead of 80, one wave per SIMD fewer)
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" : "+v"(a[r]));
        float acc[R + 1];
        acc[R] = NORM ? wave_sum(ss) : 0.0f;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = wave_sum(P::sum(a[r]));
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r <= R; ++r) part[wave][r] = acc[r];
        }
        __syncthreads();
        if (threadIdx.x < RG * R) {
            const int g2 = threadIdx.x / R, r = threadIdx.x % R, n = b0 + g2 * R + r;
            if (n < p.N) {
                float v = part[g2 * KW][r], s2 = part[g2 * KW][R];
#pragma unroll
                for (int k = 1; k < KW; ++k) { v += part[g2 * KW + k][r]; s2 += part[g2 * KW + k][R]; }
                v *= P::row_scale(p, n);
                if (NORM) v *= rsqrtf(s2 / (float)p.K + p.eps);
                store_out<X>(p, n, v);
            }
        }
        __syncthreads();
    }
}

// Batched decode GEMV for B environments decoded in lockstep (SURVEY.md 8f-1 / BASELINE configs[4]):
//   Y[b][n] = epi(W[n,:] . x'_b + bias[n]) + res[b][n],   x'_b = x_b or rmsnorm(x_b) * g  (folded, no prologue)
// Every weight byte is streamed from HBM once for all B activations.  Workgroup = 4 rows (SwiGLU: 2 outputs), its 4 waves
// split K; per chunk position a lane loads 4 weight chunks (non-temporal) + B activation chunks (L2-resident) and does
// 4 * B * 8 FMAs.  Partial sums (and the per-env sum of squares) are reduced across waves through LDS.
template <typename T, int EPI, bool NORM, int B>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_batched_kernel(GemvBatchArgs p) {
    constexpr int EPC = Elt<T>::PER_CHUNK, R = 4, STRIDE = 64 * GEMV_WAVES;       // (R = 8 measured no better at B = 8: dot2-issue bound)
    __shared__ float part[GEMV_WAVES][R * B + B];
    const int nch = p.K / EPC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const T* W = (const T*)p.W;
    const T* xg = (const T*)p.x;
    const T* gg = (const T*)p.norm_w;
    const int n_units = EPI == EPI_SWIGLU ? p.N / R : (p.N + R - 1) / R;      // one unit = R weight rows
    constexpr HeadForm F = head_form(EPI);
    constexpr bool AMAX = epi_is_argmax(EPI), TGT = F.tgt, TOPK = F.topk, ENT = F.ent, LSE = F.lse, SMP = F.smp;
    static_assert(!(TOPK && NORM), "EPI_*_TOPK has no fused-norm form");
    static_assert(!(ENT && NORM), "EPI_*_ENT has no fused-norm form");
    // EPI_*_TOPK: thread b < B keeps env b's TOPK_C best (y, column) pairs of the workgroup's units in registers, y descending then column
    // ascending (static indices: the insertion is an unrolled shift).  Units and their columns ascend, so an equal value stays behind.
    [[maybe_unused]] float tk_v[TOPK ? TOPK_C : 1];
    [[maybe_unused]] int tk_i[TOPK ? TOPK_C : 1];
    if constexpr (TOPK) {
#pragma unroll
        for (int e = 0; e < TOPK_C; ++e) { tk_v[e] = -INFINITY; tk_i[e] = 0x7FFFFFFF; }
    }
    [[maybe_unused]] auto tk_insert = [&](float y, int col) {
        if constexpr (TOPK) {
            if (!(y > tk_v[TOPK_C - 1])) return;      // NaN, -inf, or not above the last entry
            bool placed = false;
#pragma unroll
            for (int e = TOPK_C - 1; e >= 1; --e) {
                if (placed) continue;
                if (tk_v[e - 1] >= y) { tk_v[e] = y; tk_i[e] = col; placed = true; }
                else { tk_v[e] = tk_v[e - 1]; tk_i[e] = tk_i[e - 1]; }
            }
            if (!placed) { tk_v[0] = y; tk_i[0] = col; }
        }
    };
    static_assert(!(SMP && NORM), "EPI_SAMPLE has no fused-norm form");
    static_assert(!(TGT && NORM), "EPI_TARGET has no fused-norm form");
    [[maybe_unused]] int my_tgt = -1;                                         // EPI_TARGET: thread b < B holds env b's named column
    if constexpr (TGT) if (tid < B) my_tgt = p.tg.tgt[tid];
    float best = -INFINITY;                                                   // EPI_ARGMAX: thread b < B tracks env b (EPI_SAMPLE: the best z)
    int best_i = 0x7FFFFFFF;
    float lm = -INFINITY, ls = 0.0f;                                          // EPI_ARGMAX_LSE: env b's (max, sum exp(l - max)) over the workgroup's units
    [[maybe_unused]] float lt = 0.0f;                                         // EPI_*_ENT: env b's sum (l - max) exp(l - max) beside ls
    [[maybe_unused]] float best_raw = -INFINITY;                              // EPI_SAMPLE: the y of the best z
    // EPI_SAMPLE: thread r * B + b evaluates the noise of column n0 + r for env b (one Philox per thread and unit); thread b reads its R values
    [[maybe_unused]] __shared__ float gn[SMP ? R * B : 1];
    [[maybe_unused]] int smp_stream = 0, smp_draw = 0;
    if constexpr (SMP) if (tid < R * B) { smp_stream = p.smp.stream[tid % B]; smp_draw = p.smp.draw[tid % B]; }
    for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
        const T* rows[R];
        int n0;
        if (EPI == EPI_SWIGLU) {          // outputs j0 .. j0+R/2-1: rows (gate j, up j) pairs of the [gate 32 | up 32] packing
            const int j0 = u * (R / 2);
            n0 = j0;
#pragma unroll
            for (int o = 0; o < R / 2; ++o) {
                const size_t gr = swiglu_gate_row(j0 + o);
                rows[2 * o] = W + gr * p.ldw;
                rows[2 * o + 1] = W + (gr + 32) * p.ldw;
            }
        } else {
            n0 = u * R;
#pragma unroll
            for (int r = 0; r < R; ++r) rows[r] = W + (size_t)min(n0 + r, p.N - 1) * p.ldw;
        }
        float acc[R][B], ss[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            ss[b] = 0.0f;
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][b] = 0.0f;
        }
        for (int ci = wave * 64 + lane; ci < nch; ci += STRIDE) {
            uint4 w[R], xr[B];
#pragma unroll
            for (int r = 0; r < R; ++r) w[r] = load_nt(rows[r] + (size_t)ci * EPC);
#pragma unroll
            for (int b = 0; b < B; ++b) xr[b] = *(const uint4*)(xg + (size_t)b * p.ldx + (size_t)ci * EPC);
            if (sizeof(T) == 2 && !NORM) {
                // bf16: packed dot products straight on the bf16 pairs (v_dot2c_f32_bf16), no conversions
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    const unsigned xw[4] = {xr[b].x, xr[b].y, xr[b].z, xr[b].w};
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const unsigned ww[4] = {w[r].x, w[r].y, w[r].z, w[r].w};
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            acc[r][b] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, ww[q]), __builtin_bit_cast(bf16x2_t, xw[q]),
                                                                        acc[r][b], false);
                    }
                }
            } else {
                float gf[EPC];
                if (NORM) chunk_to_f32<T>(*(const uint4*)(gg + (size_t)ci * EPC), gf);
                float wf[R][EPC];
#pragma unroll
                for (int r = 0; r < R; ++r) chunk_to_f32<T>(w[r], wf[r]);
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    float xf[EPC];
                    chunk_to_f32<T>(xr[b], xf);
                    if (NORM) {
#pragma unroll
                        for (int e = 0; e < EPC; ++e) { ss[b] = fmaf(xf[e], xf[e], ss[b]); xf[e] *= gf[e]; }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int e = 0; e < EPC; ++e) acc[r][b] = fmaf(wf[r][e], xf[e], acc[r][b]);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (NORM) ss[b] = wave_sum(ss[b]);
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][b] = wave_sum(acc[r][b]);
        }
        if constexpr (SMP) if (tid < R * B) gn[tid] = gumbel_noise(p.smp.seed_lo, p.smp.seed_hi, smp_stream, smp_draw, u * R + tid / B);
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < B; ++b) {
                part[wave][R * B + b] = ss[b];
#pragma unroll
                for (int r = 0; r < R; ++r) part[wave][r * B + b] = acc[r][b];
            }
        }
        __syncthreads();
        auto total = [&](int k) { return part[0][k] + part[1][k] + part[2][k] + part[3][k]; };
        if (EPI == EPI_SWIGLU) {
            if (tid < (R / 2) * B) {
                const int o = tid / B, b = tid % B;
                const float sc = NORM ? rsqrtf(total(R * B + b) / (float)p.K + p.eps) : 1.0f;
                const float gt = total((2 * o) * B + b) * sc, up = total((2 * o + 1) * B + b) * sc;
                ((T*)p.y)[(size_t)b * p.ldy + n0 + o] = from_f32<T>(silu_f(gt) * up);
            }
        } else if (AMAX) {
            if (tid < B) {
                const uint8_t* fl = p.pen_flags ? p.pen_flags + (size_t)p.pen_rows[tid] * p.N : nullptr;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float v = total(r * B + tid);
                    if (fl && n0 + r < p.N && fl[n0 + r]) v = v < 0.0f ? v * p.pen : v / p.pen;
                    if constexpr (TGT) {
                        // y = fl(v * inv_t) (inv_t == 1.0f: v itself), then the scored form's compares and sums on y; the one thread of the
                        // grid that meets column tgt[b] -- a unit belongs to one workgroup, row b to thread b -- stores it (-1 meets none)
                        v *= p.tg.inv_t;
                        if (n0 + r < p.N && n0 + r == my_tgt) p.tg.tgt_val[tid] = v;
                    }
                    if constexpr (SMP) {
                        const float y = v * p.smp.inv_t, z = __fadd_rn(y, gn[r * B + tid]);       // (fl(y + G), as in gemv_rows_kernel)
                        if (n0 + r < p.N) {
                            if (z > best) { best = z; best_i = n0 + r; best_raw = y; }
                            if constexpr (ENT) ent_add(y, lm, ls, lt); else lse_add(y, lm, ls);
                            tk_insert(y, n0 + r);
                        }
                        continue;
                    }
                    if (n0 + r < p.N && v > best) { best = v; best_i = n0 + r; }      // units ascend per workgroup: first max wins
                    // (the clamped rows of the last unit count once.  The arg-max ignores a fused norm's positive row factor, as the plain
                    // form does; a probability cannot: the SUM takes fl(v * factor), whose maximum is fl(best * factor) -- rounding is
                    // monotone -- so the final kernel rebuilds the partial's maximum from part_val and row_scale[b])
                    if constexpr (ENT) { if (n0 + r < p.N) ent_add(v, lm, ls, lt); }
                    else if (LSE && n0 + r < p.N) lse_add(NORM ? v * rsqrtf(total(R * B + tid) / (float)p.K + p.eps) : v, lm, ls);
                    if (TOPK && n0 + r < p.N) tk_insert(v, n0 + r);
                }
            }
        } else if (tid < R * B) {
            const int r = tid / B, b = tid % B, n = n0 + r;
            if (n < p.N) {
                float v = total(r * B + b);
                if (NORM) v *= rsqrtf(total(R * B + b) / (float)p.K + p.eps);
                if (p.bias) v += to_f32(((const T*)p.bias)[n]);
                if (p.res) v += to_f32(((const T*)p.res)[(size_t)b * p.ldr + n]);
                ((T*)p.y)[(size_t)b * p.ldy + n] = from_f32<T>(v);
            }
        }
        __syncthreads();
    }
    if (AMAX && tid < B) {
        p.part_val[(size_t)tid * gridDim.x + blockIdx.x] = best;
        p.part_idx[(size_t)tid * gridDim.x + blockIdx.x] = best_i;
        if constexpr (TOPK) {
#pragma unroll
            for (int e = 0; e < TOPK_C; ++e) {
                p.cand_val[((size_t)tid * gridDim.x + blockIdx.x) * TOPK_C + e] = tk_v[e];
                p.cand_idx[((size_t)tid * gridDim.x + blockIdx.x) * TOPK_C + e] = tk_i[e];
            }
        }
        if constexpr (ENT) p.part_ent[(size_t)tid * gridDim.x + blockIdx.x] = lt;
        if constexpr (SMP) {
            p.part_sum[(size_t)tid * gridDim.x + blockIdx.x] = ls;
            p.smp.part_max[(size_t)tid * gridDim.x + blockIdx.x] = lm;
            p.smp.part_raw[(size_t)tid * gridDim.x + blockIdx.x] = best_raw;
        }
        if (LSE) {
            p.part_sum[(size_t)tid * gridDim.x + blockIdx.x] = ls;
            // every workgroup computes the same factor from the same sums in the same order: workgroup 0 publishes it
            if (NORM && blockIdx.x == 0) p.row_scale[tid] = rsqrtf((part[0][R * B + tid] + part[1][R * B + tid] + part[2][R * B + tid] + part[3][R * B + tid]) / (float)p.K + p.eps);
        }
    }
}

// (block_sum_256, sample_merge, row_argmax_256, row_lse_sum_256 -- the merges of one row's partials on 256 threads -- live in common.h:
// topk_merge_kernel of misc.hip computes its (V, S) through them too)

// final arg-max of env b = blockIdx.x over its per-workgroup partials
// LSE: also env b's log-probability of that token from its partial sums ps (NaN for token -1); rs (optional): the positive factor of
// row b by which the producer scaled the logits it summed (a fused norm), so that partial k's maximum there is fl(pv[k] * rs[b])
// SMP (with LSE): the EPI_SAMPLE merge -- the token on (pv, pi) as before; its y from pr of the partial that owns it; the log-sum-exp on
// (pm, ps); score = y - V - log S
template <bool LSE, bool SMP = false>
__global__ __launch_bounds__(256) void argmax_final_batched_kernel(const float* pv, const int* pi, int n, int* out_tokens, const float* ps,
                                                                   float* scores, const float* rs, const float* pr = nullptr,
                                                                   const float* pm = nullptr) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const float* v0 = pv + (size_t)blockIdx.x * n;
    const int* i0 = pi + (size_t)blockIdx.x * n;
    row_argmax_256(v0, i0, n, sv, si);
    if (threadIdx.x == 0) out_tokens[blockIdx.x] = si[0] == 0x7FFFFFFF ? -1 : si[0];    // no finite logit: -1 (in-range for the next gather, an error on the host)
    if constexpr (SMP) {
        const int tok = si[0];
        const size_t o = (size_t)blockIdx.x * n;
        const SampleMerge mg = sample_merge(pi + o, pr + o, pm + o, ps + o, n, tok, sv, si);
        if (threadIdx.x == 0) scores[blockIdx.x] = tok == 0x7FFFFFFF ? __builtin_nanf("") : mg.raw - mg.V + lse_logprob(mg.S);
        return;
    }
    if (LSE) {
        const float sc = rs ? rs[blockIdx.x] : 1.0f;
        const float V = sv[0] * sc;
        const int tok = si[0];
        const float S = row_lse_sum_256(ps + (size_t)blockIdx.x * n, v0, n, sc, V, sv);
        if (threadIdx.x == 0) scores[blockIdx.x] = tok == 0x7FFFFFFF ? __builtin_nanf("") : lse_logprob(S);
    }
}

// EPI_TARGET merge of row b = blockIdx.x: argmax_final_batched_kernel<true>'s arg-max and (V, S) through the two helpers above (so
// greedy_ids / greedy_logprobs are that kernel's bits), then the named column's score from the captured y: (tgt_val - V) - log S.
// tgt[b] < 0: NaN, tgt_val[b] is not read.  A NaN y gives NaN, a -inf y gives -inf (V is finite or the row is NaN already).
__global__ __launch_bounds__(256) void target_final_batched_kernel(const float* pv, const int* pi, const float* ps, int n, const int* tgt,
                                                                   const float* tgt_val, int* greedy_ids, float* greedy_logprobs, float* logprobs) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const float* v0 = pv + (size_t)blockIdx.x * n;
    const int* i0 = pi + (size_t)blockIdx.x * n;
    row_argmax_256(v0, i0, n, sv, si);
    const float V = sv[0];
    const int tok = si[0];
    const float S = row_lse_sum_256(ps + (size_t)blockIdx.x * n, v0, n, 1.0f, V, sv);       // (factor 1: v0[k] * 1.0f is v0[k])
    if (threadIdx.x == 0) {
        const float lp = lse_logprob(S), nan = __builtin_nanf("");
        greedy_ids[blockIdx.x] = tok == 0x7FFFFFFF ? -1 : tok;
        greedy_logprobs[blockIdx.x] = tok == 0x7FFFFFFF ? nan : lp;
        const int t = tgt[blockIdx.x];
        // (t - V) - log S written as -(log S - (t - V)): the same rounding, and with t == V it is lp to the sign of a zero (S == 1: -0)
        logprobs[blockIdx.x] = t < 0 || tok == 0x7FFFFFFF ? nan : -(-lp - (tgt_val[blockIdx.x] - V));
    }
}

// per-row e4m3 quantisation: one workgroup per row, scale = max|w| / 448 floored at 2^-126 (1 for an all-zero row), round-to-nearest-even;
// a NaN element gives a NaN byte and leaves the scale alone (e4m3_row_scale / e4m3_clamp, common.h)
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const bf16* w, int ld, uint8_t* q, float* scale, int cols) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    const bf16* wr = w + row * ld;
    float amax = 0.0f;
    for (int ci = threadIdx.x; ci < cols / 8; ci += 256) {
        float f[8];
        chunk_to_f32<bf16>(*(const uint4*)(wr + (size_t)ci * 8), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
    }
    amax = wave_max(amax);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = e4m3_row_scale(amax);
    if (threadIdx.x == 0) scale[row] = sc;
    const float inv = 1.0f / sc;
    for (int ci = threadIdx.x; ci < cols / 8; ci += 256) {
        float f[8];
        chunk_to_f32<bf16>(*(const uint4*)(wr + (size_t)ci * 8), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = e4m3_clamp(f[e] * inv);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        *(uint2*)(q + row * cols + (size_t)ci * 8) = make_uint2((unsigned)lo, (unsigned)hi);
    }
}

// MXFP4 quantisation of a bf16 matrix (OCP MX conversion): one workgroup per row, one thread per block of 32 elements.
//   e = floor(log2(max |w|)) - 2 clamped to [-127, 127] (0 for an all-zero block), scale byte e + 127;
//   code = E2M1 of w / 2^e (exact in fp32), round to nearest even, saturating at 6.
// A block that holds a NaN or an infinity gets the scale byte 0xFF (E8M0 NaN, as the OCP MX conversion prescribes); its codes are unspecified.
// The rounding is written as comparisons against the seven midpoints of the grid (ties to the code with an even mantissa bit) rather
// than with v_cvt_scalef32_pk_fp4_f32: this runs once per weight load, and the bytes are then defined by this text alone.
SVLN_DEV unsigned e2m1_code(float v) {
    const float a = fabsf(v);
    const unsigned c = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) + (unsigned)(a >= 1.75f) + (unsigned)(a > 2.5f) +
                       (unsigned)(a >= 3.5f) + (unsigned)(a > 5.0f);
    return c | (v < 0.0f ? 8u : 0u);
}
__global__ __launch_bounds__(256) void quant_mxfp4_rows_kernel(const bf16* w, int ld, uint8_t* q, uint8_t* e8, int cols) {
    const size_t row = blockIdx.x;
    const bf16* wr = w + row * ld;
    const int nblk = cols / 32;
    for (int bi = threadIdx.x; bi < nblk; bi += 256) {
        float f[32];
#pragma unroll
        for (int h = 0; h < 4; ++h) chunk_to_f32<bf16>(*(const uint4*)(wr + (size_t)bi * 32 + h * 8), f + 8 * h);
        float amax = 0.0f;
        bool nonfinite = false;
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            const float a = fabsf(f[e]);
            amax = fmaxf(amax, a);
            nonfinite |= !(a < __builtin_inff());           // NaN or inf
        }
        int ex = 0;
        if (amax > 0.0f) {
            ex = (int)((__float_as_uint(amax) >> 23) & 0xFF) - 127 - 2;        // (a subnormal amax reads as -129 and clamps)
            ex = ex < -127 ? -127 : ex > 127 ? 127 : ex;
        }
        unsigned d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned v = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) v |= e2m1_code(ldexpf(f[8 * k + e], -ex)) << (4 * e);
            d[k] = v;
        }
        *(uint4*)(q + row * (size_t)(cols / 2) + (size_t)bi * 16) = make_uint4(d[0], d[1], d[2], d[3]);
        e8[row * (size_t)nblk + bi] = nonfinite ? (uint8_t)0xFF : (uint8_t)(ex + 127);
    }
}

// P12 encoder (format: WP12 above): one workgroup per row.  Histogram of hi7 in LDS; bin i's rank = the bins that beat it (greater count,
// or the same count and a lower value); ranks 0 .. 7 with a non-zero count are the table; then wave w packs blocks w, w + 4, ...: a
// block with a miss anywhere (wave vote) sets its mask bit, writes zeros and counts into *fb_count (one atomic per row).
__global__ __launch_bounds__(256) void p12_pack_rows_kernel(const bf16* w, int ld, uint8_t* packed, uint8_t* rec, unsigned* fb_count, int cols) {
    __shared__ unsigned hist[128];
    __shared__ unsigned char code[128];
    __shared__ unsigned tab[8], mask[2], nfb;
    const size_t row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = cols / 8, nblk = (cols + 511) / 512;
    const bf16* wr = w + row * ld;
    uint8_t* pr = packed + row * p12_row_bytes(cols);
    if (tid < 128) hist[tid] = 0;
    if (tid < 8) tab[tid] = 0xFFFFFFFFu;
    if (tid < 2) mask[tid] = 0;
    if (tid == 0) nfb = 0;
    __syncthreads();
    for (int ci = tid; ci < nch; ci += 256) {
        const uint4 v = *(const uint4*)(wr + (size_t)ci * 8);
        const unsigned d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) { atomicAdd(&hist[(d[q] >> 8) & 0x7F], 1u); atomicAdd(&hist[(d[q] >> 24) & 0x7F], 1u); }
    }
    __syncthreads();
    if (tid < 128 && hist[tid] > 0) {
        int rank = 0;
        for (int j = 0; j < 128; ++j) rank += hist[j] > hist[tid] || (hist[j] == hist[tid] && j < tid);
        if (rank < 8) tab[rank] = (unsigned)tid;
    }
    __syncthreads();
    if (tid == 0)                                   // fewer than eight distinct values: the last entry repeats (entry 0 exists: cols >= 8)
        for (int j = 1; j < 8; ++j) if (tab[j] == 0xFFFFFFFFu) tab[j] = tab[j - 1];
    __syncthreads();
    if (tid < 128) {
        unsigned c = 0xFF;
        for (int j = 7; j >= 0; --j) if (tab[j] == (unsigned)tid) c = (unsigned)j;      // the lowest j of a repeated entry
        code[tid] = (unsigned char)c;
    }
    __syncthreads();
    for (int blk = wave; blk < nblk; blk += 4) {
        const int ci = blk * 64 + lane;
        unsigned lo0 = 0, lo1 = 0, cd = 0;
        bool miss = false;
        if (ci < nch) {
            const uint4 v = *(const uint4*)(wr + (size_t)ci * 8);
            const unsigned d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned b = (d[e / 2] >> (16 * (e % 2))) & 0xFFFFu;
                const unsigned c = code[(b >> 8) & 0x7F];
                miss |= c == 0xFF;
                if (e < 4) lo0 |= (b & 0xFF) << (8 * e); else lo1 |= (b & 0xFF) << (8 * (e - 4));
                cd |= (((b >> 15) << 3) | (c & 7)) << (8 * (e & 3) + 4 * (e >> 2));
            }
        }
        const bool fb = __ballot(miss) != 0;
        if (fb) { lo0 = lo1 = cd = 0; }
        *(uint2*)(pr + (size_t)blk * 768 + 8 * lane) = make_uint2(lo0, lo1);
        *(unsigned*)(pr + (size_t)blk * 768 + 512 + 4 * lane) = cd;
        if (fb && lane == 0) { atomicOr(&mask[blk >> 5], 1u << (blk & 31)); atomicAdd(&nfb, 1u); }
    }
    __syncthreads();
    if (tid == 0) {
        *(uint4*)(rec + row * 16) = make_uint4(tab[0] | tab[1] << 8 | tab[2] << 16 | tab[3] << 24, tab[4] | tab[5] << 8 | tab[6] << 16 | tab[7] << 24,
                                               mask[0], mask[1]);
        if (fb_count && nfb) atomicAdd(fb_count, nfb);
    }
}
// TEST-ONLY: the bf16 rows a P12 matrix stands for -- p12_decode on the packed blocks, the bf16 original on the fallback blocks
__global__ __launch_bounds__(256) void p12_unpack_rows_kernel(const uint8_t* packed, const uint8_t* rec, const bf16* w, int ld, bf16* out, int ldo,
                                                              int cols) {
    const size_t row = blockIdx.x;
    const uint4 r = *(const uint4*)(rec + row * 16);
    const uint8_t* pr = packed + row * p12_row_bytes(cols);
    for (int ci = threadIdx.x; ci < cols / 8; ci += 256) {
        const int blk = ci >> 6, l = ci & 63;
        uint4 v;
        if ((((blk & 32) ? r.w : r.z) >> (blk & 31)) & 1u) {
            v = *(const uint4*)(w + row * ld + (size_t)ci * 8);
        } else {
            const uint2 lo = *(const uint2*)(pr + (size_t)blk * 768 + 8 * l);
            v = p12_decode(lo.x, lo.y, *(const unsigned*)(pr + (size_t)blk * 768 + 512 + 4 * l), r.x, r.y);
        }
        *(uint4*)(out + row * ldo + (size_t)ci * 8) = v;
    }
}

// final arg-max over per-workgroup partials: greatest value, lowest index on ties (torch.argmax on CPU)
// With `ctl` it is also one step of the greedy loop (GenerationMixin._sample: append, stop on EOS / max_new_tokens): see GenCtl.
// LSE: also the token's log-probability from the partial sums ps, to scores[ctl->count] before the count advances (scores[0] without ctl)
// SMP (with LSE): the EPI_SAMPLE merge (sample_merge) instead: score = y of the token - V - log S
template <bool LSE, bool SMP = false>
__global__ __launch_bounds__(256) void argmax_final_kernel(const float* pv, const int* pi, int n, int* out_token, float* out_top, GenCtl* ctl,
                                                           const int* eos, int* out_ids, uint8_t* pen_flags, const float* ps, float* scores,
                                                           const float* pr = nullptr, const float* pm = nullptr) {
    __shared__ float sv[256];
    if (ctl && ctl->done) return;
    __shared__ int si[256];
    __shared__ float s2[256];
    float v = -INFINITY, v2 = -INFINITY;
    int i = 0x7FFFFFFF;
    for (int k = threadIdx.x; k < n; k += 256) {
        const float c = pv[k];
        const int ci = pi[k];
        if (c > v || (c == v && ci < i)) { v2 = v; v = c; i = ci; } else if (c > v2) v2 = c;
    }
    sv[threadIdx.x] = v; si[threadIdx.x] = i; s2[threadIdx.x] = v2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float a = sv[threadIdx.x], b = sv[threadIdx.x + s];
            const int ai = si[threadIdx.x], bi = si[threadIdx.x + s];
            const float a2 = s2[threadIdx.x], b2 = s2[threadIdx.x + s];
            if (b > a || (b == a && bi < ai)) { sv[threadIdx.x] = b; si[threadIdx.x] = bi; s2[threadIdx.x] = fmaxf(a, b2); }
            else s2[threadIdx.x] = fmaxf(a2, b);
        }
        __syncthreads();
    }
    const int tok = si[0] == 0x7FFFFFFF ? -1 : si[0];      // no finite logit (NaN / -inf everywhere): -1, which the next embedding gather
                                                           // reads as frame-feature row 0 (in range) and the host reports as an error
    if (threadIdx.x == 0) {
        *out_token = tok;
        if (out_top) { out_top[0] = sv[0]; out_top[1] = s2[0]; }
    }
    if constexpr (SMP) {
        const SampleMerge mg = sample_merge(pi, pr, pm, ps, n, si[0], s2, si);
        if (threadIdx.x == 0) scores[ctl ? ctl->count : 0] = tok < 0 ? __builtin_nanf("") : mg.raw - mg.V + lse_logprob(mg.S);
    } else if (LSE) {
        const float V = sv[0];
        __syncthreads();                          // sv / s2 have been read: s2 is reused by the sum
        float mine = 0.0f;
        for (int k = threadIdx.x; k < n; k += 256) mine += lse_rescale(ps[k], pv[k], V);
        const float S = block_sum_256(mine, s2);
        if (threadIdx.x == 0) scores[ctl ? ctl->count : 0] = tok < 0 ? __builtin_nanf("") : lse_logprob(S);
    }
    if (ctl) {
        int hit = 0;
        for (int k = threadIdx.x; k < ctl->n_eos; k += 256) hit |= eos[k] == tok;
        hit = __syncthreads_or(hit);
        if (threadIdx.x == 0) {
            const int c = ctl->count;
            out_ids[c] = tok;
            if (pen_flags && tok >= 0) pen_flags[tok] = 1;
            ctl->count = c + 1;
            if (hit || tok < 0 || c + 1 >= ctl->max_new) ctl->done = 1;      // EOS is appended, never fed
            else { ctl->pos += 1; ctl->kv_len += 1; }
        }
    }
}

}  // namespace

int gemv_grid(int N) {
    // wave-per-4-rows kernel: 4 row groups per workgroup iteration.  Prefer a grid (<= 1280 workgroups, ~5 per CU)
    // that divides the row groups evenly so no wave runs an extra iteration (9472 groups -> 1184 workgroups x 2).
    const int groups = (N + 3) / 4;
    const int wg_groups = (groups + GEMV_WAVES - 1) / GEMV_WAVES;       // workgroup-iterations needed
    if (wg_groups <= 1280) return wg_groups < 1 ? 1 : wg_groups;
    if (wg_groups > 4 * 1280) return 1024;          // many iterations per wave (lm_head): imbalance is negligible, 1024 measured best
    if (groups % GEMV_WAVES == 0)
        for (int g = 1280; g >= 640; --g)
            if (wg_groups % g == 0) return g;
    return 1024;
}

template <typename T> void launch_gemv(hipStream_t s, const GemvArgs& a) { launch_gemv_timed<T>(s, a, nullptr, nullptr); }

// start/stop (optional) receive the kernel's own begin/end timestamps (hipExtLaunchKernelGGL)
#define SVLN_LAUNCH(kern, grid, block, lds)                                                        \
    do {                                                                                          \
        if (start || stop) hipExtLaunchKernelGGL(kern, grid, block, lds, s, start, stop, 0, a);   \
        else hipLaunchKernelGGL(kern, grid, block, lds, s, a);                                    \
    } while (0)
template <typename P, int KW> static void launch_ksplit(hipStream_t s, const GemvArgs& a, hipEvent_t start, hipEvent_t stop) {
    const int per_wg = P::KS_R * (GEMV_WAVES / KW);
    int grid = (a.N + per_wg - 1) / per_wg;
    if (grid > 2048) grid = 2048;
    if (a.norm_w) SVLN_LAUNCH((gemv_ksplit_kernel<P, true, KW>), dim3(grid), dim3(GEMV_THREADS), 0);
    else SVLN_LAUNCH((gemv_ksplit_kernel<P, false, KW>), dim3(grid), dim3(GEMV_THREADS), 0);
}
template <typename P> static void launch_gemv_fmt(hipStream_t s, const GemvArgs& a, hipEvent_t start, hipEvent_t stop) {
    if (a.epi == EPI_NONE && a.N <= 8192) {
        // a row of more than 128 chunks (K > 4096 for MXFP4, the only format that asks) gives all four waves a share of K
        if (a.K > 4096) launch_ksplit<P, GEMV_WAVES>(s, a, start, stop);
        else launch_ksplit<P, P::KS_KW_NARROW>(s, a, start, stop);
        return;
    }
    const size_t lds = (size_t)a.K * sizeof(float);
    dim3 g(gemv_grid(a.N)), b(GEMV_THREADS);
    // (the arg-max forms keep gemv_grid: the number of partials is part of their contract with the final kernels)
    if (P::ROWS_GRID_CAP && !epi_is_argmax(a.epi) && g.x > (unsigned)P::ROWS_GRID_CAP) g.x = P::ROWS_GRID_CAP;
    if (a.epi == EPI_NONE) SVLN_LAUNCH((gemv_rows_kernel<P, EPI_NONE>), g, b, lds);
    else if (a.epi == EPI_SWIGLU) SVLN_LAUNCH((gemv_rows_kernel<P, EPI_SWIGLU>), g, b, lds);
    else with_head_epi<GEMV_ROWS_EPIS>(a.epi, [&](auto e) { SVLN_LAUNCH((gemv_rows_kernel<P, decltype(e)::value>), g, b, lds); });
}
#undef SVLN_LAUNCH
template <typename T> void launch_gemv_timed(hipStream_t s, const GemvArgs& a, hipEvent_t start, hipEvent_t stop) {
    // (MXFP4 / e4m3 weights: bf16 engine only; the engine refuses to enable them otherwise)
    if (a.w4) launch_gemv_fmt<WMxfp4>(s, a, start, stop);
    else if (a.w8) launch_gemv_fmt<WE4m3>(s, a, start, stop);
    else if (a.wp) launch_gemv_fmt<WP12>(s, a, start, stop);        // (bf16 engine only too: W / ldw stay the bf16 original)
    else launch_gemv_fmt<WPlain<T>>(s, a, start, stop);
}
int gemv_batched_grid(int N, int epi, int B) {
    const int R = 4;
    (void)B;
    const int units = epi == EPI_SWIGLU ? N / R : (N + R - 1) / R;
    return units < 2048 ? (units < 1 ? 1 : units) : 2048;
}
template <typename T, int EPI, bool NORM> static void launch_gb(hipStream_t s, const GemvBatchArgs& a) {
    dim3 g(gemv_batched_grid(a.N, EPI, a.B)), b(GEMV_THREADS);
    switch (a.B) {
        case 1: hipLaunchKernelGGL((gemv_batched_kernel<T, EPI, NORM, 1>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((gemv_batched_kernel<T, EPI, NORM, 2>), g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL((gemv_batched_kernel<T, EPI, NORM, 4>), g, b, 0, s, a); break;
        case 8: hipLaunchKernelGGL((gemv_batched_kernel<T, EPI, NORM, 8>), g, b, 0, s, a); break;
        default: break;
    }
}
template <typename T> void launch_gemv_batched(hipStream_t s, const GemvBatchArgs& a) {
    const bool norm = a.norm_w != nullptr;
    if (a.epi == EPI_NONE) { if (norm) launch_gb<T, EPI_NONE, true>(s, a); else launch_gb<T, EPI_NONE, false>(s, a); return; }
    if (a.epi == EPI_SWIGLU) { if (norm) launch_gb<T, EPI_SWIGLU, true>(s, a); else launch_gb<T, EPI_SWIGLU, false>(s, a); return; }
    // the refusals of the arg-max forms: after them a fused norm meets a form that has it (gemv_batched_norm_has)
    const HeadForm f = head_form(a.epi);
    if (f.topk && (norm || !a.cand_val || !a.cand_idx)) throw std::runtime_error("batched GEMV: EPI_*_TOPK takes candidate arrays and no fused norm");
    if (f.ent && (norm || !a.part_ent)) throw std::runtime_error("batched GEMV: EPI_*_ENT takes part_ent and no fused norm");
    if (f.tgt && (norm || a.pen_flags || !a.tg.tgt || !a.tg.tgt_val)) throw std::runtime_error("batched GEMV: EPI_TARGET takes targets, no fused norm and no penalty flags");
    if (f.smp && norm) throw std::runtime_error("batched GEMV: EPI_SAMPLE has no fused-norm form");
    with_head_epi<GEMV_BATCHED_EPIS>(a.epi, [&](auto e) {
        constexpr int E = decltype(e)::value;
        if constexpr (gemv_batched_norm_has(E)) if (norm) return launch_gb<T, E, true>(s, a);
        launch_gb<T, E, false>(s, a);
    });
}
template void launch_gemv_batched<bf16>(hipStream_t, const GemvBatchArgs&);
template void launch_gemv_batched<float>(hipStream_t, const GemvBatchArgs&);
void launch_argmax_final_batched(hipStream_t s, const float* pv, const int* pi, int n, int B, int* out_tokens, const float* ps, float* scores,
                                 const float* rs, const float* pr, const float* pm) {
    if (pr) hipLaunchKernelGGL((argmax_final_batched_kernel<true, true>), dim3(B), dim3(256), 0, s, pv, pi, n, out_tokens, ps, scores, rs, pr, pm);
    else if (ps) hipLaunchKernelGGL((argmax_final_batched_kernel<true, false>), dim3(B), dim3(256), 0, s, pv, pi, n, out_tokens, ps, scores, rs, pr, pm);
    else hipLaunchKernelGGL((argmax_final_batched_kernel<false, false>), dim3(B), dim3(256), 0, s, pv, pi, n, out_tokens, ps, scores, rs, pr, pm);
}
void launch_target_final_batched(hipStream_t s, const float* pv, const int* pi, const float* ps, int n, int B, const int* tgt, const float* tgt_val,
                                 int* greedy_ids, float* greedy_logprobs, float* logprobs) {
    hipLaunchKernelGGL(target_final_batched_kernel, dim3(B), dim3(256), 0, s, pv, pi, ps, n, tgt, tgt_val, greedy_ids, greedy_logprobs, logprobs);
}
template void launch_gemv_timed<bf16>(hipStream_t, const GemvArgs&, hipEvent_t, hipEvent_t);
template void launch_gemv_timed<float>(hipStream_t, const GemvArgs&, hipEvent_t, hipEvent_t);
void launch_quant_fp8_rows(hipStream_t s, const void* w_bf16, int ld, void* w8, float* scale, int64_t rows, int cols) {
    hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, (const bf16*)w_bf16, ld, (uint8_t*)w8, scale, cols);
}
void launch_quant_mxfp4_rows(hipStream_t s, const void* w_bf16, int ld, void* q4, uint8_t* e8, int64_t rows, int cols) {
    hipLaunchKernelGGL(quant_mxfp4_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, (const bf16*)w_bf16, ld, (uint8_t*)q4, e8, cols);
}
void launch_p12_pack_rows(hipStream_t s, const void* w_bf16, int ld, void* packed, void* rec, unsigned* fb_count, int64_t rows, int cols) {
    hipLaunchKernelGGL(p12_pack_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, (const bf16*)w_bf16, ld, (uint8_t*)packed, (uint8_t*)rec, fb_count, cols);
}
void launch_p12_unpack_rows(hipStream_t s, const void* packed, const void* rec, const void* w_bf16, int ld, void* out, int ldo, int64_t rows, int cols) {
    hipLaunchKernelGGL(p12_unpack_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, (const uint8_t*)packed, (const uint8_t*)rec, (const bf16*)w_bf16, ld,
                       (bf16*)out, ldo, cols);
}
// (every kernel that may ask for more than 64 KiB of dynamic LDS goes through set_max_lds: a refusal is reported at engine creation)
template <typename P> static void gemv_rows_attrs() {
    set_max_lds((const void*)gemv_rows_kernel<P, EPI_NONE>, GEMV_ROWS_MAX_LDS);
    set_max_lds((const void*)gemv_rows_kernel<P, EPI_SWIGLU>, GEMV_ROWS_MAX_LDS);
    for_each_head_epi<GEMV_ROWS_EPIS>([](auto e) {
        constexpr int E = decltype(e)::value;
        set_max_lds((const void*)gemv_rows_kernel<P, E>, head_form(E).topk ? GEMV_ROWS_TOPK_MAX_LDS : GEMV_ROWS_MAX_LDS);
    });
}
void gemv_init_attrs() {
    gemv_rows_attrs<WMxfp4>(); gemv_rows_attrs<WE4m3>(); gemv_rows_attrs<WP12>(); gemv_rows_attrs<WPlain<bf16>>(); gemv_rows_attrs<WPlain<float>>();
}
template void launch_gemv<bf16>(hipStream_t, const GemvArgs&);
template void launch_gemv<float>(hipStream_t, const GemvArgs&);

void launch_argmax_step(hipStream_t s, const float* pv, const int* pi, int n, int* out_token, float* out_top, GenCtl* ctl, const int* eos,
                        int* out_ids, uint8_t* pen_flags, const float* ps, float* scores, const float* pr, const float* pm) {
    if (pr) hipLaunchKernelGGL((argmax_final_kernel<true, true>), dim3(1), dim3(256), 0, s, pv, pi, n, out_token, out_top, ctl, eos, out_ids, pen_flags, ps, scores, pr, pm);
    else if (ps) hipLaunchKernelGGL((argmax_final_kernel<true, false>), dim3(1), dim3(256), 0, s, pv, pi, n, out_token, out_top, ctl, eos, out_ids, pen_flags, ps, scores, pr, pm);
    else hipLaunchKernelGGL((argmax_final_kernel<false, false>), dim3(1), dim3(256), 0, s, pv, pi, n, out_token, out_top, ctl, eos, out_ids, pen_flags, ps, scores, pr, pm);
}
void launch_argmax_final(hipStream_t s, const float* pv, const int* pi, int n, int* out_token, float* out_top, const float* ps, float* scores,
                         const float* pr, const float* pm) {
    launch_argmax_step(s, pv, pi, n, out_token, out_top, nullptr, nullptr, nullptr, nullptr, ps, scores, pr, pm);
}
namespace {
__global__ __launch_bounds__(256) void gumbel_kernel(uint32_t seed_lo, uint32_t seed_hi, int stream, int draw, int n0, int count, float* out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < count) out[k] = gumbel_noise(seed_lo, seed_hi, stream, draw, n0 + k);
}
}  // namespace
void launch_gumbel(hipStream_t s, uint32_t seed_lo, uint32_t seed_hi, int stream, int draw, int n0, int count, float* out) {
    hipLaunchKernelGGL(gumbel_kernel, dim3((count + 255) / 256), dim3(256), 0, s, seed_lo, seed_hi, stream, draw, n0, count, out);
}
namespace {
__global__ __launch_bounds__(256) void set_flags_kernel(uint8_t* flags, const int* ids, const int* count, int n_host, int value) {
    const int n = count ? *count : n_host;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256)
        if (ids[k] >= 0) flags[ids[k]] = (uint8_t)value;
}
}  // namespace
void launch_set_flags(hipStream_t s, uint8_t* flags, const int* ids, const int* count, int n_host, int value) {
    hipLaunchKernelGGL(set_flags_kernel, dim3(count ? 16 : (n_host + 255) / 256 > 0 ? (n_host + 255) / 256 : 1), dim3(256), 0, s, flags, ids, count, n_host, value);
}

}  // namespace svln
