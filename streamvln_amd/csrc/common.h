// Shared device helpers for the StreamVLN HIP engine (gfx950 / CDNA4 only).
//
// Every kernel is written once, generic over the storage type T in {bf16, float}:
//   * bf16  -- the shipping compute type (bf16 storage, fp32 accumulate, MFMA 32x32x16 bf16)
//   * float -- parity mode (fp32 storage, MFMA 32x32x2 f32 = exact fp32 fma chain), used to
//              meet the north-star tolerance (token ids identical, hidden states <= 1e-3)
//              against the fp32 CPU oracle.
// The common currency is the 16-byte chunk (uint4): 8 bf16 or 4 floats.  All row strides and
// K extents are multiples of one chunk, so staging / LDS layouts are byte-identical for both
// types and only the MFMA issue differs (mma_chunk below).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define SVLN_DEV __device__ __forceinline__
#define SVLN_HD __host__ __device__ __forceinline__        // also host code: the dealing logic of decode_layer_walk.h

struct fp8_t { uint8_t v; };        // OCP e4m3 storage (operands of the opt-in fp8 MFMA products; never an output type)
template <typename T> struct Elt;
template <> struct Elt<fp8_t> { static constexpr int PER_CHUNK = 16; static constexpr int BYTES = 1; };
template <> struct Elt<bf16> { static constexpr int PER_CHUNK = 8; static constexpr int BYTES = 2; };
template <> struct Elt<float> { static constexpr int PER_CHUNK = 4; static constexpr int BYTES = 4; };

SVLN_DEV float to_f32(bf16 v) { return (float)v; }
SVLN_DEV float to_f32(float v) { return v; }
template <typename T> SVLN_DEV T from_f32(float v);
template <> SVLN_DEV bf16 from_f32<bf16>(float v) { return (bf16)v; }    // v_cvt_pk_bf16_f32: RNE, NaN-safe
template <> SVLN_DEV float from_f32<float>(float v) { return v; }

SVLN_DEV uint4 zero_chunk() { return make_uint4(0u, 0u, 0u, 0u); }

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
// streaming (read-once) 16-byte load: non-temporal so weight bytes do not displace reusable lines
SVLN_DEV uint4 load_nt(const void* p) {
    const u32x4 v = __builtin_nontemporal_load((const u32x4*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// unpack one 16-byte chunk to floats (8 for bf16, 4 for float)
template <typename T> SVLN_DEV void chunk_to_f32(const uint4& c, float* out);
template <> SVLN_DEV void chunk_to_f32<bf16>(const uint4& c, float* out) {
    out[0] = __uint_as_float(c.x << 16); out[1] = __uint_as_float(c.x & 0xFFFF0000u);
    out[2] = __uint_as_float(c.y << 16); out[3] = __uint_as_float(c.y & 0xFFFF0000u);
    out[4] = __uint_as_float(c.z << 16); out[5] = __uint_as_float(c.z & 0xFFFF0000u);
    out[6] = __uint_as_float(c.w << 16); out[7] = __uint_as_float(c.w & 0xFFFF0000u);
}
template <> SVLN_DEV void chunk_to_f32<float>(const uint4& c, float* out) {
    out[0] = __uint_as_float(c.x); out[1] = __uint_as_float(c.y);
    out[2] = __uint_as_float(c.z); out[3] = __uint_as_float(c.w);
}

SVLN_DEV uint32_t pack_bf16x2(float lo, float hi) {
    bf16 a = (bf16)lo, b = (bf16)hi;
    return (uint32_t)__builtin_bit_cast(unsigned short, a) | ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
}

template <typename T> SVLN_DEV uint4 f32_to_chunk(const float* in);
template <> SVLN_DEV uint4 f32_to_chunk<bf16>(const float* in) {
    return make_uint4(pack_bf16x2(in[0], in[1]), pack_bf16x2(in[2], in[3]), pack_bf16x2(in[4], in[5]),
                      pack_bf16x2(in[6], in[7]));
}
template <> SVLN_DEV uint4 f32_to_chunk<float>(const float* in) {
    return make_uint4(__float_as_uint(in[0]), __float_as_uint(in[1]), __float_as_uint(in[2]), __float_as_uint(in[3]));
}

// One "macro" matrix step on 16-byte fragments.  Lane l = (r = l & 31, h = l >> 5) holds chunk
// (2s + h) of row r of both operands (K-contiguous rows: an NT product).
//   bf16 : one v_mfma_f32_32x32x16_bf16   (lane half h holds k = 8h + j, j = 0..7)
//   float: four v_mfma_f32_32x32x2_f32    (MFMA j pairs k = j [h=0] with k = 4 + j [h=1])
// D layout (both): col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
template <typename T> SVLN_DEV void mma_chunk(const uint4& a, const uint4& b, f32x16& acc);
template <> SVLN_DEV void mma_chunk<bf16>(const uint4& a, const uint4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
template <> SVLN_DEV void mma_chunk<float>(const uint4& a, const uint4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

// e4m3 operands: a 16-byte chunk holds 16 k values = two v_mfma_f32_32x32x16_fp8_fp8 (8 bytes per lane each); both operands use the
// same byte -> k assignment, so the products pair up correctly whatever the order inside the chunk.  Same rate as the bf16 MFMA,
// half the operand bytes per k.
template <> SVLN_DEV void mma_chunk<fp8_t>(const uint4& a, const uint4& b, f32x16& acc) {
    const long a0 = (long)(((unsigned long)a.y << 32) | a.x), a1 = (long)(((unsigned long)a.w << 32) | a.z);
    const long b0 = (long)(((unsigned long)b.y << 32) | b.x), b1 = (long)(((unsigned long)b.w << 32) | b.z);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a1, b1, acc, 0, 0, 0);
}

// The same e4m3 bytes on the block-scaled instructions (opt-in, svln_set_fp8_scaled_mfma): fp8s_t is the operand tag of that form.  A lane
// holds 32 bytes per operand -- for the 32x32x64 form the two chunks (2s + h) and (2(s + 1) + h) that lane half h reads for the macro
// steps s and s + 1 above, for the 16x16x128 form two chunks of lane group l >> 4 -- and again both operands use the same byte -> k
// assignment, so the products pair up whatever k order the instruction gives the 32 bytes.  Format selectors 0 = e4m3 (OCP e4m3fn); the
// E8M0 block scales are neutral (127 = 2^0 in every byte, opsel 0): the numeric scheme is that of mma_chunk<fp8_t>, at twice the rate.
// Accumulator layouts: 32x32 as acc_row below, 16x16 as v_mfma_f32_16x16x32_bf16.
struct fp8s_t { uint8_t v; };
template <> struct Elt<fp8s_t> { static constexpr int PER_CHUNK = 16; static constexpr int BYTES = 1; };
typedef __attribute__((ext_vector_type(8))) int i32x8;
constexpr int E8M0_ONE_X4 = 0x7f7f7f7f;
SVLN_DEV i32x8 frag32(const u32x4& lo, const u32x4& hi) {
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}
SVLN_DEV void mma_scaled_32x32x64(const i32x8& a, const i32x8& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 0, 0, 0, E8M0_ONE_X4, 0, E8M0_ONE_X4);
}
SVLN_DEV void mma_scaled_16x16x128(const i32x8& a, const i32x8& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0, E8M0_ONE_X4, 0, E8M0_ONE_X4);
}

SVLN_DEV int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

SVLN_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
SVLN_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The per-row e4m3 scheme shared by quant_fp8_rows_kernel (gemv.hip) and splitk_rownorm_kernel (gemm.hip).  amax = max |w| with fmaxf, so
// a NaN element does not enter it.  The scale is amax / 448 floored at 2^-126 (1 for an all-zero row): 1 / scale is then finite and
// normal, and a zero of a tiny row stays zero instead of 0 * inf.  A NaN element passes the clamp and becomes a NaN byte.
SVLN_DEV float e4m3_row_scale(float amax) { return amax > 0.0f ? fmaxf(amax / 448.0f, 0x1p-126f) : 1.0f; }
SVLN_DEV float e4m3_clamp(float x) { return x != x ? x : fminf(fmaxf(x, -448.0f), 448.0f); }

// Online log-sum-exp pieces of EPI_ARGMAX_LSE (kernels.h) on v_exp_f32 / v_log_f32.  A partial is (m, s): the maximum of the logits it
// owns and s = sum exp(l - m) over them; the partial that owns nothing is (-inf, 0).
SVLN_DEV float lse_exp(float d) { return __builtin_amdgcn_exp2f(1.4426950408889634f * d); }
// logit v joins (m, s): a new maximum rescales the sum (from m = -inf: 0 * 0 = 0); a -inf logit adds 0, not exp(-inf - -inf)
SVLN_DEV void lse_add(float v, float& m, float& s) {
    if (v > m) { s = fmaf(s, lse_exp(m - v), 1.0f); m = v; }
    else s += v == -INFINITY ? 0.0f : lse_exp(v - m);
}
// (m, s) seen from a maximum V >= m: s * exp(m - V); the empty partial is 0 whatever V is (a NaN sum stays NaN)
SVLN_DEV float lse_rescale(float s, float m, float V) { return s == 0.0f ? 0.0f : s * lse_exp(m - V); }
// log-probability of the winning logit from S = sum exp(l - V) >= 1
SVLN_DEV float lse_logprob(float S) { return -0.6931471805599453f * __builtin_amdgcn_logf(S); }
// Entropy pieces of the EPI_*_ENT forms (svln_token_entropy): a partial carries t = sum (l - m) exp(l - m) beside (m, s); the row's
// entropy is log S - T / S with T merged like S.  ent_term: one logit's share seen from m (a -inf logit adds 0, not -inf * 0; NaN stays).
SVLN_DEV float ent_term(float v, float m) { const float d = v - m; return v == -INFINITY ? 0.0f : d * lse_exp(d); }
// logit v joins (m, s, t): lse_add's own (m, s) update -- the same expressions, hence the same bits -- and t beside it.  A new maximum
// shifts t by (m - v) s before the rescale; the empty state stays t = 0 (not (-inf - v) * 0)
SVLN_DEV void ent_add(float v, float& m, float& s, float& t) {
    if (v > m) t = s == 0.0f ? 0.0f : (t + (m - v) * s) * lse_exp(m - v);
    else t += ent_term(v, m);
    lse_add(v, m, s);
}
// (m, s, t) seen from a maximum V >= m: the t beside lse_rescale(s, m, V); the empty partial is 0 whatever V is (a NaN sum stays NaN)
SVLN_DEV float ent_rescale(float t, float s, float m, float V) { return s == 0.0f ? 0.0f : (t + (m - V) * s) * lse_exp(m - V); }
// H = log S - T / S in nats
SVLN_DEV float ent_value(float S, float T) { return 0.6931471805599453f * __builtin_amdgcn_logf(S) - T / S; }

// ---- merges of one row's arg-max partials on a 256-thread workgroup (the final kernels of gemv.hip, topk_merge_kernel of misc.hip)
// S = sum over the 256 threads' shares `mine` of the rescaled partial sums, through `red` (a fixed tree: the same bits every launch)
SVLN_DEV float block_sum_256(float mine, float* red) {
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// EPI_SAMPLE merge of one row's n partials on 256 threads: raw = pr[k] of the partial with pi[k] == tok (unique; 0 when tok owns none),
// V = max_k pm[k], S = sum_k ps[k] * exp(pm[k] - V), all on fixed trees.  red / redi: 256 words each, free to overwrite; ends synchronised.
struct SampleMerge { float raw, V, S; };
SVLN_DEV SampleMerge sample_merge(const int* pi, const float* pr, const float* pm, const float* ps, int n, int tok, float* red, int* redi) {
    __syncthreads();                              // red / redi have been read by every thread
    float m = -INFINITY, raw = 0.0f;
    for (int k = threadIdx.x; k < n; k += 256) {
        m = pm[k] > m ? pm[k] : m;
        if (pi[k] == tok) raw = pr[k];
    }
    red[threadIdx.x] = m; redi[threadIdx.x] = __float_as_int(raw);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
            redi[threadIdx.x] |= redi[threadIdx.x + s];       // one thread holds the bits, the others 0
        }
        __syncthreads();
    }
    SampleMerge r;
    r.V = red[0]; r.raw = __int_as_float(redi[0]);
    __syncthreads();
    float mine = 0.0f;
    for (int k = threadIdx.x; k < n; k += 256) mine += lse_rescale(ps[k], pm[k], r.V);
    r.S = block_sum_256(mine, red);
    return r;
}

// The merge of one row's n partials on 256 threads, shared by argmax_final_batched_kernel and target_final_batched_kernel (one body: the
// two kernels' ids and sums are the same bits by construction).
// row_argmax_256: greatest value, lowest index on ties -> sv[0], si[0] (0x7FFFFFFF: no finite logit); ends synchronised.
SVLN_DEV void row_argmax_256(const float* v0, const int* i0, int n, float* sv, int* si) {
    float v = -INFINITY;
    int i = 0x7FFFFFFF;
    for (int k = threadIdx.x; k < n; k += 256) {
        const float c = v0[k];
        const int ci = i0[k];
        if (c > v || (c == v && ci < i)) { v = c; i = ci; }
    }
    sv[threadIdx.x] = v; si[threadIdx.x] = i;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (threadIdx.x < s2) {
            const float b = sv[threadIdx.x + s2];
            const int bi = si[threadIdx.x + s2];
            if (b > sv[threadIdx.x] || (b == sv[threadIdx.x] && bi < si[threadIdx.x])) { sv[threadIdx.x] = b; si[threadIdx.x] = bi; }
        }
        __syncthreads();
    }
}
// row_lse_sum_256: S = sum_k lse_rescale(ps[k], v0[k] * sc, V) on the fixed tree; sv must have been read by every thread's caller already
SVLN_DEV float row_lse_sum_256(const float* ps, const float* v0, int n, float sc, float V, float* sv) {
    __syncthreads();                          // sv is reused by the sum
    float mine = 0.0f;
    for (int k = threadIdx.x; k < n; k += 256) mine += lse_rescale(ps[k], v0[k] * sc, V);
    return block_sum_256(mine, sv);
}

// Noise of EPI_SAMPLE (kernels.h): a pure function of (seed, stream, draw, column), whatever kernel, tile, wave or row evaluates it.
// Philox4x32-10 (Salmon et al., SC'11) on counter (column, draw, stream, 0) and key (seed lo, seed hi); output word 0.
SVLN_DEV uint32_t philox4x32_10_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
// standard Gumbel from 23 random bits: u = ((w >> 9) + 0.5) * 2^-23 is exact in fp32 and lies in [2^-24, 1 - 2^-24] (24 bits would round
// 16777215.5 to 2^24: u = 1, G = +inf); E = -ln u in [2^-24 (1 + ..), 16.64], G = -ln E.  Both logarithms are v_log_f32 (1 ulp of log2,
// also next to u = 1 where the result is small: its error is relative) times fl(ln 2): E is good to ~2 ulp over the whole range, which
// the upper tail of G (u -> 1), where the winners come from, needs; |G error| <= 2^-18 max(1, |G|) is the tested bound.
SVLN_DEV float gumbel_from_bits(uint32_t w) {
    const float u = ((float)(w >> 9) + 0.5f) * 0x1p-23f;
    const float E = -0.6931471805599453f * __builtin_amdgcn_logf(u);
    return -0.6931471805599453f * __builtin_amdgcn_logf(E);
}
SVLN_DEV float gumbel_noise(uint32_t seed_lo, uint32_t seed_hi, int stream, int draw, int column) {
    return gumbel_from_bits(philox4x32_10_w0((uint32_t)column, (uint32_t)draw, (uint32_t)stream, 0u, seed_lo, seed_hi));
}

// activation functions (fp32).  sigmoid on the hardware transcendentals (v_exp_f32 / v_rcp_f32, ~1 ulp each: a few ulp of fp32 in all, far
// inside the 1e-3 parity bar) instead of libm's expf / tanhf and an IEEE division: an epilogue evaluates 64-128 activations per lane per
// 256 x 256 tile, and with libm (~35-50 instructions each) that was 35 of the 90 us of the nine-frame fc1 product and ~10 % of gate/up at
// T = 1952.  gelu_tanh uses 0.5 (1 + tanh u) = sigmoid(2u).
SVLN_DEV float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
SVLN_DEV float gelu_tanh_f(float x) {      // ACT2FN["gelu_pytorch_tanh"]  (siglip_encoder.py:83)
    const float k2 = 2.0f * 0.7978845608028654f;   // 2 sqrt(2/pi)
    return x * sigmoid_f(k2 * (x + 0.044715f * x * x * x));
}
SVLN_DEV float gelu_erf_f(float x) {       // nn.GELU()  (multimodal_projector/builder.py:45)
    return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f));
}
SVLN_DEV float silu_f(float x) { return x * sigmoid_f(x); }

// EPI_SWIGLU weight packing: 64-row blocks = [gate 32 | up 32].  The gate row of output j; its up row lies 32 further.
SVLN_HD size_t swiglu_gate_row(int j) { return (size_t)(j >> 5) * 64 + (j & 31); }

// ---- synthetic weights: identical arithmetic to streamvln_amd/weights.py ---------------------
SVLN_DEV uint64_t splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
SVLN_DEV float synth_value(uint64_t seed_t, uint64_t idx, float step, float base) {
    uint64_t z = splitmix64(seed_t + idx * 0x9E3779B97F4A7C15ull);
    float m = (float)(uint32_t)(z >> 40);
    float v = __fmul_rn(__fsub_rn(m, 8388608.0f), step);
    return base != 0.0f ? __fadd_rn(base, v) : v;
}
