// Allowed-token lm_head (svln_set_allowed_tokens): the product over a LISTED subset of the weight rows.
//
//   gemv_subset_kernel<T, EPI>   x_{a_j}(b) = W[a_j, :] . x[b, :] for the n <= 256 listed rows a_0 < ... < a_{n-1} and B <= 32 activation rows,
//       one wave per listed id, GEMV_SUBSET_WAVES per workgroup.  Lane l takes the 16-byte chunks l, l + 64, ... of the weight row and of the
//       activation row, converts to fp32 and runs one fmaf chain in element order; the wave total is wave_sum (a fixed butterfly).  The
//       summation order is therefore a function of K alone: not of B (the rows of a group of SUBSET_RB are independent chains), not of the
//       list, not of the id's place in it.  The same (weight row, activation row) pair gives the same bits from every caller.
//       Epilogue: repetition penalty on the flag of the VOCABULARY id, then ONE arg-max partial per listed id in the layout the final
//       kernels (gemv.hip) read, row stride n: part_val[b][j] = the processed value (z under EPI_SAMPLE), part_idx[b][j] = a_j or the
//       "owns nothing" word 0x7FFFFFFF when the value may not win (NaN, -inf), part_sum = 1 (0 for -inf, NaN for NaN), and under
//       EPI_SAMPLE part_max = part_raw = y.  launch_argmax_step / _final / _final_batched then run unchanged on n partials.
//   subset_logprobs_kernel       row b of the partials -> out[row][j] = y_j - logsumexp_i y_i (fixed trees: the same bits every launch).
//
// Roofline: n weight rows (458 KB at 64 ids of K = 3584 bf16) instead of the 1.09 GB lm_head: latency, not bandwidth.
#include "common.h"
#include "kernels.h"

namespace svln {

namespace {

constexpr int GEMV_SUBSET_WAVES = 4;     // listed ids per workgroup
constexpr int SUBSET_RB = 4;             // activation rows per pass over the weight row (independent accumulators)

template <typename T, int EPI>
__global__ __launch_bounds__(GEMV_SUBSET_WAVES * 64) void gemv_subset_kernel(GemvSubsetArgs p) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    constexpr HeadForm F = head_form(EPI);
    constexpr bool TGT = F.tgt, LSE = F.lse, SMP = F.smp;
    if (p.skip && *p.skip) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * GEMV_SUBSET_WAVES + wave;
    if (j >= p.n) return;                 // (no barrier below: a wave may leave alone)
    const int id = p.ids[j];              // validated on the host: 0 <= id < V
    const T* wrow = (const T*)p.W + (size_t)id * p.ldw;
    const T* xg = (const T*)p.x;
    const int nch = p.K / EPC;
    for (int b0 = 0; b0 < p.B; b0 += SUBSET_RB) {
        const T* xr[SUBSET_RB];
        float acc[SUBSET_RB];
#pragma unroll
        for (int r = 0; r < SUBSET_RB; ++r) {         // a ragged last group repeats the last row; nothing of it is written
            xr[r] = xg + (size_t)min(b0 + r, p.B - 1) * p.ldx;
            acc[r] = 0.0f;
        }
        for (int ci = lane; ci < nch; ci += 64) {
            float wf[EPC];
            chunk_to_f32<T>(*(const uint4*)(wrow + (size_t)ci * EPC), wf);
#pragma unroll
            for (int r = 0; r < SUBSET_RB; ++r) {
                float xf[EPC];
                chunk_to_f32<T>(*(const uint4*)(xr[r] + (size_t)ci * EPC), xf);
#pragma unroll
                for (int e = 0; e < EPC; ++e) acc[r] = fmaf(wf[e], xf[e], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < SUBSET_RB; ++r) acc[r] = wave_sum(acc[r]);
        if (lane != 0) continue;
#pragma unroll
        for (int r = 0; r < SUBSET_RB; ++r) {
            const int b = b0 + r;
            if (b >= p.B) break;
            float v = acc[r];
            if (p.pen_flags) {
                const uint8_t* fl = p.pen_flags + (p.pen_rows ? (size_t)p.pen_rows[b] * p.V : 0);
                if (fl[id]) v = v < 0.0f ? v * p.pen : v / p.pen;
            }
            const size_t o = (size_t)b * p.n + j;
            float y = v, val = v;
            if constexpr (TGT) y = val = v * p.tg_inv_t;       // a forced turn: the scored partials on y, no noise (1.0f with sampling off)
            if constexpr (SMP) {
                y = v * p.smp.inv_t;
                val = __fadd_rn(y, gumbel_noise(p.smp.seed_lo, p.smp.seed_hi, p.smp.stream[b], p.smp.draw[b] + (p.smp.count ? *p.smp.count : 0), id));       // (fl(y + G), never fma(v, inv_t, G))
                p.smp.part_raw[o] = y;
                p.smp.part_max[o] = y;
            }
            p.part_val[o] = val;
            p.part_idx[o] = val > -INFINITY ? id : 0x7FFFFFFF;       // NaN and -inf own nothing: they never win
            if (LSE || SMP) p.part_sum[o] = y == -INFINITY ? 0.0f : y != y ? y : 1.0f;
        }
    }
}

// out[row][j] = y_j - logsumexp_i y_i over the n entries of partial row b = blockIdx.x; row = *row_dev (generating path: GenCtl::count,
// before the step kernel advances it) or b.  A NaN entry makes the row NaN; a row of -inf only is NaN too.
__global__ __launch_bounds__(256) void subset_logprobs_kernel(const float* src, int n, float* out, const int* row_dev, const int* skip) {
    __shared__ float red[256];
    if (skip && *skip) return;
    const int t = threadIdx.x;
    const float y = t < n ? src[(size_t)blockIdx.x * n + t] : -INFINITY;
    red[t] = y;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = fmaxf(red[t], red[t + s]);       // (fmaxf drops a NaN; the sum below keeps it)
        __syncthreads();
    }
    const float m = red[0];
    __syncthreads();
    red[t] = t < n ? (y == -INFINITY ? 0.0f : lse_exp(y - m)) : 0.0f;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float lse = m + 0.6931471805599453f * __builtin_amdgcn_logf(red[0]);
    const size_t row = row_dev ? (size_t)*row_dev : (size_t)blockIdx.x;
    if (t < n) out[row * n + t] = y - lse;
}

template <typename T, int EPI> void launch_subset_epi(hipStream_t s, const GemvSubsetArgs& a) {
    const int grid = (a.n + GEMV_SUBSET_WAVES - 1) / GEMV_SUBSET_WAVES;
    hipLaunchKernelGGL((gemv_subset_kernel<T, EPI>), dim3(grid), dim3(GEMV_SUBSET_WAVES * 64), 0, s, a);
}

}  // namespace

template <typename T> void launch_gemv_subset(hipStream_t s, const GemvSubsetArgs& a) {
    with_head_epi<GEMV_SUBSET_EPIS>(a.epi, [&](auto e) { launch_subset_epi<T, decltype(e)::value>(s, a); });
}
template void launch_gemv_subset<bf16>(hipStream_t, const GemvSubsetArgs&);
template void launch_gemv_subset<float>(hipStream_t, const GemvSubsetArgs&);

void launch_subset_logprobs(hipStream_t s, const float* src, int n, int B, float* out, const int* row_dev, const int* skip) {
    hipLaunchKernelGGL(subset_logprobs_kernel, dim3(B), dim3(256), 0, s, src, n, out, row_dev, skip);
}

}  // namespace svln
