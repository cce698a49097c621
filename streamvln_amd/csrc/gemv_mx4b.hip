// Batched decode GEMV over MXFP4 weights for B <= 8 environments decoded in lockstep (svln_set_mxfp4_batched):
//   Y[b][n] = epi(sum_k Wq[n][k] * X[b][k] + bias[n]) + res[b][n]
// Weight-only: Wq is the engine's MXFP4 copy in the layout of the batch-1 GEMVs (q4 [N][ldw / 2] code bytes, e8 [N][ldw / 32] E8M0 scale
// bytes: gemv.hip WMxfp4), X stays bf16, the products are exact dequantised weight x bf16 activation, fp32 accumulate.
//
// The batch-1 conversion path (16 converts + 16 packed FMAs per block and per row of X) is far past the VALU budget at B = 8, so the
// product runs on v_mfma_f32_16x16x32_bf16: sixteen weight rows are the A operand, the B activation rows (padded with zeros to the
// tile's 16 columns) the B operand.  Lane (r = lane & 15, g = lane >> 4) loads ONE 16-byte MX block of weight row r -- block 4 s + g of
// super-step s (128 elements of K) -- with its scale byte, dequantises it in registers (v_cvt_scalef32_pk_bf16_fp4: one byte -> two
// scaled bf16 values) and spends it over four MFMAs, dword j of the block on MFMA j.  MFMA j of super-step s therefore sums over
// k = 128 s + 32 g + 8 j + (0 .. 7), g = 0 .. 3: a permutation of K inside the super-step, which the activation fragment repeats -- lane
// (b, g) holds x[b][128 s + 32 g + 8 j ..], the 64 contiguous bytes under its own block index.  A block index at or past K / 32 (K is a
// multiple of 32, not of 128) loads nothing and contributes zeros on both sides.
//
// Geometry: a workgroup owns one tile -- 16 rows (EPI_NONE), 16 gate rows and their 16 up rows (EPI_SWIGLU), 32 rows (EPI_ARGMAX) -- and
// its KW waves split the super-steps (interleaved), each with U blocks per row in flight; partial tiles are reduced through LDS.  KW =
// 16 when the launch has fewer than 512 tiles (q|k|v, o_proj, down_proj: 224-288 tiles for 256 CUs), 4 otherwise (gate/up, lm_head), with
// a grid-stride loop over the tiles.  Rows past N are clamped on load and never stored; columns b >= B are never stored.
//
// Algorithmic bytes per launch = N * K * 17 / 32 from HBM (+ the B rows of x per tile from L2).  Measured (profiles/mxfp4_batched.json,
// DESIGN.md 4.1): gate/up at B = 8 takes 38.9 us for 72.1 MB = 1.85 TB/s, 0.23 of the 8 TB/s specification -- NOT at the HBM roofline.
// U, the 512-tile switch to 16 waves and the one-tile workgroup are first choices, not tuned ones: at K = 3584 with 16 waves a wave has at
// most two real blocks per row in flight, every tile re-reads x from L2 (about as many bytes as the weights for gate/up), and the x loads
// sit inside the convert / MFMA loop without a prefetch.
#include "common.h"
#include "kernels.h"

namespace svln {

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
constexpr int MX4B_U = 4;               // blocks per weight row and lane in flight (untuned)
constexpr int MX4B_WIDE_TILES = 512;    // fewer tiles than this: 16 waves on K (untuned)

// one dword of E2M1 codes (8 weights) -> 8 scaled bf16 values, element order = nibble order
SVLN_DEV bf16x8 dequant8(unsigned d, float sc) {
    const bf16x2_t v0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 0);
    const bf16x2_t v1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 1);
    const bf16x2_t v2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 2);
    const bf16x2_t v3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 3);
    return bf16x8{v0[0], v0[1], v1[0], v1[1], v2[0], v2[1], v3[0], v3[1]};
}

template <int EPI, int KW>
__global__ __launch_bounds__(64 * KW) void gemv_mx4b_kernel(GemvMx4BatchArgs p) {
    constexpr int NT = EPI == EPI_NONE ? 1 : 2, U = MX4B_U;      // 16-row groups (accumulators) per tile
    __shared__ float part[KW][NT][16][17];                      // [wave][group][row][b], rows padded: conflict-free both ways
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;                     // weight row of the group / activation row b; block of the super-step
    const int nblk = p.K >> 5;
    const size_t qld = (size_t)(p.ldw >> 1), sld = (size_t)(p.ldw >> 5);
    const uint8_t* q4 = (const uint8_t*)p.q4;
    const bool xon = r < p.B;
    const bf16* xrow = (const bf16*)p.x + (size_t)(xon ? r : 0) * p.ldx;
    const int n_tiles = EPI == EPI_SWIGLU ? p.N >> 5 : (p.N + 16 * NT - 1) / (16 * NT);
    float best = -INFINITY;                                     // EPI_ARGMAX: thread (b, row 0) tracks env b
    int best_i = 0x7FFFFFFF;
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint8_t* qp[NT];
        const uint8_t* sp[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const size_t row = EPI == EPI_SWIGLU ? swiglu_gate_row(16 * t) + 32 * a + r : (size_t)min(16 * (NT * t + a) + r, p.N - 1);
            qp[a] = q4 + row * qld;
            sp[a] = p.e8 + row * sld;
        }
        f32x4 acc[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) acc[a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int s0 = wave; 4 * s0 < nblk; s0 += KW * U) {
            uint4 w[U][NT];
            unsigned sc[U][NT];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int blk = 4 * (s0 + KW * u) + g;
                const bool ok = blk < nblk;
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    w[u][a] = ok ? load_nt(qp[a] + (size_t)blk * 16) : zero_chunk();
                    sc[u][a] = ok ? (unsigned)sp[a][blk] : 127u;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int blk = 4 * (s0 + KW * u) + g;
                uint4 xf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xf[j] = (xon && blk < nblk) ? *(const uint4*)(xrow + (size_t)blk * 32 + 8 * j) : zero_chunk();
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    const float scale = __uint_as_float(sc[u][a] << 23);         // E8M0 -> fp32
                    const unsigned d[4] = {w[u][a].x, w[u][a].y, w[u][a].z, w[u][a].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dequant8(d[j], scale), __builtin_bit_cast(bf16x8, xf[j]), acc[a], 0, 0, 0);
                }
            }
        }
        // D[row = 4 g + i][col = r]: weight row of the group x activation row
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) part[wave][a][4 * g + i][r] = acc[a][i];
        __syncthreads();
        if (tid < 256) {
            const int b = tid >> 4, rr = tid & 15;
            float v[NT];
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                v[a] = part[0][a][rr][b];
#pragma unroll
                for (int k = 1; k < KW; ++k) v[a] += part[k][a][rr][b];
            }
            if (EPI == EPI_SWIGLU) {
                if (b < p.B) ((bf16*)p.y)[(size_t)b * p.ldy + 16 * t + rr] = from_f32<bf16>(silu_f(v[0]) * v[1]);
            } else if (EPI == EPI_ARGMAX) {
                const uint8_t* fl = p.pen_flags && b < p.B ? p.pen_flags + (size_t)p.pen_rows[b] * p.N : nullptr;
                float cv = -INFINITY;
                int ci = 0x7FFFFFFF;
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    const int n = 16 * (NT * t + a) + rr;
                    if (n < p.N) {
                        float x = v[a];
                        if (fl && fl[n]) x = x < 0.0f ? x * p.pen : x / p.pen;
                        if (x > cv) { cv = x; ci = n; }                          // rows ascend: first max wins
                    }
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(cv, o, 16);
                    const int oi = __shfl_xor(ci, o, 16);
                    if (ov > cv || (ov == cv && oi < ci)) { cv = ov; ci = oi; }
                }
                if (cv > best) { best = cv; best_i = ci; }                       // tiles ascend per workgroup: first max wins
            } else {
                const int n = 16 * t + rr;
                if (b < p.B && n < p.N) {
                    float x = v[0];
                    if (p.bias) x += to_f32(((const bf16*)p.bias)[n]);
                    if (p.res) x += to_f32(((const bf16*)p.res)[(size_t)b * p.ldr + n]);
                    ((bf16*)p.y)[(size_t)b * p.ldy + n] = from_f32<bf16>(x);
                }
            }
        }
        __syncthreads();
    }
    if (EPI == EPI_ARGMAX && tid < 256 && (tid & 15) == 0 && (tid >> 4) < p.B) {
        p.part_val[(size_t)(tid >> 4) * gridDim.x + blockIdx.x] = best;
        p.part_idx[(size_t)(tid >> 4) * gridDim.x + blockIdx.x] = best_i;
    }
}

int mx4b_tiles(int N, int epi) { return epi == EPI_NONE ? (N + 15) / 16 : epi == EPI_SWIGLU ? N / 32 : (N + 31) / 32; }

}  // namespace

int gemv_mx4b_grid(int N, int epi) {
    const int tiles = mx4b_tiles(N, epi), cap = epi == EPI_ARGMAX ? 1024 : 2048;      // (arg-max partials: [B][<= 2048] in the engine)
    return tiles < 1 ? 1 : tiles < cap ? tiles : cap;
}
void launch_gemv_mx4b(hipStream_t s, const GemvMx4BatchArgs& a) {
    const dim3 g(gemv_mx4b_grid(a.N, a.epi));
    const bool wide = mx4b_tiles(a.N, a.epi) < MX4B_WIDE_TILES;
    switch (a.epi) {
        case EPI_NONE:
            if (wide) hipLaunchKernelGGL((gemv_mx4b_kernel<EPI_NONE, 16>), g, dim3(1024), 0, s, a);
            else hipLaunchKernelGGL((gemv_mx4b_kernel<EPI_NONE, 4>), g, dim3(256), 0, s, a);
            break;
        case EPI_SWIGLU:
            if (wide) hipLaunchKernelGGL((gemv_mx4b_kernel<EPI_SWIGLU, 16>), g, dim3(1024), 0, s, a);
            else hipLaunchKernelGGL((gemv_mx4b_kernel<EPI_SWIGLU, 4>), g, dim3(256), 0, s, a);
            break;
        case EPI_ARGMAX: hipLaunchKernelGGL((gemv_mx4b_kernel<EPI_ARGMAX, 4>), g, dim3(256), 0, s, a); break;
        default: break;
    }
}

}  // namespace svln
