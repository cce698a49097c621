// Bandwidth-bound helper kernels of the path (norms, RoPE + KV append, ViT K/V packing,
// patch extraction, bilinear token pooling, embedding splice, weight synthesis / conversion).
// All of them are HBM/L2-bound byte movers: 16-byte vector accesses, one wave per row where a
// row reduction is needed, no LDS.
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace svln {

namespace {

// ------------------------------------------------------------------------------------------ norms
// one wave per row; three cached passes (the row stays in L1/L2): statistics in fp32.  y2r (optional): a second copy of the normalised row.
template <typename T>
__device__ __forceinline__ void rmsnorm_row(const T* xr, const T* g, T* yr, T* y2r, int n, float eps, int lane) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    const int nch = n / EPC;
    float ss = 0.0f;
    for (int ci = lane; ci < nch; ci += 64) {
        float f[EPC];
        chunk_to_f32<T>(*(const uint4*)(xr + (size_t)ci * EPC), f);
#pragma unroll
        for (int e = 0; e < EPC; ++e) ss += f[e] * f[e];
    }
    ss = wave_sum(ss);
    const float sc = rsqrtf(ss / (float)n + eps);
    for (int ci = lane; ci < nch; ci += 64) {
        float f[EPC], gf[EPC];
        chunk_to_f32<T>(*(const uint4*)(xr + (size_t)ci * EPC), f);
        chunk_to_f32<T>(*(const uint4*)(g + (size_t)ci * EPC), gf);
#pragma unroll
        for (int e = 0; e < EPC; ++e) f[e] = gf[e] * (f[e] * sc);
        const uint4 o = f32_to_chunk<T>(f);
        *(uint4*)(yr + (size_t)ci * EPC) = o;
        if (y2r) *(uint4*)(y2r + (size_t)ci * EPC) = o;
    }
}
// y2 (optional): a second copy of the normalised rows starting at row *y2_row (device scalar, clamped to y2_cap - 1) of y2 -- the hidden tap
// of a decode step whose index only the device knows (GenCtl.count), so the launch can sit in a captured graph
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const T* x, const T* g, T* y, int rows, int n, float eps, const int* skip, T* y2,
                                                      const int* y2_row, int y2_cap) {
    if (skip && *skip) return;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    T* y2r = y2 ? y2 + (size_t)min(*y2_row + row, y2_cap - 1) * n : nullptr;
    rmsnorm_row<T>(x + (size_t)row * n, g, y + (size_t)row * n, y2r, n, eps, lane);
}
// The head of a scheduler iteration that carries rides (svln_set_batch_draft): row r of y = the norm of row src_rows[r] of x (rmsnorm_row:
// bit-equal to rmsnorm_kernel on that row), copied as well to row tap_rows[r] of `tap` unless that is < 0.  Both lists are device arrays
// of `rows` ints the host has checked against the row counts of x and tap.
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_indexed_kernel(const T* x, const T* g, T* y, const int* src_rows, const int* tap_rows, T* tap,
                                                              int rows, int n, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = tap_rows[row];
    rmsnorm_row<T>(x + (size_t)src_rows[row] * n, g, y + (size_t)row * n, t >= 0 ? tap + (size_t)t * n : nullptr, n, eps, lane);
}

template <typename T>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* x, const T* g, const T* b, T* y, int rows, int n, float eps) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T* xr = x + (size_t)row * n;
    T* yr = y + (size_t)row * n;
    const int nch = n / EPC;
    float s = 0.0f;
    for (int ci = lane; ci < nch; ci += 64) {
        float f[EPC];
        chunk_to_f32<T>(*(const uint4*)(xr + (size_t)ci * EPC), f);
#pragma unroll
        for (int e = 0; e < EPC; ++e) s += f[e];
    }
    const float mu = wave_sum(s) / (float)n;
    float v = 0.0f;
    for (int ci = lane; ci < nch; ci += 64) {
        float f[EPC];
        chunk_to_f32<T>(*(const uint4*)(xr + (size_t)ci * EPC), f);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v += (f[e] - mu) * (f[e] - mu);
    }
    const float sc = rsqrtf(wave_sum(v) / (float)n + eps);
    for (int ci = lane; ci < nch; ci += 64) {
        float f[EPC], gf[EPC], bf[EPC];
        chunk_to_f32<T>(*(const uint4*)(xr + (size_t)ci * EPC), f);
        chunk_to_f32<T>(*(const uint4*)(g + (size_t)ci * EPC), gf);
        chunk_to_f32<T>(*(const uint4*)(b + (size_t)ci * EPC), bf);
#pragma unroll
        for (int e = 0; e < EPC; ++e) f[e] = (f[e] - mu) * sc * gf[e] + bf[e];
        *(uint4*)(yr + (size_t)ci * EPC) = f32_to_chunk<T>(f);
    }
}

// --------------------------------------------------------------------------------- RoPE + KV append
// grid (T, nq + nkv + nkv), 64 threads: lane d pairs (d, d + 64) of a 128-wide head.
// q heads: rotate in place.  k heads: rotate, write K page row.  v heads: write transposed Vt page.
// A wave per (row, head), four heads per workgroup (70 000 single-wave workgroups at T = 1952 are dispatch-bound).
// MIRROR (the folded candidates call): a k / v wave whose position lies in logical page p.mirror_page repeats its stores at the same
// in-page offsets of the p.n_mirror physical pages p.mirror_dst lists -- the values are computed once and stored 1 + n_mirror times.
// q heads and rows of other pages do what the plain form does; the plain form (MIRROR = false) carries none of this.
template <typename T, bool MIRROR = false>
__global__ __launch_bounds__(256) void rope_kv_kernel(RopeKvArgs p) {
    const int i = blockIdx.x, hd = blockIdx.y * 4 + (threadIdx.x >> 6), d = threadIdx.x & 63;
    if (hd >= p.nq + 2 * p.nkv) return;
    const int P = p.dyn_pos ? *p.dyn_pos : p.P;
    const int pos = P + i;
    T* row = (T*)p.qkv + (size_t)i * p.ld + (size_t)hd * 128;
    const float x1 = to_f32(row[d]), x2 = to_f32(row[d + 64]);
    const int page = p.page_table[pos >> 6], off = pos & 63;
    if (hd < p.nq + p.nkv) {
        const float c = p.rope_tab[(size_t)pos * 128 + d], s = p.rope_tab[(size_t)pos * 128 + 64 + d];
        const float o1 = x1 * c - x2 * s, o2 = x2 * c + x1 * s;     // q*cos + rotate_half(q)*sin
        if (hd < p.nq) {
            row[d] = from_f32<T>(o1);
            row[d + 64] = from_f32<T>(o2);
        } else {
            const int kh = hd - p.nq;
            T* kr = (T*)p.Kpool + (((size_t)page * p.nkv + kh) * 64 + off) * 128;
            const T k1 = from_f32<T>(o1), k2 = from_f32<T>(o2);
            kr[d] = k1;
            kr[d + 64] = k2;
            if constexpr (MIRROR) {
                if ((pos >> 6) == p.mirror_page)
                    for (int m = 0; m < p.n_mirror; ++m) {
                        T* mr = (T*)p.Kpool + (((size_t)p.mirror_dst[m] * p.nkv + kh) * 64 + off) * 128;
                        mr[d] = k1;
                        mr[d + 64] = k2;
                    }
            }
        }
    } else {
        const int kh = hd - p.nq - p.nkv;
        T* vt = (T*)p.Vpool + ((size_t)page * p.nkv + kh) * 128 * 64;
        const T v1 = from_f32<T>(x1), v2 = from_f32<T>(x2);
        vt[(size_t)d * 64 + off] = v1;
        vt[(size_t)(d + 64) * 64 + off] = v2;
        if constexpr (MIRROR) {
            if ((pos >> 6) == p.mirror_page)
                for (int m = 0; m < p.n_mirror; ++m) {
                    T* mt = (T*)p.Vpool + ((size_t)p.mirror_dst[m] * p.nkv + kh) * 128 * 64;
                    mt[(size_t)d * 64 + off] = v1;
                    mt[(size_t)(d + 64) * 64 + off] = v2;
                }
        }
    }
}

// cos/sin of pos * inv_freq[d] in fp32 (Qwen2RotaryEmbedding, modeling_qwen2.py:119-131), tabulated once
__global__ __launch_bounds__(64) void rope_table_kernel(float* tab, const float* inv_freq, int positions) {
    const int pos = blockIdx.x, d = threadIdx.x;
    const float ang = (float)pos * inv_freq[d];
    tab[(size_t)pos * 128 + d] = cosf(ang);
    tab[(size_t)pos * 128 + 64 + d] = sinf(ang);
}

// 128-bit content key of each frame: two position-dependent, order-independent 64-bit sums over the pixel words
// (64-bit atomic adds of per-thread partial sums), used to memoise pooled frame features (engine feature cache).
__global__ __launch_bounds__(256) void frame_hash_kernel(const uint32_t* pix, size_t words_per_frame, unsigned long long* out) {
    const int f = blockIdx.y;
    const uint32_t* p = pix + (size_t)f * words_per_frame;
    unsigned long long a = 0, b = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words_per_frame; i += (size_t)gridDim.x * 256) {
        const uint64_t v = (uint64_t)p[i] | ((uint64_t)i << 32);
        a += splitmix64(v ^ 0x243F6A8885A308D3ull);
        b += splitmix64(v * 0x9E3779B97F4A7C15ull + 0x13198A2E03707344ull);
    }
    atomicAdd(out + 2 * f, a);
    atomicAdd(out + 2 * f + 1, b);
}

// ViT K/V packing: qkv [F*S][3*Hv] -> K pages [tile][F*heads][64][HDP] (zero padded), Vt [tile][F*heads][VROWS][64].
// One workgroup per (64-key tile, frame*head).  K rows are copied as 16-byte chunks; V goes through an LDS tile
// [64 keys][HD] (16-byte chunk loads, row pitch padded by one chunk against bank conflicts) and leaves transposed as
// 16-byte chunks of 8 (4 for fp32) consecutive keys per head dim.  Requires HD % chunk == 0 and ld % chunk == 0.
template <typename T>
__global__ __launch_bounds__(256) void vit_kv_pack_kernel(const T* qkv, int ld, T* Kpool, T* Vpool, int F, int S, int heads, int HD,
                                                          int HDP, int VROWS) {
    extern __shared__ __attribute__((aligned(16))) char pack_smem[];
    constexpr int EPC = Elt<T>::PER_CHUNK;
    T* vt = (T*)pack_smem;
    const int tile = blockIdx.x, kh = blockIdx.y;          // kh = f*heads + head
    const int f = kh / heads, head = kh % heads, Hv = heads * HD;
    const int nkv = F * heads;
    const int hc = HD / EPC, hpc = HDP / EPC, pitch = HD + EPC;
    T* kp = Kpool + ((size_t)tile * nkv + kh) * 64 * HDP;
    T* vp = Vpool + ((size_t)tile * nkv + kh) * VROWS * 64;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (int e = threadIdx.x; e < 64 * hpc; e += 256) {
        const int key = e / hpc, cchunk = e % hpc, s = tile * 64 + key;
        uint4 v = zero;
        if (s < S && cchunk < hc) v = *(const uint4*)(qkv + (size_t)(f * S + s) * ld + Hv + head * HD + cchunk * EPC);
        *(uint4*)(kp + (size_t)key * HDP + cchunk * EPC) = v;
    }
    for (int e = threadIdx.x; e < 64 * hc; e += 256) {
        const int key = e / hc, cchunk = e % hc, s = tile * 64 + key;
        uint4 v = zero;
        if (s < S) v = *(const uint4*)(qkv + (size_t)(f * S + s) * ld + 2 * Hv + head * HD + cchunk * EPC);
        *(uint4*)(vt + key * pitch + cchunk * EPC) = v;
    }
    __syncthreads();
    constexpr int KC = 64 / EPC;                          // key chunks per Vt row
    for (int e = threadIdx.x; e < VROWS * KC; e += 256) {
        const int d = e / KC, kc = e % KC;
        T out[EPC];
#pragma unroll
        for (int j = 0; j < EPC; ++j) out[j] = d < HD ? vt[(kc * EPC + j) * pitch + d] : from_f32<T>(0.0f);
        *(uint4*)(vp + (size_t)d * 64 + kc * EPC) = *(const uint4*)out;
    }
}

// ------------------------------------------------------------------------------------------ vision
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const float* pix, T* out, int F, int image, int patch, int kp) {
    const int side = image / patch;
    const int prow = blockIdx.x;                          // f*side*side + py*side + px
    const int f = prow / (side * side), pp = prow % (side * side), py = pp / side, px = pp % side;
    const int kreal = 3 * patch * patch;
    for (int k = threadIdx.x; k < kp; k += 256) {
        float v = 0.0f;
        if (k < kreal) {
            const int c = k / (patch * patch), rem = k % (patch * patch), ky = rem / patch, kx = rem % patch;
            v = pix[(((size_t)f * 3 + c) * image + (py * patch + ky)) * image + px * patch + kx];
        }
        out[(size_t)prow * kp + k] = from_f32<T>(v);
    }
}

// bilinear pooling, ATen upsample_bilinear2d order: w0y*(w0x*a + w1x*b) + w1y*(w0x*c + w1x*d)
template <typename T>
__global__ __launch_bounds__(256) void pool_kernel(const T* in, T* out, const int* tap_idx, const float* tap_w, int side, int oside, int C) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    const int o = blockIdx.x;                              // f*oside*oside + oy*oside + ox
    const int f = o / (oside * oside), oo = o % (oside * oside), oy = oo / oside, ox = oo % oside;
    const int y0 = tap_idx[2 * oy], y1 = tap_idx[2 * oy + 1], x0 = tap_idx[2 * ox], x1 = tap_idx[2 * ox + 1];
    const float wy0 = tap_w[2 * oy], wy1 = tap_w[2 * oy + 1], wx0 = tap_w[2 * ox], wx1 = tap_w[2 * ox + 1];
    const T* base = in + (size_t)f * side * side * C;
    const T* a = base + (size_t)(y0 * side + x0) * C;
    const T* b = base + (size_t)(y0 * side + x1) * C;
    const T* c = base + (size_t)(y1 * side + x0) * C;
    const T* d = base + (size_t)(y1 * side + x1) * C;
    T* orow = out + (size_t)o * C;
    for (int ci = threadIdx.x; ci < C / EPC; ci += 256) {
        float fa[EPC], fb[EPC], fc[EPC], fd[EPC], r[EPC];
        chunk_to_f32<T>(*(const uint4*)(a + (size_t)ci * EPC), fa);
        chunk_to_f32<T>(*(const uint4*)(b + (size_t)ci * EPC), fb);
        chunk_to_f32<T>(*(const uint4*)(c + (size_t)ci * EPC), fc);
        chunk_to_f32<T>(*(const uint4*)(d + (size_t)ci * EPC), fd);
#pragma unroll
        for (int e = 0; e < EPC; ++e) r[e] = wy0 * (wx0 * fa[e] + wx1 * fb[e]) + wy1 * (wx0 * fc[e] + wx1 * fd[e]);
        *(uint4*)(orow + (size_t)ci * EPC) = f32_to_chunk<T>(r);
    }
}

template <typename T>
__device__ __forceinline__ void copy_row(T* o, const T* s, int n) {       // one workgroup of 256 threads, 16 bytes per access
    constexpr int EPC = Elt<T>::PER_CHUNK;
    for (int ci = threadIdx.x; ci < n / EPC; ci += 256) *(uint4*)(o + (size_t)ci * EPC) = *(const uint4*)(s + (size_t)ci * EPC);
}
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const int* src, const T* embed, const T* feats, T* out, int n, const int* skip) {
    if (skip && *skip) return;
    const int row = blockIdx.x;
    const int sidx = src[row];
    copy_row<T>(out + (size_t)row * n, sidx >= 0 ? embed + (size_t)sidx * n : feats + (size_t)(-(sidx + 1)) * n, n);
}
// ragged form for the draft rows of several prefill segments (svln_set_batch_draft): list[i] = (destination row of out, token id); the
// host has checked both against the row workspace and the vocabulary
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_ragged_kernel(const int2* list, const T* embed, T* out, int n) {
    const int2 d = list[blockIdx.x];
    copy_row<T>(out + (size_t)d.x * n, embed + (size_t)d.y * n, n);
}


// ------------------------------------------------------------------------------ draft-verified greedy decode
// The rows of the next verify pass (svln_set_speculative).  c = tokens emitted so far, row 0 = the last emitted token at position
// GenCtl.pos, row i >= 1 = draft[c + i - 1] at pos + i.  Rows used: up to `rows`, fewer when the draft runs out, when max_new leaves room
// for fewer tokens or when pos + i would reach max_positions; the FED TOKENS of the rows past them repeat row 0's (the dense products
// always carry `rows` rows; the attention and the verify step read vctl[1], so the attention output of those rows is never written and
// what they carry from o_proj on is stale buffer contents, which nothing reads).  vctl: [0] = usable draft length (host), [1] = rows used (written here).
__global__ __launch_bounds__(64) void verify_feed_kernel(const GenCtl* ctl, const int* token, const int* draft, int* vctl, int* fed, int rows,
                                                        int max_positions) {
    if (ctl->done) return;
    const int i = threadIdx.x;
    if (i >= rows) return;
    const int c = ctl->count, dlen = vctl[0];
    int n = rows;
    n = min(n, max(dlen - c + 1, 1));
    n = min(n, ctl->max_new - c);
    n = min(n, max_positions - ctl->pos);
    n = max(n, 0);
    fed[i] = (i >= 1 && i < n) ? draft[c + i - 1] : *token;
    if (i == 0) vctl[1] = n;
}

// One verify step on the arg-maxes cand[0 .. n) of the n = min(*n_rows, max_rows) rows fed with fed[0 .. n): cand[0] is always emitted,
// cand[i] iff every earlier row was emitted without stopping and cand[i - 1] == fed[i] (the guess that row i was fed is what the model
// emitted).  Stops are launch_argmax_step's: an EOS id (appended, not fed), the max_new-th token, a non-finite arg-max (-1).  Appends to
// out_ids, advances GenCtl, leaves the last emitted token in *out_token, copies the final-norm row xn[i] of every emitted token to
// hid_tap[min(its index, tap_cap - 1)] and adds to stats[0] (passes) / stats[1] (tokens emitted by passes).  No-op when done is set.
template <typename T>
__global__ __launch_bounds__(256) void verify_step_kernel(const int* fed, const int* cand, const int* n_rows, int max_rows, GenCtl* ctl,
                                                          const int* eos, int* out_ids, int* out_token, const T* xn, T* hid_tap, int H,
                                                          int tap_cap, int* stats) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    __shared__ int s_emit, s_c0, s_eos[8];
    const int was_done = ctl->done, n = min(min(*n_rows, max_rows), 8), n_eos = ctl->n_eos;
    if (was_done) return;                  // (uniform: thread 0 writes the flag only behind the barriers below)
    for (int i = 0; i < n; ++i) {          // is cand[i] an EOS id?  (the set may be large: all threads search it)
        int hit = 0;
        for (int k = threadIdx.x; k < n_eos; k += 256) hit |= eos[k] == cand[i];
        hit = __syncthreads_or(hit);
        if (threadIdx.x == 0) s_eos[i] = hit;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = ctl->count, max_new = ctl->max_new;
        int e = 0, stop = 0, last = -1;
        for (int i = 0; i < n && !stop; ++i) {
            if (i > 0 && cand[i - 1] != fed[i]) break;
            const int tok = cand[i];
            out_ids[c + e] = tok;
            ++e;
            last = tok;
            stop = tok < 0 || c + e >= max_new || s_eos[i];
        }
        if (e > 0) {
            *out_token = last;
            ctl->count = c + e;
            const int adv = stop ? e - 1 : e;          // the stopping token is appended, never fed
            ctl->pos += adv; ctl->kv_len += adv;
            if (stop) ctl->done = 1;
        }
        stats[0] += 1; stats[1] += e;
        s_emit = e; s_c0 = c;
    }
    __syncthreads();
    const int e = s_emit, c0 = s_c0, nch = H / EPC;
    for (int q = threadIdx.x; q < e * nch; q += 256) {
        const int j = q / nch, ci = q - j * nch;
        *(uint4*)(hid_tap + (size_t)min(c0 + j, tap_cap - 1) * H + (size_t)ci * EPC) = *(const uint4*)(xn + (size_t)j * H + (size_t)ci * EPC);
    }
}

// Several drafts of ONE turn, verified by one prefill pass (svln_generate_drafts).  Head rows: row 0 = the prompt's last row, then the
// rows draft g fed, k_g = clamp(k[g], 0, r) of them, sequence by sequence (row 1 + k_0 + .. + k_{g-1} + j was fed fed[g r + j]).  For every
// g the rule of verify_step_kernel runs on the row list [row 0, rows of g]: token 0 is always emitted, token i iff every earlier one was
// emitted without stopping and the arg-max of list row i - 1 equals fed[g r + i - 1]; stops are an EOS id (appended, never fed), the
// max_new-th token and a non-finite arg-max (-1).  The winner is the largest emitted count, a tie goes to the lowest g.  For the winner:
// out_ids, *out_token, GenCtl (count += e, pos / kv_len advance by e, by e - 1 on a stop, done), the final-norm row of every emitted token
// to hid_tap[min(its index, tap_cap - 1)], scores[index] = the row's log-probability when cand_score is given, rec = {winner, e, stop,
// head rows read}, stats[0] += 1 (passes), stats[1] += e (tokens).  One workgroup of 256 threads; no-op when done is set.
template <typename T>
__global__ __launch_bounds__(256) void draft_select_kernel(const DraftSelectArgs a) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    __shared__ int s_eos[DRAFT_SELECT_ROWS], s_emit, s_c0, s_base;
    GenCtl* ctl = a.ctl;
    const int was_done = ctl->done, n_eos = ctl->n_eos, G = min(a.G, 8), r = a.r;
    if (was_done) return;                  // (uniform: thread 0 writes the flag only behind the barriers below)
    int nh = 1;
    for (int g = 0; g < G; ++g) nh += min(max(a.k[g], 0), r);
    nh = min(nh, DRAFT_SELECT_ROWS);
    for (int i = 0; i < nh; ++i) {         // is cand[i] an EOS id?  (the set may be large: all threads search it)
        int hit = 0;
        for (int q = threadIdx.x; q < n_eos; q += 256) hit |= a.eos[q] == a.cand[i];
        hit = __syncthreads_or(hit);
        if (threadIdx.x == 0) s_eos[i] = hit;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = ctl->count, max_new = ctl->max_new;
        int best = -1, best_e = 0, best_stop = 0, best_base = 1, base = 1;
        for (int g = 0; g < G; ++g) {
            const int kg = min(max(a.k[g], 0), r);
            int e = 0, stop = 0, prev = 0;
            for (int i = 0; i <= kg && !stop && base + i - 1 < nh; ++i) {
                if (i > 0 && prev != a.fed[g * r + i - 1]) break;
                const int row = i == 0 ? 0 : base + i - 1;
                prev = a.cand[row];
                ++e;
                stop = prev < 0 || c + e >= max_new || s_eos[row];
            }
            if (e > best_e) { best = g; best_e = e; best_stop = stop; best_base = base; }
            base += kg;
        }
        int last = -1;
        for (int i = 0; i < best_e; ++i) {
            last = a.cand[i == 0 ? 0 : best_base + i - 1];
            a.out_ids[c + i] = last;
        }
        if (best_e > 0) {
            *a.out_token = last;
            ctl->count = c + best_e;
            const int adv = best_stop ? best_e - 1 : best_e;          // the stopping token is appended, never fed
            ctl->pos += adv; ctl->kv_len += adv;
            if (best_stop) ctl->done = 1;
        }
        a.rec[0] = best; a.rec[1] = best_e; a.rec[2] = best_stop; a.rec[3] = nh;
        a.stats[0] += 1; a.stats[1] += best_e;
        s_emit = best_e; s_c0 = c; s_base = best_base;
    }
    __syncthreads();
    const int e = s_emit, c0 = s_c0, wb = s_base, nch = a.H / EPC;
    const T* xn = (const T*)a.xn; T* tap = (T*)a.hid_tap;
    for (int q = threadIdx.x; q < e * nch; q += 256) {
        const int j = q / nch, ci = q - j * nch, row = j == 0 ? 0 : wb + j - 1;
        *(uint4*)(tap + (size_t)min(c0 + j, a.tap_cap - 1) * a.H + (size_t)ci * EPC) = *(const uint4*)(xn + (size_t)row * a.H + (size_t)ci * EPC);
    }
    if (a.cand_score && (int)threadIdx.x < e) a.scores[c0 + threadIdx.x] = a.cand_score[threadIdx.x == 0 ? 0 : wb + (int)threadIdx.x - 1];
}

// --------------------------------------------------------------------------- slow-memory token pruning
// OPT-IN EXTENSION (BASELINE configs[3]; SURVEY.md a-13: the reference has no counterpart, parity is pinned only by this
// project's own CPU restatement oracle/streamvln_oracle.py: prune_memory_tokens).  Rule: score_i = cos(M_i, mean_j M_j) over the
// N memory tokens; the `keep` tokens with the SMALLEST score (the least like the average token; ties: lower index) survive,
// in their original order.  Four launches: column partial sums (64-row blocks, fixed order -> deterministic), mean, per-token
// score (one wave per token), rank by counting (one wave per token), compaction of the kept indices (one workgroup, ballot scan).
template <typename T>
__global__ __launch_bounds__(256) void mem_colsum_kernel(const T* m, int n_rows, int H, float* partial) {
    const int col = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * 64;
    if (col >= H) return;
    float acc = 0.0f;
    for (int r = r0; r < min(r0 + 64, n_rows); ++r) acc += to_f32(m[(size_t)r * H + col]);
    partial[(size_t)blockIdx.y * H + col] = acc;
}
__global__ __launch_bounds__(256) void mem_mean_kernel(const float* partial, int n_blocks, int n_rows, int H, float* mean) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= H) return;
    float mu = 0.0f;
    for (int b = 0; b < n_blocks; ++b) mu += partial[(size_t)b * H + col];
    mean[col] = mu / (float)n_rows;
}
template <typename T>
__global__ __launch_bounds__(256) void mem_score_kernel(const T* m, int n_rows, int H, const float* mean, float* score) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    float dot = 0.0f, nn = 0.0f, mm = 0.0f;
    for (int ci = lane; ci < H / EPC; ci += 64) {
        float f[EPC];
        chunk_to_f32<T>(*(const uint4*)(m + (size_t)row * H + (size_t)ci * EPC), f);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float mu = mean[ci * EPC + e];
            dot = fmaf(f[e], mu, dot); nn = fmaf(f[e], f[e], nn); mm = fmaf(mu, mu, mm);
        }
    }
    dot = wave_sum(dot); nn = wave_sum(nn); mm = wave_sum(mm);
    if (lane == 0) score[row] = dot / fmaxf(sqrtf(nn) * sqrtf(mm), 1e-20f);
}
// rank by counting, one wave per token: flag[i] = (number of tokens that sort before i) < keep.  n / 4 workgroups instead of the single
// workgroup of round 2 (162 us at n = 1568).
__global__ __launch_bounds__(256) void mem_rank_kernel(const float* score, int n, int keep, int* flag) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float si = score[i];
    int rank = 0;
    for (int j = lane; j < n; j += 64) {
        const float sj = score[j];
        rank += (sj < si || (sj == si && j < i)) ? 1 : 0;
    }
    rank = (int)wave_sum((float)rank);        // counts <= 2^24 are exact in fp32
    if (lane == 0) flag[i] = rank < keep ? 1 : 0;
}
// sel = ascending indices of the flagged tokens: one workgroup, block-wide exclusive scan of the flags (wave ballots + wave totals)
__global__ __launch_bounds__(1024) void mem_compact_kernel(const int* flag, int n, int* sel) {
    __shared__ int wtot[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const int f = i < n ? flag[i] : 0;
        const unsigned long long b = __ballot(f != 0);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(b);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        if (f) sel[off + before] = i;
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += wtot[w]; base += t; }
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------- weights
SVLN_DEV int64_t map_row(int64_t r, RowMap m) { return (r / m.blk) * (int64_t)m.blk * m.nint + (int64_t)m.phase * m.blk + r % m.blk; }

template <typename T>
__global__ __launch_bounds__(256) void synth_kernel(T* dst, int dst_ld, int64_t rows, int cols, RowMap m, uint64_t seed_t, float step,
                                                    float base) {
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols;
        const int c = (int)(i - r * cols);
        // weights are defined as bf16 values (like the real checkpoint); the fp32 engine stores them widened
        dst[map_row(r, m) * dst_ld + c] = from_f32<T>(to_f32((bf16)synth_value(seed_t, (uint64_t)i, step, base)));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void convert_kernel(T* dst, int dst_ld, int64_t rows, int cols, RowMap m, const void* src, int src_is_f32) {
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols;
        const int c = (int)(i - r * cols);
        const float v = src_is_f32 ? ((const float*)src)[i] : to_f32(((const bf16*)src)[i]);
        dst[map_row(r, m) * dst_ld + c] = from_f32<T>(v);
    }
}

template <typename T> __global__ void to_f32_kernel(const T* s, float* d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d[i] = to_f32(s[i]);
}
template <typename T> __global__ void from_f32_kernel(const float* s, T* d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d[i] = from_f32<T>(s[i]);
}

int grid_for(int64_t n) {
    int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace



template <typename T> void launch_rmsnorm(hipStream_t s, const void* x, const void* g, void* y, int rows, int n, float eps, const int* skip,
                                          void* y2, const int* y2_row, int y2_cap) {
    if (rows <= 0) return;
    hipLaunchKernelGGL((rmsnorm_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, (const T*)x, (const T*)g, (T*)y, rows, n, eps, skip, (T*)y2,
                       y2_row, y2_cap);
}
template <typename T> void launch_rmsnorm_indexed(hipStream_t s, const void* x, const void* g, void* y, const int* src_rows, const int* tap_rows,
                                                  void* tap, int rows, int n, float eps) {
    if (rows <= 0) return;
    hipLaunchKernelGGL((rmsnorm_indexed_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, (const T*)x, (const T*)g, (T*)y, src_rows, tap_rows,
                       (T*)tap, rows, n, eps);
}
template <typename T> void launch_layernorm(hipStream_t s, const void* x, const void* g, const void* b, void* y, int rows, int n, float eps) {
    if (rows <= 0) return;
    hipLaunchKernelGGL((layernorm_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, s, (const T*)x, (const T*)g, (const T*)b, (T*)y, rows, n, eps);
}
template <typename T> void launch_rope_kv(hipStream_t s, const RopeKvArgs& a) {
    if (a.n_mirror < 0 || a.n_mirror > ROPE_MIRROR_MAX || (a.n_mirror > 0 && !a.mirror_dst))
        throw std::runtime_error("rope_kv: 0 .. 7 mirror pages with a device list");
    const dim3 grid(a.T, (a.nq + 2 * a.nkv + 3) / 4);
    if (a.n_mirror > 0) hipLaunchKernelGGL((rope_kv_kernel<T, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((rope_kv_kernel<T>), grid, dim3(256), 0, s, a);
}
void launch_frame_hash(hipStream_t s, const float* pix, int F, size_t words_per_frame, unsigned long long* out) {
    hipLaunchKernelGGL(frame_hash_kernel, dim3(64, F), dim3(256), 0, s, (const uint32_t*)pix, words_per_frame, out);
}
void launch_rope_table(hipStream_t s, float* tab, const float* inv_freq, int positions) {
    hipLaunchKernelGGL(rope_table_kernel, dim3(positions), dim3(64), 0, s, tab, inv_freq, positions);
}
template <typename T> void launch_vit_kv_pack(hipStream_t s, const void* qkv, int ld, void* Kpool, void* Vpool, int F, int S, int heads,
                                             int head_dim) {
    constexpr int EPC = Elt<T>::PER_CHUNK;
    const int hdc = (((head_dim + EPC - 1) / EPC) + 1) & ~1;
    const int vrows = ((head_dim + 31) / 32) * 32;
    const size_t lds = (size_t)64 * (head_dim + EPC) * sizeof(T);
    hipLaunchKernelGGL((vit_kv_pack_kernel<T>), dim3((S + 63) / 64, F * heads), dim3(256), lds, s, (const T*)qkv, ld, (T*)Kpool, (T*)Vpool, F, S,
                       heads, head_dim, hdc * EPC, vrows);
}
template <typename T> void launch_patchify(hipStream_t s, const float* pix, void* out, int F, int image, int patch, int kp) {
    const int side = image / patch;
    hipLaunchKernelGGL((patchify_kernel<T>), dim3(F * side * side), dim3(256), 0, s, pix, (T*)out, F, image, patch, kp);
}
template <typename T> void launch_pool(hipStream_t s, const void* in, void* out, const int* tap_idx, const float* tap_w, int F, int side,
                                       int out_side, int C) {
    hipLaunchKernelGGL((pool_kernel<T>), dim3(F * out_side * out_side), dim3(256), 0, s, (const T*)in, (T*)out, tap_idx, tap_w, side, out_side, C);
}
template <typename T> void launch_gather_rows(hipStream_t s, const int* src, const void* embed, const void* feats, void* out, int rows, int n,
                                              const int* skip) {
    if (rows <= 0) return;
    hipLaunchKernelGGL((gather_rows_kernel<T>), dim3(rows), dim3(256), 0, s, src, (const T*)embed, (const T*)feats, (T*)out, n, skip);
}
template <typename T> void launch_gather_rows_ragged(hipStream_t s, const int* list, const void* embed, void* out, int rows, int n) {
    if (rows <= 0) return;
    hipLaunchKernelGGL((gather_rows_ragged_kernel<T>), dim3(rows), dim3(256), 0, s, (const int2*)list, (const T*)embed, (T*)out, n);
}
void launch_verify_feed(hipStream_t s, const GenCtl* ctl, const int* token, const int* draft, int* vctl, int* fed, int rows, int max_positions) {
    hipLaunchKernelGGL(verify_feed_kernel, dim3(1), dim3(64), 0, s, ctl, token, draft, vctl, fed, rows, max_positions);
}
template <typename T> void launch_verify_step(hipStream_t s, const int* fed, const int* cand, const int* n_rows, int max_rows, GenCtl* ctl,
                                              const int* eos, int* out_ids, int* out_token, const void* xn, void* hid_tap, int H, int tap_cap,
                                              int* stats) {
    hipLaunchKernelGGL((verify_step_kernel<T>), dim3(1), dim3(256), 0, s, fed, cand, n_rows, max_rows, ctl, eos, out_ids, out_token, (const T*)xn,
                       (T*)hid_tap, H, tap_cap, stats);
}
template <typename T> void launch_draft_select(hipStream_t s, const DraftSelectArgs& a) {
    hipLaunchKernelGGL((draft_select_kernel<T>), dim3(1), dim3(256), 0, s, a);
}
// scratch: partial [ceil(n/64)][H] floats, mean [H], score [n]; sel [keep] ints (ascending row indices)
template <typename T> void launch_memory_prune(hipStream_t s, const void* m, int n_rows, int H, int keep, float* partial, float* mean, float* score,
                                               int* sel) {
    const int nb = (n_rows + 63) / 64;
    hipLaunchKernelGGL((mem_colsum_kernel<T>), dim3((H + 255) / 256, nb), dim3(256), 0, s, (const T*)m, n_rows, H, partial);
    hipLaunchKernelGGL(mem_mean_kernel, dim3((H + 255) / 256), dim3(256), 0, s, partial, nb, n_rows, H, mean);
    hipLaunchKernelGGL((mem_score_kernel<T>), dim3((n_rows + 3) / 4), dim3(256), 0, s, (const T*)m, n_rows, H, mean, score);
    int* flag = (int*)partial;              // the column partial sums are consumed by now: their buffer (>= ceil(n / 64) * H floats) holds the n flags
    hipLaunchKernelGGL(mem_rank_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, s, score, n_rows, keep, flag);
    hipLaunchKernelGGL(mem_compact_kernel, dim3(1), dim3(1024), 0, s, flag, n_rows, sel);
}
template <typename T> void launch_synth(hipStream_t s, void* dst, int dst_ld, int64_t rows, int cols, RowMap m, uint64_t seed_t,
                                        float half_width, float base) {
    const float step = half_width / 8388608.0f;
    hipLaunchKernelGGL((synth_kernel<T>), dim3(grid_for(rows * cols)), dim3(256), 0, s, (T*)dst, dst_ld, rows, cols, m, seed_t, step, base);
}
template <typename T> void launch_convert(hipStream_t s, void* dst, int dst_ld, int64_t rows, int cols, RowMap m, const void* src, int src_is_f32) {
    hipLaunchKernelGGL((convert_kernel<T>), dim3(grid_for(rows * cols)), dim3(256), 0, s, (T*)dst, dst_ld, rows, cols, m, src, src_is_f32);
}
template <typename T> void launch_to_f32(hipStream_t s, const void* src, float* dst, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL((to_f32_kernel<T>), dim3(grid_for(n)), dim3(256), 0, s, (const T*)src, dst, n);
}
template <typename T> void launch_from_f32(hipStream_t s, const float* src, void* dst, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL((from_f32_kernel<T>), dim3(grid_for(n)), dim3(256), 0, s, src, (T*)dst, n);
}

// svln_top_logprobs: the merge of one row's candidates (contract: kernels.h, launch_topk_merge).  One workgroup per row.  (V, S) first, on
// the device functions of the scored final kernels and the same partials, so that the emitted id's entry is its score bit for bit.  Then
// every thread takes its share of the n_part x c candidates into registers once (TOPK_MERGE_PER_THREAD each; what may not be listed -- NaN, -inf, padding, a partial that owns nothing -- becomes (-inf, none)) and k
// rounds pick the best pair strictly behind the previous winner in (y descending, column ascending) order: columns are unique, so the
// rounds list distinct columns and nothing is marked.  A round is a scan of the registers, a wave reduction on shuffles and ONE barrier:
// the four waves' winners go through LDS slots that alternate by round, and every thread merges them alike.
namespace {
// The selection rounds of topk_merge_kernel and truncate_partials_kernel (one body: the two kernels list the same winners by construction).
// cv / ci: one row's `total` candidates; wv / wi: [2][4] LDS slots; thread j < k leaves with round j's winner in (my_v, my_i), every
// other thread -- and a round behind the last listable candidate -- with (-inf, 0x7FFFFFFF).
template <int TOPK_MERGE_PER_THREAD>
SVLN_DEV void topk_select_256(const float* cv, const int* ci, int total, int k, float (*wv)[4], int (*wi)[4], float& my_v, int& my_i) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float rv[TOPK_MERGE_PER_THREAD];
    int ri[TOPK_MERGE_PER_THREAD];
#pragma unroll
    for (int u = 0; u < TOPK_MERGE_PER_THREAD; ++u) {
        const int t = tid + 256 * u, tc = min(t, total - 1);      // (clamped, not conditional: every load is in flight at once)
        const float a = cv[tc];
        const int ai = ci[tc];
        const bool listable = t < total && a > -INFINITY && ai != 0x7FFFFFFF;
        rv[u] = listable ? a : -INFINITY;
        ri[u] = listable ? ai : 0x7FFFFFFF;
    }
    float prev_v = INFINITY;
    int prev_i = -1;
    my_v = -INFINITY; my_i = 0x7FFFFFFF;
    for (int j = 0; j < k; ++j) {
        float v = -INFINITY;
        int i = 0x7FFFFFFF;
#pragma unroll
        for (int u = 0; u < TOPK_MERGE_PER_THREAD; ++u) {
            const float a = rv[u];
            const int ai = ri[u];
            const bool behind = a < prev_v || (a == prev_v && ai > prev_i);         // not listed yet
            if (behind && ai != 0x7FFFFFFF && (a > v || (a == v && ai < i))) { v = a; i = ai; }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float ov = __shfl_xor(v, d, 64);
            const int oi = __shfl_xor(i, d, 64);
            if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
        }
        if (lane == 0) { wv[j & 1][wave] = v; wi[j & 1][wave] = i; }
        __syncthreads();                          // (the slots of round j are written again in round j + 2, behind round j + 1's barrier)
        prev_v = wv[j & 1][0]; prev_i = wi[j & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = wv[j & 1][w];
            const int oi = wi[j & 1][w];
            if (ov > prev_v || (ov == prev_v && oi < prev_i)) { prev_v = ov; prev_i = oi; }
        }
        // (-inf, none) once the row is exhausted: nothing lies behind it, the later rounds find nothing either
        if (tid == j) { my_v = prev_v; my_i = prev_i; }
    }
}
// TOPK_MERGE_PER_THREAD x 256 threads candidates: 32 holds the full vocabulary's 1024 single-env partials x TOPK_C, 64 the 2048 partials
// the batched GEMV and the MFMA tiles can give
template <int TOPK_MERGE_PER_THREAD>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* cand_val, const int* cand_idx, int n_part, int c, int k, const float* pv,
                                                         const int* pi, const float* ps, const float* pm, int* top_ids, float* top_logprobs,
                                                         const int* row_dev, const int* skip) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ float wv[2][4];
    __shared__ int wi[2][4];
    if (skip && *skip) return;
    const int tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * n_part;
    float V, S;
    if (pm) {                                     // sampled: V = max part_max, S on (part_max, part_sum); no token is looked up (-1 owns no partial)
        const SampleMerge mg = sample_merge(pi + o, pm + o, pm + o, ps + o, n_part, -1, sv, si);
        V = mg.V; S = mg.S;
    } else {
        row_argmax_256(pv + o, pi + o, n_part, sv, si);
        V = sv[0];
        S = row_lse_sum_256(ps + o, pv + o, n_part, 1.0f, V, sv);
    }
    float my_v;                                   // thread j < k keeps round j's winner
    int my_i;
    topk_select_256<TOPK_MERGE_PER_THREAD>(cand_val + o * c, cand_idx + o * c, n_part * c, k, wv, wi, my_v, my_i);
    if (tid < k) {
        const size_t row = row_dev ? (size_t)*row_dev : (size_t)blockIdx.x;
        // the expressions of the final kernels: the sampled score is raw - V + lse_logprob(S); the greedy one is lse_logprob(S), and
        // (y - V) - log S written as -(log S - (y - V)) equals it to the sign of a zero when y == V (target_final_batched_kernel)
        float lp;
        if (pm) lp = my_v - V + lse_logprob(S);
        else lp = -(-lse_logprob(S) - (my_v - V));
        top_ids[row * k + tid] = my_i == 0x7FFFFFFF ? -1 : my_i;
        top_logprobs[row * k + tid] = my_i == 0x7FFFFFFF ? -INFINITY : lp;
    }
}
// svln_sampling_truncation: one row's candidates -> the 8-entry partial row of the truncated turn (contract: kernels.h,
// launch_truncate_partials).  The selection rounds above leave winner j with thread j; the eight (y, column) pairs go through LDS to
// thread 0, which accumulates the prefix c_j serially in fp32 and counts the kept prefix; threads 0 .. 7 then write one entry each, the
// kept ones with the noise of their own column.
template <int TOPK_MERGE_PER_THREAD>
__global__ __launch_bounds__(256) void truncate_partials_kernel(const float* cand_val, const int* cand_idx, int n_part, int c, int k, float top_p,
                                                                SampleArgs smp, float* tr_val, int* tr_idx, float* tr_sum, const int* skip) {
    __shared__ float wv[2][4];
    __shared__ int wi[2][4];
    __shared__ float ly[TOPK_C];
    __shared__ int li[TOPK_C];
    __shared__ int n_keep;
    if (skip && *skip) return;
    const int tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * n_part;
    float my_v;
    int my_i;
    topk_select_256<TOPK_MERGE_PER_THREAD>(cand_val + o * c, cand_idx + o * c, n_part * c, k, wv, wi, my_v, my_i);
    if (tid < TOPK_C) { ly[tid] = my_v; li[tid] = my_i; }
    __syncthreads();
    if (tid == 0) {
        int kept = 0;
        if (li[0] != 0x7FFFFFFF) {
            int kk = 1;                           // k' = the listed prefix
            while (kk < TOPK_C && li[kk] != 0x7FFFFFFF) ++kk;
            float total = 0.0f;                   // c_j = c_{j-1} + e_j, serially in index order
            for (int j = 0; j < kk; ++j) total += lse_exp(ly[j] - ly[0]);
            const float bound = top_p * total;
            float before = 0.0f;                  // c_{j-1}: the same additions in the same order, hence the same bits
            kept = 1;                             // entry 0 is always kept; the kept set is a prefix: the masses ascend
            for (int j = 1; j < kk; ++j) {
                before += lse_exp(ly[j - 1] - ly[0]);
                if (!(top_p >= 1.0f || before < bound)) break;
                kept = j + 1;
            }
        }
        n_keep = kept;
    }
    __syncthreads();
    if (tid < TOPK_C) {
        const bool keep = tid < n_keep;
        float z = -INFINITY;
        if (keep) {
            const int b = blockIdx.x;
            z = __fadd_rn(my_v, gumbel_noise(smp.seed_lo, smp.seed_hi, smp.stream[b], smp.draw[b] + (smp.count ? *smp.count : 0), my_i));      // the epilogues' fl(y + G)
        }
        const size_t q = (size_t)blockIdx.x * TOPK_C + tid;
        tr_val[q] = z;
        tr_idx[q] = keep ? my_i : 0x7FFFFFFF;
        smp.part_raw[q] = keep ? my_v : 0.0f;
        smp.part_max[q] = keep ? my_v : -INFINITY;
        tr_sum[q] = keep ? 1.0f : 0.0f;
    }
}
// svln_token_entropy: the entropy of one row from its partials (contract: kernels.h, launch_entropy_merge).  One workgroup per row.
// (V, S) as in topk_merge_kernel -- the device functions of the scored final kernels on the same partials, the same bits -- then T on the
// same fixed tree, every partial's t seen from V by ent_rescale (pe == nullptr: t = 0, one id per partial), and H = log S - T / S.
__global__ __launch_bounds__(256) void entropy_merge_kernel(const float* pv, const int* pi, const float* ps, const float* pm, const float* pe,
                                                            int n_part, float* out, const int* row_dev, const int* skip) {
    __shared__ float sv[256];
    __shared__ int si[256];
    if (skip && *skip) return;
    const size_t o = (size_t)blockIdx.x * n_part;
    float V, S;
    bool none;
    const float* m0 = pm ? pm + o : pv + o;       // the maxima the partial sums are relative to
    if (pm) {                                     // sampled: V = max part_max, S on (part_max, part_sum); no token is looked up
        const SampleMerge mg = sample_merge(pi + o, pm + o, pm + o, ps + o, n_part, -1, sv, si);
        V = mg.V; S = mg.S;
        none = V == -INFINITY;
    } else {
        row_argmax_256(pv + o, pi + o, n_part, sv, si);
        V = sv[0];
        none = si[0] == 0x7FFFFFFF;
        S = row_lse_sum_256(ps + o, pv + o, n_part, 1.0f, V, sv);
    }
    __syncthreads();                              // sv[0] has been read by every thread
    float mine = 0.0f;
    for (int k = threadIdx.x; k < n_part; k += 256) mine += ent_rescale(pe ? pe[o + k] : 0.0f, ps[o + k], m0[k], V);
    const float T = block_sum_256(mine, sv);
    if (threadIdx.x == 0) {
        const size_t row = row_dev ? (size_t)*row_dev : (size_t)blockIdx.x;
        out[row] = none ? __builtin_nanf("") : ent_value(S, T);
    }
}
}  // namespace
void launch_entropy_merge(hipStream_t s, const float* part_val, const int* part_idx, const float* part_sum, const float* part_max,
                          const float* part_ent, int n_part, int B, float* out, const int* row_dev, const int* skip) {
    hipLaunchKernelGGL(entropy_merge_kernel, dim3(B), dim3(256), 0, s, part_val, part_idx, part_sum, part_max, part_ent, n_part, out, row_dev, skip);
}
void launch_topk_merge(hipStream_t s, const float* cand_val, const int* cand_idx, int n_part, int c, int B, int k, const float* part_val,
                       const int* part_idx, const float* part_sum, const float* part_max, int* top_ids, float* top_logprobs, const int* row_dev,
                       const int* skip) {
    const size_t total = (size_t)n_part * c;
    if (total > (size_t)256 * 64) throw std::runtime_error("topk merge: more candidates than the kernel's registers hold");
    if (total <= (size_t)256 * 32)
        hipLaunchKernelGGL(topk_merge_kernel<32>, dim3(B), dim3(256), 0, s, cand_val, cand_idx, n_part, c, k, part_val, part_idx, part_sum, part_max,
                           top_ids, top_logprobs, row_dev, skip);
    else
        hipLaunchKernelGGL(topk_merge_kernel<64>, dim3(B), dim3(256), 0, s, cand_val, cand_idx, n_part, c, k, part_val, part_idx, part_sum, part_max,
                           top_ids, top_logprobs, row_dev, skip);
}

void launch_truncate_partials(hipStream_t s, const float* cand_val, const int* cand_idx, int n_part, int c, int B, int top_k, float top_p,
                              const SampleArgs& smp, float* tr_val, int* tr_idx, float* tr_sum, const int* skip) {
    const size_t total = (size_t)n_part * c;
    if (n_part < 1 || c < 1 || B < 1) throw std::runtime_error("truncate partials: empty candidate rows");
    if (total > (size_t)256 * 64) throw std::runtime_error("truncate partials: more candidates than the kernel's registers hold");
    if (top_k < 1 || top_k > TOPK_C || !(top_p > 0.0f && top_p <= 1.0f)) throw std::runtime_error("truncate partials: top_k must be 1 .. 8 and top_p in (0, 1]");
    if (total <= (size_t)256 * 32)
        hipLaunchKernelGGL(truncate_partials_kernel<32>, dim3(B), dim3(256), 0, s, cand_val, cand_idx, n_part, c, top_k, top_p, smp, tr_val, tr_idx,
                           tr_sum, skip);
    else
        hipLaunchKernelGGL(truncate_partials_kernel<64>, dim3(B), dim3(256), 0, s, cand_val, cand_idx, n_part, c, top_k, top_p, smp, tr_val, tr_idx,
                           tr_sum, skip);
}

// One select step of a beam turn (contract: kernels.h, launch_beam_select).  One wave: thread r * 8 + j owns pool item (r, j) -- the
// finished hypothesis r itself (j = 0) or child j of the live hypothesis r -- and its place in the new set is the number of items that
// beat it (score descending, then r, then j ascending: the thread index).  Thread c < n_new then builds hypothesis c from its parent's
// row of the old state; thread 0 hands out the page sets serially (a child's set depends on the children before it) and writes the record.
namespace {
__global__ __launch_bounds__(64) void beam_select_kernel(BeamSelectArgs a) {
    __shared__ float s_score[64];
    __shared__ int s_valid[64];
    __shared__ int s_sel[BEAM_MAX_W];
    __shared__ int s_live[BEAM_MAX_W];
    const int tid = threadIdx.x, r = tid >> 3, j = tid & 7;
    const int n = a.in->n;
    bool valid = false;
    float s = -INFINITY;
    if (r < n) {
        if (a.in->fin[r]) {
            valid = j == 0;
            s = a.in->score[r];
        } else if (j < a.W && a.list_ids[r * a.W + j] >= 0) {
            valid = true;
            s = __fadd_rn(a.in->score[r], a.list_lps[r * a.W + j]);
        }
    }
    valid = valid && s == s;                       // a NaN score has no place in an order: the item is not in the pool (beam_ref.step)
    s_score[tid] = s; s_valid[tid] = valid;
    if (tid < BEAM_MAX_W) s_sel[tid] = -1;
    __syncthreads();
    int place = 0, n_valid = 0;
    for (int o = 0; o < 64; ++o) {
        if (!s_valid[o]) continue;
        ++n_valid;
        const float os = s_score[o];
        place += (os > s || (os == s && o < tid)) ? 1 : 0;
    }
    if (valid && place < a.W) s_sel[place] = tid;
    __syncthreads();
    const int n_new = n_valid < a.W ? n_valid : a.W;
    if (tid < BEAM_MAX_W) {
        int fin = 1;
        if (tid < n_new) {
            const int it = s_sel[tid], pr = it >> 3, pj = it & 7;
            const int len = a.in->len[pr];
            const int* ii = a.in_ids + (size_t)pr * a.len_cap;
            const float* il = a.in_lps + (size_t)pr * a.len_cap;
            int* oi = a.out_ids + (size_t)tid * a.len_cap;
            float* ol = a.out_lps + (size_t)tid * a.len_cap;
            for (int k = 0; k < len; ++k) { oi[k] = ii[k]; ol[k] = il[k]; }
            int nlen = len;
            if (!a.in->fin[pr]) {
                const int tok = a.list_ids[pr * a.W + pj];
                oi[len] = tok; ol[len] = a.list_lps[pr * a.W + pj];
                nlen = len + 1;
                fin = nlen >= a.limit;
                for (int k = 0; k < a.n_eos; ++k) fin |= a.eos[k] == tok;
            }
            a.out->len[tid] = nlen; a.out->fin[tid] = fin; a.out->score[tid] = s_score[it];
        }
        s_live[tid] = !fin;
    }
    __syncthreads();
    int first = -1, n_live = 0;
    for (int c = BEAM_MAX_W - 1; c >= 0; --c) if (s_live[c]) { first = c; ++n_live; }
    if (tid < a.B && first >= 0) {
        const int c = tid < n_new && s_live[tid] ? tid : first;
        a.tok_b[tid] = a.out_ids[(size_t)c * a.len_cap + a.out->len[c] - 1];
    }
    if (tid == 0) {
        unsigned held = 0, claimed = 0;
        int n_rows = 0, np = 0;
        for (int q = 0; q < n; ++q) { held |= 1u << a.in->set_of[q]; n_rows += a.in->fin[q] ? 0 : 1; }
        for (int c = 0; c < BEAM_MAX_W; ++c) {
            if (c >= n_new) { a.rec[4 + c] = -1; a.rec[4 + BEAM_MAX_W + c] = -1; a.rec[4 + 2 * BEAM_MAX_W + c] = -1; continue; }
            const int it = s_sel[c], src = a.in->set_of[it >> 3];
            int dst = src;
            if ((claimed >> src) & 1u) {
                dst = __ffs((int)(~(held | claimed) & 0xFFFFu)) - 1;       // 16 sets, at most 8 held and 7 taken: one is always left
                for (int i = 0; i < a.n_cp; ++i) {
                    a.pair_src[np] = a.set_pages[src * a.set_stride + i];
                    a.pair_dst[np] = a.set_pages[dst * a.set_stride + i];
                    ++np;
                }
            }
            claimed |= 1u << dst;
            a.out->set_of[c] = dst;
            a.rec[4 + c] = it >> 3; a.rec[4 + BEAM_MAX_W + c] = it & 7; a.rec[4 + 2 * BEAM_MAX_W + c] = dst;
        }
        a.out->n = n_new;
        a.rec[0] = n_new; a.rec[1] = n_live; a.rec[2] = n_rows; a.rec[3] = np;
    }
}
}  // namespace
void launch_beam_select(hipStream_t s, const BeamSelectArgs& a) {
    if (a.W < 1 || a.W > BEAM_MAX_W || a.B < 1 || a.B > 64 || a.limit < 1 || a.limit > a.len_cap || a.n_cp < 0 || a.n_cp > BEAM_CP_MAX || a.n_eos < 0)
        throw std::runtime_error("beam select: W must be 1 .. 8, limit 1 .. len_cap, n_cp 0 .. 8");
    hipLaunchKernelGGL(beam_select_kernel, dim3(1), dim3(64), 0, s, a);
}

#define SVLN_INST(T)                                                                                                              \
    template void launch_rmsnorm<T>(hipStream_t, const void*, const void*, void*, int, int, float, const int*, void*, const int*, int);                              \
    template void launch_rmsnorm_indexed<T>(hipStream_t, const void*, const void*, void*, const int*, const int*, void*, int, int, float);                          \
    template void launch_layernorm<T>(hipStream_t, const void*, const void*, const void*, void*, int, int, float);               \
    template void launch_gather_rows_ragged<T>(hipStream_t, const int*, const void*, void*, int, int);                            \
    template void launch_rope_kv<T>(hipStream_t, const RopeKvArgs&);                                                              \
    template void launch_vit_kv_pack<T>(hipStream_t, const void*, int, void*, void*, int, int, int, int);                         \
    template void launch_patchify<T>(hipStream_t, const float*, void*, int, int, int, int);                                       \
    template void launch_pool<T>(hipStream_t, const void*, void*, const int*, const float*, int, int, int, int);                  \
    template void launch_gather_rows<T>(hipStream_t, const int*, const void*, const void*, void*, int, int, const int*);                      \
    template void launch_verify_step<T>(hipStream_t, const int*, const int*, const int*, int, GenCtl*, const int*, int*, int*, const void*,    \
                                        void*, int, int, int*);                                                                  \
    template void launch_draft_select<T>(hipStream_t, const DraftSelectArgs&);                                                    \
    template void launch_memory_prune<T>(hipStream_t, const void*, int, int, int, float*, float*, float*, int*);                   \
    template void launch_synth<T>(hipStream_t, void*, int, int64_t, int, RowMap, uint64_t, float, float);                          \
    template void launch_convert<T>(hipStream_t, void*, int, int64_t, int, RowMap, const void*, int);                              \
    template void launch_to_f32<T>(hipStream_t, const void*, float*, int64_t);                                                    \
    template void launch_from_f32<T>(hipStream_t, const float*, void*, int64_t);
SVLN_INST(bf16)
SVLN_INST(float)

}  // namespace svln
