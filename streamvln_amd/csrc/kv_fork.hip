// Fork of one KV page (svln_generate_group): the partly filled page of a prompt is copied, in every layer's K and V^T pool, to the
// private pages of the other sequences of the group -- one launch per group turn.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace svln {

// pools[p] (p < gridDim.y): base of one pool, pages of `chunks` 16-byte chunks each.  Thread (blockIdx.x * 256 + threadIdx.x) owns one
// chunk of the page: it is loaded from page `src` ONCE and stored to the n_dst pages of `dst` (distinct, none equal to src: checked by
// the host, as are the page bounds).  A page is nkv x 64 x 128 elements of T in either pool (K [nkv][64][128], V^T [nkv][128][64]).
template <typename T>
__global__ void __launch_bounds__(256) kv_page_copy_kernel(T* const* __restrict__ pools, int src, const int* __restrict__ dst, int n_dst, int chunks) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    uint4* base = reinterpret_cast<uint4*>(pools[blockIdx.y]);
    const uint4 v = base[(size_t)src * chunks + c];
    for (int d = 0; d < n_dst; ++d) base[(size_t)dst[d] * chunks + c] = v;
}

// True size (4 kv heads, bf16): 4096 chunks per page x 56 pools = 896 workgroups of 256 threads, one chunk per thread -- under the
// ~2048-workgroup cap of a memory-bound grid, so no grid-stride loop; 64 KB read + n_dst x 64 KB written per pool.
template <typename T> void launch_kv_page_copy(hipStream_t s, void* const* pools, int n_pools, int src_page, const int* dst_pages, int n_dst,
                                               int64_t page_elems) {
    if (n_pools <= 0 || n_dst <= 0) return;
    const int chunks = (int)(page_elems / Elt<T>::PER_CHUNK);
    hipLaunchKernelGGL((kv_page_copy_kernel<T>), dim3((chunks + 255) / 256, n_pools), dim3(256), 0, s, (T* const*)pools, src_page, dst_pages, n_dst,
                       chunks);
}

template void launch_kv_page_copy<bf16>(hipStream_t, void* const*, int, int, const int*, int, int64_t);
template void launch_kv_page_copy<float>(hipStream_t, void* const*, int, int, const int*, int, int64_t);

// The hand-over of a beam step: the copy above with one source per destination.  blockIdx.z = the pair: page src[z] -> page dst[z] of
// pool blockIdx.y.  No page is both read and written (checked by the host, as are the bounds and the distinct destinations), so the
// pairs are independent; a source that serves several destinations is read once per pair (64 KB at the true size; supposed, not
// measured: the repeats hit L2).
template <typename T>
__global__ void __launch_bounds__(256) kv_page_gather_kernel(T* const* __restrict__ pools, const int* __restrict__ src, const int* __restrict__ dst,
                                                             int chunks) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    uint4* base = reinterpret_cast<uint4*>(pools[blockIdx.y]);
    base[(size_t)dst[blockIdx.z] * chunks + c] = base[(size_t)src[blockIdx.z] * chunks + c];
}

template <typename T> void launch_kv_page_gather(hipStream_t s, void* const* pools, int n_pools, const int* src_pages, const int* dst_pages, int n,
                                                 int64_t page_elems) {
    if (n_pools <= 0 || n <= 0) return;
    const int chunks = (int)(page_elems / Elt<T>::PER_CHUNK);
    hipLaunchKernelGGL((kv_page_gather_kernel<T>), dim3((chunks + 255) / 256, n_pools, n), dim3(256), 0, s, (T* const*)pools, src_pages, dst_pages,
                       chunks);
}

template void launch_kv_page_gather<bf16>(hipStream_t, void* const*, int, const int*, const int*, int, int64_t);
template void launch_kv_page_gather<float>(hipStream_t, void* const*, int, const int*, const int*, int, int64_t);

}  // namespace svln
