// r1_device_sort.hip — the device's one prefix sum and one radix sort (r1_device_sort.h), shared by the re-sort (r1_resort.hip, DESIGN.md
// §4.29) and the regrid (r1_regrid.hip, §4.31).  THE RULE of the three files: every hand-over between workgroups is a KERNEL BOUNDARY, as
// in r1_refit.hip and for its reason (§4.10) — no look-back, no arrival counter, no lane ever waits for another workgroup's store, no
// atomic on device memory.  The prefix sum is the three-launch form — block sums, the sums' own prefix sum (the same three launches again
// where they exceed a block), apply; of the sort only `hist` goes from workgroup to workgroup, between the launches of a pass.  One lane
// per item, vector stores, plain HIP C++; nothing here is near a trace kernel.
#include <hip/hip_runtime.h>

#include "r1_device_sort.h"
#include "r1_internal.h"

// inclusive prefix sum of one value per lane over the workgroup, through LDS
__device__ inline uint32_t block_inclusive(uint32_t v, uint32_t *sh)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < R1_SORT_BLOCK; off <<= 1)
    {
        const uint32_t add = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    return sh[t];
}

// sums[block] = the sum of the block's items
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_scan_sums_kernel(const uint32_t *__restrict__ data, uint32_t n, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t sh[R1_SORT_BLOCK];
    const uint32_t i = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    const uint32_t inc = block_inclusive(i < n ? data[i] : 0u, sh);
    if (threadIdx.x == R1_SORT_BLOCK - 1)
        sums[blockIdx.x] = inc;
}

// data[i] = the sum of the items in front of i, in place: the block's own items in front of it, plus base[block] (the blocks in front; null: 0)
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_scan_apply_kernel(uint32_t *__restrict__ data, uint32_t n, const uint32_t *__restrict__ base)
{
    __shared__ uint32_t sh[R1_SORT_BLOCK];
    const uint32_t i = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    const uint32_t v = i < n ? data[i] : 0u;
    const uint32_t inc = block_inclusive(v, sh);
    if (i < n)
        data[i] = inc - v + (base ? base[blockIdx.x] : 0u);
}

extern "C" void r1_scan_enqueue(uint32_t *data, uint32_t n, uint32_t *sums, hipStream_t stream)
{
    const unsigned nb = r1_blocks(n);
    if (nb <= 1)
    {
        hipLaunchKernelGGL(r1_scan_apply_kernel, dim3(1), dim3(R1_SORT_BLOCK), 0, stream, data, n, (const uint32_t *)nullptr);
        return;
    }
    hipLaunchKernelGGL(r1_scan_sums_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, data, n, sums);
    r1_scan_enqueue(sums, nb, sums + nb, stream);
    hipLaunchKernelGGL(r1_scan_apply_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, data, n, (const uint32_t *)sums);
}

// ---- radix sort: one stable pass over an 8-bit digit is a histogram, its prefix sum and a scatter -------------------------------------------

// the items of a list: the device's count where there is one, never more than the launch is sized for
__device__ inline uint32_t radix_items(const R1RadixArgs &A) { return A.n_dev ? min(*A.n_dev, A.n_max) : A.n_max; }

// blockIdx.y: the list.  hist[(list * 256 + digit) * blocks + block] = how many of the block's keys have that digit
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_radix_hist_kernel(R1RadixArgs A, int from, uint32_t shift)
{
    __shared__ uint32_t count[256];
    const uint32_t t = threadIdx.x, i = blockIdx.x * R1_SORT_BLOCK + t, l = blockIdx.y;
    count[t] = 0u;
    __syncthreads();
    if (i < radix_items(A))
        atomicAdd(&count[(A.key[from][(size_t)l * A.n_max + i] >> shift) & 255u], 1u); // (LDS; a count does not depend on the order of its additions)
    __syncthreads();
    A.hist[(l * 256u + t) * gridDim.x + blockIdx.x] = count[t];
}

// hist holds its own exclusive prefix sum: the entry of (list, digit, block) less the list's first entry is where the block's first key of
// that digit goes; the keys of one digit keep their order within the block (the lanes in front with the same digit are counted): a stable pass
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_radix_scatter_kernel(R1RadixArgs A, int from, uint32_t shift)
{
    __shared__ uint32_t digit[R1_SORT_BLOCK];
    const uint32_t t = threadIdx.x, i = blockIdx.x * R1_SORT_BLOCK + t, l = blockIdx.y, n = radix_items(A);
    const size_t at = (size_t)l * A.n_max;
    uint32_t key = 0u, d = 256u; // (256: a lane behind the last key, no digit)
    if (i < n)
        key = A.key[from][at + i], d = (key >> shift) & 255u;
    digit[t] = d;
    __syncthreads();
    if (i >= n)
        return;
    uint32_t rank = 0u;
    for (uint32_t u = 0; u < t; ++u)
        rank += digit[u] == d ? 1u : 0u;
    const uint32_t dest = A.hist[(l * 256u + d) * gridDim.x + blockIdx.x] - A.hist[l * 256u * gridDim.x] + rank;
    if (dest < A.n_max) // (always: the counts of one list sum to its items)
    {
        A.key[1 - from][at + dest] = key;
        A.val[1 - from][at + dest] = A.val[from][at + i];
    }
}

extern "C" int r1_radix_sort_enqueue(const R1RadixArgs *a, uint32_t top_key, hipStream_t stream)
{
    const dim3 grid(r1_blocks(a->n_max), a->lists);
    int cur = 0;
    for (uint32_t shift = 0; shift == 0 || (shift < 32u && (top_key >> shift)); shift += 8u, cur ^= 1)
    {
        hipLaunchKernelGGL(r1_radix_hist_kernel, grid, dim3(R1_SORT_BLOCK), 0, stream, *a, cur, shift);
        r1_scan_enqueue(a->hist, (uint32_t)r1_radix_hist_words(a->n_max, a->lists), a->sums, stream);
        hipLaunchKernelGGL(r1_radix_scatter_kernel, grid, dim3(R1_SORT_BLOCK), 0, stream, *a, cur, shift);
    }
    return cur;
}
