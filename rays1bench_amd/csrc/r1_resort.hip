// r1_resort.hip — r1_resort_spheres: the movable spheres re-dealt into the box tree's leaf slots on the device, by the rule of
// r1_bvh_sort.h — the host restatement's own (r1_bvh.cpp r1_bvh_resort_host), id for id.  The topology, every table shape and every trace
// kernel stay; the refit that follows (r1_refit.hip) recomputes the boxes.
//
//   1. three sorted lists: the movable spheres by (key, active index) on each axis — a stable LSD radix sort, four 8-bit digits, input in
//      active order: per-block histogram, prefix sum, scatter;
//   2. per depth of the tree: every splitting node's axis from the ends of its segment in the three lists; one flag per sphere (does it go to
//      child 0?); the flags' prefix sum in each list's order; a stable partition of every segment of every list;
//   3. write-back of slot / ids / prims from the x list.
//
// Every hand-over between workgroups is a KERNEL BOUNDARY, as in r1_refit.hip and for its reason (§4.10): no look-back, no arrival counter, no
// lane ever waits for another workgroup's store.  The prefix sum is the three-launch form — block sums, the sums' own prefix sum (the same
// three launches again where they exceed a block), apply.  One lane per item, vector stores, plain HIP C++; nothing here is near a trace kernel.
#include <hip/hip_runtime.h>

#include "r1_bvh_sort.h"
#include "r1_internal.h"

#define R1_SORT_BLOCK 256 // lanes per workgroup = items per workgroup, in every kernel here: r1_sort_sums_words() and tests/test_gpu_resort.py count with it

static inline unsigned sort_blocks(uint32_t n) { return (n + R1_SORT_BLOCK - 1) / R1_SORT_BLOCK; }

// ---- prefix sum ----------------------------------------------------------------------------------------------------------------------------

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

// exclusive prefix sum of data[0, n) in place; sums: r1_sort_sums_words(n) words of scratch
static void scan_enqueue(uint32_t *data, uint32_t n, uint32_t *sums, hipStream_t stream)
{
    const unsigned nb = sort_blocks(n);
    if (nb <= 1)
    {
        hipLaunchKernelGGL(r1_scan_apply_kernel, dim3(1), dim3(R1_SORT_BLOCK), 0, stream, data, n, (const uint32_t *)nullptr);
        return;
    }
    hipLaunchKernelGGL(r1_scan_sums_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, data, n, sums);
    scan_enqueue(sums, nb, sums + nb, stream);
    hipLaunchKernelGGL(r1_scan_apply_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, data, n, (const uint32_t *)sums);
}

// the same for r1_regrid.hip
extern "C" void r1_scan_enqueue(uint32_t *data, uint32_t n, uint32_t *sums, hipStream_t stream) { scan_enqueue(data, n, sums, stream); }

// words of block sums a prefix sum over n items needs, all levels
extern "C" size_t r1_sort_sums_words(size_t n)
{
    size_t words = 0;
    while (n > R1_SORT_BLOCK)
        n = (n + R1_SORT_BLOCK - 1) / R1_SORT_BLOCK, words += n;
    return words;
}

// ---- the three sorted lists ----------------------------------------------------------------------------------------------------------------

// one lane per (axis, movable sphere): its key on that axis and itself, in active order
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_key_kernel(R1SortArgs A)
{
    const uint32_t i = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    if (i >= 3u * A.m)
        return;
    const uint32_t a = i / A.m, s = A.mov[i - a * A.m];
    A.key[0][i] = r1s_key(r1s_clamp(A.exact[4 * (size_t)s + a]));
    A.list[0][i] = s;
}

// blockIdx.y: the axis.  hist[(axis * 256 + digit) * blocks + block] = how many of the block's keys have that digit
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_hist_kernel(R1SortArgs A, int from, uint32_t shift)
{
    __shared__ uint32_t count[256];
    const uint32_t t = threadIdx.x, i = blockIdx.x * R1_SORT_BLOCK + t, a = blockIdx.y;
    count[t] = 0u;
    __syncthreads();
    if (i < A.m)
        atomicAdd(&count[(A.key[from][a * A.m + i] >> shift) & 255u], 1u);
    __syncthreads();
    A.hist[(a * 256u + t) * gridDim.x + blockIdx.x] = count[t];
}

// hist holds its own exclusive prefix sum: the entry of (axis, digit, block) less the axis' first entry is where the block's first key of that
// digit goes; the keys of one digit keep their order within the block (the lanes in front with the same digit are counted): a stable pass
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_scatter_kernel(R1SortArgs A, int from, uint32_t shift)
{
    __shared__ uint32_t digit[R1_SORT_BLOCK];
    const uint32_t t = threadIdx.x, i = blockIdx.x * R1_SORT_BLOCK + t, a = blockIdx.y;
    uint32_t key = 0u, d = 256u; // (256: a lane behind the last key, no digit)
    if (i < A.m)
        key = A.key[from][a * A.m + i], d = (key >> shift) & 255u;
    digit[t] = d;
    __syncthreads();
    if (i >= A.m)
        return;
    uint32_t rank = 0u;
    for (uint32_t u = 0; u < t; ++u)
        rank += digit[u] == d ? 1u : 0u;
    const uint32_t dest = A.hist[(a * 256u + d) * gridDim.x + blockIdx.x] - A.hist[a * 256u * gridDim.x] + rank;
    if (dest < A.m) // (always: the counts of one axis sum to m)
    {
        A.key[1 - from][a * A.m + dest] = key;
        A.list[1 - from][a * A.m + dest] = A.list[from][a * A.m + i];
    }
}

// ---- per depth ---------------------------------------------------------------------------------------------------------------------------------

// one lane per splitting node of the depth, seg[begin, end): the axis on which its spheres reach furthest
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_axis_kernel(R1SortArgs A, int cur, uint32_t begin, uint32_t end)
{
    const uint32_t g = begin + blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    if (g >= end)
        return;
    const R1SortSeg sg = A.seg[g];
    float first[3], last[3];
    for (uint32_t a = 0; a < 3u; ++a)
    {
        const uint32_t *l = A.list[cur] + a * A.m;
        first[a] = r1s_clamp(A.exact[4 * (size_t)l[sg.b] + a]), last[a] = r1s_clamp(A.exact[4 * (size_t)l[sg.e - 1u] + a]);
    }
    A.seg_axis[g] = (uint32_t)r1s_axis(first, last);
}

// one lane per position: the sphere there in its node's chosen list goes to child 0 if it stands among the first k of the segment
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_flag_kernel(R1SortArgs A, int cur, const uint32_t *__restrict__ pos_seg)
{
    const uint32_t p = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    if (p >= A.m)
        return;
    const uint32_t g = pos_seg[p];
    if (g == R1S_NONE)
        return;
    const R1SortSeg sg = A.seg[g];
    A.flag[A.list[cur][A.seg_axis[g] * A.m + p]] = p < sg.b + sg.k ? 1u : 0u;
}

// one lane per entry of the three lists: its sphere's flag, in list order (0 outside every splitting node)
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_gather_kernel(R1SortArgs A, int cur, const uint32_t *__restrict__ pos_seg)
{
    const uint32_t i = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    if (i >= 3u * A.m)
        return;
    const uint32_t p = i % A.m;
    A.scan[i] = pos_seg[p] != R1S_NONE ? A.flag[A.list[cur][i]] : 0u;
}

// one lane per entry of the three lists: the stable partition of its segment (r1s_dest); entries outside every splitting node stay
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_partition_kernel(R1SortArgs A, int cur, const uint32_t *__restrict__ pos_seg)
{
    const uint32_t i = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    if (i >= 3u * A.m)
        return;
    const uint32_t p = i % A.m, at = i - p, g = pos_seg[p], s = A.list[cur][i];
    if (g == R1S_NONE)
    {
        A.list[1 - cur][i] = s;
        return;
    }
    const R1SortSeg sg = A.seg[g];
    const uint32_t dest = r1s_dest(sg.b, sg.k, p, A.scan[i] - A.scan[at + sg.b], A.flag[s] != 0u);
    if (dest < A.m) // (always: every list holds the same spheres in [b, e), k of them flagged)
        A.list[1 - cur][at + dest] = s;
}

// ---- write-back ------------------------------------------------------------------------------------------------------------------------------

// one lane per position: the sphere the x list has there moves into the position's slot — ids, the slot table, centre and radius_sq from exact
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_sort_write_kernel(R1SortArgs A, int cur)
{
    const uint32_t p = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    if (p >= A.m)
        return;
    const uint32_t s = A.list[cur][p], q = A.mslot[p];
    A.ids[q] = s;
    A.slot[s] = q;
    const float *e = A.exact + 4 * (size_t)s;
    float *pr = A.prims + 8 * (size_t)(q >> 1) + (q & 1u);
    pr[0] = e[0], pr[2] = e[1], pr[4] = e[2], pr[6] = e[3];
}

// depth_off: [depths + 1] (host memory) offsets of each depth's splitting nodes in seg.  a->m > 0.
extern "C" hipError_t r1_launch_resort(const R1SortArgs *a, const uint32_t *depth_off, uint32_t depths, hipStream_t stream)
{
    const uint32_t m = a->m, nb = sort_blocks(m), nb3 = sort_blocks(3u * m);
    hipLaunchKernelGGL(r1_sort_key_kernel, dim3(nb3), dim3(R1_SORT_BLOCK), 0, stream, *a);
    int cur = 0;
    for (uint32_t shift = 0; shift < 32u; shift += 8u, cur ^= 1)
    {
        hipLaunchKernelGGL(r1_sort_hist_kernel, dim3(nb, 3), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, shift);
        scan_enqueue(a->hist, 3u * 256u * nb, a->sums, stream);
        hipLaunchKernelGGL(r1_sort_scatter_kernel, dim3(nb, 3), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, shift);
    }
    for (uint32_t d = 0; d < depths; ++d, cur ^= 1)
    {
        const uint32_t *pos_seg = a->pos_seg + (size_t)d * m;
        hipLaunchKernelGGL(r1_sort_axis_kernel, dim3(sort_blocks(depth_off[d + 1] - depth_off[d])), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, depth_off[d],
                           depth_off[d + 1]);
        hipLaunchKernelGGL(r1_sort_flag_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, pos_seg);
        hipLaunchKernelGGL(r1_sort_gather_kernel, dim3(nb3), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, pos_seg);
        scan_enqueue(a->scan, 3u * m, a->sums, stream);
        hipLaunchKernelGGL(r1_sort_partition_kernel, dim3(nb3), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, pos_seg);
    }
    hipLaunchKernelGGL(r1_sort_write_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, *a, cur);
    return hipGetLastError();
}
