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
// Every hand-over between workgroups is a KERNEL BOUNDARY: the rule at the top of r1_device_sort.hip, whose prefix sum and radix sort these
// steps use.  One lane per item, vector stores, plain HIP C++; nothing here is near a trace kernel.
#include <hip/hip_runtime.h>

#include "r1_bvh_sort.h"
#include "r1_device_sort.h"
#include "r1_internal.h"

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
    const uint32_t m = a->m, nb = r1_blocks(m), nb3 = r1_blocks(3u * m);
    hipLaunchKernelGGL(r1_sort_key_kernel, dim3(nb3), dim3(R1_SORT_BLOCK), 0, stream, *a);
    const R1RadixArgs keys = {{a->key[0], a->key[1]}, {a->list[0], a->list[1]}, a->hist, a->sums, m, 3u, nullptr};
    int cur = r1_radix_sort_enqueue(&keys, 0xFFFFFFFFu, stream); // (a key is any 32 bits: four passes)
    for (uint32_t d = 0; d < depths; ++d, cur ^= 1)
    {
        const uint32_t *pos_seg = a->pos_seg + (size_t)d * m;
        hipLaunchKernelGGL(r1_sort_axis_kernel, dim3(r1_blocks(depth_off[d + 1] - depth_off[d])), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, depth_off[d],
                           depth_off[d + 1]);
        hipLaunchKernelGGL(r1_sort_flag_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, pos_seg);
        hipLaunchKernelGGL(r1_sort_gather_kernel, dim3(nb3), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, pos_seg);
        r1_scan_enqueue(a->scan, 3u * m, a->sums, stream);
        hipLaunchKernelGGL(r1_sort_partition_kernel, dim3(nb3), dim3(R1_SORT_BLOCK), 0, stream, *a, cur, pos_seg);
    }
    hipLaunchKernelGGL(r1_sort_write_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, *a, cur);
    return hipGetLastError();
}
