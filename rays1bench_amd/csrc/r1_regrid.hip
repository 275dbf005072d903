// r1_regrid.hip — r1_regrid: the moved spheres re-registered in the uniform grid on the device, by the rule of
// r1_grid_fill.h — the host restatement's own (r1_grid.cpp r1_grid_regrid_host), byte for byte.  The plan of the build stays, every table
// keeps its place and shape, no trace or query kernel changes: they read the tables, n_out and the far test's box from device memory.
//
//   1. classify: one lane per active sphere — outlier, registered (and in how many cells) or neither; the workgroup's extents;
//   2. reduce the extents: the far test's box and the flat axes' one cell, into both R1GridArgs;
//   3. prefix sums of the cell counts and of the outlier flags; the total against the capacity, n_out and v2 into both R1GridArgs;
//   4. emit the (cell, id) pairs at each sphere's offset, in sphere order, and the outlier list;
//   5. sort the pairs by cell: a stable LSD radix sort, as many 8-bit passes as the cell index needs — ids ascend within a cell;
//   6. write back: a cell's start by binary search in the sorted keys, the ids, zeros behind them; 32-bit table and (small form) 16-bit.
//
// Every hand-over between workgroups is a KERNEL BOUNDARY: the rule at the top of r1_device_sort.hip, whose prefix sum and radix sort these
// steps use.  The pair count lives in device memory only: every kernel behind step 3 is launched for the capacity and reads the count (0 on
// overflow) — nothing is read back, nothing is written past the capacity.  One lane per item, vector stores, plain HIP C++.
#include <hip/hip_runtime.h>

#include "r1_device_sort.h"
#include "r1_grid_fill.h"
#include "r1_internal.h"

// the workgroup's minimum (is_min) or maximum of one value per lane, in every lane
__device__ inline double block_extreme(double v, bool is_min, double *sh)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t off = R1_SORT_BLOCK / 2; off > 0; off >>= 1)
    {
        if (t < off)
        {
            const double o = sh[t + off];
            sh[t] = is_min ? r1f_min(sh[t], o) : r1f_max(sh[t], o);
        }
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// the workgroup's extent from its lanes', in every lane
__device__ inline void block_extent(R1GridExtent &e, double *sh)
{
    for (int a = 0; a < 3; ++a)
    {
        e.rlo[a] = block_extreme(e.rlo[a], true, sh), e.rhi[a] = block_extreme(e.rhi[a], false, sh);
        e.clo[a] = block_extreme(e.clo[a], true, sh), e.chi[a] = block_extreme(e.chi[a], false, sh);
    }
    e.rho_max = block_extreme(e.rho_max, false, sh);
}

// ---- 1. classify ---------------------------------------------------------------------------------------------------------------------------

// one lane per active sphere and one behind the last (entry na of span and oflag: 0, the prefix sums' total goes there)
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_regrid_classify_kernel(R1RegridArgs A)
{
    __shared__ double sh[R1_SORT_BLOCK];
    const uint32_t i = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    R1GridExtent e;
    e.clear();
    if (i <= A.na)
    {
        uint32_t span = 0u, klass = R1GF_NONE;
        if (i < A.na)
        {
            const float *x = A.exact + 4 * (size_t)i;
            double rho;
            bool cand;
            klass = r1gf_classify(A.plan, x[0], x[1], x[2], A.radii[2 * (size_t)i], A.radii[2 * (size_t)i + 1], rho, span, cand);
            e.add(x[0], x[1], x[2], rho, cand, klass == R1GF_CANDIDATE);
        }
        A.span[i] = span;
        A.oflag[i] = klass == R1GF_OUTLIER ? 1u : 0u;
    }
    block_extent(e, sh);
    if (threadIdx.x == 0)
    {
        double *p = A.part + (size_t)R1GF_EXTENT_WORDS * blockIdx.x;
        for (int a = 0; a < 3; ++a)
            p[a] = e.rlo[a], p[3 + a] = e.rhi[a], p[6 + a] = e.clo[a], p[9 + a] = e.chi[a];
        p[12] = e.rho_max;
    }
}

// ---- 2. the geometry -------------------------------------------------------------------------------------------------------------------------

__device__ inline void put_geometry(R1GridArgs *g, const float lo[3], const float cell[3], const float inv_cell[3], const float clo[3], const float chi[3])
{
    for (int a = 0; a < 3; ++a)
        g->geom.lo[a] = lo[a], g->geom.cell[a] = cell[a], g->geom.inv_cell[a] = inv_cell[a], g->geom.clo[a] = clo[a], g->geom.chi[a] = chi[a];
}

// one workgroup: the `blocks` extents of step 1 merged; lane 0 writes the geometry into both R1GridArgs
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_regrid_geometry_kernel(R1RegridArgs A, uint32_t blocks)
{
    __shared__ double sh[R1_SORT_BLOCK];
    R1GridExtent e;
    e.clear();
    for (uint32_t b = threadIdx.x; b < blocks; b += R1_SORT_BLOCK)
    {
        const double *p = A.part + (size_t)R1GF_EXTENT_WORDS * b;
        R1GridExtent o;
        for (int a = 0; a < 3; ++a)
            o.rlo[a] = p[a], o.rhi[a] = p[3 + a], o.clo[a] = p[6 + a], o.chi[a] = p[9 + a];
        o.rho_max = p[12];
        e.merge(o);
    }
    block_extent(e, sh);
    if (threadIdx.x != 0)
        return;
    float lo[3], cell[3], inv_cell[3], clo[3], chi[3];
    r1gf_geometry(A.plan, e, lo, cell, inv_cell, clo, chi);
    put_geometry(A.g16, lo, cell, inv_cell, clo, chi);
    put_geometry(A.g32, lo, cell, inv_cell, clo, chi);
}

// ---- 3. the totals -----------------------------------------------------------------------------------------------------------------------------

// one lane: behind the prefix sums.  The pair count every later kernel works with, n_out and v2
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_regrid_total_kernel(R1RegridArgs A)
{
    if (blockIdx.x != 0 || threadIdx.x != 0)
        return;
    const uint32_t total = A.span[A.na], n_out = A.oflag[A.na];
    const bool overflow = total > A.cap;
    A.stat[R1GF_STAT_PAIRS] = overflow ? 0u : total;
    A.stat[R1GF_STAT_OVERFLOW] = overflow ? 1u : 0u;
    A.stat[R1GF_STAT_TOTAL] = total;
    A.stat[3] = n_out;
    // overflow: v2 = -1 makes r1g_far true for every origin, every ray takes the tree fallback — exact, only slow.  Nothing registered:
    // every origin is safe, as the builder has it
    const float v2 = overflow ? -1.0f : (total ? A.plan.v2 : __builtin_inff());
    A.g16->n_out = n_out, A.g32->n_out = n_out;
    A.g16->geom.v2 = v2, A.g32->geom.v2 = v2;
}

// ---- 4. emit -----------------------------------------------------------------------------------------------------------------------------------

// one lane per active sphere: its pairs at its offset (its cells again: the count is the first pass's), its place in the outlier list
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_regrid_emit_kernel(R1RegridArgs A)
{
    const uint32_t i = blockIdx.x * R1_SORT_BLOCK + threadIdx.x;
    if (i >= A.na)
        return;
    const uint32_t at = A.span[i], n = A.span[i + 1u] - at;
    if (n && n <= R1_GRID_SPAN_LIMIT && !A.stat[R1GF_STAT_OVERFLOW] && at <= A.cap && n <= A.cap - at) // (the last two: always, the total is within the capacity)
    {
        const float *x = A.exact + 4 * (size_t)i;
        const double rho = r1gf_rho(x[0], x[1], x[2], A.radii[2 * (size_t)i + 1], A.plan.V, A.plan.delta);
        r1gf_cells(A.plan, x[0], x[1], x[2], rho, A.key[0] + at, A.val[0] + at, i);
    }
    const uint32_t o = A.oflag[i];
    if (A.oflag[i + 1u] != o && o < A.na) // (o < na: always)
        A.outliers[o] = i;
}

// ---- 6. write-back -------------------------------------------------------------------------------------------------------------------------------

// one lane per table entry: cell q's start = the first sorted pair whose cell is >= q (entry cells: the pair count); then the ids, zeros behind
// them up to the capacity and (16-bit table) to the end of its last 16-byte row
__global__ void __launch_bounds__(R1_SORT_BLOCK) r1_regrid_write_kernel(R1RegridArgs A, int cur)
{
    const uint32_t idx = blockIdx.x * R1_SORT_BLOCK + threadIdx.x, n = A.stat[R1GF_STAT_PAIRS], n_start = A.plan.n_start, words = n_start + A.cap;
    uint32_t v = 0u;
    if (idx < n_start)
    {
        const uint32_t *key = A.key[cur];
        uint32_t lo = 0u, hi = n; // the answer is in [lo, hi]
        while (lo < hi)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (key[mid] < idx)
                lo = mid + 1u;
            else
                hi = mid;
        }
        v = lo;
    }
    else if (idx < words)
    {
        const uint32_t k = idx - n_start;
        v = k < n ? A.val[cur][k] : 0u;
    }
    if (idx < words)
        A.tab32[idx] = v;
    if (A.small && idx < A.tab16_halves)
        A.tab16[idx] = (uint16_t)v;
}

// a->na > 0.  Everything on `stream`, nothing waited for.
extern "C" hipError_t r1_launch_regrid(const R1RegridArgs *a, hipStream_t stream)
{
    const unsigned nb = r1_blocks((size_t)a->na + 1u);
    hipLaunchKernelGGL(r1_regrid_classify_kernel, dim3(nb), dim3(R1_SORT_BLOCK), 0, stream, *a);
    hipLaunchKernelGGL(r1_regrid_geometry_kernel, dim3(1), dim3(R1_SORT_BLOCK), 0, stream, *a, (uint32_t)nb);
    r1_scan_enqueue(a->span, a->na + 1u, a->sums, stream);
    r1_scan_enqueue(a->oflag, a->na + 1u, a->sums, stream);
    hipLaunchKernelGGL(r1_regrid_total_kernel, dim3(1), dim3(R1_SORT_BLOCK), 0, stream, *a);
    hipLaunchKernelGGL(r1_regrid_emit_kernel, dim3(r1_blocks(a->na)), dim3(R1_SORT_BLOCK), 0, stream, *a);
    // 5. the sort: the device's count of pairs, keys up to the largest cell index (n_start = cells + 1 >= 2)
    const R1RadixArgs pairs = {{a->key[0], a->key[1]}, {a->val[0], a->val[1]}, a->hist, a->sums, a->cap, 1u, a->stat + R1GF_STAT_PAIRS};
    const int cur = r1_radix_sort_enqueue(&pairs, a->plan.n_start - 2u, stream);
    const size_t entries = a->small && a->tab16_halves > a->plan.n_start + a->cap ? a->tab16_halves : (size_t)a->plan.n_start + a->cap;
    hipLaunchKernelGGL(r1_regrid_write_kernel, dim3(r1_blocks(entries)), dim3(R1_SORT_BLOCK), 0, stream, *a, cur);
    return hipGetLastError();
}
