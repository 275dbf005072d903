// r1_trace_rays.hip — path queries (r1_trace_rays, r1_trace_rays_device): the reference's color(Ray(o, d), scene, 0)
// (rayweek1.cpp:517-534) for caller-supplied rays and caller-supplied stream states.  The cast kernels' loops (r1_cast.hip) with a path
// to shade: a lane loads its ray (two 16-byte loads) and its seed (one), walks (bvh_advance, grid_trace or sweep_reference of
// r1_trace.hpp, as they are), calls shade_level, and then either starts the next walk of the same path or writes one 16-byte record
// {r, g, b, color() invocations} and takes the next ray.  Same walks and same shade_level as the trace kernels, so the same bits.
//
// The attenuation stack is shade_level<true>'s: one hit index per entry in a global workspace laid out [entry][thread of the launch]
// (coalesced; r1_queries.cpp sizes it max_bounces x threads).  It needs no LDS, so these kernels keep the cast kernels' LDS budget, and
// it holds 32-bit indices, so small and big scenes share the code.
// t_max of a ray is ignored: color() always passes FLT_MAX (rayweek1.cpp:519).  A ray with a non-finite origin or (normalised)
// direction runs no color(): its record is {0, 0, 0, 0} (path_load's rule is cast_load's).  A stream state of zero is replaced before
// the path starts (r1_seed_guard, rays1_seed.h): xorshift32 stays at zero for ever and random_in_unit_sphere would never return.
#include "r1_trace.hpp"
#include "r1_internal.h"

#ifndef R1_PATHQ_WAVES
#define R1_PATHQ_WAVES 6 // the occupancy bound the compiler is given for the tree and grid kernels.  They come to 58 .. 60 VGPRs under it, so eight waves per
#endif                   // SIMD fit all the same; asked for eight, the compiler parks 12 .. 20 SGPRs in VGPR lanes (44 .. 48 v_readlane / v_writelane in the
                         // loops) to reach the same register count (profiles/r14/trace_rays_kernel_meta.txt)

namespace
{

__device__ __forceinline__ bool pathq_finite(const float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// ray i of the launch: the path at depth 0; false: the ray runs no color()
__device__ __forceinline__ bool pathq_load(const R1TraceRaysArgs &A, const uint32_t i, Path &p)
{
    const float4 a = A.rays[2 * (size_t)i], b = A.rays[2 * (size_t)i + 1];
    p.o = mk(a.x, a.y, a.z);
    p.d = vunit(mk(b.x, b.y, b.z)); // Ray::Ray, rayweek1.cpp:107
    r1_sample_seed sd;
    if (A.seeds)                    // (wave-uniform)
    {
        const uint4 s = A.seeds[i];
        sd.scalar = s.x, sd.lane0 = s.y, sd.lane1 = s.z, sd.lane2 = s.w;
    }
    else
        sd = r1_seed_sample(0u, A.first + i, 0u);
    sd = r1_seed_guard(sd);
    p.s_scalar = sd.scalar, p.s0 = sd.lane0, p.s1 = sd.lane1, p.s2 = sd.lane2;
    p.k = i, p.depth = 0, p.sp = 0;
    return pathq_finite(p.o.x) && pathq_finite(p.o.y) && pathq_finite(p.o.z) && pathq_finite(p.d.x) && pathq_finite(p.d.y) && pathq_finite(p.d.z);
}

__device__ __forceinline__ void pathq_store(const R1TraceRaysArgs &A, const uint32_t i, const V3 col, const uint32_t rays)
{
    A.out[i] = make_float4(col.x, col.y, col.z, __uint_as_float(rays));
}

} // namespace

// ---- box tree ---------------------------------------------------------------------------------------------------------------------------
// r1_cast_tree_kernel's loop — persistent waves, chunks of the ray array from one atomic cursor, bvh_advance with CARRY — where a lane
// whose walk is complete shades: a path that goes on starts its next walk at the root next to the walks the wave carries, a path that
// has ended writes its record and the lane refills.  The node table is staged in LDS exactly as r1_cast_tree_kernel stages it.
template <bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, R1_PATHQ_WAVES) r1_pathq_tree_kernel(const R1TraceRaysArgs A)
{
    constexpr bool LN = !BIG;
    typedef typename IdxType<!LN>::type TS; // traversal-stack entry: uint16_t with the LDS table, else uint32_t
    extern __shared__ uint32_t s_trav[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t gtid = blockIdx.x * R1_BLOCK + threadIdx.x;
    const size_t trav_words = (size_t)A.t.bvh_depth * R1_BLOCK * sizeof(TS) / 4;
    const float4 *lnodes = (const float4 *)(s_trav + trav_words);
    const uint32_t top = LN ? 0u : A.t.bvh_lds_f4 >> 2;
    {
        float4 *dst = (float4 *)(s_trav + trav_words);
        for (uint32_t i = (uint32_t)tid; i < A.t.bvh_lds_f4; i += R1_BLOCK)
        {
            float4 q = A.t.scene.bvh_nodes[i];
            if (LN && (i & 3u) == 3u) // {A K child0 child1}: 16-bit child references
                q.z = __uint_as_float(r1_ref16(__float_as_uint(q.z))), q.w = __uint_as_float(r1_ref16(__float_as_uint(q.w)));
            dst[i] = q;
        }
        // (written by the threads that copied those rows: program order)
        if (LN && tid == 3)
            ((float *)dst)[13] = __uint_as_float(A.t.scene.bvh_root_leaf | (A.t.scene.bvh_flat_e >= 0.0f ? 4u : 0u));
        if (LN && tid == 7 && A.t.scene.bvh_flat_e >= 0.0f)
            ((float *)dst)[28] = A.t.scene.bvh_flat_m, ((float *)dst)[29] = A.t.scene.bvh_flat_e;
        __syncthreads();
    }

    Path p;
    p.o = mk(0, 0, 0), p.d = mk(0, 0, 1);
    p.s_scalar = p.s0 = p.s1 = p.s2 = 1u, p.k = 0u, p.depth = 0, p.sp = 0;
    bool alive = false;
    Trav tv;
    trav_start(tv);
    tv.cur = R1_BVH_DONE;
    uint32_t q_next = 0, q_end = 0;
    bool exhausted = false;
    for (;;)
    {
        // ---- refill: the lanes without a path take the next rays of the wave's chunk ----
        unsigned long long need = __ballot(!alive);
        while (need)
        {
            if (q_next == q_end)
            {
                if (exhausted)
                    break;
                if (!chunk_claim(A.cursor, A.claim, A.n, lane, q_next, q_end))
                {
                    exhausted = true;
                    break;
                }
            }
            const uint32_t avail = q_end - q_next;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            if (!alive && rank < avail)
            {
                alive = pathq_load(A, q_next + rank, p);
                if (alive)
                    trav_start(tv);
                else
                    pathq_store(A, p.k, mk(0, 0, 0), 0u); // no color(); the lane asks again
            }
            q_next += min((uint32_t)__popcll(need), avail);
            need = __ballot(!alive);
        }
        const unsigned long long live = __ballot(alive);
        if (live == 0ull)
            break;
        // ---- walk with carry-over, then one color() level for the lanes whose walk is complete ----
        bvh_advance<false, true, LN, TS>(A.t.scene, p.o, p.d, tv, (TS *)s_trav, tid, (uint32_t)__popcll(live), nullptr, lnodes, top);
        if (alive && tv.cur == R1_BVH_DONE)
        {
            V3 col;
            const int hit = tv.best_id != 0xFFFFFFFFu ? (int)tv.best_id : -1;
            if (shade_level<true>(A.t, p, hit, tv.best, nullptr, A.gstride, gtid, tid, col))
            {
                pathq_store(A, p.k, col, path_rays(p));
                alive = false;
            }
            else
                trav_start(tv); // the scattered ray starts its walk at the root
        }
    }
}

// ---- uniform grid -----------------------------------------------------------------------------------------------------------------------
// r1_cast_grid_kernel's shape: grid_trace is a complete walk per call, so a wave works its chunk off 64 rays at a time and loops over
// the bounces of those 64 paths until the last of them has ended.
template <bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, R1_PATHQ_WAVES) r1_pathq_grid_kernel(const R1TraceRaysArgs A)
{
    extern __shared__ uint32_t s_trav[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t gtid = blockIdx.x * R1_BLOCK + threadIdx.x;
    const size_t gtrav_words = (size_t)A.t.bvh_depth * R1_BLOCK;
    const uint16_t *ltab = (const uint16_t *)(s_trav + gtrav_words);
    if (!BIG)
    {
        float4 *dst = (float4 *)(s_trav + gtrav_words);
        const R1GridCArgs *ga = (const R1GridCArgs *)(uintptr_t)A.t.grid;
        const float4 *src = (const float4 *)(const r1_gu32 *)ga->tab;
        const uint32_t n16 = ga->lds_bytes / 16u;
        for (uint32_t i = (uint32_t)tid; i < n16; i += R1_BLOCK)
            dst[i] = src[i];
        __syncthreads();
    }
    uint32_t q_next = 0, q_end = 0;
    for (;;)
    {
        if (q_next == q_end && !chunk_claim(A.cursor, A.claim, A.n, lane, q_next, q_end))
            break;
        const uint32_t ray = q_next + (uint32_t)lane;
        const bool mine = ray < q_end;
        q_next = min(q_next + 64u, q_end);
        Path p;
        p.o = mk(0, 0, 0), p.d = mk(0, 0, 1);
        p.s_scalar = p.s0 = p.s1 = p.s2 = 1u, p.k = 0u, p.depth = 0, p.sp = 0;
        bool alive = false;
        if (mine)
        {
            alive = pathq_load(A, ray, p);
            if (!alive)
                pathq_store(A, ray, mk(0, 0, 0), 0u);
        }
        while (__ballot(alive) != 0ull)
        {
            float best;
            uint32_t best_id;
            const bool fb = grid_trace<false, !BIG>(A.t, (R1GridCArgs *)(uintptr_t)A.t.grid, alive, p.o, p.d, best, best_id, ltab, tid, nullptr);
            if (__ballot(fb) != 0ull)
            {
                // fallback: the tree walk from scratch, exact for any origin; the outliers' offer is kept (the tree presents them again)
                Trav fv;
                trav_start(fv);
                fv.best = best, fv.best_id = best_id;
                if (!fb)
                    fv.cur = R1_BVH_DONE;
                bvh_advance<false, false, false, uint32_t>(A.t.scene, p.o, p.d, fv, s_trav, tid, 64u, nullptr, nullptr);
                best = fv.best, best_id = fv.best_id;
            }
            if (alive)
            {
                V3 col;
                const int hit = best_id != 0xFFFFFFFFu ? (int)best_id : -1;
                if (shade_level<true>(A.t, p, hit, best, nullptr, A.gstride, gtid, tid, col))
                {
                    pathq_store(A, ray, col, path_rays(p));
                    alive = false;
                }
            }
        }
    }
}

// ---- reference form: every active sphere through exact_test in index order, level by level (the on-device cross-check) -------------------
__global__ void __launch_bounds__(R1_BLOCK) r1_pathq_reference_kernel(const R1TraceRaysArgs A)
{
    const uint32_t stride = gridDim.x * R1_BLOCK;
    const uint32_t gtid = blockIdx.x * R1_BLOCK + threadIdx.x;
    for (uint32_t i = gtid; i < A.n; i += stride)
    {
        Path p;
        V3 col = mk(0, 0, 0);
        uint32_t rays = 0u;
        if (pathq_load(A, i, p))
        {
            for (;;)
            {
                float t_hit = FLT_MAX;
                int hit = -1;
                sweep_reference(A.t.scene, p.o, p.d, t_hit, hit);
                if (shade_level<true>(A.t, p, hit, t_hit, nullptr, A.gstride, gtid, (int)threadIdx.x, col))
                    break;
            }
            rays = path_rays(p);
        }
        pathq_store(A, i, col, rays);
    }
}

// ---- launchers (called from r1_queries.cpp) --------------------------------------------------------------------------------------------------
// variant: R1_V_TREE, R1_V_GRID or R1_V_REFERENCE — the structure the rays walk
#define R1_PATHQ_DISPATCH(X)                                                                                                           \
    if (variant == R1_V_REFERENCE)                                                                                                     \
        X(r1_pathq_reference_kernel);                                                                                                  \
    else if (variant == R1_V_GRID && big)                                                                                              \
        X(r1_pathq_grid_kernel<true>);                                                                                                 \
    else if (variant == R1_V_GRID)                                                                                                     \
        X(r1_pathq_grid_kernel<false>);                                                                                                \
    else if (variant == R1_V_TREE && big)                                                                                              \
        X(r1_pathq_tree_kernel<true>);                                                                                                 \
    else if (variant == R1_V_TREE)                                                                                                     \
        X(r1_pathq_tree_kernel<false>);

extern "C" hipError_t r1_launch_trace_rays(const R1TraceRaysArgs *args, int variant, int big, int blocks, size_t dyn_lds, hipStream_t stream)
{
    if (variant != R1_V_REFERENCE && variant != R1_V_TREE && variant != R1_V_GRID)
        return hipErrorInvalidValue;
#define R1_GO(K) hipLaunchKernelGGL((K), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args)
    R1_PATHQ_DISPATCH(R1_GO)
#undef R1_GO
    return hipGetLastError();
}

extern "C" hipError_t r1_trace_rays_occupancy(int variant, int big, size_t dyn_lds, int *blocks_per_cu)
{
#define R1_OCC(K) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (K), R1_BLOCK, dyn_lds)
    R1_PATHQ_DISPATCH(R1_OCC)
#undef R1_OCC
    return hipErrorInvalidValue;
}
