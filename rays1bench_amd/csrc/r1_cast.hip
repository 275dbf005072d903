// r1_cast.hip — ray queries (r1_cast_rays, r1_cast_rays_device): Hitable::hit(Ray(o, d), 0.001f, t_max, &rec) of the
// reference (rayweek1.cpp:104-108, :152-339) for caller-supplied rays, through the same walks as the trace kernels (r1_trace.hpp:
// bvh_advance, grid_trace, sweep_reference) without color().  A lane loads its ray as two 16-byte loads, normalises it as the Ray
// constructor does (vunit), walks, and writes one 32-byte record (R1_CAST_CLOSEST) or one byte (R1_CAST_ANY).
//
// t_max is strict (rayweek1.cpp:298, :307: `temp < t_max`).  A sphere's offer is fixed before the compare with t_max (the comment above
// exact_offer), so the answer is the minimum offer, ties to the lowest index, IF it is < t_max.  The tree walk is seeded with best = t_max
// so that it prunes what lies beyond; the walks' update rule (t < best) | (t == best & id < best_id) starts at best_id = 0xFFFFFFFF and
// so admits an offer EQUAL to t_max — which is why every form ends in cast_store's `best < t_max`: an admitted t == t_max is a miss, and
// anything below it replaces it by the same rule.  The grid's walk starts at FLT_MAX and is filtered the same way.
// A ray with a non-finite origin or (normalised) direction, or a t_max that is NaN or <= 0.001, is a miss before any walk (cast_load).
#include "r1_trace.hpp"
#include "r1_internal.h"

#ifndef R1_CAST_WAVES_SMALL
#define R1_CAST_WAVES_SMALL 8 // waves per SIMD the small-scene kernels are built for (registers, LDS: profiles/r10/cast.txt)
#endif
#ifndef R1_CAST_WAVES_BIG
#define R1_CAST_WAVES_BIG 8
#endif

namespace
{

__device__ __forceinline__ bool cast_finite(const float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// ray i: origin, unit direction, t_max (+inf -> FLT_MAX); false: the ray is a miss without a walk
__device__ __forceinline__ bool cast_load(const R1CastArgs &A, const uint32_t i, V3 &o, V3 &d, float &t_max)
{
    const float4 a = A.rays[2 * (size_t)i], b = A.rays[2 * (size_t)i + 1];
    o = mk(a.x, a.y, a.z);
    d = vunit(mk(b.x, b.y, b.z)); // Ray::Ray, rayweek1.cpp:107
    t_max = a.w > FLT_MAX ? FLT_MAX : a.w;
    return cast_finite(o.x) && cast_finite(o.y) && cast_finite(o.z) && cast_finite(d.x) && cast_finite(d.y) && cast_finite(d.z) && t_max > 0.001f; // (false for a NaN t_max)
}

// ray i's result: the hit record of rayweek1.cpp:316-322 (as shade_level computes hp and n), or the miss record; R1_CAST_ANY: one byte
__device__ __forceinline__ void cast_store(const R1CastArgs &A, const uint32_t i, const uint32_t best_id, const float best, const float t_max, const V3 o,
                                           const V3 d)
{
    const bool hit = best_id != 0xFFFFFFFFu && best < t_max;
    if (A.mode != 0u) // (wave-uniform)
    {
        ((uint8_t *)A.out)[i] = hit ? 1 : 0;
        return;
    }
    float4 r0 = make_float4(FLT_MAX, __int_as_float(-1), 0.0f, 0.0f), r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (hit)
    {
        const f4 e = ((const f4 *)A.t.scene.exact)[best_id];
        const float inv_radius = ((const f4 *)A.t.scene.shade)[best_id].x;
        const uint32_t scene_index = ((const r1_gu32 *)A.active_to_scene)[best_id];
        const V3 hp = vadd(o, vscale(d, best));
        const V3 n = vscale(vsub(hp, mk(e.x, e.y, e.z)), inv_radius);
        r0 = make_float4(best, __uint_as_float(scene_index), hp.x, hp.y);
        r1 = make_float4(hp.z, n.x, n.y, n.z);
    }
    float4 *dst = (float4 *)A.out + 2 * (size_t)i;
    dst[0] = r0, dst[1] = r1;
}

// A wave's next chunk of the ray array, from the launch's one cursor; false: none left.  Called by all 64 lanes, wave-uniform result.
__device__ __forceinline__ bool cast_claim(const R1CastArgs &A, const int lane, uint32_t &q_next, uint32_t &q_end)
{
    return chunk_claim(A.cursor, A.claim, A.n, lane, q_next, q_end);
}

} // namespace

// ---- box tree ---------------------------------------------------------------------------------------------------------------------------
// Persistent: the waves claim chunks of the ray array from one atomic cursor, and bvh_advance runs with CARRY — a lane whose walk is
// complete writes its record and takes the next ray while the longest walks of the wave go on (the shape of the trace kernels' loop,
// r1_trace_body, without a path to shade).  Small scenes (!BIG): the workgroup's LDS copy of the node table with 16-bit references, the
// root step's code in node 0's K slot and the flat tree's y slab in node 1's pad slots, where bvh_advance<LN> looks for them — staged as
// r1_trace_body stages them (that function is left alone: its kernels' code must not move).  Big scenes: the breadth-first top of the
// table in LDS, the rest through the vector L1.
template <bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, (BIG ? R1_CAST_WAVES_BIG : R1_CAST_WAVES_SMALL)) r1_cast_tree_kernel(const R1CastArgs A)
{
    constexpr bool LN = !BIG;
    typedef typename IdxType<!LN>::type TS; // traversal-stack entry: uint16_t with the LDS table, else uint32_t
    extern __shared__ uint32_t s_trav[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
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

    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    float t_max = FLT_MAX;
    uint32_t ray = 0;
    bool alive = false;
    Trav tv;
    trav_start(tv);
    tv.cur = R1_BVH_DONE;
    uint32_t q_next = 0, q_end = 0;
    bool exhausted = false;
    for (;;)
    {
        // ---- refill: the lanes without a ray take the next ones of the wave's chunk ----
        unsigned long long need = __ballot(!alive);
        while (need)
        {
            if (q_next == q_end)
            {
                if (exhausted)
                    break;
                if (!cast_claim(A, lane, q_next, q_end))
                {
                    exhausted = true;
                    break;
                }
            }
            const uint32_t avail = q_end - q_next;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            if (!alive && rank < avail)
            {
                ray = q_next + rank;
                alive = cast_load(A, ray, o, d, t_max);
                if (alive)
                    trav_start(tv), tv.best = t_max;
                else
                    cast_store(A, ray, 0xFFFFFFFFu, FLT_MAX, FLT_MAX, o, d); // a miss without a walk; the lane asks again
            }
            q_next += min((uint32_t)__popcll(need), avail);
            need = __ballot(!alive);
        }
        const unsigned long long live = __ballot(alive);
        if (live == 0ull)
            break;
        // ---- walk with carry-over, then the lanes whose walk is complete write their record ----
        bvh_advance<false, true, LN, TS>(A.t.scene, o, d, tv, (TS *)s_trav, tid, (uint32_t)__popcll(live), nullptr, lnodes, top);
        if (alive && tv.cur == R1_BVH_DONE)
        {
            cast_store(A, ray, tv.best_id, tv.best, t_max, o, d);
            alive = false;
        }
    }
}

// ---- uniform grid -----------------------------------------------------------------------------------------------------------------------
// grid_trace is a complete walk per call, so a wave works its chunk off 64 rays at a time.  Small scenes: the grid's 16-bit table in LDS
// behind the fallback's traversal stack; rays too far for the grid take the tree walk from the global table (root_leaf = 0 in the
// arguments: it starts at the root), exactly as the grid trace kernel arranges it.
template <bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, (BIG ? R1_CAST_WAVES_BIG : R1_CAST_WAVES_SMALL)) r1_cast_grid_kernel(const R1CastArgs A)
{
    extern __shared__ uint32_t s_trav[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
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
        if (q_next == q_end && !cast_claim(A, lane, q_next, q_end))
            break;
        const uint32_t ray = q_next + (uint32_t)lane;
        const bool mine = ray < q_end;
        q_next = min(q_next + 64u, q_end);
        V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
        float t_max = FLT_MAX;
        bool alive = false;
        if (mine)
            alive = cast_load(A, ray, o, d, t_max);
        float best;
        uint32_t best_id;
        const bool fb = grid_trace<false, !BIG>(A.t, (R1GridCArgs *)(uintptr_t)A.t.grid, alive, o, d, best, best_id, ltab, tid, nullptr);
        if (__ballot(fb) != 0ull)
        {
            // fallback: the tree walk from scratch, exact for any origin; the outliers' offer is kept (the tree presents them again)
            Trav fv;
            trav_start(fv);
            fv.best = best, fv.best_id = best_id;
            if (!fb)
                fv.cur = R1_BVH_DONE;
            bvh_advance<false, false, false, uint32_t>(A.t.scene, o, d, fv, s_trav, tid, 64u, nullptr, nullptr);
            best = fv.best, best_id = fv.best_id;
        }
        if (mine)
            cast_store(A, ray, alive ? best_id : 0xFFFFFFFFu, best, t_max, o, d);
    }
}

// ---- reference form: every active sphere through exact_test in index order (the reference's own loop; the on-device cross-check) ----------
// exact_test compares with the running t_max itself, strictly: seeded with the ray's t_max it IS rayweek1.cpp:284-314.
__global__ void __launch_bounds__(R1_BLOCK) r1_cast_reference_kernel(const R1CastArgs A)
{
    const uint32_t stride = gridDim.x * R1_BLOCK;
    for (uint32_t i = blockIdx.x * R1_BLOCK + threadIdx.x; i < A.n; i += stride)
    {
        V3 o, d;
        float t_max;
        int hit = -1;
        float t_hit = FLT_MAX;
        if (cast_load(A, i, o, d, t_max))
        {
            t_hit = t_max;
            sweep_reference(A.t.scene, o, d, t_hit, hit);
        }
        cast_store(A, i, (uint32_t)hit, hit >= 0 ? t_hit : FLT_MAX, t_max, o, d);
    }
}

#ifdef R1_TUNING
// The plain form of the tree cast, for measuring only (R1_CAST_PLAIN=1 in the tuning library; tools/cast_bench.py): r1_wf_intersect's —
// grid-stride, one complete walk per ray from the table in global memory, the longest of 64 walks sets the wave's trip count.
__global__ void __launch_bounds__(R1_BLOCK) r1_cast_plain_kernel(const R1CastArgs A)
{
    extern __shared__ uint32_t s_trav[];
    const uint32_t stride = gridDim.x * R1_BLOCK;
    const uint32_t rounds = (A.n + stride - 1) / stride; // every lane makes the same number of trips (bvh_advance is called by all 64)
    for (uint32_t r = 0; r < rounds; ++r)
    {
        const uint32_t i = r * stride + blockIdx.x * R1_BLOCK + threadIdx.x;
        V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
        float t_max = FLT_MAX;
        bool alive = false;
        if (i < A.n)
            alive = cast_load(A, i, o, d, t_max);
        Trav tv;
        trav_start(tv);
        tv.best = t_max;
        if (!alive)
            tv.cur = R1_BVH_DONE;
        bvh_advance<false, false, false, uint32_t>(A.t.scene, o, d, tv, s_trav, (int)threadIdx.x, 64u, nullptr, nullptr);
        if (i < A.n)
            cast_store(A, i, alive ? tv.best_id : 0xFFFFFFFFu, tv.best, t_max, o, d);
    }
}
#endif

// ---- launchers (called from r1_queries.cpp) --------------------------------------------------------------------------------------------------
// variant: R1_V_TREE, R1_V_GRID or R1_V_REFERENCE — the structure the rays walk; plain: the tuning library's plain tree form
#define R1_CAST_DISPATCH(X)                                                                                                            \
    if (variant == R1_V_REFERENCE)                                                                                                     \
        X(r1_cast_reference_kernel);                                                                                                   \
    else if (variant == R1_V_GRID && big)                                                                                              \
        X(r1_cast_grid_kernel<true>);                                                                                                  \
    else if (variant == R1_V_GRID)                                                                                                     \
        X(r1_cast_grid_kernel<false>);                                                                                                 \
    else if (variant == R1_V_TREE && big)                                                                                              \
        X(r1_cast_tree_kernel<true>);                                                                                                  \
    else if (variant == R1_V_TREE)                                                                                                     \
        X(r1_cast_tree_kernel<false>);

extern "C" hipError_t r1_launch_cast(const R1CastArgs *args, int variant, int big, int plain, int blocks, size_t dyn_lds, hipStream_t stream)
{
#ifdef R1_TUNING
    if (plain && variant == R1_V_TREE)
    {
        hipLaunchKernelGGL(r1_cast_plain_kernel, dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);
        return hipGetLastError();
    }
#endif
    if (plain || (variant != R1_V_REFERENCE && variant != R1_V_TREE && variant != R1_V_GRID))
        return hipErrorInvalidValue;
#define R1_GO(K) hipLaunchKernelGGL((K), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args)
    R1_CAST_DISPATCH(R1_GO)
#undef R1_GO
    return hipGetLastError();
}

extern "C" hipError_t r1_cast_occupancy(int variant, int big, int plain, size_t dyn_lds, int *blocks_per_cu)
{
#ifdef R1_TUNING
    if (plain && variant == R1_V_TREE)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, r1_cast_plain_kernel, R1_BLOCK, dyn_lds);
#endif
#define R1_OCC(K) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (K), R1_BLOCK, dyn_lds)
    R1_CAST_DISPATCH(R1_OCC)
#undef R1_OCC
    return hipErrorInvalidValue;
}
