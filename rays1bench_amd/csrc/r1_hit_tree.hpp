// r1_hit_tree.hpp — the walk of the box tree (R1_VARIANT_BVH): the box test, the leaf tests (leaf_quad, leaf_root), the traversal state and
// bvh_advance, the walk with carry-over; sweep_bvh is one complete walk.  Internal linkage (anonymous namespace).
#ifndef R1_HIT_TREE_HPP
#define R1_HIT_TREE_HPP

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "r1_device.h"
#include "r1_exact_math.h"
#include "r1_offer.h"
#include "r1_dev_math.hpp"

#pragma clang fp contract(off)

namespace
{

// ---- sweep through the optional spatial index (R1_VARIANT_BVH) -------------
// Per-lane ordered traversal of the binary box tree built by r1_bvh.cpp.  Only the choice of
// spheres presented to exact_offer differs from the exhaustive sweeps; the boxes are inflated
// by pad = A |o - C|^2 + K (conservative with respect to the reference's fp32 test, see
// r1_bvh.cpp) and a subtree is skipped only if its inflated box is missed or lies entirely
// beyond the closest offer so far.  Result = minimum offer, ties to the lowest sphere index —
// the reference's in-order rule (see exact_offer).  The traversal stack lives in LDS,
// [entry][thread]; the builder bounds the tree depth by R1_BVH_STACK.
#define R1_BVH_DONE 0xFFFFFFFFu

// STATS (diagnostic build): wstat[2] wave trips of the node loop, [3] wave trips of the leaf
// pair loop, [9] node visits summed over lanes, [5] sphere-pair tests summed over lanes, [16] leaf trips
// summed over lanes (published in stats slot 14).
// One child box {m, e} against the ray, inflated by the node's pad (pa = pad * |1/d| per axis, computed once
// per node visit for both children; pad = A |o - C|^2 + K, conservative with respect to the reference's fp32
// sphere test AND to this test's own rounding: r1_bvh.cpp).  Slab form a = m / d - o / d (one fused
// multiply-add per axis, oi = o * (1/d) rounded once per ray), b = e |1/d| + pa: 17 VALU instructions per
// box against 28 for the round-1 form that measured |m - o|^2 per box.  Scalar arithmetic on purpose: the
// packed form (both children per v_pk_* instruction) costs the same issue cycles on this chip
// (profiles/r01/isa_issue_costs.txt) but more VGPRs.
__device__ __forceinline__ bool bvh_box(const float mx, const float my, const float mz, const float ex, const float ey, const float ez,
                                        const V3 pa, const V3 oi, const V3 inv, const V3 ainv, const float best, float &t_near)
{
    const float ax = __fmaf_rn(mx, inv.x, -oi.x), ay = __fmaf_rn(my, inv.y, -oi.y), az = __fmaf_rn(mz, inv.z, -oi.z);
    const float bx = __fmaf_rn(ex, ainv.x, pa.x), by = __fmaf_rn(ey, ainv.y, pa.y), bz = __fmaf_rn(ez, ainv.z, pa.z);
    // NaN (an axis the ray does not move along: inf - inf, 0 x inf) drops out of fmaxf/fminf: no constraint
    const float tn = fmaxf(fmaxf(ax - bx, ay - by), az - bz);
    const float tf = fminf(fminf(ax + bx, ay + by), az + bz);
    t_near = tn;
    // (three compares instead of tn <= fminf(tf, best): fminf makes the compiler canonicalise `best` every trip; a NaN tn or tf
    //  — every axis unconstrained — fails them either way)
    return tn <= tf && tn <= best && tf >= 0.0f;
}

// Up to TWO sphere pairs (four spheres) of a leaf for this lane's ray: first pass 1 of Hitable::hit for all
// four (rayweek1.cpp:192-202: nb, discr), then pass 2 (:294-313: square root, roots, strict compares) only
// for the spheres whose discriminant has a clear sign bit (:204), one per trip of a wave-uniform loop.  A
// lane rarely holds more than one such sphere in a leaf, so the wave runs the expensive half ~2 times per
// four spheres instead of four times (it used to cost 155 VALU instructions per pair, two thirds of them
// pass 2).  Same offers as exact_offer, same update rule (minimum offer, ties to the lowest sphere index).
// `pairs` = 1 or 2; an odd sphere's partner has radius_sq = -inf (discriminant -inf: never flagged).
// BOTH pairs are fetched and evaluated whatever `pairs` says: a one-pair leaf reads the first pair of the next leaf in
// the table — or, behind the last leaf, the sentinel pair r1_scene.cpp appends — and `mask` keeps those two slots from ever being flagged,
// whatever their discriminants come out as (finite, inf, NaN).  The branch around the second fetch cost eight register copies (pair A
// into pair B's registers), an exec-mask region and the compare in front of every leaf, on scenes whose leaves nearly all hold two pairs.
template <int OFFER>
__device__ __forceinline__ void leaf_quad(const float4 *__restrict__ prims, const uint32_t *__restrict__ ids, const uint32_t first,
                                          const uint32_t pairs, const V3 o, const V3 d, float &best, uint32_t &best_id)
{
    float nb[4], ds[4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
    {
        if (h)
            __builtin_amdgcn_sched_barrier(0); // pair B's arithmetic stays behind pair A's: left to mix them, hipcc spills in the 72-register builds (all four loads still issue together)
        const float4 p0 = prims[2 * (size_t)first + 2 * h], p1 = prims[2 * (size_t)first + 2 * h + 1];
#pragma unroll
        for (int s = 0; s < 2; ++s)
        {
            const int q = 2 * h + s;
            const float cx = s ? p0.y : p0.x, cy = s ? p0.w : p0.z, cz = s ? p1.y : p1.x, rsq = s ? p1.w : p1.z;
            const float cox = cx - o.x, coy = cy - o.y, coz = cz - o.z;
            nb[q] = __fmaf_rn(coz, d.z, __fmaf_rn(coy, d.y, cox * d.x));
            const float c = __fmaf_rn(coz, coz, __fmaf_rn(coy, coy, cox * cox)) - rsq;
            ds[q] = nb[q] * nb[q] - c;
        }
    }
    // bit q of `mask`: slot q's discriminant has a clear sign bit (rayweek1.cpp:204).  The four sign bits are shifted together with
    // v_alignbit_b32 ((hi:lo) >> 31 = hi << 1 | sign of lo): 4 + 3 instructions instead of 12 for compare + select + or per slot.
    uint32_t sgn = __float_as_uint(ds[3]) >> 31;
    sgn = __builtin_amdgcn_alignbit(sgn, __float_as_uint(ds[2]), 31u);
    sgn = __builtin_amdgcn_alignbit(sgn, __float_as_uint(ds[1]), 31u);
    sgn = __builtin_amdgcn_alignbit(sgn, __float_as_uint(ds[0]), 31u);
    uint32_t mask = ~sgn & (pairs < 2u ? 3u : 15u);
    // Straight-line body, selects instead of branches: every lane of the leaf runs every trip (a lane without a flagged sphere left
    // computes on slot 3's numbers and is kept from the update by `have`), and the sphere's index is fetched before its offer is
    // known to count.  The branched form (only lanes with a flagged sphere, the index only for an offer in range) cost seven register
    // moves per trip for the loop-carried best / best_id and two exec-mask regions.
    // A guarded do-while on purpose: written as `while (ballot)`, the loop-carried best / best_id went through a second register pair —
    // two copies in front of the loop and two more in every trip; in this form the selects below write the caller's registers.
    unsigned long long flagged = __builtin_amdgcn_ballot_w64(mask != 0u); // wave-uniform
    if (flagged != 0ull)
    do
    {
        const bool have = mask != 0u;
        const uint32_t q = (uint32_t)__builtin_ctz(mask | 8u); // the lowest flagged slot; 3 for a lane that has none left
        mask &= mask - 1u;
        const float n_ = q == 0u ? nb[0] : (q == 1u ? nb[1] : (q == 2u ? nb[2] : nb[3]));
        const float d_ = q == 0u ? ds[0] : (q == 1u ? ds[1] : (q == 2u ? ds[2] : ds[3]));
        const uint32_t id = ids[2 * (size_t)first + q];
        const float root = r1_sqrt_exact_lanes(d_, flagged); // (a lane without a flagged sphere holds slot 3's discriminant, of any sign: it does not vote)
        const float t1 = n_ - root;
        const float t = (t1 > 0.001f) ? t1 : n_ + root;
        // (bitwise on purpose: && / || become nested exec-mask regions)
        const bool upd = have & r1_offer_update_form<OFFER>(t, id, best, best_id);
        best = upd ? t : best;
        best_id = upd ? id : best_id;
        flagged = __builtin_amdgcn_ballot_w64(mask != 0u);
    } while (flagged != 0ull);
}

// The leaf of the ROOT step (bvh_advance), sphere by sphere: all lanes of the step test the SAME <= 4 spheres — the ground and the big
// balls — and nearly every lane's line meets the ground, so the slot leaf_quad's loop searches for is the same slot for everybody.  Here
// each slot runs pass 1 and ONE vote, and pass 2 in straight-line code under it where any lane of the step is flagged: no slot search, no
// select chains over nb[4] / ds[4] (the arrays are gone), no loop vote, and `first` / `pairs` are wave-uniform (the caller makes them
// scalars), so the spheres and their indices arrive by scalar loads.  113 + 22 v VALU instructions (v: slots with a flagged lane)
// against 120 + 52 t (t: the most flagged slots any lane holds) — DESIGN.md §4.26.  The offers are leaf_quad's operation for operation
// and the slots come in index order, so the result is the same minimum offer with ties to the lowest index; an odd sphere's partner
// (radius_sq = -inf: discriminant -inf) is never flagged, and a one-pair leaf fetches one pair.
template <int OFFER>
__device__ __forceinline__ void leaf_root(const float4 *__restrict__ prims, const uint32_t *__restrict__ ids, const uint32_t first,
                                          const uint32_t pairs, const V3 o, const V3 d, float &best, uint32_t &best_id)
{
    typedef const uint32_t __attribute__((address_space(4))) *cu32_ptr;
    const cf4_ptr sp = (cf4_ptr)(const f4 *)prims + 2 * (size_t)first;
    const cu32_ptr si = (cu32_ptr)ids + 2 * (size_t)first;
#pragma unroll
    for (int h = 0; h < 2; ++h)
    {
        if (h && pairs < 2u) // (wave-uniform)
            break;
        const f4 p0 = sp[2 * h], p1 = sp[2 * h + 1];
#pragma unroll
        for (int s = 0; s < 2; ++s)
        {
            const float cx = s ? p0.y : p0.x, cy = s ? p0.w : p0.z, cz = s ? p1.y : p1.x, rsq = s ? p1.w : p1.z;
            const float cox = cx - o.x, coy = cy - o.y, coz = cz - o.z;
            const float nb = __fmaf_rn(coz, d.z, __fmaf_rn(coy, d.y, cox * d.x));
            const float c = __fmaf_rn(coz, coz, __fmaf_rn(coy, coy, cox * cox)) - rsq;
            const float ds = nb * nb - c;
            // the lanes of the step whose discriminant has a clear sign bit (rayweek1.cpp:204); the others hold anything below and never update
            const unsigned long long any = __builtin_amdgcn_ballot_w64((int)__float_as_uint(ds) >= 0);
            if (any != 0ull)
            {
                const bool flag = (int)__float_as_uint(ds) >= 0;
                const uint32_t id = si[2 * h + s]; // (behind the vote: fetched with the pair, the two indices cost the big-scene PIXEL build ten more lane moves and no run was faster)
                const float root = r1_sqrt_exact_lanes(ds, any);
                const float t1 = nb - root;
                const float t = (t1 > 0.001f) ? t1 : nb + root;
                const bool upd = flag & r1_offer_update_form<OFFER>(t, id, best, best_id);
                best = upd ? t : best;
                best_id = upd ? id : best_id;
            }
        }
    }
}

// Traversal-stack entries.  Big scenes: the 32-bit child reference as it is.  Small scenes (the kernels that keep the node table in LDS:
// <= 256 nodes, <= 1023 spheres = 512 pairs): 16 bits — bit 15 leaf, bits 12..14 the pair count, bits 0..11 the node or first pair —
// which halves the stack in LDS (4 KB instead of 8 for the large scene's tree: together with the 10-word attenuation stack and the
// node table 22 KB per workgroup = seven workgroups per CU with the whole attenuation stack of round 2 in LDS).
__device__ __forceinline__ void trav_put(uint32_t *trav, const int at, const uint32_t ref) { trav[at] = ref; }
__device__ __forceinline__ uint32_t trav_get(const uint32_t *trav, const int at) { return trav[at]; }
// (the small-scene kernels walk with the 16-bit form throughout: the child references are converted once, when the workgroup copies
// the node table into LDS — r1_ref16 — so a push is a 16-bit store and a pop a zero-extending load)
__device__ __forceinline__ void trav_put(uint16_t *trav, const int at, const uint32_t ref) { trav[at] = (uint16_t)ref; }
__device__ __forceinline__ uint32_t trav_get(const uint16_t *trav, const int at) { return trav[at]; }
__device__ __forceinline__ uint32_t r1_ref16(const uint32_t ref) { return ((ref >> 16) & 0xF000u) | (ref & 0x0FFFu); }

// Traversal state of one lane.  It lives in registers ACROSS the outer loop of the trace kernel
// (carry-over, below); the stack entries are in LDS, [entry][thread].
struct Trav
{
    uint32_t cur;     // node or leaf reference being visited, R1_BVH_DONE when the walk is complete
    int sp;           // entries on the traversal stack
    float best;       // closest offer so far (FLT_MAX: none)
    uint32_t best_id; // its sphere (0xFFFFFFFF: none)
};

__device__ __forceinline__ void trav_start(Trav &t)
{
    t.cur = 0u, t.sp = 0, t.best = FLT_MAX, t.best_id = 0xFFFFFFFFu;
}

#ifndef R1_CARRY_DIV
#define R1_CARRY_DIV 6u // a walk phase ends when at most 1 / R1_CARRY_DIV of the live lanes are still walking (2 / 3 / 4 / 6 / 8: 30.3 / 31.6 / 31.9 / 32.1 / 32.0 Grays/s)
#endif
// Advances every lane whose walk is not complete.  CARRY = false: until all walks are complete (the
// classic while-while loop).  CARRY = true: returns as soon as at most a quarter of the `n_alive` live
// lanes of the wave are still walking; those lanes keep their state and go on in the next call, next
// to the fresh rays of the lanes that have been shaded and refilled meanwhile.  The longest of 64
// walks no longer sets the trip count of the loops for everybody (a wave made 14.3 node trips for a mean
// of 7.0 visits per lane), at the price of shading ~3/4 of the wave at a time.  Called by all 64 lanes.
// The walk is while-while: all lanes on inner nodes descend until each has reached a leaf or finished, then the leaves
// are tested.  (Round 2 also carried a voting form — one step per trip, of the kind most walking lanes wait for: lane
// utilisation of the node / leaf steps 0.53 / 0.69 -> 0.74 / 0.75, and 5 % SLOWER once the node table sat in LDS, because
// the vote costs ~20 VALU instructions per trip; removed in round 3)
// LN: the node table is read from `lnodes`, the workgroup's copy in LDS (the trace kernel on small scenes), instead of S.bvh_nodes.
// SLOTS: the root step tests its leaf with leaf_root instead of leaf_quad (r1_builds.h r1_root_by_slots: one choice per build).
// OFFER: the form of the closest-offer rule in the leaf tests (r1_offer.h r1_offer_better_form; the grid kernels' fallback walk passes the grid's).
// FLAT: is the tree flat (visit_flat below)?  R1_FLAT_ASK: the table says — bit 2 of the code in the LDS copy of node 0, read where it is
// needed; every kernel r1_pick reaches.  R1_FLAT_YES / R1_FLAT_NO: the launch knows (LN walks only): one node loop is instantiated, and the
// slab, the choice of the node loop and the F update after a leaf read no flag (r1_flatwalk_kernel).
#define R1_FLAT_ASK (-1)
#define R1_FLAT_NO 0
#define R1_FLAT_YES 1
#ifndef R1_ROOT_SCALAR
// FLAT = R1_FLAT_YES: the root step's wave-uniform words by scalar loads (1) or from the LDS copy, as every other walk (0).  Left at 0: with
// the words in scalar registers across the root leaf's test hipcc parks the kernel-argument pointer in a lane of the spill register and fetches
// it back twice per iteration — 32 lane moves in the main loop against the generic kernel's 30 (28 at 0), profiles/r32/flat_walk_counts.txt —
// and the library with it ran at the generic kernel's rate (profiles/r32/flat_walk_ab.txt).  `make tuning EXTRA=-DR1_ROOT_SCALAR=1` builds it.
#define R1_ROOT_SCALAR 0
#endif
template <bool STATS, bool CARRY, bool LN, typename TS, bool SLOTS = false, int OFFER = R1_OFFER_FORM, int FLAT = R1_FLAT_ASK>
__device__ __forceinline__ void bvh_advance(const R1DeviceScene &S, const V3 o, const V3 d, Trav &tv, TS *trav, const int tid,
                                            const uint32_t n_alive, unsigned long long *wstat, const float4 *lnodes /* LDS */, const uint32_t top = 0u /* !LN: nodes [0, top) are in lnodes */)
{
    static_assert(FLAT == R1_FLAT_ASK || LN, "a walk that knows its tree's flatness reads the table from LDS");
    // The root step's words are the same for every lane.  A walk that knows its tree is flat fetches them by scalar loads — node 0 from the
    // table in global memory through a constant-address-space pointer, the root-leaf code and the slab from the arguments, which is where the
    // staging code takes them from — instead of a v_mov of an LDS address and a per-lane ds_read each.  Same words, same operations.
    constexpr bool ROOT_S = FLAT == R1_FLAT_YES && R1_ROOT_SCALAR != 0;
    typedef const float __attribute__((address_space(4))) *cf_ptr;
    const cf_ptr sf = (cf_ptr)(const float *)S.bvh_nodes; // (used where ROOT_S)
    const float4 *__restrict__ nodes = S.bvh_nodes;
    const float4 *__restrict__ prims = S.bvh_prims;
    const uint32_t *__restrict__ ids = S.bvh_ids;
    // v_rcp_f32 (1 ulp) is enough here: the reciprocals only feed the conservative box test, whose
    // pad budgets for its own rounding (r1_bvh.cpp)
    const V3 inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    const V3 ainv = mk(fabsf(inv.x), fabsf(inv.y), fabsf(inv.z));
    V3 oi = mk(o.x * inv.x, o.y * inv.y, o.z * inv.z); // (flat trees: oi.y becomes N once the root step is over, see visit_flat)
    const float rx = o.x - S.bvh_centre[0], ry = o.y - S.bvh_centre[1], rz = o.z - S.bvh_centre[2];
    const float r2 = __fmaf_rn(rz, rz, __fmaf_rn(ry, ry, rx * rx)); // |o - C|^2 of pad = A r2 + K
    V3 pa_ray = mk(0.0f, 0.0f, 0.0f);
    if (LN)
    {
        const float pad_ray = (ROOT_S ? sf[12] : lnodes[3].x) * r2; // the tree's A (every node carries it)
        pa_ray = mk(pad_ray * ainv.x, pad_ray * ainv.y, pad_ray * ainv.z);
    }
    float best = tv.best;
    uint32_t best_id = tv.best_id;
    uint32_t cur = tv.cur;
    int sp = tv.sp;
    // child references: bit 31 leaf / bits 28..30 pair count / 28 bits of index — or, in the LDS copy of a small scene's table,
    // bit 15 / bits 12..14 / 12 bits (see trav_put)
    constexpr uint32_t LEAF_BIT = LN ? 0x8000u : 0x80000000u, INDEX_MASK = LN ? 0x0FFFu : 0x0FFFFFFFu;
    constexpr int COUNT_SHIFT = LN ? 12 : 28;
    // one visit of the inner node `cur`: both children's boxes, nearer child next, farther one on the stack (or the stack's top if neither is hit)
    auto visit_node = [&]() {
        if (STATS)
        {
            wstat[9] += 1;
            if ((tid & 63) == __ffsll((long long)__ballot(1)) - 1)
                wstat[2] += 1;
        }
        // {m0x m1x m0y m1y} {m0z m1z e0x e1x} {e0y e1y e0z e1z} {A K child0 child1}
        float4 q0, q1, q2, q3;
        if (LN || cur < top)
        {
            q0 = lnodes[4 * cur + 0], q1 = lnodes[4 * cur + 1], q2 = lnodes[4 * cur + 2], q3 = lnodes[4 * cur + 3];
            if (!LN)
                asm volatile("" : "+v"(q0.x), "+v"(q1.x), "+v"(q2.x), "+v"(q3.x));
        }
        else
            q0 = nodes[4 * (size_t)cur + 0], q1 = nodes[4 * (size_t)cur + 1], q2 = nodes[4 * (size_t)cur + 2],
            q3 = nodes[4 * (size_t)cur + 3];
        float tn0, tn1;
        // The pad.  Table in LDS (LN): A R2 |1/d| of the whole tree, computed once per call (`pa_ray`; the nodes' K are part of
        // their half extents, r1_bvh.cpp).  Table in global memory: per node, pad = A dist2 + K with dist2 = R2 or — wave-uniform,
        // scenes of small spheres — |m0 + m1 - 2 o|^2; such trees always run through these kernels (r1_frame.cpp big_scene).
        V3 pa = pa_ray;
        if (!LN)
        {
            float dist2 = r2;
            if (S.bvh_pad_local)
            {
                const float sx = __fmaf_rn(-2.0f, o.x, q0.x + q0.y), sy = __fmaf_rn(-2.0f, o.y, q0.z + q0.w), sz = __fmaf_rn(-2.0f, o.z, q1.x + q1.y);
                dist2 = __fmaf_rn(sz, sz, __fmaf_rn(sy, sy, sx * sx));
            }
            const float pad = __fmaf_rn(q3.x, dist2, q3.y);
            pa = mk(pad * ainv.x, pad * ainv.y, pad * ainv.z);
        }
        const bool h0 = bvh_box(q0.x, q0.z, q1.x, q1.z, q2.x, q2.z, pa, oi, inv, ainv, best, tn0);
        const bool h1 = bvh_box(q0.y, q0.w, q1.y, q1.w, q2.y, q2.w, pa, oi, inv, ainv, best, tn1);
        const uint32_t c0 = __float_as_uint(q3.z), c1 = __float_as_uint(q3.w);
        if (h0 && h1)
        {
            const bool swap = tn1 < tn0;
            trav_put(trav, sp * R1_BLOCK + tid, swap ? c0 : c1);
            ++sp;
            cur = swap ? c1 : c0;
        }
        else if (h0)
            cur = c0;
        else if (h1)
            cur = c1;
        else if (sp > 0)
            cur = trav_get(trav, --sp * R1_BLOCK + tid);
        else
            cur = R1_BVH_DONE;
    };
    // Flat trees (r1_bvh.cpp "flat axis"; the small-scene kernels, y): every box the node loop tests lies in ONE y slab (m_u, e_u), wider
    // than the narrowest of them by a few per cent.  The slab is tested once per call,
    //      a_u = m_u / d.y - o.y / d.y   b_u = e_u |1 / d.y| + pa.y   N = max(a_u - b_u, 0)   F = min(a_u + b_u, best)   (F again after a leaf)
    // and a child box costs its two other axes and ONE compare: max(tn, 0) <= min(tf, best) holds iff tn <= tf && tn <= best && tf >= 0,
    // because best > 0 always (>= 0.001 or FLT_MAX).  11 VALU instructions per box instead of 17, 40 bytes of the node instead of 56, and
    // the m_y / e_y words are not fetched.  A box tested with the union's slab instead of its own is a
    // wider box: every sphere that matters is still presented, and the result is the minimum offer with ties to the lowest index in any
    // order — so two children that both contain the origin (entry distances clamped to N alike) are no longer swapped, to no effect.  NaN
    // axes drop out of max3 / min3 as in bvh_box; a ray without any finite axis passes where bvh_box failed it: the conservative side.
    // N and F live where the generic loop keeps oi.y and pa.y (`oi.y`, `pa_ray.y` below), and ONE outer loop serves both walks, picking its
    // node loop by the tree's flag (a scalar: the compiler keeps it in one SGPR).  Two copies of the outer loop, or N / F in registers of
    // their own, spilled 5-22 VGPRs to scratch in the 72-register builds; this form leaves every tree kernel the VGPR count it had.
    // F = min(a_u + b_u, best) follows `best` where it moves — after a leaf: recomputed before each run of the node loop instead, the
    // synchronous-frame and PIXEL kernels took 1-6 VGPRs more and the rate was 0.1 % lower.
    auto visit_flat = [&]() {
        if (STATS)
        {
            wstat[9] += 1;
            if ((tid & 63) == __ffsll((long long)__ballot(1)) - 1)
                wstat[2] += 1;
        }
        const float4 q0 = lnodes[4 * cur + 0], q1 = lnodes[4 * cur + 1], q2 = lnodes[4 * cur + 2], q3 = lnodes[4 * cur + 3];
        const float ax0 = __fmaf_rn(q0.x, inv.x, -oi.x), az0 = __fmaf_rn(q1.x, inv.z, -oi.z);
        const float bx0 = __fmaf_rn(q1.z, ainv.x, pa_ray.x), bz0 = __fmaf_rn(q2.z, ainv.z, pa_ray.z);
        const float ax1 = __fmaf_rn(q0.y, inv.x, -oi.x), az1 = __fmaf_rn(q1.y, inv.z, -oi.z);
        const float bx1 = __fmaf_rn(q1.w, ainv.x, pa_ray.x), bz1 = __fmaf_rn(q2.w, ainv.z, pa_ray.z);
        const float tn0 = fmaxf(fmaxf(ax0 - bx0, az0 - bz0), oi.y), tf0 = fminf(fminf(ax0 + bx0, az0 + bz0), pa_ray.y);
        const float tn1 = fmaxf(fmaxf(ax1 - bx1, az1 - bz1), oi.y), tf1 = fminf(fminf(ax1 + bx1, az1 + bz1), pa_ray.y);
        const bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
        const uint32_t c0 = __float_as_uint(q3.z), c1 = __float_as_uint(q3.w);
        if (h0 && h1)
        {
            const bool swap = tn1 < tn0;
            trav_put(trav, sp * R1_BLOCK + tid, swap ? c0 : c1);
            ++sp;
            cur = swap ? c1 : c0;
        }
        else if (h0)
            cur = c0;
        else if (h1)
            cur = c1;
        else if (sp > 0)
            cur = trav_get(trav, --sp * R1_BLOCK + tid);
        else
            cur = R1_BVH_DONE;
    };
    // The root step outside the loops (r1_bvh.cpp: the root of the reference's scenes is [a leaf of <= 2 pairs that every ray tests | the
    // rest], S.bvh_root_leaf): the lanes that start a walk in this call (cur == 0: no child reference points at the root) test that leaf
    // and then the box of the other child, all of them together and in straight-line code, and go on at the other child.  Same offers, same
    // pruning rule as a visit of node 0 followed by the leaf; one node trip and one leaf trip fewer per ray in the divergent loops below.
    // (the small-scene kernels find the code in the K slot of their LDS copy of node 0 — the trace kernel puts it there, K itself is folded
    //  into the half extents for their trees — instead of holding a scalar register for it through the whole kernel)
    const uint32_t root_leaf = LN && !ROOT_S ? __float_as_uint(lnodes[3].y) & 3u : S.bvh_root_leaf; // (bit 2 of the LDS copy's code: a flat tree, see r1_trace_kernel)
    if (root_leaf != 0u && cur == 0u) // (the first condition is wave-uniform)
    {
        // column of the OTHER child in the node's rows (ROOT_S: an index of scalar loads — written as selects between the two columns, hipcc
        // makes two v_mov and a v_cndmask of every word)
        const int k = ROOT_S ? __builtin_amdgcn_readfirstlane(root_leaf == 1u ? 1 : 0) : (root_leaf == 1u ? 1 : 0);
        const float *nf = (const float *)lnodes; // node 0: always in the workgroup's LDS copy (big scenes keep the top of the tree there: at least node 0, r1_frame.cpp fill_walk)
        // (ROOT_S: the table's 32-bit references, converted on the scalar pipe to the 16-bit form the LDS copy holds)
        const uint32_t leaf = ROOT_S ? r1_ref16(__float_as_uint(sf[14 + (1 - k)])) : __float_as_uint(nf[14 + (1 - k)]);
        const uint32_t other = ROOT_S ? r1_ref16(__float_as_uint(sf[14 + k])) : __float_as_uint(nf[14 + k]);
        const uint32_t lp = (leaf >> COUNT_SHIFT) & 7u;
        if (STATS)
        {
            wstat[5] += (unsigned long long)lp, wstat[16] += 1ull, wstat[17] += 1ull; // ([17]: root steps = one box test each, stats slot 15)
            if ((tid & 63) == __ffsll((long long)__ballot(1)) - 1)
                wstat[3] += 1;
        }
        if (SLOTS) // (the reference is the same LDS word for every lane: made a scalar, the compiler cannot know)
            leaf_root<OFFER>(prims, ids, (uint32_t)__builtin_amdgcn_readfirstlane((int)(leaf & INDEX_MASK)), (uint32_t)__builtin_amdgcn_readfirstlane((int)lp), o, d, best, best_id);
        else
            leaf_quad<OFFER>(prims, ids, leaf & INDEX_MASK, lp, o, d, best, best_id);
        // (the other child's box is fetched only now: six more live registers across the leaf test spill in the 7-wave builds)
        V3 pa = pa_ray;
        if (!LN)
        {
            float dist2 = r2;
            if (S.bvh_pad_local)
            {
                const float sx = __fmaf_rn(-2.0f, o.x, nf[0] + nf[1]), sy = __fmaf_rn(-2.0f, o.y, nf[2] + nf[3]), sz = __fmaf_rn(-2.0f, o.z, nf[4] + nf[5]);
                dist2 = __fmaf_rn(sz, sz, __fmaf_rn(sy, sy, sx * sx));
            }
            const float pad = __fmaf_rn(nf[12], dist2, nf[13]);
            pa = mk(pad * ainv.x, pad * ainv.y, pad * ainv.z);
        }
        float tn;
        const bool h = ROOT_S ? bvh_box(sf[0 + k], sf[2 + k], sf[4 + k], sf[6 + k], sf[8 + k], sf[10 + k], pa, oi, inv, ainv, best, tn)
                              : bvh_box(nf[0 + k], nf[2 + k], nf[4 + k], nf[6 + k], nf[8 + k], nf[10 + k], pa, oi, inv, ainv, best, tn);
        cur = h ? other : R1_BVH_DONE;
        // (the sibling's own visit taken into this step as well — `if (cur < LEAF_BIT) visit_node();` here — measured 35.5 against 36.2
        //  Grays/s: a generic visit runs at 0.54 lane utilisation inside the loop and at the ~0.34 of the starting lanes out here)
    }
    // Flat trees: the slab, once per call and after the root step (its leaf has moved `best`, and it tests node 0's box with all three
    // axes).  A ray whose slab interval is empty, N > F, is done — whatever its walk still holds lies in the slab (every leaf box below
    // the boxes of the loop does), so every test it could still make would fail: the root step's "N <= F", which holds as well for a walk
    // carried over from an earlier call.
    // (the flag is made a scalar: the compiler cannot know that a value from LDS is wave-uniform, and a branch it takes for divergent runs
    //  both node loops one after the other)
    // (FLAT = R1_FLAT_YES: the slab stays behind a condition on a scalar the compiler cannot see through, one s_cmp.  With the slab in
    //  straight-line code hipcc keeps -oi in registers of its own and forms them with three v_xor on either side of the root step: six
    //  more VALU instructions per call than the flag's branch costs the generic kernel)
    int slab_known = 1;
    if (FLAT == R1_FLAT_YES)
        asm volatile("" : "+s"(slab_known));
    if ((FLAT == R1_FLAT_YES && slab_known != 0) || (FLAT == R1_FLAT_ASK && LN && (__builtin_amdgcn_readfirstlane((int)__float_as_uint(lnodes[3].y)) & 4) != 0))
    {
        const float m_u = ROOT_S ? S.bvh_flat_m : lnodes[7].x, e_u = ROOT_S ? S.bvh_flat_e : lnodes[7].y;
        const float a_u = __fmaf_rn(m_u, inv.y, -oi.y), b_u = __fmaf_rn(e_u, ainv.y, pa_ray.y);
        const float tyf = a_u + b_u;
        oi.y = fmaxf(a_u - b_u, 0.0f);
        // (a compare instead of fminf: the compiler canonicalises both operands of an fminf; a NaN sum — a ray that does not move along y — leaves `best`)
        pa_ray.y = tyf < best ? tyf : best;
        cur = oi.y <= pa_ray.y ? cur : R1_BVH_DONE;
    }
    for (;;)
    {
        const unsigned long long walking = __ballot(cur != R1_BVH_DONE);
        if (walking == 0ull)
            break;
        if (CARRY && R1_CARRY_DIV * (uint32_t)__popcll(walking) <= n_alive)
            break; // (n_alive <= 3: never true while a lane walks, so the last walks of a wave run to their end)
        // inner nodes: descend to the nearer child, remember the farther one
        if (FLAT == R1_FLAT_YES)
            while (cur < LEAF_BIT)
                visit_flat();
        else if (FLAT == R1_FLAT_NO)
            while (cur < LEAF_BIT)
                visit_node();
        else if (LN && (__builtin_amdgcn_readfirstlane((int)__float_as_uint(lnodes[3].y)) & 4) != 0)
            while (cur < LEAF_BIT)
                visit_flat();
        else
            while (cur < LEAF_BIT) // (R1_BVH_DONE has the leaf bit set in either form: one compare)
                visit_node();
        if (cur != R1_BVH_DONE)
        {
            // leaf: `cnt` PAIRS of spheres {cx_a cx_b cy_a cy_b} {cz_a cz_b rsq_a rsq_b}; an odd
            // sphere's partner has radius_sq = -inf (discriminant -inf: never offers a hit)
            const uint32_t first = cur & INDEX_MASK, cnt = (cur >> COUNT_SHIFT) & 7u;
            if (LN)
            {
                // The LDS walks' trees have leaves of at most R1_BVH_LEAF = 4 spheres = 2 pairs (r1_frame.cpp big_scene sends any other tree
                // through the !LN kernels): one leaf_quad call, no pair loop, and a 12-bit `first` the sphere-index fetch can add to a scalar base.
                static_assert(R1_BVH_LEAF <= 4, "the LDS walks test a leaf with ONE leaf_quad call: at most two pairs");
                if (STATS)
                {
                    wstat[5] += (unsigned long long)cnt, wstat[16] += 1ull;
                    if ((tid & 63) == __ffsll((long long)__ballot(1)) - 1)
                        wstat[3] += 1;
                }
                leaf_quad<OFFER>(prims, ids, first, cnt, o, d, best, best_id);
            }
            else
            for (uint32_t j = 0; j < cnt; j += 2u)
            {
                const uint32_t take = cnt - j < 2u ? 1u : 2u;
                if (STATS)
                {
                    wstat[5] += (unsigned long long)take; // sphere pairs tested by this lane
                    wstat[16] += 1ull;                    // leaf trips of this lane
                    if ((tid & 63) == __ffsll((long long)__ballot(1)) - 1)
                        wstat[3] += 1;
                }
                leaf_quad<OFFER>(prims, ids, first + j, take, o, d, best, best_id);
            }
            cur = sp > 0 ? trav_get(trav, --sp * R1_BLOCK + tid) : R1_BVH_DONE;
            if (FLAT == R1_FLAT_YES || (FLAT == R1_FLAT_ASK && LN && (__builtin_amdgcn_readfirstlane((int)__float_as_uint(lnodes[3].y)) & 4) != 0))
                pa_ray.y = best < pa_ray.y ? best : pa_ray.y; // F = min(a_u + b_u, best): best has moved in the leaf, and only down
        }
    }
    tv.cur = cur, tv.sp = sp, tv.best = best, tv.best_id = r1_offer_settle_form<OFFER>(best, best_id); // (form 2: "none" again where the walk only held an offer of FLT_MAX, r1_offer.h)
}

// one complete walk (the wavefront kernels)
template <bool STATS>
__device__ __forceinline__ void sweep_bvh(const R1DeviceScene &S, const bool alive, const V3 o, const V3 d, float &t_max, int &hit_index,
                                          uint32_t *trav, const int tid, unsigned long long *wstat)
{
    Trav tv;
    trav_start(tv);
    if (!alive)
        tv.cur = R1_BVH_DONE;
    bvh_advance<STATS, false, false, uint32_t>(S, o, d, tv, trav, tid, 64u, wstat, nullptr);
    if (tv.best_id != 0xFFFFFFFFu)
    {
        t_max = tv.best;
        hit_index = (int)tv.best_id;
    }
}

} // namespace

#endif // R1_HIT_TREE_HPP
