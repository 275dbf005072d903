// r1_query_kernels.hip — the kernels of the ray queries (r1_cast_rays*), of the path queries (r1_trace_rays*, §4.22) and of the
// scatter queries (r1_scatter_rays*, §4.34), and of the feature frames (r1_render_features*, §4.38), whose rays are the camera's own:
// caller-supplied rays through the trace kernels' walks as they are — sweep_reference (r1_hit_sweep.hpp), bvh_advance (r1_hit_tree.hpp), grid_trace
// (r1_hit_grid.hpp) — claimed with chunk_claim (r1_sample.hpp) and, the path jobs, shaded by shade_level (r1_shade.hpp).  There is
// one loop per structure — box tree, uniform grid, reference form — and a JOB says what a lane does with a ray: how it is loaded and
// when it is no ray at all, how its walk is seeded, what a complete walk leads to and which record is written.
//   Args                     the kernel's argument struct; every job's has t, cursor, n and claim
//   waves(big)               the occupancy bound given to the compiler
//   idle()                   the state of a lane without a ray (the walks are called by all 64 lanes)
//   load(A, i)               ray i of the launch (the feature job: pixel i, and its first sample's ray); false: it takes no walk
//   seed(best)               where a walk's closest offer starts, if not at FLT_MAX
//   O(), D()                 what the walk follows
//   step(A, id, t, ..)       a walk is complete (id 0xFFFFFFFF: nothing hit); true: the ray's answer is known, false: O(), D() are the job's next walk
//   finish(A, i, walked)     writes ray i's record and frees the lane; walked false: the ray took no walk (load said so)
//   BOUNCES                  false: step() always returns true — one walk per ray.  The grid loop then drops its loop over walks and writes the record
//                            of a ray without a walk behind the walk with the others: a second place that writes records costs the cast's grid kernels
//                            6 VGPRs (profiles/r15/query_kernel_meta.txt)
// The loops keep the ray's index themselves and hand it to finish(): a job holds no state that is unset before its first load.
#include "r1_hit_sweep.hpp"
#include "r1_hit_tree.hpp"
#include "r1_hit_grid.hpp"
#include "r1_sample.hpp"
#include "r1_shade.hpp"
#include "r1_internal.h"

#ifndef R1_CAST_WAVES_SMALL
#define R1_CAST_WAVES_SMALL 8 // waves per SIMD the cast kernels for small scenes are built for (registers, LDS: profiles/r10/cast.txt)
#endif
#ifndef R1_CAST_WAVES_BIG
#define R1_CAST_WAVES_BIG 8
#endif
#ifndef R1_PATHQ_WAVES
#define R1_PATHQ_WAVES 6 // the occupancy bound the compiler is given for the path jobs' tree and grid kernels.  They come to 58 .. 60 VGPRs under it, so eight
#endif                   // waves per SIMD fit all the same; asked for eight, the compiler parks 12 .. 20 SGPRs in VGPR lanes (44 .. 48 v_readlane / v_writelane in
                         // the loops) to reach the same register count (profiles/r14/trace_rays_kernel_meta.txt)

namespace
{

__device__ __forceinline__ bool query_finite(const float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

} // namespace

// ---- the cast job: Hitable::hit(Ray(o, d), 0.001f, t_max, &rec) of the reference (rayweek1.cpp:104-108, :152-339) ----------------------------
// One 32-byte record per ray (R1_CAST_CLOSEST) or one byte (R1_CAST_ANY); no color().
// t_max is strict (rayweek1.cpp:298, :307: `temp < t_max`).  A sphere's offer is fixed before the compare with t_max (the comment above
// exact_offer), so the answer is the minimum offer, ties to the lowest index, IF it is < t_max.  The tree walk is seeded with best = t_max
// so that it prunes what lies beyond; the walks' update rule (t < best) | (t == best & id < best_id) starts at best_id = 0xFFFFFFFF and
// so admits an offer EQUAL to t_max — which is why every form ends in store's `best < t_max`: an admitted t == t_max is a miss, and
// anything below it replaces it by the same rule (r1_offer.h: written as one compare of {t bits, index}; its form 2 admits a t of FLT_MAX
// against a t_max of FLT_MAX in the same way, and bvh_advance settles that back to "none" before this store sees it).  The grid's walk starts at FLT_MAX and is filtered the same way; the reference form's
// exact_test compares with the running t_max itself, strictly: seeded with the ray's t_max it IS rayweek1.cpp:284-314.
// A ray with a non-finite origin or (normalised) direction, or a t_max that is NaN or <= 0.001, is a miss before any walk (load).
struct R1CastJob
{
    typedef R1CastArgs Args;
    static constexpr bool BOUNCES = false;
    static constexpr int waves(const bool big) { return big ? R1_CAST_WAVES_BIG : R1_CAST_WAVES_SMALL; }
    static constexpr bool root_by_slots(const bool big) { return !big; } // (r1_builds.h r1_root_by_slots: the big-scene cast kernel would spill seven SGPRs with it)

    V3 o, d;
    float t_max; // (+inf -> FLT_MAX)
    uint32_t best_id; // the walk's answer (step)
    float best;

    __device__ __forceinline__ void idle() { o = mk(0, 0, 0), d = mk(0, 0, 1), t_max = FLT_MAX; }
    __device__ __forceinline__ bool load(const Args &A, const uint32_t i)
    {
        const float4 a = A.rays[2 * (size_t)i], b = A.rays[2 * (size_t)i + 1];
        o = mk(a.x, a.y, a.z);
        d = vunit(mk(b.x, b.y, b.z)); // Ray::Ray, rayweek1.cpp:107
        t_max = a.w > FLT_MAX ? FLT_MAX : a.w;
        return query_finite(o.x) && query_finite(o.y) && query_finite(o.z) && query_finite(d.x) && query_finite(d.y) && query_finite(d.z) && t_max > 0.001f; // (false for a NaN t_max)
    }
    __device__ __forceinline__ void seed(float &best) const { best = t_max; }
    __device__ __forceinline__ V3 O() const { return o; }
    __device__ __forceinline__ V3 D() const { return d; }
    __device__ __forceinline__ bool step(const Args &, const uint32_t id, const float t, uint32_t, int)
    {
        best_id = id, best = t;
        return true;
    }
    __device__ __forceinline__ void finish(const Args &A, const uint32_t i, const bool walked) const { store(A, i, walked ? best_id : 0xFFFFFFFFu, best); }
    // the hit record of rayweek1.cpp:316-322 (as shade_level computes hp and n), or the miss record; R1_CAST_ANY: one byte
    __device__ __forceinline__ void store(const Args &A, const uint32_t ray, const uint32_t best_id, const float best) const
    {
        const bool hit = best_id != 0xFFFFFFFFu && best < t_max;
        if (A.mode != 0u) // (wave-uniform)
        {
            ((uint8_t *)A.out)[ray] = hit ? 1 : 0;
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
        float4 *dst = (float4 *)A.out + 2 * (size_t)ray;
        dst[0] = r0, dst[1] = r1;
    }
};

// ---- the path job: color(Ray(o, d), scene, 0) of the reference (rayweek1.cpp:517-534) with the caller's stream states -------------------------
// A complete walk is one level of color(): shade_level, and then either the next walk of the same path or one 16-byte record
// {r, g, b, color() invocations}.  Same walks and same shade_level as the trace kernels, so the same bits.
// The attenuation stack is shade_level<true>'s: one hit index per entry in a global workspace laid out [entry][thread of the launch]
// (coalesced; r1_queries.cpp sizes it max_bounces x threads).  It needs no LDS, so these kernels keep the cast kernels' LDS budget, and
// it holds 32-bit indices, so small and big scenes share the code.
// t_max of a ray is ignored: color() always passes FLT_MAX (rayweek1.cpp:519).  A ray with a non-finite origin or (normalised) direction runs no
// color(): its record is {0, 0, 0, 0} (load's rule is the cast job's).  A stream state of zero is replaced before the path starts (r1_seed_guard, rays1_seed.h): xorshift32
// stays at zero for ever and random_in_unit_sphere would never return.
struct R1PathJob
{
    typedef R1TraceRaysArgs Args;
    static constexpr bool BOUNCES = true;
    static constexpr int waves(bool) { return R1_PATHQ_WAVES; }
    static constexpr bool root_by_slots(bool) { return true; }

    Path p; // (p.k: the ray's index in the launch)
    V3 col; // the path's radiance once step() has said that it ended

    __device__ __forceinline__ void idle()
    {
        p.o = mk(0, 0, 0), p.d = mk(0, 0, 1);
        p.s_scalar = p.s0 = p.s1 = p.s2 = 1u, p.k = 0u, p.depth = 0, p.sp = 0;
    }
    __device__ __forceinline__ bool load(const Args &A, const uint32_t i)
    {
        const float4 a = A.rays[2 * (size_t)i], b = A.rays[2 * (size_t)i + 1];
        p.o = mk(a.x, a.y, a.z);
        p.d = vunit(mk(b.x, b.y, b.z)); // Ray::Ray, rayweek1.cpp:107
        r1_sample_seed sd;
        if (A.seeds) // (wave-uniform)
        {
            const uint4 s = A.seeds[i];
            sd.scalar = s.x, sd.lane0 = s.y, sd.lane1 = s.z, sd.lane2 = s.w;
        }
        else
            sd = r1_seed_sample(0u, A.first + i, 0u);
        sd = r1_seed_guard(sd);
        p.s_scalar = sd.scalar, p.s0 = sd.lane0, p.s1 = sd.lane1, p.s2 = sd.lane2;
        p.k = i, p.depth = 0, p.sp = 0;
        return query_finite(p.o.x) && query_finite(p.o.y) && query_finite(p.o.z) && query_finite(p.d.x) && query_finite(p.d.y) && query_finite(p.d.z);
    }
    __device__ __forceinline__ void seed(float &) const {}
    __device__ __forceinline__ V3 O() const { return p.o; }
    __device__ __forceinline__ V3 D() const { return p.d; }
    __device__ __forceinline__ bool step(const Args &A, const uint32_t best_id, const float best, const uint32_t gtid, const int tid)
    {
        const int hit = best_id != 0xFFFFFFFFu ? (int)best_id : -1;
        return shade_level<true>(A.t, p, hit, best, nullptr, A.gstride, gtid, tid, col); // false: the scattered ray is in p, the next walk
    }
    __device__ __forceinline__ void finish(const Args &A, const uint32_t i, const bool walked) const
    {
        A.out[i] = walked ? make_float4(col.x, col.y, col.z, __uint_as_float(path_rays(p))) : make_float4(0.0f, 0.0f, 0.0f, 0.0f); // (no walk: no color())
    }
};

// ---- the scatter job: one color() body (rayweek1.cpp:517-534) with the recursion left to the caller -------------------------
// The path job's load — same r1_seed_guard in the same place — with R1_SCATTER_UNIT_DIRECTIONS deciding whether the direction is normalised
// (wave-uniform: a flag of the launch), one walk, and then in finish() the sky's three lines of shade_level or its hit arm, scatter_hit
// (r1_shade.hpp): the very function shade_level calls, so the level cannot drift from the trace kernels'.  No depth, no attenuation stack:
// 80 bytes per ray — the record, the scattered ray, the advanced states — as five whole 16-byte stores.  rays_out may be rays and seeds_out
// seeds: a lane has read ray i before it writes ray i, and no lane touches another lane's ray.
// Registers (profiles/r29/scatter_kernel_meta.txt, beside the cast's r10 / r15 and the path's r14): the job carries the Path's ten words through
// the walk where the cast carries seven, and scatter_hit's rejection loop and dielectric arm sit behind it.  Under the cast's bound of eight
// waves the compiler parks 6 .. 15 SGPRs in VGPR lanes (12 .. 32 v_readlane / v_writelane), with or without the root step by slots; under
// seven, 2 in three of the kernels; under the path job's six none, at 52 .. 60 VGPRs — so eight waves per SIMD fit all the same.  waves():
// R1_PATHQ_WAVES.  root_by_slots(): true, as the path job — at six waves the big-scene tree kernel holds it without a spill (58 VGPRs, 96
// SGPRs), which the cast's at eight does not.
struct R1ScatterJob
{
    typedef R1ScatterArgs Args;
    static constexpr bool BOUNCES = false;
    static constexpr int waves(bool) { return R1_PATHQ_WAVES; }
    static constexpr bool root_by_slots(bool) { return true; }

    Path p;
    uint32_t best_id; // the walk's answer (step)
    float best;

    __device__ __forceinline__ void idle()
    {
        p.o = mk(0, 0, 0), p.d = mk(0, 0, 1);
        p.s_scalar = p.s0 = p.s1 = p.s2 = 1u, p.k = 0u, p.depth = 0, p.sp = 0;
    }
    __device__ __forceinline__ bool load(const Args &A, const uint32_t i)
    {
        const float4 a = A.rays[2 * (size_t)i], b = A.rays[2 * (size_t)i + 1];
        p.o = mk(a.x, a.y, a.z);
        p.d = mk(b.x, b.y, b.z);
        if (!(A.flags & R1_SCATTER_UNIT_DIRECTIONS)) // (wave-uniform)
            p.d = vunit(p.d); // Ray::Ray, rayweek1.cpp:107
        r1_sample_seed sd;
        if (A.seeds) // (wave-uniform)
        {
            const uint4 s = A.seeds[i];
            sd.scalar = s.x, sd.lane0 = s.y, sd.lane1 = s.z, sd.lane2 = s.w;
        }
        else
            sd = r1_seed_sample(0u, A.first + i, 0u);
        sd = r1_seed_guard(sd);
        p.s_scalar = sd.scalar, p.s0 = sd.lane0, p.s1 = sd.lane1, p.s2 = sd.lane2;
        p.k = i, p.depth = 0, p.sp = 0;
        return query_finite(p.o.x) && query_finite(p.o.y) && query_finite(p.o.z) && query_finite(p.d.x) && query_finite(p.d.y) && query_finite(p.d.z);
    }
    __device__ __forceinline__ void seed(float &) const {}
    __device__ __forceinline__ V3 O() const { return p.o; }
    __device__ __forceinline__ V3 D() const { return p.d; }
    __device__ __forceinline__ bool step(const Args &, const uint32_t id, const float t, uint32_t, int)
    {
        best_id = id, best = t;
        return true;
    }
    __device__ __forceinline__ void finish(const Args &A, const uint32_t i, const bool walked)
    {
        // no walk: R1_SCATTER_NONE {0 0 0 NONE} {FLT_MAX -1 R1_MAT_NONE 0}, a ray of zero bytes, the guarded states
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(R1_SCATTER_NONE));
        float4 r1 = make_float4(FLT_MAX, __int_as_float(-1), __uint_as_float((uint32_t)R1_MAT_NONE), 0.0f);
        float4 n0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n1 = n0;
        if (walked)
        {
            if (best_id != 0xFFFFFFFFu)
            {
                uint32_t type;
                f4 sh;
                const bool on = scatter_hit(A.t.scene, p, (int)best_id, best, type, sh);
                const uint32_t scene_index = ((const r1_gu32 *)A.active_to_scene)[best_id];
                const bool glass = type == 2u;
                r0 = on ? make_float4(glass ? 1.0f : sh.y, glass ? 1.0f : sh.z, glass ? 1.0f : sh.w, __int_as_float(R1_SCATTER_SCATTERED))
                        : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(R1_SCATTER_ABSORBED)); // Metal::scatter() == false, rayweek1.cpp:432
                r1 = make_float4(best, __uint_as_float(scene_index), __uint_as_float(type), 0.0f);
                n0 = make_float4(p.o.x, p.o.y, p.o.z, FLT_MAX);
                n1 = make_float4(p.d.x, p.d.y, p.d.z, 0.0f);
            }
            else
            {
                // miss: sky (rayweek1.cpp:532-534), lerp = (1 - t) * a + t * b (mymath.h:212-216): shade_level's three lines
                const float t = 0.5f * (p.d.y + 1.0f);
                const float omt = 1.0f - t;
                r0 = make_float4(omt * 1.0f + t * 0.5f, omt * 1.0f + t * 0.7f, omt * 1.0f + t * 1.0f, __int_as_float(R1_SCATTER_SKY));
            }
        }
        float4 *rec = A.out + 2 * (size_t)i, *ray = A.rays_out + 2 * (size_t)i;
        rec[0] = r0, rec[1] = r1;
        ray[0] = n0, ray[1] = n1;
        A.seeds_out[i] = make_uint4(p.s_scalar, p.s0, p.s1, p.s2);
    }
};

// ---- the feature job: first-hit albedo, normal and depth of a frame's own primary rays, summed per pixel ------------------
// An item is a PIXEL of a window of the frame, not a ray: load() makes sample 0's ray with camera_ray — the function r1_camera_rays_kernel
// and start_sample call, so the ray is the render's — and step() adds what the walk found and makes the next sample's ray; the job
// BOUNCES until the pixel's spp samples are through.  The camera and the frame's numbers are read from the kernel arguments where a sample
// starts, and camera_ray's stream states die with it: nothing but the sums, the ray, the pixel and the sample index crosses a walk.
//   hit      albedo += the sphere's (1, 1, 1 for a dielectric: Material::scatter's weight, the scatter job's rule), normal += (p - centre) *
//            inv_radius (the cast job's n), depth += t, hits += 1
//   miss     albedo += the sky of the ray (shade_level's three lines); normal, depth and hits stay
//   a sample whose origin or normalised direction is not finite (the cast job's load rule) adds nothing and takes no walk
// Plain fp32 adds in sample order, then one multiply by (float)(1.0f / spp) each: r1_render_linear's arithmetic, so a pixel without a
// hit has that call's value.  One 32-byte record per pixel as two 16-byte stores; no atomics, no LDS of its own, no sample records.
// Registers (profiles/r34/features_kernel_meta.txt, beside the cast's r10 / r15, the path's r14 and the scatter's r29): the job carries 16 words
// across a walk — seven sums, hits, the ray, the pixel, the sample — where the cast carries seven and the scatter job ten.  Under the bounds
// 4, 5 and 6 waves the compiler gives one and the same code: 57 VGPRs (tree) and 61 (grid), so eight waves per SIMD fit all the same, with
// the SGPR file at its limit of 106 and 2 .. 11 SGPRs parked in VGPR lanes (4 .. 33 v_readlane / v_writelane): the camera's 19 words beside
// the walk's table bases.  Under eight it keeps 78 SGPRs and parks 27 .. 48 (81 .. 152 lane moves, 100 .. 150 instructions more) for 54 .. 60
// VGPRs.  Without the root step by slots the small-scene tree kernel parks none and is 152 instructions shorter; the others do not change.
// On the device (profiles/r34/features.txt) eight waves and the plain root step both stay inside the run-to-run spread of six waves with
// the step: waves() R1_PATHQ_WAVES' value, root_by_slots() true, as the path and scatter jobs.
#ifndef R1_FEATURE_WAVES
#define R1_FEATURE_WAVES 6
#endif
#ifndef R1_FEATURE_ROOT_BY_SLOTS
#define R1_FEATURE_ROOT_BY_SLOTS true
#endif
struct R1FeatureJob
{
    typedef R1FeatureArgs Args;
    static constexpr bool BOUNCES = true;
    static constexpr int waves(bool) { return R1_FEATURE_WAVES; }
    static constexpr bool root_by_slots(bool) { return R1_FEATURE_ROOT_BY_SLOTS; }

    V3 o, d;        // the sample's ray
    V3 albedo, normal;
    float depth;
    uint32_t hits;
    uint32_t xy;    // x | y << 16: the pixel in the frame (width, height <= 65535)
    uint32_t s;     // the sample the ray belongs to

    __device__ __forceinline__ void idle()
    {
        o = mk(0, 0, 0), d = mk(0, 0, 1);
        albedo = normal = mk(0, 0, 0), depth = 0.0f, hits = 0u, xy = 0u, s = 0u;
    }
    // the ray of the first finite sample from s on; false: the pixel has none left
    __device__ __forceinline__ bool aim(const Args &A)
    {
        for (; s < (uint32_t)A.t.spp; ++s)
        {
            Path p;
            const int x = (int)(xy & 0xFFFFu), y = (int)(xy >> 16);
            d = vunit(camera_ray(A.t.width, A.t.inv_w, A.t.inv_h, A.t.cam, p, x, y, s, A.t.seed)); // Ray::Ray, rayweek1.cpp:107
            o = p.o;
            if (query_finite(o.x) && query_finite(o.y) && query_finite(o.z) && query_finite(d.x) && query_finite(d.y) && query_finite(d.z))
                return true;
        }
        return false;
    }
    __device__ __forceinline__ bool load(const Args &A, const uint32_t i)
    {
        const uint32_t w = A.first + i; // the pixel's index in the window
        const uint32_t wy = fastdiv(w, A.div_win_w), wx = w - wy * A.win_w;
        xy = (A.x0 + wx) | ((A.y0 + wy) << 16);
        albedo = normal = mk(0, 0, 0), depth = 0.0f, hits = 0u, s = 0u;
        return aim(A);
    }
    __device__ __forceinline__ void seed(float &) const {}
    __device__ __forceinline__ V3 O() const { return o; }
    __device__ __forceinline__ V3 D() const { return d; }
    __device__ __forceinline__ bool step(const Args &A, const uint32_t id, const float t, uint32_t, int)
    {
        if (id != 0xFFFFFFFFu)
        {
            // the hit record of rayweek1.cpp:316-322 as the cast job stores it; the rows as scatter_hit reads them
            const f4 e = ((const f4 *)A.t.scene.exact)[id];
            const f4 sh = ((const f4 *)A.t.scene.shade)[id];
            const bool glass = __float_as_uint(((const f4 *)A.t.scene.mat)[id].x) == 2u;
            const V3 hp = vadd(o, vscale(d, t));
            const V3 n = vscale(vsub(hp, mk(e.x, e.y, e.z)), sh.x);
            albedo = vadd(albedo, mk(glass ? 1.0f : sh.y, glass ? 1.0f : sh.z, glass ? 1.0f : sh.w));
            normal = vadd(normal, n);
            depth += t;
            ++hits;
        }
        else
        {
            // miss: sky (rayweek1.cpp:532-534), lerp = (1 - t) * a + t * b (mymath.h:212-216): shade_level's three lines
            const float k = 0.5f * (d.y + 1.0f);
            const float omk = 1.0f - k;
            albedo = vadd(albedo, mk(omk * 1.0f + k * 0.5f, omk * 1.0f + k * 0.7f, omk * 1.0f + k * 1.0f));
        }
        ++s;
        return !aim(A); // false: the next sample's ray is in o, d
    }
    // (walked false: every sample was non-finite — the sums are the zeros load() left)
    __device__ __forceinline__ void finish(const Args &A, const uint32_t, const bool) const
    {
        const float inv = A.t.inv_spp;
        const uint32_t wx = (xy & 0xFFFFu) - A.x0, wy = (xy >> 16) - A.y0;
        float4 *dst = A.out + 2 * ((size_t)wy * A.stride + wx);
        dst[0] = make_float4(albedo.x * inv, albedo.y * inv, albedo.z * inv, depth * inv);
        dst[1] = make_float4(normal.x * inv, normal.y * inv, normal.z * inv, __uint_as_float(hits));
    }
};

// ---- LDS staging (as r1_trace_body stages its own copies) ---------------------------------------------------------------------------------
namespace
{

// The workgroup's copy of the node table at dst.  Small scenes (LN): the whole table with 16-bit child references, the root step's code
// in node 0's K slot and the flat tree's y slab in node 1's pad slots, where bvh_advance<LN> looks for them.  Big scenes: the
// breadth-first top of the table; the rest goes through the vector L1.
// (T by value: read through a reference, the root step's words are no longer kernel arguments the compiler may fetch ahead of the
// tid tests, and the prologue comes out nine instructions longer than r1_trace_body's)
template <bool LN>
__device__ __forceinline__ void stage_nodes(const R1TraceArgs T, float4 *dst, const int tid)
{
    for (uint32_t i = (uint32_t)tid; i < T.bvh_lds_f4; i += R1_BLOCK)
    {
        float4 q = T.scene.bvh_nodes[i];
        if (LN && (i & 3u) == 3u) // {A K child0 child1}: 16-bit child references
            q.z = __uint_as_float(r1_ref16(__float_as_uint(q.z))), q.w = __uint_as_float(r1_ref16(__float_as_uint(q.w)));
        dst[i] = q;
    }
    // (written by the threads that copied those rows: program order)
    if (LN && tid == 3)
        ((float *)dst)[13] = __uint_as_float(T.scene.bvh_root_leaf | (T.scene.bvh_flat_e >= 0.0f ? 4u : 0u));
    if (LN && tid == 7 && T.scene.bvh_flat_e >= 0.0f)
        ((float *)dst)[28] = T.scene.bvh_flat_m, ((float *)dst)[29] = T.scene.bvh_flat_e;
    __syncthreads();
}

// small scenes: the workgroup's copy of the grid's 16-bit cell table and ids at dst
__device__ __forceinline__ void stage_grid(const R1TraceArgs T, float4 *dst, const int tid)
{
    const R1GridCArgs *ga = (const R1GridCArgs *)(uintptr_t)T.grid;
    const float4 *src = (const float4 *)(const r1_gu32 *)ga->tab;
    const uint32_t n16 = ga->lds_bytes / 16u;
    for (uint32_t i = (uint32_t)tid; i < n16; i += R1_BLOCK)
        dst[i] = src[i];
    __syncthreads();
}

} // namespace

// ---- box tree ---------------------------------------------------------------------------------------------------------------------------
// Persistent: the waves claim chunks of the ray array from one atomic cursor, and bvh_advance runs with CARRY — a lane whose walk is
// complete hands it to its job and, once the job has written its record, takes the next ray while the longest walks of the wave go on
// (the shape of the trace kernels' loop, r1_trace_body).  A job that goes on (a path that scattered) starts its next walk at the root
// next to the walks the wave carries.  LDS: the traversal stack, then the node table (stage_nodes).
template <class JOB, bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, JOB::waves(BIG)) r1_query_tree_kernel(const typename JOB::Args A)
{
    constexpr bool LN = !BIG;
    typedef typename IdxType<!LN>::type TS; // traversal-stack entry: uint16_t with the LDS table, else uint32_t
    extern __shared__ uint32_t s_trav[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t gtid = blockIdx.x * R1_BLOCK + threadIdx.x;
    const size_t trav_words = (size_t)A.t.bvh_depth * R1_BLOCK * sizeof(TS) / 4;
    const float4 *lnodes = (const float4 *)(s_trav + trav_words);
    const uint32_t top = LN ? 0u : A.t.bvh_lds_f4 >> 2;
    stage_nodes<LN>(A.t, (float4 *)(s_trav + trav_words), tid);

    JOB J;
    J.idle();
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
                ray = q_next + rank;
                alive = J.load(A, ray);
                if (alive)
                    trav_start(tv), J.seed(tv.best);
                else
                    J.finish(A, ray, false); // no walk; the lane asks again
            }
            q_next += min((uint32_t)__popcll(need), avail);
            need = __ballot(!alive);
        }
        const unsigned long long live = __ballot(alive);
        if (live == 0ull)
            break;
        // ---- walk with carry-over, then the job of the lanes whose walk is complete ----
        bvh_advance<false, true, LN, TS, JOB::root_by_slots(BIG)>(A.t.scene, J.O(), J.D(), tv, (TS *)s_trav, tid, (uint32_t)__popcll(live), nullptr, lnodes, top);
        if (alive && tv.cur == R1_BVH_DONE)
        {
            if (J.step(A, tv.best_id, tv.best, gtid, tid))
            {
                J.finish(A, ray, true);
                alive = false;
            }
            else
                trav_start(tv), J.seed(tv.best);
        }
    }
}

// ---- uniform grid -----------------------------------------------------------------------------------------------------------------------
// grid_trace is a complete walk per call, so a wave works its chunk off 64 rays at a time; a job that BOUNCES loops over the walks of
// those 64 until the last of them has ended.  Small scenes: the grid's 16-bit table in LDS behind the fallback's traversal stack; rays
// too far for the grid take the tree walk from the global table (root_leaf = 0 in the arguments: it starts at the root), exactly as the
// grid trace kernel arranges it.
template <class JOB, bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, JOB::waves(BIG)) r1_query_grid_kernel(const typename JOB::Args A)
{
    extern __shared__ uint32_t s_trav[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t gtid = blockIdx.x * R1_BLOCK + threadIdx.x;
    const size_t gtrav_words = (size_t)A.t.bvh_depth * R1_BLOCK;
    const uint16_t *ltab = (const uint16_t *)(s_trav + gtrav_words);
    if (!BIG)
        stage_grid(A.t, (float4 *)(s_trav + gtrav_words), tid);
    uint32_t q_next = 0, q_end = 0;
    for (;;)
    {
        if (q_next == q_end && !chunk_claim(A.cursor, A.claim, A.n, lane, q_next, q_end))
            break;
        const uint32_t ray = q_next + (uint32_t)lane;
        const bool mine = ray < q_end;
        q_next = min(q_next + 64u, q_end);
        JOB J;
        J.idle();
        bool alive = false;
        if (mine)
        {
            alive = J.load(A, ray);
            if (JOB::BOUNCES && !alive)
                J.finish(A, ray, false); // (!BOUNCES: written below)
        }
        while (!JOB::BOUNCES || __ballot(alive) != 0ull)
        {
            float best;
            uint32_t best_id;
            const bool fb = grid_trace<false, !BIG>(A.t, (R1GridCArgs *)(uintptr_t)A.t.grid, alive, J.O(), J.D(), best, best_id, ltab, tid, nullptr);
            if (__ballot(fb) != 0ull)
            {
                // fallback: the tree walk from scratch, exact for any origin; the outliers' offer is kept (the tree presents them again)
                Trav fv;
                trav_start(fv);
                fv.best = best, fv.best_id = best_id;
                if (!fb)
                    fv.cur = R1_BVH_DONE;
                bvh_advance<false, false, false, uint32_t, false, R1_OFFER_FORM_GRID>(A.t.scene, J.O(), J.D(), fv, s_trav, tid, 64u, nullptr, nullptr);
                best = fv.best, best_id = fv.best_id;
            }
            if ((JOB::BOUNCES ? alive : mine) && J.step(A, best_id, best, gtid, tid))
            {
                J.finish(A, ray, JOB::BOUNCES || alive); // (BOUNCES: only a lane that is alive comes here)
                alive = false;
            }
            if (!JOB::BOUNCES)
                break; // (one walk per ray: no vote)
        }
    }
}

// ---- reference form: every active sphere through exact_test in index order, walk by walk (the reference's own loop; the on-device cross-check) ----
template <class JOB>
__global__ void __launch_bounds__(R1_BLOCK) r1_query_reference_kernel(const typename JOB::Args A)
{
    const uint32_t stride = gridDim.x * R1_BLOCK;
    const uint32_t gtid = blockIdx.x * R1_BLOCK + threadIdx.x;
    for (uint32_t i = gtid; i < A.n; i += stride)
    {
        JOB J;
        const bool alive = J.load(A, i);
        while (alive)
        {
            float t_hit = FLT_MAX;
            int hit = -1;
            J.seed(t_hit);
            sweep_reference(A.t.scene, J.O(), J.D(), t_hit, hit);
            if (J.step(A, (uint32_t)hit, hit >= 0 ? t_hit : FLT_MAX, gtid, (int)threadIdx.x))
                break;
        }
        J.finish(A, i, alive);
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
        R1CastJob J;
        J.idle();
        bool alive = false;
        if (i < A.n)
            alive = J.load(A, i);
        Trav tv;
        trav_start(tv);
        J.seed(tv.best);
        if (!alive)
            tv.cur = R1_BVH_DONE;
        bvh_advance<false, false, false, uint32_t>(A.t.scene, J.O(), J.D(), tv, s_trav, (int)threadIdx.x, 64u, nullptr, nullptr);
        J.step(A, tv.best_id, tv.best, 0u, 0);
        if (i < A.n)
            J.finish(A, i, alive);
    }
}
#endif

// ---- launchers (called from r1_queries.cpp) --------------------------------------------------------------------------------------------------
// variant: R1_V_TREE, R1_V_GRID or R1_V_REFERENCE — the structure the rays walk; null: no such kernel
template <class JOB>
static const void *query_kernel(const int variant, const int big)
{
    if (variant == R1_V_REFERENCE)
        return (const void *)r1_query_reference_kernel<JOB>;
    if (variant == R1_V_GRID)
        return big ? (const void *)r1_query_grid_kernel<JOB, true> : (const void *)r1_query_grid_kernel<JOB, false>;
    if (variant == R1_V_TREE)
        return big ? (const void *)r1_query_tree_kernel<JOB, true> : (const void *)r1_query_tree_kernel<JOB, false>;
    return nullptr;
}

// plain: the tuning library's plain tree form of the cast job
static const void *query_kernel(const int job, const int variant, const int big, const int plain)
{
#ifdef R1_TUNING
    if (plain && job == R1_JOB_CAST && variant == R1_V_TREE)
        return (const void *)r1_cast_plain_kernel;
#endif
    if (plain)
        return nullptr;
    return job == R1_JOB_CAST       ? query_kernel<R1CastJob>(variant, big)
           : job == R1_JOB_PATH     ? query_kernel<R1PathJob>(variant, big)
           : job == R1_JOB_SCATTER  ? query_kernel<R1ScatterJob>(variant, big)
           : job == R1_JOB_FEATURES ? query_kernel<R1FeatureJob>(variant, big)
                                    : nullptr;
}

// One launcher and one occupancy query, keyed by job, structure and big; args: the job's argument struct.  The C names below are their
// typed fronts for r1_queries.cpp.
static hipError_t query_launch(int job, const void *args, int variant, int big, int plain, int blocks, size_t dyn_lds, hipStream_t stream)
{
    const void *kernel = query_kernel(job, variant, big, plain);
    if (!kernel)
        return hipErrorInvalidValue;
    void *argv[1] = {(void *)args};
    (void)hipLaunchKernel(kernel, dim3(blocks), dim3(R1_BLOCK), argv, dyn_lds, stream);
    return hipGetLastError(); // (a launch's error, read and cleared as behind hipLaunchKernelGGL)
}

static hipError_t query_occupancy(int job, int variant, int big, int plain, size_t dyn_lds, int *blocks_per_cu)
{
    const void *kernel = query_kernel(job, variant, big, plain);
    if (!kernel)
        return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, kernel, R1_BLOCK, dyn_lds);
}

extern "C" hipError_t r1_launch_cast(const R1CastArgs *args, int variant, int big, int plain, int blocks, size_t dyn_lds, hipStream_t stream)
{
    return query_launch(R1_JOB_CAST, args, variant, big, plain, blocks, dyn_lds, stream);
}
extern "C" hipError_t r1_cast_occupancy(int variant, int big, int plain, size_t dyn_lds, int *blocks_per_cu)
{
    return query_occupancy(R1_JOB_CAST, variant, big, plain, dyn_lds, blocks_per_cu);
}
extern "C" hipError_t r1_launch_trace_rays(const R1TraceRaysArgs *args, int variant, int big, int blocks, size_t dyn_lds, hipStream_t stream)
{
    return query_launch(R1_JOB_PATH, args, variant, big, 0, blocks, dyn_lds, stream);
}
extern "C" hipError_t r1_trace_rays_occupancy(int variant, int big, size_t dyn_lds, int *blocks_per_cu)
{
    return query_occupancy(R1_JOB_PATH, variant, big, 0, dyn_lds, blocks_per_cu);
}
extern "C" hipError_t r1_launch_scatter_rays(const R1ScatterArgs *args, int variant, int big, int blocks, size_t dyn_lds, hipStream_t stream)
{
    return query_launch(R1_JOB_SCATTER, args, variant, big, 0, blocks, dyn_lds, stream);
}
extern "C" hipError_t r1_scatter_rays_occupancy(int variant, int big, size_t dyn_lds, int *blocks_per_cu)
{
    return query_occupancy(R1_JOB_SCATTER, variant, big, 0, dyn_lds, blocks_per_cu);
}
extern "C" hipError_t r1_launch_features(const R1FeatureArgs *args, int variant, int big, int blocks, size_t dyn_lds, hipStream_t stream)
{
    return query_launch(R1_JOB_FEATURES, args, variant, big, 0, blocks, dyn_lds, stream);
}
extern "C" hipError_t r1_features_occupancy(int variant, int big, size_t dyn_lds, int *blocks_per_cu)
{
    return query_occupancy(R1_JOB_FEATURES, variant, big, 0, dyn_lds, blocks_per_cu);
}
