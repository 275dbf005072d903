// r1_shade.hpp — one color() level behind the hit test (shade_level) and the attenuation stack it pushes to and unwinds.
// Internal linkage (anonymous namespace).
#ifndef R1_SHADE_HPP
#define R1_SHADE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "r1_device.h"
#include "r1_exact_math.h"
#include "r1_scatter.h"
#include "r1_stack_words.h"
#include "r1_dev_math.hpp"

#pragma clang fp contract(off)

// The shade phase's bookkeeping, trimmed, each step behind a macro so that the tuning build can measure it alone
// (`make tuning EXTRA=-DR1_STACK_PAD=0`).
#ifndef R1_STACK_PAD
#define R1_STACK_PAD 1 // small scenes: attenuation words padded with the identity row (r1_stack_words.h); 0: the unwind selects 1.0f for the empty slots
#endif
#ifndef R1_HIT_OFFSET32
#define R1_HIT_OFFSET32 1 // small scenes: the hit record's three rows through the tables' scalar bases and one 32-bit byte offset
#endif

namespace
{

// Attenuation stack.  Small scenes: packed in LDS, three 10-bit sphere indices per word.  Big
// scenes (> 1023 active spheres): one u32 per entry in a global workspace laid out
// [entry][global thread] (coalesced); its traffic is nothing next to a 100 k-sphere sweep.
template <bool BIG, int LW = R1_STACK_WORDS>
__device__ __forceinline__ void stack_push(uint32_t *stack, uint32_t *gstack, uint32_t gstride, uint32_t gtid, int tid, int sp, uint32_t idx)
{
    if (BIG)
    {
        gstack[(size_t)sp * gstride + gtid] = idx;
        return;
    }
    if (LW < R1_STACK_WORDS && sp >= 3 * LW) // deep entries (rare): global workspace, [entry - 3 LW][global thread]
    {
        // (the lane's part of the address is formed HERE: as a loop-invariant 64-bit value it is hoisted out of the tracing loop and spilled to scratch)
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        const uint32_t g = (gtid & ~(uint32_t)(R1_BLOCK - 1)) | (uint32_t)t_; // (= gtid, rebuilt from the workgroup's wave-uniform part)
        ((r1_gu32 *)gstack)[(uint32_t)(sp - 3 * LW) * gstride + g] = idx;
        return;
    }
    if (R1_STACK_PAD)
    {
        // (sp is in [0, 51): an unsigned multiply-shift, not the signed division)
        const uint32_t w = r1_stack_word((uint32_t)sp), sh = r1_stack_shift((uint32_t)sp, w);
        uint32_t *const slot = stack + w * R1_BLOCK + tid;
        *slot = r1_stack_push_word(*slot, sh, idx); // (sh == 0 opens the word: the pad in its upper slots, nothing of its old contents kept)
        return;
    }
    const int w = sp / 3, sh = (sp - 3 * w) * 10;
    uint32_t v = stack[w * R1_BLOCK + tid];
    v = (v & ~(0x3FFu << sh)) | (idx << sh);
    stack[w * R1_BLOCK + tid] = v;
}
template <bool BIG>
__device__ __forceinline__ uint32_t stack_get(const uint32_t *stack, const uint32_t *gstack, uint32_t gstride, uint32_t gtid, int tid, int e)
{
    if (BIG)
        return gstack[(size_t)e * gstride + gtid];
    const int w = e / 3, sh = (e - 3 * w) * 10;
    return (stack[w * R1_BLOCK + tid] >> sh) & 0x3FFu;
}

// ---- the hit arm of a color() level: the hit record (rayweek1.cpp:316-322), the material's draws, Material::scatter (r1_scatter.h) and the
// Ray constructor's normalisation.  The scattered ray replaces p.o, p.d and the stream states of p advance.  Returns whether the material
// scattered: false is Metal::scatter() == false (rayweek1.cpp:432).  type: R1_MAT_* of the sphere; sh: its {inv_radius, albedo rgb}.
// Shared by shade_level — every trace kernel and the path queries — and the scatter queries' job (r1_query_kernels.hip), which is this
// arm and nothing else.
// SMALL: the caller knows 0 <= hit <= 1022 (a small scene) — the three rows are addressed by the tables' wave-uniform bases and one 32-bit
// byte offset, as the unwind's gathers are, instead of three 64-bit per-lane addresses.
template <bool SMALL = false>
__device__ __forceinline__ bool scatter_hit(const R1DeviceScene &S, Path &p, const int hit, const float t_hit, uint32_t &type, f4 &sh)
{
    // hit record (rayweek1.cpp:316-322)
    f4 e, mt;
    if (SMALL)
    {
        const uint32_t off = (uint32_t)hit * (uint32_t)sizeof(f4);
        e = *(const f4 *)((const char *)S.exact + off);
        sh = *(const f4 *)((const char *)S.shade + off);
        mt = *(const f4 *)((const char *)S.mat + off);
    }
    else
    {
        e = ((const f4 *)S.exact)[hit];
        sh = ((const f4 *)S.shade)[hit];
        mt = ((const f4 *)S.mat)[hit];
    }
    const V3 hp = vadd(p.o, vscale(p.d, t_hit));
    const V3 n = vscale(vsub(hp, mk(e.x, e.y, e.z)), sh.x);
    type = __float_as_uint(mt.x);
    // Lambertian and Metal both draw random_in_unit_sphere from the x4 stream
    // (rayweek1.cpp:405, :430; Metal even with fuzz == 0): one shared loop
    V3 rius = mk(0, 0, 0);
    if (type != 2u)
        rius = random_in_unit_sphere(p);
    V3 dir; // un-normalised scattered direction; Ray::Ray normalises (rayweek1.cpp:107)
    if (type == 0u)
        dir = r1s_lambertian(hp, n, rius); // Lambertian::scatter rayweek1.cpp:403-409
    else
    {
        // Metal and Dielectric both reflect (rayweek1.cpp:414-417): once, for whichever of the two arms the wave's lanes take
        // (r1_scatter.h)
        const float ddn = vdot(p.d, n);
        const V3 refl = r1s_reflect(p.d, n, ddn);
        if (type == 1u)
            dir = r1s_metal(refl, rius, mt.y); // Metal::scatter rayweek1.cpp:427-433
        else
        {
            // Dielectric::scatter rayweek1.cpp:470-511 (attenuation 1: nothing to push), without the outward normal;
            // mt.z = 1.0f / _refIdx, divided on the host (same IEEE division)
            const R1Dielectric k = r1s_dielectric(p.d, n, ddn, mt.y, mt.z);
            // refract rayweek1.cpp:439-452
            float reflect_prob = 1.0f;
            V3 refracted = mk(0, 0, 0);
            if (k.discriminant > 0)
            {
                refracted = r1s_refracted(p.d, n, ddn, k, r1_sqrt_exact(k.discriminant, true));
                reflect_prob = r1s_schlick(mt.w, k.cosine); // rayweek1.cpp:454-459
            }
            dir = (rand01(p.s_scalar) < reflect_prob) ? refl : refracted;
        }
    }
    const V3 nd = vunit_guarded(dir);
    p.o = hp;
    p.d = nd;
    return type == 2u || type == 0u || vdot(nd, n) > 0;
}

// ---- one color() level after the hit test (rayweek1.cpp:517-534): count the ray, then either
// scatter (new ray in p, hit index pushed on the attenuation stack) or finish the path: sky
// colour times the stacked attenuations, or black.  Returns true when the path has ended, with
// its radiance in `col`.  Shared by the megakernel and the wavefront kernels.
template <bool BIG, int LW = R1_STACK_WORDS>
__device__ __forceinline__ bool shade_level(const R1TraceArgs &A, Path &p, const int hit, const float t_hit, uint32_t *s_stack,
                                            const uint32_t gstride, const uint32_t gtid, const int tid, V3 &col)
{
    bool done = false; // (this level's ray, rayweek1.cpp:517, is counted through the depth: path_rays)
    col = mk(0, 0, 0);
    if (hit >= 0)
    {
        if (p.depth < A.max_bounces)
        {
            uint32_t type;
            f4 sh;
            if (scatter_hit<!BIG && R1_HIT_OFFSET32>(A.scene, p, hit, t_hit, type, sh))
            {
                if (type != 2u)
                {
                    stack_push<BIG, LW>(s_stack, A.gstack, gstride, gtid, tid, p.sp, (uint32_t)hit);
                    ++p.sp;
                }
            }
            else
                done = true; // Metal::scatter() == false -> Vec3(0,0,0), rayweek1.cpp:432, :528
            if (!done)
                ++p.depth; // (a path that ends here keeps its depth: its rays = depth + 1 whichever way it ends)
        }
        else
            done = true; // depth == MAX_BOUNCES: no scatter, no draws, black (rayweek1.cpp:523-528)
    }
    else
    {
        // miss: sky (rayweek1.cpp:532-534), lerp = (1 - t) * a + t * b (mymath.h:212-216)
        const float t = 0.5f * (p.d.y + 1.0f);
        const float omt = 1.0f - t;
        col = mk(omt * 1.0f + t * 0.5f, omt * 1.0f + t * 0.7f, omt * 1.0f + t * 1.0f);
        // unwind: attenuation * color(...) innermost first (rayweek1.cpp:525)
        if (BIG)
        {
            for (int e = p.sp - 1; e >= 0; --e)
            {
                const float4 sh = A.scene.shade[stack_get<BIG>(s_stack, A.gstack, gstride, gtid, tid, e)];
                col = mk(sh.y * col.x, sh.z * col.y, sh.w * col.z);
            }
        }
        else if (p.sp > 0)
        {
            int top = p.sp;
            if (LW < R1_STACK_WORDS)
            {
                int t2 = tid;
                asm volatile("" : "+v"(t2)); // (as in stack_push)
                const uint32_t g = (gtid & ~(uint32_t)(R1_BLOCK - 1)) | (uint32_t)t2;
                for (int e = top - 1; e >= 3 * LW; --e) // the deep entries first (innermost attenuation first)
                {
                    const float4 sh = A.scene.shade[((const r1_gu32 *)A.gstack)[(uint32_t)(e - 3 * LW) * gstride + g]];
                    col = mk(sh.y * col.x, sh.z * col.y, sh.w * col.z);
                }
                top = top < 3 * LW ? top : 3 * LW;
            }
            // packed stack: one LDS word holds entries 3w, 3w+1, 3w+2 (10 bits each); walk it word by word from the top
            // entry down.  The three albedos of a word are fetched together, whether the word is full or not (any 10-bit
            // index is inside the table, r1_sweep.cpp), and the slots above the top entry multiply by 1.0f, which changes
            // no bit: one round trip to the table per word instead of one per entry.
            int t_ = tid;
            asm volatile("" : "+v"(t_)); // (the lane's LDS offset is formed here: hoisted out of the tracing loop, tid * 4 was a spilled register reloaded at every path's end)
            if (R1_STACK_PAD)
            {
                // every word the same way: the slots above the top entry hold the pad, whose row is {0, 1, 1, 1} (r1_stack_words.h)
                // (not unrolled: a wave runs the longest of its lanes' trip counts, and a remainder loop in front of a four-word body adds its own)
#pragma clang loop unroll(disable)
                for (int w = (int)r1_stack_word((uint32_t)(top - 1)); w >= 0; --w)
                {
                    const uint32_t v = s_stack[w * R1_BLOCK + t_];
                    const float4 s2 = A.scene.shade[(v >> 20) & 0x3FFu], s1 = A.scene.shade[(v >> 10) & 0x3FFu], s0 = A.scene.shade[v & 0x3FFu];
                    float c[3] = {col.x, col.y, col.z};
                    const float a2[3] = {s2.y, s2.z, s2.w}, a1[3] = {s1.y, s1.z, s1.w}, a0[3] = {s0.y, s0.z, s0.w};
                    r1_stack_fold(c, a2, a1, a0);
                    col = mk(c[0], c[1], c[2]);
                }
            }
            else
            {
                int w = (top - 1) / 3, j = (top - 1) - 3 * w;
                for (; w >= 0; --w, j = 2)
                {
                    const uint32_t v = s_stack[w * R1_BLOCK + t_];
                    const float4 s2 = A.scene.shade[(v >> 20) & 0x3FFu], s1 = A.scene.shade[(v >> 10) & 0x3FFu], s0 = A.scene.shade[v & 0x3FFu];
                    const bool u2 = j >= 2, u1 = j >= 1;
                    col = mk((u2 ? s2.y : 1.0f) * col.x, (u2 ? s2.z : 1.0f) * col.y, (u2 ? s2.w : 1.0f) * col.z);
                    col = mk((u1 ? s1.y : 1.0f) * col.x, (u1 ? s1.z : 1.0f) * col.y, (u1 ? s1.w : 1.0f) * col.z);
                    col = mk(s0.y * col.x, s0.z * col.y, s0.w * col.z);
                }
            }
        }
        done = true;
    }
    return done;
}

} // namespace

#endif // R1_SHADE_HPP
