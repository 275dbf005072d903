// r1_exact_math.h — the correctly rounded fp32 square root of the trace kernels, and the reciprocal length of their ray
// normalisation (below), cheaper than the compiler's.
//
// Under -fhip-fp32-correctly-rounded-divide-sqrt `__builtin_sqrtf` becomes 16 VALU instructions: v_sqrt_f32 and a +-1 ulp
// correction (nine), plus seven that only serve inputs below 2^-96 (a 2^32 / 2^-16 scaling), zeros and +inf (a class
// fix-up).  r1_sqrt_exact() returns the same bits for EVERY input and spends those seven only where a wave holds such an
// input: one wave-uniform decision, then either a short sequence that is exact on
//     D = [2^-96, FLT_MAX]   (sign clear, exponent field 31..254)
// or the compiler's own function for the whole wave.  Two short sequences are kept here (R1_SQRT_FORM):
//   2 (B, the default)  v_rsq_f32 and five fused multiply-adds: eight instructions, one of them transcendental.  Equal to
//                       the rounded root on D for the v_rsq_f32 of gfx950 — established by comparing all 2^32 inputs on
//                       the chip (tools/check_exact_math.hip, tests/test_gpu_exact_math.py), not by argument; its numpy
//                       restatement fails below 2^-96 (tests/test_exact_math_host.py), which is why D ends there.
//   1 (A)               the compiler's nine: v_sqrt_f32, +-1 ulp, two fused multiply-adds, two compare / select pairs.  On D
//                       the scaling multiplies by one and the class fix-up never fires: the same function by construction.
//   0                   __builtin_sqrtf everywhere (what the kernels did before).
// DESIGN.md §4.18.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef R1_SQRT_FORM
#define R1_SQRT_FORM 2
#endif

// x in D: bits in [0x0F800000, 0x7F7FFFFF] — one add, one unsigned compare
__device__ __forceinline__ bool r1_sqrt_in_domain(const float x) { return (__float_as_uint(x) - 0x0F800000u) < 0x70000000u; }

// Form B.  y ~ 1/sqrt(x); g ~ sqrt(x), h ~ 1/(2 sqrt(x)); one coupled Newton step on both (r = 1/2 - h g), then the
// residual d = x - g^2 (exact in the fma) corrects g once more: the last fma rounds the root once.
__device__ __forceinline__ float r1_sqrt_rsq(const float x)
{
    const float y = __builtin_amdgcn_rsqf(x);
    float g = x * y;
    float h = 0.5f * y;
    const float r = __builtin_fmaf(-h, g, 0.5f);
    g = __builtin_fmaf(g, r, g);
    h = __builtin_fmaf(h, r, h);
    const float d = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(d, h, g);
}

// Form A.  s = v_sqrt_f32(x) is within 1 ulp; the residuals of its two neighbours decide which of the three is the rounded root.
__device__ __forceinline__ float r1_sqrt_ulp(const float x)
{
    float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    const float e_dn = __builtin_fmaf(-dn, s, x), e_up = __builtin_fmaf(-up, s, x);
    s = e_dn <= 0.0f ? dn : s;
    s = e_up > 0.0f ? up : s;
    return s;
}

template <int FORM>
__device__ __forceinline__ float r1_sqrt_on_domain(const float x)
{
    return FORM == 2 ? r1_sqrt_rsq(x) : (FORM == 1 ? r1_sqrt_ulp(x) : __builtin_sqrtf(x));
}

// Called by all lanes of the wave that are in the caller's branch; the result is defined for the lanes of `active_lanes` only
// (the others may hold anything and never force the slow arm).  `fast` tells the checker which arm the wave took.
// (the ballot is fed by the compare itself — through a bool it is lowered to v_cndmask 0/1 + v_cmp_ne — and makes the condition a
//  scalar: the compiler would run both arms under exec masks for a condition it takes for divergent)
template <int FORM>
__device__ __forceinline__ float r1_sqrt_exact_form(const float x, const unsigned long long active_lanes, bool &fast)
{
    if (FORM == 0)
    {
        fast = false;
        return __builtin_sqrtf(x);
    }
    fast = (active_lanes & __builtin_amdgcn_ballot_w64((__float_as_uint(x) - 0x0F800000u) >= 0x70000000u)) == 0ull;
    if (__builtin_expect(fast, 1))
        return r1_sqrt_on_domain<FORM>(x);
    return __builtin_sqrtf(x);
}

// the form for a caller that holds the ballot of its active lanes already (leaf_quad: its loop condition)
__device__ __forceinline__ float r1_sqrt_exact_lanes(const float x, const unsigned long long active_lanes)
{
    bool fast;
    return r1_sqrt_exact_form<R1_SQRT_FORM>(x, active_lanes, fast);
}

__device__ __forceinline__ float r1_sqrt_exact(const float x, const bool active)
{
    return r1_sqrt_exact_lanes(x, __builtin_amdgcn_ballot_w64(active)); // (active == true: the exec mask)
}

// ---- the reciprocal length of a ray direction: RN(1 / RN(sqrt(x))), the bits of `1.0f / __builtin_sqrtf(x)`
//
// The compiler's expression is 27 VALU instructions: its root (16) and its division (11: v_div_scale x2, v_rcp_f32, six
// fma / mul, v_div_fmas, v_div_fixup).  Here form B's root g is followed by a seed q of its reciprocal and Newton steps
// e = fma(-g, q, 1); q = fma(e, q, q).  The result is a unary function of x: like the root it is admissible only where the
// comparison of all 2^32 inputs on the chip finds no difference (tools/check_exact_rlen.hip, tests/test_gpu_exact_rlen.py;
// the figures below are that comparison's on an MI355X, profiles/r16/check_exact_rlen_form_*.txt).  R1_RLEN_FORM:
//   4 (the default)  q = v_rcp_f32(g), one step: 11 instructions, two of them transcendental.  0 mismatches.
//   3                q = v_rcp_f32(g) and the compiler's division chain without its no-ops: 16.  On D the root lies in
//                    [2^-48, 2^64), where v_div_scale returns its operands unscaled, v_div_fmas is an fma and v_div_fixup a
//                    move: the same function by construction, the form to fall back to.  0 mismatches.
//   1, 2             q = h + h (form B's h ~ 1/(2 sqrt(x)): no second transcendental), one step (11) / two steps (13).  NOT
//                    exact: 560 / 224 mismatches on D.  Two steps miss exactly the roots with an all-ones mantissa, whose
//                    reciprocal lies 2^-48 above a rounding tie and is approached from below.  Kept as the record of that.
//   0                `1.0f / __builtin_sqrtf(x)` everywhere (what the kernels did before)
#ifndef R1_RLEN_FORM
#define R1_RLEN_FORM 4
#endif

// x in D, y = v_rsq_f32(x)
template <int FORM>
__device__ __forceinline__ float r1_rlen_from_rsq(const float x, const float y)
{
    float g = x * y;
    float h = 0.5f * y;
    const float r = __builtin_fmaf(-h, g, 0.5f);
    g = __builtin_fmaf(g, r, g);
    h = __builtin_fmaf(h, r, h);
    const float d = __builtin_fmaf(-g, g, x);
    g = __builtin_fmaf(d, h, g); // r1_sqrt_rsq up to here: g = RN(sqrt(x))
    if (FORM == 3)
    {
        float q = __builtin_amdgcn_rcpf(g);
        float e = __builtin_fmaf(-g, q, 1.0f);
        q = __builtin_fmaf(e, q, q);
        float p = q; // (the chain's n * r with n == 1)
        e = __builtin_fmaf(-g, p, 1.0f);
        p = __builtin_fmaf(e, q, p);
        e = __builtin_fmaf(-g, p, 1.0f);
        return __builtin_fmaf(e, q, p);
    }
    float q = FORM == 4 ? __builtin_amdgcn_rcpf(g) : h + h;
    float e = __builtin_fmaf(-g, q, 1.0f);
    q = __builtin_fmaf(e, q, q);
    if (FORM == 2)
    {
        e = __builtin_fmaf(-g, q, 1.0f);
        q = __builtin_fmaf(e, q, q);
    }
    return q;
}

template <int FORM>
__device__ __forceinline__ float r1_rlen_on_domain(const float x)
{
    return FORM == 0 ? 1.0f / __builtin_sqrtf(x) : r1_rlen_from_rsq<FORM>(x, __builtin_amdgcn_rsqf(x));
}

// One wave-uniform decision, as r1_sqrt_exact_form: called by all lanes of the caller's branch, defined for `active_lanes`.
template <int FORM>
__device__ __forceinline__ float r1_rlen_guarded_form(const float x, const unsigned long long active_lanes, bool &fast)
{
    if (FORM == 0)
    {
        fast = false;
        return 1.0f / __builtin_sqrtf(x);
    }
    fast = (active_lanes & __builtin_amdgcn_ballot_w64((__float_as_uint(x) - 0x0F800000u) >= 0x70000000u)) == 0ull;
    if (__builtin_expect(fast, 1))
        return r1_rlen_on_domain<FORM>(x);
    return 1.0f / __builtin_sqrtf(x);
}

__device__ __forceinline__ float r1_rlen_guarded(const float x, const unsigned long long active_lanes)
{
    bool fast;
    return r1_rlen_guarded_form<R1_RLEN_FORM>(x, active_lanes, fast);
}

// Branch-free, for every bit pattern (the site inside the refill loop, where any new control flow costs the timed kernels
// eleven spilled SGPRs: §4.23).  Below 2^-96 the input is scaled by 2^64 and the result by 2^32: both are exact, both roundings
// commute with them, and no result is subnormal (1/sqrt(x) <= 2^74.5).  Whatever is not a positive number after the scaling
// — +-0, +inf, NaN, negative — takes the value v_rsq_f32 returned for it: +-inf, 0, NaN.  Those are exactly the lanes whose
// sequence ends in a NaN (0 * inf, inf * 0, or a NaN seed; on D every step is finite), so the route is `r != r`, one v_cmp_u_f32:
// a v_cmp_class would hold its mask in a VGPR of every kernel (+1 VGPR in 45 code objects, a wave per SIMD in five).
template <int FORM>
__device__ __forceinline__ float r1_rlen_total_form(const float x)
{
    if (FORM == 0)
        return 1.0f / __builtin_sqrtf(x);
    const bool tiny = x < 0x1p-96f;
    const float xs = tiny ? x * 0x1p+64f : x;
    const float y = __builtin_amdgcn_rsqf(xs);
    float r = r1_rlen_from_rsq<FORM>(xs, y);
    r = tiny ? r * 0x1p+32f : r;
    return r != r ? y : r;
}

__device__ __forceinline__ float r1_rlen_total(const float x) { return r1_rlen_total_form<R1_RLEN_FORM>(x); }
