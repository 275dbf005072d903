// r1_exact_math.h — the correctly rounded fp32 square root of the trace kernels, cheaper than the compiler's.
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
