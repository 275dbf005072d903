// r1_dev_math.hpp — what every device function of the trace kernels is written in: the address-space typedefs, V3 and its operations in the
// reference's operation order, the xorshift32 streams, and a path's state.  Internal linkage (anonymous namespace).
#ifndef R1_DEV_MATH_HPP
#define R1_DEV_MATH_HPP

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "r1_device.h"
#include "r1_exact_math.h"

#pragma clang fp contract(off)

namespace
{

struct V3
{
    float x, y, z;
};

// read-only tables are addressed through the constant address space so that a wave-uniform
// index turns into scalar loads (SMEM) instead of vector loads
typedef float f4 __attribute__((ext_vector_type(4)));
typedef const f4 __attribute__((address_space(4))) *cf4_ptr;
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float f16 __attribute__((ext_vector_type(16)));
typedef const f16 __attribute__((address_space(4))) *cf16_ptr;
// a word of global memory (explicit: keeps rarely used stores / loads from becoming generic ones)
typedef uint32_t __attribute__((address_space(1))) r1_gu32;
typedef const R1GridArgs __attribute__((address_space(4))) R1GridCArgs; // the grid's arguments (device memory, read with scalar loads)

// Correctly rounded sqrt.  NOT __fsqrt_rn: without
// OCML_BASIC_ROUNDED_OPERATIONS hipcc maps __fsqrt_rn to the approximate v_sqrt_f32.  Plain
// sqrtf() and `/` are IEEE under -fhip-fp32-correctly-rounded-divide-sqrt (set in the Makefile).
// The hit tests and refract take their roots through r1_sqrt_exact (r1_exact_math.h): the same bits from half the instructions wherever no
// lane of the wave holds a tiny, zero, negative, infinite or NaN input, the compiler's function for the wave otherwise.
__device__ __forceinline__ float ieee_sqrt(float x) { return __builtin_sqrtf(x); }

__device__ __forceinline__ V3 mk(float x, float y, float z)
{
    V3 r;
    r.x = x, r.y = y, r.z = z;
    return r;
}
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 vscale(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 vneg(V3 a) { return mk(-a.x, -a.y, -a.z); }
// mymath.h:205-207: sum(a*b) = (x + y) + z
__device__ __forceinline__ float vdot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// mymath.h:211: v * (1.0f / length(v)); Ray::Ray normalises every direction (rayweek1.cpp:107).  The reciprocal length has the bits of
// 1.0f / ieee_sqrt(x) for every x, from one v_rsq_f32 (r1_exact_math.h): vunit is branch-free (the refill
// loop's site takes no new control flow without spilling the camera), vunit_guarded decides once per wave and belongs where the
// lanes of a branch normalise together (the ballot runs under the branch's exec mask).
__device__ __forceinline__ V3 vunit(V3 v) { return vscale(v, r1_rlen_total(vdot(v, v))); }
__device__ __forceinline__ V3 vunit_guarded(V3 v) { return vscale(v, r1_rlen_guarded(vdot(v, v), __builtin_amdgcn_ballot_w64(true))); }
__device__ __forceinline__ V3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }

// mymath.h:17-25
__device__ __forceinline__ uint32_t xorshift32(uint32_t &state)
{
    uint32_t x = state;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 15;
    state = x;
    return x;
}
// mymath.h:27-35 and the x4 forms :41-73 — all exact: a 24-bit integer times a power of two
__device__ __forceinline__ float rand01(uint32_t &s) { return (float)(xorshift32(s) & 0xFFFFFFu) * (1.0f / 16777216.0f); }
// myrand02 - 1 (mymath.h:32-35, :58-73; used as `myrand02_x4(state) - Vec3(1,1,1)` :229 and in
// random_in_unit_disk): the product with 2^-23 is exact, so the fused form rounds once, exactly
// where the reference's subtraction rounds
__device__ __forceinline__ float rand02_minus1(uint32_t &s) { return __fmaf_rn((float)(xorshift32(s) & 0xFFFFFFu), 1.0f / 8388608.0f, -1.0f); }

template <bool BIG>
struct IdxType
{
    typedef uint16_t type;
};
template <>
struct IdxType<true>
{
    typedef uint32_t type;
};

struct Path
{
    V3 o, d;                        // Ray::_origin, Ray::_dir (unit)
    uint32_t s_scalar, s0, s1, s2;  // ThreadData::state, lanes 0..2 of ThreadData::state4
    uint32_t k;                     // local sample index (output slot)
    // (color() invocations of the sample = depth + 1 when the path ends — every level counts one ray, rayweek1.cpp:517, and the depth
    //  grows by one per level that goes on: path_rays)
    int depth;                      // color()'s depth argument
    int sp;                         // entries on the attenuation stack
};

// color() invocations of a path that has just ended (shade_level returned true)
__device__ __forceinline__ uint32_t path_rays(const Path &p) { return (uint32_t)p.depth + 1u; }

// mymath.h:224-235
__device__ __forceinline__ V3 random_in_unit_sphere(Path &p)
{
    V3 r;
    do
    {
        r = mk(rand02_minus1(p.s0), rand02_minus1(p.s1), rand02_minus1(p.s2));
    } while (vdot(r, r) >= 1);
    return r;
}

} // namespace

#endif // R1_DEV_MATH_HPP
