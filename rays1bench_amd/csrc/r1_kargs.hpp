// r1_kargs.hpp — the trace kernel's arguments read again from the kernarg segment at the place of use (fresh_args, R1_FRESH_ARGS;
// DESIGN.md §4.13).  Internal linkage (anonymous namespace).
#ifndef R1_KARGS_HPP
#define R1_KARGS_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "r1_device.h"

namespace
{

// The kernel's arguments read again from the kernarg segment (scalar loads, constant cache) at the place of use, through a pointer the
// optimiser cannot trace back to the prologue's loads.  hipcc keeps every argument field the loop uses in an SGPR from the prologue on;
// this kernel needs ~190 of them, ~90 live in lanes of two VGPRs, and every use of such a one is a v_readlane — a VALU issue slot, and
// whole 16-register tuples at a time (the fast-division constants of start_sample alone: ~90 v_readlane per loop iteration, 478 in the
// kernel).  A field read through R1_FRESH_ARGS is an s_load where it is used and occupies an SGPR only there.
typedef const __attribute__((address_space(4))) uint32_t *r1_kargs_ptr;
static_assert(sizeof(R1TraceArgs) % 4 == 0 && __is_trivially_copyable(R1TraceArgs), "fresh_args copies the argument block word by word");
union R1ArgWords
{
    R1TraceArgs a;
    uint32_t w[sizeof(R1TraceArgs) / 4];
    __device__ R1ArgWords() {}
};
// (a pointer that arrives as two loaded words is a generic pointer to the optimiser — flat loads.  The kernel's pointer arguments all
//  point to global memory: they are fetched as what they are, pointers into address space 1, the way clang passes them to a kernel)
template <typename T>
__device__ __forceinline__ T *global_ptr_at(r1_kargs_ptr k, const size_t offset)
{
    typedef __attribute__((address_space(1))) T *gptr;
    return (T *)*(const __attribute__((address_space(4))) gptr *)((const __attribute__((address_space(4))) char *)k + offset);
}
__device__ __forceinline__ void fresh_args(R1ArgWords &u)
{
    r1_kargs_ptr k = (r1_kargs_ptr)__builtin_amdgcn_kernarg_segment_ptr(); // (the kernel's one argument starts the segment)
    asm volatile("" : "+s"(k));
#pragma unroll
    for (uint32_t i = 0; i < sizeof(R1TraceArgs) / 4; ++i)
        u.w[i] = k[i]; // (only the words that are used afterwards are fetched)
#define R1_G(f) u.a.f = global_ptr_at<__typeof__(*u.a.f)>(k, __builtin_offsetof(R1TraceArgs, f));
    R1_G(scene.sweep) R1_G(scene.exact) R1_G(scene.shade) R1_G(scene.exact_g) R1_G(scene.members) R1_G(scene.mat) R1_G(scene.bvh_nodes) R1_G(scene.bvh_prims)
    R1_G(scene.bvh_ids) R1_G(queue) R1_G(samples) R1_G(num_rays) R1_G(gstack) R1_G(stats) R1_G(land_cnt) R1_G(land.out) R1_G(land.rays_dst)
    R1_G(land.frame_rays) R1_G(land.frame_left) R1_G(land.clear_heads) R1_G(land.owed_spill) R1_G(land.error) R1_G(grid)
#undef R1_G
}
#define R1_FRESH_ARGS(L)                                                                                                                  \
    R1ArgWords L##_words;                                                                                                                 \
    fresh_args(L##_words);                                                                                                                \
    const R1TraceArgs &L = L##_words.a;

} // namespace

#endif // R1_KARGS_HPP
