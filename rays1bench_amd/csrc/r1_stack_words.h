// r1_stack_words.h — the packed attenuation stack of the small-scene kernels (r1_shade.hpp stack_push, shade_level), written once and shared
// with the host (tools/check_stack_words.cpp, tests/test_stack_words_host.py), so that the CPU test checks the kernels' own code.
// DESIGN.md §4.35.
//
// A word holds the hit indices of entries 3w, 3w + 1 and 3w + 2 of a path, ten bits each (at most R1_MAX_ACTIVE_10BIT = 1023 active spheres:
// indices 0 .. 1022).  Index 1023 is the PAD: row 1023 of the shade table is {0, 1, 1, 1} (r1_sweep.cpp), so a slot that holds it multiplies
// the radiance by 1.0f, which changes no bit.  A word is opened — its first entry pushed — with the pad in its two upper slots, and later
// entries replace a pad (r1_stack_push_word); the unwind then folds every word of the path the same way, three gathers and nine multiplies, whether its upper
// slots are taken or not.
#ifndef R1_STACK_WORDS_H
#define R1_STACK_WORDS_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define R1_STACK_HD __host__ __device__ __forceinline__
#else
#define R1_STACK_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define R1_STACK_PAD_INDEX 1023u // (= R1_MAX_ACTIVE_10BIT, r1_device.h: the one 10-bit index no sphere has)

// entry sp -> its word: sp / 3 for sp in [0, 32768) as one 24-bit multiply and a shift (0x5556 = ceil(2^16 / 3); the stack holds at most 51 entries)
R1_STACK_HD uint32_t r1_stack_word(const uint32_t sp)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(sp, 0x5556u) >> 16;
#else
    return (sp * 0x5556u) >> 16;
#endif
}

// entry sp of word w = r1_stack_word(sp) -> the bit its ten bits start at: 10 (sp % 3) = 10 sp - 30 w, by 24-bit multiplies
R1_STACK_HD uint32_t r1_stack_shift(const uint32_t sp, const uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(__mul24((int)w, -30) + (int)__umul24(sp, 10u));
#else
    return sp * 10u - w * 30u;
#endif
}

// a word as its first entry leaves it: idx below two pads (bits 30 and 31 are nobody's: set here, never read)
R1_STACK_HD uint32_t r1_stack_open(const uint32_t idx)
{
    return idx | 0xFFFFFC00u;
}

// A push: the word with entry idx in the slot at bit sh, the slots below it as they were and EVERY slot above it the pad.  One form for
// every slot, no compare and no branch: with sh == 0 nothing of the old word is kept — that is r1_stack_open(idx), whatever an earlier
// path left there — and a later entry replaces a pad by its index and puts the pads above it back.
R1_STACK_HD uint32_t r1_stack_push_word(const uint32_t v, const uint32_t sh, const uint32_t idx)
{
    return (v & ~(0xFFFFFFFFu << sh)) | ((idx | 0xFFFFFC00u) << sh);
}

// One word of the unwind: col = a0 * (a1 * (a2 * col)) per channel, innermost — the highest slot — first.  s2, s1, s0: the albedo rgb of
// slots 2, 1, 0 as the table holds them (the pad's row for a slot above the path's top entry).
R1_STACK_HD void r1_stack_fold(float col[3], const float s2[3], const float s1[3], const float s0[3])
{
    for (int c = 0; c < 3; ++c)
        col[c] = s2[c] * col[c];
    for (int c = 0; c < 3; ++c)
        col[c] = s1[c] * col[c];
    for (int c = 0; c < 3; ++c)
        col[c] = s0[c] * col[c];
}

#endif // R1_STACK_WORDS_H
