// r1_offer.h — the closest-offer update rule of the hit tests as ONE unsigned compare, written once and shared with the host
// (tools/check_offer_host.cpp, tests/test_offer_rule_host.py), so that the CPU test checks the kernels' own code.  DESIGN.md §4.33.
//
// ---- the closest-offer rule ----
// Every walk keeps the minimum offer with ties to the lowest sphere index (the reference's in-order loop with its strict `<`):
//     better = (t < best) | ((t == best) & (id < best_id))
// three compares.  A positive float's bit pattern orders as an unsigned integer, so with
//     key(t, id) = bits(t) << 32 | id
// the rule is key(t, id) < key(best, best_id): one v_cmp_lt_u64 on the register pairs (id : t) and (best_id : best).
// PRECONDITION: `t > 0.001f` has been tested (the caller ANDs it in, in either order) — t is a positive number or +inf, never a
// NaN — and `best` is a positive number: >= 0.001, FLT_MAX for "none", or a caller's t_max (the query walks).  Then
//   * bits(t) < bits(best)  <=>  t < best,  and  bits(t) == bits(best)  <=>  t == best  (no zeros, no NaN on either side);
//   * +inf orders above FLT_MAX and loses, as it does in the float compare.
// Without the precondition the two differ only where the float rule is false for every id: a NaN `t` equal in bits to a NaN `best`.
// `t < FLT_MAX` is NOT part of this function: with the "none" state (FLT_MAX, 0xFFFFFFFF) a t of FLT_MAX itself would win the key
// compare where the rule rejects it.  Form 1 keeps that compare in the callers as it was.  Form 2 folds it exactly: the callers drop it, so
// a walk whose closest offer so far is "none" may come to hold (FLT_MAX, id) — the only state the compare makes reachable: +inf orders
// above FLT_MAX, and below FLT_MAX the key compare implies t <= best < FLT_MAX — and r1_offer_settle puts "none" back where the walk
// hands its state on (once per call of bvh_advance instead of once per sphere).  In between, (FLT_MAX, id) and (FLT_MAX, none) behave
// alike: every box test and every offer below FLT_MAX sees best = FLT_MAX either way, and offers of FLT_MAX itself only trade ids that
// the settle discards.  A query walk that starts at a caller's t_max < FLT_MAX never leaves best <= t_max, where the compare was implied.
#ifndef R1_OFFER_H
#define R1_OFFER_H

#include <float.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define R1_OFFER_HD __host__ __device__ __forceinline__
#else
#define R1_OFFER_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

R1_OFFER_HD uint32_t r1_offer_bits(const float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
#endif
}

// {t bits, sphere index}: what the sweeps' exact phases combine with a 64-bit atomic min, and what r1_offer_better compares
R1_OFFER_HD unsigned long long r1_offer_key(const float t, const uint32_t id)
{
    return ((unsigned long long)r1_offer_bits(t) << 32) | id;
}

// The rule above in either form — 1 and 2: the key compare, 0: the three compares written out; precondition: t > 0.001f already tested, best positive.
// R1_OFFER_FORM is the tree walks' (leaf_quad, leaf_root: frame and query kernels; 0 is what they did before, 1 the compare alone: kept for the A/B).
// R1_OFFER_FORM_GRID is the grid kernels' — grid_trace and the tree walk they fall back to — and stays 0: the compare wants (id : t) and
// (best_id : best) in adjacent register pairs, which took every grid kernel four more VGPRs and the small-scene LAT / PASS / LISTED builds
// from 62 to 66, a wave per SIMD.
#ifndef R1_OFFER_FORM
#define R1_OFFER_FORM 2
#endif
#ifndef R1_OFFER_FORM_GRID
#define R1_OFFER_FORM_GRID 0
#endif

template <int FORM>
R1_OFFER_HD bool r1_offer_better_form(const float t, const uint32_t id, const float best, const uint32_t best_id)
{
    if (FORM != 0)
        return r1_offer_key(t, id) < r1_offer_key(best, best_id);
    return (t < best) | ((t == best) & (id < best_id));
}

// the whole update predicate of a leaf test for a lane that holds a candidate: in range (0.001, FLT_MAX) and better
template <int FORM>
R1_OFFER_HD bool r1_offer_update_form(const float t, const uint32_t id, const float best, const uint32_t best_id)
{
    if (FORM == 2)
        return (t > 0.001f) & r1_offer_better_form<FORM>(t, id, best, best_id);
    return (t > 0.001f) & (t < FLT_MAX) & r1_offer_better_form<FORM>(t, id, best, best_id);
}

// form 2: the index a walk hands on with its closest offer `best` (forms 0 and 1: best_id as it is)
template <int FORM>
R1_OFFER_HD uint32_t r1_offer_settle_form(const float best, const uint32_t best_id)
{
    return FORM == 2 ? (best < FLT_MAX ? best_id : 0xFFFFFFFFu) : best_id;
}

R1_OFFER_HD bool r1_offer_better(const float t, const uint32_t id, const float best, const uint32_t best_id)
{
    return r1_offer_better_form<R1_OFFER_FORM>(t, id, best, best_id);
}

#endif // R1_OFFER_H
