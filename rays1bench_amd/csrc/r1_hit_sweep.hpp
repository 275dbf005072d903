// r1_hit_sweep.hpp — the exhaustive hit tests: the reference's per-sphere test (exact_test, exact_offer), the sweep in the reference's form
// (sweep_reference), the grouped sweep with its wave-cooperative exact phase (sweep_prefilter) and the cooperative sweep of a frame's tail
// (cooperative_sweep).  Internal linkage (anonymous namespace).
#ifndef R1_HIT_SWEEP_HPP
#define R1_HIT_SWEEP_HPP

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

// ---- the exact ray/sphere test: pass 1 + pass 2 of Hitable::hit for ONE sphere -----------
// rayweek1.cpp:192-202 (co, nb, c, discr with the reference's two FMA chains), :204 (sign
// bit), :294-313 (roots, strict compares, t_max shrinks).  Candidates must be presented in
// increasing index order (ties keep the earlier sphere).
__device__ __forceinline__ void exact_test(const f4 e, uint32_t idx, const V3 o, const V3 d, float &t_max, int &hit_index)
{
    const float cox = e.x - o.x;
    const float coy = e.y - o.y;
    const float coz = e.z - o.z;
    const float nb = __fmaf_rn(coz, d.z, __fmaf_rn(coy, d.y, cox * d.x));
    const float c = __fmaf_rn(coz, coz, __fmaf_rn(coy, coy, cox * cox)) - e.w;
    const float discr = nb * nb - c;
    if (!(__float_as_uint(discr) >> 31))
    {
        const float discr_sq = r1_sqrt_exact(discr, true); // (the lanes inside this branch vote: the ballot runs under its exec mask)
        float temp = nb - discr_sq;
        if (temp < t_max && temp > 0.001f)
        {
            t_max = temp;
            hit_index = (int)idx;
        }
        else
        {
            temp = nb + discr_sq;
            if (temp < t_max && temp > 0.001f)
            {
                t_max = temp;
                hit_index = (int)idx;
            }
        }
    }
}

// ---- sweep, reference form: every active sphere through exact_test ------------------------
__device__ __forceinline__ void sweep_reference(const R1DeviceScene &S, const V3 o, const V3 d, float &t_max, int &hit_index)
{
    const cf4_ptr tab = (cf4_ptr)S.exact;
    for (uint32_t i = 0; i < S.n_active; ++i)
        exact_test(tab[i], i, o, d, t_max, hit_index); // uniform index => scalar loads
}

// ---- sweep, prefilter form -----------------------------------------------------------------
// For unit d:  discr = (co.d)^2 - |co|^2 + r^2  with co = c - o
//            = (c.d - o.d)^2 - (|o|^2 - 2 c.o) - (|c|^2 - r^2)
// The test is applied to GROUPS of <= R1_GROUP_MAX nearby spheres through a bounding sphere
// (g, R) that contains every member (host, r1_sweep.cpp build_groups):
// Per ray:    negod = -(o.d), m2o = -2 o, oo' = |o|^2 (1 - 2^-15)
// Per group:  Kp = (|g|^2 - R^2) - 2^-15 (C^2 + R^2), rounded down, C^2 >= |g|^2 and every |c_i|^2
// Test:       fma(nb', nb', -t') >= Kp   with two 3-FMA chains nb', t'        => 7 FMA + 1 compare
// If the REFERENCE flags member i (its fp32 discriminant has a clear sign bit), the ray's line
// passes within sqrt(r_i^2 + E1) of c_i (E1 = the reference form's fp32 error), hence within
// R + E1/(2 r_i) of g, i.e. the group's real-number discriminant is >= -R E1 / r_i; with
// R <= 3.5 r_i (R1_GROUP_RATIO) and the error of this form itself that is > -2^-15 (C^2 + R^2 +
// |o|^2), so the group is flagged here; cooperative_exact then applies the
// reference's own rule to each member.
// What ONE candidate sphere offers a ray, independent of the other candidates: pass 2 of
// Hitable::hit (rayweek1.cpp:294-313) accepts t1 = nb - s when t1 > t_min, otherwise
// t2 = nb + s when t2 > t_min, each only if it is below the running t_max; since t2 >= t1 a
// sphere whose t1 fails `< t_max` cannot pass with t2, so the sphere's offer is fixed and the
// loop result is the minimum offer, ties to the lowest index (strict `<` keeps the earlier one).
// Returns FLT_MAX for "no offer".
__device__ __forceinline__ float exact_offer(const f4 e, const V3 o, const V3 d)
{
    const float cox = e.x - o.x;
    const float coy = e.y - o.y;
    const float coz = e.z - o.z;
    const float nb = __fmaf_rn(coz, d.z, __fmaf_rn(coy, d.y, cox * d.x));
    const float c = __fmaf_rn(coz, coz, __fmaf_rn(coy, coy, cox * cox)) - e.w;
    const float discr = nb * nb - c;
    float offer = FLT_MAX;
    if (!(__float_as_uint(discr) >> 31))
    {
        const float discr_sq = r1_sqrt_exact(discr, true); // (the lanes inside this branch vote: the ballot runs under its exec mask)
        const float t1 = nb - discr_sq;
        const float t = (t1 > 0.001f) ? t1 : nb + discr_sq;
        if (t > 0.001f && t < FLT_MAX)
            offer = t;
    }
    return offer;
}

// Wave-cooperative exact phase.  Flag counts per lane are very uneven (mean ~3 groups, max of
// 64 lanes ~10, a few rays skim a whole row of spheres), so the (ray, group) pairs of the whole
// wave are compacted into one dense LDS list and re-tested 64 member slots at a time by
// whichever lane comes next: full-width trips instead of mostly-empty ones.  Offers are
// combined per ray with a 64-bit LDS atomic min on {t bits, sphere index}: closest hit, ties to
// the lowest index — the reference's rule.  All of this must be called by ALL 64 lanes.
// IDX = uint16_t (<= 1023 groups: 6 lane bits + 10 group bits per pair) or uint32_t (6 + 26).
template <typename IDX>
struct PairBits
{
    static constexpr int value = sizeof(IDX) == 2 ? 10 : 26;
    static constexpr int cap = sizeof(IDX) == 2 ? R1_PAIR_CAP_SMALL : R1_PAIR_CAP; // pairs of one wave
};

// Inclusive prefix sum over the 64 lanes with data-parallel-primitive moves (no LDS round trips: the __shfl_up form was six dependent
// ds_bpermute_b32 plus compare / select / add each): Kogge-Stone inside every row of 16 lanes (row_shr 1, 2, 4, 8; lanes shifted in from
// outside the row read 0), then lane 15 of a row added to the next row (row_bcast:15 into rows 1 and 3) and lane 31 to the upper half
// (row_bcast:31 into rows 2 and 3).  All 64 lanes must be active.
__device__ __forceinline__ int wave_inclusive_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false); // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false); // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false); // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false); // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2, 3
    return v;
}

// `total` (lane, group) pairs are in `pairs`.  SLOTS == R1_GROUP_MAX: each pair expands to its
// member slots — 16 pairs x 4 members fill a trip, a lane takes pair (base + lane) / 4, member
// lane % 4.  SLOTS == 1: the pairs are single-sphere groups, one lane each.
// `rays` (optional): this wave's ray table in LDS, component c of lane l at rays[c * R1_BLOCK + l] — a lane then fetches its
// owner's ray with six ds_read_b32 (8 issue cycles each) instead of six ds_bpermute_b32 (24).  The table overlays the flag
// words / candidate lists, which are dead once the pair list is built.
template <bool STATS, typename IDX, int SLOTS>
__device__ __forceinline__ void exact_trips(const R1DeviceScene &S, const V3 o, const V3 d, const int total, const IDX *pairs,
                                            unsigned long long *best /* this wave's [64] */, const int lane, unsigned long long *wstat,
                                            const float *rays = nullptr)
{
    constexpr int IDX_BITS = PairBits<IDX>::value;
    constexpr int SHIFT = SLOTS == 1 ? 0 : 2;
    static_assert(SLOTS == 1 || (SLOTS == 4 && R1_GROUP_MAX == 4), "member-slot mapping assumes 4 spheres per group");
    const int slots = total * SLOTS;
    if (STATS)
        wstat[2] += (unsigned long long)((slots + 63) >> 6);
    for (int base = 0; base < slots; base += 64) // wave-uniform trip count
    {
        const int j = (base + lane) >> SHIFT;
        const bool have_pair = j < total;
        const uint32_t pr = have_pair ? (uint32_t)pairs[j] : ((uint32_t)lane << IDX_BITS);
        const int owner = (int)(pr >> IDX_BITS);
        const uint32_t grp = pr & ((1u << IDX_BITS) - 1u);
        const uint32_t slot = grp * R1_GROUP_MAX + (SLOTS == 1 ? 0u : (uint32_t)(lane & (R1_GROUP_MAX - 1)));
        const uint32_t idx = have_pair ? S.members[slot] : 0xFFFFFFFFu;
        const f4 sphere = ((const f4 *)S.exact_g)[slot]; // (no pair: group 0's slots, fetched and not used)
        V3 ro, rd;
        if (rays)
        {
            ro = mk(rays[0 * R1_BLOCK + owner], rays[1 * R1_BLOCK + owner], rays[2 * R1_BLOCK + owner]);
            rd = mk(rays[3 * R1_BLOCK + owner], rays[4 * R1_BLOCK + owner], rays[5 * R1_BLOCK + owner]);
        }
        else
        {
            ro.x = __shfl(o.x, owner, 64), ro.y = __shfl(o.y, owner, 64), ro.z = __shfl(o.z, owner, 64);
            rd.x = __shfl(d.x, owner, 64), rd.y = __shfl(d.y, owner, 64), rd.z = __shfl(d.z, owner, 64);
        }
        if (idx != 0xFFFFFFFFu)
        {
            const float t = exact_offer(sphere, ro, rd);
            if (t < FLT_MAX)
                atomicMin(&best[owner], r1_offer_key(t, idx)); // (the rule of r1_offer_better, applied by the LDS atomic)
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// writes this lane's ray into the wave's LDS ray table (see exact_trips); returns the wave's base pointer
__device__ __forceinline__ const float *publish_rays(uint32_t *scratch /* [>= 6][R1_BLOCK] */, const V3 o, const V3 d, const int tid)
{
    float *t = (float *)scratch;
    __builtin_amdgcn_wave_barrier(); // every lane has read what it needed from the scratch rows
    t[0 * R1_BLOCK + tid] = o.x, t[1 * R1_BLOCK + tid] = o.y, t[2 * R1_BLOCK + tid] = o.z;
    t[3 * R1_BLOCK + tid] = d.x, t[4 * R1_BLOCK + tid] = d.y, t[5 * R1_BLOCK + tid] = d.z;
    __builtin_amdgcn_wave_barrier();
    return t + (tid & ~63);
}

// Append path (big scenes): every lane holds `cnt` flagged group indices in cand[j][tid].
template <bool STATS, typename IDX>
__device__ __forceinline__ void cooperative_exact(const R1DeviceScene &S, const V3 o, const V3 d, int cnt, const uint32_t *cand,
                                                  IDX *pairs /* this wave's [R1_PAIR_CAP] */, unsigned long long *best /* this wave's [64] */,
                                                  const int tid, const int lane, unsigned long long *wstat)
{
    constexpr int IDX_BITS = PairBits<IDX>::value;
    const int incl = wave_inclusive_scan(cnt);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    const int excl = incl - cnt;
    for (int j = 0; j < cnt; ++j)
        pairs[excl + j] = (IDX)(((uint32_t)lane << IDX_BITS) | cand[j * R1_BLOCK + tid]);
    static_assert(R1_CAND_CAP >= 6, "the ray table needs six rows of the candidate list");
    const float *rays = publish_rays(const_cast<uint32_t *>(cand), o, d, tid);
    exact_trips<STATS, IDX, R1_GROUP_MAX>(S, o, d, total, pairs, best, lane, wstat, rays);
}

// Bit path (<= 1023 groups): every lane holds `nwords` 32-bit flag words in words[w][tid]; bit
// 31 - p of word w flags group gbase + 32 w + p.  More than R1_PAIR_CAP pairs in the wave (a
// wave of rays that all skim rows of spheres) are worked off half a word at a time: 16 flags per
// lane always fit.
template <bool STATS, typename IDX>
__device__ __forceinline__ void cooperative_bits(const R1DeviceScene &S, const V3 o, const V3 d, const uint32_t nwords, const uint32_t gbase,
                                                 const uint32_t *words, IDX *pairs, unsigned long long *best, const int tid, const int lane,
                                                 unsigned long long *wstat)
{
    constexpr int IDX_BITS = PairBits<IDX>::value;
    // flags of multi-member groups (ids < n_multi) and of single spheres are counted apart: the
    // former go to the front of `pairs`, the latter to its back, and are worked off with 4 and 1
    // member slot per pair.  Both counts ride one prefix sum (16 bits each).
    int cnt = 0;
    for (uint32_t w = 0; w < nwords; ++w)
    {
        const uint32_t word = words[w * R1_BLOCK + tid];
        const int first = (int)(gbase + 32u * w);      // group of bit 31
        const int nm = (int)S.n_multi - first;         // groups of this word below n_multi
        const uint32_t multi_mask = nm >= 32 ? 0xFFFFFFFFu : (nm <= 0 ? 0u : ~(0xFFFFFFFFu >> nm));
        cnt += __popc(word & multi_mask) + (__popc(word & ~multi_mask) << 16);
    }
    const int incl = wave_inclusive_scan(cnt);
    const int totals = __builtin_amdgcn_readlane(incl, 63);
    const int total_m = totals & 0xFFFF, total_s = totals >> 16;
    if (STATS)
        wstat[9] += (unsigned long long)((cnt & 0xFFFF) + (cnt >> 16));
    if (totals == 0)
        return;
    constexpr int CAP = PairBits<IDX>::cap;
    if (total_m + total_s <= CAP)
    {
        int pos_m = (incl - cnt) & 0xFFFF;
        int pos_s = CAP - 1 - ((incl - cnt) >> 16); // singles grow down from the end
        for (uint32_t w = 0; w < nwords; ++w)
        {
            uint32_t word = words[w * R1_BLOCK + tid];
            while (word)
            {
                const int p = __clz((int)word);
                word &= ~(0x80000000u >> p);
                const uint32_t g = gbase + 32u * w + (uint32_t)p;
                const IDX v = (IDX)(((uint32_t)lane << IDX_BITS) | g);
                if (g < S.n_multi)
                    pairs[pos_m++] = v;
                else
                    pairs[pos_s--] = v;
            }
        }
        static_assert(R1_BIT_WORDS >= 6 && R1_CAND_CAP >= 8, "the ray table needs six rows of the flag words");
        const float *rays = publish_rays(const_cast<uint32_t *>(words), o, d, tid); // the words of this batch are consumed
        exact_trips<STATS, IDX, R1_GROUP_MAX>(S, o, d, total_m, pairs, best, lane, wstat, rays);
        exact_trips<STATS, IDX, 1>(S, o, d, total_s, pairs + (CAP - total_s), best, lane, wstat, rays);
        return;
    }
    // more pairs than the list holds: work the flag words off in segments of CAP / 64 bits, whose
    // flags always fit (64 lanes x SEG bits)
    constexpr uint32_t SEG = (uint32_t)CAP / 64u, PER_WORD = 32u / SEG;
    for (uint32_t seg = 0; seg < PER_WORD * nwords; ++seg)
    {
        const uint32_t w = seg / PER_WORD, part = seg - w * PER_WORD;
        uint32_t word = words[w * R1_BLOCK + tid] & (((1u << SEG) - 1u) << (32u - SEG * (part + 1u)));
        const int c2 = __popc(word);
        const int incl2 = wave_inclusive_scan(c2);
        const int total2 = __builtin_amdgcn_readlane(incl2, 63);
        int pos = incl2 - c2;
        while (word)
        {
            const int p = __clz((int)word);
            word &= ~(0x80000000u >> p);
            pairs[pos++] = (IDX)(((uint32_t)lane << IDX_BITS) | (gbase + 32u * w + (uint32_t)p));
        }
        __builtin_amdgcn_wave_barrier();
        exact_trips<STATS, IDX, R1_GROUP_MAX>(S, o, d, total2, pairs, best, lane, wstat);
    }
}

// The sweep itself (formula and slack: see the comment block above exact_offer).  Called by all 64 lanes; lanes with
// alive == false never flag a candidate but help in the cooperative exact phase.
template <bool STATS, typename IDX, bool BLOCK_SYNC>
__device__ __forceinline__ void sweep_prefilter(const R1DeviceScene &S, const bool alive, const V3 o, const V3 d, float &t_max,
                                                int &hit_index, uint32_t *cand /* flag words [R1_BIT_WORDS][R1_BLOCK], or (big scenes) flagged groups [R1_CAND_CAP][R1_BLOCK] */,
                                                IDX *pairs /* [R1_BLOCK/64][R1_PAIR_CAP] */,
                                                unsigned long long *best /* [R1_BLOCK] */, f4 *tile /* BLOCK_SYNC: [2][R1_TILE_F4] */,
                                                const int tid, unsigned long long *wstat)
{
    const int lane = tid & 63;
    IDX *wpairs = pairs + (tid >> 6) * PairBits<IDX>::cap;
    unsigned long long *wbest = best + (tid & ~63);
    const unsigned long long NONE = ~0ull;

    const float negod = -__fmaf_rn(o.z, d.z, __fmaf_rn(o.y, d.y, o.x * d.x));
    const float oo = __fmaf_rn(o.z, o.z, __fmaf_rn(o.y, o.y, o.x * o.x));
    // dead lanes: t' = +inf => q = -inf (or NaN) => never >= Kp
    const float oo_adj = alive ? __fmaf_rn(oo, -0x1p-15f, oo) : __builtin_inff();
    const float mx = -2.0f * o.x, my = -2.0f * o.y, mz = -2.0f * o.z;

    wbest[lane] = NONE;
    int cnt = 0;

    // Pair layout (r1_sweep.cpp): 8 floats per two spheres {cx0 cx1 cy0 cy1 cz0 cz1 Kp0 Kp1}, so
    // that every v_pk_fma_f32 takes an aligned SGPR pair straight from the scalar load: two
    // spheres per VALU instruction, 3.5 + 1 instructions per sphere.  A chunk = 8 spheres =
    // two s_load_dwordx16; the NEXT chunk is requested before the current one is evaluated
    // (the table carries one never-candidate chunk of padding behind the last real one).
    const v2f dxx = {d.x, d.x}, dyy = {d.y, d.y}, dzz = {d.z, d.z};
    const v2f mxx = {mx, mx}, myy = {my, my}, mzz = {mz, mz};
    const v2f nod = {negod, negod}, ooa = {oo_adj, oo_adj};
    const cf16_ptr tab = (cf16_ptr)S.sweep;
    const uint32_t chunks = S.n_sweep >> 3; // r1_sweep.cpp pads to 8 spheres + one prefetch chunk

#define R1_PAIR(P, L, B)                                                                                               \
    {                                                                                                                  \
        const v2f cx = {L[B + 0], L[B + 1]}, cy = {L[B + 2], L[B + 3]}, cz = {L[B + 4], L[B + 5]};                     \
        const v2f nb = __builtin_elementwise_fma(cz, dzz, __builtin_elementwise_fma(cy, dyy, __builtin_elementwise_fma(cx, dxx, nod))); \
        const v2f t = __builtin_elementwise_fma(cz, mzz, __builtin_elementwise_fma(cy, myy, __builtin_elementwise_fma(cx, mxx, ooa))); \
        const v2f q = __builtin_elementwise_fma(nb, nb, -t);                                                           \
        c[2 * P] = q.x >= L[B + 6];                                                                                    \
        c[2 * P + 1] = q.y >= L[B + 7];                                                                                \
        any |= __ballot(c[2 * P]) | __ballot(c[2 * P + 1]);                                                            \
    }
#define R1_CHUNK_EVAL(L0, L1, CH)                                                                                      \
    {                                                                                                                  \
        bool c[8];                                                                                                     \
        unsigned long long any = 0;                                                                                    \
        R1_PAIR(0, L0, 0) R1_PAIR(1, L0, 8) R1_PAIR(2, L1, 0) R1_PAIR(3, L1, 8)                                        \
        if (any) /* wave-uniform: scalar branch */                                                                     \
        {                                                                                                              \
            /* a chunk adds at most 8 entries per lane: make room first, then append unchecked */                      \
            if (__ballot(cnt > R1_CAND_CAP - 8))                                                                       \
            {                                                                                                          \
                cooperative_exact<STATS, IDX>(S, o, d, cnt, cand, wpairs, wbest, tid, lane, wstat);                    \
                cnt = 0;                                                                                               \
            }                                                                                                          \
            _Pragma("unroll") for (int u = 0; u < 8; ++u) if (c[u])                                                    \
            {                                                                                                          \
                cand[cnt * R1_BLOCK + tid] = (uint32_t)(8 * (CH) + u);                                                 \
                ++cnt;                                                                                                 \
            }                                                                                                          \
        }                                                                                                              \
    }
    if (!BLOCK_SYNC)
    {
        // Flags are kept as BITS, one per group, shifted into a per-lane word: no branch, no
        // per-flag bookkeeping in the sweep; a word goes to LDS every 32 groups and the wave works a
        // batch of R1_BIT_WORDS words (256 groups) off at a time in cooperative_bits.  The word
        // collects the SIGN of q - Kp (one packed subtract per pair of groups + one v_alignbit_b32
        // per group: bits = 2 bits + sign; 13.4 issue cycles per pair against 17.2 for v_cmp +
        // v_addc, profiles/r01/isa_issue_costs.txt) and is inverted when stored: q >= Kp <=> the
        // difference is not negative (a float difference has the exact sign; equal gives +0).
#define R1_FLAG(RV) bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(RV), 31);
        // two pairs of groups side by side, statement by statement: the chains of one pair fill the wait states hipcc otherwise pads the
        // other's dependent v_pk_fma_f32 with (two s_nop per pair in the one-pair form)
#define R1_PAIR2_BITS(LA, BA, LB, BB)                                                                                  \
    {                                                                                                                  \
        const v2f cxa = {LA[BA + 0], LA[BA + 1]}, cya = {LA[BA + 2], LA[BA + 3]}, cza = {LA[BA + 4], LA[BA + 5]};      \
        const v2f cxb = {LB[BB + 0], LB[BB + 1]}, cyb = {LB[BB + 2], LB[BB + 3]}, czb = {LB[BB + 4], LB[BB + 5]};      \
        v2f nba = __builtin_elementwise_fma(cxa, dxx, nod), nbb = __builtin_elementwise_fma(cxb, dxx, nod);            \
        v2f ta = __builtin_elementwise_fma(cxa, mxx, ooa), tb = __builtin_elementwise_fma(cxb, mxx, ooa);              \
        nba = __builtin_elementwise_fma(cya, dyy, nba), nbb = __builtin_elementwise_fma(cyb, dyy, nbb);                \
        ta = __builtin_elementwise_fma(cya, myy, ta), tb = __builtin_elementwise_fma(cyb, myy, tb);                    \
        nba = __builtin_elementwise_fma(cza, dzz, nba), nbb = __builtin_elementwise_fma(czb, dzz, nbb);                \
        ta = __builtin_elementwise_fma(cza, mzz, ta), tb = __builtin_elementwise_fma(czb, mzz, tb);                    \
        const v2f qa = __builtin_elementwise_fma(nba, nba, -ta), qb = __builtin_elementwise_fma(nbb, nbb, -tb);        \
        const v2f kpa = {LA[BA + 6], LA[BA + 7]}, kpb = {LB[BB + 6], LB[BB + 7]};                                      \
        const v2f ra = qa - kpa, rb = qb - kpb;                                                                        \
        R1_FLAG(ra.x) R1_FLAG(ra.y) R1_FLAG(rb.x) R1_FLAG(rb.y)                                                        \
    }
#define R1_CHUNK_BITS(L0, L1) {R1_PAIR2_BITS(L0, 0, L0, 8) R1_PAIR2_BITS(L1, 0, L1, 8)}
        uint32_t bits = 0;
        uint32_t nwords = 0, gbase = 0; // wave-uniform
        // two register sets (A, B) alternate: while one chunk is evaluated the next one loads
        f16 a0 = tab[0], a1 = tab[1];
        uint32_t ch = 0;
        for (; ch + 1 < chunks; ch += 2)
        {
            // Scalar loads return out of order, so lgkmcnt can only be waited to 0: make set A land
            // BEFORE set B is requested (the empty asm "uses" A, which places the wait here), then
            // evaluate A with B in flight and no further wait.
            asm volatile("" ::"s"(a0[0]), "s"(a1[0]));
            const f16 b0 = tab[2 * ch + 2], b1 = tab[2 * ch + 3];
            __builtin_amdgcn_sched_barrier(0);
            R1_CHUNK_BITS(a0, a1)
            asm volatile("" ::"s"(b0[0]), "s"(b1[0]));
            a0 = tab[2 * ch + 4], a1 = tab[2 * ch + 5];
            __builtin_amdgcn_sched_barrier(0);
            R1_CHUNK_BITS(b0, b1)
            if (ch & 2u) // 32 groups since the last word
            {
                cand[nwords * R1_BLOCK + tid] = ~bits;
                if (++nwords == R1_BIT_WORDS)
                {
                    cooperative_bits<STATS, IDX>(S, o, d, nwords, gbase, cand, wpairs, wbest, tid, lane, wstat);
                    nwords = 0;
                    gbase = (ch + 2) * 8;
                }
            }
        }
        if (ch < chunks) // odd number of chunks: the last one is already in set A
        {
            R1_CHUNK_BITS(a0, a1)
            ++ch;
        }
        if (ch & 3u) // a partial word: left-align it
        {
            cand[nwords * R1_BLOCK + tid] = ~bits << (32u - 8u * (ch & 3u));
            ++nwords;
        }
        if (STATS)
        {
            wstat[5] += __builtin_readcyclecounter() - wstat[15];
            wstat[15] = __builtin_readcyclecounter();
        }
        cooperative_bits<STATS, IDX>(S, o, d, nwords, gbase, cand, wpairs, wbest, tid, lane, wstat);
#undef R1_CHUNK_BITS
#undef R1_PAIR2_BITS
#undef R1_FLAG
    }
    else
    {
        // Big scenes (BASELINE config 5: 100 k spheres = 3.2 MB of table).  The scalar cache
        // sustains under 1 B/clk/CU on misses (measured: 100 k spheres ran at a quarter of the
        // small-scene rate), so the table goes through the VECTOR memory path instead: the
        // workgroup stages R1_TILE_SPHERES-sphere tiles into LDS with coalesced 16-byte loads
        // (each byte fetched once per workgroup and shared by its 256 rays), double-buffered,
        // one barrier per tile, and every wave reads the tile back with broadcast ds_read_b128.
        // The whole workgroup runs the bounce loop in lock step (see the kernel).
        const f4 *gsrc = (const f4 *)S.sweep;
        const uint32_t n_tiles = S.n_sweep / R1_TILE_SPHERES;
        f4 r0 = gsrc[tid], r1 = gsrc[R1_BLOCK + tid];
        __syncthreads(); // every wave has left the previous sweep's last tile
        tile[tid] = r0, tile[R1_BLOCK + tid] = r1;
        __syncthreads();
        for (uint32_t ti = 0; ti < n_tiles; ++ti)
        {
            const f4 *cur = tile + (ti & 1u) * R1_TILE_F4;
            const f4 *nsrc = gsrc + (size_t)(ti + 1) * R1_TILE_F4; // the table carries one padding tile
            r0 = nsrc[tid], r1 = nsrc[R1_BLOCK + tid];
#pragma unroll 2
            for (uint32_t cc = 0; cc < R1_TILE_SPHERES / 8; ++cc)
            {
                const f4 *q4 = cur + cc * 8;
                const f4 x0 = q4[0], x1 = q4[1], x2 = q4[2], x3 = q4[3], x4 = q4[4], x5 = q4[5], x6 = q4[6], x7 = q4[7];
                const f16 l0 = __builtin_shufflevector(__builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7),
                                                       __builtin_shufflevector(x2, x3, 0, 1, 2, 3, 4, 5, 6, 7), 0, 1, 2, 3, 4, 5, 6, 7, 8,
                                                       9, 10, 11, 12, 13, 14, 15);
                const f16 l1 = __builtin_shufflevector(__builtin_shufflevector(x4, x5, 0, 1, 2, 3, 4, 5, 6, 7),
                                                       __builtin_shufflevector(x6, x7, 0, 1, 2, 3, 4, 5, 6, 7), 0, 1, 2, 3, 4, 5, 6, 7, 8,
                                                       9, 10, 11, 12, 13, 14, 15);
                R1_CHUNK_EVAL(l0, l1, ti * (R1_TILE_SPHERES / 8) + cc)
            }
            f4 *nxt = tile + ((ti + 1u) & 1u) * R1_TILE_F4;
            nxt[tid] = r0, nxt[R1_BLOCK + tid] = r1;
            __syncthreads();
        }
    }
#undef R1_CHUNK_EVAL
#undef R1_PAIR
    if (BLOCK_SYNC)
        cooperative_exact<STATS, IDX>(S, o, d, cnt, cand, wpairs, wbest, tid, lane, wstat);
    const unsigned long long key = wbest[lane];
    if (key != NONE)
    {
        t_max = __uint_as_float((uint32_t)(key >> 32));
        hit_index = (int)(uint32_t)(key & 0xFFFFFFFFull);
    }
}

// ---- the tail of a frame: a few live paths per wave ------------------------------------------------
// Every live ray of the wave in turn against ALL active spheres, lane l testing spheres l, l + 64, ...
// with the reference's per-sphere arithmetic (exact_offer), then the minimum offer, ties to the lowest
// index (the reference's in-order rule, see exact_offer).  Same result as the other sweeps; meant for
// waves that have only a handful of paths left (R1TraceArgs::coop_lanes): one such step costs the wave
// ~n_active / 64 sphere tests per ray and a single round of coalesced loads instead of a walk down the
// tree made of dependent fetches.  Called by all 64 lanes.
__device__ __forceinline__ void cooperative_sweep(const R1DeviceScene &S, unsigned long long live, const V3 o, const V3 d, float &t_max,
                                                  int &hit_index, const int lane)
{
    const f4 *__restrict__ tab = (const f4 *)S.exact;
    while (live) // wave-uniform
    {
        const int src = __ffsll((long long)live) - 1;
        live &= live - 1ull;
        const V3 ro = mk(__shfl(o.x, src, 64), __shfl(o.y, src, 64), __shfl(o.z, src, 64));
        const V3 rd = mk(__shfl(d.x, src, 64), __shfl(d.y, src, 64), __shfl(d.z, src, 64));
        unsigned long long key = ~0ull;
        for (uint32_t i = (uint32_t)lane; i < S.n_active; i += 64u)
        {
            const float t = exact_offer(tab[i], ro, rd);
            if (t < FLT_MAX)
            {
                const unsigned long long k = r1_offer_key(t, i); // t > 0: bit order = value order (r1_offer.h)
                key = k < key ? k : key;
            }
        }
        // the reference flags ~0.5 % of the spheres per ray: walk the few lanes that hold an offer
        unsigned long long best = ~0ull;
        unsigned long long offers = __ballot(key != ~0ull);
        while (offers)
        {
            const int l = __ffsll((long long)offers) - 1;
            offers &= offers - 1ull;
            const unsigned long long k = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(key >> 32), l) << 32) |
                                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, l);
            best = k < best ? k : best;
        }
        if (lane == src && best != ~0ull)
        {
            t_max = __uint_as_float((uint32_t)(best >> 32));
            hit_index = (int)(uint32_t)best;
        }
    }
}

} // namespace

#endif // R1_HIT_SWEEP_HPP
