// r1_hit_grid.hpp — the walk of the uniform grid (R1_VARIANT_GRID): grid_trace, over the cell walk of r1_grid_dda.h and exact_offer of
// r1_hit_sweep.hpp.  Internal linkage (anonymous namespace).
#ifndef R1_HIT_GRID_HPP
#define R1_HIT_GRID_HPP

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "r1_device.h"
#include "r1_grid_dda.h"
#include "r1_offer.h"
#include "r1_dev_math.hpp"
#include "r1_hit_sweep.hpp"

#pragma clang fp contract(off)

namespace
{

// ---- walk of the optional uniform grid (R1_VARIANT_GRID) ---------------------------------
// Per lane: the outliers (every ray, wave-uniform loop: scalar loads), then — unless the origin is too far for the grid's pad
// (r1g_far: the lane takes the fallback, the tree walk the caller runs) — the cells along the ray in order of entry t, every
// registered sphere of a cell through exact_offer, until the next cell is entered beyond the closest offer or the ray leaves the box
// (r1_grid_dda.h; why that presents every sphere that matters: r1_grid.cpp).  Result = minimum offer, ties to the lowest index.
// SMALL: the cell table and the ids are the workgroup's 16-bit copy in LDS (`ltab`); else 32-bit, through the vector L1.
// STATS: wstat[2] wave trips of the walk loop, [5] sphere tests summed over lanes, [9] cell steps summed over lanes, [17] outlier
// tests summed over lanes (published in stats slot 15); the caller counts the fallback lanes.
// Returns true if this lane takes the fallback.
template <bool STATS, bool SMALL>
__device__ __forceinline__ bool grid_trace(const R1TraceArgs &GA, R1GridCArgs *G, const bool alive, const V3 o, const V3 d,
                                           float &best, uint32_t &best_id, const uint16_t *ltab, const int tid, unsigned long long *wstat)
{
    R1GridCArgs &geom_args = *G;
    auto &geom = geom_args.geom; // (read in place: scalar loads where the walk uses a field)
    best = FLT_MAX, best_id = 0xFFFFFFFFu;
    if (!alive)
        return false;
    for (uint32_t k = 0; k < G->n_out; ++k) // (uniform index: scalar loads)
    {
        const uint32_t id = ((const __attribute__((address_space(4))) uint32_t *)G->outliers)[k];
        const float t = exact_offer(((cf4_ptr)GA.scene.exact)[id], o, d);
        const bool upd = (t < FLT_MAX) & r1_offer_better_form<R1_OFFER_FORM_GRID>(t, id, best, best_id); // (exact_offer: t > 0.001, or FLT_MAX)
        best = upd ? t : best;
        best_id = upd ? id : best_id;
    }
    if (STATS)
        wstat[17] += G->n_out, wstat[5] += G->n_out;
    if (r1g_far(geom, o.x, o.y, o.z))
        return true;
    R1GridRay r;
    bool walking = r1g_setup(geom, o.x, o.y, o.z, d.x, d.y, d.z, best, r);
    const f4 *__restrict__ tab = (const f4 *)GA.scene.exact;
    while (walking)
    {
        if (STATS)
        {
            wstat[9] += 1;
            if ((tid & 63) == __ffsll((long long)__ballot(1)) - 1)
                wstat[2] += 1;
        }
        const uint32_t c = r1g_cell(geom, r);
        const r1_gu32 *gtab = (const r1_gu32 *)G->tab;
        uint32_t k = SMALL ? (uint32_t)ltab[c] : gtab[c];
        const uint32_t e = SMALL ? (uint32_t)ltab[c + 1u] : gtab[c + 1u];
        if (STATS)
            wstat[5] += e - k;
        for (; k < e; ++k)
        {
            const uint32_t id = SMALL ? (uint32_t)ltab[G->n_start + k] : gtab[G->n_start + k];
            const float t = exact_offer(tab[id], o, d);
            const bool upd = (t < FLT_MAX) & r1_offer_better_form<R1_OFFER_FORM_GRID>(t, id, best, best_id); // (exact_offer: t > 0.001, or FLT_MAX)
            best = upd ? t : best;
            best_id = upd ? id : best_id;
        }
        walking = r1g_step(geom, r, best);
    }
    return false;
}

} // namespace

#endif // R1_HIT_GRID_HPP
