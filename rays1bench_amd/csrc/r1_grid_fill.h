// r1_grid_fill.h — the arithmetic that re-registers moved spheres in the uniform grid (r1_regrid), shared by the device
// kernels (r1_regrid.hip) and the host restatement (r1_grid.cpp r1_grid_regrid_host), as r1_bvh_fill.h is shared by the builder and the refit.
// The rule is "geometry kept": the PLAN — what r1_build_grid decided for the arrays of r1_set_scene: which axes are flat, the cells of the
// others, V, the coordinate bound M, the walk margin delta, the outlier radius `big` — stays, and every sphere is classified against it by
// the builder's own expressions (r1_grid.cpp, quoted by line below).
//
// Everything here is correctly rounded fp64 + - * / sqrt and floor, comparisons and selects, and conversions to and from fp32
// (-ffp-contract=off holds for host and device code): both sides compute the same bits.  No library routine whose rounding could differ.
#ifndef R1_GRID_FILL_H
#define R1_GRID_FILL_H

#include <stdint.h>

#include "r1_bvh_fill.h"

#define R1_GRID_SPAN_LIMIT 64 // = R1_GRID_SPAN_MAX (r1_grid.h): a ball that overlaps more cells is an outlier
#define R1_REGRID_SLACK 2     // the id table holds R1_REGRID_SLACK x the plan's registrations + 64; a named constant, not a tuning knob

// What a regrid keeps of the build (by value in the kernels' arguments)
struct R1GridPlan
{
    float lo[3], cell[3], inv_cell[3]; // the build's; a flat axis's are re-stretched by every regrid
    int32_t n[3];
    int32_t flat[3];
    double V, delta, big, M;
    float v2;         // V^2 rounded down, as the build stored it
    uint32_t n_start; // cells + 1
    uint32_t regs;    // the build's registrations
};

// the id table's capacity
R1F_HD uint32_t r1gf_capacity(uint32_t plan_regs) { return (uint32_t)R1_REGRID_SLACK * plan_regs + 64u; }

// nextafterf(f, -inf) for finite f
R1F_HD float r1gf_next_down(float f) { return -r1f_next_up(-f); }
// largest float <= v / smallest float >= v (r1_grid.cpp round_down_f, round_up_f)
R1F_HD float r1gf_round_down(double v)
{
    float f = (float)v;
    if ((double)f > v)
        f = r1gf_next_down(f);
    return f;
}
R1F_HD float r1gf_round_up(double v)
{
    float f = (float)v;
    if ((double)f < v)
        f = r1f_next_up(f);
    return f;
}

// The registration radius rho_i (r1_grid.cpp:105-107, :151, :165) of a sphere with test radius rt at centre c, for the plan's V and delta
R1F_HD double r1gf_rho(float cx, float cy, float cz, double rt, double V, double delta)
{
    const double u = 0x1p-24;
    const double r_floor = 1e-4 * (1.0 + r1f_abs((double)cx) + r1f_abs((double)cy) + r1f_abs((double)cz));
    const double reff = r1f_max(rt, r_floor);
    const double rho0 = reff + (23.0 * u * V * V + 2.0 * u * rt * rt) / (2.0 * reff) + 5.0 * u * V;
    return (rho0 + delta) * (1.0 + 0x1p-40);
}

// The cells the ball (c, rho) overlaps, by the builder's exact ball-cell test (r1_grid.cpp cells_of), in its order (z, y, x).  The ball
// lies inside the box (r1gf_candidate), so a flat axis contributes its one cell at distance 0 whatever the re-stretch makes of it.
// keys == null: counts, and stops above R1_GRID_SPAN_LIMIT; else writes the (cell, id) pairs of a sphere whose count is known to be within
// the limit.  An axis range of more than limit + 2 cells overlaps more than `limit`: the ball's centre lies in a cell of each other axis,
// and along this one every cell strictly between the range's ends is within rho (the ends hold c -+ rho up to the builder's 1e-9) — so
// the count is above the limit without the loop, which then never walks more than (limit + 2)^3 cells.
R1F_HD uint32_t r1gf_cells(const R1GridPlan &P, float cx, float cy, float cz, double rho, uint32_t *keys, uint32_t *vals, uint32_t id)
{
    const double c[3] = {cx, cy, cz};
    int jlo[3], jhi[3];
    for (int a = 0; a < 3; ++a)
    {
        if (P.flat[a])
        {
            jlo[a] = jhi[a] = 0;
            continue;
        }
        const double lo = P.lo[a], cell = P.cell[a], top = (double)(P.n[a] - 1);
        const double l = __builtin_floor((c[a] - rho - lo) / cell - 1e-9), h = __builtin_floor((c[a] + rho - lo) / cell + 1e-9);
        jlo[a] = l < 0.0 ? 0 : (l > top ? P.n[a] - 1 : (int)l);
        jhi[a] = h < 0.0 ? 0 : (h > top ? P.n[a] - 1 : (int)h);
        if (jhi[a] - jlo[a] + 1 > R1_GRID_SPAN_LIMIT + 2)
            return R1_GRID_SPAN_LIMIT + 1u;
    }
    uint32_t count = 0;
    for (int jz = jlo[2]; jz <= jhi[2]; ++jz)
        for (int jy = jlo[1]; jy <= jhi[1]; ++jy)
            for (int jx = jlo[0]; jx <= jhi[0]; ++jx)
            {
                const int j[3] = {jx, jy, jz};
                double d2 = 0;
                for (int a = 0; a < 3; ++a)
                {
                    if (P.flat[a])
                        continue;
                    const double b0 = (double)P.lo[a] + j[a] * (double)P.cell[a], b1 = (double)P.lo[a] + (j[a] + 1) * (double)P.cell[a];
                    const double q = c[a] < b0 ? b0 - c[a] : (c[a] > b1 ? c[a] - b1 : 0.0);
                    d2 += q * q;
                }
                if (d2 <= rho * rho * (1.0 + 1e-12))
                {
                    if (keys)
                        keys[count] = (uint32_t)((jz * P.n[1] + jy) * P.n[0] + jx), vals[count] = id;
                    if (++count > R1_GRID_SPAN_LIMIT)
                        return count;
                }
            }
    return count;
}

#define R1GF_NONE 0u      // a non-finite centre: in neither list (the refit already says the sphere is never hit)
#define R1GF_OUTLIER 1u   // tested by every ray before the walk
#define R1GF_CANDIDATE 2u // radius and box admit it: the flat axes are stretched over these; registered unless its span is too large

// Steps 1-3 but for the span: a sphere's class against the plan, and its rho.  rb, rt: the device's radii row {bound, test}
R1F_HD uint32_t r1gf_candidate(const R1GridPlan &P, float cx, float cy, float cz, double rb, double rt, double &rho)
{
    rho = 0.0;
    if (!r1f_finite(cx) || !r1f_finite(cy) || !r1f_finite(cz))
        return R1GF_NONE;
    rho = r1gf_rho(cx, cy, cz, rt, P.V, P.delta);
    if (rb > P.big)
        return R1GF_OUTLIER;
    const double c[3] = {cx, cy, cz};
    for (int a = 0; a < 3; ++a)
    {
        // (the box must contain every registration ball and M must bound the box: r1_grid.cpp's exactness argument)
        const double lo = P.flat[a] ? -P.M : (double)P.lo[a];
        const double hi = P.flat[a] ? P.M : (double)P.lo[a] + (double)P.n[a] * (double)P.cell[a];
        if (c[a] - rho < lo || c[a] + rho > hi)
            return R1GF_OUTLIER;
    }
    return R1GF_CANDIDATE;
}

// The whole rule for one sphere: its class (R1GF_CANDIDATE here means REGISTERED), its rho, and the cells it registers in
R1F_HD uint32_t r1gf_classify(const R1GridPlan &P, float cx, float cy, float cz, double rb, double rt, double &rho, uint32_t &span, bool &candidate)
{
    span = 0u;
    const uint32_t k = r1gf_candidate(P, cx, cy, cz, rb, rt, rho);
    candidate = k == R1GF_CANDIDATE;
    if (!candidate)
        return k;
    span = r1gf_cells(P, cx, cy, cz, rho, nullptr, nullptr, 0u);
    if (span > R1_GRID_SPAN_LIMIT)
    {
        span = 0u;
        return R1GF_OUTLIER;
    }
    return R1GF_CANDIDATE;
}

// A flat axis's one cell over the current candidates (r1_grid.cpp:204, :213), clamped into [-M, M]: clo, chi the candidates' centres on
// the axis, rho_max their largest rho.  (The float roundings and the builder's 1 + 1e-12 may pass M by 2^-23 of it: delta's 32 u against
// the 6 sqrt(3) 2 u < 21 u the walk needs covers that many times over.)
R1F_HD void r1gf_stretch(double clo, double chi, double rho_max, double M, float &lo, float &cell, float &inv_cell)
{
    lo = r1gf_round_down(r1f_max(clo - rho_max, -M));
    const double top = r1f_min(chi + rho_max, M);
    cell = r1gf_round_up((top - (double)lo) * (1.0 + 1e-12));
    inv_cell = (float)(1.0 / (double)cell);
}

// What one workgroup (or the host's one pass) knows of its spheres: the box of the registered centres, and per axis the candidates'
// centres and their largest rho.  Min and max only: the order of merging changes no bit.
struct R1GridExtent
{
    double rlo[3], rhi[3]; // registered centres
    double clo[3], chi[3]; // candidates' centres
    double rho_max;        // of the candidates
    R1F_HD void clear()
    {
        for (int a = 0; a < 3; ++a)
            rlo[a] = clo[a] = 1e300, rhi[a] = chi[a] = -1e300;
        rho_max = 0.0;
    }
    R1F_HD void add(float cx, float cy, float cz, double rho, bool candidate, bool registered)
    {
        const double c[3] = {cx, cy, cz};
        for (int a = 0; a < 3; ++a)
        {
            if (candidate)
                clo[a] = r1f_min(clo[a], c[a]), chi[a] = r1f_max(chi[a], c[a]);
            if (registered)
                rlo[a] = r1f_min(rlo[a], c[a]), rhi[a] = r1f_max(rhi[a], c[a]);
        }
        if (candidate)
            rho_max = r1f_max(rho_max, rho);
    }
    R1F_HD void merge(const R1GridExtent &e)
    {
        for (int a = 0; a < 3; ++a)
        {
            rlo[a] = r1f_min(rlo[a], e.rlo[a]), rhi[a] = r1f_max(rhi[a], e.rhi[a]);
            clo[a] = r1f_min(clo[a], e.clo[a]), chi[a] = r1f_max(chi[a], e.chi[a]);
        }
        rho_max = r1f_max(rho_max, e.rho_max);
    }
};
#define R1GF_EXTENT_WORDS 13 // doubles of an R1GridExtent

// Steps 5 and 6: the geometry a regrid writes, from the extent of all spheres: the flat axes' lo / cell / inv_cell (the plan's where
// there is no candidate) and the far test's box clo / chi (zero where nothing is registered, as the builder leaves it)
R1F_HD void r1gf_geometry(const R1GridPlan &P, const R1GridExtent &e, float lo[3], float cell[3], float inv_cell[3], float clo[3], float chi[3])
{
    for (int a = 0; a < 3; ++a)
    {
        lo[a] = P.lo[a], cell[a] = P.cell[a], inv_cell[a] = P.inv_cell[a];
        if (P.flat[a] && e.clo[a] <= e.chi[a])
            r1gf_stretch(e.clo[a], e.chi[a], e.rho_max, P.M, lo[a], cell[a], inv_cell[a]);
        const bool any = e.rlo[a] <= e.rhi[a];
        clo[a] = any ? (float)e.rlo[a] : 0.0f, chi[a] = any ? (float)e.rhi[a] : 0.0f;
    }
}

// What the regrid kernels read and write (r1_regrid.hip), device memory; by value in their arguments.  Laid out at a scene's first regrid.
struct R1GridArgs; // r1_device.h
struct R1RegridArgs
{
    R1GridPlan plan;
    const float *exact;        // [active][4] {cx cy cz radius_sq}
    const double *radii;       // [active][2] {bound radius, test radius}
    uint32_t na;               // active spheres, > 0
    uint32_t cap;              // the id table's capacity (r1gf_capacity)
    uint32_t small;            // 1: the 16-bit table is written too
    uint32_t tab16_halves;     // entries of tab16: n_start + cap, rounded up to whole 16-byte rows
    R1GridArgs *g16, *g32;     // the two R1GridArgs the kernels read (r1_context grid_dev, grid_dev32)
    uint32_t *tab32;           // [n_start + cap] the starts, then the ids
    uint16_t *tab16;           // [tab16_halves]
    uint32_t *outliers;        // [na]
    // scratch
    uint32_t *span, *oflag;    // [na + 1] each: a sphere's cells / whether it is an outlier, then their prefix sums in place (entry na: the total)
    double *part;              // [blocks of na + 1][R1GF_EXTENT_WORDS] the workgroups' extents
    uint32_t *key[2], *val[2]; // [cap] each: the (cell, id) pairs, two buffers taken in turn by the sort's passes
    uint32_t *hist;            // [256][blocks of cap]
    uint32_t *sums;            // the prefix sums' block sums
    uint32_t *stat;            // R1GF_STAT_*
};
#define R1GF_STAT_PAIRS 0    // the pairs the tables hold: the total, or 0 on overflow
#define R1GF_STAT_OVERFLOW 1 // 1: the total exceeds the capacity
#define R1GF_STAT_TOTAL 2
#define R1GF_STAT_WORDS 4

#endif
