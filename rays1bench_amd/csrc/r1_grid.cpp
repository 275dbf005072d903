// r1_grid.cpp — host-side builder of the uniform grid (R1_VARIANT_GRID, SURVEY.md §8f-1: "a uniform grid/BVH over the 100 k-sphere
// field, kept optional so brute-force parity mode remains").  Like the box tree (r1_bvh.cpp) the grid only decides WHICH spheres are
// presented to the reference's per-sphere test (exact_offer in r1_hit_sweep.hpp = rayweek1.cpp:192-202, :294-313); it is conservative with
// respect to that fp32 test, not to geometry, so pixels and ray counts stay bit-identical to the exhaustive sweep.
//
// Structure.  Outliers — spheres more than R1_GRID_OUTLIER_RATIO (4) x the median radius, or whose padded ball would register in more
// than R1_GRID_SPAN_MAX cells (the reference's ground and its three r = 2 balls) — are tested by every ray with exact_offer before the walk,
// as the tree's root leaf is.  The other spheres are registered in a uniform grid over their padded balls: cells per axis from the
// spheres' density (about one sphere per cell) or, where the centres sit on a lattice along the axis, the lattice's pitch with the
// centres in the middle of the cells; an axis along which the centres spread less than the median padded radius gets ONE cell, so the
// reference's flat lattices are walked in 2-D without a special case.  Storage is CSR: cell start offsets + one array of active sphere
// indices (16-bit entries for the small-scene kernel, which keeps both in LDS; 32-bit otherwise).
//
// Exactness.  Let u = 2^-24 and v = c - o.  r1_bvh.cpp shows that when the reference flags a sphere and offers it a t, the point
// o + t d (real arithmetic) lies within  rho(|v|) = r_eff + E1 / (2 r_eff) + 5 u |v|  of the centre, E1 <= 23 u |v|^2 + 2 u r^2,
// r_eff = max(r, r_floor) with r_floor = 1e-4 (1 + |c|_1) for degenerate radii.  The bound grows with |v| = |c - o|, which does not
// depend on t: so instead of a t up to which the walk is safe, the grid bounds the ORIGIN.  Choose V; register sphere i in every cell its
// ball of radius
//      rho_i = r_eff,i + (23 u V^2 + 2 u r_i^2) / (2 r_eff,i) + 5 u V + delta,      delta = 32 u (2 M + V)  (the walk's rounding, below)
// overlaps (an exact ball-box test in double; M bounds every coordinate of the grid's box).  A ray whose origin lies within V of every
// registered centre — r1g_far: the farthest point of the centres' box, computed from below against V^2 (1 - 2^-20) rounded down, 6u
// relative error covered — then has |v| <= V for every registered sphere, and every offer t' of such a sphere puts o + t' d within
// rho_i - delta of its centre.  Lanes whose origin is farther take the FALLBACK: the tree walk from scratch (exact for any origin).
// (With the tree's per-ray pad A |o - C|^2 + K one would still have to bound the walk's t by a t_safe = V - r_max - P; bounding |v|
// through the origin is tighter and costs one test per ray.  info.v_safe is that V.)
//
// The walk (r1_grid_dda.h).  Boundary k of axis a is X = lo_a + k cell_a; its t is computed as fmaf(k, cell_a, lo_a - o_a) x (1 / d_a):
// three correctly rounded operations, so the real point at the computed t is within e = 6 u (|X| + |o_a|) <= 6 u (2 M + V) of the plane
// along axis a (|o_a| <= M + V for a ray that does not take the fallback), whatever d_a is; the first cell, picked by
// floorf((p - lo) / cell) at the entry point p, is off by less than that too.  So for every t in a walked cell's computed range
// [t at which it was entered, smallest next-boundary t] the real point o + t d is within e of that cell on every axis, i.e. within
// sqrt(3) e < delta / 2 of its box.  The ranges of the walked cells join up from t_start = max(0, entry into the box) — an offer
// below it (or past the exit) would put o + t' d outside the box shrunk by delta, which contains every registration ball shrunk by delta.
// Hence a sphere that offers t' within the walked range lies in a walked cell's list: the walk presents every sphere whose offer
// is <= the t at which it stops.  It stops when the next cell is entered at t > best (STRICTLY: a sphere that ties best is entered at
// t <= best and the lowest-index rule needs it) or when the ray leaves the box; the rounding margin is in delta, not in the compare.
// Every constant is derived in double and rounded up.  Duplicate registrations are harmless: a sphere presented twice makes the same
// offer and loses the index tie to itself.
#include <hip/hip_runtime.h>

#include "r1_device.h"
#include "r1_grid_dda.h"
#include "../../include/rays1.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "r1_grid.h"
#include "r1_grid_fill.h"
#include "r1_internal.h"

int r1_active_spheres(const r1_scene *s, std::vector<uint32_t> &active_to_scene); // r1_bvh.cpp
double r1_bound_radius(float radius_sq, float inv_radius);

namespace
{

float round_down_f(double v)
{
    float f = (float)v;
    if ((double)f > v)
        f = nextafterf(f, -INFINITY);
    return f;
}
float round_up_f(double v)
{
    float f = (float)v;
    if ((double)f < v)
        f = nextafterf(f, INFINITY);
    return f;
}

void empty_grid(R1Grid &g)
{
    for (int a = 0; a < 3; ++a)
        g.geom.lo[a] = 0.0f, g.geom.cell[a] = 1.0f, g.geom.inv_cell[a] = 1.0f, g.geom.n[a] = 1, g.geom.clo[a] = g.geom.chi[a] = 0.0f;
    g.geom.v2 = INFINITY; // nothing registered: every origin is safe
    g.start.assign(2, 0u);
    g.ids.clear();
}

} // namespace

// Builds the grid over the `na` active spheres (fp32 arrays in active order, rbound = r1_bound_radius).
void r1_build_grid(uint32_t na, const float *cx, const float *cy, const float *cz, const float *rsq, const double *rbound, R1Grid &g)
{
    const auto t_begin = std::chrono::steady_clock::now();
    const double u = ldexp(1.0, -24);
    g = R1Grid();
    empty_grid(g);
    static const double ratio_env = r1_knob_f("R1_GRID_OUTLIER_RATIO", 4.0);
    static const double vscale_env = r1_knob_f("R1_GRID_V_SCALE", 1.0);
    static const double vmin_env = r1_knob_f("R1_GRID_V_MIN", 16.0);
    static const double cell_env = r1_knob_f("R1_GRID_CELL_SCALE", 1.0);
    static const int span_env = (int)r1_knob("R1_GRID_SPAN_MAX", R1_GRID_SPAN_MAX);

    std::vector<uint8_t> out(na, 0);
    std::vector<double> rtest(na), reff(na);
    for (uint32_t i = 0; i < na; ++i)
    {
        const double r = rbound[i];
        rtest[i] = rsq[i] > 0 ? std::min(r, std::sqrt((double)rsq[i])) : 0.0;
        const double r_floor = 1e-4 * (1.0 + std::fabs((double)cx[i]) + std::fabs((double)cy[i]) + std::fabs((double)cz[i]));
        reff[i] = std::max(rtest[i], r_floor);
    }
    if (na)
    {
        std::vector<double> rs(rbound, rbound + na);
        std::nth_element(rs.begin(), rs.begin() + na / 2, rs.end());
        const double big = g.big = ratio_env * rs[na / 2];
        for (uint32_t i = 0; i < na; ++i)
            out[i] = rbound[i] > big ? 1 : 0;
    }
    auto finish = [&]() {
        g.outliers.clear();
        for (uint32_t i = 0; i < na; ++i)
            if (out[i])
                g.outliers.push_back(i);
        g.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    };
    std::vector<uint32_t> reg;
    for (uint32_t i = 0; i < na; ++i)
        if (!out[i])
            reg.push_back(i);
    if (reg.empty())
    {
        finish();
        return;
    }

    // the centres' box and V
    double clo[3] = {1e300, 1e300, 1e300}, chi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t i : reg)
    {
        const double c[3] = {cx[i], cy[i], cz[i]};
        for (int a = 0; a < 3; ++a)
            clo[a] = std::min(clo[a], c[a]), chi[a] = std::max(chi[a], c[a]);
    }
    double diag2 = 0, mc = 0;
    for (int a = 0; a < 3; ++a)
        diag2 += (chi[a] - clo[a]) * (chi[a] - clo[a]), mc = std::max(mc, std::max(std::fabs(clo[a]), std::fabs(chi[a])));
    const double V = std::max(vmin_env, vscale_env * std::sqrt(diag2));
    // registration radii: first without the walk's margin, which needs M (a bound on the box's coordinates), then with it
    std::vector<double> rho(na, 0.0);
    double rho_max = 0;
    for (uint32_t i : reg)
    {
        rho[i] = reff[i] + (23.0 * u * V * V + 2.0 * u * rtest[i] * rtest[i]) / (2.0 * reff[i]) + 5.0 * u * V;
        rho_max = std::max(rho_max, rho[i]);
    }
    // The walk's margin delta needs M, a bound on the coordinates of the cells' box, which follows the radii: lay the cells out with an
    // estimate of M, measure the box, and repeat with the measured bound until it holds (the box grows by ~delta: twice at most)
    std::vector<double> rho0(rho);
    double M = mc + 2.0 * rho_max + 1.0, delta = 0;
    for (int pass = 0;; ++pass)
    {
        delta = 32.0 * u * (2.0 * M + V) + ldexp(1.0, -100);
        rho_max = 0;
        std::vector<double> rr;
        for (uint32_t i : reg)
        {
            rho[i] = (rho0[i] + delta) * (1.0 + ldexp(1.0, -40));
            rho_max = std::max(rho_max, rho[i]);
            rr.push_back(rho[i]);
        }
        std::nth_element(rr.begin(), rr.begin() + rr.size() / 2, rr.end());
        const double rho_med = rr[rr.size() / 2];
        // cells per axis
        const double nreg = (double)reg.size();
        bool flat[3];
        int k = 0;
        double vol = 1;
        for (int a = 0; a < 3; ++a)
        {
            flat[a] = chi[a] - clo[a] <= rho_med;
            if (!flat[a])
                ++k, vol *= chi[a] - clo[a] + 2.0 * rho_max;
        }
        const double s_vol = k ? std::pow(vol / nreg, 1.0 / k) * cell_env : 1.0;
        double s[3] = {1, 1, 1};
        for (int a = 0; a < 3; ++a)
        {
            if (flat[a])
                continue;
            std::vector<float> v;
            for (uint32_t i : reg)
                v.push_back(a == 0 ? cx[i] : (a == 1 ? cy[i] : cz[i]));
            std::sort(v.begin(), v.end());
            const size_t m = (size_t)(std::unique(v.begin(), v.end()) - v.begin());
            const double pitch = m >= 2 ? (chi[a] - clo[a]) / (double)(m - 1) : 0.0;
            s[a] = (pitch >= 0.5 * s_vol && pitch <= 2.0 * s_vol) ? pitch : s_vol; // a lattice along this axis: its pitch
        }
        for (int grow = 0;; ++grow)
        {
            double cells = 1;
            for (int a = 0; a < 3; ++a)
            {
                double lo, cell;
                int n;
                if (flat[a])
                    lo = clo[a] - rho_max, cell = chi[a] - clo[a] + 2.0 * rho_max, n = 1;
                else
                {
                    const double h = std::max(rho_max, 0.5 * s[a]); // (a lattice: centres in the middle of their cells)
                    lo = clo[a] - h, cell = s[a];
                    n = (int)std::max(1.0, std::ceil((chi[a] - clo[a] + 2.0 * h) / cell - 1e-9));
                    n = std::min(n, R1_GRID_AXIS_MAX);
                }
                g.geom.lo[a] = round_down_f(lo);
                g.geom.cell[a] = round_up_f(flat[a] ? (chi[a] + rho_max - (double)g.geom.lo[a]) * (1.0 + 1e-12) : cell); // (a flat axis: the one cell covers all)
                // the box must hold every registration ball: more cells (or, at the cap, larger ones)
                while ((double)g.geom.lo[a] + (double)n * (double)g.geom.cell[a] < chi[a] + rho_max)
                {
                    if (n < R1_GRID_AXIS_MAX)
                        ++n;
                    else
                        g.geom.cell[a] = round_up_f((chi[a] + rho_max - (double)g.geom.lo[a]) / n * (1.0 + 1e-6));
                }
                g.geom.n[a] = n;
                g.geom.inv_cell[a] = (float)(1.0 / (double)g.geom.cell[a]);
                cells *= n;
            }
            if (cells <= 8.0 * nreg + 4096.0 || grow > 60)
                break;
            for (int a = 0; a < 3; ++a)
                s[a] *= 1.25;
        }
        double bound_m = 0;
        for (int a = 0; a < 3; ++a)
            bound_m = std::max(bound_m, std::max(std::fabs((double)g.geom.lo[a]), std::fabs((double)g.geom.lo[a] + g.geom.n[a] * (double)g.geom.cell[a])));
        g.M = M, g.delta = delta; // (the plan of a regrid: this pass's)
        for (int a = 0; a < 3; ++a)
            g.flat[a] = flat[a];
        if (bound_m <= M || pass >= 4)
            break;
        M = bound_m * (1.0 + 1e-3) + 1.0;
    }
    const int nx = g.geom.n[0], ny = g.geom.n[1], nz = g.geom.n[2];
    const size_t ncells = (size_t)nx * ny * nz;

    // registration: every cell the ball (c_i, rho_i) overlaps (exact ball-box distance in double)
    auto cells_of = [&](uint32_t i, auto &&fn) {
        const double c[3] = {cx[i], cy[i], cz[i]};
        int jlo[3], jhi[3];
        for (int a = 0; a < 3; ++a)
        {
            const double lo = g.geom.lo[a], cell = g.geom.cell[a];
            jlo[a] = (int)std::floor((c[a] - rho[i] - lo) / cell - 1e-9);
            jhi[a] = (int)std::floor((c[a] + rho[i] - lo) / cell + 1e-9);
            jlo[a] = std::max(jlo[a], 0), jhi[a] = std::min(jhi[a], g.geom.n[a] - 1);
        }
        for (int jz = jlo[2]; jz <= jhi[2]; ++jz)
            for (int jy = jlo[1]; jy <= jhi[1]; ++jy)
                for (int jx = jlo[0]; jx <= jhi[0]; ++jx)
                {
                    const int j[3] = {jx, jy, jz};
                    double d2 = 0;
                    for (int a = 0; a < 3; ++a)
                    {
                        const double b0 = g.geom.lo[a] + j[a] * (double)g.geom.cell[a], b1 = g.geom.lo[a] + (j[a] + 1) * (double)g.geom.cell[a];
                        const double q = c[a] < b0 ? b0 - c[a] : (c[a] > b1 ? c[a] - b1 : 0.0);
                        d2 += q * q;
                    }
                    if (d2 <= rho[i] * rho[i] * (1.0 + 1e-12))
                        fn((size_t)((jz * ny + jy) * nx + jx));
                }
    };
    std::vector<uint32_t> cnt(ncells + 1, 0);
    for (uint32_t i : reg)
    {
        uint32_t span = 0;
        cells_of(i, [&](size_t) { ++span; });
        if ((int)span > span_env)
            out[i] = 1; // registers in too many cells: an outlier after all
        else
            cells_of(i, [&](size_t cidx) { ++cnt[cidx]; });
    }
    g.start.assign(ncells + 1, 0u);
    for (size_t q = 0; q < ncells; ++q)
        g.start[q + 1] = g.start[q] + cnt[q];
    g.ids.assign(g.start[ncells], 0u);
    std::vector<uint32_t> fill(g.start.begin(), g.start.end() - 1);
    g.max_occupancy = 0;
    for (uint32_t i : reg) // (ascending active index within every cell)
        if (!out[i])
            cells_of(i, [&](size_t cidx) { g.ids[fill[cidx]++] = i; });
    for (size_t q = 0; q < ncells; ++q)
        g.max_occupancy = std::max(g.max_occupancy, cnt[q]);
    // the far test's box: the REGISTERED centres (fp32 values: exact)
    double glo[3] = {1e300, 1e300, 1e300}, ghi[3] = {-1e300, -1e300, -1e300};
    bool any = false;
    g.pad = 0;
    for (uint32_t i : reg)
        if (!out[i])
        {
            any = true;
            const double c[3] = {cx[i], cy[i], cz[i]};
            for (int a = 0; a < 3; ++a)
                glo[a] = std::min(glo[a], c[a]), ghi[a] = std::max(ghi[a], c[a]);
            g.pad = std::max(g.pad, rho[i] - rbound[i]);
        }
    for (int a = 0; a < 3; ++a)
        g.geom.clo[a] = any ? (float)glo[a] : 0.0f, g.geom.chi[a] = any ? (float)ghi[a] : 0.0f;
    g.geom.v2 = any ? round_down_f(V * V * (1.0 - ldexp(1.0, -20))) : INFINITY;
    g.v_safe = V;
    finish();
}

// The active spheres of a caller's scene as fp32 arrays (the same filter and order as r1_set_scene)
static int grid_from_scene(const r1_scene *s, R1Grid &g, std::vector<uint32_t> &scene_index, std::vector<float> &ex)
{
    if (r1_active_spheres(s, scene_index) != R1_OK)
        return R1_EINVAL;
    const uint32_t na = (uint32_t)scene_index.size();
    std::vector<float> x(na + 1), y(na + 1), z(na + 1), r(na + 1);
    std::vector<double> rb(na + 1);
    ex.assign(4 * (size_t)na + 4, 0.0f);
    for (uint32_t a = 0; a < na; ++a)
    {
        const uint32_t i = scene_index[a];
        x[a] = s->center_x[i], y[a] = s->center_y[i], z[a] = s->center_z[i], r[a] = s->radius_sq[i];
        rb[a] = r1_bound_radius(s->radius_sq[i], s->inv_radius[i]);
        ex[4 * a] = x[a], ex[4 * a + 1] = y[a], ex[4 * a + 2] = z[a], ex[4 * a + 3] = r[a];
    }
    r1_build_grid(na, x.data(), y.data(), z.data(), r.data(), rb.data(), g);
    return R1_OK;
}

int r1_grid_from_scene(const r1_scene *s, R1Grid &g)
{
    std::vector<uint32_t> scene_index;
    std::vector<float> ex;
    return grid_from_scene(s, g, scene_index, ex);
}

// info and the optional outputs of r1_grid_describe, r1_grid_regrid_describe and r1_grid_download, from a grid in active indices
int r1_grid_report(const R1Grid &g, const std::vector<uint32_t> &scene_index, bool overflow, r1_grid_info *info, uint32_t *start_out, size_t start_cap,
                   uint32_t *ids_out, size_t ids_cap, uint32_t *outliers_out, size_t outliers_cap)
{
    memset(info, 0, sizeof(*info));
    for (int a = 0; a < 3; ++a)
    {
        info->lo[a] = g.geom.lo[a], info->cell[a] = g.geom.cell[a], info->cells[a] = g.geom.n[a];
        info->hi[a] = (float)((double)g.geom.lo[a] + g.geom.n[a] * (double)g.geom.cell[a]);
        info->centre_lo[a] = g.geom.clo[a], info->centre_hi[a] = g.geom.chi[a];
    }
    info->pad = (float)g.pad;
    info->v_safe = (float)g.v_safe;
    info->spheres = (int32_t)scene_index.size();
    info->outliers = (int32_t)g.outliers.size();
    info->registrations = overflow ? -1 : (int32_t)g.ids.size();
    info->max_occupancy = (int32_t)g.max_occupancy;
    info->build_ms = (float)g.build_ms;
    if (start_out)
    {
        if (start_cap < g.start.size())
            return R1_ELIMIT;
        memcpy(start_out, g.start.data(), g.start.size() * 4);
    }
    if (ids_out)
    {
        if (ids_cap < g.ids.size())
            return R1_ELIMIT;
        for (size_t q = 0; q < g.ids.size(); ++q)
            ids_out[q] = scene_index[g.ids[q]];
    }
    if (outliers_out)
    {
        if (outliers_cap < g.outliers.size())
            return R1_ELIMIT;
        for (size_t q = 0; q < g.outliers.size(); ++q)
            outliers_out[q] = scene_index[g.outliers[q]];
    }
    return R1_OK;
}

extern "C" int r1_grid_describe(const r1_scene *s, r1_grid_info *info, uint32_t *start_out, size_t start_cap, uint32_t *ids_out, size_t ids_cap,
                                uint32_t *outliers_out, size_t outliers_cap)
{
    if (!s || !info || !s->center_x || !s->center_y || !s->center_z || !s->radius_sq || !s->inv_radius)
        return R1_EINVAL;
    R1Grid g;
    std::vector<uint32_t> scene_index;
    std::vector<float> ex;
    if (grid_from_scene(s, g, scene_index, ex) != R1_OK)
        return R1_EINVAL;
    return r1_grid_report(g, scene_index, false, info, start_out, start_cap, ids_out, ids_cap, outliers_out, outliers_cap);
}

// exact_offer (r1_hit_sweep.hpp) on the host: the same operations, the same order
static float host_offer(const float *e, const float o[3], const float d[3])
{
    const float cox = e[0] - o[0], coy = e[1] - o[1], coz = e[2] - o[2];
    const float nb = fmaf(coz, d[2], fmaf(coy, d[1], cox * d[0]));
    const float c = fmaf(coz, coz, fmaf(coy, coy, cox * cox)) - e[3];
    const float discr = nb * nb - c;
    uint32_t bits;
    memcpy(&bits, &discr, 4);
    float offer = FLT_MAX;
    if (!(bits >> 31))
    {
        const float root = sqrtf(discr);
        const float t1 = nb - root;
        const float t = (t1 > 0.001f) ? t1 : nb + root;
        if (t > 0.001f && t < FLT_MAX)
            offer = t;
    }
    return offer;
}

// One ray through given tables (active indices; ex: the spheres' exact rows), as the kernel walks them
static void visit_tables(const R1Grid &g, const std::vector<uint32_t> &scene_index, const std::vector<float> &ex, const float o[3], const float d[3],
                         uint32_t *presented, size_t cap, size_t *n_presented, int32_t *hit_index, float *hit_t, int32_t *fallback)
{
    size_t np = 0;
    float best = FLT_MAX;
    uint32_t best_id = 0xFFFFFFFFu;
    auto present = [&](uint32_t a) {
        if (presented && np < cap)
            presented[np] = scene_index[a];
        ++np;
        const float t = host_offer(&ex[4 * (size_t)a], o, d);
        if (t < FLT_MAX && (t < best || (t == best && a < best_id)))
            best = t, best_id = a;
    };
    for (uint32_t a : g.outliers) // 1. the outliers
        present(a);
    *fallback = r1g_far(g.geom, o[0], o[1], o[2]) ? 1 : 0;
    if (*fallback)
    {
        // the kernel's fallback is the tree walk from scratch, exact for any origin: its result is the exhaustive minimum
        for (uint32_t a = 0; a < (uint32_t)scene_index.size(); ++a)
        {
            const float t = host_offer(&ex[4 * (size_t)a], o, d);
            if (t < FLT_MAX && (t < best || (t == best && a < best_id)))
                best = t, best_id = a;
        }
    }
    else
    {
        R1GridRay r;
        if (r1g_setup(g.geom, o[0], o[1], o[2], d[0], d[1], d[2], best, r)) // 2. the grid's box
            do                                                             // 3.-5. the cells in order of entry t
            {
                const uint32_t cidx = r1g_cell(g.geom, r);
                for (uint32_t q = g.start[cidx]; q < g.start[cidx + 1]; ++q)
                    present(g.ids[q]);
            } while (r1g_step(g.geom, r, best));
    }
    *n_presented = np;
    *hit_index = best_id == 0xFFFFFFFFu ? -1 : (int32_t)scene_index[best_id];
    *hit_t = best;
}

extern "C" int r1_grid_visit(const r1_scene *s, const float o[3], const float d[3], uint32_t *presented, size_t cap, size_t *n_presented,
                             int32_t *hit_index, float *hit_t, int32_t *fallback)
{
    if (!s || !o || !d || !n_presented || !hit_index || !hit_t || !fallback || !s->center_x || !s->center_y || !s->center_z ||
        !s->radius_sq || !s->inv_radius)
        return R1_EINVAL;
    R1Grid g;
    std::vector<uint32_t> scene_index;
    std::vector<float> ex;
    if (grid_from_scene(s, g, scene_index, ex) != R1_OK)
        return R1_EINVAL;
    visit_tables(g, scene_index, ex, o, d, presented, cap, n_presented, hit_index, hit_t, fallback);
    return R1_OK;
}

// ---- regrid: the moved spheres re-registered against the build's plan -----------------------------------------

static_assert(R1_GRID_SPAN_LIMIT == R1_GRID_SPAN_MAX, "r1_grid_fill.h counts cells up to the builder's limit");

void r1_grid_plan(const R1Grid &g, R1GridPlan &p)
{
    memset(&p, 0, sizeof(p));
    for (int a = 0; a < 3; ++a)
        p.lo[a] = g.geom.lo[a], p.cell[a] = g.geom.cell[a], p.inv_cell[a] = g.geom.inv_cell[a], p.n[a] = g.geom.n[a], p.flat[a] = g.flat[a] ? 1 : 0;
    p.V = g.v_safe, p.delta = g.delta, p.big = g.big, p.M = g.M;
    // (a build that registered nothing stores v2 = inf: the plan keeps the V it chose, as r1_build_grid rounds it)
    p.v2 = round_down_f(g.v_safe * g.v_safe * (1.0 - ldexp(1.0, -20)));
    p.n_start = (uint32_t)g.start.size();
    p.regs = (uint32_t)g.ids.size();
}

// the plan of the grid of `built`, for tests: doubles4 = {V, delta, big, M}, flat3 = which axes have one cell
extern "C" int r1_grid_plan_describe(const r1_scene *built, double *doubles4, int32_t *flat3)
{
    if (!built || !doubles4 || !flat3 || !built->center_x || !built->center_y || !built->center_z || !built->radius_sq || !built->inv_radius)
        return R1_EINVAL;
    R1Grid g;
    if (r1_grid_from_scene(built, g) != R1_OK)
        return R1_EINVAL;
    R1GridPlan p;
    r1_grid_plan(g, p);
    doubles4[0] = p.V, doubles4[1] = p.delta, doubles4[2] = p.big, doubles4[3] = p.M;
    for (int a = 0; a < 3; ++a)
        flat3[a] = p.flat[a];
    return R1_OK;
}

bool r1_grid_regrid_host(const R1GridPlan &P, uint32_t na, const float *exact, const double *radii, R1Grid &out)
{
    out = R1Grid();
    // 1. classify: class, span and the extents
    std::vector<uint32_t> span(na, 0u);
    std::vector<uint8_t> outl(na, 0);
    std::vector<double> rho(na, 0.0);
    R1GridExtent ext;
    ext.clear();
    size_t total = 0;
    for (uint32_t i = 0; i < na; ++i)
    {
        const float *e = exact + 4 * (size_t)i;
        bool cand;
        const uint32_t k = r1gf_classify(P, e[0], e[1], e[2], radii[2 * (size_t)i], radii[2 * (size_t)i + 1], rho[i], span[i], cand);
        outl[i] = k == R1GF_OUTLIER;
        ext.add(e[0], e[1], e[2], rho[i], cand, k == R1GF_CANDIDATE);
        total += span[i];
    }
    // 2. the geometry
    for (int a = 0; a < 3; ++a)
        out.geom.n[a] = P.n[a];
    r1gf_geometry(P, ext, out.geom.lo, out.geom.cell, out.geom.inv_cell, out.geom.clo, out.geom.chi);
    // 3. the outlier list, the total against the capacity
    for (uint32_t i = 0; i < na; ++i)
        if (outl[i])
            out.outliers.push_back(i);
    const bool overflow = total > r1gf_capacity(P.regs);
    out.geom.v2 = overflow ? -1.0f : (total ? P.v2 : INFINITY);
    out.v_safe = P.V, out.M = P.M, out.delta = P.delta, out.big = P.big;
    for (int a = 0; a < 3; ++a)
        out.flat[a] = P.flat[a] != 0;
    out.start.assign(P.n_start, 0u);
    if (overflow)
        return true;
    // 4. + 5. the (cell, id) pairs in sphere order, sorted by cell: ascending ids within a cell
    std::vector<std::pair<uint32_t, uint32_t>> pairs(total);
    size_t at = 0;
    uint32_t keys[R1_GRID_SPAN_LIMIT + 1], vals[R1_GRID_SPAN_LIMIT + 1];
    for (uint32_t i = 0; i < na; ++i)
        if (span[i])
        {
            const float *e = exact + 4 * (size_t)i;
            const uint32_t n = r1gf_cells(P, e[0], e[1], e[2], rho[i], keys, vals, i);
            for (uint32_t k = 0; k < n; ++k)
                pairs[at++] = {keys[k], vals[k]};
            out.pad = std::max(out.pad, rho[i] - radii[2 * (size_t)i]);
        }
    std::sort(pairs.begin(), pairs.end());
    // 6. the starts
    out.ids.resize(total);
    for (size_t q = 0; q < total; ++q)
        out.ids[q] = pairs[q].second, ++out.start[pairs[q].first + 1];
    for (size_t q = 1; q < out.start.size(); ++q)
    {
        out.max_occupancy = std::max(out.max_occupancy, out.start[q]);
        out.start[q] += out.start[q - 1];
    }
    return false;
}

// the plan of `built` and the moved scene's rows in active order: exact [na][4], radii [na][2] as the device's set kernel writes them
static int regrid_inputs(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq, const float *inv_radius,
                         R1GridPlan &plan, std::vector<uint32_t> &scene_index, std::vector<float> &ex, std::vector<double> &radii)
{
    if (!built || !x || !y || !z || (!radius_sq) != (!inv_radius) || !built->center_x || !built->center_y || !built->center_z || !built->radius_sq ||
        !built->inv_radius)
        return R1_EINVAL;
    R1Grid g;
    if (grid_from_scene(built, g, scene_index, ex) != R1_OK)
        return R1_EINVAL;
    r1_grid_plan(g, plan);
    const uint32_t na = (uint32_t)scene_index.size();
    radii.assign(2 * (size_t)na + 2, 0.0);
    for (uint32_t a = 0; a < na; ++a)
    {
        const uint32_t i = scene_index[a];
        float rsq, inv;
        r1f_radius_rows(radius_sq ? radius_sq[i] : built->radius_sq[i], inv_radius ? inv_radius[i] : built->inv_radius[i], rsq, inv, &radii[2 * (size_t)a]);
        ex[4 * (size_t)a] = x[i], ex[4 * (size_t)a + 1] = y[i], ex[4 * (size_t)a + 2] = z[i], ex[4 * (size_t)a + 3] = rsq;
    }
    return R1_OK;
}

extern "C" int r1_grid_regrid_describe(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                                       const float *inv_radius, r1_grid_info *info, uint32_t *start_out, size_t start_cap, uint32_t *ids_out,
                                       size_t ids_cap, uint32_t *outliers_out, size_t outliers_cap)
{
    if (!info)
        return R1_EINVAL;
    const auto t_begin = std::chrono::steady_clock::now();
    R1GridPlan plan;
    std::vector<uint32_t> scene_index;
    std::vector<float> ex;
    std::vector<double> radii;
    int rc = regrid_inputs(built, x, y, z, radius_sq, inv_radius, plan, scene_index, ex, radii);
    if (rc)
        return rc;
    R1Grid g;
    const bool overflow = r1_grid_regrid_host(plan, (uint32_t)scene_index.size(), ex.data(), radii.data(), g);
    g.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return r1_grid_report(g, scene_index, overflow, info, start_out, start_cap, ids_out, ids_cap, outliers_out, outliers_cap);
}

extern "C" int r1_grid_regrid_visit(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                                    const float *inv_radius, const float o[3], const float d[3], uint32_t *presented, size_t cap,
                                    size_t *n_presented, int32_t *hit_index, float *hit_t, int32_t *fallback)
{
    if (!o || !d || !n_presented || !hit_index || !hit_t || !fallback)
        return R1_EINVAL;
    R1GridPlan plan;
    std::vector<uint32_t> scene_index;
    std::vector<float> ex;
    std::vector<double> radii;
    int rc = regrid_inputs(built, x, y, z, radius_sq, inv_radius, plan, scene_index, ex, radii);
    if (rc)
        return rc;
    R1Grid g;
    r1_grid_regrid_host(plan, (uint32_t)scene_index.size(), ex.data(), radii.data(), g);
    visit_tables(g, scene_index, ex, o, d, presented, cap, n_presented, hit_index, hit_t, fallback);
    return R1_OK;
}
