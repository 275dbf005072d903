// r1_grid_dda.h — the uniform grid's cell walk (R1_VARIANT_GRID), shared by the trace kernel (r1_hit_grid.hpp grid_trace) and the
// host's r1_grid_visit (r1_grid.cpp), so that the CPU tests check the kernel's own arithmetic.  Why the walk is exact: r1_grid.cpp.
//
// Only correctly rounded operations: + - x, fmaf, floorf and IEEE '/' for the once-per-ray reciprocals (the build passes
// -fhip-fp32-correctly-rounded-divide-sqrt and -ffp-contract=off; no v_rcp_f32, no fast math here).  Three scalar lanes (x, y, z)
// instead of arrays: an axis chosen per lane would index an array dynamically, which puts it in scratch memory on the device.
#ifndef R1_GRID_DDA_H
#define R1_GRID_DDA_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#define R1_GRID_HD __host__ __device__ __forceinline__

// What the walk needs of the grid (by value in the kernel arguments: R1TraceArgs::grid)
struct R1GridGeom
{
    float lo[3];       // the grid's box: cell j of axis a spans [lo + j cell, lo + (j + 1) cell] (real numbers)
    float cell[3];     // cell size per axis
    float inv_cell[3]; // 1 / cell (only picks the first cell: any rounding is covered, r1_grid.cpp)
    int32_t n[3];      // cells per axis (a flat axis has one)
    float clo[3];      // box of the registered spheres' centres: an origin farther than sqrt(v2) from any point of it
    float chi[3];      //   takes the fallback (the tree walk)
    float v2;          // V^2 rounded down: the grid is exact for every ray whose origin is within V of every registered centre
};

// One lane's walk
struct R1GridRay
{
    float bx, by, bz;    // lo - o
    float ix, iy, iz;    // 1 / d per axis (0 for an axis the ray does not move along)
    int32_t jx, jy, jz;  // current cell
    int32_t sx, sy, sz;  // step per axis: +1 / -1, 0 for an axis the ray does not move along
    float tx, ty, tz;    // t at which the ray leaves the current cell through each axis' next boundary (+inf: never)
};

// origin too far from the registered centres for the registration pad (r1_grid.cpp): the lane takes the fallback.  Computed from
// below (relative error <= 6u) against V^2 (1 - 2^-20) rounded down; a non-finite origin always takes it
template <class GG> // (R1GridGeom, or on the device the same read in place from the constant address space)
R1_GRID_HD bool r1g_far(GG &g, const float ox, const float oy, const float oz)
{
    const float mx = fmaxf(fabsf(ox - g.clo[0]), fabsf(ox - g.chi[0]));
    const float my = fmaxf(fabsf(oy - g.clo[1]), fabsf(oy - g.chi[1]));
    const float mz = fmaxf(fabsf(oz - g.clo[2]), fabsf(oz - g.chi[2]));
    const float d2 = fmaf(mz, mz, fmaf(my, my, mx * mx));
    return !(d2 <= g.v2); // (NaN: far)
}

// t of boundary k of one axis: (lo + k cell - o) / d as fmaf(k, cell, lo - o) x (1 / d)
R1_GRID_HD float r1g_bound(const int32_t k, const float cell, const float b, const float inv) { return fmaf((float)k, cell, b) * inv; }

// per axis: the slab [lo, lo + n cell] as t range, the first cell's index, the step and the next boundary's t
R1_GRID_HD void r1g_axis(const float lo, const float cell, const float inv_cell, const int32_t n, const float o, const float dd, float &b,
                         float &iv, int32_t &s, float &t_in, float &t_out, bool &inside)
{
    b = lo - o;
    iv = 1.0f / dd;
    s = dd > 0.0f ? 1 : (dd < 0.0f ? -1 : 0);
    if (!(fabsf(iv) < INFINITY)) // does not move along this axis (|d| below 2^-128): no constraint on t, the origin's slab decides
    {
        iv = 0.0f, s = 0;
        t_in = -INFINITY, t_out = INFINITY;
        inside = o >= lo && o <= fmaf((float)n, cell, lo);
        return;
    }
    const float t0 = b * iv, t1 = r1g_bound(n, cell, b, iv);
    t_in = fminf(t0, t1), t_out = fmaxf(t0, t1);
    inside = true;
}

R1_GRID_HD int32_t r1g_first(const float p, const float lo, const float inv_cell, const int32_t n)
{
    const float q = floorf((p - lo) * inv_cell);
    const int32_t j = q < 0.0f ? 0 : (q >= (float)n ? n - 1 : (int32_t)q);
    return j;
}

// Setup: false if the ray misses the grid's box or reaches it only beyond `best` (no registered sphere can then offer a hit that
// matters).  Otherwise the walk starts in the cell that holds the entry point, t_start = max(0, entry).
template <class GG> // (R1GridGeom, or on the device the same read in place from the constant address space)
R1_GRID_HD bool r1g_setup(GG &g, const float ox, const float oy, const float oz, const float dx, const float dy, const float dz,
                          const float best, R1GridRay &r)
{
    float inx, outx, iny, outy, inz, outz;
    bool okx, oky, okz;
    r1g_axis(g.lo[0], g.cell[0], g.inv_cell[0], g.n[0], ox, dx, r.bx, r.ix, r.sx, inx, outx, okx);
    r1g_axis(g.lo[1], g.cell[1], g.inv_cell[1], g.n[1], oy, dy, r.by, r.iy, r.sy, iny, outy, oky);
    r1g_axis(g.lo[2], g.cell[2], g.inv_cell[2], g.n[2], oz, dz, r.bz, r.iz, r.sz, inz, outz, okz);
    const float t0 = fmaxf(fmaxf(inx, iny), fmaxf(inz, 0.0f));
    const float t1 = fminf(fminf(outx, outy), outz);
    if (!(okx & oky & okz) || !(t0 <= t1) || t0 > best)
        return false;
    // the cell that holds the entry point (p = o + t0 d; an axis without motion: o itself)
    r.jx = r1g_first(r.sx ? fmaf(t0, dx, ox) : ox, g.lo[0], g.inv_cell[0], g.n[0]);
    r.jy = r1g_first(r.sy ? fmaf(t0, dy, oy) : oy, g.lo[1], g.inv_cell[1], g.n[1]);
    r.jz = r1g_first(r.sz ? fmaf(t0, dz, oz) : oz, g.lo[2], g.inv_cell[2], g.n[2]);
    r.tx = r.sx ? r1g_bound(r.jx + (r.sx > 0), g.cell[0], r.bx, r.ix) : INFINITY;
    r.ty = r.sy ? r1g_bound(r.jy + (r.sy > 0), g.cell[1], r.by, r.iy) : INFINITY;
    r.tz = r.sz ? r1g_bound(r.jz + (r.sz > 0), g.cell[2], r.bz, r.iz) : INFINITY;
    return true;
}

template <class GG> // (R1GridGeom, or on the device the same read in place from the constant address space)
R1_GRID_HD uint32_t r1g_cell(GG &g, const R1GridRay &r) { return ((uint32_t)r.jz * (uint32_t)g.n[1] + (uint32_t)r.jy) * (uint32_t)g.n[0] + (uint32_t)r.jx; }

// After the current cell's spheres have been tested: false = the walk is over — the next cell is entered at a t beyond `best` (STRICTLY
// beyond: a sphere whose offer ties `best` lies in a cell entered at t <= best and must be presented for the lowest-index rule), or the
// ray leaves the box.  Otherwise moves to the next cell (the axis with the smallest boundary t; ties x, y, z).
template <class GG> // (R1GridGeom, or on the device the same read in place from the constant address space)
R1_GRID_HD bool r1g_step(GG &g, R1GridRay &r, const float best)
{
    const float t_out = fminf(fminf(r.tx, r.ty), r.tz);
    if (!(t_out <= best))
        return false;
    const bool ax = r.tx <= r.ty && r.tx <= r.tz;
    const bool ay = !ax && r.ty <= r.tz;
    const bool az = !ax && !ay;
    r.jx += ax ? r.sx : 0;
    r.jy += ay ? r.sy : 0;
    r.jz += az ? r.sz : 0;
    // (each axis' next boundary recomputed and kept only for the chosen one: selects between computed values, no divergent branch and
    //  no select between two fields of the grid, which the compiler turns into a load from a selected address — scratch memory)
    if ((ax & (r.jx < 0 || r.jx >= g.n[0])) | (ay & (r.jy < 0 || r.jy >= g.n[1])) | (az & (r.jz < 0 || r.jz >= g.n[2])))
        return false;
    const float tx = r1g_bound(r.jx + (r.sx > 0), g.cell[0], r.bx, r.ix);
    const float ty = r1g_bound(r.jy + (r.sy > 0), g.cell[1], r.by, r.iy);
    const float tz = r1g_bound(r.jz + (r.sz > 0), g.cell[2], r.bz, r.iz);
    r.tx = ax ? tx : r.tx;
    r.ty = ay ? ty : r.ty;
    r.tz = az ? tz : r.tz;
    return true;
}

#endif
