// r1_grid.h — the uniform grid of R1_VARIANT_GRID on the host (built by r1_grid.cpp, uploaded by r1_scene_grid.cpp ensure_grid).
#ifndef R1_GRID_H
#define R1_GRID_H

#include <stdint.h>
#include <vector>

#include "r1_grid_dda.h"

#define R1_GRID_SPAN_MAX 64    // a sphere whose padded ball overlaps more cells is an outlier (tested by every ray before the walk)
#define R1_GRID_AXIS_MAX 4096  // cells per axis at most
#define R1_GRID_LDS_HALVES 8192 // small-scene kernel: cell starts + sphere ids (16 bits each) it keeps in LDS (16 KB); larger grids run the big kernel

struct r1_scene;

struct R1Grid
{
    R1GridGeom geom;
    std::vector<uint32_t> start;    // [cells + 1] CSR offsets into ids; cell (jx, jy, jz) = (jz ny + jy) nx + jx
    std::vector<uint32_t> ids;      // active sphere indices, ascending within a cell
    std::vector<uint32_t> outliers; // active indices every ray tests before the walk (ascending)
    uint32_t max_occupancy = 0;
    double pad = 0;    // largest registration pad: rho_i - r_i over the registered spheres
    double v_safe = 0; // V: origins within V of every registered centre walk the grid, the others take the tree
    double build_ms = 0;
    // the plan a regrid keeps (r1_grid_fill.h R1GridPlan): the last layout pass's coordinate bound and walk margin, the
    // outlier radius (R1_GRID_OUTLIER_RATIO x the median bound radius) and which axes got one cell
    double M = 0, delta = 0, big = 0;
    bool flat[3] = {false, false, false};
};

void r1_build_grid(uint32_t na, const float *cx, const float *cy, const float *cz, const float *rsq, const double *rbound, R1Grid &g);
int r1_grid_from_scene(const r1_scene *s, R1Grid &g); // the active spheres of s, filtered as r1_set_scene does

struct r1_grid_info;
// info and the optional outputs of r1_grid_describe, r1_grid_regrid_describe and r1_grid_download, from a grid in active indices
int r1_grid_report(const R1Grid &g, const std::vector<uint32_t> &scene_index, bool overflow, r1_grid_info *info, uint32_t *start_out, size_t start_cap,
                   uint32_t *ids_out, size_t ids_cap, uint32_t *outliers_out, size_t outliers_cap);

struct R1GridPlan;
void r1_grid_plan(const R1Grid &g, R1GridPlan &p); // what a regrid keeps of a build
// The host restatement of r1_regrid (r1_regrid.hip's steps through r1_grid_fill.h): the na active spheres' rows exact [na][4] and radii
// [na][2] re-registered against the plan.  out: geom, start, ids, outliers, pad, max_occupancy; returns true if the registrations exceed
// the id table's capacity (then v2 = -1, every start 0, no ids).
bool r1_grid_regrid_host(const R1GridPlan &p, uint32_t na, const float *exact, const double *radii, R1Grid &out);

#endif
