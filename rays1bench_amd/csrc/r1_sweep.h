// r1_sweep.h — the sweep's tables on the host (built by r1_sweep.cpp, uploaded by r1_scene.cpp): the sphere groups of level 1 in pair
// layout, their members, and the per-sphere rows the exact phase and the shading read.
#ifndef R1_SWEEP_H
#define R1_SWEEP_H

#include <stdint.h>

#include <vector>

#include "../../include/rays1.h"

struct R1Sweep
{
    std::vector<float> sweep;      // pair layout {cx0 cx1 cy0 cy1 cz0 cz1 Kp0 Kp1}, n_sweep groups + one chunk / tile of prefetch padding
    std::vector<float> exact;      // [active] {cx, cy, cz, radius_sq}
    std::vector<float> shade;      // [active] {inv_radius, albedo r, g, b}
    std::vector<float> mat;        // [active] {type, ref_idx, 1 / ref_idx, schlick r0}
    std::vector<uint32_t> members; // [n_sweep + padding][R1_GROUP_MAX] active indices, 0xFFFFFFFF = none
    std::vector<float> exact_g;    // the members' exact rows in group order, {0, 0, 0, -inf} = none
    uint32_t n_groups = 0, n_multi = 0, n_sweep = 0; // groups; those of 2..R1_GROUP_MAX members, which come first; groups padded
    std::vector<double> rbound;    // [active] r1_bound_radius: what the group bounds cover (the tree builder and the refit radii take it too)
    // per group, what its Kp was made from (r1_sweep_describe)
    std::vector<double> cover;     // R: |c_i - g| + rbound_i <= R for every member, g the stored fp32 centre
    std::vector<double> rule;      // the bounding radius around the fp64 centre that the R1_GROUP_RATIO rule was applied to
    std::vector<double> c_max2;    // max(|g|^2, max_i |c_i|^2), g the fp64 centre
};

// The tables for the active spheres of s (active_to_scene: r1_active_spheres).  No HIP call, no context.
void r1_build_sweep(const r1_scene *s, const std::vector<uint32_t> &active_to_scene, R1Sweep &out);

#endif
