// r1_bvh.h — what r1_bvh.cpp hands to the rest of the host code: the built tree, the topology tables of a refit and of a re-sort, and the host
// forms of both.
#ifndef R1_BVH_H
#define R1_BVH_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "r1_bvh_fill.h"
#include "r1_bvh_sort.h"
#include "../../include/rays1.h"

struct R1Bvh
{
    std::vector<float> nodes;   // 16 floats per node, see R1DeviceScene::bvh_nodes
    std::vector<float> prims;   // leaf order, 8 floats per PAIR of spheres: {cx_a cx_b cy_a cy_b cz_a cz_b rsq_a rsq_b}
    std::vector<uint32_t> ids;  // 2 per pair: active index, 0xFFFFFFFF for the partner of an odd sphere
    std::vector<uint8_t> pair_pinned; // 1 per pair: the pair's leaf was made by the builder's outlier peel, a re-sort leaves its spheres where they are
    int max_depth = 0;          // inner nodes on the longest root-to-leaf path
    uint32_t n_leaves = 0;
    float centre[3] = {0, 0, 0}; // C of the pad formula (r1_bvh.cpp's header)
    int pad_local = 0;           // 1: pad measured per node (scenes of small spheres), 0: from `centre`
    int root_leaf = 0;           // 1 / 2: child 0 / 1 of the root is a leaf of <= 2 sphere pairs and the other child an inner node (the root step), 0: no
    int flat_axis = -1;          // 0 / 1 / 2: every box the node loop tests has nearly the same slab along this axis (r1_bvh.cpp "flat axis"), -1: none
    float flat_m = 0, flat_e = 0; // that axis: centre and half extent of the union of those slabs, rounded outward
    R1FillConst fill;            // the constants r1_bvh_fill.h's functions take: what a refit of this tree computes with
};

// What a refit needs besides the tree itself: all of it topology, unchanged by any move of the spheres.  Boxes are kept in
// one scratch array: entry n < nodes is inner node n's (the union of its two children's), entry nodes + l leaf l's.
struct R1RefitTopo
{
    std::vector<uint32_t> slot;      // [active spheres] the sphere's slot in ids / prims (the inverse of R1Bvh::ids)
    std::vector<uint32_t> leaf_ref;  // [leaves] the leaf's child reference (first pair, pairs)
    std::vector<uint32_t> child_box; // [2 x nodes] scratch entry of a node's child, 0xFFFFFFFF: an empty leaf
    std::vector<uint32_t> by_height; // [nodes] the nodes sorted by height (0: both children are leaves)
    std::vector<uint32_t> height_off; // [heights + 1] by_height[height_off[h] .. height_off[h + 1]) are the nodes of height h
};

// R1RefitTopo's tables behind the scene -> active map in one array of words, as the device holds them (r1_context refit_tab); off[k]: where
// scene_to_active, slot, leaf_ref, child_box, by_height begin
inline void r1_refit_pack(const std::vector<uint32_t> &scene_to_active, const R1RefitTopo &t, std::vector<uint32_t> &tab, size_t off[5])
{
    const std::vector<uint32_t> *parts[5] = {&scene_to_active, &t.slot, &t.leaf_ref, &t.child_box, &t.by_height};
    tab.clear();
    for (int k = 0; k < 5; ++k)
        off[k] = tab.size(), tab.insert(tab.end(), parts[k]->begin(), parts[k]->end());
}

// What a re-sort needs besides the tree and the refit's tables (r1_bvh_sort.h): topology too.  Positions 0 .. M are the movable
// slots in ascending slot order; a splitting node is an inner node whose two children both hold movable slots.
struct R1SortTopo
{
    std::vector<uint32_t> mov;       // [M] the movable spheres, ascending active index (a re-sort permutes them among the movable slots)
    std::vector<uint32_t> mslot;     // [M] position p's slot in ids / prims
    std::vector<R1SortSeg> seg;      // the splitting nodes, depth by depth (depths without one are left out), ascending b within a depth
    std::vector<uint32_t> depth_off; // [depths + 1] seg[depth_off[d] .. depth_off[d + 1]) are depth d's
    std::vector<uint32_t> pos_seg;   // [depths][M] the index in `seg` of depth d's node that holds position p, or R1S_NONE
};

// R1SortTopo's tables in one array of words, as the device holds them (r1_context sort_tab); off[k]: where mov, mslot, seg (3 words each), pos_seg begin
inline void r1_sort_pack(const R1SortTopo &s, std::vector<uint32_t> &tab, size_t off[4])
{
    const size_t m = s.mov.size();
    off[0] = 0, off[1] = m, off[2] = 2 * m, off[3] = 2 * m + 3 * s.seg.size();
    tab.assign(off[3] + s.pos_seg.size(), 0u);
    if (m)
        memcpy(&tab[off[0]], s.mov.data(), m * 4), memcpy(&tab[off[1]], s.mslot.data(), m * 4);
    if (!s.seg.empty())
        memcpy(&tab[off[2]], s.seg.data(), s.seg.size() * sizeof(R1SortSeg));
    if (!s.pos_seg.empty())
        memcpy(&tab[off[3]], s.pos_seg.data(), s.pos_seg.size() * 4);
}

void r1_build_bvh(uint32_t na, const float *cx, const float *cy, const float *cz, const float *rsq, const double *rbound, int leaf_max, R1Bvh &out);
int r1_active_spheres(const r1_scene *s, std::vector<uint32_t> &active_to_scene); // inv_radius != 0, finite
double r1_bound_radius(float radius_sq, float inv_radius);
double r1_test_radius(double rbound, float radius_sq); // the radius whose error terms the pad follows (r1f_sphere_box's r_test)
void r1_bvh_topology(const R1Bvh &b, uint32_t na, R1RefitTopo &t);
// The device refit's steps on the host, in its order and with its tables: new node rows for centres cx, cy, cz (active order; non-finite:
// the sphere is in no box).  A tree of 0 spheres is left alone.
void r1_bvh_sort_topology(const R1Bvh &b, R1SortTopo &s);
// The device re-sort's steps on the host, over its tables: the movable spheres re-dealt into the movable slots by r1_bvh_sort.h's rule for
// centres cx, cy, cz (active order); rewrites b.ids, b.prims (centre and rsq of the moved spheres) and t.slot.  The refit is the caller's.
void r1_bvh_resort_host(R1Bvh &b, R1RefitTopo &t, const R1SortTopo &s, const float *cx, const float *cy, const float *cz, const float *rsq);
void r1_bvh_refit_host(R1Bvh &b, const R1RefitTopo &t, uint32_t na, const float *cx, const float *cy, const float *cz, const float *rsq,
                       const double *rbound);

#endif
