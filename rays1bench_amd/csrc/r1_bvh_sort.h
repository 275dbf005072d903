// r1_bvh_sort.h — the rule by which the spheres are re-dealt into the box tree's leaf slots (r1_resort_spheres), shared by
// the host restatement (r1_bvh.cpp r1_bvh_resort_host) and the device kernels (r1_resort.hip), as r1_bvh_fill.h shares the refit's arithmetic.
//
// The tree keeps its topology.  A leaf the builder made by its outlier peel is PINNED (the ground and the big balls of the reference's
// scenes): its spheres keep their slots.  Every other occupied slot is MOVABLE; the movable slots in ascending slot order are the positions
// 0 .. M, and every inner node owns a contiguous segment [b, e) of them: child 0 the first k (its movable count), child 1 the rest.  Top
// down, a node with 0 < k < e - b picks the axis along which its spheres' centres reach furthest (the fp32 difference of the clamped
// largest and smallest coordinate; equal extents: x, then y, then z) and hands the k spheres smallest on that axis — by (key, active index):
// every composite key is distinct, so the result does not depend on the sorting algorithm — to child 0.  Inside a leaf the spheres stand
// in the order of x.
//
// Compares, selects and integer arithmetic only (one fp32 subtraction of finite values): the host and the device compute the same result.
#ifndef R1_BVH_SORT_H
#define R1_BVH_SORT_H

#include <stdint.h>

#include "r1_bvh_fill.h"

#define R1S_NONE 0xFFFFFFFFu

// The coordinate the rule orders by: the fp32 centre coordinate, a non-finite one replaced by +FLT_MAX (such a sphere is never hit and in no
// box: only the tree's quality is at stake for it), -0 by +0 (so that the key's order is the floats' own).
R1F_HD float r1s_clamp(float v)
{
    if (!r1f_finite(v))
        return 3.402823466e38f;
    return v == 0.0f ? 0.0f : v;
}

// Order-preserving map of a clamped coordinate to uint32: a < b as floats <=> key(a) < key(b)
R1F_HD uint32_t r1s_key(float clamped)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, clamped);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// (key, active index) of a before that of b
R1F_HD bool r1s_before(uint32_t key_a, uint32_t a, uint32_t key_b, uint32_t b) { return key_a < key_b || (key_a == key_b && a < b); }

// The split axis of a node from the clamped coordinates of the first and the last sphere of its segment in each axis' sorted list
R1F_HD int r1s_axis(const float first[3], const float last[3])
{
    const float ex = last[0] - first[0], ey = last[1] - first[1], ez = last[2] - first[2];
    int axis = 0;
    float best = ex;
    if (ey > best)
        axis = 1, best = ey;
    if (ez > best)
        axis = 2;
    return axis;
}

// Where the stable partition of a node's segment [b, e) puts the entry at position p of a list: `left` says whether the entry's sphere goes
// to child 0, left_rank counts the entries of [b, p) that do.
R1F_HD uint32_t r1s_dest(uint32_t b, uint32_t k, uint32_t p, uint32_t left_rank, bool left) { return left ? b + left_rank : b + k + (p - b - left_rank); }

// One splitting node of the re-sort (0 < k < e - b), in the tables both sides walk: its segment and child 0's share of it
struct R1SortSeg
{
    uint32_t b, k, e;
};

// What the re-sort's kernels read and write (r1_resort.hip), device memory; by value in their arguments.  M movable spheres, lists of 3 M
// entries (axis-major).
struct R1SortArgs
{
    const float *exact;        // [active][4] {cx cy cz radius_sq}: the device's truth
    float *prims;              // the tree's leaf spheres, 8 floats per pair: rewritten for movable slots
    uint32_t *ids;             // the tree's leaf slots: rewritten for movable slots
    uint32_t *slot;            // [active] the sphere's slot (R1RefitArgs::slot): rewritten for movable spheres
    const uint32_t *mov;       // [M] the movable spheres, ascending active index
    const uint32_t *mslot;     // [M] the movable slots, ascending: position p's slot
    const R1SortSeg *seg;      // the splitting nodes, depth by depth
    const uint32_t *pos_seg;   // [depths][M] the splitting node of that depth whose segment holds position p, or R1S_NONE
    uint32_t *list[2];         // [3 M] the sorted lists, two buffers taken in turn
    uint32_t *key[2];          // [3 M] the radix sort's keys, two buffers taken in turn
    uint32_t *seg_axis;        // [splitting nodes] the axis each chose
    uint32_t *flag;            // [active] 1: the sphere goes to child 0 of its node at the current depth
    uint32_t *scan;            // [3 M] flags in list order, then their exclusive prefix sum (in place)
    uint32_t *hist;            // [3][256][blocks of M] the radix sort's per-block digit counts, then their exclusive prefix sum (in place)
    uint32_t *sums;            // the scan's block sums, level after level
    uint32_t m;
};

#endif
