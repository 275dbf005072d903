// r1_bvh.cpp — host-side builder of the optional spatial index.
//
// The reference has no acceleration structure ("it's even more insane idea to use linear
// searching", README.md:163; the nested-Hitable stub at rayweek1.cpp:328-349 is unused): every
// ray is tested against every sphere.  R1_VARIANT_BVH keeps the reference's per-sphere
// arithmetic (exact_offer in r1_hit_sweep.hpp = rayweek1.cpp:192-202, :294-313) and only decides
// WHICH spheres are presented to it, through a binary tree of axis-aligned boxes that is
// conservative with respect to the reference's fp32 test, so that pixels and ray counts stay
// bit-identical to the exhaustive sweep (tests/test_gpu_parity.py::test_bvh_*).
//
// Conservativeness.  Let u = 2^-24, v = c - o.  The reference's fp32 discriminant differs from
// the real-number one by E1 <= 23 u |v|^2 + 2 u r^2 (co rounding, two FMA chains, the square,
// the final subtraction, and |d| = 1 +- 3u).  A sphere whose reference discriminant has a clear
// sign bit therefore has its centre within sqrt(r^2 + E1) <= r_eff + E1 / (2 r_eff) of the
// ray's line (r_eff = max(r, r_floor); the r_floor/2 this costs a degenerate sphere is added
// to the pad), and the point at its offered t lies within that distance + 5 u |v| of the
// centre.  A child box is stored as centre m and half extent e and has to be inflated by at least
//      pad_min = w2 * |m - o|^2 + k
// with  w2 = 2 * (40 u * max_i 1 / (2 r_eff,i)) + 2^-19   and   k = w2 * h^2 + 2^-20 + ...,
// h = max_i |c_i - m|, using |v|^2 <= 2 |m - o|^2 + 2 h^2.  The 2^-19 / 2^-20 terms cover the
// rounding of the slab test itself: products and differences (<= 6u D in position units, D the
// largest distance involved) and the 1-ulp reciprocals of the direction (v_rcp_f32, <= 2^-22 D),
// together < 2^-20.7 D <= 2^-21.7 (1 + D^2), against a budget of 2^-20 (1 + D^2).
//
// What the kernel evaluates (r1_hit_tree.hpp::bvh_box) is ONE fused multiply-add per node,
//      pad = A * R2 + K,      R2 = |o - C|^2 computed once per ray,
// C a fixed point of the scene (the per-axis median of the sphere centres, R1Bvh::centre), and
// A = 2 w2 + u, K = k + 2 w2 g^2 + u (1 + |C|_1), g = |m - C|, w2, k and g each CHILD's own (these trees fold K
// into the half extents child by child, below, so nothing forces both children to carry the larger one; A is
// the tree's maximum, >= 2 w2 + u of every child):
// |m - o|^2 <= 2 |o - C|^2 + 2 |m - C|^2, so pad >= pad_min for each child, at the price of boxes
// a few 1e-2 units wider than necessary (large scene: pad ~0.03 next to r = 0.45).  (One K per NODE, the worse
// child's, made the sibling of the ground sphere — m_y = -1000.5, g = 1000 — 17.5 units too wide on every side:
// the box of the root step, which 30.6 % of all rays passed only to fail both boxes of the node below.)  The u terms pay for
// the slab test's own form a = m * (1/d) - o * (1/d) (fused, o * (1/d) rounded once per ray): next to
// the errors budgeted above it adds u |o| (1 + u) in position units, and |o| <= |o - C| + |C| <=
// (1 + R2) / 2 + |C|.  A and K are rounded up with 2^-18 relative headroom for the fp32 evaluation
// of R2 (3 u) and of the fused multiply-add (u).
//
// Scenes of small spheres (R1Bvh::pad_local; the 100 004-sphere lattice: r = 0.034, spacing 0.08): w2 grows with 1 / r and
// a pad measured from ONE point of the scene (~0.1 there) would bury the boxes.  Such trees measure the distance per node:
//      pad = A * |s|^2 + K,   s = m0 + m1 - 2 o = 2 (m_n - o),  m_n the midpoint of the two child centres,
// A = (1 + eps) w2 / 4 + u / 8, K = k + (1 + 1 / eps) w2 g^2 + u (1/2 + |m_n|) + ..., g = |m0 - m1| / 2 = |m_c - m_n|:
// |m_c - o|^2 <= (|m_n - o| + g)^2 <= (1 + eps) |s|^2 / 4 + (1 + 1 / eps) g^2 for every eps > 0 (eps = g / the scene's
// scale: tight for origins that far away), and |o| <= |s| / 2 + |m_n| <= (1 + |s|^2 / 4) / 2 + |m_n|.  s is computed in
// fp32 (error per component <= delta = 4 u (|m0|_inf + |m1|_inf + 2 |o|_inf) <= 4 u (3 M + |s|), M = |m0|_inf + |m1|_inf);
// |s|^2 <= (1 + 2^-10) |s'|^2 + (1 + 2^10) 3 delta^2 puts 2^-10 more on A and A 3075 * 288 u^2 M^2 on K (the |s|^2
// part of delta^2 is 1e-10 relative).  9 VALU instructions per node visit instead of 1, still 7 fewer than round 1's form.
// The choice is made per tree from the median radius and the median distance from C: local when 4 w2_med G^2 > r_med / 4.
// Every constant is rounded up.  Extra visits are harmless: leaves apply the reference's rule.
#include <hip/hip_runtime.h>

#include "r1_device.h"
#include "r1_bvh.h"
#include "r1_internal.h"
#include "../../include/rays1.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace
{

typedef R1Box Box;                                       // r1_bvh_fill.h: the arithmetic the device refit shares
inline float round_up(double v) { return r1f_round_up(v); }

struct Builder
{
    const float *cx, *cy, *cz, *rsq; // active order, the fp32 values the exact test reads
    const double *rbound;             // radius the boxes must cover (r1_bound_radius)
    std::vector<Box> sphere;
    std::vector<uint32_t> order;
    R1Bvh *out;
    int leaf_max;
    double centre[3]; // C of the pad formula, == out->centre
    bool pad_local = false;

    static const uint32_t LEAF = 0x80000000u;

    Box bound(uint32_t b, uint32_t e) const
    {
        Box r;
        r.clear();
        for (uint32_t i = b; i < e; ++i)
            r.merge(sphere[order[i]]);
        return r;
    }

    uint32_t make_leaf(uint32_t b, uint32_t e, bool pinned = false)
    {
        // spheres are stored in PAIRS (two spheres per pair of 16-byte loads); the partner of
        // an odd sphere has radius_sq = -inf, which makes its discriminant -inf: never flagged
        const uint32_t first = (uint32_t)(out->ids.size() / 2);
        const uint32_t pairs = (e - b + 1) / 2;
        for (uint32_t q = 0; q < pairs; ++q)
        {
            const uint32_t ia = order[b + 2 * q];
            const bool has_b = b + 2 * q + 1 < e;
            const uint32_t ib = has_b ? order[b + 2 * q + 1] : ia;
            const float pad_r = -INFINITY;
            const float v[8] = {cx[ia], has_b ? cx[ib] : 0.0f, cy[ia], has_b ? cy[ib] : 0.0f,
                                cz[ia], has_b ? cz[ib] : 0.0f, rsq[ia], has_b ? rsq[ib] : pad_r};
            out->prims.insert(out->prims.end(), v, v + 8);
            out->ids.push_back(ia);
            out->ids.push_back(has_b ? ib : 0xFFFFFFFFu);
            out->pair_pinned.push_back(pinned ? 1 : 0); // (a side table: r1_bvh_sort.h)
        }
        ++out->n_leaves;
        return LEAF | (pairs << 28) | first;
    }

    // returns the child reference for order[b, e); bx = its bounds; peeled: these are the outliers a peel set apart (one leaf, pinned)
    uint32_t build(uint32_t b, uint32_t e, int depth, const Box &bx, bool peeled = false)
    {
        const uint32_t n = e - b;
        if (n <= (uint32_t)leaf_max)
            return make_leaf(b, e, peeled);

        // levels a balanced split of n spheres still needs; SAH only while the depth budget allows
        int need = 0;
        while (((uint64_t)leaf_max << need) < n)
            ++need;
        const bool force_median = depth + need + 1 >= R1_BVH_STACK;

        uint32_t mid = 0;
        int axis = 0;
        bool peel = false;
        // Outliers first: a few spheres much larger than the rest of the node (the ground and the r = 2 balls among the
        // r = 0.45 lattice of the reference's large scene) would inflate every box on their way down a centroid split
        // (the balls sat four levels deep and made the boxes above them 2.7 high instead of 0.5).  Up to `leaf_max`
        // spheres more than R1_BVH_PEEL_RATIO (4) x the node's median radius become ONE leaf here and the rest keeps tight
        // boxes: large scene 24.3 -> 26.5 Grays/s, 100 004-sphere scene 12.2 -> 12.8 (tools: R1_BVH_PEEL=0 switches it off).
        static const int peel_env = (int)r1_knob("R1_BVH_PEEL", 1);
        if (peel_env && !force_median && depth + need + 2 < R1_BVH_STACK && n > 2u * (uint32_t)leaf_max) // (a peel costs a level)
        {
            std::vector<double> rs(n);
            for (uint32_t i = 0; i < n; ++i)
                rs[i] = sphere[order[b + i]].rmax;
            std::nth_element(rs.begin(), rs.begin() + n / 2, rs.end());
            static const double ratio_env = r1_knob_f("R1_BVH_PEEL_RATIO", 4.0);
            const double big = ratio_env * rs[n / 2];
            uint32_t nb = 0;
            for (uint32_t i = b; i < e; ++i)
                nb += sphere[order[i]].rmax > big ? 1u : 0u;
            if (nb >= 1 && nb <= (uint32_t)leaf_max)
            {
                std::stable_partition(order.begin() + b, order.begin() + e, [&](uint32_t q) { return sphere[q].rmax > big; });
                mid = b + nb, peel = true;
            }
        }
        if (mid == 0)
        {
            double ext[3];
            for (int a = 0; a < 3; ++a)
                ext[a] = bx.chi[a] - bx.clo[a];
            axis = ext[1] > ext[0] ? 1 : 0;
            if (ext[2] > ext[axis])
                axis = 2;
        }
        if (!force_median && mid == 0)
        {
            // binned surface-area heuristic over the three axes (16 bins on the centres)
            const int NB = 16;
            double best = 1e300;
            int best_axis = -1, best_bin = -1;
            for (int a = 0; a < 3; ++a)
            {
                const double lo = bx.clo[a], ext = bx.chi[a] - bx.clo[a];
                if (!(ext > 0))
                    continue;
                Box bins[NB];
                uint32_t cnt[NB];
                for (int i = 0; i < NB; ++i)
                    bins[i].clear(), cnt[i] = 0;
                const double scale = NB / ext;
                for (uint32_t i = b; i < e; ++i)
                {
                    const Box &s = sphere[order[i]];
                    int bi = (int)((s.clo[a] - lo) * scale);
                    bi = bi < 0 ? 0 : (bi >= NB ? NB - 1 : bi);
                    bins[bi].merge(s), ++cnt[bi];
                }
                double right_area[NB];
                uint32_t right_cnt[NB];
                Box acc;
                acc.clear();
                uint32_t c = 0;
                for (int i = NB - 1; i > 0; --i)
                {
                    if (cnt[i])
                        acc.merge(bins[i]);
                    c += cnt[i];
                    right_area[i] = c ? acc.area() : 0, right_cnt[i] = c;
                }
                acc.clear(), c = 0;
                for (int i = 0; i < NB - 1; ++i)
                {
                    if (cnt[i])
                        acc.merge(bins[i]);
                    c += cnt[i];
                    if (c == 0 || right_cnt[i + 1] == 0)
                        continue;
                    const double cost = acc.area() * c + right_area[i + 1] * right_cnt[i + 1];
                    if (cost < best)
                        best = cost, best_axis = a, best_bin = i;
                }
            }
            if (best_axis >= 0)
            {
                const int a = best_axis;
                const double lo = bx.clo[a], scale = NB / (bx.chi[a] - bx.clo[a]);
                auto it = std::partition(order.begin() + b, order.begin() + e, [&](uint32_t s) {
                    int bi = (int)((sphere[s].clo[a] - lo) * scale);
                    bi = bi < 0 ? 0 : (bi >= NB ? NB - 1 : bi);
                    return bi <= best_bin;
                });
                mid = (uint32_t)(it - order.begin());
            }
        }
        if (mid <= b || mid >= e)
        {
            // median along the widest axis of the centres (also: all centres equal)
            mid = b + n / 2;
            const int a = axis;
            std::nth_element(order.begin() + b, order.begin() + mid, order.begin() + e, [&](uint32_t p, uint32_t q) {
                return sphere[p].clo[a] < sphere[q].clo[a] || (sphere[p].clo[a] == sphere[q].clo[a] && p < q);
            });
        }

        const uint32_t node = (uint32_t)(out->nodes.size() / 16);
        out->nodes.resize(out->nodes.size() + 16);
        out->max_depth = std::max(out->max_depth, depth + 1);
        const Box b0 = bound(b, mid), b1 = bound(mid, e);
        const uint32_t c0 = build(b, mid, depth + 1, b0, peel);
        const uint32_t c1 = build(mid, e, depth + 1, b1);
        fill(node, b0, c0, b1, c1);
        return node;
    }

    // the node's row from its children's boxes (r1_bvh_fill.h) and the child references
    void fill(uint32_t node, const Box &b0, uint32_t c0, const Box &b1, uint32_t c1)
    {
        float *p = &out->nodes[16 * (size_t)node];
        r1f_fill(out->fill, b0, b1, p);
        memcpy(&p[14], &c0, 4);
        memcpy(&p[15], &c1, 4);
    }
};

} // namespace

// Builds the tree over the `na` active spheres (fp32 arrays in active order).  Node 0 is always
// an inner node (the root), even for 0 or 1 spheres.
void r1_build_bvh(uint32_t na, const float *cx, const float *cy, const float *cz, const float *rsq, const double *rbound, int leaf_max,
                  R1Bvh &out)
{
    out.nodes.clear(), out.prims.clear(), out.ids.clear(), out.pair_pinned.clear();
    out.max_depth = 0, out.n_leaves = 0;
    if (leaf_max < 1)
        leaf_max = 1;
    if (leaf_max > 14)
        leaf_max = 14; // 7 pairs
    Builder B;
    B.cx = cx, B.cy = cy, B.cz = cz, B.rsq = rsq, B.rbound = rbound;
    B.out = &out;
    B.leaf_max = leaf_max;
    B.sphere.resize(na);
    B.order.resize(na);
    for (uint32_t a = 0; a < na; ++a)
    {
        B.order[a] = a;
        Box &s = B.sphere[a];
        // extents cover rbound (>= the radius the exact test reads, r1_bound_radius); the error terms
        // E1 / (2 r) follow the radius the test itself uses, sqrt(radius_sq) — the smaller, safer one
        r1f_sphere_box(cx[a], cy[a], cz[a], rbound[a], r1_test_radius(rbound[a], rsq[a]), s);
    }
    // C: the per-axis median of the centres (the ground sphere's centre, 1000 units below, must not drag it away)
    for (int k = 0; k < 3; ++k)
    {
        const float *src = k == 0 ? cx : (k == 1 ? cy : cz);
        std::vector<float> v(src, src + na);
        double med = 0;
        if (na)
        {
            std::nth_element(v.begin(), v.begin() + na / 2, v.end());
            med = v[na / 2];
        }
        out.centre[k] = (float)med;
        B.centre[k] = (double)out.centre[k]; // exactly the fp32 value the kernel subtracts
    }
    // pad formula of this tree (see the header): per node for scenes of small spheres
    {
        std::vector<double> rr(na), dd(na);
        for (uint32_t a = 0; a < na; ++a)
        {
            rr[a] = B.sphere[a].rmax;
            const double dx = cx[a] - B.centre[0], dy = cy[a] - B.centre[1], dz = cz[a] - B.centre[2];
            dd[a] = dx * dx + dy * dy + dz * dz;
        }
        bool local = false;
        if (na)
        {
            std::nth_element(rr.begin(), rr.begin() + na / 2, rr.end());
            std::nth_element(dd.begin(), dd.begin() + na / 2, dd.end());
            const double r_med = std::max(rr[na / 2], 1e-30), G2 = 4.0 * dd[na / 2];
            const double w2_med = 80.0 * ldexp(1.0, -24) / (2.0 * r_med) + ldexp(1.0, -19);
            local = 4.0 * w2_med * G2 > 0.25 * r_med;
        }
        static const int pad_env = (int)r1_knob("R1_BVH_PAD_LOCAL", -1); // tuning experiments
        if (pad_env >= 0)
            local = pad_env != 0;
        B.pad_local = local;
        out.pad_local = local ? 1 : 0;
        // what fill() computes with, and every later refit of this tree (r1_bvh_fill.h)
        static const int child_k = (int)r1_knob("R1_BVH_CHILD_K", 1); // tuning experiments: 0 = both children carry the worse child's K
        for (int k = 0; k < 3; ++k)
            out.fill.centre[k] = B.centre[k];
        out.fill.d_typ = na ? std::max(std::sqrt(4.0 * dd[na / 2]), 1e-30) : 1.0; // twice the median distance of the centres from C
        out.fill.pad_local = out.pad_local, out.fill.child_k = child_k;
    }
    // the root is node 0
    out.nodes.resize(16);
    Box empty;
    empty.clear();
    auto fill_root_with = [&](const Box &b0, uint32_t c0, const Box *b1, uint32_t c1) {
        if (b1)
        {
            B.fill(0, b0, c0, *b1, c1);
            return;
        }
        // one child only: the other never passes (half extent -inf) and is an empty leaf anyway
        B.fill(0, b0, c0, b0, c1);
        float *p = &out.nodes[0];
        p[7] = p[9] = p[11] = -INFINITY;
    };
    const uint32_t EMPTY_LEAF = Builder::LEAF; // count 0
    if (na == 0)
    {
        Box z;
        z.clear();
        for (int k = 0; k < 3; ++k)
            z.lo[k] = z.hi[k] = z.clo[k] = z.chi[k] = 0;
        fill_root_with(z, EMPTY_LEAF, nullptr, EMPTY_LEAF);
        float *p = &out.nodes[0];
        p[6] = p[8] = p[10] = -INFINITY;
        out.max_depth = 1;
    }
    else if (na <= (uint32_t)leaf_max)
    {
        const Box all = B.bound(0, na);
        const uint32_t leaf = B.make_leaf(0, na);
        fill_root_with(all, leaf, nullptr, EMPTY_LEAF);
        out.max_depth = 1;
    }
    else
    {
        // build() allocates its node first: make the top call land on node 0
        out.nodes.clear();
        const Box all = B.bound(0, na);
        const uint32_t root = B.build(0, na, 0, all);
        (void)root; // == 0
    }
    // Node order: the top of the tree breadth first (the first R1_BVH_TOP_NODES nodes = the levels every walk starts
    // with, which the big-scene kernels keep in LDS), the rest depth first below them (a parent next to its first child,
    // as build() allocates them).  Child references are rewritten; node 0 stays the root.
    {
        const uint32_t nn = (uint32_t)(out.nodes.size() / 16);
        static const int top_env = (int)r1_knob("R1_BVH_TOP", R1_BVH_TOP_NODES); // tuning experiments
        const uint32_t top = (uint32_t)std::max(0, top_env);
        if (nn > 1 && top > 1)
        {
            auto child = [&](uint32_t n, int c) {
                uint32_t r;
                memcpy(&r, &out.nodes[16 * (size_t)n + 14 + c], 4);
                return r;
            };
            std::vector<uint32_t> order_new; // old index of the node at each new position
            order_new.reserve(nn);
            std::vector<uint32_t> frontier(1, 0u);
            size_t head = 0;
            while (head < frontier.size() && frontier.size() < top) // breadth first until `top` nodes are known
            {
                const uint32_t n = frontier[head++];
                for (int c = 0; c < 2; ++c)
                    if (!(child(n, c) & Builder::LEAF))
                        frontier.push_back(child(n, c));
            }
            // frontier[0 .. head) are expanded, frontier[head ..) are the roots of the remaining subtrees
            std::vector<char> placed(nn, 0);
            for (uint32_t n : frontier)
                order_new.push_back(n), placed[n] = 1;
            for (size_t f = head; f < frontier.size(); ++f) // depth first below every unexpanded top node
            {
                std::vector<uint32_t> stack;
                for (int c = 1; c >= 0; --c)
                    if (!(child(frontier[f], c) & Builder::LEAF))
                        stack.push_back(child(frontier[f], c));
                while (!stack.empty())
                {
                    const uint32_t n = stack.back();
                    stack.pop_back();
                    if (placed[n])
                        continue;
                    order_new.push_back(n), placed[n] = 1;
                    for (int c = 1; c >= 0; --c)
                        if (!(child(n, c) & Builder::LEAF))
                            stack.push_back(child(n, c));
                }
            }
            if (order_new.size() == nn)
            {
                std::vector<uint32_t> new_of(nn);
                for (uint32_t i = 0; i < nn; ++i)
                    new_of[order_new[i]] = i;
                std::vector<float> moved(out.nodes.size());
                for (uint32_t i = 0; i < nn; ++i)
                {
                    memcpy(&moved[16 * (size_t)i], &out.nodes[16 * (size_t)order_new[i]], 64);
                    for (int c = 0; c < 2; ++c)
                    {
                        uint32_t r;
                        memcpy(&r, &moved[16 * (size_t)i + 14 + c], 4);
                        if (!(r & Builder::LEAF))
                        {
                            r = new_of[r];
                            memcpy(&moved[16 * (size_t)i + 14 + c], &r, 4);
                        }
                    }
                }
                out.nodes.swap(moved);
            }
        }
    }
    // Trees whose pad is measured from the scene's centre: ONE A for the whole tree (the largest of the nodes': pad only grows) and
    // every child's K folded into its half extents (fill()), e' = e + K rounded up — b = e |1/d| + (A R2 + K) |1/d| = e' |1/d| + (A R2) |1/d| —
    // so that the kernels which keep the table in LDS evaluate A R2 |1/d| once per RAY instead of a fused multiply-add and three
    // products per node visit (bvh_advance; 51 -> 47 VALU instructions per visit).  The same number of fp32 roundings as before on the
    // way to b (product, product, fused multiply-add), covered by the same 2^-18 headroom on A and K.  Nodes keep {A, 0} in the pad
    // slots: the kernels that read the pad per node (table in global memory) and the CPU restatement of the visit rule see the same rule.
    if (!B.pad_local)
    {
        const size_t nn = out.nodes.size() / 16;
        float a_max = 0.0f;
        for (size_t n = 0; n < nn; ++n)
            a_max = std::max(a_max, out.nodes[16 * n + 12]);
        for (size_t n = 0; n < nn; ++n)
            out.nodes[16 * n + 12] = a_max;
    }
    // The root of the reference's scenes is [one leaf of outliers: the ground + the three big balls | the lattice] (the peeling above),
    // and EVERY ray tests that leaf.  The tree kernels take this step out of the walk's divergent loops: a ray that starts its walk tests
    // the root's leaf child (<= 2 pairs) and then the box of the other child in straight-line code, together with the other rays of the
    // wave that start in the same iteration, and the walk begins at the other child (bvh_advance).  root_leaf says whether the root has
    // that shape and which child is the leaf.
    out.root_leaf = 0;
    if (out.nodes.size() >= 16)
    {
        uint32_t c[2];
        memcpy(c, &out.nodes[14], 8);
        for (int k = 0; k < 2; ++k)
        {
            const uint32_t pairs = (c[k] >> 28) & 7u;
            if ((c[k] & Builder::LEAF) && !(c[1 - k] & Builder::LEAF) && pairs >= 1 && pairs <= 2)
                out.root_leaf = k + 1;
        }
    }
    // Flat axis.  The reference's scenes are lattices of equal spheres on a plane: every box the node loop tests (the child boxes of
    // every inner node, but for a root that has the root-step shape: its boxes are tested outside the loop) has, within a few per cent,
    // the same slab along the plane's normal, and a third of the loop's box arithmetic recomputes it.  For the trees the `LN` walks
    // take (pad from the scene's centre, table in LDS) the builder names the axis — at most one — along which the UNION of those slabs
    // is at most R1_BVH_FLAT_RATIO x the narrowest of them, and stores the union as (m_u, e_u) rounded outward: m_u - e_u <= m - e and
    // m_u + e_u >= m + e in real arithmetic for every such box, K included.  bvh_advance tests that ONE slab once per call instead of
    // each box's own: a wider box is a conservative box, and the slab test has the form and the operand sizes the pad budgets for.
    // Among several such axes the one with the smallest ratio; equal ratios: y, then x, then z.  The decision depends on the scene alone.
    // 1.25: the large scene has 1.12, the medium one (spheres at y = 0, 1 and 1.5) 2.30 — forcing the union there costs +15 % node
    // visits.  1.0 / 1.25 / 1.5 on the large scene: DESIGN.md 4.17.  0 = never flat.
    out.flat_axis = -1, out.flat_m = out.flat_e = 0.0f;
    {
        static const double ratio_env = r1_knob_f("R1_BVH_FLAT_RATIO", 1.25);
        const size_t nn = out.nodes.size() / 16;
        // (a tree of one node has no walk to shorten — its one or two boxes would pass for flat along every axis — and the kernels keep
        //  the slab in node 1's pad slots)
        if (ratio_env > 0 && !B.pad_local && nn >= 2 && nn <= R1_NODES_LDS_MAX && na <= R1_MAX_ACTIVE_10BIT)
        {
            double best_ratio = 1e300;
            for (int a : {1, 0, 2})
            {
                double L = 1e300, H = -1e300, narrow = 1e300;
                for (size_t n = out.root_leaf ? 1 : 0; n < nn; ++n)
                    for (int c = 0; c < 2; ++c)
                    {
                        const double m = out.nodes[16 * n + 2 * a + c], e = out.nodes[16 * n + 6 + 2 * a + c];
                        if (!(e >= 0)) // (-inf: a child that never passes)
                            continue;
                        L = std::min(L, m - e), H = std::max(H, m + e), narrow = std::min(narrow, 2.0 * e);
                    }
                if (!(H >= L) || !(narrow > 0) || !std::isfinite(H - L))
                    continue;
                const double ratio = (H - L) / narrow;
                if (ratio <= ratio_env && ratio < best_ratio)
                {
                    best_ratio = ratio;
                    const float mu = (float)(0.5 * (L + H));
                    out.flat_axis = a, out.flat_m = mu, out.flat_e = round_up(std::max(H - (double)mu, (double)mu - L));
                }
            }
        }
    }
    // keep the tables non-empty for the uploader
    if (out.prims.empty())
        out.prims.assign(8, 0.0f), out.ids.assign(2, 0xFFFFFFFFu), out.pair_pinned.assign(1, 0);
}

// The hittable ("active") spheres of a caller's scene, in scene order: inv_radius != 0
// (rayweek1.cpp:291).  A sphere with a non-finite centre or radius_sq can never be hit by the
// reference's arithmetic (NaN/inf discriminant or roots fail every compare, rayweek1.cpp:204,
// :297-309) and is dropped like a placeholder, which also keeps such values out of the builders.
// One helper for r1_set_scene and r1_bvh_describe, so both see the same spheres.
int r1_active_spheres(const r1_scene *s, std::vector<uint32_t> &active_to_scene)
{
    active_to_scene.clear();
    for (uint32_t i = 0; i < s->count; ++i)
    {
        if (std::isnan(s->inv_radius[i]))
        {
            r1_set_error("scene: sphere %u has inv_radius NaN", i);
            return R1_EINVAL;
        }
        if (s->inv_radius[i] == 0)
            continue;
        if (!std::isfinite(s->center_x[i]) || !std::isfinite(s->center_y[i]) || !std::isfinite(s->center_z[i]) ||
            !std::isfinite(s->radius_sq[i]))
            continue;
        active_to_scene.push_back(i);
    }
    return R1_OK;
}

// Radius every conservative bound (group bounding spheres, tree boxes) must cover.  The hit test
// reads radius_sq only (rayweek1.cpp:198); SphereSOA::add stores radius_sq = r*r and inv_radius =
// 1/r of the same r (soa_sphere.cpp:70-85), but a C-ABI caller may hand over arrays that disagree
// (or a negative inv_radius): taking the larger of the two keeps every bound conservative for
// whatever the exact test can accept instead of silently dropping hits.
double r1_bound_radius(float radius_sq, float inv_radius) { return r1f_bound_radius(radius_sq, inv_radius); }

// The radius whose error terms E1 / (2 r) the pad follows: the one the exact test itself uses, sqrt(radius_sq), never more than the bound
// radius — the smaller, safer one (r1f_sphere_box's r_test).  Both in r1_bvh_fill.h: the device derives them too (r1_update_spheres*).
double r1_test_radius(double rbound, float radius_sq) { return r1f_test_radius(rbound, radius_sq); }

// ---- refit ----------------------------------------------------------------------

static int node_height(const R1Bvh &b, uint32_t n, std::vector<int> &h)
{
    if (h[n] >= 0)
        return h[n];
    int v = 0;
    for (int c = 0; c < 2; ++c)
    {
        uint32_t r;
        memcpy(&r, &b.nodes[16 * (size_t)n + 14 + c], 4);
        if (!(r & 0x80000000u))
            v = std::max(v, 1 + node_height(b, r, h)); // (at most R1_BVH_STACK levels)
    }
    return h[n] = v;
}

void r1_bvh_topology(const R1Bvh &b, uint32_t na, R1RefitTopo &t)
{
    const uint32_t NONE = 0xFFFFFFFFu, nn = (uint32_t)(b.nodes.size() / 16);
    t.slot.assign(na ? na : 1, NONE);
    for (size_t q = 0; q < b.ids.size(); ++q)
        if (b.ids[q] < na)
            t.slot[b.ids[q]] = (uint32_t)q;
    t.leaf_ref.clear();
    t.child_box.assign(2 * (size_t)nn, NONE);
    for (uint32_t n = 0; n < nn; ++n)
        for (int c = 0; c < 2; ++c)
        {
            uint32_t r;
            memcpy(&r, &b.nodes[16 * (size_t)n + 14 + c], 4);
            if (!(r & 0x80000000u))
                t.child_box[2 * (size_t)n + c] = r;
            else if ((r >> 28) & 7u)
                t.child_box[2 * (size_t)n + c] = nn + (uint32_t)t.leaf_ref.size(), t.leaf_ref.push_back(r);
        }
    std::vector<int> h(nn, -1);
    int top = 0;
    for (uint32_t n = 0; n < nn; ++n)
        top = std::max(top, node_height(b, n, h));
    t.height_off.assign((size_t)top + 2, 0u);
    for (uint32_t n = 0; n < nn; ++n)
        ++t.height_off[(size_t)h[n] + 1];
    for (int k = 0; k <= top; ++k)
        t.height_off[(size_t)k + 1] += t.height_off[k];
    t.by_height.assign(nn, 0u);
    std::vector<uint32_t> at(t.height_off.begin(), t.height_off.end() - 1);
    for (uint32_t n = 0; n < nn; ++n)
        t.by_height[at[h[n]]++] = n;
}

void r1_bvh_refit_host(R1Bvh &b, const R1RefitTopo &t, uint32_t na, const float *cx, const float *cy, const float *cz, const float *rsq,
                       const double *rbound)
{
    if (na == 0)
        return; // nothing to refit
    const size_t nn = b.nodes.size() / 16, nl = t.leaf_ref.size();
    std::vector<float> exact(4 * (size_t)na);
    std::vector<double> radii(2 * (size_t)na);
    for (uint32_t a = 0; a < na; ++a)
    {
        exact[4 * (size_t)a + 0] = cx[a], exact[4 * (size_t)a + 1] = cy[a], exact[4 * (size_t)a + 2] = cz[a], exact[4 * (size_t)a + 3] = rsq[a];
        radii[2 * (size_t)a + 0] = rbound[a], radii[2 * (size_t)a + 1] = r1_test_radius(rbound[a], rsq[a]);
    }
    std::vector<R1Box> box(nn + nl);
    for (size_t l = 0; l < nl; ++l) // "leaf boxes"
        r1f_refit_leaf(t.leaf_ref[l], b.ids.data(), exact.data(), radii.data(), box[nn + l]);
    float a_max = 0.0f;
    for (size_t k = 0; k + 1 < t.height_off.size(); ++k) // one launch per height, lowest first
        for (uint32_t i = t.height_off[k]; i < t.height_off[k + 1]; ++i)
            a_max = std::max(a_max, r1f_refit_node(b.fill, t.by_height[i], t.child_box.data(), box.data(), b.nodes.data()));
    if (!b.pad_local) // "finish": ONE A for the whole tree, as the builder's last step
        for (size_t n = 0; n < nn; ++n)
            b.nodes[16 * n + 12] = a_max;
    b.flat_axis = -1, b.flat_m = b.flat_e = 0.0f; // (no slab is computed for a moved scene)
}

// ---- re-sort --------------------------------------------------------

// movable slots below `ref`, in the order a walk with child 0 first meets them: the builder's slot order
static uint32_t sort_walk(const R1Bvh &b, uint32_t ref, size_t depth, R1SortTopo &s, std::vector<std::vector<R1SortSeg>> &by_depth)
{
    if (ref & 0x80000000u)
    {
        const uint32_t first = ref & 0x0FFFFFFFu, pairs = (ref >> 28) & 7u;
        uint32_t m = 0;
        for (uint32_t q = 2u * first; q < 2u * (first + pairs); ++q)
            if (b.ids[q] != 0xFFFFFFFFu && !b.pair_pinned[q >> 1])
                s.mslot.push_back(q), s.mov.push_back(b.ids[q]), ++m;
        return m;
    }
    uint32_t c[2];
    memcpy(c, &b.nodes[16 * (size_t)ref + 14], 8);
    const uint32_t at = (uint32_t)s.mslot.size();
    const uint32_t k = sort_walk(b, c[0], depth + 1, s, by_depth);
    const uint32_t m = k + sort_walk(b, c[1], depth + 1, s, by_depth);
    if (k > 0 && k < m)
    {
        if (by_depth.size() <= depth)
            by_depth.resize(depth + 1);
        by_depth[depth].push_back(R1SortSeg{at, k, at + m});
    }
    return m;
}

void r1_bvh_sort_topology(const R1Bvh &b, R1SortTopo &s)
{
    s.mov.clear(), s.mslot.clear(), s.seg.clear(), s.pos_seg.clear();
    s.depth_off.assign(1, 0u);
    std::vector<std::vector<R1SortSeg>> by_depth;
    if (b.nodes.size() >= 16)
        sort_walk(b, 0u, 0, s, by_depth);
    std::sort(s.mov.begin(), s.mov.end());
    const size_t m = s.mov.size();
    for (const std::vector<R1SortSeg> &level : by_depth)
    {
        if (level.empty())
            continue;
        const size_t row = s.pos_seg.size();
        s.pos_seg.resize(row + m, R1S_NONE);
        for (const R1SortSeg &g : level) // (the walk meets one depth's nodes in ascending b)
        {
            for (uint32_t p = g.b; p < g.e; ++p)
                s.pos_seg[row + p] = (uint32_t)s.seg.size();
            s.seg.push_back(g);
        }
        s.depth_off.push_back((uint32_t)s.seg.size());
    }
}

void r1_bvh_resort_host(R1Bvh &b, R1RefitTopo &t, const R1SortTopo &s, const float *cx, const float *cy, const float *cz, const float *rsq)
{
    const size_t m = s.mov.size();
    if (m == 0)
        return;
    const float *const c[3] = {cx, cy, cz};
    // "three sorted lists": (key, active index) — every composite key is distinct, so any sorting algorithm gives this order
    std::vector<uint32_t> list[3], next(m);
    for (int a = 0; a < 3; ++a)
    {
        list[a] = s.mov;
        std::sort(list[a].begin(), list[a].end(), [&](uint32_t p, uint32_t q) { return r1s_before(r1s_key(r1s_clamp(c[a][p])), p, r1s_key(r1s_clamp(c[a][q])), q); });
    }
    std::vector<uint8_t> left(t.slot.size(), 0);
    std::vector<uint32_t> axis(s.seg.size(), 0u);
    for (size_t d = 0; d + 1 < s.depth_off.size(); ++d) // "per depth of the tree"
    {
        const uint32_t *pos_seg = &s.pos_seg[d * m];
        for (uint32_t g = s.depth_off[d]; g < s.depth_off[d + 1]; ++g) // "axis"
        {
            float first[3], last[3];
            for (int a = 0; a < 3; ++a)
                first[a] = r1s_clamp(c[a][list[a][s.seg[g].b]]), last[a] = r1s_clamp(c[a][list[a][s.seg[g].e - 1]]);
            axis[g] = (uint32_t)r1s_axis(first, last);
        }
        for (uint32_t p = 0; p < m; ++p) // "flag"
            if (pos_seg[p] != R1S_NONE)
                left[list[axis[pos_seg[p]]][p]] = p < s.seg[pos_seg[p]].b + s.seg[pos_seg[p]].k ? 1 : 0;
        for (int a = 0; a < 3; ++a) // "prefix sum and stable segmented partition"
        {
            uint32_t sum = 0, base = 0;
            for (uint32_t p = 0; p < m; ++p)
            {
                const uint32_t g = pos_seg[p], sphere = list[a][p];
                if (g == R1S_NONE)
                {
                    next[p] = sphere;
                    continue;
                }
                if (p == s.seg[g].b)
                    base = sum;
                next[r1s_dest(s.seg[g].b, s.seg[g].k, p, sum - base, left[sphere] != 0)] = sphere;
                sum += left[sphere];
            }
            list[a].swap(next);
        }
    }
    for (uint32_t p = 0; p < m; ++p) // "write-back": inside a leaf the spheres stand in the order of the x list
    {
        const uint32_t sphere = list[0][p], q = s.mslot[p];
        b.ids[q] = sphere, t.slot[sphere] = q;
        float *pr = &b.prims[8 * (size_t)(q >> 1) + (q & 1u)];
        pr[0] = cx[sphere], pr[2] = cy[sphere], pr[4] = cz[sphere], pr[6] = rsq[sphere];
    }
}

// the tree r1_set_scene builds for `s`, and what it was built from (active order)
struct Described
{
    std::vector<float> x, y, z, r;
    std::vector<double> rb;
    std::vector<uint32_t> scene_index;
    uint32_t na = 0;
    R1Bvh b;
};
static int describe_build(const r1_scene *s, int32_t leaf_max, Described &d)
{
    if (!s->center_x || !s->center_y || !s->center_z || !s->radius_sq || !s->inv_radius)
        return R1_EINVAL;
    if (r1_active_spheres(s, d.scene_index) != R1_OK)
        return R1_EINVAL;
    for (uint32_t i : d.scene_index)
    {
        d.x.push_back(s->center_x[i]), d.y.push_back(s->center_y[i]), d.z.push_back(s->center_z[i]), d.r.push_back(s->radius_sq[i]);
        d.rb.push_back(r1_bound_radius(s->radius_sq[i], s->inv_radius[i]));
    }
    d.na = (uint32_t)d.x.size();
    if (d.na == 0)
        d.x.push_back(0), d.y.push_back(0), d.z.push_back(0), d.r.push_back(0), d.rb.push_back(0);
    r1_build_bvh(d.na, d.x.data(), d.y.data(), d.z.data(), d.r.data(), d.rb.data(),
                 leaf_max > 0 ? leaf_max : (d.na > R1_MAX_ACTIVE_10BIT ? 2 * R1_BVH_LEAF : R1_BVH_LEAF), d.b);
    return R1_OK;
}
static void describe_info(const Described &d, r1_bvh_info *info)
{
    const R1Bvh &b = d.b;
    info->nodes = (int32_t)(b.nodes.size() / 16);
    info->leaves = (int32_t)b.n_leaves;
    info->depth = b.max_depth;
    info->stack_entries = R1_BVH_STACK;
    info->spheres = (int32_t)d.na;
    for (int k = 0; k < 3; ++k)
        info->centre[k] = b.centre[k];
    info->pad_local = b.pad_local;
    info->root_leaf = b.root_leaf;
    info->flat_axis = b.flat_axis, info->flat_m = b.flat_m, info->flat_e = b.flat_e;
    info->pairs = (int32_t)(b.ids.size() / 2);
}

// Host-only pin of the refit (include/rays1.h): the tree of `built`, refitted to the scene-indexed centres x, y, z and, where given, to the
// scene-indexed radii — each pair as the device's set kernel writes it (r1f_radius_rows: a pair that would make the sphere inactive leaves it
// never hittable, radius_sq -inf and radii {0, 0}).
static int refit_describe(const char *who, const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                          const float *inv_radius, int32_t leaf_max, r1_bvh_info *info, float *nodes_out, size_t nodes_cap)
{
    if (!built || !info || !x || !y || !z || !radius_sq != !inv_radius)
    {
        r1_set_error("%s: null argument", who);
        return R1_EINVAL;
    }
    Described d;
    int rc = describe_build(built, leaf_max, d);
    if (rc)
        return rc;
    R1RefitTopo t;
    r1_bvh_topology(d.b, d.na, t);
    for (uint32_t a = 0; a < d.na; ++a)
    {
        const uint32_t i = d.scene_index[a];
        d.x[a] = x[i], d.y[a] = y[i], d.z[a] = z[i];
        if (radius_sq)
        {
            float inv;
            double rr[2];
            r1f_radius_rows(radius_sq[i], inv_radius[i], d.r[a], inv, rr);
            d.rb[a] = rr[0]; // (r1_bvh_refit_host derives the test radius from this and d.r as r1f_radius_rows does)
        }
    }
    r1_bvh_refit_host(d.b, t, d.na, d.x.data(), d.y.data(), d.z.data(), d.r.data(), d.rb.data());
    describe_info(d, info);
    info->flat_axis = -1, info->flat_m = info->flat_e = 0.0f;
    if (nodes_out)
    {
        if (nodes_cap < d.b.nodes.size())
            return R1_ELIMIT;
        memcpy(nodes_out, d.b.nodes.data(), d.b.nodes.size() * 4);
    }
    return R1_OK;
}

extern "C" int r1_bvh_refit_describe(const r1_scene *built, const float *x, const float *y, const float *z, int32_t leaf_max, r1_bvh_info *info,
                                     float *nodes_out, size_t nodes_cap)
{
    return refit_describe("r1_bvh_refit_describe", built, x, y, z, nullptr, nullptr, leaf_max, info, nodes_out, nodes_cap);
}

extern "C" int r1_bvh_refit_describe_spheres(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                                             const float *inv_radius, int32_t leaf_max, r1_bvh_info *info, float *nodes_out, size_t nodes_cap)
{
    return refit_describe("r1_bvh_refit_describe_spheres", built, x, y, z, radius_sq, inv_radius, leaf_max, info, nodes_out, nodes_cap);
}

// Host-only pin of the re-sort (include/rays1.h): the tree of `built`, its movable spheres re-dealt by r1_bvh_sort.h's rule to the scene-indexed
// centres (and radii, taken as refit_describe takes them), then refitted.
extern "C" int r1_bvh_resort_describe(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                                      const float *inv_radius, int32_t leaf_max, r1_bvh_info *info, float *nodes_out, size_t nodes_cap,
                                      uint32_t *ids_out, size_t ids_cap)
{
    if (!built || !info || !x || !y || !z || !radius_sq != !inv_radius)
    {
        r1_set_error("r1_bvh_resort_describe: null argument");
        return R1_EINVAL;
    }
    Described d;
    int rc = describe_build(built, leaf_max, d);
    if (rc)
        return rc;
    R1RefitTopo t;
    R1SortTopo s;
    r1_bvh_topology(d.b, d.na, t);
    r1_bvh_sort_topology(d.b, s);
    for (uint32_t a = 0; a < d.na; ++a)
    {
        const uint32_t i = d.scene_index[a];
        d.x[a] = x[i], d.y[a] = y[i], d.z[a] = z[i];
        if (radius_sq)
        {
            float inv;
            double rr[2];
            r1f_radius_rows(radius_sq[i], inv_radius[i], d.r[a], inv, rr);
            d.rb[a] = rr[0];
        }
    }
    r1_bvh_resort_host(d.b, t, s, d.x.data(), d.y.data(), d.z.data(), d.r.data());
    r1_bvh_refit_host(d.b, t, d.na, d.x.data(), d.y.data(), d.z.data(), d.r.data(), d.rb.data());
    describe_info(d, info);
    info->flat_axis = -1, info->flat_m = info->flat_e = 0.0f;
    if (nodes_out)
    {
        if (nodes_cap < d.b.nodes.size())
            return R1_ELIMIT;
        memcpy(nodes_out, d.b.nodes.data(), d.b.nodes.size() * 4);
    }
    if (ids_out)
    {
        if (ids_cap < d.b.ids.size())
            return R1_ELIMIT;
        for (size_t i = 0; i < d.b.ids.size(); ++i)
            ids_out[i] = d.b.ids[i] == 0xFFFFFFFFu || d.na == 0 ? 0xFFFFFFFFu : d.scene_index[d.b.ids[i]];
    }
    return R1_OK;
}

// Host-only view of the index (include/rays1.h): what r1_set_scene would build for this scene.
extern "C" int r1_bvh_describe(const r1_scene *s, int32_t leaf_max, r1_bvh_info *info, float *nodes_out, size_t nodes_cap, uint32_t *ids_out,
                               size_t ids_cap)
{
    if (!s || !info)
        return R1_EINVAL;
    Described d;
    int rc = describe_build(s, leaf_max, d);
    if (rc)
        return rc;
    const R1Bvh &b = d.b;
    describe_info(d, info);
    if (nodes_out)
    {
        if (nodes_cap < b.nodes.size())
            return R1_ELIMIT;
        memcpy(nodes_out, b.nodes.data(), b.nodes.size() * 4);
    }
    if (ids_out)
    {
        if (ids_cap < b.ids.size())
            return R1_ELIMIT;
        for (size_t i = 0; i < b.ids.size(); ++i) // leaf slot (2 per pair) -> index into the caller's scene arrays
            ids_out[i] = b.ids[i] == 0xFFFFFFFFu || d.na == 0 ? 0xFFFFFFFFu : d.scene_index[b.ids[i]];
    }
    return R1_OK;
}
