// r1_bvh_fill.h — the arithmetic that turns sphere bounds into the box tree's node rows, shared by the host builder (r1_bvh.cpp) and the
// device refit (r1_refit.hip).  r1_bvh.cpp's header has the formulas and their proofs; they hold for any fixed point C and any eps > 0, so the
// tree's constants — centre, pad_local, d_typ: fixed when the tree is built — serve every later position of the spheres.
//
// Everything here is correctly rounded fp64 + - * / sqrt, comparisons and selects, and conversions to and from fp32 (the Makefile's
// -ffp-contract=off holds for host and device code): the host and the device compute the same bits from the same inputs.  No library call
// whose rounding could differ between the two: min / max / abs are spelled as selects, the step to the next float is integer arithmetic.
#ifndef R1_BVH_FILL_H
#define R1_BVH_FILL_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define R1F_HD __host__ __device__ inline
#else
#define R1F_HD inline
#endif

R1F_HD double r1f_min(double a, double b) { return b < a ? b : a; } // std::min
R1F_HD double r1f_max(double a, double b) { return a < b ? b : a; } // std::max
R1F_HD double r1f_abs(double a) { return __builtin_fabs(a); }
R1F_HD bool r1f_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e38f; } // false for NaN and +-inf

// nextafterf(f, +inf)
R1F_HD float r1f_next_up(float f)
{
    if (f != f || f == __builtin_inff())
        return f;
    if (f == 0.0f)
        return __builtin_bit_cast(float, (uint32_t)1u);
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return __builtin_bit_cast(float, f > 0.0f ? b + 1u : b - 1u);
}

// smallest float >= v, then one more step up (guards the double->float conversion)
R1F_HD float r1f_round_up(double v)
{
    float f = (float)v;
    if ((double)f < v)
        f = r1f_next_up(f);
    return r1f_next_up(f);
}

// ---- what the builders derive per sphere from the caller's arrays (r1_bvh.cpp r1_bound_radius / r1_test_radius, r1_sweep.cpp's material rows):
// here so that the device derives the same bits when a sphere's radius or material changes in place (r1_refit.hip) ----

// Radius every conservative bound must cover: the larger of sqrt(radius_sq) and 1 / |inv_radius| (r1_bvh.cpp r1_bound_radius has the why)
R1F_HD double r1f_bound_radius(float radius_sq, float inv_radius)
{
    const double from_sq = radius_sq > 0 ? __builtin_sqrt((double)radius_sq) : 0.0;
    const double from_inv = r1f_finite(inv_radius) && inv_radius != 0 ? 1.0 / r1f_abs((double)inv_radius) : 0.0;
    return r1f_max(from_sq, from_inv);
}

// The radius whose error terms the pad follows: sqrt(radius_sq), never more than the bound radius (r1f_sphere_box's r_test)
R1F_HD double r1f_test_radius(double rbound, float radius_sq) { return radius_sq > 0 ? r1f_min(rbound, __builtin_sqrt((double)radius_sq)) : 0.0; }

// Would r1_active_spheres keep a sphere of this pair?  inv_radius != 0 (rayweek1.cpp:291) and not NaN, radius_sq finite.
R1F_HD bool r1f_hittable_radius(float radius_sq, float inv_radius) { return inv_radius == inv_radius && inv_radius != 0 && r1f_finite(radius_sq); }

// A new {radius_sq, inv_radius} of an active sphere, as every table holds it: rsq (exact[a].w and the sphere's word of its leaf pair), inv
// (shade[a].x) and radii {bound, test}.  A pair r1_active_spheres would drop makes the sphere never hittable in place: radius_sq = -inf as the
// partner of an odd sphere has it (the exact test's discriminant is -inf), radii {0, 0}.
R1F_HD void r1f_radius_rows(float radius_sq, float inv_radius, float &rsq, float &inv, double radii[2])
{
    if (!r1f_hittable_radius(radius_sq, inv_radius))
    {
        rsq = -__builtin_inff(), inv = 0.0f, radii[0] = radii[1] = 0.0;
        return;
    }
    rsq = radius_sq, inv = inv_radius;
    radii[0] = r1f_bound_radius(radius_sq, inv_radius);
    radii[1] = r1f_test_radius(radii[0], radius_sq);
}

// A material's row {type, param, 1 / ref_idx, schlick r0}: the dielectric constants the reference recomputes per hit with IEEE fp32 operations
// (rayweek1.cpp:489 `1.0f / _refIdx`, :456-457 schlick r0), the same operations in the same order, done once.  Both need a correctly rounded
// fp32 divide that keeps denormals (the Makefile's -fhip-fp32-correctly-rounded-divide-sqrt on the device; DESIGN.md §4.27 has the check).
R1F_HD void r1f_material_row(uint32_t type, float param, float row[4])
{
    const float ref_idx = param;
    float r0 = (1 - ref_idx) / (1 + ref_idx);
    r0 = r0 * r0;
    row[0] = __builtin_bit_cast(float, type);
    row[1] = ref_idx;
    row[2] = type == 2u /* R1_MAT_DIELECTRIC */ ? 1.0f / ref_idx : 0.0f;
    row[3] = type == 2u ? r0 : 0.0f;
}

struct R1Box
{
    double lo[3], hi[3];   // of the spheres' extents c +- r
    double clo[3], chi[3]; // of the centres
    double kmax;           // max 1 / (2 r_eff)
    double rmax;           // max r
    double floor_pad;      // max r_floor / 2 over degenerate members
    R1F_HD void clear()
    {
        for (int a = 0; a < 3; ++a)
            lo[a] = clo[a] = 1e300, hi[a] = chi[a] = -1e300;
        kmax = rmax = floor_pad = 0;
    }
    R1F_HD void zero() // the box of a tree without spheres
    {
        for (int a = 0; a < 3; ++a)
            lo[a] = clo[a] = hi[a] = chi[a] = 0;
        kmax = rmax = floor_pad = 0;
    }
    R1F_HD bool empty() const { return lo[0] > hi[0]; } // nothing merged since clear()
    R1F_HD void merge(const R1Box &b)
    {
        for (int a = 0; a < 3; ++a)
        {
            lo[a] = r1f_min(lo[a], b.lo[a]), hi[a] = r1f_max(hi[a], b.hi[a]);
            clo[a] = r1f_min(clo[a], b.clo[a]), chi[a] = r1f_max(chi[a], b.chi[a]);
        }
        kmax = r1f_max(kmax, b.kmax), rmax = r1f_max(rmax, b.rmax), floor_pad = r1f_max(floor_pad, b.floor_pad);
    }
    R1F_HD double area() const
    {
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    }
};

// One sphere's box.  c: the fp32 centre the exact test reads; r: the radius the boxes must cover (r1_bound_radius, >= the radius the exact test
// reads); r_test: the radius the test itself uses, min(r, sqrt(radius_sq)) or 0 — the error terms E1 / (2 r) follow this smaller, safer one.
R1F_HD void r1f_sphere_box(float cx, float cy, float cz, double r, double r_test, R1Box &s)
{
    const double c[3] = {cx, cy, cz};
    // degenerate radii: bound sqrt(r^2 + E1) - r through r_floor (AM-GM), see r1_bvh.cpp
    const double r_floor = 1e-4 * (1.0 + r1f_abs(c[0]) + r1f_abs(c[1]) + r1f_abs(c[2]));
    const double r_eff = r1f_max(r_test, r_floor);
    for (int k = 0; k < 3; ++k)
        s.lo[k] = c[k] - r, s.hi[k] = c[k] + r, s.clo[k] = s.chi[k] = c[k];
    s.kmax = 1.0 / (2.0 * r_eff);
    s.rmax = r;
    s.floor_pad = r_test < r_floor ? 0.5 * r_floor : 0.0;
}

// The constants of a tree's pad formula, fixed when the tree is built
struct R1FillConst
{
    double centre[3]; // C: exactly the fp32 values the kernel subtracts
    double d_typ;     // pad_local: the distance at which the per-node pad is tight (twice the median distance of the centres from C at build time)
    int pad_local;    // 1: pad measured per node (scenes of small spheres), 0: from `centre`
    int child_k;      // 1 (always, outside tuning experiments): each child carries its own K
};

// child box -> {m, e} in fp32 covering [lo, hi], and this child's (w2, k)
R1F_HD void r1f_encode(const R1Box &bx, float m[3], float e[3], double &w2, double &k)
{
    double h2 = 0;
    for (int a = 0; a < 3; ++a)
    {
        m[a] = (float)(0.5 * (bx.lo[a] + bx.hi[a]));
        e[a] = r1f_round_up(r1f_max(bx.hi[a] - (double)m[a], (double)m[a] - bx.lo[a]));
        const double hc = r1f_max(r1f_abs(bx.clo[a] - (double)m[a]), r1f_abs(bx.chi[a] - (double)m[a]));
        h2 += hc * hc;
    }
    const double u = 0x1p-24;
    w2 = 2.0 * (40.0 * u * bx.kmax) + 0x1p-19;
    k = w2 * h2 + 0x1p-20 + 4.0 * u * bx.rmax + bx.floor_pad;
}

// Words 0..13 of a node's row, {m0x m1x m0y m1y} {m0z m1z e0x e1x} {e0y e1y e0z e1z} {A K . .}, from its two children's boxes; the child
// references (words 14, 15) are the caller's.
// pad = A |o - C|^2 + K, or A |m0 + m1 - 2 o|^2 + K (r1_bvh.cpp's header): >= w2 |m - o|^2 + k for both children
R1F_HD void r1f_fill(const R1FillConst &T, const R1Box &b0, const R1Box &b1, float *p)
{
    float m0[3], e0[3], m1[3], e1[3];
    double w0, k0, w1, k1;
    r1f_encode(b0, m0, e0, w0, k0);
    r1f_encode(b1, m1, e1, w1, k1);
    const double u = 0x1p-24, w2 = r1f_max(w0, w1), k = r1f_max(k0, k1);
    const double head = 1.0 + 0x1p-18;
    float A, K;
    if (!T.pad_local)
    {
        const double c1n = r1f_abs(T.centre[0]) + r1f_abs(T.centre[1]) + r1f_abs(T.centre[2]);
        double g2c[2], kc[2] = {k0, k1}, wc[2] = {w0, w1};
        for (int j = 0; j < 2; ++j)
        {
            const float *m = j ? m1 : m0;
            double q = 0;
            for (int a = 0; a < 3; ++a)
                q += ((double)m[a] - T.centre[a]) * ((double)m[a] - T.centre[a]);
            g2c[j] = q;
        }
        if (!T.child_k)
            g2c[0] = g2c[1] = r1f_max(g2c[0], g2c[1]), kc[0] = kc[1] = k, wc[0] = wc[1] = w2;
        A = r1f_round_up((2.0 * w2 + u) * head), K = 0.0f;
        // K folded into the half extents here, e' = e + K rounded up, each child its own (see r1_build_bvh: "ONE A for the whole tree")
        for (int j = 0; j < 2; ++j)
        {
            float *e = j ? e1 : e0;
            const float Kc = r1f_round_up((kc[j] + 2.0 * wc[j] * g2c[j] + u * (1.0 + c1n)) * head);
            for (int a = 0; a < 3; ++a)
                e[a] = r1f_round_up((double)e[a] + (double)Kc);
        }
    }
    else
    {
        double g2 = 0, mn2 = 0, M = 0, M0 = 0, M1 = 0;
        for (int a = 0; a < 3; ++a)
        {
            const double h = 0.5 * ((double)m0[a] - (double)m1[a]), mn = 0.5 * ((double)m0[a] + (double)m1[a]);
            g2 += h * h, mn2 += mn * mn;
            M0 = r1f_max(M0, r1f_abs((double)m0[a])), M1 = r1f_max(M1, r1f_abs((double)m1[a]));
        }
        M = M0 + M1;
        // (D + g)^2 <= (1 + eps) D^2 + (1 + 1 / eps) g^2 for every eps > 0: tight at D = g / eps.  eps = g / d_typ makes the
        // pad exact for origins d_typ away (the scene's scale), instead of twice what is needed (eps = 1) everywhere
        const double eps = r1f_min(1.0, r1f_max(1.0 / 64.0, __builtin_sqrt(g2) / T.d_typ));
        const double a_loc = (0.25 * (1.0 + eps) * w2 + u / 8.0) * (1.0 + 0x1p-10);
        A = r1f_round_up(a_loc * head);
        K = r1f_round_up((k + (1.0 + 1.0 / eps) * w2 * g2 + u * (0.5 + __builtin_sqrt(mn2)) + a_loc * 3075.0 * 288.0 * u * u * M * M) * head);
    }
    p[0] = m0[0], p[1] = m1[0], p[2] = m0[1], p[3] = m1[1];
    p[4] = m0[2], p[5] = m1[2], p[6] = e0[0], p[7] = e1[0];
    p[8] = e0[1], p[9] = e1[1], p[10] = e0[2], p[11] = e1[2];
    p[12] = A, p[13] = K;
}

// The refit's form of r1f_fill: a child without a sphere in it — an empty leaf (the second child of the root of a tree of <= leaf_max
// spheres), or a subtree whose spheres all have non-finite centres — never passes: half extents -inf; its centre and its share of the pad
// are its sibling's, as the builder writes a one-child root.  Both children empty: the box of a tree without spheres (all zero).
R1F_HD void r1f_fill_refit(const R1FillConst &T, const R1Box &b0, const R1Box &b1, float *p)
{
    const bool n0 = b0.empty(), n1 = b1.empty();
    if (!n0 && !n1)
    {
        r1f_fill(T, b0, b1, p);
        return;
    }
    R1Box z;
    z.zero();
    const R1Box &only = n0 ? (n1 ? z : b1) : b0;
    r1f_fill(T, only, only, p);
    const float ninf = -__builtin_inff();
    if (n0)
        p[6] = p[8] = p[10] = ninf;
    if (n1)
        p[7] = p[9] = p[11] = ninf;
}

// ---- the refit's steps, one call per leaf / per node: the device kernels (r1_refit.hip) and the host restatement (r1_bvh_refit_host) run
// these same functions over the same tables (R1RefitTopo, r1_bvh.h) ----

// A leaf's box from its spheres' current centres.  ref: the leaf's child reference; ids: the tree's leaf slots (2 per pair, active indices);
// exact: [active][4] {cx cy cz radius_sq}; radii: [active][2] {bound radius, test radius}.  A sphere with a non-finite centre can never be
// hit and is in no box.
R1F_HD void r1f_refit_leaf(uint32_t ref, const uint32_t *ids, const float *exact, const double *radii, R1Box &bx)
{
    const uint32_t first = ref & 0x0FFFFFFFu, pairs = (ref >> 28) & 7u;
    bx.clear();
    for (uint32_t q = 2u * first; q < 2u * (first + pairs); ++q)
    {
        const uint32_t a = ids[q];
        if (a == 0xFFFFFFFFu)
            continue;
        const float cx = exact[4 * (size_t)a + 0], cy = exact[4 * (size_t)a + 1], cz = exact[4 * (size_t)a + 2];
        if (!r1f_finite(cx) || !r1f_finite(cy) || !r1f_finite(cz))
            continue;
        R1Box s;
        r1f_sphere_box(cx, cy, cz, radii[2 * (size_t)a + 0], radii[2 * (size_t)a + 1], s);
        bx.merge(s);
    }
}

// Node n's row (words 0..13) from its children's boxes, and its own box for its parent.  child_box: [2 x nodes] scratch entry of each child
// (0xFFFFFFFF: an empty leaf); box: the scratch (entries of all children of n are final).  Returns the row's A.
R1F_HD float r1f_refit_node(const R1FillConst &T, uint32_t n, const uint32_t *child_box, R1Box *box, float *nodes)
{
    R1Box b0, b1;
    const uint32_t i0 = child_box[2 * (size_t)n + 0], i1 = child_box[2 * (size_t)n + 1];
    if (i0 != 0xFFFFFFFFu)
        b0 = box[i0];
    else
        b0.clear();
    if (i1 != 0xFFFFFFFFu)
        b1 = box[i1];
    else
        b1.clear();
    float row[14];
    r1f_fill_refit(T, b0, b1, row);
    float *p = nodes + 16 * (size_t)n;
    for (int k = 0; k < 14; ++k)
        p[k] = row[k];
    b0.merge(b1);
    box[n] = b0;
    return row[12];
}

// What the refit kernels read and write (r1_refit.hip), device memory; by value in their arguments
struct R1RefitArgs
{
    float *exact;                    // [active][4] {cx cy cz radius_sq}: the move writes xyz
    float *prims;                    // the tree's leaf spheres, 8 floats per pair {cx_a cx_b cy_a cy_b cz_a cz_b rsq_a rsq_b}: the move writes the centre
    float *nodes;                    // [nodes][16]: words 0..13 are rewritten, the child references stay
    const uint32_t *ids;             // the tree's leaf slots, 2 per pair: active indices
    const uint32_t *scene_to_active; // [spheres of the scene] 0xFFFFFFFF: not active
    const uint32_t *slot;            // [active] the sphere's slot in ids / prims
    const double *radii;             // [active][2] {bound radius, test radius}
    const uint32_t *leaf_ref;        // [leaves]
    const uint32_t *child_box;       // [2 x nodes]
    const uint32_t *by_height;       // [nodes]
    R1Box *box;                      // [nodes + leaves] scratch
    uint32_t *a_max;                 // the largest A of the refitted rows, as the bits of a positive float
    uint32_t n_nodes, n_leaves;
    R1FillConst fill;
};

// What r1_refit_set_kernel reads and writes besides (r1_update_spheres*): the scene's shading rows and the refit's radii, and the caller's
// arrays of the range (device-readable memory, entry i belongs to scene index first + i; a group that is not written: null)
struct R1SetArgs
{
    float *shade;  // [active][4] {inv_radius, albedo r, g, b}
    float *mat;    // [active][4] {type, param, 1 / ref_idx, schlick r0}
    double *radii; // [active][2]: R1RefitArgs::radii, writable
    const float *radius_sq, *inv_radius;
    const uint8_t *mat_type;
    const float *albedo_r, *albedo_g, *albedo_b, *mat_param;
};
#define R1_SET_RADII 1u
#define R1_SET_MATERIALS 2u

#endif
