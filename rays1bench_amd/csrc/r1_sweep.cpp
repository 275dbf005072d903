// r1_sweep.cpp — host builder of the sweep's tables (R1_VARIANT_PREFILTER, r1_hit_sweep.hpp sweep_prefilter): sphere groups with a conservative
// bounding sphere each, in pair layout, and the per-sphere rows.  Host code only: no HIP call, no context; r1_sweep_describe shows the
// tables to tests/test_sweep_host.py.

#include <math.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "r1_sweep.h"
#include "r1_bvh.h" // r1_active_spheres, r1_bound_radius
#include "r1_device.h"
#include "r1_internal.h"

// largest float <= v, then one more step down (guards the double->float conversion)
static float round_down(double v)
{
    float f = (float)v;
    if ((double)f > v)
        f = nextafterf(f, -INFINITY);
    return nextafterf(f, -INFINITY);
}

// ---- sphere groups (level 1 of the sweep) ------------------------------------------------------
// The sweep tests GROUPS of up to R1_GROUP_MAX nearby spheres against a bounding sphere first and
// re-tests the members of flagged groups exactly (r1_hit_sweep.hpp exact_trips).  Grouping is a pure work
// reduction: every active sphere belongs to exactly one group, the group test is conservative,
// and hits are still resolved per sphere in the reference's arithmetic and index order.
struct R1Group
{
    double gx, gy, gz, radius; // bounding sphere: |c_i - g| + r_i <= radius for every member
    double c_max2;             // max(|g|^2, max_i |c_i|^2): magnitude that scales the fp32 error terms
    uint32_t member[R1_GROUP_MAX];
    int n;
};

static uint64_t spread21(uint64_t v) // 21 bits -> every third bit
{
    v &= 0x1FFFFF;
    v = (v | v << 32) & 0x1F00000000FFFFull;
    v = (v | v << 16) & 0x1F0000FF0000FFull;
    v = (v | v << 8) & 0x100F00F00F00F00Full;
    v = (v | v << 4) & 0x10C30C30C30C30C3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

static void bound_of(const std::vector<uint32_t> &m, const std::vector<double> &x, const std::vector<double> &y,
                     const std::vector<double> &z, const std::vector<double> &r, R1Group &g)
{
    // centre: middle of the members' axis-aligned extent (tight for the 2x2 blocks of a lattice)
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t a : m)
    {
        const double c[3] = {x[a], y[a], z[a]};
        for (int k = 0; k < 3; ++k)
            lo[k] = fmin(lo[k], c[k] - r[a]), hi[k] = fmax(hi[k], c[k] + r[a]);
    }
    g.gx = 0.5 * (lo[0] + hi[0]), g.gy = 0.5 * (lo[1] + hi[1]), g.gz = 0.5 * (lo[2] + hi[2]);
    g.radius = 0;
    g.c_max2 = g.gx * g.gx + g.gy * g.gy + g.gz * g.gz;
    for (uint32_t a : m)
    {
        const double dx = x[a] - g.gx, dy = y[a] - g.gy, dz = z[a] - g.gz;
        g.radius = fmax(g.radius, sqrt(dx * dx + dy * dy + dz * dz) + r[a]);
        g.c_max2 = fmax(g.c_max2, x[a] * x[a] + y[a] * y[a] + z[a] * z[a]);
    }
}

// lone[a]: sphere a must stay a group of its own (its radius_sq and inv_radius disagree, so the
// R <= R1_GROUP_RATIO x r bound of the slack analysis cannot be relied on; a single-sphere group
// needs no such bound: flagged by the reference means dist^2 <= r^2 + E1 <= R^2 + E1)
static std::vector<R1Group> build_groups(uint32_t na, const std::vector<double> &x, const std::vector<double> &y,
                                         const std::vector<double> &z, const std::vector<double> &r, const std::vector<char> &lone)
{
    // Grouping trades level-1 tests for extra member slots in the exact phase: it pays once the
    // sweep is long (large scene: 484 spheres, 1.5x), not for a few dozen spheres (medium scene:
    // 46 spheres, 27.2 vs 24.5 Grays/s ungrouped vs grouped) — R1_GROUP_MAX overrides for tuning.
    static const long gmax_env = (long)r1_knob("R1_GROUP_MAX", 0); // 0: automatic
    const long gmax_want = gmax_env > 0 ? gmax_env : (na > R1_GROUP_MIN_SPHERES ? R1_GROUP_MAX : 1);
    const int gmax = gmax_want > R1_GROUP_MAX ? R1_GROUP_MAX : (int)gmax_want;
    std::vector<R1Group> groups;
    auto close = [&](const std::vector<uint32_t> &m) {
        R1Group g;
        memset(&g, 0, sizeof(g));
        bound_of(m, x, y, z, r, g);
        g.n = (int)m.size();
        for (int k = 0; k < R1_GROUP_MAX; ++k)
            g.member[k] = k < g.n ? m[k] : 0xFFFFFFFFu;
        groups.push_back(g);
    };
    if (na == 0)
        return groups;
    // spheres much larger than the typical one (the ground, the r = 2 balls) stay alone
    std::vector<double> rs(r.begin(), r.begin() + na);
    std::nth_element(rs.begin(), rs.begin() + na / 2, rs.end());
    const double r_med = rs[na / 2];
    std::vector<uint32_t> small;
    for (uint32_t a = 0; a < na; ++a)
        if (gmax > 1 && r[a] <= 2.5 * r_med && !lone[a])
            small.push_back(a);
        else
            close(std::vector<uint32_t>(1, a));
    if (small.empty())
        return groups;
    // Morton order of the centres, then greedy runs of <= gmax spheres whose bounding sphere
    // stays within R1_GROUP_RATIO x the smallest member radius (keeps the bound selective and the
    // slack analysis of DESIGN.md §4.1 valid)
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t a : small)
    {
        lo[0] = fmin(lo[0], x[a]), hi[0] = fmax(hi[0], x[a]);
        lo[1] = fmin(lo[1], y[a]), hi[1] = fmax(hi[1], y[a]);
        lo[2] = fmin(lo[2], z[a]), hi[2] = fmax(hi[2], z[a]);
    }
    const double ext = fmax(fmax(hi[0] - lo[0], hi[1] - lo[1]), fmax(hi[2] - lo[2], 1e-30));
    std::vector<std::pair<uint64_t, uint32_t>> keyed;
    for (uint32_t a : small)
    {
        const uint64_t qx = (uint64_t)((x[a] - lo[0]) / ext * 2097151.0), qy = (uint64_t)((y[a] - lo[1]) / ext * 2097151.0),
                       qz = (uint64_t)((z[a] - lo[2]) / ext * 2097151.0);
        keyed.push_back({spread21(qx) | spread21(qy) << 1 | spread21(qz) << 2, a});
    }
    std::sort(keyed.begin(), keyed.end());
    std::vector<uint32_t> cur;
    for (auto &ka : keyed)
    {
        std::vector<uint32_t> tryg = cur;
        tryg.push_back(ka.second);
        bool ok = (int)tryg.size() <= gmax;
        if (ok && tryg.size() > 1)
        {
            R1Group g;
            bound_of(tryg, x, y, z, r, g);
            double rmin = 1e300;
            for (uint32_t a : tryg)
                rmin = fmin(rmin, r[a]);
            static const double ratio = r1_knob_f("R1_GROUP_RATIO", R1_GROUP_RATIO);
            ok = g.radius <= (ratio < R1_GROUP_RATIO ? ratio : R1_GROUP_RATIO) * rmin; // the slack analysis needs <= R1_GROUP_RATIO
        }
        if (ok)
            cur = tryg;
        else
        {
            close(cur);
            cur.assign(1, ka.second);
        }
    }
    if (!cur.empty())
        close(cur);
    return groups;
}

void r1_build_sweep(const r1_scene *s, const std::vector<uint32_t> &active_to_scene, R1Sweep &out)
{
    const uint32_t na = (uint32_t)active_to_scene.size();
    // level 1 of the sweep: groups of nearby spheres with a bounding sphere each
    std::vector<double> ax(na ? na : 1), ay(na ? na : 1), az(na ? na : 1);
    std::vector<double> &ar_ = out.rbound;
    ar_.assign(na ? na : 1, 0.0);
    std::vector<char> lone(na ? na : 1, 0);
    for (uint32_t a = 0; a < na; ++a)
    {
        const uint32_t i = active_to_scene[a];
        ax[a] = s->center_x[i], ay[a] = s->center_y[i], az[a] = s->center_z[i];
        ar_[a] = r1_bound_radius(s->radius_sq[i], s->inv_radius[i]); // what the exact test can accept, never less
        const double r_test = s->radius_sq[i] > 0 ? sqrt((double)s->radius_sq[i]) : 0.0;
        lone[a] = !(r_test >= ar_[a] * (1.0 - 1e-3)); // SphereSOA::add keeps them within 2 ulp (soa_sphere.cpp:70-85)
    }
    std::vector<R1Group> groups = build_groups(na, ax, ay, az, ar_, lone);
    // multi-member groups first: a flagged group with id >= n_multi is a single sphere and takes
    // one member slot of the exact phase instead of R1_GROUP_MAX
    std::stable_partition(groups.begin(), groups.end(), [](const R1Group &g) { return g.n > 1; });
    const uint32_t ng = (uint32_t)groups.size();
    uint32_t n_multi = 0;
    while (n_multi < ng && groups[n_multi].n > 1)
        ++n_multi;

    // small scenes: whole 8-group chunks + one prefetch chunk; big scenes: whole LDS tiles + one
    // prefetch tile
    const bool big_scene = na > R1_MAX_ACTIVE_10BIT;
    const uint32_t ns = big_scene ? ((ng + R1_TILE_SPHERES - 1) / R1_TILE_SPHERES) * R1_TILE_SPHERES : ((ng + 7u) & ~7u);

    // sweep table: pair layout + one chunk of prefetch padding (see r1_device.h)
    const uint32_t ns_alloc = ns + (big_scene ? R1_TILE_SPHERES : 8);
    std::vector<float> &sweep = out.sweep, &exact = out.exact, &shade = out.shade, &mat = out.mat;
    sweep.assign(4 * (size_t)ns_alloc, 0.0f), exact.assign(4 * (size_t)(na ? na : 1), 0.0f);
    shade.assign(4 * (size_t)(na > R1_MAX_ACTIVE_10BIT ? na : R1_MAX_ACTIVE_10BIT + 1), 0.0f); // small scenes: any 10-bit index may be read (unwind)
    // small scenes: row R1_MAX_ACTIVE_10BIT — the one 10-bit index no sphere has — is the identity {0, 1, 1, 1}: what the empty slots of an
    // attenuation word point at (r1_stack_words.h).  No update touches it: r1_update_spheres* write the rows of active spheres alone.
    if (na <= R1_MAX_ACTIVE_10BIT)
        shade[4 * (size_t)R1_MAX_ACTIVE_10BIT + 1] = shade[4 * (size_t)R1_MAX_ACTIVE_10BIT + 2] = shade[4 * (size_t)R1_MAX_ACTIVE_10BIT + 3] = 1.0f;
    mat.assign(4 * (size_t)(na ? na : 1), 0.0f);
    std::vector<uint32_t> &members = out.members;
    members.assign((size_t)R1_GROUP_MAX * ns_alloc, 0xFFFFFFFFu);
    out.cover.assign(ng, 0.0), out.rule.assign(ng, 0.0), out.c_max2.assign(ng, 0.0);
    auto sweep_slot = [&](uint32_t a, int comp) -> float & { return sweep[8 * (size_t)(a >> 1) + 2 * comp + (a & 1)]; };
    for (uint32_t a = 0; a < ns_alloc; ++a) // never-candidate default
        sweep_slot(a, 0) = sweep_slot(a, 1) = sweep_slot(a, 2) = 0, sweep_slot(a, 3) = INFINITY;
    for (uint32_t g = 0; g < ng; ++g)
    {
        const R1Group &G = groups[g];
        // the bounding sphere as fp32 centre + a radius that still covers the members after the
        // centre is rounded to fp32
        const float gx = (float)G.gx, gy = (float)G.gy, gz = (float)G.gz;
        double R = 0;
        for (int k = 0; k < G.n; ++k)
        {
            const uint32_t a = G.member[k];
            const double dx = ax[a] - gx, dy = ay[a] - gy, dz = az[a] - gz;
            R = fmax(R, sqrt(dx * dx + dy * dy + dz * dz) + ar_[a]);
            members[(size_t)R1_GROUP_MAX * g + k] = a;
        }
        R *= 1.0 + 1e-12;
        const double g2 = (double)gx * gx + (double)gy * gy + (double)gz * gz;
        // Kp = (|g|^2 - R^2) - 2^-15 (C^2 + R^2), rounded down.  C^2 bounds |g|^2 and every
        // member's |c|^2.  The slack covers the fp32 error of the group test itself AND of any
        // member's reference test carried over to the bound: see sweep_prefilter.
        const double kp = (g2 - R * R) - ldexp(fmax(G.c_max2, g2) + R * R, -15) - 1e-30;
        sweep_slot(g, 0) = gx, sweep_slot(g, 1) = gy, sweep_slot(g, 2) = gz, sweep_slot(g, 3) = round_down(kp);
        out.cover[g] = R, out.rule[g] = G.radius, out.c_max2[g] = G.c_max2;
    }
    for (uint32_t a = 0; a < na; ++a)
    {
        const uint32_t i = active_to_scene[a];
        const float cx = s->center_x[i], cy = s->center_y[i], cz = s->center_z[i], rsq = s->radius_sq[i];
        exact[4 * a + 0] = cx, exact[4 * a + 1] = cy, exact[4 * a + 2] = cz, exact[4 * a + 3] = rsq;
        shade[4 * a + 0] = s->inv_radius[i], shade[4 * a + 1] = s->albedo_r[i], shade[4 * a + 2] = s->albedo_g[i],
                      shade[4 * a + 3] = s->albedo_b[i];
        // the material's row, dielectric constants included: r1_bvh_fill.h, the arithmetic r1_update_spheres* runs on the device too
        r1f_material_row(s->mat_type[i], s->mat_param[i], &mat[4 * a]);
    }

    // the members' spheres once more, in group order (exact_trips fetches sphere and index side by side)
    std::vector<float> &exact_g = out.exact_g;
    exact_g.assign(4 * (size_t)R1_GROUP_MAX * ns_alloc, 0.0f);
    for (size_t k = 0; k < (size_t)R1_GROUP_MAX * ns_alloc; ++k)
    {
        const uint32_t a = members[k];
        for (int q = 0; q < 4; ++q)
            exact_g[4 * k + q] = a != 0xFFFFFFFFu ? exact[4 * (size_t)a + q] : (q == 3 ? -INFINITY : 0.0f);
    }
    out.n_groups = ng, out.n_multi = n_multi, out.n_sweep = ns;
}

// internal (tests/test_sweep_host.py): the tables r1_set_scene would build for s.  Every buffer may be NULL; one that is given and too
// short: R1_ELIMIT.  groups_out: per group {centre x, y, z (the stored fp32 values), stored Kp, R, the radius the R1_GROUP_RATIO rule
// saw, c_max2, n}; members_out: active indices (active_out maps them to scene indices).
extern "C" int r1_sweep_describe(const r1_scene *s, r1_sweep_info *info, double *groups_out, size_t groups_cap, float *sweep_out, size_t sweep_cap,
                                 uint32_t *members_out, size_t members_cap, float *exact_g_out, size_t exact_g_cap, uint32_t *active_out,
                                 size_t active_cap)
{
    if (!s || !info || !s->center_x || !s->center_y || !s->center_z || !s->radius_sq || !s->inv_radius || !s->mat_type || !s->albedo_r ||
        !s->albedo_g || !s->albedo_b || !s->mat_param)
        return R1_EINVAL;
    std::vector<uint32_t> active;
    if (r1_active_spheres(s, active) != R1_OK)
        return R1_EINVAL;
    R1Sweep t;
    r1_build_sweep(s, active, t);
    memset(info, 0, sizeof(*info));
    info->spheres = (int32_t)active.size();
    info->groups = (int32_t)t.n_groups, info->multi = (int32_t)t.n_multi, info->n_sweep = (int32_t)t.n_sweep;
    info->slots = (int32_t)(t.members.size() / R1_GROUP_MAX);
    info->group_max = R1_GROUP_MAX;
    if (groups_out)
    {
        if (groups_cap < 8 * (size_t)t.n_groups)
            return R1_ELIMIT;
        for (uint32_t g = 0; g < t.n_groups; ++g)
        {
            double *o = groups_out + 8 * (size_t)g;
            for (int comp = 0; comp < 4; ++comp)
                o[comp] = t.sweep[8 * (size_t)(g >> 1) + 2 * comp + (g & 1)];
            o[4] = t.cover[g], o[5] = t.rule[g], o[6] = t.c_max2[g];
            int n = 0;
            while (n < R1_GROUP_MAX && t.members[(size_t)R1_GROUP_MAX * g + n] != 0xFFFFFFFFu)
                ++n;
            o[7] = n;
        }
    }
    if (sweep_out)
    {
        if (sweep_cap < t.sweep.size())
            return R1_ELIMIT;
        memcpy(sweep_out, t.sweep.data(), t.sweep.size() * 4);
    }
    if (members_out)
    {
        if (members_cap < t.members.size())
            return R1_ELIMIT;
        memcpy(members_out, t.members.data(), t.members.size() * 4);
    }
    if (exact_g_out)
    {
        if (exact_g_cap < t.exact_g.size())
            return R1_ELIMIT;
        memcpy(exact_g_out, t.exact_g.data(), t.exact_g.size() * 4);
    }
    if (active_out)
    {
        if (active_cap < active.size())
            return R1_ELIMIT;
        if (!active.empty())
            memcpy(active_out, active.data(), active.size() * 4);
    }
    return R1_OK;
}
