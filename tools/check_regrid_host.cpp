// tools/check_regrid_host.cpp — the host regrid driven directly, a stand-alone program: r1_build_grid, r1_grid_plan and
// r1_grid_regrid_host on clouds of its own making, among them what no scene reaches through r1_grid_regrid_describe:
//
//   check_regrid_host outliers   every sphere an outlier (thrown out of the box, then blown up beyond `big`): no registrations, v2 = inf,
//                                a zero far box, the plan's geometry kept
//   check_regrid_host touch      a ball on the box face: the last fp32 centre whose ball ends inside the box is registered, the next one
//                                up is an outlier, and the tables of the first hold what exactness needs
//   check_regrid_host zeros      centres of -0.0 and +0.0 give the same tables and the same geometry as values (the far box of centres keeps
//                                the sign of a zero it holds, as the builder's does: r1g_far subtracts it, no comparison reads the sign)
//   check_regrid_host twice      a regrid to B after a regrid to A equals a regrid straight to B, and one more to B changes no byte
//
// tests/test_regrid_host.py builds it with g++ against r1_grid.cpp and r1_bvh.cpp, the host sources it drives, and runs all four.  It is
// also the program for -fsanitize=address,undefined (host code only, no GPU, no library loaded into another process):
//     clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//         -I<hip include dir> tools/check_regrid_host.cpp rays1bench_amd/csrc/r1_grid.cpp rays1bench_amd/csrc/r1_bvh.cpp -o check_regrid_host_asan
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../rays1bench_amd/csrc/r1_grid.h"
#include "../rays1bench_amd/csrc/r1_grid_fill.h"
#include "../rays1bench_amd/csrc/r1_internal.h"

double r1_bound_radius(float radius_sq, float inv_radius); // r1_bvh.cpp

// (the library's error text lives in r1_capi.cpp, next to the HIP runtime: this program links the grid's host sources only)
void r1_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

#define NEED(c)                                                \
    do                                                         \
    {                                                          \
        if (!(c))                                              \
        {                                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
            return 1;                                          \
        }                                                      \
    } while (0)

static uint32_t lcg_state = 4321u;
static float lcg() // [0, 1)
{
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (float)(lcg_state >> 8) * (1.0f / 16777216.0f);
}

// a cloud in active order: the builder's arrays and the device's rows
struct Cloud
{
    std::vector<float> x, y, z, rsq, exact;
    std::vector<double> rb, radii;
    uint32_t n = 0;
    void add(float cx, float cy, float cz, float r)
    {
        x.push_back(cx), y.push_back(cy), z.push_back(cz), rsq.push_back(r * r), rb.push_back(r1_bound_radius(r * r, 1.0f / r)), ++n;
    }
    void rows() // exact [n][4], radii [n][2], as r1_set_scene and the set kernel write them
    {
        exact.assign(4 * (size_t)n + 4, 0.0f), radii.assign(2 * (size_t)n + 2, 0.0);
        for (uint32_t i = 0; i < n; ++i)
        {
            exact[4 * i] = x[i], exact[4 * i + 1] = y[i], exact[4 * i + 2] = z[i], exact[4 * i + 3] = rsq[i];
            radii[2 * i] = rb[i], radii[2 * i + 1] = r1f_test_radius(rb[i], rsq[i]);
        }
    }
};

// a jittered lattice of nx x nz small spheres in the plane y = 0.2 and a ground sphere: the shape of the reference's large scene
static Cloud lattice(int nx, int nz)
{
    Cloud c;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < nx; ++j)
        {
            const float dx = 0.6f * lcg(), dz = 0.6f * lcg();
            c.add(1.1f * (float)j + dx, 0.2f, 1.1f * (float)k + dz, 0.2f);
        }
    c.add(0.0f, -1000.0f, 0.0f, 1000.0f);
    c.rows();
    return c;
}

static bool same_grid(const R1Grid &a, const R1Grid &b)
{
    return memcmp(&a.geom, &b.geom, sizeof(a.geom)) == 0 && a.start == b.start && a.ids == b.ids && a.outliers == b.outliers &&
           a.max_occupancy == b.max_occupancy && memcmp(&a.pad, &b.pad, 8) == 0;
}

// what exactness needs of regridded tables (r1_grid.cpp's argument): every registered ball inside the box, the box inside [-M, M] (up to
// the float roundings r1gf_stretch names), ids ascending per cell, every finite sphere in exactly one list, the far box = the registered centres'
static int check_tables(const R1GridPlan &P, const Cloud &c, const R1Grid &g)
{
    const size_t ncells = (size_t)g.geom.n[0] * g.geom.n[1] * g.geom.n[2];
    NEED(g.start.size() == ncells + 1 && g.start[0] == 0 && g.start[ncells] == g.ids.size());
    std::vector<int> seen(c.n, 0);
    for (size_t q = 0; q < ncells; ++q)
        for (uint32_t k = g.start[q]; k < g.start[q + 1]; ++k)
        {
            NEED(g.ids[k] < c.n && (k == g.start[q] || g.ids[k - 1] < g.ids[k]));
            seen[g.ids[k]] |= 1;
        }
    for (size_t k = 0; k < g.outliers.size(); ++k)
    {
        NEED(g.outliers[k] < c.n && (k == 0 || g.outliers[k - 1] < g.outliers[k]));
        seen[g.outliers[k]] |= 2;
    }
    double clo[3] = {1e300, 1e300, 1e300}, chi[3] = {-1e300, -1e300, -1e300};
    bool any = false;
    for (uint32_t i = 0; i < c.n; ++i)
    {
        const float *e = &c.exact[4 * (size_t)i];
        const bool finite = r1f_finite(e[0]) && r1f_finite(e[1]) && r1f_finite(e[2]);
        NEED(seen[i] == (finite ? (seen[i] & 1 ? 1 : 2) : 0));
        if (seen[i] != 1)
            continue;
        any = true;
        const double rho = r1gf_rho(e[0], e[1], e[2], c.radii[2 * (size_t)i + 1], P.V, P.delta);
        for (int a = 0; a < 3; ++a)
        {
            const double lo = g.geom.lo[a], hi = (double)g.geom.lo[a] + g.geom.n[a] * (double)g.geom.cell[a];
            NEED((double)e[a] - rho >= lo && (double)e[a] + rho <= hi);
            NEED(fabs(lo) <= P.M * (1.0 + 0x1p-22) && fabs(hi) <= P.M * (1.0 + 0x1p-22));
            clo[a] = std::min(clo[a], (double)e[a]), chi[a] = std::max(chi[a], (double)e[a]);
        }
    }
    for (int a = 0; a < 3; ++a)
        NEED(g.geom.clo[a] == (any ? (float)clo[a] : 0.0f) && g.geom.chi[a] == (any ? (float)chi[a] : 0.0f));
    NEED(any ? g.geom.v2 == P.v2 : g.geom.v2 == INFINITY);
    return 0;
}

static int build(const Cloud &c, R1Grid &g, R1GridPlan &P)
{
    r1_build_grid(c.n, c.x.data(), c.y.data(), c.z.data(), c.rsq.data(), c.rb.data(), g);
    r1_grid_plan(g, P);
    // the scene's own rows reproduce the builder
    R1Grid again;
    NEED(!r1_grid_regrid_host(P, c.n, c.exact.data(), c.radii.data(), again));
    NEED(same_grid(g, again));
    return 0;
}

static int run_outliers()
{
    Cloud c = lattice(12, 9);
    R1Grid g, out;
    R1GridPlan P;
    NEED(build(c, g, P) == 0);
    NEED(!g.ids.empty() && g.outliers.size() == 1);
    Cloud far = c;
    for (uint32_t i = 0; i < far.n; ++i)
        far.x[i] += 700.0f;
    far.rows();
    NEED(!r1_grid_regrid_host(P, far.n, far.exact.data(), far.radii.data(), out));
    NEED(out.ids.empty() && out.outliers.size() == far.n && out.geom.v2 == INFINITY);
    NEED(std::all_of(out.start.begin(), out.start.end(), [](uint32_t s) { return s == 0; }) && out.start.size() == g.start.size());
    for (int a = 0; a < 3; ++a)
        NEED(out.geom.lo[a] == g.geom.lo[a] && out.geom.cell[a] == g.geom.cell[a] && out.geom.clo[a] == 0.0f && out.geom.chi[a] == 0.0f);
    NEED(check_tables(P, far, out) == 0);
    // ... and by their radii: every bound radius above `big`, the centres where they were
    Cloud fat = c;
    for (uint32_t i = 0; i < fat.n; ++i)
    {
        const float r = 10.0f + (float)i;
        fat.rsq[i] = r * r, fat.rb[i] = r1_bound_radius(r * r, 1.0f / r);
    }
    fat.rows();
    NEED(!r1_grid_regrid_host(P, fat.n, fat.exact.data(), fat.radii.data(), out));
    NEED(out.ids.empty() && out.outliers.size() == fat.n && check_tables(P, fat, out) == 0);
    printf("every sphere an outlier: %u outliers, no registrations, v2 = inf\n", far.n);
    return 0;
}

static int run_touch()
{
    Cloud c = lattice(10, 8);
    R1Grid g, in, outside;
    R1GridPlan P;
    NEED(build(c, g, P) == 0);
    NEED(!P.flat[0] && P.flat[1] && !P.flat[2]);
    const double hi = (double)P.lo[0] + (double)P.n[0] * (double)P.cell[0];
    const double rho = r1gf_rho(0.0f, c.y[0], c.z[0], c.radii[1], P.V, P.delta); // (test radius above r_floor: rho does not follow the centre)
    // the largest fp32 x whose ball [x - rho, x + rho] ends inside the box, by the rule's own expression
    float x = (float)(hi - rho);
    while ((double)x + rho > hi)
        x = r1gf_next_down(x);
    while ((double)r1f_next_up(x) + rho <= hi)
        x = r1f_next_up(x);
    Cloud t = c;
    t.x[0] = x, t.rows();
    NEED(r1gf_rho(x, c.y[0], c.z[0], c.radii[1], P.V, P.delta) == rho);
    NEED(!r1_grid_regrid_host(P, t.n, t.exact.data(), t.radii.data(), in));
    NEED(std::find(in.ids.begin(), in.ids.end(), 0u) != in.ids.end() && std::find(in.outliers.begin(), in.outliers.end(), 0u) == in.outliers.end());
    NEED(check_tables(P, t, in) == 0);
    t.x[0] = r1f_next_up(x), t.rows();
    NEED(!r1_grid_regrid_host(P, t.n, t.exact.data(), t.radii.data(), outside));
    NEED(std::find(outside.ids.begin(), outside.ids.end(), 0u) == outside.ids.end() && outside.outliers.front() == 0u);
    NEED(check_tables(P, t, outside) == 0);
    printf("ball on the box face: x = %.9g registered (x + rho - hi = %.3g), the next fp32 up an outlier\n", (double)x, (double)x + rho - hi);
    return 0;
}

static int run_zeros()
{
    Cloud c = lattice(9, 7);
    // a column and a row of the lattice on the planes x = 0 and z = 0
    for (uint32_t i = 0; i + 1 < c.n; ++i)
    {
        if (i % 9 == 0)
            c.x[i] = 0.0f;
        if (i / 9 == 0)
            c.z[i] = 0.0f;
    }
    c.rows();
    R1Grid g, plus, minus;
    R1GridPlan P;
    NEED(build(c, g, P) == 0);
    Cloud m = c;
    for (uint32_t i = 0; i < m.n; ++i)
    {
        m.x[i] = m.x[i] == 0.0f ? -0.0f : m.x[i];
        m.z[i] = m.z[i] == 0.0f ? -0.0f : m.z[i];
    }
    m.y[3] = -0.0f, c.y[3] = 0.0f;
    c.rows(), m.rows();
    NEED(!r1_grid_regrid_host(P, c.n, c.exact.data(), c.radii.data(), plus));
    NEED(!r1_grid_regrid_host(P, m.n, m.exact.data(), m.radii.data(), minus));
    NEED(check_tables(P, c, plus) == 0 && check_tables(P, m, minus) == 0);
    NEED(plus.start == minus.start && plus.ids == minus.ids && plus.outliers == minus.outliers && plus.pad == minus.pad);
    bool signs = false;
    for (int a = 0; a < 3; ++a)
    {
        NEED(plus.geom.lo[a] == minus.geom.lo[a] && plus.geom.cell[a] == minus.geom.cell[a] && plus.geom.inv_cell[a] == minus.geom.inv_cell[a]);
        NEED(memcmp(&plus.geom.lo[a], &minus.geom.lo[a], 4) == 0 && memcmp(&plus.geom.cell[a], &minus.geom.cell[a], 4) == 0);
        NEED(plus.geom.clo[a] == minus.geom.clo[a] && plus.geom.chi[a] == minus.geom.chi[a]);
        signs |= memcmp(&plus.geom.clo[a], &minus.geom.clo[a], 4) != 0;
    }
    NEED(plus.geom.v2 == minus.geom.v2);
    printf("signed zeros: the same tables and geometry%s\n", signs ? "; the far box keeps a zero's sign" : "");
    return 0;
}

static int run_twice()
{
    Cloud c = lattice(14, 10);
    R1Grid g;
    R1GridPlan P;
    NEED(build(c, g, P) == 0);
    Cloud a = c, b = c;
    for (uint32_t i = 0; i + 1 < c.n; ++i)
    {
        a.x[i] += 0.3f * (lcg() - 0.5f), a.z[i] += 0.3f * (lcg() - 0.5f), a.y[i] = 0.2f + 2.5f * lcg();
        b.x[i] += 0.2f * (lcg() - 0.5f), b.z[i] += 0.2f * (lcg() - 0.5f), b.y[i] = 0.2f + (i % 3 ? 0.0f : 1.5f * lcg());
    }
    a.rows(), b.rows();
    R1Grid ga, gb, gab, gbb;
    NEED(!r1_grid_regrid_host(P, b.n, b.exact.data(), b.radii.data(), gb));
    NEED(!r1_grid_regrid_host(P, a.n, a.exact.data(), a.radii.data(), ga));
    NEED(check_tables(P, a, ga) == 0 && check_tables(P, b, gb) == 0 && !same_grid(ga, gb));
    // the state a regrid leaves is the plan, which it does not change: the plan of the regridded grid is the plan it was made with
    R1GridPlan Pa;
    r1_grid_plan(ga, Pa);
    for (int k = 0; k < 3; ++k) // (but for the flat axis's stretched cell, which every regrid computes anew, and the build's own counts)
        if (Pa.flat[k])
            Pa.lo[k] = P.lo[k], Pa.cell[k] = P.cell[k], Pa.inv_cell[k] = P.inv_cell[k];
    Pa.regs = P.regs;
    NEED(memcmp(&Pa, &P, sizeof(P)) == 0);
    NEED(!r1_grid_regrid_host(Pa, b.n, b.exact.data(), b.radii.data(), gab));
    NEED(same_grid(gab, gb));
    NEED(!r1_grid_regrid_host(Pa, b.n, b.exact.data(), b.radii.data(), gbb));
    NEED(same_grid(gbb, gb));
    printf("regrid of a regridded state: unchanged (%zu registrations, %zu outliers)\n", gb.ids.size(), gb.outliers.size());
    return 0;
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "outliers"))
        return run_outliers();
    if (!strcmp(what, "touch"))
        return run_touch();
    if (!strcmp(what, "zeros"))
        return run_zeros();
    if (!strcmp(what, "twice"))
        return run_twice();
    fprintf(stderr, "usage: check_regrid_host outliers | touch | zeros | twice\n");
    return 2;
}
