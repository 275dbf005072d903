// tools/check_update_host.cpp — sphere updates on the host, a stand-alone program with two jobs.
//
// 1. `check_update_host radii` / `check_update_host materials`: reads lines of hexadecimal fp32 bit patterns from stdin and prints what
//    csrc/r1_bvh_fill.h derives from them, as bit patterns — per line "radius_sq inv_radius" -> "hittable rsq inv bound test" (r1f_radius_rows, with
//    r1f_bound_radius and r1f_test_radius of the pair as given in front: "bound0 test0"), or "type param" -> the four words of r1f_material_row.
//    tests/test_update_spheres_host.py compiles this file alone (g++, the header only) and compares with a numpy restatement.
//        g++ -O2 -std=c++17 -ffp-contract=off tools/check_update_host.cpp -o check_update_host
// 2. With -DR1_CHECK_LIBRARY, linked against the library's host sources, `check_update_host scene` edits the large scene (radii, centres),
//    runs the host restatement of the refit (r1_bvh_refit_describe_spheres) and the host query forms (r1_cast_rays_host, r1_trace_rays_host) on the
//    edited arrays and checks what can be checked without a device: the rows are finite or -inf, the identity refit is the builder's.  This is the
//    program for -fsanitize=address,undefined (host code only, no GPU, no library loaded into another process):
//        clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -DR1_CHECK_LIBRARY -D__HIP_PLATFORM_AMD__
//            -I/opt/rocm/include tools/check_update_host.cpp rays1bench_amd/csrc/{r1_bvh,r1_host,r1_queries_host,r1_sweep}.cpp -pthread -o check_update_host_asan
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../rays1bench_amd/csrc/r1_bvh_fill.h"

static uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }
static unsigned long long bits(double d) { return __builtin_bit_cast(unsigned long long, d); }
static float f32(uint32_t b) { return __builtin_bit_cast(float, b); }

static int rows(bool radii)
{
    unsigned a, b;
    while (scanf("%x %x", &a, &b) == 2)
        if (radii)
        {
            float rsq, inv;
            double rr[2];
            const double b0 = r1f_bound_radius(f32(a), f32(b)), t0 = r1f_test_radius(b0, f32(a));
            r1f_radius_rows(f32(a), f32(b), rsq, inv, rr);
            printf("%016llx %016llx %d %08x %08x %016llx %016llx\n", bits(b0), bits(t0), (int)r1f_hittable_radius(f32(a), f32(b)), bits(rsq), bits(inv), bits(rr[0]),
                   bits(rr[1]));
        }
        else
        {
            float row[4];
            r1f_material_row(a, f32(b), row);
            printf("%08x %08x %08x %08x\n", bits(row[0]), bits(row[1]), bits(row[2]), bits(row[3]));
        }
    return 0;
}

#ifdef R1_CHECK_LIBRARY
#include <stdarg.h>

#include "../include/rays1.h"
#include "../rays1bench_amd/csrc/r1_internal.h"

// (the library's error text lives in r1_capi.cpp, next to the HIP runtime: this program links the host sources only)
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

static int scene()
{
    r1_host_scene *hs = nullptr;
    NEED(r1_host_scene_create(R1_SCENE_LARGE, 96, 64, 0, 0, &hs) == R1_OK);
    const r1_scene *s = r1_host_scene_spheres(hs);
    const uint32_t n = s->count;
    std::vector<float> x(s->center_x, s->center_x + n), y(s->center_y, s->center_y + n), z(s->center_z, s->center_z + n);
    std::vector<float> rsq(s->radius_sq, s->radius_sq + n), inv(s->inv_radius, s->inv_radius + n);
    r1_bvh_info info, built;
    NEED(r1_bvh_describe(s, 0, &built, nullptr, 0, nullptr, 0) == R1_OK);
    std::vector<float> rows0(16 * (size_t)built.nodes), rows(16 * (size_t)built.nodes);
    NEED(r1_bvh_describe(s, 0, &built, rows0.data(), rows0.size(), nullptr, 0) == R1_OK);
    // identity: the builder's rows
    NEED(r1_bvh_refit_describe_spheres(s, x.data(), y.data(), z.data(), rsq.data(), inv.data(), 0, &info, rows.data(), rows.size()) == R1_OK);
    NEED(memcmp(rows.data(), rows0.data(), rows.size() * 4) == 0);
    NEED(r1_bvh_refit_describe_spheres(s, x.data(), y.data(), z.data(), nullptr, nullptr, 0, &info, rows.data(), rows.size()) == R1_OK);
    NEED(memcmp(rows.data(), rows0.data(), rows.size() * 4) == 0);
    NEED(r1_bvh_refit_describe_spheres(s, x.data(), y.data(), z.data(), rsq.data(), nullptr, 0, &info, rows.data(), rows.size()) == R1_EINVAL);
    // the edit: every hittable sphere breathes (radius x 0.5 .. 2 by index), every third is lifted, one gets a pair that would make it inactive
    uint32_t edited = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (inv[i] != 0)
        {
            const float r = (1.0f / inv[i]) * (0.5f + 0.25f * (float)(i % 7u));
            rsq[i] = r * r, inv[i] = 1.0f / r;
            if (i % 3u == 0)
                y[i] += 0.5f;
            if (++edited == 40)
                inv[i] = 0.0f;
        }
    NEED(r1_bvh_refit_describe_spheres(s, x.data(), y.data(), z.data(), rsq.data(), inv.data(), 0, &info, rows.data(), rows.size()) == R1_OK);
    NEED(info.nodes == built.nodes && info.flat_axis == -1);
    for (size_t k = 0; k < rows.size(); ++k)
        if (k % 16 < 14)
            NEED(rows[k] == rows[k] && (fabsf(rows[k]) <= 3.402823466e38f || rows[k] == -INFINITY));
    NEED(memcmp(rows.data(), rows0.data(), rows.size() * 4) != 0);
    // the host query forms on the edited arrays
    r1_scene e = *s;
    e.center_x = x.data(), e.center_y = y.data(), e.center_z = z.data(), e.radius_sq = rsq.data(), e.inv_radius = inv.data();
    const size_t nr = 512;
    std::vector<r1_ray> rays(nr);
    for (size_t q = 0; q < nr; ++q)
    {
        const uint32_t i = (uint32_t)((q * 7919u) % n);
        r1_ray &r = rays[q];
        r.o[0] = 13.0f, r.o[1] = 2.0f, r.o[2] = 3.0f, r.t_max = 3.402823466e38f, r.pad = 0;
        r.d[0] = x[i] - r.o[0], r.d[1] = y[i] - r.o[1], r.d[2] = z[i] - r.o[2];
    }
    std::vector<r1_hit> hits(nr);
    std::vector<uint8_t> any(nr);
    std::vector<r1_radiance> rad(nr);
    NEED(r1_cast_rays_host(&e, R1_CAST_CLOSEST, rays.data(), nr, hits.data()) == R1_OK);
    NEED(r1_cast_rays_host(&e, R1_CAST_ANY, rays.data(), nr, any.data()) == R1_OK);
    NEED(r1_trace_rays_host(&e, 50, rays.data(), nullptr, nr, rad.data()) == R1_OK);
    size_t n_hit = 0;
    for (size_t q = 0; q < nr; ++q)
    {
        NEED((hits[q].index >= 0) == (any[q] != 0));
        NEED(hits[q].index < (int32_t)n && (hits[q].index < 0 || inv[(size_t)hits[q].index] != 0));
        NEED(rad[q].rays >= 1);
        n_hit += any[q];
    }
    NEED(n_hit > nr / 2);
    r1_host_scene_destroy(hs);
    printf("scene: %u spheres, %d nodes refitted, %zu of %zu rays hit\n", n, info.nodes, n_hit, nr);
    return 0;
}
#endif

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "radii") == 0)
        return rows(true);
    if (argc == 2 && strcmp(argv[1], "materials") == 0)
        return rows(false);
#ifdef R1_CHECK_LIBRARY
    if (argc == 2 && strcmp(argv[1], "scene") == 0)
        return scene();
#endif
    fprintf(stderr, "usage: check_update_host radii | materials  (hexadecimal fp32 pairs on stdin)%s\n",
#ifdef R1_CHECK_LIBRARY
            " | scene"
#else
            ""
#endif
    );
    return 2;
}
