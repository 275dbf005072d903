// tools/check_features_host.cpp — feature frames on the host, a stand-alone program over the library's host sources only:
// r1_render_features_host on a 33 x 17 x 3 frame of the medium scene.  It checks the host form against the contract folded here in C from
// r1_camera_rays + r1_cast_rays_host + the scene arrays — every record, bit for bit, and that the frame has pixels without a hit, with some
// and with all —, a strided window against the whole frame with nothing written between the rows, the NULL region, and the refusals, which
// write nothing.
// tests/test_features_host.py builds and runs it as it is; this is also the program for -fsanitize=address,undefined (host code only, no GPU,
// no library loaded into another process):
//     clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//         -I<hip include dir> tools/check_features_host.cpp rays1bench_amd/csrc/{r1_queries_host,r1_host,r1_bvh}.cpp -pthread
//         -o check_features_host_asan
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/rays1.h"
#include "../rays1bench_amd/csrc/r1_internal.h"

// (the library's error text lives in r1_capi.cpp, next to the HIP runtime: this program links the host sources only)
static char g_error[512];
void r1_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
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

// the contract for pixel (x, y): the fold of the cast records of its samples' camera rays (compiled with -ffp-contract=off)
static int fold_pixel(const r1_scene *sc, const r1_camera *cam, const r1_params *p, int x, int y, r1_feature *out)
{
    r1_feature f;
    memset(&f, 0, sizeof(f));
    for (int s = 0; s < p->spp; ++s)
    {
        r1_ray ray;
        r1_sample_seed seed;
        r1_hit hit;
        if (r1_camera_rays(cam, p, &x, &y, &s, 1, &ray, &seed) != R1_OK || r1_cast_rays_host(sc, R1_CAST_CLOSEST, &ray, 1, &hit) != R1_OK)
            return 1;
        if (hit.index >= 0)
        {
            const bool glass = sc->mat_type[hit.index] == R1_MAT_DIELECTRIC;
            f.albedo[0] += glass ? 1.0f : sc->albedo_r[hit.index];
            f.albedo[1] += glass ? 1.0f : sc->albedo_g[hit.index];
            f.albedo[2] += glass ? 1.0f : sc->albedo_b[hit.index];
            for (int k = 0; k < 3; ++k)
                f.normal[k] += hit.n[k];
            f.depth += hit.t;
            f.hits += 1u;
        }
        else
        {
            // the sky of the ray: unit_vector as mymath.h:211 (v * (1 / length)), then rayweek1.cpp:532-534
            const float len = sqrtf(ray.d[0] * ray.d[0] + ray.d[1] * ray.d[1] + ray.d[2] * ray.d[2]);
            const float dy = ray.d[1] * (1.0f / len);
            const float t = 0.5f * (dy + 1.0f), omt = 1.0f - t;
            f.albedo[0] += omt * 1.0f + t * 0.5f, f.albedo[1] += omt * 1.0f + t * 0.7f, f.albedo[2] += omt * 1.0f + t * 1.0f;
        }
    }
    const float inv = (float)(1.0f / p->spp);
    for (int k = 0; k < 3; ++k)
        f.albedo[k] *= inv, f.normal[k] *= inv;
    f.depth *= inv;
    *out = f;
    return 0;
}

int main()
{
    const int w = 33, h = 17, spp = 3;
    r1_host_scene *hs = nullptr;
    NEED(r1_host_scene_create(R1_SCENE_MEDIUM, w, h, 0, 0, &hs) == R1_OK);
    const r1_scene *sc = r1_host_scene_spheres(hs);
    const r1_camera *cam = r1_host_scene_camera(hs);
    r1_params p = {w, h, spp, 50, 4242u, 32, 32, 0, 1, R1_VARIANT_DEFAULT};
    const size_t n = (size_t)w * h;

    // the whole frame (region NULL) against the fold
    r1_feature mark;
    memset(&mark, 0xA5, sizeof(mark));
    std::vector<r1_feature> whole(n, mark);
    NEED(r1_render_features_host(sc, cam, &p, nullptr, whole.data()) == R1_OK);
    size_t none = 0, some = 0, all = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            r1_feature f;
            NEED(fold_pixel(sc, cam, &p, x, y, &f) == 0);
            NEED(memcmp(&f, &whole[(size_t)y * w + x], sizeof(f)) == 0);
            none += f.hits == 0, some += f.hits > 0 && f.hits < (uint32_t)spp, all += f.hits == (uint32_t)spp;
        }
    NEED(none >= 10 && some >= 10 && all >= 10 && none + some + all == n);
    printf("frame %dx%dx%d: every record the fold of its cast records; %zu pixels without a hit, %zu with some, %zu with all\n", w, h, spp, none, some, all);

    // a strided window: the frame's records, nothing written outside
    const r1_region win = {5, 3, 21, 9, 29};
    const size_t pad = 2, span = (size_t)(win.height - 1) * win.out_stride + win.width;
    std::vector<r1_feature> buf(pad + span + pad, mark);
    NEED(r1_render_features_host(sc, cam, &p, &win, buf.data() + pad) == R1_OK);
    for (size_t i = 0; i < buf.size(); ++i)
    {
        const size_t k = i - pad, row = k / (size_t)win.out_stride, col = k % (size_t)win.out_stride;
        const bool inside = i >= pad && i < pad + span && col < (size_t)win.width;
        NEED(memcmp(&buf[i], inside ? &whole[(size_t)(win.y0 + row) * w + win.x0 + col] : &mark, sizeof(mark)) == 0);
    }
    const r1_region full = {0, 0, w, h, 0}, last = {w - 1, h - 1, 1, 1, 0};
    std::vector<r1_feature> again(n, mark);
    NEED(r1_render_features_host(sc, cam, &p, &full, again.data()) == R1_OK && memcmp(again.data(), whole.data(), n * sizeof(mark)) == 0);
    printf("window %d,%d %dx%d stride %d and the full window: the frame's records, nothing written outside\n", win.x0, win.y0, win.width, win.height, win.out_stride);

    // refusals write nothing
    std::vector<r1_feature> untouched(n, mark);
    const r1_region bad = {w - 2, 0, 3, 3, 0};
    r1_params q = p;
    g_error[0] = 0;
    NEED(r1_render_features_host(sc, cam, &p, &bad, untouched.data()) == R1_EINVAL && strstr(g_error, "x0 + width") != nullptr);
    NEED(r1_render_features_host(nullptr, cam, &p, &full, untouched.data()) == R1_EINVAL);
    NEED(r1_render_features_host(sc, nullptr, &p, &full, untouched.data()) == R1_EINVAL);
    NEED(r1_render_features_host(sc, cam, nullptr, &full, untouched.data()) == R1_EINVAL);
    NEED(r1_render_features_host(sc, cam, &p, &full, nullptr) == R1_EINVAL);
    q.num_shards = 2;
    NEED(r1_render_features_host(sc, cam, &q, nullptr, untouched.data()) == R1_EINVAL && strstr(g_error, "num_shards") != nullptr);
    q = p, q.spp = 0;
    NEED(r1_render_features_host(sc, cam, &q, nullptr, untouched.data()) == R1_EINVAL);
    q = p, q.max_bounces = 0;
    NEED(r1_render_features_host(sc, cam, &q, nullptr, untouched.data()) == R1_EINVAL);
    for (size_t i = 0; i < n; ++i)
        NEED(memcmp(&untouched[i], &mark, sizeof(mark)) == 0);
    NEED(r1_render_features_host(sc, cam, &p, &last, untouched.data()) == R1_OK);
    NEED(memcmp(&untouched[0], &whole[n - 1], sizeof(mark)) == 0 && memcmp(&untouched[1], &mark, sizeof(mark)) == 0);
    printf("refusals wrote nothing\n");
    r1_host_scene_destroy(hs);
    return 0;
}
