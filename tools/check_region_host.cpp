// tools/check_region_host.cpp — region renders on the host, a stand-alone program over the library's host sources only:
// r1_region_check and r1_render_region_host on a 33 x 17 x 2 frame of the medium scene with an off-origin window and a row stride.  It checks what
// needs no second implementation: the window's values are the whole frame's (r1_render_linear_host) at those pixels, bit for bit, and so is the
// full-frame window; the count is at least the window's samples and the windows of a split add up to the frame's; nothing between the rows or
// around the window is written; a refusal writes nothing.
// tests/test_region_host.py builds and runs it as it is; this is also the program for -fsanitize=address,undefined (host code only, no GPU, no
// library loaded into another process):
//     clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//         -I<hip include dir> tools/check_region_host.cpp rays1bench_amd/csrc/{r1_linear_host,r1_queries_host,r1_host,r1_bvh}.cpp -pthread
//         -o check_region_host_asan
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

int main()
{
    const int w = 33, h = 17, spp = 2;
    r1_host_scene *hs = nullptr;
    NEED(r1_host_scene_create(R1_SCENE_MEDIUM, w, h, 0, 0, &hs) == R1_OK);
    const r1_scene *sc = r1_host_scene_spheres(hs);
    const r1_camera *cam = r1_host_scene_camera(hs);
    r1_params p = {w, h, spp, 50, 10001u, 32, 32, 0, 1, R1_VARIANT_DEFAULT};

    // the rules
    const r1_region full = {0, 0, w, h, 0}, last = {w - 1, h - 1, 1, 1, 0};
    NEED(r1_region_check(&p, &full) == R1_OK && r1_region_check(&p, &last) == R1_OK);
    const r1_region bad[] = {{-1, 0, 3, 3, 0}, {0, -1, 3, 3, 0}, {0, 0, 0, 3, 0}, {0, 0, 3, 0, 0}, {w - 2, 0, 3, 3, 0}, {0, h - 2, 3, 3, 0}, {0, 0, 5, 5, 4}};
    const char *const names[] = {"x0", "y0", "width", "height", "x0 + width", "y0 + height", "out_stride"};
    for (size_t k = 0; k < sizeof(bad) / sizeof(bad[0]); ++k)
    {
        g_error[0] = 0;
        NEED(r1_region_check(&p, &bad[k]) == R1_EINVAL);
        NEED(strstr(g_error, names[k]) != nullptr);
    }
    NEED(r1_region_check(nullptr, &full) == R1_EINVAL && r1_region_check(&p, nullptr) == R1_EINVAL);
    r1_params q = p;
    q.num_shards = 2;
    NEED(r1_region_check(&q, &full) == R1_EINVAL && strstr(g_error, "num_shards") != nullptr);
    const int refused[] = {R1_VARIANT_STATS, R1_VARIANT_BVH_STATS, R1_VARIANT_WAVEFRONT, R1_VARIANT_GRID_STATS};
    for (int v : refused)
    {
        q = p, q.variant = v;
        NEED(r1_region_check(&q, &full) == R1_EINVAL);
    }
    q = p, q.width = 40000, q.height = 40000; // 3.2e9 samples: no frame of r1_render, but windows of it are served
    const r1_region far_corner = {39991, 39993, 9, 7, 0}, too_many = {0, 0, 32768, 32768, 0};
    NEED(r1_params_check(&q) == R1_ELIMIT && r1_region_check(&q, &far_corner) == R1_OK && r1_region_check(&q, &too_many) == R1_ELIMIT);
    q.width = q.height = 46341;
    NEED(r1_region_check(&q, &last) == R1_ELIMIT);
    printf("rules: %zu windows refused by the field they name, 4 variants, num_shards 2, 2^31 pixels and 2^31 samples\n", sizeof(bad) / sizeof(bad[0]));

    // the value: the whole frame's, at the window's pixels
    const size_t n = (size_t)w * h * 3;
    std::vector<float> whole(n, -1.0f);
    uint64_t whole_rays = 0;
    NEED(r1_render_linear_host(sc, cam, &p, whole.data(), &whole_rays) == R1_OK);
    const float mark = -7.0f;
    const r1_region win = {5, 3, 21, 9, 29}; // off-origin, rows 29 pixels apart
    const size_t pad = 4, span = ((size_t)(win.height - 1) * win.out_stride + win.width) * 3;
    std::vector<float> buf(pad + span + pad, mark);
    uint64_t rays = 0;
    NEED(r1_render_region_host(sc, cam, &p, &win, buf.data() + pad, &rays) == R1_OK);
    NEED(rays >= (uint64_t)win.width * win.height * spp && rays < whole_rays);
    for (size_t i = 0; i < buf.size(); ++i)
    {
        const size_t k = i - pad, row = k / ((size_t)win.out_stride * 3), col = k % ((size_t)win.out_stride * 3);
        const bool inside = i >= pad && i < pad + span && col < (size_t)win.width * 3;
        if (!inside)
            NEED(buf[i] == mark); // between the rows, in front of the window and behind it
        else
            NEED(memcmp(&buf[i], &whole[((size_t)(win.y0 + row) * w + win.x0) * 3 + col], 4) == 0);
    }
    printf("window %d,%d %dx%d stride %d: %llu rays, every value the whole frame's, nothing written outside\n", win.x0, win.y0, win.width, win.height, win.out_stride,
           (unsigned long long)rays);

    // the full-frame window is the frame; the four windows of a split, pasted with out_stride = w, are the frame and add up to its count
    std::vector<float> again(n, mark);
    uint64_t rays_full = 0;
    NEED(r1_render_region_host(sc, cam, &p, &full, again.data(), &rays_full) == R1_OK);
    NEED(rays_full == whole_rays && memcmp(again.data(), whole.data(), n * 4) == 0);
    std::vector<float> paste(n, mark);
    uint64_t sum = 0;
    const int sx = 13, sy = 6;
    const r1_region quads[4] = {{0, 0, sx, sy, w}, {sx, 0, w - sx, sy, w}, {0, sy, sx, h - sy, w}, {sx, sy, w - sx, h - sy, w}};
    for (const r1_region &r : quads)
    {
        uint64_t part = 0;
        NEED(r1_render_region_host(sc, cam, &p, &r, paste.data() + ((size_t)r.y0 * w + r.x0) * 3, &part) == R1_OK);
        sum += part;
    }
    NEED(sum == whole_rays && memcmp(paste.data(), whole.data(), n * 4) == 0);
    printf("full window and four pasted quadrants: the frame, %llu rays\n", (unsigned long long)whole_rays);

    // refusals write nothing
    std::vector<float> untouched(n, mark);
    NEED(r1_render_region_host(sc, cam, &p, &bad[4], untouched.data(), &rays) == R1_EINVAL);
    NEED(r1_render_region_host(nullptr, cam, &p, &full, untouched.data(), nullptr) == R1_EINVAL);
    NEED(r1_render_region_host(sc, cam, &p, &full, nullptr, nullptr) == R1_EINVAL);
    for (size_t i = 0; i < n; ++i)
        NEED(untouched[i] == mark);
    NEED(r1_render_region_host(sc, cam, &p, &last, untouched.data(), nullptr) == R1_OK); // (num_rays_out may be NULL)
    NEED(memcmp(untouched.data(), &whole[n - 3], 12) == 0 && untouched[3] == mark);
    printf("refusals wrote nothing\n");
    r1_host_scene_destroy(hs);
    return 0;
}
