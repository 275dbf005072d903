// tools/check_linear_host.cpp — linear frames on the host, a stand-alone program over the library's host sources only:
// r1_render_linear_host, r1_quantise_linear and r1_pfm_write_rgb32f on a 33 x 17 x 2 frame of the medium scene.  It checks what needs no
// second implementation: every value is finite and within [0, 1], the frame does not depend on the tile fields, the quantised bytes are
// (uint8)(int)(sqrtf(v) * 255.99f), the refusals write nothing, and the PFM file read back is the header and the frame's bytes.
// tests/test_linear_host.py builds and runs it as it is; this is also the program for -fsanitize=address,undefined (host code only, no
// GPU, no library loaded into another process):
//     clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//         -I<hip include dir> tools/check_linear_host.cpp rays1bench_amd/csrc/{r1_linear_host,r1_queries_host,r1_host,r1_bvh}.cpp -pthread
//         -o check_linear_host_asan
//     check_linear_host_asan <a file name for the PFM>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

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

int main(int argc, const char *argv[])
{
    if (argc != 2)
    {
        fprintf(stderr, "usage: check_linear_host FILE.pfm\n");
        return 2;
    }
    const int w = 33, h = 17, spp = 2;
    r1_host_scene *hs = nullptr;
    NEED(r1_host_scene_create(R1_SCENE_MEDIUM, w, h, 0, 0, &hs) == R1_OK);
    r1_params p = {w, h, spp, 50, 10001u, 32, 32, 0, 1, R1_VARIANT_DEFAULT};
    const size_t n = (size_t)w * h * 3;
    std::vector<float> lin(n, -1.0f), again(n, -1.0f);
    uint64_t rays = 0, rays2 = 0;
    NEED(r1_render_linear_host(r1_host_scene_spheres(hs), r1_host_scene_camera(hs), &p, lin.data(), &rays) == R1_OK);
    NEED(rays >= (uint64_t)w * h * spp);
    for (size_t i = 0; i < n; ++i)
        NEED(lin[i] >= 0.0f && lin[i] <= 1.0f);
    p.tile_w = 16, p.tile_h = 8; // the linear frame does not depend on the tile size
    NEED(r1_render_linear_host(r1_host_scene_spheres(hs), r1_host_scene_camera(hs), &p, again.data(), &rays2) == R1_OK);
    NEED(rays2 == rays && memcmp(lin.data(), again.data(), n * 4) == 0);
    p.num_shards = 2;
    NEED(r1_render_linear_host(r1_host_scene_spheres(hs), r1_host_scene_camera(hs), &p, again.data(), nullptr) == R1_EINVAL);
    p.num_shards = 1;
    NEED(r1_render_linear_host(nullptr, r1_host_scene_camera(hs), &p, again.data(), nullptr) == R1_EINVAL);
    printf("linear frame %dx%dx%d: %llu rays, every value within [0, 1]\n", w, h, spp, (unsigned long long)rays);

    std::vector<uint8_t> q(n, 0xA5);
    NEED(r1_quantise_linear(lin.data(), n, q.data()) == R1_OK);
    for (size_t i = 0; i < n; ++i)
        NEED(q[i] == (uint8_t)(int)(sqrtf(lin[i]) * 255.99f));
    const float edge[5] = {0.0f, -0.0f, 1.0f, 0.25f, 4.0f};
    uint8_t eq[5];
    NEED(r1_quantise_linear(edge, 5, eq) == R1_OK);
    NEED(eq[0] == 0 && eq[1] == 0 && eq[2] == 255 && eq[3] == 127 && eq[4] == (uint8_t)511);
    const float bad[4] = {-1.0f, NAN, INFINITY, 3.0e38f};
    for (int k = 0; k < 4; ++k)
    {
        float v[3] = {0.5f, bad[k], 0.5f};
        uint8_t o[3] = {7, 7, 7};
        NEED(r1_quantise_linear(v, 3, o) == R1_EINVAL);
        NEED(o[0] == 7 && o[1] == 7 && o[2] == 7);
    }
    NEED(r1_quantise_linear(nullptr, 0, nullptr) == R1_OK && r1_quantise_linear(nullptr, 1, q.data()) == R1_EINVAL);
    printf("quantised: %zu bytes as (uint8)(int)(sqrtf(v) * 255.99f); -1, NaN, +inf and 3e38 refused\n", n);

    NEED(r1_pfm_write_rgb32f(argv[1], w, h, lin.data()) == R1_OK);
    FILE *f = fopen(argv[1], "rb");
    NEED(f != nullptr);
    char want[64];
    const int hl = snprintf(want, sizeof(want), "PF\n%d %d\n-1.0\n", w, h);
    std::vector<char> file((size_t)hl + n * 4 + 1);
    const size_t got = fread(file.data(), 1, file.size(), f);
    fclose(f);
    NEED(got == (size_t)hl + n * 4);
    NEED(memcmp(file.data(), want, (size_t)hl) == 0 && memcmp(file.data() + hl, lin.data(), n * 4) == 0);
    NEED(r1_pfm_write_rgb32f(nullptr, w, h, lin.data()) == R1_EINVAL && r1_pfm_write_rgb32f(argv[1], 0, h, lin.data()) == R1_EINVAL);
    printf("pfm: header and %zu bytes read back\n", n * 4);
    r1_host_scene_destroy(hs);
    return 0;
}
