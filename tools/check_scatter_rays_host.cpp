// tools/check_scatter_rays_host.cpp — the scatter queries on the host, a stand-alone program over the library's host sources
// only: r1_camera_rays, then levels of r1_scatter_rays_host and the fold of include/rays1.h on a 33 x 17 x 2 frame of the medium scene,
// which must equal r1_trace_rays_host at that depth limit bit for bit; a level in place; rays that take no step; zero stream states;
// the refusals, which write nothing.  tests/test_scatter_rays_host.py checks the same against the reference's records; this is the program
// for -fsanitize=address,undefined (host code only, no GPU, no library loaded into another process):
//     clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//         -I<hip include dir> tools/check_scatter_rays_host.cpp rays1bench_amd/csrc/{r1_queries_host,r1_host,r1_bvh}.cpp -pthread
//         -o check_scatter_rays_host_asan
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/rays1.h"
#include "../include/rays1_seed.h"
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

// the fold: levels 0 .. bounces over the rays still alive, compacted between levels; out: {r, g, b, rays} per ray of the call
static int fold(const r1_scene *sc, const std::vector<r1_ray> &rays0, const std::vector<r1_sample_seed> &seeds0, const int bounces,
                std::vector<r1_radiance> &out, size_t events[4])
{
    const size_t n = rays0.size();
    out.assign(n, r1_radiance{0.0f, 0.0f, 0.0f, 0u});
    std::vector<std::vector<float>> weights(n); // the SCATTERED weights of a path, first to last
    std::vector<size_t> alive(n);
    for (size_t i = 0; i < n; ++i)
        alive[i] = i;
    std::vector<r1_ray> rays = rays0, next_rays;
    std::vector<r1_sample_seed> seeds = seeds0, next_seeds;
    std::vector<r1_scatter> rec;
    for (int level = 0; level <= bounces && !alive.empty(); ++level)
    {
        const size_t m = alive.size();
        rec.assign(m, r1_scatter{});
        // in place: rays_out is rays, seeds_out is seeds
        if (r1_scatter_rays_host(sc, level ? R1_SCATTER_UNIT_DIRECTIONS : 0, rays.data(), seeds.data(), m, rays.data(), seeds.data(), rec.data()) != R1_OK)
            return 1;
        std::vector<size_t> go;
        next_rays.clear(), next_seeds.clear();
        for (size_t k = 0; k < m; ++k)
        {
            const size_t i = alive[k];
            const r1_scatter &s = rec[k];
            if (s.event < 0 || s.event > 3 || s.pad != 0)
                return 1;
            events[s.event]++;
            if (s.event != R1_SCATTER_NONE)
                out[i].rays++;
            if (s.event == R1_SCATTER_SKY)
            {
                float c[3] = {s.weight[0], s.weight[1], s.weight[2]};
                for (size_t e = weights[i].size(); e >= 3; e -= 3)
                    for (int ch = 0; ch < 3; ++ch)
                        c[ch] = weights[i][e - 3 + ch] * c[ch];
                out[i].r = c[0], out[i].g = c[1], out[i].b = c[2];
            }
            else if (s.event == R1_SCATTER_SCATTERED)
            {
                weights[i].insert(weights[i].end(), s.weight, s.weight + 3);
                go.push_back(i), next_rays.push_back(rays[k]), next_seeds.push_back(seeds[k]);
            }
        }
        alive.swap(go), rays.swap(next_rays), seeds.swap(next_seeds);
    }
    return 0;
}

int main()
{
    const int w = 33, h = 17, spp = 2;
    r1_host_scene *hs = nullptr;
    NEED(r1_host_scene_create(R1_SCENE_MEDIUM, w, h, 0, 0, &hs) == R1_OK);
    const r1_scene *sc = r1_host_scene_spheres(hs);
    const r1_params p = {w, h, spp, 50, 10001u, 32, 32, 0, 1, R1_VARIANT_DEFAULT};
    const size_t n = (size_t)w * h * spp;
    std::vector<int32_t> x(n), y(n), s(n);
    for (size_t k = 0; k < n; ++k)
        s[k] = (int32_t)(k % spp), x[k] = (int32_t)((k / spp) % w), y[k] = (int32_t)(k / spp / w);
    std::vector<r1_ray> rays(n);
    std::vector<r1_sample_seed> seeds(n);
    NEED(r1_camera_rays(r1_host_scene_camera(hs), &p, x.data(), y.data(), s.data(), n, rays.data(), seeds.data()) == R1_OK);

    // the fold of the steps is the trace, at a shallow and at the deepest limit
    for (const int bounces : {1, 3, 50, 51})
    {
        std::vector<r1_radiance> got, want(n);
        size_t events[4] = {0, 0, 0, 0};
        NEED(fold(sc, rays, seeds, bounces, got, events) == 0);
        NEED(r1_trace_rays_host(sc, bounces, rays.data(), seeds.data(), n, want.data()) == R1_OK);
        NEED(memcmp(got.data(), want.data(), n * sizeof(r1_radiance)) == 0);
        NEED(events[R1_SCATTER_SCATTERED] > 0 && events[R1_SCATTER_SKY] > 0 && events[R1_SCATTER_NONE] == 0);
        printf("fold at %2d bounces: %zu scattered, %zu sky, %zu absorbed: the host trace's %zu records\n", bounces, events[0], events[1], events[2], n);
    }

    // out of place equals in place; NULL seeds are the seeding contract's
    std::vector<r1_ray> r1(n), r2 = rays;
    std::vector<r1_sample_seed> s1(n), s2 = seeds;
    std::vector<r1_scatter> o1(n), o2(n);
    NEED(r1_scatter_rays_host(sc, 0, rays.data(), seeds.data(), n, r1.data(), s1.data(), o1.data()) == R1_OK);
    NEED(r1_scatter_rays_host(sc, 0, r2.data(), s2.data(), n, r2.data(), s2.data(), o2.data()) == R1_OK);
    NEED(memcmp(r1.data(), r2.data(), n * 32) == 0 && memcmp(s1.data(), s2.data(), n * 16) == 0 && memcmp(o1.data(), o2.data(), n * 32) == 0);
    std::vector<r1_sample_seed> contract(n);
    for (size_t i = 0; i < n; ++i)
        contract[i] = r1_seed_guard(r1_seed_sample(0u, (uint32_t)i, 0u));
    NEED(r1_scatter_rays_host(sc, 0, rays.data(), nullptr, n, r1.data(), s1.data(), o1.data()) == R1_OK);
    NEED(r1_scatter_rays_host(sc, 0, rays.data(), contract.data(), n, r2.data(), s2.data(), o2.data()) == R1_OK);
    NEED(memcmp(r1.data(), r2.data(), n * 32) == 0 && memcmp(s1.data(), s2.data(), n * 16) == 0 && memcmp(o1.data(), o2.data(), n * 32) == 0);
    printf("in place and NULL seeds: the same %zu records\n", n);

    // rays that take no step, and all-zero stream states (replaced: the call returns)
    std::vector<r1_ray> odd(rays.begin(), rays.begin() + 64);
    std::vector<r1_sample_seed> zero(64, r1_sample_seed{0u, 0u, 0u, 0u});
    for (size_t i = 0; i < 64; i += 4)
    {
        odd[i].o[i % 3] = i % 8 ? NAN : -INFINITY;
        odd[i + 1].d[0] = odd[i + 1].d[1] = odd[i + 1].d[2] = i % 8 ? 0.0f : 1e-30f;
    }
    NEED(r1_scatter_rays_host(sc, 0, odd.data(), zero.data(), 64, r1.data(), s1.data(), o1.data()) == R1_OK);
    const r1_sample_seed guarded = r1_seed_guard(zero[0]);
    const r1_ray no_ray = {};
    size_t none = 0;
    for (size_t i = 0; i < 64; ++i)
    {
        if (i % 4 < 2)
        {
            NEED(o1[i].event == R1_SCATTER_NONE && o1[i].t == FLT_MAX && o1[i].index == -1 && o1[i].mat_type == R1_MAT_NONE && o1[i].pad == 0);
            NEED(o1[i].weight[0] == 0 && o1[i].weight[1] == 0 && o1[i].weight[2] == 0);
            NEED(memcmp(&r1[i], &no_ray, 32) == 0 && memcmp(&s1[i], &guarded, 16) == 0);
            ++none;
        }
        else
            NEED(o1[i].event != R1_SCATTER_NONE && (o1[i].event != R1_SCATTER_SKY || memcmp(&s1[i], &guarded, 16) == 0));
    }
    printf("%zu rays without a step among 64, all-zero states replaced\n", none);

    // refusals write nothing
    std::vector<r1_scatter> untouched(4, r1_scatter{{7, 7, 7}, 7, 7, 7, 7, 7});
    NEED(r1_scatter_rays_host(sc, 2, rays.data(), seeds.data(), 4, r1.data(), s1.data(), untouched.data()) == R1_EINVAL);
    NEED(r1_scatter_rays_host(nullptr, 0, rays.data(), seeds.data(), 4, r1.data(), s1.data(), untouched.data()) == R1_EINVAL);
    NEED(r1_scatter_rays_host(sc, 0, nullptr, seeds.data(), 4, r1.data(), s1.data(), untouched.data()) == R1_EINVAL);
    NEED(r1_scatter_rays_host(sc, 0, rays.data(), seeds.data(), 4, nullptr, s1.data(), untouched.data()) == R1_EINVAL);
    NEED(r1_scatter_rays_host(sc, 0, rays.data(), seeds.data(), 4, r1.data(), nullptr, untouched.data()) == R1_EINVAL);
    NEED(r1_scatter_rays_host(sc, 0, rays.data(), seeds.data(), 4, r1.data(), s1.data(), nullptr) == R1_EINVAL);
    NEED(r1_scatter_rays_host(sc, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == R1_OK);
    for (const r1_scatter &u : untouched)
        NEED(u.event == 7 && u.pad == 7 && u.weight[0] == 7);
    printf("refusals: six, nothing written\n");
    r1_host_scene_destroy(hs);
    return 0;
}
