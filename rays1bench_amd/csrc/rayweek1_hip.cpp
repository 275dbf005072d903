// rayweek1_hip.cpp — the drop-in host program: the reference's entry points for the hot path
//     Scene *create_small_scene() / create_medium_scene() / create_large_scene()
//                                       (/root/reference/src/step13/rayweek1.cpp:552 / :582 / :654)
//     RESULT benchmark(Scene *scene, Pix *pixels, bool write_tga, const char *scene_name)
//                                       (rayweek1.cpp:845-927)
//     main: -w, -n N                    (rayweek1.cpp:930-988)
// kept with the same signatures, ownership (benchmark() deletes the scene it is given,
// rayweek1.cpp:905), stdout block (:895-902), out_<scene>.txt (common.h:47-77) and TGA
// (common.h:86-122), but rendering through librays1.so (include/rays1.h) on a MI355X.
// This file holds that surface: the types, the options, benchmark(), the logs and main.  What runs after the benchmark() runs
// (--pipeline, --orbit, --bounce, --pulse) is rayweek1_demos.cpp; rayweek1_options.h lies between the two.
//
// What the reference fixes at compile time (common.h:19-28) is a run-time option here:
//     --width W --height H --spp S --seed N --device D --devices N --variant V
//       (V = R1_VARIANT_*: 0 default, 1 reference-form sweep, 2 exhaustive sweep, 4 box tree, 6 wavefront, 7 uniform grid)
// Defaults are the reference's multi-threaded defaults: 1280x720, 250 spp.
// --devices N splits the frame over N HIP devices inside this one process, tile t -> device
// t % N (the in-process twin of the reference's thread pool, rayweek1.cpp:785-842):
//     --gather rccl (default when the N devices are distinct GPUs): r1_multi_render — every device
//         renders its tiles, ONE ncclAllGather of the tile blocks + ray counts over xGMI, device 0
//         assembles the image and copies it to the host once (the join of rayweek1.cpp:804-813)
//     --gather host: one host thread + r1_context per device, each device copies its own tiles
//         into the caller's pixel buffer (also works oversubscribed: N contexts on fewer GPUs)
// bench.py's one-process-per-GPU form (torch.distributed) gathers the same records.
// --passes K renders each frame progressively (r1_render_pass): K contiguous passes whose sample counts differ by at most one, pixels
// asked for on the last pass only; the timed span covers all of them, and the image and ray count are those of the one-launch frame.
// --adaptive MAXDELTA[,MEANQ8] [--min-spp N] [--pass-spp N] renders each frame through r1_render_adaptive: --spp is the cap, a tile stops
// sampling once its pixels have settled (include/rays1.h); the report gains one "<scene> adaptive:" line.  MEANQ8 defaults to 65280 (no bound
// on the mean), --min-spp and --pass-spp to 16.
// --linear renders each frame through r1_render_linear: the fp32 frame comes home, the pixels of the TGA are r1_quantise_linear's — the bytes
// r1_render returns — and -w also writes out_<scene>.pfm; the report gains one "<scene> linear:" line.
// --region X,Y,W,H renders each frame through r1_render_region: window (X, Y, W, H) of the --width x --height frame (row 0 = bottom row), the
// crop of the whole frame byte for byte; the pixels, the TGA and the counts of the report and of out_<scene>.txt are the window's, and the report
// gains one "<scene> region:" line.
// --features also renders each frame's feature frame through r1_render_features (the window's, with --region): first-hit albedo, normal and
// depth per pixel, aligned with the frame; -w also writes out_<scene>_albedo.pfm, _normal.pfm and _depth.pfm (depth in all three channels),
// and the report gains one "<scene> features:" line with the device time.
// --denoise [ITERATIONS] is --linear, and each frame is also rendered through r1_render_denoised (ITERATIONS a-trous iterations, 3 if not given;
// normal_power_log2 6, sigma_color 1, sigma_depth 0.1, demodulated): -w also writes out_<scene>_denoised.pfm next to the noisy out_<scene>.pfm,
// and the report gains one "<scene> denoise:" line with the device time.
// --denoise-guided [ITERATIONS] is the same through r1_render_denoised_guided (the variance-guided filter: sigma_color 2, variance_floor 1e-4): the same
// file, one "<scene> denoise-guided:" line; not with --denoise, and not with --spp 1, which carries no variance.
// --backend hip (default) | cpu-step1 | cpu-step12: the reference's two single-thread CPU stages
// (r1_cpu_backends.cpp) behind the same benchmark(), for the README-style table
// (README.md:38-84).  Named backends of this program only — never a fallback: with --backend hip and no
// usable device the program exits with an error.

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "rayweek1_options.h"

// ---- common.h types ----------------------------------------------------------------------------

struct RESULT // common.h:36-45
{
    double elapsed_seconds;
    uint64_t num_rays;
    double get_mrays_per_sec() const { return elapsed_seconds ? (num_rays / elapsed_seconds / 1000000.0) : 0; }
};

struct Pix // common.h:80-83
{
    uint8_t r, g, b;
};

// ---- run-time configuration ------------------------------------------------------------------------

Options g_opt;
int r1cpu_step12_render(const r1_scene *scene, const r1_camera *cam, int width, int height, int spp, int max_bounces, uint8_t *rgb,
                        uint64_t *num_rays); // r1_cpu_backends.cpp
int r1cpu_step1_render(int scene_kind, const r1_scene *scene, const r1_camera *cam, int width, int height, int spp, uint8_t *rgb,
                       uint64_t *num_rays);
static std::vector<r1_context *> g_ctx; // one per device in use (--gather host)
static r1_multi *g_multi = nullptr;     // --gather rccl
static std::vector<double> g_device_seconds; // per benchmark() call, for the JSON record
static r1_launch_info g_last_info;
static float *g_linear = nullptr; // --linear: the frame r1_render_linear fills (page-locked where the device allows it)
static std::vector<float> g_denoised;       // --denoise: the denoised frame of the last benchmark() call
static std::vector<r1_feature> g_features; // --features: the feature frame of the last benchmark() call

r1_params frame_params()
{
    r1_params p;
    memset(&p, 0, sizeof(p));
    p.width = g_opt.width, p.height = g_opt.height, p.spp = g_opt.spp, p.max_bounces = g_opt.max_bounces;
    p.seed = g_opt.seed;
    p.tile_w = 32, p.tile_h = 32; // rayweek1.cpp:855-856
    p.shard = 0, p.num_shards = 1;
    p.variant = g_opt.variant;
    return p;
}

// ---- Scene ---------------------------------------------------------------------------------------

class Scene // rayweek1.cpp:539-549: owns its spheres/materials, deleted by benchmark()
{
  public:
    r1_host_scene *host = nullptr;
    int kind = 0; // R1_SCENE_*
    const r1_scene *hitables = nullptr;
    const r1_camera *camera = nullptr;
    ~Scene() { r1_host_scene_destroy(host); }
};

static Scene *make_scene(int kind)
{
    Scene *s = new Scene;
    if (r1_host_scene_create(kind, g_opt.width, g_opt.height, 0, 0, &s->host) != R1_OK)
    {
        fprintf(stderr, "scene build failed: %s\n", r1_last_error());
        exit(1);
    }
    s->kind = kind;
    s->hitables = r1_host_scene_spheres(s->host);
    s->camera = r1_host_scene_camera(s->host);
    return s;
}

Scene *create_small_scene() { return make_scene(R1_SCENE_SMALL); }
Scene *create_medium_scene() { return make_scene(R1_SCENE_MEDIUM); }
Scene *create_large_scene() { return make_scene(R1_SCENE_LARGE); }

// ---- benchmark -------------------------------------------------------------------------------------

// What a backend hands benchmark() for one frame; the pixels are in the caller's buffer.  A backend that fails says so on stderr.
struct Frame
{
    int rc = R1_OK;
    uint64_t rays = 0;
    double device_seconds = 0;
    r1_launch_info info = {};
    std::string lines; // the backend's own lines of the report block: before the `device time:` line (hip only) and after it
    std::string lines_after;
};

static std::string line(const char *format, ...) __attribute__((format(printf, 1, 2)));
static std::string line(const char *format, ...)
{
    char text[512];
    va_list args;
    va_start(args, format);
    vsnprintf(text, sizeof(text), format, args);
    va_end(args);
    return text;
}

// the reference's single-thread CPU stages (r1_cpu_backends.cpp), same timer span and report
static Frame cpu_frame(const Scene *scene, Pix *pixels)
{
    Frame f;
    if (g_opt.backend == 12)
        r1cpu_step12_render(scene->hitables, scene->camera, g_opt.width, g_opt.height, g_opt.spp, g_opt.max_bounces, &pixels[0].r, &f.rays);
    else
        r1cpu_step1_render(scene->kind, scene->hitables, scene->camera, g_opt.width, g_opt.height, g_opt.spp, &pixels[0].r, &f.rays);
    f.info.spheres_padded = (int32_t)scene->hitables->count;
    f.lines = line("backend:        %s (1 host thread, no GPU)\n", g_opt.backend == 12 ? "cpu-step12" : "cpu-step1");
    return f;
}

// tile split over the devices + one RCCL all-gather, behind one call
static Frame multi_frame(const Scene *scene, Pix *pixels, const r1_params &p, const char *scene_name)
{
    Frame f;
    f.rc = r1_multi_set_scene(g_multi, scene->hitables, scene->camera);
    if (f.rc == R1_OK)
        f.rc = r1_multi_render(g_multi, &p, &pixels[0].r, &f.rays, &f.device_seconds);
    if (f.rc != R1_OK)
    {
        fprintf(stderr, "%s: render failed (%d): %s\n", scene_name, f.rc, r1_last_error());
        return f;
    }
    int32_t nd = 0, ver = 0;
    r1_multi_info(g_multi, &nd, &ver, &f.info);
    f.lines = line("devices:        %d (first hip:%d, %d CUs, %d workgroups x %d threads), gather: RCCL %d all-gather\n", nd, g_opt.device,
                   f.info.compute_units, f.info.blocks, f.info.threads_per_block, ver);
    return f;
}

// one host thread per device; with one device this is a plain call
static Frame context_frame(const Scene *scene, Pix *pixels, const r1_params &p, const char *scene_name)
{
    Frame f;
    const int nd = (int)g_ctx.size();
    std::vector<int> rcs(nd, R1_OK);
    std::vector<uint64_t> rays(nd, 0);
    std::vector<double> dev_s(nd, 0.0);
    std::vector<std::string> errs(nd);
    r1_adaptive_result adapt_res;
    memset(&adapt_res, 0, sizeof(adapt_res));
    double features_s = 0.0, denoise_s = 0.0;
    auto worker = [&](int i) {
        r1_params q = p;
        q.shard = i, q.num_shards = nd;
        int rc = r1_set_scene(g_ctx[i], scene->hitables, scene->camera);
        if (rc == R1_OK && g_opt.passes > 0)
        {
            // --passes K (one device): K contiguous passes, sizes differing by at most one; pixels on the last pass only
            int32_t first = 0;
            for (int k = 0; k < g_opt.passes && rc == R1_OK; ++k)
            {
                q.spp = g_opt.spp / g_opt.passes + (k < g_opt.spp % g_opt.passes ? 1 : 0);
                const bool last = k == g_opt.passes - 1;
                rc = r1_render_pass(g_ctx[i], &q, first, last ? &pixels[0].r : nullptr, &rays[i]);
                double trace_ms = 0, total_ms = 0;
                if (rc == R1_OK && r1_last_timing(g_ctx[i], &trace_ms, &total_ms) == R1_OK)
                    dev_s[i] += total_ms * 1e-3;
                first += q.spp;
            }
        }
        else if (rc == R1_OK && g_opt.adaptive)
        {
            // --adaptive (one device): the device time is the sum over the passes
            size_t n_pass = 0;
            rc = r1_adaptive_schedule(&q, &g_opt.adapt, nullptr, 0, &n_pass);
            if (rc == R1_OK)
                rc = r1_timing_begin(g_ctx[i], (int32_t)n_pass);
            if (rc == R1_OK)
            {
                rc = r1_render_adaptive(g_ctx[i], &q, &g_opt.adapt, &pixels[0].r, &rays[i], nullptr, &adapt_res);
                double trace_ms = 0, total_ms = 0;
                const int rc2 = r1_timing_end(g_ctx[i], &trace_ms, &total_ms, nullptr);
                dev_s[i] = total_ms * 1e-3;
                rc = rc != R1_OK ? rc : rc2;
            }
        }
        else if (rc == R1_OK && g_opt.linear)
        {
            // --linear (one device): the fp32 frame, then the bytes it quantises to
            rc = r1_render_linear(g_ctx[i], &q, g_linear, &rays[i], &dev_s[i]);
            if (rc == R1_OK)
                rc = r1_quantise_linear(g_linear, (size_t)q.width * q.height * 3, &pixels[0].r);
        }
        else if (rc == R1_OK && g_opt.region) // --region (one device): the window's pixels, dense at the start of the buffer
            rc = r1_render_region(g_ctx[i], &q, &g_opt.window, &pixels[0].r, &rays[i], &dev_s[i]);
        else if (rc == R1_OK)
            rc = r1_render(g_ctx[i], &q, &pixels[0].r, &rays[i], &dev_s[i]);
        if (rc == R1_OK && g_opt.denoise) // --denoise (one device): the same frame again, rendered, guided and filtered on the device
        {
            uint64_t again = 0;
            g_denoised.assign((size_t)q.width * q.height * 3, 0.0f);
            rc = r1_render_denoised(g_ctx[i], &q, &g_opt.denoise_opt, g_denoised.data(), &again, &denoise_s);
        }
        if (rc == R1_OK && g_opt.denoise_guided) // --denoise-guided (one device): the same frame again with its variance frame, guided and filtered
        {
            uint64_t again = 0;
            g_denoised.assign((size_t)q.width * q.height * 3, 0.0f);
            rc = r1_render_denoised_guided(g_ctx[i], &q, &g_opt.guided_opt, g_denoised.data(), &again, &denoise_s);
        }
        if (rc == R1_OK && g_opt.features) // --features (one device): the feature frame of what was just rendered — the frame, or --region's window
        {
            const r1_region *const win = g_opt.region ? &g_opt.window : nullptr;
            g_features.assign(win ? (size_t)win->width * win->height : (size_t)q.width * q.height, r1_feature());
            rc = r1_render_features(g_ctx[i], &q, win, g_features.data(), &features_s);
        }
        rcs[i] = rc;
        if (rc != R1_OK)
            errs[i] = r1_last_error(); // thread-local in the library
    };
    std::vector<std::thread> th;
    for (int i = 1; i < nd; ++i)
        th.emplace_back(worker, i);
    worker(0);
    for (auto &t : th)
        t.join();
    for (int i = 0; i < nd; ++i)
    {
        f.rays += rays[i]; // rayweek1.cpp:809-813
        f.device_seconds = dev_s[i] > f.device_seconds ? dev_s[i] : f.device_seconds;
        if (rcs[i] != R1_OK && f.rc == R1_OK)
        {
            f.rc = rcs[i];
            fprintf(stderr, "%s: device %d: %s\n", scene_name, i, errs[i].c_str());
        }
    }
    if (f.rc != R1_OK)
    {
        fprintf(stderr, "%s: render failed (%d)\n", scene_name, f.rc);
        return f;
    }
    r1_last_launch_info(g_ctx[0], &f.info);
    f.lines = line("devices:        %d (first hip:%d, %d CUs, %d workgroups x %d threads)\n", nd, g_opt.device, f.info.compute_units, f.info.blocks,
                   f.info.threads_per_block);
    static const char *const kernel_names[] = {"default", "reference-form sweep", "grouped exhaustive sweep", "grouped exhaustive sweep + counters",
                                               "box tree", "box tree + counters", "wavefront", "uniform grid", "uniform grid + counters"};
    f.lines += line("kernel:         %s (%d hittable spheres, %d inner nodes)\n", f.info.kernel >= 0 && f.info.kernel <= 8 ? kernel_names[f.info.kernel] : "?",
                    f.info.spheres_active, f.info.bvh_nodes);
    if (g_opt.passes > 0)
        f.lines += line("passes:         %d\n", g_opt.passes);
    const uint64_t total_samples = (uint64_t)g_opt.width * g_opt.height * g_opt.spp;
    if (g_opt.adaptive)
        f.lines_after = line("%s adaptive: passes %d, tiles settled %d / %d, samples %llu (%.4f of cap x pixels), rays %llu (%.4f of cap x pixels)\n", scene_name,
                             adapt_res.passes, adapt_res.tiles_settled, adapt_res.tiles, (unsigned long long)adapt_res.samples,
                             (double)adapt_res.samples / (double)total_samples, (unsigned long long)f.rays, (double)f.rays / (double)total_samples);
    if (g_opt.linear)
    {
        double sum = 0;
        float top = 0;
        const size_t n = (size_t)g_opt.width * g_opt.height * 3;
        for (size_t k = 0; k < n; ++k)
            sum += g_linear[k], top = g_linear[k] > top ? g_linear[k] : top;
        f.lines_after = line("%s linear: %dx%dx3 fp32 (%.2f MB), mean %.6f, max %.6f, bytes from r1_quantise_linear\n", scene_name, g_opt.width, g_opt.height,
                             (double)n * 4 / 1e6, sum / (double)n, (double)top);
    }
    if (g_opt.region)
        f.lines_after = line("%s region: %d,%d %dx%d of %dx%d (%.4f of the frame's pixels), samples %llu, rays %llu\n", scene_name, g_opt.window.x0, g_opt.window.y0,
                             g_opt.window.width, g_opt.window.height, g_opt.width, g_opt.height,
                             (double)g_opt.window.width * g_opt.window.height / ((double)g_opt.width * g_opt.height),
                             (unsigned long long)((uint64_t)g_opt.window.width * g_opt.window.height * g_opt.spp), (unsigned long long)f.rays);
    if (g_opt.denoise)
    {
        double sum = 0;
        for (const float v : g_denoised)
            sum += v;
        f.lines_after += line("%s denoise: %d iterations, normal power 2^%d, sigma colour %g, sigma depth %g, %s, mean %.6f, device time %.3fms (render, features, filter)\n",
                              scene_name, g_opt.denoise_opt.iterations, g_opt.denoise_opt.normal_power_log2, (double)g_opt.denoise_opt.sigma_color,
                              (double)g_opt.denoise_opt.sigma_depth, (g_opt.denoise_opt.flags & R1_DENOISE_DEMODULATE) ? "demodulated" : "not demodulated",
                              sum / (double)g_denoised.size(), denoise_s * 1e3);
    }
    if (g_opt.denoise_guided)
    {
        double sum = 0;
        for (const float v : g_denoised)
            sum += v;
        const r1_denoise_opt &b = g_opt.guided_opt.base;
        f.lines_after += line("%s denoise-guided: %d iterations, normal power 2^%d, sigma colour %g, sigma depth %g, variance floor %g, %s, mean %.6f, device time %.3fms "
                              "(render with moments, features, filter)\n",
                              scene_name, b.iterations, b.normal_power_log2, (double)b.sigma_color, (double)b.sigma_depth, (double)g_opt.guided_opt.variance_floor,
                              (b.flags & R1_DENOISE_DEMODULATE) ? "demodulated" : "not demodulated", sum / (double)g_denoised.size(), denoise_s * 1e3);
    }
    if (g_opt.features)
    {
        uint64_t hits = 0, covered = 0;
        for (const r1_feature &v : g_features)
            hits += v.hits, covered += v.hits ? 1 : 0;
        f.lines_after += line("%s features: %zu pixels, %llu with a hit, coverage %.4f of the samples, device time %.3fms\n", scene_name, g_features.size(),
                              (unsigned long long)covered, (double)hits / ((double)g_features.size() * g_opt.spp), features_s * 1e3);
    }
    return f;
}

RESULT benchmark(Scene *scene, Pix *pixels, bool write_tga, const char *scene_name)
{
    RESULT result = {0, 0};
    auto t0 = std::chrono::high_resolution_clock::now(); // Timer, rayweek1.cpp:848

    const r1_params p = frame_params();
    const Frame f = g_opt.backend != 0 ? cpu_frame(scene, pixels) : (g_multi ? multi_frame(scene, pixels, p, scene_name) : context_frame(scene, pixels, p, scene_name));
    if (f.rc != R1_OK)
    {
        // the reference has no error convention: the backend has reported, return RESULT{0,0}
        g_device_seconds.push_back(0.0); // one entry per benchmark() call, failed ones included (log_json indexes by run)
        delete scene;
        return result;
    }
    result.num_rays = f.rays;
    result.elapsed_seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count(); // :891
    g_last_info = f.info;
    g_device_seconds.push_back(f.device_seconds);

    printf("%s\n", scene_name);
    printf("elapsed time:   %.3fs\n", result.elapsed_seconds);
    // (the image benchmark() hands back: the frame, or --region's window)
    const int out_w = g_opt.region ? g_opt.window.width : g_opt.width, out_h = g_opt.region ? g_opt.window.height : g_opt.height;
    printf("total samples:  %llu\n", (unsigned long long)((uint64_t)out_w * out_h * g_opt.spp));
    printf("total rays:     %llu\n", (unsigned long long)result.num_rays);
    printf("mrays/s:        %0.2f\n", result.get_mrays_per_sec());
    fputs(f.lines.c_str(), stdout);
    if (g_opt.backend == 0)
        printf("device time:    %.3fms (%0.2f mrays/s)\n", f.device_seconds * 1e3, f.device_seconds ? result.num_rays / f.device_seconds / 1e6 : 0.0);
    fputs(f.lines_after.c_str(), stdout);
    printf("\n");

    delete scene; // rayweek1.cpp:905

    if (write_tga)
    {
        char filename[128];
        snprintf(filename, sizeof(filename), "out_%s.tga", scene_name);
        r1_tga_write_rgb24(filename, out_w, out_h, &pixels[0].r); // swaps R/B in `pixels`, as the reference
        if (g_opt.linear)
        {
            snprintf(filename, sizeof(filename), "out_%s.pfm", scene_name);
            r1_pfm_write_rgb32f(filename, g_opt.width, g_opt.height, g_linear);
        }
        if (g_opt.denoise || g_opt.denoise_guided)
        {
            snprintf(filename, sizeof(filename), "out_%s_denoised.pfm", scene_name);
            r1_pfm_write_rgb32f(filename, g_opt.width, g_opt.height, g_denoised.data());
        }
        if (g_opt.features)
        {
            // three planes of the feature frame, each as RGB fp32: albedo, normal, depth (in all three channels)
            std::vector<float> plane(g_features.size() * 3);
            static const char *const names[3] = {"albedo", "normal", "depth"};
            for (int k = 0; k < 3; ++k)
            {
                for (size_t i = 0; i < g_features.size(); ++i)
                    for (int ch = 0; ch < 3; ++ch)
                        plane[3 * i + ch] = k == 0 ? g_features[i].albedo[ch] : k == 1 ? g_features[i].normal[ch] : g_features[i].depth;
                snprintf(filename, sizeof(filename), "out_%s_%s.pfm", scene_name, names[k]);
                r1_pfm_write_rgb32f(filename, out_w, out_h, plane.data());
            }
        }
    }
    return result;
}

static void log_results(const char *version, const char *scene, const RESULT *results, int num_runs) // common.h:47-77
{
    double el[32];
    uint64_t rays[32];
    for (int i = 0; i < num_runs; ++i)
        el[i] = results[i].elapsed_seconds, rays[i] = results[i].num_rays;
    r1_log_results(version, scene, el, rays, num_runs);
}

// next to the reference's out_<scene>.txt (parsed by update_readme.py) a JSON
// record with what the HIP backend can add: device count, per-run device time, and the
// roofline fractions in the survey's accounting (16 B and 16 flop per ray-sphere test).
static void log_json(const char *version, const char *scene, const RESULT *results, int num_runs)
{
    char filename[128];
    snprintf(filename, sizeof(filename), "out_%s.json", scene);
    if (g_device_seconds.size() < (size_t)num_runs)
        return;
    FILE *f = fopen(filename, "wt");
    if (!f)
        return;
    double el = 0, dev = 0;
    uint64_t rays = 0;
    const size_t first = g_device_seconds.size() - (size_t)num_runs;
    fprintf(f, "{\"version\": \"%s\", \"scene\": \"%s\", \"width\": %d, \"height\": %d, \"spp\": %d, \"devices\": %d,\n \"runs\": [", version, scene,
            g_opt.width, g_opt.height, g_opt.spp, g_opt.devices);
    for (int i = 0; i < num_runs; ++i)
    {
        fprintf(f, "%s{\"elapsed_seconds\": %.6f, \"num_rays\": %llu, \"device_seconds\": %.6f}", i ? ", " : "", results[i].elapsed_seconds,
                (unsigned long long)results[i].num_rays, g_device_seconds[first + i]);
        el += results[i].elapsed_seconds, dev += g_device_seconds[first + i], rays += results[i].num_rays;
    }
    const double per_ray = 16.0 * g_last_info.spheres_padded; // bytes == flop per ray in the survey's model
    const double rays_per_dev_s = dev > 0 ? rays / dev : 0;
    fprintf(f, "],\n \"mrays_per_s\": %.3f, \"device_mrays_per_s\": %.3f, \"spheres_padded\": %d, \"spheres_active\": %d,\n", el > 0 ? rays / el / 1e6 : 0.0,
            rays_per_dev_s / 1e6, g_last_info.spheres_padded, g_last_info.spheres_active);
    // the two device-only fractions are null for the CPU stages (devices == 0): nothing ran on a GPU
    if (g_opt.devices > 0)
        fprintf(f, " \"algorithmic_bytes_per_ray\": %.0f, \"hbm_algorithmic_fraction_of_8TBs\": %.4f, \"fp32_vector_fraction_of_157TFs\": %.4f}\n", per_ray,
                rays_per_dev_s * per_ray / 8.0e12 / (double)g_opt.devices, rays_per_dev_s * per_ray / 157.3e12 / (double)g_opt.devices);
    else
        fprintf(f, " \"algorithmic_bytes_per_ray\": %.0f, \"hbm_algorithmic_fraction_of_8TBs\": null, \"fp32_vector_fraction_of_157TFs\": null}\n", per_ray);
    fclose(f);
}

int main(int argc, const char *argv[])
{
    Options &o = g_opt;
    bool write_tga = false;
    bool passes_given = false, orbit_given = false, bounce_given = false, pulse_given = false, adapt_fields_ok = true, adapt_sub_given = false, region_fields_ok = true;
    int num_runs = 1;
    const static int MAX_NUMS = 32;
    RESULT results[MAX_NUMS];

    // the options whose value is one integer: name, target, and what is set when the option was given
    struct IntOption
    {
        const char *name;
        int *value;
        bool *given;
    };
    const IntOption int_options[] = {
        {"--width", &o.width, nullptr},         {"--height", &o.height, nullptr},     {"--spp", &o.spp, nullptr},
        {"--device", &o.device, nullptr},       {"--devices", &o.devices, nullptr},   {"--variant", &o.variant, nullptr},
        {"--pipeline", &o.pipeline, nullptr},   {"--inflight", &o.inflight, nullptr}, {"--orbit", &o.orbit, &orbit_given},
        {"--bounce", &o.bounce, &bounce_given}, {"--pulse", &o.pulse, &pulse_given},  {"--passes", &o.passes, &passes_given},
        {"--min-spp", &o.adapt.min_spp, &adapt_sub_given}, {"--pass-spp", &o.adapt.pass_spp, &adapt_sub_given},
    };
    for (int i = 1; i < argc; ++i)
    {
        if (strcmp(argv[i], "-w") == 0)
        {
            write_tga = true;
            continue;
        }
        if (strcmp(argv[i], "--linear") == 0)
        {
            o.linear = true;
            continue;
        }
        if (strcmp(argv[i], "--features") == 0)
        {
            o.features = true;
            continue;
        }
        if (strcmp(argv[i], "--denoise-guided") == 0) // (its value is optional, as --denoise's)
        {
            o.denoise_guided = o.linear = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9')
                o.guided_opt.base.iterations = atoi(argv[++i]);
            continue;
        }
        if (strcmp(argv[i], "--denoise") == 0) // (its value is optional: taken where the next argument is a number)
        {
            o.denoise = o.linear = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9')
                o.denoise_opt.iterations = atoi(argv[++i]);
            continue;
        }
        if (i + 1 >= argc)
        {
            if (strcmp(argv[i], "--region") == 0) // (ignored, it would render the whole frame)
                o.region = true, region_fields_ok = false;
            break; // every other option takes a value: as the last argument it is ignored
        }
        const char *const value = argv[i + 1];
        const IntOption *row = nullptr;
        for (const IntOption &r : int_options)
            if (strcmp(argv[i], r.name) == 0)
                row = &r;
        if (row)
        {
            *row->value = atoi(value);
            if (row->given)
                *row->given = true;
        }
        else if (strcmp(argv[i], "-n") == 0)
        {
            int n = atoi(value);
            if (n >= 1 && n < MAX_NUMS)
                num_runs = n;
            else
                printf("Invalid num_runs parameter: %d\n", n);
        }
        else if (strcmp(argv[i], "--seed") == 0)
            o.seed = (uint32_t)strtoul(value, 0, 0);
        else if (strcmp(argv[i], "--adaptive") == 0)
        {
            // MAXDELTA[,MEANQ8]
            o.adaptive = true;
            char *end = nullptr;
            o.adapt.max_delta = (int32_t)strtol(value, &end, 10);
            adapt_fields_ok = end != value;
            if (adapt_fields_ok && *end == ',')
            {
                const char *w = end + 1;
                o.adapt.mean_delta_q8 = (int32_t)strtol(w, &end, 10);
                adapt_fields_ok = end != w;
            }
            adapt_fields_ok = adapt_fields_ok && *end == 0;
        }
        else if (strcmp(argv[i], "--region") == 0)
        {
            // X,Y,W,H
            o.region = true;
            int n_read = 0;
            region_fields_ok = sscanf(value, "%d,%d,%d,%d%n", &o.window.x0, &o.window.y0, &o.window.width, &o.window.height, &n_read) == 4 && value[n_read] == 0;
        }
        else if (strcmp(argv[i], "--backend") == 0)
            o.backend = strcmp(value, "hip") == 0 ? 0 : (strcmp(value, "cpu-step1") == 0 ? 1 : (strcmp(value, "cpu-step12") == 0 ? 12 : -1));
        else if (strcmp(argv[i], "--gather") == 0)
            o.gather = strcmp(value, "rccl") == 0 ? 1 : (strcmp(value, "host") == 0 ? 0 : -2);
        else
            continue; // no option of this program: ignored
        ++i; // the value
    }
    if (o.width <= 0 || o.height <= 0 || o.spp <= 0 || o.devices < 1 || o.devices > 64 || o.gather == -2 || o.backend < 0)
    {
        fprintf(stderr, "bad --width/--height/--spp/--devices/--gather/--backend\n");
        return 1;
    }
    // what every option below needs: the hip backend and one device (no --gather rccl); all but --passes itself also no --passes
    const bool one_hip_device = o.backend == 0 && o.devices <= 1 && o.gather != 1;
    const bool one_pass = one_hip_device && !passes_given;
    const bool tree_variant = o.variant == R1_VARIANT_DEFAULT || o.variant == R1_VARIANT_BVH; // an update refits the box tree only
    if (orbit_given && (o.orbit < 1 || !one_pass || o.inflight < 1 || o.inflight > 64))
    {
        fprintf(stderr, "bad --orbit %d: needs FRAMES >= 1, the hip backend, one device (no --gather rccl), no --passes and 1 <= --inflight <= 64\n", o.orbit);
        return 1;
    }
    if (bounce_given && (o.bounce < 1 || !one_pass || o.adaptive || !tree_variant))
    {
        fprintf(stderr, "bad --bounce %d: needs FRAMES >= 1, the hip backend, one device (no --gather rccl), --variant 0 or 4 (an update refits the box tree only), "
                        "no --passes and no --adaptive\n", o.bounce);
        return 1;
    }
    if (pulse_given && (o.pulse < 1 || !one_pass || o.adaptive || !tree_variant))
    {
        fprintf(stderr, "bad --pulse %d: needs FRAMES >= 1, the hip backend, one device (no --gather rccl), --variant 0 or 4 (a change of radius refits the box tree only), "
                        "no --passes and no --adaptive\n", o.pulse);
        return 1;
    }
    if (passes_given && (o.passes < 1 || o.passes > o.spp || !one_hip_device || o.pipeline > 0))
    {
        fprintf(stderr, "bad --passes %d: needs 1 <= K <= spp (%d), the hip backend, one device (no --gather rccl) and no --pipeline\n", o.passes, o.spp);
        return 1;
    }
    if ((o.adaptive || adapt_sub_given) &&
        (!o.adaptive || !adapt_fields_ok || o.adapt.min_spp < 1 || o.adapt.pass_spp < 1 || o.adapt.max_delta < -1 || o.adapt.max_delta > 255 ||
         o.adapt.mean_delta_q8 < 0 || o.adapt.mean_delta_q8 > 65280 || !one_pass || o.pipeline > 0 || orbit_given ||
         !(tree_variant || o.variant == R1_VARIANT_PREFILTER || o.variant == R1_VARIANT_GRID)))
    {
        fprintf(stderr, "bad --adaptive MAXDELTA[,MEANQ8] / --min-spp / --pass-spp: needs -1 <= MAXDELTA <= 255, 0 <= MEANQ8 <= 65280, --min-spp and --pass-spp >= 1 "
                        "(both only with --adaptive), the hip backend, one device (no --gather rccl), --variant 0, 2, 4 or 7, and no --passes, --pipeline or --orbit\n");
        return 1;
    }

    if (o.denoise && (!one_pass || o.adaptive || o.region || !(tree_variant || o.variant == R1_VARIANT_GRID || o.variant == R1_VARIANT_REFERENCE) ||
                      o.denoise_opt.iterations < 1 || o.denoise_opt.iterations > R1_DENOISE_MAX_ITERATIONS))
    {
        fprintf(stderr, "bad --denoise [ITERATIONS]: needs 1..%d iterations, the hip backend, one device (no --gather rccl), --variant 0, 1, 4 or 7, no --passes, "
                        "no --adaptive and no --region\n", R1_DENOISE_MAX_ITERATIONS);
        return 1;
    }

    if (o.denoise_guided && (o.denoise || o.spp < 2 || !one_pass || o.adaptive || o.region ||
                             !(tree_variant || o.variant == R1_VARIANT_GRID || o.variant == R1_VARIANT_REFERENCE) || o.guided_opt.base.iterations < 1 ||
                             o.guided_opt.base.iterations > R1_DENOISE_MAX_ITERATIONS))
    {
        fprintf(stderr, "bad --denoise-guided [ITERATIONS]: needs 1..%d iterations, --spp 2 or more, the hip backend, one device (no --gather rccl), --variant 0, 1, 4 or 7, "
                        "no --denoise, no --passes, no --adaptive and no --region\n", R1_DENOISE_MAX_ITERATIONS);
        return 1;
    }

    if (o.linear && (!one_pass || o.adaptive))
    {
        fprintf(stderr, "bad --linear: needs the hip backend, one device (no --gather rccl), no --passes and no --adaptive\n");
        return 1;
    }

    if (o.features && (!one_pass || o.adaptive || !(tree_variant || o.variant == R1_VARIANT_GRID || o.variant == R1_VARIANT_REFERENCE)))
    {
        fprintf(stderr, "bad --features: needs the hip backend, one device (no --gather rccl), --variant 0, 1, 4 or 7, no --passes and no --adaptive\n");
        return 1;
    }

    if (o.region)
    {
        // what r1_render_region cannot serve is refused here, before a device is touched, as --linear's is; the window itself by r1_region_check
        if (!region_fields_ok || !one_pass || o.adaptive || o.linear)
        {
            fprintf(stderr, "bad --region X,Y,W,H: needs four integers, the hip backend, one device (no --gather rccl), no --passes, no --adaptive and no --linear\n");
            return 1;
        }
        const r1_params fp = frame_params();
        if (r1_region_check(&fp, &o.window) != R1_OK)
        {
            fprintf(stderr, "bad --region %d,%d,%d,%d: %s\n", o.window.x0, o.window.y0, o.window.width, o.window.height, r1_last_error());
            return 1;
        }
    }

    if ((o.pipeline > 0 || o.orbit > 0) && o.backend == 0)
    {
        // Frames in flight only overlap when their streams sit on different hardware queues; the ROCm default is 4.  One queue
        // per frame in flight + one for the context benchmark() renders through (two streams that share a queue run their frames
        // one after the other); at most 23: beyond that the process runs out of them.  Must be set before the first HIP call.
        char q[16];
        snprintf(q, sizeof(q), "%d", o.inflight < 1 ? 2 : (o.inflight > 22 ? 23 : o.inflight + 1));
        setenv("GPU_MAX_HW_QUEUES", q, 0);
    }
    // HIP context creation stays outside the timed region and is shared by all -n runs.
    // Devices wrap around the visible ones, so --devices 2 also works (oversubscribed) on one GPU.
    const int visible = o.backend == 0 ? r1_device_count() : 0;
    if (o.backend != 0)
        o.devices = 0, o.gather = 0; // the CPU stages touch no device
    if (o.gather == -1)
        o.gather = o.devices > 1 && o.device + o.devices <= visible ? 1 : 0; // RCCL needs distinct devices
    if (o.gather == 1)
    {
        std::vector<int32_t> devs;
        for (int i = 0; i < o.devices; ++i)
            devs.push_back(o.device + i);
        if (visible <= 0 || r1_multi_create(o.devices, devs.data(), &g_multi) != R1_OK)
        {
            fprintf(stderr, "cannot create the RCCL device group: %s\n", r1_last_error());
            return 2;
        }
    }
    for (int i = 0; i < o.devices && !g_multi; ++i)
    {
        r1_context *c = nullptr;
        if (visible <= 0 || r1_create((o.device + i) % visible, &c) != R1_OK)
        {
            fprintf(stderr, "cannot create HIP context: %s\n", r1_last_error());
            return 2;
        }
        g_ctx.push_back(c);
    }

    // The pixel buffer benchmark() fills (rayweek1.cpp:961 allocates it with new[]).  With the HIP backend it is page-locked memory
    // (r1_host_alloc).  The tiles land in it straight from the trace launch only where the launch takes the in-kernel landing
    // (Landing::used in r1_render.cpp's render_host: the big-scene kernels); every other frame is trace + resolve + one copy of the
    // image, which page-locked memory only makes faster (any other memory works too).
    Pix *pixels = nullptr;
    bool pixels_pinned = false;
    const size_t n_pixels = o.region ? (size_t)o.window.width * o.window.height : (size_t)o.width * o.height; // (--region: the window's, whatever the frame's size)
    if (o.backend == 0)
    {
        void *mem = nullptr;
        if (r1_host_alloc(n_pixels * sizeof(Pix), &mem) == R1_OK)
            pixels = (Pix *)mem, pixels_pinned = true;
    }
    if (!pixels)
        pixels = new Pix[n_pixels];
    memset(pixels, 0, n_pixels * sizeof(pixels[0]));

    bool linear_pinned = false;
    if (o.linear)
    {
        void *mem = nullptr;
        const size_t bytes = (size_t)o.width * o.height * 3 * sizeof(float);
        if (r1_host_alloc(bytes, &mem) == R1_OK)
            g_linear = (float *)mem, linear_pinned = true;
        else
            g_linear = new float[(size_t)o.width * o.height * 3];
        memset(g_linear, 0, bytes);
    }

    const char *version = o.backend == 0 ? "hip" : (o.backend == 12 ? "cpu-step12" : "cpu-step1");
    const struct
    {
        const char *name;
        int kind;
        Scene *(*create)();
    } scenes[] = {{"small", R1_SCENE_SMALL, create_small_scene}, {"medium", R1_SCENE_MEDIUM, create_medium_scene}, {"large", R1_SCENE_LARGE, create_large_scene}};

    for (const auto &s : scenes)
    {
        for (int i = 0; i < num_runs; ++i)
            results[i] = benchmark(s.create(), pixels, write_tga, s.name);
        log_results(version, s.name, results, num_runs);
        log_json(version, s.name, results, num_runs);
    }

    // the demos: FRAMES frames of every scene each, in this order
    const struct
    {
        int frames;
        Demo run;
    } demos[] = {{o.backend == 0 && o.inflight >= 1 && o.inflight <= 64 ? o.pipeline : 0, pipelined}, {o.orbit, orbit}, {o.bounce, bounce}, {o.pulse, pulse}};
    int rc_demo = 0;
    for (const auto &d : demos)
        for (const auto &s : scenes)
            if (d.frames > 0)
                rc_demo |= d.run(s.name, s.kind, d.frames, write_tga);

    if (pixels_pinned)
        r1_host_free(pixels);
    else
        delete[] pixels;
    if (linear_pinned)
        r1_host_free(g_linear);
    else
        delete[] g_linear;
    for (r1_context *c : g_ctx)
        r1_destroy(c);
    r1_multi_destroy(g_multi);
    return rc_demo ? 3 : 0;
}
