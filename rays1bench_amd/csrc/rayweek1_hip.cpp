// rayweek1_hip.cpp — the drop-in host program: the reference's entry points for the hot path
//     Scene *create_small_scene() / create_medium_scene() / create_large_scene()
//                                       (/root/reference/src/step13/rayweek1.cpp:552 / :582 / :654)
//     RESULT benchmark(Scene *scene, Pix *pixels, bool write_tga, const char *scene_name)
//                                       (rayweek1.cpp:845-927)
//     main: -w, -n N                    (rayweek1.cpp:930-988)
// kept with the same signatures, ownership (benchmark() deletes the scene it is given,
// rayweek1.cpp:905), stdout block (:895-902), out_<scene>.txt (common.h:47-77) and TGA
// (common.h:86-122), but rendering through librays1.so (include/rays1.h) on a MI355X.
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
// --backend hip (default) | cpu-step1 | cpu-step12: the reference's two single-thread CPU stages
// (r1_cpu_backends.cpp) behind the same benchmark(), for the README-style table
// (README.md:38-84).  Named backends of this program only — never a fallback: with --backend hip and no
// usable device the program exits with an error.

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rays1.h"

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

// ---- run-time configuration (the reference's SCREEN_W / SCREEN_H / NUM_SAMPLES_PER_PIXEL) --------

static int g_screen_w = 1280;
static int g_screen_h = 720;
static int g_spp = 10 * 25;
static int g_max_bounces = 50;
static uint32_t g_seed = 10001;
static int g_device = 0;
static int g_variant = R1_VARIANT_DEFAULT;
static int g_devices = 1;
static int g_backend = 0; // 0 hip, 1 cpu-step1, 12 cpu-step12
static int g_pipeline = 0; // --pipeline FRAMES: after the benchmark() runs, FRAMES frames per scene with several in flight (r1_render_async)
static int g_inflight = 20;
static int g_bounce = 0;   // --bounce FRAMES: after the benchmark() runs, FRAMES frames per scene with the lattice spheres bobbing in y, one r1_update_centers between frames
static int g_pulse = 0;    // --pulse FRAMES: after the benchmark() runs, FRAMES frames per scene with the lattice spheres' radii breathing and their albedo cycling, one r1_update_spheres between frames
static int g_orbit = 0;    // --orbit FRAMES: after the benchmark() runs, FRAMES frames per scene with the camera turned about the vertical axis through lookat (r1_render_path_async)
static int g_passes = 0;   // --passes K: every frame in K progressive passes (r1_render_pass); 0 = one r1_render
static bool g_adaptive = false; // --adaptive: every frame through r1_render_adaptive
static r1_adaptive g_adapt = {16, 16, 0, 65280};
int r1cpu_step12_render(const r1_scene *scene, const r1_camera *cam, int width, int height, int spp, int max_bounces, uint8_t *rgb,
                        uint64_t *num_rays); // r1_cpu_backends.cpp
int r1cpu_step1_render(int scene_kind, const r1_scene *scene, const r1_camera *cam, int width, int height, int spp, uint8_t *rgb,
                       uint64_t *num_rays);
static std::vector<r1_context *> g_ctx; // one per device in use (--gather host)
static r1_multi *g_multi = nullptr;     // --gather rccl
static int g_gather = -1;               // -1 auto, 0 host, 1 rccl
static std::vector<double> g_device_seconds; // per benchmark() call, for the JSON record
static r1_launch_info g_last_info;

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
    if (r1_host_scene_create(kind, g_screen_w, g_screen_h, 0, 0, &s->host) != R1_OK)
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

RESULT benchmark(Scene *scene, Pix *pixels, bool write_tga, const char *scene_name)
{
    RESULT result = {0, 0};
    auto t0 = std::chrono::high_resolution_clock::now(); // Timer, rayweek1.cpp:848

    r1_params p;
    memset(&p, 0, sizeof(p));
    p.width = g_screen_w, p.height = g_screen_h, p.spp = g_spp, p.max_bounces = g_max_bounces;
    p.seed = g_seed;
    p.tile_w = 32, p.tile_h = 32; // rayweek1.cpp:855-856
    p.shard = 0, p.num_shards = 1;
    p.variant = g_variant;

    if (g_backend != 0)
    {
        // the reference's single-thread CPU stages (r1_cpu_backends.cpp), same timer span and report
        if (g_backend == 12)
            r1cpu_step12_render(scene->hitables, scene->camera, g_screen_w, g_screen_h, g_spp, g_max_bounces, &pixels[0].r, &result.num_rays);
        else
            r1cpu_step1_render(scene->kind, scene->hitables, scene->camera, g_screen_w, g_screen_h, g_spp, &pixels[0].r, &result.num_rays);
        result.elapsed_seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        g_device_seconds.push_back(0.0);
        memset(&g_last_info, 0, sizeof(g_last_info));
        g_last_info.spheres_padded = (int32_t)scene->hitables->count;
        printf("%s\n", scene_name);
        printf("elapsed time:   %.3fs\n", result.elapsed_seconds);
        printf("total samples:  %llu\n", (unsigned long long)((uint64_t)g_screen_w * g_screen_h * g_spp));
        printf("total rays:     %llu\n", (unsigned long long)result.num_rays);
        printf("mrays/s:        %0.2f\n", result.get_mrays_per_sec());
        printf("backend:        %s (1 host thread, no GPU)\n", g_backend == 12 ? "cpu-step12" : "cpu-step1");
        printf("\n");
        delete scene; // rayweek1.cpp:905
        if (write_tga)
        {
            char filename[128];
            snprintf(filename, sizeof(filename), "out_%s.tga", scene_name);
            r1_tga_write_rgb24(filename, g_screen_w, g_screen_h, &pixels[0].r);
        }
        return result;
    }
    if (g_multi)
    {
        // tile split over the devices + one RCCL all-gather, behind one call
        double device_seconds = 0;
        int rc = r1_multi_set_scene(g_multi, scene->hitables, scene->camera);
        if (rc == R1_OK)
            rc = r1_multi_render(g_multi, &p, &pixels[0].r, &result.num_rays, &device_seconds);
        if (rc != R1_OK)
        {
            fprintf(stderr, "%s: render failed (%d): %s\n", scene_name, rc, r1_last_error());
            result.num_rays = 0;
            g_device_seconds.push_back(0.0);
            delete scene;
            return result;
        }
        result.elapsed_seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count(); // :891
        int32_t nd = 0, ver = 0;
        r1_launch_info li;
        memset(&li, 0, sizeof(li));
        r1_multi_info(g_multi, &nd, &ver, &li);
        g_last_info = li;
        g_device_seconds.push_back(device_seconds);
        printf("%s\n", scene_name);
        printf("elapsed time:   %.3fs\n", result.elapsed_seconds);
        printf("total samples:  %llu\n", (unsigned long long)((uint64_t)g_screen_w * g_screen_h * g_spp));
        printf("total rays:     %llu\n", (unsigned long long)result.num_rays);
        printf("mrays/s:        %0.2f\n", result.get_mrays_per_sec());
        printf("devices:        %d (first hip:%d, %d CUs, %d workgroups x %d threads), gather: RCCL %d all-gather\n", nd, g_device, li.compute_units,
               li.blocks, li.threads_per_block, ver);
        printf("device time:    %.3fms (%0.2f mrays/s)\n", device_seconds * 1e3, device_seconds ? result.num_rays / device_seconds / 1e6 : 0.0);
        printf("\n");
        delete scene; // rayweek1.cpp:905
        if (write_tga)
        {
            char filename[128];
            snprintf(filename, sizeof(filename), "out_%s.tga", scene_name);
            r1_tga_write_rgb24(filename, g_screen_w, g_screen_h, &pixels[0].r);
        }
        return result;
    }

    // one host thread per device; with one device this is a plain call
    const int nd = (int)g_ctx.size();
    std::vector<int> rcs(nd, R1_OK);
    std::vector<uint64_t> rays(nd, 0);
    std::vector<double> dev_s(nd, 0.0);
    std::vector<std::string> errs(nd);
    r1_adaptive_result adapt_res;
    memset(&adapt_res, 0, sizeof(adapt_res));
    auto worker = [&](int i) {
        r1_params q = p;
        q.shard = i, q.num_shards = nd;
        int rc = r1_set_scene(g_ctx[i], scene->hitables, scene->camera);
        if (rc == R1_OK && g_passes > 0)
        {
            // --passes K (one device): K contiguous passes, sizes differing by at most one; pixels on the last pass only
            int32_t first = 0;
            for (int k = 0; k < g_passes && rc == R1_OK; ++k)
            {
                q.spp = g_spp / g_passes + (k < g_spp % g_passes ? 1 : 0);
                const bool last = k == g_passes - 1;
                rc = r1_render_pass(g_ctx[i], &q, first, last ? &pixels[0].r : nullptr, &rays[i]);
                double trace_ms = 0, total_ms = 0;
                if (rc == R1_OK && r1_last_timing(g_ctx[i], &trace_ms, &total_ms) == R1_OK)
                    dev_s[i] += total_ms * 1e-3;
                first += q.spp;
            }
        }
        else if (rc == R1_OK && g_adaptive)
        {
            // --adaptive (one device): the device time is the sum over the passes
            size_t n_pass = 0;
            rc = r1_adaptive_schedule(&q, &g_adapt, nullptr, 0, &n_pass);
            if (rc == R1_OK)
                rc = r1_timing_begin(g_ctx[i], (int32_t)n_pass);
            if (rc == R1_OK)
            {
                rc = r1_render_adaptive(g_ctx[i], &q, &g_adapt, &pixels[0].r, &rays[i], nullptr, &adapt_res);
                double trace_ms = 0, total_ms = 0;
                const int rc2 = r1_timing_end(g_ctx[i], &trace_ms, &total_ms, nullptr);
                dev_s[i] = total_ms * 1e-3;
                rc = rc != R1_OK ? rc : rc2;
            }
        }
        else if (rc == R1_OK)
            rc = r1_render(g_ctx[i], &q, &pixels[0].r, &rays[i], &dev_s[i]);
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
    double device_seconds = 0;
    int rc = R1_OK;
    for (int i = 0; i < nd; ++i)
    {
        result.num_rays += rays[i]; // rayweek1.cpp:809-813
        device_seconds = dev_s[i] > device_seconds ? dev_s[i] : device_seconds;
        if (rcs[i] != R1_OK && rc == R1_OK)
        {
            rc = rcs[i];
            fprintf(stderr, "%s: device %d: %s\n", scene_name, i, errs[i].c_str());
        }
    }
    if (rc != R1_OK)
    {
        // the reference has no error convention: report and return RESULT{0,0}
        fprintf(stderr, "%s: render failed (%d)\n", scene_name, rc);
        result.num_rays = 0;
        g_device_seconds.push_back(0.0); // one entry per benchmark() call, failed ones included (log_json indexes by run)
        delete scene;
        return result;
    }
    result.elapsed_seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count(); // :891

    r1_launch_info li;
    memset(&li, 0, sizeof(li));
    r1_last_launch_info(g_ctx[0], &li);
    g_last_info = li;
    g_device_seconds.push_back(device_seconds);
    uint64_t total_samples = (uint64_t)g_screen_w * g_screen_h * g_spp;

    printf("%s\n", scene_name);
    printf("elapsed time:   %.3fs\n", result.elapsed_seconds);
    printf("total samples:  %llu\n", (unsigned long long)total_samples);
    printf("total rays:     %llu\n", (unsigned long long)result.num_rays);
    printf("mrays/s:        %0.2f\n", result.get_mrays_per_sec());
    printf("devices:        %d (first hip:%d, %d CUs, %d workgroups x %d threads)\n", nd, g_device, li.compute_units, li.blocks,
           li.threads_per_block);
    static const char *const kernel_names[] = {"default", "reference-form sweep", "grouped exhaustive sweep", "grouped exhaustive sweep + counters",
                                               "box tree", "box tree + counters", "wavefront", "uniform grid", "uniform grid + counters"};
    printf("kernel:         %s (%d hittable spheres, %d inner nodes)\n", li.kernel >= 0 && li.kernel <= 8 ? kernel_names[li.kernel] : "?",
           li.spheres_active, li.bvh_nodes);
    if (g_passes > 0)
        printf("passes:         %d\n", g_passes);
    printf("device time:    %.3fms (%0.2f mrays/s)\n", device_seconds * 1e3, device_seconds ? result.num_rays / device_seconds / 1e6 : 0.0);
    if (g_adaptive)
        printf("%s adaptive: passes %d, tiles settled %d / %d, samples %llu (%.4f of cap x pixels), rays %llu (%.4f of cap x pixels)\n", scene_name,
               adapt_res.passes, adapt_res.tiles_settled, adapt_res.tiles, (unsigned long long)adapt_res.samples, (double)adapt_res.samples / (double)total_samples,
               (unsigned long long)result.num_rays, (double)result.num_rays / (double)total_samples);
    printf("\n");

    delete scene; // rayweek1.cpp:905

    if (write_tga)
    {
        char filename[128];
        snprintf(filename, sizeof(filename), "out_%s.tga", scene_name);
        r1_tga_write_rgb24(filename, g_screen_w, g_screen_h, &pixels[0].r); // swaps R/B in `pixels`, as the reference
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
            g_screen_w, g_screen_h, g_spp, g_devices);
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
    if (g_devices > 0)
        fprintf(f, " \"algorithmic_bytes_per_ray\": %.0f, \"hbm_algorithmic_fraction_of_8TBs\": %.4f, \"fp32_vector_fraction_of_157TFs\": %.4f}\n", per_ray,
                rays_per_dev_s * per_ray / 8.0e12 / (double)g_devices, rays_per_dev_s * per_ray / 157.3e12 / (double)g_devices);
    else
        fprintf(f, " \"algorithmic_bytes_per_ray\": %.0f, \"hbm_algorithmic_fraction_of_8TBs\": null, \"fp32_vector_fraction_of_157TFs\": null}\n", per_ray);
    fclose(f);
}

// ---- frames in flight from the C++ host (no reference counterpart: benchmark() renders ONE frame and waits) --------
// The `-n` runs of main (rayweek1.cpp:969-984) are independent frames.  Rendered one after the other each pays the
// tail of its own longest bounce chains; kept in flight — one context, stream and page-locked pixel buffer per frame,
// r1_render_async — the next frames fill the chip while one drains, and every frame still ends with its pixels and
// ray count on the host (the Timer span of rayweek1.cpp:848 -> :891, pipelined).  Prints one line per scene.
static int pipelined(const char *scene_name, int kind, int frames)
{
    const int k = g_inflight < frames ? g_inflight : frames;
    const bool multi = g_gather == 1 && g_devices >= 1 && g_multi; // --gather rccl: every frame in flight is split over the N devices (r1_multi)
    r1_host_scene *hs = nullptr;
    if (r1_host_scene_create(kind, g_screen_w, g_screen_h, 0, 0, &hs) != R1_OK)
        return 1;
    r1_params p;
    memset(&p, 0, sizeof(p));
    p.width = g_screen_w, p.height = g_screen_h, p.spp = g_spp, p.max_bounces = g_max_bounces, p.seed = g_seed;
    p.tile_w = 32, p.tile_h = 32, p.shard = 0, p.num_shards = 1, p.variant = g_variant;
    const size_t rec = r1_frame_record_bytes(&p); // image, padded to 8 bytes, + uint64 ray count
    std::vector<r1_context *> ctx((size_t)k, nullptr);
    std::vector<r1_multi *> mul((size_t)k, nullptr);
    std::vector<uint8_t *> host((size_t)k, nullptr);
    int rc = R1_OK;
    const int visible = r1_device_count();
    std::vector<int32_t> devs;
    for (int i = 0; i < g_devices; ++i)
        devs.push_back(g_device + i);
    for (int i = 0; i < k && rc == R1_OK; ++i) // every context first, the scenes afterwards: the streams get their own hardware queues
        rc = multi ? r1_multi_create(g_devices, devs.data(), &mul[(size_t)i]) : r1_create(g_device % (visible > 0 ? visible : 1), &ctx[(size_t)i]);
    for (int i = 0; i < k && rc == R1_OK; ++i)
    {
        rc = multi ? r1_multi_set_scene(mul[(size_t)i], r1_host_scene_spheres(hs), r1_host_scene_camera(hs))
                   : r1_set_scene(ctx[(size_t)i], r1_host_scene_spheres(hs), r1_host_scene_camera(hs));
        if (rc == R1_OK)
            rc = r1_host_alloc(rec, (void **)&host[(size_t)i]);
    }
    auto enqueue = [&](size_t s) {
        return multi ? r1_multi_render_async(mul[s], &p, host[s]) : r1_render_async(ctx[s], &p, host[s], (uint64_t *)(host[s] + rec - 8), nullptr);
    };
    auto wait = [&](size_t s) { return multi ? r1_multi_sync(mul[s]) : r1_sync(ctx[s]); };
    uint64_t rays = 0;
    double secs = 0;
    if (rc == R1_OK)
    {
        for (int pass = 0; pass < 2 && rc == R1_OK; ++pass) // pass 0: workspaces and queues (not timed)
        {
            rays = 0;
            const int n = pass ? frames : k;
            auto t0 = std::chrono::high_resolution_clock::now();
            for (int f = 0; f < n && rc == R1_OK; ++f)
            {
                const size_t s = (size_t)(f % k);
                if (f >= k) // the slot's previous frame has to have landed before its buffer is reused
                {
                    rc = wait(s);
                    rays += *(const uint64_t *)(host[s] + rec - 8);
                }
                if (rc == R1_OK)
                    rc = enqueue(s);
            }
            for (int i = 0; i < k && rc == R1_OK; ++i)
            {
                rc = wait((size_t)i);
                if (i < n)
                    rays += *(const uint64_t *)(host[(size_t)i] + rec - 8);
            }
            secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        }
    }
    if (rc == R1_OK)
        printf("%s pipelined:  %d frames, %d in flight%s, %.3f ms per frame, %llu rays, %0.2f mrays/s (pixels + count on the host)\n", scene_name, frames,
               k, multi ? " (each split over the devices, RCCL all-gather)" : "", secs / frames * 1e3, (unsigned long long)rays, rays / secs / 1e6);
    else
        fprintf(stderr, "pipelined %s: %s\n", scene_name, r1_last_error());
    for (int i = 0; i < k; ++i)
    {
        r1_host_free(host[(size_t)i]);
        r1_destroy(ctx[(size_t)i]);
        r1_multi_destroy(mul[(size_t)i]);
    }
    r1_host_scene_destroy(hs);
    return rc == R1_OK ? 0 : 1;
}

// ---- a moving camera (no reference counterpart: its camera is fixed when the scene is built) -------------------------
// --orbit FRAMES: the scene's own camera (r1_host_scene_view) turned about the vertical axis through lookat, frame f at angle 2 pi f / FRAMES
// (frame 0 is the scene's camera bit for bit: cos 0 = 1, sin 0 = 0), every frame with benchmark()'s seed.  The frames are rendered as camera-path
// batches — consecutive frames of the orbit in ONE launch, each through its own camera (r1_render_path_async) — over --inflight contexts, the
// records landing in page-locked memory.  Prints one line per scene; with -w writes frame 0 and the middle frame.
static int orbit(const char *scene_name, int kind, int frames, bool write_tga)
{
    r1_host_scene *hs = nullptr;
    if (r1_host_scene_create(kind, g_screen_w, g_screen_h, 0, 0, &hs) != R1_OK)
        return 1;
    r1_params p;
    memset(&p, 0, sizeof(p));
    p.width = g_screen_w, p.height = g_screen_h, p.spp = g_spp, p.max_bounces = g_max_bounces, p.seed = g_seed;
    p.tile_w = 32, p.tile_h = 32, p.shard = 0, p.num_shards = 1, p.variant = g_variant;
    float from[3], at[3], up[3], vfov = 0, aperture = 0, focus = 0;
    int rc = r1_host_scene_view(hs, from, at, up, &vfov, &aperture, &focus);
    std::vector<r1_camera> cams((size_t)frames);
    for (int f = 0; f < frames && rc == R1_OK; ++f)
    {
        const double a = 2.0 * M_PI * (double)f / (double)frames;
        const float cs = (float)cos(a), sn = (float)sin(a);
        const float dx = from[0] - at[0], dz = from[2] - at[2];
        const float eye[3] = {at[0] + (dx * cs + dz * sn), from[1], at[2] + (dz * cs - dx * sn)};
        rc = r1_camera_look_at(eye, at, up, vfov, (float)g_screen_w / (float)g_screen_h, aperture, focus, &cams[(size_t)f]);
    }
    // frames per launch: the orbit dealt evenly to the contexts, at most 16 (all frames of a launch are delivered together) and within the
    // 2^31 padded sample slots of a launch
    const int k = g_inflight < frames ? g_inflight : frames;
    const uint64_t slots = (uint64_t)((g_screen_w + 31) / 32) * (uint64_t)((g_screen_h + 31) / 32) * 1024u * (uint64_t)g_spp;
    int per = (frames + k - 1) / k;
    per = per > 16 ? 16 : per;
    if (slots && (uint64_t)per * slots >= ((uint64_t)1 << 31))
        per = (int)((((uint64_t)1 << 31) - 1) / slots);
    per = per < 1 ? 1 : per;
    const int launches = (frames + per - 1) / per;
    const size_t rec = r1_frame_record_bytes(&p); // image, padded to 8 bytes, + uint64 ray count
    const size_t img_bytes = (size_t)g_screen_w * g_screen_h * 3;
    std::vector<r1_context *> ctx((size_t)k, nullptr);
    std::vector<uint8_t *> host((size_t)k, nullptr);
    const int visible = r1_device_count();
    for (int i = 0; i < k && rc == R1_OK; ++i) // every context first, the scenes afterwards: the streams get their own hardware queues
        rc = r1_create(g_device % (visible > 0 ? visible : 1), &ctx[(size_t)i]);
    for (int i = 0; i < k && rc == R1_OK; ++i)
    {
        rc = r1_set_scene(ctx[(size_t)i], r1_host_scene_spheres(hs), r1_host_scene_camera(hs));
        if (rc == R1_OK)
            rc = r1_host_alloc(rec * (size_t)per, (void **)&host[(size_t)i]);
    }
    const int keep_frame[2] = {0, frames / 2}; // -w: the frames written afterwards
    std::vector<uint8_t> keep[2];
    uint64_t rays = 0;
    double secs = 0;
    auto landed = [&](int launch) { // the launch's records are on the host: count its rays, keep the frames that are written
        const size_t s = (size_t)(launch % k);
        const int f0 = launch * per, n = frames - f0 < per ? frames - f0 : per;
        for (int i = 0; i < n; ++i)
        {
            rays += *(const uint64_t *)(host[s] + (size_t)(i + 1) * rec - 8);
            for (int w = 0; w < 2; ++w)
                if (write_tga && f0 + i == keep_frame[w])
                    keep[w].assign(host[s] + (size_t)i * rec, host[s] + (size_t)i * rec + img_bytes);
        }
    };
    for (int pass = 0; pass < 2 && rc == R1_OK; ++pass) // pass 0: workspaces and queues (not timed)
    {
        rays = 0;
        const int n = pass ? launches : (k < launches ? k : launches);
        auto t0 = std::chrono::high_resolution_clock::now();
        for (int l = 0; l < n && rc == R1_OK; ++l)
        {
            const size_t s = (size_t)(l % k);
            if (l >= k) // the slot's previous launch has to have landed before its buffer is reused
            {
                rc = r1_sync(ctx[s]);
                landed(l - k);
            }
            const int f0 = l * per;
            if (rc == R1_OK)
                rc = r1_render_path_async(ctx[s], &p, frames - f0 < per ? frames - f0 : per, 0u, &cams[(size_t)f0], host[s], nullptr);
        }
        for (int l = n > k ? n - k : 0; l < n && rc == R1_OK; ++l)
        {
            rc = r1_sync(ctx[(size_t)(l % k)]);
            landed(l);
        }
        secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    }
    if (rc == R1_OK)
        printf("%s orbit:  %d frames, %d per launch, %d in flight, %.3f ms per frame, %llu rays, %0.2f mrays/s (one camera per frame, pixels + count on the host)\n",
               scene_name, frames, per, k, secs / frames * 1e3, (unsigned long long)rays, rays / secs / 1e6);
    else
        fprintf(stderr, "orbit %s: %s\n", scene_name, r1_last_error());
    for (int w = 0; w < 2 && rc == R1_OK && write_tga; ++w)
        if (!keep[w].empty() && (w == 0 || keep_frame[1] != keep_frame[0]))
        {
            char filename[128];
            snprintf(filename, sizeof(filename), "orbit_%s_%03d.tga", scene_name, keep_frame[w]);
            r1_tga_write_rgb24(filename, g_screen_w, g_screen_h, keep[w].data());
        }
    for (int i = 0; i < k; ++i)
    {
        r1_host_free(host[(size_t)i]);
        r1_destroy(ctx[(size_t)i]);
    }
    r1_host_scene_destroy(hs);
    return rc == R1_OK ? 0 : 1;
}

// ---- moving spheres (no reference counterpart: its scenes are fixed when they are built) ------------------------------
// --bounce FRAMES: the lattice spheres — every hittable sphere but the four largest (the ground and the three big balls) — bob in y.  Sphere i
// (scene index) of radius r_i sits in frame f at
//      y_i(f) = y_i + (r_i / 2) * (1 + sin(2 pi (f / FRAMES + (i mod 8) / 8)))
// evaluated in fp64 and rounded to fp32: eight phase groups, half a radius of amplitude, one period over the run; no clock, no random number.
// One r1_update_centers is enqueued between frames and nothing else about the scene is touched: the box tree is refitted on the device, never
// rebuilt.  Every frame with benchmark()'s seed, through r1_render_async into page-locked memory.  Prints one `bounce:` line per scene with the
// mean time of an update (enqueue to stream idle) and of a frame; with -w writes frame 0 and the middle frame.
static int bounce(const char *scene_name, int kind, int frames, bool write_tga)
{
    r1_host_scene *hs = nullptr;
    if (r1_host_scene_create(kind, g_screen_w, g_screen_h, 0, 0, &hs) != R1_OK)
        return 1;
    const r1_scene *sc = r1_host_scene_spheres(hs);
    r1_params p;
    memset(&p, 0, sizeof(p));
    p.width = g_screen_w, p.height = g_screen_h, p.spp = g_spp, p.max_bounces = g_max_bounces, p.seed = g_seed;
    p.tile_w = 32, p.tile_h = 32, p.shard = 0, p.num_shards = 1, p.variant = g_variant;
    // the four largest hittable spheres stay where they are
    std::vector<uint32_t> act;
    for (uint32_t i = 0; i < sc->count; ++i)
        if (sc->inv_radius[i] != 0)
            act.push_back(i);
    std::stable_sort(act.begin(), act.end(), [&](uint32_t a, uint32_t b) { return sc->radius_sq[a] > sc->radius_sq[b]; });
    std::vector<char> bobs(sc->count ? sc->count : 1, 0);
    for (size_t k = 4; k < act.size(); ++k)
        bobs[act[k]] = 1;
    std::vector<float> y(sc->center_y, sc->center_y + sc->count);
    const size_t img_bytes = (size_t)g_screen_w * g_screen_h * 3, rec = r1_frame_record_bytes(&p);
    r1_context *ctx = nullptr;
    uint8_t *host = nullptr;
    const int visible = r1_device_count();
    int rc = r1_create(g_device % (visible > 0 ? visible : 1), &ctx);
    if (rc == R1_OK)
        rc = r1_set_scene(ctx, sc, r1_host_scene_camera(hs));
    if (rc == R1_OK)
        rc = r1_host_alloc(rec, (void **)&host);
    const int keep_frame[2] = {0, frames / 2};
    std::vector<uint8_t> keep[2];
    uint64_t rays = 0;
    double t_update = 0, t_render = 0;
    for (int f = -1; f < frames && rc == R1_OK; ++f) // f = -1: workspaces and queues (frame 0 once more, not timed)
    {
        const int ff = f < 0 ? 0 : f;
        for (uint32_t i = 0; i < sc->count; ++i)
            if (bobs[i])
            {
                const double r = sqrt((double)sc->radius_sq[i]);
                y[i] = (float)((double)sc->center_y[i] + 0.5 * r * (1.0 + sin(2.0 * M_PI * ((double)ff / (double)frames + (double)(i % 8u) / 8.0))));
            }
        auto t0 = std::chrono::high_resolution_clock::now();
        rc = r1_update_centers(ctx, 0, sc->count, sc->center_x, y.data(), sc->center_z, nullptr);
        if (rc == R1_OK)
            rc = r1_sync(ctx);
        auto t1 = std::chrono::high_resolution_clock::now();
        if (rc == R1_OK)
            rc = r1_render_async(ctx, &p, host, (uint64_t *)(host + rec - 8), nullptr);
        if (rc == R1_OK)
            rc = r1_sync(ctx);
        auto t2 = std::chrono::high_resolution_clock::now();
        if (f < 0 || rc != R1_OK)
            continue;
        t_update += std::chrono::duration<double>(t1 - t0).count(), t_render += std::chrono::duration<double>(t2 - t1).count();
        rays += *(const uint64_t *)(host + rec - 8);
        for (int w = 0; w < 2; ++w)
            if (write_tga && f == keep_frame[w])
                keep[w].assign(host, host + img_bytes);
    }
    if (rc == R1_OK)
        printf("%s bounce: %d frames, %zu of %u spheres moving, update %.3f ms per frame (enqueue to idle), render %.3f ms per frame, %llu rays, %0.2f mrays/s\n",
               scene_name, frames, act.size() > 4 ? act.size() - 4 : (size_t)0, sc->count, t_update / frames * 1e3, t_render / frames * 1e3,
               (unsigned long long)rays, rays / (t_update + t_render) / 1e6);
    else
        fprintf(stderr, "bounce %s: %s\n", scene_name, r1_last_error());
    for (int w = 0; w < 2 && rc == R1_OK && write_tga; ++w)
        if (!keep[w].empty() && (w == 0 || keep_frame[1] != keep_frame[0]))
        {
            char filename[128];
            snprintf(filename, sizeof(filename), "bounce_%s_%03d.tga", scene_name, keep_frame[w]);
            r1_tga_write_rgb24(filename, g_screen_w, g_screen_h, keep[w].data());
        }
    r1_host_free(host);
    r1_destroy(ctx);
    r1_host_scene_destroy(hs);
    return rc == R1_OK ? 0 : 1;
}

// --pulse FRAMES: the lattice spheres (as for --bounce) breathe and change colour.  In frame f, with t = f / FRAMES, sphere i (scene index) has
//      radius  r_i * (1 + 0.3 sin(2 pi t) cos(2 pi (i mod 8) / 8))          stored as SphereSOA::add stores a radius: r * r and 1 / r in fp32
//      albedo  a_i + (a_i rotated r -> g -> b -> r  -  a_i) * (1 - cos(2 pi t)) / 2
// the factors evaluated in fp64 and rounded to fp32; a factor of exactly 1 (frame 0) keeps the scene's own pair, so frame 0 is benchmark()'s
// frame.  Material types and parameters stay.  One r1_update_spheres (radii and materials of every sphere) is enqueued between frames: the
// box tree is refitted on the device, never rebuilt.  Prints one `pulse:` line per scene; with -w writes frame 0 and the middle frame.
static int pulse(const char *scene_name, int kind, int frames, bool write_tga)
{
    r1_host_scene *hs = nullptr;
    if (r1_host_scene_create(kind, g_screen_w, g_screen_h, 0, 0, &hs) != R1_OK)
        return 1;
    const r1_scene *sc = r1_host_scene_spheres(hs);
    r1_params p;
    memset(&p, 0, sizeof(p));
    p.width = g_screen_w, p.height = g_screen_h, p.spp = g_spp, p.max_bounces = g_max_bounces, p.seed = g_seed;
    p.tile_w = 32, p.tile_h = 32, p.shard = 0, p.num_shards = 1, p.variant = g_variant;
    // the four largest hittable spheres stay as they are
    std::vector<uint32_t> act;
    for (uint32_t i = 0; i < sc->count; ++i)
        if (sc->inv_radius[i] != 0)
            act.push_back(i);
    std::stable_sort(act.begin(), act.end(), [&](uint32_t a, uint32_t b) { return sc->radius_sq[a] > sc->radius_sq[b]; });
    std::vector<char> pulses(sc->count ? sc->count : 1, 0);
    for (size_t k = 4; k < act.size(); ++k)
        pulses[act[k]] = 1;
    std::vector<float> rsq(sc->radius_sq, sc->radius_sq + sc->count), inv(sc->inv_radius, sc->inv_radius + sc->count);
    std::vector<float> ar(sc->albedo_r, sc->albedo_r + sc->count), ag(sc->albedo_g, sc->albedo_g + sc->count), ab(sc->albedo_b, sc->albedo_b + sc->count);
    const size_t img_bytes = (size_t)g_screen_w * g_screen_h * 3, rec = r1_frame_record_bytes(&p);
    r1_context *ctx = nullptr;
    uint8_t *host = nullptr;
    const int visible = r1_device_count();
    int rc = r1_create(g_device % (visible > 0 ? visible : 1), &ctx);
    if (rc == R1_OK)
        rc = r1_set_scene(ctx, sc, r1_host_scene_camera(hs));
    if (rc == R1_OK)
        rc = r1_host_alloc(rec, (void **)&host);
    const int keep_frame[2] = {0, frames / 2};
    std::vector<uint8_t> keep[2];
    uint64_t rays = 0;
    double t_update = 0, t_render = 0;
    for (int f = -1; f < frames && rc == R1_OK; ++f) // f = -1: workspaces and queues (frame 0 once more, not timed)
    {
        const int ff = f < 0 ? 0 : f;
        const double t = (double)ff / (double)frames, swing = 0.3 * sin(2.0 * M_PI * t), mix = 0.5 * (1.0 - cos(2.0 * M_PI * t));
        for (uint32_t i = 0; i < sc->count; ++i)
            if (pulses[i])
            {
                const double scale = 1.0 + swing * cos(2.0 * M_PI * (double)(i % 8u) / 8.0);
                rsq[i] = sc->radius_sq[i], inv[i] = sc->inv_radius[i];
                if (scale != 1.0)
                {
                    const float r = (float)(scale / (double)sc->inv_radius[i]);
                    rsq[i] = r * r, inv[i] = 1.0f / r;
                }
                const float a[3] = {sc->albedo_r[i], sc->albedo_g[i], sc->albedo_b[i]};
                ar[i] = (float)((double)a[0] + ((double)a[2] - (double)a[0]) * mix);
                ag[i] = (float)((double)a[1] + ((double)a[0] - (double)a[1]) * mix);
                ab[i] = (float)((double)a[2] + ((double)a[1] - (double)a[2]) * mix);
            }
        r1_sphere_update u;
        memset(&u, 0, sizeof(u));
        u.radius_sq = rsq.data(), u.inv_radius = inv.data();
        u.mat_type = sc->mat_type, u.albedo_r = ar.data(), u.albedo_g = ag.data(), u.albedo_b = ab.data(), u.mat_param = sc->mat_param;
        auto t0 = std::chrono::high_resolution_clock::now();
        rc = r1_update_spheres(ctx, 0, sc->count, &u, nullptr);
        if (rc == R1_OK)
            rc = r1_sync(ctx);
        auto t1 = std::chrono::high_resolution_clock::now();
        if (rc == R1_OK)
            rc = r1_render_async(ctx, &p, host, (uint64_t *)(host + rec - 8), nullptr);
        if (rc == R1_OK)
            rc = r1_sync(ctx);
        auto t2 = std::chrono::high_resolution_clock::now();
        if (f < 0 || rc != R1_OK)
            continue;
        t_update += std::chrono::duration<double>(t1 - t0).count(), t_render += std::chrono::duration<double>(t2 - t1).count();
        rays += *(const uint64_t *)(host + rec - 8);
        for (int w = 0; w < 2; ++w)
            if (write_tga && f == keep_frame[w])
                keep[w].assign(host, host + img_bytes);
    }
    if (rc == R1_OK)
        printf("%s pulse: %d frames, %zu of %u spheres pulsing, update %.3f ms per frame (enqueue to idle), render %.3f ms per frame, %llu rays, %0.2f mrays/s\n",
               scene_name, frames, act.size() > 4 ? act.size() - 4 : (size_t)0, sc->count, t_update / frames * 1e3, t_render / frames * 1e3,
               (unsigned long long)rays, rays / (t_update + t_render) / 1e6);
    else
        fprintf(stderr, "pulse %s: %s\n", scene_name, r1_last_error());
    for (int w = 0; w < 2 && rc == R1_OK && write_tga; ++w)
        if (!keep[w].empty() && (w == 0 || keep_frame[1] != keep_frame[0]))
        {
            char filename[128];
            snprintf(filename, sizeof(filename), "pulse_%s_%03d.tga", scene_name, keep_frame[w]);
            r1_tga_write_rgb24(filename, g_screen_w, g_screen_h, keep[w].data());
        }
    r1_host_free(host);
    r1_destroy(ctx);
    r1_host_scene_destroy(hs);
    return rc == R1_OK ? 0 : 1;
}

int main(int argc, const char *argv[])
{
    bool write_tga = false;
    bool passes_given = false, orbit_given = false, bounce_given = false, pulse_given = false, adapt_fields_ok = true, adapt_sub_given = false;
    int num_runs = 1;
    const static int MAX_NUMS = 32;
    RESULT results[MAX_NUMS];

    for (int i = 1; i < argc; ++i)
    {
        if (strcmp(argv[i], "-w") == 0)
            write_tga = true;
        else if (strcmp(argv[i], "-n") == 0 && i + 1 < argc)
        {
            int n = atoi(argv[++i]);
            if (n >= 1 && n < MAX_NUMS)
                num_runs = n;
            else
                printf("Invalid num_runs parameter: %d\n", n);
        }
        else if (strcmp(argv[i], "--width") == 0 && i + 1 < argc)
            g_screen_w = atoi(argv[++i]);
        else if (strcmp(argv[i], "--height") == 0 && i + 1 < argc)
            g_screen_h = atoi(argv[++i]);
        else if (strcmp(argv[i], "--spp") == 0 && i + 1 < argc)
            g_spp = atoi(argv[++i]);
        else if (strcmp(argv[i], "--seed") == 0 && i + 1 < argc)
            g_seed = (uint32_t)strtoul(argv[++i], 0, 0);
        else if (strcmp(argv[i], "--device") == 0 && i + 1 < argc)
            g_device = atoi(argv[++i]);
        else if (strcmp(argv[i], "--devices") == 0 && i + 1 < argc)
            g_devices = atoi(argv[++i]);
        else if (strcmp(argv[i], "--variant") == 0 && i + 1 < argc)
            g_variant = atoi(argv[++i]);
        else if (strcmp(argv[i], "--pipeline") == 0 && i + 1 < argc)
            g_pipeline = atoi(argv[++i]);
        else if (strcmp(argv[i], "--inflight") == 0 && i + 1 < argc)
            g_inflight = atoi(argv[++i]);
        else if (strcmp(argv[i], "--orbit") == 0 && i + 1 < argc)
        {
            g_orbit = atoi(argv[++i]);
            orbit_given = true;
        }
        else if (strcmp(argv[i], "--bounce") == 0 && i + 1 < argc)
        {
            g_bounce = atoi(argv[++i]);
            bounce_given = true;
        }
        else if (strcmp(argv[i], "--pulse") == 0 && i + 1 < argc)
        {
            g_pulse = atoi(argv[++i]);
            pulse_given = true;
        }
        else if (strcmp(argv[i], "--passes") == 0 && i + 1 < argc)
        {
            g_passes = atoi(argv[++i]);
            passes_given = true;
        }
        else if (strcmp(argv[i], "--adaptive") == 0 && i + 1 < argc)
        {
            // MAXDELTA[,MEANQ8]
            g_adaptive = true;
            const char *v = argv[++i];
            char *end = nullptr;
            g_adapt.max_delta = (int32_t)strtol(v, &end, 10);
            adapt_fields_ok = end != v;
            if (adapt_fields_ok && *end == ',')
            {
                const char *w = end + 1;
                g_adapt.mean_delta_q8 = (int32_t)strtol(w, &end, 10);
                adapt_fields_ok = end != w;
            }
            adapt_fields_ok = adapt_fields_ok && *end == 0;
        }
        else if (strcmp(argv[i], "--min-spp") == 0 && i + 1 < argc)
            g_adapt.min_spp = atoi(argv[++i]), adapt_sub_given = true;
        else if (strcmp(argv[i], "--pass-spp") == 0 && i + 1 < argc)
            g_adapt.pass_spp = atoi(argv[++i]), adapt_sub_given = true;
        else if (strcmp(argv[i], "--backend") == 0 && i + 1 < argc)
        {
            const char *b = argv[++i];
            g_backend = strcmp(b, "hip") == 0 ? 0 : (strcmp(b, "cpu-step1") == 0 ? 1 : (strcmp(b, "cpu-step12") == 0 ? 12 : -1));
        }
        else if (strcmp(argv[i], "--gather") == 0 && i + 1 < argc)
        {
            const char *g = argv[++i];
            g_gather = strcmp(g, "rccl") == 0 ? 1 : (strcmp(g, "host") == 0 ? 0 : -2);
        }
    }
    if (g_screen_w <= 0 || g_screen_h <= 0 || g_spp <= 0 || g_devices < 1 || g_devices > 64 || g_gather == -2 || g_backend < 0)
    {
        fprintf(stderr, "bad --width/--height/--spp/--devices/--gather/--backend\n");
        return 1;
    }
    if (orbit_given && (g_orbit < 1 || g_backend != 0 || g_devices > 1 || g_gather == 1 || passes_given || g_inflight < 1 || g_inflight > 64))
    {
        fprintf(stderr, "bad --orbit %d: needs FRAMES >= 1, the hip backend, one device (no --gather rccl), no --passes and 1 <= --inflight <= 64\n", g_orbit);
        return 1;
    }
    if (bounce_given && (g_bounce < 1 || g_backend != 0 || g_devices > 1 || g_gather == 1 || passes_given || g_adaptive ||
                         !(g_variant == R1_VARIANT_DEFAULT || g_variant == R1_VARIANT_BVH)))
    {
        fprintf(stderr, "bad --bounce %d: needs FRAMES >= 1, the hip backend, one device (no --gather rccl), --variant 0 or 4 (an update refits the box tree only), "
                        "no --passes and no --adaptive\n", g_bounce);
        return 1;
    }
    if (pulse_given && (g_pulse < 1 || g_backend != 0 || g_devices > 1 || g_gather == 1 || passes_given || g_adaptive ||
                        !(g_variant == R1_VARIANT_DEFAULT || g_variant == R1_VARIANT_BVH)))
    {
        fprintf(stderr, "bad --pulse %d: needs FRAMES >= 1, the hip backend, one device (no --gather rccl), --variant 0 or 4 (a change of radius refits the box tree only), "
                        "no --passes and no --adaptive\n", g_pulse);
        return 1;
    }
    if (passes_given && (g_passes < 1 || g_passes > g_spp || g_backend != 0 || g_devices > 1 || g_gather == 1 || g_pipeline > 0))
    {
        fprintf(stderr, "bad --passes %d: needs 1 <= K <= spp (%d), the hip backend, one device (no --gather rccl) and no --pipeline\n", g_passes, g_spp);
        return 1;
    }
    if ((g_adaptive || adapt_sub_given) && (!g_adaptive || !adapt_fields_ok || g_adapt.min_spp < 1 || g_adapt.pass_spp < 1 || g_adapt.max_delta < -1 || g_adapt.max_delta > 255 ||
                                            g_adapt.mean_delta_q8 < 0 || g_adapt.mean_delta_q8 > 65280 || g_backend != 0 || g_devices > 1 || g_gather == 1 || passes_given ||
                                            g_pipeline > 0 || orbit_given ||
                                            !(g_variant == R1_VARIANT_DEFAULT || g_variant == R1_VARIANT_PREFILTER || g_variant == R1_VARIANT_BVH || g_variant == R1_VARIANT_GRID)))
    {
        fprintf(stderr, "bad --adaptive MAXDELTA[,MEANQ8] / --min-spp / --pass-spp: needs -1 <= MAXDELTA <= 255, 0 <= MEANQ8 <= 65280, --min-spp and --pass-spp >= 1 "
                        "(both only with --adaptive), the hip backend, one device (no --gather rccl), --variant 0, 2, 4 or 7, and no --passes, --pipeline or --orbit\n");
        return 1;
    }

    if ((g_pipeline > 0 || g_orbit > 0) && g_backend == 0)
    {
        // Frames in flight only overlap when their streams sit on different hardware queues; the ROCm default is 4.  One queue
        // per frame in flight + one for the context benchmark() renders through (two streams that share a queue run their frames
        // one after the other); at most 23: beyond that the process runs out of them.  Must be set before the first HIP call.
        char q[16];
        snprintf(q, sizeof(q), "%d", g_inflight < 1 ? 2 : (g_inflight > 22 ? 23 : g_inflight + 1));
        setenv("GPU_MAX_HW_QUEUES", q, 0);
    }
    // HIP context creation stays outside the timed region and is shared by all -n runs.
    // Devices wrap around the visible ones, so --devices 2 also works (oversubscribed) on one GPU.
    const int visible = g_backend == 0 ? r1_device_count() : 0;
    if (g_backend != 0)
        g_devices = 0, g_gather = 0; // the CPU stages touch no device
    if (g_gather == -1)
        g_gather = g_devices > 1 && g_device + g_devices <= visible ? 1 : 0; // RCCL needs distinct devices
    if (g_gather == 1)
    {
        std::vector<int32_t> devs;
        for (int i = 0; i < g_devices; ++i)
            devs.push_back(g_device + i);
        if (visible <= 0 || r1_multi_create(g_devices, devs.data(), &g_multi) != R1_OK)
        {
            fprintf(stderr, "cannot create the RCCL device group: %s\n", r1_last_error());
            return 2;
        }
    }
    for (int i = 0; i < g_devices && !g_multi; ++i)
    {
        r1_context *c = nullptr;
        if (visible <= 0 || r1_create((g_device + i) % visible, &c) != R1_OK)
        {
            fprintf(stderr, "cannot create HIP context: %s\n", r1_last_error());
            return 2;
        }
        g_ctx.push_back(c);
    }

    // The pixel buffer benchmark() fills (rayweek1.cpp:961 allocates it with new[]).  With the HIP backend it is page-locked memory
    // (r1_host_alloc): the trace launch then stores every finished tile straight into it and r1_render copies nothing
    // (include/rays1.h; any other memory works too and costs one copy of the image per frame).
    Pix *pixels = nullptr;
    bool pixels_pinned = false;
    if (g_backend == 0)
    {
        void *mem = nullptr;
        if (r1_host_alloc((size_t)g_screen_w * g_screen_h * sizeof(Pix), &mem) == R1_OK)
            pixels = (Pix *)mem, pixels_pinned = true;
    }
    if (!pixels)
        pixels = new Pix[(size_t)g_screen_w * g_screen_h];
    memset(pixels, 0, (size_t)g_screen_w * g_screen_h * sizeof(pixels[0]));

    const char *version = g_backend == 0 ? "hip" : (g_backend == 12 ? "cpu-step12" : "cpu-step1");

    for (int i = 0; i < num_runs; ++i)
        results[i] = benchmark(create_small_scene(), pixels, write_tga, "small");
    log_results(version, "small", results, num_runs);
    log_json(version, "small", results, num_runs);

    for (int i = 0; i < num_runs; ++i)
        results[i] = benchmark(create_medium_scene(), pixels, write_tga, "medium");
    log_results(version, "medium", results, num_runs);
    log_json(version, "medium", results, num_runs);

    for (int i = 0; i < num_runs; ++i)
        results[i] = benchmark(create_large_scene(), pixels, write_tga, "large");
    log_results(version, "large", results, num_runs);
    log_json(version, "large", results, num_runs);

    int rc_pipe = 0;
    if (g_pipeline > 0 && g_backend == 0 && g_inflight >= 1 && g_inflight <= 64)
    {
        rc_pipe |= pipelined("small", R1_SCENE_SMALL, g_pipeline);
        rc_pipe |= pipelined("medium", R1_SCENE_MEDIUM, g_pipeline);
        rc_pipe |= pipelined("large", R1_SCENE_LARGE, g_pipeline);
    }

    if (g_orbit > 0)
    {
        rc_pipe |= orbit("small", R1_SCENE_SMALL, g_orbit, write_tga);
        rc_pipe |= orbit("medium", R1_SCENE_MEDIUM, g_orbit, write_tga);
        rc_pipe |= orbit("large", R1_SCENE_LARGE, g_orbit, write_tga);
    }

    if (g_bounce > 0)
    {
        rc_pipe |= bounce("small", R1_SCENE_SMALL, g_bounce, write_tga);
        rc_pipe |= bounce("medium", R1_SCENE_MEDIUM, g_bounce, write_tga);
        rc_pipe |= bounce("large", R1_SCENE_LARGE, g_bounce, write_tga);
    }

    if (g_pulse > 0)
    {
        rc_pipe |= pulse("small", R1_SCENE_SMALL, g_pulse, write_tga);
        rc_pipe |= pulse("medium", R1_SCENE_MEDIUM, g_pulse, write_tga);
        rc_pipe |= pulse("large", R1_SCENE_LARGE, g_pulse, write_tga);
    }

    if (pixels_pinned)
        r1_host_free(pixels);
    else
        delete[] pixels;
    for (r1_context *c : g_ctx)
        r1_destroy(c);
    r1_multi_destroy(g_multi);
    return rc_pipe ? 3 : 0;
}
