// rayweek1_demos.cpp — what the drop-in host program runs after its benchmark() runs, none of it with a reference counterpart (the
// reference renders ONE fixed frame and waits): --pipeline and --orbit keep frames in flight over a ring of contexts, --bounce and --pulse
// animate the spheres between frames.  A new animation is a step (see Bounce) plus its rows in rayweek1_hip.cpp's option and demo tables.

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "rayweek1_options.h"

typedef std::chrono::high_resolution_clock Clock;

static double seconds(Clock::time_point from, Clock::time_point to) { return std::chrono::duration<double>(to - from).count(); }

// -w: a demo's frames 0 and FRAMES / 2, remembered as they land and written once the run has succeeded.
struct KeptFrames
{
    const int index[2];
    const bool on;
    std::vector<uint8_t> rgb[2];

    KeptFrames(int frames, bool write_tga) : index{0, frames / 2}, on(write_tga) {}

    void landed(int frame, const uint8_t *image)
    {
        for (int w = 0; w < 2; ++w)
            if (on && frame == index[w])
                rgb[w].assign(image, image + (size_t)g_opt.width * g_opt.height * 3);
    }

    void write(const char *demo, const char *scene_name)
    {
        for (int w = 0; w < 2; ++w)
            if (!rgb[w].empty() && (w == 0 || index[1] != index[0]))
            {
                char filename[128];
                snprintf(filename, sizeof(filename), "%s_%s_%03d.tga", demo, scene_name, index[w]);
                r1_tga_write_rgb24(filename, g_opt.width, g_opt.height, rgb[w].data());
            }
    }
};

// ---- frames in flight ------------------------------------------------------------------------------------------------------------------
// A demo's scene and its slots: per slot one context and stream (under --gather rccl one r1_multi, every launch split over the N devices)
// and one page-locked buffer the launch's records land in.  Rendered one after the other each frame pays the tail of its own longest
// bounce chains; kept in flight the next frames fill the chip while one drains.
struct Ring
{
    r1_host_scene *hs = nullptr;
    bool multi = false;
    std::vector<r1_context *> ctx;
    std::vector<r1_multi *> mul;
    std::vector<uint8_t *> host;

    explicit Ring(int kind) { r1_host_scene_create(kind, g_opt.width, g_opt.height, 0, 0, &hs); } // hs stays null where it fails

    ~Ring()
    {
        for (size_t s = 0; s < host.size(); ++s)
        {
            r1_host_free(host[s]);
            r1_destroy(ctx[s]);
            r1_multi_destroy(mul[s]);
        }
        r1_host_scene_destroy(hs);
    }

    int open(int k, bool rccl, size_t slot_bytes)
    {
        multi = rccl;
        ctx.assign((size_t)k, nullptr), mul.assign((size_t)k, nullptr), host.assign((size_t)k, nullptr);
        const int visible = r1_device_count();
        std::vector<int32_t> devs;
        for (int i = 0; i < g_opt.devices; ++i)
            devs.push_back(g_opt.device + i);
        int rc = R1_OK;
        for (size_t s = 0; s < host.size() && rc == R1_OK; ++s) // every context first, the scenes afterwards: the streams get their own hardware queues
            rc = multi ? r1_multi_create(g_opt.devices, devs.data(), &mul[s]) : r1_create(g_opt.device % (visible > 0 ? visible : 1), &ctx[s]);
        for (size_t s = 0; s < host.size() && rc == R1_OK; ++s)
        {
            rc = multi ? r1_multi_set_scene(mul[s], r1_host_scene_spheres(hs), r1_host_scene_camera(hs))
                       : r1_set_scene(ctx[s], r1_host_scene_spheres(hs), r1_host_scene_camera(hs));
            if (rc == R1_OK)
                rc = r1_host_alloc(slot_bytes, (void **)&host[s]);
        }
        return rc;
    }

    int wait(size_t s) { return multi ? r1_multi_sync(mul[s]) : r1_sync(ctx[s]); }

    // `launches` launches, launch l through slot l % k: enqueue(l, slot) starts one, landed(l) returns the rays of one whose records are on
    // the host.  Run twice: first as many launches as there are slots, for the workspaces and queues (not timed), then all of them.
    template <class Enqueue, class Landed> int run(int launches, Enqueue enqueue, Landed landed, uint64_t *rays, double *secs)
    {
        const int k = (int)host.size();
        int rc = R1_OK;
        for (int pass = 0; pass < 2 && rc == R1_OK; ++pass)
        {
            *rays = 0;
            const int n = pass ? launches : (k < launches ? k : launches);
            const Clock::time_point t0 = Clock::now();
            for (int l = 0; l < n && rc == R1_OK; ++l)
            {
                if (l >= k) // the slot's previous launch has to have landed before its buffer is reused
                {
                    rc = wait((size_t)(l % k));
                    *rays += landed(l - k);
                }
                if (rc == R1_OK)
                    rc = enqueue(l, (size_t)(l % k));
            }
            for (int l = n > k ? n - k : 0; l < n && rc == R1_OK; ++l)
            {
                rc = wait((size_t)(l % k));
                *rays += landed(l);
            }
            *secs = seconds(t0, Clock::now());
        }
        return rc;
    }
};

// --pipeline FRAMES: the `-n` runs of main (rayweek1.cpp:969-984) are independent frames; here --inflight of them are in flight
// (r1_render_async), and every frame still ends with its pixels and ray count on the host (the Timer span of rayweek1.cpp:848 -> :891,
// pipelined).  Prints one line per scene.
int pipelined(const char *scene_name, int kind, int frames, bool)
{
    const r1_params p = frame_params();
    const size_t rec = r1_frame_record_bytes(&p); // image, padded to 8 bytes, + uint64 ray count
    Ring ring(kind);
    if (!ring.hs)
        return 1;
    const int k = g_opt.inflight < frames ? g_opt.inflight : frames;
    int rc = ring.open(k, g_opt.gather == 1, rec);
    uint64_t rays = 0;
    double secs = 0;
    if (rc == R1_OK)
        rc = ring.run(
            frames,
            [&](int, size_t s) {
                return ring.multi ? r1_multi_render_async(ring.mul[s], &p, ring.host[s])
                                  : r1_render_async(ring.ctx[s], &p, ring.host[s], (uint64_t *)(ring.host[s] + rec - 8), nullptr);
            },
            [&](int l) { return *(const uint64_t *)(ring.host[(size_t)(l % k)] + rec - 8); }, &rays, &secs);
    if (rc == R1_OK)
        printf("%s pipelined:  %d frames, %d in flight%s, %.3f ms per frame, %llu rays, %0.2f mrays/s (pixels + count on the host)\n", scene_name, frames,
               k, ring.multi ? " (each split over the devices, RCCL all-gather)" : "", secs / frames * 1e3, (unsigned long long)rays, rays / secs / 1e6);
    else
        fprintf(stderr, "pipelined %s: %s\n", scene_name, r1_last_error());
    return rc == R1_OK ? 0 : 1;
}

// --orbit FRAMES: the scene's own camera (r1_host_scene_view) turned about the vertical axis through lookat, frame f at angle 2 pi f / FRAMES
// (frame 0 is the scene's camera bit for bit: cos 0 = 1, sin 0 = 0), every frame with benchmark()'s seed.  The frames are rendered as camera-path
// batches — consecutive frames of the orbit in ONE launch, each through its own camera (r1_render_path_async) — over --inflight contexts.
// Prints one line per scene.
int orbit(const char *scene_name, int kind, int frames, bool write_tga)
{
    const r1_params p = frame_params();
    Ring ring(kind);
    if (!ring.hs)
        return 1;
    float from[3], at[3], up[3], vfov = 0, aperture = 0, focus = 0;
    int rc = r1_host_scene_view(ring.hs, from, at, up, &vfov, &aperture, &focus);
    std::vector<r1_camera> cams((size_t)frames);
    for (int f = 0; f < frames && rc == R1_OK; ++f)
    {
        const double a = 2.0 * M_PI * (double)f / (double)frames;
        const float cs = (float)cos(a), sn = (float)sin(a);
        const float dx = from[0] - at[0], dz = from[2] - at[2];
        const float eye[3] = {at[0] + (dx * cs + dz * sn), from[1], at[2] + (dz * cs - dx * sn)};
        rc = r1_camera_look_at(eye, at, up, vfov, (float)g_opt.width / (float)g_opt.height, aperture, focus, &cams[(size_t)f]);
    }
    // frames per launch: the orbit dealt evenly to the contexts, at most 16 (all frames of a launch are delivered together) and within the
    // 2^31 padded sample slots of a launch
    const int k = g_opt.inflight < frames ? g_opt.inflight : frames;
    const uint64_t slots = (uint64_t)((g_opt.width + 31) / 32) * (uint64_t)((g_opt.height + 31) / 32) * 1024u * (uint64_t)g_opt.spp;
    int per = (frames + k - 1) / k;
    per = per > 16 ? 16 : per;
    if (slots && (uint64_t)per * slots >= ((uint64_t)1 << 31))
        per = (int)((((uint64_t)1 << 31) - 1) / slots);
    per = per < 1 ? 1 : per;
    const size_t rec = r1_frame_record_bytes(&p); // image, padded to 8 bytes, + uint64 ray count
    if (rc == R1_OK)
        rc = ring.open(k, false, rec * (size_t)per);
    KeptFrames kept(frames, write_tga);
    uint64_t rays = 0;
    double secs = 0;
    if (rc == R1_OK)
        rc = ring.run(
            (frames + per - 1) / per,
            [&](int l, size_t s) {
                const int f0 = l * per;
                return r1_render_path_async(ring.ctx[s], &p, frames - f0 < per ? frames - f0 : per, 0u, &cams[(size_t)f0], ring.host[s], nullptr);
            },
            [&](int l) {
                const uint8_t *records = ring.host[(size_t)(l % k)];
                const int f0 = l * per, n = frames - f0 < per ? frames - f0 : per;
                uint64_t sum = 0;
                for (int i = 0; i < n; ++i)
                {
                    sum += *(const uint64_t *)(records + (size_t)(i + 1) * rec - 8);
                    kept.landed(f0 + i, records + (size_t)i * rec);
                }
                return sum;
            },
            &rays, &secs);
    if (rc == R1_OK)
    {
        printf("%s orbit:  %d frames, %d per launch, %d in flight, %.3f ms per frame, %llu rays, %0.2f mrays/s (one camera per frame, pixels + count on the host)\n",
               scene_name, frames, per, k, secs / frames * 1e3, (unsigned long long)rays, rays / secs / 1e6);
        kept.write("orbit", scene_name);
    }
    else
        fprintf(stderr, "orbit %s: %s\n", scene_name, r1_last_error());
    return rc == R1_OK ? 0 : 1;
}

// ---- animated spheres --------------------------------------------------------------------------------------------------------------------
// --bounce and --pulse change the lattice spheres — every hittable sphere but the four largest (the ground and the three big balls) —
// between frames: one update is enqueued per frame and nothing else about the scene is touched, so the box tree is refitted on the device,
// never rebuilt.  Every frame with benchmark()'s seed, through r1_render_async into page-locked memory.  An animation is a Step:
//     static const char *name, *verb      the option without its dashes, and what the report line says the lattice spheres are doing
//     Step(scene)                         the arrays it edits, as the scene has them
//     void edit(lattice, ff, frames)      the arrays of frame ff of `frames`: no clock, no random number
//     int enqueue(ctx)                    the update call with them
// Prints one `<name>:` line per scene with the mean time of an update (enqueue to stream idle) and of a frame.
template <class Step> static int animate(const char *scene_name, int kind, int frames, bool write_tga)
{
    const r1_params p = frame_params();
    const size_t rec = r1_frame_record_bytes(&p);
    Ring ring(kind);
    if (!ring.hs)
        return 1;
    const r1_scene *sc = r1_host_scene_spheres(ring.hs);
    std::vector<uint32_t> lattice;
    for (uint32_t i = 0; i < sc->count; ++i)
        if (sc->inv_radius[i] != 0)
            lattice.push_back(i);
    std::stable_sort(lattice.begin(), lattice.end(), [&](uint32_t a, uint32_t b) { return sc->radius_sq[a] > sc->radius_sq[b]; });
    lattice.erase(lattice.begin(), lattice.begin() + (lattice.size() < 4 ? lattice.size() : 4)); // the four largest stay as they are
    Step step(sc);
    int rc = ring.open(1, false, rec);
    KeptFrames kept(frames, write_tga);
    uint64_t rays = 0;
    double t_update = 0, t_render = 0;
    for (int f = -1; f < frames && rc == R1_OK; ++f) // f = -1: workspaces and queues (frame 0 once more, not timed)
    {
        step.edit(lattice, f < 0 ? 0 : f, frames);
        const Clock::time_point t0 = Clock::now();
        rc = step.enqueue(ring.ctx[0]);
        if (rc == R1_OK)
            rc = r1_sync(ring.ctx[0]);
        const Clock::time_point t1 = Clock::now();
        if (rc == R1_OK)
            rc = r1_render_async(ring.ctx[0], &p, ring.host[0], (uint64_t *)(ring.host[0] + rec - 8), nullptr);
        if (rc == R1_OK)
            rc = r1_sync(ring.ctx[0]);
        if (f < 0 || rc != R1_OK)
            continue;
        t_update += seconds(t0, t1), t_render += seconds(t1, Clock::now());
        rays += *(const uint64_t *)(ring.host[0] + rec - 8);
        kept.landed(f, ring.host[0]);
    }
    if (rc == R1_OK)
    {
        printf("%s %s: %d frames, %zu of %u spheres %s, update %.3f ms per frame (enqueue to idle), render %.3f ms per frame, %llu rays, %0.2f mrays/s\n",
               scene_name, Step::name, frames, lattice.size(), sc->count, Step::verb, t_update / frames * 1e3, t_render / frames * 1e3,
               (unsigned long long)rays, rays / (t_update + t_render) / 1e6);
        kept.write(Step::name, scene_name);
    }
    else
        fprintf(stderr, "%s %s: %s\n", Step::name, scene_name, r1_last_error());
    return rc == R1_OK ? 0 : 1;
}

// --bounce FRAMES: the lattice spheres bob in y.  Sphere i (scene index) of radius r_i sits in frame f at
//      y_i(f) = y_i + (r_i / 2) * (1 + sin(2 pi (f / FRAMES + (i mod 8) / 8)))
// evaluated in fp64 and rounded to fp32: eight phase groups, half a radius of amplitude, one period over the run.
struct Bounce
{
    static constexpr const char *name = "bounce", *verb = "moving";
    const r1_scene *sc;
    std::vector<float> y;

    explicit Bounce(const r1_scene *scene) : sc(scene), y(scene->center_y, scene->center_y + scene->count) {}

    void edit(const std::vector<uint32_t> &lattice, int ff, int frames)
    {
        for (uint32_t i : lattice)
        {
            const double r = sqrt((double)sc->radius_sq[i]);
            y[i] = (float)((double)sc->center_y[i] + 0.5 * r * (1.0 + sin(2.0 * M_PI * ((double)ff / (double)frames + (double)(i % 8u) / 8.0))));
        }
    }

    int enqueue(r1_context *ctx) { return r1_update_centers(ctx, 0, sc->count, sc->center_x, y.data(), sc->center_z, nullptr); }
};

// --pulse FRAMES: the lattice spheres breathe and change colour.  In frame f, with t = f / FRAMES, sphere i (scene index) has
//      radius  r_i * (1 + 0.3 sin(2 pi t) cos(2 pi (i mod 8) / 8))          stored as SphereSOA::add stores a radius: r * r and 1 / r in fp32
//      albedo  a_i + (a_i rotated r -> g -> b -> r  -  a_i) * (1 - cos(2 pi t)) / 2
// the factors evaluated in fp64 and rounded to fp32; a factor of exactly 1 (frame 0) keeps the scene's own pair, so frame 0 is benchmark()'s
// frame.  Material types and parameters stay; the update carries the radii and materials of every sphere.
struct Pulse
{
    static constexpr const char *name = "pulse", *verb = "pulsing";
    const r1_scene *sc;
    std::vector<float> rsq, inv, ar, ag, ab;

    explicit Pulse(const r1_scene *scene)
        : sc(scene), rsq(scene->radius_sq, scene->radius_sq + scene->count), inv(scene->inv_radius, scene->inv_radius + scene->count),
          ar(scene->albedo_r, scene->albedo_r + scene->count), ag(scene->albedo_g, scene->albedo_g + scene->count),
          ab(scene->albedo_b, scene->albedo_b + scene->count)
    {
    }

    void edit(const std::vector<uint32_t> &lattice, int ff, int frames)
    {
        const double t = (double)ff / (double)frames, swing = 0.3 * sin(2.0 * M_PI * t), mix = 0.5 * (1.0 - cos(2.0 * M_PI * t));
        for (uint32_t i : lattice)
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
    }

    int enqueue(r1_context *ctx)
    {
        r1_sphere_update u;
        memset(&u, 0, sizeof(u));
        u.radius_sq = rsq.data(), u.inv_radius = inv.data();
        u.mat_type = sc->mat_type, u.albedo_r = ar.data(), u.albedo_g = ag.data(), u.albedo_b = ab.data(), u.mat_param = sc->mat_param;
        return r1_update_spheres(ctx, 0, sc->count, &u, nullptr);
    }
};

int bounce(const char *scene_name, int kind, int frames, bool write_tga) { return animate<Bounce>(scene_name, kind, frames, write_tga); }
int pulse(const char *scene_name, int kind, int frames, bool write_tga) { return animate<Pulse>(scene_name, kind, frames, write_tga); }
