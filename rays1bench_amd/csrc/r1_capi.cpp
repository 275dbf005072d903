// r1_capi.cpp — the C-ABI of include/rays1.h on top of the HIP runtime: context, scene
// upload, launches, timing.  Host code only (the kernels live in r1_trace.hpp).
//
// There is no CPU fallback anywhere in this file: without a HIP device every compute
// entry point returns R1_ENODEVICE / R1_EHIP.

#include <hip/hip_runtime.h>
#include <cmath>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "../../include/rays1.h"
#include "r1_device.h"
#include "r1_grid.h"

#include "r1_bvh.h" // r1_bvh.cpp: the built tree, a refit's topology tables
#include "r1_internal.h"

// ---- errors ---------------------------------------------------------------------------------

static thread_local char g_error[512] = "";

extern "C" void r1_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

extern "C" const char *r1_last_error(void) { return g_error; }
extern "C" int r1_abi_version(void) { return R1_ABI_VERSION; }

#define R1_HIP(call)                                                                                                   \
    do                                                                                                                 \
    {                                                                                                                  \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
        {                                                                                                              \
            r1_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);                   \
            return e_ == hipErrorOutOfMemory ? R1_ENOMEM : R1_EHIP;                                                    \
        }                                                                                                              \
    } while (0)

// ---- context ----------------------------------------------------------------------------------

struct DevBuf
{
    void *p = nullptr;
    size_t cap = 0;
};

struct r1_context
{
    int device = 0;
    int cus = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    hipEvent_t last0 = nullptr, last1 = nullptr, last2 = nullptr; // the events the last enqueued frame recorded (own set or ring slot)
    bool timing_valid = false;
    // optional per-frame event ring (r1_timing_begin/_end): 3 events per frame
    std::vector<hipEvent_t> ring;
    int ring_frames = 0, ring_used = 0;
    bool ring_on = false;

    // scene
    DevBuf sweep, exact, exact_g, shade, mat, members;
    DevBuf bvh_nodes, bvh_prims, bvh_ids; // R1_VARIANT_BVH (r1_bvh.cpp)
    // R1_VARIANT_GRID (r1_grid.cpp): built on the first render that asks for it after r1_set_scene (ensure_grid)
    DevBuf grid_tab, grid_out, grid_dev;  // cell table + ids, outliers, the R1GridArgs the kernels read
    DevBuf grid_tab32, grid_dev32;        // the same in the big-scene kernel's 32-bit form (small scenes: for PIXEL mode, see big_scene)
    bool grid_valid = false;
    bool grid_small = false;  // 16-bit tables that the small-scene kernel keeps in LDS
    R1GridArgs grid_args;     // (pointers into grid_tab / grid_out; a copy of it in grid_dev)
    DevBuf wf_paths, wf_hits, wf_queue, wf_counts; // R1_VARIANT_WAVEFRONT workspace
    DevBuf wave_log;                               // STATS builds: per-wave {start, queue empty, end, iterations}
    unsigned long long wave_log_ptr = 0;
    uint32_t wave_log_waves = 0;
    uint32_t n_bvh_nodes = 0, n_bvh_leaves = 0;
    int bvh_depth = 0;
    float bvh_centre[3] = {0, 0, 0};
    int bvh_pad_local = 0;
    int bvh_root_leaf = 0;
    float bvh_flat_m = 0.0f, bvh_flat_e = -1.0f; // the tree's flat y slab (r1_bvh.cpp), e < 0: none
    uint32_t n_active = 0, n_sweep = 0, n_padded_scene = 0, n_groups = 0, n_multi = 0;
    std::vector<uint32_t> active_to_scene;
    R1DeviceCamera cam;
    bool have_scene = false;
    // what the device tables were built from: r1_set_scene with the same arrays again (the drop-in's benchmark()
    // uploads its scene on every run, rayweek1.cpp:969-984) keeps the tables and the tree
    std::vector<float> src_f32[9];
    std::vector<uint8_t> src_mat;
    r1_camera src_cam;

    // per-frame workspace
    DevBuf counters, samples, image;
    // frame batches: the batch's numbers live in one of eight device slots (counter tail + 64 + 32 i), written by a one-thread launch whose
    // values travel in its kernel arguments (an asynchronous copy from a host member could be overtaken by the next call)
    R1BatchArgs batch_args_last = {0, 0, {0, 0, 0}, 0};
    hipStream_t batch_args_stream = nullptr;
    int batch_args_slot = -1;
    // camera paths: the launch's table of cameras (R1PathArgs::cameras), two halves taken in turn so that a launch still reading the
    // previous table is not disturbed; written in stream order by launches whose values travel in their kernel arguments
    DevBuf path_cams;
    int path_cams_half = 0;
    // R1_LAND (tiles resolved inside the trace kernel): per-context state
    bool land_prev = false;      // the last launch through this context was a LAND launch
    int land_parity = 0;         // the set of queue heads that launch used
    uint32_t land_gen = 0;       // launch generation: the tag of its sample records (1 .. 2^24 - 1)
    bool land_armed = false;     // the countdowns / accumulators behind the counter block hold the values of land_key
    r1_params land_key;
    int land_frames = 0;
    DevBuf batch_rays;  // frame batches: per-frame ray-count accumulators of the resolve launch + its finished-workgroup counter
    int tile_frames = 0; // frames per launch the tile arithmetic below was made for
    bool counters_clean = false; // the last frame's resolve launch zeroed the counter block: the next frame needs no memset
    r1_params tile_key;
    bool tile_key_valid = false;
    uint32_t n_local_tiles = 0, total_samples = 0, full = 0;

    // one page-locked, device-visible word: the synchronous entry points let the frame's last launch store the ray count
    // straight into host memory (8 bytes over PCIe at the end of r1_resolve_kernel) instead of enqueueing a second copy
    unsigned long long *host_word = nullptr, *host_word_dev = nullptr;
    int default_variant = R1_V_TREE;    // what R1_VARIANT_DEFAULT resolves to for the scene in the context (r1_set_scene): synchronous frames
    int default_variant_tp = R1_V_TREE; // ... and frames in flight (the throughput kernels: measured apart, the two kernel families do not rank alike)
    int occupancy[8 * 2 * 2 * R1_MODES] = {0}; // blocks per CU of the trace kernel's builds, [occupancy_slot(build)]
    bool pixel_mode = false; // r1_set_pixel_mode
    DevBuf gstack;
    DevBuf land_spill; // R1_LAND: [waves of the grid][tiles of the launch] every wave's list of the tiles it took chunks from
    // progressive passes (r1_render_pass): the frame being accumulated
    DevBuf accum;              // [local tile][pixel of the padded tile] fp32 {r, g, b, 0}
    bool pass_valid = false;   // accum holds samples [0, pass_samples) of pass_key's frame (false after r1_set_scene or a failed pass)
    r1_params pass_key;        // the params that started it (spp: that pass's)
    int32_t pass_samples = 0;
    uint64_t pass_rays = 0;    // color() calls of those samples
    // adaptive sampling (r1_render_adaptive): `accum` is its `all` accumulator, indexed by tile of the frame as accum_even is
    DevBuf accum_even;         // [tile][pixel of the padded tile] the sums over the samples of even global index
    DevBuf adapt_list;         // two tile lists of a frame's tiles each (this pass's, the next one's), then the next one's length
    DevBuf adapt_report;       // [tile] R1TileReport
    // ray queries (r1_cast_rays*): nothing here is read or written by a render
    DevBuf active_dev;         // active_to_scene on the device, uploaded once per r1_set_scene
    DevBuf cast_cursors;       // R1_CAST_CURSORS ray cursors, 128 bytes apart, taken in turn
    uint32_t cast_cursor_next = 0;
    DevBuf cast_ws;            // r1_cast_rays: one chunk's rays and results (R1_CAST_CHUNK x 64 bytes)
    int cast_occupancy[8] = {0}; // blocks per CU of the cast kernels, [structure slot * 2 + big]
    // moving spheres (r1_update_centers*): the refit's tables — topology, uploaded once per r1_set_scene — and its scratch
    DevBuf refit_tab;          // uint32: scene -> active index, then R1RefitTopo's slot, leaf_ref, child_box, by_height
    DevBuf refit_radii;        // [active][2] fp64 {bound radius, test radius}
    DevBuf refit_box;          // 256 bytes (word 0: the largest A), then [nodes + leaves] R1Box
    R1RefitArgs refit;         // pointers into the tables above and the scene's
    std::vector<uint32_t> refit_height_off; // R1RefitTopo::height_off
    std::vector<uint32_t> scene_to_active;  // 0xFFFFFFFF: not active
    bool moved = false;        // an update since the last r1_set_scene: the sphere groups and the grid are stale, src_f32 may be
    float *stage = nullptr, *stage_dev = nullptr; // host form: page-locked staging of the centres, read by the move kernel
    size_t stage_cap = 0;      // floats
    hipEvent_t stage_ev = nullptr; // recorded behind the move kernel that reads `stage`
    bool stage_busy = false;

    r1_launch_info info;
};

static int ensure(DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap && b.p)
        return R1_OK;
    if (b.p)
    {
        R1_HIP(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes < 256 ? 256 : bytes;
    R1_HIP(hipMalloc(&b.p, want));
    b.cap = want;
    return R1_OK;
}

static void release(DevBuf &b)
{
    if (b.p)
        (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

extern "C" int r1_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
    {
        r1_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return R1_ENODEVICE;
    }
    return n;
}

extern "C" int r1_create(int device, r1_context **out)
{
    if (!out)
        return R1_EINVAL;
    *out = nullptr;
    int n = r1_device_count();
    if (n <= 0)
    {
        if (n == 0)
            r1_set_error("no HIP device visible (librays1 has no CPU fallback)");
        return R1_ENODEVICE;
    }
    if (device < 0 || device >= n)
    {
        r1_set_error("device %d out of range (0..%d)", device, n - 1);
        return R1_EINVAL;
    }
    r1_context *c = new (std::nothrow) r1_context();
    if (!c)
        return R1_ENOMEM;
    c->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess)
        e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipEventCreate(&c->ev0);
    if (e == hipSuccess)
        e = hipEventCreate(&c->ev1);
    if (e == hipSuccess)
        e = hipEventCreate(&c->ev2);
    if (e != hipSuccess)
    {
        r1_set_error("r1_create: %s", hipGetErrorString(e));
        delete c;
        return R1_EHIP;
    }
    if (hipHostMalloc((void **)&c->host_word, 64, hipHostMallocMapped) == hipSuccess)
    {
        memset(c->host_word, 0, 64); // (the runtime may hand back a recycled block: word 2 is land_check's "a resolver gave up" flag)
        if (hipHostGetDevicePointer((void **)&c->host_word_dev, c->host_word, 0) != hipSuccess)
        {
            (void)hipHostFree(c->host_word);
            c->host_word = c->host_word_dev = nullptr;
        }
    }
    else
        c->host_word = nullptr; // (not fatal: the count is copied instead)
    (void)hipGetLastError();
    c->cus = prop.multiProcessorCount;
    memset(&c->info, 0, sizeof(c->info));
    c->info.compute_units = c->cus;
    *out = c;
    return R1_OK;
}

// internal (r1_multi.cpp): the context's own stream, so that the in-process multi-GPU path runs its collectives on the stream the
// context's uploads and frames already use instead of a second stream per device (every stream wants a hardware queue)
extern "C" void *r1_context_stream(r1_context *c) { return c ? (void *)c->stream : nullptr; }

// internal (tests/test_builds_host.py): r1_pick as the frames' choose_kernel calls it
extern "C" int r1_pick_build(int variant, int big, int want, int *build4)
{
    R1Build b = {0, false, false, 0};
    if (!r1_pick(variant, big != 0, want, b))
        return 0;
    build4[0] = b.variant, build4[1] = b.stats ? 1 : 0, build4[2] = b.big ? 1 : 0, build4[3] = b.mode;
    return 1;
}

// internal (the same test): what the predicates of r1_builds.h answer
extern "C" void r1_build_facts(int variant, int mode, int big, int *facts6)
{
    facts6[0] = r1_is_tree(variant), facts6[1] = r1_is_grid(variant), facts6[2] = r1_is_stats(variant), facts6[3] = r1_base_variant(variant);
    facts6[4] = r1_mode_is_tp_family(mode), facts6[5] = r1_runs_as_latency(mode, big != 0);
}

extern "C" void r1_destroy(r1_context *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    release(c->sweep), release(c->exact), release(c->exact_g), release(c->shade), release(c->mat), release(c->members);
    release(c->bvh_nodes), release(c->bvh_prims), release(c->bvh_ids), release(c->grid_tab), release(c->grid_out), release(c->grid_dev), release(c->grid_tab32), release(c->grid_dev32);
    release(c->wf_paths), release(c->wf_hits), release(c->wf_queue), release(c->wf_counts);
    release(c->land_spill), release(c->gstack), release(c->counters), release(c->samples), release(c->image), release(c->batch_rays);
    release(c->wave_log), release(c->accum), release(c->path_cams), release(c->accum_even), release(c->adapt_list), release(c->adapt_report);
    release(c->active_dev), release(c->cast_cursors), release(c->cast_ws);
    release(c->refit_tab), release(c->refit_radii), release(c->refit_box);
    if (c->stage)
        (void)hipHostFree(c->stage);
    if (c->stage_ev)
        (void)hipEventDestroy(c->stage_ev);
    if (c->host_word)
        (void)hipHostFree(c->host_word);
    for (hipEvent_t e : c->ring)
        (void)hipEventDestroy(e);
    if (c->ev0)
        (void)hipEventDestroy(c->ev0);
    if (c->ev1)
        (void)hipEventDestroy(c->ev1);
    if (c->ev2)
        (void)hipEventDestroy(c->ev2);
    if (c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c;
}

// ---- scene upload -------------------------------------------------------------------------------

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
// re-tests the members of flagged groups exactly (r1_trace.hpp).  Grouping is a pure work
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

// ---- R1_VARIANT_DEFAULT -------------------------------------------------------------------------------------------------------------
// DEFAULT is the box tree for every scene: a property of the build, so what a context launches depends on its arguments only and
// the ranks of a multi-GPU job always run the same kernel.  (Round 3 timed scenes of 9..127 spheres through both kernels when
// they were set, because the reference's dense medium scene was 4-5 % faster through the ungrouped sweep in round 2.  Since the
// root step of the walk the tree is ahead on every row of the crossover table, profiles/r04/tree_vs_sweep_crossover*.txt — by
// 0-3 % for one synchronous frame of the medium scene, 7 % with frames in flight — and a probe inside r1_set_scene made the first
// timed benchmark() call, the kernel choice of each rank and a 62 MB workspace depend on a wall-clock race: VERDICT r03 / ADVICE r03.)
struct Batch;
struct Landing;
struct Pass;
static int enqueue_frame(r1_context *c, const r1_params *p, void *d_out, int block_layout, void *d_rays, hipStream_t st, bool throughput_mode,
                         const Batch *batch = nullptr, Landing *landing = nullptr, const Pass *pass = nullptr);

// what the kernels read of a camera (Camera::getRay, rayweek1.cpp:381-386, does not use w)
static R1DeviceCamera device_camera(const r1_camera &cam)
{
    R1DeviceCamera d;
    memcpy(d.origin, cam.origin, 12);
    memcpy(d.lower_left, cam.lower_left, 12);
    memcpy(d.horizontal, cam.horizontal, 12);
    memcpy(d.vertical, cam.vertical, 12);
    memcpy(d.u, cam.u, 12);
    memcpy(d.v, cam.v, 12);
    d.lens_radius = cam.lens_radius;
    return d;
}

extern "C" int r1_set_scene(r1_context *c, const r1_scene *s, const r1_camera *cam)
{
    if (!c || !s || !cam || !s->center_x || !s->center_y || !s->center_z || !s->radius_sq || !s->inv_radius || !s->mat_type ||
        !s->albedo_r || !s->albedo_g || !s->albedo_b || !s->mat_param)
    {
        r1_set_error("r1_set_scene: null argument");
        return R1_EINVAL;
    }
    c->pass_valid = false; // (a progressive frame does not continue across a scene upload, even of the same arrays)
    R1_HIP(hipSetDevice(c->device));

    const float *const src[9] = {s->center_x, s->center_y, s->center_z, s->radius_sq, s->inv_radius, s->albedo_r, s->albedo_g, s->albedo_b, s->mat_param};
    // (not after r1_update_centers*: the device holds other centres than src_f32, or the groups and the grid are those of other centres)
    if (c->have_scene && !c->moved && c->src_mat.size() == s->count && memcmp(&c->src_cam, cam, sizeof(*cam)) == 0 &&
        (s->count == 0 || memcmp(c->src_mat.data(), s->mat_type, s->count) == 0))
    {
        bool same = true;
        for (int k = 0; k < 9 && same; ++k)
            same = s->count == 0 || memcmp(c->src_f32[k].data(), src[k], (size_t)s->count * 4) == 0;
        if (same)
            return R1_OK; // bit-identical scene and camera: everything on the device is current
    }
    c->have_scene = false;
    c->grid_valid = false;

    // active spheres: inv_radius != 0 (rayweek1.cpp:291); order preserved so that ties keep
    // the earlier index as in the reference's in-order resolve loop
    int rc_active = r1_active_spheres(s, c->active_to_scene);
    if (rc_active != R1_OK)
        return rc_active;
    for (uint32_t i : c->active_to_scene)
        if (s->mat_type[i] > R1_MAT_DIELECTRIC)
        {
            r1_set_error("r1_set_scene: sphere %u is hittable but has no material", i);
            return R1_EINVAL;
        }
    const uint32_t na = (uint32_t)c->active_to_scene.size();
    if (na > R1_MAX_ACTIVE)
    {
        r1_set_error("r1_set_scene: %u hittable spheres; this build supports up to %u", na, R1_MAX_ACTIVE);
        return R1_ELIMIT;
    }
    // level 1 of the sweep: groups of nearby spheres with a bounding sphere each
    std::vector<double> ax(na ? na : 1), ay(na ? na : 1), az(na ? na : 1), ar_(na ? na : 1);
    std::vector<char> lone(na ? na : 1, 0);
    for (uint32_t a = 0; a < na; ++a)
    {
        const uint32_t i = c->active_to_scene[a];
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
    std::vector<float> sweep(4 * (size_t)ns_alloc), exact(4 * (size_t)(na ? na : 1)),
        shade(4 * (size_t)(na > R1_MAX_ACTIVE_10BIT ? na : R1_MAX_ACTIVE_10BIT + 1)), // small scenes: any 10-bit index may be read (unwind)
        mat(4 * (size_t)(na ? na : 1));
    std::vector<uint32_t> members((size_t)R1_GROUP_MAX * ns_alloc, 0xFFFFFFFFu);
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
    }
    for (uint32_t a = 0; a < na; ++a)
    {
        const uint32_t i = c->active_to_scene[a];
        const float cx = s->center_x[i], cy = s->center_y[i], cz = s->center_z[i], rsq = s->radius_sq[i];
        exact[4 * a + 0] = cx, exact[4 * a + 1] = cy, exact[4 * a + 2] = cz, exact[4 * a + 3] = rsq;
        shade[4 * a + 0] = s->inv_radius[i], shade[4 * a + 1] = s->albedo_r[i], shade[4 * a + 2] = s->albedo_g[i],
                      shade[4 * a + 3] = s->albedo_b[i];
        uint32_t type = s->mat_type[i];
        memcpy(&mat[4 * a], &type, 4);
        const float ref_idx = s->mat_param[i];
        mat[4 * a + 1] = ref_idx;
        // Dielectric constants the reference recomputes per hit with IEEE float ops
        // (rayweek1.cpp:489 `1.0f / _refIdx`, :456-457 schlick r0): same operations, done once
        float r0 = (1 - ref_idx) / (1 + ref_idx);
        r0 = r0 * r0;
        mat[4 * a + 2] = type == R1_MAT_DIELECTRIC ? 1.0f / ref_idx : 0.0f;
        mat[4 * a + 3] = type == R1_MAT_DIELECTRIC ? r0 : 0.0f;
    }

    // the members' spheres once more, in group order (exact_trips fetches sphere and index side by side)
    std::vector<float> exact_g(4 * (size_t)R1_GROUP_MAX * ns_alloc);
    for (size_t k = 0; k < (size_t)R1_GROUP_MAX * ns_alloc; ++k)
    {
        const uint32_t a = members[k];
        for (int q = 0; q < 4; ++q)
            exact_g[4 * k + q] = a != 0xFFFFFFFFu ? exact[4 * (size_t)a + q] : (q == 3 ? -INFINITY : 0.0f);
    }

    // the optional spatial index over the same active spheres (R1_VARIANT_BVH)
    R1Bvh bvh;
    {
        std::vector<float> fx(na ? na : 1), fy(na ? na : 1), fz(na ? na : 1), fr(na ? na : 1);
        for (uint32_t a = 0; a < na; ++a)
            fx[a] = exact[4 * a + 0], fy[a] = exact[4 * a + 1], fz[a] = exact[4 * a + 2], fr[a] = exact[4 * a + 3];
        static const int leaf_env = (int)r1_knob("R1_BVH_LEAF", 0);
        // leaf size: 4 spheres (2 pairs) on the reference's scenes; 8 on big lattices (measured:
        // 100 004 spheres 3.43 ms against 3.67 ms per 1920x1080x4 frame)
        const int leaf_default = na > R1_MAX_ACTIVE_10BIT ? 2 * R1_BVH_LEAF : R1_BVH_LEAF;
        r1_build_bvh(na, fx.data(), fy.data(), fz.data(), fr.data(), ar_.data(), leaf_env > 0 ? leaf_env : leaf_default, bvh);
        if (bvh.max_depth > R1_BVH_STACK)
        {
            r1_set_error("r1_set_scene: spatial index deeper (%d) than the traversal stack (%d)", bvh.max_depth, R1_BVH_STACK);
            return R1_ELIMIT;
        }
    }

    // leaf_quad fetches a sphere index speculatively for lanes that hold no flagged sphere (slot 3 of the step, whatever the step's
    // pair count): two sentinel words behind the last pair keep that read inside the table
    bvh.ids.resize(bvh.ids.size() + 2, 0xFFFFFFFFu);
    int rc;
    if ((rc = ensure(c->bvh_nodes, bvh.nodes.size() * 4)) || (rc = ensure(c->bvh_prims, bvh.prims.size() * 4)) ||
        (rc = ensure(c->bvh_ids, bvh.ids.size() * 4)))
        return rc;
    if ((rc = ensure(c->sweep, sweep.size() * 4)) || (rc = ensure(c->exact, exact.size() * 4)) ||
        (rc = ensure(c->shade, shade.size() * 4)) || (rc = ensure(c->mat, mat.size() * 4)) ||
        (rc = ensure(c->members, members.size() * 4)) || (rc = ensure(c->exact_g, exact_g.size() * 4)))
        return rc;
    // Uploads go through the context's OWN stream (then one wait): librays1 never touches the null stream.  A process
    // that keeps K frames in flight on K contexts with GPU_MAX_HW_QUEUES = K would otherwise hand one of its K hardware
    // queues to the null stream, and two frames would share a queue and run one after the other (measured: 20 frames
    // land in 20.1 ms instead of 17.0, tools/submit_times.py, profiles/r03/stream_queue_mapping.txt).
    R1_HIP(hipStreamSynchronize(c->stream));
    R1_HIP(hipMemcpyAsync(c->sweep.p, sweep.data(), sweep.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->exact.p, exact.data(), exact.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->shade.p, shade.data(), shade.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->mat.p, mat.data(), mat.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->members.p, members.data(), members.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->exact_g.p, exact_g.data(), exact_g.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->bvh_nodes.p, bvh.nodes.data(), bvh.nodes.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->bvh_prims.p, bvh.prims.data(), bvh.prims.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->bvh_ids.p, bvh.ids.data(), bvh.ids.size() * 4, hipMemcpyHostToDevice, c->stream));
    // ray queries report SCENE indices: the active spheres' scene indices, once per scene
    if ((rc = ensure(c->active_dev, (size_t)(na ? na : 1) * 4)))
        return rc;
    if (na)
        R1_HIP(hipMemcpyAsync(c->active_dev.p, c->active_to_scene.data(), (size_t)na * 4, hipMemcpyHostToDevice, c->stream));
    // what a refit needs besides the tree (r1_update_centers*): topology and the radii, once per scene
    R1RefitTopo topo;
    r1_bvh_topology(bvh, na, topo);
    c->scene_to_active.assign(s->count ? s->count : 1, 0xFFFFFFFFu);
    for (uint32_t a = 0; a < na; ++a)
        c->scene_to_active[c->active_to_scene[a]] = a;
    std::vector<uint32_t> rtab;
    size_t roff[5];
    {
        const std::vector<uint32_t> *parts[5] = {&c->scene_to_active, &topo.slot, &topo.leaf_ref, &topo.child_box, &topo.by_height};
        for (int k = 0; k < 5; ++k)
            roff[k] = rtab.size(), rtab.insert(rtab.end(), parts[k]->begin(), parts[k]->end());
    }
    std::vector<double> radii(2 * (size_t)(na ? na : 1), 0.0);
    for (uint32_t a = 0; a < na; ++a)
        radii[2 * (size_t)a + 0] = ar_[a], radii[2 * (size_t)a + 1] = r1_test_radius(ar_[a], exact[4 * (size_t)a + 3]);
    const size_t n_box = bvh.nodes.size() / 16 + topo.leaf_ref.size();
    if ((rc = ensure(c->refit_tab, rtab.size() * 4)) || (rc = ensure(c->refit_radii, radii.size() * 8)) ||
        (rc = ensure(c->refit_box, 256 + n_box * sizeof(R1Box))))
        return rc;
    R1_HIP(hipMemcpyAsync(c->refit_tab.p, rtab.data(), rtab.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->refit_radii.p, radii.data(), radii.size() * 8, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream)); // the host vectors go out of scope
    {
        R1RefitArgs &r = c->refit;
        const uint32_t *tab = (const uint32_t *)c->refit_tab.p;
        r.exact = (float *)c->exact.p, r.prims = (float *)c->bvh_prims.p, r.nodes = (float *)c->bvh_nodes.p, r.ids = (const uint32_t *)c->bvh_ids.p;
        r.scene_to_active = tab + roff[0], r.slot = tab + roff[1], r.leaf_ref = tab + roff[2], r.child_box = tab + roff[3], r.by_height = tab + roff[4];
        r.radii = (const double *)c->refit_radii.p;
        r.a_max = (uint32_t *)c->refit_box.p, r.box = (R1Box *)((char *)c->refit_box.p + 256);
        r.n_nodes = (uint32_t)(bvh.nodes.size() / 16), r.n_leaves = (uint32_t)topo.leaf_ref.size();
        r.fill = bvh.fill;
        c->refit_height_off = topo.height_off;
    }
    c->moved = false;
    c->n_bvh_nodes = (uint32_t)(bvh.nodes.size() / 16);
    c->n_bvh_leaves = bvh.n_leaves;
    c->bvh_depth = bvh.max_depth;
    for (int k = 0; k < 3; ++k)
        c->bvh_centre[k] = bvh.centre[k];
    c->bvh_pad_local = bvh.pad_local;
    c->bvh_root_leaf = bvh.root_leaf;
    // (the kernels' flat walk is written for y, the up axis of the reference's scenes; a tree flat along x or z walks the generic loop)
    c->bvh_flat_m = bvh.flat_axis == 1 ? bvh.flat_m : 0.0f, c->bvh_flat_e = bvh.flat_axis == 1 ? bvh.flat_e : -1.0f;
    for (int &o : c->occupancy)
        o = 0; // the tree kernels' LDS footprint follows the tree (depth of the traversal stack, size of the node table)
    for (int &o : c->cast_occupancy)
        o = 0;
    c->n_groups = ng;
    c->n_multi = n_multi;

    c->n_active = na;
    c->n_sweep = ns;
    c->n_padded_scene = s->count;
    c->cam = device_camera(*cam);
    for (int k = 0; k < 9; ++k)
        c->src_f32[k].assign(src[k], src[k] + s->count);
    c->src_mat.assign(s->mat_type, s->mat_type + s->count);
    c->src_cam = *cam;
    c->have_scene = true;
    c->default_variant = c->default_variant_tp = R1_V_TREE;
    return R1_OK;
}

// The camera alone: it travels by value in every launch's arguments, so nothing is built, uploaded or waited for, and launches already
// enqueued keep the camera they were enqueued with.
extern "C" int r1_set_camera(r1_context *c, const r1_camera *cam)
{
    if (!c || !cam)
    {
        r1_set_error("r1_set_camera: %s is NULL", !c ? "ctx" : "camera");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("r1_set_camera: no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    c->pass_valid = false; // (a progressive frame does not continue across a change of view, as across r1_set_scene)
    c->cam = device_camera(*cam);
    c->src_cam = *cam;       // r1_set_scene(same arrays, this camera) is still the shortcut
    return R1_OK;
}

// ---- moving spheres (include/rays1.h "moving spheres", r1_refit.hip) --------------------------------------------------

static int update_check(const char *who, r1_context *c, uint32_t first, uint32_t count, const void *x, const void *y, const void *z)
{
    if (!c)
    {
        r1_set_error("%s: ctx is NULL", who);
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("%s: no scene set (call r1_set_scene first)", who);
        return R1_EINVAL;
    }
    if ((uint64_t)first + count > c->n_padded_scene)
    {
        r1_set_error("%s: spheres [%u, %llu) are beyond the scene's %u", who, first, (unsigned long long)first + count, c->n_padded_scene);
        return R1_EINVAL;
    }
    if (count && (!x || !y || !z))
    {
        r1_set_error("%s: x, y and z must not be NULL with count > 0", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

// The move and the refit on `st`, centres from memory the device can read; then what an update changes in the context.  Nothing is waited
// for.  `moved_ev` (or null) is recorded straight behind the move kernel, the only reader of the centres.  Leaves the launch info and the
// timing events alone.
static int update_enqueue(r1_context *c, uint32_t first, uint32_t count, const float *dx, const float *dy, const float *dz, hipStream_t st,
                          hipEvent_t moved_ev)
{
    R1_HIP(r1_launch_refit_move(&c->refit, first, count, dx, dy, dz, st));
    if (moved_ev)
        R1_HIP(hipEventRecord(moved_ev, st));
    if (c->n_active) // (a tree of 0 spheres has nothing to refit)
        R1_HIP(r1_launch_refit(&c->refit, c->refit_height_off.data(), (uint32_t)c->refit_height_off.size() - 1u, st));
    c->moved = true;
    c->grid_valid = false;
    c->pass_valid = false; // (a progressive frame does not continue across a change of the scene)
    // the flat y slab (r1_bvh.cpp) is dropped, not refitted: it travels by value in the launches' arguments, and spheres that leave the
    // plane are exactly the case it must not miss.  The kernels take the generic loop they already have.
    c->bvh_flat_m = 0.0f, c->bvh_flat_e = -1.0f;
    return R1_OK;
}

extern "C" int r1_update_centers(r1_context *c, uint32_t first, uint32_t count, const float *x, const float *y, const float *z, void *hip_stream)
{
    int rc = update_check("r1_update_centers", c, first, count, x, y, z);
    if (rc || count == 0)
        return rc;
    for (uint32_t i = 0; i < count; ++i)
        if (c->scene_to_active[first + i] != 0xFFFFFFFFu && !(std::isfinite(x[i]) && std::isfinite(y[i]) && std::isfinite(z[i])))
        {
            r1_set_error("r1_update_centers: the new centre of sphere %u is not finite", first + i);
            return R1_EINVAL;
        }
    R1_HIP(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // the staging buffer: the move kernel of the previous update may still be reading it
    if (c->stage_busy)
        R1_HIP(hipEventSynchronize(c->stage_ev));
    c->stage_busy = false;
    if (!c->stage_ev)
        R1_HIP(hipEventCreateWithFlags(&c->stage_ev, hipEventDisableTiming));
    if (c->stage_cap < 3 * (size_t)count)
    {
        if (c->stage)
            R1_HIP(hipHostFree(c->stage));
        c->stage = c->stage_dev = nullptr, c->stage_cap = 0;
        R1_HIP(hipHostMalloc((void **)&c->stage, 3 * (size_t)count * 4, hipHostMallocMapped));
        R1_HIP(hipHostGetDevicePointer((void **)&c->stage_dev, c->stage, 0));
        c->stage_cap = 3 * (size_t)count;
    }
    memcpy(c->stage, x, (size_t)count * 4), memcpy(c->stage + count, y, (size_t)count * 4), memcpy(c->stage + 2 * (size_t)count, z, (size_t)count * 4);
    c->stage_busy = true; // (from here on: a launch that failed half-way may still have enqueued the move)
    if ((rc = update_enqueue(c, first, count, c->stage_dev, c->stage_dev + count, c->stage_dev + 2 * (size_t)count, st, c->stage_ev)))
        return rc;
    // the context's host copies follow (entries of spheres that are not active too: they are what r1_set_scene would be given)
    memcpy(c->src_f32[0].data() + first, x, (size_t)count * 4), memcpy(c->src_f32[1].data() + first, y, (size_t)count * 4);
    memcpy(c->src_f32[2].data() + first, z, (size_t)count * 4);
    return R1_OK;
}

extern "C" int r1_update_centers_device(r1_context *c, uint32_t first, uint32_t count, const void *d_x, const void *d_y, const void *d_z, void *hip_stream)
{
    int rc = update_check("r1_update_centers_device", c, first, count, d_x, d_y, d_z);
    if (rc || count == 0)
        return rc;
    if (((uintptr_t)d_x | (uintptr_t)d_y | (uintptr_t)d_z) & 3u)
    {
        r1_set_error("r1_update_centers_device: d_x, d_y and d_z must be 4-byte aligned");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    return update_enqueue(c, first, count, (const float *)d_x, (const float *)d_y, (const float *)d_z, hip_stream ? (hipStream_t)hip_stream : c->stream, nullptr);
}

extern "C" int r1_bvh_download(r1_context *c, float *nodes_out, size_t nodes_cap, size_t *nodes)
{
    if (!c || !nodes)
    {
        r1_set_error("r1_bvh_download: %s is NULL", !c ? "ctx" : "nodes");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("r1_bvh_download: no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    *nodes = c->n_bvh_nodes;
    if (!nodes_out)
        return R1_OK;
    if (nodes_cap < 16 * (size_t)c->n_bvh_nodes)
        return R1_ELIMIT;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipMemcpyAsync(nodes_out, c->bvh_nodes.p, 64 * (size_t)c->n_bvh_nodes, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

// ---- per-frame setup ------------------------------------------------------------------------------

static bool same_tiling(const r1_params &a, const r1_params &b)
{
    return a.width == b.width && a.height == b.height && a.spp == b.spp && a.tile_w == b.tile_w && a.tile_h == b.tile_h &&
           a.shard == b.shard && a.num_shards == b.num_shards;
}

static R1FastDiv make_div(uint32_t d)
{
    R1FastDiv r;
    uint32_t sh = 0;
    while ((2u << sh) <= d && sh < 31)
        ++sh; // floor(log2 d)
    if ((d & (d - 1)) == 0)
    {
        r.pow2 = 1, r.shift = sh, r.mul = 0;
    }
    else
    {
        r.pow2 = 0, r.shift = sh;
        r.mul = (uint32_t)((((uint64_t)1 << (32 + sh)) + d - 1) / d);
    }
    return r;
}

static int prepare_tiles(r1_context *c, const r1_params *p, int n_frames)
{
    if (c->tile_key_valid && same_tiling(c->tile_key, *p) && c->tile_frames == n_frames)
        return R1_OK;
    const int tiles_x = (p->width + p->tile_w - 1) / p->tile_w;
    const int tiles_y = (p->height + p->tile_h - 1) / p->tile_h;
    const int total = tiles_x * tiles_y;
    const uint32_t local = total > p->shard ? (uint32_t)((total - p->shard + p->num_shards - 1) / p->num_shards) : 0u;
    const uint64_t full = (uint64_t)p->tile_w * p->tile_h * p->spp;
    if (full * local * (uint64_t)n_frames >= ((uint64_t)1 << 31) || (uint64_t)total * p->num_shards >= ((uint64_t)1 << 31))
    {
        r1_set_error("%d frame(s) of %dx%dx%d with %dx%d tiles exceed 2^31 sample slots per launch", n_frames, p->width, p->height, p->spp, p->tile_w,
                     p->tile_h);
        return R1_ELIMIT;
    }
    c->n_local_tiles = local;
    c->full = (uint32_t)full;
    c->total_samples = (uint32_t)(full * local * (uint64_t)n_frames); // the launch's queue: frame-major
    c->tile_key = *p;
    c->tile_frames = n_frames;
    c->tile_key_valid = true;
    return R1_OK;
}

// The context's counter allocation: [0, R1_COUNTER_BYTES) queue heads (set 0), ray count, diagnostic counters — the block the round-3
// kernels zero between frames; then R1_COUNTER_TAIL bytes: +0 the published ray count, +64 eight batch-argument slots, +1024 queue heads
// (set 1); then, per launch (R1_LAND): frame_rays[F] (uint64), frame_left[F] (uint32, padded), tile_cnt[F x local tiles] (uint32).
// Called by every entry point BEFORE it takes addresses inside the allocation (it may move when the launch needs more room).
static size_t land_frames_off() { return (size_t)R1_COUNTER_BYTES + R1_COUNTER_TAIL; }
static int ensure_counters(r1_context *c, const r1_params *p, int n_frames)
{
    int rc = prepare_tiles(c, p, n_frames);
    if (rc)
        return rc;
    const size_t F = (size_t)(n_frames > 0 ? n_frames : 1);
    const size_t tiles = F * (size_t)(c->n_local_tiles ? c->n_local_tiles : 1);
    const size_t need = land_frames_off() + ((F * 16 + 127) & ~(size_t)127) + tiles * 4 * R1_LAND_CNT_STRIDE;
    if (c->counters.p && need <= c->counters.cap)
        return R1_OK;
    R1_HIP(hipStreamSynchronize(c->stream)); // (a frame in flight on another stream is the caller's to order: one frame per context at a time)
    if ((rc = ensure(c->counters, need + need / 2)))
        return rc;
    R1_HIP(hipMemsetAsync(c->counters.p, 0, c->counters.cap, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    c->counters_clean = true;
    c->land_prev = false, c->land_armed = false, c->land_parity = 0;
    c->batch_args_slot = -1;
    return R1_OK;
}

// Frame batch of the throughput entry points: n_frames frames in one launch (r1_device.h R1TraceArgs::n_frames); frame f is
// written to d_out + f * out_stride and its uint64 ray count to d_out + f * out_stride + rays_offset.
struct Batch
{
    int n_frames = 1;
    uint32_t seed_stride = 0;
    size_t out_stride = 0, rays_offset = 0;
    const r1_camera *cameras = nullptr; // a camera path: [n_frames], host memory; null: every frame through the context's camera
};

// Where the caller finally wants the frame, if the device can write there (page-locked host memory): launches that resolve their own
// tiles (R1_LAND) store the pixels and the count there directly and set `used`; the entry point then enqueues no copy.
struct Landing
{
    void *out = nullptr;  // device address of the caller's pixels (row-major image, or the frame records of a batch)
    void *rays = nullptr; // ... of its ray count (single frames)
    bool used = false;
};

// A progressive pass (r1_render_pass): samples [first_sample, first_sample + spp) traced by the R1_MODE_PASS kernels, then r1_accum_kernel instead of
// the resolve launch.  d_out of enqueue_frame receives the preview unless `image` is false.
// A pass of r1_render_adaptive has a tile list: the launch's tiles are list[0, n_listed) of the frame's, traced by the R1_MODE_LISTED kernels and summed
// and tested by r1_adapt_accum_kernel (accumulators and reports: the context's, indexed by tile of the frame).
struct Pass
{
    int32_t first_sample = 0;
    bool image = true;
    const uint32_t *list = nullptr; // device memory
    uint32_t n_listed = 0;
    const r1_adaptive *rule = nullptr;
};

// device address of page-locked host memory (r1_host_alloc, hipHostMalloc, hipHostRegister), or null for anything else
static void *mapped_host(const void *ptr)
{
    if (!ptr)
        return nullptr;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess)
    {
        (void)hipGetLastError(); // ordinary (pageable) memory is not an error here
        return nullptr;
    }
    return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
}

// R1_VARIANT_GRID: builds the uniform grid of the context's scene (from the arrays r1_set_scene received, so that r1_grid_describe and
// r1_grid_visit see the same grid) and uploads it, once per scene.  Contexts that never ask for the grid pay nothing for it.
static int ensure_grid(r1_context *c)
{
    if (c->grid_valid)
        return R1_OK;
    r1_scene s;
    s.count = (uint32_t)c->src_mat.size();
    s.center_x = c->src_f32[0].data(), s.center_y = c->src_f32[1].data(), s.center_z = c->src_f32[2].data();
    s.radius_sq = c->src_f32[3].data(), s.inv_radius = c->src_f32[4].data(), s.mat_type = c->src_mat.data();
    s.albedo_r = c->src_f32[5].data(), s.albedo_g = c->src_f32[6].data(), s.albedo_b = c->src_f32[7].data(), s.mat_param = c->src_f32[8].data();
    R1Grid g;
    if (r1_grid_from_scene(&s, g) != R1_OK)
    {
        r1_set_error("grid: the scene's spheres could not be read");
        return R1_EINVAL;
    }
    // small-scene kernel: 16-bit cell starts and ids, all of it copied into every workgroup's LDS
    const size_t halves = g.start.size() + g.ids.size();
    c->grid_small = c->n_active <= R1_MAX_ACTIVE_10BIT && halves <= R1_GRID_LDS_HALVES && g.ids.size() < 65536u;
    std::vector<uint32_t> tab32;
    std::vector<uint16_t> tab16;
    size_t tab_bytes;
    if (c->grid_small)
    {
        tab16.assign((halves + 7) & ~(size_t)7, 0); // (whole 16-byte rows: the kernel copies float4)
        for (size_t q = 0; q < g.start.size(); ++q)
            tab16[q] = (uint16_t)g.start[q];
        for (size_t q = 0; q < g.ids.size(); ++q)
            tab16[g.start.size() + q] = (uint16_t)g.ids[q];
        tab_bytes = tab16.size() * 2;
    }
    tab32 = g.start;
    tab32.insert(tab32.end(), g.ids.begin(), g.ids.end());
    if (!c->grid_small)
        tab_bytes = tab32.size() * 4;
    std::vector<uint32_t> outl = g.outliers;
    if (outl.empty())
        outl.push_back(0u);
    int rc;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipDeviceSynchronize()); // (launches of an earlier grid may still read the buffers that are about to be replaced)
    if ((rc = ensure(c->grid_tab, tab_bytes)) || (rc = ensure(c->grid_out, outl.size() * 4)) || (rc = ensure(c->grid_tab32, tab32.size() * 4)))
        return rc;
    R1_HIP(hipMemcpyAsync(c->grid_tab32.p, tab32.data(), tab32.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->grid_tab.p, c->grid_small ? (const void *)tab16.data() : (const void *)tab32.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->grid_out.p, outl.data(), outl.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    R1GridArgs &G = c->grid_args;
    memset(&G, 0, sizeof(G));
    G.geom = g.geom;
    G.outliers = (const uint32_t *)c->grid_out.p;
    G.n_out = (uint32_t)g.outliers.size();
    G.n_start = (uint32_t)g.start.size();
    G.tab = (const uint32_t *)c->grid_tab.p;
    G.lds_bytes = c->grid_small ? (uint32_t)tab_bytes : 0u;
    R1GridArgs G32 = G;
    G32.tab = (const uint32_t *)c->grid_tab32.p, G32.lds_bytes = 0;
    if ((rc = ensure(c->grid_dev, sizeof(G))) || (rc = ensure(c->grid_dev32, sizeof(G))))
        return rc;
    R1_HIP(hipMemcpyAsync(c->grid_dev.p, c->grid_small ? &G : &G32, sizeof(G), hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->grid_dev32.p, &G32, sizeof(G), hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    c->grid_valid = true;
    return R1_OK;
}

// ---- one frame, step by step (enqueue_frame at the end) ------------------------------------------------------------------------------

// What a frame launches: decided once by choose_kernel, read by every step.
struct Choice
{
    int variant;      // what was asked for, R1_V_* (DEFAULT resolved): r1_launch_info's kernel; a diagnostic wish (r1_is_stats) keeps its counters
                      // even where the product build runs in its place
    R1Build b;        // the build of the trace body that runs (r1_pick); the wavefront variant: the build its launches are sized by
    bool land;        // tiles resolved inside the trace kernel: the product kernels' launches; the diagnostic builds, the reference-form
                      // sweep, the wavefront variant and PIXEL mode keep the round-3 form (records + r1_resolve_kernel, or no records at all)
    bool fused_clear; // the frame's last launch publishes the ray count and zeroes the counter block (close_frame)
};

// Big-scene kernels — 32-bit hit indices, the attenuation stack in a global workspace (the packed LDS stack holds 10-bit indices) and the
// tree's node table through the vector L1: > 1023 hittable spheres, or — tree kernels — a node table too large for LDS, or a tree whose pad
// is measured per node (small spheres: only the kernels that walk the table in global memory carry that arm, bvh_advance); grid kernels:
// tables too large for LDS — the small-scene grid kernel's fallback reads the tree from global memory, any tree will do — and PIXEL mode
// (`grid_pixel`), which the grid runs through its big-scene kernel only: the small one's PIXEL build would spill.  Tried for the tree kernel
// on small scenes too (more workgroups per CU): 15 % slower.  A grid's answer holds after ensure_grid.
static bool big_scene(const r1_context *c, bool tree, bool grid, bool grid_pixel)
{
    return c->n_active > R1_MAX_ACTIVE_10BIT || (tree && (c->n_bvh_nodes > R1_NODES_LDS_MAX || c->bvh_pad_local)) || (grid && (!c->grid_small || grid_pixel));
}

// The public enum's numbers are the internal ones.  DEFAULT = the box tree (a property of the build, see above); PREFILTER always forces
// the exhaustive sweep, BVH always the tree; all of them produce the same pixels.
static int resolve_variant(const r1_context *c, int32_t wanted, bool throughput_mode)
{
    static_assert(R1_VARIANT_REFERENCE == R1_V_REFERENCE && R1_VARIANT_PREFILTER == R1_V_SWEEP && R1_VARIANT_STATS == R1_V_SWEEP_STATS &&
                  R1_VARIANT_BVH == R1_V_TREE && R1_VARIANT_BVH_STATS == R1_V_TREE_STATS && R1_VARIANT_WAVEFRONT == R1_V_WAVEFRONT &&
                  R1_VARIANT_GRID == R1_V_GRID && R1_VARIANT_GRID_STATS == R1_V_GRID_STATS, "the kernels' variant numbers (r1_builds.h)");
    if (wanted == R1_VARIANT_DEFAULT)
        return throughput_mode ? c->default_variant_tp : c->default_variant;
    return wanted >= R1_VARIANT_REFERENCE && wanted <= R1_VARIANT_GRID_STATS ? wanted : R1_V_SWEEP;
}

// Kernel choice, after the launch's tiles are known (size_tiles) and the grid is built.  Kernel mode: the host-returning entry points run
// in latency mode, the throughput entry point with few long-lived waves per frame — per-sample records + r1_resolve_kernel either way,
// unless r1_set_pixel_mode chose PIXEL mode for the throughput entry point (a lane owns a pixel: no sample records, no resolve launch,
// ~10 % slower).  Refuses what is not built; changes nothing.
static int choose_kernel(const r1_context *c, const r1_params *p, int variant, bool throughput_mode, const Batch *batch, const Pass *pass, Choice &k)
{
    k.variant = variant;
    const bool wavefront = variant == R1_V_WAVEFRONT;
    const bool big = big_scene(c, r1_is_tree(variant), r1_is_grid(variant), throughput_mode && c->pixel_mode);
    const bool frames = batch && batch->n_frames > 1; // (a batch or path of one frame: the single-frame kernel, a path's camera by value)
    static const int tp_mode_env = (int)r1_knob("R1_TP_MODE", -1); // tuning experiments: R1_MODE_TP, _LAT or _PIXEL for the throughput entry points
    int want = R1_MODE_LAT;
    if (pass)
        want = pass->list ? R1_MODE_LISTED : R1_MODE_PASS;
    else if (throughput_mode && (c->pixel_mode || tp_mode_env == R1_MODE_PIXEL))
        want = R1_MODE_PIXEL;
    else if (throughput_mode && !(tp_mode_env == R1_MODE_LAT && !big)) // (big scenes have no latency build: the knob leaves them alone)
        want = !frames ? R1_MODE_TP : batch->cameras ? R1_MODE_PATH : R1_MODE_BATCH;
    // (the wavefront variant has kernels of its own; its grid is sized as the grouped sweep's frames in flight are)
    const bool built = wavefront ? r1_pick(R1_V_SWEEP, big, R1_MODE_TP, k.b) : r1_pick(variant, big, want, k.b);
    if (!built && pass)
    {
        r1_set_error("variant %d has no progressive-pass build", p->variant);
        return R1_EINVAL;
    }
    if (batch && (!built || !r1_mode_is_tp_family(k.b.mode) || wavefront || r1_is_stats(variant) || variant == R1_V_REFERENCE))
    {
        r1_set_error("frame batches run through the throughput kernels only (no PIXEL mode, no diagnostic / reference-form / wavefront variant)");
        return R1_EINVAL;
    }
    if (!built)
    {
        r1_set_error("variant %d has no kernel for this call", p->variant);
        return R1_EINVAL;
    }
    k.land = r1_build_lands(k.b.variant, k.b.stats, k.b.mode) && c->total_samples > 0;
    // Frames without a resolve launch, and the diagnostic builds, whose counters are read back afterwards, count into the caller's word
    // and clear with memsets.
    k.fused_clear = !k.land && k.b.mode != R1_MODE_PIXEL && c->n_local_tiles && c->total_samples && !r1_is_stats(variant);
    return R1_OK;
}

// The launch's tiles: the counter allocation (which may move: addresses inside it are taken after this) and the context's tile numbers.
// A listed pass has the list's length as its tile count — grid size, queue length and record buffer follow from it — so n_local_tiles and
// total_samples are rewritten BEFORE anything is sized, and the cached tiling, which no longer describes the params it is kept under, is
// dropped: the next call derives its own.  A pass of r1_render_pass gets its accumulator.
static int size_tiles(r1_context *c, const r1_params *p, int n_frames, const Pass *pass)
{
    int rc = ensure_counters(c, p, n_frames);
    if (rc)
        return rc;
    if (pass && pass->list)
    {
        c->n_local_tiles = pass->n_listed;
        c->total_samples = c->full * pass->n_listed;
        c->tile_key_valid = false;
    }
    else if (pass)
        return ensure(c->accum, (size_t)c->n_local_tiles * p->tile_w * p->tile_h * 16);
    return R1_OK;
}

// The launch's sample records (none in PIXEL mode), and a batch's partial ray counts where a resolve launch will follow
static int ensure_records(r1_context *c, const r1_params *p, const Choice &k, const Batch *batch, hipStream_t st)
{
    int rc;
    if (batch && !(R1_LAND && k.variant == R1_V_TREE))
    {
        // partial ray counts of the resolve launch: one uint64 per (tile of the batch, workgroup column)
        const size_t cols = ((size_t)p->tile_w * p->tile_h + 255) / 256;
        if ((rc = ensure(c->batch_rays, (size_t)batch->n_frames * (c->n_local_tiles ? c->n_local_tiles : 1) * cols * 8)))
            return rc;
    }
    if (k.b.mode == R1_MODE_PIXEL)
        return R1_OK;
    const size_t want = (size_t)(c->total_samples ? c->total_samples : 1) * 16;
    const bool fresh = !c->samples.p || c->samples.cap < want;
    if ((rc = ensure(c->samples, want)))
        return rc;
    if (fresh) // a record is recognised by its launch's tag: fresh memory must not carry one by accident
        R1_HIP(hipMemsetAsync(c->samples.p, 0, c->samples.cap, st));
    return R1_OK;
}

// The context's scene as the kernels read it: every table and number of R1DeviceScene (renders and ray queries alike)
static void fill_scene(const r1_context *c, R1DeviceScene &s)
{
    s.sweep = (const float4 *)c->sweep.p, s.exact = (const float4 *)c->exact.p, s.exact_g = (const float4 *)c->exact_g.p;
    s.shade = (const float4 *)c->shade.p, s.mat = (const float4 *)c->mat.p, s.members = (const uint32_t *)c->members.p;
    s.n_active = c->n_active, s.n_sweep = c->n_sweep, s.n_multi = c->n_multi;
    s.bvh_nodes = (const float4 *)c->bvh_nodes.p, s.bvh_prims = (const float4 *)c->bvh_prims.p, s.bvh_ids = (const uint32_t *)c->bvh_ids.p;
    for (int k = 0; k < 3; ++k)
        s.bvh_centre[k] = c->bvh_centre[k];
    s.bvh_pad_local = (uint32_t)c->bvh_pad_local, s.bvh_root_leaf = (uint32_t)c->bvh_root_leaf;
    s.bvh_flat_m = c->bvh_flat_m, s.bvh_flat_e = c->bvh_flat_e;
}

// The walk's share of the arguments, trace and cast kernels alike: the traversal stack's depth and the workgroups' LDS copy of the node
// table — all of it for small scenes, the first `top_nodes` >= 1 in breadth-first order for big ones (the walk's root step reads node 0
// from the LDS copy); none where the tree is walked from global memory (!tree_lds: a fallback, the plain cast).
static void fill_walk(const r1_context *c, bool tree_lds, bool big, uint32_t top_nodes, R1TraceArgs &a)
{
    a.bvh_depth = c->bvh_depth > 0 ? c->bvh_depth : 1;
    a.bvh_lds_f4 = !tree_lds ? 0u : (!big ? 4u * c->n_bvh_nodes : 4u * std::min(c->n_bvh_nodes, top_nodes));
}

// Everything of R1TraceArgs that follows from the context, the params and the kernel choice; the batch block, the grid size and the
// landing are the later steps'.  Takes addresses inside the counter allocation: after size_tiles.
static void frame_args(const r1_context *c, const r1_params *p, const Choice &k, const Batch *batch, void *d_out, int block_layout, void *d_rays, R1TraceArgs &a)
{
    memset(&a, 0, sizeof(a));
    fill_scene(c, a.scene);
    a.cam = batch && batch->cameras && batch->n_frames == 1 ? device_camera(batch->cameras[0]) : c->cam;
    a.width = p->width, a.height = p->height, a.spp = p->spp, a.max_bounces = p->max_bounces;
    a.seed = p->seed;
    a.inv_w = 1.0f / p->width, a.inv_h = 1.0f / p->height; // Vec3 inv_image_size(1.0f / td.image_w, 1.0f / td.image_h, 0) rayweek1.cpp:746
    a.tile_w = p->tile_w, a.tile_h = p->tile_h, a.tiles_x = (p->width + p->tile_w - 1) / p->tile_w;
    a.shard = p->shard, a.num_shards = p->num_shards;
    a.n_local_tiles = c->n_local_tiles, a.full = c->full, a.total_samples = c->total_samples;
    a.div_full = make_div(c->full), a.div_spp = make_div((uint32_t)p->spp), a.div_tw = make_div((uint32_t)p->tile_w), a.div_tx = make_div((uint32_t)a.tiles_x);
    a.queue = (uint32_t *)((char *)c->counters.p + 1024);
    static const int coop_env = (int)r1_knob("R1_COOP_LANES", -1);
    a.coop_lanes = coop_env >= 0 ? (uint32_t)coop_env : R1_COOP_LANES;
    a.samples = (float4 *)c->samples.p;
    a.num_rays = k.fused_clear ? (unsigned long long *)((char *)c->counters.p + 32) : (unsigned long long *)d_rays;
    a.stats = r1_is_stats(k.variant) ? (unsigned long long *)((char *)c->counters.p + 128) : nullptr;
    if (r1_is_grid(k.variant))
        a.grid = (const R1GridArgs *)(k.b.big ? c->grid_dev32.p : c->grid_dev.p), a.scene.bvh_root_leaf = 0u; // (the grid kernels' fallback walks the tree from its root: no root step, r1_trace.hpp)
    static const int big_top_env = (int)r1_knob("R1_BIG_TOP", R1_BVH_TOP_NODES); // tuning experiments
    fill_walk(c, r1_is_tree(k.variant), k.b.big, (uint32_t)std::max(1, big_top_env), a);
    if (k.b.mode == R1_MODE_PIXEL)
    {
        // the queue holds the padded pixels of the shard's tiles, and `samples` is the output the kernel resolves into
        const uint32_t tp = (uint32_t)(p->tile_w * p->tile_h);
        a.full = tp, a.div_full = make_div(tp), a.total_samples = c->n_local_tiles * tp;
        a.samples = (float4 *)d_out, a.block_layout = block_layout;
        a.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
    }
}

// Takes a batch-argument slot (eight 32-byte slots in the counter allocation behind the published ray count) and writes `words` into it by a
// launch of its own, in stream order: the previous launch through this context has finished reading its copy by the time this one is
// written, and a NEW slot leaves a launch still reading the previous numbers undisturbed.  `cache` (a batch's numbers): an unchanged batch
// on the same stream reuses its slot and writes nothing.  cache == null (a path, whose block ends in a table address, and a pass): always a
// new slot, and batch_args_last is cleared, so that a batch that follows takes a new slot too (its numbers never equal the cleared ones:
// n_frames >= 2).  Returns the slot.
static int put_batch_args(r1_context *c, const void *words, int n_words, const R1BatchArgs *cache, hipStream_t st, const R1BatchArgs **slot)
{
    char *const slots = (char *)c->counters.p + R1_COUNTER_BYTES + 64;
    if (!cache || c->batch_args_slot < 0 || c->batch_args_stream != st || memcmp(cache, &c->batch_args_last, sizeof(*cache)) != 0)
    {
        c->batch_args_slot = (c->batch_args_slot + 1) & 7;
        if (cache)
            c->batch_args_last = *cache;
        else
            memset(&c->batch_args_last, 0, sizeof(c->batch_args_last));
        c->batch_args_stream = st;
        R1_HIP((n_words == 8 ? r1_launch_put8 : r1_launch_put6)(slots + 32 * c->batch_args_slot, (const uint32_t *)words, st));
    }
    *slot = (const R1BatchArgs *)(slots + 32 * c->batch_args_slot);
    return R1_OK;
}

// A camera path's table of cameras in device memory, written in stream order into the half of path_cams the previous path did not use.
// The one step of a frame that allocates on the heap (the rows travel in the arguments of the launches that write them).
static int put_path_cameras(r1_context *c, const Batch *batch, hipStream_t st, const float **table_out)
{
    const int n_frames = batch->n_frames;
    const size_t half = ((size_t)n_frames * R1_PATH_CAM_F4 * 16 + 255) & ~(size_t)255;
    int rc = ensure(c->path_cams, 2 * half); // (growing frees the old table: hipFree waits for the launches that read it)
    if (rc)
        return rc;
    c->path_cams_half ^= 1;
    char *const table = (char *)c->path_cams.p + (c->path_cams_half ? c->path_cams.cap / 2 : 0);
    std::vector<float> rows((size_t)n_frames * R1_PATH_CAM_F4 * 4, 0.0f);
    for (int f = 0; f < n_frames; ++f)
    {
        const R1DeviceCamera d = device_camera(batch->cameras[f]);
        static_assert(sizeof(R1DeviceCamera) == 19 * 4 && R1_PATH_CAM_F4 * 4 >= 19, "a table row holds an R1DeviceCamera");
        memcpy(&rows[(size_t)f * R1_PATH_CAM_F4 * 4], &d, sizeof(d));
    }
    R1_HIP(r1_launch_put_cameras(table, rows.data(), n_frames, st));
    *table_out = (const float *)table;
    return R1_OK;
}

// R1TraceArgs::batch (null in a single frame): a batch's numbers, behind them a path's camera table; or a pass's first sample and tile
// list, which the R1_MODE_PASS / _LISTED kernels read where a sample is seeded.
static int put_batch_block(r1_context *c, const Choice &k, const Batch *batch, const Pass *pass, hipStream_t st, R1TraceArgs &a)
{
    static_assert(sizeof(R1BatchArgs) == 24 && sizeof(R1PassArgs) == 24, "r1_launch_put6 writes the six words of R1BatchArgs / R1PassArgs");
    static_assert(sizeof(R1PathArgs) == 32 && __builtin_offsetof(R1PathArgs, cameras) == 24, "r1_launch_put8 writes the eight words of R1PathArgs into a 32-byte slot");
    int rc;
    if (r1_mode_is_batch(k.b.mode))
    {
        const bool path = k.b.mode == R1_MODE_PATH;
        R1PathArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.batch.n_frames = (uint32_t)batch->n_frames, pa.batch.seed_stride = batch->seed_stride;
        pa.batch.div_tiles = make_div(c->n_local_tiles ? c->n_local_tiles : 1u), pa.batch.n_local_tiles = c->n_local_tiles;
        if (path && (rc = put_path_cameras(c, batch, st, &pa.cameras)))
            return rc;
        if ((rc = put_batch_args(c, &pa, path ? 8 : 6, path ? nullptr : &pa.batch, st, &a.batch)))
            return rc;
    }
    if (pass)
    {
        R1PassArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.first_sample = (uint32_t)pass->first_sample;
        pa.list = pass->list;
        return put_batch_args(c, &pa, 6, nullptr, st, &a.batch);
    }
    return R1_OK;
}

// Workgroups per CU of the chosen kernel with the dynamic LDS its launch will have (r1_walk_lds: the size r1_launch_trace launches with),
// 1 .. 8.  Asked once per build and scene: the tree kernels' LDS footprint follows the tree, r1_set_scene clears the cache.
static int occupancy_slot(const R1Build &b) { return ((b.variant * 2 + (b.stats ? 1 : 0)) * 2 + (b.big ? 1 : 0)) * R1_MODES + b.mode; }
static int blocks_per_cu(r1_context *c, const Choice &k, const R1TraceArgs &a, int *per_cu)
{
    R1Build b = k.b;
    if (r1_mode_is_batch(b.mode))
        b.mode = R1_MODE_TP; // (the batch build of a kernel has the occupancy of its single-frame build)
    int &occ = c->occupancy[occupancy_slot(b)];
    if (occ == 0)
        R1_HIP(r1_trace_occupancy(b, r1_walk_lds(b.variant, b.big, a.bvh_depth, a.bvh_lds_f4, c->grid_args.lds_bytes), &occ));
    static const int per_cu_env = (int)r1_knob("R1_BLOCKS_PER_CU", 0); // tuning experiments
    *per_cu = std::min(std::max(occ, 1), 8);
    if (per_cu_env > 0 && per_cu_env < *per_cu)
        *per_cu = per_cu_env;
    return R1_OK;
}

// The persistent grid and how its waves take work from the queue.  Changes nothing but its result.
struct GridSize { long long blocks; uint32_t chunk_min, chunk_max, nq; };
// total: sample slots of the launch; pixels: PIXEL mode — the padded pixels the queue holds instead — else 0; latency: r1_runs_as_latency of the build
static GridSize size_grid(int cus, int per_cu, uint32_t total, uint32_t pixels, bool pixel_mode, bool latency, bool throughput_mode, int num_shards)
{
    GridSize g;
    // Latency mode (the synchronous host entry points: one frame, the caller waits): as many waves as fit, every lane at least one
    // sample.  Throughput mode (the device-resident entry point, frames in flight on several streams): a wave's lanes run dry one by one
    // at the end of its share (the longest bounce chain of 64 lanes is ~20 sweeps), so a wave needs many times that much work to stay
    // full — give every lane >= R1_SAMPLES_PER_LANE samples and let the other frames fill the CUs a small frame leaves.
    static const long long spl_env = r1_knob("R1_SAMPLES_PER_LANE", R1_SAMPLES_PER_LANE);
    static const long long minb_env = r1_knob("R1_MIN_BLOCKS", R1_MIN_BLOCKS);
    long long needed = ((long long)total + R1_BLOCK - 1) / R1_BLOCK;
    if (throughput_mode)
    {
        // few, long-lived workgroups per frame (>= R1_SAMPLES_PER_LANE samples per lane), but not fewer
        // than R1_MIN_BLOCKS while that still leaves R1_SAMPLES_PER_LANE_MIN samples per lane
        const long long spl = num_shards > 1 ? R1_SAMPLES_PER_LANE_SHARD : (spl_env > 0 ? spl_env : 1);
        const long long hi = ((long long)total + R1_BLOCK * spl - 1) / (R1_BLOCK * spl);
        const long long lo = ((long long)total + R1_BLOCK * R1_SAMPLES_PER_LANE_MIN - 1) / (R1_BLOCK * R1_SAMPLES_PER_LANE_MIN);
        needed = std::max(hi, std::min(minb_env, lo));
    }
    g.blocks = std::max(1LL, std::min((long long)cus * per_cu, needed));
    // Queue chunk per atomic: guided (remaining / (2 waves)) between chunk_min and chunk_max.  Large
    // chunks keep a wave on consecutive samples (coherent primary rays, whole sample-record lines)
    // and save atomics — measured at N = 1: 256 -> 1.227 ms, 1024 -> 1.197, 4096 -> 1.231 —
    // but they must stay small against a wave's share of the frame (8 shards: 1024 costs 12 %).
    static const int chunk_max_env = (int)r1_knob("R1_CHUNK", 0), chunk_min_env = (int)r1_knob("R1_CHUNK_MIN", 0), nq_env = (int)r1_knob("R1_NQ", 0);
    const long long waves = g.blocks * (R1_BLOCK / 64);
    if (pixel_mode) // chunks in pixels (a wave holds 64 pixels at a time)
    {
        g.chunk_max = (uint32_t)std::min(128LL, std::max(16LL, (long long)pixels / (waves * 12)));
        g.chunk_min = 8;
    }
    else
    {
        const long long cm = std::min<long long>(R1_CHUNK_BIG, std::max<long long>(R1_CHUNK, (long long)total / (waves * 12)));
        g.chunk_max = chunk_max_env > 0 ? (uint32_t)chunk_max_env : (uint32_t)cm;
        g.chunk_min = std::min(chunk_min_env > 0 ? (uint32_t)chunk_min_env : R1_CHUNK_MIN, g.chunk_max);
    }
    // Latency mode: every wave of the full grid takes one wave-full of samples per atomic (what a wave still holds when the queue runs
    // dry is the frame's tail: with 256-sample chunks the waves found the queue empty over a span of 0.7 ms), which one counter cannot
    // serve: sub-queues.
    g.nq = 1;
    if (latency)
    {
        // a wave only ever pulls from its home sub-queue (r1_trace.hpp: home = (4 (block / 8) + wave) % nq), so every
        // sub-queue needs home waves: the full groups of 8 workgroups must cover all nq residues
        const long long nq = std::min<long long>({nq_env > 0 ? nq_env : R1_SUBQUEUES, 4 * (g.blocks / 8), (R1_COUNTER_BYTES - 1024) / 128});
        if (nq > 1)
        {
            g.nq = (uint32_t)nq;
            g.chunk_max = g.chunk_min = chunk_max_env > 0 ? (uint32_t)chunk_max_env : 64u;
        }
    }
    return g;
}

// Landing set-up (tiles resolved inside the trace kernel): the launch's set of queue heads, its record tag, the armed countdowns, where the
// tiles land and the waves' tile lists.
// Launches alternate between two sets of queue heads and wave counts; workgroup 0 zeroes the set the launch before used, which nobody
// touches any more (a workgroup that starts late still asks its own queue for work after the frame's last tile has been summed, so a
// launch cannot clear its own).  After anything else has run through this context both sets (and the round-3 block) are cleared here.
// land_prev and land_armed are cleared BEFORE anything here can fail, and they and land_parity are committed by enqueue_frame only once
// the trace launch is enqueued: until then the context counts as neither, so a call refused from here on (tile lists too long, an
// allocation, the launch) sends the next one through both memsets and the arming launch — it would otherwise take the set the last
// launch that ran left exhausted, and no tile would be summed.
static int land_setup(r1_context *c, const r1_params *p, const Batch *batch, Landing *landing, long long blocks, int block_layout, hipStream_t st,
                      R1TraceArgs &a, void *&d_out, void *&d_rays, int &land_parity)
{
    const int n_frames = batch ? batch->n_frames : 1;
    const bool prev = c->land_prev, armed = c->land_armed;
    c->land_prev = false, c->land_armed = false;
    land_parity = prev ? c->land_parity ^ 1 : 0;
    if (!prev)
    {
        R1_HIP(hipMemsetAsync(c->counters.p, 0, R1_COUNTER_BYTES, st));
        R1_HIP(hipMemsetAsync((char *)c->counters.p + R1_COUNTER_BYTES + 1024, 0, R1_COUNTER_BYTES - 1024, st)); // (not the batch-argument slots in front of it)
    }
    char *const set0 = (char *)c->counters.p + 1024, *const set1 = (char *)c->counters.p + R1_COUNTER_BYTES + 1024;
    a.queue = (uint32_t *)(land_parity ? set1 : set0);
    a.land.clear_heads = (uint32_t *)(land_parity ? set0 : set1);
    a.land.clear_count = (R1_COUNTER_BYTES - 1024) / 128;
    static_assert((R1_COUNTER_BYTES - 1024) / 128 <= R1_BLOCK && R1_COUNTER_TAIL >= 1024 + (R1_COUNTER_BYTES - 1024), "the second set of queue heads fits the tail");
    // the launch's generation tags its sample records (1 .. 2^24 - 1; on wrap-around the records are wiped).  Advanced at once, even by
    // a call that is refused later: a tag no launch used costs nothing, one used again could let stale records pass for new ones
    c->land_gen = (c->land_gen + 1) & 0xFFFFFFu;
    if (c->land_gen == 0)
    {
        R1_HIP(hipMemsetAsync(c->samples.p, 0, c->samples.cap, st));
        c->land_gen = 1;
    }
    a.land_tag = c->land_gen << 8;
    a.land_res = 1; // (a landing launch: r1_launch_trace checks that the kernel and the launch agree)
    unsigned long long *frame_rays = (unsigned long long *)((char *)c->counters.p + land_frames_off());
    uint32_t *frame_left = (uint32_t *)(frame_rays + n_frames);
    a.land_cnt = (uint32_t *)((char *)frame_rays + (((size_t)n_frames * 16 + 127) & ~(size_t)127)); // (every countdown on a 128-byte line of its own)
    if (!armed || c->land_frames != n_frames || !same_tiling(c->land_key, *p))
    {
        R1_HIP(r1_launch_land_arm(a.land_cnt, frame_rays, frame_left, (uint32_t)n_frames, c->n_local_tiles, p->width, p->height, p->spp, p->tile_w, p->tile_h,
                                  a.tiles_x, p->shard, p->num_shards, st));
        c->land_frames = n_frames, c->land_key = *p; // (land_armed: committed with the launch)
    }
    if (landing && landing->out && (batch || landing->rays))
    {
        d_out = landing->out;
        if (!batch)
            d_rays = landing->rays;
        landing->used = true;
    }
    a.land.out = (uint8_t *)d_out, a.land.rays_dst = (unsigned long long *)d_rays;
    a.land.out_stride = batch ? batch->out_stride : 0, a.land.rays_offset = batch ? batch->rays_offset : 0, a.land.rays_in_out = batch ? 1u : 0u;
    a.land.frame_rays = frame_rays, a.land.frame_left = frame_left;
    a.land.n_frames = (uint32_t)n_frames, a.land.block_layout = (uint32_t)block_layout;
    a.land.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
    a.land.error = c->host_word_dev ? (uint32_t *)(c->host_word_dev + 1) : nullptr;
    // every wave's list of tiles: a row as long as the launch has tiles (the cursors only move forward: a wave meets a tile at
    // most once; with uneven residency — twenty frames in flight, a frame's first workgroups do most of its work — a
    // shorter list overflowed at 250 spp)
    const size_t tiles_all = (size_t)c->n_local_tiles * n_frames;
    const size_t bytes = (size_t)blocks * (R1_BLOCK / 64) * tiles_all * 4;
    if (bytes > ((size_t)2 << 30))
    {
        r1_set_error("frames in flight: %zu tiles x %lld waves need %zu MB of tile lists; render this frame synchronously or in shards", tiles_all,
                     (long long)blocks * (R1_BLOCK / 64), bytes >> 20);
        return R1_ELIMIT;
    }
    int rc = ensure(c->land_spill, bytes);
    if (rc)
        return rc;
    a.land.owed_spill = (uint32_t *)c->land_spill.p;
    a.land.spill_stride = (uint32_t)tiles_all;
    a.num_rays = nullptr;
    return R1_OK;
}

// The frame's three events: the context's own, or the next slot of the timing ring (r1_timing_begin)
static void take_events(r1_context *c, hipEvent_t e[3])
{
    e[0] = c->ev0, e[1] = c->ev1, e[2] = c->ev2;
    if (c->ring_on && c->ring_frames > 0)
    {
        const int slot = c->ring_used < c->ring_frames ? c->ring_used : c->ring_frames - 1;
        e[0] = c->ring[3 * slot], e[1] = c->ring[3 * slot + 1], e[2] = c->ring[3 * slot + 2];
        if (c->ring_used < c->ring_frames)
            ++c->ring_used;
    }
}

// What the trace launch finds in memory: the attenuation stack's global workspace, a clean counter block (the last frame's closing launch
// left it so, or a memset does), the diagnostic builds' wave log, and a zero in the caller's count word where the kernel counts into it.
static int prepare_memory(r1_context *c, const Choice &k, long long blocks, int per_cu, void *d_rays, hipStream_t st, R1TraceArgs &a)
{
    int rc;
    // (the small-scene tree kernels keep the first 3 * R1_STACK_LDS_WORDS stack entries in LDS and use the workspace beyond)
    if (k.b.big || (R1_STACK_LDS_WORDS < R1_STACK_WORDS && (r1_is_tree(k.variant) || r1_is_grid(k.variant))))
    {
        // sized for the largest grid of this kernel (not this frame's): a frame with a bigger grid must not reallocate
        // (sized for the build that keeps the fewest words in LDS: the latency / diagnostic builds keep R1_STACK_LDS_WORDS, the throughput builds R1_STACK_LDS_WORDS_TP)
        const size_t entries = k.b.big ? R1_STACK_ENTRIES : R1_STACK_ENTRIES - 3 * (R1_STACK_LDS_WORDS < R1_STACK_LDS_WORDS_TP ? R1_STACK_LDS_WORDS : R1_STACK_LDS_WORDS_TP);
        const size_t max_blocks = std::max((size_t)blocks, (size_t)c->cus * (size_t)per_cu);
        if ((rc = ensure(c->gstack, entries * max_blocks * R1_BLOCK * 4)))
            return rc;
        a.gstack = (uint32_t *)c->gstack.p;
    }
    if (!k.land && !c->counters_clean)
        R1_HIP(hipMemsetAsync(c->counters.p, 0, R1_COUNTER_BYTES, st));
    c->counters_clean = false;
    if (r1_is_stats(k.variant))
    {
        c->wave_log_waves = (uint32_t)blocks * (R1_BLOCK / 64);
        if ((rc = ensure(c->wave_log, (size_t)c->wave_log_waves * 32)))
            return rc;
        R1_HIP(hipMemsetAsync(c->wave_log.p, 0, (size_t)c->wave_log_waves * 32, st));
        c->wave_log_ptr = (unsigned long long)c->wave_log.p;
        R1_HIP(hipMemcpyAsync((char *)c->counters.p + 128 + 16 * 8, &c->wave_log_ptr, 8, hipMemcpyHostToDevice, st));
    }
    if (!k.fused_clear && !k.land)
        R1_HIP(hipMemsetAsync(d_rays, 0, 8, st));
    return R1_OK;
}

// The wavefront variant's launches: path state, per-level queues and the attenuation stack live in HBM.  *blocks: the grid it ran with.
static int launch_wavefront(r1_context *c, const R1TraceArgs &a, hipStream_t st, long long *blocks)
{
    int rc;
    const size_t n = c->total_samples;
    if (n > ((size_t)1 << 24))
    {
        r1_set_error("R1_VARIANT_WAVEFRONT keeps every path of the frame in memory: %zu sample slots > 2^24", n);
        return R1_ELIMIT;
    }
    if ((rc = ensure(c->wf_paths, 3 * n * 16)) || (rc = ensure(c->wf_hits, n * 8)) || (rc = ensure(c->wf_queue, 2 * n * 4)) ||
        (rc = ensure(c->wf_counts, (R1_STACK_ENTRIES + 2) * 4)) || (rc = ensure(c->gstack, (size_t)R1_STACK_ENTRIES * n * 4)))
        return rc;
    R1WaveArgs w;
    memset(&w, 0, sizeof(w));
    w.t = a;
    w.t.gstack = (uint32_t *)c->gstack.p;
    w.paths = (float4 *)c->wf_paths.p, w.hits = (float2 *)c->wf_hits.p, w.counts = (uint32_t *)c->wf_counts.p;
    w.queue[0] = (uint32_t *)c->wf_queue.p, w.queue[1] = (uint32_t *)c->wf_queue.p + n;
    w.n_paths = (uint32_t)n;
    *blocks = std::min((long long)((n + R1_BLOCK - 1) / R1_BLOCK), (long long)c->cus * 8);
    R1_HIP(hipMemsetAsync(c->wf_counts.p, 0, (R1_STACK_ENTRIES + 2) * 4, st));
    R1_HIP(r1_launch_wavefront(&w, (int)*blocks, st));
    return R1_OK;
}

// The frame's closing launch: the accumulation and test of a listed pass, the accumulation of a pass, nothing (a landing launch resolved its
// tiles itself; PIXEL mode wrote pixels), the resolve launch, or — a batch's shard without tiles — its frames' zero counts.
// fused_clear: that launch publishes the ray count and zeroes the counter block for the next frame, which saves the two memset launches
// in front of every frame (they cost nothing to execute and ~10 us each to dispatch: a rank of an 8-GPU run renders its share of a frame
// in 140 us).
static int close_frame(r1_context *c, const r1_params *p, const Choice &k, const Batch *batch, const Pass *pass, int tiles_x, void *d_out, int block_layout,
                       void *d_rays, bool throughput_mode, hipStream_t st)
{
    const unsigned long long *rays_src = k.fused_clear ? (const unsigned long long *)((char *)c->counters.p + 32) : nullptr;
    unsigned long long *rays_dst = k.fused_clear ? (unsigned long long *)d_rays : nullptr;
    uint32_t *reset = k.fused_clear ? (uint32_t *)c->counters.p : nullptr;
    static const int resolve_rows = (int)r1_knob("R1_RESOLVE_ROWS", R1_RESOLVE_ROWS_TP); // tuning experiments
    if (k.b.mode == R1_MODE_LISTED && c->n_local_tiles)
    {
        // adaptive sampling: the records go into the listed tiles' two accumulators, their `all` bytes into d_out, and every listed tile is tested
        const int32_t n = pass->first_sample + p->spp;
        R1AdaptArgs ad;
        memset(&ad, 0, sizeof(ad));
        ad.samples = (const float4 *)c->samples.p, ad.list = pass->list;
        ad.all = (float4 *)c->accum.p, ad.even = (float4 *)c->accum_even.p;
        ad.out = (uint8_t *)d_out, ad.report = (R1TileReport *)c->adapt_report.p;
        ad.width = p->width, ad.height = p->height, ad.spp = p->spp;
        ad.tile_w = p->tile_w, ad.tile_h = p->tile_h, ad.tiles_x = tiles_x;
        ad.n_listed = pass->n_listed, ad.first_sample = (uint32_t)pass->first_sample;
        ad.inv_all = (float)(1.0f / n), ad.inv_even = (float)(1.0f / ((n + 1) / 2)); // rayweek1.cpp:765 at the samples each accumulator holds
        ad.max_delta = pass->rule->max_delta, ad.mean_delta_q8 = (uint32_t)pass->rule->mean_delta_q8;
        ad.rays_src = rays_src, ad.rays_dst = rays_dst, ad.reset = reset;
        R1_HIP(r1_launch_adapt_accum(&ad, st));
    }
    else if (pass && c->n_local_tiles)
    {
        // progressive pass: the records go into the accumulator, and the preview of samples [0, first_sample + spp) into d_out
        R1AccumArgs ac;
        memset(&ac, 0, sizeof(ac));
        ac.samples = (const float4 *)c->samples.p, ac.accum = (float4 *)c->accum.p;
        ac.out = pass->image ? (uint8_t *)d_out : nullptr;
        ac.full = c->full, ac.n_local_tiles = c->n_local_tiles;
        ac.width = p->width, ac.height = p->height, ac.spp = p->spp;
        ac.tile_w = p->tile_w, ac.tile_h = p->tile_h, ac.tiles_x = tiles_x;
        ac.fresh = pass->first_sample == 0 ? 1u : 0u;
        ac.inv_n = (float)(1.0f / (pass->first_sample + p->spp)); // rayweek1.cpp:765 at the accumulated spp
        ac.rays_src = rays_src, ac.rays_dst = rays_dst, ac.reset = reset;
        R1_HIP(r1_launch_accum(&ac, st));
    }
    else if (k.land)
        ; // the trace launch resolved its tiles itself
    else if (c->n_local_tiles && k.b.mode != R1_MODE_PIXEL)
    {
        R1ResolveArgs r;
        memset(&r, 0, sizeof(r));
        r.samples = (const float4 *)c->samples.p;
        r.full = c->full, r.n_local_tiles = c->n_local_tiles;
        r.width = p->width, r.height = p->height, r.spp = p->spp;
        r.tile_w = p->tile_w, r.tile_h = p->tile_h, r.tiles_x = tiles_x;
        r.shard = p->shard, r.num_shards = p->num_shards;
        r.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
        r.out = (uint8_t *)d_out, r.block_layout = block_layout;
        r.n_frames = (uint32_t)(batch ? batch->n_frames : 1);
        if (batch)
        {
            r.out_stride = batch->out_stride, r.rays_offset = batch->rays_offset;
            r.frame_rays = (unsigned long long *)c->batch_rays.p;
        }
        r.rays_src = rays_src, r.rays_dst = rays_dst, r.reset = reset;
        R1_HIP(r1_launch_resolve(&r, throughput_mode ? resolve_rows : 0, st));
    }
    else if (batch) // a shard without tiles: its frames' counts are zero
        for (int f = 0; f < batch->n_frames; ++f)
            R1_HIP(hipMemsetAsync((char *)d_out + (size_t)f * batch->out_stride + batch->rays_offset, 0, 8, st));
    return R1_OK;
}

// Enqueues the frame (trace + resolve) on `st`.  d_out / d_rays are device addresses; d_rays == NULL stands for the context's own
// count word (counters + R1_COUNTER_BYTES; the allocation may move in here, so callers take that address afterwards).
static int enqueue_frame(r1_context *c, const r1_params *p, void *d_out, int block_layout, void *d_rays, hipStream_t st,
                         bool throughput_mode, const Batch *batch, Landing *landing, const Pass *pass)
{
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    const int variant = resolve_variant(c, p->variant, throughput_mode);
    if (c->moved && variant != R1_V_REFERENCE && !r1_is_tree(variant))
    {
        r1_set_error("variant %d: the scene has moved (r1_update_centers) and only the box tree was refitted, not the sphere groups and the uniform grid; "
                     "r1_set_scene rebuilds them", variant);
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    if (r1_is_grid(variant) && (rc = ensure_grid(c)))
        return rc;
    if ((rc = size_tiles(c, p, batch ? batch->n_frames : 1, pass)))
        return rc;
    if (!d_rays) // (only now: the counter allocation may have moved)
        d_rays = (char *)c->counters.p + R1_COUNTER_BYTES;
    Choice k;
    if ((rc = choose_kernel(c, p, variant, throughput_mode, batch, pass, k)) || (rc = ensure_records(c, p, k, batch, st)))
        return rc;

    R1TraceArgs a;
    frame_args(c, p, k, batch, d_out, block_layout, d_rays, a);
    if ((rc = put_batch_block(c, k, batch, pass, st, a)))
        return rc;
    int per_cu = 1, land_parity = 0;
    if ((rc = blocks_per_cu(c, k, a, &per_cu)))
        return rc;
    const bool pixel_mode = k.b.mode == R1_MODE_PIXEL;
    const GridSize g = size_grid(c->cus, per_cu, c->total_samples, pixel_mode ? a.total_samples : 0u, pixel_mode, r1_runs_as_latency(k.b.mode, k.b.big), throughput_mode, p->num_shards);
    a.chunk_min = g.chunk_min, a.chunk_max = g.chunk_max, a.nq = g.nq;
    long long blocks = g.blocks;
    if (k.land && (rc = land_setup(c, p, batch, landing, blocks, block_layout, st, a, d_out, d_rays, land_parity)))
        return rc;
    hipEvent_t e[3];
    take_events(c, e);
    if ((rc = prepare_memory(c, k, blocks, per_cu, d_rays, st, a)))
        return rc;

    R1_HIP(hipEventRecord(e[0], st));
    if (c->total_samples && variant != R1_V_WAVEFRONT)
        R1_HIP(r1_launch_trace(&a, k.b, (int)blocks, r1_is_grid(variant) && !k.b.big ? c->grid_args.lds_bytes : 0u, st));
    if (c->total_samples && variant == R1_V_WAVEFRONT && (rc = launch_wavefront(c, a, st, &blocks)))
        return rc;
    R1_HIP(hipEventRecord(e[1], st));
    if ((rc = close_frame(c, p, k, batch, pass, a.tiles_x, d_out, block_layout, d_rays, throughput_mode, st)))
        return rc;
    c->counters_clean = k.fused_clear;
    c->land_prev = k.land;
    if (k.land)
        c->land_parity = land_parity, c->land_armed = true;
    R1_HIP(hipEventRecord(e[2], st));
    c->last0 = e[0], c->last1 = e[1], c->last2 = e[2];
    c->timing_valid = true;

    c->info.blocks = (int32_t)blocks, c->info.threads_per_block = R1_BLOCK, c->info.samples = c->total_samples;
    c->info.tiles_in_kernel = k.land ? 1 : 0;
    c->info.kernel = variant; // internal numbering = the public enum (DEFAULT resolved)
    c->info.spheres_active = (int32_t)c->n_active, c->info.spheres_padded = (int32_t)c->n_padded_scene, c->info.groups = (int32_t)c->n_groups;
    c->info.bvh_nodes = (int32_t)c->n_bvh_nodes, c->info.bvh_leaves = (int32_t)c->n_bvh_leaves, c->info.bvh_depth = c->bvh_depth;
    return R1_OK;
}

// ---- public render entry points ---------------------------------------------------------------------

// a resolver of an earlier launch gave up waiting (R1_LAND_MAX_WAIT): the frames of that launch are not valid
static int land_check(r1_context *c)
{
    if (c->host_word && ((volatile uint32_t *)c->host_word)[2])
    {
        ((volatile uint32_t *)c->host_word)[2] = 0;
        r1_set_error("a launch did not resolve all of its tiles (a resolver workgroup gave up waiting): its frames are not valid");
        return R1_EHIP;
    }
    return R1_OK;
}

static int render_host(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, double *device_seconds_out,
                       float *samples_out)
{
    if (!c || !p || !rgb_out)
    {
        r1_set_error("r1_render: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (samples_out && p->num_shards != 1)
    {
        r1_set_error("r1_render_samples needs num_shards == 1");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const bool sharded = p->num_shards > 1;
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    const size_t out_bytes = sharded ? r1_shard_block_bytes(p) : img_bytes;
    if ((rc = ensure(c->image, out_bytes + 64)))
        return rc;
    // the ray count: stored by the frame's last launch straight into the context's page-locked word (no second copy to
    // enqueue and wait for); the diagnostic builds count with atomics and keep a device word + copy
    const bool stats = r1_is_stats(p->variant);
    const bool direct = !stats && c->host_word_dev;
    // a page-locked pixel buffer (r1_host_alloc) receives the tiles straight from the trace kernel's resolvers: no copy either
    Landing land_to;
    if (direct && !sharded)
        land_to.out = mapped_host(rgb_out), land_to.rays = c->host_word_dev;
    if ((rc = enqueue_frame(c, p, c->image.p, sharded ? 1 : 0, direct ? (void *)c->host_word_dev : nullptr, c->stream, false, nullptr, &land_to)))
        return rc;
    void *const d_rays = direct ? (void *)c->host_word_dev : (void *)((char *)c->counters.p + R1_COUNTER_BYTES); // (behind the block the frame's last launch zeroes)

    uint64_t rays = 0;
    if (!sharded)
    {
        if (!land_to.used)
            R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
        if (!direct)
            R1_HIP(hipMemcpyAsync(&rays, d_rays, 8, hipMemcpyDeviceToHost, c->stream));
        R1_HIP(hipStreamSynchronize(c->stream));
    }
    else
    {
        std::vector<uint8_t> block(out_bytes);
        R1_HIP(hipMemcpyAsync(block.data(), c->image.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
        if (!direct)
            R1_HIP(hipMemcpyAsync(&rays, d_rays, 8, hipMemcpyDeviceToHost, c->stream));
        R1_HIP(hipStreamSynchronize(c->stream));
        const int tiles_x = (p->width + p->tile_w - 1) / p->tile_w;
        for (uint32_t lt = 0; lt < c->n_local_tiles; ++lt)
        {
            const int t = p->shard + (int)lt * p->num_shards;
            const int x0 = (t % tiles_x) * p->tile_w, y0 = (t / tiles_x) * p->tile_h;
            const int tw = p->tile_w < p->width - x0 ? p->tile_w : p->width - x0;
            const int th = p->tile_h < p->height - y0 ? p->tile_h : p->height - y0;
            for (int ly = 0; ly < th; ++ly)
                memcpy(rgb_out + ((size_t)(y0 + ly) * p->width + x0) * 3,
                       block.data() + ((size_t)lt * p->tile_h * p->tile_w + (size_t)ly * p->tile_w) * 3, (size_t)tw * 3);
        }
    }
    if ((rc = land_check(c)))
        return rc;
    if (direct)
        rays = *(volatile unsigned long long *)c->host_word;
    if (num_rays_out)
        *num_rays_out = rays;
    if (device_seconds_out)
    {
        float ms = 0;
        R1_HIP(hipEventElapsedTime(&ms, c->last0, c->last2)); // the events THIS frame recorded (a ring slot while r1_timing_begin is on)
        *device_seconds_out = ms * 1e-3;
    }
    if (samples_out)
    {
        // device order is [padded tile][sample][pixel in tile]; the ABI order is
        // ((y*width + x)*spp + s)
        std::vector<float> tmp((size_t)c->total_samples * 4);
        R1_HIP(hipMemcpyAsync(tmp.data(), c->samples.p, tmp.size() * 4, hipMemcpyDeviceToHost, c->stream));
        R1_HIP(hipStreamSynchronize(c->stream));
        const int tiles_x = (p->width + p->tile_w - 1) / p->tile_w;
        for (uint32_t lt = 0; lt < c->n_local_tiles; ++lt)
        {
            const int x0 = ((int)lt % tiles_x) * p->tile_w, y0 = ((int)lt / tiles_x) * p->tile_h;
            const int tw = p->tile_w < p->width - x0 ? p->tile_w : p->width - x0;
            const int th = p->tile_h < p->height - y0 ? p->tile_h : p->height - y0;
            const float *src = tmp.data() + (size_t)lt * c->full * 4;
            const size_t tile_px = (size_t)p->tile_w * p->tile_h;
            for (int ly = 0; ly < th; ++ly)
                for (int lx = 0; lx < tw; ++lx)
                    for (int sm = 0; sm < p->spp; ++sm)
                    {
                        float *dst = samples_out + (((size_t)(y0 + ly) * p->width + (x0 + lx)) * p->spp + sm) * 4;
                        memcpy(dst, src + ((size_t)sm * tile_px + (size_t)(ly * p->tile_w + lx)) * 4, 16);
                        if (c->land_prev) // the launch tagged its records' ray-count words (R1_LAND): the ABI's word is the count alone
                        {
                            uint32_t wv;
                            memcpy(&wv, dst + 3, 4);
                            wv &= 255u;
                            memcpy(dst + 3, &wv, 4);
                        }
                    }
        }
    }
    return R1_OK;
}

extern "C" int r1_render(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    return render_host(c, p, rgb_out, num_rays_out, device_seconds_out, nullptr);
}

extern "C" int r1_render_samples(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, float *samples_out)
{
    if (!samples_out)
    {
        r1_set_error("r1_render_samples: null samples_out");
        return R1_EINVAL;
    }
    return render_host(c, p, rgb_out, num_rays_out, nullptr, samples_out);
}

// Progressive rendering: samples [first_sample, first_sample + spp) of every pixel, added in sample order to the context's fp32 accumulator.  The
// accumulator then holds exactly the sums the resolve of a frame of first_sample + spp samples computes (a sample's streams depend on (seed,
// pixel, sample index) only, include/rays1_seed.h), so every preview is that frame's image, bit for bit.
static bool same_pass_frame(const r1_params &a, const r1_params &b) // every field but spp
{
    return a.width == b.width && a.height == b.height && a.max_bounces == b.max_bounces && a.seed == b.seed && a.tile_w == b.tile_w &&
           a.tile_h == b.tile_h && a.shard == b.shard && a.num_shards == b.num_shards && a.variant == b.variant;
}

extern "C" int r1_render_pass(r1_context *c, const r1_params *p, int32_t first_sample, uint8_t *rgb_out, uint64_t *num_rays_out)
{
    if (!c || !p)
    {
        r1_set_error("r1_render_pass: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_pass renders whole frames (num_shards == 1)");
        return R1_EINVAL;
    }
    if (r1_is_stats(p->variant) || p->variant == R1_VARIANT_WAVEFRONT)
    {
        r1_set_error("r1_render_pass: variant %d (a diagnostic build or the wavefront variant) has no progressive-pass build", p->variant);
        return R1_EINVAL;
    }
    if (first_sample < 0 || (int64_t)first_sample + p->spp > (int64_t)INT32_MAX)
    {
        r1_set_error("r1_render_pass: first_sample %d + spp %d is not within [0, INT32_MAX]", first_sample, p->spp);
        return R1_EINVAL;
    }
    if (first_sample > 0 && !(c->pass_valid && c->pass_samples == first_sample && same_pass_frame(c->pass_key, *p)))
    {
        if (!c->pass_valid)
            r1_set_error("r1_render_pass: no accumulation to continue (start one with first_sample 0)");
        else if (c->pass_samples != first_sample)
            r1_set_error("r1_render_pass: first_sample %d, but %d samples are accumulated", first_sample, c->pass_samples);
        else
            r1_set_error("r1_render_pass: the parameters differ from those that started the accumulation (only spp may change)");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    int32_t tiles = 0;
    if ((rc = r1_tile_count(p, &tiles, nullptr)))
        return rc;
    if ((uint64_t)p->tile_w * p->tile_h * p->spp * (uint64_t)tiles >= ((uint64_t)1 << 31))
    {
        r1_set_error("a pass of %dx%dx%d with %dx%d tiles exceeds 2^31 sample slots per launch", p->width, p->height, p->spp, p->tile_w, p->tile_h);
        return R1_ELIMIT;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    if (rgb_out && (rc = ensure(c->image, img_bytes + 64)))
        return rc;
    // from here on a failure leaves the accumulator in an unknown state: only first_sample == 0 is accepted next
    c->pass_valid = false;
    const bool direct = c->host_word_dev != nullptr; // the pass's ray count straight into the page-locked word, as r1_render
    Pass ps;
    ps.first_sample = first_sample;
    ps.image = rgb_out != nullptr;
    if ((rc = enqueue_frame(c, p, c->image.p, 0, direct ? (void *)c->host_word_dev : nullptr, c->stream, false, nullptr, nullptr, &ps)))
        return rc;
    uint64_t rays = 0;
    if (rgb_out)
        R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
    if (!direct)
        R1_HIP(hipMemcpyAsync(&rays, (char *)c->counters.p + R1_COUNTER_BYTES, 8, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    if (direct)
        rays = *(volatile unsigned long long *)c->host_word;
    c->pass_rays = (first_sample == 0 ? 0u : c->pass_rays) + rays;
    c->pass_samples = first_sample + p->spp;
    c->pass_key = *p;
    c->pass_valid = true;
    if (num_rays_out)
        *num_rays_out = c->pass_rays;
    return R1_OK;
}

// ---- adaptive sampling --------------------------------------------------------------
static bool adaptive_variant(int v) { return v == R1_VARIANT_DEFAULT || v == R1_VARIANT_PREFILTER || v == R1_VARIANT_BVH || v == R1_VARIANT_GRID; }

// The one place the options of r1_render_adaptive are validated: the cumulative sample counts after every pass.
extern "C" int r1_adaptive_schedule(const r1_params *p, const r1_adaptive *o, int32_t *n_out, size_t cap, size_t *count)
{
    if (!p || !o || (!n_out && !count))
    {
        r1_set_error("r1_adaptive_schedule: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("adaptive sampling renders whole frames (num_shards == 1, not %d)", p->num_shards);
        return R1_EINVAL;
    }
    if (!adaptive_variant(p->variant))
    {
        r1_set_error("adaptive sampling: variant %d (the reference form, a diagnostic build or the wavefront variant) has no listed-tile build", p->variant);
        return R1_EINVAL;
    }
    if (o->min_spp < 1)
    {
        r1_set_error("adaptive sampling: min_spp %d is not >= 1", o->min_spp);
        return R1_EINVAL;
    }
    if (o->pass_spp < 1)
    {
        r1_set_error("adaptive sampling: pass_spp %d is not >= 1", o->pass_spp);
        return R1_EINVAL;
    }
    if (o->max_delta < -1 || o->max_delta > 255)
    {
        r1_set_error("adaptive sampling: max_delta %d is not within [-1, 255]", o->max_delta);
        return R1_EINVAL;
    }
    if (o->mean_delta_q8 < 0 || o->mean_delta_q8 > 65280)
    {
        r1_set_error("adaptive sampling: mean_delta_q8 %d is not within [0, 65280]", o->mean_delta_q8);
        return R1_EINVAL;
    }
    int32_t tiles = 0;
    if ((rc = r1_tile_count(p, &tiles, nullptr)))
        return rc;
    const int32_t n0 = o->min_spp < p->spp ? o->min_spp : p->spp;
    const int32_t longest = std::max(n0, std::min(o->pass_spp, p->spp - n0)); // samples of the longest pass
    if ((uint64_t)p->tile_w * p->tile_h * (uint64_t)longest * (uint64_t)tiles >= ((uint64_t)1 << 31))
    {
        r1_set_error("a pass of %dx%dx%d with %dx%d tiles exceeds 2^31 sample slots per launch", p->width, p->height, longest, p->tile_w, p->tile_h);
        return R1_ELIMIT;
    }
    if ((uint64_t)p->tile_w * p->tile_h > ((uint64_t)1 << 22))
    {
        r1_set_error("adaptive sampling: tiles of %dx%d pixels exceed 2^22 (a tile's err_sum is a 32-bit sum of byte differences)", p->tile_w, p->tile_h);
        return R1_ELIMIT;
    }
    const size_t n_pass = 1 + ((size_t)(p->spp - n0) + (size_t)o->pass_spp - 1) / (size_t)o->pass_spp;
    if (count)
        *count = n_pass;
    if (!n_out)
        return R1_OK;
    if (cap < n_pass)
    {
        r1_set_error("r1_adaptive_schedule: cap %zu, the schedule has %zu passes", cap, n_pass);
        return R1_EINVAL;
    }
    int64_t n = n0;
    for (size_t k = 0; k < n_pass; ++k, n += o->pass_spp)
        n_out[k] = (int32_t)std::min<int64_t>(n, p->spp);
    return R1_OK;
}

static_assert(sizeof(r1_tile_report) == sizeof(R1TileReport) && sizeof(r1_tile_report) == 16 && sizeof(r1_adaptive_result) == 24, "public structs without padding; the device writes r1_tile_report's layout");

extern "C" int r1_render_adaptive(r1_context *c, const r1_params *p, const r1_adaptive *opt, uint8_t *rgb_out, uint64_t *num_rays_out, r1_tile_report *tiles_out,
                                  r1_adaptive_result *result_out)
{
    if (!c || !p || !opt || !rgb_out)
    {
        r1_set_error("r1_render_adaptive: null argument");
        return R1_EINVAL;
    }
    size_t n_pass = 0;
    int rc = r1_adaptive_schedule(p, opt, nullptr, 0, &n_pass);
    if (rc)
        return rc;
    std::vector<int32_t> sched(n_pass);
    if ((rc = r1_adaptive_schedule(p, opt, sched.data(), n_pass, nullptr)))
        return rc;
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    int32_t tiles = 0;
    if ((rc = r1_tile_count(p, &tiles, nullptr)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    const size_t tile_px = (size_t)p->tile_w * p->tile_h;
    if ((rc = ensure(c->image, img_bytes + 64)) || (rc = ensure(c->accum, (size_t)tiles * tile_px * 16)) || (rc = ensure(c->accum_even, (size_t)tiles * tile_px * 16)) ||
        (rc = ensure(c->adapt_list, ((size_t)2 * tiles + 1) * 4)) || (rc = ensure(c->adapt_report, (size_t)tiles * sizeof(R1TileReport))))
        return rc;
    c->pass_valid = false; // (the `all` accumulator is r1_render_pass's: an accumulation of the context ends here, as at first_sample 0)
    const bool direct = c->host_word_dev != nullptr; // ray count and list length straight into the context's page-locked words, as r1_render_pass
    uint32_t *const lists[2] = {(uint32_t *)c->adapt_list.p, (uint32_t *)c->adapt_list.p + tiles};
    uint32_t *const d_count = direct ? (uint32_t *)c->host_word_dev + 4 : (uint32_t *)c->adapt_list.p + 2 * (size_t)tiles;
    R1_HIP(r1_launch_adapt_compact(nullptr, (uint32_t)tiles, (const R1TileReport *)c->adapt_report.p, 0u, lists[0], d_count, c->stream)); // every tile, in order
    uint32_t m = (uint32_t)tiles;
    uint64_t rays_sum = 0;
    int32_t passes = 0;
    for (size_t k = 0; k < n_pass && m; ++k)
    {
        const int32_t first = k ? sched[k - 1] : 0;
        r1_params pp = *p;
        pp.spp = sched[k] - first;
        Pass ps;
        ps.first_sample = first;
        ps.list = lists[k & 1], ps.n_listed = m, ps.rule = opt;
        if ((rc = enqueue_frame(c, &pp, c->image.p, 0, direct ? (void *)c->host_word_dev : nullptr, c->stream, false, nullptr, nullptr, &ps)))
            return rc;
        R1_HIP(r1_launch_adapt_compact(lists[k & 1], m, (const R1TileReport *)c->adapt_report.p, sched[k] == p->spp ? 1u : 0u, lists[(k & 1) ^ 1], d_count, c->stream));
        uint64_t rays = 0;
        uint32_t next = 0;
        if (!direct)
        {
            R1_HIP(hipMemcpyAsync(&rays, (char *)c->counters.p + R1_COUNTER_BYTES, 8, hipMemcpyDeviceToHost, c->stream));
            R1_HIP(hipMemcpyAsync(&next, d_count, 4, hipMemcpyDeviceToHost, c->stream));
        }
        R1_HIP(hipStreamSynchronize(c->stream));
        if (direct)
            rays = *(volatile unsigned long long *)c->host_word, next = ((volatile uint32_t *)c->host_word)[4];
        rays_sum += rays; // (summed on the host, pass by pass, as r1_render_pass does)
        ++passes;
        if (next > m)
        {
            r1_set_error("r1_render_adaptive: a pass left %u active tiles of %u", next, m);
            return R1_EHIP;
        }
        m = next;
    }
    std::vector<r1_tile_report> local;
    r1_tile_report *rep = tiles_out;
    if (!rep)
    {
        local.resize((size_t)tiles);
        rep = local.data();
    }
    R1_HIP(hipMemcpyAsync(rep, c->adapt_report.p, (size_t)tiles * sizeof(R1TileReport), hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    if (num_rays_out)
        *num_rays_out = rays_sum;
    if (result_out)
    {
        const int tiles_x = (p->width + p->tile_w - 1) / p->tile_w;
        uint64_t samples = 0;
        int32_t settled = 0;
        for (int32_t t = 0; t < tiles; ++t)
        {
            const int x0 = (t % tiles_x) * p->tile_w, y0 = (t / tiles_x) * p->tile_h;
            const int tw = p->tile_w < p->width - x0 ? p->tile_w : p->width - x0;
            const int th = p->tile_h < p->height - y0 ? p->tile_h : p->height - y0;
            samples += (uint64_t)rep[t].spp * (uint64_t)(tw * th);
            settled += rep[t].settled ? 1 : 0;
        }
        result_out->samples = samples;
        result_out->passes = passes, result_out->tiles = tiles, result_out->tiles_settled = settled, result_out->reserved = 0;
    }
    return R1_OK;
}

// Pipelined form of r1_render (frames in flight, results on the HOST): the frame is enqueued with the throughput
// kernels on `hip_stream` (or the context's stream), followed by the copies of the row-major image and of the ray
// count into the caller's buffers.  Nothing is waited for: the buffers are valid once the stream is idle (r1_sync for
// the context's stream).  One frame per context at a time — a caller keeps K frames in flight with K contexts, as
// bench.py does.  Page-locked buffers (r1_host_alloc) let the copies overlap the other frames' kernels; pageable
// memory works but makes each copy wait for its frame.
extern "C" int r1_render_async(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, void *hip_stream)
{
    if (!c || !p || ((rgb_out == nullptr) != (num_rays_out == nullptr)))
    {
        r1_set_error("r1_render_async: null argument (rgb_out and num_rays_out are given together, or both NULL)");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_async renders whole frames (num_shards == 1); shards go through r1_render_shard_device");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    if ((rc = ensure(c->image, img_bytes + 64)))
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // page-locked buffers (r1_host_alloc) receive the tiles and the count straight from the trace kernel's resolvers: nothing to copy
    Landing land_to;
    if (rgb_out && ((uintptr_t)num_rays_out & 7u) == 0)
        land_to.out = mapped_host(rgb_out), land_to.rays = mapped_host(num_rays_out);
    if ((rc = enqueue_frame(c, p, c->image.p, 0, nullptr, st, true, nullptr, &land_to)))
        return rc;
    if (rgb_out && !land_to.used) // (both NULL: the frame stays in the context's device buffers — a measurement aid, bench.py's value_device_resident)
    {
        R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, st));
        R1_HIP(hipMemcpyAsync(num_rays_out, (char *)c->counters.p + R1_COUNTER_BYTES, 8, hipMemcpyDeviceToHost, st));
    }
    return R1_OK;
}

// n_frames frames of the same scene, camera and size in ONE launch (frame f seeded params->seed + f * seed_stride): the
// persistent waves flow from one frame into the next, so the ramp and drain of a launch are paid once per batch.
// Whole frames (num_shards == 1): host_frames receives n_frames frame records (r1_frame_record_bytes each) with ONE copy.
extern "C" int r1_render_batch_async(r1_context *c, const r1_params *p, int32_t n_frames, uint32_t seed_stride, void *host_frames, void *hip_stream)
{
    if (!c || !p || n_frames < 1)
    {
        r1_set_error("r1_render_batch_async: bad argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_batch_async renders whole frames (num_shards == 1); shards go through r1_render_shard_device_batch");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t frame = r1_frame_record_bytes(p);
    if ((rc = ensure(c->image, frame * (size_t)n_frames)))
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    Batch b;
    b.n_frames = n_frames, b.seed_stride = seed_stride, b.out_stride = frame, b.rays_offset = frame - 8;
    Landing land_to;
    if (host_frames && ((uintptr_t)host_frames & 7u) == 0)
        land_to.out = mapped_host(host_frames);
    if ((rc = enqueue_frame(c, p, c->image.p, 0, nullptr, st, true, &b, &land_to)))
        return rc;
    if (host_frames && !land_to.used) // (NULL: the frames stay in the context's device buffer — a measurement aid)
        R1_HIP(hipMemcpyAsync(host_frames, c->image.p, frame * (size_t)n_frames, hipMemcpyDeviceToHost, st));
    return R1_OK;
}

// A camera path: r1_render_batch_async with cameras[f] in place of the context's camera for frame f (the R1_MODE_PATH kernels; one frame: the
// single-frame kernel with cameras[0] by value).  The context's own camera is not touched.
extern "C" int r1_render_path_async(r1_context *c, const r1_params *p, int32_t n_frames, uint32_t seed_stride, const r1_camera *cameras, void *host_frames,
                                    void *hip_stream)
{
    if (!c || !p || !cameras || n_frames < 1)
    {
        r1_set_error("r1_render_path_async: bad argument (%s)", !c ? "ctx is NULL" : !p ? "params is NULL" : !cameras ? "cameras is NULL" : "n_frames < 1");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_path_async renders whole frames (num_shards == 1)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t frame = r1_frame_record_bytes(p);
    if ((rc = ensure(c->image, frame * (size_t)n_frames)))
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    Batch b;
    b.n_frames = n_frames, b.seed_stride = seed_stride, b.out_stride = frame, b.rays_offset = frame - 8;
    b.cameras = cameras;
    Landing land_to;
    if (host_frames && ((uintptr_t)host_frames & 7u) == 0)
        land_to.out = mapped_host(host_frames);
    if ((rc = enqueue_frame(c, p, c->image.p, 0, nullptr, st, true, &b, &land_to)))
        return rc;
    if (host_frames && !land_to.used) // (NULL: the frames stay in the context's device buffer — a measurement aid)
        R1_HIP(hipMemcpyAsync(host_frames, c->image.p, frame * (size_t)n_frames, hipMemcpyDeviceToHost, st));
    return R1_OK;
}

// The same for one shard of n_frames frames: d_records receives n_frames records (r1_shard_record_bytes each: dense tile
// block + uint64 ray count), device memory — what a rank hands to ONE all-gather per batch.
extern "C" int r1_render_shard_device_batch(r1_context *c, const r1_params *p, int32_t n_frames, uint32_t seed_stride, void *d_records, void *hip_stream)
{
    if (!c || !p || !d_records || n_frames < 1 || ((uintptr_t)d_records & 7u))
    {
        r1_set_error("r1_render_shard_device_batch: bad argument (d_records must be 8-byte aligned)");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const size_t record = r1_shard_record_bytes(p);
    Batch b;
    b.n_frames = n_frames, b.seed_stride = seed_stride, b.out_stride = record, b.rays_offset = record - 8;
    return enqueue_frame(c, p, d_records, 1, nullptr, st, true, &b);
}

// ---- ray queries (include/rays1.h "ray queries", r1_cast.hip) ------------------------------------------------------------

static_assert(sizeof(r1_ray) == 32 && sizeof(r1_hit) == 32, "the cast kernels read and write these layouts as two float4");

// the checks every cast entry point makes before it touches anything; *structure: what the rays walk — R1_V_TREE, R1_V_GRID or R1_V_REFERENCE
static int cast_check(const char *who, r1_context *c, int32_t variant, int32_t mode, int *structure)
{
    if (!c)
    {
        r1_set_error("%s: ctx is NULL", who);
        return R1_EINVAL;
    }
    if (mode != R1_CAST_CLOSEST && mode != R1_CAST_ANY)
    {
        r1_set_error("%s: mode %d is neither R1_CAST_CLOSEST nor R1_CAST_ANY", who, mode);
        return R1_EINVAL;
    }
    switch (variant)
    {
    case R1_VARIANT_DEFAULT:
    case R1_VARIANT_BVH: *structure = R1_V_TREE; break;
    case R1_VARIANT_GRID: *structure = R1_V_GRID; break;
    case R1_VARIANT_REFERENCE: *structure = R1_V_REFERENCE; break;
    default:
        r1_set_error("%s: variant %d casts no rays (DEFAULT, BVH, GRID and REFERENCE do)", who, variant);
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("%s: no scene set (call r1_set_scene first)", who);
        return R1_EINVAL;
    }
    if (c->moved && *structure == R1_V_GRID)
    {
        r1_set_error("%s: the scene has moved (r1_update_centers) and the uniform grid was not refitted; r1_set_scene rebuilds it", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

// Enqueues the cast of n rays (device memory) on `st`; waits for nothing (the first grid cast after r1_set_scene builds the grid, as the
// first grid render does).  Touches none of the state a render reads: no counter block, no sample records, no launch info, no events.
static int cast_enqueue(r1_context *c, int structure, int32_t mode, const void *d_rays, size_t n, void *d_out, hipStream_t st)
{
    int rc;
    R1_HIP(hipSetDevice(c->device));
    if (c->n_active == 0)
        structure = R1_V_REFERENCE; // (no sphere can be hit: the reference form's loop of zero trips writes the misses; there is no tree to stage)
    if (structure == R1_V_GRID && (rc = ensure_grid(c)))
        return rc;
    const bool big = big_scene(c, structure == R1_V_TREE, structure == R1_V_GRID, false);
    static const int plain_env = (int)r1_knob("R1_CAST_PLAIN", 0); // tuning library only: the plain form of the tree cast (r1_cast.hip), for measuring
    const int plain = structure == R1_V_TREE && plain_env ? 1 : 0;

    R1CastArgs a;
    memset(&a, 0, sizeof(a));
    fill_scene(c, a.t.scene); // (the sweep's tables ride along: the cast kernels read none of them)
    // (the grid's fallback and the plain form walk the tree from its root, read from global memory: no root step)
    if (structure == R1_V_GRID || plain)
        a.t.scene.bvh_root_leaf = 0u;
    fill_walk(c, structure == R1_V_TREE && !plain, big, R1_BVH_TOP_NODES, a.t);
    if (structure == R1_V_GRID)
        a.t.grid = (const R1GridArgs *)(big ? c->grid_dev32.p : c->grid_dev.p);
    a.active_to_scene = (const uint32_t *)c->active_dev.p;
    a.mode = (uint32_t)mode;
    // (the plain form: a 32-bit traversal stack and no node table)
    const size_t dyn_lds = plain ? (size_t)a.t.bvh_depth * R1_BLOCK * 4 : r1_walk_lds(structure, big, a.t.bvh_depth, a.t.bvh_lds_f4, c->grid_args.lds_bytes);
    int &occ = c->cast_occupancy[(structure == R1_V_TREE ? 0 : structure == R1_V_GRID ? 2 : 4) + (big ? 1 : 0)];
    if (occ == 0)
        R1_HIP(r1_cast_occupancy(structure, big ? 1 : 0, plain, dyn_lds, &occ));
    const int per_cu = occ < 1 ? 1 : (occ > 8 ? 8 : occ);
    if ((rc = ensure(c->cast_cursors, (size_t)R1_CAST_CURSORS * 128)))
        return rc;
    for (size_t at = 0; at < n; at += R1_CAST_LAUNCH_MAX)
    {
        const uint32_t m = (uint32_t)std::min<size_t>(n - at, R1_CAST_LAUNCH_MAX);
        a.rays = (const float4 *)((const char *)d_rays + at * sizeof(r1_ray));
        a.out = (char *)d_out + at * (mode == R1_CAST_ANY ? 1 : sizeof(r1_hit));
        a.n = m;
        // persistent: as many workgroups as the chip holds, fewer where the rays run out; a wave claims 64 .. 256 rays at a time,
        // about an eighth of its share (the waves that finish first take the rest)
        const uint32_t blocks = (uint32_t)std::min<size_t>((size_t)c->cus * per_cu, ((size_t)m + R1_BLOCK - 1) / R1_BLOCK);
        const uint32_t share = m / (blocks * (R1_BLOCK / 64) * 8u);
        a.claim = std::min(256u, std::max(64u, (share + 63u) & ~63u));
        a.cursor = (uint32_t *)((char *)c->cast_cursors.p + 128 * (c->cast_cursor_next++ % R1_CAST_CURSORS));
        R1_HIP(hipMemsetAsync(a.cursor, 0, 4, st));
        R1_HIP(r1_launch_cast(&a, structure, big ? 1 : 0, plain, (int)blocks, dyn_lds, st));
    }
    return R1_OK;
}

extern "C" int r1_cast_rays_device(r1_context *c, int32_t variant, int32_t mode, const void *d_rays, size_t n, void *d_out, void *hip_stream)
{
    int structure = 0;
    int rc = cast_check("r1_cast_rays_device", c, variant, mode, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!d_rays || !d_out || ((uintptr_t)d_rays & 15u) || ((uintptr_t)d_out & 15u))
    {
        r1_set_error("r1_cast_rays_device: d_rays and d_out must be non-NULL device memory, 16-byte aligned");
        return R1_EINVAL;
    }
    return cast_enqueue(c, structure, mode, d_rays, n, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_cast_rays(r1_context *c, int32_t variant, int32_t mode, const r1_ray *rays, size_t n, void *out)
{
    int structure = 0;
    int rc = cast_check("r1_cast_rays", c, variant, mode, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!rays || !out)
    {
        r1_set_error("r1_cast_rays: rays and out must not be NULL with n > 0");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    // one chunk's rays, then its results (32 bytes per ray each): device memory stays bounded for any n
    const size_t chunk = std::min<size_t>(n, R1_CAST_CHUNK);
    if ((rc = ensure(c->cast_ws, chunk * 64)))
        return rc;
    char *const d_rays = (char *)c->cast_ws.p, *const d_out = d_rays + chunk * 32;
    const size_t out_each = mode == R1_CAST_ANY ? 1 : sizeof(r1_hit);
    for (size_t at = 0; at < n; at += chunk)
    {
        const size_t m = std::min(chunk, n - at);
        R1_HIP(hipMemcpyAsync(d_rays, rays + at, m * sizeof(r1_ray), hipMemcpyHostToDevice, c->stream));
        if ((rc = cast_enqueue(c, structure, mode, d_rays, m, d_out, c->stream)))
            return rc;
        R1_HIP(hipMemcpyAsync((char *)out + at * out_each, d_out, m * out_each, hipMemcpyDeviceToHost, c->stream));
        R1_HIP(hipStreamSynchronize(c->stream)); // (the next chunk reuses the workspace)
    }
    return R1_OK;
}

extern "C" int r1_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0)
        return R1_EINVAL;
    *out = nullptr;
    if (r1_device_count() <= 0)
        return R1_ENODEVICE;
    R1_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return R1_OK;
}

extern "C" void r1_host_free(void *p)
{
    if (p)
        (void)hipHostFree(p);
}

extern "C" int r1_render_shard_device(r1_context *c, const r1_params *p, void *d_block, void *d_num_rays, void *hip_stream)
{
    if (!c || !p || !d_block || !d_num_rays)
    {
        r1_set_error("r1_render_shard_device: null argument");
        return R1_EINVAL;
    }
    if ((uintptr_t)d_num_rays & 7u)
    {
        r1_set_error("r1_render_shard_device: d_num_rays must be 8-byte aligned (a uint64 the kernels store and add to atomically)");
        return R1_EINVAL;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    return enqueue_frame(c, p, d_block, 1, d_num_rays, st, true);
}

extern "C" int r1_render_shard_device_once(r1_context *c, const r1_params *p, void *d_block, void *d_num_rays, void *hip_stream)
{
    if (!c || !p || !d_block || !d_num_rays)
    {
        r1_set_error("r1_render_shard_device_once: null argument");
        return R1_EINVAL;
    }
    if ((uintptr_t)d_num_rays & 7u)
    {
        r1_set_error("r1_render_shard_device_once: d_num_rays must be 8-byte aligned");
        return R1_EINVAL;
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    return enqueue_frame(c, p, d_block, 1, d_num_rays, st, false);
}

static int assemble_common(r1_context *c, const r1_params *p, const void *d_blocks, size_t shard_stride_bytes, void *d_rgb, void *d_total_rays,
                           void *hip_stream, int n_frames = 1, size_t frame_in = 0, size_t frame_out = 0)
{
    if (!c || !p || !d_blocks || !d_rgb)
    {
        r1_set_error("r1_assemble_device: null argument");
        return R1_EINVAL;
    }
    int32_t total = 0, per = 0;
    int rc = r1_tile_count(p, &total, &per);
    if (rc)
        return rc;
    const size_t tight = (size_t)per * p->tile_w * p->tile_h * 3;
    if (shard_stride_bytes == 0)
        shard_stride_bytes = tight;
    if (shard_stride_bytes < tight)
    {
        r1_set_error("r1_assemble_device: shard stride %zu smaller than a shard block (%zu bytes)", shard_stride_bytes, tight);
        return R1_EINVAL;
    }
    if (d_total_rays && (((uintptr_t)d_total_rays | (uintptr_t)d_blocks | shard_stride_bytes | frame_in | frame_out) & 7u))
    {
        r1_set_error("r1_assemble_device_records: records and totals must be 8-byte aligned");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int tiles_x = (p->width + p->tile_w - 1) / p->tile_w;
    const size_t record = r1_shard_record_bytes(p);
    R1_HIP(r1_launch_assemble(d_blocks, d_rgb, p->width, p->height, p->tile_w, p->tile_h, tiles_x, p->num_shards, shard_stride_bytes, n_frames, frame_in,
                              frame_out, record - 8, d_total_rays ? (long long)((char *)d_total_rays - (char *)d_rgb) : 0, d_total_rays ? 1 : 0, st));
    return R1_OK;
}

extern "C" int r1_assemble_device_strided(r1_context *c, const r1_params *p, const void *d_blocks, size_t shard_stride_bytes, void *d_rgb,
                                          void *hip_stream)
{
    return assemble_common(c, p, d_blocks, shard_stride_bytes, d_rgb, nullptr, hip_stream);
}

extern "C" int r1_assemble_device_records(r1_context *c, const r1_params *p, const void *d_records, void *d_rgb, void *d_total_rays, void *hip_stream)
{
    if (!d_total_rays)
    {
        r1_set_error("r1_assemble_device_records: null d_total_rays");
        return R1_EINVAL;
    }
    return assemble_common(c, p, d_records, r1_shard_record_bytes(p), d_rgb, d_total_rays, hip_stream);
}

// Batches: d_gathered = what one all-gather of every shard's n_frames records returns, [shard][frame][record]; d_frames receives
// n_frames frame records (r1_frame_record_bytes each: row-major image, padded to 8 bytes, + the frame's uint64 ray count).
extern "C" int r1_assemble_device_records_batch(r1_context *c, const r1_params *p, int32_t n_frames, const void *d_gathered, void *d_frames,
                                                void *hip_stream)
{
    if (n_frames < 1 || !d_frames)
    {
        r1_set_error("r1_assemble_device_records_batch: bad argument");
        return R1_EINVAL;
    }
    const size_t record = r1_shard_record_bytes(p), frame = r1_frame_record_bytes(p);
    if (!record)
        return R1_EINVAL;
    return assemble_common(c, p, d_gathered, record * (size_t)n_frames, d_frames, (char *)d_frames + frame - 8, hip_stream, n_frames, record, frame);
}

extern "C" int r1_assemble_device(r1_context *c, const r1_params *p, const void *d_blocks, void *d_rgb, void *hip_stream)
{
    return r1_assemble_device_strided(c, p, d_blocks, 0, d_rgb, hip_stream);
}

extern "C" int r1_set_pixel_mode(r1_context *c, int32_t on)
{
    if (!c)
        return R1_EINVAL;
    c->pixel_mode = on != 0;
    return R1_OK;
}

extern "C" int r1_sync(r1_context *c)
{
    if (!c)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    return land_check(c);
}

extern "C" int r1_last_timing(r1_context *c, double *trace_kernel_ms, double *total_ms)
{
    if (!c || !c->timing_valid)
    {
        r1_set_error("r1_last_timing: nothing rendered yet");
        return R1_EINVAL;
    }
    R1_HIP(hipEventSynchronize(c->last2));
    float a = 0, b = 0;
    R1_HIP(hipEventElapsedTime(&a, c->last0, c->last1));
    R1_HIP(hipEventElapsedTime(&b, c->last0, c->last2));
    if (trace_kernel_ms)
        *trace_kernel_ms = a;
    if (total_ms)
        *total_ms = b;
    return R1_OK;
}

extern "C" int r1_last_stats(r1_context *c, uint64_t *out16)
{
    if (!c || !out16 || !c->counters.p)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    R1_HIP(hipMemcpyAsync(out16, (char *)c->counters.p + 128, 128, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

extern "C" int r1_last_wave_log(r1_context *c, uint64_t *out, size_t cap_waves, uint32_t *waves)
{
    if (!c || !waves)
        return R1_EINVAL;
    *waves = c->wave_log_waves;
    if (!out)
        return R1_OK;
    if (cap_waves < c->wave_log_waves || !c->wave_log.p)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    R1_HIP(hipMemcpyAsync(out, c->wave_log.p, (size_t)c->wave_log_waves * 32, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

extern "C" int r1_timing_begin(r1_context *c, int32_t max_frames)
{
    if (!c || max_frames < 1 || max_frames > 100000)
    {
        r1_set_error("r1_timing_begin: bad argument");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    while ((int)c->ring.size() < 3 * max_frames)
    {
        hipEvent_t e;
        R1_HIP(hipEventCreate(&e));
        c->ring.push_back(e);
    }
    c->ring_frames = max_frames;
    c->ring_used = 0;
    c->ring_on = true;
    return R1_OK;
}

extern "C" int r1_timing_end(r1_context *c, double *trace_ms_sum, double *total_ms_sum, int32_t *frames)
{
    if (!c || !c->ring_on)
    {
        r1_set_error("r1_timing_end without r1_timing_begin");
        return R1_EINVAL;
    }
    c->ring_on = false;
    double a = 0, b = 0;
    for (int i = 0; i < c->ring_used; ++i)
    {
        float x = 0, y = 0;
        R1_HIP(hipEventSynchronize(c->ring[3 * i + 2]));
        R1_HIP(hipEventElapsedTime(&x, c->ring[3 * i], c->ring[3 * i + 1]));
        R1_HIP(hipEventElapsedTime(&y, c->ring[3 * i], c->ring[3 * i + 2]));
        a += x, b += y;
    }
    if (trace_ms_sum)
        *trace_ms_sum = a;
    if (total_ms_sum)
        *total_ms_sum = b;
    if (frames)
        *frames = c->ring_used;
    return R1_OK;
}

extern "C" int r1_last_launch_info(r1_context *c, r1_launch_info *out)
{
    if (!c || !out)
        return R1_EINVAL;
    *out = c->info;
    return R1_OK;
}

// internal (tools/land_debug.py): the context's counter allocation as it is after the stream has drained
extern "C" int r1_debug_dump_counters(r1_context *c, void *out, size_t bytes, size_t *have)
{
    if (!c || !out || !c->counters.p)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    const size_t n = bytes < c->counters.cap ? bytes : c->counters.cap;
    R1_HIP(hipMemcpy(out, c->counters.p, n, hipMemcpyDeviceToHost));
    if (have)
        *have = n;
    return R1_OK;
}
