// r1_context.h — what the files that implement the C-ABI on the HIP runtime share: the context, its device buffers, and the steps that
// one of them defines and another calls.  Private to r1_capi.cpp (context, errors, timing), r1_scene.cpp (scene upload),
// r1_scene_update.cpp (moving spheres, sphere updates, re-sort), r1_scene_grid.cpp (the grid's upload, regrid), r1_frame.cpp (one frame,
// step by step), r1_render.cpp (the render entry points), r1_queries.cpp (ray and path queries), r1_denoise.cpp (denoised frames) and r1_accumulate.cpp (accumulated frames); C-linkage functions
// shared between files stay in r1_internal.h.
#ifndef R1_CONTEXT_H
#define R1_CONTEXT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/rays1.h"
#include "r1_device.h"
#include "r1_grid.h"
#include "r1_grid_fill.h"
#include "r1_bvh.h" // r1_bvh.cpp: the built tree, a refit's topology tables
#include "r1_internal.h"

#pragma GCC visibility push(hidden)

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

// A device allocation that only grows (ensure) and is freed with its owner: a context's buffers go when the context is deleted, on the
// device that is current then.
struct DevBuf
{
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf()
    {
        if (p)
            (void)hipFree(p);
    }
};

inline int ensure(DevBuf &b, size_t bytes)
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
    // r1_regrid (r1_regrid.hip).  grid_valid says "the tables are those of the spheres the device holds": every update clears
    // it, a regrid sets it again.  grid_planned says "the grid's buffers and plan belong to this scene": only r1_set_scene clears it.
    bool grid_planned = false;
    R1GridPlan grid_plan;     // what ensure_grid's build decided for the arrays of r1_set_scene
    bool regrid_ready = false; // the scene's first regrid has grown the tables to the capacity and laid out the scratch
    R1RegridArgs regrid;
    DevBuf regrid_ws;
    DevBuf wf_paths, wf_hits, wf_queue, wf_counts; // R1_VARIANT_WAVEFRONT workspace
    DevBuf wave_log;                               // STATS builds: per-wave {start, queue empty, end, iterations}
    unsigned long long wave_log_ptr = 0;
    uint32_t wave_log_waves = 0;
    uint32_t n_bvh_nodes = 0, n_bvh_leaves = 0;
    int bvh_depth = 0;
    uint32_t bvh_leaf_pairs = 0; // the most sphere pairs in a leaf (R1_BVH_LEAF / 2 unless a tuning knob builds larger leaves)
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
    // frame batches: the batch's numbers live in one of the batch-argument slots of the counter allocation (r1_device.h R1_TAIL_BATCH_SLOTS), written by a one-thread launch whose
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

    // 64 page-locked, device-visible bytes (r1_device.h R1HostWords): the synchronous entry points let the frame's last launch store the
    // ray count straight into host memory (8 bytes over PCIe at the end of r1_resolve_kernel) instead of enqueueing a second copy
    R1HostWords *host_word = nullptr, *host_word_dev = nullptr; // the host's address, the device's
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
    // linear frames (r1_render_linear*, r1_pass_linear, r1_render_adaptive_linear): `image` is sized for bytes
    DevBuf linear;             // row-major width*height*3 floats, where the caller's memory is not the device's to write
    DevBuf moments;            // variance frames (r1_render_moments): row-major width*height r1_moment records, on the same terms
    // ray queries (r1_cast_rays*): nothing here is read or written by a render
    DevBuf active_dev;         // active_to_scene on the device, uploaded once per r1_set_scene
    DevBuf cast_cursors;       // R1_CAST_CURSORS ray cursors, 128 bytes apart, taken in turn
    uint32_t cast_cursor_next = 0;
    DevBuf cast_ws;            // r1_cast_rays, r1_trace_rays: one chunk's rays, seeds and records (R1_CAST_CHUNK x 64 bytes)
    int query_occupancy[R1_JOBS][8] = {{0}}; // blocks per CU of the query kernels, [job][structure slot * 2 + big]; follows the tree as `occupancy` does
    // denoised frames (r1_denoise*, r1_render_denoised*): the filter's records, then what the composed forms keep beside them
    DevBuf denoise_ws;         // r1_denoise.cpp denoise_layout; nothing here is read or written by a render
    // accumulated frames (r1_accumulate*, r1_render_accumulated*; r1_accumulate.cpp)
    DevBuf history_ws;         // a 256-byte head (a composed frame's ray count), two history slots {f, M, A} and a dense output frame
    DevBuf accumulate_io;      // r1_accumulate: the eight images of a call on host memory, dense
    int history_slot = -1;     // the slot that holds the last accumulated frame; -1: the history is empty
    int32_t history_w = 0, history_h = 0, history_spp = 0;
    r1_camera history_cam;     // the context's camera at that call
    // path queries (r1_trace_rays*): one launch in flight per context
    DevBuf trace_stack;        // the paths' attenuation stack, [max_bounces][threads of the launch] hit indices
    // moving spheres (r1_update_centers*): the refit's tables — topology, uploaded once per r1_set_scene — and its scratch
    DevBuf refit_tab;          // uint32: scene -> active index, then R1RefitTopo's slot, leaf_ref, child_box, by_height
    DevBuf refit_radii;        // [active][2] fp64 {bound radius, test radius}
    DevBuf refit_box;          // 256 bytes (word 0: the largest A), then [nodes + leaves] R1Box
    R1RefitArgs refit;         // pointers into the tables above and the scene's
    std::vector<uint32_t> refit_height_off; // R1RefitTopo::height_off
    std::vector<uint32_t> scene_to_active;  // 0xFFFFFFFF: not active
    // re-sort (r1_resort_spheres): its topology tables, uploaded with the refit's, and its scratch, kept from call to call
    DevBuf sort_tab;           // uint32: R1SortTopo's mov, mslot, seg (3 words each), pos_seg
    DevBuf sort_ws;            // uint32: two list buffers and two key buffers of 3 M, the scan's 3 M, the flags, the nodes' axes, the histogram, the block sums
    R1SortArgs sort;           // pointers into the two above and the scene's; m == 0: nothing is movable
    std::vector<uint32_t> sort_depth_off; // R1SortTopo::depth_off
    uint32_t n_bvh_ids = 0;    // leaf slots of the tree (2 per pair), without the sentinel words behind them
    bool moved = false;        // an update since the last r1_set_scene: the sphere groups and the grid are stale, src_f32 may be
    bool src_stale = false;    // r1_update_spheres_device since the last r1_set_scene: the host copies (src_f32, src_mat) never saw its values
    float *stage = nullptr, *stage_dev = nullptr; // host form: page-locked staging of the caller's arrays, read by the move and the set kernel
    size_t stage_cap = 0;      // floats
    hipEvent_t stage_ev = nullptr; // recorded behind the last kernel that reads `stage`
    bool stage_busy = false;

    r1_launch_info info;
    int walk_form = 0; // r1_last_walk_form: what r1_launch_trace said of the last trace launch (1: a flat twin ran)
};

// an address inside the context's counter allocation, by its offset in the layout of r1_device.h (R1_CNT_*, R1_TAIL_*, r1_land_area)
inline char *counter_at(const r1_context *c, size_t offset) { return (char *)c->counters.p + offset; }

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
// the resolve launch.  FrameJob::out receives the preview unless `image` is false.
// A pass of r1_render_adaptive has a tile list: the launch's tiles are list[0, n_listed) of the frame's, traced by the R1_MODE_LISTED kernels and summed
// and tested by r1_adapt_accum_kernel (accumulators and reports: the context's, indexed by tile of the frame).
// A region render (r1_render_region*) is a pass with a region: first_sample 0, the launch's tiles cut from the region's own corner
// (enqueue_frame takes its tile geometry from the region's size), traced by the region twins of the R1_MODE_PASS kernels and closed by
// r1_resolve_region_kernel, which stores FrameJob::out (bytes; may be null), region_linear (floats; may be null) or both with the region's row
// stride.  No accumulator is touched: a progressive accumulation of the context stays as it is.
struct Pass
{
    int32_t first_sample = 0;
    bool image = true;
    const uint32_t *list = nullptr; // device memory
    uint32_t n_listed = 0;
    const r1_adaptive *rule = nullptr;
    const r1_region *region = nullptr; // r1_region_check has passed it
    float *region_linear = nullptr;    // device address
};

// A linear frame (r1_render_linear*): behind the frame's trace and whatever closes it, r1_resolve_linear_kernel sums the records
// the trace left in the context's `samples` into `out`.  The launch keeps per-sample records: PIXEL mode is not chosen, whatever the switch says.
// A variance frame (r1_render_moments*) is a linear frame with `moments` set: r1_resolve_moments_kernel takes the launch's
// place and stores both.
struct Linear
{
    float *out = nullptr;    // device address of width*height*3 floats, row-major (device memory, or page-locked host memory)
    void *moments = nullptr; // device address of width*height r1_moment records, row-major, 16-byte aligned; null: a linear frame alone
};

// What an entry point asks enqueue_frame for: the call sites set the fields they need by name on a local.
struct FrameJob
{
    void *out = nullptr;     // device address of the pixels: row-major image, dense tile block (block_layout 1), a batch's records
    int block_layout = 0;
    void *rays = nullptr;    // device address of the uint64 ray count; null: the context's own count word (R1_TAIL_RAYS)
    hipStream_t st = nullptr;
    bool throughput = false; // the throughput kernels (frames in flight), not the latency ones
    const Batch *batch = nullptr;
    Landing *landing = nullptr;
    const Pass *pass = nullptr;
    const Linear *linear = nullptr;
};

// ---- the steps that cross a file boundary ------------------------------------------------------------------------------------------------

// r1_capi.cpp: a resolver of an earlier launch gave up waiting (the error of r1_sync and of the synchronous render)
int land_check(r1_context *c);

// r1_scene.cpp
R1DeviceCamera device_camera(const r1_camera &cam); // what the kernels read of a camera
// R1_OK, or the refusal (error text set, in `who`'s name) of a null context, of a null `arg` where the call names one, of a context without a scene
int need_scene(const char *who, const r1_context *c, const char *arg_name = nullptr, const void *arg = nullptr);
void forget_occupancy(r1_context *c);               // the cached blocks per CU of the trace and query kernels: their LDS footprint has changed

// r1_scene_grid.cpp
int ensure_grid(r1_context *c);                     // R1_VARIANT_GRID: the grid of the context's scene, built and uploaded once per scene

// r1_frame.cpp
R1FastDiv make_div(uint32_t d);                     // the launch constant by which the kernels' fastdiv divides (r1_device.h R1FastDiv)
bool big_scene(const r1_context *c, bool tree, bool grid, bool grid_pixel);
void fill_scene(const r1_context *c, R1DeviceScene &s);
void fill_walk(const r1_context *c, bool tree_lds, bool big, uint32_t top_nodes, R1TraceArgs &a);
int enqueue_frame(r1_context *c, const r1_params *p, FrameJob job); // (by value: the landing set-up redirects its copy's out and rays)

// Two events of the call's own around `work` on the context's stream, then the stream is waited for: the context's events describe the last
// render.  What the synchronous forms of the filters and of the accumulation time their device work with.
template <class F> static int timed_sync(r1_context *c, const char *who, double *seconds_out, F work)
{
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (seconds_out)
    {
        R1_HIP(hipEventCreate(&ev[0]));
        if (hipEventCreate(&ev[1]) != hipSuccess)
        {
            (void)hipEventDestroy(ev[0]);
            r1_set_error("%s: hipEventCreate failed", who);
            return R1_EHIP;
        }
    }
    // (from here on nothing returns before the events are destroyed)
    hipError_t e = ev[0] ? hipEventRecord(ev[0], c->stream) : hipSuccess;
    int rc = e == hipSuccess ? work() : R1_OK;
    if (rc == R1_OK && e == hipSuccess && ev[1])
        e = hipEventRecord(ev[1], c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream); // (also behind a failed step: nothing of this call is left in flight)
    float ms = 0;
    if (rc == R1_OK && e == hipSuccess && ev[0])
        e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    if (ev[0])
        (void)hipEventDestroy(ev[0]), (void)hipEventDestroy(ev[1]);
    if (rc == R1_OK && e != hipSuccess)
    {
        r1_set_error("%s: %s", who, hipGetErrorString(e));
        rc = R1_EHIP;
    }
    if (rc == R1_OK && seconds_out)
        *seconds_out = ms * 1e-3;
    return rc;
}

// The end of a composed synchronous render (r1_render_denoised, r1_render_denoised_guided, r1_render_accumulated): `enqueue` under timed_sync,
// then the frame of n pixels at d_rgb and the 8-byte ray word at d_rays come home, and a resolver that gave up is reported.
template <class F>
static int timed_render_home(r1_context *c, const char *who, double *seconds_out, const void *d_rgb, const void *d_rays, size_t n, float *rgb_out,
                             uint64_t *num_rays_out, F enqueue)
{
    int rc = timed_sync(c, who, seconds_out, enqueue);
    if (rc)
        return rc;
    uint64_t rays = 0;
    R1_HIP(hipMemcpyAsync(rgb_out, d_rgb, n * 12, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipMemcpyAsync(&rays, d_rays, 8, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    if ((rc = land_check(c)))
        return rc;
    if (num_rays_out)
        *num_rays_out = rays;
    return R1_OK;
}

// What their device siblings refuse behind their own checks: the two outputs, then a context without a scene (before a workspace is grown:
// a refused call changes nothing)
inline int device_outputs_check(const char *who, const r1_context *c, const void *d_rgb_f32, const void *d_num_rays)
{
    if (!d_rgb_f32 || !d_num_rays || ((uintptr_t)d_rgb_f32 & 3u) || ((uintptr_t)d_num_rays & 7u))
    {
        r1_set_error("%s: d_rgb_f32 must be non-NULL and 4-byte aligned, d_num_rays non-NULL and 8-byte aligned", who);
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    return R1_OK;
}

#pragma GCC visibility pop

#endif
