// r1_frame.cpp — one frame on a stream, step by step: the launch's tiles and counters, the kernel choice, the arguments, the grid size,
// the landing set-up, the trace launch and the launch that closes the frame (enqueue_frame at the end calls them in order).

#include <string.h>

#include <algorithm>
#include <vector>

#include "r1_context.h"


// ---- per-frame setup ------------------------------------------------------------------------------

static bool same_tiling(const r1_params &a, const r1_params &b)
{
    return a.width == b.width && a.height == b.height && a.spp == b.spp && a.tile_w == b.tile_w && a.tile_h == b.tile_h &&
           a.shard == b.shard && a.num_shards == b.num_shards;
}

R1FastDiv make_div(uint32_t d)
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

static int prepare_tiles(r1_context *c, const r1_params *p, const R1TileGeom &g, int n_frames)
{
    if (c->tile_key_valid && same_tiling(c->tile_key, *p) && c->tile_frames == n_frames)
        return R1_OK;
    const int total = r1_tiles(g);
    const uint32_t local = r1_shard_tiles(total, p->shard, p->num_shards);
    const uint64_t full = (uint64_t)p->tile_w * p->tile_h * p->spp;
    if (full * local * (uint64_t)n_frames >= ((uint64_t)1 << 31) || (uint64_t)total * p->num_shards >= ((uint64_t)1 << 31))
    {
        r1_set_error("%d frame(s) of %dx%dx%d with %dx%d tiles exceed 2^31 sample slots per launch", n_frames, g.width, g.height, p->spp, p->tile_w,
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

// The context's counter allocation (its layout: r1_device.h R1_CNT_*, R1_TAIL_*, r1_land_area), sized for the launch's landing area.
// Called by every entry point BEFORE it takes addresses inside the allocation (it may move when the launch needs more room).
static int ensure_counters(r1_context *c, const r1_params *p, const R1TileGeom &g, int n_frames)
{
    int rc = prepare_tiles(c, p, g, n_frames);
    if (rc)
        return rc;
    const size_t F = (size_t)(n_frames > 0 ? n_frames : 1);
    const size_t tiles = F * (size_t)(c->n_local_tiles ? c->n_local_tiles : 1);
    const size_t need = r1_land_area(F, tiles).end;
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
// is measured per node (small spheres: only the kernels that walk the table in global memory carry that arm, bvh_advance), or a tree with
// leaves of more than two sphere pairs (a tuning library's R1_BVH_LEAF: only those kernels keep the pair loop of a leaf visit); grid kernels:
// tables too large for LDS — the small-scene grid kernel's fallback reads the tree from global memory, any tree will do — and PIXEL mode
// (`grid_pixel`), which the grid runs through its big-scene kernel only: the small one's PIXEL build would spill.  Tried for the tree kernel
// on small scenes too (more workgroups per CU): 15 % slower.  A grid's answer holds after ensure_grid.
bool big_scene(const r1_context *c, bool tree, bool grid, bool grid_pixel)
{
    return c->n_active > R1_MAX_ACTIVE_10BIT || (tree && (c->n_bvh_nodes > R1_NODES_LDS_MAX || c->bvh_pad_local || c->bvh_leaf_pairs > 2u)) || (grid && (!c->grid_small || grid_pixel));
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
// `records`: the caller reads the sample records afterwards (a linear frame), so PIXEL mode, which keeps none, is not chosen.
static int choose_kernel(const r1_context *c, const r1_params *p, const FrameJob &job, int variant, Choice &k)
{
    const bool throughput_mode = job.throughput, records = job.linear != nullptr;
    k.variant = variant;
    const bool wavefront = variant == R1_V_WAVEFRONT;
    const bool pixel_wish = throughput_mode && c->pixel_mode && !records;
    const bool big = big_scene(c, r1_is_tree(variant), r1_is_grid(variant), pixel_wish);
    const bool frames = job.batch && job.batch->n_frames > 1; // (a batch or path of one frame: the single-frame kernel, a path's camera by value)
    static const int tp_mode_env = (int)r1_knob("R1_TP_MODE", -1); // tuning experiments: R1_MODE_TP, _LAT or _PIXEL for the throughput entry points
    int want = R1_MODE_LAT;
    if (job.pass)
        want = job.pass->list ? R1_MODE_LISTED : R1_MODE_PASS;
    else if (pixel_wish || (throughput_mode && !records && tp_mode_env == R1_MODE_PIXEL))
        want = R1_MODE_PIXEL;
    else if (throughput_mode && !(tp_mode_env == R1_MODE_LAT && !big)) // (big scenes have no latency build: the knob leaves them alone)
        want = !frames ? R1_MODE_TP : job.batch->cameras ? R1_MODE_PATH : R1_MODE_BATCH;
    // (the wavefront variant has kernels of its own; its grid is sized as the grouped sweep's frames in flight are)
    const bool built = wavefront ? r1_pick(R1_V_SWEEP, big, R1_MODE_TP, k.b) : r1_pick(variant, big, want, k.b);
    if (!built && job.pass)
    {
        r1_set_error("variant %d has no progressive-pass build", p->variant);
        return R1_EINVAL;
    }
    if (job.batch && (!built || !r1_mode_is_tp_family(k.b.mode) || wavefront || r1_is_stats(variant) || variant == R1_V_REFERENCE))
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
// A region's tiles are those of a frame of the region's size (g is that frame's geometry): derived afresh, and the cached tiling is dropped
// as for a listed pass — the key would describe the params' frame, not the region.  A region has no accumulator.
static int size_tiles(r1_context *c, const r1_params *p, const R1TileGeom &g, const FrameJob &job)
{
    const bool region = job.pass && job.pass->region;
    if (region)
        c->tile_key_valid = false;
    int rc = ensure_counters(c, p, g, job.batch ? job.batch->n_frames : 1);
    if (region)
        c->tile_key_valid = false;
    if (rc)
        return rc;
    if (region)
        return R1_OK;
    if (job.pass && job.pass->list)
    {
        c->n_local_tiles = job.pass->n_listed;
        c->total_samples = c->full * job.pass->n_listed;
        c->tile_key_valid = false;
    }
    else if (job.pass)
        return ensure(c->accum, (size_t)c->n_local_tiles * r1_tile_slots(g) * 16);
    return R1_OK;
}

// The launch's sample records (none in PIXEL mode), and a batch's partial ray counts where a resolve launch will follow
static int ensure_records(r1_context *c, const R1TileGeom &g, const Choice &k, const FrameJob &job)
{
    int rc;
    if (job.batch && k.variant != R1_V_TREE)
    {
        // partial ray counts of the resolve launch: one uint64 per (tile of the batch, workgroup column)
        const size_t cols = ((size_t)r1_tile_slots(g) + 255) / 256;
        if ((rc = ensure(c->batch_rays, (size_t)job.batch->n_frames * (c->n_local_tiles ? c->n_local_tiles : 1) * cols * 8)))
            return rc;
    }
    if (k.b.mode == R1_MODE_PIXEL)
        return R1_OK;
    const size_t want = (size_t)(c->total_samples ? c->total_samples : 1) * 16;
    const bool fresh = !c->samples.p || c->samples.cap < want;
    if ((rc = ensure(c->samples, want)))
        return rc;
    if (fresh) // a record is recognised by its launch's tag: fresh memory must not carry one by accident
        R1_HIP(hipMemsetAsync(c->samples.p, 0, c->samples.cap, job.st));
    return R1_OK;
}

// The context's scene as the kernels read it: every table and number of R1DeviceScene (renders and ray queries alike)
void fill_scene(const r1_context *c, R1DeviceScene &s)
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
void fill_walk(const r1_context *c, bool tree_lds, bool big, uint32_t top_nodes, R1TraceArgs &a)
{
    a.bvh_depth = c->bvh_depth > 0 ? c->bvh_depth : 1;
    a.bvh_lds_f4 = !tree_lds ? 0u : (!big ? 4u * c->n_bvh_nodes : 4u * std::min(c->n_bvh_nodes, top_nodes));
}

// Everything of R1TraceArgs that follows from the context, the params and the kernel choice; the batch block, the grid size and the
// landing are the later steps'.  Takes addresses inside the counter allocation: after size_tiles.
static void frame_args(const r1_context *c, const r1_params *p, const Choice &k, const FrameJob &job, const R1TileGeom &g, R1TraceArgs &a)
{
    memset(&a, 0, sizeof(a));
    fill_scene(c, a.scene);
    a.cam = job.batch && job.batch->cameras && job.batch->n_frames == 1 ? device_camera(job.batch->cameras[0]) : c->cam;
    // (g: the frame's geometry — a region's: the launch's bound test and record places see a frame of the region's size, while 1/W and 1/H stay the
    //  whole frame's, with which the region's lanes aim their samples, r1_sample.hpp start_sample)
    a.width = g.width, a.height = g.height, a.spp = p->spp, a.max_bounces = p->max_bounces;
    a.seed = p->seed;
    a.inv_w = 1.0f / p->width, a.inv_h = 1.0f / p->height; // Vec3 inv_image_size(1.0f / td.image_w, 1.0f / td.image_h, 0) rayweek1.cpp:746
    a.tile_w = g.tile_w, a.tile_h = g.tile_h, a.tiles_x = g.tiles_x;
    a.shard = p->shard, a.num_shards = p->num_shards;
    a.n_local_tiles = c->n_local_tiles, a.full = c->full, a.total_samples = c->total_samples;
    a.div_full = make_div(c->full), a.div_spp = make_div((uint32_t)p->spp), a.div_tw = make_div((uint32_t)p->tile_w), a.div_tx = make_div((uint32_t)a.tiles_x);
    a.queue = (uint32_t *)counter_at(c, R1_CNT_HEADS);
    static const int coop_env = (int)r1_knob("R1_COOP_LANES", -1);
    a.coop_lanes = coop_env >= 0 ? (uint32_t)coop_env : R1_COOP_LANES;
    a.samples = (float4 *)c->samples.p;
    a.num_rays = k.fused_clear ? (unsigned long long *)counter_at(c, R1_CNT_RAYS) : (unsigned long long *)job.rays;
    a.stats = r1_is_stats(k.variant) ? (unsigned long long *)counter_at(c, R1_CNT_STATS) : nullptr;
    if (r1_is_grid(k.variant))
        a.grid = (const R1GridArgs *)(k.b.big ? c->grid_dev32.p : c->grid_dev.p), a.scene.bvh_root_leaf = 0u; // (the grid kernels' fallback walks the tree from its root: no root step, r1_hit_tree.hpp bvh_advance)
    static const int big_top_env = (int)r1_knob("R1_BIG_TOP", R1_BVH_TOP_NODES); // tuning experiments
    fill_walk(c, r1_is_tree(k.variant), k.b.big, (uint32_t)std::max(1, big_top_env), a);
    if (k.b.mode == R1_MODE_PIXEL)
    {
        // the queue holds the padded pixels of the shard's tiles, and `samples` is the output the kernel resolves into
        const uint32_t tp = r1_tile_slots(g);
        a.full = tp, a.div_full = make_div(tp), a.total_samples = c->n_local_tiles * tp;
        a.samples = (float4 *)job.out, a.block_layout = job.block_layout;
        a.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
    }
}

// Takes a batch-argument slot (R1_BATCH_SLOTS slots in the counter allocation's tail, R1_TAIL_BATCH_SLOTS) and writes `words` into it by a
// launch of its own, in stream order: the previous launch through this context has finished reading its copy by the time this one is
// written, and a NEW slot leaves a launch still reading the previous numbers undisturbed.  `cache` (a batch's numbers): an unchanged batch
// on the same stream reuses its slot and writes nothing.  cache == null (a path, whose block ends in a table address, and a pass): always a
// new slot, and batch_args_last is cleared, so that a batch that follows takes a new slot too (its numbers never equal the cleared ones:
// n_frames >= 2).  Returns the slot.
static int put_batch_args(r1_context *c, const void *words, int n_words, const R1BatchArgs *cache, hipStream_t st, const R1BatchArgs **slot)
{
    char *const slots = counter_at(c, R1_TAIL_BATCH_SLOTS);
    static_assert((R1_BATCH_SLOTS & (R1_BATCH_SLOTS - 1)) == 0, "the slots are taken in turn with a mask");
    if (!cache || c->batch_args_slot < 0 || c->batch_args_stream != st || memcmp(cache, &c->batch_args_last, sizeof(*cache)) != 0)
    {
        c->batch_args_slot = (c->batch_args_slot + 1) & (int)(R1_BATCH_SLOTS - 1);
        if (cache)
            c->batch_args_last = *cache;
        else
            memset(&c->batch_args_last, 0, sizeof(c->batch_args_last));
        c->batch_args_stream = st;
        R1_HIP((n_words == 8 ? r1_launch_put8 : r1_launch_put6)(slots + R1_BATCH_SLOT_BYTES * c->batch_args_slot, (const uint32_t *)words, st));
    }
    *slot = (const R1BatchArgs *)(slots + R1_BATCH_SLOT_BYTES * c->batch_args_slot);
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
static int put_batch_block(r1_context *c, const r1_params *p, const Choice &k, const FrameJob &job, R1TraceArgs &a)
{
    static_assert(sizeof(R1BatchArgs) == 24 && sizeof(R1PassArgs) == 24, "r1_launch_put6 writes the six words of R1BatchArgs / R1PassArgs");
    static_assert(sizeof(R1PathArgs) == 32 && __builtin_offsetof(R1PathArgs, cameras) == 24, "r1_launch_put8 writes the eight words of R1PathArgs into a 32-byte slot");
    int rc;
    if (r1_mode_is_batch(k.b.mode))
    {
        const bool path = k.b.mode == R1_MODE_PATH;
        R1PathArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.batch.n_frames = (uint32_t)job.batch->n_frames, pa.batch.seed_stride = job.batch->seed_stride;
        pa.batch.div_tiles = make_div(c->n_local_tiles ? c->n_local_tiles : 1u), pa.batch.n_local_tiles = c->n_local_tiles;
        if (path && (rc = put_path_cameras(c, job.batch, job.st, &pa.cameras)))
            return rc;
        if ((rc = put_batch_args(c, &pa, path ? 8 : 6, path ? nullptr : &pa.batch, job.st, &a.batch)))
            return rc;
    }
    if (job.pass)
    {
        R1PassArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.first_sample = (uint32_t)job.pass->first_sample;
        pa.list = job.pass->list;
        if (job.pass->region) // (the corner the lanes add, and the frame's width they seed with)
            pa.x0 = (uint32_t)job.pass->region->x0, pa.y0 = (uint32_t)job.pass->region->y0, pa.frame_w = (uint32_t)p->width;
        return put_batch_args(c, &pa, 6, nullptr, job.st, &a.batch);
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
// pixels: PIXEL mode — the padded pixels the queue holds instead of the launch's sample slots — else 0
static GridSize size_grid(const r1_context *c, const Choice &k, const FrameJob &job, int per_cu, uint32_t pixels, int num_shards)
{
    const int cus = c->cus;
    const uint32_t total = c->total_samples;
    const bool pixel_mode = k.b.mode == R1_MODE_PIXEL, latency = r1_runs_as_latency(k.b.mode, k.b.big), throughput_mode = job.throughput;
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
        // a wave only ever pulls from its home sub-queue (r1_trace.hpp r1_trace_body: home = (4 (block / 8) + wave) % nq), so every
        // sub-queue needs home waves: the full groups of 8 workgroups must cover all nq residues
        const long long nq = std::min<long long>({nq_env > 0 ? nq_env : R1_SUBQUEUES, 4 * (g.blocks / 8), (long long)R1_HEADS});
        if (nq > 1)
        {
            g.nq = (uint32_t)nq;
            g.chunk_max = g.chunk_min = chunk_max_env > 0 ? (uint32_t)chunk_max_env : 64u;
        }
    }
    return g;
}

// Landing set-up (tiles resolved inside the trace kernel): the launch's set of queue heads, its record tag, the armed countdowns, where the
// tiles land — the caller's own memory where the device can write there, which redirects the job's out and rays for the steps behind this
// one — and the waves' tile lists.
// Launches alternate between two sets of queue heads and wave counts; workgroup 0 zeroes the set the launch before used, which nobody
// touches any more (a workgroup that starts late still asks its own queue for work after the frame's last tile has been summed, so a
// launch cannot clear its own).  After anything else has run through this context both sets (and the round-3 block) are cleared here.
// land_prev and land_armed are cleared BEFORE anything here can fail, and they and land_parity are committed by enqueue_frame only once
// the trace launch is enqueued: until then the context counts as neither, so a call refused from here on (tile lists too long, an
// allocation, the launch) sends the next one through both memsets and the arming launch — it would otherwise take the set the last
// launch that ran left exhausted, and no tile would be summed.
static int land_setup(r1_context *c, const r1_params *p, FrameJob &job, long long blocks, R1TraceArgs &a, int &land_parity)
{
    const int n_frames = job.batch ? job.batch->n_frames : 1;
    const hipStream_t st = job.st;
    const bool prev = c->land_prev, armed = c->land_armed;
    c->land_prev = false, c->land_armed = false;
    land_parity = prev ? c->land_parity ^ 1 : 0;
    if (!prev)
    {
        R1_HIP(hipMemsetAsync(c->counters.p, 0, R1_COUNTER_BYTES, st));
        R1_HIP(hipMemsetAsync(counter_at(c, R1_TAIL_HEADS), 0, R1_HEADS * 4 * R1_HEAD_WORDS, st)); // (not the batch-argument slots in front of it)
    }
    char *const set0 = counter_at(c, R1_CNT_HEADS), *const set1 = counter_at(c, R1_TAIL_HEADS);
    a.queue = (uint32_t *)(land_parity ? set1 : set0);
    a.land.clear_heads = (uint32_t *)(land_parity ? set0 : set1);
    a.land.clear_count = R1_HEADS;
    static_assert(R1_HEADS <= R1_BLOCK, "workgroup 0 clears a set of queue heads in one or a few trips");
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
    const R1LandArea area = r1_land_area((size_t)n_frames, 0);
    unsigned long long *frame_rays = (unsigned long long *)counter_at(c, area.frame_rays);
    uint32_t *frame_left = (uint32_t *)counter_at(c, area.frame_left);
    a.land_cnt = (uint32_t *)counter_at(c, area.tile_cnt); // (every countdown on a 128-byte line of its own)
    if (!armed || c->land_frames != n_frames || !same_tiling(c->land_key, *p))
    {
        const R1TileGeom g = r1_tile_geom(p->width, p->height, p->tile_w, p->tile_h); // (only where the tiling changed: the arming launch)
        const R1LandArmArgs arm = {a.land_cnt, frame_rays, frame_left, (uint32_t)n_frames, c->n_local_tiles, g, p->spp, p->shard, p->num_shards};
        R1_HIP(r1_launch_land_arm(&arm, st));
        c->land_frames = n_frames, c->land_key = *p; // (land_armed: committed with the launch)
    }
    if (job.landing && job.landing->out && (job.batch || job.landing->rays))
    {
        job.out = job.landing->out;
        if (!job.batch)
            job.rays = job.landing->rays;
        job.landing->used = true;
    }
    a.land.out = (uint8_t *)job.out, a.land.rays_dst = (unsigned long long *)job.rays;
    a.land.out_stride = job.batch ? job.batch->out_stride : 0, a.land.rays_offset = job.batch ? job.batch->rays_offset : 0, a.land.rays_in_out = job.batch ? 1u : 0u;
    a.land.frame_rays = frame_rays, a.land.frame_left = frame_left;
    a.land.n_frames = (uint32_t)n_frames, a.land.block_layout = (uint32_t)job.block_layout;
    a.land.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
    a.land.error = c->host_word_dev ? &c->host_word_dev->land_error : nullptr;
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
static int prepare_memory(r1_context *c, const Choice &k, const FrameJob &job, long long blocks, int per_cu, R1TraceArgs &a)
{
    const hipStream_t st = job.st;
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
        R1_HIP(hipMemcpyAsync(counter_at(c, R1_CNT_WAVE_LOG), &c->wave_log_ptr, 8, hipMemcpyHostToDevice, st));
    }
    if (!k.fused_clear && !k.land)
        R1_HIP(hipMemsetAsync(job.rays, 0, 8, st));
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
static int close_frame(r1_context *c, const r1_params *p, const Choice &k, const FrameJob &job, const R1TileGeom &g)
{
    const hipStream_t st = job.st;
    R1FrameClose close = {nullptr, nullptr, nullptr};
    if (k.fused_clear)
        close = {(const unsigned long long *)counter_at(c, R1_CNT_RAYS), (unsigned long long *)job.rays, (uint32_t *)c->counters.p};
    static const int resolve_rows = (int)r1_knob("R1_RESOLVE_ROWS", R1_RESOLVE_ROWS_TP); // tuning experiments
    if (k.b.mode == R1_MODE_LISTED && c->n_local_tiles)
    {
        // adaptive sampling: the records go into the listed tiles' two accumulators, their `all` bytes into job.out, and every listed tile is tested
        const int32_t n = job.pass->first_sample + p->spp;
        R1AdaptArgs ad = {};
        ad.samples = (const float4 *)c->samples.p, ad.list = job.pass->list;
        ad.all = (float4 *)c->accum.p, ad.even = (float4 *)c->accum_even.p;
        ad.out = (uint8_t *)job.out, ad.report = (R1TileReport *)c->adapt_report.p;
        ad.geom = g, ad.spp = p->spp;
        ad.n_listed = job.pass->n_listed, ad.first_sample = (uint32_t)job.pass->first_sample;
        ad.inv_all = (float)(1.0f / n), ad.inv_even = (float)(1.0f / ((n + 1) / 2)); // rayweek1.cpp:765 at the samples each accumulator holds
        ad.max_delta = job.pass->rule->max_delta, ad.mean_delta_q8 = (uint32_t)job.pass->rule->mean_delta_q8;
        ad.close = close;
        R1_HIP(r1_launch_adapt_accum(&ad, st));
    }
    else if (job.pass && job.pass->region && c->n_local_tiles)
    {
        // region render: the records of the region's tiles, resolved into the caller's window (bytes, floats or both)
        const r1_region *const rg = job.pass->region;
        R1RegionArgs r = {};
        r.samples = (const float4 *)c->samples.p;
        r.out_u8 = (uint8_t *)job.out, r.out_f32 = job.pass->region_linear;
        r.full = c->full, r.n_tiles = c->n_local_tiles;
        r.geom = g, r.spp = p->spp;
        r.stride = (uint32_t)(rg->out_stride ? rg->out_stride : rg->width);
        r.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
        r.close = close;
        R1_HIP(r1_launch_resolve_region(&r, st));
    }
    else if (job.pass && c->n_local_tiles)
    {
        // progressive pass: the records go into the accumulator, and the preview of samples [0, first_sample + spp) into job.out
        R1AccumArgs ac = {};
        ac.samples = (const float4 *)c->samples.p, ac.accum = (float4 *)c->accum.p;
        ac.out = job.pass->image ? (uint8_t *)job.out : nullptr;
        ac.full = c->full, ac.n_local_tiles = c->n_local_tiles;
        ac.geom = g, ac.spp = p->spp;
        ac.fresh = job.pass->first_sample == 0 ? 1u : 0u;
        ac.inv_n = (float)(1.0f / (job.pass->first_sample + p->spp)); // rayweek1.cpp:765 at the accumulated spp
        ac.close = close;
        R1_HIP(r1_launch_accum(&ac, st));
    }
    else if (k.land)
        ; // the trace launch resolved its tiles itself
    else if (c->n_local_tiles && k.b.mode != R1_MODE_PIXEL)
    {
        R1ResolveArgs r = {};
        r.samples = (const float4 *)c->samples.p;
        r.full = c->full, r.n_local_tiles = c->n_local_tiles;
        r.geom = g, r.spp = p->spp;
        r.shard = p->shard, r.num_shards = p->num_shards;
        r.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
        r.out = (uint8_t *)job.out, r.block_layout = job.block_layout;
        r.n_frames = (uint32_t)(job.batch ? job.batch->n_frames : 1);
        if (job.batch)
        {
            r.out_stride = job.batch->out_stride, r.rays_offset = job.batch->rays_offset;
            r.frame_rays = (unsigned long long *)c->batch_rays.p;
        }
        r.close = close;
        R1_HIP(r1_launch_resolve(&r, job.throughput ? resolve_rows : 0, st));
    }
    else if (job.batch) // a shard without tiles: its frames' counts are zero
        for (int f = 0; f < job.batch->n_frames; ++f)
            R1_HIP(hipMemsetAsync((char *)job.out + (size_t)f * job.batch->out_stride + job.batch->rays_offset, 0, 8, st));
    return R1_OK;
}

// A linear frame's one more launch: the records the trace launch left, summed as the resolve sums them, into linear->out.
// Whole single frames (the entry points see to it), so a tile of the launch is a tile of the frame.
static int resolve_linear(const r1_context *c, const r1_params *p, const FrameJob &job, const R1TileGeom &g)
{
    if (!c->n_local_tiles || !c->total_samples)
        return R1_OK;
    if (job.linear->moments) // a variance frame: one launch in the linear one's place stores both
    {
        R1MomentsArgs m = {};
        m.samples = (const float4 *)c->samples.p, m.out = job.linear->out, m.moments = (uint4 *)job.linear->moments;
        m.full = c->full, m.n_tiles = c->n_local_tiles;
        m.geom = g, m.spp = p->spp;
        m.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
        m.inv_nn = p->spp > 1 ? 1.0f / ((float)p->spp * (float)(p->spp - 1)) : 0.0f;
        R1_HIP(r1_launch_resolve_moments(&m, job.throughput ? R1_RESOLVE_ROWS_TP : 0, job.st));
        return R1_OK;
    }
    R1LinearArgs l = {};
    l.samples = (const float4 *)c->samples.p, l.out = job.linear->out;
    l.full = c->full, l.n_tiles = c->n_local_tiles;
    l.geom = g, l.spp = p->spp;
    l.inv_spp = (float)(1.0f / p->spp); // rayweek1.cpp:765
    R1_HIP(r1_launch_resolve_linear(&l, job.throughput ? R1_RESOLVE_ROWS_TP : 0, job.st));
    return R1_OK;
}

// Enqueues the frame (trace + whatever closes it) on job.st.  job.out / job.rays are device addresses; job.rays == NULL stands for the context's
// own count word (R1_TAIL_RAYS of the counter allocation; the allocation may move in here, so callers take that address afterwards).
int enqueue_frame(r1_context *c, const r1_params *p, FrameJob job)
{
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    const r1_region *const region = job.pass ? job.pass->region : nullptr;
    int rc = region ? r1_region_check(p, region) : r1_params_check(p); // (a region's frame need not fit one launch)
    if (rc)
        return rc;
    const hipStream_t st = job.st;
    const int variant = resolve_variant(c, p->variant, job.throughput);
    if (c->moved && variant != R1_V_REFERENCE && !r1_is_tree(variant) && !(r1_is_grid(variant) && c->grid_valid)) // (a grid r1_regrid re-registered serves)
    {
        r1_set_error("variant %d: the scene has moved (r1_update_centers) and only the box tree was refitted, not the sphere groups and the uniform grid; "
                     "r1_set_scene rebuilds them", variant);
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    if (r1_is_grid(variant) && (rc = ensure_grid(c)))
        return rc;
    // the frame's geometry, for every step and closing launch; a region's: that of a frame of the region's size, tiles cut from its own corner
    const R1TileGeom g = region ? r1_tile_geom(region->width, region->height, p->tile_w, p->tile_h) : r1_tile_geom(p->width, p->height, p->tile_w, p->tile_h);
    if ((rc = size_tiles(c, p, g, job)))
        return rc;
    if (!job.rays) // (only now: the counter allocation may have moved)
        job.rays = counter_at(c, R1_TAIL_RAYS);
    Choice k;
    if ((rc = choose_kernel(c, p, job, variant, k)) || (rc = ensure_records(c, g, k, job)))
        return rc;

    R1TraceArgs a;
    frame_args(c, p, k, job, g, a);
    if ((rc = put_batch_block(c, p, k, job, a)))
        return rc;
    int per_cu = 1, land_parity = 0;
    if ((rc = blocks_per_cu(c, k, a, &per_cu)))
        return rc;
    const GridSize gs = size_grid(c, k, job, per_cu, k.b.mode == R1_MODE_PIXEL ? a.total_samples : 0u, p->num_shards);
    a.chunk_min = gs.chunk_min, a.chunk_max = gs.chunk_max, a.nq = gs.nq;
    long long blocks = gs.blocks;
    if (k.land && (rc = land_setup(c, p, job, blocks, a, land_parity)))
        return rc;
    hipEvent_t e[3];
    take_events(c, e);
    if ((rc = prepare_memory(c, k, job, blocks, per_cu, a)))
        return rc;

    R1_HIP(hipEventRecord(e[0], st));
    c->walk_form = 0;
    if (c->total_samples && variant != R1_V_WAVEFRONT)
        R1_HIP(r1_launch_trace(&a, k.b, (int)blocks, r1_is_grid(variant) && !k.b.big ? c->grid_args.lds_bytes : 0u, st, &c->walk_form, region ? 1 : 0));
    if (c->total_samples && variant == R1_V_WAVEFRONT && (rc = launch_wavefront(c, a, st, &blocks)))
        return rc;
    R1_HIP(hipEventRecord(e[1], st));
    if ((rc = close_frame(c, p, k, job, g)))
        return rc;
    c->counters_clean = k.fused_clear;
    c->land_prev = k.land;
    if (k.land)
        c->land_parity = land_parity, c->land_armed = true;
    if (job.linear && (rc = resolve_linear(c, p, job, g)))
        return rc;
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
