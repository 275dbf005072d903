// r1_device.h — device-side data layout shared by the device headers (r1_trace.hpp and the headers it is made of) and the host files behind
// r1_context.h: launch geometry, the layout of the context's counter allocation and host words, the kernels' argument structs.
#ifndef R1_DEVICE_H
#define R1_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#include "r1_grid_dda.h"
#include "r1_tile.h"

// Launch geometry of the trace kernel.
#define R1_BLOCK 256        // threads per workgroup = 4 wave64
#define R1_BIT_WORDS 8      // small scenes: per-lane flag words in LDS, 32 groups each, worked off 256 groups at a time
#define R1_CAND_CAP 16      // big scenes: per-lane flagged-group slots in LDS (flushed when a lane passes CAP-8)
#define R1_PAIR_CAP 1024    // (lane, sphere) pairs of one wave, big scenes: 64 lanes x R1_CAND_CAP
#define R1_PAIR_CAP_SMALL 512 // same, small scenes (bit path): 4 KB less LDS per workgroup = a fifth workgroup per CU
#define R1_STACK_WORDS 17   // ceil(51 / 3) packed 10-bit hit indices per lane (max_bounces <= 51)
#ifndef R1_STACK_LDS_WORDS
#define R1_STACK_LDS_WORDS 10 // tree kernel, small scenes: words of the packed stack kept in LDS (30 entries); deeper entries (rare) go to
#endif                        // the global workspace.  10 KB instead of 17: with the 128-node table (8 KB) and the 16-bit traversal stack (4 KB,
                              // round 3) a workgroup holds 22 KB = SEVEN workgroups per CU (23.4 KB each at most; six with round 2's 32-bit
                              // traversal stack); 4 / 6 / 8 / 10 / 12 words at six workgroups: 28.4 / 29.1 / 29.3 (32.3) / (32.5) / 28.2 Grays/s
#ifndef R1_STACK_LDS_WORDS_TP
#define R1_STACK_LDS_WORDS_TP 10 // the same for the THROUGHPUT builds of that kernel (r1_mode_is_tp_family), kept apart for experiments: 6 words with the 32-bit
#endif                           // traversal stack was the first way to seven workgroups (+3 % from the wave, -1.7 % from the deeper global overflow)
#define R1_RESOLVE_ROWS_TP 256 // frames in flight: rows of workgroups of the resolve launch (0 = one per tile; 16 / 64 / 256 / one per tile: 29.4 / 30.6 / 31.3 / 30.7 Grays/s over 20 steps, 34.9 / 34.85 / 34.87 / 34.7 over 300), see tile_row_grid (r1_close_kernels.hip)
#define R1_NODES_LDS_MAX 256  // tree kernel: scenes whose tree has at most this many nodes (16 KB) run the small-scene kernels, which keep
                              // the node table in LDS; bigger trees run the big-scene kernels (node table through the vector L1)
#define R1_CHUNK 256        // most samples a wave takes from the global queue per atomic (small frames) ...
#define R1_CHUNK_BIG 1024   // ... growing with a wave's share of the frame up to this (r1_frame.cpp size_grid)
#define R1_CHUNK_MIN 32      // fewest (end of the queue: guided self-scheduling)
#define R1_GROUP_MAX 4         // spheres per group (level 1 of the sweep tests group bounds)
#define R1_GROUP_MIN_SPHERES 128 // scenes with fewer active spheres are swept ungrouped
#define R1_GROUP_RATIO 3.5     // a group's bounding radius stays within this factor of its smallest member radius
#define R1_SAMPLES_PER_LANE 125    // throughput mode grid sizing: samples each lane should get (r1_frame.cpp size_grid): 1200x800x10 -> 300
                                   // workgroups per frame.  Re-tuned after DESIGN §4.13 (a cheaper refill shifts the balance towards fewer,
                                   // longer-lived workgroups; tools/spl_sweep2.sh, three alternating rounds): 100 / 115 / 125 / 135 / 150 samples
                                   // -> 36.46 / 36.75 / 36.90 / 37.00 / 37.3 Grays/s over 300 steps and 32.7 / 33.3 / 33.4 / 32.7 / 32.0 over the
                                   // driver's 20 (a burst drains better with more, shorter-lived workgroups; a long run loses to their drains) ...
#define R1_SAMPLES_PER_LANE_SHARD 100 // ... a rank's share of a frame (num_shards > 1) keeps 100: 0.1054 against 0.1069 ms per frame for an
                                   // emulated rank of eight ...
#define R1_MIN_BLOCKS 128          // ... but at least this many workgroups per frame (the per-rank frames of a 4- or 8-GPU run:
                                   // 0.301 ms per frame against 0.329 with 256) ...
#define R1_SAMPLES_PER_LANE_MIN 32 // ... as long as a lane still gets this many samples
#define R1_TILE_SPHERES 512    // big-scene sweep: spheres per LDS tile (8 KB in pair layout), two tiles in LDS
#define R1_TILE_F4 (R1_TILE_SPHERES / 2 * 2) // float4 per tile: 2 per pair of spheres
#define R1_MAX_ACTIVE_10BIT 1023
#define R1_MAX_ACTIVE (1u << 21) // big-scene kernels: 26-bit pair indices, limit kept at 2 M spheres
#define R1_STACK_ENTRIES 51
#define R1_BVH_STACK 32        // R1_VARIANT_BVH: per-lane traversal stack entries in LDS = most inner nodes on a path
#define R1_BVH_TOP_NODES 63    // box tree: the first nodes in breadth-first order (6 levels); the big-scene kernels keep them in LDS (4 KB: 0 / 63 / 127 / 255 nodes -> 12.9 / 13.3 / 13.0 / 12.6 Grays/s on 100 004 spheres, the larger copies cost workgroups per CU)
#define R1_BVH_LEAF 4          // spheres per leaf (<= 14; stored as pairs)
#define R1_SUBQUEUES 16        // latency mode: sub-queues of the sample queue (R1TraceArgs::nq)
#define R1_COUNTER_BYTES 4096  // block 0 of the context's counter allocation (R1_CNT_* below), zeroed between frames
#define R1_COOP_LANES 2        // R1TraceArgs::coop_lanes (one synchronous frame: 2 -> 1.144 ms, 4 -> 1.160, 8 -> 1.193, 16 -> 1.263)
// Tiles resolved INSIDE the trace kernel (R1_LAND: round 4; r1_land.hpp has the protocol): the throughput kernels sum every
// 32 x 32 tile themselves, on the XCD that traced it, and store the pixels where the frame is wanted — device memory or the caller's
// page-locked host buffer.  No resolve launch, no copy.
#include "r1_builds.h" // the names of variants and modes, the predicates (r1_build_lands: which builds land their tiles), the list of builds
#define R1_LAND_CNT_STRIDE 32u  // words between two tiles' countdowns: every countdown on its own 128-byte line (an atomic on ONE line sustains ~88 M/s on this chip,
                               // tools/ubench_atomic.hip; the ~40 tiles a synchronous frame's waves work on at a time shared two lines at first: 3.8 ms per frame instead of 1.1)
#define R1_LAND_MAX_WAIT (1u << 16) // passes over a claimed tile that still find a record of an earlier launch before the wave gives up and flags the launch
                                    // (a record's store is on its way for microseconds; a bug would otherwise hang the device instead of failing the call)
#define R1_COUNTER_TAIL 4096   // the tail of the counter allocation, behind block 0 (R1_TAIL_* below), never zeroed as a whole
#define R1_LAND_MAX_XCD 8u     // XCDs of the chip: each has a cursor among the queue heads (r1_land.hpp)

// ---- the context's counter allocation (r1_context::counters), byte offsets from its start ------------------------------------------
// Block 0, [0, R1_COUNTER_BYTES): what a frame counts in.  The frame's closing launch — or a memset — zeroes all of it between frames.
constexpr size_t R1_CNT_RAYS = 32;      // uint64: the ray count the trace kernel accumulates (the 32 bytes in front of it are not used)
constexpr size_t R1_CNT_STATS = 128;    // R1_STATS_WORDS uint64: the diagnostic builds' published counters (R1TraceArgs::stats, r1_last_stats) ...
constexpr uint32_t R1_STATS_WORDS = 16;
constexpr size_t R1_CNT_WAVE_LOG = R1_CNT_STATS + 8 * R1_STATS_WORDS; // ... and behind them, as stats[R1_STATS_WORDS], the address of the wave log
constexpr size_t R1_CNT_HEADS = 1024;   // the queue heads (R1TraceArgs::queue): R1_HEADS of them, each on a 128-byte line of its own
constexpr uint32_t R1_HEAD_WORDS = 32;  // uint32 words from one head to the next
constexpr uint32_t R1_HEADS = (R1_COUNTER_BYTES - R1_CNT_HEADS) / (4 * R1_HEAD_WORDS);
// The tail, [R1_COUNTER_BYTES, R1_COUNTER_BYTES + R1_COUNTER_TAIL)
constexpr size_t R1_TAIL_RAYS = R1_COUNTER_BYTES + 0;           // uint64: the published ray count (the count word of a caller that names none)
constexpr size_t R1_TAIL_BATCH_SLOTS = R1_COUNTER_BYTES + 64;   // R1_BATCH_SLOTS batch-argument slots of R1_BATCH_SLOT_BYTES (R1BatchArgs, R1PathArgs, R1PassArgs)
constexpr uint32_t R1_BATCH_SLOTS = 8, R1_BATCH_SLOT_BYTES = 32;
constexpr size_t R1_TAIL_HEADS = R1_COUNTER_BYTES + 1024;       // the second set of queue heads: landing launches alternate between the sets, and
                                                                // workgroup 0 of a launch zeroes the set the launch before it used
// Behind the tail, per landing launch of F frames: frame_rays[F] (uint64 accumulators), frame_left[F] (uint32 tiles to go), then — from the
// next 128-byte line on — the tiles' countdowns, R1_LAND_CNT_STRIDE words apart
constexpr size_t R1_CNT_LAND = (size_t)R1_COUNTER_BYTES + R1_COUNTER_TAIL;
struct R1LandArea
{
    size_t frame_rays, frame_left, tile_cnt, end;
};
constexpr R1LandArea r1_land_area(size_t n_frames, size_t tiles)
{
    const size_t cnt = R1_CNT_LAND + ((n_frames * 16 + 127) & ~(size_t)127);
    return {R1_CNT_LAND, R1_CNT_LAND + n_frames * 8, cnt, cnt + tiles * 4 * R1_LAND_CNT_STRIDE};
}
// The queue heads by role (index of the head; word R1_HEAD_WORDS * index of R1TraceArgs::queue)
constexpr uint32_t R1_HEAD_XCD = 0;        // landing launches: heads [0, R1_LAND_MAX_XCD) are the XCDs' cursors {group + 1, next sample slot} (uint64)
constexpr uint32_t R1_HEAD_SUBQUEUE = 0;   // latency launches: heads [0, nq <= R1_SUBQUEUES) are the sub-queues' chunk counters; any other launch: head 0 is the queue
constexpr uint32_t R1_HEAD_DISPENSER = 16; // landing launches: the next unclaimed tile group
constexpr uint32_t R1_HEAD_DEBUG = 17, R1_HEAD_DEBUG_COUNT = 7; // R1_LAND_DEBUG builds (tools/land_debug.py)
static_assert(R1_CNT_RAYS + 8 <= R1_CNT_STATS && R1_CNT_WAVE_LOG + 8 <= R1_CNT_HEADS && R1_CNT_HEADS + R1_HEADS * 4 * R1_HEAD_WORDS == R1_COUNTER_BYTES,
              "block 0: ray count, published counters, wave log address, queue heads");
static_assert(8 <= R1_TAIL_BATCH_SLOTS - R1_TAIL_RAYS && R1_TAIL_BATCH_SLOTS + R1_BATCH_SLOTS * R1_BATCH_SLOT_BYTES <= R1_TAIL_HEADS &&
                  R1_TAIL_HEADS + R1_HEADS * 4 * R1_HEAD_WORDS <= R1_CNT_LAND,
              "the tail: published ray count, batch-argument slots, the second set of queue heads");
static_assert(R1_HEAD_XCD + R1_LAND_MAX_XCD <= R1_HEAD_DISPENSER && R1_HEAD_SUBQUEUE + R1_SUBQUEUES <= R1_HEAD_DISPENSER && R1_HEAD_DISPENSER < R1_HEAD_DEBUG &&
                  R1_HEAD_DEBUG + R1_HEAD_DEBUG_COUNT <= R1_HEADS,
              "the queue heads' roles fit the heads and do not overlap");
static_assert(R1_LAND_CNT_STRIDE * 4 == 128 && R1_CNT_LAND % 128 == 0 && r1_land_area(3, 1).tile_cnt % 128 == 0, "every countdown on a 128-byte line of its own");

// The context's page-locked, device-visible host words (r1_context::host_word): what a launch stores straight into host memory
struct R1HostWords
{
    unsigned long long rays; // the frame's ray count (the synchronous entry points)
    uint32_t land_error;     // set by a wave that gave up on a tile (R1LandArgs::error); read and cleared by land_check
    uint32_t pad0;
    uint32_t adapt_count;    // adaptive sampling: the next pass's list length
    uint32_t pad1[11];
};
static_assert(sizeof(R1HostWords) == 64 && offsetof(R1HostWords, land_error) == 8 && offsetof(R1HostWords, adapt_count) == 16, "the host words' layout");

// Tuning knobs.  The SHIPPED library never reads the environment: what it does depends on its arguments only.  A build made
// with -DR1_TUNING (`make tuning` -> lib/librays1_tuning.so; the scripts under tools/ load it explicitly) reads the R1_*
// variables named at the call sites, once per process — launch shapes and conservative index layouts that produce the
// same pixels and ray counts; the defaults are what every number in DESIGN.md refers to.
#ifdef R1_TUNING
#include <stdlib.h>
static inline long long r1_knob(const char *name, long long dflt)
{
    const char *v = getenv(name);
    return v ? atoll(v) : dflt;
}
static inline double r1_knob_f(const char *name, double dflt)
{
    const char *v = getenv(name);
    return v ? atof(v) : dflt;
}
#else
static inline long long r1_knob(const char *, long long dflt) { return dflt; }
static inline double r1_knob_f(const char *, double dflt) { return dflt; }
#endif

// Division of n < 2^31 by a launch constant: pow2 ? n >> shift : mulhi(n, mul) >> shift, with
// mul = ceil(2^(32+shift) / d), shift = floor(log2 d) (exact for every n < 2^31; r1_frame.cpp make_div).
struct R1FastDiv
{
    uint32_t mul, shift, pow2;
};

// Frame batches (R1TraceArgs::batch), device memory
struct R1BatchArgs
{
    uint32_t n_frames;   // >= 2
    uint32_t seed_stride;
    R1FastDiv div_tiles; // by n_local_tiles
    uint32_t n_local_tiles;
};

// Camera paths (r1_render_path_async, the R1_MODE_PATH builds): a batch's numbers and, behind them, the table of its frames' cameras — n_frames
// entries of R1_PATH_CAM_F4 float4 (an R1DeviceCamera's 19 floats and one of padding: 16-byte aligned rows), device memory.  Eight words: one
// batch-argument slot, written by r1_launch_put8.
#define R1_PATH_CAM_F4 5
struct R1PathArgs
{
    struct R1BatchArgs batch;
    const float *cameras;
};

// Progressive passes (r1_render_pass, the R1_MODE_PASS builds): the pass's first global sample index, device memory behind R1TraceArgs::batch
// (null in every single-frame launch).  Six words: written by r1_launch_put6 into a batch-argument slot.
// Adaptive sampling (r1_render_adaptive, the R1_MODE_LISTED builds): behind it the pass's tile list — the launch's local tile j is tile list[j] of
// the frame — device memory; null in a pass of r1_render_pass, whose kernels never read it.
// Region renders (r1_render_region*, r1_region_kernel): the region's corner in the frame and the frame's width, which the lanes add and
// seed with once a sample has passed the bound test of the region's own tiles; zero in every other pass, whose kernels never read them.
struct R1PassArgs
{
    uint32_t first_sample;
    uint32_t x0;
    const uint32_t *list;
    uint32_t y0, frame_w;
};

// What the waves that sum finished tiles need (R1_LAND); by value in the kernel arguments, read when a wave has run out of samples.
struct R1LandArgs
{
    uint8_t *out;                   // frame 0's pixels: row-major image (block_layout 0) or dense tile block (1); device memory or page-locked host memory
    unsigned long long *rays_dst;   // !rays_in_out: the frame's ray count (device memory or a page-locked host word)
    unsigned long long out_stride;  // frame f of a batch: out + f * out_stride
    unsigned long long rays_offset; // rays_in_out: frame f's uint64 count at out + f * out_stride + rays_offset
    unsigned long long *frame_rays; // [n_frames] ray-count accumulators (zero between launches)
    uint32_t *frame_left;           // [n_frames] tiles not yet resolved (n_local_tiles between launches)
    uint32_t *clear_heads;          // queue heads and wave counts of the set the PREVIOUS launch through this context used: zeroed by workgroup 0
    uint32_t clear_count;           // ... that many words, R1_HEAD_WORDS words apart
    uint32_t n_frames;              // frames of the launch (1: a single frame)
    uint32_t rays_in_out, block_layout;
    float inv_spp;                  // (float)(1.0f / spp), rayweek1.cpp:765
    uint32_t *owed_spill;           // [waves of the grid][spill_stride]: a wave's list of the tiles it took chunks from, beyond the 24 entries it keeps in LDS
    uint32_t spill_stride;          // = tiles of the launch (a wave meets a tile at most once)
    uint32_t *error;                // page-locked host word (or null): set if a wave gave up on a tile (R1_LAND_MAX_WAIT) — never in a correct run
};

// Everything the trace kernel needs; passed by value (kernarg segment => SGPRs).
struct R1DeviceScene
{
    // Prefilter table over the GROUPS of active spheres (inv_radius != 0; <= R1_GROUP_MAX nearby
    // spheres per group, bounding sphere (g, R)), 8 floats per PAIR of groups
    // {gx0 gx1 gy0 gy1 gz0 gz1 Kp0 Kp1}, Kp = |g|^2 - R^2 - slack; padded with never-candidate
    // entries (Kp = +inf) to a multiple of 8 spheres PLUS one extra chunk of 8 (prefetch target).
    const float4 *sweep;
    // Exact table, same indexing: {cx, cy, cz, radius_sq} and {inv_radius, albedo rgb},
    // {type, param}.
    const float4 *exact;
    const float4 *shade;   // {inv_radius, albedo_r, albedo_g, albedo_b}
    const float4 *exact_g;   // the same {cx, cy, cz, radius_sq} in GROUP order, [n_sweep (+pad)][R1_GROUP_MAX] ({0, 0, 0, -inf} = none: never an offer):
                             // the exact phase fetches a member's sphere and its index side by side instead of one after the other
    const uint32_t *members; // [n_sweep (+pad)][R1_GROUP_MAX] active indices of a group's spheres, 0xFFFFFFFF = none
    const float4 *mat;     // {bit_cast<float>(type), param, 1/ref_idx, ((1-ref)/(1+ref))^2} (last two: dielectrics)
    uint32_t n_multi;      // groups [0, n_multi) have 2..R1_GROUP_MAX members, groups >= n_multi exactly one
    uint32_t n_active;     // real entries
    uint32_t n_sweep;      // GROUPS, padded to a multiple of 8 (+8 prefetch); big scenes: of R1_TILE_SPHERES (+ one tile)
    // R1_VARIANT_BVH (r1_bvh.cpp): binary tree of boxes over the active spheres.  Node = 4 float4:
    // {m0x m1x m0y m1y} {m0z m1z e0x e1x} {e0y e1y e0z e1z} {A K child0 child1}; child i has
    // centre m_i and half extent e_i, inflated per ray by pad = A |o - bvh_centre|^2 + K.  Child
    // reference: bit 31 clear = inner node index; set = leaf, bits 28..30 number of sphere PAIRS,
    // bits 0..27 first pair of bvh_prims (2 float4 per pair {cx_a cx_b cy_a cy_b} {cz_a cz_b rsq_a
    // rsq_b}) / bvh_ids (2 active indices per pair).  Node 0 is the root.  Behind the last pair of either table stands a sentinel
    // (one pair of radius_sq = -inf; two words 0xFFFFFFFF): a leaf test reads one pair past a leaf that ends on an odd pair (r1_scene.cpp).
    const float4 *bvh_nodes;
    const float4 *bvh_prims;
    const uint32_t *bvh_ids;
    float bvh_centre[3];
    uint32_t bvh_pad_local; // 1: pad = A |m0 + m1 - 2 o|^2 + K (scenes of small spheres, r1_bvh.cpp)
    uint32_t bvh_root_leaf; // 1 / 2: child 0 / 1 of the root is a leaf of <= 2 pairs that every ray tests: the root step of bvh_advance; 0: none
    float bvh_flat_m, bvh_flat_e; // flat trees (r1_bvh.cpp "flat axis", y only): the y slab every box of the node loop lies in; bvh_flat_e < 0: not flat.
                                  // Read once, where the small-scene tree kernels copy the node table into LDS (bvh_advance finds it there)
};

// R1_VARIANT_GRID (r1_grid.cpp): the uniform grid's walk geometry and tables (device memory, R1TraceArgs::grid).  `tab` = [cells + 1] CSR offsets, then the registered
// active sphere indices; 16-bit entries for the small-scene kernel (which copies all of it into LDS), 32-bit for the big one.
struct R1GridArgs
{
    R1GridGeom geom;
    const uint32_t *outliers; // active indices every ray tests before the walk
    uint32_t n_out;
    uint32_t n_start;         // cells + 1: where the sphere ids begin in tab
    const uint32_t *tab;
    uint32_t lds_bytes;       // small-scene kernel: bytes of tab in LDS behind the fallback's traversal stack (multiple of 16)
};

struct R1DeviceCamera
{
    float origin[3], lower_left[3], horizontal[3], vertical[3], u[3], v[3];
    float lens_radius;
};

struct R1TraceArgs
{
    R1DeviceScene scene;
    R1DeviceCamera cam;
    int32_t width, height, spp, max_bounces;
    uint32_t seed;
    float inv_w, inv_h;          // 1.0f / width, 1.0f / height (IEEE divisions done on the host)
    int32_t tile_w, tile_h, tiles_x;
    int32_t shard, num_shards;
    uint32_t n_local_tiles;      // tiles this shard owns (per frame)
    // Frame batches (throughput entry points): ONE launch carries n_frames frames of the same scene, camera and size.  The
    // queue is frame-major — padded tile index j = f * n_local_tiles + (local tile of frame f) — so the persistent waves flow
    // from one frame into the next without draining (a wave's last ~40 iterations run with few live lanes; per frame of
    // 1200x800x10 that is ~8 % of its iterations, per 1/8-frame of an 8-GPU rank ~25 %).  Frame f is seeded seed + f * seed_stride.
    // The batch's numbers sit behind a pointer (null: a single frame) and are fetched with scalar loads where a sample starts:
    // five more kernel arguments cost the tree kernel nine more spilled SGPRs and 2 % of its rate.
    const struct R1BatchArgs *batch;
    // Sample slots are enumerated over PADDED tiles: slot k = (local tile j, pixel in the
    // tile_w x tile_h tile, sample s) = ((j * tile_h + ly) * tile_w + lx) * spp + s.  Slots of
    // pixels outside the image (right/top edge tiles) are void: skipped by the tracer, never
    // written, ignored by the resolve pass.
    uint32_t full;               // tile_w * tile_h * spp slots per local tile
    R1FastDiv div_full, div_spp, div_tw, div_tx; // by full, spp, tile_w, tiles_x
    uint32_t total_samples;      // n_local_tiles * full (queue length)
    uint32_t chunk_min, chunk_max; // samples a wave takes from the queue per atomic (guided: remaining / (2 waves), clamped)
    uint32_t *queue;             // global sample counter(s) (zeroed before the launch); head i at queue + R1_HEAD_WORDS * i (its own 128-byte line; roles: R1_HEAD_*)
    uint32_t nq;                 // 1: one guided queue (chunk_min..chunk_max).  > 1 (latency mode): nq sub-queues of fixed chunks of
                                 // chunk_max slots, chunk c belongs to sub-queue c % nq and a wave only pulls from sub-queue wave % nq:
                                 // a returning atomic on ONE line sustains 88 M/s on this chip (tools/ubench_atomic.hip), too few for
                                 // 6144 waves taking a wave-full at a time
    float4 *samples;             // [total_samples] {r, g, b, bit_cast<float>(rays)}.  PIXEL mode (r1_sample.hpp struct Pixel): the
                                 // queue holds PIXELS (full = tile_w * tile_h, total_samples = padded pixels of the shard) and this
                                 // is the uint8 RGB output the kernel resolves into
    unsigned long long *num_rays; // accumulated color() invocations
    uint32_t *gstack;             // big scenes: attenuation stack [R1_STACK_ENTRIES][grid threads], else null
    unsigned long long *stats;    // diagnostic counters (R1_VARIANT_STATS builds only), else null
    uint32_t bvh_lds_f4;          // tree kernels: float4 of the node table each workgroup copies into LDS behind the traversal stack (0: none)
    int32_t bvh_depth;            // tree kernels: traversal stack entries per thread (dynamic LDS = depth * R1_BLOCK * 4)
    int32_t block_layout;         // PIXEL mode: 1 = `samples` is a dense tile block (pixel index = queue slot), 0 = a row-major image
    float inv_spp;                // PIXEL mode: (float)(1.0f / spp), rayweek1.cpp:765
    // R1_LAND (tiles resolved inside the kernel; the throughput builds of the product kernels)
    uint32_t land_res;            // 1: a landing launch (the throughput builds take no other)
    uint32_t land_tag;            // launch generation << 8, or-ed into every sample record's ray-count word: a record is the launch's own iff its tag matches
    uint32_t *land_cnt;           // [n_frames * n_local_tiles] x R1_LAND_CNT_STRIDE words: samples each tile still lacks; the tracing waves subtract, the wave that
                                  // owes the tile re-arms
    R1LandArgs land;
    const R1GridArgs *grid;       // R1_VARIANT_GRID: the grid's arguments, in device memory (one pointer here: the other kernels' argument block
                                  // keeps its size and layout, and so their code)
    uint32_t coop_lanes;          // small scenes: once the queue is empty, a wave with <= coop_lanes live paths tests each of them
                                  // against ALL spheres, 64 at a time across the wave (cooperative_sweep), instead of walking the tree
                                  // with 60 lanes masked off: the frame's tail is a few 51-bounce chains, and this shortens a step
                                  // of such a chain from ~16 k cycles of dependent node fetches to ~4 k
};

// Dynamic LDS of a workgroup that walks the box tree (variant R1_V_TREE) or the uniform grid (R1_V_GRID), trace and cast kernels alike, their diagnostic
// builds included; 0 for anything else.
// Tree: the traversal stack — bvh_depth entries per thread, 16-bit for small scenes and 32-bit for big ones — then bvh_lds_f4 float4 of the
// node table.  Grid: the tree fallback's stack (32-bit entries), then (small scenes) grid_lds bytes of cell table and ids.  The occupancy
// query and the launch both size by this one function: the grid of a frame is sized for the occupancy its launch has.
static inline size_t r1_walk_lds(int variant, bool big, int32_t bvh_depth, uint32_t bvh_lds_f4, size_t grid_lds)
{
    if (r1_is_tree(variant))
        return (size_t)bvh_depth * R1_BLOCK * (big ? 4 : 2) + (size_t)bvh_lds_f4 * 16;
    if (r1_is_grid(variant))
        return (size_t)bvh_depth * R1_BLOCK * 4 + (big ? 0 : grid_lds);
    return 0;
}

// Wavefront variant (R1_VARIANT_WAVEFRONT): the same path tracer split into
// generate / intersect / shade kernels with the paths and per-level queues in HBM.
struct R1WaveArgs
{
    R1TraceArgs t;        // scene, camera, frame, samples, num_rays; gstack = attenuation stack [entry][path]
    float4 *paths;        // [3][n_paths]: {ox oy oz dx} {dy dz s_scalar s0} {s1 s2 k rays|depth<<8|sp<<16}
    float2 *hits;         // [n_paths] {t, bit_cast<float>(hit index)}
    uint32_t *queue[2];   // path slots alive at the current / next level
    uint32_t *counts;     // [R1_STACK_ENTRIES + 2] queue length per level (zeroed before the frame)
    uint32_t n_paths;     // = total_samples: path slot = sample slot
    int32_t level;        // color() depth this launch works on
};

// The jobs of the query kernels (r1_query_kernels.hip): what a lane does with a caller-supplied ray
enum
{
    R1_JOB_CAST = 0, // ray queries: closest hit or occlusion
    R1_JOB_PATH = 1, // path queries: color()
    R1_JOB_SCATTER = 2, // scatter queries: one color() level
    R1_JOB_FEATURES = 3, // feature frames: the camera's own rays, first-hit albedo, normal and depth summed per pixel
    R1_JOBS = 4
};

// Ray queries (r1_cast_rays / r1_cast_rays_device, r1_query_kernels.hip): caller-supplied rays through the trace kernels' walks.
struct R1CastArgs
{
    R1TraceArgs t;          // what the walks read: scene tables, bvh_lds_f4, bvh_depth, grid (everything else zero)
    const float4 *rays;     // [n][2] {ox oy oz t_max} {dx dy dz -}: the public r1_ray
    void *out;              // mode 0: [n][2] float4 {t, bit_cast<float>(scene index), px, py} {pz, nx, ny, nz}: the public r1_hit; mode 1: [n] bytes
    const uint32_t *active_to_scene; // [n_active] scene index of an active sphere
    uint32_t *cursor;       // the launch's ray cursor (zero before the launch): the waves claim `claim` rays at a time
    uint32_t n;             // <= R1_CAST_LAUNCH_MAX
    uint32_t mode;          // R1_CAST_CLOSEST 0 / R1_CAST_ANY 1
    uint32_t claim;         // rays per claim (a multiple of 64)
};
#define R1_CAST_LAUNCH_MAX (1u << 30) // rays per launch (32-bit ray indices with room for a claim beyond the end); longer arrays take several launches
#define R1_CAST_CURSORS 64u           // cursors of a context, 128 bytes apart, taken in turn: launches in flight on different streams each have their own

// Path queries (r1_trace_rays / r1_trace_rays_device, r1_query_kernels.hip): color() for caller-supplied rays, through the same walks and
// the same shade_level.
struct R1TraceRaysArgs
{
    R1TraceArgs t;          // what the walks and shade_level read: scene tables, bvh_lds_f4, bvh_depth, grid, max_bounces, gstack — the attenuation
                            // stack, [max_bounces][gstride] hit indices (everything else zero)
    const float4 *rays;     // [n][2] {ox oy oz -} {dx dy dz -}: the public r1_ray
    const uint4 *seeds;     // [n] {scalar, lane0, lane1, lane2}: the public r1_sample_seed; null: r1_seed_sample(0, first + i, 0)
    float4 *out;            // [n] {r, g, b, bit_cast<float>(rays)}: the public r1_radiance
    uint32_t *cursor;       // the launch's ray cursor (zero before the launch): the waves claim `claim` rays at a time
    uint32_t n;             // <= R1_CAST_LAUNCH_MAX
    uint32_t claim;         // rays per claim (a multiple of 64)
    uint32_t first;         // index within the call of the launch's ray 0 (seeds == null)
    uint32_t gstride;       // threads of the launch
};

// Scatter queries (r1_scatter_rays / r1_scatter_rays_device, r1_query_kernels.hip): one color() level for caller-supplied rays — the
// path job's load, one walk, the hit arm of shade_level — with the scattered ray, the advanced stream states and a record as the result.
struct R1ScatterArgs
{
    R1TraceArgs t;          // what the walks and the hit arm read: scene tables, bvh_lds_f4, bvh_depth, grid (everything else zero)
    const float4 *rays;     // [n][2] {ox oy oz -} {dx dy dz -}: the public r1_ray
    const uint4 *seeds;     // [n] the public r1_sample_seed; null: r1_seed_sample(0, first + i, 0)
    float4 *rays_out;       // [n][2] {hit point, FLT_MAX} {scattered direction, 0}, or zero; may be `rays` itself
    uint4 *seeds_out;       // [n] the states after the level's draws; may be `seeds` itself
    float4 *out;            // [n][2] {weight rgb, event} {t, scene index, material type, 0}: the public r1_scatter
    const uint32_t *active_to_scene; // [n_active] scene index of an active sphere
    uint32_t *cursor;       // the launch's ray cursor (zero before the launch): the waves claim `claim` rays at a time
    uint32_t n;             // <= R1_CAST_LAUNCH_MAX
    uint32_t claim;         // rays per claim (a multiple of 64)
    uint32_t first;         // index within the call of the launch's ray 0 (seeds == null)
    uint32_t flags;         // R1_SCATTER_UNIT_DIRECTIONS: the directions are used as they are
};

// Feature frames (r1_render_features / r1_render_features_device, r1_query_kernels.hip): an item of the launch is a PIXEL of a
// window of the frame; its lane makes the pixel's samples one after the other with camera_ray (r1_sample.hpp), walks each and sums the first
// hit's albedo, normal and depth in registers.  Nothing is read but the scene tables: the frame is in the arguments.
struct R1FeatureArgs
{
    R1TraceArgs t;          // what the walks read (scene tables, bvh_lds_f4, bvh_depth, grid) and the frame camera_ray reads where a sample starts:
                            // cam, width, spp, seed, inv_w, inv_h, and inv_spp = (float)(1.0f / spp) (everything else zero)
    float4 *out;            // pixel (x, y) of the frame at out + ((y - y0) * stride + (x - x0)) * 2: {albedo rgb, depth} {normal xyz, hits}, the public r1_feature
    uint32_t *cursor;       // the launch's pixel cursor (zero before the launch): the waves claim `claim` pixels at a time
    uint32_t n;             // pixels of the launch, <= R1_CAST_LAUNCH_MAX
    uint32_t claim;         // pixels per claim (a multiple of 64)
    uint32_t first;         // index within the window, row-major, of the launch's pixel 0
    uint32_t x0, y0;        // the window's corner in the frame
    uint32_t win_w;         // the window's width ...
    R1FastDiv div_win_w;    // ... and the division by it (window index < 2^31)
    uint32_t stride;        // pixels between the starts of two rows of the output, >= win_w
};

// r1_camera_rays_kernel (r1_aux_kernels.hip): the primary rays and stream states of samples [first, first + n) of a frame, in r1_render_samples' order
struct R1CameraRaysArgs
{
    R1DeviceCamera cam;     // by value
    float4 *rays;           // [n][2] the public r1_ray: {origin, FLT_MAX} {un-normalised direction, 0}
    uint4 *seeds;           // [n] the states after the camera's draws
    unsigned long long first, n;
    int32_t width, spp;
    uint32_t seed;
    float inv_w, inv_h;     // 1.0f / width, 1.0f / height (IEEE divisions done on the host)
};

// What the launch that closes a frame does for the next one (R1ResolveArgs, R1AccumArgs, R1AdaptArgs), by its first workgroup, after the trace
// kernel: publish the ray count the trace kernel accumulated in the context's counter block, then zero the block — two memset launches per frame less
struct R1FrameClose
{
    const unsigned long long *rays_src; // null: the trace kernel counted into the caller's word itself, nothing to do
    unsigned long long *rays_dst;
    uint32_t *reset;             // R1_COUNTER_BYTES to zero, or null
};

struct R1ResolveArgs
{
    const float4 *samples;
    uint32_t full;
    R1TileGeom geom;
    int32_t spp;
    int32_t shard, num_shards;
    uint32_t n_local_tiles;      // per frame
    float inv_spp;               // (float)(1.0f / spp)
    uint8_t *out;                // row-major image or dense tile block (of frame 0)
    int32_t block_layout;        // 0: row-major width*height*3, 1: dense tile block
    // frame batches: frame f resolves tiles [f * n_local_tiles, (f + 1) * n_local_tiles) of the sample records into
    // out + f * out_stride; its ray count — the sum of its samples' counts, rayweek1.cpp:809-813 — is left as partial sums
    // in frame_rays[(tile of the batch) * gridDim.x + blockIdx.x] (plain stores, no atomics) and added up per frame by
    // r1_batch_counts_kernel into out + f * out_stride + rays_offset (uint64)
    uint32_t n_frames;
    size_t out_stride, rays_offset;
    unsigned long long *frame_rays; // null: single frame, the trace kernel counted
    R1FrameClose close;
};

// Progressive passes (r1_accum_kernel, in place of the resolve launch): adds the pass's records, in sample order, to the context's per-pixel
// fp32 accumulator and (optionally) quantises the sum of samples [0, first_sample + spp) into the row-major image.
struct R1AccumArgs
{
    const float4 *samples;       // the pass's records, [local tile][pass-local sample][pixel of the padded tile]
    float4 *accum;               // [local tile][pixel of the padded tile] {r, g, b, 0}
    uint8_t *out;                // row-major width*height*3 preview, or null: accumulate only
    uint32_t full;               // tile_w * tile_h * spp
    R1TileGeom geom;
    int32_t spp;                 // the pass's samples
    uint32_t n_local_tiles;
    uint32_t fresh;              // 1: the pass starts the accumulation (first_sample == 0): start from 0.0f
    float inv_n;                 // (float)(1.0f / n), n = first_sample + spp
    R1FrameClose close;          // the pass's ray count
};

// Adaptive sampling (r1_render_adaptive): a tile's report on the device, in the layout of the public r1_tile_report
struct R1TileReport
{
    int32_t spp, settled;
    uint32_t err_max, err_sum;
};

// r1_adapt_accum_kernel, in place of r1_accum_kernel after a pass over listed tiles: workgroup j adds the records of list position j to tile
// list[j]'s two accumulators (every sample; the samples of even global index), quantises both as the resolve does, stores the bytes of the
// first into the image and tests the tile: err_max / err_sum over |byte_all - byte_even|, all integer.
struct R1AdaptArgs
{
    const float4 *samples;       // the pass's records, [list position][pass-local sample][pixel of the padded tile]
    const uint32_t *list;        // [n_listed] tiles of the frame
    float4 *all, *even;          // [tile of the frame][pixel of the padded tile] {r, g, b, 0}
    uint8_t *out;                // row-major width*height*3
    R1TileReport *report;        // [tile of the frame]
    R1TileGeom geom;
    int32_t spp;                 // the pass's samples
    uint32_t n_listed;
    uint32_t first_sample;       // global index of the pass's first sample (0: the accumulators start from 0.0f)
    float inv_all, inv_even;     // (float)(1.0f / n), (float)(1.0f / ((n + 1) / 2)), n = first_sample + spp
    int32_t max_delta;           // the rule: err_max <= max_delta (-1: never) ...
    uint32_t mean_delta_q8;      // ... and err_sum * 256 <= mean_delta_q8 * 3 * (pixels of the tile inside the image)
    R1FrameClose close;          // the pass's ray count
};

// Linear frames.  r1_resolve_linear_kernel, one more launch behind a whole frame's trace and whatever closes it: the sums
// r1_resolve_kernel takes over the records the trace left, times inv_spp, stored as fp32 — the value the byte is quantised from.
struct R1LinearArgs
{
    const float4 *samples;       // [tile][sample][pixel of the padded tile]; x, y, z alone are used (a landing launch tags the w word)
    float *out;                  // row-major width*height*3 floats
    uint32_t full;               // tile_w * tile_h * spp
    R1TileGeom geom;
    int32_t spp;
    uint32_t n_tiles;
    float inv_spp;               // (float)(1.0f / spp)
};

// Variance frames.  r1_resolve_moments_kernel, launched INSTEAD of r1_resolve_linear_kernel: the same walk and the same
// sums, then a second walk over the pixel's records for the squared deviations from the stored mean; it stores the linear value and the
// pixel's r1_moment record.
struct R1MomentsArgs
{
    const float4 *samples;       // as R1LinearArgs::samples
    float *out;                  // row-major width*height*3 floats: r1_resolve_linear_kernel's values
    uint4 *moments;              // row-major width*height records {var r, var g, var b as fp32 bits, spp}, 16-byte aligned
    uint32_t full;               // tile_w * tile_h * spp
    R1TileGeom geom;
    int32_t spp;
    uint32_t n_tiles;
    float inv_spp;               // (float)(1.0f / spp)
    float inv_nn;                // spp > 1: 1.0f / ((float)spp * (float)(spp - 1)); unused at spp == 1, where every var is +0.0f
};

// Region renders (r1_resolve_region_kernel): the records of a launch over the REGION's tiles (geom: a frame of the region's size),
// summed as the resolve sums them, into a window whose rows lie `stride` pixels apart: bytes, floats or both.
struct R1RegionArgs
{
    const float4 *samples;       // [tile of the region][sample][pixel of the padded tile]; x, y, z alone are used
    uint8_t *out_u8;             // pixel (x, y) of the region at out_u8 + (y * stride + x) * 3, or null
    float *out_f32;              // ... at out_f32 + (y * stride + x) * 3, or null
    uint32_t full;               // tile_w * tile_h * spp
    R1TileGeom geom;             // the region's own tiling: width and height are the region's
    int32_t spp;
    uint32_t n_tiles;
    uint32_t stride;             // pixels between the starts of two rows of the output, >= geom.width
    float inv_spp;               // (float)(1.0f / spp)
    R1FrameClose close;
};

// r1_accum_linear_kernel: the read-out of the accumulators of r1_render_pass and r1_render_adaptive, the padded [tile][pixel] layout to
// row-major, times (float)(1.0f / n): n uniform (report == null, inv_n) or the tile's own (report[tile].spp).
struct R1ReadoutArgs
{
    const float4 *accum;         // [tile][pixel of the padded tile] {r, g, b, 0}
    const R1TileReport *report;  // [tile], or null
    float *out;                  // row-major width*height*3 floats
    R1TileGeom geom;
    uint32_t n_tiles;
    float inv_n;                 // report == null: (float)(1.0f / n)
};

// r1_land_arm_kernel: the countdowns and per-frame accumulators of a landing launch of n_frames frames of n_local_tiles tiles (r1_land_area)
struct R1LandArmArgs
{
    uint32_t *tile_cnt;
    unsigned long long *frame_rays;
    uint32_t *frame_left;
    uint32_t n_frames, n_local_tiles;
    R1TileGeom geom;
    int32_t spp, shard, num_shards;
};

// r1_assemble_kernel.  blocks: gathered tile blocks or records; per frame f (0 .. n_frames - 1): shard sh's block at blocks + f * frame_in + sh *
// shard_stride, image at rgb + f * frame_out.  want_total: the shards' uint64 counts at (block start + total_offset) are summed into the uint64 at
// (the frame's image + total_out).
struct R1AssembleArgs
{
    const uint8_t *blocks;
    uint8_t *rgb;
    R1TileGeom geom;
    int32_t num_shards, n_frames;
    size_t shard_stride, frame_in, frame_out, total_offset;
    long long total_out;
    int32_t want_total;
};

#endif
