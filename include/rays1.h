/* rays1.h — C-ABI of librays1.so, the MI355X-native replacement for the per-pixel /
 * per-sample path-tracing hot path of montib/rays1bench `src/step13`.
 *
 * The reference has no FFI or plugin interface: its boundary for this path is three
 * scene builders and one function in a single translation unit
 *     Scene *create_small_scene()/create_medium_scene()/create_large_scene()
 *                                      src/step13/rayweek1.cpp:552 / :582 / :654
 *     RESULT benchmark(Scene*, Pix*, bool write_tga, const char *scene_name)
 *                                      src/step13/rayweek1.cpp:845
 * This header is what a maintainer would bind from that function (INTEGRATION.md shows
 * the patch): plain C, POD structs, caller-owned memory, integer return codes, no
 * exceptions, no C++/torch types.  `rays1bench_amd/csrc/rayweek1_hip.cpp` is the
 * drop-in host program built on top of it (same entry points, CLI and output files).
 *
 * Threading: one call at a time per context (the reference calls benchmark() serially
 * from main, rayweek1.cpp:969-984).  All functions return R1_OK (0) or a negative
 * R1_E* code; r1_last_error() describes the last failure on the calling thread.
 * There is NO CPU fallback: without a usable HIP device every compute entry point
 * fails with R1_ENODEVICE.
 *
 * Environment variables.  None.  The shipped library never reads the environment: what it computes and how it
 * launches depends on its arguments only.  (A separate build with -DR1_TUNING, `make -C rays1bench_amd/csrc tuning`
 * -> lib/librays1_tuning.so, reads R1_* launch-shape and index-layout knobs for the measurements under tools/ and
 * profiles/; it is loaded explicitly by those scripts, never by the product or its tests, and every knob only chooses
 * among forms that produce the same pixels and ray counts.)
 */
#ifndef RAYS1_H
#define RAYS1_H

#include <stddef.h>
#include <stdint.h>

#include "rays1_seed.h" /* r1_sample_seed: the four stream states of a path (path queries) */

#ifdef __cplusplus
extern "C" {
#endif

#define R1_ABI_VERSION 4

enum
{
    R1_OK = 0,
    R1_EINVAL = -1,    /* bad argument (null pointer, non-positive size, bad sharding) */
    R1_ENODEVICE = -2, /* no HIP device / HIP runtime unusable                        */
    R1_EHIP = -3,      /* a HIP call failed; see r1_last_error()                      */
    R1_ENOMEM = -4,    /* device or host allocation failed                            */
    R1_ELIMIT = -5     /* scene / image exceeds a documented limit                    */
};

/* Material classes of the reference (rayweek1.cpp:396-511), flattened. */
enum
{
    R1_MAT_LAMBERTIAN = 0, /* albedo                              rayweek1.cpp:396-412 */
    R1_MAT_METAL = 1,      /* albedo, param = fuzz (<= 1)         rayweek1.cpp:419-436 */
    R1_MAT_DIELECTRIC = 2, /* param = refraction index            rayweek1.cpp:461-511 */
    R1_MAT_NONE = 255      /* placeholder sphere (material == nullptr, rayweek1.cpp:574-576) */
};

/* Mirror of SphereSOA::InstanceData (src/step13/soa_sphere.h:38-53) with the
 * polymorphic `Material*` column replaced by a flat material table.  `count` includes
 * the reference's padding placeholders (centre 1e9, inv_radius 0); spheres with
 * inv_radius == 0 (placeholders AND non-positive radii, soa_sphere.cpp:81) are never
 * hit, exactly as rayweek1.cpp:291 (and so are spheres with a non-finite centre or
 * radius_sq, which the reference's arithmetic can never hit).  `radius_sq[i]` and
 * `inv_radius[i]` must belong to the same radius, as SphereSOA::add stores them
 * (soa_sphere.cpp:70-85).  All arrays are host memory, length `count`, owned by the
 * caller and only read during the call they are passed to. */
typedef struct r1_scene
{
    uint32_t count;
    const float *center_x;
    const float *center_y;
    const float *center_z;
    const float *radius_sq;
    const float *inv_radius;
    const uint8_t *mat_type; /* R1_MAT_* */
    const float *albedo_r;
    const float *albedo_g;
    const float *albedo_b;
    const float *mat_param; /* fuzz (metal) or refraction index (dielectric) */
} r1_scene;

/* Mirror of struct Camera after Camera::init (rayweek1.cpp:364-395). */
typedef struct r1_camera
{
    float origin[3];
    float lower_left[3];
    float horizontal[3];
    float vertical[3];
    float u[3];
    float v[3];
    float w[3];
    float lens_radius;
} r1_camera;

/* Runtime replacements for the reference's compile-time configuration
 * (src/common/common.h:19-28: SCREEN_W, SCREEN_H, NUM_SAMPLES_PER_PIXEL, MAX_BOUNCES)
 * plus the build-defined seeding contract (include/rays1_seed.h) and sharding.
 * Limits (R1_ELIMIT): width, height <= 65535 and width * height * spp < 2^31; per launch, the padded sample slots
 * (tiles of the launch * tile_w * tile_h * spp, times the frames of a batch) < 2^31.  Any tile size within them is
 * rendered, a tile whose sample records span more than 4 GiB included. */
typedef struct r1_params
{
    int32_t width;       /* SCREEN_W                                              */
    int32_t height;      /* SCREEN_H                                              */
    int32_t spp;         /* NUM_SAMPLES_PER_PIXEL                                 */
    int32_t max_bounces; /* MAX_BOUNCES (reference: 50); 1..R1_MAX_BOUNCES_LIMIT  */
    uint32_t seed;       /* frame seed of the per-sample seeding contract         */
    int32_t tile_w;      /* tile size for multi-device sharding (reference: 32)   */
    int32_t tile_h;
    int32_t shard;       /* this device renders tiles t with t % num_shards == shard */
    int32_t num_shards;  /* 1 = whole frame                                       */
    int32_t variant;     /* R1_VARIANT_*; 0 = default kernel                      */
} r1_params;

#define R1_MAX_BOUNCES_LIMIT 51

enum
{
    R1_VARIANT_DEFAULT = 0,   /* BVH for every scene (a property of the build: what a context launches depends on its
                                 arguments only; same pixels as every other variant; r1_launch_info.kernel says which ran) */
    R1_VARIANT_REFERENCE = 1, /* pass 1 in the reference's exact arithmetic (rayweek1.cpp:190-202),
                                 no prefilter; slower, used to cross-check the default       */
    R1_VARIANT_PREFILTER = 2, /* the exhaustive sweep (every ray against every sphere, as Hitable::hit does,
                                 rayweek1.cpp:182-322): conservative grouped prefilter + exact re-test */
    R1_VARIANT_STATS = 3,     /* PREFILTER plus in-kernel phase/utilisation counters (diagnostic; r1_last_stats) */
    R1_VARIANT_BVH = 4,       /* optional spatial index (the reference has none, README.md:163): a conservative
                                 box tree chooses the spheres given to the reference's per-sphere test; results
                                 are bit-identical to the exhaustive sweeps   */
    R1_VARIANT_BVH_STATS = 5, /* BVH plus traversal counters (diagnostic; r1_last_stats slots [2] node-loop trips,
                                 [3] leaf-loop trips, [5] sphere-pair tests, [9] node visits, [14] leaf trips x lanes, [15] root steps: the root's leaf and
                                 the box of its other child tested outside the walk's loops) */
    R1_VARIANT_WAVEFRONT = 6, /* the same tracer as separate generate / intersect / shade kernels with the paths
                                 and per-level queues in HBM; a comparison build: same pixels,
                                 slower than the megakernel; frames of <= 2^24 sample slots       */
    R1_VARIANT_GRID = 7,      /* optional uniform grid: outliers tested by every ray, then
                                 a cell walk presents the registered spheres to the reference's per-sphere test; rays
                                 whose origin is too far for the grid's pad take the tree walk (fallback).  Built on the
                                 first render that asks for it after r1_set_scene; bit-identical to the exhaustive sweeps */
    R1_VARIANT_GRID_STATS = 8 /* GRID plus walk counters (diagnostic; r1_last_stats slots [2] wave trips of the cell-walk
                                 loop, [5] sphere tests summed over lanes (outliers and cells), [9] cell steps summed over
                                 lanes, [14] lanes that took the fallback, [15] outlier tests summed over lanes) */
};

typedef struct r1_context r1_context; /* opaque: device, stream, events, workspace */

/* ---- lifetime ------------------------------------------------------------------- */

/* Library ABI version (R1_ABI_VERSION of the build). */
int r1_abi_version(void);

/* Creates a context on HIP device `device` (stream, timing events, scene + workspace
 * buffers are cached in it so that the `-n` runs of rayweek1.cpp:969-984 do not pay
 * context creation inside the timed region).  *out is NULL on failure. */
int r1_create(int device, r1_context **out);
void r1_destroy(r1_context *ctx);

/* Text of the last error on this thread ("" if none). Never NULL. */
const char *r1_last_error(void);

/* Number of visible HIP devices, or a negative R1_E* code. */
int r1_device_count(void);

/* ---- the hot path ---------------------------------------------------------------- */

/* Uploads (and caches) the scene + camera in the context: builds the device-side
 * sphere table and material table.  Replaces what benchmark() receives as `Scene*`
 * (rayweek1.cpp:845, :851). */
int r1_set_scene(r1_context *ctx, const r1_scene *scene, const r1_camera *camera);

/* Replaces the context's camera and nothing else: no table is built or uploaded and nothing is waited for (r1_set_scene with a
 * camera that differs in one bit rebuilds the sphere groups and the box tree and drops the uniform grid).  The camera travels by
 * value in every launch's arguments, so launches already enqueued keep the camera they were enqueued with.  Needs a scene
 * (R1_EINVAL before the first r1_set_scene).  Ends a progressive accumulation as r1_set_scene does (the next r1_render_pass with
 * first_sample > 0 returns R1_EINVAL).  r1_set_scene(the same arrays, this camera) afterwards still finds everything current. */
int r1_set_camera(r1_context *ctx, const r1_camera *camera);

/* ---- moving spheres ---- */

/* New centres for the spheres [first, first + count) of the scene: SCENE indices into the arrays given to the last r1_set_scene,
 * placeholders counted; entries of spheres that are not active (inv_radius == 0, or non-finite at r1_set_scene) are ignored.  Radii and
 * materials stay (r1_update_spheres below changes them too); the active set and the active order do not change: only r1_set_scene changes
 * them.  x, y, z are host memory, `count`
 * floats each, read during the call only (through a page-locked staging buffer of the context).  The centres are written in place
 * into the tables the box-tree kernels read and the tree is REFITTED on the device: its topology stays, every box is recomputed
 * bottom-up from the new centres in the builder's own arithmetic (r1_bvh_fill.h), one small launch per height of the tree.  Leaves
 * apply the reference's own per-sphere test, ties go to the lowest active index and a box only has to be conservative, so every render
 * and every ray query afterwards gives bit-identical pixels, ray counts and hit records to a fresh context after r1_set_scene with the
 * moved arrays; a tree whose topology has gone stale only visits more nodes (what tools/update_bench.py measures of
 * that, and so the point at which r1_set_scene pays).
 * Everything is enqueued on `hip_stream` (a hipStream_t; NULL = the context's stream) and nothing is waited for but the previous
 * update's reading of the staging buffer: work enqueued earlier on that stream sees the old scene, work enqueued later the new one.
 * What keeps working: renders with R1_VARIANT_DEFAULT, _BVH, _BVH_STATS and _REFERENCE (which reads only the sphere table the update
 * rewrites), r1_cast_rays* with DEFAULT, BVH and REFERENCE.  What stops until the next r1_set_scene: the sphere groups of the
 * exhaustive sweep and the uniform grid are NOT refitted, so R1_VARIANT_PREFILTER, _STATS, _WAVEFRONT, _GRID and _GRID_STATS renders
 * and a GRID cast return R1_EINVAL (r1_last_error says that the scene has moved and that r1_set_scene rebuilds them).  The tree's flat
 * y slab (r1_bvh_info.flat_axis) is dropped: the kernels take their generic loop.
 * R1_EINVAL before the first r1_set_scene, for first + count beyond the scene's count, for NULL pointers with count > 0, and for a
 * non-finite new centre of an ACTIVE sphere (nothing is changed or enqueued then); count == 0 is R1_OK and touches nothing.  An update
 * ends a progressive accumulation as r1_set_camera does and leaves r1_last_launch_info / r1_last_timing alone.  The context's host
 * copies of the centres follow, but after ANY update r1_set_scene rebuilds everything, whatever arrays it is given (the original ones
 * included), and re-enables every variant.
 * One update at a time per context: an update rewrites the context's tables in place through ONE scratch area and changes the context's
 * host state (the refused variants, the dropped slab) when it is ENQUEUED, not when it runs.  Updates of one context therefore go to
 * one stream, or the caller orders them; renders and casts that must see a given state go to that stream too, or are ordered against it
 * by the caller.  r1_set_scene waits for the context's OWN stream only and may reallocate every table: an update or a frame still in
 * flight on another stream must have finished before it is called.  One thread at a time per context, as for every entry point.
 * There is no r1_multi form: more than one device has never run on hardware here. */
int r1_update_centers(r1_context *ctx, uint32_t first, uint32_t count, const float *x, const float *y, const float *z, void *hip_stream);

/* The same from DEVICE memory: three device pointers to `count` floats each, 4-byte aligned (R1_EINVAL otherwise), read by a launch on
 * `hip_stream`; waits for nothing.  The host cannot see the values: a sphere whose new centre is non-finite can never be hit (see
 * r1_scene), the refit leaves it out of every box, and the pixels equal r1_set_scene with the same arrays, where that sphere is
 * dropped as inactive.  The context's host copies of the centres are NOT updated. */
int r1_update_centers_device(r1_context *ctx, uint32_t first, uint32_t count, const void *d_x, const void *d_y, const void *d_z, void *hip_stream);

/* ---- sphere updates: radii and materials too ---- */

/* New values for the spheres [first, first + count) of the scene, in three GROUPS: centres (center_x, _y, _z), radii (radius_sq, inv_radius: of
 * the same radius, as in r1_scene) and materials (mat_type with albedo_r, _g, _b and mat_param).  Every group: all of its pointers or none
 * (NULL = this property stays).  Arrays of `count` entries each; entry i belongs to scene index first + i. */
typedef struct r1_sphere_update
{
    const float *center_x, *center_y, *center_z;
    const float *radius_sq, *inv_radius;
    const uint8_t *mat_type;
    const float *albedo_r, *albedo_g, *albedo_b, *mat_param;
} r1_sphere_update;

/* r1_update_centers' contract for every property of a sphere but its being active: afterwards every render, ray query and path query through
 * the context is bit-identical — pixels, ray counts, sample records, hit records — to a fresh context after r1_set_scene with the edited
 * arrays.  Indices, ignored entries of spheres that are not active, the staging of the host arrays, the stream order (everything is enqueued
 * on `hip_stream`, nothing is waited for but the previous update's reading of the staging buffer), "one update at a time per context" and the
 * end of a progressive accumulation are r1_update_centers' own; the active set and the active order never change; there is no r1_multi form.
 *   centres    r1_update_centers' rules (a non-finite new centre of an active sphere: R1_EINVAL).
 *   radii      the device rewrites the radius in every table the box-tree kernels and the shading read and REFITS the tree (with the centres,
 *              if both are given: one refit).  The context is then in the state of a centre update: the flat y slab is dropped, PREFILTER,
 *              STATS, WAVEFRONT, GRID, GRID_STATS and a GRID cast return R1_EINVAL ("the scene has moved") until the next r1_set_scene (the
 *              grid: or until r1_regrid, below).  An
 *              active sphere whose new pair would make it inactive (inv_radius 0 or NaN, radius_sq not finite) is R1_EINVAL; a negative
 *              inv_radius and pairs that disagree are accepted as r1_set_scene accepts them.
 *   materials  the device rewrites the sphere's albedo and material row.  Nothing else changes: no refit, every variant and the grid stay
 *              valid, the flat slab stays.  mat_type > R1_MAT_DIELECTRIC for an active sphere is R1_EINVAL.
 * R1_EINVAL before anything is changed or enqueued: before the first r1_set_scene, first + count beyond the scene, then (count == 0 is R1_OK
 * and touches nothing) u == NULL, a group given in part, every group NULL, and the value rules above.  The context's host copies follow.
 * After ANY update r1_set_scene, whatever arrays it is given, leaves the context equal to a fresh one. */
int r1_update_spheres(r1_context *ctx, uint32_t first, uint32_t count, const r1_sphere_update *u, void *hip_stream);

/* The same from DEVICE memory: the float arrays 4-byte aligned (R1_EINVAL otherwise; mat_type needs no alignment), read by launches on
 * `hip_stream`; waits for nothing.  The host cannot see the values: a radius pair that would make a sphere inactive leaves it never hittable
 * (its pixels equal r1_set_scene with those arrays, where the sphere is dropped), an entry whose mat_type is no material is skipped (the
 * sphere keeps its material), a non-finite centre is r1_update_centers_device's.  The context's host copies are NOT updated. */
int r1_update_spheres_device(r1_context *ctx, uint32_t first, uint32_t count, const r1_sphere_update *u, void *hip_stream);

/* ---- re-sort: the spheres re-dealt into the tree's leaves ---- */

/* A refit keeps the tree's topology, so the tree goes stale as the spheres wander.  This call keeps the topology too —
 * every table shape, every kernel — and re-deals the spheres into the leaf slots on the device, by a rank split along the widest axis of
 * the centres at every inner node (csrc/r1_bvh_sort.h has the rule; leaves the builder made of outliers, the ground and the big balls of
 * the reference's scenes, keep their spheres), from the centres the device holds; then it refits.  Enqueued on `hip_stream` (NULL: the
 * context's stream); waits for nothing.  Afterwards every render, ray query and path query is bit-identical — pixels, ray counts, hit
 * records, sample records — to a fresh context after r1_set_scene with the context's current spheres: the updates' own contract.
 * It counts as an update for the context's state: the flat y slab is dropped; PREFILTER, STATS, WAVEFRONT, GRID, GRID_STATS and a GRID
 * cast return R1_EINVAL ("the scene has moved") until the next r1_set_scene; a progressive accumulation ends; "one update at a time per
 * context" holds; r1_last_launch_info / r1_last_timing are left alone.  Valid before any update too.  R1_EINVAL before the first
 * r1_set_scene.  A tree without a movable sphere: R1_OK, nothing is changed or enqueued, the state stays.  A pure function of the
 * centres, the active order and the topology: a second call with no update in between changes no byte.  r1_update_centers* and
 * r1_update_spheres* keep working afterwards.  There is no r1_multi form. */
int r1_resort_spheres(r1_context *ctx, void *hip_stream);

/* Diagnostic, synchronous (as r1_bvh_download): the tree's leaf slots as the device holds them, as scene indices (0xFFFFFFFF: the empty
 * partner of an odd sphere) — what r1_bvh_describe returns in ids_out before any re-sort, r1_bvh_resort_describe after one.  *n receives
 * the number of slots; ids_out may be NULL (the count alone), else ids_cap >= *n (R1_ELIMIT otherwise). */
int r1_bvh_ids_download(r1_context *ctx, uint32_t *ids_out, size_t ids_cap, size_t *n);

/* Diagnostic, synchronous (waits for the context's stream, as r1_bvh_download): the device's per-sphere rows of the n active spheres, in
 * active order: exact [n][4] {cx cy cz radius_sq}, shade [n][4] {inv_radius, albedo r g b}, mat [n][4] {type, the bits of param, of
 * 1 / ref_idx and of schlick's r0}, radii [n][2] {bound radius, test radius} (fp64).  Each may be NULL; all NULL: *n_active alone.
 * R1_ELIMIT if cap_active (entries of each given array, in spheres) < n. */
int r1_tables_download(r1_context *ctx, float *exact, float *shade, uint32_t *mat, double *radii, size_t cap_active, size_t *n_active);

/* Renders the frame (or this shard's tiles of it) and returns everything on the host.
 * Replaces TileRenderScheduler::run + render_tile (rayweek1.cpp:785-842, :722-782).
 *   rgb_out      width*height*3 bytes, row-major, row 0 = bottom row, Pix{r,g,b}
 *                (common.h:80-83, rayweek1.cpp:750); with num_shards > 1 only this
 *                shard's tiles are written, other bytes are left untouched.
 *   num_rays_out number of color() invocations (rayweek1.cpp:517) of this shard.
 *   device_seconds_out  (optional) GPU time of the kernels, from HIP events.
 * A trace launch that lands its tiles itself (from this call: the big-scene kernels) resolves each 32 x 32 tile as soon as its
 * samples are complete and, where rgb_out is page-locked memory (r1_host_alloc), stores it straight into rgb_out.  Every other frame is trace +
 * resolve + ONE copy of the finished image, which page-locked memory only makes faster. */
int r1_render(r1_context *ctx, const r1_params *params, uint8_t *rgb_out, uint64_t *num_rays_out,
              double *device_seconds_out);

/* Same, plus the per-sample results the resolve pass sums: samples_out receives
 * width*height*spp records of 4 floats {r, g, b, bit_cast<float>(uint32 rays)} in the
 * order ((y*width + x)*spp + s).  For parity tests; whole frame only (num_shards 1). */
int r1_render_samples(r1_context *ctx, const r1_params *params, uint8_t *rgb_out, uint64_t *num_rays_out,
                      float *samples_out);

/* Progressive rendering: traces samples [first_sample, first_sample + params->spp) of every pixel and adds them,
 * in sample order, to the context's per-pixel fp32 accumulator.  A sample's streams depend on (seed, pixel, sample
 * index) only (rays1_seed.h), and the resolve sums a pixel's samples in sample order with plain fp32 adds, so the
 * accumulator then holds exactly what r1_render sums for spp = first_sample + params->spp.
 *   first_sample == 0  starts a new accumulation (any earlier one is discarded).
 *   first_sample > 0   continues the context's accumulation: first_sample must equal the samples accumulated so far,
 *                      every field of *params but spp must equal the call that started it (size, seed, max_bounces,
 *                      tile size, shard fields, variant), and no r1_set_scene may have happened since.  Otherwise
 *                      the call returns R1_EINVAL and leaves the accumulation untouched.  A call that fails after it
 *                      has enqueued work invalidates it: only first_sample == 0 is accepted next.
 *   params->spp        this pass's samples, bounded per pass by the limits of r1_render (2^31 samples and 2^31
 *                      padded sample slots); first_sample + spp <= INT32_MAX; nothing else bounds the total.
 *   rgb_out            (may be NULL: accumulate only) the row-major image of samples [0, first_sample + spp),
 *                      byte-identical to r1_render with that spp and the same other fields wherever that call is
 *                      within its limits.
 *   num_rays_out       (may be NULL) the cumulative color() count, equal to that r1_render's.
 * Whole frames only (num_shards == 1).  Variants DEFAULT, REFERENCE, PREFILTER, BVH and GRID, small and big scenes;
 * the diagnostic variants and WAVEFRONT return R1_EINVAL.  PIXEL mode (r1_set_pixel_mode) does not apply.
 * Synchronous, like r1_render; r1_last_launch_info and r1_last_timing describe the last pass.  r1_render,
 * r1_render_async and r1_render_batch_async may be called on the context between passes without disturbing the
 * accumulation.  Each pass keeps 16 bytes per sample of that pass on the device (as r1_render does per frame) and
 * the accumulator 16 bytes per pixel. */
int r1_render_pass(r1_context *ctx, const r1_params *params, int32_t first_sample, uint8_t *rgb_out, uint64_t *num_rays_out);

/* Adaptive sampling: the frame is rendered in passes, and a tile stops sampling once its pixels have settled.
 *
 * The rule (integer, exact).  Per pixel two fp32 sums, both taken in sample order with plain adds: `all` over the samples
 * [0, n) and `even` over those of even index in [0, n) — (n + 1) / 2 of them.  Both are quantised as r1_render quantises a
 * pixel (times (float)(1.0f / count), correctly rounded square root, (uint8)(int)(c * 255.99f)).  Over a tile's pixels inside
 * the image and the three channels:
 *     err_max = max |byte_all - byte_even|        err_sum = sum |byte_all - byte_even|
 *     settled = err_max <= max_delta  and  err_sum * 256 <= mean_delta_q8 * 3 * (pixels of the tile inside the image)
 * (64-bit products).  max_delta = -1 can never hold: every tile runs to the cap.  max_delta = 255 with mean_delta_q8 = 65280
 * always holds: every tile stops after the first pass.
 *
 * The schedule.  params->spp is the cap (a frame of that spp must be within the limits of r1_render's params).  n_0 = min(min_spp, spp), n_{k+1} = min(n_k + pass_spp, spp).  Pass k traces the
 * samples [n_{k-1}, n_k) of every tile still active; then every active tile is tested at n_k, and one that is settled or has
 * reached the cap leaves.  The test is made at the cap too. */
typedef struct r1_adaptive
{
    int32_t min_spp;        /* >= 1: samples every tile gets before its first test              */
    int32_t pass_spp;       /* >= 1: samples per further pass                                   */
    int32_t max_delta;      /* -1 .. 255                                                        */
    int32_t mean_delta_q8;  /* 0 .. 65280: mean |byte_all - byte_even| allowed, in 1/256 bytes  */
} r1_adaptive;

typedef struct r1_tile_report /* one per tile, tile t = ty * tiles_x + tx */
{
    int32_t spp;            /* samples of each of its pixels in the image                        */
    int32_t settled;        /* 1: the rule held at `spp` (tested at the cap too); 0: it ran into the cap unsettled */
    uint32_t err_max, err_sum; /* at its last test                                              */
} r1_tile_report;

typedef struct r1_adaptive_result
{
    uint64_t samples;       /* pixel-samples traced: sum over tiles of spp * pixels inside the image */
    int32_t passes, tiles, tiles_settled, reserved;
} r1_adaptive_result;

/* Pure arithmetic, no device: validates *opt against *params exactly as r1_render_adaptive does and writes the cumulative
 * sample counts n_0 < n_1 < ... = params->spp to n_out[0, *count).  R1_EINVAL, with the offending field's name in
 * r1_last_error, for options out of range, num_shards != 1, a variant r1_render_adaptive refuses, or cap < the number of
 * passes (*count is set then too); R1_ELIMIT where a pass would exceed the per-launch limits of r1_render_pass, or a tile has
 * more than 2^22 pixels.  n_out may be NULL (count only), count may be NULL. */
int r1_adaptive_schedule(const r1_params *params, const r1_adaptive *opt, int32_t *n_out, size_t cap, size_t *count);

/* Renders the frame by that rule and schedule.  Synchronous.  The contract:
 *   1. every tile's pixels in rgb_out (row-major, width*height*3) equal r1_render with spp = tiles_out[t].spp and otherwise
 *      equal params, cropped to the tile, byte for byte (a sample's streams depend on (seed, pixel, sample index) only);
 *   2. *num_rays_out (may be NULL) is the number of color() calls of exactly those samples;
 *   3. tiles_out (may be NULL; one entry per tile of the frame) is what the rule gives on those samples: it does not depend
 *      on the kernel variant, the order of the tiles in a launch or the machine.
 * result_out may be NULL.  Whole frames only (num_shards == 1).  Variants DEFAULT, PREFILTER, BVH and GRID, small and big
 * scenes; REFERENCE, the diagnostic variants and WAVEFRONT return R1_EINVAL.  Per pass the limits of r1_render_pass apply
 * (R1_ELIMIT).  The call discards a progressive accumulation of the context as r1_render_pass(first_sample = 0) does and
 * leaves none behind (r1_render_pass with first_sample > 0 returns R1_EINVAL afterwards); r1_render, r1_render_async,
 * batches and paths on the same context are undisturbed before and after.  r1_last_launch_info and r1_last_timing describe
 * the last pass.  Device memory: 16 bytes per sample of the longest pass, 32 bytes per pixel of the padded tiles. */
int r1_render_adaptive(r1_context *ctx, const r1_params *params, const r1_adaptive *opt, uint8_t *rgb_out, uint64_t *num_rays_out,
                       r1_tile_report *tiles_out, r1_adaptive_result *result_out);

/* ---- linear frames: fp32 radiance per pixel beside the 8-bit image ---- */

/* The value.  For pixel (x, y), channel c and n samples: S = 0.0f, then S += radiance_c(sample s) for s = 0 .. n - 1 — plain fp32 adds
 * in sample order, rayweek1.cpp:762, what the resolve launch does — and L = S * (float)(1.0f / n), one fp32 multiply, rayweek1.cpp:765.
 * L is what the byte image is quantised from: (uint8)(int)(sqrtf(L) * 255.99f) equals r1_render's byte, for every pixel of every frame
 * (r1_quantise_linear below does that step on the host).  A linear frame has the layout of rgb_out of r1_render with floats for bytes:
 * row-major, row 0 = bottom row, three floats per pixel, width * height * 12 bytes.  Whole frames only: num_shards != 1 is R1_EINVAL in
 * every call below.  No trace kernel differs: a frame runs the launches it always ran — its byte image goes into the context's device
 * buffer — and one more launch sums the sample records they left (16 bytes per sample on the device, as for r1_render). */

/* r1_render with a linear frame for the byte image: synchronous, every variant r1_render accepts, the same ray count, device_seconds_out
 * with the extra launch in it.  Page-locked rgb_out (r1_host_alloc) is written by that launch itself, any other memory by one copy.
 * Leaves a progressive accumulation alone, as r1_render does. */
int r1_render_linear(r1_context *ctx, const r1_params *params, float *rgb_out, uint64_t *num_rays_out, double *device_seconds_out);

/* r1_render_async with a linear frame: r1_render_async's rules — the throughput kernels, enqueued on `hip_stream` (NULL = the context's
 * stream), nothing is waited for, one frame per context at a time, rgb_out and num_rays_out given together or both NULL (the frame then
 * stays in the context's device buffers).  Page-locked memory (r1_host_alloc; num_rays_out 8-byte aligned) is written by the launches
 * themselves, pageable memory by copies enqueued behind them; both are valid once the stream is idle.  PIXEL mode (r1_set_pixel_mode)
 * keeps no sample records, so this call does not use it, whatever the switch says: the frame runs the record-keeping throughput kernels. */
int r1_render_linear_async(r1_context *ctx, const r1_params *params, float *rgb_out, uint64_t *num_rays_out, void *hip_stream);

/* The same frame into DEVICE memory, for a tensor that stays on the GPU: d_rgb_f32 receives width * height * 3 floats (4-byte aligned),
 * d_num_rays one uint64 (8-byte aligned); R1_EINVAL otherwise, and nothing is enqueued.  Everything is enqueued on `hip_stream`, nothing
 * is waited for.  PIXEL mode does not apply, as above. */
int r1_render_linear_device(r1_context *ctx, const r1_params *params, void *d_rgb_f32, void *d_num_rays, void *hip_stream);

/* The context's progressive accumulation (r1_render_pass) as a linear frame of the samples it holds; *samples_out (may be NULL) receives
 * that count.  Synchronous.  R1_EINVAL while there is no valid accumulation (none started, or ended by r1_set_scene, r1_set_camera, an
 * update or r1_render_adaptive).  It changes nothing: r1_render_pass(first_sample = that count) continues as before, r1_last_launch_info
 * and r1_last_timing keep describing the last render. */
int r1_pass_linear(r1_context *ctx, float *rgb_out, int32_t *samples_out);

/* r1_render_adaptive with a linear frame: the same schedule, the same rule — which is defined on bytes —, the same reports, result and
 * ray count; every tile's pixels equal r1_render_linear with spp = tiles_out[t].spp, cropped to the tile, bit for bit. */
int r1_render_adaptive_linear(r1_context *ctx, const r1_params *params, const r1_adaptive *opt, float *rgb_out, uint64_t *num_rays_out,
                              r1_tile_report *tiles_out, r1_adaptive_result *result_out);

/* Host only, pure arithmetic: out[i] = (uint8_t)(int)(sqrtf(linear[i]) * 255.99f), rayweek1.cpp:766-775 for one channel, with the
 * host's correctly rounded sqrtf.  A value whose (int) is undefined — negative (-0.0f counts as zero), NaN, infinite, or so large that
 * the product is no int — is R1_EINVAL, and no byte is written then.  n_values == 0 is R1_OK. */
int r1_quantise_linear(const float *linear, size_t n_values, uint8_t *out);

/* The CPU form of r1_render_linear, no device: r1_camera_rays and r1_trace_rays_host for every sample, summed as above.  Slow (every ray
 * against every sphere), meant for small frames: it is what lets the value be checked without a GPU.  num_rays_out may be NULL. */
int r1_render_linear_host(const r1_scene *scene, const r1_camera *camera, const r1_params *params, float *rgb_out, uint64_t *num_rays_out);

/* ---- region renders: a window of the frame, bit for bit its crop ---- */

/* A window of the frame `params` describes.  params keeps the meaning it has in r1_render: its width and height fix the pixel index
 * y * width + x of the seeds (rays1_seed.h) and the camera's 1/W, 1/H, so a sample's streams depend on (seed, pixel of the FRAME, sample
 * index) alone and the window's pixels are the frame's, whatever else the launch traces. */
typedef struct r1_region
{
    int32_t x0, y0;        /* lower-left pixel of the window in the frame (row 0 = bottom row, as everywhere) */
    int32_t width, height; /* its size in pixels, >= 1; x0 + width <= params->width, y0 + height <= params->height */
    int32_t out_stride;    /* pixels between the starts of two rows of the OUTPUT image; 0 = width, else >= width */
} r1_region;

/* Results, with stride = out_stride ? out_stride : width:
 *   bytes    pixel (x, y) of the region at out + ((size_t)y * stride + x) * 3 equals pixel (x0 + x, y0 + y) of r1_render(params), byte for byte;
 *   linear   floats at out + ((size_t)y * stride + x) * 3 equal r1_render_linear's value of that pixel, bit for bit;
 *   records  equal r1_render_samples' records of those pixels, in the region's own order ((y * region.width + x) * spp + s), dense;
 *   count    the color() calls of exactly the region's samples = the sum of those records' count words;
 *   with out_stride > width the bytes between the rows are not written: out_stride = params->width and out = frame + (y0 * W + x0) * 3
 *   patch a window into a caller's whole frame.
 * Limits: params must pass every check of r1_params_check except the sample total; the frame has width * height < 2^31 (the pixel index
 * stays an int) and need not fit one launch; the region is bounded as a frame of its own size is: region.width * region.height * spp
 * < 2^31 and the padded sample slots of its tiles < 2^31, else R1_ELIMIT.  So a 40 000 x 40 000 x 2 frame, which r1_render refuses, is
 * rendered window by window.  Whole-frame sharding is not combined with regions (num_shards != 1: R1_EINVAL); the variants are those
 * r1_render_pass accepts (DEFAULT, REFERENCE, PREFILTER, BVH, GRID; the diagnostic variants and WAVEFRONT: R1_EINVAL).  After an update
 * regions are served and refused as frames are.  PIXEL mode does not apply.  One region render per context at a time, as for any frame.
 * The region's tiles (params->tile_w x tile_h) are cut from the region's own corner. */

/* Pure arithmetic, no device: the one place the rules above are checked; every call below uses it.  R1_EINVAL names the offending
 * field in r1_last_error; R1_ELIMIT as above. */
int r1_region_check(const r1_params *params, const r1_region *region);

/* Synchronous; r1_render's rules otherwise: it leaves a progressive accumulation alone, and r1_last_launch_info / r1_last_timing
 * describe it.  num_rays_out and device_seconds_out may be NULL. */
int r1_render_region(r1_context *ctx, const r1_params *params, const r1_region *region, uint8_t *rgb_out, uint64_t *num_rays_out,
                     double *device_seconds_out);

/* The same, plus the records: samples_out receives region.width * region.height * spp records of 4 floats (r1_render_samples' record). */
int r1_render_region_samples(r1_context *ctx, const r1_params *params, const r1_region *region, uint8_t *rgb_out, uint64_t *num_rays_out,
                             float *samples_out);

/* The linear form: three floats per pixel (r1_render_linear's value). */
int r1_render_region_linear(r1_context *ctx, const r1_params *params, const r1_region *region, float *rgb_out, uint64_t *num_rays_out,
                            double *device_seconds_out);

/* Into DEVICE memory: d_rgb_u8 (bytes) and d_rgb_f32 (floats, 4-byte aligned) — either or both, R1_EINVAL if neither — and d_num_rays
 * (one uint64, 8-byte aligned, not NULL).  Everything is enqueued on `hip_stream` (NULL = the context's stream) and nothing is waited
 * for, as with r1_render_linear_device.  A refused call enqueues nothing. */
int r1_render_region_device(r1_context *ctx, const r1_params *params, const r1_region *region, void *d_rgb_u8, void *d_rgb_f32,
                            void *d_num_rays, void *hip_stream);

/* The CPU form, no device: r1_camera_rays + r1_trace_rays_host per sample, summed as r1_render_linear_host sums; honours out_stride
 * (nothing between the rows is written).  Bytes come from r1_quantise_linear.  num_rays_out may be NULL. */
int r1_render_region_host(const r1_scene *scene, const r1_camera *camera, const r1_params *params, const r1_region *region, float *linear_out,
                          uint64_t *num_rays_out);

/* ---- feature frames: first-hit albedo, normal and depth per pixel ---- */

/* The guide images a denoiser, an upscaler or a compositor wants beside a noisy frame, aligned with it pixel for pixel.  For pixel (x, y)
 * of the frame `params` describes (width, height, spp, seed) and the context's camera, the samples s = 0 .. spp - 1 in that order:
 *   ray      what r1_camera_rays returns for (x, y, s) — the same draws, the pixel index y * width + x of the FRAME — normalised once, as the
 *            Ray constructor does: the primary ray r1_render traces for that sample;
 *   hit      Hitable::hit(ray, 0.001f, FLT_MAX): R1_CAST_CLOSEST's record;
 *   a sample with a hit adds the sphere's albedo_r / _g / _b as the scene arrays hold them (a dielectric: 1, 1, 1, the weight of its
 *            scatter) to albedo, the record's n to normal, its t to depth and 1 to hits;
 *   a sample without one adds the sky's colour for its ray to albedo — u = 0.5f * (d.y + 1.0f), (1 - u) * 1.0f + u * {0.5f, 0.7f, 1.0f} — and
 *            nothing else;
 *   a sample whose origin or normalised direction is not finite adds nothing and is not tested.
 * Each of the seven sums starts at 0.0f and takes plain fp32 adds in sample order; then one fp32 multiply by (float)(1.0f / spp) each —
 * r1_render_linear's arithmetic.  Normals are not re-normalised; depth * spp / hits is the mean distance over the hits, hits / spp the
 * coverage.  A pixel with hits == 0 has albedo equal to r1_render_linear's value of that pixel, bit for bit: every sample's radiance is the
 * sky of its primary ray. */
typedef struct r1_feature
{
    float albedo[3];
    float depth;
    float normal[3];
    uint32_t hits; /* samples of the pixel with a hit, 0 .. spp */
} r1_feature;

/* A feature frame has r1_render's layout with records for pixels: row-major, row 0 = bottom row.  `region` is r1_region's window, out_stride
 * (in pixels, here records) included — nothing between the rows is written, the window's records are the frame's — and NULL means the
 * whole frame, {0, 0, width, height, 0}.  The rules are r1_region_check's, applied to that region (so num_shards != 1 is R1_EINVAL, and
 * max_bounces and the tile fields are checked and otherwise unused).  params->variant follows the queries' rule: DEFAULT and BVH walk the
 * box tree, GRID the uniform grid (built on first use; far origins take the tree), REFERENCE tests every sphere; any other variant is
 * R1_EINVAL.  The call is a query: a progressive accumulation survives it, r1_last_launch_info and r1_last_timing keep describing the
 * last render, after an update it sees the moved scene (GRID: R1_EINVAL, "the scene has moved", until r1_regrid), and the camera is the
 * context's, as r1_set_scene or r1_set_camera left it.  Refusals, in this order: ctx NULL; params, region or variant; no scene yet; out
 * NULL (device form: or not 16-byte aligned).  A refused call enqueues nothing.
 * Synchronous; `out` is host memory; device_seconds_out may be NULL. */
int r1_render_features(r1_context *ctx, const r1_params *params, const r1_region *region, r1_feature *out, double *device_seconds_out);

/* The same into DEVICE memory (16-byte aligned): everything is enqueued on `hip_stream` (NULL = the context's stream), nothing is waited
 * for.  No workspace but the launch's cursor: any number of these launches of a context may be in flight. */
int r1_render_features_device(r1_context *ctx, const r1_params *params, const r1_region *region, void *d_out, void *hip_stream);

/* The CPU form, no device: r1_camera_rays + r1_cast_rays_host per sample and the sums above.  Slow (every ray against every sphere); it
 * is what the other two are checked against.  params->variant is checked as r1_region_check checks it and otherwise unused. */
int r1_render_features_host(const r1_scene *scene, const r1_camera *camera, const r1_params *params, const r1_region *region, r1_feature *out);

/* ---- denoised frames: an edge-avoiding a-trous filter over the feature guides ---- */

/* The filter of a noisy linear frame L (r1_render_linear's layout: three floats per pixel, row 0 = bottom row) guided by the feature frame f
 * of the same frame (r1_render_features): a 5 x 5 B3-spline kernel applied `iterations` times with its taps 1, 2, 4, ... pixels apart, every
 * tap weighted by how well its normal, its depth and its current colour agree with the centre's.  The arithmetic is one contract, and the
 * device forms equal r1_denoise_host bit for bit.  Plain fp32; every * + - / and sqrtf below is one correctly rounded operation in the order
 * written, nothing is fused, min / max / clamp are selects, the weights are rational (no exp), subnormal values are kept.
 *   prepare, per pixel p:
 *     surf = hits > 0;  a_c = DEMODULATE ? (albedo_c < 1/256 ? 1/256 : albedo_c) : 1;  e_c = L_c / a_c
 *     nn = (nx*nx + ny*ny) + nz*nz;  l = sqrtf(nn);  nh = l > 0 ? n / l : 0 (one division per component)
 *     m = surf ? depth / (float)hits : 0      (the mean distance of the pixel's hits, up to the factor spp both sides of a ratio share)
 *   iteration i = 0 .. iterations - 1, cur = e at first:
 *     step = 1 << i;  sc = sigma_color * 2^-i;  sc2 = sc * sc
 *     a pixel that is not surf keeps its value; for a surf pixel p: S_c = 0, W = 0, then the taps q = p + step * (dx, dy), dy = -2 .. 2 in
 *     the outer loop and dx = -2 .. 2 in the inner one; a tap off the image or not surf is skipped
 *       h = H[dy + 2] * H[dx + 2], H = {1/16, 1/4, 3/8, 1/4, 1/16} (exact products); the centre tap has w = h; any other tap
 *       c = (nh_p.x*nh_q.x + nh_p.y*nh_q.y) + nh_p.z*nh_q.z;  c = c < 0 ? 0 : c;  c = c > 1 ? 1 : c;  c = c * c, normal_power_log2 times
 *       mx = m_p < m_q ? m_q : m_p;  den = sigma_depth * mx;  rz = den > 0 ? (m_p - m_q) / den : 0;  xz = rz * rz
 *       d = cur_p - cur_q;  dc = (d.r*d.r + d.g*d.g) + d.b*d.b;  xc = dc / sc2
 *       w = (h * c) / ((1 + xz) * (1 + xc))
 *       S_c = S_c + w * cur_q,c (multiply, then add);  W = W + w
 *     next_c = S_c / W  (W is at least 9/64, the centre's)
 *   end: out_c = cur_c * a_c for surf pixels; every other pixel of out has L's bits — all of its samples saw the sky of their primary rays,
 *   the pixel is free of noise.
 * No address depends on pixel data; non-finite input propagates by IEEE rules and cannot fault.
 * What to choose: the filter removes noise and detail alike, and the fewer samples a frame has the better the trade.  At 1-4 spp three
 * iterations with normal_power_log2 6, sigma_color 1, sigma_depth 0.1 and DEMODULATE cut the error against a converged frame to 0.4-0.85 of
 * the noisy frame's; at 16 spp three or more iterations gain little or make the frame WORSE and one iteration is what still helps
 * (DESIGN.md 4.39 has the figures).  A scene whose spheres are a few pixels each wants a lower normal_power_log2 (4). */
#define R1_DENOISE_DEMODULATE 1u       /* divide by the first-hit albedo before the filter, multiply after it: texture edges survive */
#define R1_DENOISE_MAX_ITERATIONS 8
#define R1_DENOISE_MAX_POWER_LOG2 10
typedef struct r1_denoise_opt
{
    int32_t iterations;        /* 1 .. 8: the taps of the last one are 2^(iterations - 1) pixels apart */
    int32_t normal_power_log2; /* k in 0 .. 10: the normals' cosine is raised to 2^k */
    float sigma_color;         /* > 0, finite */
    float sigma_depth;         /* > 0, finite: relative to the larger of the two mean distances */
    uint32_t flags;            /* R1_DENOISE_DEMODULATE or 0 */
} r1_denoise_opt;

/* The three images of a call: width x height pixels each, rows `*_stride` PIXELS apart (three floats of L and out, one record of f); a
 * stride of 0 means width.  Nothing between the rows is read or written. */
typedef struct r1_denoise_frame
{
    int32_t width, height;
    int32_t linear_stride, feature_stride, out_stride;
} r1_denoise_frame;

/* The rules of both structs, pure arithmetic, the one place they are checked: R1_EINVAL names the offending field (width, height, a stride
 * that is neither 0 nor >= width, iterations, normal_power_log2, sigma_color, sigma_depth, flags), R1_ELIMIT at width * height >= 2^31. */
int r1_denoise_check(const r1_denoise_frame *frame, const r1_denoise_opt *opt);

/* The definition: the contract above on the CPU, no device.  `out` may be L (L is consumed before out is written); f must not overlap out. */
int r1_denoise_host(const r1_denoise_frame *frame, const r1_denoise_opt *opt, const float *L, const r1_feature *f, float *out);

/* The same on DEVICE memory: d_L and d_out 4-byte aligned, d_f 16-byte aligned, d_out may be d_L.  Everything is enqueued on `hip_stream`
 * (NULL = the context's stream), nothing is waited for.  The filter's records (48 bytes a pixel) live in a workspace of the context that
 * grows on first use, as the queries' does: ONE denoise per context may be in flight, ordered by the stream.  Like the queries it changes no
 * state a render reads: a progressive accumulation survives it, r1_last_launch_info and r1_last_timing keep describing the last render.
 * Needs no scene.  Refusals, in this order: ctx NULL; frame or options (r1_denoise_check); then pointers and alignment.  A refused call
 * enqueues nothing. */
int r1_denoise_device(r1_context *ctx, const r1_denoise_frame *frame, const r1_denoise_opt *opt, const void *d_L, const void *d_f, void *d_out, void *hip_stream);

/* The same on HOST memory, synchronous: L and f go up, out comes home; device_seconds_out (may be NULL) is the filter's time alone. */
int r1_denoise(r1_context *ctx, const r1_denoise_frame *frame, const r1_denoise_opt *opt, const float *L, const r1_feature *f, float *out,
               double *device_seconds_out);

/* A frame rendered and denoised: r1_render_linear_device + r1_render_features_device + r1_denoise_device of the whole frame `params`
 * describes, on one stream, the feature frame in the context's workspace; rgb_out is r1_render_linear's layout, the ray count is
 * r1_render_linear's.  params->variant must be one both parts accept — DEFAULT, BVH, GRID or REFERENCE — else R1_EINVAL; for the rest the
 * rules are r1_render_linear's, and so is the state the call leaves (launch info, timing).  Refusals, in
 * this order: ctx NULL; params or options NULL, the options, the variant; then pointers and alignment; then what r1_render_linear refuses.
 * A refused call enqueues nothing.  Synchronous; device_seconds_out (may be NULL): render, features and filter together. */
int r1_render_denoised(r1_context *ctx, const r1_params *params, const r1_denoise_opt *opt, float *rgb_out, uint64_t *num_rays_out,
                       double *device_seconds_out);

/* The same into DEVICE memory (d_rgb_f32 4-byte aligned, d_num_rays 8-byte aligned), enqueued on `hip_stream`, waits for nothing. */
int r1_render_denoised_device(r1_context *ctx, const r1_params *params, const r1_denoise_opt *opt, void *d_rgb_f32, void *d_num_rays, void *hip_stream);

/* ---- variance frames: the variance of every pixel's mean beside its linear value ---- */

/* What a variance-guided filter, an error-driven sampling rule or a confidence display wants beside a linear frame: how far each pixel's
 * mean can be trusted.  The contract — plain fp32, every operation correctly rounded, in the order written, nothing fused.  For pixel
 * (x, y), channel c, n = spp and the pixel's sample records x_s (r1_render_samples' records):
 *   L_c    exactly r1_render_linear's value: S = 0.0f; S += x_s,c for s = 0 .. n - 1; L = S * (float)(1.0f / n)
 *   D_c    D = 0.0f; then for s = 0 .. n - 1: d = x_s,c - L_c; D = D + d * d — a second walk over the same records, in sample order
 *   var_c  n > 1 ? D_c * (1.0f / ((float)n * (float)(n - 1))) : 0.0f
 * var is the unbiased estimate of the variance of the pixel's MEAN (the sample variance over n).  It is never negative; for n = 1 it is
 * +0.0f, bits 0, whatever the records hold — one sample carries no variance.  A record that is not finite makes its pixel's var NaN or
 * infinite by IEEE rules and touches no other pixel. */
typedef struct r1_moment
{
    float var[3];
    uint32_t samples; /* n: the samples behind L and var */
} r1_moment;

/* A variance frame has r1_render's layout with 16-byte records for pixels, as a feature frame has: row-major, row 0 = bottom row, dense,
 * width * height * 16 bytes.  The three forms below follow r1_render_linear, r1_render_linear_device and r1_render_linear_host in every
 * rule: whole frames only (num_shards != 1: R1_EINVAL), every variant r1_render_linear accepts, the same ray count, PIXEL mode does not
 * apply, a progressive accumulation is left alone, r1_last_launch_info and r1_last_timing describe the frame.  rgb_out is r1_render_linear's
 * frame bit for bit.  The cost is no further launch: the one that closes a linear frame is replaced by one that walks the records twice and
 * stores both outputs, inside the timed span.  A refused call enqueues nothing.
 * Not provided: variance from a progressive or adaptive accumulation, of a region, of a frame in flight (r1_render_linear_async), of a
 * batch, a shard or an r1_multi frame — their accumulators hold sums only, and a second moment wants the records of all samples at once. */

/* Synchronous; rgb_out and moments_out are host memory (page-locked memory, moments_out 16-byte aligned, is written by the launch itself);
 * num_rays_out and device_seconds_out may be NULL. */
int r1_render_moments(r1_context *ctx, const r1_params *params, float *rgb_out, r1_moment *moments_out, uint64_t *num_rays_out,
                      double *device_seconds_out);

/* Into DEVICE memory: d_rgb_f32 (width * height * 3 floats, 4-byte aligned), d_moments (width * height records, 16-byte aligned),
 * d_num_rays (one uint64, 8-byte aligned); R1_EINVAL otherwise.  Everything is enqueued on `hip_stream` (NULL = the context's stream),
 * nothing is waited for. */
int r1_render_moments_device(r1_context *ctx, const r1_params *params, void *d_rgb_f32, void *d_moments, void *d_num_rays, void *hip_stream);

/* The CPU form, no device: r1_render_linear_host's frame and ray count and the records above.  Slow; it is what the other two are checked
 * against.  num_rays_out may be NULL. */
int r1_render_moments_host(const r1_scene *scene, const r1_camera *camera, const r1_params *params, float *rgb_out, r1_moment *moments_out,
                           uint64_t *num_rays_out);

/* ---- variance-guided denoised frames: the a-trous filter with a colour tolerance that follows each pixel's noise ---- */

/* The "denoised frames" contract above with these changes and no others.  V is the variance frame of L (r1_render_moments: var of the
 * pixel's mean), a_c the prepare step's albedo divisor, K3 = {1/4, 1/2, 1/4}.  Plain fp32, one correctly rounded operation per step, in
 * the order written.
 *   prepare     v = surf ? (V_r / (a_r * a_r) + V_g / (a_g * a_g)) + V_b / (a_b * a_b) : 0 — the variance of the demodulated value in the
 *               metric dc uses.  V of a pixel without a hit is never read into any result.
 *   iteration i, surf pixel p, before the taps: G = 0, K = 0; dy = -1 .. 1 in the outer loop, dx = -1 .. 1 in the inner one, q = p + (dx, dy)
 *               — one pixel apart at every step —, a tap off the image or not surf is skipped; k = K3[dy + 1] * K3[dx + 1];
 *               G = G + k * v_q; K = K + k; then g = G / K (K is at least 1/4, the centre's)
 *   colour term sc2 = sigma_color * sigma_color in every iteration (no 2^-i: the variance shrinks through the passes by itself);
 *               den = sc2 * g + variance_floor; xc = dc / den
 *   the sums    also T = T + (w * w) * v_q for every tap taken, the centre included with w = h; next_c = S_c / W; v_next = T / (W * W)
 * The end step, the normal and depth terms, the tap order and what a pixel without a hit keeps are unchanged.
 * What to choose: normal_power_log2 6, sigma_depth 0.1 and DEMODULATE as above, sigma_color 2 and variance_floor 1e-4, three iterations.
 * On the medium scene that cuts the error against a converged frame to 0.52 / 0.53 / 0.61 of the noisy frame's at 2 / 4 / 16 spp where the
 * fixed tolerance reaches 0.47 / 0.56 / 0.89, and five iterations no longer make a 16-spp frame worse (0.64 against 1.07); at 1 spp there
 * is no variance: use r1_denoise there (DESIGN.md 4.40 has the table). */
typedef struct r1_denoise_guided_opt
{
    r1_denoise_opt base;
    float variance_floor; /* > 0, finite */
    uint32_t reserved;    /* 0 */
} r1_denoise_guided_opt;

/* The four images of a call; strides in PIXELS (three floats of L and out, one record of f and of V), 0 means width. */
typedef struct r1_denoise_guided_frame
{
    int32_t width, height;
    int32_t linear_stride, feature_stride, moment_stride, out_stride;
} r1_denoise_guided_frame;

/* Pure arithmetic: r1_denoise_check's rules for the fields the structs share, then moment_stride, variance_floor and reserved; R1_EINVAL
 * names the field. */
int r1_denoise_guided_check(const r1_denoise_guided_frame *frame, const r1_denoise_guided_opt *opt);

/* The definition, on the CPU.  `out` may be L; f and V must not overlap out. */
int r1_denoise_guided_host(const r1_denoise_guided_frame *frame, const r1_denoise_guided_opt *opt, const float *L, const r1_feature *f,
                           const r1_moment *V, float *out);

/* On DEVICE memory: r1_denoise_device's rules (d_V 16-byte aligned as d_f; 56 bytes a pixel of the context's workspace; one denoise per
 * context in flight; no state a render reads changes).  Refusals: ctx NULL; the check; pointers and alignment.  Nothing is enqueued then. */
int r1_denoise_guided_device(r1_context *ctx, const r1_denoise_guided_frame *frame, const r1_denoise_guided_opt *opt, const void *d_L,
                             const void *d_f, const void *d_V, void *d_out, void *hip_stream);

/* On HOST memory, synchronous; device_seconds_out (may be NULL): the filter alone. */
int r1_denoise_guided(r1_context *ctx, const r1_denoise_guided_frame *frame, const r1_denoise_guided_opt *opt, const float *L,
                      const r1_feature *f, const r1_moment *V, float *out, double *device_seconds_out);

/* r1_render_moments_device + r1_render_features_device + the guided filter on one stream: r1_render_denoised's rules, and params->spp < 2
 * is R1_EINVAL naming spp — one sample carries no variance; use r1_render_denoised at 1 spp. */
int r1_render_denoised_guided(r1_context *ctx, const r1_params *params, const r1_denoise_guided_opt *opt, float *rgb_out,
                              uint64_t *num_rays_out, double *device_seconds_out);
int r1_render_denoised_guided_device(r1_context *ctx, const r1_params *params, const r1_denoise_guided_opt *opt, void *d_rgb_f32,
                                     void *d_num_rays, void *hip_stream);

/* ---- accumulated frames: history reprojected along a camera path ---- */

/* Temporal accumulation, the stage in front of the filters above: each pixel of the current frame looks up where its surface point was on
 * the PREVIOUS frame's screen, fetches the history there if the surfaces agree, and blends.  No new record type: a history is a previous
 * call's outputs (A: three floats a pixel, M: r1_moment with `samples` = the history's length) plus that frame's feature frame and camera.
 * One fp32 contract; r1_accumulate_host defines it and the device forms equal it bit for bit.  Plain fp32; every + - * / and sqrtf below is
 * one correctly rounded operation in the order written, nothing is fused, min / max / abs / clamp are selects, subnormal values are kept,
 * and floorf (exact) is the only library call.  a . b is (a.x*b.x + a.y*b.y) + a.z*b.z.
 *   inputs    the current frame: L and V (r1_render_moments) and f (r1_render_features) and the camera `cam` they were rendered through;
 *             the history: A_prev, f_prev, M_prev and the camera `prev` of that frame; spp of the current render and spp_prev of the render
 *             that made f_prev — they scale `depth` back to a distance, and nothing else.
 *   plan      r1_reproject_plan, once per call, on the host, shared by both forms.  From prev, with dl = lower_left - origin:
 *             pu = dl . u;  pv = dl . v;  pw = dl . w;  hu = horizontal . u;  vv = vertical . v;
 *             inv_w = 1.0f / (float)width;  inv_h = 1.0f / (float)height (as the renders form them).
 *             pw, hu or vv zero or not finite: R1_EINVAL naming camera_prev.
 *   pixel (x, y):  n = V.samples
 *     no surface   f.hits == 0 or n == 0: A_out has L's bits and M_out has V's bits.  (hits == 0: every sample saw the sky of its primary
 *                  ray, the pixel is free of noise, as for the filters.)
 *     world point  s = ((float)x + 0.5f) * inv_w;  t = ((float)y + 0.5f) * inv_h
 *                  d = ((cam.lower_left + cam.horizontal * s) + cam.vertical * t) - cam.origin     (camera_ray_at's order, no lens offset)
 *                  dh = d / sqrtf(d . d)  (one division per component);  m = (f.depth / (float)f.hits) * (float)spp;  P = cam.origin + dh * m
 *                  A PINHOLE reconstruction: the lens offsets of the samples are ignored, so with an aperture P is the point in focus
 *                  only to first order, and the depth test below is what forgives it.
 *     previous     q = P - prev.origin;  a = q . prev.u;  b = q . prev.v;  c = q . prev.w
 *     screen       the point is in front of the previous camera iff c * pw > 0 (a NaN fails)
 *     position     k = pw / c;  sx = (a * k - pu) / hu;  sy = (b * k - pv) / vv
 *                  px = sx * (float)width - 0.5f;  py = sy * (float)height - 0.5f
 *                  history exists only if px > -1 && px < (float)width && py > -1 && py < (float)height — comparisons of floats: NaN and
 *                  +-inf fail BEFORE any conversion to an integer
 *                  x0 = (int)floorf(px);  fx = px - floorf(px);  y0 and fy likewise
 *     expected     e = sqrtf(q . q)
 *     taps         B = 0, C = 0, U = 0, N = 2^32 - 1; (j, i) in {0, 1}^2, j in the outer loop, the tap at (x0 + i, y0 + j) with the bilinear
 *                  weight b = (i ? fx : 1 - fx) * (j ? fy : 1 - fy).  A tap is skipped if it is off the image (tested on the integers,
 *                  first); or b is not > 0; or f_prev.hits == 0; or M_prev.samples == 0; or, with
 *                  m_q = (f_prev.depth / (float)f_prev.hits) * (float)spp_prev, t = e - m_q, t = t < 0 ? -t : t, mx = e < m_q ? m_q : e,
 *                  not t <= depth_tolerance * mx (a NaN skips); or nh . nh_q < normal_min_cos, nh the unit normal by the filters' prepare
 *                  rule (zero where the normals cancel).  A tap taken: B = B + b;  C_c = C_c + b * A_prev_c;  U_c = U_c + b * M_prev.var_c;
 *                  N = M_prev.samples < N ? M_prev.samples : N
 *     blend        if B > 0: hist = C / B;  vh = U / B;  N_new = max(n, min(N + n, max_samples)) in 64 bits (N near 2^32 cannot wrap);
 *                  alpha = n >= N_new ? 1.0f : (float)n / (float)N_new;  A_out = hist + (L - hist) * alpha;
 *                  var_out = ((1 - alpha) * (1 - alpha)) * vh + (alpha * alpha) * V.var;  samples_out = N_new.
 *                  Otherwise the pixel is as for "no surface".
 * The b-weighted mean of the four history variances is a deliberate approximation: the four pixels share samples of earlier frames, so
 * they are correlated and the true variance of the mean is not the mean of the variances; it errs towards a larger variance.
 * Addresses DO depend on pixel data here, which the filters' contracts rule out.  The guard order above is what keeps them on the image:
 * the float comparisons on px and py come first and fail for NaN and infinities, floorf's results are then integers in -1 .. width - 1 and
 * -1 .. height - 1, and each tap's (x0 + i, y0 + j) is tested against the image before an address is formed from it.  Every tap address is
 * formed from integers already tested to lie on the image; non-finite or absurd input loses its history and cannot fault.
 * Aliasing: the call is a gather, so A_out / M_out must not overlap A_prev / M_prev / f_prev — equal pointers are refused (R1_EINVAL).
 * A_out may be L and M_out may be V: a pixel's own records are consumed before its outputs are written.
 * Moving spheres need no motion vectors in this contract: a point on a sphere that moved re-projects to where the sphere was not, and
 * the depth and normal tests drop that history — the pixel starts again from its own samples.  Per-sphere motion vectors, which would keep
 * it, are out of scope.
 * What to choose (tools/accumulate_prototype.py on the medium scene): max_samples 32, depth_tolerance 0.05,
 * normal_min_cos 0.9. */
typedef struct r1_accumulate_opt
{
    uint32_t max_samples;  /* >= 1: the cap of the history length; it turns the running mean into an exponential one */
    float depth_tolerance; /* > 0, finite: relative to the larger of the two distances */
    float normal_min_cos;  /* finite, -1 .. 1 */
    uint32_t flags;        /* 0 */
} r1_accumulate_opt;

/* The eight images of a call: width x height pixels each, rows `*_stride` PIXELS apart (three floats of L, A_prev and A_out, one record of
 * the others); a stride of 0 means width.  Nothing between the rows is read or written. */
typedef struct r1_accumulate_frame
{
    int32_t width, height;
    int32_t linear_stride, moment_stride, feature_stride;                /* L, V, f */
    int32_t prev_stride, prev_feature_stride, prev_moment_stride;        /* A_prev, f_prev, M_prev */
    int32_t out_stride, out_moment_stride;                               /* A_out, M_out */
} r1_accumulate_frame;

/* Through what the two frames were rendered */
typedef struct r1_accumulate_view
{
    r1_camera camera;      /* of L, V and f */
    r1_camera camera_prev; /* of the history */
    int32_t spp;           /* >= 1: of the render that made f */
    int32_t spp_prev;      /* >= 1: of the render that made f_prev */
} r1_accumulate_view;

/* The images: host memory for r1_accumulate_host and r1_accumulate, device memory for r1_accumulate_device */
typedef struct r1_accumulate_images
{
    const void *L;      /* float[3] a pixel */
    const void *V;      /* r1_moment */
    const void *f;      /* r1_feature */
    const void *A_prev; /* float[3] a pixel */
    const void *f_prev; /* r1_feature */
    const void *M_prev; /* r1_moment */
    void *A_out;        /* float[3] a pixel; may be L */
    void *M_out;        /* r1_moment; may be V */
} r1_accumulate_images;

/* What one call computes once for all of its pixels (the "plan" above) */
typedef struct r1_reproject_plan
{
    float pu, pv, pw, hu, vv, inv_w, inv_h;
} r1_reproject_plan;

/* The rules of the three structs, pure arithmetic, the one place they are checked: R1_EINVAL names the offending field (width, height, a
 * stride that is neither 0 nor >= width, max_samples, depth_tolerance, normal_min_cos, flags, spp, spp_prev, camera_prev when the plan is
 * unusable), R1_ELIMIT at width * height >= 2^31.  plan_out (may be NULL) receives the plan. */
int r1_accumulate_check(const r1_accumulate_frame *frame, const r1_accumulate_opt *opt, const r1_accumulate_view *view, r1_reproject_plan *plan_out);

/* The definition: the contract above on the CPU, no device.  Refusals: the check; then a NULL image; then an output equal to a history
 * image. */
int r1_accumulate_host(const r1_accumulate_frame *frame, const r1_accumulate_opt *opt, const r1_accumulate_view *view, const r1_accumulate_images *images);

/* The same on DEVICE memory: L, A_prev and A_out 4-byte aligned, the feature and moment images 16-byte aligned.  One launch, enqueued on
 * `hip_stream` (NULL = the context's stream), nothing is waited for.  It needs no workspace: any number of calls may be in flight.  Like
 * the filters it changes no state a render reads and needs no scene.  Refusals, in this order: ctx NULL; the check; then pointers,
 * alignment and aliasing.  A refused call enqueues nothing. */
int r1_accumulate_device(r1_context *ctx, const r1_accumulate_frame *frame, const r1_accumulate_opt *opt, const r1_accumulate_view *view,
                         const r1_accumulate_images *d_images, void *hip_stream);

/* The same on HOST memory, synchronous: the six inputs go up, the two outputs come home; device_seconds_out (may be NULL) is the kernel's
 * time alone. */
int r1_accumulate(r1_context *ctx, const r1_accumulate_frame *frame, const r1_accumulate_opt *opt, const r1_accumulate_view *view,
                  const r1_accumulate_images *images, double *device_seconds_out);

/* The composed, stateful form: on one stream r1_render_moments_device, then r1_render_features_device, then the accumulation against the
 * CONTEXT'S history, which the call then replaces by its own unfiltered result, feature frame, camera and spp.  guided_opt NULL: rgb_out is
 * the accumulated frame.  Otherwise r1_denoise_guided_device filters the ACCUMULATED frame with the accumulated variance and the current
 * features into rgb_out (the history keeps the unfiltered accumulation), and params->spp < 2 is R1_EINVAL as in r1_render_denoised_guided;
 * without the filter any spp is served.  "Previous camera" is the context's camera at the previous accumulated call, "current" the
 * context's camera now, as r1_set_scene or r1_set_camera left it.  The history is empty — the frame passes through unchanged, rgb_out is
 * r1_render_moments' frame — on the first call, after r1_accumulate_reset, after r1_set_scene, and when width or height differ from the
 * history's; r1_update_*, r1_resort_spheres and r1_regrid keep it.  A previous camera through which nothing can be projected also passes
 * the frame through.  The history (60 bytes a pixel, twice) lives in a workspace of the context that grows on first use; the calls of a
 * context are ordered by one stream, or by the caller.  Variants and refusal order are r1_render_denoised_guided's: ctx NULL; params or
 * acc_opt NULL, the params, the options, the variant, spp with a filter; pointers and alignment; then what r1_render_moments refuses.  A
 * refused call enqueues nothing and keeps the history.  The state left is r1_render_moments': launch info and timing describe the frame,
 * a progressive accumulation survives.  Synchronous; device_seconds_out (may be NULL): everything enqueued. */
int r1_render_accumulated(r1_context *ctx, const r1_params *params, const r1_accumulate_opt *acc_opt, const r1_denoise_guided_opt *guided_opt,
                          float *rgb_out, uint64_t *num_rays_out, double *device_seconds_out);

/* The same into DEVICE memory (d_rgb_f32 4-byte aligned, d_num_rays 8-byte aligned), enqueued on `hip_stream`, waits for nothing. */
int r1_render_accumulated_device(r1_context *ctx, const r1_params *params, const r1_accumulate_opt *acc_opt, const r1_denoise_guided_opt *guided_opt,
                                 void *d_rgb_f32, void *d_num_rays, void *hip_stream);

/* Forgets the context's history: the next accumulated frame passes through.  Waits for nothing, frees nothing. */
int r1_accumulate_reset(r1_context *ctx);

/* Pipelined form of r1_render — frames in flight whose results land on the HOST.  The reference times
 * dispatch -> pixels + ray count on the host (rayweek1.cpp:848 -> :891) for ONE frame and waits; a caller that
 * renders frame after frame (main's `-n` runs, rayweek1.cpp:969-984) can keep several in flight instead: the call
 * enqueues the frame (throughput kernels: few long-lived waves per frame) on `hip_stream` (a hipStream_t; NULL =
 * the context's stream) and returns without waiting.  Buffers from r1_host_alloc (page-locked, num_rays_out 8-byte
 * aligned) are written by the launch itself: every tile lands in rgb_out (row-major, width*height*3 bytes, as
 * r1_render) when its samples are complete, the ray count when the frame's last tile has — no resolve launch, no copy.
 * Pageable memory works too: the frame is then resolved into the context's device image and two copies follow the
 * launch, each waiting for its frame.  Both buffers are valid once the stream is idle (r1_sync for the context's
 * stream).  One frame per context at a time (the calls on a context are ordered by one stream, or by the caller): K
 * frames in flight = K contexts.  Whole frames only (num_shards == 1).  rgb_out and num_rays_out both NULL: the frame is
 * rendered and left in the context's device buffers (a measurement aid). */
int r1_render_async(r1_context *ctx, const r1_params *params, uint8_t *rgb_out, uint64_t *num_rays_out, void *hip_stream);

/* Frame BATCHES: n_frames frames of the same scene, camera and size in ONE launch; frame f is seeded
 * params->seed + f * seed_stride (0: identical frames; 1: independent frames of consecutive seeds — the passes of a
 * progressive render that ADD UP are r1_render_pass's).  The trace kernel is
 * persistent — a wave keeps refilling its lanes from a queue of samples — and what a launch costs beyond its samples is
 * its ramp and, above all, its drain: the last ~40 iterations of every wave run with few live lanes.  In a batch the
 * queue is frame-major and the waves flow from one frame into the next, so that cost is paid once per batch instead of
 * once per frame (measured: DESIGN.md §4.9).  The price is latency: all frames of a batch are delivered together.
 * host_frames receives n_frames frame records of r1_frame_record_bytes() each — the row-major image (as r1_render),
 * padded to a multiple of 8 bytes, then the frame's uint64 ray count — written by the launch itself when the memory is
 * page-locked (r1_host_alloc), else with ONE copy enqueued behind the launch; nothing
 * is waited for (as r1_render_async; NULL leaves the frames on the device).  Whole
 * frames only.  Each frame's pixels and count equal what r1_render returns for its seed. */
size_t r1_frame_record_bytes(const r1_params *params);
int r1_render_batch_async(r1_context *ctx, const r1_params *params, int32_t n_frames, uint32_t seed_stride, void *host_frames, void *hip_stream);

/* Camera PATHS: r1_render_batch_async with cameras[f] in place of the context's camera for frame f — a turntable or a
 * fly-through in one launch, the waves flowing from frame to frame (the MODE 5 kernels: where a sample starts, its lane loads the
 * camera of the sample's frame from a device table).  Same frame records, same page-locked / pageable / NULL host_frames
 * behaviour, same limits (R1_ELIMIT) and the same variants accepted and refused as r1_render_batch_async; whole frames only,
 * n_frames >= 1.  `cameras` is host memory, n_frames entries, read during the call only.  The context's own camera is not
 * changed.  Frame f's pixels and count equal r1_render with seed params->seed + f * seed_stride after
 * r1_set_camera(ctx, &cameras[f]).  There is no sharded device form (r1_render_shard_device_batch with cameras) and no
 * r1_multi form of it: more than one device has never run on hardware here, and camera paths add nothing to that debt. */
int r1_render_path_async(r1_context *ctx, const r1_params *params, int32_t n_frames, uint32_t seed_stride, const r1_camera *cameras, void *host_frames,
                         void *hip_stream);

/* Page-locked, device-visible host memory for the render entry points' outputs (hipHostMalloc / hipHostFree). */
int r1_host_alloc(size_t bytes, void **out);
void r1_host_free(void *p);

/* ---- device-resident variants (multi-GPU gather, benchmarks) ----------------------- */

/* Number of tiles / bytes of the dense tile block one shard produces for `params`
 * (every shard's block is padded to the same size so it can be all-gathered). */
int r1_tile_count(const r1_params *params, int32_t *tiles_total, int32_t *tiles_per_shard);
size_t r1_shard_block_bytes(const r1_params *params);
/* Bytes of one shard's gather RECORD: its tile block padded to a multiple of 8, followed by its uint64 ray count
 * (at r1_shard_record_bytes() - 8, 8-byte aligned for any tile size), so that one all-gather moves pixels and
 * counts together (the reference sums `out_num_rays` after the join, rayweek1.cpp:809-813). */
size_t r1_shard_record_bytes(const r1_params *params);

/* Enqueues the render of this shard on the context's stream (or on `hip_stream` if
 * non-NULL, a hipStream_t) and writes DEVICE memory only:
 *   d_block      r1_shard_block_bytes() bytes: tiles_per_shard tiles of tile_h*tile_w*3
 *                bytes each, local tile j = global tile shard + j*num_shards
 *   d_num_rays   one uint64 (overwritten); must be 8-byte aligned (R1_EINVAL otherwise)
 * Does not synchronise.  Sized for throughput: meant to be called for several frames in
 * flight (one context + stream per frame in flight). */
int r1_render_shard_device(r1_context *ctx, const r1_params *params, void *d_block, void *d_num_rays, void *hip_stream);

/* A batch of n_frames frames of this shard in one launch (see r1_render_batch_async): d_records receives n_frames
 * records of r1_shard_record_bytes() each (dense tile block, padded to 8 bytes, + the shard's uint64 ray count of that
 * frame), 8-byte aligned device memory — what a rank hands to ONE all-gather per batch. */
int r1_render_shard_device_batch(r1_context *ctx, const r1_params *params, int32_t n_frames, uint32_t seed_stride, void *d_records, void *hip_stream);

/* PIXEL mode for r1_render_shard_device (off by default).  On: a lane of the trace kernel owns a pixel and runs
 * its spp samples one after the other, so the `col += color()` of rayweek1.cpp:762 happens in a register in the
 * reference's order and the resolved pixel (rayweek1.cpp:765-775) is all the frame writes — 3 bytes per pixel
 * instead of 16 bytes per sample, no resolve launch, no per-sample workspace (3.9 GB per frame in flight at
 * 1200x800x250).  Same pixels and ray counts; measured ~10 % slower on the reference's scenes (a frame's last
 * pixels are ten dependent samples long), which is why it is a choice.  The host-returning entry points and
 * r1_render_samples always keep per-sample records. */
int r1_set_pixel_mode(r1_context *ctx, int32_t on);

/* Same outputs, sized for latency instead: ONE frame whose result the caller waits for (the full
 * persistent grid and the latency-mode kernels of r1_render).  Used by r1_multi_render. */
int r1_render_shard_device_once(r1_context *ctx, const r1_params *params, void *d_block, void *d_num_rays, void *hip_stream);

/* Scatters `num_shards` gathered blocks (concatenated in shard order, device memory)
 * into the row-major image d_rgb (width*height*3 bytes, device memory). */
int r1_assemble_device(r1_context *ctx, const r1_params *params, const void *d_blocks, void *d_rgb, void *hip_stream);

/* Same, for blocks that are `shard_stride_bytes` apart (>= r1_shard_block_bytes; 0 = tight):
 * lets a caller append per-shard trailers (e.g. the 8-byte ray count) to the gathered records so
 * that one all-gather moves pixels and counts together. */
int r1_assemble_device_strided(r1_context *ctx, const r1_params *params, const void *d_blocks, size_t shard_stride_bytes,
                               void *d_rgb, void *hip_stream);

/* Same for gathered RECORDS (num_shards x r1_shard_record_bytes(), the layout one all-gather returns): scatters the
 * tile blocks into d_rgb and writes the sum of the shards' ray counts — the join of rayweek1.cpp:809-813 — to
 * *d_total_rays (device memory, 8-byte aligned; e.g. right behind the image, so that one copy brings both home). */
int r1_assemble_device_records(r1_context *ctx, const r1_params *params, const void *d_records, void *d_rgb, void *d_total_rays,
                               void *hip_stream);

/* Batches: d_gathered = the result of ONE all-gather of every shard's n_frames records, [shard][frame][record];
 * d_frames receives n_frames frame records (r1_frame_record_bytes each: image + summed ray count). */
int r1_assemble_device_records_batch(r1_context *ctx, const r1_params *params, int32_t n_frames, const void *d_gathered, void *d_frames,
                                     void *hip_stream);

/* Blocks until the context's stream is idle. */
int r1_sync(r1_context *ctx);

/* HIP-event duration (ms) of the trace kernel / of all kernels of the last render
 * enqueued through this context (valid after r1_sync or a host-returning call). */
int r1_last_timing(r1_context *ctx, double *trace_kernel_ms, double *total_ms);

/* Per-frame kernel timing over a run of frames: between r1_timing_begin and r1_timing_end
 * every render enqueued through the context records its own HIP events (on the stream it
 * is launched on) instead of the single "last frame" set; r1_timing_end waits for them and
 * returns the summed trace-kernel and trace+resolve durations (ms) and the frame count.
 * Frames beyond max_frames reuse the last slot. */
int r1_timing_begin(r1_context *ctx, int32_t max_frames);
int r1_timing_end(r1_context *ctx, double *trace_ms_sum, double *total_ms_sum, int32_t *frames);

/* Diagnostic counters of the last R1_VARIANT_STATS render through the context's own stream:
 * 16 uint64: [0] wave iterations, [1] alive lanes summed over iterations, [2] candidate-loop
 * trips, [3] lanes that overflowed the candidate list, [4..7] cycles in refill / pass 1 /
 * candidate re-test / shade, [8] wave cycles, [9] candidates, [14] (tree) leaf trips summed over lanes, [15] (tree) root steps. */
int r1_last_stats(r1_context *ctx, uint64_t *out16);

/* Per-wave log of the last R1_VARIANT_*_STATS render: 4 uint64 per wave {start, sample queue found
 * empty, end (100 MHz device clock), outer iterations}.  out == NULL only returns the wave count.  Diagnostic. */
int r1_last_wave_log(r1_context *ctx, uint64_t *out, size_t cap_waves, uint32_t *waves);

/* Launch geometry and occupancy facts of the last render (for reports). */
typedef struct r1_launch_info
{
    int32_t compute_units;
    int32_t blocks;
    int32_t threads_per_block;
    int32_t spheres_active; /* spheres with inv_radius != 0 that the sweep visits */
    int32_t spheres_padded; /* `count` of the scene (N_pad of the reference)     */
    int32_t groups;         /* sphere groups the first sweep level tests          */
    uint64_t samples;       /* pixel-samples traced                              */
    int32_t kernel;         /* R1_VARIANT_* the launch actually ran (DEFAULT resolved) */
    int32_t bvh_nodes;      /* inner nodes of the spatial index                   */
    int32_t bvh_leaves;
    int32_t bvh_depth;      /* inner nodes on the longest root-to-leaf path       */
    int32_t tiles_in_kernel; /* 1: the trace launch summed its tiles itself (frames in flight); 0: a resolve launch followed */
} r1_launch_info;
int r1_last_launch_info(r1_context *ctx, r1_launch_info *out);

/* The form of the box-tree walk in the context's last trace launch: 1 — the kernel with the tree's flat axis compiled in (frames in flight
 * and batches of R1_VARIANT_BVH on a small scene whose current tree is flat; decided per launch, so an update that changes the tree's
 * flatness is followed), 0 — every other launch, and before the first.  Negative: ctx is NULL.  Diagnostic, for tests and reports;
 * r1_launch_info keeps its layout and its `kernel`. */
int r1_last_walk_form(r1_context *ctx);

/* ---- one process, N GPUs: tile split + one RCCL all-gather per frame --------------------- */

/* The multi-GPU form of benchmark()'s join (rayweek1.cpp:804-813, :773-775) behind ONE call, so that
 * the reference's four-argument benchmark() stays a single function: tile t is
 * rendered by device t % N (r1_params.shard / num_shards are set by the library), every device's
 * record (dense tile block + its uint64 ray count) goes through one ncclAllGather over xGMI, device 0
 * assembles the row-major image and copies it to the host once.  RCCL is loaded at run time
 * (librccl.so.1); r1_multi_create fails with R1_ENODEVICE where it is missing — no fallback.
 * `devices` = N distinct HIP device ordinals (NULL: 0..N-1).  One call at a time per r1_multi. */
typedef struct r1_multi r1_multi;
int r1_multi_create(int32_t n_devices, const int32_t *devices, r1_multi **out);
void r1_multi_destroy(r1_multi *m);
int r1_multi_set_scene(r1_multi *m, const r1_scene *scene, const r1_camera *camera);
/* r1_set_camera on every device's context. */
int r1_multi_set_camera(r1_multi *m, const r1_camera *camera);
/* rgb_out / num_rays_out as r1_render (whole frame); device_seconds_out (optional): render + gather
 * on the slowest device, from HIP events. */
int r1_multi_render(r1_multi *m, const r1_params *params, uint8_t *rgb_out, uint64_t *num_rays_out, double *device_seconds_out);
/* Frames in flight across the N GPUs from one process: the enqueue-only form of r1_multi_render (throughput kernels, this
 * object's own all-gather, device 0 assembles image + summed count into ONE frame record — r1_frame_record_bytes() — and copies
 * it into `host_frame`, page-locked memory).  Nothing is waited for; r1_multi_sync waits for this object's frame.  A caller
 * keeps K frames in flight with K r1_multi objects (each owns a communicator), as K r1_contexts do on one GPU. */
int r1_multi_render_async(r1_multi *m, const r1_params *params, void *host_frame);
/* The same for a batch of n_frames frames (seeds params->seed + f * seed_stride) per launch, all-gather and copy (see
 * r1_render_batch_async): host_frames receives n_frames frame records. */
int r1_multi_render_batch_async(r1_multi *m, const r1_params *params, int32_t n_frames, uint32_t seed_stride, void *host_frames);
int r1_multi_sync(r1_multi *m);
/* Where everything lies in the buffers of an n_devices-device frame or batch of n_frames frames: pure arithmetic (no device, no
 * r1_multi object), the very function the r1_multi_* entry points size and address their buffers with; so the layout of an N-GPU
 * run can be checked on a machine with one GPU or none (the join it describes: rayweek1.cpp:869-877, :809-813). */
typedef struct r1_multi_layout_info
{
    size_t block_bytes;        /* a device's dense tile block of ONE frame (r1_shard_block_bytes) */
    size_t record_bytes;       /* the block padded to 8 bytes + the device's uint64 ray count (r1_shard_record_bytes) */
    size_t count_offset;       /* the count's offset in a record */
    size_t send_bytes;         /* what a device hands to the all-gather: its n_frames records */
    size_t gathered_bytes;     /* what it receives: [device][frame][record] */
    size_t frame_record_bytes; /* an assembled frame: row-major image padded to 8 bytes + the frame's uint64 count (r1_frame_record_bytes) */
    size_t frame_count_offset;
    size_t host_bytes;         /* the one copy to the host: n_frames frame records */
    size_t counts_pitch;       /* distance between two devices' records in the gathered buffer */
} r1_multi_layout_info;
int r1_multi_layout(const r1_params *params, int32_t n_devices, int32_t n_frames, r1_multi_layout_info *out);
/* Facts for reports: device count, RCCL version code (ncclGetVersion), launch info of the first device. */
int r1_multi_info(r1_multi *m, int32_t *n_devices, int32_t *rccl_version, r1_launch_info *first_device);

/* ---- ray queries: Hitable::hit for caller-supplied rays --------------------------------- */

/* The contract of all three entry points is the reference's `Hitable::hit(Ray(o, d), 0.001f, t_max, &rec)` (rayweek1.cpp:104-108,
 * :152-339), bit for bit:
 *   direction  d is normalised as the Ray constructor does it, d * (1 / sqrt(dot(d, d))), in fp32.
 *   t_min      color()'s 0.001f, not a parameter (the per-sphere test hard-codes it and the box tree's proof is written for t > 0).
 *   t_max      strict: a root is accepted only if it is < t_max.  +inf is taken as FLT_MAX; NaN or a value <= 0.001f gives a miss.
 *   non-finite a ray with a non-finite component in o, or in d after normalisation (a zero direction normalises to NaN), is a miss,
 *              decided before any walk and identically in all three entry points.
 * R1_CAST_CLOSEST: `out` is n r1_hit records in ray order: t, the SCENE index of the hit sphere (an index into the r1_scene arrays,
 * placeholders counted), p = o + t * d_unit (multiply, then add) and n = (p - centre) * inv_radius, as rayweek1.cpp:316-322; a miss is
 * index = -1, t = FLT_MAX, p = n = 0.  Spheres with inv_radius == 0 are never returned (rayweek1.cpp:291).
 * R1_CAST_ANY: `out` is n bytes, 1 where R1_CAST_CLOSEST would report a hit, else 0 — the same walk, storing one byte (33 instead of
 * 64 bytes of memory traffic per ray).  There is no early exit. */
typedef struct r1_ray
{
    float o[3];
    float t_max;
    float d[3];
    uint32_t pad; /* ignored */
} r1_ray; /* 32 bytes */

typedef struct r1_hit
{
    float t;
    int32_t index;
    float p[3];
    float n[3];
} r1_hit; /* 32 bytes */

enum
{
    R1_CAST_CLOSEST = 0,
    R1_CAST_ANY = 1
};

/* Rays a single launch of r1_cast_rays covers: that call copies in, casts and copies out R1_CAST_CHUNK rays at a time through a
 * workspace cached in the context (64 bytes per ray of a chunk: 64 MiB), so device memory stays bounded for any n. */
#define R1_CAST_CHUNK (1u << 20)

/* Casts n rays from host memory against the scene cached in the context (r1_set_scene) and returns the results on the host.
 * Synchronous.  variant: R1_VARIANT_DEFAULT / R1_VARIANT_BVH (box tree), R1_VARIANT_GRID (uniform grid, built on first use as a
 * render builds it; rays whose origin is too far for the grid take the tree walk) or R1_VARIANT_REFERENCE (every active sphere in
 * index order, the reference's own loop: the on-device cross-check); every other variant returns R1_EINVAL.  All of them return the
 * same bytes.  Small and big scenes.  R1_EINVAL for a NULL ctx, a mode that is not R1_CAST_*, a variant that casts no rays
 * (r1_last_error names it) and before the first r1_set_scene; then n == 0 is R1_OK and touches nothing; then R1_EINVAL for NULL
 * pointers.  A cast changes no state another entry point sees: a progressive
 * accumulation survives it, r1_last_launch_info / r1_last_timing keep describing the last render, the camera plays no part. */
int r1_cast_rays(r1_context *ctx, int32_t variant, int32_t mode, const r1_ray *rays, size_t n, void *out);

/* The same over DEVICE memory: enqueues the cast on `hip_stream` (a hipStream_t; NULL = the context's stream) and waits for
 * nothing.  d_rays (n r1_ray) and d_out (n r1_hit, or n bytes) are device memory, both 16-byte aligned (R1_EINVAL otherwise). */
int r1_cast_rays_device(r1_context *ctx, int32_t variant, int32_t mode, const void *d_rays, size_t n, void *d_out, void *hip_stream);

/* The same without a device: every ray against every sphere in the reference's arithmetic, on host threads.  For callers without
 * a GPU at hand, and the checker of the two entry points above (tests/golden/cast_*.bin pin it to the reference's own output). */
int r1_cast_rays_host(const r1_scene *scene, int32_t mode, const r1_ray *rays, size_t n, void *out);

/* ---- path queries: color() for caller-supplied rays ---------------------------------------- */

/* Radiance along rays that no camera of this library generated (panoramas, stereo pairs, orthographic views, light probes, re-traced
 * samples).  The contract of the three trace forms is the reference's `color(Ray(o, d), scene, 0)` (rayweek1.cpp:517-534), bit for
 * bit: out[i] = {what it returns, the number of color() invocations it made}, with ThreadData::state = seeds[i].scalar and lanes 0..2
 * of ThreadData::state4 = seeds[i].lane0..2 when it is called.
 *   direction    d is normalised as the Ray constructor does it, d * (1 / sqrt(dot(d, d))), in fp32 — once.
 *   t_max, pad   of the r1_ray are ignored: color() always passes FLT_MAX.
 *   max_bounces  MAX_BOUNCES, 1..R1_MAX_BOUNCES_LIMIT; anything else is R1_EINVAL.
 *   non-finite   a ray with a non-finite component in o, or in d after normalisation (a zero direction normalises to NaN, one of
 *                1e-30 to infinity), runs no color(): its record is {0, 0, 0, rays = 0}.  The ray queries' test, identical in all
 *                three forms.
 *   zero states  xorshift32 has the fixed point 0, and random_in_unit_sphere on an all-zero stream never ends: a stream state of 0
 *                is replaced by r1_nonzero()'s constant before the path starts (r1_seed_guard of rays1_seed.h, called by the
 *                device's load and by the host form).  This is the guard against a caller-made GPU hang.
 *   seeds NULL   ray i is seeded with the seeding contract's states for (seed 0, pixel (uint32_t)i, sample 0); for the device form
 *                i is the index within the call.
 *   variants     as for the ray queries: R1_VARIANT_DEFAULT / _BVH (box tree), _GRID, _REFERENCE, same bytes from each; every other
 *                variant is R1_EINVAL (r1_last_error names it).  After r1_update_centers* GRID is refused ("the scene has moved"),
 *                the others see the moved scene.
 *   no spheres   a scene without an active sphere gives the sky for every valid ray.
 * Argument rules, in the ray queries' order: R1_EINVAL for a NULL ctx, then for a bad variant or max_bounces, then before the first
 * r1_set_scene; then n == 0 is R1_OK and touches nothing; then R1_EINVAL for NULL rays / out.
 * A trace changes no state another entry point sees: a progressive accumulation survives it, r1_last_launch_info / r1_last_timing
 * keep describing the last render, the context's camera plays no part.
 * Launches in flight: ONE trace launch per context.  The attenuation stack of the paths is a per-context workspace of max_bounces x
 * 4 bytes per thread of the launch — at most 51 x 4 x 256 threads x 8 workgroups per compute unit, 107 MB on a 256-CU device; typical
 * launches hold fewer workgroups — which grows on demand and is freed with the context.  K traces in flight = K contexts, as for frames. */
typedef struct r1_radiance
{
    float r, g, b;
    uint32_t rays;
} r1_radiance; /* 16 bytes: the record of r1_render_samples */

/* Rays the host-memory form works through at a time, in the workspace the ray queries cache in the context (64 bytes per ray: 32 ray +
 * 16 seed + 16 record). */
#define R1_TRACE_CHUNK (1u << 20)

/* Host memory in and out, synchronous. */
int r1_trace_rays(r1_context *ctx, int32_t variant, int32_t max_bounces, const r1_ray *rays, const r1_sample_seed *seeds, size_t n,
                  r1_radiance *out);

/* The same over DEVICE memory: enqueues on `hip_stream` (a hipStream_t; NULL = the context's stream) and waits for nothing.  d_rays
 * (n r1_ray), d_seeds (n r1_sample_seed, or NULL) and d_out (n r1_radiance) are 16-byte aligned (R1_EINVAL otherwise). */
int r1_trace_rays_device(r1_context *ctx, int32_t variant, int32_t max_bounces, const void *d_rays, const void *d_seeds, size_t n,
                         void *d_out, void *hip_stream);

/* The same without a device: every active sphere in index order with the host's exact test (the one behind r1_cast_rays_host), the
 * color() levels in scalar C++ in the reference's operation order, on host threads.  The checker of the two forms above. */
int r1_trace_rays_host(const r1_scene *scene, int32_t max_bounces, const r1_ray *rays, const r1_sample_seed *seeds, size_t n,
                       r1_radiance *out);

/* Host only, pure arithmetic: rayweek1.cpp:757-760 under the seeding contract.  For sample s[i] of pixel (x[i], y[i]) of a
 * params->width x height image with params->seed: the ray's origin (origin + lens offset), the UN-normalised direction exactly as
 * getRay hands it to the Ray constructor (the trace forms normalise once; twice may differ in the last bit), t_max = FLT_MAX, and the
 * four stream states AFTER the camera's draws (the jitter draw that advances lanes 0..2, the rejection loop of random_in_unit_disk on
 * the scalar stream).  This followed by any trace form equals that sample's record of r1_render_samples, bit for bit.  R1_EINVAL for
 * NULL pointers with n > 0, a pixel outside the image, or s < 0. */
int r1_camera_rays(const r1_camera *camera, const r1_params *params, const int32_t *x, const int32_t *y, const int32_t *s, size_t n,
                   r1_ray *rays_out, r1_sample_seed *seeds_out);

/* The same on the device, for a run of samples in r1_render_samples' order: for k in [first, first + n), sample s of pixel (x, y) with
 * (y * width + x) * spp + s == k; d_rays[k - first] and d_seeds[k - first] receive, byte for byte, what r1_camera_rays writes for that
 * sample.  camera NULL: the context's (r1_set_scene / r1_set_camera); a camera given travels by value in the launch's arguments.  Enqueues
 * on `hip_stream` (NULL: the context's stream) and waits for nothing.  R1_EINVAL for a NULL ctx or params, an empty image, spp < 1,
 * num_shards != 1, first + n beyond width * height * spp, no camera at all (camera NULL before the first r1_set_scene); then n == 0 is
 * R1_OK; then R1_EINVAL for NULL or misaligned (16 bytes) d_rays / d_seeds. */
int r1_camera_rays_device(r1_context *ctx, const r1_camera *camera, const r1_params *params, size_t first, size_t n, void *d_rays,
                          void *d_seeds, void *hip_stream);

/* ---- scatter queries: one color() level for caller-supplied rays --------------------------- */

/* The level between a cast and a trace: ONE call of the reference's color() body (rayweek1.cpp:517-534) — the hit test, then
 * Material::scatter — with the recursion left to the caller: another termination rule, per-bounce outputs, paths kept as data.  For ray i
 * the three forms write, byte for byte alike, the record out[i], the scattered ray rays_out[i] and the advanced stream states seeds_out[i].
 *   direction    without R1_SCATTER_UNIT_DIRECTIONS d is normalised as the Ray constructor does it (the trace forms' rule); with the flag d
 *                is used as it is: a scattered direction IS normalised, and normalising it twice can change its last bit.  The flag is the
 *                caller's promise that every d is a unit vector as a step wrote it (the rays_out of SCATTERED and ABSORBED records; the
 *                zero bytes behind SKY and NONE are no ray).  For any other finite d the call still returns, but the walks are built for
 *                unit directions and the variants need not agree.
 *   non-finite   the ray queries' test on o and on the direction actually used.  A ray that fails it: R1_SCATTER_NONE, the record zero but
 *                t = FLT_MAX, index = -1, mat_type = R1_MAT_NONE; rays_out[i] zero bytes; seeds_out[i] the guarded input; nothing drawn.
 *   seeds        r1_trace_rays' rules: NULL = the seeding contract's states for (seed 0, pixel i, sample 0), i the index within the call;
 *                r1_seed_guard on load in every form (a zero stream state never reaches random_in_unit_sphere).
 *   walk         Hitable::hit(r, 0.001f, FLT_MAX); t_max and pad of the input are ignored.
 *   miss         R1_SCATTER_SKY: weight = the sky's colour for the direction (rayweek1.cpp:532-534), nothing drawn, seeds_out[i] the
 *                guarded input, rays_out[i] zero bytes.
 *   hit          always scatters (the depth limit is the caller's): t, index (SCENE index, as r1_hit), mat_type of the sphere;
 *                rays_out[i] = {hit point, FLT_MAX, scattered direction (unit), 0}; seeds_out[i] the states after the draws.
 *                R1_SCATTER_ABSORBED: Metal whose scattered direction points below the surface (rayweek1.cpp:432): weight 0.
 *                R1_SCATTER_SCATTERED: otherwise; weight = the albedo for Lambertian and Metal, exactly 1.0f for Dielectric.
 * THE FOLD.  Run levels 0 .. B on the rays still alive: level 0 without the flag, every later level with it on the previous level's
 * rays_out / seeds_out.  Count one ray per level whose event is not NONE.  SKY ends the path with col = weight, then col = w_e * col per
 * channel over the SCATTERED weights of the path from the last to the first; ABSORBED ends it black; SCATTERED at level B ends it black.
 * The result is r1_trace_rays(max_bounces = B)'s {r, g, b, rays}, bit for bit (a Dielectric's 1.0f multiplies exactly), and over
 * r1_camera_rays' output r1_render_samples' records.
 * Variants, refusals and argument order are the ray queries': R1_EINVAL for a NULL ctx, then for flags with unknown bits, then a variant
 * that serves no rays, then before the first r1_set_scene and for GRID after an update until r1_regrid; then n == 0 is R1_OK; then NULL
 * pointers.  A step changes no state another entry point sees and uses no per-context workspace but the launch's cursor: several scatter
 * launches of one context may be in flight. */
typedef struct r1_scatter
{
    float weight[3];   /* see the events */
    int32_t event;     /* R1_SCATTER_* */
    float t;           /* hit distance; FLT_MAX without a hit */
    int32_t index;     /* SCENE index of the hit sphere, -1 without a hit */
    uint32_t mat_type; /* R1_MAT_* of the hit sphere, R1_MAT_NONE without a hit */
    uint32_t pad;      /* written as 0 */
} r1_scatter; /* 32 bytes */

enum
{
    R1_SCATTER_SCATTERED = 0,
    R1_SCATTER_SKY = 1,
    R1_SCATTER_ABSORBED = 2,
    R1_SCATTER_NONE = 3
};
enum
{
    R1_SCATTER_UNIT_DIRECTIONS = 1 /* flags: the directions are unit vectors already (a previous step's rays_out) */
};

/* Host memory in and out, synchronous, R1_TRACE_CHUNK rays at a time (128 bytes per ray of a chunk in the cached workspace). */
int r1_scatter_rays(r1_context *ctx, int32_t variant, int32_t flags, const r1_ray *rays, const r1_sample_seed *seeds, size_t n,
                    r1_ray *rays_out, r1_sample_seed *seeds_out, r1_scatter *out);

/* The same over DEVICE memory: enqueues on `hip_stream` (NULL = the context's stream) and waits for nothing.  Every pointer 16-byte
 * aligned; d_seeds may be NULL.  d_rays_out == d_rays and d_seeds_out == d_seeds (in place) are allowed; any other overlap of an output
 * with an input or with another output is R1_EINVAL, and nothing is enqueued. */
int r1_scatter_rays_device(r1_context *ctx, int32_t variant, int32_t flags, const void *d_rays, const void *d_seeds, size_t n,
                           void *d_rays_out, void *d_seeds_out, void *d_out, void *hip_stream);

/* The same without a device, through the very level r1_trace_rays_host is the fold of.  The checker of the two forms above. */
int r1_scatter_rays_host(const r1_scene *scene, int32_t flags, const r1_ray *rays, const r1_sample_seed *seeds, size_t n,
                         r1_ray *rays_out, r1_sample_seed *seeds_out, r1_scatter *out);

/* ---- host-side helpers of the drop-in (no GPU needed) ------------------------------ */

/* Shape of the spatial index R1_VARIANT_BVH uses (r1_bvh.cpp; the reference has no such
 * structure, README.md:163).  Builds it on the host exactly as r1_set_scene does.  Optional
 * outputs: `nodes_out` receives 16 floats per inner node {m0x m1x m0y m1y | m0z m1z e0x e1x |
 * e0y e1y e0z e1z | A K child0 child1} (child i: box centre m_i, half extent e_i, both inflated
 * per ray by A |o - info.centre|^2 + K, or A |m_0 + m_1 - 2 o|^2 + K if info.pad_local; reference:
 * bit 31 = leaf, then bits 28..30 = number of sphere PAIRS and bits 0..27 the first pair; else
 * inner node index), `ids_out[2 * pair + {0, 1}]` the scene index of each leaf sphere
 * (0xFFFFFFFF = the empty partner of an odd sphere); needs 2 * info.pairs entries.
 * leaf_max <= 0 selects the build's default spheres per leaf. */
typedef struct r1_bvh_info
{
    int32_t nodes, leaves, depth, stack_entries, spheres, pairs;
    float centre[3];   /* C of the kernel's box inflation pad = A |o - C|^2 + K (r1_bvh.cpp) */
    int32_t pad_local; /* 1: the tree uses pad = A |m0 + m1 - 2 o|^2 + K instead (scenes of small spheres) */
    int32_t root_leaf; /* 1 / 2: child 0 / 1 of the root is a leaf of <= 2 sphere pairs and the other child an inner node — the kernels test
                          that leaf and the other child's box once per ray outside the walk's loops; 0: the root has no such shape */
    int32_t flat_axis; /* 0 / 1 / 2: along this axis every box the walk's node loop tests (the child boxes of every inner node but a root of the
                          root-step shape) lies in the slab [flat_m - flat_e, flat_m + flat_e], which is at most 1.25 x as wide as the
                          narrowest of them; the small-scene tree kernels test that slab once per ray instead of each box's own (axis 1: y).
                          -1: no such axis (and always for pad_local trees and trees beyond the small-scene kernels' limits) */
    float flat_m, flat_e;
} r1_bvh_info;
int r1_bvh_describe(const r1_scene *scene, int32_t leaf_max, r1_bvh_info *info, float *nodes_out, size_t nodes_cap, uint32_t *ids_out,
                    size_t ids_cap);

/* The CPU-side pin of the refit's arithmetic (no GPU): builds the tree of `built` exactly as r1_set_scene does, refits it on the host —
 * the device refit's steps over the same topology tables, in r1_bvh_fill.h's arithmetic — to the scene-indexed centres x, y, z
 * (built->count entries each; entries of spheres that are not active are ignored, a non-finite centre leaves its sphere out of every
 * box) and returns the node rows.  The ids are those of r1_bvh_describe(built); info->flat_axis is -1.  A child without a sphere in it
 * (an empty leaf, or a subtree whose centres are all non-finite) has half extents -inf.  R1_EINVAL for NULL built, info, x, y or z. */
int r1_bvh_refit_describe(const r1_scene *built, const float *x, const float *y, const float *z, int32_t leaf_max, r1_bvh_info *info,
                          float *nodes_out, size_t nodes_cap);

/* The same with scene-indexed radii as well (radius_sq and inv_radius, built->count entries each; both NULL: the built scene's): the pin of
 * r1_update_spheres*' refit.  Each pair is taken as the device's set kernel writes it: one that would make its sphere inactive leaves the
 * sphere never hittable, a point in its boxes. */
int r1_bvh_refit_describe_spheres(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                                  const float *inv_radius, int32_t leaf_max, r1_bvh_info *info, float *nodes_out, size_t nodes_cap);

/* The CPU-side pin of r1_resort_spheres (no GPU): builds the tree of `built`, re-deals its movable spheres for the scene-indexed centres
 * and radii (as r1_bvh_refit_describe_spheres takes them; radius_sq and inv_radius both NULL: the built scene's) by the device's steps
 * over the same tables (csrc/r1_bvh_sort.h), refits, and returns the node rows and the leaf slots (scene indices, 0xFFFFFFFF: empty, as
 * r1_bvh_describe).  Pinned and empty slots are those of r1_bvh_describe(built); info->flat_axis is -1. */
int r1_bvh_resort_describe(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                           const float *inv_radius, int32_t leaf_max, r1_bvh_info *info, float *nodes_out, size_t nodes_cap, uint32_t *ids_out,
                           size_t ids_cap);

/* Diagnostic, synchronous: the node rows of the context's tree as the device holds them (16 floats per node, as r1_bvh_describe), after
 * waiting for the context's stream (an update enqueued on another stream is the caller's to wait for).  *nodes receives the number of
 * nodes; nodes_out may be NULL (the count alone), else nodes_cap >= 16 * *nodes floats (R1_ELIMIT otherwise).  Before any update it
 * equals r1_bvh_describe, after one r1_bvh_refit_describe, bit for bit. */
int r1_bvh_download(r1_context *ctx, float *nodes_out, size_t nodes_cap, size_t *nodes);

/* Shape of the uniform grid R1_VARIANT_GRID uses (r1_grid.cpp), built on the host exactly as the render path builds it.  Optional
 * outputs: `start_out` the cells' CSR offsets (cells[0] * cells[1] * cells[2] + 1 entries; cell (jx, jy, jz) is
 * (jz * cells[1] + jy) * cells[0] + jx), `ids_out` the registered spheres of each cell (`registrations` entries, scene indices, ascending
 * within a cell), `outliers_out` the spheres every ray tests before the walk (`outliers` entries, scene indices). */
typedef struct r1_grid_info
{
    float lo[3], hi[3];     /* the grid's box: cell j of axis a spans [lo + j cell, lo + (j + 1) cell] */
    int32_t cells[3];       /* cells per axis (a flat axis has one) */
    float cell[3];          /* cell size per axis */
    float pad;              /* registration pad: the largest rho_i - r_i of a registered sphere (its ball of radius rho_i is registered) */
    float v_safe;           /* V: the grid is exact for rays whose origin lies within V of every registered centre; the others take the
                               tree walk (plays the part of a t_safe, see r1_grid.cpp) */
    float centre_lo[3], centre_hi[3]; /* box of the registered centres (the fallback test: farthest point of it from the origin > V) */
    int32_t spheres;        /* active spheres */
    int32_t outliers;       /* spheres tested by every ray */
    int32_t registrations;  /* entries of all cells together */
    int32_t max_occupancy;  /* most spheres in one cell */
    float build_ms;         /* host time of the build */
} r1_grid_info;
int r1_grid_describe(const r1_scene *scene, r1_grid_info *info, uint32_t *start_out, size_t start_cap, uint32_t *ids_out, size_t ids_cap,
                     uint32_t *outliers_out, size_t outliers_cap);

/* One ray through the grid on the host, in the kernel's own arithmetic (r1_grid_dda.h) and with its stopping rule: `presented`
 * receives (up to `cap`) the scene indices of the spheres given to the per-sphere test, in order — the outliers, then the walked
 * cells' lists — and *n_presented their number; *hit_index / *hit_t the final hit (minimum offer, ties to the lowest index; -1 and
 * FLT_MAX for none); *fallback = 1 if the ray takes the tree walk instead (its hit is then the exhaustive minimum, which that walk
 * returns).  Builds the grid on every call.  No GPU needed. */
int r1_grid_visit(const r1_scene *scene, const float o[3], const float d[3], uint32_t *presented, size_t cap, size_t *n_presented,
                  int32_t *hit_index, float *hit_t, int32_t *fallback);

/* ---- regrid: moved spheres re-registered in the uniform grid ---- */

/* Every update and r1_resort_spheres leave the uniform grid stale: GRID, GRID_STATS and a GRID query return R1_EINVAL ("the scene has
 * moved").  This call re-registers the spheres the device holds in the grid, on the device, by the rule "geometry kept": the PLAN of the
 * grid built for the arrays of r1_set_scene stays — which axes are flat, the cells of the others, V, the margins, the outlier radius — and
 * every sphere is an outlier (its radius, its ball outside the plan's box, or too many cells) or registered in the cells its ball overlaps;
 * a flat axis's one cell is re-stretched over the spheres.  Enqueued on `hip_stream` (NULL: the context's stream); nothing is read back.
 * Afterwards renders and queries through GRID and GRID_STATS are accepted again and bit-identical — pixels, ray counts, records — to a
 * fresh context after r1_set_scene with the context's current spheres, until the next update or re-sort; PREFILTER, STATS and WAVEFRONT
 * stay refused.  It is not an update: the flat slab, a progressive accumulation, r1_last_launch_info / r1_last_timing stay as they are;
 * "one update at a time per context" holds for it.  A pure function of the plan and the device's rows: a second call changes no byte.
 * The id table has a fixed capacity, twice the plan's registrations + 64 (from the first regrid of a scene on; a scene whose 16-bit
 * tables no longer fit the small kernel's LDS then runs the big-scene kernel).  Spheres that would register beyond it leave the grid
 * in OVERFLOW: every ray takes the tree fallback — still exact, only slow — until a later regrid fits; r1_grid_download reports it.
 * R1_EINVAL before the first r1_set_scene.  On a scene that has not moved it builds the grid as the first GRID render would, then
 * re-registers.  On a moved scene whose grid was never built: R1_EINVAL — call r1_regrid once, or render once through the grid, before
 * the first update (the plan can only come from the arrays r1_set_scene received).  There is no r1_multi form. */
int r1_regrid(r1_context *ctx, void *hip_stream);

/* Diagnostic, synchronous: the grid as the device holds it, after waiting for the device; `info` and the optional outputs as
 * r1_grid_describe fills them (build_ms 0).  Overflow is reported as info->registrations = -1 (every start is then 0, no ids).
 * R1_EINVAL while the context holds no current grid (never built, or stale); R1_ELIMIT if a given capacity is too small. */
int r1_grid_download(r1_context *ctx, r1_grid_info *info, uint32_t *start_out, size_t start_cap, uint32_t *ids_out, size_t ids_cap,
                     uint32_t *outliers_out, size_t outliers_cap);

/* The CPU-side pin of r1_regrid (no GPU): the plan of the grid of `built`, then the device's steps over the scene-indexed centres and
 * radii (as r1_bvh_refit_describe_spheres takes them; radius_sq and inv_radius both NULL: the built scene's) through the same functions
 * (csrc/r1_grid_fill.h).  Outputs as r1_grid_describe; overflow as r1_grid_download reports it. */
int r1_grid_regrid_describe(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                            const float *inv_radius, r1_grid_info *info, uint32_t *start_out, size_t start_cap, uint32_t *ids_out,
                            size_t ids_cap, uint32_t *outliers_out, size_t outliers_cap);

/* r1_grid_visit through the tables r1_grid_regrid_describe returns, against the moved spheres. */
int r1_grid_regrid_visit(const r1_scene *built, const float *x, const float *y, const float *z, const float *radius_sq,
                         const float *inv_radius, const float o[3], const float d[3], uint32_t *presented, size_t cap, size_t *n_presented,
                         int32_t *hit_index, float *hit_t, int32_t *fallback);

enum
{
    R1_SCENE_SMALL = 0,  /* create_small_scene   rayweek1.cpp:552 */
    R1_SCENE_MEDIUM = 1, /* create_medium_scene  rayweek1.cpp:582 */
    R1_SCENE_LARGE = 2,  /* create_large_scene   rayweek1.cpp:654 */
    R1_SCENE_GRID = 3    /* build-defined: the large generator scaled to grid_w x grid_h spheres */
};

typedef struct r1_host_scene r1_host_scene; /* owns the arrays an r1_scene points to */

/* Builds one of the reference scenes for an image of width x height (the aspect the
 * reference takes from SCREEN_W/SCREEN_H, rayweek1.cpp:564).  grid_w/grid_h are only
 * used by R1_SCENE_GRID (0 = the reference's 30 x 16). */
int r1_host_scene_create(int kind, int32_t width, int32_t height, int32_t grid_w, int32_t grid_h, r1_host_scene **out);
void r1_host_scene_destroy(r1_host_scene *hs);
const r1_scene *r1_host_scene_spheres(const r1_host_scene *hs);
const r1_camera *r1_host_scene_camera(const r1_host_scene *hs);
/* The arguments the scene builder gave Camera::init (rayweek1.cpp:564, :595, :666), so that a caller can move the reference's
 * own camera; the aspect is the width / height the scene was created for. */
int r1_host_scene_view(const r1_host_scene *hs, float lookfrom[3], float lookat[3], float vup[3], float *vfov_degrees, float *aperture,
                       float *focus_dist);

/* Camera::init (rayweek1.cpp:366-379) in the reference's arithmetic — tan evaluated in double and rounded once, which is what the
 * reference's optimised builds contain.  Host only.  R1_EINVAL for NULL pointers; otherwise it computes
 * what that arithmetic computes, NaNs included (lookfrom == lookat, vup parallel to the view direction). */
int r1_camera_look_at(const float lookfrom[3], const float lookat[3], const float vup[3], float vfov_degrees, float aspect, float aperture,
                      float focus_dist, r1_camera *out);

/* tga_write_rgb24 (common.h:86-122): writes a 24-bit TGA and, like the reference,
 * leaves `pixels` with R and B swapped.  Returns R1_OK or R1_EINVAL if the file
 * cannot be opened. */
int r1_tga_write_rgb24(const char *filename, int32_t width, int32_t height, uint8_t *pixels);

/* Beside it, for a linear frame: a PFM file — the header "PF\n<width> <height>\n-1.0\n", then the rows from the bottom up as
 * little-endian fp32 RGB, which is this library's row order: nothing is flipped, `pixels` is not changed.  R1_OK, or R1_EINVAL for a
 * NULL or empty argument or a file that cannot be written. */
int r1_pfm_write_rgb32f(const char *filename, int32_t width, int32_t height, const float *pixels);

/* log_results (common.h:47-77): writes out_<scene>.txt as
 * `version|%.3fs|%llu|%0.3f mrays/s|` averaged over the runs. */
int r1_log_results(const char *version, const char *scene, const double *elapsed_seconds, const uint64_t *num_rays,
                   int32_t num_runs);

#ifdef __cplusplus
}
#endif

#endif /* RAYS1_H */
