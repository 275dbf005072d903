// r1_internal.h — the C-linkage functions of the library that one file defines and another calls, and that include/rays1.h does not declare.
// Included by the file that defines each of them and by every file that calls it: with C linkage a prototype that drifts would still link,
// this way it does not compile.
#ifndef R1_INTERNAL_H
#define R1_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rays1.h"
#include "r1_device.h"

struct R1RefitArgs; // r1_bvh_fill.h
struct R1SetArgs;
struct R1SortArgs; // r1_bvh_sort.h
struct R1RegridArgs; // r1_grid_fill.h
struct R1RadixArgs; // r1_device_sort.h
struct R1VFilterArgs; // r1_denoise.h
struct R1ReprojectArgs; // r1_reproject.h

// what r1_sweep_describe says of the sweep's tables besides the arrays
struct r1_sweep_info
{
    int32_t spheres;   // active spheres
    int32_t groups, multi, n_sweep; // R1Sweep's n_groups, n_multi, n_sweep
    int32_t slots;     // groups the tables hold: n_sweep + the prefetch chunk or tile
    int32_t group_max; // R1_GROUP_MAX
};

extern "C"
{
// r1_capi.cpp
void r1_set_error(const char *fmt, ...);
void *r1_context_stream(r1_context *c); // the context's own stream (r1_multi.cpp runs its collectives on it)
int r1_pick_build(int variant, int big, int want, int *build4); // r1_pick for tests: 1 and build4 = {variant, stats, big, mode}, or 0
void r1_build_facts(int variant, int mode, int big, int *facts6);  // the predicates for tests: {tree, grid, stats, base variant, tp family, runs as latency}

// r1_sweep.cpp: the sweep's tables for tests, as r1_set_scene builds them (buffers: caller's, with capacities in elements; NULL: not wanted)
int r1_sweep_describe(const r1_scene *s, r1_sweep_info *info, double *groups_out, size_t groups_cap, float *sweep_out, size_t sweep_cap,
                      uint32_t *members_out, size_t members_cap, float *exact_g_out, size_t exact_g_cap, uint32_t *active_out, size_t active_cap);

// r1_grid.cpp: the plan a regrid keeps of the grid of `built` (r1_grid_fill.h R1GridPlan), for tests: {V, delta, big, M} and the flat axes
int r1_grid_plan_describe(const r1_scene *built, double *doubles4, int32_t *flat3);

// r1_host.cpp
int r1_params_check(const r1_params *p);

// r1_trace_<family>.hip (r1_trace_tu.inc): the family's builds, by walking its list; hipErrorInvalidValue: not one of them
// (_launch_region: the region twin of a R1_MODE_PASS build, r1_region_kernel)
#define R1_TU_DECL(NAME)                                                                                                       \
    hipError_t r1_tu_##NAME##_launch(const R1TraceArgs *args, R1Build b, int blocks, size_t dyn_lds, hipStream_t stream);     \
    hipError_t r1_tu_##NAME##_launch_region(const R1TraceArgs *args, R1Build b, int blocks, size_t dyn_lds, hipStream_t stream); \
    hipError_t r1_tu_##NAME##_occupancy(R1Build b, size_t dyn_lds, int *blocks_per_cu);
R1_TU_DECL(tree_small)
R1_TU_DECL(tree_big)
R1_TU_DECL(sweep_small)
R1_TU_DECL(sweep_big)
R1_TU_DECL(grid_small)
R1_TU_DECL(grid_big)
#undef R1_TU_DECL
// r1_trace_tree_small.hip: the flat twin of build b (r1_flatwalk_kernel); hipErrorInvalidValue: b has none
hipError_t r1_tu_tree_small_launch_flat(const R1TraceArgs *args, R1Build b, int blocks, size_t dyn_lds, hipStream_t stream);

// r1_aux_kernels.hip: the trace launch and occupancy dispatch, the wavefront variant, the put kernels
hipError_t r1_launch_trace(const R1TraceArgs *args, R1Build b, int blocks, size_t grid_lds, hipStream_t stream, int *walk_form, int region);
hipError_t r1_trace_occupancy(R1Build b, size_t dyn_lds, int *blocks_per_cu);
hipError_t r1_launch_wavefront(R1WaveArgs *w, int blocks, hipStream_t stream);
hipError_t r1_launch_put6(void *dst, const uint32_t *words, hipStream_t stream);
hipError_t r1_launch_put8(void *dst, const uint32_t *words, hipStream_t stream);
hipError_t r1_launch_put_cameras(void *dst, const float *cameras20, int n, hipStream_t stream); // n cameras of 20 floats each, host memory read during the call

// r1_close_kernels.hip: what closes a frame.  max_rows: at most this many rows of workgroups (0: one per tile, up to 65535)
hipError_t r1_launch_resolve(const R1ResolveArgs *args, int max_rows, hipStream_t stream);
hipError_t r1_launch_accum(const R1AccumArgs *args, hipStream_t stream);
hipError_t r1_launch_adapt_accum(const R1AdaptArgs *args, hipStream_t stream);
hipError_t r1_launch_resolve_linear(const R1LinearArgs *args, int max_rows, hipStream_t stream); // linear frames
hipError_t r1_launch_resolve_moments(const R1MomentsArgs *args, int max_rows, hipStream_t stream); // variance frames
hipError_t r1_launch_resolve_region(const R1RegionArgs *args, hipStream_t stream); // region renders
hipError_t r1_launch_accum_linear(const R1ReadoutArgs *args, hipStream_t stream);
hipError_t r1_launch_adapt_compact(const uint32_t *cur, uint32_t n_cur, const R1TileReport *report, uint32_t at_cap, uint32_t *next, uint32_t *count_out,
                                   hipStream_t stream);
hipError_t r1_launch_land_arm(const R1LandArmArgs *args, hipStream_t stream);
hipError_t r1_launch_assemble(const R1AssembleArgs *args, hipStream_t stream);

// r1_query_kernels.hip, the cast job; variant: R1_V_TREE, R1_V_GRID or R1_V_REFERENCE; plain: the tuning library's plain tree form
hipError_t r1_launch_cast(const R1CastArgs *args, int variant, int big, int plain, int blocks, size_t dyn_lds, hipStream_t stream);
hipError_t r1_cast_occupancy(int variant, int big, int plain, size_t dyn_lds, int *blocks_per_cu);

// r1_query_kernels.hip, the path job; variant as for r1_launch_cast
hipError_t r1_launch_trace_rays(const R1TraceRaysArgs *args, int variant, int big, int blocks, size_t dyn_lds, hipStream_t stream);
hipError_t r1_trace_rays_occupancy(int variant, int big, size_t dyn_lds, int *blocks_per_cu);

// r1_query_kernels.hip, the scatter job; variant as for r1_launch_cast
hipError_t r1_launch_scatter_rays(const R1ScatterArgs *args, int variant, int big, int blocks, size_t dyn_lds, hipStream_t stream);
hipError_t r1_scatter_rays_occupancy(int variant, int big, size_t dyn_lds, int *blocks_per_cu);

// r1_query_kernels.hip, the feature job (an item is a pixel); variant as for r1_launch_cast
hipError_t r1_launch_features(const R1FeatureArgs *args, int variant, int big, int blocks, size_t dyn_lds, hipStream_t stream);
hipError_t r1_features_occupancy(int variant, int big, size_t dyn_lds, int *blocks_per_cu);

// r1_denoise_kernels.hip: the kernels of denoised frames and of their variance-guided form (§4.40).  guided: the r1_vfilter
// kernels, which read all of *args; otherwise the r1_denoise kernels, which read args->d alone.  staged: tile and halo through LDS (steps <=
// R1D_STAGE_MAX_STEP, else hipErrorInvalidValue); last: the pass that re-modulates and writes `out`
hipError_t r1_launch_denoise_prepare(const R1VFilterArgs *args, int guided, hipStream_t stream);
hipError_t r1_launch_denoise_pass(const R1VFilterArgs *args, int guided, int staged, int last, hipStream_t stream);

// r1_reproject_kernels.hip: the kernel of accumulated frames
hipError_t r1_launch_reproject(const R1ReprojectArgs *args, hipStream_t stream);
// r1_accumulate_host.cpp: the kernel's arguments from the public structs (the check has passed and left `plan`); what every form refuses of
// the images behind the check — a NULL pointer, an output that is a history image
void r1_accumulate_args(const r1_accumulate_frame *fr, const r1_accumulate_opt *o, const r1_accumulate_view *v, const r1_reproject_plan *plan,
                        const r1_accumulate_images *im, R1ReprojectArgs *a);
int r1_accumulate_images_check(const char *who, const r1_accumulate_images *im);

// r1_aux_kernels.hip: r1_camera_rays_device
hipError_t r1_launch_camera_rays(const R1CameraRaysArgs *args, hipStream_t stream);

// r1_refit.hip: the kernels of r1_update_centers* 
hipError_t r1_launch_refit_move(const R1RefitArgs *a, uint32_t first, uint32_t count, const float *x, const float *y, const float *z, hipStream_t stream);
hipError_t r1_launch_refit_set(const R1RefitArgs *a, const R1SetArgs *s, uint32_t first, uint32_t count, uint32_t groups, hipStream_t stream); // r1_update_spheres* (§4.27)
hipError_t r1_launch_refit(const R1RefitArgs *a, const uint32_t *height_off, uint32_t heights, hipStream_t stream);

// r1_resort.hip: the kernels of r1_resort_spheres
hipError_t r1_launch_resort(const R1SortArgs *a, const uint32_t *depth_off, uint32_t depths, hipStream_t stream);

// r1_regrid.hip: the kernels of r1_regrid
hipError_t r1_launch_regrid(const R1RegridArgs *a, hipStream_t stream);

// r1_device_sort.hip: the prefix sum and the radix sort of both (r1_device_sort.h has the sizes of their scratch)
// exclusive prefix sum of data[0, n) in place, three launches per level; sums: r1_scan_sums_words(n) words of scratch
void r1_scan_enqueue(uint32_t *data, uint32_t n, uint32_t *sums, hipStream_t stream);
// every list of *a sorted by its keys, 8 bits a pass for as long as top_key (no key is larger) has bits left; returns which of the two buffers holds the result
int r1_radix_sort_enqueue(const R1RadixArgs *a, uint32_t top_key, hipStream_t stream);
}

#endif
