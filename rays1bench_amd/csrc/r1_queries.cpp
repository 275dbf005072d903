// r1_queries.cpp — ray queries: closest hit and occlusion for caller-supplied rays through the context's tree or grid.

#include <string.h>

#include <algorithm>

#include "r1_context.h"


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

// ---- path queries (include/rays1.h "path queries", r1_trace_rays.hip) ------------------------------------------------------

static_assert(sizeof(r1_sample_seed) == 16 && sizeof(r1_radiance) == 16, "the path-query kernels read and write these layouts as one 16-byte word");
static_assert(R1_TRACE_CHUNK == R1_CAST_CHUNK, "r1_trace_rays works in the ray queries' workspace: 64 bytes per ray of a chunk");

// the checks every trace entry point makes before it touches anything, in cast_check's order
static int trace_check(const char *who, r1_context *c, int32_t variant, int32_t max_bounces, int *structure)
{
    if (!c)
    {
        r1_set_error("%s: ctx is NULL", who);
        return R1_EINVAL;
    }
    switch (variant)
    {
    case R1_VARIANT_DEFAULT:
    case R1_VARIANT_BVH: *structure = R1_V_TREE; break;
    case R1_VARIANT_GRID: *structure = R1_V_GRID; break;
    case R1_VARIANT_REFERENCE: *structure = R1_V_REFERENCE; break;
    default:
        r1_set_error("%s: variant %d traces no rays (DEFAULT, BVH, GRID and REFERENCE do)", who, variant);
        return R1_EINVAL;
    }
    if (max_bounces < 1 || max_bounces > R1_MAX_BOUNCES_LIMIT)
    {
        r1_set_error("%s: max_bounces %d is not in 1..%d", who, max_bounces, R1_MAX_BOUNCES_LIMIT);
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

// Enqueues the trace of n rays (device memory; d_seeds may be null: ray i is then seeded as ray first + i of the call) on `st`; waits for nothing.  As cast_enqueue: none of the state a render
// reads is touched.  The attenuation stack is the context's: one trace launch in flight per context (launches on one stream follow each other).
static int trace_enqueue(r1_context *c, int structure, int32_t max_bounces, const void *d_rays, const void *d_seeds, size_t first, size_t n, void *d_out, hipStream_t st)
{
    int rc;
    R1_HIP(hipSetDevice(c->device));
    if (c->n_active == 0)
        structure = R1_V_REFERENCE; // (no sphere can be hit: the reference form's loop of zero trips gives every path the sky; there is no tree to stage)
    if (structure == R1_V_GRID && (rc = ensure_grid(c)))
        return rc;
    const bool big = big_scene(c, structure == R1_V_TREE, structure == R1_V_GRID, false);

    R1TraceRaysArgs a;
    memset(&a, 0, sizeof(a));
    fill_scene(c, a.t.scene);
    if (structure == R1_V_GRID) // (the grid's fallback walks the tree from its root, read from global memory: no root step)
        a.t.scene.bvh_root_leaf = 0u;
    fill_walk(c, structure == R1_V_TREE, big, R1_BVH_TOP_NODES, a.t);
    if (structure == R1_V_GRID)
        a.t.grid = (const R1GridArgs *)(big ? c->grid_dev32.p : c->grid_dev.p);
    a.t.max_bounces = max_bounces;
    const size_t dyn_lds = r1_walk_lds(structure, big, a.t.bvh_depth, a.t.bvh_lds_f4, c->grid_args.lds_bytes);
    int &occ = c->trace_occupancy[(structure == R1_V_TREE ? 0 : structure == R1_V_GRID ? 2 : 4) + (big ? 1 : 0)];
    if (occ == 0)
        R1_HIP(r1_trace_rays_occupancy(structure, big ? 1 : 0, dyn_lds, &occ));
    const int per_cu = occ < 1 ? 1 : (occ > 8 ? 8 : occ);
    if ((rc = ensure(c->cast_cursors, (size_t)R1_CAST_CURSORS * 128)))
        return rc;
    for (size_t at = 0; at < n; at += R1_CAST_LAUNCH_MAX)
    {
        const uint32_t m = (uint32_t)std::min<size_t>(n - at, R1_CAST_LAUNCH_MAX);
        a.rays = (const float4 *)((const char *)d_rays + at * sizeof(r1_ray));
        a.seeds = d_seeds ? (const uint4 *)((const char *)d_seeds + at * sizeof(r1_sample_seed)) : nullptr;
        a.out = (float4 *)((char *)d_out + at * sizeof(r1_radiance));
        a.n = m;
        a.first = (uint32_t)(first + at);
        // persistent, sized as a cast: as many workgroups as the chip holds, fewer where the rays run out; 64 .. 256 rays per claim
        const uint32_t blocks = (uint32_t)std::min<size_t>((size_t)c->cus * per_cu, ((size_t)m + R1_BLOCK - 1) / R1_BLOCK);
        const uint32_t share = m / (blocks * (R1_BLOCK / 64) * 8u);
        a.claim = std::min(256u, std::max(64u, (share + 63u) & ~63u));
        a.gstride = blocks * R1_BLOCK;
        if ((rc = ensure(c->trace_stack, (size_t)max_bounces * a.gstride * 4)))
            return rc;
        a.t.gstack = (uint32_t *)c->trace_stack.p;
        a.cursor = (uint32_t *)((char *)c->cast_cursors.p + 128 * (c->cast_cursor_next++ % R1_CAST_CURSORS));
        R1_HIP(hipMemsetAsync(a.cursor, 0, 4, st));
        R1_HIP(r1_launch_trace_rays(&a, structure, big ? 1 : 0, (int)blocks, dyn_lds, st));
    }
    return R1_OK;
}

extern "C" int r1_trace_rays_device(r1_context *c, int32_t variant, int32_t max_bounces, const void *d_rays, const void *d_seeds, size_t n, void *d_out,
                                    void *hip_stream)
{
    int structure = 0;
    int rc = trace_check("r1_trace_rays_device", c, variant, max_bounces, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!d_rays || !d_out || ((uintptr_t)d_rays & 15u) || ((uintptr_t)d_seeds & 15u) || ((uintptr_t)d_out & 15u))
    {
        r1_set_error("r1_trace_rays_device: d_rays and d_out must be non-NULL device memory, and they and d_seeds 16-byte aligned");
        return R1_EINVAL;
    }
    return trace_enqueue(c, structure, max_bounces, d_rays, d_seeds, 0, n, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_trace_rays(r1_context *c, int32_t variant, int32_t max_bounces, const r1_ray *rays, const r1_sample_seed *seeds, size_t n, r1_radiance *out)
{
    int structure = 0;
    int rc = trace_check("r1_trace_rays", c, variant, max_bounces, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!rays || !out)
    {
        r1_set_error("r1_trace_rays: rays and out must not be NULL with n > 0");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    // one chunk's rays, seeds and records (32 + 16 + 16 bytes per ray) in the ray queries' workspace: device memory stays bounded for any n
    const size_t chunk = std::min<size_t>(n, R1_TRACE_CHUNK);
    if ((rc = ensure(c->cast_ws, chunk * 64)))
        return rc;
    char *const d_rays = (char *)c->cast_ws.p, *const d_seeds = d_rays + chunk * 32, *const d_out = d_seeds + chunk * 16;
    for (size_t at = 0; at < n; at += chunk)
    {
        const size_t m = std::min(chunk, n - at);
        R1_HIP(hipMemcpyAsync(d_rays, rays + at, m * sizeof(r1_ray), hipMemcpyHostToDevice, c->stream));
        if (seeds)
            R1_HIP(hipMemcpyAsync(d_seeds, seeds + at, m * sizeof(r1_sample_seed), hipMemcpyHostToDevice, c->stream));
        if ((rc = trace_enqueue(c, structure, max_bounces, d_rays, seeds ? d_seeds : nullptr, at, m, d_out, c->stream)))
            return rc;
        R1_HIP(hipMemcpyAsync(out + at, d_out, m * sizeof(r1_radiance), hipMemcpyDeviceToHost, c->stream));
        R1_HIP(hipStreamSynchronize(c->stream)); // (the next chunk reuses the workspace)
    }
    return R1_OK;
}
