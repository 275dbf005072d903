// r1_queries.cpp — caller-supplied rays through the context's tree or grid: the ray queries (closest hit and occlusion; include/rays1.h
// "ray queries"), the path queries (radiance; "path queries", §4.22) and the scatter queries (one color() level; "scatter
// queries", §4.34).  All are jobs of the kernels of r1_query_kernels.hip and share the checks, the launch plan and the chunked loop of the
// host-memory forms below.  Feature frames ("feature frames", §4.38) are a fourth job through the same checks and plan: a query whose rays
// are the frame's own.  r1_camera_rays_device, the generator of device-resident rays, stands at the end.

#include <string.h>

#include <algorithm>

#include "r1_context.h"

static_assert(sizeof(r1_ray) == 32 && sizeof(r1_hit) == 32, "the cast job reads and writes these layouts as two float4");
static_assert(sizeof(r1_sample_seed) == 16 && sizeof(r1_radiance) == 16, "the path job reads and writes these layouts as one 16-byte word");
static_assert(R1_TRACE_CHUNK == R1_CAST_CHUNK, "r1_trace_rays and r1_scatter_rays work in the ray queries' workspace, through the same loop: 64 / 128 bytes per ray of a chunk");
static_assert(sizeof(r1_scatter) == 32, "the scatter job writes this layout as two float4");
static_assert(sizeof(r1_feature) == 32, "the feature job writes this layout as two float4");

// The checks every entry point makes before it touches anything; `extra` is the cast's mode, the trace's max_bounces or the step's flags, tested
// where each job has always tested it: the mode and the flags before the variant, the bounces after.  *structure: what the rays walk — R1_V_TREE, R1_V_GRID or
// R1_V_REFERENCE.
static int query_check(const char *who, int job, r1_context *c, int32_t variant, int32_t extra, int *structure)
{
    if (!c)
    {
        r1_set_error("%s: ctx is NULL", who);
        return R1_EINVAL;
    }
    if (job == R1_JOB_CAST && extra != R1_CAST_CLOSEST && extra != R1_CAST_ANY)
    {
        r1_set_error("%s: mode %d is neither R1_CAST_CLOSEST nor R1_CAST_ANY", who, extra);
        return R1_EINVAL;
    }
    if (job == R1_JOB_SCATTER && (extra & ~R1_SCATTER_UNIT_DIRECTIONS))
    {
        r1_set_error("%s: flags %d has bits other than R1_SCATTER_UNIT_DIRECTIONS", who, extra);
        return R1_EINVAL;
    }
    switch (variant)
    {
    case R1_VARIANT_DEFAULT:
    case R1_VARIANT_BVH: *structure = R1_V_TREE; break;
    case R1_VARIANT_GRID: *structure = R1_V_GRID; break;
    case R1_VARIANT_REFERENCE: *structure = R1_V_REFERENCE; break;
    default:
        r1_set_error("%s: variant %d %s no rays (DEFAULT, BVH, GRID and REFERENCE do)", who, variant,
                     job == R1_JOB_CAST ? "casts" : job == R1_JOB_PATH ? "traces" : job == R1_JOB_SCATTER ? "scatters" : "walks");
        return R1_EINVAL;
    }
    if (job == R1_JOB_PATH && (extra < 1 || extra > R1_MAX_BOUNCES_LIMIT))
    {
        r1_set_error("%s: max_bounces %d is not in 1..%d", who, extra, R1_MAX_BOUNCES_LIMIT);
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("%s: no scene set (call r1_set_scene first)", who);
        return R1_EINVAL;
    }
    if (c->moved && *structure == R1_V_GRID && !c->grid_valid) // (a grid r1_regrid re-registered serves)
    {
        r1_set_error("%s: the scene has moved (r1_update_centers) and the uniform grid was not refitted; r1_set_scene rebuilds it", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------------------------
// What a query of either job launches with: made once per call (query_plan), then walked launch by launch (query_slice).
struct QueryPlan
{
    int job = 0, structure = 0, plain = 0; // plain: the tuning library's plain form of the tree cast (r1_query_kernels.hip), for measuring
    bool big = false;
    R1TraceArgs t;      // what the walks read: scene tables, bvh_lds_f4, bvh_depth, grid (everything else zero)
    size_t dyn_lds = 0;
    int per_cu = 1;     // workgroups a CU holds
};

// one launch of a plan: rays [at, at + n) of the call
struct QuerySlice
{
    size_t at = 0;
    uint32_t n = 0, blocks = 0, claim = 0;
    uint32_t *cursor = nullptr;
};

static hipError_t query_occupancy(const QueryPlan &P, int *occ)
{
    return P.job == R1_JOB_CAST       ? r1_cast_occupancy(P.structure, P.big, P.plain, P.dyn_lds, occ)
           : P.job == R1_JOB_PATH     ? r1_trace_rays_occupancy(P.structure, P.big, P.dyn_lds, occ)
           : P.job == R1_JOB_FEATURES ? r1_features_occupancy(P.structure, P.big, P.dyn_lds, occ)
                                      : r1_scatter_rays_occupancy(P.structure, P.big, P.dyn_lds, occ);
}

// Waits for nothing (the first grid query after r1_set_scene builds the grid, as the first grid render does) and touches none of the
// state a render reads: no counter block, no sample records, no launch info, no events.
static int query_plan(r1_context *c, int job, int structure, QueryPlan &P)
{
    int rc;
    R1_HIP(hipSetDevice(c->device));
    if (c->n_active == 0)
        structure = R1_V_REFERENCE; // (no sphere can be hit: the reference form's loop of zero trips writes the misses, or gives every path the sky; there is no tree to stage)
    if (structure == R1_V_GRID && (rc = ensure_grid(c)))
        return rc;
    static const int plain_env = (int)r1_knob("R1_CAST_PLAIN", 0); // tuning library only
    P.job = job, P.structure = structure;
    P.plain = job == R1_JOB_CAST && structure == R1_V_TREE && plain_env ? 1 : 0;
    P.big = big_scene(c, structure == R1_V_TREE, structure == R1_V_GRID, false);
    memset(&P.t, 0, sizeof(P.t));
    fill_scene(c, P.t.scene); // (the sweep's tables ride along: the query kernels read none of them)
    // (the grid's fallback and the plain form walk the tree from its root, read from global memory: no root step)
    if (structure == R1_V_GRID || P.plain)
        P.t.scene.bvh_root_leaf = 0u;
    fill_walk(c, structure == R1_V_TREE && !P.plain, P.big, R1_BVH_TOP_NODES, P.t);
    if (structure == R1_V_GRID)
        P.t.grid = (const R1GridArgs *)(P.big ? c->grid_dev32.p : c->grid_dev.p);
    // (the plain form: a 32-bit traversal stack and no node table)
    P.dyn_lds = P.plain ? (size_t)P.t.bvh_depth * R1_BLOCK * 4 : r1_walk_lds(structure, P.big, P.t.bvh_depth, P.t.bvh_lds_f4, c->grid_args.lds_bytes);
    int &occ = c->query_occupancy[job][(structure == R1_V_TREE ? 0 : structure == R1_V_GRID ? 2 : 4) + (P.big ? 1 : 0)];
    if (occ == 0)
        R1_HIP(query_occupancy(P, &occ));
    P.per_cu = occ < 1 ? 1 : (occ > 8 ? 8 : occ);
    return ensure(c->cast_cursors, (size_t)R1_CAST_CURSORS * 128);
}

// The next launch of n rays; false: none left.  Persistent: as many workgroups as the chip holds, fewer where the rays run out; a wave
// claims 64 .. 256 rays at a time, about an eighth of its share (the waves that finish first take the rest).  The cursors are taken in
// turn, so that launches in flight on different streams do not share one.
// walks: what one item of the launch costs in walks — 1 for a ray; a feature frame's item is a pixel of spp walks, and the eighth of a wave's
// share is counted in walks, so that the tail of a launch — its slowest claim — stays what it is for rays: from spp 4 on that is the
// minimum, one wave-full of 64 pixels.  The minimum is two wave-fulls once the launch fills the chip (more pixels than lanes; below that a
// larger claim would only leave waves without one): a frame of a million pixels is 15 000 claims of 64 on ONE cursor, which sustains ~88 M
// returning atomics a second (tools/ubench_atomic.hip), and the walks of a claim are short.  Measured with R1_FEATURE_CLAIM of the tuning library
// (profiles/r34/features.txt), claims of 64 / 128 / 256 pixels, ms per frame: the large scene at 1200 x 800 x 10 0.349 / 0.331 / 0.415 (tree)
// and 0.289 / 0.260 / 0.302 (grid); config 5's scene at 1920 x 1080 x 4 0.747 / 0.734 / 0.810 (tree) and 0.530 / 0.457 / 0.429 (grid).
static bool query_slice(r1_context *c, const QueryPlan &P, size_t n, QuerySlice &s, uint32_t walks = 1)
{
    s.at += s.n;
    if (s.at >= n)
        return false;
    s.n = (uint32_t)std::min<size_t>(n - s.at, R1_CAST_LAUNCH_MAX);
    s.blocks = (uint32_t)std::min<size_t>((size_t)c->cus * P.per_cu, ((size_t)s.n + R1_BLOCK - 1) / R1_BLOCK);
    const uint32_t waves = s.blocks * (R1_BLOCK / 64);
    const uint32_t share = s.n / (waves * 8u) / walks;
    const uint32_t least = P.job == R1_JOB_FEATURES && s.n / 64u > waves ? 128u : 64u;
    s.claim = std::min(256u, std::max(least, (share + 63u) & ~63u));
    static const uint32_t feature_claim = (uint32_t)r1_knob("R1_FEATURE_CLAIM", 0); // tuning library only
    if (P.job == R1_JOB_FEATURES && feature_claim)
        s.claim = (feature_claim + 63u) & ~63u;
    s.cursor = (uint32_t *)((char *)c->cast_cursors.p + 128 * (c->cast_cursor_next++ % R1_CAST_CURSORS));
    return true;
}

// Enqueues the cast of n rays (device memory) on `st`.
static int cast_enqueue(r1_context *c, int structure, int32_t mode, const void *d_rays, size_t n, void *d_out, hipStream_t st)
{
    QueryPlan P;
    int rc = query_plan(c, R1_JOB_CAST, structure, P);
    if (rc)
        return rc;
    R1CastArgs a;
    memset(&a, 0, sizeof(a));
    a.t = P.t;
    a.active_to_scene = (const uint32_t *)c->active_dev.p;
    a.mode = (uint32_t)mode;
    for (QuerySlice s; query_slice(c, P, n, s);)
    {
        a.rays = (const float4 *)((const char *)d_rays + s.at * sizeof(r1_ray));
        a.out = (char *)d_out + s.at * (mode == R1_CAST_ANY ? 1 : sizeof(r1_hit));
        a.n = s.n, a.claim = s.claim, a.cursor = s.cursor;
        R1_HIP(hipMemsetAsync(a.cursor, 0, 4, st));
        R1_HIP(r1_launch_cast(&a, P.structure, P.big, P.plain, (int)s.blocks, P.dyn_lds, st));
    }
    return R1_OK;
}

// Enqueues the trace of n rays (device memory; d_seeds may be null: ray i is then seeded as ray first + i of the call) on `st`.  The
// attenuation stack is the context's: one trace launch in flight per context (launches on one stream follow each other).
static int trace_enqueue(r1_context *c, int structure, int32_t max_bounces, const void *d_rays, const void *d_seeds, size_t first, size_t n, void *d_out, hipStream_t st)
{
    QueryPlan P;
    int rc = query_plan(c, R1_JOB_PATH, structure, P);
    if (rc)
        return rc;
    R1TraceRaysArgs a;
    memset(&a, 0, sizeof(a));
    a.t = P.t;
    a.t.max_bounces = max_bounces;
    for (QuerySlice s; query_slice(c, P, n, s);)
    {
        a.rays = (const float4 *)((const char *)d_rays + s.at * sizeof(r1_ray));
        a.seeds = d_seeds ? (const uint4 *)((const char *)d_seeds + s.at * sizeof(r1_sample_seed)) : nullptr;
        a.out = (float4 *)((char *)d_out + s.at * sizeof(r1_radiance));
        a.n = s.n, a.claim = s.claim, a.cursor = s.cursor;
        a.first = (uint32_t)(first + s.at);
        a.gstride = s.blocks * R1_BLOCK;
        if ((rc = ensure(c->trace_stack, (size_t)max_bounces * a.gstride * 4)))
            return rc;
        a.t.gstack = (uint32_t *)c->trace_stack.p;
        R1_HIP(hipMemsetAsync(a.cursor, 0, 4, st));
        R1_HIP(r1_launch_trace_rays(&a, P.structure, P.big, (int)s.blocks, P.dyn_lds, st));
    }
    return R1_OK;
}

// Enqueues one level for n rays (device memory; d_seeds may be null, as for a trace) on `st`.  No workspace but the launch's cursor:
// any number of scatter launches of a context may be in flight.
static int scatter_enqueue(r1_context *c, int structure, int32_t flags, const void *d_rays, const void *d_seeds, size_t first, size_t n, void *d_rays_out,
                           void *d_seeds_out, void *d_out, hipStream_t st)
{
    QueryPlan P;
    int rc = query_plan(c, R1_JOB_SCATTER, structure, P);
    if (rc)
        return rc;
    R1ScatterArgs a;
    memset(&a, 0, sizeof(a));
    a.t = P.t;
    a.active_to_scene = (const uint32_t *)c->active_dev.p;
    a.flags = (uint32_t)flags;
    for (QuerySlice s; query_slice(c, P, n, s);)
    {
        a.rays = (const float4 *)((const char *)d_rays + s.at * sizeof(r1_ray));
        a.seeds = d_seeds ? (const uint4 *)((const char *)d_seeds + s.at * sizeof(r1_sample_seed)) : nullptr;
        a.rays_out = (float4 *)((char *)d_rays_out + s.at * sizeof(r1_ray));
        a.seeds_out = (uint4 *)((char *)d_seeds_out + s.at * sizeof(r1_sample_seed));
        a.out = (float4 *)((char *)d_out + s.at * sizeof(r1_scatter));
        a.n = s.n, a.claim = s.claim, a.cursor = s.cursor;
        a.first = (uint32_t)(first + s.at);
        R1_HIP(hipMemsetAsync(a.cursor, 0, 4, st));
        R1_HIP(r1_launch_scatter_rays(&a, P.structure, P.big, (int)s.blocks, P.dyn_lds, st));
    }
    return R1_OK;
}

// one result array of a host-memory form: `each` bytes per ray
struct ChunkOut
{
    void *host;
    size_t each;
};

// The host-memory forms: one chunk's rays, then (seed_each != 0) its seeds, then its results — 64 bytes per ray at the most for a cast or a
// trace, 128 for a step (32 + 16 in, 32 + 32 + 16 out) — in the cached workspace, so device memory stays bounded for any n.
// enqueue(d_rays, d_seeds or null, at, m, d_out[]) launches one chunk on the context's stream; d_out[k] is the chunk's part of outs[k].
template <size_t K, class ENQUEUE>
static int query_chunks(r1_context *c, const r1_ray *rays, const r1_sample_seed *seeds, size_t seed_each, size_t n, const ChunkOut (&outs)[K], ENQUEUE enqueue)
{
    int rc;
    R1_HIP(hipSetDevice(c->device));
    const size_t chunk = std::min<size_t>(n, R1_CAST_CHUNK);
    size_t each = sizeof(r1_ray) + seed_each;
    for (const ChunkOut &o : outs)
        each += (o.each + 15) & ~(size_t)15;
    if ((rc = ensure(c->cast_ws, chunk * std::max<size_t>(each, 64))))
        return rc;
    char *const d_rays = (char *)c->cast_ws.p, *const d_seeds = d_rays + chunk * sizeof(r1_ray);
    char *d_out[K];
    d_out[0] = d_seeds + chunk * seed_each;
    for (size_t k = 1; k < K; ++k)
        d_out[k] = d_out[k - 1] + chunk * ((outs[k - 1].each + 15) & ~(size_t)15);
    for (size_t at = 0; at < n; at += chunk)
    {
        const size_t m = std::min(chunk, n - at);
        R1_HIP(hipMemcpyAsync(d_rays, rays + at, m * sizeof(r1_ray), hipMemcpyHostToDevice, c->stream));
        if (seeds)
            R1_HIP(hipMemcpyAsync(d_seeds, seeds + at, m * seed_each, hipMemcpyHostToDevice, c->stream));
        if ((rc = enqueue(d_rays, seeds ? d_seeds : nullptr, at, m, d_out)))
            return rc;
        for (size_t k = 0; k < K; ++k)
            R1_HIP(hipMemcpyAsync((char *)outs[k].host + at * outs[k].each, d_out[k], m * outs[k].each, hipMemcpyDeviceToHost, c->stream));
        R1_HIP(hipStreamSynchronize(c->stream)); // (the next chunk reuses the workspace)
    }
    return R1_OK;
}

// ---- ray queries -------------------------------------------------------------------------------------------------------------------------

extern "C" int r1_cast_rays_device(r1_context *c, int32_t variant, int32_t mode, const void *d_rays, size_t n, void *d_out, void *hip_stream)
{
    int structure = 0;
    int rc = query_check("r1_cast_rays_device", R1_JOB_CAST, c, variant, mode, &structure);
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
    int rc = query_check("r1_cast_rays", R1_JOB_CAST, c, variant, mode, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!rays || !out)
    {
        r1_set_error("r1_cast_rays: rays and out must not be NULL with n > 0");
        return R1_EINVAL;
    }
    const ChunkOut outs[1] = {{out, mode == R1_CAST_ANY ? (size_t)1 : sizeof(r1_hit)}};
    return query_chunks(c, rays, nullptr, 0, n, outs, [=](const void *d_rays, const void *, size_t, size_t m, char *const *d_out) {
        return cast_enqueue(c, structure, mode, d_rays, m, d_out[0], c->stream);
    });
}

// ---- path queries ------------------------------------------------------------------------------------------------------------------------

extern "C" int r1_trace_rays_device(r1_context *c, int32_t variant, int32_t max_bounces, const void *d_rays, const void *d_seeds, size_t n, void *d_out,
                                    void *hip_stream)
{
    int structure = 0;
    int rc = query_check("r1_trace_rays_device", R1_JOB_PATH, c, variant, max_bounces, &structure);
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
    int rc = query_check("r1_trace_rays", R1_JOB_PATH, c, variant, max_bounces, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!rays || !out)
    {
        r1_set_error("r1_trace_rays: rays and out must not be NULL with n > 0");
        return R1_EINVAL;
    }
    const ChunkOut outs[1] = {{out, sizeof(r1_radiance)}};
    return query_chunks(c, rays, seeds, sizeof(r1_sample_seed), n, outs, [=](const void *d_rays, const void *d_seeds, size_t at, size_t m, char *const *d_out) {
        return trace_enqueue(c, structure, max_bounces, d_rays, d_seeds, at, m, d_out[0], c->stream);
    });
}

// ---- scatter queries ---------------------------------------------------------------------------------------------------------------------

// [a, a + na) and [b, b + nb) share a byte
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

extern "C" int r1_scatter_rays_device(r1_context *c, int32_t variant, int32_t flags, const void *d_rays, const void *d_seeds, size_t n, void *d_rays_out,
                                      void *d_seeds_out, void *d_out, void *hip_stream)
{
    int structure = 0;
    int rc = query_check("r1_scatter_rays_device", R1_JOB_SCATTER, c, variant, flags, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!d_rays || !d_rays_out || !d_seeds_out || !d_out ||
        (((uintptr_t)d_rays | (uintptr_t)d_seeds | (uintptr_t)d_rays_out | (uintptr_t)d_seeds_out | (uintptr_t)d_out) & 15u))
    {
        r1_set_error("r1_scatter_rays_device: d_rays, d_rays_out, d_seeds_out and d_out must be non-NULL device memory, and they and d_seeds 16-byte aligned");
        return R1_EINVAL;
    }
    // in place is d_rays_out == d_rays and d_seeds_out == d_seeds, exactly: a lane reads ray i before it writes ray i.  Anything else that
    // shares bytes lets one lane's result land in a ray another lane has yet to read.
    const size_t nr = n * sizeof(r1_ray), ns = n * sizeof(r1_sample_seed), no = n * sizeof(r1_scatter);
    const struct
    {
        const void *p;
        size_t bytes;
    } in[2] = {{d_rays, nr}, {d_seeds, ns}}, res[3] = {{d_rays_out, nr}, {d_seeds_out, ns}, {d_out, no}};
    bool bad = false;
    for (int o = 0; o < 3; ++o)
    {
        for (int i = 0; i < 2; ++i)
            if (!(o == i && res[o].p == in[i].p) && ranges_overlap(res[o].p, res[o].bytes, in[i].p, in[i].bytes))
                bad = true;
        for (int q = o + 1; q < 3; ++q)
            if (ranges_overlap(res[o].p, res[o].bytes, res[q].p, res[q].bytes))
                bad = true;
    }
    if (bad)
    {
        r1_set_error("r1_scatter_rays_device: an output overlaps an input or another output (d_rays_out == d_rays and d_seeds_out == d_seeds alone are allowed)");
        return R1_EINVAL;
    }
    return scatter_enqueue(c, structure, flags, d_rays, d_seeds, 0, n, d_rays_out, d_seeds_out, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_scatter_rays(r1_context *c, int32_t variant, int32_t flags, const r1_ray *rays, const r1_sample_seed *seeds, size_t n, r1_ray *rays_out,
                               r1_sample_seed *seeds_out, r1_scatter *out)
{
    int structure = 0;
    int rc = query_check("r1_scatter_rays", R1_JOB_SCATTER, c, variant, flags, &structure);
    if (rc)
        return rc;
    if (n == 0)
        return R1_OK;
    if (!rays || !rays_out || !seeds_out || !out)
    {
        r1_set_error("r1_scatter_rays: rays, rays_out, seeds_out and out must not be NULL with n > 0");
        return R1_EINVAL;
    }
    const ChunkOut outs[3] = {{out, sizeof(r1_scatter)}, {rays_out, sizeof(r1_ray)}, {seeds_out, sizeof(r1_sample_seed)}};
    return query_chunks(c, rays, seeds, sizeof(r1_sample_seed), n, outs, [=](const void *d_rays, const void *d_seeds, size_t at, size_t m, char *const *d_out) {
        return scatter_enqueue(c, structure, flags, d_rays, d_seeds, at, m, d_out[1], d_out[2], d_out[0], c->stream);
    });
}

// ---- feature frames ----------------------------------------------------------------------------------------------------
// A query whose rays are the frame's own: the checks, the plan, the slices and the cursors are the queries', an item of a launch is a pixel
// of the window.  Like every query it touches none of the state a render reads.

// The refusals of both forms, in the documented order (NULL ctx; params, region, variant; no scene; then the caller tests `out`).  *win: the
// region the call renders — the caller's, or the whole frame.
static int features_check(const char *who, r1_context *c, const r1_params *p, const r1_region *region, r1_region *win, int *structure)
{
    if (!c)
    {
        r1_set_error("%s: ctx is NULL", who);
        return R1_EINVAL;
    }
    if (!p)
    {
        r1_set_error("%s: params is NULL", who);
        return R1_EINVAL;
    }
    const r1_region whole = {0, 0, p->width, p->height, 0};
    *win = region ? *region : whole;
    int rc = r1_region_check(p, win);
    if (rc)
        return rc;
    return query_check(who, R1_JOB_FEATURES, c, p->variant, 0, structure);
}

// Enqueues window `win` of the frame (r1_region_check has passed it) on `st`: pixel (x, y) of the window at d_out + (y * stride + x) records.
static int features_enqueue(r1_context *c, int structure, const r1_params *p, const r1_region &win, void *d_out, hipStream_t st)
{
    QueryPlan P;
    int rc = query_plan(c, R1_JOB_FEATURES, structure, P);
    if (rc)
        return rc;
    R1FeatureArgs a;
    memset(&a, 0, sizeof(a));
    a.t = P.t;
    a.t.cam = c->cam;
    a.t.width = p->width, a.t.height = p->height, a.t.spp = p->spp, a.t.seed = p->seed;
    a.t.inv_w = 1.0f / p->width, a.t.inv_h = 1.0f / p->height; // rayweek1.cpp:746
    a.t.inv_spp = (float)(1.0f / p->spp);                        // rayweek1.cpp:765
    a.out = (float4 *)d_out;
    a.x0 = (uint32_t)win.x0, a.y0 = (uint32_t)win.y0;
    a.win_w = (uint32_t)win.width, a.div_win_w = make_div(a.win_w);
    a.stride = (uint32_t)(win.out_stride ? win.out_stride : win.width);
    const size_t n = (size_t)win.width * (size_t)win.height;
    for (QuerySlice s; query_slice(c, P, n, s, (uint32_t)p->spp);)
    {
        a.first = (uint32_t)s.at;
        a.n = s.n, a.claim = s.claim, a.cursor = s.cursor;
        R1_HIP(hipMemsetAsync(a.cursor, 0, 4, st));
        R1_HIP(r1_launch_features(&a, P.structure, P.big, (int)s.blocks, P.dyn_lds, st));
    }
    return R1_OK;
}

extern "C" int r1_render_features_device(r1_context *c, const r1_params *p, const r1_region *region, void *d_out, void *hip_stream)
{
    r1_region win;
    int structure = 0;
    int rc = features_check("r1_render_features_device", c, p, region, &win, &structure);
    if (rc)
        return rc;
    if (!d_out || ((uintptr_t)d_out & 15u))
    {
        r1_set_error("r1_render_features_device: d_out must be non-NULL device memory, 16-byte aligned");
        return R1_EINVAL;
    }
    return features_enqueue(c, structure, p, win, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

// The host-memory form: bands of whole rows of the window, R1_CAST_CHUNK pixels at the most, densely in the queries' workspace (32 bytes a
// pixel: device memory stays bounded for any frame), each copied home with the caller's row stride before the next reuses the workspace.
// The device time is taken with events of the call's own: the context's describe the last render.
extern "C" int r1_render_features(r1_context *c, const r1_params *p, const r1_region *region, r1_feature *out, double *device_seconds_out)
{
    r1_region win;
    int structure = 0;
    int rc = features_check("r1_render_features", c, p, region, &win, &structure);
    if (rc)
        return rc;
    if (!out)
    {
        r1_set_error("r1_render_features: out is NULL");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t stride = win.out_stride ? (size_t)win.out_stride : (size_t)win.width;
    const int32_t band_rows = (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)win.height, R1_CAST_CHUNK / (size_t)win.width));
    if ((rc = ensure(c->cast_ws, (size_t)band_rows * win.width * sizeof(r1_feature))))
        return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (device_seconds_out)
    {
        R1_HIP(hipEventCreate(&ev[0]));
        if (hipEventCreate(&ev[1]) != hipSuccess)
        {
            (void)hipEventDestroy(ev[0]);
            r1_set_error("r1_render_features: hipEventCreate failed");
            return R1_EHIP;
        }
    }
    // (from here on nothing returns before the events are destroyed: a failed step ends the loop)
    double seconds = 0.0;
    hipError_t e = hipSuccess;
    for (int32_t y = 0; y < win.height && rc == R1_OK && e == hipSuccess; y += band_rows)
    {
        const int32_t rows = std::min(band_rows, win.height - y);
        const r1_region band = {win.x0, win.y0 + y, win.width, rows, 0};
        if (ev[0])
            e = hipEventRecord(ev[0], c->stream);
        if (e == hipSuccess)
            rc = features_enqueue(c, structure, p, band, c->cast_ws.p, c->stream);
        if (rc == R1_OK && e == hipSuccess && ev[1])
            e = hipEventRecord(ev[1], c->stream);
        if (rc == R1_OK && e == hipSuccess)
            e = hipMemcpy2DAsync(out + (size_t)y * stride, stride * sizeof(r1_feature), c->cast_ws.p, (size_t)win.width * sizeof(r1_feature),
                                 (size_t)win.width * sizeof(r1_feature), (size_t)rows, hipMemcpyDeviceToHost, c->stream);
        if (rc == R1_OK && e == hipSuccess)
            e = hipStreamSynchronize(c->stream); // (the next band reuses the workspace)
        if (rc == R1_OK && e == hipSuccess && ev[0])
        {
            float ms = 0;
            e = hipEventElapsedTime(&ms, ev[0], ev[1]);
            seconds += ms * 1e-3;
        }
    }
    if (ev[0])
        (void)hipEventDestroy(ev[0]), (void)hipEventDestroy(ev[1]);
    if (rc == R1_OK && e != hipSuccess)
    {
        r1_set_error("r1_render_features: %s", hipGetErrorString(e));
        rc = R1_EHIP;
    }
    if (rc == R1_OK && device_seconds_out)
        *device_seconds_out = seconds;
    return rc;
}

// ---- camera rays on the device -------------------------------------------------------------------------------------------------------------

extern "C" int r1_camera_rays_device(r1_context *c, const r1_camera *camera, const r1_params *p, size_t first, size_t n, void *d_rays, void *d_seeds,
                                     void *hip_stream)
{
    if (!c)
    {
        r1_set_error("r1_camera_rays_device: ctx is NULL");
        return R1_EINVAL;
    }
    if (!p || p->width <= 0 || p->height <= 0 || p->spp < 1)
    {
        r1_set_error("r1_camera_rays_device: null params, an empty image or spp < 1");
        return R1_EINVAL;
    }
    if (p->num_shards != 1)
    {
        r1_set_error("r1_camera_rays_device: whole frames only (num_shards %d)", p->num_shards);
        return R1_EINVAL;
    }
    const size_t total = (size_t)p->width * (size_t)p->height * (size_t)p->spp;
    if (first > total || n > total - first)
    {
        r1_set_error("r1_camera_rays_device: samples [%zu, %zu + %zu) reach beyond the frame's %zu", first, first, n, total);
        return R1_EINVAL;
    }
    if (!camera && !c->have_scene)
    {
        r1_set_error("r1_camera_rays_device: no camera given and no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    if (n == 0)
        return R1_OK;
    if (!d_rays || !d_seeds || (((uintptr_t)d_rays | (uintptr_t)d_seeds) & 15u))
    {
        r1_set_error("r1_camera_rays_device: d_rays and d_seeds must be non-NULL device memory, 16-byte aligned");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    R1CameraRaysArgs a;
    memset(&a, 0, sizeof(a));
    a.cam = camera ? device_camera(*camera) : c->cam;
    a.rays = (float4 *)d_rays, a.seeds = (uint4 *)d_seeds;
    a.first = first, a.n = n;
    a.width = p->width, a.spp = p->spp, a.seed = p->seed;
    a.inv_w = 1.0f / p->width, a.inv_h = 1.0f / p->height; // rayweek1.cpp:746
    R1_HIP(r1_launch_camera_rays(&a, hip_stream ? (hipStream_t)hip_stream : c->stream));
    return R1_OK;
}
