// r1_scene.cpp — what a context knows of its scene: r1_set_scene (active spheres, the sweep's tables, the box tree, the refit's tables;
// uploads through the context's own stream), the camera alone, moving spheres, sphere updates, the re-sort, the uniform grid built on
// first use, and the regrid that re-registers moved spheres in it.

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "r1_context.h"
#include "r1_sweep.h"

// ---- R1_VARIANT_DEFAULT -------------------------------------------------------------------------------------------------------------
// DEFAULT is the box tree for every scene: a property of the build, so what a context launches depends on its arguments only and
// the ranks of a multi-GPU job always run the same kernel.  (Round 3 timed scenes of 9..127 spheres through both kernels when
// they were set, because the reference's dense medium scene was 4-5 % faster through the ungrouped sweep in round 2.  Since the
// root step of the walk the tree is ahead on every row of the crossover table, profiles/r04/tree_vs_sweep_crossover*.txt — by
// 0-3 % for one synchronous frame of the medium scene, 7 % with frames in flight — and a probe inside r1_set_scene made the first
// timed benchmark() call, the kernel choice of each rank and a 62 MB workspace depend on a wall-clock race: VERDICT r03 / ADVICE r03.)

// what the kernels read of a camera (Camera::getRay, rayweek1.cpp:381-386, does not use w)
R1DeviceCamera device_camera(const r1_camera &cam)
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
    // (not after r1_update_centers*: the device holds other centres than src_f32, or the groups and the grid are those of other centres;
    // nor after a device-form r1_update_spheres_device of materials, which the host copies never saw)
    if (c->have_scene && !c->moved && !c->src_stale && c->src_mat.size() == s->count && memcmp(&c->src_cam, cam, sizeof(*cam)) == 0 &&
        (s->count == 0 || memcmp(c->src_mat.data(), s->mat_type, s->count) == 0))
    {
        bool same = true;
        for (int k = 0; k < 9 && same; ++k)
            same = s->count == 0 || memcmp(c->src_f32[k].data(), src[k], (size_t)s->count * 4) == 0;
        if (same)
            return R1_OK; // bit-identical scene and camera: everything on the device is current
    }
    c->have_scene = false;
    c->grid_valid = false, c->grid_planned = false, c->regrid_ready = false;

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
    // the sweep's tables (r1_sweep.cpp): sphere groups, their members, the per-sphere rows
    R1Sweep sw;
    r1_build_sweep(s, c->active_to_scene, sw);

    // the optional spatial index over the same active spheres (R1_VARIANT_BVH)
    R1Bvh bvh;
    {
        std::vector<float> fx(na ? na : 1), fy(na ? na : 1), fz(na ? na : 1), fr(na ? na : 1);
        for (uint32_t a = 0; a < na; ++a)
            fx[a] = sw.exact[4 * a + 0], fy[a] = sw.exact[4 * a + 1], fz[a] = sw.exact[4 * a + 2], fr[a] = sw.exact[4 * a + 3];
        static const int leaf_env = (int)r1_knob("R1_BVH_LEAF", 0);
        // leaf size: 4 spheres (2 pairs) on the reference's scenes; 8 on big lattices (measured:
        // 100 004 spheres 3.43 ms against 3.67 ms per 1920x1080x4 frame)
        const int leaf_default = na > R1_MAX_ACTIVE_10BIT ? 2 * R1_BVH_LEAF : R1_BVH_LEAF;
        r1_build_bvh(na, fx.data(), fy.data(), fz.data(), fr.data(), sw.rbound.data(), leaf_env > 0 ? leaf_env : leaf_default, bvh);
        if (bvh.max_depth > R1_BVH_STACK)
        {
            r1_set_error("r1_set_scene: spatial index deeper (%d) than the traversal stack (%d)", bvh.max_depth, R1_BVH_STACK);
            return R1_ELIMIT;
        }
    }
    // what a re-sort needs besides (r1_resort_spheres): which slots are movable and the splitting nodes' segments, computed before the sentinels
    R1SortTopo stopo;
    r1_bvh_sort_topology(bvh, stopo);
    const uint32_t n_ids = (uint32_t)bvh.ids.size();
    // leaf_quad fetches a sphere index speculatively for lanes that hold no flagged sphere (slot 3 of the step, whatever the step's
    // pair count): two sentinel words behind the last pair keep that read inside the table
    bvh.ids.resize(bvh.ids.size() + 2, 0xFFFFFFFFu);
    // ... and the second PAIR of every leaf, whatever the leaf's pair count: behind the table's last leaf, which may hold
    // one pair, that is this sentinel pair — centres 0, both radius_sq = -inf like an odd sphere's partner.  Not part of the tree: no leaf
    // reference counts it, no slot of the refit's tables points at it (r1_bvh_topology is computed from the ids in front of it).
    {
        const float sentinel[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -INFINITY, -INFINITY};
        bvh.prims.insert(bvh.prims.end(), sentinel, sentinel + 8);
    }

    // what a refit needs besides the tree (r1_update_centers*): topology and the radii, once per scene
    R1RefitTopo topo;
    r1_bvh_topology(bvh, na, topo);
    // the most pairs a leaf holds: the kernels that keep the node table in LDS test a leaf in ONE step of two pairs (r1_frame.cpp big_scene)
    uint32_t leaf_pairs = 0;
    for (uint32_t ref : topo.leaf_ref)
        leaf_pairs = std::max(leaf_pairs, (ref >> 28) & 7u);
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
    std::vector<uint32_t> stab;
    size_t soff[4];
    {
        const size_t m = stopo.mov.size();
        soff[0] = 0, soff[1] = m, soff[2] = 2 * m, soff[3] = 2 * m + 3 * stopo.seg.size();
        stab.resize(soff[3] + stopo.pos_seg.size());
        if (m)
            memcpy(&stab[soff[0]], stopo.mov.data(), m * 4), memcpy(&stab[soff[1]], stopo.mslot.data(), m * 4);
        if (!stopo.seg.empty())
            memcpy(&stab[soff[2]], stopo.seg.data(), stopo.seg.size() * sizeof(R1SortSeg));
        if (!stopo.pos_seg.empty())
            memcpy(&stab[soff[3]], stopo.pos_seg.data(), stopo.pos_seg.size() * 4);
    }
    std::vector<double> radii(2 * (size_t)(na ? na : 1), 0.0);
    for (uint32_t a = 0; a < na; ++a)
        radii[2 * (size_t)a + 0] = sw.rbound[a], radii[2 * (size_t)a + 1] = r1_test_radius(sw.rbound[a], sw.exact[4 * (size_t)a + 3]);
    const size_t n_box = bvh.nodes.size() / 16 + topo.leaf_ref.size();

    // Uploads go through the context's OWN stream (then one wait): librays1 never touches the null stream.  A process
    // that keeps K frames in flight on K contexts with GPU_MAX_HW_QUEUES = K would otherwise hand one of its K hardware
    // queues to the null stream, and two frames would share a queue and run one after the other (measured: 20 frames
    // land in 20.1 ms instead of 17.0, tools/submit_times.py, profiles/r03/stream_queue_mapping.txt).
    const struct
    {
        DevBuf &buf;
        const void *data;
        size_t bytes;
    } uploads[] = {
        {c->sweep, sw.sweep.data(), sw.sweep.size() * 4},
        {c->exact, sw.exact.data(), sw.exact.size() * 4},
        {c->shade, sw.shade.data(), sw.shade.size() * 4},
        {c->mat, sw.mat.data(), sw.mat.size() * 4},
        {c->members, sw.members.data(), sw.members.size() * 4},
        {c->exact_g, sw.exact_g.data(), sw.exact_g.size() * 4},
        {c->bvh_nodes, bvh.nodes.data(), bvh.nodes.size() * 4},
        {c->bvh_prims, bvh.prims.data(), bvh.prims.size() * 4},
        {c->bvh_ids, bvh.ids.data(), bvh.ids.size() * 4},
        {c->active_dev, c->active_to_scene.data(), (size_t)na * 4}, // ray queries report SCENE indices: the active spheres' scene indices
        {c->refit_tab, rtab.data(), rtab.size() * 4},
        {c->refit_radii, radii.data(), radii.size() * 8},
        {c->sort_tab, stab.data(), stab.size() * 4},
    };
    int rc;
    for (const auto &u : uploads)
        if ((rc = ensure(u.buf, u.bytes)))
            return rc;
    if ((rc = ensure(c->refit_box, 256 + n_box * sizeof(R1Box))))
        return rc;
    R1_HIP(hipStreamSynchronize(c->stream));
    for (const auto &u : uploads)
        if (u.bytes)
            R1_HIP(hipMemcpyAsync(u.buf.p, u.data, u.bytes, hipMemcpyHostToDevice, c->stream));
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
        // the re-sort's tables; its scratch is laid out at the first r1_resort_spheres of the scene (sort.list[0] == null until then)
        R1SortArgs &q = c->sort;
        const uint32_t *st = (const uint32_t *)c->sort_tab.p;
        memset(&q, 0, sizeof(q));
        q.exact = r.exact, q.prims = r.prims, q.ids = (uint32_t *)c->bvh_ids.p, q.slot = (uint32_t *)c->refit_tab.p + roff[1];
        q.mov = st + soff[0], q.mslot = st + soff[1], q.seg = (const R1SortSeg *)(st + soff[2]), q.pos_seg = st + soff[3];
        q.m = (uint32_t)stopo.mov.size();
        c->sort_depth_off = stopo.depth_off;
        c->n_bvh_ids = n_ids;
    }
    c->moved = false, c->src_stale = false;
    c->n_bvh_nodes = (uint32_t)(bvh.nodes.size() / 16);
    c->n_bvh_leaves = bvh.n_leaves;
    c->bvh_depth = bvh.max_depth;
    c->bvh_leaf_pairs = leaf_pairs;
    for (int k = 0; k < 3; ++k)
        c->bvh_centre[k] = bvh.centre[k];
    c->bvh_pad_local = bvh.pad_local;
    c->bvh_root_leaf = bvh.root_leaf;
    // (the kernels' flat walk is written for y, the up axis of the reference's scenes; a tree flat along x or z walks the generic loop)
    c->bvh_flat_m = bvh.flat_axis == 1 ? bvh.flat_m : 0.0f, c->bvh_flat_e = bvh.flat_axis == 1 ? bvh.flat_e : -1.0f;
    for (int &o : c->occupancy)
        o = 0; // the tree kernels' LDS footprint follows the tree (depth of the traversal stack, size of the node table)
    memset(c->query_occupancy, 0, sizeof(c->query_occupancy));
    c->n_groups = sw.n_groups;
    c->n_multi = sw.n_multi;

    c->n_active = na;
    c->n_sweep = sw.n_sweep;
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

// The page-locked staging buffer of the host forms, at least `floats` floats of it, free to be written: the kernels of the previous update may
// still be reading it, so their event is waited for first.
static int stage_reserve(r1_context *c, size_t floats)
{
    if (c->stage_busy)
        R1_HIP(hipEventSynchronize(c->stage_ev));
    c->stage_busy = false;
    if (!c->stage_ev)
        R1_HIP(hipEventCreateWithFlags(&c->stage_ev, hipEventDisableTiming));
    if (c->stage_cap < floats)
    {
        if (c->stage)
            R1_HIP(hipHostFree(c->stage));
        c->stage = c->stage_dev = nullptr, c->stage_cap = 0;
        R1_HIP(hipHostMalloc((void **)&c->stage, floats * 4, hipHostMallocMapped));
        R1_HIP(hipHostGetDevicePointer((void **)&c->stage_dev, c->stage, 0));
        c->stage_cap = floats;
    }
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
    if ((rc = stage_reserve(c, 3 * (size_t)count)))
        return rc;
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

// ---- sphere updates: radii and materials besides the centres (include/rays1.h "sphere updates", r1_refit.hip) -----------

// which groups of *u are given (bit 0 centres, R1_SET_RADII << 1, R1_SET_MATERIALS << 1), or -1: a group given in part, or none at all
static int update_groups(const char *who, const r1_sphere_update *u)
{
    const int nc = !!u->center_x + !!u->center_y + !!u->center_z, nr = !!u->radius_sq + !!u->inv_radius;
    const int nm = !!u->mat_type + !!u->albedo_r + !!u->albedo_g + !!u->albedo_b + !!u->mat_param;
    if ((nc && nc != 3) || (nr && nr != 2) || (nm && nm != 5))
    {
        r1_set_error("%s: the %s group is given in part (all of a group's pointers, or none)", who, nc && nc != 3 ? "centres" : (nr && nr != 2 ? "radii" : "materials"));
        return -1;
    }
    if (!nc && !nr && !nm)
    {
        r1_set_error("%s: every group of the update is NULL with count > 0", who);
        return -1;
    }
    return (nc ? 1 : 0) | (nr ? (int)(R1_SET_RADII << 1) : 0) | (nm ? (int)(R1_SET_MATERIALS << 1) : 0);
}

// update_check's rules in its order, then count == 0 (R1_OK, *groups stays 0), then the rules of *u
static int spheres_check(const char *who, r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *u, int *groups)
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
    if (count == 0)
        return R1_OK;
    if (!u)
    {
        r1_set_error("%s: u is NULL", who);
        return R1_EINVAL;
    }
    return (*groups = update_groups(who, u)) < 0 ? R1_EINVAL : R1_OK;
}

// The launches on `st`, every array of *d from memory the device can read: the move (the centres' own kernel), the set kernel, `read_ev` (or
// null) straight behind the last reader of the caller's arrays, then ONE refit if a centre or a radius changed; then what the update changes in
// the context.  A change of radius leaves the context in the state of a centre update; materials alone change no index and refuse nothing.
static int spheres_enqueue(r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *d, int groups, hipStream_t st, hipEvent_t read_ev)
{
    if (groups & 1)
        R1_HIP(r1_launch_refit_move(&c->refit, first, count, d->center_x, d->center_y, d->center_z, st));
    if (groups >> 1)
    {
        R1SetArgs s;
        s.shade = (float *)c->shade.p, s.mat = (float *)c->mat.p, s.radii = (double *)c->refit_radii.p;
        s.radius_sq = d->radius_sq, s.inv_radius = d->inv_radius, s.mat_type = d->mat_type;
        s.albedo_r = d->albedo_r, s.albedo_g = d->albedo_g, s.albedo_b = d->albedo_b, s.mat_param = d->mat_param;
        R1_HIP(r1_launch_refit_set(&c->refit, &s, first, count, (uint32_t)groups >> 1, st));
    }
    if (read_ev)
        R1_HIP(hipEventRecord(read_ev, st));
    c->pass_valid = false; // (a progressive frame does not continue across a change of the scene)
    if (!(groups & (1 | (int)(R1_SET_RADII << 1))))
        return R1_OK;
    if (c->n_active) // (a tree of 0 spheres has nothing to refit)
        R1_HIP(r1_launch_refit(&c->refit, c->refit_height_off.data(), (uint32_t)c->refit_height_off.size() - 1u, st));
    c->moved = true;
    c->grid_valid = false;
    c->bvh_flat_m = 0.0f, c->bvh_flat_e = -1.0f; // the flat y slab is dropped, as update_enqueue drops it
    return R1_OK;
}

extern "C" int r1_update_spheres(r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *u, void *hip_stream)
{
    int groups = 0, rc = spheres_check("r1_update_spheres", c, first, count, u, &groups);
    if (rc || count == 0)
        return rc;
    const bool centres = groups & 1, radii = groups & (int)(R1_SET_RADII << 1), mats = groups & (int)(R1_SET_MATERIALS << 1);
    for (uint32_t i = 0; i < count; ++i)
    {
        if (c->scene_to_active[first + i] == 0xFFFFFFFFu)
            continue;
        if (centres && !(std::isfinite(u->center_x[i]) && std::isfinite(u->center_y[i]) && std::isfinite(u->center_z[i])))
        {
            r1_set_error("r1_update_spheres: the new centre of sphere %u is not finite", first + i);
            return R1_EINVAL;
        }
        if (radii && !r1f_hittable_radius(u->radius_sq[i], u->inv_radius[i]))
        {
            r1_set_error("r1_update_spheres: the new radius of sphere %u (radius_sq %g, inv_radius %g) would make it inactive; the active set does not change",
                         first + i, (double)u->radius_sq[i], (double)u->inv_radius[i]);
            return R1_EINVAL;
        }
        if (mats && u->mat_type[i] > R1_MAT_DIELECTRIC)
        {
            r1_set_error("r1_update_spheres: sphere %u is hittable but mat_type %u is no material", first + i, (unsigned)u->mat_type[i]);
            return R1_EINVAL;
        }
    }
    R1_HIP(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // the staging buffer (the centres' own, grown): up to 9 floats and 1 byte per sphere; the previous update's kernels may still be reading it
    const size_t n_f32 = (centres ? 3 : 0) + (radii ? 2 : 0) + (mats ? 4 : 0);
    if ((rc = stage_reserve(c, n_f32 * count + (mats ? ((size_t)count + 3) / 4 : 0))))
        return rc;
    // the given arrays one after the other, the material types behind the last of them
    const float *const src[9] = {u->center_x, u->center_y, u->center_z, u->radius_sq, u->inv_radius, u->albedo_r, u->albedo_g, u->albedo_b, u->mat_param};
    const float *dev[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t at = 0;
    for (int k = 0; k < 9; ++k)
        if (src[k])
            memcpy(c->stage + at, src[k], (size_t)count * 4), dev[k] = c->stage_dev + at, at += count;
    r1_sphere_update d;
    d.center_x = dev[0], d.center_y = dev[1], d.center_z = dev[2], d.radius_sq = dev[3], d.inv_radius = dev[4];
    d.albedo_r = dev[5], d.albedo_g = dev[6], d.albedo_b = dev[7], d.mat_param = dev[8], d.mat_type = nullptr;
    if (mats)
        memcpy(c->stage + at, u->mat_type, count), d.mat_type = (const uint8_t *)(c->stage_dev + at);
    c->stage_busy = true; // (from here on: a launch that failed half-way may still have enqueued a reader)
    if ((rc = spheres_enqueue(c, first, count, &d, groups, st, c->stage_ev)))
        return rc;
    // the context's host copies follow (entries of spheres that are not active too: they are what r1_set_scene would be given)
    for (int k = 0; k < 9; ++k)
        if (src[k])
            memcpy(c->src_f32[k].data() + first, src[k], (size_t)count * 4);
    if (mats)
        memcpy(c->src_mat.data() + first, u->mat_type, count);
    return R1_OK;
}

extern "C" int r1_update_spheres_device(r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *u, void *hip_stream)
{
    int groups = 0, rc = spheres_check("r1_update_spheres_device", c, first, count, u, &groups);
    if (rc || count == 0)
        return rc;
    if (((uintptr_t)u->center_x | (uintptr_t)u->center_y | (uintptr_t)u->center_z | (uintptr_t)u->radius_sq | (uintptr_t)u->inv_radius | (uintptr_t)u->albedo_r |
         (uintptr_t)u->albedo_g | (uintptr_t)u->albedo_b | (uintptr_t)u->mat_param) & 3u)
    {
        r1_set_error("r1_update_spheres_device: every float array must be 4-byte aligned");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    if ((rc = spheres_enqueue(c, first, count, u, groups, hip_stream ? (hipStream_t)hip_stream : c->stream, nullptr)))
        return rc;
    c->src_stale = true; // the host cannot see the values: r1_set_scene rebuilds whatever it is given
    return R1_OK;
}

// ---- re-sort: the spheres re-dealt into the tree's leaves (include/rays1.h "re-sort", r1_resort.hip) ----------------------

// the scratch of the scene's re-sorts, laid out once per scene in an allocation that only grows
static int resort_scratch(r1_context *c)
{
    R1SortArgs &q = c->sort;
    if (q.list[0])
        return R1_OK;
    const size_t m = q.m, na = c->n_active ? c->n_active : 1, n_seg = c->sort_depth_off.back();
    const size_t hist = 3 * 256 * ((m + 255) / 256);
    const size_t sums = std::max(r1_sort_sums_words(3 * m), r1_sort_sums_words(hist));
    const size_t words = 5 * 3 * m + na + (n_seg ? n_seg : 1) + hist + (sums ? sums : 1);
    int rc = ensure(c->sort_ws, words * 4);
    if (rc)
        return rc;
    uint32_t *w = (uint32_t *)c->sort_ws.p;
    q.list[1] = w + 3 * m, q.key[0] = w + 6 * m, q.key[1] = w + 9 * m, q.scan = w + 12 * m;
    q.flag = w + 15 * m, q.seg_axis = q.flag + na, q.hist = q.seg_axis + (n_seg ? n_seg : 1), q.sums = q.hist + hist;
    q.list[0] = w;
    return R1_OK;
}

extern "C" int r1_resort_spheres(r1_context *c, void *hip_stream)
{
    if (!c)
    {
        r1_set_error("r1_resort_spheres: ctx is NULL");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("r1_resort_spheres: no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    if (c->sort.m == 0) // nothing is movable: nothing changes, the context's state included
        return R1_OK;
    R1_HIP(hipSetDevice(c->device));
    int rc = resort_scratch(c);
    if (rc)
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    R1_HIP(r1_launch_resort(&c->sort, c->sort_depth_off.data(), (uint32_t)c->sort_depth_off.size() - 1u, st));
    R1_HIP(r1_launch_refit(&c->refit, c->refit_height_off.data(), (uint32_t)c->refit_height_off.size() - 1u, st));
    // the context's state: that of an update (update_enqueue)
    c->moved = true;
    c->grid_valid = false;
    c->pass_valid = false;
    c->bvh_flat_m = 0.0f, c->bvh_flat_e = -1.0f;
    return R1_OK;
}

extern "C" int r1_bvh_ids_download(r1_context *c, uint32_t *ids_out, size_t ids_cap, size_t *n)
{
    if (!c || !n)
    {
        r1_set_error("r1_bvh_ids_download: %s is NULL", !c ? "ctx" : "n");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("r1_bvh_ids_download: no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    *n = c->n_bvh_ids;
    if (!ids_out)
        return R1_OK;
    if (ids_cap < c->n_bvh_ids)
        return R1_ELIMIT;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipMemcpyAsync(ids_out, c->bvh_ids.p, 4 * (size_t)c->n_bvh_ids, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->n_bvh_ids; ++i) // active index -> index into the caller's scene arrays, as r1_bvh_describe gives them
        ids_out[i] = ids_out[i] < c->n_active ? c->active_to_scene[ids_out[i]] : 0xFFFFFFFFu;
    return R1_OK;
}

extern "C" int r1_tables_download(r1_context *c, float *exact, float *shade, uint32_t *mat, double *radii, size_t cap_active, size_t *n_active)
{
    if (!c || !n_active)
    {
        r1_set_error("r1_tables_download: %s is NULL", !c ? "ctx" : "n_active");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("r1_tables_download: no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    const size_t na = *n_active = c->n_active;
    if (!exact && !shade && !mat && !radii)
        return R1_OK;
    if (cap_active < na)
        return R1_ELIMIT;
    R1_HIP(hipSetDevice(c->device));
    const struct
    {
        void *dst;
        const void *src;
        size_t bytes;
    } parts[4] = {{exact, c->exact.p, 16 * na}, {shade, c->shade.p, 16 * na}, {mat, c->mat.p, 16 * na}, {radii, c->refit_radii.p, 16 * na}};
    for (const auto &q : parts)
        if (q.dst && q.bytes)
            R1_HIP(hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
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

// R1_VARIANT_GRID: builds the uniform grid of the context's scene (from the arrays r1_set_scene received, so that r1_grid_describe and
// r1_grid_visit see the same grid) and uploads it, once per scene.  Contexts that never ask for the grid pay nothing for it.
int ensure_grid(r1_context *c)
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
    r1_grid_plan(g, c->grid_plan); // what a later r1_regrid keeps
    c->grid_planned = true, c->regrid_ready = false;
    return R1_OK;
}

// ---- regrid: the moved spheres re-registered in the uniform grid (include/rays1.h "regrid", r1_regrid.hip) ------------------

// A scene's first regrid: the tables grown to the capacity (both forms; the small one only if it holds the capacity), the outlier list to
// one entry per sphere, the scratch laid out, both R1GridArgs uploaded again with the new addresses — once per scene, kept from then on.
static int regrid_layout(r1_context *c)
{
    if (c->regrid_ready)
        return R1_OK;
    const R1GridPlan &P = c->grid_plan;
    const uint32_t na = c->n_active, cap = r1gf_capacity(P.regs);
    const size_t words = (size_t)P.n_start + cap, halves16 = (words + 7) & ~(size_t)7; // (whole 16-byte rows: the kernel copies float4)
    const bool small = na <= R1_MAX_ACTIVE_10BIT && words <= R1_GRID_LDS_HALVES && cap <= 65535u;
    const size_t nb = r1_regrid_blocks((size_t)na + 1), nbc = r1_regrid_blocks(cap), hist = 256 * nbc;
    const size_t sums = std::max(r1_sort_sums_words((size_t)na + 1), r1_sort_sums_words(hist));
    const size_t part_bytes = nb * R1GF_EXTENT_WORDS * sizeof(double);
    const size_t ws_words = 2 * ((size_t)na + 1) + 4 * (size_t)cap + hist + (sums ? sums : 1) + R1GF_STAT_WORDS;
    int rc;
    R1_HIP(hipDeviceSynchronize()); // (launches through the grid may still read the buffers that are about to be replaced)
    if ((rc = ensure(c->grid_tab32, words * 4)) || (rc = ensure(c->grid_tab, small ? halves16 * 2 : 256)) || (rc = ensure(c->grid_out, (size_t)na * 4)) ||
        (rc = ensure(c->regrid_ws, part_bytes + ws_words * 4)))
        return rc;
    R1GridArgs &G = c->grid_args;
    memset(&G, 0, sizeof(G));
    for (int a = 0; a < 3; ++a)
        G.geom.lo[a] = P.lo[a], G.geom.cell[a] = P.cell[a], G.geom.inv_cell[a] = P.inv_cell[a], G.geom.n[a] = P.n[a];
    G.geom.v2 = -1.0f; // (until the first regrid's kernels have run: every ray the tree)
    G.outliers = (const uint32_t *)c->grid_out.p;
    G.n_out = 0;
    G.n_start = P.n_start;
    G.tab = (const uint32_t *)(small ? c->grid_tab.p : c->grid_tab32.p);
    G.lds_bytes = small ? (uint32_t)(halves16 * 2) : 0u;
    R1GridArgs G32 = G;
    G32.tab = (const uint32_t *)c->grid_tab32.p, G32.lds_bytes = 0;
    R1_HIP(hipMemcpyAsync(c->grid_dev.p, small ? &G : &G32, sizeof(G), hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->grid_dev32.p, &G32, sizeof(G), hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemsetAsync(c->grid_tab32.p, 0, words * 4, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    c->grid_small = small;
    for (int &o : c->occupancy)
        o = 0; // the small grid kernels' LDS footprint follows lds_bytes
    memset(c->query_occupancy, 0, sizeof(c->query_occupancy));

    R1RegridArgs &r = c->regrid;
    memset(&r, 0, sizeof(r));
    r.plan = P;
    r.exact = (const float *)c->exact.p, r.radii = (const double *)c->refit_radii.p;
    r.na = na, r.cap = cap, r.small = small ? 1u : 0u, r.tab16_halves = small ? (uint32_t)halves16 : 0u;
    r.g16 = (R1GridArgs *)c->grid_dev.p, r.g32 = (R1GridArgs *)c->grid_dev32.p;
    r.tab32 = (uint32_t *)c->grid_tab32.p, r.tab16 = small ? (uint16_t *)c->grid_tab.p : nullptr, r.outliers = (uint32_t *)c->grid_out.p;
    r.part = (double *)c->regrid_ws.p;
    uint32_t *w = (uint32_t *)((char *)c->regrid_ws.p + part_bytes);
    r.span = w, r.oflag = w + na + 1, w += 2 * ((size_t)na + 1);
    r.key[0] = w, r.key[1] = w + cap, r.val[0] = w + 2 * (size_t)cap, r.val[1] = w + 3 * (size_t)cap, w += 4 * (size_t)cap;
    r.hist = w, r.sums = w + hist, r.stat = r.sums + (sums ? sums : 1);
    c->regrid_ready = true;
    return R1_OK;
}

extern "C" int r1_regrid(r1_context *c, void *hip_stream)
{
    if (!c)
    {
        r1_set_error("r1_regrid: ctx is NULL");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("r1_regrid: no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    int rc;
    R1_HIP(hipSetDevice(c->device));
    if (!c->grid_planned)
    {
        if (c->moved)
        {
            // (host-form updates overwrite the context's copies of the arrays: the plan can only come from those r1_set_scene received)
            r1_set_error("r1_regrid: the scene has moved and its grid was never built; call r1_regrid once, or render once through the grid, "
                         "before the first update");
            return R1_EINVAL;
        }
        if ((rc = ensure_grid(c)))
            return rc;
    }
    if (c->n_active == 0) // nothing to register: the build's empty tables serve every position of no spheres
    {
        c->grid_valid = true;
        return R1_OK;
    }
    c->grid_valid = false; // (a launch that failed half-way leaves no grid)
    if ((rc = regrid_layout(c)))
        return rc;
    R1_HIP(r1_launch_regrid(&c->regrid, hip_stream ? (hipStream_t)hip_stream : c->stream));
    c->grid_valid = true;
    return R1_OK;
}

extern "C" int r1_grid_download(r1_context *c, r1_grid_info *info, uint32_t *start_out, size_t start_cap, uint32_t *ids_out, size_t ids_cap,
                                uint32_t *outliers_out, size_t outliers_cap)
{
    if (!c || !info)
    {
        r1_set_error("r1_grid_download: %s is NULL", !c ? "ctx" : "info");
        return R1_EINVAL;
    }
    if (!c->have_scene || !c->grid_valid)
    {
        r1_set_error("r1_grid_download: %s", !c->have_scene ? "no scene set (call r1_set_scene first)"
                                                            : "the context holds no current grid (render through it once, or call r1_regrid)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipDeviceSynchronize());
    R1GridArgs G;
    R1_HIP(hipMemcpy(&G, c->grid_dev32.p, sizeof(G), hipMemcpyDeviceToHost));
    R1Grid g;
    g.geom = G.geom;
    g.start.assign(G.n_start, 0u);
    R1_HIP(hipMemcpy(g.start.data(), G.tab, (size_t)G.n_start * 4, hipMemcpyDeviceToHost));
    if (g.start.back() > (uint64_t)R1_GRID_SPAN_MAX * c->n_active)
    {
        r1_set_error("r1_grid_download: the device's cell table ends at %u registrations for %u spheres", g.start.back(), c->n_active);
        return R1_EHIP;
    }
    g.ids.assign(g.start.back(), 0u);
    if (!g.ids.empty())
        R1_HIP(hipMemcpy(g.ids.data(), G.tab + G.n_start, g.ids.size() * 4, hipMemcpyDeviceToHost));
    g.outliers.assign(G.n_out, 0u);
    if (G.n_out)
        R1_HIP(hipMemcpy(g.outliers.data(), G.outliers, (size_t)G.n_out * 4, hipMemcpyDeviceToHost));
    const uint32_t na = c->n_active;
    for (uint32_t id : g.ids)
        if (id >= na)
        {
            r1_set_error("r1_grid_download: the device's id table names sphere %u of %u", id, na);
            return R1_EHIP;
        }
    for (uint32_t id : g.outliers)
        if (id >= na)
        {
            r1_set_error("r1_grid_download: the device's outlier list names sphere %u of %u", id, na);
            return R1_EHIP;
        }
    for (size_t q = 1; q < g.start.size(); ++q)
        g.max_occupancy = std::max(g.max_occupancy, g.start[q] - g.start[q - 1]);
    // pad and V as r1_grid_describe reports them: from the rows the device holds
    g.v_safe = c->grid_plan.V;
    if (!g.ids.empty())
    {
        std::vector<float> ex(4 * (size_t)na);
        std::vector<double> radii(2 * (size_t)na);
        R1_HIP(hipMemcpy(ex.data(), c->exact.p, ex.size() * 4, hipMemcpyDeviceToHost));
        R1_HIP(hipMemcpy(radii.data(), c->refit_radii.p, radii.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t id : g.ids)
            g.pad = std::max(g.pad, r1gf_rho(ex[4 * (size_t)id], ex[4 * (size_t)id + 1], ex[4 * (size_t)id + 2], radii[2 * (size_t)id + 1], c->grid_plan.V, c->grid_plan.delta) -
                                        radii[2 * (size_t)id]);
    }
    return r1_grid_report(g, c->active_to_scene, G.geom.v2 < 0.0f, info, start_out, start_cap, ids_out, ids_cap, outliers_out, outliers_cap);
}
