// r1_scene.cpp — what a context knows of its scene: r1_set_scene (active spheres, the sweep's tables, the box tree, the refit's and the
// re-sort's tables; uploads through the context's own stream), the camera alone, and the downloads of the tree and the tables.  The scene
// edited in place is r1_scene_update.cpp, its uniform grid r1_scene_grid.cpp.

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

// The refusals every entry point that needs a scene begins with: no context, (where the call has one) no `arg` for its result or its input,
// no scene.
int need_scene(const char *who, const r1_context *c, const char *arg_name, const void *arg)
{
    if (!c || (arg_name && !arg))
    {
        r1_set_error("%s: %s is NULL", who, !c ? "ctx" : arg_name);
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("%s: no scene set (call r1_set_scene first)", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

// the blocks-per-CU caches follow the kernels' LDS footprint: whoever changes that (a new tree, a grid of another form) empties them
void forget_occupancy(r1_context *c)
{
    for (int &o : c->occupancy)
        o = 0;
    memset(c->query_occupancy, 0, sizeof(c->query_occupancy));
}

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
    c->history_slot = -1;  // (nor does the history of accumulated frames)
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
    std::vector<uint32_t> rtab, stab;
    size_t roff[5], soff[4];
    r1_refit_pack(c->scene_to_active, topo, rtab, roff);
    r1_sort_pack(stopo, stab, soff);
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
    forget_occupancy(c); // the tree kernels' LDS footprint follows the tree (depth of the traversal stack, size of the node table)
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
    int rc = need_scene("r1_set_camera", c, "camera", cam);
    if (rc)
        return rc;
    c->pass_valid = false; // (a progressive frame does not continue across a change of view, as across r1_set_scene)
    c->cam = device_camera(*cam);
    c->src_cam = *cam;       // r1_set_scene(same arrays, this camera) is still the shortcut
    return R1_OK;
}

extern "C" int r1_bvh_ids_download(r1_context *c, uint32_t *ids_out, size_t ids_cap, size_t *n)
{
    int rc = need_scene("r1_bvh_ids_download", c, "n", n);
    if (rc)
        return rc;
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
    int rc = need_scene("r1_tables_download", c, "n_active", n_active);
    if (rc)
        return rc;
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
    int rc = need_scene("r1_bvh_download", c, "nodes", nodes);
    if (rc)
        return rc;
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
