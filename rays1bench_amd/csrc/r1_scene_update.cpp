// r1_scene_update.cpp — the scene edited in place on the device: moving spheres (r1_update_centers*), sphere updates
// (r1_update_spheres*, §4.27; the centres' forms are its front ends), the staging of the host forms, and the re-sort (r1_resort_spheres, §4.29).
// The kernels are r1_refit.hip's and r1_resort.hip's.

#include <string.h>

#include <algorithm>
#include <cmath>

#include "r1_context.h"
#include "r1_device_sort.h"

// What every change of a centre, a radius or a slot leaves in the context (after its launches).
static void scene_changed(r1_context *c)
{
    c->moved = true;
    c->grid_valid = false;
    c->pass_valid = false; // (a progressive frame does not continue across a change of the scene)
    // the flat y slab (r1_bvh.cpp) is dropped, not refitted: it travels by value in the launches' arguments, and spheres that leave the
    // plane are exactly the case it must not miss.  The kernels take the generic loop they already have.
    c->bvh_flat_m = 0.0f, c->bvh_flat_e = -1.0f;
}

// the first rules of every update: a context with a scene, and spheres [first, first + count) of it
static int spheres_in_range(const char *who, r1_context *c, uint32_t first, uint32_t count)
{
    int rc = need_scene(who, c);
    if (rc)
        return rc;
    if ((uint64_t)first + count > c->n_padded_scene)
    {
        r1_set_error("%s: spheres [%u, %llu) are beyond the scene's %u", who, first, (unsigned long long)first + count, c->n_padded_scene);
        return R1_EINVAL;
    }
    return R1_OK;
}

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

// the range, then count == 0 (R1_OK, *groups stays 0), then the rules of *u
static int spheres_check(const char *who, r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *u, int *groups)
{
    int rc = spheres_in_range(who, c, first, count);
    if (rc || count == 0)
        return rc;
    if (!u)
    {
        r1_set_error("%s: u is NULL", who);
        return R1_EINVAL;
    }
    return (*groups = update_groups(who, u)) < 0 ? R1_EINVAL : R1_OK;
}

// the range, then the three arrays of the centres' forms; *u: the update of the centres alone
static int centres_check(const char *who, r1_context *c, uint32_t first, uint32_t count, const void *x, const void *y, const void *z, r1_sphere_update *u)
{
    int rc = spheres_in_range(who, c, first, count);
    if (rc)
        return rc;
    if (count && (!x || !y || !z))
    {
        r1_set_error("%s: x, y and z must not be NULL with count > 0", who);
        return R1_EINVAL;
    }
    memset(u, 0, sizeof(*u));
    u->center_x = (const float *)x, u->center_y = (const float *)y, u->center_z = (const float *)z;
    return R1_OK;
}

// The launches on `st`, every array of *d from memory the device can read: the move (the centres' own kernel), the set kernel, `read_ev` (or
// null) straight behind the last reader of the caller's arrays, then ONE refit if a centre or a radius changed; then what the update changes in
// the context.  A change of radius leaves the context in the state of a centre update; materials alone change no index and refuse nothing.
// Nothing is waited for; the launch info and the timing events are left alone.
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
        // (the set kernel writes the rows of active spheres alone — active indices stop at R1_MAX_ACTIVE_10BIT - 1 in a small scene — so row
        //  R1_MAX_ACTIVE_10BIT of the small-scene shade table, the identity row the attenuation words' pads point at (r1_sweep.cpp), stays)
        R1_HIP(r1_launch_refit_set(&c->refit, &s, first, count, (uint32_t)groups >> 1, st));
    }
    if (read_ev)
        R1_HIP(hipEventRecord(read_ev, st));
    c->pass_valid = false; // (a progressive frame does not continue across a change of the scene)
    if (!(groups & (1 | (int)(R1_SET_RADII << 1))))
        return R1_OK;
    if (c->n_active) // (a tree of 0 spheres has nothing to refit)
        R1_HIP(r1_launch_refit(&c->refit, c->refit_height_off.data(), (uint32_t)c->refit_height_off.size() - 1u, st));
    scene_changed(c);
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

// The host forms behind their checks of the arguments (count > 0, `groups` of *u given): the values of the active spheres checked, the
// arrays staged, the launches, the context's host copies.
static int update_from_host(const char *who, r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *u, int groups, void *hip_stream)
{
    const bool centres = groups & 1, radii = groups & (int)(R1_SET_RADII << 1), mats = groups & (int)(R1_SET_MATERIALS << 1);
    for (uint32_t i = 0; i < count; ++i)
    {
        if (c->scene_to_active[first + i] == 0xFFFFFFFFu)
            continue;
        if (centres && !(std::isfinite(u->center_x[i]) && std::isfinite(u->center_y[i]) && std::isfinite(u->center_z[i])))
        {
            r1_set_error("%s: the new centre of sphere %u is not finite", who, first + i);
            return R1_EINVAL;
        }
        if (radii && !r1f_hittable_radius(u->radius_sq[i], u->inv_radius[i]))
        {
            r1_set_error("%s: the new radius of sphere %u (radius_sq %g, inv_radius %g) would make it inactive; the active set does not change", who,
                         first + i, (double)u->radius_sq[i], (double)u->inv_radius[i]);
            return R1_EINVAL;
        }
        if (mats && u->mat_type[i] > R1_MAT_DIELECTRIC)
        {
            r1_set_error("%s: sphere %u is hittable but mat_type %u is no material", who, first + i, (unsigned)u->mat_type[i]);
            return R1_EINVAL;
        }
    }
    R1_HIP(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // the staging buffer: up to 9 floats and 1 byte per sphere (3 floats for centres alone); the previous update's kernels may still be reading it
    const size_t n_f32 = (centres ? 3 : 0) + (radii ? 2 : 0) + (mats ? 4 : 0);
    int rc = stage_reserve(c, n_f32 * count + (mats ? ((size_t)count + 3) / 4 : 0));
    if (rc)
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

// the device forms behind their checks: the launches alone
static int update_from_device(r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *u, int groups, void *hip_stream)
{
    R1_HIP(hipSetDevice(c->device));
    return spheres_enqueue(c, first, count, u, groups, hip_stream ? (hipStream_t)hip_stream : c->stream, nullptr);
}

extern "C" int r1_update_centers(r1_context *c, uint32_t first, uint32_t count, const float *x, const float *y, const float *z, void *hip_stream)
{
    r1_sphere_update u;
    int rc = centres_check("r1_update_centers", c, first, count, x, y, z, &u);
    if (rc || count == 0)
        return rc;
    return update_from_host("r1_update_centers", c, first, count, &u, 1, hip_stream);
}

extern "C" int r1_update_centers_device(r1_context *c, uint32_t first, uint32_t count, const void *d_x, const void *d_y, const void *d_z, void *hip_stream)
{
    r1_sphere_update u;
    int rc = centres_check("r1_update_centers_device", c, first, count, d_x, d_y, d_z, &u);
    if (rc || count == 0)
        return rc;
    if (((uintptr_t)d_x | (uintptr_t)d_y | (uintptr_t)d_z) & 3u)
    {
        r1_set_error("r1_update_centers_device: d_x, d_y and d_z must be 4-byte aligned");
        return R1_EINVAL;
    }
    return update_from_device(c, first, count, &u, 1, hip_stream); // (the host copies of the centres stay: `moved` keeps r1_set_scene from trusting them)
}

extern "C" int r1_update_spheres(r1_context *c, uint32_t first, uint32_t count, const r1_sphere_update *u, void *hip_stream)
{
    int groups = 0, rc = spheres_check("r1_update_spheres", c, first, count, u, &groups);
    if (rc || count == 0)
        return rc;
    return update_from_host("r1_update_spheres", c, first, count, u, groups, hip_stream);
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
    if ((rc = update_from_device(c, first, count, u, groups, hip_stream)))
        return rc;
    c->src_stale = true; // the host cannot see the values: r1_set_scene rebuilds whatever it is given
    return R1_OK;
}

// ---- re-sort: the spheres re-dealt into the tree's leaves (include/rays1.h "re-sort") -----------------------------------------------------------

// the scratch of the scene's re-sorts, laid out once per scene in an allocation that only grows
static int resort_scratch(r1_context *c)
{
    R1SortArgs &q = c->sort;
    if (q.list[0])
        return R1_OK;
    const size_t m = q.m, na = c->n_active ? c->n_active : 1, n_seg = c->sort_depth_off.back();
    const size_t hist = r1_radix_hist_words(m, 3);
    const size_t sums = std::max(r1_scan_sums_words(3 * m), r1_scan_sums_words(hist));
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
    int rc = need_scene("r1_resort_spheres", c);
    if (rc)
        return rc;
    if (c->sort.m == 0) // nothing is movable: nothing changes, the context's state included
        return R1_OK;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = resort_scratch(c)))
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    R1_HIP(r1_launch_resort(&c->sort, c->sort_depth_off.data(), (uint32_t)c->sort_depth_off.size() - 1u, st));
    R1_HIP(r1_launch_refit(&c->refit, c->refit_height_off.data(), (uint32_t)c->refit_height_off.size() - 1u, st));
    scene_changed(c);
    return R1_OK;
}
