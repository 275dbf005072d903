"""GPU tests of sphere updates: r1_update_spheres* rewrites radii and materials in the tables the kernels read — and refits
the box tree where a radius changed — on the device.  The contract is r1_update_centers': every render, ray query and path query afterwards
gives, byte for byte and ray for ray, what a FRESH context gives after r1_set_scene with the edited arrays.  Nothing here has a tolerance."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_bvh_host import F
from test_gpu_update import (CASES, MOVED_RULE, PROGRAM_SCENES, edge_arrays, edge_camera, expect_refusal, first_difference, params, program_lattice, same,
                             same_tga)
from test_refit_host import edge_scene, lattice_of, raw_from_arrays
from test_update_spheres_host import RADIUS_FAMILIES, radius_family

pytestmark = pytest.mark.gpu

MATERIAL_FAMILIES = ("identity", "permute", "dielectric_1.5", "dielectric_1.0", "metal_fuzz0", "metal_fuzz1", "albedo0", "albedo1")
MAT_KEYS = ("mat_type", "albedo_r", "albedo_g", "albedo_b", "mat_param")
# r1_last_stats slots of the tree's diagnostic build that are sums over LANES — node visits, leaf trips x lanes, root steps — and so do not depend
# on which samples shared a wave (the trip counts of the wave's loops, slots 2 and 3, do)
WALK_SLOTS = (9, 14, 15)
EVERY_VARIANT = (binding.VARIANT_DEFAULT, binding.VARIANT_REFERENCE, binding.VARIANT_PREFILTER, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID)


@pytest.fixture(scope="module")
def upd():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def fresh():
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    """name -> (Scene, arrays): built once, never changed."""
    out = {}
    for name, (w, h, spp, pad_local, big) in CASES.items():
        if name == "large":
            sc = r1.create_large_scene(w, h)
        else:
            gw, gh = (int(v) for v in name[4:].split("x"))
            sc = r1.create_grid_scene(w, h, gw, gh)
        out[name] = (sc, sc.arrays())
    return out


def edited(a, centers=None, radii=None, materials=None):
    """The scene's arrays with the given groups replaced (whole-scene arrays): what r1_set_scene is given for the comparison."""
    d = dict(a)
    for keys, group in ((("center_x", "center_y", "center_z"), centers), (("radius_sq", "inv_radius"), radii), (MAT_KEYS, materials)):
        if group is not None:
            d.update(zip(keys, group))
    return d


def build_fresh(fresh, d, cam):
    cs, keep = raw_from_arrays(d)
    fresh.set_scene_raw(cs, cam)
    return cs, keep


def material_family(a, family, seed=5):
    """(mat_type, albedo_r, albedo_g, albedo_b, mat_param), scene-indexed: a fixed function of the scene's arrays, the family and the seed.
    Entries of spheres that are not active keep their values (mat_type 255 for the reference's placeholders)."""
    m = [a[k].copy() for k in MAT_KEYS]
    act = np.nonzero(a["inv_radius"] != 0)[0]
    if family == "identity":
        return tuple(m)
    if family == "permute":
        p = act[np.random.default_rng(seed).permutation(len(act))]
        for v in m:
            v[act] = v[p]
    elif family.startswith("dielectric_"):
        m[0][act], m[4][act] = 2, F(family.split("_")[1])
    elif family.startswith("metal_fuzz"):
        m[0][act], m[4][act] = 1, F(family[-1])
    elif family.startswith("albedo"):
        for v in m[1:4]:
            v[act] = F(family[-1])
    else:
        raise ValueError(family)
    return tuple(m)


def tables_equal(got, want, what):
    assert sorted(got) == sorted(want) == ["exact", "mat", "radii", "shade"]
    for k in got:
        assert got[k].shape == want[k].shape, (what, k)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k] != want[k])
            assert False, (what, k, len(bad), "first", bad[0].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


# ---- 1: radii --------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", RADIUS_FAMILIES)
@pytest.mark.parametrize("name", list(CASES))
def test_radius_update_equals_fresh_build(upd, fresh, scenes, name, family):
    sc, a = scenes[name]
    x, y, z, rsq, inv = radius_family(a, family)
    centers = (x, y, z) if family == "with_centres" else None
    upd.set_scene(sc)
    upd.update_spheres(0, centers=centers, radii=(rsq, inv))
    build_fresh(fresh, edited(a, centers, (rsq, inv)), sc.camera.contents)
    p = params(name)
    want = fresh.render(p)[:2]
    same(upd.render(p)[:2], want, (name, family, "default"))
    assert upd.launch_info()["kernel"] == binding.VARIANT_BVH
    same(upd.render(params(name, binding.VARIANT_BVH))[:2], want, (name, family, "bvh"))
    same(upd.render(params(name, binding.VARIANT_REFERENCE))[:2], want, (name, family, "reference on the updated context"))
    if family == "all_x1.5":
        upd.set_scene(sc)
        assert upd.render(p)[0].tobytes() != want[0].tobytes(), (name, family, "the update must show")
        upd.update_spheres(0, radii=(rsq, inv))
        gs, ws = upd.render_samples(p), fresh.render_samples(p)
        assert gs[1] == ws[1] == want[1] and gs[0].tobytes() == want[0].tobytes()
        assert gs[2].tobytes() == ws[2].tobytes(), (name, family, "samples")
    got, host = upd.bvh_download(), binding.bvh_refit_describe_spheres(sc.spheres.contents, x, y, z, rsq, inv)[1]
    assert got.shape == host.shape and got.tobytes() == host.tobytes(), (name, family, first_difference(got, host))
    tables_equal(upd.tables_download(), fresh.tables_download(), (name, family))


@pytest.mark.parametrize("n_active", [0, 1, 4, 5])
def test_radius_update_on_edge_trees_with_placeholders(upd, fresh, n_active):
    cs, arrs, mt = edge_scene(n_active)
    a = edge_arrays(arrs, mt)
    w, h = 64, 48
    cam = edge_camera(w, h)
    p = r1.make_params(w, h, 3, 31)
    x, y, z, rsq, inv = radius_family(a, "with_centres")
    upd.set_scene_raw(cs, cam)
    upd.update_spheres(0, centers=(x, y, z), radii=(rsq, inv))
    build_fresh(fresh, edited(a, (x, y, z), (rsq, inv)), cam)
    want = fresh.render(p)[:2]
    same(upd.render(p)[:2], want, (n_active, "default"))
    same(upd.render(r1.make_params(w, h, 3, 31, variant=binding.VARIANT_REFERENCE))[:2], want, (n_active, "reference"))
    assert upd.bvh_download().tobytes() == binding.bvh_refit_describe_spheres(cs, x, y, z, rsq, inv)[1].tobytes()
    tables_equal(upd.tables_download(), fresh.tables_download(), n_active)


# ---- 2: materials ----------------------------------------------------------------------------------------------------------------------------


def every_variant_equals_fresh(upd, fresh, name, what):
    for variant in EVERY_VARIANT:
        same(upd.render(params(name, variant))[:2], fresh.render(params(name, variant))[:2], (what, "variant", variant))


@pytest.mark.parametrize("family", MATERIAL_FAMILIES)
@pytest.mark.parametrize("name", list(CASES))
def test_material_update_equals_fresh_build_in_every_variant(upd, fresh, scenes, name, family):
    sc, a = scenes[name]
    mats = material_family(a, family)
    upd.set_scene(sc)
    upd.render(params(name, binding.VARIANT_BVH_STATS))
    walk_before = [upd.last_stats()["raw"][k] for k in WALK_SLOTS]
    upd.update_spheres(0, materials=mats)
    build_fresh(fresh, edited(a, materials=mats), sc.camera.contents)
    every_variant_equals_fresh(upd, fresh, name, (name, family))
    if family not in ("identity",):
        fresh.set_scene(sc)
        assert fresh.render(params(name))[0].tobytes() != upd.render(params(name))[0].tobytes(), (name, family, "the update must show")
        build_fresh(fresh, edited(a, materials=mats), sc.camera.contents)
    tables_equal(upd.tables_download(), fresh.tables_download(), (name, family))
    assert upd.bvh_download().tobytes() == binding.bvh_describe(sc.spheres.contents)[1].tobytes()  # no refit: the builder's rows
    upd.render(params(name))
    info = upd.launch_info()
    fresh.render(params(name))
    assert info == fresh.launch_info() and info["kernel"] == binding.VARIANT_BVH  # the tree kernel, the same launch as on the fresh context
    # r1_launch_info has no field for the flat y slab (it travels in the launch's arguments), and pixels are the same with and without it.
    # What does tell the two walks apart is the diagnostic build's node visits (slot 9, a sum over lanes): the flat walk tests one y slab for
    # all boxes instead of each box's own, so it enters other nodes than the generic loop.  The identity family traces the same paths before
    # and after the update, so the counters can be compared: they stay after a materials update and change after an identity update of the
    # centres, which drops the slab.
    if family == "identity":
        assert binding.bvh_describe(sc.spheres.contents)[0]["flat_axis"] == (1 if name == "large" else -1)
        upd.render(params(name, binding.VARIANT_BVH_STATS))
        assert [upd.last_stats()["raw"][k] for k in WALK_SLOTS] == walk_before, "the walk's counters before the update"
        if name == "large":
            upd.update_centers(0, a["center_x"], a["center_y"], a["center_z"])
            upd.render(params(name, binding.VARIANT_BVH_STATS))
            assert upd.last_stats()["raw"][9] != walk_before[0], "node visits of the generic loop: the comparison above can see a dropped slab"


@pytest.mark.parametrize("name", list(CASES))
def test_material_update_of_a_partial_range_spanning_placeholders(upd, fresh, scenes, name):
    sc, a = scenes[name]
    n = sc.count
    first = n // 2
    assert (a["inv_radius"][first:] == 0).any() and (a["inv_radius"][first:] != 0).any() and (a["mat_type"][first:] > 2).any()
    full = material_family(a, "permute", seed=9)
    part = tuple(v[first:] for v in full)
    merged = tuple(np.concatenate([a[k][:first], v]) for k, v in zip(MAT_KEYS, part))
    upd.set_scene(sc)
    upd.update_spheres(first, materials=part)
    build_fresh(fresh, edited(a, materials=merged), sc.camera.contents)
    every_variant_equals_fresh(upd, fresh, name, (name, "partial range"))
    tables_equal(upd.tables_download(), fresh.tables_download(), (name, "partial range"))


# ---- 3: mixed and repeated -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(CASES))
def test_one_call_equals_three_calls_equals_fresh_build(upd, fresh, scenes, name):
    sc, a = scenes[name]
    x, y, z, rsq, inv = radius_family(a, "with_centres")
    mats = material_family(a, "permute")
    p = params(name)
    build_fresh(fresh, edited(a, (x, y, z), (rsq, inv), mats), sc.camera.contents)
    want, want_tables = fresh.render(p)[:2], fresh.tables_download()
    want_rows = binding.bvh_refit_describe_spheres(sc.spheres.contents, x, y, z, rsq, inv)[1]
    upd.set_scene(sc)
    upd.update_spheres(0, centers=(x, y, z), radii=(rsq, inv), materials=mats)
    same(upd.render(p)[:2], want, (name, "one call"))
    tables_equal(upd.tables_download(), want_tables, (name, "one call"))
    assert upd.bvh_download().tobytes() == want_rows.tobytes()
    upd.set_scene(sc)
    upd.update_spheres(0, materials=mats)
    upd.update_spheres(0, radii=(rsq, inv))
    upd.update_spheres(0, centers=(x, y, z))
    same(upd.render(p)[:2], want, (name, "three calls"))
    same(upd.render(params(name, binding.VARIANT_REFERENCE))[:2], want, (name, "three calls, reference"))
    tables_equal(upd.tables_download(), want_tables, (name, "three calls"))
    assert upd.bvh_download().tobytes() == want_rows.tobytes()


@pytest.mark.parametrize("name", ["large", "grid160x100"])
def test_ten_successive_updates_equal_one_and_interleave_with_update_centers(upd, fresh, scenes, name):
    """Each update starts from the previous state; boxes and rows are recomputed, never accumulated.  Odd steps move the centres through
    r1_update_centers, even steps change radii and materials through r1_update_spheres."""
    sc, a = scenes[name]
    lat = lattice_of(a)
    rng = np.random.default_rng(98)
    x, y, z = (a[k].copy() for k in ("center_x", "center_y", "center_z"))
    rsq, inv = a["radius_sq"].copy(), a["inv_radius"].copy()
    mats = material_family(a, "identity")
    upd.set_scene(sc)
    for step in range(10):
        if step % 2:
            for v in (x, y, z):
                v[lat] = (v[lat] + rng.uniform(-0.15, 0.15, len(lat))).astype(F)
            upd.update_centers(0, x, y, z)
        else:
            rad = (F(1) / inv[lat] * rng.uniform(0.8, 1.25, len(lat))).astype(F)
            rsq[lat], inv[lat] = (rad * rad).astype(F), (F(1) / rad).astype(F)
            mats = material_family(edited(a, materials=mats), "permute", seed=step)
            upd.update_spheres(0, radii=(rsq, inv), materials=mats)
    got, want = upd.bvh_download(), binding.bvh_refit_describe_spheres(sc.spheres.contents, x, y, z, rsq, inv)[1]
    assert got.tobytes() == want.tobytes(), first_difference(got, want)
    build_fresh(fresh, edited(a, (x, y, z), (rsq, inv), mats), sc.camera.contents)
    p = params(name)
    same(upd.render(p)[:2], fresh.render(p)[:2], (name, "after ten updates"))
    tables_equal(upd.tables_download(), fresh.tables_download(), (name, "after ten updates"))


# ---- 4: the device form ----------------------------------------------------------------------------------------------------------------------


def to_device(arrays):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in arrays]
    return t, tuple(v.data_ptr() for v in t)


@pytest.mark.parametrize("name", ["large", "grid160x100"])
def test_device_form_equals_host_form(upd, fresh, scenes, name):
    sc, a = scenes[name]
    p = params(name)
    n = sc.count
    x, y, z, rsq, inv = radius_family(a, "with_centres")
    mats = material_family(a, "permute")
    upd.set_scene(sc)
    upd.update_spheres(0, centers=(x, y, z), radii=(rsq, inv), materials=mats)
    host_form, host_rows, host_tables = upd.render(p)[:2], upd.bvh_download(), upd.tables_download()
    upd.set_scene(sc)
    tc, pc = to_device((x, y, z))
    tr, pr = to_device((rsq, inv))
    tm, pm = to_device(mats)
    upd.update_spheres_device(0, n, centers=pc, radii=pr, materials=pm)
    same(upd.render(p)[:2], host_form, (name, "device form"))
    assert upd.bvh_download().tobytes() == host_rows.tobytes()
    tables_equal(upd.tables_download(), host_tables, (name, "device form"))
    build_fresh(fresh, edited(a, (x, y, z), (rsq, inv), mats), sc.camera.contents)
    same(host_form, fresh.render(p)[:2], (name, "host form"))
    # a partial range, each group alone, mat_type at an odd address
    first, count = 7, n - 20
    upd.set_scene(sc)
    upd.update_spheres_device(first, count, radii=tuple(v[first:].data_ptr() for v in tr))
    upd.update_spheres_device(first, count, materials=tuple(v[first:].data_ptr() for v in tm))
    assert tm[0][first:].data_ptr() % 4 != 0
    part = edited(a)
    for k, v in zip(("radius_sq", "inv_radius") + MAT_KEYS, (rsq, inv) + tuple(mats)):
        part[k] = a[k].copy()
        part[k][first:first + count] = v[first:first + count]
    build_fresh(fresh, part, sc.camera.contents)
    same(upd.render(p)[:2], fresh.render(p)[:2], (name, "device form, partial range"))
    tables_equal(upd.tables_download(), fresh.tables_download(), (name, "device form, partial range"))


@pytest.mark.parametrize("name", ["large", "grid160x100"])
def test_device_form_entries_the_host_form_refuses(upd, fresh, scenes, name):
    """inv_radius 0: the sphere is never hittable and the pixels are r1_set_scene's, where it is dropped.  mat_type 7: the entry is skipped,
    the sphere keeps its material."""
    sc, a = scenes[name]
    p = params(name)
    n = sc.count
    lat = lattice_of(a)
    gone, kept = lat[len(lat) // 3], lat[len(lat) // 2]
    rsq, inv = a["radius_sq"].copy(), a["inv_radius"].copy()
    inv[gone] = 0
    upd.set_scene(sc)
    tr, pr = to_device((rsq, inv))
    upd.update_spheres_device(0, n, radii=pr)
    build_fresh(fresh, edited(a, radii=(rsq, inv)), sc.camera.contents)
    want = fresh.render(p)[:2]
    same(upd.render(p)[:2], want, (name, "inv_radius 0"))
    same(upd.render(params(name, binding.VARIANT_REFERENCE))[:2], want, (name, "inv_radius 0, reference"))
    got, host = upd.bvh_download(), binding.bvh_refit_describe_spheres(sc.spheres.contents, a["center_x"], a["center_y"], a["center_z"], rsq, inv)[1]
    assert got.tobytes() == host.tobytes(), first_difference(got, host)
    t = upd.tables_download()
    row = int(np.nonzero(np.nonzero(a["inv_radius"] != 0)[0] == gone)[0][0])
    assert t["exact"][row, 3] == -np.inf and t["shade"][row, 0] == 0 and (t["radii"][row] == 0).all()
    # mat_type 7 on one sphere, new materials on all the others
    mats = [v.copy() for v in material_family(a, "permute", seed=3)]
    mats[0][kept] = 7
    upd.set_scene(sc)
    tm, pm = to_device(mats)
    upd.update_spheres_device(0, n, materials=pm)
    ref = [v.copy() for v in mats]
    for v, k in zip(ref, MAT_KEYS):
        v[kept] = a[k][kept]
    build_fresh(fresh, edited(a, materials=tuple(ref)), sc.camera.contents)
    for variant in EVERY_VARIANT:
        same(upd.render(params(name, variant))[:2], fresh.render(params(name, variant))[:2], (name, "mat_type 7", variant))
    tables_equal(upd.tables_download(), fresh.tables_download(), (name, "mat_type 7"))
    # after a device-form update of materials alone r1_set_scene rebuilds, whatever it is given: the original arrays give the original scene
    upd.set_scene(sc)
    fresh.set_scene(sc)
    same(upd.render(p)[:2], fresh.render(p)[:2], (name, "r1_set_scene(original arrays) after a device-form materials update"))
    tables_equal(upd.tables_download(), fresh.tables_download(), (name, "after r1_set_scene"))


# ---- 5: queries -------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(CASES))
def test_ray_and_path_queries_after_updates(upd, fresh, scenes, name):
    sc, a = scenes[name]
    x, y, z, rsq, inv = radius_family(a, "all_x1.5")
    mats = material_family(a, "permute")
    upd.set_scene(sc)
    upd.update_spheres(0, radii=(rsq, inv))
    upd.update_spheres(0, materials=mats)
    cs, keep = build_fresh(fresh, edited(a, radii=(rsq, inv), materials=mats), sc.camera.contents)
    rng = np.random.default_rng(17)
    n = 4096
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = np.stack([rng.uniform(-12, 12, n), rng.uniform(0.5, 6, n), rng.uniform(-12, 12, n)], 1)
    act = np.nonzero(a["inv_radius"] != 0)[0]
    tgt = act[rng.integers(0, len(act), n)]
    d = np.stack([x[tgt], y[tgt], z[tgt]], 1).astype(np.float64) + rng.normal(0, 0.05, (n, 3)) - rays[:, 0:3]
    rays[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    rays[:, 3] = np.where(rng.random(n) < 0.25, rng.uniform(0.5, 8, n), np.finfo(F).max).astype(F)
    for mode in (binding.CAST_CLOSEST, binding.CAST_ANY):
        want = binding.cast_rays_host(cs, rays, mode)
        assert (want["index"] >= 0).sum() > n // 4 if mode == binding.CAST_CLOSEST else want.sum() > n // 4
        assert fresh.cast_rays(rays, mode).tobytes() == want.tobytes(), (name, mode, "fresh")
        for variant in (binding.VARIANT_DEFAULT, binding.VARIANT_REFERENCE):
            assert upd.cast_rays(rays, mode, variant).tobytes() == want.tobytes(), (name, mode, variant)
    expect_refusal(lambda: upd.cast_rays(rays, binding.CAST_CLOSEST, binding.VARIANT_GRID), MOVED_RULE)
    want = binding.trace_rays_host(cs, rays)
    assert (want["rays"] > 1).sum() > n // 4
    assert fresh.trace_rays(rays).tobytes() == want.tobytes(), (name, "trace, fresh")
    for variant in (binding.VARIANT_DEFAULT, binding.VARIANT_REFERENCE):
        assert upd.trace_rays(rays, variant=variant).tobytes() == want.tobytes(), (name, "trace", variant)
    # materials alone: the grid keeps serving queries
    upd.set_scene(sc)
    upd.update_spheres(0, materials=mats)
    cs, keep = build_fresh(fresh, edited(a, materials=mats), sc.camera.contents)
    want = binding.trace_rays_host(cs, rays)
    for variant in (binding.VARIANT_DEFAULT, binding.VARIANT_GRID, binding.VARIANT_REFERENCE):
        assert upd.trace_rays(rays, variant=variant).tobytes() == want.tobytes(), (name, "trace after materials", variant)
    assert upd.cast_rays(rays, binding.CAST_CLOSEST, binding.VARIANT_GRID).tobytes() == fresh.cast_rays(rays, binding.CAST_CLOSEST).tobytes()


# ---- 6: stream order --------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["large", "grid40x30"])
def test_stream_order_and_a_path_batch_after_an_update(upd, fresh, scenes, name):
    sc, a = scenes[name]
    w, h = CASES[name][:2]
    p = params(name)
    x, y, z, rsq, inv = radius_family(a, "all_x1.5")
    mats = material_family(a, "permute")
    fa, fb = binding.HostFrames(w, h, 1), binding.HostFrames(w, h, 1)
    cams = binding.orbit_cameras(sc, 5)[1:4]
    hp = binding.HostFrames(w, h, 3)
    try:
        upd.set_scene(sc)
        upd.render_async(p, fa)                                  # frame A: the old scene
        upd.update_spheres(0, radii=(rsq, inv), materials=mats)
        upd.render_async(p, fb)                                  # frame B: the new one
        upd.sync()                                               # one wait for all three
        fresh.set_scene(sc)
        old = fresh.render(p)[:2]
        assert fa.rays(0) == old[1] and fa.image(0).tobytes() == old[0].tobytes(), "frame A must see the old scene"
        build_fresh(fresh, edited(a, radii=(rsq, inv), materials=mats), sc.camera.contents)
        new = fresh.render(p)[:2]
        assert fb.rays(0) == new[1] and fb.image(0).tobytes() == new[0].tobytes(), "frame B must see the new scene"
        assert old[0].tobytes() != new[0].tobytes()
        upd.render_path_async(p, cams, hp, seed_stride=3)
        upd.sync()
        for f, cam in enumerate(cams):
            fresh.set_camera(cam)
            img, rays, _ = fresh.render(r1.make_params(w, h, p.spp, p.seed + 3 * f))
            assert hp.rays(f) == rays and hp.image(f).tobytes() == img.tobytes(), (name, "path frame", f)
    finally:
        fa.close(), fb.close(), hp.close()


# ---- 7: state ---------------------------------------------------------------------------------------------------------------------------------


def test_state_rules(upd, fresh, scenes):
    import torch
    sc, a = scenes["large"]
    n = sc.count
    p = params("large")
    L = binding.lib()
    x, y, z, rsq, inv = radius_family(a, "all_x1.5")
    mats = material_family(a, "permute")
    lat = lattice_of(a)
    blank = r1.Renderer(0)
    try:
        expect_refusal(lambda: blank.update_spheres(0, radii=(rsq, inv)), "no scene set")
        t = torch.zeros(8, device="cuda")
        expect_refusal(lambda: blank.update_spheres_device(0, 8, radii=(t.data_ptr(), t.data_ptr())), "no scene set")
    finally:
        blank.close()
    upd.set_scene(sc)
    fresh.set_scene(sc)
    original = upd.render(p)[:2]
    tables0, rows0 = upd.tables_download(), upd.bvh_download()
    # rule 4, each refusal: R1_EINVAL, and nothing changes
    u = binding.SphereUpdate()
    assert L.r1_update_spheres(upd._c, 3, 0, None, None) == binding.R1_OK                       # count == 0 touches nothing, whatever u
    assert L.r1_update_spheres_device(upd._c, 3, 0, C.byref(u), None) == binding.R1_OK
    for fn in (L.r1_update_spheres, L.r1_update_spheres_device):
        assert fn(upd._c, 0, n, None, None) == binding.R1_EINVAL                                # u == NULL
        assert fn(upd._c, 0, n, C.byref(u), None) == binding.R1_EINVAL                          # every group NULL
        assert b"every group" in L.r1_last_error()
    expect_refusal(lambda: upd.update_spheres(1, radii=(rsq, inv)), "beyond the scene")
    expect_refusal(lambda: upd.update_spheres(n, materials=tuple(v[:1] for v in mats)), "beyond the scene")
    dev, ptr = to_device((rsq, inv) + tuple(mats) + (x, y, z))
    for missing in range(2):                                                                    # a group given in part
        part = binding.SphereUpdate()
        setattr(part, ("radius_sq", "inv_radius")[missing], rsq.ctypes.data)
        assert L.r1_update_spheres(upd._c, 0, n, C.byref(part), None) == binding.R1_EINVAL and b"in part" in L.r1_last_error()
    for k in MAT_KEYS:
        part = binding.SphereUpdate()
        for kk, v in zip(MAT_KEYS, mats):
            if kk != k:
                setattr(part, kk, v.ctypes.data)
        assert L.r1_update_spheres(upd._c, 0, n, C.byref(part), None) == binding.R1_EINVAL and b"in part" in L.r1_last_error()
    part = binding.SphereUpdate()
    part.center_x, part.center_z = ptr[7], ptr[9]
    assert L.r1_update_spheres_device(upd._c, 0, n, C.byref(part), None) == binding.R1_EINVAL and b"in part" in L.r1_last_error()
    expect_refusal(lambda: upd.update_spheres_device(0, n - 1, radii=(ptr[0] + 2, ptr[1])), "4-byte aligned")
    expect_refusal(lambda: upd.update_spheres_device(0, n - 1, materials=(ptr[2], ptr[3], ptr[4] + 1, ptr[5], ptr[6])), "4-byte aligned")
    for bad_rsq, bad_inv in ((1.0, 0.0), (1.0, np.nan), (np.inf, 1.0), (np.nan, 1.0)):          # the active set does not change
        r2, i2 = rsq.copy(), inv.copy()
        r2[lat[3]], i2[lat[3]] = bad_rsq, bad_inv
        expect_refusal(lambda: upd.update_spheres(0, radii=(r2, i2)), "inactive")
    m2 = [v.copy() for v in mats]
    m2[0][lat[5]] = 3
    expect_refusal(lambda: upd.update_spheres(0, materials=tuple(m2)), "no material")
    yb = y.copy()
    yb[lat[3]] = np.inf
    expect_refusal(lambda: upd.update_spheres(0, centers=(x, yb, z), radii=(rsq, inv)), "not finite")
    same(upd.render(p)[:2], original, "after refused updates")
    tables_equal(upd.tables_download(), tables0, "after refused updates")
    assert upd.bvh_download().tobytes() == rows0.tobytes()
    for variant in EVERY_VARIANT:
        same(upd.render(params("large", variant))[:2], original, ("every variant before any update", variant))
    # a progressive accumulation ends at any update, materials alone included; an update is no launch of a frame
    half = r1.make_params(p.width, p.height, 2, p.seed)
    for kind in ("materials", "radii"):
        upd.render_pass(half, 0)
        upd.render_pass(half, 2)
        upd.render_pass(half, 0)
        before = upd.launch_info()
        if kind == "materials":
            upd.update_spheres(0, materials=material_family(a, "identity"))
        else:
            upd.update_spheres(0, radii=(rsq, inv))
        assert upd.launch_info() == before
        with pytest.raises(binding.R1Error) as e:
            upd.render_pass(half, 2)
        assert e.value.code == binding.R1_EINVAL
        if kind == "materials":  # nothing is refused, and r1_set_scene with the same arrays still finds everything current
            for variant in EVERY_VARIANT:
                same(upd.render(params("large", variant))[:2], original, ("after an identity materials update", variant))
    # after the radii update: the variants whose structures were not refitted stop, and say why
    for variant in (binding.VARIANT_PREFILTER, binding.VARIANT_STATS, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID, binding.VARIANT_GRID_STATS):
        expect_refusal(lambda: upd.render(params("large", variant)), MOVED_RULE)
        expect_refusal(lambda: upd.render(params("large", variant)), "r1_set_scene rebuilds")
    rays = np.zeros((4, 8), F)
    rays[:, 6] = -1
    rays[:, 3] = 100
    expect_refusal(lambda: upd.cast_rays(rays, binding.CAST_CLOSEST, binding.VARIANT_GRID), MOVED_RULE)
    grown = upd.render(p)[:2]
    same(upd.render(params("large", binding.VARIANT_BVH_STATS))[:2], grown, "the tree's diagnostic build after an update")
    build_fresh(fresh, edited(a, radii=(rsq, inv)), sc.camera.contents)
    same(grown, fresh.render(p)[:2], "grown")
    assert grown[0].tobytes() != original[0].tobytes()
    # the trap: r1_set_scene with the ORIGINAL arrays must rebuild, not find "everything current"
    upd.set_scene(sc)
    same(upd.render(p)[:2], original, "r1_set_scene(original arrays) after an update")
    for variant in EVERY_VARIANT:
        same(upd.render(params("large", variant))[:2], original, ("re-enabled", variant))
    tables_equal(upd.tables_download(), tables0, "r1_set_scene(original arrays)")
    # the same through the device form, where the host copies never saw the values
    upd.update_spheres_device(0, n, radii=(ptr[0], ptr[1]))
    same(upd.render(p)[:2], grown, "device form")
    upd.set_scene(sc)
    same(upd.render(p)[:2], original, "r1_set_scene(original arrays) after a device-form update")
    # host-form materials: the host copies follow, and r1_set_scene with either set of arrays leaves a fresh context's state
    upd.update_spheres(0, materials=mats)
    got = upd.render(p)[:2]
    cs, keep = raw_from_arrays(edited(a, materials=mats))
    upd.set_scene_raw(cs, sc.camera.contents)
    for variant in EVERY_VARIANT:
        same(upd.render(params("large", variant))[:2], got, ("r1_set_scene(edited arrays) on the updated context", variant))
    upd.set_scene(sc)
    same(upd.render(params("large", binding.VARIANT_GRID))[:2], original, "r1_set_scene(original arrays) after a materials update")
    tables_equal(upd.tables_download(), tables0, "back to the original")


# ---- 8: the drop-in program --------------------------------------------------------------------------------------------------------------------


def program_pulse(a, f, frames):
    """(radii, materials) of frame f of --pulse FRAMES for r1_update_spheres: the program's rule restated, the factors in fp64 and rounded to
    fp32; math.sin and math.cos are the C library's.  A scale of exactly 1 keeps the scene's own radius_sq and inv_radius; otherwise the radius
    is fp32(scale / fp64(inv_radius)), stored as r * r and 1 / r in fp32.  Material types and parameters stay."""
    rsq, inv = a["radius_sq"].copy(), a["inv_radius"].copy()
    alb = [a[k].copy() for k in ("albedo_r", "albedo_g", "albedo_b")]
    t = f / frames
    swing, mix = 0.3 * math.sin(2.0 * math.pi * t), 0.5 * (1.0 - math.cos(2.0 * math.pi * t))
    for i in program_lattice(a):
        scale = 1.0 + swing * math.cos(2.0 * math.pi * (i % 8) / 8.0)
        if scale != 1.0:
            r = F(scale / float(a["inv_radius"][i]))
            rsq[i], inv[i] = r * r, F(1.0) / r
        own = [float(a[k][i]) for k in ("albedo_r", "albedo_g", "albedo_b")]
        for c in range(3):  # each channel towards the one before it: r -> g -> b -> r
            alb[c][i] = F(own[c] + (own[(c + 2) % 3] - own[c]) * mix)
    return (rsq, inv), (a["mat_type"], alb[0], alb[1], alb[2], a["mat_param"])


def test_rayweek1_hip_pulse(upd, tmp_path):
    """--pulse: one `pulse:` line per scene; with -w the first and the middle frame, which differ; the first is benchmark()'s own frame, the
    middle one is, in bytes, what a context renders after r1_update_spheres with the program's rule."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rays1bench_amd", "lib", "rayweek1_hip")
    w, h, spp = 64, 48, 2
    out = subprocess.run([exe, "--pulse", "3", "-n", "1", "-w", "--width", str(w), "--height", str(h), "--spp", str(spp)], cwd=tmp_path,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " pulse: " in l]
    assert [l.split()[0] for l in lines] == ["small", "medium", "large"], out.stdout[-2000:]
    for l in lines:
        m = re.search(r"pulse: 3 frames, (\d+) of (\d+) spheres pulsing, update ([0-9.]+) ms per frame .* render ([0-9.]+) ms per frame, (\d+) rays", l)
        assert m and int(m.group(5)) > 0, l
    assert "480 of" in lines[2]
    for scene in ("small", "medium", "large"):
        first, middle = ((tmp_path / f"pulse_{scene}_{f:03d}.tga").read_bytes() for f in (0, 1))
        assert len(first) == len(middle) == 18 + w * h * 3
        assert (first != middle) == (scene != "small"), scene  # (the small scene has no lattice: its four spheres stay)
        assert first == (tmp_path / f"out_{scene}.tga").read_bytes(), (scene, "frame 0 of --pulse is the frame without it")
    for scene, make in PROGRAM_SCENES:
        sc = make(w, h)
        radii, materials = program_pulse(sc.arrays(), 1, 3)
        upd.set_scene(sc)
        upd.update_spheres(0, radii=radii, materials=materials)
        same_tga(tmp_path / f"pulse_{scene}_001.tga", w, h, upd.render(r1.make_params(w, h, spp, 10001))[0], scene)
