"""GPU tests of the re-sort: r1_resort_spheres re-deals the spheres into the box tree's leaf slots on the device — the
topology, every table shape and every trace kernel stay — and refits.  The contract is the updates' own: every render and query afterwards
gives, byte for byte and ray for ray, what a FRESH context gives after r1_set_scene with the context's current spheres; and the device's
ids and rows equal the host restatement's (r1_bvh_resort_describe), bit for bit.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_bvh_host import EMPTY, F
from test_gpu_update import CASES, MOVED_RULE, edge_arrays, edge_camera, expect_refusal, first_difference, fresh_render, params, same
from test_refit_host import edge_scene, lattice_of, moved_centres, raw_from_arrays

pytestmark = pytest.mark.gpu

# The kernels of r1_resort.hip work in blocks of 256 lanes, one item per lane (R1_SORT_BLOCK, r1_device_sort.h), and their prefix sum and
# their radix sort are r1_device_sort.hip's: the three-launch form that recurses where the block sums exceed a block.  With M movable spheres:
#   the flags' prefix sum runs over 3 M items:   one block alone while 3 M <= 256      (M <= 85),
#                                                a second level from               M = 86,
#                                                a third level from 3 M > 65 536:  M = 21 846;
#   the radix sort's histogram has 3 x 256 x ceil(M / 256) entries: one block of keys per axis while M <= 256, many blocks from M = 257;
#                                                its prefix sum has two levels from M = 1 and a third from 768 ceil(M / 256) > 65 536: M = 21 761.
# The cases lie on both sides of each: the edge trees (M <= 5), large (M = 480: many blocks, second level), grid40x30 (1200), grid160x100
# (16 000: the largest two-level case) and grid400x250 (100 000: the third level of both) — asserted in test_the_cases_cover_every_level.
SORT_BLOCK = 256
LEVELS = (85, 256, 21760, 21845)  # the largest M below each threshold above
BIG = "grid400x250"
BIG_FRAME = (96, 54, 1)


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
        sc = r1.create_large_scene(w, h) if name == "large" else r1.create_grid_scene(w, h, *(int(v) for v in name[4:].split("x")))
        out[name] = (sc, sc.arrays())
    sc = r1.create_grid_scene(BIG_FRAME[0], BIG_FRAME[1], 400, 250)
    out[BIG] = (sc, sc.arrays())
    return out


def frame(name, variant=0, seed=777):
    return r1.make_params(*BIG_FRAME, seed, variant=variant) if name == BIG else params(name, variant, seed)


def host_resort(sc, x, y, z, rsq=None, inv=None):
    info, rows, ids = binding.bvh_resort_describe(sc.spheres.contents, x, y, z, rsq, inv)
    return rows, ids


def device_equals_host(upd, sc, x, y, z, what, rsq=None, inv=None):
    rows, ids = host_resort(sc, x, y, z, rsq, inv)
    got_ids, got_rows = upd.bvh_ids_download(), upd.bvh_download()
    assert got_ids.shape == ids.shape and np.array_equal(got_ids, ids), (what, "ids", np.nonzero(got_ids != ids)[0][:8])
    assert got_rows.shape == rows.shape
    assert got_rows.tobytes() == rows.tobytes(), (what, first_difference(got_rows, rows))
    return ids


def test_the_cases_cover_every_level(scenes):
    m = {name: len(lattice_of(a)) for name, (sc, a) in scenes.items()}
    assert m == {"large": 480, "grid40x30": 1200, "grid160x100": 16000, BIG: 100000}, m
    edge = 5
    assert edge <= LEVELS[0] < m["large"]                                     # the flags' prefix sum: one block | two levels
    assert edge <= LEVELS[1] < m["large"]                                     # the radix sort: one block of keys | many
    assert m["grid160x100"] <= LEVELS[2] < LEVELS[3] < m[BIG]                 # the third level of both prefix sums
    assert 3 * LEVELS[0] <= SORT_BLOCK < 3 * (LEVELS[0] + 1) and 3 * LEVELS[3] <= SORT_BLOCK ** 2 < 3 * (LEVELS[3] + 1)
    assert 768 * (-(-LEVELS[2] // SORT_BLOCK)) <= SORT_BLOCK ** 2 < 768 * (-(-(LEVELS[2] + 1) // SORT_BLOCK))


# ---- equals a fresh build; device equals host ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("move", ("identity", "permute", "jitter", "far"))
@pytest.mark.parametrize("name", list(CASES))
def test_resort_equals_fresh_build(upd, fresh, scenes, name, move):
    sc, a = scenes[name]
    x, y, z = moved_centres(a, move)
    upd.set_scene(sc)
    info = binding.bvh_describe(sc.spheres.contents)[0]
    assert info["pad_local"] == CASES[name][3] and (info["spheres"] > 1023) == CASES[name][4], info
    upd.update_centers(0, x, y, z)
    upd.resort_spheres()
    p = frame(name)
    want = fresh_render(fresh, a, sc.camera.contents, x, y, z, p)
    same(upd.render(p)[:2], want, (name, move, "default"))
    assert upd.launch_info()["kernel"] == binding.VARIANT_BVH
    same(upd.render(frame(name, binding.VARIANT_BVH))[:2], want, (name, move, "bvh"))
    same(upd.render(frame(name, binding.VARIANT_REFERENCE))[:2], want, (name, move, "reference on the re-sorted context"))
    if move == "permute":
        gs, ws = upd.render_samples(p), fresh.render_samples(p)
        assert gs[1] == ws[1] and gs[2].tobytes() == ws[2].tobytes(), (name, move, "samples")


@pytest.mark.parametrize("name", list(CASES))
def test_device_ids_and_rows_equal_the_host_resort(upd, scenes, name):
    sc, a = scenes[name]
    upd.set_scene(sc)
    built = binding.bvh_describe(sc.spheres.contents)
    assert np.array_equal(upd.bvh_ids_download(), built[2])  # before any re-sort: the builder's ids
    upd.resort_spheres()                                     # valid before any update
    device_equals_host(upd, sc, a["center_x"], a["center_y"], a["center_z"], (name, "no update"))
    for move in ("permute", "jitter", "far", "collapse", "lift"):
        x, y, z = moved_centres(a, move)
        upd.update_centers(0, x, y, z)
        upd.resort_spheres()
        ids = device_equals_host(upd, sc, x, y, z, (name, move))
        assert np.array_equal(np.sort(ids), np.sort(built[2]))


def test_one_large_tree(upd, fresh, scenes):
    """100 000 movable spheres: the third level of both prefix sums, 391 blocks of keys per axis."""
    sc, a = scenes[BIG]
    x, y, z = moved_centres(a, "permute")
    upd.set_scene(sc)
    upd.update_centers(0, x, y, z)
    upd.resort_spheres()
    device_equals_host(upd, sc, x, y, z, BIG)
    p = frame(BIG)
    same(upd.render(p)[:2], fresh_render(fresh, a, sc.camera.contents, x, y, z, p), BIG)


# ---- updates after a re-sort ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(CASES))
def test_updates_after_a_resort(upd, fresh, scenes, name):
    import torch
    sc, a = scenes[name]
    cam, p = sc.camera.contents, frame(name)
    upd.set_scene(sc)
    x, y, z = moved_centres(a, "permute")
    upd.update_centers(0, x, y, z)
    upd.resort_spheres()
    # the slot table was rewritten: a host-form move must find every sphere
    x, y, z = moved_centres(a, "jitter")
    upd.update_centers(0, x, y, z)
    same(upd.render(p)[:2], fresh_render(fresh, a, cam, x, y, z, p), (name, "host-form move after a re-sort"))
    # the device form
    x, y, z = moved_centres(a, "lift")
    t = [torch.from_numpy(v).cuda() for v in (x, y, z)]
    upd.update_centers_device(0, len(x), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    same(upd.render(p)[:2], fresh_render(fresh, a, cam, x, y, z, p), (name, "device-form move after a re-sort"))
    # radii
    lat = lattice_of(a)
    rad = np.sqrt(a["radius_sq"].astype(np.float64))
    rad[lat] *= np.random.default_rng(3).uniform(0.6, 1.4, len(lat))
    rsq, inv = (rad * rad).astype(F), (1.0 / np.maximum(rad, 1e-30)).astype(F)
    inv[a["inv_radius"] == 0] = 0
    upd.update_spheres(0, radii=(rsq, inv))
    edited = dict(a)
    edited["radius_sq"], edited["inv_radius"] = rsq, inv
    want = fresh_render(fresh, edited, cam, x, y, z, p)
    same(upd.render(p)[:2], want, (name, "radii after a re-sort"))
    # and a re-sort of all that
    upd.resort_spheres()
    same(upd.render(p)[:2], want, (name, "second re-sort"))
    same(upd.render(frame(name, binding.VARIANT_REFERENCE))[:2], want, (name, "second re-sort, reference"))
    ids = device_equals_host(upd, sc, x, y, z, (name, "second re-sort"), rsq, inv)
    # nothing changed in between: no byte changes
    rows = upd.bvh_download()
    upd.resort_spheres()
    assert upd.bvh_ids_download().tobytes() == ids.tobytes() and upd.bvh_download().tobytes() == rows.tobytes()
    same(upd.render(p)[:2], want, (name, "third re-sort"))


# ---- it helps ---------------------------------------------------------------------------------------------------------------------------------


def test_node_visits_drop_below_the_refit_alone(upd, fresh, scenes):
    """DESIGN.md §4.29 records the three figures.  Only the ordering is asserted: the CPU box areas predict about 17 x the fresh build's for
    the refit alone against about 1.1 x after the re-sort."""
    sc, a = scenes["large"]
    x, y, z = moved_centres(a, "permute")
    p = frame("large", binding.VARIANT_BVH_STATS)
    upd.set_scene(sc)
    upd.update_centers(0, x, y, z)
    refit = upd.render(p)[:2]
    visits_refit = upd.last_stats()["raw"][9]
    upd.resort_spheres()
    resorted = upd.render(p)[:2]
    visits_resorted = upd.last_stats()["raw"][9]
    cs, keep = raw_from_arrays(a, x, y, z)
    fresh.set_scene_raw(cs, sc.camera.contents)
    built = fresh.render(p)[:2]
    visits_fresh = fresh.last_stats()["raw"][9]
    print(f"node visits, large after permute, {p.width}x{p.height}x{p.spp}: refit alone {visits_refit}, re-sorted {visits_resorted}, fresh build {visits_fresh}")
    same(refit, built, "refit alone"), same(resorted, built, "re-sorted")
    assert 0 < visits_resorted < visits_refit, (visits_resorted, visits_refit, visits_fresh)


# ---- queries ----------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(CASES))
def test_ray_and_path_queries_after_a_resort(upd, scenes, name):
    sc, a = scenes[name]
    x, y, z = moved_centres(a, "permute")
    upd.set_scene(sc)
    upd.update_centers(0, x, y, z)
    upd.resort_spheres()
    cs, keep = raw_from_arrays(a, x, y, z)
    rng = np.random.default_rng(19)
    n = 4096
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = np.stack([rng.uniform(-12, 12, n), rng.uniform(0.5, 6, n), rng.uniform(-12, 12, n)], 1)
    act = np.nonzero(a["inv_radius"] != 0)[0]
    tgt = act[rng.integers(0, len(act), n)]
    d = np.stack([x[tgt], y[tgt], z[tgt]], 1).astype(np.float64) + rng.normal(0, 0.05, (n, 3)) - rays[:, 0:3]
    rays[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    rays[:, 3] = np.where(rng.random(n) < 0.25, rng.uniform(0.5, 8, n), np.finfo(F).max).astype(F)
    for mode in (binding.CAST_CLOSEST, binding.CAST_ANY):
        want = upd.cast_rays(rays, mode, binding.VARIANT_REFERENCE)
        assert want.tobytes() == binding.cast_rays_host(cs, rays, mode).tobytes(), (name, mode, "reference form")
        assert (want["index"] >= 0).sum() > n // 4 if mode == binding.CAST_CLOSEST else want.sum() > n // 4
        assert upd.cast_rays(rays, mode, binding.VARIANT_DEFAULT).tobytes() == want.tobytes(), (name, mode)
    expect_refusal(lambda: upd.cast_rays(rays, binding.CAST_CLOSEST, binding.VARIANT_GRID), MOVED_RULE)
    want = upd.trace_rays(rays, variant=binding.VARIANT_REFERENCE)
    assert (want["rays"] > 1).sum() > n // 4
    assert upd.trace_rays(rays, variant=binding.VARIANT_DEFAULT).tobytes() == want.tobytes(), (name, "trace")


# ---- stream order -----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["large", "grid40x30"])
def test_stream_order(upd, fresh, scenes, name):
    """Frame A, the re-sort and frame B on one stream, one wait: both frames are the moved scene's — the re-sort changes no pixel — and what
    frame B walked shows in the ids alone."""
    sc, a = scenes[name]
    w, h = CASES[name][:2]
    p = frame(name)
    x, y, z = moved_centres(a, "permute")
    fa, fb = binding.HostFrames(w, h, 1), binding.HostFrames(w, h, 1)
    try:
        upd.set_scene(sc)
        upd.update_centers(0, x, y, z)
        upd.render_async(p, fa)
        upd.resort_spheres()
        upd.render_async(p, fb)
        upd.sync()
        want = fresh_render(fresh, a, sc.camera.contents, x, y, z, p)
        assert fa.rays(0) == want[1] and fa.image(0).tobytes() == want[0].tobytes(), "frame A: the refitted tree"
        assert fb.rays(0) == want[1] and fb.image(0).tobytes() == want[0].tobytes(), "frame B: the re-sorted tree"
        ids = device_equals_host(upd, sc, x, y, z, (name, "after both frames"))
        assert not np.array_equal(ids, binding.bvh_describe(sc.spheres.contents)[2])
    finally:
        fa.close(), fb.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------------


def test_state_rules(upd, fresh, scenes):
    sc, a = scenes["large"]
    p = frame("large")
    blank = r1.Renderer(0)
    try:
        expect_refusal(lambda: blank.resort_spheres(), "no scene set")
        expect_refusal(lambda: blank.bvh_ids_download(), "no scene set")
    finally:
        blank.close()
    assert binding.lib().r1_resort_spheres(None, None) == binding.R1_EINVAL
    upd.set_scene(sc)
    original = upd.render(p)[:2]
    same(upd.render(frame("large", binding.VARIANT_GRID))[:2], original, "grid before the re-sort")
    # a progressive accumulation ends; the launch info stays
    half = r1.make_params(p.width, p.height, 2, p.seed)
    upd.render_pass(half, 0)
    before = upd.launch_info()
    upd.resort_spheres()
    assert upd.launch_info() == before
    with pytest.raises(binding.R1Error) as e:
        upd.render_pass(half, 2)
    assert e.value.code == binding.R1_EINVAL
    # the variants whose structures were not re-sorted stop, and say why
    for variant in (binding.VARIANT_PREFILTER, binding.VARIANT_GRID):
        expect_refusal(lambda: upd.render(frame("large", variant)), MOVED_RULE)
    same(upd.render(p)[:2], original, "the unmoved scene, re-sorted")
    # r1_set_scene re-enables them — with the same arrays too: it must rebuild, not find "everything current"
    upd.set_scene(sc)
    assert np.array_equal(upd.bvh_ids_download(), binding.bvh_describe(sc.spheres.contents)[2])
    same(upd.render(frame("large", binding.VARIANT_GRID))[:2], original, "grid re-enabled")
    same(upd.render(frame("large", binding.VARIANT_PREFILTER))[:2], original, "prefilter re-enabled")
    # a scene without a movable sphere: R1_OK, and the state stays
    cs, arrs, mt = edge_scene(0)
    cam = edge_camera(64, 48)
    q = r1.make_params(64, 48, 2, 31)
    upd.set_scene_raw(cs, cam)
    empty = upd.render(q)[:2]
    upd.render_pass(r1.make_params(64, 48, 1, 31), 0)
    upd.resort_spheres()
    upd.render_pass(r1.make_params(64, 48, 1, 31), 1)  # the accumulation goes on
    same(upd.render(r1.make_params(64, 48, 2, 31, variant=binding.VARIANT_GRID))[:2], empty, "grid after a re-sort of nothing")


# ---- edge trees -------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_active", [0, 1, 4, 5])
def test_edge_trees_with_placeholders(upd, fresh, n_active):
    import torch
    cs, arrs, mt = edge_scene(n_active)
    a = edge_arrays(arrs, mt)
    w, h = 64, 48
    cam = edge_camera(w, h)
    p = r1.make_params(w, h, 3, 31)
    rng = np.random.default_rng(60 + n_active)
    x, y, z = ((arrs[k] + rng.uniform(-2, 2, cs.count)).astype(F) for k in ("center_x", "center_y", "center_z"))
    upd.set_scene_raw(cs, cam)
    upd.update_centers(0, x, y, z)
    upd.resort_spheres()
    want = fresh_render(fresh, a, cam, x, y, z, p)
    same(upd.render(p)[:2], want, (n_active, "default"))
    same(upd.render(r1.make_params(w, h, 3, 31, variant=binding.VARIANT_REFERENCE))[:2], want, (n_active, "reference"))
    info, rows, ids = binding.bvh_resort_describe(cs, x, y, z)
    assert np.array_equal(upd.bvh_ids_download(), ids) and upd.bvh_download().tobytes() == rows.tobytes()
    if n_active == 0:
        return
    # a NaN centre through the device form: the sphere can never be hit; r1_set_scene with the same arrays drops it
    act = np.nonzero(arrs["inv_radius"] != 0)[0]
    xn = x.copy()
    xn[act[-1]] = np.nan
    t = [torch.from_numpy(v).cuda() for v in (xn, y, z)]
    upd.update_centers_device(0, len(xn), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    upd.resort_spheres()
    same(upd.render(p)[:2], fresh_render(fresh, a, cam, xn, y, z, p), (n_active, "NaN centre"))
    info, rows, ids = binding.bvh_resort_describe(cs, xn, y, z)
    assert np.array_equal(upd.bvh_ids_download(), ids) and upd.bvh_download().tobytes() == rows.tobytes()
