"""GPU tests of the uniform grid's (R1_VARIANT_GRID) paths that tests/test_gpu_grid.py does not reach: the fallback tree walk with hits
(and waves that mix fallback and walking lanes), the small-scene kernel's hand-over to the big-scene one at R1_GRID_LDS_HALVES, the
tree's adversarial families, degenerate outlier / cell layouts, and scene changes and the throughput entry points.

Every frame is compared bit for bit with the reference-form kernel (R1_VARIANT_REFERENCE) and with the CPU oracle; every test also
shows that it reached the path it is about (R1_VARIANT_GRID_STATS slot 14 counts fallback lanes, or a precondition read from
r1_grid_describe / r1_grid_visit), so that it cannot pass without exercising it.  tests/test_grid_host.py checks the same
preconditions without a GPU."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o
from test_gpu_bvh import _as_ccamera, _as_cscene, _look, oparams, oracle_scene, same, spheres
from test_gpu_configs import _same_bits_or_both_nan

pytestmark = pytest.mark.gpu

GRID, GRID_STATS, REF = binding.VARIANT_GRID, binding.VARIANT_GRID_STATS, binding.VARIANT_REFERENCE
FB, OUTLIER_TESTS = 14, 15  # r1_last_stats slots of the grid's diagnostic build (include/rays1.h)


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def rays_of(samples):
    return samples[:, 3].copy().view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def halves(cs):
    """16-bit entries the small-scene grid kernel would keep in LDS: cell starts + registrations (r1_scene_grid.cpp ensure_grid)."""
    info, start, ids, outl = binding.grid_describe(cs)
    return len(start) + info["registrations"]


# ---- scenes (shared with tests/test_grid_host.py, which checks their preconditions on the host) -------------------------------------


TELE_FROM, TELE_AT, TELE_FOV = (80.0, 14.0, 18.0), (0.0, 0.5, 0.0), 12.0


def telephoto(sa, w, h):
    """A 12-degree pinhole from (80, 14, 18), far beyond V of the reference's lattices, looking at their middle."""
    return r1o.SceneArrays(sa.arrays, _look(TELE_FROM, TELE_AT, TELE_FOV, w / h, 0.0, 10.0))


def straddling_lens(sa, w, h, lens_radius=3.0):
    """A lens camera whose centre lies at V from the farthest corner of the registered centres' box (bisection, as
    tests/test_grid_host.py's v_safe test), looking at the scene: part of the lens is inside V (the grid walks) and part is outside
    (the fallback), so waves mix both."""
    info = binding.grid_describe(_as_cscene(sa))[0]
    clo, chi, v = info["centre_lo"].astype(np.float64), info["centre_hi"].astype(np.float64), float(info["v_safe"])
    mid, dirn = 0.5 * (clo + chi), unit(np.asarray(TELE_FROM) - 0.5 * (clo + chi))
    lo_s, hi_s = 0.0, 4 * v
    for _ in range(80):
        s = 0.5 * (lo_s + hi_s)
        o = mid + s * dirn
        lo_s, hi_s = (s, hi_s) if np.sqrt((np.maximum(np.abs(o - clo), np.abs(o - chi)) ** 2).sum()) < v else (lo_s, s)
    frm = mid + lo_s * dirn
    return r1o.SceneArrays(sa.arrays, _look(frm, TELE_AT, 30.0, w / h, 2 * lens_radius, np.linalg.norm(frm - TELE_AT)))


def tie_scene(w, h):
    """120 groups of four coincident registered spheres (equal centre and radius, random materials: only the lowest index may win) and
    one outlier (r = 3.5 > 4 x the median) partly in front of them, seen with a telephoto pinhole from beyond V."""
    rng = np.random.default_rng(4041)
    g = 120
    c = np.repeat(rng.uniform(-4, 4, (g, 3)) * [1, 0.5, 1], 4, axis=0)
    rad = np.repeat(rng.uniform(0.5, 0.9, g), 4)
    c = np.concatenate([c, [[6.0, 1.0, -4.5]]])
    rad = np.concatenate([rad, [3.5]])
    sa = r1o.SceneArrays(spheres(c, rad, rng), _look((55.0, 18.0, 20.0), (1.0, 0.0, -1.0), 8, w / h, 0.0, 10.0))
    return sa, 4 * g  # (the outlier's index)


def dense_box(n, radius):
    """n spheres of one radius, centres uniform in [-10, 10]^3 (prefixes of one draw): the table grows with the radius."""
    c = np.random.default_rng(5).uniform(-10, 10, (1023, 3))[:n]
    return c, np.full(n, radius)


def deep_box():
    """800 spheres of a dense box and a chain of 200 whose centres converge geometrically on one point (each SAH split peels a few off):
    a tree twice as deep as the large scene's, with a table just under R1_GRID_LDS_HALVES."""
    rng = np.random.default_rng(5)
    c = rng.uniform(-10, 10, (800, 3))
    d = 6.0 * 2.0 ** -np.arange(200)
    tail = np.stack([d, np.zeros(200), np.zeros(200)], 1) + [3.0, 2.0, 1.0]
    return np.concatenate([c, tail]), np.full(1000, 1.15)


LIMIT_SCENES = {"under": lambda: dense_box(1001, 1.12), "over": lambda: dense_box(1002, 1.12), "deep": deep_box}
LIMIT_CAMERA = ((0.0, 2.0, 14.0), (0.0, 0.0, 0.0), 60)  # within V (34.6) of every registered centre: the walk, not the fallback


def limit_scene(kind, w, h):
    c, rad = LIMIT_SCENES[kind]()
    frm, at, fov = LIMIT_CAMERA
    return r1o.SceneArrays(spheres(c, rad, np.random.default_rng(17)), _look(frm, at, fov, w / h, 0.1, 14.0))


SHAPES = ["all_outliers", "one_registered", "no_outliers", "300_outliers", "coincident_centres", "collinear_x", "collinear_y", "collinear_z"]


def shape_scene(shape, w, h):
    """Degenerate layouts of the grid builder (r1_grid.cpp): (scene arrays and camera, expected describe fields)."""
    rng = np.random.default_rng(500 + SHAPES.index(shape))
    cam = _look((9.0, 5.0, 16.0), (0.0, 0.0, 0.0), 45, w / h, 0.05, 18.0)
    if shape == "all_outliers":  # 500 balls of r = 5 in a box of 10: every padded ball spans more than R1_GRID_SPAN_MAX cells
        c, rad = rng.uniform(-5, 5, (500, 3)), np.full(500, 5.0)
        cam = _look((14.0, 8.0, 22.0), (0.0, 0.0, 0.0), 50, w / h, 0.05, 25.0)
        want = {"outliers": 500, "registrations": 0, "registered": []}
    elif shape == "one_registered":  # a crowd of r = 8 (every one spans too many cells) and one small sphere beside it: the only registered one
        c = np.concatenate([rng.uniform(-5, 5, (500, 3)), [[14.0, 0.0, 14.0]]])
        rad = np.concatenate([np.full(500, 8.0), [1.0]])
        cam = _look((24.0, 3.0, 20.0), (9.0, 0.0, 9.0), 50, w / h, 0.05, 12.0)
        want = {"outliers": 500, "registered": [500]}
    elif shape == "no_outliers":
        c, rad = rng.uniform(-8, 8, (300, 3)), rng.uniform(0.3, 0.9, 300)
        want = {"outliers": 0}
    elif shape == "300_outliers":  # 700 small ones and 300 of r > 4 x the median
        c = rng.uniform(-9, 9, (1000, 3))
        rad = np.concatenate([rng.uniform(0.05, 0.15, 700), rng.uniform(0.7, 1.6, 300)])
        rad = rad[rng.permutation(1000)]
        want = {"outliers": 300}
    elif shape == "coincident_centres":  # every centre the same point: one cell
        c = np.tile([[0.5, 0.25, -0.5]], (240, 1))
        rad = np.repeat(rng.uniform(1.0, 3.5, 60), 4)
        cam = _look((6.0, 3.0, 8.0), (0.5, 0.25, -0.5), 45, w / h, 0.05, 9.0)
        want = {"outliers": 0, "cells": (1, 1, 1)}
    else:  # centres on one line along x, y or z: one cell across each of the other two axes
        a = "xyz".index(shape[-1])
        c = np.full((300, 3), 0.25)
        c[:, a] = rng.uniform(-12, 12, 300)
        rad = rng.uniform(0.2, 0.6, 300)
        frm, at, up = np.full(3, 0.25), np.full(3, 0.25), np.zeros(3)
        frm[a], at[a], frm[(a + 1) % 3], up[(a + 1) % 3] = -16.0, 4.0, 2.5, 1.0  # from one end, a little to the side, along the line
        cam = _look(frm, at, 10, w / h, 0.05, 16.0, up)
        want = {"outliers": 0, "cells": tuple(None if k == a else 1 for k in range(3))}
    return r1o.SceneArrays(spheres(c, rad, rng), cam), want


def check_shape(cs, want):
    """the grid_describe fields `want` names; "registered": the sorted scene indices registered in some cell.  Returns the info."""
    info, start, ids, outl = binding.grid_describe(cs)
    for k, v in want.items():
        if k == "registered":
            assert sorted(set(ids[:info["registrations"]].tolist())) == v, v
        elif k == "cells":
            for a in range(3):
                assert info["cells"][a] > 1 if v[a] is None else info["cells"][a] == v[a], (info["cells"], v)
        else:
            assert info[k] == v, (k, info[k], v)
    return info


def boundary_plane_scene(w, h):
    """Rays that run exactly in a cell-boundary plane x = lo + k cell (exact in fp32): horizontal = 0, so d.x = 0 for every primary
    ray, and the origin's x is the plane.  Returns the scene and the plane's x."""
    rng = np.random.default_rng(610)
    n = 400
    c = rng.uniform(-6, 6, (n, 3))
    rad = rng.uniform(0.2, 0.7, n)
    arr = spheres(c, rad, rng)
    cam = np.zeros(22, np.float32)
    info = binding.grid_describe(_as_cscene(r1o.SceneArrays(arr, cam)))[0]
    lo, cell, n_x = float(info["lo"][0]), float(info["cell"][0]), int(info["cells"][0])
    for k in range(n_x // 2, n_x):
        x = np.float32(lo + k * cell)
        if float(x) == float(np.float32(lo)) + k * float(np.float32(cell)):
            break
    else:
        raise AssertionError("no cell boundary of the grid is exact in fp32")
    cam[0:3] = (x, 0.5, 11.0)               # (within V of every registered centre: the walk, not the fallback)
    cam[3:6] = (x, -4.0, 1.0)               # lower_left: d.x = 0 exactly
    cam[6:9], cam[9:12] = (0, 9.0, 0), (0, 0, -9.0)  # `horizontal` along y, `vertical` along -z: both without an x component
    cam[12:15], cam[15:18], cam[18:21] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    return r1o.SceneArrays(arr, cam), x


# ---- comparison ----------------------------------------------------------------------------------------------------------------------


def check_grid(renderer, sa, w, h, spp, seed, oracle="frame", **kw):
    """GRID against the reference-form kernel (samples, ray count, pixels) and the CPU oracle: the whole frame, or 120 random
    pixel-samples (oracle="samples") for scenes too large for a brute-force frame.  Returns the grid's frame."""
    renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
    got = renderer.render_samples(r1.make_params(w, h, spp, seed, variant=GRID, **kw))
    assert renderer.launch_info()["kernel"] == GRID
    ref = renderer.render_samples(r1.make_params(w, h, spp, seed, variant=REF, **kw))
    assert got[1] == ref[1], (got[1], ref[1])
    assert got[2].tobytes() == ref[2].tobytes()
    assert got[0].tobytes() == ref[0].tobytes()
    if oracle == "frame":
        oimg, orays, osamples = r1o.render_frame(sa, oparams(r1.make_params(w, h, spp, seed, **kw)), want_samples=True)
        assert got[1] == orays
        assert (rays_of(got[2]) == rays_of(osamples)).all()
        assert _same_bits_or_both_nan(got[2][:, :3], osamples[:, :3])
    else:
        rng = np.random.default_rng(seed)
        xs, ys, ss = rng.integers(0, w, 120), rng.integers(0, h, 120), rng.integers(0, spp, 120)
        rgb, orays = r1o.trace_samples(sa, w, h, seed, xs, ys, ss, kw.get("max_bounces", 50))
        pick = got[2][(ys * w + xs) * spp + ss]
        assert (rays_of(pick) == orays).all()
        assert pick[:, :3].tobytes() == rgb.tobytes()
    return got


def grid_stats(renderer, w, h, spp, seed, want):
    """The diagnostic build on the scene set last: same frame as `want`; returns its raw counters."""
    img, rays, _ = renderer.render(r1.make_params(w, h, spp, seed, variant=GRID_STATS))
    assert renderer.launch_info()["kernel"] == GRID_STATS
    assert rays == want[1] and img.tobytes() == want[0].tobytes()
    return renderer.last_stats()["raw"]


# ---- A. the fallback with hits ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["large", "lattice"])
def test_fallback_walk_hits_from_beyond_v(renderer, kind):
    """Every primary ray starts beyond V: the lane takes the fallback tree walk, and most of them hit (the frame has more than 1.5 rays
    per sample).  The bounced rays start inside V, so the same frame switches back to the grid.  The large scene (484 spheres) runs the
    small-scene grid kernel, the 48 x 36 lattice (1 732 spheres) the big-scene one."""
    w, h, spp = 96, 64, 2
    sc = r1.create_large_scene(w, h) if kind == "large" else r1.create_grid_scene(w, h, 48, 36)
    sa = telephoto(oracle_scene(sc), w, h)
    assert binding.grid_visit(_as_cscene(sa), sa.camera_array[0:3], unit(np.subtract(TELE_AT, TELE_FROM)).astype(np.float32))[3]
    got = check_grid(renderer, sa, w, h, spp, 41)
    raw = grid_stats(renderer, w, h, spp, 41, got)
    n = w * h * spp
    assert raw[FB] >= 0.9 * n, (raw[FB], n)
    assert got[1] > 1.5 * n, got[1]
    assert raw[OUTLIER_TESTS] > 0


def test_fallback_and_walk_in_the_same_waves(renderer):
    """A lens that straddles V: some lanes of a wave take the fallback, their neighbours walk the grid; both keep their hits."""
    w, h, spp = 96, 64, 3
    sa = straddling_lens(oracle_scene(r1.create_large_scene(w, h)), w, h)
    got = check_grid(renderer, sa, w, h, spp, 43)
    raw = grid_stats(renderer, w, h, spp, 43, got)
    n = w * h * spp
    assert 0.1 * n < raw[FB] < 0.9 * n, (raw[FB], n)
    assert got[1] > 1.5 * n, got[1]


def test_fallback_keeps_the_lowest_index_of_coincident_spheres(renderer):
    """Ties seen from beyond V: groups of four coincident registered spheres (the fallback's tree walk must keep the first) behind an
    outlier whose offer, carried over from the outlier loop, competes with the tree's."""
    w, h, spp = 96, 64, 3
    sa, big = tie_scene(w, h)
    info, start, ids, outl = binding.grid_describe(_as_cscene(sa))
    assert outl.tolist() == [big] and set(ids.tolist()) == set(range(big))
    got = check_grid(renderer, sa, w, h, spp, 45)
    raw = grid_stats(renderer, w, h, spp, 45, got)
    n = w * h * spp
    assert raw[FB] >= 0.9 * n and got[1] > 1.3 * n, (raw[FB], got[1], n)


# ---- B. the small-scene grid kernel's table limit ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", list(LIMIT_SCENES))
def test_table_just_under_and_over_the_lds_limit(renderer, kind):
    """<= 1023 spheres whose 16-bit table (cell starts + registrations) is just under R1_GRID_LDS_HALVES (the small-scene kernel keeps
    it in LDS, more than 4096 registrations) or just over it (the big-scene kernel, 32-bit table); and a deep tree with a table at the
    limit: the largest LDS footprint of the small-scene kernel (traversal stack of the fallback + table).  Each through the synchronous
    frame, r1_render_async and PIXEL mode."""
    torch = pytest.importorskip("torch")
    from rays1bench_amd import sharding
    w, h, spp = 80, 60, 2
    sa = limit_scene(kind, w, h)
    cs = _as_cscene(sa)
    hv = halves(cs)
    info = binding.grid_describe(cs)[0]
    assert info["spheres"] <= 1023 and info["registrations"] > 4096
    assert (8000 <= hv <= 8192) if kind != "over" else (8192 < hv <= 8400), hv
    got = check_grid(renderer, sa, w, h, spp, 51)
    if kind == "deep":
        assert renderer.launch_info()["bvh_depth"] >= 15, renderer.launch_info()
    p = r1.make_params(w, h, spp, 51, variant=GRID)
    hf = binding.HostFrames(w, h, 1)
    renderer.render_async(p, hf)
    renderer.sync()
    assert renderer.launch_info()["kernel"] == GRID
    assert hf.rays(0) == got[1] and hf.image(0).tobytes() == got[0].tobytes()
    hf.close()
    nbytes = binding.shard_block_bytes(p)
    rec = torch.zeros(nbytes + sharding.RECORD_TRAILER, dtype=torch.uint8, device="cuda")
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    renderer.set_pixel_mode(True)
    try:
        renderer.render_shard_device(p, rec.data_ptr(), rec.data_ptr() + nbytes, st)
        renderer.assemble_device_strided(p, rec.data_ptr(), nbytes + sharding.RECORD_TRAILER, out.data_ptr(), st)
        torch.cuda.synchronize()
    finally:
        renderer.set_pixel_mode(False)
    assert sharding.total_rays(rec, 1) == got[1]
    assert out.cpu().numpy().tobytes() == got[0].tobytes()


# ---- C. the tree's adversarial families on the grid ------------------------------------------------------------------------------------


def test_grid_deep_paths_between_two_huge_spheres(renderer):
    """As test_gpu_bvh.py's: paths bounce dozens of times between a floor and a ceiling of radius 1000 (two outliers), so the attenuation
    stack runs past what the kernel keeps in LDS and is unwound with colour."""
    rng = np.random.default_rng(78)
    w, h, spp = 64, 40, 4
    n = 140
    c = np.concatenate([[[0.0, -1001.0, 0.0], [0.0, 1001.0, 0.0]], rng.uniform(-6, 6, (n - 2, 3)) * np.array([1.0, 0.12, 1.0])])
    rad = np.concatenate([[1000.0, 1000.0], rng.uniform(0.05, 0.25, n - 2)])
    arr = spheres(c, rad, rng)
    arr["mat_type"][:2] = 0
    for k, v in (("albedo_r", 0.97), ("albedo_g", 0.93), ("albedo_b", 0.9)):
        arr[k][:2] = v
    cam = r1.create_small_scene(w, h).camera_array().copy()
    cam[0:3] = (0.0, 0.0, 3.0)
    cam[3:6] = (-2.0, -1.25, 1.0)
    cam[6:9], cam[9:12] = (4.0, 0.0, 0.0), (0.0, 2.5, 0.0)
    sa = r1o.SceneArrays(arr, cam)
    assert sorted(binding.grid_describe(_as_cscene(sa))[3].tolist()) == [0, 1]
    got = check_grid(renderer, sa, w, h, spp, 32)
    n_rays = rays_of(got[2])
    deep_and_lit = (n_rays > 33) & (n_rays < 51) & (got[2][:, :3].sum(1) > 0)
    assert deep_and_lit.sum() > 20, int(deep_and_lit.sum())


def test_grid_axis_parallel_rays(renderer):
    """Every primary ray exactly (0, 0, -1): two axes without motion (r1g_axis: the origin's slab decides)."""
    rng = np.random.default_rng(8)
    w, h, spp = 48, 32, 4
    n = 200
    c = rng.uniform(-2, 2, (n, 3))
    c[:, 2] -= 6
    c[:20, :2] = 0
    arr = spheres(c, rng.uniform(0.05, 0.5, n), rng)
    cam = np.zeros(22, np.float32)
    cam[3:6] = (0, 0, -1)
    cam[12:15], cam[15:18], cam[18:21] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    got = check_grid(renderer, r1o.SceneArrays(arr, cam), w, h, spp, 4)
    assert got[1] > w * h * spp


def test_grid_rays_in_a_cell_boundary_plane(renderer):
    """Primary rays with d.x = 0 whose origin lies exactly on a cell boundary x = lo + k cell: the walk never crosses an x boundary and
    the first cell is picked by floorf on the plane itself."""
    w, h, spp = 64, 48, 3
    sa, x = boundary_plane_scene(w, h)
    got = check_grid(renderer, sa, w, h, spp, 61)
    assert got[1] > 1.3 * w * h * spp  # (the plane cuts through the cloud: most primary rays hit)


def test_grid_non_finite_spheres_are_never_hit(renderer):
    rng = np.random.default_rng(12)
    w, h, spp = 64, 40, 3
    n = 60
    arr = spheres(rng.uniform(-3, 3, (n, 3)), rng.uniform(0.1, 0.5, n), rng)
    arr["center_x"][3], arr["center_y"][7], arr["center_z"][11] = np.nan, np.inf, -np.inf
    arr["radius_sq"][13], arr["radius_sq"][17] = np.inf, np.nan
    sa = r1o.SceneArrays(arr, r1.create_small_scene(w, h).camera_array())
    info, start, ids, outl = binding.grid_describe(_as_cscene(sa))
    assert info["spheres"] == n - 5 and not ({3, 7, 11, 13, 17} & (set(ids.tolist()) | set(outl.tolist())))
    got = check_grid(renderer, sa, w, h, spp, 3)
    assert got[1] > w * h * spp


def test_grid_random_scene_stress(renderer):
    """40 random scenes (as test_gpu_bvh.py's stress, other seeds): uniform, clustered, lattice-like and shell layouts, radii over three
    decades, a ground sphere in some, cameras inside and outside the cloud."""
    rng = np.random.default_rng(20261016)
    w, h, spp = 48, 32, 2
    base = r1.create_small_scene(w, h)
    fallbacks = 0
    for trial in range(40):
        n = int(rng.integers(1, 401))
        layout = trial % 4
        if layout == 0:
            c = rng.uniform(-10, 10, (n, 3))
        elif layout == 1:
            c = rng.normal(0, 0.8, (n, 3)) + rng.uniform(-6, 6, (1, 3))
        elif layout == 2:
            g = int(np.ceil(np.sqrt(n)))
            ij = np.stack(np.meshgrid(np.arange(g), np.arange(g)), -1).reshape(-1, 2)[:n]
            c = np.concatenate([ij - g / 2 + rng.uniform(0, 0.9, (n, 2)), np.full((n, 1), 0.2)], 1)[:, [0, 2, 1]]
        else:
            u = rng.normal(0, 1, (n, 3))
            c = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(2, 9)
        rad = np.exp(rng.uniform(np.log(3e-3), np.log(3.0), n))
        if trial % 5 == 0:
            rad[0], c[0] = 500.0, (0, -500.5, 0)
        arr = spheres(c, rad, rng)
        cam = base.camera_array().copy()
        if trial % 3 == 0:
            shift = c.mean(0).astype(np.float32) - cam[0:3]
            cam[0:3] += shift
            cam[3:6] += shift
        sa = r1o.SceneArrays(arr, cam)
        renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
        got = renderer.render_samples(r1.make_params(w, h, spp, 3000 + trial, variant=GRID))
        ref = renderer.render_samples(r1.make_params(w, h, spp, 3000 + trial, variant=REF))
        assert same(got, ref), (trial, n, layout)
        if trial % 8 == 0:
            oimg, orays, osamples = r1o.render_frame(sa, oparams(r1.make_params(w, h, spp, 3000 + trial)), want_samples=True)
            assert got[1] == orays and got[2].tobytes() == osamples.tobytes(), trial
        fallbacks += binding.grid_visit(_as_cscene(sa), cam[0:3], unit(cam[3:6] + 0.5 * cam[6:9] + 0.5 * cam[9:12] - cam[0:3]).astype(np.float32))[3]
    assert fallbacks < 40  # (most cameras within V: the walk itself is what is stressed)


def test_grid_300k_spheres_against_oracle_samples(renderer):
    """A 640 x 480 lattice (307 204 spheres): the big-scene grid kernel against the oracle's brute force on 120 pixel-samples, the
    tree and a tiling of its own."""
    w, h, spp = 128, 72, 2
    sc = r1.create_grid_scene(w, h, 640, 480)
    renderer.set_scene(sc)
    a = renderer.render_samples(r1.make_params(w, h, spp, 78, variant=GRID))
    assert renderer.launch_info()["kernel"] == GRID and renderer.launch_info()["spheres_active"] == 640 * 480 + 4
    b = renderer.render_samples(r1.make_params(w, h, spp, 78, tile_w=16, tile_h=8, variant=GRID))
    assert same(a, b)
    t = renderer.render_samples(r1.make_params(w, h, spp, 78, variant=binding.VARIANT_BVH))
    assert same(a, t)
    sa = oracle_scene(sc)
    rng = np.random.default_rng(4)
    xs, ys, ss = rng.integers(0, w, 120), rng.integers(0, h, 120), rng.integers(0, spp, 120)
    rgb, orays = r1o.trace_samples(sa, w, h, 78, xs, ys, ss)
    got = a[2][(ys * w + xs) * spp + ss]
    assert (rays_of(got) == orays).all()
    assert got[:, :3].tobytes() == rgb.tobytes()


# ---- D. outlier and degenerate grids ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", SHAPES)
def test_grid_outlier_and_cell_shapes(renderer, shape):
    """Every sphere an outlier (empty cells, v2 = inf), one registered sphere, no outliers (a dummy entry, n_out = 0), 300 outliers
    (the wave-uniform loop), one cell for coincident centres, one row of cells for collinear ones: shapes asserted before the frame."""
    w, h, spp = 72, 48, 3
    sa, want = shape_scene(shape, w, h)
    info = check_shape(_as_cscene(sa), want)
    got = check_grid(renderer, sa, w, h, spp, 70 + SHAPES.index(shape))
    raw = grid_stats(renderer, w, h, spp, 70 + SHAPES.index(shape), got)
    if info["outliers"]:  # (every walk tests all outliers)
        assert raw[OUTLIER_TESTS] > 0 and raw[OUTLIER_TESTS] % info["outliers"] == 0
    else:
        assert raw[OUTLIER_TESTS] == 0
    assert got[1] > 1.1 * w * h * spp  # (the scene is in view)


# ---- E. scene changes and the throughput paths -------------------------------------------------------------------------------------------


def test_grid_scene_changes_on_one_context():
    """One context: a small table, a table over the LDS limit (<= 1023 spheres), a scene of more than 1023 spheres, then the first scene
    again (GRID, DEFAULT, GRID).  The grid is rebuilt lazily after every r1_set_scene and its buffers reused; every frame equals a fresh
    context's reference-form frame."""
    w, h, spp = 80, 60, 2
    small = oracle_scene(r1.create_large_scene(w, h))
    over = limit_scene("over", w, h)
    big = oracle_scene(r1.create_grid_scene(w, h, 48, 36))
    assert halves(_as_cscene(small)) < 2048 and halves(_as_cscene(over)) > 8192
    want = {}
    fresh = r1.Renderer(0)
    try:
        for name, sa in (("small", small), ("over", over), ("big", big)):
            fresh.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
            want[name] = fresh.render(r1.make_params(w, h, spp, 90, variant=REF))[:2]
    finally:
        fresh.close()
    ctx = r1.Renderer(0)
    try:
        for name, sa, variant in (("small", small, GRID), ("over", over, GRID), ("big", big, GRID), ("small", small, GRID),
                                  ("small", small, binding.VARIANT_DEFAULT), ("small", small, GRID)):
            ctx.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
            img, rays, _ = ctx.render(r1.make_params(w, h, spp, 90, variant=variant))
            assert rays == want[name][1] and img.tobytes() == want[name][0].tobytes(), (name, variant)
    finally:
        ctx.close()


def test_grid_frames_in_flight_ragged_sizes(renderer):
    """As test_gpu_parity.py's frames in flight, through the grid: six contexts, ragged frames, five rounds each."""
    rends = [r1.Renderer(0) for _ in range(6)]
    try:
        for (w, h, spp) in ((31, 17, 9), (77, 45, 3)):
            sc = r1.create_large_scene(w, h)
            renderer.set_scene(sc)
            for r_ in rends:
                r_.set_scene(sc)
            hfs = [binding.HostFrames(w, h, 1) for _ in rends]
            for rnd in range(5):
                seeds = [1000 * rnd + 17 * k + w + 3 for k in range(len(rends))]
                for hf in hfs:
                    hf._all[:] = 0xCD
                for r_, hf, sd in zip(rends, hfs, seeds):
                    r_.render_async(r1.make_params(w, h, spp, sd, variant=GRID), hf)
                for r_ in rends:
                    r_.sync()
                for hf, sd in zip(hfs, seeds):
                    img, rays, _ = renderer.render(r1.make_params(w, h, spp, sd, variant=REF))
                    assert hf.rays(0) == rays, (w, h, spp, rnd, sd)
                    assert hf.image(0).tobytes() == img.tobytes(), (w, h, spp, rnd, sd)
            for hf in hfs:
                hf.close()
    finally:
        for r_ in rends:
            r_.close()
