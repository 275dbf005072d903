"""GPU test of the shade phase's scatter arithmetic (rays1bench_amd/csrc/r1_scatter.h, DESIGN.md §4.25: one reflection for Metal and
Dielectric, no outward normal) through every trace build: frames of 64 x 48 x 4 samples with up to 51 bounces, byte for byte and in ray
count against the CPU ORACLE's, as tests/test_gpu_builds_edges.py does.  The scenes are the materials' own:

  glass      dielectric spheres only — ground included — that overlap and nest, with indices on both sides of 1: paths run inside glass,
             meet total internal reflection and end at the depth limit or the sky with nothing on the attenuation stack;
  metal0/1   metal only, fuzz exactly 0 / exactly 1;
  mixed      the three materials at random;
  centre     an axis-aligned camera without a lens at the centre of a glass sphere, every primary ray exactly (0, 0, -1), with metal,
             glass and Lambertian spheres on the axes: normal incidence, components of d and n that are +0 and -0.

each in a `small` size (the small-scene kernels) and a `big` one (fillers of the scene's own material past 1023 spheres).  Every build of
r1_builds.h is reached: the tree, the sweep and the grid through the synchronous frame with its records (LAT; big: TP), r1_render_async
(TP), PIXEL mode, a batch (BATCH), a camera path (PATH), progressive passes (PASS) and the adaptive call (LISTED); the reference form and
the diagnostic builds through the synchronous frame; and the path-query entry over the frame's own camera rays.  No tolerance anywhere.  The small size's frames and records are also held as fixtures
from the reference's own code at 51 bounces (tests/golden/ref_scatter_*.bin; tests/test_reference_edges_host.py, tests/test_gpu_reference_edges.py)."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import edge_scenes as es
from test_trace_rays_host import assert_records, frame_samples

gpu = pytest.mark.gpu  # (the scenes' own properties are checked on the oracle's frames, without a device)

F = np.float32
W, H, SPP, BOUNCES, STRIDE, SEED = 64, 48, 4, 51, 7, 977
SCENES = ("glass", "metal0", "metal1", "mixed", "centre")
SIZES = ("small", "big")
FAMILIES = {"sweep": binding.VARIANT_PREFILTER, "tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID}
SYNC_ONLY = {"reference": binding.VARIANT_REFERENCE, "sweep_stats": binding.VARIANT_STATS, "tree_stats": binding.VARIANT_BVH_STATS,
             "grid_stats": binding.VARIANT_GRID_STATS}
QUERY = {"default": binding.VARIANT_DEFAULT, "tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID, "reference": binding.VARIANT_REFERENCE}


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------


def _uniform(arr, mat_type, param):
    n = len(arr["center_x"])
    arr["mat_type"] = np.full(n, mat_type, np.uint8)
    arr["mat_param"] = np.broadcast_to(np.asarray(param, F), (n,)).copy()
    return arr


def _field(rng, n=60):
    """a ground sphere and n spheres of radius 0.2 .. 0.7 standing on it, many of them overlapping, some inside others"""
    c = np.zeros((n + 1, 3))
    rad = np.concatenate([[1000.0], rng.uniform(0.2, 0.7, n)])
    c[0] = (0.0, -1000.0, 0.0)
    c[1:, 0], c[1:, 2] = rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 2.0, n)
    c[1:, 1] = rad[1:]
    for k in range(1, n, 4):  # nested: a smaller sphere inside its neighbour
        c[k + 1] = c[k] + rng.uniform(-0.05, 0.05, 3)
        rad[k + 1] = rad[k] * rng.uniform(0.4, 0.7)
    return c, rad


def _camera():
    lookfrom, lookat = np.array([0.0, 1.6, 6.0]), np.array([0.0, 0.5, 0.0])
    return es.look(lookfrom, lookat, 45.0, W / H, 0.05, np.linalg.norm(lookfrom - lookat))


def _scene(name, size):
    rng = np.random.default_rng({"glass": 11, "metal0": 12, "metal1": 13, "mixed": 14, "centre": 15}[name])
    if name == "centre":
        # sphere 0: glass around the camera; on the axes metal at fuzz 0, glass and Lambertian; then a random field further out
        c = [(0, 0, 0), (0, 0, -3), (0, 0, 3), (3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0)]
        c = np.concatenate([np.array(c, np.float64), rng.uniform(-6, 6, (40, 3)) + np.array([0.0, 0.0, -9.0])])
        rad = np.concatenate([np.full(7, 1.0), rng.uniform(0.3, 0.9, 40)])
        arr = es.spheres(c, rad, rng)
        arr["mat_type"][:7] = (2, 1, 2, 1, 0, 2, 1)
        arr["mat_param"][:7] = (1.5, 0.0, 2.4, 0.0, 0.0, 0.5, 1.0)
        cam = np.zeros(22, F)
        cam[3:6] = (0, 0, -1)  # lower_left - origin: the direction of every primary ray (horizontal = vertical = 0, no lens)
        cam[12:15], cam[15:18], cam[18:21] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
        spread, fill = (0.8, 0.8, 0.8), None
    else:
        c, rad = _field(rng)
        arr = es.spheres(c, rad, rng)
        cam, spread = _camera(), (0.8, 0.3, 0.8)
        fill = {"glass": 2, "metal0": 1, "metal1": 1, "mixed": None}[name]
        if name == "glass":
            n = len(rad)
            _uniform(arr, 2, np.where(np.arange(n) % 3 == 2, rng.uniform(0.4, 0.9, n), rng.uniform(1.2, 2.4, n)))
            arr["mat_param"][0] = 1.5
        elif name != "mixed":
            _uniform(arr, 1, 0.0 if name == "metal0" else 1.0)
            for k in ("albedo_r", "albedo_g", "albedo_b"):
                arr[k][:] = rng.uniform(0.7, 0.98, len(rad)).astype(F)
    if size == "big":
        n0 = len(arr["center_x"])
        arr = es.with_fillers(arr, np.asarray(cam, np.float64)[0:3], rng, spread)
        if fill is not None:  # the fillers take the scene's material
            arr["mat_type"][n0:] = fill
            arr["mat_param"][n0:] = arr["mat_param"][1] if fill == 1 else rng.uniform(1.2, 2.4, len(arr["mat_param"]) - n0).astype(F)
    cam = np.asarray(cam, F)
    return r1o.SceneArrays(es.pad8(arr), cam), es.turned(cam, 4.0)


@pytest.fixture(scope="module")
def scenes():
    """(name, size) -> (scene, second camera, the oracle's frames), built on first use and left unchanged: "main" = camera 0 at SEED,
    "batch1" = camera 0 at SEED + STRIDE, "path1" = camera 1 at SEED + STRIDE, each as (image bytes, rays, records (n, 4))"""
    cache = {}

    def oracle(sa, seed):
        img, rays, samples = r1o.render_frame(sa, r1o.make_params(W, H, SPP, seed, max_bounces=BOUNCES), want_samples=True)
        samples = np.ascontiguousarray(samples, F).reshape(-1, 4)
        samples.setflags(write=False)
        return img.tobytes(), int(rays), samples

    def get(name, size):
        if (name, size) not in cache:
            sa, cam2 = _scene(name, size)
            fr = {"main": oracle(sa, SEED), "batch1": oracle(sa, SEED + STRIDE), "path1": oracle(es.with_camera(sa, cam2), SEED + STRIDE)}
            cache[name, size] = (sa, cam2, fr)
        return cache[name, size]

    return get


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def ray_words(samples):
    return np.ascontiguousarray(samples[:, 3]).view(np.uint32)


# ---- what the scenes must show (on the oracle's records: no device involved) -------------------------------------------------------------


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_scene_shows_its_property_in_the_oracles_frame(scenes, name, size):
    sa, cam2, fr = scenes(name, size)
    types = sa.arrays["mat_type"][sa.arrays["inv_radius"] != 0]
    assert len(types) <= 1023 if size == "small" else len(types) > 1023
    rec = fr["main"][2]
    rays = ray_words(rec)
    if name == "glass":
        assert (types == 2).all()
        assert rays.max() == BOUNCES + 1 and (rays >= 20).mean() > 0.02  # paths kept inside glass by total reflection, to the depth limit
        assert (rec[rays <= BOUNCES, :3] > 0).all()                       # attenuation 1 everywhere: what reaches the sky keeps its colour
    elif name.startswith("metal"):
        assert (types == 1).all() and set(np.unique(sa.arrays["mat_param"][sa.arrays["inv_radius"] != 0])) == {F(name[-1])}
        absorbed = (rec[:, :3] == 0).all(1)
        assert (absorbed.mean() > 0.05) if name == "metal1" else (rays.max() >= 6)  # fuzz 1 scatters below the surface: black
    elif name == "mixed":
        assert set(types.tolist()) == {0, 1, 2} and rays.max() >= 10
    else:
        assert (sa.camera_array[6:12] == 0).all() and rays.min() >= 2 and len(np.unique(rays)) >= 6 and rays.max() >= 12


# ---- the frames ----------------------------------------------------------------------------------------------------------------------------


def params(variant, seed, spp=SPP, tile=32):
    return r1.make_params(W, H, spp, seed, max_bounces=BOUNCES, tile_w=tile, tile_h=tile, variant=variant)


def check(got, want, what):
    for f, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], f"{what}, frame {f}: {g[1]} rays, the oracle counts {w[1]}"
        diff = int((np.frombuffer(g[0], np.uint8) != np.frombuffer(w[0], np.uint8)).sum())
        assert diff == 0, f"{what}, frame {f}: {diff} bytes differ from the oracle's frame"


def check_records(got, want, what):
    a, b = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = np.nonzero((a != b).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} records differ from the oracle's, first at {bad[:8]}: {a[bad[:3]]} != {b[bad[:3]]}"


def sync_frame(renderer, variant, fr, what, size):
    img, rays, samples = renderer.render_samples(params(variant, SEED))
    check([(img.tobytes(), rays)], [fr["main"]], what)
    check_records(samples, fr["main"][2], what)
    info = renderer.launch_info()
    assert info["kernel"] == variant, (what, info)
    assert info["spheres_active"] <= 1023 if size == "small" else info["spheres_active"] > 1023, info


@gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_every_call_of_a_family_renders_the_oracles_frame(renderer, scenes, name, size, family):
    sa, cam2, fr = scenes(name, size)
    variant = FAMILIES[family]
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    sync_frame(renderer, variant, fr, "sync", size)
    # r1_render_async into page-locked memory, then the same in PIXEL mode
    for pixel in (False, True):
        hf = binding.HostFrame(W, H)
        try:
            renderer.set_pixel_mode(pixel)
            renderer.render_async(params(variant, SEED), hf)
            renderer.sync()
            check([(hf.image.tobytes(), hf.rays)], [fr["main"]], "pixel" if pixel else "async")
        finally:
            renderer.set_pixel_mode(False)
            hf.close()
    # a batch of two and a path over the two cameras
    hf = binding.HostFrames(W, H, 2)
    try:
        renderer.render_batch_async(params(variant, SEED), 2, hf, seed_stride=STRIDE)
        renderer.sync()
        check([(hf.image(f).tobytes(), hf.rays(f)) for f in range(2)], [fr["main"], fr["batch1"]], "batch")
        renderer.render_path_async(params(variant, SEED), [es.ccamera(sa.camera_array), es.ccamera(cam2)], hf, seed_stride=STRIDE)
        renderer.sync()
        check([(hf.image(f).tobytes(), hf.rays(f)) for f in range(2)], [fr["main"], fr["path1"]], "path")
    finally:
        hf.close()
    # progressive passes 1 + 3, and the adaptive call with its rule off: 2 + 2 samples, the second pass over a tile list
    renderer.render_pass(params(variant, SEED, 1), 0)
    img, rays = renderer.render_pass(params(variant, SEED, SPP - 1), 1)
    check([(img.tobytes(), rays)], [fr["main"]], "pass")
    img, rays, tiles, res = renderer.render_adaptive(params(variant, SEED, SPP, 16), 2, 2, -1, 0)
    assert (tiles["spp"] == SPP).all()
    check([(img.tobytes(), rays)], [fr["main"]], "adaptive")
    assert renderer.launch_info()["kernel"] == variant


@gpu
@pytest.mark.parametrize("build", sorted(SYNC_ONLY))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_reference_form_and_diagnostic_builds_render_the_oracles_synchronous_frame(renderer, scenes, name, size, build):
    sa, cam2, fr = scenes(name, size)
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    sync_frame(renderer, SYNC_ONLY[build], fr, build, size)


@gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_path_queries_return_the_oracles_records(renderer, scenes, name, size):
    """the frame's own camera rays and stream states (r1_camera_rays) through r1_trace_rays: the records of the oracle's frame"""
    sa, cam2, fr = scenes(name, size)
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    x, y, s = frame_samples(W, H, SPP)
    rays, seeds = binding.camera_rays(es.ccamera(sa.camera_array), params(0, SEED), x, y, s)
    rec = fr["main"][2]
    for what, variant in QUERY.items():
        assert_records(renderer.trace_rays(rays, seeds, BOUNCES, variant), rec[:, :3], ray_words(rec), (name, size, what))
