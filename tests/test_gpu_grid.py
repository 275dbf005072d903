"""GPU parity tests of the optional uniform grid (R1_VARIANT_GRID).

The grid only chooses which spheres are given to the reference's per-sphere test (rays whose origin is too far for its pad take the
tree walk instead), and must never lose a sphere the reference would hit: every test requires BIT-IDENTICAL samples, ray counts and
pixels against the exhaustive kernels, the tree, the reference's own fixtures or the CPU oracle."""
import json
import os

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o
from test_gpu_bvh import MAKE, _as_ccamera, _as_cscene, _look, oparams, oracle_scene, pad8, same, spheres

pytestmark = pytest.mark.gpu

GRID, GRID_STATS = binding.VARIANT_GRID, binding.VARIANT_GRID_STATS
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def rays_of(samples):
    return samples[:, 3].copy().view(np.uint32)


def test_grid_variants_really_run_the_grid(renderer):
    """An unknown variant used to run the sweep: 7 and 8 must run the grid kernels, whatever the entry point."""
    w, h, spp = 96, 64, 2
    renderer.set_scene(r1.create_large_scene(w, h))
    want = renderer.render(r1.make_params(w, h, spp, 3, variant=binding.VARIANT_PREFILTER))
    got = renderer.render(r1.make_params(w, h, spp, 3, variant=GRID))
    assert renderer.launch_info()["kernel"] == GRID
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    hf = binding.HostFrames(w, h, 3)
    renderer.render_async(r1.make_params(w, h, spp, 3, variant=GRID), hf)
    renderer.sync()
    assert renderer.launch_info()["kernel"] == GRID and renderer.launch_info()["tiles_in_kernel"] == 0
    assert hf.rays(0) == want[1] and hf.image(0).tobytes() == want[0].tobytes()
    renderer.render_batch_async(r1.make_params(w, h, spp, 3, variant=GRID), 3, hf, seed_stride=0)
    renderer.sync()
    assert renderer.launch_info()["kernel"] == GRID
    assert all(hf.rays(f) == want[1] and hf.image(f).tobytes() == want[0].tobytes() for f in range(3))
    hf.close()
    st = renderer.render(r1.make_params(w, h, spp, 3, variant=GRID_STATS))
    assert renderer.launch_info()["kernel"] == GRID_STATS
    assert st[0].tobytes() == want[0].tobytes() and st[1] == want[1]


@pytest.mark.parametrize("name", ["small", "medium", "large"])
def test_grid_matches_reference_fixture_1200x800x10(renderer, name):
    g = r1o.read_golden(os.path.join(GOLD, f"samples_{name}_1200x800x10.bin"))
    w, h, spp, seed, _ = g["hdr"].tolist()
    renderer.set_scene(MAKE[name](w, h))
    img, rays, samples = renderer.render_samples(r1.make_params(w, h, spp, seed, variant=GRID))
    assert renderer.launch_info()["kernel"] == GRID
    got = samples[(g["y"].astype(np.int64) * w + g["x"]) * spp + g["s"]]
    assert (rays_of(got) == g["rays"]).all()
    assert (got[:, :3].view(np.uint32) == g["rgb"].reshape(-1, 3).view(np.uint32)).all()
    with open(os.path.join(GOLD, "full_1200x800x10.json")) as f:
        full = json.load(f)[name]
    assert abs(rays - full["rays"]) <= max(4, full["rays"] * 1e-5), (rays, full["rays"])
    # and the whole frame equals the exhaustive sweep's, every sample
    ref = renderer.render_samples(r1.make_params(w, h, spp, seed, variant=binding.VARIANT_PREFILTER))
    assert same((img, rays, samples), ref)


def test_grid_second_seed_and_ragged_fixtures(renderer):
    g = r1o.read_golden(os.path.join(GOLD, "samples_large_320x200x64.bin"))
    w, h, spp, seed, _ = g["hdr"].tolist()
    renderer.set_scene(r1.create_large_scene(w, h))
    img, rays, samples = renderer.render_samples(r1.make_params(w, h, spp, seed, variant=GRID))
    got = samples[(g["y"].astype(np.int64) * w + g["x"]) * spp + g["s"]]
    assert (rays_of(got) == g["rays"]).all() and got[:, :3].tobytes() == g["rgb"].tobytes()
    g = r1o.read_golden(os.path.join(GOLD, "frame_medium_77x45x3.bin"))
    w, h, spp, seed = g["hdr"].tolist()
    renderer.set_scene(r1.create_medium_scene(w, h))
    img, rays, _ = renderer.render(r1.make_params(w, h, spp, seed, variant=GRID))
    assert rays == int(g["rays"][0]) and img.tobytes() == g["image"].tobytes()


@pytest.mark.parametrize("n_active", [0, 1, 7, 8, 9, 1023, 1024])
def test_grid_sphere_count_edges(renderer, n_active):
    w, h, spp = 64, 48, 2
    src = r1.create_grid_scene(w, h, 36, 30)
    arr = src.arrays()
    keep = np.nonzero(arr["inv_radius"] != 0)[0][-n_active:] if n_active else np.zeros(0, np.int64)
    sa = r1o.SceneArrays(pad8({k: v[keep] for k, v in arr.items()}), src.camera_array())
    renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
    got = renderer.render_samples(r1.make_params(w, h, spp, 9, variant=GRID))
    assert renderer.launch_info()["kernel"] == GRID
    ref = renderer.render_samples(r1.make_params(w, h, spp, 9, variant=binding.VARIANT_REFERENCE))
    assert same(got, ref)


CASES = ["mixed_radii", "far_camera", "tiny_spheres", "coincident", "noise_dominated", "collinear", "dense_cluster", "nested"]


@pytest.mark.parametrize("case", CASES)
def test_grid_is_exact_on_adversarial_scenes(renderer, case):
    rng = np.random.default_rng(300 + CASES.index(case))
    w, h, spp = 72, 48, 3
    cam = r1.create_small_scene(w, h).camera_array().copy()
    n = 300
    if case == "mixed_radii":
        c, rad = rng.uniform(-12, 12, (n, 3)), np.exp(rng.uniform(np.log(0.02), np.log(6.0), n))
    elif case == "far_camera":
        shift = np.array([700.0, 260.0, 410.0], np.float32)
        c, rad = rng.uniform(-8, 8, (n, 3)) + shift, rng.uniform(0.2, 0.8, n)
        cam[0:3] += shift
        cam[3:6] += shift
    elif case == "tiny_spheres":
        c, rad = rng.uniform(-3, 3, (n, 3)), np.exp(rng.uniform(np.log(1e-3), np.log(0.05), n))
    elif case == "coincident":
        c, rad = np.repeat(rng.uniform(-3, 3, (n // 6, 3)), 6, axis=0), np.repeat(rng.uniform(0.1, 0.6, n // 6), 6)
    elif case == "dense_cluster":
        c, rad = rng.normal(0, 1.2, (n, 3)), rng.uniform(0.05, 0.35, n)
    elif case == "nested":
        centres = rng.uniform(-4, 4, (12, 3))
        c, rad = centres[rng.integers(0, 12, n)], rng.uniform(0.05, 2.5, n)
    elif case == "noise_dominated":
        shift = np.array([-420.0, 380.0, 210.0], np.float32)
        c, rad = rng.uniform(-1.5, 1.5, (n, 3)) + shift, np.full(n, 2e-3)
        c[:40] = rng.uniform(-1.5, 1.5, (40, 3))
        rad[:20] = 0.4
        rad[-1], c[-1] = 300.0, np.array([0.0, -302.0, 0.0])
    else:
        c = np.zeros((n, 3))
        c[:, 0] = rng.uniform(-20, 20, n)
        c[:, 1] = 0.25
        rad = rng.uniform(0.05, 0.3, n)
    sa = r1o.SceneArrays(spheres(c, rad, rng), cam)
    renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
    got = renderer.render_samples(r1.make_params(w, h, spp, 1234, variant=GRID))
    ref = renderer.render_samples(r1.make_params(w, h, spp, 1234, variant=binding.VARIANT_REFERENCE))
    assert same(got, ref)
    oimg, orays, osamples = r1o.render_frame(sa, oparams(r1.make_params(w, h, spp, 1234)), want_samples=True)
    assert got[1] == orays and got[2].tobytes() == osamples.tobytes()


@pytest.mark.parametrize("bounces", [1, 3, 50, 51])
def test_grid_bounce_limits(renderer, bounces):
    w, h, spp = 80, 60, 3
    renderer.set_scene(r1.create_large_scene(w, h))
    got = renderer.render_samples(r1.make_params(w, h, spp, 5, max_bounces=bounces, variant=GRID))
    ref = renderer.render_samples(r1.make_params(w, h, spp, 5, max_bounces=bounces, variant=binding.VARIANT_REFERENCE))
    assert same(got, ref)


def test_grid_shards_and_tiles(renderer):
    w, h, spp = 200, 120, 3
    renderer.set_scene(r1.create_large_scene(w, h))
    base = renderer.render(r1.make_params(w, h, spp, 77, variant=binding.VARIANT_PREFILTER))
    odd = renderer.render(r1.make_params(w, h, spp, 77, tile_w=24, tile_h=40, variant=GRID))
    assert odd[0].tobytes() == base[0].tobytes() and odd[1] == base[1]
    total = sum(renderer.render(r1.make_params(w, h, spp, 77, shard=s, num_shards=3, variant=GRID))[1] for s in range(3))
    assert total == base[1]


def test_grid_big_scenes(renderer):
    """Config 5's scene (100 004 spheres, the big-scene grid kernel): a crop equals the LDS-tiled sweep, and a frame of the
    1920 x 1080 camera equals the tree."""
    w, h, spp = 160, 90, 2
    renderer.set_scene(r1.create_grid_scene(w, h, 400, 250))
    a = renderer.render_samples(r1.make_params(w, h, spp, 5, variant=binding.VARIANT_PREFILTER))
    b = renderer.render_samples(r1.make_params(w, h, spp, 5, variant=GRID))
    assert renderer.launch_info()["kernel"] == GRID
    assert same(a, b)
    sc = r1.create_grid_scene(1920, 1080, 400, 250)
    sa = oracle_scene(sc)
    renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
    w, h, spp = 240, 135, 2  # (the 1920 x 1080 camera's aspect)
    a = renderer.render_samples(r1.make_params(w, h, spp, 8, variant=binding.VARIANT_BVH))
    b = renderer.render_samples(r1.make_params(w, h, spp, 8, variant=GRID))
    assert same(a, b)


def test_grid_entry_points_equal_r1_render(renderer):
    torch = pytest.importorskip("torch")
    w, h, spp = 150, 90, 3
    renderer.set_scene(r1.create_large_scene(w, h))
    want = [renderer.render(r1.make_params(w, h, spp, 60 + f, variant=GRID))[:2] for f in range(6)]
    # six contexts in flight
    rs = [r1.Renderer(0) for _ in range(6)]
    hfs = [binding.HostFrames(w, h, 1) for _ in range(6)]
    for k in range(6):
        rs[k].set_scene(r1.create_large_scene(w, h))
    for k in range(6):
        rs[k].render_async(r1.make_params(w, h, spp, 60 + k, variant=GRID), hfs[k])
    for k in range(6):
        rs[k].sync()
        assert hfs[k].rays(0) == want[k][1] and hfs[k].image(0).tobytes() == want[k][0].tobytes(), k
        hfs[k].close()
        rs[k].close()
    # a batch with seed stride 1
    hf = binding.HostFrames(w, h, 4)
    renderer.render_batch_async(r1.make_params(w, h, spp, 60, variant=GRID), 4, hf, seed_stride=1)
    renderer.sync()
    assert all(hf.rays(f) == want[f][1] and hf.image(f).tobytes() == want[f][0].tobytes() for f in range(4))
    hf.close()
    # the device-resident shard entry point, then PIXEL mode
    p = r1.make_params(w, h, spp, 60, variant=GRID)
    nbytes = binding.shard_block_bytes(p)
    for pixel in (False, True):
        renderer.set_pixel_mode(pixel)
        rec = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        renderer.render_shard_device(p, rec.data_ptr(), rec.data_ptr() + ((nbytes + 7) & ~7), st)
        assert renderer.launch_info()["kernel"] == GRID
        renderer.assemble_device(p, rec.data_ptr(), out.data_ptr(), st)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want[0][0].tobytes(), pixel
        assert int(rec[(nbytes + 7) & ~7:((nbytes + 7) & ~7) + 8].view(torch.int64).item()) == want[0][1], pixel
    renderer.set_pixel_mode(False)


def test_grid_stats_build(renderer):
    w, h, spp = 120, 80, 4
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    a = renderer.render(r1.make_params(w, h, spp, 21, variant=GRID))
    b = renderer.render(r1.make_params(w, h, spp, 21, variant=GRID_STATS))
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    raw = renderer.last_stats()["raw"]
    assert raw[5] > 0 and raw[9] > 0 and raw[2] > 0   # sphere tests, cell steps, wave trips of the walk
    # every hit test of the walk tests the four outliers; the synchronous frame's tail (a wave with <= 2 live paths once the queue is
    # empty) goes through cooperative_sweep instead, a few per cent of the rays
    assert raw[15] % 4 == 0 and 0.9 * 4 * b[1] <= raw[15] <= 4 * b[1]
    # the fallback count against r1_grid_visit's prediction: a pinhole camera whose every ray misses the scene (looking away),
    # once from far out (every ray takes the fallback) and once from near the lattice (none does)
    sa = oracle_scene(sc)
    cs = _as_cscene(sa)
    for origin, fb_want in (((300.0, 40.0, 300.0), True), ((3.0, 8.0, 15.0), False)):
        cam = _look(origin, (origin[0] + 10, origin[1] + 20, origin[2] + 10), 20, w / h, 0.0, 10.0)
        o = cam[0:3]
        for k in range(3):  # (the pinhole's rays share the origin: the prediction is the same for all of them)
            dd = cam[3:6] + (0.2 + 0.3 * k) * cam[6:9] + (0.3 + 0.2 * k) * cam[9:12] - o
            _, hit, _, fb = binding.grid_visit(cs, o, (dd / np.linalg.norm(dd)).astype(np.float32))
            assert fb == fb_want and hit == -1
        s2 = r1o.SceneArrays(sa.arrays, cam)
        renderer.set_scene_raw(_as_cscene(s2), _as_ccamera(s2))
        img, rays, _ = renderer.render(r1.make_params(w, h, spp, 21, variant=GRID_STATS))
        assert rays == w * h * spp  # (every path ends at the sky)
        fallbacks = renderer.last_stats()["raw"][14]
        if fb_want:  # (all primary rays, but the few of the frame's tail that cooperative_sweep tests)
            assert 0.9 * w * h * spp <= fallbacks <= w * h * spp
        else:
            assert fallbacks == 0
