"""GPU tests of the flat walk of the box-tree kernels (r1_hit_tree.hpp bvh_advance: visit_flat).

The large scene's tree is flat along y (r1_bvh_info.flat_axis == 1): the small-scene tree kernels test ONE y slab once per call of the
walk and two axes per child box.  That changes which boxes a ray passes, never what it hits: through every entry point — r1_render,
r1_render_async, a batch, progressive passes, a camera path, PIXEL mode — the frame is, bit for bit and ray for ray, what the grouped
exhaustive sweep renders (R1_VARIANT_PREFILTER: no tree at all) and what the reference's fixtures under tests/golden hold; the same
with cameras inside the slab that look along it (walks that live on N and F).  The medium scene's tree is not flat and walks as
before.  Nothing here has a tolerance."""
import os

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding, sharding
import r1o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TREE, SWEEP = binding.VARIANT_DEFAULT, binding.VARIANT_PREFILTER


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def params(w, h, spp, seed, variant=TREE):
    return r1.make_params(w, h, spp, seed, variant=variant)


def every_entry_point(rend, w, h, spp, seed, cam, variant=TREE):
    """{entry point: (image bytes, rays)} of one frame with camera `cam` (a CCamera) — and the per-sample records of r1_render_samples."""
    torch = pytest.importorskip("torch")
    p = params(w, h, spp, seed, variant)
    out = {}
    rend.set_camera(cam)
    img, rays, _ = rend.render(p)
    out["render"] = (img.tobytes(), rays)
    assert rend.launch_info()["kernel"] == (binding.VARIANT_BVH if variant == TREE else variant)
    img, rays, samples = rend.render_samples(p)
    out["render_samples"] = (img.tobytes(), rays)
    hf = binding.HostFrames(w, h, 3)
    try:
        rend.render_async(p, hf)
        rend.sync()
        out["async"] = (hf.image(0).tobytes(), hf.rays(0))
        rend.render_batch_async(p, 3, hf, seed_stride=0)
        rend.sync()
        if variant == TREE:
            assert rend.launch_info()["tiles_in_kernel"] == 1
        for f in range(3):
            out[f"batch[{f}]"] = (hf.image(f).tobytes(), hf.rays(f))
        rend.render_path_async(p, [cam] * 3, hf, seed_stride=0)
        rend.sync()
        for f in range(3):
            out[f"path[{f}]"] = (hf.image(f).tobytes(), hf.rays(f))
    finally:
        hf.close()
    # progressive passes: spp samples in two passes (the MODE 4 kernels)
    first = spp // 2
    assert 1 <= first < spp
    rend.render_pass(params(w, h, first, seed, variant), 0)
    img, rays = rend.render_pass(params(w, h, spp - first, seed, variant), first)
    out["passes"] = (img.tobytes(), rays)
    # the throughput entry point, per-sample records and PIXEL mode (lanes own pixels)
    nbytes = binding.shard_block_bytes(p)
    st = torch.cuda.current_stream().cuda_stream
    for pixel in (False, True):
        rec = torch.zeros(nbytes + sharding.RECORD_TRAILER, dtype=torch.uint8, device="cuda")
        dev = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        rend.set_pixel_mode(pixel)
        try:
            rend.render_shard_device(p, rec.data_ptr(), rec.data_ptr() + nbytes, st)
            rend.assemble_device_strided(p, rec.data_ptr(), nbytes + sharding.RECORD_TRAILER, dev.data_ptr(), st)
            torch.cuda.synchronize()
        finally:
            rend.set_pixel_mode(False)
        out["pixel_mode" if pixel else "shard_device"] = (dev.cpu().numpy().tobytes(), sharding.total_rays(rec, 1))
    return out, samples


def slab_cameras(sc, w, h):
    """Cameras inside the tree's y slab that look along it: the centre ray has d.y = 0 exactly, the others leave the slab at shallow
    angles or never.  One in the layer only the union covers (above the boxes of the spheres that are not raised), one low between the
    spheres, one outside the lattice looking in along the plane."""
    info, _, _ = binding.bvh_describe(sc.spheres.contents)
    assert info["flat_axis"] == 1, info
    lo, hi = float(info["flat_m"]) - float(info["flat_e"]), float(info["flat_m"]) + float(info["flat_e"])
    aspect = np.float32(w) / np.float32(h)
    cams = []
    for frm, to, fov, aperture in (((0.53, 0.5, 0.47), (9.0, 0.5, 5.0), 50.0, 0.0), ((-3.5, 0.2, 2.5), (6.0, 0.2, -4.0), 35.0, 0.05),
                                   ((-19.0, 0.05, 0.3), (0.0, 0.05, 0.0), 25.0, 0.0)):
        assert lo < frm[1] < hi and frm[1] == to[1]
        cams.append(r1.camera_look_at(frm, to, (0, 1, 0), fov, aspect, aperture, 5.0))
    return cams


def test_large_scene_every_entry_point_equals_the_sweep(renderer):
    w, h, spp, seed = 200, 100, 4, 10001
    sc = r1.create_large_scene(w, h)
    assert binding.bvh_describe(sc.spheres.contents)[0]["flat_axis"] == 1
    renderer.set_scene(sc)
    for name, cam in [("own", sc.camera.contents)] + [(f"slab{i}", c) for i, c in enumerate(slab_cameras(sc, w, h))]:
        renderer.set_camera(cam)
        want_img, want_rays, want_samples = renderer.render_samples(params(w, h, spp, seed, SWEEP))
        assert renderer.launch_info()["kernel"] == SWEEP
        got, samples = every_entry_point(renderer, w, h, spp, seed, cam)
        for entry, (img, rays) in got.items():
            assert rays == want_rays, (name, entry, rays, want_rays)
            assert img == want_img.tobytes(), (name, entry)
        assert samples.tobytes() == want_samples.tobytes(), name  # radiance and ray count of every sample
        if name != "own":
            assert want_rays > w * h * spp  # the camera does see the scene: rays bounce
    renderer.set_camera(sc.camera.contents)


def test_large_scene_slab_cameras_equal_the_oracle(renderer):
    w, h, spp, seed = 80, 60, 4, 10001
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    for i, cam in enumerate(slab_cameras(sc, w, h)):
        renderer.set_camera(cam)
        oimg, orays, osamples = r1o.render_frame(r1o.SceneArrays(sc.arrays(), r1.camera_to_array(cam)), r1o.make_params(w, h, spp, seed), want_samples=True)
        img, rays, samples = renderer.render_samples(params(w, h, spp, seed))
        assert renderer.launch_info()["kernel"] == binding.VARIANT_BVH
        assert rays == orays and img.tobytes() == oimg.tobytes() and samples.tobytes() == osamples.tobytes(), i
    renderer.set_camera(sc.camera.contents)


def test_large_scene_golden_frame_200x100x4(renderer):
    g = r1o.read_golden(os.path.join(GOLD, "frame_large_200x100x4.bin"))
    w, h, spp, seed = g["hdr"].tolist()
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    got, _ = every_entry_point(renderer, w, h, spp, seed, sc.camera.contents)
    for entry, (img, rays) in got.items():
        assert rays == int(g["rays"][0]), entry
        assert img == g["image"].tobytes(), entry


@pytest.mark.parametrize("fixture", ["samples_large_1200x800x10.bin", "samples_large_320x200x64.bin"])
def test_large_scene_golden_sample_records(renderer, fixture):
    """The reference's own per-sample records at the benchmark's shape (and at 64 spp with another seed), and the whole frame against the
    sweep: pixels, ray count, every sample record."""
    g = r1o.read_golden(os.path.join(GOLD, fixture))
    w, h, spp, seed, _ = g["hdr"].tolist()
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    img, rays, samples = renderer.render_samples(params(w, h, spp, seed))
    info = renderer.launch_info()
    assert info["kernel"] == binding.VARIANT_BVH
    got = samples[(g["y"].astype(np.int64) * w + g["x"]) * spp + g["s"]]
    assert (got[:, 3].copy().view(np.uint32) == g["rays"]).all()
    assert got[:, :3].tobytes() == g["rgb"].tobytes()
    simg, srays, ssamples = renderer.render_samples(params(w, h, spp, seed, SWEEP))
    assert rays == srays and img.tobytes() == simg.tobytes() and samples.tobytes() == ssamples.tobytes()
    # the frames that land on the host from the throughput kernels (bench.py's shape: tiles summed inside the kernel)
    hf = binding.HostFrames(w, h, 2)
    try:
        renderer.render_async(params(w, h, spp, seed), hf)
        renderer.sync()
        assert hf.rays(0) == srays and hf.image(0).tobytes() == simg.tobytes()
        renderer.render_batch_async(params(w, h, spp, seed), 2, hf, seed_stride=0)
        renderer.sync()
        assert renderer.launch_info()["tiles_in_kernel"] == 1
        assert hf.rays(1) == srays and hf.image(1).tobytes() == simg.tobytes()
    finally:
        hf.close()


def test_medium_scene_is_not_flat_and_equals_the_sweep(renderer):
    w, h, spp, seed = 200, 100, 4, 10001
    sc = r1.create_medium_scene(w, h)
    assert binding.bvh_describe(sc.spheres.contents)[0]["flat_axis"] == -1
    renderer.set_scene(sc)
    want_img, want_rays, want_samples = renderer.render_samples(params(w, h, spp, seed, SWEEP))
    got, samples = every_entry_point(renderer, w, h, spp, seed, sc.camera.contents)
    for entry, (img, rays) in got.items():
        assert rays == want_rays and img == want_img.tobytes(), entry
    assert samples.tobytes() == want_samples.tobytes()
    g = r1o.read_golden(os.path.join(GOLD, "frame_medium_200x100x4.bin"))
    assert want_rays == int(g["rays"][0]) and want_img.tobytes() == g["image"].tobytes()


def test_bvh_stats_build_walks_the_same_way(renderer):
    """R1_VARIANT_BVH_STATS counts the walk of the timed kernel: same pixels, and on the flat tree no more node visits than boxes exist
    to pass (a smoke check of the counters' plumbing: the figures themselves are in profiles/)."""
    w, h, spp, seed = 120, 80, 5, 10001
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    want = renderer.render(params(w, h, spp, seed))
    got = renderer.render(params(w, h, spp, seed, binding.VARIANT_BVH_STATS))
    assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes()
    steps = renderer.last_stats()["root_steps"]
    assert 0 < steps <= want[1]  # one per ray that walked
