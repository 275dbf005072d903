"""GPU test of the trace kernel's build families (rays1bench_amd/csrc/r1_builds.h): every mode a public call can ask for — the synchronous
frame (LAT; TP on a big scene), r1_render_async (TP), the same in PIXEL mode, a batch (BATCH), a camera path (PATH) and a progressive pass
from sample 0 (PASS) — through the grouped sweep, the box tree and the uniform grid, on a small scene and on one just over the small-scene
kernels' 1023 spheres; the reference form and the diagnostic builds through the synchronous frame.  All product variants produce the same
pixels, and a pass from sample 0 is that frame: every image and ray count must equal, byte for byte, the reference-form kernel's
synchronous frame with the same params (frame f of a batch or path: seed + f * seed_stride).  Nothing here has a tolerance.  (Adaptive
sampling — the LISTED builds — has tests/test_gpu_adaptive.py.)"""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

pytestmark = pytest.mark.gpu

W, H, SPP, SEED, STRIDE = 64, 48, 2, 4321, 7  # 2 x 2 tiles of 32 x 32: more than one tile, and the upper row is an edge row (48 = 32 + 16)
FAMILIES = {"sweep": binding.VARIANT_PREFILTER, "tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID}
SYNC_ONLY = {"reference": binding.VARIANT_REFERENCE, "sweep_stats": binding.VARIANT_STATS, "tree_stats": binding.VARIANT_BVH_STATS,
             "grid_stats": binding.VARIANT_GRID_STATS}
CALLS = ("sync", "async", "pixel", "batch", "path", "pass")
BATCH_RULE = "frame batches run through the throughput kernels only"
PASS_RULE = "has no progressive-pass build"


def make_scene(size):
    # big: 1092 hittable spheres, just over R1_MAX_ACTIVE_10BIT = 1023: the big-scene kernels of every family
    sc = r1.create_small_scene(W, H) if size == "small" else r1.create_grid_scene(W, H, 34, 32)
    active = int((sc.arrays()["inv_radius"] != 0).sum())
    assert active <= 1023 if size == "small" else 1023 < active < 1200, active
    return sc


def params(variant, seed=SEED):
    return r1.make_params(W, H, SPP, seed, tile_w=32, tile_h=32, variant=variant)


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    out = {size: make_scene(size) for size in ("small", "big")}
    yield out
    for sc in out.values():
        sc.close()


@pytest.fixture(scope="module")
def expected(renderer, scenes):
    """size -> [(image bytes, rays) of frame f = 0, 1]: the reference-form kernel's synchronous frame with seed SEED + f * STRIDE."""
    out = {}
    for size, sc in scenes.items():
        renderer.set_scene(sc)
        frames = []
        for f in range(2):
            img, rays, _ = renderer.render(params(binding.VARIANT_REFERENCE, SEED + f * STRIDE))
            assert rays > W * H * SPP  # (some path bounced: the frame is not the background alone)
            frames.append((img.tobytes(), rays))
        assert frames[0] != frames[1]  # the second seed gives another frame: a batch that rendered frame 0 twice would show
        out[size] = frames
    return out


def run(renderer, sc, call, variant):
    """The frames of `call` as [(image bytes, rays)]."""
    p = params(variant)
    if call == "sync":
        img, rays, _ = renderer.render(p)
        return [(img.tobytes(), rays)]
    if call == "pass":
        img, rays = renderer.render_pass(p, 0)
        return [(img.tobytes(), rays)]
    if call in ("async", "pixel"):
        hf = binding.HostFrame(W, H)
        try:
            renderer.set_pixel_mode(call == "pixel")
            renderer.render_async(p, hf)
            renderer.sync()
            return [(hf.image.tobytes(), hf.rays)]
        finally:
            renderer.set_pixel_mode(False)
            hf.close()
    hf = binding.HostFrames(W, H, 2)
    try:
        if call == "batch":
            renderer.render_batch_async(p, 2, hf, seed_stride=STRIDE)
        else:
            renderer.render_path_async(p, [sc.camera.contents, sc.camera.contents], hf, seed_stride=STRIDE)
        renderer.sync()
        return [(hf.image(f).tobytes(), hf.rays(f)) for f in range(2)]
    finally:
        hf.close()


def check(renderer, got, want, variant):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], f"frame {f}: {g[1]} rays, the reference form counts {w[1]}"
        diff = int((np.frombuffer(g[0], np.uint8) != np.frombuffer(w[0], np.uint8)).sum())
        assert diff == 0, f"frame {f}: {diff} bytes differ from the reference form's frame"
    assert renderer.launch_info()["kernel"] == variant


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("size", ["small", "big"])
def test_every_call_of_a_family_renders_the_reference_forms_frame(renderer, scenes, expected, size, family, call):
    renderer.set_scene(scenes[size])
    got = run(renderer, scenes[size], call, FAMILIES[family])
    check(renderer, got, expected[size][:len(got)], FAMILIES[family])


@pytest.mark.parametrize("name", sorted(SYNC_ONLY))
@pytest.mark.parametrize("size", ["small", "big"])
def test_reference_form_and_diagnostic_builds_render_the_same_synchronous_frame(renderer, scenes, expected, size, name):
    renderer.set_scene(scenes[size])
    check(renderer, run(renderer, scenes[size], "sync", SYNC_ONLY[name]), expected[size][:1], SYNC_ONLY[name])


@pytest.mark.parametrize("size", ["small", "big"])
def test_variants_without_a_batch_or_pass_build_are_refused(renderer, scenes, expected, size):
    """Batches and paths: the reference form, the diagnostic builds and the wavefront variant have none.  Passes: the diagnostic builds and
    the wavefront variant have none; the reference form has (r1_pass_kernel<1, big>), and its pass from sample 0 is its frame."""
    sc = scenes[size]
    renderer.set_scene(sc)

    def refused(fn, rule):
        with pytest.raises(binding.R1Error) as e:
            fn()
        assert e.value.code == binding.R1_EINVAL, e.value
        assert rule in str(e.value), e.value

    hf = binding.HostFrames(W, H, 2)
    try:
        for variant in (binding.VARIANT_REFERENCE, binding.VARIANT_STATS, binding.VARIANT_BVH_STATS, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID_STATS):
            p = params(variant)
            refused(lambda: renderer.render_batch_async(p, 2, hf, seed_stride=STRIDE), BATCH_RULE)
            refused(lambda: renderer.render_path_async(p, [sc.camera.contents, sc.camera.contents], hf, seed_stride=STRIDE), BATCH_RULE)
            if variant != binding.VARIANT_REFERENCE:
                refused(lambda: renderer.render_pass(p, 0), PASS_RULE)
    finally:
        hf.close()
    check(renderer, run(renderer, sc, "pass", binding.VARIANT_REFERENCE), expected[size][:1], binding.VARIANT_REFERENCE)
