"""GPU test of every trace build (rays1bench_amd/csrc/r1_builds.h) over the scenes of tests/edge_scenes.py — deep paths whose attenuation
stacks overflow into the global workspace, materials at the edges of their parameters and bytes that wrap, coincident spheres, hits by
rounding alone, a camera inside a sphere, axis-parallel rays, a cluster 8e4 units out — in a small and a big size each.  (Which kernels a
size reaches: the sweep and the reference form go by the sphere count alone; the grid's PIXEL mode always runs its big-scene kernel; a
tree that measures its pad per node runs through the big-scene tree kernels at any size, which of the small sizes only `noise` does —
launch_info does not show it, tests/test_edge_scenes_host.py pins it, and `noise_lds` is the noise scene that stays with the small ones.)  The matrix and the
`run` helper are those of tests/test_gpu_builds.py: the synchronous frame (with its records), r1_render_async into page-locked memory (the
tree's tiles land in the kernel), the same in PIXEL mode, a batch of two, a path over the scene's two cameras, progressive passes 1 + the
rest, and the adaptive call with the rule off and with thresholds under which tiles stop at different counts — through the grouped
sweep, the box tree and the uniform grid; the reference form, the wavefront variant and the diagnostic builds through the synchronous
frame.

The expectation is the CPU ORACLE's frame, records and ray count for that seed and camera (tests/test_edge_scenes_host.py asserts that
these frames show each scene's property), byte for byte; for the adaptive call the restated rule (tests/adaptive_rule.py) on the oracle's
records.  Nothing here has a tolerance and no GPU render is an expectation.  (The one documented deviation, pow5 against glibc's
powf(x, 5), could flip a dielectric branch of a sample; it has not been observed on these frames.)"""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import adaptive_rule as rule
import edge_scenes as es

pytestmark = pytest.mark.gpu

W, H, SPP, STRIDE = es.W, es.H, es.SPP, es.STRIDE  # 64 x 48: 2 x 2 tiles of 32 x 32, the upper row an edge row
FAMILIES = {"sweep": binding.VARIANT_PREFILTER, "tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID}
SYNC_ONLY = {"reference": binding.VARIANT_REFERENCE, "wavefront": binding.VARIANT_WAVEFRONT, "sweep_stats": binding.VARIANT_STATS,
             "tree_stats": binding.VARIANT_BVH_STATS, "grid_stats": binding.VARIANT_GRID_STATS}
CALLS = ("sync", "async", "pixel", "batch", "path", "pass", "adaptive_off", "adaptive")


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def expected():
    """(name, size) -> {"frames": [(image bytes, rays) of frame 0 and of frame 1 of a batch], "path1": frame 1 of the path, "records": the
    records of frame 0 as bytes, "full": (image bytes, rays) at the adaptive cap, "main": the oracle's records at the cap}, filled on
    first use and left unchanged."""
    cache = {}

    def get(name, size):
        if (name, size) not in cache:
            fr = es.frames(name, size)
            main = fr["main"][0]
            img0, rays0 = es.prefix_frame(main, SPP)
            one = lambda key: (fr[key][1].tobytes(), int(es.ray_words(fr[key][0]).sum()))
            cache[name, size] = {"frames": [(img0.tobytes(), rays0), one("batch1")], "path1": one("path1"),
                                 "records": np.ascontiguousarray(main[:, :, :SPP]).tobytes(), "full": one("main"), "main": main}
        return cache[name, size]

    return get


def set_scene(renderer, name, size):
    sa, cam2 = es.build(name, size)
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    return sa, cam2


def params(variant, seed, spp=SPP, tile=32):
    return r1.make_params(W, H, spp, seed, tile_w=tile, tile_h=tile, variant=variant)


def run(renderer, sa, cam2, call, variant, seed):
    """The frames of `call` as [(image bytes, rays)]; the synchronous frame's records as a third entry."""
    p = params(variant, seed)
    if call == "sync":
        img, rays, samples = renderer.render_samples(p)
        return [(img.tobytes(), rays, samples.tobytes())]
    if call == "pass":
        renderer.render_pass(params(variant, seed, 1), 0)
        img, rays = renderer.render_pass(params(variant, seed, SPP - 1), 1)
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
            renderer.render_path_async(p, [es.ccamera(sa.camera_array), es.ccamera(cam2)], hf, seed_stride=STRIDE)
        renderer.sync()
        return [(hf.image(f).tobytes(), hf.rays(f)) for f in range(2)]
    finally:
        hf.close()


def check(renderer, got, want, variant, size):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        print(f"frame {f}: {g[1]} rays, the oracle counts {w[1]}")
        assert g[1] == w[1], f"frame {f}: {g[1]} rays, the oracle counts {w[1]}"
        diff = int((np.frombuffer(g[0], np.uint8) != np.frombuffer(w[0], np.uint8)).sum())
        assert diff == 0, f"frame {f}: {diff} bytes differ from the oracle's frame"
    info = renderer.launch_info()
    assert info["kernel"] == variant
    assert info["spheres_active"] <= 1023 if size == "small" else info["spheres_active"] > 1023, info


def check_records(got, want):
    a, b = np.frombuffer(got, np.uint32).reshape(-1, 4), np.frombuffer(want, np.uint32).reshape(-1, 4)
    bad = np.nonzero((a != b).any(1))[0]
    assert bad.size == 0, f"{bad.size} records differ from the oracle's, first at {bad[:8]}: {a[bad[:3]]} != {b[bad[:3]]}"


def adaptive(renderer, variant, name, exp, rule_on):
    """The adaptive call over 16 x 16 tiles.  Rule off (max_delta -1): the full frame at the cap.  Rule on: reports and ray count are the
    restated rule's on the oracle's records, every tile's pixels the oracle's prefix frame at the tile's count."""
    p = params(variant, es.SEED[name], es.CAP, es.ADAPT_TILE)
    max_delta, mean_q8 = es.RULE if rule_on else (-1, 0)
    img, rays, tiles, res = renderer.render_adaptive(p, es.MIN_SPP, es.PASS_SPP, max_delta, mean_q8)
    want_tiles, want_rays = rule.restate(exp["main"], es.MIN_SPP, es.PASS_SPP, max_delta, mean_q8, es.ADAPT_TILE, es.ADAPT_TILE)
    print("map", rule.histogram(tiles), "the rule's", rule.histogram(want_tiles), "rays", rays, want_rays)
    for f in ("spp", "settled", "err_max", "err_sum"):
        assert np.array_equal(tiles[f], want_tiles[f]), (f, tiles[f], want_tiles[f])
    assert rays == want_rays
    boxes = rule.tile_boxes(W, H, es.ADAPT_TILE, es.ADAPT_TILE)
    assert len(tiles) == len(boxes) == res["tiles"] == 12
    for n in sorted(set(int(x) for x in tiles["spp"])):
        want = es.prefix_frame(exp["main"], n)[0]
        for t, (x0, y0, x1, y1) in enumerate(boxes):
            if int(tiles[t]["spp"]) == n:
                assert img[y0:y1, x0:x1].tobytes() == want[y0:y1, x0:x1].tobytes(), (n, t)
    assert res["samples"] == rule.samples_of(tiles, W, H, es.ADAPT_TILE, es.ADAPT_TILE)
    assert res["tiles_settled"] == int((tiles["settled"] != 0).sum())
    if rule_on:
        assert len(set(int(x) for x in tiles["spp"])) >= 2 and int(tiles["spp"].min()) < es.CAP
    else:
        assert (tiles["spp"] == es.CAP).all() and (img.tobytes(), rays) == exp["full"]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("size", es.SIZES)
@pytest.mark.parametrize("name", es.SCENES)
def test_every_call_of_a_family_renders_the_oracles_frame(renderer, expected, name, size, family, call):
    exp = expected(name, size)
    sa, cam2 = set_scene(renderer, name, size)
    variant = FAMILIES[family]
    if call.startswith("adaptive"):
        adaptive(renderer, variant, name, exp, call == "adaptive")
        assert renderer.launch_info()["kernel"] == variant
        return
    got = run(renderer, sa, cam2, call, variant, es.SEED[name])
    want = exp["frames"][:len(got)] if call != "path" else [exp["frames"][0], exp["path1"]]
    check(renderer, got, want, variant, size)
    if call == "sync":
        check_records(got[0][2], exp["records"])
    if call == "async" and family == "tree":
        assert renderer.launch_info()["tiles_in_kernel"] == 1


@pytest.mark.parametrize("build", sorted(SYNC_ONLY))
@pytest.mark.parametrize("size", es.SIZES)
@pytest.mark.parametrize("name", es.SCENES)
def test_reference_form_wavefront_and_diagnostic_builds_render_the_oracles_synchronous_frame(renderer, expected, name, size, build):
    exp = expected(name, size)
    sa, cam2 = set_scene(renderer, name, size)
    got = run(renderer, sa, cam2, "sync", SYNC_ONLY[build], es.SEED[name])
    check(renderer, got, exp["frames"][:1], SYNC_ONLY[build], size)
    check_records(got[0][2], exp["records"])
