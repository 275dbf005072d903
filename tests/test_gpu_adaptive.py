"""GPU tests of adaptive sampling (r1_render_adaptive).  A sample's streams depend on (seed, pixel, sample index) only and
a pixel's sum is taken in sample order, so a tile that stops after n samples holds the pixels of r1_render at spp = n, the ray count is
the sum over exactly the samples traced, and the tiles' reports are what the rule gives on the per-sample records — tests/adaptive_rule.py
restates it in numpy (pinned against the oracle's records in tests/test_adaptive_host.py).  Every comparison is BIT FOR BIT."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import adaptive_rule as rule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VARIANT_KERNEL = {binding.VARIANT_DEFAULT: binding.VARIANT_BVH, binding.VARIANT_PREFILTER: binding.VARIANT_PREFILTER,
                  binding.VARIANT_GRID: binding.VARIANT_GRID}


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def with_spp(p, spp):
    return r1.make_params(p.width, p.height, spp, p.seed, p.max_bounces, p.tile_w, p.tile_h, variant=p.variant)


def expect_refusal(fn, rule_text, code=binding.R1_EINVAL):
    """The call fails with `code`, and r1_last_error names `rule_text`: the refusal comes from that check, not from another one."""
    with pytest.raises(binding.R1Error) as e:
        fn()
    assert e.value.code == code, e.value
    assert rule_text in str(e.value), e.value


def check_pixels_and_result(renderer, p, min_spp, pass_spp, img, tiles, res):
    """Contract 1 (every tile's pixels are r1_render's at the tile's count) and the result block against the map."""
    boxes = rule.tile_boxes(p.width, p.height, p.tile_w, p.tile_h)
    assert len(tiles) == len(boxes) == res["tiles"]
    for n in sorted(set(int(x) for x in tiles["spp"])):
        want = renderer.render(with_spp(p, n))[0]
        for t, (x0, y0, x1, y1) in enumerate(boxes):
            if int(tiles[t]["spp"]) == n:
                assert img[y0:y1, x0:x1].tobytes() == want[y0:y1, x0:x1].tobytes(), (n, t)
    assert res["samples"] == rule.samples_of(tiles, p.width, p.height, p.tile_w, p.tile_h)
    assert res["tiles_settled"] == int((tiles["settled"] != 0).sum())
    sched = rule.schedule(p.spp, min_spp, pass_spp)
    assert res["passes"] == sched.index(int(tiles["spp"].max())) + 1


def check_contract(renderer, p, min_spp, pass_spp, max_delta, mean_q8, rec=None):
    """Renders adaptively and checks the three contracts against r1_render_samples (the records) and r1_render (the pixels) of the same
    params.  Returns (image, rays, tiles, result)."""
    img, rays, tiles, res = renderer.render_adaptive(p, min_spp, pass_spp, max_delta, mean_q8)
    if rec is None:
        rec = renderer.render_samples(p)[2].reshape(p.height, p.width, p.spp, 4)
    want_tiles, want_rays = rule.restate(rec, min_spp, pass_spp, max_delta, mean_q8, p.tile_w, p.tile_h)
    for f in ("spp", "settled", "err_max", "err_sum"):
        assert np.array_equal(tiles[f], want_tiles[f]), (f, tiles[f], want_tiles[f])
    assert rays == want_rays
    check_pixels_and_result(renderer, p, min_spp, pass_spp, img, tiles, res)
    return img, rays, tiles, res


def test_rule_off_is_the_full_render_large_1200x800x10(renderer):
    """max_delta -1 can never hold: passes of 3, 4 and 3 samples over every tile give r1_render at 10 spp (and the reference's count)."""
    with open(os.path.join(GOLD, "full_1200x800x10.json")) as f:
        full = json.load(f)["large"]
    w, h, seed = full["w"], full["h"], full["seed"]
    renderer.set_scene(r1.create_large_scene(w, h))
    p = r1.make_params(w, h, 10, seed)
    img, rays, tiles, res = renderer.render_adaptive(p, 3, 4, -1, 65280)
    assert renderer.launch_info()["kernel"] == binding.VARIANT_BVH and renderer.launch_info()["tiles_in_kernel"] == 0
    want_img, want_rays, _ = renderer.render(p)
    assert rays == want_rays and img.tobytes() == want_img.tobytes()
    assert (tiles["spp"] == 10).all() and (tiles["settled"] == 0).all()
    assert res == {"samples": w * h * 10, "passes": 3, "tiles": len(tiles), "tiles_settled": 0}
    assert abs(rays - full["rays"]) <= max(4, full["rays"] * 1e-5), (rays, full["rays"])


def test_rule_off_and_rule_always_true_320x200x64(renderer):
    w, h, cap = 320, 200, 64
    renderer.set_scene(r1.create_large_scene(w, h))
    p = r1.make_params(w, h, cap, 10001)
    img, rays, tiles, res = renderer.render_adaptive(p, 8, 8, -1, 0)
    want = renderer.render(p)
    assert rays == want[1] and img.tobytes() == want[0].tobytes()
    assert (tiles["spp"] == cap).all() and (tiles["settled"] == 0).all() and res["passes"] == 8 and res["samples"] == w * h * cap
    # always true: every tile stops at n_0, in one pass
    img, rays, tiles, res = renderer.render_adaptive(p, 8, 8, 255, 65280)
    want = renderer.render(with_spp(p, 8))
    assert rays == want[1] and img.tobytes() == want[0].tobytes()
    assert (tiles["spp"] == 8).all() and (tiles["settled"] == 1).all()
    assert res == {"samples": w * h * 8, "passes": 1, "tiles": 70, "tiles_settled": 70}
    # min_spp beyond the cap: one pass of the cap
    img, rays, tiles, res = renderer.render_adaptive(with_spp(p, 5), 8, 8, 0, 0)
    want = renderer.render(with_spp(p, 5))
    assert rays == want[1] and img.tobytes() == want[0].tobytes() and res["passes"] == 1 and (tiles["spp"] == 5).all()


@pytest.mark.parametrize("max_delta,mean_q8", [(24, 65280), (48, 768)], ids=["24-65280", "48-768"])
def test_the_fixture_frame_stops_tile_by_tile(renderer, max_delta, mean_q8):
    """Large 320 x 200, seed 10001, cap 64, (8, 8): the map is the restated rule's on r1_render_samples' records (which equal the
    reference's by the parity tests), and it is not a degenerate one."""
    w, h, cap = 320, 200, 64
    renderer.set_scene(r1.create_large_scene(w, h))
    p = r1.make_params(w, h, cap, 10001)
    img, rays, tiles, res = check_contract(renderer, p, 8, 8, max_delta, mean_q8)
    assert len(set(int(x) for x in tiles["spp"])) >= 4
    assert (tiles["spp"] == 8).any() and (tiles["settled"] == 0).any()
    assert ((tiles["settled"] == 0) <= (tiles["spp"] == cap)).all()  # (only the cap ends an unsettled tile)
    full = renderer.render(p)[1]
    assert 0 < rays < full and res["samples"] < w * h * cap


def _family_scene(case):
    if case == "big":
        return r1.create_grid_scene(256, 160, 400, 250), 256, 160, 32, 32
    if case == "ragged":
        return r1.create_medium_scene(77, 45), 77, 45, 32, 32
    if case == "ragged16x8":
        return r1.create_medium_scene(77, 45), 77, 45, 16, 8
    w, h = 96, 64
    return {"small": r1.create_small_scene, "medium": r1.create_medium_scene}[case](w, h), w, h, 32, 32


@pytest.mark.parametrize("case", ["small", "medium", "ragged", "ragged16x8", "big"])
def test_every_family(renderer, case):
    """Cap 12, (4, 4), 16 / 65280 through the tree, the grouped sweep and the grid: each against the records and renders of the SAME
    variant, and the three maps identical."""
    sc, w, h, tw, th = _family_scene(case)
    renderer.set_scene(sc)
    maps = []
    for variant in sorted(VARIANT_KERNEL):
        p = r1.make_params(w, h, 12, 77, tile_w=tw, tile_h=th, variant=variant)
        img, rays, tiles, res = renderer.render_adaptive(p, 4, 4, 16, 65280)
        assert renderer.launch_info()["kernel"] == VARIANT_KERNEL[variant], variant
        img2, rays2, tiles2, res2 = check_contract(renderer, p, 4, 4, 16, 65280)
        assert rays2 == rays and img2.tobytes() == img.tobytes() and tiles2.tobytes() == tiles.tobytes() and res2 == res  # (and it repeats)
        maps.append((tiles, rays, img))
    for tiles, rays, img in maps[1:]:
        assert tiles.tobytes() == maps[0][0].tobytes() and rays == maps[0][1] and img.tobytes() == maps[0][2].tobytes()


def test_an_odd_schedule(renderer):
    """(3, 5) under cap 14: counts 3, 8, 13, 14 — passes start at odd global samples, the last one is cut short."""
    w, h = 200, 100
    renderer.set_scene(r1.create_medium_scene(w, h))
    p = r1.make_params(w, h, 14, 4242)
    assert r1.adaptive_schedule(p, 3, 5) == [3, 8, 13, 14]
    for max_delta, mean_q8 in ((48, 768), (20, 65280), (-1, 0)):
        img, rays, tiles, res = check_contract(renderer, p, 3, 5, max_delta, mean_q8)
        assert set(int(x) for x in tiles["spp"]) <= {3, 8, 13, 14}
    assert (tiles["spp"] == 14).all() and res["passes"] == 4


def test_refusals_through_a_live_context(renderer):
    w, h = 96, 64
    fresh = r1.Renderer(0)
    try:
        expect_refusal(lambda: fresh.render_adaptive(r1.make_params(w, h, 8, 5), 4, 4, 16, 65280), "no scene set")
    finally:
        fresh.close()
    renderer.set_scene(r1.create_medium_scene(w, h))
    p = r1.make_params(w, h, 8, 91)
    want = renderer.render(p)

    def still_renders():
        got = renderer.render(p)
        assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes()

    for opt, text in (((0, 4, 16, 65280), "min_spp"), ((4, 0, 16, 65280), "pass_spp"), ((4, 4, -2, 65280), "max_delta"), ((4, 4, 256, 65280), "max_delta"),
                      ((4, 4, 16, -1), "mean_delta_q8"), ((4, 4, 16, 65281), "mean_delta_q8")):
        expect_refusal(lambda: renderer.render_adaptive(p, *opt), text)
        still_renders()
    expect_refusal(lambda: renderer.render_adaptive(r1.make_params(w, h, 8, 91, shard=0, num_shards=2), 4, 4, 16, 65280), "num_shards")
    still_renders()
    for v in (binding.VARIANT_REFERENCE, binding.VARIANT_STATS, binding.VARIANT_BVH_STATS, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID_STATS):
        expect_refusal(lambda: renderer.render_adaptive(r1.make_params(w, h, 8, 91, variant=v), 4, 4, 16, 65280), "has no listed-tile build")
        still_renders()
    expect_refusal(lambda: renderer.render_adaptive(r1.make_params(33, 33, 1000000, 91), 600000, 8, 16, 65280), "sample slots per launch", code=binding.R1_ELIMIT)
    still_renders()
    # an adaptive frame ends a progressive accumulation and leaves none behind
    renderer.render_pass(with_spp(p, 2), 0)
    renderer.render_pass(with_spp(p, 2), 2)
    img, rays, tiles, res = renderer.render_adaptive(p, 4, 4, 255, 65280)
    want4 = renderer.render(with_spp(p, 4))
    assert rays == want4[1] and img.tobytes() == want4[0].tobytes()
    expect_refusal(lambda: renderer.render_pass(with_spp(p, 2), 4), "no accumulation to continue")
    # and a new accumulation works as before
    renderer.render_pass(with_spp(p, 3), 0)
    img, rays = renderer.render_pass(with_spp(p, 5), 3)
    assert rays == want[1] and img.tobytes() == want[0].tobytes()


@pytest.mark.parametrize("case", ["small", "big"])
def test_other_calls_around_an_adaptive_frame(renderer, case):
    """r1_render_async into a page-locked frame and a batch of two, before and after an adaptive frame on the same context: the frames
    r1_render gives (the landing state of the throughput kernels survives)."""
    if case == "big":
        sc, w, h = r1.create_grid_scene(128, 80, 400, 250), 128, 80
    else:
        sc, w, h = r1.create_small_scene(96, 64), 96, 64
    renderer.set_scene(sc)
    p = r1.make_params(w, h, 12, 13)
    other = r1.make_params(w, h, 3, 500)
    want_other = renderer.render(other)
    want_b = [renderer.render(r1.make_params(w, h, 3, 500 + f)) for f in range(2)]
    hf1, hf2 = binding.HostFrames(w, h, 1), binding.HostFrames(w, h, 2)

    def others():
        renderer.render_async(other, hf1)
        renderer.sync()
        assert hf1.rays(0) == want_other[1] and hf1.image(0).tobytes() == want_other[0].tobytes()
        hf1.image(0)[:] = 0
        renderer.render_batch_async(other, 2, hf2, seed_stride=1)
        renderer.sync()
        for f in range(2):
            assert hf2.rays(f) == want_b[f][1] and hf2.image(f).tobytes() == want_b[f][0].tobytes(), f
            hf2.image(f)[:] = 0

    try:
        others()
        first = check_contract(renderer, p, 4, 4, 16, 65280)
        others()
        others()
        again = renderer.render_adaptive(p, 4, 4, 16, 65280)
        assert again[1] == first[1] and again[0].tobytes() == first[0].tobytes() and again[2].tobytes() == first[2].tobytes()
        got = renderer.render(other)
        assert got[1] == want_other[1] and got[0].tobytes() == want_other[0].tobytes()
        others()
    finally:
        hf1.close()
        hf2.close()


def test_full_size_large_1200x800_cap_250(renderer):
    """Large 1200 x 800, cap 250, (25, 25), 32 / 512: every tile's pixels are the crop of r1_render at its count; page-locked and pageable
    rgb_out give the same frame."""
    w, h, cap = 1200, 800, 250
    renderer.set_scene(r1.create_large_scene(w, h))
    p = r1.make_params(w, h, cap, 10001)
    img, rays, tiles, res = renderer.render_adaptive(p, 25, 25, 32, 512)
    check_pixels_and_result(renderer, p, 25, 25, img, tiles, res)
    assert res["samples"] == rule.samples_of(tiles, w, h)
    assert set(int(x) for x in tiles["spp"]) <= set(range(25, 251, 25))
    print("full size:", rule.histogram(tiles), "samples share", res["samples"] / (w * h * cap), "passes", res["passes"])
    hf = binding.HostFrames(w, h, 1)
    try:
        img2, rays2, tiles2, res2 = renderer.render_adaptive(p, 25, 25, 32, 512, out=hf.image(0))
        assert rays2 == rays and img2.tobytes() == img.tobytes() and tiles2.tobytes() == tiles.tobytes() and res2 == res
    finally:
        hf.close()


def test_program_adaptive_option(tmp_path, renderer):
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    w, h, cap = 160, 96, 64
    plain, adapt = tmp_path / "plain", tmp_path / "adapt"
    plain.mkdir(), adapt.mkdir()
    base = [exe, "-w", "--width", str(w), "--height", str(h), "--spp", str(cap)]
    a = subprocess.run(base, cwd=plain, capture_output=True, timeout=300)
    b = subprocess.run(base + ["--adaptive", "24", "--min-spp", "8", "--pass-spp", "8"], cwd=adapt, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    assert b.returncode == 0, b.stderr.decode()
    ta, tb = a.stdout.decode(), b.stdout.decode()
    assert "adaptive:" not in ta
    line = r"^{} adaptive: passes (\d+), tiles settled (\d+) / (\d+), samples (\d+) \((\d\.\d{{4}}) of cap x pixels\), rays (\d+) \((\d+\.\d{{4}}) of cap x pixels\)$"
    block = r"^{}\nelapsed time:   \d+\.\d{{3}}s\ntotal samples:  (\d+)\ntotal rays:     (\d+)\nmrays/s:        \d+\.\d\d\n"
    for name, make in (("small", r1.create_small_scene), ("medium", r1.create_medium_scene), ("large", r1.create_large_scene)):
        got = re.findall(line.format(name), tb, flags=re.M)
        assert len(got) == 1, (name, tb)
        passes, settled, n_tiles, samples, share, rays, per = got[0]
        rb = re.findall(block.format(name), tb, flags=re.M)
        assert len(rb) == 1 and int(rb[0][0]) == w * h * cap and int(rb[0][1]) == int(rays), name
        # the ABI path's frame
        renderer.set_scene(make(w, h))
        img, want_rays, tiles, res = renderer.render_adaptive(r1.make_params(w, h, cap, 10001), 8, 8, 24, 65280)
        assert (int(passes), int(settled), int(n_tiles), int(samples), int(rays)) == (res["passes"], res["tiles_settled"], res["tiles"], res["samples"], want_rays), name
        assert abs(float(share) - res["samples"] / (w * h * cap)) <= 1e-4
        assert (adapt / f"out_{name}.tga").read_bytes() == r1o.tga_bytes(img), name
        assert re.fullmatch(rf"hip\|\d+\.\d{{3}}s\|{rays}\|\d+\.\d{{3}} mrays/s\|", (adapt / f"out_{name}.txt").read_text())
    # the rest of the report block is the same lines plus the one `adaptive:` line (times, counts and the last launch's workgroups aside)
    strip = lambda t: [ln for ln in t.splitlines() if not re.match(r"(elapsed time|mrays/s|device time|devices|total rays|\w+ adaptive):", ln)]
    assert strip(ta) == strip(tb)
