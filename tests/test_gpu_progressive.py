"""GPU tests of progressive rendering (r1_render_pass): samples [a, b) traced with their global sample indices and added
in sample order to a per-pixel fp32 accumulator holding the sum of [0, a) give exactly the sums the one-launch resolve computes for
spp = b.  So every preview and every cumulative ray count must equal r1_render at the accumulated spp, BIT FOR BIT, and the oracle
where it is asked directly."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VARIANT_KERNEL = {binding.VARIANT_DEFAULT: binding.VARIANT_BVH, binding.VARIANT_REFERENCE: binding.VARIANT_REFERENCE,
                  binding.VARIANT_PREFILTER: binding.VARIANT_PREFILTER, binding.VARIANT_GRID: binding.VARIANT_GRID}


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def run_passes(renderer, params, sizes, image_every=True):
    """Renders `params` in passes of `sizes` samples; returns [(preview or None, cumulative rays)] after every pass."""
    out, first = [], 0
    for k, n in enumerate(sizes):
        q = r1.make_params(params.width, params.height, n, params.seed, params.max_bounces, params.tile_w, params.tile_h, variant=params.variant)
        out.append(renderer.render_pass(q, first, image=image_every or k == len(sizes) - 1))
        first += n
    return out


def with_spp(p, spp):
    return r1.make_params(p.width, p.height, spp, p.seed, p.max_bounces, p.tile_w, p.tile_h, variant=p.variant)


def expect_refusal(fn, rule, code=binding.R1_EINVAL):
    """The call fails with `code`, and r1_last_error names `rule`: the refusal comes from that check, not from another one the call also
    breaks."""
    with pytest.raises(binding.R1Error) as e:
        fn()
    assert e.value.code == code, e.value
    assert rule in str(e.value), e.value


def test_previews_are_the_renders_large_1200x800(renderer):
    """Passes of 1, 2, 4 and 3 samples: after every pass the preview and the cumulative count are r1_render's at 1, 3, 7 and 10 spp."""
    with open(os.path.join(GOLD, "full_1200x800x10.json")) as f:
        full = json.load(f)["large"]
    w, h, seed = full["w"], full["h"], full["seed"]
    renderer.set_scene(r1.create_large_scene(w, h))
    p = r1.make_params(w, h, 10, seed)
    got = run_passes(renderer, p, [1, 2, 4, 3])
    assert renderer.launch_info()["kernel"] == binding.VARIANT_BVH and renderer.launch_info()["tiles_in_kernel"] == 0
    for (img, rays), n in zip(got, [1, 3, 7, 10]):
        want_img, want_rays, _ = renderer.render(with_spp(p, n))
        assert rays == want_rays, n
        assert img.tobytes() == want_img.tobytes(), n
    assert abs(got[-1][1] - full["rays"]) <= max(4, full["rays"] * 1e-5), (got[-1][1], full["rays"])


def _family_scene(case):
    if case == "big":
        return r1.create_grid_scene(256, 160, 400, 250), 256, 160
    if case == "ragged":
        return r1.create_medium_scene(77, 45), 77, 45
    w, h = 96, 64
    return {"small": r1.create_small_scene, "medium": r1.create_medium_scene}[case](w, h), w, h


@pytest.mark.parametrize("variant", sorted(VARIANT_KERNEL), ids=lambda v: {0: "default", 1: "reference", 2: "prefilter", 7: "grid"}[v])
@pytest.mark.parametrize("case", ["small", "medium", "ragged", "big"])
def test_every_family_passes_2_3_equal_one_render_of_5(renderer, case, variant):
    sc, w, h = _family_scene(case)
    renderer.set_scene(sc)
    p = r1.make_params(w, h, 5, 77, variant=variant)
    got = run_passes(renderer, p, [2, 3])
    assert renderer.launch_info()["kernel"] == VARIANT_KERNEL[variant]
    want_img, want_rays, _ = renderer.render(p)
    assert got[-1][1] == want_rays
    assert got[-1][0].tobytes() == want_img.tobytes()
    want2 = renderer.render(with_spp(p, 2))
    assert got[0][1] == want2[1] and got[0][0].tobytes() == want2[0].tobytes()


def test_passes_equal_the_oracle_frame(renderer):
    w, h, seed = 40, 24, 4242
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    got = run_passes(renderer, r1.make_params(w, h, 7, seed), [1, 2, 4])
    oimg, orays, _ = r1o.render_frame(r1o.SceneArrays.from_c(sc.spheres, sc.camera), r1o.make_params(w, h, 7, seed))
    assert got[-1][1] == orays
    assert got[-1][0].tobytes() == oimg.tobytes()


def test_config4_full_size_in_four_passes(renderer):
    """1200 x 800 x 250 (BASELINE config 4) in passes of 1, 9, 40 and 200 samples equals one r1_render at 250 spp."""
    w, h = 1200, 800
    renderer.set_scene(r1.create_large_scene(w, h))
    p = r1.make_params(w, h, 250, 10001)
    got = run_passes(renderer, p, [1, 9, 40, 200], image_every=False)
    assert got[0][0] is None and got[-1][0] is not None
    want_img, want_rays, _ = renderer.render(p)
    assert got[-1][1] == want_rays
    assert got[-1][0].tobytes() == want_img.tobytes()


def _quantise(col, n):
    """r1_resolve_kernel's arithmetic on sequential fp32 sums: * (float)(1.0f / n), sqrtf, (uint8)(int)(c * 255.99f)."""
    c = col.astype(np.float32) * (np.float32(1.0) / np.float32(n))
    return (np.sqrt(c) * np.float32(255.99)).astype(np.int32).astype(np.uint8)


def test_a_frame_beyond_the_one_launch_ceiling(renderer):
    """256 x 128 x 65 536 = 2^31 samples: no one-launch entry point can render it; passes can, in any split, and its pixels are the oracle's
    sequential fp32 sums."""
    w, h, spp, seed = 256, 128, 65536, 31337
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    p = r1.make_params(w, h, spp, seed)
    with pytest.raises(binding.R1Error) as e:
        renderer.render(p)
    assert e.value.code == binding.R1_ELIMIT
    a = run_passes(renderer, p, [16384] * 4, image_every=False)
    b = run_passes(renderer, p, [1, 16383, 16384, 16384, 16384], image_every=False)
    assert a[-1][1] == b[-1][1] and a[-1][0].tobytes() == b[-1][0].tobytes()
    img = a[-1][0]
    sa = r1o.SceneArrays.from_c(sc.spheres, sc.camera)
    for x, y in ((0, 0), (255, 127), (131, 70), (40, 101)):
        ss = np.arange(spp)
        rgb, _ = r1o.trace_samples(sa, w, h, seed, np.full(spp, x), np.full(spp, y), ss)
        col = np.cumsum(rgb, axis=0, dtype=np.float32)[-1]  # (sequential fp32 adds in sample order, as the resolve)
        assert img[y, x].tobytes() == _quantise(col, spp).tobytes(), (x, y)


def test_pass_contract_rejections_keep_the_accumulation(renderer):
    w, h = 96, 64
    renderer.set_scene(r1.create_medium_scene(w, h))
    p = r1.make_params(w, h, 5, 91)
    q = lambda spp, **k: r1.make_params(k.get("w", w), k.get("h", h), spp, k.get("seed", 91), variant=k.get("variant", 0))
    no_build, not_accumulated, differ = "has no progressive-pass build", "samples are accumulated", "parameters differ"
    for v in (binding.VARIANT_STATS, binding.VARIANT_BVH_STATS, binding.VARIANT_GRID_STATS, binding.VARIANT_WAVEFRONT):
        expect_refusal(lambda: renderer.render_pass(q(2, variant=v), 0), no_build)
    expect_refusal(lambda: renderer.render_pass(q(2), 2), "no accumulation to continue")
    renderer.render_pass(q(2), 0)
    expect_refusal(lambda: renderer.render_pass(q(3), 3), not_accumulated)  # wrong first sample
    expect_refusal(lambda: renderer.render_pass(q(3), 1), not_accumulated)
    expect_refusal(lambda: renderer.render_pass(q(3, seed=92), 2), differ)  # changed seed
    expect_refusal(lambda: renderer.render_pass(q(3, w=97), 2), differ)     # changed size
    expect_refusal(lambda: renderer.render_pass(q(3, variant=binding.VARIANT_PREFILTER), 2), differ)  # changed variant
    expect_refusal(lambda: renderer.render_pass(q(3, variant=binding.VARIANT_STATS), 2), no_build)
    expect_refusal(lambda: renderer.render_pass(q(3), -1), "not within [0, INT32_MAX]")
    # total beyond INT32_MAX: an accumulation that gets there takes 2^31 samples per pixel, summed one after the other by one thread each
    # (minutes); this call also breaks the first-sample rule, so the error text shows which check refused it
    expect_refusal(lambda: renderer.render_pass(q(3), 2 ** 31 - 3), "not within [0, INT32_MAX]")
    shard = r1.make_params(w, h, 3, 91, shard=0, num_shards=2)
    expect_refusal(lambda: renderer.render_pass(shard, 0), "whole frames")  # (first_sample 0: only the shard rule applies)
    # a pass beyond the per-pass limit (w * h * spp >= 2^31) of an accumulation it would otherwise continue
    expect_refusal(lambda: renderer.render_pass(q(2 ** 31 // (w * h) + 1), 2), "exceeds 2^31", code=binding.R1_ELIMIT)
    img, rays = renderer.render_pass(q(3), 2)                        # continuing correctly still matches
    want = renderer.render(p)
    assert rays == want[1] and img.tobytes() == want[0].tobytes()
    # a scene upload (even of the same arrays) ends the accumulation
    renderer.set_scene(r1.create_medium_scene(w, h))
    expect_refusal(lambda: renderer.render_pass(q(1), 5), "no accumulation to continue")
    got = run_passes(renderer, p, [4, 1])
    assert got[-1][1] == want[1] and got[-1][0].tobytes() == want[0].tobytes()


@pytest.mark.parametrize("case", ["small", "big"])
def test_other_calls_between_passes_disturb_nothing(renderer, case):
    if case == "big":
        sc, w, h = r1.create_grid_scene(128, 80, 400, 250), 128, 80
    else:
        sc, w, h = r1.create_small_scene(96, 64), 96, 64
    renderer.set_scene(sc)
    p = r1.make_params(w, h, 5, 13)
    other = r1.make_params(w, h, 3, 500)
    other_sz = r1.make_params(w // 2, h // 2, 4, 600)
    want = renderer.render(p)
    want_other, want_sz = renderer.render(other), renderer.render(other_sz)
    want_b = [renderer.render(r1.make_params(w, h, 3, 500 + f)) for f in range(2)]
    hf1, hf2 = binding.HostFrames(w, h, 1), binding.HostFrames(w, h, 2)
    try:
        renderer.render_pass(with_spp(p, 1), 0)
        got_other = renderer.render(other)
        renderer.render_pass(with_spp(p, 1), 1)
        got_sz = renderer.render(other_sz)
        renderer.render_async(other, hf1)
        renderer.sync()
        img2, rays2 = renderer.render_pass(with_spp(p, 1), 2)
        renderer.render_batch_async(other, 2, hf2, seed_stride=1)
        renderer.sync()
        img, rays = renderer.render_pass(with_spp(p, 2), 3)
        assert rays == want[1] and img.tobytes() == want[0].tobytes()
        want3 = renderer.render(with_spp(p, 3))
        assert rays2 == want3[1] and img2.tobytes() == want3[0].tobytes()
        assert got_other[1] == want_other[1] and got_other[0].tobytes() == want_other[0].tobytes()
        assert got_sz[1] == want_sz[1] and got_sz[0].tobytes() == want_sz[0].tobytes()
        assert hf1.rays(0) == want_other[1] and hf1.image(0).tobytes() == want_other[0].tobytes()
        for f in range(2):
            assert hf2.rays(f) == want_b[f][1] and hf2.image(f).tobytes() == want_b[f][0].tobytes(), f
        # and the frames after the passes are still the stand-alone ones
        renderer.render_async(other, hf1)
        renderer.sync()
        assert hf1.rays(0) == want_other[1] and hf1.image(0).tobytes() == want_other[0].tobytes()
        again = renderer.render(p)
        assert again[1] == want[1] and again[0].tobytes() == want[0].tobytes()
    finally:
        hf1.close()
        hf2.close()


def test_program_passes_option(tmp_path):
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    w, h, spp = 160, 96, 7
    one, three = tmp_path / "one", tmp_path / "three"
    one.mkdir(), three.mkdir()
    base = [exe, "-w", "--width", str(w), "--height", str(h), "--spp", str(spp)]
    a = subprocess.run(base, cwd=one, capture_output=True, timeout=300)
    b = subprocess.run(base + ["--passes", "3"], cwd=three, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    assert b.returncode == 0, b.stderr.decode()
    ta, tb = a.stdout.decode(), b.stdout.decode()
    assert "passes:" not in ta and tb.count("passes:         3\n") == 3
    block = r"^{}\nelapsed time:   \d+\.\d{{3}}s\ntotal samples:  (\d+)\ntotal rays:     (\d+)\nmrays/s:        \d+\.\d\d\n"
    for name in ("small", "medium", "large"):
        ra = re.findall(block.format(name), ta, flags=re.M)
        rb = re.findall(block.format(name), tb, flags=re.M)
        assert len(ra) == 1 and ra == rb and int(rb[0][0]) == w * h * spp, name
        assert (one / f"out_{name}.tga").read_bytes() == (three / f"out_{name}.tga").read_bytes(), name
        assert re.fullmatch(rf"hip\|\d+\.\d{{3}}s\|{rb[0][1]}\|\d+\.\d{{3}} mrays/s\|", (three / f"out_{name}.txt").read_text())
        rec = json.loads((three / f"out_{name}.json").read_text())
        assert rec["runs"][0]["num_rays"] == int(rb[0][1]) and rec["runs"][0]["device_seconds"] > 0
    # the rest of the report block is the same lines, plus the one `passes:` line (times and the last launch's workgroups aside)
    strip = lambda t: [ln for ln in t.splitlines() if not re.match(r"(elapsed time|mrays/s|device time|devices|passes):", ln)]
    assert strip(ta) == strip(tb)
    assert len(re.findall(r"^devices:        1 \(", tb, flags=re.M)) == 3
