"""GPU tests of region renders (include/rays1.h): a window of the frame is, bit for bit, the crop of the whole frame — bytes,
linear values, sample records and ray count — in every variant and kernel family, for windows that sit off the frame's own tile grid, on a frame
no launch holds, after an update, into device memory, and without disturbing what else the context holds.

Expected values come from code the region path does not touch: the whole-frame calls (render_samples, render, render_linear) on the same
context, and the oracle's per-sample restatement (tests/region_cases.py oracle_window).  Every comparison is tobytes() equality."""
import os
import subprocess

import numpy as np
import pytest
import torch

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import linear_cases as lc
import region_cases as rc
from test_refit_host import moved_centres, raw_from_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def other():
    r = r1.Renderer(0)
    yield r
    r.close()


def expect_refusal(fn, text=None, code=binding.R1_EINVAL):
    with pytest.raises(binding.R1Error) as e:
        fn()
    assert e.value.code == code, e.value
    if text:
        assert text in str(e.value), e.value


def whole_frame(rend, p):
    """what the whole-frame calls return for p: (bytes (h, w, 3), count, records (h, w, spp, 4), linear (h, w, 3))"""
    img, rays, samples = rend.render_samples(p)
    lin, lin_rays, _ = rend.render_linear(p)
    plain, plain_rays, _ = rend.render(p)
    assert rays == lin_rays == plain_rays and plain.tobytes() == img.tobytes()
    return img, rays, rc.records_of(samples, p.width, p.height, p.spp), lin


def check_window(rend, p, win, frame, what):
    img, rays, rec, lin = frame
    want_rec = rc.crop(rec, win)
    want_rays = rc.count_of(want_rec)
    got, got_rays, got_samples = rend.render_region_samples(p, win)
    assert got.tobytes() == rc.crop(img, win).tobytes(), (what, "bytes", int((got != rc.crop(img, win)).sum()))
    assert got_samples.tobytes() == want_rec.tobytes(), (what, "records")
    assert got_rays == want_rays, (what, "count", got_rays, want_rays)
    plain, plain_rays, secs = rend.render_region(p, win)
    assert plain.tobytes() == got.tobytes() and plain_rays == want_rays and secs > 0, (what, "r1_render_region")
    glin, lin_rays, _ = rend.render_region_linear(p, win)
    assert glin.tobytes() == rc.crop(lin, win).tobytes() and lin_rays == want_rays, (what, "linear")
    info = rend.launch_info()
    assert info["samples"] >= win[2] * win[3] * p.spp and info["tiles_in_kernel"] == 0, (what, info)
    if win == (0, 0, p.width, p.height):
        assert got_rays == rays, (what, "the full frame's count is r1_render's")


# ---- every window, tiling, variant and kernel family against the crop of the whole frame ------------------------------------------------------


@pytest.mark.parametrize("tiling", rc.TILINGS, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("name,w,h,spp", rc.FRAMES, ids=lambda v: str(v))
def test_window_is_the_crop_of_the_whole_frame(renderer, name, w, h, spp, tiling):
    renderer.set_scene(rc.make_scene(name, w, h))
    for vname, variant in rc.VARIANTS.items():
        p = r1.make_params(w, h, spp, rc.SEED, tile_w=tiling[0], tile_h=tiling[1], variant=variant)
        frame = whole_frame(renderer, p)
        kernel = renderer.launch_info()["kernel"]
        for win in rc.windows(w, h):
            check_window(renderer, p, win, frame, (name, vname, kernel, tiling, win))
            assert renderer.launch_info()["kernel"] == kernel  # (the region ran the variant the frame ran)


@pytest.mark.parametrize("name,w,h,spp", rc.FRAMES, ids=lambda v: str(v))
def test_window_is_the_oracles_restatement(renderer, name, w, h, spp):
    sc = rc.make_scene(name, w, h)
    renderer.set_scene(sc)
    sa = r1o.SceneArrays.from_c(sc.spheres, sc.camera)
    wins = [(31, 31, 2, 2), (w - 1, h - 1, 1, 1)] + ([(5, 3, 33, 33)] if name in lc.SCENES else [])
    for win in wins:
        if win == (5, 3, 33, 33):  # (the oracle's whole frame, which tests/linear_cases.py computes once)
            orec, _ = lc.oracle_records(name, w, h, spp)
            rec = rc.crop(orec, win)
            lin, rays = lc.linear_of(rec), rc.count_of(rec)
            q = lc.quantise(lin)
        else:
            rec, lin, q, rays = rc.oracle_window(sa, w, h, spp, win)
        for tiling in rc.TILINGS[:2]:
            p = r1.make_params(w, h, spp, rc.SEED, tile_w=tiling[0], tile_h=tiling[1])
            got, got_rays, got_samples = renderer.render_region_samples(p, win)
            assert got_samples.tobytes() == rec.tobytes() and got_rays == rays and got.tobytes() == q.tobytes(), (name, win, tiling)
            glin, _, _ = renderer.render_region_linear(p, win)
            assert glin.tobytes() == lin.tobytes(), (name, win, tiling)


# ---- paste: out_stride = W into a caller's whole frame -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("vname,tiling", [("default", (32, 32)), ("prefilter", (16, 8)), ("grid", (40, 24)), ("reference", (32, 32))])
def test_four_quadrants_pasted_into_one_frame_are_the_frame(renderer, vname, tiling):
    name, w, h, spp = "medium", 77, 45, 3
    renderer.set_scene(rc.make_scene(name, w, h))
    p = r1.make_params(w, h, spp, rc.SEED, tile_w=tiling[0], tile_h=tiling[1], variant=rc.VARIANTS[vname])
    want, want_rays, _ = renderer.render(p)
    wlin, _, _ = renderer.render_linear(p)
    sx, sy = 37, 19
    quads = [(0, 0, sx, sy), (sx, 0, w - sx, sy), (0, sy, sx, h - sy), (sx, sy, w - sx, h - sy)]
    frame = np.full((h, w, 3), rc.PREFILL, np.uint8)
    flin = np.frombuffer(bytes([rc.PREFILL]) * (h * w * 12), np.float32).reshape(h, w, 3).copy()
    total = 0
    for k, (x0, y0, ww, wh) in enumerate(quads):
        before = frame.copy()
        _, rays, _ = renderer.render_region(p, (x0, y0, ww, wh), out=frame[y0:y0 + wh, x0:x0 + ww])
        total += rays
        outside = np.ones((h, w), bool)
        outside[y0:y0 + wh, x0:x0 + ww] = False
        assert (frame[outside] == before[outside]).all(), (k, "bytes outside the window were written")
        _, lrays, _ = renderer.render_region_linear(p, (x0, y0, ww, wh), out=flin[y0:y0 + wh, x0:x0 + ww])
        assert lrays == rays
    assert frame.tobytes() == want.tobytes() and total == want_rays
    assert flin.tobytes() == wlin.tobytes()


# ---- a frame no launch holds ---------------------------------------------------------------------------------------------------------------------


def test_windows_of_a_frame_beyond_one_launch(renderer):
    w, h, spp = rc.HUGE
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    sa = r1o.SceneArrays.from_c(sc.spheres, sc.camera)
    p = r1.make_params(w, h, spp, rc.SEED)
    info = renderer.launch_info()
    expect_refusal(lambda: renderer.render_into(p, np.zeros((1, 1, 3), np.uint8)), code=binding.R1_ELIMIT)
    assert renderer.launch_info() == info
    for win in rc.HUGE_WINDOWS:
        rec, lin, q, rays = rc.oracle_window(sa, w, h, spp, win)
        for vname in ("default", "prefilter", "grid", "reference"):
            pv = r1.make_params(w, h, spp, rc.SEED, variant=rc.VARIANTS[vname])
            got, got_rays, got_samples = renderer.render_region_samples(pv, win)
            assert got_samples.tobytes() == rec.tobytes() and got_rays == rays and got.tobytes() == q.tobytes(), (win, vname)
            glin, _, _ = renderer.render_region_linear(pv, win)
            assert glin.tobytes() == lin.tobytes(), (win, vname)
    expect_refusal(lambda: binding.region_check(p, (0, 0, 32768, 32768)), code=binding.R1_ELIMIT)


# ---- a moved scene -------------------------------------------------------------------------------------------------------------------------------


def test_window_of_a_moved_and_resorted_scene(renderer, other):
    w, h, spp = 96, 64, 3
    win = (40, 17, 39, 35)
    sc = r1.create_large_scene(w, h)
    a = sc.arrays()
    x, y, z = moved_centres(a, "permute")
    renderer.set_scene(sc)
    renderer.regrid()  # (the grid is built before the first update, so that r1_regrid can re-register the moved spheres in it)
    renderer.update_centers(0, x, y, z)
    renderer.resort_spheres()
    cs, keep = raw_from_arrays(a, x, y, z)
    other.set_scene_raw(cs, sc.camera.contents)
    p = r1.make_params(w, h, spp, 777)
    frame = whole_frame(other, p)  # a fresh context's frame of the moved arrays
    check_window(renderer, p, win, frame, ("moved", win))
    # as for frames: the sphere groups and the grid are stale; the grid serves again after r1_regrid
    for vname in ("prefilter", "grid"):
        pv = r1.make_params(w, h, spp, 777, variant=rc.VARIANTS[vname])
        info = renderer.launch_info()
        expect_refusal(lambda: renderer.render_region(pv, win), "the scene has moved")
        expect_refusal(lambda: renderer.render(pv), "the scene has moved")
        assert renderer.launch_info() == info
    renderer.regrid()
    pg = r1.make_params(w, h, spp, 777, variant=rc.VARIANTS["grid"])
    check_window(renderer, pg, win, frame, ("moved, regridded", win))
    expect_refusal(lambda: renderer.render_region(r1.make_params(w, h, spp, 777, variant=rc.VARIANTS["prefilter"]), win), "the scene has moved")
    check_window(renderer, r1.make_params(w, h, spp, 777, variant=rc.VARIANTS["reference"]), win, frame, ("moved, reference form", win))


# ---- into device memory --------------------------------------------------------------------------------------------------------------------------


def test_device_form_writes_both_images_with_the_stride_and_waits_for_nothing(renderer):
    name, w, h, spp = "medium", 77, 45, 3
    renderer.set_scene(rc.make_scene(name, w, h))
    p = r1.make_params(w, h, spp, rc.SEED, tile_w=16, tile_h=8)
    img, rays, rec, lin = whole_frame(renderer, p)
    wins = [(5, 3, 33, 33), (31, 31, 2, 2)]
    stream = torch.cuda.Stream()
    u8 = [torch.full((h, w, 3), rc.PREFILL, dtype=torch.uint8, device="cuda") for _ in wins]
    f32 = [torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda") for _ in wins]
    cnt = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in wins]
    torch.cuda.synchronize()
    # two calls on one stream, each writing bytes AND floats in place in a whole frame (out_stride = W), before one wait
    for k, (x0, y0, ww, wh) in enumerate(wins):
        off = y0 * w + x0
        renderer.render_region_device(p, wins[k], u8[k].data_ptr() + off * 3, f32[k].data_ptr() + off * 12, cnt[k].data_ptr(), out_stride=w, stream_ptr=stream.cuda_stream)
    stream.synchronize()
    for k, win in enumerate(wins):
        x0, y0, ww, wh = win
        got, glin = u8[k].cpu().numpy(), f32[k].cpu().numpy()
        assert rc.crop(got, win).tobytes() == rc.crop(img, win).tobytes() and rc.crop(glin, win).tobytes() == rc.crop(lin, win).tobytes(), win
        outside = np.ones((h, w), bool)
        outside[y0:y0 + wh, x0:x0 + ww] = False
        assert (got[outside] == rc.PREFILL).all() and (glin[outside] == -7.0).all(), win
        assert int(cnt[k].item()) == rc.count_of(rc.crop(rec, win)), win
    # one image alone, dense (out_stride 0), on the context's own stream
    win = wins[0]
    only = torch.full((win[3], win[2], 3), rc.PREFILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    renderer.render_region_device(p, win, only.data_ptr(), None, cnt[0].data_ptr())
    renderer.sync()
    assert only.cpu().numpy().tobytes() == rc.crop(img, win).tobytes()
    onlyf = torch.full((win[3], win[2], 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.render_region_device(p, win, None, onlyf.data_ptr(), cnt[0].data_ptr())
    renderer.sync()
    assert onlyf.cpu().numpy().tobytes() == rc.crop(lin, win).tobytes()
    # refusals enqueue nothing: misaligned and NULL pointers, a window outside the frame
    info = renderer.launch_info()
    before = (u8[0].clone(), f32[0].clone(), cnt[0].clone())
    a, b, c = u8[0].data_ptr(), f32[0].data_ptr(), cnt[0].data_ptr()
    expect_refusal(lambda: renderer.render_region_device(p, win, a, b + 1, c), "aligned")
    expect_refusal(lambda: renderer.render_region_device(p, win, a, b, c + 4), "aligned")
    expect_refusal(lambda: renderer.render_region_device(p, win, None, None, c), "null")
    expect_refusal(lambda: renderer.render_region_device(p, win, a, b, None), "null")
    expect_refusal(lambda: renderer.render_region_device(p, (w - 2, 0, 3, 3), a, b, c), "x0 + width")
    expect_refusal(lambda: renderer.render_region_device(p, win, a, b, c, out_stride=win[2] - 1), "out_stride")
    renderer.sync()
    torch.cuda.synchronize()
    assert renderer.launch_info() == info
    assert torch.equal(u8[0], before[0]) and torch.equal(f32[0].view(torch.int32), before[1].view(torch.int32)) and torch.equal(cnt[0], before[2])


# ---- what else the context holds -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("vname,tiling", [("default", (32, 32)), ("prefilter", (16, 8)), ("grid", (40, 24))])
def test_a_region_render_leaves_the_contexts_state_alone(renderer, vname, tiling):
    name, w, h = "medium", 77, 45
    renderer.set_scene(rc.make_scene(name, w, h))
    par = lambda spp: r1.make_params(w, h, spp, rc.SEED, tile_w=tiling[0], tile_h=tiling[1], variant=rc.VARIANTS[vname])  # noqa: E731
    want, want_rays, _ = renderer.render(par(4))
    win = (5, 3, 33, 33)
    # a progressive accumulation goes on across a region render (of other params)
    renderer.render_pass(par(2), 0)
    reg, reg_rays, _ = renderer.render_region(par(3), win)
    img, rays = renderer.render_pass(par(2), 2)
    assert img.tobytes() == want.tobytes() and rays == want_rays
    # r1_render before and after a region gives the same bytes, and the region is that of ITS params' frame
    frame3 = whole_frame(renderer, par(3))
    assert reg.tobytes() == rc.crop(frame3[0], win).tobytes() and reg_rays == rc.count_of(rc.crop(frame3[2], win))
    again, again_rays, _ = renderer.render(par(4))
    assert again.tobytes() == want.tobytes() and again_rays == want_rays
    # r1_last_launch_info and r1_last_timing describe the region render
    renderer.render_region(par(3), win)
    info = renderer.launch_info()
    tiles = -(-win[2] // tiling[0]) * -(-win[3] // tiling[1])
    assert info["samples"] == tiles * tiling[0] * tiling[1] * 3 and info["tiles_in_kernel"] == 0, info
    trace_ms, total_ms = renderer.last_timing()
    assert 0 < trace_ms <= total_ms
    # render_samples afterwards still returns untagged count words (1 .. 51 calls of color() per sample)
    _, srays, samples = renderer.render_samples(par(3))
    words = np.ascontiguousarray(samples[:, 3]).view(np.uint32)
    assert int(words.max()) <= 51 and int(words.min()) >= 1 and int(words.astype(np.uint64).sum()) == srays
    # each refusal leaves r1_last_launch_info as it was
    renderer.render_region(par(3), win)
    info = renderer.launch_info()
    expect_refusal(lambda: renderer.render_region(par(3), (w - 2, 0, 3, 3)), "x0 + width")
    expect_refusal(lambda: renderer.render_region(par(3), (0, 0, 0, 3)), "width")
    expect_refusal(lambda: renderer.render_region(r1.make_params(w, h, 3, shard=0, num_shards=2), win), "num_shards")
    for v in rc.REFUSED_VARIANTS:
        expect_refusal(lambda: renderer.render_region(r1.make_params(w, h, 3, variant=v), win), f"variant {v}")
    expect_refusal(lambda: renderer.render_region_samples(r1.make_params(46341, 46341, 1), (0, 0, 1, 1)), code=binding.R1_ELIMIT)
    assert renderer.launch_info() == info


def test_a_region_render_needs_a_scene():
    r = r1.Renderer(0)
    try:
        expect_refusal(lambda: r.render_region(r1.make_params(32, 16, 1), (0, 0, 8, 8)), "no scene set")
    finally:
        r.close()


# ---- the drop-in program ---------------------------------------------------------------------------------------------------------------------------


def test_program_region_writes_the_windows_pixels(renderer, tmp_path):
    w, h, spp, win = 77, 45, 3, (5, 3, 33, 33)
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", str(w), "--height", str(h), "--spp", str(spp), "--region", ",".join(str(v) for v in win), "-w"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for name, make in lc.SCENES.items():
        renderer.set_scene(make(w, h))
        want, want_rays, _ = renderer.render_region(r1.make_params(w, h, spp, 10001), win)
        data = (tmp_path / f"out_{name}.tga").read_bytes()
        assert len(data) == 18 + win[2] * win[3] * 3
        assert data[12] | (data[13] << 8) == win[2] and data[14] | (data[15] << 8) == win[3]
        bgr = np.frombuffer(data[18:], np.uint8).reshape(win[3], win[2], 3)
        assert bgr[:, :, ::-1].tobytes() == want.tobytes(), name
        line = [ln for ln in out.stdout.splitlines() if ln.startswith(f"{name} region:")]
        assert len(line) == 1 and f"{win[0]},{win[1]} {win[2]}x{win[3]} of {w}x{h}" in line[0] and f"rays {want_rays}" in line[0], (name, line)
        assert f"total rays:     {want_rays}" in out.stdout
        assert (tmp_path / f"out_{name}.txt").exists()
