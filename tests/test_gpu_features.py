"""GPU tests of feature frames (include/rays1.h): r1_render_features and r1_render_features_device against the host form
r1_render_features_host (which tests/test_features_host.py holds to the contract's numpy fold), byte for byte: every variant on small and big
scenes, trip counts below and above a wave's width, launch sizes at the seams of a wave and a claim, regions and strides, a torch tensor on
a stream of its own, the context's state before and after, moved scenes and cameras, and the drop-in program's three PFM files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
import feature_cases as fc
import linear_cases as lc
from test_refit_host import moved_centres, raw_from_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def expect_refusal(fn, text=None, code=binding.R1_EINVAL):
    with pytest.raises(binding.R1Error) as e:
        fn()
    assert e.value.code == code, e.value
    if text:
        assert text in str(e.value), e.value


def set_case(rend, name):
    sa = fc.scene(name)
    rend.set_scene_raw(lc.cscene(sa), lc.ccamera(sa))
    return sa


def mismatch(got, want):
    """what differs, for the assertion's message"""
    bad = got.view(np.uint8).reshape(got.shape + (32,)) != want.view(np.uint8).reshape(want.shape + (32,))
    return int(bad.any(axis=-1).sum()), np.argwhere(bad.any(axis=-1))[:4].tolist()


# ---- every variant on small and big scenes ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["medium", "large", "far", "inside", "far_big", "inside_big", fc.GRID, "glass", "empty"])
def test_every_variant_equals_the_host_form(renderer, name):
    set_case(renderer, name)
    want = fc.host_frame(name)
    for vname, v in fc.VARIANTS.items():
        got, secs = renderer.render_features(fc.params(name, variant=v))
        assert got.tobytes() == want.tobytes(), (name, vname, mismatch(got, want))
        assert secs > 0


@pytest.mark.parametrize("name", ["trip1", "trip65"])
def test_trip_counts_below_and_above_a_waves_width(renderer, name):
    """63 pixels: less than one wave; one walk per lane, and 65 — more walks per lane than lanes per wave"""
    set_case(renderer, name)
    want = fc.host_frame(name)
    assert want.size == 63 and min(fc.classes(want, fc.FRAMES[name][2])[::2]) >= 1
    for vname, v in fc.VARIANTS.items():
        got, _ = renderer.render_features(fc.params(name, variant=v))
        assert got.tobytes() == want.tobytes(), (name, vname, mismatch(got, want))


# ---- sizes at the seams, regions, strides -----------------------------------------------------------------------------------------------------------

SEAM_WINDOWS = [(101, 57, 1, 1), (97, 128, 63, 1), (193, 0, 64, 1), (3, 64, 65, 1), (16, 112, 241, 17)]  # 1, 63, 64, 65 and 4097 pixels


def test_sizes_at_the_seams_of_a_wave_and_a_claim(renderer):
    sa = set_case(renderer, "seams")
    want = fc.host_frame("seams")
    w, h, _ = fc.FRAMES["seams"]
    assert [ww * wh for _, _, ww, wh in SEAM_WINDOWS] == [1, 63, 64, 65, 4097]
    for vname, v in fc.VARIANTS.items():
        p = fc.params("seams", variant=v)
        for win in SEAM_WINDOWS:
            got, _ = renderer.render_features(p, win)
            assert got.tobytes() == fc.crop(want, win).tobytes(), (vname, win)
        # the whole frame at one sample a pixel: 33 153 pixels, several claims per wave
        got, _ = renderer.render_features(p)
        assert got.tobytes() == want.tobytes(), (vname, mismatch(got, want))
    # a window into a frame prefilled with 0xA5, rows out_stride = W apart: nothing between the rows is written
    win = SEAM_WINDOWS[4]
    x0, y0, ww, wh = win
    frame = np.frombuffer(bytes([fc.PREFILL]) * (h * w * 32), binding.FEATURE_DTYPE).reshape(h, w).copy()
    renderer.render_features(fc.params("seams"), win, out=frame[y0:y0 + wh, x0:x0 + ww])
    assert fc.crop(frame, win).tobytes() == fc.crop(want, win).tobytes()
    outside = np.ones((h, w), bool)
    outside[y0:y0 + wh, x0:x0 + ww] = False
    assert (frame.view(np.uint8).reshape(h, w, 32)[outside] == fc.PREFILL).all()
    assert sa is fc.scene("seams")


def test_a_frame_with_more_pixels_than_the_chip_has_lanes(renderer):
    """1280 x 1024 x 1: more pixels than 256 CUs hold lanes at any occupancy, so the launch is persistent, a wave takes several claims — of
    two wave-fulls each (r1_queries.cpp query_slice) — and the host-memory form works in two bands of rows (more than R1_CAST_CHUNK pixels)."""
    name = "claims"
    w, h, _ = fc.FRAMES[name]
    assert w * h > 8 * 256 * 256 and w * h > binding.CAST_CHUNK
    set_case(renderer, name)
    want = fc.host_frame(name)
    assert min(fc.classes(want, 1)[::2]) >= 1000
    for vname, v in fc.VARIANTS.items():
        got, _ = renderer.render_features(fc.params(name, variant=v))
        assert got.tobytes() == want.tobytes(), (vname, mismatch(got, want))


# ---- into a torch tensor on a stream of its own -----------------------------------------------------------------------------------------------------


def as_features(t):
    return t.cpu().numpy().view(binding.FEATURE_DTYPE).reshape(t.shape[:2])


def test_device_form_on_a_torch_stream_with_a_stride_and_a_misaligned_pointer(renderer):
    name = "medium"
    set_case(renderer, name)
    want = fc.host_frame(name)
    w, h, _ = fc.FRAMES[name]
    p = fc.params(name)
    stream = torch.cuda.Stream()
    dense = torch.full((h, w, 8), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # a torch operation follows the call on that stream, with no wait between them: it must see the finished records
    with torch.cuda.stream(stream):
        renderer.render_features_device(p, dense.data_ptr(), stream_ptr=stream.cuda_stream)
        copy = dense.clone()
    stream.synchronize()
    assert as_features(copy).tobytes() == want.tobytes()
    # a window in place in a whole frame (out_stride = W): the sentinel outside it stays
    win = (5, 3, 21, 9)
    x0, y0, ww, wh = win
    frame = torch.full((h, w, 8), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.render_features_device(p, frame.data_ptr() + (y0 * w + x0) * 32, region=win, stream_ptr=stream.cuda_stream, out_stride=w)
    stream.synchronize()
    got = frame.cpu().numpy()
    assert fc.crop(got.view(binding.FEATURE_DTYPE).reshape(h, w), win).tobytes() == fc.crop(want, win).tobytes()
    outside = np.ones((h, w), bool)
    outside[y0:y0 + wh, x0:x0 + ww] = False
    assert (got[outside] == -7.0).all()
    # a pointer off by 4 bytes, and NULL: refused, nothing enqueued, nothing written
    info = renderer.launch_info()
    before = frame.clone()
    expect_refusal(lambda: renderer.render_features_device(p, frame.data_ptr() + 4, stream_ptr=stream.cuda_stream), "16-byte aligned")
    expect_refusal(lambda: renderer.render_features_device(p, None, stream_ptr=stream.cuda_stream), "d_out")
    stream.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(frame.view(torch.int32), before.view(torch.int32)) and renderer.launch_info() == info


# ---- refusals, in the documented order ----------------------------------------------------------------------------------------------------------------


def test_refusals_in_the_documented_order():
    r = r1.Renderer(0)
    try:
        p = fc.params("medium")
        out = np.frombuffer(bytes([fc.PREFILL]) * (p.height * p.width * 32), binding.FEATURE_DTYPE).reshape(p.height, p.width).copy()
        L = r1.lib()
        # before the first r1_set_scene: bad params, region and variant are named first; then the missing scene; a NULL out comes last
        bad_region = binding.Region(30, 1, 4, 4, 0)
        assert L.r1_render_features(r._c, None, None, None, None) == binding.R1_EINVAL and "params" in L.r1_last_error().decode()
        assert L.r1_render_features(r._c, C.byref(p), C.byref(bad_region), None, None) == binding.R1_EINVAL and "x0 + width" in L.r1_last_error().decode()
        for v in fc.REFUSED_VARIANTS:
            q = fc.params("medium", variant=v)
            assert L.r1_render_features(r._c, C.byref(q), None, None, None) == binding.R1_EINVAL and f"variant {v}" in L.r1_last_error().decode(), v
            assert L.r1_render_features_device(r._c, C.byref(q), None, None, None) == binding.R1_EINVAL and f"variant {v}" in L.r1_last_error().decode(), v
        q = r1.make_params(p.width, p.height, p.spp, num_shards=2)
        assert L.r1_render_features(r._c, C.byref(q), None, None, None) == binding.R1_EINVAL and "num_shards" in L.r1_last_error().decode()
        assert L.r1_render_features(r._c, C.byref(p), None, None, None) == binding.R1_EINVAL and "no scene set" in L.r1_last_error().decode()
        assert L.r1_render_features_device(r._c, C.byref(p), None, None, None) == binding.R1_EINVAL and "no scene set" in L.r1_last_error().decode()
        sa = fc.scene("medium")
        r.set_scene_raw(lc.cscene(sa), lc.ccamera(sa))
        assert L.r1_render_features(r._c, C.byref(p), None, None, None) == binding.R1_EINVAL and "out is NULL" in L.r1_last_error().decode()
        expect_refusal(lambda: r.render_features(fc.params("medium", variant=binding.VARIANT_PREFILTER), out=out), "variant 2")
        assert (out.view(np.uint8) == fc.PREFILL).all()
        got, _ = r.render_features(p, out=out)
        assert got.tobytes() == fc.host_frame("medium").tobytes()
    finally:
        r.close()


# ---- what else the context holds --------------------------------------------------------------------------------------------------------------------


def test_a_feature_frame_leaves_the_contexts_state_alone(renderer):
    name = "medium"
    set_case(renderer, name)
    w, h, _ = fc.FRAMES[name]
    par = lambda spp: r1.make_params(w, h, spp, fc.SEED)  # noqa: E731
    want, want_rays, _ = renderer.render(par(4))
    # a progressive accumulation started before the call continues after it to the same bytes
    renderer.render_pass(par(2), 0)
    info = renderer.launch_info()
    timing = renderer.last_timing()
    got, _ = renderer.render_features(fc.params(name))
    assert got.tobytes() == fc.host_frame(name).tobytes()
    got, _ = renderer.render_features(fc.params(name, variant=binding.VARIANT_GRID), (5, 3, 21, 9))
    assert got.tobytes() == fc.crop(fc.host_frame(name), (5, 3, 21, 9)).tobytes()
    assert renderer.launch_info() == info and renderer.last_timing() == timing
    img, rays = renderer.render_pass(par(2), 2)
    assert img.tobytes() == want.tobytes() and rays == want_rays
    # a render before and after gives equal bytes
    again, again_rays, _ = renderer.render(par(4))
    assert again.tobytes() == want.tobytes() and again_rays == want_rays


# ---- moved scenes and cameras -------------------------------------------------------------------------------------------------------------------------


def test_after_an_update_the_frame_is_the_moved_scenes(renderer):
    w, h, spp = 64, 48, 2
    sc = r1.create_large_scene(w, h)
    a = sc.arrays()
    x, y, z = moved_centres(a, "jitter")
    renderer.set_scene(sc)
    renderer.regrid()  # (the grid is built before the update, so that r1_regrid can re-register the moved spheres in it)
    renderer.update_centers(0, x, y, z)
    cs, keep = raw_from_arrays(a, x, y, z)
    cam = sc.camera.contents
    p = lambda v: r1.make_params(w, h, spp, fc.SEED, variant=v)  # noqa: E731
    want = binding.render_features_host(cs, cam, p(0))
    still = binding.render_features_host(sc.spheres.contents, cam, p(0))
    assert want.tobytes() != still.tobytes()  # (the move shows in the frame)
    for vname in ("default", "bvh", "reference"):
        got, _ = renderer.render_features(p(fc.VARIANTS[vname]))
        assert got.tobytes() == want.tobytes(), (vname, mismatch(got, want))
    expect_refusal(lambda: renderer.render_features(p(binding.VARIANT_GRID)), "the scene has moved")
    renderer.regrid()
    got, _ = renderer.render_features(p(binding.VARIANT_GRID))
    assert got.tobytes() == want.tobytes(), ("grid, regridded", mismatch(got, want))
    renderer.resort_spheres()
    got, _ = renderer.render_features(p(binding.VARIANT_BVH))
    assert got.tobytes() == want.tobytes(), ("resorted", mismatch(got, want))


def test_after_set_camera_the_frame_follows_the_new_camera(renderer):
    name = "far"
    sa, cam2 = es.build(name, "small")
    renderer.set_scene_raw(lc.cscene(sa), lc.ccamera(sa))
    p = fc.params(name)
    got, _ = renderer.render_features(p)
    assert got.tobytes() == fc.host_frame(name).tobytes()
    renderer.set_camera(es.ccamera(cam2))
    want = binding.render_features_host(lc.cscene(sa), es.ccamera(cam2), p)
    assert want.tobytes() != fc.host_frame(name).tobytes()
    for vname, v in fc.VARIANTS.items():
        got, _ = renderer.render_features(fc.params(name, variant=v))
        assert got.tobytes() == want.tobytes(), (vname, mismatch(got, want))


def test_a_camera_without_a_finite_ray_gives_records_of_zeros_and_takes_no_walk(renderer):
    """every sample non-finite (the cast job's load rule): no walk, a record of zeros from each of the three loops"""
    from test_features_host import nan_camera
    name = "medium"
    sa = set_case(renderer, name)
    renderer.set_camera(nan_camera(sa))
    w, h, _ = fc.FRAMES[name]
    for vname, v in fc.VARIANTS.items():
        out = np.frombuffer(bytes([fc.PREFILL]) * (h * w * 32), binding.FEATURE_DTYPE).reshape(h, w).copy()
        got, _ = renderer.render_features(fc.params(name, variant=v), out=out)
        assert got is out and not got.view(np.uint8).any(), vname
    renderer.set_camera(lc.ccamera(sa))
    got, _ = renderer.render_features(fc.params(name))
    assert got.tobytes() == fc.host_frame(name).tobytes()


# ---- the drop-in program ---------------------------------------------------------------------------------------------------------------------------


def read_pfm(path, w, h):
    data = path.read_bytes()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 12, path
    return np.frombuffer(data[len(head):], np.float32).reshape(h, w, 3)


def test_program_features_writes_the_three_planes(renderer, tmp_path):
    w, h, spp = 40, 24, 3
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", str(w), "--height", str(h), "--spp", str(spp), "--features", "-w"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for name, make in lc.SCENES.items():
        renderer.set_scene(make(w, h))
        want, _ = renderer.render_features(r1.make_params(w, h, spp, 10001))
        assert read_pfm(tmp_path / f"out_{name}_albedo.pfm", w, h).tobytes() == want["albedo"].tobytes(), name
        assert read_pfm(tmp_path / f"out_{name}_normal.pfm", w, h).tobytes() == want["normal"].tobytes(), name
        assert read_pfm(tmp_path / f"out_{name}_depth.pfm", w, h).tobytes() == np.repeat(want["depth"][:, :, None], 3, axis=2).tobytes(), name
        line = [ln for ln in out.stdout.splitlines() if ln.startswith(f"{name} features:")]
        assert len(line) == 1 and f"{w * h} pixels" in line[0] and "device time" in line[0], (name, line)
        assert (tmp_path / f"out_{name}.tga").exists()
