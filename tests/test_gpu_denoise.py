"""GPU tests of denoised frames (include/rays1.h): r1_denoise_device and r1_denoise against the host form r1_denoise_host
(which tests/test_denoise_host.py holds to the contract's numpy form), byte for byte: frames of one pixel, of less than a kernel, across
workgroup tiles with clipped halos on all four edges, and large enough for whole step-16 kernels; every iteration count through the
LDS-staged and the direct passes; the ends of normal_power_log2; both flags; a torch tensor on a stream of its own; in place; strides and
sentinels; refusals; r1_render_denoised against the host composition for every variant; the context's state before and after; a moved
scene; the drop-in program's PFM file; and all three device forms, in place too, against the float64 truth of the contract's prose within
its derived bound (tests/filter_truth_cases.py) — the only test here with a bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import rays1bench_amd as r1
from rays1bench_amd import binding

import denoise_cases as dc
import feature_cases as fc
import filter_truth_cases as tc
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


def mismatch(got, want):
    """what differs, for the assertion's message"""
    bad = (np.asarray(got).view(np.uint32) != np.asarray(want).view(np.uint32)).any(axis=-1)
    return int(bad.sum()), np.argwhere(bad)[:4].tolist()


def on_device(a):
    """a numpy array's bytes in a float32 device tensor (a feature frame: eight words a pixel)"""
    a = np.ascontiguousarray(a)
    words = a.view(np.float32).reshape(a.shape[:2] + (-1,)) if a.dtype == binding.FEATURE_DTYPE else a
    return torch.from_numpy(words.copy()).cuda()


def device_denoise(rend, L, f, o, stream=None):
    """r1_denoise_device of host arrays through fresh device tensors; returns the result as numpy"""
    h, w = f.shape
    dL, df = on_device(L), on_device(f)
    dout = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rend.denoise_device(w, h, o, dL.data_ptr(), df.data_ptr(), dout.data_ptr(), stream_ptr=stream.cuda_stream if stream else None)
    (stream.synchronize() if stream else rend.sync())
    torch.cuda.synchronize()
    return dout.cpu().numpy()


# ---- both device forms against the host form ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(dc.SYNTHETIC) + list(dc.DEVICE_ONLY) + list(dc.RENDERED))
def test_both_device_forms_equal_the_host_form(renderer, name):
    """1 x 1; 5 x 3 with 4 iterations (every tap of the last pass off the image); 37 x 21, 70 x 40 with 5; 65 x 33 and 257 x 17, which cross
    workgroup tiles of 32 x 8 in x and y with halos clipped on all four edges; 150 x 141 with 5 iterations, whose interior pixels have all 25
    step-16 taps on the image"""
    L, f, it = dc.inputs(name)
    h, w = f.shape
    if name == "150x141":
        assert w >= 140 and h >= 140 and it == 5 and w - 2 * 32 > 0 and h - 2 * 32 > 0
    want = dc.host_result(name)
    got = device_denoise(renderer, L, f, dc.opt(iterations=it))
    assert got.tobytes() == want.tobytes(), (name, "device", mismatch(got, want))
    got, secs = renderer.denoise(L, f, dc.opt(iterations=it))
    assert got.tobytes() == want.tobytes(), (name, "host memory", mismatch(got, want))
    assert secs > 0


@pytest.mark.parametrize("name", tc.DEVICE_CASES)
def test_the_device_forms_are_the_float64_truth_within_the_bound(renderer, name):
    """r1_denoise_device out of place and with d_out == d_L, and r1_denoise, both flag values: max |out - truth| <= (32 + 2^k / 4) n u
    max |truth|, pixels without a hit carry L's bits, and the error is the host form's to the digit"""
    L, f, _ = tc.inputs(name)
    h, w = f.shape
    for flags in tc.FLAGS:
        o = tc.options(name, flags, guided=False)
        host = tc.check_against_truth(binding.denoise_host(L, f, o), name, flags, False, "r1_denoise_host")
        errs = {"r1_denoise_device": tc.check_against_truth(device_denoise(renderer, L, f, o), name, flags, False, "r1_denoise_device")}
        dL, df = on_device(L), on_device(f)
        torch.cuda.synchronize()
        renderer.denoise_device(w, h, o, dL.data_ptr(), df.data_ptr(), dL.data_ptr())
        renderer.sync()
        errs["in place"] = tc.check_against_truth(dL.cpu().numpy(), name, flags, False, "r1_denoise_device, d_out == d_L")
        errs["r1_denoise"] = tc.check_against_truth(renderer.denoise(L, f, o)[0], name, flags, False, "r1_denoise")
        assert all(e == host for e in errs.values()), (name, flags, host, errs)


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_every_iteration_count_through_the_staged_and_the_direct_passes(renderer, iterations):
    """steps 1 and 2 stage tile and halo in LDS, steps 4 .. 32 load their taps directly; the last pass of each count is the one that writes
    `out`, so both forms are also checked as the last pass"""
    L, f, _ = dc.inputs("70x40")
    for flags in (0, binding.DENOISE_DEMODULATE):
        want = dc.host_result("70x40", iterations=iterations, flags=flags)
        got = device_denoise(renderer, L, f, dc.opt(iterations=iterations, flags=flags))
        assert got.tobytes() == want.tobytes(), (iterations, flags, mismatch(got, want))


@pytest.mark.parametrize("k", [0, 6, 10])
def test_the_ends_of_the_normal_power(renderer, k):
    for name in ("70x40", "large"):
        L, f, _ = dc.inputs(name)
        for kw in (dict(normal_power_log2=k, iterations=3), dict(normal_power_log2=k, iterations=3, flags=0, sigma_color=1e-3, sigma_depth=1e3)):
            want = dc.host_result(name, **kw)
            got = device_denoise(renderer, L, f, dc.opt(**kw))
            assert got.tobytes() == want.tobytes(), (name, kw, mismatch(got, want))


def test_the_ends_of_every_other_option(renderer):
    L, f, _ = dc.inputs("37x21")
    for kw in (dict(iterations=8), dict(iterations=1, sigma_color=1e-30, sigma_depth=1e-30), dict(iterations=2, sigma_color=3e38, sigma_depth=3e38)):
        want = dc.host_result("37x21", **kw)
        got = device_denoise(renderer, L, f, dc.opt(**kw))
        assert got.tobytes() == want.tobytes(), (kw, mismatch(got, want))


# ---- a torch tensor on a stream of its own, in place, strides ------------------------------------------------------------------------------------


def test_on_a_torch_stream_followed_by_a_torch_operation_without_a_wait(renderer):
    name = "large"
    L, f, it = dc.inputs(name)
    h, w = f.shape
    want = dc.host_result(name)
    stream = torch.cuda.Stream()
    dL, df = on_device(L), on_device(f)
    dout = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        renderer.denoise_device(w, h, dc.opt(iterations=it), dL.data_ptr(), df.data_ptr(), dout.data_ptr(), stream_ptr=stream.cuda_stream)
        copy = dout.clone()  # no wait between the call and this: it must see the finished frame
    stream.synchronize()
    assert copy.cpu().numpy().tobytes() == want.tobytes()
    assert dL.cpu().numpy().tobytes() == L.tobytes()  # (L is read only)
    # in place: out == L, again on the stream, then twice in a row (the second filters the first's result: ordered by the stream)
    with torch.cuda.stream(stream):
        renderer.denoise_device(w, h, dc.opt(iterations=it), dL.data_ptr(), df.data_ptr(), dL.data_ptr(), stream_ptr=stream.cuda_stream)
        once = dL.clone()
        renderer.denoise_device(w, h, dc.opt(iterations=it), dL.data_ptr(), df.data_ptr(), dL.data_ptr(), stream_ptr=stream.cuda_stream)
    stream.synchronize()
    assert once.cpu().numpy().tobytes() == want.tobytes()
    assert dL.cpu().numpy().tobytes() == binding.denoise_host(want, f, dc.opt(iterations=it)).tobytes()


def test_in_place_on_host_memory(renderer):
    L, f, it = dc.inputs("70x40")
    buf = L.copy()
    got, _ = renderer.denoise(buf, f, dc.opt(iterations=it), out=buf)
    assert got is buf and buf.tobytes() == dc.host_result("70x40").tobytes()


def test_strides_and_sentinels(renderer):
    name = "65x33"
    L, f, it = dc.inputs(name)
    h, w = f.shape
    want = dc.host_result(name)
    # host memory: views of buffers whose rows are further apart, 0xA5 between them
    Lv, Lbuf = dc.strided(L, w + 3)
    fv, fbuf = dc.strided(f, w + 1)
    ov, obuf = dc.strided(np.zeros_like(L), w + 5)
    got, _ = renderer.denoise(Lv, fv, dc.opt(iterations=it), out=ov)
    assert got.tobytes() == want.tobytes() and (obuf[:, w:].view(np.uint8) == dc.PREFILL).all()
    # device memory: the same three pitches; L's and f's gaps hold NaN (a value read from there would spread), out's gaps a sentinel
    ls, fs, os_ = w + 3, w + 1, w + 5
    dL = torch.full((h, ls, 3), float("nan"), dtype=torch.float32, device="cuda")
    df = torch.full((h, fs, 8), float("nan"), dtype=torch.float32, device="cuda")
    dout = torch.full((h, os_, 3), -7.0, dtype=torch.float32, device="cuda")
    dL[:, :w] = on_device(L)
    df[:, :w] = on_device(f)
    torch.cuda.synchronize()
    renderer.denoise_device(w, h, dc.opt(iterations=it), dL.data_ptr(), df.data_ptr(), dout.data_ptr(), linear_stride=ls, feature_stride=fs, out_stride=os_)
    renderer.sync()
    out = dout.cpu().numpy()
    assert out[:, :w].tobytes() == want.tobytes(), mismatch(out[:, :w], want)
    assert (out[:, w:] == -7.0).all()
    # in place with a stride: the gaps of L stay NaN
    renderer.denoise_device(w, h, dc.opt(iterations=it), dL.data_ptr(), df.data_ptr(), dL.data_ptr(), linear_stride=ls, feature_stride=fs, out_stride=ls)
    renderer.sync()
    out = dL.cpu().numpy()
    assert out[:, :w].tobytes() == want.tobytes() and np.isnan(out[:, w:]).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------


def test_refusals_enqueue_nothing(renderer):
    L, f, it = dc.inputs("37x21")
    h, w = f.shape
    o = dc.opt(iterations=it)
    dL, df = on_device(np.concatenate([L, L[:, :1]], axis=1)), torch.zeros((h, w + 1, 8), dtype=torch.float32, device="cuda")  # (room behind the frame for the offsets)
    dout = torch.full((h, w + 1, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = dout.clone()
    Lb = r1.lib()
    call = lambda *a, **k: renderer.denoise_device(w, h, o, *a, **k)  # noqa: E731
    # a pointer off by four bytes: d_f needs 16; d_L and d_out off by two bytes
    expect_refusal(lambda: call(dL.data_ptr(), df.data_ptr() + 4, dout.data_ptr()), "d_f 16-byte aligned")
    expect_refusal(lambda: call(dL.data_ptr() + 2, df.data_ptr(), dout.data_ptr()), "4-byte aligned")
    expect_refusal(lambda: call(dL.data_ptr(), df.data_ptr(), dout.data_ptr() + 2), "4-byte aligned")
    for args, says in (((None, df.data_ptr(), dout.data_ptr()), "L is NULL"), ((dL.data_ptr(), None, dout.data_ptr()), "f is NULL"),
                       ((dL.data_ptr(), df.data_ptr(), None), "out is NULL")):
        expect_refusal(lambda: call(*args), says)
    # the frame and the options come before the pointers
    expect_refusal(lambda: renderer.denoise_device(w, h, dc.opt(iterations=9), None, None, None), "iterations")
    expect_refusal(lambda: renderer.denoise_device(w, h, o, None, None, None, out_stride=w - 1), "out_stride")
    expect_refusal(lambda: renderer.denoise_device(65536, 32768, o, dL.data_ptr(), df.data_ptr(), dout.data_ptr()), "2^31", binding.R1_ELIMIT)
    expect_refusal(lambda: renderer.denoise(L, f, dc.opt(sigma_depth=0.0)), "sigma_depth")
    assert Lb.r1_denoise(renderer._c, C.byref(binding.DenoiseFrame(w, h, 0, 0, 0)), C.byref(o), None, None, None, None) == binding.R1_EINVAL
    assert "L is NULL" in Lb.r1_last_error().decode()
    renderer.sync()
    torch.cuda.synchronize()
    assert torch.equal(dout, before)
    # off by four bytes is fine for d_L and d_out: the frame one float further on
    dL4 = torch.zeros(h * w * 3 + 1, dtype=torch.float32, device="cuda")
    dL4[1:] = on_device(L).reshape(-1)
    dF = on_device(f)
    out4 = torch.full((h * w * 3 + 1,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call(dL4.data_ptr() + 4, dF.data_ptr(), out4.data_ptr() + 4)
    renderer.sync()
    got = out4.cpu().numpy()
    assert got[0] == -7.0 and got[1:].tobytes() == dc.host_result("37x21").tobytes()


# ---- a frame rendered and denoised ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", dc.RENDERED)
def test_render_denoised_equals_the_host_composition_for_every_variant(renderer, name):
    sa = fc.scene(name)
    renderer.set_scene_raw(lc.cscene(sa), lc.ccamera(sa))
    want = dc.host_result(name)  # r1_denoise_host of r1_render_linear_host's and r1_render_features_host's frames
    w, h, _ = fc.FRAMES[name]
    for vname, v in fc.VARIANTS.items():
        p = fc.params(name, variant=v)
        _, rays, _ = renderer.render_linear(p)
        got, got_rays, secs = renderer.render_denoised(p, dc.opt())
        assert got.tobytes() == want.tobytes(), (name, vname, mismatch(got, want))
        assert secs > 0 and got_rays == rays  # the ray count is r1_render_linear's
        # the device form on a stream of torch's, the ray count beside the frame
        stream = torch.cuda.Stream()
        d = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
        d_rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            renderer.render_denoised_device(p, dc.opt(), d.data_ptr(), d_rays.data_ptr(), stream_ptr=stream.cuda_stream)
            copy = d.clone()
        stream.synchronize()
        assert copy.cpu().numpy().tobytes() == want.tobytes(), (name, vname, "device")
        assert int(d_rays.item()) == got_rays


def test_a_refused_variant_and_refused_options_enqueue_nothing(renderer):
    name = "medium"
    sa = fc.scene(name)
    renderer.set_scene_raw(lc.cscene(sa), lc.ccamera(sa))
    w, h, _ = fc.FRAMES[name]
    renderer.render(fc.params(name))
    info, timing = renderer.launch_info(), renderer.last_timing()
    d = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    d_rays = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for v in fc.REFUSED_VARIANTS:
        q = fc.params(name, variant=v)
        expect_refusal(lambda: renderer.render_denoised(q, dc.opt()), f"variant {v}")
        expect_refusal(lambda: renderer.render_denoised_device(q, dc.opt(), d.data_ptr(), d_rays.data_ptr()), f"variant {v}")
    p = fc.params(name)
    expect_refusal(lambda: renderer.render_denoised(p, dc.opt(iterations=0)), "iterations")
    expect_refusal(lambda: renderer.render_denoised_device(p, dc.opt(normal_power_log2=11), d.data_ptr(), d_rays.data_ptr()), "normal_power_log2")
    expect_refusal(lambda: renderer.render_denoised_device(p, dc.opt(), d.data_ptr() + 2, d_rays.data_ptr()), "aligned")
    expect_refusal(lambda: renderer.render_denoised_device(p, dc.opt(), d.data_ptr(), d_rays.data_ptr() + 4), "aligned")
    expect_refusal(lambda: renderer.render_denoised_device(p, dc.opt(), None, d_rays.data_ptr()), "d_rgb_f32")
    expect_refusal(lambda: renderer.render_denoised(r1.make_params(w, h, 3, num_shards=2), dc.opt()), "num_shards")
    renderer.sync()
    torch.cuda.synchronize()
    assert (d == -7.0).all() and int(d_rays.item()) == -7
    assert renderer.launch_info() == info and renderer.last_timing() == timing
    # a context without a scene: the options are named first, then the missing scene
    r = r1.Renderer(0)
    try:
        expect_refusal(lambda: r.render_denoised(p, dc.opt(flags=2)), "flags")
        expect_refusal(lambda: r.render_denoised(p, dc.opt()), "no scene set")
        # a denoise needs no scene
        L, f, it = dc.inputs("37x21")
        got, _ = r.denoise(L, f, dc.opt(iterations=it))
        assert got.tobytes() == dc.host_result("37x21").tobytes()
    finally:
        r.close()


def test_a_progressive_accumulation_and_the_launch_info_survive_a_denoise(renderer):
    name = "medium"
    sa = fc.scene(name)
    renderer.set_scene_raw(lc.cscene(sa), lc.ccamera(sa))
    w, h, _ = fc.FRAMES[name]
    par = lambda spp: r1.make_params(w, h, spp, fc.SEED)  # noqa: E731
    want, want_rays, _ = renderer.render(par(4))
    renderer.render_pass(par(2), 0)
    info, timing = renderer.launch_info(), renderer.last_timing()
    L, f, it = dc.inputs("70x40")
    got, _ = renderer.denoise(L, f, dc.opt(iterations=it))
    assert got.tobytes() == dc.host_result("70x40").tobytes()
    assert device_denoise(renderer, L, f, dc.opt(iterations=it)).tobytes() == dc.host_result("70x40").tobytes()
    assert renderer.launch_info() == info and renderer.last_timing() == timing
    img, rays = renderer.render_pass(par(2), 2)
    assert img.tobytes() == want.tobytes() and rays == want_rays


def test_after_an_update_the_denoised_render_follows_the_moved_scene(renderer):
    w, h, spp = 64, 48, 2
    sc = r1.create_large_scene(w, h)
    a = sc.arrays()
    x, y, z = moved_centres(a, "jitter")
    renderer.set_scene(sc)
    p = r1.make_params(w, h, spp, fc.SEED)
    cam = sc.camera.contents
    still = binding.denoise_host(binding.render_linear_host(sc.spheres.contents, cam, p)[0], binding.render_features_host(sc.spheres.contents, cam, p), dc.opt())
    got, _, _ = renderer.render_denoised(p, dc.opt())
    assert got.tobytes() == still.tobytes()
    renderer.update_centers(0, x, y, z)
    cs, keep = raw_from_arrays(a, x, y, z)
    want = binding.denoise_host(binding.render_linear_host(cs, cam, p)[0], binding.render_features_host(cs, cam, p), dc.opt())
    assert want.tobytes() != still.tobytes()  # (the move shows in the frame)
    for vname in ("default", "bvh", "reference"):
        q = r1.make_params(w, h, spp, fc.SEED, variant=fc.VARIANTS[vname])
        got, _, _ = renderer.render_denoised(q, dc.opt())
        assert got.tobytes() == want.tobytes(), (vname, mismatch(got, want))


# ---- the drop-in program ---------------------------------------------------------------------------------------------------------------------------


def read_pfm(path, w, h):
    data = path.read_bytes()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert data.startswith(head) and len(data) == len(head) + w * h * 12, path
    return np.frombuffer(data[len(head):], np.float32).reshape(h, w, 3)


def test_program_denoise_writes_the_denoised_frame_next_to_the_noisy_one(renderer, tmp_path):
    w, h, spp = 40, 24, 3
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", str(w), "--height", str(h), "--spp", str(spp), "--denoise", "2", "-w"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for name, make in lc.SCENES.items():
        renderer.set_scene(make(w, h))
        p = r1.make_params(w, h, spp, 10001)
        want, _, _ = renderer.render_denoised(p, dc.opt(iterations=2))
        assert read_pfm(tmp_path / f"out_{name}_denoised.pfm", w, h).tobytes() == want.tobytes(), name
        noisy = read_pfm(tmp_path / f"out_{name}.pfm", w, h)
        assert noisy.tobytes() != want.tobytes()
        line = [ln for ln in out.stdout.splitlines() if ln.startswith(f"{name} denoise:")]
        assert len(line) == 1 and "2 iterations" in line[0] and "device time" in line[0], (name, line)
