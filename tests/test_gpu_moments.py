"""GPU tests of variance frames (include/rays1.h): r1_render_moments and r1_render_moments_device return r1_render_linear's
frame and ray count and, per pixel, the record r1_render_moments_host returns — which tests/test_moments_host.py pins to the contract
restated on the oracle's records.  Every such expectation is BYTE FOR BYTE.  Against float64 (tests/moment_cases.py): the
device's variances within the derived bound of the plain statistic on the records r1_render_samples returns for the same params, and the
ratio over 48 seeds that says the estimate is unbiased and of the mean — the only two tests here with a bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import rays1bench_amd as r1
from rays1bench_amd import binding

import linear_cases as lc
import moment_cases as mc
from test_refit_host import moved_centres, raw_from_arrays

pytestmark = pytest.mark.gpu

V = binding
VARIANTS = {"default": V.VARIANT_DEFAULT, "bvh": V.VARIANT_BVH, "grid": V.VARIANT_GRID, "reference": V.VARIANT_REFERENCE, "prefilter": V.VARIANT_PREFILTER}


@pytest.fixture()
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def device_frame(renderer, p, stream=None):
    """r1_render_moments_device into tensors prefilled with NaN bits: (L, moments, ray count) on the host"""
    h, w = p.height, p.width
    frame = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    mom = torch.full((h, w, 4), -1, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    renderer.render_moments_device(p, frame.data_ptr(), mom.data_ptr(), count.data_ptr(), stream.cuda_stream if stream else None)
    (stream.synchronize() if stream else renderer.sync())
    return frame.cpu().numpy(), mom.cpu().numpy().view(binding.MOMENT_DTYPE).reshape(h, w), int(count.item())


def expect_refusal(fn, text=None, code=binding.R1_EINVAL):
    with pytest.raises(binding.R1Error) as e:
        fn()
    assert e.value.code == code, e.value
    if text:
        assert text in str(e.value), e.value


@pytest.mark.parametrize("name,w,h,spp", lc.FRAMES, ids=lambda v: str(v))
def test_both_device_forms_are_the_host_form_whatever_the_tiles(renderer, name, w, h, spp):
    renderer.set_scene(lc.SCENES[name](w, h))
    want_L, want, want_rays = mc.host_frame(name, w, h, spp)
    for tw, th in lc.TILES:  # 40 x 24 and 16 x 8 leave ragged edge tiles on every frame
        p = r1.make_params(w, h, spp, lc.SEED, tile_w=tw, tile_h=th)
        lin, mom, rays, secs = renderer.render_moments(p)
        assert rays == want_rays and secs > 0, (tw, th)
        assert lc.same_bits(lin, want_L), (tw, th, mc.differing(lin, want_L))
        assert mc.same_records(mom, want), (tw, th, mc.differing(mom["var"], want["var"]))
        lin_d, mom_d, rays_d = device_frame(renderer, p)
        assert rays_d == want_rays, (tw, th)
        assert lc.same_bits(lin_d, want_L) and mc.same_records(mom_d, want), (tw, th, mc.differing(mom_d["var"], want["var"]))
    plain, plain_rays, _ = renderer.render_linear(r1.make_params(w, h, spp, lc.SEED))
    assert plain_rays == want_rays and lc.same_bits(plain, want_L)


@pytest.mark.parametrize("name,w,h,spp", [fr for fr in lc.FRAMES if fr[3] > 1] + [("large", 24, 15, 64), ("medium", 24, 15, 2)], ids=lambda v: str(v))
def test_both_device_forms_are_the_float64_variance_of_the_mean_of_the_devices_own_records(renderer, name, w, h, spp):
    """var against x.var(ddof=1) / n in float64 of the records r1_render_samples returns for the same params:
    |var - truth| <= (2n + 8) u truth + n^2 / (n - 1) u^2 L64^2"""
    renderer.set_scene(lc.SCENES[name](w, h))
    p = r1.make_params(w, h, spp, lc.SEED)
    _, rays, samples = renderer.render_samples(p)
    rec = samples.reshape(h, w, spp, 4)
    lin, mom, got_rays, _ = renderer.render_moments(p)
    assert got_rays == rays
    assert np.abs(lin.astype(np.float64) - mc.truth_variance(rec)[1]).max() <= (spp + 1) * 2.0 ** -24 * np.abs(rec[..., :3]).max()  # (the records are this frame's)
    a = mc.check_variance(mom, rec, f"r1_render_moments {name} {w}x{h}")
    _, mom_d, _ = device_frame(renderer, p)
    b = mc.check_variance(mom_d, rec, f"r1_render_moments_device {name} {w}x{h}")
    assert a == b


@pytest.mark.parametrize("n", mc.SEEDS_SPP)
def test_the_estimate_is_unbiased_and_of_the_mean_over_48_seeds(renderer, n):
    """R = sum var_over_seeds(L) / sum mean_over_seeds(var) from r1_render_moments' frames: nearer to 1 than to n / (n - 1)"""
    name, w, h = mc.SEEDS_FRAME
    renderer.set_scene(lc.SCENES[name](w, h))
    frames = [renderer.render_moments(r1.make_params(w, h, n, seed))[:2] for seed in mc.SEEDS]
    R = mc.seeds_ratio(frames)
    print(f"{name} {w}x{h}x{n}, {len(mc.SEEDS)} seeds: R = {R:.4f}, band {np.exp(mc.seeds_band(n)):.4f}")
    assert abs(np.log(R)) < mc.seeds_band(n)


@pytest.mark.parametrize("vname", sorted(VARIANTS))
def test_every_variant_gives_the_same_records_and_the_linear_frames_count(renderer, vname):
    name, w, h, spp = "medium", 77, 45, 3
    renderer.set_scene(lc.SCENES[name](w, h))
    want_L, want, want_rays = mc.host_frame(name, w, h, spp)
    p = r1.make_params(w, h, spp, lc.SEED, variant=VARIANTS[vname])
    lin, mom, rays, _ = renderer.render_moments(p)
    info, timing = renderer.launch_info(), renderer.last_timing()
    assert lc.same_bits(lin, want_L) and mc.same_records(mom, want) and rays == want_rays
    plain, plain_rays, _ = renderer.render_linear(p)
    assert plain_rays == rays and lc.same_bits(plain, lin)
    assert renderer.launch_info() == info  # the same launch describes both
    assert timing is not None
    lin_d, mom_d, rays_d = device_frame(renderer, p)
    assert lc.same_bits(lin_d, want_L) and mc.same_records(mom_d, want) and rays_d == want_rays


def test_device_form_into_tensors_on_a_stream_of_its_own_two_calls_one_wait(renderer):
    name, w, h, spp = "large", 200, 100, 4
    renderer.set_scene(lc.SCENES[name](w, h))
    frame = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    mom = torch.full((h, w, 4), -1, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    renderer.render_moments_device(r1.make_params(w, h, spp, 4242), frame.data_ptr(), mom.data_ptr(), count.data_ptr(), stream.cuda_stream)
    renderer.render_moments_device(r1.make_params(w, h, spp, lc.SEED), frame.data_ptr(), mom.data_ptr(), count.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    want_L, want, want_rays = mc.host_frame(name, w, h, spp)
    got = mom.cpu().numpy().view(binding.MOMENT_DTYPE).reshape(h, w)
    assert lc.same_bits(frame.cpu().numpy(), want_L) and mc.same_records(got, want) and int(count.item()) == want_rays


def test_pixel_mode_switched_on_still_keeps_the_records(renderer):
    name, w, h, spp = "medium", 33, 33, 7
    renderer.set_scene(lc.SCENES[name](w, h))
    renderer.set_pixel_mode(1)
    want_L, want, want_rays = mc.host_frame(name, w, h, spp)
    lin, mom, rays = device_frame(renderer, r1.make_params(w, h, spp, lc.SEED))
    assert lc.same_bits(lin, want_L) and mc.same_records(mom, want) and rays == want_rays
    lin, mom, rays, _ = renderer.render_moments(r1.make_params(w, h, spp, lc.SEED))
    assert lc.same_bits(lin, want_L) and mc.same_records(mom, want) and rays == want_rays


def test_after_update_centers_the_records_are_those_of_the_moved_scene(renderer):
    w, h, spp = 64, 40, 3
    sc = r1.create_large_scene(w, h)
    a = sc.arrays()
    x, y, z = moved_centres(a, "permute")
    renderer.set_scene(sc)
    renderer.update_centers(0, x, y, z)
    p = r1.make_params(w, h, spp, 777)
    lin, mom, rays, _ = renderer.render_moments(p)
    cs, _keep = raw_from_arrays(a, x, y, z)
    want_L, want, want_rays = binding.render_moments_host(cs, sc.camera.contents, p)
    assert rays == want_rays and lc.same_bits(lin, want_L) and mc.same_records(mom, want)
    lin_d, mom_d, rays_d = device_frame(renderer, p)
    assert rays_d == want_rays and lc.same_bits(lin_d, want_L) and mc.same_records(mom_d, want)


def test_a_progressive_accumulation_survives_and_refusals_enqueue_nothing(renderer):
    name, w, h = "small", 64, 48
    L = r1.lib()
    fresh = r1.Renderer(0)
    p = r1.make_params(w, h, 2, lc.SEED)
    try:  # before r1_set_scene
        expect_refusal(lambda: fresh.render_moments(p), "no scene")
    finally:
        fresh.close()
    renderer.set_scene(lc.SCENES[name](w, h))
    renderer.render_pass(p, 0, image=False)  # a running accumulation of 2 samples
    info = renderer.launch_info()
    out = np.zeros((h, w, 3), np.float32)
    mom = np.zeros((h, w), binding.MOMENT_DTYPE)
    fp, mp, rays = out.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(mom.ctypes.data), C.c_uint64()
    two = r1.make_params(w, h, 2, lc.SEED, shard=0, num_shards=2)
    c = renderer._c
    dev = torch.full((w * h * 3,), 0.5, dtype=torch.float32, device="cuda")
    dmom = torch.full((w * h * 4 + 4,), 9, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    calls = [(lambda: L.r1_render_moments(c, C.byref(two), fp, mp, C.byref(rays), None), "num_shards"),
             (lambda: L.r1_render_moments_device(c, C.byref(two), dev.data_ptr(), dmom.data_ptr(), cnt.data_ptr(), None), "num_shards"),
             (lambda: L.r1_render_moments(c, C.byref(p), None, mp, C.byref(rays), None), "null"),
             (lambda: L.r1_render_moments(c, C.byref(p), fp, None, C.byref(rays), None), "null"),
             (lambda: L.r1_render_moments(c, None, fp, mp, C.byref(rays), None), "null"),
             (lambda: L.r1_render_moments_device(c, C.byref(p), None, dmom.data_ptr(), cnt.data_ptr(), None), "null"),
             (lambda: L.r1_render_moments_device(c, C.byref(p), dev.data_ptr(), None, cnt.data_ptr(), None), "null"),
             (lambda: L.r1_render_moments_device(c, C.byref(p), dev.data_ptr(), dmom.data_ptr(), None, None), "null"),
             (lambda: L.r1_render_moments_device(c, C.byref(p), dev.data_ptr() + 2, dmom.data_ptr(), cnt.data_ptr(), None), "aligned"),
             (lambda: L.r1_render_moments_device(c, C.byref(p), dev.data_ptr(), dmom.data_ptr() + 8, cnt.data_ptr(), None), "d_moments must be 16-byte aligned"),
             (lambda: L.r1_render_moments_device(c, C.byref(p), dev.data_ptr(), dmom.data_ptr(), cnt.data_ptr() + 4, None), "aligned")]
    for k, (call, text) in enumerate(calls):
        assert call() == binding.R1_EINVAL, k
        assert text in L.r1_last_error().decode(), (k, L.r1_last_error())
        assert renderer.launch_info() == info, k
    torch.cuda.synchronize()
    assert not out.any() and not mom.view(np.uint32).any()
    assert bool((dev == 0.5).all()) and bool((dmom == 9).all()) and bool((cnt == 5).all())
    # the accumulation survived every refusal — and a variance frame, which is no refusal: it continues at 2 and ends as the 5-sample frame
    lin, got, _, _ = renderer.render_moments(r1.make_params(w, h, 3, 99))
    assert (got["samples"] == 3).all()
    img, total = renderer.render_pass(r1.make_params(w, h, 3, lc.SEED), 2)
    want = renderer.render(r1.make_params(w, h, 5, lc.SEED))
    assert total == want[1] and img.tobytes() == want[0].tobytes()
