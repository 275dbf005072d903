"""GPU tests of accumulated frames (include/rays1.h): r1_accumulate_device and r1_accumulate return r1_accumulate_host's two
images — which tests/test_accumulate_host.py pins to the contract restated in numpy — byte for byte, and r1_render_accumulated* the host
composition's frames along a camera path, under the history rules: every sentence of the composed form's paragraph in the header has a test
here.  One bound: the device forms against the reprojection computed in float64 (tests/reproject_truth_cases.py), the tolerance worked
out there; everything else is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rays1bench_amd as r1
from rays1bench_amd import binding

import accumulate_cases as ac
import denoise_cases as dc
import guided_cases as gc
import linear_cases as lc
import reproject_truth_cases as rt
from test_gpu_update import MOVED_RULE
from test_gpu_update_spheres import edited, material_family
from test_refit_host import moved_centres, raw_from_arrays
from test_update_spheres_host import radius_family

pytestmark = pytest.mark.gpu

WORDS = (3, 4, 8, 3, 8, 4, 3, 4)  # of a pixel of L, V, f, A_prev, f_prev, M_prev, A_out, M_out


@pytest.fixture()
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def words(a):
    """a frame as int32 words (h, w, k), a writable copy"""
    a = np.array(a)
    return a.view(np.int32).reshape(a.shape[0], a.shape[1], -1)


def unwords(A, M):
    """the two output tensors as (float32 (h, w, 3), MOMENT_DTYPE (h, w))"""
    A, M = A.cpu().numpy(), M.cpu().numpy()
    return A.view(np.float32), np.ascontiguousarray(M).view(binding.MOMENT_DTYPE).reshape(M.shape[:2])


def device_result(renderer, frames, view, o, in_place=False, stream=None, pitches=None):
    """r1_accumulate_device on tensors holding the six frames; the outputs are prefilled with 0x7FC00000 (a NaN, and 2 143 289 344 samples).
    pitches: eight row pitches in pixels, the words between the rows of the inputs NaN"""
    h, w = frames[0].shape[:2]
    pitches = pitches or (w,) * 8
    fill = 0x7FC00000
    t = []
    for a, k, pitch in zip(frames, WORDS, pitches):
        buf = torch.full((h, pitch, k), fill, dtype=torch.int32, device="cuda")
        buf[:, :w] = torch.from_numpy(words(a)).cuda()
        t.append(buf)
    if in_place:
        t += [t[0], t[1]]
    else:
        t += [torch.full((h, pitches[6], 3), fill, dtype=torch.int32, device="cuda"), torch.full((h, pitches[7], 4), fill, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    strides = None if all(p == w for p in pitches) else ((pitches[0], pitches[1]) + tuple(pitches[2:6]) + ((pitches[0], pitches[1]) if in_place else tuple(pitches[6:])))
    renderer.accumulate_device(w, h, view, o, *[x.data_ptr() for x in t], stream_ptr=stream, strides=strides)
    return t


def fetch(renderer, t, w):
    renderer.sync()
    A, M = unwords(t[6][:, :w].contiguous(), t[7][:, :w].contiguous())
    return A, M


def check_both_forms(renderer, frames, view, want, o=None, tag=None):
    o = o or ac.opt()
    w = frames[0].shape[1]
    got = fetch(renderer, device_result(renderer, frames, view, o), w)
    assert ac.same(got, want), (tag, "device")
    A, M, secs = renderer.accumulate(*frames, view, o)
    assert ac.same((A, M), want) and secs > 0, (tag, "host memory")


@pytest.mark.parametrize("how", ["seeds", "orbit"])
@pytest.mark.parametrize("name", sorted(ac.RENDERED))
def test_both_device_forms_are_the_host_form_on_rendered_pairs(renderer, name, how):
    frames, view = ac.rendered_inputs(name, how)
    check_both_forms(renderer, frames, view, ac.host_result("rendered", name, how), tag=(name, how))


@pytest.mark.parametrize("name", sorted(ac.SYNTHETIC) + ["150x141"])
def test_both_device_forms_are_the_host_form_under_every_camera_pair(renderer, name):
    for pair in ac.PAIRS:
        frames, view = ac.synthetic_inputs(name, pair)
        check_both_forms(renderer, frames, view, ac.host_result("synthetic", name, pair), tag=(name, pair))


@pytest.mark.parametrize("name", ["65x33", "257x17"])
def test_tiles_crossed_in_x_and_y(renderer, name):
    for pair in ("identical", "left", "zoom"):
        frames, view = ac.synthetic_inputs(name, pair)
        check_both_forms(renderer, frames, view, ac.host_result("synthetic", name, pair), tag=(name, pair))


def test_synthetic_frames_under_two_rotated_cameras(renderer):
    """the guard classes of the synthetic frames through a previous camera that is not axis-aligned: host form, numpy and both device forms"""
    name, pair = ac.ROTATED_AT, ac.ROTATED_PAIR
    frames, view = ac.synthetic_inputs(name, pair)
    for options in sorted(ac.OPTION_SETS):
        o = ac.opt(**ac.OPTION_SETS[options])
        want = ac.host_result("synthetic", name, pair, options)
        assert ac.same(ac.numpy_accumulate(*frames, view, o), want), options
        check_both_forms(renderer, frames, view, want, o, tag=(name, pair, options))
        assert ac.same(fetch(renderer, device_result(renderer, frames, view, o, in_place=True), frames[0].shape[1]), want), (options, "in place")


@functools.lru_cache(maxsize=None)
def truth_host_result(size, prev):
    """r1_accumulate_host of a case of reproject_truth_cases, read-only"""
    c = rt.case(size, prev)
    A, M = binding.accumulate_host(*c["frames"], c["view"], c["opt"])
    A.setflags(write=False), M.setflags(write=False)
    return A, M


@pytest.mark.parametrize("size,prev", rt.CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_every_device_form_looks_where_float64_geometry_says(renderer, size, prev):
    """tests/reproject_truth_cases.py: the history is the ramp (x, y, 1), so A_out is where the kernel looked; against the plane's point
    projected through the previous camera in float64, within 32 * 2^-24 * max(w, h) pixels (the fp32 restatement measures at most 6.53 of
    those units), and bit for bit the host form."""
    c = rt.case(size, prev)
    frames, view, o, w = c["frames"], c["view"], c["opt"], c["size"][0]
    want = truth_host_result(size, prev)
    for in_place in (False, True):
        got = fetch(renderer, device_result(renderer, frames, view, o, in_place=in_place), w)
        err = rt.check_against_truth(c, got, (size, prev, "device", in_place))
        assert ac.same(got, want), (size, prev, "device", in_place)
    A, M, _ = renderer.accumulate(*frames, view, o)
    rt.check_against_truth(c, (A, M), (size, prev, "host memory"))
    print(f"{size} {prev}: {err:.2f} x 2^-24 max(w, h) px over {c['compared'].mean():.3f} of the frame")
    check_both_forms(renderer, frames, view, want, o, tag=(size, prev))


@pytest.mark.parametrize("options", sorted(ac.OPTION_SETS))
def test_option_sets(renderer, options):
    for name, pair in (("37x21", "identical"), ("70x40", "zoom")):
        frames, view = ac.synthetic_inputs(name, pair)
        check_both_forms(renderer, frames, view, ac.host_result("synthetic", name, pair, options), ac.opt(**ac.OPTION_SETS[options]), tag=(name, pair, options))


def test_strides_with_nan_between_the_rows_of_every_input(renderer):
    name, pair = "37x21", "right"
    frames, view = ac.synthetic_inputs(name, pair)
    w = frames[0].shape[1]
    pitches = tuple(w + 1 + k for k in range(8))
    t = device_result(renderer, frames, view, ac.opt(), pitches=pitches)
    got = fetch(renderer, t, w)
    assert ac.same(got, ac.host_result("synthetic", name, pair))
    assert bool((t[6][:, w:] == 0x7FC00000).all()) and bool((t[7][:, w:] == 0x7FC00000).all())  # nothing between the rows is written


def test_in_place_and_on_a_torch_stream_of_its_own_followed_by_a_torch_operation(renderer):
    name, pair = "150x141", "zoom"
    frames, view = ac.synthetic_inputs(name, pair)
    want = ac.host_result("synthetic", name, pair)
    w = frames[0].shape[1]
    assert ac.same(fetch(renderer, device_result(renderer, frames, view, ac.opt(), in_place=True), w), want)  # A_out = L, M_out = V
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = device_result(renderer, frames, view, ac.opt(), stream=stream.cuda_stream)
        doubled = t[6] * 2  # (ordered behind the kernel by the stream alone: no wait in between)
    stream.synchronize()
    A, M = unwords(t[6], t[7])
    assert ac.same((A, M), want)
    assert doubled.cpu().numpy().tobytes() == (words(want[0]) * 2).tobytes()


def test_refusals_enqueue_nothing_and_leave_the_launch_info_as_it_was(renderer):
    w, h = 64, 48
    Lb = r1.lib()
    renderer.set_scene(lc.SCENES["small"](w, h))
    p = r1.make_params(w, h, 2, lc.SEED)
    renderer.render_pass(p, 0, image=False)
    info = renderer.launch_info()
    frames, view = ac.synthetic_inputs("37x21", "identical")
    fw, fh = 37, 21
    t = [torch.full((fh, fw, k), 5, dtype=torch.int32, device="cuda") for k in WORDS]
    cnt = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptrs = [x.data_ptr() for x in t]
    fr = binding.AccumulateFrame(fw, fh, 0, 0, 0, 0, 0, 0, 0, 0)
    c, o, go = renderer._c, ac.opt(), gc.opt()

    def device(images, opt=o, v=view, frame=fr):
        im = binding.AccumulateImages(*images)
        return Lb.r1_accumulate_device(c, C.byref(frame), C.byref(opt), C.byref(v), C.byref(im), None)

    def swapped(k, value):
        images = list(ptrs)
        images[k] = value
        return images

    flat = ac.view_of(view.camera, view.camera_prev, 4, 3)
    flat.camera_prev.w = (C.c_float * 3)(0, 0, 0)
    flat.camera_prev.lower_left = flat.camera_prev.origin
    calls = [lambda: device(swapped(0, None)), lambda: device(swapped(7, None)), lambda: device(swapped(0, ptrs[0] + 2)), lambda: device(swapped(1, ptrs[1] + 4)),
             lambda: device(swapped(2, ptrs[2] + 8)), lambda: device(swapped(5, ptrs[5] + 4)), lambda: device(swapped(7, ptrs[7] + 8)),
             lambda: device(swapped(6, ptrs[3])), lambda: device(swapped(7, ptrs[5])), lambda: device(swapped(7, ptrs[4])),  # overlapping history
             lambda: device(ptrs, opt=ac.opt(max_samples=0)), lambda: device(ptrs, v=flat),
             lambda: device(ptrs, frame=binding.AccumulateFrame(fw, fh, 0, 0, 0, 0, 0, 3, 0, 0)),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(p), C.byref(o), None, None, cnt.data_ptr(), None),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(p), C.byref(o), None, ptrs[0] + 2, cnt.data_ptr(), None),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(p), C.byref(o), None, ptrs[0], cnt.data_ptr() + 4, None),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(p), None, None, ptrs[0], cnt.data_ptr(), None),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(p), C.byref(ac.opt(flags=1)), None, ptrs[0], cnt.data_ptr(), None),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(p), C.byref(o), C.byref(gc.opt(variance_floor=0.0)), ptrs[0], cnt.data_ptr(), None),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(r1.make_params(w, h, 1, lc.SEED)), C.byref(o), C.byref(go), ptrs[0], cnt.data_ptr(), None),
             lambda: Lb.r1_render_accumulated_device(c, C.byref(r1.make_params(w, h, 2, lc.SEED, variant=binding.VARIANT_PREFILTER)), C.byref(o), None, ptrs[0],
                                                     cnt.data_ptr(), None)]
    for k, call in enumerate(calls):
        assert call() == binding.R1_EINVAL, (k, Lb.r1_last_error())
        assert renderer.launch_info() == info, k
    with pytest.raises(binding.R1Error) as e:  # spp 1 with a filter is refused ...
        renderer.render_accumulated(r1.make_params(w, h, 1, lc.SEED), o, go)
    assert e.value.code == binding.R1_EINVAL and "spp" in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((x == 5).all()) for x in t) and bool((cnt == 5).all())
    # an accumulation of caller-held images is a query: the progressive accumulation continues at 2 and ends as the 5-sample frame
    check_both_forms(renderer, frames, view, ac.host_result("synthetic", "37x21", "identical"))
    assert renderer.launch_info() == info
    img, total = renderer.render_pass(r1.make_params(w, h, 3, lc.SEED), 2)
    want = renderer.render(r1.make_params(w, h, 5, lc.SEED))
    assert total == want[1] and img.tobytes() == want[0].tobytes()


# ---- the composed, stateful form ---------------------------------------------------------------------------------------------------------------


def host_path(cs, cams, w, h, spp, seeds, go=None, o=None):
    """[(frame that goes out, ray count)] of the host composition along `cams`: r1_render_moments_host + r1_render_features_host +
    r1_accumulate_host against the frame before (+ r1_denoise_guided_host of the accumulated frame)"""
    return [(s["out"], s["rays"]) for s in host_steps(cs, cams, w, h, spp, seeds, go, o)]


def per_frame(v, n):
    """v for each of n frames: a list or tuple holds one value a frame, anything else is every frame's"""
    if isinstance(v, (list, tuple)):
        assert len(v) == n
        return list(v)
    return [v] * n


def host_steps(cs, cams, w, h, spp, seeds, go=None, o=None):
    """host_path with its parts: one dict a frame — out (what goes out), rays, L, V, f (the frame's own renders), A, M (the history it
    leaves), passed (True where the frame passed through).  cs, w, h, spp and go may be lists with one value a frame.  The rules of the
    composed form as the header states them: the history is empty at the first frame and where the size changed; a previous camera the
    plan refuses passes the frame through; spp_prev is the spp of the frame before; the history is the unfiltered accumulation."""
    o = o or ac.opt()
    n = len(cams)
    steps, A, M, fp, cam_p, spp_p, size_p = [], None, None, None, None, None, None
    for cam, seed, cs_k, w_k, h_k, spp_k, go_k in zip(cams, seeds, per_frame(cs, n), per_frame(w, n), per_frame(h, n), per_frame(spp, n), per_frame(go, n)):
        p = r1.make_params(w_k, h_k, spp_k, seed)
        L, V, rays = binding.render_moments_host(cs_k, cam, p)
        f = binding.render_features_host(cs_k, cam, p)
        passed = A is None or size_p != (w_k, h_k)
        if not passed:
            view = ac.view_of(cam, cam_p, spp_k, spp_p)
            try:
                binding.accumulate_check(binding.AccumulateFrame(w_k, h_k, 0, 0, 0, 0, 0, 0, 0, 0), o, view)
            except binding.R1Error:
                passed = True
        if passed:
            A, M = L, V
        else:
            A, M = binding.accumulate_host(L, V, f, A, fp, M, view, o)
        fp, cam_p, spp_p, size_p = f, cam, spp_k, (w_k, h_k)
        steps.append({"out": binding.denoise_guided_host(A, f, M, go_k) if go_k is not None else A, "rays": rays, "L": L, "V": V, "f": f, "A": A, "M": M,
                      "passed": passed})
    return steps


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("filtered", [False, True], ids=["accumulated", "accumulated_and_filtered"])
@pytest.mark.parametrize("name,w,h,spp", [("medium", 33, 17, 2), ("large", 40, 24, 2)], ids=lambda v: str(v))
def test_render_accumulated_is_the_host_composition_along_a_camera_path(renderer, name, w, h, spp, filtered):
    sc = lc.SCENES[name](w, h)
    cams = binding.orbit_cameras(sc, 64)[:4]
    seeds = [lc.SEED + k for k in range(4)]
    go = gc.opt() if filtered else None
    want = host_path(sc.spheres.contents, cams, w, h, spp, seeds, go)
    for variant in (binding.VARIANT_DEFAULT, binding.VARIANT_BVH, binding.VARIANT_GRID, binding.VARIANT_REFERENCE):
        renderer.set_scene(sc)  # (the history is empty again)
        for k, cam in enumerate(cams):
            renderer.set_camera(cam)
            img, rays, secs = renderer.render_accumulated(r1.make_params(w, h, spp, seeds[k], variant=variant), ac.opt(), go)
            assert rays == want[k][1] and secs > 0 and differing(img, want[k][0]) == 0, (variant, k, differing(img, want[k][0]))
    # the device form on a stream of its own, the same path
    renderer.accumulate_reset()
    frame = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k, cam in enumerate(cams):
        renderer.set_camera(cam)
        renderer.render_accumulated_device(r1.make_params(w, h, spp, seeds[k]), ac.opt(), go, frame.data_ptr(), count.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert differing(frame.cpu().numpy(), want[k][0]) == 0 and int(count.item()) == want[k][1], k
    assert renderer.launch_info()["samples"] > 0  # the state left is the render's


def test_the_history_rules(renderer):
    name, w, h, spp = "medium", 33, 17, 2
    sc = lc.SCENES[name](w, h)
    cams = binding.orbit_cameras(sc, 64)[:3]
    renderer.set_scene(sc)
    o = ac.opt()

    def moments(p):
        L, _, rays, _ = renderer.render_moments(p)
        return L, rays

    def passes_through(p):
        img, rays, _ = renderer.render_accumulated(p, o)
        L, want_rays = moments(p)
        return differing(img, L) == 0 and rays == want_rays

    def accumulates(p):
        img, _, _ = renderer.render_accumulated(p, o)
        return differing(img, moments(p)[0]) > 0

    p = lambda k, ww=w, hh=h: r1.make_params(ww, hh, spp, lc.SEED + k)  # noqa: E731
    assert passes_through(p(0))          # the first call
    assert accumulates(p(1))             # ... and the second has a history
    renderer.accumulate_reset()
    assert passes_through(p(2))          # after r1_accumulate_reset
    assert accumulates(p(3))
    assert passes_through(p(4, 40, 24))  # a changed size
    assert accumulates(p(5, 40, 24))
    renderer.set_scene(sc)
    assert passes_through(p(6, 40, 24))  # after r1_set_scene
    # r1_update_centers keeps the history: the next frame is the host composition on the moved arrays
    renderer.set_scene(sc)
    a = sc.arrays()
    x, y, z = moved_centres(a, "jitter")
    renderer.set_camera(cams[0])
    first, _, _ = renderer.render_accumulated(p(0), o)
    renderer.update_centers(0, x, y, z)
    renderer.set_camera(cams[1])
    second, rays, _ = renderer.render_accumulated(p(1), o)
    moved, keep = raw_from_arrays(a, x, y, z)  # (keep: the arrays `moved` points to)
    L0, V0, _ = binding.render_moments_host(sc.spheres.contents, cams[0], p(0))
    f0 = binding.render_features_host(sc.spheres.contents, cams[0], p(0))
    L1, V1, want_rays = binding.render_moments_host(moved, cams[1], p(1))
    f1 = binding.render_features_host(moved, cams[1], p(1))
    A1, _ = binding.accumulate_host(L1, V1, f1, L0, f0, V0, ac.view_of(cams[1], cams[0], spp, spp), o)
    assert differing(first, L0) == 0 and rays == want_rays
    assert differing(second, A1) == 0 and differing(second, L1) > 0  # (history was kept where the surfaces still agree)
    del keep


def test_a_progressive_accumulation_survives_accumulated_frames(renderer):
    w, h = 64, 48
    sc = lc.SCENES["small"](w, h)
    renderer.set_scene(sc)
    renderer.render_accumulated(r1.make_params(w, h, 2, lc.SEED), ac.opt())
    renderer.render_pass(r1.make_params(w, h, 2, lc.SEED), 0, image=False)
    renderer.render_accumulated(r1.make_params(w, h, 2, lc.SEED + 1), ac.opt(), gc.opt())
    img, total = renderer.render_pass(r1.make_params(w, h, 3, lc.SEED), 2)
    want = renderer.render(r1.make_params(w, h, 5, lc.SEED))
    assert total == want[1] and img.tobytes() == want[0].tobytes()


# ---- the history rules, sentence by sentence ------------------------------------------------------------------------------------------------------

NAME, W, H = "medium", 33, 17
ALL_VARIANTS = (binding.VARIANT_DEFAULT, binding.VARIANT_BVH, binding.VARIANT_GRID, binding.VARIANT_REFERENCE)


@functools.lru_cache(maxsize=None)
def medium():
    """(scene, four cameras of its orbit): built once, never changed"""
    sc = lc.SCENES[NAME](W, H)
    return sc, tuple(binding.orbit_cameras(sc, 64)[:4])


def seeds_of(n):
    return [lc.SEED + k for k in range(n)]


def run_path(renderer, cams, seeds, w=W, h=H, spp=2, go=None, variant=binding.VARIANT_DEFAULT, o=None):
    """[(frame, rays)] of r1_render_accumulated along `cams` on the context as it stands; w, h, spp, go and variant may be lists"""
    n = len(cams)
    out = []
    for cam, seed, w_k, h_k, spp_k, go_k, variant_k in zip(cams, seeds, per_frame(w, n), per_frame(h, n), per_frame(spp, n), per_frame(go, n), per_frame(variant, n)):
        renderer.set_camera(cam)
        img, rays, _ = renderer.render_accumulated(r1.make_params(w_k, h_k, spp_k, seed, variant=variant_k), o or ac.opt(), go_k)
        out.append((img, rays))
    return out


def assert_path(got, want, tag):
    assert len(got) == len(want)
    for k, (g, s) in enumerate(zip(got, want)):
        assert g[1] == s["rays"] and differing(g[0], s["out"]) == 0, (tag, k, differing(g[0], s["out"]))


def assert_accumulates(steps, tag=None):
    """a self-check of a case: these frames are not their own pass-through frames, so a lost history would show"""
    for k, s in enumerate(steps):
        assert not s["passed"] and differing(s["A"], s["L"]) > 0, (tag, k)


@pytest.mark.parametrize("filtered", [False, True], ids=["accumulated", "accumulated_and_filtered"])
def test_spp_changes_along_the_path(renderer, filtered):
    """"... which the call then replaces by its own unfiltered result, feature frame, camera and SPP": spp_prev is the spp of the frame before"""
    sc, cams = medium()
    spp, seeds = [2, 4, 3, 2], seeds_of(4)
    go = gc.opt() if filtered else None
    want = host_steps(sc.spheres.contents, cams, W, H, spp, seeds, go)
    assert_accumulates(want[1:])
    for k in (1, 2, 3):  # the case tells the two apart: with the frame's own spp for spp_prev the composition is another frame
        s, b = want[k], want[k - 1]
        wrong, _ = binding.accumulate_host(s["L"], s["V"], s["f"], b["A"], b["f"], b["M"], ac.view_of(cams[k], cams[k - 1], spp[k], spp[k]), ac.opt())
        assert differing(wrong, s["A"]) > 0, k
    renderer.set_scene(sc)
    assert_path(run_path(renderer, cams, seeds, spp=spp, go=go), want, "spp 2, 4, 3, 2")


def test_the_variant_switched_between_frames(renderer):
    sc, cams = medium()
    seeds = seeds_of(4)
    want = host_steps(sc.spheres.contents, cams, W, H, 2, seeds)
    assert_accumulates(want[1:])
    renderer.set_scene(sc)
    assert_path(run_path(renderer, cams, seeds, variant=list(ALL_VARIANTS)), want, "DEFAULT, BVH, GRID, REFERENCE")


def test_the_filter_switched_on_off_on(renderer):
    """"(the history keeps the unfiltered accumulation)" whatever went out: a frame behind a filtered one is the unfiltered path's"""
    sc, cams = medium()
    seeds = seeds_of(4)
    go = [gc.opt(), None, gc.opt(), None]
    want = host_steps(sc.spheres.contents, cams, W, H, 2, seeds, go)
    assert_accumulates(want[1:])
    assert differing(want[0]["out"], want[0]["A"]) > 0  # (the filter changes the frame, so a history of filtered frames would show)
    renderer.set_scene(sc)
    assert_path(run_path(renderer, cams, seeds, go=go), want, "on, off, on, off")


@pytest.mark.parametrize("how", ["update_spheres", "resort_spheres", "regrid"])
def test_updates_resort_and_regrid_keep_the_history(renderer, how):
    """"r1_update_*, r1_resort_spheres and r1_regrid keep it": the next frame is the host composition on the updated arrays against the
    history of the arrays as they were"""
    sc, cams = medium()
    a = sc.arrays()
    variant = binding.VARIANT_GRID if how == "regrid" else binding.VARIANT_DEFAULT
    renderer.set_scene(sc)
    first = run_path(renderer, cams[:1], seeds_of(1), variant=variant)  # (through the grid where it is to be re-registered: that builds it)
    if how == "update_spheres":
        x, y, z, rsq, inv = radius_family(a, "lattice_x0.25")
        mats = material_family(a, "permute")
        renderer.update_spheres(0, radii=(rsq, inv), materials=mats)
        after = edited(a, None, (rsq, inv), mats)
    else:
        x, y, z = moved_centres(a, "jitter")
        renderer.update_centers(0, x, y, z)
        renderer.resort_spheres() if how == "resort_spheres" else renderer.regrid()
        after = edited(a, (x, y, z))
    moved, keep = raw_from_arrays(after)  # (keep: the arrays `moved` points to)
    want = host_steps([sc.spheres.contents, moved], cams[:2], W, H, 2, seeds_of(2))
    assert_accumulates(want[1:], how)
    renderer.set_camera(cams[1])
    img, rays, _ = renderer.render_accumulated(r1.make_params(W, H, 2, lc.SEED + 1, variant=variant), ac.opt())
    assert_path(first + [(img, rays)], want, how)
    del keep


def test_a_refused_call_keeps_the_history(renderer):
    """"A refused call enqueues nothing and keeps the history": one refusal of each kind in the documented order, down to what
    r1_render_moments refuses, between two frames; the second is the host path's, not a pass-through"""
    sc, cams = medium()
    a = sc.arrays()
    x, y, z = moved_centres(a, "jitter")
    moved, keep = raw_from_arrays(edited(a, (x, y, z)))
    want = host_steps([sc.spheres.contents, moved], cams[:2], W, H, 2, seeds_of(2))
    assert_accumulates(want[1:])
    Lb, c, o, go = r1.lib(), renderer._c, ac.opt(), gc.opt()
    renderer.set_scene(sc)
    first = run_path(renderer, cams[:1], seeds_of(1))
    renderer.update_centers(0, x, y, z)  # (keeps the history; the grid is stale from here on)
    renderer.set_camera(cams[1])
    frame = torch.full((H, W, 3), 5.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    info = renderer.launch_info()

    def p(spp=2, **kw):
        return r1.make_params(W, H, spp, lc.SEED + 1, **kw)

    refused = [(lambda: renderer.render_accumulated(p(), ac.opt(flags=1)), "flags"),
               (lambda: renderer.render_accumulated(p(), ac.opt(max_samples=0)), "max_samples"),
               (lambda: renderer.render_accumulated(p(), o, gc.opt(variance_floor=0.0)), "variance_floor"),
               (lambda: renderer.render_accumulated(p(variant=binding.VARIANT_PREFILTER), o), "variant"),
               (lambda: renderer.render_accumulated(p(spp=1), o, go), "spp"),
               (lambda: renderer.render_accumulated_device(p(), o, None, frame.data_ptr() + 2, cnt.data_ptr()), "aligned"),
               (lambda: renderer.render_accumulated_device(p(), o, None, frame.data_ptr(), cnt.data_ptr() + 4), "aligned"),
               (lambda: renderer.render_accumulated(p(shard=0, num_shards=2), o), "num_shards"),                    # r1_render_moments' own
               (lambda: renderer.render_accumulated(p(variant=binding.VARIANT_GRID), o), MOVED_RULE),                # ... the stale grid
               (lambda: renderer.render_accumulated_device(p(variant=binding.VARIANT_GRID), o, go, frame.data_ptr(), cnt.data_ptr()), MOVED_RULE)]
    for k, (call, text) in enumerate(refused):
        with pytest.raises(binding.R1Error) as e:
            call()
        assert e.value.code == binding.R1_EINVAL and text in str(e.value), (k, e.value)
        assert renderer.launch_info() == info, k
    assert Lb.r1_render_accumulated(c, None, C.byref(o), None, None, None, None) == binding.R1_EINVAL
    torch.cuda.synchronize()
    assert bool((frame == 5).all()) and bool((cnt == 5).all())  # nothing was enqueued
    img, rays, _ = renderer.render_accumulated(p(), o)
    assert_path(first + [(img, rays)], want, "after the refusals")
    del keep


def without_w(cam):
    """a copy of `cam` with w = 0: it renders as before — the kernels read origin, lower_left, horizontal, vertical, u, v and the lens
    radius — but as a PREVIOUS camera its plan has pw = 0, through which nothing can be projected"""
    out = binding.CCamera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(out))
    out.w = (C.c_float * 3)(0, 0, 0)
    return out


def test_a_previous_camera_through_which_nothing_projects(renderer):
    """"A previous camera through which nothing can be projected also passes the frame through" — and the frame behind it accumulates again"""
    sc, cams = medium()
    flat = without_w(cams[1])
    with pytest.raises(binding.R1Error) as e:
        binding.accumulate_check(binding.AccumulateFrame(W, H, 0, 0, 0, 0, 0, 0, 0, 0), ac.opt(), ac.view_of(cams[2], flat, 2, 2))
    assert e.value.code == binding.R1_EINVAL and "camera_prev" in str(e.value)
    path, seeds = [cams[0], flat, cams[2], cams[3]], seeds_of(4)
    want = host_steps(sc.spheres.contents, path, W, H, 2, seeds)
    assert [s["passed"] for s in want] == [True, False, True, False]
    usual = host_steps(sc.spheres.contents, [cams[0], cams[1]], W, H, 2, seeds[:2])
    assert differing(want[1]["out"], usual[1]["out"]) == 0  # as the CURRENT camera it is cams[1]: w is not read
    assert_accumulates([want[1], want[3]])
    renderer.set_scene(sc)
    got = run_path(renderer, path, seeds)
    assert_path(got, want, "c0, flat, c2, c3")
    renderer.set_camera(cams[2])
    L, _, rays, _ = renderer.render_moments(r1.make_params(W, H, 2, seeds[2]))
    assert differing(got[2][0], L) == 0 and got[2][1] == rays  # the frame behind the flat camera is r1_render_moments' frame
    # ... and as the first frame of a path it is the render itself
    renderer.accumulate_reset()
    assert_path(run_path(renderer, [flat, cams[2]], seeds[1:3]), host_steps(sc.spheres.contents, [flat, cams[2]], W, H, 2, seeds[1:3]), "flat first")


def test_a_changed_size_that_does_not_grow_the_workspace(renderer):
    """"... and when width or height differ from the history's": smaller, and the same pixel count with width and height swapped"""
    sc, cams = medium()
    w, h = [40, 33, 33, 17, 17], [24, 17, 17, 33, 33]
    path, seeds = [cams[0], cams[1], cams[2], cams[3], cams[0]], seeds_of(5)
    want = host_steps(sc.spheres.contents, path, w, h, 2, seeds)
    assert [s["passed"] for s in want] == [True, True, False, True, False]
    assert_accumulates([want[2], want[4]])
    renderer.set_scene(sc)
    got = run_path(renderer, path, seeds, w=w, h=h)
    assert_path(got, want, "40x24, 33x17, 33x17, 17x33, 17x33")
    for k in (1, 3):  # exactly where the size changed: r1_render_moments' frame
        renderer.set_camera(path[k])
        L, _, rays, _ = renderer.render_moments(r1.make_params(w[k], h[k], 2, seeds[k]))
        assert differing(got[k][0], L) == 0 and got[k][1] == rays, k


def query_rays(cam, n=64):
    """n rays from the camera's origin through its screen"""
    c = ac.cam_fields(cam)
    rays = np.zeros(n, binding.RAY_DTYPE)
    s = (np.arange(n, dtype=np.float32) + np.float32(0.5)) / np.float32(n)
    rays["o"] = c["origin"]
    rays["d"] = (c["lower_left"] + c["horizontal"] * s[:, None] + c["vertical"] * s[::-1, None]) - c["origin"]
    rays["t_max"] = np.float32(1e30)
    return rays


def test_the_history_survives_the_other_calls_of_the_context(renderer):
    """between two accumulated frames every other kind of call runs once at the same size; the second frame is still the host path's"""
    sc, cams = medium()
    seeds = seeds_of(2)
    want = host_steps(sc.spheres.contents, cams[:2], W, H, 2, seeds, [None, gc.opt()])
    assert_accumulates(want[1:])
    renderer.set_scene(sc)
    first = run_path(renderer, cams[:1], seeds[:1])
    p = r1.make_params(W, H, 2, 99)
    renderer.render(p)
    renderer.render_pass(p, 0)
    renderer.render_adaptive(r1.make_params(W, H, 4, 99), 1, 1, -1, 0)
    renderer.render_region(p, (3, 2, 20, 9))
    renderer.render_linear(p)
    renderer.render_moments(p)
    renderer.render_features(p)
    renderer.render_denoised(p, dc.opt())
    renderer.render_denoised_guided(p, gc.opt())
    frames, view = ac.synthetic_inputs("37x21", "identical")
    check_both_forms(renderer, frames, view, ac.host_result("synthetic", "37x21", "identical"))
    rays = query_rays(cams[0])
    assert len(renderer.cast_rays(rays)) == len(rays) and len(renderer.trace_rays(rays)) == len(rays)
    hf = binding.HostFrame(W, H)
    try:
        renderer.render_async(p, hf)
        renderer.sync()
        assert hf.rays > 0
    finally:
        hf.close()
    assert_path(first + run_path(renderer, cams[1:2], seeds[1:], go=gc.opt()), want, "after the other calls")


def test_two_streams_ordered_by_the_caller(renderer):
    """"the calls of a context are ordered by one stream, or by the caller": frame k on stream A, frame k + 1 on stream B behind an event
    of A, frame k + 2 through the synchronous form once both are idle"""
    sc, cams = medium()
    seeds = seeds_of(3)
    want = host_steps(sc.spheres.contents, cams[:3], W, H, 2, seeds)
    assert_accumulates(want[1:])
    renderer.set_scene(sc)
    out = [torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    renderer.set_camera(cams[0])
    renderer.render_accumulated_device(r1.make_params(W, H, 2, seeds[0]), ac.opt(), None, out[0].data_ptr(), count[0:].data_ptr(), A.cuda_stream)
    B.wait_stream(A)
    renderer.set_camera(cams[1])
    renderer.render_accumulated_device(r1.make_params(W, H, 2, seeds[1]), ac.opt(), None, out[1].data_ptr(), count[1:].data_ptr(), B.cuda_stream)
    A.synchronize()
    B.synchronize()
    got = [(out[k].cpu().numpy(), int(count[k].item())) for k in range(2)]
    assert_path(got + run_path(renderer, cams[2:3], seeds[2:]), want, "stream A, stream B, synchronous")
