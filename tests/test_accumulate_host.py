"""CPU tests of accumulated frames (include/rays1.h): every new name is declared, exported and bound; r1_accumulate_host equals
the contract restated in numpy (tests/accumulate_cases.py) bit for bit on rendered pairs and on synthetic pairs asserted to hold every block
the contract names, under seven camera pairs and option sets that cover both ends of every range; a pixel without history carries L's and V's
bits; the sample count's cap; variances stay non-negative; strides with sentinel bytes; in place; every refusal with its text; the quality of
an orbit and of a static camera on the medium scene; the census of the new kernel; the stand-alone program under the sanitizers; and both CPU
forms against the reprojection computed in float64 (tests/reproject_truth_cases.py) under cameras that are not axis-aligned.  What the
device computes: tests/test_gpu_accumulate.py.  Only the quality tests and the float64 comparison have bounds."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import accumulate_cases as ac
import denoise_cases as dc
import guided_cases as gc
import reproject_truth_cases as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("r1_accumulate_check", "r1_accumulate_host", "r1_accumulate_device", "r1_accumulate", "r1_render_accumulated", "r1_render_accumulated_device",
       "r1_accumulate_reset")


def test_every_new_name_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    names = {s[0] for s in binding.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(r1.lib(), name) and name in names, name
    assert re.search(r"#define R1_ABI_VERSION 4\b", hdr)
    assert C.sizeof(binding.AccumulateOpt) == 16 and C.sizeof(binding.AccumulateFrame) == 40 and C.sizeof(binding.AccumulateView) == 2 * 88 + 8
    assert C.sizeof(binding.AccumulateImages) == 64 and C.sizeof(binding.ReprojectPlan) == 28
    for m in ("accumulate", "accumulate_device", "render_accumulated", "render_accumulated_device", "accumulate_reset"):
        assert callable(getattr(binding.Renderer, m, None)), m
    for fn in ("make_accumulate_opt", "accumulate_check", "accumulate_host"):
        assert callable(getattr(binding, fn, None)), fn


def check_properties(frames, got, o, blended):
    """what holds for every result (blended: the pixels the restatement blends): a pixel without history carries L's and V's bits; the cap;
    variances of inputs >= 0 stay >= 0"""
    L, V = np.array(frames[0]), np.array(frames[1])
    A, M = got
    keep = ~blended
    assert ac.bits(A).reshape(A.shape[:2] + (12,))[keep].tobytes() == ac.bits(L).reshape(A.shape[:2] + (12,))[keep].tobytes()
    assert ac.bits(M).reshape(M.shape + (16,))[keep].tobytes() == ac.bits(V).reshape(M.shape + (16,))[keep].tobytes()
    assert (M["samples"] <= np.maximum(V["samples"], o.max_samples)).all()
    assert (M["samples"][blended] >= V["samples"][blended]).all()
    assert (M["var"][blended] >= 0).all()


@pytest.mark.parametrize("options", sorted(ac.OPTION_SETS))
@pytest.mark.parametrize("how", ["seeds", "orbit"])
@pytest.mark.parametrize("name", sorted(ac.RENDERED))
def test_host_form_equals_the_numpy_form_on_rendered_pairs(name, how, options):
    frames, view = ac.rendered_inputs(name, how)
    o = ac.opt(**ac.OPTION_SETS[options])
    *want, stats = ac.numpy_accumulate(*frames, view, o, want_stats=True)
    got = binding.accumulate_host(*frames, view, o)
    assert ac.same(got, want), (name, how, options)
    check_properties(frames, got, o, stats["mask"])
    assert stats["blended"] > 0 or options in ("high ends", "low ends")  # (normal_min_cos 1 or depth_tolerance 1e-30 leave little)


@pytest.mark.parametrize("options", sorted(ac.OPTION_SETS))
@pytest.mark.parametrize("pair", ac.PAIRS)
@pytest.mark.parametrize("name", sorted(ac.SYNTHETIC))
def test_host_form_equals_the_numpy_form_on_synthetic_pairs(name, pair, options):
    frames, view = ac.synthetic_inputs(name, pair)
    o = ac.opt(**ac.OPTION_SETS[options])
    *want, stats = ac.numpy_accumulate(*frames, view, o, want_stats=True)
    got = binding.accumulate_host(*frames, view, o)
    assert ac.same(got, want), (name, pair, options)
    check_properties(frames, got, o, stats["mask"])
    if pair == "turned":  # c * pw <= 0 at every pixel: the current frame, bit for bit, in both images
        assert ac.same(got, (np.array(frames[0]), np.array(frames[1])))


@pytest.mark.parametrize("name", ["37x21", "70x40"])
def test_synthetic_pairs_hold_every_block_and_the_camera_pairs_do_what_they_are_for(name):
    w, h = ac.SYNTHETIC[name]
    L, V, f, A_prev, f_prev, M_prev = ac.synthetic(w, h)
    k = ac.classes(V, f, f_prev, M_prev)
    for what, count in k.items():
        assert count > 0, (what, k)
    stats = {}
    for pair in ac.PAIRS:
        frames, view = ac.synthetic_inputs(name, pair)
        stats[pair] = ac.numpy_accumulate(*frames, view, ac.opt(), want_stats=True)[2]
    s = stats["identical"]
    assert s["blended"] > 0 and s["fx exactly 0"] > 0  # (iv): the camera is axis-aligned, columns reproject onto themselves exactly
    assert all(v > 0 for v in s["skipped"].values()), s["skipped"]  # every reason to skip a tap occurs
    for pair in ("left", "right", "down", "up"):  # (ii): a strip along that edge re-projects off the image, the rest does not
        s = stats[pair]
        assert s["off by edge"][pair] > 0 and s["history"] > 0 and s["blended"] > 0, (pair, s)
        assert sum(s["off by edge"].values()) == s["off by edge"][pair]
    s = stats["zoom"]  # (iii): one tap column on the image at either side
    assert s["px in (-1, 0)"] > 0 and s["px in (w - 1, w)"] > 0 and s["blended"] > 0
    s = stats["turned"]  # (v)
    assert s["history"] == 0 and s["behind the previous camera"] == s["surface without history"] > 0
    # the wrap case: a history of 0xFFFFFFF0 samples is blended and ends at the cap, not at a wrapped sum
    frames, view = ac.synthetic_inputs(name, "identical")
    A, M = ac.host_result("synthetic", name, "identical", "high ends")
    lifted = (M["samples"] >= ac.WRAP)
    assert lifted.sum() > 0 and (M["samples"][lifted] == ac.WRAP + ac.SPP).all()


def test_synthetic_frames_under_two_rotated_cameras():
    """the six guard classes of the synthetic frames (NaN depth, the wrap, ...) through a previous camera that is not axis-aligned"""
    name, pair = ac.ROTATED_AT, ac.ROTATED_PAIR
    frames, view = ac.synthetic_inputs(name, pair)
    assert all(abs(x) > 0.01 for k in ("u", "v") for x in ac.cam_fields(view.camera_prev)[k])  # (no component of the basis is 0)
    for options in sorted(ac.OPTION_SETS):
        o = ac.opt(**ac.OPTION_SETS[options])
        *want, stats = ac.numpy_accumulate(*frames, view, o, want_stats=True)
        got = binding.accumulate_host(*frames, view, o)
        assert ac.same(got, want), options
        check_properties(frames, got, o, stats["mask"])
        if options == "defaults":
            s = stats
    assert s["blended"] > 0 and s["surface without history"] > 0 and s["fx exactly 0"] == 0, s
    for why in ("off the image", "hits", "samples", "depth", "normal"):
        assert s["skipped"][why] > 0, s["skipped"]


# ---- against the geometry in float64 ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("size,prev", rt.CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_both_cpu_forms_look_where_float64_geometry_says(size, prev):
    """tests/reproject_truth_cases.py: the history is the ramp (x, y, 1), so A_out is the reprojected screen position; the truth is the
    plane's point projected through the previous camera in float64.  Bound: 32 * 2^-24 * max(w, h) pixels; measured (printed here, table
    in reproject_truth_cases.py and DESIGN.md §4.41) at most 6.53 of those units."""
    c = rt.case(size, prev)
    *want, stats = ac.numpy_accumulate(*c["frames"], c["view"], c["opt"], want_stats=True)
    got = binding.accumulate_host(*c["frames"], c["view"], c["opt"])
    print(f"{size} {prev}: compared {c['compared'].mean():.3f} of the frame, numpy {rt.error_in_units(c, want[0]):.2f}, host {rt.error_in_units(c, got[0]):.2f} "
          f"x 2^-24 max(w, h) px")
    assert stats["skipped"]["depth"] == 0 and stats["skipped"]["normal"] == 0 and stats["skipped"]["hits"] == 0 and stats["skipped"]["samples"] == 0
    assert (stats["mask"] | ~c["compared"]).all()  # every compared pixel is blended
    rt.check_against_truth(c, want, (size, prev, "numpy"))
    rt.check_against_truth(c, got, (size, prev, "host"))
    assert ac.same(got, want), (size, prev)  # ... and the two stay bit-equal on camera pairs neither has seen


def test_the_truth_cases_tell_the_mistakes_apart():
    """the float64 truth moves by half a pixel or more under each mistake it is there to catch — a self-check of the cases, in float64
    alone: nothing of the code under test runs here"""
    c = rt.case("70x40", "general")
    w, h = c["size"]
    m = c["compared"]
    cur, was = rt.cameras("general", w, h)
    o, dh, dist = rt.plane_distance(cur, w, h)
    good = c["truth"][..., :2] / (1.0 - rt.ALPHA)

    def moved(P, cam=was):
        px, py, _ = rt.screen_position(P, cam, w, h)
        return float(np.abs(np.stack([px, py], -1) - good)[m].max())

    assert moved(o + dh * dist[..., None]) == 0.0
    assert moved(o + dh * (dist * rt.SPP_PREV / rt.SPP)[..., None]) >= 0.5       # spp_prev where spp belongs
    assert moved(o + dh[::-1] * dist[::-1][..., None]) >= 0.5                    # t from the other edge
    assert moved(o + dh * dist[..., None], cur) >= 0.5                            # the current camera for the previous one
    assert rt.tolerance(w, h) < 1e-3


@pytest.mark.parametrize("name,pair", [("37x21", "left"), ("70x40", "zoom")])
def test_in_place_equals_the_result_without_aliasing(name, pair):
    frames, view = ac.synthetic_inputs(name, pair)
    L, V = np.array(frames[0]), np.array(frames[1])
    A, M = binding.accumulate_host(L, V, *frames[2:], view, ac.opt(), A_out=L, M_out=V)
    assert A is L and M is V and ac.same((L, V), ac.host_result("synthetic", name, pair))


@pytest.mark.parametrize("name,pair", [("37x21", "right"), ("5x3", "identical")])
def test_strides_with_sentinel_bytes_between_the_rows_stay_untouched(name, pair):
    frames, view = ac.synthetic_inputs(name, pair)
    w = frames[0].shape[1]
    views, bufs = zip(*[dc.strided(np.array(a), w + 1 + k) for k, a in enumerate(frames)])
    Ao, Aob = dc.strided(np.zeros_like(np.array(frames[0])), w + 9)
    Mo, Mob = dc.strided(np.zeros_like(np.array(frames[1])), w + 8)
    before = [b.tobytes() for b in bufs]
    got = binding.accumulate_host(*views, view, ac.opt(), A_out=Ao, M_out=Mo)
    assert ac.same(got, ac.host_result("synthetic", name, pair))
    assert [b.tobytes() for b in bufs] == before
    assert (Aob[:, w:].view(np.uint8) == dc.PREFILL).all() and (Mob[:, w:].view(np.uint8) == dc.PREFILL).all()


def test_every_refusal_with_its_text():
    Lb = r1.lib()
    frames, view = ac.synthetic_inputs("5x3", "identical")
    good = binding.AccumulateFrame(5, 3, 0, 0, 0, 0, 0, 0, 0, 0)
    assert isinstance(binding.accumulate_check(good, ac.opt(), view), binding.ReprojectPlan)
    plan = binding.accumulate_check(binding.AccumulateFrame(5, 3, 5, 6, 7, 8, 9, 10, 11, 12), ac.opt(), view)
    assert plan.pw == -1.0 and plan.hu == 2.0 and plan.inv_w == np.float32(1) / np.float32(5)
    strides = ("linear_stride", "moment_stride", "feature_stride", "prev_stride", "prev_feature_stride", "prev_moment_stride", "out_stride", "out_moment_stride")
    bad = [(binding.AccumulateFrame(0, 3, 0, 0, 0, 0, 0, 0, 0, 0), ac.opt(), view, "width"), (binding.AccumulateFrame(5, 0, 0, 0, 0, 0, 0, 0, 0, 0), ac.opt(), view, "height")]
    for k, field in enumerate(strides):
        fr = binding.AccumulateFrame(5, 3, 0, 0, 0, 0, 0, 0, 0, 0)
        setattr(fr, field, 4)
        bad.append((fr, ac.opt(), view, field))
    flat = ac.view_of(view.camera, view.camera_prev, 4, 3)
    flat.camera_prev.w = (C.c_float * 3)(0, 0, 0)
    flat.camera_prev.lower_left = flat.camera_prev.origin
    nanv = ac.view_of(view.camera, view.camera_prev, 4, 3)
    nanv.camera_prev.horizontal = (C.c_float * 3)(float("nan"), 0, 0)
    bad += [(good, ac.opt(max_samples=0), view, "max_samples"), (good, ac.opt(depth_tolerance=0.0), view, "depth_tolerance"),
            (good, ac.opt(depth_tolerance=-1.0), view, "depth_tolerance"), (good, ac.opt(depth_tolerance=float("inf")), view, "depth_tolerance"),
            (good, ac.opt(depth_tolerance=float("nan")), view, "depth_tolerance"), (good, ac.opt(normal_min_cos=1.5), view, "normal_min_cos"),
            (good, ac.opt(normal_min_cos=-1.5), view, "normal_min_cos"), (good, ac.opt(normal_min_cos=float("nan")), view, "normal_min_cos"),
            (good, ac.opt(flags=1), view, "flags"), (good, ac.opt(), ac.view_of(view.camera, view.camera_prev, 0, 3), "spp"),
            (good, ac.opt(), ac.view_of(view.camera, view.camera_prev, 4, 0), "spp_prev"), (good, ac.opt(), flat, "camera_prev"), (good, ac.opt(), nanv, "camera_prev")]
    for fr, o, v, field in bad:
        with pytest.raises(binding.R1Error) as e:
            binding.accumulate_check(fr, o, v)
        assert e.value.code == binding.R1_EINVAL and field in str(e.value), (field, e.value)
    with pytest.raises(binding.R1Error) as e:
        binding.accumulate_check(binding.AccumulateFrame(65536, 32768, 0, 0, 0, 0, 0, 0, 0, 0), ac.opt(), view)
    assert e.value.code == binding.R1_ELIMIT
    for args, text in (((None, C.byref(ac.opt()), C.byref(view), None), "frame is NULL"), ((C.byref(good), None, C.byref(view), None), "options is NULL"),
                       ((C.byref(good), C.byref(ac.opt()), None, None), "view is NULL")):
        assert Lb.r1_accumulate_check(*args) == binding.R1_EINVAL and text in Lb.r1_last_error().decode()
    # the host form: the check first, then the images; nothing is written
    arrays = [np.array(a) for a in frames]
    A_out, M_out = np.full(arrays[0].shape, 7, np.float32), np.zeros(arrays[1].shape, binding.MOMENT_DTYPE)
    M_out["samples"] = 7
    ptrs = [a.ctypes.data for a in arrays] + [A_out.ctypes.data, M_out.ctypes.data]
    names = ("L", "V", "f", "A_prev", "f_prev", "M_prev", "A_out", "M_out")

    def host(images, o=None, v=None):
        im = binding.AccumulateImages(*images)
        return Lb.r1_accumulate_host(C.byref(good), C.byref(o or ac.opt()), C.byref(v or view), C.byref(im))

    for k, name in enumerate(names):
        images = list(ptrs)
        images[k] = None
        assert host(images) == binding.R1_EINVAL and f"{name} is NULL" in Lb.r1_last_error().decode()
    for out, hist in ((6, 3), (6, 4), (6, 5), (7, 3), (7, 4), (7, 5)):  # overlapping history: the call is a gather
        images = list(ptrs)
        images[out] = ptrs[hist]
        assert host(images) == binding.R1_EINVAL and "overlaps the history" in Lb.r1_last_error().decode() and names[hist] in Lb.r1_last_error().decode()
    images = list(ptrs)
    images[7] = ptrs[6]
    assert host(images) == binding.R1_EINVAL and "A_out may be L" in Lb.r1_last_error().decode()
    assert host(ptrs, o=ac.opt(max_samples=0)) == binding.R1_EINVAL and host(ptrs, v=flat) == binding.R1_EINVAL
    assert Lb.r1_accumulate_host(C.byref(good), C.byref(ac.opt()), C.byref(view), None) == binding.R1_EINVAL and "images is NULL" in Lb.r1_last_error().decode()
    assert (A_out == 7).all() and (M_out["samples"] == 7).all() and not M_out["var"].any()
    # the device forms refuse a null context first, without a device
    p = r1.make_params(16, 8, 2)
    for call in (lambda: Lb.r1_accumulate_device(None, None, None, None, None, None), lambda: Lb.r1_accumulate(None, None, None, None, None, None),
                 lambda: Lb.r1_render_accumulated(None, C.byref(p), None, None, None, None, None),
                 lambda: Lb.r1_render_accumulated_device(None, None, None, None, None, None, None), lambda: Lb.r1_accumulate_reset(None)):
        assert call() == binding.R1_EINVAL and "ctx is NULL" in Lb.r1_last_error().decode()


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------

W, H = 160, 100


def accumulate_path(frames, spp):
    """the last frame's (A, M) after each frame was accumulated by r1_accumulate_host against the one before"""
    A = M = fp = cam_p = None
    for L, V, f, cam in frames:
        if A is None:
            A, M = np.array(L), np.array(V)
        else:
            A, M = binding.accumulate_host(L, V, f, A, fp, M, ac.view_of(cam, cam_p, spp, spp), ac.opt())
        fp, cam_p = f, cam
    return A, M


def path_frames(n, spp, path):
    keys = [(path, k) if path else None for k in range(n)]
    frames = [ac.render("medium", W, H, spp, 4242 + k, key) + (ac.camera_of("medium", W, H, key),) for k, key in enumerate(keys)]
    sc = r1.create_medium_scene(W, H)
    ref, _ = binding.render_linear_host(sc.spheres.contents, frames[-1][3], r1.make_params(W, H, 512, 777))
    return frames, ref


def test_an_orbit_accumulated_beats_its_last_frame_noisy_and_filtered():
    """medium 160 x 100 (the full size: nothing was shrunk), 2 spp, eight frames along orbit_cameras(scene, 720)[:8], seeds 4242 + frame,
    against the last camera at 512 spp, seed 777.  tools/accumulate_prototype.py, the numpy restatement, measured
    RMSE(accumulated) / RMSE(noisy last frame) = 0.4214 and RMSE(accumulated, then guided) / RMSE(guided filter of the last frame alone) =
    0.7517; asserted are the midpoints between those ratios and 1: 0.7107 and 0.8759."""
    frames, ref = path_frames(8, 2, 720)
    L, V, f, _ = frames[-1]
    A, M = accumulate_path(frames, 2)
    noisy, acc = dc.rmse(L, ref), dc.rmse(A, ref)
    alone = dc.rmse(binding.denoise_guided_host(L, f, V, gc.opt()), ref)
    both = dc.rmse(binding.denoise_guided_host(A, f, M, gc.opt()), ref)
    print(f"orbit: noisy {noisy:.5f}, accumulated / noisy {acc / noisy:.4f}, guided alone / noisy {alone / noisy:.4f}, accumulated then guided / guided alone {both / alone:.4f}")
    assert acc < noisy and both < alone
    assert acc / noisy < 0.7107
    assert both / alone < 0.8759


def test_a_static_camera_accumulated_beats_its_last_frame():
    """medium 160 x 100, four frames of 4 spp through the scene's camera, seeds 4242 + frame, against 512 spp, seed 777.  The prototype
    measured RMSE(accumulated) / RMSE(noisy last frame) = 0.5765 (16 samples behind most pixels: 0.5 would be ideal); asserted is the midpoint
    to 1, 0.7883."""
    frames, ref = path_frames(4, 4, None)
    A, M = accumulate_path(frames, 4)
    noisy, acc = dc.rmse(frames[-1][0], ref), dc.rmse(A, ref)
    print(f"static: noisy {noisy:.5f}, accumulated / noisy {acc / noisy:.4f}")
    assert acc < noisy
    assert acc / noisy < 0.7883


# ---- the built library ------------------------------------------------------------------------------------------------------------------------


def test_census_of_the_reproject_kernel():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    k = kernel_meta.collect(lib)
    own = sorted(n for n in k if "r1_reproject" in n)
    assert len(own) == 1 and "r1_reproject_kernel" in own[0], own
    for taken in ("r1_denoise", "r1_vfilter", "r1_pass_kernel", "r1_region_kernel", "r1_resolve_", "r1_query_"):  # the other features' censuses count by these
        assert taken not in own[0]
    a = k[own[0]]
    print(own[0], {x: a[x] for x in ("vgpr", "sgpr", "sgpr_spill", "lane_moves", "insts", "lds")})  # (recorded in DESIGN.md §4.41)
    assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, a
    assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0 and int(a["sgpr_spill"]) == 0, a
    assert int(a["lds"]) == 0  # the source window of a tile depends on the data: nothing is staged
    assert int(a["vgpr"]) <= 128  # four waves a SIMD fit


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/check_accumulate_host.cpp built with the one host source it drives, under the address and undefined-behaviour sanitizers: a
    stand-alone program of its own, no GPU, nothing loaded into another process."""
    import subprocess
    out = str(tmp_path_factory.mktemp("accumulate_host") / "check_accumulate_host")
    src = [os.path.join(ROOT, "tools", "check_accumulate_host.cpp"), os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_accumulate_host.cpp")]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-o", out])
    return out


def test_stand_alone_program_under_the_sanitizers(check_program):
    import subprocess
    out = subprocess.run([check_program], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for says in ("every value the contract's under 7 camera pairs x 5 sets of options", "buffers that end with their last pixel", "in place: A_out = L and M_out = V",
                 "refusals wrote nothing"):
        assert says in out.stdout
