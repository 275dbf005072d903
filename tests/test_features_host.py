"""CPU tests of feature frames (include/rays1.h): the three names are declared, exported and bound; the host form
r1_render_features_host equals the contract folded in numpy float32 from r1_camera_rays + r1_cast_rays_host + the scene arrays, on cases whose
coverage classes are asserted from the host form itself; a pixel without a hit has r1_render_linear_host's value; a region is the crop of the
frame and leaves the bytes between its rows alone; the refusal table; the drop-in program refuses --features with what it cannot serve; the
census of the five feature kernels in the built library; tools/check_features_host.cpp.  What the device computes is checked in
tests/test_gpu_features.py.  Every comparison is tobytes() equality."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
import feature_cases as fc
import linear_cases as lc
import region_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("r1_render_features", "r1_render_features_device", "r1_render_features_host")


def test_every_new_name_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    names = {s[0] for s in binding.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(r1.lib(), name) and name in names, name
    assert re.search(r"typedef\s+struct\s+r1_feature\s*\{\s*float\s+albedo\s*\[\s*3\s*\]\s*;\s*float\s+depth\s*;\s*float\s+normal\s*\[\s*3\s*\]\s*;\s*uint32_t\s+hits\s*;\s*\}\s*r1_feature\s*;", hdr)
    ptr = r"\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+r1_render_features\s*\(\s*r1_context" + ptr + r",\s*const\s+r1_params" + ptr + r",\s*const\s+r1_region" + ptr + r",\s*r1_feature" + ptr +
                     r",\s*double" + ptr + r"\)\s*;", hdr)
    assert re.search(r"\bint\s+r1_render_features_device\s*\(\s*r1_context" + ptr + r",\s*const\s+r1_params" + ptr + r",\s*const\s+r1_region" + ptr + r",\s*void" + ptr +
                     r",\s*void" + ptr + r"\)\s*;", hdr)
    assert re.search(r"\bint\s+r1_render_features_host\s*\(\s*const\s+r1_scene" + ptr + r",\s*const\s+r1_camera" + ptr + r",\s*const\s+r1_params" + ptr +
                     r",\s*const\s+r1_region" + ptr + r",\s*r1_feature" + ptr + r"\)\s*;", hdr)
    assert re.search(r"#define R1_ABI_VERSION 4\b", hdr) and r1.lib().r1_abi_version() == 4
    assert binding.FEATURE_DTYPE.itemsize == 32
    assert [binding.FEATURE_DTYPE.fields[k][1] for k in ("albedo", "depth", "normal", "hits")] == [0, 12, 16, 28]
    for m in ("render_features", "render_features_device"):
        assert callable(getattr(binding.Renderer, m, None)), m
    assert callable(getattr(binding, "render_features_host", None))


# ---- the host form against the fold -----------------------------------------------------------------------------------------------------------

# the coverage classes the issue recorded from r1_camera_rays + r1_cast_rays_host: (pixels with no hit, with some, with all)
CLASSES = {"medium": (70, 19, 472), "far": (1669, 138, 1265), "inside": (0, 0, 3072)}


@pytest.mark.parametrize("name", ["medium", "large", "far", "inside", "glass", "empty"])
def test_host_form_equals_the_numpy_fold(name):
    p, sa = fc.params(name), fc.scene(name)
    got = fc.host_frame(name)
    assert got.dtype == binding.FEATURE_DTYPE and got.shape == (p.height, p.width)
    assert got.tobytes() == fc.fold(sa, p).tobytes()
    cls = fc.classes(got, p.spp)
    print(name, "pixels with no hit / some / all:", cls)
    if name in CLASSES:
        assert cls == CLASSES[name]
    if name in ("medium", "far"):
        assert min(cls) >= 10
    if name == "glass":  # every hit is a dielectric's: the albedo of a pixel whose samples all hit is spp additions of 1.0f, times 1 / spp
        full = got["hits"] == p.spp
        assert full.sum() >= 10
        ones = np.zeros(3, np.float32)
        for _ in range(p.spp):
            ones = ones + np.float32(1)
        assert (got["albedo"][full] == ones * (np.float32(1) / np.float32(p.spp))).all()
        assert (sa.arrays["mat_type"][sa.arrays["inv_radius"] != 0] == binding.MAT_DIELECTRIC).all()
    if name == "empty":
        assert cls == (p.width * p.height, 0, 0)
        assert not got["normal"].any() and not got["depth"].any() and (got["albedo"] > 0).all()


def test_medium_shows_every_material_and_pixels_that_see_two_spheres():
    p, sa = fc.params("medium"), fc.scene("medium")
    _, _, hits = fc.window_samples(sa, p, (0, 0, p.width, p.height))
    idx = hits["index"]
    counts = np.bincount(sa.arrays["mat_type"][idx[idx >= 0]], minlength=3)
    print("first-hit materials (Lambertian, Metal, Dielectric):", counts.tolist())
    assert counts.tolist() == [1053, 310, 83]
    two = sum(len(set(px[px >= 0].tolist())) >= 2 for px in idx.reshape(-1, p.spp))
    print("pixels whose samples see two different spheres:", two)
    assert two >= 10


@pytest.mark.parametrize("name", ["medium", "large"])
def test_a_pixel_without_a_hit_has_the_linear_frames_value(name):
    p, sa = fc.params(name), fc.scene(name)
    got = fc.host_frame(name)
    lin, _ = binding.render_linear_host(lc.cscene(sa), lc.ccamera(sa), p)
    sky = got["hits"] == 0
    assert sky.sum() >= 10
    assert got["albedo"][sky].tobytes() == lin[sky].tobytes()
    # (and the pixels with a hit are not the linear frame's: the link is no identity of the two calls)
    assert got["albedo"][~sky].tobytes() != lin[~sky].tobytes()


def nan_camera(sa):
    """the scene's camera with an origin that is no number: every sample's ray is non-finite"""
    cam = np.array(sa.camera_array, np.float32)
    cam[0] = np.nan
    return es.ccamera(cam)


def test_a_pixel_whose_samples_are_all_non_finite_is_a_record_of_zeros():
    p, sa = fc.params("medium"), fc.scene("medium")
    got = binding.render_features_host(lc.cscene(sa), nan_camera(sa), p)
    assert got.shape == (p.height, p.width) and not got.view(np.uint8).any()


# ---- regions ----------------------------------------------------------------------------------------------------------------------------------


# the windows tests/region_cases.py names, of the large scene's 64 x 48 frame: the full frame, off-origin over four tiles, 2 x 2 across a tile
# corner, one whole tile, the last pixel (1 x 1 in the top-right corner), the top row (a full row), the last column (touching that corner)
REGION_FRAME = "large"
REGION_WINDOWS = rc.windows(*fc.FRAMES[REGION_FRAME][:2])


@pytest.mark.parametrize("win", REGION_WINDOWS, ids=lambda v: str(v).replace(" ", ""))
def test_a_region_is_the_crop_of_the_frame(win):
    p, sa = fc.params(REGION_FRAME), fc.scene(REGION_FRAME)
    whole = fc.host_frame(REGION_FRAME)
    got = fc.host_of(sa, p, win)
    assert got.shape == (win[3], win[2]) and got.tobytes() == fc.crop(whole, win).tobytes()
    # into a frame prefilled with 0xA5, rows out_stride = W apart: the window's records in place, every other byte still 0xA5
    x0, y0, ww, wh = win
    frame = np.frombuffer(bytes([fc.PREFILL]) * (p.height * p.width * 32), binding.FEATURE_DTYPE).reshape(p.height, p.width).copy()
    binding.render_features_host(lc.cscene(sa), lc.ccamera(sa), p, win, out=frame[y0:y0 + wh, x0:x0 + ww])
    assert fc.crop(frame, win).tobytes() == got.tobytes()
    outside = np.ones((p.height, p.width), bool)
    outside[y0:y0 + wh, x0:x0 + ww] = False
    assert (frame.view(np.uint8).reshape(p.height, p.width, 32)[outside] == fc.PREFILL).all()


def test_the_null_region_is_the_whole_frame():
    p, sa = fc.params("medium"), fc.scene("medium")
    assert fc.host_of(sa, p, (0, 0, p.width, p.height)).tobytes() == fc.host_frame("medium").tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------


def test_host_form_refusals_write_nothing():
    L = r1.lib()
    sa, p = fc.scene("medium"), fc.params("medium")
    out = np.frombuffer(bytes([fc.PREFILL]) * (p.height * p.width * 32), binding.FEATURE_DTYPE).copy()
    sc, cam, dst = C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.c_void_p(out.ctypes.data)
    ok, bad = binding.Region(2, 1, 4, 4, 0), binding.Region(30, 1, 4, 4, 0)
    for a in ((None, cam, C.byref(p), C.byref(ok), dst), (sc, None, C.byref(p), C.byref(ok), dst), (sc, cam, None, C.byref(ok), dst), (sc, cam, C.byref(p), C.byref(ok), None)):
        assert L.r1_render_features_host(*a) == binding.R1_EINVAL
    assert L.r1_render_features_host(sc, cam, C.byref(p), C.byref(bad), dst) == binding.R1_EINVAL
    assert "x0 + width" in L.r1_last_error().decode()
    assert L.r1_render_features_host(sc, cam, C.byref(p), C.byref(binding.Region(0, 0, 5, 5, 4)), dst) == binding.R1_EINVAL
    assert "out_stride" in L.r1_last_error().decode()
    for kw, says in ((dict(num_shards=2), "num_shards"), (dict(spp=0), "bad r1_params"), (dict(max_bounces=0), "bad r1_params"), (dict(tile_w=0), "bad r1_params"),
                     (dict(variant=9), "bad r1_params"), (dict(variant=binding.VARIANT_WAVEFRONT), "variant 6")):
        args = dict(width=p.width, height=p.height, spp=p.spp)
        args.update(kw)
        q = r1.make_params(**args)
        assert L.r1_render_features_host(sc, cam, C.byref(q), None, dst) == binding.R1_EINVAL, kw
        assert says in L.r1_last_error().decode(), (kw, L.r1_last_error())
    assert (out.view(np.uint8) == fc.PREFILL).all()


def test_device_forms_refuse_in_the_documented_order_without_a_device():
    """NULL ctx comes first, whatever else is wrong: the one refusal that needs no context (the rest of the order: tests/test_gpu_features.py)."""
    L = r1.lib()
    p = fc.params("medium")
    assert L.r1_render_features(None, None, None, None, None) == binding.R1_EINVAL and "ctx is NULL" in L.r1_last_error().decode()
    assert L.r1_render_features_device(None, C.byref(p), None, None, None) == binding.R1_EINVAL and "ctx is NULL" in L.r1_last_error().decode()


# ---- the drop-in program --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("args", [["--features", "--passes", "2"], ["--features", "--adaptive", "24"], ["--features", "--devices", "2"],
                                  ["--features", "--backend", "cpu-step12"], ["--features", "--backend", "cpu-step1"], ["--features", "--gather", "rccl"],
                                  ["--variant", "2", "--features"], ["--variant", "6", "--features"]], ids=lambda a: "_".join(a).replace("--", ""))
def test_program_refuses_features_with_what_it_cannot_serve_before_touching_a_device(tmp_path, args):
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", "32", "--height", "16", "--spp", "8", *args], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 1, (out.returncode, out.stderr)
    assert b"--features" in out.stderr
    assert b"cannot create HIP context" not in out.stderr
    assert not any(tmp_path.iterdir())  # (nothing rendered, nothing written)


# ---- the built library ------------------------------------------------------------------------------------------------------------------------


def test_census_of_the_feature_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    k = kernel_meta.collect(lib)
    own = sorted(n for n in k if "R1FeatureJob" in n)
    assert len(own) == 5, own
    assert sum("r1_query_tree_kernel" in n for n in own) == 2 and sum("r1_query_grid_kernel" in n for n in own) == 2
    assert sum("r1_query_reference_kernel" in n for n in own) == 1
    for name in own:
        a = k[name]
        print(name, {x: a[x] for x in ("vgpr", "sgpr", "sgpr_spill", "lane_moves", "insts", "lds")})  # (recorded in DESIGN.md §4.38)
        assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, (name, a)
        assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0, (name, a)
        assert int(a["vgpr"]) <= 64, (name, a["vgpr"])  # eight waves per SIMD fit: the launch's occupancy is what the LDS allows


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/check_features_host.cpp built with the host sources it drives (no sanitizer here: DESIGN.md §4.38 has that run)."""
    out = str(tmp_path_factory.mktemp("features_host") / "check_features_host")
    src = [os.path.join(ROOT, "tools", "check_features_host.cpp")] + [os.path.join(ROOT, "rays1bench_amd", "csrc", f) for f in
                                                                     ("r1_queries_host.cpp", "r1_host.cpp", "r1_bvh.cpp")]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-pthread", "-o", out])
    return out


def test_stand_alone_program(check_program):
    out = subprocess.run([check_program], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for says in ("70 pixels without a hit, 19 with some, 472 with all", "window 5,3 21x9 stride 29", "refusals wrote nothing"):
        assert says in out.stdout
