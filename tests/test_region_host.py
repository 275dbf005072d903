"""CPU tests of region renders (include/rays1.h): every new name is declared, exported and bound; r1_region_check's table; the host
form r1_render_region_host followed by r1_quantise_linear gives the crop of the REFERENCE's own image bytes on the frame fixtures, with the count of
the oracle's records over the window, and leaves the bytes outside a strided window alone; on a 40 000 x 40 000 x 2 frame, which no single launch
holds, it equals the ORACLE's per-sample restatement; the drop-in program refuses --region with what it cannot serve; the census of the region
kernels in the built library; tools/check_region_host.cpp.  What the device computes is checked in tests/test_gpu_region.py.
Every comparison is tobytes() equality."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import linear_cases as lc
import region_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

NEW = ("r1_region_check", "r1_render_region", "r1_render_region_samples", "r1_render_region_linear", "r1_render_region_device", "r1_render_region_host")


def test_every_new_name_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    names = {s[0] for s in binding.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(r1.lib(), name) and name in names, name
    assert re.search(r"typedef\s+struct\s+r1_region\s*\{\s*int32_t\s+x0\s*,\s*y0\s*;\s*int32_t\s+width\s*,\s*height\s*;\s*int32_t\s+out_stride\s*;\s*\}\s*r1_region\s*;", hdr)
    assert re.search(r"\bint\s+r1_region_check\s*\(\s*const\s+r1_params\s*\*\s*\w+\s*,\s*const\s+r1_region\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+r1_render_region_device\s*\(\s*r1_context\s*\*\s*\w+\s*,\s*const\s+r1_params\s*\*\s*\w+\s*,\s*const\s+r1_region\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"#define R1_ABI_VERSION 4\b", hdr) and r1.lib().r1_abi_version() == 4
    assert C.sizeof(binding.Region) == 20
    for m in ("render_region", "render_region_samples", "render_region_linear", "render_region_device"):
        assert callable(getattr(binding.Renderer, m, None)), m
    for f in ("region_check", "render_region_host"):
        assert callable(getattr(binding, f, None)), f


# ---- r1_region_check ------------------------------------------------------------------------------------------------------------------------

W, H, SPP = 77, 45, 3


def refusal(params, region, out_stride=0):
    """(code, text) of r1_region_check's refusal, or (R1_OK, "")"""
    try:
        binding.region_check(params, region, out_stride)
    except binding.R1Error as e:
        return e.code, str(e)
    return binding.R1_OK, ""


@pytest.mark.parametrize("frame,region", [((W, H, SPP), (0, 0, W, H)), ((W, H, SPP), (W - 1, H - 1, 1, 1)), (rc.HUGE, (39991, 39993, 9, 7)), (rc.HUGE, (0, 0, 8, 8))],
                         ids=["full_frame", "last_pixel", "9x7_of_40000x40000x2", "8x8_of_40000x40000x2"])
def test_region_check_accepts(frame, region):
    assert refusal(r1.make_params(*frame), region) == (binding.R1_OK, "")
    assert refusal(r1.make_params(*frame), region, out_stride=region[2]) == (binding.R1_OK, "")
    assert refusal(r1.make_params(*frame), region, out_stride=frame[0]) == (binding.R1_OK, "")


def test_the_huge_frame_is_no_frame_of_r1_render():
    assert r1.lib().r1_params_check(C.byref(r1.make_params(*rc.HUGE))) == binding.R1_ELIMIT


@pytest.mark.parametrize("region,stride,names", [((-1, 0, 3, 3), 0, "x0"), ((0, -1, 3, 3), 0, "y0"), ((0, 0, 0, 3), 0, "width"), ((0, 0, 3, 0), 0, "height"),
                                                 ((W - 2, 0, 3, 3), 0, "x0 + width"), ((0, H - 2, 3, 3), 0, "y0 + height"), ((0, 0, 5, 5), 4, "out_stride"),
                                                 ((0, 0, 5, 5), -1, "out_stride")], ids=lambda v: str(v).replace(" ", ""))
def test_region_check_names_the_offending_field(region, stride, names):
    code, text = refusal(r1.make_params(W, H, SPP), region, stride)
    assert code == binding.R1_EINVAL and names in text, text
    # (x0 + width == W + 1 exactly, out_stride == width - 1 exactly: the first value that is wrong)
    assert refusal(r1.make_params(W, H, SPP), (W - 3, H - 3, 3, 3), 3) == (binding.R1_OK, "")


def test_region_check_refuses_shards_and_the_variants_without_a_pass_build():
    code, text = refusal(r1.make_params(W, H, SPP, shard=0, num_shards=2), (0, 0, 8, 8))
    assert code == binding.R1_EINVAL and "num_shards" in text
    for v in rc.REFUSED_VARIANTS:
        code, text = refusal(r1.make_params(W, H, SPP, variant=v), (0, 0, 8, 8))
        assert code == binding.R1_EINVAL and f"variant {v}" in text, (v, text)
    assert sorted(rc.REFUSED_VARIANTS) == [3, 5, 6, 8]
    for v in rc.VARIANTS.values():
        assert refusal(r1.make_params(W, H, SPP, variant=v), (0, 0, 8, 8))[0] == binding.R1_OK
    # every other check of r1_params_check still holds
    for bad in (dict(spp=0), dict(tile_w=0), dict(max_bounces=0), dict(variant=9)):
        kw = dict(width=W, height=H, spp=SPP)
        kw.update(bad)
        assert refusal(r1.make_params(**kw), (0, 0, 8, 8))[0] == binding.R1_EINVAL, bad


def test_region_check_limits():
    # W * H >= 2^31: the pixel index would not be an int
    assert 46341 * 46341 >= 2 ** 31 > 46340 * 46340
    code, text = refusal(r1.make_params(46341, 46341, 1), (0, 0, 1, 1))
    assert code == binding.R1_ELIMIT and "2^31" in text
    assert refusal(r1.make_params(46340, 46340, 1), (0, 0, 1, 1))[0] == binding.R1_OK
    # a region of 2^31 samples, and one sample fewer than a launch holds
    assert refusal(r1.make_params(*rc.HUGE), (0, 0, 32768, 32768))[0] == binding.R1_ELIMIT
    assert refusal(r1.make_params(40000, 40000, 1), (0, 0, 32768, 32768))[0] == binding.R1_OK
    # the padded slots of its tiles: 33 x 33 pixels in 32 x 32 tiles are four tiles
    assert refusal(r1.make_params(40000, 40000, 2 ** 19 - 1), (0, 0, 33, 33))[0] == binding.R1_OK          # 4096 * (2^19 - 1) < 2^31
    assert refusal(r1.make_params(40000, 40000, 2 ** 19), (0, 0, 33, 33))[0] == binding.R1_ELIMIT           # 1089 * 2^19 < 2^31 <= 4096 * 2^19


# ---- the host form against the reference's fixtures ----------------------------------------------------------------------------------------

FIXTURES = {"medium": ("frame_medium_77x45x3.bin", "scene_medium_77x45.bin"), "large": ("frame_large_200x100x4.bin", "scene_large_200x100.bin")}
FIXTURE_WINDOWS = {"medium": [(0, 0, 77, 45), (5, 3, 33, 33), (76, 44, 1, 1), (0, 44, 77, 1), (76, 0, 1, 45)],
                   "large": [(5, 3, 33, 33), (199, 99, 1, 1), (0, 99, 200, 1), (199, 0, 1, 100)]}
_fixture_cache = {}


def fixture(name):
    """(w, h, spp, seed, the reference's image (h, w, 3), the scene, the oracle's records (h, w, spp, 4)); read and computed once, left unchanged"""
    if name not in _fixture_cache:
        g = r1o.read_golden(os.path.join(GOLD, FIXTURES[name][0]))
        w, h, spp, seed = (int(v) for v in g["hdr"].tolist())
        sa = r1o.SceneArrays.from_golden(r1o.read_golden(os.path.join(GOLD, FIXTURES[name][1])))
        oimg, orays, samples = r1o.render_frame(sa, r1o.make_params(w, h, spp, seed), want_samples=True)
        assert oimg.tobytes() == g["image"].tobytes() and orays == int(g["rays"][0])  # (the oracle is pinned to the reference)
        image = g["image"].reshape(h, w, 3)
        rec = rc.records_of(samples, w, h, spp)
        image.setflags(write=False), rec.setflags(write=False)
        _fixture_cache[name] = (w, h, spp, seed, image, sa, rec)
    return _fixture_cache[name]


@pytest.mark.parametrize("name,win", [(n, w) for n in FIXTURES for w in FIXTURE_WINDOWS[n]], ids=lambda v: str(v).replace(" ", ""))
def test_host_window_quantised_is_the_crop_of_the_references_frame(name, win):
    w, h, spp, seed, image, sa, rec = fixture(name)
    p = r1.make_params(w, h, spp, seed)
    lin, rays = binding.render_region_host(lc.cscene(sa), lc.ccamera(sa), p, win)
    assert lin.dtype == np.float32 and lin.shape == (win[3], win[2], 3)
    assert binding.quantise_linear(lin).tobytes() == rc.crop(image, win).tobytes()
    assert rays == rc.count_of(rc.crop(rec, win))
    assert lin.tobytes() == lc.linear_of(rc.crop(rec, win)).tobytes()
    # with out_stride = W into a frame pre-filled with 0xCD: the window's bytes in place, every other byte still 0xCD
    frame = np.frombuffer(bytes([rc.PREFILL]) * (h * w * 12), np.float32).reshape(h, w, 3).copy()
    x0, y0, ww, wh = win
    _, rays2 = binding.render_region_host(lc.cscene(sa), lc.ccamera(sa), p, win, out=frame[y0:y0 + wh, x0:x0 + ww])
    assert rays2 == rays and rc.crop(frame, win).tobytes() == lin.tobytes()
    outside = np.ones((h, w), bool)
    outside[y0:y0 + wh, x0:x0 + ww] = False
    assert (frame.view(np.uint8).reshape(h, w, 12)[outside] == rc.PREFILL).all()


def test_host_window_does_not_depend_on_the_tile_fields():
    w, h, spp, seed, image, sa, rec = fixture("medium")
    win = (5, 3, 33, 33)
    want = lc.linear_of(rc.crop(rec, win)).tobytes()
    for tw, th in rc.TILINGS:
        lin, _ = binding.render_region_host(lc.cscene(sa), lc.ccamera(sa), r1.make_params(w, h, spp, seed, tile_w=tw, tile_h=th), win)
        assert lin.tobytes() == want, (tw, th)


# ---- the host form against the oracle, on a frame no launch holds ---------------------------------------------------------------------------


@pytest.mark.parametrize("win", rc.HUGE_WINDOWS, ids=lambda v: str(v).replace(" ", ""))
def test_host_window_of_the_huge_frame_is_the_oracles_restatement(win):
    w, h, spp = rc.HUGE
    sc = r1.create_large_scene(w, h)
    sa = r1o.SceneArrays.from_c(sc.spheres, sc.camera)
    rec, lin, q, rays = rc.oracle_window(sa, w, h, spp, win)
    got, got_rays = binding.render_region_host(lc.cscene(sa), lc.ccamera(sa), r1.make_params(w, h, spp, rc.SEED), win)
    assert got.tobytes() == lin.tobytes() and got_rays == rays
    assert binding.quantise_linear(got).tobytes() == q.tobytes()
    # (the frame's geometry matters: the same window of a frame of the window's own size is another picture)
    small, _ = binding.render_region_host(lc.cscene(sa), lc.ccamera(sa), r1.make_params(win[2], win[3], spp, rc.SEED), (0, 0, win[2], win[3]))
    assert small.tobytes() != got.tobytes()


def test_host_form_refusals_write_nothing():
    L = r1.lib()
    sa = lc.scene_arrays("small", 16, 8)
    out = np.full((8, 16, 3), -7.0, np.float32)
    rays = C.c_uint64()
    p = r1.make_params(16, 8, 2)
    ok, bad = binding.Region(2, 1, 4, 4, 0), binding.Region(14, 1, 4, 4, 0)
    args = (C.c_void_p(out.ctypes.data), C.byref(rays))
    assert L.r1_render_region_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p), C.byref(bad), *args) == binding.R1_EINVAL
    assert "x0 + width" in L.r1_last_error().decode()
    for a in ((None, C.byref(lc.ccamera(sa)), C.byref(p), C.byref(ok)), (C.byref(lc.cscene(sa)), None, C.byref(p), C.byref(ok)),
              (C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), None, C.byref(ok)), (C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p), None)):
        assert L.r1_render_region_host(*a, *args) == binding.R1_EINVAL
    assert L.r1_render_region_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p), C.byref(ok), None, C.byref(rays)) == binding.R1_EINVAL
    assert (out == -7.0).all()
    assert L.r1_render_region_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p), C.byref(ok), args[0], None) == binding.R1_OK
    assert (out.reshape(-1)[:48] != -7.0).all() and (out.reshape(-1)[48:] == -7.0).all()


# ---- the drop-in program --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("args", [["--region", "0,0,8,8", "--passes", "2"], ["--region", "0,0,8,8", "--adaptive", "24"], ["--region", "0,0,8,8", "--devices", "2"],
                                  ["--region", "0,0,8,8", "--backend", "cpu-step12"], ["--region", "0,0,8,8", "--backend", "cpu-step1"],
                                  ["--region", "0,0,8,8", "--gather", "rccl"], ["--linear", "--region", "0,0,8,8"], ["--region", "0,0,8"], ["--region", "0,0,8,8,8"],
                                  ["--region", "a,b,c,d"], ["--region", "30,0,8,8"], ["--region", "0,0,0,8"], ["--variant", "6", "--region", "0,0,8,8"], ["--region"]],
                         ids=lambda a: "_".join(a).replace("--", ""))
def test_program_refuses_region_with_what_it_cannot_serve_before_touching_a_device(tmp_path, args):
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", "32", "--height", "16", "--spp", "8", *args], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 1, (out.returncode, out.stderr)
    assert b"--region" in out.stderr
    assert b"cannot create HIP context" not in out.stderr
    assert not any(tmp_path.iterdir())  # (nothing rendered, nothing written)


# ---- the built library ------------------------------------------------------------------------------------------------------------------------


def test_census_of_the_region_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    k = kernel_meta.collect(lib)
    twins = sorted(n for n in k if "r1_region_kernel" in n)
    passes = sorted(n for n in k if "r1_pass_kernel" in n)
    assert len(twins) == len(passes) == 8, (twins, passes)
    seen = set()
    for name in twins:
        # (the name r1_pick's table is pinned by, tests/test_builds_host.py, does not match the twins)
        assert not re.search(r"r1_(trace|grid|pass|path|adaptive)_kernel", name), name
        m = re.search(r"r1_region_kernelILi(\d)ELb([01])E", name)
        assert m, name
        seen.add((int(m.group(1)), m.group(2)))
        sib = [n for n in passes if f"r1_pass_kernelILi{m.group(1)}ELb{m.group(2)}E" in n]
        assert len(sib) == 1, (name, sib)
        a, b = k[name], k[sib[0]]
        keys = ("vgpr", "sgpr", "sgpr_spill", "lane_moves", "insts", "lds")
        print(name, {x: a[x] for x in keys}, "sibling", {x: b[x] for x in keys})  # (SGPRs and lane moves: recorded in DESIGN.md §4.37, not capped)
        assert int(a["vgpr"]) <= int(b["vgpr"]), (name, a["vgpr"], b["vgpr"])
        assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0, (name, a)
        assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, (name, a)
        assert a["lds"] == b["lds"], (name, a["lds"], b["lds"])  # (the sibling's occupancy sizes the twin's grid)
    assert seen == {(v, b) for v in (1, 2, 4, 7) for b in ("0", "1")}
    own = [n for n in k if "r1_resolve_region_kernel" in n]
    assert len(own) == 1, own
    a = k[own[0]]
    assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, a
    assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0 and int(a["sgpr_spill"]) == 0, a


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/check_region_host.cpp built with the host sources it drives (no sanitizer here: DESIGN.md §4.37 has that run)."""
    out = str(tmp_path_factory.mktemp("region_host") / "check_region_host")
    src = [os.path.join(ROOT, "tools", "check_region_host.cpp")] + [os.path.join(ROOT, "rays1bench_amd", "csrc", f) for f in
                                                                   ("r1_linear_host.cpp", "r1_queries_host.cpp", "r1_host.cpp", "r1_bvh.cpp")]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-pthread", "-o", out])
    return out


def test_stand_alone_program(check_program):
    out = subprocess.run([check_program], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for says in ("rules: 7 windows refused", "window 5,3 21x9 stride 29", "full window and four pasted quadrants", "refusals wrote nothing"):
        assert says in out.stdout
