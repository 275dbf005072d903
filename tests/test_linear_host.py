"""CPU tests of linear frames (include/rays1.h): every new name is declared, exported and bound; r1_render_linear_host
followed by r1_quantise_linear gives the REFERENCE's own image bytes and ray totals on the frame fixtures; r1_render_linear_host equals the
value restated in numpy on the ORACLE's per-sample records, bit for bit; r1_quantise_linear and the PFM writer; the adaptive frame of
tests/linear_cases.py has, by the oracle's records alone, tiles that stop early and tiles that reach the cap; tools/check_linear_host.cpp.
What the device computes is checked in tests/test_gpu_linear.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import adaptive_rule as rule
import linear_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

NEW = ("r1_render_linear", "r1_render_linear_async", "r1_render_linear_device", "r1_pass_linear", "r1_render_adaptive_linear", "r1_quantise_linear",
       "r1_render_linear_host", "r1_pfm_write_rgb32f")


def test_every_new_name_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    names = {s[0] for s in binding.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(r1.lib(), name) and name in names, name
    assert re.search(r"\bint\s+r1_render_linear\s*\(\s*r1_context\s*\*\s*\w+\s*,\s*const\s+r1_params\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*,"
                     r"\s*double\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+r1_quantise_linear\s*\(\s*const\s+float\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"#define R1_ABI_VERSION 4\b", hdr)
    for m in ("render_linear", "render_linear_async", "render_linear_device", "pass_linear", "render_adaptive_linear"):
        assert callable(getattr(binding.Renderer, m, None)), m
    for f in ("render_linear_host", "quantise_linear", "pfm_write_rgb32f"):
        assert callable(getattr(binding, f, None)), f


@pytest.mark.parametrize("fixture,scene", [("frame_medium_77x45x3.bin", "scene_medium_77x45.bin"), ("frame_small_200x100x4.bin", "scene_small_200x100.bin"),
                                           ("frame_medium_200x100x4.bin", "scene_medium_200x100.bin"), ("frame_large_200x100x4.bin", "scene_large_200x100.bin")])
def test_host_frame_quantised_is_the_references_own_frame(fixture, scene):
    """identity 2 against the reference itself: its image bytes and its ray total"""
    g = r1o.read_golden(os.path.join(GOLD, fixture))
    w, h, spp, seed = g["hdr"].tolist()
    sa = r1o.SceneArrays.from_golden(r1o.read_golden(os.path.join(GOLD, scene)))
    lin, rays = binding.render_linear_host(lc.cscene(sa), lc.ccamera(sa), r1.make_params(w, h, spp, seed))
    assert lin.dtype == np.float32 and lin.shape == (h, w, 3)
    assert rays == int(g["rays"][0])
    q = binding.quantise_linear(lin)
    assert q.tobytes() == g["image"].tobytes(), int((q.reshape(-1) != g["image"]).sum())
    assert q.tobytes() == lc.quantise(lin).tobytes()


@pytest.mark.parametrize("name,w,h,spp", [f for f in lc.FRAMES if f[1:] != (200, 100, 4)], ids=lambda v: str(v))
def test_host_frame_is_the_sequential_sum_of_the_oracles_records(name, w, h, spp):
    """identity 1: bit for bit as uint32 views, and whatever the tile size"""
    rec, rays = lc.oracle_records(name, w, h, spp)
    want = lc.linear_of(rec)
    sa = lc.scene_arrays(name, w, h)
    for tw, th in lc.TILES:
        lin, got_rays = binding.render_linear_host(lc.cscene(sa), lc.ccamera(sa), r1.make_params(w, h, spp, lc.SEED, tile_w=tw, tile_h=th))
        assert got_rays == rays, (tw, th)
        assert lc.same_bits(lin, want), (tw, th, int((lin.view(np.uint32) != want.view(np.uint32)).sum()))
    if spp == 1:  # (float)(1.0f / 1) == 1: the frame is the records themselves
        assert lc.same_bits(want, np.float32(0) + rec[:, :, 0, :3])


def test_host_frame_refusals():
    L = r1.lib()
    sa = lc.scene_arrays("small", 16, 8)
    out = np.zeros((8, 16, 3), np.float32)
    rays = C.c_uint64()
    args = (out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(rays))
    p = r1.make_params(16, 8, 2)
    assert L.r1_render_linear_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p), *args) == binding.R1_OK
    assert L.r1_render_linear_host(None, C.byref(lc.ccamera(sa)), C.byref(p), *args) == binding.R1_EINVAL
    assert L.r1_render_linear_host(C.byref(lc.cscene(sa)), None, C.byref(p), *args) == binding.R1_EINVAL
    assert L.r1_render_linear_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), None, *args) == binding.R1_EINVAL
    assert L.r1_render_linear_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p), None, C.byref(rays)) == binding.R1_EINVAL
    p2 = r1.make_params(16, 8, 2, shard=0, num_shards=2)
    assert L.r1_render_linear_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p2), *args) == binding.R1_EINVAL
    assert "num_shards" in L.r1_last_error().decode()
    assert L.r1_render_linear_host(C.byref(lc.cscene(sa)), C.byref(lc.ccamera(sa)), C.byref(p), args[0], None) == binding.R1_OK


def test_quantise_linear():
    v = np.array([0.0, -0.0, 1.0, 0.25, 0.5, 1e-12, 0.99999994, 4.0, 1.0 / 65536.0], np.float32)
    want = [0, 0, 255, 127, 181, 0, 255, 255, 0]
    got = binding.quantise_linear(v)
    assert got.dtype == np.uint8 and got.tolist() == want
    assert got.tobytes() == lc.quantise(v).tobytes()
    # every float in [0, 1] that is a multiple of 2^-16, and its two neighbours: the host's sqrtf is numpy's correctly rounded one
    grid = (np.arange(0, 65537, dtype=np.float32) / np.float32(65536))
    for a in (grid, np.nextafter(grid, np.float32(2)), np.nextafter(grid[1:], np.float32(0))):
        assert binding.quantise_linear(a).tobytes() == lc.quantise(a).tobytes()
    assert binding.quantise_linear(np.zeros((0,), np.float32)).shape == (0,)
    assert binding.quantise_linear(np.full((3, 5, 3), 0.25, np.float32)).shape == (3, 5, 3)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf"), 3e38, -1e-45], ids=str)
def test_quantise_linear_refuses_what_int_cannot_hold(bad):
    L = r1.lib()
    v = np.array([0.5, bad, 0.5], np.float32)
    out = np.full(3, 7, np.uint8)
    rc = L.r1_quantise_linear(v.ctypes.data_as(C.POINTER(C.c_float)), 3, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == binding.R1_EINVAL and "value 1" in L.r1_last_error().decode()
    assert out.tolist() == [7, 7, 7]  # nothing written
    assert L.r1_quantise_linear(None, 3, out.ctypes.data_as(C.POINTER(C.c_uint8))) == binding.R1_EINVAL
    assert L.r1_quantise_linear(v.ctypes.data_as(C.POINTER(C.c_float)), 3, None) == binding.R1_EINVAL


def test_pfm_writer(tmp_path):
    w, h = 7, 5
    rng = np.random.default_rng(5)
    img = rng.random((h, w, 3), dtype=np.float32)
    img[0, 0] = [0.0, -0.0, 1.5]
    path = str(tmp_path / "frame.pfm")
    assert binding.pfm_write_rgb32f(path, w, h, img)
    data = open(path, "rb").read()
    head = b"PF\n7 5\n-1.0\n"
    assert data[:len(head)] == head and len(data) == len(head) + w * h * 12
    back = np.frombuffer(data[len(head):], "<f4").reshape(h, w, 3)  # row 0 of the file = row 0 of the frame = the bottom row: no flip
    assert lc.same_bits(back, img)
    assert img[0, 0].tolist() == [0.0, -0.0, 1.5]  # (the caller's pixels are not changed, unlike the TGA writer's)
    L = r1.lib()
    p = img.ctypes.data_as(C.POINTER(C.c_float))
    assert L.r1_pfm_write_rgb32f(None, w, h, p) == binding.R1_EINVAL
    assert L.r1_pfm_write_rgb32f(path.encode(), w, h, None) == binding.R1_EINVAL
    assert L.r1_pfm_write_rgb32f(path.encode(), 0, h, p) == binding.R1_EINVAL
    assert L.r1_pfm_write_rgb32f(str(tmp_path / "no" / "dir.pfm").encode(), w, h, p) == binding.R1_EINVAL


@pytest.mark.parametrize("tile", sorted(lc.ADAPTIVE_RULES), ids=lambda t: f"{t[0]}x{t[1]}")
def test_the_adaptive_frame_stops_some_tiles_and_caps_others(tile):
    """What tests/test_gpu_linear.py's adaptive case rests on, from the oracle's records alone: under the chosen rule the restated stopping
    rule ends at least one tile before the cap and runs at least one into it — and the linear crops of the two kinds differ in their
    scale, so a read-out with one n for every tile cannot pass."""
    name, w, h, cap = lc.ADAPTIVE_FRAME
    rec, _ = lc.oracle_records(name, w, h, cap)
    max_delta, mean_q8 = lc.ADAPTIVE_RULES[tile]
    rep, rays = rule.restate(rec, lc.ADAPTIVE_MIN, lc.ADAPTIVE_PASS, max_delta, mean_q8, *tile)
    early, capped = rep["spp"] < cap, rep["spp"] == cap
    assert early.any() and capped.any(), rule.histogram(rep)
    assert set(int(n) for n in rep["spp"]) <= set(rule.schedule(cap, lc.ADAPTIVE_MIN, lc.ADAPTIVE_PASS))
    boxes = rule.tile_boxes(w, h, *tile)
    t = int(np.nonzero(early)[0][0])
    x0, y0, x1, y1 = boxes[t]
    n = int(rep[t]["spp"])
    own, at_cap = lc.linear_of(rec, n)[y0:y1, x0:x1], lc.linear_of(rec, cap)[y0:y1, x0:x1]
    assert not lc.same_bits(own, at_cap)
    # (the scale alone tells them apart too: the sums of n samples times 1 / cap)
    sums = np.zeros_like(own)
    for s in range(n):
        sums = sums + rec[y0:y1, x0:x1, s, :3]
    assert not lc.same_bits(own, sums * (np.float32(1) / np.float32(cap)))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/check_linear_host.cpp built with the host sources it drives (no sanitizer here: DESIGN.md §4.32 has that run)."""
    out = str(tmp_path_factory.mktemp("linear_host") / "check_linear_host")
    src = [os.path.join(ROOT, "tools", "check_linear_host.cpp")] + [os.path.join(ROOT, "rays1bench_amd", "csrc", f) for f in
                                                                   ("r1_linear_host.cpp", "r1_queries_host.cpp", "r1_host.cpp", "r1_bvh.cpp")]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-pthread", "-o", out])
    return out


def test_stand_alone_program(check_program, tmp_path):
    pfm = tmp_path / "check.pfm"
    out = subprocess.run([check_program, str(pfm)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for says in ("linear frame 33x17x2", "quantised: 1683 bytes", "pfm: header and 6732 bytes read back"):
        assert says in out.stdout
    # the file it wrote is the library's frame for those params, read back here
    sc = r1.create_medium_scene(33, 17)
    sa = r1o.SceneArrays.from_c(sc.spheres, sc.camera)
    lin, _ = binding.render_linear_host(lc.cscene(sa), lc.ccamera(sa), r1.make_params(33, 17, 2))
    data = pfm.read_bytes()
    assert data.startswith(b"PF\n33 17\n-1.0\n") and data[len(b"PF\n33 17\n-1.0\n"):] == lin.astype("<f4").tobytes()


@pytest.mark.parametrize("args", [["--linear", "--passes", "2"], ["--linear", "--adaptive", "24"], ["--linear", "--devices", "2"], ["--linear", "--backend", "cpu-step12"],
                                  ["--linear", "--gather", "rccl"], ["--adaptive", "24", "--linear"]], ids=lambda a: "_".join(a).replace("--", ""))
def test_program_rejects_bad_linear_options_before_touching_a_device(tmp_path, args):
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", "32", "--height", "16", "--spp", "8", *args], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 1, (out.returncode, out.stderr)
    assert b"--linear" in out.stderr
    assert b"cannot create HIP context" not in out.stderr
    assert not any(tmp_path.iterdir())  # (nothing rendered, nothing written)
