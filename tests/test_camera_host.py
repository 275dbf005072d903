"""CPU tests of camera paths (r1_set_camera, r1_render_path_async, r1_camera_look_at, r1_host_scene_view): the MODE 5
kernels' census (six r1_path_kernel instances, each within the register budget of its frame-batch sibling), the public Camera::init
against the reference's fixtures, the refusals that need no device, and the drop-in program's --orbit option.  Pixels and ray counts
are checked on the GPU (tests/test_gpu_camera_path.py)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
MAKE = {"small": r1.create_small_scene, "medium": r1.create_medium_scene, "large": r1.create_large_scene}
# the scene / size pairs tests/test_host.py lists
SIZES = {"small": [(1200, 800), (1280, 720), (200, 100), (80, 60), (70, 50)],
         "medium": [(1200, 800), (1280, 720), (200, 100), (80, 60), (77, 45)],
         "large": [(1200, 800), (1280, 720), (200, 100), (80, 60), (1920, 1080), (320, 200)]}


def waves_per_simd(vgpr, sgpr):
    """Waves of one kernel a gfx950 SIMD holds by its registers: 512 VGPRs per lane allocated in blocks of 8, 800 SGPRs allocated in
    blocks of 16 (the figures DESIGN.md §4.4 and r1_trace.hpp's TraceWaves budget with), at most 8."""
    v = (int(vgpr) + 7) // 8 * 8
    s = (int(sgpr) + 15) // 16 * 16
    return min(8, 512 // v, 800 // s)


def test_census_of_the_path_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    k = kernel_meta.collect(lib)
    paths = sorted(n for n in k if "r1_path_kernel" in n)
    assert len(paths) == 6, paths
    # r1_path_kernel<VARIANT, BIG> and its MODE 3 sibling: r1_trace_kernel<VARIANT, false, BIG, 3>, or r1_grid_kernel<false, BIG, 3>
    seen = set()
    for name in paths:
        m = re.search(r"r1_path_kernelILi(\d)ELb([01])E", name)
        assert m, name
        variant, big = int(m.group(1)), m.group(2)
        seen.add((variant, big))
        tag = f"r1_grid_kernelILb0ELb{big}ELi3E" if variant == 7 else f"r1_trace_kernelILi{variant}ELb0ELb{big}ELi3E"
        sib = [n for n in k if tag in n]
        assert len(sib) == 1, (name, sib)
        a, b = k[name], k[sib[0]]
        print(name, {x: a[x] for x in ("vgpr", "sgpr", "sgpr_spill", "lane_moves", "insts")}, "sibling", {x: b[x] for x in ("vgpr", "sgpr", "sgpr_spill", "lane_moves", "insts")})
        assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, (name, a)
        assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0, (name, a)
        assert waves_per_simd(a["vgpr"], a["sgpr"]) >= waves_per_simd(b["vgpr"], b["sgpr"]), (name, a["vgpr"], a["sgpr"], b["vgpr"], b["sgpr"])
        assert a["lds"] == b["lds"], (name, a["lds"], b["lds"])  # (and the same workgroups per CU by LDS)
        if variant == 4 and big == "0":
            assert int(a["vgpr"]) <= 72, name
        if variant == 4 and big == "1":
            assert int(a["vgpr"]) <= 64 and int(a["sgpr"]) <= 96, name
    assert seen == {(v, b) for v in (2, 4, 7) for b in ("0", "1")}


def test_waves_helper_on_the_known_budgets():
    assert waves_per_simd(72, 94) == 7 and waves_per_simd(73, 94) == 6 and waves_per_simd(64, 96) == 8 and waves_per_simd(64, 97) == 7
    assert waves_per_simd(96, 106) == 5


@pytest.mark.parametrize("name", ["small", "medium", "large"])
def test_look_at_reproduces_every_camera_fixture(name):
    for (w, h) in SIZES[name]:
        g = r1o.read_golden(os.path.join(GOLD, f"scene_{name}_{w}x{h}.bin"))
        sc = MAKE[name](w, h)
        v = sc.view()
        cam = r1.camera_look_at(v["lookfrom"], v["lookat"], v["vup"], v["vfov"], v["aspect"], v["aperture"], v["focus_dist"])
        assert r1.camera_to_array(cam).tobytes() == g["camera"].tobytes(), (name, w, h)
        assert r1.camera_to_array(binding.orbit_cameras(sc, 5)[0]).tobytes() == g["camera"].tobytes(), (name, w, h)
        sc.close()


def test_view_is_the_references_arguments():
    f32 = np.float32
    want = {"small": ((2, 1, 2), f32(0.1), 5), "medium": ((0, 2, 3), f32(0.1) * f32(0.2), 3), "large": ((3, 8, 15), f32(0.1), 10)}
    for name, (lookfrom, aperture, focus) in want.items():
        v = MAKE[name](1200, 800).view()
        assert v["lookfrom"].tolist() == list(lookfrom) and v["lookat"].tolist() == [0, 0, 0] and v["vup"].tolist() == [0, 1, 0], name
        assert v["vfov"] == 60 and v["aperture"] == aperture and v["focus_dist"] == focus, (name, v)
        assert v["aperture"].dtype == np.float32 and v["aspect"] == f32(1200) / f32(800)
    assert abs(float(want["medium"][1]) - 0.02) < 1e-8
    g = r1.create_grid_scene(256, 160, 400, 250).view()
    assert g["lookfrom"].tolist() == [3, 8, 15]


def test_look_at_computes_nans_rather_than_refusing():
    cam = r1.camera_look_at((1, 2, 3), (1, 2, 3), (0, 1, 0), 60, 1.5, 0.1, 5)  # lookfrom == lookat: unit(0) = 0 * inf
    a = r1.camera_to_array(cam)
    assert np.isnan(a[18:21]).all() and a[21] == np.float32(0.1) / 2 and a[:3].tolist() == [1, 2, 3]


def test_null_arguments_are_einval_and_named():
    L = r1.lib()
    v3 = (C.c_float * 3)(0, 1, 0)
    cam = binding.CCamera()
    for i, arg in enumerate(("lookfrom", "lookat", "vup")):
        a = [v3, v3, v3]
        a[i] = None
        assert L.r1_camera_look_at(a[0], a[1], a[2], 60, 1.5, 0.1, 5, C.byref(cam)) == binding.R1_EINVAL
        assert arg in L.r1_last_error().decode()
    assert L.r1_camera_look_at(v3, v3, v3, 60, 1.5, 0.1, 5, None) == binding.R1_EINVAL
    assert "out" in L.r1_last_error().decode()
    sc = r1.create_small_scene(64, 32)
    f = [C.c_float() for _ in range(3)]
    ok = [sc._h, v3, v3, v3, C.byref(f[0]), C.byref(f[1]), C.byref(f[2])]
    for i, arg in enumerate(("scene", "lookfrom", "lookat", "vup", "vfov_degrees", "aperture", "focus_dist")):
        a = list(ok)
        a[i] = None
        assert L.r1_host_scene_view(*a) == binding.R1_EINVAL
        assert arg in L.r1_last_error().decode(), arg
    assert L.r1_host_scene_view(*ok) == binding.R1_OK
    p = r1.make_params(64, 32, 2)
    assert L.r1_set_camera(None, C.byref(cam)) == binding.R1_EINVAL
    assert "ctx" in L.r1_last_error().decode()
    assert L.r1_multi_set_camera(None, C.byref(cam)) == binding.R1_EINVAL
    assert "multi" in L.r1_last_error().decode()
    assert L.r1_render_path_async(None, C.byref(p), 1, 0, C.byref(cam), None, None) == binding.R1_EINVAL
    assert "ctx" in L.r1_last_error().decode()


def test_new_entry_points_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    names = {s[0] for s in binding.SYMBOLS}
    for fn in ("r1_camera_look_at", "r1_host_scene_view", "r1_set_camera", "r1_multi_set_camera", "r1_render_path_async"):
        assert re.search(rf"\bint\s+{fn}\s*\(", hdr), fn
        assert hasattr(r1.lib(), fn) and fn in names, fn
    assert re.search(r"#define R1_ABI_VERSION 4\b", hdr)
    for cls, meth in ((binding.Renderer, "set_camera"), (binding.Renderer, "render_path_async"), (binding.MultiRenderer, "set_camera"), (binding.Scene, "view")):
        assert callable(getattr(cls, meth, None)), meth
    assert callable(binding.camera_look_at)


def test_a_c99_program_uses_the_camera_entry_points(tmp_path):
    src = tmp_path / "cam.c"
    src.write_text('#include "rays1.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '    r1_params p = {64, 32, 4, 50, 1, 32, 32, 0, 1, R1_VARIANT_DEFAULT};\n'
                   '    r1_host_scene *hs = NULL;\n'
                   '    float from[3], at[3], up[3], vfov, aperture, focus;\n'
                   '    r1_camera cam;\n'
                   '    const r1_camera *own;\n'
                   '    int i, same = 1;\n'
                   '    if (r1_host_scene_create(R1_SCENE_LARGE, 64, 32, 0, 0, &hs) != R1_OK) return 2;\n'
                   '    if (r1_host_scene_view(hs, from, at, up, &vfov, &aperture, &focus) != R1_OK) return 3;\n'
                   '    if (r1_camera_look_at(from, at, up, vfov, 64.0f / 32.0f, aperture, focus, &cam) != R1_OK) return 4;\n'
                   '    own = r1_host_scene_camera(hs);\n'
                   '    for (i = 0; i < 3; ++i) same = same && cam.lower_left[i] == own->lower_left[i] && cam.w[i] == own->w[i];\n'
                   '    if (!same || cam.lens_radius != own->lens_radius) return 5;\n'
                   '    if (r1_set_camera(NULL, &cam) != R1_EINVAL || r1_multi_set_camera(NULL, &cam) != R1_EINVAL) return 6;\n'
                   '    if (r1_render_path_async(NULL, &p, 1, 0u, &cam, NULL, NULL) != R1_EINVAL) return 7;\n'
                   '    r1_host_scene_destroy(hs);\n'
                   '    printf("ok\\n");\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "cam"
    libdir = os.path.join(ROOT, "rays1bench_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lrays1", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("args", [["--orbit", "0"], ["--orbit", "-1"], ["--orbit", "4", "--passes", "2", "--spp", "4"], ["--orbit", "4", "--devices", "2"],
                                  ["--orbit", "4", "--gather", "rccl"], ["--orbit", "4", "--backend", "cpu-step12"], ["--orbit", "4", "--backend", "cpu-step1"]],
                         ids=["zero", "negative", "passes", "devices", "gather-rccl", "cpu-step12", "cpu-step1"])
def test_program_rejects_bad_orbit_before_touching_a_device(tmp_path, args):
    out = subprocess.run([EXE, "--width", "32", "--height", "16", *args], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 1, (out.returncode, out.stderr)
    assert b"--orbit" in out.stderr
    assert b"cannot create HIP context" not in out.stderr
    assert not any(tmp_path.iterdir())  # (nothing rendered, nothing written)


def test_the_oracle_renders_an_orbit_camera_differently():
    """Guards the GPU tests' fixtures against a degenerate orbit: a turned camera is a valid camera to the oracle, and it sees another image."""
    w, h = 40, 24
    for name in ("small", "large"):
        sc = MAKE[name](w, h)
        cams = binding.orbit_cameras(sc, 7)
        arrays = sc.arrays()
        p = r1o.make_params(w, h, 2, 321)
        own = r1o.render_frame(r1o.SceneArrays(arrays, sc.camera_array()), p)
        first = r1o.render_frame(r1o.SceneArrays(arrays, r1.camera_to_array(cams[0])), p)
        assert first[1] == own[1] and first[0].tobytes() == own[0].tobytes(), name
        images = {own[0].tobytes()}
        for f in range(1, 7):
            a = r1.camera_to_array(cams[f])
            assert np.isfinite(a).all(), (name, f)
            img, rays, _ = r1o.render_frame(r1o.SceneArrays(arrays, a), p)
            assert rays >= w * h * 2
            images.add(img.tobytes())
        assert len(images) == 7, name
