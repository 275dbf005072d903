"""CPU tests of the product's host side: the C-ABI library loads and exports every symbol
include/rays1.h declares, the scene builders reproduce the reference's scenes bit-for-bit
(fixtures dumped from the reference by oracle/gen_golden.py), output formats match
common.h, and compute entry points fail loudly without a GPU."""
import ctypes as C
import os
import sys
import re

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "rays1.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(r1_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    L = r1.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in include/rays1.h but not exported"
    assert declared == {s[0] for s in binding.SYMBOLS}
    assert L.r1_abi_version() == 4


def test_struct_layouts_match_header():
    # sizes the C compiler gives the PODs of rays1.h (pointers 8 B, 4-byte scalars)
    assert C.sizeof(binding.CScene) == 8 + 10 * 8
    assert C.sizeof(binding.CCamera) == 22 * 4
    assert C.sizeof(binding.Params) == 10 * 4
    assert C.sizeof(r1o.Scene) == C.sizeof(binding.CScene)
    assert C.sizeof(r1o.Params) == C.sizeof(binding.Params)


SIZES = {"small": [(1200, 800), (1280, 720), (200, 100), (80, 60), (70, 50)],
         "medium": [(1200, 800), (1280, 720), (200, 100), (80, 60), (77, 45)],
         "large": [(1200, 800), (1280, 720), (200, 100), (80, 60), (1920, 1080), (320, 200)]}


@pytest.mark.parametrize("name", ["small", "medium", "large"])
def test_scene_builders_match_reference_bitwise(name):
    make = {"small": r1.create_small_scene, "medium": r1.create_medium_scene, "large": r1.create_large_scene}[name]
    for (w, h) in SIZES[name]:
        g = r1o.read_golden(os.path.join(GOLD, f"scene_{name}_{w}x{h}.bin"))
        sc = make(w, h)
        a = sc.arrays()
        assert sc.count == int(g["dims"][2]) == {"small": 8, "medium": 48, "large": 488}[name]
        for gk, fk in r1o.GOLD_TO_FIELD.items():
            assert a[fk].tobytes() == g[gk].tobytes(), (name, w, h, fk)
        assert sc.camera_array().tobytes() == g["camera"].tobytes(), (name, w, h)
        sc.close()


def test_large_scene_facts_from_survey():
    sc = r1.create_large_scene(1200, 800)
    a = sc.arrays()
    assert (a["center_x"][0], a["center_z"][0]) == (np.float32(-16.5), np.float32(-8.8))
    assert a["radius_sq"][0] == np.float32(0.45) * np.float32(0.45)
    assert np.allclose([a["albedo_r"][1], a["albedo_g"][1], a["albedo_b"][1]], [0.31764707, 0.93333334, 0.86666668], atol=1e-7)
    assert (a["center_x"][483], a["center_y"][483], a["radius_sq"][483]) == (-5, 3, 4)
    assert (a["inv_radius"][484:] == 0).all() and (a["mat_type"][484:] == 255).all()
    assert (a["center_x"][484:] == np.float32(999999999)).all()
    # SURVEY.md §8c quotes the lower-left corner of the 1280x720 camera
    assert np.allclose(r1.create_large_scene(1280, 720).camera_array()[3:6], [-8.27781, -1.750378, 10.947312], atol=1e-5)


def test_grid_scene_reduces_to_large_and_scales():
    big = r1.create_grid_scene(1200, 800, 30, 16)
    ref = r1.create_large_scene(1200, 800)
    for k, v in ref.arrays().items():
        assert big.arrays()[k].tobytes() == v.tobytes(), k
    g = r1.create_grid_scene(1920, 1080, 400, 250)
    a = g.arrays()
    assert g.count == 100008 and int((a["inv_radius"] != 0).sum()) == 100004
    assert abs(a["center_x"][:100000].min() + 16.5) < 1e-3 and a["radius_sq"][0] < 0.002
    assert set(np.unique(a["mat_type"])) == {0, 1, 2, 255}


def test_tile_and_shard_arithmetic():
    p = r1.make_params(1200, 800, 10)
    assert binding.tile_count(p) == (950, 950)  # 38 x 25 tiles
    assert binding.shard_block_bytes(p) == 950 * 32 * 32 * 3
    p8 = r1.make_params(1200, 800, 10, shard=3, num_shards=8)
    assert binding.tile_count(p8) == (950, 119)
    assert binding.shard_block_bytes(p8) == 119 * 32 * 32 * 3
    bad = r1.make_params(1200, 800, 10, shard=8, num_shards=8)
    with pytest.raises(r1.R1Error) as e:
        binding.tile_count(bad)
    assert e.value.code == binding.R1_EINVAL
    with pytest.raises(r1.R1Error) as e:
        binding.tile_count(r1.make_params(60000, 60000, 10))
    assert e.value.code == binding.R1_ELIMIT


def test_tga_and_log_results_formats(tmp_path):
    os.chdir(tmp_path)
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    keep = img.copy()
    r1.tga_write_rgb24("out_x.tga", 7, 5, img)
    assert open("out_x.tga", "rb").read() == r1o.tga_bytes(keep)
    assert (img == keep[:, :, ::-1]).all()  # caller's buffer left R/B-swapped (common.h:108-114)
    r1.log_results("hip", "large", [r1.RESULT(0.5, 27_000_000), r1.RESULT(1.5, 27_000_002)])
    # common.h:70-73 format, parsed by update_readme.py:30-31
    assert open("out_large.txt").read() == "hip|1.000s|27000001|27.000 mrays/s|"


def test_compute_entry_points_fail_loudly_without_gpu():
    if r1.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(r1.R1Error) as e:
        r1.Renderer(0)
    assert e.value.code == binding.R1_ENODEVICE
    assert "no CPU fallback" in str(e.value) or "hipGetDeviceCount" in str(e.value)


def test_product_does_not_touch_the_oracle():
    """The product path must not include, import, link or load anything under oracle/."""
    pkg = os.path.join(ROOT, "rays1bench_amd")
    bad = re.compile(r'#\s*include\s*[<"][^>"]*oracle|import\s+r1o|from\s+oracle|libr1_oracle|oracle/_ref|CDLL\([^)]*oracle')
    seen = 0
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".cpp", ".hip", ".h", ".hpp", ".inc")) or fn == "Makefile":
                seen += 1
                assert not bad.search(open(os.path.join(dp, fn)).read()), fn
    assert seen >= 7


def test_rayweek1_hip_fails_loudly_without_gpu(tmp_path):
    """The drop-in host program has no CPU path: without a HIP device it exits non-zero."""
    import subprocess
    if r1.device_count() > 0:
        pytest.skip("a GPU is present")
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", "32", "--height", "32", "--spp", "1"], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 2
    assert b"cannot create HIP context" in out.stderr
    assert not os.path.exists(tmp_path / "out_large.txt")


def test_headers_are_plain_c99_and_link_against_the_library(tmp_path):
    """The drop-in boundary is a C ABI: include/*.h must compile as strict C99 (no C++ or torch types)
    and a C program must link against librays1.so and reach a host-only entry point."""
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text('#include "rays1.h"\n#include "rays1_seed.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '    r1_params p = {64, 32, 1, 50, 1, 32, 32, 0, 1, R1_VARIANT_DEFAULT};\n'
                   '    int32_t total = 0, per = 0;\n'
                   '    if (r1_abi_version() != R1_ABI_VERSION || r1_tile_count(&p, &total, &per) != R1_OK) return 1;\n'
                   '    r1_sample_seed s = r1_seed_sample(10001u, 7u, 3u);\n'
                   '    printf("%d %d %u\\n", (int)total, (int)per, (unsigned)s.scalar);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "abi"
    libdir = os.path.join(ROOT, "rays1bench_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lrays1", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr.decode()
    total, per, scalar = out.stdout.decode().split()
    assert (int(total), int(per)) == (2, 2) and int(scalar) != 0


# ---- the reference's single-thread CPU stages behind the drop-in's benchmark() --------


def _run_backend(tmp_path, backend, w, h, spp):
    """rayweek1_hip --backend cpu-*: no GPU is touched, so this runs here.  Returns {scene: (rays, rgb image)}."""
    import re
    import subprocess
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--backend", backend, "-w", "--width", str(w), "--height", str(h), "--spp", str(spp)], cwd=tmp_path,
                         capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()
    text = out.stdout.decode()
    assert f"backend:        {backend} (1 host thread, no GPU)" in text
    res = {}
    for name in ("small", "medium", "large"):
        rays = int(re.search(rf"^{name}\n.*\n.*\ntotal rays:     (\d+)", text, flags=re.M).group(1))
        tga = open(os.path.join(tmp_path, f"out_{name}.tga"), "rb").read()
        assert tga[:18] == bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, w & 255, w >> 8, h & 255, h >> 8, 24, 0])
        res[name] = (rays, np.frombuffer(tga[18:], np.uint8).reshape(h, w, 3)[:, :, ::-1])
        assert re.fullmatch(rf"{backend}\|\d+\.\d{{3}}s\|{rays}\|\d+\.\d{{3}} mrays/s\|", open(os.path.join(tmp_path, f"out_{name}.txt")).read())
        # the JSON record parses (the device-only fractions were 0/0 = -nan with devices == 0) and says what ran
        import json
        rec = json.load(open(os.path.join(tmp_path, f"out_{name}.json")))
        assert rec["devices"] == 0 and rec["version"] == backend and rec["runs"][0]["num_rays"] == rays
        assert rec["hbm_algorithmic_fraction_of_8TBs"] is None and rec["fp32_vector_fraction_of_157TFs"] is None
    return res


@pytest.mark.parametrize("fixture", ["step1_small_200x100x1.bin", "step1_small_64x48x3.bin"])
def test_cpu_step1_backend_matches_the_reference_fixture(tmp_path, fixture):
    """BASELINE config 1 (small scene, 200x100, 1 spp, step1 CPU): the product's own step1 backend against the
    fixture written by the reference's step1 translation unit (36 392 rays, TGA md5 a6a0ee7a...)."""
    g = r1o.read_golden(os.path.join(ROOT, "tests", "golden", fixture))
    w, h, spp = g["hdr"].tolist()
    res = _run_backend(tmp_path, "cpu-step1", w, h, spp)
    assert res["small"][0] == int(g["rays"][0])
    assert res["small"][1].tobytes() == g["image"].tobytes()
    if fixture.startswith("step1_small_200x100x1"):
        import hashlib
        assert hashlib.md5(open(os.path.join(tmp_path, "out_small.tga"), "rb").read()).hexdigest() == "a6a0ee7a9eb9d99fc175d4809f32da96"
        # medium / large under step1 semantics are compiler-flag sensitive in the reference itself
        # (48 608 vs 48 666, 53 929 vs 53 167 rays: SURVEY.md §8c): statistics only
        assert abs(res["medium"][0] - 48637) < 0.02 * 48637 and abs(res["large"][0] - 53548) < 0.03 * 53548


@pytest.mark.parametrize("size", [(80, 60, 4), (70, 50, 3)])
def test_cpu_step12_backend_matches_the_sequential_fixtures(tmp_path, size):
    """The single-thread build of step13 (rayweek1.cpp:879-888: sequential streams 10001 / (1007, 1005, 1003, 1001)),
    i.e. what step12 computes, against the fixtures written by the reference's own render_tile."""
    w, h, spp = size
    res = _run_backend(tmp_path, "cpu-step12", w, h, spp)
    for name in ("small", "medium", "large"):
        path = os.path.join(ROOT, "tests", "golden", f"seq_{name}_{w}x{h}x{spp}.bin")
        if not os.path.exists(path):
            continue
        g = r1o.read_golden(path)
        assert res[name][0] == int(g["rays"][0]), name
        assert res[name][1].tobytes() == g["image"].tobytes(), name


def test_cpu_backends_are_named_choices_of_the_host_program_only():
    """No CPU path in the library, no fallback: librays1.so exports nothing of the CPU stages, the hip backend
    without a device is an error, and an unknown backend is rejected."""
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", binding.lib_path()], capture_output=True, text=True).stdout
    assert "r1cpu_" not in syms
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    bad = subprocess.run([exe, "--backend", "cpu"], capture_output=True, timeout=60)
    assert bad.returncode != 0
    if r1.device_count() == 0:
        hip = subprocess.run([exe, "--width", "16", "--height", "16", "--spp", "1"], capture_output=True, timeout=60)
        assert hip.returncode != 0 and b"HIP" in hip.stderr


def test_record_sizes_keep_the_ray_counts_aligned():
    """r1_shard_record_bytes / r1_frame_record_bytes (host arithmetic, no GPU): the uint64 ray count behind a tile block or an
    image is 8-byte aligned for any tile and image size, and sharding.py mirrors the C arithmetic."""
    from rays1bench_amd import sharding
    for w, h, shards, tw, th in ((1200, 800, 8, 32, 32), (93, 61, 3, 5, 7), (7, 5, 2, 3, 3), (1, 1, 1, 1, 1), (1921, 1081, 5, 31, 17)):
        p = r1.make_params(w, h, 2, 1, tile_w=tw, tile_h=th, shard=0, num_shards=shards)
        block, rec, frame = binding.shard_block_bytes(p), binding.shard_record_bytes(p), binding.frame_record_bytes(p)
        assert rec % 8 == 0 and rec - 8 >= block and rec - 16 < block
        assert frame % 8 == 0 and frame - 8 >= w * h * 3 and frame - 16 < w * h * 3
        assert rec == sharding.record_bytes(w, h, shards, tw, th) and block == sharding.block_bytes(w, h, shards, tw, th)
        rng = np.random.default_rng(w)
        blk = rng.integers(0, 255, block, dtype=np.uint8)
        one = sharding.make_record(blk, 123456789012)
        assert one.size == rec and int(one[rec - 8:].view(np.uint64)[0]) == 123456789012 and one[:block].tobytes() == blk.tobytes()
    bad = r1.make_params(0, 5, 1)
    assert binding.shard_record_bytes(bad) == 0 and binding.frame_record_bytes(bad) == 0


def test_code_object_census_no_mfma_no_generic_loads_no_scratch():
    """north_star: no MFMA on this path.  VERDICT r03 item 4: no generic (flat) loads — hipcc merges a select between an LDS and a
    global address into one generic load — and no scratch in any product kernel: every r1_* kernel of librays1.so's gfx950 code
    objects (one per translation unit) is read with llvm-readelf / llvm-objdump (tools/kernel_meta.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    k = kernel_meta.collect(lib)
    traces = [n for n in k if "r1_trace_kernel" in n]
    assert len(traces) == 19 and len(k) >= 25  # the trace kernel's instances + wavefront / resolve / assemble / helpers
    for name, m in k.items():
        assert m["v_mfma"] == 0, name
        assert m["flat_load"] == 0, name
        diagnostic = re.search(r"r1_trace_kernelILi\d+ELb1E", name) is not None  # r1_trace_kernel<VARIANT, STATS = true, ...>
        if not diagnostic:  # (the diagnostic builds keep 18 64-bit counters per lane and write a per-wave log through a pointer read from memory)
            assert m["flat_store"] == 0, name
            assert int(m["scratch"]) == 0 and m["scratch_insts"] == 0 and int(m["vgpr_spill"]) == 0, (name, m)
    # register budgets the launch geometry relies on: 7 waves per SIMD for the small-scene throughput tree kernels, 8 for the big-scene ones
    for name in traces:
        if "ILi4ELb0ELb0ELi0E" in name or "ILi4ELb0ELb0ELi3E" in name:
            assert int(k[name]["vgpr"]) <= 72, name
        if "ILi4ELb0ELb1ELi0E" in name or "ILi4ELb0ELb1ELi3E" in name:
            assert int(k[name]["vgpr"]) <= 64 and int(k[name]["sgpr"]) <= 96, name
    # the product kernels re-read their arguments per phase instead of carrying them in spilled SGPRs — v_readlane /
    # v_writelane (a VALU issue slot each) stay rare: 97 in the tree kernel (580 before; 16 of them at the wave's exit, where the in-kernel
    # tile sum builds a 64-bit-based descriptor per load), 4 in the synchronous one, 20 in the sweep
    for tag, most in (("ILi4ELb0ELb0ELi0E", 120), ("ILi4ELb0ELb0ELi3E", 120), ("ILi4ELb0ELb0ELi1E", 40), ("ILi2ELb0ELb0ELi0E", 60)):
        name = [n for n in traces if tag in n][0]
        assert k[name]["lane_moves"] <= most, (name, k[name]["lane_moves"])
