"""CPU tests of adaptive sampling (r1_render_adaptive / r1_adaptive_schedule, include/rays1.h): the entry points are
declared, exported and bound, a strict-C99 caller compiles and links, the schedule and every refusal of the options are right without a
device, the rule restated in numpy (tests/adaptive_rule.py) gives the known map on the ORACLE's records of the fixture frame, and the
code object holds the new kernels at their siblings' registers.  Pixels, counts and maps of the device are checked in
tests/test_gpu_adaptive.py."""
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

import adaptive_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")


def test_adaptive_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+r1_render_adaptive\s*\(\s*r1_context\s*\*\s*\w+\s*,\s*const\s+r1_params\s*\*\s*\w+\s*,\s*const\s+r1_adaptive\s*\*\s*\w+\s*,"
                     r"\s*uint8_t\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*,\s*r1_tile_report\s*\*\s*\w+\s*,\s*r1_adaptive_result\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+r1_adaptive_schedule\s*\(\s*const\s+r1_params\s*\*\s*\w+\s*,\s*const\s+r1_adaptive\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,"
                     r"\s*size_t\s+\w+\s*,\s*size_t\s*\*\s*\w+\s*\)\s*;", hdr)
    assert re.search(r"#define R1_ABI_VERSION 4\b", hdr)
    names = {s[0] for s in binding.SYMBOLS}
    for name in ("r1_render_adaptive", "r1_adaptive_schedule"):
        assert hasattr(r1.lib(), name) and name in names, name
    assert callable(getattr(binding.Renderer, "render_adaptive", None)) and callable(getattr(binding, "adaptive_schedule", None))
    assert C.sizeof(binding.Adaptive) == 16 and C.sizeof(binding.TileReport) == 16 and C.sizeof(binding.AdaptiveResult) == 24
    assert binding.TILE_REPORT_DTYPE.itemsize == 16


def test_render_adaptive_refuses_null_context():
    L = r1.lib()
    p = r1.make_params(64, 32, 8)
    opt = binding.Adaptive(4, 4, 16, 65280)
    img = (C.c_uint8 * (64 * 32 * 3))()
    rays = C.c_uint64()
    assert L.r1_render_adaptive(None, C.byref(p), C.byref(opt), img, C.byref(rays), None, None) == binding.R1_EINVAL
    assert "null" in L.r1_last_error().decode()
    assert L.r1_render_adaptive(None, None, None, None, None, None, None) == binding.R1_EINVAL


def test_a_c99_program_calls_the_adaptive_entry_points(tmp_path):
    src = tmp_path / "adaptive.c"
    src.write_text('#include "rays1.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '    r1_params p = {64, 32, 14, 50, 1, 32, 32, 0, 1, R1_VARIANT_DEFAULT};\n'
                   '    r1_adaptive opt = {3, 5, 24, 65280};\n'
                   '    r1_tile_report tiles[2];\n'
                   '    r1_adaptive_result res;\n'
                   '    int32_t n[8];\n'
                   '    size_t count = 0;\n'
                   '    uint8_t rgb[64 * 32 * 3];\n'
                   '    uint64_t rays = 0;\n'
                   '    int rc = r1_adaptive_schedule(&p, &opt, n, 8, &count);\n'
                   '    if (rc != R1_OK || count != 4 || n[0] != 3 || n[1] != 8 || n[2] != 13 || n[3] != 14) return 2;\n'
                   '    if (sizeof(r1_tile_report) != 16 || sizeof(r1_adaptive_result) != 24 || sizeof(r1_adaptive) != 16) return 3;\n'
                   '    rc = r1_render_adaptive(NULL, &p, &opt, rgb, &rays, tiles, &res);\n'
                   '    printf("%d\\n", rc);\n'
                   '    return rc == R1_EINVAL ? 0 : 1;\n}\n')
    exe = tmp_path / "adaptive"
    libdir = os.path.join(ROOT, "rays1bench_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lrays1", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_schedules():
    assert r1.adaptive_schedule(r1.make_params(64, 32, 64), 8, 8) == [8, 16, 24, 32, 40, 48, 56, 64]
    assert r1.adaptive_schedule(r1.make_params(64, 32, 14), 3, 5) == [3, 8, 13, 14]
    assert r1.adaptive_schedule(r1.make_params(64, 32, 14), 14, 5) == [14]
    assert r1.adaptive_schedule(r1.make_params(64, 32, 14), 200, 1) == [14]
    assert r1.adaptive_schedule(r1.make_params(64, 32, 250), 25, 25, 32, 512) == list(range(25, 251, 25))
    for cap, a, b in ((64, 8, 8), (14, 3, 5), (14, 20, 3), (250, 1, 7)):
        assert r1.adaptive_schedule(r1.make_params(64, 32, cap), a, b) == rule.schedule(cap, a, b)


def _refused(params, opt, field, code=binding.R1_EINVAL):
    L = r1.lib()
    n = C.c_size_t(12345)
    out = (C.c_int32 * 64)()
    rc = L.r1_adaptive_schedule(C.byref(params), C.byref(binding.Adaptive(*opt)), out, 64, C.byref(n))
    assert rc == code, (field, rc)
    assert field in L.r1_last_error().decode(), (field, L.r1_last_error())


def test_schedule_refuses_every_bad_field_by_name():
    p = r1.make_params(64, 32, 64)
    _refused(p, (0, 8, 24, 65280), "min_spp")
    _refused(p, (8, 0, 24, 65280), "pass_spp")
    _refused(p, (8, 8, -2, 65280), "max_delta")
    _refused(p, (8, 8, 256, 65280), "max_delta")
    _refused(p, (8, 8, 24, -1), "mean_delta_q8")
    _refused(p, (8, 8, 24, 65281), "mean_delta_q8")
    _refused(r1.make_params(64, 32, 64, shard=0, num_shards=2), (8, 8, 24, 65280), "num_shards")
    for v in (1, 3, 5, 6, 8):
        _refused(r1.make_params(64, 32, 64, variant=v), (8, 8, 24, 65280), "variant")
    for v in (0, 2, 4, 7):
        assert len(r1.adaptive_schedule(r1.make_params(64, 32, 64, variant=v), 8, 8)) == 8
    # the limits of the rule are accepted
    assert r1.adaptive_schedule(p, 8, 8, -1, 0)[-1] == 64 and r1.adaptive_schedule(p, 8, 8, 255, 65280)[-1] == 64
    # a pass beyond the per-launch limit of r1_render_pass (33 x 33 pixels are four padded tiles of 32 x 32: 4096 slots per sample)
    _refused(r1.make_params(33, 33, 1000000), (600000, 8, 24, 65280), "sample slots per launch", code=binding.R1_ELIMIT)
    assert r1.adaptive_schedule(r1.make_params(33, 33, 1000000), 500000, 500000) == [500000, 1000000]


def test_schedule_cap_too_small_sets_the_count():
    L = r1.lib()
    p, opt = r1.make_params(64, 32, 64), binding.Adaptive(8, 8, 24, 65280)
    n = C.c_size_t(0)
    out = (C.c_int32 * 8)(*([-7] * 8))
    assert L.r1_adaptive_schedule(C.byref(p), C.byref(opt), out, 7, C.byref(n)) == binding.R1_EINVAL
    assert n.value == 8 and "cap" in L.r1_last_error().decode()
    assert list(out) == [-7] * 8
    assert L.r1_adaptive_schedule(C.byref(p), C.byref(opt), None, 0, C.byref(n)) == binding.R1_OK and n.value == 8
    assert L.r1_adaptive_schedule(C.byref(p), C.byref(opt), out, 8, None) == binding.R1_OK and list(out) == list(range(8, 65, 8))
    assert L.r1_adaptive_schedule(None, C.byref(opt), out, 8, C.byref(n)) == binding.R1_EINVAL
    assert L.r1_adaptive_schedule(C.byref(p), None, out, 8, C.byref(n)) == binding.R1_EINVAL


@pytest.fixture(scope="module")
def oracle_records():
    """The oracle's per-sample records of the fixture frame: large 320 x 200, seed 10001, 64 spp."""
    w, h, cap, seed = 320, 200, 64, 10001
    sa = r1o.SceneArrays.from_golden(r1o.read_golden(os.path.join(GOLD, "scene_large_320x200.bin")))
    _, rays, samples = r1o.render_frame(sa, r1o.make_params(w, h, cap, seed), want_samples=True)
    rec = samples.reshape(h, w, cap, 4)
    assert int(rec[..., 3].view(np.uint32).sum()) == rays
    return rec


@pytest.mark.parametrize("max_delta,mean_q8,want,never", [
    (24, 65280, {8: 15, 16: 5, 24: 6, 32: 3, 40: 1, 48: 4, 56: 2, 64: 34}, 31),
    (48, 768, {8: 27, 16: 4, 24: 2, 32: 2, 40: 2, 48: 3, 56: 1, 64: 29}, 28)], ids=["24-65280", "48-768"])
def test_the_rule_on_the_oracles_records_gives_the_known_map(oracle_records, max_delta, mean_q8, want, never):
    rep, rays = rule.restate(oracle_records, 8, 8, max_delta, mean_q8)
    assert len(rep) == 70
    assert rule.histogram(rep) == want
    assert int((rep["settled"] == 0).sum()) == never and (rep["spp"][rep["settled"] == 0] == 64).all()
    # what makes the GPU tests on this frame meaningful: several distinct counts, tiles that stop at once, tiles that never settle
    assert len(want) >= 4 and want[8] >= 1 and never >= 1
    full = int(oracle_records[..., 3].view(np.uint32).sum())
    assert 0 < rays < full


def test_the_rule_at_its_limits(oracle_records):
    rec = oracle_records[:64, :96, :16]
    rep, rays = rule.restate(rec, 4, 4, -1, 65280)
    assert (rep["spp"] == 16).all() and (rep["settled"] == 0).all()
    assert rays == int(rec[..., 3].view(np.uint32).sum())
    rep, rays = rule.restate(rec, 4, 4, 255, 65280)
    assert (rep["spp"] == 4).all() and (rep["settled"] == 1).all()
    assert rays == int(rec[:, :, :4, 3].view(np.uint32).sum())


def test_census_of_the_adaptive_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    k = kernel_meta.collect(lib)
    listed = sorted(n for n in k if "r1_adaptive_kernel" in n)
    assert len(listed) == 6, listed
    # r1_adaptive_kernel<VARIANT, BIG> and its MODE 4 sibling r1_pass_kernel<VARIANT, BIG>: the list fetch costs no register (above
    # the sibling by 0 VGPRs and 0 SGPRs)
    extra_vgpr, extra_sgpr = 0, 0
    seen = set()
    for name in listed:
        m = re.search(r"r1_adaptive_kernelILi(\d)ELb([01])E", name)
        assert m, name
        seen.add((int(m.group(1)), m.group(2)))
        sib = [n for n in k if f"r1_pass_kernelILi{m.group(1)}ELb{m.group(2)}E" in n]
        assert len(sib) == 1, (name, sib)
        a, b = k[name], k[sib[0]]
        keys = ("vgpr", "sgpr", "sgpr_spill", "lane_moves", "insts", "lds")
        print(name, {x: a[x] for x in keys}, "sibling", {x: b[x] for x in keys})
        assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, (name, a)
        assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0, (name, a)
        assert int(a["vgpr"]) <= int(b["vgpr"]) + extra_vgpr and int(a["sgpr"]) <= int(b["sgpr"]) + extra_sgpr, (name, a["vgpr"], a["sgpr"], b["vgpr"], b["sgpr"])
        assert int(a["sgpr_spill"]) <= int(b["sgpr_spill"]), (name, a["sgpr_spill"], b["sgpr_spill"])
        assert a["lds"] == b["lds"], (name, a["lds"], b["lds"])
    assert seen == {(v, b) for v in (2, 4, 7) for b in ("0", "1")}
    for tag in ("r1_adapt_accum_kernel", "r1_adapt_compact_kernel"):
        own = [n for n in k if tag in n]
        assert len(own) == 1, (tag, own)
        a = k[own[0]]
        assert a["v_mfma"] == 0 and a["flat_load"] == 0 and a["flat_store"] == 0, (tag, a)
        assert int(a["scratch"]) == 0 and a["scratch_insts"] == 0 and int(a["vgpr_spill"]) == 0 and int(a["sgpr_spill"]) == 0, (tag, a)


@pytest.mark.parametrize("args", [["--adaptive", "256"], ["--adaptive", "-2"], ["--adaptive", "24,65281"], ["--adaptive", "24,"], ["--adaptive", "x"],
                                  ["--adaptive", "24", "--min-spp", "0"], ["--adaptive", "24", "--pass-spp", "0"], ["--min-spp", "4"],
                                  ["--adaptive", "24", "--devices", "2"], ["--adaptive", "24", "--backend", "cpu-step12"],
                                  ["--adaptive", "24", "--passes", "2"], ["--adaptive", "24", "--pipeline", "4"], ["--adaptive", "24", "--variant", "1"],
                                  ["--adaptive", "24", "--variant", "6"], ["--adaptive", "24", "--gather", "rccl"]],
                         ids=lambda a: "_".join(a).replace("--", "").replace(",", "c"))
def test_program_rejects_bad_adaptive_options_before_touching_a_device(tmp_path, args):
    out = subprocess.run([EXE, "--width", "32", "--height", "16", "--spp", "8", *args], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 1, (out.returncode, out.stderr)
    assert b"--adaptive" in out.stderr
    assert b"cannot create HIP context" not in out.stderr
    assert not any(tmp_path.iterdir())  # (nothing rendered, nothing written)
