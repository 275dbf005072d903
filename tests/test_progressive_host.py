"""CPU tests of progressive rendering (r1_render_pass, include/rays1.h): the entry point is declared, exported and bound, it refuses
what it must refuse without a device, a strict-C99 caller compiles and links, and the drop-in program's --passes option rejects bad
combinations before it touches a device.  The pixels and ray counts are checked on the GPU (tests/test_gpu_progressive.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")


def test_render_pass_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+r1_render_pass\s*\(\s*r1_context\s*\*\s*\w+\s*,\s*const\s+r1_params\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*uint8_t\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)\s*;", hdr)
    assert hasattr(r1.lib(), "r1_render_pass")
    assert "r1_render_pass" in {s[0] for s in binding.SYMBOLS}
    assert callable(getattr(binding.Renderer, "render_pass", None))


def test_render_pass_refuses_null_context_or_params():
    L = r1.lib()
    p = r1.make_params(64, 32, 2)
    img = (C.c_uint8 * (64 * 32 * 3))()
    rays = C.c_uint64()
    assert L.r1_render_pass(None, C.byref(p), 0, img, C.byref(rays)) == binding.R1_EINVAL
    assert L.r1_render_pass(None, None, 0, None, None) == binding.R1_EINVAL
    assert "null" in L.r1_last_error().decode()


def test_a_c99_program_calls_render_pass(tmp_path):
    src = tmp_path / "pass.c"
    src.write_text('#include "rays1.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '    r1_params p = {64, 32, 4, 50, 1, 32, 32, 0, 1, R1_VARIANT_DEFAULT};\n'
                   '    uint8_t rgb[64 * 32 * 3];\n'
                   '    uint64_t rays = 0;\n'
                   '    int rc = r1_render_pass(NULL, &p, 0, rgb, &rays);\n'
                   '    printf("%d\\n", rc);\n'
                   '    return rc == R1_EINVAL ? 0 : 1;\n}\n')
    exe = tmp_path / "pass"
    libdir = os.path.join(ROOT, "rays1bench_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lrays1", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert out.returncode == 0, (out.stdout, out.stderr)


@pytest.mark.parametrize("args", [["--passes", "0"], ["--passes", "5", "--spp", "3"], ["--passes", "2", "--devices", "2"],
                                  ["--passes", "2", "--backend", "cpu-step12"], ["--passes", "2", "--pipeline", "4"], ["--passes", "-1"],
                                  ["--passes", "2", "--gather", "rccl"]],
                         ids=["zero", "more-than-spp", "devices", "cpu-backend", "pipeline", "negative", "gather-rccl"])
def test_program_rejects_bad_passes_before_touching_a_device(tmp_path, args):
    out = subprocess.run([EXE, "--width", "32", "--height", "16", *args], cwd=tmp_path, capture_output=True, timeout=120)
    assert out.returncode == 1, (out.returncode, out.stderr)
    assert b"--passes" in out.stderr
    assert b"cannot create HIP context" not in out.stderr
    assert not any(tmp_path.iterdir())  # (nothing rendered, nothing written)
