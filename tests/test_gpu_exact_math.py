"""The square root of the trace kernels (rays1bench_amd/csrc/r1_exact_math.h) against the compiler's
correctly rounded __builtin_sqrtf for ALL 2^32 fp32 bit patterns, on this GPU.

r1_sqrt_exact's short sequence starts from v_rsq_f32, whose bits only the chip defines: it is admissible only because this
comparison finds no difference.  rays1bench_amd/lib/check_exact_math (tools/check_exact_math.hip, built by the Makefile's
default target with the kernels' flags and header) makes three sweeps of 2^26 waves:

  pass 1   64 consecutive patterns per wave, all lanes active: equal bits everywhere, and the short sequence taken by exactly
           the waves whose patterns all lie in D = [2^-96, FLT_MAX] — 0x70000000 / 64 of 2^26 = 43.75 %;
  pass 2a  lanes 0x04000001 apart (both signs, tiny, normal, inf, NaN in every wave), all active: the compiler's arm, equal;
  pass 2b  the same waves, the lanes outside D inactive: the short sequence in every wave, the active lanes equal.

A missing binary is a failure: a skip would let a wrong sequence through."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "rays1bench_amd", "lib", "check_exact_math")
TIME_LIMIT_S = 300  # (three sweeps take a few milliseconds each on an MI355X; the limit covers a cold start of the runtime)
WAVES = 1 << 26


def run_checker(*args):
    assert os.access(CHECKER, os.X_OK), f"{CHECKER} is missing: build() makes it (rays1bench_amd/csrc/Makefile, default target)"
    p = subprocess.run([CHECKER, *args], capture_output=True, text=True, timeout=TIME_LIMIT_S)
    print(p.stdout)
    print(p.stderr)
    figures = {}
    for line in p.stdout.splitlines():
        key, _, value = line.partition(" ")
        if key.endswith("_mismatch"):
            figures.setdefault("records", []).append(value)
        else:
            figures[key] = value
    return p.returncode, figures


def check_figures(rc, f, form):
    assert f["form"] == str(form) and f["arch"].startswith("gfx950")
    for name, fast in (("pass1", 0x70000000 // 64), ("pass2a", 0), ("pass2b", WAVES)):
        assert int(f[f"{name}_waves"]) == WAVES
        assert int(f[f"{name}_mismatches"]) == 0, f.get("records")
        assert int(f[f"{name}_fast_waves"]) == fast == int(f[f"{name}_fast_waves_expected"])
        assert int(f[f"{name}_arm_errors"]) == 0
        assert abs(float(f[f"{name}_fast_share"]) - fast / WAVES) < 1e-6
        assert float(f[f"{name}_ms"]) > 0.0
    assert int(f["mismatches"]) == 0 and f["verdict"] == "PASS" and "records" not in f
    assert rc == 0


def test_the_shipped_square_root_equals_the_compilers_for_every_input(tmp_path):
    out = tmp_path / "check_exact_math.txt"
    rc, f = run_checker("--out", str(out))
    assert f["form"] == f["shipped_form"] == "2", "the kernels ship another form than DESIGN.md §4.18 says"
    check_figures(rc, f, 2)
    assert "verdict PASS" in out.read_text()


def test_the_fallback_form_equals_it_as_well():
    """form A (v_sqrt_f32 and the +-1 ulp correction: the compiler's sequence without its scaling and class fix-up), kept in the
    header as the form to fall back to"""
    rc, f = run_checker("--form", "1")
    check_figures(rc, f, 1)
