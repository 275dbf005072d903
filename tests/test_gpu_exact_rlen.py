"""The reciprocal length of the trace kernels' ray normalisation (rays1bench_amd/csrc/r1_exact_math.h: r1_rlen_guarded,
r1_rlen_total) against the compiler's `1.0f / __builtin_sqrtf(x)` for ALL 2^32 fp32 bit patterns, on this GPU.

The short sequence starts from v_rsq_f32 and v_rcp_f32, whose bits only the chip defines: it is admissible only because this
comparison finds no difference.  rays1bench_amd/lib/check_exact_rlen (tools/check_exact_rlen.hip, built by the Makefile's
default target with the kernels' flags and header) makes four sweeps of 2^26 waves:

  pass 1   the guarded form, 64 consecutive patterns per wave, all lanes active: equal bits everywhere, and the short sequence
           taken by exactly the waves whose patterns all lie in D = [2^-96, FLT_MAX] — 0x70000000 / 64 of 2^26;
  pass 2a  lanes 0x04000001 apart (both signs, tiny, normal, inf, NaN in every wave), all active: the compiler's arm, equal;
  pass 2b  the same waves, the lanes outside D inactive: the short sequence in every wave, the active lanes equal;
  pass 3   the branch-free total form, all 2^32 patterns: equal for every one — tiny, subnormal, +-0, +-inf, negative, NaN.

A missing binary is a failure: a skip would let a wrong sequence through."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "rays1bench_amd", "lib", "check_exact_rlen")
TIME_LIMIT_S = 300  # (four sweeps take a few milliseconds each on an MI355X; the limit covers a cold start of the runtime)
WAVES = 1 << 26
SHIPPED, FALLBACK = 4, 3


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
    for name, fast in (("pass1", 0x70000000 // 64), ("pass2a", 0), ("pass2b", WAVES), ("pass3", 0)):
        assert int(f[f"{name}_waves"]) == WAVES
        assert int(f[f"{name}_mismatches"]) == 0, f.get("records")
        assert int(f[f"{name}_fast_waves"]) == fast == int(f[f"{name}_fast_waves_expected"])
        assert int(f[f"{name}_arm_errors"]) == 0
        assert float(f[f"{name}_ms"]) > 0.0
    assert int(f["mismatches"]) == 0 and f["verdict"] == "PASS" and "records" not in f
    assert rc == 0


def test_the_shipped_reciprocal_length_equals_the_compilers_for_every_input(tmp_path):
    out = tmp_path / "check_exact_rlen.txt"
    rc, f = run_checker("--out", str(out))
    assert f["form"] == f["shipped_form"] == str(SHIPPED)
    check_figures(rc, f, SHIPPED)
    assert "verdict PASS" in out.read_text()
    # the classes the total form routes to v_rsq_f32's own value: +-0 -> +-inf, +inf -> 0, NaN and negative -> NaN
    for x, want in (("0x00000000", "0x7f800000"), ("0x80000000", "0xff800000"), ("0x7f800000", "0x00000000")):
        assert f[f"probe_{x}"] == f"rsq {want} total {want} want {want}"


def test_the_shipped_form_is_the_one_the_design_names():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.23"):]
    m = re.search(r"`R1_RLEN_FORM` \*\*(\d)\*\* ships", section)
    assert m, "DESIGN.md §4.23 no longer says which form ships"
    header = open(os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_exact_math.h")).read()
    assert re.search(rf"#define R1_RLEN_FORM {m.group(1)}\b", header) and int(m.group(1)) == SHIPPED


def test_the_fallback_form_equals_it_as_well():
    """form 3 (form B's root, v_rcp_f32 and the compiler's division chain without its no-ops), kept in the header as the form
    to fall back to"""
    rc, f = run_checker("--form", str(FALLBACK))
    check_figures(rc, f, FALLBACK)
