"""CPU test of the device headers under rays1bench_amd/csrc (no GPU): each of them compiles when it is the only thing a translation unit
includes — it has its own guard, includes what it uses and opens and closes its own namespace — with the Makefile's compiler and flags,
for gfx950 and the host, without a warning.  What keeps "self-contained" true after the next edit of r1_trace.hpp's parts."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rays1bench_amd", "csrc")
# every header that holds device code: r1_trace.hpp and the headers it is made of, and the four shared with host code
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp"))) + ["r1_scatter.h", "r1_exact_math.h", "r1_grid_dda.h", "r1_tile.h"]


def _makefile_var(name):
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, flags=re.M).group(1).strip()


def test_the_list_names_the_trace_kernel_and_its_parts():
    assert "r1_trace.hpp" in HEADERS and len(HEADERS) >= 12
    for name in HEADERS:
        assert os.path.exists(os.path.join(CSRC, name)), name


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    hipcc = _makefile_var("HIPCC")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    tu = tmp_path / "alone.hip"
    tu.write_text('#include "%s"\n' % header)
    cmd = [hipcc, "--offload-arch=" + _makefile_var("ARCH")] + _makefile_var("FLAGS").split() + ["-fsyntax-only", "-I", CSRC, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # (the driver notes that it links nothing: `argument unused during compilation: '--hip-link'`)
    lines = [l for l in (r.stdout + r.stderr).splitlines() if l.strip() and "--hip-link" not in l]
    assert lines == [], "\n".join(lines)
