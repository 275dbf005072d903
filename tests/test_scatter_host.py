"""CPU test of the scatter arithmetic the trace kernels share (rays1bench_amd/csrc/r1_scatter.h): a stand-alone program
(tools/check_scatter_host.cpp) runs the header on the host and compares the Dielectric arm without the outward normal (form 1) with the
reference's form (0), and both with the ORACLE's own reflect, refract and scatter (oracle/r1_oracle.c behind
tools/check_scatter_oracle.c), bit for bit: directions, Material::scatter's result and the stream states after the draws.  Inputs: 10^7
seeded random unit d and n with refraction indices on both sides of 1, and the edges — ddn = +0 and -0, components of d and n that are +-0,
grazing incidence, cosines a few 1e-8 to either side of total reflection, fuzz 0 and 1.  Zero mismatches are required, and the counters
show that every edge was reached.  Frames of the device: tests/test_gpu_scatter.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_INPUTS = 10_000_000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("scatter")
    oracle_o, host_o, exe = str(d / "oracle.o"), str(d / "host.o"), str(d / "check_scatter_host")
    # the oracle's translation unit with the oracle's flags (oracle/Makefile), the header with the arithmetic contract of the product's
    subprocess.check_call(["gcc", "-O3", "-std=gnu11", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-w",
                           f'-DR1_ORACLE_TU="{os.path.join(ROOT, "oracle", "r1_oracle.c")}"', "-c",
                           os.path.join(ROOT, "tools", "check_scatter_oracle.c"), "-o", oracle_o])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-c",
                           os.path.join(ROOT, "tools", "check_scatter_host.cpp"), "-o", host_o])
    subprocess.check_call(["g++", host_o, oracle_o, "-o", exe, "-lm", "-pthread"])
    return exe


@pytest.fixture(scope="module")
def counters(program):
    out = subprocess.run([program, str(RANDOM_INPUTS), "2026"], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    c["returncode"] = out.returncode
    return c


def test_both_forms_and_the_oracle_agree_bit_for_bit(counters):
    assert counters["random_inputs"] >= 10 ** 7
    assert counters["mismatches"] == 0 and counters["returncode"] == 0, counters


def test_the_inputs_reach_every_edge(counters):
    c = counters
    assert c["ddn_pos_zero"] > 1000 and c["ddn_neg_zero"] > 1000      # both zeros of dot(d, n)
    assert c["zero_components"] > 10000 and c["grazing"] > 100000
    assert c["inside"] > 10 ** 6 and c["outside"] > 10 ** 6             # both sides of the surface
    assert c["index_below_one"] > 10 ** 6 and c["index_above_one"] > 10 ** 6
    assert c["total_reflection"] > 10 ** 5 and c["refracting"] > 10 ** 6
    assert c["just_above"] > 10 ** 4                                    # 0 < discriminant < 1e-5
    assert c["fuzz_zero"] > 10000 and c["fuzz_one"] > 10000
    assert c["chose_reflected"] > 10 ** 6 and c["chose_refracted"] > 10 ** 6 and c["metal_absorbed"] > 10 ** 5


def test_the_program_reports_a_wrong_form(tmp_path):
    """The comparison can fail: the same program over a header whose form 1 keeps `root`'s sign inside the sphere."""
    src = open(os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_scatter.h")).read()
    good = "const float r = k.inside ? -root : root;"
    assert src.count(good) == 1
    os.makedirs(tmp_path / "rays1bench_amd" / "csrc")
    os.makedirs(tmp_path / "tools")
    (tmp_path / "rays1bench_amd" / "csrc" / "r1_scatter.h").write_text(src.replace(good, "const float r = root;"))
    for name in ("check_scatter_host.cpp", "check_scatter_oracle.c"):
        (tmp_path / "tools" / name).write_text(open(os.path.join(ROOT, "tools", name)).read())
    exe = str(tmp_path / "wrong")
    subprocess.check_call(["gcc", "-O3", "-std=gnu11", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-w",
                           f'-DR1_ORACLE_TU="{os.path.join(ROOT, "oracle", "r1_oracle.c")}"', "-c", str(tmp_path / "tools" / "check_scatter_oracle.c"),
                           "-o", str(tmp_path / "oracle.o")])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", str(tmp_path / "tools" / "check_scatter_host.cpp"),
                           str(tmp_path / "oracle.o"), "-o", exe, "-lm", "-pthread"])
    out = subprocess.run([exe, "1000", "1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "MISMATCH" in out.stderr
    assert int(dict(line.split() for line in out.stdout.splitlines())["mismatches"]) > 1000
