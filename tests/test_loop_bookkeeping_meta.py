"""CPU test of the register budget of the frames-in-flight tree kernels (no GPU): r1_trace_tree_small.hip is cross-compiled for gfx950 with
the Makefile's compiler and flags, as tests/test_device_headers_host.py compiles the headers, and the code object's metadata notes must show
r1_trace_kernel<4,false,false,0> (R1_MODE_TP) and <4,false,false,3> (R1_MODE_BATCH) at no more than 73 VGPRs and 96 SGPRs, with no scratch
and no spilled VGPR: what seven workgroups per CU ask of them (r1_trace.hpp TraceWaves; 512 / 7 -> 73, 800 / 8 -> 96 after rounding).
Only the metadata is read (llvm-readelf --notes); the instructions are not looked at."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rays1bench_amd", "csrc")
MAX_VGPR, MAX_SGPR = 73, 96
# r1_trace_kernel<VARIANT = 4 (R1_V_TREE), STATS = false, BIG = false, MODE>: the Itanium mangling of the template arguments
KERNELS = {"TP": "_Z15r1_trace_kernelILi4ELb0ELb0ELi0EEv11R1TraceArgs", "BATCH": "_Z15r1_trace_kernelILi4ELb0ELb0ELi3EEv11R1TraceArgs"}


def _makefile_var(name):
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, flags=re.M).group(1).strip()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """kernel name -> {metadata key: value} of the translation unit's gfx950 code object"""
    hipcc = _makefile_var("HIPCC")
    readelf = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "llvm-readelf")
    if not os.path.exists(hipcc) or not os.path.exists(readelf):
        pytest.skip("no hipcc")
    co = str(tmp_path_factory.mktemp("meta") / "tree_small.co")
    cmd = [hipcc, "--offload-arch=" + _makefile_var("ARCH")] + _makefile_var("FLAGS").split() + \
          ["--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", co, os.path.join(CSRC, "r1_trace_tree_small.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count", text)[1:]:
        fields = dict(re.findall(r"^\s*(?:- )?(\.[a-z_]+):\s*(\S+)\s*$", ".agpr_count" + block, flags=re.M))
        out[fields[".name"]] = fields
    return out


def test_the_translation_unit_holds_both_kernels(notes):
    for mode, name in KERNELS.items():
        assert name in notes, (mode, sorted(notes))


@pytest.mark.parametrize("mode", sorted(KERNELS))
def test_register_budget_of_the_frames_in_flight_tree_kernels(notes, mode):
    m = notes[KERNELS[mode]]
    vgpr, sgpr, scratch = int(m[".vgpr_count"]), int(m[".sgpr_count"]), int(m[".private_segment_fixed_size"])
    print(f"{mode}: {vgpr} VGPRs, {sgpr} SGPRs ({m['.sgpr_spill_count']} spilled to lanes), scratch {scratch} bytes, "
          f"{m['.vgpr_spill_count']} VGPRs spilled")
    assert vgpr <= MAX_VGPR, vgpr
    assert sgpr <= MAX_SGPR, sgpr
    assert scratch == 0, scratch
    assert int(m[".vgpr_spill_count"]) == 0
