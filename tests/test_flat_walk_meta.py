"""CPU test of the flat twins of the frames-in-flight tree kernels (no GPU): r1_trace_tree_small.hip is cross-compiled for
gfx950 with the Makefile's compiler and flags, as tests/test_loop_bookkeeping_meta.py compiles it, and the code object's metadata notes must
show r1_flatwalk_kernel<0> (R1_MODE_TP) and <3> (R1_MODE_BATCH) at no more than 72 VGPRs and 96 SGPRs, with no scratch and no spilled VGPR —
the registers of the generic kernels they replace at launch, whose occupancy the launch geometry was sized for — next to the two
r1_trace_kernel instances of that test, which stay.  Only the metadata is read (llvm-readelf --notes); the instructions are not looked at."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rays1bench_amd", "csrc")
MAX_VGPR, MAX_SGPR = 72, 96
# r1_flatwalk_kernel<MODE>: the Itanium mangling of the template argument
TWINS = {"TP": "_Z18r1_flatwalk_kernelILi0EEv11R1TraceArgs", "BATCH": "_Z18r1_flatwalk_kernelILi3EEv11R1TraceArgs"}
GENERIC = {"TP": "_Z15r1_trace_kernelILi4ELb0ELb0ELi0EEv11R1TraceArgs", "BATCH": "_Z15r1_trace_kernelILi4ELb0ELb0ELi3EEv11R1TraceArgs"}


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


def test_the_translation_unit_holds_both_twins_and_both_generic_kernels(notes):
    for mode in sorted(TWINS):
        assert TWINS[mode] in notes, (mode, sorted(notes))
        assert GENERIC[mode] in notes, (mode, sorted(notes))
    # no twin carries a name the build table's census reads (tests/test_builds_host.py build_of)
    for name in TWINS.values():
        assert not re.search(r"r1_(trace|grid|pass|path|adaptive)_kernel", name)


@pytest.mark.parametrize("mode", sorted(TWINS))
def test_register_budget_of_the_flat_twins(notes, mode):
    m = notes[TWINS[mode]]
    vgpr, sgpr, scratch = int(m[".vgpr_count"]), int(m[".sgpr_count"]), int(m[".private_segment_fixed_size"])
    print(f"{mode}: {vgpr} VGPRs, {sgpr} SGPRs ({m['.sgpr_spill_count']} spilled to lanes), scratch {scratch} bytes, "
          f"{m['.vgpr_spill_count']} VGPRs spilled")
    assert vgpr <= MAX_VGPR, vgpr
    assert sgpr <= MAX_SGPR, sgpr
    assert scratch == 0, scratch
    assert int(m[".vgpr_spill_count"]) == 0
    # the twin takes its sibling's place in a grid sized for the sibling: no more registers per wave than it
    g = notes[GENERIC[mode]]
    assert vgpr <= int(g[".vgpr_count"]) and sgpr <= int(g[".sgpr_count"]), (m, g)
