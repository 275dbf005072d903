"""The trace kernel's builds (rays1bench_amd/csrc/r1_builds.h; no GPU): which build a call reaches is decided in one place, r1_pick, from the
variant, the scene's size class and the mode the caller would like.  Checked here: the choice over all 8 x 2 x 7 inputs against a table
written out below (what the three layers that used to decide it chose), the predicates host and device code share, and that the builds
r1_pick can reach are exactly the trace-body kernels in the library — a kernel no call reaches, or a choice no translation unit builds,
fails the last test."""
import ctypes as C
import os
import re
import sys

import pytest

from rays1bench_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TP, LAT, PIXEL, BATCH, PASS, PATH, LISTED = range(7)
N = None

# (variant, big) -> for each mode asked, TP .. LISTED: the build that runs (variant, stats, big, mode), or N: refused
PICKS = {
    (1, 0): [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0), N, (1, 0, 0, 4), N, N],
    (1, 1): [(1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), N, (1, 0, 1, 4), N, N],
    (2, 0): [(2, 0, 0, 0), (2, 0, 0, 1), (2, 0, 0, 2), (2, 0, 0, 3), (2, 0, 0, 4), (2, 0, 0, 5), (2, 0, 0, 6)],
    (2, 1): [(2, 0, 1, 0), (2, 0, 1, 0), (2, 0, 1, 2), (2, 0, 1, 3), (2, 0, 1, 4), (2, 0, 1, 5), (2, 0, 1, 6)],
    (3, 0): [(2, 1, 0, 1), (2, 1, 0, 1), (2, 1, 0, 1), N, N, N, N],
    (3, 1): [(2, 0, 1, 0), (2, 0, 1, 0), (2, 0, 1, 0), N, N, N, N],
    (4, 0): [(4, 0, 0, 0), (4, 0, 0, 1), (4, 0, 0, 2), (4, 0, 0, 3), (4, 0, 0, 4), (4, 0, 0, 5), (4, 0, 0, 6)],
    (4, 1): [(4, 0, 1, 0), (4, 0, 1, 0), (4, 0, 1, 2), (4, 0, 1, 3), (4, 0, 1, 4), (4, 0, 1, 5), (4, 0, 1, 6)],
    (5, 0): [(4, 1, 0, 1), (4, 1, 0, 1), (4, 1, 0, 1), N, N, N, N],
    (5, 1): [(4, 1, 1, 0), (4, 1, 1, 0), (4, 1, 1, 0), N, N, N, N],
    (6, 0): [N, N, N, N, N, N, N],
    (6, 1): [N, N, N, N, N, N, N],
    (7, 0): [(7, 0, 0, 0), (7, 0, 0, 1), N, (7, 0, 0, 3), (7, 0, 0, 4), (7, 0, 0, 5), (7, 0, 0, 6)],
    (7, 1): [(7, 0, 1, 0), (7, 0, 1, 0), (7, 0, 1, 2), (7, 0, 1, 3), (7, 0, 1, 4), (7, 0, 1, 5), (7, 0, 1, 6)],
    (8, 0): [(7, 1, 0, 1), (7, 1, 0, 1), (7, 1, 0, 1), N, N, N, N],
    (8, 1): [(7, 1, 1, 0), (7, 1, 1, 0), (7, 1, 1, 0), N, N, N, N],
}


def pick(variant, big, want):
    f = binding.lib().r1_pick_build
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 4)(-1, -1, -1, -1)
    return tuple(out) if f(variant, big, want, out) else None


def test_the_table_has_the_counts_the_parent_had():
    flat = [b for row in PICKS.values() for b in row]
    assert len(PICKS) == 16 and all(len(row) == 7 for row in PICKS.values())
    assert sum(b is not None for b in flat) == 67 and sum(b is None for b in flat) == 45
    assert len({b for b in flat if b is not None}) == 47


def test_pick_equals_the_table_for_every_input():
    got = {(v, big): [pick(v, big, want) for want in range(7)] for v in range(1, 9) for big in (0, 1)}
    wrong = [(key, want, got[key][want], PICKS[key][want]) for key in PICKS for want in range(7) if got[key][want] != PICKS[key][want]]
    assert not wrong, wrong
    # what is no variant or no mode is refused, not read as its neighbour
    for v, big, want in ((0, 0, TP), (9, 1, TP), (-1, 0, LAT), (4, 0, 7), (4, 1, -1)):
        assert pick(v, big, want) is None, (v, big, want)


def test_predicates_match_their_tables():
    f = binding.lib().r1_build_facts
    f.restype, f.argtypes = None, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]

    def facts(variant=0, mode=0, big=0):
        out = (C.c_int * 6)()
        f(variant, mode, big, out)
        return list(out)

    #            variant: 0  1  2  3  4  5  6  7  8  9
    tree, grid, stats = [0, 0, 0, 0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 0, 1, 0, 0, 1, 0]
    base = [0, 1, 2, 2, 4, 4, 6, 7, 7, 9]
    for v in range(10):
        assert facts(variant=v)[:4] == [tree[v], grid[v], stats[v], base[v]], v
    #       mode: TP LAT PIXEL BATCH PASS PATH LISTED
    tp_family = [1, 0, 0, 1, 0, 1, 0]
    lat_small = [0, 1, 0, 0, 1, 0, 1]
    lat_big = [0, 1, 0, 0, 0, 0, 0]
    for m in range(7):
        assert facts(mode=m)[4] == tp_family[m], m
        assert facts(mode=m, big=0)[5] == lat_small[m] and facts(mode=m, big=1)[5] == lat_big[m], m


def build_of(name):
    """The build (variant, stats, big, mode) of a trace-body kernel, from its mangled template arguments; None: another kernel."""
    m = re.search(r"r1_trace_kernelILi(\d)ELb([01])ELb([01])ELi(\d)EE", name)
    if m:
        return tuple(int(x) for x in m.groups())
    m = re.search(r"r1_grid_kernelILb([01])ELb([01])ELi(\d)EE", name)
    if m:
        return (7, int(m.group(1)), int(m.group(2)), int(m.group(3)))
    for tag, mode in (("r1_pass_kernel", PASS), ("r1_path_kernel", PATH), ("r1_adaptive_kernel", LISTED)):
        m = re.search(tag + r"ILi(\d)ELb([01])EE", name)
        if m:
            return (int(m.group(1)), 0, int(m.group(2)), mode)
    assert not re.search(r"r1_(trace|grid|pass|path|adaptive)_kernel", name), f"a trace-body kernel this test cannot read: {name}"
    return None


def test_library_holds_exactly_the_builds_pick_can_reach():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "rays1bench_amd", "lib", "librays1.so")
    if not (os.path.exists(lib) and os.path.exists(kernel_meta.LLVM + "/llvm-objdump")):
        pytest.skip("no library / no LLVM tools")
    names = [n for n in kernel_meta.collect(lib) if build_of(n) is not None]
    built = {build_of(n) for n in names}
    assert len(names) == len(built), "two kernels of one build"
    reached = {pick(v, big, want) for v in range(1, 9) for big in (0, 1) for want in range(7)} - {None}
    assert built - reached == set(), f"built, and no call reaches them: {sorted(built - reached)}"
    assert reached - built == set(), f"picked, and not in the library: {sorted(reached - built)}"
    assert len(built) == 47
