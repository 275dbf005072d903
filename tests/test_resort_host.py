"""CPU tests of the re-sort (csrc/r1_bvh_sort.h through r1_bvh_resort_describe; no GPU): the steps r1_resort_spheres runs on the device, restated
on the host over the same tables.

A re-sort keeps the tree's topology and re-deals the movable spheres into the leaf slots: top down, every inner node hands the k spheres
smallest along the widest axis of its spheres' centres to child 0, k being the number of movable slots below child 0.  Leaves the builder made
of outliers (the ground and the big balls) are pinned.  The refit that follows makes the boxes; leaves apply the reference's own test, so every
arrangement renders the same pixels and only the tree's quality is at stake.  Checked here: structure, boxes and the visit rule, the rule
restated independently in NumPy, the quality the feature is for, idempotence, and the edge trees.  Nothing has a tolerance but the two quality
bounds the issue sets (<= 1.25 x the fresh build's box area after a re-sort, >= 10 x after the refit alone on a permuted lattice)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_bvh_host import EMPTY, LEAF, REF, F, _raw_scene, leaf_slots, subtree_slots
from test_refit_host import MOVES, check_boxes, check_rays, edge_scene, lattice_of, make_scene, moved_centres, raw_from_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("large", "grid40x30", "grid160x100", "grid400x250")
FLT_MAX = np.finfo(F).max

_cache = {}


def built(name):
    """(Scene, arrays, info, nodes, ids) of a scene as r1_bvh_describe builds it: computed once, never changed."""
    if name not in _cache:
        sc = make_scene(name)
        info, nodes, ids = binding.bvh_describe(sc.spheres.contents)
        _cache[name] = (sc, sc.arrays(), info, nodes, ids)
    return _cache[name]


def pinned_slots(a, info, nodes, ids):
    """The slots a re-sort must leave alone on the project's scenes: the builder peels the ground and the three big balls — every active sphere
    outside lattice_of() — into ONE leaf under the root (info.root_leaf says which child), and the lattice of near-equal radii offers no
    further outlier.  That holds for these scenes, not for the builder: it peels per node, against that node's own median radius, so a peel
    can recur below the root (tests/resort_scenes.py tiers("low"): a cluster of r = 0.1 with two r = 1.0 spheres beside a cluster of r = 1.0
    pins a second leaf at depth 3); resort_scenes.peeled_leaves restates the rule for any tree and tests/test_resort_scenes_host.py holds
    the re-sort to it.  Returned: sorted slot indices; checked: that leaf holds exactly those spheres."""
    if not info["root_leaf"]:
        return []
    ref = int(nodes[0].view(np.uint32)[REF[info["root_leaf"] - 1]])
    slots = [s for s in leaf_slots(ref) if ids[s] != EMPTY]
    outliers = np.setdiff1d(np.nonzero(a["inv_radius"] != 0)[0], lattice_of(a))
    assert sorted(int(ids[s]) for s in slots) == outliers.tolist()
    return slots


def spacing_of(a):
    """One lattice spacing: the side of the square each lattice sphere has to itself in the xz plane."""
    lat = lattice_of(a)
    x, z = a["center_x"][lat].astype(np.float64), a["center_z"][lat].astype(np.float64)
    return float(np.sqrt((x.max() - x.min()) * (z.max() - z.min()) / len(lat)))


def displaced(a, spacings, seed=7):
    """Every lattice centre displaced uniformly by up to +-spacings lattice spacings in x and z."""
    rng = np.random.default_rng(seed)
    x, y, z = (a[k].astype(F).copy() for k in ("center_x", "center_y", "center_z"))
    lat, s = lattice_of(a), spacing_of(a) * spacings
    x[lat] = (x[lat] + rng.uniform(-s, s, len(lat))).astype(F)
    z[lat] = (z[lat] + rng.uniform(-s, s, len(lat))).astype(F)
    return x, y, z


def centres(a, move):
    return displaced(a, 4.0) if move == "displace4" else moved_centres(a, move)


def box_area(nodes):
    """The summed surface area of all child boxes below the root: both children of every node but the root (whose own two boxes are the pinned
    leaf's, with the ground sphere, and the whole lattice's — the same in every arrangement), children that never pass (e = -inf) left out."""
    e = nodes[1:, 6:12].astype(np.float64).reshape(-1, 3, 2)
    w = 2.0 * e
    ok = np.isfinite(w).all(1)
    area = 2.0 * (w[:, 0] * w[:, 1] + w[:, 1] * w[:, 2] + w[:, 2] * w[:, 0])
    return float(area[ok].sum())


# ---- the entry points --------------------------------------------------------------------------------------------------------------------


def test_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rays1.h")).read()
    assert int(re.search(r"#define R1_ABI_VERSION (\d+)", header).group(1)) == 4 == binding.lib().r1_abi_version()
    bound = {name for name, _, _ in binding.SYMBOLS}
    for name in ("r1_resort_spheres", "r1_bvh_resort_describe", "r1_bvh_ids_download"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in bound, name
        getattr(binding.lib(), name)
    assert callable(binding.bvh_resort_describe) and callable(r1.Renderer.resort_spheres) and callable(r1.Renderer.bvh_ids_download)
    # NULL pointers, and radii given in part
    sc, a, info, nodes, ids = built("large")
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
    x, y, z, r = a["center_x"], a["center_y"], a["center_z"], a["radius_sq"]
    bi = binding.BvhInfo()
    call = binding.lib().r1_bvh_resort_describe
    cs = sc.spheres.contents
    assert call(None, fp(x), fp(y), fp(z), None, None, 0, C.byref(bi), None, 0, None, 0) == binding.R1_EINVAL
    assert call(C.byref(cs), None, fp(y), fp(z), None, None, 0, C.byref(bi), None, 0, None, 0) == binding.R1_EINVAL
    assert call(C.byref(cs), fp(x), fp(y), fp(z), fp(r), None, 0, C.byref(bi), None, 0, None, 0) == binding.R1_EINVAL
    assert call(C.byref(cs), fp(x), fp(y), fp(z), None, None, 0, None, None, 0, None, 0) == binding.R1_EINVAL
    assert call(C.byref(cs), fp(x), fp(y), fp(z), None, None, 0, C.byref(bi), None, 0, None, 0) == binding.R1_OK
    small = np.zeros(4, np.uint32)
    assert call(C.byref(cs), fp(x), fp(y), fp(z), None, None, 0, C.byref(bi), None, 0, small.ctypes.data_as(C.POINTER(C.c_uint32)), 4) == binding.R1_ELIMIT


# ---- structure, boxes, the visit rule ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("move", ("identity",) + MOVES)
@pytest.mark.parametrize("name", SCENES)
def test_structure_boxes_and_visit_rule(name, move):
    sc, a, info, nodes0, ids0 = built(name)
    x, y, z = centres(a, move)
    rinfo, nodes, ids = binding.bvh_resort_describe(sc.spheres.contents, x, y, z)
    # a permutation of the builder's ids; pinned and empty slots as they were
    assert ids.shape == ids0.shape and np.array_equal(np.sort(ids), np.sort(ids0))
    assert np.array_equal(ids == EMPTY, ids0 == EMPTY)
    pin = pinned_slots(a, info, nodes0, ids0)
    assert len(pin) == 4 and np.array_equal(ids[pin], ids0[pin])
    # the tree's shape
    for k in ("nodes", "leaves", "depth", "pairs", "spheres", "root_leaf", "pad_local", "stack_entries"):
        assert rinfo[k] == info[k], k
    assert rinfo["flat_axis"] == -1
    assert nodes.shape == nodes0.shape and nodes[:, 14:].tobytes() == nodes0[:, 14:].tobytes()
    # boxes and the visit rule on the re-sorted tree (grid400x250: 100 004 spheres, the boxes alone)
    assert check_boxes(nodes, ids, x, y, z, a["radius_sq"]) == 2 * len(nodes)
    if name != "grid400x250":
        check_rays(rinfo, nodes, ids, x, y, z, a["radius_sq"], a["inv_radius"] != 0, seed=13, n_rays=36 if len(nodes) <= 2000 else 18)


# ---- the rule, restated independently ---------------------------------------------------------------------------------------------------


def numpy_resort(nodes, ids0, pinned, x, y, z):
    """The rank split per node: widest axis of the centres (ties x, then y, then z), the k smallest by (coordinate, index) to child 0, k = the
    movable slots below child 0; inside a leaf the order of x.  Recursive, on sets of spheres — no lists kept sorted, no tables."""
    with np.errstate(invalid="ignore"):
        c = [np.where(np.isfinite(v), v, FLT_MAX).astype(F) + F(0.0) for v in (x, y, z)]  # (+ 0: -0 orders as +0)
    ids = ids0.copy()
    pinned = set(pinned)
    refs = nodes.view(np.uint32)

    def movable(ref):
        return [s for s in subtree_slots(nodes, ref) if ids0[s] != EMPTY and s not in pinned]

    def deal(ref, spheres):
        if ref & LEAF:
            slots = movable(ref)
            assert len(slots) == len(spheres)
            ids[slots] = spheres[np.lexsort((spheres, c[0][spheres]))]
            return
        c0, c1 = int(refs[ref][REF[0]]), int(refs[ref][REF[1]])
        k = len(movable(c0))
        if 0 < k < len(spheres):
            with np.errstate(over="ignore"):
                ext = [F(c[ax][spheres].max()) - F(c[ax][spheres].min()) for ax in range(3)]
            axis = int(np.argmax(ext))  # (the first of equal extents)
            spheres = spheres[np.lexsort((spheres, c[axis][spheres]))]
        if k:
            deal(c0, spheres[:k])
        if k < len(spheres):
            deal(c1, spheres[k:])

    deal(0, np.sort(ids0[movable(0)]))
    return ids


@pytest.mark.parametrize("move", ["permute", "jitter"])
@pytest.mark.parametrize("name", ["large", "grid40x30"])
def test_numpy_restatement_reproduces_the_ids(name, move):
    sc, a, info, nodes0, ids0 = built(name)
    x, y, z = moved_centres(a, move)
    got = binding.bvh_resort_describe(sc.spheres.contents, x, y, z)[2]
    want = numpy_resort(nodes0, ids0, pinned_slots(a, info, nodes0, ids0), x, y, z)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert not np.array_equal(got, ids0)


# ---- quality ------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("move", ["permute", "displace4"])
@pytest.mark.parametrize("name", SCENES)
def test_resorted_boxes_are_close_to_a_fresh_build(name, move):
    sc, a, info, nodes0, ids0 = built(name)
    x, y, z = centres(a, move)
    cs, keep = raw_from_arrays(a, x, y, z)
    fresh = box_area(binding.bvh_describe(cs)[1])
    resorted = box_area(binding.bvh_resort_describe(sc.spheres.contents, x, y, z)[1])
    refit = box_area(binding.bvh_refit_describe(sc.spheres.contents, x, y, z)[1])
    print(f"{name} {move}: refit {refit / fresh:.3f}, re-sort {resorted / fresh:.3f} x the fresh build's box area")
    assert resorted <= 1.25 * fresh, (resorted / fresh, refit / fresh)
    if move == "permute":
        assert refit >= 10.0 * fresh, refit / fresh  # the staleness the feature removes


# ---- idempotence --------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/check_resort_host.cpp built with r1_bvh.cpp, the one host source it drives (no sanitizer here: DESIGN.md §4.29 has that run)."""
    out = str(tmp_path_factory.mktemp("resort_host") / "check_resort_host")
    src = [os.path.join(ROOT, "tools", "check_resort_host.cpp"), os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_bvh.cpp")]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-o", out])
    return out


def test_resorting_the_resorted_arrangement_changes_nothing(check_program):
    """The re-sort is a function of the centres, the active order and the topology — not of where the spheres stand.  r1_bvh_resort_describe
    always starts from the builder's arrangement, so the stand-alone program drives the host steps themselves: the arrangement after a
    re-sort to centres A and then to centres B is the arrangement after a re-sort straight to B, and one more re-sort to B started from it
    returns it unchanged — ids, leaf table, slot table and rows."""
    sc, a, info, nodes0, ids0 = built("large")
    xb, yb, zb = moved_centres(a, "jitter")
    _, rows_b, ids_b = binding.bvh_resort_describe(sc.spheres.contents, xb, yb, zb)
    again = binding.bvh_resort_describe(sc.spheres.contents, xb, yb, zb)
    assert again[1].tobytes() == rows_b.tobytes() and again[2].tobytes() == ids_b.tobytes()  # (no state between calls)
    out = subprocess.run([check_program, "twice"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "unchanged" in out.stdout


# ---- edge trees ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_active", [0, 1, 4, 5])
def test_edge_trees(n_active):
    cs, arrs, mt = edge_scene(n_active)
    info, nodes0, ids0 = binding.bvh_describe(cs)
    rng = np.random.default_rng(50 + n_active)
    x, y, z = ((arrs[k] + rng.uniform(-3, 3, cs.count)).astype(F) for k in ("center_x", "center_y", "center_z"))
    rinfo, nodes, ids = binding.bvh_resort_describe(cs, x, y, z)
    assert np.array_equal(np.sort(ids), np.sort(ids0)) and np.array_equal(ids == EMPTY, ids0 == EMPTY)
    assert nodes[:, 14:].tobytes() == nodes0[:, 14:].tobytes()
    assert np.array_equal(ids, numpy_resort(nodes0, ids0, [], x, y, z))
    if n_active == 0:
        assert nodes.tobytes() == nodes0.tobytes()  # nothing movable: nothing happens
        return
    if n_active <= 4:  # one leaf: its spheres in the order of x
        occupied = ids[ids != EMPTY]
        assert np.array_equal(occupied, occupied[np.lexsort((occupied, x[occupied]))])
    check_boxes(nodes, ids, x, y, z, arrs["radius_sq"])
    check_rays(rinfo, nodes, ids, x, y, z, arrs["radius_sq"], arrs["inv_radius"] != 0, seed=3, n_rays=18)


def test_collapsed_centres_go_by_index():
    """All centres on one point: every extent is 0 (axis x), every key ties, and the spheres fill the movable slots in ascending index."""
    sc, a, info, nodes0, ids0 = built("large")
    x, y, z = moved_centres(a, "collapse")
    ids = binding.bvh_resort_describe(sc.spheres.contents, x, y, z)[2]
    pin = set(pinned_slots(a, info, nodes0, ids0))
    movable = [s for s in range(len(ids)) if ids0[s] != EMPTY and s not in pin]
    assert np.array_equal(ids[movable], np.sort(ids0[movable]))


def test_non_finite_centres_land_somewhere_and_the_finite_spheres_keep_their_boxes():
    sc, a, info, nodes0, ids0 = built("grid40x30")
    x, y, z = moved_centres(a, "jitter")
    lat = lattice_of(a)
    i_nan, i_inf = int(lat[len(lat) // 3]), int(lat[2 * len(lat) // 3])
    x[i_nan], z[i_inf] = np.nan, np.inf
    rinfo, nodes, ids = binding.bvh_resort_describe(sc.spheres.contents, x, y, z)
    assert np.array_equal(np.sort(ids), np.sort(ids0))
    assert not np.isnan(nodes[:, :14]).any()
    check_boxes(nodes, ids, x, y, z, a["radius_sq"])
    check_rays(rinfo, nodes, ids, x, y, z, a["radius_sq"], a["inv_radius"] != 0, seed=5, n_rays=18)
    assert np.array_equal(ids, numpy_resort(nodes0, ids0, pinned_slots(a, info, nodes0, ids0), x, y, z))  # keyed as +FLT_MAX on that axis


# ---- the stand-alone program: trees no scene reaches, and the steps run twice ---------------------------------------------------------------


def test_stand_alone_program_every_leaf_pinned_and_hand_made_trees(check_program):
    """What no scene reaches through the builder — every leaf pinned (the peel always leaves a movable rest), pinned leaves on both sides of
    movable ones — on hand-pinned trees inside the program."""
    out = subprocess.run([check_program, "trees"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "every leaf pinned: nothing moved" in out.stdout
