"""Host test of what tests/test_gpu_resort_edges.py and tests/test_gpu_resort_builds.py rest on (tests/resort_scenes.py; no GPU,
DESIGN.md §4.29): the builder peels per node, so a tree can have pinned leaves BELOW the root — `tiers` has such scenes, `peeled_leaves`
restates which leaves they are from the builder's rule alone, and r1_bvh_resort_describe must leave exactly those alone, whatever moves;
the key sets are what they claim to be (each digit set really leaves one radix pass alone responsible for the order); and the conditions the
GPU matrix takes for granted — a re-sort without any update already re-deals the leaves of 40 of update_scenes' 43 scenes, the roll those of
42, the flat slab goes on exactly the ten named in FLAT, and the lattices of the block-edge grids have exactly the counts at the thresholds — hold.
Nothing here has a tolerance."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
import resort_scenes as rsc
import update_scenes as us
from test_bvh_host import EMPTY, F
from test_refit_host import MOVES, check_boxes, check_rays, lattice_of, moved_centres
from test_resort_host import built, numpy_resort, pinned_slots
from test_update_scenes_host import tree_of

# the grids whose lattices stand ON the thresholds of the re-sort's kernels (tests/test_gpu_resort.py LEVELS) and on full last blocks
EDGE_GRIDS = {(17, 5): 85, (43, 2): 86, (16, 16): 256, (257, 1): 257, (32, 16): 512, (160, 136): 21760, (47, 463): 21761, (85, 257): 21845,
              (66, 331): 21846}
# the scenes of update_scenes whose builder tree has a flat slab (flat_axis 1), which a re-sort drops: `leaf-n7-small`, the small
# `root-k1/k3/k4/twins` in both orders and `edge-palette-small` — ten scenes (1 + 8 + 1)
FLAT = {"leaf-n7-small", "edge-palette-small"} | {f"root-{n}-{o}-small" for n in ("k1", "k3", "k4", "twins") for o in ("front", "back")}


@pytest.fixture(scope="module", params=rsc.TIERS)
def tier(request):
    sa = rsc.tiers(request.param)
    info, nodes, ids = binding.bvh_describe(es.cscene(sa))
    return request.param, sa, info, nodes, ids


# ---- pinned leaves below the root ----------------------------------------------------------------------------------------------------------


def test_the_rule_finds_the_one_root_leaf_of_the_projects_scenes():
    """On the lattices the restated rule and test_resort_host.pinned_slots name the same four slots"""
    for name in ("large", "grid40x30", "grid160x100"):
        sc, a, info, nodes, ids = built(name)
        assert rsc.pinned_of(a, nodes, ids) == pinned_slots(a, info, nodes, ids), name
        assert [d for d, slots in rsc.peeled_leaves(a, nodes, ids)] == [1], name


def test_tier_scenes_have_pinned_leaves_below_the_root(tier):
    which, sa, info, nodes, ids = tier
    leaves = rsc.peeled_leaves(sa.arrays, nodes, ids)
    print(which, {k: info[k] for k in ("nodes", "depth", "root_leaf", "spheres")}, leaves)
    assert len(leaves) >= 2 and max(d for d, slots in leaves) >= 3 and info["root_leaf"] == 1
    assert sorted(d for d, slots in leaves)[0] == 1
    pin = rsc.pinned_of(sa.arrays, nodes, ids)
    movable = [s for s in range(len(ids)) if ids[s] != EMPTY and s not in pin]
    if which == "both-sides":
        deep = [slots for d, slots in leaves if d >= 3][0]
        assert min(movable) < deep[0] and deep[-1] < max(movable)
    if which == "two-depths":
        assert len({d for d, slots in leaves if d >= 2}) >= 2
    if which == "placeholders":
        live = sa.arrays["inv_radius"] != 0
        assert not live[0::2].any() and live[1:2 * info["spheres"]:2].all() and int(live.sum()) == info["spheres"]


@pytest.mark.parametrize("move", ("identity",) + MOVES + ("pinned-too",))
def test_tier_scenes_resorted(tier, move):
    which, sa, info, nodes0, ids0 = tier
    a = sa.arrays
    x, y, z = rsc.tier_moves(sa, nodes0, ids0)[move] if move == "pinned-too" else moved_centres(a, move)
    rinfo, nodes, ids = binding.bvh_resort_describe(es.cscene(sa), x, y, z)
    pin = rsc.pinned_of(a, nodes0, ids0)
    assert np.array_equal(ids[pin], ids0[pin]), (which, move, "a pinned slot changed its id")
    assert np.array_equal(np.sort(ids), np.sort(ids0)) and np.array_equal(ids == EMPTY, ids0 == EMPTY)
    want = numpy_resort(nodes0, ids0, pin, x, y, z)
    assert np.array_equal(ids, want), (which, move, np.nonzero(ids != want)[0][:8])
    if move not in ("identity", "far", "coincident"):
        assert not np.array_equal(ids, ids0)
    assert nodes[:, 14:].tobytes() == nodes0[:, 14:].tobytes()
    assert check_boxes(nodes, ids, x, y, z, a["radius_sq"]) == 2 * len(nodes)
    check_rays(rinfo, nodes, ids, x, y, z, a["radius_sq"], a["inv_radius"] != 0, seed=17, n_rays=18)


def test_pinning_is_topology_not_radius(tier):
    """The pinned spheres shrunk to their node's ordinary radius (and the ground to a ball): no outlier is left, and they stay where they are"""
    which, sa, info, nodes0, ids0 = tier
    a = sa.arrays
    pin = rsc.pinned_of(a, nodes0, ids0)
    rad = np.sqrt(a["radius_sq"].astype(np.float64))
    rad[ids0[pin]] = rad[a["inv_radius"] != 0].min()
    rsq, inv = (rad * rad).astype(F), np.where(a["inv_radius"] != 0, 1.0 / np.maximum(rad, 1e-30), 0.0).astype(F)
    x, y, z = moved_centres(a, "permute")
    rinfo, nodes, ids = binding.bvh_resort_describe(es.cscene(sa), x, y, z, rsq, inv)
    edited = dict(a, radius_sq=rsq, inv_radius=inv)
    assert rsc.peeled_leaves(edited, nodes, ids) == []  # (the rule no longer names them)
    assert np.array_equal(ids[pin], ids0[pin])
    assert np.array_equal(ids, numpy_resort(nodes0, ids0, pin, x, y, z))
    assert check_boxes(nodes, ids, x, y, z, rsq) == 2 * len(nodes)


# ---- keys ----------------------------------------------------------------------------------------------------------------------------------


def test_the_key_map_restated():
    v = np.array([-np.inf, -rsc.FLT_MAX, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, rsc.FLT_MAX], F)
    k = rsc.key_of(v)
    assert k[0] == k[-1] and k[4] == k[5] and (np.diff(k[1:].astype(np.int64)) >= 0).all() and len(set(k.tolist())) == 7
    assert rsc.key_of(np.array([np.nan], F))[0] == k[-1]
    assert np.array_equal(rsc.key_of(rsc.float_of(k)), k)


@pytest.mark.parametrize("name", list(rsc.key_sets()))
def test_key_sets_resorted_on_the_host_equal_the_restatement(name):
    sc, a = rsc.grid40x30()
    info, nodes0, ids0 = binding.bvh_describe(sc.spheres.contents)
    lat = lattice_of(a)
    assert len(lat) == 1200
    x, y, z = rsc.key_sets()[name]
    rest = np.setdiff1d(np.arange(len(x)), lat)
    for v, k in zip((x, y, z), ("center_x", "center_y", "center_z")):
        assert v[rest].tobytes() == a[k][rest].tobytes()  # pinned spheres and placeholders untouched
    finite = all(np.isfinite(v[lat]).all() for v in (x, y, z))
    assert finite == (name not in rsc.NON_FINITE_SETS)
    pin = rsc.pinned_of(a, nodes0, ids0)
    rinfo, nodes, ids = binding.bvh_resort_describe(sc.spheres.contents, x, y, z)
    want = numpy_resort(nodes0, ids0, pin, x, y, z)
    assert np.array_equal(ids, want), (name, np.nonzero(ids != want)[0][:8])
    assert np.array_equal(ids[pin], ids0[pin]) and not np.array_equal(ids, ids0)
    assert not np.isnan(nodes[:, :14]).any()
    keys = rsc.key_of(x[lat])
    if name == "signed-zero":
        assert np.signbit(x[lat]).sum() == 600 and (x[lat] == 0).all() and len(set(keys.tolist())) == 1
        # were -0 keyed by its own bits it would stand in front of +0: the order of x, and with it the ids, would differ
        raw = x[lat].view(np.uint32)
        wrong = np.where(raw & np.uint32(0x80000000), ~raw, raw | np.uint32(0x80000000))
        assert not np.array_equal(np.lexsort((lat, wrong)), np.lexsort((lat, keys)))
    if name == "denormals":
        tiny = np.finfo(F).tiny
        assert (np.abs(x[lat]) < tiny).all() and (x[lat] != 0).sum() > 1000 and np.signbit(x[lat]).sum() > 400
        assert len(set(keys.tolist())) == 13  # -6 .. 6 times the smallest denormal, the two zeros one key
    if name == "flt-max":
        with np.errstate(over="ignore"):
            ext = [F(v[lat].max()) - F(v[lat].min()) for v in (x, y, z)]
        assert all(np.isposinf(e) for e in ext)
        assert len({tuple(t) for t in np.stack([np.sign(v[lat]) for v in (x, y, z)], 1).tolist()}) == 8
    if name in rsc.NON_FINITE_SETS:
        for v in (y, z):
            w = v[lat]
            for test in (np.isnan, np.isposinf, np.isneginf):
                where = np.nonzero(test(w))[0]
                assert len(set((where // 256).tolist())) == 5, (name, "every block of the 1200 has one")
        assert np.isfinite(x[lat]).all()
    if name in rsc.DIGIT_SETS:
        byte = rsc.DIGIT_SETS.index(name)
        mask = np.uint32(255) << np.uint32(8 * byte)
        assert len(set((keys & ~mask).tolist())) == 1 and len(set((keys & mask).tolist())) == 250
        assert len(set(y[lat].tolist())) == 1 and len(set(z[lat].tolist())) == 1
        order = np.lexsort((np.arange(1200), keys))
        without = np.lexsort((np.arange(1200), keys & ~mask))  # the other three passes alone: the order of the index
        assert not np.array_equal(order, without) and np.array_equal(without, np.arange(1200))
        for edge in (256, 512, 768, 1024):
            assert keys[edge - 1] == keys[edge], (name, edge, "a pair of equal keys straddles every block edge")
        # x is every splitting node's axis, so the ids are the x list's order dealt into the movable slots
        movable = [s for s in range(len(ids)) if ids0[s] != EMPTY and s not in set(pin)]
        assert np.array_equal(ids[movable], lat[order])


# ---- what the GPU matrix takes for granted ---------------------------------------------------------------------------------------------------


def resorted_ids(case_id, sa):
    x, y, z = (sa.arrays[k] for k in us.CENTRE_KEYS)
    return binding.bvh_resort_describe(es.cscene(us.scene(case_id)[0]), x, y, z)


def test_a_resort_alone_and_the_roll_redeal_the_leaves_of_the_43_scenes():
    same_identity, same_roll, flat = [], [], set()
    for cid in us.IDS:
        sa, _ = us.scene(cid)
        info, nodes, ids = tree_of(cid)
        rinfo, rnodes, rids = resorted_ids(cid, sa)
        if np.array_equal(rids, ids):
            same_identity.append(cid)
        new = rsc.rolled(sa)
        assert (new.arrays["inv_radius"] != 0).tolist() == (sa.arrays["inv_radius"] != 0).tolist()
        for k in us.RADIUS_KEYS + us.MAT_KEYS:
            assert new.arrays[k].tobytes() == sa.arrays[k].tobytes()
        if np.array_equal(resorted_ids(cid, new)[2], ids):
            same_roll.append(cid)
        assert info["flat_axis"] in (-1, 1) and rinfo["flat_axis"] == -1
        if info["flat_axis"] == 1:
            flat.add(cid)
    print("a re-sort alone keeps the ids of", same_identity, "; after the roll of", same_roll)
    assert len(us.IDS) - len(same_identity) >= 40, same_identity
    assert len(us.IDS) - len(same_roll) >= 42, same_roll
    for cid in ("root-twins-front-small", "leaf-coincident-small", "leaf-coincident-big", "leaf-n3-big", "leaf-n7-small"):
        assert cid not in same_identity, cid
    assert flat == FLAT, sorted(flat ^ FLAT)


def test_the_grids_stand_on_the_thresholds():
    from test_gpu_resort import LEVELS, SORT_BLOCK
    got = {}
    for (gw, gh), m in EDGE_GRIDS.items():
        sc = r1.create_grid_scene(96, 54, gw, gh)
        got[gw, gh] = len(lattice_of(sc.arrays()))
        sc.close()
    assert got == EDGE_GRIDS, got
    counts = set(EDGE_GRIDS.values())
    for level in LEVELS:
        assert {level, level + 1} <= counts, level
    assert {SORT_BLOCK, 2 * SORT_BLOCK} <= counts  # full last blocks
