"""GPU tests of the re-sort where tests/test_gpu_resort.py does not go (the scenes are tests/resort_scenes.py's and
tests/test_resort_scenes_host.py asserts what they are):

  pinned below the root   trees whose builder peeled outliers again deep in the tree: the movable positions have a gap, `mslot` is not
                          contiguous by leaves and a pinned child 0 stands inside the segments;
  block edges             lattices whose movable count M stands ON every threshold of the prefix sums and of the radix sort (LEVELS and
                          LEVELS + 1) and on full last blocks (256, 512);
  keys                    signed zeros, denormals, +-FLT_MAX on every axis, +-inf and NaN on y and z across several blocks, and keys that
                          differ in one digit byte alone, so that each radix pass is alone responsible for an order.

The device's ids and rows equal r1_bvh_resort_describe's byte for byte; every render equals a FRESH context's after r1_set_scene with the
context's current spheres.  No GPU render of the re-sorted context is an expectation and nothing has a tolerance."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
import resort_scenes as rsc
from test_gpu_resort import LEVELS, SORT_BLOCK, device_equals_host, fresh, upd  # noqa: F401  (the module-scoped fixtures)
from test_gpu_update import first_difference, fresh_render, same
from test_refit_host import lattice_of, moved_centres
from test_resort_scenes_host import EDGE_GRIDS

pytestmark = pytest.mark.gpu

W, H, SPP = es.W, es.H, es.SPP
EDGE_FRAME = (96, 54, 1)
VARIANTS = (("default", binding.VARIANT_DEFAULT), ("tree", binding.VARIANT_BVH), ("reference", binding.VARIANT_REFERENCE))


def equals_host(upd, cs, x, y, z, what):
    """the device's ids and rows against r1_bvh_resort_describe of the scene `cs` was built from; returns (ids, rows)"""
    info, rows, ids = binding.bvh_resort_describe(cs, x, y, z)
    got_ids, got_rows = upd.bvh_ids_download(), upd.bvh_download()
    assert got_ids.shape == ids.shape and np.array_equal(got_ids, ids), (what, "ids", np.nonzero(got_ids != ids)[0][:8])
    assert got_rows.shape == rows.shape
    assert got_rows.tobytes() == rows.tobytes(), (what, first_difference(got_rows, rows))
    return ids, rows


# ---- pinned leaves below the root ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("move", ("permute", "far", "pinned-too"))
@pytest.mark.parametrize("which", rsc.TIERS)
def test_trees_with_pinned_leaves_below_the_root(upd, fresh, which, move):
    sa = rsc.tiers(which)
    a, cs, cam = sa.arrays, es.cscene(sa), es.ccamera(sa.camera_array)
    info, nodes0, ids0 = binding.bvh_describe(cs)
    pin = rsc.pinned_of(a, nodes0, ids0)
    assert len(rsc.peeled_leaves(a, nodes0, ids0)) >= 2
    x, y, z = rsc.tier_moves(sa, nodes0, ids0)[move]
    upd.set_scene_raw(cs, cam)
    upd.update_centers(0, x, y, z)
    upd.resort_spheres()
    ids, rows = equals_host(upd, cs, x, y, z, (which, move))
    assert np.array_equal(ids[pin], ids0[pin]) and not np.array_equal(ids, ids0)
    params = lambda variant: r1.make_params(W, H, SPP, rsc.TIER_SEED, variant=variant)
    want = fresh_render(fresh, a, cam, x, y, z, params(0))
    for tag, variant in VARIANTS:
        same(upd.render(params(variant))[:2], want, (which, move, tag))
    # a second re-sort changes no byte
    upd.resort_spheres()
    assert upd.bvh_ids_download().tobytes() == ids.tobytes() and upd.bvh_download().tobytes() == rows.tobytes(), (which, move, "second re-sort")
    # a host-form move of EVERY live sphere finds each of them: the slot table of the pinned spheres is untouched, that of the movable ones
    # was rewritten (a sphere written into another's slot would show in the frame)
    live = np.nonzero(a["inv_radius"] != 0)[0]
    rng = np.random.default_rng(23)
    x2, y2, z2 = ((v + np.where(a["inv_radius"] != 0, rng.uniform(-0.3, 0.3, len(v)), 0.0)).astype(np.float32) for v in (x, y, z))
    assert (x2[live] != x[live]).all()
    upd.update_centers(0, x2, y2, z2)
    assert upd.bvh_ids_download().tobytes() == ids.tobytes()
    want2 = fresh_render(fresh, a, cam, x2, y2, z2, params(0))
    assert want2[0].tobytes() != want[0].tobytes(), "the move must show in the frame"
    same(upd.render(params(0))[:2], want2, (which, move, "host-form move after the re-sort"))
    same(upd.render(params(binding.VARIANT_REFERENCE))[:2], want2, (which, move, "host-form move after the re-sort, reference"))
    upd.resort_spheres()
    equals_host(upd, cs, x2, y2, z2, (which, move, "re-sorted after the move"))
    same(upd.render(params(0))[:2], want2, (which, move, "re-sorted after the move"))


# ---- block edges -----------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def edge_grids():
    """(grid_w, grid_h) -> (Scene, arrays): built once, never changed"""
    out = {}
    for gw, gh in EDGE_GRIDS:
        sc = r1.create_grid_scene(EDGE_FRAME[0], EDGE_FRAME[1], gw, gh)
        out[gw, gh] = (sc, sc.arrays())
    return out


def test_the_grids_stand_on_every_threshold(edge_grids):
    m = sorted(len(lattice_of(a)) for sc, a in edge_grids.values())
    assert m == sorted(EDGE_GRIDS.values())
    assert set(m) == {v for level in LEVELS for v in (level, level + 1)} | {SORT_BLOCK, 2 * SORT_BLOCK}


@pytest.mark.parametrize("move", ("permute", "collapse"))
@pytest.mark.parametrize("grid", list(EDGE_GRIDS), ids=[f"{gw}x{gh}-M{m}" for (gw, gh), m in EDGE_GRIDS.items()])
def test_block_edges(upd, fresh, edge_grids, grid, move):
    sc, a = edge_grids[grid]
    assert len(lattice_of(a)) == EDGE_GRIDS[grid]
    x, y, z = moved_centres(a, move)
    upd.set_scene(sc)
    upd.update_centers(0, x, y, z)
    upd.resort_spheres()
    ids = device_equals_host(upd, sc, x, y, z, (grid, move))
    if move == "permute":  # (collapsed centres go by index, which on a lattice of one row is the builder's order)
        assert not np.array_equal(ids, binding.bvh_describe(sc.spheres.contents)[2])
    p = r1.make_params(*EDGE_FRAME, 777)
    same(upd.render(p)[:2], fresh_render(fresh, a, sc.camera.contents, x, y, z, p), (grid, move))


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(rsc.key_sets()))
def test_key_sets(upd, fresh, name):
    """Through the device form, which takes any bits.  A sphere with a non-finite centre can never be hit and r1_set_scene with the same arrays
    leaves it out, so the fresh context is the expectation of the non-finite sets as well (as test_gpu_resort's NaN case has it)."""
    import torch
    sc, a = rsc.grid40x30()
    x, y, z = rsc.key_sets()[name]
    upd.set_scene(sc)
    t = [torch.from_numpy(np.array(v)).cuda() for v in (x, y, z)]
    upd.update_centers_device(0, len(x), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    upd.resort_spheres()
    ids = device_equals_host(upd, sc, x, y, z, name)
    assert not np.array_equal(ids, binding.bvh_describe(sc.spheres.contents)[2])
    p = r1.make_params(W, H, SPP, 777)
    want = fresh_render(fresh, a, sc.camera.contents, x, y, z, p)
    same(upd.render(p)[:2], want, (name, "default"))
    same(upd.render(r1.make_params(W, H, SPP, 777, variant=binding.VARIANT_REFERENCE))[:2], want, (name, "reference"))
    upd.sync()
