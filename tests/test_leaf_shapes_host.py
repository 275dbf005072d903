"""Host test of the leaf tables tests/test_gpu_leaf_fetch.py relies on, and of what the sentinel pair behind the pair table must not
change: r1_bvh_describe reports the tree — its pairs, its sphere slots, its leaves — and not the sentinel, which
r1_set_scene appends for the kernels' unconditional fetch of a leaf's second pair.  (The pair table itself is not reachable from the
host: the sentinel's values are covered by the GPU test, whose one-sphere last leaf reads them.)"""
import numpy as np
import pytest

from rays1bench_amd import binding

import edge_scenes as es
import leaf_scenes as ls


@pytest.mark.parametrize("name", sorted(ls.LEAVES))
def test_the_small_scenes_have_the_leaf_shapes_the_gpu_test_is_about(name):
    sa, _ = ls.build(name, "small")
    info, nodes, ids = binding.bvh_describe(es.cscene(sa))
    leaves = ls.leaves_of(nodes)
    assert leaves == ls.LEAVES[name]
    assert ids.astype(np.int32).tolist() == ls.IDS[name]
    # the counts are the tree's own: every pair belongs to a leaf, every active sphere has one slot, nothing stands behind the last leaf
    n = es.active(sa)
    assert info["spheres"] == n == int((ids != 0xFFFFFFFF).sum()) and sorted(ids[ids != 0xFFFFFFFF].tolist()) == list(range(n))
    assert info["pairs"] == ids.size // 2 == sum(p for _, p in leaves) == leaves[-1][0] + leaves[-1][1]
    assert info["leaves"] == len(leaves) and all(1 <= p <= 2 for _, p in leaves)
    assert [f for f, _ in leaves] == [sum(p for _, p in leaves[:k]) for k in range(len(leaves))]  # (back to back)


def test_the_shapes_cover_what_a_leaf_visit_can_meet():
    last = {name: ls.LEAVES[name][-1] for name in ls.LEAVES}
    assert last["n5"][1] == 1 and ls.IDS["n5"][-2:] == [3, 4]   # the last leaf is one full pair
    assert last["n7"][1] == 1 and ls.IDS["n7"][-2:] == [6, -1]  # the last leaf is one sphere: partner -inf, then the sentinel pair
    assert ls.LEAVES["behind"][0] == (0, 1) and ls.IDS["behind"][:4] == [0, 1, 2, 3]  # a one-pair leaf, real spheres right behind it in the table
    c, _ = ls.LAYOUT["behind"]
    assert c[2][:2] == c[0][:2] and c[3][:2] == c[1][:2] and c[2][2] > c[0][2]        # ... and behind it in space, seen from the camera
    assert {p for v in ls.LEAVES.values() for _, p in v} == {1, 2}
    info, _, _ = binding.bvh_describe(es.cscene(ls.build("n7", "small")[0]))
    assert info["root_leaf"] != 0  # the one-sphere leaf is the root step's


@pytest.mark.parametrize("name", ls.SCENES)
def test_the_big_sizes_have_leaves_of_odd_pair_counts(name):
    """Leaves of up to 8 spheres: the pair loop of the big-scene kernels ends on a step of ONE pair for 1 and 3 pairs."""
    sa, _ = ls.build(name, "big")
    assert es.active(sa) > 1023
    info, nodes, ids = binding.bvh_describe(es.cscene(sa))
    counts = {p for _, p in ls.leaves_of(nodes)}
    assert counts & {1, 3} and max(counts) <= 4 and info["pairs"] == ids.size // 2
