"""GPU tests of the flat twins of the frames-in-flight tree kernels (r1_trace.hpp r1_flatwalk_kernel, r1_aux_kernels.hip
r1_launch_trace): a landing launch of the small-scene tree builds TP and BATCH whose tree is flat runs the kernel with the flat axis compiled
into its walk, every other launch the generic kernel, and r1_last_walk_form says which.

Every frame is 64 x 48 at 4 spp, or 33 x 40 at 3 spp (ragged tiles), and every comparison is an equality of bytes and ray counts with
R1_VARIANT_REFERENCE on the same context — the exhaustive sweep in the reference's form, which reads no tree.  Nothing here has a tolerance.

What "flat" means at a launch is the context's slab, bvh_flat_e >= 0 in the launch's arguments.  include/rays1.h: every update of a centre or
a radius DROPS the slab (it is not refitted), whatever the new values are, and an update of materials alone keeps it.  So a launch after
r1_update_centers runs the generic kernel (form 0) also where the moved spheres still lie in the plane, a launch after a materials update
the twin (form 1), and r1_set_scene with the edited arrays brings the twin back.  The scenes whose root leaf is child 1 of the root, and
flat trees without a root leaf, are built here from tests/root_leaf_scenes.py's lattice: the builder puts a peeled leaf into child 0, so no
fixture has them.  Their shapes are asserted from r1_bvh_describe, not from a render."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import edge_scenes as es
import root_leaf_scenes as rs

pytestmark = pytest.mark.gpu

F = np.float32
TREE, REFERENCE = binding.VARIANT_BVH, binding.VARIANT_REFERENCE
SHAPES = {"full": (64, 48, 4), "ragged": (33, 40, 3)}
SEED, STRIDE = 2032, 7
FLAT, GENERIC = 1, 0


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------


def lattice_scene(extra=()):
    """tests/root_leaf_scenes.py's 4 x 4 lattice of radius-0.2 spheres and its camera, followed by `extra` spheres ((centre, radius))."""
    rng = np.random.default_rng(3200 + len(extra))
    c = rs.lattice("k1") + [c for c, _ in extra]
    rad = [0.2] * 16 + [r for _, r in extra]
    arr = es.spheres(np.asarray(c, np.float64), np.asarray(rad, np.float64), rng)
    return r1o.SceneArrays(es.pad8(arr), es.look(rs.CAMERA_FROM, rs.CAMERA_AT, 50.0, rs.W / rs.H, 0.0, 9.0))


def scene(name):
    """(CScene, CCamera, the object that owns their memory) of a scene by name."""
    if name in ("large", "medium", "small"):
        sc = {"large": r1.create_large_scene, "medium": r1.create_medium_scene, "small": r1.create_small_scene}[name](64, 48)
        return sc.spheres.contents, sc.camera.contents, sc
    if name == "lattice":        # no outlier: both children of the root are inner nodes
        sa = lattice_scene()
    elif name == "leaf_child1":  # three more spheres of the lattice's size on its plane, 8 units to the right: the last child of the root, a leaf
        sa = lattice_scene(tuple(((8.0 + 0.6 * i, 0.2, 2.0), 0.2) for i in range(3)))
    elif name.startswith("edge_"):
        sa = es.build(name[5:], "small")[0]
    else:
        sa = rs.build(name, "front", "small")[0]
    return es.cscene(sa), es.ccamera(sa.camera_array), sa


# name -> (r1_bvh_info.root_leaf, flat along y, more than one node)
SCENES = {"large": (1, True, True), "k4": (1, True, True), "leaf_child1": (2, True, True), "lattice": (0, True, True),
          "edge_deep": (1, False, True), "medium": (1, False, True), "edge_coincident": (0, False, True), "small": (0, False, False)}


def describe(name):
    cs, _, keep = scene(name)
    info, nodes, _ = binding.bvh_describe(cs)
    return info, nodes


def set_scene(rend, name):
    info, nodes = describe(name)
    root_leaf, flat, inner = SCENES[name]
    assert info["root_leaf"] == root_leaf and (info["flat_axis"] == 1) == flat and (len(nodes) > 1) == inner, (name, info)
    assert info["spheres"] <= 1023 and info["pad_local"] == 0, info  # the small-scene tree kernels
    cs, cam, keep = scene(name)
    rend.set_scene_raw(cs, cam)
    return keep


# ---- frames ------------------------------------------------------------------------------------------------------------------------------


def params(shape, seed, variant):
    w, h, spp = SHAPES[shape]
    return r1.make_params(w, h, spp, seed, variant=variant)


def reference(rend, shape, seed):
    img, rays, _ = rend.render(params(shape, seed, REFERENCE))
    assert rend.launch_info()["kernel"] == REFERENCE and rend.walk_form() == GENERIC
    return img.tobytes(), rays


def same(got, want, tag):
    print(f"{tag}: {got[1]} rays, the reference counts {want[1]}")
    assert got[1] == want[1], (tag, got[1], want[1])
    diff = int((np.frombuffer(got[0], np.uint8) != np.frombuffer(want[0], np.uint8)).sum())
    assert diff == 0, f"{tag}: {diff} bytes differ from the reference's frame"


def in_flight(rend, shape, form, tag, batches=(1, 2, 3)):
    """r1_render_async and r1_render_batch_async of 1, 2 and 3 frames against the reference, and the form of each launch."""
    w, h, _ = SHAPES[shape]
    want = [reference(rend, shape, SEED + f * STRIDE) for f in range(max(batches))]
    hf = binding.HostFrames(w, h, max(batches))
    try:
        rend.render_async(params(shape, SEED, TREE), hf)
        rend.sync()
        assert rend.walk_form() == form, (tag, "async")
        info = rend.launch_info()
        assert info["kernel"] == TREE and info["tiles_in_kernel"] == 1, info
        same((hf.image(0).tobytes(), hf.rays(0)), want[0], (tag, "async"))
        for n in batches:
            hf._all[:] = 0
            rend.render_batch_async(params(shape, SEED, TREE), n, hf, seed_stride=STRIDE)
            rend.sync()
            assert rend.walk_form() == form, (tag, "batch", n)
            assert rend.launch_info()["kernel"] == TREE and rend.launch_info()["tiles_in_kernel"] == 1
            for f in range(n):
                same((hf.image(f).tobytes(), hf.rays(f)), want[f], (tag, "batch", n, f))
    finally:
        hf.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_large_scene_in_flight_runs_the_flat_twin(renderer, shape):
    set_scene(renderer, "large")
    in_flight(renderer, shape, FLAT, "large")


@pytest.mark.parametrize("name", ["edge_deep", "medium", "edge_coincident"])
def test_a_tree_that_is_not_flat_runs_the_generic_kernel(renderer, name):
    set_scene(renderer, name)
    in_flight(renderer, "full", GENERIC, name)


@pytest.mark.parametrize("name", ["leaf_child1", "k4", "lattice"])
def test_flat_trees_with_the_root_leaf_in_either_child_and_without_one(renderer, name):
    """r1_bvh_info.root_leaf 2, 1 and 0 (set_scene asserts it from r1_bvh_describe)"""
    set_scene(renderer, name)
    in_flight(renderer, "full", FLAT, name)
    in_flight(renderer, "ragged", FLAT, name, batches=(2,))


def test_a_one_node_tree(renderer):
    set_scene(renderer, "small")
    in_flight(renderer, "full", GENERIC, "small")


def test_the_synchronous_frame_keeps_the_generic_kernel(renderer):
    set_scene(renderer, "large")
    want = reference(renderer, "full", SEED)
    img, rays, _ = renderer.render(params("full", SEED, TREE))
    assert renderer.walk_form() == GENERIC and renderer.launch_info()["kernel"] == TREE
    same((img.tobytes(), rays), want, "sync")
    in_flight(renderer, "full", FLAT, "after sync", batches=(1,))  # (and the next launch in flight is the twin's again)


# ---- updates: every launch follows the tree the context holds ------------------------------------------------------------------------------


def test_updates_are_followed_launch_by_launch(renderer):
    """`k4` (the ground and three balls in front of a 4 x 4 lattice, spheres 4 .. 19): a materials update keeps the slab and the twin; a move
    inside the plane drops the slab as every centre update does, so the generic kernel serves; a lattice sphere lifted out of the plane
    likewise; r1_set_scene with the moved arrays of the first move builds a flat tree again."""
    sa = set_scene(renderer, "k4")
    a = {k: v.copy() for k, v in sa.arrays.items()}
    in_flight(renderer, "full", FLAT, "built", batches=(2,))
    lat = slice(4, 20)
    rng = np.random.default_rng(32)
    mt = np.roll(a["mat_type"][lat], 3)
    alb = [np.roll(a[k][lat], 5) for k in ("albedo_r", "albedo_g", "albedo_b")]
    renderer.update_spheres(4, materials=(mt, alb[0], alb[1], alb[2], np.where(mt == 2, F(1.5), F(0.25)).astype(F)))
    in_flight(renderer, "full", FLAT, "materials", batches=(2,))
    x = (a["center_x"][lat] + rng.uniform(-0.05, 0.05, 16)).astype(F)
    z = (a["center_z"][lat] + rng.uniform(-0.05, 0.05, 16)).astype(F)
    y = a["center_y"][lat].copy()
    renderer.update_centers(4, x, y, z)
    in_flight(renderer, "full", GENERIC, "moved in the plane", batches=(2,))
    y[5] = F(1.1)
    renderer.update_centers(4, x, y, z)
    in_flight(renderer, "full", GENERIC, "one sphere lifted", batches=(2,))
    # a new build of the arrays moved inside the plane: flat, the twin
    y[5] = a["center_y"][4 + 5]
    a["center_x"][lat], a["center_y"][lat], a["center_z"][lat] = x, y, z
    moved = r1o.SceneArrays(a, sa.camera_array)
    assert binding.bvh_describe(es.cscene(moved))[0]["flat_axis"] == 1
    renderer.set_scene_raw(es.cscene(moved), es.ccamera(moved.camera_array))
    in_flight(renderer, "full", FLAT, "rebuilt", batches=(2,))


def test_an_update_that_changes_the_roots_other_child_box(renderer):
    """The lattice's corner sphere grows and moves outward: node 0's box of the inner child changes in the refit (asserted from
    r1_bvh_download against the built table), and the next launches walk the refitted table."""
    sa = set_scene(renderer, "k4")
    a = sa.arrays
    before = renderer.bvh_download()[0].copy()
    renderer.update_spheres(4, centers=(a["center_x"][4:5] - F(0.9), a["center_y"][4:5] + F(0.3), a["center_z"][4:5] - F(0.9)),
                            radii=(np.full(1, 0.25, F), np.full(1, 2.0, F)))  # radius 0.5
    after = renderer.bvh_download()[0]
    k = 1  # (root_leaf 1: child 0 is the leaf, the other child's words are the odd ones of the first three rows)
    assert (before[k:12:2] != after[k:12:2]).any(), (before, after)
    in_flight(renderer, "full", GENERIC, "refitted", batches=(1, 3))


# ---- two contexts, two streams --------------------------------------------------------------------------------------------------------------


def test_two_contexts_one_flat_one_not_with_launches_in_flight_on_two_streams():
    torch = pytest.importorskip("torch")
    w, h, _ = SHAPES["full"]
    names, forms = ("large", "edge_deep"), (FLAT, GENERIC)
    ctxs = [r1.Renderer(0) for _ in names]
    streams = [torch.cuda.Stream() for _ in names]
    frames = [[binding.HostFrames(w, h, 1) for _ in range(3)] for _ in names]
    try:
        keep = [set_scene(c, n) for c, n in zip(ctxs, names)]
        torch.cuda.synchronize()
        for f in range(3):
            for k, c in enumerate(ctxs):
                c.render_async(params("full", SEED + 11 * f + k, TREE), frames[k][f], streams[k].cuda_stream)
                assert c.walk_form() == forms[k], (names[k], f)
        for s in streams:
            s.synchronize()
        for k, c in enumerate(ctxs):
            for f in range(3):
                same((frames[k][f].image(0).tobytes(), frames[k][f].rays(0)), reference(c, "full", SEED + 11 * f + k), (names[k], f))
        del keep
    finally:
        for row in frames:
            for hf in row:
                hf.close()
        for c in ctxs:
            c.close()
