"""GPU test of the leaf visit that fetches both sphere pairs of a leaf whatever its pair count over the scenes of
tests/leaf_scenes.py: one to seven spheres in front of the camera — every leaf shape, a one-pair leaf whose neighbours in the pair table
stand behind it on the camera's rays, a one-pair leaf at the end of the table (its second pair is the sentinel r1_set_scene appends) — and
tests/edge_scenes.py's coincident spheres, each small (the kernels that walk the node table in LDS: one leaf_quad call per leaf) and
big (fillers past 1023 spheres: the big-scene kernels, leaves of up to four pairs, the pair loop).

Every tree entry point tests/test_gpu_builds_edges.py drives (its call list and helpers, by import), the diagnostic build, the grid
kernels' fallback walk (a camera far outside the grid's reach), r1_cast_rays and r1_trace_rays, and all of it again after
r1_update_centers, whose refit must leave the sentinel alone.  64 x 48 x 2 frames; the expectation is the CPU oracle's frame, records and
ray count, byte for byte, and for the queries the host forms' answers.  Nothing here has a tolerance."""
import functools

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import adaptive_rule as rule
import edge_scenes as es
import leaf_scenes as ls
import test_gpu_builds_edges as tbe
from test_gpu_cast import same_hits

pytestmark = pytest.mark.gpu

W, H, SPP = ls.W, ls.H, ls.SPP
TREE, TREE_STATS, GRID, GRID_STATS = binding.VARIANT_BVH, binding.VARIANT_BVH_STATS, binding.VARIANT_GRID, binding.VARIANT_GRID_STATS
FAR_FROM = (40.0, 300.0, -600.0)  # the telephoto camera of the grid's fallback: every primary ray starts beyond the grid's reach


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def set_scene(renderer, name, size, sa=None):
    built, cam2 = ls.build(name, size)
    sa = built if sa is None else sa
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    return sa, cam2


def assert_shape(name):
    """The small size's tree holds the leaves this module is about."""
    if name not in ls.LEAVES:
        return
    sa, _ = ls.build(name, "small")
    info, nodes, ids = binding.bvh_describe(es.cscene(sa))
    assert ls.leaves_of(nodes) == ls.LEAVES[name] and ids.astype(np.int32).tolist() == ls.IDS[name], (ls.leaves_of(nodes), ids)


def frames(name, size, call):
    f0 = ls.oracle(name, size, "frame")[:2]
    if call == "batch":
        return [f0, ls.oracle(name, size, "batch1")[:2]]
    if call == "path":
        return [f0, ls.oracle(name, size, "path1")[:2]]
    return [f0]


def adaptive(renderer, name, size, rule_on):
    """tests/test_gpu_builds_edges.py's adaptive call: the restated rule on the oracle's records at the cap (rule off: the full frame)."""
    img_full, rays_full, records = ls.oracle(name, size, "frame", es.CAP)
    main = np.frombuffer(records, np.float32).reshape(H, W, es.CAP, 4)
    max_delta, mean_q8 = es.RULE if rule_on else (-1, 0)
    img, rays, tiles, res = renderer.render_adaptive(tbe.params(TREE, ls.seed_of(name), es.CAP, es.ADAPT_TILE), es.MIN_SPP, es.PASS_SPP,
                                                    max_delta, mean_q8)
    want_tiles, want_rays = rule.restate(main, es.MIN_SPP, es.PASS_SPP, max_delta, mean_q8, es.ADAPT_TILE, es.ADAPT_TILE)
    for f in ("spp", "settled", "err_max", "err_sum"):
        assert np.array_equal(tiles[f], want_tiles[f]), (f, tiles[f], want_tiles[f])
    assert rays == want_rays
    boxes = rule.tile_boxes(W, H, es.ADAPT_TILE, es.ADAPT_TILE)
    for n in sorted(set(int(x) for x in tiles["spp"])):
        want = es.prefix_frame(main, n)[0]
        for t, (x0, y0, x1, y1) in enumerate(boxes):
            if int(tiles[t]["spp"]) == n:
                assert img[y0:y1, x0:x1].tobytes() == want[y0:y1, x0:x1].tobytes(), (n, t)
    if not rule_on:
        assert (img.tobytes(), rays) == (img_full, rays_full)


@pytest.mark.parametrize("call", tbe.CALLS)
@pytest.mark.parametrize("size", ls.SIZES)
@pytest.mark.parametrize("name", ls.SCENES)
def test_every_tree_call_renders_the_oracles_frame(renderer, name, size, call):
    assert_shape(name)
    sa, cam2 = set_scene(renderer, name, size)
    if call.startswith("adaptive"):
        adaptive(renderer, name, size, call == "adaptive")
        assert renderer.launch_info()["kernel"] == TREE
        return
    got = tbe.run(renderer, sa, cam2, call, TREE, ls.seed_of(name))
    tbe.check(renderer, got, frames(name, size, call), TREE, size)
    if call == "sync":
        tbe.check_records(got[0][2], ls.oracle(name, size, "frame")[2])


@pytest.mark.parametrize("size", ls.SIZES)
@pytest.mark.parametrize("name", ls.SCENES)
def test_the_diagnostic_build_renders_the_oracles_frame(renderer, name, size):
    sa, cam2 = set_scene(renderer, name, size)
    got = tbe.run(renderer, sa, cam2, "sync", TREE_STATS, ls.seed_of(name))
    tbe.check(renderer, got, frames(name, size, "sync"), TREE_STATS, size)
    tbe.check_records(got[0][2], ls.oracle(name, size, "frame")[2])


@functools.lru_cache(maxsize=None)
def far_scene(name, size):
    """The scene seen through a telephoto lens from FAR_FROM, and the oracle's frame."""
    sa, _ = ls.build(name, size)
    at = np.array([sa.arrays[k][0] for k in ("center_x", "center_y", "center_z")], np.float64)
    dist = float(np.linalg.norm(np.asarray(FAR_FROM) - at))
    far = es.with_camera(sa, es.look(FAR_FROM, at, 1.2, W / H, 0.0, dist))
    img, rays, _ = r1o.render_frame(far, r1o.make_params(W, H, SPP, ls.seed_of(name)), want_samples=True)
    return far, img.tobytes(), int(rays)


@pytest.mark.parametrize("size", ls.SIZES)
@pytest.mark.parametrize("name", ls.SCENES)
def test_the_grids_fallback_walk_renders_the_oracles_frame(renderer, name, size):
    far, img, rays = far_scene(name, size)
    o = far.camera_array[0:3]
    d = (far.camera_array[3:6] + 0.5 * far.camera_array[6:9] + 0.5 * far.camera_array[9:12] - o).astype(np.float32)
    assert binding.grid_visit(es.cscene(far), o, d / np.linalg.norm(d))[3], "the camera is within the grid's reach: no fallback"
    set_scene(renderer, name, size, far)
    for variant in (GRID, GRID_STATS):
        got = tbe.run(renderer, far, None, "sync", variant, ls.seed_of(name))
        tbe.check(renderer, got, [(img, rays)], variant, size)
    assert renderer.last_stats()["raw"][14] > 0  # lanes that took the fallback


def query_rays(sa):
    """237 camera rays spread over the frame, the same from FAR_FROM's side (the grid's fallback), and 16 that start inside the scene."""
    near = es.primary_rays(sa.camera_array)[::13]
    far = near.copy()
    far[:, 0:3] = near[:, 0:3] + 900.0 * (near[:, 4:7] / np.linalg.norm(near[:, 4:7], axis=1, keepdims=True)) * np.float32(-1.0)
    inner = near[:16].copy()
    inner[:, 0:3] = (0.0, 0.6, 1.5)
    inner[:, 4:7] = np.random.default_rng(5).normal(0.0, 1.0, (16, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([near, far, inner]).astype(np.float32))


def check_queries(renderer, sa, tag, variants=(TREE, GRID)):
    rays = query_rays(sa)
    cs = es.cscene(sa)
    want = binding.cast_rays_host(cs, rays)
    assert (want["index"] >= 0).any()
    want_any = binding.cast_rays_host(cs, rays, binding.CAST_ANY)
    radiance = binding.trace_rays_host(cs, rays)
    for variant in variants:
        same_hits(renderer.cast_rays(rays, binding.CAST_CLOSEST, variant), want, (tag, variant))
        same_hits(renderer.cast_rays(rays, binding.CAST_ANY, variant), want_any, (tag, variant, "any"))
        assert renderer.trace_rays(rays, variant=variant).tobytes() == radiance.tobytes(), (tag, variant)


@pytest.mark.parametrize("size", ls.SIZES)
@pytest.mark.parametrize("name", ls.SCENES)
def test_ray_queries_equal_the_host_forms(renderer, name, size):
    sa, _ = set_scene(renderer, name, size)
    check_queries(renderer, sa, (name, size))


@pytest.mark.parametrize("size", ls.SIZES)
@pytest.mark.parametrize("name", ls.SCENES)
def test_frames_and_queries_after_a_move_are_the_moved_scenes(renderer, name, size):
    """r1_update_centers writes live slots of the pair table and refits the boxes; the sentinel pair and the odd spheres' partners stay."""
    sa, cam2 = set_scene(renderer, name, size)
    new = ls.moved(name, size)
    renderer.update_centers(0, new.arrays["center_x"], new.arrays["center_y"], new.arrays["center_z"])
    want = [ls.oracle(name, size, "moved")[:2]]
    for call in ("sync", "async"):
        got = tbe.run(renderer, new, cam2, call, TREE, ls.seed_of(name))
        tbe.check(renderer, got, want, TREE, size)
    check_queries(renderer, new, (name, size, "moved"), (TREE,))  # (the grid is not refitted: its calls are refused after a move)
