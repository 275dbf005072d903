"""GPU test of the root step's sphere-by-sphere leaf test (leaf_root) over the scenes of tests/root_leaf_scenes.py: root
leaves of one sphere, one pair, three and four spheres, with the outliers at the front and at the back of the sphere table, twins whose
every hit is a tie, a leaf behind the camera, each small (the kernels that walk the node table in LDS) and big (the big-scene kernels; the
wide lattice gives those a two-pair root leaf).

Every tree entry point tests/test_gpu_builds_edges.py drives (its call list and helpers, by import), the diagnostic build with its records,
r1_cast_rays and r1_trace_rays against the host forms, the grid kernels' fallback walk and a frame after r1_update_centers on `k4`, and
hand-made ray batches through r1_cast_rays: a wave in which one ray grazes a ball with a discriminant of exactly 0 (the whole wave takes
the compiler's square root for that slot), one in which no slot is voted, one in which every lane flags another single sphere or none,
and one started inside a ball (the second root is the offer).  64 x 48 x 2 frames; the expectation is the CPU oracle's frame, records and
ray count, byte for byte, and for the queries the host forms' answers.  Nothing here has a tolerance."""
import functools

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import adaptive_rule as rule
import edge_scenes as es
import root_leaf_scenes as rs
import test_gpu_builds_edges as tbe
from test_gpu_cast import same_hits

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP = rs.W, rs.H, rs.SPP
TREE, TREE_STATS, GRID, GRID_STATS = binding.VARIANT_BVH, binding.VARIANT_BVH_STATS, binding.VARIANT_GRID, binding.VARIANT_GRID_STATS
FAR_FROM = (40.0, 300.0, -600.0)  # the telephoto camera of the grid's fallback: every primary ray starts beyond the grid's reach
# (scene, order, size): every scene in both orders and sizes, and the wide lattice
CASES = [(n, o, s) for n in rs.SCENES for o in rs.ORDERS for s in rs.SIZES] + [(rs.WIDE, o, "big") for o in rs.ORDERS]
IDS = ["-".join(c) for c in CASES]


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def set_scene(renderer, name, order, size, sa=None):
    rs.assert_shape(name, order, size)
    built, cam2 = rs.build(name, order, size)
    sa = built if sa is None else sa
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    return sa, cam2


def frames(name, order, size, call):
    f0 = rs.oracle(name, order, size, "frame")[:2]
    if call == "batch":
        return [f0, rs.oracle(name, order, size, "batch1")[:2]]
    if call == "path":
        return [f0, rs.oracle(name, order, size, "path1")[:2]]
    return [f0]


def adaptive(renderer, name, order, size, rule_on):
    """tests/test_gpu_builds_edges.py's adaptive call: the restated rule on the oracle's records at the cap (rule off: the full frame)."""
    img_full, rays_full, records = rs.oracle(name, order, size, "frame", es.CAP)
    main = np.frombuffer(records, np.float32).reshape(H, W, es.CAP, 4)
    max_delta, mean_q8 = es.RULE if rule_on else (-1, 0)
    img, rays, tiles, res = renderer.render_adaptive(tbe.params(TREE, rs.SEED, es.CAP, es.ADAPT_TILE), es.MIN_SPP, es.PASS_SPP, max_delta, mean_q8)
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
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_tree_call_renders_the_oracles_frame(renderer, case, call):
    name, order, size = case
    sa, cam2 = set_scene(renderer, name, order, size)
    if call.startswith("adaptive"):
        adaptive(renderer, name, order, size, call == "adaptive")
        assert renderer.launch_info()["kernel"] == TREE
        return
    got = tbe.run(renderer, sa, cam2, call, TREE, rs.SEED)
    tbe.check(renderer, got, frames(name, order, size, call), TREE, size)
    if call == "sync":
        tbe.check_records(got[0][2], rs.oracle(name, order, size, "frame")[2])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_diagnostic_build_renders_the_oracles_frame_and_records(renderer, case):
    name, order, size = case
    sa, cam2 = set_scene(renderer, name, order, size)
    got = tbe.run(renderer, sa, cam2, "sync", TREE_STATS, rs.SEED)
    tbe.check(renderer, got, frames(name, order, size, "sync"), TREE_STATS, size)
    tbe.check_records(got[0][2], rs.oracle(name, order, size, "frame")[2])
    st = renderer.last_stats()
    if name != "behind" or size == "small":
        assert st.get("root_steps", 0) > 0  # the step ran (one per walk that starts)


def query_rays(sa):
    """237 camera rays spread over the frame, the same from 900 units behind their origins, and 16 that start inside the lattice."""
    near = es.primary_rays(sa.camera_array)[::13]
    far = near.copy()
    far[:, 0:3] = near[:, 0:3] + 900.0 * (near[:, 4:7] / np.linalg.norm(near[:, 4:7], axis=1, keepdims=True)) * np.float32(-1.0)
    inner = near[:16].copy()
    inner[:, 0:3] = (0.0, 0.6, 2.0)
    inner[:, 4:7] = np.random.default_rng(5).normal(0.0, 1.0, (16, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([near, far, inner]).astype(np.float32))


def check_queries(renderer, sa, tag, variants=(TREE,)):
    rays = query_rays(sa)
    cs = es.cscene(sa)
    want = binding.cast_rays_host(cs, rays)
    want_any = binding.cast_rays_host(cs, rays, binding.CAST_ANY)
    radiance = binding.trace_rays_host(cs, rays)
    for variant in variants:
        same_hits(renderer.cast_rays(rays, binding.CAST_CLOSEST, variant), want, (tag, variant))
        same_hits(renderer.cast_rays(rays, binding.CAST_ANY, variant), want_any, (tag, variant, "any"))
        assert renderer.trace_rays(rays, variant=variant).tobytes() == radiance.tobytes(), (tag, variant)
    return want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ray_queries_equal_the_host_forms(renderer, case):
    name, order, size = case
    sa, _ = set_scene(renderer, name, order, size)
    want = check_queries(renderer, sa, case)
    if name != "behind":
        assert (want["index"] >= 0).any()


@functools.lru_cache(maxsize=None)
def far_scene(order, size):
    """`k4` seen through a telephoto lens from FAR_FROM, and the oracle's frame."""
    sa, _ = rs.build("k4", order, size)
    at = np.array([0.0, 0.3, 2.0])
    dist = float(np.linalg.norm(np.asarray(FAR_FROM) - at))
    far = es.with_camera(sa, es.look(FAR_FROM, at, 1.2, W / H, 0.0, dist))
    img, rays, _ = r1o.render_frame(far, r1o.make_params(W, H, SPP, rs.SEED), want_samples=True)
    return far, img.tobytes(), int(rays)


@pytest.mark.parametrize("size", rs.SIZES)
@pytest.mark.parametrize("order", rs.ORDERS)
def test_the_grids_fallback_walk_renders_the_oracles_frame(renderer, order, size):
    far, img, rays = far_scene(order, size)
    o = far.camera_array[0:3]
    d = (far.camera_array[3:6] + 0.5 * far.camera_array[6:9] + 0.5 * far.camera_array[9:12] - o).astype(np.float32)
    assert binding.grid_visit(es.cscene(far), o, d / np.linalg.norm(d))[3], "the camera is within the grid's reach: no fallback"
    set_scene(renderer, "k4", order, size, far)
    for variant in (GRID, GRID_STATS):
        got = tbe.run(renderer, far, None, "sync", variant, rs.SEED)
        tbe.check(renderer, got, [(img, rays)], variant, size)
    assert renderer.last_stats()["raw"][14] > 0  # lanes that took the fallback


@pytest.mark.parametrize("size", rs.SIZES)
@pytest.mark.parametrize("order", rs.ORDERS)
def test_frames_and_queries_after_a_move_are_the_moved_scenes(renderer, order, size):
    sa, cam2 = set_scene(renderer, "k4", order, size)
    new = rs.moved("k4", order, size)
    renderer.update_centers(0, new.arrays["center_x"], new.arrays["center_y"], new.arrays["center_z"])
    want = [rs.oracle("k4", order, size, "moved")[:2]]
    for call in ("sync", "async"):
        got = tbe.run(renderer, new, cam2, call, TREE, rs.SEED)
        tbe.check(renderer, got, want, TREE, size)
    check_queries(renderer, new, ("k4", order, size, "moved"))


# ---- hand-made batches of 64 rays: one wave of the cast kernel, all of them in one root step -------------------------------------------


def batch(o, d):
    rays = np.zeros((len(o), 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = np.asarray(o, F), np.finfo(F).max, np.asarray(d, F)
    return np.ascontiguousarray(rays)


def discriminants(sa, ids, rays):
    """Pass 1 of the reference's test in float32 for spheres `ids`: [ray, sphere].  (No fused multiply-add here: used only where every
    intermediate is exact, or for a sign with a margin.)"""
    a = sa.arrays
    out = np.zeros((len(rays), len(ids)), F)
    for k, i in enumerate(ids):
        co = np.stack([a["center_x"][i] - rays[:, 0], a["center_y"][i] - rays[:, 1], a["center_z"][i] - rays[:, 2]], 1).astype(F)
        nb = (co[:, 0] * rays[:, 4] + co[:, 1] * rays[:, 5] + co[:, 2] * rays[:, 6]).astype(F)
        c = ((co * co).sum(1).astype(F) - a["radius_sq"][i]).astype(F)
        out[:, k] = nb * nb - c
    return out


def cast_both(renderer, sa, rays, tag):
    want = binding.cast_rays_host(es.cscene(sa), rays)
    same_hits(renderer.cast_rays(rays, binding.CAST_CLOSEST, TREE), want, tag)
    same_hits(renderer.cast_rays(rays, binding.CAST_ANY, TREE), binding.cast_rays_host(es.cscene(sa), rays, binding.CAST_ANY), (tag, "any"))
    return want


@pytest.mark.parametrize("order", rs.ORDERS)
def test_a_wave_with_one_grazing_ray_takes_the_slow_root_for_that_slot(renderer, order):
    """Origin (0, 1, -10) + (1, 0, 0) r, direction (0, 0, 1), against the ball at (0, 1, 4.5): r = 1 exactly gives nb = 14.5, c = 210.25
    and a discriminant of exactly +0 — outside the short square root's domain, so the slot's whole wave takes the compiler's."""
    sa, _ = set_scene(renderer, "k4", order, "small")
    ground, ball = rs.outlier_ids("k4", order)[:2]
    r = (np.arange(64) - 32) / 8.0 + 1.0 / 16.0  # odd sixteenths: never +-1
    r[40] = 1.0
    rays = batch(np.stack([r, np.ones(64), np.full(64, -10.0)], 1), np.tile([0.0, 0.0, 1.0], (64, 1)))
    ds = discriminants(sa, [ball], rays)[:, 0]
    assert ds[40] == 0.0 and not np.signbit(ds[40]) and int((ds == 0.0).sum()) == 1
    want = cast_both(renderer, sa, rays, ("graze", order))
    assert want["index"][40] == ball and want["t"][40] == F(14.5)


@pytest.mark.parametrize("order", rs.ORDERS)
def test_a_wave_whose_lines_meet_no_outlier_votes_no_slot(renderer, order):
    """From five units above the ground, up and away from the balls at slopes under 0.09: the lines clear the ground sphere (5 - 500 s^2
    > 0) and pass the balls two units above their tops."""
    sa, _ = set_scene(renderer, "k4", order, "small")
    rng = np.random.default_rng(11)
    d = np.stack([rng.uniform(-0.3, 0.3, 64), rng.uniform(0.01, 0.085, 64), np.full(64, -1.0)], 1)
    d[:, 1] *= np.sqrt(d[:, 0] ** 2 + 1.0)  # (slope against the horizontal run)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    rays = batch(np.tile([0.0, 5.0, -7.0], (64, 1)), d)
    assert (discriminants(sa, rs.outlier_ids("k4", order), rays).astype(np.float64) < -1.0).all()
    want = cast_both(renderer, sa, rays, ("none", order))
    assert (want["index"] < 0).all()


@pytest.mark.parametrize("order", rs.ORDERS)
def test_a_wave_whose_lanes_each_flag_another_single_sphere_or_none(renderer, order):
    """Horizontal rays at y = 1.8 (a horizontal line never meets the ground sphere) through one ball each or between them, and rays straight
    down beside the balls: lane i flags ball 1, ball 2, ball 3, nothing or the ground alone, by i mod 5."""
    sa, _ = set_scene(renderer, "k4", order, "small")
    oid = rs.outlier_ids("k4", order)
    rng = np.random.default_rng(12)
    o, d, flagged = [], [], []
    for i in range(64):
        j = rng.uniform(-0.3, 0.3)
        kind = i % 5
        if kind < 3:
            o.append(((0.0, -2.2, 2.2)[kind] + j, 1.8, -9.0)), d.append((0.0, 0.0, 1.0)), flagged.append(oid[1 + kind])
        elif kind == 3:
            o.append((1.1 if i % 2 else -1.1, 1.8, -9.0)), d.append((0.0, 0.0, 1.0)), flagged.append(-1)
        else:
            o.append((5.0 + j, 3.0, -5.0)), d.append((0.0, -1.0, 0.0)), flagged.append(oid[0])
    rays = batch(o, d)
    clear = np.signbit(discriminants(sa, oid, rays)) == False  # noqa: E712  ([ray, outlier]: the sign bit is clear)
    for i in range(64):
        assert [oid[k] for k in np.nonzero(clear[i])[0]] == ([flagged[i]] if flagged[i] >= 0 else []), (i, clear[i])
    want = cast_both(renderer, sa, rays, ("single", order))
    assert want["index"].tolist() == flagged


@pytest.mark.parametrize("order", rs.ORDERS)
def test_a_wave_started_inside_a_ball_is_offered_the_second_root(renderer, order):
    sa, _ = set_scene(renderer, "k4", order, "small")
    ball = rs.outlier_ids("k4", order)[1]
    rng = np.random.default_rng(13)
    o = np.asarray([0.0, 1.0, 4.5]) + rng.uniform(-0.4, 0.4, (64, 3))
    d = rng.normal(0.0, 1.0, (64, 3))
    d[:, 1] = np.abs(d[:, 1])  # upwards: the ball's far side, not the ground under it
    rays = batch(o, d / np.linalg.norm(d, axis=1, keepdims=True))
    want = cast_both(renderer, sa, rays, ("inside", order))
    assert (want["index"] == ball).all() and (want["t"] > 0.5).all() and (want["t"] < 1.5).all()
