"""Scenes of one to seven spheres whose box trees hold every leaf shape a leaf visit can meet: leaves of one and of two
sphere pairs, with and without an odd sphere (partner radius_sq = -inf), a one-pair leaf followed in the pair table by another leaf's
spheres, and a one-pair leaf at the END of the table, whose second pair — fetched without a branch — is the sentinel pair r1_set_scene
appends.  LEAVES[name] is the leaf table r1_bvh_describe must report for the small size, [(first pair, pairs)] in table order, and
IDS[name] the sphere of every slot (-1: the partner of an odd sphere): tests assert them, so a change of the builder cannot silently
take a shape away.  The `big` size adds tests/edge_scenes.py's fillers (past 1023 active spheres: the big-scene kernels, leaves of up to
four pairs, the pair loop).  One oracle run per (scene, size, camera, seed, spp) is cached here.  The small size's frames and records are also
held as fixtures from the reference's own code (tests/golden/ref_leaf_*.bin; tests/test_reference_edges_host.py, tests/test_gpu_reference_edges.py)."""
import functools

import numpy as np

import r1o

import edge_scenes as es

F = np.float32
W, H, SPP, STRIDE, SEED = es.W, es.H, es.SPP, es.STRIDE, 2718
CAMERA_FROM, CAMERA_AT = (0.0, 1.0, -7.0), (0.0, 0.3, 1.0)


def row(xs):
    """Spheres of radius 0.5 side by side along x, each a little farther from the camera than the one before."""
    return [(x, 0.0, 0.2 * i) for i, x in enumerate(xs)], [0.5] * len(xs)


def centred(n):
    return [1.1 * (i - (n - 1) / 2) for i in range(n)]


# name -> (centres, radii)
LAYOUT = {
    "n1": row(centred(1)), "n2": row(centred(2)), "n3": row(centred(3)), "n4": row(centred(4)), "n6": row(centred(6)),
    # three on the left, two on the right: the LAST leaf is one full pair
    "n5": row([-2.4, -1.3, -0.2, 1.6, 2.7]),
    # six close together and one large sphere far behind them: the last leaf is ONE sphere (its partner -inf, its second pair the sentinel),
    # and it is the leaf of the root step
    "n7": ([(-1.5, 0, 0.0), (-0.5, 0, 0.2), (0.5, 0, 0.4), (1.5, 0, 0.6), (-1.0, 0.9, 0.8), (1.0, 0.9, 1.0), (0.0, 2.0, 25.0)], [0.5] * 6 + [4.0]),
    # a one-pair leaf (spheres 0 and 1) whose neighbours in the table, spheres 2 and 3, stand right behind them on the camera's rays
    "behind": ([(-0.55, 0, 0), (0.55, 0, 0), (-0.55, 0, 3.0), (0.55, 0, 3.0), (0, 0.9, 3.0)], [0.5, 0.5, 0.8, 0.8, 0.8]),
}
LEAVES = {"n1": [(0, 1)], "n2": [(0, 1)], "n3": [(0, 2)], "n4": [(0, 2)], "n5": [(0, 2), (2, 1)], "n6": [(0, 2), (2, 2)],
          "n7": [(0, 2), (2, 2), (4, 1)], "behind": [(0, 1), (1, 2)]}
IDS = {"n1": [0, -1], "n2": [0, 1], "n3": [0, 1, 2, -1], "n4": [0, 1, 2, 3], "n5": [0, 1, 2, -1, 3, 4], "n6": [0, 1, 2, -1, 3, 4, 5, -1],
       "n7": [0, 1, 4, -1, 3, 2, 5, -1, 6, -1], "behind": [0, 1, 2, 3, 4, -1]}
SCENES = tuple(LAYOUT) + ("coincident",)  # (tests/edge_scenes.py's: six spheres per centre and radius, ties)
SIZES = es.SIZES


def leaves_of(nodes):
    """[(first pair, pairs)] of the non-empty leaves a node table refers to, in table order."""
    refs = np.ascontiguousarray(nodes[:, 14:16]).view(np.uint32).ravel()
    return sorted((int(r & 0x0FFFFFFF), int((r >> 28) & 7)) for r in refs if r & 0x80000000 and (r >> 28) & 7)


@functools.lru_cache(maxsize=None)
def build(name, size):
    """(r1o.SceneArrays, the second camera's 22 floats), as tests/edge_scenes.py's build."""
    if name == "coincident":
        return es.build(name, size)
    rng = np.random.default_rng(1700 + sorted(LAYOUT).index(name))
    c, rad = LAYOUT[name]
    arr = es.spheres(np.asarray(c, np.float64), np.asarray(rad, np.float64), rng)
    dist = float(np.linalg.norm(np.subtract(CAMERA_FROM, CAMERA_AT)))
    return es.finish(arr, es.look(CAMERA_FROM, CAMERA_AT, 50.0, W / H, 0.0, dist), size, rng, (1.5, 0.6, 1.5))


def seed_of(name):
    return es.SEED[name] if name == "coincident" else SEED


def moved(name, size):
    """The scene's spheres after a move: new centres (scene indices; every sphere a little, by its own amount — no leaf keeps its box) and
    the oracle's scene for them."""
    sa, cam2 = build(name, size)
    n = len(sa.arrays["center_x"])
    rng = np.random.default_rng(99)
    shift = rng.uniform(-0.25, 0.25, (n, 3)).astype(F)
    arr = {k: v.copy() for k, v in sa.arrays.items()}
    live = arr["inv_radius"] != 0
    for a, k in enumerate(("center_x", "center_y", "center_z")):
        arr[k] = np.where(live, arr[k] + shift[:, a], arr[k]).astype(F)
    return r1o.SceneArrays(arr, sa.camera_array)


@functools.lru_cache(maxsize=None)
def oracle(name, size, what, spp=SPP):
    """(image bytes, rays, records as bytes) of the oracle's frame: what = "frame" (camera 0, the scene's seed), "batch1" (camera 0, seed +
    STRIDE), "path1" (the turned camera, seed + STRIDE) or "moved" (camera 0, the scene's seed, the spheres of moved())."""
    sa, cam2 = build(name, size)
    seed = seed_of(name) + (0 if what in ("frame", "moved") else STRIDE)
    if what == "path1":
        sa = es.with_camera(sa, cam2)
    if what == "moved":
        sa = moved(name, size)
    img, rays, samples = r1o.render_frame(sa, r1o.make_params(W, H, spp, seed), want_samples=True)
    return img.tobytes(), int(rays), samples.tobytes()
