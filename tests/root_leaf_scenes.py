"""Scenes whose box tree has the root-step shape (r1_bvh.cpp: the root is [a leaf of <= 2 pairs that every ray tests | the rest]) with every
leaf the root step's sphere-by-sphere test can meet: one sphere (its partner -inf), one full pair, two pairs with an empty
fourth slot, two full pairs — plus a control whose root leaf is the ground alone above a tree that is not flat, twins (two of the leaf's
spheres coincide: every hit on them is a tie the lower index must win) and a leaf that stands behind the camera (flagged by the lines of
many rays, offered by none).

The base is a 4 x 4 lattice of radius-0.2 spheres, pitch 0.6, resting on y = 0, seen from (0, 1, -7).  The outliers — the ground and up to
four balls of radius 1 — stand once in FRONT of the lattice in the sphere table and once at its BACK (ORDERS), so that the leaf's sphere
indices are the lowest and the highest of the scene.  SHAPE[name] is what r1_bvh_describe must report for the root leaf at the small
size: (pairs, the outliers of its slots in slot order, -1 an empty slot; flat axis); assert_shape() checks it, so a change of the builder
cannot silently take a shape away.  The `big` size adds tests/edge_scenes.py's fillers (past 1023 active spheres: the big-scene kernels);
among 1080 tiny spheres the builder peels the ground alone, so the big trees' root leaf is one sphere and its -inf partner — the
one-pair arm of the root step — and `behind`, which has no ground, has no root leaf there (asserted as well: the generic walk).
`wide` is `k4` over a 34 x 34 lattice and no fillers: 1160 spheres whose median radius is the lattice's, so the big-scene kernels meet a
root leaf of two full pairs as well (one size: `big`).
One oracle run per (scene, order, size, camera, seed, spp) is cached here.  The small size's frames and records, both orders, are also held as
fixtures from the reference's own code (tests/golden/ref_root_*.bin; tests/test_reference_edges_host.py, tests/test_gpu_reference_edges.py)."""
import functools

import numpy as np

import r1o
from rays1bench_amd import binding

import edge_scenes as es

F = np.float32
W, H, SPP, STRIDE, SEED = es.W, es.H, es.SPP, es.STRIDE, 1926
CAMERA_FROM, CAMERA_AT = (0.0, 1.0, -7.0), (0.0, 0.3, 2.0)
ORDERS = ("front", "back")
SIZES = es.SIZES

GROUND = ((0.0, -1000.0, 0.0), 1000.0)
BALLS = [((0.0, 1.0, 4.5), 1.0), ((-2.2, 1.0, 3.5), 1.0), ((2.2, 1.0, 3.5), 1.0), ((0.0, 1.0, 7.0), 1.0)]
# name -> the outliers, in table order
OUTLIERS = {
    "k1": [GROUND],
    "k2": [GROUND] + BALLS[:1],
    "k3": [GROUND] + BALLS[:2],
    "k4": [GROUND] + BALLS[:3],
    "k5": [GROUND] + BALLS[:4],
    "twins": [GROUND, BALLS[0], BALLS[0], BALLS[2]],
    "behind": [((-3.0, 1.0, -12.0), 1.0), ((-1.0, 1.0, -13.0), 1.0), ((1.0, 1.0, -14.0), 1.0), ((3.0, 1.0, -12.5), 1.0)],
}
SCENES = tuple(OUTLIERS)
OUTLIERS["wide"] = OUTLIERS["k4"]
WIDE = "wide"  # (not in SCENES: it has one size)


def lattice(name):
    n = 34 if name == WIDE else 4
    return [((i - (n - 1) / 2) * 0.6, 0.2, 2.0 + (j - 1.5) * 0.6) for j in range(n) for i in range(n)]


# name -> (pairs of the root leaf, its slots as positions in OUTLIERS[name] (-1: empty), the tree is flat along y)
SHAPE = {
    "k1": (1, [0, -1], True),
    "k2": (1, [0, 1], True),
    "k3": (2, [0, 1, 2, -1], True),
    "k4": (2, [0, 1, 2, 3], True),
    "k5": (1, [0, -1], False),
    "twins": (2, [0, 1, 2, 3], True),
    "behind": (2, [0, 1, 2, 3], True),
}


def outlier_ids(name, order):
    """The sphere indices of OUTLIERS[name], in their order."""
    k = len(OUTLIERS[name])
    n = len(lattice(name))
    return list(range(k)) if order == "front" else list(range(n, n + k))


@functools.lru_cache(maxsize=None)
def build(name, order, size, swap_twins=False):
    """(r1o.SceneArrays, the second camera's 22 floats), as tests/edge_scenes.py's build.  swap_twins: the two coincident balls of `twins`
    trade materials (the frame in which the tie went to the higher index)."""
    rng = np.random.default_rng(1900 + list(OUTLIERS).index(name))
    LATTICE = lattice(name)
    out_c, out_r = [c for c, _ in OUTLIERS[name]], [r for _, r in OUTLIERS[name]]
    lat_r = [0.2] * len(LATTICE)
    c, rad = (out_c + LATTICE, out_r + lat_r) if order == "front" else (LATTICE + out_c, lat_r + out_r)
    # (materials are drawn for [outliers, lattice] whatever the order: both orders show the same picture)
    arr = es.spheres(np.asarray(out_c + LATTICE, np.float64), np.asarray(out_r + lat_r, np.float64), rng)
    if order == "back":
        k = len(out_c)
        perm = list(range(k, k + len(LATTICE))) + list(range(k))
        arr = {key: v[perm].copy() for key, v in arr.items()}
    assert np.array_equal(arr["center_x"], np.asarray(c, np.float64)[:, 0].astype(F)) and np.array_equal(arr["radius_sq"], (np.asarray(rad, F) ** 2).astype(F))
    if swap_twins:
        a, b = outlier_ids(name, order)[1:3]
        for key in ("mat_type", "albedo_r", "albedo_g", "albedo_b", "mat_param"):
            arr[key][[a, b]] = arr[key][[b, a]]
    assert size == "big" or name != WIDE
    return es.finish(arr, es.look(CAMERA_FROM, CAMERA_AT, 50.0, W / H, 0.0, 9.0), "small" if name == WIDE else size, rng, (1.5, 0.3, 1.5))


def root_leaf_of(sa):
    """(info, pairs of the root leaf, the sphere of each of its slots with -1 for an empty one) from r1_bvh_describe; pairs = 0: the
    root has no leaf of the root step's shape."""
    info, nodes, ids = binding.bvh_describe(es.cscene(sa))
    if info["root_leaf"] == 0:
        return info, 0, []
    ref = int(np.ascontiguousarray(nodes[0, 14:16]).view(np.uint32)[info["root_leaf"] - 1])
    assert ref & 0x80000000
    first, pairs = ref & 0x0FFFFFFF, (ref >> 28) & 7
    return info, pairs, ids[2 * first:2 * first + 2 * pairs].astype(np.int32).tolist()


def assert_shape(name, order, size):
    """The root leaf holds the outliers SHAPE[name] names (small) or the ground alone (big; none for `behind`)."""
    sa, _ = build(name, order, size)
    info, pairs, slots = root_leaf_of(sa)
    want_pairs, want_slots, flat = SHAPE["k4" if name == WIDE else name] if size == "small" or name == WIDE else (1, [0, -1], False)
    oid = outlier_ids(name, order)
    if size == "big" and name == "behind":
        assert info["root_leaf"] == 0 and es.active(sa) > 1023, (name, order, info)
        return
    assert info["root_leaf"] != 0 and pairs == want_pairs, (name, order, size, info, pairs)
    assert slots == [oid[k] if k >= 0 else -1 for k in want_slots], (name, order, size, slots)
    if size == "small":
        assert (info["flat_axis"] == 1) == flat, (name, order, info)
        assert info["pad_local"] == 0 and es.active(sa) <= 1023
    else:
        assert es.active(sa) > 1023


def moved(name, order, size):
    """The scene's spheres after a move (every live sphere a little, by its own amount), as tests/leaf_scenes.py's."""
    sa, _ = build(name, order, size)
    n = len(sa.arrays["center_x"])
    shift = np.random.default_rng(98).uniform(-0.05, 0.05, (n, 3)).astype(F)
    arr = {k: v.copy() for k, v in sa.arrays.items()}
    live = arr["inv_radius"] != 0
    for a, k in enumerate(("center_x", "center_y", "center_z")):
        arr[k] = np.where(live, arr[k] + shift[:, a], arr[k]).astype(F)
    return r1o.SceneArrays(arr, sa.camera_array)


@functools.lru_cache(maxsize=None)
def oracle(name, order, size, what, spp=SPP):
    """(image bytes, rays, records as bytes) of the oracle's frame: what = "frame" (camera 0, SEED), "batch1" (camera 0, SEED + STRIDE),
    "path1" (the turned camera, SEED + STRIDE), "moved" (camera 0, SEED, the spheres of moved()) or "swapped" (`twins` with the twins'
    materials traded)."""
    sa, cam2 = build(name, order, size, what == "swapped")
    seed = SEED + (0 if what in ("frame", "moved", "swapped") else STRIDE)
    if what == "path1":
        sa = es.with_camera(sa, cam2)
    if what == "moved":
        sa = moved(name, order, size)
    img, rays, samples = r1o.render_frame(sa, r1o.make_params(W, H, spp, seed), want_samples=True)
    return img.tobytes(), int(rays), samples.tobytes()
