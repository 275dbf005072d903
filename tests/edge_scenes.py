"""Scenes that reach what the generators' scenes do not: deep paths, the edges of the materials' parameters, ties, hits by rounding alone,
a camera inside a sphere, axis-parallel rays and a cluster 8e4 units out — each in a `small` size (the small-scene kernels: at most 1023
active spheres and 256 tree nodes) and a `big` one (the same spheres plus tiny fillers, past 1023), with a second camera a few degrees off
the first.  tests/test_edge_scenes_host.py asserts on the CPU oracle's records that every scene shows its property in every frame the GPU
tests render; tests/test_gpu_builds_edges.py and tests/test_gpu_cast_edges.py run every trace build and the ray queries over them.

The geometry restates what tests/test_gpu_bvh.py and tests/test_gpu_configs.py construct (their helpers, their generators' seeds); the
`palette` scene is new, and so is `noise_lds`: a tree of mostly tiny spheres measures its pad per node and then runs through the big-scene
tree kernels whatever its size, as `noise`/small does, so `noise_lds` takes hits by rounding alone through the small-scene tree kernels.  One oracle run per (scene, size, camera, seed) is cached here and shared by the test modules: a sample depends
on (seed, pixel, sample index) only, so the run at the largest spp holds every smaller frame as a prefix.

The small size's expectations — frames, records and the hits of every fourth query ray — are also held as fixtures from the reference's own
code (tests/golden/ref_edge_*.bin), to which tests/test_reference_edges_host.py holds the oracle and tests/test_gpu_reference_edges.py the kernels."""
import ctypes as C
import functools

import numpy as np

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import adaptive_rule as rule
from test_cast_host import cscene
from test_gpu_cast import unit_ball

F = np.float32
SCENES = ("deep", "palette", "coincident", "noise", "noise_lds", "inside", "axis", "far")
SIZES = ("small", "big")
W, H, SPP, STRIDE = 64, 48, 2, 7
# the adaptive call: cap, min_spp, pass_spp and 16 x 16 tiles (12 at 64 x 48)
CAP, MIN_SPP, PASS_SPP, ADAPT_TILE = 6, 2, 2, 16
# per scene: the frames' seed (frame 1 of a batch or path: seed + STRIDE); for all: the thresholds (max_delta, mean_delta_q8) of the
# adaptive call, under which no scene's map is a degenerate one (tests/test_edge_scenes_host.py)
SEED = {**dict.fromkeys(SCENES, 4321), "deep": 31}
RULE = (128, 8192)
BIG_ACTIVE = 1100          # active spheres of a big scene
TURN_DEGREES = 4.0         # the second camera
PLACEHOLDER = {"center_x": 999999999.0, "center_y": 999999999.0, "center_z": 999999999.0, "mat_type": 255}


# ---- helpers (tests/test_gpu_bvh.py: pad8, random_materials, spheres, _look) ---------------------------------------------------------


def pad8(arr):
    n = len(arr["center_x"])
    pad = (-n) % 8
    for k in arr:
        arr[k] = np.concatenate([arr[k], np.full(pad, PLACEHOLDER.get(k, 0), arr[k].dtype)])
    return arr


def random_materials(rng, n):
    mt = rng.integers(0, 3, n).astype(np.uint8)
    return {"mat_type": mt,
            "albedo_r": rng.uniform(0.1, 0.95, n).astype(F), "albedo_g": rng.uniform(0.1, 0.95, n).astype(F),
            "albedo_b": rng.uniform(0.1, 0.95, n).astype(F),
            "mat_param": np.where(mt == 2, rng.uniform(1.1, 2.4, n), rng.uniform(0, 1, n)).astype(F)}


def spheres(c, rad, rng):
    """Unpadded arrays of spheres at centres c with radii rad and random (narrow) materials."""
    c = np.asarray(c, F)
    rad = np.asarray(rad, F)
    arr = {"center_x": c[:, 0].copy(), "center_y": c[:, 1].copy(), "center_z": c[:, 2].copy(), "radius_sq": rad * rad,
           "inv_radius": (F(1.0) / rad).astype(F)}
    arr.update(random_materials(rng, len(rad)))
    return arr


def look(lookfrom, lookat, vfov, aspect, aperture, focus, vup=(0, 1, 0)):
    """The 22 floats of a camera built as the reference's Camera constructor does (rayweek1.cpp:365-380), in numpy."""
    lf, la, up = (np.asarray(x, F) for x in (lookfrom, lookat, vup))
    hh = F(np.tan(np.deg2rad(vfov) / 2))
    hw = F(aspect) * hh
    w = lf - la
    w = w / np.linalg.norm(w)
    u = np.cross(up, w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    fo = F(focus)
    ll = lf - hw * fo * u - hh * fo * v - fo * w
    return np.concatenate([lf, ll, 2 * hw * fo * u, 2 * hh * fo * v, u, v, w, [F(aperture / 2)]]).astype(F)


def small_scene_camera(w, h):
    """The 22 floats of the small scene's camera at w x h."""
    sc = r1.create_small_scene(w, h)
    try:
        return sc.camera_array().copy()
    finally:
        sc.close()


def turned(cam, degrees=TURN_DEGREES):
    """`cam` turned about the vertical axis through its origin: the second camera of a scene (same origin, so what is clear of the one's
    first metre is clear of the other's)."""
    a = np.deg2rad(degrees)
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    c = np.asarray(cam, np.float64)
    out = c.copy()
    out[3:6] = c[0:3] + rot @ (c[3:6] - c[0:3])
    for k in (6, 9, 12, 15, 18):
        out[k:k + 3] = rot @ c[k:k + 3]
    return out.astype(F)


def with_fillers(arr, origin, rng, spread):
    """The big size: tiny spheres (radius 0.01 .. 0.06, random materials) scattered around the scene's own spheres — centre = a sphere of
    the field (radius < 100) + N(0, spread) — until BIG_ACTIVE are active.  None within 1.2 units of the camera origin, so every camera
    ray's first metre is as in the small size.  They follow the scene's spheres: no index of those changes."""
    n0 = len(arr["center_x"])
    c0 = np.stack([arr["center_x"], arr["center_y"], arr["center_z"]], 1).astype(np.float64)
    field = np.nonzero(arr["radius_sq"] < 1.0e4)[0]
    need = BIG_ACTIVE - int((arr["inv_radius"] != 0).sum())
    cs = np.empty((0, 3))
    while cs.shape[0] < need:
        c = c0[rng.choice(field, 2 * need)] + rng.normal(0.0, 1.0, (2 * need, 3)) * np.asarray(spread, np.float64)
        cs = np.concatenate([cs, c[np.linalg.norm(c - np.asarray(origin, np.float64), axis=1) > 1.2]])
    fill = spheres(cs[:need], rng.uniform(0.01, 0.06, need), rng)
    return {k: np.concatenate([arr[k][:n0], fill[k]]) for k in arr}


def finish(arr, cam, size, rng, spread, degrees=TURN_DEGREES):
    if size == "big":
        arr = with_fillers(arr, np.asarray(cam, np.float64)[0:3], rng, spread)
    cam = np.asarray(cam, F)
    return r1o.SceneArrays(pad8(arr), cam), turned(cam, degrees)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------


def deep(size):
    """test_bvh_deep_paths_between_two_huge_spheres: a gap of two units between a floor and a ceiling sphere of radius 1000, bright
    Lambertian: paths stack more than 30 attenuations and escape sideways to the sky."""
    rng = np.random.default_rng(77)
    n = 140
    c = np.concatenate([[[0.0, -1001.0, 0.0], [0.0, 1001.0, 0.0]], rng.uniform(-6, 6, (n - 2, 3)) * np.array([1.0, 0.12, 1.0])])
    rad = np.concatenate([[1000.0, 1000.0], rng.uniform(0.05, 0.25, n - 2)])
    arr = spheres(c, rad, rng)
    arr["mat_type"][:2] = 0
    for k, v in (("albedo_r", 0.97), ("albedo_g", 0.93), ("albedo_b", 0.9)):
        arr[k][:2] = v
    cam = small_scene_camera(64, 40)
    cam[0:3] = (0.0, 0.0, 3.0)                       # origin in the middle of the gap
    cam[3:6] = (-2.0, -1.25, 3.0 - 2.0)              # lower_left
    cam[6:9], cam[9:12] = (4.0, 0.0, 0.0), (0.0, 2.5, 0.0)
    return finish(arr, cam, size, rng, (4.0, 0.3, 4.0))


PALETTE = [(0, (0.0, 0.0, 0.0), 0.0), (0, (1.0, 1.0, 1.0), 0.0), (0, (1.8, 1.6, 1.4), 0.0), (0, (0.5, 0.0, 1.0), 0.0),
           (1, (0.9, 0.9, 0.9), 0.0), (1, (0.8, 0.8, 0.8), 1.0), (1, (1.0, 1.0, 1.0), 0.0), (1, (0.7, 0.6, 0.5), 0.3),
           (2, (1.0, 1.0, 1.0), 1.0), (2, (1.0, 1.0, 1.0), 0.5), (2, (1.0, 1.0, 1.0), 2.0 / 3.0), (2, (1.0, 1.0, 1.0), 1.5),
           (2, (1.0, 1.0, 1.0), 2.4), (2, (1.0, 1.0, 1.0), 1000.0), (2, (1.0, 1.0, 1.0), 0.001)]


def palette(size):
    """A Lambertian ground of albedo 0.5 and 45 spheres of radius 0.5 on a jittered 9 x 5 lattice whose materials cycle through the edges
    of include/rays1.h's contract (fuzz <= 1, any albedo, any positive index): albedo 0, 1 and above 1 — the only input that takes a
    pixel's c * 255.99f past 255, where the reference's unclamped byte wraps —, fuzz exactly 0 and exactly 1, refraction indices at and
    below 1 (total reflection from outside, 1 - cosine at the far end of pow5) and far from 1."""
    rng = np.random.default_rng(2026)
    ij = np.stack(np.meshgrid(np.arange(9), np.arange(5), indexing="ij"), -1).reshape(-1, 2)
    c = np.zeros((46, 3))
    c[0] = (0.0, -1000.0, 0.0)
    c[1:, 0] = (ij[:, 0] - 4) * 1.15 + rng.uniform(-0.07, 0.07, 45)
    c[1:, 1] = 0.5
    c[1:, 2] = (ij[:, 1] - 2) * 1.15 + rng.uniform(-0.07, 0.07, 45)
    rad = np.concatenate([[1000.0], np.full(45, 0.5)])
    arr = spheres(c, rad, rng)
    mats = [(0, (0.5, 0.5, 0.5), 0.0)] + [PALETTE[k % len(PALETTE)] for k in range(45)]
    arr["mat_type"] = np.array([m[0] for m in mats], np.uint8)
    for ch, k in enumerate(("albedo_r", "albedo_g", "albedo_b")):
        arr[k] = np.array([m[1][ch] for m in mats], F)
    arr["mat_param"] = np.array([m[2] for m in mats], F)
    lookfrom, lookat = np.array([0.0, 4.5, 8.0]), np.array([0.0, 0.3, 0.0])
    cam = look(lookfrom, lookat, 40.0, W / H, 0.0, np.linalg.norm(lookfrom - lookat))
    return finish(arr, cam, size, rng, (0.8, 0.4, 0.8))


def coincident(size):
    """CASES["coincident"] of test_bvh_is_exact_on_adversarial_scenes: 6 spheres per centre and radius; the lowest index wins a tie."""
    rng = np.random.default_rng(100 + 6)
    n = 300
    c, rad = np.repeat(rng.uniform(-3, 3, (n // 6, 3)), 6, axis=0), np.repeat(rng.uniform(0.1, 0.6, n // 6), 6)
    return finish(spheres(c, rad, rng), small_scene_camera(W, H), size, rng, (0.6, 0.6, 0.6))


def noise(size):
    """CASES["noise_dominated"]: radius 2e-3 seen from ~600 units — discriminant error ~ 2^-22 * 3.6e5 >> r^2 = 4e-6, hits by rounding
    alone —, some spheres near the camera and a big mirror ball behind that sends rays back at the far cluster."""
    rng = np.random.default_rng(100 + 5)
    n = 300
    shift = np.array([-420.0, 380.0, 210.0], F)
    c, rad = rng.uniform(-1.5, 1.5, (n, 3)) + shift, np.full(n, 2e-3)
    c[:40] = rng.uniform(-1.5, 1.5, (40, 3))
    rad[:20] = 0.4
    rad[-1] = 300.0
    c[-1] = np.array([0.0, -302.0, 0.0])
    return finish(spheres(c, rad, rng), small_scene_camera(W, H), size, rng, (0.8, 0.8, 0.8))


NOISE_LDS_FAR = 140  # spheres 0 .. 139 of `noise_lds`: radius 2e-3, 600 units from the camera


def noise_lds(size):
    """`noise` for the small-scene tree kernels.  A tree whose median radius is tiny measures its pad per node (R1Bvh::pad_local), and such
    a tree runs through the big-scene tree kernels whatever its size: `noise`/small does.  Here fewer than half of the spheres are the
    2e-3 ones, so the small size keeps one pad and walks the node table in LDS with the packed stack; and the camera looks straight at the
    far cluster through a field of view of half a degree, so that the frame's PRIMARY rays hit by rounding alone (the 140 discs together
    cover less than a fifth of one pixel) — which r1_cast_rays_host can show.  Ordinary spheres stand behind the cluster as a background."""
    rng = np.random.default_rng(1105)
    shift = np.array([-420.0, 380.0, 210.0])
    away = shift / np.linalg.norm(shift)
    c = np.concatenate([rng.uniform(-1.5, 1.5, (NOISE_LDS_FAR, 3)) + shift, rng.uniform(-6, 6, (160, 3)) + shift + 10.0 * away])
    rad = np.concatenate([np.full(NOISE_LDS_FAR, 2e-3), rng.uniform(0.2, 0.5, 160)])
    cam = look((0.0, 0.0, 0.0), shift, 0.5, W / H, 0.0, np.linalg.norm(shift))
    return finish(spheres(c, rad, rng), cam, size, rng, (0.8, 0.8, 0.8), degrees=0.05)


def inside(size):
    """test_camera_inside_a_radius_50_sphere with a Lambertian shell: every ray starts inside sphere 0, whose far root is the hit, and
    the origin lies in every enclosing box."""
    rng = np.random.default_rng(82)
    n = 140
    c = rng.uniform(-18, 18, (n, 3))
    rad = rng.uniform(0.2, 1.6, n)
    c[0], rad[0] = (0.0, 0.0, 0.0), 50.0
    arr = spheres(c, rad, rng)
    arr["mat_type"][0], arr["mat_param"][0] = 0, 0.3
    return finish(arr, small_scene_camera(W, H), size, rng, (2.0, 2.0, 2.0))


def axis(size):
    """test_bvh_axis_parallel_rays: horizontal = vertical = 0 and no lens — every primary ray is exactly (0, 0, -1), so two reciprocal
    direction components are infinite (0 x inf in the slab and DDA arithmetic)."""
    rng = np.random.default_rng(7)
    n = 200
    c = rng.uniform(-2, 2, (n, 3))
    c[:, 2] -= 6
    c[:20, :2] = 0  # several exactly on the axis the rays run along
    arr = spheres(c, rng.uniform(0.05, 0.5, n), rng)
    cam = np.zeros(22, F)
    cam[3:6] = (0, 0, -1)                      # lower_left - origin = direction
    cam[12:15], cam[15:18], cam[18:21] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    return finish(arr, cam, size, rng, (0.7, 0.7, 0.7))


def far(size):
    """test_cluster_1e4_to_1e5_units_from_the_origin's second shift: fp32 spacing out there is the size of the small radii; the small
    scene's view, shifted with the cluster."""
    rng = np.random.default_rng(83)
    n = 200
    shift = np.array([3.0e4, -8.0e4, 1.2e4], np.float64)
    c = rng.uniform(-7, 7, (n, 3)) + shift
    rad = np.exp(rng.uniform(np.log(0.02), np.log(1.2), n))
    cam = small_scene_camera(W, H).astype(np.float64)
    cam[0:3] += shift
    cam[3:6] += shift
    return finish(spheres(c, rad, rng), cam, size, rng, (1.5, 1.5, 1.5))


BUILDERS = {"deep": deep, "palette": palette, "coincident": coincident, "noise": noise, "noise_lds": noise_lds, "inside": inside, "axis": axis,
            "far": far}


@functools.lru_cache(maxsize=None)
def build(name, size):
    """(r1o.SceneArrays, the second camera's 22 floats)"""
    return BUILDERS[name](size)


def with_camera(sa, cam22):
    return r1o.SceneArrays(sa.arrays, cam22)


def ccamera(cam22):
    cc = binding.CCamera()
    cam = np.asarray(cam22, F)
    for i, n in enumerate(("origin", "lower_left", "horizontal", "vertical", "u", "v", "w")):
        setattr(cc, n, (C.c_float * 3)(*cam[3 * i:3 * i + 3].tolist()))
    cc.lens_radius = float(cam[21])
    return cc


def active(sa):
    return int((sa.arrays["inv_radius"] != 0).sum())


def primary_rays(cam22, w=W, h=H):
    """One ray through the middle of every pixel from the camera's origin (no lens), as float32 (w * h, 8) rows for the ray queries,
    pixel (x, y) at row y * w + x."""
    cam = np.asarray(cam22, F)
    u = ((np.arange(w, dtype=F) + F(0.5)) / F(w))[None, :, None]
    v = ((np.arange(h, dtype=F) + F(0.5)) / F(h))[:, None, None]
    d = (cam[3:6] + u * cam[6:9] + v * cam[9:12] - cam[0:3]).astype(F).reshape(-1, 3)
    rays = np.zeros((w * h, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = cam[0:3], np.finfo(F).max, d
    return rays


# ---- the oracle's frames ---------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def oracle_run(name, size, camera, seed, spp):
    """The oracle's records rec[H, W, spp, 4] and image for camera 0 (the scene's) or 1 (the turned one).  Callers ask for one spp per
    (scene, size, camera, seed): the largest they need."""
    sa, cam2 = build(name, size)
    if camera == 1:
        sa = with_camera(sa, cam2)
    img, rays, samples = r1o.render_frame(sa, r1o.make_params(W, H, spp, seed), want_samples=True)
    rec = samples.reshape(H, W, spp, 4)
    rec.setflags(write=False)
    img.setflags(write=False)
    assert int(ray_words(rec).sum()) == rays
    return rec, img


def ray_words(rec):
    return np.ascontiguousarray(rec[..., 3]).view(np.uint32).astype(np.uint64)


def summed(rec, n):
    """Every pixel's sum of its first n samples: sequential fp32 sums in sample order."""
    col = np.zeros(rec.shape[:2] + (3,), F)
    for s in range(n):
        col = col + rec[:, :, s, :3]
    return col


def prefix_frame(rec, n):
    """(image, rays) of the frame at spp = n <= rec.shape[2], in r1_resolve_kernel's arithmetic."""
    return rule.quantise(summed(rec, n), n), int(ray_words(rec[:, :, :n]).sum())


def scaled(rec, n):
    """A pixel's c * 255.99f before the casts (adaptive_rule.quantise's arithmetic)."""
    return np.sqrt(summed(rec, n) * (F(1.0) / F(n))) * F(255.99)


def frames(name, size):
    """What the GPU tests expect, all from the oracle: {"main": records of camera 0 at SEED[name], CAP samples; "batch1": camera 0 at
    seed + STRIDE, SPP samples; "path1": camera 1 at seed + STRIDE, SPP samples}, each as (rec, image at that spp)."""
    seed = SEED[name]
    return {"main": oracle_run(name, size, 0, seed, CAP), "batch1": oracle_run(name, size, 0, seed + STRIDE, SPP),
            "path1": oracle_run(name, size, 1, seed + STRIDE, SPP)}


# ---- the ray queries' ray set ---------------------------------------------------------------------------------------------------------


CAST_RAYS, CAST_PRIMARY, CAST_BOUNDED = 4096, 1920, 256
CAST_HIT_FRACTION = (0.2, 0.8)  # the share of the rays that must hit, every scene


def cast_primary(name, sa, cam2, rng):
    """The 1920 primary rays of a scene's cast set: the upper 30 rows of the 64 x 48 frame of camera 0.  Two scenes differ.  `deep`: the two
    radius-1000 spheres close the gap for every ray steeper than sqrt(4 / 2000) = 0.045 (the gap at distance d is 2 + d^2 / 1000), which at
    64 x 48 leaves 4 rows of misses; its rays are the rows about the horizon of the 128 x 96 frame, 8 of camera 0 and 7 of the turned
    camera, most of which escape.  `axis`: the
    frame's primary rays are one ray, so 64 of it stay and the others keep its direction — 928 exactly (0, 0, -1), 928 the turned
    camera's — but leave from origins spread over the cloud's cross-section, so that 0 x inf goes through many boxes, cells and leaves."""
    if name == "deep":
        return np.concatenate([primary_rays(sa.camera_array, 128, 96)[44 * 128:52 * 128], primary_rays(cam2, 128, 96)[44 * 128:51 * 128]])
    if name != "axis":
        return primary_rays(sa.camera_array)[(H - 30) * W:]
    one, two = primary_rays(sa.camera_array)[:64], primary_rays(cam2)[:1]
    beams = np.concatenate([np.repeat(one[:1], 928, 0), np.repeat(two, 928, 0)])
    beams[:, 0:3] = np.stack([rng.uniform(-2.2, 2.2, 1856), rng.uniform(-2.2, 2.2, 1856), rng.uniform(0.0, 1.0, 1856)], 1).astype(F)
    return np.concatenate([one, beams])


@functools.lru_cache(maxsize=None)
def cast_rays(name, size):
    """4096 rays, float32 (n, 8) rows {o, t_max, d, -}: 1920 primary rays (cast_primary: no lens, through the pixels' middles), 1920 scatter
    rays from their hit points — origin p, direction n + a point of the unit ball, as ray_mix of tests/test_gpu_cast.py builds them — and
    a sixteenth, 256, of those rays again with t_max at the hit's own t (a miss of that root: the compare is strict), the float below
    it and the float above it."""
    sa, cam2 = build(name, size)
    rng = np.random.default_rng(SEED[name] + (1 if size == "big" else 0))
    host = lambda r: binding.cast_rays_host(cscene(sa), r)
    primary = cast_primary(name, sa, cam2, rng)
    assert primary.shape == (CAST_PRIMARY, 8)
    h = host(primary)
    hit = np.nonzero(h["index"] >= 0)[0]
    pick = rng.choice(hit, CAST_RAYS - CAST_PRIMARY - CAST_BOUNDED)
    scatter = np.zeros((pick.size, 8), F)
    scatter[:, 0:3], scatter[:, 3] = h["p"][pick], np.finfo(F).max
    scatter[:, 4:7] = (h["n"][pick].astype(np.float64) + unit_ball(rng, pick.size)).astype(F)
    free = np.concatenate([primary, scatter])
    hf = host(free)
    hit = np.nonzero(hf["index"] >= 0)[0]
    pick = rng.choice(hit, CAST_BOUNDED, replace=hit.size < CAST_BOUNDED)
    bounded = free[pick].copy()
    t = hf["t"][pick]
    forms = np.stack([t, np.nextafter(t, F(0)), np.nextafter(t, np.finfo(F).max)])
    bounded[:, 3] = forms[np.arange(CAST_BOUNDED) % 3, np.arange(CAST_BOUNDED)]
    rays = np.ascontiguousarray(np.concatenate([free, bounded]).astype(F))
    rays.setflags(write=False)
    return rays
