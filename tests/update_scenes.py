"""The edits r1_update_centers* and r1_update_spheres* are given on the trees where an update can go wrong, and the frames the CPU oracle
renders of the edited arrays.  CASES lists 43 scenes: the leaf shapes of tests/leaf_scenes.py (an odd sphere whose
partner word is -inf, a one-pair leaf whose second pair is the sentinel, a one-sphere leaf at the end of the pair table), the root leaves of
tests/root_leaf_scenes.py (one to four spheres, twins, the outliers at the front and at the back of the sphere table, the two-pair root
leaf of the big-scene kernels) and the edge scenes of tests/edge_scenes.py whose radii and materials are the unusual ones.

edit() changes centres, radii, materials or all three of every live sphere; dropped() is what a device-form update with inv_radius 0 leaves
behind.  frames() is edge_scenes.frames for the edited scene — same seeds, stride and cameras —, one oracle run per (scene, edit, camera,
seed), cached per process and left unchanged.  tests/test_update_scenes_host.py asserts that these expectations mean something (the edit
shows, the changed spheres are the ones the shapes are about); tests/test_gpu_update_builds.py holds every trace build to them."""
import collections
import functools
import os

import numpy as np

import r1o

import adaptive_rule as rule
import edge_scenes as es
import leaf_scenes as ls
import root_leaf_scenes as rs

F = np.float32
W, H, SPP, STRIDE, CAP = es.W, es.H, es.SPP, es.STRIDE, es.CAP
KINDS = ("move", "radii", "materials", "all")
CENTRE_KEYS = ("center_x", "center_y", "center_z")
RADIUS_KEYS = ("radius_sq", "inv_radius")
MAT_KEYS = ("mat_type", "albedo_r", "albedo_g", "albedo_b", "mat_param")
GROUND_RSQ = 1.0e4               # spheres above this radius_sq are grounds: their radius changes by one part in 2^13
LONE_MATERIALS = ((1, 0.9, 0.6, 0.2, 0.25), (0, 0.2, 0.6, 0.9, 0.0))  # a scene of one live sphere: (not metal, metal) takes this

# id, build() -> (r1o.SceneArrays, the second camera), the frames' seed; then what the tests select by
Case = collections.namedtuple("Case", "id build seed group name size order")


def _cases():
    out = []
    for name in ("n1", "n3", "n5", "n7", "behind", "coincident"):
        for size in ls.SIZES:
            out.append(Case(f"leaf-{name}-{size}", functools.partial(ls.build, name, size), ls.seed_of(name), "leaf", name, size, None))
    for name in ("k1", "k3", "k4", "k5", "twins"):
        for order in rs.ORDERS:
            for size in rs.SIZES:
                out.append(Case(f"root-{name}-{order}-{size}", functools.partial(rs.build, name, order, size), rs.SEED, "root", name, size, order))
    out.append(Case("root-wide-front-big", functools.partial(rs.build, rs.WIDE, "front", "big"), rs.SEED, "root", rs.WIDE, "big", "front"))
    for name in ("palette", "noise_lds", "inside", "deep", "far"):
        for size in es.SIZES:
            out.append(Case(f"edge-{name}-{size}", functools.partial(es.build, name, size), es.SEED[name], "edge", name, size, None))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
assert len(CASES) == len(BY_ID) == 43


def live_of(sa):
    return np.nonzero(sa.arrays["inv_radius"] != 0)[0]


def edit(sa, kind, seed=41):
    """The scene's arrays after an edit of every live sphere (inv_radius != 0): a fixed function of the arrays, the kind and the seed.
    Placeholders keep every word.
      move       every centre by its own fp32 offset, uniform in +-0.05 per axis
      radii      the PAIR is scaled, never rebuilt from a square root: radius_sq * f * f and inv_radius / f in fp32, f uniform in
                 [0.7, 1.3] per sphere, so a pair that disagrees or is degenerate stays one; grounds (radius_sq > 1e4) take f = 1 +- 2^-13
                 and rise or sink by about 0.1
      materials  the five material words of the previous live sphere (a roll by one); a lone live sphere takes a fixed other material
      all        the three together"""
    assert kind in KINDS, kind
    n = sa.count
    rng = np.random.default_rng(seed)
    shift = rng.uniform(-0.05, 0.05, (n, 3)).astype(F)
    f = rng.uniform(0.7, 1.3, n).astype(F)
    ground_f = np.where(rng.integers(0, 2, n) == 1, F(1) + F(2.0 ** -13), F(1) - F(2.0 ** -13)).astype(F)
    arr = {k: v.copy() for k, v in sa.arrays.items()}
    live = arr["inv_radius"] != 0
    idx = np.nonzero(live)[0]
    if kind in ("move", "all"):
        for a, k in enumerate(CENTRE_KEYS):
            arr[k] = np.where(live, arr[k] + shift[:, a], arr[k]).astype(F)
    if kind in ("radii", "all"):
        f = np.where(arr["radius_sq"] > F(GROUND_RSQ), ground_f, f).astype(F)
        with np.errstate(invalid="ignore", over="ignore"):
            rsq = ((arr["radius_sq"] * f).astype(F) * f).astype(F)
            inv = (arr["inv_radius"] / f).astype(F)
        arr["radius_sq"], arr["inv_radius"] = np.where(live, rsq, arr["radius_sq"]).astype(F), np.where(live, inv, arr["inv_radius"]).astype(F)
        # no pair may become one the host form refuses (r1f_hittable_radius: a finite non-zero inv_radius, a finite radius_sq)
        assert (np.isfinite(arr["radius_sq"][idx]) & np.isfinite(arr["inv_radius"][idx]) & (arr["inv_radius"][idx] != 0)).all()
    if kind in ("materials", "all"):
        if len(idx) == 1:
            new = LONE_MATERIALS[1 if int(arr["mat_type"][idx[0]]) == 1 else 0]
            for k, v in zip(MAT_KEYS, new):
                arr[k][idx[0]] = v
        elif len(idx) > 1:
            for k in MAT_KEYS:
                arr[k][idx] = sa.arrays[k][np.roll(idx, 1)]
    return r1o.SceneArrays(arr, sa.camera_array)


def dropped(sa, which):
    """The arrays a device-form update with inv_radius = 0 for the spheres `which` leaves behind: the oracle's scene has them as placeholders;
    the active order of the others is unchanged, so ties still go the same way."""
    arr = {k: v.copy() for k, v in sa.arrays.items()}
    arr["inv_radius"][np.atleast_1d(which)] = 0
    return r1o.SceneArrays(arr, sa.camera_array)


def groups_of(sa, kind=None):
    """(centers, radii, materials) of the scene's arrays as r1_update_spheres takes them; with a kind, only the groups that edit changes"""
    a = sa.arrays
    c, r, m = tuple(a[k] for k in CENTRE_KEYS), tuple(a[k] for k in RADIUS_KEYS), tuple(a[k] for k in MAT_KEYS)
    if kind is None or kind == "all":
        return c, r, m
    return (c if kind == "move" else None), (r if kind == "radii" else None), (m if kind == "materials" else None)


@functools.lru_cache(maxsize=None)
def scene(case_id, kind=None):
    """(r1o.SceneArrays, the second camera) of a case, unedited (kind None) or after edit(kind)"""
    sa, cam2 = BY_ID[case_id].build()
    return (sa if kind is None else edit(sa, kind)), cam2


class OracleFrames(dict):
    """edge_scenes.frames for any arrays: {"main": camera 0 at `seed`, CAP samples; "batch1": camera 0 at seed + STRIDE, SPP samples;
    "path1": camera 1 at seed + STRIDE, SPP samples}, each (records [H, W, spp, 4], image at that spp), read-only; a frame is rendered when
    it is first asked for."""

    def __init__(self, sa, cam2, seed):
        super().__init__()
        self.sa, self.cam2, self.seed = sa, cam2, seed

    def __missing__(self, key):
        sa, n = {"main": (self.sa, CAP), "batch1": (self.sa, SPP), "path1": (es.with_camera(self.sa, self.cam2), SPP)}[key]
        # (as many threads as the environment allows for, where it says so: the oracle would otherwise start one per hardware thread)
        img, rays, samples = r1o.render_frame(sa, r1o.make_params(W, H, n, self.seed + (0 if key == "main" else STRIDE)), want_samples=True,
                                              nthreads=int(os.environ.get("OMP_NUM_THREADS", "0") or 0))
        rec = samples.reshape(H, W, n, 4)
        rec.setflags(write=False)
        img.setflags(write=False)
        assert int(es.ray_words(rec).sum()) == rays
        self[key] = (rec, img)
        return self[key]


class Expected:
    """The oracle's frames of one scene in the form tests/test_gpu_builds_edges.py's helpers take: fr = the OracleFrames; frame0 and
    frames = [(image bytes, rays) of frame 0 and of frame 1 of a batch], path1 = frame 1 of the path, records = frame 0's records as bytes,
    full = (image bytes, rays) at the cap, main = the records at the cap; ruled(on) and prefix(n) the adaptive call's expectation.  Each is
    worked out when it is first asked for and kept."""

    def __init__(self, sa, cam2, seed):
        self.fr = OracleFrames(sa, cam2, seed)
        self._kept = {}

    def _one(self, key):
        return self.fr[key][1].tobytes(), int(es.ray_words(self.fr[key][0]).sum())

    @property
    def main(self):
        return self.fr["main"][0]

    @functools.cached_property
    def frame0(self):
        img0, rays0 = es.prefix_frame(self.main, SPP)
        return img0.tobytes(), rays0

    @functools.cached_property
    def frames(self):
        return [self.frame0, self._one("batch1")]

    @functools.cached_property
    def path1(self):
        return self._one("path1")

    @functools.cached_property
    def records(self):
        return np.ascontiguousarray(self.main[:, :, :SPP]).tobytes()

    @functools.cached_property
    def full(self):
        return self._one("main")

    def ruled(self, rule_on):
        """(the restated rule's reports, its ray count) under es.RULE (on) or with the rule off, over 16 x 16 tiles"""
        if ("ruled", rule_on) not in self._kept:
            max_delta, mean_q8 = es.RULE if rule_on else (-1, 0)
            self._kept["ruled", rule_on] = rule.restate(self.main, es.MIN_SPP, es.PASS_SPP, max_delta, mean_q8, es.ADAPT_TILE, es.ADAPT_TILE)
        return self._kept["ruled", rule_on]

    def prefix(self, n):
        """the image of the frame's first n samples"""
        if ("prefix", n) not in self._kept:
            self._kept["prefix", n] = es.prefix_frame(self.main, n)[0]
        return self._kept["prefix", n]


_expected = {}  # the one cache: key -> Expected, per process


def expected_of(key, make):
    """The Expected of the scene make() -> (sa, cam2, seed) returns, one per `key`"""
    if key not in _expected:
        _expected[key] = Expected(*make())
    return _expected[key]


def expected(case, kind=None):
    """What the GPU tests expect of `case` after edit(kind) (None: unedited), all from the oracle"""
    case = BY_ID[case] if isinstance(case, str) else case
    return expected_of((case.id, kind), lambda: scene(case.id, kind) + (case.seed,))


def frames(case, kind=None):
    """edge_scenes.frames for the edited scene: expected(case, kind)'s OracleFrames"""
    return expected(case, kind).fr


def camera_samples():
    """x, y, s of every pixel's first sample, in the order of the records: the rays of the query tests (r1_camera_rays)"""
    y, x = np.meshgrid(np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), indexing="ij")
    return x.reshape(-1), y.reshape(-1), np.zeros(W * H, np.int32)
