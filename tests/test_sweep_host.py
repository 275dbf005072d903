"""CPU tests of the sweep's tables (R1_VARIANT_PREFILTER): the host builder rays1bench_amd/csrc/r1_sweep.cpp, seen
through r1_sweep_describe.  The sweep tests GROUPS of nearby spheres against a bounding sphere and re-tests the members of flagged groups
exactly, so it computes the reference's pixels only while the group test is conservative: whenever the reference's own fp32 discriminant
accepts a member, the group must be flagged.  Checked here: the partition into groups, the covering radius and the Kp bound in float64,
the table layout the kernel reads (r1_hit_sweep.hpp sweep_prefilter, exact_trips), and the conservative property itself on rays, with the
kernel's fp32 FMA chains restated in numpy."""
import re

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes
from test_bvh_host import _raw_scene
from test_cast_host import cscene
from test_grid_host import _fma

F = np.float32
NONE = 0xFFFFFFFF


def _define(name):
    src = open(binding.os.path.join(binding.HERE, "csrc", "r1_device.h")).read()
    return float(re.search(r"#define %s\s+([0-9.]+)" % name, src).group(1))


GROUP_MAX, GROUP_MIN_SPHERES, GROUP_RATIO = int(_define("R1_GROUP_MAX")), int(_define("R1_GROUP_MIN_SPHERES")), _define("R1_GROUP_RATIO")
TILE_SPHERES, MAX_ACTIVE_10BIT = int(_define("R1_TILE_SPHERES")), int(_define("R1_MAX_ACTIVE_10BIT"))

REFERENCE = ["small", "medium", "large", "lattice"]
EDGES = [f"{name}/{size}" for name in ("coincident", "far", "inside") for size in edge_scenes.SIZES]


def scene(kind):
    """(CScene, arrays, the camera's 22 floats, whatever keeps them alive)"""
    if "/" in kind:
        sa = edge_scenes.build(*kind.split("/"))[0]
        return cscene(sa), sa.arrays, np.asarray(sa.camera_array, F), sa
    w, h = 96, 64
    sc = {"small": r1.create_small_scene, "medium": r1.create_medium_scene, "large": r1.create_large_scene}[kind](w, h) if kind != "lattice" \
        else r1.create_grid_scene(w, h, 48, 36)
    return sc.spheres.contents, sc.arrays(), sc.camera_array(), sc


def bound_radius(arrs):
    """r1_bound_radius (r1_bvh.cpp) in float64: the larger of sqrt(radius_sq) and 1 / |inv_radius|"""
    rsq, inv = arrs["radius_sq"].astype(np.float64), arrs["inv_radius"].astype(np.float64)
    from_sq = np.sqrt(np.where(rsq > 0, rsq, 0.0))
    ok = np.isfinite(inv) & (inv != 0)
    return np.maximum(from_sq, np.where(ok, 1.0 / np.abs(np.where(ok, inv, 1.0)), 0.0))


class Tables:
    """r1_sweep_describe's answer with the group rows decoded from the RAW sweep table by the layout the kernel reads, and the active
    spheres' centres, radius_sq and bound radii in active order."""

    def __init__(self, cs, arrs):
        self.d = d = binding.sweep_describe(cs)
        self.ng, self.na = d["groups"], d["spheres"]
        act = d["active"].astype(np.int64)
        self.c32 = np.stack([arrs["center_x"][act], arrs["center_y"][act], arrs["center_z"][act]], 1).astype(F)
        self.rsq = arrs["radius_sq"][act].astype(F)
        self.rb = bound_radius(arrs)[act]
        # pair layout {cx0 cx1 cy0 cy1 cz0 cz1 Kp0 Kp1}: component q of group g at [g >> 1][2 q + (g & 1)]
        sw = d["sweep"].reshape(-1, 4, 2)
        self.slot_rows = sw.transpose(0, 2, 1).reshape(-1, 4)  # [slot] {cx, cy, cz, Kp}
        self.g32 = self.slot_rows[:self.ng, :3].copy()
        self.kp = self.slot_rows[:self.ng, 3].copy()
        self.members = d["members"]
        self.n = (self.members[:self.ng] != NONE).sum(1)
        self.R, self.rule, self.c_max2 = (d["group_rows"][:, k] for k in (4, 5, 6))


def check_partition_and_layout(t, arrs):
    d, ng, na = t.d, t.ng, t.na
    fin = np.isfinite(arrs["center_x"]) & np.isfinite(arrs["center_y"]) & np.isfinite(arrs["center_z"]) & np.isfinite(arrs["radius_sq"])
    assert d["active"].tolist() == np.nonzero((arrs["inv_radius"] != 0) & fin)[0].tolist()
    assert d["group_max"] == GROUP_MAX
    # every active sphere is a member of exactly one group; a group's members fill its first n slots, the rest hold 0xFFFFFFFF
    m = t.members
    assert sorted(m[m != NONE].tolist()) == list(range(na))
    assert (m[ng:] == NONE).all()
    for k in range(GROUP_MAX):
        assert ((m[:ng, k] != NONE) == (k < t.n)).all()
    assert (t.n >= 1).all() and (d["group_rows"][:, 7] == t.n).all()
    # groups of more than one member come first, and n_multi counts them
    assert (t.n[:d["multi"]] > 1).all() and (t.n[d["multi"]:] == 1).all()
    # layout: whole chunks of 8 (big scenes: whole LDS tiles), one more chunk or tile of never-candidate padding behind them
    big = na > MAX_ACTIVE_10BIT
    step = TILE_SPHERES if big else 8
    assert d["n_sweep"] % step == 0 and d["n_sweep"] >= ng and d["n_sweep"] - ng < step
    assert d["slots"] == d["n_sweep"] + step
    assert d["sweep"].shape == (d["slots"] // 2, 8) and m.shape == (d["slots"], GROUP_MAX)
    assert (t.slot_rows[ng:, :3] == 0).all() and np.isposinf(t.slot_rows[ng:, 3]).all()
    assert (d["group_rows"][:, :4] == t.slot_rows[:ng].astype(np.float64)).all()
    # exact_g: the exact row of the member in that slot, {0, 0, 0, -inf} for none
    exact = np.concatenate([np.concatenate([t.c32, t.rsq[:, None]], 1), np.zeros((1, 4), F)])  # (+ a row for "none" to index)
    want = np.where((m != NONE)[:, :, None], exact[np.where(m != NONE, m, 0).astype(np.int64)], np.array([0, 0, 0, -np.inf], F))
    assert want.astype(F).tobytes() == d["exact_g"].tobytes()


def check_bounds(t):
    g = t.g32.astype(np.float64)
    c = t.c32.astype(np.float64)
    g2 = g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]
    rmin = np.full(t.ng, np.inf)
    for k in range(GROUP_MAX):
        have = t.members[:t.ng, k] != NONE
        a = np.where(have, t.members[:t.ng, k], 0).astype(np.int64)
        dx, dy, dz = c[a, 0] - g[:, 0], c[a, 1] - g[:, 1], c[a, 2] - g[:, 2]
        reach = np.sqrt(dx * dx + dy * dy + dz * dz) + t.rb[a]
        assert (reach[have] <= t.R[have]).all()  # the covering bound, no tolerance: R is the largest of these times 1 + 1e-12
        rmin = np.where(have, np.minimum(rmin, t.rb[a]), rmin)
        assert (t.c_max2[have] >= (c[a, 0] * c[a, 0] + c[a, 1] * c[a, 1] + c[a, 2] * c[a, 2])[have]).all()
    multi = t.n > 1
    assert (t.rule[multi] <= GROUP_RATIO * rmin[multi]).all()
    kp_max = (g2 - t.R * t.R) - 2.0 ** -15 * (np.maximum(t.c_max2, g2) + t.R * t.R)
    assert (t.kp.astype(np.float64) <= kp_max).all()
    return rmin


def check_lone_and_large(t, arrs):
    """a sphere whose radius_sq and inv_radius disagree, or one larger than 2.5 x the median bound radius, is a group of one"""
    act = t.d["active"].astype(np.int64)
    r_test = np.sqrt(np.maximum(arrs["radius_sq"][act].astype(np.float64), 0.0))
    lone = ~(r_test >= t.rb * (1.0 - 1e-3))
    large = t.rb > 2.5 * np.sort(t.rb)[t.na // 2] if t.na else np.zeros(0, bool)
    size_of = np.zeros(t.na, np.int64)
    for k in range(GROUP_MAX):
        have = t.members[:t.ng, k] != NONE
        size_of[t.members[:t.ng, k][have].astype(np.int64)] = t.n[have]
    assert (size_of[lone | large] == 1).all()
    return int(lone.sum()), int(large.sum())


# ---- the conservative property on rays ---------------------------------------------------------------------------------------------


def make_rays(t, cam, n, rng):
    """n rays: origins at the camera and at points inside the field of spheres, each aimed at a point within 1.5 bound radii of a
    randomly chosen sphere's centre.  float32 (n, 3) origins and (nearly) unit directions."""
    c = t.c32.astype(np.float64)
    k = rng.integers(0, t.na, n)
    v = rng.normal(size=(n, 3))
    aim = c[k] + v / np.linalg.norm(v, axis=1)[:, None] * (1.5 * t.rb[k] * rng.uniform(0, 1, n))[:, None]
    j = rng.integers(0, t.na, n)
    w = rng.normal(size=(n, 3))
    inside = c[j] + w / np.linalg.norm(w, axis=1)[:, None] * (t.rb[j] * rng.uniform(1.5, 4.0, n))[:, None]
    o = np.where((np.arange(n) % 2 == 0)[:, None], np.asarray(cam[0:3], np.float64)[None], inside).astype(F)
    d = aim - o.astype(np.float64)
    return o, (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)


def reference_accepts(t, o, d):
    """[ray, sphere]: the sign bit of the reference's fp32 discriminant is clear (rayweek1.cpp:192-204; exact_offer, r1_hit_sweep.hpp)"""
    ox, oy, oz, dx, dy, dz = (v[:, None] for v in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]))
    cox, coy, coz = (t.c32[None, :, 0] - ox).astype(F), (t.c32[None, :, 1] - oy).astype(F), (t.c32[None, :, 2] - oz).astype(F)
    nb = _fma(coz, dz, _fma(coy, dy, (cox * dx).astype(F)))
    cc = (_fma(coz, coz, _fma(coy, coy, (cox * cox).astype(F))) - t.rsq[None]).astype(F)
    return ~np.signbit(((nb * nb).astype(F) - cc).astype(F))


def group_flags(t, o, d):
    """[ray, group]: sweep_prefilter's test q >= Kp — two 3-FMA chains and one more FMA per group, per-ray terms as the kernel forms them"""
    ox, oy, oz, dx, dy, dz = (v[:, None] for v in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]))
    negod = (-_fma(oz, dz, _fma(oy, dy, (ox * dx).astype(F)))).astype(F)
    oo = _fma(oz, oz, _fma(oy, oy, (ox * ox).astype(F)))
    oo_adj = _fma(oo, F(-2.0 ** -15), oo)
    mx, my, mz = (F(-2.0) * ox).astype(F), (F(-2.0) * oy).astype(F), (F(-2.0) * oz).astype(F)
    cx, cy, cz = t.g32[None, :, 0], t.g32[None, :, 1], t.g32[None, :, 2]
    nb = _fma(cz, dz, _fma(cy, dy, _fma(cx, dx, negod)))
    tt = _fma(cz, mz, _fma(cy, my, _fma(cx, mx, oo_adj)))
    q = _fma(nb, nb, -tt)
    return q >= t.kp[None]


def check_conservative(t, cam, seed, n_rays=3072, chunk=256):
    rng = np.random.default_rng(seed)
    o, d = make_rays(t, cam, n_rays, rng)
    group_of = np.zeros(t.na, np.int64)
    for k in range(GROUP_MAX):
        have = t.members[:t.ng, k] != NONE
        group_of[t.members[:t.ng, k][have].astype(np.int64)] = np.nonzero(have)[0]
    rays_with_a_flag, accepted = 0, 0
    for at in range(0, n_rays, chunk):
        ref = reference_accepts(t, o[at:at + chunk], d[at:at + chunk])
        grp = group_flags(t, o[at:at + chunk], d[at:at + chunk])
        ray, sph = np.nonzero(ref)
        missed = ~grp[ray, group_of[sph]]
        assert not missed.any(), (o[at + ray[missed][0]], d[at + ray[missed][0]], int(sph[missed][0]))
        rays_with_a_flag += int(ref.any(1).sum())
        accepted += len(ray)
    # the property must not hold by missing everything: an aim point at a distance drawn evenly from [0, 1.5] radii of a centre lies
    # inside that sphere for two rays of three, and the reference accepts every one of those, whatever else stands in the way
    assert rays_with_a_flag >= 0.2 * n_rays, (rays_with_a_flag, n_rays)
    return rays_with_a_flag, accepted


@pytest.mark.parametrize("kind", REFERENCE + EDGES)
def test_tables_bounds_and_the_conservative_group_test(kind):
    cs, arrs, cam, keep = scene(kind)
    t = Tables(cs, arrs)
    check_partition_and_layout(t, arrs)
    check_bounds(t)
    lone, large = check_lone_and_large(t, arrs)
    assert lone == 0  # (the generators' radius_sq and inv_radius agree)
    if kind == "medium":  # at most R1_GROUP_MIN_SPHERES spheres: ungrouped
        assert t.na <= GROUP_MIN_SPHERES and t.ng == t.na and t.d["multi"] == 0
    if kind in ("large", "lattice"):  # the ground and the three r = 2 balls stand alone, the lattice is grouped
        assert large == 4 and t.d["multi"] > 0 and t.ng < t.na // 2
    if kind == "lattice" or kind.endswith("/big"):
        assert t.na > MAX_ACTIVE_10BIT and t.d["n_sweep"] % TILE_SPHERES == 0
    check_conservative(t, cam, 500 + (REFERENCE + EDGES).index(kind))


def test_spheres_whose_two_radii_disagree_stay_alone():
    sc = r1.create_large_scene(96, 64)
    base = sc.arrays()
    act = np.nonzero(base["inv_radius"] != 0)[0]  # (without the generator's placeholders)
    n = len(act)
    c = np.stack([base["center_x"], base["center_y"], base["center_z"]], 1)[act]
    cs, arrs, mt = _raw_scene(c, np.sqrt(base["radius_sq"][act].astype(np.float64)))
    odd = np.arange(10, n, 7)
    arrs["inv_radius"][odd[0::3]] *= F(0.5)     # inv_radius says twice the radius
    arrs["inv_radius"][odd[1::3]] *= F(-1.0)    # negative: its magnitude counts
    arrs["radius_sq"][odd[2::3]] *= F(0.25)     # radius_sq says half the radius
    t = Tables(cs, arrs)
    check_partition_and_layout(t, arrs)
    check_bounds(t)
    lone, large = check_lone_and_large(t, arrs)
    assert lone == len(odd[0::3]) + len(odd[2::3]) and t.d["multi"] > 0
    check_conservative(t, sc.camera_array(), 77, n_rays=1024)


def test_empty_and_single_sphere_scenes():
    for n in (0, 1):
        cs, arrs, mt = _raw_scene(np.zeros((max(n, 1), 3)) + [1.0, 2.0, -3.0], np.full(max(n, 1), 0.5))
        if n == 0:
            arrs["inv_radius"][0] = 0.0  # a placeholder: no active sphere
        t = Tables(cs, arrs)
        assert (t.na, t.ng, t.d["multi"], t.d["n_sweep"], t.d["slots"]) == (n, n, 0, 8 * n, 8 * n + 8)
        check_partition_and_layout(t, arrs)
        check_bounds(t)
    arrs["inv_radius"][0] = np.nan  # NaN inv_radius: an error, as r1_set_scene
    with pytest.raises(binding.R1Error):
        binding.sweep_describe(cs)
