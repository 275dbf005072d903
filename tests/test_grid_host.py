"""CPU tests of the uniform grid (R1_VARIANT_GRID): the host builder (r1_grid_describe) and the kernel's own walk
arithmetic and stopping rule, run on the host (r1_grid_visit, r1_grid_dda.h), against a brute-force restatement of the reference's
per-sphere test.  The grid must never lose the sphere the exhaustive sweep would hit: every test compares hits bit for bit."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_bvh_host import ref_flagged, _raw_scene

F = np.float32
U = 2.0 ** -24


def test_variant_constants_follow_the_header():
    assert (binding.VARIANT_GRID, binding.VARIANT_GRID_STATS) == (7, 8)
    hdr = open(binding.os.path.join(binding.HERE, "..", "include", "rays1.h")).read()
    assert "R1_VARIANT_GRID = 7" in hdr and "R1_VARIANT_GRID_STATS = 8" in hdr


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def offers(cx, cy, cz, rsq, o, d):
    """exact_offer (r1_hit_sweep.hpp, rayweek1.cpp:192-202, :294-313) vectorised over spheres: the t each sphere offers, inf for none."""
    cox, coy, coz = (cx - o[0]).astype(F), (cy - o[1]).astype(F), (cz - o[2]).astype(F)
    nb = _fma(coz, d[2], _fma(coy, d[1], (cox * d[0]).astype(F)))
    c = (_fma(coz, coz, _fma(coy, coy, (cox * cox).astype(F))) - rsq).astype(F)
    discr = ((nb * nb).astype(F) - c).astype(F)
    ok = ~np.signbit(discr)
    root = np.sqrt(np.where(ok, discr, 0).astype(F)).astype(F)
    t1 = (nb - root).astype(F)
    t = np.where(t1 > F(0.001), t1, (nb + root).astype(F)).astype(F)
    good = ok & (t > F(0.001)) & (t < F(np.finfo(F).max))
    return np.where(good, t, np.inf)


def brute(arrs, o, d):
    """Minimum offer over all hittable spheres, ties to the lowest index: (scene index or -1, t)."""
    act = active(arrs)
    t = offers(arrs["center_x"][act], arrs["center_y"][act], arrs["center_z"][act], arrs["radius_sq"][act], o, d)
    if not np.isfinite(t).any():
        return -1, None, t, act
    k = int(np.argmin(t))  # (argmin: the first of equal minima = the lowest index)
    return int(act[k]), float(t[k]), t, act


def active(arrs):
    fin = np.isfinite(arrs["center_x"]) & np.isfinite(arrs["center_y"]) & np.isfinite(arrs["center_z"]) & np.isfinite(arrs["radius_sq"])
    return np.nonzero((arrs["inv_radius"] != 0) & fin)[0]


def check_ray(cs, arrs, o, d, expect_fallback=None):
    o, d = np.asarray(o, F), np.asarray(d, F)
    shown, hit, t, fb = binding.grid_visit(cs, o, d)
    want, want_t, tall, act = brute(arrs, o, d)
    assert hit == want, (o, d, hit, want, fb)
    if want >= 0:
        assert F(t) == F(want_t)
    if expect_fallback is not None:
        assert fb == expect_fallback
    if not fb:
        # every sphere the reference flags with an offer <= the final t was presented
        stop = t if want >= 0 else np.inf
        must = set(act[np.isfinite(tall) & (tall <= stop)].tolist())
        assert must <= set(shown.tolist()), sorted(must - set(shown.tolist()))[:5]
    return fb


def cell_boxes(info):
    n = [int(x) for x in info["cells"]]
    lo, cell = info["lo"].astype(np.float64), info["cell"].astype(np.float64)
    jz, jy, jx = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    j = np.stack([jx.ravel(), jy.ravel(), jz.ravel()], 1)  # row q = cell (jz * ny + jy) * nx + jx
    return lo + j * cell, lo + (j + 1) * cell


def check_structure(cs, arrs):
    info, start, ids, outl = binding.grid_describe(cs)
    act = active(arrs)
    assert info["spheres"] == len(act)
    reg = set(ids.tolist())
    assert set(outl.tolist()) | reg == set(act.tolist())  # outliers + registered = every hittable sphere
    assert not (set(outl.tolist()) & reg)
    assert (np.diff(start.astype(np.int64)) >= 0).all() and start[-1] == len(ids) == info["registrations"]
    assert np.diff(start.astype(np.int64)).max(initial=0) == info["max_occupancy"]
    lo, hi = cell_boxes(info)
    c = np.stack([arrs["center_x"], arrs["center_y"], arrs["center_z"]], 1).astype(np.float64)
    rb = np.maximum(np.sqrt(np.maximum(arrs["radius_sq"].astype(np.float64), 0)), 1.0 / np.abs(np.where(arrs["inv_radius"] != 0, arrs["inv_radius"], np.inf)))
    for i in sorted(reg):
        q = np.clip(c[i], lo, hi) - c[i]
        overl = np.nonzero((q * q).sum(1) <= rb[i] ** 2)[0]  # every cell the sphere itself overlaps ...
        lists = set(np.nonzero([(ids[start[k]:start[k + 1]] == i).any() for k in overl])[0].tolist())
        assert len(lists) == len(overl), (i, len(lists), len(overl))
        # ... and the grid's box holds its registration ball
        assert (c[i] - rb[i] >= info["lo"] - 1e-6).all() and (c[i] + rb[i] <= info["hi"] + 1e-6).all()
    return info, start, ids, outl


SCENES = [("small", 0, 0), ("medium", 0, 0), ("large", 0, 0), ("grid", 400, 250)]


def make(kind, gw, gh):
    return {"small": r1.create_small_scene, "medium": r1.create_medium_scene, "large": r1.create_large_scene}[kind](320, 200) if kind != "grid" \
        else r1.create_grid_scene(320, 200, gw, gh)


@pytest.mark.parametrize("kind,gw,gh", SCENES)
def test_structure_on_the_reference_scenes(kind, gw, gh):
    sc = make(kind, gw, gh)
    arrs = sc.arrays()
    if kind == "grid":  # (100 004 spheres: the per-sphere check on a sample)
        info, start, ids, outl = binding.grid_describe(sc.spheres.contents)
        assert set(outl.tolist()) | set(ids.tolist()) == set(active(arrs).tolist())
    else:
        info, start, ids, outl = check_structure(sc.spheres.contents, arrs)
    if kind in ("large", "grid"):
        # the flat lattice of the reference (y in {0, 0.1}) is walked in 2-D; its outliers are the ground and the three big balls
        assert info["cells"][1] == 1
        assert info["outliers"] == 4
        big = np.sort(np.sqrt(arrs["radius_sq"][outl]))
        assert big[-1] == F(1000) and (big[:3] == F(2)).all()
    if kind == "large":
        assert (info["cells"][0], info["cells"][2]) == (30, 16) and info["max_occupancy"] == 1 and info["registrations"] == 480


def test_describe_filters_like_set_scene():
    rng = np.random.default_rng(5)
    c = rng.uniform(-4, 4, (40, 3))
    rad = rng.uniform(0.2, 0.6, 40)
    cs, arrs, mt = _raw_scene(c, rad)
    arrs["inv_radius"][3] = 0.0            # placeholder
    arrs["center_x"][7] = np.inf          # non-finite centre
    arrs["radius_sq"][11] = np.nan        # non-finite radius_sq
    info, start, ids, outl = check_structure(cs, arrs)
    seen = set(ids.tolist()) | set(outl.tolist())
    assert not ({3, 7, 11} & seen) and info["spheres"] == 37
    arrs["inv_radius"][5] = np.nan        # NaN inv_radius: an error, as r1_set_scene
    with pytest.raises(binding.R1Error):
        binding.grid_describe(cs)


def camera_rays(cam, n, rng):
    o = cam[0:3].astype(np.float64)
    s, t = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    d = cam[3:6][None] + s[:, None] * cam[6:9][None] + t[:, None] * cam[9:12][None] - o[None]
    d /= np.linalg.norm(d, axis=1)[:, None]
    return [(o, dd) for dd in d]


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


@pytest.mark.parametrize("kind,gw,gh", SCENES[:3] + [("grid", 60, 40)])
def test_visit_rule_against_brute_force(kind, gw, gh):
    rng = np.random.default_rng(11)
    sc = make(kind, gw, gh)
    arrs = sc.arrays()
    cs = sc.spheres.contents
    info, start, ids, outl = binding.grid_describe(cs)
    act = active(arrs)
    c = np.stack([arrs["center_x"], arrs["center_y"], arrs["center_z"]], 1)[act].astype(np.float64)
    r = np.sqrt(arrs["radius_sq"][act].astype(np.float64))
    rays = camera_rays(sc.camera_array(), 60, rng)
    for _ in range(60):  # bounce rays from sphere surfaces
        k = rng.integers(0, len(act))
        n = unit(rng.normal(size=3))
        rays.append((c[k] + n * r[k] * 1.0001, unit(n + rng.normal(size=3))))
    for _ in range(10):  # origins 300 units out, aimed back at the scene
        o = unit(rng.normal(size=3) * [1, 0.2, 1]) * 300 + [0, 5, 0]
        rays.append((o, unit(c[rng.integers(0, len(act))] - o)))
    for a in range(3):   # axis-parallel rays
        for sgn in (1, -1):
            d = np.zeros(3)
            d[a] = sgn
            rays.append((c[rng.integers(0, len(act))] - d * 7 + rng.normal(size=3) * 0.3, d))
    lo, cell, nc = info["lo"].astype(np.float64), info["cell"].astype(np.float64), info["cells"]
    for _ in range(20):  # through cell corners and along cell faces
        j = np.array([rng.integers(0, nc[a] + 1) for a in range(3)])
        p = lo + j * cell
        o = p + unit(rng.normal(size=3)) * 5
        rays.append((o, unit(p - o)))
        a = rng.integers(0, 3)
        d = unit(rng.normal(size=3))
        d[a] = 0
        o = p - 6 * unit(d)
        o[a] = F(p[a])
        rays.append((o, unit(d)))
    fb = 0
    for o, d in rays:
        fb += check_ray(cs, arrs, o.astype(F), d.astype(F))
    assert fb >= 1  # (the far origins)
    assert fb < len(rays) // 3  # (and the bounce rays that start on the ground far away: a minority)


def test_far_origins_take_the_fallback_and_v_safe_is_where_it_starts():
    sc = r1.create_large_scene(320, 200)
    arrs, cs = sc.arrays(), sc.spheres.contents
    info, start, ids, outl = binding.grid_describe(cs)
    clo, chi, v = info["centre_lo"].astype(np.float64), info["centre_hi"].astype(np.float64), float(info["v_safe"])
    rng = np.random.default_rng(3)
    act = active(arrs)
    for q in range(40):
        # origins whose farthest registered-centre box corner is at v_safe (1 -+ 1e-3): inside walk the grid, outside fall back
        dirn = unit(rng.normal(size=3) * [1, 0.3, 1] + [0, 0.4, 0])
        mid = 0.5 * (clo + chi)
        lo_s, hi_s = 0.0, 4 * v
        for _ in range(80):
            s = 0.5 * (lo_s + hi_s)
            o = mid + s * dirn
            dist = np.sqrt((np.maximum(np.abs(o - clo), np.abs(o - chi)) ** 2).sum())
            lo_s, hi_s = (s, hi_s) if dist < v else (lo_s, s)
        for f, want in ((0.999, False), (1.001, True)):
            o = (mid + lo_s * f * dirn).astype(F) if f < 1 else (mid + hi_s * f * dirn).astype(F)
            k = act[rng.integers(0, len(act))]
            tgt = np.array([arrs["center_x"][k], arrs["center_y"][k], arrs["center_z"][k]], np.float64)
            # graze the sphere: aim at its rim
            d = unit(tgt + unit(np.cross(tgt - o, [0, 1, 0])) * np.sqrt(arrs["radius_sq"][k]) * rng.choice([0.999, 1.0, 1.001]) - o)
            check_ray(cs, arrs, o, d.astype(F), expect_fallback=want)


@pytest.mark.parametrize("seed", range(8))
def test_random_scenes(seed):
    rng = np.random.default_rng(200 + seed)
    n = int(rng.integers(1, 400))
    c = rng.uniform(-10, 10, (n, 3)) * rng.choice([[1, 1, 1], [1, 0.01, 1]])
    rad = np.exp(rng.uniform(np.log(0.05), np.log(1.0), n))
    if seed % 3 == 0:
        rad[rng.integers(0, n)] = 50.0
    if seed % 4 == 1:
        c[n // 2:] = c[: n - n // 2]  # duplicates
    cs, arrs, mt = _raw_scene(c, rad)
    check_structure(cs, arrs)
    for q in range(80):
        o = rng.uniform(-14, 14, 3)
        k = rng.integers(0, n)
        tgt = c[k] + rng.normal(size=3) * rad[k] * rng.choice([0.0, 0.9, 1.0, 1.02])
        check_ray(cs, arrs, o.astype(F), unit(tgt - o).astype(F))


@pytest.mark.parametrize("family", ["degenerate_radii", "camera_inside_big_sphere", "far_cluster", "ties"])
def test_visit_rule_on_adversarial_families(family):
    rng = np.random.default_rng({"degenerate_radii": 81, "camera_inside_big_sphere": 82, "far_cluster": 83, "ties": 84}[family])
    n = 160
    if family == "degenerate_radii":
        c = rng.uniform(-3, 3, (n, 3))
        rad = np.exp(rng.uniform(np.log(1e-12), np.log(1e-6), n))
        origin = lambda: rng.uniform(-4, 4, 3)
    elif family == "camera_inside_big_sphere":
        c = rng.uniform(-20, 20, (n, 3))
        rad = rng.uniform(0.1, 1.5, n)
        c[0], rad[0] = (0.0, 0.0, 0.0), 50.0
        origin = lambda: rng.uniform(-20, 20, 3)
    elif family == "far_cluster":
        shift = np.array([3.0e4, -8.0e4, 1.2e4]) * rng.uniform(0.4, 1.2)
        c = rng.uniform(-6, 6, (n, 3)) + shift
        rad = np.exp(rng.uniform(np.log(0.02), np.log(1.0), n))
        origin = lambda: rng.uniform(-9, 9, 3) + shift
    else:  # coincident pairs: equal offers, the lower index must win
        base = rng.uniform(-5, 5, (n // 2, 3))
        c = np.repeat(base, 2, axis=0)
        rad = np.repeat(rng.uniform(0.2, 0.7, n // 2), 2)
        origin = lambda: rng.uniform(-8, 8, 3)
    cs, arrs, mt = _raw_scene(c, rad)
    cx, cy, cz, rsq = arrs["center_x"], arrs["center_y"], arrs["center_z"], arrs["radius_sq"]
    hits = 0
    for q in range(120):
        o = origin().astype(F)
        i = int(rng.integers(0, n))
        target = np.array([cx[i], cy[i], cz[i]], np.float64) + rng.normal(0, 1, 3) * rad[i] * rng.choice([0.0, 0.7, 1.0, 1.05])
        d = unit(target - o.astype(np.float64)).astype(F)
        hits += int(ref_flagged(cx, cy, cz, rsq, o, d).any())
        check_ray(cs, arrs, o, d)
        if family == "ties":
            shown, hit, t, fb = binding.grid_visit(cs, o, d)
            if hit >= 0:
                assert hit % 2 == 0  # of two coincident spheres, the first
    assert hits > 0


def test_pad_constants_against_a_monte_carlo_worst_case():
    """rho(|v|) = r_eff + (23 u |v|^2 + 2 u r^2) / (2 r_eff) + 5 u |v| (r1_grid.cpp): where the reference's fp32 test puts a hit point,
    measured on rays that graze spheres from far away — the worst case of the bound — must stay inside it."""
    rng = np.random.default_rng(9)
    worst = 0.0
    for q in range(4000):
        r = float(np.exp(rng.uniform(np.log(0.01), np.log(2.0))))
        vlen = float(rng.uniform(5, 400))
        c = rng.uniform(-50, 50, 3)
        o = (c + unit(rng.normal(size=3)) * vlen).astype(F)
        rim = unit(np.cross(c - o, rng.normal(size=3)))
        d = unit(c + rim * r * rng.uniform(0.99, 1.01) - o.astype(np.float64)).astype(F)
        cf = c.astype(F)
        t = offers(np.array([cf[0]]), np.array([cf[1]]), np.array([cf[2]]), np.array([F(r * r)]), o, d)[0]
        if not np.isfinite(t):
            continue
        p = o.astype(np.float64) + float(t) * d.astype(np.float64)
        dist = np.linalg.norm(p - cf.astype(np.float64))
        v = np.linalg.norm(cf.astype(np.float64) - o.astype(np.float64))
        r_t = np.sqrt(float(F(r * r)))
        bound = r_t + (23 * U * v * v + 2 * U * r_t * r_t) / (2 * r_t) + 5 * U * v
        worst = max(worst, (dist - r_t) / (bound - r_t))
    assert 0 < worst < 1.0, worst


# ---- preconditions of tests/test_gpu_grid_edges.py: each fixture still reaches the path its GPU test is about --------------------------


def _edges():
    import test_gpu_grid_edges as e  # (its GPU tests are marked gpu; the scene builders run anywhere)
    return e


def _cs(sa):
    from test_gpu_bvh import _as_cscene
    return _as_cscene(sa)


@pytest.mark.parametrize("kind", ["large", "lattice"])
def test_telephoto_rays_take_the_fallback_and_hit(kind):
    e = _edges()
    w, h = 96, 64
    sc = r1.create_large_scene(w, h) if kind == "large" else r1.create_grid_scene(w, h, 48, 36)
    sa = e.telephoto(r1o_scene(sc), w, h)
    cs, rng = _cs(sa), np.random.default_rng(21)
    hits = 0
    rays = camera_rays(sa.camera_array, 63, rng)
    for o, d in rays:
        check_ray(cs, sa.arrays, o.astype(F), d.astype(F), expect_fallback=True)
        hits += brute(sa.arrays, o.astype(F), d.astype(F))[0] >= 0
    assert hits > len(rays) // 2, hits


def test_straddling_lens_and_tie_scene_preconditions():
    e = _edges()
    w, h = 96, 64
    sa = e.straddling_lens(r1o_scene(r1.create_large_scene(w, h)), w, h)
    cam, cs = sa.camera_array, _cs(sa)
    d = unit(cam[3:6] + 0.5 * cam[6:9] + 0.5 * cam[9:12] - cam[0:3])
    near, far = cam[0:3] - cam[21] * 0.9 * cam[12:15], cam[0:3] + cam[21] * 0.9 * cam[12:15]
    flags = {check_ray(cs, sa.arrays, o.astype(F), d.astype(F)) for o in (near, far)}
    assert flags == {True, False}  # the lens crosses V: one rim walks the grid, the other takes the fallback
    sa, big = e.tie_scene(w, h)
    cs = _cs(sa)
    info, start, ids, outl = binding.grid_describe(cs)
    assert outl.tolist() == [big] and set(ids.tolist()) == set(range(big))
    hit_groups, hit_outlier = 0, 0
    for o, d in camera_rays(sa.camera_array, 120, np.random.default_rng(22)):
        check_ray(cs, sa.arrays, o.astype(F), d.astype(F), expect_fallback=True)
        hit = brute(sa.arrays, o.astype(F), d.astype(F))[0]
        hit_groups += 0 <= hit < big
        hit_outlier += hit == big
        assert hit < 0 or hit == big or hit % 4 == 0  # of four coincident spheres, the first
    assert hit_groups >= 10 and hit_outlier >= 5, (hit_groups, hit_outlier)


def test_limit_scenes_sit_at_the_lds_limit():
    e = _edges()
    for kind in e.LIMIT_SCENES:
        sa = e.limit_scene(kind, 80, 60)
        cs = _cs(sa)
        info = binding.grid_describe(cs)[0]
        hv = e.halves(cs)
        assert info["spheres"] <= 1023 and info["registrations"] > 4096, kind
        assert (8000 <= hv <= binding_lds_halves()) if kind != "over" else (binding_lds_halves() < hv <= 8400), (kind, hv)
        if kind == "deep":
            assert binding.bvh_describe(cs)[0]["depth"] >= 15
        for o_, d in camera_rays(sa.camera_array, 6, np.random.default_rng(23)):
            check_ray(cs, sa.arrays, o_.astype(F), d.astype(F), expect_fallback=False)


def binding_lds_halves():
    import re
    src = open(binding.os.path.join(binding.HERE, "csrc", "r1_grid.h")).read()
    return int(re.search(r"#define R1_GRID_LDS_HALVES (\d+)", src).group(1))


def test_outlier_and_cell_shapes():
    e = _edges()
    rng = np.random.default_rng(24)
    for shape in e.SHAPES:
        sa, want = e.shape_scene(shape, 72, 48)
        cs = _cs(sa)
        info = e.check_shape(cs, want)
        check_structure(cs, sa.arrays)
        hits = 0
        for o, d in camera_rays(sa.camera_array, 40, rng):
            check_ray(cs, sa.arrays, o.astype(F), d.astype(F))
            hits += brute(sa.arrays, o.astype(F), d.astype(F))[0] >= 0
        assert hits >= 4, (shape, hits)
        if shape == "all_outliers":
            assert float(info["v_safe"]) >= 16 and info["max_occupancy"] == 0


def test_boundary_plane_rays_against_brute_force():
    e = _edges()
    sa, x = e.boundary_plane_scene(64, 48)
    cs = _cs(sa)
    info = binding.grid_describe(cs)[0]
    k = (np.float64(x) - np.float64(info["lo"][0])) / np.float64(info["cell"][0])
    assert k == int(k) and 0 < k < info["cells"][0]  # exactly on an inner boundary
    cam = sa.camera_array
    hits = 0
    for o, d in camera_rays(cam, 80, np.random.default_rng(25)):
        o, d = o.astype(F), d.astype(F)
        assert o[0] == x and d[0] == 0
        assert not check_ray(cs, sa.arrays, o, d)
        hits += brute(sa.arrays, o, d)[0] >= 0
    assert hits > 20, hits


def r1o_scene(sc):
    import r1o
    return r1o.SceneArrays.from_c(sc.spheres, sc.camera)
