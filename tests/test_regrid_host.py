"""CPU tests of the regrid: r1_grid_regrid_describe, the host restatement of r1_regrid through the device's own functions
(csrc/r1_grid_fill.h).  The rule is "geometry kept": the plan of the grid built for the arrays of r1_set_scene stays, and every sphere is
an outlier or registered in the cells its ball overlaps.  Checked here: the scene's own arrays reproduce the builder byte for byte; under
every move the tables keep what the exactness argument of r1_grid.cpp needs (balls inside the box, the box inside [-M, M], the far test's
box = the registered centres'); a NumPy restatement of the per-sphere rule reproduces the lists; the walk of the regridded tables presents
every sphere whose offer matters; overflow, non-finite centres and the edge scenes."""
import os
import re

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_bvh_host import F, _raw_scene
from test_grid_host import active, brute, camera_rays, unit
from test_refit_host import MOVES, edge_scene, lattice_of, make_scene, moved_centres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("small", "medium", "large", "grid40x30", "grid160x100")
SPAN_MAX, SLACK = 64, 2  # R1_GRID_SPAN_MAX (r1_grid.h), R1_REGRID_SLACK (r1_grid_fill.h)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def scenes():
    """name -> (Scene, arrays, grid_describe, grid_plan): built once, never changed."""
    out = {}
    for name in SCENES:
        sc = make_scene(name)
        out[name] = (sc, sc.arrays(), binding.grid_describe(sc.spheres.contents), binding.grid_plan(sc.spheres.contents))
    return out


def capacity(built):
    return SLACK * built[0]["registrations"] + 64


def tables_equal(got, want, what):
    for k in want[0]:
        if k != "build_ms":
            assert np.array_equal(np.asarray(got[0][k]), np.asarray(want[0][k])), (what, k, got[0][k], want[0][k])
    for n, g, w in zip(("start", "ids", "outliers"), got[1:], want[1:]):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, n)


def test_the_names_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rays1.h")).read(), flags=re.S)
    bound = {s[0] for s in binding.SYMBOLS}
    for name in ("r1_regrid", "r1_grid_download", "r1_grid_regrid_describe"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(binding.lib(), name) and name in bound, name
    assert callable(r1.Renderer.regrid) and callable(r1.Renderer.grid_download) and callable(binding.regrid_describe)
    assert binding.lib().r1_regrid(None, None) == binding.R1_EINVAL
    assert binding.lib().r1_grid_download(None, None, None, 0, None, 0, None, 0) == binding.R1_EINVAL
    assert binding.lib().r1_abi_version() == 4


@pytest.mark.parametrize("name", SCENES)
def test_the_scenes_own_arrays_reproduce_the_builder_byte_for_byte(scenes, name):
    sc, a, built, plan = scenes[name]
    got = binding.regrid_describe(sc.spheres.contents, a["center_x"], a["center_y"], a["center_z"])
    tables_equal(got, built, name)
    # ... with the radii given as well, and a regrid is a function of its inputs alone
    again = binding.regrid_describe(sc.spheres.contents, a["center_x"], a["center_y"], a["center_z"], a["radius_sq"], a["inv_radius"])
    tables_equal(again, built, (name, "radii given"))


# ---- the per-sphere rule in NumPy, from its sets alone ---------------------------------------------------------------------------------------


def rho_of(c, rt, plan):
    """r1gf_rho: r1_grid.cpp:105-107, :151, :165 with the plan's V and delta, operation for operation in fp64."""
    V, delta = plan["V"], plan["delta"]
    r_floor = 1e-4 * (1.0 + np.abs(c[:, 0]) + np.abs(c[:, 1]) + np.abs(c[:, 2]))
    reff = np.maximum(rt, r_floor)
    rho0 = reff + (23.0 * U * V * V + 2.0 * U * rt * rt) / (2.0 * reff) + 5.0 * U * V
    return (rho0 + delta) * (1.0 + 2.0 ** -40)


def radii_rows(rsq, inv):
    """{bound, test} as r1f_radius_rows writes them for a hittable pair."""
    rsq, inv = rsq.astype(np.float64), inv.astype(np.float64)
    from_sq = np.where(rsq > 0, np.sqrt(np.maximum(rsq, 0)), 0.0)
    with np.errstate(divide="ignore"):
        from_inv = np.where(np.isfinite(inv) & (inv != 0), 1.0 / np.abs(inv), 0.0)
    rb = np.maximum(from_sq, from_inv)
    return rb, np.where(rsq > 0, np.minimum(rb, from_sq), 0.0)


def restate(built, plan, act, x, y, z, rsq, inv):
    """The rule of DESIGN.md §4.31 for the active spheres `act` (scene indices, ascending): (outliers, per-cell id lists, candidates, rho),
    from sets alone — every cell against every ball, no tables."""
    info = built[0]
    c = np.stack([x[act], y[act], z[act]], 1).astype(np.float64)
    rb, rt = radii_rows(rsq[act], inv[act])
    finite = np.isfinite(c).all(1)
    cz = np.where(finite[:, None], c, 0.0)
    rho = rho_of(cz, rt, plan)
    lo, cell, n = info["lo"].astype(np.float64), info["cell"].astype(np.float64), info["cells"]
    flat = plan["flat"]
    blo = np.where(flat, -plan["M"], lo)
    bhi = np.where(flat, plan["M"], lo + n * cell)
    inside = ((cz - rho[:, None] >= blo) & (cz + rho[:, None] <= bhi)).all(1)
    cand = finite & ~(rb > plan["big"]) & inside
    # the cells' boxes on the non-flat axes (a flat axis: one cell that holds every candidate, distance 0)
    jz, jy, jx = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    j = np.stack([jx.ravel(), jy.ravel(), jz.ravel()], 1)
    b0, b1 = lo + j * cell, lo + (j + 1) * cell
    lists = [[] for _ in range(len(j))]
    outl = []
    for k in range(len(act)):
        if not finite[k]:
            continue
        if not cand[k]:
            outl.append(int(act[k]))
            continue
        q = np.where(cz[k] < b0, b0 - cz[k], np.where(cz[k] > b1, cz[k] - b1, 0.0))
        q[:, flat] = 0.0
        cells = np.nonzero((q * q).sum(1) <= rho[k] * rho[k] * (1.0 + 1e-12))[0]
        if len(cells) > SPAN_MAX:
            outl.append(int(act[k]))
        else:
            for q_ in cells:
                lists[q_].append(int(act[k]))
    return outl, lists, cand, rho


RADII = (0.5, 2.0)
CASES = [(name, move) for name in ("small", "medium", "large", "grid40x30") for move in MOVES + tuple("radii x %g" % f for f in RADII)]


def moved_arrays(a, move):
    """(x, y, z, radius_sq, inv_radius) scene-indexed, for a move of MOVES or "radii x <factor>"."""
    if move.startswith("radii x "):
        f = F(float(move[8:]))
        return a["center_x"], a["center_y"], a["center_z"], (a["radius_sq"] * f * f).astype(F), (a["inv_radius"] / f).astype(F)
    return moved_centres(a, move) + (a["radius_sq"], a["inv_radius"])


@pytest.mark.parametrize("name,move", CASES)
def test_moved_tables_keep_what_exactness_needs_and_equal_the_numpy_rule(scenes, name, move):
    sc, a, built, plan = scenes[name]
    x, y, z, rsq, inv = moved_arrays(a, move)
    info, start, ids, outl = binding.regrid_describe(sc.spheres.contents, x, y, z, rsq, inv)
    act = np.nonzero(a["inv_radius"] != 0)[0]
    want_out, want_lists, cand, rho = restate(built, plan, act, x, y, z, rsq, inv)
    assert outl.tolist() == want_out, (name, move, "outliers")              # ascending, as the rule gives them
    assert info["outliers"] == len(outl) and info["spheres"] == len(act)
    total = sum(len(q) for q in want_lists)
    if total > capacity(built):
        assert info["registrations"] == -1 and not start.any() and len(ids) == 0
        return
    assert info["registrations"] == total == len(ids) == start[-1]
    for q, want in enumerate(want_lists):                                   # ascending ids in every cell
        assert ids[start[q]:start[q + 1]].tolist() == want, (name, move, "cell", q)
    reg = set(ids.tolist())
    # every live finite sphere is in exactly one of the two lists
    assert not (reg & set(outl.tolist())) and reg | set(outl.tolist()) == set(act.tolist())
    # the geometry: the plan's on the non-flat axes; the box holds every registered ball and lies inside [-M, M]
    flat = plan["flat"]
    assert np.array_equal(info["cells"], built[0]["cells"])
    assert np.array_equal(info["lo"][~flat], built[0]["lo"][~flat]) and np.array_equal(info["cell"][~flat], built[0]["cell"][~flat])
    lo = info["lo"].astype(np.float64)
    hi = lo + info["cells"] * info["cell"].astype(np.float64)
    assert (np.abs(lo) <= plan["M"] * (1 + 2.0 ** -22)).all() and (np.abs(hi) <= plan["M"] * (1 + 2.0 ** -22)).all()
    pos = {int(s): k for k, s in enumerate(act)}
    c = np.stack([x, y, z], 1).astype(np.float64)
    for i in reg:
        assert (c[i] - rho[pos[i]] >= lo).all() and (c[i] + rho[pos[i]] <= hi).all(), (name, move, i)
    # the far test's box is the registered centres'
    if reg:
        r = sorted(reg)
        assert np.array_equal(info["centre_lo"], c[r].min(0).astype(F)) and np.array_equal(info["centre_hi"], c[r].max(0).astype(F))
    else:
        assert not info["centre_lo"].any() and not info["centre_hi"].any()
    if move == "lift" and name != "medium":
        # the flat axis's one cell is re-stretched over the lifted spheres: the lattice stays registered
        assert flat[1] and info["outliers"] == built[0]["outliers"] and info["cell"][1] > built[0]["cell"][1]
    if move == "far":
        moved = np.nonzero(x != a["center_x"])[0]
        assert len(moved) == 1 and set(moved.tolist()) <= set(outl.tolist())


def test_lift_on_grid160x100_keeps_the_lattice_registered(scenes):
    sc, a, built, plan = scenes["grid160x100"]
    x, y, z = moved_centres(a, "lift")
    info, start, ids, outl = binding.regrid_describe(sc.spheres.contents, x, y, z)
    assert info["outliers"] == built[0]["outliers"] == 4 and info["registrations"] == built[0]["registrations"] == 16000
    assert np.array_equal(outl, built[3]) and np.array_equal(np.diff(start.astype(np.int64)), np.diff(built[1].astype(np.int64)))


# ---- the walk of the regridded tables ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("move", ("jitter", "lift", "far", "coincident", "radii x 0.5", "radii x 2"))
@pytest.mark.parametrize("name", ("small", "medium", "large"))
def test_the_walk_presents_every_sphere_whose_offer_matters(scenes, name, move):
    """test_grid_host.py's check_ray over the regridded tables (r1_grid_regrid_visit: r1_grid_dda.h's arithmetic, the kernel's stopping
    rule): camera, bounce, axis-parallel and cell-face rays against the brute-force minimum over the moved spheres."""
    sc, a, built, plan = scenes[name]
    cs = sc.spheres.contents
    x, y, z, rsq, inv = moved_arrays(a, move)
    arrs = dict(a)
    arrs.update(center_x=x, center_y=y, center_z=z, radius_sq=rsq, inv_radius=inv)
    info = binding.regrid_describe(cs, x, y, z, rsq, inv)[0]
    rng = np.random.default_rng(23)
    act = active(arrs)
    c = np.stack([x, y, z], 1)[act].astype(np.float64)
    r = np.sqrt(rsq[act].astype(np.float64))
    rays = camera_rays(sc.camera_array(), 40, rng)
    for _ in range(40):  # bounce rays from sphere surfaces
        k = rng.integers(0, len(act))
        n = unit(rng.normal(size=3))
        rays.append((c[k] + n * r[k] * 1.0001, unit(n + rng.normal(size=3))))
    for ax in range(3):  # axis-parallel rays
        for sgn in (1, -1):
            d = np.zeros(3)
            d[ax] = sgn
            rays.append((c[rng.integers(0, len(act))] - d * 7 + rng.normal(size=3) * 0.3, d))
    lo, cell, nc = info["lo"].astype(np.float64), info["cell"].astype(np.float64), info["cells"]
    for _ in range(12):  # through cell corners and along cell faces
        j = np.array([rng.integers(0, nc[ax] + 1) for ax in range(3)])
        p = lo + j * cell
        o = p + unit(rng.normal(size=3)) * 5
        rays.append((o, unit(p - o)))
        ax = rng.integers(0, 3)
        d = unit(rng.normal(size=3))
        d[ax] = 0
        o = p - 6 * unit(d)
        o[ax] = F(p[ax])
        rays.append((o, unit(d)))
    walked = 0
    for o, d in rays:
        o, d = o.astype(F), d.astype(F)
        shown, hit, t, fb = binding.regrid_visit(cs, x, y, z, o, d, rsq, inv)
        want, want_t, tall, act_ = brute(arrs, o, d)
        assert hit == want, (name, move, o, d, hit, want, fb)
        if want >= 0:
            assert F(t) == F(want_t)
        if not fb:
            walked += 1
            stop = t if want >= 0 else np.inf
            must = set(act_[np.isfinite(tall) & (tall <= stop)].tolist())
            assert must <= set(shown.tolist()), (name, move, sorted(must - set(shown.tolist()))[:5])
    if info["registrations"] == -1:  # (large under radii x 2 overflows: 2 x 480 + 64 entries; every ray the fallback, still exact)
        assert (name, move) == ("large", "radii x 2") and walked == 0
    else:
        assert walked > len(rays) // 2, (name, move, walked)  # (the grid was walked, not only the fallback)


# ---- overflow ----------------------------------------------------------------------------------------------------------------------------------------


def test_overflow_on_grid40x30(scenes):
    """Radii x 3 on grid 40 x 30 exceed the capacity (2 x 1200 + 64 = 2464).  So do x 2 and x 1.25 on this scene: its cells are the lattice's
    pitch (0.825) and its balls of radius 0.2 fill a quarter of one, so a ball a quarter larger already reaches its four neighbours and
    the 140 spheres of the rim leave the box.  The factors that separate are 1.1 (the build's 1200 registrations) and 1.25."""
    sc, a, built, plan = scenes["grid40x30"]
    cs = sc.spheres.contents
    assert built[0]["registrations"] == 1200 and capacity(built) == 2464
    for f, over in ((1.1, False), (1.25, True), (2.0, True), (3.0, True)):
        x, y, z, rsq, inv = moved_arrays(a, "radii x %g" % f)
        info, start, ids, outl = binding.regrid_describe(cs, x, y, z, rsq, inv)
        assert (info["registrations"] == -1) == over, (f, info["registrations"])
        if over:
            assert not start.any() and len(start) == 1201 and len(ids) == 0
            # v2 = -1: every origin is far, every ray takes the tree fallback
            o = np.array([0.0, 1.0, 0.0], F)
            shown, hit, t, fb = binding.regrid_visit(cs, x, y, z, o, unit([0.1, -1, 0.2]).astype(F), rsq, inv)
            assert fb and sorted(shown.tolist()) == sorted(outl.tolist())
        else:
            assert info["registrations"] == 1200


# ---- edge inputs -----------------------------------------------------------------------------------------------------------------------------------


def test_non_finite_centres_are_in_neither_list(scenes):
    sc, a, built, plan = scenes["large"]
    cs = sc.spheres.contents
    lat = lattice_of(a)
    x, y, z = (a[k].copy() for k in ("center_x", "center_y", "center_z"))
    x[lat[3]] = np.nan
    y[lat[7]] = np.inf
    info, start, ids, outl = binding.regrid_describe(cs, x, y, z)
    seen = set(ids.tolist()) | set(outl.tolist())
    assert not ({int(lat[3]), int(lat[7])} & seen) and len(seen) == info["spheres"] - 2
    assert info["registrations"] == built[0]["registrations"] - 2 and info["outliers"] == built[0]["outliers"]
    assert np.isfinite(info["lo"]).all() and np.isfinite(info["cell"]).all() and np.isfinite(info["centre_lo"]).all()
    # the ground's centre NaN: an outlier less
    x, y, z = (a[k].copy() for k in ("center_x", "center_y", "center_z"))
    z[int(built[3][0])] = np.nan
    info, start, ids, outl = binding.regrid_describe(cs, x, y, z)
    assert outl.tolist() == built[3][1:].tolist() and np.array_equal(ids, built[2])


@pytest.mark.parametrize("n_active", [0, 1, 4, 5])
def test_edge_scenes(n_active):
    cs, arrs, mt = edge_scene(n_active)
    built = binding.grid_describe(cs)
    tables_equal(binding.regrid_describe(cs, arrs["center_x"], arrs["center_y"], arrs["center_z"]), built, n_active)
    rng = np.random.default_rng(40 + n_active)
    x, y, z = ((arrs[k] + rng.uniform(-0.5, 0.5, cs.count)).astype(F) for k in ("center_x", "center_y", "center_z"))
    info, start, ids, outl = binding.regrid_describe(cs, x, y, z)
    act = np.nonzero(arrs["inv_radius"] != 0)[0]
    assert info["spheres"] == n_active and set(ids.tolist()) | set(outl.tolist()) == set(act.tolist())
    assert not (set(ids.tolist()) & set(outl.tolist())) and len(start) == len(built[1])
    if n_active == 0:
        assert info["registrations"] == 0 and info["outliers"] == 0


def test_a_scene_that_is_all_outliers():
    """Every sphere thrown out of the plan's box: no registrations, v2 = inf as the builder leaves a grid without any (no ray is far), a
    zero far box, and every sphere in the outlier list in ascending order."""
    rng = np.random.default_rng(9)
    cs, arrs, mt = _raw_scene(rng.uniform(-3, 3, (30, 3)), rng.uniform(0.2, 0.4, 30))
    built = binding.grid_describe(cs)
    assert built[0]["registrations"] > 0
    x = (arrs["center_x"] + F(500)).astype(F)
    info, start, ids, outl = binding.regrid_describe(cs, x, arrs["center_y"], arrs["center_z"])
    assert info["registrations"] == 0 and not start.any() and outl.tolist() == list(range(30))
    assert not info["centre_lo"].any() and not info["centre_hi"].any()
    assert np.array_equal(info["lo"], built[0]["lo"]) and np.array_equal(info["cell"], built[0]["cell"])
    shown, hit, t, fb = binding.regrid_visit(cs, x, arrs["center_y"], arrs["center_z"], np.array([500, 0, 9], F), np.array([0, 0, -1], F))
    assert not fb and shown.tolist() == list(range(30))
    arrs2 = dict(arrs)
    arrs2["center_x"] = x
    assert hit == brute(arrs2, np.array([500, 0, 9], F), np.array([0, 0, -1], F))[0]


def test_null_pointers_and_partial_radii_are_refused(scenes):
    sc, a, built, plan = scenes["small"]
    cs = sc.spheres.contents
    with pytest.raises(binding.R1Error):
        binding.regrid_describe(cs, a["center_x"], a["center_y"], a["center_z"], a["radius_sq"], None)
    with pytest.raises(binding.R1Error):
        binding.regrid_describe(cs, a["center_x"][:-1], a["center_y"], a["center_z"])
    info = binding.GridInfo()
    assert binding.lib().r1_grid_regrid_describe(None, None, None, None, None, None, info, None, 0, None, 0, None, 0) == binding.R1_EINVAL


# ---- the stand-alone program ---------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    """tools/check_regrid_host.cpp built with r1_grid.cpp and r1_bvh.cpp, the host sources it drives (no sanitizer here: DESIGN.md §4.31
    has that run)."""
    import subprocess
    out = str(tmp_path_factory.mktemp("regrid_host") / "check_regrid_host")
    src = [os.path.join(ROOT, "tools", "check_regrid_host.cpp")] + [os.path.join(ROOT, "rays1bench_amd", "csrc", f) for f in ("r1_grid.cpp", "r1_bvh.cpp")]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-o", out])
    return out


@pytest.mark.parametrize("what,says", [("outliers", "every sphere an outlier"), ("touch", "ball on the box face"), ("zeros", "signed zeros: the same tables"),
                                       ("twice", "regrid of a regridded state: unchanged")])
def test_stand_alone_program_on_inputs_no_scene_reaches(check_program, what, says):
    import subprocess
    out = subprocess.run([check_program, what], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert says in out.stdout
