"""CPU tests of the flat axis of a box tree (r1_bvh.cpp "flat axis", r1_hit_tree.hpp bvh_advance: visit_flat; no GPU).

The builder names at most one axis along which the union of the slabs of every box the node loop tests is at most 1.25 x the
narrowest of them, and reports the union as (flat_m, flat_e) rounded outward; the small-scene tree kernels then test that ONE slab
once per call (N = max(a_u - b_u, 0), F = min(a_u + b_u, best)) and two axes per child box.  Checked here: the decision on the
reference's scenes and on synthetic lattices on either side of the ratio; that the slab contains what it stands for; the box of the
root step (a K of its own for each child); and a numpy restatement of the flat walk, fp32 step by step, against brute force — every
sphere the reference's test flags is presented, and with pruning the walk returns the minimum offer with ties to the lowest index."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

from test_bvh_host import E, EMPTY, LEAF, M, REF, _raw_scene, leaf_slots, ref_flagged

F = np.float32
FLT_MAX = np.finfo(np.float32).max
RATIO = 1.25  # R1_BVH_FLAT_RATIO of the shipped build (r1_bvh.cpp)


def loop_boxes(info, nodes, axis):
    """(lo, hi) in float64 of every child box the node loop tests: the children of every inner node but a root of the root-step shape."""
    out = []
    for n in range(1 if info["root_leaf"] else 0, len(nodes)):
        for c in (0, 1):
            m, e = float(nodes[n][M[c][axis]]), float(nodes[n][E[c][axis]])
            if e >= 0:  # (-inf: a child that never passes)
                out.append((m - e, m + e))
    return out


def rule(info, nodes):
    """The builder's rule restated: (axis or -1, {axis: ratio})."""
    ratios = {}
    for a in (1, 0, 2):  # equal ratios: y, then x, then z
        b = loop_boxes(info, nodes, a)
        narrow = min(hi - lo for lo, hi in b)
        ratios[a] = (max(hi for _, hi in b) - min(lo for lo, _ in b)) / narrow if narrow > 0 else np.inf
    ok = [a for a in (1, 0, 2) if ratios[a] <= RATIO]
    return (min(ok, key=lambda a: ratios[a]) if ok else -1), ratios


def check_slab(info, nodes):
    a = info["flat_axis"]
    lo, hi = float(info["flat_m"]) - float(info["flat_e"]), float(info["flat_m"]) + float(info["flat_e"])
    for blo, bhi in loop_boxes(info, nodes, a):
        assert lo <= blo and bhi <= hi, (lo, hi, blo, bhi)
    return lo, hi


# ---- the decision ---------------------------------------------------------------------------------------------------------------------


def test_large_scene_is_flat_along_y_and_the_slab_contains_every_box_of_the_loop():
    sc = r1.create_large_scene(1200, 800)
    info, nodes, ids = binding.bvh_describe(sc.spheres.contents)
    assert info["flat_axis"] == 1 and info["root_leaf"] != 0 and info["pad_local"] == 0, info
    lo, hi = check_slab(info, nodes)
    # every box of nodes >= 1, both children, explicitly (the issue's wording)
    for n in range(1, len(nodes)):
        for c in (0, 1):
            m, e = float(nodes[n][M[c][1]]), float(nodes[n][E[c][1]])
            assert lo <= m - e and m + e <= hi, (n, c)
    # the lattice: r = 0.45 spheres on y = 0, one in twenty raised by 0.1 — the slab is about 1.01 high, 1.12 x the narrowest box
    assert 0.95 < hi - lo < 1.06, (lo, hi)
    axis, ratios = rule(info, nodes)
    assert axis == 1 and 1.0 < ratios[1] < 1.2 and ratios[0] > 5 and ratios[2] > 5, ratios


@pytest.mark.parametrize("kind", ["medium", "small", "grid400x250"])
def test_scenes_that_are_not_flat(kind):
    sc = {"medium": lambda: r1.create_medium_scene(1200, 800), "small": lambda: r1.create_small_scene(1200, 800),
          "grid400x250": lambda: r1.create_grid_scene(1920, 1080, 400, 250)}[kind]()
    info, nodes, ids = binding.bvh_describe(sc.spheres.contents)
    assert info["flat_axis"] == -1 and info["flat_m"] == 0 and info["flat_e"] == 0, info
    if kind == "medium":  # by its boxes: spheres at y = 0, 1 and 1.5 (the 100 004-sphere lattice is out by its pad and its size, the small
        assert info["pad_local"] == 0 and 2 <= len(nodes) <= 256  # scene by its tree of one node: no walk to shorten)
        assert rule(info, nodes)[0] == -1 and rule(info, nodes)[1][1] > 2.0, rule(info, nodes)
    if kind == "small":
        assert len(nodes) == 1


def lattice(nx, nz, raise_by, up=1, ground=True, seed=3):
    """nx x nz spheres of r = 0.45 on a plane, one in five raised by `raise_by` along `up`; optionally the reference's ground sphere."""
    rng = np.random.default_rng(seed)
    gx, gz = np.meshgrid(np.arange(nx) - nx / 2, np.arange(nz) - nz / 2, indexing="ij")
    n = nx * nz
    c = np.zeros((n, 3))
    plane = [a for a in range(3) if a != up]
    c[:, plane[0]] = gx.ravel() * 1.1 + rng.uniform(-0.05, 0.05, n)
    c[:, plane[1]] = gz.ravel() * 1.1 + rng.uniform(-0.05, 0.05, n)
    c[:, up] = np.where(np.arange(n) % 5 == 0, raise_by, 0.0)
    rad = np.full(n, 0.45)
    if ground:
        g = np.zeros(3)
        g[up] = -1000.45
        c, rad = np.concatenate([c, g[None]]), np.concatenate([rad, [1000.0]])
    return c, rad


@pytest.mark.parametrize("up", [1, 0, 2])
@pytest.mark.parametrize("ground", [True, False])
@pytest.mark.parametrize("raise_by,flat", [(0.0, True), (0.1, True), (0.17, True), (0.3, False), (0.5, False), (1.0, False)])
def test_synthetic_lattices_decide_as_the_rule_says(raise_by, flat, ground, up):
    """Heights on either side of the ratio: the boxes are 0.9 + pad high, so a rise of 0.17 gives ~1.19 and one of 0.3 ~1.33.  With the
    ground sphere the root has the root-step shape (its boxes are not the loop's); without, node 0's boxes count.  The same lattice
    standing on x or z is reported along that axis (the kernels act on y only)."""
    c, rad = lattice(16, 12, raise_by, up, ground)
    cs, arrs, mt = _raw_scene(c, rad)
    info, nodes, ids = binding.bvh_describe(cs)
    assert (info["root_leaf"] != 0) == ground
    axis, ratios = rule(info, nodes)
    assert abs(ratios[up] - RATIO) > 1e-3, ratios  # the cases are not at the threshold, where the restatement's rounding would decide
    assert axis == (up if flat else -1), (ratios, info)
    assert info["flat_axis"] == axis, (info, ratios)
    if flat:
        check_slab(info, nodes)
        lo, hi = float(info["flat_m"]) - float(info["flat_e"]), float(info["flat_m"]) + float(info["flat_e"])
        b = loop_boxes(info, nodes, up)
        # rounded outward, and by no more than a few ulps
        assert min(x for x, _ in b) - lo < 1e-5 and hi - max(x for _, x in b) < 1e-5
    else:
        assert info["flat_m"] == 0 and info["flat_e"] == 0


def test_too_many_spheres_or_nodes_for_the_lds_walks_are_never_flat():
    c, rad = lattice(40, 30, 0.0)  # 1201 spheres: beyond the 10-bit indices of the small-scene kernels
    cs, arrs, mt = _raw_scene(c, rad)
    info, nodes, ids = binding.bvh_describe(cs)
    assert info["spheres"] == 1201 and info["flat_axis"] == -1


def test_the_root_steps_box_is_the_lattice():
    """A K of its own for each child (r1_bvh.cpp fill): the sibling of the ground sphere's leaf no longer carries the ground's
    K = 2 w2 1000^2.  Node 0's inner-child box is within 0.1 of the lattice's extent on every axis."""
    sc = r1.create_large_scene(1200, 800)
    a = sc.arrays()
    info, nodes, ids = binding.bvh_describe(sc.spheres.contents)
    k = 1 if info["root_leaf"] == 1 else 0  # the inner child
    root = nodes[0].view(np.uint32)
    assert not root[REF[k]] & LEAF and root[REF[1 - k]] & LEAF
    outliers = set(ids[list(leaf_slots(int(root[REF[1 - k]])))].tolist()) - {EMPTY}
    active = [i for i in np.nonzero(a["inv_radius"] != 0)[0].tolist() if i not in outliers]
    cc = np.stack([a["center_x"], a["center_y"], a["center_z"]], 1).astype(np.float64)[active]
    rr = np.sqrt(a["radius_sq"].astype(np.float64))[active]
    lo, hi = (cc - rr[:, None]).min(0), (cc + rr[:, None]).max(0)
    m, e = nodes[0][list(M[k])].astype(np.float64), nodes[0][list(E[k])].astype(np.float64)
    assert ((m - e <= lo) & (lo - (m - e) < 0.1)).all(), (m - e, lo)
    assert ((m + e >= hi) & ((m + e) - hi < 0.1)).all(), (m + e, hi)


# ---- the flat walk, restated ----------------------------------------------------------------------------------------------------------


def fma(a, b, c):  # exactly rounded fp32 fma (the product of two fp32 is exact in fp64; inf / NaN propagate alike)
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def offers(cx, cy, cz, rsq, o, d):
    """What the reference's test offers for every sphere (leaf_quad / exact_offer): t in fp32, +inf for none."""
    cox, coy, coz = (cx - o[0]).astype(F), (cy - o[1]).astype(F), (cz - o[2]).astype(F)
    nb = fma(coz, np.full_like(coz, d[2]), fma(coy, np.full_like(coy, d[1]), (cox * d[0]).astype(F)))
    cc = (fma(coz, coz, fma(coy, coy, (cox * cox).astype(F))) - rsq).astype(F)
    discr = ((nb * nb).astype(F) - cc).astype(F)
    ok = ~np.signbit(discr)
    root = np.sqrt(np.where(ok, discr, 0).astype(F)).astype(F)
    t1 = (nb - root).astype(F)
    t = np.where(t1 > F(0.001), t1, (nb + root).astype(F)).astype(F)
    return np.where(ok & (t > F(0.001)) & (t < FLT_MAX), t, F(np.inf)).astype(F)


def flat_walk(info, nodes, ids, o, d, jitter, sphere_t=None):
    """bvh_advance<LN> on a flat tree, fp32 step by step: the root step (the leaf every ray tests, then node 0's other box with all
    three axes AND N <= F), the node loop with N / F and two axes per box, nearer child first.  sphere_t None: no distance pruning
    (best stays FLT_MAX) — returns the leaf slots the ray is shown.  sphere_t (offers per scene index): the pruned walk — returns
    (slots shown, best, best_id)."""
    assert info["flat_axis"] == 1 and not info["pad_local"]
    o = o.astype(F)
    best, best_id = F(FLT_MAX), EMPTY
    shown = []

    def leaf(ref):
        nonlocal best, best_id
        for s in leaf_slots(ref):
            shown.append(s)
            i = int(ids[s])
            if sphere_t is not None and i != EMPTY:
                t = sphere_t[i]
                if t < best or (t == best and i < best_id):
                    best, best_id = t, i

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F(1) / d.astype(F)).astype(F)
        inv = np.where(np.isfinite(inv), np.nextafter(inv, np.where(jitter > 0, F(np.inf), F(-np.inf)).astype(F)), inv).astype(F)
        ainv = np.abs(inv)
        oi = (o * inv).astype(F)
        r = (o - info["centre"].astype(F)).astype(F)
        r2 = fma(r[2], r[2], fma(r[1], r[1], F(r[0] * r[0])))
        pa = (F(nodes[0][12] * r2) * ainv).astype(F)
        cur = 0
        if info["root_leaf"]:
            k = 1 if info["root_leaf"] == 1 else 0
            row = nodes[0]
            leaf(int(row.view(np.uint32)[REF[1 - k]]))
            a = fma(row[list(M[k])], inv, -oi)
            b = fma(row[list(E[k])], ainv, pa)
            tn = np.fmax(np.fmax(F(a[0] - b[0]), F(a[1] - b[1])), F(a[2] - b[2]))
            tf = np.fmin(np.fmin(F(a[0] + b[0]), F(a[1] + b[1])), F(a[2] + b[2]))
            cur = int(row.view(np.uint32)[REF[k]]) if (tn <= tf and tn <= best and tf >= 0) else None
        a_u, b_u = fma(info["flat_m"], inv[1], -oi[1]), fma(info["flat_e"], ainv[1], pa[1])
        tyf = F(a_u + b_u)
        N = np.fmax(F(a_u - b_u), F(0))
        Fv = tyf if tyf < best else best
        if not N <= Fv:
            cur = None
        stack = []
        while cur is not None:
            if cur & LEAF:
                leaf(cur)
                Fv = best if best < Fv else Fv
                cur = stack.pop() if stack else None
                continue
            row = nodes[cur]
            refs = row.view(np.uint32)
            hit, tn = [False, False], [F(0), F(0)]
            for c in (0, 1):
                ax, az = fma(row[M[c][0]], inv[0], -oi[0]), fma(row[M[c][2]], inv[2], -oi[2])
                bx, bz = fma(row[E[c][0]], ainv[0], pa[0]), fma(row[E[c][2]], ainv[2], pa[2])
                tn[c] = np.fmax(np.fmax(F(ax - bx), F(az - bz)), N)
                tf = np.fmin(np.fmin(F(ax + bx), F(az + bz)), Fv)
                hit[c] = bool(tn[c] <= tf)
            c0, c1 = int(refs[REF[0]]), int(refs[REF[1]])
            if hit[0] and hit[1]:
                swap = tn[1] < tn[0]
                stack.append(c0 if swap else c1)
                cur = c1 if swap else c0
            elif hit[0]:
                cur = c0
            elif hit[1]:
                cur = c1
            else:
                cur = stack.pop() if stack else None
    return shown if sphere_t is None else (shown, best, best_id)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


def ray_families(info, rng, extent):
    """(name, o, d) — random rays and the families the flat walk's own arithmetic is sensitive to."""
    lo, hi = float(info["flat_m"]) - float(info["flat_e"]), float(info["flat_m"]) + float(info["flat_e"])
    ex, ez = extent
    xz = lambda s=1.0: (rng.uniform(-ex, ex) * s, rng.uniform(-ez, ez) * s)
    for q in range(260):  # camera-like and bounce-like rays
        x, z = xz(1.2)
        o = np.array([x, rng.uniform(0.0, 6.0), z], F)
        tx, tz = xz()
        yield "random", o, unit(np.array([tx, rng.uniform(-0.5, 1.0), tz]) - o)
    for q in range(120):  # d.y = 0 exactly: inside the slab, outside it, and within an ulp of its faces
        x, z = xz(1.3)
        y = [rng.uniform(lo, hi), rng.uniform(hi, hi + 2), rng.uniform(lo - 2, lo), hi, lo, np.nextafter(F(hi), F(np.inf)), np.nextafter(F(lo), F(-np.inf)),
             np.nextafter(F(hi), F(-np.inf)), 0.0, 0.45][q % 10]
        ang = rng.uniform(0, 2 * np.pi)
        yield "d.y=0", np.array([x, y, z], F), np.array([np.cos(ang), 0.0, np.sin(ang)], F)
    for q in range(120):  # origins in the layer only the union covers (above the unraised spheres' boxes), any direction
        x, z = xz()
        o = np.array([x, rng.uniform(0.45, 0.56), z], F)
        dd = rng.normal(0, 1, 3)
        if q % 3 == 0:
            dd[1] *= 0.02  # nearly along the layer
        yield "layer", o, unit(dd)
    for q in range(120):  # grazing the slab's faces: through a point on a face at a shallow angle, from outside and from inside
        x, z = xz()
        face = hi if q % 2 else lo
        p = np.array([x, face, z])
        dd = np.array([rng.normal(), rng.normal() * 10.0 ** rng.uniform(-7, -1), rng.normal()])
        dd = dd / np.linalg.norm(dd)
        o = (p - dd * rng.uniform(0.0, 30.0)).astype(F)
        yield "graze", o, unit(dd)
    for q in range(60):  # axis-parallel: infinite reciprocals, NaN axes
        x, z = xz()
        o = np.array([x, rng.uniform(lo - 0.5, hi + 0.5), z], F)
        if q % 5 == 0:
            o[rng.integers(0, 3)] = 0.0  # 0 x inf
        yield "axis", o, np.array([(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)][q % 4], F)
    for q in range(60):  # along y alone: x and z carry no finite constraint
        x, z = xz()
        if q % 4 == 0:
            x, z = np.round(x * 0.9), np.round(z * 0.9)  # through sphere centres' neighbourhood
        up = q % 2 == 0
        o = np.array([x, rng.uniform(-3.0, lo) if up else rng.uniform(hi, 6.0), z], F)
        if q % 6 == 5:
            o[1] = rng.uniform(lo, hi)  # starts inside the slab
        yield "y-only", o, np.array([0, 1 if up else -1, 0], F)


def run_families(info, nodes, ids, arrs, extent, seed):
    rng = np.random.default_rng(seed)
    cx, cy, cz, rsq = arrs["center_x"], arrs["center_y"], arrs["center_z"], arrs["radius_sq"]
    active = arrs["inv_radius"] != 0
    seen = {}
    for name, o, d in ray_families(info, rng, extent):
        jitter = rng.integers(0, 2, 3) * 2 - 1
        flagged = set(np.nonzero(ref_flagged(cx, cy, cz, rsq, o, d) & active)[0].tolist())
        shown = set(ids[flat_walk(info, nodes, ids, o, d, jitter)].tolist()) - {EMPTY}
        assert flagged <= shown, (name, o, d, sorted(flagged - shown)[:5])
        # with pruning: the minimum offer, ties to the lowest index, as brute force finds it
        t = np.where(active, offers(cx, cy, cz, rsq, o, d), F(np.inf)).astype(F)
        _, best, best_id = flat_walk(info, nodes, ids, o, d, jitter, sphere_t=t)
        if np.isfinite(t).any():
            want = int(np.nonzero(t == t.min())[0][0])
            assert best_id == want and best == t[want], (name, o, d, best_id, want)
        else:
            assert best_id == EMPTY, (name, o, d, best_id)
        s = seen.setdefault(name, [0, 0])
        s[0] += 1
        s[1] += len(flagged) > 0
    return seen


def test_flat_walk_presents_every_flagged_sphere_and_returns_the_minimum_offer_large_scene():
    sc = r1.create_large_scene(1200, 800)
    info, nodes, ids = binding.bvh_describe(sc.spheres.contents)
    seen = run_families(info, nodes, ids, sc.arrays(), (16.0, 9.0), 11)
    assert set(seen) == {"random", "d.y=0", "layer", "graze", "axis", "y-only"}
    for name, (n, with_candidates) in seen.items():
        assert with_candidates > n // 8, (name, n, with_candidates)  # the family does meet spheres


@pytest.mark.parametrize("ground", [True, False])
def test_flat_walk_on_a_synthetic_lattice(ground):
    """Without the ground sphere the root has no root-step shape: the walk starts in the loop at node 0, whose boxes the slab covers."""
    c, rad = lattice(16, 12, 0.17, 1, ground)
    cs, arrs, mt = _raw_scene(c, rad)
    info, nodes, ids = binding.bvh_describe(cs)
    assert info["flat_axis"] == 1 and (info["root_leaf"] != 0) == ground
    seen = run_families(info, nodes, ids, arrs, (9.0, 7.0), 12 + ground)
    assert sum(v[1] for v in seen.values()) > 100
