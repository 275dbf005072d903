"""GPU test of RE-SORTED scenes in every trace build and on the edge trees, as tests/test_gpu_update_builds.py is for updated
ones and with its helpers: after r1_resort_spheres on a context that holds one of the 43 scenes of tests/update_scenes.py, every render and
query gives what the CPU ORACLE gives for the context's current spheres — bytes, records and ray counts.  A re-sort changes no sphere, so
the oracle's frames of the arrays are the expectation whatever the leaves look like; but it re-deals the leaves of 40 of the 43 scenes even
when nothing has moved (the builder does not order leaves by x), among them the twins and the coincident spheres, whose equal-t hits must
still go the reference's way, and the odd spheres next to a -inf partner word (tests/test_resort_scenes_host.py asserts all of this).

States, each after r1_set_scene(original):
  resort              the re-sort alone                                              the oracle's unedited frames
  all+resort          update_scenes' `all` edit in one r1_update_spheres, re-sort     the `all` frames
  roll+resort         resort_scenes.rolled in one r1_update_centers, re-sort           the roll's frames
  resort+materials    the re-sort, then a materials-only update                        the `materials` frames

  a. MATRIX_IDS (15 scenes) x the four states: all eight calls of tests/test_gpu_builds_edges.py through the tree; sync through DEFAULT, the
     tree's diagnostic build (with records) and the reference form; pass through the reference form.  The rule-on adaptive call is left out
     where the restated rule stops every tile of the expected frame at one count (test_update_scenes_host.ADAPTIVE_SKIP's criterion).
  b. the ten scenes whose tree has a flat slab: the frame before the re-sort (slab in use), after it (dropped) and after r1_set_scene with the
     same arrays (back); the grid and the sweep are refused in between and work again afterwards.
  c. the device form after a re-sort on the big sizes of `n3`, `n7`, `k3`, `k4`: inv_radius 0 for a root-leaf sphere, a partner-less odd
     sphere and the live partner of a full pair OF THE RE-SORTED TREE, so the entry goes through the re-written slot table; a second re-sort.
  d. stream order: call, re-sort, the same call, ONE wait, for async, pixel, batch and path.
  e. r1_cast_rays (closest, any) and r1_trace_rays over the frame's camera rays on all 43 scenes after `resort` and `roll+resort`.

One case collects the steps that differ and fails once.  Nothing has a tolerance and no GPU render is an expectation."""
import functools

import numpy as np
import pytest

from rays1bench_amd import binding

import adaptive_rule as rule
import edge_scenes as es
import resort_scenes as rsc
import root_leaf_scenes as rs
import update_scenes as us
import test_gpu_builds_edges as tbe
from test_gpu_builds_edges import renderer  # noqa: F401  (the module-scoped fixture)
from test_gpu_cast import same_hits
from test_gpu_update import first_difference
from test_gpu_update_builds import MATRIX_IDS, Collector, adaptive, enqueue, landed, one_call, refused, rotated, start, to_device, wanted  # noqa: F401
from test_resort_scenes_host import FLAT
from test_update_scenes_host import odd_spheres, tree_of

pytestmark = pytest.mark.gpu

W, H = us.W, us.H
TREE, REFERENCE, GRID, SWEEP = binding.VARIANT_BVH, binding.VARIANT_REFERENCE, binding.VARIANT_GRID, binding.VARIANT_PREFILTER
CALLS = tbe.CALLS
MOVED_RULE = "the scene has moved"
STATES = ("resort", "all+resort", "roll+resort", "resort+materials")
BIG_FOUR = ["leaf-n3-big", "leaf-n7-big", "root-k3-back-big", "root-k4-front-big"]
assert set(BIG_FOUR) <= set(us.IDS) and FLAT <= set(us.IDS)


def arrays_of(case, state):
    """the arrays the context holds after `state`"""
    sa, _ = us.scene(case.id)
    if state == "roll+resort":
        return rsc.rolled(sa)
    return sa if state == "resort" else us.scene(case.id, "all" if state == "all+resort" else "materials")[0]


def expected_of(case, state):
    if state == "roll+resort":
        return us.expected_of(("roll", case.id), lambda: (rsc.rolled(us.scene(case.id)[0]), us.scene(case.id)[1], case.seed))
    return us.expected(case, {"resort": None, "all+resort": "all", "resort+materials": "materials"}[state])


def enter(renderer, case, state):
    """the state's calls on a context that holds the original scene; returns the arrays it then holds"""
    new = arrays_of(case, state)
    if state == "all+resort":
        centers, radii, materials = us.groups_of(new)
        renderer.update_spheres(0, centers=centers, radii=radii, materials=materials)
    elif state == "roll+resort":
        renderer.update_centers(0, *us.groups_of(new)[0])
    renderer.resort_spheres()
    if state == "resort+materials":
        renderer.update_spheres(0, materials=us.groups_of(new)[2])
    return new


def runs_rule_on(exp):
    hist = rule.histogram(exp.ruled(True)[0])
    return len(hist) >= 2 and min(hist) < es.CAP


# ---- a: every call through the tree, in every state ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("cid", MATRIX_IDS)
def test_every_tree_call_on_a_resorted_scene_renders_the_oracles_frames(renderer, cid, state):
    case = us.BY_ID[cid]
    exp = expected_of(case, state)
    _, cam2 = start(renderer, case)
    new = enter(renderer, case, state)
    c = Collector((cid, state))
    steps = [(f"tree {call}", call, TREE, None) for call in CALLS if call != "adaptive" or runs_rule_on(exp)]
    steps += [("default sync", "sync", binding.VARIANT_DEFAULT, TREE), ("tree_stats sync", "sync", binding.VARIANT_BVH_STATS, None),
              ("reference sync", "sync", REFERENCE, None), ("reference pass", "pass", REFERENCE, None)]
    for tag, call, variant, kernel in rotated(steps, us.IDS.index(cid) * 5 + STATES.index(state)):
        c.step(tag, lambda: one_call(renderer, case, new, cam2, exp, call, variant, kernel))
    c.done()


# ---- b: the flat slab goes and comes back ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cid", sorted(FLAT))
def test_the_flat_slab_is_dropped_by_a_resort_and_comes_back_with_set_scene(renderer, cid):
    case = us.BY_ID[cid]
    exp = us.expected(case)
    info, nodes, ids = tree_of(cid)
    assert info["flat_axis"] == 1
    sa, cam2 = start(renderer, case)
    c = Collector((cid, "flat slab"))
    sync = lambda variant: one_call(renderer, case, sa, cam2, exp, "sync", variant)
    for tag, variant in (("tree", TREE), ("grid", GRID), ("sweep", SWEEP)):
        c.step(f"before the re-sort, {tag}", lambda: sync(variant))
    renderer.resort_spheres()
    for tag, variant in (("grid", GRID), ("sweep", SWEEP)):
        c.step(f"{tag} refused", lambda: refused(lambda: tbe.run(renderer, sa, cam2, "sync", variant, case.seed), MOVED_RULE))
    c.step("after the re-sort, tree", lambda: sync(TREE))
    c.step("after the re-sort, async", lambda: one_call(renderer, case, sa, cam2, exp, "async", TREE))

    def rebuilt():
        assert np.array_equal(renderer.bvh_ids_download(), ids) and renderer.bvh_download().tobytes() == nodes.tobytes()

    start(renderer, case)
    c.step("r1_set_scene with the same arrays rebuilds", rebuilt)
    for tag, variant in (("tree", TREE), ("grid", GRID), ("sweep", SWEEP)):
        c.step(f"after r1_set_scene, {tag}", lambda: sync(variant))
    c.done()


# ---- c: the device form through the re-written slot table -----------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def resorted_tree(cid):
    sa, _ = us.scene(cid)
    return binding.bvh_resort_describe(es.cscene(sa), *(sa.arrays[k] for k in us.CENTRE_KEYS))


@functools.lru_cache(maxsize=None)
def named_spheres(cid):
    """test_gpu_update_builds.named_spheres on the RE-SORTED tree of the unmoved scene: {"root": the last sphere of the root leaf (pinned: where
    the builder put it), "odd": a sphere whose partner word is -inf, "partner": the second sphere of a full pair}, of the odd spheres and of
    the partners one that the re-sort gave another slot and whose going shows in the oracle's frame (tried in the order of how many primary rays hit them)."""
    case = us.BY_ID[cid]
    sa, cam2 = us.scene(cid)
    rinfo, rows, ids = resorted_tree(cid)
    index = binding.cast_rays_host(es.cscene(sa), es.primary_rays(sa.camera_array))["index"]
    seen = np.bincount(index[index >= 0], minlength=sa.count)
    def slot_of(table):
        out, occupied = np.full(sa.count, -1), table != 0xFFFFFFFF
        out[table[occupied]] = np.nonzero(occupied)[0]
        return out

    moved = slot_of(ids) != slot_of(tree_of(cid)[2])  # per sphere: the re-sort gave it another slot (placeholders: never)

    def shows(sphere):
        exp = us.expected_of((cid, "dropped after a re-sort", sphere), lambda: (us.dropped(sa, sphere), cam2, case.seed))
        return exp.frame0[0] != us.expected(case).frame0[0]

    def most(spheres):
        order = spheres[np.lexsort((-seen[spheres], ~moved[spheres]))]  # those the re-sort moved first, the most seen of them first
        return next((int(s) for s in order[:12] if shows(int(s))), int(order[0]))

    out = {}
    if case.group == "root":
        out["root"] = [s for s in rs.root_leaf_of(sa)[2] if s >= 0][-1]
    odd = odd_spheres(ids)
    if odd.size:
        out["odd"] = most(odd)
    pairs = ids.reshape(-1, 2).astype(np.int64)
    full = pairs[(pairs != 0xFFFFFFFF).all(1)]
    if len(full):
        out["partner"] = most(full[:, 1])
    return out


DROPS = [(cid, which) for cid in BIG_FOUR for which in ("root", "odd", "partner") if not (which == "root" and cid.startswith("leaf"))]


@pytest.mark.parametrize("cid,which", DROPS)
def test_device_form_drop_after_a_resort_and_a_second_resort(renderer, cid, which):
    case = us.BY_ID[cid]
    spheres = named_spheres(cid)
    assert which in spheres, (cid, which, spheres)
    sphere = spheres[which]
    before = tree_of(cid)[2]
    if which != "root":  # the re-sort moved it: the builder's slot table would send the entry elsewhere
        assert int(np.nonzero(resorted_tree(cid)[2] == sphere)[0][0]) != int(np.nonzero(before == sphere)[0][0]), (cid, which, sphere)
    sa, cam2 = start(renderer, case)
    gone = us.dropped(sa, sphere)
    exp = us.expected_of((cid, "dropped after a re-sort", sphere), lambda: (gone, cam2, case.seed))
    assert exp.frame0[0] != us.expected(case).frame0[0], "the sphere that goes must show in the frame"
    renderer.resort_spheres()
    held, ptrs = to_device(us.groups_of(gone, "radii")[1])
    renderer.update_spheres_device(0, sa.count, radii=ptrs)
    c = Collector((cid, f"inv_radius 0 on {which} sphere {sphere} after a re-sort"))
    k = DROPS.index((cid, which))
    for call in rotated(("sync", "batch", "pixel"), k):
        c.step(call, lambda: one_call(renderer, case, gone, cam2, exp, call, TREE))
    renderer.resort_spheres()
    for call in rotated(("sync", "async", "pass"), k):
        c.step(f"second re-sort, {call}", lambda: one_call(renderer, case, gone, cam2, exp, call, TREE))
    c.step("second re-sort, reference", lambda: one_call(renderer, case, gone, cam2, exp, "sync", REFERENCE))

    def tables():
        x, y, z = (sa.arrays[k] for k in us.CENTRE_KEYS)
        info, rows, ids = binding.bvh_resort_describe(es.cscene(sa), x, y, z, gone.arrays["radius_sq"], gone.arrays["inv_radius"])
        got_ids, got_rows = renderer.bvh_ids_download(), renderer.bvh_download()
        assert np.array_equal(got_ids, ids), ("ids", np.nonzero(got_ids != ids)[0][:8])
        assert got_rows.tobytes() == rows.tobytes(), first_difference(got_rows, rows)

    c.step("ids and rows equal the host's with the dropped radii", tables)
    renderer.sync()  # (the device arrays are freed with this case: nothing may still read them)
    c.done()


# ---- d: stream order ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("call", ("async", "pixel", "batch", "path"))
@pytest.mark.parametrize("cid", BIG_FOUR)
def test_frames_enqueued_before_and_behind_a_resort_are_the_oracles(renderer, cid, call):
    """Frame A walks the builder's leaves, frame B the re-sorted ones; the re-sort between them waits for nothing and changes no pixel."""
    case = us.BY_ID[cid]
    exp = us.expected(case)
    sa, cam2 = start(renderer, case)
    make = (lambda: binding.HostFrame(W, H)) if call in ("async", "pixel") else (lambda: binding.HostFrames(W, H, 2))
    fa, fb = make(), make()
    try:
        renderer.set_pixel_mode(call == "pixel")
        enqueue(renderer, sa, cam2, call, case.seed, fa)
        renderer.resort_spheres()
        enqueue(renderer, sa, cam2, call, case.seed, fb)
        renderer.sync()                                       # one wait for all three
        got_a, got_b = landed(call, fa), landed(call, fb)
    finally:
        renderer.set_pixel_mode(False)
        fa.close(), fb.close()
    c = Collector((cid, call, "stream order"))
    c.step("frame A, the builder's leaves", lambda: tbe.check(renderer, got_a, wanted(exp, call), TREE, case.size))
    c.step("frame B, the re-sorted leaves", lambda: tbe.check(renderer, got_b, wanted(exp, call), TREE, case.size))

    def resorted():
        ids = renderer.bvh_ids_download()
        assert np.array_equal(ids, resorted_tree(cid)[2]) and not np.array_equal(ids, tree_of(cid)[2])

    c.step("the ids after both frames", resorted)
    c.done()


# ---- e: queries --------------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def query_expectation(cid, state):
    """test_gpu_update_builds.query_expectation for the arrays of `state`: the frame's own camera rays and stream states, and the host forms'
    answers on those arrays"""
    case = us.BY_ID[cid]
    new = arrays_of(case, state)
    x, y, s = us.camera_samples()
    rays, seeds = binding.camera_rays(es.ccamera(new.camera_array), binding.make_params(W, H, us.CAP, case.seed), x, y, s)
    cs = es.cscene(new)
    return (rays, seeds, binding.cast_rays_host(cs, rays, binding.CAST_CLOSEST), binding.cast_rays_host(cs, rays, binding.CAST_ANY),
            binding.trace_rays_host(cs, rays, seeds, 50))


@pytest.mark.parametrize("cid", us.IDS)
def test_ray_and_path_queries_on_resorted_scenes_equal_the_host_forms(renderer, cid):
    case = us.BY_ID[cid]
    c = Collector((cid, "queries"))
    for state in ("resort", "roll+resort"):
        start(renderer, case)
        enter(renderer, case, state)
        rays, seeds, closest, occluded, radiance = query_expectation(cid, state)
        for tag, variant in (("tree", TREE), ("reference", REFERENCE)):
            c.step(f"{state} {tag} closest", lambda: same_hits(renderer.cast_rays(rays, binding.CAST_CLOSEST, variant), closest, (cid, state, tag)))
            c.step(f"{state} {tag} any", lambda: same_hits(renderer.cast_rays(rays, binding.CAST_ANY, variant), occluded, (cid, state, tag, "any")))

            def trace():
                got = renderer.trace_rays(rays, seeds, 50, variant)
                bad = np.nonzero((got.view(np.uint32).reshape(-1, 4) != radiance.view(np.uint32).reshape(-1, 4)).any(1))[0]
                assert bad.size == 0, f"{bad.size} of {len(rays)} records differ from r1_trace_rays_host, first at {bad[:8]}"

            c.step(f"{state} {tag} trace", trace)
        c.step(f"{state} grid refused", lambda: refused(lambda: renderer.cast_rays(rays[:64], binding.CAST_CLOSEST, GRID), MOVED_RULE))
    c.done()
