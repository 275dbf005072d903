"""GPU test of updated scenes in every trace build and on the edge trees: after ONE r1_update_centers* or
r1_update_spheres* call on a context that holds the original scene, every render and query gives what the CPU ORACLE gives for the edited
arrays — bytes, records and ray counts — over the 43 scenes of tests/update_scenes.py: the leaf shapes (an odd sphere next to a -inf
partner word, a one-sphere leaf in front of the sentinel pair), the root leaves the root step reads through the scalar cache, and the edge
scenes with unusual radii and materials, small (the LDS kernels) and big (the big-scene kernels).

  a. move, radii, all: all eight calls of tests/test_gpu_builds_edges.py (sync with records, async, pixel, batch, path, pass, adaptive with
     the rule off and on) through the tree; sync through DEFAULT, the tree's diagnostic build (with records) and the reference form; pass
     through the reference form.
  b. materials alone, after which the grouped sweep and the grid stay valid: all eight calls through the tree, the sweep and the grid, the
     five synchronous-only builds; the grid had been built before the update in every other case and is built after it in the others.
  c. after a radii update every call through the sweep and the grid is refused and leaves nothing behind.
  d. the device form: all three groups, a never-hittable entry (inv_radius 0) on a sphere of the root leaf, on a partner-less odd sphere and
     on the live partner of a full pair, and a mat_type 7 entry, which is skipped.
  e. stream order: call, update, the same call, ONE wait — for async, pixel, batch and path, around a materials update (the set kernel alone)
     and a radii update, both of which change root-leaf spheres.
  f. r1_cast_rays (closest, any) and r1_trace_rays over the frame's own camera rays against the host forms on the edited arrays.

One test case is one (scene, edit): r1_set_scene(original), one update, then the calls one after the other — every call is made in every
case, and their order rotates from case to case, so that each call is also the first one after an update.  A case collects the calls that
differ and fails once, naming all of them.  Frames are 64 x 48 at 2 samples, the adaptive call at its cap of 6, tiles 32 x 32 (adaptive:
16 x 16).  Nothing here has a tolerance and no GPU render is an expectation: every comparison is with update_scenes.frames or with the
restated rule on the oracle's records (tests/test_update_scenes_host.py asserts that the edits show and on which pairs the rule-on adaptive
call has a map worth the name: ADAPTIVE_SKIP's pairs leave that one call out).

Thinned for time, along scenes alone — no call and no edit is left out anywhere: (a) and (b) run on MATRIX_IDS, 15 of the 43 scenes: the
small size of every leaf scene (`n1`, `n3`, `n5`, `n7`, `behind`, `coincident`: odd spheres next to a -inf partner word, the one-sphere leaf
in front of the sentinel pair), of eight root-leaf scenes (`k1`/front, `k3` and `k4` in both orders, `k5`/front, `twins`/front: root leaves
of one to four spheres read through the scalar cache, at the front and at the back of the sphere table) and of `palette` (the materials' edge
values), and `wide` (the two-pair root leaf in the big-scene kernels).  (c) to (f) keep scenes the matrix leaves out: (d) and (e) the big
sizes of `n3`, `n7`, `k3` and `k4`, (f) all 43.  The bound is this module's wall time against tests/test_gpu_builds_edges.py's in one
session; DESIGN.md §4.27 has the figures.

The adaptive call is restated here and not imported: test_gpu_builds_edges.adaptive takes its seed from edge_scenes.SEED by the scene's
name, which the leaf and root scenes are not in; the assertions are the same."""
import functools

import numpy as np
import pytest

from rays1bench_amd import binding
import r1o

import adaptive_rule as rule
import edge_scenes as es
import root_leaf_scenes as rs
import update_scenes as us
import test_gpu_builds_edges as tbe
from test_gpu_builds_edges import renderer  # noqa: F401  (the module-scoped fixture)
from test_gpu_cast import same_hits
from test_update_scenes_host import ADAPTIVE_SKIP, odd_spheres, tree_of

pytestmark = pytest.mark.gpu

W, H, SPP = us.W, us.H, us.SPP
TREE, REFERENCE, GRID = binding.VARIANT_BVH, binding.VARIANT_REFERENCE, binding.VARIANT_GRID
CALLS, FAMILIES, SYNC_ONLY = tbe.CALLS, tbe.FAMILIES, tbe.SYNC_ONLY
MOVED_RULE = "the scene has moved"
TREE_KINDS = ("move", "radii", "all")
# (a) and (b): 15 of the 43 scenes (the module's docstring says why these)
MATRIX_IDS = [f"leaf-{n}-small" for n in ("n1", "n3", "n5", "n7", "behind", "coincident")] + \
             [f"root-{n}-small" for n in ("k1-front", "k3-front", "k3-back", "k4-front", "k4-back", "k5-front", "twins-front")] + \
             ["root-wide-front-big", "edge-palette-small"]
assert set(MATRIX_IDS) <= set(us.IDS)


# ---- the steps of a case ------------------------------------------------------------------------------------------------------------------


def start(renderer, case):
    """r1_set_scene with the case's ORIGINAL arrays"""
    sa, cam2 = us.scene(case.id)
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    return sa, cam2


def update(renderer, case, kind):
    """ONE update call: r1_update_centers for a move, r1_update_spheres with the groups that changed for the others"""
    new, _ = us.scene(case.id, kind)
    centers, radii, materials = us.groups_of(new, kind)
    if kind == "move":
        renderer.update_centers(0, *centers)
    else:
        renderer.update_spheres(0, centers=centers, radii=radii, materials=materials)
    return new


def adaptive(renderer, variant, seed, exp, rule_on):
    """tests/test_gpu_builds_edges.py's adaptive call with the seed given: over 16 x 16 tiles; rule off (max_delta -1): the full frame at
    the cap; rule on: reports and ray count are the restated rule's on the oracle's records, every tile's pixels the oracle's prefix frame at
    the tile's count."""
    p = tbe.params(variant, seed, es.CAP, es.ADAPT_TILE)
    max_delta, mean_q8 = es.RULE if rule_on else (-1, 0)
    img, rays, tiles, res = renderer.render_adaptive(p, es.MIN_SPP, es.PASS_SPP, max_delta, mean_q8)
    want_tiles, want_rays = exp.ruled(rule_on)
    print("map", rule.histogram(tiles), "the rule's", rule.histogram(want_tiles), "rays", rays, want_rays)
    for f in ("spp", "settled", "err_max", "err_sum"):
        assert np.array_equal(tiles[f], want_tiles[f]), (f, tiles[f], want_tiles[f])
    assert rays == want_rays
    boxes = rule.tile_boxes(W, H, es.ADAPT_TILE, es.ADAPT_TILE)
    assert len(tiles) == len(boxes) == res["tiles"] == 12
    for n in sorted(set(int(x) for x in tiles["spp"])):
        want = exp.prefix(n)
        for t, (x0, y0, x1, y1) in enumerate(boxes):
            if int(tiles[t]["spp"]) == n:
                assert img[y0:y1, x0:x1].tobytes() == want[y0:y1, x0:x1].tobytes(), (n, t)
    assert res["samples"] == rule.samples_of(tiles, W, H, es.ADAPT_TILE, es.ADAPT_TILE)
    assert res["tiles_settled"] == int((tiles["settled"] != 0).sum())
    if rule_on:
        assert len(set(int(x) for x in tiles["spp"])) >= 2 and int(tiles["spp"].min()) < es.CAP
    else:
        assert (tiles["spp"] == es.CAP).all() and (img.tobytes(), rays) == exp.full
    assert renderer.launch_info()["kernel"] == variant


def wanted(exp, call):
    """[(image bytes, rays)] of the frames `call` renders"""
    if call == "path":
        return [exp.frame0, exp.path1]
    return exp.frames if call == "batch" else [exp.frame0]


def one_call(renderer, case, sa, cam2, exp, call, variant, kernel=None):
    """One call through `variant` against `exp` (update_scenes.Expected); launch_info's kernel (`kernel`, or the variant) and the small / big
    split as test_gpu_builds_edges.check asserts them; the synchronous frame's records too."""
    if call.startswith("adaptive"):
        adaptive(renderer, variant, case.seed, exp, call == "adaptive")
        return
    got = tbe.run(renderer, sa, cam2, call, variant, case.seed)
    tbe.check(renderer, got, wanted(exp, call), variant if kernel is None else kernel, case.size)
    if call == "sync":
        tbe.check_records(got[0][2], exp.records)
    if call == "async" and variant == TREE:
        assert renderer.launch_info()["tiles_in_kernel"] == 1  # (as test_gpu_builds_edges.py asserts it: the tiles land in the kernel)


class Collector:
    """The steps of one case: a step whose comparison fails is noted and the case goes on, so that one run names every call that differs.
    An error of the device or the runtime is no comparison: it ends the whole run, and nothing more is started on the device."""

    def __init__(self, what):
        self.what, self.failed = what, []

    def step(self, tag, fn):
        try:
            fn()
        except AssertionError as e:
            self.failed.append(f"{tag}: {str(e)[:300]}")
        except binding.R1Error as e:
            if e.code in (binding.R1_EHIP, binding.R1_ENOMEM, binding.R1_ENODEVICE):
                pytest.exit(f"{self.what} {tag}: {e} — a device error: nothing more is run", returncode=3)
            self.failed.append(f"{tag}: refused: {e}")

    def done(self):
        assert not self.failed, f"{self.what}: {len(self.failed)} steps differ:\n  " + "\n  ".join(self.failed)


def rotated(seq, k):
    seq = list(seq)
    k %= len(seq)
    return seq[k:] + seq[:k]


def runs_rule_on(case, kind):
    return (case.id, kind) not in ADAPTIVE_SKIP


# ---- a: the tree family, every call --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", TREE_KINDS)
@pytest.mark.parametrize("cid", MATRIX_IDS)
def test_every_tree_call_after_a_move_or_a_radii_update_renders_the_oracles_frames(renderer, cid, kind):
    case = us.BY_ID[cid]
    exp = us.expected(case, kind)
    _, cam2 = start(renderer, case)
    new = update(renderer, case, kind)
    c = Collector((cid, kind))
    steps = [(f"tree {call}", call, TREE, None) for call in CALLS if call != "adaptive" or runs_rule_on(case, kind)]
    steps += [("default sync", "sync", binding.VARIANT_DEFAULT, TREE), ("tree_stats sync", "sync", binding.VARIANT_BVH_STATS, None),
              ("reference sync", "sync", REFERENCE, None), ("reference pass", "pass", REFERENCE, None)]
    for tag, call, variant, kernel in rotated(steps, us.IDS.index(cid) * 3 + TREE_KINDS.index(kind)):
        c.step(tag, lambda: one_call(renderer, case, new, cam2, exp, call, variant, kernel))
    c.done()


# ---- b: materials alone, every family ------------------------------------------------------------------------------------------------------


def materials_case(renderer, case, grid_first):
    exp = us.expected(case, "materials")
    sa, cam2 = start(renderer, case)
    if grid_first:  # the grid exists before the update; otherwise ensure_grid builds it afterwards, from the host copies the update wrote
        tbe.check(renderer, tbe.run(renderer, sa, cam2, "sync", GRID, case.seed), [us.expected(case).frame0], GRID, case.size)
    new = update(renderer, case, "materials")
    return exp, new, cam2


def grid_first_of(cid, k=0):
    return (us.IDS.index(cid) + k) % 2 == 1


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("cid", MATRIX_IDS)
def test_every_call_of_every_family_after_a_materials_update_renders_the_oracles_frames(renderer, cid, family):
    case = us.BY_ID[cid]
    exp, new, cam2 = materials_case(renderer, case, grid_first_of(cid, sorted(FAMILIES).index(family)))
    c = Collector((cid, "materials", family))
    calls = [call for call in CALLS if call != "adaptive" or runs_rule_on(case, "materials")]
    for call in rotated(calls, us.IDS.index(cid) + sorted(FAMILIES).index(family)):
        c.step(f"{family} {call}", lambda: one_call(renderer, case, new, cam2, exp, call, FAMILIES[family]))
    c.done()


@pytest.mark.parametrize("cid", MATRIX_IDS)
def test_the_synchronous_only_builds_after_a_materials_update_render_the_oracles_frame(renderer, cid):
    case = us.BY_ID[cid]
    exp, new, cam2 = materials_case(renderer, case, not grid_first_of(cid))
    c = Collector((cid, "materials", "sync only"))
    for build in rotated(sorted(SYNC_ONLY), us.IDS.index(cid)):
        c.step(build, lambda: one_call(renderer, case, new, cam2, exp, "sync", SYNC_ONLY[build]))
    c.done()


# ---- c: refusals leave nothing behind ------------------------------------------------------------------------------------------------------


def refused(fn, text):
    with pytest.raises(binding.R1Error) as e:
        fn()
    assert e.value.code == binding.R1_EINVAL and text in str(e.value), e.value


@pytest.mark.parametrize("cid", ["leaf-n7-small", "root-k4-front-small", "edge-palette-big"])
def test_refused_calls_after_a_radii_update_leave_nothing_behind(renderer, cid):
    case = us.BY_ID[cid]
    exp = us.expected(case, "radii")
    _, cam2 = start(renderer, case)
    renderer.render_pass(tbe.params(TREE, case.seed, 1), 0)  # an accumulation of one sample on the original scene
    new = update(renderer, case, "radii")
    refused(lambda: renderer.render_pass(tbe.params(TREE, case.seed, SPP - 1), 1), "no accumulation to continue")
    for family in ("sweep", "grid"):
        for call in CALLS:
            if call.startswith("adaptive"):
                fn = lambda: renderer.render_adaptive(tbe.params(FAMILIES[family], case.seed, es.CAP, es.ADAPT_TILE), es.MIN_SPP, es.PASS_SPP,
                                                      *(es.RULE if call == "adaptive" else (-1, 0)))
            else:
                fn = lambda: tbe.run(renderer, new, cam2, call, FAMILIES[family], case.seed)
            refused(fn, MOVED_RULE)
        for call in ("batch", "pass"):  # after the refusals of this family: the tree's next frames
            one_call(renderer, case, new, cam2, exp, call, TREE)
    refused(lambda: renderer.render_pass(tbe.params(TREE, case.seed, 1), SPP + 1), "samples are accumulated")
    one_call(renderer, case, new, cam2, exp, "sync", TREE)


# ---- d: the device form --------------------------------------------------------------------------------------------------------------------

DEVICE_CASES = [c.id for c in us.CASES if (c.name, c.order) in (("k4", "front"), ("k3", "back"), ("n3", None), ("n7", None), (rs.WIDE, "front"))]
DEVICE_CALLS = ("sync", "batch", "pixel", "adaptive_off")


def to_device(arrays):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in arrays]
    return t, tuple(v.data_ptr() for v in t)


@functools.lru_cache(maxsize=None)
def named_spheres(cid):
    """The spheres of a case's ORIGINAL tree that the device form's odd entries go to: {"root": the last sphere of the root leaf (a ball;
    the ground where the root leaf is the ground alone), "odd": a sphere whose partner word is -inf, "partner": the second sphere of a full
    pair}; of the odd spheres and of the partners the one that most of the frame's primary rays hit, so that its entry shows."""
    case = us.BY_ID[cid]
    sa, _ = us.scene(cid)
    info, nodes, ids = tree_of(cid)
    index = binding.cast_rays_host(es.cscene(sa), es.primary_rays(sa.camera_array))["index"]
    seen = np.bincount(index[index >= 0], minlength=sa.count)
    most = lambda spheres: int(spheres[np.argmax(seen[spheres])])
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


def device_calls(renderer, case, sa, cam2, exp, what, k=0):
    c = Collector((case.id, what))
    for call in rotated(DEVICE_CALLS, k):
        c.step(call, lambda: one_call(renderer, case, sa, cam2, exp, call, TREE))
    c.done()


@pytest.mark.parametrize("cid", DEVICE_CASES)
def test_device_form_of_all_three_groups_renders_the_host_forms_expectation(renderer, cid):
    case = us.BY_ID[cid]
    exp = us.expected(case, "all")
    sa, cam2 = start(renderer, case)
    new, _ = us.scene(cid, "all")
    groups = [to_device(g) for g in us.groups_of(new)]
    renderer.update_spheres_device(0, sa.count, centers=groups[0][1], radii=groups[1][1], materials=groups[2][1])
    device_calls(renderer, case, new, cam2, exp, "device form, all", DEVICE_CASES.index(cid))
    renderer.sync()  # (the device arrays are freed with this frame: nothing may still read them)


# (scene, which sphere): the root leaf exists on the root scenes; `k4`/front/small, 4 + 16 spheres in full pairs, has no odd sphere
DEVICE_DROPS = [(cid, which) for cid in DEVICE_CASES for which in ("root", "odd", "partner")
                if not (which == "root" and cid.startswith("leaf")) and not (which == "odd" and cid == "root-k4-front-small")]


@pytest.mark.parametrize("cid,which", DEVICE_DROPS)
def test_device_form_entry_that_can_never_be_hit_renders_the_scene_without_that_sphere(renderer, cid, which):
    case = us.BY_ID[cid]
    spheres = named_spheres(cid)
    assert which in spheres, (cid, which, spheres)
    sa, cam2 = start(renderer, case)
    gone = us.dropped(sa, spheres[which])
    exp = us.expected_of((cid, "dropped", which), lambda: (gone, cam2, case.seed))
    assert exp.frame0[0] != us.expected(case).frame0[0], "the sphere that goes must show in the frame"
    held, ptrs = to_device(us.groups_of(gone, "radii")[1])
    renderer.update_spheres_device(0, sa.count, radii=ptrs)
    device_calls(renderer, case, gone, cam2, exp, f"inv_radius 0 on {which} sphere {spheres[which]}", DEVICE_CASES.index(cid))
    renderer.sync()


@pytest.mark.parametrize("cid", DEVICE_CASES)
def test_device_form_entry_of_mat_type_7_is_skipped(renderer, cid):
    case = us.BY_ID[cid]
    spheres = named_spheres(cid)
    kept = spheres.get("root", spheres.get("odd"))
    sa, cam2 = start(renderer, case)
    new, _ = us.scene(cid, "materials")
    want = {k: v.copy() for k, v in new.arrays.items()}
    for k in us.MAT_KEYS:
        want[k][kept] = sa.arrays[k][kept]
    want = r1o.SceneArrays(want, sa.camera_array)
    exp = us.expected_of((cid, "mat_type 7"), lambda: (want, cam2, case.seed))
    assert exp.frame0[0] != us.expected(case, "materials").frame0[0], "the kept material must show in the frame"
    given = [v.copy() for v in us.groups_of(new, "materials")[2]]
    given[0][kept] = 7
    held, ptrs = to_device(given)
    renderer.update_spheres_device(0, sa.count, materials=ptrs)
    device_calls(renderer, case, want, cam2, exp, f"mat_type 7 on sphere {kept}", DEVICE_CASES.index(cid))
    renderer.sync()


# ---- e: stream order in every throughput form ----------------------------------------------------------------------------------------------


def enqueue(renderer, sa, cam2, call, seed, hf):
    p = tbe.params(TREE, seed)
    if call in ("async", "pixel"):
        renderer.render_async(p, hf)
    elif call == "batch":
        renderer.render_batch_async(p, 2, hf, seed_stride=us.STRIDE)
    else:
        renderer.render_path_async(p, [es.ccamera(sa.camera_array), es.ccamera(cam2)], hf, seed_stride=us.STRIDE)


def landed(call, hf):
    if call in ("async", "pixel"):
        return [(hf.image.tobytes(), hf.rays)]
    return [(hf.image(f).tobytes(), hf.rays(f)) for f in range(2)]


@pytest.mark.parametrize("kind", ("materials", "radii"))
@pytest.mark.parametrize("call", ("async", "pixel", "batch", "path"))
@pytest.mark.parametrize("cid", ["root-k4-front-small", "root-k4-front-big", "root-wide-front-big", "leaf-n7-small"])
def test_frames_enqueued_before_and_behind_an_update_see_the_old_and_the_new_scene(renderer, cid, call, kind):
    case = us.BY_ID[cid]
    old, new_exp = us.expected(case), us.expected(case, kind)
    sa, cam2 = start(renderer, case)
    make = (lambda: binding.HostFrame(W, H)) if call in ("async", "pixel") else (lambda: binding.HostFrames(W, H, 2))
    fa, fb = make(), make()
    try:
        renderer.set_pixel_mode(call == "pixel")
        enqueue(renderer, sa, cam2, call, case.seed, fa)      # A: the old scene
        new = update(renderer, case, kind)
        enqueue(renderer, new, cam2, call, case.seed, fb)     # B: the new one
        renderer.sync()                                       # one wait for all three
        got_a, got_b = landed(call, fa), landed(call, fb)
    finally:
        renderer.set_pixel_mode(False)
        fa.close(), fb.close()
    want_a, want_b = wanted(old, call), wanted(new_exp, call)
    assert all(a[0] != b[0] for a, b in zip(want_a, want_b)), "the update must show in every frame"
    c = Collector((cid, call, kind))
    c.step("frame A must see the old scene", lambda: tbe.check(renderer, got_a, want_a, TREE, case.size))
    c.step("frame B must see the new scene", lambda: tbe.check(renderer, got_b, want_b, TREE, case.size))
    c.done()


# ---- f: queries ----------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def query_expectation(cid, kind):
    """The frame's own camera rays and stream states — every pixel's first sample, 3 072 rays — and the host forms' answers on the edited
    arrays (tests/test_update_scenes_host.py holds them to the oracle's records on these very rays)."""
    case = us.BY_ID[cid]
    new, _ = us.scene(cid, kind)
    x, y, s = us.camera_samples()
    rays, seeds = binding.camera_rays(es.ccamera(new.camera_array), binding.make_params(W, H, us.CAP, case.seed), x, y, s)
    cs = es.cscene(new)
    return (rays, seeds, binding.cast_rays_host(cs, rays, binding.CAST_CLOSEST), binding.cast_rays_host(cs, rays, binding.CAST_ANY),
            binding.trace_rays_host(cs, rays, seeds, 50))


def check_queries(renderer, c, cid, kind, variants):
    rays, seeds, closest, occluded, radiance = query_expectation(cid, kind)
    for tag, variant in variants:
        c.step(f"{tag} closest", lambda: same_hits(renderer.cast_rays(rays, binding.CAST_CLOSEST, variant), closest, (cid, kind, tag)))
        c.step(f"{tag} any", lambda: same_hits(renderer.cast_rays(rays, binding.CAST_ANY, variant), occluded, (cid, kind, tag, "any")))

        def trace():
            got = renderer.trace_rays(rays, seeds, 50, variant)
            bad = np.nonzero((got.view(np.uint32).reshape(-1, 4) != radiance.view(np.uint32).reshape(-1, 4)).any(1))[0]
            assert bad.size == 0, f"{bad.size} of {len(rays)} records differ from r1_trace_rays_host, first at {bad[:8]}"

        c.step(f"{tag} trace", trace)


@pytest.mark.parametrize("cid", us.IDS)
def test_ray_and_path_queries_after_updates_equal_the_host_forms_on_the_edited_arrays(renderer, cid):
    case = us.BY_ID[cid]
    c = Collector((cid, "queries"))
    start(renderer, case)
    update(renderer, case, "all")
    check_queries(renderer, c, cid, "all", (("tree", TREE), ("reference", REFERENCE)))
    c.step("grid refused", lambda: refused(lambda: renderer.cast_rays(query_expectation(cid, "all")[0][:64], binding.CAST_CLOSEST, GRID), MOVED_RULE))
    start(renderer, case)
    update(renderer, case, "materials")
    check_queries(renderer, c, cid, "materials", (("tree", TREE), ("reference", REFERENCE), ("grid", GRID)))
    c.done()
