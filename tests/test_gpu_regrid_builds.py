"""GPU test of the REGRIDDED grid in every call and on the edge scenes, as tests/test_gpu_update_builds.py is for updated
scenes and tests/test_gpu_resort_builds.py for re-sorted ones, and with their helpers: after r1_set_scene(original), one update and r1_regrid,
every render and query through R1_VARIANT_GRID gives what the CPU ORACLE gives for the edited arrays — bytes, records, ray counts and the
bits of the linear frame — and r1_grid_download returns r1_grid_regrid_describe's tables byte for byte.  tests/test_gpu_regrid.py holds a
regridded context to a fresh one through the synchronous frame, one r1_render_async pair and the queries, on the library's own scenes; here
the throughput kernels, the PIXEL build (always the big-scene kernel and the 32-bit table), batches, paths, passes, the adaptive kernel,
device shards and linear frames run on it, over tests/regrid_scenes.py: a cluster 8e4 units out, a camera inside a sphere, the corridor
between two r = 1000 spheres, coincident spheres, radii of 2e-3 600 units away, flat grids.

The calls of a case ("every call"): the eight of tests/test_gpu_builds_edges.py through GRID (sync with records, async, pixel, batch, path,
pass, adaptive with the rule off and on); sync with records through GRID_STATS; r1_render_linear and r1_render_linear_async against
linear_cases.linear_of on the oracle's records (a NaN for a NaN) with the ray count; two device shards + r1_assemble_device against frame 0.

  a. RUN_IDS (11 of the 15 scenes of regrid_scenes.MATRIX_IDS) x move, radii, all: the grid built by a render before the update in half of the
     cases, by r1_regrid in the others.
  b. the form flip, `edge-far-small` (all) and limit_scene("under") (lift): at most 1023 spheres whose table fits the small-scene kernel's
     LDS at the build and whose capacity (twice the build's registrations + 64) does not, so the scene runs the big-scene grid kernel from its
     first regrid on.  Every call before the first regrid and after it; after r1_set_scene of the same scene the small form is back.
     launch_info does not show small against big (as it does not for `noise` in tests/test_gpu_builds_edges.py):
     tests/test_regrid_scenes_host.py::test_the_first_regrid_moves_the_scene_to_the_big_form pins the precondition from r1_scene_grid.cpp's
     rule, and that is the evidence that both forms ran.
  c. overflow in every call: `large` + collapse (small form) and grid 40 x 30 + collapse (big form): v2 = -1 sends every ray of every mode
     to the tree fallback, over a tree that was itself refitted; r1_grid_download reports -1; then the original centres, a regrid and one
     call against the unmoved frame.
  d. stream order: call, update, regrid, the same call, ONE wait, for async, pixel, batch, path and the linear async form; once with the
     scene's first regrid inside the sequence (it waits for the device itself) and once with a regrid before frame A (nothing waits).
  e. three rounds on one context without r1_set_scene: edit(seed 41, 42, 43) of the original, regrid, one call each; then r1_resort_spheres,
     regrid and one call.
  f. the device forms: r1_update_spheres_device with all three groups, and an inv_radius 0 entry on a registered sphere against the oracle on
     dropped(); then regrid; sync, pixel, batch and the adaptive call.
  g. r1_cast_rays (closest, any) and r1_trace_rays through GRID over the frame's camera rays after `all` + regrid on all 43 scenes of
     tests/update_scenes.py against the host forms on the edited arrays (tests/test_gpu_update_builds.py (f) asserts that without a regrid
     the grid is refused there).

Thinned for time, along scenes alone — no call and no edit is left out anywhere: (a) leaves out the big sizes of `deep`, `far`, `noise_lds` and
`palette`, and (d) runs on `edge-far-small` and `edge-palette-small` without `edge-deep-big`: the oracle's deep paths among 1 100 spheres and
the scene's set-up cost 0.1 to 0.4 s a case.  `edge-deep-big` stays in (e), (f) and (g), the other three in (g); of the scenes past 1023
spheres (a) keeps `inside`, `coincident` and `wide`, and (d)'s frames behind `edge-far-small`'s first regrid run the big form.  The bound is
this module's wall time against tests/test_gpu_builds_edges.py's in one session; DESIGN.md §4.31 has the figures.

One case collects the steps that differ and fails once; the order of a case's calls rotates from case to case, so that each call is also
the first one behind a regrid.  Frames are 64 x 48 at 2 samples, the adaptive call at its cap of 6.  Nothing here has a tolerance and no GPU
render is an expectation."""
import functools

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
import linear_cases as lc
import regrid_scenes as rgs
import update_scenes as us
import test_gpu_builds_edges as tbe
from test_gpu_builds_edges import renderer  # noqa: F401  (the module-scoped fixture)
from test_gpu_regrid import tables_equal
from test_gpu_update_builds import Collector, check_queries, one_call, rotated, to_device, wanted

pytestmark = pytest.mark.gpu

W, H, SPP = us.W, us.H, us.SPP
GRID, GRID_STATS = binding.VARIANT_GRID, binding.VARIANT_GRID_STATS
CALLS = tbe.CALLS
EVERY = tuple(f"grid {call}" for call in CALLS) + ("grid_stats sync", "linear", "linear async", "two shards")
IDS = rgs.MATRIX_IDS + list(rgs.PRODUCT)
# (a): 11 of the 15 matrix scenes (the module's docstring says which went and why)
RUN_IDS = [cid for cid in rgs.MATRIX_IDS if cid not in ("edge-deep-big", "edge-far-big", "edge-noise_lds-big", "edge-palette-big")]
assert len(RUN_IDS) == 11


# ---- the steps of a case ------------------------------------------------------------------------------------------------------------------


def device_error_ends_the_run(test):
    """Collector.step's rule for the calls between the steps (r1_set_scene, the update, r1_regrid): an error of the device or the runtime
    ends the whole run, and nothing more is started on the device."""
    @functools.wraps(test)
    def guarded(*args, **kwargs):
        try:
            return test(*args, **kwargs)
        except binding.R1Error as e:
            if e.code in (binding.R1_EHIP, binding.R1_ENOMEM, binding.R1_ENODEVICE):
                pytest.exit(f"{test.__name__}: {e} — a device error: nothing more is run", returncode=3)
            raise
    return guarded


def start(renderer, cid):
    """r1_set_scene with the ORIGINAL arrays"""
    sa, cam2 = rgs.scene(cid)
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    return sa, cam2


def plan(renderer, cid, by_render):
    """The grid of the original scene, which a later regrid keeps the plan of: built by a render through it, or by r1_regrid"""
    if by_render:
        sa, cam2 = rgs.scene(cid)
        case = rgs.case_of(cid)
        tbe.check(renderer, tbe.run(renderer, sa, cam2, "sync", GRID, case.seed), [rgs.expected(cid).frame0], GRID, case.size)
    else:
        renderer.regrid()


def update(renderer, cid, kind):
    """ONE update call: r1_update_centers for a move, r1_update_spheres with the groups that changed for the others"""
    new, _ = rgs.scene(cid, kind)
    centers, radii, materials = us.groups_of(new, "move" if cid in rgs.PRODUCT else kind)
    if radii is None and materials is None:
        renderer.update_centers(0, *centers)
    else:
        renderer.update_spheres(0, centers=centers, radii=radii, materials=materials)
    return new


def by_render_of(cid, k=0):
    return (IDS.index(cid) + k) % 2 == 1


def same_linear(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{int(bad.sum())} values of the linear frame differ from the oracle's sums, first at {np.argwhere(bad)[:3].tolist()}"


def linear_call(renderer, case, exp, in_flight):
    p = tbe.params(GRID, case.seed)
    if in_flight:
        lf = binding.LinearHostFrame(W, H)
        try:
            renderer.render_linear_async(p, lf.ptr, lf.rays_ptr)
            renderer.sync()
            got, rays = lf.image.copy(), lf.rays
        finally:
            lf.close()
    else:
        got, rays, _ = renderer.render_linear(p)
    print(f"linear: {rays} rays, the oracle counts {exp.frame0[1]}")
    assert rays == exp.frame0[1], f"{rays} rays, the oracle counts {exp.frame0[1]}"
    same_linear(got, lc.linear_of(exp.main, SPP))
    assert renderer.launch_info()["kernel"] == GRID


def shards_call(renderer, case, exp):
    """two device shards on the context's stream, r1_assemble_device, one wait"""
    import torch
    shards = 2
    p = [r1.make_params(W, H, SPP, case.seed, tile_w=32, tile_h=32, shard=s, num_shards=shards, variant=GRID) for s in range(shards)]
    nbytes = binding.shard_block_bytes(p[0])
    assert nbytes == binding.shard_block_bytes(p[1])
    blocks = torch.zeros((shards, nbytes), dtype=torch.uint8, device="cuda")
    rays = torch.zeros(shards, dtype=torch.int64, device="cuda")
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    for s in range(shards):
        renderer.render_shard_device(p[s], blocks[s].data_ptr(), rays[s:].data_ptr())
    renderer.assemble_device(p[0], blocks.data_ptr(), out.data_ptr())
    renderer.sync()
    tbe.check(renderer, [(out.cpu().numpy().tobytes(), int(rays.sum().item()))], [exp.frame0], GRID, case.size)


def step_of(renderer, cid, sa, cam2, exp, tag):
    case = rgs.case_of(cid)
    if tag.startswith("grid "):
        return lambda: one_call(renderer, case, sa, cam2, exp, tag[5:], GRID)
    if tag == "grid_stats sync":
        return lambda: one_call(renderer, case, sa, cam2, exp, "sync", GRID_STATS)
    if tag.startswith("linear"):
        return lambda: linear_call(renderer, case, exp, tag == "linear async")
    assert tag == "two shards"
    return lambda: shards_call(renderer, case, exp)


def every_call(renderer, c, cid, sa, cam2, exp, k, prefix=""):
    """EVERY, rotated by k; the rule-on adaptive call where the restated rule on the oracle's records stops tiles at different counts
    (tests/test_regrid_scenes_host.py names the frames on which it does not)"""
    tags = [t for t in EVERY if t != "grid adaptive" or rgs.rule_shows(exp)]
    for tag in rotated(tags, k):
        c.step(prefix + tag, step_of(renderer, cid, sa, cam2, exp, tag))


def tables_step(renderer, c, cid, kind, what="the device's tables"):
    c.step(what, lambda: tables_equal(renderer.grid_download(), rgs.tables(cid, kind)[1], (cid, kind)))


# ---- a: the matrix ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", rgs.KINDS)
@pytest.mark.parametrize("cid", RUN_IDS)
@device_error_ends_the_run
def test_every_call_through_the_regridded_grid_renders_the_oracles_frames(renderer, cid, kind):
    k = rgs.KINDS.index(kind)
    exp = rgs.expected(cid, kind)
    _, cam2 = start(renderer, cid)
    plan(renderer, cid, by_render_of(cid, k))
    new = update(renderer, cid, kind)
    renderer.regrid()
    c = Collector((cid, kind))
    tables_step(renderer, c, cid, kind)
    every_call(renderer, c, cid, new, cam2, exp, IDS.index(cid) * 3 + k)
    c.done()


# ---- b: the form flip ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cid,kind", rgs.FLIP, ids=lambda v: str(v))
@device_error_ends_the_run
def test_every_call_before_and_after_the_regrid_that_moves_the_scene_to_the_big_form(renderer, cid, kind):
    """(the docstring of the module, b: launch_info cannot show which form ran; the host file's precondition is the evidence)"""
    k = IDS.index(cid)
    old, exp = rgs.expected(cid), rgs.expected(cid, kind)
    sa, cam2 = start(renderer, cid)
    c = Collector((cid, kind, "form flip"))
    every_call(renderer, c, cid, sa, cam2, old, k, "small form, ")
    c.step("the build's tables", lambda: tables_equal(renderer.grid_download(), rgs.tables(cid, kind)[0], (cid, "build")))
    new = update(renderer, cid, kind)
    renderer.regrid()
    tables_step(renderer, c, cid, kind)
    every_call(renderer, c, cid, new, cam2, exp, k + 5, "big form, ")
    start(renderer, cid)
    for tag in rotated(EVERY, k + 1)[:2]:
        c.step("after r1_set_scene, " + tag, step_of(renderer, cid, sa, cam2, old, tag))
    c.done()


# ---- c: overflow --------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cid", ["large-collapse", "grid40x30-collapse"])
@device_error_ends_the_run
def test_every_call_through_an_overflowed_grid_and_back(renderer, cid):
    k = IDS.index(cid)
    old, exp = rgs.expected(cid), rgs.expected(cid, "x")
    sa, cam2 = start(renderer, cid)
    plan(renderer, cid, by_render_of(cid))
    new = update(renderer, cid, "x")
    renderer.regrid()
    c = Collector((cid, "overflow"))

    def overflowed():
        got = renderer.grid_download()
        assert got[0]["registrations"] == -1 and not got[1].any() and len(got[2]) == 0
        tables_equal(got, rgs.tables(cid, "x")[1], (cid, "overflow"))

    c.step("the device's tables", overflowed)
    every_call(renderer, c, cid, new, cam2, exp, k)
    renderer.update_centers(0, *us.groups_of(sa, "move")[0])
    renderer.regrid()
    c.step("back: the build's tables", lambda: tables_equal(renderer.grid_download(), rgs.tables(cid, "x")[0], (cid, "back")))
    tag = rotated(EVERY, k + 3)[0]
    c.step("back: " + tag, step_of(renderer, cid, sa, cam2, old, tag))
    c.done()


# ---- d: stream order ----------------------------------------------------------------------------------------------------------------------

ORDER_CALLS = ("async", "pixel", "batch", "path", "linear")


def enqueue(renderer, sa, cam2, call, seed, target):
    p = tbe.params(GRID, seed)
    if call in ("async", "pixel"):
        renderer.render_async(p, target)
    elif call == "batch":
        renderer.render_batch_async(p, 2, target, seed_stride=us.STRIDE)
    elif call == "path":
        renderer.render_path_async(p, [es.ccamera(sa.camera_array), es.ccamera(cam2)], target, seed_stride=us.STRIDE)
    else:
        renderer.render_linear_async(p, target.ptr, target.rays_ptr)


def target_of(call):
    if call == "linear":
        return binding.LinearHostFrame(W, H)
    return binding.HostFrame(W, H) if call in ("async", "pixel") else binding.HostFrames(W, H, 2)


def check_landed(renderer, case, call, target, exp):
    if call == "linear":
        assert target.rays == exp.frame0[1], f"{target.rays} rays, the oracle counts {exp.frame0[1]}"
        same_linear(target.image, lc.linear_of(exp.main, SPP))
        return
    got = [(target.image.tobytes(), target.rays)] if call in ("async", "pixel") else [(target.image(f).tobytes(), target.rays(f)) for f in range(2)]
    tbe.check(renderer, got, wanted(exp, call), GRID, case.size)


@pytest.mark.parametrize("first_inside", (True, False), ids=("first-regrid-inside", "regrid-before"))
@pytest.mark.parametrize("call", ORDER_CALLS)
@pytest.mark.parametrize("cid", ["edge-far-small", "edge-palette-small"])
@device_error_ends_the_run
def test_frames_enqueued_before_and_behind_an_update_and_a_regrid_see_the_old_and_the_new_grid(renderer, cid, call, first_inside):
    case = us.BY_ID[cid]
    kind = "all"
    old, new_exp = rgs.expected(cid), rgs.expected(cid, kind)
    assert all(a[0] != b[0] for a, b in zip(wanted(old, call), wanted(new_exp, call))), "the update must show in every frame"
    sa, cam2 = start(renderer, cid)
    if not first_inside:
        renderer.regrid()  # the scene's first: the tables at their capacity, the scratch laid out; the next one waits for nothing
    fa, fb = target_of(call), target_of(call)
    try:
        renderer.set_pixel_mode(call == "pixel")
        enqueue(renderer, sa, cam2, call, case.seed, fa)      # A: the old scene (first_inside: through the grid the launch builds)
        new = update(renderer, cid, kind)
        renderer.regrid()
        enqueue(renderer, new, cam2, call, case.seed, fb)     # B: the new one
        renderer.sync()                                       # one wait for all four
        c = Collector((cid, call, "first regrid inside" if first_inside else "regrid before"))
        c.step("frame A must see the old scene", lambda: check_landed(renderer, case, call, fa, old))
        c.step("frame B must see the new scene", lambda: check_landed(renderer, case, call, fb, new_exp))
    finally:
        renderer.set_pixel_mode(False)
        fa.close(), fb.close()
    tables_step(renderer, c, cid, kind, "the device's tables after both frames")
    c.done()


# ---- e: three rounds on one context -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cid", rgs.ROUND_IDS)
@device_error_ends_the_run
def test_three_rounds_of_update_and_regrid_and_a_resort_on_one_context(renderer, cid):
    k = IDS.index(cid)
    sa, cam2 = start(renderer, cid)
    cs = es.cscene(sa)
    plan(renderer, cid, by_render_of(cid))
    c = Collector((cid, "rounds"))
    for n, seed in enumerate(rgs.ROUND_SEEDS):
        new, exp = rgs.round_scene(cid, seed), rgs.round_expected(cid, seed)
        centers, radii, materials = us.groups_of(new)
        renderer.update_spheres(0, centers=centers, radii=radii, materials=materials)
        renderer.regrid()
        want = binding.regrid_describe(cs, *rgs.regrid_arrays(new))
        c.step(f"round {n}: the device's tables", lambda: tables_equal(renderer.grid_download(), want, (cid, seed)))
        tag = rotated(EVERY, k + 5 * n)[0]
        c.step(f"round {n}: {tag}", step_of(renderer, cid, new, cam2, exp, tag))
    renderer.resort_spheres()
    renderer.regrid()
    c.step("re-sort: the device's tables", lambda: tables_equal(renderer.grid_download(), want, (cid, "re-sort")))
    tag = rotated(EVERY, k + 2)[0]
    c.step(f"re-sort: {tag}", step_of(renderer, cid, new, cam2, exp, tag))
    c.done()


# ---- f: the device forms ------------------------------------------------------------------------------------------------------------------

DEVICE_CALLS = ("sync", "pixel", "batch", "adaptive_off")


def device_calls(renderer, c, cid, sa, cam2, exp, k):
    for call in rotated(DEVICE_CALLS, k):
        c.step(f"grid {call}", step_of(renderer, cid, sa, cam2, exp, f"grid {call}"))


@pytest.mark.parametrize("cid", rgs.DEVICE_IDS)
@device_error_ends_the_run
def test_device_form_of_all_three_groups_then_a_regrid(renderer, cid):
    k = rgs.DEVICE_IDS.index(cid)
    exp = us.expected(cid, "all")
    sa, cam2 = start(renderer, cid)
    plan(renderer, cid, by_render_of(cid, 1))
    new, _ = us.scene(cid, "all")
    groups = [to_device(g) for g in us.groups_of(new)]
    renderer.update_spheres_device(0, sa.count, centers=groups[0][1], radii=groups[1][1], materials=groups[2][1])
    renderer.regrid()
    c = Collector((cid, "device form, all"))
    tables_step(renderer, c, cid, "all")
    device_calls(renderer, c, cid, new, cam2, exp, k)
    renderer.sync()  # (the device arrays are freed with this case: nothing may still read them)
    c.done()


@pytest.mark.parametrize("cid", rgs.DEVICE_IDS)
@device_error_ends_the_run
def test_device_form_entry_that_can_never_be_hit_then_a_regrid(renderer, cid):
    k = rgs.DEVICE_IDS.index(cid)
    sphere = rgs.dropped_sphere(cid)
    sa, cam2 = start(renderer, cid)
    gone = us.dropped(sa, sphere)
    exp = rgs.dropped_expected(cid)
    assert exp.frame0[0] != us.expected(cid).frame0[0], "the sphere that goes must show in the frame"
    plan(renderer, cid, by_render_of(cid))
    held, ptrs = to_device(us.groups_of(gone, "radii")[1])
    renderer.update_spheres_device(0, sa.count, radii=ptrs)
    renderer.regrid()
    c = Collector((cid, f"inv_radius 0 on sphere {sphere}"))
    want = binding.regrid_describe(es.cscene(sa), *rgs.regrid_arrays(gone))

    assert want[0]["registrations"] < rgs.tables(cid, "all")[0][0]["registrations"]  # (its ball of radius 0 overlaps fewer cells)
    c.step("the device's tables", lambda: tables_equal(renderer.grid_download(), want, (cid, "dropped")))
    device_calls(renderer, c, cid, gone, cam2, exp, k + 1)
    renderer.sync()
    c.done()


# ---- g: queries ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cid", us.IDS)
@device_error_ends_the_run
def test_ray_and_path_queries_through_the_regridded_grid_equal_the_host_forms(renderer, cid):
    start(renderer, cid)
    renderer.regrid()
    update(renderer, cid, "all")
    renderer.regrid()
    c = Collector((cid, "queries"))
    check_queries(renderer, c, cid, "all", (("grid", GRID),))
    c.done()
