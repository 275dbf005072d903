"""GPU test of the padded attenuation words (rays1bench_amd/csrc/r1_stack_words.h): the small-scene kernels open a word of
the packed stack with index 1023 in its upper slots, row 1023 of the shade table is {0, 1, 1, 1}, and the unwind folds every word alike.
What could go wrong: a pad missing above a path's top entry (a stale index of an earlier path multiplies in), the quotient or the shift of
a push, the seam between the words in LDS and the entries in the global workspace (entry 30), and a row 1023 that some update overwrites.

  deep        tests/edge_scenes.py's deep-path scene, 64x48x2 at 50 bounces, through every small-scene family — tree TP (r1_render_async),
              LAT (r1_render_samples) and PASS (r1_render_pass), the grid and the sweep, synchronous and in flight — and r1_trace_rays_device
              through the tree, the grid and the reference form: equal to the REFERENCE variant's frame and to tests/golden/ref_edge_deep.bin,
              the reference's own frame and records
  deep_opaque the same spheres with the glass turned Lambertian, so that a path's stack holds exactly its depth: the oracle's records show
              paths ending in the sky with 0, 1 and 2 entries in the top word, with 30 and 31 entries (the last word in LDS full; one entry
              beyond it), and paths ending at max_bounces; the same builds, against the oracle and the REFERENCE variant
  n1023       1023 active spheres on a lattice that the primary rays cover: index 1022 is a sphere, row 1023 is not
  updates     r1_update_spheres and r1_update_spheres_device of every sphere's material on deep_opaque: r1_tables_download and the frames of
              the tree builds equal a fresh context's

Exact everywhere."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import edge_scenes as es
import reference_cases as rc
from test_trace_rays_host import frame_samples

pytestmark = pytest.mark.gpu

F = np.float32
W, H = es.W, es.H
OPAQUE_SPP, OPAQUE_SEED, BOUNCES = 4, 31, 50
LDS_ENTRIES = 30  # R1_STACK_LDS_WORDS (_TP) = 10 words of three entries
SYNC = {"tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID, "sweep": binding.VARIANT_PREFILTER, "reference": binding.VARIANT_REFERENCE}
ASYNC = {"tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID, "sweep": binding.VARIANT_PREFILTER}
QUERY = {"tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID, "reference": binding.VARIANT_REFERENCE}


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def fresh():
    r = r1.Renderer(0)
    yield r
    r.close()


def set_scene(rend, sa):
    rend.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))


def deep_opaque(materials=None):
    sa, _ = es.build("deep", "small")
    arr = {k: v.copy() for k, v in sa.arrays.items()}
    arr["mat_type"][arr["mat_type"] == 2] = 0
    if materials is not None:
        for k, v in zip(("mat_type", "albedo_r", "albedo_g", "albedo_b", "mat_param"), materials):
            arr[k] = v.copy()
    return r1o.SceneArrays(arr, sa.camera_array)


_oracle = {}


def oracle_frame(tag, sa, spp, seed):
    """(image, rays, records (n, 4)) of the CPU oracle; computed once per tag and left unchanged"""
    if tag not in _oracle:
        img, rays, samples = r1o.render_frame(sa, r1o.make_params(W, H, spp, seed, BOUNCES), want_samples=True)
        samples = samples.reshape(-1, 4)
        samples.setflags(write=False)
        _oracle[tag] = (img, rays, samples)
    return _oracle[tag]


def every_build(rend, sa, spp, seed, want, what):
    """the frame (image bytes, rays) — and the records where the route has them — through every small-scene family"""
    img_w, rays_w, rec_w = want
    set_scene(rend, sa)
    for tag, variant in SYNC.items():
        img, rays, samples = rend.render_samples(r1.make_params(W, H, spp, seed, max_bounces=BOUNCES, variant=variant))
        info = rend.launch_info()
        assert info["kernel"] == variant and info["spheres_active"] <= 1023, info
        assert rays == rays_w, f"{what}: synchronous {tag}: {rays} rays, expected {rays_w}"
        assert img.tobytes() == img_w.tobytes(), f"{what}: synchronous {tag}: the frame differs"
        if rec_w is not None:
            a, b = samples.reshape(-1, 4).view(np.uint32), np.asarray(rec_w).view(np.uint32)
            bad = np.nonzero((a != b).any(1))[0]
            assert bad.size == 0, f"{what}: synchronous {tag}: {bad.size} records differ, first at {bad[:8].tolist()}"
    hf = binding.HostFrame(W, H)
    try:
        for tag, variant in ASYNC.items():
            rend.render_async(r1.make_params(W, H, spp, seed, max_bounces=BOUNCES, variant=variant), hf)
            rend.sync()
            assert rend.launch_info()["kernel"] == variant
            assert hf.rays == rays_w, f"{what}: r1_render_async {tag}: {hf.rays} rays, expected {rays_w}"
            assert np.asarray(hf.image).tobytes() == img_w.tobytes(), f"{what}: r1_render_async {tag}: the frame differs"
    finally:
        hf.close()
    for tag in ("tree", "grid", "sweep"):
        img, rays = rend.render_pass(r1.make_params(W, H, spp, seed, max_bounces=BOUNCES, variant=SYNC[tag]), 0)
        assert rays == rays_w and img.tobytes() == img_w.tobytes(), f"{what}: r1_render_pass {tag}: {rays} rays, expected {rays_w}"


def query_device(rend, sa, spp, seed, rec_w, what):
    import torch
    x, y, s = frame_samples(W, H, spp)
    rays, seeds = binding.camera_rays(es.ccamera(sa.camera_array), r1.make_params(W, H, spp, seed, max_bounces=BOUNCES), x, y, s)
    n = rays.shape[0]
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(F).reshape(n, 8).copy()).cuda()
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds).view(np.int32).reshape(n, 4).copy()).cuda()
    want = np.asarray(rec_w).view(np.uint32)
    for tag, variant in QUERY.items():
        d_out = torch.full((n, 4), -1.0, dtype=torch.float32, device="cuda")
        rend.trace_rays_device(d_rays.data_ptr(), d_seeds.data_ptr(), n, d_out.data_ptr(), BOUNCES, variant)
        torch.cuda.synchronize()
        rend.sync()
        got = d_out.cpu().numpy().view(np.uint32)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, f"{what}: r1_trace_rays_device {tag}: {bad.size} records differ, first at {bad[:8].tolist()}"


def test_deep_scene_is_the_references_through_every_small_scene_family(renderer):
    case = rc.BY_ID["edge-deep"]
    g = rc.fixture(case)
    sa = rc.scene_of(case, 0)
    assert (case.spp, case.bounces) == (es.SPP, BOUNCES)
    set_scene(renderer, sa)
    img, rays, samples = renderer.render_samples(r1.make_params(W, H, case.spp, case.seed, max_bounces=BOUNCES, variant=binding.VARIANT_REFERENCE))
    rc.assert_frame(g, "", img, rays, "deep: the REFERENCE variant")
    rc.assert_records(g, samples, "deep: the REFERENCE variant")
    assert int(samples.reshape(-1, 4).view(np.uint32)[:, 3].max()) > LDS_ENTRIES + 2  # paths deeper than the words in LDS
    every_build(renderer, sa, case.spp, case.seed, (img, rays, samples.reshape(-1, 4)), "deep")
    query_device(renderer, sa, case.spp, case.seed, samples.reshape(-1, 4), "deep")


def stack_depths(records):
    """deep_opaque: every scatter pushes, so a path that ended in the sky (radiance not all zero: the sky is at least 0.5) had rays - 1
    entries on its stack; a black path ended at Metal's refusal or at max_bounces"""
    rec = np.asarray(records)
    rays = rec.view(np.uint32)[:, 3].astype(np.int64)
    sky = (rec[:, :3] != 0).any(1)
    return rays[sky] - 1, rays[~sky]


def test_deep_opaque_paths_end_in_every_slot_at_the_seam_and_at_the_bounce_limit(renderer):
    sa = deep_opaque()
    img, rays, rec = oracle_frame("opaque", sa, OPAQUE_SPP, OPAQUE_SEED)
    depths, black = stack_depths(rec)
    hist = np.bincount(depths, minlength=BOUNCES + 2)
    print("stack entries of the paths that end in the sky:", hist.tolist())
    for residue in (0, 1, 2):
        assert hist[1:][(np.arange(1, hist.size) % 3) == residue].sum() > 0, residue  # the top word holds 3, 1, 2 entries
    assert hist[LDS_ENTRIES] > 0 and hist[LDS_ENTRIES + 1] > 0 and hist[LDS_ENTRIES - 1] > 0, hist[LDS_ENTRIES - 1:LDS_ENTRIES + 2]
    assert hist[LDS_ENTRIES + 2:].sum() > 0
    assert (black == BOUNCES + 1).sum() > 0  # paths that end at max_bounces: no unwind, whatever their stack holds
    set_scene(renderer, sa)
    ref = renderer.render_samples(r1.make_params(W, H, OPAQUE_SPP, OPAQUE_SEED, max_bounces=BOUNCES, variant=binding.VARIANT_REFERENCE))
    assert ref[1] == rays and ref[0].tobytes() == img.tobytes()
    assert ref[2].reshape(-1, 4).view(np.uint32).tobytes() == np.asarray(rec).view(np.uint32).tobytes()
    every_build(renderer, sa, OPAQUE_SPP, OPAQUE_SEED, (img, rays, rec), "deep_opaque")
    query_device(renderer, sa, OPAQUE_SPP, OPAQUE_SEED, rec, "deep_opaque")


def lattice_1023():
    """1023 spheres of radius 0.4 on a 33 x 31 lattice in the plane z = 0, random opaque and glass materials, seen from the front by a camera
    whose 64 x 48 primary rays cover the lattice"""
    rng = np.random.default_rng(1023)
    ij = np.stack(np.meshgrid(np.arange(33), np.arange(31), indexing="ij"), -1).reshape(-1, 2)
    c = np.zeros((1023, 3))
    c[:, 0], c[:, 1] = (ij[:, 0] - 16) * 1.0, (ij[:, 1] - 15) * 1.0
    c[:, 2] = rng.uniform(-0.3, 0.3, 1023)
    arr = es.spheres(c, np.full(1023, 0.4), rng)
    lookfrom, lookat = np.array([0.0, 0.0, 34.0]), np.array([0.0, 0.0, 0.0])
    cam = es.look(lookfrom, lookat, 50.0, W / H, 0.0, 34.0)
    return r1o.SceneArrays(es.pad8(arr), np.asarray(cam, F))


def test_a_scene_of_exactly_1023_spheres_uses_index_1022_and_not_row_1023(renderer):
    sa = lattice_1023()
    assert es.active(sa) == 1023
    hits = binding.cast_rays_host(es.cscene(sa), es.primary_rays(sa.camera_array))
    seen = np.unique(hits["index"][hits["index"] >= 0])
    assert seen.size > 900, seen.size  # the primary rays alone reach nearly every sphere, whichever of them the tree numbers 1022
    img, rays, rec = oracle_frame("n1023", sa, 2, 77)
    set_scene(renderer, sa)
    every_build(renderer, sa, 2, 77, (img, rays, rec), "n1023")
    assert renderer.tables_download()["shade"].shape == (1023, 4)


def tables_equal(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("form", ["host", "device"])
def test_material_updates_of_every_sphere_leave_the_identity_row(renderer, fresh, form):
    base = deep_opaque()
    n = len(base.arrays["center_x"])
    rng = np.random.default_rng(5)
    mt = base.arrays["mat_type"].copy()
    on = mt != 255
    mt[on] = rng.integers(0, 2, int(on.sum())).astype(np.uint8)  # opaque still: Lambertian or Metal
    mt[:2] = 0
    mats = (mt, rng.uniform(0.5, 0.99, n).astype(F), rng.uniform(0.5, 0.99, n).astype(F), rng.uniform(0.5, 0.99, n).astype(F),
            rng.uniform(0.0, 0.3, n).astype(F))
    set_scene(renderer, base)
    if form == "host":
        renderer.update_spheres(0, materials=mats)
    else:
        import torch
        t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in mats]
        renderer.update_spheres_device(0, n, materials=tuple(v.data_ptr() for v in t))
        renderer.sync()
    edited = deep_opaque(mats)
    set_scene(fresh, edited)
    tables_equal(renderer.tables_download(), fresh.tables_download(), form)
    p = r1.make_params(W, H, 2, 911, max_bounces=BOUNCES, variant=binding.VARIANT_BVH)
    want = fresh.render(p)[:2]
    assert int(want[1]) > 2 * W * H * 5  # deep paths still
    got = renderer.render(p)[:2]
    assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes(), (form, "synchronous", got[1], want[1])
    hf = binding.HostFrame(W, H)
    try:
        renderer.render_async(p, hf)
        renderer.sync()
        assert hf.rays == want[1] and np.asarray(hf.image).tobytes() == want[0].tobytes(), (form, "in flight", hf.rays, want[1])
    finally:
        hf.close()
    img, rays, _ = oracle_frame("edited", edited, 2, 911)
    assert rays == want[1] and img.tobytes() == want[0].tobytes()
