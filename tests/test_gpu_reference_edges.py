"""GPU test of the kernels against the REFERENCE on the suite's edge scenes: the small size of every scene of tests/edge_scenes.py,
tests/leaf_scenes.py, tests/root_leaf_scenes.py (both orders) and tests/test_gpu_scatter.py, whose expectations every other GPU module
takes from the CPU oracle.  Here they are tests/golden/ref_*.bin — the frames, records and hit records that the reference's own
Hitable::hit, Material::scatter and color gave on the same arrays (tests/reference_cases.py, oracle/gen_edge_golden.py) — and nothing
calls the oracle: a misreading of the reference that the oracle and the kernels share passes every other module and fails here.
(tests/test_reference_edges_host.py holds the oracle and the host forms to the same files, without a device.)

Per scene, 64 x 48 at 2 samples (the scatter scenes: 4 samples, up to 51 bounces), all exact:
  the synchronous frame with its records through the sweep, the tree, the grid, the reference form, the wavefront variant and the three
  diagnostic builds; r1_render_async into page-locked memory (the tile sum in the kernel, the throughput builds) through the tree, the
  sweep and the grid; a batch of two and a path over the scene's two cameras through the tree; the path query over the frame's own camera
  rays and — for the scenes with a ray set — the ray queries, CLOSEST and ANY, through the tree, the grid and the reference form; then the
  queries again after r1_update_centers with the scene's own centres (an identity move: the tree is refitted and walked by the generic
  walk, without its flat slab), where the grid is refused."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
import reference_cases as rc
from test_trace_rays_host import frame_samples

pytestmark = pytest.mark.gpu

F = np.float32
SYNC = {"sweep": binding.VARIANT_PREFILTER, "tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID, "reference": binding.VARIANT_REFERENCE,
        "wavefront": binding.VARIANT_WAVEFRONT, "sweep_stats": binding.VARIANT_STATS, "tree_stats": binding.VARIANT_BVH_STATS,
        "grid_stats": binding.VARIANT_GRID_STATS}
ASYNC = {"tree": binding.VARIANT_BVH, "sweep": binding.VARIANT_PREFILTER, "grid": binding.VARIANT_GRID}
QUERY = {"tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID, "reference": binding.VARIANT_REFERENCE}


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def params(case, variant, k=0):
    return r1.make_params(rc.W, rc.H, case.spp, case.seed + k * case.stride, max_bounces=case.bounces, variant=variant)


def set_scene(renderer, case):
    sa = rc.scene_of(case, 0)
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    return sa


@pytest.mark.parametrize("build", sorted(SYNC))
@pytest.mark.parametrize("cid", rc.IDS)
def test_synchronous_frame_and_records_are_the_references(renderer, cid, build):
    case = rc.BY_ID[cid]
    g = rc.fixture(case)
    set_scene(renderer, case)
    img, rays, samples = renderer.render_samples(params(case, SYNC[build]))
    rc.assert_frame(g, "", img, rays, f"{cid} main: {build}")
    rc.assert_records(g, samples, f"{cid} main: {build}")
    info = renderer.launch_info()
    assert info["kernel"] == SYNC[build] and info["spheres_active"] <= 1023, info


@pytest.mark.parametrize("family", sorted(ASYNC))
@pytest.mark.parametrize("cid", rc.IDS)
def test_frame_landing_on_the_host_is_the_references(renderer, cid, family):
    case = rc.BY_ID[cid]
    g = rc.fixture(case)
    set_scene(renderer, case)
    hf = binding.HostFrame(rc.W, rc.H)
    try:
        renderer.render_async(params(case, ASYNC[family]), hf)
        renderer.sync()
        rc.assert_frame(g, "", hf.image, hf.rays, f"{cid} main: r1_render_async, {family}")
    finally:
        hf.close()
    assert renderer.launch_info()["kernel"] == ASYNC[family]


@pytest.mark.parametrize("cid", rc.IDS)
def test_batch_and_camera_path_are_the_references(renderer, cid):
    case = rc.BY_ID[cid]
    g = rc.fixture(case)
    sa = set_scene(renderer, case)
    cam2 = case.build()[1]
    p = params(case, binding.VARIANT_BVH)
    hf = binding.HostFrames(rc.W, rc.H, 2)
    try:
        renderer.render_batch_async(p, 2, hf, seed_stride=case.stride)
        renderer.sync()
        rc.assert_frame(g, "", hf.image(0), hf.rays(0), f"{cid} main: batch")
        rc.assert_frame(g, "b1", hf.image(1), hf.rays(1), f"{cid} batch1")
        renderer.render_path_async(p, [es.ccamera(sa.camera_array), es.ccamera(cam2)], hf, seed_stride=case.stride)
        renderer.sync()
        rc.assert_frame(g, "", hf.image(0), hf.rays(0), f"{cid} main: path")
        rc.assert_frame(g, "p1", hf.image(1), hf.rays(1), f"{cid} path1")
    finally:
        hf.close()


def query_all(renderer, case, g, sa, variants, what):
    x, y, s = frame_samples(rc.W, rc.H, case.spp)
    rays, seeds = binding.camera_rays(es.ccamera(sa.camera_array), params(case, 0), x, y, s)
    cast = rc.cast_rays_of(case) if case.cast else None
    for tag, variant in variants.items():
        got = renderer.trace_rays(rays, seeds, case.bounces, variant)
        assert got.dtype == binding.RADIANCE_DTYPE and got.shape == (rc.W * rc.H * case.spp,)
        rc.assert_records(g, got.view(F).reshape(-1, 4), f"{case.id} main: r1_trace_rays, {tag}{what}")
        if cast is not None:
            rc.assert_hits(g, renderer.cast_rays(cast, binding.CAST_CLOSEST, variant), f"{case.id}: r1_cast_rays, {tag}{what}")
            rc.assert_occluded(g, renderer.cast_rays(cast, binding.CAST_ANY, variant), f"{case.id}: r1_cast_rays ANY, {tag}{what}")


@pytest.mark.parametrize("cid", rc.IDS)
def test_queries_are_the_references_before_and_after_an_identity_move(renderer, cid):
    case = rc.BY_ID[cid]
    g = rc.fixture(case)
    sa = set_scene(renderer, case)
    query_all(renderer, case, g, sa, QUERY, "")
    a = sa.arrays
    renderer.update_centers(0, a["center_x"], a["center_y"], a["center_z"])
    try:
        query_all(renderer, case, g, sa, {k: v for k, v in QUERY.items() if k != "grid"}, ", moved")
        x, y, s = frame_samples(rc.W, rc.H, 1)
        rays, seeds = binding.camera_rays(es.ccamera(sa.camera_array), params(case, 0), x[:64], y[:64], s[:64])
        with pytest.raises(binding.R1Error, match="the scene has moved"):
            renderer.trace_rays(rays, seeds, case.bounces, binding.VARIANT_GRID)
        with pytest.raises(binding.R1Error, match="the scene has moved"):
            renderer.cast_rays(rays, binding.CAST_CLOSEST, binding.VARIANT_GRID)
    finally:
        set_scene(renderer, case)  # (a fresh build: the next test's scene does not start from a moved one)
