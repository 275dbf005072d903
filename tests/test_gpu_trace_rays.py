"""GPU tests of the path queries (r1_trace_rays / r1_trace_rays_device): the path-query kernels (r1_query_kernels.hip)
against the reference's own color() through tests/golden/samples_*.bin, against r1_render_samples for whole frames, and against
r1_trace_rays_host — which tests/test_trace_rays_host.py pins to the same fixtures and to the oracle — everywhere else.  The box tree, the
uniform grid and the reference form must return the same bytes.  Every comparison is exact: bytes of r, g, b and equality of rays.
No ray with a zero stream state is sent to the device by any test: the substitution is r1_seed_guard, which the CPU tests cover — a
broken guard would show as a hang, not as a failed assert."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_cast_host import cscene
from test_gpu_cast import ray_mix
from test_refit_host import moved_centres, raw_from_arrays
from test_trace_rays_host import SAMPLE_FIXTURES, assert_records, ccam, fixture_rays, frame_samples

pytestmark = pytest.mark.gpu

F = np.float32
DEFAULT, REFERENCE, BVH, GRID = binding.VARIANT_DEFAULT, binding.VARIANT_REFERENCE, binding.VARIANT_BVH, binding.VARIANT_GRID
ACCEPTED = (DEFAULT, BVH, GRID, REFERENCE)
CHUNK = binding.TRACE_CHUNK
MOVED_RULE = "the scene has moved"


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def same(got, want, what):
    assert got.dtype == want.dtype == binding.RADIANCE_DTYPE and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.unique(np.nonzero(got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4))[0])
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} records differ, first at {bad[:8]}: {got[bad[:3]]} != {want[bad[:3]]}")


def random_seeds(rng, n):
    """four non-zero stream states per ray"""
    return rng.integers(1, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)


@pytest.fixture(scope="module")
def fixtures():
    """the four sample fixtures as rays and stream states, computed once"""
    return {file: fixture_rays(scene, file) for scene, file in SAMPLE_FIXTURES}


# ---- 4: the reference's fixtures on the device -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene,file", SAMPLE_FIXTURES)
def test_trace_equals_the_reference_fixture(renderer, fixtures, scene, file):
    """every sample of the fixture through every accepted variant (small-scene kernels, paths 51 deep)"""
    sa, rays, seeds, g = fixtures[file]
    renderer.set_scene_raw(cscene(sa), ccam(sa))
    for variant in ACCEPTED:
        assert_records(renderer.trace_rays(rays, seeds, 50, variant), g["rgb"], g["rays"], (file, variant))


# ---- 5: whole frames -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,w,h,spp", (("medium", 77, 45, 3), ("large", 80, 60, 4)))
def test_camera_rays_traced_equal_render_samples(renderer, name, w, h, spp):
    sc = {"medium": r1.create_medium_scene, "large": r1.create_large_scene}[name](w, h)
    renderer.set_scene(sc)
    p = r1.make_params(w, h, spp, 4242)
    _, total, rec = renderer.render_samples(p)
    x, y, s = frame_samples(w, h, spp)
    rays, seeds = binding.camera_rays(sc.camera.contents, p, x, y, s)
    for variant in (BVH, GRID):
        got = renderer.trace_rays(rays, seeds, 50, variant)
        assert_records(got, rec[:, :3], np.ascontiguousarray(rec[:, 3]).view(np.uint32), (name, variant))
        assert int(got["rays"].astype(np.uint64).sum()) == total
    # in another order: a record belongs to its ray
    perm = np.random.default_rng(3).permutation(len(x))
    got = renderer.trace_rays(rays[perm], seeds[perm], 50, BVH)
    assert_records(got, rec[perm, :3], np.ascontiguousarray(rec[perm, 3]).view(np.uint32), (name, "permuted"))
    sc.close()


# ---- 6: big-scene kernels ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("grid_wh,pad_local", (((40, 30), 0), ((160, 100), 1)))
def test_big_scenes(renderer, grid_wh, pad_local):
    """Scenes beyond the small-scene kernels' limits, one tree padded from the centre and one per node: 4099 seeded rays of the ray
    queries' class mix (camera rays, origins in the volume, 2e4 .. 1e5 away — the grid's fallback —, inside spheres, scatter rays,
    axis-parallel and grazing directions), all four variants against the host form"""
    sc = r1.create_grid_scene(1920, 1080, *grid_wh)
    info = binding.bvh_describe(sc.spheres.contents)[0]
    assert info["pad_local"] == pad_local and info["spheres"] > 1023, info
    renderer.set_scene(sc)
    cs = sc.spheres.contents
    n = 4099
    rays = ray_mix(sc.arrays(), sc.camera_array(), n, 41, lambda r: binding.cast_rays_host(cs, r))
    seeds = random_seeds(np.random.default_rng(42), n)
    want = binding.trace_rays_host(cs, rays, seeds, 50)
    assert (want["rays"] >= 3).mean() > 0.1 and (want["rays"] == 1).any() and want["rays"].max() >= 8
    for variant in ACCEPTED:
        same(renderer.trace_rays(rays, seeds, 50, variant), want, (grid_wh, variant))
    sc.close()


def test_sizes_on_the_large_scene(renderer, fixtures):
    sa, rays, seeds, g = fixtures[SAMPLE_FIXTURES[2][1]]
    renderer.set_scene_raw(cscene(sa), ccam(sa))
    for variant in (BVH, GRID, REFERENCE):
        for n in (1, 63, 64, 65):
            assert_records(renderer.trace_rays(rays[:n], seeds[:n], 50, variant), g["rgb"][:3 * n], g["rays"][:n], (variant, n))
    assert renderer.trace_rays(rays[:0], seeds[:0]).shape == (0,)
    assert binding.lib().r1_trace_rays(renderer._c, 0, 50, None, None, 0, None) == binding.R1_OK
    assert binding.lib().r1_trace_rays_device(renderer._c, 0, 50, None, None, 0, None, None) == binding.R1_OK


# ---- 7: other bounce limits, NULL seeds ----------------------------------------------------------------------------------------------------


def test_bounce_limits_and_null_seeds_on_the_deep_scene(renderer):
    import edge_scenes as es
    sa, _ = es.build("deep", "small")
    renderer.set_scene_raw(cscene(sa), es.ccamera(sa.camera_array))
    x, y, s = frame_samples(es.W, es.H, 2)
    rays, seeds = binding.camera_rays(es.ccamera(sa.camera_array), binding.make_params(es.W, es.H, 2, es.SEED["deep"]), x, y, s)
    deep = binding.trace_rays_host(cscene(sa), rays, seeds, 51)
    assert deep["rays"].max() >= 31
    for mb in (1, 2, 51):
        want = deep if mb == 51 else binding.trace_rays_host(cscene(sa), rays, seeds, mb)
        assert want["rays"].max() <= mb + 1
        for variant in (BVH, GRID, REFERENCE):
            same(renderer.trace_rays(rays, seeds, mb, variant), want, (mb, variant))
    want = binding.trace_rays_host(cscene(sa), rays, None, 50)
    for variant in (BVH, REFERENCE):
        same(renderer.trace_rays(rays, None, 50, variant), want, ("NULL seeds", variant))


# ---- 8: chunking ---------------------------------------------------------------------------------------------------------------------------


def test_the_host_memory_form_works_in_chunks(renderer, fixtures):
    """2^20 + 77 rays on the small scene: the second chunk's records follow the first's, with explicit seeds and with NULL seeds (ray i
    of the CALL is seeded with pixel i)"""
    sa, rays, seeds, g = fixtures[SAMPLE_FIXTURES[0][1]]
    renderer.set_scene_raw(cscene(sa), ccam(sa))
    n = CHUNK + 77
    idx = np.arange(n) % len(rays)
    big_rays, big_seeds = np.ascontiguousarray(rays[idx]), np.ascontiguousarray(seeds[idx])
    big_rays["o"][:, 0] += (np.arange(n) % 5).astype(F) * F(0.0625)  # (not all copies alike)
    same(renderer.trace_rays(big_rays, big_seeds, 50, BVH), binding.trace_rays_host(cscene(sa), big_rays, big_seeds, 50), "chunks")
    same(renderer.trace_rays(big_rays, None, 50, GRID), binding.trace_rays_host(cscene(sa), big_rays, None, 50), "chunks, NULL seeds")


# ---- 9: the device form --------------------------------------------------------------------------------------------------------------------


def test_device_form_on_a_torch_stream(renderer, fixtures):
    """Torch tensors on a non-default stream, two traces back to back (tree, then the grid without seeds), one wait"""
    import torch
    sa, rays, seeds, g = fixtures[SAMPLE_FIXTURES[1][1]]
    renderer.set_scene_raw(cscene(sa), ccam(sa))
    n = len(rays)
    want_null = binding.trace_rays_host(cscene(sa), rays, None, 50)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays.view(F).reshape(-1, 8).copy()).cuda()
        d_seeds = torch.from_numpy(seeds.view(np.int32).reshape(-1, 4).copy()).cuda()
        d_a = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        d_b = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        st.synchronize()
        renderer.trace_rays_device(d_rays.data_ptr(), d_seeds.data_ptr(), n, d_a.data_ptr(), 50, BVH, st.cuda_stream)
        renderer.trace_rays_device(d_rays.data_ptr(), None, n, d_b.data_ptr(), 50, GRID, st.cuda_stream)
        st.synchronize()
    assert_records(d_a.cpu().numpy().view(binding.RADIANCE_DTYPE).reshape(-1), g["rgb"], g["rays"], "device form")
    same(d_b.cpu().numpy().view(binding.RADIANCE_DTYPE).reshape(-1), want_null, "device form, NULL seeds")
    # misaligned or NULL device pointers are refused
    E, L = binding.R1_EINVAL, binding.lib()
    pr, ps, po = d_rays.data_ptr(), d_seeds.data_ptr(), d_a.data_ptr()
    assert L.r1_trace_rays_device(renderer._c, 0, 50, C.c_void_p(pr + 4), C.c_void_p(ps), n - 1, C.c_void_p(po), None) == E
    assert L.r1_trace_rays_device(renderer._c, 0, 50, C.c_void_p(pr), C.c_void_p(ps + 8), n - 1, C.c_void_p(po), None) == E
    assert L.r1_trace_rays_device(renderer._c, 0, 50, C.c_void_p(pr), C.c_void_p(ps), n - 1, C.c_void_p(po + 4), None) == E
    assert L.r1_trace_rays_device(renderer._c, 0, 50, None, C.c_void_p(ps), n, C.c_void_p(po), None) == E
    assert L.r1_trace_rays_device(renderer._c, 0, 50, C.c_void_p(pr), C.c_void_p(ps), n, None, None) == E


# ---- 10: moved scenes ----------------------------------------------------------------------------------------------------------------------


def test_traces_after_an_update_see_the_moved_scene(renderer):
    w, h, spp = 80, 60, 2
    sc = r1.create_large_scene(w, h)
    a = sc.arrays()
    x, y, z = moved_centres(a, "lift")
    renderer.set_scene(sc)
    renderer.update_centers(0, x, y, z)
    cs, keep = raw_from_arrays(a, x, y, z)
    px, py, ps = frame_samples(w, h, spp)
    rays, seeds = binding.camera_rays(sc.camera.contents, r1.make_params(w, h, spp, 99), px, py, ps)
    fresh = r1.Renderer(0)
    try:
        fresh.set_scene_raw(cs, sc.camera.contents)
        want = fresh.trace_rays(rays, seeds, 50, BVH)
    finally:
        fresh.close()
    same(want, binding.trace_rays_host(cs, rays, seeds, 50), "fresh context, moved arrays")
    assert want.tobytes() != binding.trace_rays_host(sc.spheres.contents, rays, seeds, 50).tobytes()  # (the move shows)
    for variant in (DEFAULT, REFERENCE):
        same(renderer.trace_rays(rays, seeds, 50, variant), want, ("moved", variant))
    with pytest.raises(binding.R1Error) as e:
        renderer.trace_rays(rays, seeds, 50, GRID)
    assert e.value.code == binding.R1_EINVAL and MOVED_RULE in str(e.value)
    renderer.set_scene(sc)  # (rebuilds everything: the next test finds an un-moved context)
    sc.close()


# ---- 11: state -----------------------------------------------------------------------------------------------------------------------------


def test_traces_disturb_no_render(renderer, fixtures):
    """r1_render before and after a trace: identical bytes and ray count, launch info and timing still the render's; a progressive
    accumulation interrupted by traces continues and ends equal to r1_render at the full spp"""
    w, h = 160, 96
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    _, rays, seeds, _ = fixtures[SAMPLE_FIXTURES[2][1]]
    rays, seeds = rays[:2048], seeds[:2048]
    for variant in (BVH, GRID):
        p = r1.make_params(w, h, 6, 77, variant=variant)
        img0, n0 = renderer.render(p)[:2]
        info0, timing0 = renderer.launch_info(), renderer.last_timing()
        a = renderer.trace_rays(rays, seeds, 50, BVH)
        b = renderer.trace_rays(rays, seeds, 50, GRID)
        assert renderer.launch_info() == info0 and renderer.last_timing() == timing0
        assert a.tobytes() == b.tobytes()
        img1, n1 = renderer.render(p)[:2]
        assert img0.tobytes() == img1.tobytes() and n0 == n1
        renderer.render_pass(r1.make_params(w, h, 2, 77, variant=variant), 0)
        renderer.trace_rays(rays, seeds, 50, GRID)
        renderer.render_pass(r1.make_params(w, h, 3, 77, variant=variant), 2)
        renderer.trace_rays(rays, None, 7, REFERENCE)
        imgp, np_ = renderer.render_pass(r1.make_params(w, h, 1, 77, variant=variant), 5)[:2]
        assert imgp.tobytes() == img0.tobytes() and np_ == n0
    sc.close()


def test_refusals_leave_the_next_trace_correct(renderer, fixtures):
    sa, rays, seeds, g = fixtures[SAMPLE_FIXTURES[1][1]]
    renderer.set_scene_raw(cscene(sa), ccam(sa))
    L, E = binding.lib(), binding.R1_EINVAL
    n = 256
    out = np.zeros(n, binding.RADIANCE_DTYPE)
    args = (rays.ctypes.data, seeds.ctypes.data, n, out.ctypes.data)
    for variant in (binding.VARIANT_PREFILTER, binding.VARIANT_STATS, binding.VARIANT_BVH_STATS, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID_STATS, 9, -1):
        assert L.r1_trace_rays(renderer._c, variant, 50, *args) == E
        assert str(variant).encode() in L.r1_last_error()
    for mb in (0, 52, -3):
        assert L.r1_trace_rays(renderer._c, 0, mb, *args) == E and b"max_bounces" in L.r1_last_error()
    assert L.r1_trace_rays(renderer._c, 0, 50, None, seeds.ctypes.data, n, out.ctypes.data) == E
    assert L.r1_trace_rays(renderer._c, 0, 50, rays.ctypes.data, seeds.ctypes.data, n, None) == E
    assert not out.view(np.uint8).any()
    assert_records(renderer.trace_rays(rays[:n], seeds[:n], 50, BVH), g["rgb"][:3 * n], g["rays"][:n], "after refusals")
    fresh = r1.Renderer(0)
    try:
        assert L.r1_trace_rays(fresh._c, 0, 50, *args) == E and b"scene" in L.r1_last_error()
        assert L.r1_trace_rays_device(fresh._c, 0, 50, C.c_void_p(256), None, 4, C.c_void_p(512), None) == E and b"scene" in L.r1_last_error()
    finally:
        fresh.close()


def test_a_scene_without_an_active_sphere_gives_the_sky(renderer, fixtures):
    sa, rays, seeds, _ = fixtures[SAMPLE_FIXTURES[0][1]]
    arrays = {k: v.copy() for k, v in sa.arrays.items()}
    arrays["inv_radius"][:] = 0
    import r1o
    empty = r1o.SceneArrays(arrays, sa.camera_array)
    renderer.set_scene_raw(cscene(empty), ccam(empty))
    want = binding.trace_rays_host(cscene(empty), rays[:1000], seeds[:1000], 50)
    assert (want["rays"] == 1).all() and (want["b"] > 0.99).all()
    for variant in ACCEPTED:
        same(renderer.trace_rays(rays[:1000], seeds[:1000], 50, variant), want, ("sky", variant))


# ---- 12: the panorama's rays ---------------------------------------------------------------------------------------------------------------


def test_equirectangular_rays_poles_included(renderer):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import panorama
    sc = r1.create_large_scene(1200, 800)
    renderer.set_scene(sc)
    w, h, spp = 64, 32, 2
    rays, seeds = panorama.equirect_rays(sc.camera_array()[0:3], w, h, spp, 7)
    assert (rays[:w * spp, 4:7] == np.array([0, -1, 0], F)).all() and (rays[-w * spp:, 4:7] == np.array([0, 1, 0], F)).all()
    want = binding.trace_rays_host(sc.spheres.contents, rays, seeds, 50)
    assert (want["rays"][:w * spp] >= 2).all() and (want["rays"][-w * spp:] == 1).all()  # down: the ground; up: the sky
    for variant in (BVH, GRID, REFERENCE):
        same(renderer.trace_rays(rays, seeds, 50, variant), want, ("panorama", variant))
    img = panorama.resolve(want, w, h, spp)
    assert img.shape == (h, w, 3) and img[-1].min() > 100
    sc.close()
