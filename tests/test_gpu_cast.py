"""GPU tests of the ray queries (r1_cast_rays / r1_cast_rays_device): the cast kernels (r1_query_kernels.hip) against the
reference's own Hitable::hit through tests/golden/cast_*.bin, and against r1_cast_rays_host — which tests/test_cast_host.py pins to the
same fixtures — on large seeded ray sets.  The box tree, the uniform grid and the reference form must return the same bytes.  Every
comparison is exact: the contract is bit identity."""
import ctypes as C

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_cast_host import FLT_MAX, assert_equals_fixture, cscene, fixture, scene_of

pytestmark = pytest.mark.gpu

F = np.float32
DEFAULT, REFERENCE, BVH, GRID = binding.VARIANT_DEFAULT, binding.VARIANT_REFERENCE, binding.VARIANT_BVH, binding.VARIANT_GRID
ACCEPTED = (DEFAULT, BVH, GRID, REFERENCE)
CLOSEST, ANY = binding.CAST_CLOSEST, binding.CAST_ANY
CHUNK = binding.CAST_CHUNK


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def set_golden_scene(renderer, name):
    sa = scene_of(name)
    renderer.set_scene_raw(cscene(sa), C.cast(C.pointer(sa.camera), C.POINTER(binding.CCamera)).contents)
    return sa


def unit_ball(rng, n):
    out = np.empty((0, 3))
    while out.shape[0] < n:
        v = rng.uniform(-1.0, 1.0, (2 * n + 8, 3))
        out = np.concatenate([out, v[(v * v).sum(1) < 1.0]])
    return out[:n]


def unit_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def pack(o, d):
    r = np.zeros((o.shape[0], 8), F)
    r[:, 0:3], r[:, 3], r[:, 4:7] = o.astype(F), FLT_MAX, d.astype(F)
    return r


def ray_mix(arrays, cam, n, seed, host):
    """n seeded rays in the fixtures' class mix (tools/gen_cast_golden.py: camera, volume with far origins, scatter from hit points, axis-
    parallel, grazing, bounded t_max), in the fixtures' proportions; `host(rays)` answers the rays the scatter and bounded classes build on."""
    rng = np.random.default_rng(seed)
    cx, cy, cz = (arrays[k].astype(np.float64) for k in ("center_x", "center_y", "center_z"))
    rad = np.sqrt(np.maximum(arrays["radius_sq"].astype(np.float64), 0.0))
    real = (arrays["inv_radius"] != 0) & np.isfinite(arrays["center_x"])
    field = real & (rad < 100.0)
    c = np.stack([cx, cy, cz], 1)
    lo, hi = c[field].min(0), c[field].max(0)
    size = np.maximum(hi - lo, 1.0)
    glo, ghi = lo - 0.5 * size, hi + 0.5 * size
    q = n // 16  # camera 4, volume 4, scatter 4, axis 2, grazing 1, bounded 1 sixteenths
    # camera: jittered primary rays
    u, v = rng.random(4 * q).astype(F), rng.random(4 * q).astype(F)
    cam = cam.astype(F)
    d = cam[3:6][None, :] + u[:, None] * cam[6:9][None, :] + v[:, None] * cam[9:12][None, :] - cam[0:3][None, :]
    camera = pack(np.repeat(cam[0:3][None, :], 4 * q, 0), d)
    # volume
    o, d = rng.uniform(glo, ghi, (4 * q, 3)), unit_dirs(rng, 4 * q)
    far = max(4 * q // 16, 1)
    o[:far] = 0.5 * (lo + hi) + unit_dirs(rng, far) * rng.uniform(2.0e4, 1.0e5, (far, 1))
    d[:far] = rng.uniform(lo, hi, (far, 3)) - o[:far]
    ins = rng.choice(np.nonzero(field)[0], far)
    o[far:2 * far] = c[ins] + 0.5 * rad[ins][:, None] * unit_ball(rng, far)
    volume = pack(o, d)
    # scatter
    first = np.concatenate([camera, volume])
    h = host(first)
    hit = np.nonzero(h["index"] >= 0)[0]
    pick = rng.choice(hit, 4 * q)
    scatter = pack(h["p"][pick], h["n"][pick].astype(np.float64) + unit_ball(rng, 4 * q))
    # axis-parallel
    o = np.round(rng.uniform(glo, ghi, (2 * q, 3)) * 2.0) / 2.0
    d = rng.uniform(-1.0, 1.0, (2 * q, 3))
    d[np.abs(d) < 0.05] = 0.5
    two = rng.integers(0, 2, 2 * q) == 1
    ax0 = rng.integers(0, 3, 2 * q)
    ax1 = (ax0 + 1 + rng.integers(0, 2, 2 * q)) % 3
    rows = np.arange(2 * q)
    d[rows, ax0] = np.where(rng.integers(0, 2, 2 * q) == 1, -0.0, 0.0)
    d[rows[two], ax1[two]] = np.where(rng.integers(0, 2, int(two.sum())) == 1, -0.0, 0.0)
    axis = pack(o, d)
    # grazing
    sph = rng.choice(np.nonzero(real)[0], q)
    o = rng.uniform(glo, ghi, (q, 3))
    o[:, 1] = rng.uniform(3.0, 10.0, q)
    w = c[sph] - o
    L = np.linalg.norm(w, axis=1)
    r = rad[sph]
    inside = L <= 1.05 * r
    o[inside] = c[sph][inside] - (w[inside] / L[inside][:, None]) * 3.0 * r[inside][:, None]
    w = c[sph] - o
    L = np.linalg.norm(w, axis=1)
    w /= L[:, None]
    perp = np.cross(w, unit_dirs(rng, q))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    s = 1.0 + np.where(rng.integers(0, 2, q) == 1, 1.0, -1.0) * 2.0 ** (-rng.integers(8, 23, q).astype(np.float64))
    tangent = c[sph] - w * (r * r / L)[:, None] + perp * (r * np.sqrt(1.0 - (r / L) ** 2) * s)[:, None]
    uu = (tangent - o) / np.linalg.norm(tangent - o, axis=1, keepdims=True)
    low = (np.arange(q) % 2 == 1)[:, None]
    start = np.where(low, tangent + uu * (0.5 * np.minimum(r, 1.0))[:, None], o)
    grazing = pack(start, np.where(low, o - start, tangent - o))
    # bounded
    free = np.concatenate([camera, volume, scatter, axis, grazing])
    rest = n - free.shape[0]
    cand = np.concatenate([np.arange(8 * q), 12 * q + np.arange(3 * q)])  # (camera, volume, axis, grazing: answered below; scatter is not needed)
    cand = rng.choice(cand, min(cand.size, 4 * rest), replace=False)
    hb = host(free[cand])
    hit = np.nonzero(hb["index"] >= 0)[0]
    pick = rng.choice(hit, rest, replace=hit.size < rest)
    bounded = free[cand[pick]].copy()
    t = hb["t"][pick]
    forms = np.stack([t, np.nextafter(t, F(0)), np.nextafter(t, FLT_MAX), t / F(2), np.full(rest, F(0.001)), np.full(rest, np.nextafter(F(0.001), F(1))),
                      np.full(rest, F(0.0011)), np.full(rest, F(0)), np.full(rest, np.inf, F), np.full(rest, np.nan, F)])
    bounded[:, 3] = forms[np.arange(rest) % forms.shape[0], np.arange(rest)]
    return np.ascontiguousarray(np.concatenate([free, bounded]).astype(F))


def same_hits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.tobytes() != b.tobytes():
        bad = np.nonzero(a != b)[0] if a.dtype == np.uint8 else np.nonzero((a["index"] != b["index"]) | (a["t"].view(np.uint32) != b["t"].view(np.uint32)))[0]
        raise AssertionError(f"{what}: {bad.size} of {a.shape[0]} rays differ, first at {bad[:8]}: {a[bad[:3]]} != {b[bad[:3]]}")


@pytest.mark.parametrize("variant", ACCEPTED)
@pytest.mark.parametrize("name", ("small", "medium", "large"))
def test_cast_equals_the_reference_fixture(renderer, name, variant):
    """index, t, p and n of all 4096 fixture rays, bitwise, through every accepted variant; ANY bytes equal index >= 0."""
    set_golden_scene(renderer, name)
    rays, g = fixture(name)
    hits = renderer.cast_rays(rays, CLOSEST, variant)
    assert_equals_fixture(hits, g, (name, variant))
    occ = renderer.cast_rays(rays, ANY, variant)
    assert occ.dtype == np.uint8 and occ.tobytes() == (g["index"] != 0xFFFFFFFF).astype(np.uint8).tobytes()


def test_a_million_rays_on_the_large_scene(renderer):
    """2^20 seeded rays of the fixtures' class mix: tree = grid = reference form = r1_cast_rays_host, byte for byte, both modes."""
    sc = r1.create_large_scene(1200, 800)
    renderer.set_scene(sc)
    cs = sc.spheres.contents
    rays = ray_mix(sc.arrays(), sc.camera_array(), 1 << 20, 31, lambda r: binding.cast_rays_host(cs, r))
    want = binding.cast_rays_host(cs, rays)
    frac = float((want["index"] >= 0).mean())
    assert 0.2 < frac < 0.8, frac
    want_any = (want["index"] >= 0).astype(np.uint8)
    for variant in (BVH, GRID, REFERENCE):
        same_hits(renderer.cast_rays(rays, CLOSEST, variant), want, ("large", variant))
        same_hits(renderer.cast_rays(rays, ANY, variant), want_any, ("large any", variant))


@pytest.mark.parametrize("grid_wh,n", (((50, 32), 1 << 18), ((400, 250), 1 << 16)))
def test_big_scenes(renderer, grid_wh, n):
    """Scenes beyond the small-scene kernels' limits (1 604 spheres; config 5's 100 004): the big-scene tree and grid casts and the
    reference form against the exhaustive host form (config 5: 2^16 rays x 100 004 spheres, well under a minute on 16 host threads)."""
    sc = r1.create_grid_scene(1920, 1080, *grid_wh)
    renderer.set_scene(sc)
    cs = sc.spheres.contents
    rays = ray_mix(sc.arrays(), sc.camera_array(), n, 37, lambda r: binding.cast_rays_host(cs, r))
    want = binding.cast_rays_host(cs, rays)
    assert 0.2 < float((want["index"] >= 0).mean()) < 0.8
    for variant in (BVH, GRID, REFERENCE):
        same_hits(renderer.cast_rays(rays, CLOSEST, variant), want, (grid_wh, variant))
    same_hits(renderer.cast_rays(rays, ANY, BVH), (want["index"] >= 0).astype(np.uint8), (grid_wh, "any"))


def test_sizes_and_ray_order(renderer):
    """n = 1, 63, 64, 65, the host form's chunk size - 1, + 0, + 1 and 2 x + 1: every ray answered, in ray order (a ray's answer does not
    depend on its neighbours, so a prefix of the rays gets a prefix of the answers); n = 0 touches nothing."""
    sa = set_golden_scene(renderer, "large")
    base, _ = fixture("large")
    reps = (2 * CHUNK + 1 + 4095) // 4096
    rays = np.ascontiguousarray(np.tile(base, (reps, 1))[:2 * CHUNK + 1])
    rays[:, 0] += (np.arange(rays.shape[0]) % 7).astype(F) * F(0.125)  # (not all copies alike)
    want = binding.cast_rays_host(cscene(sa), rays)
    for variant in (BVH, GRID):
        for n in (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
            same_hits(renderer.cast_rays(rays[:n], CLOSEST, variant), want[:n], (variant, n))
        for n in (1, 65, CHUNK + 1):
            same_hits(renderer.cast_rays(rays[:n], ANY, variant), (want[:n]["index"] >= 0).astype(np.uint8), (variant, n, "any"))
    assert renderer.cast_rays(rays[:0]).shape == (0,)
    assert binding.lib().r1_cast_rays(renderer._c, 0, 0, None, 0, None) == binding.R1_OK
    assert binding.lib().r1_cast_rays_device(renderer._c, 0, 0, None, 0, None, None) == binding.R1_OK


def test_device_form_on_a_torch_stream(renderer):
    """Torch tensors on a non-default stream, two casts back to back (CLOSEST then ANY, then the grid), nothing waited for in between."""
    import torch
    sa = set_golden_scene(renderer, "medium")
    base, _ = fixture("medium")
    rays = np.ascontiguousarray(np.tile(base, (40, 1)))
    want = binding.cast_rays_host(cscene(sa), rays)
    n = rays.shape[0]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays).cuda(non_blocking=False)
        d_hits = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        d_hits2 = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        d_any = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st.synchronize()
        renderer.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), CLOSEST, BVH, st.cuda_stream)
        renderer.cast_rays_device(d_rays.data_ptr(), n, d_any.data_ptr(), ANY, BVH, st.cuda_stream)
        renderer.cast_rays_device(d_rays.data_ptr(), n, d_hits2.data_ptr(), CLOSEST, GRID, st.cuda_stream)
        st.synchronize()
    assert d_hits.cpu().numpy().tobytes() == want.tobytes()
    assert d_hits2.cpu().numpy().tobytes() == want.tobytes()
    assert d_any.cpu().numpy().tobytes() == (want["index"] >= 0).astype(np.uint8).tobytes()
    # misaligned or NULL device pointers are refused
    E = binding.R1_EINVAL
    L = binding.lib()
    assert L.r1_cast_rays_device(renderer._c, 0, 0, C.c_void_p(d_rays.data_ptr() + 4), n - 1, C.c_void_p(d_hits.data_ptr()), None) == E
    assert L.r1_cast_rays_device(renderer._c, 0, 0, C.c_void_p(d_rays.data_ptr()), n - 1, C.c_void_p(d_hits.data_ptr() + 8), None) == E
    assert L.r1_cast_rays_device(renderer._c, 0, 0, None, n, C.c_void_p(d_hits.data_ptr()), None) == E
    assert L.r1_cast_rays_device(renderer._c, 0, 0, C.c_void_p(d_rays.data_ptr()), n, None, None) == E


def test_a_cast_sees_the_scene_not_the_camera(renderer):
    sa = set_golden_scene(renderer, "small")
    rs, gs = fixture("small")
    assert_equals_fixture(renderer.cast_rays(rs, CLOSEST, GRID), gs, "small")
    set_golden_scene(renderer, "large")
    rl, gl = fixture("large")
    for variant in (BVH, GRID, REFERENCE):
        assert_equals_fixture(renderer.cast_rays(rl, CLOSEST, variant), gl, ("large after small", variant))
    other = scene_of("medium")
    renderer.set_camera(C.cast(C.pointer(other.camera), C.POINTER(binding.CCamera)).contents)
    for variant in (BVH, GRID):
        assert_equals_fixture(renderer.cast_rays(rl, CLOSEST, variant), gl, ("after set_camera", variant))


def test_casts_disturb_no_render(renderer):
    """r1_render before and after a cast: identical bytes and ray count, and the launch info still describes the render; a progressive
    accumulation interrupted by casts continues and ends equal to r1_render at the full spp."""
    w, h = 160, 96
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    rays, _ = fixture("large")
    for variant in (BVH, GRID):
        p = r1.make_params(w, h, 6, 77, variant=variant)
        img0, n0 = renderer.render(p)[:2]
        info0, timing0 = renderer.launch_info(), renderer.last_timing()
        a = renderer.cast_rays(rays, CLOSEST, BVH)
        b = renderer.cast_rays(rays, ANY, GRID)
        assert renderer.launch_info() == info0 and renderer.last_timing() == timing0
        img1, n1 = renderer.render(p)[:2]
        assert img0.tobytes() == img1.tobytes() and n0 == n1
        assert b.tobytes() == (a["index"] >= 0).astype(np.uint8).tobytes()
        # progressive: 2 + 3 + 1 samples with casts in between
        renderer.render_pass(r1.make_params(w, h, 2, 77, variant=variant), 0)
        renderer.cast_rays(rays, CLOSEST, GRID)
        renderer.render_pass(r1.make_params(w, h, 3, 77, variant=variant), 2)
        renderer.cast_rays(rays, ANY, REFERENCE)
        imgp, np_ = renderer.render_pass(r1.make_params(w, h, 1, 77, variant=variant), 5)[:2]
        assert imgp.tobytes() == img0.tobytes() and np_ == n0


def test_refusals_leave_the_next_cast_correct(renderer):
    sa = set_golden_scene(renderer, "medium")
    rays, g = fixture("medium")
    L = binding.lib()
    out = np.zeros(rays.shape[0], binding.HIT_DTYPE)
    E = binding.R1_EINVAL
    for variant in (binding.VARIANT_PREFILTER, binding.VARIANT_STATS, binding.VARIANT_BVH_STATS, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID_STATS, 9, -1):
        assert L.r1_cast_rays(renderer._c, variant, 0, rays.ctypes.data, rays.shape[0], out.ctypes.data) == E
        assert str(variant).encode() in L.r1_last_error()
        assert not out.view(np.uint8).any()
    for mode in (2, -1):
        assert L.r1_cast_rays(renderer._c, 0, mode, rays.ctypes.data, rays.shape[0], out.ctypes.data) == E
    assert L.r1_cast_rays(renderer._c, 0, 0, None, 4, out.ctypes.data) == E
    assert L.r1_cast_rays(renderer._c, 0, 0, rays.ctypes.data, 4, None) == E
    assert_equals_fixture(renderer.cast_rays(rays, CLOSEST, BVH), g, "after refusals")
    # before the first r1_set_scene
    fresh = r1.Renderer(0)
    try:
        assert L.r1_cast_rays(fresh._c, 0, 0, rays.ctypes.data, 4, out.ctypes.data) == E and b"scene" in L.r1_last_error()
        assert L.r1_cast_rays_device(fresh._c, 0, 0, C.c_void_p(256), 4, C.c_void_p(512), None) == E
    finally:
        fresh.close()
