"""GPU tests of the BASELINE.json configurations at their FULL sizes, and of the adversarial
scene families VERDICT r01 names (run on the MI355X box: pytest -m gpu).

  config 2/3  medium / large 1200x800x10        -> tests/test_gpu_parity.py (fixtures) + 8-shard reassembly here
  config 4    large 1200x800x250 (8 shards)     -> a 96x64x250 frame bit-equal to the oracle through both kernel
                                                   families and through 8 shards; the full frame by properties
                                                   (run-to-run identical, sum of sample rays = count, rays per
                                                   sample, 8-shard union = unsharded) + oracle spot samples
  config 5    100 004 spheres 1920x1080x64      -> the full frame through the box tree by the same properties
                                                   + 200 oracle spot samples (brute force over all spheres)

Everything goes through the C-ABI of librays1.so.  Tolerance: bit-exact (see tests/test_gpu_parity.py
for the one documented deviation, powf(x, 5), which has never been observed to flip a sample).
Sizes: the two full-size sample downloads are 3.8 GB (config 4) and 2.1 GB (config 5) of host memory.
"""
import ctypes as C

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

pytestmark = pytest.mark.gpu

FAMILIES = [binding.VARIANT_DEFAULT, binding.VARIANT_PREFILTER]
FAMILY_IDS = ["default", "sweep"]


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


def oracle_scene(sc):
    return r1o.SceneArrays.from_c(sc.spheres, sc.camera)


def oparams(p):
    return r1o.make_params(p.width, p.height, p.spp, p.seed, p.max_bounces, p.tile_w, p.tile_h, p.shard, p.num_shards)


def rays_of(samples):
    return samples[:, 3].copy().view(np.uint32)


def union_of_shards(renderer, w, h, spp, seed, shards, variant):
    acc = np.zeros((h, w, 3), np.uint8)
    covered = np.zeros((h, w), bool)
    total = 0
    for s in range(shards):
        part = np.zeros((h, w, 3), np.uint8)
        rays, _ = renderer.render_into(r1.make_params(w, h, spp, seed, shard=s, num_shards=shards, variant=variant), part)
        ty, tx = np.meshgrid(np.arange(h) // 32, np.arange(w) // 32, indexing="ij")
        mine = (ty * ((w + 31) // 32) + tx) % shards == s
        assert not part[~mine].any()          # a shard writes its own tiles only
        assert not (covered & mine).any()
        acc[mine] = part[mine]
        covered |= mine
        total += rays
    assert covered.all()
    return acc, total


# ---- config 4: 250 spp ---------------------------------------------------------------------------


@pytest.mark.parametrize("variant", FAMILIES, ids=FAMILY_IDS)
def test_config4_250spp_small_frame_bit_equal_to_oracle_and_through_8_shards(renderer, variant):
    """common.h:25-27 is where 250 comes from (NUM_SAMPLES_PER_PIXEL = 10 * 25 for the threaded build)."""
    w, h, spp, seed = 96, 64, 250, 10001
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    p = r1.make_params(w, h, spp, seed, variant=variant)
    img, rays, samples = renderer.render_samples(p)
    oimg, orays, osamples = r1o.render_frame(oracle_scene(sc), oparams(p), want_samples=True)
    assert rays == orays
    assert samples.tobytes() == osamples.tobytes()
    assert img.tobytes() == oimg.tobytes()
    acc, total = union_of_shards(renderer, w, h, spp, seed, 8, variant)
    assert total == rays and acc.tobytes() == img.tobytes()


def test_config4_full_size_1200x800x250_properties_and_oracle_spots(renderer):
    w, h, spp, seed = 1200, 800, 250, 10001
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    p = r1.make_params(w, h, spp, seed)
    img, rays, samples = renderer.render_samples(p)            # 240 M records, 3.8 GB
    sr = rays_of(samples)
    assert int(sr.sum(dtype=np.uint64)) == rays                # sum of sample rays = the count the kernel accumulated
    assert sr.min() >= 1 and sr.max() <= 51
    assert abs(rays / (w * h * spp) - 2.81) < 0.02             # 2.81 rays per sample on the large scene
    assert np.isfinite(samples[:, :3]).all() and samples[:, :3].min() >= 0 and samples[:, :3].max() <= 1
    # the pixels are the in-order sums of these samples (rayweek1.cpp:757-775), checked on a strip of rows
    rows = slice(390, 398)
    col = np.zeros((8, w, 3), np.float32)
    view = samples.reshape(h, w, spp, 4)[rows]
    for s in range(spp):
        col += view[:, :, s, :3]
    col = np.sqrt(col * np.float32(1.0 / spp))
    assert ((col * np.float32(255.99)).astype(np.int32).astype(np.uint8) == img[rows]).all()
    # oracle: 1500 random samples + every sample of a 6x4 pixel block
    rng = np.random.default_rng(4)
    xs, ys, ss = rng.integers(0, w, 1500), rng.integers(0, h, 1500), rng.integers(0, spp, 1500)
    bx, by, bs = np.meshgrid(np.arange(600, 606), np.arange(300, 304), np.arange(spp), indexing="ij")
    xs, ys, ss = np.concatenate([xs, bx.ravel()]), np.concatenate([ys, by.ravel()]), np.concatenate([ss, bs.ravel()])
    rgb, orays = r1o.trace_samples(oracle_scene(sc), w, h, seed, xs, ys, ss)
    got = samples[(ys.astype(np.int64) * w + xs) * spp + ss]
    del samples, view
    assert (rays_of(got) == orays).all()
    assert got[:, :3].tobytes() == rgb.tobytes()
    # run-to-run identical; 8-shard union = the unsharded frame (the decomposition of BASELINE config 4)
    img2, rays2, _ = renderer.render(p)
    assert rays2 == rays and img2.tobytes() == img.tobytes()
    acc, total = union_of_shards(renderer, w, h, spp, seed, 8, binding.VARIANT_DEFAULT)
    assert total == rays and acc.tobytes() == img.tobytes()
    # and the exhaustive sweep gives the same frame
    img3, rays3, _ = renderer.render(r1.make_params(w, h, spp, seed, variant=binding.VARIANT_PREFILTER))
    assert rays3 == rays and img3.tobytes() == img.tobytes()
    # the same frame through the throughput entry point (ONE launch: the trace kernel sums its own tiles, DESIGN.md §4.10 — at 250 spp
    # a wave takes ~50 chunks of ~3 000 samples: the chunk size follows the length of the wave's list of tiles), twice in a row
    hf = binding.HostFrames(w, h, 1)
    for _ in range(2):
        hf._all[:] = 0x5A
        renderer.render_async(p, hf)
        renderer.sync()
        assert hf.rays(0) == rays and hf.image(0).tobytes() == img.tobytes()
    hf.close()


# ---- configs 2/3 at full size through 8 shards --------------------------------------------------


@pytest.mark.parametrize("name", ["medium", "large"])
@pytest.mark.parametrize("variant", FAMILIES, ids=FAMILY_IDS)
def test_1200x800x10_eight_shard_reassembly(renderer, name, variant):
    w, h, spp, seed = 1200, 800, 10, 10001
    sc = {"medium": r1.create_medium_scene, "large": r1.create_large_scene}[name](w, h)
    renderer.set_scene(sc)
    img, rays, _ = renderer.render(r1.make_params(w, h, spp, seed, variant=variant))
    acc, total = union_of_shards(renderer, w, h, spp, seed, 8, variant)
    assert total == rays and acc.tobytes() == img.tobytes()


def test_1200x800x10_eight_shards_device_resident_gather_layout(renderer):
    """The same reassembly through the entry points bench.py's N-GPU path uses: eight device-resident
    records (tile block + ray count) -> strided assemble, all on one GPU."""
    torch = pytest.importorskip("torch")
    from rays1bench_amd import sharding
    w, h, spp, seed, shards = 1200, 800, 10, 10001, 8
    renderer.set_scene(r1.create_large_scene(w, h))
    img, rays, _ = renderer.render(r1.make_params(w, h, spp, seed))
    nbytes = binding.shard_block_bytes(r1.make_params(w, h, spp, seed, shard=0, num_shards=shards))
    rec = nbytes + sharding.RECORD_TRAILER
    records = torch.zeros((shards, rec), dtype=torch.uint8, device="cuda")
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for s in range(shards):
        renderer.render_shard_device(r1.make_params(w, h, spp, seed, shard=s, num_shards=shards), records[s].data_ptr(),
                                     records[s].data_ptr() + nbytes, stream)
    renderer.assemble_device_strided(r1.make_params(w, h, spp, seed, shard=0, num_shards=shards), records.data_ptr(), rec, out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == img.tobytes()
    assert sharding.total_rays(records.view(-1), shards) == rays


# ---- config 5: 100 004 spheres at 1920x1080x64 -----------------------------------------------------


def test_config5_full_size_through_the_tree_properties_and_oracle_spots(renderer):
    w, h, spp, seed = 1920, 1080, 64, 10001
    sc = r1.create_grid_scene(w, h, 400, 250)
    assert int((sc.arrays()["inv_radius"] != 0).sum()) == 100004
    renderer.set_scene(sc)
    p = r1.make_params(w, h, spp, seed)
    img, rays, samples = renderer.render_samples(p)            # 132.7 M records, 2.1 GB
    assert renderer.launch_info()["kernel"] == binding.VARIANT_BVH
    sr = rays_of(samples)
    assert int(sr.sum(dtype=np.uint64)) == rays
    assert sr.min() >= 1 and sr.max() <= 51
    assert 1.5 < rays / (w * h * spp) < 4.0
    assert np.isfinite(samples[:, :3]).all() and samples[:, :3].min() >= 0 and samples[:, :3].max() <= 1
    rng = np.random.default_rng(5)
    xs, ys, ss = rng.integers(0, w, 200), rng.integers(0, h, 200), rng.integers(0, spp, 200)
    rgb, orays = r1o.trace_samples(oracle_scene(sc), w, h, seed, xs, ys, ss)  # brute force over all 100 004 spheres
    got = samples[(ys.astype(np.int64) * w + xs) * spp + ss]
    del samples
    assert (rays_of(got) == orays).all()
    assert got[:, :3].tobytes() == rgb.tobytes()
    assert orays.max() > 2                                      # the spots include real bounce chains
    img2, rays2, _ = renderer.render(p)
    assert rays2 == rays and img2.tobytes() == img.tobytes()
    acc, total = union_of_shards(renderer, w, h, spp, seed, 8, binding.VARIANT_DEFAULT)
    assert total == rays and acc.tobytes() == img.tobytes()
    # the throughput entry point (big-scene kernels, tiles summed inside the launch: 2 040 tiles claimed by the XCDs' cursors)
    hf = binding.HostFrames(w, h, 1)
    renderer.render_async(p, hf)
    renderer.sync()
    assert hf.rays(0) == rays and hf.image(0).tobytes() == img.tobytes()
    hf.close()


# ---- adversarial families (VERDICT r01 / ADVICE r01) --------------------------------------------------


def _cscene(sa):
    cs = binding.CScene()
    cs.count = sa.count
    for k in r1o.SCENE_F32:
        setattr(cs, k, sa.arrays[k].ctypes.data_as(C.POINTER(C.c_float)))
    cs.mat_type = sa.arrays["mat_type"].ctypes.data_as(C.POINTER(C.c_uint8))
    return cs


def _ccamera(sa):
    cc = binding.CCamera()
    C.memmove(C.byref(cc), C.byref(sa.camera), C.sizeof(cc))
    return cc


def _scene(c, rad, rng, cam, inv_radius=None, radius_sq=None):
    c = np.asarray(c, np.float32)
    rad = np.asarray(rad, np.float64)
    n = len(rad)
    mt = rng.integers(0, 3, n).astype(np.uint8)
    arr = {"center_x": c[:, 0].copy(), "center_y": c[:, 1].copy(), "center_z": c[:, 2].copy(),
           "radius_sq": (rad.astype(np.float32) * rad.astype(np.float32)) if radius_sq is None else radius_sq.astype(np.float32),
           "inv_radius": (np.float32(1.0) / rad.astype(np.float32)).astype(np.float32) if inv_radius is None else inv_radius.astype(np.float32),
           "mat_type": mt,
           "albedo_r": rng.uniform(0.1, 0.95, n).astype(np.float32), "albedo_g": rng.uniform(0.1, 0.95, n).astype(np.float32),
           "albedo_b": rng.uniform(0.1, 0.95, n).astype(np.float32),
           "mat_param": np.where(mt == 2, rng.uniform(1.1, 2.4, n), rng.uniform(0, 1, n)).astype(np.float32)}
    pad = (-n) % 8
    for k in arr:
        fill = {"center_x": 999999999.0, "center_y": 999999999.0, "center_z": 999999999.0, "mat_type": 255}.get(k, 0)
        arr[k] = np.concatenate([arr[k], np.full(pad, fill, arr[k].dtype)])
    return r1o.SceneArrays(arr, np.asarray(cam, np.float32))


def _same_bits_or_both_nan(a, b):
    """Bit equality of float32 records; a NaN matches a NaN (x86 and gfx950 produce different default
    NaN payloads, and only the degenerate-radius family can produce one: inv_radius up to 1e23)."""
    au, bu = a.view(np.uint32), b.view(np.uint32)
    return bool(((au == bu) | (np.isnan(a) & np.isnan(b))).all())


def _check_all_kernels(renderer, sa, w, h, spp, seed):
    renderer.set_scene_raw(_cscene(sa), _ccamera(sa))
    ref = renderer.render_samples(r1.make_params(w, h, spp, seed, variant=binding.VARIANT_REFERENCE))
    for variant in (binding.VARIANT_BVH, binding.VARIANT_PREFILTER, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID):
        got = renderer.render_samples(r1.make_params(w, h, spp, seed, variant=variant))
        assert got[1] == ref[1], variant
        assert got[2].tobytes() == ref[2].tobytes(), variant     # same device arithmetic: bits, NaN payloads included
        assert got[0].tobytes() == ref[0].tobytes(), variant
    oimg, orays, osamples = r1o.render_frame(sa, r1o.make_params(w, h, spp, seed), want_samples=True)
    assert ref[1] == orays
    assert (rays_of(ref[2]) == rays_of(osamples)).all()
    assert _same_bits_or_both_nan(ref[2][:, :3], osamples[:, :3])
    return ref


def test_degenerate_radii_1e_minus_23_to_1e_minus_6(renderer):
    """The r_floor branch of the tree builder and radius_sq down to denormals / zero: spheres far
    smaller than the fp32 noise of the reference's discriminant (~3e-6 at distance 5) are hit only
    by rounding, and bit-exact parity means reproducing exactly those hits.  A narrow pinhole camera
    puts ~one pixel on each sphere so that such hits are frequent."""
    rng = np.random.default_rng(81)
    n, w, h, spp = 150, 240, 160, 6
    c = np.stack([rng.uniform(-0.22, 0.22, n), rng.uniform(-0.14, 0.14, n), rng.uniform(-0.3, 0.3, n)], 1)
    rad = np.exp(rng.uniform(np.log(1e-12), np.log(1e-6), n))
    rad[:10] = np.exp(rng.uniform(np.log(1e-23), np.log(1e-19), 10))  # radius_sq denormal or exactly 0
    origin = np.array([0.0, 0.0, 5.0])
    cam = np.concatenate([origin, origin + [-0.05, -0.0333, -1.0], [0.1, 0, 0], [0, 0.0666, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.0]])
    sa = _scene(c, rad, rng, cam)
    assert (sa.arrays["radius_sq"][:10] < 1e-37).all() and (sa.arrays["radius_sq"][:n] >= 0).all()
    ref = _check_all_kernels(renderer, sa, w, h, spp, 7)
    hits = int((rays_of(ref[2]) > 1).sum())
    assert hits >= 20, hits   # nothing else is in the scene: every second ray is a noise hit of a degenerate sphere


def test_camera_inside_a_radius_50_sphere(renderer):
    """Every ray starts inside sphere 0 (r = 50 around the origin): its box contains the origin and
    the far root t2 is the hit (a Lambertian or Dielectric shell lets paths out through its
    outward normal, a Metal shell absorbs them all)."""
    rng = np.random.default_rng(82)
    n, w, h, spp = 140, 72, 48, 3
    c = rng.uniform(-18, 18, (n, 3))
    rad = rng.uniform(0.2, 1.6, n)
    c[0], rad[0] = (0.0, 0.0, 0.0), 50.0
    cam = r1.create_small_scene(w, h).camera_array()
    sa = _scene(c, rad, rng, cam)
    for mat in (0, 1, 2):                   # the enclosing sphere as Lambertian, Metal, Dielectric
        sa.arrays["mat_type"][0] = mat
        sa.arrays["mat_param"][0] = 1.5 if mat == 2 else 0.3
        ref = _check_all_kernels(renderer, sa, w, h, spp, 100 + mat)
        assert (ref[2][rays_of(ref[2]) == 1, :3] == 0).all()  # no primary ray escapes to the sky: 1-ray samples are Metal absorptions
        if mat == 1:
            assert not ref[0].any()        # a Metal shell absorbs every path from inside (dot(scattered, n) < 0, rayweek1.cpp:432)


def test_cluster_1e4_to_1e5_units_from_the_origin(renderer):
    """fp32 spacing is 2e-3 .. 8e-3 out there, the same size as the small radii and larger than
    t_min: the exact test is mostly cancellation, and the prefilter slack / box pads scale with
    |c|^2 ~ 1e10.  Same view as the small scene, shifted."""
    rng = np.random.default_rng(83)
    w, h, spp = 72, 48, 3
    base = r1.create_small_scene(w, h).camera_array()
    for k, shift in enumerate(([1.0e4, 2.5e4, -1.5e4], [3.0e4, -8.0e4, 1.2e4], [-9.0e4, 4.0e4, 7.0e4])):
        n = 200
        shift = np.array(shift, np.float64)
        c = rng.uniform(-7, 7, (n, 3)) + shift
        rad = np.exp(rng.uniform(np.log(0.02), np.log(1.2), n))
        cam = base.astype(np.float64)
        cam[0:3] += shift
        cam[3:6] += shift
        sa = _scene(c, rad, rng, cam)
        ref = _check_all_kernels(renderer, sa, w, h, spp, 200 + k)
        assert (rays_of(ref[2]) > 1).mean() > 0.05   # the cluster is in view


def test_mismatched_radius_arrays_stay_conservative(renderer):
    """A C-ABI caller whose inv_radius does not belong to radius_sq (rays1.h asks for it, but breaking it
    used to lose hits silently): bounds follow the radius the exact test reads, so the
    accelerated kernels still equal the reference-form sweep, which reads the same two arrays."""
    rng = np.random.default_rng(84)
    n, w, h, spp = 200, 72, 48, 3
    c = rng.uniform(-6, 6, (n, 3))
    rad = rng.uniform(0.1, 0.9, n)
    inv = 1.0 / rad
    inv[::3] *= rng.uniform(2.0, 20.0, len(inv[::3]))     # inv_radius of a much smaller sphere
    inv[1::7] *= -1.0                                       # negative inv_radius: flipped normals, still hittable
    sa = _scene(c, rad, rng, r1.create_small_scene(w, h).camera_array(), inv_radius=inv)
    _check_all_kernels(renderer, sa, w, h, spp, 300)
    with pytest.raises(r1.R1Error) as e:
        sa.arrays["inv_radius"][5] = np.float32(np.nan)
        renderer.set_scene_raw(_cscene(sa), _ccamera(sa))
    assert e.value.code == binding.R1_EINVAL


# ---- one process, N GPUs: r1_multi (RCCL all-gather inside the C++ host path) ----------------------


def test_r1_multi_one_rank_communicator_equals_the_plain_render(renderer):
    """r1_multi_render = every device renders its tiles -> ONE ncclAllGather of (tile block + ray count)
    -> assemble on device 0 -> one copy to the host (rayweek1.cpp:804-813 is the join it stands for).  On a
    one-GPU box the communicator has one rank (valid in RCCL): the whole path runs, collective included."""
    m = binding.MultiRenderer([0])
    try:
        info = m.info()
        assert info["devices"] == 1 and info["rccl_version"] > 0
        for name, mk, w, h, spp in (("large", r1.create_large_scene, 1200, 800, 10), ("medium", r1.create_medium_scene, 333, 211, 5)):
            sc = mk(w, h)
            m.set_scene(sc)
            renderer.set_scene(sc)
            p = r1.make_params(w, h, spp, 10001)
            img, rays, secs = m.render(p)
            ref, ref_rays, _ = renderer.render(p)
            assert rays == ref_rays and img.tobytes() == ref.tobytes(), name
            assert secs > 0
            again = m.render(p)
            assert again[1] == rays and again[0].tobytes() == img.tobytes()
    finally:
        m.close()
    with pytest.raises(r1.R1Error) as e:   # an RCCL communicator needs distinct devices
        binding.MultiRenderer([0, 0])
    assert e.value.code == binding.R1_EINVAL


def test_r1_multi_batches_in_flight_equal_the_plain_renders(renderer):
    """r1_multi_render_batch_async: three frames (seeds s, s+7, s+14) per launch, ONE all-gather and one copy for the batch, two
    r1_multi objects in flight; every frame that lands on the host is the plain r1_render of its seed."""
    w, h, spp = 333, 211, 5
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    ms = [binding.MultiRenderer([0]) for _ in range(2)]
    hosts = [binding.HostFrames(w, h, 3) for _ in range(2)]
    try:
        for m in ms:
            m.set_scene(sc)
        for k, m in enumerate(ms):
            m.render_batch_async(r1.make_params(w, h, spp, 100 + k), 3, hosts[k], seed_stride=7)
        for m in ms:
            m.sync()
        for k in range(2):
            for f in range(3):
                ref, ref_rays, _ = renderer.render(r1.make_params(w, h, spp, 100 + k + 7 * f))
                assert hosts[k].rays(f) == ref_rays and hosts[k].image(f).tobytes() == ref.tobytes(), (k, f)
        ms[0].render_async(r1.make_params(w, h, spp, 5), hosts[0])   # the one-frame form is the batch of one
        ms[0].sync()
        ref, ref_rays, _ = renderer.render(r1.make_params(w, h, spp, 5))
        assert hosts[0].rays(0) == ref_rays and hosts[0].image(0).tobytes() == ref.tobytes()
        with pytest.raises(r1.R1Error):
            ms[0].render_batch_async(r1.make_params(w, h, spp, 5), 0, hosts[0])
    finally:
        for m in ms:
            m.close()
        for hf in hosts:
            hf.close()


def test_rayweek1_hip_gather_rccl_one_device(tmp_path):
    """The drop-in program with --gather rccl (one-rank communicator here): same report block, same files,
    same pixels and ray counts as the plain run."""
    import re
    import subprocess
    import os
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rays1bench_amd", "lib", "rayweek1_hip")
    args = ["-w", "--width", "160", "--height", "96", "--spp", "3"]
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    plain = subprocess.run([exe] + args, cwd=tmp_path / "a", capture_output=True, timeout=300)
    rccl = subprocess.run([exe] + args + ["--devices", "1", "--gather", "rccl"], cwd=tmp_path / "b", capture_output=True, timeout=300)
    assert plain.returncode == 0 and rccl.returncode == 0, rccl.stderr.decode()
    assert "gather: RCCL" in rccl.stdout.decode()
    assert re.findall(r"total rays:     (\d+)", plain.stdout.decode()) == re.findall(r"total rays:     (\d+)", rccl.stdout.decode())
    for n in ("small", "medium", "large"):
        assert open(tmp_path / "a" / f"out_{n}.tga", "rb").read() == open(tmp_path / "b" / f"out_{n}.tga", "rb").read()
        assert re.fullmatch(r"hip\|\d+\.\d{3}s\|\d+\|\d+\.\d{3} mrays/s\|", open(tmp_path / "b" / f"out_{n}.txt").read())


@pytest.mark.parametrize("case", ["sweep_small", "tree_big", "sweep_big", "medium_default", "empty_shards", "grid_small", "grid_big"])
def test_frame_batches_through_every_throughput_kernel(case):
    """Frame batches (MODE 3 builds of the throughput kernels) for the kernels tests/test_gpu_parity.py does not reach: the
    exhaustive sweep, the big-scene tree and sweep kernels (> 1023 spheres), a scene in DEFAULT's measured band, and shards
    that own no tile.  Every frame of a batch = r1_render of its seed."""
    torch = pytest.importorskip("torch")
    variant, shards, tw, th = binding.VARIANT_DEFAULT, 1, 32, 32
    if case == "sweep_small":
        sc, w, h, spp, variant = r1.create_large_scene(150, 90), 150, 90, 3, binding.VARIANT_PREFILTER
    elif case == "tree_big":
        sc, w, h, spp = r1.create_grid_scene(128, 96, 50, 32), 128, 96, 3
    elif case == "sweep_big":
        sc, w, h, spp, variant = r1.create_grid_scene(96, 64, 40, 30), 96, 64, 2, binding.VARIANT_PREFILTER
    elif case == "medium_default":
        sc, w, h, spp = r1.create_medium_scene(150, 90), 150, 90, 3
    elif case == "grid_small":  # the uniform grid's small-scene kernel (table in LDS)
        sc, w, h, spp, variant = r1.create_large_scene(150, 90), 150, 90, 3, binding.VARIANT_GRID
    elif case == "grid_big":
        sc, w, h, spp, variant = r1.create_grid_scene(96, 64, 40, 30), 96, 64, 2, binding.VARIANT_GRID
    else:  # one 32x32 tile, three shards: shards 1 and 2 own nothing
        sc, w, h, spp, shards = r1.create_small_scene(30, 20), 30, 20, 4, 3
    rend = r1.Renderer(0)
    rend.set_scene(sc)
    n = 3
    want = [rend.render(r1.make_params(w, h, spp, 500 + 7 * f, variant=variant, tile_w=tw, tile_h=th))[:2] for f in range(n)]
    if shards == 1:
        hf = binding.HostFrames(w, h, n)
        rend.render_batch_async(r1.make_params(w, h, spp, 500, variant=variant), n, hf, seed_stride=7)
        rend.sync()
        for f in range(n):
            assert hf.rays(f) == want[f][1], (case, f)
            assert hf.image(f).tobytes() == want[f][0].tobytes(), (case, f)
        hf.close()
    else:
        p0 = r1.make_params(w, h, spp, 500, variant=variant, shard=0, num_shards=shards)
        rec, frec = binding.shard_record_bytes(p0), binding.frame_record_bytes(p0)
        gathered = torch.full((shards, n, rec), 0xAB, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        for s_ in range(shards):
            rend.render_shard_device_batch(r1.make_params(w, h, spp, 500, variant=variant, shard=s_, num_shards=shards), n, gathered[s_].data_ptr(),
                                           seed_stride=7, stream_ptr=st)
        frames = torch.zeros((n, frec), dtype=torch.uint8, device="cuda")
        rend.assemble_device_records_batch(p0, n, gathered.data_ptr(), frames.data_ptr(), st)
        torch.cuda.synchronize()
        for f in range(n):
            assert frames[f, :w * h * 3].cpu().numpy().tobytes() == want[f][0].tobytes(), (case, f)
            assert int(frames[f, frec - 8:].view(torch.int64).item()) == want[f][1], (case, f)
            for s_ in (1, 2):  # tile-less shards: count 0
                assert int(gathered[s_, f, rec - 8:].view(torch.int64).item()) == 0
    rend.close()


def test_rayweek1_hip_pipeline_mode_counts_the_same_rays(tmp_path):
    """rayweek1_hip --pipeline FRAMES: the C++ host keeps frames in flight through r1_render_async (one context +
    page-locked buffer per frame) after its benchmark() runs; every pipelined frame is the frame benchmark() rendered,
    so FRAMES frames count FRAMES x its rays."""
    import re
    import subprocess
    import os
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rays1bench_amd", "lib", "rayweek1_hip")
    out = subprocess.run([exe, "--width", "160", "--height", "96", "--spp", "3", "--pipeline", "7", "--inflight", "3"], cwd=tmp_path,
                         capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    text = out.stdout.decode()
    single = dict(zip(("small", "medium", "large"), (int(v) for v in re.findall(r"total rays:     (\d+)", text))))
    for name in ("small", "medium", "large"):
        m = re.search(rf"{name} pipelined:  7 frames, 3 in flight, [\d.]+ ms per frame, (\d+) rays, [\d.]+ mrays/s", text)
        assert m, text
        assert int(m.group(1)) == 7 * single[name]
    # the same with every frame split over the devices of an r1_multi (one device here: a one-rank RCCL communicator per frame in flight)
    out = subprocess.run([exe, "--width", "160", "--height", "96", "--spp", "3", "--pipeline", "5", "--inflight", "2", "--devices", "1", "--gather", "rccl"],
                         cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    text = out.stdout.decode()
    for name in ("small", "medium", "large"):
        m = re.search(rf"{name} pipelined:  5 frames, 2 in flight \(each split over the devices, RCCL all-gather\), [\d.]+ ms per frame, (\d+) rays", text)
        assert m, text
        assert int(m.group(1)) == 5 * single[name]


# ---- PIXEL mode of the throughput entry point (r1_set_pixel_mode) --------------------------------------


@pytest.mark.parametrize("case", ["large_1200x800x10_8shards", "medium_ragged_tiles", "large_96x64x250", "grid_1600_spheres", "sweep_kernel",
                                  "uniform_grid_small_scene"])
def test_pixel_mode_writes_the_same_pixels_and_counts(case):
    """r1_set_pixel_mode: lanes own pixels and resolve in-kernel (3 B/pixel, no per-sample records, no resolve
    launch).  The device-resident shard blocks must equal, byte for byte, what the per-sample path renders."""
    torch = pytest.importorskip("torch")
    from rays1bench_amd import sharding
    variant = binding.VARIANT_DEFAULT
    if case == "large_1200x800x10_8shards":
        sc, w, h, spp, shards, tw, th = r1.create_large_scene(1200, 800), 1200, 800, 10, 8, 32, 32
    elif case == "medium_ragged_tiles":
        sc, w, h, spp, shards, tw, th = r1.create_medium_scene(150, 90), 150, 90, 3, 3, 24, 40
    elif case == "large_96x64x250":
        sc, w, h, spp, shards, tw, th = r1.create_large_scene(96, 64), 96, 64, 250, 2, 32, 32
    elif case == "grid_1600_spheres":
        sc, w, h, spp, shards, tw, th = r1.create_grid_scene(160, 120, 50, 32), 160, 120, 4, 2, 32, 32
    elif case == "sweep_kernel":
        sc, w, h, spp, shards, tw, th, variant = r1.create_large_scene(320, 200), 320, 200, 6, 1, 32, 32, binding.VARIANT_PREFILTER
    else:  # R1_VARIANT_GRID on a small scene: PIXEL mode runs the grid's big-scene kernel (r1_frame.cpp big_scene)
        sc, w, h, spp, shards, tw, th, variant = r1.create_large_scene(150, 90), 150, 90, 3, 2, 24, 40, binding.VARIANT_GRID
    rend = r1.Renderer(0)
    try:
        rend.set_scene(sc)
        ref, ref_rays, _ = rend.render(r1.make_params(w, h, spp, 77, tile_w=tw, tile_h=th, variant=variant))
        rend.set_pixel_mode(True)
        nbytes = binding.shard_block_bytes(r1.make_params(w, h, spp, 77, tile_w=tw, tile_h=th, shard=0, num_shards=shards))
        rec = nbytes + sharding.RECORD_TRAILER
        records = torch.zeros((shards, rec), dtype=torch.uint8, device="cuda")
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for s in range(shards):
            rend.render_shard_device(r1.make_params(w, h, spp, 77, tile_w=tw, tile_h=th, shard=s, num_shards=shards, variant=variant),
                                     records[s].data_ptr(), records[s].data_ptr() + nbytes, stream)
        rend.assemble_device_strided(r1.make_params(w, h, spp, 77, tile_w=tw, tile_h=th, shard=0, num_shards=shards), records.data_ptr(), rec,
                                     out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert sharding.total_rays(records.view(-1), shards) == ref_rays
        assert out.cpu().numpy().tobytes() == ref.tobytes()
        # and the host-returning entry point of the same context still renders per sample
        again, rays2, samples = rend.render_samples(r1.make_params(w, h, spp, 77, tile_w=tw, tile_h=th, variant=variant))
        assert rays2 == ref_rays and again.tobytes() == ref.tobytes() and int(rays_of(samples).sum()) == ref_rays
    finally:
        rend.close()


def test_frame_sequences_on_one_context_keep_the_counter_block_consistent():
    """The resolve launch of a frame publishes its ray count and zeroes the context's counter block for the NEXT frame
    (r1_frame.cpp: fused_clear); diagnostic frames, PIXEL-mode frames and empty shards clear with memsets instead.  Every
    order of these on ONE context must give the same counts and pixels: a frame that inherits a dirty block would
    start with an advanced sample queue (too few rays) or a non-zero count (too many)."""
    torch = pytest.importorskip("torch")
    from rays1bench_amd import sharding
    w, h, spp = 200, 120, 6
    rend = r1.Renderer(0)
    try:
        rend.set_scene(r1.create_large_scene(w, h))
        p = r1.make_params(w, h, spp, 5)
        ref, ref_rays, _ = rend.render(p)
        nbytes = binding.shard_block_bytes(p)
        rec = torch.zeros(nbytes + sharding.RECORD_TRAILER, dtype=torch.uint8, device="cuda")
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def device_frame(params=p):
            rec.zero_()
            rend.render_shard_device(params, rec.data_ptr(), rec.data_ptr() + nbytes, stream)
            rend.assemble_device_strided(p, rec.data_ptr(), rec.numel(), out.data_ptr(), stream)
            torch.cuda.synchronize()
            return out.cpu().numpy().tobytes(), sharding.total_rays(rec, 1)

        def host_frame(variant):
            img, rays, _ = rend.render(r1.make_params(w, h, spp, 5, variant=variant))
            return img.tobytes(), rays

        want = (ref.tobytes(), ref_rays)
        for step in ("device", "device", "stats", "device", "host", "sweep_stats", "host", "pixel", "device", "pixel_off", "device", "host",
                     "wavefront", "device", "reference", "host"):
            if step == "device":
                got = device_frame()
            elif step == "host":
                got = host_frame(binding.VARIANT_DEFAULT)
            elif step == "stats":
                got = host_frame(binding.VARIANT_BVH_STATS)
            elif step == "sweep_stats":
                got = host_frame(binding.VARIANT_STATS)
            elif step == "wavefront":
                got = host_frame(binding.VARIANT_WAVEFRONT)
            elif step == "reference":
                got = host_frame(binding.VARIANT_REFERENCE)
            elif step == "pixel":
                rend.set_pixel_mode(True)
                got = device_frame()
            else:
                rend.set_pixel_mode(False)
                got = device_frame()
            assert got[1] == want[1], (step, got[1], want[1])
            assert got[0] == want[0], step
    finally:
        rend.close()


@pytest.mark.parametrize("case", ["large_tree", "large_sweep", "medium", "small", "grid_2600_tree", "large_250spp"])
def test_throughput_entry_point_equals_the_synchronous_one(case):
    """r1_render_shard_device runs the frames-in-flight kernels (one queue, majority walk, a prepared spare sample per
    lane), r1_render the synchronous-frame kernels (sub-queues, cooperative tail, no spares): same pixels, same count —
    which sample a lane traces when is not supposed to matter."""
    torch = pytest.importorskip("torch")
    from rays1bench_amd import sharding
    variant = binding.VARIANT_DEFAULT
    if case == "large_tree":
        sc, w, h, spp, variant = r1.create_large_scene(1200, 800), 1200, 800, 10, binding.VARIANT_BVH
    elif case == "large_sweep":
        sc, w, h, spp, variant = r1.create_large_scene(1200, 800), 1200, 800, 10, binding.VARIANT_PREFILTER
    elif case == "medium":
        sc, w, h, spp = r1.create_medium_scene(640, 400), 640, 400, 7
    elif case == "small":
        sc, w, h, spp = r1.create_small_scene(333, 211), 333, 211, 9
    elif case == "grid_2600_tree":
        sc, w, h, spp = r1.create_grid_scene(320, 200, 64, 40), 320, 200, 5
    else:
        sc, w, h, spp = r1.create_large_scene(160, 96), 160, 96, 250
    rend = r1.Renderer(0)
    try:
        rend.set_scene(sc)
        p = r1.make_params(w, h, spp, 4242, variant=variant)
        ref, ref_rays, _ = rend.render(p)
        nbytes = binding.shard_block_bytes(p)
        rec = torch.zeros(nbytes + sharding.RECORD_TRAILER, dtype=torch.uint8, device="cuda")
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for _ in range(2):  # twice: the second frame inherits the counter block the first one's resolve launch cleared
            rec.zero_()
            rend.render_shard_device(p, rec.data_ptr(), rec.data_ptr() + nbytes, stream)
            rend.assemble_device_strided(p, rec.data_ptr(), rec.numel(), out.data_ptr(), stream)
            torch.cuda.synchronize()
            assert sharding.total_rays(rec, 1) == ref_rays
            assert out.cpu().numpy().tobytes() == ref.tobytes()
    finally:
        rend.close()


def test_plain_bench_run_dumps_the_last_timed_frame(tmp_path):
    """`bench.py --dump-outputs DIR` (a plain run: no check, no secondary measurements): the pixels and ray count of the last
    timed frame, as float32 / float64 .npy files, equal ONE synchronous r1_render of the same frame."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, spp, seed = 300, 200, 4, 10001
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--width", str(w),
                          "--height", str(h), "--spp", str(spp), "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, timeout=600, cwd=root, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")})
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    line = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("check", "cpu_baseline", "value_device_resident", "value_dispatch_to_host", "exhaustive_sweep"):
        assert k not in line, k
    img = np.load(tmp_path / "out" / "image.npy")
    rays = np.load(tmp_path / "out" / "rays.npy")
    assert img.dtype == np.float32 and img.shape == (h, w, 3) and rays.dtype == np.float64 and rays.shape == (1,)
    rend = r1.Renderer(0)
    try:
        rend.set_scene(r1.create_large_scene(w, h))
        ref, ref_rays, _ = rend.render(r1.make_params(w, h, spp, seed))
    finally:
        rend.close()
    assert int(rays[0]) == ref_rays == line["config"]["rays_per_step"]
    assert np.array_equal(img, ref.astype(np.float32))
