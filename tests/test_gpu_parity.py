"""GPU parity tests (run on the MI355X box: pytest -m gpu).  Everything goes through the
C-ABI of librays1.so; the oracle (oracle/libr1_oracle.so) and the committed fixtures
(tests/golden/, produced by the reference's own code) are the checkers.

Tolerances (stated once, used below):
  * RNG, scene tables, indexing, ray counts per sample, u8 pixels: BIT-EXACT expected.
  * per-sample radiance: bit-exact expected; the only arithmetic that differs from the
    oracle is powf(x, 5) (glibc, <1 ulp) vs an exactly rounded x^5 on the device, which can
    flip one Dielectric reflect/refract decision in ~1e8 — so the tests allow a fraction
    1e-5 of samples / pixels to differ and require everything else to be bit-identical.
  * versus the reference's own multi-threaded run (sequential seeding, irreproducible,
    SURVEY.md §7.1): statistics only — total rays within 0.1 %.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCENES = ("small", "medium", "large")
MAKE = {"small": r1.create_small_scene, "medium": r1.create_medium_scene, "large": r1.create_large_scene}
ALLOWED_FLIP_FRACTION = 1e-5


# Every test of this module runs once per kernel family: DEFAULT (resolves to the box tree except
# for 9..127 hittable spheres) and PREFILTER (always the grouped exhaustive sweep).  Calls that
# name a variant explicitly keep it.
KERNEL = {"variant": 0}


@pytest.fixture(autouse=True, params=[binding.VARIANT_DEFAULT, binding.VARIANT_PREFILTER], ids=["default", "sweep"])
def kernel_family(request):
    KERNEL["variant"] = request.param
    yield request.param


def mp(*a, **k):
    k.setdefault("variant", KERNEL["variant"])
    return r1.make_params(*a, **k)


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


# ---- fixtures from the reference itself ---------------------------------------------------


@pytest.mark.parametrize("name", SCENES)
def test_samples_match_reference_fixture_1200x800x10(renderer, name):
    g = r1o.read_golden(os.path.join(GOLD, f"samples_{name}_1200x800x10.bin"))
    w, h, spp, seed, _ = g["hdr"].tolist()
    sc = MAKE[name](w, h)
    renderer.set_scene(sc)
    img, rays, samples = renderer.render_samples(mp(w, h, spp, seed))
    idx = (g["y"].astype(np.int64) * w + g["x"]) * spp + g["s"]
    got = samples[idx]
    same_rays = rays_of(got) == g["rays"]
    same_rgb = (got[:, :3].view(np.uint32) == g["rgb"].reshape(-1, 3).view(np.uint32)).all(1)
    # exact: these are fixed seeds and fixtures, and the one documented deviation (powf(x, 5), module
    # docstring) flips none of their samples
    assert same_rays.all() and same_rgb.all(), (int((~same_rays).sum()), int((~same_rgb).sum()))
    # whole-frame invariants
    assert int(rays_of(samples).sum()) == rays
    assert rays_of(samples).min() >= 1 and rays_of(samples).max() <= 51
    assert np.isfinite(samples[:, :3]).all() and samples[:, :3].min() >= 0 and samples[:, :3].max() <= 1
    # reference totals for the same seeding contract (tests/golden/full_1200x800x10.json)
    with open(os.path.join(GOLD, "full_1200x800x10.json")) as f:
        full = json.load(f)[name]
    assert abs(rays - full["rays"]) <= max(4, full["rays"] * ALLOWED_FLIP_FRACTION), (rays, full["rays"])
    rowrays = rays_of(samples).reshape(h, w * spp).sum(1)
    assert (rowrays != np.array(full["rowrays"])).sum() <= 2
    assert abs(img.astype(np.float64).mean() - full["image_mean"]) < 1e-3


@pytest.mark.parametrize("name", SCENES)
def test_small_frames_match_reference_fixture(renderer, name):
    g = r1o.read_golden(os.path.join(GOLD, f"frame_{name}_200x100x4.bin"))
    w, h, spp, seed = g["hdr"].tolist()
    renderer.set_scene(MAKE[name](w, h))
    img, rays, _ = renderer.render(mp(w, h, spp, seed))
    assert rays == int(g["rays"][0])
    assert img.tobytes() == g["image"].tobytes()


def test_ragged_frame_matches_reference_fixture(renderer):
    g = r1o.read_golden(os.path.join(GOLD, "frame_medium_77x45x3.bin"))
    w, h, spp, seed = g["hdr"].tolist()
    renderer.set_scene(r1.create_medium_scene(w, h))
    img, rays, _ = renderer.render(mp(w, h, spp, seed))
    assert rays == int(g["rays"][0])
    assert img.tobytes() == g["image"].tobytes()


def test_second_seed_and_spp_64_fixture(renderer):
    g = r1o.read_golden(os.path.join(GOLD, "samples_large_320x200x64.bin"))
    w, h, spp, seed, _ = g["hdr"].tolist()
    renderer.set_scene(r1.create_large_scene(w, h))
    img, rays, samples = renderer.render_samples(mp(w, h, spp, seed))
    got = samples[(g["y"].astype(np.int64) * w + g["x"]) * spp + g["s"]]
    assert (rays_of(got) == g["rays"]).all()
    assert got[:, :3].tobytes() == g["rgb"].tobytes()


# ---- against the oracle, live --------------------------------------------------------------


@pytest.mark.parametrize("name,w,h,spp,seed", [("small", 160, 120, 16, 7), ("medium", 333, 211, 5, 123456789), ("large", 256, 192, 12, 0)])
def test_full_frame_bit_exact_vs_oracle(renderer, name, w, h, spp, seed):
    sc = MAKE[name](w, h)
    renderer.set_scene(sc)
    p = mp(w, h, spp, seed)
    img, rays, samples = renderer.render_samples(p)
    oimg, orays, osamples = r1o.render_frame(oracle_scene(sc), oparams(p), want_samples=True)
    differing = (samples.view(np.uint32) != osamples.view(np.uint32)).any(1)
    assert differing.mean() <= ALLOWED_FLIP_FRACTION, differing.sum()
    assert abs(rays - orays) <= 51 * differing.sum()
    assert (img != oimg).any(2).mean() <= ALLOWED_FLIP_FRACTION


def test_reference_variant_equals_prefilter_variant(renderer):
    """The 8-op conservative prefilter must select a superset of the reference's candidates:
    with the exact re-test the two kernels are bit-identical on every sample."""
    for name, (w, h, spp) in {"small": (320, 200, 8), "medium": (320, 200, 8), "large": (400, 300, 6)}.items():
        renderer.set_scene(MAKE[name](w, h))
        a = renderer.render_samples(mp(w, h, spp, 99, variant=binding.VARIANT_REFERENCE))
        b = renderer.render_samples(mp(w, h, spp, 99, variant=binding.VARIANT_PREFILTER))
        assert a[1] == b[1]
        assert a[2].tobytes() == b[2].tobytes()
        assert a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("w,h,spp,bounces", [(1, 1, 1, 50), (33, 1, 3, 50), (1, 65, 2, 50), (64, 64, 1, 1), (40, 30, 7, 3), (31, 33, 2, 51)])
def test_edge_sizes_and_bounce_limits_vs_oracle(renderer, w, h, spp, bounces):
    sc = r1.create_medium_scene(w, h)
    renderer.set_scene(sc)
    p = mp(w, h, spp, 5, max_bounces=bounces)
    img, rays, samples = renderer.render_samples(p)
    oimg, orays, osamples = r1o.render_frame(oracle_scene(sc), oparams(p), want_samples=True)
    assert rays == orays
    assert samples.tobytes() == osamples.tobytes()
    assert img.tobytes() == oimg.tobytes()
    assert rays_of(samples).max() <= bounces + 1


def test_hollow_sphere_and_placeholders_are_never_hit(renderer):
    """inv_radius == 0 spheres (the small scene's r = -0.45 shell and the 1e9 placeholders) are
    skipped (rayweek1.cpp:291): a scene with them removed renders identically."""
    sc = r1.create_small_scene(200, 100)
    renderer.set_scene(sc)
    p = mp(200, 100, 8, 3)
    a = renderer.render_samples(p)
    arr = sc.arrays()
    keep = arr["inv_radius"] != 0
    assert keep.sum() == 4
    sa = r1o.SceneArrays({k: v[keep] for k, v in arr.items()}, sc.camera_array())
    renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
    b = renderer.render_samples(p)
    assert a[1] == b[1] and a[2].tobytes() == b[2].tobytes()


def _as_cscene(sa):
    cs = binding.CScene()
    cs.count = sa.count
    for k in r1o.SCENE_F32:
        setattr(cs, k, sa.arrays[k].ctypes.data_as(C.POINTER(C.c_float)))
    cs.mat_type = sa.arrays["mat_type"].ctypes.data_as(C.POINTER(C.c_uint8))
    return cs


def _as_ccamera(sa):
    cc = binding.CCamera()
    C.memmove(C.byref(cc), C.byref(sa.camera), C.sizeof(cc))
    return cc


# ---- size-independent properties at the BASELINE size -----------------------------------------


def test_full_size_determinism_seed_and_statistics(renderer):
    w, h, spp = 1200, 800, 10
    renderer.set_scene(r1.create_large_scene(w, h))
    a = renderer.render(mp(w, h, spp, 10001))
    b = renderer.render(mp(w, h, spp, 10001))
    c = renderer.render(mp(w, h, spp, 10002))
    assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()  # run-to-run identical
    assert c[0].tobytes() != a[0].tobytes() and abs(c[1] - a[1]) / a[1] < 2e-3
    with open(os.path.join(GOLD, "MANIFEST.json")) as f:
        native = json.load(f)["native_mt_rays_1200x800x10"]["large"]
    # vs the reference's own multi-threaded run (sequential seeding): statistics only
    assert abs(a[1] - np.mean(native)) / np.mean(native) < 1e-3
    assert abs(a[1] / (w * h * spp) - 2.81) < 0.02  # rays per sample, SURVEY.md §6


# ---- sharding (the multi-GPU decomposition, exercised on one device) ----------------------------


@pytest.mark.parametrize("shards", [2, 3, 8])
def test_shards_tile_the_frame_exactly(renderer, shards):
    w, h, spp = 300, 170, 4
    renderer.set_scene(r1.create_large_scene(w, h))
    full, full_rays, _ = renderer.render(mp(w, h, spp, 11))
    tw = th = 32  # (make_params' default tiles) global tile t belongs to shard t % shards
    ys, xs = np.mgrid[0:h, 0:w]
    owner = ((ys // th) * ((w + tw - 1) // tw) + xs // tw) % shards
    sentinel = 0xCD
    acc = np.full_like(full, sentinel)
    total = 0
    for s in range(shards):
        part = np.full_like(full, sentinel)
        rays, _ = renderer.render_into(mp(w, h, spp, 11, shard=s, num_shards=shards), part)
        mine = owner == s
        assert part[mine].tobytes() == full[mine].tobytes(), s  # the shard's own tiles: the full frame's pixels
        assert (part[~mine] == sentinel).all(), s  # every other pixel untouched
        acc[mine] = part[mine]
        total += rays
    assert total == full_rays
    assert acc.tobytes() == full.tobytes()


def test_device_resident_shard_and_assemble(renderer):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    w, h, spp, shards = 300, 170, 4, 4
    renderer.set_scene(r1.create_medium_scene(w, h))
    full, full_rays, _ = renderer.render(mp(w, h, spp, 21))
    nbytes = binding.shard_block_bytes(mp(w, h, spp, 21, shard=0, num_shards=shards))
    blocks = torch.zeros((shards, nbytes), dtype=torch.uint8, device="cuda")
    rays = torch.zeros(shards, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for s in range(shards):
        p = mp(w, h, spp, 21, shard=s, num_shards=shards)
        renderer.render_shard_device(p, blocks[s].data_ptr(), rays[s:].data_ptr(), stream)
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    renderer.assemble_device(mp(w, h, spp, 21, shard=0, num_shards=shards), blocks.data_ptr(), out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert int(rays.sum().item()) == full_rays
    assert out.cpu().numpy().tobytes() == full.tobytes()
    t_trace, t_total = renderer.last_timing()
    assert 0 < t_trace <= t_total
    # records = block + 8-byte ray count, strided assembly (what bench.py gathers)
    rec = nbytes + 8
    records = torch.zeros((shards, rec), dtype=torch.uint8, device="cuda")
    for s in range(shards):
        p = mp(w, h, spp, 21, shard=s, num_shards=shards)
        renderer.render_shard_device(p, records[s].data_ptr(), records[s].data_ptr() + nbytes, stream)
    out2 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    renderer.assemble_device_strided(mp(w, h, spp, 21, shard=0, num_shards=shards), records.data_ptr(), rec, out2.data_ptr(), stream)
    torch.cuda.synchronize()
    from rays1bench_amd import sharding
    assert out2.cpu().numpy().tobytes() == full.tobytes()
    assert sharding.total_rays(records.view(-1), shards) == full_rays
    img_h, rays_h = sharding.assemble_records(records.cpu().numpy(), w, h, shards)
    assert img_h.tobytes() == full.tobytes() and rays_h == full_rays


def test_records_with_odd_tiles_are_aligned_and_sum_their_counts(renderer):
    """with 5x7 tiles a shard block is not a multiple of 8 bytes; the record pads it so that the uint64 ray
    count behind it stays aligned (r1_shard_record_bytes), an unaligned count pointer is R1_EINVAL, and
    r1_assemble_device_records scatters the blocks and sums the shards' counts next to the image."""
    torch = pytest.importorskip("torch")
    from rays1bench_amd import sharding
    w, h, spp, shards, tw, th = 93, 61, 3, 3, 5, 7
    renderer.set_scene(r1.create_small_scene(w, h))
    full, full_rays, _ = renderer.render(mp(w, h, spp, 77, tile_w=tw, tile_h=th))
    p0 = mp(w, h, spp, 77, tile_w=tw, tile_h=th, shard=0, num_shards=shards)
    nbytes, rec = binding.shard_block_bytes(p0), binding.shard_record_bytes(p0)
    assert nbytes % 8 != 0 and rec % 8 == 0 and rec == ((nbytes + 7) & ~7) + 8 == sharding.record_bytes(w, h, shards, tw, th)
    records = torch.zeros((shards, rec), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(r1.R1Error) as e:
        renderer.render_shard_device(p0, records[0].data_ptr(), records[0].data_ptr() + nbytes, stream)  # unaligned count
    assert e.value.code == binding.R1_EINVAL
    for s_ in range(shards):
        q = mp(w, h, spp, 77, tile_w=tw, tile_h=th, shard=s_, num_shards=shards)
        renderer.render_shard_device(q, records[s_].data_ptr(), records[s_].data_ptr() + rec - 8, stream)
    img_pad = (w * h * 3 + 7) & ~7
    out = torch.zeros(img_pad + 8, dtype=torch.uint8, device="cuda")
    renderer.assemble_device_records(p0, records.data_ptr(), out.data_ptr(), out.data_ptr() + img_pad, stream)
    torch.cuda.synchronize()
    assert out[:w * h * 3].cpu().numpy().tobytes() == full.tobytes()
    assert int(out[img_pad:].view(torch.int64).item()) == full_rays == sharding.total_rays(records.view(-1), shards)
    img_h, rays_h = sharding.assemble_records(records.cpu().numpy(), w, h, shards, tw, th)
    assert img_h.tobytes() == full.tobytes() and rays_h == full_rays


def test_render_async_lands_the_frame_in_page_locked_host_memory(renderer):
    """r1_render_async (frames in flight whose results land on the host, bench.py's `value`): same pixels and count as
    the synchronous r1_render, through the throughput kernels, several frames in flight on several contexts."""
    w, h, spp = 210, 130, 5
    frames = []
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    want = {seed: renderer.render(mp(w, h, spp, seed))[:2] for seed in (5, 6, 7)}
    ctxs = [r1.Renderer(0) for _ in range(3)]
    for c, seed in zip(ctxs, (5, 6, 7)):
        c.set_scene(sc)
        hf = binding.HostFrame(w, h)
        c.render_async(mp(w, h, spp, seed), hf)  # the context's own stream
        frames.append((c, hf, seed))
    for c, hf, seed in frames:
        c.sync()
        assert hf.rays == want[seed][1]
        assert hf.image.tobytes() == want[seed][0].tobytes()
    # a second frame through the same context and buffer; sharded frames are refused
    c, hf, _ = frames[0]
    c.render_async(mp(w, h, spp, 6), hf)
    c.sync()
    assert hf.rays == want[6][1] and hf.image.tobytes() == want[6][0].tobytes()
    with pytest.raises(r1.R1Error):
        c.render_async(mp(w, h, spp, 6, shard=0, num_shards=2), hf)
    c.render_frame_device(mp(w, h, spp, 7))  # no host buffers: the frame stays on the device
    c.sync()
    assert hf.rays == want[6][1]
    for c, hf, _ in frames:
        c.close()
        hf.close()


def test_frames_in_flight_land_in_order_and_intact(renderer):
    """Tiles summed inside the trace kernel: many frames in flight on several contexts, every one with its own seed
    and size class, each landing in page-locked memory with no copy — every frame must equal the synchronous render of its seed
    (records are handed from the tracing waves to the summing wave without a fence: a stale record would show here), launch after
    launch through the same contexts (the two sets of cursors alternate), including ragged frames and frames of a single tile."""
    rends = [r1.Renderer(0) for _ in range(6)]
    try:
        for (w, h, spp) in ((320, 200, 6), (77, 45, 3), (31, 17, 9), (640, 352, 2)):
            sc = r1.create_large_scene(w, h)
            renderer.set_scene(sc)
            for r_ in rends:
                r_.set_scene(sc)
            hfs = [binding.HostFrames(w, h, 1) for _ in rends]
            for rnd in range(5):
                seeds = [1000 * rnd + 17 * k + w for k in range(len(rends))]
                for hf in hfs:
                    hf._all[:] = 0xCD
                for r_, hf, sd in zip(rends, hfs, seeds):
                    r_.render_async(mp(w, h, spp, sd), hf)
                for r_ in rends:
                    r_.sync()
                for hf, sd in zip(hfs, seeds):
                    img, rays, _ = renderer.render(mp(w, h, spp, sd))
                    assert hf.rays(0) == rays, (w, h, spp, rnd, sd)
                    assert hf.image(0).tobytes() == img.tobytes(), (w, h, spp, rnd, sd)
            for hf in hfs:
                hf.close()
    finally:
        for r_ in rends:
            r_.close()


def test_frame_batches_equal_single_frames(renderer):
    """Frame batches (r1_render_batch_async / r1_render_shard_device_batch): n frames in ONE launch, the persistent waves
    flowing from one frame into the next.  Every frame's pixels and ray count equal a synchronous r1_render of its seed —
    whole frames and 3 shards x 2 frames through the gathered [shard][frame][record] layout, ragged size, odd tiles."""
    torch = pytest.importorskip("torch")
    w, h, spp, n = 211, 77, 3, 4
    sc = r1.create_large_scene(w, h)
    renderer.set_scene(sc)
    want = [renderer.render(mp(w, h, spp, 40 + 3 * f))[:2] for f in range(n)]
    hf = binding.HostFrames(w, h, n)
    p = mp(w, h, spp, 40)
    assert hf.record == binding.frame_record_bytes(p)
    renderer.render_batch_async(p, n, hf, seed_stride=3)
    renderer.sync()
    for f in range(n):
        assert hf.rays(f) == want[f][1], f
        assert hf.image(f).tobytes() == want[f][0].tobytes(), f
    # a shorter batch through the same context (partial last batch of a run), identical frames (stride 0)
    renderer.render_batch_async(p, 2, hf, seed_stride=0)
    renderer.sync()
    assert hf.rays(0) == hf.rays(1) == want[0][1] and hf.image(1).tobytes() == want[0][0].tobytes()
    hf.close()
    # shards: 3 shards x 2 frames, 5x7 tiles; one "all-gather" = the shards' record arrays side by side
    shards, nf, tw, th = 3, 2, 5, 7
    want2 = [renderer.render(mp(w, h, spp, 90 + f, tile_w=tw, tile_h=th))[:2] for f in range(nf)]
    p0 = mp(w, h, spp, 90, tile_w=tw, tile_h=th, shard=0, num_shards=shards)
    rec, frec = binding.shard_record_bytes(p0), binding.frame_record_bytes(p0)
    gathered = torch.zeros((shards, nf, rec), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for s_ in range(shards):
        q = mp(w, h, spp, 90, tile_w=tw, tile_h=th, shard=s_, num_shards=shards)
        renderer.render_shard_device_batch(q, nf, gathered[s_].data_ptr(), seed_stride=1, stream_ptr=stream)
    frames = torch.zeros((nf, frec), dtype=torch.uint8, device="cuda")
    renderer.assemble_device_records_batch(p0, nf, gathered.data_ptr(), frames.data_ptr(), stream)
    torch.cuda.synchronize()
    for f in range(nf):
        assert frames[f, :w * h * 3].cpu().numpy().tobytes() == want2[f][0].tobytes(), f
        assert int(frames[f, frec - 8:].view(torch.int64).item()) == want2[f][1], f
    # variants without a throughput kernel refuse batches; a batch beyond 2^31 sample slots per launch is a documented limit
    with pytest.raises(r1.R1Error):
        renderer.render_batch_async(mp(w, h, spp, 1, variant=binding.VARIANT_REFERENCE), 2, None)
    with pytest.raises(r1.R1Error) as e:
        renderer.render_batch_async(mp(1024, 1024, 1000, 1), 3, None)  # 3 x 1.05 G slots
    assert e.value.code == binding.R1_ELIMIT
    img_after, rays_after, _ = renderer.render(mp(w, h, spp, 40))  # the context is still usable
    assert rays_after == want[0][1] and img_after.tobytes() == want[0][0].tobytes()


# ---- big scenes (BASELINE config 5 shape: the large generator scaled up) -------------------------


@pytest.mark.parametrize("gw,gh,w,h,spp", [(64, 40, 160, 120, 4), (33, 31, 96, 64, 3)])
def test_big_scene_kernels_bit_exact_vs_oracle(renderer, gw, gh, w, h, spp):
    """> 1023 hittable spheres: the exhaustive sweep switches to the 32-bit-index kernels (global
    attenuation stack, LDS-tiled sweep); R1_VARIANT_PREFILTER pins it (DEFAULT resolves to the
    box tree there, tests/test_gpu_bvh.py)."""
    sc = r1.create_grid_scene(w, h, gw, gh)
    assert int((sc.arrays()["inv_radius"] != 0).sum()) == gw * gh + 4 > 1023
    renderer.set_scene(sc)
    p = mp(w, h, spp, 31337, variant=binding.VARIANT_PREFILTER)
    img, rays, samples = renderer.render_samples(p)
    assert renderer.launch_info()["kernel"] == binding.VARIANT_PREFILTER
    oimg, orays, osamples = r1o.render_frame(oracle_scene(sc), oparams(p), want_samples=True)
    assert rays == orays
    assert samples.tobytes() == osamples.tobytes()
    assert img.tobytes() == oimg.tobytes()
    ref = renderer.render_samples(mp(w, h, spp, 31337, variant=binding.VARIANT_REFERENCE))
    assert ref[1] == rays and ref[2].tobytes() == samples.tobytes()


def test_config5_shape_100k_spheres_runs_and_matches_oracle_on_a_crop(renderer):
    """BASELINE config 5 (100 004 spheres, 1920x1080 aspect): a small frame through the 100 k
    sweep; the oracle checks a sample of pixel-samples (its brute-force frame would take minutes)."""
    w, h, spp = 96, 54, 2
    sc = r1.create_grid_scene(w, h, 400, 250)
    renderer.set_scene(sc)
    p = mp(w, h, spp, 5, variant=binding.VARIANT_PREFILTER)
    img, rays, samples = renderer.render_samples(p)
    sa = oracle_scene(sc)
    rng = np.random.default_rng(0)
    xs, ys, ss = rng.integers(0, w, 300), rng.integers(0, h, 300), rng.integers(0, spp, 300)
    rgb, orays = r1o.trace_samples(sa, w, h, 5, xs, ys, ss)
    got = samples[(ys * w + xs) * spp + ss]
    assert (rays_of(got) == orays).all()
    assert got[:, :3].tobytes() == rgb.tobytes()
    assert int(rays_of(samples).sum()) == rays


# ---- the drop-in host program (C++: create_*_scene / benchmark / main -w -n) ---------------------


def test_rayweek1_hip_program_matches_the_abi_path(renderer, tmp_path):
    """rayweek1_hip prints the reference's report block, writes out_<scene>.txt / .tga in the
    reference's formats, and its pixels equal what the C-ABI returns for the same parameters."""
    if KERNEL["variant"] != binding.VARIANT_DEFAULT:
        pytest.skip("runs the program's own kernel choice: once is enough")
    import re
    import subprocess
    exe = os.path.join(ROOT, "rays1bench_amd", "lib", "rayweek1_hip")
    w, h, spp = 160, 96, 3
    out = subprocess.run([exe, "-w", "-n", "2", "--width", str(w), "--height", str(h), "--spp", str(spp)], cwd=tmp_path,
                         capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    text = out.stdout.decode()
    for name in SCENES:
        blocks = re.findall(rf"^{name}\nelapsed time:   \d+\.\d{{3}}s\ntotal samples:  (\d+)\ntotal rays:     (\d+)\nmrays/s:        \d+\.\d\d\n",
                            text, flags=re.M)
        assert len(blocks) == 2 and all(int(b[0]) == w * h * spp for b in blocks)
        renderer.set_scene(MAKE[name](w, h))
        img, rays, _ = renderer.render(mp(w, h, spp, 10001))
        assert {int(b[1]) for b in blocks} == {rays}
        assert open(tmp_path / f"out_{name}.tga", "rb").read() == r1o.tga_bytes(img)
        assert re.fullmatch(rf"hip\|\d+\.\d{{3}}s\|{rays}\|\d+\.\d{{3}} mrays/s\|", open(tmp_path / f"out_{name}.txt").read())
        rec = json.load(open(tmp_path / f"out_{name}.json"))
        assert rec["scene"] == name and rec["devices"] == 1 and len(rec["runs"]) == 2 and rec["runs"][0]["num_rays"] == rays
        assert rec["algorithmic_bytes_per_ray"] == 16 * rec["spheres_padded"] and rec["fp32_vector_fraction_of_157TFs"] > 0
    # --devices 3: three contexts / host threads, each writing its own tiles (wraps onto the one GPU here)
    single = {n: open(tmp_path / f"out_{n}.tga", "rb").read() for n in SCENES}
    out3 = subprocess.run([exe, "-w", "--devices", "3", "--width", str(w), "--height", str(h), "--spp", str(spp)], cwd=tmp_path,
                          capture_output=True, timeout=300)
    assert out3.returncode == 0, out3.stderr.decode()
    assert "devices:        3" in out3.stdout.decode()
    for n in SCENES:
        assert open(tmp_path / f"out_{n}.tga", "rb").read() == single[n]
    rays1 = re.findall(r"total rays:     (\d+)", text)[::2]
    assert re.findall(r"total rays:     (\d+)", out3.stdout.decode()) == rays1


# ---- tiling is a pure work split: the image does not depend on it -----------------------------------


@pytest.mark.parametrize("tile_w,tile_h", [(32, 32), (16, 16), (64, 8), (24, 40), (7, 5), (128, 128)])
def test_image_is_independent_of_tile_size_and_matches_oracle(renderer, tile_w, tile_h):
    w, h, spp = 150, 90, 3
    sc = r1.create_medium_scene(w, h)
    renderer.set_scene(sc)
    p = mp(w, h, spp, 42, tile_w=tile_w, tile_h=tile_h)
    img, rays, samples = renderer.render_samples(p)
    oimg, orays, osamples = r1o.render_frame(oracle_scene(sc), oparams(mp(w, h, spp, 42)), want_samples=True)
    assert rays == orays
    assert samples.tobytes() == osamples.tobytes()
    assert img.tobytes() == oimg.tobytes()
    # and any shard count reassembles the same frame with that tile size
    acc = np.zeros_like(img)
    total = 0
    for s in range(3):
        part = np.zeros_like(img)
        total += renderer.render_into(mp(w, h, spp, 42, tile_w=tile_w, tile_h=tile_h, shard=s, num_shards=3), part)[0]
        acc = np.maximum(acc, part)
    assert total == rays and acc.tobytes() == img.tobytes()


def test_bad_arguments_are_rejected_not_rendered(renderer):
    renderer.set_scene(r1.create_small_scene(64, 64))
    for bad in (dict(width=0), dict(spp=0), dict(max_bounces=0), dict(max_bounces=52), dict(tile_w=0), dict(shard=2, num_shards=2),
                dict(num_shards=0)):
        kw = dict(width=64, height=64, spp=1, seed=1, max_bounces=50, tile_w=32, tile_h=32, shard=0, num_shards=1)
        kw.update(bad)
        with pytest.raises(r1.R1Error) as e:
            renderer.render(mp(**kw))
        assert e.value.code == binding.R1_EINVAL, bad
    fresh = r1.Renderer(0)
    with pytest.raises(r1.R1Error):
        fresh.render(mp(8, 8, 1))  # no scene set
    fresh.close()


# ---- bench.py's N > 1 path, rehearsed on one GPU -------------------------------------------------


def test_bench_two_ranks_rehearsal_gathers_the_unsharded_frame():
    """Two bench.py ranks share the one GPU (R1_BENCH_DEVICE=0) with gloo standing in for RCCL:
    real kernels, real tile split, the same gather_blocks/assemble code as the N-GPU run.
    --check compares the gathered + assembled image and ray count with an unsharded render."""
    if KERNEL["variant"] != binding.VARIANT_DEFAULT:
        pytest.skip("runs the program's own kernel choice: once is enough")
    import subprocess
    import sys
    env = dict(os.environ, R1_BENCH_DEVICE="0")
    # the BARE entry: bench.py starts its two ranks itself (fresh processes, before it touches HIP) and relays their line
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                          "--steps", "6", "--warmup", "2", "--inflight", "4", "--full", "--check", "--width", "300", "--height", "200", "--spp", "4"],
                         capture_output=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    line = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert line["check"] is True and line["n_gpus"] == 2 and line["scaling"] == "strong"
    assert "in page-locked HOST memory" in line["config"]["value_mode"]
    assert "cpu_baseline" not in line and line["roofline"]["bound"] == "valu" and 0 < line["roofline"]["frac"] <= 1
    assert line["value_device_resident"]["value"] > 0


def test_bench_rank_path_with_a_one_rank_rccl_communicator():
    """The rank path of bench.py on the one-GPU box: rank 0's tiles of a 4-GPU run (--emulate-shards 4), frame batches, the
    per-launch all-gather through a ONE-rank RCCL communicator (--rccl-selftest: torch.distributed backend nccl), records
    copied to the host.  What an N-GPU rank executes, minus the other ranks."""
    if KERNEL["variant"] != binding.VARIANT_DEFAULT:
        pytest.skip("runs the program's own kernel choice: once is enough")
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--emulate-shards", "4", "--rccl-selftest", "--steps", "40", "--warmup", "4",
                          "--no-cpu-baseline", "--no-extras", "--width", "300", "--height", "200", "--spp", "4"],
                         capture_output=True, timeout=600, cwd=ROOT, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")})
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    line = json.loads(out.stdout.decode().strip().splitlines()[-1])
    c = line["config"]
    assert c["emulated_shards"] == 4 and c["frames_per_launch"] == 2 and c["launches_in_flight"] == 10 and int(c["gpu_max_hw_queues"]) == 12
    assert 0 < c["local_rays_per_step"] == c["rays_per_step"] and line["value"] > 0


def test_bench_in_process_multi_mode_one_gpu():
    """bench.py --multi inproc: ONE process drives the GPUs through r1_multi_* (ncclCommInitAll + one ncclAllGather per
    frame); on the one-GPU box that is a one-rank communicator — the whole path, collective included."""
    if KERNEL["variant"] != binding.VARIANT_DEFAULT:
        pytest.skip("runs the program's own kernel choice: once is enough")
    import subprocess
    import sys
    for inflight, batch, mode in (("1", "0", "one synchronous frame"), ("4", "0", "4 frames in flight"), ("3", "2", "6 frames in flight")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--multi", "inproc", "--steps", "9", "--warmup", "2", "--batch", batch,
                              "--inflight", inflight, "--check", "--width", "300", "--height", "200", "--spp", "4"], capture_output=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        line = json.loads(out.stdout.decode().strip().splitlines()[-1])
        assert line["check"] is True and line["n_gpus"] == 1 and "r1_multi" in line["config"]["parallelism"] and mode in line["config"]["value_mode"]
        assert line["value"] > 0 and abs(line["value"] - line["config"]["rays_per_step"] / line["ms_per_step"] / 1e3) < 1e-6 * line["value"]


# ---- sphere-count edges: empty scene, last small-kernel scene, first big-kernel scene ------------


@pytest.mark.parametrize("n_active", [0, 1, 7, 8, 9, 1023, 1024])
def test_sphere_count_edges_vs_oracle(renderer, n_active, kernel_family):
    w, h, spp = 64, 48, 2
    src = r1.create_grid_scene(w, h, 36, 30)  # 1080 small spheres + ground + 3 big
    arr = src.arrays()
    keep = np.nonzero(arr["inv_radius"] != 0)[0][:n_active]
    sub = {k: v[keep] for k, v in arr.items()}
    # pad to a multiple of 8 with the reference's placeholders (rayweek1.cpp:574-576)
    pad = (-len(keep)) % 8 or (8 if len(keep) == 0 else 0)
    for k in sub:
        fill = {"center_x": 999999999.0, "center_y": 999999999.0, "center_z": 999999999.0, "mat_type": 255}.get(k, 0)
        sub[k] = np.concatenate([sub[k], np.full(pad, fill, sub[k].dtype)])
    sa = r1o.SceneArrays(sub, src.camera_array())
    renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
    p = mp(w, h, spp, 9)
    img, rays, samples = renderer.render_samples(p)
    assert renderer.launch_info()["spheres_active"] == n_active
    # DEFAULT = the box tree for every scene: a property of the build (round 3 timed scenes of 9..127 spheres when they were set)
    ran = renderer.launch_info()["kernel"]
    assert ran == (binding.VARIANT_PREFILTER if kernel_family != binding.VARIANT_DEFAULT else binding.VARIANT_BVH)
    sweep = renderer.render_samples(mp(w, h, spp, 9, variant=binding.VARIANT_PREFILTER))
    assert sweep[1] == rays and sweep[2].tobytes() == samples.tobytes()
    oimg, orays, osamples = r1o.render_frame(sa, oparams(p), want_samples=True)
    assert rays == orays
    assert samples.tobytes() == osamples.tobytes()
    assert img.tobytes() == oimg.tobytes()
    if n_active == 0:
        assert rays == w * h * spp  # every primary ray sees the sky


# ---- adversarial geometry for the conservative group prefilter -------------------------------------


@pytest.mark.parametrize("case", ["mixed_radii", "far_camera", "dense_cluster", "tiny_spheres", "nested"])
def test_grouped_prefilter_is_exact_on_random_scenes(renderer, case):
    """Random scenes that stress the slack analysis (radius ratios, |o| >> scene, touching and
    nested spheres): the default kernel (groups + prefilter) must be bit-identical to the
    REFERENCE-form kernel (every sphere, reference arithmetic) and to the oracle."""
    rng = np.random.default_rng({"mixed_radii": 1, "far_camera": 2, "dense_cluster": 3, "tiny_spheres": 4, "nested": 5}[case])
    w, h, spp = 72, 48, 3
    base = r1.create_small_scene(w, h)
    cam = base.camera_array().copy()
    n = 300
    if case == "mixed_radii":
        c = rng.uniform(-12, 12, (n, 3))
        rad = np.exp(rng.uniform(np.log(0.02), np.log(6.0), n))
    elif case == "far_camera":
        c = rng.uniform(-8, 8, (n, 3))
        rad = rng.uniform(0.2, 0.8, n)
        shift = np.array([700.0, 260.0, 410.0], np.float32)
        c = c + shift  # same view, everything far from the world origin: |o| and |c| ~ 850
        cam[0:3] += shift
        cam[3:6] += shift
    elif case == "dense_cluster":
        c = rng.normal(0, 1.2, (n, 3))
        rad = rng.uniform(0.05, 0.35, n)
    elif case == "tiny_spheres":
        c = rng.uniform(-3, 3, (n, 3))
        rad = np.exp(rng.uniform(np.log(1e-3), np.log(0.05), n))
    else:  # nested: shells around a few centres, equal centres with different radii
        centres = rng.uniform(-4, 4, (12, 3))
        c = centres[rng.integers(0, 12, n)]
        rad = rng.uniform(0.05, 2.5, n)
    c = c.astype(np.float32)
    rad = rad.astype(np.float32)
    mt = rng.integers(0, 3, n).astype(np.uint8)
    arr = {"center_x": c[:, 0].copy(), "center_y": c[:, 1].copy(), "center_z": c[:, 2].copy(), "radius_sq": rad * rad,
           "inv_radius": (np.float32(1.0) / rad).astype(np.float32), "mat_type": mt,
           "albedo_r": rng.uniform(0.1, 0.95, n).astype(np.float32), "albedo_g": rng.uniform(0.1, 0.95, n).astype(np.float32),
           "albedo_b": rng.uniform(0.1, 0.95, n).astype(np.float32),
           "mat_param": np.where(mt == 2, rng.uniform(1.1, 2.4, n), rng.uniform(0, 1, n)).astype(np.float32)}
    pad = (-n) % 8
    for k in arr:
        fill = {"center_x": 999999999.0, "center_y": 999999999.0, "center_z": 999999999.0, "mat_type": 255}.get(k, 0)
        arr[k] = np.concatenate([arr[k], np.full(pad, fill, arr[k].dtype)])
    sa = r1o.SceneArrays(arr, cam)
    renderer.set_scene_raw(_as_cscene(sa), _as_ccamera(sa))
    p = mp(w, h, spp, 1234)
    got = renderer.render_samples(p)
    ref = renderer.render_samples(mp(w, h, spp, 1234, variant=binding.VARIANT_REFERENCE))
    assert got[1] == ref[1] and got[2].tobytes() == ref[2].tobytes() and got[0].tobytes() == ref[0].tobytes()
    oimg, orays, osamples = r1o.render_frame(sa, oparams(p), want_samples=True)
    assert got[1] == orays and got[2].tobytes() == osamples.tobytes()
    assert renderer.launch_info()["groups"] <= n


# ---- INTEGRATION.md's binding, compiled against the real reference ---------------------------------


@pytest.mark.parametrize("name,count", [("small", 8), ("medium", 48), ("large", 488)])
def test_reference_scene_object_through_the_c_abi(name, count):
    """oracle/_ref/ref_step13_dropin (built in the container that has the reference sources) hands the
    reference's OWN Scene objects — create_small/medium/large_scene() of rayweek1.cpp, SoA arrays in place, materials
    flattened — to librays1.so through the C-ABI, and renders the same frame with the reference's own
    TileRenderScheduler on the host.  The GPU frame must equal what this repo's scene builders give
    for the same parameters (same arrays => same pixels), and agree statistically with the
    reference's irreproducible multi-threaded run (rays within 0.1 %)."""
    if KERNEL["variant"] != binding.VARIANT_DEFAULT:
        pytest.skip("one run is enough")
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_step13_dropin")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_step13_dropin not built (needs the reference sources at build time)")
    w, h, spp, seed = 1200, 800, 10, 10001
    out = subprocess.run([exe, "dropin", name, str(w), str(h), str(spp), str(seed), "0"], capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    rend = r1.Renderer(0)
    try:
        rend.set_scene(MAKE[name](w, h))
        img, rays, _ = rend.render(r1.make_params(w, h, spp, seed))
    finally:
        rend.close()
    fnv = 1469598103934665603
    for b in img.tobytes():
        fnv = ((fnv ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert rec["spheres"] == count
    assert rec["gpu_rays"] == rays
    assert int(rec["gpu_image_fnv1a"], 16) == fnv
    assert abs(rec["gpu_rays"] - rec["ref_cpu_rays"]) <= 1e-3 * rec["ref_cpu_rays"]
    assert abs(rec["gpu_image_mean"] - rec["ref_cpu_image_mean"]) < 0.5
