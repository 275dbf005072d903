"""CPU test of tests/edge_scenes.py: every scene, size, camera and seed that tests/test_gpu_builds_edges.py and
tests/test_gpu_cast_edges.py use is rendered by the oracle (r1o.render_frame with records), and the scene must show the property it is
there for in every such frame.  These are conditions, not tolerances: a GPU test over a scene that lost its property proves nothing.

Frames per (scene, size), all 64 x 48: `main` = the scene's camera at its seed, 6 samples (the adaptive call's cap; the 2-sample frame of
the other calls is its prefix), `batch1` = the same camera at seed + 7, 2 samples, `path1` = the turned camera at seed + 7, 2 samples.

Measured with the oracle (frames in the order main at 2 samples / batch1 / path1; seeds: deep 31 and 38, the others 4321 and 4328):

  deep       small  140 spheres,  48 nodes, pad global; samples with 33 < rays < 51 and colour 59 / 46 / 59; map at 128 / 8192 {2: 2, 4: 6, 6: 4}; cast rays that hit 65.6 %
  deep       big   1100 spheres, 197 nodes, pad per node; samples with 33 < rays < 51 and colour 67 / 49 / 67; map at 128 / 8192 {2: 2, 4: 5, 6: 5}; cast rays that hit 68.8 %
  palette    small   46 spheres,  14 nodes, pad global; channels with c * 255.99f >= 256 146 / 130 / 188 (at 6 samples 126), largest 331 / 305 / 331; map at 128 / 8192 {2: 4, 4: 3, 6: 5}; cast rays that hit 56.4 %
  palette    big   1100 spheres, 187 nodes, pad per node; channels with c * 255.99f >= 256 124 / 101 / 158 (at 6 samples 107), largest 331 / 305 / 331; map at 128 / 8192 {2: 3, 4: 3, 6: 6}; cast rays that hit 57.1 %
  coincident small  300 spheres,  99 nodes, pad global; samples with rays > 1 2388 / 2368 / 2234; primary hits on a sphere with twins 1191 / 1111; map at 128 / 8192 {2: 4, 4: 8}; cast rays that hit 33.9 %
  coincident big   1100 spheres, 188 nodes, pad global; samples with rays > 1 2552 / 2517 / 2397; primary hits on a sphere with twins 1167 / 1089; map at 128 / 8192 {2: 3, 4: 8, 6: 1}; cast rays that hit 37.6 %
  noise      small  300 spheres,  94 nodes, pad per node; samples with rays > 1 5013 / 5007 / 5012; map at 128 / 8192 {2: 3, 4: 6, 6: 3}; cast rays that hit 53.2 %
  noise      big   1100 spheres, 190 nodes, pad global; samples with rays > 1 5020 / 5012 / 5016; map at 128 / 8192 {2: 3, 4: 6, 6: 3}; cast rays that hit 53.9 %
  noise_lds  small  300 spheres,  98 nodes, pad global; samples with rays > 1 3108 / 3081 / 3107; primary hits on a 2e-3 sphere 563 / 576; map at 128 / 8192 {4: 3, 6: 9}; cast rays that hit 43.2 %
  noise_lds  big   1100 spheres, 193 nodes, pad per node; samples with rays > 1 4070 / 4080 / 4046; primary hits on a 2e-3 sphere 283 / 288; map at 128 / 8192 {4: 1, 6: 11}; cast rays that hit 47.1 %
  inside     small  140 spheres,  47 nodes, pad global; samples with rays > 1 6141 / 6139 / 6137; map at 128 / 8192 {2: 10, 4: 2}; cast rays that hit 56.5 %
  inside     big   1100 spheres, 192 nodes, pad per node; samples with rays > 1 6141 / 6139 / 6137; map at 128 / 8192 {2: 10, 4: 2}; cast rays that hit 55.5 %
  axis       small  200 spheres,  68 nodes, pad global; samples with rays > 1 6144 / 6144 / 6144; map at 128 / 8192 {4: 7, 6: 5}; cast rays that hit 52.9 %
  axis       big   1100 spheres, 202 nodes, pad global; samples with rays > 1 6144 / 6144 / 6144; map at 128 / 8192 {4: 7, 6: 5}; cast rays that hit 55.2 %
  far        small  200 spheres,  71 nodes, pad global; samples with rays > 1 2627 / 2641 / 2549; map at 128 / 8192 {2: 2, 4: 8, 6: 2}; cast rays that hit 44.0 %
  far        big   1100 spheres, 200 nodes, pad per node; samples with rays > 1 2696 / 2704 / 2634; map at 128 / 8192 {2: 2, 4: 6, 6: 4}; cast rays that hit 44.8 %

No record of any frame holds a NaN or an Inf.

Rays per sample in `deep`, 6144 samples per frame (a sample of r rays stacks r - 1 attenuations; the frames are those the async, pixel,
batch and path calls render):

                          1    2-9  10-19  20-31  32-39  40-50     51   more than 19
  small main at 2       331    142    109     74     47     43   5398       5562
  small batch1          329    115     96     79     34     36   5455       5604
  small path1           312    117    113     66     46     37   5453       5602
  big   main at 2       292    168    125    104     49     57   5349       5559
  big   batch1          289    137    117     90     45     40   5426       5601
  big   path1           283    144    118     81     49     44   5425       5599
"""
import numpy as np
import pytest

import r1o
from rays1bench_amd import binding

import adaptive_rule as rule
import edge_scenes as es

CASES = [(name, size) for name in es.SCENES for size in es.SIZES]
KEYS = ("main", "batch1", "path1")


def frame_records(name, size):
    """[(key, rec of the smallest frame the GPU tests render from that run: SPP samples)]: counts only grow with more samples"""
    fr = es.frames(name, size)
    return [(k, fr[k][0][:, :, :es.SPP]) for k in KEYS]


def deep_and_lit(rec):
    rw = es.ray_words(rec)
    return int(((rw > 33) & (rw < 51) & (rec[..., :3].sum(-1) > 0)).sum())


def wrapped(rec):
    return es.scaled(rec, rec.shape[2]) >= 256


def primary_hits(name, size, camera):
    sa, cam2 = es.build(name, size)
    return binding.cast_rays_host(es.cscene(sa), es.primary_rays(cam2 if camera else sa.camera_array))["index"]


def rule_map(name, size):
    rep, rays = rule.restate(es.frames(name, size)["main"][0], es.MIN_SPP, es.PASS_SPP, *es.RULE, es.ADAPT_TILE, es.ADAPT_TILE)
    return rep, rays


@pytest.mark.parametrize("name", es.SCENES)
def test_sizes_fillers_and_second_camera(name):
    small, cam2 = es.build(name, "small")
    big, cam2_big = es.build(name, "big")
    info, _, _ = binding.bvh_describe(es.cscene(small))
    assert es.active(small) <= 1023 and info["nodes"] <= 256, (es.active(small), info["nodes"])
    # a tree that measures its pad per node (median radius tiny) runs through the big-scene tree kernels whatever its size: of the small
    # sizes only `noise` does, and `noise_lds` is there to take hits by rounding alone through the small-scene tree kernels
    assert info["pad_local"] == (1 if name == "noise" else 0), info
    assert es.active(big) == es.BIG_ACTIVE > 1023
    # the big size is the small one plus fillers behind it: same spheres at the same indices, same cameras
    n0 = es.active(small)
    assert (small.arrays["inv_radius"][:n0] != 0).all()
    for k, v in small.arrays.items():
        assert v[:n0].tobytes() == big.arrays[k][:n0].tobytes(), k
    assert small.camera_array.tobytes() == big.camera_array.tobytes() and cam2.tobytes() == cam2_big.tobytes()
    a = big.arrays
    fill = slice(n0, es.BIG_ACTIVE)
    rad = np.sqrt(a["radius_sq"][fill].astype(np.float64))
    assert (a["inv_radius"][fill] != 0).all() and rad.min() >= 0.0099 and rad.max() <= 0.0601, (rad.min(), rad.max())
    c = np.stack([a["center_x"][fill], a["center_y"][fill], a["center_z"][fill]], 1).astype(np.float64)
    # clear of the first metre of every ray that leaves the cameras' (common) origin
    assert (np.linalg.norm(c - big.camera_array[0:3].astype(np.float64), axis=1) - rad).min() > 1.0
    assert (a["inv_radius"][es.BIG_ACTIVE:] == 0).all() and big.count % 8 == 0 and small.count % 8 == 0
    # the second camera: the same origin, the view a few degrees off
    cam = small.camera_array.astype(np.float64)
    assert cam2[0:3].tobytes() == small.camera_array[0:3].tobytes()
    mid = lambda q: q[3:6] + 0.5 * q[6:9] + 0.5 * q[9:12] - q[0:3]
    d0, d1 = mid(cam), mid(cam2.astype(np.float64))
    angle = np.degrees(np.arccos(np.dot(d0, d1) / np.linalg.norm(d0) / np.linalg.norm(d1)))
    # (`noise_lds` sees half a degree in all: its second camera is a tenth of that off)
    assert (0.03 < angle < 0.07) if name == "noise_lds" else (2.0 < angle < 6.0), angle


@pytest.mark.parametrize("name,size", CASES)
def test_records_are_finite_and_prefixes_are_frames(name, size):
    """No NaN or Inf anywhere (so records can be compared as bytes), and the restated resolve (tests/adaptive_rule.py: quantise) on a
    run's records gives the oracle's own image — at the run's spp and, for `main`, at the 2-sample prefix the other calls render."""
    fr = es.frames(name, size)
    for k in KEYS:
        rec, img = fr[k]
        assert np.isfinite(rec[..., :3]).all(), k
        got, rays = es.prefix_frame(rec, rec.shape[2])
        assert got.tobytes() == img.tobytes(), k
    sa, _ = es.build(name, size)
    img2, rays2, _ = r1o.render_frame(sa, r1o.make_params(es.W, es.H, es.SPP, es.SEED[name]))
    got, rays = es.prefix_frame(fr["main"][0], es.SPP)
    assert rays == rays2 and got.tobytes() == img2.tobytes()
    # the frames of a batch or path differ from frame 0: rendering frame 0 twice would show
    assert fr["batch1"][1].tobytes() != img2.tobytes() and fr["path1"][1].tobytes() != fr["batch1"][1].tobytes()


@pytest.mark.parametrize("size", es.SIZES)
def test_deep_paths_stack_more_than_30_attenuations_and_escape_lit(size):
    for k, rec in frame_records("deep", size):
        assert deep_and_lit(rec) > 20, (k, deep_and_lit(rec))


@pytest.mark.parametrize("size", es.SIZES)
def test_palette_wraps_bytes(size):
    fr = es.frames("palette", size)
    for k in KEYS:
        rec, img = fr[k]
        for n in sorted({es.SPP, rec.shape[2]}):
            r = rec[:, :, :n]
            over = wrapped(r)
            assert int(over.sum()) >= 100, (k, n, int(over.sum()))
            image = es.prefix_frame(rec, n)[0]  # (the oracle's image: test_records_are_finite_and_prefixes_are_frames)
            v = es.scaled(r, n)[over].astype(np.int64)
            assert (image[over] == (v & 255)).all() and (v >= 256).all()
    sa, _ = es.build("palette", size)
    m = sa.arrays
    assert ((m["mat_type"] == 2) & (m["mat_param"] <= 1) & (m["mat_param"] > 0)).sum() >= 9  # indices at and below 1
    assert ((m["mat_type"] == 1) & (m["mat_param"] == 0)).any() and ((m["mat_type"] == 1) & (m["mat_param"] == 1)).any()
    assert ((m["mat_type"] == 0) & (m["albedo_r"] == 0) & (m["albedo_g"] == 0) & (m["albedo_b"] == 0)).any() and m["albedo_r"].max() > 1


@pytest.mark.parametrize("name,size", [c for c in CASES if c[0] not in ("deep", "palette")])
def test_paths_bounce(name, size):
    for k, rec in frame_records(name, size):
        bounced = int((es.ray_words(rec) > 1).sum())
        assert bounced >= 20, (k, bounced)


@pytest.mark.parametrize("size", es.SIZES)
def test_noise_lds_primary_rays_hit_by_rounding_alone(size):
    """At least 20 primary rays of either camera hit one of the 2e-3 spheres 600 units out, whose 140 discs together cover less than a
    fifth of one pixel."""
    sa, _ = es.build("noise_lds", size)
    far = slice(0, es.NOISE_LDS_FAR)
    assert (sa.arrays["radius_sq"][far] == np.float32(2e-3) ** 2).all()
    c = np.stack([sa.arrays[k][far] for k in ("center_x", "center_y", "center_z")], 1).astype(np.float64)
    dist = np.linalg.norm(c - sa.camera_array[0:3], axis=1)
    assert dist.min() > 590
    pixel = np.linalg.norm(sa.camera_array[6:9].astype(np.float64)) / es.W  # a pixel's width at the focus distance, the cluster's
    assert es.NOISE_LDS_FAR * np.pi * 2e-3 ** 2 < pixel ** 2 / 5
    for camera in (0, 1):
        idx = primary_hits("noise_lds", size, camera)
        assert int(((idx >= 0) & (idx < es.NOISE_LDS_FAR)).sum()) >= 20, camera


@pytest.mark.parametrize("size", es.SIZES)
def test_inside_no_primary_ray_escapes(size):
    for k, rec in frame_records("inside", size):
        one = es.ray_words(rec) == 1
        assert (rec[..., :3][one] == 0).all(), k
    sa, _ = es.build("inside", size)
    a = sa.arrays
    o = sa.camera_array[0:3].astype(np.float64)
    assert ((o - [a["center_x"][0], a["center_y"][0], a["center_z"][0]]) ** 2).sum() < a["radius_sq"][0] == 2500 and a["mat_type"][0] == 0


@pytest.mark.parametrize("size", es.SIZES)
def test_coincident_ties_go_to_the_lowest_index(size):
    sa, _ = es.build("coincident", size)
    a = sa.arrays
    for k in ("center_x", "center_y", "center_z", "radius_sq"):
        assert (a[k][:300].reshape(50, 6) == a[k][:300:6, None]).all(), k
    for camera in (0, 1):
        idx = primary_hits("coincident", size, camera)
        twins = idx[(idx >= 0) & (idx < 300)]
        assert twins.size >= 20, (camera, twins.size)
        assert (twins % 6 == 0).all(), camera


@pytest.mark.parametrize("size", es.SIZES)
def test_axis_primary_directions_are_bit_equal(size):
    sa, cam2 = es.build("axis", size)
    assert not sa.camera_array[6:12].any() and not cam2[6:12].any() and sa.camera_array[21] == 0
    for cam in (sa.camera_array, cam2):
        d = es.primary_rays(cam)[:, 4:7]
        assert (d.view(np.uint32) == d[0].view(np.uint32)).all()
    assert es.primary_rays(sa.camera_array)[0, 4:7].tolist() == [0.0, 0.0, -1.0]


@pytest.mark.parametrize("name,size", CASES)
def test_the_adaptive_map_is_not_degenerate(name, size):
    rep, rays = rule_map(name, size)
    assert len(rep) == 12
    hist = rule.histogram(rep)
    assert len(hist) >= 2 and min(hist) < es.CAP, hist
    assert 0 < rays < int(es.ray_words(es.frames(name, size)["main"][0]).sum())


@pytest.mark.parametrize("name,size", CASES)
def test_primary_and_scatter_rays_hit_and_miss(name, size):
    """The ray set of tests/test_gpu_cast_edges.py: 20 - 80 % of its rays hit and the bounded class sits on the hits' own roots."""
    rays = es.cast_rays(name, size)
    sa, _ = es.build(name, size)
    assert rays.shape == (4096, 8) and np.isfinite(rays[:, :3]).all() and np.isfinite(rays[:, 4:7]).all()
    hits = binding.cast_rays_host(es.cscene(sa), rays)
    frac = float((hits["index"] >= 0).mean())
    assert es.CAST_HIT_FRACTION == (0.2, 0.8) and 0.2 <= frac <= 0.8, frac
    # bounded rays: t_max == t misses that root, the float above it finds it again
    b = slice(es.CAST_RAYS - es.CAST_BOUNDED, es.CAST_RAYS)
    k = np.arange(es.CAST_BOUNDED) % 3
    assert (hits["t"][b][k == 2] < rays[b][k == 2, 3]).all() and (hits["index"][b][k == 2] >= 0).all()
    assert ((hits["index"][b][k == 0] < 0) | (hits["t"][b][k == 0] < rays[b][k == 0, 3])).all()
