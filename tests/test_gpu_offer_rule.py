"""GPU test of the closest-offer update rule in the kernels (rays1bench_amd/csrc/r1_offer.h): every frame build of the
tree, the grid and the sweep that exists — enumerated as tests/test_gpu_builds.py does: the synchronous frame, r1_render_async, the same
in PIXEL mode, a batch of two, a camera path, a progressive pass from sample 0, and the family's diagnostic build — over the scenes in
which the rule decides the picture:

  coincident            tests/edge_scenes.py: six spheres per centre and radius — every hit an exact tie in t between different indices
  root twins, behind    tests/root_leaf_scenes.py, both table orders: two coincident balls in the root step's leaf (the lower index must
                        win, whether the leaf's indices are the scene's lowest or highest), and a root leaf behind the camera (flagged by
                        many rays, offered by none)
  leaf behind, n2, n4   tests/leaf_scenes.py: a one-pair leaf whose table neighbours stand behind it on the rays, a one-pair and a two-pair leaf
  large                 one 64 x 48 x 2 frame of the large scene (the benchmark's)

each of the modules' scenes in its small and its big size, at the modules' 64 x 48 frames and seeds.  Images and ray counts must equal,
byte for byte, the committed reference fixtures (tests/golden/ref_*.bin through tests/reference_cases.py: the small sizes) where one
exists, and the grouped exhaustive sweep's synchronous frames (R1_VARIANT_PREFILTER) otherwise: the big sizes and the large scene.
The ray queries: rays whose finite t_max equals a sphere's exact offer — the walks, seeded with best = t_max, admit t == t_max, and the
store rejects it — must miss, and hit that sphere again with t_max one float up; tree and grid against the reference form, every word."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

import edge_scenes as es
import leaf_scenes as ls
import reference_cases as rc
import root_leaf_scenes as rl

pytestmark = pytest.mark.gpu

F = np.float32
W, H = es.W, es.H
FAMILIES = {"sweep": binding.VARIANT_PREFILTER, "tree": binding.VARIANT_BVH, "grid": binding.VARIANT_GRID}
STATS = {"sweep": binding.VARIANT_STATS, "tree": binding.VARIANT_BVH_STATS, "grid": binding.VARIANT_GRID_STATS}
CALLS = ("sync", "async", "pixel", "batch", "path", "pass", "stats")

# id -> (build() -> (SceneArrays, second camera), seed, spp, stride, fixture case id or None)
SCENES = {}
for _size in es.SIZES:
    SCENES[f"coincident-{_size}"] = ((lambda s=_size: es.build("coincident", s)), es.SEED["coincident"], es.SPP, es.STRIDE,
                                     "edge-coincident" if _size == "small" else None)
    for _name in ("twins", "behind"):
        for _order in rl.ORDERS:
            SCENES[f"root-{_name}-{_order}-{_size}"] = ((lambda n=_name, o=_order, s=_size: rl.build(n, o, s)), rl.SEED, rl.SPP, rl.STRIDE,
                                                        f"root-{_name}-{_order}" if _size == "small" else None)
    for _name in ("behind", "n2", "n4"):
        SCENES[f"leaf-{_name}-{_size}"] = ((lambda n=_name, s=_size: ls.build(n, s)), ls.seed_of(_name), ls.SPP, ls.STRIDE,
                                           f"leaf-{_name}" if _size == "small" else None)
LARGE = "large"
LARGE_SEED, LARGE_SPP, LARGE_STRIDE = 10001, 2, 7


@pytest.fixture(scope="module")
def renderer():
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def large_scene():
    sc = r1.create_large_scene(W, H)
    yield sc
    sc.close()


def shape_of(sid):
    """(seed, spp, stride, bounces, fixture case or None)"""
    if sid == LARGE:
        return LARGE_SEED, LARGE_SPP, LARGE_STRIDE, 50, None
    _, seed, spp, stride, cid = SCENES[sid]
    return seed, spp, stride, 50, rc.BY_ID[cid] if cid else None


def set_scene(renderer, large_scene, sid):
    """Sets the scene; returns its two cameras as CCamera (the large scene and the scenes without a fixture: its own camera twice)."""
    if sid == LARGE:
        renderer.set_scene(large_scene)
        return [large_scene.camera.contents, large_scene.camera.contents]
    sa, cam2 = SCENES[sid][0]()
    renderer.set_scene_raw(es.cscene(sa), es.ccamera(sa.camera_array))
    return [es.ccamera(sa.camera_array), es.ccamera(cam2 if SCENES[sid][4] else sa.camera_array)]


def params(sid, variant, k=0):
    seed, spp, stride, bounces, _ = shape_of(sid)
    return r1.make_params(W, H, spp, seed + k * stride, max_bounces=bounces, tile_w=32, tile_h=32, variant=variant)


@pytest.fixture(scope="module")
def sweep_frames(renderer, large_scene):
    """sid -> [(image bytes, rays) of seed, of seed + stride]: the grouped exhaustive sweep's synchronous frames, for the scenes without a
    fixture; rendered on first use and left unchanged."""
    cache = {}

    def get(sid):
        if sid not in cache:
            set_scene(renderer, large_scene, sid)
            out = []
            for k in range(2):
                img, rays, _ = renderer.render(params(sid, binding.VARIANT_PREFILTER, k))
                assert rays > W * H * shape_of(sid)[1] or "behind" in sid
                out.append((img.tobytes(), int(rays)))
            assert renderer.launch_info()["kernel"] == binding.VARIANT_PREFILTER
            cache[sid] = out
        return cache[sid]

    return get


def run(renderer, cams, sid, call, family):
    """The frames of `call` as [(image, rays)]."""
    variant = STATS[family] if call == "stats" else FAMILIES[family]
    p = params(sid, variant)
    if call in ("sync", "stats"):
        img, rays, _ = renderer.render(p)
        got = [(img, rays)]
    elif call == "pass":
        img, rays = renderer.render_pass(p, 0)
        got = [(img, rays)]
    elif call in ("async", "pixel"):
        hf = binding.HostFrame(W, H)
        try:
            renderer.set_pixel_mode(call == "pixel")
            renderer.render_async(p, hf)
            renderer.sync()
            got = [(hf.image.copy(), hf.rays)]
        finally:
            renderer.set_pixel_mode(False)
            hf.close()
    else:
        hf = binding.HostFrames(W, H, 2)
        try:
            stride = shape_of(sid)[2]
            if call == "batch":
                renderer.render_batch_async(p, 2, hf, seed_stride=stride)
            else:
                renderer.render_path_async(p, cams, hf, seed_stride=stride)
            renderer.sync()
            got = [(hf.image(f).copy(), hf.rays(f)) for f in range(2)]
        finally:
            hf.close()
    assert renderer.launch_info()["kernel"] == variant
    return got


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("sid", list(SCENES) + [LARGE])
def test_every_frame_build_keeps_the_closest_offer_with_ties_to_the_lower_index(renderer, large_scene, sweep_frames, sid, family):
    case = shape_of(sid)[4]
    g = rc.fixture(case) if case else None
    want = None if case else sweep_frames(sid)
    cams = set_scene(renderer, large_scene, sid)
    for call in CALLS:
        got = run(renderer, cams, sid, call, family)
        for f, (img, rays) in enumerate(got):
            what = f"{sid}, {family}, {call}, frame {f}"
            if g is not None:
                rc.assert_frame(g, ("", "p1" if call == "path" else "b1")[f], img, rays, what)
            else:
                assert int(rays) == want[f][1], f"{what}: {int(rays)} rays, the exhaustive sweep counts {want[f][1]}"
                diff = int((np.ascontiguousarray(img, np.uint8).reshape(-1) != np.frombuffer(want[f][0], np.uint8)).sum())
                assert diff == 0, f"{what}: {diff} bytes differ from the exhaustive sweep's frame"


@pytest.mark.parametrize("sid", ["root-twins-front-small", "root-twins-back-small", "coincident-small", "root-twins-front-big"])
def test_a_t_max_equal_to_the_exact_offer_is_a_miss_and_one_float_up_a_hit(renderer, large_scene, sid):
    """r1_cast_rays with a finite t_max: the walks start at best = t_max, best_id = none, so the rule admits an offer EQUAL to t_max and the
    store's strict compare rejects it (r1_query_kernels.hip R1CastJob)."""
    sa, _ = SCENES[sid][0]()
    set_scene(renderer, large_scene, sid)
    free = es.primary_rays(sa.camera_array)
    ref = renderer.cast_rays(free, binding.CAST_CLOSEST, binding.VARIANT_REFERENCE)
    hit = np.nonzero(ref["index"] >= 0)[0]
    assert hit.size > 200, hit.size
    at, up = free[hit].copy(), free[hit].copy()
    at[:, 3] = ref["t"][hit]
    up[:, 3] = np.nextafter(ref["t"][hit], F(np.inf))
    if "twins" in sid:
        a, b = rl.outlier_ids("twins", sid.split("-")[2])[1:3]
        # the coincident balls: every hit on them is a tie in t, and the lower index wins (some rays must see them; how many, the fillers decide)
        assert (ref["index"][hit] == a).sum() > 0 and (ref["index"][hit] == b).sum() == 0
    want_at = renderer.cast_rays(at, binding.CAST_CLOSEST, binding.VARIANT_REFERENCE)
    want_up = renderer.cast_rays(up, binding.CAST_CLOSEST, binding.VARIANT_REFERENCE)
    # t == t_max is rejected by the strict compare: the ray misses the sphere it would hit, and whatever it reports lies strictly nearer — nothing does
    assert (want_at["index"] == -1).all()
    assert np.array_equal(want_up["index"], ref["index"][hit]) and want_up["t"].tobytes() == ref["t"][hit].tobytes()
    for tag, variant in (("tree", binding.VARIANT_BVH), ("grid", binding.VARIANT_GRID)):
        for rays, want, what in ((free, ref, "free"), (at, want_at, "t_max = t"), (up, want_up, "t_max = next float")):
            got = renderer.cast_rays(rays, binding.CAST_CLOSEST, variant)
            assert got.tobytes() == want.tobytes(), f"{sid}: r1_cast_rays, {tag}, {what}: records differ from the reference form's"
            occ = renderer.cast_rays(rays, binding.CAST_ANY, variant)
            assert occ.tobytes() == (want["index"] >= 0).astype(np.uint8).tobytes(), f"{sid}: r1_cast_rays ANY, {tag}, {what}"
