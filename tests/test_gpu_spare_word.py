"""GPU test of who holds a spare sample in the frames-in-flight tree kernels — r1_trace_kernel<4,false,false,TP>, its BATCH build and
r1_path_kernel<4,false> — written beside the attempt to read "this lane holds a spare" from the spare's own stream state instead of a
bool (measured, not kept; the kernels carry the bool).  It pins what either form must keep: a lane that takes a spare it
does not hold renders a sample twice or a stale one, a lane that never sees its spare loses one, and either shows in the pixels and in
the ray count.  The same three builds take §4.35's shade-phase changes through frames with ragged edges.

  scenes    large and medium at 96x64x4 and at the ragged 77x45x3 (edge tiles with void slots, sample counts no chunk size divides); large and
            medium at 200x100x4, the committed golden frames' shape
  routes    r1_render_async (TP), r1_render_batch_async of 3 frames (BATCH), r1_render_path_async over 3 cameras (PATH): the three builds
  against   one synchronous r1_render of the same frame (the latency build, which keeps no spare), byte for byte with the ray count, and the
            committed golden frames where one exists (frame_medium_77x45x3.bin, frame_*_200x100x4.bin)
  33x33x5   one full tile and three edge tiles of 1/32 live slots: a wave's chunk of the last tiles is nearly all void slots, so lanes ask twice
            and more for a spare, and the lanes still without one when the queue runs dry must end with none
  8x4x1     fewer samples than a wave has lanes

Every frame lands in a record filled with 0xCD.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import edge_scenes as es

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0xCD
STRIDE = 7
SCENES = {"large": r1.create_large_scene, "medium": r1.create_medium_scene}
# (scene, width, height, spp, golden file or None)
FRAMES = [(s, w, h, spp, None) for s in ("large", "medium") for (w, h, spp) in ((96, 64, 4), (77, 45, 3))]
FRAMES += [("large", 200, 100, 4, "frame_large_200x100x4.bin"), ("medium", 200, 100, 4, "frame_medium_200x100x4.bin"),
           ("large", 33, 33, 5, None), ("large", 8, 4, 1, None)]
FRAMES[3] = ("medium", 77, 45, 3, "frame_medium_77x45x3.bin")
ROUTES = ("async", "batch3", "path3")


def frame_id(f):
    return "%s_%dx%dx%d" % f[:4]


@pytest.fixture(scope="module")
def contexts():
    """(the context under test, the reference context)"""
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    rs = [r1.Renderer(0) for _ in range(2)]
    yield rs
    for r in rs:
        r.close()


def golden(name):
    g = r1o.read_golden(os.path.join(GOLD, name))
    w, h, spp, seed = g["hdr"].tolist()[:4]
    return (w, h, spp, seed), g["image"], int(g["rays"][0])


def base_seed(frame):
    return golden(frame[4])[0][3] if frame[4] else 61001 + 53 * FRAMES.index(frame)


def cameras(frame):
    """three cameras of a path: the scene's own, and two turned about the vertical axis"""
    sc = SCENES[frame[0]](frame[1], frame[2])
    try:
        cam = sc.camera_array().copy()
    finally:
        sc.close()
    return [cam, es.turned(cam, 3.0), es.turned(cam, -5.0)]


@pytest.fixture(scope="module")
def expected(contexts):
    """(frame, camera index, seed) -> (image bytes, rays) of one synchronous R1_VARIANT_BVH frame; rendered on first use, left unchanged"""
    cache = {}

    def get(frame, cam_index, seed):
        key = (frame[:4], cam_index, seed)
        if key not in cache:
            ref = contexts[1]
            name, w, h, spp, gold = frame
            sc = SCENES[name](w, h)
            ref.set_scene(sc)
            ref.set_camera(es.ccamera(cameras(frame)[cam_index]))
            img, rays, _ = ref.render(r1.make_params(w, h, spp, seed, variant=binding.VARIANT_BVH))
            info = ref.launch_info()
            assert info["kernel"] == binding.VARIANT_BVH and info["tiles_in_kernel"] == 0, info
            sc.close()
            if gold and cam_index == 0 and seed == golden(gold)[0][3]:
                shape, image, grays = golden(gold)
                assert shape[:3] == (w, h, spp)
                assert (img.tobytes(), rays) == (image.tobytes(), grays), (frame_id(frame), rays, grays)
            cache[key] = (img.tobytes(), rays)
        return cache[key]

    return get


def compare(tag, img, rays, want):
    print(f"{tag}: {rays} rays, the synchronous frame counts {want[1]}")
    assert rays == want[1], f"{tag}: {rays} rays, the synchronous frame counts {want[1]}"
    a, b = np.frombuffer(img.tobytes(), np.uint8), np.frombuffer(want[0], np.uint8)
    diff = int((a != b).sum())
    assert diff == 0, f"{tag}: {diff} bytes differ from the synchronous frame, {int((a == SENTINEL).sum())} at the sentinel"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("frame", FRAMES, ids=frame_id)
def test_the_three_trimmed_builds_equal_the_synchronous_frame(contexts, expected, frame, route):
    rend = contexts[0]
    name, w, h, spp, _ = frame
    seed = base_seed(frame)
    n = 1 if route == "async" else 3
    cams = cameras(frame)
    want = [expected(frame, f if route == "path3" else 0, seed + STRIDE * f) for f in range(n)]
    sc = SCENES[name](w, h)
    hf = binding.HostFrames(w, h, n)
    try:
        hf._all[:] = SENTINEL
        rend.set_scene(sc)
        p = r1.make_params(w, h, spp, seed, variant=binding.VARIANT_BVH)
        if route == "async":
            rend.render_async(p, hf)
        elif route == "batch3":
            rend.render_batch_async(p, 3, hf, seed_stride=STRIDE)
        else:
            rend.render_path_async(p, [es.ccamera(c) for c in cams], hf, seed_stride=STRIDE)
        rend.sync()
        info = rend.launch_info()
        assert info["kernel"] == binding.VARIANT_BVH and info["tiles_in_kernel"] == 1, info
        for f in range(n):
            compare(f"{frame_id(frame)} {route} frame {f}", hf.image(f), hf.rays(f), want[f])
    finally:
        hf.close()
        sc.close()
