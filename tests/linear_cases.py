"""What tests/test_linear_host.py and tests/test_gpu_linear.py share (linear frames, include/rays1.h): the value restated in
numpy on the ORACLE's per-sample records, the frames both files use, and the adaptive frame whose rule the host file shows to stop some
tiles early and run others into the cap — so that the GPU file's adaptive case cannot pass on a map without both."""
import ctypes as C
import functools

import numpy as np

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

SEED = 10001
SCENES = {"small": r1.create_small_scene, "medium": r1.create_medium_scene, "large": r1.create_large_scene}
# (scene, width, height, spp): ragged tiles with an odd spp; one sample (inv = 1); the fixtures' size; one tile and a bit, 7 samples
FRAMES = [("medium", 77, 45, 3), ("small", 64, 48, 1), ("large", 200, 100, 4), ("medium", 33, 33, 7)]
TILES = [(32, 32), (16, 8), (40, 24)]

# The adaptive frame: medium 77 x 45, cap 12, passes of 4; per tile size a rule (max_delta, mean_delta_q8) under which the restated rule
# (tests/adaptive_rule.py) on the oracle's records stops tiles at 4 or 8 samples AND runs tiles into the cap (test_linear_host.py asserts it).
ADAPTIVE_FRAME = ("medium", 77, 45, 12)
ADAPTIVE_MIN, ADAPTIVE_PASS = 4, 4
ADAPTIVE_RULES = {(16, 8): (48, 1536), (32, 32): (48, 1536), (40, 24): (64, 65280)}


def cscene(sa):
    return C.cast(C.pointer(sa.scene), C.POINTER(binding.CScene)).contents


def ccamera(sa):
    return C.cast(C.pointer(sa.camera), C.POINTER(binding.CCamera)).contents


def scene_arrays(name, w, h):
    sc = SCENES[name](w, h)
    return r1o.SceneArrays.from_c(sc.spheres, sc.camera)


@functools.lru_cache(maxsize=None)
def oracle_records(name, w, h, spp, seed=SEED):
    """The oracle's records of the frame, (h, w, spp, 4) float32, and its ray count; computed once and left unchanged."""
    _, rays, samples = r1o.render_frame(scene_arrays(name, w, h), r1o.make_params(w, h, spp, seed), want_samples=True)
    rec = samples.reshape(h, w, spp, 4)
    rec.setflags(write=False)
    return rec, rays


def linear_of(rec, n=None):
    """The contract on records (h, w, >= n, 4): S = 0.0f; S += radiance(sample s) for s < n, in float32; L = S * (float32(1) / float32(n))."""
    n = rec.shape[2] if n is None else n
    acc = np.zeros(rec.shape[:2] + (3,), np.float32)
    for s in range(n):
        acc = acc + rec[:, :, s, :3]
    out = acc * (np.float32(1) / np.float32(n))
    assert out.dtype == np.float32
    return out


def same_bits(a, b):
    """float32 arrays equal bit for bit, as uint32 views"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def quantise(linear):
    """identity 2 in numpy: (uint8)(int)(sqrtf(L) * 255.99f)"""
    return (np.sqrt(np.ascontiguousarray(linear, np.float32)) * np.float32(255.99)).astype(np.int32).astype(np.uint8)
