"""What tests/test_region_host.py and tests/test_gpu_region.py share (region renders, include/rays1.h): the scenes and frames, the
tilings, the variants, the windows, and the expected values — crops of whole-frame results, and the oracle's per-sample restatement
(oracle/r1o.py trace_samples) summed in numpy as tests/linear_cases.py sums.  Nothing here has a tolerance."""
import numpy as np

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

import linear_cases as lc

SEED = lc.SEED
GRID = "grid40x30"  # create_grid_scene(w, h, 40, 30): 1 200 lattice spheres, above the 10-bit limit: the big-scene kernels
# (scene, width, height, spp)
FRAMES = [("small", 64, 48, 1), ("medium", 77, 45, 3), ("large", 200, 100, 4), (GRID, 64, 48, 2)]
TILINGS = [(32, 32), (16, 8), (40, 24)]
VARIANTS = {"default": binding.VARIANT_DEFAULT, "reference": binding.VARIANT_REFERENCE, "prefilter": binding.VARIANT_PREFILTER, "bvh": binding.VARIANT_BVH,
            "grid": binding.VARIANT_GRID}
REFUSED_VARIANTS = (binding.VARIANT_STATS, binding.VARIANT_BVH_STATS, binding.VARIANT_WAVEFRONT, binding.VARIANT_GRID_STATS)
HUGE = (40000, 40000, 2)  # a frame r1_render refuses: 3.2e9 samples
HUGE_WINDOWS = [(39991, 39993, 9, 7), (0, 0, 8, 8)]
PREFILL = 0xCD


def make_scene(name, w, h):
    return r1.create_grid_scene(w, h, 40, 30) if name == GRID else lc.SCENES[name](w, h)


def windows(w, h):
    """The windows of a w x h frame (every frame here is at least 64 x 45): the full frame; off-origin over four 32 x 32 tiles with void slots;
    2 x 2 across the corner (32, 32) of the frame's own 32 x 32 grid — a region whose grid were the frame's would cut it into four tiles —;
    one whole tile off the origin; the last pixel; the top row; the last column, taller than a tile."""
    return [(0, 0, w, h), (5, 3, 33, 33), (31, 31, 2, 2), (32, 0, 32, 32), (w - 1, h - 1, 1, 1), (0, h - 1, w, 1), (w - 1, 0, 1, h)]


def crop(a, win):
    """rows y0 .. y0 + h, columns x0 .. x0 + w of an image-shaped array (row 0 = bottom row, as everywhere)"""
    x0, y0, w, h = win
    return np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])


def records_of(samples, w, h, spp):
    """r1_render_samples' records as (h, w, spp, 4)"""
    return samples.reshape(h, w, spp, 4)


def count_of(rec):
    """the sum of the count words of records (..., 4) float32"""
    return int(np.ascontiguousarray(rec[..., 3]).view(np.uint32).astype(np.uint64).sum())


def oracle_window(sa, w, h, spp, win, seed=SEED):
    """The oracle's restatement of a window of the w x h frame, sample by sample at the frame's own geometry: records (wh, ww, spp, 4) with the count
    as the fourth word's bits, the linear value summed as tests/linear_cases.py sums, the bytes, and the count."""
    x0, y0, ww, wh = win
    ys, xs, ss = np.meshgrid(np.arange(y0, y0 + wh), np.arange(x0, x0 + ww), np.arange(spp), indexing="ij")
    rgb, rays = r1o.trace_samples(sa, w, h, seed, xs.reshape(-1), ys.reshape(-1), ss.reshape(-1))
    rec = np.zeros((wh, ww, spp, 4), np.float32)
    rec[..., :3] = rgb.reshape(wh, ww, spp, 3)
    rec[..., 3] = rays.astype(np.uint32).view(np.float32).reshape(wh, ww, spp)
    lin = lc.linear_of(rec)
    return rec, lin, lc.quantise(lin), int(rays.astype(np.uint64).sum())
