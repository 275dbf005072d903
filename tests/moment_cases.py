"""What tests/test_moments_host.py and tests/test_gpu_moments.py share (variance frames, include/rays1.h): the contract restated
in numpy on per-sample records — whole-frame float32 operations written from the header's text — and the host form's frames, computed once.
The frames, tiles and seed are tests/linear_cases.py's."""
import functools

import numpy as np

import rays1bench_amd as r1
from rays1bench_amd import binding

import linear_cases as lc


def moments_of(rec, n=None):
    """The contract on records (h, w, >= n, 4): L as lc.linear_of; D = 0.0f, then d = x_s - L; D = D + d * d for s < n, in sample order;
    var = n > 1 ? D * (1.0f / ((float)n * (float)(n - 1))) : +0.0f.  Returns (L, MOMENT_DTYPE array (h, w))."""
    n = rec.shape[2] if n is None else n
    L = lc.linear_of(rec, n)
    D = np.zeros(rec.shape[:2] + (3,), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):  # (records that are not finite propagate by IEEE rules)
        for s in range(n):
            d = rec[:, :, s, :3] - L
            D = D + d * d
    assert D.dtype == np.float32
    mom = np.zeros(rec.shape[:2], binding.MOMENT_DTYPE)
    if n > 1:
        scale = np.float32(1) / (np.float32(n) * np.float32(n - 1))
        assert scale.dtype == np.float32
        mom["var"] = D * scale
    mom["samples"] = n
    return L, mom


def same_records(a, b):
    """two MOMENT_DTYPE arrays equal byte for byte"""
    return a.dtype == b.dtype == binding.MOMENT_DTYPE and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


@functools.lru_cache(maxsize=None)
def host_frame(name, w, h, spp, seed=lc.SEED):
    """r1_render_moments_host of the frame: (L, moments, ray count), computed once and left unchanged"""
    sc = lc.SCENES[name](w, h)
    lin, mom, rays = binding.render_moments_host(sc.spheres.contents, sc.camera.contents, r1.make_params(w, h, spp, seed))
    lin.setflags(write=False), mom.setflags(write=False)
    return lin, mom, rays
