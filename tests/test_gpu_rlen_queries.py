"""The reciprocal length of r1_exact_math.h inside a kernel: r1_cast_rays and r1_trace_rays normalise caller-supplied
directions with the trace kernels' own vunit — the branch-free total form — so directions whose squared length is zero, subnormal, tiny,
at both sides of 2^-96, ordinary or overflowed reach every arm of it.  Hits, t and radiance must have the bits of r1_cast_rays_host /
r1_trace_rays_host (the host's 1.0f / sqrtf), through the box tree, the uniform grid and the reference form.

A few hundred rays on the small scene: per length 32 rays aimed at the spheres and one axis-parallel ray.  This is the smallest shape at
which a wrong arm shows in a kernel; all 2^32 inputs of the function itself are tests/test_gpu_exact_rlen.py's."""
import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding
from test_gpu_cast import same_hits

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = np.finfo(F).max
VARIANTS = (binding.VARIANT_DEFAULT, binding.VARIANT_GRID, binding.VARIANT_REFERENCE)
# |d|: x = |d|^2 is 0 (2^-150: every square rounds to zero), subnormal (2^-140), tiny (2^-120), just below 2^-96 (2^-98), in D (2^-94, 1,
# 2^120), overflowed (2^130); and d = 0
EXPONENTS = (-75, -70, -60, -49, -47, 0, 60, 65)
PER_LENGTH = 32


def squared_length(d):
    """x as vdot computes it: (x x + y y) + z z, every step rounded to fp32"""
    with np.errstate(over="ignore", under="ignore"):
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


@pytest.fixture(scope="module")
def case():
    """the scene, the rays, their stream states and the host's answers, computed once"""
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    sc = r1.create_small_scene(96, 64)
    a = sc.arrays()
    rng = np.random.default_rng(1623)
    real = np.nonzero((a["inv_radius"] != 0) & np.isfinite(a["center_x"]))[0]
    c = np.stack([a["center_x"], a["center_y"], a["center_z"]], 1).astype(np.float64)[real]
    o = sc.camera_array().astype(np.float64)[0:3]
    aim = c[rng.integers(0, c.shape[0], PER_LENGTH)] + rng.uniform(-0.3, 0.3, (PER_LENGTH, 3)) - o
    aim = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(F)  # (about unit: the power of two below sets the length, exactly)
    down = c[np.argmin(np.abs(c[:, 1] - 1.0))] + np.array([0.0, 5.0, 0.0])  # above a sphere that stands on the ground
    blocks = []
    for e in EXPONENTS + (None,):
        scale = F(0.0) if e is None else F(2.0) ** F(e)
        rays = np.zeros((PER_LENGTH + 1, 8), F)
        rays[:, 3] = FLT_MAX
        rays[:PER_LENGTH, 0:3], rays[:PER_LENGTH, 4:7] = o.astype(F), aim * scale
        rays[PER_LENGTH, 0:3], rays[PER_LENGTH, 4:7] = down.astype(F), np.array([0.0, -1.0, -0.0], F) * scale
        blocks.append(rays)
    rays = np.ascontiguousarray(np.concatenate(blocks))
    seeds = rng.integers(1, 1 << 32, (rays.shape[0], 4), dtype=np.uint64).astype(np.uint32)
    cs = sc.spheres.contents
    rend = r1.Renderer(0)
    rend.set_scene(sc)
    yield {"renderer": rend, "rays": rays, "seeds": seeds, "hits": binding.cast_rays_host(cs, rays),
           "any": binding.cast_rays_host(cs, rays, binding.CAST_ANY), "radiance": binding.trace_rays_host(cs, rays, seeds, 50)}
    rend.close()


def test_the_rays_reach_every_class_of_squared_length(case):
    x = squared_length(case["rays"][:, 4:7]).reshape(len(EXPONENTS) + 1, PER_LENGTH + 1)
    tiny_normal, edge = F(2.0) ** F(-126), F(2.0) ** F(-96)
    assert (x[0] == 0).all()                                                                        # 2^-75: zero
    assert ((x[1] > 0) & (x[1] < tiny_normal)).all()                                                # 2^-70: subnormal
    assert ((x[2] >= tiny_normal) & (x[2] < F(2.0) ** F(-110))).all()                               # 2^-60: tiny
    assert (x[3] < edge).all() and (x[3] > edge / F(16)).all()                                      # 2^-49: just below 2^-96
    assert (x[4] >= edge).all() and (x[4] < edge * F(16)).all()                                     # 2^-47: just inside D
    assert (np.abs(x[5] - 1) < 1e-5).all() and np.isfinite(x[6]).all()                              # 1 and 2^60: in D
    assert np.isinf(x[7]).all() and (x[8] == 0).all()                                               # 2^65: overflowed; d = 0
    # and the host's answers are not all misses: the short lengths still aim at the spheres once normalised
    hit = (case["hits"]["index"] >= 0).reshape(x.shape)
    assert hit[1:7].sum(1).min() >= PER_LENGTH // 2 and hit[1:7, PER_LENGTH].all(), hit.sum(1)
    assert not hit[0].any() and not hit[8].any()  # 1 / sqrt(0) = inf, 0 x inf = NaN: a miss (tests/test_cast_host.py)
    paths = case["radiance"]["rays"].reshape(x.shape)
    assert (paths[1:7] >= 1).all() and (paths[1:7] >= 2).any() and not paths[0].any() and not paths[8].any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_casts_of_scaled_directions_equal_the_host(case, variant):
    same_hits(case["renderer"].cast_rays(case["rays"], binding.CAST_CLOSEST, variant), case["hits"], variant)
    same_hits(case["renderer"].cast_rays(case["rays"], binding.CAST_ANY, variant), case["any"], (variant, "any"))


@pytest.mark.parametrize("variant", VARIANTS)
def test_paths_of_scaled_directions_equal_the_host(case, variant):
    got = case["renderer"].trace_rays(case["rays"], case["seeds"], 50, variant)
    want = case["radiance"]
    if got.tobytes() != want.tobytes():
        bad = np.unique(np.nonzero(got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4))[0])
        raise AssertionError(f"variant {variant}: {bad.size} of {got.shape[0]} records differ, first at {bad[:8]}: {got[bad[:3]]} != {want[bad[:3]]}")
