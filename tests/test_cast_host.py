"""CPU tests of the ray queries (include/rays1.h "ray queries"): r1_cast_rays_host — every ray against every sphere in
the reference's arithmetic — pinned to the reference's OWN Hitable::hit through tests/golden/cast_{small,medium,large}.bin (written by
tools/gen_cast_golden.py from the reference's translation unit), bit for bit and for every ray; then the rules of the contract that the
fixtures cannot hold (non-finite rays, the t_max edge values), and the argument errors of the device entry points that need no device.
Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import r1o
from rays1bench_amd import binding

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("small", "medium", "large")
F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
CLASSES = (("camera", 1024), ("volume", 1024), ("scatter", 1024), ("axis", 512), ("grazing", 256), ("bounded", 256))


def scene_of(name):
    return r1o.SceneArrays.from_golden(r1o.read_golden(os.path.join(GOLD, f"scene_{name}_200x100.bin")))


def cscene(sa):
    """the binding's view of an r1o scene (same layout: r1_scene)"""
    return C.cast(C.pointer(sa.scene), C.POINTER(binding.CScene)).contents


def fixture(name):
    g = r1o.read_golden(os.path.join(GOLD, f"cast_{name}.bin"))
    return g["rays"].reshape(-1, 8), g


def assert_equals_fixture(hits, g, what):
    """index, t, p and n of every ray, bitwise"""
    n = hits.shape[0]
    assert n == g["index"].shape[0] == 4096
    assert hits["index"].astype(np.uint32).tobytes() == g["index"].tobytes(), what  # (-1 is 0xFFFFFFFF)
    assert hits["t"].tobytes() == g["t"].tobytes(), what
    assert np.ascontiguousarray(hits["p"]).tobytes() == g["p"].tobytes(), what
    assert np.ascontiguousarray(hits["n"]).tobytes() == g["n"].tobytes(), what


def test_struct_sizes_and_constants_follow_the_header():
    assert binding.RAY_DTYPE.itemsize == 32 and binding.HIT_DTYPE.itemsize == 32
    hdr = open(os.path.join(binding.HERE, "..", "include", "rays1.h")).read()
    assert "R1_CAST_CLOSEST = 0" in hdr and "R1_CAST_ANY = 1" in hdr and "#define R1_CAST_CHUNK (1u << 20)" in hdr
    assert (binding.CAST_CLOSEST, binding.CAST_ANY, binding.CAST_CHUNK) == (0, 1, 1 << 20)
    assert binding.HIT_DTYPE.fields["index"][1] == 4 and binding.HIT_DTYPE.fields["p"][1] == 8 and binding.HIT_DTYPE.fields["n"][1] == 20
    assert binding.RAY_DTYPE.fields["t_max"][1] == 12 and binding.RAY_DTYPE.fields["d"][1] == 16


@pytest.mark.parametrize("name", SCENES)
def test_fixture_is_what_the_generator_promises(name):
    """4096 rays in the documented classes; at least 5 % hits and 5 % misses in each of the first five; the miss records' form."""
    rays, g = fixture(name)
    assert rays.shape == (4096, 8) and rays.dtype == np.float32
    hit = g["index"] != 0xFFFFFFFF
    at = 0
    for cls, n in CLASSES:
        h = int(hit[at:at + n].sum())
        if cls != "bounded":
            assert h * 20 >= n and (n - h) * 20 >= n, (name, cls, h)
        at += n
    assert (g["t"][~hit] == FLT_MAX).all() and not g["p"].reshape(-1, 3)[~hit].any() and not g["n"].reshape(-1, 3)[~hit].any()


@pytest.mark.parametrize("name", SCENES)
def test_host_cast_equals_the_reference_on_every_ray(name):
    """What makes r1_cast_rays_host a checker: index, t, p and n of all 4096 fixture rays, bitwise; ANY bytes equal index >= 0."""
    sa = scene_of(name)
    rays, g = fixture(name)
    hits = binding.cast_rays_host(cscene(sa), rays, binding.CAST_CLOSEST)
    assert_equals_fixture(hits, g, name)
    occ = binding.cast_rays_host(cscene(sa), rays, binding.CAST_ANY)
    assert occ.dtype == np.uint8 and occ.tobytes() == (hits["index"] >= 0).astype(np.uint8).tobytes()
    # the structured input form is the same bytes
    again = binding.cast_rays_host(cscene(sa), rays.view(binding.RAY_DTYPE).reshape(-1), binding.CAST_CLOSEST)
    assert again.tobytes() == hits.tobytes()


@pytest.mark.parametrize("name", SCENES)
def test_t_max_is_strict(name):
    """t_max equal to the hit's own t is a miss, the next float above it the same hit, the next below a miss of that sphere's root; +inf
    is FLT_MAX; NaN, 0.001 and everything below give a miss."""
    sa = scene_of(name)
    rays, g = fixture(name)
    free = rays[:3840]
    hit = np.nonzero(g["index"][:3840] != 0xFFFFFFFF)[0]
    base, t = free[hit].copy(), g["t"][:3840][hit]
    ref = binding.cast_rays_host(cscene(sa), base)
    assert ref["t"].tobytes() == t.tobytes()

    r = base.copy()
    r[:, 3] = t
    assert (binding.cast_rays_host(cscene(sa), r)["index"] == -1).all()
    assert not binding.cast_rays_host(cscene(sa), r, binding.CAST_ANY).any()
    r[:, 3] = np.nextafter(t, FLT_MAX)
    assert binding.cast_rays_host(cscene(sa), r).tobytes() == ref.tobytes()
    r[:, 3] = np.inf
    assert binding.cast_rays_host(cscene(sa), r).tobytes() == ref.tobytes()
    r[:, 3] = np.nextafter(t, F(0))
    below = binding.cast_rays_host(cscene(sa), r)
    assert ((below["index"] == -1) | (below["t"] < r[:, 3])).all()
    for bad in (np.nan, F(0.001), np.nextafter(F(0.001), F(0)), F(0), F(-1), -np.inf):
        r[:, 3] = bad
        out = binding.cast_rays_host(cscene(sa), r)
        assert (out["index"] == -1).all() and (out["t"] == FLT_MAX).all() and not out["p"].any() and not out["n"].any(), bad
    # just above 0.001 the compare is made: nothing can lie in (0.001, t_max) unless a root does
    r[:, 3] = np.nextafter(F(0.001), F(1))
    assert (binding.cast_rays_host(cscene(sa), r)["index"] == -1).all()


def test_non_finite_rays_are_misses():
    """A non-finite component in o, or in d after normalisation (a zero direction, an infinite one, a NaN), is a miss in both modes."""
    sa = scene_of("large")
    rays, g = fixture("large")
    hit = np.nonzero(g["index"][:1024] != 0xFFFFFFFF)[0][:64]
    base = rays[hit].copy()
    cases = []
    for col in (0, 1, 2, 4, 5, 6):
        for v in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[:, col] = v
            cases.append(r)
    z = base.copy()
    z[:, 4:7] = 0.0
    cases.append(z)
    z = base.copy()
    z[:, 4:7] = -0.0
    cases.append(z)
    for r in cases:
        out = binding.cast_rays_host(cscene(sa), r)
        assert (out["index"] == -1).all() and (out["t"] == FLT_MAX).all() and not out["p"].any() and not out["n"].any()
        assert not binding.cast_rays_host(cscene(sa), r, binding.CAST_ANY).any()
    # the pad word is ignored
    p = base.copy()
    p.view(np.uint32)[:, 7] = 0xDEADBEEF
    assert binding.cast_rays_host(cscene(sa), p).tobytes() == binding.cast_rays_host(cscene(sa), base).tobytes()


def test_direction_is_normalised_as_the_ray_constructor_does():
    """d * (1 / sqrt(dot(d, d))) in fp32: p - o equals t times that direction, operation by operation."""
    sa = scene_of("medium")
    rays, g = fixture("medium")
    out = binding.cast_rays_host(cscene(sa), rays[:1024])
    h = out["index"] >= 0
    d = rays[:1024, 4:7]
    dot = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)
    scale = (F(1) / np.sqrt(dot.astype(F)).astype(F)).astype(F)
    du = (d * scale[:, None]).astype(F)
    p = (rays[:1024, 0:3] + (out["t"][:, None] * du).astype(F)).astype(F)
    assert p[h].tobytes() == np.ascontiguousarray(out["p"][h]).tobytes()


def test_placeholders_and_dead_spheres_are_never_returned():
    """inv_radius == 0 (rayweek1.cpp:291) — the reference's padding placeholders and any sphere a caller marks so — is never hit, and
    the index is the SCENE index (placeholders counted)."""
    sa = scene_of("small")
    rays, g = fixture("small")
    assert (sa.arrays["inv_radius"] == 0).any()  # the reference pads its arrays
    out = binding.cast_rays_host(cscene(sa), rays)
    h = out["index"][out["index"] >= 0]
    assert (sa.arrays["inv_radius"][h] != 0).all()
    # kill the most-hit sphere: no ray returns it any more, and the rays that never met it keep their answer
    victim = int(np.bincount(h).argmax())
    arrays = {k: v.copy() for k, v in sa.arrays.items()}
    arrays["inv_radius"][victim] = 0
    sb = r1o.SceneArrays(arrays, sa.camera_array)
    out2 = binding.cast_rays_host(cscene(sb), rays)
    assert (out2["index"] != victim).all()
    # a placeholder in FRONT of the others shifts no index: scene indices, not active ones
    arrays = {k: np.concatenate([v[-1:], v]) for k, v in sa.arrays.items()}
    assert arrays["inv_radius"][0] == 0
    sc = r1o.SceneArrays(arrays, sa.camera_array)
    out3 = binding.cast_rays_host(cscene(sc), rays)
    assert (out3["index"][out["index"] >= 0] == out["index"][out["index"] >= 0] + 1).all() and out3["t"].tobytes() == out["t"].tobytes()


def test_n_zero_order_and_thread_split():
    sa = scene_of("large")
    rays, g = fixture("large")
    L = binding.lib()
    assert L.r1_cast_rays_host(C.byref(cscene(sa)), 0, None, 0, None) == binding.R1_OK
    assert binding.cast_rays_host(cscene(sa), rays[:0]).shape == (0,)
    whole = binding.cast_rays_host(cscene(sa), rays)
    for n in (1, 63, 255, 256, 257, 1000):
        assert binding.cast_rays_host(cscene(sa), rays[:n]).tobytes() == whole[:n].tobytes(), n
    perm = np.random.default_rng(5).permutation(4096)
    assert binding.cast_rays_host(cscene(sa), rays[perm]).tobytes() == whole[perm].tobytes()


def test_argument_errors_without_a_device():
    L = binding.lib()
    sa = scene_of("small")
    rays, _ = fixture("small")
    out = np.zeros(4, binding.HIT_DTYPE)
    r = np.ascontiguousarray(rays[:4])
    E = binding.R1_EINVAL
    assert L.r1_cast_rays_host(C.byref(cscene(sa)), 2, r.ctypes.data, 4, out.ctypes.data) == E and b"mode" in L.r1_last_error()
    assert L.r1_cast_rays_host(C.byref(cscene(sa)), -1, r.ctypes.data, 4, out.ctypes.data) == E
    assert L.r1_cast_rays_host(None, 0, r.ctypes.data, 4, out.ctypes.data) == E
    assert L.r1_cast_rays_host(C.byref(cscene(sa)), 0, None, 4, out.ctypes.data) == E
    assert L.r1_cast_rays_host(C.byref(cscene(sa)), 0, r.ctypes.data, 4, None) == E
    # the device entry points: a NULL context is refused before anything is touched (no device needed)
    assert L.r1_cast_rays(None, 0, 0, r.ctypes.data, 4, out.ctypes.data) == E and b"ctx" in L.r1_last_error()
    assert L.r1_cast_rays_device(None, 0, 0, C.c_void_p(256), 4, C.c_void_p(512), None) == E and b"ctx" in L.r1_last_error()
    with pytest.raises(binding.R1Error):
        binding.cast_rays_host(cscene(sa), np.zeros((4, 7), np.float32))
    with pytest.raises(binding.R1Error):
        binding.cast_rays_host(cscene(sa), np.zeros((4, 8), np.float64))
