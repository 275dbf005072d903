"""CPU tests of the scatter queries (include/rays1.h "scatter queries"): r1_scatter_rays_host is one color() level, and the
fold of its levels — done here in NumPy float32, with none of the library's own trace — is a sample's record: pinned to the reference's own
color() through tests/golden/samples_*.bin (34 000 records) and tests/golden/ref_scatter_*.bin (the five scatter scenes at 51 bounces),
and to r1_trace_rays_host on the deep scene at other limits.  Then what the inputs must show for that to mean something (all four events,
every material, absorbed metal, paths to the depth limit), the flag, the fields' rules, zero stream states (in a child process with a
time limit) and the argument rules.  Every comparison is of bytes or bits, a NaN for a NaN; no case is left out anywhere."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import r1o
from rays1bench_amd import binding

import edge_scenes as es
import reference_cases as rc
from test_cast_host import cscene
from test_trace_rays_host import NONZERO, SAMPLE_FIXTURES, assert_records, ccam, fixture_rays, frame_samples

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
SCATTERED, SKY, ABSORBED, NONE = binding.SCATTER_SCATTERED, binding.SCATTER_SKY, binding.SCATTER_ABSORBED, binding.SCATTER_NONE
UNIT = binding.SCATTER_UNIT_DIRECTIONS
SCATTER_SCENES = ("glass", "metal0", "metal1", "mixed", "centre")
NAMES = ("r1_scatter_rays", "r1_scatter_rays_device", "r1_scatter_rays_host", "r1_camera_rays_device")


class Folded:
    """the fold of a ray set: records (RADIANCE_DTYPE) and, per level, (indices of the rays still alive, their step's Scatter)"""

    def __init__(self, records, levels):
        self.records, self.levels = records, levels


def fold(step, rays, seeds, bounces, unit_after_first=True):
    """The fold of include/rays1.h in NumPy float32: levels 0 .. bounces on the rays still alive, level 0 without the flag, the later ones
    with it on the previous level's rays_out / seeds_out; one ray counted per level whose event is not NONE; SKY ends a path with
    col = weight, then col = w_e * col over its SCATTERED weights from the last to the first; ABSORBED and SCATTERED at the last level
    end it black.  step(rays, seeds, flags) -> binding.Scatter."""
    n = len(rays)
    rec = np.zeros(n, binding.RADIANCE_DTYPE)
    col = np.zeros((n, 3), F)
    weights, levels = [], []
    alive = np.arange(n)
    cur_rays, cur_seeds = rays, seeds
    for level in range(bounces + 1):
        if alive.size == 0:
            break
        out = step(cur_rays, cur_seeds, UNIT if (level > 0 and unit_after_first) else 0)
        levels.append((alive, out))
        ev = out.records["event"]
        assert np.isin(ev, (SCATTERED, SKY, ABSORBED, NONE)).all()
        rec["rays"][alive] += (ev != NONE).astype(np.uint32)
        w = np.ones((n, 3), F)  # (the slots of other paths multiply nothing that is read)
        w[alive[ev == SCATTERED]] = out.records["weight"][ev == SCATTERED]
        sky = alive[ev == SKY]
        c = out.records["weight"][ev == SKY].astype(F)
        for e in range(level - 1, -1, -1):
            c = (weights[e][sky] * c).astype(F)
        col[sky] = c
        weights.append(w)
        go = ev == SCATTERED
        alive, cur_rays, cur_seeds = alive[go], np.ascontiguousarray(out.rays[go]), np.ascontiguousarray(out.seeds[go])
    rec["r"], rec["g"], rec["b"] = col[:, 0], col[:, 1], col[:, 2]
    return Folded(rec, levels)


def host_step(sa):
    cs = cscene(sa)
    return lambda rays, seeds, flags: binding.scatter_rays_host(cs, rays, seeds, flags)


def scatter_case(name):
    """(scene, rays, seeds, the reference fixture) of a scatter scene's small size: the 64 x 48 x 4 frame of tests/test_gpu_scatter.py"""
    case = rc.BY_ID[f"scatter-{name}"]
    sa = rc.scene_of(case, 0)
    x, y, s = frame_samples(rc.W, rc.H, case.spp)
    p = binding.make_params(rc.W, rc.H, case.spp, case.seed, max_bounces=case.bounces)
    rays, seeds = binding.camera_rays(es.ccamera(sa.camera_array), p, x, y, s)
    return case, sa, rays, seeds


@pytest.fixture(scope="module")
def scatter_folds():
    """name -> (case, scene, rays, seeds, Folded at 51 bounces), computed on first use and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            case, sa, rays, seeds = scatter_case(name)
            cache[name] = (case, sa, rays, seeds, fold(host_step(sa), rays, seeds, case.bounces))
        return cache[name]

    return get


# ---- 1: names and sizes --------------------------------------------------------------------------------------------------------------------


def test_names_sizes_and_constants_follow_the_header():
    hdr = open(os.path.join(binding.HERE, "..", "include", "rays1.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in bound and getattr(binding.lib(), name), name
    assert "#define R1_ABI_VERSION 4" in hdr
    assert binding.SCATTER_DTYPE.itemsize == 32
    assert [binding.SCATTER_DTYPE.fields[k][1] for k in ("weight", "event", "t", "index", "mat_type", "pad")] == [0, 12, 16, 20, 24, 28]
    for key, value in (("R1_SCATTER_SCATTERED", SCATTERED), ("R1_SCATTER_SKY", SKY), ("R1_SCATTER_ABSORBED", ABSORBED), ("R1_SCATTER_NONE", NONE),
                       ("R1_SCATTER_UNIT_DIRECTIONS", UNIT), ("R1_MAT_NONE", binding.MAT_NONE)):
        assert int(re.search(key + r" = (\d+)", hdr).group(1)) == value, key
    assert (SCATTERED, SKY, ABSORBED, NONE, UNIT) == (0, 1, 2, 3, 1)
    assert callable(binding.Renderer.scatter_rays) and callable(binding.Renderer.scatter_rays_device) and callable(binding.Renderer.camera_rays_device)
    s = binding.Scatter(1, 2, 3)
    assert (s.records, s.rays, s.seeds) == (1, 2, 3) == tuple(s)


# ---- 2: pinned to the reference ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene,file", SAMPLE_FIXTURES)
def test_fold_of_host_steps_equals_the_reference_on_every_sample(scene, file):
    sa, rays, seeds, g = fixture_rays(scene, file)
    got = fold(host_step(sa), rays, seeds, 50)
    assert_records(got.records, g["rgb"], g["rays"], file)
    assert len(got.levels) >= 8


@pytest.mark.parametrize("name", SCATTER_SCENES)
def test_fold_equals_the_references_records_on_the_scatter_scenes(scatter_folds, name):
    case, sa, rays, seeds, got = scatter_folds(name)
    assert case.bounces == 51
    g = rc.fixture(case)
    rc.assert_records(g, got.records.view(F).reshape(-1, 4), f"{name}: fold of r1_scatter_rays_host")
    assert int(got.records["rays"].astype(np.uint64).sum()) == int(g["rays"][0])


@pytest.mark.parametrize("bounces", (1, 2, 50, 51))
def test_fold_equals_the_host_trace_on_the_deep_scene(bounces):
    sa, _ = es.build("deep", "small")
    x, y, s = frame_samples(es.W, es.H, 2)
    rays, seeds = binding.camera_rays(es.ccamera(sa.camera_array), binding.make_params(es.W, es.H, 2, es.SEED["deep"]), x, y, s)
    want = binding.trace_rays_host(cscene(sa), rays, seeds, bounces)
    got = fold(host_step(sa), rays, seeds, bounces)
    assert got.records.tobytes() == want.tobytes()
    assert want["rays"].max() <= bounces + 1 and (want["rays"].max() == bounces + 1 if bounces < 50 else want["rays"].max() >= 31)


# ---- 3: the inputs mean something (asserted on the host form's output: the reference alone decides) -----------------------------------------


def test_inputs_show_every_event_material_and_the_depth_limit(scatter_folds):
    events, scattered_types = set(), set()
    deepest = 0
    for name in SCATTER_SCENES:
        case, sa, rays, seeds, got = scatter_folds(name)
        types = sa.arrays["mat_type"]
        for alive, out in got.levels:
            r = out.records
            events |= set(np.unique(r["event"]).tolist())
            scattered_types |= set(np.unique(r["mat_type"][r["event"] == SCATTERED]).tolist())
            hit = r["event"] != SKY
            assert (r["mat_type"][hit] == types[r["index"][hit]]).all() and (r["index"][~hit] == -1).all()
        deepest = max(deepest, len(got.levels))
        first = got.levels[0][1].records
        if name == "metal1":
            hits = first["event"] != SKY
            assert hits.sum() > 1000 and (first["event"][hits] == ABSORBED).mean() > 0.05  # fuzz 1 scatters below the surface
        if name == "glass":
            for alive, out in got.levels:
                r = out.records
                assert (r["weight"][r["event"] == SCATTERED].view(np.uint32) == F(1.0).view(np.uint32)).all()
                assert not (r["event"] == ABSORBED).any()
    assert events == {SCATTERED, SKY, ABSORBED}  # (NONE: the non-finite rays below)
    assert scattered_types == {binding.MAT_LAMBERTIAN, binding.MAT_METAL, binding.MAT_DIELECTRIC}
    assert deepest == 52  # level 51 was run: a path scattered 51 times


# ---- 4: the flag ---------------------------------------------------------------------------------------------------------------------------


def test_the_flag_matters_and_later_levels_are_the_host_traces(scatter_folds):
    case, sa, rays, seeds, got = scatter_folds("mixed")
    step = host_step(sa)
    # unit inputs produced by a step: every level's scattered rays
    unit_rays = np.concatenate([out.rays[out.records["event"] == SCATTERED] for _, out in got.levels])
    unit_seeds = np.concatenate([out.seeds[out.records["event"] == SCATTERED] for _, out in got.levels])
    assert len(unit_rays) > 10000
    on, off = step(unit_rays, unit_seeds, UNIT), step(unit_rays, unit_seeds, 0)
    both = (on.records["event"] != SKY) & (off.records["event"] != SKY)
    differ = (on.rays["d"].view(np.uint32) != off.rays["d"].view(np.uint32)).any(1) & both
    assert differ.any(), "normalising a scattered direction again never changed a bit: the flag is untested"
    # with the flag, level k + 1 is the host trace's: the fold cut at every small limit is the trace at that limit
    cs = cscene(sa)
    for b in (1, 2, 3, 4, 5, 6):
        assert fold(step, rays, seeds, b).records.tobytes() == binding.trace_rays_host(cs, rays, seeds, b).tobytes(), b
    # and without it the fold is another: the second normalisation shows in the records
    assert fold(step, rays, seeds, 6, unit_after_first=False).records.tobytes() != binding.trace_rays_host(cs, rays, seeds, 6).tobytes()


# ---- 5: field rules ------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def medium():
    """1024 samples of the medium fixture: scene, rays, seeds, and the host form's level 0"""
    sa, rays, seeds, g = fixture_rays(*SAMPLE_FIXTURES[1])
    rays, seeds = rays[:1024].copy(), seeds[:1024].copy()
    return sa, rays, seeds, binding.scatter_rays_host(cscene(sa), rays, seeds, 0)


def none_records(n):
    want = np.zeros(n, binding.SCATTER_DTYPE)
    want["event"], want["t"], want["index"], want["mat_type"] = NONE, FLT_MAX, -1, binding.MAT_NONE
    return want


def test_rays_that_take_no_step(medium):
    sa, rays, seeds, level0 = medium
    base = rays.view(F).reshape(-1, 8)[:64].copy()
    cases = []
    for col in (0, 1, 2):
        for v in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[:, col] = v
            cases.append((r, (0, UNIT)))
    for v in (0.0, 1e-30):  # (normalised: 1 / 0.  With the flag such a direction is used as it is: the caller's promise was broken)
        r = base.copy()
        r[:, 4:7] = v
        cases.append((r, (0,)))
    for v in (np.nan, np.inf):
        r = base.copy()
        r[:, 5] = v
        cases.append((r, (0, UNIT)))
    sd = seeds[:64].copy()
    sd["lane1"][::2] = 0  # (the guarded input comes back)
    guarded = sd.copy()
    guarded["lane1"][::2] = NONZERO
    for r, flag_set in cases:
        for flags in flag_set:
            out = binding.scatter_rays_host(cscene(sa), r, sd, flags)
            assert out.records.tobytes() == none_records(64).tobytes(), (r[0], flags)
            assert not out.rays.view(np.uint8).any() and out.seeds.tobytes() == guarded.tobytes(), (r[0], flags)
    # among valid rays
    mixed = base.copy()
    mixed[::3, 4:7] = 0.0
    out = binding.scatter_rays_host(cscene(sa), mixed, seeds[:64], 0)
    keep = np.ones(64, bool)
    keep[::3] = False
    assert (out.records["event"][~keep] == NONE).all()
    for got, want in zip(out, level0):
        assert got[keep].tobytes() == want[:64][keep].tobytes()


def test_sky_and_hit_fields_and_ignored_inputs(medium):
    sa, rays, seeds, level0 = medium
    rec, nr, ns = level0
    sky, hit = rec["event"] == SKY, rec["event"] != SKY
    assert sky.sum() > 50 and hit.sum() > 50 and not (rec["event"] == NONE).any()
    # SKY: zero rays_out, the input states, the sky's colour of the normalised direction
    assert not nr[sky].view(np.uint8).any() and ns[sky].tobytes() == seeds[sky].tobytes()
    assert (rec["t"][sky] == FLT_MAX).all() and (rec["index"][sky] == -1).all() and (rec["mat_type"][sky] == binding.MAT_NONE).all()
    d = rays["d"][sky]
    dot = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])).astype(F) + (d[:, 2] * d[:, 2]).astype(F)
    dy = (d[:, 1] * (F(1) / np.sqrt(dot).astype(F)).astype(F)).astype(F)
    t = (F(0.5) * (dy + F(1))).astype(F)
    omt = (F(1) - t).astype(F)
    want = np.stack([omt + (t * F(0.5)).astype(F), omt + (t * F(0.7)).astype(F), omt + t], 1).astype(F)
    assert rec["weight"][sky].tobytes() == want.tobytes()
    # hits: t, index and the hit point are the ray query's; the scattered ray starts there with t_max FLT_MAX, pad 0 and a unit direction
    cast = binding.cast_rays_host(cscene(sa), rays)
    assert rec["t"].tobytes() == cast["t"].tobytes() and rec["index"].tobytes() == cast["index"].tobytes()
    assert np.ascontiguousarray(nr["o"][hit]).tobytes() == np.ascontiguousarray(cast["p"][hit]).tobytes()
    assert (nr["t_max"][hit] == FLT_MAX).all() and not nr["pad"].any() and not rec["pad"].any()
    assert np.abs(np.linalg.norm(nr["d"][hit].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (rec["mat_type"][hit] == sa.arrays["mat_type"][rec["index"][hit]]).all()
    albedo = np.stack([sa.arrays[k][rec["index"][hit]] for k in ("albedo_r", "albedo_g", "albedo_b")], 1)
    glass = (rec["mat_type"][hit] == binding.MAT_DIELECTRIC)[:, None]
    lit = (rec["event"][hit] == SCATTERED)[:, None]
    assert rec["weight"][hit].tobytes() == np.where(lit, np.where(glass, F(1), albedo), F(0)).astype(F).tobytes()
    assert (ns[hit].view(np.uint32).reshape(-1, 4) != seeds[hit].view(np.uint32).reshape(-1, 4)).any(1).all()  # (every material draws)
    # t_max and pad of the input are ignored; a direction scaled by a power of two is the same ray
    r = rays.copy()
    r["t_max"] = np.resize(np.array([0.0, -1.0, 0.5, np.nan, np.inf, 1e-3], F), len(r))
    r["pad"] = 0xDEADBEEF
    r["d"] *= F(4.0)
    for got, want in zip(binding.scatter_rays_host(cscene(sa), r, seeds, 0), level0):
        assert got.tobytes() == want.tobytes()
    # the plain input forms, the thread split and the order of the rays change nothing
    again = binding.scatter_rays_host(cscene(sa), rays.view(F).reshape(-1, 8)[:300], seeds.view(np.uint32).reshape(-1, 4)[:300], 0)
    perm = np.random.default_rng(5).permutation(len(rays))
    shuffled = binding.scatter_rays_host(cscene(sa), rays[perm], seeds[perm], 0)
    for got, sh, want in zip(again, shuffled, level0):
        assert got.tobytes() == want[:300].tobytes() and sh.tobytes() == want[perm].tobytes()


def test_index_is_a_scene_index_with_placeholders_in_front_of_every_sphere(medium):
    sa, rays, seeds, level0 = medium
    n = len(sa.arrays["inv_radius"])
    arrays = {}
    for k, v in sa.arrays.items():
        w = np.repeat(v, 2)
        if k == "inv_radius":
            w[0::2] = 0
        if k == "mat_type":
            w[0::2] = 255
        arrays[k] = w
    spaced = r1o.SceneArrays(arrays, sa.camera_array)
    out = binding.scatter_rays_host(cscene(spaced), rays, seeds, 0)
    hit = level0.records["event"] != SKY
    assert hit.any() and (out.records["index"][hit] == 2 * level0.records["index"][hit] + 1).all() and (out.records["index"][~hit] == -1).all()
    want = level0.records.copy()
    want["index"] = out.records["index"]
    assert out.records.tobytes() == want.tobytes() and out.rays.tobytes() == level0.rays.tobytes() and out.seeds.tobytes() == level0.seeds.tobytes()
    assert len(arrays["inv_radius"]) == 2 * n


def test_null_seeds_are_the_seeding_contract_of_seed_0(medium):
    sa, rays, _, _ = medium
    cs = cscene(sa)
    # what r1_trace_rays_host makes of NULL seeds is pinned in tests/test_trace_rays_host.py: a step with NULL seeds is that trace's level
    assert fold(lambda r, s, f: binding.scatter_rays_host(cs, r, s, f), rays, None, 50).records.tobytes() == binding.trace_rays_host(cs, rays, None, 50).tobytes()


# ---- 6: zero stream states -----------------------------------------------------------------------------------------------------------------

ZERO_STATES = """
import sys
import numpy as np
sys.path[:0] = {path!r}
from rays1bench_amd import binding
from test_cast_host import cscene
from test_trace_rays_host import NONZERO, SAMPLE_FIXTURES, fixture_rays
sa, rays, seeds, g = fixture_rays(*SAMPLE_FIXTURES[1])
rays, seeds = rays[:1024].copy(), seeds[:1024].copy()
cs = cscene(sa)
for k in ("scalar", "lane0", "lane1", "lane2"):
    zero, const = seeds.copy(), seeds.copy()
    zero[k], const[k] = 0, NONZERO
    for a, b in zip(binding.scatter_rays_host(cs, rays, zero, 0), binding.scatter_rays_host(cs, rays, const, 0)):
        assert a.tobytes() == b.tobytes(), k
zero, const = np.zeros(len(rays), binding.SEED_DTYPE), np.full((len(rays), 4), NONZERO, np.uint32)
got, want = binding.scatter_rays_host(cs, rays, zero, 0), binding.scatter_rays_host(cs, rays, const, 0)
for a, b in zip(got, want):
    assert a.tobytes() == b.tobytes()
sky = got.records["event"] == binding.SCATTER_SKY
assert sky.any() and (~sky).any()
assert (got.seeds[sky].view(np.uint32) == NONZERO).all()           # nothing drawn: the guarded input
assert (got.seeds[~sky].view(np.uint32).reshape(-1, 4) != NONZERO).any(1).all()  # drawn from the replaced states
print("zero states replaced")
"""


def test_a_zero_stream_state_is_replaced_and_the_call_returns():
    """in a child process with a time limit: a zero state that reached random_in_unit_sphere would never come back"""
    here = os.path.dirname(os.path.abspath(__file__))
    path = [here, os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")]
    done = subprocess.run([sys.executable, "-c", ZERO_STATES.format(path=path)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "zero states replaced" in done.stdout, done.stderr[-2000:]


# ---- 7: argument errors --------------------------------------------------------------------------------------------------------------------


def test_argument_errors_in_the_documented_order_and_n_zero(medium):
    sa, rays, seeds, level0 = medium
    L, E = binding.lib(), binding.R1_EINVAL
    cs = cscene(sa)
    rec, nr, ns = np.zeros(4, binding.SCATTER_DTYPE), np.zeros(4, binding.RAY_DTYPE), np.zeros(4, binding.SEED_DTYPE)
    ptrs = (nr.ctypes.data, ns.ctypes.data, rec.ctypes.data)
    assert L.r1_scatter_rays_host(C.byref(cs), 0, None, None, 0, None, None, None) == binding.R1_OK
    assert len(binding.scatter_rays_host(cs, rays[:0], seeds[:0]).records) == 0
    # flags first, then the scene, then n == 0, then the pointers
    assert L.r1_scatter_rays_host(None, 2, None, None, 0, None, None, None) == E and b"flags" in L.r1_last_error()
    assert L.r1_scatter_rays_host(C.byref(cs), -1, rays.ctypes.data, seeds.ctypes.data, 4, *ptrs) == E and b"flags" in L.r1_last_error()
    assert L.r1_scatter_rays_host(None, 0, None, None, 0, None, None, None) == E and b"scene" in L.r1_last_error()
    assert L.r1_scatter_rays_host(C.byref(cs), 0, None, seeds.ctypes.data, 4, *ptrs) == E
    for k in range(3):
        p = list(ptrs)
        p[k] = None
        assert L.r1_scatter_rays_host(C.byref(cs), 0, rays.ctypes.data, seeds.ctypes.data, 4, *p) == E and b"null" in L.r1_last_error()
    assert not rec.view(np.uint8).any() and not nr.view(np.uint8).any() and not ns.view(np.uint8).any()
    # the device entry points: a NULL context is refused before anything is touched (no device needed)
    assert L.r1_scatter_rays(None, 0, 0, rays.ctypes.data, seeds.ctypes.data, 4, *ptrs) == E and b"ctx" in L.r1_last_error()
    assert L.r1_scatter_rays_device(None, 0, 0, C.c_void_p(256), None, 4, C.c_void_p(512), C.c_void_p(1024), C.c_void_p(2048), None) == E
    assert b"ctx" in L.r1_last_error()
    p = binding.make_params(8, 8, 1, 1)
    assert L.r1_camera_rays_device(None, None, C.byref(p), 0, 4, C.c_void_p(256), C.c_void_p(512), None) == E and b"ctx" in L.r1_last_error()
    with pytest.raises(binding.R1Error):
        binding.scatter_rays_host(cs, rays, seeds[:5])
    with pytest.raises(binding.R1Error):
        binding.scatter_rays_host(cs, np.zeros((4, 7), F))
    # in place on the host: rays_out may be rays, seeds_out may be seeds
    r, s, o = rays.copy(), seeds.copy(), np.zeros(len(rays), binding.SCATTER_DTYPE)
    assert L.r1_scatter_rays_host(C.byref(cs), 0, r.ctypes.data, s.ctypes.data, len(r), r.ctypes.data, s.ctypes.data, o.ctypes.data) == binding.R1_OK
    assert o.tobytes() == level0.records.tobytes() and r.tobytes() == level0.rays.tobytes() and s.tobytes() == level0.seeds.tobytes()
    for n in (1, 63, 255, 256, 257, 1000):
        for got, want in zip(binding.scatter_rays_host(cs, rays[:n], seeds[:n]), level0):
            assert got.tobytes() == want[:n].tobytes(), n


# ---- 8: the stand-alone program ------------------------------------------------------------------------------------------------------------


def test_stand_alone_program(tmp_path):
    """tools/check_scatter_rays_host.cpp built with the host sources it drives (no sanitizer here: DESIGN.md §4.34 has that run)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "check_scatter_rays_host")
    src = [os.path.join(root, "tools", "check_scatter_rays_host.cpp")] + [os.path.join(root, "rays1bench_amd", "csrc", f) for f in
                                                                          ("r1_queries_host.cpp", "r1_host.cpp", "r1_bvh.cpp")]
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    assert os.path.isdir(inc), "the HIP headers are needed to compile the library's host sources"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + inc] + src + ["-pthread", "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    for says in ("fold at  1 bounces", "fold at 51 bounces", "in place and NULL seeds", "32 rays without a step among 64", "refusals: six"):
        assert says in done.stdout, done.stdout
