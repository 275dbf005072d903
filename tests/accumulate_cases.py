"""What tests/test_accumulate_host.py, tests/test_gpu_accumulate.py and tools/accumulate_prototype.py share (accumulated frames,
include/rays1.h): the contract restated in numpy float32 from the header's text — whole-frame array operations, nothing of
the C —, seeded synthetic frame pairs asserted to hold every class of input the contract names, the camera pairs, the rendered pairs, and
the host form's results, computed once per case and left unchanged.  Nothing here has a tolerance."""
import ctypes as C
import functools

import numpy as np

import rays1bench_amd as r1
from rays1bench_amd import binding

import denoise_cases as dc
import feature_cases as fc
import linear_cases as lc

F = np.float32
U32 = np.uint32
WRAP = 0xFFFFFFF0
# the defaults DESIGN.md §4.41 chose on the medium scene
OPT = dict(max_samples=32, depth_tolerance=0.05, normal_min_cos=0.9)
# option sets: the defaults, then both ends of every range
OPTION_SETS = {"defaults": {}, "max_samples 1": dict(max_samples=1), "max_samples below n": dict(max_samples=2),
               "low ends": dict(max_samples=1, depth_tolerance=1e-30, normal_min_cos=-1.0),
               "high ends": dict(max_samples=0xFFFFFFFF, depth_tolerance=1e30, normal_min_cos=1.0),
               "cos -1": dict(normal_min_cos=-1.0, depth_tolerance=0.5), "cos 1": dict(normal_min_cos=1.0, depth_tolerance=0.5)}
SYNTHETIC = {"1x1": (1, 1), "5x3": (5, 3), "37x21": (37, 21), "70x40": (70, 40)}
DEVICE_ONLY = {"65x33": (65, 33), "257x17": (257, 17), "150x141": (150, 141)}
PAIRS = ("identical", "left", "right", "down", "up", "zoom", "turned")  # (i), (ii) x 4, (iii), (v); (iv) is "identical": the camera is axis-aligned
ROTATED_PAIR, ROTATED_AT = "general", "37x21"  # reproject_truth_cases' two cameras, neither axis-aligned: run at that one size
RENDERED = {"medium": (33, 17, 3), "large": (64, 48, 4)}
SPP, SPP_PREV = 4, 3  # of the synthetic pairs: dc.synthetic's hits are 1 .. 4


def opt(**kw):
    d = dict(OPT)
    d.update(kw)
    return binding.make_accumulate_opt(**d)


def cam_fields(cam):
    """a CCamera's vectors as float32 arrays"""
    return {k: np.array(list(getattr(cam, k)), F) for k in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w")}


def make_camera(origin, u, v, w, half_w, half_h):
    """a pinhole CCamera at `origin` with the orthonormal basis (u, v, w), the screen one unit in front (along -w), in float32"""
    o, u, v, w = (np.asarray(a, F) for a in (origin, u, v, w))
    cam = binding.CCamera()
    ll = ((o - F(half_w) * u) - F(half_h) * v) - w
    for k, val in (("origin", o), ("lower_left", ll), ("horizontal", F(2) * F(half_w) * u), ("vertical", F(2) * F(half_h) * v), ("u", u), ("v", v), ("w", w)):
        setattr(cam, k, (C.c_float * 3)(*[float(x) for x in val.astype(F)]))
    cam.lens_radius = 0.0
    return cam


def camera_pair(pair, w, h):
    """(current, previous) of a synthetic frame: the current camera sits at the origin and looks along -z, axis-aligned — but for
    ROTATED_PAIR, where both cameras are turned about all three axes"""
    if pair == ROTATED_PAIR:
        import reproject_truth_cases as rt  # (it imports this module)
        return rt.cameras("general", w, h)
    hw, hh = 1.0, float(F(h) / F(w))
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    cur = make_camera((0, 0, 0), X, Y, Z, hw, hh)
    step = 6.0 * 2.5 * 2.0 / max(w, 4)  # a surface 2.5 away moves 6 pixels on the previous screen
    if pair == "identical":
        prev = make_camera((0, 0, 0), X, Y, Z, hw, hh)
    elif pair in ("left", "right"):
        prev = make_camera((step if pair == "left" else -step, 0, 0), X, Y, Z, hw, hh)
    elif pair in ("down", "up"):
        prev = make_camera((0, step if pair == "down" else -step, 0), X, Y, Z, hw, hh)
    elif pair == "zoom":  # the previous screen is smaller by 1 + 1 / (w - 1): column 0 lands at px = -1/2, column w - 1 at w - 1/2
        k = 1.0 / (1.0 + 1.0 / max(w - 1, 1))
        prev = make_camera((0, 0, 0), X, Y, Z, hw * k, hh * k)
    else:
        assert pair == "turned"  # by 180 degrees about y
        prev = make_camera((0, 0, 0), (-1, 0, 0), Y, (0, 0, -1), hw, hh)
    return cur, prev


def view_of(cur, prev, spp, spp_prev):
    return binding.make_accumulate_view(cur, prev, spp, spp_prev)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def unit(n):
    """the filters' prepare rule: nh = l > 0 ? n / l : 0"""
    l = np.sqrt(dot(n, n))
    return np.where((l > 0)[..., None], n / np.where(l > 0, l, F(1))[..., None], F(0)).astype(F)


def numpy_accumulate(L, V, f, A_prev, f_prev, M_prev, view, o, want_stats=False):
    """The contract in numpy float32: (A_out (h, w, 3), M_out MOMENT_DTYPE (h, w)).  One rounded operation per element and line, in the order of
    the header's text; a skipped tap leaves the sums untouched.  want_stats: also what the tests assert about the cases themselves."""
    L = np.asarray(L, F)
    h, w = L.shape[:2]
    cam, prev = cam_fields(view.camera), cam_fields(view.camera_prev)
    with np.errstate(all="ignore"):
        dl = prev["lower_left"] - prev["origin"]
        pu, pv, pw = dot(dl, prev["u"]), dot(dl, prev["v"]), dot(dl, prev["w"])
        hu, vv = dot(prev["horizontal"], prev["u"]), dot(prev["vertical"], prev["v"])
        inv_w, inv_h = F(1) / F(w), F(1) / F(h)
        wf, hf = F(w), F(h)
        n = V["samples"].astype(U32)
        hits = f["hits"].astype(U32)
        surface = (hits != 0) & (n != 0)
        s = ((np.arange(w).astype(F) + F(0.5)) * inv_w)[None, :, None]
        t = ((np.arange(h).astype(F) + F(0.5)) * inv_h)[:, None, None]
        d = ((cam["lower_left"] + cam["horizontal"] * s) + cam["vertical"] * t) - cam["origin"]
        dh = d / np.sqrt(dot(d, d))[..., None]
        m = (f["depth"] / hits.astype(F)) * F(view.spp)
        P = cam["origin"] + dh * m[..., None]
        q = (P - prev["origin"]).astype(F)
        a, b, c = dot(q, prev["u"]), dot(q, prev["v"]), dot(q, prev["w"])
        front = c * pw > 0
        k = pw / c
        sx, sy = (a * k - pu) / hu, (b * k - pv) / vv
        px, py = sx * wf - F(0.5), sy * hf - F(0.5)
        exists = surface & front & (px > -1) & (px < wf) & (py > -1) & (py < hf)
        flx, fly = np.floor(px), np.floor(py)
        x0, y0 = np.where(exists, flx, 0).astype(np.int64), np.where(exists, fly, 0).astype(np.int64)
        fx, fy = (px - flx).astype(F), (py - fly).astype(F)
        e = np.sqrt(dot(q, q))
        nh = unit(f["normal"].astype(F))
        B, Cs, U = np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
        N = np.full((h, w), 0xFFFFFFFF, np.uint64)
        tol, min_cos = F(o.depth_tolerance), F(o.normal_min_cos)
        taken_any = np.zeros((h, w), int)
        skipped = {"off the image": 0, "weight": 0, "hits": 0, "samples": 0, "depth": 0, "normal": 0}
        for j in (0, 1):
            for i in (0, 1):
                tx, ty = x0 + i, y0 + j
                on = exists & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                cx, cy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)  # (where `on` is false the gathered records are not used)
                fq, mq, aq = f_prev[cy, cx], M_prev[cy, cx], np.asarray(A_prev, F)[cy, cx]
                bw = ((fx if i else F(1) - fx) * (fy if j else F(1) - fy)).astype(F)
                m_q = (fq["depth"] / fq["hits"].astype(F)) * F(view.spp_prev)
                df = e - m_q
                df = np.where(df < 0, -df, df)
                mx = np.where(e < m_q, m_q, e)
                tests = (("off the image", on), ("weight", bw > 0), ("hits", fq["hits"] != 0), ("samples", mq["samples"] != 0), ("depth", df <= tol * mx),
                         ("normal", ~(dot(nh, unit(fq["normal"].astype(F))) < min_cos)))
                take = exists.copy()
                for name, passed in tests:
                    skipped[name] += int((take & ~passed).sum())
                    take &= passed
                taken_any += take
                B = np.where(take, B + bw, B)
                Cs = np.where(take[..., None], Cs + bw[..., None] * aq, Cs)
                U = np.where(take[..., None], U + bw[..., None] * mq["var"], U)
                N = np.where(take & (mq["samples"] < N), mq["samples"].astype(np.uint64), N)
        blend = exists & (B > 0)
        Bs = np.where(blend, B, F(1))[..., None]
        hist, vh = Cs / Bs, U / Bs
        N_new = np.maximum(n.astype(np.uint64), np.minimum(N + n.astype(np.uint64), np.uint64(o.max_samples)))
        alpha = np.where(n.astype(np.uint64) >= N_new, F(1), n.astype(F) / N_new.astype(U32).astype(F)).astype(F)[..., None]
        A_new = hist + (L - hist) * alpha
        var_new = ((F(1) - alpha) * (F(1) - alpha)) * vh + (alpha * alpha) * V["var"]
    A_out = L.copy()
    M_out = np.array(V)
    A_out.view(U32)[blend] = np.ascontiguousarray(A_new.astype(F)).view(U32)[blend]
    M_out["var"].view(U32)[blend] = np.ascontiguousarray(var_new.astype(F)).view(U32)[blend]
    M_out["samples"][blend] = N_new[blend].astype(U32)
    if not want_stats:
        return A_out, M_out
    ex = exists
    stats = {"mask": blend, "history": int(ex.sum()), "surface without history": int((surface & ~ex).sum()), "blended": int(blend.sum()),
             "px in (-1, 0)": int((ex & (px < 0)).sum()), "px in (w - 1, w)": int((ex & (px > wf - F(1))).sum()), "fx exactly 0": int((ex & (fx == 0)).sum()),
             "behind the previous camera": int((surface & ~front).sum()), "taps taken": int(taken_any.sum()), "skipped": skipped,
             "off by edge": {"left": int((surface & front & ~(px > -1)).sum()), "right": int((surface & front & ~(px < wf)).sum()),
                             "down": int((surface & front & ~(py > -1)).sum()), "up": int((surface & front & ~(py < hf)).sum())}}
    return A_out, M_out, stats


@functools.lru_cache(maxsize=None)
def synthetic(w, h, seed=5150):
    """(L, V, f, A_prev, f_prev, M_prev) of a seeded w x h pair of frames: dc.synthetic's frame as the current one, a history that agrees with it
    in most places, and — where the size allows — every block classes() counts.  Read-only."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    L, f0 = dc.synthetic(w, h)
    f = f0.copy()
    hits = f["hits"]
    surf = hits > 0
    # a scene the cameras can share: most pixels 2.5 away, as dc.synthetic has them; the x 1000 outliers stay
    f_prev = f.copy()
    move = rng.random((h, w)) < 0.15
    f_prev["depth"][move] *= rng.uniform(1.2, 3.0, (h, w)).astype(F)[move]          # history of another surface
    turn = rng.random((h, w)) < 0.10
    f_prev["normal"][turn] = -f_prev["normal"][turn]                                  # ... or of its other side
    f_prev["hits"] = np.where(surf, rng.integers(1, SPP_PREV + 1, (h, w)), 0).astype(U32)
    f_prev["depth"] = np.where(surf, f_prev["depth"] / np.maximum(hits, 1).astype(F) * f_prev["hits"].astype(F) * F(SPP / SPP_PREV), F(0)).astype(F)
    V = np.zeros((h, w), binding.MOMENT_DTYPE)
    V["var"] = (rng.uniform(0.0, 0.05, (h, w, 3)) ** 2).astype(F)
    V["samples"] = SPP
    M_prev = np.zeros((h, w), binding.MOMENT_DTYPE)
    M_prev["var"] = (rng.uniform(0.0, 0.03, (h, w, 3)) ** 2).astype(F)
    M_prev["samples"] = rng.integers(1, 40, (h, w)).astype(U32)
    A_prev = (np.asarray(L) * rng.uniform(0.8, 1.25, (h, w, 3)).astype(F)).astype(F)
    if w >= 12 and h >= 8:
        d = f["depth"]
        d[8, 2], d[8, 3], d[8, 4], d[8, 5] = np.nan, np.inf, 1e30, 0.0               # on hit pixels (row 8 has hits)
        f["hits"][8, 2:6] = np.maximum(f["hits"][8, 2:6], 1)
        f_prev["hits"][10:13, 12:16] = 0                                             # a history without a hit
        M_prev["samples"][14:16, 3:9] = 0                                            # ... and one of no length
        M_prev["samples"][4:7, w - 9:w - 4] = WRAP                                    # N + n would wrap in 32 bits
        M_prev["samples"][rng.random((h, w)) < 0.03] = WRAP
        V["samples"][h - 2, 4:8] = 0                                                 # n == 0
        f_prev["depth"][2, 12:15] = [np.nan, np.inf, -1.0]
        A_prev[17 % h, 5:8] = [1e38, 1e-41, 0.0]                                      # (finite: a NaN the blend MAKES has no agreed bits)
    else:
        M_prev["samples"][0, 0] = WRAP
    for a in (V, f, A_prev, f_prev, M_prev):
        a.setflags(write=False)
    return L, V, f, A_prev, f_prev, M_prev


def classes(V, f, f_prev, M_prev):
    """How many pixels of a synthetic pair fall into each block the issue lists"""
    hit = f["hits"] > 0
    d = f["depth"]
    n = f["normal"]
    zero_normal = (dot(n, n) == 0)
    return {"depth NaN on hit pixels": int((hit & np.isnan(d)).sum()), "depth +inf on hit pixels": int((hit & np.isposinf(d)).sum()),
            "depth 1e30 on hit pixels": int((hit & (d == F(1e30))).sum()), "depth 0 on hit pixels": int((hit & (d == 0)).sum()),
            "hits 0 in the current frame": int((~hit).sum()), "hits 0 in the previous frame": int((f_prev["hits"] == 0).sum()),
            "M_prev.samples 0": int((M_prev["samples"] == 0).sum()), "M_prev.samples 0xFFFFFFF0": int((M_prev["samples"] == WRAP).sum()),
            "cancelled normals on hit pixels": int((hit & zero_normal).sum()), "n 0": int((V["samples"] == 0).sum())}


def synthetic_inputs(name, pair):
    """(six frames, view) of a synthetic case under a camera pair"""
    w, h = {**SYNTHETIC, **DEVICE_ONLY}[name]
    cur, prev = camera_pair(pair, w, h)
    return synthetic(w, h), view_of(cur, prev, SPP, SPP_PREV)


# ---- rendered pairs ------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def render(scene_name, w, h, spp, seed, cam_key=None):
    """(L, V, f) of r1_render_moments_host / r1_render_features_host through camera `cam_key` = (n, k): orbit_cameras(scene, n)[k]; None: the
    scene's own.  Read-only."""
    sc = lc.SCENES[scene_name](w, h)
    cam = sc.camera.contents if cam_key is None else binding.orbit_cameras(sc, cam_key[0])[cam_key[1]]
    p = r1.make_params(w, h, spp, seed)
    L, V, _ = binding.render_moments_host(sc.spheres.contents, cam, p)
    f = binding.render_features_host(sc.spheres.contents, cam, p)
    for a in (L, V, f):
        a.setflags(write=False)
    return L, V, f


def camera_of(scene_name, w, h, cam_key=None):
    sc = lc.SCENES[scene_name](w, h)
    cam = binding.CCamera()
    C.memmove(C.byref(cam), C.byref(sc.camera.contents if cam_key is None else binding.orbit_cameras(sc, cam_key[0])[cam_key[1]]), C.sizeof(cam))
    return cam


def rendered_inputs(name, how):
    """(six frames, view) of a rendered pair: how = "seeds" (the same camera, seeds 4242 and 4243) or "orbit" (orbit_cameras(scene, 64)[0] then
    [1]); the history is the previous render itself (A_prev = its L, M_prev = its V)"""
    w, h, spp = RENDERED[name]
    keys = (None, None) if how == "seeds" else ((64, 0), (64, 1))
    Lp, Vp, fp = render(name, w, h, spp, fc.SEED, keys[0])
    L, V, f = render(name, w, h, spp, fc.SEED + 1, keys[1])
    return (L, V, f, Lp, fp, Vp), view_of(camera_of(name, w, h, keys[1]), camera_of(name, w, h, keys[0]), spp, spp)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same(got, want):
    """(A, M) pairs equal byte for byte"""
    return got[0].shape == want[0].shape and bits(got[0]).tobytes() == bits(want[0]).tobytes() and bits(got[1]).tobytes() == bits(want[1]).tobytes()


@functools.lru_cache(maxsize=None)
def host_result(kind, name, pair, options="defaults"):
    """r1_accumulate_host of a case: kind "synthetic" (pair: a camera pair) or "rendered" (pair: "seeds" or "orbit").  Read-only."""
    frames, view = synthetic_inputs(name, pair) if kind == "synthetic" else rendered_inputs(name, pair)
    A, M = binding.accumulate_host(*frames, view, opt(**OPTION_SETS[options]))
    A.setflags(write=False), M.setflags(write=False)
    return A, M
