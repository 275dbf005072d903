"""What tests/test_accumulate_host.py and tests/test_gpu_accumulate.py share to hold accumulated frames (include/rays1.h)
against the geometry they claim to compute: an analytic plane seen through two cameras that are not axis-aligned, the feature frames of both
and the reprojected screen position of every pixel in numpy float64, from the cameras' fields alone — nothing of the C sources, nothing of
the plan's pu / pv / pw.  The history image is the ramp A_prev[y, x] = (x, y, 1): where all four taps are taken the bilinear history is
(px, py, 1), so the call's own output says where it looked, and a floorf that lands on the other side of an integer changes nothing."""
import functools

import numpy as np

from rays1bench_amd import binding

import accumulate_cases as ac

D = np.float64
F = np.float32
SIZES = {"33x17": (33, 17), "70x40": (70, 40), "257x17": (257, 17), "150x141": (150, 141)}
PREVIOUS = ("general", "identical", "dolly", "lens", "half the hits")  # "lens": the contract ignores it; "half the hits": f.hits = 2 of spp = 4
CASES = [(size, prev) for size in SIZES for prev in PREVIOUS]
SPP, SPP_PREV = 4, 3  # different, so that the two cannot be swapped
HISTORY = 1 << 24     # M_prev.samples: N_new = 2^24 + 1, (float)N_new = 2^24, alpha = 2^-24 exactly
ALPHA = 2.0 ** -24
OPT = dict(max_samples=0xFFFFFFFF, depth_tolerance=0.05, normal_min_cos=0.9)
P0 = np.array([0.0, 0.0, -2.5], D)
NORMAL = np.array([0.2, 0.3, 1.0], D) / np.sqrt(0.2 * 0.2 + 0.3 * 0.3 + 1.0)
MIN_COMPARED = 0.60   # of a frame's pixels; the least is "dolly" at 257x17 with 61.5 %
# |A_out.xy - truth.xy| <= TOLERANCE_ULPS * 2^-24 * max(w, h) pixels.  A screen position up to max(w, h) carries 2^-24 * max(w, h) / 2 of
# rounding a step, and the chain from the pixel centre to px has some twenty steps.  Measured with ac.numpy_accumulate, the fp32
# restatement (not the code under test), the maxima over a case's compared pixels, in units of 2^-24 * max(w, h):
#              general  identical  dolly     ("lens" and "half the hits" measure what "general" does, to the digit: the lens is ignored and
#   33x17       3.81     2.82      2.71       depth / hits * spp is exact for hits 2 of spp 4)
#   70x40       5.79     4.51      4.19
#   257x17      4.18     4.91      5.15
#   150x141     6.53     5.93      5.29
# 6.53 units are 5.8e-5 px at 150x141; 5.15 are 7.9e-5 px at width 257.  32 leaves five times the worst; every mistake of the geometry (a
# half-pixel offset, t from the other edge, pu for pv, spp for spp_prev) is half a pixel or more, thousands of units.
TOLERANCE_ULPS = 32.0


def tolerance(w, h):
    return TOLERANCE_ULPS * ALPHA * max(w, h)


def rotated_basis(yaw, pitch, roll):
    """(u, v, w) of the axis-aligned basis turned by roll about z, then pitch about x, then yaw about y"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], D)
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], D)
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]], D)
    R = Ry @ Rx @ Rz
    return R[:, 0], R[:, 1], R[:, 2]


def cameras(prev, w, h):
    """(current, previous) CCamera of a case"""
    hw, hh = 0.8, 0.8 * h / w
    cur_basis = rotated_basis(0.3, -0.2, 0.1)
    cur = ac.make_camera((0.3, 0.7, 1.1), *cur_basis, hw, hh)
    if prev in ("general", "lens", "half the hits"):
        was = ac.make_camera((0.45, 0.62, 1.0), *rotated_basis(0.34, -0.17, 0.13), hw, hh)
    elif prev == "identical":
        was = ac.make_camera((0.3, 0.7, 1.1), *cur_basis, hw, hh)
    else:
        assert prev == "dolly"
        was = ac.make_camera((0.3, 0.7, 0.6), *cur_basis, hw, hh)
    if prev == "lens":
        cur.lens_radius = was.lens_radius = 0.05
    return cur, was


def fields(cam):
    """a camera's vectors as stored, widened to float64"""
    return {k: v.astype(D) for k, v in ac.cam_fields(cam).items()}


def plane_distance(cam, w, h):
    """(o, dh (h, w, 3), t (h, w)): the unit pixel-centre rays of `cam` and their distance to the plane, float64"""
    c = fields(cam)
    s = ((np.arange(w, dtype=D) + 0.5) / w)[None, :, None]
    t = ((np.arange(h, dtype=D) + 0.5) / h)[:, None, None]
    d = c["lower_left"] + c["horizontal"] * s + c["vertical"] * t - c["origin"]
    dh = d / np.sqrt((d * d).sum(-1))[..., None]
    dist = ((P0 - c["origin"]) @ NORMAL) / (dh @ NORMAL)
    assert (dist > 0).all()  # every ray meets the plane in front of the camera
    return c["origin"], dh, dist


def feature_frame(dist, spp, hits):
    """the feature frame of a plane pixel: `hits` of `spp` samples hit, each at `dist`: depth is their sum over spp, normal their sum"""
    h, w = dist.shape
    f = np.zeros((h, w), binding.FEATURE_DTYPE)
    f["albedo"] = F(0.5)
    f["depth"] = (dist * (hits / spp)).astype(F)
    f["normal"] = (NORMAL * hits).astype(F)
    f["hits"] = hits
    return f


def screen_position(P, cam, w, h):
    """(px, py, in front) of the points P on `cam`'s screen in float64: the (sx, sy, k) with lower_left + sx horizontal + sy vertical -
    origin = k (P - origin), solved by Cramer's rule — the camera's basis vectors u, v, w are not used"""
    c = fields(cam)
    q = P - c["origin"]
    a, b, r = c["horizontal"], c["vertical"], c["origin"] - c["lower_left"]

    def det(x, y, z):
        return (x * np.cross(y, z)).sum(-1)

    # sx a + sy b - k q = r
    mq = -q
    A = np.broadcast_to(a, q.shape)
    B = np.broadcast_to(b, q.shape)
    R = np.broadcast_to(r, q.shape)
    den = det(A, B, mq)
    with np.errstate(all="ignore"):
        sx, sy, k = det(R, B, mq) / den, det(A, R, mq) / den, det(A, B, R) / den
    return sx * w - 0.5, sy * h - 0.5, k > 0


@functools.lru_cache(maxsize=None)
def case(size, prev):
    """A case, computed once and read-only: dict of the six frames, the view, the options, `truth` (h, w, 3) float64 — what A_out holds
    where `compared` (h, w) is set — and `samples`, the history length every compared pixel ends with"""
    w, h = SIZES[size]
    cur, was = cameras(prev, w, h)
    hits = 2 if prev == "half the hits" else SPP
    o, dh, dist = plane_distance(cur, w, h)
    _, dh_p, dist_p = plane_distance(was, w, h)
    f, f_prev = feature_frame(dist, SPP, hits), feature_frame(dist_p, SPP_PREV, SPP_PREV)
    P = o + dh * dist[..., None]
    px, py, front = screen_position(P, was, w, h)
    compared = front & (px >= 0.01) & (px <= w - 1.01) & (py >= 0.01) & (py <= h - 1.01)
    # no tap of a compared pixel fails the depth test: the distance expected against the previous frame's at the four taps, with room to spare.
    # (Taps lighter than 1e-4 are left to the fp32 count in tests/test_accumulate_host.py: under the identical camera px is x to within
    # rounding, and whether the tap of the next column or row weighs 1e-6 or exactly 0 — and so is tested at all — is a matter of fp32.)
    e =np.sqrt(((P - fields(was)["origin"]) ** 2).sum(-1))
    x0, y0 = np.where(compared, np.floor(px), 0).astype(int), np.where(compared, np.floor(py), 0).astype(int)
    for j in (0, 1):
        for i in (0, 1):
            m_q = dist_p[np.clip(y0 + j, 0, h - 1), np.clip(x0 + i, 0, w - 1)]
            weight = (px - x0 if i else 1 - (px - x0)) * (py - y0 if j else 1 - (py - y0))
            tested = compared & (weight > 1e-4)
            assert (np.abs(e - m_q)[tested] <= 0.04 * np.maximum(e, m_q)[tested]).all(), (size, prev, i, j)
    truth = np.stack([px, py, np.ones_like(px)], -1) * (1.0 - ALPHA)
    L = np.zeros((h, w, 3), F)
    V = np.zeros((h, w), binding.MOMENT_DTYPE)
    V["samples"] = 1
    M_prev = np.zeros((h, w), binding.MOMENT_DTYPE)
    M_prev["samples"] = HISTORY
    A_prev = np.ones((h, w, 3), F)
    A_prev[..., 0] = np.arange(w, dtype=F)[None, :]
    A_prev[..., 1] = np.arange(h, dtype=F)[:, None]
    frames = (L, V, f, A_prev, f_prev, M_prev)
    for a in frames + (truth, compared):
        a.setflags(write=False)
    return {"size": (w, h), "frames": frames, "view": ac.view_of(cur, was, SPP, SPP_PREV), "opt": ac.opt(**OPT), "truth": truth, "compared": compared,
            "samples": HISTORY + 1}


def error_in_units(c, A):
    """max |A.xy - truth.xy| over the compared pixels, in units of 2^-24 * max(w, h)"""
    w, h = c["size"]
    m = c["compared"]
    return float(np.abs(np.asarray(A, D)[..., :2] - c["truth"][..., :2])[m].max() / (ALPHA * max(w, h)))


def check_against_truth(c, got, tag=None):
    """asserts that (A, M) is the float64 truth at the compared pixels, that these are most of the frame, and that every one was blended"""
    A, M = got
    w, h = c["size"]
    m = c["compared"]
    assert m.sum() >= MIN_COMPARED * w * h, (tag, int(m.sum()), w * h)
    assert (M["samples"][m] == c["samples"]).all(), (tag, "a compared pixel was not blended")
    assert not M["var"][m].any(), tag
    err = error_in_units(c, A)
    assert err <= TOLERANCE_ULPS, (tag, err)
    z = np.asarray(A)[..., 2][m]
    one = F(1.0 - ALPHA)
    assert ((z >= np.nextafter(one, F(0))) & (z <= np.nextafter(one, F(2)))).all(), (tag, float(z.min()), float(z.max()))
    return err
