"""What tests/test_denoise_guided_host.py and tests/test_gpu_denoise_guided.py share (variance-guided denoised frames, include/rays1.h,
DESIGN.md §4.40): the guided contract restated in numpy float32 from its text — tests/denoise_cases.py's numpy_denoise with the contract's
four changes —, a seeded variance frame for denoise_cases' synthetic frames that holds every class of value the contract names, the
rendered cases, and the host form's results, computed once.  Nothing here has a tolerance."""
import functools

import numpy as np

import rays1bench_amd as r1
from rays1bench_amd import binding

import denoise_cases as dc
import feature_cases as fc
import linear_cases as lc

F = np.float32
H5 = dc.H5
K3 = np.array([1 / 4, 1 / 2, 1 / 4], F)
# the defaults DESIGN.md §4.40 chose on the medium scene
OPT = dict(iterations=3, normal_power_log2=6, sigma_color=2.0, sigma_depth=0.1, flags=binding.DENOISE_DEMODULATE, variance_floor=1e-4)
# option sets: the defaults, then both flag values and both ends of every range
OPTION_SETS = {"defaults": {}, "low ends": dict(iterations=1, normal_power_log2=0, sigma_color=1e-3, sigma_depth=1e-3, variance_floor=1e-30, flags=0),
               "high ends": dict(iterations=8, normal_power_log2=10, sigma_color=1e3, sigma_depth=1e3, variance_floor=1e30),
               "plain": dict(flags=0, variance_floor=1e-6, sigma_color=1.0)}


def opt(**kw):
    d = dict(OPT)
    d.update(kw)
    return binding.make_denoise_guided_opt(**d)


def numpy_guided(L, f, V, o):
    """The contract for a DenoiseGuidedOpt o and a MOMENT_DTYPE frame V"""
    b = o.base
    return numpy_denoise_guided(L, f, V["var"], b.iterations, b.normal_power_log2, b.sigma_color, b.sigma_depth, o.variance_floor,
                                bool(b.flags & binding.DENOISE_DEMODULATE))


def numpy_denoise_guided(L, f, V, iterations, normal_power_log2, sigma_color, sigma_depth, variance_floor, demodulate=True):
    """L (h, w, 3) float32, f FEATURE_DTYPE (h, w), V (h, w, 3) float32 variances of L -> (h, w, 3).  One rounded float32 operation per
    element and line, in the order of the text above; a skipped tap leaves the sums untouched."""
    L = np.asarray(L, F)
    h, w = L.shape[:2]
    surf = f["hits"] > 0
    with np.errstate(all="ignore"):
        a = np.where(f["albedo"] < F(1 / 256), F(1 / 256), f["albedo"]).astype(F) if demodulate else np.ones((h, w, 3), F)
        e = L / a
        n = f["normal"].astype(F)
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        ln = np.sqrt(nn)
        nh = np.where((ln > 0)[..., None], n / ln[..., None], F(0)).astype(F)
        m = np.where(surf, f["depth"] / np.maximum(f["hits"], 1).astype(F), F(0)).astype(F)
        Vs = np.where(surf[..., None], V, F(0)).astype(F)  # (V of a pixel without a hit is never read into a result)
        v = np.where(surf, (Vs[..., 0] / (a[..., 0] * a[..., 0]) + Vs[..., 1] / (a[..., 1] * a[..., 1])) + Vs[..., 2] / (a[..., 2] * a[..., 2]), F(0)).astype(F)
        cur = e.copy()
        sd, floor = F(sigma_depth), F(variance_floor)
        sc2 = F(sigma_color) * F(sigma_color)
        for i in range(iterations):
            step = 1 << i
            # the 3 x 3 prefilter of v, one pixel apart
            v1, s1 = np.pad(v, 1), np.pad(surf, 1)
            G, K = np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    ys, xs = slice(1 + dy, 1 + dy + h), slice(1 + dx, 1 + dx + w)
                    k = K3[dy + 1] * K3[dx + 1]
                    G = np.where(s1[ys, xs], G + k * v1[ys, xs], G)
                    K = np.where(s1[ys, xs], K + k, K)
            g = G / np.where(surf, K, F(1))
            den_c = sc2 * g + floor
            pad = 2 * step
            cur_p = np.pad(cur, ((pad, pad), (pad, pad), (0, 0)))
            nh_p = np.pad(nh, ((pad, pad), (pad, pad), (0, 0)))
            m_p, v_p, surf_p = np.pad(m, pad), np.pad(v, pad), np.pad(surf, pad)
            S, W, T = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ys, xs = slice(pad + dy * step, pad + dy * step + h), slice(pad + dx * step, pad + dx * step + w)
                    cq, nq, mq, vq, taken = cur_p[ys, xs], nh_p[ys, xs], m_p[ys, xs], v_p[ys, xs], surf_p[ys, xs]
                    hh = H5[dy + 2] * H5[dx + 2]
                    if dx == 0 and dy == 0:
                        wt = np.full((h, w), hh, F)
                    else:
                        c = (nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1]) + nh[..., 2] * nq[..., 2]
                        c = np.where(c < 0, F(0), c)
                        c = np.where(c > 1, F(1), c)
                        for _ in range(normal_power_log2):
                            c = c * c
                        mx = np.where(m < mq, mq, m)
                        den = sd * mx
                        rz = np.where(den > 0, (m - mq) / np.where(den > 0, den, F(1)), F(0))
                        xz = rz * rz
                        d = cur - cq
                        dcol = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                        xc = dcol / den_c
                        wt = (hh * c) / ((F(1) + xz) * (F(1) + xc))
                    wt = wt.astype(F)
                    S = np.where(taken[..., None], S + wt[..., None] * cq, S)
                    W = np.where(taken, W + wt, W)
                    T = np.where(taken, T + (wt * wt) * vq, T)
            Ws = np.where(surf, W, F(1))
            cur = np.where(surf[..., None], S / Ws[..., None], cur).astype(F)
            v = np.where(surf, T / (Ws * Ws), F(0)).astype(F)
        out = np.where(surf[..., None], cur * a, L)
    assert out.dtype == F
    return out


@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """(L, f) of dc.synthetic(w, h) with, where the size allows, one hit pixel whose eight neighbours have no hit.  Read-only."""
    L, f = dc.synthetic(w, h)
    f = f.copy()
    if w >= 24 and h >= 18:
        ring = f[14:17, 19:22]
        centre = ring[1, 1].copy()
        ring[...] = np.zeros((), binding.FEATURE_DTYPE)
        if centre["hits"] == 0:
            centre["hits"], centre["depth"], centre["normal"], centre["albedo"] = 2, 5.0, (0, 0, 2), (0.5, 0.25, 0.75)
        ring[1, 1] = centre
    f.setflags(write=False)
    return L, f


@functools.lru_cache(maxsize=None)
def synthetic_v(w, h, seed=4040):
    """A seeded MOMENT_DTYPE frame for synthetic(w, h) that holds, where the size allows, every class v_classes() counts.  Read-only."""
    _, f = synthetic(w, h)
    surf = f["hits"] > 0
    rng = np.random.default_rng(seed + 1000 * w + h)
    V = np.zeros((h, w), binding.MOMENT_DTYPE)
    var = (rng.uniform(0.0, 0.05, (h, w, 3)) ** 2).astype(F)
    if w >= 12 and h >= 8:
        var[6:9, 2:8] = 0                      # a block of var = 0 (on hit pixels, mostly)
        var[h - 6, 1:4] = F(1e30)              # sums that overflow
        var[1, 1:5] = F(1e-41)                 # subnormal values
        var[rng.random((h, w)) < 0.03] = F(1e-42)
    else:
        var[0, 0] = [0, F(1e-41), F(1e30)] if w == 1 else var[0, 0]
    var[~surf] = np.nan                        # never read into any result
    V["var"] = var
    V["samples"] = 4
    V.setflags(write=False)
    return V


def v_classes(f, V):
    """How many pixels of a frame fall into each class of variance input the contract names"""
    surf = f["hits"] > 0
    h, w = surf.shape
    var = V["var"]
    sp = np.pad(surf, 1)
    neigh = sum(sp[1 + dy:1 + dy + h, 1 + dx:1 + dx + w].astype(int) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) - surf.astype(int)
    tiny = np.finfo(F).tiny
    zero_blocks = sum(1 for y in range(h - 1) for x in range(w - 1) if surf[y:y + 2, x:x + 2].all() and not var[y:y + 2, x:x + 2].any())
    return {"2x2 blocks of var 0 on hit pixels": zero_blocks, "values of 1e30 on hit pixels": int((surf[..., None] & (var == F(1e30))).sum()),
            "subnormal values on hit pixels": int((surf[..., None] & (var > 0) & (var < tiny)).sum()),
            "NaN on pixels without a hit": int((~surf[..., None] & np.isnan(var)).sum()), "NaN on hit pixels": int((surf[..., None] & np.isnan(var)).sum()),
            "hit pixels alone in their 3x3": int((surf & (neigh == 0)).sum())}


@functools.lru_cache(maxsize=None)
def rendered(name, seed=fc.SEED):
    """(L, f, V) of a rendered case: dc.rendered's frames and r1_render_moments_host's variance frame of the same params.  Read-only."""
    L, f = dc.rendered(name, seed)
    sa, p = fc.scene(name), fc.params(name, seed=seed)
    L2, V, _ = binding.render_moments_host(lc.cscene(sa), lc.ccamera(sa), p)
    assert L2.tobytes() == L.tobytes()
    V.setflags(write=False)
    return L, f, V


def inputs(name):
    """(L, f, V, iterations) of a case by name"""
    if name in dc.RENDERED:
        return rendered(name) + (OPT["iterations"],)
    w, h, it = {**dc.SYNTHETIC, **dc.DEVICE_ONLY}[name]
    return synthetic(w, h) + (synthetic_v(w, h), it)


@functools.lru_cache(maxsize=None)
def host_result(name, **kw):
    """r1_denoise_guided_host of the case with opt(**kw) (iterations: the case's unless given).  Read-only."""
    L, f, V, it = inputs(name)
    kw.setdefault("iterations", it)
    out = binding.denoise_guided_host(L, f, V, opt(**kw))
    out.setflags(write=False)
    return out
