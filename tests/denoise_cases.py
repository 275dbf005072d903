"""What tests/test_denoise_host.py and tests/test_gpu_denoise.py share (denoised frames, include/rays1.h): the contract
re-stated in numpy float32 from its text — whole-frame array operations over shifted views, nothing of the C —, seeded synthetic frames
that hold every class of input the contract names, the rendered cases (tests/feature_cases.py's frames with r1_render_linear_host's), and
the host form's results, computed once per case and left unchanged.  Nothing here has a tolerance."""
import functools

import numpy as np

import rays1bench_amd as r1
from rays1bench_amd import binding

import feature_cases as fc
import linear_cases as lc

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)
PREFILL = 0xA5
# the options the issue measured with, and the ends of every option's range
OPT = dict(iterations=3, normal_power_log2=6, sigma_color=1.0, sigma_depth=0.1, flags=binding.DENOISE_DEMODULATE)
# name -> (width, height, iterations): the synthetic frames of the host test, then those only the device tests need
SYNTHETIC = {"1x1": (1, 1, 3), "5x3": (5, 3, 4), "37x21": (37, 21, 3), "70x40": (70, 40, 5)}
DEVICE_ONLY = {"65x33": (65, 33, 3), "257x17": (257, 17, 3), "150x141": (150, 141, 5)}
RENDERED = ("medium", "large")  # feature_cases' 33 x 17 x 3 and 64 x 48 x 4


def opt(**kw):
    d = dict(OPT)
    d.update(kw)
    return binding.make_denoise_opt(**d)


def numpy_denoise(L, f, o):
    """The contract in numpy float32.  L (h, w, 3), f FEATURE_DTYPE (h, w), o a DenoiseOpt -> (h, w, 3).  Every line is one rounded operation
    per element, in the contract's order; a skipped tap leaves the sums untouched (np.where chooses the old sum)."""
    L = np.asarray(L, F)
    h, w = L.shape[:2]
    surf = f["hits"] > 0
    with np.errstate(all="ignore"):
        if o.flags & binding.DENOISE_DEMODULATE:
            a = np.where(f["albedo"] < F(1 / 256), F(1 / 256), f["albedo"]).astype(F)
        else:
            a = np.ones((h, w, 3), F)
        e = L / a
        n = f["normal"].astype(F)
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        l = np.sqrt(nn)
        nh = np.where((l > 0)[..., None], n / l[..., None], F(0)).astype(F)
        m = np.where(surf, f["depth"] / np.maximum(f["hits"], 1).astype(F), F(0)).astype(F)
        cur = e.copy()
        sigma_depth = F(o.sigma_depth)
        for i in range(o.iterations):
            step = 1 << i
            sc = F(o.sigma_color) * F(2.0 ** -i)
            sc2 = sc * sc
            pad = 2 * step
            cur_p = np.pad(cur, ((pad, pad), (pad, pad), (0, 0)))
            nh_p = np.pad(nh, ((pad, pad), (pad, pad), (0, 0)))
            m_p = np.pad(m, pad)
            surf_p = np.pad(surf, pad)  # (off the image: False, the tap is skipped)
            S, W = np.zeros((h, w, 3), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ys, xs = slice(pad + dy * step, pad + dy * step + h), slice(pad + dx * step, pad + dx * step + w)
                    cq, nq, mq, taken = cur_p[ys, xs], nh_p[ys, xs], m_p[ys, xs], surf_p[ys, xs]
                    hh = H5[dy + 2] * H5[dx + 2]
                    if dx == 0 and dy == 0:
                        wt = np.full((h, w), hh, F)
                    else:
                        c = (nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1]) + nh[..., 2] * nq[..., 2]
                        c = np.where(c < 0, F(0), c)
                        c = np.where(c > 1, F(1), c)
                        for _ in range(o.normal_power_log2):
                            c = c * c
                        mx = np.where(m < mq, mq, m)
                        den = sigma_depth * mx
                        rz = np.where(den > 0, (m - mq) / np.where(den > 0, den, F(1)), F(0))
                        xz = rz * rz
                        d = cur - cq
                        dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                        xc = dc / sc2
                        wt = (hh * c) / ((F(1) + xz) * (F(1) + xc))
                    wt = wt.astype(F)
                    S = np.where(taken[..., None], S + wt[..., None] * cq, S)
                    W = np.where(taken, W + wt, W)
            nxt = S / np.where(surf, W, F(1))[..., None]
            cur = np.where(surf[..., None], nxt, cur).astype(F)
        out = np.where(surf[..., None], cur * a, L)
    assert out.dtype == F
    return out


@functools.lru_cache(maxsize=None)
def synthetic(w, h, seed=20240):
    """(L, f) of a seeded w x h frame that holds, where its size allows, every class classes() counts.  Read-only."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    f = np.zeros((h, w), binding.FEATURE_DTYPE)
    hits = rng.integers(1, 5, (h, w)).astype(np.uint32)
    hits[rng.random((h, w)) < 0.04] = 0
    if w >= 12 and h >= 8:
        hits[2:6, 3:10] = 0      # a block without a hit, wider than a step-1 kernel
        hits[h - 3:, w - 5:] = 0  # ... and one in a corner
    surf = hits > 0
    # normals: sums of `hits` unit vectors, so lengths vary; a palette whose pairwise cosines make c^(2^k) subnormal (0.25^64 = 2^-128) and zero
    palette = np.array([[0, 0, 1], [np.sqrt(15) / 4, 0, 0.25], [0.995, 0, 0.1], [0, 1, 0], [0, 0, -1], [0.6, 0, 0.8]], F)
    pick = rng.integers(0, len(palette) + 2, (h, w))
    rnd = rng.normal(size=(h, w, 3)).astype(F)
    rnd /= np.linalg.norm(rnd, axis=-1, keepdims=True).astype(F)
    normal = np.where((pick < len(palette))[..., None], palette[np.minimum(pick, len(palette) - 1)], rnd).astype(F)
    normal = normal * (hits.astype(F) * rng.uniform(0.3, 1.0, (h, w)).astype(F))[..., None]
    normal[rng.random((h, w)) < 0.03] = 0  # a hit pixel whose normals cancel
    # mean distances: many equal, some a thousand times the others
    mean = np.where(rng.random((h, w)) < 0.5, F(2.5), rng.uniform(0.5, 20.0, (h, w)).astype(F)).astype(F)
    mean[rng.random((h, w)) < 0.1] *= F(1000)
    albedo = rng.uniform(0.05, 1.0, (h, w, 3)).astype(F)
    albedo[rng.random((h, w)) < 0.05] = 0
    albedo[rng.random((h, w)) < 0.05] = F(1 / 1024)
    L = (albedo * rng.uniform(0.0, 2.0, (h, w, 3)).astype(F) + rng.uniform(0.0, 0.05, (h, w, 3)).astype(F)).astype(F)
    L[:, w // 2:] *= np.where(rng.random((h, w - w // 2)) < 0.3, F(1e4), F(1))[..., None]  # colour steps of 1e4
    f["hits"] = hits
    f["albedo"] = albedo
    f["normal"] = np.where(surf[..., None], normal, F(0))
    f["depth"] = np.where(surf, mean * hits.astype(F), F(0))
    L.setflags(write=False), f.setflags(write=False)
    return L, f


def classes(L, f, k=6):
    """How many pixels (or horizontal neighbour pairs of hit pixels) of a frame fall into each class of input the contract names."""
    surf = f["hits"] > 0
    n = f["normal"]
    with np.errstate(all="ignore"):
        l = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        nh = np.where((l > 0)[..., None], n / l[..., None], F(0)).astype(F)
        m = np.where(surf, f["depth"] / np.maximum(f["hits"], 1).astype(F), F(0)).astype(F)
        pair = surf[:, 1:] & surf[:, :-1]
        c = (nh[:, 1:, 0] * nh[:, :-1, 0] + nh[:, 1:, 1] * nh[:, :-1, 1]) + nh[:, 1:, 2] * nh[:, :-1, 2]
        c = np.clip(c, F(0), F(1))
        cosine = c.copy()
        for _ in range(k):
            c = c * c
        ratio = np.maximum(m[:, 1:], m[:, :-1]) / np.minimum(m[:, 1:], m[:, :-1])
        e = L / np.where(f["albedo"] < F(1 / 256), F(1 / 256), f["albedo"])
        jump = np.abs(e[:, 1:] - e[:, :-1]).max(axis=-1)
    tiny = np.finfo(F).tiny
    blocks = sum(1 for y in range(surf.shape[0] - 2) for x in range(surf.shape[1] - 2) if not surf[y:y + 3, x:x + 3].any())
    return {"no-hit 3x3 blocks": blocks, "no-hit pixels": int((~surf).sum()), "hit pixels": int(surf.sum()),
            "hit pixels with a zero normal": int((surf & (l == 0)).sum()),
            "albedo 0": int((surf[..., None] & (f["albedo"] == 0)).sum()), "albedo in (0, 1/256)": int((surf[..., None] & (f["albedo"] > 0) & (f["albedo"] < F(1 / 256))).sum()),
            "equal depths": int((pair & (m[:, 1:] == m[:, :-1])).sum()), "depths 1000x apart": int((pair & (ratio >= 1000)).sum()),
            "colour steps >= 1e4": int((pair & (jump >= 1e4)).sum()),
            "c^(2^k) subnormal": int((pair & (c > 0) & (c < tiny)).sum()), "c^(2^k) zero from c > 0": int((pair & (c == 0) & (cosine > 0)).sum())}


@functools.lru_cache(maxsize=None)
def rendered(name, seed=fc.SEED):
    """(L, f) of a rendered case: r1_render_linear_host's frame and feature_cases' host feature frame of the same params.  Read-only."""
    sa, p = fc.scene(name), fc.params(name, seed=seed)
    L, _ = binding.render_linear_host(lc.cscene(sa), lc.ccamera(sa), p)
    L.setflags(write=False)
    return L, fc.host_frame(name, seed)


def inputs(name):
    """(L, f, iterations) of a case by name"""
    if name in RENDERED:
        return rendered(name) + (OPT["iterations"],)
    w, h, it = {**SYNTHETIC, **DEVICE_ONLY}[name]
    return synthetic(w, h) + (it,)


@functools.lru_cache(maxsize=None)
def host_result(name, **kw):
    """r1_denoise_host of the case with opt(**kw) (iterations: the case's unless given): what every device result is compared with.  Read-only."""
    L, f, it = inputs(name)
    kw.setdefault("iterations", it)
    out = binding.denoise_host(L, f, opt(**kw))
    out.setflags(write=False)
    return out


def strided(a, pitch, fill=PREFILL):
    """a copy of `a` as a view of a buffer whose rows are `pitch` pixels apart, every other byte `fill`: (view, buffer)"""
    h, w = a.shape[:2]
    buf = np.frombuffer(bytes([fill]) * (h * pitch * a.dtype.itemsize * int(np.prod(a.shape[2:], dtype=int))), a.dtype).copy().reshape((h, pitch) + a.shape[2:])
    view = buf[:, :w]
    view[...] = a
    return view, buf


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
