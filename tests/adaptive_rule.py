"""The stopping rule of r1_render_adaptive (include/rays1.h) restated in numpy, for tests/test_adaptive_host.py and
tests/test_gpu_adaptive.py.  Input: per-sample records rec[h, w, cap, 4] (r, g, b as float32, the ray count as the bits of the fourth
word), as r1_render_samples and the oracle's render_frame(..., want_samples=True) return them."""
import numpy as np


def quantise(col, n):
    """r1_resolve_kernel's arithmetic on sequential fp32 sums: * (float)(1.0f / n), sqrtf, (uint8)(int)(c * 255.99f)
    (tests/test_gpu_progressive.py:_quantise)."""
    c = col.astype(np.float32) * (np.float32(1.0) / np.float32(n))
    return (np.sqrt(c) * np.float32(255.99)).astype(np.int32).astype(np.uint8)


def schedule(cap, min_spp, pass_spp):
    n = [min(min_spp, cap)]
    while n[-1] < cap:
        n.append(min(n[-1] + pass_spp, cap))
    return n


def tile_boxes(w, h, tile_w=32, tile_h=32):
    """[(x0, y0, x1, y1)] of tile t = ty * tiles_x + tx, clipped to the image."""
    return [(x0, y0, min(x0 + tile_w, w), min(y0 + tile_h, h)) for y0 in range(0, h, tile_h) for x0 in range(0, w, tile_w)]


def restate(rec, min_spp, pass_spp, max_delta, mean_delta_q8, tile_w=32, tile_h=32):
    """Returns (reports, rays): reports a structured array (spp, settled, err_max, err_sum) per tile, rays the color() calls of the
    samples s < spp(tile) of every pixel."""
    h, w, cap, _ = rec.shape
    sched = set(schedule(cap, min_spp, pass_spp))
    boxes = tile_boxes(w, h, tile_w, tile_h)
    rep = np.zeros(len(boxes), np.dtype([("spp", np.int32), ("settled", np.int32), ("err_max", np.uint32), ("err_sum", np.uint32)]))
    active = [True] * len(boxes)
    all_ = np.zeros((h, w, 3), np.float32)
    even = np.zeros((h, w, 3), np.float32)
    for s in range(cap):
        all_ = all_ + rec[:, :, s, :3]
        if s % 2 == 0:
            even = even + rec[:, :, s, :3]
        if s + 1 not in sched:
            continue
        d = np.abs(quantise(all_, s + 1).astype(np.int64) - quantise(even, (s + 2) // 2).astype(np.int64))
        for t, (x0, y0, x1, y1) in enumerate(boxes):
            if not active[t]:
                continue
            dt = d[y0:y1, x0:x1]
            err_max, err_sum = int(dt.max()), int(dt.sum())
            settled = err_max <= max_delta and err_sum * 256 <= mean_delta_q8 * 3 * (x1 - x0) * (y1 - y0)
            rep[t] = (s + 1, int(settled), err_max, err_sum)
            if settled or s + 1 == cap:
                active[t] = False
    assert not any(active)
    words = np.ascontiguousarray(rec[..., 3]).view(np.uint32).astype(np.uint64)
    rays = 0
    for t, (x0, y0, x1, y1) in enumerate(boxes):
        rays += int(words[y0:y1, x0:x1, :int(rep[t]["spp"])].sum())
    return rep, rays


def histogram(rep):
    """{final sample count: tiles}"""
    n, c = np.unique(rep["spp"], return_counts=True)
    return {int(a): int(b) for a, b in zip(n, c)}


def samples_of(rep, w, h, tile_w=32, tile_h=32):
    return sum(int(rep[t]["spp"]) * (x1 - x0) * (y1 - y0) for t, (x0, y0, x1, y1) in enumerate(tile_boxes(w, h, tile_w, tile_h)))
