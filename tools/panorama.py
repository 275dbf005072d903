#!/usr/bin/env python3
"""tools/panorama.py — an equirectangular 360 x 180 degree view from a point, through the path queries (Renderer.trace_rays, DESIGN.md
§4.22): the example of what they are for — a view no camera of the library generates.  Needs a GPU.

Pixel (x, y) of a W x H image looks along longitude 2 pi (x + (s + 1/2) / spp) / W (sample s of spp: stratified along the row) and
latitude pi (y / (H - 1) - 1/2): row 0 looks straight down, row H - 1 straight up — exactly (0, -1, 0) and (0, 1, 0).  A sample's stream
states are the seeding contract's, r1_seed_sample(seed, y * W + x, s), computed here on the host; a pixel's samples are summed in sample
order in fp32 and quantised as the reference does (rayweek1.cpp:765-775); the image is written with r1_tga_write_rgb24.
usage: tools/panorama.py [--scene small|medium|large] [--width W] [--height H] [--spp N] [--seed S] [--from X Y Z] [--variant V] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32
M32 = np.uint64(0xFFFFFFFF)


def _mix32(v):
    """r1_mix32 of include/rays1_seed.h on uint64 arrays holding 32-bit values"""
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & M32
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & M32
    return v ^ (v >> np.uint64(16))


def seed_samples(seed, pixel, sample):
    """r1_seed_sample(seed, pixel[i], sample[i]) of include/rays1_seed.h as uint32 (n, 4) rows {scalar, lane0, lane1, lane2}"""
    pixel, sample = np.asarray(pixel, np.uint64), np.asarray(sample, np.uint64)
    h = _mix32(np.uint64((int(seed) ^ 0xA511E9B3) & 0xFFFFFFFF) + np.zeros_like(pixel))
    h = _mix32((h + pixel * np.uint64(0x9E3779B9)) & M32)
    h = _mix32(h ^ ((sample * np.uint64(0x85EBCA6B) + np.uint64(0xC2B2AE35)) & M32))
    out = np.zeros((pixel.shape[0], 4), np.uint32)
    for k, add in enumerate((0x01234567, 0x3C6EF372, 0xDAA66D2B, 0x78DDE6E4)):
        v = _mix32((h + np.uint64(add)) & M32)
        out[:, k] = np.where(v == 0, 0x6C078965, v).astype(np.uint32)  # r1_nonzero
    return out


def equirect_rays(origin, w, h, spp, seed):
    """(rays float32 (w * h * spp, 8), seeds uint32 (w * h * spp, 4)) of the panorama from `origin`, in the order ((y * w + x) * spp + s)"""
    assert w >= 1 and h >= 2 and spp >= 1
    y, x, s = (v.reshape(-1) for v in np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij"))
    lon = 2.0 * np.pi * (x + (s + 0.5) / spp) / w
    lat = np.pi * (y / (h - 1.0) - 0.5)
    c = np.cos(lat)
    c[(y == 0) | (y == h - 1)] = 0.0  # the poles, exactly
    rays = np.zeros((x.shape[0], 8), F)
    rays[:, 0:3] = np.asarray(origin, F)
    rays[:, 3] = np.finfo(F).max
    rays[:, 4], rays[:, 5], rays[:, 6] = c * np.cos(lon), np.sin(lat), c * np.sin(lon)
    return rays, seed_samples(seed, y * w + x, s)


def resolve(records, w, h, spp):
    """(h, w, 3) bytes: every pixel's samples summed in sample order in fp32, then col * (1 / spp), sqrt, (uint8)(int)(c * 255.99f)"""
    rec = records.reshape(h, w, spp)
    col = np.zeros((h, w, 3), F)
    for s in range(spp):
        col = col + np.stack([rec["r"][:, :, s], rec["g"][:, :, s], rec["b"][:, :, s]], -1)
    col = np.sqrt((col * (F(1.0) / F(spp))).astype(F)).astype(F)
    with np.errstate(invalid="ignore"):
        return (col * F(255.99)).astype(F).astype(np.int32).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="large", choices=("small", "medium", "large"))
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--seed", type=int, default=10001)
    ap.add_argument("--from", dest="origin", type=float, nargs=3, default=None, help="the view point (default: the scene's lookfrom)")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--max-bounces", type=int, default=50)
    ap.add_argument("--out", default="out_panorama.tga")
    args = ap.parse_args()
    import rays1bench_amd as r1
    from rays1bench_amd import binding
    if r1.device_count() < 1:
        sys.exit("panorama.py: no HIP device (the trace runs on the GPU; there is no fallback)")
    make = {"small": r1.create_small_scene, "medium": r1.create_medium_scene, "large": r1.create_large_scene}[args.scene]
    sc = make(args.width, args.height)
    origin = args.origin if args.origin is not None else sc.camera_array()[0:3]
    rays, seeds = equirect_rays(origin, args.width, args.height, args.spp, args.seed)
    rend = r1.Renderer(0)
    rend.set_scene(sc)
    rec = rend.trace_rays(rays, seeds, args.max_bounces, args.variant)
    img = np.ascontiguousarray(resolve(rec, args.width, args.height, args.spp))
    binding.tga_write_rgb24(args.out, args.width, args.height, img)
    print(f"{args.out}: {args.width} x {args.height} x {args.spp} from {np.asarray(origin, F).tolist()}, {int(rec['rays'].astype(np.uint64).sum())} rays")
    rend.close()
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
