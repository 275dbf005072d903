#!/usr/bin/env python3
"""tools/wavefront.py — a frame rendered level by level on the device with the scatter queries (include/rays1.h "scatter queries",
DESIGN.md §4.34): the worked example of the fold, and its measurement.

    r1_camera_rays_device  ->  r1_scatter_rays_device per level, in place, on the rays still alive (boolean-mask compaction in torch
    between the levels)  ->  the fold (SKY's colour times the path's SCATTERED weights from the last to the first)  ->  the resolve's sum
    in sample order.

Nothing leaves the device between the first ray and the last record; torch does the plumbing, every level's arithmetic is the library's.
`stepped_records` is what tests/test_gpu_scatter_rays.py holds against r1_render_samples, bit for bit.

As a program it checks the stepped frame of the large scene against r1_render_samples (records, ray count, image bytes) and then
measures, in one session, alternating, warmed up, on the host clock around a device synchronisation, medians with the spread:
  (a) one step over the 1200 x 800 x 1 camera rays beside r1_cast_rays_device (CLOSEST) on the same rays;
  (b) the stepped 1200 x 800 x 10 frame beside r1_trace_rays_device on the same rays and beside r1_render;
  (c) r1_camera_rays_device beside the host's r1_camera_rays plus the upload.
No thresholds: the numbers are written down.  The stepped frame is expected to lose to the megakernel; the report says by how much.
usage: tools/wavefront.py [--rounds N] [--out FILE]   (FILE: profiles/rNN/scatter_rays.txt, NN the next free number)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before librays1: one HIP runtime per process)
import rays1bench_amd as r1  # noqa: E402
from rays1bench_amd import binding  # noqa: E402

SCATTERED, SKY, NONE = binding.SCATTER_SCATTERED, binding.SCATTER_SKY, binding.SCATTER_NONE


def camera_rays(rend, params, first=0, n=None, camera=None):
    """the frame's samples [first, first + n) as device tensors: rays (n, 8) and stream states (n, 4), int32 words"""
    n = params.width * params.height * params.spp - first if n is None else n
    rays = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    seeds = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    rend.camera_rays_device(params, first, n, rays.data_ptr(), seeds.data_ptr(), camera=camera, stream=torch.cuda.current_stream().cuda_stream)
    return rays, seeds


def stepped_records(rend, rays, seeds, bounces, variant=0):
    """The fold over device tensors `rays` (n, 8) and `seeds` (n, 4) (int32 words; both are consumed: the steps run in place).  Returns
    (records (n, 4) int32 words {r, g, b, rays} on the device, rays alive at each level)."""
    st = torch.cuda.current_stream().cuda_stream
    n = rays.shape[0]
    alive = torch.arange(n, device="cuda")
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    col = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    lit = torch.zeros(n, dtype=torch.bool, device="cuda")
    path = []  # per level: (rays that SCATTERED there, their weights)
    sizes = []
    for level in range(bounces + 1):
        m = alive.numel()
        if m == 0:
            break
        sizes.append(m)
        rec = torch.empty((m, 8), dtype=torch.int32, device="cuda")
        rend.scatter_rays_device(rays.data_ptr(), seeds.data_ptr(), m, rays.data_ptr(), seeds.data_ptr(), rec.data_ptr(),
                                 binding.SCATTER_UNIT_DIRECTIONS if level else 0, variant, st)
        event = rec[:, 3]
        weight = rec[:, :3].view(torch.float32)
        count[alive] += (event != NONE).to(torch.int32)
        sky = event == SKY
        col[alive[sky]] = weight[sky]
        lit[alive[sky]] = True
        go = event == SCATTERED
        alive = alive[go]
        path.append((alive, weight[go]))
        rays, seeds = rays[go].contiguous(), seeds[go].contiguous()  # (compaction: the next level's launch covers the survivors alone)
    # a0 * (a1 * (... * sky)): the weights from the last to the first, on the paths that reached the sky; the others stay black
    for idx, w in reversed(path):
        col[idx] = torch.where(lit[idx, None], w * col[idx], col[idx])
    out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    out[:, :3] = col.view(torch.int32)
    out[:, 3] = count
    return out, sizes


def stepped_frame(rend, params, variant=0):
    """the whole frame: (records (n, 4) int32 words on the device, rays alive per level)"""
    rays, seeds = camera_rays(rend, params)
    return stepped_records(rend, rays, seeds, params.max_bounces, variant)


def resolve_linear(records, params):
    """the resolve's sum in sample order, times (float)(1.0f / spp): float32 (h, w, 3) on the device"""
    rec = records[:, :3].view(torch.float32).reshape(params.height, params.width, params.spp, 3)
    acc = torch.zeros((params.height, params.width, 3), dtype=torch.float32, device="cuda")
    for s in range(params.spp):
        acc = acc + rec[:, :, s]
    return acc * float(np.float32(1) / np.float32(params.spp))


def timed(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def report(say, title, forms, rounds, unit_count, unit):
    """forms: [(name, run)], alternating; round 0 warms up"""
    res = {name: [] for name, _ in forms}
    for rnd in range(rounds + 1):
        for name, run in forms:
            t = timed(run)
            if rnd:
                res[name].append(t)
    say()
    say(title)
    say(f"{'form':<58} {'median ms':>10} {'min':>9} {'max':>9} {unit:>14}")
    for name, _ in forms:
        v = res[name]
        m = statistics.median(v)
        say(f"{name:<58} {m * 1e3:>10.3f} {min(v) * 1e3:>9.3f} {max(v) * 1e3:>9.3f} {unit_count / m / 1e9:>14.3f}")
    return {name: statistics.median(v) for name, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    w, h, spp, seed = 1200, 800, 10, 10001
    scene = r1.create_large_scene(w, h)
    rend = r1.Renderer(0)
    rend.set_scene(scene)
    p = r1.make_params(w, h, spp, seed)
    st = torch.cuda.current_stream().cuda_stream

    # ---- the check: the stepped frame is r1_render_samples' -------------------------------------------------------------------------------
    img, total, samples = rend.render_samples(p)
    rec, sizes = stepped_frame(rend, p)
    got = rec.cpu().numpy()
    assert got.tobytes() == samples.view(np.int32).tobytes(), "the stepped frame's records are not r1_render_samples'"
    assert int(got[:, 3].astype(np.uint64).sum()) == total
    assert binding.quantise_linear(resolve_linear(rec, p).cpu().numpy()).tobytes() == img.tobytes()
    li = rend.launch_info()
    say(f"scatter queries, large scene {w}x{h}, seed {seed}, {li['compute_units']} CUs; {args.rounds} rounds alternating after one warm-up round, "
        f"host clock around a device synchronisation, medians with min and max")
    say(f"check: the stepped {w}x{h}x{spp} frame equals r1_render_samples: {len(got)} records bit for bit, {total} rays, the image's bytes; "
        f"{len(sizes)} levels, rays alive per level: {sizes[:6]} ... {sizes[-3:]}")

    # ---- (a) one step beside one cast ------------------------------------------------------------------------------------------------------
    p1 = r1.make_params(w, h, 1, seed)
    n1 = w * h
    rays1, seeds1 = camera_rays(rend, p1)
    hits = torch.empty((n1, 8), dtype=torch.int32, device="cuda")
    r_out, s_out, rec1 = torch.empty_like(rays1), torch.empty_like(seeds1), torch.empty((n1, 8), dtype=torch.int32, device="cuda")
    forms = []
    for name, variant in (("tree", binding.VARIANT_BVH), ("grid", binding.VARIANT_GRID)):
        forms.append((f"r1_cast_rays_device CLOSEST, {name}", lambda v=variant: rend.cast_rays_device(rays1.data_ptr(), n1, hits.data_ptr(), binding.CAST_CLOSEST, v, st)))
        forms.append((f"r1_scatter_rays_device, {name}", lambda v=variant: rend.scatter_rays_device(rays1.data_ptr(), seeds1.data_ptr(), n1, r_out.data_ptr(),
                                                                                                   s_out.data_ptr(), rec1.data_ptr(), 0, v, st)))
    report(say, f"(a) one level over the {n1} camera rays of {w}x{h}x1 (Grays/s: rays of the launch)", forms, args.rounds, n1, "Grays/s")

    # ---- (b) the stepped frame beside the path query and the megakernel ----------------------------------------------------------------------
    n = w * h * spp
    rays, seeds = camera_rays(rend, p)
    radiance = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    hf = binding.HostFrame(w, h)

    def stepped(variant):
        r, s = rays.clone(), seeds.clone()  # (the steps run in place; the copies are part of what a caller who keeps the primary rays pays)
        stepped_records(rend, r, s, p.max_bounces, variant)

    forms = [("r1_render (megakernel, image on the host)", lambda: rend.render_into(p, hf.image)),
             ("r1_trace_rays_device, tree", lambda: rend.trace_rays_device(rays.data_ptr(), seeds.data_ptr(), n, radiance.data_ptr(), p.max_bounces, binding.VARIANT_BVH, st)),
             ("stepped: scatter levels + torch compaction + fold, tree", lambda: stepped(binding.VARIANT_BVH)),
             ("r1_trace_rays_device, grid", lambda: rend.trace_rays_device(rays.data_ptr(), seeds.data_ptr(), n, radiance.data_ptr(), p.max_bounces, binding.VARIANT_GRID, st)),
             ("stepped: scatter levels + torch compaction + fold, grid", lambda: stepped(binding.VARIANT_GRID))]
    med = report(say, f"(b) the {w}x{h}x{spp} frame, {total} rays (Grays/s: color() calls of the frame)", forms, args.rounds, total, "Grays/s")
    say(f"the stepped frame takes {med[forms[2][0]] / med[forms[1][0]]:.2f} x the path query's time (tree), {med[forms[4][0]] / med[forms[3][0]]:.2f} x (grid), "
        f"and {med[forms[2][0]] / med[forms[0][0]]:.2f} x r1_render's")
    hf.close()

    # ---- (c) the camera's rays: device form beside host form plus upload ---------------------------------------------------------------------
    y, x, s = np.meshgrid(np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), np.arange(spp, dtype=np.int32), indexing="ij")
    x, y, s = x.reshape(-1), y.reshape(-1), s.reshape(-1)
    cam = scene.camera.contents

    def host_form():
        hr, hs = binding.camera_rays(cam, p, x, y, s)
        rays.copy_(torch.from_numpy(hr.view(np.int32).reshape(-1, 8)))
        seeds.copy_(torch.from_numpy(hs.view(np.int32).reshape(-1, 4)))

    forms = [("r1_camera_rays (host) + upload", host_form),
             ("r1_camera_rays_device", lambda: rend.camera_rays_device(p, 0, n, rays.data_ptr(), seeds.data_ptr(), stream=st))]
    report(say, f"(c) the {n} camera rays and stream states of {w}x{h}x{spp}, {n * 48 / 1e6:.0f} MB (Grays/s: rays made)", forms, args.rounds, n, "Grays/s")
    hr, hs = binding.camera_rays(cam, p, x, y, s)
    assert rays.cpu().numpy().tobytes() == hr.tobytes() and seeds.cpu().numpy().tobytes() == hs.tobytes()
    say("the device form's bytes are the host form's")

    rend.close()
    scene.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
