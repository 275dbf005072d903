#!/usr/bin/env python3
"""tools/trace_rays_bench.py — what the path queries cost (r1_trace_rays*); measurement tool, needs a GPU and torch,
reads no file outside the repository.  Fails without a device: there is no fallback.

The rays of a whole frame come from r1_camera_rays and are uploaded once, so a trace follows the very same paths as r1_render of that
frame; the ratio of the two times is the price of 64 bytes of memory traffic per ray (32 ray + 16 seed + 16 record) and of the generic
loop (one attenuation-stack entry in global memory per bounce, no tiles).
  (a) large scene, 1200 x 800 x 10 (the benchmark's 9.6 M samples): r1_trace_rays_device per variant, HIP events around the enqueue,
      against r1_render's trace-kernel time (r1_last_timing) of the same frame and variant; alternating, --pairs pairs after a warm-up.
  (b) the same on config 5's scene (create_grid_scene 400 x 250: 100 004 spheres) at 1920 x 1080 x 4.
  (c) the host-memory form, 2^22 rays of (a), copies included (host clock).
None of these is a threshold.  Writes its report to profiles/r14/trace_rays.txt (--out FILE: somewhere else).
usage: tools/trace_rays_bench.py [--pairs N] [--skip-config5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_samples(w, h, spp):
    y, x, s = np.meshgrid(np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), np.arange(spp, dtype=np.int32), indexing="ij")
    return x.reshape(-1), y.reshape(-1), s.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "trace_rays.txt"))
    args = ap.parse_args()
    import torch
    import rays1bench_amd as r1
    from rays1bench_amd import binding
    if r1.device_count() < 1:
        sys.exit("trace_rays_bench.py: no HIP device (nothing is measured without one)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    V = (("tree", binding.VARIANT_BVH), ("grid", binding.VARIANT_GRID))
    rend = r1.Renderer(0)
    stream = torch.cuda.Stream()

    def workload(sc, w, h, spp, seed):
        rend.set_scene(sc)
        p0 = r1.make_params(w, h, spp, seed)
        x, y, s = frame_samples(w, h, spp)
        rays, seeds = binding.camera_rays(sc.camera.contents, p0, x, y, s)
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).cuda()
        d_seeds = torch.from_numpy(seeds.view(np.int32).reshape(-1, 4)).cuda()
        d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        img = np.zeros((h, w, 3), np.uint8)
        for name, variant in V:
            p = r1.make_params(w, h, spp, seed, variant=variant)

            def trace_ms():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record(stream)
                    rend.trace_rays_device(d_rays.data_ptr(), d_seeds.data_ptr(), n, d_out.data_ptr(), 50, variant, stream.cuda_stream)
                    e1.record(stream)
                    e1.synchronize()
                return e0.elapsed_time(e1)

            def render_ms():
                rays_n = rend.render_into(p, img)[0]
                return rend.last_timing()[0], rays_n

            trace_ms(), render_ms()  # warm-up: occupancy queries, the grid's build, workspaces
            t_trace, t_render, rays_n = [], [], 0
            for _ in range(args.pairs):
                t_trace.append(trace_ms())
                tr, rays_n = render_ms()
                t_render.append(tr)
            traced = int(d_out.cpu().numpy().view(np.uint32)[:, 3].astype(np.uint64).sum())
            mt, mr = statistics.median(t_trace), statistics.median(t_render)
            say(f"  {name:<5} r1_trace_rays_device {mt:8.3f} ms (min {min(t_trace):.3f}, max {max(t_trace):.3f})   r1_render's trace kernel {mr:8.3f} ms "
                f"(min {min(t_render):.3f}, max {max(t_render):.3f})   ratio {mt / mr:5.2f}   {rays_n / mt / 1e6:6.2f} against {rays_n / mr / 1e6:6.2f} Grays/s"
                f"   color() calls {'equal' if traced == rays_n else 'DIFFER'} ({traced})")
        return rays, seeds

    w, h, spp = 1200, 800, 10
    sc = r1.create_large_scene(w, h)
    say(f"(a) large scene ({int((sc.arrays()['inv_radius'] != 0).sum())} spheres), {w} x {h} x {spp} = {w * h * spp} rays from r1_camera_rays, resident on the device; "
        f"{args.pairs} alternating pairs after a warm-up, medians")
    rays, seeds = workload(sc, w, h, spp, 10001)
    say()
    n = 1 << 22
    say(f"(c) the host-memory form, the first {n} rays of (a), copies included (host clock, {args.pairs} calls after a warm-up)")
    for name, variant in V:
        rend.trace_rays(rays[:n], seeds[:n], 50, variant)
        t = []
        for _ in range(args.pairs):
            t0 = time.perf_counter()
            rend.trace_rays(rays[:n], seeds[:n], 50, variant)
            t.append((time.perf_counter() - t0) * 1e3)
        say(f"  {name:<5} r1_trace_rays {statistics.median(t):8.3f} ms (min {min(t):.3f}, max {max(t):.3f}) = {n / statistics.median(t) / 1e3:6.2f} M rays/s")
    sc.close()
    if not args.skip_config5:
        w, h, spp = 1920, 1080, 4
        sc = r1.create_grid_scene(w, h, 400, 250)
        say()
        say(f"(b) config 5's scene ({int((sc.arrays()['inv_radius'] != 0).sum())} spheres), {w} x {h} x {spp} = {w * h * spp} rays")
        workload(sc, w, h, spp, 10001)
        sc.close()
    rend.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
