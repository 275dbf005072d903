#!/usr/bin/env python3
"""tools/update_bench.py — moving spheres (r1_update_centers*) against the only way there was to move one, r1_set_scene
(measurement tool; needs a GPU, reads no file outside the repository).

On the 100 004-sphere lattice of BASELINE config 5 (grid 400 x 250) at 1200 x 800 x 10, one context, in ONE session and alternating:
  (a) the time of one update of every centre, host form and device form (enqueue to stream idle), against one r1_set_scene with the
      same moved arrays;
  (b) the frame time after a refit for displacements of 0, 0.25, 1 and 4 lattice spacings (every lattice sphere, in a fixed pseudo-random
      direction of the plane) against a fresh build of the same moved scene — the number that tells a caller when to rebuild; the two
      frames are compared byte for byte on the way.
On the large scene (484 spheres, a tree with a flat y slab):
  (c) a frame after an identity update against one before it: the price of the dropped slab.
Frames are r1_render_async into page-locked memory, timed from the enqueue to the stream idle by the host's clock.
Writes its report to profiles/r11/update.txt (--out FILE: somewhere else).
usage: tools/update_bench.py [--rounds N] [--frames N] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("center_x", "center_y", "center_z", "radius_sq", "inv_radius", "albedo_r", "albedo_g", "albedo_b", "mat_param")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="frames per timing of (b) and (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "update.txt"), help="where the report is written")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rays1bench_amd as r1
    from rays1bench_amd import binding

    def lattice_of(a):
        """scene indices of the lattice: every hittable sphere but the four largest (the ground and the three big balls)"""
        act = np.nonzero(a["inv_radius"] != 0)[0]
        return np.setdiff1d(act, act[np.argsort(a["radius_sq"][act], kind="stable")[-4:]])

    def raw_from_arrays(a, x, y, z):
        """a CScene over the scene's arrays with other centres (the returned dict keeps the arrays alive)"""
        keep = {k: np.ascontiguousarray(a[k], np.float32).copy() for k in FIELDS}
        keep["center_x"], keep["center_y"], keep["center_z"] = (np.ascontiguousarray(v, np.float32).copy() for v in (x, y, z))
        keep["mat_type"] = np.ascontiguousarray(a["mat_type"], np.uint8).copy()
        cs = binding.CScene()
        cs.count = len(keep["mat_type"])
        for k in FIELDS:
            setattr(cs, k, keep[k].ctypes.data_as(C.POINTER(C.c_float)))
        cs.mat_type = keep["mat_type"].ctypes.data_as(C.POINTER(C.c_uint8))
        return cs, keep

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def spread(v):
        return f"{statistics.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n = {len(v)})"

    w, h, spp, seed = 1200, 800, 10, 10001
    p = r1.make_params(w, h, spp, seed)
    hf = binding.HostFrames(w, h, 1)

    def frame_ms(ctx, n):
        def go():
            ctx.render_async(p, hf)
            ctx.sync()
        go()  # workspaces
        return [ms(go) for _ in range(n)]

    # ---- config 5's scene ----
    sc = r1.create_grid_scene(w, h, 400, 250)
    a = sc.arrays()
    lat = lattice_of(a)
    n = sc.count
    spacing = float(np.ptp(a["center_x"][lat])) / 399.0
    say(f"config 5's scene: {n} spheres ({len(lat)} in the lattice, spacing {spacing:.4f}), {w} x {h} x {spp}, one context")
    rng = np.random.default_rng(5)
    ang = rng.uniform(0, 2 * np.pi, len(lat))

    def displaced(d):
        x, y, z = (a[k].copy() for k in ("center_x", "center_y", "center_z"))
        x[lat] = (x[lat] + d * spacing * np.cos(ang)).astype(np.float32)
        z[lat] = (z[lat] + d * spacing * np.sin(ang)).astype(np.float32)
        return x, y, z

    ctx, other = r1.Renderer(0), r1.Renderer(0)
    ctx.set_scene(sc)
    say()
    say("(a) one update of all centres against one r1_set_scene with the same arrays (alternating, displacements 0.25 and 0.5 by turns)")
    t_host, t_dev, t_set = [], [], []
    for r in range(args.rounds + 1):
        x, y, z = displaced(0.25 + 0.25 * (r % 2))
        tx, ty, tz = (torch.from_numpy(v).cuda() for v in (x, y, z))
        torch.cuda.synchronize()
        cs, keep = raw_from_arrays(a, x, y, z)

        def host_form():
            ctx.update_centers(0, x, y, z)
            ctx.sync()

        def device_form():
            binding._check(binding.lib().r1_update_centers_device(ctx._c, 0, n, tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), None))
            ctx.sync()

        th, td, ts = ms(host_form), ms(device_form), ms(lambda: ctx.set_scene_raw(cs, sc.camera.contents))
        if r:  # (round 0: staging buffer, first launches)
            t_host.append(th), t_dev.append(td), t_set.append(ts)
        ctx.set_scene(sc)
    say(f"  r1_update_centers         {spread(t_host)}")
    say(f"  r1_update_centers_device  {spread(t_dev)}")
    say(f"  r1_set_scene              {spread(t_set)}")
    say(f"  r1_set_scene / update: host form {statistics.median(t_set) / statistics.median(t_host):.1f} x, device form "
        f"{statistics.median(t_set) / statistics.median(t_dev):.1f} x")
    li = ctx.launch_info()
    say(f"  (tree: {li['bvh_nodes']} nodes, {li['bvh_leaves']} leaves, depth {li['bvh_depth']}: one launch per height)")
    say()
    say(f"(b) frame time after a refit against a fresh build of the same moved scene ({args.frames} frames per timing, {args.rounds} rounds, alternating)")
    for d in (0.0, 0.25, 1.0, 4.0):
        x, y, z = displaced(d)
        cs, keep = raw_from_arrays(a, x, y, z)
        ctx.set_scene(sc)
        ctx.update_centers(0, x, y, z)
        other.set_scene_raw(cs, sc.camera.contents)
        t_refit, t_fresh, same = [], [], True
        for r in range(args.rounds):
            t_refit += frame_ms(ctx, args.frames)
            img_refit, rays_refit = hf.image(0).copy(), hf.rays(0)
            t_fresh += frame_ms(other, args.frames)
            same = same and rays_refit == hf.rays(0) and img_refit.tobytes() == hf.image(0).tobytes()
        mr, mf = statistics.median(t_refit), statistics.median(t_fresh)
        say(f"  displacement {d:4.2f} spacings: refitted {mr:7.3f} ms (min {min(t_refit):.3f}), fresh build {mf:7.3f} ms (min {min(t_fresh):.3f}), "
            f"refitted / fresh {mr / mf:5.2f}; pixels and rays {'equal' if same else 'DIFFER'}")
    ctx.close(), other.close()

    # ---- the large scene: the dropped flat slab ----
    say()
    sc2 = r1.create_large_scene(w, h)
    a2 = sc2.arrays()
    before, after = r1.Renderer(0), r1.Renderer(0)
    before.set_scene(sc2), after.set_scene(sc2)
    after.update_centers(0, a2["center_x"], a2["center_y"], a2["center_z"])
    say(f"(c) large scene ({sc2.count} spheres, flat y slab): a frame after an identity update against one before it ({args.frames} frames per timing, "
        f"{args.rounds} rounds, alternating)")
    t_b, t_a = [], []
    for r in range(args.rounds):
        t_b += frame_ms(before, args.frames)
        t_a += frame_ms(after, args.frames)
    say(f"  before (flat walk)    {spread(t_b)}")
    say(f"  after (generic loop)  {spread(t_a)}")
    say(f"  after / before: {statistics.median(t_a) / statistics.median(t_b):.3f}")
    before.close(), after.close()
    hf.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
