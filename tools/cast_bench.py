#!/usr/bin/env python3
"""tools/cast_bench.py — throughput of the ray queries (r1_cast_rays_device); measurement tool, needs a GPU and torch,
reads no file outside the repository.

The device form, rays resident on the device: after a warm-up, a host clock around enough enqueued casts to fill at least 0.5 s, ending
in r1_sync.  Grays/s, and beside each rate the algorithmic bytes it moves (64 per ray for CLOSEST: 32 in, 32 out; 33 for ANY) as a share
of 8 TB/s, so that the bound that applies can be named.

Workloads, large scene: 9.6 M primary rays (1200 x 800 pixels, 10 seeded jitters each, in pixel order), the same rays shuffled, and 9.6 M
scatter rays built from the first set's hits (origin = hit point, direction = normal + a vector of the unit ball); tree and grid, CLOSEST
and ANY.  Config 5 (100 004 spheres): primary rays at 1920 x 1080.

--ab N: what decides the kernel form.  N pairs of fresh child processes load lib/librays1_tuning.so (`make tuning`), alternating
R1_CAST_PLAIN=0 (the persistent form: LDS node table, walks carried over, lanes refilled) and =1 (the plain form: grid-stride, one
complete walk per ray from the table in global memory), each on the shuffled and the scatter workload of the tree.
usage: tools/cast_bench.py [--out FILE] [--ab N] [--skip-config5] [--min-seconds S]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12


def unit_ball(rng, n):
    out = np.empty((0, 3), np.float32)
    while out.shape[0] < n:
        v = rng.uniform(-1.0, 1.0, (n // 2 + 1024, 3)).astype(np.float32)
        out = np.concatenate([out, v[(v * v).sum(1) < 1.0]])
    return out[:n]


def primary_rays(cam, w, h, jitters, seed):
    """primary rays of `cam` (22 floats) in pixel order, `jitters` per pixel, lens radius 0"""
    rng = np.random.default_rng(seed)
    n = w * h * jitters
    pix = np.repeat(np.arange(w * h), jitters)
    u = ((pix % w).astype(np.float32) + rng.random(n, np.float32)) / np.float32(w)
    v = ((pix // w).astype(np.float32) + rng.random(n, np.float32)) / np.float32(h)
    cam = cam.astype(np.float32)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = cam[0:3]
    rays[:, 3] = np.finfo(np.float32).max
    rays[:, 4:7] = cam[3:6][None, :] + u[:, None] * cam[6:9][None, :] + v[:, None] * cam[9:12][None, :] - cam[0:3][None, :]
    return rays


class Bench:
    def __init__(self, min_seconds):
        import torch
        import rays1bench_amd as r1
        from rays1bench_amd import binding
        self.torch, self.r1, self.binding = torch, r1, binding
        self.rend = r1.Renderer(0)
        self.min_seconds = min_seconds

    def upload(self, rays):
        return self.torch.from_numpy(np.ascontiguousarray(rays)).cuda()

    def hits_of(self, d_rays):
        n = d_rays.shape[0]
        out = self.torch.zeros((n, 8), dtype=self.torch.float32, device="cuda")
        self.rend.cast_rays_device(d_rays.data_ptr(), n, out.data_ptr(), 0, 0)
        self.rend.sync()
        return out.cpu().numpy().view(self.binding.HIT_DTYPE).reshape(-1)

    def rate(self, d_rays, mode, variant):
        """Grays/s of the device form over casts enqueued back to back"""
        n = d_rays.shape[0]
        out = self.torch.zeros((n, 8) if mode == 0 else (n,), dtype=self.torch.float32 if mode == 0 else self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()

        def run(reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                self.rend.cast_rays_device(d_rays.data_ptr(), n, out.data_ptr(), mode, variant)
            self.rend.sync()
            return time.perf_counter() - t0

        run(2)  # warm-up: occupancy query, the grid's build, the first launch
        one = run(2) / 2
        reps = max(3, int(self.min_seconds * 1.2 / one) + 1)
        t = run(reps)
        return n * reps / t / 1e9, reps, t

    def scatter_from(self, rays, hits, seed):
        rng = np.random.default_rng(seed)
        hit = np.nonzero(hits["index"] >= 0)[0]
        pick = rng.choice(hit, rays.shape[0])
        out = np.zeros_like(rays)
        out[:, 0:3] = hits["p"][pick]
        out[:, 3] = np.finfo(np.float32).max
        out[:, 4:7] = hits["n"][pick] + unit_ball(rng, rays.shape[0])
        return out


def fmt(rate, mode):
    per = 64 if mode == 0 else 33
    return f"{rate:7.3f} Grays/s  {rate * 1e9 * per / 1e12:6.3f} TB/s = {rate * 1e9 * per / HBM * 100:5.1f} % of 8 TB/s"


def large_workloads(b):
    sc = b.r1.create_large_scene(1200, 800)
    b.rend.set_scene(sc)
    rays = primary_rays(sc.camera_array(), 1200, 800, 10, 101)
    d_primary = b.upload(rays)
    hits = b.hits_of(d_primary)
    shuffled = rays[np.random.default_rng(102).permutation(rays.shape[0])]
    scatter = b.scatter_from(rays, hits, 103)
    return sc, {"primary": d_primary, "shuffled": b.upload(shuffled), "scatter": b.upload(scatter)}, float((hits["index"] >= 0).mean())


def child(args):
    """one process of --ab: the tree on the shuffled and scatter workloads, one JSON line"""
    from rays1bench_amd import binding
    binding.set_lib_path(os.path.join(ROOT, "rays1bench_amd", "lib", "librays1_tuning.so"))
    b = Bench(args.min_seconds)
    _, loads, _ = large_workloads(b)
    res = {}
    for name in ("shuffled", "scatter"):
        for mode in (0, 1):
            res[f"{name}/{'CLOSEST' if mode == 0 else 'ANY'}"] = b.rate(loads[name], mode, b.binding.VARIANT_BVH)[0]
    print("CAST_AB " + json.dumps(res), flush=True)
    b.rend.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--ab", type=int, default=0, help="pairs of persistent / plain runs in the tuning library")
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--skip-product", action="store_true", help="only the --ab comparison")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not args.skip_product:
        b = Bench(args.min_seconds)
        V = {"tree": b.binding.VARIANT_BVH, "grid": b.binding.VARIANT_GRID}
        sc, loads, frac = large_workloads(b)
        say(f"large scene ({int((sc.arrays()['inv_radius'] != 0).sum())} spheres), 9.6 M rays per cast, {frac * 100:.1f} % of the primary rays hit; device form, "
            f"host clock over >= {args.min_seconds} s of enqueued casts ending in r1_sync")
        for name, d_rays in loads.items():
            for sname, variant in V.items():
                for mode in (0, 1):
                    rate, reps, t = b.rate(d_rays, mode, variant)
                    say(f"  {name:<9} {sname:<5} {'CLOSEST' if mode == 0 else 'ANY':<8} {fmt(rate, mode)}   ({reps} casts in {t:.3f} s)")
        sc.close()
        if not args.skip_config5:
            w, h = 1920, 1080
            sc = b.r1.create_grid_scene(w, h, 400, 250)
            b.rend.set_scene(sc)
            d_rays = b.upload(primary_rays(sc.camera_array(), w, h, 1, 104))
            say(f"config 5 ({int((sc.arrays()['inv_radius'] != 0).sum())} spheres), {w * h} primary rays per cast")
            for sname, variant in V.items():
                for mode in (0, 1):
                    rate, reps, t = b.rate(d_rays, mode, variant)
                    say(f"  primary   {sname:<5} {'CLOSEST' if mode == 0 else 'ANY':<8} {fmt(rate, mode)}   ({reps} casts in {t:.3f} s)")
            sc.close()
        b.rend.close()
    if args.ab:
        say()
        say(f"kernel form, tree, lib/librays1_tuning.so, {args.ab} alternating pairs of fresh processes (Grays/s): persistent = LDS node table + carried walks + refill; "
            "plain = grid-stride, complete walks from the global table")
        runs = {"persistent": [], "plain": []}
        for _ in range(args.ab):
            for form, knob in (("persistent", "0"), ("plain", "1")):
                env = dict(os.environ, R1_CAST_PLAIN=knob)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--min-seconds", str(args.min_seconds)], env=env, capture_output=True, text=True,
                                   timeout=600)
                got = [ln for ln in p.stdout.splitlines() if ln.startswith("CAST_AB ")]
                if p.returncode != 0 or not got:
                    say(f"  {form}: child failed ({p.returncode}): {p.stderr[-400:]}")
                    return 1  # (nothing more is started on the GPU after a failure)
                runs[form].append(json.loads(got[0][8:]))
        for key in runs["persistent"][0]:
            a = [r[key] for r in runs["persistent"]]
            c = [r[key] for r in runs["plain"]]
            say(f"  {key:<18} persistent {' '.join(f'{x:7.3f}' for x in a)}   plain {' '.join(f'{x:7.3f}' for x in c)}   persistent / plain = {np.mean(a) / np.mean(c):.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
