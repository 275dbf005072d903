#!/usr/bin/env python3
"""tools/region_bench.py — what a region render costs beside the whole frame (include/rays1.h; measurement tool).

One session, runs alternating, medians; every window checked against the crop of the whole frame before anything is timed.
  (a) per scene — the large scene at 1200 x 800 x 10, config 5's scene (100 004 spheres) at 1920 x 1080 x 64 — centred square windows of
      32, 64, 128, 256 and 512 pixels and the full frame through r1_render_region, beside r1_render of the whole frame: device ms (HIP events
      of the library) and host ms, rays, rays/s, and the window's time as a share of the whole frame's beside its share of the frame's rays;
  (b) the edit loop on config 5's scene: one r1_update_spheres of one sphere's material + a region render of a 256 x 256 window around it,
      beside the same update + r1_render of the whole frame.
No thresholds: the numbers are written down, nothing is tuned.
usage: tools/region_bench.py [--rounds N] [--out FILE]   (FILE: profiles/rNN/region.txt, NN the next free number)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before librays1: one HIP runtime per process)
import rays1bench_amd as r1  # noqa: E402


def med(v):
    return statistics.median(v)


def centred(w, h, n):
    return ((w - n) // 2, (h - n) // 2, n, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    seed = 10001
    rend = r1.Renderer(0)
    scenes = [("the large scene", lambda w, h: r1.create_large_scene(w, h), 1200, 800, 10), ("config 5's scene", lambda w, h: r1.create_grid_scene(w, h, 400, 250), 1920, 1080, 64)]
    say(f"region renders beside the whole frame; {args.rounds} rounds alternating after one warm-up round, medians; seed {seed}, 32 x 32 tiles, R1_VARIANT_DEFAULT")
    last = None
    for title, make, w, h, spp in scenes:
        sc = make(w, h)
        rend.set_scene(sc)
        p = r1.make_params(w, h, spp, seed)
        ref_img, ref_rays, _ = rend.render(p)
        wins = [centred(w, h, n) for n in (32, 64, 128, 256, 512)] + [(0, 0, w, h)]
        rays_of = {}
        for win in wins:  # checked before anything is timed
            img, rays, _ = rend.render_region(p, win)
            x0, y0, ww, wh = win
            assert img.tobytes() == np.ascontiguousarray(ref_img[y0:y0 + wh, x0:x0 + ww]).tobytes(), (title, win)
            rays_of[win] = rays
        assert rays_of[wins[-1]] == ref_rays
        frame = np.zeros((h, w, 3), np.uint8)
        outs = {win: np.zeros((win[3], win[2], 3), np.uint8) for win in wins}
        forms = [("r1_render, whole frame", None)] + [(f"region {win[2]}x{win[3]} at {win[0]},{win[1]}", win) for win in wins]
        res = {name: {"wall": [], "dev": []} for name, _ in forms}
        for rnd in range(args.rounds + 1):
            for name, win in forms:
                t0 = time.perf_counter()
                if win is None:
                    got, dev = rend.render_into(p, frame)
                else:
                    _, got, dev = rend.render_region(p, win, out=outs[win])
                wall = time.perf_counter() - t0
                assert got == (ref_rays if win is None else rays_of[win]), name
                if rnd:  # (round 0 warms up)
                    res[name]["wall"].append(wall), res[name]["dev"].append(dev)
        li = rend.launch_info()
        say()
        say(f"(a) {title}, {w}x{h}x{spp}: {li['spheres_active']} hittable spheres, {ref_rays} rays per frame, {li['compute_units']} CUs")
        say(f"{'form':<32} {'device ms':>10} {'host ms':>9} {'rays':>13} {'device Grays/s':>15} {'time share':>11} {'ray share':>10}")
        d0 = med(res[forms[0][0]]["dev"])
        for name, win in forms:
            d, t = med(res[name]["dev"]), med(res[name]["wall"])
            rays = ref_rays if win is None else rays_of[win]
            say(f"{name:<32} {d * 1e3:>10.3f} {t * 1e3:>9.3f} {rays:>13d} {rays / d / 1e9:>15.2f} {d / d0:>11.4f} {rays / ref_rays:>10.4f}")
        last = (sc, p, w, h, ref_img)

    # ---- (b) the edit loop: recolour one sphere, look at it again -----------------------------------------------------------------------------
    sc, p, w, h, ref_img = last
    a = sc.arrays()
    act = np.nonzero(a["inv_radius"] != 0)[0]
    i = int(act[len(act) // 2])  # one lattice sphere
    win = centred(w, h, 256)
    mats = []
    for k in range(2):  # two materials taken in turn: a diffuse red, and the sphere's own
        mt, ar, ag, ab, mp = (a[f][i:i + 1].copy() for f in ("mat_type", "albedo_r", "albedo_g", "albedo_b", "mat_param"))
        if k == 0:
            mt[:], ar[:], ag[:], ab[:], mp[:] = 0, 0.9, 0.1, 0.1, 0.0
        mats.append((mt, ar, ag, ab, mp))
    frame = np.zeros((h, w, 3), np.uint8)
    out = np.zeros((win[3], win[2], 3), np.uint8)
    t_region, t_frame, t_update = [], [], []
    for rnd in range(args.rounds + 1):
        m = mats[rnd % 2]
        t0 = time.perf_counter()
        rend.update_spheres(i, materials=m)
        rend.render_region(p, win, out=out)
        t1 = time.perf_counter()
        rend.update_spheres(i, materials=m)
        rend.render_into(p, frame)
        t2 = time.perf_counter()
        rend.update_spheres(i, materials=m)
        rend.sync()
        t3 = time.perf_counter()
        x0, y0, ww, wh = win
        assert out.tobytes() == np.ascontiguousarray(frame[y0:y0 + wh, x0:x0 + ww]).tobytes()
        if rnd:
            t_region.append(t1 - t0), t_frame.append(t2 - t1), t_update.append(t3 - t2)
    say()
    say(f"(b) the edit loop on config 5's scene, {w}x{h}x{p.spp} (host clock): r1_update_spheres of sphere {i}'s material, then a look at it")
    say(f"  update + r1_render_region {win[2]}x{win[3]}   {med(t_region) * 1e3:9.3f} ms")
    say(f"  update + r1_render, whole frame     {med(t_frame) * 1e3:9.3f} ms   ({med(t_frame) / med(t_region):.1f} x)")
    say(f"  the update alone (+ r1_sync)        {med(t_update) * 1e3:9.3f} ms")
    rend.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
