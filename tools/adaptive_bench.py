#!/usr/bin/env python3
"""tools/adaptive_bench.py — adaptive sampling (r1_render_adaptive) against what the library had before it (measurement
tool; needs a GPU, reads no file outside the repository).

One context, one session, the forms alternating over the rounds:
  (a) what the feature costs with nothing to gain: the large scene at 1200 x 800, cap 250, schedules (25, 25) and (50, 50), rule off
      (max_delta -1: every tile runs to the cap) against r1_render_pass driven with the same pass sizes, and one r1_render at the cap;
  (b) what it saves: the same frame and schedules at 255 / 128, 32 / 512 and 48 / 768, and the 100 004-sphere lattice of BASELINE
      config 5 at 1920 x 1080, cap 64, (16, 16): samples and rays traced as shares of the full frame, device and host time as shares of
      the rule-off run and of one r1_render at the cap, the image's mean and maximum byte difference from that r1_render, and the tiles
      every pass carried.
Device clock: the library's events (r1_timing_begin / r1_timing_end) summed over the passes of a call.  Host clock: around the call.
usage: tools/adaptive_bench.py [--rounds N] [--out FILE] [--skip-config5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--skip-config5", action="store_true")
    args = ap.parse_args()
    import rays1bench_amd as r1
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rend = r1.Renderer(0)

    def timed(n_launches, call):
        """(device ms summed over the call's launches, host ms, the call's result)"""
        rend.timing_begin(max(1, n_launches))
        t0 = time.perf_counter()
        out = call()
        host = (time.perf_counter() - t0) * 1e3
        _, dev, _ = rend.timing_end()
        return dev, host, out

    def passes(p, sched):
        first, out = 0, None
        for k, n in enumerate(sched):
            q = r1.make_params(p.width, p.height, n - first, p.seed, p.max_bounces, p.tile_w, p.tile_h, variant=p.variant)
            out = rend.render_pass(q, first, image=k == len(sched) - 1)
            first = n
        return out

    def study(label, scene, p, schedules, settings):
        rend.set_scene(scene)
        w, h, cap = p.width, p.height, p.spp
        say()
        say(f"{label}: {w}x{h}, cap {cap}, seed {p.seed}, 32 x 32 tiles, {args.rounds} rounds alternating; ms = median (every round)")
        forms = [("r1_render at the cap", None, None, lambda: timed(1, lambda: rend.render(p)))]
        for a, b in schedules:
            sched = r1.adaptive_schedule(p, a, b)
            forms.append((f"r1_render_pass x {len(sched)}", (a, b), None, lambda sched=sched: timed(len(sched), lambda: passes(p, sched))))
            forms.append((f"adaptive, rule off", (a, b), (-1, 0), lambda a=a, b=b, n=len(sched): timed(n, lambda: rend.render_adaptive(p, a, b, -1, 0))))
            for md, mq in settings:
                forms.append((f"adaptive {md} / {mq}", (a, b), (md, mq),
                              lambda a=a, b=b, md=md, mq=mq, n=len(sched): timed(n, lambda: rend.render_adaptive(p, a, b, md, mq))))
        res = [[] for _ in forms]
        for _, _, _, run in forms:  # warm-up: workspaces, occupancy queries, the first launch of every kernel
            run()
        for _ in range(args.rounds):
            for i, (_, _, _, run) in enumerate(forms):
                res[i].append(run())
        full_img, full_rays = res[0][0][2][0], res[0][0][2][1]
        dev0, host0 = statistics.median(x[0] for x in res[0]), statistics.median(x[1] for x in res[0])
        say(f"  {'form':<24} {'schedule':>9} {'device ms':>10} {'host ms':>9}   {'device, every round':<26} {'samples':>8} {'rays':>7} {'dev/off':>8} {'host/off':>8} "
            f"{'dev/render':>10} {'saved t/rays':>12} {'mean |d|':>8} {'max |d|':>7}  tiles per pass")
        off = {}
        for i, (name, sch, rule, _) in enumerate(forms):
            dev, host = statistics.median(x[0] for x in res[i]), statistics.median(x[1] for x in res[i])
            rounds = " ".join(f"{x[0]:.3f}" for x in res[i])
            out = res[i][0][2]
            img, rays = out[0], out[1]
            diff = np.abs(img.astype(np.int32) - full_img.astype(np.int32))
            sch_s = f"{sch[0]}+{sch[1]}.." if sch else "-"
            if rule is None:
                assert rays == full_rays and diff.max() == 0, name
                if sch:
                    off[("pass", sch)] = (dev, host, [x[0] for x in res[i]])
                say(f"  {name:<24} {sch_s:>9} {dev:>10.3f} {host:>9.3f}   {rounds:<26} {1.0:>8.4f} {1.0:>7.4f} {'':>8} {'':>8} {dev / dev0:>10.4f}")
                continue
            tiles, result = out[2], out[3]
            if rule[0] < 0:
                assert rays == full_rays and diff.max() == 0, name
                off[sch] = (dev, host)
            sched = r1.adaptive_schedule(p, sch[0], sch[1])
            per_pass = " ".join(str(int((tiles["spp"] >= n).sum())) for n in sched[:result["passes"]])
            s_share, r_share = result["samples"] / (w * h * cap), rays / full_rays
            d_off, h_off = off[sch]
            saved = (1 - dev / d_off) / (1 - r_share) if r_share < 1 else float("nan")
            say(f"  {name:<24} {sch_s:>9} {dev:>10.3f} {host:>9.3f}   {rounds:<26} {s_share:>8.4f} {r_share:>7.4f} {dev / d_off:>8.4f} {host / h_off:>8.4f} "
                f"{dev / dev0:>10.4f} {saved:>12.3f} {diff.mean():>8.3f} {int(diff.max()):>7d}  {per_pass}")
        for sch in schedules:
            if ("pass", sch) in off:
                pd, ph, prounds = off[("pass", sch)]
                od, oh = off[sch]
                say(f"  cost with nothing to gain, {sch[0]}+{sch[1]}..: rule off / r1_render_pass = {od / pd:.4f} device, {oh / ph:.4f} host; "
                    f"r1_render_pass itself ranges {min(prounds):.3f} .. {max(prounds):.3f} ms over the rounds ({(max(prounds) / min(prounds) - 1) * 100:.1f} %)")

    settings = [(255, 128), (32, 512), (48, 768)]
    w, h = 1200, 800
    sc = r1.create_large_scene(w, h)
    study("large scene (484 spheres)", sc, r1.make_params(w, h, 250, 10001), [(25, 25), (50, 50)], settings)
    sc.close()
    if not args.skip_config5:
        w, h = 1920, 1080
        sc = r1.create_grid_scene(w, h, 400, 250)
        study("config 5 (100 004 spheres, 400 x 250 lattice)", sc, r1.make_params(w, h, 64, 10001), [(16, 16)], settings)
        sc.close()
    rend.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
