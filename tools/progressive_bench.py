#!/usr/bin/env python3
"""tools/progressive_bench.py — progressive passes (r1_render_pass) against one r1_render of the same frame (measurement tool).

One context, one session, alternating: the large scene at 1200 x 800, one r1_render at 250 spp against the same 250 samples in passes of
10, 25, 50 and 125, every form checked for the same pixels and ray count; rays/s on the host clock (call to call, pixels on the host) and on
the device (HIP events of the library, summed over the passes); the accumulate launch's time (r1_last_timing: total - trace) and its rate
over its compulsory bytes (the pass's records + 2 x 16 B of accumulator per pixel + 3 B of preview per pixel; the first pass reads no
accumulator).  Then one frame beyond the one-launch ceiling: 1920 x 1080 x 2048 in 8 passes.
usage: tools/progressive_bench.py [--rounds N] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rays1bench_amd as r1  # noqa: E402
from rays1bench_amd import binding  # noqa: E402


def one_render(rend, p):
    t0 = time.perf_counter()
    img, rays, _ = rend.render(p)
    wall = time.perf_counter() - t0
    trace_ms, total_ms = rend.last_timing()
    return img, rays, wall, total_ms * 1e-3, [total_ms - trace_ms]


def in_passes(rend, p, size):
    """p.spp samples in passes of `size` (the last one shorter if need be); pixels asked for on the last pass only."""
    first, dev, tails = 0, 0.0, []
    img, rays = None, 0
    t0 = time.perf_counter()
    while first < p.spp:
        n = min(size, p.spp - first)
        q = r1.make_params(p.width, p.height, n, p.seed, p.max_bounces, p.tile_w, p.tile_h, variant=p.variant)
        img, rays = rend.render_pass(q, first, image=first + n == p.spp)
        trace_ms, total_ms = rend.last_timing()
        dev += total_ms * 1e-3
        tails.append(total_ms - trace_ms)
        first += n
    return img, rays, time.perf_counter() - t0, dev, tails


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rend = r1.Renderer(0)
    w, h, spp = 1200, 800, 250
    rend.set_scene(r1.create_large_scene(w, h))
    p = r1.make_params(w, h, spp, 10001)
    forms = [("r1_render 250", None)] + [(f"passes of {s}", s) for s in (10, 25, 50, 125)]
    run = lambda s: one_render(rend, p) if s is None else in_passes(rend, p, s)
    ref_img, ref_rays = None, None
    for _, s in forms:  # warm-up: workspaces, occupancy queries, the first launch of every kernel
        img, rays = run(s)[:2]
        ref_img, ref_rays = (img, rays) if ref_img is None else (ref_img, ref_rays)
        assert rays == ref_rays and img.tobytes() == ref_img.tobytes(), s
    res = {name: {"wall": [], "dev": [], "tail": []} for name, _ in forms}
    for _ in range(args.rounds):
        for name, s in forms:
            img, rays, wall, dev, tails = run(s)
            assert rays == ref_rays and img.tobytes() == ref_img.tobytes(), name
            res[name]["wall"].append(wall)
            res[name]["dev"].append(dev)
            res[name]["tail"].append(tails)
    li = rend.launch_info()
    say(f"progressive passes, large scene {w}x{h}x{spp}, seed 10001, {ref_rays} rays per frame, kernel {li['kernel']} "
        f"(DEFAULT), {li['compute_units']} CUs; {args.rounds} rounds alternating, medians; every form bit-identical to r1_render")
    say(f"{'form':<16} {'launches':>8} {'host ms':>9} {'host Grays/s':>13} {'vs render':>9} {'device ms':>10} {'device Grays/s':>15} {'vs render':>9}"
        f" {'host min ms':>12} {'host - device ms, every round':>30}")
    base_w = statistics.median(res[forms[0][0]]["wall"])
    base_d = statistics.median(res[forms[0][0]]["dev"])
    for name, s in forms:
        mw, md = statistics.median(res[name]["wall"]), statistics.median(res[name]["dev"])
        n = 1 if s is None else -(-spp // s)
        gaps = " ".join(f"{(a - b) * 1e3:.2f}" for a, b in zip(res[name]["wall"], res[name]["dev"]))
        say(f"{name:<16} {n:>8} {mw * 1e3:>9.2f} {ref_rays / mw / 1e9:>13.2f} {base_w / mw * 100:>8.1f}% {md * 1e3:>10.2f} "
            f"{ref_rays / md / 1e9:>15.2f} {base_d / md * 100:>8.1f}% {min(res[name]['wall']) * 1e3:>12.2f}   {gaps}")
    say()
    say("after the trace kernel (r1_last_timing total - trace): the resolve launch of r1_render, the accumulate launch of a pass")
    px = w * h
    for name, s in forms:
        tails = [t for rnd in res[name]["tail"] for t in rnd]
        if s is None:
            say(f"  resolve   (250 spp): median {statistics.median(tails) * 1e3:7.1f} us, {px * spp * 16 / 1e9:.2f} GB of records + 3 B/pixel "
                f"-> {(px * spp * 16 + 3 * px) / (statistics.median(tails) * 1e-3) / 1e12:.2f} TB/s")
            continue
        later = [t for rnd in res[name]["tail"] for t in rnd[1:]]  # (passes after the first read the accumulator too)
        t = statistics.median(later)
        compulsory = px * s * 16 + 2 * 16 * px + 3 * px
        say(f"  accumulate ({s:>3} spp): median {t * 1e3:7.1f} us over {compulsory / 1e9:.3f} GB compulsory -> {compulsory / (t * 1e-3) / 1e12:.2f} TB/s "
            f"(first pass: {statistics.median([rnd[0] for rnd in res[name]['tail']]) * 1e3:.1f} us)")
    say()
    # beyond the one-launch ceiling: 1920 x 1080 x 2048 = 4.2 G samples (r1_render stops at 2^31 samples, 1028 spp with 32 x 32 tiles)
    W, H, S, K = 1920, 1080, 2048, 8
    rend.set_scene(r1.create_large_scene(W, H))
    big = r1.make_params(W, H, S, 10001)
    try:
        rend.render(big)
        say("r1_render 1920x1080x2048: accepted (unexpected)")
    except binding.R1Error as e:
        say(f"r1_render 1920x1080x2048: refused ({e.code}: R1_ELIMIT expected)")
    img, rays, wall, dev, tails = in_passes(rend, big, S // K)
    say(f"1920x1080x2048 in {K} passes of {S // K}: {rays} rays, host {wall:.3f} s ({rays / wall / 1e9:.2f} Grays/s), device {dev:.3f} s "
        f"({rays / dev / 1e9:.2f} Grays/s), accumulate launches {statistics.median(tails[1:]) * 1e3:.1f} us median, image mean {img.mean():.3f}")
    rend.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
