#!/usr/bin/env python3
"""tools/moments_bench.py — what a variance frame costs beside a linear frame (include/rays1.h; measurement tool).

One session, forms alternating after a warm-up round, median of N rounds with min .. max.  Per scene — the large scene at 1200 x 800 x 10
and config 5's scene (100 004 spheres) at 1920 x 1080 x 4 — and before anything is timed the variance frame's linear values are checked
against r1_render_linear's, bit for bit, and its variances against a float64 computation on the frame's own records:
  (a) a synchronous frame on the device clock (the library's HIP events: trace, close and the resolve launch): r1_render_moments against
      r1_render_linear.  The launches in front of the last are the same, so the difference is r1_resolve_moments_kernel against
      r1_resolve_linear_kernel: the second walk over the records and 16 more bytes stored per pixel;
  (b) one frame into device memory on the host clock, from the enqueue to the stream idle: r1_render_moments_device against
      r1_render_linear_device;
  (c) what a caller had to do before: r1_render_samples brings the records home, torch takes them back up and computes mean and variance
      (host clock, the whole of it).
No thresholds: the numbers are written down, nothing is tuned.
usage: tools/moments_bench.py [--rounds N] [--out FILE]   (FILE: profiles/rNN/moments.txt, NN the next free number)"""
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


def spread(v, scale=1e3):
    return f"{statistics.median(v) * scale:9.3f} ({min(v) * scale:.3f} .. {max(v) * scale:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    scenes = [("large scene", r1.create_large_scene, 1200, 800, 10),
              ("config 5's scene", lambda w, h: r1.create_grid_scene(w, h, 400, 250), 1920, 1080, 4)]
    say(f"variance frames beside linear frames; {args.rounds} rounds alternating after a warm-up round, median (min .. max), milliseconds")
    for title, make, w, h, spp in scenes:
        p = r1.make_params(w, h, spp, 10001)
        rend = r1.Renderer(0)
        rend.set_scene(make(w, h))
        lin, ref_rays, _ = rend.render_linear(p)
        got, mom, rays, _ = rend.render_moments(p)
        assert rays == ref_rays and got.tobytes() == lin.tobytes() and (mom["samples"] == spp).all() and (mom["var"] >= 0).all()
        _, _, samples = rend.render_samples(p)
        rec = samples.reshape(h, w, spp, 4)[..., :3].astype(np.float64)
        want = rec.var(axis=2, ddof=1) / spp
        err = np.abs(mom["var"] - want).max() / want.max()
        assert err < 1e-5, err  # (fp32 against fp64, relative to the frame's largest variance)
        del rec, want
        say()
        say(f"{title} {w}x{h}x{spp}: {ref_rays} rays per frame, {rend.launch_info()['compute_units']} CUs; bytes per pixel written by the closing launch: "
            f"12 (linear) against 28 (variance frame); records read: {16 * spp} against {32 * spp} (the second half from cache)")

        # ---- (a) synchronous, device clock -------------------------------------------------------------------------------------------
        forms = [("r1_render_linear", lambda: rend.render_linear(p)[1:]), ("r1_render_moments", lambda: rend.render_moments(p)[2:])]
        dev = {name: [] for name, _ in forms}
        for rnd in range(args.rounds + 1):
            for name, run in forms:
                got_rays, secs = run()
                assert got_rays == ref_rays
                if rnd:  # (round 0 warms up)
                    dev[name].append(secs)
        say("(a) one synchronous frame, device clock (trace + close + resolve launch)")
        for name, _ in forms:
            say(f"  {name:<40} {spread(dev[name])}")
        say(f"  the second walk: {(statistics.median(dev['r1_render_moments']) - statistics.median(dev['r1_render_linear'])) * 1e6:+.1f} us")

        # ---- (b) device form, host clock ---------------------------------------------------------------------------------------------
        out_f = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        out_m = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        st = torch.cuda.Stream()
        devs = [("r1_render_linear_device", lambda: rend.render_linear_device(p, out_f.data_ptr(), count.data_ptr(), st.cuda_stream)),
                ("r1_render_moments_device", lambda: rend.render_moments_device(p, out_f.data_ptr(), out_m.data_ptr(), count.data_ptr(), st.cuda_stream))]

        def records_to_torch():
            _, _, s = rend.render_samples(p)
            t = torch.from_numpy(s).to("cuda", non_blocking=False).view(h, w, spp, 4)[..., :3]
            mean, var = t.mean(dim=2), t.var(dim=2, unbiased=True) / spp
            torch.cuda.synchronize()
            return mean, var

        def alternate(runs):
            wall = {name: [] for name, _ in runs}
            for rnd in range(args.rounds + 1):
                for name, run in runs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    st.synchronize()
                    if rnd:
                        wall[name].append(time.perf_counter() - t0)
            return wall

        wall = alternate(devs)  # (the two device forms alone: the round trip of (c) between them would leave the next form a cold start)
        assert out_f.cpu().numpy().tobytes() == lin.tobytes() and out_m.cpu().numpy().tobytes() == mom.tobytes() and int(count.item()) == ref_rays
        say("(b) one frame into device memory, host clock from the enqueue to the stream idle")
        for name, _ in devs:
            say(f"  {name:<40} {spread(wall[name])}")
        say(f"  moments - linear: {(statistics.median(wall['r1_render_moments_device']) - statistics.median(wall['r1_render_linear_device'])) * 1e6:+.1f} us")
        trip = alternate([("r1_render_samples -> torch mean, var", records_to_torch)])
        say("(c) the records brought home and taken up again, host clock")
        say(f"  {'r1_render_samples -> torch mean, var':<40} {spread(trip['r1_render_samples -> torch mean, var'])}")
        rend.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
