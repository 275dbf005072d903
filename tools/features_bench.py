#!/usr/bin/env python3
"""tools/features_bench.py — what a feature frame costs (include/rays1.h; measurement tool).

One session on one device; the forms alternate, one warm-up round each, host clock from the first enqueue to the stream being idle; medians
and the run-to-run spread (min .. max).  Per scene — the large scene at 1200 x 800 x 10, config 5's scene (100 004 spheres) at
1920 x 1080 x 4 — and per structure (box tree, uniform grid), everything in device memory:
  (a) r1_render_features_device;
  (b) the composition the library offered before it: r1_camera_rays_device + r1_cast_rays_device (32 + 16 bytes written and 32 read per
      sample, 32 written per hit record), then a gather of the albedo table and a per-pixel sum in torch — the baseline.  Its sums are
      torch's, so it is compared with (a) to a tolerance, not to the bit;
  (c) for scale, r1_render_linear_device of the same frame: the path-traced frame the guide images go with.
(a) is checked against (b) before anything is timed.  No thresholds: the numbers are written down.
usage: tools/features_bench.py [--rounds N] [--out FILE] [--lib LIBRARY] [--only-features]
  --lib            another build of the library (librays1_tuning.so reads R1_FEATURE_CLAIM: pixels per claim)
  --only-features  form (a) alone (for comparing builds and claims)"""
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


def composition(rend, p, variant, tabs, bufs, st):
    """(b): rays and seeds of every sample, their hit records, then albedo / normal / depth / hits per pixel in torch; returns (h * w, 8) floats"""
    n = p.width * p.height * p.spp
    rays, seeds, hits = bufs
    rend.camera_rays_device(p, 0, n, rays.data_ptr(), seeds.data_ptr(), stream=st.cuda_stream)
    rend.cast_rays_device(rays.data_ptr(), n, hits.data_ptr(), variant=variant, stream=st.cuda_stream)
    with torch.cuda.stream(st):
        idx = hits[:, 1].view(torch.int32).long()
        hit = idx >= 0
        d = rays[:, 4:7]
        dy = d[:, 1] / d.norm(dim=1)
        t = 0.5 * (dy + 1.0)
        sky = (1.0 - t)[:, None] + t[:, None] * tabs["sky"]
        albedo = torch.where(hit[:, None], tabs["albedo"][idx.clamp(min=0)], sky)
        rest = torch.where(hit[:, None], torch.cat([hits[:, 0:1], hits[:, 5:8], torch.ones_like(hits[:, 0:1])], dim=1), torch.zeros_like(hits[:, 0:5]))
        out = torch.cat([albedo, rest], dim=1).view(p.height * p.width, p.spp, 8).sum(dim=1)
        out[:, :7] *= 1.0 / p.spp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--only-features", action="store_true")
    args = ap.parse_args()
    if args.lib:
        binding.set_lib_path(os.path.abspath(args.lib))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    seed = 10001
    rend = r1.Renderer(0)
    st = torch.cuda.Stream()
    scenes = [("the large scene", lambda w, h: r1.create_large_scene(w, h), 1200, 800, 10),
              ("config 5's scene", lambda w, h: r1.create_grid_scene(w, h, 400, 250), 1920, 1080, 4)]
    say(f"feature frames; {args.rounds} rounds alternating after one warm-up round, host clock from enqueue to stream idle, median (min .. max) ms; seed {seed}"
        + (f"; library {os.path.basename(args.lib)}, R1_FEATURE_CLAIM={os.environ.get('R1_FEATURE_CLAIM', '-')}" if args.lib else ""))
    for title, make, w, h, spp in scenes:
        sc = make(w, h)
        rend.set_scene(sc)
        a = sc.arrays()
        n = w * h * spp
        glass = torch.from_numpy((a["mat_type"] == binding.MAT_DIELECTRIC)).cuda()
        tabs = {"albedo": torch.where(glass[:, None], torch.ones(1, 3, device="cuda"),
                                      torch.from_numpy(np.stack([a["albedo_r"], a["albedo_g"], a["albedo_b"]], axis=1).astype(np.float32)).cuda()),
                "sky": torch.tensor([0.5, 0.7, 1.0], device="cuda")}
        feat = torch.zeros((h * w, 8), dtype=torch.float32, device="cuda")
        lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        bufs = None if args.only_features else (torch.zeros((n, 8), dtype=torch.float32, device="cuda"), torch.zeros((n, 4), dtype=torch.int32, device="cuda"),
                                                torch.zeros((n, 8), dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        say()
        say(f"{title}, {w}x{h}x{spp}: {int((a['inv_radius'] != 0).sum())} hittable spheres, {w * h} pixels, {n} samples")
        for vname, variant in (("box tree", binding.VARIANT_BVH), ("uniform grid", binding.VARIANT_GRID)):
            p = r1.make_params(w, h, spp, seed, variant=variant)
            forms = [("(a) r1_render_features_device", lambda: rend.render_features_device(p, feat.data_ptr(), stream_ptr=st.cuda_stream))]
            if not args.only_features:
                forms.append(("(b) camera rays + cast + torch sums", lambda: composition(rend, p, variant, tabs, bufs, st)))
                forms.append(("(c) r1_render_linear_device", lambda: rend.render_linear_device(p, lin.data_ptr(), cnt.data_ptr(), stream_ptr=st.cuda_stream)))
                # (a) against (b) before anything is timed: hits exactly, the sums to torch's summation order
                forms[0][1]()
                other = forms[1][1]()
                st.synchronize()
                assert torch.equal(feat[:, 7].view(torch.int32), other[:, 7].to(torch.int32)), (title, vname, "hits")
                assert torch.allclose(feat[:, :3], other[:, :3], rtol=1e-4, atol=1e-5) and torch.allclose(feat[:, 3], other[:, 3], rtol=1e-4), (title, vname)
                assert torch.allclose(feat[:, 4:7], other[:, 4:7], rtol=1e-4, atol=1e-5), (title, vname, "normals")
            res = {name: [] for name, _ in forms}
            for rnd in range(args.rounds + 1):
                for name, run in forms:
                    st.synchronize()
                    t0 = time.perf_counter()
                    run()
                    st.synchronize()
                    if rnd:  # (round 0 warms up)
                        res[name].append(time.perf_counter() - t0)
            base = statistics.median(res[forms[1][0]]) if len(forms) > 1 else None
            for name, _ in forms:
                v = res[name]
                m = statistics.median(v)
                say(f"  {vname:<13} {name:<38} {m * 1e3:9.3f} ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}) ms  {n / m / 1e9:7.3f} G samples/s"
                    + (f"  {base / m:6.2f} x (b)" if base else ""))
    rend.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
