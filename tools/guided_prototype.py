#!/usr/bin/env python3
"""tools/guided_prototype.py — the sweep the defaults of the variance-guided filter rest on (measurement tool, CPU only,
no device), over the numpy restatement of the contract in tests/guided_cases.py, which tests/test_denoise_guided_host.py pins to the host form.

The filter is tests/denoise_cases.py's numpy_denoise (the §4.39 contract) with these changes and no others; V is a variance frame
(r1_render_moments_host), a_c the prepare step's albedo divisor, K3 = {1/4, 1/2, 1/4}:
  prepare      v = surf ? (V_r / (a_r * a_r) + V_g / (a_g * a_g)) + V_b / (a_b * a_b) : 0 — the variance of the demodulated value in dc's metric
  iteration    before the taps G = 0, K = 0; dy = -1 .. 1 outer, dx = -1 .. 1 inner, q = p + (dx, dy), one pixel apart at every step; a tap
               off the image or not surf is skipped; k = K3[dy + 1] * K3[dx + 1]; G = G + k * v_q; K = K + k; g = G / K
  colour term  sc2 = sigma_color * sigma_color in every iteration (no 2^-i); den = sc2 * g + variance_floor; xc = dc / den
  gains        T = T + (w * w) * v_q, the centre included with w = h; next_c = S_c / W; v_next = T / (W * W)
Measured as §4.39's table is: medium 160 x 100 and large 200 x 100, seed 4242, against 512 spp at seed 777, at 2, 4 and 16 spp; RMSE as a
share of the noisy frame's, 3 and 5 iterations; sigma_color in {1, 2, 4} x variance_floor in {1e-6, 1e-4}, normal_power_log2 6 and
sigma_depth 0.1 held; the unguided filter (r1_denoise_host, §4.39's options) beside it.
usage: tools/guided_prototype.py [--out FILE] [--scenes medium,large]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import rays1bench_amd as r1  # noqa: E402
from rays1bench_amd import binding  # noqa: E402
import denoise_cases as dc  # noqa: E402
import linear_cases as lc  # noqa: E402
from guided_cases import numpy_denoise_guided  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="medium,large")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sizes = {"medium": (160, 100), "large": (200, 100)}
    sweep = [(sc, fl) for sc in (1.0, 2.0, 4.0) for fl in (1e-6, 1e-4)]
    say("RMSE against 512 spp (seed 777) as a share of the noisy frame's (seed 4242); k = 6, sigma_depth 0.1, DEMODULATE; inputs from "
        "r1_render_moments_host and r1_render_features_host; unguided = r1_denoise_host with sigma_color 1")
    for name in args.scenes.split(","):
        w, h = sizes[name]
        sa = lc.scene_arrays(name, w, h)
        cs, cc = lc.cscene(sa), lc.ccamera(sa)
        ref, _ = binding.render_linear_host(cs, cc, r1.make_params(w, h, 512, 777))
        say()
        say(f"{name} {w}x{h}")
        say(f"{'spp':>4} {'iters':>5} {'noisy RMSE':>11} {'unguided':>9} " + " ".join(f"{f'sc {sc:g} fl {fl:g}':>15}" for sc, fl in sweep))
        for spp in (2, 4, 16):
            p = r1.make_params(w, h, spp, 4242)
            L, mom, _ = binding.render_moments_host(cs, cc, p)
            f = binding.render_features_host(cs, cc, p)
            noisy = dc.rmse(L, ref)
            for it in (3, 5):
                plain = dc.rmse(binding.denoise_host(L, f, dc.opt(iterations=it)), ref) / noisy
                row = [dc.rmse(numpy_denoise_guided(L, f, mom["var"], it, 6, sc, 0.1, fl), ref) / noisy for sc, fl in sweep]
                say(f"{spp:>4} {it:>5} {noisy:>11.5f} {plain:>9.4f} " + " ".join(f"{r:>15.4f}" for r in row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
