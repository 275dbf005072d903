#!/usr/bin/env python3
"""tools/denoise_bench.py — what a denoised frame costs (include/rays1.h; measurement tool).

One session on one device; the forms alternate, one warm-up round each, host clock from the first enqueue to the stream being idle; medians
and the run-to-run spread (min .. max).  The large scene at 1200 x 800 and 1920 x 1080, 4 spp, with 3 and 5 iterations (normal_power_log2 6,
sigma_color 1, sigma_depth 0.1, demodulated), everything in device memory:
  (a) r1_denoise_device;
  (b) the same contract composed from torch slices on the device: 25 shifted views per pass of padded copies, every line of the contract
      one torch operation — the baseline a user would write.  Its output is compared with (a): the largest difference and the share of
      values equal to the bit are reported (torch's division and its fused kernels need not round as the contract does);
  (c) for scale, r1_render_linear_device + r1_render_features_device of the same frame: what the filter's inputs cost.
Then the passes one by one: (a) with 1 .. 6 iterations, the time of pass i taken as the difference of the medians of i + 1 and i iterations
(the pass that writes `out` stores 12 bytes a pixel instead of 16: the difference is that of the work added), and the bytes it must move —
48 a pixel: two records read once, one written — over that time.  With --lib librays1_tuning.so the environment variable
R1_DENOISE_STAGE_MAX_STEP says up to which step a pass stages its taps in LDS (0: never; the library's default is r1_denoise.h's): one run
per value compares the two forms step by step.  No thresholds: the numbers are written down.
usage: tools/denoise_bench.py [--rounds N] [--out FILE] [--lib LIBRARY] [--only-denoise]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before librays1: one HIP runtime per process)
import rays1bench_amd as r1  # noqa: E402
from rays1bench_amd import binding  # noqa: E402

H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def composition(L, f, o):
    """(b): the contract in torch on the current stream.  L (h, w, 3), f (h, w, 8) float32 with the hit count's bits in word 7."""
    h, w = L.shape[:2]
    hits = f[..., 7].view(torch.int32)
    surf = hits > 0
    albedo = f[..., 0:3]
    a = torch.where(albedo < 1 / 256, torch.full_like(albedo, 1 / 256), albedo) if o.flags & binding.DENOISE_DEMODULATE else torch.ones_like(albedo)
    cur = L / a
    n = f[..., 4:7]
    ln = torch.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    nh = torch.where((ln > 0)[..., None], n / ln[..., None], torch.zeros_like(n))
    m = torch.where(surf, f[..., 3] / hits.clamp(min=1).float(), torch.zeros_like(ln))
    pad2 = torch.nn.functional.pad
    for i in range(o.iterations):
        step = 1 << i
        sc = o.sigma_color * 2.0 ** -i
        sc2 = sc * sc
        p = 2 * step
        cur_p, nh_p = pad2(cur, (0, 0, p, p, p, p)), pad2(nh, (0, 0, p, p, p, p))
        m_p, surf_p = pad2(m, (p, p, p, p)), pad2(surf.float(), (p, p, p, p)) > 0
        S, W = torch.zeros_like(cur), torch.zeros_like(m)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = slice(p + dy * step, p + dy * step + h), slice(p + dx * step, p + dx * step + w)
                cq, nq, mq, taken = cur_p[ys, xs], nh_p[ys, xs], m_p[ys, xs], surf_p[ys, xs]
                hh = H5[dy + 2] * H5[dx + 2]
                if dx == 0 and dy == 0:
                    wt = torch.full_like(m, hh)
                else:
                    c = ((nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1]) + nh[..., 2] * nq[..., 2]).clamp(0, 1)
                    for _ in range(o.normal_power_log2):
                        c = c * c
                    mx = torch.maximum(m, mq)
                    den = o.sigma_depth * mx
                    rz = torch.where(den > 0, (m - mq) / den, torch.zeros_like(den))
                    d = cur - cq
                    dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wt = (hh * c) / ((1 + rz * rz) * (1 + dc / sc2))
                S = torch.where(taken[..., None], S + wt[..., None] * cq, S)
                W = torch.where(taken, W + wt, W)
        cur = torch.where(surf[..., None], S / torch.where(surf, W, torch.ones_like(W))[..., None], cur)
    return torch.where(surf[..., None], cur * a, L)


def guided_section(args, rend, st, say, timed, seed, spp):
    """r1_denoise_guided_device beside r1_denoise_device at 3 and 5 iterations, then its passes one by one; 56 bytes a pixel a pass: two
    16-byte records and v read once, a record and v written."""
    say()
    say(f"variance-guided filter (sigma_color 2, variance_floor 1e-4) beside the unguided one; R1_VFILTER_STAGE_MAX_STEP={os.environ.get('R1_VFILTER_STAGE_MAX_STEP', '-')}")
    for w, h in ((1200, 800), (1920, 1080)):
        rend.set_scene(r1.create_large_scene(w, h))
        p = r1.make_params(w, h, spp, seed, variant=binding.VARIANT_BVH)
        L = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        f = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
        V = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rend.render_moments_device(p, L.data_ptr(), V.data_ptr(), cnt.data_ptr(), stream_ptr=st.cuda_stream)
        rend.render_features_device(p, f.data_ptr(), stream_ptr=st.cuda_stream)
        st.synchronize()
        say(f"{w}x{h}")

        def guided(i):
            return lambda: rend.denoise_guided_device(w, h, binding.make_denoise_guided_opt(iterations=i), L.data_ptr(), f.data_ptr(), V.data_ptr(), out.data_ptr(),
                                                      stream_ptr=st.cuda_stream)

        def plain(i):
            return lambda: rend.denoise_device(w, h, binding.make_denoise_opt(iterations=i), L.data_ptr(), f.data_ptr(), out.data_ptr(), stream_ptr=st.cuda_stream)

        for it in (3, 5):
            forms = [(f"r1_denoise_device, {it} iterations", plain(it)), (f"r1_denoise_guided_device, {it} iterations", guided(it))]
            res = timed(forms, st)
            for name, _ in forms:
                v = res[name]
                say(f"  {name:<44} {statistics.median(v) * 1e3:9.3f} ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}) ms")
        forms = [(i, guided(i)) for i in range(1, 7)]
        res = timed(forms, st)
        med = {i: statistics.median(res[i]) for i, _ in forms}
        say(f"  guided passes: prepare + pass of step 1 {med[1] * 1e3:.3f} ms (one iteration); 56 bytes a pixel = {56 * w * h / 1e6:.1f} MB a pass")
        for i in range(1, 6):
            dt = med[i + 1] - med[i]
            say(f"    pass of step {1 << i:<2} {dt * 1e3:8.3f} ms  {56 * w * h / dt / 1e12 if dt > 0 else float('nan'):6.3f} TB/s of the 56-byte floor"
                f"   ({i + 1} iterations {med[i + 1] * 1e3:.3f} ms, {min(res[i + 1]) * 1e3:.3f} .. {max(res[i + 1]) * 1e3:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--only-denoise", action="store_true", help="form (a) and its passes alone (for comparing builds and R1_DENOISE_STAGE_MAX_STEP)")
    ap.add_argument("--guided", action="store_true", help="also the variance-guided filter beside the unguided one (DESIGN.md §4.40); with --lib "
                    "librays1_tuning.so R1_VFILTER_STAGE_MAX_STEP says up to which step its passes stage their taps in LDS (0: never)")
    args = ap.parse_args()
    if args.lib:
        binding.set_lib_path(os.path.abspath(args.lib))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(forms, st):
        res = {name: [] for name, _ in forms}
        for rnd in range(args.rounds + 1):
            for name, run in forms:
                st.synchronize()
                t0 = time.perf_counter()
                run()
                st.synchronize()
                if rnd:  # (round 0 warms up)
                    res[name].append(time.perf_counter() - t0)
        return res

    seed, spp = 4242, 4
    rend = r1.Renderer(0)
    st = torch.cuda.Stream()
    say(f"denoised frames; {args.rounds} rounds alternating after one warm-up round, host clock from enqueue to stream idle, median (min .. max) ms; the large scene at "
        f"{spp} spp, seed {seed}, box tree" + (f"; library {os.path.basename(args.lib)}, R1_DENOISE_STAGE_MAX_STEP={os.environ.get('R1_DENOISE_STAGE_MAX_STEP', '-')}" if args.lib else ""))
    for w, h in ((1200, 800), (1920, 1080)):
        rend.set_scene(r1.create_large_scene(w, h))
        p = r1.make_params(w, h, spp, seed, variant=binding.VARIANT_BVH)
        L = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        f = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
        out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def inputs():
            rend.render_linear_device(p, L.data_ptr(), cnt.data_ptr(), stream_ptr=st.cuda_stream)
            rend.render_features_device(p, f.data_ptr(), stream_ptr=st.cuda_stream)

        inputs()
        st.synchronize()
        surf = int((f[..., 7].view(torch.int32) > 0).sum())
        say()
        say(f"{w}x{h}: {w * h} pixels, {surf} with a hit")
        for it in (3, 5):
            o = binding.make_denoise_opt(iterations=it)
            forms = [(f"(a) r1_denoise_device, {it} iterations", lambda o=o: rend.denoise_device(w, h, o, L.data_ptr(), f.data_ptr(), out.data_ptr(), stream_ptr=st.cuda_stream))]
            if not args.only_denoise:
                def torch_form(o=o):
                    with torch.cuda.stream(st):
                        return composition(L, f, o)
                forms.append((f"(b) the contract in torch slices, {it} iterations", torch_form))
                forms.append(("(c) r1_render_linear_device + r1_render_features_device", inputs))
                forms[0][1]()
                other = forms[1][1]()
                st.synchronize()
                diff = (out - other).abs()
                scale = float(out.abs().max())
                say(f"  {it} iterations: (a) against (b): largest difference {float(diff.max()):.3e} (largest value {scale:.3e}), "
                    f"{float((out.view(torch.int32) == other.view(torch.int32)).float().mean()) * 100:.3f} % of the values equal to the bit")
            res = timed(forms, st)
            base = statistics.median(res[forms[1][0]]) if len(forms) > 1 else None
            for name, _ in forms:
                v = res[name]
                m = statistics.median(v)
                say(f"  {name:<58} {m * 1e3:9.3f} ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}) ms" + (f"  {base / m:6.2f} x (b)" if base else ""))
        # the passes one by one
        forms = [(i, lambda i=i: rend.denoise_device(w, h, binding.make_denoise_opt(iterations=i), L.data_ptr(), f.data_ptr(), out.data_ptr(), stream_ptr=st.cuda_stream))
                 for i in range(1, 7)]
        res = timed(forms, st)
        med = {i: statistics.median(res[i]) for i, _ in forms}
        say(f"  passes: prepare + pass of step 1 {med[1] * 1e3:.3f} ms (one iteration); 48 bytes a pixel = {48 * w * h / 1e6:.1f} MB a pass")
        for i in range(1, 6):
            dt = med[i + 1] - med[i]
            say(f"    pass of step {1 << i:<2} {dt * 1e3:8.3f} ms  {48 * w * h / dt / 1e12 if dt > 0 else float('nan'):6.3f} TB/s of the 48-byte floor"
                f"   ({i + 1} iterations {med[i + 1] * 1e3:.3f} ms, {min(res[i + 1]) * 1e3:.3f} .. {max(res[i + 1]) * 1e3:.3f})")
    if args.guided:
        guided_section(args, rend, st, say, timed, seed, spp)
    rend.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
