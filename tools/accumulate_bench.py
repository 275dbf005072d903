#!/usr/bin/env python3
"""tools/accumulate_bench.py — what an accumulated frame costs (include/rays1.h; measurement tool).

One session on one device; the forms alternate, one warm-up round each, host clock from the first enqueue to the stream being idle; medians
and the run-to-run spread (min .. max).  The large scene at 1200 x 800 and 1920 x 1080, 2 spp, box tree; an ORBIT: the frames go through
orbit_cameras(scene, 720), r1_set_camera per frame, so every accumulation has a history that moved by a few pixels.
  (a) r1_accumulate_device alone on two consecutive frames of the orbit held in device memory;
  (b) the same contract in torch indexing on the device, every line of the contract one torch operation, the taps by advanced indexing —
      what a user would write.  Whether its two images equal (a)'s to the bit is reported (torch's division and its fused kernels need not
      round as the contract does; where a coordinate differs by a rounding the tap is another pixel);
  (c) a frame of render_accumulated_device with the guided filter beside render_denoised_guided_device of the same params: what the
      accumulation adds to a filtered frame — the kernel, and the copy the unfiltered history costs nothing of here.
Then the kernel's time against its byte floor: the pixel's own records read once (60 bytes), four taps at most (240 bytes, of which
neighbouring pixels share most), 28 bytes written; the floor counts each of the three history images read once: 60 + 60 + 28 bytes a pixel.
No thresholds: the numbers are written down.
usage: tools/accumulate_bench.py [--rounds N] [--out FILE] [--lib LIBRARY]"""
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


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def unit(n):
    ln = torch.sqrt(dot(n, n))
    return torch.where((ln > 0)[..., None], n / torch.where(ln > 0, ln, torch.ones_like(ln))[..., None], torch.zeros_like(n))


def composition(L, V, f, Ap, fp, Mp, cam, prev, spp, spp_prev, o):
    """(b): the contract in torch on the current stream.  L, Ap (h, w, 3); V, Mp (h, w, 4) and f, fp (h, w, 8) float32 with the counts' bits in
    their last words; cam, prev: dicts of float32 device vectors."""
    h, w = L.shape[:2]
    dev = L.device
    dl = prev["lower_left"] - prev["origin"]
    pu, pv, pw = dot(dl, prev["u"]), dot(dl, prev["v"]), dot(dl, prev["w"])
    hu, vv = dot(prev["horizontal"], prev["u"]), dot(prev["vertical"], prev["v"])
    n = V[..., 3].view(torch.int32).long() & 0xFFFFFFFF
    hits = f[..., 7].view(torch.int32).long() & 0xFFFFFFFF
    surface = (hits != 0) & (n != 0)
    s = ((torch.arange(w, device=dev, dtype=torch.float32) + 0.5) * (1.0 / w))[None, :, None]
    t = ((torch.arange(h, device=dev, dtype=torch.float32) + 0.5) * (1.0 / h))[:, None, None]
    d = ((cam["lower_left"] + cam["horizontal"] * s) + cam["vertical"] * t) - cam["origin"]
    dh = d / torch.sqrt(dot(d, d))[..., None]
    m = (f[..., 3] / hits.float()) * float(spp)
    q = (cam["origin"] + dh * m[..., None]) - prev["origin"]
    a, b, c = dot(q, prev["u"]), dot(q, prev["v"]), dot(q, prev["w"])
    k = pw / c
    px, py = ((a * k - pu) / hu) * float(w) - 0.5, ((b * k - pv) / vv) * float(h) - 0.5
    exists = surface & (c * pw > 0) & (px > -1) & (px < w) & (py > -1) & (py < h)
    flx, fly = torch.floor(px), torch.floor(py)
    x0, y0 = torch.where(exists, flx, torch.zeros_like(flx)).long(), torch.where(exists, fly, torch.zeros_like(fly)).long()
    fx, fy = px - flx, py - fly
    e = torch.sqrt(dot(q, q))
    nh = unit(f[..., 4:7])
    B, Cs, U = torch.zeros_like(e), torch.zeros_like(L), torch.zeros_like(L)
    N = torch.full_like(n, 0xFFFFFFFF)
    for j in (0, 1):
        for i in (0, 1):
            tx, ty = x0 + i, y0 + j
            on = exists & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            cx, cy = tx.clamp(0, w - 1), ty.clamp(0, h - 1)
            fq, mq, aq = fp[cy, cx], Mp[cy, cx], Ap[cy, cx]
            hq = fq[..., 7].view(torch.int32).long() & 0xFFFFFFFF
            sq = mq[..., 3].view(torch.int32).long() & 0xFFFFFFFF
            bw = (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy)
            m_q = (fq[..., 3] / hq.float()) * float(spp_prev)
            take = on & (bw > 0) & (hq != 0) & (sq != 0) & ((e - m_q).abs() <= o.depth_tolerance * torch.maximum(e, m_q))
            take = take & ~(dot(nh, unit(fq[..., 4:7])) < o.normal_min_cos)
            B = torch.where(take, B + bw, B)
            Cs = torch.where(take[..., None], Cs + bw[..., None] * aq, Cs)
            U = torch.where(take[..., None], U + bw[..., None] * mq[..., 0:3], U)
            N = torch.where(take & (sq < N), sq, N)
    blend = exists & (B > 0)
    Bs = torch.where(blend, B, torch.ones_like(B))[..., None]
    hist, vh = Cs / Bs, U / Bs
    N_new = torch.maximum(n, torch.minimum(N + n, torch.full_like(n, int(o.max_samples))))
    alpha = torch.where(n >= N_new, torch.ones_like(e), n.float() / N_new.float())[..., None]
    A_out = torch.where(blend[..., None], hist + (L - hist) * alpha, L)
    var = torch.where(blend[..., None], ((1 - alpha) * (1 - alpha)) * vh + (alpha * alpha) * V[..., 0:3], V[..., 0:3])
    samples = torch.where(blend, N_new, n).int().view(torch.float32)
    return A_out, torch.cat([var, samples[..., None]], dim=-1)


def cam_tensors(cam):
    return {k: torch.tensor(list(getattr(cam, k)), dtype=torch.float32, device="cuda") for k in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--lib", default=None)
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

    seed, spp = 4242, 2
    rend = r1.Renderer(0)
    st = torch.cuda.Stream()
    o, go = binding.make_accumulate_opt(), binding.make_denoise_guided_opt()
    say(f"accumulated frames; {args.rounds} rounds alternating after one warm-up round, host clock from enqueue to stream idle, median (min .. max) ms; the large "
        f"scene at {spp} spp, seeds {seed} + frame, box tree, along orbit_cameras(scene, 720)" + (f"; library {os.path.basename(args.lib)}" if args.lib else ""))
    for w, h in ((1200, 800), (1920, 1080)):
        sc = r1.create_large_scene(w, h)
        cams = binding.orbit_cameras(sc, 720)
        rend.set_scene(sc)
        frames = []
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        for k in (0, 1):
            L = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            V = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            f = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rend.set_camera(cams[k])
            p = r1.make_params(w, h, spp, seed + k, variant=binding.VARIANT_BVH)
            rend.render_moments_device(p, L.data_ptr(), V.data_ptr(), cnt.data_ptr(), stream_ptr=st.cuda_stream)
            rend.render_features_device(p, f.data_ptr(), stream_ptr=st.cuda_stream)
            st.synchronize()
            frames.append((L, V, f))
        (Ap, Mp, fp), (L, V, f) = frames
        A_out, M_out = torch.zeros_like(L), torch.zeros_like(V)
        view = binding.make_accumulate_view(cams[1], cams[0], spp, spp)
        ct, pt = cam_tensors(cams[1]), cam_tensors(cams[0])
        torch.cuda.synchronize()

        def kernel():
            rend.accumulate_device(w, h, view, o, L.data_ptr(), V.data_ptr(), f.data_ptr(), Ap.data_ptr(), fp.data_ptr(), Mp.data_ptr(), A_out.data_ptr(), M_out.data_ptr(),
                                   stream_ptr=st.cuda_stream)

        def torch_form():
            with torch.cuda.stream(st):
                return composition(L, V, f, Ap, fp, Mp, ct, pt, spp, spp, o)

        kernel()
        tA, tM = torch_form()
        st.synchronize()
        blended = int((M_out[..., 3].view(torch.int32) != V[..., 3].view(torch.int32)).sum())
        eqA = float((A_out.view(torch.int32) == tA.view(torch.int32)).float().mean()) * 100
        eqM = float((M_out.view(torch.int32) == tM.view(torch.int32)).float().mean()) * 100
        say()
        say(f"{w}x{h}: {w * h} pixels, {int((f[..., 7].view(torch.int32) > 0).sum())} with a hit, {blended} with a longer history behind them")
        say(f"  (a) against (b): {eqA:.4f} % of A_out's and {eqM:.4f} % of M_out's words equal to the bit" + (" — equal" if eqA == 100 and eqM == 100 else " — not equal"))
        forms = [("(a) r1_accumulate_device", kernel), ("(b) the contract in torch indexing", torch_form)]
        res = timed(forms, st)
        base = statistics.median(res[forms[1][0]])
        for name, _ in forms:
            v = res[name]
            m = statistics.median(v)
            say(f"  {name:<62} {m * 1e3:9.3f} ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}) ms  {base / m:6.2f} x (b)")
        ka = statistics.median(res[forms[0][0]])
        floor = (60 + 60 + 28) * w * h
        say(f"  the kernel against its byte floor: {floor / 1e6:.1f} MB (60 own + 60 history + 28 written a pixel) in {ka * 1e3:.3f} ms = {floor / ka / 1e12:.3f} TB/s "
            "(host clock: the launch's latency is in it)")
        # (c) a filtered frame with and without the accumulation in front of the filter
        out = torch.zeros_like(L)
        state = {"k": 0}

        def accumulated():
            k = state["k"] = state["k"] + 1
            rend.set_camera(cams[k % 720])
            rend.render_accumulated_device(r1.make_params(w, h, spp, seed + k, variant=binding.VARIANT_BVH), o, go, out.data_ptr(), cnt.data_ptr(), st.cuda_stream)

        def filtered():
            k = state["k"]
            rend.set_camera(cams[k % 720])
            rend.render_denoised_guided_device(r1.make_params(w, h, spp, seed + k, variant=binding.VARIANT_BVH), go, out.data_ptr(), cnt.data_ptr(), st.cuda_stream)

        forms = [("(c) render_accumulated_device with the guided filter", accumulated), ("(c) render_denoised_guided_device", filtered)]
        res = timed(forms, st)
        for name, _ in forms:
            v = res[name]
            say(f"  {name:<62} {statistics.median(v) * 1e3:9.3f} ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}) ms")
        d = statistics.median(res[forms[0][0]]) - statistics.median(res[forms[1][0]])
        say(f"  the accumulation's share of a filtered frame: {d * 1e3:+.3f} ms of {statistics.median(res[forms[0][0]]) * 1e3:.3f} ms")
    rend.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
