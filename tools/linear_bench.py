#!/usr/bin/env python3
"""tools/linear_bench.py — what a linear frame costs beside the byte image (include/rays1.h; measurement tool).

One session, runs alternating, medians; the large scene at 1200 x 800 x 10, seed 10001, every linear frame checked against the bytes
(r1_quantise_linear of it equals r1_render's image) before anything is timed.  A linear frame is one more launch and 4 x the bytes home:
  (a) a synchronous frame: r1_render_linear against r1_render, on the device clock (HIP events of the library) and on the host clock,
      into page-locked and into pageable memory;
  (b) four frames in flight: r1_render_linear_async against r1_render_async, four contexts and streams, page-locked targets, one wait;
  (c) r1_pass_linear against a pass's byte preview: a pass of 10 samples with and without its image, and the read-out alone;
  (d) the device form: r1_render_linear_device against r1_render_shard_device + r1_assemble_device, into device memory, one wait.
No thresholds: the numbers are written down, nothing is tuned.
usage: tools/linear_bench.py [--rounds N] [--out FILE]   (FILE: profiles/rNN/linear.txt, NN the next free number)"""
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


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    w, h, spp, seed = 1200, 800, 10, 10001
    scene = r1.create_large_scene(w, h)
    p = r1.make_params(w, h, spp, seed)
    rend = r1.Renderer(0)
    rend.set_scene(scene)
    ref_img, ref_rays, _ = rend.render(p)
    lin, rays, _ = rend.render_linear(p)
    assert rays == ref_rays and binding.quantise_linear(lin).tobytes() == ref_img.tobytes()
    li = rend.launch_info()
    say(f"linear frames, large scene {w}x{h}x{spp}, seed {seed}, {ref_rays} rays per frame, {li['compute_units']} CUs; {args.rounds} rounds alternating, "
        f"medians; bytes per frame home: {w * h * 3 / 1e6:.2f} MB (image) against {w * h * 12 / 1e6:.2f} MB (linear)")

    # ---- (a) synchronous --------------------------------------------------------------------------------------------------------------
    pinned_b, pinned_f = binding.HostFrame(w, h), binding.LinearHostFrame(w, h)
    page_b, page_f = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32)
    forms = [("r1_render, page-locked", lambda: rend.render_into(p, pinned_b.image)), ("r1_render_linear, page-locked", lambda: rend.render_linear(p, pinned_f.image)[1:]),
             ("r1_render, pageable", lambda: rend.render_into(p, page_b)), ("r1_render_linear, pageable", lambda: rend.render_linear(p, page_f)[1:])]
    res = {name: {"wall": [], "dev": []} for name, _ in forms}
    for rnd in range(args.rounds + 1):
        for name, run in forms:
            t0 = time.perf_counter()
            got_rays, dev = run()
            wall = time.perf_counter() - t0
            assert got_rays == ref_rays, name
            if rnd:  # (round 0 warms up)
                res[name]["wall"].append(wall), res[name]["dev"].append(dev)
    assert binding.quantise_linear(pinned_f.image).tobytes() == ref_img.tobytes() and pinned_f.image.tobytes() == page_f.tobytes()
    say()
    say("(a) one synchronous frame")
    say(f"{'form':<32} {'device ms':>10} {'device Grays/s':>15} {'host ms':>9} {'host Grays/s':>13}")
    for name, _ in forms:
        d, t = med(res[name]["dev"]), med(res[name]["wall"])
        say(f"{name:<32} {d * 1e3:>10.3f} {ref_rays / d / 1e9:>15.2f} {t * 1e3:>9.3f} {ref_rays / t / 1e9:>13.2f}")
    for kind in ("page-locked", "pageable"):
        a, b = res[f"r1_render, {kind}"], res[f"r1_render_linear, {kind}"]
        say(f"  linear - bytes, {kind}: device {(med(b['dev']) - med(a['dev'])) * 1e6:+.1f} us, host {(med(b['wall']) - med(a['wall'])) * 1e6:+.1f} us")

    # ---- (b) four frames in flight ----------------------------------------------------------------------------------------------------
    K = 4
    ctxs = [r1.Renderer(0) for _ in range(K)]
    streams = [torch.cuda.Stream() for _ in range(K)]
    tb, tf = [binding.HostFrame(w, h) for _ in range(K)], [binding.LinearHostFrame(w, h) for _ in range(K)]
    for c in ctxs:
        c.set_scene(scene)

    def flight_bytes():
        for k, c in enumerate(ctxs):
            c.render_async(p, tb[k], streams[k].cuda_stream)

    def flight_linear():
        for k, c in enumerate(ctxs):
            c.render_linear_async(p, tf[k].ptr, tf[k].rays_ptr, streams[k].cuda_stream)

    flights = [("4 x r1_render_async", flight_bytes), ("4 x r1_render_linear_async", flight_linear)]
    times = {name: [] for name, _ in flights}
    for rnd in range(args.rounds + 1):
        for name, run in flights:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            for s in streams:
                s.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
    for k in range(K):
        assert tb[k].rays == ref_rays and tb[k].image.tobytes() == ref_img.tobytes()
        assert tf[k].rays == ref_rays and tf[k].image.tobytes() == lin.tobytes()
    say()
    say("(b) four frames in flight (four contexts and streams, page-locked targets, the span from the first enqueue to the last stream idle)")
    for name, _ in flights:
        t = med(times[name])
        say(f"{name:<32} {t * 1e3:>9.3f} ms for 4 frames, {t / K * 1e3:.3f} ms per frame, {K * ref_rays / t / 1e9:.2f} Grays/s")
    say(f"  linear - bytes: {(med(times[flights[1][0]]) - med(times[flights[0][0]])) / K * 1e6:+.1f} us per frame")

    # ---- (c) progressive -----------------------------------------------------------------------------------------------------------------
    t_prev, t_acc, t_read = [], [], []
    for rnd in range(args.rounds + 1):
        t0 = time.perf_counter()
        rend.render_pass(p, 0, image=True)
        t1 = time.perf_counter()
        rend.render_pass(p, 0, image=False)
        t2 = time.perf_counter()
        got, n = rend.pass_linear(p)
        t3 = time.perf_counter()
        assert n == spp and got.tobytes() == lin.tobytes()
        if rnd:
            t_prev.append(t1 - t0), t_acc.append(t2 - t1), t_read.append(t3 - t2)
    say()
    say("(c) a pass of 10 samples (host clock; the wrapper's frame is pageable memory)")
    say(f"  r1_render_pass with its byte preview   {med(t_prev) * 1e3:9.3f} ms")
    say(f"  r1_render_pass, accumulate only        {med(t_acc) * 1e3:9.3f} ms   (the preview: {(med(t_prev) - med(t_acc)) * 1e6:+.1f} us)")
    say(f"  r1_pass_linear (read-out + copy)       {med(t_read) * 1e3:9.3f} ms")

    # ---- (d) device-resident ----------------------------------------------------------------------------------------------------------
    nbytes = binding.shard_block_bytes(p)
    block = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out_f = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = streams[0]

    def dev_bytes():
        rend.render_shard_device(p, block.data_ptr(), count.data_ptr(), st.cuda_stream)
        rend.assemble_device(p, block.data_ptr(), out_b.data_ptr(), st.cuda_stream)

    def dev_linear():
        rend.render_linear_device(p, out_f.data_ptr(), count.data_ptr(), st.cuda_stream)

    devs = [("shard_device + assemble_device", dev_bytes), ("r1_render_linear_device", dev_linear)]
    dtimes = {name: [] for name, _ in devs}
    for rnd in range(args.rounds + 1):
        for name, run in devs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            st.synchronize()
            if rnd:
                dtimes[name].append(time.perf_counter() - t0)
    assert out_b.cpu().numpy().tobytes() == ref_img.tobytes() and out_f.cpu().numpy().tobytes() == lin.tobytes() and int(count.item()) == ref_rays
    say()
    say("(d) one frame into device memory (throughput kernels, host clock from the enqueue to the stream idle)")
    for name, _ in devs:
        t = med(dtimes[name])
        say(f"{name:<32} {t * 1e3:>9.3f} ms, {ref_rays / t / 1e9:.2f} Grays/s")
    say(f"  linear - bytes: {(med(dtimes[devs[1][0]]) - med(dtimes[devs[0][0]])) * 1e6:+.1f} us")

    for c in ctxs:
        c.close()
    for f in tb + tf + [pinned_b, pinned_f]:
        f.close()
    rend.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
