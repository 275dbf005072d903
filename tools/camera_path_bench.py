#!/usr/bin/env python3
"""tools/camera_path_bench.py — camera paths (r1_set_camera, r1_render_path_async) against what the library had before
them (measurement tool; needs a GPU, reads no file outside the repository).

For the large scene and for the 100 004-sphere lattice of BASELINE config 5, both at 1200 x 800 x 10, over an orbit of distinct cameras
(binding.orbit_cameras), in ONE session and alternating, K contexts in flight:
  (a) the price of the per-frame camera in the kernel: r1_render_path_async against r1_render_batch_async of the same frames per
      launch — with the scene's own camera in every entry of the table (the same samples, bit for bit: the fetch alone) and with
      the orbit's cameras;
  (b) a moving camera, three ways: camera-path batches; r1_set_camera + r1_render_async per frame; and r1_set_scene(scene,
      camera_f) + r1_render_async per frame — the only form there was before r1_set_camera;
  (c) host time of one r1_set_camera against one r1_set_scene with a changed camera.
Every form's frames land in page-locked host memory; times are host wall clock from the first enqueue to the last frame landed.
usage: tools/camera_path_bench.py [--rounds N] [--inflight K] [--batch B] [--frames N] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inflight", type=int, default=8, help="contexts (frames or batches in flight); also GPU_MAX_HW_QUEUES of the run")
    ap.add_argument("--batch", type=int, default=4, help="frames per launch of the batch forms")
    ap.add_argument("--frames", type=int, default=64, help="frames of the orbit (config 5: half of it)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    os.environ["GPU_MAX_HW_QUEUES"] = str(max(2, min(32, args.inflight)))  # one hardware queue per context in flight; before HIP starts
    import rays1bench_amd as r1
    from rays1bench_amd import binding
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    K, B = args.inflight, args.batch
    w, h, spp, seed = 1200, 800, 10, 10001
    p = r1.make_params(w, h, spp, seed)
    ctxs = [r1.Renderer(0) for _ in range(K)]
    hfb = [binding.HostFrames(w, h, B) for _ in range(K)]
    hf1 = [binding.HostFrames(w, h, 1) for _ in range(K)]

    def batches(n, launch):
        """n frames as launches of B over the K contexts; launch(slot, first frame, frames).  Returns (seconds, rays)."""
        count = [0] * K
        rays = 0
        t0 = time.perf_counter()
        for l in range((n + B - 1) // B):
            s = l % K
            if l >= K:
                ctxs[s].sync()
                rays += sum(hfb[s].rays(i) for i in range(count[s]))
            count[s] = min(B, n - l * B)
            launch(s, l * B, count[s])
        for s in range(K):
            ctxs[s].sync()
            rays += sum(hfb[s].rays(i) for i in range(count[s]))
        return time.perf_counter() - t0, rays

    def frames(n, prepare):
        """n single frames over the K contexts; prepare(slot, frame) sets the view.  Returns (seconds, rays)."""
        used = [False] * K
        rays = 0
        t0 = time.perf_counter()
        for f in range(n):
            s = f % K
            if used[s]:
                ctxs[s].sync()
                rays += hf1[s].rays(0)
            prepare(s, f)
            ctxs[s].render_async(p, hf1[s])
            used[s] = True
        for s in range(K):
            if used[s]:
                ctxs[s].sync()
                rays += hf1[s].rays(0)
        return time.perf_counter() - t0, rays

    say(f"camera paths, {w}x{h}x{spp}, seed {seed}, {K} contexts in flight (GPU_MAX_HW_QUEUES={os.environ['GPU_MAX_HW_QUEUES']}), {B} frames per launch of the batch forms, "
        f"{args.rounds} rounds alternating; host wall clock, frames landed in page-locked memory")
    for label, make, n in (("large scene (484 spheres)", lambda: r1.create_large_scene(w, h), args.frames),
                           ("config 5 (100 004 spheres, 400 x 250 lattice)", lambda: r1.create_grid_scene(w, h, 400, 250), max(B, args.frames // 2))):
        sc = make()
        cams = binding.orbit_cameras(sc, n)
        own = sc.camera.contents
        cs = sc.spheres.contents
        for c in ctxs:
            c.set_scene(sc)
        forms = [
            ("batch, one camera (r1_render_batch_async)", lambda: batches(n, lambda s, f0, m: ctxs[s].render_batch_async(p, m, hfb[s], seed_stride=0))),
            ("path, one camera in every entry", lambda: batches(n, lambda s, f0, m: ctxs[s].render_path_async(p, [own] * m, hfb[s]))),
            ("path, orbit cameras", lambda: batches(n, lambda s, f0, m: ctxs[s].render_path_async(p, cams[f0:f0 + m], hfb[s]))),
            ("r1_set_camera + r1_render_async per frame", lambda: frames(n, lambda s, f: ctxs[s].set_camera(cams[f]))),
            ("r1_set_scene(camera_f) + r1_render_async per frame", lambda: frames(n, lambda s, f: ctxs[s].set_scene_raw(cs, cams[f]))),
        ]
        # the forms agree: frame 1 of the orbit through a path, through r1_set_camera and through r1_set_scene
        ctxs[0].render_path_async(p, cams[:2], hfb[0])
        ctxs[0].sync()
        want = (hfb[0].image(1).tobytes(), hfb[0].rays(1))
        for prep in (lambda: ctxs[0].set_camera(cams[1]), lambda: ctxs[0].set_scene_raw(cs, cams[1])):
            prep()
            ctxs[0].render_async(p, hf1[0])
            ctxs[0].sync()
            assert (hf1[0].image(0).tobytes(), hf1[0].rays(0)) == want
        res = {name: [] for name, _ in forms}
        for name, run in forms:  # warm-up: workspaces, occupancy queries, the first launch of every kernel
            run()
            for c in ctxs:
                c.set_camera(own)
        for _ in range(args.rounds):
            for name, run in forms:
                res[name].append(run())
                for c in ctxs:
                    c.set_camera(own)  # (every form starts from the scene's own camera)
        li = ctxs[0].launch_info()
        say()
        say(f"{label}: {n} frames per run, kernel {li['kernel']} (DEFAULT)")
        say(f"  {'form':<52} {'ms/frame':>9} {'Grays/s':>8} {'ms/frame, every round':>24}   rays per run")
        base = None
        for name, _ in forms:
            ms = [t / n * 1e3 for t, _ in res[name]]
            med = statistics.median(ms)
            rays = res[name][0][1]
            gr = statistics.median([r / t / 1e9 for t, r in res[name]])
            base = med if base is None else base
            say(f"  {name:<52} {med:>9.3f} {gr:>8.2f} {' '.join(f'{x:.3f}' for x in ms):>24}   {rays}")
        b = statistics.median([t for t, _ in res[forms[0][0]]])
        one = statistics.median([t for t, _ in res[forms[1][0]]])
        orbit = statistics.median([t for t, _ in res[forms[2][0]]])
        setcam = statistics.median([t for t, _ in res[forms[3][0]]])
        setscene = statistics.median([t for t, _ in res[forms[4][0]]])
        say(f"  (a) path with one camera / batch: {one / b:.4f} (same samples); spread of the batch form over the rounds: "
            f"{(max(t for t, _ in res[forms[0][0]]) / min(t for t, _ in res[forms[0][0]]) - 1) * 100:.1f} %")
        say(f"  (b) per orbit frame: r1_set_scene form / path batches = {setscene / orbit:.2f}x, r1_set_scene form / r1_set_camera form = {setscene / setcam:.2f}x")
        # (c) host time of the two calls alone
        t_cam, t_scene = [], []
        for i in range(9):
            t0 = time.perf_counter()
            ctxs[0].set_camera(cams[(i + 1) % n])
            t_cam.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctxs[0].set_scene_raw(cs, cams[(i + 2) % n])
            t_scene.append(time.perf_counter() - t0)
        say(f"  (c) host time of one call: r1_set_camera {statistics.median(t_cam) * 1e6:.1f} us, r1_set_scene with a changed camera "
            f"{statistics.median(t_scene) * 1e3:.2f} ms (medians of 9)")
        sc.close()
    for x in hfb + hf1:
        x.close()
    for c in ctxs:
        c.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
