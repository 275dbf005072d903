#!/usr/bin/env python3
"""tools/update_bench.py — moving spheres (r1_update_centers*) and sphere updates (r1_update_spheres*, §4.27) against the
only way there was to change a sphere, r1_set_scene (measurement tool; needs a GPU, reads no file outside the repository).

On the 100 004-sphere lattice of BASELINE config 5 (grid 400 x 250) at 1200 x 800 x 10, one context, in ONE session and alternating:
  (a) the time of one update of every centre, host form and device form (enqueue to stream idle), against one r1_set_scene with the
      same moved arrays;
  (b) the frame time after a refit for displacements of 0, 0.25, 1 and 4 lattice spacings (every lattice sphere, in a fixed pseudo-random
      direction of the plane) against a fresh build of the same moved scene — the number that tells a caller when to rebuild; the two
      frames are compared byte for byte on the way.
On the large scene (484 spheres, a tree with a flat y slab):
  (c) a frame after an identity update against one before it: the price of the dropped slab.
On config 5's scene again, sphere updates (none of these is a pass / fail threshold):
  (d) one update of all radii, host form and device form, against one r1_set_scene with the same arrays;
  (e) one materials-only update (every albedo and material row, no refit), host and device form, against the same;
  (f) the frame time after a radii update that scales the lattice radii by 0.5, 1 and 2 against a fresh build of that scene (the refitted
      tree keeps the topology of the original radii), the two frames compared byte for byte on the way, with the node visits and leaf
      trips of both trees from the diagnostic build.
The re-sort (r1_resort_spheres, §4.29; none of these is a pass / fail threshold either):
  (g.1) the time of one re-sort (enqueue to stream idle) on config 5's scene and on the large scene, beside one update of all centres and one
        r1_set_scene;
  (g.2) on config 5's scene, the frame after the refit alone, after the re-sort and after a fresh build of the same moved scene, for
        displacements of 0, 0.25, 1 and 4 spacings and for the lattice's centres permuted among its spheres — three contexts, alternating in
        one session, pixels and rays compared in every triple; and from it the displacement from which a re-sort pays for itself.
The regrid (r1_regrid, §4.31; none of these is a pass / fail threshold either):
  (h.1) the time of one regrid (enqueue to stream idle) on the large scene and on config 5's scene, beside r1_set_scene plus the first frame
        through the grid (which builds and uploads it) with the same arrays;
  (h.2) on the large scene, the frame through the grid after update + regrid, through the tree after the same update, and through the grid
        of a fresh r1_set_scene, for `jitter` and `lift` of tests/test_refit_host.py and displacements of 0.25, 1 and 4 spacings — three
        contexts, alternating in one session, pixels and rays compared in every triple; with the outliers, the registrations and the
        launch's workgroups per CU before and after the scene's first regrid (which grows the small kernel's LDS tables to the capacity).
Frames are r1_render_async into page-locked memory, timed from the enqueue to the stream idle by the host's clock.
Writes its report to profiles/r20/update.txt (--out FILE: somewhere else), section (g)'s to profiles/r22/resort.txt (--resort-out FILE) and
section (h)'s to profiles/r24/regrid.txt (--regrid-out FILE).  --section all: (a)-(g), as before; (h) runs on its own.
usage: tools/update_bench.py [--rounds N] [--frames N] [--out FILE] [--section all|a-f|g|h] [--resort-out FILE] [--regrid-out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("center_x", "center_y", "center_z", "radius_sq", "inv_radius", "albedo_r", "albedo_g", "albedo_b", "mat_param")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="frames per timing of (b) and (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "update.txt"), help="where the report is written")
    ap.add_argument("--section", choices=("all", "a-f", "g", "h"), default="all", help="g: the re-sort's section alone; h: the regrid's")
    ap.add_argument("--resort-out", default=os.path.join(ROOT, "profiles", "r22", "resort.txt"), help="where section (g)'s report is written")
    ap.add_argument("--regrid-out", default=os.path.join(ROOT, "profiles", "r24", "regrid.txt"), help="where section (h)'s report is written")
    args = ap.parse_args()
    import numpy as np
    import torch
    import rays1bench_amd as r1
    from rays1bench_amd import binding

    def lattice_of(a):
        """scene indices of the lattice: every hittable sphere but the four largest (the ground and the three big balls)"""
        act = np.nonzero(a["inv_radius"] != 0)[0]
        return np.setdiff1d(act, act[np.argsort(a["radius_sq"][act], kind="stable")[-4:]])

    def raw_from_arrays(a, x, y, z, **other):
        """a CScene over the scene's arrays with other centres, and other arrays by name (the returned dict keeps the arrays alive)"""
        keep = {k: np.ascontiguousarray(a[k], np.float32).copy() for k in FIELDS}
        keep["center_x"], keep["center_y"], keep["center_z"] = (np.ascontiguousarray(v, np.float32).copy() for v in (x, y, z))
        for k, v in other.items():
            keep[k] = np.ascontiguousarray(v, np.float32).copy()
        keep["mat_type"] = np.ascontiguousarray(a["mat_type"], np.uint8).copy()
        cs = binding.CScene()
        cs.count = len(keep["mat_type"])
        for k in FIELDS:
            setattr(cs, k, keep[k].ctypes.data_as(C.POINTER(C.c_float)))
        cs.mat_type = keep["mat_type"].ctypes.data_as(C.POINTER(C.c_uint8))
        return cs, keep

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def spread(v):
        return f"{statistics.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n = {len(v)})"

    w, h, spp, seed = 1200, 800, 10, 10001
    p = r1.make_params(w, h, spp, seed)
    hf = binding.HostFrames(w, h, 1)

    def frame_ms(ctx, n):
        def go():
            ctx.render_async(p, hf)
            ctx.sync()
        go()  # workspaces
        return [ms(go) for _ in range(n)]

    def section_g():
        """the re-sort; its own report"""
        del lines[:]
        sc = r1.create_grid_scene(w, h, 400, 250)
        a = sc.arrays()
        lat = lattice_of(a)
        spacing = float(np.ptp(a["center_x"][lat])) / 399.0
        rng = np.random.default_rng(5)
        ang = rng.uniform(0, 2 * np.pi, len(lat))

        def displaced(d):
            x, y, z = (a[k].copy() for k in ("center_x", "center_y", "center_z"))
            if d == "permuted":
                q = lat[np.random.default_rng(7).permutation(len(lat))]
                x[lat], y[lat], z[lat] = x[q], y[q], z[q]
                return x, y, z
            x[lat] = (x[lat] + d * spacing * np.cos(ang)).astype(np.float32)
            z[lat] = (z[lat] + d * spacing * np.sin(ang)).astype(np.float32)
            return x, y, z

        say(f"(g.1) one re-sort against one update of all centres and one r1_set_scene ({args.rounds} rounds, alternating; enqueue to stream idle, host clock)")
        resort_ms = {}
        for title, scene in (("config 5's scene", sc), ("the large scene", r1.create_large_scene(w, h))):
            b = scene.arrays()
            ctx = r1.Renderer(0)
            ctx.set_scene(scene)
            t_sort, t_upd, t_set = [], [], []
            for r in range(args.rounds + 1):
                bx = (b["center_x"] + np.float32(0.01 * (r % 2))).astype(np.float32)
                cs, keep = raw_from_arrays(b, bx, b["center_y"], b["center_z"])

                def update():
                    ctx.update_centers(0, bx, b["center_y"], b["center_z"])
                    ctx.sync()

                def resort():
                    ctx.resort_spheres()
                    ctx.sync()

                tu, tr, ts = ms(update), ms(resort), ms(lambda: ctx.set_scene_raw(cs, scene.camera.contents))
                if r:  # (round 0: scratch, staging buffer, first launches)
                    t_sort.append(tr), t_upd.append(tu), t_set.append(ts)
            info = binding.bvh_describe(scene.spheres.contents)[0]
            say(f"  {title}: {scene.count} spheres, {len(lattice_of(b))} movable, tree of {info['nodes']} nodes, depth {info['depth']}")
            say(f"    r1_resort_spheres  {spread(t_sort)}")
            say(f"    r1_update_centers  {spread(t_upd)}")
            say(f"    r1_set_scene       {spread(t_set)}")
            say(f"    r1_set_scene / re-sort {statistics.median(t_set) / statistics.median(t_sort):.1f} x")
            resort_ms[title] = statistics.median(t_sort)
            ctx.close()
        say()
        say(f"(g.2) config 5's scene, {w} x {h} x {spp}: the frame after the refit alone, after the re-sort, after a fresh build of the same moved scene "
            f"({args.frames} frames per timing, {args.rounds} rounds, alternating; permuted: 1 frame per timing, 2 rounds)")
        refit, sorted_, fresh = r1.Renderer(0), r1.Renderer(0), r1.Renderer(0)
        cost = resort_ms["config 5's scene"]
        for d in (0.0, 0.25, 1.0, 4.0, "permuted"):
            x, y, z = displaced(d)
            cs, keep = raw_from_arrays(a, x, y, z)
            for c in (refit, sorted_):
                c.set_scene(sc)
                c.update_centers(0, x, y, z)
            sorted_.resort_spheres()
            fresh.set_scene_raw(cs, sc.camera.contents)
            frames, rounds = (1, 2) if d == "permuted" else (args.frames, args.rounds)
            t = {"refit": [], "sorted": [], "fresh": []}
            same = True
            for r in range(rounds):
                out = []
                for name, c in (("refit", refit), ("sorted", sorted_), ("fresh", fresh)):
                    t[name] += frame_ms(c, frames)
                    out.append((hf.image(0).tobytes(), hf.rays(0)))
                same = same and out[0] == out[1] == out[2]
            m = {k: statistics.median(v) for k, v in t.items()}
            label = "lattice permuted         " if d == "permuted" else f"displacement {d:4.2f} spacings"
            gain = m["refit"] - m["sorted"]
            pays = f"pays for itself after {cost / gain:.1f} frames" if gain > 0 else "does not pay"
            say(f"  {label}: refit alone {m['refit']:9.3f} ms, re-sorted {m['sorted']:8.3f} ms, fresh build {m['fresh']:8.3f} ms; refit / fresh {m['refit'] / m['fresh']:7.2f}, "
                f"re-sorted / fresh {m['sorted'] / m['fresh']:5.2f}; a re-sort ({cost:.3f} ms) {pays}; pixels and rays {'equal' if same else 'DIFFER'}")
        refit.close(), sorted_.close(), fresh.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.resort_out)), exist_ok=True)
        with open(args.resort_out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def section_h():
        """the regrid; its own report"""
        del lines[:]
        grid_p = r1.make_params(w, h, spp, seed, variant=binding.VARIANT_GRID)

        def grid_frame(ctx):
            ctx.render_async(grid_p, hf)
            ctx.sync()

        def frames_of(ctx, params, n):
            def go():
                ctx.render_async(params, hf)
                ctx.sync()
            go()  # workspaces
            return [ms(go) for _ in range(n)]

        large = r1.create_large_scene(w, h)
        say(f"(h.1) one regrid against r1_set_scene plus the first frame through the grid, the same arrays ({args.rounds} rounds, alternating; enqueue to stream "
            f"idle, host clock; the first frame is {w} x {h} x {spp} and builds and uploads the grid)")
        for title, scene in (("the large scene", large), ("config 5's scene", r1.create_grid_scene(w, h, 400, 250))):
            b = scene.arrays()
            ctx = r1.Renderer(0)
            ctx.set_scene(scene)
            grid_frame(ctx)  # workspaces, the kernels' first launch
            plain = frames_of(ctx, grid_p, 3)
            t_grid, t_upd, t_set, t_first = [], [], [], []
            for r in range(args.rounds + 1):
                bx = (b["center_x"] + np.float32(0.01 * (r % 2))).astype(np.float32)
                cs, keep = raw_from_arrays(b, bx, b["center_y"], b["center_z"])
                ctx.regrid()  # (the plan of this r1_set_scene, the scene's first regrid: tables grown, scratch laid out)
                ctx.sync()

                def update():
                    ctx.update_centers(0, bx, b["center_y"], b["center_z"])
                    ctx.sync()

                def regrid():
                    ctx.regrid()
                    ctx.sync()

                tu, tg = ms(update), ms(regrid)
                ts, tf = ms(lambda: ctx.set_scene_raw(cs, scene.camera.contents)), ms(lambda: grid_frame(ctx))
                if r:  # (round 0: scratch, staging buffer, first launches)
                    t_grid.append(tg), t_upd.append(tu), t_set.append(ts), t_first.append(tf)
            info = binding.grid_describe(scene.spheres.contents)[0]
            say(f"  {title}: {scene.count} spheres, grid of {int(info['cells'][0])} x {int(info['cells'][1])} x {int(info['cells'][2])} cells, "
                f"{info['registrations']} registrations, {info['outliers']} outliers")
            say(f"    r1_regrid                        {spread(t_grid)}")
            say(f"    r1_update_centers                {spread(t_upd)}")
            say(f"    r1_set_scene                     {spread(t_set)}")
            say(f"    first frame through the grid     {spread(t_first)}")
            say(f"    a later frame through the grid   {spread(plain)}")
            first_cost = statistics.median(t_set) + statistics.median(t_first) - statistics.median(plain)
            say(f"    (r1_set_scene + the grid's build) / (update + regrid): {first_cost / (statistics.median(t_upd) + statistics.median(t_grid)):.1f} x")
            ctx.close()
        say()
        say(f"(h.2) the large scene, {w} x {h} x {spp}: the frame through the grid after update + regrid, through the tree after the same update, through the grid of a "
            f"fresh r1_set_scene ({args.frames} frames per timing, {args.rounds} rounds, alternating)")
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_refit_host import moved_centres
        a = large.arrays()
        lat = lattice_of(a)
        spacing = float(binding.grid_describe(large.spheres.contents)[0]["cell"][0])  # (the grid's cells along x are the lattice's pitch)
        ang = np.random.default_rng(5).uniform(0, 2 * np.pi, len(lat))

        def moved(d):
            if isinstance(d, str):
                return moved_centres(a, d)
            x, y, z = (a[k].copy() for k in ("center_x", "center_y", "center_z"))
            x[lat] = (x[lat] + d * spacing * np.cos(ang)).astype(np.float32)
            z[lat] = (z[lat] + d * spacing * np.sin(ang)).astype(np.float32)
            return x, y, z

        regridded, tree, fresh = r1.Renderer(0), r1.Renderer(0), r1.Renderer(0)
        tree_p = r1.make_params(w, h, spp, seed)
        regridded.set_scene(large), tree.set_scene(large)
        grid_frame(regridded)
        before = regridded.launch_info()
        built = regridded.grid_download()[0]
        regridded.regrid()
        grid_frame(regridded)
        after = regridded.launch_info()
        say(f"  lattice spacing {spacing:.3f}; the build: {built['registrations']} registrations, {built['outliers']} outliers; workgroups per CU "
            f"{before['blocks'] / before['compute_units']:.2f} ({before['blocks']} on {before['compute_units']} CUs) before the first regrid, "
            f"{after['blocks'] / after['compute_units']:.2f} ({after['blocks']}) after it (kernel {after['kernel']})")
        for d in ("jitter", "lift", 0.25, 1.0, 4.0):
            x, y, z = moved(d)
            cs, keep = raw_from_arrays(a, x, y, z)
            for c in (regridded, tree):
                c.update_centers(0, x, y, z)
            regridded.regrid()
            fresh.set_scene_raw(cs, large.camera.contents)
            info = regridded.grid_download()[0]
            t = {"regridded": [], "tree": [], "fresh": []}
            same = True
            for r in range(args.rounds):
                out = []
                for name, c, params in (("regridded", regridded, grid_p), ("tree", tree, tree_p), ("fresh", fresh, grid_p)):
                    t[name] += frames_of(c, params, args.frames)
                    out.append((hf.image(0).tobytes(), hf.rays(0)))
                same = same and out[0] == out[1] == out[2]
            m = {k: statistics.median(v) for k, v in t.items()}
            fresh_info = fresh.grid_download()[0]
            label = f"{d:<24s}" if isinstance(d, str) else f"displacement {d:4.2f} spacings"
            regs = "overflow" if info["registrations"] < 0 else f"{info['registrations']:4d} registrations"
            say(f"  {label}: regridded {m['regridded']:7.3f} ms ({regs}, {info['outliers']:3d} outliers), refitted tree {m['tree']:7.3f} ms, fresh grid "
                f"{m['fresh']:7.3f} ms ({fresh_info['registrations']} registrations, {fresh_info['outliers']} outliers); regridded / tree "
                f"{m['regridded'] / m['tree']:5.2f}, regridded / fresh {m['regridded'] / m['fresh']:5.2f}; pixels and rays {'equal' if same else 'DIFFER'}")
        regridded.close(), tree.close(), fresh.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.regrid_out)), exist_ok=True)
        with open(args.regrid_out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if args.section in ("g", "h"):
        section_g() if args.section == "g" else section_h()
        hf.close()
        return

    # ---- config 5's scene ----
    sc = r1.create_grid_scene(w, h, 400, 250)
    a = sc.arrays()
    lat = lattice_of(a)
    n = sc.count
    spacing = float(np.ptp(a["center_x"][lat])) / 399.0
    say(f"config 5's scene: {n} spheres ({len(lat)} in the lattice, spacing {spacing:.4f}), {w} x {h} x {spp}, one context")
    rng = np.random.default_rng(5)
    ang = rng.uniform(0, 2 * np.pi, len(lat))

    def displaced(d):
        x, y, z = (a[k].copy() for k in ("center_x", "center_y", "center_z"))
        x[lat] = (x[lat] + d * spacing * np.cos(ang)).astype(np.float32)
        z[lat] = (z[lat] + d * spacing * np.sin(ang)).astype(np.float32)
        return x, y, z

    ctx, other = r1.Renderer(0), r1.Renderer(0)
    ctx.set_scene(sc)
    say()
    say("(a) one update of all centres against one r1_set_scene with the same arrays (alternating, displacements 0.25 and 0.5 by turns)")
    t_host, t_dev, t_set = [], [], []
    for r in range(args.rounds + 1):
        x, y, z = displaced(0.25 + 0.25 * (r % 2))
        tx, ty, tz = (torch.from_numpy(v).cuda() for v in (x, y, z))
        torch.cuda.synchronize()
        cs, keep = raw_from_arrays(a, x, y, z)

        def host_form():
            ctx.update_centers(0, x, y, z)
            ctx.sync()

        def device_form():
            binding._check(binding.lib().r1_update_centers_device(ctx._c, 0, n, tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), None))
            ctx.sync()

        th, td, ts = ms(host_form), ms(device_form), ms(lambda: ctx.set_scene_raw(cs, sc.camera.contents))
        if r:  # (round 0: staging buffer, first launches)
            t_host.append(th), t_dev.append(td), t_set.append(ts)
        ctx.set_scene(sc)
    say(f"  r1_update_centers         {spread(t_host)}")
    say(f"  r1_update_centers_device  {spread(t_dev)}")
    say(f"  r1_set_scene              {spread(t_set)}")
    say(f"  r1_set_scene / update: host form {statistics.median(t_set) / statistics.median(t_host):.1f} x, device form "
        f"{statistics.median(t_set) / statistics.median(t_dev):.1f} x")
    bi = binding.bvh_describe(sc.spheres.contents)[0]
    say(f"  (tree: {bi['nodes']} nodes, {bi['leaves']} leaves, depth {bi['depth']}: one launch per height)")
    say()
    say(f"(b) frame time after a refit against a fresh build of the same moved scene ({args.frames} frames per timing, {args.rounds} rounds, alternating)")
    for d in (0.0, 0.25, 1.0, 4.0):
        x, y, z = displaced(d)
        cs, keep = raw_from_arrays(a, x, y, z)
        ctx.set_scene(sc)
        ctx.update_centers(0, x, y, z)
        other.set_scene_raw(cs, sc.camera.contents)
        t_refit, t_fresh, same = [], [], True
        for r in range(args.rounds):
            t_refit += frame_ms(ctx, args.frames)
            img_refit, rays_refit = hf.image(0).copy(), hf.rays(0)
            t_fresh += frame_ms(other, args.frames)
            same = same and rays_refit == hf.rays(0) and img_refit.tobytes() == hf.image(0).tobytes()
        mr, mf = statistics.median(t_refit), statistics.median(t_fresh)
        say(f"  displacement {d:4.2f} spacings: refitted {mr:7.3f} ms (min {min(t_refit):.3f}), fresh build {mf:7.3f} ms (min {min(t_fresh):.3f}), "
            f"refitted / fresh {mr / mf:5.2f}; pixels and rays {'equal' if same else 'DIFFER'}")
    ctx.close(), other.close()

    # ---- the large scene: the dropped flat slab ----
    say()
    sc2 = r1.create_large_scene(w, h)
    a2 = sc2.arrays()
    before, after = r1.Renderer(0), r1.Renderer(0)
    before.set_scene(sc2), after.set_scene(sc2)
    after.update_centers(0, a2["center_x"], a2["center_y"], a2["center_z"])
    say(f"(c) large scene ({sc2.count} spheres, flat y slab): a frame after an identity update against one before it ({args.frames} frames per timing, "
        f"{args.rounds} rounds, alternating)")
    t_b, t_a = [], []
    for r in range(args.rounds):
        t_b += frame_ms(before, args.frames)
        t_a += frame_ms(after, args.frames)
    say(f"  before (flat walk)    {spread(t_b)}")
    say(f"  after (generic loop)  {spread(t_a)}")
    say(f"  after / before: {statistics.median(t_a) / statistics.median(t_b):.3f}")
    before.close(), after.close()

    # ---- sphere updates on config 5's scene ----
    cx, cy, cz = (a[k] for k in ("center_x", "center_y", "center_z"))

    def scaled(f):
        """the lattice radii times f, stored as SphereSOA::add stores a radius"""
        rad = np.zeros(n, np.float32)
        rad[lat] = (np.float32(f) / a["inv_radius"][lat]).astype(np.float32)
        rsq, inv = a["radius_sq"].copy(), a["inv_radius"].copy()
        rsq[lat], inv[lat] = (rad[lat] * rad[lat]).astype(np.float32), (np.float32(1) / rad[lat]).astype(np.float32)
        return rsq, inv

    ctx, other = r1.Renderer(0), r1.Renderer(0)
    ctx.set_scene(sc)

    def one_update(title, label, host_args, dev_ptrs, cs):
        t_host, t_dev, t_set = [], [], []
        for r in range(args.rounds + 1):
            def host_form():
                ctx.update_spheres(0, **host_args[r % 2])
                ctx.sync()

            def device_form():
                ctx.update_spheres_device(0, n, stream_ptr=None, **dev_ptrs[r % 2])
                ctx.sync()

            th, td, ts = ms(host_form), ms(device_form), ms(lambda: ctx.set_scene_raw(cs[r % 2], sc.camera.contents))
            if r:
                t_host.append(th), t_dev.append(td), t_set.append(ts)
            ctx.set_scene(sc)
        say(title)
        say(f"  r1_update_spheres ({label})         {spread(t_host)}")
        say(f"  r1_update_spheres_device ({label})  {spread(t_dev)}")
        say(f"  r1_set_scene                        {spread(t_set)}")
        say(f"  r1_set_scene / update: host form {statistics.median(t_set) / statistics.median(t_host):.1f} x, device form "
            f"{statistics.median(t_set) / statistics.median(t_dev):.1f} x")

    say()
    host_args, dev_ptrs, keep_alive, css = [], [], [], []  # (keep_alive: the device arrays behind dev_ptrs)
    for f in (0.8, 1.25):
        rsq, inv = scaled(f)
        t = [torch.from_numpy(v).cuda() for v in (rsq, inv)]
        host_args.append({"radii": (rsq, inv)}), dev_ptrs.append({"radii": tuple(v.data_ptr() for v in t)}), keep_alive.append(t)
        css.append(raw_from_arrays(a, cx, cy, cz, radius_sq=rsq, inv_radius=inv))
    torch.cuda.synchronize()
    one_update("(d) one update of all radii against one r1_set_scene with the same arrays (alternating, lattice radii x 0.8 and x 1.25 by turns)", "radii",
               host_args, dev_ptrs, [c[0] for c in css])
    say()
    host_args, dev_ptrs, keep_alive, css = [], [], [], []
    for turn in (1, 2):
        alb = [np.roll(np.stack([a["albedo_r"], a["albedo_g"], a["albedo_b"]]), turn, 0)[k].copy() for k in range(3)]
        mats = (a["mat_type"], alb[0], alb[1], alb[2], a["mat_param"])
        t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in mats]
        host_args.append({"materials": mats}), dev_ptrs.append({"materials": tuple(v.data_ptr() for v in t)}), keep_alive.append(t)
        css.append(raw_from_arrays(a, cx, cy, cz, albedo_r=alb[0], albedo_g=alb[1], albedo_b=alb[2]))
    torch.cuda.synchronize()
    one_update("(e) one materials-only update (every albedo and material row; no refit) against one r1_set_scene with the same arrays (alternating, "
               "the albedo channels rotated by one and by two)", "materials", host_args, dev_ptrs, [c[0] for c in css])
    say()
    say(f"(f) frame time after a radii update against a fresh build of the same scene ({args.frames} frames per timing, {args.rounds} rounds, alternating)")
    for f in (0.5, 1.0, 2.0):
        rsq, inv = scaled(f)
        cs, keep = raw_from_arrays(a, cx, cy, cz, radius_sq=rsq, inv_radius=inv)
        ctx.set_scene(sc)
        ctx.update_spheres(0, radii=(rsq, inv))
        other.set_scene_raw(cs, sc.camera.contents)
        t_refit, t_fresh, same = [], [], True
        for r in range(args.rounds):
            t_refit += frame_ms(ctx, args.frames)
            img_refit, rays_refit = hf.image(0).copy(), hf.rays(0)
            t_fresh += frame_ms(other, args.frames)
            same = same and rays_refit == hf.rays(0) and img_refit.tobytes() == hf.image(0).tobytes()
        mr, mf = statistics.median(t_refit), statistics.median(t_fresh)
        visits = []
        for c in (ctx, other):  # the walk itself, from the tree's diagnostic build: node visits and leaf trips summed over lanes, one frame
            c.render(r1.make_params(w, h, spp, seed, variant=binding.VARIANT_BVH_STATS))
            raw = c.last_stats()["raw"]
            visits.append((raw[9], raw[14]))
        say(f"  lattice radii x {f:3.1f}: refitted {mr:7.3f} ms (min {min(t_refit):.3f}), fresh build {mf:7.3f} ms (min {min(t_fresh):.3f}), "
            f"refitted / fresh {mr / mf:5.2f}; pixels and rays {'equal' if same else 'DIFFER'}")
        say(f"      node visits per frame: refitted {visits[0][0]}, fresh {visits[1][0]} ({visits[0][0] / visits[1][0]:.2f}); "
            f"leaf trips x lanes: refitted {visits[0][1]}, fresh {visits[1][1]} ({visits[0][1] / visits[1][1]:.2f})")
    ctx.close(), other.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.section == "all":
        section_g()
    hf.close()


if __name__ == "__main__":
    main()
