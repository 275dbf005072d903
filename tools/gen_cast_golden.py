#!/usr/bin/env python3
"""tools/gen_cast_golden.py — writes tests/golden/cast_{small,medium,large}.bin: 4096 seeded rays per scene and what the REFERENCE'S
OWN Hitable::hit answers for them (oracle/ref_harness.cpp's `rawcast`, which includes the reference's translation unit by path and is
compiled with the STRICT flags of oracle/Makefile into the git-ignored oracle/_ref/; no reference source text and nothing compiled from it
enters this repository).  Runs only where the reference's sources are present; the tests read the committed files.

    python tools/gen_cast_golden.py --ref /path/to/reference

Files are in the "R1GOLD01" tagged format (oracle/r1o.py read_golden): rays (f, 8 per ray: ox oy oz t_max dx dy dz 0), index (u,
0xFFFFFFFF = miss), t, p, n (f).  The reference's scene is tests/golden/scene_<name>_200x100.bin — its own dump of create_<name>_scene(),
from which the tests load the spheres too — loaded back into the reference's Scene by the harness, which checks on every load that its
dump gives the file's words again.  The generator asserts that the reference reports at least 5 % hits and 5 % misses in each of the
first five ray classes; re-seed if a class misses that, never relax it.

Ray classes (the same recipe for each scene; `field` = the box of the centres of the spheres of radius < 100, i.e. without the ground):
  camera   1024  primary rays of the fixture camera through pixel centres of a 200x100 frame, lens radius 0
  volume   1024  origins uniform in the field grown by half its size, random directions; 64 of them start > 10^4 units away and aim
                 at the field (the grid's far fallback), 32 start inside a sphere
  scatter  1024  origin = the reference's hit point of a camera / volume ray, direction = its normal + a random vector of the unit
                 ball: they start on a surface, where the 0.001 rule decides, and some start inside
  axis      512  one or two direction components exactly +0 or -0, origins snapped to a lattice of 0.5
  grazing   256  aimed at the tangent circle of a random sphere, the circle scaled by 1 +- 2^-k, k = 8..22; every second one runs
                 the other way along its line, from just past the tangent point up to the sky (the others meet the ground behind it)
  bounded   256  rays of the classes above that hit, with t_max = the reference's t bitwise, its two nextafter neighbours, t / 2, and
                 values around 0.001
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import r1o  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEEDS = {"small": 20001, "medium": 20002, "large": 20003}
FLT_MAX = np.float32(np.finfo(np.float32).max)
CLASSES = (("camera", 1024), ("volume", 1024), ("scatter", 1024), ("axis", 512), ("grazing", 256), ("bounded", 256))
f32 = np.float32


def build_harness(ref, tmp):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref", "REF=" + ref])
    return os.path.join(ROOT, "oracle", "_ref", "ref_step13_strict")


def reference_hits(exe, tmp, scene, rays):
    """rays (n, 8) float32 -> (index u32, t, p, n) from the reference on the scene of tests/golden/scene_<scene>_200x100.bin"""
    sp, rp, hp = (os.path.join(tmp, n) for n in ("scene.bin", "rays.f32", "hits.bin"))
    sa = r1o.SceneArrays.from_golden(r1o.read_golden(os.path.join(GOLD, f"scene_{scene}_200x100.bin")))
    with open(sp, "wb") as f:
        f.write(r1o.scene_file_bytes(sa))
    np.ascontiguousarray(rays, f32).tofile(rp)
    subprocess.check_call([exe, "rawcast", sp, rp, hp])
    w = np.fromfile(hp, np.uint32).reshape(-1, 8)
    fl = w.view(f32)
    return w[:, 1].copy(), fl[:, 0].copy(), fl[:, 2:5].copy(), fl[:, 5:8].copy()


def unit_ball(rng, n):
    out = np.empty((0, 3))
    while out.shape[0] < n:
        v = rng.uniform(-1.0, 1.0, (2 * n + 8, 3))
        out = np.concatenate([out, v[(v * v).sum(1) < 1.0]])
    return out[:n]


def unit_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def pack(o, d, t_max=None):
    n = o.shape[0]
    r = np.zeros((n, 8), f32)
    r[:, 0:3] = o.astype(f32)
    r[:, 3] = FLT_MAX if t_max is None else t_max
    r[:, 4:7] = d.astype(f32)
    return r


def make_rays(exe, tmp, name, gold):
    rng = np.random.default_rng(SEEDS[name])
    cx, cy, cz, rsq, invr = (gold[k].astype(np.float64) for k in ("cx", "cy", "cz", "rsq", "invr"))
    real = (gold["invr"] != 0) & np.isfinite(gold["cx"])
    rad = np.sqrt(np.maximum(rsq, 0.0))
    field = real & (rad < 100.0)
    c = np.stack([cx, cy, cz], 1)
    lo, hi = c[field].min(0), c[field].max(0)
    size = np.maximum(hi - lo, 1.0)
    glo, ghi = lo - 0.5 * size, hi + 0.5 * size
    ids = np.nonzero(field)[0]

    # camera
    cam = gold["camera"].astype(f32)
    pix = rng.choice(200 * 100, 1024, replace=False)
    u = ((pix % 200).astype(f32) + f32(0.5)) / f32(200)
    v = ((pix // 200).astype(f32) + f32(0.5)) / f32(100)
    d = cam[3:6][None, :] + u[:, None] * cam[6:9][None, :] + v[:, None] * cam[9:12][None, :] - cam[0:3][None, :]
    camera = pack(np.repeat(cam[0:3][None, :], 1024, 0), d)

    # volume
    o = rng.uniform(glo, ghi, (1024, 3))
    d = unit_dirs(rng, 1024)
    far_dir = unit_dirs(rng, 64)
    target = rng.uniform(lo, hi, (64, 3))
    o[:64] = 0.5 * (lo + hi) + far_dir * rng.uniform(2.0e4, 1.0e5, (64, 1))
    d[:64] = target - o[:64]
    inside = rng.choice(ids, 32)
    o[64:96] = c[inside] + 0.5 * rad[inside][:, None] * unit_ball(rng, 32)
    volume = pack(o, d)

    # scatter: from the reference's own hits of the rays above
    first = np.concatenate([camera, volume])
    idx, t, p, nrm = reference_hits(exe, tmp, name, first)
    hit = np.nonzero(idx != 0xFFFFFFFF)[0]
    assert hit.size >= 256, (name, hit.size)
    pick = rng.choice(hit, 1024, replace=hit.size < 1024)
    scatter = pack(p[pick], nrm[pick].astype(np.float64) + unit_ball(rng, 1024))

    # axis-parallel
    o = np.round(rng.uniform(glo, ghi, (512, 3)) * 2.0) / 2.0
    d = rng.uniform(-1.0, 1.0, (512, 3))
    d[np.abs(d) < 0.05] = 0.5
    zeros = rng.integers(1, 3, 512)  # one or two zero components
    for i in range(512):
        ax = rng.choice(3, zeros[i], replace=False)
        d[i, ax] = np.where(rng.integers(0, 2, zeros[i]) == 1, -0.0, 0.0)
    axis = pack(o, d)

    # grazing
    sph = rng.choice(np.nonzero(real)[0], 256)
    o = rng.uniform(glo, ghi, (256, 3))
    o[:, 1] = rng.uniform(0.02, max(ghi[1], 2.0), 256)
    low = np.arange(256) % 2 == 1  # every second ray runs the other way along its line: from just past the tangent point up to the sky
    o[low, 1] = rng.uniform(3.0, 10.0, int(low.sum()))  # (a steep line: the neighbours of a dense field are not in its way)
    w = c[sph] - o
    L = np.linalg.norm(w, axis=1)
    r = rad[sph]
    outside = L > 1.05 * r
    o[~outside] = c[sph][~outside] + (w[~outside] / L[~outside][:, None]) * -3.0 * r[~outside][:, None]  # (inside the sphere: step out along the axis)
    w = c[sph] - o
    L = np.linalg.norm(w, axis=1)
    w /= L[:, None]
    perp = np.cross(w, unit_dirs(rng, 256))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    k = rng.integers(8, 23, 256)
    s = 1.0 + np.where(rng.integers(0, 2, 256) == 1, 1.0, -1.0) * 2.0 ** (-k.astype(np.float64))
    tangent = c[sph] - w * (r * r / L)[:, None] + perp * (r * np.sqrt(1.0 - (r / L) ** 2) * s)[:, None]
    u = (tangent - o) / np.linalg.norm(tangent - o, axis=1, keepdims=True)
    start = np.where(low[:, None], tangent + u * (0.5 * np.minimum(r, 1.0))[:, None], o)
    grazing = pack(start, np.where(low[:, None], o - start, tangent - o))

    # bounded: rays of the classes above that hit, with t_max at and around the reference's t and around 0.001
    free = np.concatenate([camera, volume, scatter, axis, grazing])
    idx, t, p, nrm = reference_hits(exe, tmp, name, free)
    hit = np.nonzero(idx != 0xFFFFFFFF)[0]
    pick = rng.choice(hit, 256, replace=False)
    bounded = free[pick].copy()
    th = t[pick]
    tiny = f32(0.001)
    forms = [th, np.nextafter(th, f32(0)), np.nextafter(th, FLT_MAX), th / f32(2), np.full(256, tiny), np.full(256, np.nextafter(tiny, f32(1))),
             np.full(256, np.nextafter(tiny, f32(0))), np.full(256, f32(0.0011)), np.full(256, f32(0)), np.full(256, f32(-1))]
    # (the first four forms twice as often as the ones around 0.001)
    order = np.array([0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
    which = order[np.arange(256) % order.size]
    bounded[:, 3] = np.stack(forms, 0)[which, np.arange(256)]

    return np.concatenate([free, bounded]).astype(f32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference's source tree (the directory that holds src/step13)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_harness(args.ref, tmp)
        for name in ("small", "medium", "large"):
            gold = r1o.read_golden(os.path.join(GOLD, f"scene_{name}_200x100.bin"))
            rays = make_rays(exe, tmp, name, gold)
            assert rays.shape == (4096, 8)
            idx, t, p, nrm = reference_hits(exe, tmp, name, rays)
            at = 0
            for cls, n in CLASSES:
                hits = int((idx[at:at + n] != 0xFFFFFFFF).sum())
                print(f"{name:7s} {cls:8s} {n:5d} rays  {hits:5d} hits  {n - hits:5d} misses")
                if cls != "bounded":
                    assert hits * 20 >= n and (n - hits) * 20 >= n, (name, cls, hits, n)
                at += n
            out = os.path.join(GOLD, f"cast_{name}.bin")
            r1o.write_golden(out, (("rays", "f", rays), ("index", "u", idx), ("t", "f", t), ("p", "f", p), ("n", "f", nrm)))
            assert os.path.getsize(out) <= 280130
            with open(out, "rb") as f:
                print(f"{name:7s} {os.path.basename(out)} md5 {hashlib.md5(f.read()).hexdigest()}")


if __name__ == "__main__":
    main()
