"""The frames and ray sets whose expectations are held as REFERENCE fixtures (tests/golden/ref_*.bin, written by oracle/gen_edge_golden.py
from the reference's own Hitable::hit, Material::scatter and color run on the scene's arrays): the `small` size of every scene of
tests/edge_scenes.py, tests/leaf_scenes.py, tests/root_leaf_scenes.py (both orders) and tests/test_gpu_scatter.py, at the seeds, cameras
and shapes those modules use.  tests/test_reference_edges_host.py holds the oracle and the host forms to them, tests/test_gpu_reference_edges.py
the kernels; the generator imports this module too, so the three cannot disagree about a case.

A fixture (the tagged format of r1o.read_golden) holds, for the frames `main` (the scene's camera at its seed), `batch1` (the same camera
at seed + STRIDE) and `path1` (the turned camera at seed + STRIDE), all 64 x 48 at the module's SPP:

  hdr        w, h, spp, seed, depth limit, STRIDE
  sha256     of the scene file (r1o.scene_file_bytes) the reference was given for `main` and `batch1`;  p1sha256: for `path1`
  rays, rowrays (b1rays, b1rows, p1rays, p1rows)    the ray count and the per-row counts of every frame, in full
  image (b1image, p1image)  the frame's bytes — or imgsha (b1imgsha, p1imgsha), their SHA-256
  samples    the records of `main` (radiance + ray word per sample) — or recsha, the SHA-256 of their bytes
  castsha, hits   (CAST cases) the SHA-256 of the 1024 query rays' bytes and the reference's 32-byte hit records {t, index, p, n}

What is held in full and what as a digest follows from the size the fixtures may take together (1.5 MB): every comparison is the same
equality either way; a digest only says less about WHERE a difference lies (the per-row ray counts, always in full, say which rows).
The edge scenes keep everything in full — their records are looked into (deep paths, wrapped bytes, twins, tiny spheres) —, the scatter
scenes their three images, the leaf and root-leaf scenes digests."""
import collections
import hashlib
import os

import numpy as np

import r1o

import edge_scenes as es
import leaf_scenes as ls
import root_leaf_scenes as rl
import test_gpu_scatter as sc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = es.W, es.H
CAST_STEP, CAST_OFFSET = 4, 0  # every fourth ray of edge_scenes.cast_rays(name, "small"): 1024 rays
REGENERATE = "the scene has drifted from its fixture: regenerate with oracle/gen_edge_golden.py"

# full: which of a case's data the fixture holds in full — "images" (all three), "records" (of `main`)
Case = collections.namedtuple("Case", "id file build seed spp bounces stride full cast")


def _cases():
    out = []
    for name in es.SCENES:
        out.append(Case(f"edge-{name}", f"ref_edge_{name}.bin", (lambda name=name: es.build(name, "small")), es.SEED[name], es.SPP, 50,
                        es.STRIDE, ("images", "records"), name))
    for name in ls.SCENES:
        # (leaf_scenes' `coincident` IS edge_scenes' — same arrays, same seed —, so its ray set is the edge fixture's)
        out.append(Case(f"leaf-{name}", f"ref_leaf_{name}.bin", (lambda name=name: ls.build(name, "small")), ls.seed_of(name), ls.SPP, 50,
                        ls.STRIDE, (), None))
    for name in rl.SCENES:
        for order in rl.ORDERS:
            out.append(Case(f"root-{name}-{order}", f"ref_root_{name}_{order}.bin", (lambda name=name, order=order: rl.build(name, order, "small")),
                            rl.SEED, rl.SPP, 50, rl.STRIDE, (), None))
    for name in sc.SCENES:
        out.append(Case(f"scatter-{name}", f"ref_scatter_{name}.bin", (lambda name=name: sc._scene(name, "small")), sc.SEED, sc.SPP, sc.BOUNCES,
                        sc.STRIDE, ("images",), None))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
CAST_IDS = [c.id for c in CASES if c.cast]
FRAMES = (("main", "", 0, 0), ("batch1", "b1", 0, 1), ("path1", "p1", 1, 1))  # (frame, tag prefix, camera, seed + stride * this)


def sha(data):
    return np.frombuffer(hashlib.sha256(bytes(data)).digest(), np.uint8)


def scene_of(case, camera=0):
    """the case's r1o.SceneArrays with the scene's camera (0) or the turned one (1)"""
    sa, cam2 = case.build()
    return es.with_camera(sa, cam2) if camera else sa


def cast_rays_of(case):
    rays = np.ascontiguousarray(es.cast_rays(case.cast, "small")[CAST_OFFSET::CAST_STEP])
    assert rays.shape == (1024, 8)
    return rays


_fixtures = {}


def fixture(case):
    """the case's fixture, read once and left unchanged; fails if the scene no longer is the one the reference was given"""
    if case.id not in _fixtures:
        g = r1o.read_golden(os.path.join(GOLD, case.file))
        for a in g.values():
            a.setflags(write=False)
        _fixtures[case.id] = g
    g = _fixtures[case.id]
    assert g["hdr"].tolist() == [W, H, case.spp, case.seed, case.bounces, case.stride], (case.id, REGENERATE)
    assert sha(r1o.scene_file_bytes(scene_of(case, 0))).tobytes() == g["sha256"].tobytes(), (case.id, REGENERATE)
    assert sha(r1o.scene_file_bytes(scene_of(case, 1))).tobytes() == g["p1sha256"].tobytes(), (case.id, REGENERATE)
    if case.cast:
        assert sha(cast_rays_of(case).tobytes()).tobytes() == g["castsha"].tobytes(), (case.id, REGENERATE)
    return g


def assert_frame(g, prefix, image, rays, what):
    """a frame's ray count, then its bytes (or their digest), against the fixture's frame `prefix`"""
    want = int(g[prefix + "rays"][0])
    assert int(rays) == want, f"{what}: {int(rays)} rays, the reference counts {want}"
    image = np.ascontiguousarray(image, np.uint8).reshape(-1)
    if prefix + "image" in g:
        diff = int((image != g[prefix + "image"]).sum())
        assert diff == 0, f"{what}: {diff} bytes differ from the reference's frame"
    else:
        assert sha(image.tobytes()).tobytes() == g[prefix + "imgsha"].tobytes(), f"{what}: the frame's bytes are not the reference's"


def assert_records(g, samples, what):
    """the records of `main` (n, 4) float32 — radiance and ray word — against the fixture's, then the per-row counts they imply"""
    a = np.ascontiguousarray(samples, np.float32).reshape(-1, 4).view(np.uint32)
    rows = a[:, 3].astype(np.uint64).reshape(H, -1).sum(1)
    bad_rows = np.nonzero(rows != g["rowrays"])[0]
    assert bad_rows.size == 0, f"{what}: the ray counts of rows {bad_rows[:8].tolist()} differ from the reference's"
    if "samples" in g:
        b = g["samples"].view(np.uint32).reshape(-1, 4)
        bad = np.nonzero((a != b).any(1))[0]
        assert bad.size == 0, f"{what}: {bad.size} records differ from the reference's, first at {bad[:8].tolist()}: {a[bad[:3]]} != {b[bad[:3]]}"
    else:
        assert sha(a.tobytes()).tobytes() == g["recsha"].tobytes(), f"{what}: the records' bytes are not the reference's"


def hits_of(g):
    """the fixture's hit records as (index int32, t, p (n, 3), n (n, 3))"""
    w = g["hits"].reshape(-1, 8)
    f = w.view(np.float32)
    return w[:, 1].astype(np.int32), f[:, 0], f[:, 2:5], f[:, 5:8]


def assert_hits(g, hits, what):
    """binding.HIT_DTYPE records against the reference's, every word"""
    index, t, p, n = hits_of(g)
    assert hits.shape == (1024,), what
    bad = np.nonzero(hits["index"] != index)[0]
    assert bad.size == 0, f"{what}: {bad.size} rays name another sphere than the reference, first {bad[:8].tolist()}: {hits['index'][bad[:8]].tolist()} != {index[bad[:8]].tolist()}"
    assert hits["t"].tobytes() == t.tobytes(), what
    assert np.ascontiguousarray(hits["p"]).tobytes() == np.ascontiguousarray(p).tobytes(), what
    assert np.ascontiguousarray(hits["n"]).tobytes() == np.ascontiguousarray(n).tobytes(), what


def assert_occluded(g, occ, what):
    assert occ.dtype == np.uint8 and occ.tobytes() == (hits_of(g)[0] >= 0).astype(np.uint8).tobytes(), what
