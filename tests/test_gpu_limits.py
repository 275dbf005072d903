"""Frames at the C-ABI's 32-bit limits: the one-launch ceiling of 2^31 padded sample slots (one frame, a batch), frame ray counts above
2^32, one tile whose records span 4 GiB and more, sides of 65 535 pixels, extreme tilings, the wavefront variant's 2^24 slots and seeds
that wrap.  Every render is compared bit for bit with an independent path: r1_render_pass in several small passes (bit-exact with r1_render
by contract), r1_render on kernels that sum no tile inside the trace launch, or the oracle on spot pixels.  Every case also
asserts that it reached the path it is about (launch_info: kernel, tiles_in_kernel) or, for a refusal, the code and the rule named.

Each case runs in a child process with a time limit (`python tests/test_gpu_limits.py CASE` runs one alone and prints a JSON summary); its
contexts are closed before it ends, so device memory peaks near one 2^31-slot frame (32 GiB of records).  Once a child has run out of time,
the cases after it are skipped: a launch that spins on the GPU is not followed by more launches.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "oracle")):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    import torch  # noqa: F401  (before librays1: one HIP runtime per process)
    if os.environ.get("R1_TEST_LIB"):
        from rays1bench_amd import binding as _binding
        _binding.set_lib_path(os.environ["R1_TEST_LIB"])

import numpy as np
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding, sharding
import r1o

pytestmark = pytest.mark.gpu

SENTINEL = 0xCD
CHILD_TIMEOUT_S = 240
SLOTS = "2^31 sample slots per launch"  # the padded-slot rule (r1_frame.cpp prepare_tiles, r1_render.cpp r1_render_pass)
BVH, TILE4G_SPPS = binding.VARIANT_BVH, (8191, 8192, 16383, 16384, 20000)


# ---- helpers --------------------------------------------------------------------------------------------------------------------------

def same(a, b, what):
    """(image, rays) pairs equal, every byte and the count."""
    assert a[1] == b[1], (what, "rays", a[1], b[1])
    if a[0].tobytes() != b[0].tobytes():
        diff = (a[0] != b[0]).any(axis=2)
        ys, xs = np.nonzero(diff)
        raise AssertionError(f"{what}: {int(diff.sum())} pixels differ, first at x={int(xs[0])} y={int(ys[0])}")


def refused(fn, rule, code=binding.R1_ELIMIT):
    with pytest.raises(binding.R1Error) as e:
        fn()
    assert e.value.code == code and rule in str(e.value), str(e.value)


def refused_async(rend, p, rule):
    """r1_render_async of p is refused (its target is sized for p all the same)."""
    hf = binding.HostFrames(p.width, p.height, 1)
    try:
        refused(lambda: rend.render_async(p, hf), rule)
    finally:
        hf.close()


def params(w, h, spp, seed, **kw):
    return r1.make_params(w, h, spp, seed, **kw)


def passes(rend, p, sizes):
    """The frame of p rendered in passes of `sizes` samples: (image, cumulative rays)."""
    assert sum(sizes) == p.spp
    first, img, rays = 0, None, 0
    for k, n in enumerate(sizes):
        q = r1.make_params(p.width, p.height, n, p.seed, p.max_bounces, p.tile_w, p.tile_h, variant=p.variant)
        img, rays = rend.render_pass(q, first, image=k == len(sizes) - 1)
        first += n
    return img, rays


def split(spp, most):
    return [most] * (spp // most) + ([spp % most] if spp % most else [])


def render(rend, p, land=False, kernel=BVH):
    out = rend.render(p)
    info = rend.launch_info()
    assert info["kernel"] == kernel and info["tiles_in_kernel"] == (1 if land else 0), info
    return out[0], out[1]


def render_async(rend, p):
    """r1_render_async into page-locked memory filled with a sentinel: the frame's tiles are summed inside the trace launch."""
    hf = binding.HostFrames(p.width, p.height, 1)
    try:
        hf._all[:] = SENTINEL
        rend.render_async(p, hf)
        rend.sync()
        info = rend.launch_info()
        assert info["tiles_in_kernel"] == 1 and info["kernel"] == BVH, info
        return hf.image(0).copy(), hf.rays(0)
    finally:
        hf.close()


def batch_async(rend, p, n, stride):
    hf = binding.HostFrames(p.width, p.height, n)
    try:
        hf._all[:] = SENTINEL
        rend.render_batch_async(p, n, hf, seed_stride=stride)
        rend.sync()
        info = rend.launch_info()
        assert info["tiles_in_kernel"] == 1 and info["kernel"] == BVH, info
        return [(hf.image(f).copy(), hf.rays(f)) for f in range(n)]
    finally:
        hf.close()


def batch_device_records(rend, p, n, stride):
    """r1_render_shard_device_batch (one shard) + r1_assemble_device_records_batch: n frames assembled on the device."""
    import torch
    p0 = r1.make_params(p.width, p.height, p.spp, p.seed, p.max_bounces, p.tile_w, p.tile_h, 0, 1, p.variant)
    rec, frec = binding.shard_record_bytes(p0), binding.frame_record_bytes(p0)
    gathered = torch.full((n, rec), SENTINEL, dtype=torch.uint8, device="cuda")
    frames = torch.full((n, frec), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rend.render_shard_device_batch(p0, n, gathered.data_ptr(), seed_stride=stride, stream_ptr=st)
    rend.assemble_device_records_batch(p0, n, gathered.data_ptr(), frames.data_ptr(), st)
    torch.cuda.synchronize()
    host = frames.cpu().numpy()
    nb = p.width * p.height * 3
    return [(host[f, :nb].reshape(p.height, p.width, 3), int(host[f, frec - 8:].view(np.uint64)[0])) for f in range(n)]


def sharded(rend, p, shards):
    """Every shard of p through r1_render_shard_device, the blocks assembled on the device: the union of the shards."""
    import torch
    q = [r1.make_params(p.width, p.height, p.spp, p.seed, p.max_bounces, p.tile_w, p.tile_h, s, shards, p.variant) for s in range(shards)]
    rec = binding.shard_record_bytes(q[0])  # (the block padded to 8 bytes, then the shard's uint64 count)
    records = torch.full((shards, rec), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((p.height, p.width, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for s in range(shards):
        rend.render_shard_device(q[s], records[s].data_ptr(), records[s].data_ptr() + rec - 8, st)
    rend.assemble_device_strided(q[0], records.data_ptr(), rec, out.data_ptr(), st)
    torch.cuda.synchronize()
    return out.cpu().numpy(), sharding.total_rays(records.view(-1), shards)


def quantise(col, n):
    """r1_resolve_kernel's arithmetic on sequential fp32 sums: * (float)(1.0f / n), sqrtf, (uint8)(int)(c * 255.99f)."""
    c = col.astype(np.float32) * (np.float32(1.0) / np.float32(n))
    return (np.sqrt(c) * np.float32(255.99)).astype(np.int32).astype(np.uint8)


def oracle_spots(scene, p, img, spots):
    """Pixels of img against the oracle: every sample traced on the CPU and summed in sample order in fp32."""
    sa = r1o.SceneArrays.from_c(scene.spheres, scene.camera)
    for x, y in spots:
        rgb, _ = r1o.trace_samples(sa, p.width, p.height, p.seed, np.full(p.spp, x), np.full(p.spp, y), np.arange(p.spp))
        col = np.cumsum(rgb, axis=0, dtype=np.float32)[-1]
        assert img[y, x].tobytes() == quantise(col, p.spp).tobytes(), (x, y, img[y, x], quantise(col, p.spp))


# ---- the cases (each in a child process) ----------------------------------------------------------------------------------------------

def case_ceiling_frame():
    """1920 x 1080 x 1028 with 32 x 32 tiles: 2040 tiles x 1024 slots x 1028 = 2 147 450 880 padded slots, one launch, on every entry
    point that renders a whole frame; x 1029 is 2 133 792 000 samples (legal unpadded) but 2 149 539 840 padded slots: refused."""
    w, h, spp, seed = 1920, 1080, 1028, 7771
    sc = r1.create_large_scene(w, h)
    p = params(w, h, spp, seed)
    out = {"padded_slots": 2040 * 1024 * spp}
    assert out["padded_slots"] < 2 ** 31 <= 2040 * 1024 * (spp + 1) and w * h * (spp + 1) < 2 ** 31
    rend = r1.Renderer(0)
    try:
        rend.set_scene(sc)
        t0 = time.perf_counter()
        want = passes(rend, p, [257] * 4)
        out["passes_s"] = time.perf_counter() - t0
        out["rays"] = want[1]
        assert want[1] > 2 ** 32, want[1]  # the frame's ray count needs more than 32 bits
        oracle_spots(sc, p, want[0], [(0, 0), (1919, 1079), (960, 540)])  # first tile, the highest slot (last tile, last sample), middle
        t0 = time.perf_counter()
        same(render(rend, p), want, "r1_render")
        out["r1_render_s"] = time.perf_counter() - t0
        same(render_async(rend, p), want, "r1_render_async")
        for shards in (1, 2, 3):
            same(sharded(rend, p, shards), want, f"device frame, {shards} shard(s)")
        rend.set_pixel_mode(True)
        same(sharded(rend, p, 1), want, "PIXEL mode")
        assert rend.launch_info()["tiles_in_kernel"] == 0
        rend.set_pixel_mode(False)
        same(render(rend, params(w, h, spp, seed, variant=binding.VARIANT_PREFILTER), kernel=binding.VARIANT_PREFILTER), want, "exhaustive sweep")
        same(render(rend, params(w, h, spp, seed, variant=binding.VARIANT_GRID), kernel=binding.VARIANT_GRID), want, "grid")
        over = params(w, h, spp + 1, seed)
        assert binding.tile_count(over) == (2040, 2040)  # (the host's unpadded check lets it through)
        refused(lambda: rend.render(over), SLOTS)
        refused_async(rend, over, SLOTS)
        refused(lambda: sharded(rend, over, 1), SLOTS)
        refused(lambda: rend.render_pass(over, 0), SLOTS)
        same(render_async(rend, p), want, "r1_render_async after the refusals")
    finally:
        rend.close()
    m = binding.MultiRenderer([0])  # (after the context is gone: one 32 GiB workspace at a time)
    try:
        m.set_scene(sc)
        img, rays, _ = m.render(p)
        same((img, rays), want, "r1_multi_render, one device")
    finally:
        m.close()
    return out


def case_ceiling_exact():
    """2040 x 1020 (64 x 32 tiles of 32 x 32): x 1023 is 2 145 386 496 padded slots and renders; x 1024 is exactly 2^31 padded slots
    (2 130 739 200 samples) and is refused."""
    w, h, seed = 2040, 1020, 99
    sc = r1.create_large_scene(w, h)
    p = params(w, h, 1023, seed)
    rend = r1.Renderer(0)
    out = {}
    try:
        rend.set_scene(sc)
        want = passes(rend, p, [341] * 3)
        out["rays"] = want[1]
        assert want[1] > 2 ** 32
        oracle_spots(sc, p, want[0], [(2039, 1019)])
        same(render(rend, p), want, "r1_render")
        same(render_async(rend, p), want, "r1_render_async")
        over = params(w, h, 1024, seed)
        assert binding.tile_count(over) == (2048, 2048)
        refused(lambda: rend.render(over), SLOTS)
        refused_async(rend, over, SLOTS)
        refused(lambda: rend.render_pass(over, 0), SLOTS)
        refused(lambda: rend.render_batch_async(over, 1, None), SLOTS)
        same(render(rend, p), want, "r1_render after the refusals")
    finally:
        rend.close()
    return out


def case_ceiling_batch():
    """Two 1920 x 1080 x 514 frames in one launch: 2 x 2040 x 1024 x 514 = 2 147 450 880 slots; x 515 is refused.  Each frame equals
    r1_render of its seed."""
    w, h, spp, seed = 1920, 1080, 514, 123457
    p = params(w, h, spp, seed)
    rend = r1.Renderer(0)
    out = {}
    try:
        rend.set_scene(r1.create_large_scene(w, h))
        want = [render(rend, params(w, h, spp, seed + f)) for f in range(2)]
        out["rays"] = [x[1] for x in want]
        for f, got in enumerate(batch_async(rend, p, 2, 1)):
            same(got, want[f], f"r1_render_batch_async frame {f}")
        for f, got in enumerate(batch_device_records(rend, p, 2, 1)):
            same(got, want[f], f"device records batch frame {f}")
        over = params(w, h, spp + 1, seed)
        refused(lambda: rend.render_batch_async(over, 2, None, seed_stride=1), SLOTS)
        refused(lambda: batch_device_records(rend, over, 2, 1), SLOTS)
        same(render_async(rend, p), want[0], "r1_render_async after the refusals")
    finally:
        rend.close()
    return out


def _tile4g(spp):
    """One 128 x 128 tile of spp samples: its records span 16 384 x spp x 16 bytes (2^31 at 8192, 2^32 at 16 384, beyond at 20 000), all
    summed by one wave inside the trace launch: r1_render_async, a 2-frame batch, and r1_render on a 1 604-sphere lattice (big-scene
    kernels: the synchronous path sums tiles in the trace launch too); r1_render of the large scene (a resolve launch) and passes of
    <= 4096 samples are the comparators."""
    w = h = 128
    seed = 50000 + spp
    p = params(w, h, spp, seed, tile_w=128, tile_h=128)
    rend = r1.Renderer(0)
    out = {"span_bytes": 16384 * spp * 16}
    try:
        sc = r1.create_large_scene(w, h)
        rend.set_scene(sc)
        want = passes(rend, p, split(spp, 4096))
        out["rays"] = want[1]
        if spp == TILE4G_SPPS[-1]:
            oracle_spots(sc, p, want[0], [(127, 127)])
        same(render(rend, p), want, "r1_render (resolve launch)")
        t0 = time.perf_counter()
        same(render_async(rend, p), want, "r1_render_async")
        out["async_s"] = time.perf_counter() - t0
        b = batch_async(rend, p, 2, 1)
        same(b[0], want, "batch frame 0")
        same(b[1], render(rend, params(w, h, spp, seed + 1, tile_w=128, tile_h=128)), "batch frame 1")
        lattice = r1.create_grid_scene(w, h, 40, 40)
        rend.set_scene(lattice)
        want = passes(rend, p, split(spp, 4096))
        same(render(rend, p, land=True), want, "r1_render, 1 604 spheres")
        assert rend.launch_info()["spheres_active"] > 1023
    finally:
        rend.close()
    return out


def case_tile_16384_squared():
    """One 16 384 x 16 384 tile (tile_px x 16 = 2^32 bytes per sample row) over a 128 x 16 384 frame at 1 spp: the records of the tile's
    upper half lie beyond 2 GiB, those of its last row just below 4 GiB."""
    w, h, seed = 128, 16384, 6060
    p = params(w, h, 1, seed, tile_w=16384, tile_h=16384)
    rend = r1.Renderer(0)
    out = {}
    try:
        sc = r1.create_large_scene(w, h)
        rend.set_scene(sc)
        want = render(rend, p)
        same(passes(rend, p, [1]), want, "one pass")
        oracle_spots(sc, p, want[0], [(127, 16383), (0, 8192)])
        same(render_async(rend, p), want, "r1_render_async")
        b = batch_async(rend, p, 2, 1)
        same(b[0], want, "batch frame 0")
        same(b[1], render(rend, params(w, h, 1, seed + 1, tile_w=16384, tile_h=16384)), "batch frame 1")
        # the same frame in 32 x 32 tiles: the pixels do not depend on the tiling
        same(render(rend, params(w, h, 1, seed)), want, "32 x 32 tiles")
        rend.set_scene(r1.create_grid_scene(w, h, 40, 40))
        same(render(rend, p, land=True), passes(rend, p, [1]), "r1_render, 1 604 spheres")
        out["rays"] = want[1]
    finally:
        rend.close()
    return out


def case_sides_and_tilings():
    """65 535 x 1 and 1 x 65 535 frames (65 536 refused), 1 x 1 tiles, a 65 535 x 1 tile, and a frame whose LAND tile lists pass 2 GB."""
    rend = r1.Renderer(0)
    out = {}
    try:
        for w, h in ((65535, 1), (1, 65535)):
            p = params(w, h, 4, 777)
            rend.set_scene(r1.create_large_scene(w, h))
            want = passes(rend, p, [3, 1])
            same(render(rend, p), want, f"{w}x{h} r1_render")
            same(render_async(rend, p), want, f"{w}x{h} r1_render_async")
            same(sharded(rend, p, 3), want, f"{w}x{h} 3 shards")
            big = params(w + (w > 1), h + (h > 1), 4, 777)
            refused(lambda: rend.render(big), "exceeds 2^31 samples")
            refused_async(rend, big, "exceeds 2^31 samples")
        # a tile as wide as the frame, one row high
        w, h = 65535, 3
        rend.set_scene(r1.create_large_scene(w, h))
        want = render(rend, params(w, h, 3, 55))
        same(render(rend, params(w, h, 3, 55, tile_w=65535, tile_h=1)), want, "65535 x 1 tiles")
        same(render_async(rend, params(w, h, 3, 55, tile_w=65535, tile_h=1)), want, "65535 x 1 tiles, async")
        # one pixel per tile
        w = h = 256
        rend.set_scene(r1.create_large_scene(w, h))
        want = render(rend, params(w, h, 2, 56))
        one = params(w, h, 2, 56, tile_w=1, tile_h=1)
        assert binding.tile_count(one) == (65536, 65536)
        same(render(rend, one), want, "1 x 1 tiles")
        same(render_async(rend, one), want, "1 x 1 tiles, async")
        same(sharded(rend, one, 3), want, "1 x 1 tiles, 3 shards")
        # 1.2 M tiles of 1 x 1 in flight need > 2 GB of tile lists: refused there, rendered synchronously
        w, h = 1200, 1000
        rend.set_scene(r1.create_large_scene(w, h))
        want = render(rend, params(w, h, 1, 57))
        one = params(w, h, 1, 57, tile_w=1, tile_h=1)
        same(render(rend, one), want, "1.2 M tiles of 1 x 1, r1_render")
        refused_async(rend, one, "tile lists")
        same(render_async(rend, params(w, h, 1, 57)), want, "r1_render_async after the refusal")
    finally:
        rend.close()
    return out


def case_wavefront_cap():
    """R1_VARIANT_WAVEFRONT keeps every path in memory up to 2^24 slots: 512 x 512 x 64 renders, x 65 is refused."""
    w, h = 512, 512
    rend = r1.Renderer(0)
    try:
        rend.set_scene(r1.create_large_scene(w, h))
        want = render(rend, params(w, h, 64, 31))
        same(render(rend, params(w, h, 64, 31, variant=binding.VARIANT_WAVEFRONT), kernel=binding.VARIANT_WAVEFRONT), want, "wavefront")
        refused(lambda: rend.render(params(w, h, 65, 31, variant=binding.VARIANT_WAVEFRONT)), "> 2^24")
        same(render(rend, params(w, h, 64, 31, variant=binding.VARIANT_WAVEFRONT), kernel=binding.VARIANT_WAVEFRONT), want, "wavefront again")
    finally:
        rend.close()
    return {}


def case_seeds():
    """Seeds 0 and 0xFFFFFFFF against the oracle, whole frames; a 4-frame batch from 0xFFFFFFF0 with stride 7 wraps mod 2^32 at its last
    frame (seed 5), and every frame equals r1_render at its wrapped seed (host frames and device records)."""
    w, h, spp = 96, 64, 4
    sc = r1.create_large_scene(w, h)
    sa = r1o.SceneArrays.from_c(sc.spheres, sc.camera)
    rend = r1.Renderer(0)
    try:
        rend.set_scene(sc)
        for seed in (0, 0xFFFFFFFF):
            oimg, orays = r1o.render_frame(sa, r1o.make_params(w, h, spp, seed))[:2]
            same(render(rend, params(w, h, spp, seed)), (oimg, orays), f"seed {seed:#x} vs the oracle")
        first, stride, n = 0xFFFFFFF0, 7, 4
        seeds = [(first + stride * f) % 2 ** 32 for f in range(n)]
        assert seeds[-1] == 5
        want = [render(rend, params(w, h, spp, s)) for s in seeds]
        oimg, orays = r1o.render_frame(sa, r1o.make_params(w, h, spp, 5))[:2]
        same(want[-1], (oimg, orays), "seed 5 vs the oracle")
        for f, got in enumerate(batch_async(rend, params(w, h, spp, first), n, stride)):
            same(got, want[f], f"batch frame {f} (seed {seeds[f]:#x})")
        for f, got in enumerate(batch_device_records(rend, params(w, h, spp, first), n, stride)):
            same(got, want[f], f"device records batch frame {f} (seed {seeds[f]:#x})")
    finally:
        rend.close()
    return {"seeds": seeds}


CASES = {"ceiling_frame": case_ceiling_frame, "ceiling_exact": case_ceiling_exact, "ceiling_batch": case_ceiling_batch}
CASES.update({f"tile4g_{spp}": (lambda s: lambda: _tile4g(s))(spp) for spp in TILE4G_SPPS})
CASES.update({"tile_16384_squared": case_tile_16384_squared, "sides_and_tilings": case_sides_and_tilings,
              "wavefront_cap": case_wavefront_cap, "seeds": case_seeds})

_timed_out = []


@pytest.mark.parametrize("case", list(CASES))
def test_limits(case):
    if _timed_out:
        pytest.skip(f"case {_timed_out[0]} ran out of time: no more launches from this file")
    env = dict(os.environ)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), case]
    try:
        res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _timed_out.append(case)
        raise AssertionError(f"{case}: no result within {CHILD_TIMEOUT_S} s")
    stdout, stderr = res.stdout.decode(errors="replace"), res.stderr.decode(errors="replace")
    assert res.returncode == 0, f"child exit {res.returncode}\n{stdout[-3000:]}\n{stderr[-3000:]}"
    summary = json.loads(stdout.strip().splitlines()[-1])
    print(json.dumps(summary))
    assert summary["ok"] and summary["case"] == case


if __name__ == "__main__":
    name = sys.argv[1] if len(sys.argv) > 1 else None
    try:
        t = time.perf_counter()
        result = CASES[name]()
        result.update(case=name, ok=True, case_s=time.perf_counter() - t)
        print(json.dumps(result))
    except BaseException as ex:  # the first mismatch, a missing refusal (pytest.raises) or an unexpected one ends the case
        print(json.dumps({"case": name, "ok": False, "error": f"{type(ex).__name__}: {ex}"}))
        sys.exit(1)
