"""Frames in flight through the tiles-summed-in-the-trace-kernel path (R1_LAND) at the shapes bench.py times, and one
context through every change of state around it, refused calls included.

Every frame gets a seed of its own, lands in a target filled with 0xCD first (pixels and count word), and must equal r1_render of its seed
on a separate reference context, every byte of the image and the ray count exactly.  For the large scene r1_render is the latency kernel
followed by a resolve launch (no tile is summed inside the trace launch), so the reference takes another path; for the 100 004-sphere
scene r1_render would take the LAND kernel too, so its reference is the exhaustive sweep (R1_VARIANT_PREFILTER) with a resolve launch.
A frame that never lands, or that lands from a stale launch, keeps the sentinel or another seed's pixels and fails here.

The shapes bench.py times run in a child process with bench's hardware-queue count (GPU_MAX_HW_QUEUES=20, bench.py QUEUES_SINGLE): the
pytest process gets 4 queues, so no more than 4 of its launches overlap.  `python tests/test_gpu_inflight.py CASE` runs one case
alone (R1_TEST_LIB selects another build of the library, as in tests/conftest.py) and prints a JSON summary.
"""
import ctypes as C
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
from rays1bench_amd import binding

pytestmark = pytest.mark.gpu

SENTINEL = 0xCD
CHILD_QUEUES = "20"  # bench.py QUEUES_SINGLE: the queue count of the timed run
CHILD_TIMEOUT_S = 300


class _Record:
    """Record i of a HostFrames as the target of Renderer.render_async (pixels, then the uint64 count at rays_offset)."""

    def __init__(self, hf, i):
        self.ptr, self.rays_offset = hf.ptr + i * hf.record, hf.rays_offset


def _mismatch(img, rays, want):
    """None if (img, rays) equal want = (image, rays); else what differs."""
    if rays == want[1] and img.tobytes() == want[0].tobytes():
        return None
    return {"rays": int(rays), "want_rays": int(want[1]), "pixels_differing": int((img != want[0]).any(axis=2).sum()),
            "pixels_at_sentinel": int((img == SENTINEL).all(axis=2).sum()), "pixels": int(img.shape[0] * img.shape[1])}


# ---- 1a: the timed configuration, in a child process --------------------------------------------------------------------------------

# case: (scene, width, height, spp, slots, launches per slot, frames per launch)
CASES = {
    "tree_10spp": ("large", 1200, 800, 10, 20, 3, 1),      # bench.py's headline: 20 slots, here 3 launches each without a fence
    "tree_250spp": ("large", 1200, 800, 250, 20, 1, 1),    # BASELINE config 4: ~3.9 GB of records per context
    "big_config5": ("config5", 480, 270, 4, 4, 2, 1),      # BASELINE config 5's 100 004 spheres on a crop
    "batch_10spp": ("large", 1200, 800, 10, 10, 1, 2),     # r1_render_batch_async, 2 frames per launch, seed_stride 1
}


def _child(case):
    """One case of 1a: the slots are built as bench.py's Slot (one Renderer, one torch stream, one set of page-locked frames each), every
    launch is queued on its slot's stream, one fence, then every frame is compared.  Returns the summary; raises at the first mismatch."""
    import torch
    kind, w, h, spp, n_slots, rounds, per_launch = CASES[case]
    scene = r1.create_grid_scene(w, h, 400, 250) if kind == "config5" else r1.create_large_scene(w, h)
    ref_variant = binding.VARIANT_PREFILTER if kind == "config5" else binding.VARIANT_DEFAULT
    summary = {"case": case, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "shape": [w, h, spp], "slots": n_slots,
               "launches_per_slot": rounds, "frames_per_launch": per_launch}
    t_case = time.perf_counter()

    class Slot:
        def __init__(self):
            self.rend = r1.Renderer(0)
            self.rend.set_scene(scene)
            self.host = binding.HostFrames(w, h, rounds * per_launch)
            self.host._all[:] = SENTINEL
            self.stream = torch.cuda.Stream()

        def close(self):
            self.rend.close()
            self.host.close()

    slots = [Slot() for _ in range(n_slots)]
    ref = r1.Renderer(0)
    try:
        ref.set_scene(scene)
        # every frame's seed: frame f of launch rnd of slot k (distinct across slots, launches and frames of a batch)
        seed = {(k, rnd, f): 7919 + 1000 * rnd + per_launch * k + f for k in range(n_slots) for rnd in range(rounds) for f in range(per_launch)}
        assert len(set(seed.values())) == len(seed)
        timed = case == "tree_10spp"
        if timed:
            # setup, as bench.py's: workspace allocated and each stream's hardware queue opened before the launches that are timed
            # (a synchronous frame on the context's own stream is no LAND launch: the three launches below start the cursor sets afresh)
            for k, sl in enumerate(slots):
                sl.rend.render(r1.make_params(w, h, spp, 3 + k))
                with torch.cuda.stream(sl.stream):
                    torch.zeros(1, device="cuda").add_(1)
                sl.rend.timing_begin(rounds)
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for rnd in range(rounds):
            for k, sl in enumerate(slots):
                p = r1.make_params(w, h, spp, seed[(k, rnd, 0)])
                if per_launch == 1:
                    sl.rend.render_async(p, _Record(sl.host, rnd), sl.stream.cuda_stream)
                else:
                    sl.rend.render_batch_async(p, per_launch, _Record(sl.host, rnd * per_launch), 1, sl.stream.cuda_stream)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        for sl in slots:
            sl.rend.sync()  # r1_sync: land_check, so a launch whose resolver gave up fails here
            info = sl.rend.launch_info()
            assert info["tiles_in_kernel"] == 1, info
            if kind == "config5":
                assert info["spheres_active"] > 1023 and info["kernel"] == binding.VARIANT_BVH, info
        if timed:
            trace_ms = 0.0
            for sl in slots:
                a, _, n = sl.rend.timing_end()
                assert n == rounds, n
                trace_ms += a
            summary["launch_overlap"] = trace_ms * 1e-3 / wall  # bench.py's launch_overlap: per-launch device time / wall time
        summary["wall_ms"] = wall * 1e3
        frames = 0
        for rnd in range(rounds):
            for k, sl in enumerate(slots):
                for f in range(per_launch):
                    sd = seed[(k, rnd, f)]
                    img, rays, _ = ref.render(r1.make_params(w, h, spp, sd, variant=ref_variant))
                    assert ref.launch_info()["tiles_in_kernel"] == 0  # the reference path sums no tile inside its trace launch
                    i = rnd * per_launch + f
                    bad = _mismatch(sl.host.image(i), sl.host.rays(i), (img, rays))
                    if bad:
                        bad.update(case=case, slot=k, launch=rnd, frame_of_launch=f, seed=sd)
                        raise AssertionError(json.dumps(bad))
                    frames += 1
        summary["frames"] = frames
    finally:
        for sl in slots:
            sl.close()
        ref.close()
    summary["case_s"] = time.perf_counter() - t_case
    return summary


@pytest.mark.parametrize("case", list(CASES))
def test_frames_in_flight_at_the_timed_shapes(case):
    """1a: bench.py's frames in flight with bench's queue count, in a fresh child process; every frame equal to its reference."""
    n_slots, rounds, per_launch = CASES[case][4:]
    env = dict(os.environ)
    env["GPU_MAX_HW_QUEUES"] = CHILD_QUEUES
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), case]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, timeout=CHILD_TIMEOUT_S)
    stdout, stderr = out.stdout.decode(errors="replace"), out.stderr.decode(errors="replace")
    assert out.returncode == 0, f"child exit {out.returncode}\n{stdout[-3000:]}\n{stderr[-3000:]}"
    summary = json.loads(stdout.strip().splitlines()[-1])
    print(json.dumps(summary))
    assert summary["ok"] and summary["case"] == case
    assert summary["gpu_max_hw_queues"] == CHILD_QUEUES
    assert summary["frames"] == n_slots * rounds * per_launch
    if case == "tree_10spp":
        assert summary["launch_overlap"] > 2, summary  # the frames really were in flight together


# ---- 1b: one context through every state change ------------------------------------------------------------------------------------


def test_one_context_through_every_state_change_and_refusal():
    """One context renders LAND frames (R1_LAND: tiles summed in the trace launch) around every other kind of call it can get, a new
    seed at each step, each rendered frame checked against its reference: the two cursor sets alternating, pageable targets (LAND
    into the device image, then two copies), an unaligned count pointer (the copy path), a frame with no target, a grid frame (resolve
    launch), calls refused before the LAND state is touched, and a call refused after it was: the tile lists of a frame that need more
    than 2 GB.  A refusal must leave the context as it found it — the next frame must not take the cursor set the last launch exhausted."""
    w, h, spp = 320, 200, 6
    L = binding.lib()
    rend, ref = r1.Renderer(0), r1.Renderer(0)
    hf = binding.HostFrames(w, h, 1)
    seeds = iter(range(30011, 30111))
    try:
        sc = r1.create_large_scene(w, h)
        rend.set_scene(sc)
        ref.set_scene(sc)

        def want(p):
            img, rays, _ = ref.render(p)
            return img, rays

        def check(img, rays, p, step, land=True):
            assert rend.launch_info()["tiles_in_kernel"] == (1 if land else 0), step
            bad = _mismatch(img, rays, want(p))
            assert bad is None, (step, p.seed, bad)

        def land_frame(step):
            p = r1.make_params(w, h, spp, next(seeds))
            hf._all[:] = SENTINEL
            rend.render_async(p, hf)
            rend.sync()
            check(hf.image(0).copy(), hf.rays(0), p, step)

        # 1. page-locked targets, twice: the second launch takes the other cursor set
        land_frame("1a")
        land_frame("1b")
        # 2. pageable numpy buffers through the C-ABI: LAND into the context's device image, then the two copies the header promises
        p = r1.make_params(w, h, spp, next(seeds))
        img = np.full((h, w, 3), SENTINEL, np.uint8)
        cnt = np.full(1, 0xCDCDCDCDCDCDCDCD, np.uint64)
        binding._check(L.r1_render_async(rend._c, C.byref(p), img.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         cnt.ctypes.data_as(C.POINTER(C.c_uint64)), None))
        rend.sync()
        check(img, int(cnt[0]), p, "2 pageable")
        land_frame("2 after")
        # 3. a page-locked image with a count pointer that is not 8-byte aligned: the copy path
        p = r1.make_params(w, h, spp, next(seeds))
        pad = (w * h * 3 + 7) & ~7
        blk = C.c_void_p()
        binding._check(L.r1_host_alloc(pad + 16, C.byref(blk)))
        raw = None
        try:
            raw = np.frombuffer((C.c_uint8 * (pad + 16)).from_address(blk.value), np.uint8)
            raw[:] = SENTINEL
            binding._check(L.r1_render_async(rend._c, C.byref(p), C.cast(blk.value, C.POINTER(C.c_uint8)),
                                             C.cast(blk.value + pad + 1, C.POINTER(C.c_uint64)), None))
            rend.sync()
            got = raw.copy()  # (checked below, after the block is freed: no view of freed memory may reach a traceback)
        finally:
            raw = None
            L.r1_host_free(blk)
        check(got[:w * h * 3].reshape(h, w, 3), int(got[pad + 1:pad + 9].view(np.uint64)[0]), p, "3 unaligned count")
        assert (got[w * h * 3:pad + 1] == SENTINEL).all() and (got[pad + 9:] == SENTINEL).all()
        land_frame("3 after")
        # 4. a frame with no target stays on the device (and leaves the last target alone), then async again
        hf._all[:] = SENTINEL
        rend.render_frame_device(r1.make_params(w, h, spp, next(seeds)))
        rend.sync()
        assert rend.launch_info()["tiles_in_kernel"] == 1
        assert (hf._all == SENTINEL).all()
        land_frame("4 after")
        # 5. a grid frame (a resolve launch, not LAND), then the tree again
        p = r1.make_params(w, h, spp, next(seeds), variant=binding.VARIANT_GRID)
        hf._all[:] = SENTINEL
        rend.render_async(p, hf)
        rend.sync()
        assert rend.launch_info()["kernel"] == binding.VARIANT_GRID
        check(hf.image(0).copy(), hf.rays(0), p, "5 grid", land=False)
        land_frame("5 after")
        land_frame("5 after, other set")
        # 6. refusals before any LAND state is touched: a sharded frame, a batch beyond 2^31 sample slots
        with pytest.raises(r1.R1Error) as e:
            rend.render_async(r1.make_params(w, h, spp, next(seeds), shard=0, num_shards=2), hf)
        assert e.value.code == binding.R1_EINVAL
        with pytest.raises(r1.R1Error) as e:
            rend.render_batch_async(r1.make_params(1024, 1024, 1000, next(seeds)), 3, None)  # 3 x 1.05 G slots
        assert e.value.code == binding.R1_ELIMIT
        land_frame("6 after")
        # 7. a refusal after the LAND state was committed: 1200x1000 frames of 1x1 tiles at 1 spp are 1.2 M tiles; in flight they get 128
        #    workgroups (R1_MIN_BLOCKS) x 4 waves, and every wave a list row as long as the launch has tiles: 128 x 4 x 1.2 M x 4 B = 2.4 GB
        #    > 2 GB.  A synchronous frame of that shape first, so the counter allocation has grown before (growing it would reset the
        #    context's LAND state and hide the fault)
        bw, bh = 1200, 1000
        big = r1.make_params(bw, bh, 1, next(seeds), tile_w=1, tile_h=1)
        rend.render(big)
        land_frame("7 before")
        bhf = binding.HostFrames(bw, bh, 1)
        try:
            with pytest.raises(r1.R1Error) as e:
                rend.render_async(r1.make_params(bw, bh, 1, next(seeds), tile_w=1, tile_h=1), bhf)
            assert e.value.code == binding.R1_ELIMIT and "tile lists" in str(e.value), str(e.value)
        finally:
            bhf.close()
        land_frame("7 first after the refusal")
        land_frame("7 second after the refusal")
    finally:
        hf.close()
        rend.close()
        ref.close()


# ---- 1c: recycled page-locked memory -------------------------------------------------------------------------------------------------


def test_contexts_on_recycled_page_locked_memory_render_and_sync():
    """r1_create's 64-byte page-locked word block carries land_check's "a resolver gave up" flag (word 2): a context must start with it
    clear.  Blocks of that size are filled with 0xFF and freed first, then several contexts each render and sync one LAND frame.
    This only fails where the runtime hands such a block back to r1_create; on a runtime that never recycles them it passes either way."""
    w, h, spp = 160, 96, 3
    L = binding.lib()
    freed = []
    for _ in range(48):
        blk = C.c_void_p()
        binding._check(L.r1_host_alloc(64, C.byref(blk)))
        C.memset(blk, 0xFF, 64)
        freed.append(blk)
    for blk in freed:
        L.r1_host_free(blk)
    sc = r1.create_large_scene(w, h)
    ref = r1.Renderer(0)
    rends = [r1.Renderer(0) for _ in range(8)]
    hfs = [binding.HostFrames(w, h, 1) for _ in rends]
    try:
        ref.set_scene(sc)
        for k, (r_, hf) in enumerate(zip(rends, hfs)):
            r_.set_scene(sc)
            p = r1.make_params(w, h, spp, 40503 + k)
            hf._all[:] = SENTINEL
            r_.render_async(p, hf)
            r_.sync()
            assert r_.launch_info()["tiles_in_kernel"] == 1
            img, rays, _ = ref.render(p)
            bad = _mismatch(hf.image(0), hf.rays(0), (img, rays))
            assert bad is None, (k, bad)
    finally:
        for r_, hf in zip(rends, hfs):
            r_.close()
            hf.close()
        ref.close()


if __name__ == "__main__":
    try:
        result = _child(sys.argv[1])
        result["ok"] = True
        print(json.dumps(result))
    except Exception as ex:  # the first mismatch (or a refused call) ends the case
        print(json.dumps({"case": sys.argv[1] if len(sys.argv) > 1 else None, "ok": False, "error": f"{type(ex).__name__}: {ex}"}))
        sys.exit(1)
