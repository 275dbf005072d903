"""GPU route map of the launches that close a frame (rays1bench_amd/csrc/r1_close_kernels.hip, the tile geometry of r1_tile.h): every route
below renders the reference's own ragged frame, tests/golden/frame_medium_77x45x3.bin (image and ray count; the seed is in its header), on
create_medium_scene(77, 45), with tiles of 16x8 (5 x 6 tiles, the last column 13 wide, the last row 5 high) and of 40x24 (2 x 2 tiles, so
that shard 4 of 5 has none).  Bit for bit: the bytes and the count of the fixture, nothing else.

  render                      the resolve launch of a synchronous frame (r1_resolve_kernel), variants BVH, PREFILTER, GRID
  render_async                a frame in flight into a HostFrame: the ragged countdowns r1_land_arm_kernel sets
  render_pass                 passes of 1 and 2 samples (r1_accum_kernel): the second preview is the frame
  render_adaptive, rule off   three listed passes of 1 sample (r1_adapt_accum_kernel, r1_adapt_compact_kernel): every tile reports 3 samples
  shards, single frames       render_shard_device for every shard of 3 and of 5, r1_assemble_kernel over the records
  shards, batches             the same in batches of two frames, PREFILTER (r1_batch_counts_kernel's partial sums; the zero counts of a
                              shard without tiles) and BVH"""
import os

import pytest
import torch

import rays1bench_amd as r1
from rays1bench_amd import binding
import r1o

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_medium_77x45x3.bin")
TILES = [(16, 8), (40, 24)]
SHARDS = (3, 5)


@pytest.fixture(scope="module")
def fixture():
    g = r1o.read_golden(GOLD)
    w, h, spp, seed = g["hdr"].tolist()
    assert (w, h, spp) == (77, 45, 3)
    return w, h, spp, seed, g["image"].tobytes(), int(g["rays"][0])


@pytest.fixture(scope="module")
def renderer(fixture):
    assert r1.device_count() >= 1, "no HIP device: the product has no CPU fallback"
    r = r1.Renderer(0)
    r.set_scene(r1.create_medium_scene(fixture[0], fixture[1]))
    yield r
    r.close()


def params(fixture, tile, spp=None, **k):
    w, h, n, seed = fixture[:4]
    return r1.make_params(w, h, n if spp is None else spp, seed, tile_w=tile[0], tile_h=tile[1], **k)


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("variant", ["BVH", "PREFILTER", "GRID"])
def test_render_resolves_the_fixture(renderer, fixture, tile, variant):
    img, rays, _ = renderer.render(params(fixture, tile, variant=getattr(binding, "VARIANT_" + variant)))
    assert rays == fixture[5] and img.tobytes() == fixture[4]


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_render_async_lands_the_fixture(renderer, fixture, tile):
    hf = binding.HostFrame(fixture[0], fixture[1])
    try:
        renderer.render_async(params(fixture, tile), hf)
        renderer.sync()
        assert hf.rays == fixture[5] and hf.image.tobytes() == fixture[4]
    finally:
        hf.close()


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_passes_of_one_and_two_samples_accumulate_the_fixture(renderer, fixture, tile):
    renderer.render_pass(params(fixture, tile, spp=1), 0)
    img, rays = renderer.render_pass(params(fixture, tile, spp=2), 1)
    assert rays == fixture[5] and img.tobytes() == fixture[4]


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_adaptive_with_the_rule_off_samples_the_fixture(renderer, fixture, tile):
    img, rays, tiles, res = renderer.render_adaptive(params(fixture, tile), 1, 1, -1, 0)
    assert (tiles["spp"] == 3).all() and (tiles["settled"] == 0).all() and res["passes"] == 3
    assert res["samples"] == 3 * fixture[0] * fixture[1]
    assert rays == fixture[5] and img.tobytes() == fixture[4]


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("shards", SHARDS)
def test_shards_assemble_to_the_fixture(renderer, fixture, tile, shards):
    w, h = fixture[:2]
    p0 = params(fixture, tile, shard=0, num_shards=shards)
    rec = binding.shard_record_bytes(p0)
    records = torch.full((shards, rec), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for s in range(shards):
        renderer.render_shard_device(params(fixture, tile, shard=s, num_shards=shards), records[s].data_ptr(), records[s].data_ptr() + rec - 8, st)
    pad = (w * h * 3 + 7) & ~7
    out = torch.zeros(pad + 8, dtype=torch.uint8, device="cuda")
    renderer.assemble_device_records(p0, records.data_ptr(), out.data_ptr(), out.data_ptr() + pad, st)
    torch.cuda.synchronize()
    assert int(out[pad:].view(torch.int64).item()) == fixture[5]
    assert out[:w * h * 3].cpu().numpy().tobytes() == fixture[4]
    if tile == (40, 24) and shards == 5:  # four tiles: the fifth shard has none
        assert int(records[4, rec - 8:].view(torch.int64).item()) == 0


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("variant", ["PREFILTER", "BVH"])
def test_batches_of_shards_assemble_to_the_fixture_twice(renderer, fixture, tile, shards, variant):
    w, h = fixture[:2]
    v = getattr(binding, "VARIANT_" + variant)
    p0 = params(fixture, tile, shard=0, num_shards=shards, variant=v)
    rec, frec = binding.shard_record_bytes(p0), binding.frame_record_bytes(p0)
    gathered = torch.full((shards, 2, rec), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for s in range(shards):
        renderer.render_shard_device_batch(params(fixture, tile, shard=s, num_shards=shards, variant=v), 2, gathered[s].data_ptr(), seed_stride=0, stream_ptr=st)
    frames = torch.zeros((2, frec), dtype=torch.uint8, device="cuda")
    renderer.assemble_device_records_batch(p0, 2, gathered.data_ptr(), frames.data_ptr(), st)
    torch.cuda.synchronize()
    for f in range(2):
        assert int(frames[f, frec - 8:].view(torch.int64).item()) == fixture[5], f
        assert frames[f, :w * h * 3].cpu().numpy().tobytes() == fixture[4], f
        if tile == (40, 24) and shards == 5:
            assert int(gathered[4, f, rec - 8:].view(torch.int64).item()) == 0, f
