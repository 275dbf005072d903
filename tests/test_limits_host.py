"""CPU tests of the host arithmetic at the C-ABI's 32-bit limits (no GPU): the unpadded sample limit of r1_params_check (w * h * spp <
2^31, sides <= 65535), and the byte sizes of records, frames and multi-device layouts at shapes whose sizes pass 2^32 bytes.  Every expected
value is computed here with Python integers, so a size that wraps in 32 bits on the C side fails.  The padded-slot limit of a launch
(tile_w * tile_h * spp * tiles < 2^31) needs a context: tests/test_gpu_limits.py."""
import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

# the shapes tests/test_gpu_limits.py renders at the one-launch ceiling
CEILING_FRAMES = [(1920, 1080, 1028), (2040, 1020, 1023), (2048, 1024, 1023), (65535, 1, 1), (1, 65535, 1), (65535, 32767, 1)]


def _tiles(n, t):
    return (n + t - 1) // t


def _refused(p, text="exceeds 2^31 samples"):
    with pytest.raises(r1.R1Error) as e:
        binding.tile_count(p)
    assert e.value.code == binding.R1_ELIMIT and text in str(e.value), str(e.value)
    assert binding.frame_record_bytes(p) == 0 and binding.shard_record_bytes(p) == 0 and binding.shard_block_bytes(p) == 0


def test_sample_limit_is_w_h_spp_below_2_31():
    assert binding.tile_count(r1.make_params(2048, 1024, 1023)) == (64 * 32, 64 * 32)
    _refused(r1.make_params(2048, 1024, 1024))                      # exactly 2^31
    _refused(r1.make_params(1024, 1024, 2048))
    _refused(r1.make_params(46341, 46341, 1))                       # 2^31 + 50 873 pixels at one sample
    assert binding.tile_count(r1.make_params(46340, 46340, 1)) == (1449 * 1449, 1449 * 1449)
    _refused(r1.make_params(65535, 32769, 1))
    # the unpadded count decides here: 65535 x 32768 x 1 is 2^31 - 32 768 samples, although its 32 x 32 tiles hold 2^31 slots
    assert binding.tile_count(r1.make_params(65535, 32768, 1)) == (2048 * 1024, 2048 * 1024)
    # spp at the top of int32: one pixel
    assert binding.tile_count(r1.make_params(1, 1, 2 ** 31 - 1)) == (1, 1)


@pytest.mark.parametrize("w,h", [(65535, 1), (1, 65535), (65535, 2), (65535, 32767)])
def test_sides_up_to_65535_pixels(w, h):
    p = r1.make_params(w, h, 1)
    assert binding.tile_count(p) == (_tiles(w, 32) * _tiles(h, 32),) * 2
    _refused(r1.make_params(65536, h, 1))
    _refused(r1.make_params(w, 65536, 1))
    _refused(r1.make_params(h, 65536, 1))


def test_tile_counts_of_extreme_tilings():
    # 1 x 1 tiles: one tile per pixel, up to 2^31 - 1 of them
    assert binding.tile_count(r1.make_params(256, 256, 1, tile_w=1, tile_h=1)) == (65536, 65536)
    assert binding.tile_count(r1.make_params(65535, 32767, 1, tile_w=1, tile_h=1)) == (65535 * 32767,) * 2
    assert binding.tile_count(r1.make_params(65535, 32767, 1, tile_w=1, tile_h=1, shard=6, num_shards=7)) == (65535 * 32767, _tiles(65535 * 32767, 7))
    # one tile larger than the frame, and a 65535 x 1 tile
    assert binding.tile_count(r1.make_params(100, 100, 3, tile_w=16384, tile_h=16384)) == (1, 1)
    assert binding.tile_count(r1.make_params(65535, 4, 7, tile_w=65535, tile_h=1)) == (4, 4)


@pytest.mark.parametrize("w,h,spp", CEILING_FRAMES)
def test_record_bytes_at_the_ceiling_shapes(w, h, spp):
    for tw, th in ((32, 32), (1, 1), (128, 128), (65535, 1)):
        for shards in (1, 2, 3, 8):
            p = r1.make_params(w, h, spp, tile_w=tw, tile_h=th, shard=shards - 1, num_shards=shards)
            tiles = _tiles(w, tw) * _tiles(h, th)
            per = (tiles + shards - 1) // shards
            block = per * tw * th * 3
            assert binding.tile_count(p) == (tiles, per)
            assert binding.shard_block_bytes(p) == block, (w, h, tw, th, shards)
            assert binding.shard_record_bytes(p) == (block + 7) // 8 * 8 + 8, (w, h, tw, th, shards)
            assert binding.frame_record_bytes(p) == (w * h * 3 + 7) // 8 * 8 + 8


def test_record_bytes_past_4_gib():
    # the largest frame and blocks pass 2^32 bytes: a 32-bit size would have wrapped
    big = r1.make_params(65535, 32767, 1, tile_w=1, tile_h=1)
    assert binding.frame_record_bytes(big) == 6442156048 > 2 ** 32
    assert binding.shard_record_bytes(big) == 6442156048  # (1 x 1 tiles: the block is the image, pixel for pixel)
    assert binding.shard_record_bytes(r1.make_params(65535, 32767, 1, shard=1, num_shards=2)) == 1024 * 1024 * 3072 + 8
    assert binding.shard_record_bytes(r1.make_params(65535, 32767, 1)) == 2048 * 1024 * 3072 + 8 > 2 ** 32


@pytest.mark.parametrize("n_devices", [1, 2, 8])
@pytest.mark.parametrize("n_frames", [1, 3])
def test_multi_layout_of_a_ceiling_frame(n_devices, n_frames):
    w, h, spp = 1920, 1080, 1028
    L = binding.multi_layout(r1.make_params(w, h, spp), n_devices, n_frames)
    per = (60 * 34 + n_devices - 1) // n_devices       # 2040 tiles of 32 x 32
    block = per * 32 * 32 * 3
    record = (block + 7) // 8 * 8 + 8
    frame = w * h * 3 + 8                              # (6 220 800 is a multiple of 8)
    assert L == {"block_bytes": block, "record_bytes": record, "count_offset": record - 8, "send_bytes": record * n_frames,
                 "gathered_bytes": record * n_frames * n_devices, "frame_record_bytes": frame, "frame_count_offset": frame - 8,
                 "host_bytes": frame * n_frames, "counts_pitch": record * n_frames}
    assert binding.multi_layout(r1.make_params(65535, 32767, 1, tile_w=1, tile_h=1), n_devices, n_frames)["host_bytes"] == 6442156048 * n_frames
    with pytest.raises(r1.R1Error) as e:
        binding.multi_layout(r1.make_params(2048, 1024, 1024), n_devices, n_frames)
    assert e.value.code == binding.R1_EINVAL
