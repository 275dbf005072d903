"""CPU test of the tile geometry the closing kernels and the host share (rays1bench_amd/csrc/r1_tile.h): a stand-alone program
(tools/check_tile_host.cpp) compiles the header for the host and compares it with the rules written out from the pixel's side in 64-bit
arithmetic.

Every width and height in 1..40 x every tile_w and tile_h in 1..9, and the tiles 16x8 and 40x24, x num_shards 1, 3, 5 = 398 400 cases.  In
each: the tiles' rects partition the image; the slot walk of a tile visits each of its pixels inside the image once and no void slot; the
row-major addresses of the frame are a permutation of 0 .. w*h-1; the shards' tiles are disjoint and cover the frame (shards without a
tile included); a shard's dense-block addresses are distinct and inside r1_shard_block_bytes.  Then the first and last tile of the shapes at
the 32-bit limits (tests/test_limits_host.py, tests/test_gpu_limits.py) against the 64-bit restatement.  Zero mismatches, and the exact
number of cases, tiles and pixels: nothing is skipped silently."""
import os
import subprocess

import pytest

import rays1bench_amd as r1
from rays1bench_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = range(1, 41)
TILES = [(tw, th) for tw in range(1, 10) for th in range(1, 10)] + [(16, 8), (40, 24)]
SHARDS = (1, 3, 5)


def _compile(src_root, exe):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(src_root, "tools", "check_tile_host.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    c = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    c["returncode"] = out.returncode
    return c, out.stderr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(ROOT, str(tmp_path_factory.mktemp("tile") / "check_tile_host"))


def test_the_header_is_the_written_out_rule_in_every_case(exe):
    c, _ = _run(exe)
    tiles = lambda n, t: (n + t - 1) // t  # noqa: E731
    assert c["cases"] == 40 * 40 * 83 * 3 == len(SIDES) ** 2 * len(TILES) * len(SHARDS)
    assert c["tiles"] == len(SHARDS) * sum(tiles(w, tw) * tiles(h, th) for w in SIDES for h in SIDES for tw, th in TILES)
    assert c["pixels"] == len(SHARDS) * len(TILES) * sum(SIDES) ** 2
    assert c["void_slots"] == len(SHARDS) * sum(tiles(w, tw) * tiles(h, th) * tw * th - w * h for w in SIDES for h in SIDES for tw, th in TILES) > 0
    assert c["empty_shards"] == sum(max(0, ns - tiles(w, tw) * tiles(h, th)) for w in SIDES for h in SIDES for tw, th in TILES for ns in SHARDS) > 0
    assert c["limit_cases"] == 4 * len(SHARDS)
    assert c["mismatches"] == 0 and c["returncode"] == 0, c


@pytest.mark.parametrize("w,h,tw,th,ns", [(77, 45, 16, 8, 3), (77, 45, 40, 24, 5), (65535, 32767, 1, 1, 5), (40000, 40000, 16384, 16384, 3)])
def test_the_programs_block_size_is_r1_shard_block_bytes(exe, w, h, tw, th, ns):
    c, _ = _run(exe, "block", str(w), str(h), str(tw), str(th), str(ns))
    assert c["block_bytes"] == binding.shard_block_bytes(r1.make_params(w, h, 1, tile_w=tw, tile_h=th, shard=ns - 1, num_shards=ns)) > 0


@pytest.mark.parametrize("what", ["rect", "void", "shard"])
def test_the_program_reports_a_wrong_rule(tmp_path, what):
    """The comparison can fail: the same program over a header whose edge tiles are not cut, whose slot walk admits the column behind a cut
    tile, and whose shards own one tile too few."""
    src = open(os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_tile.h")).read()
    good, bad = {"rect": ("g.tile_w < g.width - x0 ? g.tile_w : g.width - x0", "g.tile_w"),
                 "void": ("return *lx < r.tw && *ly < r.th;", "return *lx <= r.tw && *ly < r.th;"),
                 "shard": ("(total - shard + num_shards - 1) / num_shards", "(total - shard) / num_shards")}[what]
    assert src.count(good) == 1
    os.makedirs(tmp_path / "rays1bench_amd" / "csrc")
    os.makedirs(tmp_path / "tools")
    (tmp_path / "rays1bench_amd" / "csrc" / "r1_tile.h").write_text(src.replace(good, bad))
    (tmp_path / "tools" / "check_tile_host.cpp").write_text(open(os.path.join(ROOT, "tools", "check_tile_host.cpp")).read())
    c, err = _run(_compile(str(tmp_path), str(tmp_path / "wrong")))
    assert c["returncode"] == 1 and "MISMATCH" in err and c["mismatches"] > 1000
