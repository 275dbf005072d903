// tools/check_tile_host.cpp — runs rays1bench_amd/csrc/r1_tile.h on the host (tests/test_tile_host.py) against the tile rules written out here in
// 64-bit arithmetic, from the pixel's side: pixel (x, y) lies in tile (y / tile_h) * ceil(width / tile_w) + x / tile_w, at (x % tile_w, y % tile_h).
//   check_tile_host            every width and height in 1..40 x every tile_w and tile_h in 1..9, and the tiles 16x8 and 40x24, x num_shards 1, 3, 5;
//                              then the first and last tile of the shapes at the 32-bit limits
//   check_tile_host block W H TILE_W TILE_H NUM_SHARDS    prints the bytes this program takes for a shard's dense block (r1_shard_block_bytes' rule)
// Prints "name value" lines; exit status 1 and "MISMATCH ..." lines on stderr (the first few) where the two sides differ.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../rays1bench_amd/csrc/r1_tile.h"

static unsigned long long mismatches = 0;
static void report(const char *what, const long long w, const long long h, const long long tw, const long long th, const long long ns, const long long at)
{
    if (mismatches++ < 10)
        fprintf(stderr, "MISMATCH %s %lldx%lld tiles %lldx%lld shards %lld at %lld\n", what, w, h, tw, th, ns, at);
}

// ---- the rules, restated ----
static int64_t ceil_div(const int64_t a, const int64_t b) { return (a + b - 1) / b; }
struct Rect64
{
    int64_t x0, y0, x1, y1; // [x0, x1) x [y0, y1)
};
static Rect64 rect_of(const int64_t w, const int64_t h, const int64_t tw, const int64_t th, const int64_t tile)
{
    const int64_t col = tile % ceil_div(w, tw), row = tile / ceil_div(w, tw);
    Rect64 r = {col * tw, row * th, (col + 1) * tw, (row + 1) * th};
    if (r.x1 > w)
        r.x1 = w;
    if (r.y1 > h)
        r.y1 = h;
    return r;
}
// r1_shard_block_bytes (r1_host.cpp): every shard's block has room for the most tiles a shard can own
static int64_t block_bytes(const int64_t w, const int64_t h, const int64_t tw, const int64_t th, const int64_t ns)
{
    return ceil_div(ceil_div(w, tw) * ceil_div(h, th), ns) * tw * th * 3;
}

static bool same_rect(const R1TileRect &a, const Rect64 &b) { return a.x0 == b.x0 && a.y0 == b.y0 && a.x0 + a.tw == b.x1 && a.y0 + a.th == b.y1; }

static unsigned long long cases = 0, tiles_seen = 0, pixels_seen = 0, void_slots = 0, empty_shards = 0;

static void one_case(const int w, const int h, const int tw, const int th, const int ns)
{
    ++cases;
    const R1TileGeom g = r1_tile_geom(w, h, tw, th);
    const int64_t total = ceil_div(w, tw) * ceil_div(h, th);
    if (g.tiles_x != ceil_div(w, tw) || r1_tiles_y(g) != ceil_div(h, th) || r1_tiles(g) != total || r1_tile_slots(g) != (uint32_t)(tw * th))
        report("counts", w, h, tw, th, ns, 0);
    // the rects partition the image; a tile's slot walk visits each of its pixels once and no void slot; the row-major addresses are a permutation
    std::vector<int> owner((size_t)w * h, -1), visits((size_t)w * h, 0), addressed((size_t)w * h, 0);
    for (int64_t t = 0; t < total; ++t)
    {
        ++tiles_seen;
        const R1TileRect r = r1_tile_rect(g, (uint32_t)t);
        const Rect64 want = rect_of(w, h, tw, th, t);
        if (!same_rect(r, want) || r.tw < 1 || r.th < 1)
            report("rect", w, h, tw, th, ns, t);
        for (int64_t y = want.y0; y < want.y1; ++y)
            for (int64_t x = want.x0; x < want.x1; ++x)
            {
                if (owner[(size_t)(y * w + x)] != -1 || r1_tile_at(g, (int)x, (int)y) != t)
                    report("partition", w, h, tw, th, ns, y * w + x);
                owner[(size_t)(y * w + x)] = (int)t;
            }
        for (int64_t pix = 0; pix < (int64_t)tw * th; ++pix)
        {
            int lx = -1, ly = -1;
            const bool inside = r1_tile_pixel(g, r, (uint32_t)pix, &lx, &ly);
            const int64_t x = want.x0 + pix % tw, y = want.y0 + pix / tw;
            if (inside != (x < w && y < h) || lx != pix % tw || ly != pix / tw)
                report("slot", w, h, tw, th, ns, pix);
            if (!inside)
            {
                ++void_slots;
                continue;
            }
            ++pixels_seen;
            const size_t a = r1_pixel_row_major(g, r, lx, ly);
            if ((int64_t)a != y * w + x || a >= (size_t)w * h)
            {
                report("row-major", w, h, tw, th, ns, pix);
                continue;
            }
            ++visits[a], ++addressed[a];
        }
    }
    for (size_t i = 0; i < (size_t)w * h; ++i)
        if (owner[i] < 0 || visits[i] != 1 || addressed[i] != 1)
            report("cover", w, h, tw, th, ns, (long long)i);
    // the shards' tiles are disjoint and cover the frame; a shard's dense-block addresses are distinct and inside its block
    std::vector<int> shard_of((size_t)total, -1);
    const int64_t bytes = block_bytes(w, h, tw, th, ns);
    for (int s = 0; s < ns; ++s)
    {
        const uint32_t local = r1_shard_tiles((int32_t)total, s, ns);
        int64_t want_local = 0;
        for (int64_t t = s; t < total; t += ns)
            ++want_local;
        if (local != want_local)
            report("shard tiles", w, h, tw, th, ns, s);
        if (!local)
            ++empty_shards;
        std::vector<char> used((size_t)(bytes / 3), 0);
        for (uint32_t lt = 0; lt < local; ++lt)
        {
            const uint32_t tile = r1_shard_tile(s, lt, ns);
            if (tile >= total || shard_of[tile] != -1 || r1_tile_shard((int)tile, ns) != s || r1_tile_local((int)tile, ns) != (int)lt)
            {
                report("shard rule", w, h, tw, th, ns, tile);
                continue;
            }
            shard_of[tile] = s;
            const R1TileRect r = r1_tile_rect(g, tile);
            for (int ly = 0; ly < r.th; ++ly)
                for (int lx = 0; lx < r.tw; ++lx)
                {
                    const size_t a = r1_pixel_block(g, lt, lx, ly);
                    if ((int64_t)a != ((int64_t)lt * th + ly) * tw + lx || (int64_t)a * 3 + 3 > bytes || used[a])
                    {
                        report("block", w, h, tw, th, ns, (long long)a);
                        continue;
                    }
                    used[a] = 1;
                }
        }
    }
    for (int64_t t = 0; t < total; ++t)
        if (shard_of[(size_t)t] < 0)
            report("shards cover", w, h, tw, th, ns, t);
}

// the first and the last tile of a frame at the 32-bit limits: rect, corner pixels' addresses, the shard rule
static unsigned long long limit_cases = 0;
static void limit_case(const int w, const int h, const int tw, const int th, const int ns)
{
    ++limit_cases;
    const R1TileGeom g = r1_tile_geom(w, h, tw, th);
    const int64_t total = ceil_div(w, tw) * ceil_div(h, th);
    if (r1_tiles(g) != total)
        report("limit counts", w, h, tw, th, ns, 0);
    const int64_t ends[2] = {0, total - 1};
    for (const int64_t t : ends)
    {
        const R1TileRect r = r1_tile_rect(g, (uint32_t)t);
        const Rect64 want = rect_of(w, h, tw, th, t);
        if (!same_rect(r, want))
            report("limit rect", w, h, tw, th, ns, t);
        const int64_t s = t % ns, lt = t / ns;
        if (r1_shard_tile((int32_t)s, (uint32_t)lt, ns) != t || r1_tile_shard((int)t, ns) != s || r1_tile_local((int)t, ns) != lt ||
            lt >= r1_shard_tiles((int32_t)total, (int32_t)s, ns))
            report("limit shard", w, h, tw, th, ns, t);
        const int64_t slots[2] = {0, (want.y1 - want.y0 - 1) * tw + (want.x1 - want.x0 - 1)}; // the tile's first and last pixel inside the image
        for (const int64_t pix : slots)
        {
            int lx = -1, ly = -1;
            if (!r1_tile_pixel(g, r, (uint32_t)pix, &lx, &ly) || lx != pix % tw || ly != pix / tw)
                report("limit slot", w, h, tw, th, ns, pix);
            if ((int64_t)r1_pixel_row_major(g, r, lx, ly) != (want.y0 + ly) * (int64_t)w + want.x0 + lx)
                report("limit row-major", w, h, tw, th, ns, pix);
            const int64_t a = (int64_t)r1_pixel_block(g, (uint32_t)lt, lx, ly);
            if (a != (lt * th + ly) * tw + lx || a * 3 + 3 > block_bytes(w, h, tw, th, ns))
                report("limit block", w, h, tw, th, ns, pix);
        }
        if (r.tw < tw || r.th < th) // an edge tile: the slot behind its last column, or its last row, is void
        {
            int lx, ly;
            const int64_t pix = r.tw < tw ? r.tw : (int64_t)r.th * tw;
            if (r1_tile_pixel(g, r, (uint32_t)pix, &lx, &ly))
                report("limit void", w, h, tw, th, ns, pix);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc == 7 && argv[1][0] == 'b')
    {
        printf("block_bytes %lld\n", (long long)block_bytes(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6])));
        return 0;
    }
    const int shards[3] = {1, 3, 5};
    for (int w = 1; w <= 40; ++w)
        for (int h = 1; h <= 40; ++h)
            for (const int ns : shards)
            {
                for (int tw = 1; tw <= 9; ++tw)
                    for (int th = 1; th <= 9; ++th)
                        one_case(w, h, tw, th, ns);
                one_case(w, h, 16, 8, ns);
                one_case(w, h, 40, 24, ns);
            }
    for (const int ns : shards)
    {
        limit_case(65535, 32767, 1, 1, ns);       // 2^31 - 98 303 tiles of one pixel
        limit_case(100, 100, 16384, 16384, ns);   // one tile of 2^28 slots
        limit_case(40000, 40000, 16384, 16384, ns); // nine of them, the last column and row cut
        limit_case(65535, 4, 65535, 1, ns);       // tiles of one row
    }
    printf("cases %llu\ntiles %llu\npixels %llu\nvoid_slots %llu\nempty_shards %llu\nlimit_cases %llu\nmismatches %llu\n", cases, tiles_seen, pixels_seen,
           void_slots, empty_shards, limit_cases, mismatches);
    return mismatches ? 1 : 0;
}
