// r1_tile.h — the tile geometry of a frame, once, for the host and the device: a frame is cut into tiles of tile_w x tile_h pixels, numbered row by
// row; the last column and row of tiles may be cut by the image's edge.  Work is laid out over PADDED tiles (tile_w * tile_h slots each, slot = ly *
// tile_w + lx), so an edge tile has void slots.  Shard `shard` of `num_shards` owns tiles shard, shard + num_shards, ...: its local tile lt is tile
// shard + lt * num_shards.  A pixel is stored row-major in the image or, for a shard, in its dense block: [local tile][ly][lx].
// Plain C++: the closing kernels (r1_close_kernels.hip), the host steps (r1_frame.cpp, r1_render.cpp) and tools/check_tile_host.cpp read the same
// lines.  The integer widths are the kernels': tile numbers and slots are uint32 (< 2^31, r1_frame.cpp prepare_tiles), addresses are size_t.
// The trace kernel's own resolver (r1_land.hpp) keeps its copy of the rect rule: its arguments are R1TraceArgs'.
#ifndef R1_TILE_H
#define R1_TILE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define R1_TILE_HD __host__ __device__ __forceinline__
#else
#define R1_TILE_HD inline
#endif

struct R1TileGeom { int32_t width, height, tile_w, tile_h, tiles_x; };
R1_TILE_HD R1TileGeom r1_tile_geom(const int32_t width, const int32_t height, const int32_t tile_w, const int32_t tile_h)
{
    return {width, height, tile_w, tile_h, (width + tile_w - 1) / tile_w};
}
R1_TILE_HD int32_t r1_tiles_y(const R1TileGeom &g) { return (g.height + g.tile_h - 1) / g.tile_h; }
R1_TILE_HD int32_t r1_tiles(const R1TileGeom &g) { return g.tiles_x * r1_tiles_y(g); }
R1_TILE_HD uint32_t r1_tile_slots(const R1TileGeom &g) { return (uint32_t)(g.tile_w * g.tile_h); } // of a padded tile

// the shard rule, its inverse for a tile of the frame, and the tiles a shard owns of `total`
R1_TILE_HD uint32_t r1_shard_tile(const int32_t shard, const uint32_t lt, const int32_t num_shards) { return (uint32_t)shard + lt * (uint32_t)num_shards; }
R1_TILE_HD int r1_tile_shard(const int tile, const int num_shards) { return tile % num_shards; }
R1_TILE_HD int r1_tile_local(const int tile, const int num_shards) { return tile / num_shards; }
R1_TILE_HD uint32_t r1_shard_tiles(const int32_t total, const int32_t shard, const int32_t num_shards)
{
    return total > shard ? (uint32_t)((total - shard + num_shards - 1) / num_shards) : 0u;
}

// tile `tile` of the frame: its corner and its size inside the image; the tile that holds pixel (x, y)
struct R1TileRect { int x0, y0, tw, th; };
R1_TILE_HD R1TileRect r1_tile_rect(const R1TileGeom &g, const uint32_t tile)
{
    const int x0 = (int)(tile % (uint32_t)g.tiles_x) * g.tile_w;
    const int y0 = (int)(tile / (uint32_t)g.tiles_x) * g.tile_h;
    return {x0, y0, g.tile_w < g.width - x0 ? g.tile_w : g.width - x0, g.tile_h < g.height - y0 ? g.tile_h : g.height - y0};
}
R1_TILE_HD int r1_tile_at(const R1TileGeom &g, const int x, const int y) { return (y / g.tile_h) * g.tiles_x + (x / g.tile_w); }

// slot `pix` of the padded tile -> (lx, ly); false: a void slot of an edge tile
R1_TILE_HD bool r1_tile_pixel(const R1TileGeom &g, const R1TileRect &r, const uint32_t pix, int *lx, int *ly)
{
    *ly = (int)(pix / (uint32_t)g.tile_w);
    *lx = (int)(pix - (uint32_t)*ly * (uint32_t)g.tile_w);
    return *lx < r.tw && *ly < r.th;
}

// where pixel (lx, ly) of a tile is stored, in pixels: the row-major image, the dense block of the shard whose local tile lt it is
R1_TILE_HD size_t r1_pixel_row_major(const R1TileGeom &g, const R1TileRect &r, const int lx, const int ly) { return (size_t)(r.y0 + ly) * g.width + (r.x0 + lx); }
R1_TILE_HD size_t r1_pixel_block(const R1TileGeom &g, const uint32_t lt, const int lx, const int ly) { return ((size_t)lt * g.tile_h + (size_t)ly) * g.tile_w + lx; }

#endif
