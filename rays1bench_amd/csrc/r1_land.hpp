// r1_land.hpp — tiles resolved inside the trace kernel (R1_LAND).  Internal linkage (anonymous namespace).
// The reference resolves a pixel where it traced it (rayweek1.cpp:762-775).  Here the samples of a pixel end on different lanes and
// waves, and their fp32 sum must run in sample order, so every sample still leaves a 16-byte record; but the records of a 32 x 32
// tile are summed by the waves of the trace launch itself, and the pixels go straight to where the frame is wanted (device memory or
// the caller's page-locked host buffer): no second launch waiting for workgroup slots behind persistent waves, no copy.
// What makes it cheap is that a tile never leaves its XCD.  The eight XCDs' L2s are not coherent with each other: records traced on
// one XCD and summed on another must be written through to memory (sc1 stores: +7 % on the tracing loop, measured) and waited for
// by workgroups that do nothing else (+14 %): profiles/r04/land_cross_xcd_cost_breakdown.txt, the first form of this code.  So:
//   * a tile belongs to the XCD that CLAIMS it: every XCD has a cursor {tile (or group of 8 tiles), next sample slot} its waves take their
//     chunks from; the wave that takes the last chunk (or finds nothing installed yet) claims the launch's next unclaimed tile(s) for its
//     XCD and installs it; waves that meet a used-up tile meanwhile wait for that (microseconds).  Nothing
//     is assumed about which XCD a workgroup runs on — the dispatcher deals them round-robin, starting wherever the last launch
//     stopped — and XCDs that run faster simply claim more tiles;
//   * the waves of an XCD store the records with plain stores and count the samples they finish per tile — in LDS, for the tiles of the
//     wave's current and previous chunk — and subtract the count from the tile's countdown when the wave moves on to another tile: one
//     fire-and-forget atomic per chunk (an atomic per finished sample group and iteration cost 7 %: the vector-memory counter of this
//     chip is in order, so every iteration's first load waited for the memory-side atomic in front of it; a returning one per chunk 3 %);
//   * a wave that has run out of work looks at the tiles it ever took a chunk from (a short list in its LDS row): a countdown at zero is
//     swapped for a mark, and the wave that wins the swap sums the tile — its records sit in this XCD's L2 or in memory, nowhere else —
//     adds the tile's rays to the frame's count and re-arms the countdown for the next launch.  Of the waves that worked on a tile the
//     last to get there finds it complete, so every tile is summed.  The wave that takes the frame's last tile off publishes the ray
//     count.  (The list: 24 entries in LDS, the rest in a row of global memory long enough for every tile of the launch.)
//   * every record carries the launch's tag in its ray-count word: a countdown is not ordered after the stores it counts, so a wave
//     that finds a record of an earlier launch in a tile it owes simply reads the tile again (past the vector L1: sc0 loads).
// Per launch, behind the queue pointer (one of two sets of queue heads, zeroed by the launch after; r1_device.h R1_HEAD_*): head x = XCD x's
// cursor (uint64); head R1_HEAD_DISPENSER = the launch's next unclaimed tile.
#ifndef R1_LAND_HPP
#define R1_LAND_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "r1_device.h"
#include "r1_dev_math.hpp"
#include "r1_sample.hpp" // fastdiv

#pragma clang fp contract(off)

namespace
{

#define R1_LAND_OWED 24u        // tiles of a wave's list kept in LDS (the rest: its row of the spill area in global memory)
#define R1_LAND_LOADS 8      // records of one pixel a lane keeps in flight while it sums a tile (4 registers each; 10 spill in the 72-register builds)

__device__ __forceinline__ uint32_t xcc_id() { return (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u; } // HW_REG_XCC_ID[3:0]

// What a wave knows about the tiles it works on — kept in LDS (a row of R1_LAND_ROW words per wave), NOT in registers: the tracing loop
// is at its register budget, and every wave-uniform value carried around it cost spilled scalar registers, whose lanes take a
// vector register from the loop (five such values: +6.5 % per frame, profiles/r04/land_xcd_local_steps.txt).
//   [0] t0, [1] n0: tile of the wave's current chunk, samples of it the wave has finished since it last subtracted
//   [2] t1, [3] n1: the same for the previous chunk's tile
//   [4] touched: tiles this wave has taken chunks from; [8 ...]: their indices (the first R1_LAND_OWED of them)
#define R1_LAND_ROW 32u
#define R1_LAND_CLAIMED 0xFFFFFFFFu

// the wave takes a chunk from tile t for the first time (or again): t goes on the list of tiles it looks at before it exits.  ONE lane.
__device__ __forceinline__ void land_note(const R1TraceArgs &A, uint32_t *row, const uint32_t t)
{
    const uint32_t at = row[4];
    row[4] = at + 1u;
    // (past R1_LAND_OWED the wave's row of the spill area, which has room for every tile of the launch: the XCD's cursor only moves
    //  forward, so a wave meets a tile at most once — however unevenly the launch's workgroups get their slots, the list cannot overflow)
    if (at < R1_LAND_OWED)
        row[8u + at] = t;
    else
    {
        // (32-bit index on a scalar base: as a 64-bit per-lane address the row's part of it is hoisted out of the tracing loop and spilled to scratch)
        uint32_t tx = threadIdx.x;
        asm volatile("" : "+v"(tx)); // (formed here, not hoisted)
        const uint32_t wave = blockIdx.x * (R1_BLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(tx >> 6));
        ((r1_gu32 *)A.land.owed_spill)[(size_t)wave * A.land.spill_stride + at] = t;
    }
}

// subtract n finished samples from tile t's countdown: fire and forget (a RETURNING atomic here — "who reaches zero owes the tile" —
// stalled the wave for a memory-side round trip at every chunk: +3 % per frame).  Who sums the tile is settled when waves exit.
__device__ __forceinline__ void land_flush(const R1TraceArgs &A, const uint32_t t, const uint32_t n)
{
    if (n == 0u)
        return;
    (void)__hip_atomic_fetch_sub(A.land_cnt + t * R1_LAND_CNT_STRIDE, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// this lane has just stored the record of sample slot k: one more finished sample of its tile.  Per lane, no wave-uniform state.
__device__ __forceinline__ void land_count(const R1TraceArgs &A, uint32_t *row, const uint32_t k)
{
    const uint32_t j = fastdiv(k, A.div_full); // tile of the launch: k = (j spp + s) tile_px + pix
    if (j == row[0])
        atomicAdd(&row[1], 1u); // (LDS)
    else if (j == row[2])
        atomicAdd(&row[3], 1u);
    else
        land_flush(A, j, 1u); // (rare: a path that outlived two chunks; its tile is on the wave's list since the chunk was taken)
}

// the wave's next chunk comes from tile t.  ONE lane.
__device__ __forceinline__ void land_chunk(const R1TraceArgs &A, uint32_t *row, const uint32_t t)
{
    const uint32_t t0 = row[0];
    if (t == t0)
        return;
    land_flush(A, row[2], row[3]);
    row[2] = t0, row[3] = row[1];
    row[0] = t, row[1] = 0u;
    land_note(A, row, t);
}

// One tile of the launch (t = frame * n_local_tiles + local tile) by ONE wave, lane l taking pixels l, l + 64, ...: false if a record
// did not carry the launch's tag (nothing is accounted then; pixels written from such a pass are overwritten by the pass that
// succeeds — the host sees the buffer only after the kernel).  Same arithmetic and order as r1_resolve_kernel = rayweek1.cpp:762-775.
template <int LOADS /* records of one pixel a lane keeps in flight: 4 registers each */>
__device__ __forceinline__ bool land_resolve_tile(const R1TraceArgs &A, const uint32_t t, const int lane)
{
    const R1LandArgs &L = A.land;
    const uint32_t f = t / A.n_local_tiles, lt = t - f * A.n_local_tiles;
    const uint32_t tile = (uint32_t)A.shard + lt * (uint32_t)A.num_shards;
    const uint32_t ty = tile / (uint32_t)A.tiles_x, tx = tile - ty * (uint32_t)A.tiles_x;
    const int x0 = (int)tx * A.tile_w, y0 = (int)ty * A.tile_h;
    const int tw = min(A.tile_w, A.width - x0), th = min(A.tile_h, A.height - y0);
    const uint32_t tile_px = (uint32_t)(A.tile_w * A.tile_h);
    // the tile's records [s][pixel], read with sc0 loads (buffer form: 16 bytes at once): they must come from the L2, not from this CU's
    // vector L1 — a pass that meets a record whose store is still on its way would otherwise find the same stale line again.
    // A tile's records can span 4 GiB and more (tile_px * spp < 2^31 records of 16 bytes), beyond what a buffer's 32-bit range and offset
    // reach: every load gets a descriptor of its own, based (64-bit address) at the wave's 64 pixels of that sample, and an offset < 1 KiB
    const float4 *const recs = A.samples + (size_t)t * A.full;
    constexpr int SC0 = 1;
    typedef uint32_t land_u4 __attribute__((ext_vector_type(4)));
    uint8_t *const out = L.out + (size_t)f * L.out_stride;
    const uint32_t spp = (uint32_t)A.spp;
    uint32_t bad = 0;
    unsigned long long rays = 0;
    for (uint32_t p0 = 0; p0 < tile_px; p0 += 64u) // (wave-uniform: the descriptors below stay in SGPRs)
    {
        const uint32_t pix = p0 + (uint32_t)lane;
        const int ly = (int)(pix / (uint32_t)A.tile_w), lx = (int)(pix - (uint32_t)ly * (uint32_t)A.tile_w);
        if (pix >= tile_px || lx >= tw || ly >= th)
            continue; // void slots of an edge tile
        const int range = (int)(min(64u, tile_px - p0) * 16u); // (a load outside the tile reads zeros, never a neighbour's records)
        float cr = 0, cg = 0, cb = 0;
        for (uint32_t s0 = 0; s0 < spp; s0 += LOADS)
        {
            const uint32_t n = min((uint32_t)LOADS, spp - s0); // (wave-uniform)
            const float4 *const row = recs + (size_t)s0 * tile_px + p0;
            land_u4 v[LOADS];
#pragma unroll
            for (uint32_t u = 0; u < LOADS; ++u)
                if (u < n)
                {
                    const __amdgpu_buffer_rsrc_t rec = __builtin_amdgcn_make_buffer_rsrc((void *)(row + (size_t)u * tile_px), 0, range, 0x00020000);
                    v[u] = __builtin_amdgcn_raw_buffer_load_b128(rec, lane * 16, 0, SC0);
                }
#pragma unroll
            for (uint32_t u = 0; u < LOADS; ++u)
                if (u < n)
                {
                    cr += __uint_as_float(v[u].x), cg += __uint_as_float(v[u].y), cb += __uint_as_float(v[u].z); // col += color(...) rayweek1.cpp:762
                    bad |= (v[u].w & ~255u) ^ A.land_tag;
                    rays += v[u].w & 255u;
                }
        }
        cr *= L.inv_spp, cg *= L.inv_spp, cb *= L.inv_spp;
        cr = ieee_sqrt(cr), cg = ieee_sqrt(cg), cb = ieee_sqrt(cb);
        const size_t o = L.block_layout ? ((size_t)lt * tile_px + pix) * 3 : ((size_t)(y0 + ly) * A.width + (x0 + lx)) * 3;
        out[o + 0] = (uint8_t)(int)(cr * 255.99f);
        out[o + 1] = (uint8_t)(int)(cg * 255.99f);
        out[o + 2] = (uint8_t)(int)(cb * 255.99f);
    }
    if (__ballot(bad != 0u))
        return false;
    for (int off = 32; off > 0; off >>= 1)
        rays += __shfl_down(rays, off, 64);
    if (lane == 0)
    {
        __hip_atomic_store(A.land_cnt + t * R1_LAND_CNT_STRIDE, (uint32_t)(tw * th) * spp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // re-armed for the next launch
        // the tile's rays, then one tile less to go: the second atomic is issued only when the first has been performed, so whoever
        // takes the frame's last tile off finds every tile's rays added — and publishes the count (rayweek1.cpp:809-813)
        const unsigned long long before = __hip_atomic_fetch_add(L.frame_rays + f, rays, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::"v"(before));
        const uint32_t left = __hip_atomic_fetch_sub(L.frame_left + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left == 1u)
        {
            const unsigned long long total = __hip_atomic_exchange(L.frame_rays + f, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *(L.rays_in_out ? (unsigned long long *)(out + L.rays_offset) : L.rays_dst) = total;
            __hip_atomic_store(L.frame_left + f, A.n_local_tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // as the next launch expects it
        }
    }
    return true;
}

// A tracing wave has run out of work: it subtracts what it still holds, then looks at every tile it ever took a chunk from.  A countdown
// at zero means every sample of the tile has been counted; the wave that swaps the zero for the CLAIMED mark sums the tile.  Every tile
// finds its wave: of the waves that worked on a tile, the last to get here has seen all the others subtract (they waited for their
// atomics before they looked), so it reads zero unless another wave already has the tile.
template <int LOADS>
__device__ __forceinline__ void land_exit(const R1TraceArgs &A, uint32_t *row, const int lane)
{
    if (lane == 0)
    {
        land_flush(A, row[2], row[3]);
        land_flush(A, row[0], row[1]);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): this wave's record stores, subtractions and spilled list entries have been performed
    __builtin_amdgcn_wave_barrier();
    const uint32_t touched = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[4]);
    for (uint32_t base = 0; base < touched; base += 64u) // (wave-uniform; one trip unless the list spilled)
    {
        const uint32_t i = base + (uint32_t)lane;
        uint32_t t = 0u, c = 1u;
        if (i < touched)
        {
            if (i < R1_LAND_OWED)
            {
                t = row[8u + i];
                asm volatile("" : "+v"(t)); // (two loads kept apart: a select between an LDS and a global address becomes a generic load)
            }
            else
            {
                const uint32_t wave = blockIdx.x * (R1_BLOCK / 64) + (threadIdx.x >> 6);
                t = ((const r1_gu32 *)A.land.owed_spill)[(size_t)wave * A.land.spill_stride + i];
            }
            // (device scope: the countdowns are only ever touched by atomics, which are performed behind the L2s)
            c = __hip_atomic_load(A.land_cnt + t * R1_LAND_CNT_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c == 0u) // every lane that reads zero tries for its tile; one wave of the XCD wins it
            {
                uint32_t seen = 0u;
                if (!__hip_atomic_compare_exchange_strong(A.land_cnt + t * R1_LAND_CNT_STRIDE, &seen, R1_LAND_CLAIMED, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT))
                    c = 1u;
            }
        }
        unsigned long long mine = __ballot(c == 0u);
        while (mine)
        {
            const int b = __ffsll((long long)mine) - 1;
            mine &= mine - 1ull;
            const uint32_t tt = (uint32_t)__builtin_amdgcn_readlane((int)t, b);
            // a record whose store is still on its way (the countdown is not ordered after the stores) shows an old tag: read again
            uint32_t tries = 0;
            while (!land_resolve_tile<LOADS>(A, tt, lane))
                if (++tries == R1_LAND_MAX_WAIT)
                {
                    if (lane == 0 && A.land.error)
                        *A.land.error = 1u; // never in a correct run; the host reports the launch as failed
                    break;
                }
        }
    }
}

} // namespace

#endif // R1_LAND_HPP
