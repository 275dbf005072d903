// r1_close_kernels.hip — the kernels that close a frame behind the trace launch (resolve, region resolve, linear resolve and read-out, progressive accumulate, adaptive
// accumulate and compact, batch counts, assemble, landing arm, variance resolve) and their launchers, called from r1_frame.cpp and r1_render.cpp.  The tile geometry is
// r1_tile.h's; quantise_pixel is the trace kernels' (r1_sample.hpp).  The trace kernel's own resolver: r1_land.hpp.
#include "r1_sample.hpp"
#include "r1_internal.h"

namespace
{

// The closing prologue, by the launch's first workgroup behind the trace kernel (the caller says which: `first_workgroup && C.rays_src`): publish
// the ray count the trace kernel accumulated in the context's counter block, then zero the block for the next frame — two memset launches per
// frame less.
__device__ __forceinline__ void close_prologue(const R1FrameClose &C)
{
    static_assert(R1_COUNTER_BYTES == 256 * 16, "one 16-byte store per thread zeroes the counter block");
    if (threadIdx.x == 0)
        *C.rays_dst = *C.rays_src;
    __syncthreads();
    if (C.reset)
        ((uint4 *)C.reset)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

// One pixel's records of a tile, added in sample order to the sums the caller starts (0.0f, or an accumulator): s = the pixel's first record, the
// samples tile_px records apart ([tile][sample][pixel]).  each(i, record): what else a kernel takes from sample i's record.
struct Nothing { __device__ void operator()(int, const float4 &) const {} };
template <class Each = Nothing>
__device__ __forceinline__ void sum_records(const float4 *s, const uint32_t tile_px, const int spp, float &cr, float &cg, float &cb, Each each = Each())
{
    for (int i = 0; i < spp; ++i)
    {
        const float4 v = s[(size_t)i * tile_px];
        cr += v.x, cg += v.y, cb += v.z; // col += color(...) rayweek1.cpp:762
        each(i, v);
    }
}

// The four-wave reduction of a 256-thread workgroup, in two steps around the caller's __syncthreads() (a kernel that reduces two values pays one
// barrier): every wave's result into part[wave], then the four parts combined.  Integers: the order of the reduction cannot matter.
template <class T, class Op> __device__ __forceinline__ void reduce_waves(T v, T *part, Op op)
{
    for (int off = 32; off > 0; off >>= 1)
        v = op(v, (T)__shfl_down(v, off, 64));
    if ((threadIdx.x & 63u) == 0)
        part[threadIdx.x >> 6] = v;
}
template <class T, class Op> __device__ __forceinline__ T reduce_parts(const T *part, Op op) { return op(op(op(part[0], part[1]), part[2]), part[3]); }
struct Sum { template <class T> __device__ T operator()(const T a, const T b) const { return a + b; } };
struct Max { template <class T> __device__ T operator()(const T a, const T b) const { return max(a, b); } };

} // namespace

// Resolve: one thread per pixel of this shard; sums the spp samples in sample order and
// quantises exactly as rayweek1.cpp:765-775.
__global__ void __launch_bounds__(256) r1_resolve_kernel(const R1ResolveArgs A)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && A.close.rays_src)
        close_prologue(A.close);
    const uint32_t tiles_stride = gridDim.y;
    const uint32_t tiles_all = A.n_local_tiles * (A.n_frames ? A.n_frames : 1u);
    const uint32_t tile_px = r1_tile_slots(A.geom);
    for (uint32_t lt_all = blockIdx.y; lt_all < tiles_all; lt_all += tiles_stride)
    {
        const uint32_t f = lt_all / A.n_local_tiles, lt = lt_all - f * A.n_local_tiles; // frame of the batch, its local tile
        uint8_t *const out = A.out + (size_t)f * A.out_stride;
        const R1TileRect rect = r1_tile_rect(A.geom, r1_shard_tile(A.shard, lt, A.num_shards));
        const uint32_t base = lt_all * A.full;
        unsigned long long rays = 0;
        for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < tile_px; pix += gridDim.x * blockDim.x)
        {
            int lx, ly;
            if (!r1_tile_pixel(A.geom, rect, pix, &lx, &ly))
                continue; // void slots of an edge tile
            float cr = 0, cg = 0, cb = 0;
            sum_records(A.samples + base + pix, tile_px, A.spp, cr, cg, cb, [&](int, const float4 &v) { rays += __float_as_uint(v.w); });
            uint8_t r, g, b;
            quantise_pixel(cr, cg, cb, A.inv_spp, r, g, b);
            const size_t o = (A.block_layout ? r1_pixel_block(A.geom, lt, lx, ly) : r1_pixel_row_major(A.geom, rect, lx, ly)) * 3;
            out[o + 0] = r, out[o + 1] = g, out[o + 2] = b;
        }
        if (A.frame_rays) // frame batches: the frame's ray count is the sum over its samples (rayweek1.cpp:809-813)
        {
            // no atomics: 15 000 waves adding to one word per frame cost more than the whole resolve (a returning or
            // non-returning atomic on ONE line sustains ~88 M/s on this chip, tools/ubench_atomic.hip).  Every workgroup
            // stores ONE partial sum per tile it touches; r1_batch_counts_kernel adds them up per frame.
            __shared__ unsigned long long s_part[4];
            reduce_waves(rays, s_part, Sum());
            __syncthreads();
            if (threadIdx.x == 0)
                A.frame_rays[(size_t)lt_all * gridDim.x + blockIdx.x] = reduce_parts(s_part, Sum());
            __syncthreads();
        }
    }
}

// Linear frames (r1_render_linear*): one more launch behind a whole frame's trace and whatever closes it.  The resolve's
// indexing and its sums — 0.0f plus the records' x, y, z in sample order — times inv_spp, the first line of quantise_pixel, stored as
// three floats per pixel.  The w word is not used: a landing launch leaves its tag there.
__global__ void __launch_bounds__(256) r1_resolve_linear_kernel(const R1LinearArgs A)
{
    const uint32_t tile_px = r1_tile_slots(A.geom);
    for (uint32_t lt = blockIdx.y; lt < A.n_tiles; lt += gridDim.y)
    {
        const R1TileRect rect = r1_tile_rect(A.geom, lt);
        for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < tile_px; pix += gridDim.x * blockDim.x)
        {
            int lx, ly;
            if (!r1_tile_pixel(A.geom, rect, pix, &lx, &ly))
                continue; // void slots of an edge tile
            float cr = 0, cg = 0, cb = 0;
            sum_records(A.samples + (size_t)lt * A.full + pix, tile_px, A.spp, cr, cg, cb);
            float *const o = A.out + r1_pixel_row_major(A.geom, rect, lx, ly) * 3;
            o[0] = cr * A.inv_spp, o[1] = cg * A.inv_spp, o[2] = cb * A.inv_spp; // col *= 1 / spp rayweek1.cpp:765
        }
    }
}

// Region renders (r1_render_region*): in place of the resolve launch behind a launch of r1_region_kernel.  The resolve's walk over
// [tile][sample][pixel] records with the region's own tile geometry — void slots of its edge tiles skipped — and the resolve's sums; the pixel goes
// to (y * stride + x) of the caller's window as bytes (quantise_pixel), as floats (its first line: the sum times inv_spp), or both.  Nothing
// between the rows is written.  The w word is not read: the trace launch counted its rays itself, and the prologue publishes that count.
__global__ void __launch_bounds__(256) r1_resolve_region_kernel(const R1RegionArgs A)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && A.close.rays_src)
        close_prologue(A.close);
    const uint32_t tile_px = r1_tile_slots(A.geom);
    for (uint32_t lt = blockIdx.y; lt < A.n_tiles; lt += gridDim.y)
    {
        const R1TileRect rect = r1_tile_rect(A.geom, lt);
        for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < tile_px; pix += gridDim.x * blockDim.x)
        {
            int lx, ly;
            if (!r1_tile_pixel(A.geom, rect, pix, &lx, &ly))
                continue; // void slots of an edge tile
            float cr = 0, cg = 0, cb = 0;
            sum_records(A.samples + (size_t)lt * A.full + pix, tile_px, A.spp, cr, cg, cb);
            const size_t o = ((size_t)(rect.y0 + ly) * A.stride + (size_t)(rect.x0 + lx)) * 3;
            if (A.out_f32)
                A.out_f32[o + 0] = cr * A.inv_spp, A.out_f32[o + 1] = cg * A.inv_spp, A.out_f32[o + 2] = cb * A.inv_spp; // col *= 1 / spp rayweek1.cpp:765
            if (A.out_u8)
            {
                uint8_t r, g, b;
                quantise_pixel(cr, cg, cb, A.inv_spp, r, g, b);
                A.out_u8[o + 0] = r, A.out_u8[o + 1] = g, A.out_u8[o + 2] = b;
            }
        }
    }
}

// The read-out of the accumulators (r1_pass_linear, r1_render_adaptive_linear): r1_accum_kernel's indexing over the padded [tile][pixel]
// sums, each times (float)(1.0f / n) — n the same for every tile, or (A.report) the samples the tile's own report says it holds.
__global__ void __launch_bounds__(256) r1_accum_linear_kernel(const R1ReadoutArgs A)
{
    const uint32_t tile_px = r1_tile_slots(A.geom);
    for (uint32_t lt = blockIdx.y; lt < A.n_tiles; lt += gridDim.y)
    {
        const R1TileRect rect = r1_tile_rect(A.geom, lt);
        const float inv = A.report ? (float)(1.0f / A.report[lt].spp) : A.inv_n; // rayweek1.cpp:765 at the samples the sums hold
        for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < tile_px; pix += gridDim.x * blockDim.x)
        {
            int lx, ly;
            if (!r1_tile_pixel(A.geom, rect, pix, &lx, &ly))
                continue; // void slots of an edge tile
            const float4 a = A.accum[(size_t)lt * tile_px + pix];
            float *const o = A.out + r1_pixel_row_major(A.geom, rect, lx, ly) * 3;
            o[0] = a.x * inv, o[1] = a.y * inv, o[2] = a.z * inv;
        }
    }
}

// Progressive passes (r1_render_pass): in place of the resolve launch.  One thread per pixel of a padded tile, as the resolve: the
// accumulator (or 0.0f on the pass that starts the frame) plus the pass's records in sample order — the same sequence of fp32 adds the
// resolve of the whole frame makes — stored back, then quantised as the resolve does with n = first_sample + spp samples summed.
__global__ void __launch_bounds__(256) r1_accum_kernel(const R1AccumArgs A)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && A.close.rays_src)
        close_prologue(A.close); // the pass's ray count, the counter block zeroed for the next launch
    const uint32_t tile_px = r1_tile_slots(A.geom);
    for (uint32_t lt = blockIdx.y; lt < A.n_local_tiles; lt += gridDim.y)
    {
        const R1TileRect rect = r1_tile_rect(A.geom, lt);
        for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < tile_px; pix += gridDim.x * blockDim.x)
        {
            int lx, ly;
            if (!r1_tile_pixel(A.geom, rect, pix, &lx, &ly))
                continue; // void slots of an edge tile
            float4 *const acc = A.accum + (size_t)lt * tile_px + pix;
            float cr = 0, cg = 0, cb = 0;
            if (!A.fresh)
            {
                const float4 a = *acc;
                cr = a.x, cg = a.y, cb = a.z;
            }
            sum_records(A.samples + (size_t)lt * A.full + pix, tile_px, A.spp, cr, cg, cb);
            *acc = make_float4(cr, cg, cb, 0.0f);
            if (A.out)
            {
                uint8_t r, g, b;
                quantise_pixel(cr, cg, cb, A.inv_n, r, g, b);
                uint8_t *const o = A.out + r1_pixel_row_major(A.geom, rect, lx, ly) * 3;
                o[0] = r, o[1] = g, o[2] = b;
            }
        }
    }
}

// Adaptive sampling (r1_render_adaptive): in place of r1_accum_kernel after a pass over listed tiles.  Workgroup j serves list position j,
// i.e. tile list[j]: per pixel the `all` accumulator plus the pass's records in sample order, the `even` accumulator plus those of even
// GLOBAL sample index, both stored back (indexed by tile, so that they survive the list shrinking) and quantised as the resolve does; the
// `all` bytes go into the image; |byte_all - byte_even| over the tile's pixels inside the image and the three channels is reduced to its
// maximum and its sum — integers, so the order of the reduction cannot matter — and one lane tests the rule and writes the tile's report.
__global__ void __launch_bounds__(256) r1_adapt_accum_kernel(const R1AdaptArgs A)
{
    if (blockIdx.x == 0 && A.close.rays_src)
        close_prologue(A.close); // the pass's ray count, the counter block zeroed for the next launch
    __shared__ uint32_t s_max[4], s_sum[4];
    const uint32_t tile_px = r1_tile_slots(A.geom);
    for (uint32_t j = blockIdx.x; j < A.n_listed; j += gridDim.x)
    {
        const uint32_t tile = A.list[j];
        const R1TileRect rect = r1_tile_rect(A.geom, tile);
        uint32_t emax = 0, esum = 0;
        for (uint32_t pix = threadIdx.x; pix < tile_px; pix += blockDim.x)
        {
            int lx, ly;
            if (!r1_tile_pixel(A.geom, rect, pix, &lx, &ly))
                continue; // void slots of an edge tile
            float4 *const pa = A.all + (size_t)tile * tile_px + pix, *const pe = A.even + (size_t)tile * tile_px + pix;
            float ar = 0, ag = 0, ab = 0, er = 0, eg = 0, eb = 0;
            if (A.first_sample)
            {
                const float4 a = *pa, e = *pe;
                ar = a.x, ag = a.y, ab = a.z, er = e.x, eg = e.y, eb = e.z;
            }
            // [list position][sample][pixel]
            sum_records(A.samples + ((size_t)j * (uint32_t)A.spp) * tile_px + pix, tile_px, A.spp, ar, ag, ab, [&](int i, const float4 &v) {
                if (((A.first_sample + (uint32_t)i) & 1u) == 0u)
                    er += v.x, eg += v.y, eb += v.z;
            });
            *pa = make_float4(ar, ag, ab, 0.0f);
            *pe = make_float4(er, eg, eb, 0.0f);
            uint8_t r, g, b, r2, g2, b2;
            quantise_pixel(ar, ag, ab, A.inv_all, r, g, b);
            quantise_pixel(er, eg, eb, A.inv_even, r2, g2, b2);
            uint8_t *const o = A.out + r1_pixel_row_major(A.geom, rect, lx, ly) * 3;
            o[0] = r, o[1] = g, o[2] = b;
            const uint32_t dr = (uint32_t)abs((int)r - (int)r2), dg = (uint32_t)abs((int)g - (int)g2), db = (uint32_t)abs((int)b - (int)b2);
            emax = max(emax, max(dr, max(dg, db)));
            esum += dr + dg + db;
        }
        reduce_waves(emax, s_max, Max());
        reduce_waves(esum, s_sum, Sum());
        __syncthreads();
        if (threadIdx.x == 0)
        {
            emax = reduce_parts(s_max, Max());
            esum = reduce_parts(s_sum, Sum());
            const bool settled = (int32_t)emax <= A.max_delta &&
                                 (unsigned long long)esum * 256ull <= (unsigned long long)A.mean_delta_q8 * 3ull * (unsigned long long)(rect.tw * rect.th);
            R1TileReport rp;
            rp.spp = (int32_t)A.first_sample + A.spp, rp.settled = settled ? 1 : 0, rp.err_max = emax, rp.err_sum = esum;
            A.report[tile] = rp;
        }
        __syncthreads();
    }
}

// The next pass's list: the tiles of this pass's list that are still active — not settled, and (`at_cap` == 0) not at the cap — in the
// order they had, which is ascending; their number goes to *count_out (a page-locked host word, or device memory).  One workgroup: a wave
// places its tiles by ballot + prefix popcount, the four waves through LDS.  cur == null: every tile of the frame, in order (the first pass).
__global__ void __launch_bounds__(256) r1_adapt_compact_kernel(const uint32_t *cur, uint32_t n_cur, const R1TileReport *report, uint32_t at_cap,
                                                               uint32_t *next, uint32_t *count_out)
{
    __shared__ uint32_t s_cnt[4];
    uint32_t base = 0;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i0 = 0; i0 < n_cur; i0 += 256u)
    {
        const uint32_t i = i0 + threadIdx.x;
        uint32_t tile = 0;
        bool keep = false;
        if (i < n_cur)
        {
            tile = cur ? cur[i] : i;
            keep = cur ? (!at_cap && report[tile].settled == 0) : true;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0)
            s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; ++w)
            before += s_cnt[w];
        const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (keep)
            next[base + before + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = tile;
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0)
        *count_out = base;
}

// Frame batches: frame f's ray count = the sum of the partial sums the resolve launch left per (tile, workgroup column);
// one workgroup per frame; the count goes next to the frame's pixels (out + f * out_stride + rays_offset).
__global__ void __launch_bounds__(256)
    r1_batch_counts_kernel(const unsigned long long *__restrict__ partial, uint32_t per_frame, uint8_t *__restrict__ out, size_t out_stride,
                           size_t rays_offset)
{
    __shared__ unsigned long long s_part[4];
    const unsigned long long *src = partial + (size_t)blockIdx.x * per_frame;
    unsigned long long sum = 0;
    for (uint32_t i = threadIdx.x; i < per_frame; i += blockDim.x)
        sum += src[i];
    reduce_waves(sum, s_part, Sum());
    __syncthreads();
    if (threadIdx.x == 0)
        *(unsigned long long *)(out + (size_t)blockIdx.x * out_stride + rays_offset) = reduce_parts(s_part, Sum());
}

// Scatter gathered dense tile blocks (shard-major) into a row-major image.  Frame batches: blockIdx.y = frame; the
// frame's blocks start frame_in bytes after `blocks` (gathered layout [shard][frame][record]) and its image frame_out
// bytes after `rgb`.
__global__ void __launch_bounds__(256) r1_assemble_kernel(const R1AssembleArgs A)
{
    const uint8_t *__restrict__ blocks = A.blocks + (size_t)blockIdx.y * A.frame_in;
    uint8_t *__restrict__ rgb = A.rgb + (size_t)blockIdx.y * A.frame_out;
    // gathered RECORDS (block + uint64 count at the end of every record): the frame's ray count is the sum of the
    // shards' counts (rayweek1.cpp:809-813), written next to the image so that one copy brings both to the host
    if (A.want_total && blockIdx.x == 0 && threadIdx.x == 0)
    {
        unsigned long long sum = 0;
        for (int sh = 0; sh < A.num_shards; ++sh)
            sum += *(const unsigned long long *)(blocks + (size_t)sh * A.shard_stride + A.total_offset);
        *(unsigned long long *)(rgb + A.total_out) = sum;
    }
    const size_t n = (size_t)A.geom.width * A.geom.height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    {
        const int y = (int)(i / (size_t)A.geom.width), x = (int)(i - (size_t)y * A.geom.width);
        const int tile = r1_tile_at(A.geom, x, y);
        const size_t src = (size_t)r1_tile_shard(tile, A.num_shards) * A.shard_stride +
                           r1_pixel_block(A.geom, (uint32_t)r1_tile_local(tile, A.num_shards), x % A.geom.tile_w, y % A.geom.tile_h) * 3;
        const uint8_t r = blocks[src + 0], gr = blocks[src + 1], b = blocks[src + 2]; // (all three read before the first store: the pair loads and stores stay)
        rgb[3 * i + 0] = r, rgb[3 * i + 1] = gr, rgb[3 * i + 2] = b;
    }
}

// R1_LAND: the per-tile countdowns and per-frame accumulators of a context, set when its tiling changes (afterwards the resolvers
// re-arm what they consume): tile t of the launch lacks (valid pixels of its tile) x spp samples.
__global__ void __launch_bounds__(256) r1_land_arm_kernel(const R1LandArmArgs A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < A.n_frames)
        A.frame_rays[i] = 0ull, A.frame_left[i] = A.n_local_tiles;
    if (i >= A.n_frames * A.n_local_tiles)
        return;
    const R1TileRect rect = r1_tile_rect(A.geom, r1_shard_tile(A.shard, i % A.n_local_tiles, A.num_shards));
    A.tile_cnt[(size_t)i * R1_LAND_CNT_STRIDE] = (uint32_t)(rect.tw * rect.th * A.spp);
}

// Variance frames (r1_render_moments*): in place of r1_resolve_linear_kernel, with its indexing, tile walk and sums, so L has
// its bits.  Then the pixel's records once more in sample order (they come from cache): d = x - L; D = D + d * d, plain fp32, nothing fused
// (-ffp-contract=off); var = D * inv_nn, the unbiased variance of the pixel's MEAN, and +0.0f for one sample whatever the records hold.
// One 16-byte store of {var r, var g, var b, spp} per pixel.
__global__ void __launch_bounds__(256) r1_resolve_moments_kernel(const R1MomentsArgs A)
{
    const uint32_t tile_px = r1_tile_slots(A.geom);
    for (uint32_t lt = blockIdx.y; lt < A.n_tiles; lt += gridDim.y)
    {
        const R1TileRect rect = r1_tile_rect(A.geom, lt);
        for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < tile_px; pix += gridDim.x * blockDim.x)
        {
            int lx, ly;
            if (!r1_tile_pixel(A.geom, rect, pix, &lx, &ly))
                continue; // void slots of an edge tile
            const float4 *const s = A.samples + (size_t)lt * A.full + pix;
            float cr = 0, cg = 0, cb = 0;
            sum_records(s, tile_px, A.spp, cr, cg, cb);
            const float lr = cr * A.inv_spp, lg = cg * A.inv_spp, lb = cb * A.inv_spp; // col *= 1 / spp rayweek1.cpp:765
            float dr = 0, dg = 0, db = 0;
            for (int i = 0; i < A.spp; ++i)
            {
                const float4 v = s[(size_t)i * tile_px];
                const float er = v.x - lr, eg = v.y - lg, eb = v.z - lb;
                dr = dr + er * er, dg = dg + eg * eg, db = db + eb * eb;
            }
            const size_t px = r1_pixel_row_major(A.geom, rect, lx, ly);
            float *const o = A.out + px * 3;
            o[0] = lr, o[1] = lg, o[2] = lb;
            const bool many = A.spp > 1;
            A.moments[px] = make_uint4(many ? __float_as_uint(dr * A.inv_nn) : 0u, many ? __float_as_uint(dg * A.inv_nn) : 0u,
                                       many ? __float_as_uint(db * A.inv_nn) : 0u, (uint32_t)A.spp);
        }
    }
}

// ---- launchers (called from r1_frame.cpp, r1_render.cpp) -----------------------------------------------------

// The grid of a tile-row launch: workgroups of 256 threads across a padded tile's slots, one row of them per tile (at most 65535 rows; a row walks
// tiles row, row + rows, ...).  max_rows > 0: at most this many rows.  Frames in flight use FEW, long-lived workgroups: a resolve launch shares the
// chip with persistent trace workgroups and gets a slot only when one of them exits, so what it costs is the number of slot grants it needs, not
// its 26 us of work (profiles/r03/burst_timeline_20_frames.txt).
static dim3 tile_row_grid(const R1TileGeom &g, const uint32_t tiles, const int max_rows)
{
    const int bx = (g.tile_w * g.tile_h + 255) / 256;
    int by = (int)(tiles < 65535u ? tiles : 65535u);
    if (max_rows > 0 && by > max_rows)
        by = max_rows;
    return dim3(bx, by);
}

extern "C" hipError_t r1_launch_land_arm(const R1LandArmArgs *args, hipStream_t stream)
{
    const uint32_t n_frames = args->n_frames, n = n_frames * args->n_local_tiles > n_frames ? n_frames * args->n_local_tiles : n_frames;
    hipLaunchKernelGGL(r1_land_arm_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t r1_launch_resolve(const R1ResolveArgs *args, int max_rows, hipStream_t stream)
{
    const dim3 grid = tile_row_grid(args->geom, args->n_local_tiles * (args->n_frames ? args->n_frames : 1u), max_rows);
    hipLaunchKernelGGL(r1_resolve_kernel, grid, dim3(256), 0, stream, *args);
    if (args->frame_rays) // frame batches: per-frame ray counts from the launch's partial sums ([tile of the batch][bx])
        hipLaunchKernelGGL(r1_batch_counts_kernel, dim3(args->n_frames), dim3(256), 0, stream, args->frame_rays, args->n_local_tiles * grid.x, args->out,
                           args->out_stride, args->rays_offset);
    return hipGetLastError();
}

// one row of workgroups per tile, as the synchronous frame's resolve launch
extern "C" hipError_t r1_launch_accum(const R1AccumArgs *args, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_accum_kernel, tile_row_grid(args->geom, args->n_local_tiles, 0), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

// linear frames: as r1_launch_accum; a frame in flight takes the resolve's few rows
extern "C" hipError_t r1_launch_resolve_linear(const R1LinearArgs *args, int max_rows, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_resolve_linear_kernel, tile_row_grid(args->geom, args->n_tiles, max_rows), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

// variance frames: r1_launch_resolve_linear's grid
extern "C" hipError_t r1_launch_resolve_moments(const R1MomentsArgs *args, int max_rows, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_resolve_moments_kernel, tile_row_grid(args->geom, args->n_tiles, max_rows), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

// region renders: one row of workgroups per tile of the region, as r1_launch_accum
extern "C" hipError_t r1_launch_resolve_region(const R1RegionArgs *args, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_resolve_region_kernel, tile_row_grid(args->geom, args->n_tiles, 0), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t r1_launch_accum_linear(const R1ReadoutArgs *args, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_accum_linear_kernel, tile_row_grid(args->geom, args->n_tiles, 0), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

// one workgroup per listed tile (at most 65535, each walking list positions a grid apart), then the next pass's list
extern "C" hipError_t r1_launch_adapt_accum(const R1AdaptArgs *args, hipStream_t stream)
{
    const int bx = (int)(args->n_listed < 65535u ? args->n_listed : 65535u);
    hipLaunchKernelGGL(r1_adapt_accum_kernel, dim3(bx), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t r1_launch_adapt_compact(const uint32_t *cur, uint32_t n_cur, const R1TileReport *report, uint32_t at_cap, uint32_t *next,
                                              uint32_t *count_out, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_adapt_compact_kernel, dim3(1), dim3(256), 0, stream, cur, n_cur, report, at_cap, next, count_out);
    return hipGetLastError();
}

extern "C" hipError_t r1_launch_assemble(const R1AssembleArgs *args, hipStream_t stream)
{
    const size_t n = (size_t)args->geom.width * args->geom.height;
    int grid = (int)((n + 255) / 256);
    if (grid > 8192)
        grid = 8192;
    hipLaunchKernelGGL(r1_assemble_kernel, dim3(grid, args->n_frames > 0 ? args->n_frames : 1), dim3(256), 0, stream, *args);
    return hipGetLastError();
}
