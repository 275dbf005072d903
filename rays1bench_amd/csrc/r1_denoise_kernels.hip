// r1_denoise_kernels.hip — the kernels of denoised frames (include/rays1.h "denoised frames"): r1_denoise_prepare_kernel turns a
// linear frame and its feature frame into the filter's two 16-byte records per pixel, r1_denoise_pass_kernel is one a-trous iteration.  The
// arithmetic is r1_denoise.h's, line for line what r1_denoise_host runs; the 25 taps of a pixel are taken in the contract's order (dy outer,
// dx inner) by one thread, so the sums have one order.
//
// A workgroup owns a 32 x 8 tile (r1_tile.h), a thread one pixel; a wave is two rows of 32 pixels, so the records of a tap row are two
// contiguous 512-byte runs.  STAGED: the workgroup first copies its tile plus a halo of 2 * step pixels into LDS — a pixel off the image
// becomes a guide with surf = 0, which is how a tap off the image is skipped — and the taps are two ds_read_b128 each; otherwise a tap is two
// global_load_dwordx4 at an address that depends on the pixel's position only.  LAST: the pass re-modulates and stores three floats with the
// caller's stride instead of a record.
#include <hip/hip_runtime.h>

#include "r1_denoise.h"
#include "r1_internal.h"
#include "r1_tile.h"

static_assert(sizeof(R1DenoiseCur) == 16 && sizeof(R1DenoiseGuide) == 16, "a tap is two 16-byte loads");
static_assert(R1D_TILE_W * R1D_TILE_H == 256, "one thread per pixel of a tile");

#define R1D_HALO_MAX (2 * R1D_STAGE_MAX_STEP)
#define R1D_STAGE_W (R1D_TILE_W + 2 * R1D_HALO_MAX)
#define R1D_STAGE_H (R1D_TILE_H + 2 * R1D_HALO_MAX)

// a record travels as one 16-byte word, through global memory and through LDS
__device__ __forceinline__ R1DenoiseCur as_cur(const float4 v) { return {{v.x, v.y, v.z}, v.w}; }
__device__ __forceinline__ R1DenoiseGuide as_guide(const float4 v) { return {{v.x, v.y, v.z}, v.w}; }
__device__ __forceinline__ float4 word(const R1DenoiseCur &c) { return make_float4(c.e[0], c.e[1], c.e[2], c.m); }
__device__ __forceinline__ float4 word(const R1DenoiseGuide &g) { return make_float4(g.nh[0], g.nh[1], g.nh[2], g.surf); }

__global__ void __launch_bounds__(256) r1_denoise_prepare_kernel(const R1DenoiseArgs A)
{
    const R1TileGeom g = r1_tile_geom(A.width, A.height, R1D_TILE_W, R1D_TILE_H);
    const R1TileRect r = r1_tile_rect(g, blockIdx.x);
    int lx, ly;
    if (!r1_tile_pixel(g, r, threadIdx.x, &lx, &ly))
        return;
    const size_t x = (size_t)(r.x0 + lx), y = (size_t)(r.y0 + ly);
    const float *__restrict__ Lp = A.L + (y * A.linear_stride + x) * 3;
    const float4 *__restrict__ fp = (const float4 *)A.f + (y * A.feature_stride + x) * 2;
    const float L[3] = {Lp[0], Lp[1], Lp[2]};
    const float4 f0 = fp[0], f1 = fp[1]; // {albedo rgb, depth} {normal xyz, hits}
    const float albedo[3] = {f0.x, f0.y, f0.z}, normal[3] = {f1.x, f1.y, f1.z};
    R1DenoiseCur cur;
    R1DenoiseGuide gd;
    r1d_prepare(L, albedo, f0.w, normal, __float_as_uint(f1.w), A.flags, cur, gd);
    const size_t i = y * (size_t)A.width + x;
    ((float4 *)A.next)[i] = word(cur);
    ((float4 *)A.guide)[i] = word(gd);
}

template <bool STAGED, bool LAST>
__global__ void __launch_bounds__(256) r1_denoise_pass_kernel(const R1DenoiseArgs A)
{
    __shared__ float4 s_cur[STAGED ? R1D_STAGE_W * R1D_STAGE_H : 1];
    __shared__ float4 s_guide[STAGED ? R1D_STAGE_W * R1D_STAGE_H : 1];
    const float4 *__restrict__ const g_cur = (const float4 *)A.cur, *__restrict__ const g_guide = (const float4 *)A.guide;
    const R1TileGeom g = r1_tile_geom(A.width, A.height, R1D_TILE_W, R1D_TILE_H);
    const R1TileRect r = r1_tile_rect(g, blockIdx.x);
    const int step = A.step, halo = 2 * step;
    const int sw = R1D_TILE_W + 2 * halo; // the staged rows' pitch (STAGED: halo <= R1D_HALO_MAX, the launch sees to it)
    if (STAGED)
    {
        const int sh = r.th + 2 * halo;
        for (int s = (int)threadIdx.x; s < sw * sh; s += 256)
        {
            const int sy = s / sw, sx = s - sy * sw;
            const int qx = r.x0 - halo + sx, qy = r.y0 - halo + sy;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gd = c;
            if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height)
            {
                const size_t i = (size_t)qy * (size_t)A.width + (size_t)qx;
                c = g_cur[i], gd = g_guide[i];
            }
            s_cur[s] = c, s_guide[s] = gd;
        }
        __syncthreads();
    }
    int lx, ly;
    if (!r1_tile_pixel(g, r, threadIdx.x, &lx, &ly))
        return;
    const int x = r.x0 + lx, y = r.y0 + ly;
    const size_t ip = (size_t)y * (size_t)A.width + (size_t)x;
    R1DenoiseCur p;
    R1DenoiseGuide gp;
    if (STAGED)
        p = as_cur(s_cur[(ly + halo) * sw + lx + halo]), gp = as_guide(s_guide[(ly + halo) * sw + lx + halo]);
    else
        p = as_cur(g_cur[ip]), gp = as_guide(g_guide[ip]);
    R1DenoiseCur nx = p; // a pixel without a hit keeps its value; m travels with every pixel
    const bool surf = gp.surf != 0.0f;
    if (surf)
    {
        float S[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f;
#pragma unroll 1
        for (int dy = -2; dy <= 2; ++dy)
        {
            const float hy = r1d_h(dy);
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx)
            {
                R1DenoiseCur q;
                R1DenoiseGuide gq;
                if (STAGED)
                {
                    const int s = (ly + halo + dy * step) * sw + lx + halo + dx * step;
                    gq = as_guide(s_guide[s]), q = as_cur(s_cur[s]);
                }
                else
                {
                    const int qx = x + dx * step, qy = y + dy * step;
                    if (qx < 0 || qx >= A.width || qy < 0 || qy >= A.height)
                        continue;
                    const size_t iq = (size_t)qy * (size_t)A.width + (size_t)qx;
                    gq = as_guide(g_guide[iq]), q = as_cur(g_cur[iq]);
                }
                if (gq.surf == 0.0f)
                    continue;
                const float h = hy * r1d_h(dx);
                const float w = (dx == 0 && dy == 0) ? h : r1d_weight(h, p, gp, q, gq, A.k, A.sigma_depth, A.sc2);
                r1d_accumulate(w, q, S, W);
            }
        }
        for (int c = 0; c < 3; ++c)
            nx.e[c] = S[c] / W;
    }
    if (!LAST)
    {
        ((float4 *)A.next)[ip] = word(nx);
        return;
    }
    float *__restrict__ o = A.out + ((size_t)y * A.out_stride + (size_t)x) * 3;
    if (surf)
    {
        const float4 f0 = ((const float4 *)A.f)[((size_t)y * A.feature_stride + (size_t)x) * 2];
        o[0] = nx.e[0] * r1d_albedo(f0.x, A.flags), o[1] = nx.e[1] * r1d_albedo(f0.y, A.flags), o[2] = nx.e[2] * r1d_albedo(f0.z, A.flags);
    }
    else
        o[0] = nx.e[0], o[1] = nx.e[1], o[2] = nx.e[2];
}

static uint32_t denoise_tiles(const R1DenoiseArgs *a) { return (uint32_t)r1_tiles(r1_tile_geom(a->width, a->height, R1D_TILE_W, R1D_TILE_H)); }

extern "C" hipError_t r1_launch_denoise_prepare(const R1DenoiseArgs *args, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_denoise_prepare_kernel, dim3(denoise_tiles(args)), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

// staged: tile and halo through LDS (only for steps <= R1D_STAGE_MAX_STEP: refused otherwise); last: the pass that writes `out`
extern "C" hipError_t r1_launch_denoise_pass(const R1DenoiseArgs *args, int staged, int last, hipStream_t stream)
{
    if (args->step < 1 || (staged && args->step > R1D_STAGE_MAX_STEP))
        return hipErrorInvalidValue;
    const dim3 grid(denoise_tiles(args)), block(256);
    if (staged && last)
        hipLaunchKernelGGL((r1_denoise_pass_kernel<true, true>), grid, block, 0, stream, *args);
    else if (staged)
        hipLaunchKernelGGL((r1_denoise_pass_kernel<true, false>), grid, block, 0, stream, *args);
    else if (last)
        hipLaunchKernelGGL((r1_denoise_pass_kernel<false, true>), grid, block, 0, stream, *args);
    else
        hipLaunchKernelGGL((r1_denoise_pass_kernel<false, false>), grid, block, 0, stream, *args);
    return hipGetLastError();
}
