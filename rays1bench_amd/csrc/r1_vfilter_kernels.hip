// r1_vfilter_kernels.hip — the kernels of variance-guided denoised frames (include/rays1.h "variance-guided denoised frames"):
// r1_vfilter_prepare_kernel is r1_denoise_prepare_kernel plus the pixel's v, r1_vfilter_pass_kernel one guided a-trous iteration.  Geometry,
// records and tap order are r1_denoise_kernels.hip's — a 32 x 8 tile a workgroup, a pixel a thread, dy rolled, dx unrolled, the 25 adds of a
// pixel by one thread in the contract's order — and the arithmetic is r1_denoise.h's, line for line what r1_denoise_guided_host runs.
//
// Layout: the unguided filter's two 16-byte records stay as they are ({e, m} ping and pong, {nh, surf} once), so r1d_prepare and r1d_weight
// serve unchanged; v, the one value that must ping-pong besides e, is a dense float a pixel of its own, ping and pong.  A tap is two 16-byte
// loads and one 4-byte load — 56 bytes a pixel of workspace instead of 48.  Packing v into the e record would have kept a tap at two loads but
// needs a place for m or surf in the guide record; not done, not measured.  STAGED: tile plus a halo of 2 * step pixels in LDS, v beside the
// records ((32 + 8) x (8 + 8) x 36 bytes); the 3 x 3 prefilter reads within one pixel, which every halo covers.
#include <hip/hip_runtime.h>

#include "r1_denoise.h"
#include "r1_internal.h"
#include "r1_tile.h"

#define R1V_HALO_MAX (2 * R1D_STAGE_MAX_STEP)
#define R1V_STAGE_W (R1D_TILE_W + 2 * R1V_HALO_MAX)
#define R1V_STAGE_H (R1D_TILE_H + 2 * R1V_HALO_MAX)

namespace
{
__device__ __forceinline__ R1DenoiseCur as_cur(const float4 v) { return {{v.x, v.y, v.z}, v.w}; }
__device__ __forceinline__ R1DenoiseGuide as_guide(const float4 v) { return {{v.x, v.y, v.z}, v.w}; }
__device__ __forceinline__ float4 word(const R1DenoiseCur &c) { return make_float4(c.e[0], c.e[1], c.e[2], c.m); }
__device__ __forceinline__ float4 word(const R1DenoiseGuide &g) { return make_float4(g.nh[0], g.nh[1], g.nh[2], g.surf); }
} // namespace

__global__ void __launch_bounds__(256) r1_vfilter_prepare_kernel(const R1VFilterArgs B)
{
    const R1DenoiseArgs &A = B.d;
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
    const float4 mv = ((const float4 *)B.V)[y * B.moment_stride + x]; // {var rgb, samples}
    const float albedo[3] = {f0.x, f0.y, f0.z}, normal[3] = {f1.x, f1.y, f1.z}, var[3] = {mv.x, mv.y, mv.z};
    R1DenoiseCur cur;
    R1DenoiseGuide gd;
    r1d_prepare(L, albedo, f0.w, normal, __float_as_uint(f1.w), A.flags, cur, gd);
    const size_t i = y * (size_t)A.width + x;
    ((float4 *)A.next)[i] = word(cur);
    ((float4 *)A.guide)[i] = word(gd);
    B.v_next[i] = r1d_prepare_v(var, albedo, __float_as_uint(f1.w), A.flags);
}

template <bool STAGED, bool LAST>
__global__ void __launch_bounds__(256) r1_vfilter_pass_kernel(const R1VFilterArgs B)
{
    __shared__ float4 s_cur[STAGED ? R1V_STAGE_W * R1V_STAGE_H : 1];
    __shared__ float4 s_guide[STAGED ? R1V_STAGE_W * R1V_STAGE_H : 1];
    __shared__ float s_v[STAGED ? R1V_STAGE_W * R1V_STAGE_H : 1];
    const R1DenoiseArgs &A = B.d;
    const float4 *__restrict__ const g_cur = (const float4 *)A.cur, *__restrict__ const g_guide = (const float4 *)A.guide;
    const float *__restrict__ const g_v = B.v_cur;
    const R1TileGeom g = r1_tile_geom(A.width, A.height, R1D_TILE_W, R1D_TILE_H);
    const R1TileRect r = r1_tile_rect(g, blockIdx.x);
    const int step = A.step, halo = 2 * step;
    const int sw = R1D_TILE_W + 2 * halo; // the staged rows' pitch (STAGED: halo <= R1V_HALO_MAX, the launch sees to it)
    if (STAGED)
    {
        const int sh = r.th + 2 * halo;
        for (int s = (int)threadIdx.x; s < sw * sh; s += 256)
        {
            const int sy = s / sw, sx = s - sy * sw;
            const int qx = r.x0 - halo + sx, qy = r.y0 - halo + sy;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gd = c;
            float vq = 0.0f;
            if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height)
            {
                const size_t i = (size_t)qy * (size_t)A.width + (size_t)qx;
                c = g_cur[i], gd = g_guide[i], vq = g_v[i];
            }
            s_cur[s] = c, s_guide[s] = gd, s_v[s] = vq;
        }
        __syncthreads();
    }
    int lx, ly;
    if (!r1_tile_pixel(g, r, threadIdx.x, &lx, &ly))
        return;
    const int x = r.x0 + lx, y = r.y0 + ly;
    const size_t ip = (size_t)y * (size_t)A.width + (size_t)x;
    const int sp = (ly + halo) * sw + lx + halo;
    R1DenoiseCur p;
    R1DenoiseGuide gp;
    float vx;
    if (STAGED)
        p = as_cur(s_cur[sp]), gp = as_guide(s_guide[sp]), vx = s_v[sp];
    else
        p = as_cur(g_cur[ip]), gp = as_guide(g_guide[ip]), vx = g_v[ip];
    R1DenoiseCur nx = p; // a pixel without a hit keeps its value and its v of 0; m travels with every pixel
    const bool surf = gp.surf != 0.0f;
    if (surf)
    {
        float G = 0.0f, K = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
            {
                float sq, vq;
                if (STAGED)
                {
                    const int s = sp + dy * sw + dx;
                    sq = s_guide[s].w, vq = s_v[s];
                }
                else
                {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= A.width || qy < 0 || qy >= A.height)
                        continue;
                    const size_t iq = (size_t)qy * (size_t)A.width + (size_t)qx;
                    sq = g_guide[iq].w, vq = g_v[iq];
                }
                if (sq == 0.0f)
                    continue;
                r1d_prefilter_tap(r1d_k3(dy) * r1d_k3(dx), vq, G, K);
            }
        const float den = r1d_den(A.sc2, G / K, B.variance_floor);
        float S[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f, T = 0.0f;
#pragma unroll 1
        for (int dy = -2; dy <= 2; ++dy)
        {
            const float hy = r1d_h(dy);
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx)
            {
                R1DenoiseCur q;
                R1DenoiseGuide gq;
                float vq;
                if (STAGED)
                {
                    const int s = sp + dy * step * sw + dx * step;
                    gq = as_guide(s_guide[s]), q = as_cur(s_cur[s]), vq = s_v[s];
                }
                else
                {
                    const int qx = x + dx * step, qy = y + dy * step;
                    if (qx < 0 || qx >= A.width || qy < 0 || qy >= A.height)
                        continue;
                    const size_t iq = (size_t)qy * (size_t)A.width + (size_t)qx;
                    gq = as_guide(g_guide[iq]), q = as_cur(g_cur[iq]), vq = g_v[iq];
                }
                if (gq.surf == 0.0f)
                    continue;
                const float h = hy * r1d_h(dx);
                const float w = (dx == 0 && dy == 0) ? h : r1d_weight(h, p, gp, q, gq, A.k, A.sigma_depth, den);
                r1d_accumulate(w, q, S, W);
                r1d_accumulate_v(w, vq, T);
            }
        }
        for (int c = 0; c < 3; ++c)
            nx.e[c] = S[c] / W;
        vx = T / (W * W);
    }
    if (!LAST)
    {
        ((float4 *)A.next)[ip] = word(nx);
        B.v_next[ip] = vx;
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

static uint32_t vfilter_tiles(const R1VFilterArgs *a) { return (uint32_t)r1_tiles(r1_tile_geom(a->d.width, a->d.height, R1D_TILE_W, R1D_TILE_H)); }

extern "C" hipError_t r1_launch_vfilter_prepare(const R1VFilterArgs *args, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_vfilter_prepare_kernel, dim3(vfilter_tiles(args)), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

// staged: tile and halo through LDS (only for steps <= R1D_STAGE_MAX_STEP: refused otherwise); last: the pass that writes `out`
extern "C" hipError_t r1_launch_vfilter_pass(const R1VFilterArgs *args, int staged, int last, hipStream_t stream)
{
    if (args->d.step < 1 || (staged && args->d.step > R1D_STAGE_MAX_STEP))
        return hipErrorInvalidValue;
    const dim3 grid(vfilter_tiles(args)), block(256);
    if (staged && last)
        hipLaunchKernelGGL((r1_vfilter_pass_kernel<true, true>), grid, block, 0, stream, *args);
    else if (staged)
        hipLaunchKernelGGL((r1_vfilter_pass_kernel<true, false>), grid, block, 0, stream, *args);
    else if (last)
        hipLaunchKernelGGL((r1_vfilter_pass_kernel<false, true>), grid, block, 0, stream, *args);
    else
        hipLaunchKernelGGL((r1_vfilter_pass_kernel<false, false>), grid, block, 0, stream, *args);
    return hipGetLastError();
}
