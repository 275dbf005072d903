// r1_denoise_kernels.hip — the kernels of both a-trous filters: denoised frames (include/rays1.h "denoised frames") and their
// variance-guided form ("variance-guided denoised frames", §4.40).  r1_denoise_prepare_kernel turns a linear frame and its feature frame into
// the filter's two 16-byte records per pixel, r1_denoise_pass_kernel is one a-trous iteration; r1_vfilter_prepare_kernel and
// r1_vfilter_pass_kernel are the same two bodies with GUIDED set, which adds the pixel's v — one dense float a pixel, ping and pong, beside
// the records (56 bytes a pixel of workspace instead of 48; packing v into the e record would have kept a tap at two loads but needs a place
// for m or surf: not done, not measured).  The arithmetic is r1_denoise.h's, line for line what r1_denoise_host and r1_denoise_guided_host
// run; the 25 taps of a pixel are taken in the contract's order (dy outer, dx inner) by one thread, so the sums have one order.
//
// A workgroup owns a 32 x 8 tile (r1_tile.h), a thread one pixel; a wave is two rows of 32 pixels, so the records of a tap row are two
// contiguous 512-byte runs.  STAGED: the workgroup first copies its tile plus a halo of 2 * step pixels into LDS — a pixel off the image
// becomes a guide with surf = 0, which is how a tap off the image is skipped — and the taps are two ds_read_b128 each (GUIDED: and a
// ds_read_b32; the 3 x 3 prefilter of v reads within one pixel, which every halo covers); otherwise a tap is two global_load_dwordx4 at an
// address that depends on the pixel's position only.  LAST: the pass re-modulates and stores three floats with the caller's stride instead
// of a record.
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

// GUIDED: V {var rgb, samples} a pixel, rows moment_stride pixels apart, and the v the first pass reads; otherwise unused
template <bool GUIDED>
__device__ __forceinline__ void prepare(const R1DenoiseArgs &A, const float *V, uint32_t moment_stride, float *v_next)
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
    float var[3] = {0.0f, 0.0f, 0.0f};
    if (GUIDED)
    {
        const float4 mv = ((const float4 *)V)[y * moment_stride + x];
        var[0] = mv.x, var[1] = mv.y, var[2] = mv.z;
    }
    R1DenoiseCur cur;
    R1DenoiseGuide gd;
    r1d_prepare(L, albedo, f0.w, normal, __float_as_uint(f1.w), A.flags, cur, gd);
    const size_t i = y * (size_t)A.width + x;
    ((float4 *)A.next)[i] = word(cur);
    ((float4 *)A.guide)[i] = word(gd);
    if (GUIDED)
        v_next[i] = r1d_prepare_v(var, albedo, __float_as_uint(f1.w), A.flags);
}

// GUIDED: g_v is the v the pass reads, v_next what it writes unless LAST (A.sc2: sigma_color squared); otherwise unused
template <bool GUIDED, bool STAGED, bool LAST>
__device__ __forceinline__ void pass(const R1DenoiseArgs &A, const float *const g_v, float *const v_next, const float variance_floor)
{
    __shared__ float4 s_cur[STAGED ? R1D_STAGE_W * R1D_STAGE_H : 1];
    __shared__ float4 s_guide[STAGED ? R1D_STAGE_W * R1D_STAGE_H : 1];
    __shared__ float s_v[STAGED && GUIDED ? R1D_STAGE_W * R1D_STAGE_H : 1];
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
            float vq = 0.0f;
            if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height)
            {
                const size_t i = (size_t)qy * (size_t)A.width + (size_t)qx;
                c = g_cur[i], gd = g_guide[i];
                if (GUIDED)
                    vq = g_v[i];
            }
            s_cur[s] = c, s_guide[s] = gd;
            if (GUIDED)
                s_v[s] = vq;
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
    float vx = 0.0f;
    if (STAGED)
        p = as_cur(s_cur[sp]), gp = as_guide(s_guide[sp]);
    else
        p = as_cur(g_cur[ip]), gp = as_guide(g_guide[ip]);
    if (GUIDED)
        vx = STAGED ? s_v[sp] : g_v[ip];
    R1DenoiseCur nx = p; // a pixel without a hit keeps its value (and its v of 0); m travels with every pixel
    const bool surf = gp.surf != 0.0f;
    if (surf)
    {
        float sc2 = A.sc2; // GUIDED: the pixel's own denominator, from the 3 x 3 prefilter of v
        if (GUIDED)
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
            sc2 = r1d_den(A.sc2, G / K, variance_floor);
        }
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
                // (vq is deliberately not initialised: behind `= 0.0f` the compiler loads a direct tap's surf alone, waits, and loads the
                // rest behind the test — a second round trip a tap, the guided passes of steps >= 4 a fifth slower; profiles/r38/denoise_ab.txt)
                float vq;
                if (STAGED)
                {
                    // (each family keeps the form of the index it was tuned with: the other one costs the staged unguided passes a VGPR and
                    // schedules the staged guided ones apart from the measured kernels, 1-3 us a pass slower at 1920 x 1080)
                    const int s = GUIDED ? sp + dy * step * sw + dx * step : (ly + halo + dy * step) * sw + lx + halo + dx * step;
                    gq = as_guide(s_guide[s]), q = as_cur(s_cur[s]);
                    if (GUIDED)
                        vq = s_v[s];
                }
                else
                {
                    const int qx = x + dx * step, qy = y + dy * step;
                    if (qx < 0 || qx >= A.width || qy < 0 || qy >= A.height)
                        continue;
                    const size_t iq = (size_t)qy * (size_t)A.width + (size_t)qx;
                    gq = as_guide(g_guide[iq]), q = as_cur(g_cur[iq]);
                    if (GUIDED)
                        vq = g_v[iq];
                }
                if (gq.surf == 0.0f)
                    continue;
                const float h = hy * r1d_h(dx);
                const float w = (dx == 0 && dy == 0) ? h : r1d_weight(h, p, gp, q, gq, A.k, A.sigma_depth, sc2);
                r1d_accumulate(w, q, S, W);
                if (GUIDED)
                    r1d_accumulate_v(w, vq, T);
            }
        }
        for (int c = 0; c < 3; ++c)
            nx.e[c] = S[c] / W;
        if (GUIDED)
            vx = T / (W * W);
    }
    if (!LAST)
    {
        ((float4 *)A.next)[ip] = word(nx);
        if (GUIDED)
            v_next[ip] = vx;
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

__global__ void __launch_bounds__(256) r1_denoise_prepare_kernel(const R1DenoiseArgs A) { prepare<false>(A, nullptr, 0u, nullptr); }
__global__ void __launch_bounds__(256) r1_vfilter_prepare_kernel(const R1VFilterArgs B) { prepare<true>(B.d, B.V, B.moment_stride, B.v_next); }
template <bool STAGED, bool LAST>
__global__ void __launch_bounds__(256) r1_denoise_pass_kernel(const R1DenoiseArgs A) { pass<false, STAGED, LAST>(A, nullptr, nullptr, 0.0f); }
template <bool STAGED, bool LAST>
__global__ void __launch_bounds__(256) r1_vfilter_pass_kernel(const R1VFilterArgs B) { pass<true, STAGED, LAST>(B.d, B.v_cur, B.v_next, B.variance_floor); }

static dim3 tiles(const R1DenoiseArgs &a) { return dim3((uint32_t)r1_tiles(r1_tile_geom(a.width, a.height, R1D_TILE_W, R1D_TILE_H))); }

// guided: the r1_vfilter kernels, which take all of *b; otherwise the r1_denoise kernels, which take b->d
static hipError_t launch(const void *kernel, const R1VFilterArgs *b, int guided, hipStream_t stream)
{
    void *args[1] = {guided ? (void *)b : (void *)&b->d};
    return hipLaunchKernel(kernel, tiles(b->d), dim3(256), args, 0, stream);
}

extern "C" hipError_t r1_launch_denoise_prepare(const R1VFilterArgs *b, int guided, hipStream_t stream)
{
    return launch(guided ? (const void *)r1_vfilter_prepare_kernel : (const void *)r1_denoise_prepare_kernel, b, guided, stream);
}

// staged: tile and halo through LDS (only for steps <= R1D_STAGE_MAX_STEP: refused otherwise); last: the pass that writes `out`
extern "C" hipError_t r1_launch_denoise_pass(const R1VFilterArgs *b, int guided, int staged, int last, hipStream_t stream)
{
    static const void *const kernels[2][2][2] = {
        {{(const void *)r1_denoise_pass_kernel<false, false>, (const void *)r1_denoise_pass_kernel<false, true>},
         {(const void *)r1_denoise_pass_kernel<true, false>, (const void *)r1_denoise_pass_kernel<true, true>}},
        {{(const void *)r1_vfilter_pass_kernel<false, false>, (const void *)r1_vfilter_pass_kernel<false, true>},
         {(const void *)r1_vfilter_pass_kernel<true, false>, (const void *)r1_vfilter_pass_kernel<true, true>}}}; // [guided][staged][last]
    if (b->d.step < 1 || (staged && b->d.step > R1D_STAGE_MAX_STEP))
        return hipErrorInvalidValue;
    return launch(kernels[!!guided][!!staged][!!last], b, guided, stream);
}
