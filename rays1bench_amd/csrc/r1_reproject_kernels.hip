// r1_reproject_kernels.hip — the kernel of accumulated frames (include/rays1.h "accumulated frames"): r1_reproject_kernel,
// one launch a call.  Geometry is the filters' — a 32 x 8 tile a workgroup (r1_tile.h), a pixel a thread — and the arithmetic is
// r1_reproject.h's, line for line what r1_accumulate_host runs.
//
// Memory: the pixel's own L is three dwords, f two 16-byte loads, V one; consecutive lanes read consecutive pixels of a row.  The taps are a
// gather: the four records of a pixel lie where its surface was on the previous screen, so the source window of a tile depends on the data
// and nothing is staged in LDS; under a camera that turns slowly the lanes of a row still read neighbouring pixels and the four taps of
// neighbouring lanes overlap, which the caches serve.  A tap is up to 60 bytes (f_prev 32, M_prev 16, A_prev 12).
//
// Load order: all of a pixel's tap loads are issued before the first test.  Tap coordinates are CLAMPED to the image for the loads (a tap
// off the image reads the edge pixel's records and is then skipped by the test on the unclamped integers), so every lane with history
// issues the same twelve loads with no branch between them and none waits for another's result; loading a tap's A and M only behind its
// feature test would save bytes where taps fail and serialise two round trips to memory where they pass, which is the common case.  The
// bits are the same either way.  No pointer is selected: every load has its own base.
#include <hip/hip_runtime.h>

#include "r1_internal.h"
#include "r1_reproject.h"
#include "r1_tile.h"

__global__ void __launch_bounds__(256) r1_reproject_kernel(const R1ReprojectArgs A)
{
    const R1TileGeom g = r1_tile_geom(A.width, A.height, R1D_TILE_W, R1D_TILE_H);
    const R1TileRect r = r1_tile_rect(g, blockIdx.x);
    int lx, ly;
    if (!r1_tile_pixel(g, r, threadIdx.x, &lx, &ly))
        return;
    const int x = r.x0 + lx, y = r.y0 + ly;
    const size_t sx = (size_t)x, sy = (size_t)y;
    const float *Lp = A.L + (sy * A.linear_stride + sx) * 3;
    const float L[3] = {Lp[0], Lp[1], Lp[2]};
    const float4 mv = ((const float4 *)A.V)[sy * A.moment_stride + sx];               // {var rgb, samples}
    const float4 *fp = (const float4 *)A.f + (sy * A.feature_stride + sx) * 2;
    const float4 f0 = fp[0], f1 = fp[1];                                              // {albedo rgb, depth} {normal xyz, hits}
    const uint32_t n = __float_as_uint(mv.w), hits = __float_as_uint(f1.w);
    const float var[3] = {mv.x, mv.y, mv.z};
    float out[3] = {L[0], L[1], L[2]};
    float4 mo = mv;
    int x0 = 0, y0 = 0;
    float fx = 0.0f, fy = 0.0f, e = 0.0f, q[3];
    bool history = hits != 0u && n != 0u;
    if (history)
    {
        r1r_world(A.view, x, y, f0.w, hits, q);
        history = r1r_project(A.view, q, x0, y0, fx, fy, e);
    }
    if (history)
    {
        // -1 <= x0 <= width - 1 and -1 <= y0 <= height - 1 here (r1r_project); the loads go to the clamped pixel, the test sees the integers
        float4 t0[4], t1[4], tm[4];
        float ta[4][3];
        bool on[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const int i = k & 1, j = k >> 1;
            const int tx = x0 + i, ty = y0 + j;
            on[k] = tx >= 0 && tx < A.width && ty >= 0 && ty < A.height;
            const int cx = tx < 0 ? 0 : tx >= A.width ? A.width - 1 : tx;
            const int cy = ty < 0 ? 0 : ty >= A.height ? A.height - 1 : ty;
            const float4 *fq = (const float4 *)A.f_prev + ((size_t)cy * A.prev_feature_stride + (size_t)cx) * 2;
            t0[k] = fq[0], t1[k] = fq[1];
            tm[k] = ((const float4 *)A.M_prev)[(size_t)cy * A.prev_moment_stride + (size_t)cx];
            const float *aq = A.A_prev + ((size_t)cy * A.prev_stride + (size_t)cx) * 3;
            ta[k][0] = aq[0], ta[k][1] = aq[1], ta[k][2] = aq[2];
        }
        const float normal[3] = {f1.x, f1.y, f1.z};
        float nh[3];
        r1r_unit_normal(normal, nh);
        R1ReprojectSums s;
        r1r_sums_clear(s);
#pragma unroll
        for (int k = 0; k < 4; ++k) // k = j * 2 + i: j in the outer loop
        {
            const float b = r1r_weight(k & 1, k >> 1, fx, fy);
            const float nq[3] = {t1[k].x, t1[k].y, t1[k].z}, vq[3] = {tm[k].x, tm[k].y, tm[k].z};
            const uint32_t samples = __float_as_uint(tm[k].w);
            if (on[k] && r1r_tap_taken(b, e, nh, t0[k].w, nq, __float_as_uint(t1[k].w), samples, A.view.spp_prev, A.depth_tolerance, A.normal_min_cos))
                r1r_tap_add(b, ta[k], vq, samples, s);
        }
        if (s.B > 0.0f)
        {
            float vo[3];
            const uint32_t N_new = r1r_blend(s, L, var, n, A.max_samples, out, vo);
            mo = make_float4(vo[0], vo[1], vo[2], __uint_as_float(N_new));
        }
    }
    float *o = A.A_out + (sy * A.out_stride + sx) * 3;
    o[0] = out[0], o[1] = out[1], o[2] = out[2];
    ((float4 *)A.M_out)[sy * A.out_moment_stride + sx] = mo;
}

extern "C" hipError_t r1_launch_reproject(const R1ReprojectArgs *args, hipStream_t stream)
{
    const uint32_t tiles = (uint32_t)r1_tiles(r1_tile_geom(args->width, args->height, R1D_TILE_W, R1D_TILE_H));
    hipLaunchKernelGGL(r1_reproject_kernel, dim3(tiles), dim3(256), 0, stream, *args);
    return hipGetLastError();
}
