// r1_reproject.h — the arithmetic of accumulated frames (include/rays1.h "accumulated frames"), once, for the host form
// (r1_accumulate_host.cpp) and the kernel (r1_reproject_kernels.hip): the plan of a call, the world point of a pixel, its position on the
// previous camera's screen with the guards in front of every integer, the test and the sums of a tap, and the blend.  Both sides call these
// lines.
//
// The rules are r1_denoise.h's: correctly rounded fp32 + - * / sqrt, comparisons and selects, one operation per step in the order written
// (-ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt hold for host and device code; subnormal values are kept); the one library
// call is floorf, which is exact.  A dot product is (a.x * b.x + a.y * b.y) + a.z * b.z everywhere.
#ifndef R1_REPROJECT_H
#define R1_REPROJECT_H

#include <stdint.h>

#include "r1_denoise.h" // R1D_HD; r1d_prepare: the rule that makes a unit normal of a feature record's sum of normals

// Computed once per call on the host from the PREVIOUS camera and the frame's size
struct R1ReprojectPlan
{
    float pu, pv, pw; // (lower_left - origin) . u, . v, . w
    float hu, vv;     // horizontal . u, vertical . v
    float inv_w, inv_h;
};

// What the arithmetic reads of the two cameras and the two renders, by value in the kernel's arguments
struct R1ReprojectView
{
    float o[3], ll[3], hz[3], vt[3];  // the current camera: origin, lower_left, horizontal, vertical
    float op[3], up[3], vp[3], wp[3]; // the previous camera: origin, u, v, w
    R1ReprojectPlan plan;
    float spp, spp_prev;              // (float)spp of the current render and of the render that made f_prev
    float wf, hf;                     // (float)width, (float)height
};

R1D_HD float r1r_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// false: pw, hu or vv is zero or not finite — no pixel can be projected through that camera
R1D_HD bool r1r_plan(const float origin[3], const float lower_left[3], const float horizontal[3], const float vertical[3], const float u[3], const float v[3],
                     const float w[3], int width, int height, R1ReprojectPlan &p)
{
    const float dl[3] = {lower_left[0] - origin[0], lower_left[1] - origin[1], lower_left[2] - origin[2]};
    p.pu = r1r_dot(dl, u), p.pv = r1r_dot(dl, v), p.pw = r1r_dot(dl, w);
    p.hu = r1r_dot(horizontal, u), p.vv = r1r_dot(vertical, v);
    p.inv_w = 1.0f / (float)width, p.inv_h = 1.0f / (float)height;
    const float big = 3.402823466e38f;
    const bool fin = p.pw >= -big && p.pw <= big && p.hu >= -big && p.hu <= big && p.vv >= -big && p.vv <= big;
    return fin && p.pw != 0.0f && p.hu != 0.0f && p.vv != 0.0f;
}

// The unit normal of a record (zero where the normals cancel): r1d_prepare's lines, with nothing of a colour in them
R1D_HD void r1r_unit_normal(const float normal[3], float nh[3])
{
    const float none[3] = {0.0f, 0.0f, 0.0f};
    R1DenoiseCur cur;
    R1DenoiseGuide g;
    r1d_prepare(none, none, 0.0f, normal, 0u, 0u, cur, g);
    nh[0] = g.nh[0], nh[1] = g.nh[1], nh[2] = g.nh[2];
}

// The mean hit distance of a record with hits > 0, from the render's spp
R1D_HD float r1r_distance(float depth, uint32_t hits, float spp) { return (depth / (float)hits) * spp; }

// The world point the pixel (x, y) of the current frame shows, a pinhole reconstruction: q = P - origin_prev
R1D_HD void r1r_world(const R1ReprojectView &v, int x, int y, float depth, uint32_t hits, float q[3])
{
    const float s = ((float)x + 0.5f) * v.plan.inv_w, t = ((float)y + 0.5f) * v.plan.inv_h;
    float d[3];
    for (int c = 0; c < 3; ++c)
        d[c] = ((v.ll[c] + v.hz[c] * s) + v.vt[c] * t) - v.o[c];
    const float l = __builtin_sqrtf(r1r_dot(d, d));
    const float m = r1r_distance(depth, hits, v.spp);
    for (int c = 0; c < 3; ++c)
    {
        const float dh = d[c] / l;
        const float P = v.o[c] + dh * m;
        q[c] = P - v.op[c];
    }
}

// Where q lies on the previous camera's screen.  false: no history.  Every guard is a comparison of floats that a NaN fails, and the only
// conversions to an integer stand behind all of them: -1 <= x0 <= width - 1 and -1 <= y0 <= height - 1 whatever the frames held.
R1D_HD bool r1r_project(const R1ReprojectView &v, const float q[3], int &x0, int &y0, float &fx, float &fy, float &e)
{
    const float a = r1r_dot(q, v.up), b = r1r_dot(q, v.vp), c = r1r_dot(q, v.wp);
    if (!(c * v.plan.pw > 0.0f))
        return false;
    const float k = v.plan.pw / c;
    const float sx = (a * k - v.plan.pu) / v.plan.hu, sy = (b * k - v.plan.pv) / v.plan.vv;
    const float px = sx * v.wf - 0.5f, py = sy * v.hf - 0.5f;
    if (!(px > -1.0f && px < v.wf && py > -1.0f && py < v.hf))
        return false;
    const float flx = __builtin_floorf(px), fly = __builtin_floorf(py);
    x0 = (int)flx, y0 = (int)fly;
    fx = px - flx, fy = py - fly;
    e = __builtin_sqrtf(r1r_dot(q, q));
    return true;
}

// The bilinear weight of tap (i, j)
R1D_HD float r1r_weight(int i, int j, float fx, float fy) { return (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy); }

// The sums over the taps taken
struct R1ReprojectSums
{
    float B, C[3], U[3];
    uint32_t N;
};
R1D_HD void r1r_sums_clear(R1ReprojectSums &s)
{
    s.B = 0.0f, s.N = 0xFFFFFFFFu;
    for (int c = 0; c < 3; ++c)
        s.C[c] = 0.0f, s.U[c] = 0.0f;
}

// Is the tap whose records are on the image taken?  b: its bilinear weight; e: the expected distance; nh: the pixel's unit normal
R1D_HD bool r1r_tap_taken(float b, float e, const float nh[3], float depth_q, const float normal_q[3], uint32_t hits_q, uint32_t samples_q, float spp_prev,
                          float depth_tolerance, float normal_min_cos)
{
    if (!(b > 0.0f) || hits_q == 0u || samples_q == 0u)
        return false;
    const float mq = r1r_distance(depth_q, hits_q, spp_prev);
    float diff = e - mq;
    diff = diff < 0.0f ? -diff : diff;
    const float mx = e < mq ? mq : e;
    if (!(diff <= depth_tolerance * mx))
        return false;
    float nq[3];
    r1r_unit_normal(normal_q, nq);
    return !(r1r_dot(nh, nq) < normal_min_cos);
}

R1D_HD void r1r_tap_add(float b, const float A[3], const float var[3], uint32_t samples, R1ReprojectSums &s)
{
    s.B = s.B + b;
    for (int c = 0; c < 3; ++c)
    {
        s.C[c] = s.C[c] + b * A[c];
        s.U[c] = s.U[c] + b * var[c];
    }
    s.N = samples < s.N ? samples : s.N;
}

// The blend of a pixel whose sums have B > 0: n = V.samples >= 1.  Returns samples_out.
R1D_HD uint32_t r1r_blend(const R1ReprojectSums &s, const float L[3], const float var[3], uint32_t n, uint32_t max_samples, float A_out[3], float var_out[3])
{
    const uint64_t sum = (uint64_t)s.N + (uint64_t)n;
    const uint64_t capped = sum < (uint64_t)max_samples ? sum : (uint64_t)max_samples;
    const uint32_t N_new = capped < (uint64_t)n ? n : (uint32_t)capped;
    const float alpha = n >= N_new ? 1.0f : (float)n / (float)N_new;
    const float keep = 1.0f - alpha;
    for (int c = 0; c < 3; ++c)
    {
        const float hist = s.C[c] / s.B, vh = s.U[c] / s.B;
        A_out[c] = hist + (L[c] - hist) * alpha;
        var_out[c] = (keep * keep) * vh + (alpha * alpha) * var[c];
    }
    return N_new;
}

// ---- what the kernel reads and writes (r1_reproject_kernels.hip), device memory; by value in its arguments ----
// A workgroup of 256 threads owns one 32 x 8 tile of the frame (r1_tile.h's geometry, R1D_TILE_W x R1D_TILE_H as the filters'), a thread one
// pixel.  Strides in pixels, never 0 here.
struct R1ReprojectArgs
{
    const float *L;       // 3 floats a pixel
    const float *V;       // 4 words a pixel {var r, g, b, samples}, 16-byte aligned
    const float *f;       // 8 words a pixel, 16-byte aligned
    const float *A_prev;  // the history: 3 floats a pixel ...
    const float *f_prev;  // ... its feature frame ...
    const float *M_prev;  // ... and its moments, samples = the history's length
    float *A_out;         // may be L
    float *M_out;         // may be V
    int32_t width, height;
    uint32_t linear_stride, moment_stride, feature_stride, prev_stride, prev_feature_stride, prev_moment_stride, out_stride, out_moment_stride;
    uint32_t max_samples;
    float depth_tolerance, normal_min_cos;
    R1ReprojectView view;
};

#endif
