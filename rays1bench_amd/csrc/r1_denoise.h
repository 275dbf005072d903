// r1_denoise.h — the arithmetic of denoised frames (include/rays1.h "denoised frames"), once, for the host form
// (r1_denoise_host.cpp) and the kernels (r1_denoise_kernels.hip): the prepare step of a pixel, the 5-tap table, the weight of a tap and
// the accumulation of one.  Both sides call these lines.
//
// Everything here is correctly rounded fp32 + - * / sqrt, comparisons and selects (the Makefile's -ffp-contract=off and
// -fhip-fp32-correctly-rounded-divide-sqrt hold for host and device code; subnormal values are kept on both sides): the host and the device
// compute the same bits from the same inputs.  No library call whose rounding could differ between the two — the weights are rational, there
// is no exp —, min / max / clamp are spelled as selects, as r1_bvh_fill.h spells them.
#ifndef R1_DENOISE_H
#define R1_DENOISE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define R1D_HD __host__ __device__ inline
#else
#define R1D_HD inline
#endif

#define R1D_DEMODULATE 1u /* R1_DENOISE_DEMODULATE */

// What the filter keeps of a pixel, two 16-byte records: the value being filtered with the mean hit distance (rewritten by every pass, m
// carried along), and the guide (written once).
struct alignas(16) R1DenoiseCur { float e[3], m; };
struct alignas(16) R1DenoiseGuide { float nh[3], surf; }; // surf: 1.0f where hits > 0, else 0.0f

// The 5-tap B3 spline {1/16, 1/4, 3/8, 1/4, 1/16} at offset d = -2 .. 2; the product of two of them is exact.
R1D_HD float r1d_h(int d)
{
    const int a = d < 0 ? -d : d;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// The albedo a pixel is divided by before the filter and multiplied by after it
R1D_HD float r1d_albedo(float albedo, uint32_t flags)
{
    return (flags & R1D_DEMODULATE) ? (albedo < 0.00390625f ? 0.00390625f : albedo) : 1.0f;
}

// Prepare: the two records of a pixel from its linear value L and its feature record.  A pixel without a hit is never a tap and is never
// filtered: its record keeps L's bits, which is what the frame's end stores for it.
R1D_HD void r1d_prepare(const float L[3], const float albedo[3], float depth, const float normal[3], uint32_t hits, uint32_t flags, R1DenoiseCur &cur,
                        R1DenoiseGuide &g)
{
    const bool surf = hits > 0u;
    for (int c = 0; c < 3; ++c)
        cur.e[c] = surf ? L[c] / r1d_albedo(albedo[c], flags) : L[c];
    const float nn = (normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2];
    const float l = __builtin_sqrtf(nn);
    for (int c = 0; c < 3; ++c)
        g.nh[c] = l > 0.0f ? normal[c] / l : 0.0f;
    cur.m = surf ? depth / (float)hits : 0.0f;
    g.surf = surf ? 1.0f : 0.0f;
}

// The weight of a tap q of pixel p that is not the centre (the centre's weight is its h).  h: r1d_h(dy) * r1d_h(dx); k: normal_power_log2;
// sc2: the pass's (sigma_color * 2^-i)^2.
R1D_HD float r1d_weight(float h, const R1DenoiseCur &p, const R1DenoiseGuide &gp, const R1DenoiseCur &q, const R1DenoiseGuide &gq, uint32_t k, float sigma_depth,
                        float sc2)
{
    float c = (gp.nh[0] * gq.nh[0] + gp.nh[1] * gq.nh[1]) + gp.nh[2] * gq.nh[2];
    c = c < 0.0f ? 0.0f : c;
    c = c > 1.0f ? 1.0f : c;
    for (uint32_t j = 0; j < k; ++j)
        c = c * c;
    const float mx = p.m < q.m ? q.m : p.m;
    const float den = sigma_depth * mx;
    const float rz = den > 0.0f ? (p.m - q.m) / den : 0.0f;
    const float xz = rz * rz;
    const float dr = p.e[0] - q.e[0], dg = p.e[1] - q.e[1], db = p.e[2] - q.e[2];
    const float dc = (dr * dr + dg * dg) + db * db;
    const float xc = dc / sc2;
    return (h * c) / ((1.0f + xz) * (1.0f + xc));
}

// One tap into the sums: S_c = S_c + w * q_c (multiply, then add), W = W + w
R1D_HD void r1d_accumulate(float w, const R1DenoiseCur &q, float S[3], float &W)
{
    for (int c = 0; c < 3; ++c)
        S[c] = S[c] + w * q.e[c];
    W = W + w;
}

// The pass's colour scale: sigma_color * 2^-i, exact (or a correctly rounded subnormal, the same on both sides), squared
R1D_HD float r1d_sc2(float sigma_color, int i)
{
    const float sc = sigma_color * __builtin_bit_cast(float, (uint32_t)(127 - i) << 23);
    return sc * sc;
}

// ---- the variance-guided form (include/rays1.h "variance-guided denoised frames"): what it adds to the lines above ----
// The records stay as they are; the variance v of a pixel's demodulated value is one more float a pixel, ping and pong.  r1d_weight serves
// unchanged with r1d_den's value for sc2: xc = dc / den.

// Prepare: v = surf ? (V_r / (a_r * a_r) + V_g / (a_g * a_g)) + V_b / (a_b * a_b) : 0; V of a pixel without a hit is not used
R1D_HD float r1d_prepare_v(const float V[3], const float albedo[3], uint32_t hits, uint32_t flags)
{
    if (hits == 0u)
        return 0.0f;
    const float ar = r1d_albedo(albedo[0], flags), ag = r1d_albedo(albedo[1], flags), ab = r1d_albedo(albedo[2], flags);
    return (V[0] / (ar * ar) + V[1] / (ag * ag)) + V[2] / (ab * ab);
}

// The 3-tap table {1/4, 1/2, 1/4} at offset d = -1 .. 1, and one tap of the 3 x 3 prefilter of v: G = G + k * v_q, K = K + k
R1D_HD float r1d_k3(int d) { return d == 0 ? 0.5f : 0.25f; }
R1D_HD void r1d_prefilter_tap(float k, float vq, float &G, float &K)
{
    G = G + k * vq;
    K = K + k;
}

// The colour term's denominator of a pixel: sc2 * g + variance_floor, sc2 = sigma_color * sigma_color in every iteration
R1D_HD float r1d_den(float sc2, float g, float variance_floor) { return sc2 * g + variance_floor; }

// One tap into the variance sum: T = T + (w * w) * v_q
R1D_HD void r1d_accumulate_v(float w, float vq, float &T) { T = T + (w * w) * vq; }

// ---- what the kernels read and write (r1_denoise_kernels.hip), device memory; by value in their arguments ----
// A workgroup of 256 threads owns one 32 x 8 tile of the frame (r1_tile.h's geometry: tiles numbered row by row, slot = ly * 32 + lx, edge
// tiles cut by the image); a thread owns one pixel.  The records are dense, width apart; only L, f and out have the caller's strides.
#define R1D_TILE_W 32
#define R1D_TILE_H 8
#ifndef R1D_STAGE_MAX_STEP
#define R1D_STAGE_MAX_STEP 2 // the largest step whose taps a workgroup can stage in LDS: tile plus a halo of 2 * step pixels, (32 + 8) x (8 + 8) records of 32 bytes
#endif
#define R1D_STAGE_DEFAULT_MAX_STEP 2 // ... and the largest step the library stages (r1_denoise.cpp; measured)
struct R1DenoiseArgs
{
    const float *L;             // prepare: the linear frame, 3 floats a pixel, rows linear_stride pixels apart
    const float *f;             // prepare and the last pass: the feature frame, 8 words a pixel, rows feature_stride pixels apart (16-byte aligned)
    const R1DenoiseCur *cur;    // a pass: what it reads ...
    R1DenoiseCur *next;         // ... and writes (prepare: the first pass's `cur`); unused by the last pass
    R1DenoiseGuide *guide;      // written by prepare, read by every pass
    float *out;                 // the last pass: 3 floats a pixel, rows out_stride pixels apart; may be L
    int32_t width, height;
    uint32_t linear_stride, feature_stride, out_stride;
    uint32_t flags, k;
    float sigma_depth, sc2;
    int32_t step;
};

// The guided kernels (r1_vfilter_*): the same records and fields (d.sc2: sigma_color squared), and the variance beside them
struct R1VFilterArgs
{
    R1DenoiseArgs d;
    const float *V;             // prepare: the variance frame, 4 words a pixel {var r, g, b, samples}, rows moment_stride pixels apart (16-byte aligned)
    const float *v_cur;         // a pass: one float a pixel, dense ...
    float *v_next;              // ... and what it writes (prepare: the first pass's v_cur); unused by the last pass
    uint32_t moment_stride;
    float variance_floor;
};

#endif
