// r1_denoise_host.cpp — denoised frames without a device (include/rays1.h "denoised frames"): r1_denoise_check, the one place
// the rules of a frame and of the options are tested, and r1_denoise_host, the definition the device forms (r1_denoise.cpp, r1_denoise_kernels.hip)
// are held to bit for bit.  The arithmetic is r1_denoise.h's: the kernels call the same lines.  No HIP runtime call here:
// tools/check_denoise_host.cpp links this file alone.
#include <math.h>
#include <string.h>

#include <new>
#include <vector>

#include "r1_denoise.h"
#include "r1_internal.h"

static_assert(R1_DENOISE_DEMODULATE == R1D_DEMODULATE, "r1_denoise.h reads the public flag");
static_assert(sizeof(r1_feature) == 32, "a feature record is eight words");

extern "C" int r1_denoise_check(const r1_denoise_frame *fr, const r1_denoise_opt *o)
{
    if (!fr || !o)
    {
        r1_set_error("r1_denoise_check: %s is NULL", !fr ? "frame" : "options");
        return R1_EINVAL;
    }
    if (fr->width <= 0 || fr->height <= 0)
    {
        r1_set_error("r1_denoise_frame: %s %d is not positive", fr->width <= 0 ? "width" : "height", fr->width <= 0 ? fr->width : fr->height);
        return R1_EINVAL;
    }
    if ((int64_t)fr->width * fr->height >= (int64_t)1 << 31)
    {
        r1_set_error("r1_denoise_frame: a frame of %dx%d pixels exceeds 2^31", fr->width, fr->height);
        return R1_ELIMIT;
    }
    const int32_t strides[3] = {fr->linear_stride, fr->feature_stride, fr->out_stride};
    static const char *const names[3] = {"linear_stride", "feature_stride", "out_stride"};
    for (int i = 0; i < 3; ++i)
        if (strides[i] != 0 && strides[i] < fr->width)
        {
            r1_set_error("r1_denoise_frame: %s %d is neither 0 nor at least the width %d", names[i], strides[i], fr->width);
            return R1_EINVAL;
        }
    if (o->iterations < 1 || o->iterations > R1_DENOISE_MAX_ITERATIONS)
    {
        r1_set_error("r1_denoise_opt: iterations %d is not in 1..%d", o->iterations, R1_DENOISE_MAX_ITERATIONS);
        return R1_EINVAL;
    }
    if (o->normal_power_log2 < 0 || o->normal_power_log2 > R1_DENOISE_MAX_POWER_LOG2)
    {
        r1_set_error("r1_denoise_opt: normal_power_log2 %d is not in 0..%d", o->normal_power_log2, R1_DENOISE_MAX_POWER_LOG2);
        return R1_EINVAL;
    }
    if (!(o->sigma_color > 0.0f) || !(fabsf(o->sigma_color) <= 3.402823466e38f))
    {
        r1_set_error("r1_denoise_opt: sigma_color %g is not positive and finite", (double)o->sigma_color);
        return R1_EINVAL;
    }
    if (!(o->sigma_depth > 0.0f) || !(fabsf(o->sigma_depth) <= 3.402823466e38f))
    {
        r1_set_error("r1_denoise_opt: sigma_depth %g is not positive and finite", (double)o->sigma_depth);
        return R1_EINVAL;
    }
    if (o->flags & ~(uint32_t)R1_DENOISE_DEMODULATE)
    {
        r1_set_error("r1_denoise_opt: flags %u has bits other than R1_DENOISE_DEMODULATE", o->flags);
        return R1_EINVAL;
    }
    return R1_OK;
}

extern "C" int r1_denoise_host(const r1_denoise_frame *fr, const r1_denoise_opt *o, const float *L, const r1_feature *f, float *out)
{
    int rc = r1_denoise_check(fr, o);
    if (rc)
        return rc;
    if (!L || !f || !out)
    {
        r1_set_error("r1_denoise_host: %s is NULL", !L ? "L" : !f ? "f" : "out");
        return R1_EINVAL;
    }
    const int w = fr->width, h = fr->height;
    const size_t n = (size_t)w * h;
    const size_t ls = fr->linear_stride ? fr->linear_stride : w, fs = fr->feature_stride ? fr->feature_stride : w, os = fr->out_stride ? fr->out_stride : w;
    R1DenoiseCur *cur = new (std::nothrow) R1DenoiseCur[n], *next = new (std::nothrow) R1DenoiseCur[n];
    R1DenoiseGuide *guide = new (std::nothrow) R1DenoiseGuide[n];
    if (!cur || !next || !guide)
    {
        delete[] cur, delete[] next, delete[] guide;
        r1_set_error("r1_denoise_host: out of memory for a frame of %dx%d", w, h);
        return R1_ENOMEM;
    }
    // prepare: L is consumed here (out may be L)
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            const r1_feature &v = f[(size_t)y * fs + x];
            r1d_prepare(L + ((size_t)y * ls + x) * 3, v.albedo, v.depth, v.normal, v.hits, o->flags, cur[(size_t)y * w + x], guide[(size_t)y * w + x]);
        }
    const uint32_t k = (uint32_t)o->normal_power_log2;
    for (int i = 0; i < o->iterations; ++i)
    {
        const int step = 1 << i;
        const float sc2 = r1d_sc2(o->sigma_color, i);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
            {
                const size_t ip = (size_t)y * w + x;
                const R1DenoiseCur &p = cur[ip];
                const R1DenoiseGuide &gp = guide[ip];
                R1DenoiseCur nx = p;
                if (gp.surf != 0.0f)
                {
                    float S[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f;
                    for (int dy = -2; dy <= 2; ++dy)
                        for (int dx = -2; dx <= 2; ++dx)
                        {
                            const int qx = x + dx * step, qy = y + dy * step;
                            if (qx < 0 || qx >= w || qy < 0 || qy >= h)
                                continue;
                            const size_t iq = (size_t)qy * w + qx;
                            if (guide[iq].surf == 0.0f)
                                continue;
                            const float hh = r1d_h(dy) * r1d_h(dx);
                            const float wt = (dx == 0 && dy == 0) ? hh : r1d_weight(hh, p, gp, cur[iq], guide[iq], k, o->sigma_depth, sc2);
                            r1d_accumulate(wt, cur[iq], S, W);
                        }
                    for (int c = 0; c < 3; ++c)
                        nx.e[c] = S[c] / W;
                }
                next[ip] = nx;
            }
        R1DenoiseCur *t = cur;
        cur = next, next = t;
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            const size_t ip = (size_t)y * w + x;
            const r1_feature &v = f[(size_t)y * fs + x];
            float *o3 = out + ((size_t)y * os + x) * 3;
            for (int c = 0; c < 3; ++c)
                o3[c] = guide[ip].surf != 0.0f ? cur[ip].e[c] * r1d_albedo(v.albedo[c], o->flags) : cur[ip].e[c];
        }
    delete[] cur, delete[] next, delete[] guide;
    return R1_OK;
}
