// r1_denoise_guided_host.cpp — variance-guided denoised frames without a device (include/rays1.h "variance-guided denoised frames",
// DESIGN.md §4.40): r1_denoise_guided_check and r1_denoise_guided_host, the definition the device forms (r1_denoise.cpp,
// r1_vfilter_kernels.hip) are held to bit for bit.  The arithmetic is r1_denoise.h's; the base rules are r1_denoise_check's
// (r1_denoise_host.cpp).  No HIP runtime call here.
#include <math.h>

#include <new>

#include "r1_denoise.h"
#include "r1_internal.h"

static_assert(sizeof(r1_moment) == 16, "a moment record is four words");

extern "C" int r1_denoise_guided_check(const r1_denoise_guided_frame *fr, const r1_denoise_guided_opt *o)
{
    if (!fr || !o)
    {
        r1_set_error("r1_denoise_guided_check: %s is NULL", !fr ? "frame" : "options");
        return R1_EINVAL;
    }
    const r1_denoise_frame base = {fr->width, fr->height, fr->linear_stride, fr->feature_stride, fr->out_stride};
    int rc = r1_denoise_check(&base, &o->base);
    if (rc)
        return rc;
    if (fr->moment_stride != 0 && fr->moment_stride < fr->width)
    {
        r1_set_error("r1_denoise_guided_frame: moment_stride %d is neither 0 nor at least the width %d", fr->moment_stride, fr->width);
        return R1_EINVAL;
    }
    if (!(o->variance_floor > 0.0f) || !(fabsf(o->variance_floor) <= 3.402823466e38f))
    {
        r1_set_error("r1_denoise_guided_opt: variance_floor %g is not positive and finite", (double)o->variance_floor);
        return R1_EINVAL;
    }
    if (o->reserved != 0u)
    {
        r1_set_error("r1_denoise_guided_opt: reserved %u is not 0", o->reserved);
        return R1_EINVAL;
    }
    return R1_OK;
}

extern "C" int r1_denoise_guided_host(const r1_denoise_guided_frame *fr, const r1_denoise_guided_opt *go, const float *L, const r1_feature *f, const r1_moment *V,
                                      float *out)
{
    int rc = r1_denoise_guided_check(fr, go);
    if (rc)
        return rc;
    if (!L || !f || !V || !out)
    {
        r1_set_error("r1_denoise_guided_host: %s is NULL", !L ? "L" : !f ? "f" : !V ? "V" : "out");
        return R1_EINVAL;
    }
    const r1_denoise_opt *o = &go->base;
    const int w = fr->width, h = fr->height;
    const size_t n = (size_t)w * h;
    const size_t ls = fr->linear_stride ? fr->linear_stride : w, fs = fr->feature_stride ? fr->feature_stride : w, os = fr->out_stride ? fr->out_stride : w;
    const size_t ms = fr->moment_stride ? fr->moment_stride : w;
    R1DenoiseCur *cur = new (std::nothrow) R1DenoiseCur[n], *next = new (std::nothrow) R1DenoiseCur[n];
    R1DenoiseGuide *guide = new (std::nothrow) R1DenoiseGuide[n];
    float *v = new (std::nothrow) float[n], *vn = new (std::nothrow) float[n];
    if (!cur || !next || !guide || !v || !vn)
    {
        delete[] cur, delete[] next, delete[] guide, delete[] v, delete[] vn;
        r1_set_error("r1_denoise_guided_host: out of memory for a frame of %dx%d", w, h);
        return R1_ENOMEM;
    }
    // prepare: L is consumed here (out may be L)
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            const r1_feature &ft = f[(size_t)y * fs + x];
            const size_t ip = (size_t)y * w + x;
            r1d_prepare(L + ((size_t)y * ls + x) * 3, ft.albedo, ft.depth, ft.normal, ft.hits, o->flags, cur[ip], guide[ip]);
            v[ip] = r1d_prepare_v(V[(size_t)y * ms + x].var, ft.albedo, ft.hits, o->flags);
        }
    const uint32_t k = (uint32_t)o->normal_power_log2;
    const float sc2 = o->sigma_color * o->sigma_color;
    for (int i = 0; i < o->iterations; ++i)
    {
        const int step = 1 << i;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
            {
                const size_t ip = (size_t)y * w + x;
                const R1DenoiseCur &p = cur[ip];
                const R1DenoiseGuide &gp = guide[ip];
                R1DenoiseCur nx = p;
                float vx = v[ip]; // (0 for a pixel without a hit, and it stays 0)
                if (gp.surf != 0.0f)
                {
                    float G = 0.0f, K = 0.0f;
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx)
                        {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qx >= w || qy < 0 || qy >= h)
                                continue;
                            const size_t iq = (size_t)qy * w + qx;
                            if (guide[iq].surf == 0.0f)
                                continue;
                            r1d_prefilter_tap(r1d_k3(dy) * r1d_k3(dx), v[iq], G, K);
                        }
                    const float den = r1d_den(sc2, G / K, go->variance_floor);
                    float S[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f, T = 0.0f;
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
                            const float wt = (dx == 0 && dy == 0) ? hh : r1d_weight(hh, p, gp, cur[iq], guide[iq], k, o->sigma_depth, den);
                            r1d_accumulate(wt, cur[iq], S, W);
                            r1d_accumulate_v(wt, v[iq], T);
                        }
                    for (int c = 0; c < 3; ++c)
                        nx.e[c] = S[c] / W;
                    vx = T / (W * W);
                }
                next[ip] = nx, vn[ip] = vx;
            }
        R1DenoiseCur *t = cur;
        cur = next, next = t;
        float *tv = v;
        v = vn, vn = tv;
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            const size_t ip = (size_t)y * w + x;
            const r1_feature &ft = f[(size_t)y * fs + x];
            float *o3 = out + ((size_t)y * os + x) * 3;
            for (int c = 0; c < 3; ++c)
                o3[c] = guide[ip].surf != 0.0f ? cur[ip].e[c] * r1d_albedo(ft.albedo[c], o->flags) : cur[ip].e[c];
        }
    delete[] cur, delete[] next, delete[] guide, delete[] v, delete[] vn;
    return R1_OK;
}
