// r1_denoise_host.cpp — both a-trous filters without a device (include/rays1.h "denoised frames" and "variance-guided denoised frames",
// DESIGN.md §4.39, §4.40): r1_denoise_check and r1_denoise_guided_check, the one place the rules of a frame and of the options are tested, and
// r1_denoise_host and r1_denoise_guided_host, the definitions the device forms (r1_denoise.cpp, r1_denoise_kernels.hip) are held to bit for
// bit.  The two host forms are one loop (filter_host): the guided one is the unguided one with a variance frame.  The arithmetic is
// r1_denoise.h's: the kernels call the same lines.  No HIP runtime call here: tools/check_denoise_host.cpp and
// tools/check_denoise_guided_host.cpp link this file alone.
#include <math.h>

#include <memory>
#include <new>
#include <utility>

#include "r1_denoise.h"
#include "r1_internal.h"

static_assert(R1_DENOISE_DEMODULATE == R1D_DEMODULATE, "r1_denoise.h reads the public flag");
static_assert(sizeof(r1_feature) == 32, "a feature record is eight words");
static_assert(sizeof(r1_moment) == 16, "a moment record is four words");

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

// Both host forms; `who` has passed its check.  V, its stride ms and the floor: the guided form's (V == nullptr: the unguided one, which has no
// v, scales sigma_color by 2^-i from pass to pass and leaves the prefilter out).
static int filter_host(const char *who, const r1_denoise_frame *fr, const r1_denoise_opt *o, const float *L, const r1_feature *f, const r1_moment *V, size_t ms,
                       float variance_floor, float *out)
{
    const bool guided = V != nullptr;
    const int w = fr->width, h = fr->height;
    const size_t n = (size_t)w * h;
    const size_t ls = fr->linear_stride ? fr->linear_stride : w, fs = fr->feature_stride ? fr->feature_stride : w, os = fr->out_stride ? fr->out_stride : w;
    std::unique_ptr<R1DenoiseCur[]> cur(new (std::nothrow) R1DenoiseCur[n]), next(new (std::nothrow) R1DenoiseCur[n]);
    std::unique_ptr<R1DenoiseGuide[]> guide(new (std::nothrow) R1DenoiseGuide[n]);
    std::unique_ptr<float[]> v(guided ? new (std::nothrow) float[n] : nullptr), vn(guided ? new (std::nothrow) float[n] : nullptr);
    if (!cur || !next || !guide || (guided && (!v || !vn)))
    {
        r1_set_error("%s: out of memory for a frame of %dx%d", who, w, h);
        return R1_ENOMEM;
    }
    // prepare: L is consumed here (out may be L)
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            const r1_feature &ft = f[(size_t)y * fs + x];
            const size_t ip = (size_t)y * w + x;
            r1d_prepare(L + ((size_t)y * ls + x) * 3, ft.albedo, ft.depth, ft.normal, ft.hits, o->flags, cur[ip], guide[ip]);
            if (guided)
                v[ip] = r1d_prepare_v(V[(size_t)y * ms + x].var, ft.albedo, ft.hits, o->flags);
        }
    const uint32_t k = (uint32_t)o->normal_power_log2;
    for (int i = 0; i < o->iterations; ++i)
    {
        const int step = 1 << i;
        const float sc2 = guided ? o->sigma_color * o->sigma_color : r1d_sc2(o->sigma_color, i);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
            {
                const size_t ip = (size_t)y * w + x;
                const R1DenoiseCur &p = cur[ip];
                const R1DenoiseGuide &gp = guide[ip];
                R1DenoiseCur nx = p;
                float vx = guided ? v[ip] : 0.0f; // (0 for a pixel without a hit, and it stays 0)
                if (gp.surf != 0.0f)
                {
                    float den = sc2; // the colour term's denominator; guided: the pixel's own, from the 3 x 3 prefilter of v
                    if (guided)
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
                        den = r1d_den(sc2, G / K, variance_floor);
                    }
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
                            if (guided)
                                r1d_accumulate_v(wt, v[iq], T);
                        }
                    for (int c = 0; c < 3; ++c)
                        nx.e[c] = S[c] / W;
                    if (guided)
                        vx = T / (W * W);
                }
                next[ip] = nx;
                if (guided)
                    vn[ip] = vx;
            }
        std::swap(cur, next);
        std::swap(v, vn);
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
    return filter_host("r1_denoise_host", fr, o, L, f, nullptr, 0, 0.0f, out);
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
    const r1_denoise_frame base = {fr->width, fr->height, fr->linear_stride, fr->feature_stride, fr->out_stride};
    return filter_host("r1_denoise_guided_host", &base, &go->base, L, f, V, fr->moment_stride ? (size_t)fr->moment_stride : (size_t)fr->width, go->variance_floor, out);
}
