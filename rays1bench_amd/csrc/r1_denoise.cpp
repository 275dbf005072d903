// r1_denoise.cpp — denoised frames on the device (include/rays1.h "denoised frames"): r1_denoise_device enqueues the prepare
// kernel and one pass kernel per iteration (r1_denoise_kernels.hip) over the context's workspace; r1_denoise is the same on host memory;
// r1_render_denoised* compose r1_render_linear_device + r1_render_features_device + the filter on one stream.  The rules are checked in
// r1_denoise_check (r1_denoise_host.cpp), the arithmetic is r1_denoise.h's.  Like a query, the filter touches none of the state a render reads.
#include <string.h>

#include "r1_context.h"
#include "r1_denoise.h"

// The context's workspace: a 256-byte head (the ray count of a composed render), the filter's records — ping, pong, guide: 48 bytes a pixel —
// and, for the forms that own their inputs, a dense feature frame and a dense linear frame.
struct DenoiseLayout
{
    size_t cur[2], guide, features, linear, bytes;
};
static DenoiseLayout denoise_layout(size_t n, bool with_inputs)
{
    DenoiseLayout l;
    l.cur[0] = 256, l.cur[1] = l.cur[0] + 16 * n, l.guide = l.cur[1] + 16 * n;
    l.features = l.guide + 16 * n, l.linear = l.features + 32 * n;
    l.bytes = with_inputs ? l.linear + 12 * n : l.features;
    return l;
}

static int pointers_check(const char *who, const void *L, const void *f, const void *out, bool device)
{
    if (!L || !f || !out)
    {
        r1_set_error("%s: %s is NULL", who, !L ? "L" : !f ? "f" : "out");
        return R1_EINVAL;
    }
    if (device && (((uintptr_t)L & 3u) || ((uintptr_t)out & 3u) || ((uintptr_t)f & 15u)))
    {
        r1_set_error("%s: d_L and d_out must be 4-byte aligned and d_f 16-byte aligned", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

// Enqueues the filter on `st`; every check has passed and the workspace holds at least denoise_layout(n, .).  The passes of the small steps
// stage their taps in LDS (DESIGN.md §4.39 has the measurement that put the limit where it is).
static int denoise_enqueue(r1_context *c, const r1_denoise_frame *fr, const r1_denoise_opt *o, const void *d_L, const void *d_f, void *d_out, hipStream_t st)
{
    const DenoiseLayout l = denoise_layout((size_t)fr->width * fr->height, false);
    char *const ws = (char *)c->denoise_ws.p;
    R1DenoiseArgs a;
    memset(&a, 0, sizeof(a));
    a.L = (const float *)d_L, a.f = (const float *)d_f, a.out = (float *)d_out;
    a.guide = (R1DenoiseGuide *)(ws + l.guide);
    a.width = fr->width, a.height = fr->height;
    a.linear_stride = (uint32_t)(fr->linear_stride ? fr->linear_stride : fr->width);
    a.feature_stride = (uint32_t)(fr->feature_stride ? fr->feature_stride : fr->width);
    a.out_stride = (uint32_t)(fr->out_stride ? fr->out_stride : fr->width);
    a.flags = o->flags, a.k = (uint32_t)o->normal_power_log2, a.sigma_depth = o->sigma_depth;
    a.next = (R1DenoiseCur *)(ws + l.cur[0]);
    R1_HIP(r1_launch_denoise_prepare(&a, st));
    static const int stage_max = (int)r1_knob("R1_DENOISE_STAGE_MAX_STEP", R1D_STAGE_DEFAULT_MAX_STEP); // tuning library only; 0: every pass loads its taps directly
    for (int i = 0; i < o->iterations; ++i)
    {
        a.step = 1 << i, a.sc2 = r1d_sc2(o->sigma_color, i);
        a.cur = (const R1DenoiseCur *)(ws + l.cur[i & 1]), a.next = (R1DenoiseCur *)(ws + l.cur[(i + 1) & 1]);
        R1_HIP(r1_launch_denoise_pass(&a, a.step <= stage_max && a.step <= R1D_STAGE_MAX_STEP, i == o->iterations - 1, st));
    }
    return R1_OK;
}

extern "C" int r1_denoise_device(r1_context *c, const r1_denoise_frame *fr, const r1_denoise_opt *o, const void *d_L, const void *d_f, void *d_out,
                                 void *hip_stream)
{
    if (!c)
    {
        r1_set_error("r1_denoise_device: ctx is NULL");
        return R1_EINVAL;
    }
    int rc = r1_denoise_check(fr, o);
    if (rc || (rc = pointers_check("r1_denoise_device", d_L, d_f, d_out, true)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = ensure(c->denoise_ws, denoise_layout((size_t)fr->width * fr->height, false).bytes)))
        return rc;
    return denoise_enqueue(c, fr, o, d_L, d_f, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

// (timed_sync, the two events around a call's device work: r1_context.h)
extern "C" int r1_denoise(r1_context *c, const r1_denoise_frame *fr, const r1_denoise_opt *o, const float *L, const r1_feature *f, float *out,
                          double *device_seconds_out)
{
    if (!c)
    {
        r1_set_error("r1_denoise: ctx is NULL");
        return R1_EINVAL;
    }
    int rc = r1_denoise_check(fr, o);
    if (rc || (rc = pointers_check("r1_denoise", L, f, out, false)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    const size_t w = (size_t)fr->width, h = (size_t)fr->height;
    const DenoiseLayout l = denoise_layout(w * h, true);
    if ((rc = ensure(c->denoise_ws, l.bytes)))
        return rc;
    char *const ws = (char *)c->denoise_ws.p;
    const size_t ls = fr->linear_stride ? fr->linear_stride : w, fs = fr->feature_stride ? fr->feature_stride : w, os = fr->out_stride ? fr->out_stride : w;
    // the caller's rows go up densely, the filter works in place on the dense linear frame, its rows come home with the caller's stride
    R1_HIP(hipMemcpy2DAsync(ws + l.linear, w * 12, L, ls * 12, w * 12, h, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpy2DAsync(ws + l.features, w * sizeof(r1_feature), f, fs * sizeof(r1_feature), w * sizeof(r1_feature), h, hipMemcpyHostToDevice, c->stream));
    const r1_denoise_frame dense = {fr->width, fr->height, 0, 0, 0};
    if ((rc = timed_sync(c, "r1_denoise", device_seconds_out, [&] { return denoise_enqueue(c, &dense, o, ws + l.linear, ws + l.features, ws + l.linear, c->stream); })))
        return rc;
    R1_HIP(hipMemcpy2DAsync(out, os * 12, ws + l.linear, w * 12, w * 12, h, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

// ---- a frame rendered and denoised ---------------------------------------------------------------------------------------------------------

// What both composed forms refuse before anything is enqueued, in the documented order up to the pointers; *fr: the whole frame, dense
static int composed_check(const char *who, const r1_context *c, const r1_params *p, const r1_denoise_opt *o, r1_denoise_frame *fr)
{
    if (!c)
    {
        r1_set_error("%s: ctx is NULL", who);
        return R1_EINVAL;
    }
    if (!p || !o)
    {
        r1_set_error("%s: %s is NULL", who, !p ? "params" : "options");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    const r1_denoise_frame whole = {p->width, p->height, 0, 0, 0};
    *fr = whole;
    if ((rc = r1_denoise_check(fr, o)))
        return rc;
    if (p->variant != R1_VARIANT_DEFAULT && p->variant != R1_VARIANT_BVH && p->variant != R1_VARIANT_GRID && p->variant != R1_VARIANT_REFERENCE)
    {
        r1_set_error("%s: variant %d renders no feature frame (DEFAULT, BVH, GRID and REFERENCE do)", who, p->variant);
        return R1_EINVAL;
    }
    return R1_OK;
}

// The three parts on `st`.  The linear render comes first: what it refuses (no scene, shards, a moved scene's stale tables) is refused
// before anything is enqueued, and the feature frame refuses nothing the render has passed.
static int composed_enqueue(r1_context *c, const r1_params *p, const r1_denoise_opt *o, const r1_denoise_frame *fr, void *d_rgb, void *d_rays, hipStream_t st)
{
    int rc = r1_render_linear_device(c, p, d_rgb, d_rays, st);
    if (rc)
        return rc;
    // (the workspace was sized by the caller: r1_render_linear_device allocates nothing of it)
    void *const d_f = (char *)c->denoise_ws.p + denoise_layout((size_t)fr->width * fr->height, true).features;
    if ((rc = r1_render_features_device(c, p, nullptr, d_f, st)))
        return rc;
    return denoise_enqueue(c, fr, o, d_rgb, d_f, d_rgb, st);
}

extern "C" int r1_render_denoised_device(r1_context *c, const r1_params *p, const r1_denoise_opt *o, void *d_rgb_f32, void *d_num_rays, void *hip_stream)
{
    r1_denoise_frame fr;
    int rc = composed_check("r1_render_denoised_device", c, p, o, &fr);
    if (rc)
        return rc;
    if (!d_rgb_f32 || !d_num_rays || ((uintptr_t)d_rgb_f32 & 3u) || ((uintptr_t)d_num_rays & 7u))
    {
        r1_set_error("r1_render_denoised_device: d_rgb_f32 must be non-NULL and 4-byte aligned, d_num_rays non-NULL and 8-byte aligned");
        return R1_EINVAL;
    }
    if (!c->have_scene) // (before the workspace is grown: a refused call changes nothing)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    if ((rc = ensure(c->denoise_ws, denoise_layout((size_t)fr.width * fr.height, true).bytes)))
        return rc;
    return composed_enqueue(c, p, o, &fr, d_rgb_f32, d_num_rays, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_render_denoised(r1_context *c, const r1_params *p, const r1_denoise_opt *o, float *rgb_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    r1_denoise_frame fr;
    int rc = composed_check("r1_render_denoised", c, p, o, &fr);
    if (rc)
        return rc;
    if (!rgb_out)
    {
        r1_set_error("r1_render_denoised: rgb_out is NULL");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)fr.width * fr.height;
    const DenoiseLayout l = denoise_layout(n, true);
    if ((rc = ensure(c->denoise_ws, l.bytes)))
        return rc;
    char *const ws = (char *)c->denoise_ws.p;
    if ((rc = timed_sync(c, "r1_render_denoised", device_seconds_out, [&] { return composed_enqueue(c, p, o, &fr, ws + l.linear, ws, c->stream); })))
        return rc;
    uint64_t rays = 0;
    R1_HIP(hipMemcpyAsync(rgb_out, ws + l.linear, n * 12, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipMemcpyAsync(&rays, ws, 8, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    if ((rc = land_check(c)))
        return rc;
    if (num_rays_out)
        *num_rays_out = rays;
    return R1_OK;
}

// ---- the variance-guided form (include/rays1.h "variance-guided denoised frames") -------------------------------------------
// The same workspace with more in it: behind the unguided layout's inputs the two dense v arrays (4 bytes a pixel each) and, for the forms
// that own their inputs, a dense variance frame.  The unguided forms never look that far, so the two filters share the allocation.
struct GuidedLayout
{
    DenoiseLayout d;
    size_t v[2], moments, bytes;
};
static GuidedLayout guided_layout(size_t n, bool with_inputs)
{
    GuidedLayout l;
    l.d = denoise_layout(n, true);
    l.v[0] = l.d.bytes, l.v[1] = l.v[0] + 4 * n;
    l.moments = (l.v[1] + 4 * n + 15) & ~(size_t)15;
    l.bytes = with_inputs ? l.moments + 16 * n : l.moments;
    return l;
}

static int guided_enqueue(r1_context *c, const r1_denoise_guided_frame *fr, const r1_denoise_guided_opt *go, const void *d_L, const void *d_f, const void *d_V,
                          void *d_out, hipStream_t st)
{
    const r1_denoise_opt *o = &go->base;
    const GuidedLayout l = guided_layout((size_t)fr->width * fr->height, false);
    char *const ws = (char *)c->denoise_ws.p;
    R1VFilterArgs b;
    memset(&b, 0, sizeof(b));
    R1DenoiseArgs &a = b.d;
    a.L = (const float *)d_L, a.f = (const float *)d_f, a.out = (float *)d_out;
    a.guide = (R1DenoiseGuide *)(ws + l.d.guide);
    a.width = fr->width, a.height = fr->height;
    a.linear_stride = (uint32_t)(fr->linear_stride ? fr->linear_stride : fr->width);
    a.feature_stride = (uint32_t)(fr->feature_stride ? fr->feature_stride : fr->width);
    a.out_stride = (uint32_t)(fr->out_stride ? fr->out_stride : fr->width);
    a.flags = o->flags, a.k = (uint32_t)o->normal_power_log2, a.sigma_depth = o->sigma_depth;
    a.sc2 = o->sigma_color * o->sigma_color; // in every iteration
    b.V = (const float *)d_V, b.moment_stride = (uint32_t)(fr->moment_stride ? fr->moment_stride : fr->width);
    b.variance_floor = go->variance_floor;
    a.next = (R1DenoiseCur *)(ws + l.d.cur[0]), b.v_next = (float *)(ws + l.v[0]);
    R1_HIP(r1_launch_vfilter_prepare(&b, st));
    // tuning library only; 0: every pass loads its taps directly.  The default is the unguided filter's, not yet measured for these kernels
    static const int stage_max = (int)r1_knob("R1_VFILTER_STAGE_MAX_STEP", R1D_STAGE_DEFAULT_MAX_STEP);
    for (int i = 0; i < o->iterations; ++i)
    {
        a.step = 1 << i;
        a.cur = (const R1DenoiseCur *)(ws + l.d.cur[i & 1]), a.next = (R1DenoiseCur *)(ws + l.d.cur[(i + 1) & 1]);
        b.v_cur = (const float *)(ws + l.v[i & 1]), b.v_next = (float *)(ws + l.v[(i + 1) & 1]);
        R1_HIP(r1_launch_vfilter_pass(&b, a.step <= stage_max && a.step <= R1D_STAGE_MAX_STEP, i == o->iterations - 1, st));
    }
    return R1_OK;
}

static int guided_pointers_check(const char *who, const void *L, const void *f, const void *V, const void *out, bool device)
{
    if (!L || !f || !V || !out)
    {
        r1_set_error("%s: %s is NULL", who, !L ? "L" : !f ? "f" : !V ? "V" : "out");
        return R1_EINVAL;
    }
    if (device && (((uintptr_t)L & 3u) || ((uintptr_t)out & 3u) || ((uintptr_t)f & 15u) || ((uintptr_t)V & 15u)))
    {
        r1_set_error("%s: d_L and d_out must be 4-byte aligned, d_f and d_V 16-byte aligned", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

extern "C" int r1_denoise_guided_device(r1_context *c, const r1_denoise_guided_frame *fr, const r1_denoise_guided_opt *o, const void *d_L, const void *d_f,
                                        const void *d_V, void *d_out, void *hip_stream)
{
    if (!c)
    {
        r1_set_error("r1_denoise_guided_device: ctx is NULL");
        return R1_EINVAL;
    }
    int rc = r1_denoise_guided_check(fr, o);
    if (rc || (rc = guided_pointers_check("r1_denoise_guided_device", d_L, d_f, d_V, d_out, true)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = ensure(c->denoise_ws, guided_layout((size_t)fr->width * fr->height, false).bytes)))
        return rc;
    return guided_enqueue(c, fr, o, d_L, d_f, d_V, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_denoise_guided(r1_context *c, const r1_denoise_guided_frame *fr, const r1_denoise_guided_opt *o, const float *L, const r1_feature *f,
                                 const r1_moment *V, float *out, double *device_seconds_out)
{
    if (!c)
    {
        r1_set_error("r1_denoise_guided: ctx is NULL");
        return R1_EINVAL;
    }
    int rc = r1_denoise_guided_check(fr, o);
    if (rc || (rc = guided_pointers_check("r1_denoise_guided", L, f, V, out, false)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    const size_t w = (size_t)fr->width, h = (size_t)fr->height;
    const GuidedLayout l = guided_layout(w * h, true);
    if ((rc = ensure(c->denoise_ws, l.bytes)))
        return rc;
    char *const ws = (char *)c->denoise_ws.p;
    const size_t ls = fr->linear_stride ? fr->linear_stride : w, fs = fr->feature_stride ? fr->feature_stride : w, os = fr->out_stride ? fr->out_stride : w;
    const size_t ms = fr->moment_stride ? fr->moment_stride : w;
    R1_HIP(hipMemcpy2DAsync(ws + l.d.linear, w * 12, L, ls * 12, w * 12, h, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpy2DAsync(ws + l.d.features, w * sizeof(r1_feature), f, fs * sizeof(r1_feature), w * sizeof(r1_feature), h, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpy2DAsync(ws + l.moments, w * sizeof(r1_moment), V, ms * sizeof(r1_moment), w * sizeof(r1_moment), h, hipMemcpyHostToDevice, c->stream));
    const r1_denoise_guided_frame dense = {fr->width, fr->height, 0, 0, 0, 0};
    if ((rc = timed_sync(c, "r1_denoise_guided", device_seconds_out,
                         [&] { return guided_enqueue(c, &dense, o, ws + l.d.linear, ws + l.d.features, ws + l.moments, ws + l.d.linear, c->stream); })))
        return rc;
    R1_HIP(hipMemcpy2DAsync(out, os * 12, ws + l.d.linear, w * 12, w * 12, h, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

// What both composed guided forms refuse before anything is enqueued: the unguided forms' list, the guided options, and one sample
static int guided_composed_check(const char *who, const r1_context *c, const r1_params *p, const r1_denoise_guided_opt *o, r1_denoise_guided_frame *fr)
{
    r1_denoise_frame base;
    int rc = composed_check(who, c, p, o ? &o->base : nullptr, &base);
    if (rc)
        return rc;
    const r1_denoise_guided_frame whole = {p->width, p->height, 0, 0, 0, 0};
    *fr = whole;
    if ((rc = r1_denoise_guided_check(fr, o)))
        return rc;
    if (p->spp < 2)
    {
        r1_set_error("%s: spp %d carries no variance (at least 2; r1_render_denoised serves one sample)", who, p->spp);
        return R1_EINVAL;
    }
    return R1_OK;
}

static int guided_composed_enqueue(r1_context *c, const r1_params *p, const r1_denoise_guided_opt *o, const r1_denoise_guided_frame *fr, void *d_rgb, void *d_rays,
                                   hipStream_t st)
{
    const GuidedLayout l = guided_layout((size_t)fr->width * fr->height, true);
    char *const ws = (char *)c->denoise_ws.p; // (sized by the caller: the two renders allocate nothing of it)
    int rc = r1_render_moments_device(c, p, d_rgb, ws + l.moments, d_rays, st);
    if (rc || (rc = r1_render_features_device(c, p, nullptr, ws + l.d.features, st)))
        return rc;
    return guided_enqueue(c, fr, o, d_rgb, ws + l.d.features, ws + l.moments, d_rgb, st);
}

extern "C" int r1_render_denoised_guided_device(r1_context *c, const r1_params *p, const r1_denoise_guided_opt *o, void *d_rgb_f32, void *d_num_rays, void *hip_stream)
{
    r1_denoise_guided_frame fr;
    int rc = guided_composed_check("r1_render_denoised_guided_device", c, p, o, &fr);
    if (rc)
        return rc;
    if (!d_rgb_f32 || !d_num_rays || ((uintptr_t)d_rgb_f32 & 3u) || ((uintptr_t)d_num_rays & 7u))
    {
        r1_set_error("r1_render_denoised_guided_device: d_rgb_f32 must be non-NULL and 4-byte aligned, d_num_rays non-NULL and 8-byte aligned");
        return R1_EINVAL;
    }
    if (!c->have_scene) // (before the workspace is grown: a refused call changes nothing)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    if ((rc = ensure(c->denoise_ws, guided_layout((size_t)fr.width * fr.height, true).bytes)))
        return rc;
    return guided_composed_enqueue(c, p, o, &fr, d_rgb_f32, d_num_rays, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_render_denoised_guided(r1_context *c, const r1_params *p, const r1_denoise_guided_opt *o, float *rgb_out, uint64_t *num_rays_out,
                                         double *device_seconds_out)
{
    r1_denoise_guided_frame fr;
    int rc = guided_composed_check("r1_render_denoised_guided", c, p, o, &fr);
    if (rc)
        return rc;
    if (!rgb_out)
    {
        r1_set_error("r1_render_denoised_guided: rgb_out is NULL");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)fr.width * fr.height;
    const GuidedLayout l = guided_layout(n, true);
    if ((rc = ensure(c->denoise_ws, l.bytes)))
        return rc;
    char *const ws = (char *)c->denoise_ws.p;
    if ((rc = timed_sync(c, "r1_render_denoised_guided", device_seconds_out,
                         [&] { return guided_composed_enqueue(c, p, o, &fr, ws + l.d.linear, ws, c->stream); })))
        return rc;
    uint64_t rays = 0;
    R1_HIP(hipMemcpyAsync(rgb_out, ws + l.d.linear, n * 12, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipMemcpyAsync(&rays, ws, 8, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    if ((rc = land_check(c)))
        return rc;
    if (num_rays_out)
        *num_rays_out = rays;
    return R1_OK;
}
