// r1_denoise.cpp — both a-trous filters on the device (include/rays1.h "denoised frames" and "variance-guided denoised frames", DESIGN.md §4.39,
// §4.40): r1_denoise_device and r1_denoise_guided_device enqueue the prepare kernel and one pass kernel per iteration (r1_denoise_kernels.hip)
// over the context's workspace; r1_denoise and r1_denoise_guided are the same on host memory; r1_render_denoised* compose a linear or a
// variance frame + r1_render_features_device + the filter on one stream.  Inside this file there is one filter: the unguided one is the guided
// one without a variance frame (Filter).  The rules are checked in r1_denoise_check and r1_denoise_guided_check (r1_denoise_host.cpp), the
// arithmetic is r1_denoise.h's.  Like a query, the filter touches none of the state a render reads.
#include <string.h>

#include "r1_context.h"
#include "r1_denoise.h"

// A call of either filter, its check passed: the guided form's frame and options; the unguided form has no V, no moment_stride, no floor
struct Filter
{
    bool guided;
    r1_denoise_guided_frame fr;
    r1_denoise_guided_opt o;
};
static Filter unguided_filter(const r1_denoise_frame &fr, const r1_denoise_opt &o)
{
    return {false, {fr.width, fr.height, fr.linear_stride, fr.feature_stride, 0, fr.out_stride}, {o, 0.0f, 0u}};
}

// The context's workspace: a 256-byte head (the ray count of a composed render), the filter's records — ping, pong, guide: 48 bytes a pixel —
// and, for the forms that own their inputs, a dense feature frame and a dense linear frame.  The guided filter has more in the same
// allocation: behind those inputs the two dense v arrays (4 bytes a pixel each) and, for the forms that own their inputs, a dense variance
// frame.  The unguided forms never look that far and never ask for it.
struct Layout
{
    size_t cur[2], guide, features, linear, v[2], moments, bytes;
};
static Layout layout(size_t n, bool guided, bool with_inputs)
{
    Layout l;
    l.cur[0] = 256, l.cur[1] = l.cur[0] + 16 * n, l.guide = l.cur[1] + 16 * n;
    l.features = l.guide + 16 * n, l.linear = l.features + 32 * n;
    l.v[0] = l.linear + 12 * n, l.v[1] = l.v[0] + 4 * n;
    l.moments = (l.v[1] + 4 * n + 15) & ~(size_t)15;
    if (guided)
        l.bytes = with_inputs ? l.moments + 16 * n : l.moments;
    else
        l.bytes = with_inputs ? l.v[0] : l.features;
    return l;
}

static int ctx_check(const char *who, const r1_context *c)
{
    if (!c)
        r1_set_error("%s: ctx is NULL", who);
    return c ? R1_OK : R1_EINVAL;
}

static int pointers_check(const char *who, bool guided, const void *L, const void *f, const void *V, const void *out, bool device)
{
    if (!L || !f || (guided && !V) || !out)
    {
        r1_set_error("%s: %s is NULL", who, !L ? "L" : !f ? "f" : guided && !V ? "V" : "out");
        return R1_EINVAL;
    }
    if (device && (((uintptr_t)L & 3u) || ((uintptr_t)out & 3u) || ((uintptr_t)f & 15u) || (guided && ((uintptr_t)V & 15u))))
    {
        r1_set_error(guided ? "%s: d_L and d_out must be 4-byte aligned, d_f and d_V 16-byte aligned" : "%s: d_L and d_out must be 4-byte aligned and d_f 16-byte aligned", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

// Enqueues the filter on `st`; every check has passed and the workspace holds at least layout(n, F.guided, false).  The passes of the small
// steps stage their taps in LDS (DESIGN.md §4.39 has the measurement that put the limit where it is).
static int enqueue(r1_context *c, const Filter &F, const void *d_L, const void *d_f, const void *d_V, void *d_out, hipStream_t st)
{
    const r1_denoise_guided_frame &fr = F.fr;
    const r1_denoise_opt &o = F.o.base;
    const Layout l = layout((size_t)fr.width * fr.height, F.guided, false);
    char *const ws = (char *)c->denoise_ws.p;
    R1VFilterArgs b;
    memset(&b, 0, sizeof(b));
    R1DenoiseArgs &a = b.d;
    a.L = (const float *)d_L, a.f = (const float *)d_f, a.out = (float *)d_out;
    a.guide = (R1DenoiseGuide *)(ws + l.guide);
    a.width = fr.width, a.height = fr.height;
    a.linear_stride = (uint32_t)(fr.linear_stride ? fr.linear_stride : fr.width);
    a.feature_stride = (uint32_t)(fr.feature_stride ? fr.feature_stride : fr.width);
    a.out_stride = (uint32_t)(fr.out_stride ? fr.out_stride : fr.width);
    a.flags = o.flags, a.k = (uint32_t)o.normal_power_log2, a.sigma_depth = o.sigma_depth;
    a.next = (R1DenoiseCur *)(ws + l.cur[0]);
    if (F.guided)
    {
        a.sc2 = o.sigma_color * o.sigma_color; // in every iteration
        b.V = (const float *)d_V, b.moment_stride = (uint32_t)(fr.moment_stride ? fr.moment_stride : fr.width);
        b.variance_floor = F.o.variance_floor;
        b.v_next = (float *)(ws + l.v[0]);
    }
    R1_HIP(r1_launch_denoise_prepare(&b, F.guided, st));
    // tuning library only; 0: every pass loads its taps directly.  The guided default is the unguided filter's, not yet measured for its kernels
    static const int stage_max[2] = {(int)r1_knob("R1_DENOISE_STAGE_MAX_STEP", R1D_STAGE_DEFAULT_MAX_STEP),
                                     (int)r1_knob("R1_VFILTER_STAGE_MAX_STEP", R1D_STAGE_DEFAULT_MAX_STEP)};
    for (int i = 0; i < o.iterations; ++i)
    {
        a.step = 1 << i;
        a.cur = (const R1DenoiseCur *)(ws + l.cur[i & 1]), a.next = (R1DenoiseCur *)(ws + l.cur[(i + 1) & 1]);
        if (F.guided)
            b.v_cur = (const float *)(ws + l.v[i & 1]), b.v_next = (float *)(ws + l.v[(i + 1) & 1]);
        else
            a.sc2 = r1d_sc2(o.sigma_color, i);
        R1_HIP(r1_launch_denoise_pass(&b, F.guided, a.step <= stage_max[F.guided] && a.step <= R1D_STAGE_MAX_STEP, i == o.iterations - 1, st));
    }
    return R1_OK;
}

// The device forms behind their checks of the context, the frame and the options
static int filter_device(const char *who, r1_context *c, const Filter &F, const void *d_L, const void *d_f, const void *d_V, void *d_out, void *hip_stream)
{
    int rc = pointers_check(who, F.guided, d_L, d_f, d_V, d_out, true);
    if (rc)
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = ensure(c->denoise_ws, layout((size_t)F.fr.width * F.fr.height, F.guided, false).bytes)))
        return rc;
    return enqueue(c, F, d_L, d_f, d_V, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

// ... and the forms on host memory (timed_sync, the two events around a call's device work: r1_context.h)
static int filter_sync(const char *who, r1_context *c, const Filter &F, const float *L, const r1_feature *f, const r1_moment *V, float *out, double *device_seconds_out)
{
    int rc = pointers_check(who, F.guided, L, f, V, out, false);
    if (rc)
        return rc;
    R1_HIP(hipSetDevice(c->device));
    const r1_denoise_guided_frame &fr = F.fr;
    const size_t w = (size_t)fr.width, h = (size_t)fr.height;
    const Layout l = layout(w * h, F.guided, true);
    if ((rc = ensure(c->denoise_ws, l.bytes)))
        return rc;
    char *const ws = (char *)c->denoise_ws.p;
    const size_t ls = fr.linear_stride ? fr.linear_stride : w, fs = fr.feature_stride ? fr.feature_stride : w, os = fr.out_stride ? fr.out_stride : w;
    const size_t ms = fr.moment_stride ? fr.moment_stride : w;
    // the caller's rows go up densely, the filter works in place on the dense linear frame, its rows come home with the caller's stride
    R1_HIP(hipMemcpy2DAsync(ws + l.linear, w * 12, L, ls * 12, w * 12, h, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpy2DAsync(ws + l.features, w * sizeof(r1_feature), f, fs * sizeof(r1_feature), w * sizeof(r1_feature), h, hipMemcpyHostToDevice, c->stream));
    if (F.guided)
        R1_HIP(hipMemcpy2DAsync(ws + l.moments, w * sizeof(r1_moment), V, ms * sizeof(r1_moment), w * sizeof(r1_moment), h, hipMemcpyHostToDevice, c->stream));
    const Filter dense = {F.guided, {fr.width, fr.height, 0, 0, 0, 0}, F.o};
    const void *const d_V = F.guided ? ws + l.moments : nullptr;
    if ((rc = timed_sync(c, who, device_seconds_out, [&] { return enqueue(c, dense, ws + l.linear, ws + l.features, d_V, ws + l.linear, c->stream); })))
        return rc;
    R1_HIP(hipMemcpy2DAsync(out, os * 12, ws + l.linear, w * 12, w * 12, h, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

extern "C" int r1_denoise_device(r1_context *c, const r1_denoise_frame *fr, const r1_denoise_opt *o, const void *d_L, const void *d_f, void *d_out,
                                 void *hip_stream)
{
    int rc = ctx_check("r1_denoise_device", c);
    if (rc || (rc = r1_denoise_check(fr, o)))
        return rc;
    return filter_device("r1_denoise_device", c, unguided_filter(*fr, *o), d_L, d_f, nullptr, d_out, hip_stream);
}

extern "C" int r1_denoise(r1_context *c, const r1_denoise_frame *fr, const r1_denoise_opt *o, const float *L, const r1_feature *f, float *out,
                          double *device_seconds_out)
{
    int rc = ctx_check("r1_denoise", c);
    if (rc || (rc = r1_denoise_check(fr, o)))
        return rc;
    return filter_sync("r1_denoise", c, unguided_filter(*fr, *o), L, f, nullptr, out, device_seconds_out);
}

extern "C" int r1_denoise_guided_device(r1_context *c, const r1_denoise_guided_frame *fr, const r1_denoise_guided_opt *o, const void *d_L, const void *d_f,
                                        const void *d_V, void *d_out, void *hip_stream)
{
    int rc = ctx_check("r1_denoise_guided_device", c);
    if (rc || (rc = r1_denoise_guided_check(fr, o)))
        return rc;
    return filter_device("r1_denoise_guided_device", c, {true, *fr, *o}, d_L, d_f, d_V, d_out, hip_stream);
}

extern "C" int r1_denoise_guided(r1_context *c, const r1_denoise_guided_frame *fr, const r1_denoise_guided_opt *o, const float *L, const r1_feature *f,
                                 const r1_moment *V, float *out, double *device_seconds_out)
{
    int rc = ctx_check("r1_denoise_guided", c);
    if (rc || (rc = r1_denoise_guided_check(fr, o)))
        return rc;
    return filter_sync("r1_denoise_guided", c, {true, *fr, *o}, L, f, V, out, device_seconds_out);
}

// ---- a frame rendered and denoised ---------------------------------------------------------------------------------------------------------

// What the composed forms refuse before anything is enqueued, in the documented order up to the pointers; *F: the whole frame, dense.
// go: the guided forms' options (o is their base), which add their own rules and one sample behind the unguided forms' list; else null
static int composed_check(const char *who, const r1_context *c, const r1_params *p, const r1_denoise_opt *o, const r1_denoise_guided_opt *go, Filter *F)
{
    int rc = ctx_check(who, c);
    if (rc)
        return rc;
    if (!p || !o)
    {
        r1_set_error("%s: %s is NULL", who, !p ? "params" : "options");
        return R1_EINVAL;
    }
    if ((rc = r1_params_check(p)))
        return rc;
    const r1_denoise_frame whole = {p->width, p->height, 0, 0, 0};
    if ((rc = r1_denoise_check(&whole, o)))
        return rc;
    if (p->variant != R1_VARIANT_DEFAULT && p->variant != R1_VARIANT_BVH && p->variant != R1_VARIANT_GRID && p->variant != R1_VARIANT_REFERENCE)
    {
        r1_set_error("%s: variant %d renders no feature frame (DEFAULT, BVH, GRID and REFERENCE do)", who, p->variant);
        return R1_EINVAL;
    }
    *F = unguided_filter(whole, *o);
    if (!go)
        return R1_OK;
    F->guided = true, F->o = *go;
    if ((rc = r1_denoise_guided_check(&F->fr, go)))
        return rc;
    if (p->spp < 2)
    {
        r1_set_error("%s: spp %d carries no variance (at least 2; r1_render_denoised serves one sample)", who, p->spp);
        return R1_EINVAL;
    }
    return R1_OK;
}

// The three parts on `st`.  The linear (guided: variance) render comes first: what it refuses (no scene, shards, a moved scene's stale tables)
// is refused before anything is enqueued, and the feature frame refuses nothing the render has passed.  The workspace was sized by the
// caller: the two renders allocate nothing of it.
static int composed_enqueue(r1_context *c, const r1_params *p, const Filter &F, void *d_rgb, void *d_rays, hipStream_t st)
{
    const Layout l = layout((size_t)F.fr.width * F.fr.height, F.guided, true);
    char *const ws = (char *)c->denoise_ws.p;
    int rc = F.guided ? r1_render_moments_device(c, p, d_rgb, ws + l.moments, d_rays, st) : r1_render_linear_device(c, p, d_rgb, d_rays, st);
    if (rc || (rc = r1_render_features_device(c, p, nullptr, ws + l.features, st)))
        return rc;
    return enqueue(c, F, d_rgb, ws + l.features, F.guided ? ws + l.moments : nullptr, d_rgb, st);
}

static int composed_device(const char *who, r1_context *c, const r1_params *p, const r1_denoise_opt *o, const r1_denoise_guided_opt *go, void *d_rgb_f32,
                           void *d_num_rays, void *hip_stream)
{
    Filter F;
    int rc = composed_check(who, c, p, o, go, &F);
    if (rc || (rc = device_outputs_check(who, c, d_rgb_f32, d_num_rays)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = ensure(c->denoise_ws, layout((size_t)F.fr.width * F.fr.height, F.guided, true).bytes)))
        return rc;
    return composed_enqueue(c, p, F, d_rgb_f32, d_num_rays, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

static int composed_sync(const char *who, r1_context *c, const r1_params *p, const r1_denoise_opt *o, const r1_denoise_guided_opt *go, float *rgb_out,
                         uint64_t *num_rays_out, double *device_seconds_out)
{
    Filter F;
    int rc = composed_check(who, c, p, o, go, &F);
    if (rc)
        return rc;
    if (!rgb_out)
    {
        r1_set_error("%s: rgb_out is NULL", who);
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)F.fr.width * F.fr.height;
    const Layout l = layout(n, F.guided, true);
    if ((rc = ensure(c->denoise_ws, l.bytes)))
        return rc;
    char *const ws = (char *)c->denoise_ws.p;
    return timed_render_home(c, who, device_seconds_out, ws + l.linear, ws, n, rgb_out, num_rays_out,
                             [&] { return composed_enqueue(c, p, F, ws + l.linear, ws, c->stream); });
}

extern "C" int r1_render_denoised_device(r1_context *c, const r1_params *p, const r1_denoise_opt *o, void *d_rgb_f32, void *d_num_rays, void *hip_stream)
{
    return composed_device("r1_render_denoised_device", c, p, o, nullptr, d_rgb_f32, d_num_rays, hip_stream);
}

extern "C" int r1_render_denoised(r1_context *c, const r1_params *p, const r1_denoise_opt *o, float *rgb_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    return composed_sync("r1_render_denoised", c, p, o, nullptr, rgb_out, num_rays_out, device_seconds_out);
}

// (null options: refused as the unguided forms refuse theirs, before `go` is looked at)
extern "C" int r1_render_denoised_guided_device(r1_context *c, const r1_params *p, const r1_denoise_guided_opt *go, void *d_rgb_f32, void *d_num_rays, void *hip_stream)
{
    return composed_device("r1_render_denoised_guided_device", c, p, go ? &go->base : nullptr, go, d_rgb_f32, d_num_rays, hip_stream);
}

extern "C" int r1_render_denoised_guided(r1_context *c, const r1_params *p, const r1_denoise_guided_opt *go, float *rgb_out, uint64_t *num_rays_out,
                                         double *device_seconds_out)
{
    return composed_sync("r1_render_denoised_guided", c, p, go ? &go->base : nullptr, go, rgb_out, num_rays_out, device_seconds_out);
}
