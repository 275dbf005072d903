// r1_accumulate.cpp — accumulated frames on the device (include/rays1.h "accumulated frames"): r1_accumulate_device enqueues
// r1_reproject_kernel (r1_reproject_kernels.hip) on the caller's images; r1_accumulate is the same on host memory; r1_render_accumulated*
// compose r1_render_moments_device + r1_render_features_device + the accumulation against the context's history (+ the guided filter) on
// one stream.  The rules are checked in r1_accumulate_check (r1_accumulate_host.cpp), the arithmetic is r1_reproject.h's.  Like the filters,
// the accumulation touches none of the state a render reads.
#include <string.h>

#include "r1_context.h"
#include "r1_reproject.h"

static int device_images_check(const char *who, const r1_accumulate_images *im)
{
    int rc = r1_accumulate_images_check(who, im);
    if (rc)
        return rc;
    const uintptr_t four = (uintptr_t)im->L | (uintptr_t)im->A_prev | (uintptr_t)im->A_out;
    const uintptr_t sixteen = (uintptr_t)im->V | (uintptr_t)im->f | (uintptr_t)im->f_prev | (uintptr_t)im->M_prev | (uintptr_t)im->M_out;
    if ((four & 3u) || (sixteen & 15u))
    {
        r1_set_error("%s: L, A_prev and A_out must be 4-byte aligned, the feature and moment images 16-byte aligned", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

static int accumulate_enqueue(const r1_accumulate_frame *fr, const r1_accumulate_opt *o, const r1_accumulate_view *v, const r1_reproject_plan *plan,
                              const r1_accumulate_images *im, hipStream_t st)
{
    R1ReprojectArgs a;
    r1_accumulate_args(fr, o, v, plan, im, &a);
    R1_HIP(r1_launch_reproject(&a, st));
    return R1_OK;
}

extern "C" int r1_accumulate_device(r1_context *c, const r1_accumulate_frame *fr, const r1_accumulate_opt *o, const r1_accumulate_view *v,
                                    const r1_accumulate_images *im, void *hip_stream)
{
    if (!c)
    {
        r1_set_error("r1_accumulate_device: ctx is NULL");
        return R1_EINVAL;
    }
    r1_reproject_plan plan;
    int rc = r1_accumulate_check(fr, o, v, &plan);
    if (rc || (rc = device_images_check("r1_accumulate_device", im)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    return accumulate_enqueue(fr, o, v, &plan, im, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_accumulate(r1_context *c, const r1_accumulate_frame *fr, const r1_accumulate_opt *o, const r1_accumulate_view *v, const r1_accumulate_images *im,
                             double *device_seconds_out)
{
    if (!c)
    {
        r1_set_error("r1_accumulate: ctx is NULL");
        return R1_EINVAL;
    }
    r1_reproject_plan plan;
    int rc = r1_accumulate_check(fr, o, v, &plan);
    if (rc || (rc = r1_accumulate_images_check("r1_accumulate", im)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    const size_t w = (size_t)fr->width, h = (size_t)fr->height, n = w * h;
    // the eight images, dense: the feature and moment images first (16-byte records), the three-float images behind them
    const size_t item[8] = {12, 16, 32, 12, 32, 16, 12, 16};
    const int order[8] = {2, 4, 1, 5, 7, 0, 3, 6};
    size_t at[8], bytes = 0;
    for (int k = 0; k < 8; ++k)
        at[order[k]] = bytes, bytes += item[order[k]] * n;
    if ((rc = ensure(c->accumulate_io, bytes)))
        return rc;
    char *const ws = (char *)c->accumulate_io.p;
    const void *const src[6] = {im->L, im->V, im->f, im->A_prev, im->f_prev, im->M_prev};
    const int32_t stride[8] = {fr->linear_stride, fr->moment_stride,      fr->feature_stride, fr->prev_stride,
                               fr->prev_feature_stride, fr->prev_moment_stride, fr->out_stride,     fr->out_moment_stride};
    for (int k = 0; k < 6; ++k)
        R1_HIP(hipMemcpy2DAsync(ws + at[k], w * item[k], src[k], (stride[k] ? (size_t)stride[k] : w) * item[k], w * item[k], h, hipMemcpyHostToDevice, c->stream));
    const r1_accumulate_frame dense = {fr->width, fr->height, 0, 0, 0, 0, 0, 0, 0, 0};
    const r1_accumulate_images dim = {ws + at[0], ws + at[1], ws + at[2], ws + at[3], ws + at[4], ws + at[5], ws + at[6], ws + at[7]};
    if ((rc = timed_sync(c, "r1_accumulate", device_seconds_out, [&] { return accumulate_enqueue(&dense, o, v, &plan, &dim, c->stream); })))
        return rc;
    void *const dst[2] = {im->A_out, im->M_out};
    for (int k = 6; k < 8; ++k)
        R1_HIP(hipMemcpy2DAsync(dst[k - 6], (stride[k] ? (size_t)stride[k] : w) * item[k], ws + at[k], w * item[k], w * item[k], h, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

// ---- a frame rendered and accumulated against the context's history --------------------------------------------------------------------------

extern "C" int r1_accumulate_reset(r1_context *c)
{
    if (!c)
    {
        r1_set_error("r1_accumulate_reset: ctx is NULL");
        return R1_EINVAL;
    }
    c->history_slot = -1;
    return R1_OK;
}

// The history workspace: a 256-byte head, two slots of {f, M, A} — a call renders into the slot the history is not in and accumulates in
// place there (A_out = L, M_out = V) — and, for the synchronous form, the frame that goes home.
struct HistoryLayout
{
    size_t f[2], M[2], A[2], out, bytes;
};
static HistoryLayout history_layout(size_t n)
{
    HistoryLayout l;
    size_t at = 256;
    for (int s = 0; s < 2; ++s)
    {
        l.f[s] = at, at += 32 * n;
        l.M[s] = at, at += 16 * n;
        l.A[s] = at, at += (12 * n + 15) & ~(size_t)15;
    }
    l.out = at, l.bytes = at + 12 * n;
    return l;
}

// What both composed forms refuse before anything is enqueued, in the documented order up to the pointers
static int composed_check(const char *who, const r1_context *c, const r1_params *p, const r1_accumulate_opt *o, const r1_denoise_guided_opt *go)
{
    if (!c)
    {
        r1_set_error("%s: ctx is NULL", who);
        return R1_EINVAL;
    }
    if (!p || !o)
    {
        r1_set_error("%s: %s is NULL", who, !p ? "params" : "acc_opt");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    // the options, with a view every frame passes: the context's own camera stands in for both, the history's is checked where it is used
    const r1_accumulate_frame whole = {p->width, p->height, 0, 0, 0, 0, 0, 0, 0, 0};
    r1_accumulate_view probe;
    memset(&probe, 0, sizeof(probe));
    probe.camera_prev.lower_left[2] = -1.0f, probe.camera_prev.horizontal[0] = 1.0f, probe.camera_prev.vertical[1] = 1.0f;
    probe.camera_prev.u[0] = 1.0f, probe.camera_prev.v[1] = 1.0f, probe.camera_prev.w[2] = 1.0f;
    probe.camera = probe.camera_prev, probe.spp = probe.spp_prev = 1;
    if ((rc = r1_accumulate_check(&whole, o, &probe, nullptr)))
        return rc;
    if (go)
    {
        const r1_denoise_guided_frame gf = {p->width, p->height, 0, 0, 0, 0};
        if ((rc = r1_denoise_guided_check(&gf, go)))
            return rc;
    }
    if (p->variant != R1_VARIANT_DEFAULT && p->variant != R1_VARIANT_BVH && p->variant != R1_VARIANT_GRID && p->variant != R1_VARIANT_REFERENCE)
    {
        r1_set_error("%s: variant %d renders no feature frame (DEFAULT, BVH, GRID and REFERENCE do)", who, p->variant);
        return R1_EINVAL;
    }
    if (go && p->spp < 2)
    {
        r1_set_error("%s: spp %d carries no variance for the filter (at least 2; without a filter any spp is served)", who, p->spp);
        return R1_EINVAL;
    }
    return R1_OK;
}

// The parts on `st`; the history workspace holds history_layout(n).  The render comes first: what it refuses (shards, a moved scene's stale
// tables) is refused before anything is enqueued and before the history is touched.
static int composed_enqueue(r1_context *c, const r1_params *p, const r1_accumulate_opt *o, const r1_denoise_guided_opt *go, void *d_rgb, void *d_rays, hipStream_t st)
{
    const size_t n = (size_t)p->width * p->height;
    const HistoryLayout l = history_layout(n);
    char *const ws = (char *)c->history_ws.p;
    const bool usable = c->history_slot >= 0 && c->history_w == p->width && c->history_h == p->height;
    const int prev = usable ? c->history_slot : 1, cur = 1 - prev;
    int rc = r1_render_moments_device(c, p, ws + l.A[cur], ws + l.M[cur], d_rays, st);
    if (rc)
        return rc;
    c->history_slot = -1; // (until everything of this frame is enqueued: a failure below leaves no half-made history behind)
    if ((rc = r1_render_features_device(c, p, nullptr, ws + l.f[cur], st)))
        return rc;
    if (usable)
    {
        const r1_accumulate_frame whole = {p->width, p->height, 0, 0, 0, 0, 0, 0, 0, 0};
        r1_accumulate_view v;
        v.camera = c->src_cam, v.camera_prev = c->history_cam, v.spp = p->spp, v.spp_prev = c->history_spp;
        r1_reproject_plan plan;
        // (a previous camera through which nothing projects: the frame passes through, as with no history)
        if (r1_accumulate_check(&whole, o, &v, &plan) == R1_OK)
        {
            const r1_accumulate_images im = {ws + l.A[cur], ws + l.M[cur], ws + l.f[cur], ws + l.A[prev], ws + l.f[prev], ws + l.M[prev], ws + l.A[cur], ws + l.M[cur]};
            if ((rc = accumulate_enqueue(&whole, o, &v, &plan, &im, st)))
                return rc;
        }
    }
    if (go)
    {
        const r1_denoise_guided_frame gf = {p->width, p->height, 0, 0, 0, 0};
        if ((rc = r1_denoise_guided_device(c, &gf, go, ws + l.A[cur], ws + l.f[cur], ws + l.M[cur], d_rgb, st)))
            return rc;
    }
    else
        R1_HIP(hipMemcpyAsync(d_rgb, ws + l.A[cur], n * 12, hipMemcpyDeviceToDevice, st));
    c->history_slot = cur, c->history_w = p->width, c->history_h = p->height, c->history_spp = p->spp, c->history_cam = c->src_cam;
    return R1_OK;
}

// the history workspace at its size for this frame; one that had to grow held no history of this size
static int history_ensure(r1_context *c, const r1_params *p)
{
    const size_t bytes = history_layout((size_t)p->width * p->height).bytes;
    if (!c->history_ws.p || c->history_ws.cap < bytes)
        c->history_slot = -1;
    return ensure(c->history_ws, bytes);
}

extern "C" int r1_render_accumulated_device(r1_context *c, const r1_params *p, const r1_accumulate_opt *o, const r1_denoise_guided_opt *go, void *d_rgb_f32,
                                            void *d_num_rays, void *hip_stream)
{
    int rc = composed_check("r1_render_accumulated_device", c, p, o, go);
    if (rc || (rc = device_outputs_check("r1_render_accumulated_device", c, d_rgb_f32, d_num_rays)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = history_ensure(c, p)))
        return rc;
    return composed_enqueue(c, p, o, go, d_rgb_f32, d_num_rays, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

extern "C" int r1_render_accumulated(r1_context *c, const r1_params *p, const r1_accumulate_opt *o, const r1_denoise_guided_opt *go, float *rgb_out,
                                     uint64_t *num_rays_out, double *device_seconds_out)
{
    int rc = composed_check("r1_render_accumulated", c, p, o, go);
    if (rc)
        return rc;
    if (!rgb_out)
    {
        r1_set_error("r1_render_accumulated: rgb_out is NULL");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    if ((rc = history_ensure(c, p)))
        return rc;
    const size_t n = (size_t)p->width * p->height;
    const HistoryLayout l = history_layout(n);
    char *const ws = (char *)c->history_ws.p;
    return timed_render_home(c, "r1_render_accumulated", device_seconds_out, ws + l.out, ws, n, rgb_out, num_rays_out,
                             [&] { return composed_enqueue(c, p, o, go, ws + l.out, ws, c->stream); });
}
