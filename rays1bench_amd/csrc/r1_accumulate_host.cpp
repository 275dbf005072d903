// r1_accumulate_host.cpp — accumulated frames without a device (include/rays1.h "accumulated frames"): r1_accumulate_check,
// the step from the public structs to what the arithmetic reads (r1_accumulate_args, shared with r1_accumulate.cpp), and r1_accumulate_host,
// the definition the device forms (r1_accumulate.cpp, r1_reproject_kernels.hip) are held to bit for bit.  The arithmetic is r1_reproject.h's.
// No HIP runtime call here.
#include <math.h>
#include <string.h>

#include "r1_internal.h"
#include "r1_reproject.h"

static_assert(sizeof(r1_moment) == 16 && sizeof(r1_feature) == 32, "the records the taps read");
static_assert(sizeof(r1_reproject_plan) == sizeof(R1ReprojectPlan), "the public plan is the arithmetic's");

static bool finite32(float v) { return fabsf(v) <= 3.402823466e38f; }

extern "C" int r1_accumulate_check(const r1_accumulate_frame *fr, const r1_accumulate_opt *o, const r1_accumulate_view *v, r1_reproject_plan *plan_out)
{
    if (!fr || !o || !v)
    {
        r1_set_error("r1_accumulate_check: %s is NULL", !fr ? "frame" : !o ? "options" : "view");
        return R1_EINVAL;
    }
    if (fr->width < 1 || fr->height < 1)
    {
        r1_set_error("r1_accumulate_frame: %s %d is not positive", fr->width < 1 ? "width" : "height", fr->width < 1 ? fr->width : fr->height);
        return R1_EINVAL;
    }
    if ((int64_t)fr->width * fr->height >= ((int64_t)1 << 31))
    {
        r1_set_error("r1_accumulate_frame: width * height = %lld pixels, the limit is 2^31 - 1", (long long)fr->width * fr->height);
        return R1_ELIMIT;
    }
    const struct
    {
        const char *name;
        int32_t value;
    } strides[8] = {{"linear_stride", fr->linear_stride},
                    {"moment_stride", fr->moment_stride},
                    {"feature_stride", fr->feature_stride},
                    {"prev_stride", fr->prev_stride},
                    {"prev_feature_stride", fr->prev_feature_stride},
                    {"prev_moment_stride", fr->prev_moment_stride},
                    {"out_stride", fr->out_stride},
                    {"out_moment_stride", fr->out_moment_stride}};
    for (const auto &s : strides)
        if (s.value != 0 && s.value < fr->width)
        {
            r1_set_error("r1_accumulate_frame: %s %d is neither 0 nor at least the width %d", s.name, s.value, fr->width);
            return R1_EINVAL;
        }
    if (o->max_samples < 1u)
    {
        r1_set_error("r1_accumulate_opt: max_samples %u is not at least 1", o->max_samples);
        return R1_EINVAL;
    }
    if (!(o->depth_tolerance > 0.0f) || !finite32(o->depth_tolerance))
    {
        r1_set_error("r1_accumulate_opt: depth_tolerance %g is not positive and finite", (double)o->depth_tolerance);
        return R1_EINVAL;
    }
    if (!(o->normal_min_cos >= -1.0f && o->normal_min_cos <= 1.0f))
    {
        r1_set_error("r1_accumulate_opt: normal_min_cos %g is not in -1 .. 1", (double)o->normal_min_cos);
        return R1_EINVAL;
    }
    if (o->flags != 0u)
    {
        r1_set_error("r1_accumulate_opt: flags %u is not 0", o->flags);
        return R1_EINVAL;
    }
    if (v->spp < 1 || v->spp_prev < 1)
    {
        r1_set_error("r1_accumulate_view: %s %d is not positive", v->spp < 1 ? "spp" : "spp_prev", v->spp < 1 ? v->spp : v->spp_prev);
        return R1_EINVAL;
    }
    R1ReprojectPlan plan;
    const r1_camera &p = v->camera_prev;
    if (!r1r_plan(p.origin, p.lower_left, p.horizontal, p.vertical, p.u, p.v, p.w, fr->width, fr->height, plan))
    {
        r1_set_error("r1_accumulate_view: camera_prev projects nothing (pw %g, hu %g, vv %g must be finite and not zero)", (double)plan.pw, (double)plan.hu,
                     (double)plan.vv);
        return R1_EINVAL;
    }
    if (plan_out)
        memcpy(plan_out, &plan, sizeof(plan));
    return R1_OK;
}

// The kernel's and the host loop's arguments from the public structs; the check has passed.  The images' pointers are taken as they are.
extern "C" void r1_accumulate_args(const r1_accumulate_frame *fr, const r1_accumulate_opt *o, const r1_accumulate_view *v, const r1_reproject_plan *plan,
                                   const r1_accumulate_images *im, R1ReprojectArgs *a)
{
    memset(a, 0, sizeof(*a));
    a->L = (const float *)im->L, a->V = (const float *)im->V, a->f = (const float *)im->f;
    a->A_prev = (const float *)im->A_prev, a->f_prev = (const float *)im->f_prev, a->M_prev = (const float *)im->M_prev;
    a->A_out = (float *)im->A_out, a->M_out = (float *)im->M_out;
    a->width = fr->width, a->height = fr->height;
    const auto stride = [&](int32_t s) { return (uint32_t)(s ? s : fr->width); };
    a->linear_stride = stride(fr->linear_stride), a->moment_stride = stride(fr->moment_stride), a->feature_stride = stride(fr->feature_stride);
    a->prev_stride = stride(fr->prev_stride), a->prev_feature_stride = stride(fr->prev_feature_stride), a->prev_moment_stride = stride(fr->prev_moment_stride);
    a->out_stride = stride(fr->out_stride), a->out_moment_stride = stride(fr->out_moment_stride);
    a->max_samples = o->max_samples, a->depth_tolerance = o->depth_tolerance, a->normal_min_cos = o->normal_min_cos;
    R1ReprojectView &w = a->view;
    for (int c = 0; c < 3; ++c)
    {
        w.o[c] = v->camera.origin[c], w.ll[c] = v->camera.lower_left[c], w.hz[c] = v->camera.horizontal[c], w.vt[c] = v->camera.vertical[c];
        w.op[c] = v->camera_prev.origin[c], w.up[c] = v->camera_prev.u[c], w.vp[c] = v->camera_prev.v[c], w.wp[c] = v->camera_prev.w[c];
    }
    memcpy(&w.plan, plan, sizeof(w.plan));
    w.spp = (float)v->spp, w.spp_prev = (float)v->spp_prev;
    w.wf = (float)fr->width, w.hf = (float)fr->height;
}

// NULL images, then an output that is a history image: what every form refuses behind the check
extern "C" int r1_accumulate_images_check(const char *who, const r1_accumulate_images *im)
{
    if (!im)
    {
        r1_set_error("%s: images is NULL", who);
        return R1_EINVAL;
    }
    const void *const p[8] = {im->L, im->V, im->f, im->A_prev, im->f_prev, im->M_prev, im->A_out, im->M_out};
    static const char *const names[8] = {"L", "V", "f", "A_prev", "f_prev", "M_prev", "A_out", "M_out"};
    for (int i = 0; i < 8; ++i)
        if (!p[i])
        {
            r1_set_error("%s: %s is NULL", who, names[i]);
            return R1_EINVAL;
        }
    for (int o = 6; o < 8; ++o)
        for (int h = 3; h < 6; ++h)
            if (p[o] == p[h])
            {
                r1_set_error("%s: %s overlaps the history (%s): the call is a gather, its outputs must be apart from A_prev, f_prev and M_prev", who, names[o],
                             names[h]);
                return R1_EINVAL;
            }
    if (im->A_out == im->M_out || im->A_out == im->V || im->A_out == im->f || im->M_out == im->L || im->M_out == im->f)
    {
        r1_set_error("%s: A_out may be L and M_out may be V, and neither may be another image of the call", who);
        return R1_EINVAL;
    }
    return R1_OK;
}

extern "C" int r1_accumulate_host(const r1_accumulate_frame *fr, const r1_accumulate_opt *o, const r1_accumulate_view *v, const r1_accumulate_images *im)
{
    r1_reproject_plan plan;
    int rc = r1_accumulate_check(fr, o, v, &plan);
    if (rc || (rc = r1_accumulate_images_check("r1_accumulate_host", im)))
        return rc;
    R1ReprojectArgs a;
    r1_accumulate_args(fr, o, v, &plan, im, &a);
    const r1_moment *const V = (const r1_moment *)im->V, *const Mp = (const r1_moment *)im->M_prev;
    const r1_feature *const f = (const r1_feature *)im->f, *const fp = (const r1_feature *)im->f_prev;
    r1_moment *const Mo = (r1_moment *)im->M_out;
    for (int y = 0; y < a.height; ++y)
        for (int x = 0; x < a.width; ++x)
        {
            // the pixel's own records are consumed before its outputs are written (A_out may be L, M_out may be V)
            const float *Lp = a.L + ((size_t)y * a.linear_stride + x) * 3;
            const float L[3] = {Lp[0], Lp[1], Lp[2]};
            const r1_moment mv = V[(size_t)y * a.moment_stride + x];
            const r1_feature ft = f[(size_t)y * a.feature_stride + x];
            float A[3] = {L[0], L[1], L[2]};
            r1_moment mo = mv;
            const uint32_t n = mv.samples;
            int x0 = 0, y0 = 0;
            float fx = 0.0f, fy = 0.0f, e = 0.0f, q[3];
            bool history = ft.hits != 0u && n != 0u;
            if (history)
            {
                r1r_world(a.view, x, y, ft.depth, ft.hits, q);
                history = r1r_project(a.view, q, x0, y0, fx, fy, e);
            }
            if (history)
            {
                float nh[3];
                r1r_unit_normal(ft.normal, nh);
                R1ReprojectSums s;
                r1r_sums_clear(s);
                for (int j = 0; j < 2; ++j)
                    for (int i = 0; i < 2; ++i)
                    {
                        const int tx = x0 + i, ty = y0 + j;
                        if (tx < 0 || tx >= a.width || ty < 0 || ty >= a.height)
                            continue;
                        const r1_feature &fq = fp[(size_t)ty * a.prev_feature_stride + tx];
                        const r1_moment &mq = Mp[(size_t)ty * a.prev_moment_stride + tx];
                        const float b = r1r_weight(i, j, fx, fy);
                        if (!r1r_tap_taken(b, e, nh, fq.depth, fq.normal, fq.hits, mq.samples, a.view.spp_prev, a.depth_tolerance, a.normal_min_cos))
                            continue;
                        r1r_tap_add(b, a.A_prev + ((size_t)ty * a.prev_stride + tx) * 3, mq.var, mq.samples, s);
                    }
                if (s.B > 0.0f)
                    mo.samples = r1r_blend(s, L, mv.var, n, a.max_samples, A, mo.var);
            }
            float *Ao = a.A_out + ((size_t)y * a.out_stride + x) * 3;
            Ao[0] = A[0], Ao[1] = A[1], Ao[2] = A[2];
            Mo[(size_t)y * a.out_moment_stride + x] = mo;
        }
    return R1_OK;
}
