// r1_linear_host.cpp — linear frames without a GPU (include/rays1.h): r1_render_linear_host, the CPU form of
// r1_render_linear built from r1_camera_rays and r1_trace_rays_host, and r1_render_moments_host beside it (§4.40); r1_quantise_linear, the step from a linear value to the byte; and
// r1_pfm_write_rgb32f.  Compiled as every host file is, with -ffp-contract=off and without -ffast-math: the sums below are plain fp32
// adds in sample order, and sqrtf is the host's correctly rounded one.

#include "../../include/rays1.h"
#include "r1_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

// rayweek1.cpp:757-765 for every pixel of window `win` of the frame: S = 0.0f; S += color(sample s) for s = 0 .. spp - 1; L = S * (float)(1.0f / spp),
// stored at rgb_out + (y * stride + x) * 3 for pixel (x, y) of the window.  The whole frame is the window (0, 0, width, height) with stride width.
// moments_out (may be null; dense, win.width records a row): the pixel's r1_moment record, DESIGN.md §4.40 — a second walk over the same records.
static int render_window_host(const r1_scene *scene, const r1_camera *camera, const r1_params *p, const r1_region &win, float *rgb_out, uint64_t *num_rays_out,
                              r1_moment *moments_out = nullptr)
{
    int rc;
    // a few rows of pixels at a time: the rays, seeds and records of their samples (64 bytes a sample) stay small for any frame
    const size_t spp = (size_t)p->spp, n_pixels = (size_t)win.width * win.height;
    const size_t stride = win.out_stride ? (size_t)win.out_stride : (size_t)win.width;
    const size_t chunk = (((size_t)1 << 16) + spp - 1) / spp; // pixels
    std::vector<int32_t> x, y, s;
    std::vector<r1_ray> rays;
    std::vector<r1_sample_seed> seeds;
    std::vector<r1_radiance> rec;
    const float inv = (float)(1.0f / p->spp); // rayweek1.cpp:765
    const float inv_nn = p->spp > 1 ? 1.0f / ((float)p->spp * (float)(p->spp - 1)) : 0.0f;
    uint64_t total = 0;
    for (size_t p0 = 0; p0 < n_pixels; p0 += chunk)
    {
        const size_t np = n_pixels - p0 < chunk ? n_pixels - p0 : chunk, n = np * spp;
        x.resize(n), y.resize(n), s.resize(n), rays.resize(n), seeds.resize(n), rec.resize(n);
        for (size_t i = 0; i < np; ++i)
            for (size_t k = 0; k < spp; ++k)
            {
                x[i * spp + k] = win.x0 + (int32_t)((p0 + i) % (size_t)win.width), y[i * spp + k] = win.y0 + (int32_t)((p0 + i) / (size_t)win.width);
                s[i * spp + k] = (int32_t)k;
            }
        if ((rc = r1_camera_rays(camera, p, x.data(), y.data(), s.data(), n, rays.data(), seeds.data())) ||
            (rc = r1_trace_rays_host(scene, p->max_bounces, rays.data(), seeds.data(), n, rec.data())))
            return rc;
        for (size_t i = 0; i < np; ++i)
        {
            float cr = 0.0f, cg = 0.0f, cb = 0.0f;
            for (size_t k = 0; k < spp; ++k)
            {
                const r1_radiance &v = rec[i * spp + k];
                cr += v.r, cg += v.g, cb += v.b; // col += color(...) rayweek1.cpp:762
                total += v.rays;
            }
            float *const o = rgb_out + ((p0 + i) / (size_t)win.width * stride + (p0 + i) % (size_t)win.width) * 3;
            o[0] = cr * inv, o[1] = cg * inv, o[2] = cb * inv;
            if (!moments_out)
                continue;
            const float lr = o[0], lg = o[1], lb = o[2];
            float dr = 0.0f, dg = 0.0f, db = 0.0f;
            for (size_t k = 0; k < spp; ++k)
            {
                const r1_radiance &v = rec[i * spp + k];
                const float er = v.r - lr, eg = v.g - lg, eb = v.b - lb;
                dr = dr + er * er, dg = dg + eg * eg, db = db + eb * eb;
            }
            r1_moment &m = moments_out[p0 + i];
            m.var[0] = p->spp > 1 ? dr * inv_nn : 0.0f, m.var[1] = p->spp > 1 ? dg * inv_nn : 0.0f, m.var[2] = p->spp > 1 ? db * inv_nn : 0.0f;
            m.samples = (uint32_t)p->spp;
        }
    }
    if (num_rays_out)
        *num_rays_out = total;
    return R1_OK;
}

extern "C" int r1_render_linear_host(const r1_scene *scene, const r1_camera *camera, const r1_params *p, float *rgb_out, uint64_t *num_rays_out)
{
    if (!scene || !camera || !p || !rgb_out)
    {
        r1_set_error("r1_render_linear_host: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_linear_host renders whole frames (num_shards == 1, not %d)", p->num_shards);
        return R1_EINVAL;
    }
    const r1_region whole = {0, 0, p->width, p->height, 0};
    return render_window_host(scene, camera, p, whole, rgb_out, num_rays_out);
}

// The CPU form of r1_render_moments: r1_render_linear_host's frame and ray count, and the moment records beside it
extern "C" int r1_render_moments_host(const r1_scene *scene, const r1_camera *camera, const r1_params *p, float *rgb_out, r1_moment *moments_out, uint64_t *num_rays_out)
{
    if (!scene || !camera || !p || !rgb_out || !moments_out)
    {
        r1_set_error("r1_render_moments_host: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_moments_host renders whole frames (num_shards == 1, not %d)", p->num_shards);
        return R1_EINVAL;
    }
    const r1_region whole = {0, 0, p->width, p->height, 0};
    return render_window_host(scene, camera, p, whole, rgb_out, num_rays_out, moments_out);
}

// The CPU form of r1_render_region_linear: the window's pixels of the FRAME — r1_camera_rays seeds and aims with params' width
// and height — summed as above, rows out_stride pixels apart.
extern "C" int r1_render_region_host(const r1_scene *scene, const r1_camera *camera, const r1_params *p, const r1_region *region, float *linear_out,
                                     uint64_t *num_rays_out)
{
    if (!scene || !camera || !p || !region || !linear_out)
    {
        r1_set_error("r1_render_region_host: null argument");
        return R1_EINVAL;
    }
    int rc = r1_region_check(p, region);
    if (rc)
        return rc;
    return render_window_host(scene, camera, p, *region, linear_out, num_rays_out);
}

// rayweek1.cpp:766-775 for one channel: (uint8)(int)(sqrtf(v) * 255.99f).  Refused before a byte is written: a value whose (int) is
// undefined — negative (-0.0f is zero), NaN, infinite, or so large that the product is no int.
extern "C" int r1_quantise_linear(const float *linear, size_t n_values, uint8_t *out)
{
    if (n_values == 0)
        return R1_OK;
    if (!linear || !out)
    {
        r1_set_error("r1_quantise_linear: null argument");
        return R1_EINVAL;
    }
    for (size_t i = 0; i < n_values; ++i)
        if (!(linear[i] >= 0.0f) || !(sqrtf(linear[i]) * 255.99f < 2147483648.0f))
        {
            r1_set_error("r1_quantise_linear: value %zu (%g) is negative, NaN, infinite or beyond what (int) holds", i, (double)linear[i]);
            return R1_EINVAL;
        }
    for (size_t i = 0; i < n_values; ++i)
        out[i] = (uint8_t)(int)(sqrtf(linear[i]) * 255.99f);
    return R1_OK;
}

// A PFM file: "PF\n<w> <h>\n-1.0\n", then the rows from the bottom up as little-endian fp32 RGB — this library's row order
extern "C" int r1_pfm_write_rgb32f(const char *filename, int32_t width, int32_t height, const float *pixels)
{
    if (!filename || !pixels || width <= 0 || height <= 0)
        return R1_EINVAL;
    FILE *f = fopen(filename, "wb");
    if (!f)
        return R1_EINVAL;
    const size_t n = (size_t)width * height * 3;
    bool ok = fprintf(f, "PF\n%d %d\n-1.0\n", width, height) > 0;
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
    for (size_t i = 0; i < n && ok; ++i)
    {
        uint32_t w;
        memcpy(&w, pixels + i, 4);
        const uint8_t b[4] = {(uint8_t)w, (uint8_t)(w >> 8), (uint8_t)(w >> 16), (uint8_t)(w >> 24)};
        ok = fwrite(b, 1, 4, f) == 4;
    }
#else
    ok = ok && fwrite(pixels, sizeof(float), n, f) == n;
#endif
    ok = (fclose(f) == 0) && ok;
    return ok ? R1_OK : R1_EINVAL;
}
