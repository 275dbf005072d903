// tools/check_accumulate_host.cpp — r1_accumulate_host (rays1bench_amd/csrc/r1_accumulate_host.cpp alone) driven stand-alone: the contract of
// include/rays1.h "accumulated frames" once more in plain C loops over dense arrays, with nothing of r1_reproject.h, compared bit for bit on
// seeded frame pairs under several camera pairs and sets of options; every image in a buffer sized exactly to its last pixel, dense and with
// strides, so a sanitizer sees any access between or behind the rows and any tap off the image; in place; the refusals.  Built by
// tests/test_accumulate_host.py with -fsanitize=address,undefined and -ffp-contract=off.  No GPU, no HIP runtime call.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/rays1.h"
#include "../rays1bench_amd/csrc/r1_internal.h"

// (the library's error text lives in r1_capi.cpp, next to the HIP runtime: this program links the host source only)
static char g_error[512];
void r1_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

#define NEED(c)                                                \
    do                                                         \
    {                                                          \
        if (!(c))                                              \
        {                                                      \
            fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, g_error); \
            return 1;                                          \
        }                                                      \
    } while (0)

// splitmix64: the frames' values
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64()
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)((next_u64() >> 40) * (1.0 / 16777216.0)); }
static bool chance(double p) { return (next_u64() >> 11) * (1.0 / 9007199254740992.0) < p; }

static float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static void unit3(const float *n, float *nh)
{
    const float l = sqrtf(dot3(n, n));
    for (int c = 0; c < 3; ++c)
        nh[c] = l > 0.0f ? n[c] / l : 0.0f;
}

// The contract, dense arrays
static void contract(int w, int h, const r1_accumulate_opt &o, const r1_accumulate_view &v, const float *L, const r1_moment *V, const r1_feature *f,
                     const float *Ap, const r1_feature *fp, const r1_moment *Mp, float *Ao, r1_moment *Mo)
{
    const r1_camera &cam = v.camera, &prev = v.camera_prev;
    float dl[3];
    for (int c = 0; c < 3; ++c)
        dl[c] = prev.lower_left[c] - prev.origin[c];
    const float pu = dot3(dl, prev.u), pv = dot3(dl, prev.v), pw = dot3(dl, prev.w), hu = dot3(prev.horizontal, prev.u), vv = dot3(prev.vertical, prev.v);
    const float inv_w = 1.0f / (float)w, inv_h = 1.0f / (float)h;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            const size_t ip = (size_t)y * w + x;
            const uint32_t n = V[ip].samples;
            float out[3] = {L[ip * 3], L[ip * 3 + 1], L[ip * 3 + 2]};
            r1_moment mo = V[ip];
            if (f[ip].hits != 0 && n != 0)
            {
                const float s = ((float)x + 0.5f) * inv_w, t = ((float)y + 0.5f) * inv_h;
                float d[3], q[3];
                for (int c = 0; c < 3; ++c)
                    d[c] = ((cam.lower_left[c] + cam.horizontal[c] * s) + cam.vertical[c] * t) - cam.origin[c];
                const float len = sqrtf(dot3(d, d));
                const float m = (f[ip].depth / (float)f[ip].hits) * (float)v.spp;
                for (int c = 0; c < 3; ++c)
                {
                    const float dh = d[c] / len;
                    const float P = cam.origin[c] + dh * m;
                    q[c] = P - prev.origin[c];
                }
                const float a = dot3(q, prev.u), b = dot3(q, prev.v), c = dot3(q, prev.w);
                if (c * pw > 0.0f)
                {
                    const float k = pw / c;
                    const float sx = (a * k - pu) / hu, sy = (b * k - pv) / vv;
                    const float px = sx * (float)w - 0.5f, py = sy * (float)h - 0.5f;
                    if (px > -1.0f && px < (float)w && py > -1.0f && py < (float)h)
                    {
                        const int x0 = (int)floorf(px), y0 = (int)floorf(py);
                        const float fx = px - floorf(px), fy = py - floorf(py);
                        const float e = sqrtf(dot3(q, q));
                        float nh[3];
                        unit3(f[ip].normal, nh);
                        float B = 0.0f, C[3] = {0, 0, 0}, U[3] = {0, 0, 0};
                        uint32_t N = 0xFFFFFFFFu;
                        for (int j = 0; j < 2; ++j)
                            for (int i = 0; i < 2; ++i)
                            {
                                const int tx = x0 + i, ty = y0 + j;
                                if (tx < 0 || tx >= w || ty < 0 || ty >= h)
                                    continue;
                                const size_t iq = (size_t)ty * w + tx;
                                const float bw = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                                if (!(bw > 0.0f) || fp[iq].hits == 0 || Mp[iq].samples == 0)
                                    continue;
                                const float mq = (fp[iq].depth / (float)fp[iq].hits) * (float)v.spp_prev;
                                float df = e - mq;
                                df = df < 0.0f ? -df : df;
                                const float mx = e < mq ? mq : e;
                                if (!(df <= o.depth_tolerance * mx))
                                    continue;
                                float nq[3];
                                unit3(fp[iq].normal, nq);
                                if (dot3(nh, nq) < o.normal_min_cos)
                                    continue;
                                B = B + bw;
                                for (int ch = 0; ch < 3; ++ch)
                                {
                                    C[ch] = C[ch] + bw * Ap[iq * 3 + ch];
                                    U[ch] = U[ch] + bw * Mp[iq].var[ch];
                                }
                                N = Mp[iq].samples < N ? Mp[iq].samples : N;
                            }
                        if (B > 0.0f)
                        {
                            uint64_t N_new = (uint64_t)N + n;
                            N_new = N_new < o.max_samples ? N_new : o.max_samples;
                            N_new = N_new < n ? n : N_new;
                            const float alpha = n >= N_new ? 1.0f : (float)n / (float)(uint32_t)N_new;
                            for (int ch = 0; ch < 3; ++ch)
                            {
                                const float hist = C[ch] / B, vh = U[ch] / B;
                                out[ch] = hist + (L[ip * 3 + ch] - hist) * alpha;
                                mo.var[ch] = ((1.0f - alpha) * (1.0f - alpha)) * vh + (alpha * alpha) * V[ip].var[ch];
                            }
                            mo.samples = (uint32_t)N_new;
                        }
                    }
                }
            }
            Ao[ip * 3] = out[0], Ao[ip * 3 + 1] = out[1], Ao[ip * 3 + 2] = out[2];
            Mo[ip] = mo;
        }
}

static r1_camera camera(float ox, float oy, float oz, float ux, float wz, float half_w, float half_h)
{
    // u = (ux, 0, 0), v = (0, 1, 0), w = (0, 0, wz): ux = wz = 1 looks along -z, ux = wz = -1 is that camera turned by 180 degrees about y
    r1_camera c;
    memset(&c, 0, sizeof(c));
    c.origin[0] = ox, c.origin[1] = oy, c.origin[2] = oz;
    c.u[0] = ux, c.v[1] = 1.0f, c.w[2] = wz;
    for (int k = 0; k < 3; ++k)
    {
        c.lower_left[k] = ((c.origin[k] - half_w * c.u[k]) - half_h * c.v[k]) - c.w[k];
        c.horizontal[k] = 2.0f * half_w * c.u[k], c.vertical[k] = 2.0f * half_h * c.v[k];
    }
    return c;
}

// an image of w x h pixels with `stride` pixels between its rows, in a buffer that ends with its last pixel
template <class T> static std::vector<T> strided(const std::vector<T> &dense, int w, int h, int per, int stride, T fill)
{
    std::vector<T> out(((size_t)(h - 1) * stride + w) * per, fill);
    for (int y = 0; y < h; ++y)
        for (int i = 0; i < w * per; ++i)
            out[(size_t)y * stride * per + i] = dense[(size_t)y * w * per + i];
    return out;
}

int main()
{
    const int w = 41, h = 23;
    const size_t n = (size_t)w * h;
    std::vector<float> L(n * 3), Ap(n * 3);
    std::vector<r1_moment> V(n), Mp(n);
    std::vector<r1_feature> f(n), fp(n);
    for (size_t i = 0; i < n; ++i)
    {
        const uint32_t hits = chance(0.06) ? 0u : 1u + (uint32_t)(next_u64() % 4);
        const float mean = chance(0.5) ? 2.5f : uniform(0.5f, 20.0f);
        memset(&f[i], 0, sizeof(f[i]));
        f[i].hits = hits, f[i].depth = hits ? mean * (float)hits / 4.0f : 0.0f;
        for (int c = 0; c < 3; ++c)
        {
            f[i].albedo[c] = uniform(0.0f, 1.0f);
            f[i].normal[c] = hits && !chance(0.03) ? uniform(-1.0f, 1.0f) : 0.0f;
            L[i * 3 + c] = uniform(0.0f, 2.0f), Ap[i * 3 + c] = uniform(0.0f, 2.0f);
            V[i].var[c] = uniform(0.0f, 0.01f), Mp[i].var[c] = uniform(0.0f, 0.005f);
        }
        V[i].samples = chance(0.02) ? 0u : 4u;
        fp[i] = f[i];
        if (chance(0.15))
            fp[i].depth *= uniform(1.2f, 3.0f);
        if (chance(0.1))
            for (int c = 0; c < 3; ++c)
                fp[i].normal[c] = -fp[i].normal[c];
        if (chance(0.05))
            fp[i].hits = 0;
        Mp[i].samples = chance(0.04) ? 0u : chance(0.05) ? 0xFFFFFFF0u : 1u + (uint32_t)(next_u64() % 40);
    }
    const float poison[4] = {NAN, INFINITY, 1e30f, 0.0f};
    for (int k = 0; k < 4; ++k)
        f[(size_t)5 * w + 7 + k].depth = poison[k], f[(size_t)5 * w + 7 + k].hits = 2, fp[(size_t)9 * w + 3 + k].depth = poison[k];

    const float hh = (float)h / (float)w;
    const r1_camera cur = camera(0, 0, 0, 1, 1, 1, hh);
    const float zoom = 1.0f / (1.0f + 1.0f / (float)(w - 1));
    const r1_camera prevs[7] = {camera(0, 0, 0, 1, 1, 1, hh),   camera(0.7f, 0, 0, 1, 1, 1, hh),  camera(-0.7f, 0, 0, 1, 1, 1, hh), camera(0, 0.7f, 0, 1, 1, 1, hh),
                                camera(0, -0.7f, 0, 1, 1, 1, hh), camera(0, 0, 0, 1, 1, zoom, hh * zoom), camera(0, 0, 0, -1, -1, 1, hh)};
    const r1_accumulate_opt opts[5] = {{32u, 0.05f, 0.9f, 0u}, {1u, 1e-30f, -1.0f, 0u}, {0xFFFFFFFFu, 1e30f, 1.0f, 0u}, {2u, 0.5f, -1.0f, 0u}, {16u, 0.5f, 1.0f, 0u}};
    const r1_accumulate_frame dense = {w, h, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<float> want_A(n * 3), got_A(n * 3);
    std::vector<r1_moment> want_M(n), got_M(n);
    size_t blended = 0, turned_same = 0;
    for (int pc = 0; pc < 7; ++pc)
        for (int po = 0; po < 5; ++po)
        {
            r1_accumulate_view v;
            v.camera = cur, v.camera_prev = prevs[pc], v.spp = 4, v.spp_prev = 4;
            contract(w, h, opts[po], v, L.data(), V.data(), f.data(), Ap.data(), fp.data(), Mp.data(), want_A.data(), want_M.data());
            const r1_accumulate_images im = {L.data(), V.data(), f.data(), Ap.data(), fp.data(), Mp.data(), got_A.data(), got_M.data()};
            NEED(r1_accumulate_host(&dense, &opts[po], &v, &im) == R1_OK);
            NEED(memcmp(got_A.data(), want_A.data(), n * 12) == 0 && memcmp(got_M.data(), want_M.data(), n * 16) == 0);
            for (size_t i = 0; i < n; ++i)
                blended += memcmp(&got_M[i], &V[i], 16) != 0;
            if (pc == 6)
                turned_same += memcmp(got_A.data(), L.data(), n * 12) == 0 && memcmp(got_M.data(), V.data(), n * 16) == 0;
        }
    NEED(blended > 1000 && turned_same == 5);
    printf("every value the contract's under 7 camera pairs x 5 sets of options (%zu pixels blended)\n", blended);

    // strides, every buffer ending with its last pixel; then in place (A_out = L, M_out = V)
    r1_accumulate_view v;
    v.camera = cur, v.camera_prev = prevs[1], v.spp = 4, v.spp_prev = 4;
    contract(w, h, opts[0], v, L.data(), V.data(), f.data(), Ap.data(), fp.data(), Mp.data(), want_A.data(), want_M.data());
    {
        const r1_accumulate_frame fr = {w, h, w + 3, w + 2, w + 1, w + 4, w + 5, w + 6, w + 7, w + 8};
        const r1_moment m0 = {{0, 0, 0}, 0};
        r1_feature f0;
        memset(&f0, 0, sizeof(f0));
        auto sL = strided(L, w, h, 3, fr.linear_stride, -1.0f);
        auto sV = strided(V, w, h, 1, fr.moment_stride, m0);
        auto sf = strided(f, w, h, 1, fr.feature_stride, f0);
        auto sAp = strided(Ap, w, h, 3, fr.prev_stride, -1.0f);
        auto sfp = strided(fp, w, h, 1, fr.prev_feature_stride, f0);
        auto sMp = strided(Mp, w, h, 1, fr.prev_moment_stride, m0);
        std::vector<float> oA(((size_t)(h - 1) * fr.out_stride + w) * 3, -7.0f);
        std::vector<r1_moment> oM((size_t)(h - 1) * fr.out_moment_stride + w, r1_moment{{-7.0f, -7.0f, -7.0f}, 7u});
        const r1_accumulate_images im = {sL.data(), sV.data(), sf.data(), sAp.data(), sfp.data(), sMp.data(), oA.data(), oM.data()};
        NEED(r1_accumulate_host(&fr, &opts[0], &v, &im) == R1_OK);
        for (int y = 0; y < h; ++y)
        {
            NEED(memcmp(&oA[(size_t)y * fr.out_stride * 3], &want_A[(size_t)y * w * 3], (size_t)w * 12) == 0);
            NEED(memcmp(&oM[(size_t)y * fr.out_moment_stride], &want_M[(size_t)y * w], (size_t)w * 16) == 0);
            for (int x = w; y + 1 < h && x < fr.out_stride; ++x)
                NEED(oA[((size_t)y * fr.out_stride + x) * 3] == -7.0f);
            for (int x = w; y + 1 < h && x < fr.out_moment_stride; ++x)
                NEED(oM[(size_t)y * fr.out_moment_stride + x].samples == 7u);
        }
        printf("strides %d .. %d in buffers that end with their last pixel\n", fr.feature_stride, fr.out_moment_stride);
    }
    {
        std::vector<float> wL(L);
        std::vector<r1_moment> wV(V);
        const r1_accumulate_images im = {wL.data(), wV.data(), f.data(), Ap.data(), fp.data(), Mp.data(), wL.data(), wV.data()};
        NEED(r1_accumulate_host(&dense, &opts[0], &v, &im) == R1_OK);
        NEED(memcmp(wL.data(), want_A.data(), n * 12) == 0 && memcmp(wV.data(), want_M.data(), n * 16) == 0);
        printf("in place: A_out = L and M_out = V\n");
    }

    // the refusals: nothing is written
    {
        std::vector<float> oA(n * 3, 7.0f);
        std::vector<r1_moment> oM(n, r1_moment{{7.0f, 7.0f, 7.0f}, 7u});
        r1_accumulate_images im = {L.data(), V.data(), f.data(), Ap.data(), fp.data(), Mp.data(), oA.data(), oM.data()};
        r1_accumulate_opt bad = opts[0];
        bad.max_samples = 0;
        NEED(r1_accumulate_host(&dense, &bad, &v, &im) == R1_EINVAL && strstr(g_error, "max_samples"));
        bad = opts[0], bad.depth_tolerance = 0.0f;
        NEED(r1_accumulate_host(&dense, &bad, &v, &im) == R1_EINVAL && strstr(g_error, "depth_tolerance"));
        bad = opts[0], bad.normal_min_cos = NAN;
        NEED(r1_accumulate_host(&dense, &bad, &v, &im) == R1_EINVAL && strstr(g_error, "normal_min_cos"));
        bad = opts[0], bad.flags = 1;
        NEED(r1_accumulate_host(&dense, &bad, &v, &im) == R1_EINVAL && strstr(g_error, "flags"));
        r1_accumulate_view flat = v;
        memset(flat.camera_prev.w, 0, sizeof(flat.camera_prev.w));
        for (int k = 0; k < 3; ++k)
            flat.camera_prev.lower_left[k] = flat.camera_prev.origin[k];
        NEED(r1_accumulate_host(&dense, &opts[0], &flat, &im) == R1_EINVAL && strstr(g_error, "camera_prev"));
        r1_accumulate_frame short_rows = dense;
        short_rows.prev_feature_stride = w - 1;
        NEED(r1_accumulate_host(&short_rows, &opts[0], &v, &im) == R1_EINVAL && strstr(g_error, "prev_feature_stride"));
        im.A_out = Ap.data();
        NEED(r1_accumulate_host(&dense, &opts[0], &v, &im) == R1_EINVAL && strstr(g_error, "overlaps the history"));
        im.A_out = oA.data(), im.M_out = Mp.data();
        NEED(r1_accumulate_host(&dense, &opts[0], &v, &im) == R1_EINVAL && strstr(g_error, "overlaps the history"));
        im.M_out = nullptr;
        NEED(r1_accumulate_host(&dense, &opts[0], &v, &im) == R1_EINVAL && strstr(g_error, "M_out is NULL"));
        for (size_t i = 0; i < n; ++i)
            NEED(oA[i * 3] == 7.0f && oM[i].samples == 7u);
        printf("refusals wrote nothing\n");
    }
    return 0;
}
