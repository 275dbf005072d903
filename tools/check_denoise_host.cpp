// tools/check_denoise_host.cpp — denoised frames on the host, a stand-alone program over the library's host source only:
// r1_denoise_host on a seeded synthetic frame of 37 x 21 pixels.  It checks the host form against the contract re-stated here in C — plain
// loops over plain arrays, none of r1_denoise.h — for every value, bit for bit, with and without demodulation and at the ends of the options'
// ranges; that every pixel without a hit keeps L's bits; that out == L gives the same frame; a strided window with nothing read or written
// between the rows; and the refusals, which write nothing.
// tests/test_denoise_host.py builds and runs it with -fsanitize=address,undefined (host code only, no GPU, no library loaded into another
// process):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//         -I<hip include dir> tools/check_denoise_host.cpp rays1bench_amd/csrc/r1_denoise_host.cpp -o check_denoise_host
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
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
            return 1;                                          \
        }                                                      \
    } while (0)

// splitmix64: the frame's values
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

// The contract (include/rays1.h "denoised frames"), dense arrays: L [n][3], f [n] -> out [n][3]
static void contract(int w, int h, const r1_denoise_opt &o, const float *L, const r1_feature *f, float *out)
{
    const size_t n = (size_t)w * h;
    std::vector<float> a(3 * n), cur(3 * n), nxt(3 * n), nh(3 * n), m(n);
    std::vector<char> surf(n);
    static const float H[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    for (size_t p = 0; p < n; ++p)
    {
        surf[p] = f[p].hits > 0;
        for (int c = 0; c < 3; ++c)
        {
            a[3 * p + c] = (o.flags & R1_DENOISE_DEMODULATE) ? (f[p].albedo[c] < 1.0f / 256 ? 1.0f / 256 : f[p].albedo[c]) : 1.0f;
            cur[3 * p + c] = L[3 * p + c] / a[3 * p + c];
        }
        const float *v = f[p].normal;
        const float nn = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        const float l = sqrtf(nn);
        for (int c = 0; c < 3; ++c)
            nh[3 * p + c] = l > 0 ? v[c] / l : 0.0f;
        m[p] = surf[p] ? f[p].depth / (float)f[p].hits : 0.0f;
    }
    for (int i = 0; i < o.iterations; ++i)
    {
        const int step = 1 << i;
        const float sc = o.sigma_color * ldexpf(1.0f, -i), sc2 = sc * sc;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
            {
                const size_t p = (size_t)y * w + x;
                if (!surf[p])
                {
                    for (int c = 0; c < 3; ++c)
                        nxt[3 * p + c] = cur[3 * p + c];
                    continue;
                }
                float S[3] = {0, 0, 0}, W = 0;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx)
                    {
                        const int qx = x + step * dx, qy = y + step * dy;
                        if (qx < 0 || qy < 0 || qx >= w || qy >= h)
                            continue;
                        const size_t q = (size_t)qy * w + qx;
                        if (!surf[q])
                            continue;
                        const float hh = H[dy + 2] * H[dx + 2];
                        float wt = hh;
                        if (dx != 0 || dy != 0)
                        {
                            float c = (nh[3 * p] * nh[3 * q] + nh[3 * p + 1] * nh[3 * q + 1]) + nh[3 * p + 2] * nh[3 * q + 2];
                            c = c < 0 ? 0 : c;
                            c = c > 1 ? 1 : c;
                            for (int j = 0; j < o.normal_power_log2; ++j)
                                c = c * c;
                            const float mx = m[p] < m[q] ? m[q] : m[p];
                            const float den = o.sigma_depth * mx;
                            const float rz = den > 0 ? (m[p] - m[q]) / den : 0.0f;
                            const float xz = rz * rz;
                            const float dr = cur[3 * p] - cur[3 * q], dg = cur[3 * p + 1] - cur[3 * q + 1], db = cur[3 * p + 2] - cur[3 * q + 2];
                            const float dc = (dr * dr + dg * dg) + db * db;
                            const float xc = dc / sc2;
                            wt = (hh * c) / ((1 + xz) * (1 + xc));
                        }
                        for (int c = 0; c < 3; ++c)
                        {
                            const float t = wt * cur[3 * q + c];
                            S[c] = S[c] + t;
                        }
                        W = W + wt;
                    }
                for (int c = 0; c < 3; ++c)
                    nxt[3 * p + c] = S[c] / W;
            }
        cur.swap(nxt);
    }
    for (size_t p = 0; p < n; ++p)
        for (int c = 0; c < 3; ++c)
            out[3 * p + c] = surf[p] ? cur[3 * p + c] * a[3 * p + c] : L[3 * p + c];
}

int main()
{
    const int w = 37, h = 21;
    const size_t n = (size_t)w * h;
    std::vector<float> L(3 * n);
    std::vector<r1_feature> f(n);
    size_t none = 0, zero_normal = 0, dark = 0, far = 0, bright = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            const size_t p = (size_t)y * w + x;
            r1_feature &v = f[p];
            memset(&v, 0, sizeof(v));
            const bool hole = (x >= 3 && x < 10 && y >= 2 && y < 6) || chance(0.04);
            v.hits = hole ? 0u : 1u + (uint32_t)(next_u64() % 4);
            const int kind = (int)(next_u64() % 6);
            const float dir[6][3] = {{0, 0, 1}, {0.96824584f, 0, 0.25f}, {0.995f, 0, 0.1f}, {0, 1, 0}, {0, 0, -1}, {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)}};
            const bool cancel = chance(0.03);
            float mean = chance(0.5) ? 2.5f : uniform(0.5f, 20.0f);
            if (chance(0.1))
                mean *= 1000.0f, far += v.hits > 0;
            for (int c = 0; c < 3; ++c)
            {
                v.albedo[c] = chance(0.05) ? 0.0f : chance(0.05) ? 1.0f / 1024 : uniform(0.05f, 1.0f);
                dark += v.hits > 0 && v.albedo[c] < 1.0f / 256;
                v.normal[c] = v.hits && !cancel ? dir[kind][c] * (float)v.hits * 0.7f : 0.0f;
                L[3 * p + c] = v.albedo[c] * uniform(0, 2) + uniform(0, 0.05f);
            }
            if (x >= w / 2 && chance(0.3))
                L[3 * p] *= 1e4f, L[3 * p + 1] *= 1e4f, L[3 * p + 2] *= 1e4f, bright += 1;
            v.depth = v.hits ? mean * (float)v.hits : 0.0f;
            none += v.hits == 0, zero_normal += v.hits > 0 && cancel;
        }
    NEED(none >= 28 && zero_normal >= 3 && dark >= 10 && far >= 10 && bright >= 10);

    const r1_denoise_frame fr = {w, h, 0, 0, 0};
    const r1_denoise_opt opts[] = {{3, 6, 1.0f, 0.1f, R1_DENOISE_DEMODULATE}, {3, 6, 1.0f, 0.1f, 0},     {1, 0, 1.0f, 0.1f, R1_DENOISE_DEMODULATE},
                                   {8, 10, 1e-3f, 1e3f, R1_DENOISE_DEMODULATE}, {5, 4, 1e3f, 1e-3f, 0}};
    std::vector<float> want(3 * n), got(3 * n);
    for (const r1_denoise_opt &o : opts)
    {
        contract(w, h, o, L.data(), f.data(), want.data());
        memset(got.data(), 0xA5, 3 * n * sizeof(float));
        NEED(r1_denoise_host(&fr, &o, L.data(), f.data(), got.data()) == R1_OK);
        NEED(memcmp(got.data(), want.data(), 3 * n * sizeof(float)) == 0);
        size_t changed = 0;
        for (size_t p = 0; p < n; ++p)
        {
            if (f[p].hits == 0)
                NEED(memcmp(&got[3 * p], &L[3 * p], 12) == 0);
            else
                changed += memcmp(&got[3 * p], &L[3 * p], 12) != 0;
        }
        NEED(changed >= n / 2);
        // in place: out == L
        std::vector<float> inplace(L);
        NEED(r1_denoise_host(&fr, &o, inplace.data(), f.data(), inplace.data()) == R1_OK);
        NEED(memcmp(inplace.data(), want.data(), 3 * n * sizeof(float)) == 0);
    }
    printf("frame %dx%d: every value the contract's under %zu sets of options; %zu pixels without a hit keep L's bits; in place the same\n", w, h,
           sizeof(opts) / sizeof(opts[0]), none);

    // a strided window: the three images each with rows further apart than the width, marks between the rows, exactly sized buffers
    // (one element more read or written is the address sanitizer's to report)
    const r1_denoise_frame wide = {w, h, w + 3, w + 1, w + 5};
    const r1_denoise_opt &o = opts[0];
    contract(w, h, o, L.data(), f.data(), want.data());
    std::vector<float> Ls(((size_t)(h - 1) * wide.linear_stride + w) * 3), outs(((size_t)(h - 1) * wide.out_stride + w) * 3);
    std::vector<r1_feature> fs((size_t)(h - 1) * wide.feature_stride + w);
    memset(Ls.data(), 0xFF, Ls.size() * sizeof(float)); // (NaN between the rows: a value read from there would spread)
    memset(fs.data(), 0xFF, fs.size() * sizeof(r1_feature));
    memset(outs.data(), 0xA5, outs.size() * sizeof(float));
    for (int y = 0; y < h; ++y)
    {
        memcpy(&Ls[(size_t)y * wide.linear_stride * 3], &L[(size_t)y * w * 3], (size_t)w * 12);
        memcpy(&fs[(size_t)y * wide.feature_stride], &f[(size_t)y * w], (size_t)w * sizeof(r1_feature));
    }
    NEED(r1_denoise_host(&wide, &o, Ls.data(), fs.data(), outs.data()) == R1_OK);
    for (size_t i = 0; i < outs.size() / 3; ++i)
    {
        const size_t row = i / (size_t)wide.out_stride, col = i % (size_t)wide.out_stride;
        static const unsigned char mark[12] = {0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5, 0xA5};
        NEED(memcmp(&outs[3 * i], col < (size_t)w ? (const void *)&want[(row * w + col) * 3] : (const void *)mark, 12) == 0);
    }
    printf("strides %d, %d, %d: the frame's values, nothing written between the rows\n", wide.linear_stride, wide.feature_stride, wide.out_stride);

    // refusals write nothing and name the field
    std::vector<float> untouched(3 * n);
    memset(untouched.data(), 0xA5, 3 * n * sizeof(float));
    struct Bad
    {
        r1_denoise_frame fr;
        r1_denoise_opt o;
        int rc;
        const char *says;
    };
    const float inf = INFINITY, nan = NAN;
    const Bad bad[] = {{{0, h, 0, 0, 0}, o, R1_EINVAL, "width"},
                       {{w, -1, 0, 0, 0}, o, R1_EINVAL, "height"},
                       {{65536, 32768, 0, 0, 0}, o, R1_ELIMIT, "2^31"},
                       {{w, h, w - 1, 0, 0}, o, R1_EINVAL, "linear_stride"},
                       {{w, h, 0, 1, 0}, o, R1_EINVAL, "feature_stride"},
                       {{w, h, 0, 0, -4}, o, R1_EINVAL, "out_stride"},
                       {fr, {0, 6, 1.0f, 0.1f, 1}, R1_EINVAL, "iterations"},
                       {fr, {9, 6, 1.0f, 0.1f, 1}, R1_EINVAL, "iterations"},
                       {fr, {3, -1, 1.0f, 0.1f, 1}, R1_EINVAL, "normal_power_log2"},
                       {fr, {3, 11, 1.0f, 0.1f, 1}, R1_EINVAL, "normal_power_log2"},
                       {fr, {3, 6, 0.0f, 0.1f, 1}, R1_EINVAL, "sigma_color"},
                       {fr, {3, 6, inf, 0.1f, 1}, R1_EINVAL, "sigma_color"},
                       {fr, {3, 6, nan, 0.1f, 1}, R1_EINVAL, "sigma_color"},
                       {fr, {3, 6, 1.0f, -0.1f, 1}, R1_EINVAL, "sigma_depth"},
                       {fr, {3, 6, 1.0f, inf, 1}, R1_EINVAL, "sigma_depth"},
                       {fr, {3, 6, 1.0f, 0.1f, 2}, R1_EINVAL, "flags"}};
    for (const Bad &b : bad)
    {
        g_error[0] = 0;
        NEED(r1_denoise_check(&b.fr, &b.o) == b.rc && strstr(g_error, b.says) != nullptr);
        NEED(r1_denoise_host(&b.fr, &b.o, L.data(), f.data(), untouched.data()) == b.rc);
    }
    NEED(r1_denoise_check(nullptr, &o) == R1_EINVAL && strstr(g_error, "frame") != nullptr);
    NEED(r1_denoise_check(&fr, nullptr) == R1_EINVAL && strstr(g_error, "options") != nullptr);
    NEED(r1_denoise_host(&fr, &o, nullptr, f.data(), untouched.data()) == R1_EINVAL && strstr(g_error, "L is NULL") != nullptr);
    NEED(r1_denoise_host(&fr, &o, L.data(), nullptr, untouched.data()) == R1_EINVAL && strstr(g_error, "f is NULL") != nullptr);
    NEED(r1_denoise_host(&fr, &o, L.data(), f.data(), nullptr) == R1_EINVAL && strstr(g_error, "out is NULL") != nullptr);
    for (size_t i = 0; i < 3 * n; ++i)
        NEED(memcmp(&untouched[i], "\xA5\xA5\xA5\xA5", 4) == 0);
    printf("refusals wrote nothing\n");
    return 0;
}
