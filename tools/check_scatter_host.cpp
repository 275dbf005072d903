// tools/check_scatter_host.cpp — rays1bench_amd/csrc/r1_scatter.h on the host: the Dielectric arm without the outward normal
// (R1_SCATTER_FORM 1) against the reference's form (0), and both against the oracle's own reflect, refract and scatter
// (tools/check_scatter_oracle.c), bit for bit.  tests/test_scatter_host.py builds and runs it; DESIGN.md §4.25.
//
//   check_scatter_host [random inputs, default 10000000] [seed, default 2026]
// prints one `name value` line per counter and exits 0 only if `mismatches` is 0.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rays1bench_amd/csrc/r1_scatter.h"

extern "C"
{
    void r1so_reflect(const float v[3], const float n[3], float out[3]);
    int r1so_refract(const float v[3], const float outward[3], float ni_over_nt, float out[3]);
    int r1so_scatter(int mat_type, float mat_param, const float d[3], const float p[3], const float n[3], uint32_t streams[5], float out[3]);
}

namespace
{

struct V3
{
    float x, y, z;
};

uint32_t bits(const float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
bool same(const float a, const float b) { return bits(a) == bits(b); }
bool same(const V3 a, const V3 b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
bool same(const V3 a, const float *b) { return same(a.x, b[0]) && same(a.y, b[1]) && same(a.z, b[2]); }

// the draws and the normalisation as shade_level makes them (r1_shade.hpp)
uint32_t xorshift32(uint32_t &state)
{
    uint32_t x = state;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 15;
    state = x;
    return x;
}
float rand01(uint32_t &s) { return (float)(xorshift32(s) & 0xFFFFFFu) * (1.0f / 16777216.0f); }
float rand02_minus1(uint32_t &s) { return fmaf((float)(xorshift32(s) & 0xFFFFFFu), 1.0f / 8388608.0f, -1.0f); }
V3 unit(const V3 v)
{
    const float r = 1.0f / sqrtf(r1s_dot(v, v));
    return V3{v.x * r, v.y * r, v.z * r};
}

struct Counters
{
    uint64_t inputs, mismatches, ddn_pos_zero, ddn_neg_zero, zero_components, grazing, inside, outside, total_reflection, refracting,
        just_above, index_below_one, index_above_one, fuzz_zero, fuzz_one, chose_reflected, chose_refracted, metal_absorbed;
} C;

void report(const char *what, const V3 d, const V3 n, const int type, const float param)
{
    if (C.mismatches++ < 10)
        fprintf(stderr, "MISMATCH %s: d %08x %08x %08x n %08x %08x %08x type %d param %08x\n", what, bits(d.x), bits(d.y), bits(d.z), bits(n.x),
                bits(n.y), bits(n.z), type, bits(param));
}

// one level's scatter from the header, as shade_level calls it: the scattered (normalised) direction, Material::scatter's result
template <int FORM>
bool scatter(const int type, const float param, const V3 d, const V3 hp, const V3 n, uint32_t st[5], V3 &out, R1Dielectric &k, V3 &refracted)
{
    V3 rius{0, 0, 0};
    if (type != 2)
        do
        {
            rius = V3{rand02_minus1(st[1]), rand02_minus1(st[2]), rand02_minus1(st[3])};
        } while (r1s_dot(rius, rius) >= 1);
    V3 dir;
    if (type == 0)
        dir = r1s_lambertian(hp, n, rius);
    else
    {
        const float ddn = r1s_dot(d, n);
        const V3 refl = r1s_reflect(d, n, ddn);
        if (type == 1)
            dir = r1s_metal(refl, rius, param);
        else
        {
            float r0 = (1 - param) / (1 + param); // (r1_sweep.cpp: the host's material constants)
            r0 = r0 * r0;
            k = r1s_dielectric_form<FORM>(d, n, ddn, param, 1.0f / param);
            float reflect_prob = 1.0f;
            refracted = V3{0, 0, 0};
            if (k.discriminant > 0)
            {
                refracted = r1s_refracted_form<FORM>(d, n, ddn, k, sqrtf(k.discriminant));
                reflect_prob = r1s_schlick(r0, k.cosine);
            }
            const bool reflects = rand01(st[0]) < reflect_prob;
            if (FORM == 1)
                ++(reflects ? C.chose_reflected : C.chose_refracted);
            dir = reflects ? refl : refracted;
        }
    }
    out = unit(dir);
    return type != 1 || r1s_dot(out, n) > 0;
}

void check(const V3 d, const V3 n, const V3 hp, const int type, const float param, const uint32_t streams[5])
{
    ++C.inputs;
    const float dv[3] = {d.x, d.y, d.z}, nv[3] = {n.x, n.y, n.z}, pv[3] = {hp.x, hp.y, hp.z};
    const float ddn = r1s_dot(d, n);
    C.ddn_pos_zero += bits(ddn) == 0u, C.ddn_neg_zero += bits(ddn) == 0x80000000u;
    C.zero_components += d.x == 0 || d.y == 0 || d.z == 0 || n.x == 0 || n.y == 0 || n.z == 0;
    C.grazing += fabsf(ddn) < 1e-3f;

    // reflect
    float o3[3];
    r1so_reflect(dv, nv, o3);
    if (!same(r1s_reflect(d, n, ddn), o3))
        report("reflect", d, n, type, param);

    // the level: both forms and the oracle's scatter, with the streams they leave
    uint32_t s0[5], s1[5], so[5];
    memcpy(s0, streams, sizeof(s0)), memcpy(s1, streams, sizeof(s1)), memcpy(so, streams, sizeof(so));
    V3 out0, out1, refr0{0, 0, 0}, refr1{0, 0, 0};
    R1Dielectric k0{}, k1{};
    const bool ok0 = scatter<0>(type, param, d, hp, n, s0, out0, k0, refr0);
    const bool ok1 = scatter<1>(type, param, d, hp, n, s1, out1, k1, refr1);
    const bool oko = r1so_scatter(type, param, dv, pv, nv, so, o3) != 0;
    if (ok0 != ok1 || !same(out0, out1) || memcmp(s0, s1, 16))
        report("scatter, form 1 against form 0", d, n, type, param);
    if (ok1 != oko || !same(out1, o3) || memcmp(s1, so, 16)) // (lane 3 is the oracle's alone: the kernels carry three lanes)
        report("scatter against the oracle", d, n, type, param);
    if (type == 1)
        C.fuzz_zero += param == 0.0f, C.fuzz_one += param == 1.0f, C.metal_absorbed += !ok1;
    if (type != 2)
        return;

    // the Dielectric arm's terms, form against form, and refract against the oracle's with the reference's outward normal
    C.index_below_one += param < 1.0f, C.index_above_one += param > 1.0f;
    ++(k1.inside ? C.inside : C.outside);
    if (k0.inside != k1.inside || !same(k0.ni_over_nt, k1.ni_over_nt) || !same(k0.cosine, k1.cosine) || !same(k0.dt, k1.dt) ||
        !same(k0.discriminant, k1.discriminant) || !same(refr0, refr1))
        report("dielectric terms, form 1 against form 0", d, n, type, param);
    const float ow[3] = {k1.inside ? -n.x : n.x, k1.inside ? -n.y : n.y, k1.inside ? -n.z : n.z};
    const bool refracts = r1so_refract(dv, ow, k1.ni_over_nt, o3) != 0;
    if (refracts != (k1.discriminant > 0) || !same(refr1, o3))
        report("refract against the oracle", d, n, type, param);
    ++(refracts ? C.refracting : C.total_reflection);
    C.just_above += refracts && k1.discriminant < 1e-5f;
}

// ---- inputs: a generator of its own (splitmix64), so that the set depends on the seed alone
uint64_t g_state;
uint64_t next64()
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double uniform(const double lo, const double hi) { return lo + (hi - lo) * (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
void unit_double(double v[3])
{
    double q;
    do
    {
        for (int a = 0; a < 3; ++a)
            v[a] = uniform(-1, 1);
        q = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    } while (q >= 1 || q < 1e-4);
    for (int a = 0; a < 3; ++a)
        v[a] /= sqrt(q);
}
V3 random_unit()
{
    double v[3];
    unit_double(v);
    return unit(V3{(float)v[0], (float)v[1], (float)v[2]}); // a direction as the kernels hold it: normalised in fp32
}
// a unit vector at cosine c to n (double arithmetic, then normalised in fp32 like every ray direction)
V3 at_cosine(const V3 n, const double c)
{
    double t[3], nn[3] = {n.x, n.y, n.z};
    for (;;)
    {
        unit_double(t);
        const double along = t[0] * nn[0] + t[1] * nn[1] + t[2] * nn[2];
        double q = 0;
        for (int a = 0; a < 3; ++a)
            t[a] -= along * nn[a], q += t[a] * t[a];
        if (q < 1e-3)
            continue;
        const double s = sqrt(fmax(0.0, 1 - c * c) / q);
        return unit(V3{(float)(c * nn[0] + s * t[0]), (float)(c * nn[1] + s * t[1]), (float)(c * nn[2] + s * t[2])});
    }
}
void random_streams(uint32_t st[5])
{
    for (int a = 0; a < 5; ++a)
        st[a] = (uint32_t)next64() | 1u; // (xorshift32 has no zero state)
}
float random_index() { return (float)exp(uniform(log(0.3), log(3.0))); }
float random_param(const int type) { return type == 2 ? random_index() : (float)uniform(0, 1); }
V3 random_point() { return V3{(float)uniform(-20, 20), (float)uniform(-20, 20), (float)uniform(-20, 20)}; }

const float INDICES[] = {0.001f, 0.5f, 2.0f / 3.0f, 1.0f, 1.5f, 2.4f, 1000.0f};

void every_material(const V3 d, const V3 n)
{
    uint32_t st[5];
    random_streams(st);
    const V3 hp = random_point();
    check(d, n, hp, 0, 0.0f, st);
    check(d, n, hp, 1, 0.0f, st);
    check(d, n, hp, 1, 1.0f, st);
    for (const float idx : INDICES)
        check(d, n, hp, 2, idx, st);
}

void edges()
{
    // components that are +-0 next to exact ones: every pair of vectors of length one from these eight values (ddn = +-0 among them:
    // orthogonal axes in every sign of zero, and (0.6, 0.8, 0) . (0.8, -0.6, 0), whose two products cancel)
    const float S[8] = {0.0f, -0.0f, 1.0f, -1.0f, 0.6f, -0.6f, 0.8f, -0.8f};
    V3 units[512];
    int nu = 0;
    for (int i = 0; i < 512; ++i)
    {
        const V3 v{S[i & 7], S[(i >> 3) & 7], S[i >> 6]};
        if (fabsf(r1s_dot(v, v) - 1.0f) < 1e-6f)
            units[nu++] = v;
    }
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < nu; ++j)
            every_material(units[i], units[j]);
    // grazing incidence: |cosine| from 0 to 1e-3, both sides
    for (int q = 0; q < 20000; ++q)
    {
        const V3 n = random_unit();
        const double c = (q % 8 == 0 ? 0.0 : exp(uniform(log(1e-9), log(1e-3)))) * (q & 1 ? 1 : -1);
        every_material(at_cosine(n, c), n);
    }
    // total reflection: discriminant = 1 - r^2 (1 - dt^2) crosses zero at dt^2 = 1 - 1 / r^2, r = ni_over_nt > 1 — leaving an index
    // above one (ddn > 0), or entering an index below one (ddn < 0).  Cosines a few 1e-7 to either side of that, and exactly there
    for (int q = 0; q < 200000; ++q)
    {
        const bool leaving = q & 1;
        const double r = exp(uniform(log(1.0005), log(3.0)));
        const float idx = (float)(leaving ? r : 1 / r);
        const double rr = leaving ? (double)idx : 1.0 / (double)idx;
        const double crit = sqrt(fmax(0.0, 1 - 1 / (rr * rr)));
        const double off = (q % 5 == 0 ? 0.0 : exp(uniform(log(1e-8), log(1e-4)))) * ((q >> 1) & 1 ? 1 : -1);
        const V3 n = random_unit();
        const V3 d = at_cosine(n, (leaving ? 1 : -1) * fmin(1.0, fmax(0.0, crit + off)));
        uint32_t st[5];
        random_streams(st);
        check(d, n, random_point(), 2, idx, st);
    }
}

} // namespace

int main(int argc, char **argv)
{
    const uint64_t count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 2026ull;
    edges();
    const uint64_t edge_inputs = C.inputs;
    for (uint64_t i = 0; i < count; ++i)
    {
        const int type = (int)(i % 3);
        uint32_t st[5];
        random_streams(st);
        check(random_unit(), random_unit(), random_point(), type, random_param(type), st);
    }
#define SHOW(f) printf(#f " %llu\n", (unsigned long long)C.f);
    printf("edge_inputs %llu\nrandom_inputs %llu\n", (unsigned long long)edge_inputs, (unsigned long long)(C.inputs - edge_inputs));
    SHOW(mismatches) SHOW(ddn_pos_zero) SHOW(ddn_neg_zero) SHOW(zero_components) SHOW(grazing) SHOW(inside) SHOW(outside) SHOW(total_reflection)
    SHOW(refracting) SHOW(just_above) SHOW(index_below_one) SHOW(index_above_one) SHOW(fuzz_zero) SHOW(fuzz_one) SHOW(chose_reflected)
    SHOW(chose_refracted) SHOW(metal_absorbed)
    return C.mismatches == 0 ? 0 : 1;
}
