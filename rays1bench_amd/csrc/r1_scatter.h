// r1_scatter.h — the direction arithmetic of Material::scatter (rayweek1.cpp:403-409, :427-433, :470-511) for the three materials,
// shared by shade_level (r1_shade.hpp) and the host (tools/check_scatter_host.cpp, tests/test_scatter_host.py), so that the CPU
// test checks the kernels' own arithmetic.  The draws, the exact square root, the normalisation, the attenuation stack and the depth
// rule stay with the caller; what is here is + - x, compares and selects on fp32 (the build passes -ffp-contract=off), and x^5
// through double.  The vector type V is the caller's: any struct of three floats x, y, z.
//
// Reflection is computed once for Metal and Dielectric: ddn = dot(d, n), refl = d - n (2 ddn).  The arms are exclusive per lane, but
// a wave runs every arm one of its lanes takes, so what both need is issued once instead of twice.
//
// The Dielectric arm, R1_SCATTER_FORM:
//   1 (the default)  no outward normal.  With inside = ddn > 0:
//                        ni_over_nt = inside ? ref_idx : 1 / ref_idx        cosine = inside ? ref_idx ddn : -ddn
//                        dt         = inside ? -ddn : ddn
//                        refracted  = (d - n ddn) ni_over_nt - n (inside ? -root : root)
//   0                the reference's: outward = inside ? -n : n, dt = dot(d, outward),
//                        refracted  = (d - outward dt) ni_over_nt - outward root
//                    (what the kernels did before; kept for the A/B and the host comparison)
// Form 1 has the bits of form 0 for every input that is not a NaN:
//   * a product's magnitude does not depend on its operands' signs, and its sign — a zero's too — is the xor of theirs.  So
//     (-n.x) d.x = -(n.x d.x), (-n)(-ddn) = n ddn and (-n) root = n (-root), each exactly, zeros included;
//   * rounding to nearest is symmetric: RN(-a - b) = -RN(a + b) whenever a + b is not an exact zero.  dot(d, -n) is
//     (-p + -q) + -r for the three products p, q, r of dot(d, n) in the same order.  Form 0 takes it only for ddn > 0, where the last
//     sum is not zero; an exact zero of p + q has the same sign (+0) in both forms and vanishes in the sum with r, which is then not
//     zero itself.  Hence dt = -ddn exactly for ddn > 0, and for every other ddn (-0, +0, negative) outward is n and dt is ddn;
//   * every other operation, its operands' order, the order of the draws and the compare with the draw are the reference's.
// A NaN (a hit point at infinity) takes the same arm in both forms, since every compare with it is false; its sign bit is not
// defined by either.  tests/test_scatter_host.py compares the two forms and the oracle's scatter bit for bit on 10^7 random inputs
// and the edges (ddn = +-0, zero components, grazing incidence, both sides of total reflection); DESIGN.md §4.25.
#ifndef R1_SCATTER_H
#define R1_SCATTER_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define R1_SCATTER_HD __host__ __device__ __forceinline__
#else
#define R1_SCATTER_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#ifndef R1_SCATTER_FORM
#define R1_SCATTER_FORM 1
#endif

template <class V>
R1_SCATTER_HD V r1s_mk(const float x, const float y, const float z)
{
    V r;
    r.x = x, r.y = y, r.z = z;
    return r;
}

// mymath.h:205-207: sum(a*b) = (x + y) + z
template <class V>
R1_SCATTER_HD float r1s_dot(const V a, const V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// Lambertian::scatter rayweek1.cpp:403-409: target = p + normal + random_in_unit_sphere(); direction = target - p
template <class V>
R1_SCATTER_HD V r1s_lambertian(const V hp, const V n, const V rius)
{
    const V target = r1s_mk<V>((hp.x + n.x) + rius.x, (hp.y + n.y) + rius.y, (hp.z + n.z) + rius.z);
    return r1s_mk<V>(target.x - hp.x, target.y - hp.y, target.z - hp.z);
}

// reflect rayweek1.cpp:414-417: v - 2 * dot(v, n) * n, with ddn = dot(v, n)
template <class V>
R1_SCATTER_HD V r1s_reflect(const V d, const V n, const float ddn)
{
    const float k = 2.0f * ddn;
    return r1s_mk<V>(d.x - n.x * k, d.y - n.y * k, d.z - n.z * k);
}

// Metal::scatter rayweek1.cpp:427-433: reflected + fuzz * random_in_unit_sphere()
template <class V>
R1_SCATTER_HD V r1s_metal(const V refl, const V rius, const float fuzz)
{
    return r1s_mk<V>(refl.x + rius.x * fuzz, refl.y + rius.y * fuzz, refl.z + rius.z * fuzz);
}

// Dielectric::scatter rayweek1.cpp:470-511 up to the test of refract (:439-443): which side the ray comes from, and whether it refracts
struct R1Dielectric
{
    bool inside;        // dot(d, n) > 0: the ray leaves the sphere
    float ni_over_nt;
    float cosine;       // schlick's argument
    float dt;           // dot(d, outward normal)
    float discriminant; // > 0: the ray may refract, and its root is wanted
};

// inv_ref_idx = 1.0f / ref_idx, divided on the host (the same IEEE division)
template <int FORM, class V>
R1_SCATTER_HD R1Dielectric r1s_dielectric_form(const V d, const V n, const float ddn, const float ref_idx, const float inv_ref_idx)
{
    R1Dielectric k;
    k.inside = ddn > 0;
    k.ni_over_nt = k.inside ? ref_idx : inv_ref_idx;
    k.cosine = k.inside ? ref_idx * ddn : -ddn;
    if (FORM == 0)
    {
        const V outward = k.inside ? r1s_mk<V>(-n.x, -n.y, -n.z) : n;
        k.dt = r1s_dot(d, outward);
    }
    else
        k.dt = k.inside ? -ddn : ddn;
    k.discriminant = 1.0f - k.ni_over_nt * k.ni_over_nt * (1.0f - k.dt * k.dt);
    return k;
}

// refract rayweek1.cpp:444-447 for discriminant > 0: ni_over_nt * (uv - n * dt) - n * sqrt(discriminant), `root` the correctly rounded root
template <int FORM, class V>
R1_SCATTER_HD V r1s_refracted_form(const V d, const V n, const float ddn, const R1Dielectric k, const float root)
{
    if (FORM == 0)
    {
        const V o = k.inside ? r1s_mk<V>(-n.x, -n.y, -n.z) : n;
        return r1s_mk<V>((d.x - o.x * k.dt) * k.ni_over_nt - o.x * root, (d.y - o.y * k.dt) * k.ni_over_nt - o.y * root,
                         (d.z - o.z * k.dt) * k.ni_over_nt - o.z * root);
    }
    const float r = k.inside ? -root : root;
    return r1s_mk<V>((d.x - n.x * ddn) * k.ni_over_nt - n.x * r, (d.y - n.y * ddn) * k.ni_over_nt - n.y * r, (d.z - n.z * ddn) * k.ni_over_nt - n.z * r);
}

// exactly rounded x^5 (the reference calls powf(x, 5), rayweek1.cpp:458)
R1_SCATTER_HD float r1s_pow5(const float x)
{
    const double d = (double)x;
    const double d2 = d * d;
    return (float)(d2 * d2 * d);
}

// schlick rayweek1.cpp:454-459; r0 = ((1 - ref_idx) / (1 + ref_idx))^2 comes from the host
R1_SCATTER_HD float r1s_schlick(const float r0, const float cosine) { return r0 + (1.0f - r0) * r1s_pow5(1.0f - cosine); }

template <class V>
R1_SCATTER_HD R1Dielectric r1s_dielectric(const V d, const V n, const float ddn, const float ref_idx, const float inv_ref_idx)
{
    return r1s_dielectric_form<R1_SCATTER_FORM>(d, n, ddn, ref_idx, inv_ref_idx);
}
template <class V>
R1_SCATTER_HD V r1s_refracted(const V d, const V n, const float ddn, const R1Dielectric k, const float root)
{
    return r1s_refracted_form<R1_SCATTER_FORM>(d, n, ddn, k, root);
}

#endif
