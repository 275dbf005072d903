// r1_queries_host.cpp — the ray, path and scatter queries on the host, no GPU: r1_cast_rays_host, r1_trace_rays_host, r1_scatter_rays_host
// and r1_camera_rays (include/rays1.h), and r1_render_features_host, their fold into a feature frame (§4.38).  Every ray against every active sphere in index order, in the reference's arithmetic — its
// two FMA chains written with fmaf, everything else operation by operation (this file is compiled with -ffp-contract=off).

#include "../../include/rays1.h"
#include "../../include/rays1_seed.h"
#include "r1_internal.h"
#include "r1_host_math.h"

#include <float.h>
#include <math.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

int r1_active_spheres(const r1_scene *s, std::vector<uint32_t> &active_to_scene); // inv_radius != 0, finite (r1_bvh.cpp)

static_assert(sizeof(r1_ray) == 32 && sizeof(r1_hit) == 32, "the device reads and writes these layouts");
static_assert(sizeof(r1_radiance) == 16 && sizeof(r1_sample_seed) == 16 && sizeof(r1_scatter) == 32, "the device reads and writes these layouts");

namespace
{

using namespace r1_host_math;

inline bool finite_f(float v)
{
    uint32_t b;
    memcpy(&b, &v, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// Ray(o, d) as the reference's constructor makes it (rayweek1.cpp:107: unit_vector, mymath.h:211); false: the origin or the normalised
// direction is not finite — a miss, or no color(), without a hit test
inline bool ray_start(const r1_ray &r, V3 &o, V3 &d)
{
    o = {r.o[0], r.o[1], r.o[2]};
    d = unit({r.d[0], r.d[1], r.d[2]});
    return finite_f(o.x) && finite_f(o.y) && finite_f(o.z) && finite_f(d.x) && finite_f(d.y) && finite_f(d.z);
}

// what one sphere offers a ray (exact_offer of r1_hit_sweep.hpp, host_offer of r1_grid.cpp)
inline float cast_offer(const float *e, const V3 o, const V3 d)
{
    const float cox = e[0] - o.x, coy = e[1] - o.y, coz = e[2] - o.z;
    const float nb = fmaf(coz, d.z, fmaf(coy, d.y, cox * d.x));
    const float c = fmaf(coz, coz, fmaf(coy, coy, cox * cox)) - e[3];
    const float discr = nb * nb - c;
    uint32_t bits;
    memcpy(&bits, &discr, 4);
    float offer = FLT_MAX;
    if (!(bits >> 31))
    {
        const float root = sqrtf(discr);
        const float t1 = nb - root;
        const float t = (t1 > 0.001f) ? t1 : nb + root;
        if (t > 0.001f && t < FLT_MAX)
            offer = t;
    }
    return offer;
}

// Hitable::hit(r, 0.001f, FLT_MAX, rec) (rayweek1.cpp:152-339): the active sphere with the smallest offer — a sphere's offer is fixed
// before the compare with t_max (the comment above exact_offer in r1_hit_sweep.hpp derives it) — or na: none.  ex: [active] {cx cy cz radius_sq}
inline size_t closest(const std::vector<float> &ex, const size_t na, const V3 o, const V3 d, float &best)
{
    size_t hit = na;
    best = FLT_MAX;
    for (size_t a = 0; a < na; ++a)
    {
        const float t = cast_offer(&ex[4 * a], o, d);
        if (t < best) // (ascending index: a tie keeps the earlier sphere)
            best = t, hit = a;
    }
    return hit;
}

// the active spheres of a scene and their {cx cy cz radius_sq}
int exact_table(const r1_scene *s, std::vector<uint32_t> &scene_index, std::vector<float> &ex)
{
    if (r1_active_spheres(s, scene_index) != R1_OK)
        return R1_EINVAL;
    ex.resize(4 * scene_index.size() + 4);
    for (size_t a = 0; a < scene_index.size(); ++a)
    {
        const uint32_t i = scene_index[a];
        ex[4 * a + 0] = s->center_x[i], ex[4 * a + 1] = s->center_y[i], ex[4 * a + 2] = s->center_z[i], ex[4 * a + 3] = s->radius_sq[i];
    }
    return R1_OK;
}

// range(i0, i1) over [0, n) on host threads: pieces of at least 256 rays, at most 16 threads (results do not depend on the split: rays
// are independent)
template <class RANGE>
void split_rays(const size_t n, RANGE range)
{
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = hw ? (hw > 16u ? 16u : hw) : 1u;
    if (nt > (n + 255) / 256)
        nt = (n + 255) / 256;
    if (nt <= 1)
    {
        range((size_t)0, n);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (n + nt - 1) / nt;
    for (size_t t = 0; t < nt; ++t)
    {
        const size_t i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
        if (i0 < i1)
            pool.emplace_back(range, i0, i1);
    }
    for (std::thread &th : pool)
        th.join();
}

// ---- ray queries: Hitable::hit(Ray(o, d), 0.001f, t_max, &rec) (rayweek1.cpp:104-108) ------------------------------------------------------
// The result is the minimum offer, ties to the lowest index, accepted only if it is < t_max: the compare is strict, as rayweek1.cpp:298 / :307.
void cast_range(const std::vector<float> &ex, const std::vector<uint32_t> &scene_index, const r1_scene *s, int32_t mode, const r1_ray *rays,
                size_t i0, size_t i1, void *out)
{
    const size_t na = scene_index.size();
    for (size_t i = i0; i < i1; ++i)
    {
        const r1_ray &r = rays[i];
        V3 o, d;
        float t_max = r.t_max;
        if (t_max > FLT_MAX) // +inf
            t_max = FLT_MAX;
        const bool valid = ray_start(r, o, d) && t_max > 0.001f; // (false for NaN)
        float best = FLT_MAX;
        const size_t best_a = valid ? closest(ex, na, o, d, best) : na;
        const bool hit = best_a != na && best < t_max;
        if (mode == R1_CAST_ANY)
        {
            ((uint8_t *)out)[i] = hit ? 1 : 0;
            continue;
        }
        r1_hit h;
        memset(&h, 0, sizeof(h));
        h.t = FLT_MAX, h.index = -1;
        if (hit)
        {
            const uint32_t k = scene_index[best_a];
            h.t = best, h.index = (int32_t)k;
            const V3 hp = add(o, scale(d, best)); // point_at_parameter: _origin + t * _dir
            h.p[0] = hp.x, h.p[1] = hp.y, h.p[2] = hp.z;
            h.n[0] = (hp.x - s->center_x[k]) * s->inv_radius[k];
            h.n[1] = (hp.y - s->center_y[k]) * s->inv_radius[k];
            h.n[2] = (hp.z - s->center_z[k]) * s->inv_radius[k];
        }
        ((r1_hit *)out)[i] = h;
    }
}

// ---- path queries: color(Ray(o, d), scene, 0) (rayweek1.cpp:517-534) for caller-supplied rays and stream states --------------------------
// Per level the hit test above, then the level's scatter in scalar C++, operation by operation in the reference's order — what
// shade_level of r1_shade.hpp does on the device, with the same host-made material constants (r1_sweep.cpp).  The attenuations are
// applied innermost first once the path has reached the sky: a0 * (a1 * (... * sky)), rayweek1.cpp:525.

// mymath.h:17-35 (the x4 forms :41-73 lane by lane)
inline uint32_t xorshift32(uint32_t &state)
{
    uint32_t x = state;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 15;
    state = x;
    return x;
}
inline float rand01(uint32_t &s) { return (float)(xorshift32(s) & 0xFFFFFFu) * (1.0f / 16777216.0f); }
// myrand02 - 1: the product with 2^-23 is exact, so the fused form rounds once, where the reference's subtraction rounds
inline float rand02_minus1(uint32_t &s) { return fmaf((float)(xorshift32(s) & 0xFFFFFFu), 1.0f / 8388608.0f, -1.0f); }

struct TraceScene
{
    std::vector<float> ex;              // [active] {cx cy cz radius_sq}
    std::vector<float> shade;           // [active] {inv_radius, albedo rgb}
    std::vector<float> mat;             // [active] {param, 1 / ref_idx, ((1 - ref) / (1 + ref))^2}
    std::vector<uint8_t> type;
    std::vector<uint32_t> scene_index;  // [active] index into the r1_scene arrays
};

// One color() level behind the Ray constructor (rayweek1.cpp:519-534) for the unit ray (o, d): the hit test, then the sky, or — where
// may_scatter says that the depth limit allows it — the hit arm: hit record, draws, Material::scatter, the scattered ray in (o, d) and
// the advanced stream states in sd.  r1_trace_rays_host is the fold of this function (trace_range), r1_scatter_rays_host one call of it
// per ray (scatter_range): the two cannot drift apart.
struct Level
{
    int event;    // R1_SCATTER_SCATTERED, _SKY, _ABSORBED; LEVEL_LIMIT: a hit at the depth limit (no scatter, no draws: black)
    size_t hit;   // the active sphere, na without a hit
    float t;      // the hit distance, FLT_MAX without a hit
    V3 weight;    // SKY: the sky's colour; SCATTERED: the attenuation (albedo; 1 for a dielectric); else 0
};
enum { LEVEL_LIMIT = -1 };

inline Level level(const TraceScene &T, V3 &o, V3 &d, r1_sample_seed &sd, const bool may_scatter)
{
    const size_t na = T.type.size();
    Level L = {R1_SCATTER_SKY, na, FLT_MAX, {0, 0, 0}};
    // Hitable::hit(r, 0.001f, FLT_MAX, rec), rayweek1.cpp:519
    float best;
    const size_t hit = closest(T.ex, na, o, d, best);
    if (hit == na)
    {
        // sky (rayweek1.cpp:532-534), lerp = (1 - t) * a + t * b (mymath.h:212-216)
        const float t = 0.5f * (d.y + 1.0f);
        const float omt = 1.0f - t;
        L.weight = {omt * 1.0f + t * 0.5f, omt * 1.0f + t * 0.7f, omt * 1.0f + t * 1.0f};
        return L;
    }
    L.hit = hit, L.t = best;
    if (!may_scatter)
    {
        L.event = LEVEL_LIMIT; // depth == MAX_BOUNCES: black (rayweek1.cpp:523-528)
        return L;
    }
    // hit record (rayweek1.cpp:316-322)
    const float *e = &T.ex[4 * hit], *sh = &T.shade[4 * hit], *mt = &T.mat[3 * hit];
    const V3 hp = add(o, scale(d, best));
    const V3 n = scale(sub(hp, {e[0], e[1], e[2]}), sh[0]);
    const uint8_t type = T.type[hit];
    V3 rius = {0, 0, 0};
    if (type != R1_MAT_DIELECTRIC) // random_in_unit_sphere, mymath.h:224-235 (Lambertian and Metal both draw it, rayweek1.cpp:405, :430)
        do
        {
            rius = {rand02_minus1(sd.lane0), rand02_minus1(sd.lane1), rand02_minus1(sd.lane2)};
        } while (dot(rius, rius) >= 1);
    V3 dir;
    if (type == R1_MAT_LAMBERTIAN)
    {
        const V3 target = add(add(hp, n), rius); // rayweek1.cpp:403-409
        dir = sub(target, hp);
    }
    else if (type == R1_MAT_METAL)
    {
        const V3 refl = sub(d, scale(n, 2.0f * dot(d, n))); // rayweek1.cpp:427-433, reflect :414-417
        dir = add(refl, scale(rius, mt[0]));
    }
    else
    {
        // Dielectric::scatter rayweek1.cpp:470-511
        const float ref_idx = mt[0];
        const float ddn = dot(d, n);
        const V3 reflected = sub(d, scale(n, 2.0f * ddn));
        V3 outward;
        float ni_over_nt, cosine;
        if (ddn > 0)
        {
            outward = {-n.x, -n.y, -n.z};
            ni_over_nt = ref_idx;
            cosine = ref_idx * ddn;
        }
        else
        {
            outward = n;
            ni_over_nt = mt[1];
            cosine = -ddn;
        }
        // refract rayweek1.cpp:439-452
        const float dt = dot(d, outward);
        const float discriminant = 1.0f - ni_over_nt * ni_over_nt * (1.0f - dt * dt);
        float reflect_prob = 1.0f;
        V3 refracted = {0, 0, 0};
        if (discriminant > 0)
        {
            refracted = sub(scale(sub(d, scale(outward, dt)), ni_over_nt), scale(outward, sqrtf(discriminant)));
            // schlick rayweek1.cpp:454-459, x^5 exactly rounded (r1s_pow5 of r1_scatter.h)
            const float r0 = mt[2];
            const double x = (double)(1.0f - cosine), x2 = x * x;
            reflect_prob = r0 + (1.0f - r0) * (float)(x2 * x2 * x);
        }
        dir = (rand01(sd.scalar) < reflect_prob) ? reflected : refracted;
    }
    const V3 nd = unit(dir);
    o = hp, d = nd;
    if (type == R1_MAT_DIELECTRIC)
        L.event = R1_SCATTER_SCATTERED, L.weight = {1.0f, 1.0f, 1.0f}; // (attenuation 1, rayweek1.cpp:473)
    else if (type == R1_MAT_LAMBERTIAN || dot(nd, n) > 0)
        L.event = R1_SCATTER_SCATTERED, L.weight = {sh[1], sh[2], sh[3]};
    else
        L.event = R1_SCATTER_ABSORBED; // Metal::scatter() == false: black (rayweek1.cpp:432, :528)
    return L;
}

void trace_range(const TraceScene &T, int32_t max_bounces, const r1_ray *rays, const r1_sample_seed *seeds, size_t i0, size_t i1, r1_radiance *out)
{
    std::vector<uint32_t> stack((size_t)max_bounces);
    for (size_t i = i0; i < i1; ++i)
    {
        V3 o, d;
        r1_radiance rec = {0.0f, 0.0f, 0.0f, 0u};
        if (!ray_start(rays[i], o, d))
        {
            out[i] = rec; // no color()
            continue;
        }
        r1_sample_seed sd = r1_seed_guard(seeds ? seeds[i] : r1_seed_sample(0u, (uint32_t)i, 0u));
        int depth = 0, sp = 0;
        V3 col = {0, 0, 0};
        for (;;)
        {
            const Level L = level(T, o, d, sd, depth < max_bounces);
            if (L.event == R1_SCATTER_SKY)
            {
                // the attenuations innermost first: a0 * (a1 * (... * sky)), rayweek1.cpp:525
                col = L.weight;
                for (int e = sp - 1; e >= 0; --e)
                {
                    const float *sh = &T.shade[4 * (size_t)stack[e]];
                    col = {sh[1] * col.x, sh[2] * col.y, sh[3] * col.z};
                }
                break;
            }
            if (L.event != R1_SCATTER_SCATTERED)
                break; // the depth limit, or Metal::scatter() == false: black
            if (T.type[L.hit] != R1_MAT_DIELECTRIC)
                stack[sp++] = (uint32_t)L.hit;
            ++depth;
        }
        rec.r = col.x, rec.g = col.y, rec.b = col.z, rec.rays = (uint32_t)depth + 1u; // every level counts one ray (rayweek1.cpp:517)
        out[i] = rec;
    }
}

// ---- scatter queries: one level per ray (include/rays1.h "scatter queries") ---------------------------------------------
void scatter_range(const TraceScene &T, int32_t flags, const r1_ray *rays, const r1_sample_seed *seeds, size_t i0, size_t i1, r1_ray *rays_out,
                   r1_sample_seed *seeds_out, r1_scatter *out)
{
    for (size_t i = i0; i < i1; ++i)
    {
        const r1_ray in = rays[i]; // (read before anything of ray i is written: rays_out may be rays, seeds_out may be seeds)
        r1_sample_seed sd = r1_seed_guard(seeds ? seeds[i] : r1_seed_sample(0u, (uint32_t)i, 0u));
        V3 o, d;
        bool valid;
        if (flags & R1_SCATTER_UNIT_DIRECTIONS)
        {
            o = {in.o[0], in.o[1], in.o[2]}, d = {in.d[0], in.d[1], in.d[2]};
            valid = finite_f(o.x) && finite_f(o.y) && finite_f(o.z) && finite_f(d.x) && finite_f(d.y) && finite_f(d.z);
        }
        else
            valid = ray_start(in, o, d);
        r1_scatter rec;
        r1_ray next;
        memset(&rec, 0, sizeof(rec)), memset(&next, 0, sizeof(next));
        rec.event = R1_SCATTER_NONE, rec.t = FLT_MAX, rec.index = -1, rec.mat_type = R1_MAT_NONE;
        if (valid)
        {
            const Level L = level(T, o, d, sd, true);
            rec.event = L.event;
            rec.weight[0] = L.weight.x, rec.weight[1] = L.weight.y, rec.weight[2] = L.weight.z;
            if (L.event != R1_SCATTER_SKY)
            {
                rec.t = L.t, rec.index = (int32_t)T.scene_index[L.hit], rec.mat_type = T.type[L.hit];
                next.o[0] = o.x, next.o[1] = o.y, next.o[2] = o.z, next.t_max = FLT_MAX;
                next.d[0] = d.x, next.d[1] = d.y, next.d[2] = d.z;
            }
        }
        out[i] = rec, rays_out[i] = next, seeds_out[i] = sd;
    }
}

// the tables of a scene's active spheres as the levels read them; who: the entry point, for r1_last_error
bool null_scene(const char *who, const r1_scene *s)
{
    if (s && (!s->count || (s->center_x && s->center_y && s->center_z && s->radius_sq && s->inv_radius && s->mat_type && s->albedo_r && s->albedo_g &&
                            s->albedo_b && s->mat_param)))
        return false;
    r1_set_error("%s: null scene", who);
    return true;
}

int trace_scene(const char *who, const r1_scene *s, TraceScene &T)
{
    if (exact_table(s, T.scene_index, T.ex) != R1_OK)
        return R1_EINVAL;
    const size_t na = T.scene_index.size();
    T.shade.resize(4 * na + 4), T.mat.resize(3 * na + 3), T.type.resize(na);
    for (size_t a = 0; a < na; ++a)
    {
        const uint32_t i = T.scene_index[a];
        if (s->mat_type[i] > R1_MAT_DIELECTRIC)
        {
            r1_set_error("%s: sphere %u is hittable but has no material", who, i);
            return R1_EINVAL;
        }
        T.shade[4 * a + 0] = s->inv_radius[i], T.shade[4 * a + 1] = s->albedo_r[i], T.shade[4 * a + 2] = s->albedo_g[i], T.shade[4 * a + 3] = s->albedo_b[i];
        // the dielectric's constants as the device tables hold them (r1_sweep.cpp; rayweek1.cpp:489, :456-457): same IEEE operations, done once
        const float ref_idx = s->mat_param[i];
        float r0 = (1 - ref_idx) / (1 + ref_idx);
        r0 = r0 * r0;
        T.mat[3 * a + 0] = ref_idx, T.mat[3 * a + 1] = 1.0f / ref_idx, T.mat[3 * a + 2] = r0;
        T.type[a] = s->mat_type[i];
    }
    return R1_OK;
}

} // namespace

extern "C" int r1_cast_rays_host(const r1_scene *s, int32_t mode, const r1_ray *rays, size_t n, void *out)
{
    if (mode != R1_CAST_CLOSEST && mode != R1_CAST_ANY)
    {
        r1_set_error("r1_cast_rays_host: mode %d is neither R1_CAST_CLOSEST nor R1_CAST_ANY", mode);
        return R1_EINVAL;
    }
    if (!s || (s->count && (!s->center_x || !s->center_y || !s->center_z || !s->radius_sq || !s->inv_radius)))
    {
        r1_set_error("r1_cast_rays_host: null scene");
        return R1_EINVAL;
    }
    if (n == 0)
        return R1_OK;
    if (!rays || !out)
    {
        r1_set_error("r1_cast_rays_host: null rays or out with n > 0");
        return R1_EINVAL;
    }
    std::vector<uint32_t> scene_index;
    std::vector<float> ex;
    if (exact_table(s, scene_index, ex) != R1_OK)
        return R1_EINVAL;
    split_rays(n, [&](size_t i0, size_t i1) { cast_range(ex, scene_index, s, mode, rays, i0, i1, out); });
    return R1_OK;
}

extern "C" int r1_trace_rays_host(const r1_scene *s, int32_t max_bounces, const r1_ray *rays, const r1_sample_seed *seeds, size_t n, r1_radiance *out)
{
    if (max_bounces < 1 || max_bounces > R1_MAX_BOUNCES_LIMIT)
    {
        r1_set_error("r1_trace_rays_host: max_bounces %d is not in 1..%d", max_bounces, R1_MAX_BOUNCES_LIMIT);
        return R1_EINVAL;
    }
    if (null_scene("r1_trace_rays_host", s))
        return R1_EINVAL;
    if (n == 0)
        return R1_OK;
    if (!rays || !out)
    {
        r1_set_error("r1_trace_rays_host: null rays or out with n > 0");
        return R1_EINVAL;
    }
    TraceScene T;
    if (trace_scene("r1_trace_rays_host", s, T) != R1_OK)
        return R1_EINVAL;
    split_rays(n, [&](size_t i0, size_t i1) { trace_range(T, max_bounces, rays, seeds, i0, i1, out); });
    return R1_OK;
}

extern "C" int r1_scatter_rays_host(const r1_scene *s, int32_t flags, const r1_ray *rays, const r1_sample_seed *seeds, size_t n, r1_ray *rays_out,
                                    r1_sample_seed *seeds_out, r1_scatter *out)
{
    if (flags & ~R1_SCATTER_UNIT_DIRECTIONS)
    {
        r1_set_error("r1_scatter_rays_host: flags %d has bits other than R1_SCATTER_UNIT_DIRECTIONS", flags);
        return R1_EINVAL;
    }
    if (null_scene("r1_scatter_rays_host", s))
        return R1_EINVAL;
    if (n == 0)
        return R1_OK;
    if (!rays || !rays_out || !seeds_out || !out)
    {
        r1_set_error("r1_scatter_rays_host: null rays, rays_out, seeds_out or out with n > 0");
        return R1_EINVAL;
    }
    TraceScene T;
    if (trace_scene("r1_scatter_rays_host", s, T) != R1_OK)
        return R1_EINVAL;
    split_rays(n, [&](size_t i0, size_t i1) { scatter_range(T, flags, rays, seeds, i0, i1, rays_out, seeds_out, out); });
    return R1_OK;
}

// ---- feature frames (include/rays1.h "feature frames") --------------------------------------------------------------------
// The checker of r1_render_features*: per pixel of the window r1_camera_rays for its spp samples, cast_range — r1_cast_rays_host's loop — for
// their R1_CAST_CLOSEST records, and the seven sums as plain fp32 adds in sample order, times (float)(1.0f / spp).
extern "C" int r1_render_features_host(const r1_scene *s, const r1_camera *cam, const r1_params *p, const r1_region *region, r1_feature *out)
{
    if (!s || !cam || !p || !out)
    {
        r1_set_error("r1_render_features_host: null scene, camera, params or out");
        return R1_EINVAL;
    }
    const r1_region whole = {0, 0, p->width, p->height, 0};
    const r1_region win = region ? *region : whole;
    int rc = r1_region_check(p, &win);
    if (rc)
        return rc;
    if (s->count && (!s->center_x || !s->center_y || !s->center_z || !s->radius_sq || !s->inv_radius || !s->mat_type || !s->albedo_r || !s->albedo_g || !s->albedo_b))
    {
        r1_set_error("r1_render_features_host: null scene");
        return R1_EINVAL;
    }
    std::vector<uint32_t> scene_index;
    std::vector<float> ex;
    if (exact_table(s, scene_index, ex) != R1_OK)
        return R1_EINVAL;
    const size_t spp = (size_t)p->spp, stride = win.out_stride ? (size_t)win.out_stride : (size_t)win.width;
    const float inv = (float)(1.0f / p->spp); // rayweek1.cpp:765
    std::atomic<int> failed(R1_OK); // (r1_camera_rays cannot fail on a checked window; kept for the day it can)
    // (pixels of the window, row-major, on host threads: they are independent)
    split_rays((size_t)win.width * (size_t)win.height, [&](size_t i0, size_t i1) {
        std::vector<int32_t> xs(spp), ys(spp), ss(spp);
        std::vector<r1_ray> rays(spp);
        std::vector<r1_sample_seed> seeds(spp);
        std::vector<r1_hit> hits(spp);
        for (size_t k = 0; k < spp; ++k)
            ss[k] = (int32_t)k;
        for (size_t i = i0; i < i1; ++i)
        {
            const size_t wy = i / (size_t)win.width, wx = i % (size_t)win.width;
            for (size_t k = 0; k < spp; ++k)
                xs[k] = win.x0 + (int32_t)wx, ys[k] = win.y0 + (int32_t)wy;
            if (r1_camera_rays(cam, p, xs.data(), ys.data(), ss.data(), spp, rays.data(), seeds.data()) != R1_OK)
            {
                failed = R1_EINVAL;
                return;
            }
            cast_range(ex, scene_index, s, R1_CAST_CLOSEST, rays.data(), 0, spp, hits.data());
            r1_feature f;
            memset(&f, 0, sizeof(f));
            for (size_t k = 0; k < spp; ++k)
            {
                V3 o, d;
                if (!ray_start(rays[k], o, d))
                    continue; // a non-finite ray: nothing is added
                const r1_hit &h = hits[k];
                if (h.index >= 0)
                {
                    const bool glass = s->mat_type[h.index] == R1_MAT_DIELECTRIC; // (attenuation 1, rayweek1.cpp:473)
                    f.albedo[0] += glass ? 1.0f : s->albedo_r[h.index];
                    f.albedo[1] += glass ? 1.0f : s->albedo_g[h.index];
                    f.albedo[2] += glass ? 1.0f : s->albedo_b[h.index];
                    f.normal[0] += h.n[0], f.normal[1] += h.n[1], f.normal[2] += h.n[2];
                    f.depth += h.t;
                    f.hits += 1u;
                }
                else
                {
                    // sky (rayweek1.cpp:532-534), lerp = (1 - t) * a + t * b (mymath.h:212-216)
                    const float t = 0.5f * (d.y + 1.0f);
                    const float omt = 1.0f - t;
                    f.albedo[0] += omt * 1.0f + t * 0.5f, f.albedo[1] += omt * 1.0f + t * 0.7f, f.albedo[2] += omt * 1.0f + t * 1.0f;
                }
            }
            for (int k = 0; k < 3; ++k)
                f.albedo[k] *= inv, f.normal[k] *= inv;
            f.depth *= inv;
            out[wy * stride + wx] = f;
        }
    });
    if (failed != R1_OK)
        r1_set_error("r1_render_features_host: r1_camera_rays refused a sample of the window");
    return failed;
}

// rayweek1.cpp:757-760 under the seeding contract — start_ray of r1_sample.hpp on the host, without the Ray constructor's normalisation
extern "C" int r1_camera_rays(const r1_camera *cam, const r1_params *p, const int32_t *x, const int32_t *y, const int32_t *s, size_t n, r1_ray *rays_out,
                              r1_sample_seed *seeds_out)
{
    if (!cam || !p || p->width <= 0 || p->height <= 0)
    {
        r1_set_error("r1_camera_rays: null camera or params, or an empty image");
        return R1_EINVAL;
    }
    if (n == 0)
        return R1_OK;
    if (!x || !y || !s || !rays_out || !seeds_out)
    {
        r1_set_error("r1_camera_rays: null x, y, s, rays_out or seeds_out with n > 0");
        return R1_EINVAL;
    }
    for (size_t i = 0; i < n; ++i)
        if (x[i] < 0 || x[i] >= p->width || y[i] < 0 || y[i] >= p->height || s[i] < 0)
        {
            r1_set_error("r1_camera_rays: sample %zu is (%d, %d, %d): outside the %dx%d image, or s < 0", i, x[i], y[i], s[i], p->width, p->height);
            return R1_EINVAL;
        }
    const float inv_w = 1.0f / p->width, inv_h = 1.0f / p->height; // rayweek1.cpp:746
    const V3 cu = {cam->u[0], cam->u[1], cam->u[2]}, cv = {cam->v[0], cam->v[1], cam->v[2]}, org = {cam->origin[0], cam->origin[1], cam->origin[2]};
    const V3 ll = {cam->lower_left[0], cam->lower_left[1], cam->lower_left[2]}, hor = {cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]};
    const V3 ver = {cam->vertical[0], cam->vertical[1], cam->vertical[2]};
    for (size_t i = 0; i < n; ++i)
    {
        r1_sample_seed sd = r1_seed_sample(p->seed, (uint32_t)(y[i] * p->width + x[i]), (uint32_t)s[i]);
        // uv = (myrand01_x4(state4) + (x, y)) * (1/W, 1/H): lanes 0, 1 used, lane 2 advances too
        const float j0 = rand01(sd.lane0), j1 = rand01(sd.lane1);
        (void)xorshift32(sd.lane2);
        const float u = (j0 + (float)x[i]) * inv_w;
        const float v = (j1 + (float)y[i]) * inv_h;
        // random_in_unit_disk (rayweek1.cpp:353-362): g++ argument order => y gets the first draw
        V3 dk;
        do
        {
            const float first = rand02_minus1(sd.scalar);
            const float second = rand02_minus1(sd.scalar);
            dk = {second, first, 0.0f};
        } while (dot(dk, dk) >= 1.0f);
        // Camera::getRay (rayweek1.cpp:381-386)
        const V3 rd = scale(dk, cam->lens_radius);
        const V3 offset = add(scale(cu, rd.x), scale(cv, rd.y));
        const V3 ro = add(org, offset);
        const V3 dir = sub(sub(add(add(ll, scale(hor, u)), scale(ver, v)), org), offset);
        r1_ray &r = rays_out[i];
        r.o[0] = ro.x, r.o[1] = ro.y, r.o[2] = ro.z, r.t_max = FLT_MAX;
        r.d[0] = dir.x, r.d[1] = dir.y, r.d[2] = dir.z, r.pad = 0u;
        seeds_out[i] = sd;
    }
    return R1_OK;
}
