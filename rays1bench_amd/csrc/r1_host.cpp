// r1_host.cpp — host-side half of librays1.so that needs no GPU: the scene builders,
// the tile/shard arithmetic and the reference's output formats, behind the C-ABI of
// include/rays1.h.
//
// Scene content follows the reference (citations: /root/reference/src/step13/):
//   create_small_scene  rayweek1.cpp:552-579      create_medium_scene rayweek1.cpp:582-651
//   create_large_scene  rayweek1.cpp:654-719      Camera::init        rayweek1.cpp:366-379
//   SphereSOA::add      soa_sphere.cpp:70-85      placeholders        rayweek1.cpp:574-576
// but the container is this build's own: one flat struct-of-arrays plus a flat material
// table (type, albedo, parameter) instead of `Material*`, because the device cannot follow
// host vtables.  Arithmetic that feeds the fixtures (tests/golden/scene_*.bin) is written
// operation by operation and this file is compiled with -ffp-contract=off.

#include "../../include/rays1.h"
#include "r1_internal.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>


namespace
{

struct V3
{
    float x, y, z;
};

inline V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
// mymath.h:205-207 — lanes are summed as (x + y) + z
inline float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// mymath.h:211
inline V3 unit(V3 v) { return scale(v, 1.0f / sqrtf(dot(v, v))); }
// mymath.h:190-197 after the lane shuffles
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

inline void store(float *dst, V3 v)
{
    dst[0] = v.x;
    dst[1] = v.y;
    dst[2] = v.z;
}

// Camera::init, rayweek1.cpp:366-379 (r1_camera_look_at and the scene builders)
inline void look_at(V3 lookfrom, V3 lookat, V3 vup, float vfov, float aspect, float aperture, float focus_dist, r1_camera &cam)
{
    cam.lens_radius = aperture / 2;
    // The reference calls tanf(theta / 2).  Its value for vfov = 60 depends on who evaluates
    // it: g++ folds the call at compile time (MPFR, correctly rounded: 0x1.279a74p-1, which
    // is what the fixture binary and any -O2/-O3 build of the reference contain) while
    // glibc's run-time tanf returns 0x1.279a76p-1.  Evaluating in double and rounding once
    // gives the correctly rounded value on every toolchain.
    float theta = vfov * (float)M_PI / 180;
    float half_height = (float)tan((double)(theta / 2));
    float half_width = aspect * half_height;
    V3 w = unit(sub(lookfrom, lookat));
    V3 u = unit(cross(vup, w));
    V3 v = cross(w, u);
    V3 ll = sub(sub(sub(lookfrom, scale(u, half_width * focus_dist)), scale(v, half_height * focus_dist)), scale(w, focus_dist));
    store(cam.origin, lookfrom);
    store(cam.lower_left, ll);
    store(cam.horizontal, scale(u, 2 * half_width * focus_dist));
    store(cam.vertical, scale(v, 2 * half_height * focus_dist));
    store(cam.u, u);
    store(cam.v, v);
    store(cam.w, w);
}

} // namespace

struct r1_host_scene
{
    std::vector<float> cx, cy, cz, rsq, invr, ar, ag, ab, param;
    std::vector<uint8_t> mtype;
    r1_scene view;
    r1_camera cam;

    // SphereSOA::add, soa_sphere.cpp:70-85
    void add(V3 c, float radius, uint8_t type, V3 albedo, float p)
    {
        cx.push_back(c.x);
        cy.push_back(c.y);
        cz.push_back(c.z);
        rsq.push_back(radius * radius);
        invr.push_back(radius > 0 ? (1.0f / radius) : 0);
        mtype.push_back(type);
        ar.push_back(albedo.x);
        ag.push_back(albedo.y);
        ab.push_back(albedo.z);
        param.push_back(p);
    }
    void lambertian(V3 c, float r, V3 a) { add(c, r, R1_MAT_LAMBERTIAN, a, 0); }
    // Metal::Metal clamps fuzz to <= 1, rayweek1.cpp:422-425
    void metal(V3 c, float r, V3 a, float fuzz) { add(c, r, R1_MAT_METAL, a, fuzz < 1 ? fuzz : 1); }
    // Dielectric attenuation is (1,1,1), rayweek1.cpp:472
    void dielectric(V3 c, float r, float ref_idx) { add(c, r, R1_MAT_DIELECTRIC, {1, 1, 1}, ref_idx); }

    // "make sure num spheres is multiple of SIMD width", rayweek1.cpp:574-576 (SIMD_WIDTH 8)
    void pad_to_simd_width()
    {
        while (cx.size() % 8 != 0)
            add({999999999.f, 999999999.f, 999999999.f}, 0, R1_MAT_NONE, {0, 0, 0}, 0);
    }

    // the arguments the builder gave Camera::init (r1_host_scene_view)
    V3 view_from = {0, 0, 0}, view_at = {0, 0, 0}, view_up = {0, 1, 0};
    float view_vfov = 0, view_aperture = 0, view_focus = 0;

    void camera_init(V3 lookfrom, V3 lookat, V3 vup, float vfov, float aspect, float aperture, float focus_dist)
    {
        view_from = lookfrom, view_at = lookat, view_up = vup;
        view_vfov = vfov, view_aperture = aperture, view_focus = focus_dist;
        look_at(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, cam);
    }

    void finish()
    {
        view.count = (uint32_t)cx.size();
        view.center_x = cx.data();
        view.center_y = cy.data();
        view.center_z = cz.data();
        view.radius_sq = rsq.data();
        view.inv_radius = invr.data();
        view.mat_type = mtype.data();
        view.albedo_r = ar.data();
        view.albedo_g = ag.data();
        view.albedo_b = ab.data();
        view.mat_param = param.data();
    }
};

namespace
{

void build_small(r1_host_scene &s, float aspect)
{
    s.camera_init({2, 1, 2}, {0, 0, 0}, {0, 1, 0}, 60, aspect, 0.1f, 5.0f);
    s.lambertian({0, 0, -1}, 0.5f, {0.1f, 0.2f, 0.5f});
    s.lambertian({0, -100.5f, -1}, 100.0f, {0.8f, 0.8f, 0});
    s.metal({1, 0, -1}, 0.5f, {0.8f, 0.6f, 0.2f}, 0.3f);
    s.dielectric({-1, 0, -1}, 0.5f, 1.5f);
    s.dielectric({-1, 0, -1}, -0.45f, 1.5f); // negative radius => inv_radius 0 => never hit (rayweek1.cpp:291)
}

void build_medium(r1_host_scene &s, float aspect)
{
    s.camera_init({0, 2, 3}, {0, 0, 0}, {0, 1, 0}, 60, aspect, 0.1f * 0.2f, 3);
    s.lambertian({0, -100.5, -1}, 100, {0.8f, 0.8f, 0.8f});
    s.lambertian({2, 0, -1}, 0.5f, {0.8f, 0.4f, 0.4f});
    s.lambertian({0, 0, -1}, 0.5f, {0.4f, 0.8f, 0.4f});
    s.metal({-2, 0, -1}, 0.5f, {0.4f, 0.4f, 0.8f}, 0);
    s.metal({2, 0, 1}, 0.5f, {0.4f, 0.8f, 0.4f}, 0);
    s.metal({0, 0, 1}, 0.5f, {0.4f, 0.8f, 0.4f}, 0.2f);
    s.metal({-2, 0, 1}, 0.5f, {0.4f, 0.8f, 0.4f}, 0.6f);
    s.dielectric({0.5f, 1, 0.5f}, 0.5f, 1.5f);
    s.lambertian({-1.5f, 1.5f, 0.f}, 0.3f, {0.8f, 0.6f, 0.2f});
    // four rows of nine spheres at z = -3 .. -6, x = 4 .. -4 (rayweek1.cpp:607-642)
    static const float grey[9] = {0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f};
    static const V3 hue[9] = {{0.8f, 0.1f, 0.1f}, {0.8f, 0.5f, 0.1f}, {0.8f, 0.8f, 0.1f}, {0.4f, 0.8f, 0.1f}, {0.1f, 0.8f, 0.1f},
                              {0.1f, 0.8f, 0.5f}, {0.1f, 0.8f, 0.8f}, {0.1f, 0.1f, 0.8f}, {0.5f, 0.1f, 0.8f}};
    for (int i = 0; i < 9; ++i)
        s.lambertian({(float)(4 - i), 0, -3}, 0.5f, {grey[i], grey[i], grey[i]});
    for (int i = 0; i < 9; ++i)
        s.metal({(float)(4 - i), 0, -4}, 0.5f, {grey[i], grey[i], grey[i]}, 0);
    for (int i = 0; i < 9; ++i)
        s.metal({(float)(4 - i), 0, -5}, 0.5f, hue[i], 0);
    for (int i = 0; i < 8; ++i)
        s.lambertian({(float)(4 - i), 0, -6}, 0.5f, hue[i]);
    s.metal({-4, 0, -6}, 0.5f, hue[8], 0); // the last one of the z = -6 row is metal (rayweek1.cpp:642)
    s.lambertian({1.5f, 1.5f, -2}, 0.3f, {0.1f, 0.2f, 0.5f});
}

// create_large_scene generalised to a gw x gh grid of small spheres.  At gw = 30, gh = 16
// (scale == 1.0f exactly) every value equals the reference's (rayweek1.cpp:670-712).
// Larger grids (BASELINE config 5) shrink spacing, radius and the metal y-offset by 30/gw
// so that footprint and camera stay put; the dielectric index rule wraps at the
// reference's 480 spheres.  Albedos come from glibc rand() after srand(111), as in the
// reference (rayweek1.cpp:673, :682-684): same libc => same colours.
void build_grid(r1_host_scene &s, float aspect, int gw, int gh)
{
    s.camera_init({3, 8, 15}, {0, 0, 0}, {0, 1, 0}, 60, aspect, 0.1f, 10.0f);
    const float k = 30.0f / (float)gw;
    srand(111);
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x)
        {
            V3 pos = {(x - gw / 2) * 1.1f * k, 0, (y - gh / 2) * 1.1f * k};
            float r = (rand() & 0xff) / 255.0f;
            float g = (rand() & 0xff) / 255.0f;
            float b = (rand() & 0xff) / 255.0f;
            int i = x + y * gw;
            float radius = 0.45f * k;
            if (i % 20 == 0)
                s.dielectric(pos, radius, 1.2f + (i % 480) * 0.05f);
            else if (i % 10 == 0)
            {
                pos = add(pos, {0, 0.1f * k, 0});
                s.metal(pos, radius, {r, g, b}, 0.01f + 0.5f * y / (float)(gh));
            }
            else
                s.lambertian(pos, radius, {r, g, b});
        }
    s.lambertian({0, -1000.5f, 0}, 1000, {0.5f, 0.5f, 0.5f});
    s.metal({5, 3, 0}, 2, {0.5f, 0.5f, 0.8f}, 0.65f);
    s.dielectric({0, 3, 0}, 2, 1.5f);
    s.metal({-5, 3, 0}, 2, {0.8f, 0.2f, 0.2f}, 0.05f);
}

} // namespace

extern "C" int r1_host_scene_create(int kind, int32_t width, int32_t height, int32_t grid_w, int32_t grid_h, r1_host_scene **out)
{
    if (!out)
        return R1_EINVAL;
    *out = nullptr;
    if (width <= 0 || height <= 0 || kind < R1_SCENE_SMALL || kind > R1_SCENE_GRID)
    {
        r1_set_error("r1_host_scene_create: bad kind/size (%d, %dx%d)", kind, width, height);
        return R1_EINVAL;
    }
    r1_host_scene *s = new (std::nothrow) r1_host_scene();
    if (!s)
        return R1_ENOMEM;
    const float aspect = (float)width / (float)height; // rayweek1.cpp:564
    switch (kind)
    {
    case R1_SCENE_SMALL:
        build_small(*s, aspect);
        break;
    case R1_SCENE_MEDIUM:
        build_medium(*s, aspect);
        break;
    case R1_SCENE_LARGE:
        build_grid(*s, aspect, 30, 16);
        break;
    default:
        if (grid_w <= 0)
            grid_w = 30;
        if (grid_h <= 0)
            grid_h = 16;
        if ((int64_t)grid_w * grid_h > (1 << 21) - 16)
        {
            delete s;
            r1_set_error("r1_host_scene_create: grid %dx%d too large", grid_w, grid_h);
            return R1_ELIMIT;
        }
        build_grid(*s, aspect, grid_w, grid_h);
        break;
    }
    s->pad_to_simd_width();
    s->finish();
    *out = s;
    return R1_OK;
}

extern "C" void r1_host_scene_destroy(r1_host_scene *hs) { delete hs; }
extern "C" const r1_scene *r1_host_scene_spheres(const r1_host_scene *hs) { return hs ? &hs->view : nullptr; }
extern "C" const r1_camera *r1_host_scene_camera(const r1_host_scene *hs) { return hs ? &hs->cam : nullptr; }


extern "C" int r1_camera_look_at(const float lookfrom[3], const float lookat[3], const float vup[3], float vfov_degrees, float aspect, float aperture,
                                 float focus_dist, r1_camera *out)
{
    const char *bad = !lookfrom ? "lookfrom" : !lookat ? "lookat" : !vup ? "vup" : !out ? "out" : nullptr;
    if (bad)
    {
        r1_set_error("r1_camera_look_at: %s is NULL", bad);
        return R1_EINVAL;
    }
    look_at({lookfrom[0], lookfrom[1], lookfrom[2]}, {lookat[0], lookat[1], lookat[2]}, {vup[0], vup[1], vup[2]}, vfov_degrees, aspect, aperture, focus_dist, *out);
    return R1_OK;
}

extern "C" int r1_host_scene_view(const r1_host_scene *hs, float lookfrom[3], float lookat[3], float vup[3], float *vfov_degrees, float *aperture, float *focus_dist)
{
    const char *bad = !hs ? "scene" : !lookfrom ? "lookfrom" : !lookat ? "lookat" : !vup ? "vup" : !vfov_degrees ? "vfov_degrees" : !aperture ? "aperture" : !focus_dist ? "focus_dist" : nullptr;
    if (bad)
    {
        r1_set_error("r1_host_scene_view: %s is NULL", bad);
        return R1_EINVAL;
    }
    store(lookfrom, hs->view_from);
    store(lookat, hs->view_at);
    store(vup, hs->view_up);
    *vfov_degrees = hs->view_vfov, *aperture = hs->view_aperture, *focus_dist = hs->view_focus;
    return R1_OK;
}

// ---- tiles and shards -----------------------------------------------------------------

static int tiles_required(int tile, int size) // rayweek1.cpp:61-68
{
    int n = size / tile;
    if (n * tile < size)
        n++;
    return n;
}

extern "C" int r1_params_check(const r1_params *p)
{
    if (!p || p->width <= 0 || p->height <= 0 || p->spp <= 0 || p->tile_w <= 0 || p->tile_h <= 0 || p->num_shards < 1 ||
        p->shard < 0 || p->shard >= p->num_shards || p->max_bounces < 1 || p->max_bounces > R1_MAX_BOUNCES_LIMIT ||
        p->variant < R1_VARIANT_DEFAULT || p->variant > R1_VARIANT_GRID_STATS)
    {
        r1_set_error("bad r1_params (size %dx%dx%d, tile %dx%d, shard %d/%d, max_bounces %d, variant %d)", p ? p->width : 0,
                     p ? p->height : 0, p ? p->spp : 0, p ? p->tile_w : 0, p ? p->tile_h : 0, p ? p->shard : 0, p ? p->num_shards : 0,
                     p ? p->max_bounces : 0, p ? p->variant : 0);
        return R1_EINVAL;
    }
    if ((int64_t)p->width * p->height * p->spp >= (int64_t)1 << 31 || p->width > 65535 || p->height > 65535)
    {
        r1_set_error("image %dx%dx%d exceeds 2^31 samples", p->width, p->height, p->spp);
        return R1_ELIMIT;
    }
    return R1_OK;
}

extern "C" int r1_tile_count(const r1_params *p, int32_t *tiles_total, int32_t *tiles_per_shard)
{
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    int t = tiles_required(p->tile_w, p->width) * tiles_required(p->tile_h, p->height);
    if (tiles_total)
        *tiles_total = t;
    if (tiles_per_shard)
        *tiles_per_shard = (t + p->num_shards - 1) / p->num_shards;
    return R1_OK;
}

extern "C" size_t r1_shard_block_bytes(const r1_params *p)
{
    int32_t per = 0;
    if (r1_tile_count(p, nullptr, &per))
        return 0;
    return (size_t)per * p->tile_w * p->tile_h * 3;
}

// One shard's gather record: the dense tile block, padded to a multiple of 8 bytes, then the shard's uint64 ray
// count (8-byte aligned for any tile size: the kernels store it as one 64-bit word).
extern "C" size_t r1_shard_record_bytes(const r1_params *p)
{
    const size_t block = r1_shard_block_bytes(p);
    return block ? ((block + 7u) & ~(size_t)7u) + 8u : 0u;
}

// One whole frame as the batch entry points deliver it: the row-major image, padded to a multiple of 8 bytes, then the
// frame's uint64 ray count.
extern "C" size_t r1_frame_record_bytes(const r1_params *p)
{
    if (r1_params_check(p))
        return 0;
    return (((size_t)p->width * p->height * 3 + 7u) & ~(size_t)7u) + 8u;
}

// ---- output formats (src/common/common.h) ---------------------------------------------

extern "C" int r1_tga_write_rgb24(const char *filename, int32_t width, int32_t height, uint8_t *pixels)
{
    // common.h:86-122: 18-byte header, origin bits 0 (bottom-left), BGR payload; the
    // caller's buffer is left R/B-swapped, as in the reference.
    if (!filename || !pixels || width <= 0 || height <= 0)
        return R1_EINVAL;
    FILE *f = fopen(filename, "wb");
    if (!f)
        return R1_EINVAL;
    uint8_t header[18] = {0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, (uint8_t)(width & 0x00FF), (uint8_t)((width & 0xFF00) >> 8),
                          (uint8_t)(height & 0x00FF), (uint8_t)((height & 0xFF00) >> 8), 24, 0};
    for (int64_t i = 0; i < (int64_t)width * height; ++i)
    {
        uint8_t tmp = pixels[3 * i];
        pixels[3 * i] = pixels[3 * i + 2];
        pixels[3 * i + 2] = tmp;
    }
    fwrite(header, 1, sizeof(header), f);
    fwrite(pixels, 3, (size_t)width * height, f);
    fclose(f);
    return R1_OK;
}

extern "C" int r1_log_results(const char *version, const char *scene, const double *elapsed_seconds, const uint64_t *num_rays,
                              int32_t num_runs)
{
    // common.h:47-77: averages, then `version|%.3fs|%llu|%0.3f mrays/s|`
    if (!version || !scene || !elapsed_seconds || !num_rays || num_runs < 1 || strlen(scene) > 100)
        return R1_EINVAL;
    double el = 0;
    uint64_t rays = 0;
    for (int i = 0; i < num_runs; ++i)
    {
        el += elapsed_seconds[i];
        rays += num_rays[i];
    }
    el /= num_runs;
    rays /= (uint64_t)num_runs;
    char filename[128];
    snprintf(filename, sizeof(filename), "out_%s.txt", scene);
    FILE *f = fopen(filename, "wt");
    if (!f)
        return R1_EINVAL;
    fprintf(f, "%s|", version);
    fprintf(f, "%.3fs|", el);
    fprintf(f, "%llu|", (unsigned long long)rays);
    fprintf(f, "%0.3f mrays/s|", el ? (rays / el / 1000000.0) : 0); // RESULT::get_mrays_per_sec common.h:41-44
    fclose(f);
    return R1_OK;
}

// ---- ray queries on the host: r1_cast_rays_host -------------------------------------------------------------------------------
// Hitable::hit(Ray(o, d), 0.001f, t_max, &rec) (rayweek1.cpp:104-108, :152-339) for caller-supplied rays: every ray against every
// active sphere in index order, in the reference's arithmetic — its two FMA chains written with fmaf, everything else operation by
// operation (this file is compiled with -ffp-contract=off).  A sphere's offer is fixed before the compare with t_max (the comment
// above exact_offer in r1_trace.hpp derives it), so the result is the minimum offer, ties to the lowest index, accepted only if it
// is < t_max: the compare is strict, as rayweek1.cpp:298 / :307.

#include <float.h>

#include <functional>
#include <thread>

int r1_active_spheres(const r1_scene *s, std::vector<uint32_t> &active_to_scene); // inv_radius != 0, finite (r1_bvh.cpp)

namespace
{

inline bool finite_f(float v)
{
    uint32_t b;
    memcpy(&b, &v, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// what one sphere offers a ray (exact_offer of r1_trace.hpp, host_offer of r1_grid.cpp)
inline float cast_offer(const float *e, const float o[3], const float d[3])
{
    const float cox = e[0] - o[0], coy = e[1] - o[1], coz = e[2] - o[2];
    const float nb = fmaf(coz, d[2], fmaf(coy, d[1], cox * d[0]));
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

void cast_range(const std::vector<float> &ex, const std::vector<uint32_t> &scene_index, const r1_scene *s, int32_t mode, const r1_ray *rays,
                size_t i0, size_t i1, void *out)
{
    const size_t na = scene_index.size();
    for (size_t i = i0; i < i1; ++i)
    {
        const r1_ray &r = rays[i];
        const float scale = 1.0f / sqrtf((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]); // unit_vector, mymath.h:211
        const float d[3] = {r.d[0] * scale, r.d[1] * scale, r.d[2] * scale};
        float t_max = r.t_max;
        if (t_max > FLT_MAX) // +inf
            t_max = FLT_MAX;
        const bool valid = finite_f(r.o[0]) && finite_f(r.o[1]) && finite_f(r.o[2]) && finite_f(d[0]) && finite_f(d[1]) && finite_f(d[2]) &&
                           t_max > 0.001f; // (false for NaN)
        float best = FLT_MAX;
        size_t best_a = na;
        if (valid)
            for (size_t a = 0; a < na; ++a)
            {
                const float t = cast_offer(&ex[4 * a], r.o, d);
                if (t < best) // (ascending index: a tie keeps the earlier sphere)
                    best = t, best_a = a;
            }
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
            const float td[3] = {best * d[0], best * d[1], best * d[2]}; // point_at_parameter: _origin + t * _dir
            for (int q = 0; q < 3; ++q)
                h.p[q] = r.o[q] + td[q];
            h.n[0] = (h.p[0] - s->center_x[k]) * s->inv_radius[k];
            h.n[1] = (h.p[1] - s->center_y[k]) * s->inv_radius[k];
            h.n[2] = (h.p[2] - s->center_z[k]) * s->inv_radius[k];
        }
        ((r1_hit *)out)[i] = h;
    }
}

} // namespace

static_assert(sizeof(r1_ray) == 32 && sizeof(r1_hit) == 32, "the device reads and writes these layouts");

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
    if (r1_active_spheres(s, scene_index) != R1_OK)
        return R1_EINVAL;
    std::vector<float> ex(4 * scene_index.size() + 4);
    for (size_t a = 0; a < scene_index.size(); ++a)
    {
        const uint32_t i = scene_index[a];
        ex[4 * a + 0] = s->center_x[i], ex[4 * a + 1] = s->center_y[i], ex[4 * a + 2] = s->center_z[i], ex[4 * a + 3] = s->radius_sq[i];
    }
    // host threads: pieces of at least 256 rays, at most 16 threads (results do not depend on the split: rays are independent)
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = hw ? (hw > 16u ? 16u : hw) : 1u;
    if (nt > (n + 255) / 256)
        nt = (n + 255) / 256;
    if (nt <= 1)
    {
        cast_range(ex, scene_index, s, mode, rays, 0, n, out);
        return R1_OK;
    }
    std::vector<std::thread> pool;
    const size_t per = (n + nt - 1) / nt;
    for (size_t t = 0; t < nt; ++t)
    {
        const size_t i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
        if (i0 < i1)
            pool.emplace_back(cast_range, std::cref(ex), std::cref(scene_index), s, mode, rays, i0, i1, out);
    }
    for (std::thread &th : pool)
        th.join();
    return R1_OK;
}

// ---- path queries on the host: r1_camera_rays, r1_trace_rays_host ---------------------------------------------------
// color(Ray(o, d), scene, 0) (rayweek1.cpp:517-534) for caller-supplied rays and stream states: per level the hit test above (every
// active sphere in index order, cast_offer), then the level's scatter in scalar C++, operation by operation in the reference's order —
// what shade_level of r1_trace.hpp does on the device, with the same host-made material constants (r1_sweep.cpp).  The attenuations
// are applied innermost first once the path has reached the sky: a0 * (a1 * (... * sky)), rayweek1.cpp:525.

#include "../../include/rays1_seed.h"

namespace
{

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
};

void trace_range(const TraceScene &T, int32_t max_bounces, const r1_ray *rays, const r1_sample_seed *seeds, size_t i0, size_t i1, r1_radiance *out)
{
    const size_t na = T.type.size();
    std::vector<uint32_t> stack((size_t)max_bounces);
    for (size_t i = i0; i < i1; ++i)
    {
        const r1_ray &r = rays[i];
        V3 o = {r.o[0], r.o[1], r.o[2]};
        V3 d = unit({r.d[0], r.d[1], r.d[2]}); // Ray::Ray, rayweek1.cpp:107
        r1_radiance rec = {0.0f, 0.0f, 0.0f, 0u};
        if (!(finite_f(o.x) && finite_f(o.y) && finite_f(o.z) && finite_f(d.x) && finite_f(d.y) && finite_f(d.z)))
        {
            out[i] = rec; // no color()
            continue;
        }
        const r1_sample_seed sd = r1_seed_guard(seeds ? seeds[i] : r1_seed_sample(0u, (uint32_t)i, 0u));
        uint32_t s_scalar = sd.scalar, s0 = sd.lane0, s1 = sd.lane1, s2 = sd.lane2;
        int depth = 0, sp = 0;
        V3 col = {0, 0, 0};
        for (;;)
        {
            // Hitable::hit(r, 0.001f, FLT_MAX, rec), rayweek1.cpp:519
            float best = FLT_MAX;
            size_t hit = na;
            const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
            for (size_t a = 0; a < na; ++a)
            {
                const float t = cast_offer(&T.ex[4 * a], of, df);
                if (t < best) // (ascending index: a tie keeps the earlier sphere)
                    best = t, hit = a;
            }
            if (hit == na)
            {
                // sky (rayweek1.cpp:532-534), lerp = (1 - t) * a + t * b (mymath.h:212-216)
                const float t = 0.5f * (d.y + 1.0f);
                const float omt = 1.0f - t;
                col = {omt * 1.0f + t * 0.5f, omt * 1.0f + t * 0.7f, omt * 1.0f + t * 1.0f};
                for (int e = sp - 1; e >= 0; --e)
                {
                    const float *sh = &T.shade[4 * (size_t)stack[e]];
                    col = {sh[1] * col.x, sh[2] * col.y, sh[3] * col.z};
                }
                break;
            }
            if (depth >= max_bounces)
                break; // depth == MAX_BOUNCES: black (rayweek1.cpp:523-528)
            // hit record (rayweek1.cpp:316-322)
            const float *e = &T.ex[4 * hit], *sh = &T.shade[4 * hit], *mt = &T.mat[3 * hit];
            const V3 hp = add(o, scale(d, best));
            const V3 n = scale(sub(hp, {e[0], e[1], e[2]}), sh[0]);
            const uint8_t type = T.type[hit];
            V3 rius = {0, 0, 0};
            if (type != R1_MAT_DIELECTRIC) // random_in_unit_sphere, mymath.h:224-235 (Lambertian and Metal both draw it, rayweek1.cpp:405, :430)
                do
                {
                    rius = {rand02_minus1(s0), rand02_minus1(s1), rand02_minus1(s2)};
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
                    // schlick rayweek1.cpp:454-459, x^5 exactly rounded (pow5 of r1_trace.hpp)
                    const float r0 = mt[2];
                    const double x = (double)(1.0f - cosine), x2 = x * x;
                    reflect_prob = r0 + (1.0f - r0) * (float)(x2 * x2 * x);
                }
                dir = (rand01(s_scalar) < reflect_prob) ? reflected : refracted;
            }
            const V3 nd = unit(dir);
            o = hp, d = nd;
            if (type == R1_MAT_DIELECTRIC || type == R1_MAT_LAMBERTIAN || dot(nd, n) > 0)
            {
                if (type != R1_MAT_DIELECTRIC)
                    stack[sp++] = (uint32_t)hit;
            }
            else
                break; // Metal::scatter() == false: black (rayweek1.cpp:432, :528)
            ++depth;
        }
        rec.r = col.x, rec.g = col.y, rec.b = col.z, rec.rays = (uint32_t)depth + 1u; // every level counts one ray (rayweek1.cpp:517)
        out[i] = rec;
    }
}

} // namespace

static_assert(sizeof(r1_radiance) == 16 && sizeof(r1_sample_seed) == 16, "the device reads and writes these layouts");

extern "C" int r1_trace_rays_host(const r1_scene *s, int32_t max_bounces, const r1_ray *rays, const r1_sample_seed *seeds, size_t n, r1_radiance *out)
{
    if (max_bounces < 1 || max_bounces > R1_MAX_BOUNCES_LIMIT)
    {
        r1_set_error("r1_trace_rays_host: max_bounces %d is not in 1..%d", max_bounces, R1_MAX_BOUNCES_LIMIT);
        return R1_EINVAL;
    }
    if (!s || (s->count && (!s->center_x || !s->center_y || !s->center_z || !s->radius_sq || !s->inv_radius || !s->mat_type || !s->albedo_r ||
                            !s->albedo_g || !s->albedo_b || !s->mat_param)))
    {
        r1_set_error("r1_trace_rays_host: null scene");
        return R1_EINVAL;
    }
    if (n == 0)
        return R1_OK;
    if (!rays || !out)
    {
        r1_set_error("r1_trace_rays_host: null rays or out with n > 0");
        return R1_EINVAL;
    }
    std::vector<uint32_t> scene_index;
    if (r1_active_spheres(s, scene_index) != R1_OK)
        return R1_EINVAL;
    const size_t na = scene_index.size();
    TraceScene T;
    T.ex.resize(4 * na + 4), T.shade.resize(4 * na + 4), T.mat.resize(3 * na + 3), T.type.resize(na);
    for (size_t a = 0; a < na; ++a)
    {
        const uint32_t i = scene_index[a];
        if (s->mat_type[i] > R1_MAT_DIELECTRIC)
        {
            r1_set_error("r1_trace_rays_host: sphere %u is hittable but has no material", i);
            return R1_EINVAL;
        }
        T.ex[4 * a + 0] = s->center_x[i], T.ex[4 * a + 1] = s->center_y[i], T.ex[4 * a + 2] = s->center_z[i], T.ex[4 * a + 3] = s->radius_sq[i];
        T.shade[4 * a + 0] = s->inv_radius[i], T.shade[4 * a + 1] = s->albedo_r[i], T.shade[4 * a + 2] = s->albedo_g[i], T.shade[4 * a + 3] = s->albedo_b[i];
        // the dielectric's constants as the device tables hold them (r1_sweep.cpp; rayweek1.cpp:489, :456-457): same IEEE operations, done once
        const float ref_idx = s->mat_param[i];
        float r0 = (1 - ref_idx) / (1 + ref_idx);
        r0 = r0 * r0;
        T.mat[3 * a + 0] = ref_idx, T.mat[3 * a + 1] = 1.0f / ref_idx, T.mat[3 * a + 2] = r0;
        T.type[a] = s->mat_type[i];
    }
    // host threads, as r1_cast_rays_host: pieces of at least 256 rays, at most 16 threads (rays are independent)
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = hw ? (hw > 16u ? 16u : hw) : 1u;
    if (nt > (n + 255) / 256)
        nt = (n + 255) / 256;
    if (nt <= 1)
    {
        trace_range(T, max_bounces, rays, seeds, 0, n, out);
        return R1_OK;
    }
    std::vector<std::thread> pool;
    const size_t per = (n + nt - 1) / nt;
    for (size_t t = 0; t < nt; ++t)
    {
        const size_t i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
        if (i0 < i1)
            pool.emplace_back(trace_range, std::cref(T), max_bounces, rays, seeds, i0, i1, out);
    }
    for (std::thread &th : pool)
        th.join();
    return R1_OK;
}

// rayweek1.cpp:757-760 under the seeding contract — start_ray of r1_trace.hpp on the host, without the Ray constructor's normalisation
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
