// r1_sample.hpp — where a path starts and where its radiance goes: a wave's claim on an array of rays (chunk_claim), sample slot -> seeds and
// primary ray (start_ray, start_sample), the pixels of PIXEL mode, quantisation, and the wavefront variant's path state in memory.
// Internal linkage (anonymous namespace).
#ifndef R1_SAMPLE_HPP
#define R1_SAMPLE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "r1_device.h"
#include "r1_dev_math.hpp"
#include "../../include/rays1_seed.h"

#pragma clang fp contract(off)

namespace
{

// Ray and path queries (r1_query_kernels.hip): a wave's next chunk of an array of n rays, `claim` at a time from the launch's one cursor;
// false: none left.  Called by all 64 lanes, wave-uniform result.
__device__ __forceinline__ bool chunk_claim(uint32_t *cursor, const uint32_t claim, const uint32_t n, const int lane, uint32_t &q_next, uint32_t &q_end)
{
    uint32_t base = 0;
    if (lane == 0)
        base = atomicAdd(cursor, claim);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (base >= n)
        return false;
    q_next = base, q_end = min(base + claim, n);
    return true;
}

__device__ __forceinline__ uint32_t fastdiv(uint32_t n, const R1FastDiv dv)
{
    return dv.pow2 ? (n >> dv.shift) : (__umulhi(n, dv.mul) >> dv.shift);
}

// seeds + primary ray of sample s of pixel (x, y) (rayweek1.cpp:759-760) up to the Ray constructor: the origin in p.o, the stream states
// after the camera's draws in p, and the direction as getRay hands it to the constructor — UN-normalised — returned.  start_ray, and
// r1_camera_rays_kernel (r1_aux_kernels.hip), which stores exactly this.
// camera_ray_at: the same for a caller that has the pixel's index in the frame, `pixel` = y * width + x (a region's lanes, start_sample)
__device__ __forceinline__ V3 camera_ray_at(const uint32_t pixel, const float inv_w, const float inv_h, const R1DeviceCamera &C, Path &p, const int x, const int y,
                                            const uint32_t s, const uint32_t seed)
{
    const r1_sample_seed sd = r1_seed_sample(seed, pixel, s);
    p.s_scalar = sd.scalar;
    p.s0 = sd.lane0;
    p.s1 = sd.lane1;
    p.s2 = sd.lane2;
    p.depth = 0;
    p.sp = 0;

    // uv = (myrand01_x4(state4) + (x, y)) * (1/W, 1/H): lanes 0,1 used, lane 2 advances too
    const float j0 = rand01(p.s0), j1 = rand01(p.s1);
    (void)xorshift32(p.s2);
    const float u = (j0 + (float)x) * inv_w;
    const float v = (j1 + (float)y) * inv_h;

    // random_in_unit_disk (rayweek1.cpp:353-362): g++ argument order => y gets the first draw
    V3 dk;
    do
    {
        const float first = rand02_minus1(p.s_scalar);
        const float second = rand02_minus1(p.s_scalar);
        dk = mk(second, first, 0.0f); // 2 * Vec3(rand, rand, 0) - Vec3(1, 1, 0): z = 0 - 0
    } while (vdot(dk, dk) >= 1.0f);

    // Camera::getRay (rayweek1.cpp:381-386)
    const V3 rd = vscale(dk, C.lens_radius);
    const V3 offset = vadd(vscale(ld3(C.u), rd.x), vscale(ld3(C.v), rd.y));
    const V3 org = ld3(C.origin);
    p.o = vadd(org, offset);
    return vsub(vsub(vadd(vadd(ld3(C.lower_left), vscale(ld3(C.horizontal), u)), vscale(ld3(C.vertical), v)), org), offset);
}
__device__ __forceinline__ V3 camera_ray(const int width, const float inv_w, const float inv_h, const R1DeviceCamera &C, Path &p, const int x, const int y,
                                         const uint32_t s, const uint32_t seed)
{
    return camera_ray_at((uint32_t)(y * width + x), inv_w, inv_h, C, p, x, y, s, seed);
}

// the same with the constructor's normalisation: the primary ray in p
// C: the camera — the launch's own (A.cam), or the frame's of a camera path (start_sample)
__device__ __forceinline__ void start_ray(const R1TraceArgs &A, const R1DeviceCamera &C, Path &p, const int x, const int y, const uint32_t s, const uint32_t seed)
{
    p.d = vunit(camera_ray(A.width, A.inv_w, A.inv_h, C, p, x, y, s, seed));
}

// (local tile j, pixel `pix` of the padded tile) -> image coordinates; false outside the image (edge tiles)
__device__ __forceinline__ bool tile_pixel(const R1TraceArgs &A, const uint32_t j, const uint32_t pix, int &x, int &y)
{
    const uint32_t ly = fastdiv(pix, A.div_tw);
    const uint32_t lx = pix - ly * (uint32_t)A.tile_w;
    const uint32_t tile = (uint32_t)A.shard + j * (uint32_t)A.num_shards;
    const uint32_t ty = fastdiv(tile, A.div_tx);
    const uint32_t tx = tile - ty * (uint32_t)A.tiles_x;
    x = (int)(tx * (uint32_t)A.tile_w + lx);
    y = (int)(ty * (uint32_t)A.tile_h + ly);
    return x < A.width && y < A.height;
}

// sample slot k -> (tile, pixel, sample); then seeds + primary ray.
// Returns false for a void slot (pixel of an edge tile that lies outside the image).
// PASS (progressive passes, R1_MODE_PASS): s is the pass-local sample index — the record's place — and the sample is seeded with its global
// index s + first_sample, which the pass's R1PassArgs hold behind A.batch.
// PATH (camera paths, R1_MODE_PATH): a batch whose frame f is seen through camera f of the table behind the batch's numbers (R1PathArgs).  The
// queue is frame-major and a wave's chunk may straddle frames, so f is a per-lane value and every lane loads its frame's camera itself:
// five vector loads where start_ray needs them, dead before the walk — the builds keep the VGPR count of their R1_MODE_BATCH siblings
// (tools/kernel_meta.py).  The other form — a loop over the wave's distinct f, the camera through scalar loads, the lanes of that frame
// masked in — is not kept: hipcc proves `frame == f0` inside the masked arm, addresses the camera by the lane's own f again and hoists
// start_ray out of the loop, i.e. emits these very loads behind a loop that only builds the address.
// LIST (adaptive sampling, R1_MODE_LISTED): a PASS whose local tile j is tile list[j] of the frame (R1PassArgs::list); the record keeps the list
// position.  j is a per-lane value (a wave's chunk may straddle tiles), so every lane loads its own entry, as a camera path's lanes do.
// REGION (region renders, r1_region_kernel): a PASS whose arguments describe a frame of the REGION's size, cut into tiles from
// the region's own corner — the bound test, the record's place and everything behind them see that frame — and whose lanes, once the bound
// test is over, move the pixel by the region's corner (x0, y0) and seed and aim the sample with the WHOLE frame's width, 1/W and 1/H: A.inv_w
// and A.inv_h are the frame's, and x0, y0 and the frame's width are the three words of R1PassArgs behind first_sample (which is 0), read by
// scalar loads where that one is.  The pixel's index in the frame is a uint32 (width * height < 2^31, r1_region_check).
template <bool BATCH = false, bool PASS = false, bool PATH = false, bool LIST = false, bool REGION = false>
__device__ __forceinline__ bool start_sample(const R1TraceArgs &A, Path &p, uint32_t k)
{
    static_assert(!PATH || BATCH, "a camera path is a batch");
    static_assert(!LIST || (PASS && !BATCH), "a listed pass is a pass");
    static_assert(!REGION || (PASS && !BATCH && !LIST), "a region is a pass over tiles of its own");
    const uint32_t j = fastdiv(k, A.div_full); // padded tile, frame-major over the frames of the launch
    const uint32_t r = k - j * A.full;
    const uint32_t pix = fastdiv(r, A.div_spp);
    const uint32_t s = r - pix * (uint32_t)A.spp;
    uint32_t jl = j, seed = A.seed, frame = 0;
    if (BATCH) // (its own build of the kernel, R1_MODE_BATCH: the single-frame kernels stay as they were, to the register)
    {
        typedef const uint32_t __attribute__((address_space(4))) *cu32_ptr;
        const cu32_ptr b = (cu32_ptr)A.batch; // {n_frames, seed_stride, div_tiles{mul, shift, pow2}, n_local_tiles}
        R1FastDiv dv;
        dv.mul = b[2], dv.shift = b[3], dv.pow2 = b[4];
        const uint32_t f = fastdiv(j, dv);
        jl = j - f * b[5];
        seed += f * b[1];
        frame = f;
    }
    if (LIST)
    {
        typedef const uint32_t __attribute__((address_space(1))) *gu32_ptr;
        const gu32_ptr list = *(const __attribute__((address_space(4))) gu32_ptr *)((const __attribute__((address_space(4))) char *)A.batch + __builtin_offsetof(R1PassArgs, list));
        jl = list[j];
    }
    int x, y;
    if (!tile_pixel(A, jl, pix, x, y))
        return false;
    // output slot: samples are stored [tile][sample][pixel] so that the resolve pass reads
    // coalesced (consecutive pixels of one sample index)
    p.k = (j * (uint32_t)A.spp + s) * (uint32_t)(A.tile_w * A.tile_h) + pix;
    uint32_t s_global = s;
    if (PASS)
    {
        typedef const uint32_t __attribute__((address_space(4))) *cu32_ptr;
        s_global += ((cu32_ptr)A.batch)[0]; // R1PassArgs::first_sample
    }
    if (PATH)
    {
        // R1PathArgs::cameras: [n_frames] cameras of R1_PATH_CAM_F4 float4 each, in R1DeviceCamera's order
        typedef const f4 __attribute__((address_space(1))) *gf4_ptr;
        const gf4_ptr tab = *(const __attribute__((address_space(4))) gf4_ptr *)((const __attribute__((address_space(4))) char *)A.batch + __builtin_offsetof(R1PathArgs, cameras));
        const gf4_ptr t = tab + (size_t)frame * R1_PATH_CAM_F4;
        typedef float f3 __attribute__((ext_vector_type(3)));
        typedef const f3 __attribute__((address_space(1))) *gf3_ptr;
        const f4 c0 = t[0], c1 = t[1], c2 = t[2], c3 = t[3];
        const f3 c4 = *(gf3_ptr)(t + 4); // (the row's 20th word is padding: a loaded register nobody reads is the first one hipcc reuses, and it waits for all five loads to do so)
        const R1DeviceCamera C = {{c0.x, c0.y, c0.z}, {c0.w, c1.x, c1.y}, {c1.z, c1.w, c2.x}, {c2.y, c2.z, c2.w}, {c3.x, c3.y, c3.z}, {c3.w, c4.x, c4.y}, c4.z};
        start_ray(A, C, p, x, y, s_global, seed);
        return true;
    }
    if (REGION)
    {
        typedef const uint32_t __attribute__((address_space(4))) *cu32_ptr;
        const cu32_ptr b = (cu32_ptr)A.batch;
        static_assert(__builtin_offsetof(R1PassArgs, x0) == 4 && __builtin_offsetof(R1PassArgs, y0) == 16 && __builtin_offsetof(R1PassArgs, frame_w) == 20, "the words read here");
        const uint32_t fx = (uint32_t)x + b[1], fy = (uint32_t)y + b[4]; // the pixel in the frame
        p.d = vunit(camera_ray_at(fy * b[5] + fx, A.inv_w, A.inv_h, A.cam, p, (int)fx, (int)fy, s_global, seed));
        return true;
    }
    start_ray(A, A.cam, p, x, y, s_global, seed);
    return true;
}

// rayweek1.cpp:765-775: col *= 1 / spp; sqrtf per channel; (uint8)(int)(c * 255.99f) — the resolve launch and the progressive passes'
// accumulate launch (inv = (float)(1.0f / samples summed))
__device__ __forceinline__ void quantise_pixel(float cr, float cg, float cb, const float inv, uint8_t &r, uint8_t &g, uint8_t &b)
{
    cr *= inv, cg *= inv, cb *= inv;
    cr = ieee_sqrt(cr), cg = ieee_sqrt(cg), cb = ieee_sqrt(cb);
    r = (uint8_t)(int)(cr * 255.99f);
    g = (uint8_t)(int)(cg * 255.99f);
    b = (uint8_t)(int)(cb * 255.99f);
}

// PIXEL mode (frames in flight): a lane owns a PIXEL and runs its spp samples one after the other, so
// `col += color(...)` (rayweek1.cpp:762) happens in a register in the reference's order and the resolved
// pixel (rayweek1.cpp:765-775) is the only thing the frame writes: no per-sample records, no second kernel.
struct Pixel
{
    V3 acc;       // col of render_tile
    uint32_t xy;  // x | y << 16
    uint32_t off; // output pixel index (dense tile block: the queue slot itself; row-major image: y * width + x)
    uint32_t s;   // next sample; == spp: no pixel in hand
};

// pixel slot kp of the frame's queue = (local tile, pixel of the padded tile) -> Pixel; false for a void slot
__device__ __forceinline__ bool pixel_take(const R1TraceArgs &A, Pixel &px, const uint32_t kp)
{
    const uint32_t j = fastdiv(kp, A.div_full); // PIXEL mode: `full` = tile_w * tile_h
    int x, y;
    if (!tile_pixel(A, j, kp - j * A.full, x, y))
        return false;
    px.acc = mk(0, 0, 0);
    px.xy = (uint32_t)x | ((uint32_t)y << 16);
    px.off = A.block_layout ? kp : (uint32_t)(y * A.width + x);
    px.s = 0;
    return true;
}

// rayweek1.cpp:765-775: col *= 1 / spp; sqrtf per channel; (uint8)(int)(c * 255.99f)
__device__ __forceinline__ void pixel_write(const R1TraceArgs &A, const Pixel &px)
{
    uint8_t *o = (uint8_t *)A.samples + 3 * (size_t)px.off; // PIXEL mode: `samples` is the output image / tile block
    o[0] = (uint8_t)(int)(ieee_sqrt(px.acc.x * A.inv_spp) * 255.99f);
    o[1] = (uint8_t)(int)(ieee_sqrt(px.acc.y * A.inv_spp) * 255.99f);
    o[2] = (uint8_t)(int)(ieee_sqrt(px.acc.z * A.inv_spp) * 255.99f);
}

// Path state in memory, [3][n] float4: {ox oy oz dx} {dy dz s_scalar s0} {s1 s2 k rays|depth<<8|sp<<16}
// (0xFFFFFFFF in the last word marks a void sample slot).  Used by the wavefront variant.
#define R1_PATH_VOID 0xFFFFFFFFu
__device__ __forceinline__ void path_store(float4 *paths, const uint32_t n, const uint32_t slot, const Path &p)
{
    paths[slot] = make_float4(p.o.x, p.o.y, p.o.z, p.d.x);
    paths[(size_t)n + slot] = make_float4(p.d.y, p.d.z, __uint_as_float(p.s_scalar), __uint_as_float(p.s0));
    paths[2 * (size_t)n + slot] = make_float4(__uint_as_float(p.s1), __uint_as_float(p.s2), __uint_as_float(p.k),
                                              __uint_as_float(((uint32_t)p.depth << 8) | ((uint32_t)p.sp << 16)));
}

// returns false for a void slot
__device__ __forceinline__ bool path_load(const float4 *paths, const uint32_t n, const uint32_t slot, Path &p)
{
    const float4 a = paths[slot], b = paths[(size_t)n + slot], c = paths[2 * (size_t)n + slot];
    p.o = mk(a.x, a.y, a.z);
    p.d = mk(a.w, b.x, b.y);
    p.s_scalar = __float_as_uint(b.z), p.s0 = __float_as_uint(b.w);
    p.s1 = __float_as_uint(c.x), p.s2 = __float_as_uint(c.y);
    p.k = __float_as_uint(c.z);
    const uint32_t packed = __float_as_uint(c.w);
    p.depth = (int)((packed >> 8) & 255u), p.sp = (int)((packed >> 16) & 255u);
    return packed != R1_PATH_VOID;
}

} // namespace

#endif // R1_SAMPLE_HPP
