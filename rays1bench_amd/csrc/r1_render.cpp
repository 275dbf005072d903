// r1_render.cpp — the entry points that render: synchronous frames, progressive passes, adaptive sampling, linear frames, frames in flight, batches and
// camera paths, shards and their assembly.  Each checks its arguments, calls enqueue_frame (r1_frame.cpp) and brings the results home.

#include <string.h>

#include <algorithm>
#include <vector>

#include "r1_context.h"

// ---- public render entry points ---------------------------------------------------------------------

// device address of page-locked host memory (r1_host_alloc, hipHostMalloc, hipHostRegister), or null for anything else
static void *mapped_host(const void *ptr)
{
    if (!ptr)
        return nullptr;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess)
    {
        (void)hipGetLastError(); // ordinary (pageable) memory is not an error here
        return nullptr;
    }
    return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
}

// the frame's tile geometry (r1_tile.h), of params that r1_params_check has passed
static R1TileGeom geom_of(const r1_params *p) { return r1_tile_geom(p->width, p->height, p->tile_w, p->tile_h); }

// The ray count of a frame the caller waits for.  direct: the frame's last launch stores it straight into the context's page-locked word
// (8 bytes over PCIe, no second copy to enqueue and wait for); else it is copied from behind the counter block.  rays_word: what
// enqueue_frame is given.  read_rays: after the frame and the caller's own copies are enqueued — waits for the context's stream.
static void *rays_word(const r1_context *c, bool direct) { return direct ? (void *)&c->host_word_dev->rays : nullptr; }
static int read_rays(r1_context *c, bool direct, uint64_t *rays)
{
    if (!direct) // (behind the block the frame's last launch zeroes)
        R1_HIP(hipMemcpyAsync(rays, counter_at(c, R1_TAIL_RAYS), 8, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    if (direct)
        *rays = *(volatile unsigned long long *)&c->host_word->rays;
    return R1_OK;
}

// The records the last launch left (whole frames, num_shards == 1: local tile = tile of g's frame), brought home in the ABI's order: device order
// is [padded tile][sample][pixel in tile], the ABI's ((y * width + x) * spp + s) over g's frame — the params' frame, or a region's own.
// Waits for the context's stream.
static int gather_records(r1_context *c, const R1TileGeom &g, const int32_t spp, float *samples_out)
{
    std::vector<float> tmp((size_t)c->total_samples * 4);
    R1_HIP(hipMemcpyAsync(tmp.data(), c->samples.p, tmp.size() * 4, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t lt = 0; lt < c->n_local_tiles; ++lt)
    {
        const R1TileRect r = r1_tile_rect(g, lt);
        const float *src = tmp.data() + (size_t)lt * c->full * 4;
        const size_t tile_px = r1_tile_slots(g);
        for (int ly = 0; ly < r.th; ++ly)
            for (int lx = 0; lx < r.tw; ++lx)
                for (int sm = 0; sm < spp; ++sm)
                {
                    float *dst = samples_out + (r1_pixel_row_major(g, r, lx, ly) * spp + sm) * 4;
                    memcpy(dst, src + ((size_t)sm * tile_px + (size_t)(ly * g.tile_w + lx)) * 4, 16);
                    if (c->land_prev) // the launch tagged its records' ray-count words (R1_LAND): the ABI's word is the count alone
                    {
                        uint32_t wv;
                        memcpy(&wv, dst + 3, 4);
                        wv &= 255u;
                        memcpy(dst + 3, &wv, 4);
                    }
                }
    }
    return R1_OK;
}

static int render_host(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, double *device_seconds_out,
                       float *samples_out)
{
    if (!c || !p || !rgb_out)
    {
        r1_set_error("r1_render: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (samples_out && p->num_shards != 1)
    {
        r1_set_error("r1_render_samples needs num_shards == 1");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const bool sharded = p->num_shards > 1;
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    const size_t out_bytes = sharded ? r1_shard_block_bytes(p) : img_bytes;
    if ((rc = ensure(c->image, out_bytes + 64)))
        return rc;
    // (the diagnostic builds count with atomics and keep a device word + copy)
    const bool stats = r1_is_stats(p->variant);
    const bool direct = !stats && c->host_word_dev;
    // a page-locked pixel buffer (r1_host_alloc) receives the tiles straight from the trace kernel's resolvers: no copy either
    Landing land_to;
    if (direct && !sharded)
        land_to.out = mapped_host(rgb_out), land_to.rays = &c->host_word_dev->rays;
    FrameJob job;
    job.out = c->image.p, job.block_layout = sharded ? 1 : 0, job.rays = rays_word(c, direct), job.st = c->stream, job.landing = &land_to;
    if ((rc = enqueue_frame(c, p, job)))
        return rc;

    const R1TileGeom g = geom_of(p);
    uint64_t rays = 0;
    if (!sharded)
    {
        if (!land_to.used)
            R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
        if ((rc = read_rays(c, direct, &rays)))
            return rc;
    }
    else
    {
        std::vector<uint8_t> block(out_bytes);
        R1_HIP(hipMemcpyAsync(block.data(), c->image.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
        if ((rc = read_rays(c, direct, &rays)))
            return rc;
        for (uint32_t lt = 0; lt < c->n_local_tiles; ++lt)
        {
            const R1TileRect r = r1_tile_rect(g, r1_shard_tile(p->shard, lt, p->num_shards));
            for (int ly = 0; ly < r.th; ++ly) // a row of the tile at a time
                memcpy(rgb_out + r1_pixel_row_major(g, r, 0, ly) * 3, block.data() + r1_pixel_block(g, lt, 0, ly) * 3, (size_t)r.tw * 3);
        }
    }
    if ((rc = land_check(c)))
        return rc;
    if (num_rays_out)
        *num_rays_out = rays;
    if (device_seconds_out)
    {
        float ms = 0;
        R1_HIP(hipEventElapsedTime(&ms, c->last0, c->last2)); // the events THIS frame recorded (a ring slot while r1_timing_begin is on)
        *device_seconds_out = ms * 1e-3;
    }
    if (samples_out)
        return gather_records(c, g, p->spp, samples_out);
    return R1_OK;
}

extern "C" int r1_render(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    return render_host(c, p, rgb_out, num_rays_out, device_seconds_out, nullptr);
}

extern "C" int r1_render_samples(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, float *samples_out)
{
    if (!samples_out)
    {
        r1_set_error("r1_render_samples: null samples_out");
        return R1_EINVAL;
    }
    return render_host(c, p, rgb_out, num_rays_out, nullptr, samples_out);
}

// Progressive rendering: samples [first_sample, first_sample + spp) of every pixel, added in sample order to the context's fp32 accumulator.  The
// accumulator then holds exactly the sums the resolve of a frame of first_sample + spp samples computes (a sample's streams depend on (seed,
// pixel, sample index) only, include/rays1_seed.h), so every preview is that frame's image, bit for bit.
static bool same_pass_frame(const r1_params &a, const r1_params &b) // every field but spp
{
    return a.width == b.width && a.height == b.height && a.max_bounces == b.max_bounces && a.seed == b.seed && a.tile_w == b.tile_w &&
           a.tile_h == b.tile_h && a.shard == b.shard && a.num_shards == b.num_shards && a.variant == b.variant;
}

extern "C" int r1_render_pass(r1_context *c, const r1_params *p, int32_t first_sample, uint8_t *rgb_out, uint64_t *num_rays_out)
{
    if (!c || !p)
    {
        r1_set_error("r1_render_pass: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_pass renders whole frames (num_shards == 1)");
        return R1_EINVAL;
    }
    if (r1_is_stats(p->variant) || p->variant == R1_VARIANT_WAVEFRONT)
    {
        r1_set_error("r1_render_pass: variant %d (a diagnostic build or the wavefront variant) has no progressive-pass build", p->variant);
        return R1_EINVAL;
    }
    if (first_sample < 0 || (int64_t)first_sample + p->spp > (int64_t)INT32_MAX)
    {
        r1_set_error("r1_render_pass: first_sample %d + spp %d is not within [0, INT32_MAX]", first_sample, p->spp);
        return R1_EINVAL;
    }
    if (first_sample > 0 && !(c->pass_valid && c->pass_samples == first_sample && same_pass_frame(c->pass_key, *p)))
    {
        if (!c->pass_valid)
            r1_set_error("r1_render_pass: no accumulation to continue (start one with first_sample 0)");
        else if (c->pass_samples != first_sample)
            r1_set_error("r1_render_pass: first_sample %d, but %d samples are accumulated", first_sample, c->pass_samples);
        else
            r1_set_error("r1_render_pass: the parameters differ from those that started the accumulation (only spp may change)");
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    int32_t tiles = 0;
    if ((rc = r1_tile_count(p, &tiles, nullptr)))
        return rc;
    if ((uint64_t)p->tile_w * p->tile_h * p->spp * (uint64_t)tiles >= ((uint64_t)1 << 31))
    {
        r1_set_error("a pass of %dx%dx%d with %dx%d tiles exceeds 2^31 sample slots per launch", p->width, p->height, p->spp, p->tile_w, p->tile_h);
        return R1_ELIMIT;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    if (rgb_out && (rc = ensure(c->image, img_bytes + 64)))
        return rc;
    // from here on a failure leaves the accumulator in an unknown state: only first_sample == 0 is accepted next
    c->pass_valid = false;
    const bool direct = c->host_word_dev != nullptr; // the pass's ray count straight into the page-locked word, as r1_render
    Pass ps;
    ps.first_sample = first_sample;
    ps.image = rgb_out != nullptr;
    FrameJob job;
    job.out = c->image.p, job.rays = rays_word(c, direct), job.st = c->stream, job.pass = &ps;
    if ((rc = enqueue_frame(c, p, job)))
        return rc;
    uint64_t rays = 0;
    if (rgb_out)
        R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_rays(c, direct, &rays)))
        return rc;
    c->pass_rays = (first_sample == 0 ? 0u : c->pass_rays) + rays;
    c->pass_samples = first_sample + p->spp;
    c->pass_key = *p;
    c->pass_valid = true;
    if (num_rays_out)
        *num_rays_out = c->pass_rays;
    return R1_OK;
}

// ---- adaptive sampling --------------------------------------------------------------
static bool adaptive_variant(int v) { return v == R1_VARIANT_DEFAULT || v == R1_VARIANT_PREFILTER || v == R1_VARIANT_BVH || v == R1_VARIANT_GRID; }

// The one place the options of r1_render_adaptive are validated: the cumulative sample counts after every pass.
extern "C" int r1_adaptive_schedule(const r1_params *p, const r1_adaptive *o, int32_t *n_out, size_t cap, size_t *count)
{
    if (!p || !o || (!n_out && !count))
    {
        r1_set_error("r1_adaptive_schedule: null argument");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("adaptive sampling renders whole frames (num_shards == 1, not %d)", p->num_shards);
        return R1_EINVAL;
    }
    if (!adaptive_variant(p->variant))
    {
        r1_set_error("adaptive sampling: variant %d (the reference form, a diagnostic build or the wavefront variant) has no listed-tile build", p->variant);
        return R1_EINVAL;
    }
    if (o->min_spp < 1)
    {
        r1_set_error("adaptive sampling: min_spp %d is not >= 1", o->min_spp);
        return R1_EINVAL;
    }
    if (o->pass_spp < 1)
    {
        r1_set_error("adaptive sampling: pass_spp %d is not >= 1", o->pass_spp);
        return R1_EINVAL;
    }
    if (o->max_delta < -1 || o->max_delta > 255)
    {
        r1_set_error("adaptive sampling: max_delta %d is not within [-1, 255]", o->max_delta);
        return R1_EINVAL;
    }
    if (o->mean_delta_q8 < 0 || o->mean_delta_q8 > 65280)
    {
        r1_set_error("adaptive sampling: mean_delta_q8 %d is not within [0, 65280]", o->mean_delta_q8);
        return R1_EINVAL;
    }
    int32_t tiles = 0;
    if ((rc = r1_tile_count(p, &tiles, nullptr)))
        return rc;
    const int32_t n0 = o->min_spp < p->spp ? o->min_spp : p->spp;
    const int32_t longest = std::max(n0, std::min(o->pass_spp, p->spp - n0)); // samples of the longest pass
    if ((uint64_t)p->tile_w * p->tile_h * (uint64_t)longest * (uint64_t)tiles >= ((uint64_t)1 << 31))
    {
        r1_set_error("a pass of %dx%dx%d with %dx%d tiles exceeds 2^31 sample slots per launch", p->width, p->height, longest, p->tile_w, p->tile_h);
        return R1_ELIMIT;
    }
    if ((uint64_t)p->tile_w * p->tile_h > ((uint64_t)1 << 22))
    {
        r1_set_error("adaptive sampling: tiles of %dx%d pixels exceed 2^22 (a tile's err_sum is a 32-bit sum of byte differences)", p->tile_w, p->tile_h);
        return R1_ELIMIT;
    }
    const size_t n_pass = 1 + ((size_t)(p->spp - n0) + (size_t)o->pass_spp - 1) / (size_t)o->pass_spp;
    if (count)
        *count = n_pass;
    if (!n_out)
        return R1_OK;
    if (cap < n_pass)
    {
        r1_set_error("r1_adaptive_schedule: cap %zu, the schedule has %zu passes", cap, n_pass);
        return R1_EINVAL;
    }
    int64_t n = n0;
    for (size_t k = 0; k < n_pass; ++k, n += o->pass_spp)
        n_out[k] = (int32_t)std::min<int64_t>(n, p->spp);
    return R1_OK;
}

static_assert(sizeof(r1_tile_report) == sizeof(R1TileReport) && sizeof(r1_tile_report) == 16 && sizeof(r1_adaptive_result) == 24, "public structs without padding; the device writes r1_tile_report's layout");

static int readout_linear(r1_context *c, const r1_params *p, int32_t tiles, int32_t n_uniform, bool per_tile, float *rgb_out);

// r1_render_adaptive (rgb_out) and r1_render_adaptive_linear (linear_out): the passes are the same; what differs is which image goes home
static int render_adaptive(const char *who, r1_context *c, const r1_params *p, const r1_adaptive *opt, uint8_t *rgb_out, float *linear_out, uint64_t *num_rays_out,
                           r1_tile_report *tiles_out, r1_adaptive_result *result_out)
{
    if (!c || !p || !opt || (!rgb_out && !linear_out))
    {
        r1_set_error("%s: null argument", who);
        return R1_EINVAL;
    }
    size_t n_pass = 0;
    int rc = r1_adaptive_schedule(p, opt, nullptr, 0, &n_pass);
    if (rc)
        return rc;
    std::vector<int32_t> sched(n_pass);
    if ((rc = r1_adaptive_schedule(p, opt, sched.data(), n_pass, nullptr)))
        return rc;
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    int32_t tiles = 0;
    if ((rc = r1_tile_count(p, &tiles, nullptr)))
        return rc;
    R1_HIP(hipSetDevice(c->device));
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    const size_t tile_px = (size_t)p->tile_w * p->tile_h;
    if ((rc = ensure(c->image, img_bytes + 64)) || (rc = ensure(c->accum, (size_t)tiles * tile_px * 16)) || (rc = ensure(c->accum_even, (size_t)tiles * tile_px * 16)) ||
        (rc = ensure(c->adapt_list, ((size_t)2 * tiles + 1) * 4)) || (rc = ensure(c->adapt_report, (size_t)tiles * sizeof(R1TileReport))))
        return rc;
    c->pass_valid = false; // (the `all` accumulator is r1_render_pass's: an accumulation of the context ends here, as at first_sample 0)
    const bool direct = c->host_word_dev != nullptr; // ray count and list length straight into the context's page-locked words, as r1_render_pass
    uint32_t *const lists[2] = {(uint32_t *)c->adapt_list.p, (uint32_t *)c->adapt_list.p + tiles};
    uint32_t *const d_count = direct ? &c->host_word_dev->adapt_count : (uint32_t *)c->adapt_list.p + 2 * (size_t)tiles;
    R1_HIP(r1_launch_adapt_compact(nullptr, (uint32_t)tiles, (const R1TileReport *)c->adapt_report.p, 0u, lists[0], d_count, c->stream)); // every tile, in order
    uint32_t m = (uint32_t)tiles;
    uint64_t rays_sum = 0;
    int32_t passes = 0;
    for (size_t k = 0; k < n_pass && m; ++k)
    {
        const int32_t first = k ? sched[k - 1] : 0;
        r1_params pp = *p;
        pp.spp = sched[k] - first;
        Pass ps;
        ps.first_sample = first;
        ps.list = lists[k & 1], ps.n_listed = m, ps.rule = opt;
        FrameJob job;
        job.out = c->image.p, job.rays = rays_word(c, direct), job.st = c->stream, job.pass = &ps;
        if ((rc = enqueue_frame(c, &pp, job)))
            return rc;
        R1_HIP(r1_launch_adapt_compact(lists[k & 1], m, (const R1TileReport *)c->adapt_report.p, sched[k] == p->spp ? 1u : 0u, lists[(k & 1) ^ 1], d_count, c->stream));
        uint64_t rays = 0;
        uint32_t next = 0;
        if (!direct)
            R1_HIP(hipMemcpyAsync(&next, d_count, 4, hipMemcpyDeviceToHost, c->stream));
        if ((rc = read_rays(c, direct, &rays)))
            return rc;
        if (direct)
            next = *(volatile uint32_t *)&c->host_word->adapt_count;
        rays_sum += rays; // (summed on the host, pass by pass, as r1_render_pass does)
        ++passes;
        if (next > m)
        {
            r1_set_error("%s: a pass left %u active tiles of %u", who, next, m);
            return R1_EHIP;
        }
        m = next;
    }
    std::vector<r1_tile_report> local;
    r1_tile_report *rep = tiles_out;
    if (!rep)
    {
        local.resize((size_t)tiles);
        rep = local.data();
    }
    R1_HIP(hipMemcpyAsync(rep, c->adapt_report.p, (size_t)tiles * sizeof(R1TileReport), hipMemcpyDeviceToHost, c->stream));
    if (rgb_out)
        R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, c->stream));
    // the linear frame: every tile's `all` sums, each scaled by the samples its own report says it holds
    if (linear_out && (rc = readout_linear(c, p, tiles, 0, true, linear_out)))
        return rc;
    R1_HIP(hipStreamSynchronize(c->stream));
    if (num_rays_out)
        *num_rays_out = rays_sum;
    if (result_out)
    {
        uint64_t samples = 0;
        int32_t settled = 0;
        const R1TileGeom g = geom_of(p);
        for (int32_t t = 0; t < tiles; ++t)
        {
            const R1TileRect r = r1_tile_rect(g, (uint32_t)t);
            samples += (uint64_t)rep[t].spp * (uint64_t)(r.tw * r.th);
            settled += rep[t].settled ? 1 : 0;
        }
        result_out->samples = samples;
        result_out->passes = passes, result_out->tiles = tiles, result_out->tiles_settled = settled, result_out->reserved = 0;
    }
    return R1_OK;
}

extern "C" int r1_render_adaptive(r1_context *c, const r1_params *p, const r1_adaptive *opt, uint8_t *rgb_out, uint64_t *num_rays_out, r1_tile_report *tiles_out,
                                  r1_adaptive_result *result_out)
{
    return render_adaptive("r1_render_adaptive", c, p, opt, rgb_out, nullptr, num_rays_out, tiles_out, result_out);
}

// ---- linear frames ------------------------------------------------------------------
// The fp32 value every byte is quantised from: the pixel's sum in sample order times (float)(1.0f / n).  A whole frame is rendered as
// always — same launches, the byte image into the context's `image` — and r1_resolve_linear_kernel follows on the records the trace left
// (enqueue_frame's `linear`); the accumulators of a progressive or adaptive render are read out by r1_accum_linear_kernel.

// what every linear render refuses before it changes or enqueues anything
static int linear_check(const char *who, const r1_context *c, const r1_params *p)
{
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("%s renders whole frames (num_shards == 1, not %d)", who, p->num_shards);
        return R1_EINVAL;
    }
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    return R1_OK;
}

static size_t linear_bytes(const r1_params *p) { return (size_t)p->width * p->height * 3 * sizeof(float); }

// Where a launch stores a linear frame meant for `rgb_out`: the caller's own memory if the device can write there (page-locked), else
// the context's buffer, from which bring_linear enqueues the copy.
static int linear_target(r1_context *c, const r1_params *p, float *rgb_out, Linear &lin)
{
    lin.out = (float *)mapped_host(rgb_out);
    if (lin.out)
        return R1_OK;
    int rc = ensure(c->linear, linear_bytes(p));
    lin.out = (float *)c->linear.p;
    return rc;
}
static int bring_linear(r1_context *c, const r1_params *p, const Linear &lin, float *rgb_out, hipStream_t st)
{
    if (lin.out == (float *)c->linear.p)
        R1_HIP(hipMemcpyAsync(rgb_out, c->linear.p, linear_bytes(p), hipMemcpyDeviceToHost, st));
    return R1_OK;
}

// The same for a variance frame's records: page-locked memory is written by the launch itself if it is 16-byte aligned
static size_t moments_bytes(const r1_params *p) { return (size_t)p->width * p->height * sizeof(r1_moment); }
static int moments_target(r1_context *c, const r1_params *p, r1_moment *moments_out, Linear &lin)
{
    lin.moments = mapped_host(moments_out);
    if (lin.moments && !((uintptr_t)lin.moments & 15u)) // (the kernel stores whole records)
        return R1_OK;
    int rc = ensure(c->moments, moments_bytes(p));
    lin.moments = c->moments.p;
    return rc;
}
static int bring_moments(r1_context *c, const r1_params *p, const Linear &lin, r1_moment *moments_out, hipStream_t st)
{
    if (lin.moments == c->moments.p)
        R1_HIP(hipMemcpyAsync(moments_out, c->moments.p, moments_bytes(p), hipMemcpyDeviceToHost, st));
    return R1_OK;
}

// r1_render_linear (moments_out null) and r1_render_moments: the same frame; a variance frame's resolve launch stores the moment records too
static int render_linear_sync(const char *who, r1_context *c, const r1_params *p, float *rgb_out, r1_moment *moments_out, uint64_t *num_rays_out,
                              double *device_seconds_out)
{
    const bool want_moments = moments_out != nullptr;
    if (!c || !p || !rgb_out)
    {
        r1_set_error("%s: null argument", who);
        return R1_EINVAL;
    }
    int rc = linear_check(who, c, p);
    if (rc)
        return rc;
    R1_HIP(hipSetDevice(c->device));
    Linear lin;
    if ((rc = ensure(c->image, (size_t)p->width * p->height * 3 + 64)) || (rc = linear_target(c, p, rgb_out, lin)) ||
        (want_moments && (rc = moments_target(c, p, moments_out, lin))))
        return rc;
    const bool direct = !r1_is_stats(p->variant) && c->host_word_dev; // the ray count as r1_render brings it home
    FrameJob job;
    job.out = c->image.p, job.rays = rays_word(c, direct), job.st = c->stream, job.linear = &lin;
    if ((rc = enqueue_frame(c, p, job)) || (rc = bring_linear(c, p, lin, rgb_out, c->stream)) ||
        (want_moments && (rc = bring_moments(c, p, lin, moments_out, c->stream))))
        return rc;
    uint64_t rays = 0;
    if ((rc = read_rays(c, direct, &rays)) || (rc = land_check(c)))
        return rc;
    if (num_rays_out)
        *num_rays_out = rays;
    if (device_seconds_out)
    {
        float ms = 0;
        R1_HIP(hipEventElapsedTime(&ms, c->last0, c->last2)); // (the linear resolve included)
        *device_seconds_out = ms * 1e-3;
    }
    return R1_OK;
}

extern "C" int r1_render_linear(r1_context *c, const r1_params *p, float *rgb_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    return render_linear_sync("r1_render_linear", c, p, rgb_out, nullptr, num_rays_out, device_seconds_out);
}

// r1_render_async's rules.  The byte image stays in the context's device buffer; the landing of bytes into the caller's memory is not
// used (the float frame is what the caller gave memory for), the ray count still goes straight into a page-locked word.
extern "C" int r1_render_linear_async(r1_context *c, const r1_params *p, float *rgb_out, uint64_t *num_rays_out, void *hip_stream)
{
    if (!c || !p || ((rgb_out == nullptr) != (num_rays_out == nullptr)))
    {
        r1_set_error("r1_render_linear_async: null argument (rgb_out and num_rays_out are given together, or both NULL)");
        return R1_EINVAL;
    }
    int rc = linear_check("r1_render_linear_async", c, p);
    if (rc)
        return rc;
    R1_HIP(hipSetDevice(c->device));
    Linear lin;
    if ((rc = ensure(c->image, (size_t)p->width * p->height * 3 + 64)) || (rc = linear_target(c, p, rgb_out, lin)))
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    void *d_rays = nullptr; // (the context's own count word, copied below)
    if (num_rays_out && ((uintptr_t)num_rays_out & 7u) == 0 && !r1_is_stats(p->variant))
        d_rays = mapped_host(num_rays_out);
    FrameJob job;
    job.out = c->image.p, job.rays = d_rays, job.st = st, job.throughput = true, job.linear = &lin;
    if ((rc = enqueue_frame(c, p, job)))
        return rc;
    if (rgb_out && (rc = bring_linear(c, p, lin, rgb_out, st)))
        return rc;
    if (num_rays_out && !d_rays)
        R1_HIP(hipMemcpyAsync(num_rays_out, counter_at(c, R1_TAIL_RAYS), 8, hipMemcpyDeviceToHost, st));
    return R1_OK;
}

// r1_render_linear_device (no moments) and r1_render_moments_device
static int render_linear_to_device(const char *who, r1_context *c, const r1_params *p, void *d_rgb_f32, void *d_moments, void *d_num_rays, void *hip_stream)
{
    if (!c || !p || !d_rgb_f32 || !d_num_rays)
    {
        r1_set_error("%s: null argument", who);
        return R1_EINVAL;
    }
    if (((uintptr_t)d_rgb_f32 & 3u) || ((uintptr_t)d_num_rays & 7u))
    {
        r1_set_error("%s: d_rgb_f32 must be 4-byte aligned and d_num_rays 8-byte aligned", who);
        return R1_EINVAL;
    }
    int rc = linear_check(who, c, p);
    if (rc)
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = ensure(c->image, (size_t)p->width * p->height * 3 + 64)))
        return rc;
    Linear lin;
    lin.out = (float *)d_rgb_f32, lin.moments = d_moments;
    FrameJob job;
    job.out = c->image.p, job.rays = d_num_rays, job.st = hip_stream ? (hipStream_t)hip_stream : c->stream, job.throughput = true, job.linear = &lin;
    return enqueue_frame(c, p, job);
}

extern "C" int r1_render_linear_device(r1_context *c, const r1_params *p, void *d_rgb_f32, void *d_num_rays, void *hip_stream)
{
    return render_linear_to_device("r1_render_linear_device", c, p, d_rgb_f32, nullptr, d_num_rays, hip_stream);
}

// ---- variance frames ----------------------------------------------------------------
// A linear frame whose closing launch is r1_resolve_moments_kernel: the linear value and, from a second walk over the same records, the
// unbiased variance of each pixel's mean.  Everything else — checks, launches, state, timing — is the linear frame's.

extern "C" int r1_render_moments(r1_context *c, const r1_params *p, float *rgb_out, r1_moment *moments_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    if (!moments_out) // (the shared body takes a null target for "a linear frame alone")
    {
        r1_set_error("r1_render_moments: null argument");
        return R1_EINVAL;
    }
    return render_linear_sync("r1_render_moments", c, p, rgb_out, moments_out, num_rays_out, device_seconds_out);
}

extern "C" int r1_render_moments_device(r1_context *c, const r1_params *p, void *d_rgb_f32, void *d_moments, void *d_num_rays, void *hip_stream)
{
    if (!c || !p || !d_rgb_f32 || !d_moments || !d_num_rays)
    {
        r1_set_error("r1_render_moments_device: null argument");
        return R1_EINVAL;
    }
    if ((uintptr_t)d_moments & 15u)
    {
        r1_set_error("r1_render_moments_device: d_moments must be 16-byte aligned");
        return R1_EINVAL;
    }
    return render_linear_to_device("r1_render_moments_device", c, p, d_rgb_f32, d_moments, d_num_rays, hip_stream);
}

// The accumulators' read-out, then the frame on the host: `all` of r1_render_pass (n_uniform samples in every tile) or of an adaptive
// render (per_tile: the samples of each tile's report).  Synchronous.
static int readout_linear(r1_context *c, const r1_params *p, int32_t tiles, int32_t n_uniform, bool per_tile, float *rgb_out)
{
    Linear lin;
    int rc = linear_target(c, p, rgb_out, lin);
    if (rc)
        return rc;
    R1ReadoutArgs r = {};
    r.accum = (const float4 *)c->accum.p, r.report = per_tile ? (const R1TileReport *)c->adapt_report.p : nullptr;
    r.out = lin.out;
    r.geom = geom_of(p);
    r.n_tiles = (uint32_t)tiles;
    r.inv_n = per_tile ? 0.0f : (float)(1.0f / n_uniform); // rayweek1.cpp:765 at the accumulated spp
    R1_HIP(r1_launch_accum_linear(&r, c->stream));
    if ((rc = bring_linear(c, p, lin, rgb_out, c->stream)))
        return rc;
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

extern "C" int r1_pass_linear(r1_context *c, float *rgb_out, int32_t *samples_out)
{
    if (!c || !rgb_out)
    {
        r1_set_error("r1_pass_linear: null argument");
        return R1_EINVAL;
    }
    if (!c->pass_valid)
    {
        r1_set_error("r1_pass_linear: no accumulation to read (r1_render_pass starts one with first_sample 0; r1_set_scene, r1_set_camera and the updates end it)");
        return R1_EINVAL;
    }
    const r1_params *p = &c->pass_key;
    int32_t tiles = 0;
    int rc = r1_tile_count(p, &tiles, nullptr);
    if (rc)
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if ((rc = readout_linear(c, p, tiles, c->pass_samples, false, rgb_out)))
        return rc;
    if (samples_out)
        *samples_out = c->pass_samples;
    return R1_OK;
}

extern "C" int r1_render_adaptive_linear(r1_context *c, const r1_params *p, const r1_adaptive *opt, float *rgb_out, uint64_t *num_rays_out,
                                         r1_tile_report *tiles_out, r1_adaptive_result *result_out)
{
    return render_adaptive("r1_render_adaptive_linear", c, p, opt, nullptr, rgb_out, num_rays_out, tiles_out, result_out);
}

// ---- region renders -----------------------------------------------------------------
// A window of the frame: a pass with a region (r1_context.h Pass), so the launch path is enqueue_frame's and the state rules — moved scenes, the
// grid's validity, the landing state, a progressive accumulation left alone — are those of every frame.  The launch works on a dense image of
// the region's size in the context's buffers; the caller's row stride is applied by the copies home (host forms) or by the closing kernel
// itself (device form).

// the synchronous forms: bytes (rgb_out), floats (linear_out), records (samples_out)
static int render_region_host_out(const char *who, r1_context *c, const r1_params *p, const r1_region *rg, uint8_t *rgb_out, float *linear_out,
                                  uint64_t *num_rays_out, double *device_seconds_out, float *samples_out)
{
    if (!c || !p || !rg || (!rgb_out && !linear_out))
    {
        r1_set_error("%s: null argument", who);
        return R1_EINVAL;
    }
    int rc = r1_region_check(p, rg);
    if (rc)
        return rc;
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t n_px = (size_t)rg->width * rg->height;
    if ((rgb_out && (rc = ensure(c->image, n_px * 3 + 64))) || (linear_out && (rc = ensure(c->linear, n_px * 3 * sizeof(float)))))
        return rc;
    const bool direct = c->host_word_dev != nullptr; // the ray count straight into the page-locked word, as r1_render_pass
    r1_region dense = *rg;
    dense.out_stride = 0; // (the context's buffers hold the window densely)
    Pass ps;
    ps.region = &dense;
    ps.region_linear = linear_out ? (float *)c->linear.p : nullptr;
    FrameJob job;
    job.out = rgb_out ? c->image.p : nullptr, job.rays = rays_word(c, direct), job.st = c->stream, job.pass = &ps;
    if ((rc = enqueue_frame(c, p, job)))
        return rc;
    const size_t stride = rg->out_stride ? (size_t)rg->out_stride : (size_t)rg->width;
    if (rgb_out)
        R1_HIP(hipMemcpy2DAsync(rgb_out, stride * 3, c->image.p, (size_t)rg->width * 3, (size_t)rg->width * 3, (size_t)rg->height, hipMemcpyDeviceToHost, c->stream));
    if (linear_out)
        R1_HIP(hipMemcpy2DAsync(linear_out, stride * 12, c->linear.p, (size_t)rg->width * 12, (size_t)rg->width * 12, (size_t)rg->height, hipMemcpyDeviceToHost, c->stream));
    uint64_t rays = 0;
    if ((rc = read_rays(c, direct, &rays)) || (rc = land_check(c)))
        return rc;
    if (num_rays_out)
        *num_rays_out = rays;
    if (device_seconds_out)
    {
        float ms = 0;
        R1_HIP(hipEventElapsedTime(&ms, c->last0, c->last2));
        *device_seconds_out = ms * 1e-3;
    }
    if (samples_out) // dense in the region's own geometry: the gather of r1_render_samples
        return gather_records(c, r1_tile_geom(rg->width, rg->height, p->tile_w, p->tile_h), p->spp, samples_out);
    return R1_OK;
}

extern "C" int r1_render_region(r1_context *c, const r1_params *p, const r1_region *region, uint8_t *rgb_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    return render_region_host_out("r1_render_region", c, p, region, rgb_out, nullptr, num_rays_out, device_seconds_out, nullptr);
}

extern "C" int r1_render_region_samples(r1_context *c, const r1_params *p, const r1_region *region, uint8_t *rgb_out, uint64_t *num_rays_out, float *samples_out)
{
    if (!samples_out)
    {
        r1_set_error("r1_render_region_samples: null samples_out");
        return R1_EINVAL;
    }
    return render_region_host_out("r1_render_region_samples", c, p, region, rgb_out, nullptr, num_rays_out, nullptr, samples_out);
}

extern "C" int r1_render_region_linear(r1_context *c, const r1_params *p, const r1_region *region, float *rgb_out, uint64_t *num_rays_out, double *device_seconds_out)
{
    return render_region_host_out("r1_render_region_linear", c, p, region, nullptr, rgb_out, num_rays_out, device_seconds_out, nullptr);
}

extern "C" int r1_render_region_device(r1_context *c, const r1_params *p, const r1_region *region, void *d_rgb_u8, void *d_rgb_f32, void *d_num_rays, void *hip_stream)
{
    if (!c || !p || !region || (!d_rgb_u8 && !d_rgb_f32) || !d_num_rays)
    {
        r1_set_error("r1_render_region_device: null argument (an image — d_rgb_u8, d_rgb_f32 or both — and d_num_rays are needed)");
        return R1_EINVAL;
    }
    if (((uintptr_t)d_rgb_f32 & 3u) || ((uintptr_t)d_num_rays & 7u))
    {
        r1_set_error("r1_render_region_device: d_rgb_f32 must be 4-byte aligned and d_num_rays 8-byte aligned");
        return R1_EINVAL;
    }
    int rc = r1_region_check(p, region);
    if (rc)
        return rc;
    if (!c->have_scene)
    {
        r1_set_error("no scene set (call r1_set_scene first)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    Pass ps;
    ps.region = region; // (the closing kernel applies the caller's row stride)
    ps.region_linear = (float *)d_rgb_f32;
    FrameJob job;
    job.out = d_rgb_u8, job.rays = d_num_rays, job.st = hip_stream ? (hipStream_t)hip_stream : c->stream, job.pass = &ps;
    return enqueue_frame(c, p, job);
}

// Pipelined form of r1_render (frames in flight, results on the HOST): the frame is enqueued with the throughput
// kernels on `hip_stream` (or the context's stream), followed by the copies of the row-major image and of the ray
// count into the caller's buffers.  Nothing is waited for: the buffers are valid once the stream is idle (r1_sync for
// the context's stream).  One frame per context at a time — a caller keeps K frames in flight with K contexts, as
// bench.py does.  Page-locked buffers (r1_host_alloc) let the copies overlap the other frames' kernels; pageable
// memory works but makes each copy wait for its frame.
extern "C" int r1_render_async(r1_context *c, const r1_params *p, uint8_t *rgb_out, uint64_t *num_rays_out, void *hip_stream)
{
    if (!c || !p || ((rgb_out == nullptr) != (num_rays_out == nullptr)))
    {
        r1_set_error("r1_render_async: null argument (rgb_out and num_rays_out are given together, or both NULL)");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("r1_render_async renders whole frames (num_shards == 1); shards go through r1_render_shard_device");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t img_bytes = (size_t)p->width * p->height * 3;
    if ((rc = ensure(c->image, img_bytes + 64)))
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // page-locked buffers (r1_host_alloc) receive the tiles and the count straight from the trace kernel's resolvers: nothing to copy
    Landing land_to;
    if (rgb_out && ((uintptr_t)num_rays_out & 7u) == 0)
        land_to.out = mapped_host(rgb_out), land_to.rays = mapped_host(num_rays_out);
    FrameJob job;
    job.out = c->image.p, job.st = st, job.throughput = true, job.landing = &land_to;
    if ((rc = enqueue_frame(c, p, job)))
        return rc;
    if (rgb_out && !land_to.used) // (both NULL: the frame stays in the context's device buffers — a measurement aid, bench.py's value_device_resident)
    {
        R1_HIP(hipMemcpyAsync(rgb_out, c->image.p, img_bytes, hipMemcpyDeviceToHost, st));
        R1_HIP(hipMemcpyAsync(num_rays_out, counter_at(c, R1_TAIL_RAYS), 8, hipMemcpyDeviceToHost, st));
    }
    return R1_OK;
}

// n_frames frames of the same scene, camera and size in ONE launch (frame f seeded params->seed + f * seed_stride): the
// persistent waves flow from one frame into the next, so the ramp and drain of a launch are paid once per batch.
// Whole frames (num_shards == 1): host_frames receives n_frames frame records (r1_frame_record_bytes each) with ONE copy.
// cameras (null: the context's camera for every frame): a camera path.  `who`: the entry point, which has checked its own arguments.
static int render_frames_async(const char *who, r1_context *c, const r1_params *p, int32_t n_frames, uint32_t seed_stride, const r1_camera *cameras,
                               void *host_frames, void *hip_stream)
{
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    if (p->num_shards != 1)
    {
        r1_set_error("%s renders whole frames (num_shards == 1)%s", who, cameras ? "" : "; shards go through r1_render_shard_device_batch");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    const size_t frame = r1_frame_record_bytes(p);
    if ((rc = ensure(c->image, frame * (size_t)n_frames)))
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    Batch b;
    b.n_frames = n_frames, b.seed_stride = seed_stride, b.out_stride = frame, b.rays_offset = frame - 8;
    b.cameras = cameras;
    Landing land_to;
    if (host_frames && ((uintptr_t)host_frames & 7u) == 0)
        land_to.out = mapped_host(host_frames);
    FrameJob job;
    job.out = c->image.p, job.st = st, job.throughput = true, job.batch = &b, job.landing = &land_to;
    if ((rc = enqueue_frame(c, p, job)))
        return rc;
    if (host_frames && !land_to.used) // (NULL: the frames stay in the context's device buffer — a measurement aid)
        R1_HIP(hipMemcpyAsync(host_frames, c->image.p, frame * (size_t)n_frames, hipMemcpyDeviceToHost, st));
    return R1_OK;
}

extern "C" int r1_render_batch_async(r1_context *c, const r1_params *p, int32_t n_frames, uint32_t seed_stride, void *host_frames, void *hip_stream)
{
    if (!c || !p || n_frames < 1)
    {
        r1_set_error("r1_render_batch_async: bad argument");
        return R1_EINVAL;
    }
    return render_frames_async("r1_render_batch_async", c, p, n_frames, seed_stride, nullptr, host_frames, hip_stream);
}

// A camera path: r1_render_batch_async with cameras[f] in place of the context's camera for frame f (the R1_MODE_PATH kernels; one frame: the
// single-frame kernel with cameras[0] by value).  The context's own camera is not touched.
extern "C" int r1_render_path_async(r1_context *c, const r1_params *p, int32_t n_frames, uint32_t seed_stride, const r1_camera *cameras, void *host_frames,
                                    void *hip_stream)
{
    if (!c || !p || !cameras || n_frames < 1)
    {
        r1_set_error("r1_render_path_async: bad argument (%s)", !c ? "ctx is NULL" : !p ? "params is NULL" : !cameras ? "cameras is NULL" : "n_frames < 1");
        return R1_EINVAL;
    }
    return render_frames_async("r1_render_path_async", c, p, n_frames, seed_stride, cameras, host_frames, hip_stream);
}

// The same for one shard of n_frames frames: d_records receives n_frames records (r1_shard_record_bytes each: dense tile
// block + uint64 ray count), device memory — what a rank hands to ONE all-gather per batch.
extern "C" int r1_render_shard_device_batch(r1_context *c, const r1_params *p, int32_t n_frames, uint32_t seed_stride, void *d_records, void *hip_stream)
{
    if (!c || !p || !d_records || n_frames < 1 || ((uintptr_t)d_records & 7u))
    {
        r1_set_error("r1_render_shard_device_batch: bad argument (d_records must be 8-byte aligned)");
        return R1_EINVAL;
    }
    int rc = r1_params_check(p);
    if (rc)
        return rc;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const size_t record = r1_shard_record_bytes(p);
    Batch b;
    b.n_frames = n_frames, b.seed_stride = seed_stride, b.out_stride = record, b.rays_offset = record - 8;
    FrameJob job;
    job.out = d_records, job.block_layout = 1, job.st = st, job.throughput = true, job.batch = &b;
    return enqueue_frame(c, p, job);
}

extern "C" int r1_render_shard_device(r1_context *c, const r1_params *p, void *d_block, void *d_num_rays, void *hip_stream)
{
    if (!c || !p || !d_block || !d_num_rays)
    {
        r1_set_error("r1_render_shard_device: null argument");
        return R1_EINVAL;
    }
    if ((uintptr_t)d_num_rays & 7u)
    {
        r1_set_error("r1_render_shard_device: d_num_rays must be 8-byte aligned (a uint64 the kernels store and add to atomically)");
        return R1_EINVAL;
    }
    FrameJob job;
    job.out = d_block, job.block_layout = 1, job.rays = d_num_rays, job.st = hip_stream ? (hipStream_t)hip_stream : c->stream, job.throughput = true;
    return enqueue_frame(c, p, job);
}

extern "C" int r1_render_shard_device_once(r1_context *c, const r1_params *p, void *d_block, void *d_num_rays, void *hip_stream)
{
    if (!c || !p || !d_block || !d_num_rays)
    {
        r1_set_error("r1_render_shard_device_once: null argument");
        return R1_EINVAL;
    }
    if ((uintptr_t)d_num_rays & 7u)
    {
        r1_set_error("r1_render_shard_device_once: d_num_rays must be 8-byte aligned");
        return R1_EINVAL;
    }
    FrameJob job;
    job.out = d_block, job.block_layout = 1, job.rays = d_num_rays, job.st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    return enqueue_frame(c, p, job);
}

static int assemble_common(r1_context *c, const r1_params *p, const void *d_blocks, size_t shard_stride_bytes, void *d_rgb, void *d_total_rays,
                           void *hip_stream, int n_frames = 1, size_t frame_in = 0, size_t frame_out = 0)
{
    if (!c || !p || !d_blocks || !d_rgb)
    {
        r1_set_error("r1_assemble_device: null argument");
        return R1_EINVAL;
    }
    int32_t total = 0, per = 0;
    int rc = r1_tile_count(p, &total, &per);
    if (rc)
        return rc;
    const size_t tight = (size_t)per * p->tile_w * p->tile_h * 3;
    if (shard_stride_bytes == 0)
        shard_stride_bytes = tight;
    if (shard_stride_bytes < tight)
    {
        r1_set_error("r1_assemble_device: shard stride %zu smaller than a shard block (%zu bytes)", shard_stride_bytes, tight);
        return R1_EINVAL;
    }
    if (d_total_rays && (((uintptr_t)d_total_rays | (uintptr_t)d_blocks | shard_stride_bytes | frame_in | frame_out) & 7u))
    {
        r1_set_error("r1_assemble_device_records: records and totals must be 8-byte aligned");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    R1AssembleArgs a = {};
    a.blocks = (const uint8_t *)d_blocks, a.rgb = (uint8_t *)d_rgb;
    a.geom = geom_of(p), a.num_shards = p->num_shards, a.n_frames = n_frames;
    a.shard_stride = shard_stride_bytes, a.frame_in = frame_in, a.frame_out = frame_out;
    a.total_offset = r1_shard_record_bytes(p) - 8; // (where a record keeps its shard's count)
    a.total_out = d_total_rays ? (long long)((char *)d_total_rays - (char *)d_rgb) : 0, a.want_total = d_total_rays ? 1 : 0;
    R1_HIP(r1_launch_assemble(&a, st));
    return R1_OK;
}

extern "C" int r1_assemble_device_strided(r1_context *c, const r1_params *p, const void *d_blocks, size_t shard_stride_bytes, void *d_rgb,
                                          void *hip_stream)
{
    return assemble_common(c, p, d_blocks, shard_stride_bytes, d_rgb, nullptr, hip_stream);
}

extern "C" int r1_assemble_device_records(r1_context *c, const r1_params *p, const void *d_records, void *d_rgb, void *d_total_rays, void *hip_stream)
{
    if (!d_total_rays)
    {
        r1_set_error("r1_assemble_device_records: null d_total_rays");
        return R1_EINVAL;
    }
    return assemble_common(c, p, d_records, r1_shard_record_bytes(p), d_rgb, d_total_rays, hip_stream);
}

// Batches: d_gathered = what one all-gather of every shard's n_frames records returns, [shard][frame][record]; d_frames receives
// n_frames frame records (r1_frame_record_bytes each: row-major image, padded to 8 bytes, + the frame's uint64 ray count).
extern "C" int r1_assemble_device_records_batch(r1_context *c, const r1_params *p, int32_t n_frames, const void *d_gathered, void *d_frames,
                                                void *hip_stream)
{
    if (n_frames < 1 || !d_frames)
    {
        r1_set_error("r1_assemble_device_records_batch: bad argument");
        return R1_EINVAL;
    }
    const size_t record = r1_shard_record_bytes(p), frame = r1_frame_record_bytes(p);
    if (!record)
        return R1_EINVAL;
    return assemble_common(c, p, d_gathered, record * (size_t)n_frames, d_frames, (char *)d_frames + frame - 8, hip_stream, n_frames, record, frame);
}

extern "C" int r1_assemble_device(r1_context *c, const r1_params *p, const void *d_blocks, void *d_rgb, void *hip_stream)
{
    return r1_assemble_device_strided(c, p, d_blocks, 0, d_rgb, hip_stream);
}
