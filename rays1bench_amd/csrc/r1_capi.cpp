// r1_capi.cpp — the C-ABI of include/rays1.h on top of the HIP runtime: errors, the context's life, timing and what the last launch
// left to read.  Host code only.  The scene upload is r1_scene.cpp (its edits r1_scene_update.cpp, its grid r1_scene_grid.cpp), a frame's
// steps r1_frame.cpp, the render entry points r1_render.cpp, the ray queries r1_queries.cpp (the trace kernel lives in r1_trace.hpp).
//
// There is no CPU fallback anywhere in these files: without a HIP device every compute entry point returns R1_ENODEVICE / R1_EHIP.

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "r1_context.h"

// ---- errors ---------------------------------------------------------------------------------

static thread_local char g_error[512] = "";

extern "C" void r1_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

extern "C" const char *r1_last_error(void) { return g_error; }
extern "C" int r1_abi_version(void) { return R1_ABI_VERSION; }

// ---- context ----------------------------------------------------------------------------------

extern "C" int r1_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
    {
        r1_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return R1_ENODEVICE;
    }
    return n;
}

extern "C" int r1_create(int device, r1_context **out)
{
    if (!out)
        return R1_EINVAL;
    *out = nullptr;
    int n = r1_device_count();
    if (n <= 0)
    {
        if (n == 0)
            r1_set_error("no HIP device visible (librays1 has no CPU fallback)");
        return R1_ENODEVICE;
    }
    if (device < 0 || device >= n)
    {
        r1_set_error("device %d out of range (0..%d)", device, n - 1);
        return R1_EINVAL;
    }
    r1_context *c = new (std::nothrow) r1_context();
    if (!c)
        return R1_ENOMEM;
    c->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess)
        e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipEventCreate(&c->ev0);
    if (e == hipSuccess)
        e = hipEventCreate(&c->ev1);
    if (e == hipSuccess)
        e = hipEventCreate(&c->ev2);
    if (e != hipSuccess)
    {
        r1_set_error("r1_create: %s", hipGetErrorString(e));
        delete c;
        return R1_EHIP;
    }
    if (hipHostMalloc((void **)&c->host_word, sizeof(R1HostWords), hipHostMallocMapped) == hipSuccess)
    {
        memset(c->host_word, 0, sizeof(R1HostWords)); // (the runtime may hand back a recycled block: land_error is land_check's "a resolver gave up" flag)
        if (hipHostGetDevicePointer((void **)&c->host_word_dev, c->host_word, 0) != hipSuccess)
        {
            (void)hipHostFree(c->host_word);
            c->host_word = c->host_word_dev = nullptr;
        }
    }
    else
        c->host_word = nullptr; // (not fatal: the count is copied instead)
    (void)hipGetLastError();
    c->cus = prop.multiProcessorCount;
    memset(&c->info, 0, sizeof(c->info));
    c->info.compute_units = c->cus;
    *out = c;
    return R1_OK;
}

// internal (r1_multi.cpp): the context's own stream, so that the in-process multi-GPU path runs its collectives on the stream the
// context's uploads and frames already use instead of a second stream per device (every stream wants a hardware queue)
extern "C" void *r1_context_stream(r1_context *c) { return c ? (void *)c->stream : nullptr; }

// internal (tests/test_builds_host.py): r1_pick as the frames' choose_kernel calls it
extern "C" int r1_pick_build(int variant, int big, int want, int *build4)
{
    R1Build b = {0, false, false, 0};
    if (!r1_pick(variant, big != 0, want, b))
        return 0;
    build4[0] = b.variant, build4[1] = b.stats ? 1 : 0, build4[2] = b.big ? 1 : 0, build4[3] = b.mode;
    return 1;
}

// internal (the same test): what the predicates of r1_builds.h answer
extern "C" void r1_build_facts(int variant, int mode, int big, int *facts6)
{
    facts6[0] = r1_is_tree(variant), facts6[1] = r1_is_grid(variant), facts6[2] = r1_is_stats(variant), facts6[3] = r1_base_variant(variant);
    facts6[4] = r1_mode_is_tp_family(mode), facts6[5] = r1_runs_as_latency(mode, big != 0);
}

extern "C" void r1_destroy(r1_context *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    if (c->stage)
        (void)hipHostFree(c->stage);
    if (c->stage_ev)
        (void)hipEventDestroy(c->stage_ev);
    if (c->host_word)
        (void)hipHostFree(c->host_word);
    for (hipEvent_t e : c->ring)
        (void)hipEventDestroy(e);
    if (c->ev0)
        (void)hipEventDestroy(c->ev0);
    if (c->ev1)
        (void)hipEventDestroy(c->ev1);
    if (c->ev2)
        (void)hipEventDestroy(c->ev2);
    if (c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c; // (frees every DevBuf: on the device set above)
}

// a resolver of an earlier launch gave up waiting (R1_LAND_MAX_WAIT): the frames of that launch are not valid
int land_check(r1_context *c)
{
    volatile uint32_t *const error = c->host_word ? &c->host_word->land_error : nullptr;
    if (error && *error)
    {
        *error = 0;
        r1_set_error("a launch did not resolve all of its tiles (a resolver workgroup gave up waiting): its frames are not valid");
        return R1_EHIP;
    }
    return R1_OK;
}

extern "C" int r1_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0)
        return R1_EINVAL;
    *out = nullptr;
    if (r1_device_count() <= 0)
        return R1_ENODEVICE;
    R1_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return R1_OK;
}

extern "C" void r1_host_free(void *p)
{
    if (p)
        (void)hipHostFree(p);
}

extern "C" int r1_set_pixel_mode(r1_context *c, int32_t on)
{
    if (!c)
        return R1_EINVAL;
    c->pixel_mode = on != 0;
    return R1_OK;
}

extern "C" int r1_sync(r1_context *c)
{
    if (!c)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    return land_check(c);
}

extern "C" int r1_last_timing(r1_context *c, double *trace_kernel_ms, double *total_ms)
{
    if (!c || !c->timing_valid)
    {
        r1_set_error("r1_last_timing: nothing rendered yet");
        return R1_EINVAL;
    }
    R1_HIP(hipEventSynchronize(c->last2));
    float a = 0, b = 0;
    R1_HIP(hipEventElapsedTime(&a, c->last0, c->last1));
    R1_HIP(hipEventElapsedTime(&b, c->last0, c->last2));
    if (trace_kernel_ms)
        *trace_kernel_ms = a;
    if (total_ms)
        *total_ms = b;
    return R1_OK;
}

extern "C" int r1_last_stats(r1_context *c, uint64_t *out16)
{
    if (!c || !out16 || !c->counters.p)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    R1_HIP(hipMemcpyAsync(out16, counter_at(c, R1_CNT_STATS), 8 * R1_STATS_WORDS, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

extern "C" int r1_last_wave_log(r1_context *c, uint64_t *out, size_t cap_waves, uint32_t *waves)
{
    if (!c || !waves)
        return R1_EINVAL;
    *waves = c->wave_log_waves;
    if (!out)
        return R1_OK;
    if (cap_waves < c->wave_log_waves || !c->wave_log.p)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    R1_HIP(hipMemcpyAsync(out, c->wave_log.p, (size_t)c->wave_log_waves * 32, hipMemcpyDeviceToHost, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    return R1_OK;
}

extern "C" int r1_timing_begin(r1_context *c, int32_t max_frames)
{
    if (!c || max_frames < 1 || max_frames > 100000)
    {
        r1_set_error("r1_timing_begin: bad argument");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    while ((int)c->ring.size() < 3 * max_frames)
    {
        hipEvent_t e;
        R1_HIP(hipEventCreate(&e));
        c->ring.push_back(e);
    }
    c->ring_frames = max_frames;
    c->ring_used = 0;
    c->ring_on = true;
    return R1_OK;
}

extern "C" int r1_timing_end(r1_context *c, double *trace_ms_sum, double *total_ms_sum, int32_t *frames)
{
    if (!c || !c->ring_on)
    {
        r1_set_error("r1_timing_end without r1_timing_begin");
        return R1_EINVAL;
    }
    c->ring_on = false;
    double a = 0, b = 0;
    for (int i = 0; i < c->ring_used; ++i)
    {
        float x = 0, y = 0;
        R1_HIP(hipEventSynchronize(c->ring[3 * i + 2]));
        R1_HIP(hipEventElapsedTime(&x, c->ring[3 * i], c->ring[3 * i + 1]));
        R1_HIP(hipEventElapsedTime(&y, c->ring[3 * i], c->ring[3 * i + 2]));
        a += x, b += y;
    }
    if (trace_ms_sum)
        *trace_ms_sum = a;
    if (total_ms_sum)
        *total_ms_sum = b;
    if (frames)
        *frames = c->ring_used;
    return R1_OK;
}

extern "C" int r1_last_launch_info(r1_context *c, r1_launch_info *out)
{
    if (!c || !out)
        return R1_EINVAL;
    *out = c->info;
    return R1_OK;
}

extern "C" int r1_last_walk_form(r1_context *c) { return c ? c->walk_form : R1_EINVAL; }

// internal (tools/land_debug.py): the context's counter allocation as it is after the stream has drained
extern "C" int r1_debug_dump_counters(r1_context *c, void *out, size_t bytes, size_t *have)
{
    if (!c || !out || !c->counters.p)
        return R1_EINVAL;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipStreamSynchronize(c->stream));
    const size_t n = bytes < c->counters.cap ? bytes : c->counters.cap;
    R1_HIP(hipMemcpy(out, c->counters.p, n, hipMemcpyDeviceToHost));
    if (have)
        *have = n;
    return R1_OK;
}
