// tools/check_exact_rlen.hip — r1_rlen_guarded / r1_rlen_total (rays1bench_amd/csrc/r1_exact_math.h) against
// `1.0f / __builtin_sqrtf(x)`, bit for bit, for every fp32 bit pattern, on the GPU it runs on.  Built with the project's flags by
// the Makefile's default target into rays1bench_amd/lib/check_exact_rlen; run by tests/test_gpu_exact_rlen.py.
//
//   pass 1   the guarded form, all 2^32 patterns, lane i of a wave holding pattern base + i, all lanes active.  Also: the wave
//            took the short sequence exactly when its 64 patterns all lie in D = [2^-96, FLT_MAX].
//   pass 2a  mixed waves: lane i holds base + i * 0x04000001 (mod 2^32) — both signs, tiny, normal, infinite and NaN side by
//            side — for every base in [0, 2^26), all lanes active: the compiler's arm, every lane must equal.
//   pass 2b  the same waves with exactly the lanes outside D inactive: the short sequence must be taken, the active lanes
//            must equal, the others are not looked at.
//   pass 3   the branch-free total form, all 2^32 patterns, all lanes active: equal for every pattern — tiny, subnormal, +-0,
//            +-inf, negative, NaN with its payload.  It has no arms: its fast_waves are 0.
// usage: check_exact_rlen [--form 0|1|2|3|4] [--out FILE]     (default: the form the kernels are built with)
// Prints one `key value` line per figure and the first mismatches; exit status 0 only for zero mismatches and the expected
// arms.  Vector stores and one atomic counter (the slot of a mismatch record); every loop is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../rays1bench_amd/csrc/r1_exact_math.h"

#define CK(x)                                                                                 \
    do                                                                                        \
    {                                                                                         \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess)                                                                 \
        {                                                                                     \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                          \
        }                                                                                     \
    } while (0)

constexpr uint32_t BLOCK = 256, WAVES = 1u << 14, ITERS = 1u << 12; // 2^14 waves x 2^12 trips = 2^26 wave evaluations of 64 lanes
constexpr uint32_t GRID = WAVES * 64u / BLOCK;
constexpr uint32_t MAX_REC = 16;
struct WaveOut
{
    uint32_t mismatches, fast, fast_expected, arm_errors;
};

// D, written differently from the header on purpose: sign clear, exponent field 31..254
__device__ __forceinline__ bool in_d_fields(const uint32_t b) { return (b >> 31) == 0u && ((b >> 23) & 255u) >= 31u && ((b >> 23) & 255u) <= 254u; }

// MODE 0: pass 1, 1: pass 2a, 2: pass 2b, 3: pass 3
template <int FORM, int MODE>
__global__ void __launch_bounds__(BLOCK) check_kernel(WaveOut *out, uint32_t *rec, uint32_t *rec_count)
{
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * BLOCK + threadIdx.x) >> 6;
    uint32_t mism = 0, fastn = 0, fast_exp = 0, arm_err = 0;
    for (uint32_t it = 0; it < ITERS; ++it)
    {
        const uint32_t base = wave * ITERS + it; // [0, 2^26)
        const uint32_t bits = (MODE == 0 || MODE == 3) ? base * 64u + lane : base + lane * 0x04000001u;
        const float x = __uint_as_float(bits);
        const bool in_d = in_d_fields(bits);
        const bool active = MODE == 2 ? in_d : true;
        const unsigned long long act = __builtin_amdgcn_ballot_w64(active);
        bool fast = false;
        const float got = MODE == 3 ? r1_rlen_total_form<FORM>(x) : r1_rlen_guarded_form<FORM>(x, act, fast);
        const float want = 1.0f / __builtin_sqrtf(x);
        const bool expect_fast = FORM != 0 && MODE != 3 && (MODE == 2 || __builtin_amdgcn_ballot_w64(!in_d) == 0ull);
        fastn += fast ? 1u : 0u, fast_exp += expect_fast ? 1u : 0u, arm_err += fast != expect_fast ? 1u : 0u;
        if (active && __float_as_uint(got) != __float_as_uint(want))
        {
            ++mism;
            const uint32_t slot = atomicAdd(rec_count, 1u);
            if (slot < MAX_REC)
                rec[3 * slot] = bits, rec[3 * slot + 1] = __float_as_uint(got), rec[3 * slot + 2] = __float_as_uint(want);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        mism += __shfl_down(mism, off, 64);
    if (lane == 0u) // (the arm is a property of the wave: lane 0's count is the wave's)
    {
        WaveOut w;
        w.mismatches = mism, w.fast = fastn, w.fast_expected = fast_exp, w.arm_errors = arm_err;
        out[wave] = w;
    }
}

// what v_rsq_f32 itself returns for one input of each class, next to both functions: the class routing of the total form
// (r1_rlen_total_form) rests on these
constexpr uint32_t N_PROBE = 16;
__constant__ uint32_t probe_in[N_PROBE] = {0x00000000u, 0x80000000u, 0x00000001u, 0x007FFFFFu, 0x00800000u, 0x0F7FFFFFu, 0x0F800000u, 0x3F800000u,
                                           0x7F7FFFFFu, 0x7F800000u, 0xFF800000u, 0x80000001u, 0xBF800000u, 0x7FC00000u, 0x7F800001u, 0xFFC12345u};
template <int FORM>
__global__ void __launch_bounds__(64) probe_kernel(uint32_t *out)
{
    const uint32_t i = threadIdx.x;
    if (i < N_PROBE)
    {
        const float x = __uint_as_float(probe_in[i]);
        out[4 * i] = probe_in[i], out[4 * i + 1] = __float_as_uint(__builtin_amdgcn_rsqf(x));
        out[4 * i + 2] = __float_as_uint(r1_rlen_total_form<FORM>(x)), out[4 * i + 3] = __float_as_uint(1.0f / __builtin_sqrtf(x));
    }
}

struct PassResult
{
    unsigned long long mismatches, fast, fast_expected, arm_errors, waves;
    float ms;
    std::vector<uint32_t> rec;
};

template <int FORM, int MODE>
static PassResult run_pass(WaveOut *d_out, uint32_t *d_rec, uint32_t *d_cnt)
{
    CK(hipMemset(d_out, 0, WAVES * sizeof(WaveOut)));
    CK(hipMemset(d_rec, 0, 3 * MAX_REC * sizeof(uint32_t)));
    CK(hipMemset(d_cnt, 0, sizeof(uint32_t)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0));
    check_kernel<FORM, MODE><<<GRID, BLOCK>>>(d_out, d_rec, d_cnt);
    CK(hipGetLastError());
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    PassResult r = {};
    CK(hipEventElapsedTime(&r.ms, e0, e1));
    std::vector<WaveOut> h(WAVES);
    CK(hipMemcpy(h.data(), d_out, WAVES * sizeof(WaveOut), hipMemcpyDeviceToHost));
    for (const WaveOut &w : h)
        r.mismatches += w.mismatches, r.fast += w.fast, r.fast_expected += w.fast_expected, r.arm_errors += w.arm_errors;
    r.waves = (unsigned long long)WAVES * ITERS;
    uint32_t n = 0;
    CK(hipMemcpy(&n, d_cnt, sizeof n, hipMemcpyDeviceToHost));
    r.rec.resize(3 * (n < MAX_REC ? n : MAX_REC));
    if (!r.rec.empty())
        CK(hipMemcpy(r.rec.data(), d_rec, r.rec.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    return r;
}

template <int FORM>
static int run_form(std::string &text)
{
    WaveOut *d_out;
    uint32_t *d_rec, *d_cnt;
    CK(hipMalloc(&d_out, WAVES * sizeof(WaveOut)));
    CK(hipMalloc(&d_rec, 3 * MAX_REC * sizeof(uint32_t)));
    CK(hipMalloc(&d_cnt, sizeof(uint32_t)));
    const PassResult p[4] = {run_pass<FORM, 0>(d_out, d_rec, d_cnt), run_pass<FORM, 1>(d_out, d_rec, d_cnt), run_pass<FORM, 2>(d_out, d_rec, d_cnt),
                             run_pass<FORM, 3>(d_out, d_rec, d_cnt)};
    uint32_t *d_probe, probe[4 * N_PROBE];
    CK(hipMalloc(&d_probe, sizeof probe));
    probe_kernel<FORM><<<1, 64>>>(d_probe);
    CK(hipGetLastError());
    CK(hipMemcpy(probe, d_probe, sizeof probe, hipMemcpyDeviceToHost));
    CK(hipFree(d_probe));
    CK(hipFree(d_out));
    CK(hipFree(d_rec));
    CK(hipFree(d_cnt));
    // pass 1: the waves of 64 consecutive patterns inside [0x0F800000, 0x7F7FFFFF]; pass 2a: none (lanes 0 and 32 differ in sign);
    // pass 2b: all of them; pass 3: the total form has no arms
    const unsigned long long want_fast[4] = {FORM ? 0x70000000ull / 64ull : 0ull, 0ull, FORM ? 1ull << 26 : 0ull, 0ull};
    static const char *const names[4] = {"pass1", "pass2a", "pass2b", "pass3"};
    unsigned long long bad = 0;
    char line[256];
    for (int i = 0; i < 4; ++i)
    {
        snprintf(line, sizeof line, "%s_mismatches %llu\n%s_waves %llu\n%s_fast_waves %llu\n%s_fast_waves_expected %llu\n%s_fast_share %.6f\n%s_arm_errors %llu\n%s_ms %.3f\n",
                 names[i], p[i].mismatches, names[i], p[i].waves, names[i], p[i].fast, names[i], want_fast[i], names[i], (double)p[i].fast / (double)p[i].waves,
                 names[i], p[i].arm_errors, names[i], p[i].ms);
        text += line;
        for (size_t k = 0; k + 2 < p[i].rec.size(); k += 3)
        {
            snprintf(line, sizeof line, "%s_mismatch x 0x%08x got 0x%08x want 0x%08x\n", names[i], p[i].rec[k], p[i].rec[k + 1], p[i].rec[k + 2]);
            text += line;
        }
        bad += p[i].mismatches + p[i].arm_errors + (p[i].fast != want_fast[i]) + (p[i].fast_expected != want_fast[i]);
    }
    for (uint32_t i = 0; i < N_PROBE; ++i)
    {
        snprintf(line, sizeof line, "probe_0x%08x rsq 0x%08x total 0x%08x want 0x%08x\n", probe[4 * i], probe[4 * i + 1], probe[4 * i + 2], probe[4 * i + 3]);
        text += line;
    }
    snprintf(line, sizeof line, "mismatches %llu\nverdict %s\n", p[0].mismatches + p[1].mismatches + p[2].mismatches + p[3].mismatches, bad ? "FAIL" : "PASS");
    text += line;
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    int form = R1_RLEN_FORM;
    const char *out = nullptr;
    for (int i = 1; i < argc; ++i)
    {
        if (!strcmp(argv[i], "--form") && i + 1 < argc)
            form = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--out") && i + 1 < argc)
            out = argv[++i];
        else
        {
            fprintf(stderr, "usage: %s [--form 0|1|2|3|4] [--out FILE]\n", argv[0]);
            return 2;
        }
    }
    int n = 0;
    CK(hipGetDeviceCount(&n));
    if (n < 1)
    {
        fprintf(stderr, "check_exact_rlen: no HIP device\n");
        return 2;
    }
    CK(hipSetDevice(0));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    char head[256];
    snprintf(head, sizeof head, "device %s\narch %s\nform %d\nshipped_form %d\n", prop.name, prop.gcnArchName, form, R1_RLEN_FORM);
    std::string text = head;
    int rc;
    if (form == 4)
        rc = run_form<4>(text);
    else if (form == 3)
        rc = run_form<3>(text);
    else if (form == 2)
        rc = run_form<2>(text);
    else if (form == 1)
        rc = run_form<1>(text);
    else if (form == 0)
        rc = run_form<0>(text);
    else
    {
        fprintf(stderr, "check_exact_rlen: unknown form %d\n", form);
        return 2;
    }
    fputs(text.c_str(), stdout);
    if (out)
    {
        FILE *f = fopen(out, "w");
        if (!f)
        {
            perror(out);
            return 2;
        }
        fputs(text.c_str(), f);
        fclose(f);
    }
    return rc;
}
