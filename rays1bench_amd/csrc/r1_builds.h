// r1_builds.h — the trace kernel's builds: the names of variants and modes, the predicates host and device code decide by, the list of what
// each translation unit instantiates, and the one place where a call's wish becomes a build (r1_pick).  Included through r1_device.h.
#ifndef R1_BUILDS_H
#define R1_BUILDS_H

// Internal variant numbers = the public enum of include/rays1.h (r1_frame.cpp resolve_variant asserts it), DEFAULT resolved.
constexpr int R1_V_REFERENCE = 1;   // exhaustive sweep, the reference's form
constexpr int R1_V_SWEEP = 2;       // grouped exhaustive sweep (R1_VARIANT_PREFILTER)
constexpr int R1_V_SWEEP_STATS = 3; // ... its diagnostic build
constexpr int R1_V_TREE = 4;        // box tree (R1_VARIANT_BVH)
constexpr int R1_V_TREE_STATS = 5;
constexpr int R1_V_WAVEFRONT = 6;   // r1_aux_kernels.hip: no build of the trace body
constexpr int R1_V_GRID = 7;        // uniform grid
constexpr int R1_V_GRID_STATS = 8;

// The MODE template argument of r1_trace_body, and what a caller asks r1_pick for.
constexpr int R1_MODE_TP = 0;     // frames in flight (the throughput entry points): samples in one guided queue, few long-lived waves per frame
constexpr int R1_MODE_LAT = 1;    // latency (the synchronous entry points: one frame, full grid): sub-queues and the cooperative tail
constexpr int R1_MODE_PIXEL = 2;  // the throughput entry points after r1_set_pixel_mode: the queue holds pixels (r1_sample.hpp struct Pixel)
constexpr int R1_MODE_BATCH = 3;  // TP whose queue spans the frames of a batch (R1BatchArgs)
constexpr int R1_MODE_PASS = 4;   // a progressive pass (r1_render_pass): records take the pass-local sample index, seeds the global one (R1PassArgs)
constexpr int R1_MODE_PATH = 5;   // BATCH with one camera per frame, read from a device table where a sample starts (R1PathArgs)
constexpr int R1_MODE_LISTED = 6; // PASS whose local tile j is tile list[j] of the frame (r1_render_adaptive)
constexpr int R1_MODES = 7;

constexpr bool r1_is_tree(int variant) { return variant == R1_V_TREE || variant == R1_V_TREE_STATS; }
constexpr bool r1_is_grid(int variant) { return variant == R1_V_GRID || variant == R1_V_GRID_STATS; }
constexpr bool r1_is_stats(int variant) { return variant == R1_V_SWEEP_STATS || variant == R1_V_TREE_STATS || variant == R1_V_GRID_STATS; }
// the VARIANT template argument a variant's kernels are built with (a diagnostic build is STATS = true of its product variant)
constexpr int r1_base_variant(int variant) { return r1_is_stats(variant) ? variant - 1 : variant; }

constexpr bool r1_mode_is_batch(int mode) { return mode == R1_MODE_BATCH || mode == R1_MODE_PATH; }         // R1TraceArgs::batch -> R1BatchArgs
constexpr bool r1_mode_is_pass(int mode) { return mode == R1_MODE_PASS || mode == R1_MODE_LISTED; }         // R1TraceArgs::batch -> R1PassArgs
constexpr bool r1_mode_is_tp_family(int mode) { return mode == R1_MODE_TP || r1_mode_is_batch(mode); }      // few long-lived waves, one guided queue
// sub-queues, the full grid and the cooperative tail: the latency build, and a pass on a small scene (on a big one a pass runs as TP without landing)
constexpr bool r1_runs_as_latency(int mode, bool big) { return mode == R1_MODE_LAT || (r1_mode_is_pass(mode) && !big); }
// tiles resolved inside the kernel (R1_LAND): the throughput builds of the tree's product kernel.  The synchronous frame keeps the
// resolve launch (1.276 against 1.077 ms on the device with its tiles summed at wave exit, i.e. at the end of the frame's critical path;
// profiles/r04/land_sync_frame.txt), and so does the exhaustive sweep (its loop pays 14 % for the bookkeeping, 16.6 against 19.2 Grays/s)
constexpr bool r1_build_lands(int variant, bool stats, int mode) { return variant == R1_V_TREE && !stats && r1_mode_is_tp_family(mode); }

// The root step of the tree walk tests its leaf sphere by sphere (r1_hit_tree.hpp leaf_root) instead of through leaf_quad's slot loop: one choice
// per build, taken where the build keeps its waves per SIMD, gains no scratch and no more than a handful of spilled-SGPR lane moves with it
// (tools/kernel_meta.py; profiles/r19/kernel_meta_*.txt).  The path builds hold the camera table's scalars across the walk and
// spill 16-36 more lane moves with the leaf's spheres in scalar registers as well; the small PIXEL build 12 more.
constexpr bool r1_root_by_slots(bool stats, bool big, int mode)
{
    return stats || (mode != R1_MODE_PATH && !(mode == R1_MODE_PIXEL && !big));
}

// A build of the trace body: the template arguments of the kernel that runs (r1_trace_body<variant, stats, big, mode>).
struct R1Build
{
    int variant; // a base variant: R1_V_REFERENCE, R1_V_SWEEP, R1_V_TREE or R1_V_GRID
    bool stats, big;
    int mode;
};

// What each translation unit instantiates (r1_trace_tu.inc walks its list to launch and to ask for occupancy), X(variant, stats, big, mode).
// The grid's PIXEL mode exists for big scenes only (the small-scene build would spill; r1_frame.cpp big_scene sends small scenes there), the
// latency mode for small scenes only, the diagnostic builds in the mode a synchronous frame runs in, the reference form as TP and PASS.
#define R1_BUILDS_TREE_SMALL(X)                 \
    X(R1_V_TREE, false, false, R1_MODE_TP)      \
    X(R1_V_TREE, false, false, R1_MODE_LAT)     \
    X(R1_V_TREE, false, false, R1_MODE_PIXEL)   \
    X(R1_V_TREE, false, false, R1_MODE_BATCH)   \
    X(R1_V_TREE, false, false, R1_MODE_PASS)    \
    X(R1_V_TREE, false, false, R1_MODE_PATH)    \
    X(R1_V_TREE, false, false, R1_MODE_LISTED)  \
    X(R1_V_TREE, true, false, R1_MODE_LAT)
#define R1_BUILDS_TREE_BIG(X)                  \
    X(R1_V_TREE, false, true, R1_MODE_TP)      \
    X(R1_V_TREE, false, true, R1_MODE_PIXEL)   \
    X(R1_V_TREE, false, true, R1_MODE_BATCH)   \
    X(R1_V_TREE, false, true, R1_MODE_PASS)    \
    X(R1_V_TREE, false, true, R1_MODE_PATH)    \
    X(R1_V_TREE, false, true, R1_MODE_LISTED)  \
    X(R1_V_TREE, true, true, R1_MODE_TP)
#define R1_BUILDS_SWEEP_SMALL(X)                   \
    X(R1_V_SWEEP, false, false, R1_MODE_TP)        \
    X(R1_V_SWEEP, false, false, R1_MODE_LAT)       \
    X(R1_V_SWEEP, false, false, R1_MODE_PIXEL)     \
    X(R1_V_SWEEP, false, false, R1_MODE_BATCH)     \
    X(R1_V_SWEEP, false, false, R1_MODE_PASS)      \
    X(R1_V_SWEEP, false, false, R1_MODE_PATH)      \
    X(R1_V_SWEEP, false, false, R1_MODE_LISTED)    \
    X(R1_V_SWEEP, true, false, R1_MODE_LAT)        \
    X(R1_V_REFERENCE, false, false, R1_MODE_TP)    \
    X(R1_V_REFERENCE, false, false, R1_MODE_PASS)
#define R1_BUILDS_SWEEP_BIG(X) /* (no diagnostic build of the LDS-tiled sweep) */  \
    X(R1_V_SWEEP, false, true, R1_MODE_TP)                                         \
    X(R1_V_SWEEP, false, true, R1_MODE_PIXEL)                                      \
    X(R1_V_SWEEP, false, true, R1_MODE_BATCH)                                      \
    X(R1_V_SWEEP, false, true, R1_MODE_PASS)                                       \
    X(R1_V_SWEEP, false, true, R1_MODE_PATH)                                       \
    X(R1_V_SWEEP, false, true, R1_MODE_LISTED)                                     \
    X(R1_V_REFERENCE, false, true, R1_MODE_TP)                                     \
    X(R1_V_REFERENCE, false, true, R1_MODE_PASS)
#define R1_BUILDS_GRID_SMALL(X)                 \
    X(R1_V_GRID, false, false, R1_MODE_TP)      \
    X(R1_V_GRID, false, false, R1_MODE_LAT)     \
    X(R1_V_GRID, false, false, R1_MODE_BATCH)   \
    X(R1_V_GRID, false, false, R1_MODE_PASS)    \
    X(R1_V_GRID, false, false, R1_MODE_PATH)    \
    X(R1_V_GRID, false, false, R1_MODE_LISTED)  \
    X(R1_V_GRID, true, false, R1_MODE_LAT)
#define R1_BUILDS_GRID_BIG(X)                  \
    X(R1_V_GRID, false, true, R1_MODE_TP)      \
    X(R1_V_GRID, false, true, R1_MODE_PIXEL)   \
    X(R1_V_GRID, false, true, R1_MODE_BATCH)   \
    X(R1_V_GRID, false, true, R1_MODE_PASS)    \
    X(R1_V_GRID, false, true, R1_MODE_PATH)    \
    X(R1_V_GRID, false, true, R1_MODE_LISTED)  \
    X(R1_V_GRID, true, true, R1_MODE_TP)
#define R1_BUILDS_ALL(X) R1_BUILDS_TREE_SMALL(X) R1_BUILDS_TREE_BIG(X) R1_BUILDS_SWEEP_SMALL(X) R1_BUILDS_SWEEP_BIG(X) R1_BUILDS_GRID_SMALL(X) R1_BUILDS_GRID_BIG(X)

constexpr bool r1_same_build(const R1Build &a, int variant, bool stats, bool big, int mode)
{
    return a.variant == variant && a.stats == stats && a.big == big && a.mode == mode;
}

// is the build in the library?  Folded over the lists above: the answer and the instantiations cannot disagree
constexpr bool r1_build_exists(const R1Build &b)
{
#define R1_X(V, S, B, M) || r1_same_build(b, V, S, B, M)
    return false R1_BUILDS_ALL(R1_X);
#undef R1_X
}

// The build that runs for (variant, big) when the caller would like mode `want`; false: there is none, the call is refused.
//   the reference form exists as TP and PASS only: every single-frame wish runs as TP;
//   a diagnostic build follows the synchronous frame — LAT, big scenes TP — and serves single frames only; the LDS-tiled sweep (big scenes) has
//   none, its product build runs instead;
//   big scenes have no latency build: LAT runs as TP;
//   the grid's PIXEL mode runs through its big-scene kernel only.
constexpr bool r1_pick(int variant, bool big, int want, R1Build &b)
{
    if (variant < R1_V_REFERENCE || variant > R1_V_GRID_STATS || variant == R1_V_WAVEFRONT || want < 0 || want >= R1_MODES)
        return false;
    const bool single = want == R1_MODE_TP || want == R1_MODE_LAT || want == R1_MODE_PIXEL;
    b.variant = r1_base_variant(variant), b.stats = r1_is_stats(variant), b.big = big, b.mode = want;
    if (b.stats)
    {
        if (!single)
            return false;
        b.mode = big ? R1_MODE_TP : R1_MODE_LAT;
        if (b.variant == R1_V_SWEEP && big)
            b.stats = false;
    }
    else if (variant == R1_V_REFERENCE)
    {
        if (!single && want != R1_MODE_PASS)
            return false;
        b.mode = single ? R1_MODE_TP : R1_MODE_PASS;
    }
    else
    {
        if (want == R1_MODE_LAT && big)
            b.mode = R1_MODE_TP;
        if (variant == R1_V_GRID && want == R1_MODE_PIXEL && !big)
            return false;
    }
    return true;
}

// every pick is a build of the library (the other direction — every build is some call's pick — is tests/test_builds_host.py's)
constexpr bool r1_picks_exist()
{
    for (int variant = 0; variant <= 9; ++variant)
        for (int big = 0; big < 2; ++big)
            for (int want = 0; want < R1_MODES; ++want)
            {
                R1Build b = {0, false, false, 0};
                if (r1_pick(variant, big != 0, want, b) && !r1_build_exists(b))
                    return false;
            }
    return true;
}
static_assert(r1_picks_exist(), "r1_pick chose a build that no translation unit instantiates (R1_BUILDS_*)");

#endif
