// r1_trace.hpp — hand-written HIP for gfx950 (MI355X, wave64): the per-pixel/per-sample path-tracing hot path of rays1bench step13.
// This file: the persistent trace kernel (TraceWaves, r1_trace_body and its __global__ templates).  The device functions it is made
// of live in headers by subject, each of which compiles alone (tests/test_device_headers_host.py) and has internal linkage:
//   r1_dev_math.hpp   address-space typedefs, V3 and its operations, the xorshift32 streams, Path
//   r1_kargs.hpp      fresh_args / R1_FRESH_ARGS: the kernel's arguments read again where they are used
//   r1_hit_sweep.hpp  exact_test, exact_offer; sweep_reference, sweep_prefilter and its exact phase, cooperative_sweep
//   r1_hit_tree.hpp   bvh_box, leaf_quad, leaf_root, Trav, bvh_advance, sweep_bvh
//   r1_hit_grid.hpp   grid_trace
//   r1_sample.hpp     chunk_claim, fastdiv, start_ray, start_sample, Pixel, quantise_pixel, path_store / path_load
//   r1_shade.hpp      the attenuation stack (its words: r1_stack_words.h, shared with the host), shade_level
//   r1_land.hpp       tiles resolved inside the kernel: land_note ... land_exit
// Included by the translation units that instantiate the kernel, one per family, through r1_trace_tu.inc (r1_trace_tree_small.hip,
// r1_trace_tree_big.hip, r1_trace_sweep_small.hip, r1_trace_sweep_big.hip, r1_trace_grid_small.hip, r1_trace_grid_big.hip), so that an
// experiment on one family rebuilds one file and `make -j` builds the families side by side.  r1_aux_kernels.hip (wavefront variant), r1_close_kernels.hip
// (resolve, accumulate) and r1_query_kernels.hip (ray and path queries) include the subject headers they use, not this file.
// The includes below stand in the order the definitions had in one file.
//
// What it replaces (all in the reference's src/step13/):
//   render_tile's pixel x sample loop      rayweek1.cpp:722-782   -> r1_trace_kernel (r1_land.hpp land_resolve_tile) + r1_resolve_kernel
//   Camera::getRay / random_in_unit_disk   rayweek1.cpp:381-386 / :353-362   -> r1_sample.hpp start_ray
//   color() bounce recursion               rayweek1.cpp:515-536   -> flattened register loop (r1_trace_body, r1_shade.hpp shade_level)
//   Hitable::hit (AVX2 sweep + resolve)    rayweek1.cpp:152-339   -> sweep_prefilter / sweep_reference (r1_hit_sweep.hpp) / sweep_bvh (r1_hit_tree.hpp)
//   Lambertian/Metal/Dielectric::scatter   rayweek1.cpp:403-409 / :427-433 / :470-511   -> r1_shade.hpp shade_level over r1_scatter.h
//   TileRenderScheduler (atomic tile pop)  rayweek1.cpp:785-842   -> persistent waves + global sample queue (r1_trace_body)
//
// Design (DESIGN.md §4 has the long form and the measurements):
//   * one LANE per live path; a wave keeps its 64 lanes busy by refilling finished lanes from a
//     global sample queue (guided chunks of R1_CHUNK_MIN..R1_CHUNK samples per atomic), so the
//     bounce-count divergence of color() (1..51 rays per sample) costs no lanes;
//   * three interchangeable hit tests, bit-identical results (include/rays1.h R1_VARIANT_*): the
//     reference's form over every sphere (sweep_reference), the grouped exhaustive sweep
//     (sweep_prefilter, next two points) and a per-lane walk of a conservative box tree in front
//     of the reference's per-sphere test (sweep_bvh; the reference has no such structure);
//   * exhaustive sweep: the sphere table is wave-uniform: it is read with SCALAR loads (two alternating sets of
//     s_load_dwordx16) and fed to the VALU as SGPR-pair operands of v_pk_fma_f32 — two spheres
//     per instruction, no LDS round trip, no VGPRs.  (Scenes above 1023 spheres stream the table
//     through LDS tiles instead: the scalar cache cannot sustain a 3 MB stream.);
//   * pass 1 is a conservative prefilter, 7 FMA + 1 compare per ray-sphere test (11 in the
//     reference's form) = 4.5 VALU instructions per sphere per 64 rays; flagged (ray, sphere)
//     pairs of the whole wave are compacted in LDS and re-tested 64 at a time in the reference's
//     exact arithmetic, so results are bit-identical to the reference's candidate rule (sign bit
//     of its discriminant) and closest-hit rule (strict compares, lowest index on ties);
//   * attenuation is applied in the reference's right-nested order a0*(a1*(...*sky)) by
//     keeping the hit indices of a path in a packed per-lane LDS stack;
//   * per-sample radiance goes to HBM (16 B/sample) and a second kernel sums the samples of
//     a pixel in sample order — the reference's order — which keeps pixels deterministic.
//
// Arithmetic contract: identical operation order to oracle/r1_oracle.c (which is pinned to
// the reference bit-for-bit); no implicit FMA contraction; IEEE sqrt and division.  The only
// known difference is powf(x,5) (glibc, <1 ulp) vs an exactly rounded x^5 here.
#ifndef R1_TRACE_HPP
#define R1_TRACE_HPP

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "r1_device.h"
#include "r1_dev_math.hpp"
#include "r1_kargs.hpp"
#include "r1_hit_sweep.hpp"
#include "r1_hit_tree.hpp"
#include "r1_hit_grid.hpp"
#include "r1_sample.hpp"
#include "r1_shade.hpp"
#include "r1_land.hpp"

#pragma clang fp contract(off)

// ============================================================================================
// The trace kernel.  Persistent: grid = CUs x blocks/CU, every wave loops until the global
// sample queue is empty and its own lanes have finished their paths.
// ============================================================================================
// STATS = diagnostic build (variant R1_VARIANT_STATS): same results, plus per-phase cycle and
// utilisation counters in A.stats; never used by the product path.
// Waves per SIMD the register allocator must leave room for (second __launch_bounds__ argument): the
// product kernels are sized by their LDS (tree: 6 workgroups per CU with a 128-node table — 10 KB attenuation stack + 8 KB
// traversal stack + 8 KB nodes; exhaustive sweep: 5), so their VGPR count has to stay under 512 / 6 -> 80 and 512 / 5 -> 96.
// The big-scene tree kernel waits for node fetches from L2, not for the VALU: it is built for 8 waves per SIMD (<= 64 VGPRs,
// which it meets without the spare sample, and <= 96 SGPRs — at its natural 106 the 800 SGPRs of a SIMD hold seven waves):
// 13.1 -> 14.4 Grays/s on 100 004 spheres.
// (round 3: the small-scene tree kernels for frames in flight, R1_MODE_TP / _BATCH, run SEVEN workgroups per CU — their LDS footprint is 22 KB with
// R1_STACK_LDS_WORDS_TP — so they are built for 7 waves per SIMD: <= 73 VGPRs, which the kernel meets at 69, and <= 96 SGPRs)
template <int VARIANT, bool STATS, bool BIG, int MODE>
struct TraceWaves
{
#ifndef R1_TREE_WAVES_TP
#define R1_TREE_WAVES_TP 7
#endif
#ifndef R1_TREE_WAVES_LAT
#define R1_TREE_WAVES_LAT 6 // (the synchronous build: 67 VGPRs, seven workgroups per CU at run time; built for eight — 64 VGPRs, two words of the
                            //  LDS stack less — it spills and is no faster: profiles/r04/retune_after_fresh_args.txt)
#endif
    // (the grid's PIXEL-mode build — big-scene kernel only — is built for four waves: at eight it keeps a scratch slot for its SGPR spills)
    static constexpr int value = STATS ? 1 : (VARIANT == R1_V_GRID && MODE == R1_MODE_PIXEL) ? 4 : ((r1_is_tree(VARIANT) || r1_is_grid(VARIANT)) ? (BIG ? 8 : (r1_mode_is_tp_family(MODE) ? R1_TREE_WAVES_TP : R1_TREE_WAVES_LAT)) : (VARIANT == R1_V_SWEEP && !BIG ? 5 : 1));
};

// MODE: one of R1_MODE_* (r1_builds.h names the seven and says what each is; which (VARIANT, STATS, BIG, MODE) are built: R1_BUILDS_* there).
// The latency build (r1_runs_as_latency: R1_MODE_LAT, and a pass on a small scene) compiles in the sub-queues and the cooperative tail; the
// throughput builds (r1_mode_is_tp_family: frames in flight, few long-lived waves per frame) leave them out: they cost them registers and
// bring them nothing.  A pass on a big scene runs as R1_MODE_TP without landing; r1_accum_kernel / r1_adapt_accum_kernel sum a pass's records.
// (the body of the kernel; r1_trace_kernel and, for the uniform grid, r1_grid_kernel below are its __global__ instances; r1_pass_kernel,
// r1_path_kernel and r1_adaptive_kernel those of R1_MODE_PASS, _PATH and _LISTED)
// FLAT: what the walk knows of the tree's flat axis before it looks (r1_hit_tree.hpp bvh_advance; R1_FLAT_ASK: nothing, every kernel r1_pick reaches)
// REGION: a pass over a window of the frame (r1_sample.hpp start_sample, the one place that reads it; r1_region_kernel below)
template <int VARIANT, bool STATS, bool BIG, int MODE, int FLAT = R1_FLAT_ASK, bool REGION = false>
__device__ __forceinline__ void r1_trace_body(const R1TraceArgs A)
{
    static_assert(!REGION || MODE == R1_MODE_PASS, "a region is traced as a pass");
    constexpr bool LISTED = MODE == R1_MODE_LISTED, PASS = r1_mode_is_pass(MODE);
    constexpr bool CPATH = MODE == R1_MODE_PATH, BATCH = r1_mode_is_batch(MODE); // (a path's frames each have a camera of their own, start_sample)
    constexpr bool LAT = r1_runs_as_latency(MODE, BIG), PIX = MODE == R1_MODE_PIXEL;
    // tiles resolved inside the kernel: the throughput builds of the tree kernels; a launch through them is a landing
    // launch (r1_launch_trace checks)
    constexpr bool LAND = r1_build_lands(VARIANT, STATS, MODE);
    const uint32_t tb = blockIdx.x, n_tb = gridDim.x;
    // LAND: this workgroup's XCD (HW_REG_XCC_ID), the tiles of the launch
    const uint32_t xcd = LAND ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(xcc_id() & (R1_LAND_MAX_XCD - 1u))) : 0u;
    const uint32_t land_tiles = LAND ? A.total_samples / A.full : 0u;
#ifdef R1_LAND_DEBUG
    if (LAND && threadIdx.x == 0 && blockIdx.x < 8)
        A.queue[R1_HEAD_WORDS * (R1_HEAD_DEBUG + blockIdx.x % R1_HEAD_DEBUG_COUNT)] = 0x1000u | (xcc_id() << 4) | xcd; // (tools/land_debug.py)
#endif
    if (LAND && blockIdx.x == 0) // the cursors / wave counts the launch BEFORE this one used: nobody touches them during this launch
        for (uint32_t i = threadIdx.x; i < R1_HEAD_WORDS * A.land.clear_count; i += R1_BLOCK)
            A.land.clear_heads[i] = 0u;
    typedef typename IdxType<BIG>::type IDX;
    unsigned long long wstat[18];
    if (STATS)
    {
        for (int i = 0; i < 18; ++i)
            wstat[i] = 0;
        wstat[14] = __builtin_readcyclecounter();
    }
    // STATS builds: optional per-wave log {start, queue-empty, end (100 MHz real-time clock), iterations};
    // its address is handed over behind the published counters, r1_device.h R1_CNT_WAVE_LOG (tools/wave_timeline.py)
    unsigned long long *wave_log = nullptr;
    unsigned long long log_start = 0, log_exhausted = 0;
    if (STATS && A.stats)
    {
        wave_log = (unsigned long long *)A.stats[R1_STATS_WORDS]; // (the word behind the published slots)
        log_start = __builtin_amdgcn_s_memrealtime();
    }
    // words of the attenuation stack in LDS (the rest of a deep path's entries live in the global workspace)
    constexpr int LW = (r1_is_tree(VARIANT) || r1_is_grid(VARIANT)) ? ((r1_mode_is_tp_family(MODE) && !STATS) ? R1_STACK_LDS_WORDS_TP : R1_STACK_LDS_WORDS) : R1_STACK_WORDS;
    __shared__ uint32_t s_stack[BIG ? 1 : LW * R1_BLOCK];
    __shared__ uint32_t s_cand[VARIANT == R1_V_SWEEP ? (BIG ? R1_CAND_CAP : R1_BIT_WORDS) * R1_BLOCK : 1];
    __shared__ IDX s_pairs[VARIANT == R1_V_SWEEP ? (R1_BLOCK / 64) * PairBits<IDX>::cap : 1];
    // R1_VARIANT_BVH: traversal stack [tree depth][thread], sized at launch (dynamic LDS)
    extern __shared__ uint32_t s_trav[];
    const uint32_t gstride = n_tb * R1_BLOCK, gtid = tb * R1_BLOCK + threadIdx.x;
    __shared__ unsigned long long s_best[VARIANT == R1_V_SWEEP ? R1_BLOCK : 1];
    __shared__ f4 s_tile[BIG && VARIANT == R1_V_SWEEP ? 2 * R1_TILE_F4 : 1];

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;

    // Tree kernels, small scenes (!BIG: at most R1_NODES_LDS_MAX nodes, r1_frame.cpp big_scene): the workgroup keeps its own copy of
    // the node table in LDS, behind the traversal stack.  A node visit is four dependent 16-byte loads per lane; LDS
    // answers sooner than the vector L1, and the table no longer competes with the sphere tables for its 32 KB:
    // 26.9 -> 29.3 Grays/s, one synchronous frame 1.34 -> 1.17 ms (large scene, 128 nodes = 8 KB).
    constexpr bool LN = VARIANT == R1_V_TREE && !BIG;
    typedef typename IdxType<!LN>::type TS; // traversal-stack entry: uint16_t for the small-scene tree kernels, else uint32_t
    const size_t trav_words = VARIANT == R1_V_TREE ? (size_t)A.bvh_depth * R1_BLOCK * sizeof(TS) / 4 : 0; // (bvh_depth x 256 entries: a multiple of 16 bytes either way)
    // R1_VARIANT_GRID: the fallback's traversal stack (32-bit entries: the tree walk of bvh_advance from the table in global memory), then
    // (small scenes) the workgroup's copy of the grid's 16-bit cell table and ids
    const size_t gtrav_words = VARIANT == R1_V_GRID ? (size_t)A.bvh_depth * R1_BLOCK : 0;
    const uint16_t *ltab = (const uint16_t *)(s_trav + gtrav_words);
    // (this staging and the node table's below stay inline: moved into the query kernels' stage_grid / stage_nodes they change these kernels' code)
    if (VARIANT == R1_V_GRID && !BIG)
    {
        float4 *dst = (float4 *)(s_trav + gtrav_words);
        const R1GridCArgs *ga = (const R1GridCArgs *)(uintptr_t)A.grid;
        const float4 *src = (const float4 *)(const r1_gu32 *)ga->tab;
        const uint32_t n16 = ga->lds_bytes / 16u;
        for (uint32_t i = (uint32_t)tid; i < n16; i += R1_BLOCK)
            dst[i] = src[i];
        __syncthreads();
    }
    const float4 *lnodes = (const float4 *)(s_trav + trav_words);
    // (big scenes: A.bvh_lds_f4 covers the first nodes of the breadth-first top of the tree only)
    const uint32_t top = LN ? 0u : A.bvh_lds_f4 >> 2;
    if (VARIANT == R1_V_TREE && A.bvh_lds_f4)
    {
        float4 *dst = (float4 *)(s_trav + trav_words);
        for (uint32_t i = (uint32_t)tid; i < A.bvh_lds_f4; i += R1_BLOCK)
        {
            float4 q = A.scene.bvh_nodes[i];
            if (LN && (i & 3u) == 3u) // {A K child0 child1}: the small-scene kernels walk with 16-bit child references
                q.z = __uint_as_float(r1_ref16(__float_as_uint(q.z))), q.w = __uint_as_float(r1_ref16(__float_as_uint(q.w)));
            dst[i] = q;
        }
        // node 0's K slot (0 for these trees: K is part of the half extents) carries the root step's code, see bvh_advance (written by
        // the thread that copied that row: program order; outside the loop, where the test made the compiler peel and unroll the copy)
        // (bit 2 of the code: a flat tree, whose y slab sits in node 1's pad slots — A again and a zero in the table, and the node loop fetches
        //  neither from LDS; r1_bvh.cpp "flat axis", a flat tree has at least two nodes)
        if (LN && tid == 3)
            ((float *)dst)[13] = __uint_as_float(A.scene.bvh_root_leaf | (A.scene.bvh_flat_e >= 0.0f ? 4u : 0u));
        if (LN && tid == 7 && A.scene.bvh_flat_e >= 0.0f)
            ((float *)dst)[28] = A.scene.bvh_flat_m, ((float *)dst)[29] = A.scene.bvh_flat_e;
        __syncthreads();
    }

    Path p;
    p.o = mk(0, 0, 0), p.d = mk(0, 0, 0);
    p.s_scalar = p.s0 = p.s1 = p.s2 = 1;
    p.k = 0, p.depth = 0, p.sp = 0;
    bool alive = false;
    Pixel px; // PIXEL mode: the pixel this lane owns
    px.acc = mk(0, 0, 0), px.xy = 0, px.off = 0, px.s = (uint32_t)A.spp;
    Trav tv; // tree kernels: this lane's walk (carried over outer iterations, see bvh_advance)
    trav_start(tv);
    tv.cur = R1_BVH_DONE;
    unsigned long long lane_rays = 0;
    // Frames in flight (R1_MODE_TP; tree kernels and the small-scene exhaustive sweep, 18.25 -> 19.0 Grays/s at 96 VGPRs, its
    // limit for five waves per SIMD): every lane keeps ONE prepared sample (its primary ray and stream states,
    // 11 registers) next to the path it is tracing.  A lane whose path ends takes its own spare, and spares are generated
    // for all lanes that lack one at once — when a lane has died without one, or R1_SPARE_MIN lanes lack one — instead of
    // for the ~36 % of the lanes that died in this iteration: the ~200 instructions of hashing, lens disk and camera ray
    // run every second iteration at ~60 % of the lanes.  29.4 -> 30.5 Grays/s (thresholds 20 / 32 / 44 / never by count:
    // 30.2 / 30.5 / 30.6 / 30.4).  Not for a synchronous frame: what the lanes hold when the queue runs dry is the
    // frame's tail (1.17 -> 1.23 ms with spares).
#ifndef R1_SPARE_MIN
#define R1_SPARE_MIN 40u
#endif
    constexpr bool SPARE = !BIG && (VARIANT == R1_V_TREE || VARIANT == R1_V_SWEEP || VARIANT == R1_V_GRID) && r1_mode_is_tp_family(MODE); // (big scenes: the registers buy an eighth wave instead)
    Path spare = p;
    bool has_spare = false;
    // The bookkeeping around the loop's arithmetic, trimmed in the builds that both land their tiles and keep a spare: the
    // frames-in-flight tree kernels <4,false,false,TP / BATCH / PATH>.  Every other build keeps its code to the instruction.
    constexpr bool TRIM = LAND && SPARE;
#ifndef R1_TRIM_VOTES
#define R1_TRIM_VOTES 1 // the wave votes (0: as in every other build; `make tuning EXTRA=-DR1_TRIM_VOTES=0` measures the step alone)
#endif
#ifndef R1_TRIM_WALK
#define R1_TRIM_WALK 1 // the walk's state at the end of a sample and at the hand-over of the spare
#endif
    constexpr bool TRIM_VOTES = TRIM && R1_TRIM_VOTES, TRIM_WALK = TRIM && R1_TRIM_WALK;
    // Votes.  __ballot turns a condition the compiler holds as a lane mask into v_cndmask 0,1 + v_cmp_ne, and so does the ballot builtin on a
    // bool that is carried around the loop; on a comparison it is the one v_cmp that writes the mask.  The trimmed builds vote on comparisons
    // of per-lane words, and combine the masks on the scalar pipe.
    // Between the end of one iteration and the next one's walk a lane of a tree kernel is dead exactly when its walk is marked complete: a lane
    // that ends its sample leaves tv.cur at R1_BVH_DONE (it was `ready`), trav_start and a carried walk leave it elsewhere.  The trimmed builds
    // read `alive` from that word there, so that no lane mask lives across the refill loop (the mask and its complement were parked in four
    // lanes of the spill register in every iteration, and fetched back).
#define R1_DEAD (TRIM_VOTES ? tv.cur == R1_BVH_DONE : !alive)
#define R1_VOTE(c) (TRIM_VOTES ? (unsigned long long)__builtin_amdgcn_ballot_w64(c) : (unsigned long long)__ballot(c))

    // wave-uniform queue state.  Chunks shrink as the queue drains (guided self-scheduling):
    // a wave asks for ~1/(2*waves) of what it last saw remaining, between R1_CHUNK_MIN and
    // R1_CHUNK samples, so that the last waves to finish hold little work.
    // LAND: chunks come from the cursor of this XCD (head R1_HEAD_XCD + xcd, r1_land.hpp); q_next / q_end are sample slots of the launch either way
    uint32_t q_next = 0, q_end = 0;
    const uint32_t q_total = A.total_samples;
    uint32_t q_remaining = q_total;
    const uint32_t n_waves2 = 2u * n_tb * (R1_BLOCK / 64);
    uint32_t *const q_head = LAND ? A.queue + R1_HEAD_WORDS * (R1_HEAD_XCD + xcd) : A.queue;
    // tiles an XCD claims at a time.  A synchronous frame has the whole chip on 64-sample chunks: an XCD is through a tile in ~8 us, and
    // the ~5 us its cursor is closed while the next claim is installed would be most of that (1.65 ms per frame with one tile per claim)
    constexpr uint32_t LAND_GROUP = LAT ? 8u : 1u;
    __shared__ uint32_t s_land[LAND ? (R1_BLOCK / 64) * R1_LAND_ROW : 1];
#define row (s_land + (LAND ? (threadIdx.x >> 6) * R1_LAND_ROW : 0u)) /* this wave's row (see land_count); recomputed where it is used: one register less around the loop */
    if (LAND && lane < 8)
        row[lane] = (lane == 0 || lane == 2) ? 0xFFFFFFFFu : 0u;
    bool exhausted = false;
    // sub-queue this wave pulls from (A.nq > 1), wave-uniform
    // (workgroups b .. b + 7 sit on the eight XCDs and share their sub-queues, so every sub-queue is served from
    // every XCD: the XCDs of one chip ran this kernel up to 20 % apart in speed, tools/wave_timeline.py)
    const uint32_t home = LAT && A.nq > 1 ? __builtin_amdgcn_readfirstlane(((tb >> 3) * (R1_BLOCK / 64) + (threadIdx.x >> 6)) % A.nq) : 0u;

    for (;;)
    {
        // ---- refill finished lanes from the wave's chunk of the global sample queue ----
        if (STATS)
            wstat[15] = __builtin_readcyclecounter();
        if (PIX && !alive && px.s < (uint32_t)A.spp)
        {
            // the next sample of the pixel in hand: no queue, no index arithmetic
            start_ray(A, A.cam, p, (int)(px.xy & 0xFFFFu), (int)(px.xy >> 16), px.s, A.seed);
            alive = true;
            if (VARIANT == R1_V_TREE)
                trav_start(tv);
        }
        if (SPARE && R1_DEAD && has_spare)
        {
            p.o = spare.o, p.d = spare.d, p.s_scalar = spare.s_scalar, p.s0 = spare.s0, p.s1 = spare.s1, p.s2 = spare.s2, p.k = spare.k;
            p.depth = 0, p.sp = 0;
            alive = true, has_spare = false;
            if (TRIM_WALK)
                tv.cur = 0u; // (the rest of trav_start is in place since the lane's last sample ended, see below)
            else
                trav_start(tv);
        }
        unsigned long long need = R1_VOTE(R1_DEAD);
        if (SPARE)
        {
            const unsigned long long lack = R1_VOTE(!has_spare);
            // (the trimmed builds count the halves: the 64-bit count is compared as a 64-bit number, for which the scalar pipe has no instruction)
            const uint32_t n_lack = TRIM_VOTES ? (uint32_t)__builtin_popcount((uint32_t)lack) + (uint32_t)__builtin_popcount((uint32_t)(lack >> 32)) : (uint32_t)__popcll(lack);
            need = (need != 0ull || n_lack >= R1_SPARE_MIN) ? lack : 0ull;
        }
        while (need)
        {
            if (q_next == q_end)
            {
                if (exhausted)
                    break;
                uint32_t want, base = 0;
                if (LAT && A.nq > 1)
                {
                    // fixed chunks dealt round-robin to the sub-queues: chunk j of sub-queue `home` is chunk j nq + home
                    want = A.chunk_max;
                    if (lane == 0)
                        base = atomicAdd(A.queue + R1_HEAD_WORDS * (R1_HEAD_SUBQUEUE + home), 1u);
                    base = (__builtin_amdgcn_readfirstlane(base) * A.nq + home) * want;
                }
                else if (LAND)
                {
                    // guided as the single queue is: ~ what is left of the launch / (2 waves) — here: the tiles nobody has claimed yet
                    want = min(A.chunk_max, max(A.chunk_min, q_remaining / n_waves2));
                    base = q_total; // (exhausted unless a chunk is found)
                    for (;;)
                    {
                        unsigned long long old = 0;
                        if (lane == 0)
                            old = __hip_atomic_fetch_add((unsigned long long *)q_head, (unsigned long long)want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(old >> 32)); // group + 1; 0: none installed yet; ~0: none left
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)old);          // slots of the group handed out before this call
                        if (hi == 0xFFFFFFFFu)
                            break;
                        // a group = LAND_GROUP consecutive tiles claimed at once (the last one of a launch may be shorter)
                        const uint32_t g0 = (hi - 1u) * LAND_GROUP;
                        const uint32_t gs = hi != 0u ? min(LAND_GROUP, land_tiles - g0) * A.full : 0u;
                        const bool have = hi != 0u && lo < gs;
                        const bool advance = (hi == 0u && lo == 0u) || (have && lo + want >= gs); // exactly one wave per installed group (and per XCD at the start)
                        if (advance && lane == 0)
                        {
                            const uint32_t g = __hip_atomic_fetch_add(A.queue + R1_HEAD_WORDS * R1_HEAD_DISPENSER, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            unsigned long long nv = 0xFFFFFFFFull << 32;
                            if (g * LAND_GROUP < land_tiles)
                                nv = (unsigned long long)(g + 1u) << 32;
                            (void)__hip_atomic_exchange((unsigned long long *)q_head, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        if (have)
                        {
                            base = g0 * A.full + lo;
                            want = min(want, gs - lo);
                            q_remaining = (land_tiles - min(land_tiles, g0 + LAND_GROUP)) * A.full; // (the tiles behind this group: what the next call is guided by)
                            const uint32_t tl = fastdiv(lo, A.div_full); // the chunk's (first) tile within the group
                            if (lane == 0)
                            {
                                land_chunk(A, row, g0 + tl);
                                if (lo - tl * A.full + want > A.full) // (it runs on into the next tile: a chunk is at most one tile long)
                                    land_chunk(A, row, g0 + tl + 1u);
                            }
                            break;
                        }
                        if (advance)
                            continue; // installed the XCD's first tile myself: take from it
                        // a used-up tile (or none yet): the wave that installs the next one is a few atomics away
                        for (;;)
                        {
                            __builtin_amdgcn_s_sleep(16);
                            unsigned long long now = 0;
                            if (lane == 0)
                                now = __hip_atomic_load((unsigned long long *)q_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if ((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(now >> 32)) != hi)
                                break;
                        }
                    }
                }
                else
                {
                    want = min(A.chunk_max, max(A.chunk_min, q_remaining / n_waves2));
                    if (lane == 0)
                        base = atomicAdd(q_head, want);
                    base = __builtin_amdgcn_readfirstlane(base);
                }
                if (base >= q_total)
                {
                    // No stealing between sub-queues: chunks are dealt round-robin, so the sub-queues run dry together, the
                    // host gives every sub-queue home waves on every XCD, and looking for leftovers elsewhere costs more than
                    // it brings (nq failed atomics of ~1 us each at the end of every wave; a one-load scan of the heads
                    // spilled 50 SGPRs in this loop).
                    exhausted = true;
                    if (STATS)
                        log_exhausted = __builtin_amdgcn_s_memrealtime();
                    break;
                }
                q_next = base;
                q_end = min(base + want, q_total);
                if (!LAND)
                    q_remaining = q_total - q_end;
            }
            const uint32_t avail = q_end - q_next;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
            // (what start_sample reads: tiling, fast divisions, camera — fetched here, not carried around the loop)
            R1ArgWords FA_words;
            if (!PIX)
                fresh_args(FA_words);
            const R1TraceArgs &FA = PIX ? A : FA_words.a;
            // (Generating the primary rays in a separate full-width kernel and loading them here was
            // measured: 1.52 ms per frame against 1.28 — the extra launch per frame costs more overlap
            // between frames than the refill saves.)
            if (SPARE)
            {
                if (!has_spare && rank < avail)
                    has_spare = start_sample<BATCH, PASS, CPATH, LISTED, REGION>(FA, spare, q_next + rank); // false: void slot, ask again
            }
            else if (!alive && rank < avail)
            {
                if (PIX)
                {
                    alive = pixel_take(A, px, q_next + rank); // false: void slot, ask again
                    if (alive)
                        start_ray(A, A.cam, p, (int)(px.xy & 0xFFFFu), (int)(px.xy >> 16), 0u, A.seed);
                }
                else
                    alive = start_sample<BATCH, PASS, CPATH, LISTED, REGION>(FA, p, q_next + rank); // false: void slot, ask again
                if (VARIANT == R1_V_TREE && alive)
                    trav_start(tv);
            }
            q_next += min((uint32_t)__popcll(need), avail);
            need = SPARE ? R1_VOTE(!has_spare) : R1_VOTE(!alive);
        }
        if (SPARE && R1_DEAD && has_spare) // the lanes that had died without a spare start on the one they just got
        {
            p.o = spare.o, p.d = spare.d, p.s_scalar = spare.s_scalar, p.s0 = spare.s0, p.s1 = spare.s1, p.s2 = spare.s2, p.k = spare.k;
            p.depth = 0, p.sp = 0;
            alive = true, has_spare = false;
            if (TRIM_WALK)
                tv.cur = 0u;
            else
                trav_start(tv);
        }
        if (BIG && VARIANT == R1_V_SWEEP)
        {
            // lock-step workgroup: leave together (every wave must reach the sweep's barriers)
            if (!__syncthreads_or(alive ? 1 : 0))
                break;
        }
        else if (!TRIM_VOTES && __ballot(alive) == 0ull)
            break;
        // (the trimmed builds take the vote on `alive` once for the exit test, the priority votes and the walk, and vote on the depth word
        //  alone — one v_cmp each — masking with it on the scalar pipe; a dead lane's stale depth is masked off)
        if (TRIM_VOTES)
            alive = !R1_DEAD;
        const unsigned long long live_once = TRIM_VOTES ? (unsigned long long)__builtin_amdgcn_ballot_w64(!R1_DEAD) : 0ull;
        if (TRIM_VOTES && live_once == 0ull)
            break;
        // A frame's critical path is its longest bounce chain (up to 51 dependent sweeps, ~1/3 of
        // a 10-spp frame when the wave shares its SIMD with three others).  Waves that carry a
        // deep path ask for issue priority so that the chain finishes before the queue runs dry.
        if (TRIM_VOTES)
        {
            if ((__builtin_amdgcn_ballot_w64(p.depth >= 12) & live_once) == 0ull)
                __builtin_amdgcn_s_setprio(0);
            else if ((__builtin_amdgcn_ballot_w64(p.depth >= 36) & live_once) != 0ull)
                __builtin_amdgcn_s_setprio(3);
            else if ((__builtin_amdgcn_ballot_w64(p.depth >= 24) & live_once) != 0ull)
                __builtin_amdgcn_s_setprio(2);
            else
                __builtin_amdgcn_s_setprio(1);
        }
        else
        {
            // (one vote first: in most iterations no lane is 12 deep, and the two deeper votes are taken only behind it)
            if (__ballot(alive && p.depth >= 12) == 0ull)
                __builtin_amdgcn_s_setprio(0);
            else if (__ballot(alive && p.depth >= 36) != 0ull)
                __builtin_amdgcn_s_setprio(3);
            else if (__ballot(alive && p.depth >= 24) != 0ull)
                __builtin_amdgcn_s_setprio(2);
            else
                __builtin_amdgcn_s_setprio(1);
        }
        if (STATS)
        {
            wstat[4] += __builtin_readcyclecounter() - wstat[15];
            wstat[15] = __builtin_readcyclecounter();
            wstat[0] += 1;
            wstat[1] += (unsigned long long)__popcll(__ballot(alive));
        }

        // ---- one color() level: hit test for every live lane (rayweek1.cpp:519) ----
        float t_hit = FLT_MAX;
        int hit = -1;
        bool ready = alive; // lanes whose hit test is complete after this step (tree kernels: the others carry their walk over)
        const unsigned long long live_now = TRIM_VOTES ? live_once : __ballot(alive);
        if (LAT && !BIG && VARIANT != R1_V_REFERENCE && exhausted && (uint32_t)__popcll(live_now) <= A.coop_lanes)
        {
            cooperative_sweep(A.scene, live_now, p.o, p.d, t_hit, hit, lane); // the frame's tail: few paths left in this wave
            tv.cur = R1_BVH_DONE;                                            // (a walk in progress is simply dropped: this sweep is complete by itself)
        }
        else if (VARIANT == R1_V_REFERENCE)
        {
            if (alive)
                sweep_reference(A.scene, p.o, p.d, t_hit, hit);
        }
        else if (VARIANT == R1_V_TREE)
        {
            // while-while with carry-over
            R1_FRESH_ARGS(HA) // (table pointers, the tree's centre: fetched for the walk, free again after it)
            bvh_advance<STATS, true, LN, TS, r1_root_by_slots(STATS, BIG, MODE), R1_OFFER_FORM, FLAT>(HA.scene, p.o, p.d, tv, (TS *)s_trav, tid, (uint32_t)__popcll(live_now), wstat, lnodes, top);
            ready = alive && tv.cur == R1_BVH_DONE;
            if (tv.best_id != 0xFFFFFFFFu)
                t_hit = tv.best, hit = (int)tv.best_id;
        }
        else if (VARIANT == R1_V_GRID)
        {
            R1_FRESH_ARGS(HA) // (table pointers and the grid's geometry: fetched for the walk, free again after it)
            float best;
            uint32_t best_id;
            const bool fb = grid_trace<STATS, !BIG>(HA, (R1GridCArgs *)(uintptr_t)HA.grid, alive, p.o, p.d, best, best_id, ltab, tid, wstat);
            if (STATS)
                wstat[16] += fb ? 1ull : 0ull;
            if (__ballot(fb) != 0ull)
            {
                // fallback: the tree walk from scratch (from the root, table in global memory), exact for any origin; the
                // outliers' offer is kept (the tree presents them again: same offers, the index tie goes to the same sphere)
                Trav fv;
                trav_start(fv);
                fv.best = best, fv.best_id = best_id;
                if (!fb)
                    fv.cur = R1_BVH_DONE;
                // (grid launches carry scene.bvh_root_leaf = 0: the walk starts at the root, which it reads from global memory)
                bvh_advance<false, false, false, uint32_t, false, R1_OFFER_FORM_GRID>(HA.scene, p.o, p.d, fv, s_trav, tid, 64u, wstat, nullptr);
                best = fv.best, best_id = fv.best_id;
            }
            if (best_id != 0xFFFFFFFFu)
                t_hit = best, hit = (int)best_id;
        }
        else
        {
            R1ArgWords HA_words;
            if (!PIX)
                fresh_args(HA_words);
            const R1TraceArgs &HA = PIX ? A : HA_words.a;
            sweep_prefilter<STATS, IDX, BIG>(HA.scene, alive, p.o, p.d, t_hit, hit, s_cand, s_pairs, s_best, s_tile, tid, wstat);
        }
        if (STATS)
        {
            wstat[6] += __builtin_readcyclecounter() - wstat[15];
            wstat[15] = __builtin_readcyclecounter();
        }

        bool fin = false; // this lane's sample ended in this iteration
        // (material tables, the stack workspace, where the records go; PIXEL mode keeps the prologue's copy: its pixel_write indexes the
        //  arguments in a way that leaves the fresh copy in scratch)
        R1ArgWords SA_words;
        if (!PIX)
            fresh_args(SA_words);
        const R1TraceArgs &SA = PIX ? A : SA_words.a;
        if (ready)
        {
            V3 col;
            if (shade_level<BIG, LW>(SA, p, hit, t_hit, s_stack, gstride, gtid, tid, col))
            {
                if (PIX)
                {
                    px.acc = vadd(px.acc, col); // col += color(...), samples in order (rayweek1.cpp:762)
                    if (++px.s == (uint32_t)SA.spp)
                        pixel_write(SA, px);
                }
                else if (LAND)
                    SA.samples[p.k] = make_float4(col.x, col.y, col.z, __uint_as_float(path_rays(p) | SA.land_tag));
                else
                    SA.samples[p.k] = make_float4(col.x, col.y, col.z, __uint_as_float(path_rays(p)));
                if (!LAND)
                    lane_rays += path_rays(p); // (LAND: the waves that sum the tiles add up the records' counts)
                alive = false, fin = true;
            }
            else if (VARIANT == R1_V_TREE && !TRIM_WALK)
                trav_start(tv); // the scattered ray starts its walk at the root
            // (the trimmed builds reset the walk of every ready lane, ended samples included, and mark those complete again: the same
            //  constants for all of them — the other form kept the ended lanes' old offer alive through three register copies and three
            //  more where the branches join — and a hand-over only has to open the walk)
            if (TRIM_WALK)
            {
                trav_start(tv);
                if (fin)
                    tv.cur = R1_BVH_DONE;
            }
        }
        if (LAND && fin)
            land_count(SA, row, p.k);
        if (STATS)
            wstat[7] += __builtin_readcyclecounter() - wstat[15];
    }
    if (STATS)
    {
        // [0] wave iterations [1] alive lanes [2] candidate-loop trips [3] overflow lanes
        // [4] refill cycles [5] pass-1 cycles [6] candidate cycles [7] shade cycles [8] wave cycles
        // [9] candidates (all lanes)
        wstat[8] = __builtin_readcyclecounter() - wstat[14];
        unsigned long long c9 = wstat[9];
        for (int off = 32; off > 0; off >>= 1)
            c9 += __shfl_down(c9, off, 64);
        wstat[9] = c9;
        if (VARIANT == R1_V_TREE || VARIANT == R1_V_GRID)
        {
            // per-lane counters of sweep_bvh / grid_trace
            const int slots[5] = {2, 3, 5, 16, 17};
            for (int q = 0; q < 5; ++q)
            {
                unsigned long long c = wstat[slots[q]];
                for (int off = 32; off > 0; off >>= 1)
                    c += __shfl_down(c, off, 64);
                wstat[slots[q]] = c;
            }
        }
        if (lane == 0 && wave_log)
        {
            unsigned long long *rec = wave_log + 4 * (size_t)(blockIdx.x * (R1_BLOCK / 64) + (threadIdx.x >> 6));
            if (VARIANT == R1_V_GRID) // (the log lives in global memory: say so, no generic stores)
            {
                typedef unsigned long long __attribute__((address_space(1))) gu64;
                gu64 *grec = (gu64 *)(uintptr_t)rec;
                grec[0] = log_start, grec[1] = log_exhausted, grec[2] = __builtin_amdgcn_s_memrealtime(), grec[3] = wstat[0];
            }
            else
                rec[0] = log_start, rec[1] = log_exhausted, rec[2] = __builtin_amdgcn_s_memrealtime(), rec[3] = wstat[0];
        }
        if (lane == 0 && A.stats)
        {
            for (int i = 0; i < 10; ++i)
                atomicAdd(&A.stats[i], wstat[i]);
            atomicMax(&A.stats[10], wstat[8]);                      // longest wave (cycles)
            atomicMax(&A.stats[11], ~wstat[8]);                     // ~shortest wave
            atomicMax(&A.stats[12], (unsigned long long)__builtin_readcyclecounter());  // last wave end (this XCD's counter)
            atomicMax(&A.stats[13], ~wstat[14]);                    // ~first wave start
            if (VARIANT == R1_V_TREE || VARIANT == R1_V_GRID)
            {
                atomicAdd(&A.stats[14], wstat[16]);                 // tree: leaf trips summed over lanes (grid: fallback lanes)
                atomicAdd(&A.stats[15], wstat[17]);                 // tree: root steps (bvh_advance) summed over lanes
            }
        }
    }

    if (LAND)
        land_exit<(BIG && VARIANT == R1_V_TREE) ? 6 : R1_LAND_LOADS>(A, row, lane); // (the big-scene tree kernels are built for 64 registers)
#undef row
#undef R1_VOTE
#undef R1_DEAD
    // ray count: wave reduction, one atomic per wave (rayweek1.cpp:809-813)
    if (!LAND)
    {
        for (int off = 32; off > 0; off >>= 1)
            lane_rays += __shfl_down(lane_rays, off, 64);
        if (lane == 0 && lane_rays)
            atomicAdd(A.num_rays, lane_rays);
    }
}

template <int VARIANT, bool STATS, bool BIG, int MODE>
__global__ void __launch_bounds__(R1_BLOCK, (TraceWaves<VARIANT, STATS, BIG, MODE>::value)) r1_trace_kernel(const R1TraceArgs A)
{
    r1_trace_body<VARIANT, STATS, BIG, MODE>(A);
}

// R1_VARIANT_GRID: the same body under a name of its own (VARIANT 7)
template <bool STATS, bool BIG, int MODE>
__global__ void __launch_bounds__(R1_BLOCK, (TraceWaves<R1_V_GRID, STATS, BIG, MODE>::value)) r1_grid_kernel(const R1TraceArgs A)
{
    r1_trace_body<R1_V_GRID, STATS, BIG, MODE>(A);
}

// Flat box trees: the frames-in-flight tree kernels of small scenes, <R1_V_TREE, false, false, R1_MODE_TP / _BATCH>, with the
// walk's flat axis compiled in.  No build of r1_pick's: r1_launch_trace launches one in its sibling's place when the launch's tree is flat.
template <int MODE>
__global__ void __launch_bounds__(R1_BLOCK, (TraceWaves<R1_V_TREE, false, false, MODE>::value)) r1_flatwalk_kernel(const R1TraceArgs A)
{
    r1_trace_body<R1_V_TREE, false, false, MODE, R1_FLAT_YES>(A);
}

// Progressive passes (R1_MODE_PASS): the same body under a name of its own, for the tree, the exhaustive sweeps (grouped and reference form) and the grid
template <int VARIANT, bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, (TraceWaves<VARIANT, false, BIG, R1_MODE_PASS>::value)) r1_pass_kernel(const R1TraceArgs A)
{
    r1_trace_body<VARIANT, false, BIG, R1_MODE_PASS>(A);
}

// Region renders (r1_render_region*): the twin of every r1_pass_kernel, built for its sibling's waves.  No build of r1_pick's:
// r1_launch_trace launches one in its sibling's place when the pass carries a region.
template <int VARIANT, bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, (TraceWaves<VARIANT, false, BIG, R1_MODE_PASS>::value)) r1_region_kernel(const R1TraceArgs A)
{
    r1_trace_body<VARIANT, false, BIG, R1_MODE_PASS, R1_FLAT_ASK, true>(A);
}

// Adaptive sampling (R1_MODE_LISTED): the same body under a name of its own, for the tree, the grouped sweep and the grid; built for the
// waves of its r1_pass_kernel sibling
template <int VARIANT, bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, (TraceWaves<VARIANT, false, BIG, R1_MODE_PASS>::value)) r1_adaptive_kernel(const R1TraceArgs A)
{
    r1_trace_body<VARIANT, false, BIG, R1_MODE_LISTED>(A);
}

// Camera paths (R1_MODE_PATH): the same body under a name of its own, for the families that have a batch build: tree, grouped sweep, grid
template <int VARIANT, bool BIG>
__global__ void __launch_bounds__(R1_BLOCK, (TraceWaves<VARIANT, false, BIG, R1_MODE_PATH>::value)) r1_path_kernel(const R1TraceArgs A)
{
    r1_trace_body<VARIANT, false, BIG, R1_MODE_PATH>(A);
}

#endif // R1_TRACE_HPP
