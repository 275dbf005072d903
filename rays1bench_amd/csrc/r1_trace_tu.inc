// r1_trace_tu.inc — body of a translation unit that instantiates r1_trace_kernel for ONE family.  The including file defines
//   R1_TU_NAME   tree_small | tree_big | sweep_small | sweep_big
//   R1_TU_BIG    true / false
//   R1_TU_TREE   1: variants 4 (product) and 5 (diagnostic build); 0: variants 2 (grouped sweep), 3 (its diagnostic build, small scenes), 1 (reference form)
//   R1_TU_GRID   1: variants 7 (uniform grid) and 8 (its diagnostic build); R1_TU_TREE is 0 then
#ifndef R1_TU_GRID
#define R1_TU_GRID 0
#endif
#include "r1_trace.hpp"

#define R1_CAT2(a, b, c) a##b##c
#define R1_CAT(a, b, c) R1_CAT2(a, b, c)

// S = diagnostic build, M = mode (0 frames in flight, 1 latency, 2 pixel, 3 frame batches; 4 progressive passes: R1_TU_PASS below; 5 camera paths: R1_TU_PATH_VARIANT); calls X(V, S, M)
// for the instance that is built
#if R1_TU_GRID
// (PIXEL mode: the big-scene build only, r1_capi.cpp; r1_launch_trace refuses the small one)
#define R1_TU_DISPATCH(X)                                                                                              \
    if (variant == 8)                                                                                                  \
        X(7, true, (R1_TU_BIG ? 0 : 1));                                                                               \
    else if (mode == 2 && R1_TU_BIG)                                                                                   \
        X(7, false, (R1_TU_BIG ? 2 : 0));                                                                              \
    else if (mode == 1 && !R1_TU_BIG)                                                                                  \
        X(7, false, 1);                                                                                                \
    else if (batch)                                                                                                    \
        X(7, false, 3);                                                                                                \
    else                                                                                                               \
        X(7, false, 0);
#elif R1_TU_TREE
#define R1_TU_DISPATCH(X)                                                                                              \
    if (variant == 5)                                                                                                  \
        X(4, true, (R1_TU_BIG ? 0 : 1));                                                                               \
    else if (mode == 2)                                                                                                \
        X(4, false, 2);                                                                                                \
    else if (mode == 1 && !R1_TU_BIG)                                                                                  \
        X(4, false, (R1_TU_BIG ? 0 : 1));                                                                              \
    else if (batch)                                                                                                    \
        X(4, false, 3);                                                                                                \
    else                                                                                                               \
        X(4, false, 0);
#elif R1_TU_BIG
#define R1_TU_DISPATCH(X)                                                                                              \
    if (variant == 1)                                                                                                  \
        X(1, false, 0);                                                                                                \
    else if (mode == 2)                                                                                                \
        X(2, false, 2);                                                                                                \
    else if (batch)                                                                                                    \
        X(2, false, 3);                                                                                                \
    else                                                                                                               \
        X(2, false, 0);
#else
#define R1_TU_DISPATCH(X)                                                                                              \
    if (variant == 1)                                                                                                  \
        X(1, false, 0);                                                                                                \
    else if (variant == 3)                                                                                             \
        X(2, true, 1);                                                                                                 \
    else if (mode == 2)                                                                                                \
        X(2, false, 2);                                                                                                \
    else if (mode == 1)                                                                                                \
        X(2, false, 1);                                                                                                \
    else if (batch)                                                                                                    \
        X(2, false, 3);                                                                                                \
    else                                                                                                               \
        X(2, false, 0);
#endif

#if R1_TU_GRID
#define R1_TU_KERNEL(V, S, M) r1_grid_kernel<S, R1_TU_BIG, M>
#else
#define R1_TU_KERNEL(V, S, M) r1_trace_kernel<V, S, R1_TU_BIG, M>
#endif

// progressive passes (MODE 4, r1_render_pass): r1_pass_kernel<V, big> for the family's product variants; calls X(V) for the instance that is built
#if R1_TU_GRID
#define R1_TU_PASS(X) X(7)
#elif R1_TU_TREE
#define R1_TU_PASS(X) X(4)
#else
#define R1_TU_PASS(X)                                                                                                  \
    if (variant == 1)                                                                                                  \
        X(1)                                                                                                           \
    else                                                                                                               \
        X(2)
#endif

// camera paths (MODE 5, r1_render_path_async): r1_path_kernel<V, big> for the family's batch variant; adaptive sampling (MODE 6,
// r1_render_adaptive): r1_adaptive_kernel<V, big> for the same variant
#if R1_TU_GRID
#define R1_TU_PATH_VARIANT 7
#elif R1_TU_TREE
#define R1_TU_PATH_VARIANT 4
#else
#define R1_TU_PATH_VARIANT 2
#endif

extern "C" hipError_t R1_CAT(r1_tu_, R1_TU_NAME, _launch)(const R1TraceArgs *args, int variant, int mode, int batch, int blocks, size_t dyn_lds, hipStream_t stream)
{
#define R1_GO(V, S, M) hipLaunchKernelGGL((R1_TU_KERNEL(V, S, M)), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args)
#define R1_GO_PASS(V) hipLaunchKernelGGL((r1_pass_kernel<V, R1_TU_BIG>), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);
    if (mode == 5)
    {
        if (variant != R1_TU_PATH_VARIANT || !batch)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL((r1_path_kernel<R1_TU_PATH_VARIANT, R1_TU_BIG>), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);
    }
    else if (mode == 6)
    {
        if (variant != R1_TU_PATH_VARIANT || !batch)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL((r1_adaptive_kernel<R1_TU_PATH_VARIANT, R1_TU_BIG>), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);
    }
    else if (mode == 4)
    {
        R1_TU_PASS(R1_GO_PASS)
    }
    else
    {
        R1_TU_DISPATCH(R1_GO)
    }
#undef R1_GO_PASS
#undef R1_GO
    return hipGetLastError();
}

extern "C" hipError_t R1_CAT(r1_tu_, R1_TU_NAME, _occupancy)(int variant, int mode, size_t dyn_lds, int *blocks_per_cu)
{
    const int batch = 0; // (the batch build of a kernel has the occupancy of its single-frame build)
#define R1_OCC(V, S, M) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, R1_TU_KERNEL(V, S, M), R1_BLOCK, dyn_lds)
#define R1_OCC_PASS(V) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, r1_pass_kernel<V, R1_TU_BIG>, R1_BLOCK, dyn_lds);
    if (mode == 4)
    {
        R1_TU_PASS(R1_OCC_PASS)
    }
    if (mode == 6)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, r1_adaptive_kernel<R1_TU_PATH_VARIANT, R1_TU_BIG>, R1_BLOCK, dyn_lds);
    R1_TU_DISPATCH(R1_OCC)
#undef R1_OCC_PASS
#undef R1_OCC
}
