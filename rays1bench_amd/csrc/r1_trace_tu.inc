// r1_trace_tu.inc — body of a translation unit that instantiates the trace kernel for ONE family.  The including file defines
//   R1_TU_NAME    tree_small | tree_big | sweep_small | sweep_big | grid_small | grid_big
//   R1_TU_BUILDS  the family's list of builds, one of r1_builds.h's R1_BUILDS_*: exactly what is instantiated here
#include "r1_trace.hpp"
#include "r1_internal.h"

#define R1_CAT2(a, b, c) a##b##c
#define R1_CAT(a, b, c) R1_CAT2(a, b, c)

// the __global__ instance of build (V, S, BIG, M)
template <int V, bool S, bool BIG, int M>
static constexpr auto r1_build_kernel()
{
    static_assert(!S || !(r1_mode_is_pass(M) || M == R1_MODE_PATH), "passes and paths have no diagnostic build");
    if constexpr (M == R1_MODE_PASS)
        return &r1_pass_kernel<V, BIG>;
    else if constexpr (M == R1_MODE_PATH)
        return &r1_path_kernel<V, BIG>;
    else if constexpr (M == R1_MODE_LISTED)
        return &r1_adaptive_kernel<V, BIG>;
    else if constexpr (V == R1_V_GRID)
        return &r1_grid_kernel<S, BIG, M>;
    else
        return &r1_trace_kernel<V, S, BIG, M>;
}

extern "C" hipError_t R1_CAT(r1_tu_, R1_TU_NAME, _launch)(const R1TraceArgs *args, R1Build b, int blocks, size_t dyn_lds, hipStream_t stream)
{
#define R1_X(V, S, BIG, M)                                                                                                                 \
    if (r1_same_build(b, V, S, BIG, M))                                                                                                    \
    {                                                                                                                                      \
        hipLaunchKernelGGL((r1_build_kernel<V, S, BIG, M>()), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);                       \
        return hipGetLastError();                                                                                                          \
    }
    R1_TU_BUILDS(R1_X)
#undef R1_X
    return hipErrorInvalidValue;
}

// The region twin of build b (r1_trace.hpp r1_region_kernel; DESIGN.md §4.37): every R1_MODE_PASS build of the family has one, which takes the
// arguments, the grid and the LDS of that build.  hipErrorInvalidValue: b has no twin.
template <int V, bool S, bool BIG, int M>
static hipError_t r1_region_launch(const R1TraceArgs *args, int blocks, size_t dyn_lds, hipStream_t stream)
{
    if constexpr (M == R1_MODE_PASS)
    {
        hipLaunchKernelGGL((r1_region_kernel<V, BIG>), dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);
        return hipGetLastError();
    }
    else
        return hipErrorInvalidValue;
}

extern "C" hipError_t R1_CAT(r1_tu_, R1_TU_NAME, _launch_region)(const R1TraceArgs *args, R1Build b, int blocks, size_t dyn_lds, hipStream_t stream)
{
#define R1_X(V, S, BIG, M)                                                                                                                 \
    if (r1_same_build(b, V, S, BIG, M))                                                                                                    \
        return r1_region_launch<V, S, BIG, M>(args, blocks, dyn_lds, stream);
    R1_TU_BUILDS(R1_X)
#undef R1_X
    return hipErrorInvalidValue;
}

extern "C" hipError_t R1_CAT(r1_tu_, R1_TU_NAME, _occupancy)(R1Build b, size_t dyn_lds, int *blocks_per_cu)
{
#define R1_X(V, S, BIG, M)                                                                                                                 \
    if (r1_same_build(b, V, S, BIG, M))                                                                                                    \
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, r1_build_kernel<V, S, BIG, M>(), R1_BLOCK, dyn_lds);
    R1_TU_BUILDS(R1_X)
#undef R1_X
    return hipErrorInvalidValue;
}
