// r1_trace_tree_small.hip — the trace kernel's instantiations for one family (r1_builds.h lists them); the kernel: r1_trace.hpp, its device functions: the headers that file includes
#define R1_TU_NAME tree_small
#define R1_TU_BUILDS R1_BUILDS_TREE_SMALL
#include "r1_trace_tu.inc"

// The flat twins of this family's frames-in-flight builds (r1_trace.hpp r1_flatwalk_kernel): b is the build r1_pick chose, and
// the twin of (R1_V_TREE, false, false, R1_MODE_TP / _BATCH) takes the arguments, the grid and the LDS of that build.  hipErrorInvalidValue: b has no twin.
extern "C" hipError_t r1_tu_tree_small_launch_flat(const R1TraceArgs *args, R1Build b, int blocks, size_t dyn_lds, hipStream_t stream)
{
    if (r1_same_build(b, R1_V_TREE, false, false, R1_MODE_TP))
        hipLaunchKernelGGL(r1_flatwalk_kernel<R1_MODE_TP>, dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);
    else if (r1_same_build(b, R1_V_TREE, false, false, R1_MODE_BATCH))
        hipLaunchKernelGGL(r1_flatwalk_kernel<R1_MODE_BATCH>, dim3(blocks), dim3(R1_BLOCK), dyn_lds, stream, *args);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
