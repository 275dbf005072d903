// r1_trace_tree_small.hip — the trace kernel's instantiations for one family (r1_builds.h lists them); the kernel: r1_trace.hpp, its device functions: the headers that file includes
#define R1_TU_NAME tree_small
#define R1_TU_BUILDS R1_BUILDS_TREE_SMALL
#include "r1_trace_tu.inc"
