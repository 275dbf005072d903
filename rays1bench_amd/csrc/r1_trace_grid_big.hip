// r1_trace_grid_big.hip — the trace kernel's instantiations for one family (r1_builds.h lists them); the kernel: r1_trace.hpp, its device functions: the headers that file includes
#define R1_TU_NAME grid_big
#define R1_TU_BUILDS R1_BUILDS_GRID_BIG
#include "r1_trace_tu.inc"
