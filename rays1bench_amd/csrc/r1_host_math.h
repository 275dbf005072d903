// r1_host_math.h — the reference's Vec3 arithmetic on the host, operation by operation in the reference's order.  The files that include it
// (r1_host.cpp, r1_queries_host.cpp) are compiled with -ffp-contract=off: nothing here is contracted into an FMA.
#ifndef R1_HOST_MATH_H
#define R1_HOST_MATH_H

#include <math.h>

namespace r1_host_math
{

struct V3
{
    float x, y, z;
};

inline V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
// mymath.h:205-207 — lanes are summed as (x + y) + z
inline float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// mymath.h:211
inline V3 unit(V3 v) { return scale(v, 1.0f / sqrtf(dot(v, v))); }

} // namespace r1_host_math

#endif
