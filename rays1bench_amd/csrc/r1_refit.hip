// r1_refit.hip — moving spheres (r1_update_centers*): new centres into the tables the tree kernels read, then the box tree's
// rows recomputed bottom-up over its unchanged topology, in r1_bvh_fill.h's arithmetic — the host builder's own, bit for bit.  And sphere
// updates (r1_update_spheres*, §4.27): radii and materials into the same tables, then the same refit where a radius changed.
//
// The hand-over between the tree's heights is the KERNEL BOUNDARY: plain stores are not seen across XCDs inside a kernel, and a release fence
// costs ~105 us under load (profiles/r04/xcd_visibility.txt) — a bottom-up walk with arrival counters inside one kernel
// would pay it per node.  One small launch per height instead, all on one stream.  Nothing here is near a trace kernel's critical path:
// plain HIP C++, one lane per item, vector stores.
#include <hip/hip_runtime.h>

#include "r1_bvh_fill.h"
#include "r1_internal.h"

#define R1_REFIT_BLOCK 256

// One lane per sphere of the range [first, first + count) of the SCENE: the centre into exact[a].xyz and into the sphere's slot of the tree's
// leaf table.  radius_sq and the speculative partner slots stay as they are.  Spheres that are not active have no entry anywhere.
__global__ void __launch_bounds__(R1_REFIT_BLOCK) r1_refit_move_kernel(R1RefitArgs A, uint32_t first, uint32_t count, const float *__restrict__ x,
                                                                        const float *__restrict__ y, const float *__restrict__ z)
{
    const uint32_t i = blockIdx.x * R1_REFIT_BLOCK + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t a = A.scene_to_active[first + i];
    if (a == 0xFFFFFFFFu)
        return;
    const float cx = x[i], cy = y[i], cz = z[i];
    float *e = A.exact + 4 * (size_t)a;
    e[0] = cx, e[1] = cy, e[2] = cz;
    const uint32_t q = A.slot[a];
    float *p = A.prims + 8 * (size_t)(q >> 1) + (q & 1u);
    p[0] = cx, p[2] = cy, p[4] = cz;
}

// Radii and materials changed in place (r1_update_spheres*).  One lane per sphere of the range [first, first + count) of the
// SCENE; `groups` says which of the two groups the launch writes.  R1_SET_RADII: the new radius_sq into exact[a].w and into the sphere's word
// of its leaf pair (the slot the move kernel addresses), inv_radius into shade[a].x, {bound, test} radius into the refit's table — what the
// builders derive, in their arithmetic (r1f_radius_rows); a pair that r1_active_spheres would drop makes the sphere never hittable.
// R1_SET_MATERIALS: the albedo into shade[a].yzw and the whole mat[a] row (r1f_material_row); a type that is no material is skipped.
__global__ void __launch_bounds__(R1_REFIT_BLOCK) r1_refit_set_kernel(R1RefitArgs A, R1SetArgs S, uint32_t first, uint32_t count, uint32_t groups)
{
    const uint32_t i = blockIdx.x * R1_REFIT_BLOCK + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t a = A.scene_to_active[first + i];
    if (a == 0xFFFFFFFFu)
        return;
    float *sh = S.shade + 4 * (size_t)a;
    if (groups & R1_SET_RADII)
    {
        float rsq, inv;
        double rr[2];
        r1f_radius_rows(S.radius_sq[i], S.inv_radius[i], rsq, inv, rr);
        A.exact[4 * (size_t)a + 3] = rsq;
        const uint32_t q = A.slot[a];
        A.prims[8 * (size_t)(q >> 1) + 6 + (q & 1u)] = rsq;
        sh[0] = inv;
        S.radii[2 * (size_t)a + 0] = rr[0], S.radii[2 * (size_t)a + 1] = rr[1];
    }
    if (groups & R1_SET_MATERIALS)
    {
        const uint32_t type = S.mat_type[i];
        if (type <= 2u /* R1_MAT_DIELECTRIC */)
        {
            float row[4];
            r1f_material_row(type, S.mat_param[i], row);
            sh[1] = S.albedo_r[i], sh[2] = S.albedo_g[i], sh[3] = S.albedo_b[i];
            float *m = S.mat + 4 * (size_t)a;
            m[0] = row[0], m[1] = row[1], m[2] = row[2], m[3] = row[3];
        }
    }
}

// One lane per leaf: its spheres' boxes merged in fp64 into the leaf's scratch entry.  Lane 0 of the launch also zeroes the largest-A word
// the height launches raise (they start after this kernel has ended).
__global__ void __launch_bounds__(R1_REFIT_BLOCK) r1_refit_leaf_kernel(R1RefitArgs A)
{
    const uint32_t l = blockIdx.x * R1_REFIT_BLOCK + threadIdx.x;
    if (l == 0)
        *A.a_max = 0u;
    if (l >= A.n_leaves)
        return;
    R1Box bx;
    r1f_refit_leaf(A.leaf_ref[l], A.ids, A.exact, A.radii, bx);
    A.box[A.n_nodes + l] = bx;
}

// One lane per node of one height: by_height[begin .. end).  Both children's boxes are final: leaves' since the leaf kernel, inner nodes'
// since the launch of their (lower) height.
__global__ void __launch_bounds__(R1_REFIT_BLOCK) r1_refit_height_kernel(R1RefitArgs A, uint32_t begin, uint32_t end)
{
    const uint32_t i = begin + blockIdx.x * R1_REFIT_BLOCK + threadIdx.x;
    if (i >= end)
        return;
    const float a = r1f_refit_node(A.fill, A.by_height[i], A.child_box, A.box, A.nodes);
    atomicMax(A.a_max, __float_as_uint(a)); // (A > 0: the bits of positive floats order as the floats do)
}

// Trees whose pad is measured from the scene's centre: ONE A for the whole tree, the largest of the rows' (the builder's last step)
__global__ void __launch_bounds__(R1_REFIT_BLOCK) r1_refit_finish_kernel(R1RefitArgs A)
{
    const uint32_t n = blockIdx.x * R1_REFIT_BLOCK + threadIdx.x;
    if (n < A.n_nodes)
        A.nodes[16 * (size_t)n + 12] = __uint_as_float(*A.a_max);
}

static inline unsigned refit_blocks(uint32_t n) { return (n + R1_REFIT_BLOCK - 1) / R1_REFIT_BLOCK; }

extern "C" hipError_t r1_launch_refit_move(const R1RefitArgs *a, uint32_t first, uint32_t count, const float *x, const float *y, const float *z,
                                           hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(r1_refit_move_kernel, dim3(refit_blocks(count)), dim3(R1_REFIT_BLOCK), 0, stream, *a, first, count, x, y, z);
    return hipGetLastError();
}

extern "C" hipError_t r1_launch_refit_set(const R1RefitArgs *a, const R1SetArgs *s, uint32_t first, uint32_t count, uint32_t groups, hipStream_t stream)
{
    if (count == 0 || !(groups & (R1_SET_RADII | R1_SET_MATERIALS)))
        return hipSuccess;
    hipLaunchKernelGGL(r1_refit_set_kernel, dim3(refit_blocks(count)), dim3(R1_REFIT_BLOCK), 0, stream, *a, *s, first, count, groups);
    return hipGetLastError();
}

// height_off: [heights + 1] (host memory) offsets of each height's nodes in by_height
extern "C" hipError_t r1_launch_refit(const R1RefitArgs *a, const uint32_t *height_off, uint32_t heights, hipStream_t stream)
{
    hipLaunchKernelGGL(r1_refit_leaf_kernel, dim3(refit_blocks(a->n_leaves ? a->n_leaves : 1u)), dim3(R1_REFIT_BLOCK), 0, stream, *a);
    for (uint32_t h = 0; h < heights; ++h)
        if (height_off[h + 1] > height_off[h])
            hipLaunchKernelGGL(r1_refit_height_kernel, dim3(refit_blocks(height_off[h + 1] - height_off[h])), dim3(R1_REFIT_BLOCK), 0, stream, *a,
                               height_off[h], height_off[h + 1]);
    if (!a->fill.pad_local)
        hipLaunchKernelGGL(r1_refit_finish_kernel, dim3(refit_blocks(a->n_nodes)), dim3(R1_REFIT_BLOCK), 0, stream, *a);
    return hipGetLastError();
}
