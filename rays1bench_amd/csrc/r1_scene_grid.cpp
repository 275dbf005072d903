// r1_scene_grid.cpp — the uniform grid of a context's scene: built and uploaded on first use (ensure_grid), re-registered on the device
// after the spheres have moved (r1_regrid; the kernels are r1_regrid.hip's), and read back (r1_grid_download).

#include <string.h>

#include <algorithm>
#include <vector>

#include "r1_context.h"
#include "r1_device_sort.h"

// Both forms of the R1GridArgs the kernels read, from a filled G (tab and lds_bytes: the small form's where there is one): grid_dev receives
// G if the scene's grid is `small`, grid_dev32 always the 32-bit form.  On the context's stream; the caller waits.
static int upload_grid_args(r1_context *c, const R1GridArgs &G, bool small)
{
    R1GridArgs G32 = G;
    G32.tab = (const uint32_t *)c->grid_tab32.p, G32.lds_bytes = 0;
    int rc;
    if ((rc = ensure(c->grid_dev, sizeof(G))) || (rc = ensure(c->grid_dev32, sizeof(G))))
        return rc;
    R1_HIP(hipMemcpyAsync(c->grid_dev.p, small ? &G : &G32, sizeof(G), hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->grid_dev32.p, &G32, sizeof(G), hipMemcpyHostToDevice, c->stream));
    return R1_OK;
}

// R1_VARIANT_GRID: builds the uniform grid of the context's scene (from the arrays r1_set_scene received, so that r1_grid_describe and
// r1_grid_visit see the same grid) and uploads it, once per scene.  Contexts that never ask for the grid pay nothing for it.
int ensure_grid(r1_context *c)
{
    if (c->grid_valid)
        return R1_OK;
    r1_scene s;
    s.count = (uint32_t)c->src_mat.size();
    s.center_x = c->src_f32[0].data(), s.center_y = c->src_f32[1].data(), s.center_z = c->src_f32[2].data();
    s.radius_sq = c->src_f32[3].data(), s.inv_radius = c->src_f32[4].data(), s.mat_type = c->src_mat.data();
    s.albedo_r = c->src_f32[5].data(), s.albedo_g = c->src_f32[6].data(), s.albedo_b = c->src_f32[7].data(), s.mat_param = c->src_f32[8].data();
    R1Grid g;
    if (r1_grid_from_scene(&s, g) != R1_OK)
    {
        r1_set_error("grid: the scene's spheres could not be read");
        return R1_EINVAL;
    }
    // small-scene kernel: 16-bit cell starts and ids, all of it copied into every workgroup's LDS
    const size_t halves = g.start.size() + g.ids.size();
    c->grid_small = c->n_active <= R1_MAX_ACTIVE_10BIT && halves <= R1_GRID_LDS_HALVES && g.ids.size() < 65536u;
    std::vector<uint32_t> tab32;
    std::vector<uint16_t> tab16;
    size_t tab_bytes;
    if (c->grid_small)
    {
        tab16.assign((halves + 7) & ~(size_t)7, 0); // (whole 16-byte rows: the kernel copies float4)
        for (size_t q = 0; q < g.start.size(); ++q)
            tab16[q] = (uint16_t)g.start[q];
        for (size_t q = 0; q < g.ids.size(); ++q)
            tab16[g.start.size() + q] = (uint16_t)g.ids[q];
        tab_bytes = tab16.size() * 2;
    }
    tab32 = g.start;
    tab32.insert(tab32.end(), g.ids.begin(), g.ids.end());
    if (!c->grid_small)
        tab_bytes = tab32.size() * 4;
    std::vector<uint32_t> outl = g.outliers;
    if (outl.empty())
        outl.push_back(0u);
    int rc;
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipDeviceSynchronize()); // (launches of an earlier grid may still read the buffers that are about to be replaced)
    if ((rc = ensure(c->grid_tab, tab_bytes)) || (rc = ensure(c->grid_out, outl.size() * 4)) || (rc = ensure(c->grid_tab32, tab32.size() * 4)))
        return rc;
    R1_HIP(hipMemcpyAsync(c->grid_tab32.p, tab32.data(), tab32.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->grid_tab.p, c->grid_small ? (const void *)tab16.data() : (const void *)tab32.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipMemcpyAsync(c->grid_out.p, outl.data(), outl.size() * 4, hipMemcpyHostToDevice, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    R1GridArgs &G = c->grid_args;
    memset(&G, 0, sizeof(G));
    G.geom = g.geom;
    G.outliers = (const uint32_t *)c->grid_out.p;
    G.n_out = (uint32_t)g.outliers.size();
    G.n_start = (uint32_t)g.start.size();
    G.tab = (const uint32_t *)c->grid_tab.p;
    G.lds_bytes = c->grid_small ? (uint32_t)tab_bytes : 0u;
    if ((rc = upload_grid_args(c, G, c->grid_small)))
        return rc;
    R1_HIP(hipStreamSynchronize(c->stream));
    c->grid_valid = true;
    r1_grid_plan(g, c->grid_plan); // what a later r1_regrid keeps
    c->grid_planned = true, c->regrid_ready = false;
    return R1_OK;
}

// ---- regrid: the moved spheres re-registered in the uniform grid (include/rays1.h "regrid") -----------------------------------------------------

// A scene's first regrid: the tables grown to the capacity (both forms; the small one only if it holds the capacity), the outlier list to
// one entry per sphere, the scratch laid out, both R1GridArgs uploaded again with the new addresses — once per scene, kept from then on.
static int regrid_layout(r1_context *c)
{
    if (c->regrid_ready)
        return R1_OK;
    const R1GridPlan &P = c->grid_plan;
    const uint32_t na = c->n_active, cap = r1gf_capacity(P.regs);
    const size_t words = (size_t)P.n_start + cap, halves16 = (words + 7) & ~(size_t)7; // (whole 16-byte rows: the kernel copies float4)
    const bool small = na <= R1_MAX_ACTIVE_10BIT && words <= R1_GRID_LDS_HALVES && cap <= 65535u;
    const size_t hist = r1_radix_hist_words(cap, 1);
    const size_t sums = std::max(r1_scan_sums_words((size_t)na + 1), r1_scan_sums_words(hist));
    const size_t part_bytes = r1_blocks((size_t)na + 1) * R1GF_EXTENT_WORDS * sizeof(double);
    const size_t ws_words = 2 * ((size_t)na + 1) + 4 * (size_t)cap + hist + (sums ? sums : 1) + R1GF_STAT_WORDS;
    int rc;
    R1_HIP(hipDeviceSynchronize()); // (launches through the grid may still read the buffers that are about to be replaced)
    if ((rc = ensure(c->grid_tab32, words * 4)) || (rc = ensure(c->grid_tab, small ? halves16 * 2 : 256)) || (rc = ensure(c->grid_out, (size_t)na * 4)) ||
        (rc = ensure(c->regrid_ws, part_bytes + ws_words * 4)))
        return rc;
    R1GridArgs &G = c->grid_args;
    memset(&G, 0, sizeof(G));
    for (int a = 0; a < 3; ++a)
        G.geom.lo[a] = P.lo[a], G.geom.cell[a] = P.cell[a], G.geom.inv_cell[a] = P.inv_cell[a], G.geom.n[a] = P.n[a];
    G.geom.v2 = -1.0f; // (until the first regrid's kernels have run: every ray the tree)
    G.outliers = (const uint32_t *)c->grid_out.p;
    G.n_out = 0;
    G.n_start = P.n_start;
    G.tab = (const uint32_t *)(small ? c->grid_tab.p : c->grid_tab32.p);
    G.lds_bytes = small ? (uint32_t)(halves16 * 2) : 0u;
    if ((rc = upload_grid_args(c, G, small)))
        return rc;
    R1_HIP(hipMemsetAsync(c->grid_tab32.p, 0, words * 4, c->stream));
    R1_HIP(hipStreamSynchronize(c->stream));
    c->grid_small = small;
    forget_occupancy(c); // the small grid kernels' LDS footprint follows lds_bytes

    R1RegridArgs &r = c->regrid;
    memset(&r, 0, sizeof(r));
    r.plan = P;
    r.exact = (const float *)c->exact.p, r.radii = (const double *)c->refit_radii.p;
    r.na = na, r.cap = cap, r.small = small ? 1u : 0u, r.tab16_halves = small ? (uint32_t)halves16 : 0u;
    r.g16 = (R1GridArgs *)c->grid_dev.p, r.g32 = (R1GridArgs *)c->grid_dev32.p;
    r.tab32 = (uint32_t *)c->grid_tab32.p, r.tab16 = small ? (uint16_t *)c->grid_tab.p : nullptr, r.outliers = (uint32_t *)c->grid_out.p;
    r.part = (double *)c->regrid_ws.p;
    uint32_t *w = (uint32_t *)((char *)c->regrid_ws.p + part_bytes);
    r.span = w, r.oflag = w + na + 1, w += 2 * ((size_t)na + 1);
    r.key[0] = w, r.key[1] = w + cap, r.val[0] = w + 2 * (size_t)cap, r.val[1] = w + 3 * (size_t)cap, w += 4 * (size_t)cap;
    r.hist = w, r.sums = w + hist, r.stat = r.sums + (sums ? sums : 1);
    c->regrid_ready = true;
    return R1_OK;
}

extern "C" int r1_regrid(r1_context *c, void *hip_stream)
{
    int rc = need_scene("r1_regrid", c);
    if (rc)
        return rc;
    R1_HIP(hipSetDevice(c->device));
    if (!c->grid_planned)
    {
        if (c->moved)
        {
            // (host-form updates overwrite the context's copies of the arrays: the plan can only come from those r1_set_scene received)
            r1_set_error("r1_regrid: the scene has moved and its grid was never built; call r1_regrid once, or render once through the grid, "
                         "before the first update");
            return R1_EINVAL;
        }
        if ((rc = ensure_grid(c)))
            return rc;
    }
    if (c->n_active == 0) // nothing to register: the build's empty tables serve every position of no spheres
    {
        c->grid_valid = true;
        return R1_OK;
    }
    c->grid_valid = false; // (a launch that failed half-way leaves no grid)
    if ((rc = regrid_layout(c)))
        return rc;
    R1_HIP(r1_launch_regrid(&c->regrid, hip_stream ? (hipStream_t)hip_stream : c->stream));
    c->grid_valid = true;
    return R1_OK;
}

extern "C" int r1_grid_download(r1_context *c, r1_grid_info *info, uint32_t *start_out, size_t start_cap, uint32_t *ids_out, size_t ids_cap,
                                uint32_t *outliers_out, size_t outliers_cap)
{
    int rc = need_scene("r1_grid_download", c, "info", info);
    if (rc)
        return rc;
    if (!c->grid_valid)
    {
        r1_set_error("r1_grid_download: the context holds no current grid (render through it once, or call r1_regrid)");
        return R1_EINVAL;
    }
    R1_HIP(hipSetDevice(c->device));
    R1_HIP(hipDeviceSynchronize());
    R1GridArgs G;
    R1_HIP(hipMemcpy(&G, c->grid_dev32.p, sizeof(G), hipMemcpyDeviceToHost));
    R1Grid g;
    g.geom = G.geom;
    g.start.assign(G.n_start, 0u);
    R1_HIP(hipMemcpy(g.start.data(), G.tab, (size_t)G.n_start * 4, hipMemcpyDeviceToHost));
    if (g.start.back() > (uint64_t)R1_GRID_SPAN_MAX * c->n_active)
    {
        r1_set_error("r1_grid_download: the device's cell table ends at %u registrations for %u spheres", g.start.back(), c->n_active);
        return R1_EHIP;
    }
    g.ids.assign(g.start.back(), 0u);
    if (!g.ids.empty())
        R1_HIP(hipMemcpy(g.ids.data(), G.tab + G.n_start, g.ids.size() * 4, hipMemcpyDeviceToHost));
    g.outliers.assign(G.n_out, 0u);
    if (G.n_out)
        R1_HIP(hipMemcpy(g.outliers.data(), G.outliers, (size_t)G.n_out * 4, hipMemcpyDeviceToHost));
    const uint32_t na = c->n_active;
    for (uint32_t id : g.ids)
        if (id >= na)
        {
            r1_set_error("r1_grid_download: the device's id table names sphere %u of %u", id, na);
            return R1_EHIP;
        }
    for (uint32_t id : g.outliers)
        if (id >= na)
        {
            r1_set_error("r1_grid_download: the device's outlier list names sphere %u of %u", id, na);
            return R1_EHIP;
        }
    for (size_t q = 1; q < g.start.size(); ++q)
        g.max_occupancy = std::max(g.max_occupancy, g.start[q] - g.start[q - 1]);
    // pad and V as r1_grid_describe reports them: from the rows the device holds
    g.v_safe = c->grid_plan.V;
    if (!g.ids.empty())
    {
        std::vector<float> ex(4 * (size_t)na);
        std::vector<double> radii(2 * (size_t)na);
        R1_HIP(hipMemcpy(ex.data(), c->exact.p, ex.size() * 4, hipMemcpyDeviceToHost));
        R1_HIP(hipMemcpy(radii.data(), c->refit_radii.p, radii.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t id : g.ids)
            g.pad = std::max(g.pad, r1gf_rho(ex[4 * (size_t)id], ex[4 * (size_t)id + 1], ex[4 * (size_t)id + 2], radii[2 * (size_t)id + 1], c->grid_plan.V, c->grid_plan.delta) -
                                        radii[2 * (size_t)id]);
    }
    return r1_grid_report(g, c->active_to_scene, G.geom.v2 < 0.0f, info, start_out, start_cap, ids_out, ids_cap, outliers_out, outliers_cap);
}
