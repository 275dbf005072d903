// tools/builder_bits.cpp — the host builders' output for the five scenes of tests/test_bvh_host.py::test_tree_structure, hashed: the box tree's
// node rows and ids (r1_bvh_describe) and the sweep builder's per-sphere tables exact / shade / mat (r1_build_sweep).  Run against two builds of
// librays1.so to show that a change of the builders' code changed no bit (profiles/r11/builder_bits.txt, profiles/r20/builder_bits.txt):
//   hipcc -std=c++17 -O1 -o builder_bits tools/builder_bits.cpp -Lrays1bench_amd/lib -lrays1
//   LD_LIBRARY_PATH=<dir of one build> ./builder_bits [dump-file]     (no GPU needed; dump-file receives the raw arrays for a byte comparison)
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../rays1bench_amd/csrc/r1_bvh.h"
#include "../rays1bench_amd/csrc/r1_sweep.h"

static uint64_t fnv(const void *p, size_t n, FILE *dump)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i)
        h = (h ^ ((const uint8_t *)p)[i]) * 1099511628211ull;
    if (dump)
        fwrite(p, 1, n, dump);
    return h;
}

int main(int argc, char **argv)
{
    FILE *dump = argc > 1 ? fopen(argv[1], "wb") : nullptr;
    const struct
    {
        const char *name;
        int kind, gw, gh;
    } scenes[5] = {{"small", R1_SCENE_SMALL, 0, 0}, {"medium", R1_SCENE_MEDIUM, 0, 0}, {"large", R1_SCENE_LARGE, 0, 0},
                   {"grid64x40", R1_SCENE_GRID, 64, 40}, {"grid400x250", R1_SCENE_GRID, 400, 250}};
    for (const auto &sc : scenes)
    {
        r1_host_scene *hs = nullptr;
        if (r1_host_scene_create(sc.kind, 1200, 800, sc.gw, sc.gh, &hs) != R1_OK)
            return 1;
        const r1_scene *s = r1_host_scene_spheres(hs);
        r1_bvh_info info;
        if (r1_bvh_describe(s, 0, &info, nullptr, 0, nullptr, 0) != R1_OK)
            return 1;
        std::vector<float> nodes(16 * (size_t)info.nodes);
        std::vector<uint32_t> ids(2 * (size_t)info.pairs + 2);
        if (r1_bvh_describe(s, 0, &info, nodes.data(), nodes.size(), ids.data(), ids.size()) != R1_OK)
            return 1;
        std::vector<uint32_t> active;
        r1_active_spheres(s, active);
        R1Sweep sw;
        r1_build_sweep(s, active, sw);
        printf("%-12s nodes %6d %016llx  ids %6d %016llx  exact %7zu %016llx  shade %7zu %016llx  mat %7zu %016llx  pad_local %d root_leaf %d flat_axis %d\n",
               sc.name, info.nodes, (unsigned long long)fnv(nodes.data(), nodes.size() * 4, dump), 2 * info.pairs,
               (unsigned long long)fnv(ids.data(), 8 * (size_t)info.pairs, dump), sw.exact.size(), (unsigned long long)fnv(sw.exact.data(), sw.exact.size() * 4, dump),
               sw.shade.size(), (unsigned long long)fnv(sw.shade.data(), sw.shade.size() * 4, dump), sw.mat.size(),
               (unsigned long long)fnv(sw.mat.data(), sw.mat.size() * 4, dump), info.pad_local, info.root_leaf, info.flat_axis);
        r1_host_scene_destroy(hs);
    }
    if (dump)
        fclose(dump);
    return 0;
}
