// tools/check_resort_host.cpp — the host re-sort and refit driven directly, a stand-alone program: r1_build_bvh,
// r1_bvh_sort_topology, r1_bvh_resort_host and r1_bvh_refit_host on trees of its own making, among them what no scene reaches through
// r1_bvh_resort_describe: every leaf pinned, leaves pinned by hand between movable ones, and a re-sort STARTED from a re-sorted arrangement.
//
//   check_resort_host trees     structure on a few trees: the ids stay a permutation, pinned and empty slots stay, the slot table is the ids'
//                               inverse, the leaf table holds the centres given, every leaf's spheres stand in the order of x
//   check_resort_host twice     a re-sort to B after a re-sort to A equals a re-sort straight to B, and one more to B changes no byte
//
// tests/test_resort_host.py builds it with g++ against r1_bvh.cpp alone and runs both.  It is also the program for
// -fsanitize=address,undefined (host code only, no GPU, no library loaded into another process):
//     clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D__HIP_PLATFORM_AMD__
//         -I<hip include dir> tools/check_resort_host.cpp rays1bench_amd/csrc/r1_bvh.cpp -o check_resort_host_asan
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../rays1bench_amd/csrc/r1_bvh.h"
#include "../rays1bench_amd/csrc/r1_internal.h"

// (the library's error text lives in r1_capi.cpp, next to the HIP runtime: this program links r1_bvh.cpp only)
void r1_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

#define NEED(c)                                                \
    do                                                         \
    {                                                          \
        if (!(c))                                              \
        {                                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
            return 1;                                          \
        }                                                      \
    } while (0)

static uint32_t lcg_state = 12345u;
static float lcg() // [0, 1)
{
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (float)(lcg_state >> 8) * (1.0f / 16777216.0f);
}

struct Cloud
{
    std::vector<float> x, y, z, rsq;
    std::vector<double> rb;
    uint32_t n = 0;
    void add(float cx, float cy, float cz, float r)
    {
        x.push_back(cx), y.push_back(cy), z.push_back(cz), rsq.push_back(r * r), rb.push_back(r1_bound_radius(r * r, 1.0f / r)), ++n;
    }
};

// a ground sphere, three big balls and a jittered w x h lattice of small ones: the shape of the reference's scenes (outliers: the peel pins them)
static Cloud lattice(int w, int h, bool outliers)
{
    Cloud c;
    if (outliers)
    {
        c.add(0, -1000, 0, 1000);
        c.add(0, 1, 0, 2), c.add(-4, 1, 0, 2), c.add(4, 1, 0, 2);
    }
    for (int i = 0; i < w; ++i)
        for (int j = 0; j < h; ++j)
            c.add((float)(i - w / 2) + 0.6f * lcg(), 0.2f, (float)(j - h / 2) + 0.6f * lcg(), 0.2f);
    return c;
}

struct Tree
{
    R1Bvh b;
    R1RefitTopo t;
    R1SortTopo s;
};

static void build(const Cloud &c, int leaf_max, Tree &tr)
{
    Cloud pad = c;
    if (pad.n == 0)
        pad.x.push_back(0), pad.y.push_back(0), pad.z.push_back(0), pad.rsq.push_back(0), pad.rb.push_back(0);
    r1_build_bvh(c.n, pad.x.data(), pad.y.data(), pad.z.data(), pad.rsq.data(), pad.rb.data(), leaf_max, tr.b);
    r1_bvh_topology(tr.b, c.n, tr.t);
    r1_bvh_sort_topology(tr.b, tr.s);
}

// what must hold after a re-sort of `tr` (ids0: the ids before it) to the centres of `c`
static int check(const Tree &tr, const std::vector<uint32_t> &ids0, const Cloud &c)
{
    const R1Bvh &b = tr.b;
    NEED(b.ids.size() == ids0.size() && b.pair_pinned.size() * 2 == b.ids.size());
    std::vector<uint32_t> s0 = ids0, s1 = b.ids;
    std::sort(s0.begin(), s0.end()), std::sort(s1.begin(), s1.end());
    NEED(s0 == s1);
    for (size_t q = 0; q < ids0.size(); ++q)
    {
        NEED((ids0[q] == 0xFFFFFFFFu) == (b.ids[q] == 0xFFFFFFFFu));
        if (b.pair_pinned[q >> 1])
            NEED(ids0[q] == b.ids[q]);
        const uint32_t a = b.ids[q];
        if (a == 0xFFFFFFFFu || c.n == 0)
            continue;
        NEED(a < c.n && tr.t.slot[a] == q);
        if (b.pair_pinned[q >> 1]) // (a pinned sphere's words are the move's to write, not the re-sort's)
            continue;
        const float *p = &b.prims[8 * (q >> 1) + (q & 1)];
        NEED(memcmp(&p[0], &c.x[a], 4) == 0 && memcmp(&p[2], &c.y[a], 4) == 0 && memcmp(&p[4], &c.z[a], 4) == 0 && memcmp(&p[6], &c.rsq[a], 4) == 0);
    }
    for (size_t p = 0; p + 1 < tr.s.mslot.size(); ++p)
        NEED(tr.s.mslot[p] < tr.s.mslot[p + 1]);
    for (uint32_t ref : tr.t.leaf_ref) // a movable leaf's spheres stand in the order of (x, index)
    {
        const uint32_t first = ref & 0x0FFFFFFFu, pairs = (ref >> 28) & 7u;
        if (b.pair_pinned[first])
            continue;
        for (uint32_t q = 2 * first; q + 1 < 2 * (first + pairs); ++q)
            if (b.ids[q + 1] != 0xFFFFFFFFu)
                NEED(r1s_before(r1s_key(r1s_clamp(c.x[b.ids[q]])), b.ids[q], r1s_key(r1s_clamp(c.x[b.ids[q + 1]])), b.ids[q + 1]));
    }
    for (const R1SortSeg &g : tr.s.seg)
        NEED(g.b < g.e && g.k > 0 && g.k < g.e - g.b && g.e <= tr.s.mov.size());
    return 0;
}

static Cloud moved(const Cloud &c, int how)
{
    Cloud m = c;
    const uint32_t first = c.n > 8 ? 4 : 0;
    for (uint32_t i = first; i < c.n; ++i)
    {
        if (how == 0) // scattered over the lattice's extent
            m.x[i] = 40.0f * (lcg() - 0.5f), m.z[i] = 40.0f * (lcg() - 0.5f);
        else if (how == 1) // collapsed
            m.x[i] = 1.0f, m.y[i] = 0.5f, m.z[i] = -2.0f;
        else // jitter, some non-finite, a signed zero
            m.x[i] += lcg() - 0.5f, m.y[i] += 0.3f * lcg(), m.z[i] = i % 17 == 0 ? NAN : (i % 19 == 0 ? INFINITY : (i % 23 == 0 ? -0.0f : m.z[i]));
    }
    return m;
}

static int resort(Tree &tr, const Cloud &c)
{
    const std::vector<uint32_t> ids0 = tr.b.ids;
    Cloud pad = c;
    if (pad.n == 0)
        pad.x.push_back(0), pad.y.push_back(0), pad.z.push_back(0), pad.rsq.push_back(0), pad.rb.push_back(0);
    r1_bvh_resort_host(tr.b, tr.t, tr.s, pad.x.data(), pad.y.data(), pad.z.data(), pad.rsq.data());
    r1_bvh_refit_host(tr.b, tr.t, c.n, pad.x.data(), pad.y.data(), pad.z.data(), pad.rsq.data(), pad.rb.data());
    return check(tr, ids0, c);
}

static int trees()
{
    const int shapes[][3] = {{0, 0, 0}, {1, 1, 0}, {2, 2, 0}, {5, 1, 0}, {3, 3, 1}, {8, 8, 1}, {40, 30, 1}, {61, 47, 1}, {200, 120, 1}};
    for (const auto &sh : shapes)
        for (int leaf_max : {4, 8, 1})
        {
            const Cloud c = lattice(sh[0], sh[1], sh[2] != 0);
            for (int how = 0; how < 3; ++how)
            {
                Tree tr;
                build(c, leaf_max, tr);
                // (the peel takes at most leaf_max outliers: with one sphere per leaf the four stay in the lattice's tree, or are peeled further down)
                if (sh[2] && leaf_max >= 4 && c.n > 2u * (uint32_t)leaf_max + 4u)
                    NEED(std::count(tr.b.pair_pinned.begin(), tr.b.pair_pinned.end(), 1) >= 1 && tr.s.mov.size() == c.n - 4u);
                else if (!sh[2] || leaf_max >= 4)
                    NEED(tr.s.mov.size() == c.n);
                NEED(resort(tr, moved(c, how)) == 0);
            }
        }
    printf("built trees: the structure holds\n");
    // leaves pinned by hand: every third, then all of them
    const Cloud c = lattice(40, 30, true);
    for (int every : {3, 1})
    {
        Tree tr;
        build(c, 4, tr);
        for (size_t l = 0; l < tr.t.leaf_ref.size(); ++l)
            if (l % (size_t)every == 0)
                for (uint32_t q = tr.t.leaf_ref[l] & 0x0FFFFFFFu, e = q + ((tr.t.leaf_ref[l] >> 28) & 7u); q < e; ++q)
                    tr.b.pair_pinned[q] = 1;
        r1_bvh_sort_topology(tr.b, tr.s);
        const R1Bvh before = tr.b;
        NEED(resort(tr, moved(c, 0)) == 0);
        if (every == 1)
        {
            NEED(tr.s.mov.empty() && tr.s.seg.empty());
            NEED(tr.b.ids == before.ids && memcmp(tr.b.prims.data(), before.prims.data(), before.prims.size() * 4) == 0);
            printf("every leaf pinned: nothing moved\n");
        }
        else
            NEED(!tr.s.mov.empty() && tr.b.ids != before.ids);
    }
    return 0;
}

static int twice()
{
    for (const auto &sh : {std::pair<int, int>{8, 8}, {40, 30}, {160, 100}})
    {
        const Cloud c = lattice(sh.first, sh.second, true), a = moved(c, 0), b = moved(c, 2);
        Tree straight, via;
        build(c, 4, straight), build(c, 4, via);
        NEED(resort(straight, b) == 0);
        NEED(resort(via, a) == 0);
        NEED(via.b.ids != straight.b.ids);
        NEED(resort(via, b) == 0);
        NEED(via.b.ids == straight.b.ids && via.t.slot == straight.t.slot);
        NEED(memcmp(via.b.prims.data(), straight.b.prims.data(), straight.b.prims.size() * 4) == 0);
        NEED(memcmp(via.b.nodes.data(), straight.b.nodes.data(), straight.b.nodes.size() * 4) == 0);
        NEED(resort(via, b) == 0);
        NEED(via.b.ids == straight.b.ids && memcmp(via.b.nodes.data(), straight.b.nodes.data(), straight.b.nodes.size() * 4) == 0);
    }
    printf("a re-sort of the re-sorted arrangement: unchanged\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "trees") == 0)
        return trees();
    if (argc == 2 && strcmp(argv[1], "twice") == 0)
        return twice();
    fprintf(stderr, "usage: check_resort_host trees | twice\n");
    return 2;
}
