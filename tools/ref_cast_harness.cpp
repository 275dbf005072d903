// tools/ref_cast_harness.cpp — TEST INFRASTRUCTURE, not product code; built and run by tools/gen_cast_golden.py only.
//
// Answers rays with the reference's OWN Hitable::hit (rayweek1.cpp:152-339) through its own Ray constructor (:104-108): the
// reference's translation unit is #include'd by path from -DREF_STEP13_TU, the way oracle/ref_harness.cpp does it, and compiled with
// the STRICT flags of oracle/Makefile.  The binary is made in a temporary directory and never committed; nothing of the reference is
// copied into this repository.
//
//   ref_cast <small|medium|large> <rays.f32> <hits.bin> <spheres.f32>
//     rays.f32     n records of 8 floats {ox oy oz t_max dx dy dz pad}
//     hits.bin     n records of 8 words  {t, index (0xFFFFFFFF: miss), px py pz, nx ny nz}
//     spheres.f32  the reference's sphere arrays: count (as one uint32 word), then center_x, center_y, center_z, radius_sq, inv_radius
// The hit index is recovered by finding rec.material in the material column of the reference's struct of arrays (every real sphere
// owns its material object; placeholders have none and are never hit).

#include <stdio.h>
#include <stdlib.h>
#include <assert.h>
#include <float.h>
#include <ctime>
#include <mutex>
#include <thread>
#include <atomic>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <immintrin.h>
#include <chrono>
#include <mm_malloc.h>
#include <vector>
#include <string>

#define class struct
#define main ref_main
#include REF_STEP13_TU
#undef main
#undef class

int main(int argc, const char **argv)
{
    if (argc != 5)
    {
        fprintf(stderr, "usage: ref_cast <scene> <rays.f32> <hits.bin> <spheres.f32>\n");
        return 2;
    }
    Scene *scene = nullptr;
    if (!strcmp(argv[1], "small"))
        scene = create_small_scene();
    else if (!strcmp(argv[1], "medium"))
        scene = create_medium_scene();
    else if (!strcmp(argv[1], "large"))
        scene = create_large_scene();
    if (!scene)
        return 2;
    const SphereSOA::InstanceData *s = scene->hitables->_soa_spheres.getData();
    const uint32_t count = s->_count;

    FILE *f = fopen(argv[2], "rb");
    if (!f)
        return 3;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const size_t n = (size_t)bytes / 32;
    std::vector<float> rays(8 * n);
    if (fread(rays.data(), 32, n, f) != n)
        return 3;
    fclose(f);

    std::vector<uint32_t> out(8 * n);
    for (size_t i = 0; i < n; ++i)
    {
        const float *q = &rays[8 * i];
        const Ray r(Vec3(q[0], q[1], q[2]), Vec3(q[4], q[5], q[6]));
        HitRecord rec;
        memset(&rec, 0, sizeof(rec));
        const bool hit = scene->hitables->hit(r, 0.001f, q[3], &rec);
        uint32_t *o = &out[8 * i];
        float rec_f[7] = {FLT_MAX, 0, 0, 0, 0, 0, 0};
        uint32_t index = 0xFFFFFFFFu;
        if (hit)
        {
            uint32_t found = 0;
            for (uint32_t k = 0; k < count; ++k)
                if (s->material[k] == rec.material && s->material[k] != nullptr)
                    index = k, ++found;
            if (found != 1)
            {
                fprintf(stderr, "ray %zu: the hit's material names %u spheres\n", i, found);
                return 4;
            }
            rec_f[0] = rec.t;
            rec_f[1] = rec.p.getX(), rec_f[2] = rec.p.getY(), rec_f[3] = rec.p.getZ();
            rec_f[4] = rec.normal.getX(), rec_f[5] = rec.normal.getY(), rec_f[6] = rec.normal.getZ();
        }
        memcpy(&o[0], &rec_f[0], 4);
        o[1] = index;
        memcpy(&o[2], &rec_f[1], 24);
    }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 32, n, f) != n)
        return 5;
    fclose(f);

    f = fopen(argv[4], "wb");
    if (!f)
        return 5;
    fwrite(&count, 4, 1, f);
    fwrite(s->center_x, 4, count, f);
    fwrite(s->center_y, 4, count, f);
    fwrite(s->center_z, 4, count, f);
    fwrite(s->radius_sq, 4, count, f);
    fwrite(s->inv_radius, 4, count, f);
    fclose(f);
    return 0;
}
