// rayweek1_options.h — what the two halves of the drop-in host program share: the run-time options (rayweek1_hip.cpp parses them and
// renders benchmark()'s frames with them) and the demos that run after the benchmark() runs (rayweek1_demos.cpp).
#pragma once

#include <stdint.h>

#include "../../include/rays1.h"

// What the reference fixes at compile time (SCREEN_W / SCREEN_H / NUM_SAMPLES_PER_PIXEL, common.h:19-28) and what this program adds.
struct Options
{
    int width = 1280, height = 720, spp = 10 * 25; // the reference's multi-threaded defaults
    int max_bounces = 50;
    uint32_t seed = 10001;
    int device = 0, devices = 1;
    int variant = R1_VARIANT_DEFAULT;
    int backend = 0; // 0 hip, 1 cpu-step1, 12 cpu-step12
    int gather = -1; // -1 auto, 0 host, 1 rccl
    int passes = 0;  // --passes K: every frame in K progressive passes (r1_render_pass); 0 = one r1_render
    bool adaptive = false; // --adaptive: every frame through r1_render_adaptive
    r1_adaptive adapt = {16, 16, 0, 65280};
    bool linear = false; // --linear: every frame through r1_render_linear, the pixels through r1_quantise_linear; -w also writes out_<scene>.pfm
    bool features = false; // --features: each frame's feature frame too (r1_render_features); -w also writes out_<scene>_albedo.pfm, _normal.pfm, _depth.pfm
    // --denoise [ITERATIONS]: --linear, and each frame also through r1_render_denoised; -w also writes out_<scene>_denoised.pfm next to out_<scene>.pfm
    bool denoise = false;
    r1_denoise_opt denoise_opt = {3, 6, 1.0f, 0.1f, R1_DENOISE_DEMODULATE};
    // --denoise-guided [ITERATIONS]: --linear, and each frame also through r1_render_denoised_guided (sigma colour 2, variance floor 1e-4); the same file
    bool denoise_guided = false;
    r1_denoise_guided_opt guided_opt = {{3, 6, 2.0f, 0.1f, R1_DENOISE_DEMODULATE}, 1e-4f, 0u};
    bool region = false; // --region X,Y,W,H: every frame through r1_render_region; the pixels, the TGA and the counts are the window's
    r1_region window = {0, 0, 0, 0, 0};
    // the demos, each FRAMES frames per scene after the benchmark() runs; 0 = not asked for
    int pipeline = 0; // --pipeline: the same frame, --inflight of them in flight (r1_render_async)
    int inflight = 20;
    int orbit = 0;  // --orbit: the camera turned about the vertical axis through lookat (r1_render_path_async)
    int bounce = 0; // --bounce: the lattice spheres bobbing in y, one r1_update_centers between frames
    int pulse = 0;  // --pulse: the lattice spheres' radii breathing and their albedo cycling, one r1_update_spheres between frames
};
extern Options g_opt;

r1_params frame_params(); // the frame every part of the program renders: the options, 32 x 32 tiles, one shard

// One scene's run of a demo: prints its report line, with `write_tga` writes the first and the middle frame as <demo>_<scene>_<nnn>.tga
// (pipelined keeps no frames); returns 0, or 1 after `<demo> <scene>: <r1_last_error>` on stderr.
typedef int (*Demo)(const char *scene_name, int kind, int frames, bool write_tga);
int pipelined(const char *scene_name, int kind, int frames, bool write_tga);
int orbit(const char *scene_name, int kind, int frames, bool write_tga);
int bounce(const char *scene_name, int kind, int frames, bool write_tga);
int pulse(const char *scene_name, int kind, int frames, bool write_tga);
