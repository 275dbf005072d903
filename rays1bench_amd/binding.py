"""ctypes binding of librays1.so (include/rays1.h).  No compute happens in Python and
nothing here imports oracle/: this is the product's host-side mirror of the reference's
interface for the hot path (src/step13/rayweek1.cpp:552-719 scene builders, :845 benchmark,
src/common/common.h:36-122 RESULT / log_results / tga_write_rgb24)."""
import ctypes as C
import os
import sys
import subprocess
import time

import numpy as np

_lib = None
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")

R1_OK, R1_EINVAL, R1_ENODEVICE, R1_EHIP, R1_ENOMEM, R1_ELIMIT = 0, -1, -2, -3, -4, -5
SCENE_SMALL, SCENE_MEDIUM, SCENE_LARGE, SCENE_GRID = 0, 1, 2, 3
VARIANT_DEFAULT, VARIANT_REFERENCE, VARIANT_PREFILTER, VARIANT_STATS, VARIANT_BVH, VARIANT_BVH_STATS, VARIANT_WAVEFRONT = 0, 1, 2, 3, 4, 5, 6
VARIANT_GRID, VARIANT_GRID_STATS = 7, 8



def _stream_arg(stream_ptr):
    """hipStream_t argument of the device-pointer entry points.  0 / None means the CONTEXT'S OWN stream (a non-blocking stream: the
    library never touches the null stream), which is not ordered with torch's default stream — where a caller who passes
    torch.cuda.current_stream().cuda_stream (= 0 for the default stream) has just filled the buffers it hands over.  So for that case
    the pending work of torch's current stream is waited for here (tests and smoke only: bench.py passes streams of its own)."""
    if stream_ptr:
        return C.c_void_p(stream_ptr)
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.current_stream().synchronize()
    return None


class R1Error(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"librays1 error {code}: {text}")
        self.code = code


class CScene(C.Structure):
    _fields_ = [("count", C.c_uint32)] + [
        (n, C.POINTER(C.c_float)) for n in ("center_x", "center_y", "center_z", "radius_sq", "inv_radius")
    ] + [("mat_type", C.POINTER(C.c_uint8))] + [
        (n, C.POINTER(C.c_float)) for n in ("albedo_r", "albedo_g", "albedo_b", "mat_param")
    ]


class CCamera(C.Structure):
    _fields_ = [(n, C.c_float * 3) for n in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w")] + [
        ("lens_radius", C.c_float)
    ]


class Params(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_bounces", C.c_int32),
        ("seed", C.c_uint32), ("tile_w", C.c_int32), ("tile_h", C.c_int32),
        ("shard", C.c_int32), ("num_shards", C.c_int32), ("variant", C.c_int32),
    ]


class MultiLayout(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("block_bytes", "record_bytes", "count_offset", "send_bytes", "gathered_bytes", "frame_record_bytes",
                                          "frame_count_offset", "host_bytes", "counts_pitch")]


class LaunchInfo(C.Structure):
    _fields_ = [("compute_units", C.c_int32), ("blocks", C.c_int32), ("threads_per_block", C.c_int32),
                ("spheres_active", C.c_int32), ("spheres_padded", C.c_int32), ("groups", C.c_int32), ("samples", C.c_uint64),
                ("kernel", C.c_int32), ("bvh_nodes", C.c_int32), ("bvh_leaves", C.c_int32), ("bvh_depth", C.c_int32),
                ("tiles_in_kernel", C.c_int32)]


class BvhInfo(C.Structure):
    _fields_ = [("nodes", C.c_int32), ("leaves", C.c_int32), ("depth", C.c_int32), ("stack_entries", C.c_int32), ("spheres", C.c_int32),
                ("pairs", C.c_int32), ("centre", C.c_float * 3), ("pad_local", C.c_int32), ("root_leaf", C.c_int32),
                ("flat_axis", C.c_int32), ("flat_m", C.c_float), ("flat_e", C.c_float)]


class SphereUpdate(C.Structure):
    """r1_sphere_update: the groups of r1_update_spheres* (NULL pointers: the property stays); void pointers, host or device."""
    _fields_ = [(n, C.c_void_p) for n in ("center_x", "center_y", "center_z", "radius_sq", "inv_radius", "mat_type", "albedo_r", "albedo_g", "albedo_b",
                                          "mat_param")]


class Adaptive(C.Structure):
    """r1_adaptive: the schedule (min_spp, then pass_spp per pass, up to params.spp) and the stopping rule of r1_render_adaptive."""
    _fields_ = [("min_spp", C.c_int32), ("pass_spp", C.c_int32), ("max_delta", C.c_int32), ("mean_delta_q8", C.c_int32)]


class Region(C.Structure):
    """r1_region: a window of the frame (x0, y0: its lower-left pixel; out_stride: pixels between two rows of the output, 0 = width)."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("out_stride", C.c_int32)]


# denoised frames (r1_denoise*): the flag, the limits of the options
DENOISE_DEMODULATE = 1
DENOISE_MAX_ITERATIONS, DENOISE_MAX_POWER_LOG2 = 8, 10


class DenoiseOpt(C.Structure):
    """r1_denoise_opt: iterations 1..8, normal_power_log2 0..10, sigma_color and sigma_depth > 0 and finite, flags DENOISE_DEMODULATE or 0."""
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32)]


class DenoiseFrame(C.Structure):
    """r1_denoise_frame: the size of the three images and the pixels between two rows of each (0 = width)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("linear_stride", C.c_int32), ("feature_stride", C.c_int32), ("out_stride", C.c_int32)]


class DenoiseGuidedOpt(C.Structure):
    """r1_denoise_guided_opt: a DenoiseOpt, variance_floor > 0 and finite, reserved 0."""
    _fields_ = [("base", DenoiseOpt), ("variance_floor", C.c_float), ("reserved", C.c_uint32)]


class DenoiseGuidedFrame(C.Structure):
    """r1_denoise_guided_frame: the size of the four images and the pixels between two rows of each (0 = width)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("linear_stride", C.c_int32), ("feature_stride", C.c_int32), ("moment_stride", C.c_int32),
                ("out_stride", C.c_int32)]


def make_denoise_guided_opt(iterations=3, normal_power_log2=6, sigma_color=2.0, sigma_depth=0.1, flags=DENOISE_DEMODULATE, variance_floor=1e-4, reserved=0):
    """The options of the variance-guided filter; the defaults are the ones DESIGN.md §4.40 chose on the medium scene."""
    return DenoiseGuidedOpt(DenoiseOpt(int(iterations), int(normal_power_log2), float(sigma_color), float(sigma_depth), int(flags)), float(variance_floor), int(reserved))


class AccumulateOpt(C.Structure):
    """r1_accumulate_opt: max_samples >= 1, depth_tolerance > 0 and finite, normal_min_cos in -1 .. 1, flags 0."""
    _fields_ = [("max_samples", C.c_uint32), ("depth_tolerance", C.c_float), ("normal_min_cos", C.c_float), ("flags", C.c_uint32)]


class AccumulateFrame(C.Structure):
    """r1_accumulate_frame: the size of the eight images and the pixels between two rows of each (0 = width)."""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "linear_stride", "moment_stride", "feature_stride", "prev_stride", "prev_feature_stride",
                                         "prev_moment_stride", "out_stride", "out_moment_stride")]


class AccumulateView(C.Structure):
    """r1_accumulate_view: the cameras and the spp of the current frame and of the history."""
    _fields_ = [("camera", CCamera), ("camera_prev", CCamera), ("spp", C.c_int32), ("spp_prev", C.c_int32)]


class AccumulateImages(C.Structure):
    """r1_accumulate_images: L, V, f, A_prev, f_prev, M_prev, A_out, M_out — host or device addresses."""
    _fields_ = [(n, C.c_void_p) for n in ("L", "V", "f", "A_prev", "f_prev", "M_prev", "A_out", "M_out")]


class ReprojectPlan(C.Structure):
    """r1_reproject_plan: what one accumulation computes once for all of its pixels."""
    _fields_ = [(n, C.c_float) for n in ("pu", "pv", "pw", "hu", "vv", "inv_w", "inv_h")]


def make_accumulate_opt(max_samples=32, depth_tolerance=0.05, normal_min_cos=0.9, flags=0):
    """The options of an accumulation; the defaults are the ones DESIGN.md §4.41 chose on the medium scene."""
    return AccumulateOpt(int(max_samples), float(depth_tolerance), float(normal_min_cos), int(flags))


def make_accumulate_view(camera, camera_prev, spp, spp_prev):
    """r1_accumulate_view of two CCamera (copied) and the spp of the two renders."""
    v = AccumulateView()
    C.memmove(C.byref(v.camera), C.byref(camera), C.sizeof(CCamera))
    C.memmove(C.byref(v.camera_prev), C.byref(camera_prev), C.sizeof(CCamera))
    v.spp, v.spp_prev = int(spp), int(spp_prev)
    return v


def make_denoise_opt(iterations=3, normal_power_log2=6, sigma_color=1.0, sigma_depth=0.1, flags=DENOISE_DEMODULATE):
    """The options DESIGN.md §4.39 measured at 1-4 spp; at 16 spp and more, iterations=1."""
    return DenoiseOpt(int(iterations), int(normal_power_log2), float(sigma_color), float(sigma_depth), int(flags))


class TileReport(C.Structure):
    _fields_ = [("spp", C.c_int32), ("settled", C.c_int32), ("err_max", C.c_uint32), ("err_sum", C.c_uint32)]


class AdaptiveResult(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("passes", C.c_int32), ("tiles", C.c_int32), ("tiles_settled", C.c_int32), ("reserved", C.c_int32)]


TILE_REPORT_DTYPE = np.dtype([("spp", np.int32), ("settled", np.int32), ("err_max", np.uint32), ("err_sum", np.uint32)])
# r1_ray / r1_hit (32 bytes each) and the modes of the ray queries
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("t_max", np.float32), ("d", np.float32, 3), ("pad", np.uint32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("index", np.int32), ("p", np.float32, 3), ("n", np.float32, 3)])
CAST_CLOSEST, CAST_ANY = 0, 1
CAST_CHUNK = 1 << 20  # R1_CAST_CHUNK: rays per launch of r1_cast_rays
# r1_sample_seed / r1_radiance (16 bytes each) of the path queries
SEED_DTYPE = np.dtype([("scalar", np.uint32), ("lane0", np.uint32), ("lane1", np.uint32), ("lane2", np.uint32)])
RADIANCE_DTYPE = np.dtype([("r", np.float32), ("g", np.float32), ("b", np.float32), ("rays", np.uint32)])
TRACE_CHUNK = 1 << 20  # R1_TRACE_CHUNK: rays r1_trace_rays works through at a time
# r1_scatter (32 bytes), the events and the flag of the scatter queries
SCATTER_DTYPE = np.dtype([("weight", np.float32, 3), ("event", np.int32), ("t", np.float32), ("index", np.int32), ("mat_type", np.uint32),
                          ("pad", np.uint32)])
SCATTER_SCATTERED, SCATTER_SKY, SCATTER_ABSORBED, SCATTER_NONE = 0, 1, 2, 3
SCATTER_UNIT_DIRECTIONS = 1
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_NONE = 0, 1, 2, 255
# r1_feature (32 bytes): a pixel of a feature frame
FEATURE_DTYPE = np.dtype([("albedo", np.float32, 3), ("depth", np.float32), ("normal", np.float32, 3), ("hits", np.uint32)])
# r1_moment (16 bytes): a pixel of a variance frame
MOMENT_DTYPE = np.dtype([("var", np.float32, 3), ("samples", np.uint32)])


def make_params(width, height, spp, seed=10001, max_bounces=50, tile_w=32, tile_h=32, shard=0, num_shards=1, variant=0):
    return Params(width, height, spp, max_bounces, seed, tile_w, tile_h, shard, num_shards, variant)


_lib_path = os.path.join(LIBDIR, "librays1.so")


def lib_path():
    return _lib_path


def set_lib_path(path):
    """Explicit choice of another build of the library (bench.py --lib, tools/: e.g. lib/librays1_tuning.so, the
    -DR1_TUNING build that reads the R1_* knobs).  Must be called before the first lib(); nothing is read from the
    environment here, and the shipped file is never overwritten by an experiment."""
    global _lib_path
    if _lib is not None:
        raise R1Error(R1_EINVAL, "set_lib_path after the library was loaded")
    _lib_path = os.path.abspath(path)


def build(verbose=False):
    """Compiles librays1.so and rayweek1_hip in-tree with hipcc --offload-arch=gfx950."""
    subprocess.check_call(["make", "-j4", "-C", CSRC] + ([] if verbose else ["-s"]))


class GridInfo(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("cells", C.c_int32 * 3), ("cell", C.c_float * 3), ("pad", C.c_float),
                ("v_safe", C.c_float), ("centre_lo", C.c_float * 3), ("centre_hi", C.c_float * 3), ("spheres", C.c_int32),
                ("outliers", C.c_int32), ("registrations", C.c_int32), ("max_occupancy", C.c_int32), ("build_ms", C.c_float)]


# every symbol include/rays1.h declares: (name, restype, argtypes)
_u8p, _f32p, _u64p, _i32p, _dblp = (C.POINTER(t) for t in (C.c_uint8, C.c_float, C.c_uint64, C.c_int32, C.c_double))
_ctx = C.c_void_p
SYMBOLS = [
    ("r1_abi_version", C.c_int, []),
    ("r1_create", C.c_int, [C.c_int, C.POINTER(_ctx)]),
    ("r1_destroy", None, [_ctx]),
    ("r1_last_error", C.c_char_p, []),
    ("r1_device_count", C.c_int, []),
    ("r1_set_scene", C.c_int, [_ctx, C.POINTER(CScene), C.POINTER(CCamera)]),
    ("r1_set_camera", C.c_int, [_ctx, C.POINTER(CCamera)]),
    ("r1_render", C.c_int, [_ctx, C.POINTER(Params), _u8p, _u64p, _dblp]),
    ("r1_render_samples", C.c_int, [_ctx, C.POINTER(Params), _u8p, _u64p, _f32p]),
    ("r1_render_pass", C.c_int, [_ctx, C.POINTER(Params), C.c_int32, _u8p, _u64p]),
    ("r1_adaptive_schedule", C.c_int, [C.POINTER(Params), C.POINTER(Adaptive), _i32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r1_render_adaptive", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Adaptive), _u8p, _u64p, C.POINTER(TileReport), C.POINTER(AdaptiveResult)]),
    ("r1_tile_count", C.c_int, [C.POINTER(Params), _i32p, _i32p]),
    ("r1_shard_block_bytes", C.c_size_t, [C.POINTER(Params)]),
    ("r1_shard_record_bytes", C.c_size_t, [C.POINTER(Params)]),
    ("r1_render_async", C.c_int, [_ctx, C.POINTER(Params), _u8p, _u64p, C.c_void_p]),
    ("r1_frame_record_bytes", C.c_size_t, [C.POINTER(Params)]),
    ("r1_render_batch_async", C.c_int, [_ctx, C.POINTER(Params), C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("r1_render_path_async", C.c_int, [_ctx, C.POINTER(Params), C.c_int32, C.c_uint32, C.POINTER(CCamera), C.c_void_p, C.c_void_p]),
    ("r1_render_shard_device_batch", C.c_int, [_ctx, C.POINTER(Params), C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("r1_assemble_device_records_batch", C.c_int, [_ctx, C.POINTER(Params), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_host_alloc", C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    ("r1_host_free", None, [C.c_void_p]),
    ("r1_render_shard_device", C.c_int, [_ctx, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_set_pixel_mode", C.c_int, [_ctx, C.c_int32]),
    ("r1_render_shard_device_once", C.c_int, [_ctx, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_multi_create", C.c_int, [C.c_int32, _i32p, C.POINTER(C.c_void_p)]),
    ("r1_multi_destroy", None, [C.c_void_p]),
    ("r1_multi_set_scene", C.c_int, [C.c_void_p, C.POINTER(CScene), C.POINTER(CCamera)]),
    ("r1_multi_set_camera", C.c_int, [C.c_void_p, C.POINTER(CCamera)]),
    ("r1_multi_render", C.c_int, [C.c_void_p, C.POINTER(Params), _u8p, _u64p, _dblp]),
    ("r1_multi_render_async", C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p]),
    ("r1_multi_render_batch_async", C.c_int, [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_uint32, C.c_void_p]),
    ("r1_multi_sync", C.c_int, [C.c_void_p]),
    ("r1_multi_layout", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    ("r1_multi_info", C.c_int, [C.c_void_p, _i32p, _i32p, C.POINTER(LaunchInfo)]),
    ("r1_assemble_device", C.c_int, [_ctx, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_assemble_device_strided", C.c_int, [_ctx, C.POINTER(Params), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("r1_assemble_device_records", C.c_int, [_ctx, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_sync", C.c_int, [_ctx]),
    ("r1_last_timing", C.c_int, [_ctx, _dblp, _dblp]),
    ("r1_timing_begin", C.c_int, [_ctx, C.c_int32]),
    ("r1_timing_end", C.c_int, [_ctx, _dblp, _dblp, _i32p]),
    ("r1_last_stats", C.c_int, [_ctx, _u64p]),
    ("r1_last_launch_info", C.c_int, [_ctx, C.POINTER(LaunchInfo)]),
    ("r1_last_walk_form", C.c_int, [_ctx]),
    ("r1_last_wave_log", C.c_int, [_ctx, _u64p, C.c_size_t, C.POINTER(C.c_uint32)]),
    ("r1_host_scene_create", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ("r1_host_scene_destroy", None, [C.c_void_p]),
    ("r1_host_scene_spheres", C.POINTER(CScene), [C.c_void_p]),
    ("r1_host_scene_camera", C.POINTER(CCamera), [C.c_void_p]),
    ("r1_host_scene_view", C.c_int, [C.c_void_p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
    ("r1_camera_look_at", C.c_int, [_f32p, _f32p, _f32p, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(CCamera)]),
    ("r1_bvh_describe", C.c_int, [C.POINTER(CScene), C.c_int32, C.POINTER(BvhInfo), _f32p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]),
    ("r1_update_centers", C.c_int, [_ctx, C.c_uint32, C.c_uint32, _f32p, _f32p, _f32p, C.c_void_p]),
    ("r1_update_centers_device", C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_bvh_refit_describe", C.c_int, [C.POINTER(CScene), _f32p, _f32p, _f32p, C.c_int32, C.POINTER(BvhInfo), _f32p, C.c_size_t]),
    ("r1_update_spheres", C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.POINTER(SphereUpdate), C.c_void_p]),
    ("r1_update_spheres_device", C.c_int, [_ctx, C.c_uint32, C.c_uint32, C.POINTER(SphereUpdate), C.c_void_p]),
    ("r1_bvh_refit_describe_spheres", C.c_int, [C.POINTER(CScene), _f32p, _f32p, _f32p, _f32p, _f32p, C.c_int32, C.POINTER(BvhInfo), _f32p, C.c_size_t]),
    ("r1_tables_download", C.c_int, [_ctx, _f32p, _f32p, C.POINTER(C.c_uint32), _dblp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r1_bvh_download", C.c_int, [_ctx, _f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r1_resort_spheres", C.c_int, [_ctx, C.c_void_p]),
    ("r1_bvh_ids_download", C.c_int, [_ctx, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("r1_bvh_resort_describe", C.c_int, [C.POINTER(CScene), _f32p, _f32p, _f32p, _f32p, _f32p, C.c_int32, C.POINTER(BvhInfo), _f32p, C.c_size_t,
                                         C.POINTER(C.c_uint32), C.c_size_t]),
    ("r1_grid_describe", C.c_int, [C.POINTER(CScene), C.POINTER(GridInfo), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t,
                                   C.POINTER(C.c_uint32), C.c_size_t]),
    ("r1_grid_visit", C.c_int, [C.POINTER(CScene), _f32p, _f32p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t), _i32p, _f32p, _i32p]),
    ("r1_regrid", C.c_int, [_ctx, C.c_void_p]),
    ("r1_grid_download", C.c_int, [_ctx, C.POINTER(GridInfo), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t,
                                   C.POINTER(C.c_uint32), C.c_size_t]),
    ("r1_grid_regrid_describe", C.c_int, [C.POINTER(CScene), _f32p, _f32p, _f32p, _f32p, _f32p, C.POINTER(GridInfo), C.POINTER(C.c_uint32), C.c_size_t,
                                          C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]),
    ("r1_grid_regrid_visit", C.c_int, [C.POINTER(CScene), _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, C.POINTER(C.c_uint32), C.c_size_t,
                                       C.POINTER(C.c_size_t), _i32p, _f32p, _i32p]),
    ("r1_cast_rays", C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("r1_cast_rays_device", C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("r1_cast_rays_host", C.c_int, [C.POINTER(CScene), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("r1_trace_rays", C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("r1_trace_rays_device", C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("r1_trace_rays_host", C.c_int, [C.POINTER(CScene), C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("r1_camera_rays", C.c_int, [C.POINTER(CCamera), C.POINTER(Params), _i32p, _i32p, _i32p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("r1_camera_rays_device", C.c_int, [_ctx, C.POINTER(CCamera), C.POINTER(Params), C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_scatter_rays", C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_scatter_rays_device", C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_scatter_rays_host", C.c_int, [C.POINTER(CScene), C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_render_linear", C.c_int, [_ctx, C.POINTER(Params), _f32p, _u64p, _dblp]),
    ("r1_render_linear_async", C.c_int, [_ctx, C.POINTER(Params), _f32p, _u64p, C.c_void_p]),
    ("r1_render_linear_device", C.c_int, [_ctx, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_pass_linear", C.c_int, [_ctx, _f32p, _i32p]),
    ("r1_render_adaptive_linear", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Adaptive), _f32p, _u64p, C.POINTER(TileReport), C.POINTER(AdaptiveResult)]),
    ("r1_quantise_linear", C.c_int, [_f32p, C.c_size_t, _u8p]),
    ("r1_render_linear_host", C.c_int, [C.POINTER(CScene), C.POINTER(CCamera), C.POINTER(Params), _f32p, _u64p]),
    ("r1_render_moments", C.c_int, [_ctx, C.POINTER(Params), _f32p, C.c_void_p, _u64p, _dblp]),
    ("r1_render_moments_device", C.c_int, [_ctx, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_render_moments_host", C.c_int, [C.POINTER(CScene), C.POINTER(CCamera), C.POINTER(Params), _f32p, C.c_void_p, _u64p]),
    ("r1_region_check", C.c_int, [C.POINTER(Params), C.POINTER(Region)]),
    ("r1_render_region", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Region), C.c_void_p, _u64p, _dblp]),
    ("r1_render_region_samples", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Region), C.c_void_p, _u64p, _f32p]),
    ("r1_render_region_linear", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Region), C.c_void_p, _u64p, _dblp]),
    ("r1_render_region_device", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Region), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_render_region_host", C.c_int, [C.POINTER(CScene), C.POINTER(CCamera), C.POINTER(Params), C.POINTER(Region), C.c_void_p, _u64p]),
    ("r1_render_features", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Region), C.c_void_p, _dblp]),
    ("r1_render_features_device", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(Region), C.c_void_p, C.c_void_p]),
    ("r1_render_features_host", C.c_int, [C.POINTER(CScene), C.POINTER(CCamera), C.POINTER(Params), C.POINTER(Region), C.c_void_p]),
    ("r1_denoise_check", C.c_int, [C.POINTER(DenoiseFrame), C.POINTER(DenoiseOpt)]),
    ("r1_denoise_host", C.c_int, [C.POINTER(DenoiseFrame), C.POINTER(DenoiseOpt), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_denoise_device", C.c_int, [_ctx, C.POINTER(DenoiseFrame), C.POINTER(DenoiseOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_denoise", C.c_int, [_ctx, C.POINTER(DenoiseFrame), C.POINTER(DenoiseOpt), C.c_void_p, C.c_void_p, C.c_void_p, _dblp]),
    ("r1_render_denoised", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(DenoiseOpt), C.c_void_p, _u64p, _dblp]),
    ("r1_render_denoised_device", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(DenoiseOpt), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_denoise_guided_check", C.c_int, [C.POINTER(DenoiseGuidedFrame), C.POINTER(DenoiseGuidedOpt)]),
    ("r1_denoise_guided_host", C.c_int, [C.POINTER(DenoiseGuidedFrame), C.POINTER(DenoiseGuidedOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_denoise_guided_device", C.c_int, [_ctx, C.POINTER(DenoiseGuidedFrame), C.POINTER(DenoiseGuidedOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_denoise_guided", C.c_int, [_ctx, C.POINTER(DenoiseGuidedFrame), C.POINTER(DenoiseGuidedOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dblp]),
    ("r1_render_denoised_guided", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(DenoiseGuidedOpt), C.c_void_p, _u64p, _dblp]),
    ("r1_render_denoised_guided_device", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(DenoiseGuidedOpt), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_accumulate_check", C.c_int, [C.POINTER(AccumulateFrame), C.POINTER(AccumulateOpt), C.POINTER(AccumulateView), C.POINTER(ReprojectPlan)]),
    ("r1_accumulate_host", C.c_int, [C.POINTER(AccumulateFrame), C.POINTER(AccumulateOpt), C.POINTER(AccumulateView), C.POINTER(AccumulateImages)]),
    ("r1_accumulate_device", C.c_int, [_ctx, C.POINTER(AccumulateFrame), C.POINTER(AccumulateOpt), C.POINTER(AccumulateView), C.POINTER(AccumulateImages), C.c_void_p]),
    ("r1_accumulate", C.c_int, [_ctx, C.POINTER(AccumulateFrame), C.POINTER(AccumulateOpt), C.POINTER(AccumulateView), C.POINTER(AccumulateImages), _dblp]),
    ("r1_render_accumulated", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(AccumulateOpt), C.POINTER(DenoiseGuidedOpt), C.c_void_p, _u64p, _dblp]),
    ("r1_render_accumulated_device", C.c_int, [_ctx, C.POINTER(Params), C.POINTER(AccumulateOpt), C.POINTER(DenoiseGuidedOpt), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("r1_accumulate_reset", C.c_int, [_ctx]),
    ("r1_pfm_write_rgb32f", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, _f32p]),
    ("r1_tga_write_rgb24", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, _u8p]),
    ("r1_log_results", C.c_int, [C.c_char_p, C.c_char_p, _dblp, _u64p, C.c_int32]),
]


def lib():
    """Loads librays1.so (fails loudly if it has not been built: no fallback)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise R1Error(R1_ENODEVICE, f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                        "(there is no CPU fallback)")
        L = C.CDLL(p)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != R1_OK:
        raise R1Error(rc, lib().r1_last_error().decode(errors="replace"))


def device_count():
    n = lib().r1_device_count()
    return max(n, 0)


class Scene:
    """Host scene = what create_*_scene() returns in the reference (Scene{camera, hitables},
    rayweek1.cpp:539-549), flattened; owns the native r1_host_scene."""

    def __init__(self, kind, width, height, grid_w=0, grid_h=0, name=None):
        self._h = C.c_void_p()
        _check(lib().r1_host_scene_create(kind, width, height, grid_w, grid_h, C.byref(self._h)))
        self.kind, self.width, self.height = kind, width, height
        self.name = name or {0: "small", 1: "medium", 2: "large", 3: "grid"}[kind]
        self.spheres = lib().r1_host_scene_spheres(self._h)
        self.camera = lib().r1_host_scene_camera(self._h)

    @property
    def count(self):
        return int(self.spheres.contents.count)

    def arrays(self):
        s = self.spheres.contents
        n = s.count
        out = {k: np.ctypeslib.as_array(getattr(s, k), shape=(n,)).copy() for k in
               ("center_x", "center_y", "center_z", "radius_sq", "inv_radius", "albedo_r", "albedo_g", "albedo_b", "mat_param")}
        out["mat_type"] = np.ctypeslib.as_array(s.mat_type, shape=(n,)).copy()
        return out

    def camera_array(self):
        c = self.camera.contents
        return np.array(sum([list(getattr(c, f)) for f in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w")], [])
                        + [c.lens_radius], dtype=np.float32)

    def view(self):
        """r1_host_scene_view: the arguments the builder gave Camera::init, as a dict ready for camera_look_at (aspect: this
        scene's width / height in fp32, rayweek1.cpp:564)."""
        v = [(C.c_float * 3)() for _ in range(3)]
        s = [C.c_float() for _ in range(3)]
        _check(lib().r1_host_scene_view(self._h, v[0], v[1], v[2], C.byref(s[0]), C.byref(s[1]), C.byref(s[2])))
        return {"lookfrom": np.array(list(v[0]), np.float32), "lookat": np.array(list(v[1]), np.float32), "vup": np.array(list(v[2]), np.float32),
                "vfov": np.float32(s[0].value), "aspect": np.float32(self.width) / np.float32(self.height), "aperture": np.float32(s[1].value),
                "focus_dist": np.float32(s[2].value)}

    def close(self):
        if self._h:
            lib().r1_host_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_look_at(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist):
    """r1_camera_look_at: Camera::init (rayweek1.cpp:366-379) in the reference's arithmetic; returns a CCamera."""
    a = [np.ascontiguousarray(x, np.float32) for x in (lookfrom, lookat, vup)]
    if any(x.shape != (3,) for x in a):
        raise R1Error(R1_EINVAL, "camera_look_at: lookfrom, lookat and vup are 3-vectors")
    out = CCamera()
    _check(lib().r1_camera_look_at(a[0].ctypes.data_as(_f32p), a[1].ctypes.data_as(_f32p), a[2].ctypes.data_as(_f32p), float(vfov), float(aspect),
                                   float(aperture), float(focus_dist), C.byref(out)))
    return out


def orbit_cameras(scene, n, view=None):
    """n cameras of `scene` turned about the vertical axis through lookat, camera f at angle 2 pi f / n — rayweek1_hip --orbit's
    arithmetic (fp32; camera 0 is the scene's own camera bit for bit: cos 0 = 1, sin 0 = 0).  `view` overrides entries of scene.view()."""
    v = scene.view()
    v.update(view or {})
    f32 = np.float32
    out = []
    for f in range(n):
        a = 2.0 * np.pi * f / n
        cs, sn = f32(np.cos(a)), f32(np.sin(a))
        dx, dz = f32(v["lookfrom"][0] - v["lookat"][0]), f32(v["lookfrom"][2] - v["lookat"][2])
        eye = np.array([v["lookat"][0] + f32(f32(dx * cs) + f32(dz * sn)), v["lookfrom"][1], v["lookat"][2] + f32(f32(dz * cs) - f32(dx * sn))], f32)
        out.append(camera_look_at(eye, v["lookat"], v["vup"], v["vfov"], v["aspect"], v["aperture"], v["focus_dist"]))
    return out


def camera_to_array(cam):
    """The 22 floats of a CCamera, in the order of Scene.camera_array()."""
    return np.array(sum([list(getattr(cam, f)) for f in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w")], []) + [cam.lens_radius],
                    dtype=np.float32)


def create_small_scene(width=1280, height=720):
    return Scene(SCENE_SMALL, width, height)


def create_medium_scene(width=1280, height=720):
    return Scene(SCENE_MEDIUM, width, height)


def create_large_scene(width=1280, height=720):
    return Scene(SCENE_LARGE, width, height)


def adaptive_schedule(params, min_spp, pass_spp, max_delta=-1, mean_delta_q8=0):
    """r1_adaptive_schedule: the cumulative sample counts after every pass of r1_render_adaptive (raises R1Error as that call would)."""
    opt = Adaptive(min_spp, pass_spp, max_delta, mean_delta_q8)
    n = C.c_size_t()
    _check(lib().r1_adaptive_schedule(C.byref(params), C.byref(opt), None, 0, C.byref(n)))
    out = (C.c_int32 * n.value)()
    _check(lib().r1_adaptive_schedule(C.byref(params), C.byref(opt), out, n.value, C.byref(n)))
    return list(out)


def create_grid_scene(width, height, grid_w, grid_h):
    return Scene(SCENE_GRID, width, height, grid_w, grid_h)


_SPHERE_GROUPS = (("center_x", "center_y", "center_z"), ("radius_sq", "inv_radius"), ("mat_type", "albedo_r", "albedo_g", "albedo_b", "mat_param"))


def _sphere_update(who, centers, radii, materials, pointer_of):
    """A SphereUpdate from the three groups (None: the group's pointers stay NULL); pointer_of(field, value) gives each array's address."""
    if centers is None and radii is None and materials is None:
        raise R1Error(R1_EINVAL, f"{who}: every group is None")
    u = SphereUpdate()
    for group, fields in zip((centers, radii, materials), _SPHERE_GROUPS):
        if group is None:
            continue
        if len(group) != len(fields):
            raise R1Error(R1_EINVAL, f"{who}: {len(fields)} arrays for {fields}")
        for k, v in zip(fields, group):
            setattr(u, k, pointer_of(k, v))
    return u


class Renderer:
    """One r1_context (device, stream, cached scene + workspace)."""

    def __init__(self, device=0):
        self._c = _ctx()
        _check(lib().r1_create(device, C.byref(self._c)))
        self.device = device

    def set_scene(self, scene):
        _check(lib().r1_set_scene(self._c, scene.spheres, scene.camera))

    def set_scene_raw(self, cscene, ccamera):
        _check(lib().r1_set_scene(self._c, C.byref(cscene), C.byref(ccamera)))

    def set_camera(self, ccamera):
        """r1_set_camera: the camera alone (nothing is built, uploaded or waited for)."""
        _check(lib().r1_set_camera(self._c, C.byref(ccamera)))

    def update_centers(self, first, x, y, z, stream_ptr=None):
        """r1_update_centers: new centres for the spheres [first, first + len(x)) of the scene (scene indices, placeholders counted), host
        arrays; the box tree is refitted on the device.  Enqueues on `stream_ptr` (None: the context's stream)."""
        x, y, z = (np.ascontiguousarray(v, np.float32) for v in (x, y, z))
        if not (x.ndim == 1 and x.shape == y.shape == z.shape):
            raise R1Error(R1_EINVAL, "update_centers: x, y and z must be one-dimensional and of one length")
        _check(lib().r1_update_centers(self._c, first, x.shape[0], x.ctypes.data_as(_f32p), y.ctypes.data_as(_f32p), z.ctypes.data_as(_f32p),
                                       C.c_void_p(stream_ptr) if stream_ptr else None))

    def update_centers_device(self, first, count, d_x_ptr, d_y_ptr, d_z_ptr, stream_ptr=None):
        """r1_update_centers_device: the same from three device pointers to `count` floats each; waits for nothing."""
        _check(lib().r1_update_centers_device(self._c, first, count, C.c_void_p(d_x_ptr), C.c_void_p(d_y_ptr), C.c_void_p(d_z_ptr),
                                              _stream_arg(stream_ptr)))

    def update_spheres(self, first, centers=None, radii=None, materials=None, stream_ptr=None):
        """r1_update_spheres: new values for the spheres [first, first + n) of the scene (scene indices, placeholders counted), host arrays of
        one length n.  centers = (x, y, z); radii = (radius_sq, inv_radius); materials = (mat_type, albedo_r, albedo_g, albedo_b, mat_param);
        None: the property stays (all three None: R1_EINVAL, as the C call refuses an update without a group).  A change of centre or radius
        refits the box tree on the device; materials alone change no index.  Enqueues on `stream_ptr` (None: the context's stream)."""
        keep, n = [], None

        def host_array(k, v):
            nonlocal n
            v = np.ascontiguousarray(v, np.uint8 if k == "mat_type" else np.float32)
            if v.ndim != 1 or (n is not None and v.shape[0] != n):
                raise R1Error(R1_EINVAL, "update_spheres: every array must be one-dimensional and of one length")
            n = v.shape[0]
            keep.append(v)
            return v.ctypes.data

        u = _sphere_update("update_spheres", centers, radii, materials, host_array)
        _check(lib().r1_update_spheres(self._c, first, n, C.byref(u), C.c_void_p(stream_ptr) if stream_ptr else None))

    def update_spheres_device(self, first, count, centers=None, radii=None, materials=None, stream_ptr=None):
        """r1_update_spheres_device: the same from device pointers (ints) to `count` entries each, grouped as for update_spheres; waits for
        nothing."""
        u = _sphere_update("update_spheres_device", centers, radii, materials, lambda k, v: int(v))
        _check(lib().r1_update_spheres_device(self._c, first, count, C.byref(u), _stream_arg(stream_ptr)))

    def tables_download(self):
        """r1_tables_download: the device's rows of the active spheres, in active order (diagnostic, synchronous): {"exact": float32[n, 4],
        "shade": float32[n, 4], "mat": uint32[n, 4], "radii": float64[n, 2]}."""
        n = C.c_size_t()
        _check(lib().r1_tables_download(self._c, None, None, None, None, 0, C.byref(n)))
        t = {"exact": np.zeros((n.value, 4), np.float32), "shade": np.zeros((n.value, 4), np.float32), "mat": np.zeros((n.value, 4), np.uint32),
             "radii": np.zeros((n.value, 2), np.float64)}
        _check(lib().r1_tables_download(self._c, t["exact"].ctypes.data_as(_f32p), t["shade"].ctypes.data_as(_f32p),
                                        t["mat"].ctypes.data_as(C.POINTER(C.c_uint32)), t["radii"].ctypes.data_as(_dblp), n.value, C.byref(n)))
        return t

    def bvh_download(self):
        """r1_bvh_download: the box tree's node rows as the device holds them, float32[n, 16] (diagnostic, synchronous)."""
        n = C.c_size_t()
        _check(lib().r1_bvh_download(self._c, None, 0, C.byref(n)))
        nodes = np.zeros((n.value, 16), np.float32)
        _check(lib().r1_bvh_download(self._c, nodes.ctypes.data_as(_f32p), nodes.size, C.byref(n)))
        return nodes

    def resort_spheres(self, stream=None):
        """r1_resort_spheres: the spheres re-dealt into the box tree's leaves on the device, then the refit; the topology stays.  Enqueues on
        `stream` (a stream pointer; None: the context's stream) and waits for nothing."""
        _check(lib().r1_resort_spheres(self._c, _stream_arg(stream)))

    def regrid(self, stream=None):
        """r1_regrid: the spheres the device holds re-registered in the uniform grid on the device; GRID renders and queries are accepted
        again.  Enqueues on `stream` (a stream pointer; None: the context's stream) and waits for nothing."""
        _check(lib().r1_regrid(self._c, _stream_arg(stream)))

    def grid_download(self):
        """r1_grid_download: the grid as the device holds it, as grid_describe returns it (diagnostic, synchronous); overflow:
        info["registrations"] == -1."""
        return _grid_tables(lambda *a: lib().r1_grid_download(self._c, *a))

    def bvh_ids_download(self):
        """r1_bvh_ids_download: the tree's leaf slots as the device holds them, uint32 scene indices, 0xFFFFFFFF = empty (diagnostic,
        synchronous)."""
        n = C.c_size_t()
        _check(lib().r1_bvh_ids_download(self._c, None, 0, C.byref(n)))
        ids = np.zeros(max(n.value, 1), np.uint32)
        _check(lib().r1_bvh_ids_download(self._c, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, C.byref(n)))
        return ids[:n.value]

    def render(self, params):
        img = np.zeros((params.height, params.width, 3), np.uint8)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render(self._c, C.byref(params), img.ctypes.data_as(_u8p), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), float(secs.value)

    def render_into(self, params, img):
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render(self._c, C.byref(params), img.ctypes.data_as(_u8p), C.byref(rays), C.byref(secs)))
        return int(rays.value), float(secs.value)

    def render_samples(self, params):
        img = np.zeros((params.height, params.width, 3), np.uint8)
        samples = np.zeros((params.height * params.width * params.spp, 4), np.float32)
        rays = C.c_uint64()
        _check(lib().r1_render_samples(self._c, C.byref(params), img.ctypes.data_as(_u8p), C.byref(rays), samples.ctypes.data_as(_f32p)))
        return img, int(rays.value), samples

    def render_pass(self, params, first_sample, image=True):
        """r1_render_pass: samples [first_sample, first_sample + params.spp) added to the context's accumulator.  Returns
        (preview of samples [0, first_sample + params.spp) or None, cumulative ray count)."""
        img = np.zeros((params.height, params.width, 3), np.uint8) if image else None
        rays = C.c_uint64()
        _check(lib().r1_render_pass(self._c, C.byref(params), first_sample, img.ctypes.data_as(_u8p) if image else None, C.byref(rays)))
        return img, int(rays.value)

    def render_adaptive(self, params, min_spp, pass_spp, max_delta, mean_delta_q8, out=None):
        """r1_render_adaptive (params.spp is the cap).  Returns (image, ray count, the tiles' reports as a structured array — fields spp,
        settled, err_max, err_sum; tile t = ty * tiles_x + tx —, {"samples", "passes", "tiles", "tiles_settled"}).  `out`: a uint8 array
        of height x width x 3 to render into (page-locked memory, for instance)."""
        img = np.zeros((params.height, params.width, 3), np.uint8) if out is None else out
        opt = Adaptive(min_spp, pass_spp, max_delta, mean_delta_q8)
        total = C.c_int32()
        _check(lib().r1_tile_count(C.byref(params), C.byref(total), None))
        tiles = np.zeros(total.value, TILE_REPORT_DTYPE)
        rays, res = C.c_uint64(), AdaptiveResult()
        _check(lib().r1_render_adaptive(self._c, C.byref(params), C.byref(opt), img.ctypes.data_as(_u8p), C.byref(rays),
                                        tiles.ctypes.data_as(C.POINTER(TileReport)), C.byref(res)))
        return img, int(rays.value), tiles, {"samples": int(res.samples), "passes": int(res.passes), "tiles": int(res.tiles),
                                            "tiles_settled": int(res.tiles_settled)}

    def render_linear(self, params, out=None):
        """r1_render_linear: the frame as fp32 radiance, float32 (height, width, 3) — the value r1_render's bytes are quantised from.
        Returns (linear frame, ray count, device seconds).  `out`: a float32 array of that shape to render into."""
        img = np.zeros((params.height, params.width, 3), np.float32) if out is None else out
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render_linear(self._c, C.byref(params), img.ctypes.data_as(_f32p), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), float(secs.value)

    def render_moments(self, params):
        """r1_render_moments: the linear frame and the variance of every pixel's mean.  Returns (float32 (height, width, 3) — render_linear's
        frame bit for bit —, MOMENT_DTYPE array (height, width), ray count, device seconds)."""
        img = np.zeros((params.height, params.width, 3), np.float32)
        mom = np.zeros((params.height, params.width), MOMENT_DTYPE)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render_moments(self._c, C.byref(params), img.ctypes.data_as(_f32p), C.c_void_p(mom.ctypes.data), C.byref(rays), C.byref(secs)))
        return img, mom, int(rays.value), float(secs.value)

    def render_moments_device(self, params, d_rgb_f32_ptr, d_moments_ptr, d_rays_ptr, stream_ptr=None):
        """r1_render_moments_device: the same into device memory (width * height * 3 floats; width * height 16-byte records, 16-byte
        aligned; one uint64); enqueued on stream_ptr, waits for nothing."""
        _check(lib().r1_render_moments_device(self._c, C.byref(params), C.c_void_p(d_rgb_f32_ptr or None), C.c_void_p(d_moments_ptr or None),
                                              C.c_void_p(d_rays_ptr or None), _stream_arg(stream_ptr)))

    def render_region(self, params, region, out=None):
        """r1_render_region: window `region` = (x0, y0, width, height) of the frame `params` describes, byte for byte the crop of
        render(params).  Returns (uint8 (height, width, 3) of the region, ray count of the region's samples, device seconds).  `out`: a
        uint8 array of that shape to render into; it may be a view into a larger image (rows a multiple of three bytes apart), whose
        row pitch becomes the region's out_stride — out=frame[y0:y0 + h, x0:x0 + w] patches the window into a whole frame."""
        rg, img = _region_target(region, out, np.uint8)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render_region(self._c, C.byref(params), C.byref(rg), C.c_void_p(img.ctypes.data), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), float(secs.value)

    def render_region_samples(self, params, region, out=None):
        """r1_render_region_samples: render_region plus the records of the region's samples, float32 (height * width * spp, 4) in the
        region's own order ((y * width + x) * spp + s).  Returns (image, ray count, records)."""
        rg, img = _region_target(region, out, np.uint8)
        samples = np.zeros((max(rg.height, 0) * max(rg.width, 0) * max(params.spp, 0), 4), np.float32)
        rays = C.c_uint64()
        _check(lib().r1_render_region_samples(self._c, C.byref(params), C.byref(rg), C.c_void_p(img.ctypes.data), C.byref(rays), samples.ctypes.data_as(_f32p)))
        return img, int(rays.value), samples

    def render_region_linear(self, params, region, out=None):
        """r1_render_region_linear: the region as fp32 radiance, bit for bit the crop of render_linear(params).  Returns (float32
        (height, width, 3), ray count, device seconds).  `out`: as for render_region, a float32 array or view."""
        rg, img = _region_target(region, out, np.float32)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render_region_linear(self._c, C.byref(params), C.byref(rg), C.c_void_p(img.ctypes.data), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), float(secs.value)

    def render_region_device(self, params, region, d_rgb_u8_ptr, d_rgb_f32_ptr, d_rays_ptr, out_stride=0, stream_ptr=None):
        """r1_render_region_device: the region into device memory — bytes at d_rgb_u8_ptr, floats at d_rgb_f32_ptr (either may be None / 0),
        rows out_stride pixels apart (0 = the region's width), and one uint64 at d_rays_ptr; waits for nothing."""
        rg = Region(*[int(v) for v in region], int(out_stride))
        _check(lib().r1_render_region_device(self._c, C.byref(params), C.byref(rg), C.c_void_p(d_rgb_u8_ptr or None), C.c_void_p(d_rgb_f32_ptr or None),
                                             C.c_void_p(d_rays_ptr or None), _stream_arg(stream_ptr)))

    def render_features(self, params, region=None, out=None):
        """r1_render_features: first-hit albedo, normal, depth and hit count per pixel of the frame `params` describes, or of its window
        `region` = (x0, y0, width, height); params.variant chooses tree, grid or reference form.  Returns (FEATURE_DTYPE array (height,
        width), device seconds).  `out`: a FEATURE_DTYPE array or view of that shape whose rows lie whole records apart — that pitch
        becomes the region's out_stride, and nothing between the rows is written."""
        rg, img = _feature_target(params, region, out)
        secs = C.c_double()
        _check(lib().r1_render_features(self._c, C.byref(params), C.byref(rg) if rg is not None else None, C.c_void_p(img.ctypes.data), C.byref(secs)))
        return img, secs.value

    def render_features_device(self, params, d_out_ptr, region=None, stream_ptr=None, out_stride=0):
        """r1_render_features_device: the same into device memory at d_out_ptr (16-byte aligned), rows out_stride records apart (0 = the
        window's width); enqueued on stream_ptr, waits for nothing."""
        if region is None and not out_stride:
            rg = None
        else:
            x0, y0, w, h = (int(v) for v in region) if region is not None else (0, 0, params.width, params.height)
            rg = Region(x0, y0, w, h, int(out_stride))
        _check(lib().r1_render_features_device(self._c, C.byref(params), C.byref(rg) if rg is not None else None, C.c_void_p(d_out_ptr or None),
                                               _stream_arg(stream_ptr)))

    def denoise(self, L, f, opt, out=None):
        """r1_denoise: the a-trous filter of the linear frame L (float32 (height, width, 3)) guided by the feature frame f (FEATURE_DTYPE
        (height, width)), host memory, synchronous.  Arrays or views whose rows lie whole pixels apart: the pitches become the frame's
        strides.  `out`: None (a new dense array), or such an array — L itself for in place.  Returns (out, device seconds of the filter)."""
        fr, L, f, out = _denoise_target(L, f, out)
        secs = C.c_double()
        _check(lib().r1_denoise(self._c, C.byref(fr), C.byref(opt), C.c_void_p(L.ctypes.data), C.c_void_p(f.ctypes.data), C.c_void_p(out.ctypes.data), C.byref(secs)))
        return out, secs.value

    def denoise_device(self, width, height, opt, d_L_ptr, d_f_ptr, d_out_ptr, stream_ptr=None, linear_stride=0, feature_stride=0, out_stride=0):
        """r1_denoise_device: the same on device memory (d_L and d_out 4-byte aligned, d_f 16-byte aligned, d_out may be d_L; strides in
        pixels, 0 = width); enqueued on stream_ptr, waits for nothing.  One denoise per context in flight."""
        fr = DenoiseFrame(int(width), int(height), int(linear_stride), int(feature_stride), int(out_stride))
        _check(lib().r1_denoise_device(self._c, C.byref(fr), C.byref(opt), C.c_void_p(d_L_ptr or None), C.c_void_p(d_f_ptr or None), C.c_void_p(d_out_ptr or None),
                                       _stream_arg(stream_ptr)))

    def render_denoised(self, params, opt):
        """r1_render_denoised: the frame rendered (r1_render_linear), its feature frame and the filter, on the device.  Returns (float32
        (height, width, 3), ray count, device seconds of all three)."""
        img = np.zeros((max(params.height, 1), max(params.width, 1), 3), np.float32)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render_denoised(self._c, C.byref(params), C.byref(opt), C.c_void_p(img.ctypes.data), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), secs.value

    def render_denoised_device(self, params, opt, d_rgb_f32_ptr, d_rays_ptr, stream_ptr=None):
        """r1_render_denoised_device: the same into device memory (width * height * 3 floats, and one uint64); waits for nothing."""
        _check(lib().r1_render_denoised_device(self._c, C.byref(params), C.byref(opt), C.c_void_p(d_rgb_f32_ptr or None), C.c_void_p(d_rays_ptr or None),
                                               _stream_arg(stream_ptr)))

    def denoise_guided(self, L, f, V, opt, out=None):
        """r1_denoise_guided: the variance-guided filter of L guided by f and the variance frame V (MOMENT_DTYPE (height, width)), host memory,
        synchronous; arrays and `out` as for denoise.  Returns (out, device seconds of the filter)."""
        fr, L, f, V, out = _denoise_guided_target(L, f, V, out)
        secs = C.c_double()
        _check(lib().r1_denoise_guided(self._c, C.byref(fr), C.byref(opt), C.c_void_p(L.ctypes.data), C.c_void_p(f.ctypes.data), C.c_void_p(V.ctypes.data),
                                       C.c_void_p(out.ctypes.data), C.byref(secs)))
        return out, secs.value

    def denoise_guided_device(self, width, height, opt, d_L_ptr, d_f_ptr, d_V_ptr, d_out_ptr, stream_ptr=None, linear_stride=0, feature_stride=0, moment_stride=0,
                              out_stride=0):
        """r1_denoise_guided_device: the same on device memory (d_L and d_out 4-byte aligned, d_f and d_V 16-byte aligned, d_out may be d_L;
        strides in pixels, 0 = width); enqueued on stream_ptr, waits for nothing.  One denoise per context in flight."""
        fr = DenoiseGuidedFrame(int(width), int(height), int(linear_stride), int(feature_stride), int(moment_stride), int(out_stride))
        _check(lib().r1_denoise_guided_device(self._c, C.byref(fr), C.byref(opt), C.c_void_p(d_L_ptr or None), C.c_void_p(d_f_ptr or None), C.c_void_p(d_V_ptr or None),
                                              C.c_void_p(d_out_ptr or None), _stream_arg(stream_ptr)))

    def render_denoised_guided(self, params, opt):
        """r1_render_denoised_guided: the frame rendered with its variance frame, its feature frame and the guided filter, on the device.
        Returns (float32 (height, width, 3), ray count, device seconds of all three).  spp >= 2."""
        img = np.zeros((max(params.height, 1), max(params.width, 1), 3), np.float32)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render_denoised_guided(self._c, C.byref(params), C.byref(opt), C.c_void_p(img.ctypes.data), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), secs.value

    def render_denoised_guided_device(self, params, opt, d_rgb_f32_ptr, d_rays_ptr, stream_ptr=None):
        """r1_render_denoised_guided_device: the same into device memory (width * height * 3 floats, and one uint64); waits for nothing."""
        _check(lib().r1_render_denoised_guided_device(self._c, C.byref(params), C.byref(opt), C.c_void_p(d_rgb_f32_ptr or None), C.c_void_p(d_rays_ptr or None),
                                                      _stream_arg(stream_ptr)))

    def accumulate(self, L, V, f, A_prev, f_prev, M_prev, view, opt, A_out=None, M_out=None):
        """r1_accumulate: the accumulation of the frame (L, V, f) against the history (A_prev, f_prev, M_prev), host memory, synchronous;
        arrays and outputs as for accumulate_host.  Returns (A_out, M_out, device seconds of the kernel)."""
        fr, im, A_out, M_out, keep = _accumulate_target(L, V, f, A_prev, f_prev, M_prev, A_out, M_out)
        secs = C.c_double()
        _check(lib().r1_accumulate(self._c, C.byref(fr), C.byref(opt), C.byref(view), C.byref(im), C.byref(secs)))
        return A_out, M_out, secs.value

    def accumulate_device(self, width, height, view, opt, d_L_ptr, d_V_ptr, d_f_ptr, d_A_prev_ptr, d_f_prev_ptr, d_M_prev_ptr, d_A_out_ptr, d_M_out_ptr,
                          stream_ptr=None, strides=None):
        """r1_accumulate_device: the same on device memory (L, A_prev, A_out 4-byte aligned, the feature and moment images 16-byte aligned;
        A_out may be L, M_out may be V); `strides`: eight pixel pitches in the order of the pointers (0 = width); enqueued on stream_ptr,
        waits for nothing."""
        fr = AccumulateFrame(int(width), int(height), *[int(v) for v in (strides or (0,) * 8)])
        im = AccumulateImages(*[p or None for p in (d_L_ptr, d_V_ptr, d_f_ptr, d_A_prev_ptr, d_f_prev_ptr, d_M_prev_ptr, d_A_out_ptr, d_M_out_ptr)])
        _check(lib().r1_accumulate_device(self._c, C.byref(fr), C.byref(opt), C.byref(view), C.byref(im), _stream_arg(stream_ptr)))

    def render_accumulated(self, params, acc_opt, guided_opt=None):
        """r1_render_accumulated: the frame rendered with its variance and feature frames, accumulated against the context's history and,
        with guided_opt, filtered.  Returns (float32 (height, width, 3), ray count, device seconds of everything)."""
        img = np.zeros((max(params.height, 1), max(params.width, 1), 3), np.float32)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_render_accumulated(self._c, C.byref(params), C.byref(acc_opt), C.byref(guided_opt) if guided_opt is not None else None,
                                           C.c_void_p(img.ctypes.data), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), secs.value

    def render_accumulated_device(self, params, acc_opt, guided_opt, d_rgb_f32_ptr, d_rays_ptr, stream_ptr=None):
        """r1_render_accumulated_device: the same into device memory (width * height * 3 floats, and one uint64); waits for nothing."""
        _check(lib().r1_render_accumulated_device(self._c, C.byref(params), C.byref(acc_opt), C.byref(guided_opt) if guided_opt is not None else None,
                                                  C.c_void_p(d_rgb_f32_ptr or None), C.c_void_p(d_rays_ptr or None), _stream_arg(stream_ptr)))

    def accumulate_reset(self):
        """r1_accumulate_reset: the context's history is forgotten; the next accumulated frame passes through."""
        _check(lib().r1_accumulate_reset(self._c))

    def render_linear_async(self, params, frame_ptr, rays_ptr, stream_ptr=None):
        """r1_render_linear_async: enqueue one linear frame (throughput kernels); width * height * 3 floats land at `frame_ptr` and the
        uint64 ray count at `rays_ptr` (host addresses: a LinearHostFrame's, or pageable memory) once the stream is idle.  Both None:
        the frame stays on the device."""
        _check(lib().r1_render_linear_async(self._c, C.byref(params), C.cast(frame_ptr, _f32p) if frame_ptr else None,
                                            C.cast(rays_ptr, _u64p) if rays_ptr else None, _stream_arg(stream_ptr)))

    def render_linear_device(self, params, d_rgb_f32_ptr, d_rays_ptr, stream_ptr=None):
        """r1_render_linear_device: the linear frame into device memory (width * height * 3 floats, and one uint64); waits for nothing."""
        _check(lib().r1_render_linear_device(self._c, C.byref(params), C.c_void_p(d_rgb_f32_ptr), C.c_void_p(d_rays_ptr), _stream_arg(stream_ptr)))

    def pass_linear(self, params):
        """r1_pass_linear: the progressive accumulation as a linear frame.  `params`: those of the accumulation's passes (the C call
        keeps them; here they size the array).  Returns (float32 (height, width, 3), samples accumulated)."""
        img = np.zeros((params.height, params.width, 3), np.float32)
        n = C.c_int32()
        _check(lib().r1_pass_linear(self._c, img.ctypes.data_as(_f32p), C.byref(n)))
        return img, int(n.value)

    def render_adaptive_linear(self, params, min_spp, pass_spp, max_delta, mean_delta_q8):
        """r1_render_adaptive_linear: render_adaptive with a float32 (height, width, 3) linear frame for the byte image."""
        img = np.zeros((params.height, params.width, 3), np.float32)
        opt = Adaptive(min_spp, pass_spp, max_delta, mean_delta_q8)
        total = C.c_int32()
        _check(lib().r1_tile_count(C.byref(params), C.byref(total), None))
        tiles = np.zeros(total.value, TILE_REPORT_DTYPE)
        rays, res = C.c_uint64(), AdaptiveResult()
        _check(lib().r1_render_adaptive_linear(self._c, C.byref(params), C.byref(opt), img.ctypes.data_as(_f32p), C.byref(rays),
                                               tiles.ctypes.data_as(C.POINTER(TileReport)), C.byref(res)))
        return img, int(rays.value), tiles, {"samples": int(res.samples), "passes": int(res.passes), "tiles": int(res.tiles),
                                            "tiles_settled": int(res.tiles_settled)}

    def render_async(self, params, host_frame, stream_ptr=None):
        """r1_render_async: enqueue one frame (throughput kernels) whose pixels + ray count land in `host_frame`
        (a HostFrame) once the stream is idle."""
        _check(lib().r1_render_async(self._c, C.byref(params), C.cast(host_frame.ptr, _u8p),
                                     C.cast(host_frame.ptr + host_frame.rays_offset, _u64p), _stream_arg(stream_ptr)))

    def render_batch_async(self, params, n_frames, host_frames, seed_stride=0, stream_ptr=None):
        """r1_render_batch_async: n_frames frames in one launch; their records land in `host_frames` (a HostFrames, or None
        to leave them on the device) once the stream is idle."""
        _check(lib().r1_render_batch_async(self._c, C.byref(params), n_frames, seed_stride, C.c_void_p(host_frames.ptr) if host_frames else None,
                                           _stream_arg(stream_ptr)))

    def render_path_async(self, params, cameras, host_frames, seed_stride=0, stream_ptr=None):
        """r1_render_path_async: one frame per camera of `cameras` (a sequence of CCamera) in one launch; the records land in
        `host_frames` (a HostFrames, or None to leave them on the device) once the stream is idle."""
        arr = (CCamera * len(cameras))(*cameras)
        _check(lib().r1_render_path_async(self._c, C.byref(params), len(cameras), seed_stride, arr, C.c_void_p(host_frames.ptr) if host_frames else None,
                                          _stream_arg(stream_ptr)))

    def render_shard_device_batch(self, params, n_frames, d_records_ptr, seed_stride=0, stream_ptr=None):
        _check(lib().r1_render_shard_device_batch(self._c, C.byref(params), n_frames, seed_stride, C.c_void_p(d_records_ptr),
                                                  _stream_arg(stream_ptr)))

    def assemble_device_records_batch(self, params, n_frames, d_gathered_ptr, d_frames_ptr, stream_ptr=None):
        _check(lib().r1_assemble_device_records_batch(self._c, C.byref(params), n_frames, C.c_void_p(d_gathered_ptr), C.c_void_p(d_frames_ptr),
                                                      _stream_arg(stream_ptr)))

    def render_frame_device(self, params, stream_ptr=None):
        """r1_render_async without host buffers: the frame stays in the context's device buffers (what the copies cost)."""
        _check(lib().r1_render_async(self._c, C.byref(params), None, None, _stream_arg(stream_ptr)))

    def render_shard_device(self, params, d_block_ptr, d_rays_ptr, stream_ptr=None):
        _check(lib().r1_render_shard_device(self._c, C.byref(params), C.c_void_p(d_block_ptr), C.c_void_p(d_rays_ptr),
                                            _stream_arg(stream_ptr)))

    def assemble_device(self, params, d_blocks_ptr, d_rgb_ptr, stream_ptr=None):
        _check(lib().r1_assemble_device(self._c, C.byref(params), C.c_void_p(d_blocks_ptr), C.c_void_p(d_rgb_ptr),
                                        _stream_arg(stream_ptr)))

    def assemble_device_strided(self, params, d_blocks_ptr, shard_stride_bytes, d_rgb_ptr, stream_ptr=None):
        _check(lib().r1_assemble_device_strided(self._c, C.byref(params), C.c_void_p(d_blocks_ptr), shard_stride_bytes,
                                                C.c_void_p(d_rgb_ptr), _stream_arg(stream_ptr)))

    def assemble_device_records(self, params, d_records_ptr, d_rgb_ptr, d_total_rays_ptr, stream_ptr=None):
        _check(lib().r1_assemble_device_records(self._c, C.byref(params), C.c_void_p(d_records_ptr), C.c_void_p(d_rgb_ptr),
                                                C.c_void_p(d_total_rays_ptr), _stream_arg(stream_ptr)))

    def cast_rays(self, rays, mode=CAST_CLOSEST, variant=0):
        """r1_cast_rays: Hitable::hit for caller-supplied rays, host memory in and out.  `rays`: float32 (n, 8) rows {ox oy oz t_max dx
        dy dz -} or a RAY_DTYPE array.  Returns a HIT_DTYPE array (CAST_CLOSEST) or a uint8 array (CAST_ANY), in ray order."""
        rays = _as_rays(rays)
        out = _cast_out(rays.shape[0], mode)
        _check(lib().r1_cast_rays(self._c, variant, mode, rays.ctypes.data, rays.shape[0], out.ctypes.data))
        return out

    def cast_rays_device(self, d_rays_ptr, n, d_out_ptr, mode=CAST_CLOSEST, variant=0, stream=None):
        """r1_cast_rays_device: the same over device memory (16-byte aligned: n r1_ray in, n r1_hit or n bytes out); enqueues on
        `stream` and waits for nothing."""
        _check(lib().r1_cast_rays_device(self._c, variant, mode, C.c_void_p(d_rays_ptr), n, C.c_void_p(d_out_ptr), _stream_arg(stream)))

    def trace_rays(self, rays, seeds=None, max_bounces=50, variant=0):
        """r1_trace_rays: color() for caller-supplied rays, host memory in and out.  `rays` as for cast_rays (t_max is ignored); `seeds`: a
        SEED_DTYPE array or uint32 (n, 4) rows {scalar, lane0, lane1, lane2}, or None (ray i: the seeding contract's states for seed 0,
        pixel i, sample 0).  Returns a RADIANCE_DTYPE array in ray order."""
        rays = _as_rays(rays)
        seeds = _as_seeds(seeds, rays.shape[0])
        out = np.zeros(rays.shape[0], RADIANCE_DTYPE)
        _check(lib().r1_trace_rays(self._c, variant, max_bounces, rays.ctypes.data, seeds.ctypes.data if seeds is not None else None,
                                   rays.shape[0], out.ctypes.data))
        return out

    def trace_rays_device(self, d_rays_ptr, d_seeds_ptr, n, d_out_ptr, max_bounces=50, variant=0, stream=None):
        """r1_trace_rays_device: the same over device memory (16-byte aligned: n r1_ray and n r1_sample_seed — or 0 / None — in, n
        r1_radiance out); enqueues on `stream` (a hipStream_t value; None: the context's stream) and waits for nothing."""
        _check(lib().r1_trace_rays_device(self._c, variant, max_bounces, C.c_void_p(d_rays_ptr), C.c_void_p(d_seeds_ptr) if d_seeds_ptr else None, n,
                                          C.c_void_p(d_out_ptr), _stream_arg(stream)))

    def scatter_rays(self, rays, seeds=None, flags=0, variant=0):
        """r1_scatter_rays: one color() level — hit test, then Material::scatter — for caller-supplied rays, host memory in and out.  `rays`
        and `seeds` as for trace_rays; flags: 0 or SCATTER_UNIT_DIRECTIONS (the directions are a previous step's: not normalised again).
        Returns (Scatter records as a SCATTER_DTYPE array, the scattered rays as a RAY_DTYPE array, the advanced states as a SEED_DTYPE
        array), in ray order."""
        rays = _as_rays(rays)
        seeds = _as_seeds(seeds, rays.shape[0])
        out, rays_out, seeds_out = _scatter_out(rays.shape[0])
        _check(lib().r1_scatter_rays(self._c, variant, flags, rays.ctypes.data, seeds.ctypes.data if seeds is not None else None, rays.shape[0],
                                     rays_out.ctypes.data, seeds_out.ctypes.data, out.ctypes.data))
        return Scatter(out, rays_out, seeds_out)

    def scatter_rays_device(self, d_rays_ptr, d_seeds_ptr, n, d_rays_out_ptr, d_seeds_out_ptr, d_out_ptr, flags=0, variant=0, stream=None):
        """r1_scatter_rays_device: the same over device memory (16-byte aligned: n r1_ray and n r1_sample_seed — or 0 / None — in; n r1_ray,
        n r1_sample_seed and n r1_scatter out; d_rays_out_ptr == d_rays_ptr and d_seeds_out_ptr == d_seeds_ptr work in place); enqueues on
        `stream` and waits for nothing."""
        _check(lib().r1_scatter_rays_device(self._c, variant, flags, C.c_void_p(d_rays_ptr), C.c_void_p(d_seeds_ptr) if d_seeds_ptr else None, n,
                                            C.c_void_p(d_rays_out_ptr), C.c_void_p(d_seeds_out_ptr), C.c_void_p(d_out_ptr), _stream_arg(stream)))

    def camera_rays_device(self, params, first, n, d_rays_ptr, d_seeds_ptr, camera=None, stream=None):
        """r1_camera_rays_device: the rays and stream states of samples [first, first + n) of the frame, in render_samples' order, written
        to device memory as camera_rays writes them on the host; camera None: the context's.  Enqueues and waits for nothing."""
        _check(lib().r1_camera_rays_device(self._c, C.byref(camera) if camera is not None else None, C.byref(params), first, n,
                                           C.c_void_p(d_rays_ptr), C.c_void_p(d_seeds_ptr), _stream_arg(stream)))

    def set_pixel_mode(self, on):
        _check(lib().r1_set_pixel_mode(self._c, 1 if on else 0))

    def sync(self):
        _check(lib().r1_sync(self._c))

    def last_timing(self):
        a, b = C.c_double(), C.c_double()
        _check(lib().r1_last_timing(self._c, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def timing_begin(self, max_frames):
        _check(lib().r1_timing_begin(self._c, max_frames))

    def timing_end(self):
        a, b, n = C.c_double(), C.c_double(), C.c_int32()
        _check(lib().r1_timing_end(self._c, C.byref(a), C.byref(b), C.byref(n)))
        return float(a.value), float(b.value), int(n.value)

    def last_stats(self):
        out = (C.c_uint64 * 16)()
        _check(lib().r1_last_stats(self._c, out))
        names = ["wave_iterations", "alive_lanes", "candidate_loop_trips", "overflow_lanes", "cycles_refill", "cycles_pass1",
                 "cycles_candidates", "cycles_shade", "cycles_wave", "candidates"]
        d = {n: int(out[i]) for i, n in enumerate(names)}
        m = (1 << 64) - 1
        d["longest_wave_cycles"] = int(out[10])
        d["shortest_wave_cycles"] = m - int(out[11])
        d["span_cycles"] = int(out[12]) - (m - int(out[13]))
        d["leaf_lane_trips"] = int(out[14])  # tree diagnostic build: leaf trips summed over lanes
        d["root_steps"] = int(out[15])       # tree diagnostic build: root steps (one box test + the root's leaf, outside the walk's loops)
        d["raw"] = [int(x) for x in out]     # (the grid's diagnostic build: include/rays1.h R1_VARIANT_GRID_STATS names its slots)
        return d

    def wave_log(self):
        n = C.c_uint32()
        _check(lib().r1_last_wave_log(self._c, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.uint64)
        if n.value:
            _check(lib().r1_last_wave_log(self._c, out.ctypes.data_as(_u64p), n.value, C.byref(n)))
        return out

    def launch_info(self):
        li = LaunchInfo()
        _check(lib().r1_last_launch_info(self._c, C.byref(li)))
        return {k: int(getattr(li, k)) for k, _ in LaunchInfo._fields_}

    def walk_form(self):
        """r1_last_walk_form: 1 where the last trace launch ran a flat twin of the tree kernel, else 0"""
        form = lib().r1_last_walk_form(self._c)
        if form < 0:
            _check(form)
        return int(form)

    def close(self):
        if self._c:
            lib().r1_destroy(self._c)
            self._c = _ctx()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostFrame:
    """Page-locked host memory (r1_host_alloc) for one frame's results: height x width x 3 pixels followed by an
    8-byte-aligned uint64 ray count — the target of Renderer.render_async."""

    def __init__(self, width, height):
        self.nbytes = width * height * 3
        self.rays_offset = (self.nbytes + 7) & ~7
        p = C.c_void_p()
        _check(lib().r1_host_alloc(self.rays_offset + 8, C.byref(p)))
        self.ptr = p.value
        buf = (C.c_uint8 * (self.rays_offset + 8)).from_address(self.ptr)
        self._all = np.frombuffer(buf, np.uint8)
        self._all[:] = 0
        self.image = self._all[:self.nbytes].reshape(height, width, 3)
        self._rays = self._all[self.rays_offset:].view(np.uint64)

    @property
    def rays(self):
        return int(self._rays[0])

    def close(self):
        if self.ptr:
            self.image = self._rays = self._all = None
            lib().r1_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostFrames:
    """Page-locked host memory for the n frame records of a batch (include/rays1.h r1_frame_record_bytes: image, padded
    to 8 bytes, + uint64 ray count) — the target of Renderer.render_batch_async and of bench.py's copies."""

    def __init__(self, width, height, n):
        self.n, self.nbytes = n, width * height * 3
        self.record = ((self.nbytes + 7) & ~7) + 8
        p = C.c_void_p()
        _check(lib().r1_host_alloc(self.record * n, C.byref(p)))
        self.ptr = p.value
        buf = (C.c_uint8 * (self.record * n)).from_address(self.ptr)
        self._all = np.frombuffer(buf, np.uint8)
        self._all[:] = 0
        self._shape = (height, width, 3)
        self.rays_offset = self.record - 8  # (a one-frame HostFrames is also a valid target of Renderer.render_async)

    def image(self, i):
        return self._all[i * self.record:i * self.record + self.nbytes].reshape(self._shape)

    def rays(self, i):
        return int(self._all[(i + 1) * self.record - 8:(i + 1) * self.record].view(np.uint64)[0])

    def close(self):
        if self.ptr:
            self._all = None
            lib().r1_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiRenderer:
    """r1_multi: one process, N GPUs, tile split + one RCCL all-gather per frame (include/rays1.h)."""

    def __init__(self, devices):
        devs = (C.c_int32 * len(devices))(*devices)
        self._m = C.c_void_p()
        _check(lib().r1_multi_create(len(devices), devs, C.byref(self._m)))

    def set_scene(self, scene):
        _check(lib().r1_multi_set_scene(self._m, scene.spheres, scene.camera))

    def set_camera(self, ccamera):
        _check(lib().r1_multi_set_camera(self._m, C.byref(ccamera)))

    def render(self, params):
        img = np.zeros((params.height, params.width, 3), np.uint8)
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_multi_render(self._m, C.byref(params), img.ctypes.data_as(_u8p), C.byref(rays), C.byref(secs)))
        return img, int(rays.value), float(secs.value)

    def render_into(self, params, img):
        rays, secs = C.c_uint64(), C.c_double()
        _check(lib().r1_multi_render(self._m, C.byref(params), img.ctypes.data_as(_u8p), C.byref(rays), C.byref(secs)))
        return int(rays.value), float(secs.value)

    def render_async(self, params, host_frames):
        """r1_multi_render_async: enqueue one frame over the N GPUs; its record lands in `host_frames` (a HostFrames of 1)."""
        _check(lib().r1_multi_render_async(self._m, C.byref(params), C.c_void_p(host_frames.ptr)))

    def render_batch_async(self, params, n_frames, host_frames, seed_stride=0):
        _check(lib().r1_multi_render_batch_async(self._m, C.byref(params), n_frames, seed_stride, C.c_void_p(host_frames.ptr)))

    def sync(self):
        _check(lib().r1_multi_sync(self._m))

    def info(self):
        n, v, li = C.c_int32(), C.c_int32(), LaunchInfo()
        _check(lib().r1_multi_info(self._m, C.byref(n), C.byref(v), C.byref(li)))
        return {"devices": int(n.value), "rccl_version": int(v.value), "first_device": {k: int(getattr(li, k)) for k, _ in LaunchInfo._fields_}}

    def close(self):
        if self._m:
            lib().r1_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_block_bytes(params):
    return int(lib().r1_shard_block_bytes(C.byref(params)))


def frame_record_bytes(params):
    return int(lib().r1_frame_record_bytes(C.byref(params)))


def shard_record_bytes(params):
    return int(lib().r1_shard_record_bytes(C.byref(params)))


def tile_count(params):
    a, b = C.c_int32(), C.c_int32()
    _check(lib().r1_tile_count(C.byref(params), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def multi_layout(params, n_devices, n_frames=1):
    """r1_multi_layout: the buffer layout of an n_devices-device frame / batch (pure arithmetic, no device needed)."""
    out = MultiLayout()
    _check(lib().r1_multi_layout(C.byref(params), n_devices, n_frames, C.byref(out)))
    return {k: int(getattr(out, k)) for k, _ in MultiLayout._fields_}


def bvh_describe(cscene, leaf_max=0):
    """Host-side build of the R1_VARIANT_BVH index: (info dict, nodes float32[n,16], ids uint32[2*pairs], 0xFFFFFFFF = empty slot)."""
    info = BvhInfo()
    _check(lib().r1_bvh_describe(C.byref(cscene), leaf_max, C.byref(info), None, 0, None, 0))
    nodes = np.zeros((info.nodes, 16), np.float32)
    ids = np.zeros(max(2 * info.pairs, 2), np.uint32)
    _check(lib().r1_bvh_describe(C.byref(cscene), leaf_max, C.byref(info), nodes.ctypes.data_as(_f32p), nodes.size,
                                 ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size))
    d = {k: int(getattr(info, k)) for k, _ in BvhInfo._fields_ if k not in ("centre", "flat_m", "flat_e")}
    d["flat_m"], d["flat_e"] = np.float32(info.flat_m), np.float32(info.flat_e)
    d["centre"] = np.array(list(info.centre), np.float32)
    return d, nodes, ids[:2 * info.pairs]


def bvh_refit_describe(cscene, x, y, z, leaf_max=0):
    """r1_bvh_refit_describe: the tree r1_set_scene builds for `cscene`, refitted on the host to the scene-indexed centres x, y, z (cscene.count
    entries each): (info dict, nodes float32[n, 16]).  The ids are bvh_describe(cscene)'s."""
    return _refit_describe("bvh_refit_describe", cscene, x, y, z, None, None, leaf_max)


def bvh_refit_describe_spheres(cscene, x, y, z, radius_sq=None, inv_radius=None, leaf_max=0):
    """r1_bvh_refit_describe_spheres: bvh_refit_describe with scene-indexed radii as well (both None: the built scene's)."""
    if (radius_sq is None) != (inv_radius is None):
        raise R1Error(R1_EINVAL, "bvh_refit_describe_spheres: radius_sq and inv_radius go together")
    return _refit_describe("bvh_refit_describe_spheres", cscene, x, y, z, radius_sq, inv_radius, leaf_max)


def bvh_resort_describe(cscene, x, y, z, radius_sq=None, inv_radius=None, leaf_max=0):
    """r1_bvh_resort_describe: the tree r1_set_scene builds for `cscene`, its movable spheres re-dealt on the host for the scene-indexed centres
    (and radii; both None: the built scene's), then refitted: (info dict, nodes float32[n, 16], ids uint32[2 * pairs], 0xFFFFFFFF = empty)."""
    if (radius_sq is None) != (inv_radius is None):
        raise R1Error(R1_EINVAL, "bvh_resort_describe: radius_sq and inv_radius go together")
    arrays = [np.ascontiguousarray(v, np.float32) for v in (x, y, z) + (() if radius_sq is None else (radius_sq, inv_radius))]
    if any(v.shape != (cscene.count,) for v in arrays):
        raise R1Error(R1_EINVAL, "bvh_resort_describe: every array needs cscene.count entries")
    ptrs = [v.ctypes.data_as(_f32p) for v in arrays] + ([None, None] if radius_sq is None else [])
    info = BvhInfo()
    _check(lib().r1_bvh_resort_describe(C.byref(cscene), *ptrs, leaf_max, C.byref(info), None, 0, None, 0))
    nodes = np.zeros((info.nodes, 16), np.float32)
    ids = np.zeros(max(2 * info.pairs, 2), np.uint32)
    _check(lib().r1_bvh_resort_describe(C.byref(cscene), *ptrs, leaf_max, C.byref(info), nodes.ctypes.data_as(_f32p), nodes.size,
                                        ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size))
    d = {k: int(getattr(info, k)) for k, _ in BvhInfo._fields_ if k not in ("centre", "flat_m", "flat_e")}
    d["flat_m"], d["flat_e"] = np.float32(info.flat_m), np.float32(info.flat_e)
    d["centre"] = np.array(list(info.centre), np.float32)
    return d, nodes, ids[:2 * info.pairs]


def _refit_describe(who, cscene, x, y, z, radius_sq, inv_radius, leaf_max):
    """The two host refits, r1_<who>: the same arguments but for the radii in front of leaf_max."""
    arrays = [np.ascontiguousarray(v, np.float32) for v in (x, y, z) + (() if radius_sq is None else (radius_sq, inv_radius))]
    if any(v.shape != (cscene.count,) for v in arrays):
        raise R1Error(R1_EINVAL, f"{who}: every array needs cscene.count entries")
    ptrs = [v.ctypes.data_as(_f32p) for v in arrays]
    fn = getattr(lib(), "r1_" + who)
    if who == "bvh_refit_describe_spheres" and radius_sq is None:
        ptrs += [None, None]
    info = BvhInfo()
    _check(fn(C.byref(cscene), *ptrs, leaf_max, C.byref(info), None, 0))
    nodes = np.zeros((info.nodes, 16), np.float32)
    _check(fn(C.byref(cscene), *ptrs, leaf_max, C.byref(info), nodes.ctypes.data_as(_f32p), nodes.size))
    d = {k: int(getattr(info, k)) for k, _ in BvhInfo._fields_ if k not in ("centre", "flat_m", "flat_e")}
    d["flat_m"], d["flat_e"] = np.float32(info.flat_m), np.float32(info.flat_e)
    d["centre"] = np.array(list(info.centre), np.float32)
    return d, nodes


def _grid_tables(call):
    """The two-call protocol of r1_grid_describe and its kin: `call(info, start, start_cap, ids, ids_cap, outliers, outliers_cap)`."""
    info = GridInfo()
    _check(call(C.byref(info), None, 0, None, 0, None, 0))
    ncells = int(info.cells[0]) * int(info.cells[1]) * int(info.cells[2])
    regs = max(info.registrations, 0)
    start = np.zeros(ncells + 1, np.uint32)
    ids = np.zeros(max(regs, 1), np.uint32)
    outl = np.zeros(max(info.outliers, 1), np.uint32)
    u32p = C.POINTER(C.c_uint32)
    _check(call(C.byref(info), start.ctypes.data_as(u32p), start.size, ids.ctypes.data_as(u32p), ids.size, outl.ctypes.data_as(u32p), outl.size))
    d = {}
    for k, t in GridInfo._fields_:
        v = getattr(info, k)
        d[k] = np.array(list(v), np.float32 if k != "cells" else np.int64) if hasattr(v, "__len__") else v
    return d, start, ids[:regs], outl[:info.outliers]


def grid_describe(cscene):
    """Host-side build of the R1_VARIANT_GRID index: (info dict, start uint32[cells + 1], ids uint32[registrations], outliers uint32[n]);
    ids and outliers are scene indices."""
    return _grid_tables(lambda *a: lib().r1_grid_describe(C.byref(cscene), *a))


def _regrid_arrays(who, cscene, x, y, z, radius_sq, inv_radius):
    if (radius_sq is None) != (inv_radius is None):
        raise R1Error(R1_EINVAL, f"{who}: radius_sq and inv_radius go together")
    arrays = [np.ascontiguousarray(v, np.float32) for v in (x, y, z) + (() if radius_sq is None else (radius_sq, inv_radius))]
    if any(v.shape != (cscene.count,) for v in arrays):
        raise R1Error(R1_EINVAL, f"{who}: every array needs cscene.count entries")
    return arrays, [v.ctypes.data_as(_f32p) for v in arrays] + ([None, None] if radius_sq is None else [])


def grid_plan(cscene):
    """What a regrid keeps of the grid of `cscene` besides grid_describe's geometry (r1_grid_plan_describe, internal as r1_sweep_describe
    is): {"V", "delta", "big", "M": float, "flat": bool[3]}."""
    f = lib().r1_grid_plan_describe
    f.restype, f.argtypes = C.c_int, [C.POINTER(CScene), _dblp, _i32p]
    d4, flat = np.zeros(4, np.float64), np.zeros(3, np.int32)
    _check(f(C.byref(cscene), d4.ctypes.data_as(_dblp), flat.ctypes.data_as(_i32p)))
    return {"V": float(d4[0]), "delta": float(d4[1]), "big": float(d4[2]), "M": float(d4[3]), "flat": flat != 0}


def regrid_describe(cscene, x, y, z, radius_sq=None, inv_radius=None):
    """r1_grid_regrid_describe: the grid r1_set_scene's arrays give `cscene`, its plan kept and the scene-indexed centres (and radii; both
    None: the built scene's) re-registered on the host by the device's steps: as grid_describe returns it; overflow: registrations == -1."""
    keep, ptrs = _regrid_arrays("regrid_describe", cscene, x, y, z, radius_sq, inv_radius)
    return _grid_tables(lambda *a: lib().r1_grid_regrid_describe(C.byref(cscene), *ptrs, *a))


def regrid_visit(cscene, x, y, z, o, d, radius_sq=None, inv_radius=None, cap=1 << 16):
    """grid_visit through the regridded tables, against the moved spheres."""
    keep, ptrs = _regrid_arrays("regrid_visit", cscene, x, y, z, radius_sq, inv_radius)
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    pres = np.zeros(cap, np.uint32)
    n, hi, ht, fb = C.c_size_t(), C.c_int32(), C.c_float(), C.c_int32()
    _check(lib().r1_grid_regrid_visit(C.byref(cscene), *ptrs, o.ctypes.data_as(_f32p), d.ctypes.data_as(_f32p), pres.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      cap, C.byref(n), C.byref(hi), C.byref(ht), C.byref(fb)))
    if n.value > cap:
        return regrid_visit(cscene, x, y, z, o, d, radius_sq, inv_radius, int(n.value))
    return pres[:n.value], int(hi.value), float(ht.value), bool(fb.value)


class SweepInfo(C.Structure):
    _fields_ = [("spheres", C.c_int32), ("groups", C.c_int32), ("multi", C.c_int32), ("n_sweep", C.c_int32), ("slots", C.c_int32),
                ("group_max", C.c_int32)]


def sweep_describe(cscene):
    """Host-side build of the sweep's tables (R1_VARIANT_PREFILTER) as r1_set_scene builds them; r1_sweep_describe is internal
    (csrc/r1_internal.h, not include/rays1.h), so its prototype is set here.  Returns a dict: the SweepInfo fields; `groups`
    float64[n, 8] = per group {centre x, y, z as stored in fp32, stored Kp, covering radius R around that centre, the radius the
    R1_GROUP_RATIO rule saw, c_max2, n}; the raw tables `sweep` float32[slots / 2, 8] (pair layout), `members` uint32[slots, group_max]
    (active indices, 0xFFFFFFFF = none), `exact_g` float32[slots, group_max, 4]; `active` uint32[spheres]: active -> scene index."""
    f = lib().r1_sweep_describe
    u32p, f64p, sz = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_size_t
    f.restype, f.argtypes = C.c_int, [C.POINTER(CScene), C.POINTER(SweepInfo), f64p, sz, _f32p, sz, u32p, sz, _f32p, sz, u32p, sz]
    info = SweepInfo()
    _check(f(C.byref(cscene), C.byref(info), None, 0, None, 0, None, 0, None, 0, None, 0))
    groups = np.zeros((max(info.groups, 1), 8), np.float64)
    sweep = np.zeros((info.slots // 2, 8), np.float32)
    members = np.zeros((info.slots, info.group_max), np.uint32)
    exact_g = np.zeros((info.slots, info.group_max, 4), np.float32)
    active = np.zeros(max(info.spheres, 1), np.uint32)
    _check(f(C.byref(cscene), C.byref(info), groups.ctypes.data_as(f64p), groups.size, sweep.ctypes.data_as(_f32p), sweep.size,
             members.ctypes.data_as(u32p), members.size, exact_g.ctypes.data_as(_f32p), exact_g.size, active.ctypes.data_as(u32p), active.size))
    d = {k: int(getattr(info, k)) for k, _ in SweepInfo._fields_}
    d.update(group_rows=groups[:info.groups], sweep=sweep, members=members, exact_g=exact_g, active=active[:info.spheres])
    return d


def grid_visit(cscene, o, d, cap=1 << 16):
    """One ray through the grid on the host, in the kernel's arithmetic: (presented scene indices in order, hit index or -1, hit t,
    fallback flag)."""
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    pres = np.zeros(cap, np.uint32)
    n, hi, ht, fb = C.c_size_t(), C.c_int32(), C.c_float(), C.c_int32()
    _check(lib().r1_grid_visit(C.byref(cscene), o.ctypes.data_as(_f32p), d.ctypes.data_as(_f32p), pres.ctypes.data_as(C.POINTER(C.c_uint32)), cap,
                               C.byref(n), C.byref(hi), C.byref(ht), C.byref(fb)))
    if n.value > cap:
        return grid_visit(cscene, o, d, int(n.value))
    return pres[:n.value], int(hi.value), float(ht.value), bool(fb.value)


def _as_rays(rays):
    rays = np.asarray(rays)
    if rays.dtype == RAY_DTYPE and rays.ndim == 1:
        return np.ascontiguousarray(rays)
    if rays.dtype == np.float32 and rays.ndim == 2 and rays.shape[1] == 8:
        return np.ascontiguousarray(rays)
    raise R1Error(R1_EINVAL, "rays: a float32 (n, 8) array or a RAY_DTYPE array")


def _cast_out(n, mode):
    # (a mode the library refuses still gets a buffer that is large enough for either form: the call reports the error)
    return np.zeros(n, np.uint8) if mode == CAST_ANY else np.zeros(n, HIT_DTYPE)


def cast_rays_host(cscene, rays, mode=CAST_CLOSEST):
    """r1_cast_rays_host: every ray against every sphere in the reference's arithmetic, on host threads (no device).  Same input and
    output forms as Renderer.cast_rays."""
    rays = _as_rays(rays)
    out = _cast_out(rays.shape[0], mode)
    _check(lib().r1_cast_rays_host(C.byref(cscene), mode, rays.ctypes.data, rays.shape[0], out.ctypes.data))
    return out


def _as_seeds(seeds, n):
    if seeds is None:
        return None
    seeds = np.asarray(seeds)
    if (seeds.dtype == SEED_DTYPE and seeds.shape == (n,)) or (seeds.dtype == np.uint32 and seeds.shape == (n, 4)):
        return np.ascontiguousarray(seeds)
    raise R1Error(R1_EINVAL, "seeds: a SEED_DTYPE array or a uint32 (n, 4) array, one per ray")


def trace_rays_host(cscene, rays, seeds=None, max_bounces=50):
    """r1_trace_rays_host: color() for caller-supplied rays in scalar C++ on host threads (no device).  Same input and output forms as
    Renderer.trace_rays."""
    rays = _as_rays(rays)
    seeds = _as_seeds(seeds, rays.shape[0])
    out = np.zeros(rays.shape[0], RADIANCE_DTYPE)
    _check(lib().r1_trace_rays_host(C.byref(cscene), max_bounces, rays.ctypes.data, seeds.ctypes.data if seeds is not None else None,
                                    rays.shape[0], out.ctypes.data))
    return out


class Scatter(tuple):
    """What one step returns: (records, rays, seeds) — the SCATTER_DTYPE records, the scattered rays (RAY_DTYPE, unit directions: feed them
    to the next step with SCATTER_UNIT_DIRECTIONS) and the advanced stream states (SEED_DTYPE).  Unpacks as a 3-tuple."""

    def __new__(cls, records, rays, seeds):
        return super().__new__(cls, (records, rays, seeds))

    records = property(lambda self: self[0])
    rays = property(lambda self: self[1])
    seeds = property(lambda self: self[2])


def _scatter_out(n):
    return np.zeros(n, SCATTER_DTYPE), np.zeros(n, RAY_DTYPE), np.zeros(n, SEED_DTYPE)


def scatter_rays_host(cscene, rays, seeds=None, flags=0):
    """r1_scatter_rays_host: one color() level in scalar C++ on host threads (no device) — the level r1_trace_rays_host folds.  Same input
    and output forms as Renderer.scatter_rays."""
    rays = _as_rays(rays)
    seeds = _as_seeds(seeds, rays.shape[0])
    out, rays_out, seeds_out = _scatter_out(rays.shape[0])
    _check(lib().r1_scatter_rays_host(C.byref(cscene), flags, rays.ctypes.data, seeds.ctypes.data if seeds is not None else None, rays.shape[0],
                                      rays_out.ctypes.data, seeds_out.ctypes.data, out.ctypes.data))
    return Scatter(out, rays_out, seeds_out)


def camera_rays(ccamera, params, x, y, s):
    """r1_camera_rays: the rays (un-normalised directions, t_max = FLT_MAX) and the stream states after the camera's draws of samples
    s[i] of pixels (x[i], y[i]).  Returns (RAY_DTYPE array, SEED_DTYPE array); traced, they are those samples' records of render_samples."""
    x, y, s = (np.ascontiguousarray(v, np.int32) for v in (x, y, s))
    if not (x.ndim == 1 and x.shape == y.shape == s.shape):
        raise R1Error(R1_EINVAL, "camera_rays: x, y and s are 1-D arrays of one length")
    rays, seeds = np.zeros(x.shape[0], RAY_DTYPE), np.zeros(x.shape[0], SEED_DTYPE)
    _check(lib().r1_camera_rays(C.byref(ccamera), C.byref(params), x.ctypes.data_as(_i32p), y.ctypes.data_as(_i32p), s.ctypes.data_as(_i32p),
                                x.shape[0], rays.ctypes.data, seeds.ctypes.data))
    return rays, seeds


def render_linear_host(cscene, ccamera, params):
    """r1_render_linear_host: the linear frame on the CPU (camera_rays + trace_rays_host for every sample, summed in sample order; no
    device; slow).  Returns (float32 (height, width, 3), ray count)."""
    img = np.zeros((params.height, params.width, 3), np.float32)
    rays = C.c_uint64()
    _check(lib().r1_render_linear_host(C.byref(cscene), C.byref(ccamera), C.byref(params), img.ctypes.data_as(_f32p), C.byref(rays)))
    return img, int(rays.value)


def render_moments_host(cscene, ccamera, params):
    """r1_render_moments_host: the linear frame and its variance frame on the CPU (no device; slow) — what Renderer.render_moments is checked
    against.  Returns (float32 (height, width, 3), MOMENT_DTYPE array (height, width), ray count)."""
    img = np.zeros((params.height, params.width, 3), np.float32)
    mom = np.zeros((params.height, params.width), MOMENT_DTYPE)
    rays = C.c_uint64()
    _check(lib().r1_render_moments_host(C.byref(cscene), C.byref(ccamera), C.byref(params), img.ctypes.data_as(_f32p), C.c_void_p(mom.ctypes.data), C.byref(rays)))
    return img, mom, int(rays.value)


def _region_target(region, out, dtype):
    """(Region, array) of a host-memory region render: a new dense (height, width, 3) array, or the caller's `out` — an array or a view of that
    shape whose pixels are contiguous and whose rows lie a whole number of pixels apart: that pitch is the region's out_stride."""
    x0, y0, w, h = (int(v) for v in region)
    if out is None:
        if w < 1 or h < 1:  # (no array of that shape: let the library name the field)
            return Region(x0, y0, w, h, 0), np.zeros((1, 1, 3), dtype)
        return Region(x0, y0, w, h, 0), np.zeros((h, w, 3), dtype)
    item = np.dtype(dtype).itemsize
    if not (isinstance(out, np.ndarray) and out.dtype == np.dtype(dtype) and out.shape == (h, w, 3) and out.strides[1:] == (3 * item, item)
            and out.strides[0] % (3 * item) == 0 and out.strides[0] >= 3 * item * w and out.flags.writeable):
        raise R1Error(R1_EINVAL, f"region render: out must be a writeable {np.dtype(dtype).name} array or view of shape ({h}, {w}, 3) with whole pixels between its rows")
    return Region(x0, y0, w, h, out.strides[0] // (3 * item)), out


def region_check(params, region, out_stride=0):
    """r1_region_check: raises R1Error (code R1_EINVAL or R1_ELIMIT, the text names the field) unless `region` = (x0, y0, width, height) with
    out_stride is a window of the frame `params` describes that a region render accepts.  Pure arithmetic."""
    rg = Region(*[int(v) for v in region], int(out_stride))
    _check(lib().r1_region_check(C.byref(params), C.byref(rg)))
    return True


def render_region_host(cscene, ccamera, params, region, out=None):
    """r1_render_region_host: the region's linear values on the CPU (camera_rays + trace_rays_host per sample; no device; slow).  Returns
    (float32 (height, width, 3), ray count); `out` as for Renderer.render_region_linear.  Bytes: quantise_linear of the result."""
    rg, img = _region_target(region, out, np.float32)
    rays = C.c_uint64()
    _check(lib().r1_render_region_host(C.byref(cscene), C.byref(ccamera), C.byref(params), C.byref(rg), C.c_void_p(img.ctypes.data), C.byref(rays)))
    return img, int(rays.value)


def _feature_target(params, region, out):
    """(Region or None, array) of a host-memory feature frame: a new dense (height, width) FEATURE_DTYPE array, or the caller's `out` — an array
    or a view of that shape whose rows lie a whole number of records apart: that pitch is the region's out_stride.  None: the call's NULL
    region, the whole frame."""
    x0, y0, w, h = (int(v) for v in region) if region is not None else (0, 0, params.width, params.height)
    if out is None:
        img = np.zeros((max(h, 1), max(w, 1)), FEATURE_DTYPE)  # (a size no array has: the library names the field)
        return (Region(x0, y0, w, h, 0) if region is not None else None), img
    item = FEATURE_DTYPE.itemsize
    if not (isinstance(out, np.ndarray) and out.dtype == FEATURE_DTYPE and out.shape == (h, w) and out.strides[1] == item
            and out.strides[0] % item == 0 and out.strides[0] >= item * w and out.flags.writeable):
        raise R1Error(R1_EINVAL, f"feature frame: out must be a writeable FEATURE_DTYPE array or view of shape ({h}, {w}) with whole records between its rows")
    return Region(x0, y0, w, h, out.strides[0] // item), out


def render_features_host(cscene, ccamera, params, region=None, out=None):
    """r1_render_features_host: the feature frame on the CPU (camera_rays + cast_rays_host per sample, summed in sample order; no device;
    slow) — what Renderer.render_features is checked against.  Returns a FEATURE_DTYPE array (height, width); `region` and `out` as there."""
    rg, img = _feature_target(params, region, out)
    _check(lib().r1_render_features_host(C.byref(cscene), C.byref(ccamera), C.byref(params), C.byref(rg) if rg is not None else None,
                                         C.c_void_p(img.ctypes.data)))
    return img


def _pixel_pitch(a, what, dtype, tail, item):
    """pixels between two rows of `a`, an array or view of shape (h, w) + tail whose pixels are contiguous and whose rows lie whole pixels apart"""
    ok = isinstance(a, np.ndarray) and a.dtype == dtype and a.ndim == 2 + len(tail) and a.shape[2:] == tail and a.shape[0] > 0 and a.shape[1] > 0
    ok = ok and a.strides[1] == item and (not tail or a.strides[2] == 4) and a.strides[0] % item == 0 and a.strides[0] >= item * a.shape[1]
    if not ok:
        raise R1Error(R1_EINVAL, f"denoise: {what} must be a {np.dtype(dtype).name} array or view (height, width{', 3' if tail else ''}) with whole pixels between its rows")
    return a.strides[0] // item


def _denoise_target(L, f, out):
    """(DenoiseFrame, L, f, out) of a host-memory denoise: the pitches of the three arrays become the frame's strides; out None: a new dense array"""
    ls, fs = _pixel_pitch(L, "L", np.float32, (3,), 12), _pixel_pitch(f, "f", FEATURE_DTYPE, (), FEATURE_DTYPE.itemsize)
    h, w = L.shape[:2]
    if out is None:
        out = np.zeros((h, w, 3), np.float32)
    os_ = _pixel_pitch(out, "out", np.float32, (3,), 12)
    if f.shape != (h, w) or out.shape != (h, w, 3) or not out.flags.writeable:
        raise R1Error(R1_EINVAL, f"denoise: L {L.shape}, f {f.shape} and out {out.shape} are not one frame, or out is read-only")
    return DenoiseFrame(w, h, ls, fs, os_), L, f, out


def denoise_check(frame, opt):
    """r1_denoise_check: raises R1Error (R1_EINVAL naming the field, R1_ELIMIT at width * height >= 2^31) unless the DenoiseFrame and the
    DenoiseOpt are ones a denoise accepts.  Pure arithmetic."""
    _check(lib().r1_denoise_check(C.byref(frame), C.byref(opt)))
    return True


def denoise_host(L, f, opt, out=None):
    """r1_denoise_host: the filter on the CPU, no device: the definition Renderer.denoise is checked against.  Arguments as there; returns out."""
    fr, L, f, out = _denoise_target(L, f, out)
    _check(lib().r1_denoise_host(C.byref(fr), C.byref(opt), C.c_void_p(L.ctypes.data), C.c_void_p(f.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def _denoise_guided_target(L, f, V, out):
    """(DenoiseGuidedFrame, L, f, V, out) of a host-memory guided denoise: _denoise_target's rules, and V's pitch"""
    fr, L, f, out = _denoise_target(L, f, out)
    ms = _pixel_pitch(V, "V", MOMENT_DTYPE, (), MOMENT_DTYPE.itemsize)
    if V.shape != f.shape:
        raise R1Error(R1_EINVAL, f"denoise: V {V.shape} is not the frame of f {f.shape}")
    return DenoiseGuidedFrame(fr.width, fr.height, fr.linear_stride, fr.feature_stride, ms, fr.out_stride), L, f, V, out


def denoise_guided_check(frame, opt):
    """r1_denoise_guided_check: raises R1Error naming the field unless the DenoiseGuidedFrame and the DenoiseGuidedOpt are ones a guided
    denoise accepts.  Pure arithmetic."""
    _check(lib().r1_denoise_guided_check(C.byref(frame), C.byref(opt)))
    return True


def denoise_guided_host(L, f, V, opt, out=None):
    """r1_denoise_guided_host: the variance-guided filter on the CPU, no device: the definition Renderer.denoise_guided is checked against."""
    fr, L, f, V, out = _denoise_guided_target(L, f, V, out)
    _check(lib().r1_denoise_guided_host(C.byref(fr), C.byref(opt), C.c_void_p(L.ctypes.data), C.c_void_p(f.ctypes.data), C.c_void_p(V.ctypes.data),
                                        C.c_void_p(out.ctypes.data)))
    return out


def _accumulate_target(L, V, f, A_prev, f_prev, M_prev, A_out, M_out):
    """(AccumulateFrame, AccumulateImages, A_out, M_out, the arrays kept alive) of a host-memory accumulation: the pitches of the eight arrays
    become the frame's strides; an output that is None: a new dense array"""
    h, w = L.shape[:2]
    if A_out is None:
        A_out = np.zeros((h, w, 3), np.float32)
    if M_out is None:
        M_out = np.zeros((h, w), MOMENT_DTYPE)
    spec = (("L", L, np.float32, (3,), 12), ("V", V, MOMENT_DTYPE, (), 16), ("f", f, FEATURE_DTYPE, (), 32), ("A_prev", A_prev, np.float32, (3,), 12),
            ("f_prev", f_prev, FEATURE_DTYPE, (), 32), ("M_prev", M_prev, MOMENT_DTYPE, (), 16), ("A_out", A_out, np.float32, (3,), 12),
            ("M_out", M_out, MOMENT_DTYPE, (), 16))
    pitches = [_pixel_pitch(a, name, dt, tail, item) for name, a, dt, tail, item in spec]
    if any(a.shape[:2] != (h, w) for _, a, _, _, _ in spec) or not (A_out.flags.writeable and M_out.flags.writeable):
        raise R1Error(R1_EINVAL, "accumulate: the eight arrays are not one frame, or an output is read-only")
    keep = [a for _, a, _, _, _ in spec]
    return AccumulateFrame(w, h, *pitches), AccumulateImages(*[a.ctypes.data for a in keep]), A_out, M_out, keep


def accumulate_check(frame, opt, view):
    """r1_accumulate_check: raises R1Error (R1_EINVAL naming the field, R1_ELIMIT at width * height >= 2^31) unless the AccumulateFrame, the
    AccumulateOpt and the AccumulateView are ones an accumulation accepts; returns the call's ReprojectPlan.  Pure arithmetic."""
    plan = ReprojectPlan()
    _check(lib().r1_accumulate_check(C.byref(frame), C.byref(opt), C.byref(view), C.byref(plan)))
    return plan


def accumulate_host(L, V, f, A_prev, f_prev, M_prev, view, opt, A_out=None, M_out=None):
    """r1_accumulate_host: the accumulation on the CPU, no device: the definition Renderer.accumulate is checked against.  L, A_prev float32
    (height, width, 3); V, M_prev MOMENT_DTYPE and f, f_prev FEATURE_DTYPE (height, width); arrays or views whose rows lie whole pixels
    apart.  A_out / M_out: None (new dense arrays) or such arrays — L and V themselves for in place.  Returns (A_out, M_out)."""
    fr, im, A_out, M_out, keep = _accumulate_target(L, V, f, A_prev, f_prev, M_prev, A_out, M_out)
    _check(lib().r1_accumulate_host(C.byref(fr), C.byref(opt), C.byref(view), C.byref(im)))
    return A_out, M_out


def quantise_linear(linear):
    """r1_quantise_linear: (uint8)(int)(sqrtf(v) * 255.99f) per value of a float32 array, on the host; a uint8 array of its shape."""
    linear = np.ascontiguousarray(linear, np.float32)
    out = np.zeros(linear.shape, np.uint8)
    _check(lib().r1_quantise_linear(linear.ctypes.data_as(_f32p), linear.size, out.ctypes.data_as(_u8p)))
    return out


def pfm_write_rgb32f(filename, width, height, pixels):
    """r1_pfm_write_rgb32f: a float32 (height, width, 3) linear frame as a PFM file (rows from the bottom up, little-endian)."""
    pixels = np.ascontiguousarray(pixels, np.float32)
    if pixels.size != width * height * 3:
        raise R1Error(R1_EINVAL, "pfm_write_rgb32f: pixels must hold width * height * 3 floats")
    _check(lib().r1_pfm_write_rgb32f(filename.encode(), width, height, pixels.ctypes.data_as(_f32p)))
    return True


class LinearHostFrame:
    """Page-locked host memory (r1_host_alloc) for one linear frame: height x width x 3 floats followed by the uint64 ray count — a
    target of Renderer.render_linear_async (frame_ptr = ptr, rays_ptr = ptr + rays_offset) that its launches write themselves."""

    def __init__(self, width, height):
        self.nbytes = width * height * 12
        self.rays_offset = (self.nbytes + 7) & ~7
        p = C.c_void_p()
        _check(lib().r1_host_alloc(self.rays_offset + 8, C.byref(p)))
        self.ptr = p.value
        buf = (C.c_uint8 * (self.rays_offset + 8)).from_address(self.ptr)
        self._all = np.frombuffer(buf, np.uint8)
        self._all[:] = 0
        self.image = self._all[:self.nbytes].view(np.float32).reshape(height, width, 3)
        self._rays = self._all[self.rays_offset:].view(np.uint64)

    @property
    def rays_ptr(self):
        return self.ptr + self.rays_offset

    @property
    def rays(self):
        return int(self._rays[0])

    def close(self):
        if self.ptr:
            self.image = self._rays = self._all = None
            lib().r1_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RESULT:
    """common.h:36-45"""

    def __init__(self, elapsed_seconds=0.0, num_rays=0):
        self.elapsed_seconds = elapsed_seconds
        self.num_rays = num_rays

    def get_mrays_per_sec(self):
        return self.num_rays / self.elapsed_seconds / 1000000.0 if self.elapsed_seconds else 0


def benchmark(scene, pixels, write_tga, scene_name, spp=10, seed=10001, renderer=None, quiet=False):
    """Python twin of RESULT benchmark(Scene*, Pix*, bool, const char*) (rayweek1.cpp:845-927):
    times dispatch -> pixels + ray count on the host (timer span :848 -> :891), prints the
    report block (:895-902), consumes the scene (:905) and optionally writes out_<scene>.tga."""
    own = renderer is None
    r = renderer or Renderer(0)
    r.set_scene(scene)
    p = make_params(scene.width, scene.height, spp, seed)
    t0 = time.perf_counter()
    rays, dev_s = r.render_into(p, pixels)
    res = RESULT(time.perf_counter() - t0, rays)
    if not quiet:
        info = r.launch_info()
        print(scene_name)
        print("elapsed time:   %.3fs" % res.elapsed_seconds)
        print("total samples:  %d" % (scene.width * scene.height * spp))
        print("total rays:     %d" % res.num_rays)
        print("mrays/s:        %0.2f" % res.get_mrays_per_sec())
        print("device:         hip:%d, %d CUs, %d workgroups x %d" % (r.device, info["compute_units"], info["blocks"], info["threads_per_block"]))
        print("device time:    %.3fms" % (dev_s * 1e3))
        print()
    scene.close()
    if write_tga:
        tga_write_rgb24("out_%s.tga" % scene_name, scene.width, scene.height, pixels)
    if own:
        r.close()
    return res


def tga_write_rgb24(filename, width, height, pixels):
    _check(lib().r1_tga_write_rgb24(filename.encode(), width, height, pixels.ctypes.data_as(_u8p)))
    return True


def log_results(version, scene, results):
    n = len(results)
    el = (C.c_double * n)(*[r.elapsed_seconds for r in results])
    ry = (C.c_uint64 * n)(*[r.num_rays for r in results])
    _check(lib().r1_log_results(version.encode(), scene.encode(), el, ry, n))
