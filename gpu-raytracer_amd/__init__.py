"""ctypes front-end of the MI355X-native path tracer.

Two in-tree shared libraries are loaded from this directory:

* ``csrc/libgrt_device.so`` -- HIP kernels + the C ABI of ``include/gpu_raytracer_amd.h``
* ``host/libgrt_host.so``   -- C++ host classes (Scene, Mitsuba/OBJ loaders, BVH builders,
  Integrator/Pathtracer mirroring the reference's API) plus a flat C shim

Nothing here computes anything: it only marshals numpy arrays into those libraries.  The
libraries must have been built (``python __graft_entry__.py`` or ``make -C gpu-raytracer_amd``);
there is no Python or CPU fallback for the device path.
"""
import ctypes
import fcntl
import os
import tarfile
import tempfile
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_size_t, c_uint8, c_uint32, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
ASSET_DIR = os.path.join(REPO_ROOT, "assets")
DEVICE_LIB_PATH = os.environ.get("GRT_DEVICE_LIB") or os.path.join(_HERE, "csrc", "libgrt_device.so")  # override: kernel-variant experiments
HOST_LIB_PATH = os.path.join(_HERE, "host", "libgrt_host.so")

RT_MAX_BOUNCES = 128
RT_BATCH_SIZE = 1080 * 720
AOV_RADIANCE, AOV_RADIANCE_DIRECT, AOV_RADIANCE_INDIRECT, AOV_ALBEDO, AOV_NORMAL, AOV_POSITION, AOV_COUNT = range(7)
MATERIAL_LIGHT, MATERIAL_DIFFUSE, MATERIAL_PLASTIC, MATERIAL_DIELECTRIC, MATERIAL_CONDUCTOR = range(5)
FILTER_BOX, FILTER_TENT, FILTER_GAUSSIAN = range(3)


class GPUConfig(ctypes.Structure):  # rt_gpu_config
    _fields_ = [("reconstruction_filter", c_int32), ("aov_mask", c_uint32), ("num_bounces", c_int32),
                ("enable_mipmapping", c_int32), ("enable_next_event_estimation", c_int32),
                ("enable_multiple_importance_sampling", c_int32), ("enable_russian_roulette", c_int32),
                ("enable_svgf", c_int32), ("enable_spatial_variance", c_int32), ("enable_taa", c_int32),
                ("alpha_colour", c_float), ("alpha_moment", c_float), ("num_atrous_iterations", c_int32),
                ("sigma_z", c_float), ("sigma_n", c_float), ("sigma_l", c_float)]


class Camera(ctypes.Structure):  # rt_camera
    _fields_ = [("position", c_float * 3), ("bottom_left_corner", c_float * 3), ("x_axis", c_float * 3),
                ("y_axis", c_float * 3), ("pixel_spread_angle", c_float), ("aperture_radius", c_float),
                ("focal_distance", c_float)]


class Counters(ctypes.Structure):  # rt_counters
    _fields_ = [("trace", c_int32 * RT_MAX_BOUNCES), ("shadow", c_int32 * RT_MAX_BOUNCES),
                ("diffuse", c_int32 * RT_MAX_BOUNCES), ("plastic", c_int32 * RT_MAX_BOUNCES),
                ("dielectric", c_int32 * RT_MAX_BOUNCES), ("conductor", c_int32 * RT_MAX_BOUNCES),
                ("ms_generate", c_float), ("ms_trace", c_float), ("ms_sort", c_float), ("ms_shade", c_float),
                ("ms_shadow", c_float), ("ms_post", c_float), ("ms_total", c_float)]


class NoiseEstimateRecord(ctypes.Structure):  # rt_noise_estimate
    _fields_ = [("cells_x", ctypes.c_int32), ("cells_y", ctypes.c_int32), ("pixels", ctypes.c_int64), ("nonfinite_pixels", ctypes.c_int64), ("mean", ctypes.c_double)]


class CellSelectionRecord(ctypes.Structure):  # rt_cell_selection
    _fields_ = [("cells_x", ctypes.c_int32), ("cells_y", ctypes.c_int32), ("hot_cells", ctypes.c_int64), ("active_cells", ctypes.c_int64), ("list_pixels", ctypes.c_int64)]


class ExposureRecord(ctypes.Structure):  # rt_exposure
    _fields_ = [("pixels", ctypes.c_int64), ("dark_pixels", ctypes.c_int64), ("nonfinite_pixels", ctypes.c_int64)]


class DenoiseParams(ctypes.Structure):  # rt_denoise_params
    _fields_ = [("iterations", c_int), ("sigma_l", c_float), ("sigma_n", c_float), ("sigma_z", c_float), ("depth_floor", c_float), ("albedo_floor", c_float)]


# the values DESIGN.md 7.9 settled on (CPUConfig's denoise_* fields hold the same)
DENOISE_DEFAULTS = {"iterations": 5, "sigma_l": 4.0, "sigma_n": 128.0, "sigma_z": 1.0, "depth_floor": 1e-2, "albedo_floor": 1e-2}


def denoise_params(**params):
    unknown = set(params) - set(DENOISE_DEFAULTS)
    if unknown:
        raise TypeError("unknown denoise parameter(s): %s" % ", ".join(sorted(unknown)))
    merged = dict(DENOISE_DEFAULTS, **params)
    if int(merged["iterations"]) != merged["iterations"]:
        raise ValueError("iterations must be a whole number")
    return DenoiseParams(int(merged["iterations"]), *[float(merged[k]) for k in ("sigma_l", "sigma_n", "sigma_z", "depth_floor", "albedo_floor")])


class FireflyParams(ctypes.Structure):  # rt_firefly_params
    _fields_ = [("tiers", c_int), ("start", c_float), ("support", c_float)]


# the values DESIGN.md 7.10 proposes (CPUConfig's firefly_* fields hold the same)
FIREFLY_DEFAULTS = {"tiers": 6, "start": 1.0, "support": 4.0}


def firefly_params(**params):
    unknown = set(params) - set(FIREFLY_DEFAULTS)
    if unknown:
        raise TypeError("unknown firefly parameter(s): %s" % ", ".join(sorted(unknown)))
    merged = dict(FIREFLY_DEFAULTS, **params)
    if int(merged["tiers"]) != merged["tiers"]:
        raise ValueError("tiers must be a whole number")
    return FireflyParams(int(merged["tiers"]), float(merged["start"]), float(merged["support"]))


class DeviceLibraryMissing(RuntimeError):
    pass


_device = None
_host = None


def device_lib():
    """The C-ABI library. Raises loudly when it has not been built: there is no fallback."""
    global _device
    if _device is None:
        if not os.path.exists(DEVICE_LIB_PATH):
            raise DeviceLibraryMissing("%s is missing -- run `python __graft_entry__.py` (build()) first" % DEVICE_LIB_PATH)
        lib = ctypes.CDLL(DEVICE_LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        if hasattr(lib, "rt_abi_version") and lib.rt_abi_version() != 17:
            raise DeviceLibraryMissing("%s has ABI version %d, this front end was written for 17 -- rebuild (python __graft_entry__.py)" % (DEVICE_LIB_PATH, lib.rt_abi_version()))
        lib.rt_last_error.restype = c_char_p
        lib.rt_last_error.argtypes = [c_void_p]
        lib.rt_version.restype = c_char_p
        lib.rt_create.argtypes = [c_int, POINTER(c_void_p)]
        lib.rt_destroy.argtypes = [c_void_p]
        fp, u32p, u8p = POINTER(c_float), POINTER(c_uint32), POINTER(c_uint8)
        lib.rt_trace_rays.argtypes = [c_void_p] + [c_void_p] * 6 + [c_size_t, c_void_p, c_int, POINTER(c_float)]
        lib.rt_trace_shadow_rays.argtypes = [c_void_p] + [c_void_p] * 7 + [c_size_t, c_void_p, c_int, POINTER(c_float)]
        lib.rt_trace_stream_rays.argtypes = [c_void_p, c_int] + [c_void_p] * 6 + [c_size_t, c_void_p] + [c_void_p] * 7 + [c_size_t, c_void_p, c_void_p, c_void_p]
        lib.rt_trace_queue_rays.argtypes = [c_void_p, c_int, c_int, c_int] + [c_void_p] * 6 + [c_size_t, c_void_p] + [c_void_p] * 9 + [c_size_t] + [c_void_p] * 3 + [c_size_t, c_void_p, c_void_p]
        lib.rt_generate_rays.argtypes = [c_void_p, c_int, c_int, c_int] + [c_void_p] * 7
        lib.rt_generate_primary_rays.argtypes = [c_void_p] + [c_int] * 14 + [c_void_p, c_size_t] + [c_void_p] * 8
        lib.rt_random_samples.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_uint32, c_uint32, c_void_p]
        lib.rt_sample_texture.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]
        lib.rt_sample_table.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]
        lib.rt_sample_sky.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_sample_sky_distribution.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_sky_pdf.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_bsdf_eval.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p]
        lib.rt_bsdf_sample.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p]
        lib.rt_sample_lights.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        lib.rt_sort_rays.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_uint32] + [c_void_p] * 9
        lib.rt_shade_rays.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_uint32] + [c_void_p] * 8
        lib.rt_upload_lights.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, c_float]
        lib.rt_upload_material_normal_maps.argtypes = [c_void_p, c_void_p, c_size_t]
        lib.rt_upload_delta_lights.argtypes = [c_void_p, c_void_p, c_size_t, c_float]
        lib.rt_read_delta_lights.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, POINTER(c_size_t), POINTER(c_float)]
        lib.rt_sample_delta_lights.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_upload_geometry.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]
        lib.rt_build_tlas.argtypes = [c_void_p] * 7 + [c_size_t]
        lib.rt_read_instances.argtypes = [c_void_p] * 7
        lib.rt_set_light_tree.argtypes = [c_void_p, c_int]
        lib.rt_get_light_tree.argtypes = [c_void_p]
        lib.rt_read_light_tree.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t]
        lib.rt_sample_light_tree.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_light_tree_pmf.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_set_fog_volume.argtypes = [c_void_p, c_void_p]
        lib.rt_get_fog_volume.argtypes = [c_void_p, c_void_p, POINTER(c_int)]
        lib.rt_fog_segments.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_attenuate_shadow_rays.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_sort_rays_fog.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_uint32] + [c_void_p] * 10 + [POINTER(c_int)]
        lib.rt_set_fog_density.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int]
        lib.rt_get_fog_density_info.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_float), POINTER(c_int)]
        lib.rt_fog_density_segments.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_set_bvh_type.argtypes = [c_void_p, c_int]
        lib.rt_upload_material_opacity.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]
        lib.rt_read_material_opacity.argtypes = [c_void_p, c_int, c_void_p, c_size_t, POINTER(c_int), POINTER(c_int)]
        lib.rt_perturb_normals.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p]
        lib.rt_set_sky_sampling.argtypes = [c_void_p, c_float]
        lib.rt_set_sky.argtypes = [c_void_p, c_void_p, c_int, c_int, c_float]
        lib.rt_upload_media.argtypes = [c_void_p, c_void_p, c_size_t]
        lib.rt_upload_instances.argtypes = [c_void_p] + [c_void_p] * 5 + [c_size_t]
        lib.rt_upload_materials.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
        lib.rt_set_pixel_query.argtypes = [c_void_p, c_int]
        lib.rt_set_svgf_matrices.argtypes = [c_void_p, c_void_p, c_void_p]
        lib.rt_get_sky_sampling.argtypes = [c_void_p, POINTER(c_float)]
        lib.rt_measure_stream_bandwidth.argtypes = [c_void_p, c_size_t, c_int, POINTER(c_float)]
        lib.rt_set_profiling.argtypes = [c_void_p, c_int]
        lib.rt_set_samples_in_flight.argtypes = [c_void_p, c_int]
        lib.rt_set_batch_size.argtypes = [c_void_p, c_int]
        lib.rt_get_counters.argtypes = [c_void_p, POINTER(Counters)]
        lib.rt_render_sample.argtypes = [c_void_p, c_int]
        lib.rt_render_samples.argtypes = [c_void_p, c_int, c_int]
        lib.rt_synchronize.argtypes = [c_void_p]
        lib.rt_set_pixel_range.argtypes = [c_void_p, c_int, c_int]
        lib.rt_read_framebuffer.argtypes = [c_void_p, c_void_p]
        lib.rt_read_aov.argtypes = [c_void_p, c_int, c_void_p, c_int]
        lib.rt_framebuffer_device_ptr.argtypes = [c_void_p, POINTER(c_void_p), POINTER(c_size_t)]
        lib.rt_screen_pitch.argtypes = [c_void_p]
        lib.rt_read_svgf_state.argtypes = [c_void_p, c_int, c_void_p]
        lib.rt_read_luts.argtypes = [c_void_p] + [c_void_p] * 6
        lib.rt_set_config.argtypes = [c_void_p, POINTER(GPUConfig)]
        lib.rt_set_noise_estimate.argtypes = [c_void_p, c_int]
        lib.rt_get_noise_estimate.argtypes = [c_void_p]
        lib.rt_read_noise_moments.argtypes = [c_void_p, c_void_p]
        lib.rt_estimate_noise.argtypes = [c_void_p, c_float, POINTER(NoiseEstimateRecord), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_estimate_noise_images.argtypes = [c_void_p, c_void_p, c_void_p, c_float, POINTER(NoiseEstimateRecord), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
        lib.rt_accumulate_frames.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]
        lib.rt_set_pixel_tiles.argtypes = [c_void_p, c_int, c_int, c_int]
        lib.rt_select_active_cells.argtypes = [c_void_p, c_float, c_float, c_int, POINTER(CellSelectionRecord), c_void_p, c_size_t]
        lib.rt_set_pixel_list.argtypes = [c_void_p, c_int]
        lib.rt_get_pixel_list.argtypes = [c_void_p]
        lib.rt_read_pixel_list.argtypes = [c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]
        lib.rt_select_pixels_images.argtypes = [c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, POINTER(CellSelectionRecord), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]
        lib.rt_accumulate_list_frames.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_uint32, c_void_p]
        lib.rt_denoise.argtypes = [c_void_p, POINTER(DenoiseParams)]
        lib.rt_read_denoised.argtypes = [c_void_p, c_void_p]
        lib.rt_denoise_timed.argtypes = [c_void_p, POINTER(DenoiseParams), c_int, c_void_p, c_size_t, POINTER(c_size_t)]
        lib.rt_denoise_images.argtypes = [c_void_p, c_int, c_int, c_int] + [c_void_p] * 7 + [POINTER(DenoiseParams), c_int, c_void_p]
        lib.rt_set_firefly_cascade.argtypes = [c_void_p, POINTER(FireflyParams)]
        lib.rt_get_firefly_cascade.argtypes = [c_void_p, POINTER(FireflyParams)]
        lib.rt_read_firefly_cascade.argtypes = [c_void_p, c_void_p, c_size_t]
        lib.rt_resolve_fireflies.argtypes = [c_void_p, c_float]
        lib.rt_read_resolved.argtypes = [c_void_p, c_void_p]
        lib.rt_resolve_fireflies_timed.argtypes = [c_void_p, c_float, c_int, POINTER(c_float)]
        lib.rt_set_denoise_source.argtypes = [c_void_p, c_int]
        lib.rt_get_denoise_source.argtypes = [c_void_p]
        lib.rt_accumulate_cascade_frames.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, POINTER(FireflyParams), c_void_p, c_uint32, c_void_p]
        lib.rt_resolve_fireflies_images.argtypes = [c_void_p, c_int, c_int, c_int] + [c_void_p] * 4 + [POINTER(FireflyParams), c_int, c_void_p]
        lib.rt_measure_exposure.argtypes = [c_void_p, POINTER(ExposureRecord), c_void_p]
        lib.rt_measure_exposure_images.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, POINTER(ExposureRecord), c_void_p]
        lib.rt_estimate_noise_robust.argtypes = [c_void_p, c_float, c_float, POINTER(NoiseEstimateRecord), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, POINTER(ctypes.c_int64)]
        lib.rt_estimate_noise_robust_images.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, POINTER(NoiseEstimateRecord), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                                        POINTER(ctypes.c_int64)]
        lib.rt_select_pixels_robust_images.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_int, POINTER(CellSelectionRecord), c_void_p, c_void_p, c_void_p, c_void_p,
                                                       c_void_p, c_size_t, c_void_p, c_size_t]
        lib.rt_set_noise_robust.argtypes = [c_void_p, c_float]
        lib.rt_get_noise_robust.argtypes = [c_void_p]
        lib.rt_get_noise_robust.restype = c_float
        _device = lib
    return _device


def host_lib():
    global _host
    if _host is None:
        device_lib()  # libgrt_host.so links against it
        if not os.path.exists(HOST_LIB_PATH):
            raise DeviceLibraryMissing("%s is missing -- run `python __graft_entry__.py` (build()) first" % HOST_LIB_PATH)
        os.environ.setdefault("GRT_ASSET_DIR", ASSET_DIR)
        lib = ctypes.CDLL(HOST_LIB_PATH)
        lib.grt_last_error.restype = c_char_p
        lib.grt_config_set.argtypes = [c_char_p, c_double]
        lib.grt_config_get.argtypes = [c_char_p]
        lib.grt_config_set_string.argtypes = [c_char_p, c_char_p]
        lib.grt_scene_set_fog.argtypes = [c_void_p, POINTER(c_float)]
        lib.grt_scene_get_fog.argtypes = [c_void_p, POINTER(c_float)]
        lib.grt_scene_clear_fog.argtypes = [c_void_p]
        lib.grt_scene_set_fog_density.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int]
        lib.grt_scene_get_fog_density.argtypes = [c_void_p, POINTER(c_int), c_void_p, c_size_t]
        lib.grt_scene_clear_fog_density.argtypes = [c_void_p]
        lib.grt_vol_read.argtypes = [c_char_p, POINTER(c_int), POINTER(c_float), c_void_p, c_size_t]
        lib.grt_vol_write.argtypes = [c_char_p, c_void_p, c_int, c_int, c_int, POINTER(c_float)]
        lib.grt_config_get.restype = c_double
        lib.grt_scene_load.restype = c_void_p
        lib.grt_scene_load.argtypes = [c_char_p, c_char_p]
        lib.grt_scene_free.argtypes = [c_void_p]
        for name in ("grt_scene_mesh_count", "grt_scene_material_count", "grt_scene_texture_count", "grt_scene_mesh_data_count", "grt_scene_wait_until_loaded"):
            getattr(lib, name).argtypes = [c_void_p]
        lib.grt_scene_bvh_build_ms.argtypes = [c_void_p]
        lib.grt_scene_bvh_build_ms.restype = c_double
        lib.grt_scene_set_sky_scale.argtypes = [c_void_p, c_float]
        lib.grt_scene_set_camera.argtypes = [c_void_p, POINTER(c_float), POINTER(c_float), c_float]
        lib.grt_scene_get_camera.argtypes = [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float)]
        lib.grt_scene_set_material.argtypes = [c_void_p, c_int, c_int, POINTER(c_float), c_float]
        lib.grt_scene_material_type.argtypes = [c_void_p, c_int]
        lib.grt_scene_material_normal_map.argtypes = [c_void_p, c_int]
        lib.grt_scene_set_material_normal_map.argtypes = [c_void_p, c_int, c_int]
        lib.grt_scene_material_opacity_map.argtypes = [c_void_p, c_int, POINTER(c_int), POINTER(c_float)]
        lib.grt_scene_set_material_opacity_map.argtypes = [c_void_p, c_int, c_int, c_int, c_float]
        lib.grt_scene_add_texture.argtypes = [c_void_p, c_char_p, c_int]
        lib.grt_scene_delta_light_count.argtypes = [c_void_p]
        lib.grt_scene_get_delta_light.argtypes = [c_void_p, c_int, POINTER(c_float)]
        lib.grt_scene_add_delta_light.argtypes = [c_void_p, POINTER(c_float)]
        lib.grt_scene_clear_delta_lights.argtypes = [c_void_p]
        lib.grt_pathtracer_delta_light_share.restype = c_float
        lib.grt_pathtracer_delta_light_share.argtypes = [c_void_p]
        lib.grt_scene_texture_compressed.argtypes = [c_void_p, c_int]
        lib.grt_mesh_data_array.restype = c_void_p
        lib.grt_mesh_data_array.argtypes = [c_void_p, c_int, c_char_p, POINTER(c_size_t)]
        lib.grt_scene_set_mesh_transform.argtypes = [c_void_p, c_int, POINTER(c_float), POINTER(c_float), c_float]
        lib.grt_scene_get_mesh_transform.argtypes = [c_void_p, c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float)]
        lib.grt_pathtracer_create.restype = c_void_p
        lib.grt_pathtracer_create.argtypes = [c_void_p, c_int, c_int, c_int]
        lib.grt_ao_create.restype = c_void_p
        lib.grt_ao_create.argtypes = [c_void_p, c_int, c_int, c_int]
        lib.grt_ao_set_radius.argtypes = [c_void_p, c_float]
        lib.grt_pathtracer_free.argtypes = [c_void_p]
        lib.grt_pathtracer_update.argtypes = [c_void_p, c_float]
        lib.grt_pathtracer_render.argtypes = [c_void_p]
        lib.grt_pathtracer_set_pixel_query.argtypes = [c_void_p, c_int, c_int]
        lib.grt_pathtracer_get_pixel_query.argtypes = [c_void_p] + [POINTER(c_int)] * 4
        lib.grt_pathtracer_render_samples.argtypes = [c_void_p, c_int]
        lib.grt_pathtracer_resize.argtypes = [c_void_p, c_int, c_int]
        lib.grt_pathtracer_set_pixel_range.argtypes = [c_void_p, c_int, c_int]
        lib.grt_pathtracer_sample_index.argtypes = [c_void_p]
        lib.grt_pathtracer_screen_pitch.argtypes = [c_void_p]
        lib.grt_pathtracer_invalidate.argtypes = [c_void_p, c_char_p]
        lib.grt_pathtracer_aov_enable.argtypes = [c_void_p, c_int, c_int]
        lib.grt_pathtracer_context.restype = c_void_p
        lib.grt_pathtracer_context.argtypes = [c_void_p]
        lib.grt_pathtracer_device_blas_build_ms.restype = c_float
        lib.grt_pathtracer_device_blas_build_ms.argtypes = [c_void_p]
        lib.grt_pathtracer_static_geometry_members.restype = c_int
        lib.grt_pathtracer_static_geometry_members.argtypes = [c_void_p]
        lib.grt_pathtracer_static_geometry_whole_scene.restype = c_int
        lib.grt_pathtracer_static_geometry_whole_scene.argtypes = [c_void_p]
        lib.grt_pathtracer_skip_behind_hit.restype = c_int
        lib.grt_pathtracer_skip_behind_hit.argtypes = [c_void_p]
        lib.grt_pathtracer_static_geometry_root.restype = c_int
        lib.grt_pathtracer_static_geometry_root.argtypes = [c_void_p]
        lib.grt_pathtracer_static_geometry_top_nodes.restype = c_int
        lib.grt_pathtracer_static_geometry_top_nodes.argtypes = [c_void_p]
        lib.grt_pathtracer_set_flatten_asynchronously.restype = None
        lib.grt_pathtracer_set_flatten_asynchronously.argtypes = [c_void_p, c_int]
        lib.grt_pathtracer_set_reseat_asynchronously.restype = None
        lib.grt_pathtracer_set_reseat_asynchronously.argtypes = [c_void_p, c_int]
        lib.grt_pathtracer_reseats_completed.restype = c_int
        lib.grt_pathtracer_reseats_completed.argtypes = [c_void_p]
        lib.grt_pathtracer_reseat_pending.restype = c_int
        lib.grt_pathtracer_reseat_pending.argtypes = [c_void_p]
        lib.grt_pathtracer_last_reseat_seconds.restype = ctypes.c_double
        lib.grt_pathtracer_last_reseat_seconds.argtypes = [c_void_p]
        lib.grt_pathtracer_reflattens_completed.restype = c_int
        lib.grt_pathtracer_reflattens_completed.argtypes = [c_void_p]
        lib.grt_pathtracer_reflatten_in_progress.restype = c_int
        lib.grt_pathtracer_reflatten_in_progress.argtypes = [c_void_p]
        lib.grt_pathtracer_static_geometry_bytes.restype = ctypes.c_double
        lib.grt_pathtracer_static_geometry_bytes.argtypes = [c_void_p]
        lib.grt_pathtracer_static_geometry_build_seconds.restype = ctypes.c_double
        lib.grt_pathtracer_static_geometry_build_seconds.argtypes = [c_void_p]
        lib.grt_pathtracer_lights_total_weight.restype = c_float
        lib.grt_pathtracer_lights_total_weight.argtypes = [c_void_p]
        lib.grt_pathtracer_read_aov.argtypes = [c_void_p, c_int, c_int, c_void_p]
        lib.grt_pathtracer_read_framebuffer.argtypes = [c_void_p, c_void_p]
        lib.grt_pathtracer_save_image.argtypes = [c_void_p, c_char_p]
        lib.grt_export_image.argtypes = [c_char_p, c_int, c_int, c_int, c_void_p]
        lib.grt_pathtracer_denoise.argtypes = [c_void_p, c_void_p, c_void_p]
        lib.grt_pathtracer_save_denoised_image.argtypes = [c_void_p, c_char_p, c_void_p]
        lib.grt_pathtracer_resolve_fireflies.argtypes = [c_void_p, ctypes.c_double, c_void_p]
        lib.grt_pathtracer_save_resolved_image.argtypes = [c_void_p, c_char_p, ctypes.c_double]
        lib.grt_pathtracer_array.restype = c_void_p
        lib.grt_pathtracer_array.argtypes = [c_void_p, c_char_p, POINTER(c_size_t)]
        lib.grt_pathtracer_sky_size.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_float)]
        lib.grt_pathtracer_texture.argtypes = [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_int)]
        lib.grt_pathtracer_device_config.argtypes = [c_void_p, POINTER(GPUConfig)]
        lib.grt_pathtracer_counters.argtypes = [c_void_p, POINTER(Counters)]
        lib.grt_frame_split_create.restype = c_void_p
        lib.grt_frame_split_create.argtypes = [c_void_p, c_int, c_int, POINTER(c_int), c_int]
        lib.grt_frame_split_free.argtypes = [c_void_p]
        lib.grt_frame_split_update.argtypes = [c_void_p, c_float]
        lib.grt_frame_split_render.argtypes = [c_void_p]
        lib.grt_frame_split_render_samples.argtypes = [c_void_p, c_int]
        lib.grt_frame_split_submitting_threads.restype = c_int
        lib.grt_frame_split_submitting_threads.argtypes = [c_void_p]
        lib.grt_frame_split_rank.restype = c_void_p
        lib.grt_frame_split_rank.argtypes = [c_void_p, c_int]
        lib.grt_build_blas.restype = c_void_p
        lib.grt_build_blas.argtypes = [c_void_p, c_int]
        lib.grt_build_static_bvh.restype = c_void_p
        lib.grt_build_static_bvh.argtypes = [c_void_p, c_int, c_int]
        lib.grt_build_device_bvh.restype = c_void_p
        lib.grt_build_device_bvh.argtypes = [c_void_p, c_int, c_int]
        lib.grt_built_array.restype = c_void_p
        lib.grt_built_array.argtypes = [c_void_p, c_char_p, POINTER(c_size_t)]
        lib.grt_built_free.argtypes = [c_void_p]
        lib.grt_built_learn_slot_order.restype = c_int
        lib.grt_built_learn_slot_order.argtypes = [c_void_p, c_int, c_int]
        _host = lib
    return _host


def _host_check(status):
    if status != 0:
        raise RuntimeError(host_lib().grt_last_error().decode(errors="replace"))


def _view(ptr, nbytes, dtype):
    if not ptr or nbytes == 0:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_char * nbytes).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


# ---- scenes ---------------------------------------------------------------------------------------

SCENES = {"cornellbox": ("cornellbox.tar.xz", "cornellbox/scene.xml"), "sponza": ("sponza_geometry.tar.xz", "Sponza/scene.xml")}


def scene_path(name):
    """Path of a bundled scene's xml; archives under assets/scenes are unpacked on first use.

    'cornellbox' and 'sponza' are the geometry of the reference's Data/cornellbox and
    Data/Sponza (Crytek Sponza), packed because /root/reference does not exist on the GPU box.
    They are unpacked into assets/_cache (build() does it for Sponza). A tree built by one user and run by another
    can leave that cache readable but not writable: what it holds is used as it is, what it lacks goes to user_cache_dir().
    """
    cache = os.path.join(ASSET_DIR, "_cache")
    if name == "sponza_reference_maps":   # Sponza with the reference's own texture files (install_reference_sponza_textures)
        if not reference_sponza_textures_installed():
            raise FileNotFoundError("the reference's Sponza textures are not installed (build() copies them where /root/reference is mounted)")
        scene_path("sponza")
        return os.path.join(cache, "Sponza", "scene_reference_maps.xml")
    if name not in SCENES:
        raise KeyError("unknown bundled scene %r" % name)
    if not _unpack_scene(cache, name):
        cache = user_cache_dir()
        if not _unpack_scene(cache, name):
            raise PermissionError("cannot unpack the bundled scene %r: neither %s nor %s can be written" % (name, os.path.join(ASSET_DIR, "_cache"), cache))
    return os.path.join(cache, SCENES[name][1])


def user_cache_dir():
    """Where this user unpacks the bundled scenes that assets/_cache lacks and cannot take."""
    return os.path.join(tempfile.gettempdir(), "gpu_raytracer_amd-%d" % os.getuid(), "_cache")


def _unpack_scene(cache, name):
    """Unpacks bundled scene `name` under `cache` unless it is complete there already. False: it is not, and `cache`
    cannot be written."""
    archive, xml = SCENES[name]
    done = os.path.join(cache, "." + archive + ".complete")   # written after the last file of the scene
    if os.path.exists(done) and (name != "sponza" or _sponza_textures_unpacked(cache)):
        return True
    try:
        os.makedirs(cache, exist_ok=True)
    except PermissionError:
        return False
    lock = os.open(cache, os.O_RDONLY)   # the lock is the directory itself: taking it needs no write permission
    try:
        fcntl.flock(lock, fcntl.LOCK_EX)   # the ranks of a multi-GPU job start together
        if not os.path.exists(os.path.join(cache, xml)):
            with tarfile.open(os.path.join(ASSET_DIR, "scenes", archive)) as tar:
                tar.extractall(cache)
        if name == "sponza":
            _unpack_sponza_textures(cache)
        if not os.path.exists(done):
            open(done, "w").close()
    except PermissionError:
        # a cache another user unpacked before the markers existed: complete if it has the scene, else not ours to fill
        return os.path.exists(os.path.join(cache, xml)) and (name != "sponza" or _sponza_textures_unpacked(cache))
    finally:
        os.close(lock)   # (closing releases the lock)
    return True


REFERENCE_SPONZA_TEXTURES = "/root/reference/Data/Sponza/textures"


def install_reference_sponza_textures():
    """Called by build() (which runs where /root/reference is mounted): the 19 diffuse maps Data/Sponza/scene.xml finds upstream
    go, as they are, into assets/_cache/Sponza/textures_reference/ next to a copy of the scene file that names them
    (scene_path("sponza_reference_maps")). assets/_cache is git-ignored (nothing of the reference enters the history) but
    travels to the GPU box with the snapshot, so the benchmark there renders the real texture set instead of the quarter-size
    maps replicated 4x4 that travel inside the repository. Returns the number of maps in place (0: no reference mount)."""
    import re
    import shutil
    xml = scene_path("sponza")
    directory = os.path.dirname(xml)
    target = os.path.join(directory, "textures_reference")
    done = os.path.join(target, ".complete")
    if os.path.exists(done):
        return len([n for n in os.listdir(target) if n.endswith(".tga")])
    if not os.path.isdir(REFERENCE_SPONZA_TEXTURES):
        return 0
    text = open(xml).read()
    names = sorted(set(re.findall(r"textures[\\/]+([A-Za-z0-9_]+\.tga)", text)))
    os.makedirs(target, exist_ok=True)
    count = 0
    for name in names:
        source = os.path.join(REFERENCE_SPONZA_TEXTURES, name)
        if os.path.exists(source):       # (5 of the 24 are missing upstream as well: the loader's fallback texel, as in the reference)
            shutil.copyfile(source, os.path.join(target, name + ".part")); os.replace(os.path.join(target, name + ".part"), os.path.join(target, name))
            count += 1
    with open(os.path.join(directory, "scene_reference_maps.xml"), "w") as f:
        f.write(re.sub(r"textures[\\/]+([A-Za-z0-9_]+\.tga)", r"textures_reference/\1", text))
    open(done, "w").close()
    return count


def reference_sponza_textures_installed():
    return os.path.exists(os.path.join(ASSET_DIR, "_cache", "Sponza", "textures_reference", ".complete"))


def _sponza_textures_unpacked(cache):
    return os.path.exists(os.path.join(cache, "Sponza", "textures", ".complete")) or not os.path.exists(os.path.join(ASSET_DIR, "scenes", "sponza_textures_256.tar.xz"))


def _unpack_sponza_textures(cache):
    """The 19 diffuse maps of Data/Sponza/textures travel at a quarter of their side length
    (tools/pack_sponza_textures.py); every texel is replicated 4x4 here so that the renderer loads
    textures of the reference's dimensions (mip chain depth, memory footprint, LOD selection)."""
    done = os.path.join(cache, "Sponza", "textures", ".complete")
    archive = os.path.join(ASSET_DIR, "scenes", "sponza_textures_256.tar.xz")
    if os.path.exists(done) or not os.path.exists(archive):
        return
    os.makedirs(os.path.dirname(done), exist_ok=True)
    with tarfile.open(archive) as tar:
        for member in tar.getmembers():
            data = tar.extractfile(member).read()
            w, h, bpp, desc = np.frombuffer(data, np.uint16, 2, 12).tolist() + [data[16], data[17]]
            channels = bpp // 8
            px = np.frombuffer(data, np.uint8, w * h * channels, 18).reshape(h, w, channels)
            big = np.repeat(np.repeat(px, 4, axis=0), 4, axis=1)
            header = bytearray(data[:18])
            header[12:16] = np.array([w * 4, h * 4], np.uint16).tobytes()
            tmp = os.path.join(os.path.dirname(done), os.path.basename(member.name))
            with open(tmp + ".part", "wb") as f:
                f.write(bytes(header) + big.tobytes())
            os.replace(tmp + ".part", tmp)
    open(done, "w").close()


def config_reset():
    host_lib().grt_config_reset()


BVH_TYPES = {"sbvh": 1, "sah": 2, "bvh": 2, "bvh4": 4, "bvh8": 8}   # the reference's --bvh names (Args.cpp:71-84)


def config_set(**kwargs):
    lib = host_lib()
    for key, value in kwargs.items():
        if key == "bvh_type" and isinstance(value, str):
            value = BVH_TYPES[value.lower()]
        if key in ("fog", "fog_sigma_a", "fog_sigma_s", "fog_density") and not isinstance(value, (int, float)):   # "off" or a box; one number or three; "off" or a path
            text = str(value) if isinstance(value, (str, os.PathLike)) else ",".join(repr(float(v)) for v in value)
            if lib.grt_config_set_string(key.encode(), text.encode()) != 0:
                raise KeyError(lib.grt_last_error().decode(errors="replace"))
            continue
        if lib.grt_config_set(key.encode(), float(value)) != 0:
            raise KeyError(lib.grt_last_error().decode(errors="replace"))


def load_texture(filename, block_compression=False):
    """Decodes an image file the way the scene loader does (TGA / PPM / PNG / BMP: sRGB -> linear RGBA8 +
    box-filtered mips; DDS: stored DXT levels as they are). Returns a list of (height, width, 4) uint8 levels.
    block_compression: False = the decoded levels; True = what survives BC1 (power-of-two textures only, the
    scene loader's default); None = whatever `enable_block_compression` says."""
    lib = host_lib()
    if block_compression is not None:
        previous = config_get("enable_block_compression")
        config_set(enable_block_compression=int(bool(block_compression)))
        try:
            return load_texture(filename, None)
        finally:
            config_set(enable_block_compression=previous)
    lib.grt_texture_load.restype = c_void_p
    lib.grt_texture_load.argtypes = [c_char_p]
    lib.grt_texture_data.restype = c_void_p
    lib.grt_texture_data.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_size_t)]
    lib.grt_texture_free.argtypes = [c_void_p]
    handle = lib.grt_texture_load(str(filename).encode())
    if not handle:
        raise RuntimeError(lib.grt_last_error().decode(errors="replace"))
    w, h, levels, nbytes = c_int(), c_int(), c_int(), c_size_t()
    ptr = lib.grt_texture_data(handle, byref(w), byref(h), byref(levels), byref(nbytes))
    data = _view(ptr, nbytes.value, np.uint8).copy()
    lib.grt_texture_free(handle)
    out, offset = [], 0
    for l in range(levels.value):
        lw, lh = max(w.value >> l, 1), max(h.value >> l, 1)
        out.append(data[offset:offset + lw * lh * 4].reshape(lh, lw, 4))
        offset += lw * lh * 4
    return out


def export_image(filename, rgb):
    """Writes a (height, width, 3) float32 image (row 0 at the bottom, as the integrator holds frames)
    through the host's PPM / EXR exporters."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w, _ = rgb.shape
    lib = host_lib()
    _host_check(lib.grt_export_image(str(filename).encode(), w, w, h, rgb.ctypes.data))


def config_get(key):
    return host_lib().grt_config_get(key.encode())


class Scene:
    """reference: Src/Renderer/Scene.h -- loads one .xml/.obj scene file."""

    def __init__(self, filename, sky=None):
        lib = host_lib()
        self.handle = lib.grt_scene_load(os.fsencode(filename), os.fsencode(sky) if sky else b"")
        if not self.handle:
            raise RuntimeError("scene load failed: " + lib.grt_last_error().decode(errors="replace"))

    def close(self):
        if self.handle:
            host_lib().grt_scene_free(self.handle)
            self.handle = None

    def wait_until_loaded(self):
        _host_check(host_lib().grt_scene_wait_until_loaded(self.handle))

    @property
    def mesh_count(self):
        return host_lib().grt_scene_mesh_count(self.handle)

    @property
    def material_count(self):
        return host_lib().grt_scene_material_count(self.handle)

    @property
    def mesh_data_count(self):
        return host_lib().grt_scene_mesh_data_count(self.handle)

    @property
    def bvh_build_ms(self):
        return host_lib().grt_scene_bvh_build_ms(self.handle)

    def mesh_data_array(self, index, name, dtype):
        n = c_size_t()
        ptr = host_lib().grt_mesh_data_array(self.handle, index, name.encode(), byref(n))
        return _view(ptr, n.value, dtype)

    def describe(self):
        """One line per object the loaders produced (floats as bit patterns)."""
        lib = host_lib()
        lib.grt_scene_describe.restype = ctypes.c_size_t
        lib.grt_scene_describe.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        n = lib.grt_scene_describe(self.handle, None, 0)
        buf = ctypes.create_string_buffer(n)
        lib.grt_scene_describe(self.handle, buf, n)
        return buf.value.decode(errors="replace")

    def texture(self, index):
        """-> dict(width, height, lod_width, lod_height, mip_offsets (texels), texels (RGBA8, all levels))"""
        lib = host_lib()
        lib.grt_scene_texture_info.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        lib.grt_scene_texture_data.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        info = (ctypes.c_int * 6)()
        if lib.grt_scene_texture_info(self.handle, index, info) != 0:
            raise RuntimeError(lib.grt_last_error().decode(errors="replace"))
        texels = np.zeros((info[5], 4), np.uint8); offsets = np.zeros(info[2], np.int32)
        lib.grt_scene_texture_data(self.handle, index, texels.ctypes.data, offsets.ctypes.data)
        return dict(width=info[0], height=info[1], lod_width=info[3], lod_height=info[4], mip_offsets=offsets, texels=texels)

    def sky(self):
        lib = host_lib()
        lib.grt_scene_sky.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        out = np.zeros((lib.grt_scene_sky(self.handle, None), 4), np.float32)
        lib.grt_scene_sky(self.handle, out.ctypes.data)
        return out

    def set_camera(self, position, rotation, fov=-1.0):
        pos = (c_float * 3)(*position)
        rot = (c_float * 4)(*rotation)
        host_lib().grt_scene_set_camera(self.handle, pos, rot, float(fov))

    def get_camera(self):
        pos, rot, fov = (c_float * 3)(), (c_float * 4)(), c_float()
        host_lib().grt_scene_get_camera(self.handle, pos, rot, byref(fov))
        return list(pos), list(rot), fov.value

    def set_sky_scale(self, scale):
        host_lib().grt_scene_set_sky_scale(self.handle, float(scale))

    def mesh_transform(self, index):
        """(position[3], rotation quaternion xyzw[4], scale) of mesh `index` (Mesh.h: position / rotation / scale)."""
        pos, rot, scale = (c_float * 3)(), (c_float * 4)(), c_float()
        _host_check(host_lib().grt_scene_get_mesh_transform(self.handle, index, pos, rot, byref(scale)))
        return list(pos), list(rot), scale.value

    def set_mesh_transform(self, index, position, rotation_xyzw, scale):
        """Edit a mesh's transform as the reference's UI does; the next update() with invalidate("scene")
        (or enable_scene_update) rebuilds the TLAS."""
        _host_check(host_lib().grt_scene_set_mesh_transform(self.handle, index, (c_float * 3)(*position), (c_float * 4)(*rotation_xyzw), float(scale)))

    def set_material(self, index, mtype, diffuse=None, linear_roughness=0.5):
        d = (c_float * 3)(*diffuse) if diffuse is not None else None
        _host_check(host_lib().grt_scene_set_material(self.handle, index, mtype, d, float(linear_roughness)))

    def material_type(self, index):
        return host_lib().grt_scene_material_type(self.handle, index)

    def material_normal_map(self, index):
        """The texture index of material `index`'s tangent-space normal map, -1 for none (kept out of describe())."""
        t = host_lib().grt_scene_material_normal_map(self.handle, index)
        if t < -1:
            raise RuntimeError(host_lib().grt_last_error().decode(errors="replace"))
        return t

    def set_material_normal_map(self, index, texture):
        """Give material `index` the normal map `texture` (a texture index of this scene; -1: none). A Pathtracer sees it after
        invalidate("materials") and update()."""
        _host_check(host_lib().grt_scene_set_material_normal_map(self.handle, index, int(texture)))

    # Delta emitters: lights without area, found by next-event estimation alone. A Pathtracer sees a change after
    # invalidate("delta_lights") and update(). Kept out of describe().
    def _add_delta_light(self, kind, position, direction, intensity, cutoff, beam):
        v = (c_float * 12)(float(kind), *[float(x) for x in position], *[float(x) for x in direction], *[float(x) for x in intensity], float(cutoff), float(beam))
        index = host_lib().grt_scene_add_delta_light(self.handle, v)
        if index < 0:
            raise ValueError(host_lib().grt_last_error().decode(errors="replace"))
        return index

    def add_point_light(self, position, intensity):
        """A point light at `position` with RGB `intensity` in W/sr. Returns its index."""
        return self._add_delta_light(DELTA_LIGHT_POINT, position, (0, 0, 1), intensity, 0.0, 0.0)

    def add_spot_light(self, position, direction, intensity, cutoff, beam=None):
        """A spot at `position` shining along `direction`: `intensity` (W/sr) inside the angle `beam` from the axis, none outside `cutoff`
        (radians; beam defaults to 3/4 of the cutoff), linear in the angle between. Returns its index."""
        return self._add_delta_light(DELTA_LIGHT_SPOT, position, direction, intensity, cutoff, 0.75 * cutoff if beam is None else beam)

    def add_directional_light(self, direction, irradiance):
        """A directional light whose light travels along `direction`, with RGB `irradiance` in W/m^2 on a surface facing it. Returns its index."""
        return self._add_delta_light(DELTA_LIGHT_DIRECTIONAL, (0, 0, 0), direction, irradiance, 0.0, 0.0)

    def set_fog(self, box_min, box_max, sigma_a, sigma_s, g=0.0):
        """The scene-wide fog volume: a homogeneous medium inside the box, absorption and scattering per unit length (one number
        or RGB), Henyey-Greenstein asymmetry g in (-1, 1). Takes effect at the next update() after Pathtracer.invalidate("fog")."""
        r = fog_volume_record(box_min, box_max, sigma_a, sigma_s, g)
        values = (c_float * 13)(*[float(v) for v in r[:13]])
        _host_check(host_lib().grt_scene_set_fog(self.handle, values))

    def clear_fog(self):
        host_lib().grt_scene_clear_fog(self.handle)

    @property
    def fog(self):
        """None, or the volume as a dict {box_min, box_max, sigma_a, sigma_s (3 floats each), g}."""
        values = (c_float * 13)()
        if not host_lib().grt_scene_get_fog(self.handle, values):
            return None
        v = [float(x) for x in values]
        return dict(box_min=tuple(v[0:3]), box_max=tuple(v[3:6]), sigma_a=tuple(v[6:9]), sigma_s=tuple(v[9:12]), g=v[12])

    def set_fog_density(self, density):
        """The density grid of the fog volume: an array of shape (nz, ny, nx) of finite values >= 0, laid over the box of the fog
        volume; inside a voxel the volume's sigmas are multiplied by its value. Takes effect at the next update() after Pathtracer.invalidate("fog")."""
        d = _f32(density)
        if d.ndim != 3:
            raise ValueError("a density grid has shape (nz, ny, nx), not %r" % (d.shape,))
        _host_check(host_lib().grt_scene_set_fog_density(self.handle, d.ctypes.data, d.shape[2], d.shape[1], d.shape[0]))

    def clear_fog_density(self):
        host_lib().grt_scene_clear_fog_density(self.handle)

    @property
    def fog_density(self):
        """None, or the density grid as a float32 array of shape (nz, ny, nx)."""
        dims = (c_int * 3)()
        if not host_lib().grt_scene_get_fog_density(self.handle, dims, None, 0):
            return None
        out = np.zeros((dims[2], dims[1], dims[0]), np.float32)
        host_lib().grt_scene_get_fog_density(self.handle, dims, out.ctypes.data, out.size)
        return out

    def clear_delta_lights(self):
        host_lib().grt_scene_clear_delta_lights(self.handle)

    def delta_lights(self):
        """(N, 12) float32 {type (0 point, 1 spot, 2 directional), position[3], direction[3], intensity[3], cutoff, beam (radians)}."""
        lib = host_lib()
        out = np.zeros((lib.grt_scene_delta_light_count(self.handle), 12), np.float32)
        for i in range(out.shape[0]):
            _host_check(lib.grt_scene_get_delta_light(self.handle, i, out[i].ctypes.data_as(POINTER(c_float))))
        return out

    def material_opacity_map(self, index):
        """The opacity mask of material `index`: (texture index, channel 0..3, threshold), or None (kept out of
        describe()). Decodes the scene's textures first: the channel of a loaded `mask` is alpha when its file has four channels."""
        channel, threshold = c_int(), c_float()
        t = host_lib().grt_scene_material_opacity_map(self.handle, index, byref(channel), byref(threshold))
        if t < -1:
            raise RuntimeError(host_lib().grt_last_error().decode(errors="replace"))
        return None if t < 0 else (t, channel.value, threshold.value)

    def set_material_opacity_map(self, index, texture, channel=3, threshold=0.5):
        """Cut material `index` out by level 0 of `texture` (a data texture of this scene, add_texture(..., normal_map=True); -1: none):
        texels whose `channel` byte is below ceil(threshold * 255) let rays through. A Pathtracer sees it after invalidate("materials")
        and update()."""
        _host_check(host_lib().grt_scene_set_material_opacity_map(self.handle, index, int(texture), int(channel), float(threshold)))

    def add_texture(self, filename, normal_map=False):
        """Add an image file as a texture; normal_map=True loads it as data (no sRGB decode, never block-compressed). Returns its
        index. Textures reach the device when a Pathtracer is created: add them before."""
        t = host_lib().grt_scene_add_texture(self.handle, os.fsencode(filename), 1 if normal_map else 0)
        if t < 0:
            raise RuntimeError(host_lib().grt_last_error().decode(errors="replace"))
        return t

    def texture_compressed(self, index):
        """True when texture `index` is kept as BC1 blocks (block compression), False for RGBA8 texels."""
        c = host_lib().grt_scene_texture_compressed(self.handle, index)
        if c < 0:
            raise RuntimeError(host_lib().grt_last_error().decode(errors="replace"))
        return bool(c)


_ARRAY_DTYPES = {
    "triangles": np.float32, "bvh8_nodes": np.uint8, "bvh2_nodes": np.uint8, "bvh4_nodes": np.uint8, "reverse_indices": np.int32,
    "mesh_bvh_root_indices": np.int32, "mesh_material_ids": np.int32, "mesh_transforms": np.float32,
    "mesh_transforms_inv": np.float32, "mesh_transforms_prev": np.float32, "material_types": np.uint8,
    "materials": np.float32, "media": np.float32, "tlas_indices": np.int32, "tlas_nodes": np.uint8,
    "tlas_raw_nodes": np.uint8, "pmj_samples": np.float32, "blue_noise": np.uint8,
    "light_triangle_indices": np.int32, "light_triangle_cumulative_probability": np.float32,
    "light_mesh_cumulative_probability": np.float32, "light_mesh_triangle_span": np.int32,
    "light_mesh_transform_indices": np.int32, "sky": np.float32, "camera": np.uint8, "svgf_matrices": np.float32,
    "scene_order_roots": np.int32, "scene_order_materials": np.int32, "scene_order_transforms": np.float32,
    "scene_order_transforms_inv": np.float32, "scene_order_transforms_prev": np.float32, "scene_order_boxes": np.float32,
    "alias_mesh_ids": np.int32, "alias_triangle_ids": np.int32,
    "delta_light_records": np.float32,   # rt_delta_light, 16 words each; word 0 is the type (int32 bits)
}


class Pathtracer:
    """reference: Src/Renderer/Integrators/Pathtracer.h -- update()/render() protocol.

    device < 0 creates a host-only integrator that bakes the device data formats but cannot
    render (used by the CPU tests and the oracle).
    """

    _create = "grt_pathtracer_create"

    def __init__(self, scene, width, height, device=0):
        lib = host_lib()
        self.scene = scene
        self.handle = getattr(lib, self._create)(scene.handle, width, height, device)
        if not self.handle:
            raise RuntimeError("%s creation failed: %s" % (type(self).__name__, lib.grt_last_error().decode(errors="replace")))
        self.width, self.height = width, height

    def close(self):
        if self.handle:
            host_lib().grt_pathtracer_free(self.handle)
            self.handle = None

    def set_light_tree(self, enable):
        """The light tree of next-event estimation: config key light_tree, applied by the next update(), after the light tables are uploaded.
        The progression then restarts at sample 0. Like every config key it holds for all integrators of the process."""
        config_set(light_tree=1 if enable else 0)

    @property
    def ctx(self):
        return host_lib().grt_pathtracer_context(self.handle)

    @property
    def sample_index(self):
        return host_lib().grt_pathtracer_sample_index(self.handle)

    @property
    def pitch(self):
        return host_lib().grt_pathtracer_screen_pitch(self.handle)

    @property
    def device_blas_build_ms(self):
        """config device_blas = 1: what the BLAS build took on the device (0 when the host built the trees)."""
        return float(host_lib().grt_pathtracer_device_blas_build_ms(self.handle))

    @property
    def static_geometry_members(self):
        """config merge_static = 1: instances flattened into the one static bottom-level tree (0: none, or dissolved)."""
        return int(host_lib().grt_pathtracer_static_geometry_members(self.handle))

    @property
    def static_geometry_whole_scene(self):
        """Every instance is in the flattened tree: there is no TLAS, rays start inside the tree (rt_set_static_geometry)."""
        return bool(host_lib().grt_pathtracer_static_geometry_whole_scene(self.handle))

    @property
    def skip_behind_hit(self):
        """Closest-hit rays drop stacked groups of children behind the hit they hold (config skip_behind_hit AND a one-tree scene: rt_set_skip_behind_hit)."""
        return bool(host_lib().grt_pathtracer_skip_behind_hit(self.handle))

    @property
    def static_geometry_top_levels(self):
        """(root node of the flattened tree, nodes from it that make up its top three levels): the tree is numbered breadth-first, what
        every ray walks comes first."""
        return int(host_lib().grt_pathtracer_static_geometry_root(self.handle)), int(host_lib().grt_pathtracer_static_geometry_top_nodes(self.handle))

    def set_flatten_asynchronously(self, enable):
        """True (default): when a flattened instance starts to move the new tree is built on a worker thread while frames are rendered
        in the reference's layout; False: rebuilt inside update() (a stall of the build time)."""
        host_lib().grt_pathtracer_set_flatten_asynchronously(self.handle, 1 if enable else 0)

    def set_reseat_asynchronously(self, enable):
        """True (default): the flattened tree is seated again (config static_reseat_distance; device-built trees: for the first time) on a worker thread and its
        nodes are swapped in between two frames; False: inside update()."""
        host_lib().grt_pathtracer_set_reseat_asynchronously(self.handle, 1 if enable else 0)

    @property
    def reseats_completed(self):
        return int(host_lib().grt_pathtracer_reseats_completed(self.handle))

    @property
    def reseat_pending(self):
        return bool(host_lib().grt_pathtracer_reseat_pending(self.handle))

    @property
    def last_reseat_seconds(self):
        return float(host_lib().grt_pathtracer_last_reseat_seconds(self.handle))

    @property
    def reflattens_completed(self):
        return int(host_lib().grt_pathtracer_reflattens_completed(self.handle))

    @property
    def reflatten_in_progress(self):
        """0: none; 1: a worker thread is building the tree; 2: it is done, the next update() installs it."""
        return int(host_lib().grt_pathtracer_reflatten_in_progress(self.handle))

    @property
    def static_geometry_bytes(self):
        """Device bytes the flattened tree adds: its triangle copies (shading + traversal records + names) and its nodes."""
        return int(host_lib().grt_pathtracer_static_geometry_bytes(self.handle))

    @property
    def static_geometry_build_seconds(self):
        return float(host_lib().grt_pathtracer_static_geometry_build_seconds(self.handle))

    @property
    def lights_total_weight(self):
        return host_lib().grt_pathtracer_lights_total_weight(self.handle)

    @property
    def delta_light_share(self):
        """The share that goes with the staged delta-light records (array("delta_light_records")): cpu_config.delta_light_share, or by power."""
        return host_lib().grt_pathtracer_delta_light_share(self.handle)

    def update(self, delta=0.0):
        _host_check(host_lib().grt_pathtracer_update(self.handle, float(delta)))

    def render(self):
        _host_check(host_lib().grt_pathtracer_render(self.handle))

    def render_samples(self, count):
        """`count` samples per pixel as one wavefront; same image as `count` x (update(); render())."""
        _host_check(host_lib().grt_pathtracer_render_samples(self.handle, int(count)))

    def set_pixel_query(self, x, y):
        """Integrator::set_pixel_query (window coordinates, y top-down): which mesh / triangle is under
        this pixel? Armed for the next render(); the update() after it fetches the answer."""
        host_lib().grt_pathtracer_set_pixel_query(self.handle, int(x), int(y))

    @property
    def pixel_query(self):
        """(pixel_index, scene mesh index, triangle id, status) -- status 0 inactive, 1 pending, 2 output ready."""
        v = [c_int() for _ in range(4)]
        host_lib().grt_pathtracer_get_pixel_query(self.handle, *[byref(i) for i in v])
        return tuple(i.value for i in v)

    def invalidate(self, what):
        host_lib().grt_pathtracer_invalidate(self.handle, what.encode())

    def aov_enable(self, aov, enable=True):
        host_lib().grt_pathtracer_aov_enable(self.handle, aov, 1 if enable else 0)

    def set_pixel_range(self, offset, count):
        _host_check(host_lib().grt_pathtracer_set_pixel_range(self.handle, offset, count))

    def array(self, name):
        n = c_size_t()
        ptr = host_lib().grt_pathtracer_array(self.handle, name.encode(), byref(n))
        return _view(ptr, n.value, _ARRAY_DTYPES[name])

    def view_projection(self):
        """(view_projection, view_projection_prev) as uploaded for SVGF, 16 row-major floats each."""
        m = self.array("svgf_matrices")
        return m[:16].tolist(), m[16:].tolist()

    def camera(self):
        cam = Camera()
        raw = self.array("camera")
        ctypes.memmove(byref(cam), raw.ctypes.data, ctypes.sizeof(cam))
        return cam

    def device_config(self):
        cfg = GPUConfig()
        host_lib().grt_pathtracer_device_config(self.handle, byref(cfg))
        return cfg

    def sky(self):
        w, h, s = c_int(), c_int(), c_float()
        host_lib().grt_pathtracer_sky_size(self.handle, byref(w), byref(h), byref(s))
        return self.array("sky"), w.value, h.value, s.value

    def textures(self):
        out = []
        i = 0
        while True:
            texels, w, h, levels = c_void_p(), c_int(), c_int(), c_int()
            if host_lib().grt_pathtracer_texture(self.handle, i, byref(texels), byref(w), byref(h), byref(levels)) != 0:
                break
            count = 0
            for l in range(levels.value):
                count += max(w.value >> l, 1) * max(h.value >> l, 1)
            out.append((_view(texels.value, count * 4, np.uint8), w.value, h.value, levels.value))
            i += 1
        return out

    def texture_lod_size(self, index):
        """(lod_width, lod_height) of texture `index`: what enters its LOD bias; (0, 0) = its own size."""
        w, h = c_int(), c_int()
        lib = host_lib()
        lib.grt_pathtracer_texture_lod_size.argtypes = [c_void_p, c_int, POINTER(c_int), POINTER(c_int)]
        if lib.grt_pathtracer_texture_lod_size(self.handle, index, byref(w), byref(h)) != 0:
            raise IndexError(index)
        return w.value, h.value

    def read_framebuffer(self):
        image = np.zeros((self.height, self.pitch, 4), np.float32)
        _host_check(host_lib().grt_pathtracer_read_framebuffer(self.handle, image.ctypes.data))
        return image

    def save_image(self, filename):
        """Screenshot like the reference's `-o`: .ppm (ACES + gamma, 8 bit) or .exr (raw radiance, half),
        plus albedo.exr / normal.exr / position.exr next to it for the enabled AOVs (Main.cpp:199-246)."""
        _host_check(host_lib().grt_pathtracer_save_image(self.handle, str(filename).encode()))

    def read_aov(self, aov, accumulated=True):
        image = np.zeros((self.height, self.pitch, 4), np.float32)
        _host_check(host_lib().grt_pathtracer_read_aov(self.handle, aov, 1 if accumulated else 0, image.ctypes.data))
        return image

    def counters(self):
        c = Counters()
        _host_check(host_lib().grt_pathtracer_counters(self.handle, byref(c)))
        return c

    # ---- denoised stills
    def set_denoise(self, enable=True):
        """config denoise: from the next update() on (which restarts the progression when it switches them on) the device keeps the noise estimate and the
        ALBEDO, NORMAL and POSITION AOVs that denoise() filters by."""
        config_set(denoise=1 if enable else 0)

    @staticmethod
    def _denoise_params(params):
        if not params:
            return None   # the configuration's (config denoise_iterations, denoise_sigma_l / _n / _z)
        unknown = set(params) - set(DENOISE_DEFAULTS)
        if unknown:
            raise TypeError("unknown denoise parameter(s): %s" % ", ".join(sorted(unknown)))
        merged = {k: config_get("denoise_" + k) for k in ("iterations", "sigma_l", "sigma_n", "sigma_z")}
        merged.update(depth_floor=DENOISE_DEFAULTS["depth_floor"], albedo_floor=DENOISE_DEFAULTS["albedo_floor"])
        merged.update(params)
        return np.array([merged[k] for k in ("iterations", "sigma_l", "sigma_n", "sigma_z", "depth_floor", "albedo_floor")], np.float64)

    def denoise(self, **params):
        """Pathtracer::denoise(): the accumulated frame through the variance-guided a-trous filter. Returns (image, variance): (height, width, 3) float32 and
        the (height, width) plane of the filtered variance (0: sky, -1: a pixel that was not valid and carries the final image's colour). params: iterations,
        sigma_l, sigma_n, sigma_z, depth_floor, albedo_floor; what is not given is the configuration's. Completes the work in flight."""
        values = self._denoise_params(params)
        image = np.zeros((self.height, self.pitch, 4), np.float32)
        _host_check(host_lib().grt_pathtracer_denoise(self.handle, values.ctypes.data if values is not None else None, image.ctypes.data))
        return image[:, :self.width, :3].copy(), image[:, :self.width, 3].copy()

    def save_denoised_image(self, filename, **params):
        """save_image's exporters (.ppm, .exr) on the denoised image."""
        values = self._denoise_params(params)
        _host_check(host_lib().grt_pathtracer_save_denoised_image(self.handle, str(filename).encode(), values.ctypes.data if values is not None else None))

    # ---- firefly filter
    def set_firefly_filter(self, enable=True, auto_start=None, start_shift=None, pilot_samples=None, **params):
        """config firefly_filter (and firefly_tiers / firefly_start / firefly_support from tiers, start, support): from the next update() on (which restarts the
        progression when it switches them on) the device keeps the noise estimate and the tier cascade that resolve_fireflies() reweights.
        auto_start (config firefly_auto_start, with firefly_start_shift and firefly_pilot_samples from start_shift and pilot_samples): after the
        pilot samples the start is taken from the frame's own exposure and the progression starts over; firefly_start then says what is in force. None leaves a key alone."""
        unknown = set(params) - set(FIREFLY_DEFAULTS)
        if unknown:
            raise TypeError("unknown firefly parameter(s): %s" % ", ".join(sorted(unknown)))
        automatic = {"firefly_auto_start": None if auto_start is None else (1 if auto_start else 0), "firefly_start_shift": start_shift, "firefly_pilot_samples": pilot_samples}
        config_set(firefly_filter=1 if enable else 0, **{"firefly_" + k: v for k, v in params.items()}, **{k: v for k, v in automatic.items() if v is not None})

    def _firefly_start_state(self):
        lib = host_lib()
        lib.grt_pathtracer_firefly_start.argtypes = [c_void_p, c_void_p]
        out = np.zeros(3, np.float64)
        _host_check(lib.grt_pathtracer_firefly_start(self.handle, out.ctypes.data))
        return out

    @property
    def firefly_start(self):
        """Pathtracer::firefly_start(): the start of the cascade in force -- config firefly_start, or what auto_start measured after the pilot."""
        return float(self._firefly_start_state()[0])

    @property
    def firefly_start_measured(self):
        """True once the pilot of the current configuration has been rendered and measured (auto_start)."""
        return bool(self._firefly_start_state()[1])

    @property
    def firefly_pilot_samples_discarded(self):
        """The samples rendered and dropped by the restarts auto_start has made so far."""
        return int(self._firefly_start_state()[2])

    def resolve_fireflies(self, support=None):
        """Pathtracer::resolve_fireflies(): the tier cascade, every tier scaled by how well its neighbourhood supports it. Returns (image, held_back): (height, width, 3)
        float32 and the (height, width) plane of the luminance that was held back (-1: a pixel that was not valid and carries the final image's colour).
        support: kappa; None for the configuration's. Completes the work in flight."""
        image = np.zeros((self.height, self.pitch, 4), np.float32)
        _host_check(host_lib().grt_pathtracer_resolve_fireflies(self.handle, 0.0 if support is None else float(support), image.ctypes.data))
        return image[:, :self.width, :3].copy(), image[:, :self.width, 3].copy()

    def save_resolved_image(self, filename, support=None):
        """save_image's exporters (.ppm, .exr) on the resolved image."""
        _host_check(host_lib().grt_pathtracer_save_resolved_image(self.handle, str(filename).encode(), 0.0 if support is None else float(support)))

    # ---- noise estimate
    def set_noise_estimate(self, enable=True, robust=False, held_fraction=0.25):
        """The device keeps Welford second moments beside the radiance mean from the next update() on (which restarts the
        progression when it switches them on). Also on while config noise_target > 0.
        robust (config noise_robust and noise_held_fraction; needs the firefly filter, else one warning and the plain estimate): noise_estimate(),
        noise_map(), select_adaptive() and render_until() leave out the pixels of which the resolve holds back more than held_fraction of their brightness."""
        config_set(noise_robust=1 if robust else 0, noise_held_fraction=held_fraction)
        lib = host_lib()
        lib.grt_pathtracer_set_noise_estimate.argtypes = [c_void_p, c_int]
        lib.grt_pathtracer_set_noise_estimate.restype = None
        lib.grt_pathtracer_set_noise_estimate(self.handle, 1 if enable else 0)

    def _noise(self, entry, want_map):
        lib = host_lib()
        fn = getattr(lib, entry)
        fn.argtypes = [c_void_p] + [c_void_p] * 4 + [c_size_t] + [c_void_p] * 3
        cells_x, cells_y = _noise_cells(self.width, self.height)
        n = cells_x * cells_y
        xy = np.zeros(2, np.int32)
        sums, counts, nonfinite = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        mean_figure, pixels = np.zeros(2, np.float64), np.zeros(2, np.int64)
        pixel_map = np.zeros((self.height, self.pitch), np.float32) if want_map else None
        _host_check(fn(self.handle, xy.ctypes.data, sums.ctypes.data, counts.ctypes.data, nonfinite.ctypes.data, n, mean_figure.ctypes.data, pixels.ctypes.data,
                       pixel_map.ctypes.data if want_map else None))
        shape = (int(xy[1]), int(xy[0]))
        result = {"cells_x": int(xy[0]), "cells_y": int(xy[1]), "cell_sums": sums.reshape(shape), "cell_counts": counts.reshape(shape), "cell_nonfinite": nonfinite.reshape(shape),
                  "mean": float(mean_figure[0]), "figure": float(mean_figure[1]), "pixels": int(pixels[0]), "nonfinite_pixels": int(pixels[1]), "robust": False, "held_pixels": 0}
        if entry == "grt_pathtracer_noise":   # what the call above found beyond its fixed outputs (the firefly-robust estimate)
            lib.grt_pathtracer_noise_held.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
            held, cell_held = np.zeros(2, np.int64), np.zeros(n, np.int32)
            _host_check(lib.grt_pathtracer_noise_held(self.handle, held.ctypes.data, cell_held.ctypes.data, n))
            result.update(robust=bool(held[0]), held_pixels=int(held[1]), cell_held=cell_held.reshape(shape))
        return result, pixel_map

    def noise_estimate(self):
        """Pathtracer::noise(): the cells (16 x 16 pixels: sums of the per-pixel relative standard error, counts, non-finite counts), the mean over
        the frame and the figure -- the noise_quantile quantile of the cell means. Completes the work in flight."""
        return self._noise("grt_pathtracer_noise", False)[0]

    def noise_map(self):
        """The per-pixel relative standard error, (height, pitch) float32: -1 where the pixel takes no part, -2 where it is not finite, -3 where the robust estimate
        holds it."""
        return self._noise("grt_pathtracer_noise", True)[1]

    def select_adaptive(self, threshold):
        """Pathtracer::select_adaptive: selects the cells whose mean error is above `threshold` (config noise_floor, adaptive_dilate) and lets the
        next render calls cover their pixels only; an empty selection switches back to the whole frame. Returns {"cells", "hot_cells", "active_cells", "list_pixels"}."""
        lib = host_lib()
        lib.grt_pathtracer_select_adaptive.argtypes = [c_void_p, ctypes.c_double, c_void_p]
        out = np.zeros(4, np.int64)
        _host_check(lib.grt_pathtracer_select_adaptive(self.handle, float(threshold), out.ctypes.data))
        return {"cells": int(out[0]), "hot_cells": int(out[1]), "active_cells": int(out[2]), "list_pixels": int(out[3])}

    def adaptive_off(self):
        """Render calls cover the whole frame again."""
        lib = host_lib()
        lib.grt_pathtracer_adaptive_off.argtypes = [c_void_p]
        _host_check(lib.grt_pathtracer_adaptive_off(self.handle))

    def sample_counts(self):
        """Pathtracer::sample_counts(): (w per pixel as (height, pitch) float32 -- the number of samples each pixel's mean stands for, one
        below the samples rendered for it (sample 1 overwrites sample 0) --, the mean of w over the frame)."""
        lib = host_lib()
        lib.grt_pathtracer_sample_counts.argtypes = [c_void_p, c_void_p, POINTER(ctypes.c_double)]
        counts = np.zeros((self.height, self.pitch), np.float32)
        mean = ctypes.c_double()
        _host_check(lib.grt_pathtracer_sample_counts(self.handle, counts.ctypes.data, byref(mean)))
        return counts, mean.value

    def sample_count_map(self):
        return self.sample_counts()[0]

    def render_until(self, noise_target, max_samples, check_every=16, adaptive=False):
        """Renders until the noise figure is <= noise_target, never fewer than config noise_min_samples samples and never more than max_samples;
        the figure is asked for every `check_every` samples only (the question drains the wavefront). Returns {"samples", "figure", "mean", "capped"}.
        adaptive=True: at every check that goes on, the cells whose mean error is above noise_target are selected and the next passes render their
        pixels only; the stop criterion stays the same. The result then also has "mean_samples" (the samples rendered per pixel on average: the mean of w, plus
        sample 0) and "active_share" (per check, active cells / cells)."""
        if not (noise_target >= 0.0) or max_samples < 2 or check_every < 1:
            raise ValueError("render_until: noise_target >= 0, max_samples >= 2 and check_every >= 1 are required")
        if adaptive and config_get("enable_svgf"):
            raise ValueError("render_until: adaptive sampling needs plain path tracing (no SVGF)")
        if config_get("enable_svgf"):   # SVGF frames keep no second moments (their accumulators are the filter's images)
            import warnings
            warnings.warn("render_until: SVGF frames keep no noise estimate; rendering to max_samples")
            while True:
                self.update()
                self.render()
                if self.sample_index + 1 >= max_samples:
                    return {"samples": self.sample_index + 1, "figure": None, "mean": None, "capped": True}
        if adaptive and not noise_target > 0.0:
            raise ValueError("render_until: adaptive sampling needs noise_target > 0")
        self.set_noise_estimate(True, robust=bool(config_get("noise_robust")), held_fraction=config_get("noise_held_fraction"))   # (whatever is set stays)
        min_samples = int(config_get("noise_min_samples"))
        if not adaptive:
            return self._render_until(noise_target, max_samples, check_every, min_samples, None)
        shares = []
        try:
            result = self._render_until(noise_target, max_samples, check_every, min_samples, shares)
            result["mean_samples"] = self.sample_counts()[1] + 1.0
            result["active_share"] = shares
            return result
        finally:
            self.adaptive_off()

    def _render_until(self, noise_target, max_samples, check_every, min_samples, shares):
        estimate = None
        while True:
            self.update()
            first = self.sample_index
            if first + 1 > max_samples:
                raise ValueError("render_until: %d samples are accumulated already, max_samples is %d" % (first, max_samples))
            n = min(check_every - first % check_every, max_samples - first, 16)
            if first == 0 or n == 1:
                self.render()
            else:
                self.render_samples(n)
            samples = self.sample_index + 1
            estimate = None
            if samples >= min_samples and (samples % check_every == 0 or samples >= max_samples):
                estimate = self.noise_estimate()
                if estimate["figure"] <= noise_target:
                    break
                if shares is not None and samples < max_samples:
                    chosen = self.select_adaptive(noise_target)
                    shares.append(chosen["active_cells"] / chosen["cells"])
            if samples >= max_samples:
                break
        if estimate is None:
            estimate = self.noise_estimate()
        return {"samples": self.sample_index + 1, "figure": estimate["figure"], "mean": estimate["mean"], "capped": not estimate["figure"] <= noise_target}


# ---- kernel-level entry points of the C ABI -----------------------------------------------------------

class FrameSplit:
    """host/FrameSplit.h: one frame over several GPUs from one process -- row tiles dealt round-robin to one Pathtracer per
    entry of `devices` (an ordinal may repeat: contexts sharing a GPU exchange by peer copies), ONE grouped all-gather over
    RCCL per render(); no torch.distributed. rank(r) is that rank's Pathtracer (owned by the split)."""

    def __init__(self, scene, width, height, devices):
        lib = host_lib()
        self.scene, self.width, self.height, self.world = scene, width, height, len(devices)
        ordinals = (c_int * len(devices))(*devices)
        self.handle = lib.grt_frame_split_create(scene.handle, width, height, ordinals, len(devices))
        if not self.handle:
            raise RuntimeError("FrameSplit creation failed: %s" % lib.grt_last_error().decode(errors="replace"))

    def close(self):
        if self.handle:
            host_lib().grt_frame_split_free(self.handle)
            self.handle = None

    def rank(self, r):
        view = Pathtracer.__new__(Pathtracer)
        view.scene, view.width, view.height = self.scene, self.width, self.height
        view.handle = host_lib().grt_frame_split_rank(self.handle, r)
        view.close = lambda: None      # owned by the split
        return view

    @property
    def submitting_threads(self):
        """Host threads that enqueue the ranks' launches: one per rank (0 for a single rank: the caller's thread)."""
        return int(host_lib().grt_frame_split_submitting_threads(self.handle))

    def update(self, delta=0.0):
        _host_check(host_lib().grt_frame_split_update(self.handle, float(delta)))

    def render(self):
        _host_check(host_lib().grt_frame_split_render(self.handle))

    def render_samples(self, count):
        _host_check(host_lib().grt_frame_split_render_samples(self.handle, int(count)))

    @property
    def pitch(self):
        return self.rank(0).pitch

    def noise_estimate(self):
        """FrameSplit::noise(): the ranks' cell sums and counts added, then the same summary as Pathtracer.noise_estimate()."""
        return Pathtracer._noise(self, "grt_frame_split_noise", False)[0]


class AO(Pathtracer):
    """reference: Src/Renderer/Integrators/AO.h -- the ambient-occlusion integrator. Shares the
    update()/render()/read_* protocol and the staging arrays with Pathtracer; `radius` is AO::ao_radius."""
    _create = "grt_ao_create"

    def __init__(self, scene, width, height, device=0, radius=1.0):
        super().__init__(scene, width, height, device)
        self.radius = radius

    @property
    def radius(self):
        return self._radius

    @radius.setter
    def radius(self, value):
        _host_check(host_lib().grt_ao_set_radius(self.handle, float(value)))
        self._radius = float(value)


def _dev_check(ctx, status):
    if status != 0:
        raise RuntimeError("device layer: " + device_lib().rt_last_error(ctx).decode())


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _soa_pointers(origin, direction):
    """The six component pointers {ox, oy, oz, dx, dy, dz} of two (3, N) SoA arrays."""
    return [a[k].ctypes.data for a in (origin, direction) for k in range(3)]


def _noise_cells(width, height):
    """(cells_x, cells_y): the 16 x 16 pixel cells of the noise estimate that cover a frame."""
    return (width + 15) // 16, (height + 15) // 16


def _trace_statistics(raw10):
    """The kernels' ten statistics words as {'closest': {...}, 'shadow': {...}} with nodes / triangles / instances_transformed / instances_identity / rays."""
    names = ("nodes", "triangles", "instances_transformed", "instances_identity", "rays")
    return {kind: {name: int(raw10[5 * j + i]) for i, name in enumerate(names)} for j, kind in enumerate(("closest", "shadow"))}


class DeviceRefusal(RuntimeError):
    """A device-layer call that returned an error status (.status: the RT_ERROR_* value)."""

    def __init__(self, ctx, status):
        super().__init__("device layer (%d): %s" % (status, device_lib().rt_last_error(ctx).decode()))
        self.status = status


def set_noise_estimate(ctx, enable):
    status = device_lib().rt_set_noise_estimate(ctx, 1 if enable else 0)
    if status:
        raise DeviceRefusal(ctx, status)


def get_noise_estimate(ctx):
    return bool(device_lib().rt_get_noise_estimate(ctx))


def read_noise_moments(ctx, height, pitch):
    """rt_read_noise_moments: (height, pitch, 4) float32 {M2_r, M2_g, M2_b, w}."""
    image = np.zeros((height, pitch, 4), np.float32)
    status = device_lib().rt_read_noise_moments(ctx, image.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return image


def _estimate_noise(ctx, height, width, pitch, floor, held_fraction, images, want_map, cell_capacity):
    """The one body of estimate_noise (held_fraction None) and estimate_noise_robust. images: the caller's (height, pitch, 4) float32 images -- mean, moments and,
    robust, resolved -- or () for the context's frame."""
    robust = held_fraction is not None
    cells_x, cells_y = _noise_cells(width, height)
    n = cells_x * cells_y
    cells = {"cell_sums": np.zeros(n, np.float64), "cell_counts": np.zeros(n, np.int32), "cell_nonfinite": np.zeros(n, np.int32)}
    if robust:
        cells["cell_held"] = np.zeros(n, np.int32)
    pixel_map = np.zeros((height, pitch), np.float32) if want_map else None
    out, held_pixels = NoiseEstimateRecord(), ctypes.c_int64()
    images = [_f32(image) for image in images]
    assert all(image.shape == (height, pitch, 4) for image in images)
    # (the robust entry points take held_fraction after floor, cell_held after cell_nonfinite and the held count last)
    args = [image.ctypes.data for image in images] + [c_float(floor)] + ([c_float(held_fraction)] if robust else []) + [byref(out)] + [a.ctypes.data for a in cells.values()]
    args += [n if cell_capacity is None else cell_capacity, pixel_map.ctypes.data if want_map else None] + ([byref(held_pixels)] if robust else [])
    entry = "rt_estimate_noise" + ("_robust" if robust else "") + ("_images" if images else "")
    status = getattr(device_lib(), entry)(ctx, *args)
    if status:
        raise DeviceRefusal(ctx, status)
    result = {"cells_x": out.cells_x, "cells_y": out.cells_y, "pixels": out.pixels, "nonfinite_pixels": out.nonfinite_pixels, "mean": out.mean, "pixel_map": pixel_map}
    result.update((name, a.reshape(cells_y, cells_x)) for name, a in cells.items())
    if robust:
        result["held_pixels"] = held_pixels.value
    return result


def estimate_noise(ctx, height, width, pitch, floor=1e-2, mean=None, moments=None, want_map=True, cell_capacity=None):
    """rt_estimate_noise on the context's accumulator and moments, or -- mean and moments given, (height, pitch, 4) float32 -- rt_estimate_noise_images on
    those. Returns a dict: cells_x, cells_y, pixels, nonfinite_pixels, mean, cell_sums / cell_counts / cell_nonfinite (cells_y, cells_x), pixel_map (height, pitch)."""
    return _estimate_noise(ctx, height, width, pitch, floor, None, () if mean is None else (mean, moments), want_map, cell_capacity)


def denoise(ctx, **params):
    """rt_denoise on the context's frame; the image comes back through read_denoised."""
    record = denoise_params(**params)
    status = device_lib().rt_denoise(ctx, byref(record))
    if status:
        raise DeviceRefusal(ctx, status)


def read_denoised(ctx, height, pitch):
    """rt_read_denoised: (height, pitch, 4) float32 {r, g, b, variance}."""
    image = np.zeros((height, pitch, 4), np.float32)
    status = device_lib().rt_read_denoised(ctx, image.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return image


def denoise_timed(ctx, tiled=True, **params):
    """rt_denoise_timed: rt_denoise with an event pair around every kernel; returns the kernels' times in ms (prepare first)."""
    record = denoise_params(**params)
    ms, count = np.zeros(8, np.float32), c_size_t(0)
    status = device_lib().rt_denoise_timed(ctx, byref(record), 1 if tiled else 0, ms.ctypes.data, ms.size, byref(count))
    if status:
        raise DeviceRefusal(ctx, status)
    return ms[:count.value].copy()


def denoise_images(ctx, colour, moments, albedo, normal, position, fallback, eye, width=None, tiled=True, sentinel=None, **params):
    """rt_denoise_images: the denoiser's launchers on explicit (height, pitch, 4) float32 images; width defaults to pitch. Returns (height, pitch, 4) float32
    {r, g, b, variance}; what the kernels do not write (the padding columns) holds `sentinel` (a float32 bit pattern; default 0x7fc0dead)."""
    images = [_f32(a) for a in (colour, moments, albedo, normal, position, fallback)]
    height, pitch = images[0].shape[:2]
    assert all(a.shape == (height, pitch, 4) for a in images)
    width = pitch if width is None else width
    record = denoise_params(**params)
    out = np.full((height, pitch, 4), 0x7fc0dead if sentinel is None else sentinel, np.uint32).view(np.float32)
    eye = _f32(eye)
    assert eye.shape == (3,)
    status = device_lib().rt_denoise_images(ctx, width, height, pitch, *[a.ctypes.data for a in images], eye.ctypes.data, byref(record), 1 if tiled else 0, out.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return out


# ---- firefly filter
def set_firefly_cascade(ctx, enable=True, **params):
    """rt_set_firefly_cascade: tiers, start, support (FIREFLY_DEFAULTS); enable=False switches it off and frees the tiers."""
    status = device_lib().rt_set_firefly_cascade(ctx, byref(firefly_params(**params)) if enable else None)
    if status:
        raise DeviceRefusal(ctx, status)


def get_firefly_cascade(ctx):
    """None while the cascade is off, else {"tiers", "start", "support"}."""
    record = FireflyParams()
    if not device_lib().rt_get_firefly_cascade(ctx, byref(record)):
        return None
    return {"tiers": record.tiers, "start": record.start, "support": record.support}


def read_firefly_cascade(ctx, height, pitch):
    """rt_read_firefly_cascade: (tiers, height, pitch, 4) float32 (sum w r, sum w g, sum w b, sum w)."""
    state = get_firefly_cascade(ctx)
    tiers = np.zeros((state["tiers"] if state else 1, height, pitch, 4), np.float32)
    status = device_lib().rt_read_firefly_cascade(ctx, tiers.ctypes.data, tiers.size)
    if status:
        raise DeviceRefusal(ctx, status)
    return tiers


def resolve_fireflies(ctx, support=None):
    """rt_resolve_fireflies on the context's frame; the image comes back through read_resolved. support: None for the cascade's own."""
    if support is None:
        state = get_firefly_cascade(ctx)
        support = state["support"] if state else FIREFLY_DEFAULTS["support"]
    status = device_lib().rt_resolve_fireflies(ctx, c_float(support))
    if status:
        raise DeviceRefusal(ctx, status)


def resolve_fireflies_timed(ctx, support=FIREFLY_DEFAULTS["support"], tiled=True):
    """rt_resolve_fireflies_timed: the resolve kernel's time in ms."""
    ms = c_float(0.0)
    status = device_lib().rt_resolve_fireflies_timed(ctx, c_float(support), 1 if tiled else 0, byref(ms))
    if status:
        raise DeviceRefusal(ctx, status)
    return ms.value


def read_resolved(ctx, height, pitch):
    """rt_read_resolved: (height, pitch, 4) float32 {r, g, b, held-back luminance}."""
    image = np.zeros((height, pitch, 4), np.float32)
    status = device_lib().rt_read_resolved(ctx, image.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return image


def set_denoise_source(ctx, source):
    """rt_set_denoise_source: "mean" or "resolved"."""
    status = device_lib().rt_set_denoise_source(ctx, {"mean": 0, "resolved": 1}.get(source, source))
    if status:
        raise DeviceRefusal(ctx, status)


def resolve_fireflies_images(ctx, mean, moments, tiers, fallback, width=None, tiled=True, sentinel=None, tier_count=None, **params):
    """rt_resolve_fireflies_images: the resolve kernel on explicit images: mean, moments, fallback (height, pitch, 4) float32, tiers (K, height, pitch, 4); width
    defaults to pitch; params: start, support (the number of tiers is the array's, unless tier_count says otherwise). Returns (height, pitch, 4) float32 {r, g, b, held-back luminance}; what the kernel
    does not write (the padding columns) holds `sentinel` (a float32 bit pattern; default 0x7fc0dead)."""
    mean, moments, tiers, fallback = (_f32(a) for a in (mean, moments, tiers, fallback))
    height, pitch = mean.shape[:2]
    assert moments.shape == fallback.shape == mean.shape == (height, pitch, 4) and tiers.ndim == 4 and tiers.shape[1:] == mean.shape
    record = firefly_params(tiers=tiers.shape[0] if tier_count is None else tier_count, **params)
    assert record.tiers <= tiers.shape[0] or not 2 <= record.tiers <= 8
    out = np.full((height, pitch, 4), 0x7fc0dead if sentinel is None else sentinel, np.uint32).view(np.float32)
    status = device_lib().rt_resolve_fireflies_images(ctx, pitch if width is None else width, height, pitch, mean.ctypes.data, moments.ctypes.data, tiers.ctypes.data, fallback.ctypes.data,
                                                      byref(record), 1 if tiled else 0, out.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return out


# ---- the frame's exposure and the firefly-robust noise estimate
def measure_exposure(ctx):
    """rt_measure_exposure on the context's RADIANCE mean and moments. Returns a dict: pixels, dark_pixels, nonfinite_pixels, histogram ((256,) uint64: the pixels
    whose luminance has that biased float32 exponent)."""
    return measure_exposure_images(ctx, None, None)


def measure_exposure_images(ctx, mean, moments, width=None):
    """rt_measure_exposure_images: the exposure histogram of explicit (height, pitch, 4) float32 images; width defaults to pitch. As measure_exposure."""
    histogram, out = np.zeros(256, np.uint64), ExposureRecord()
    if mean is None:
        status = device_lib().rt_measure_exposure(ctx, byref(out), histogram.ctypes.data)
    else:
        mean, moments = _f32(mean), _f32(moments)
        height, pitch = mean.shape[:2]
        assert mean.shape == moments.shape == (height, pitch, 4)
        status = device_lib().rt_measure_exposure_images(ctx, pitch if width is None else width, height, pitch, mean.ctypes.data, moments.ctypes.data, byref(out), histogram.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return {"pixels": out.pixels, "dark_pixels": out.dark_pixels, "nonfinite_pixels": out.nonfinite_pixels, "histogram": histogram}


def exposure_start(histogram, shift=0):
    """grt_exposure_start of the host library: (start, median exponent + shift, clamped to -96 .. 96) -- start = 2 ** that --, or None for an empty histogram."""
    lib = host_lib()
    lib.grt_exposure_start.argtypes = [c_void_p, c_int, POINTER(c_float), POINTER(c_int)]
    histogram = np.ascontiguousarray(histogram, np.uint64).ravel()
    assert histogram.size == 256
    start, exponent = c_float(), c_int()
    if lib.grt_exposure_start(histogram.ctypes.data, int(shift), byref(start), byref(exponent)):
        return None
    return start.value, exponent.value


def estimate_noise_robust(ctx, height, width, pitch, floor=1e-2, held_fraction=0.25, mean=None, moments=None, resolved=None, want_map=True, cell_capacity=None):
    """rt_estimate_noise_robust on the context's frame (after a resolve of its own), or -- mean, moments and resolved given, (height, pitch, 4) float32 --
    rt_estimate_noise_robust_images on those. The dict of estimate_noise plus cell_held (cells_y, cells_x) and held_pixels; a held pixel is -3 in pixel_map."""
    return _estimate_noise(ctx, height, width, pitch, floor, held_fraction, () if mean is None else (mean, moments, resolved), want_map, cell_capacity)


def estimate_noise_robust_images(ctx, height, width, pitch, mean, moments, resolved, **given):
    """rt_estimate_noise_robust_images: estimate_noise_robust on the caller's images."""
    return estimate_noise_robust(ctx, height, width, pitch, mean=mean, moments=moments, resolved=resolved, **given)


def set_noise_robust(ctx, held_fraction):
    """rt_set_noise_robust: held_fraction in (0, 1) makes rt_select_active_cells select from the robust cells; 0 (or None, False) switches that off."""
    status = device_lib().rt_set_noise_robust(ctx, c_float(held_fraction or 0.0))
    if status:
        raise DeviceRefusal(ctx, status)


def get_noise_robust(ctx):
    return float(device_lib().rt_get_noise_robust(ctx))


def select_pixels_robust_images(ctx, height, width, pitch, mean, moments, resolved, threshold, floor=1e-2, held_fraction=0.25, dilate=1, sentinel=0xffffffff):
    """rt_select_pixels_robust_images: select_pixels_images from the robust cells of the caller's images; the dict gains cell_held (cells_y, cells_x)."""
    return _select_pixels_images(ctx, height, width, pitch, (mean, moments, resolved), threshold, floor, held_fraction, dilate, sentinel)


def _accumulate_staging(frames, images, first_sample, sample_count, merged):
    """What the three accumulate probes are handed: float32 copies of the frames and of the (height, pitch, 4) images (None stays None), one first sample and one
    sample count per submission (merged=False: the one batch holds all frames unless sample_count says otherwise) and a zeroed final image."""
    frames, images = _f32(frames).copy(), [None if image is None else _f32(image).copy() for image in images]
    if merged:
        first, count = np.asarray(first_sample, np.int32).reshape(-1).copy(), np.asarray(sample_count, np.int32).reshape(-1).copy()
    else:
        first, count = np.array([first_sample], np.int32), np.array([frames.shape[0] if sample_count is None else sample_count], np.int32)
    assert frames.ndim == 4 and frames.shape[0] == int(count.sum()) and len(first) == len(count) and all(image is None or image.shape == frames.shape[1:] for image in images)
    return frames, images, first, count, np.zeros(frames.shape[1:], np.float32)


def accumulate_cascade_frames(ctx, frames, accumulator, moments, tiers, first_sample, sample_count=None, merged=False, pixels=None, sentinel=0x7fc0dead, **params):
    """rt_accumulate_cascade_frames: accumulate_frames / accumulate_list_frames (pixels: the list, merged only) with the cascade; tiers: (K, height, pitch, 4) in
    and out; params: start, support. Returns (frames, accumulator, moments, tiers, final_image) after the ONE launch."""
    frames, (accumulator, moments), first, count, final = _accumulate_staging(frames, (accumulator, moments), first_sample, sample_count, merged)
    tiers = _f32(tiers).copy()
    assert tiers.shape[1:] == accumulator.shape
    record = firefly_params(tiers=tiers.shape[0], **params)
    pixels = None if pixels is None else np.ascontiguousarray(pixels, np.uint32)
    status = device_lib().rt_accumulate_cascade_frames(ctx, 1 if merged else 0, first.ctypes.data, count.ctypes.data, len(first), frames.ctypes.data, accumulator.ctypes.data,
                                                       moments.ctypes.data, None if pixels is None else pixels.ctypes.data, 0 if pixels is None else pixels.size, byref(record), tiers.ctypes.data, sentinel, final.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return frames, accumulator, moments, tiers, final


def accumulate_frames(ctx, frames, accumulator, moments, first_sample, sample_count=None, merged=False, sentinel=0x7fc0dead):
    """rt_accumulate_frames: one accumulate launch on explicit images over the context's pixel set. frames: (samples, height, pitch, 4) float32; accumulator and
    moments (None: the plain kernel): (height, pitch, 4). merged=False: first_sample an int, all frames one batch (<= 16). merged=True: first_sample and
    sample_count are lists, one entry per submission. Returns (frames, accumulator, moments, final_image) after the launch; final_image holds `sentinel`
    (uint32 bits) where the launch did not write."""
    frames, (accumulator, moments), first, count, final = _accumulate_staging(frames, (accumulator, moments), first_sample, sample_count, merged)
    status = device_lib().rt_accumulate_frames(ctx, 1 if merged else 0, first.ctypes.data, count.ctypes.data, len(first), frames.ctypes.data, accumulator.ctypes.data,
                                               None if moments is None else moments.ctypes.data, sentinel, final.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return frames, accumulator, moments, final


def _selection(out, flags):
    shape = (out.cells_y, out.cells_x)
    return {"cells_x": out.cells_x, "cells_y": out.cells_y, "hot_cells": out.hot_cells, "active_cells": out.active_cells, "list_pixels": out.list_pixels,
            "hot": (flags & 1).astype(bool).reshape(shape), "active": ((flags >> 1) & 1).astype(bool).reshape(shape)}


def select_active_cells(ctx, height, width, threshold, floor=1e-2, dilate=1, cell_capacity=None):
    """rt_select_active_cells on the context's accumulator and moments; the list stays with the context. Returns a dict: cells_x, cells_y,
    hot_cells, active_cells, list_pixels, hot / active (cells_y, cells_x) bool."""
    cells_x, cells_y = _noise_cells(width, height)
    n = cells_x * cells_y
    flags = np.zeros(n, np.uint8)
    out = CellSelectionRecord()
    status = device_lib().rt_select_active_cells(ctx, c_float(floor), c_float(threshold), int(dilate), byref(out), flags.ctypes.data, n if cell_capacity is None else cell_capacity)
    if status:
        raise DeviceRefusal(ctx, status)
    return _selection(out, flags)


def set_pixel_list(ctx, enable):
    status = device_lib().rt_set_pixel_list(ctx, 1 if enable else 0)
    if status:
        raise DeviceRefusal(ctx, status)


def get_pixel_list(ctx):
    return bool(device_lib().rt_get_pixel_list(ctx))


def read_pixel_list(ctx):
    """rt_read_pixel_list: the selected list, uint32 x + y * width each."""
    lib = device_lib()
    count = c_size_t()
    status = lib.rt_read_pixel_list(ctx, None, 0, byref(count))
    if status:
        raise DeviceRefusal(ctx, status)
    pixels = np.zeros(count.value, np.uint32)
    status = lib.rt_read_pixel_list(ctx, pixels.ctypes.data, pixels.size, byref(count))
    if status:
        raise DeviceRefusal(ctx, status)
    return pixels


def _select_pixels_images(ctx, height, width, pitch, images, threshold, floor, held_fraction, dilate, sentinel):
    """The one body of select_pixels_images (images: mean and moments; held_fraction None) and select_pixels_robust_images (mean, moments and resolved)."""
    robust = held_fraction is not None
    images = [_f32(image) for image in images]
    assert all(image.shape == (height, pitch, 4) for image in images)
    cells_x, cells_y = _noise_cells(width, height)
    n = cells_x * cells_y
    cells = {"cell_sums": np.zeros(n, np.float64), "cell_counts": np.zeros(n, np.int32), "cell_nonfinite": np.zeros(n, np.int32)}
    if robust:
        cells["cell_held"] = np.zeros(n, np.int32)
    flags = np.zeros(n, np.uint8)
    pixels = np.full(width * height, sentinel, np.uint32)
    out = CellSelectionRecord()
    args = [image.ctypes.data for image in images] + [c_float(floor)] + ([c_float(held_fraction)] if robust else []) + [c_float(threshold), int(dilate), byref(out)]
    args += [a.ctypes.data for a in cells.values()] + [flags.ctypes.data, n, pixels.ctypes.data, pixels.size]
    status = getattr(device_lib(), "rt_select_pixels_robust_images" if robust else "rt_select_pixels_images")(ctx, *args)
    if status:
        raise DeviceRefusal(ctx, status)
    result = _selection(out, flags)
    result.update((name, a.reshape(cells_y, cells_x)) for name, a in cells.items())
    result.update(list=pixels[:out.list_pixels].copy(), list_tail=pixels[out.list_pixels:].copy())
    return result


def select_pixels_images(ctx, height, width, pitch, mean, moments, threshold, floor=1e-2, dilate=1, sentinel=0xffffffff):
    """rt_select_pixels_images: selection and compaction on the caller's (height, pitch, 4) float32 images. Returns the dict of select_active_cells plus cell_sums /
    cell_counts / cell_nonfinite (cells_y, cells_x), list (the list_pixels entries) and list_tail (the rest of the width * height entries: still `sentinel`)."""
    return _select_pixels_images(ctx, height, width, pitch, (mean, moments), threshold, floor, None, dilate, sentinel)


def accumulate_list_frames(ctx, frames, accumulator, moments, pixels, sample_count, first_sample=None, sentinel=0x7fc0dead):
    """rt_accumulate_list_frames: one launch of the accumulate step over a pixel list. frames (samples, height, pitch, 4), accumulator and moments (height, pitch, 4) float32;
    pixels: the list (x + y * width); sample_count: one entry per submission (first_sample likewise; it does not enter the fold). Returns (frames, accumulator,
    moments, final_image) after the launch."""
    first_sample = np.full(np.size(sample_count), 16, np.int32) if first_sample is None else first_sample
    frames, (accumulator, moments), first, count, final = _accumulate_staging(frames, (accumulator, moments), first_sample, sample_count, True)
    pixels = np.ascontiguousarray(pixels, np.uint32)
    status = device_lib().rt_accumulate_list_frames(ctx, first.ctypes.data, count.ctypes.data, len(count), frames.ctypes.data, accumulator.ctypes.data, moments.ctypes.data,
                                                    pixels.ctypes.data, pixels.size, sentinel, final.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return frames, accumulator, moments, final


def noise_summary(cell_sums, cell_counts, quantile):
    """grt_noise_summary of the host library: (status, mean, figure, pixels). status 0 fine, 1 no cell has a count, -1 quantile outside (0, 1]."""
    lib = host_lib()
    lib.grt_noise_summary.argtypes = [c_void_p, c_void_p, c_size_t, ctypes.c_double, POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(ctypes.c_longlong)]
    sums = np.ascontiguousarray(cell_sums, np.float64).ravel()
    counts = np.ascontiguousarray(cell_counts, np.int32).ravel()
    mean, figure, pixels = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
    status = lib.grt_noise_summary(sums.ctypes.data, counts.ctypes.data, sums.size, float(quantile), byref(mean), byref(figure), byref(pixels))
    return status, mean.value, figure.value, pixels.value


def trace_rays(ctx, origin, direction, repeat=1):
    """rt_trace_rays: origin/direction are (3, N) float32 SoA. Returns (hits uint32[N,4], mean kernel ms)."""
    o, d = _f32(origin), _f32(direction)
    n = o.shape[1]
    hits = np.zeros((n, 4), np.uint32)
    ms = c_float()
    _dev_check(ctx, device_lib().rt_trace_rays(ctx, *_soa_pointers(o, d), n, hits.ctypes.data, repeat, byref(ms)))
    return hits, ms.value


def trace_shadow_rays(ctx, origin, direction, max_distance, repeat=1):
    o, d, m = _f32(origin), _f32(direction), _f32(max_distance)
    n = o.shape[1]
    occluded = np.zeros(n, np.uint8)
    ms = c_float()
    _dev_check(ctx, device_lib().rt_trace_shadow_rays(ctx, *_soa_pointers(o, d), m.ctypes.data, n, occluded.ctypes.data, repeat, byref(ms)))
    return occluded, ms.value


def trace_stream_rays(ctx, iteration, origin, direction, hits, shadow_origin, shadow_direction, max_distance, counting=False):
    """rt_trace_stream_rays: the merged wavefront's traversal launch on explicit rays. origin/direction (3, N) and shadow_origin /
    shadow_direction (3, M) float32 SoA, max_distance (M,); `hits` (N, 4) uint32 is what the hit records hold before the launch.
    Returns (hits, shadow_light float32[M], stats dict as get_trace_statistics or None, info int32[4])."""
    o, d = _f32(origin).reshape(3, -1), _f32(direction).reshape(3, -1)
    so, sd, m = _f32(shadow_origin).reshape(3, -1), _f32(shadow_direction).reshape(3, -1), _f32(max_distance).reshape(-1)
    n, k = o.shape[1], so.shape[1]
    if d.shape[1] != n or sd.shape[1] != k or m.size != k:
        raise ValueError("trace_stream_rays: ray arrays of different lengths")
    out = np.array(hits, np.uint32, order="C", copy=True).reshape(n, 4)
    light = np.zeros(k, np.float32)
    stats = np.zeros(10, np.uint64) if counting else None
    info = np.zeros(4, np.int32)
    _dev_check(ctx, device_lib().rt_trace_stream_rays(ctx, iteration, *_soa_pointers(o, d), n, out.ctypes.data, *_soa_pointers(so, sd), m.ctypes.data, k, light.ctypes.data,
                                                      stats.ctypes.data if counting else None, info.ctypes.data))
    return out, light, _trace_statistics(stats) if counting else None, info


TRACE_QUEUE_PLAIN, TRACE_QUEUE_COUNTING, TRACE_QUEUE_AO = 0, 1, 2   # RT_TRACE_QUEUE_*: the forms of rt_trace_queue_rays
TRACE_QUEUE_FLAG_BOUNCE_0 = 1 << 30                                  # merged form: the pixel word of a shadow ray of bounce 0


def trace_queue_rays(ctx, step, origin, direction, hits, shadow_origin, shadow_direction, max_distance, illumination, pixel_words, frames, frame_pixels,
                     merged=False, form=TRACE_QUEUE_PLAIN):
    """rt_trace_queue_rays: one bounce's traversal launches of the slots scheduler (step = bounce), or with `merged` the merged wavefront's launch
    (step = iteration), on explicit queues. origin/direction (3, N), shadow_origin/shadow_direction (3, M) float32 SoA, max_distance (M,),
    illumination (M, 3) float32, pixel_words (M,) uint32; `hits` (N, 4) uint32 is what the hit records hold before the launch; frames: three
    (frame_pixels, 4) float32 arrays {RADIANCE, RADIANCE_DIRECT, RADIANCE_INDIRECT} as they are before the launch, None for a frame the launch does
    not have. Returns (hits, [the three frames after the launch, None where None], stats dict as get_trace_statistics or None, info int32[6])."""
    o, d = _f32(origin).reshape(3, -1), _f32(direction).reshape(3, -1)
    so, sd, m = _f32(shadow_origin).reshape(3, -1), _f32(shadow_direction).reshape(3, -1), _f32(max_distance).reshape(-1)
    light = _f32(illumination).reshape(-1, 3)
    words = np.ascontiguousarray(pixel_words, np.uint32).reshape(-1)
    n, k = o.shape[1], so.shape[1]
    if d.shape[1] != n or sd.shape[1] != k or m.size != k or light.shape[0] != k or words.size != k:
        raise ValueError("trace_queue_rays: ray arrays of different lengths")
    out = np.array(hits, np.uint32, order="C", copy=True).reshape(n, 4)
    after = [None if f is None else np.array(f, np.float32, order="C", copy=True).reshape(frame_pixels, 4) for f in frames]
    if len(after) != 3:
        raise ValueError("trace_queue_rays: three frames (or None) are expected")
    counting = form == TRACE_QUEUE_COUNTING
    stats = np.zeros(10, np.uint64) if counting else None
    info = np.zeros(6, np.int32)
    _dev_check(ctx, device_lib().rt_trace_queue_rays(ctx, 1 if merged else 0, step, form, *_soa_pointers(o, d), n, out.ctypes.data, *_soa_pointers(so, sd), m.ctypes.data,
                                                     light.ctypes.data, words.ctypes.data, k, *[None if f is None else f.ctypes.data for f in after], frame_pixels,
                                                     stats.ctypes.data if counting else None, info.ctypes.data))
    return out, after, _trace_statistics(stats) if counting else None, info


def generate_rays(ctx, sample_index, pixel_offset, pixel_count):
    o = np.zeros((3, pixel_count), np.float32)
    d = np.zeros((3, pixel_count), np.float32)
    px = np.zeros(pixel_count, np.uint32)
    _dev_check(ctx, device_lib().rt_generate_rays(ctx, sample_index, pixel_offset, pixel_count, *_soa_pointers(o, d), px.ctypes.data))
    return o, d, px


def generate_primary_rays(ctx, kernel, queue, first_sample=0, sample_count=1, pixel_offset=0, pixel_count=0, tiles=(0, 0, 0), slot_base=0, iteration=0,
                          queue_before=0, queue_offset=0, order=None, pixel_list=None):
    """rt_generate_primary_rays: kernel 0 kernel_generate, 1 kernel_generate_stream, 2 kernel_generate_stream_list on the submission given here.
    `queue` (7, capacity) uint32 is what the seven queue arrays {ox, oy, oz, dx, dy, dz, pixel word} hold before the launch; tiles = (tile_pixels,
    tile_first, tile_stride); order = (block_width, band_rows), None for the scheduler's choice; pixel_list (kernel 2) replaces pixel_offset / pixel_count.
    Returns (queue after the launch (7, capacity) uint32, info int32[4] {block_width, band_rows, workgroups, count word after})."""
    out = np.array(queue, np.uint32, order="C", copy=True)
    if out.ndim != 2 or out.shape[0] != 7:
        raise ValueError("generate_primary_rays: queue must be (7, capacity)")
    px = None
    if pixel_list is not None:
        px = np.ascontiguousarray(pixel_list, np.uint32).ravel()
        pixel_count = px.size
    block_width, band_rows = (-1, -1) if order is None else order
    info = np.zeros(4, np.int32)
    status = device_lib().rt_generate_primary_rays(ctx, int(kernel), int(iteration), int(first_sample), int(sample_count), int(pixel_offset), int(pixel_count),
                                                   int(tiles[0]), int(tiles[1]), int(tiles[2]), int(slot_base), int(queue_before), int(queue_offset),
                                                   int(block_width), int(band_rows), px.ctypes.data if px is not None else None, out.shape[1],
                                                   *[out[i].ctypes.data for i in range(7)], info.ctypes.data)
    if status:
        raise DeviceRefusal(ctx, status)
    return out, info


def random_samples(ctx, dimension, pixel_indices, bounce, sample_index):
    px = np.ascontiguousarray(pixel_indices, dtype=np.uint32)
    out = np.zeros((px.size, 2), np.float32)
    _dev_check(ctx, device_lib().rt_random_samples(ctx, dimension, px.ctypes.data, px.size, bounce, sample_index, out.ctypes.data))
    return out


def sample_texture(ctx, texture_index, filter, args):
    """rt_sample_texture: args is (N, 8) {s, t, lod, dx.x, dx.y, dy.x, dy.y, pad}; filter 0 = level 0, 1 = lod, 2 = gradients.
    Returns (N, 4) float32 RGBA."""
    a = _f32(args).reshape(-1, 8)
    out = np.zeros((a.shape[0], 4), np.float32)
    _dev_check(ctx, device_lib().rt_sample_texture(ctx, texture_index, filter, a.ctypes.data, a.shape[0], out.ctypes.data))
    return out


def sample_table(ctx, table, coords):
    """rt_sample_table: lut_get_1d / _2d / _3d on `table`, a 1-, 2- or 3-d array indexed [z][y][x]; coords is (N, dims).
    Returns (N,) float32."""
    t = _f32(table)
    dims = t.ndim
    shape = t.shape[::-1] + (1,) * (3 - dims)   # nx, ny, nz
    c = np.zeros((np.asarray(coords).reshape(-1, dims).shape[0], 3), np.float32)
    c[:, :dims] = np.asarray(coords, np.float32).reshape(-1, dims)
    out = np.zeros(c.shape[0], np.float32)
    _dev_check(ctx, device_lib().rt_sample_table(ctx, t.ctypes.data, shape[0], shape[1], shape[2], dims, c.ctypes.data, c.shape[0], out.ctypes.data))
    return out


def sample_sky(ctx, directions):
    """rt_sample_sky: sample_sky on the context's sky for (N, 3) unit directions. Returns (N, 3) float32."""
    d = _f32(directions).reshape(-1, 3)
    out = np.zeros((d.shape[0], 3), np.float32)
    _dev_check(ctx, device_lib().rt_sample_sky(ctx, d.ctypes.data, d.shape[0], out.ctypes.data))
    return out


def sample_sky_distribution(ctx, uv):
    """rt_sample_sky_distribution: the sky importance sampling's inversion for (N, 2) points of [0, 1)^2 (u: column, v: row).
    Returns (N, 4) float32: the direction and its pdf in solid angle."""
    p = _f32(uv).reshape(-1, 2)
    out = np.zeros((p.shape[0], 4), np.float32)
    _dev_check(ctx, device_lib().rt_sample_sky_distribution(ctx, p.ctypes.data, p.shape[0], out.ctypes.data))
    return out


def sky_pdf(ctx, directions):
    """rt_sky_pdf: the pdf (solid angle) the sky importance sampling gives (N, 3) unit directions. Returns (N,) float32."""
    d = _f32(directions).reshape(-1, 3)
    out = np.zeros(d.shape[0], np.float32)
    _dev_check(ctx, device_lib().rt_sky_pdf(ctx, d.ctypes.data, d.shape[0], out.ctypes.data))
    return out


BSDF_PROBE_IN, BSDF_PROBE_OUT = 24, 12   # floats per probe record of rt_bsdf_eval / rt_bsdf_sample


def bsdf_eval(ctx, material_type, probes):
    """rt_bsdf_eval: the shade kernels' BSDF `material_type` (MATERIAL_DIFFUSE .. MATERIAL_CONDUCTOR) evaluated on (N, 24) probe
    records (see include/gpu_raytracer_amd.h). Returns (N, 12) float32 {ok, pdf, bsdf[3], to_light[3], medium, allow_nee, omega_i.z, pad}."""
    return _bsdf_probe(ctx, device_lib().rt_bsdf_eval, material_type, probes)


def bsdf_sample(ctx, material_type, probes):
    """rt_bsdf_sample: the same BSDF's sample on (N, 24) probe records. Returns (N, 12) float32 {ok, pdf, throughput factor[3],
    direction[3], medium, allow_nee, omega_i.z, pad}."""
    return _bsdf_probe(ctx, device_lib().rt_bsdf_sample, material_type, probes)

SORT_TRACE_WORDS, SORT_MATERIAL_WORDS = 20, 16   # RT_SORT_TRACE_WORDS, RT_SORT_MATERIAL_WORDS
STREAM_SUBMISSIONS, STAT_KINDS, MAX_BOUNCES = 128, 6, 128


def _queue_launch_staging(r, records_in, words, frame_pixels, frame_slots, bounce, sample_index, iteration, slot_table, submission_birth, capacity, sentinel, material_slot=None):
    """What sort_rays and shade_rays stage alike: the entries as (N, words) uint32, the merged form's slot table and births, the capacity, and on the result `r`
    trace_out (capacity, 20) and stats. Returns (r, the arguments of the entry point from `merged` to `sentinel`, pixels in the frames); r._staged keeps the staged
    arrays alive for the call."""
    records = np.ascontiguousarray(records_in, np.uint32).reshape(-1, words)
    n = records.shape[0]
    merged = iteration is not None
    capacity = max(n, 1) if capacity is None else int(capacity)
    r.trace_out = np.zeros((capacity, SORT_TRACE_WORDS), np.uint32)
    r.stats = np.zeros((STREAM_SUBMISSIONS, STAT_KINDS, MAX_BOUNCES), np.int32) if merged else None
    slots = np.ascontiguousarray(slot_table, np.int32).reshape(-1, 4) if merged else None
    births = np.ascontiguousarray(submission_birth, np.int32).reshape(STREAM_SUBMISSIONS) if merged else None
    r._staged = (records, slots, births)
    head = [1 if merged else 0, int(iteration if merged else bounce), int(sample_index)] + ([] if material_slot is None else [int(material_slot)])
    head += [records.ctypes.data if n else None, n, slots.ctypes.data if merged else None, slots.shape[0] if merged else 0, births.ctypes.data if merged else None,
             capacity, int(frame_slots), int(sentinel)]
    return r, head, int(frame_pixels) * int(frame_slots)


class SortResult:
    """What one sort launch left behind (rt_sort_rays): trace_out (capacity, 20) and material_out (4, capacity, 16) uint32 records read
    back to their capacity, counters int32[6] {diffuse, plastic, dielectric, conductor, next trace, this trace}, aov (4, P, 4) float32
    (RADIANCE, DIRECT, INDIRECT, ALBEDO), gbuffer_normal_and_depth (P, 4), gbuffer_ids (P, 2) int32, gbuffer_screen_prev (P, 2),
    pixel_query int32[2], stats (128, 6, 128) int32 (merged form, else None)."""


def sort_rays(ctx, trace_in, frame_pixels, frame_slots, bounce=None, sample_index=0, iteration=None, slot_table=None, submission_birth=None,
              capacity=None, sentinel=0xFFC0DE42, aov=None, gbuffer_normal_and_depth=None, gbuffer_ids=None, gbuffer_screen_prev=None, pixel_query=None, _fog=False):
    """rt_sort_rays: the production sort launch on explicit entries. trace_in: (N, 20) uint32 records. Per-bounce form: bounce and
    sample_index; merged form: iteration, slot_table (S, 4) int32 and submission_birth int32[128]. The frames hold frame_slots *
    frame_pixels pixels; aov / g-buffers / pixel_query are their contents before the launch (zeros / the sentinel when None)."""
    r, head, pixels = _queue_launch_staging(SortResult(), trace_in, SORT_TRACE_WORDS, frame_pixels, frame_slots, bounce, sample_index, iteration, slot_table, submission_birth, capacity, sentinel)
    capacity, merged = r.trace_out.shape[0], iteration is not None
    r.material_out = np.zeros((4, capacity, SORT_MATERIAL_WORDS), np.uint32)
    r.counters = np.zeros(6, np.int32)
    r.aov = np.zeros((4, pixels, 4), np.float32) if aov is None else np.array(aov, np.float32, order="C", copy=True).reshape(4, pixels, 4)
    r.gbuffer_normal_and_depth = np.zeros((pixels, 4), np.float32) if gbuffer_normal_and_depth is None else np.array(gbuffer_normal_and_depth, np.float32, order="C", copy=True).reshape(pixels, 4)
    r.gbuffer_ids = np.zeros((pixels, 2), np.int32) if gbuffer_ids is None else np.array(gbuffer_ids, np.int32, order="C", copy=True).reshape(pixels, 2)
    r.gbuffer_screen_prev = np.zeros((pixels, 2), np.float32) if gbuffer_screen_prev is None else np.array(gbuffer_screen_prev, np.float32, order="C", copy=True).reshape(pixels, 2)
    r.pixel_query = np.full(2, sentinel, np.uint32).view(np.int32) if pixel_query is None else np.array(pixel_query, np.int32, copy=True).reshape(2)
    args = (ctx, *head, r.trace_out.ctypes.data, r.material_out.ctypes.data, r.counters.ctypes.data,
            r.aov.ctypes.data, r.gbuffer_normal_and_depth.ctypes.data, r.gbuffer_ids.ctypes.data, r.gbuffer_screen_prev.ctypes.data,
            r.pixel_query.ctypes.data, r.stats.ctypes.data if merged else None)
    if _fog:
        r.shadow_out = np.zeros((capacity, 11), np.uint32); shadow_count = c_int()
        _dev_check(ctx, device_lib().rt_sort_rays_fog(*args, r.shadow_out.ctypes.data, byref(shadow_count)))
        r.shadow_count = shadow_count.value
    else:
        _dev_check(ctx, device_lib().rt_sort_rays(*args))
    return r


def sort_rays_fog(ctx, trace_in, frame_pixels, frame_slots, **kwargs):
    """rt_sort_rays_fog: sort_rays with the fog volume in force (the ..._fog instance). The SortResult also carries shadow_out (capacity, 11)
    uint32 {origin, direction, max_distance, illumination, pixel word}, the light samples of the scatter vertices, and shadow_count."""
    return sort_rays(ctx, trace_in, frame_pixels, frame_slots, _fog=True, **kwargs)


SHADE_SHADOW_WORDS = 11   # RT_SHADE_SHADOW_WORDS


class ShadeResult:
    """What one material launch left behind (rt_shade_rays), every array read back whole as uint32 words: trace_out (capacity, 20), the next
    trace queue; shadow_out (capacity, 11) {origin, direction, max_distance, illumination, pixel word}; counters int32[3] {next trace,
    shadow, this material queue}; aov (3, P, 4) (ALBEDO, NORMAL, POSITION); gbuffer_normal_and_depth (P, 4), gbuffer_ids (P, 2),
    gbuffer_screen_prev (P, 2); stats (128, 6, 128) int32 (merged form, else None). A word the launch did not write holds the sentinel."""


def shade_rays(ctx, material_slot, material_in, frame_pixels, frame_slots, bounce=None, sample_index=0, iteration=None, slot_table=None, submission_birth=None,
               capacity=None, sentinel=0xFFC0DE42):
    """rt_shade_rays: the production material launch of queue `material_slot` on explicit entries. material_in: (N, 16) uint32 records, one
    of the queues of SortResult.material_out. Per-bounce form: bounce and sample_index; merged form: iteration, slot_table (S, 4) int32 and
    submission_birth int32[128]. The frames hold frame_slots * frame_pixels pixels."""
    r, head, pixels = _queue_launch_staging(ShadeResult(), material_in, SORT_MATERIAL_WORDS, frame_pixels, frame_slots, bounce, sample_index, iteration, slot_table, submission_birth, capacity, sentinel,
                                            material_slot)
    capacity, merged = r.trace_out.shape[0], iteration is not None
    r.shadow_out = np.zeros((capacity, SHADE_SHADOW_WORDS), np.uint32)
    r.counters = np.zeros(3, np.int32)
    r.aov = np.zeros((3, pixels, 4), np.uint32)
    r.gbuffer_normal_and_depth = np.zeros((pixels, 4), np.uint32)
    r.gbuffer_ids = np.zeros((pixels, 2), np.uint32)
    r.gbuffer_screen_prev = np.zeros((pixels, 2), np.uint32)
    _dev_check(ctx, device_lib().rt_shade_rays(ctx, *head, r.trace_out.ctypes.data, r.shadow_out.ctypes.data, r.counters.ctypes.data,
                                               r.aov.ctypes.data, r.gbuffer_normal_and_depth.ctypes.data, r.gbuffer_ids.ctypes.data, r.gbuffer_screen_prev.ctypes.data,
                                               r.stats.ctypes.data if merged else None))
    return r


LIGHT_SAMPLE_OUT = 16   # floats per output record of rt_sample_lights


def sample_lights(ctx, probes, use_lds=True):
    """rt_sample_lights: the shade kernels' nee_pick_light on (N, 4) {u_mesh, u_triangle, u_1, u_2} in [0, 1), on the light tables
    the context holds; use_lds: tables chosen as the shade kernels choose them (LDS when they fit), else global memory. Returns
    (N, 16) float32 {entry, transform id, triangle, read LDS (int32 bits: .view(np.int32)), point[3], normal[3], emission[3], pad[3]}."""
    p = _f32(probes).reshape(-1, 4)
    out = np.zeros((p.shape[0], LIGHT_SAMPLE_OUT), np.float32)
    _dev_check(ctx, device_lib().rt_sample_lights(ctx, p.ctypes.data, p.shape[0], 1 if use_lds else 0, out.ctypes.data))
    return out


def upload_lights(ctx, triangle_indices, triangle_cdf, mesh_cdf, mesh_spans, mesh_transform_indices, total_weight):
    """rt_upload_lights on numpy tables (mesh_spans: (M, 2) {first, last}). Returns the status (0: RT_OK); the message of a
    refusal is rt_last_error's."""
    ti = np.ascontiguousarray(triangle_indices, dtype=np.int32); tc = _f32(triangle_cdf)
    mc = _f32(mesh_cdf); ms = np.ascontiguousarray(mesh_spans, dtype=np.int32); mt = np.ascontiguousarray(mesh_transform_indices, dtype=np.int32)
    if tc.size != ti.size or ms.size != 2 * mc.size or mt.size != mc.size:
        raise ValueError("upload_lights: tables of different lengths")
    ptr = lambda a: a.ctypes.data if a.size else None
    return device_lib().rt_upload_lights(ctx, ptr(ti), ptr(tc), ti.size, ptr(mc), ptr(ms), ptr(mt), mc.size, float(total_weight))


DELTA_LIGHT_POINT, DELTA_LIGHT_SPOT, DELTA_LIGHT_DIRECTIONAL = 0, 1, 2   # RT_DELTA_LIGHT_*
DELTA_LIGHT_WORDS = 16    # 32-bit words of an rt_delta_light and of a staged record (RT_DELTA_LIGHT_RECORD)
DELTA_SAMPLE_OUT = 12     # floats per output record of rt_sample_delta_lights
MAX_DELTA_LIGHTS = 65536  # RT_MAX_DELTA_LIGHTS


def delta_light_records(lights, weights):
    """(N, 16) float32 rt_delta_light records from (N, 12) lights {type, position[3], direction[3], intensity[3], cutoff, beam} and N weights."""
    l = _f32(lights).reshape(-1, 12)
    r = np.zeros((l.shape[0], DELTA_LIGHT_WORDS), np.float32)
    r.view(np.int32)[:, 0] = l[:, 0].astype(np.int32)
    r[:, 1:12] = l[:, 1:12]
    r[:, 12] = _f32(weights).reshape(-1)
    return r


def upload_delta_lights(ctx, records, share=1.0):
    """rt_upload_delta_lights on (N, 16) float32 rt_delta_light records (delta_light_records); records None or empty clears the table.
    Returns the status (0: RT_OK); the message of a refusal is rt_last_error's."""
    if records is None:
        return device_lib().rt_upload_delta_lights(ctx, None, 0, float(share))
    r = _f32(records).reshape(-1, DELTA_LIGHT_WORDS)
    return device_lib().rt_upload_delta_lights(ctx, r.ctypes.data if r.size else None, r.shape[0], float(share))


def read_delta_lights(ctx):
    """rt_read_delta_lights: (records (N, 16) float32 {position[3], type (int32 bits), unit direction[3], P_k, intensity[3], cos cutoff,
    cos beam, cutoff, 1 / (cutoff - beam), pad}, cdf (N,) float32, share) as staged for the kernels."""
    lib = device_lib()
    n, share = c_size_t(), c_float()
    _dev_check(ctx, lib.rt_read_delta_lights(ctx, None, None, 0, byref(n), byref(share)))
    records = np.zeros((n.value, DELTA_LIGHT_WORDS), np.float32); cdf = np.zeros(n.value, np.float32)
    _dev_check(ctx, lib.rt_read_delta_lights(ctx, records.ctypes.data, cdf.ctypes.data, n.value, byref(n), byref(share)))
    return records, cdf, share.value


def sample_delta_lights(ctx, probes):
    """rt_sample_delta_lights: the shade kernels' delta-light sample on (N, 4) {u in [0, 1), origin[3]}. Returns (N, 12) float32 {light index
    (int32 bits: .view(np.int32)), to_light[3], max_distance, radiance term[3], P_k, ok, pad[2]}."""
    p = _f32(probes).reshape(-1, 4)
    out = np.zeros((p.shape[0], DELTA_SAMPLE_OUT), np.float32)
    _dev_check(ctx, device_lib().rt_sample_delta_lights(ctx, p.ctypes.data, p.shape[0], out.ctypes.data))
    return out


MAX_LIGHT_TREE_LEAVES = 1 << 22   # RT_MAX_LIGHT_TREE_LEAVES


class LightTree:
    """What rt_read_light_tree returns: leaf_count N, padded M; nodes (2M - 1, 8) float32 {box_min[3], Phi, box_max[3], pad} in heap numbering; leaf_entry,
    leaf_triangle (N,) int32 and leaf_area, leaf_power (N,) float32 by leaf id; slot_of_leaf (N,) int32; entry_of_mesh, place_of_triangle int32."""


def set_light_tree(ctx, enable):
    """rt_set_light_tree. Returns the status (0: RT_OK); the message of a refusal is rt_last_error's."""
    return device_lib().rt_set_light_tree(ctx, 1 if enable else 0)


def read_light_tree(ctx, mesh_count=0, triangle_count=0):
    """rt_read_light_tree: the light tree as built (a LightTree; leaf_count 0 while none exists). mesh_count / triangle_count: the scene's instances and
    triangles, to read the inverse tables entry_of_mesh and place_of_triangle as well (0: not read)."""
    lib = device_lib()
    n, m = c_int(), c_int()
    _dev_check(ctx, lib.rt_read_light_tree(ctx, byref(n), byref(m), None, 0, None, None, 0, None, 0, None, 0))
    t = LightTree()
    t.leaf_count, t.padded = n.value, m.value
    nodes = np.zeros((max(2 * t.padded - 1, 0), 8), np.float32)
    leaves = np.zeros((t.leaf_count, 4), np.uint32)
    t.slot_of_leaf = np.zeros(t.leaf_count, np.int32)
    t.entry_of_mesh = np.full(mesh_count, -1, np.int32); t.place_of_triangle = np.full(triangle_count, -1, np.int32)
    if t.padded:
        _dev_check(ctx, lib.rt_read_light_tree(ctx, byref(n), byref(m), nodes.ctypes.data, nodes.shape[0], leaves.ctypes.data, t.slot_of_leaf.ctypes.data, t.leaf_count,
                                               t.entry_of_mesh.ctypes.data if mesh_count else None, mesh_count,
                                               t.place_of_triangle.ctypes.data if triangle_count else None, triangle_count))
    t.nodes = nodes
    t.leaf_entry = leaves[:, 0].view(np.int32).copy(); t.leaf_triangle = leaves[:, 1].view(np.int32).copy()
    t.leaf_area = leaves[:, 2].view(np.float32).copy(); t.leaf_power = leaves[:, 3].view(np.float32).copy()
    return t


def sample_light_tree(ctx, u, u2, points):
    """rt_sample_light_tree: the kernels' descent of the light tree on N probes -- u, u2 in [0, 1) (scalars or (N,)), points (N, 3). Returns (leaf id (N,) int32,
    -1 where the tree holds no power; node (N,) int32; pmf (N,) float32)."""
    pts = _f32(points).reshape(-1, 3)
    probes = np.empty((pts.shape[0], 5), np.float32)
    probes[:, 0] = u; probes[:, 1] = u2; probes[:, 2:] = pts
    out = np.zeros((pts.shape[0], 4), np.float32)
    _dev_check(ctx, device_lib().rt_sample_light_tree(ctx, probes.ctypes.data, probes.shape[0], out.ctypes.data))
    return out[:, 0].view(np.int32).copy(), out[:, 1].view(np.int32).copy(), out[:, 2].copy()


def light_tree_pmf(ctx, leaves, points):
    """rt_light_tree_pmf: the probability with which the descent from points[i] arrives at leaf leaves[i] (ids; a scalar or (N,)), (N,) float32."""
    pts = _f32(points).reshape(-1, 3)
    probes = np.empty((pts.shape[0], 4), np.float32)
    probes.view(np.int32)[:, 0] = leaves; probes[:, 1:] = pts
    out = np.zeros(pts.shape[0], np.float32)
    _dev_check(ctx, device_lib().rt_light_tree_pmf(ctx, probes.ctypes.data, probes.shape[0], out.ctypes.data))
    return out


FOG_VOLUME_WORDS = 16    # 32-bit words of an rt_fog_volume
FOG_SEGMENT_IN = 16      # words per probe record of rt_fog_segments
FOG_SEGMENT_OUT = 16     # words per output record of rt_fog_segments


def fog_volume_record(box_min, box_max, sigma_a, sigma_s, g=0.0):
    """An rt_fog_volume as (16,) float32: box_min[3], box_max[3], sigma_a[3], sigma_s[3], g, 3 reserved words. sigma_a / sigma_s: one number or three."""
    r = np.zeros(FOG_VOLUME_WORDS, np.float32)
    r[0:3] = _f32(box_min).reshape(3); r[3:6] = _f32(box_max).reshape(3)
    r[6:9] = np.broadcast_to(_f32(sigma_a).reshape(-1), (3,)); r[9:12] = np.broadcast_to(_f32(sigma_s).reshape(-1), (3,))
    r[12] = g
    return r


def set_fog_volume(ctx, record):
    """rt_set_fog_volume on a (16,) float32 record (fog_volume_record); None clears the volume. Returns the status (0: RT_OK); the message of a
    refusal is rt_last_error's."""
    if record is None:
        return device_lib().rt_set_fog_volume(ctx, None)
    r = _f32(record).reshape(FOG_VOLUME_WORDS)
    return device_lib().rt_set_fog_volume(ctx, r.ctypes.data)


def get_fog_volume(ctx):
    """rt_get_fog_volume: the (16,) float32 record in force, or None when no volume is set."""
    r = np.zeros(FOG_VOLUME_WORDS, np.float32); is_set = c_int()
    _dev_check(ctx, device_lib().rt_get_fog_volume(ctx, r.ctypes.data, byref(is_set)))
    return r if is_set.value else None


def fog_segment_probes(origin, direction, t_end, pixel, bounce, sample, throughput, inside_medium=0):
    """(N, 16) uint32 probe records of rt_fog_segments from per-probe arrays (scalars broadcast)."""
    o = _f32(origin).reshape(-1, 3)
    n = o.shape[0]
    r = np.zeros((n, FOG_SEGMENT_IN), np.uint32)
    f = r.view(np.float32)
    f[:, 0:3] = o; f[:, 3:6] = _f32(direction).reshape(-1, 3); f[:, 6] = _f32(t_end)
    r[:, 7] = np.asarray(pixel, np.uint32); r[:, 8] = np.asarray(bounce, np.uint32); r[:, 9] = np.asarray(sample, np.uint32)
    f[:, 10:13] = _f32(throughput).reshape(-1, 3)
    r[:, 13] = np.asarray(inside_medium, np.uint32)
    return r


def fog_segments(ctx, probes):
    """rt_fog_segments: the fog's segment step on (N, 16) uint32 records (fog_segment_probes). Returns (N, 16) uint32 {t0, t1, the two random
    numbers, scattered, distance, throughput'[3], vertex[3], pad[4]}; view the floats with .view(np.float32)."""
    p = np.ascontiguousarray(probes, np.uint32).reshape(-1, FOG_SEGMENT_IN)
    out = np.zeros((p.shape[0], FOG_SEGMENT_OUT), np.uint32)
    _dev_check(ctx, device_lib().rt_fog_segments(ctx, p.ctypes.data if p.size else None, p.shape[0], out.ctypes.data if p.size else None))
    return out


def attenuate_shadow_rays(ctx, shadow_in):
    """rt_attenuate_shadow_rays: the fog's attenuation pass, as the context's scheduler launches it, on (N, 11) uint32 shadow records
    {origin[3], direction[3], max_distance, illumination[3], pixel word}. Returns the queue after the pass."""
    q = np.ascontiguousarray(shadow_in, np.uint32).reshape(-1, SHADE_SHADOW_WORDS)
    out = np.zeros_like(q)
    _dev_check(ctx, device_lib().rt_attenuate_shadow_rays(ctx, q.ctypes.data if q.size else None, q.shape[0], out.ctypes.data if q.size else None))
    return out


def set_fog_density(ctx, density):
    """rt_set_fog_density: the density grid of the fog volume as an array of shape (nz, ny, nx), x fastest; None clears the grid.
    Returns the status (0: RT_OK); the message of a refusal is rt_last_error's."""
    if density is None:
        return device_lib().rt_set_fog_density(ctx, None, 0, 0, 0)
    d = _f32(density)
    if d.ndim != 3:
        raise ValueError("a density grid has shape (nz, ny, nx), not %r" % (d.shape,))
    nz, ny, nx = d.shape
    return device_lib().rt_set_fog_density(ctx, d.ctypes.data, nx, ny, nz)


def get_fog_density_info(ctx):
    """rt_get_fog_density_info: None without a grid, else dict(dims=(nx, ny, nz), bricks=, empty_bricks=, max_density=)."""
    dims = (c_int * 3)(); bricks = c_int(); empty = c_int(); largest = c_float(); is_set = c_int()
    _dev_check(ctx, device_lib().rt_get_fog_density_info(ctx, dims, byref(bricks), byref(empty), byref(largest), byref(is_set)))
    if not is_set.value:
        return None
    return dict(dims=tuple(dims), bricks=bricks.value, empty_bricks=empty.value, max_density=largest.value)


def fog_density_segments(ctx, probes):
    """rt_fog_density_segments: the segment step over the density grid in force on (N, 16) uint32 records (fog_segment_probes). Returns
    rt_fog_segments' records with word 12 the density length (float), word 13 the voxels read, word 14 the empty bricks crossed."""
    p = np.ascontiguousarray(probes, np.uint32).reshape(-1, FOG_SEGMENT_IN)
    out = np.zeros((p.shape[0], FOG_SEGMENT_OUT), np.uint32)
    _dev_check(ctx, device_lib().rt_fog_density_segments(ctx, p.ctypes.data if p.size else None, p.shape[0], out.ctypes.data if p.size else None))
    return out


def read_vol(path):
    """A Mitsuba 0.6 gridvolume file (VOL, version 3, float32, one channel) as (density of shape (nz, ny, nx), box (6,) float32: min[3], max[3])."""
    lib = host_lib()
    dims = (c_int * 3)(); box = (c_float * 6)()
    _host_check(lib.grt_vol_read(str(path).encode(), dims, box, None, 0))
    density = np.zeros((dims[2], dims[1], dims[0]), np.float32)
    _host_check(lib.grt_vol_read(str(path).encode(), dims, box, density.ctypes.data, density.size))
    return density, np.array(list(box), np.float32)


def write_vol(path, density, box=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0)):
    """Write `density` (nz, ny, nx) with the bounding box (min[3], max[3]) as a Mitsuba 0.6 gridvolume file."""
    d = _f32(density)
    if d.ndim != 3:
        raise ValueError("a density grid has shape (nz, ny, nx), not %r" % (d.shape,))
    b = (c_float * 6)(*[float(v) for v in box])
    _host_check(host_lib().grt_vol_write(str(path).encode(), d.ctypes.data, d.shape[2], d.shape[1], d.shape[0], b))


NORMAL_PROBE_IN = 48   # floats per probe record of rt_perturb_normals


def perturb_normals(ctx, texture_index, probes):
    """rt_perturb_normals: the shade kernels' normal-map perturbation with texture `texture_index` as the map, on (N, 48) probe
    records (see include/gpu_raytracer_amd.h). Returns (N, 4) float32 {world shading normal[3], fell back (1) or mapped (0)}."""
    p = _f32(probes).reshape(-1, NORMAL_PROBE_IN)
    out = np.zeros((p.shape[0], 4), np.float32)
    _dev_check(ctx, device_lib().rt_perturb_normals(ctx, int(texture_index), p.ctypes.data, p.shape[0], out.ctypes.data))
    return out


def upload_material_opacity(ctx, texture_ids, channels, thresholds):
    """rt_upload_material_opacity: per uploaded material a texture id (-1: none), a channel (0..3) and a threshold in (0, 1];
    texture_ids None clears the masks. Returns the status (0: RT_OK)."""
    if texture_ids is None:
        return device_lib().rt_upload_material_opacity(ctx, None, None, None, 0)
    ids = np.ascontiguousarray(texture_ids, dtype=np.int32).reshape(-1)
    ch = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
    th = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
    if ch.size != ids.size or th.size != ids.size:
        raise ValueError("upload_material_opacity: arrays of different lengths")
    keep = np.zeros(1, np.int32)   # (a non-NULL pointer for an empty table: NULL ids mean "clear")
    return device_lib().rt_upload_material_opacity(ctx, ids.ctypes.data if ids.size else keep.ctypes.data, ch.ctypes.data if ids.size else keep.ctypes.data,
                                                   th.ctypes.data if ids.size else keep.ctypes.data, ids.size)


def read_material_opacity(ctx, material):
    """rt_read_material_opacity: the mask of uploaded material `material` as a bool array [H, W] (True: opaque)."""
    w, h = c_int(), c_int()
    lib = device_lib()
    lib.rt_read_material_opacity(ctx, int(material), None, 0, byref(w), byref(h))   # (the size; fails for want of capacity)
    if w.value <= 0 or h.value <= 0:
        raise RuntimeError("device layer: " + lib.rt_last_error(ctx).decode())
    words = np.zeros((w.value * h.value + 31) // 32, np.uint32)
    _dev_check(ctx, lib.rt_read_material_opacity(ctx, int(material), words.ctypes.data, words.size, byref(w), byref(h)))
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:w.value * h.value]
    return bits.reshape(h.value, w.value).astype(bool)


def upload_material_normal_maps(ctx, texture_ids):
    """rt_upload_material_normal_maps: one texture id (-1: none) per uploaded material. Returns the status (0: RT_OK)."""
    ids = np.ascontiguousarray(texture_ids, dtype=np.int32)
    return device_lib().rt_upload_material_normal_maps(ctx, ids.ctypes.data if ids.size else None, ids.size)


def _bsdf_probe(ctx, fn, material_type, probes):
    p = _f32(probes).reshape(-1, BSDF_PROBE_IN)
    out = np.zeros((p.shape[0], BSDF_PROBE_OUT), np.float32)
    _dev_check(ctx, fn(ctx, int(material_type), p.ctypes.data, p.shape[0], out.ctypes.data))
    return out


SVGF_STATE_HISTORY_LENGTH, SVGF_STATE_HISTORY_DIRECT, SVGF_STATE_HISTORY_INDIRECT, SVGF_STATE_HISTORY_MOMENT, \
    SVGF_STATE_HISTORY_NORMAL_AND_DEPTH, SVGF_STATE_FRAME_MOMENT, SVGF_STATE_TAA_HISTORY, SVGF_STATE_TAA_CURRENT = range(8)   # RT_SVGF_STATE_*


def read_svgf_state(ctx, which):
    """rt_read_svgf_state: one of the SVGF / TAA filter's persistent images after the frames filtered so far, as a
    (height, pitch, C) array -- int32 with C = 1 for SVGF_STATE_HISTORY_LENGTH, float32 with C = 4 for the others."""
    lib = device_lib()
    # The ABI has no height query: every filter image has the final image's pitch x height pixels, and
    # rt_framebuffer_device_ptr gives that image's size in bytes (16 per pixel).
    ptr, nbytes = c_void_p(), c_size_t()
    _dev_check(ctx, lib.rt_framebuffer_device_ptr(ctx, byref(ptr), byref(nbytes)))
    pitch = lib.rt_screen_pitch(ctx)
    height = nbytes.value // (16 * pitch)
    if which == SVGF_STATE_HISTORY_LENGTH:
        out = np.zeros((height, pitch, 1), np.int32)
    else:
        out = np.zeros((height, pitch, 4), np.float32)
    _dev_check(ctx, lib.rt_read_svgf_state(ctx, int(which), out.ctypes.data))
    return out


def measure_stream_bandwidth(ctx, nbytes=1 << 30, repeat=5):
    gbps = c_float()
    _dev_check(ctx, device_lib().rt_measure_stream_bandwidth(ctx, nbytes, repeat, byref(gbps)))
    return gbps.value


def read_luts(ctx):
    shapes = [4096, 4096, 256, 256, 1024, 32]
    arrays = [np.zeros(s, np.float32) for s in shapes]
    _dev_check(ctx, device_lib().rt_read_luts(ctx, *[a.ctypes.data for a in arrays]))
    return arrays


def read_sky_tables(ctx):
    """rt_read_sky_tables: the sky importance sampling's tables as the device built them (built now if need be). Returns a dict:
    width, height, marginal (H,) float32, conditional (H, W) float32, cell_pdf (H, W) float32, row_totals (H,) float64, total (float)."""
    lib = device_lib()
    lib.rt_read_sky_tables.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double), c_size_t]
    w, h, total = c_int(), c_int(), c_double()
    _dev_check(ctx, lib.rt_read_sky_tables(ctx, byref(w), byref(h), None, None, None, None, None, 0))
    W, H = w.value, h.value
    marginal = np.zeros(H, np.float32); conditional = np.zeros((H, W), np.float32); cell_pdf = np.zeros((H, W), np.float32)
    row_totals = np.zeros(H, np.float64)
    _dev_check(ctx, lib.rt_read_sky_tables(ctx, byref(w), byref(h), marginal.ctypes.data, conditional.ctypes.data, cell_pdf.ctypes.data,
                                           row_totals.ctypes.data, byref(total), W * H))
    return dict(width=W, height=H, marginal=marginal, conditional=conditional, cell_pdf=cell_pdf, row_totals=row_totals, total=total.value)


def set_trace_statistics(ctx, enable):
    lib = device_lib()
    lib.rt_set_trace_statistics.argtypes = [c_void_p, c_int]
    _dev_check(ctx, lib.rt_set_trace_statistics(ctx, 1 if enable else 0))


def get_trace_statistics(ctx):
    """Returns {'closest': {...}, 'shadow': {...}} with nodes / triangles / instances / rays and the
    algorithmic bytes they imply (24 B ray + 16 B hit | 4 B max_distance, 80 B per node, 48 B per
    triangle, 52 B per transformed instance entry, 4 B per identity entry)."""
    lib = device_lib()
    lib.rt_get_trace_statistics.argtypes = [c_void_p, c_void_p]
    raw = np.zeros(10, np.uint64)
    _dev_check(ctx, lib.rt_get_trace_statistics(ctx, raw.ctypes.data))
    out = _trace_statistics(raw)
    for kind, hit_bytes in (("closest", 16), ("shadow", 4)):
        c = out[kind]
        c["algorithmic_bytes"] = (24 + hit_bytes) * c["rays"] + 80 * c["nodes"] + 48 * c["triangles"] + 52 * c["instances_transformed"] + 4 * c["instances_identity"]
    return out


def set_samples_in_flight(ctx, count):
    """Samples per pixel rendered concurrently (1..4); results do not depend on it."""
    _dev_check(ctx, device_lib().rt_set_samples_in_flight(ctx, int(count)))


def set_profiling(ctx, enable):
    """False/0 off; True/1 per-stage events (serialised); 2 events around the trace launches only."""
    _dev_check(ctx, device_lib().rt_set_profiling(ctx, int(enable)))


SCHEDULER_MERGED, SCHEDULER_SLOTS = 0, 1


def set_scheduler(ctx, scheduler):
    """'merged' (default): consecutive submissions feed one wavefront; 'slots': one launch chain per submission,
    several in flight on their own streams (rt_set_scheduler)."""
    if isinstance(scheduler, str):
        scheduler = {"merged": SCHEDULER_MERGED, "slots": SCHEDULER_SLOTS}[scheduler]
    lib = device_lib()
    lib.rt_set_scheduler.argtypes = [c_void_p, c_int]
    _dev_check(ctx, lib.rt_set_scheduler(ctx, int(scheduler)))




def set_svgf_tiles(ctx, enable):
    """True (default): the a-trous passes of the SVGF filter stage a workgroup's taps in LDS; False: every tap is a global
    load (rt_set_svgf_tiles). Images are bit-identical."""
    lib = device_lib()
    lib.rt_set_svgf_tiles.argtypes = [c_void_p, c_int]
    _dev_check(ctx, lib.rt_set_svgf_tiles(ctx, 1 if enable else 0))


def set_frame_pipelining(ctx, enable):
    lib = device_lib()
    lib.rt_set_frame_pipelining.argtypes = [c_void_p, c_int]
    _dev_check(ctx, lib.rt_set_frame_pipelining(ctx, 1 if enable else 0))


def set_stream_batch(ctx, paths):
    """Paths the submissions of one iteration of the merged wavefront may bring (frame pipelining on); 0: the default of
    1920 x 1080 x 4. A burst of frames declared this way enters the wavefront together (rt_set_stream_batch)."""
    lib = device_lib()
    lib.rt_set_stream_batch.argtypes = [c_void_p, ctypes.c_longlong]
    _dev_check(ctx, lib.rt_set_stream_batch(ctx, int(paths)))


def advance(ctx):
    """One iteration of the merged wavefront without new samples (no-op when nothing is in flight)."""
    lib = device_lib()
    lib.rt_advance.argtypes = [c_void_p]
    _dev_check(ctx, lib.rt_advance(ctx))


def submissions_completed(ctx):
    lib = device_lib()
    lib.rt_submissions_completed.argtypes = [c_void_p, c_void_p]
    n = ctypes.c_uint64(0)
    _dev_check(ctx, lib.rt_submissions_completed(ctx, byref(n)))
    return int(n.value)


# kinds of rt_get_launch_timings (include/gpu_raytracer_amd.h, RT_TIMING_*)
TIMING_KINDS = {"trace": 0, "shadow": 1, "sort": 2, "generate": 3, "accumulate": 4, "material_diffuse": 5, "material_plastic": 6,
                "material_dielectric": 7, "material_conductor": 8, "svgf_reproject": 9, "svgf_variance": 10, "svgf_atrous": 11,
                "svgf_finalize": 12, "taa": 13, "taa_finalize": 14}


def launch_timings(ctx, kind=0):
    """Durations (ms) of the launches of one kind timed by set_profiling(ctx, 2 or 3) since the last call for that kind."""
    kind = TIMING_KINDS.get(kind, kind)
    lib = device_lib()
    lib.rt_get_launch_timings.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p]
    n = c_int(0)
    _dev_check(ctx, lib.rt_get_launch_timings(ctx, int(kind), None, 0, byref(n)))
    out = np.zeros(max(n.value, 1), np.float32)
    _dev_check(ctx, lib.rt_get_launch_timings(ctx, int(kind), out.ctypes.data, n.value, byref(n)))
    return out[:n.value]


def trace_statistics_history(ctx):
    """(rows, 10) uint64: the trace statistics after each iteration of the merged wavefront (cumulative)."""
    lib = device_lib()
    lib.rt_get_trace_statistics_history.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    n = c_int(0)
    _dev_check(ctx, lib.rt_get_trace_statistics_history(ctx, None, 0, byref(n)))
    out = np.zeros((max(n.value, 1), 10), np.uint64)
    _dev_check(ctx, lib.rt_get_trace_statistics_history(ctx, out.ctypes.data, n.value, byref(n)))
    return out[:n.value]


def algorithmic_bytes(row10):
    """SURVEY.md 8d bytes of ten trace-statistics counters {closest: nodes, triangles, transformed, identity, rays; shadow: same}."""
    r = [int(v) for v in row10]
    closest = 40 * r[4] + 80 * r[0] + 48 * r[1] + 52 * r[2] + 4 * r[3]
    shadow = 28 * r[9] + 80 * r[5] + 48 * r[6] + 52 * r[7] + 4 * r[8]
    return closest, shadow
