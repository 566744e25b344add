"""The kernel-level entry points ("probes") refuse a NULL context before any HIP work: RT_ERROR_INVALID_ARG, and rt_last_error(NULL)
is the entry point's own message (no GPU needed). Every other pointer is NULL and every count 0, except the capacity and frame_slots
of rt_sort_rays, rt_sort_rays_fog and rt_shade_rays, which are 1."""
import ctypes
from ctypes import c_float, c_int, c_size_t, c_uint32, c_void_p

import pytest

RT_ERROR_INVALID_ARG = -1
P, I, Z, U, F = c_void_p, c_int, c_size_t, c_uint32, c_float

# name -> (argument types after the context, their values, the message's text after "<name>: ")
PROBES = {
    "rt_trace_rays":               ([P] * 6 + [Z, P, I, P],                          [None] * 6 + [0, None, 0, None],                        "NULL argument"),
    "rt_trace_shadow_rays":        ([P] * 7 + [Z, P, I, P],                          [None] * 7 + [0, None, 0, None],                        "NULL argument"),
    "rt_trace_stream_rays":        ([I] + [P] * 6 + [Z, P] + [P] * 7 + [Z, P, P, P], [0] + [None] * 6 + [0, None] + [None] * 7 + [0, None, None, None], "NULL context"),
    "rt_trace_queue_rays":         ([I, I, I] + [P] * 6 + [Z, P] + [P] * 9 + [Z] + [P] * 3 + [Z, P, P], [0, 0, 0] + [None] * 6 + [0, None] + [None] * 9 + [0] + [None] * 3 + [0, None, None], "NULL context"),
    "rt_generate_rays":            ([I, I, I] + [P] * 7,                             [0, 0, 0] + [None] * 7,                                 "NULL argument"),
    "rt_generate_primary_rays":    ([I] * 14 + [P, Z] + [P] * 8,                     [0] * 14 + [None, 0] + [None] * 8,                      "NULL context"),
    "rt_random_samples":           ([I, P, Z, U, U, P],                              [0, None, 0, 0, 0, None],                               "invalid argument"),
    "rt_sample_texture":           ([I, I, P, Z, P],                                 [0, 0, None, 0, None],                                  "NULL argument"),
    "rt_sample_table":             ([P, I, I, I, I, P, Z, P],                        [None, 0, 0, 0, 0, None, 0, None],                      "NULL argument"),
    "rt_sample_sky":               ([P, Z, P],                                       [None, 0, None],                                        "NULL argument"),
    "rt_sample_sky_distribution":  ([P, Z, P],                                       [None, 0, None],                                        "NULL argument"),
    "rt_sky_pdf":                  ([P, Z, P],                                       [None, 0, None],                                        "NULL argument"),
    "rt_bsdf_eval":                ([I, P, Z, P],                                    [0, None, 0, None],                                     "NULL argument"),
    "rt_bsdf_sample":              ([I, P, Z, P],                                    [0, None, 0, None],                                     "NULL argument"),
    "rt_sample_lights":            ([P, Z, I, P],                                    [None, 0, 0, None],                                     "NULL argument"),
    "rt_perturb_normals":          ([I, P, Z, P],                                    [0, None, 0, None],                                     "NULL argument"),
    "rt_sort_rays":                ([I, I, I, P, Z, P, Z, P, Z, Z, U] + [P] * 9,     [0, 0, 0, None, 0, None, 0, None, 1, 1, 0] + [None] * 9, "NULL context"),
    "rt_shade_rays":               ([I, I, I, I, P, Z, P, Z, P, Z, Z, U] + [P] * 8,  [0, 0, 0, 0, None, 0, None, 0, None, 1, 1, 0] + [None] * 8, "NULL context"),
    "rt_measure_stream_bandwidth": ([Z, I, P],                                       [0, 0, None],                                           "invalid argument"),
    "rt_sort_rays_fog":            ([I, I, I, P, Z, P, Z, P, Z, Z, U] + [P] * 11,    [0, 0, 0, None, 0, None, 0, None, 1, 1, 0] + [None] * 11, "NULL context"),
    "rt_sample_delta_lights":      ([P, Z, P],                                       [None, 0, None],                                        "NULL argument"),
    "rt_fog_segments":             ([P, Z, P],                                       [None, 0, None],                                        "NULL context"),
    "rt_fog_density_segments":     ([P, Z, P],                                       [None, 0, None],                                        "NULL context"),
    "rt_attenuate_shadow_rays":    ([P, Z, P],                                       [None, 0, None],                                        "NULL context"),
    "rt_accumulate_frames":        ([I, P, P, Z, P, P, P, U, P],                     [0, None, None, 0, None, None, None, 0, None],          "NULL context"),
    "rt_accumulate_list_frames":   ([P, P, Z, P, P, P, P, Z, U, P],                  [None, None, 0, None, None, None, None, 0, 0, None],    "NULL context"),
    "rt_accumulate_cascade_frames": ([I, P, P, Z, P, P, P, P, Z, P, P, U, P],        [0, None, None, 0, None, None, None, None, 0, None, None, 0, None], "NULL context"),
    "rt_estimate_noise_images":    ([P, P, F, P, P, P, P, Z, P],                     [None, None, 0.0, None, None, None, None, 0, None],     "NULL context"),
    "rt_select_pixels_images":     ([P, P, F, F, I] + [P] * 5 + [Z, P, Z],           [None, None, 0.0, 0.0, 0] + [None] * 5 + [0, None, 0],  "NULL context"),
    "rt_denoise_images":           ([I, I, I] + [P] * 8 + [I, P],                    [0, 0, 0] + [None] * 8 + [0, None],                     "NULL context"),
    "rt_resolve_fireflies_images": ([I, I, I] + [P] * 5 + [I, P],                    [0, 0, 0] + [None] * 5 + [0, None],                     "NULL context"),
    "rt_measure_exposure_images":  ([I, I, I, P, P, P, P],                           [0, 0, 0, None, None, None, None],                      "NULL context"),
    "rt_estimate_noise_robust_images": ([P, P, P, F, F] + [P] * 5 + [Z, P, P],       [None, None, None, 0.0, 0.0] + [None] * 5 + [0, None, None], "NULL context"),
    "rt_select_pixels_robust_images": ([P, P, P, F, F, F, I] + [P] * 6 + [Z, P, Z],  [None, None, None, 0.0, 0.0, 0.0, 0] + [None] * 6 + [0, None, 0], "NULL context"),
}


@pytest.fixture(scope="module")
def lib(grt):
    lib = ctypes.CDLL(grt.DEVICE_LIB_PATH)
    lib.rt_last_error.restype = ctypes.c_char_p
    lib.rt_last_error.argtypes = [c_void_p]
    return lib


def test_there_are_thirty_four_probes():
    assert len(PROBES) == 34


@pytest.mark.parametrize("name", sorted(PROBES))
def test_a_null_context_is_refused_with_the_entry_points_own_message(lib, name):
    argtypes, values, message = PROBES[name]
    assert len(argtypes) == len(values)
    entry = getattr(lib, name)
    entry.restype = c_int
    entry.argtypes = [c_void_p] + argtypes
    assert entry(None, *values) == RT_ERROR_INVALID_ARG
    assert lib.rt_last_error(None).decode() == "%s: %s" % (name, message)
