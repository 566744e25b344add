"""The host side of the kernel-level entry points ("probes") on one Cornell-box context: refusals the host decides before any HIP work
(status, message text, output untouched), the empty batch of the nine entry points that return before allocating anything, and a render
afterwards. No call here launches a probe kernel. The refusals other tests pin (rt_sort_rays in test_gpu_sort.py, rt_shade_rays in
test_gpu_material.py -- here only its checks that need no queue entry --, the table checks of rt_upload_lights in test_gpu_nee.py) are not
repeated."""
import ctypes
from ctypes import byref, c_float, c_int32, c_size_t, c_void_p

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RT_OK, RT_ERROR_INVALID_ARG = 0, -1
SENTINEL = 0xFFC0DE42
BSDF_IN, NORMAL_IN = 24, 48   # floats per probe record of rt_bsdf_* and rt_perturb_normals


class TextureDesc(ctypes.Structure):   # rt_texture_desc
    _fields_ = [("texels", c_void_p), ("width", c_int32), ("height", c_int32), ("mip_levels", c_int32),
                ("lod_width", c_int32), ("lod_height", c_int32), ("format", c_int32), ("reserved", c_int32)]


def test_refusals_empty_batches_and_a_render_afterwards(grt):
    from conftest import make_pathtracer
    scene, pt = make_pathtracer(grt, "cornellbox", 64, 64, 0)
    lib, ctx = grt.device_lib(), pt.ctx
    lib.rt_upload_textures.argtypes = [c_void_p, c_void_p, c_size_t]
    # the Cornell box has no texture: one RGBA8 texture (which no material names) lets a call get past the index check
    texels = np.full((4, 4, 4), 128, np.uint8)
    desc = TextureDesc(texels.ctypes.data, 4, 4, 1, 0, 0, 0, 0)   # format 0: RT_TEXTURE_RGBA8
    assert lib.rt_upload_textures(ctx, byref(desc), 1) == RT_OK, lib.rt_last_error(ctx)

    out = np.full(64, SENTINEL, np.uint32)
    untouched = out.copy()
    zeros = np.zeros(64, np.float32)
    o, z = out.ctypes.data, zeros.ctypes.data
    gbps = c_float(-7.0)

    textured = np.zeros(BSDF_IN, np.float32); textured.view(np.int32)[3] = 5    # word 3 of a probe's material record: its texture id
    plain = np.zeros(BSDF_IN, np.float32); plain.view(np.int32)[3] = -1         # RT_INVALID
    ones = np.zeros(4, np.float32); ones[2] = 1.0
    filter3 = np.zeros(NORMAL_IN, np.float32); filter3[41] = 3.0
    bsdf_type = "material_type must be diffuse (1), plastic (2), dielectric (3) or conductor (4)"
    refusals = [
        (lambda: lib.rt_sample_texture(ctx, 1 << 20, 0, z, 1, o), "rt_sample_texture: texture index out of range"),
        (lambda: lib.rt_sample_texture(ctx, 0, 3, z, 1, o), "rt_sample_texture: filter must be 0 (level 0), 1 (lod) or 2 (gradients)"),
        (lambda: lib.rt_sample_table(ctx, z, 2, 1, 1, 4, z, 1, o), "rt_sample_table: dims must be 1, 2 or 3"),
        (lambda: lib.rt_sample_table(ctx, z, 0, 1, 1, 1, z, 1, o), "rt_sample_table: a table side is outside [1, 65536]"),
        (lambda: lib.rt_bsdf_eval(ctx, 0, plain.ctypes.data, 1, o), "rt_bsdf_eval: " + bsdf_type),
        (lambda: lib.rt_bsdf_sample(ctx, 0, plain.ctypes.data, 1, o), "rt_bsdf_sample: " + bsdf_type),
        (lambda: lib.rt_bsdf_eval(ctx, grt.MATERIAL_DIFFUSE, textured.ctypes.data, 1, o), "rt_bsdf_eval: probe 0 names texture 5 (only RT_INVALID is probed)"),
        (lambda: lib.rt_bsdf_sample(ctx, grt.MATERIAL_DIFFUSE, textured.ctypes.data, 1, o), "rt_bsdf_sample: probe 0 names texture 5 (only RT_INVALID is probed)"),
        (lambda: lib.rt_sample_lights(ctx, z, 1, 2, o), "rt_sample_lights: use_lds must be 0 (global memory) or 1 (as the shade kernels choose)"),
        (lambda: lib.rt_sample_lights(ctx, ones.ctypes.data, 1, 1, o), "rt_sample_lights: probe 0: random number 2 is 1, outside [0, 1)"),
        (lambda: lib.rt_perturb_normals(ctx, 1 << 20, z, 1, o), "rt_perturb_normals: texture index out of range"),
        (lambda: lib.rt_perturb_normals(ctx, 0, filter3.ctypes.data, 1, o), "rt_perturb_normals: filter must be 0 (level 0), 1 (lod) or 2 (gradients)"),
        (lambda: lib.rt_trace_stream_rays(ctx, -1, *[None] * 6, 0, o, *[None] * 7, 0, o, o, o), "rt_trace_stream_rays: negative iteration"),
        (lambda: lib.rt_trace_stream_rays(ctx, 0, *[None] * 6, 0, o, *[None] * 7, 0, o, o, None), "rt_trace_stream_rays: NULL info"),
        (lambda: lib.rt_trace_stream_rays(ctx, 0, *[None] * 6, 3, o, *[None] * 7, 0, o, o, o), "rt_trace_stream_rays: NULL closest-hit ray or hit array"),
        (lambda: lib.rt_generate_rays(ctx, 0, 0, -1, *[o] * 7), "rt_generate_rays: negative pixel_count"),
        (lambda: lib.rt_generate_primary_rays(ctx, 1, 0, 0, 17, 0, 1, 0, 0, 0, 0, 0, 0, -1, -1, None, 64, *[o] * 8), "rt_generate_primary_rays: sample_count must be 1..16"),
        (lambda: lib.rt_random_samples(ctx, 7, z, 1, 0, 0, o), "rt_random_samples: invalid argument"),
        (lambda: lib.rt_measure_stream_bandwidth(ctx, 512, 1, byref(gbps)), "rt_measure_stream_bandwidth: invalid argument"),
        (lambda: lib.rt_shade_rays(ctx, 2, 0, 0, 0, None, 0, None, 0, None, 1, 1, SENTINEL, *[o] * 7, None), "rt_shade_rays: merged must be 0 (per-bounce launch) or 1 (merged wavefront)"),
        (lambda: lib.rt_shade_rays(ctx, 0, 0, 0, 4, None, 0, None, 0, None, 1, 1, SENTINEL, *[o] * 7, None), "rt_shade_rays: material_slot must be 0 (diffuse), 1 (plastic), 2 (dielectric) or 3 (conductor)"),
        (lambda: lib.rt_shade_rays(ctx, 0, 0, 0, 0, None, 0, None, 0, None, 1, 1, SENTINEL, o, None, *[o] * 5, None), "rt_shade_rays: NULL array"),
        (lambda: lib.rt_shade_rays(ctx, 1, 0, 0, 0, None, 0, None, 0, None, 1, 1, SENTINEL, *[o] * 7, None), "rt_shade_rays: NULL slot table, submission births or statistics (merged form)"),
        (lambda: lib.rt_shade_rays(ctx, 0, 127, 0, 0, None, 0, None, 0, None, 1, 1, SENTINEL, *[o] * 7, None), "rt_shade_rays: bounce outside [0, RT_MAX_BOUNCES - 1)"),
        (lambda: lib.rt_shade_rays(ctx, 0, 0, 0, 0, None, 0, None, 0, None, 0, 1, SENTINEL, *[o] * 7, None), "rt_shade_rays: capacity must be in [1, 2^28]"),
    ]
    for call, message in refusals:
        assert call() == RT_ERROR_INVALID_ARG, message
        assert lib.rt_last_error(ctx).decode() == message
        assert np.array_equal(out, untouched) and gbps.value == -7.0, message

    # the empty batch: RT_OK before anything is allocated (the Cornell box has what the sky and light probes look for first: the host
    # classes give a scene without a sky file a constant white one, and its ceiling light is in the light tables)
    empty = [
        lambda: lib.rt_sample_texture(ctx, 0, 0, z, 0, o),
        lambda: lib.rt_sample_table(ctx, z, 2, 1, 1, 1, z, 0, o),
        lambda: lib.rt_sample_sky(ctx, z, 0, o),
        lambda: lib.rt_sample_sky_distribution(ctx, z, 0, o),
        lambda: lib.rt_sky_pdf(ctx, z, 0, o),
        lambda: lib.rt_bsdf_eval(ctx, grt.MATERIAL_DIFFUSE, plain.ctypes.data, 0, o),
        lambda: lib.rt_bsdf_sample(ctx, grt.MATERIAL_DIFFUSE, plain.ctypes.data, 0, o),
        lambda: lib.rt_sample_lights(ctx, z, 0, 1, o),
        lambda: lib.rt_perturb_normals(ctx, 0, z, 0, o),
    ]
    for index, call in enumerate(empty):
        assert call() == RT_OK, (index, lib.rt_last_error(ctx))
        assert np.array_equal(out, untouched), index

    # a refused call leaves the context usable
    pt.update(); pt.render()
    assert np.isfinite(pt.read_framebuffer()).all()
    pt.close(); scene.close()
