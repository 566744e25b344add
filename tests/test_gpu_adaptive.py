"""Adaptive sampling on the MI355X: kernel_select_cells / kernel_scan_cells / kernel_compact_cells through rt_select_pixels_images,
kernel_accumulate_group_list_moments through rt_accumulate_list_frames, and the whole path -- rt_select_active_cells, rt_set_pixel_list, list submissions of the
merged wavefront, Pathtracer.render_until(adaptive=True) and the command line. The oracle does not know the feature: everything is pinned bit for bit against
the numpy restatement of adaptive_reference.py, against the float32 replay of the fold, and against uniform rendering of the same sample indices."""
import ctypes
import re
import subprocess
from ctypes import byref, c_float, c_int, c_void_p

import numpy as np
import pytest

import adaptive_cases as cases
import adaptive_reference as ref
import noise_cases
import noise_checks as checks
import noise_reference as noise

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
RT_ACCUMULATE_GROUP = 8
SENTINEL = noise_cases.SENTINEL
LIST_SENTINEL = 0xfffffff0


def _bare_context(grt, width, height, pitch):
    lib = grt.device_lib()
    lib.rt_resize.argtypes = [c_void_p, c_int, c_int]
    ctx = c_void_p()
    assert lib.rt_create(0, byref(ctx)) == 0, lib.rt_last_error(None)
    assert lib.rt_resize(ctx, width, height) == 0, lib.rt_last_error(ctx)
    assert lib.rt_screen_pitch(ctx) == pitch
    return ctx


@pytest.fixture(scope="module")
def contexts(grt):
    """One bare context per probe frame: rt_create + rt_resize, no scene (selection and accumulate launches need none)."""
    made = {name: _bare_context(grt, *frame) for name, frame in cases.FRAMES.items()}
    yield made
    for ctx in made.values():
        grt.device_lib().rt_destroy(ctx)


# ---- selection probe ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", list(cases.FRAMES))
def test_selection_probe_against_the_restatement(grt, contexts, frame):
    """Every case on one frame: cell arrays, flags, counts and every list entry bit for bit; what lies behind the list keeps the caller's sentinel; a second run
    gives the same bytes."""
    width, height, pitch = cases.FRAMES[frame]
    for name in cases.SELECTION_CASES:
        mean, moments, threshold, dilate = cases.selection_case(frame, name)
        want = noise.estimate(mean, moments, width, cases.FLOOR)
        hot, active = ref.select(want["cell_sums"], want["cell_counts"], want["cell_nonfinite"], width, height, threshold, dilate)
        pixels = ref.pixel_list(active, width, height)
        runs = [grt.select_pixels_images(contexts[frame], height, width, pitch, mean, moments, threshold, floor=cases.FLOOR, dilate=dilate, sentinel=LIST_SENTINEL) for _ in range(2)]
        got = runs[0]
        assert (got["cells_x"], got["cells_y"]) == ref.cell_grid(width, height), name
        checks.assert_same_bits(got["cell_sums"], want["cell_sums"], name + ": cell sums")
        assert np.array_equal(got["cell_counts"], want["cell_counts"]) and np.array_equal(got["cell_nonfinite"], want["cell_nonfinite"]), name
        assert np.array_equal(got["hot"], hot) and np.array_equal(got["active"], active), (name, got["hot"], hot, got["active"], active)
        assert got["hot_cells"] == hot.sum() and got["active_cells"] == active.sum() and got["list_pixels"] == len(pixels), name
        assert np.array_equal(got["list"], pixels), name
        assert (got["list_tail"] == LIST_SENTINEL).all() and len(got["list"]) + len(got["list_tail"]) == width * height, name
        for key in ("cell_sums", "cell_counts", "cell_nonfinite", "hot", "active", "list", "list_tail"):
            assert runs[0][key].tobytes() == runs[1][key].tobytes(), (name, key)
        cells = hot.size
        if name == "on_threshold":
            assert not hot.any() and got["list_pixels"] == 0                     # sum == threshold * count is not hot: the empty list
        elif name == "threshold_one_ulp_below":
            assert hot.all() and got["list_pixels"] == width * height           # ... one float32 ulp of the threshold further down it is
        elif name == "just_above":
            assert hot.ravel().tolist() == [False] * (cells - 1) + [True]        # a sum just above threshold * count is
        elif name == "every_cell_hot":
            assert hot.all() and np.array_equal(np.sort(got["list"]), np.arange(width * height))
        elif name == "nonfinite_cell":
            assert not hot.ravel()[0] and hot.sum() == cells - 1
        elif name == "unsampled_pixels":
            assert hot.ravel().tolist() == [False] * (cells - 1) + [True]
        elif name.startswith("hot_corner"):
            grid = ref.cell_grid(width, height)
            assert hot.sum() == 1 and active.sum() == (min(2, grid[0]) * min(2, grid[1]) if dilate else 1)


def test_selection_refusals(grt, contexts):
    frame = "40x24"
    width, height, pitch = cases.FRAMES[frame]
    ctx = contexts[frame]
    mean, moments = cases.images(frame)
    status = lambda call: pytest.raises(grt.DeviceRefusal, call).value.status
    for threshold in (-1.0, float("nan"), float("inf")):
        assert status(lambda: grt.select_pixels_images(ctx, height, width, pitch, mean, moments, threshold)) == RT_ERROR_INVALID_ARG
    for dilate in (-1, 2):
        assert status(lambda: grt.select_pixels_images(ctx, height, width, pitch, mean, moments, 0.5, dilate=dilate)) == RT_ERROR_INVALID_ARG
    for floor in (0.0, float("nan")):
        assert status(lambda: grt.select_pixels_images(ctx, height, width, pitch, mean, moments, 0.5, floor=floor)) == RT_ERROR_INVALID_ARG
    assert status(lambda: grt.select_active_cells(ctx, height, width, 0.5)) == RT_ERROR_NOT_READY      # the estimate is off
    assert status(lambda: grt.read_pixel_list(ctx)) == RT_ERROR_NOT_READY
    assert status(lambda: grt.set_pixel_list(ctx, True)) == RT_ERROR_INVALID_ARG                       # no selection exists
    lib = grt.device_lib()
    record = grt.CellSelectionRecord()
    assert lib.rt_select_active_cells(None, c_float(1e-2), c_float(0.5), 1, byref(record), None, 0) == RT_ERROR_INVALID_ARG
    assert b"rt_select_active_cells: NULL context" in lib.rt_last_error(None)
    assert lib.rt_set_pixel_list(None, 1) == RT_ERROR_INVALID_ARG and lib.rt_get_pixel_list(None) == 0


# ---- accumulate probe ---------------------------------------------------------------------------------------------------------------------------

ACC_FRAME = "40x24"
GROUPS = {"one_of_1": [1], "one_of_16": [16], "two": [3, 16], "eight": [1, 2, 3, 4, 5, 6, 7, 16]}
assert len(GROUPS["eight"]) == RT_ACCUMULATE_GROUP


@pytest.fixture(scope="module")
def accumulate_inputs():
    """44 sample frames with every kind of stream (noise_cases) and a start state in which the pixels' own counts are 0, 1, 2 and 255, scan position by scan position."""
    width, height, pitch = noise_cases.FRAMES[ACC_FRAME]
    frames, kinds = noise_cases.sample_frames(ACC_FRAME, 44 + 3, seed=11)
    zero = np.zeros(frames.shape[1:], np.float32)
    acc, m2, _ = noise.accumulate(frames[:3], zero, zero, 0)              # w = 2 everywhere
    count = np.full((height, pitch), -1, np.int32)
    count[:, :width] = np.array([0, 1, 2, 255])[(np.arange(width)[None, :] + np.arange(height)[:, None]) % 4]
    acc[count == 0] = 0; m2[count == 0] = 0
    m2[count == 1] = np.array([0, 0, 0, 1], np.float32)
    m2[count == 255, 3] = 255
    acc.view(np.uint32)[:, width:] = SENTINEL; m2.view(np.uint32)[:, width:] = SENTINEL
    frames = frames[3:].copy()
    for a in (frames, acc, m2):
        a.setflags(write=False)
    order = np.random.default_rng(5).permutation(width * height).astype(np.uint32)
    return frames, acc, m2, count, order


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("length", [1, 63, 64, 65, "all"])
def test_list_accumulate_probe_against_the_replay(grt, contexts, accumulate_inputs, group, length):
    width, height, pitch = cases.FRAMES[ACC_FRAME]
    frames, acc, m2, count, order = accumulate_inputs
    counts = GROUPS[group]
    given = frames[:sum(counts)]
    pixels = order if length == "all" else order[7:7 + length]
    assert set(count[pixels // width, pixels % width].tolist()) == ({0, 1, 2, 255} if len(pixels) > 1 else {int(count[pixels[0] // width, pixels[0] % width])})
    got_frames, got_acc, got_m2, got_final = grt.accumulate_list_frames(contexts[ACC_FRAME], given, acc, m2, pixels, counts, first_sample=[40 + k for k in range(len(counts))], sentinel=SENTINEL)
    want_frames, want_acc, want_m2, written, want_final = ref.accumulate_list(given, acc, m2, pixels, width, counts)
    assert written.sum() == len(pixels) and not written[:, width:].any()
    checks.assert_same_bits(got_acc, want_acc, "accumulator"); checks.assert_same_bits(got_m2, want_m2, "moments"); checks.assert_same_bits(got_frames, want_frames, "sample frames")
    sentinel = noise_cases.sentinel_image(ACC_FRAME)
    checks.assert_same_bits(got_final, np.where(written[..., None], want_final, sentinel), "final image")
    # outside the list, padding columns included: what the caller gave
    assert np.array_equal(got_acc.view(np.uint32)[~written], acc.view(np.uint32)[~written]) and np.array_equal(got_m2.view(np.uint32)[~written], m2.view(np.uint32)[~written])
    assert np.array_equal(got_frames.view(np.uint32)[:, ~written], given.view(np.uint32)[:, ~written]) and (got_final.view(np.uint32)[~written] == SENTINEL).all()
    assert (got_m2[written][:, 3] == np.maximum(count[written], 0) + sum(counts)).all()     # every pixel's own count went on
    if sum(counts) == 1:
        fresh = written & (count == 0)
        assert np.array_equal(got_acc.view(np.uint32)[fresh], given[0].view(np.uint32)[fresh]) and (got_m2[fresh] == np.array([0, 0, 0, 1], np.float32)).all()


def test_list_accumulate_probe_refusals(grt, contexts, accumulate_inputs):
    width, height, pitch = cases.FRAMES[ACC_FRAME]
    frames, acc, m2, count, order = accumulate_inputs
    ctx = contexts[ACC_FRAME]
    refusal = lambda pixels, counts=(1,): pytest.raises(grt.DeviceRefusal, lambda: grt.accumulate_list_frames(ctx, frames[:sum(counts)], acc, m2, np.array(pixels, np.uint32), list(counts))).value
    twice = refusal([5, 9, 5])
    assert twice.status == RT_ERROR_INVALID_ARG and "second time" in str(twice)
    outside = refusal([5, width * height])
    assert outside.status == RT_ERROR_INVALID_ARG and "outside" in str(outside)
    assert refusal([]).status == RT_ERROR_INVALID_ARG
    assert refusal([1], counts=(1,) * 9).status == RT_ERROR_INVALID_ARG
    lib = grt.device_lib()
    one = np.zeros(4, np.int32)
    assert lib.rt_accumulate_list_frames(None, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, one.ctypes.data) == RT_ERROR_INVALID_ARG
    assert b"rt_accumulate_list_frames: NULL context" in lib.rt_last_error(None)


# ---- the whole path: two contexts per scene, uniform samples 0 .. 15 first -----------------------------------------------------------------------

W, H, WARM = 96, 64, 16
FLOOR_UNDER_THE_QUAD = ('<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><scale value="30"/><translate y="-0.5"/></transform>'
                        '<bsdf type="diffuse"><rgb name="reflectance" value="0.6, 0.6, 0.6"/></bsdf></shape>')


def _mapped_quad_scene(directory):
    """The normal-mapped quad under an area emitter of test_gpu_normal_maps.py (rough plastic), over a diffuse floor so that every pixel sees a lit surface."""
    import normal_map_reference
    import test_gpu_normal_maps as quad
    normal_map_reference.write_tga(str(directory / "n.tga"), normal_map_reference.random_normal_map(3, 16, 16))
    bsdf = '<bsdf type="normalmap"><texture name="normalmap" type="bitmap"><string name="filename" value="n.tga"/></texture>%s</bsdf>' % quad.MODELS["plastic"]
    return quad._quad_scene(directory, "adaptive", bsdf, (0.0, 1.0, 0.0), extra=FLOOR_UNDER_THE_QUAD)


@pytest.fixture(scope="module", params=["cornellbox", "mapped_quad"])
def pair(grt, request, tmp_path_factory):
    """(scene, path tracer a, path tracer b) at 96 x 64, 3 bounces, next-event estimation on."""
    grt.config_reset()
    path = grt.scene_path("cornellbox") if request.param == "cornellbox" else _mapped_quad_scene(tmp_path_factory.mktemp("adaptive"))
    scene = grt.Scene(path)
    grt.config_set(num_bounces=3, enable_next_event_estimation=1, enable_multiple_importance_sampling=1)
    tracers = [grt.Pathtracer(scene, W, H, device=0) for _ in range(2)]
    for pt in tracers:   # all four AOVs the accumulate step folds
        for aov in (grt.AOV_ALBEDO, grt.AOV_NORMAL, grt.AOV_POSITION):
            pt.aov_enable(aov)
    lib = grt.device_lib()
    lib.rt_render_samples.argtypes = [c_void_p, c_int, c_int]
    yield scene, tracers[0], tracers[1]
    for pt in tracers:
        pt.close()
    scene.close(); grt.config_reset()


def _render(grt, pt, first, count):
    assert grt.device_lib().rt_render_samples(pt.ctx, first, count) == 0, grt.device_lib().rt_last_error(pt.ctx)


def _warm_up(grt, pt):
    """Samples 0 .. 15, uniform; the progression starts over (and every earlier list is gone)."""
    if grt.get_pixel_list(pt.ctx):
        grt.set_pixel_list(pt.ctx, False)
    grt.set_scheduler(pt.ctx, "merged"); grt.set_frame_pipelining(pt.ctx, False); grt.set_stream_batch(pt.ctx, 0)
    pt.set_noise_estimate(True); pt.invalidate("gpu_config"); pt.update()
    assert pt.sample_index == 0 and grt.get_noise_estimate(pt.ctx)
    _render(grt, pt, 0, 1)
    for first in (1, 5, 9, 13):
        _render(grt, pt, first, min(4, WARM - first))


STATE = ("mean", "moments", "final image", "albedo mean", "normal mean", "position mean")


def _state(grt, pt):
    return (pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, H, pt.pitch), pt.read_framebuffer().copy(),
            pt.read_aov(grt.AOV_ALBEDO).copy(), pt.read_aov(grt.AOV_NORMAL).copy(), pt.read_aov(grt.AOV_POSITION).copy())


def _passes(grt, pt, mode):
    """Passes 16 .. 23 over whatever pixel set the context has."""
    if mode == "burst":
        grt.set_frame_pipelining(pt.ctx, True); grt.set_stream_batch(pt.ctx, 2 * 4 * W * H)
    try:
        for first in range(WARM, WARM + 8, 1 if mode == "single" else 4):
            _render(grt, pt, first, 1 if mode == "single" else 4)
    finally:
        if mode == "burst":
            grt.set_frame_pipelining(pt.ctx, False); grt.set_stream_batch(pt.ctx, 0)


@pytest.mark.parametrize("mode", ["single", "batches_of_4", "burst"])
def test_threshold_0_list_renders_what_uniform_renders(grt, pair, mode):
    scene, a, b = pair
    for pt in (a, b):
        _warm_up(grt, pt)
    for got, want, what in zip(_state(grt, a), _state(grt, b), STATE):
        checks.assert_same_bits(got, want, what + " after the warm-up")
    chosen = grt.select_active_cells(a.ctx, H, W, 0.0, floor=grt.config_get("noise_floor"), dilate=1)
    try:
        assert chosen["active"].all() and chosen["list_pixels"] == W * H, chosen
        assert np.array_equal(grt.read_pixel_list(a.ctx), ref.pixel_list(chosen["active"], W, H))
        grt.set_pixel_list(a.ctx, True)
        assert grt.get_pixel_list(a.ctx) and not grt.get_pixel_list(b.ctx)
        _passes(grt, a, mode); _passes(grt, b, mode)
        for got, want, what in zip(_state(grt, a), _state(grt, b), STATE):
            checks.assert_same_bits(got, want, what)
        assert (_state(grt, a)[1][:, :W, 3] == WARM + 7).all()
    finally:
        grt.set_pixel_list(a.ctx, False)


def test_median_threshold_renders_the_list_and_leaves_the_rest(grt, pair):
    scene, a, b = pair
    for pt in (a, b):
        _warm_up(grt, pt)
    before = _state(grt, a)
    floor = grt.config_get("noise_floor")
    estimate = grt.estimate_noise(a.ctx, H, W, a.pitch, floor=floor, want_map=False)
    assert (estimate["cell_counts"] == 256).all()
    threshold = float(np.float32(np.median(estimate["cell_sums"] / estimate["cell_counts"])))
    chosen = grt.select_active_cells(a.ctx, H, W, threshold, floor=floor, dilate=0)
    hot, active = ref.select(estimate["cell_sums"], estimate["cell_counts"], estimate["cell_nonfinite"], W, H, threshold, 0)
    assert 0 < chosen["active_cells"] < active.size, chosen            # at least one cell is active and at least one is not
    assert np.array_equal(chosen["hot"], hot) and np.array_equal(chosen["active"], active)
    pixels = grt.read_pixel_list(a.ctx)
    assert np.array_equal(pixels, ref.pixel_list(active, W, H)) and len(pixels) == chosen["list_pixels"] == 256 * active.sum()
    grt.set_pixel_list(a.ctx, True)
    try:
        _passes(grt, a, "batches_of_4"); _passes(grt, b, "batches_of_4")
    finally:
        grt.set_pixel_list(a.ctx, False)
    listed = np.zeros((H, a.pitch), bool); listed[pixels // W, pixels % W] = True
    inside = np.zeros((H, a.pitch), bool); inside[:, :W] = True
    assert all(np.abs(image[:, :W, :3]).max() > 0 for image in before[3:])                              # the other three AOVs are being written
    for got, uniform, old, what in zip(_state(grt, a), _state(grt, b), before, STATE):
        checks.assert_same_bits(got[listed], uniform[listed], what + " of the listed pixels")
        checks.assert_same_bits(got[~listed], old[~listed], what + " of the other pixels")
    moments = _state(grt, a)[1]
    assert (moments[listed][:, 3] == WARM + 7).all() and (moments[inside & ~listed][:, 3] == WARM - 1).all()
    counts, mean = a.sample_counts()
    assert np.array_equal(counts, moments[..., 3]) and mean == pytest.approx((23 * listed.sum() + 15 * (W * H - listed.sum())) / (W * H), rel=1e-12)
    assert np.array_equal(a.sample_count_map(), counts)


def test_refusals_leave_the_context_rendering_uniformly(grt, pair):
    scene, a, b = pair
    lib = grt.device_lib()
    lib.rt_set_pixel_range.argtypes = [c_void_p, c_int, c_int]
    lib.rt_render_ao_sample.argtypes = [c_void_p, c_int, c_float]
    for pt in (a, b):
        _warm_up(grt, pt)
    floor = grt.config_get("noise_floor")
    status = lambda call: pytest.raises(grt.DeviceRefusal, call).value.status
    refused = lambda code, needle: code == RT_ERROR_INVALID_ARG and needle in lib.rt_last_error(a.ctx).decode()
    assert status(lambda: grt.set_pixel_list(a.ctx, True)) == RT_ERROR_INVALID_ARG                       # no selection since the restart
    for threshold, dilate in ((float("nan"), 1), (-0.5, 1), (float("inf"), 0), (0.5, 2), (0.5, -1)):
        assert status(lambda: grt.select_active_cells(a.ctx, H, W, threshold, floor=floor, dilate=dilate)) == RT_ERROR_INVALID_ARG
    assert status(lambda: grt.select_active_cells(a.ctx, H, W, 0.5, floor=floor, cell_capacity=5)) == RT_ERROR_INVALID_ARG
    empty = grt.select_active_cells(a.ctx, H, W, 1e30, floor=floor)
    assert empty["list_pixels"] == 0 and empty["hot_cells"] == 0 and len(grt.read_pixel_list(a.ctx)) == 0
    assert status(lambda: grt.set_pixel_list(a.ctx, True)) == RT_ERROR_INVALID_ARG and "empty" in lib.rt_last_error(a.ctx).decode()
    assert grt.select_active_cells(a.ctx, H, W, 0.0, floor=floor)["list_pixels"] > 0
    grt.set_pixel_list(a.ctx, True)
    try:
        assert refused(lib.rt_render_samples(a.ctx, 0, 1), "below 2") and refused(lib.rt_render_samples(a.ctx, 1, 4), "below 2")
        assert refused(lib.rt_render_ao_sample(a.ctx, WARM, 1.0), "AO integrator")
        blank = np.zeros((1, H, a.pitch, 4), np.float32)
        assert status(lambda: grt.accumulate_frames(a.ctx, blank, blank[0], blank[0], WARM)) == RT_ERROR_INVALID_ARG          # the uniform probe does not cover a list
        grt.set_scheduler(a.ctx, "slots")
        assert refused(lib.rt_render_samples(a.ctx, WARM, 1), "RT_SCHEDULER_MERGED")
        grt.set_scheduler(a.ctx, "merged")
        assert lib.rt_set_batch_size(a.ctx, 1024) == 0                                                    # explicit pixel batches: the merged wavefront is not taken
        assert refused(lib.rt_render_samples(a.ctx, WARM, 1), "does not take")
        assert lib.rt_set_batch_size(a.ctx, 0) == 0
        assert grt.get_pixel_list(a.ctx)                                                                  # a refusal does not switch the list off by itself
    finally:
        grt.set_scheduler(a.ctx, "merged")
        assert lib.rt_set_batch_size(a.ctx, 0) == 0
        grt.set_pixel_list(a.ctx, False)
    _passes(grt, a, "batches_of_4"); _passes(grt, b, "batches_of_4")
    for got, want, what in zip(_state(grt, a), _state(grt, b), STATE):
        checks.assert_same_bits(got, want, what + ", uniform after the refusals")
    # a pixel range or a tile split: no selection, no list (both zero the moments and drop the selection)
    assert grt.select_active_cells(a.ctx, H, W, 0.0, floor=floor)["list_pixels"] > 0
    try:
        assert lib.rt_set_pixel_range(a.ctx, W, 10 * W) == 0
        assert not grt.get_pixel_list(a.ctx) and status(lambda: grt.read_pixel_list(a.ctx)) == RT_ERROR_NOT_READY          # dropped with the moments
        assert status(lambda: grt.select_active_cells(a.ctx, H, W, 0.0, floor=floor)) == RT_ERROR_INVALID_ARG and "pixel range" in lib.rt_last_error(a.ctx).decode()
        assert status(lambda: grt.set_pixel_list(a.ctx, True)) == RT_ERROR_INVALID_ARG
        assert lib.rt_set_pixel_tiles(a.ctx, 8 * W, 0, 2) == 0
        assert status(lambda: grt.set_pixel_list(a.ctx, True)) == RT_ERROR_INVALID_ARG and "no selection" in lib.rt_last_error(a.ctx).decode()   # none can exist under a pixel set
        assert status(lambda: grt.select_active_cells(a.ctx, H, W, 0.0, floor=floor)) == RT_ERROR_INVALID_ARG and "tile split" in lib.rt_last_error(a.ctx).decode()
    finally:
        assert lib.rt_set_pixel_range(a.ctx, 0, -1) == 0
    _render(grt, a, WARM + 8, 4); _render(grt, b, WARM + 8, 4)
    for got, want, what in [row for row in zip(_state(grt, a), _state(grt, b), STATE) if row[2] != "moments"]:   # (a's moments started over with the pixel sets)
        checks.assert_same_bits(got, want, what + ", uniform after the pixel sets")
    # switching the estimate off frees the list
    grt.set_noise_estimate(a.ctx, False)
    assert status(lambda: grt.read_pixel_list(a.ctx)) == RT_ERROR_NOT_READY and status(lambda: grt.select_active_cells(a.ctx, H, W, 0.0, floor=floor)) == RT_ERROR_NOT_READY


def test_svgf_refuses_a_list_that_exists(grt, pair):
    """SVGF switched on through the config after a selection was made and the list switched on: render calls are refused, and so is switching the list on again."""
    scene, a, b = pair
    lib = grt.device_lib()
    _warm_up(grt, a)
    assert grt.select_active_cells(a.ctx, H, W, 0.0, floor=grt.config_get("noise_floor"))["list_pixels"] > 0
    grt.set_pixel_list(a.ctx, True)
    try:
        grt.config_set(enable_svgf=1); a.invalidate("gpu_config"); a.update()
        assert grt.get_pixel_list(a.ctx)
        assert lib.rt_render_samples(a.ctx, WARM, 1) == RT_ERROR_INVALID_ARG and "SVGF frames cannot cover a pixel list" in lib.rt_last_error(a.ctx).decode()
        grt.set_pixel_list(a.ctx, False)
        refusal = pytest.raises(grt.DeviceRefusal, lambda: grt.set_pixel_list(a.ctx, True)).value
        assert refusal.status == RT_ERROR_INVALID_ARG and "rt_set_pixel_list: SVGF is on" in str(refusal)
    finally:
        if grt.get_pixel_list(a.ctx):
            grt.set_pixel_list(a.ctx, False)
        grt.config_set(enable_svgf=0); a.invalidate("gpu_config"); a.update()
    for pt in (a, b):
        _warm_up(grt, pt)
    _passes(grt, a, "batches_of_4"); _passes(grt, b, "batches_of_4")
    for got, want, what in zip(_state(grt, a), _state(grt, b), STATE):
        checks.assert_same_bits(got, want, what + ", uniform after the refusals")


def test_a_restart_drops_the_list(grt, pair):
    scene, a, b = pair
    _warm_up(grt, a)
    chosen = a.select_adaptive(0.0)
    assert chosen["list_pixels"] > 0 and grt.get_pixel_list(a.ctx)
    a.invalidate("gpu_config"); a.update()
    assert a.sample_index == 0
    a.render()
    assert not grt.get_pixel_list(a.ctx)
    assert (grt.read_noise_moments(a.ctx, H, a.pitch)[:, :W] == np.array([0, 0, 0, 1], np.float32)).all()
    a.update(); a.render_samples(4)
    assert (grt.read_noise_moments(a.ctx, H, a.pitch)[:, :W, 3] == 4).all()


def test_svgf_contexts_refuse_selection(grt):
    from conftest import make_pathtracer
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, enable_svgf=1)
    try:
        grt.set_noise_estimate(pt.ctx, True)
        refusal = pytest.raises(grt.DeviceRefusal, lambda: grt.select_active_cells(pt.ctx, H, W, 0.0)).value
        assert refusal.status == RT_ERROR_INVALID_ARG and "SVGF" in str(refusal)
        with pytest.raises(ValueError, match="SVGF"):
            pt.render_until(0.1, 8, adaptive=True)
    finally:
        pt.close(); scene.close(); grt.config_reset()


# ---- a scene whose upper half sees only a constant sky ----------------------------------------------------------------------------------------------

SKY_W, SKY_H = 96, 96
SKY_SCENE = ('<scene version="0.5.0"><integrator type="path"><integer name="maxDepth" value="3"/></integrator>'
             '<sensor type="perspective"><float name="fov" value="50"/><transform name="toWorld"><lookat origin="0, 1, 6" target="0, 1, 0" up="0, 1, 0"/></transform></sensor>'
             '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><scale value="5"/></transform><bsdf type="diffuse"><rgb name="reflectance" value="0.7, 0.6, 0.5"/></bsdf></shape>'
             '<shape type="cube"><transform name="toWorld"><scale value="0.4"/><translate x="-0.8" y="0.4" z="1"/></transform><bsdf type="diffuse"><rgb name="reflectance" value="0.3, 0.5, 0.8"/></bsdf></shape>'
             '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="90"/><scale value="0.3"/><translate x="0.8" y="0.9" z="2"/></transform>'
             '<emitter type="area"><rgb name="radiance" value="15, 14, 12"/></emitter></shape></scene>')


def test_constant_sky_cells_are_never_selected(grt, tmp_path):
    """Everything the camera sees lies below its own height: one half of the frame is sky. Sky cells two cells away from geometry keep M2 = 0 and the count of the
    uniform warm-up; every cell with a noisy pixel is rendered to the cap."""
    (tmp_path / "sky.xml").write_text(SKY_SCENE)
    grt.config_reset()
    scene = grt.Scene(str(tmp_path / "sky.xml"))
    grt.config_set(num_bounces=3, enable_next_event_estimation=1, enable_multiple_importance_sampling=1, noise_min_samples=16)
    pt = grt.Pathtracer(scene, SKY_W, SKY_H, device=0)
    try:
        result = pt.render_until(1e-8, 48, check_every=16, adaptive=True)
        print("render_until(adaptive):", result)
        assert not grt.get_pixel_list(pt.ctx)                                      # render_until switches the list off when it returns
        acc, moments = pt.read_aov(grt.AOV_RADIANCE)[:, :SKY_W], grt.read_noise_moments(pt.ctx, SKY_H, pt.pitch)[:, :SKY_W]
        noisy = (moments[..., :3] != 0).any(-1)
        halves = [noisy[:SKY_H // 2], noisy[SKY_H // 2:]]
        sky_half = 0 if not halves[0].any() else 1
        assert not halves[sky_half].any() and halves[1 - sky_half].any(), "one half of the frame must be sky"
        rows = slice(0, SKY_H // 2) if sky_half == 0 else slice(SKY_H // 2, SKY_H)
        assert (acc[rows][..., :3] == acc[rows][0, 0, :3]).all() and (moments[rows][..., :3] == 0).all()
        far = slice(0, SKY_H // 2 - 32) if sky_half == 0 else slice(SKY_H // 2 + 32, SKY_H)   # the sky cells at least two cells away from the other half
        w = moments[..., 3]
        assert w[far].size == 16 * SKY_W and (w[far] == 15).all()                  # never selected: noise_min_samples - 1
        noisy_cells = noisy.reshape(SKY_H // 16, 16, SKY_W // 16, 16).any(axis=(1, 3))
        cell_w = w.reshape(SKY_H // 16, 16, SKY_W // 16, 16).transpose(0, 2, 1, 3)
        assert noisy_cells.any() and (cell_w[noisy_cells] == 47).all()             # the others end higher: at the cap
        assert result["samples"] == 48 and result["capped"] and result["figure"] == pt.noise_estimate()["figure"] > 1e-8
        counts, mean = pt.sample_counts()
        assert mean == w.mean(dtype=np.float64) and result["mean_samples"] == mean + 1 and 16 < result["mean_samples"] < result["samples"]   # below the pass count
        assert len(result["active_share"]) == 2 and all(0 < share < 1 for share in result["active_share"])
    finally:
        pt.close(); scene.close(); grt.config_reset()


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------

def test_command_line_sample_map_equals_the_library(grt, tmp_path):
    """pathtracer --noise-target t --adaptive --sample-map against the same run through the library: -N 48 in batches of 4 declares bursts of 8 submissions, so the
    figure is asked for after samples 8 and 40; t is the median cell mean after sample 8, which leaves cells on both sides."""
    from test_gpu_noise import _read_luminance_exr
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    grt.config_reset()
    scene = grt.Scene(scene_file)
    w, h = int(grt.config_get("initial_width")), int(grt.config_get("initial_height"))
    grt.config_set(noise_min_samples=8)
    pt = grt.Pathtracer(scene, w, h, device=0)
    try:
        pt.set_noise_estimate(True)
        pt.update()
        grt.set_frame_pipelining(pt.ctx, True); grt.set_stream_batch(pt.ctx, 8 * 4 * w * h)
        pt.render()
        target, next_check, shares = None, 0, []
        while pt.sample_index < 48:
            if pt.sample_index >= 8 and pt.sample_index >= next_check:
                next_check = pt.sample_index + 32
                estimate = pt.noise_estimate()
                if target is None:
                    means = estimate["cell_sums"][estimate["cell_counts"] > 0] / estimate["cell_counts"][estimate["cell_counts"] > 0]
                    target = float(np.float32(np.median(means)))
                    assert estimate["figure"] > target
                if estimate["figure"] <= target:
                    break
                chosen = pt.select_adaptive(target)
                shares.append(chosen["active_cells"] / chosen["cells"])
            pt.update()
            pt.render_samples(min(4, 48 - pt.sample_index + 1))
        last = pt.sample_index                                                     # 48, or 40 where the figure has reached the target by then
        assert last in (40, 48) and len(shares) == (2 if last == 48 else 1) and 0 < shares[0] < 1
        want, mean = pt.sample_counts()
        want = want[:, :w][::-1]
    finally:
        pt.close(); scene.close(); grt.config_reset()
    r = subprocess.run([CLI, "-s", scene_file, "-o", str(tmp_path / "out.exr"), "-N", "48", "--noise-target", "%.9g" % target, "--noise-min-samples", "8", "--adaptive",
                        "--sample-map", str(tmp_path / "samples.exr")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    m = re.search(r"Adaptive: (\S+) samples per pixel on average; (\S+) % of the cells active at the end; per check:((?: \S+)+)", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)) == pytest.approx(mean + 1, abs=1e-3) and [float(v) for v in m.group(3).split()] == pytest.approx(shares, abs=1e-3)
    assert float(m.group(2)) == pytest.approx(100 * shares[-1], abs=0.1)
    cli_map = _read_luminance_exr(tmp_path / "samples.exr")
    assert "Rendered sample %d " % last in r.stdout
    assert cli_map.shape == want.shape and cli_map.min() == 8 and cli_map.max() == last    # some pixels stopped at the first check, some went on to the end
    assert np.array_equal(cli_map, want)
