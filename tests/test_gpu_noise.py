"""The noise estimate on the MI355X: kernel_accumulate_moments / kernel_accumulate_group_moments through rt_accumulate_frames,
kernel_noise_cells through rt_estimate_noise(_images), the renders of both schedulers with the estimate on and off, FrameSplit::noise, render_until
and the command line. Every comparison with the float32 replay of noise_reference.py is bit for bit: the kernels' arithmetic is plain float32
-, /, *, + in a stated shape, and the cells' sums are a fixed tree in double."""
import ctypes
import subprocess
import warnings
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

import noise_cases as cases
import noise_checks as checks
import noise_reference as ref
from conftest import make_pathtracer

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
SENTINEL = cases.SENTINEL


@pytest.fixture(scope="module")
def contexts(grt):
    """One bare context per probe frame: rt_create + rt_resize, no scene (the accumulate and noise launches need none)."""
    lib = grt.device_lib()
    lib.rt_resize.argtypes = [c_void_p, c_int, c_int]
    made = {}
    for name, (width, height, pitch) in cases.FRAMES.items():
        ctx = c_void_p()
        assert lib.rt_create(0, byref(ctx)) == 0, lib.rt_last_error(None)
        assert lib.rt_resize(ctx, width, height) == 0, lib.rt_last_error(ctx)
        assert lib.rt_screen_pitch(ctx) == pitch
        made[name] = ctx
    yield made
    for ctx in made.values():
        lib.rt_destroy(ctx)


@pytest.fixture(scope="module")
def folded():
    """The replay, computed once: per frame the sample frames, the kinds, and the state (accumulator, moments) after k samples for every k."""
    out = {}
    for name, samples in (("40x24", 9), ("16x16", 64)):
        frames, kinds = cases.sample_frames(name, samples)
        zero = np.zeros(frames.shape[1:], np.float32)
        states = [(zero, zero)]
        for s in range(samples):
            acc, m2, _ = ref.accumulate(frames[s:s + 1], states[-1][0], states[-1][1], s)
            states.append((acc, m2))
        for state in states:
            for image in state:
                image.setflags(write=False)
        frames.setflags(write=False)
        out[name] = (frames, kinds, states)
    return out


def _with_padding(image, frame):
    """The image with the sentinel in the padding columns, as the probe's caller gives it."""
    width = cases.FRAMES[frame][0]
    out = image.copy()
    out.view(np.uint32)[:, width:] = SENTINEL
    return out


def _check_launch(frame, got, frames_in, acc_in, m2_in, first, counts, merged, mask=None):
    """One probe launch against the replay: accumulator, moments, final image, the sample frames; what lies outside the pixel set keeps what it was given."""
    width, height, pitch = cases.FRAMES[frame]
    inside = np.zeros((height, pitch), bool); inside[:, :width] = True
    if mask is not None:
        inside &= mask
    frames_out, acc, m2, final = got
    want_acc, want_m2, want_final = ref.accumulate_group(frames_in, acc_in, m2_in, first, counts, inside)
    checks.assert_same_bits(acc, want_acc, "accumulator")
    if m2_in is not None:
        checks.assert_same_bits(m2, want_m2, "moments")
    sentinel = cases.sentinel_image(frame)
    checks.assert_same_bits(final, np.where(inside[..., None], want_final, sentinel), "final image")
    want_frames = np.where(inside[None, ..., None], np.float32(0), frames_in) if merged else frames_in
    checks.assert_same_bits(frames_out, want_frames, "sample frames")
    return acc, m2


@pytest.mark.parametrize("form", ["slot", "group"])
def test_accumulate_frames_on_every_kind_of_stream(grt, contexts, folded, form):
    """9 samples from sample 0 over every kind of stream in every cell: one batch, or one group of 2 + 3 + 4. The plain kernel (no moments image) leaves the
    same accumulator, final image and frames as the moments kernel, to the bit."""
    frames, kinds, states = folded["40x24"]
    ctx = contexts["40x24"]
    start = cases.sentinel_image("40x24")   # sample 0 loads nothing: every pixel of the set is overwritten, the padding keeps the sentinel
    merged = form == "group"
    first, counts = ([0, 2, 5], [2, 3, 4]) if merged else ([0], [9])
    args = dict(first_sample=first if merged else 0, sample_count=counts if merged else None, merged=merged, sentinel=SENTINEL)
    got = grt.accumulate_frames(ctx, frames, start, start, **args)
    acc, m2 = _check_launch("40x24", got, frames, start, start, first, counts, merged)
    plain = grt.accumulate_frames(ctx, frames, start, None, **args)
    assert plain[2] is None
    checks.assert_same_bits(plain[1], acc, "accumulator without moments"); checks.assert_same_bits(plain[3], got[3], "final image without moments")
    checks.assert_same_bits(plain[0], got[0], "frames without moments")
    kind = lambda name: kinds == cases.KINDS.index(name)
    assert (m2[kind("constant")][:, :3] == 0).all() and (m2[kind("zeros")][:, :3] == 0).all() and (m2[kinds >= 0][:, 3] == 8).all()
    assert np.isinf(m2[kind("huge")][:, :3]).all() and np.isfinite(acc[kind("huge")][:, :3]).all()                 # M2 overflows beside a finite mean
    assert np.isnan(m2[kind("nan_sample")][:, 1]).all() and np.isfinite(m2[kind("nan_sample")][:, 0]).all()
    assert (m2[kind("denormals")][:, :3] >= 0).all() and (acc[kind("denormals")][:, :3] > 0).all()
    for name in ("firefly_at_1", "firefly_at_last"):
        assert (m2[kind(name)][:, :3] > 1e6).all(), name
    assert (m2[kind("firefly_at_0")][:, :3] < 10).all()                                                          # sample 0 is overwritten: its firefly leaves no trace
    assert (got[3][kind("nan_sample")] == np.array([1000, 0, 1000, 1], np.float32)).all()                         # the NaN guard of the final image


@pytest.mark.parametrize("form", ["slot", "group"])
def test_samples_0_and_1_alone_leave_no_moment(grt, contexts, folded, form):
    frames, kinds, states = folded["40x24"]
    start = cases.sentinel_image("40x24")
    merged = form == "group"
    got = grt.accumulate_frames(contexts["40x24"], frames[:2], start, start, first_sample=[0] if merged else 0, sample_count=[2] if merged else None, merged=merged, sentinel=SENTINEL)
    acc, m2 = _check_launch("40x24", got, frames[:2], start, start, [0], [2], merged)
    assert (m2[kinds >= 0] == np.array([0, 0, 0, 1], np.float32)).all()


def test_64_samples_split_three_ways_give_the_same_bits(grt, contexts, folded):
    """64 x 1 (batch form), 8 submissions x 8 and 3 + 8 + 16 + 37 (one group launch each): the same accumulator and moments, which are the replay's."""
    frames, kinds, states = folded["16x16"]
    ctx = contexts["16x16"]
    pad = lambda image: _with_padding(image, "16x16")
    acc, m2 = pad(states[0][0]), pad(states[0][1])
    for s in range(64):
        _, acc, m2, _ = grt.accumulate_frames(ctx, frames[s:s + 1], acc, m2, first_sample=s, sentinel=SENTINEL)
    results = [(acc, m2)]
    for counts in ([8] * 8, [3, 8, 16, 37]):
        first = [int(v) for v in np.cumsum([0] + counts[:-1])]
        got = grt.accumulate_frames(ctx, frames, pad(states[0][0]), pad(states[0][1]), first_sample=first, sample_count=counts, merged=True, sentinel=SENTINEL)
        results.append(_check_launch("16x16", got, frames, pad(states[0][0]), pad(states[0][1]), first, counts, True))
    for acc, m2 in results:
        checks.assert_same_bits(acc, pad(states[64][0]), "accumulator after 64 samples"); checks.assert_same_bits(m2, pad(states[64][1]), "moments after 64 samples")


@pytest.mark.parametrize("form", ["slot", "group"])
@pytest.mark.parametrize("first", [0, 1, 2, 40])
def test_first_sample(grt, contexts, folded, form, first):
    """Three samples folded from sample index `first` onto the state `first` samples leave."""
    frames, kinds, states = folded["16x16"]
    acc_in, m2_in = _with_padding(states[first][0], "16x16"), _with_padding(states[first][1], "16x16")
    merged = form == "group"
    got = grt.accumulate_frames(contexts["16x16"], frames[first:first + 3], acc_in, m2_in, first_sample=[first, first + 1] if merged else first,
                                sample_count=[1, 2] if merged else None, merged=merged, sentinel=SENTINEL)
    acc, m2 = _check_launch("16x16", got, frames[first:first + 3], acc_in, m2_in, [first, first + 1] if merged else [first], [1, 2] if merged else [3], merged)
    checks.assert_same_bits(acc, _with_padding(states[first + 3][0], "16x16"), "accumulator"); checks.assert_same_bits(m2, _with_padding(states[first + 3][1], "16x16"), "moments")


@pytest.mark.parametrize("form", ["slot", "group"])
@pytest.mark.parametrize("pixel_set", ["range_ending_mid_row", "one_row_tiles_stride_3"])
def test_pixel_sets(grt, contexts, folded, form, pixel_set):
    """The probe folds the context's own pixel set; every image keeps the caller's sentinel outside it."""
    frames, kinds, states = folded["40x24"]
    ctx, lib = contexts["40x24"], grt.device_lib()
    lib.rt_set_pixel_range.argtypes = [c_void_p, c_int, c_int]
    start = cases.sentinel_image("40x24")
    merged = form == "group"
    try:
        if pixel_set == "range_ending_mid_row":
            assert lib.rt_set_pixel_range(ctx, 45, 40 * 10 + 17) == 0
            mask = cases.pixel_set_mask("40x24", 45, 40 * 10 + 17)
        else:
            assert lib.rt_set_pixel_tiles(ctx, 40, 1, 3) == 0
            mask = cases.pixel_set_mask("40x24", tiles=(40, 1, 3))
        assert 0 < mask.sum() < 40 * 24
        got = grt.accumulate_frames(ctx, frames[:5], start, start, first_sample=[0, 3] if merged else 0, sample_count=[3, 2] if merged else None, merged=merged, sentinel=SENTINEL)
        acc, m2 = _check_launch("40x24", got, frames[:5], start, start, [0, 3] if merged else [0], [3, 2] if merged else [5], merged, mask)
        outside = ~mask
        assert (acc.view(np.uint32)[outside] == SENTINEL).all() and (m2.view(np.uint32)[outside] == SENTINEL).all() and (got[3].view(np.uint32)[outside] == SENTINEL).all()
        assert (m2[mask][:, 3] == 4).all()
    finally:
        assert lib.rt_set_pixel_range(ctx, 0, -1) == 0


def test_accumulate_frames_refusals(grt, contexts, folded):
    lib = grt.device_lib()
    one = np.zeros(1, np.int32)
    assert lib.rt_accumulate_frames(None, 0, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, None, 0, one.ctypes.data) == RT_ERROR_INVALID_ARG
    assert b"rt_accumulate_frames: NULL context" in lib.rt_last_error(None)
    frames, kinds, states = folded["16x16"]
    zero = np.zeros(frames.shape[1:], np.float32)
    refused = [(frames[:2], dict(first_sample=-1)), (frames[:2], dict(first_sample=1 << 24)),
               (frames[:9], dict(first_sample=[0] * 9, sample_count=[1] * 9, merged=True)), (frames[:0], dict(first_sample=[0], sample_count=[0], merged=True)),
               (frames[:2], dict(first_sample=[-1], sample_count=[2], merged=True))]
    for given, kwargs in refused:
        with pytest.raises(grt.DeviceRefusal) as refusal:
            grt.accumulate_frames(contexts["16x16"], given, zero, zero, **kwargs)
        assert refusal.value.status == RT_ERROR_INVALID_ARG, kwargs
    with pytest.raises(grt.DeviceRefusal) as refusal:   # 17 samples in one batch
        grt.accumulate_frames(contexts["16x16"], frames[:17], zero, zero, first_sample=0)
    assert refusal.value.status == RT_ERROR_INVALID_ARG and "16 samples" in str(refusal.value)


@pytest.mark.parametrize("frame", ["40x24", "16x16"])
@pytest.mark.parametrize("floor", [1e-2, 0.5])
def test_estimate_noise_on_probe_images(grt, contexts, folded, frame, floor):
    """kernel_noise_cells on the replay's images after 9 samples: the map, the cells' sums (doubles), counts and non-finite counts, the mean. The padding columns
    hold pixels that would count as non-finite if they were read (w = 5, NaN mean); one row of w < 2 pixels and the streams with a NaN or an overflowed M2 land in
    the right counters and in no sum."""
    frames, kinds, states = folded[frame]
    width, height, pitch = cases.FRAMES[frame]
    mean, m2 = states[9][0].copy(), states[9][1].copy()
    m2[3, :width] = states[2][1][3, :width]                      # w == 1
    m2[5, :width, 3] = 0                                          # no sample ever reached the pixel
    mean[:, width:] = np.nan; m2[:, width:] = np.array([1, 1, 1, 5], np.float32)
    want = ref.estimate(mean, m2, width, floor)
    got = grt.estimate_noise(contexts[frame], height, width, pitch, floor=floor, mean=mean, moments=m2)
    assert (got["cells_x"], got["cells_y"]) == ((width + 15) // 16, (height + 15) // 16)
    checks.assert_same_bits(got["pixel_map"], want["pixel_map"], "pixel map")
    assert np.array_equal(got["cell_counts"], want["cell_counts"]) and np.array_equal(got["cell_nonfinite"], want["cell_nonfinite"])
    checks.assert_same_bits(got["cell_sums"], want["cell_sums"], "cell sums")
    assert got["pixels"] == want["pixels"] and got["nonfinite_pixels"] == want["nonfinite_pixels"] and got["mean"] == want["mean"]
    bad = np.isin(kinds, [cases.KINDS.index("huge"), cases.KINDS.index("nan_sample")])
    bad[[3, 5]] = False
    assert got["nonfinite_pixels"] == bad.sum() > 0 and got["pixels"] == width * (height - 2) - bad.sum()
    assert (got["pixel_map"][[3, 5], :width] == -1).all() and (got["pixel_map"][:, width:] == -1).all() and ((got["pixel_map"] == -2) == bad).all()
    constant = kinds == cases.KINDS.index("constant"); constant[[3, 5]] = False
    assert (got["pixel_map"][constant] == 0).all()
    without_map = grt.estimate_noise(contexts[frame], height, width, pitch, floor=floor, mean=mean, moments=m2, want_map=False)
    checks.assert_same_bits(without_map["cell_sums"], want["cell_sums"], "cell sums without a map")


def test_estimate_noise_refusals(grt, contexts, folded):
    lib = grt.device_lib()
    ctx = contexts["40x24"]
    width, height, pitch = cases.FRAMES["40x24"]
    status = lambda call: pytest.raises(grt.DeviceRefusal, call).value.status
    assert not grt.get_noise_estimate(ctx)
    assert status(lambda: grt.estimate_noise(ctx, height, width, pitch)) == RT_ERROR_NOT_READY          # the estimate is off
    assert status(lambda: grt.read_noise_moments(ctx, height, pitch)) == RT_ERROR_NOT_READY
    grt.set_noise_estimate(ctx, True)
    try:
        assert grt.get_noise_estimate(ctx)
        assert (grt.read_noise_moments(ctx, height, pitch) == 0).all()
        assert status(lambda: grt.estimate_noise(ctx, height, width, pitch)) == RT_ERROR_NOT_READY      # nothing takes part
        for floor in (0.0, -1.0, float("nan"), float("inf")):
            assert status(lambda: grt.estimate_noise(ctx, height, width, pitch, floor=floor)) == RT_ERROR_INVALID_ARG
        assert status(lambda: grt.estimate_noise(ctx, height, width, pitch, cell_capacity=5)) == RT_ERROR_INVALID_ARG
    finally:
        grt.set_noise_estimate(ctx, False)
    record = grt.NoiseEstimateRecord()
    assert lib.rt_estimate_noise(None, ctypes.c_float(1e-2), byref(record), None, None, None, 0, None) == RT_ERROR_INVALID_ARG
    assert b"rt_estimate_noise: NULL context" in lib.rt_last_error(None)
    assert lib.rt_set_noise_estimate(None, 1) == RT_ERROR_INVALID_ARG and lib.rt_get_noise_estimate(None) == 0
    frames, kinds, states = folded["40x24"]
    assert status(lambda: grt.estimate_noise(ctx, height, width, pitch, mean=states[1][0], moments=states[1][1])) == RT_ERROR_NOT_READY   # w == 1 everywhere


# ---- renders: cornellbox, 64 x 48, 3 bounces ------------------------------------------------------------------------------------------------------

W, H, SAMPLES = 64, 48, 13   # samples 0 .. 12


def _render(grt, pt, mode, estimate):
    """13 samples in one of four ways; returns (radiance accumulator, final image, moments or None, estimate dict or None)."""
    grt.set_scheduler(pt.ctx, "slots" if mode == "slots" else "merged")
    if mode == "burst":
        grt.set_frame_pipelining(pt.ctx, True); grt.set_stream_batch(pt.ctx, 2 * 4 * W * H)
    pt.set_noise_estimate(estimate)
    pt.invalidate("gpu_config")   # the progression starts over at sample 0
    try:
        pt.update()
        assert pt.sample_index == 0 and grt.get_noise_estimate(pt.ctx) == estimate
        pt.render()
        while pt.sample_index + 1 < SAMPLES:
            pt.update()
            if mode in ("merged", "slots"):
                pt.render()
            else:
                pt.render_samples(min(4, SAMPLES - pt.sample_index))
        assert pt.sample_index == SAMPLES - 1
        acc, final = pt.read_aov(grt.AOV_RADIANCE).copy(), pt.read_framebuffer().copy()
        moments = grt.read_noise_moments(pt.ctx, H, pt.pitch) if estimate else None
        return acc, final, moments, pt.noise_estimate() if estimate else None
    finally:
        if mode == "burst":
            grt.set_frame_pipelining(pt.ctx, False); grt.set_stream_batch(pt.ctx, 0)
        grt.set_scheduler(pt.ctx, "merged")


@pytest.fixture(scope="module")
def cornell(grt):
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3)
    yield scene, pt
    pt.close(); scene.close(); grt.config_reset()


@pytest.fixture(scope="module")
def renders(grt, cornell):
    scene, pt = cornell
    return {(mode, estimate): _render(grt, pt, mode, estimate) for mode in ("merged", "slots", "batches", "burst") for estimate in (False, True)}


@pytest.mark.parametrize("mode", ["merged", "slots", "batches", "burst"])
def test_estimate_leaves_the_render_alone(grt, renders, mode):
    off, on = renders[mode, False], renders[mode, True]
    assert np.isfinite(off[0]).all() and off[0][:, :W, :3].max() > 0
    checks.assert_same_bits(on[0], off[0], "radiance accumulator"); checks.assert_same_bits(on[1], off[1], "final image")


def test_moments_are_the_same_under_every_scheduler_and_equal_the_replay(grt, cornell, renders):
    scene, pt = cornell
    acc, final, moments, estimate = renders["merged", True]
    for mode in ("slots", "batches", "burst"):
        checks.assert_same_bits(renders[mode, True][2], moments, "moments, " + mode)
    assert (moments[:, :W, 3] == SAMPLES - 1).all() and (moments[:, W:] == 0).all() and (moments[:, :W, :3] >= 0).all() and moments[:, :W, :3].max() > 0
    want = ref.estimate(acc, moments, W, grt.config_get("noise_floor"))
    assert estimate["pixels"] == want["pixels"] == W * H and estimate["nonfinite_pixels"] == 0
    checks.assert_same_bits(estimate["cell_sums"], want["cell_sums"], "cell sums"); assert np.array_equal(estimate["cell_counts"], want["cell_counts"])
    mean, figure = ref.summary(want["cell_sums"], want["cell_counts"], grt.config_get("noise_quantile"))
    assert estimate["mean"] == mean == want["mean"] and estimate["figure"] == figure and 0 < mean < 10
    checks.assert_same_bits(pt.noise_map(), want["pixel_map"], "noise map")   # (the context still holds the last render: burst, estimate on)


def test_frame_split_adds_the_ranks_cells(grt, cornell, renders):
    """Two contexts of one GPU with tiles (rank, 2): FrameSplit::noise() adds their cell sums and counts. Against one context: counts exactly, sums to
    255 * 2^-53 = 2.9e-14 relative -- the 255 double additions of a cell in another order."""
    grt.config_reset(); grt.config_set(num_bounces=3)
    scene = grt.Scene(grt.scene_path("cornellbox"))
    grt.config_set(num_bounces=3)
    split = grt.FrameSplit(scene, W, H, [0, 0])
    try:
        for r in range(2):
            split.rank(r).set_noise_estimate(True)
        split.update(); split.render()
        while split.rank(0).sample_index + 1 < SAMPLES:
            split.update(); split.render_samples(min(4, SAMPLES - split.rank(0).sample_index))
        got = split.noise_estimate()
        owned = [grt.read_noise_moments(split.rank(r).ctx, H, split.pitch)[:, :W, 3] for r in range(2)]
    finally:
        split.close(); scene.close(); grt.config_reset(); grt.config_set(num_bounces=3)   # (what the module's own path tracer was made with)
    assert ((owned[0] > 0) ^ (owned[1] > 0)).all() and (owned[0] > 0).sum() == (owned[1] > 0).sum()   # disjoint tiles; the other rank's pixels have w == 0
    one = renders["merged", True][3]
    assert np.array_equal(got["cell_counts"], one["cell_counts"]) and got["pixels"] == one["pixels"] == W * H
    assert np.all(np.abs(got["cell_sums"] - one["cell_sums"]) <= 2.9e-14 * np.abs(one["cell_sums"]))
    assert abs(got["figure"] - one["figure"]) <= 2.9e-14 * one["figure"]


def test_constant_sky_without_geometry_has_no_noise(grt, cornell):
    scene, pt = cornell
    position, rotation, fov = scene.get_camera()
    try:
        scene.set_camera((1e5, 1e5, 1e5), (0.0, 0.0, 0.0, 1.0))   # far outside the box, looking past it: every path ends in the sky
        pt.set_noise_estimate(True)
        pt.invalidate("gpu_config")
        for _ in range(5):
            pt.update(); pt.render()
        acc, moments = pt.read_aov(grt.AOV_RADIANCE)[:, :W], grt.read_noise_moments(pt.ctx, H, pt.pitch)[:, :W]
        assert (acc[..., :3] == acc[0, 0, :3]).all(), "the camera still sees geometry"
        assert (moments[..., :3] == 0).all() and (moments[..., 3] == 4).all()
        estimate = pt.noise_estimate()
        assert estimate["figure"] == 0 and estimate["mean"] == 0 and estimate["pixels"] == W * H
    finally:
        scene.set_camera(position, rotation, fov)
        pt.invalidate("gpu_config")


def test_render_until(grt, cornell):
    scene, pt = cornell
    grt.config_set(noise_min_samples=8)
    try:
        results = {}
        for target in (2.0, 0.1, 0.0):
            pt.set_noise_estimate(True); pt.invalidate("gpu_config")
            results[target] = pt.render_until(target, 24 if target == 0.0 else 96, check_every=4)
            assert results[target]["samples"] == pt.sample_index + 1
            assert results[target]["figure"] == pt.noise_estimate()["figure"]
        print("render_until:", results)
        for target in (2.0, 0.1):
            assert results[target]["samples"] >= 8                                        # never below noise_min_samples
            assert results[target]["capped"] or results[target]["figure"] <= target      # where it stopped by itself the figure is at or below the target
        assert not results[2.0]["capped"] and results[2.0]["samples"] < 96
        assert results[2.0]["samples"] <= results[0.1]["samples"]                        # a looser target stops no later
        assert results[0.0] == dict(results[0.0], samples=24, capped=True) and results[0.0]["figure"] > 0
    finally:
        grt.config_set(noise_min_samples=16)


def test_render_until_with_svgf_warns_and_runs_to_the_cap(grt):
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, enable_svgf=1)
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            result = pt.render_until(0.5, 6, check_every=2)
        assert result["samples"] == 6 and result["capped"] and result["figure"] is None
        assert len(caught) == 1 and "SVGF" in str(caught[0].message)
    finally:
        pt.close(); scene.close(); grt.config_reset()


def _read_luminance_exr(path):
    """The one-channel float file --noise-map writes (scan lines, no compression, 32-bit floats): (height, width) float32, row 0 at the top."""
    import struct
    raw = open(path, "rb").read()
    assert raw[:4] == bytes([0x76, 0x2f, 0x31, 0x01])
    pos, attrs = 8, {}
    while raw[pos] != 0:
        end = raw.index(b"\0", pos); name = raw[pos:end].decode(); pos = end + 1
        pos = raw.index(b"\0", pos) + 1
        size = struct.unpack("<i", raw[pos:pos + 4])[0]; pos += 4
        attrs[name] = raw[pos:pos + size]; pos += size
    pos += 1
    assert attrs["channels"][:2] == b"Y\0" and struct.unpack("<i", attrs["channels"][2:6])[0] == 2 and len(attrs["channels"]) == 2 + 16 + 1   # one channel, FLOAT
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    offsets = struct.unpack("<%dQ" % h, raw[pos:pos + 8 * h])
    image = np.zeros((h, w), np.float32)
    for row in range(h):
        y, size = struct.unpack("<ii", raw[offsets[row]:offsets[row] + 8])
        assert size == 4 * w
        image[y - y0] = np.frombuffer(raw[offsets[row] + 8:offsets[row] + 8 + size], np.float32)
    return image


def test_command_line(grt, tmp_path):
    """pathtracer --noise-target: never below --noise-min-samples, a looser target stops no later, the cap ends the render with the flag; --noise-map holds
    noise_map(); the AO integrator warns and runs to -N. (The scene file's film size, 1024 x 1024, and path length win over -W / -H / -b, as everywhere.)"""
    import re
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    def run(*options):
        r = subprocess.run([CLI, "-s", scene_file, "-o", str(tmp_path / "out.exr")] + [str(o) for o in options], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        m = re.search(r"Noise: figure (\S+) \(mean (\S+), target (\S+)\) after sample (\d+); (target reached|stopped at the sample cap)", r.stdout)
        return r, m
    stops = {}
    for target in (2.0, 0.05):
        r, m = run("-N", 96, "--noise-target", target, "--noise-min-samples", 8)
        assert m, r.stdout
        stops[target] = (int(m.group(4)), float(m.group(1)), m.group(5))
    print("command line:", stops)
    for target, (sample, figure, how) in stops.items():
        assert sample >= 8 and (how == "stopped at the sample cap" or figure <= target)
    assert stops[2.0][2] == "target reached" and stops[2.0][0] < 96 and stops[2.0][0] <= stops[0.05][0]
    r, m = run("-N", 24, "--noise-target", 1e-9, "--noise-map", tmp_path / "noise.exr")
    assert m and int(m.group(4)) == 24 and m.group(5) == "stopped at the sample cap" and float(m.group(1)) > 1e-9
    cli_map = _read_luminance_exr(tmp_path / "noise.exr")
    grt.config_reset()
    scene = grt.Scene(scene_file)
    w, h = int(grt.config_get("initial_width")), int(grt.config_get("initial_height"))
    pt = grt.Pathtracer(scene, w, h, device=0)
    try:
        pt.set_noise_estimate(True)
        pt.update()
        grt.set_frame_pipelining(pt.ctx, True); grt.set_stream_batch(pt.ctx, 7 * 4 * w * h)   # the burst the command line declares for -N 24
        pt.render()
        while pt.sample_index < 24:
            pt.update(); pt.render_samples(min(4, 24 - pt.sample_index + 1))
        assert pt.sample_index == 24
        want = np.maximum(pt.noise_map()[:, :w], 0)[::-1]
    finally:
        pt.close(); scene.close(); grt.config_reset()
    assert cli_map.shape == want.shape
    checks.assert_same_bits(np.ascontiguousarray(cli_map, np.float32), np.ascontiguousarray(want), "--noise-map")
    r = subprocess.run([CLI, "-s", scene_file, "-I", "ao", "-N", "3", "--noise-target", "0.5", "-o", str(tmp_path / "ao.exr")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr.count("WARNING: --noise-target") == 1 and "Rendered sample 3" in r.stdout and "Noise:" not in r.stdout
