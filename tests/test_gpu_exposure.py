"""The exposure measurement on the MI355X: kernel_exposure_histogram through rt_measure_exposure_images against numpy's histogram of the same
float32 luminances, count for count, and rt_measure_exposure on a context (Cornell box, 64 x 64, both schedulers).

Tolerance: none. The luminance is three float32 products and two sums in the kernel's order, the bin is read from the float's bits, the counts are integers."""
from ctypes import byref, c_void_p

import numpy as np
import pytest

import exposure_reference as ref
import firefly_cases
from conftest import make_pathtracer

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
F = np.float32
SIZES = [(1, 1), (16, 16), (17, 33), (130, 17), (600, 450)]   # the last: more pixels than one pass of the grid covers (1024 workgroups of 256)


def special_values():
    tiny, below_one = F(2.0 ** -149), np.nextafter(F(1), F(0))
    return np.array([tiny, F(2.0 ** -140), F(2.0 ** -126), np.nextafter(F(2.0 ** -126), F(0)), below_one, 1, 2.0 ** 127, 3.0e38, 0, -0.0, -1, np.nan, np.inf, -np.inf, 0.05, 1.5], F)


def frame(width, height, pitch, seed=0):
    """mean and moments: colours whose luminance is log-uniform over 2^-40 .. 2^40, every fifth pixel a grey special value, w cycling through 0, 0.5, 1, 2, 16, NaN;
    the padding columns hold pixels that would count (w = 5, a NaN mean) if they were read."""
    rng = np.random.default_rng(seed + width)
    lum = np.exp2(rng.uniform(-40, 40, (height, width)))
    tint = rng.uniform(0.2, 1.0, (height, width, 3))
    tint /= (tint * firefly_cases.LUMA.astype(np.float64)).sum(axis=-1, keepdims=True)
    mean = np.full((height, pitch, 4), np.nan, F); moments = np.full((height, pitch, 4), 5, F)
    mean[:, :width, :3] = tint * lum[..., None]; mean[:, :width, 3] = 1
    y, x = np.mgrid[0:height, 0:width]
    linear = x + y * width + seed
    values = special_values()
    grey = linear % 5 == 0
    mean[:, :width, :3][grey] = values[(linear[grey] // 5) % len(values)][:, None]
    mean[:, :width, 1][linear % 23 == 1] = np.inf   # one channel alone
    moments[:, :width, :3] = 1
    moments[:, :width, 3] = np.array([2, 1, 16, 0, 0.5, np.nan, 3], F)[(linear // 2) % 7]
    return mean, moments


@pytest.fixture(scope="module")
def ctx(grt):
    """A bare context: the probe needs no frame, no scene and no estimate."""
    lib = grt.device_lib()
    made = c_void_p()
    assert lib.rt_create(0, byref(made)) == 0, lib.rt_last_error(None)
    yield made
    lib.rt_destroy(made)


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_histogram_probe_against_numpy(grt, ctx, size):
    width, height = size
    pitch = (width + 32) // 32 * 32
    for seed in (0, 1, 2):
        mean, moments = frame(width, height, pitch, seed)
        want = ref.histogram(mean, moments, width)
        runs = [grt.measure_exposure_images(ctx, mean, moments, width=width) for _ in range(2)]
        got = runs[0]
        assert np.array_equal(got["histogram"], want["histogram"]), np.flatnonzero(got["histogram"] != want["histogram"])
        assert (got["pixels"], got["dark_pixels"], got["nonfinite_pixels"]) == (want["pixels"], want["dark_pixels"], want["nonfinite_pixels"])
        assert runs[1]["histogram"].tobytes() == got["histogram"].tobytes()
        assert grt.exposure_start(got["histogram"], 2) == ref.start(want["histogram"], 2)
    if width * height >= 256:
        assert want["pixels"] > 0 and want["dark_pixels"] > 0 and want["nonfinite_pixels"] > 0 and want["histogram"][0] > 0 and (want["histogram"] > 0).sum() > 40
    # the special values one at a time, as a one-row frame with every w that matters
    values = special_values()
    for w in (0, 1, 2):
        mean = np.zeros((1, 32, 4), F); mean[0, :len(values), :3] = values[:, None]
        moments = np.zeros((1, 32, 4), F); moments[0, :, 3] = w
        got, want = grt.measure_exposure_images(ctx, mean, moments, width=len(values)), ref.histogram(mean, moments, len(values))
        assert np.array_equal(got["histogram"], want["histogram"]) and (got["pixels"], got["dark_pixels"], got["nonfinite_pixels"]) == (want["pixels"], want["dark_pixels"], want["nonfinite_pixels"])
        assert (got["pixels"] == 0) == (w == 0)


def test_probe_refusals(grt, ctx):
    image = np.zeros((4, 32, 4), F)
    with pytest.raises(grt.DeviceRefusal, match="pitch at least width") as refusal:
        grt.measure_exposure_images(ctx, image, image, width=33)
    assert refusal.value.status == RT_ERROR_INVALID_ARG
    lib = grt.device_lib()
    record, histogram = grt.ExposureRecord(), np.zeros(256, np.uint64)
    assert lib.rt_measure_exposure_images(ctx, 4, 4, 32, image.ctypes.data, None, byref(record), histogram.ctypes.data) == RT_ERROR_INVALID_ARG
    assert lib.rt_measure_exposure_images(ctx, 4, 4, 32, image.ctypes.data, image.ctypes.data, None, histogram.ctypes.data) == RT_ERROR_INVALID_ARG
    assert lib.rt_measure_exposure_images(ctx, 4, 0, 32, image.ctypes.data, image.ctypes.data, byref(record), histogram.ctypes.data) == RT_ERROR_INVALID_ARG
    assert lib.rt_measure_exposure(ctx, byref(record), histogram.ctypes.data) == RT_ERROR_NOT_READY and b"noise estimate is off" in lib.rt_last_error(ctx)


# ---- on a context: cornellbox, 64 x 64, 3 bounces ---------------------------------------------------------------------------------------------------

W, H, SAMPLES = 64, 64, 6


def _render(grt, pt, samples, mode="merged"):
    grt.set_scheduler(pt.ctx, "slots" if mode == "slots" else "merged")
    pt.invalidate("gpu_config")
    pt.update()
    assert pt.sample_index == 0
    pt.render()
    while pt.sample_index + 1 < samples:
        pt.update()
        pt.render()


@pytest.fixture(scope="module")
def cornell(grt):
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, firefly_filter=1)
    yield scene, pt
    grt.set_scheduler(pt.ctx, "merged")
    pt.close(); scene.close(); grt.config_reset()


@pytest.mark.parametrize("mode", ["merged", "slots"])
def test_the_context_call_is_the_probe_on_its_images_and_leaves_the_frame_alone(grt, cornell, mode):
    scene, pt = cornell
    try:
        _render(grt, pt, SAMPLES, mode)
        state = lambda: [pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, H, pt.pitch), grt.read_firefly_cascade(pt.ctx, H, pt.pitch), pt.read_framebuffer().copy()]
        before = state()
        got = grt.measure_exposure(pt.ctx)
        for a, b in zip(before, state()):
            assert a.tobytes() == b.tobytes()
        probe = grt.measure_exposure_images(pt.ctx, before[0], before[1], width=W)
        want = ref.histogram(before[0], before[1], W)
        for other in (probe, want):
            assert np.array_equal(got["histogram"], other["histogram"]) and all(got[k] == other[k] for k in ("pixels", "dark_pixels", "nonfinite_pixels"))
        assert got["pixels"] + got["dark_pixels"] + got["nonfinite_pixels"] == W * H and got["pixels"] > W * H // 2
        print("cornellbox %d x %d, %d samples (%s): median exponent %d" % (W, H, SAMPLES, mode, grt.exposure_start(got["histogram"])[1]))
        # a render continued after the call equals the same render without it
        for _ in range(2):
            pt.update(); pt.render()
        continued = state()
        _render(grt, pt, SAMPLES + 2, mode)
        for a, b in zip(continued, state()):
            assert a.tobytes() == b.tobytes()
    finally:
        grt.set_scheduler(pt.ctx, "merged")


def test_context_refusals(grt, cornell):
    scene, pt = cornell
    lib = grt.device_lib()
    _render(grt, pt, 3)
    record, histogram = grt.ExposureRecord(), np.zeros(256, np.uint64)
    assert lib.rt_measure_exposure(pt.ctx, None, histogram.ctypes.data) == RT_ERROR_INVALID_ARG and lib.rt_measure_exposure(pt.ctx, byref(record), None) == RT_ERROR_INVALID_ARG
    config = pt.device_config()
    svgf = type(config).from_buffer_copy(config); svgf.enable_svgf = 1
    assert lib.rt_set_config(pt.ctx, byref(svgf)) == 0
    with pytest.raises(grt.DeviceRefusal, match="SVGF") as refusal:
        grt.measure_exposure(pt.ctx)
    assert refusal.value.status == RT_ERROR_NOT_READY
    assert lib.rt_set_config(pt.ctx, byref(config)) == 0
    assert grt.measure_exposure(pt.ctx)["pixels"] > 0
    # before sample 2 has been folded no pixel holds a sample's mean (w = 0 after a zeroing): an empty histogram, which exposure_start answers with None
    grt.set_noise_estimate(pt.ctx, True)
    empty = grt.measure_exposure(pt.ctx)
    assert empty["pixels"] == 0 and not empty["histogram"].any() and grt.exposure_start(empty["histogram"]) is None
    grt.set_noise_estimate(pt.ctx, False)
    with pytest.raises(grt.DeviceRefusal, match="noise estimate is off") as refusal:
        grt.measure_exposure(pt.ctx)
    assert refusal.value.status == RT_ERROR_NOT_READY
    _render(grt, pt, 3)   # the host puts its configuration back
    assert grt.measure_exposure(pt.ctx)["pixels"] > 0


# ---- automatic start (config firefly_auto_start): cornellbox, 64 x 64 ---------------------------------------------------------------------------------

PILOT, SHIFT, AFTER = 4, 2, 6
DEFAULT = 4.0   # config firefly_start: what the progression begins with, and a value no power-of-two class of this scene plus the shift gives


def _advance(pt, calls):
    for _ in range(calls):
        pt.update(); pt.render()


def _full_state(grt, pt):
    grt.resolve_fireflies(pt.ctx)
    return [pt.read_framebuffer().copy(), pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, H, pt.pitch), grt.read_firefly_cascade(pt.ctx, H, pt.pitch),
            grt.read_resolved(pt.ctx, H, pt.pitch)]


@pytest.mark.parametrize("mode", ["merged", "slots"])
def test_auto_start_is_the_pilots_histogram_and_renders_what_a_hand_set_start_renders(grt, mode):
    """(a) The start in force after the pilot is exposure_start of the histogram of a hand-rendered pilot of the same length. (b) The render that follows the restart is
    bit-identical -- final image, mean, moments, tiers, resolved image -- to a render with that start set by hand from sample 0. (c) A camera restart keeps the
    start without another pilot; a resize measures again."""
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, firefly_filter=1, firefly_start=DEFAULT)
    try:
        grt.set_scheduler(pt.ctx, mode)
        pt.render()                                  # make_pathtracer's update() was sample 0
        _advance(pt, PILOT - 1)
        assert pt.sample_index == PILOT - 1 and pt.firefly_start == DEFAULT and not pt.firefly_start_measured
        want = grt.exposure_start(grt.measure_exposure(pt.ctx)["histogram"], SHIFT)
        assert want is not None and want[0] != DEFAULT, "the pilot's start is the default: the test would show nothing"
        pt.set_firefly_filter(True, start=want[0])   # by hand, from sample 0
        _advance(pt, AFTER)
        assert pt.sample_index == AFTER - 1 and grt.get_firefly_cascade(pt.ctx)["start"] == want[0]
        by_hand = _full_state(grt, pt)
    finally:
        grt.set_scheduler(pt.ctx, "merged")
        pt.close(); scene.close(); grt.config_reset()
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, firefly_filter=1, firefly_start=DEFAULT, firefly_auto_start=1, firefly_start_shift=SHIFT, firefly_pilot_samples=PILOT)
    try:
        grt.set_scheduler(pt.ctx, mode)

        def run(count):   # `count` samples from the one update() has just set: as one call where the scheduler takes bursts, else one by one
            if mode == "merged":
                pt.render_samples(count)
            else:
                pt.render()
                _advance(pt, count - 1)
        pt.render()
        _advance(pt, PILOT - 1)
        assert pt.sample_index == PILOT - 1 and pt.firefly_start == DEFAULT and not pt.firefly_start_measured and pt.firefly_pilot_samples_discarded == 0
        _advance(pt, 1)                              # before this sample the exposure is measured; the progression starts over
        assert pt.firefly_start_measured and pt.firefly_start == want[0] and pt.sample_index == 0 and pt.firefly_pilot_samples_discarded == PILOT
        assert grt.get_firefly_cascade(pt.ctx)["start"] == want[0] and grt.config_get("firefly_start") == DEFAULT
        _advance(pt, AFTER - 1)
        assert pt.sample_index == AFTER - 1
        for a, b, what in zip(_full_state(grt, pt), by_hand, ("final image", "mean", "moments", "tiers", "resolved image")):
            assert a.tobytes() == b.tobytes(), what
        pt.invalidate("gpu_config"); pt.update()
        assert pt.sample_index == 0 and pt.firefly_start == want[0] and pt.firefly_start_measured     # (c) kept across a restart of the progression
        pt.render(); pt.update(); run(AFTER - 1)
        assert pt.sample_index == AFTER - 1 and pt.firefly_pilot_samples_discarded == PILOT
        for a, b, what in zip(_full_state(grt, pt), by_hand, ("final image", "mean", "moments", "tiers", "resolved image")):
            assert a.tobytes() == b.tobytes(), what + " after a restart"
        # a change of a firefly key measures again, and render_samples ends its burst at the pilot's end
        grt.config_set(firefly_pilot_samples=PILOT + 1)
        pt.update()
        assert pt.sample_index == 0 and not pt.firefly_start_measured and pt.firefly_start == DEFAULT
        pt.render(); pt.update(); run(PILOT + AFTER)
        assert pt.firefly_start_measured and pt.firefly_pilot_samples_discarded == 2 * PILOT + 1 and pt.sample_index == AFTER - 1
        grt.config_set(firefly_pilot_samples=PILOT)
        # ... and so does a resize
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, 48, 40) == 0
        pt.update()
        assert not pt.firefly_start_measured and pt.firefly_start == DEFAULT
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, W, H) == 0
    finally:
        grt.set_scheduler(pt.ctx, "merged")
        pt.close(); scene.close(); grt.config_reset()
