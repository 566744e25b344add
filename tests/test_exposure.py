"""The exposure measurement behind the firefly filter's automatic start, without a GPU: grt_exposure_start of the host library against the numpy
restatement and against values worked out by hand, the exponent histogram's restatement on the floats where a bit trick can go wrong, the robustness of the median
exponent that is the reason for the statistic, and the entry points' refusals."""
from ctypes import byref

import numpy as np
import pytest

import exposure_reference as ref

F = np.float32


def _histogram(**bins):
    h = np.zeros(256, np.uint64)
    for b, count in bins.items():
        h[int(b[1:])] = count
    return h


START_CASES = [
    # name, histogram, shift, (start, exponent)
    ("odd total", _histogram(b120=1, b122=1, b125=1), 0, (2.0 ** -5, -5)),                  # rank 2: the middle one
    ("even total", _histogram(b120=1, b122=1, b125=1, b126=1), 0, (2.0 ** -5, -5)),         # rank 2: the lower middle
    ("one bin", _histogram(b127=4096), 0, (1.0, 0)),
    ("tie at the rank", _histogram(b100=5, b110=5), 0, (2.0 ** -27, -27)),                  # the cumulative count REACHES rank 5 in bin 100
    ("one past the tie", _histogram(b100=5, b110=6), 0, (2.0 ** -17, -17)),                 # rank 6
    ("bin 0", _histogram(b0=3), 0, (2.0 ** -96, -96)),                                      # denormals: -127, clamped
    ("bin 0 shifted", _histogram(b0=3), 16, (2.0 ** -96, -96)),
    ("lower clamp met", _histogram(b31=1), 0, (2.0 ** -96, -96)),                           # 31 - 127 = -96
    ("lower clamp passed", _histogram(b40=1), -16, (2.0 ** -96, -96)),
    ("upper clamp met", _histogram(b207=1), 16, (2.0 ** 96, 96)),
    ("upper clamp passed", _histogram(b254=1), 4, (2.0 ** 96, 96)),
    ("shift", _histogram(b122=10), 2, (2.0 ** -3, -3)),
    ("negative shift", _histogram(b122=10), -2, (2.0 ** -7, -7)),
    ("large counts", _histogram(b90=2 ** 63, b91=2 ** 63 - 1), 0, (2.0 ** -37, -37)),       # the total is 2^64 - 1: (pixels + 1) / 2 must not wrap
]


@pytest.mark.parametrize("case", START_CASES, ids=[c[0] for c in START_CASES])
def test_exposure_start_against_hand_values_and_the_restatement(grt, case):
    name, histogram, shift, want = case
    assert ref.start(histogram, shift) == want
    assert grt.exposure_start(histogram, shift) == want


def test_exposure_start_of_an_empty_histogram_writes_nothing(grt):
    from ctypes import POINTER, c_float, c_int, c_void_p
    assert ref.start(np.zeros(256, np.uint64)) is None and grt.exposure_start(np.zeros(256, np.uint64)) is None
    lib = grt.host_lib()
    lib.grt_exposure_start.argtypes = [c_void_p, c_int, POINTER(c_float), POINTER(c_int)]
    start, exponent = c_float(7.5), c_int(-3)
    assert lib.grt_exposure_start(np.zeros(256, np.uint64).ctypes.data, 2, byref(start), byref(exponent)) == 1
    assert start.value == 7.5 and exponent.value == -3
    one = _histogram(b127=1)
    assert lib.grt_exposure_start(one.ctypes.data, 0, None, None) == 0   # either result may be left out


def test_exposure_start_keeps_the_top_boundary_finite(grt):
    """The clamp's reason: the cascade's top boundary of 8 tiers is start * 8^7."""
    start, _ = grt.exposure_start(_histogram(b254=1), 16)
    assert np.isfinite(F(start) * F(8) ** F(7)) and F(start) * F(8) ** F(7) > 0
    start, _ = grt.exposure_start(_histogram(b0=1), -16)
    assert F(start) > 0 and np.isfinite(F(1) / F(start))


def _grey(values, w):
    """A one-row frame: pixel i is grey `values[i]` with moments' w = w[i]."""
    mean = np.zeros((1, len(values), 4), F); mean[0, :, :3] = np.asarray(values, F)[:, None]; mean[0, :, 3] = 1
    moments = np.zeros((1, len(values), 4), F); moments[0, :, 3] = w
    return mean, moments


def test_histogram_restatement_on_the_floats_that_matter():
    tiny, smallest_normal, below_one, top = F(2.0 ** -149), F(2.0 ** -126), np.nextafter(F(1), F(0)), F(2.0 ** 127)
    values = [tiny, smallest_normal, below_one, F(1), top, F(0), F(-1), F(np.nan), F(np.inf)]
    for w in (0, 1, 2):
        got = ref.histogram(*_grey(values, np.full(len(values), w, F)))
        if w == 0:   # a pixel no sample has reached takes no part, whatever it holds
            assert got["pixels"] == got["dark_pixels"] == got["nonfinite_pixels"] == 0 and not got["histogram"].any()
            continue
        assert got["dark_pixels"] == 2 and got["nonfinite_pixels"] == 2 and got["pixels"] == 5
    # the bins, one value at a time: the weights 0.299 + 0.587 + 0.114 sum to 1 to within an ulp, so a grey level's luminance is the level or its float32 neighbour
    def bin_of(value):
        bins, dark, nonfinite = ref.classify(*_grey([value], [1]))
        return int(bins[0, 0]), bool(dark[0, 0]), bool(nonfinite[0, 0])
    assert bin_of(tiny) in ((0, False, False), (-1, True, False))     # 2^-149 times a weight below 1/2 may round to 0: then it is dark. Never another bin.
    assert bin_of(F(2.0 ** -140)) == (0, False, False)                 # a denormal that stays one
    lum = ref.luminance(_grey([smallest_normal], [1])[0])[0, 0]
    assert bin_of(smallest_normal)[0] == (1 if lum >= smallest_normal else 0)
    lum = ref.luminance(_grey([F(1)], [1])[0])[0, 0]
    assert bin_of(F(1))[0] == (127 if lum >= 1 else 126) and bin_of(below_one)[0] == 126
    assert bin_of(F(1.5))[0] == 127 and bin_of(F(3))[0] == 128 and bin_of(F(0.05))[0] == 122
    assert bin_of(top)[0] in (253, 254)
    assert bin_of(F(0)) == (-1, True, False) and bin_of(F(-1)) == (-1, True, False)
    assert bin_of(F(np.nan)) == (-1, False, True) and bin_of(F(np.inf)) == (-1, False, True) and bin_of(F(-np.inf)) == (-1, False, True)
    # one channel that is not finite is enough
    mean, moments = _grey([F(1)], [1]); mean[0, 0, 2] = np.nan
    assert ref.histogram(mean, moments)["nonfinite_pixels"] == 1
    # w: NaN takes no part, 0.5 takes no part, the padding is not read
    mean, moments = _grey([F(1)] * 4, [np.nan, 0.5, 1, 1])
    assert ref.histogram(mean, moments, width=3)["pixels"] == 1


def test_one_firefly_moves_the_mean_and_not_the_median_exponent(grt):
    """The statistic must not be moved by the outliers the filter exists for: one sample of 1e6 among 16 in one pixel of a 64 x 64 frame of 0.05."""
    mean = np.full((64, 64, 4), 0.05, F)
    moments = np.zeros((64, 64, 4), F); moments[..., 3] = 16
    before = ref.histogram(mean, moments)
    lit = mean.copy(); lit[10, 20, :3] = F(0.05) + (F(1e6) - F(0.05)) / F(16)
    after = ref.histogram(lit, moments)
    assert ref.luminance(lit).astype(np.float64).mean() > 8 * ref.luminance(mean).astype(np.float64).mean()
    assert ref.start(before["histogram"]) == ref.start(after["histogram"]) == (2.0 ** -5, -5)
    assert grt.exposure_start(after["histogram"], 2) == (2.0 ** -3, -3)
    assert after["histogram"][122] == 64 * 64 - 1 and after["histogram"].sum() == 64 * 64


def test_entry_points_refuse_a_null_context(grt):
    lib = grt.device_lib()
    image, histogram, record = np.zeros((1, 32, 4), F), np.zeros(256, np.uint64), grt.ExposureRecord()
    calls = {"rt_measure_exposure": lambda: lib.rt_measure_exposure(None, byref(record), histogram.ctypes.data),
             "rt_measure_exposure_images": lambda: lib.rt_measure_exposure_images(None, 1, 1, 32, image.ctypes.data, image.ctypes.data, byref(record), histogram.ctypes.data)}
    for name, call in calls.items():
        assert call() == -1
        assert lib.rt_last_error(None).decode() == name + ": NULL context"


CONFIG_REFUSALS = [("firefly_auto_start", 2), ("firefly_auto_start", -1), ("firefly_auto_start", 0.5), ("firefly_auto_start", float("nan")), ("firefly_start_shift", 17), ("firefly_start_shift", -17),
                   ("firefly_start_shift", 1.5), ("firefly_start_shift", float("nan")), ("firefly_pilot_samples", 1), ("firefly_pilot_samples", 0), ("firefly_pilot_samples", 2.5),
                   ("firefly_pilot_samples", float("inf")), ("firefly_pilot_samples", float("nan"))]


def test_config_keys(fresh_config):
    grt = fresh_config
    defaults = {"firefly_auto_start": 0, "firefly_start_shift": 0, "firefly_pilot_samples": 4, "firefly_start": 1.0}
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key
    for key, value in CONFIG_REFUSALS:
        with pytest.raises(KeyError, match=key):
            grt.config_set(**{key: value})
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key   # a refusal changes nothing
    grt.config_set(firefly_auto_start=1, firefly_start_shift=-16, firefly_pilot_samples=2)
    assert [grt.config_get(k) for k in defaults] == [1, -16, 2, 1.0]
    grt.config_set(firefly_start_shift=16, firefly_start=0.5)   # firefly_start keeps its meaning and its checks
    assert grt.config_get("firefly_start_shift") == 16 and grt.config_get("firefly_start") == 0.5
    with pytest.raises(KeyError, match="firefly_start"):
        grt.config_set(firefly_start=0.0)
    grt.config_reset()
    assert [grt.config_get(k) for k in defaults] == list(defaults.values())


def test_command_line_refuses_at_argument_parsing(grt):
    import subprocess
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    def refused(*options):
        r = subprocess.run([CLI, "-s", scene_file] + [str(o) for o in options], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Initialization" not in r.stdout, r.stdout + r.stderr
        return r.stderr
    assert "--firefly-auto-start needs --firefly-filter" in refused("--firefly-auto-start")
    for options in (("--firefly-start-shift", 1), ("--firefly-pilot", 8)):
        assert "need --firefly-auto-start" in refused("--firefly-filter", *options)
    assert "--firefly-start-shift must be between -16 and 16" in refused("--firefly-filter", "--firefly-auto-start", "--firefly-start-shift", 17)
    assert "--firefly-start-shift must be between -16 and 16" in refused("--firefly-filter", "--firefly-auto-start", "--firefly-start-shift", -17)
    assert "--firefly-pilot must be at least 2" in refused("--firefly-filter", "--firefly-auto-start", "--firefly-pilot", 1)
    assert "invalid integer" in refused("--firefly-filter", "--firefly-auto-start", "--firefly-pilot", "few")
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(option in r.stdout for option in ("--firefly-auto-start", "--firefly-start-shift", "--firefly-pilot"))
