"""The firefly filter without a GPU: the float32 restatement of firefly_reference.py against its float64 text within the first-order bound that
text writes out term by term, what the estimator guarantees by construction, the config keys, the command line's argument refusals and the entry points' NULL checks.

The float32 / float64 comparison of the resolve is made on EQUAL tiers (the restatement's): the resolve reads them as inputs."""
import subprocess
from ctypes import byref, c_float

import numpy as np
import pytest

import firefly_cases as cases
import firefly_reference as ref

U = ref.U
K, START, KAPPA = ref.DEFAULTS["tiers"], ref.DEFAULTS["start"], ref.DEFAULTS["support"]


def lum(rgb):
    rgb = np.asarray(rgb, np.float64)
    return rgb[..., 0] * ref.LUMA[0] + rgb[..., 1] * ref.LUMA[1] + rgb[..., 2] * ref.LUMA[2]


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
@pytest.mark.parametrize("first", cases.STARTS)
def test_splat_restatement_against_float64(tiers, first):
    """Eight samples per pixel over every palette level; the distance stays within the bound, the bound within 64 u of the pixel's tiers."""
    width, height, pitch = 65, 9, 96
    frames = cases.sample_frames(width, height, pitch, 8, tiers)[:, :, :width]
    _, _, state = cases.running_state(width, height, pitch, tiers, 5)
    state = state[:, :, :width]
    got32 = ref.accumulate(frames, state, first, START, np.float32)
    got64, bound = ref.accumulate(frames, state, first, START, np.float64, want_bound=True)
    assert got32.dtype == np.float32 and got64.dtype == np.float64 and np.isfinite(got64).all()
    distance = np.abs(got32.astype(np.float64) - got64)
    assert (distance <= 2 * bound + 1e-300).all(), float((distance / np.maximum(bound, 1e-300)).max())
    assert (bound <= 64 * U * np.abs(got64).sum(axis=0)).all()   # (of the pixel's tiers together: a weight near 0 leaves little in its tier and an error of u times the sample)


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
def test_resolve_restatement_against_float64(tiers):
    worst = 0.0
    for width, height in cases.SIZES:
        images = cases.resolve_case(width, height, width + 5, tiers)
        for support in (1.5, KAPPA, 40.0):
            got32 = ref.resolve(**images, width=width, support=support, dtype=np.float32)
            got64, bound = ref.resolve(**images, width=width, support=support, dtype=np.float64, want_bound=True)
            assert got32.dtype == np.float32 and np.isfinite(got64).all()
            distance = np.abs(got32.astype(np.float64) - got64)
            assert (distance <= 2 * bound).all(), (width, height, support, float((distance / np.maximum(bound, 1e-300)).max()))
            scale = np.maximum(np.abs(got64[..., :3]).max(axis=-1) + np.abs(got64[..., 3]), 1e-3)   # kept and held back together: the error of a factor scales with its tier
            worst = max(worst, float((bound[..., :3].max(axis=-1) / scale).max()))
    print("resolve, %d tiers: the bound's largest value relative to the pixel's mean %.3g" % (tiers, worst))
    assert worst < 1e-3   # small enough to mean something (its size: support near 1 divides by support - 1)


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
def test_tiers_sum_to_the_samples_and_their_count(tiers):
    frames = cases.sample_frames(63, 5, 64, 12, tiers)[:, :, :63]
    got = ref.accumulate(frames, np.zeros((tiers, 5, 63, 4), np.float32), 1, START, np.float64)
    finite = np.isfinite(frames[..., :3].sum(axis=-1))
    want = np.where(finite[..., None], frames.astype(np.float64), 0.0).sum(axis=0)
    want[..., 3] = finite.sum(axis=0)
    assert finite.sum() < finite.size and (frames[..., 0] > cases.boundaries(tiers)[-1]).any()   # some samples are not finite, some lie above the top tier
    np.testing.assert_allclose(got.sum(axis=0), want, rtol=1e-12, atol=1e-12)   # nothing is clamped away
    assert (got[..., 3] >= 0).all()


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_splat_puts_at_most_its_boundary_into_a_tier(tiers, dtype):
    b = cases.boundaries(tiers).astype(np.float64)
    levels = np.concatenate([np.exp(np.linspace(np.log(1e-3), np.log(b[-1] * 1e3), 4001)), cases.palette(tiers)[np.isfinite(cases.palette(tiers))]]).astype(np.float32)
    samples = np.repeat(levels[None, None, :, None], 3, axis=-1)
    got = cases.splat_samples(samples, tiers, START, ref, dtype).astype(np.float64)
    slack = 1 + (8 * U if dtype == np.float32 else 1e-12)
    for j in range(tiers - 1):
        assert (lum(got[j, 0, :, :3]) <= b[j] * slack).all(), j
    above = levels > b[-1]
    assert (got[tiers - 1, 0, above, 3] == 1).all() and (lum(got[tiers - 1, 0, above, :3]) > b[-1]).all()   # the top tier takes everything above it
    assert ((got[..., 3] > 0).sum(axis=0) <= 2).all()   # at most two tiers per sample


def test_a_constant_image_is_kept_whole():
    for n in (1, 7):
        samples = np.full((n, 6, 7, 3), [0.5, 20.0, 3.0], np.float32)
        state = cases.splat_samples(samples, K, START, ref, np.float32)
        mean, moments, fallback = cases.field(samples)
        parts = {}
        got = ref.resolve(mean, moments, state, fallback, dtype=np.float32, parts=parts)
        filled = state[..., 3].max(axis=(1, 2)) > 0   # (the factor of a tier that holds nothing multiplies nothing)
        assert filled.sum() == 2 and (parts["r"][filled] == 1).all() and parts["valid"].all()
        total = state[0, ..., :3]
        for j in range(1, K):
            total = total + state[j, ..., :3]
        assert got[..., :3].tobytes() == (total / np.float32(n)).tobytes() and (got[..., 3] == 0).all()


def test_a_lone_firefly_is_held_back_and_its_neighbours_are_unchanged():
    for dark, dtype in ((0.0, np.float32), (0.0, np.float64), (0.1, np.float64)):
        samples = np.full((16, 5, 5, 3), dark, np.float32)
        plain = ref.resolve(*_resolve_args(samples), dtype=dtype)
        samples[3, 2, 2] = 1e4
        parts = {}
        got = ref.resolve(*_resolve_args(samples), dtype=dtype, parts=parts)
        others = np.ones((5, 5), bool); others[2, 2] = False
        assert got[others].tobytes() == plain[others].tobytes()
        held_back = float(got[2, 2, 3]) * 16 / lum(np.full(3, 1e4))
        if dark == 0.0:   # nothing below it: the colour term is 0 too
            assert (got[2, 2, :3] == 0).all() and abs(held_back - 1) < 1e-6
        else:   # the colour term keeps luminance(R) / b_j of a tier: 1.5 / 4096 and less of the one above
            assert 1 - 1.5 / 4096 * 1.01 < held_back < 1 and 0 < lum(got[2, 2, :3]) - 1.5 / 16 < 1e4 / 16 * 1.5 / 4096 * 1.01
        assert (parts["n"][4:, 2, 2] == 1).all() and (parts["r"][4:, 2, 2] <= 1.5 / 4096 * 1.01).all()


def _resolve_args(samples, tiers=K):
    mean, moments, fallback = cases.field(samples)
    return mean, moments, cases.splat_samples(samples, tiers, START, ref, np.float32), fallback


def test_a_firefly_with_support_among_the_neighbours_is_kept():
    samples = np.zeros((16, 6, 6, 3), np.float32)
    for k, (y, x) in enumerate(((2, 2), (2, 3), (3, 2), (3, 3))):   # kappa = 4 samples, in four neighbouring pixels
        samples[k, y, x] = 1e4
    parts = {}
    got = ref.resolve(*_resolve_args(samples), support=KAPPA, dtype=np.float64, parts=parts)
    for y, x in ((2, 2), (2, 3), (3, 2), (3, 3)):
        assert (parts["r"][4:, y, x] == 1).all() and (np.abs(parts["n"][4:, y, x] - 4) < 1e-6).all()   # (1e4 lies between b_4 and b_5)
        np.testing.assert_allclose(got[y, x, :3], 1e4 / 16, rtol=1e-6)
        assert abs(got[y, x, 3]) < 1e-9
    samples[3, 3, 3] = 0.0   # three of them: a third of the way (n - 1) / (kappa - 1) = 2 / 3
    got = ref.resolve(*_resolve_args(samples), support=KAPPA, dtype=np.float64)
    np.testing.assert_allclose(got[2, 2, :3], 1e4 / 16 * 2 / 3, rtol=1e-6)


def test_the_colour_term_keeps_a_tier_below_the_lower_tiers_sum():
    samples = np.full((101, 3, 3, 3), 0.9, np.float32)
    samples[50, 1, 1] = 10.0   # alone among its neighbours (rc = 0), but the 100 samples below it sum to 90 > b_1 = 8 and > b_2 = 64
    parts = {}
    got = ref.resolve(*_resolve_args(samples), dtype=np.float64, parts=parts)
    assert abs(parts["n"][2, 1, 1] - 1) < 1e-6 and (parts["r"][:3, 1, 1] == 1).all()   # (10 lies between b_1 and b_2)
    np.testing.assert_allclose(got[1, 1, :3], (100 * 0.9 + 10.0) / 101, rtol=1e-6)
    assert abs(got[1, 1, 3]) < 1e-9


def test_samples_0_and_1_reset_the_tiers():
    frames = cases.sample_frames(3, 2, 3, 3, K)
    stale = np.full((K, 2, 3, 4), 5.0, np.float32)
    for dtype in (np.float32, np.float64):
        from_0 = ref.accumulate(frames, stale, 0, START, dtype)          # sample 0 sets the mean, sample 1 overwrites it: samples 1 and 2 remain
        from_1 = ref.accumulate(frames[1:], stale, 1, START, dtype)
        fresh = ref.accumulate(frames[1:], np.zeros_like(stale), 2, START, dtype)
        assert from_0.tobytes() == from_1.tobytes() == fresh.tobytes()
        kept = ref.accumulate(frames[1:], stale, 2, START, dtype)
        assert np.allclose(kept.sum(axis=0)[..., 3], 5.0 * K + np.isfinite(frames[1:, ..., 0]).sum(axis=0))
        w = np.array([[0, 1, 5], [0, 0, 2]], np.float32)                  # the list form: the pixel's own fold index w + 1
        listed = ref.accumulate(frames[1:], stale, w + 1, START, dtype)
        assert listed[:, w == 0].tobytes() == fresh[:, w == 0].tobytes() and listed[:, w > 0].tobytes() == kept[:, w > 0].tobytes()
    covered = np.array([[True, False, True], [False, True, False]])
    partial = ref.accumulate(frames, stale, 0, START, np.float32, pixels=covered)
    assert (partial[:, ~covered] == 5.0).all() and partial[:, covered].tobytes() == ref.accumulate(frames, stale, 0, START, np.float32)[:, covered].tobytes()


def test_samples_that_are_not_finite_and_pixels_that_are_not_valid():
    frames = np.ones((5, 1, 4, 4), np.float32)
    frames[1, 0, 0, 0] = np.nan; frames[2, 0, 1, 1] = np.inf; frames[3, 0, 2, 2] = -np.inf; frames[4, 0, 3, :3] = [np.inf, -np.inf, 0]
    state = ref.accumulate(frames, np.zeros((K, 1, 4, 4), np.float32), 1, START, np.float32)
    assert np.isfinite(state).all() and (state.sum(axis=0)[..., 3] == 4).all()   # the sample is skipped whole: its W too
    # the resolve: each rule makes its pixel invalid -- (fallback, -1) -- and takes it out of its neighbours' counts
    samples = np.zeros((8, 3, 7, 3), np.float32)
    samples[0, 1, 1:6] = 1e4   # five neighbouring fireflies in the middle row: everyone there counts 2 or 3 ...
    for rule in ("w0", "nan_w", "nan_mean", "inf_tier", "nan_tier_w"):
        mean, moments, state, fallback = _resolve_args(samples)
        state = state.copy()
        if rule == "w0": moments[1, 3, 3] = 0.0
        if rule == "nan_w": moments[1, 3, 3] = np.nan
        if rule == "nan_mean": mean[1, 3, 2] = np.nan
        if rule == "inf_tier": state[1, 1, 3, 0] = np.inf
        if rule == "nan_tier_w": state[0, 1, 3, 3] = np.nan
        parts = {}
        got = ref.resolve(mean, moments, state, fallback, dtype=np.float32, parts=parts)
        assert not parts["valid"][1, 3] and parts["valid"].sum() == 20
        assert (got[1, 3] == [7.0, 7.0, 7.0, -1.0]).all() and np.isfinite(got).all()
        assert abs(parts["n"][4, 1, 2] - 2) < 1e-6 and abs(parts["n"][5, 1, 2] - 2) < 1e-6   # ... but a neighbour of the invalid pixel counts itself and ONE neighbour
    whole = {}
    ref.resolve(*_resolve_args(samples), dtype=np.float32, parts=whole)
    assert abs(whole["n"][4, 1, 2] - 3) < 1e-6 and abs(whole["n"][5, 1, 2] - 3) < 1e-6


GROWTH = [8, 16, 32]   # every eighth sample of the centre pixel is bright: 1, 2 and 4 = kappa of them


def test_the_resolved_pixel_approaches_the_mean_as_samples_grow():
    distances = []
    for n in GROWTH:
        samples = np.full((n, 3, 3, 3), 0.5, np.float32)
        samples[7::8, 1, 1] = 100.0
        mean, moments, state, fallback = _resolve_args(samples)
        got = ref.resolve(mean, moments, state, fallback, dtype=np.float64)
        distances.append(float(lum(mean[1, 1, :3]) - lum(got[1, 1, :3])))
        assert abs(got[1, 1, 3] - distances[-1]) < 1e-5   # what is missing from the mean is what .w reports
    print("held back at N = %s: %s" % (GROWTH, distances))
    assert distances[0] > distances[1] > distances[2] and abs(distances[2]) < 1e-6


CONFIG_REFUSALS = [("firefly_filter", 2), ("firefly_filter", -1), ("firefly_filter", float("nan")), ("firefly_tiers", 1), ("firefly_tiers", 9), ("firefly_tiers", 2.5),
                   ("firefly_tiers", float("nan")), ("firefly_start", 0.0), ("firefly_start", -1.0), ("firefly_start", float("inf")), ("firefly_support", 1.0),
                   ("firefly_support", float("nan")), ("firefly_support", float("inf"))]


def test_config_keys(fresh_config):
    grt = fresh_config
    defaults = {"firefly_filter": 0, "firefly_tiers": 6, "firefly_start": 1.0, "firefly_support": 4.0}
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key
    for key, value in CONFIG_REFUSALS:
        with pytest.raises(KeyError, match=key):
            grt.config_set(**{key: value})
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key   # a refusal changes nothing
    grt.config_set(firefly_filter=1, firefly_tiers=8, firefly_start=0.25, firefly_support=2.5)
    assert [grt.config_get(k) for k in defaults] == [1, 8, 0.25, 2.5]
    grt.config_reset()
    assert grt.config_get("firefly_filter") == 0 and grt.config_get("firefly_tiers") == 6
    assert {k: ref.DEFAULTS[k] for k in grt.FIREFLY_DEFAULTS} == grt.FIREFLY_DEFAULTS


def test_command_line_refuses_at_argument_parsing(grt):
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    def refused(*options):
        r = subprocess.run([CLI, "-s", scene_file] + [str(o) for o in options], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Initialization" not in r.stdout, r.stdout + r.stderr
        return r.stderr
    for options in (("--firefly-tiers", 4), ("--firefly-start", 2), ("--firefly-support", 3), ("--firefly-map", "m.exr"), ("--firefly-unfiltered", "u.exr")):
        assert "need --firefly-filter" in refused(*options)
    assert "--firefly-tiers must be between 2 and 8" in refused("--firefly-filter", "--firefly-tiers", 9)
    assert "--firefly-tiers must be between 2 and 8" in refused("--firefly-filter", "--firefly-tiers", 1)
    assert "--firefly-start must be finite and above 0" in refused("--firefly-filter", "--firefly-start", 0)
    assert "--firefly-support must be finite and above 1" in refused("--firefly-filter", "--firefly-support", 1)
    assert "invalid integer" in refused("--firefly-filter", "--firefly-tiers", "many")
    assert "names the output file" in refused("--firefly-filter", "-o", "same.exr", "--firefly-unfiltered", "same.exr")
    assert "another image goes to" in refused("--firefly-filter", "-o", "same.exr", "--firefly-map", "same.exr")
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(option in r.stdout for option in ("--firefly-filter", "--firefly-tiers", "--firefly-start", "--firefly-support", "--firefly-map", "--firefly-unfiltered"))


def test_entry_points_refuse_a_null_context(grt):
    lib = grt.device_lib()
    record = grt.firefly_params()
    image = np.zeros((8, 1, 32, 4), np.float32)
    one = np.ones(1, np.int32)
    ms = c_float(0.0)
    calls = {"rt_set_firefly_cascade": lambda: lib.rt_set_firefly_cascade(None, byref(record)),
             "rt_read_firefly_cascade": lambda: lib.rt_read_firefly_cascade(None, image.ctypes.data, image.size),
             "rt_resolve_fireflies": lambda: lib.rt_resolve_fireflies(None, 4.0),
             "rt_read_resolved": lambda: lib.rt_read_resolved(None, image.ctypes.data),
             "rt_resolve_fireflies_timed": lambda: lib.rt_resolve_fireflies_timed(None, 4.0, 1, byref(ms)),
             "rt_set_denoise_source": lambda: lib.rt_set_denoise_source(None, 1),
             "rt_accumulate_cascade_frames": lambda: lib.rt_accumulate_cascade_frames(None, 0, one.ctypes.data, one.ctypes.data, 1, *[image.ctypes.data] * 3, None, 0, byref(record), image.ctypes.data, 0, image.ctypes.data),
             "rt_resolve_fireflies_images": lambda: lib.rt_resolve_fireflies_images(None, 1, 1, 32, *[image.ctypes.data] * 4, byref(record), 1, image.ctypes.data)}
    for name, call in calls.items():
        assert call() == -1
        assert lib.rt_last_error(None).decode() == name + ": NULL context"
    assert lib.rt_get_firefly_cascade(None, None) == 0 and lib.rt_get_denoise_source(None) == 0
    with pytest.raises(TypeError, match="unknown firefly parameter"):
        grt.firefly_params(kappa=4.0)
    with pytest.raises(ValueError):
        grt.firefly_params(tiers=2.5)
