"""The firefly-robust noise estimate without a GPU: the float32 restatement of the robust cells against the plain replay it must equal where
nothing is held, on the planted frame that shows what it is for -- one outlier no longer steers a cell, a supported bright region still does --, at the boundaries of
the definition, and the entry points' refusals."""
from ctypes import byref, c_int64

import numpy as np
import pytest

import adaptive_reference as adaptive
import noise_reference as noise
import robust_noise_cases as cases
import robust_noise_reference as ref

F = np.float32
FLOOR, TAU = cases.FLOOR, cases.TAU


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
@pytest.mark.parametrize("size", cases.SIZES, ids=["%dx%d" % s for s in cases.SIZES])
def test_with_nothing_held_the_restatement_is_the_plain_replay(size, tiers):
    width, height = size
    pitch = (width + 32) // 32 * 32
    images = cases.probe_case(width, height, pitch, tiers)
    plain = noise.estimate(images["mean"], images["moments"], width, FLOOR)
    for nothing in (0.0, -1.0, np.nan):   # nothing held back; not valid to the resolve; not a number
        resolved = images["resolved"].copy(); resolved[..., 3] = nothing
        got = ref.estimate(images["mean"], images["moments"], resolved, width, FLOOR, TAU)
        for key in ("cell_sums", "cell_counts", "cell_nonfinite", "pixel_map"):
            assert same_bits(got[key], plain[key]), key
        assert got["held_pixels"] == 0 and not got["cell_held"].any() and got["mean"] == plain["mean"] and got["pixels"] == plain["pixels"]
    # ... and with held pixels, the cells without one keep the plain bits, the others lose exactly those pixels
    got = ref.estimate(images["mean"], images["moments"], images["resolved"], width, FLOOR, TAU)
    clean = got["cell_held"] == 0
    assert same_bits(got["cell_sums"][clean], plain["cell_sums"][clean]) and same_bits(got["cell_counts"][clean], plain["cell_counts"][clean])
    assert np.array_equal(got["cell_nonfinite"], plain["cell_nonfinite"])                       # held pixels are never also counted as non-finite
    assert np.array_equal(got["cell_counts"] + got["cell_held"], plain["cell_counts"])          # ... and every one of them took part by the plain rule
    assert ((got["pixel_map"] == -3) == ref.held_pixels(images["mean"], images["moments"], images["resolved"], FLOOR, TAU)).all()
    if width * height >= 256:
        assert got["held_pixels"] > 0, "the case holds nothing back: it tests nothing"


@pytest.fixture(scope="module")
def planted():
    return {(kind, start): cases.planted_frame(kind, start) for kind in ("none", "lone", "block") for start in (1.0, 0.125)}


def _cell0_mean(estimate):
    return estimate["cell_sums"][0, 0] / estimate["cell_counts"][0, 0]


@pytest.mark.parametrize("start", [1.0, 0.125])
def test_planted_fireflies_are_held_and_a_supported_block_is_not(planted, start):
    n = cases.PLANTED_SIZE
    clean, lone, block = (planted[(kind, start)] for kind in ("none", "lone", "block"))
    plain_clean = noise.estimate(clean["mean"], clean["moments"], n, FLOOR)
    plain_lone = noise.estimate(lone["mean"], lone["moments"], n, FLOOR)
    robust_lone = ref.estimate(lone["mean"], lone["moments"], lone["resolved"], n, FLOOR, TAU)
    print("cell 0 mean error: clean %.4f, five lone fireflies %.4f, robust %.4f" % (_cell0_mean(plain_clean), _cell0_mean(plain_lone), _cell0_mean(robust_lone)))
    # a firefly pixel's e_p saturates near sqrt(3): the mean is the firefly
    for y, x in cases.LONE:
        assert 1.5 < plain_lone["pixel_map"][y, x] < np.sqrt(3.0) and robust_lone["pixel_map"][y, x] == -3
    assert _cell0_mean(plain_lone) > _cell0_mean(plain_clean) + 0.02
    # the five lone pixels are held, and nothing else
    held = ref.held_pixels(lone["mean"], lone["moments"], lone["resolved"], FLOOR, TAU)
    assert sorted(zip(*np.nonzero(held))) == sorted(cases.LONE)
    assert robust_lone["cell_held"].tolist() == [[5, 0], [0, 0]] and robust_lone["held_pixels"] == 5 and robust_lone["cell_counts"][0, 0] == 251
    # cell 0's robust sum is the sum of the unplanted frame's cell without those pixels: the same tree over the same values, zeros in the five places
    e = plain_clean["pixel_map"][:16, :16].astype(np.float64)
    for y, x in cases.LONE:
        e[y, x] = 0.0
    assert robust_lone["cell_sums"][0, 0] == noise.tree_sum(e.ravel())
    assert same_bits(robust_lone["cell_sums"].ravel()[1:], plain_clean["cell_sums"].ravel()[1:])
    assert abs(_cell0_mean(robust_lone) - _cell0_mean(plain_clean)) < 1e-3
    # at a threshold between the two means the plain selection is hot and the robust one is not
    threshold = float(F(0.5 * (_cell0_mean(plain_lone) + _cell0_mean(robust_lone))))
    others = max(plain_clean["cell_sums"].ravel()[1:] / plain_clean["cell_counts"].ravel()[1:])
    assert others < threshold, "the frame's other cells are as noisy as the planted one: the threshold separates nothing"
    hot_plain, _ = adaptive.select(plain_lone["cell_sums"], plain_lone["cell_counts"], plain_lone["cell_nonfinite"], n, n, threshold, 0)
    hot_robust, _ = ref.select(robust_lone["cell_sums"], robust_lone["cell_counts"], robust_lone["cell_nonfinite"], robust_lone["cell_held"], n, n, threshold, 0)
    assert hot_plain.tolist() == [[True, False], [False, False]] and not hot_robust.any()
    # the same sample value in a 2 x 2 block has support among its neighbours: nothing is held back, the cell stays hot -- that region really is noisy
    robust_block = ref.estimate(block["mean"], block["moments"], block["resolved"], n, FLOOR, TAU)
    plain_block = noise.estimate(block["mean"], block["moments"], n, FLOOR)
    assert robust_block["held_pixels"] == 0 and same_bits(robust_block["cell_sums"], plain_block["cell_sums"])
    hot_block, _ = ref.select(robust_block["cell_sums"], robust_block["cell_counts"], robust_block["cell_nonfinite"], robust_block["cell_held"], n, n, threshold, 0)
    assert hot_block.tolist() == [[True, False], [False, False]]
    print("cell 0 mean error with the 2 x 2 block: %.4f (threshold %.4f)" % (_cell0_mean(robust_block), threshold))


def _uniform(w=4.0, level=1.0, m2=1.0):
    mean = np.full((16, 32, 4), level, F)
    moments = np.zeros((16, 32, 4), F); moments[..., :3] = m2; moments[..., 3] = w
    resolved = np.zeros((16, 32, 4), F)
    return mean, moments, resolved


def test_cells_of_held_and_nonfinite_pixels_only_are_not_hot():
    mean, moments, resolved = _uniform()
    resolved[..., 3] = 100.0            # everything is held back ...
    mean[3, :5, 1] = np.nan             # ... but five pixels, which are not finite: never both
    got = ref.estimate(mean, moments, resolved, 16, FLOOR, TAU)
    assert got["cell_counts"][0, 0] == 0 and got["cell_nonfinite"][0, 0] == 5 and got["cell_held"][0, 0] == 251 and got["cell_sums"][0, 0] == 0.0
    assert (got["pixel_map"][3, :5] == -2).all() and (got["pixel_map"][:, :16] == -3).sum() == 251 and (got["pixel_map"][:, 16:] == -1).all()
    hot, active = ref.select(got["cell_sums"], got["cell_counts"], got["cell_nonfinite"], got["cell_held"], 16, 16, 0.0, 1)
    assert not hot.any() and not active.any()
    # the plain selection would call it hot: to it the held pixels were never judged
    hot, _ = adaptive.select(got["cell_sums"], got["cell_counts"], got["cell_nonfinite"], 16, 16, 0.0, 0)
    assert hot.all()
    # pixels not sampled enough to judge (w < 2) still make it hot, held or not by the resolve
    moments[7, 7, 3] = 1.0
    got = ref.estimate(mean, moments, resolved, 16, FLOOR, TAU)
    assert got["cell_held"][0, 0] == 250 and got["pixel_map"][7, 7] == -1
    hot, _ = ref.select(got["cell_sums"], got["cell_counts"], got["cell_nonfinite"], got["cell_held"], 16, 16, 1e9, 0)
    assert hot.all()


def test_the_held_boundary_is_exclusive():
    """resolved.w == tau * max(Y, floor) exactly is not held; one ulp above is. Above the floor and at it."""
    for level in (1.0, 0.37, 1e-4):
        mean, moments, resolved = _uniform(level=level)
        with np.errstate(all="ignore"):
            lum = (noise.LUMINANCE[0] * F(level) + noise.LUMINANCE[1] * F(level)) + noise.LUMINANCE[2] * F(level)
        bound = F(TAU) * np.fmax(lum, F(FLOOR))
        assert (bound == F(TAU) * F(FLOOR)) == (level < FLOOR)
        resolved[0, 0, 3] = bound
        resolved[0, 1, 3] = np.nextafter(bound, F(np.inf))
        resolved[0, 2, 3] = np.nextafter(bound, F(0))
        got = ref.estimate(mean, moments, resolved, 16, FLOOR, TAU)
        assert got["pixel_map"][0, 0] >= 0 and got["pixel_map"][0, 1] == -3 and got["pixel_map"][0, 2] >= 0 and got["held_pixels"] == 1


def test_entry_points_refuse_a_null_context(grt):
    lib = grt.device_lib()
    image, cells, record, selection, held = np.zeros((1, 32, 4), F), np.zeros(4, np.float64), grt.NoiseEstimateRecord(), grt.CellSelectionRecord(), c_int64()
    p = image.ctypes.data
    calls = {"rt_estimate_noise_robust": lambda: lib.rt_estimate_noise_robust(None, 1e-2, 0.25, byref(record), cells.ctypes.data, p, p, p, 1, None, byref(held)),
             "rt_set_noise_robust": lambda: lib.rt_set_noise_robust(None, 0.25),
             "rt_estimate_noise_robust_images": lambda: lib.rt_estimate_noise_robust_images(None, p, p, p, 1e-2, 0.25, byref(record), cells.ctypes.data, p, p, p, 1, None, byref(held)),
             "rt_select_pixels_robust_images": lambda: lib.rt_select_pixels_robust_images(None, p, p, p, 1e-2, 0.25, 0.1, 1, byref(selection), cells.ctypes.data, p, p, p, p, 1, p, 1)}
    for name, call in calls.items():
        assert call() == -1
        assert lib.rt_last_error(None).decode() == name + ": NULL context"
    assert lib.rt_get_noise_robust(None) == 0.0


CONFIG_REFUSALS = [("noise_robust", 2), ("noise_robust", -1), ("noise_robust", 0.5), ("noise_robust", float("nan")), ("noise_held_fraction", 0.0), ("noise_held_fraction", 1.0),
                   ("noise_held_fraction", -0.25), ("noise_held_fraction", float("nan")), ("noise_held_fraction", float("inf"))]


def test_config_keys(fresh_config):
    grt = fresh_config
    defaults = {"noise_robust": 0, "noise_held_fraction": 0.25}
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key
    for key, value in CONFIG_REFUSALS:
        with pytest.raises(KeyError, match=key):
            grt.config_set(**{key: value})
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key   # a refusal changes nothing
    grt.config_set(noise_robust=1, noise_held_fraction=0.5)
    assert [grt.config_get(k) for k in defaults] == [1, 0.5]
    grt.config_reset()
    assert [grt.config_get(k) for k in defaults] == [0, 0.25]


def test_command_line_refuses_at_argument_parsing(grt):
    import subprocess
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    def refused(*options):
        r = subprocess.run([CLI, "-s", scene_file] + [str(o) for o in options], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Initialization" not in r.stdout, r.stdout + r.stderr
        return r.stderr
    assert "--noise-robust needs --firefly-filter" in refused("--noise-target", 0.05, "--noise-robust")
    assert "--noise-robust needs --noise-target or --noise-map" in refused("--firefly-filter", "--noise-robust")
    assert "--noise-held-fraction needs --noise-robust" in refused("--firefly-filter", "--noise-target", 0.05, "--noise-held-fraction", 0.5)
    for t in (0, 1, -0.5):
        assert "--noise-held-fraction must lie inside (0, 1)" in refused("--firefly-filter", "--noise-target", 0.05, "--noise-robust", "--noise-held-fraction", t)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(option in r.stdout for option in ("--noise-robust", "--noise-held-fraction"))
