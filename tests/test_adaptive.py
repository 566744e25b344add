"""Adaptive sampling without a GPU: the numpy restatement of selection and list order against a second, brute-force writing, the list as a
permutation of exactly the active cells' in-frame pixels, the replay of the list fold, the config keys and the command line's argument refusals."""
import subprocess

import numpy as np
import pytest

import adaptive_cases as cases
import adaptive_reference as ref
import noise_reference as noise


def _reference_selection(frame, name):
    width, height, pitch = cases.FRAMES[frame]
    mean, moments, threshold, dilate = cases.selection_case(frame, name)
    e = noise.estimate(mean, moments, width, cases.FLOOR)
    hot, active = ref.select(e["cell_sums"], e["cell_counts"], e["cell_nonfinite"], width, height, threshold, dilate)
    return e, hot, active, ref.pixel_list(active, width, height)


@pytest.mark.parametrize("frame", list(cases.FRAMES))
@pytest.mark.parametrize("name", cases.SELECTION_CASES)
def test_list_is_the_brute_force_order_and_a_permutation_of_the_active_pixels(frame, name):
    width, height, pitch = cases.FRAMES[frame]
    e, hot, active, pixels = _reference_selection(frame, name)
    assert np.array_equal(pixels, cases.brute_force_list(active, width, height))
    x, y = pixels % width, pixels // width
    assert len(np.unique(pixels)) == len(pixels) and (pixels < width * height).all()
    covered = np.zeros((height, width), bool); covered[y, x] = True
    want = np.repeat(np.repeat(active, 16, axis=0), 16, axis=1)[:height, :width]
    assert np.array_equal(covered, want) and len(pixels) == ref.frame_pixels(width, height)[active].sum()
    assert (active | ~hot).all()                                                # hot cells are active


def test_selection_rules_case_by_case():
    """What each case is built to show, on the frame with 3 x 2 clipped cells."""
    frame = "40x24"
    select = lambda name: _reference_selection(frame, name)
    e, hot, active, pixels = select("on_threshold")
    assert (e["cell_sums"] == 0.5 * e["cell_counts"]).all() and not hot.any() and len(pixels) == 0       # sum == threshold * count is not hot
    e, hot, active, pixels = select("threshold_one_ulp_below")
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert below == 0.5 - 2.0 ** -25 and (e["cell_sums"] == 0.5 * e["cell_counts"]).all() and hot.all() and len(pixels) == 40 * 24   # the boundary, from the other side
    e, hot, active, pixels = select("just_above")
    assert hot.ravel().tolist() == [False] * 5 + [True] and e["cell_sums"][1, 2] > 0.5 * e["cell_counts"][1, 2] and len(pixels) == 64   # the 8 x 8 corner cell
    e, hot, active, pixels = select("every_cell_hot")
    assert hot.all() and np.array_equal(np.sort(pixels), np.arange(40 * 24))
    e, hot, active, pixels = select("nonfinite_cell")
    assert e["cell_nonfinite"][0, 0] == 256 and not hot[0, 0] and hot.sum() == 5
    e, hot, active, pixels = select("unsampled_pixels")
    assert hot.ravel().tolist() == [False] * 5 + [True] and e["cell_counts"][1, 2] == 62
    assert select("hot_corner_dilate_0")[2].sum() == 1 and select("hot_corner_dilate_1")[2].sum() == 4
    e, hot, active, pixels = select("threshold_0")
    assert not hot[0, 0] and hot.sum() == 5                                       # a sum of 0 is not above 0
    # an unclipped cell's 64 consecutive entries cover one 8 x 8 patch
    first = select("hot_corner_dilate_0")[3]
    assert len(first) == 256
    for k in range(4):
        px, py = first[64 * k:64 * k + 64] % 40, first[64 * k:64 * k + 64] // 40
        assert px.max() - px.min() == 7 and py.max() - py.min() == 7 and (px.min(), py.min()) == ref.PATCH_ORDER[k]


def test_list_fold_uses_each_pixels_own_count():
    """w = 0 takes the sample (M2 = (0, 0, 0, 1)), w = 1 makes the first Welford step, w = 15 continues as the uniform fold from sample 16 does; pixels outside
    the list keep everything."""
    rng = np.random.default_rng(3)
    height, width, pitch = 2, 4, 8
    frames = rng.uniform(0.5, 1.5, (3, height, pitch, 4)).astype(np.float32)
    acc = rng.uniform(0.5, 1.5, (height, pitch, 4)).astype(np.float32)
    m2 = rng.uniform(0.0, 1.0, (height, pitch, 4)).astype(np.float32)
    m2[0, 0] = 0; acc[0, 0] = 0            # never sampled
    m2[0, 1] = (0, 0, 0, 1)
    m2[0, 2:4, 3] = 15; m2[1, :, 3] = 15
    pixels = np.array([0, 1, 2, 4 + 1], np.uint32)
    cleared, got_acc, got_m2, written, final = ref.accumulate_list(frames, acc, m2, pixels, width, [1, 2])
    assert written.sum() == 4 and written[0, :3].all() and written[1, 1]
    assert np.array_equal(got_acc[~written], acc[~written]) and np.array_equal(got_m2[~written], m2[~written]) and np.array_equal(cleared[:, ~written], frames[:, ~written])
    assert (cleared[:, written] == 0).all()
    one, _ = noise.fold(acc[0, 0], m2[0, 0], frames[0, 0, 0], 1)
    assert np.array_equal(one, frames[0, 0, 0]) and got_m2[0, 0, 3] == 3 and got_m2[0, 1, 3] == 4 and got_m2[0, 2, 3] == 18
    uniform_acc, uniform_m2, _ = noise.accumulate(frames, acc, m2, 16)           # the uniform fold at sample indices 16, 17, 18
    assert np.array_equal(got_acc[0, 2], uniform_acc[0, 2]) and np.array_equal(got_m2[0, 2], uniform_m2[0, 2])
    with pytest.raises(AssertionError):
        ref.accumulate_list(frames, acc, m2, np.array([1, 1], np.uint32), width, [3])


def test_config_keys(fresh_config):
    grt = fresh_config
    assert grt.config_get("adaptive_sampling") == 0 and grt.config_get("adaptive_dilate") == 1
    for key, value in (("adaptive_sampling", 2), ("adaptive_sampling", -1), ("adaptive_sampling", 0.5), ("adaptive_sampling", float("nan")),
                       ("adaptive_dilate", 2), ("adaptive_dilate", -1), ("adaptive_dilate", float("nan"))):
        with pytest.raises(KeyError, match=key):
            grt.config_set(**{key: value})
    with pytest.raises(KeyError, match="adaptive_sampling"):      # nothing to select by without a noise target
        grt.config_set(adaptive_sampling=1)
    assert grt.config_get("adaptive_sampling") == 0
    grt.config_set(noise_target=0.05)
    grt.config_set(adaptive_sampling=1, adaptive_dilate=0)
    assert grt.config_get("adaptive_sampling") == 1 and grt.config_get("adaptive_dilate") == 0
    with pytest.raises(KeyError, match="noise_target"):            # ... and the target cannot go while adaptive sampling needs it
        grt.config_set(noise_target=0)
    assert grt.config_get("noise_target") == float(np.float32(0.05))
    grt.config_set(adaptive_sampling=0)
    grt.config_set(noise_target=0)
    grt.config_reset()
    assert grt.config_get("adaptive_sampling") == 0 and grt.config_get("adaptive_dilate") == 1


def test_command_line_refuses_at_argument_parsing(grt):
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    def refused(*options):
        r = subprocess.run([CLI, "-s", scene_file] + [str(o) for o in options], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Initialization" not in r.stdout, r.stdout + r.stderr
        return r.stderr
    assert "--adaptive needs --noise-target" in refused("--adaptive")
    assert "--adaptive needs --noise-target" in refused("-N", 8, "--adaptive", "--adaptive-dilate", 0)
    assert "--adaptive-dilate must be 0 or 1" in refused("--noise-target", 0.1, "--adaptive", "--adaptive-dilate", 2)
    assert "invalid integer" in refused("--noise-target", 0.1, "--adaptive", "--adaptive-dilate", "yes")
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--adaptive" in r.stdout and "--sample-map" in r.stdout and "--adaptive-dilate" in r.stdout
