"""The noise estimate without a GPU: the float32 replay of the fold with second moments against the float64 restatement, the config keys'
refusals, and grt_noise_summary -- the one function that turns cell sums and counts into the mean and the figure -- against numpy."""
import numpy as np
import pytest

import noise_cases as cases
import noise_checks as checks
import noise_reference as ref


def test_replay_second_moment_against_float64():
    """|M2_32 - M2_64| <= C * u * (n * M2 + n^1.5 * x_max * sqrt(M2) + n * u * x_max^2) for n = 2 .. 255 samples of every stream; prints the worst ratio per stream."""
    worst = {}
    for name, stream in cases.CPU_STREAMS.items():
        worst[name] = 0.0
        for seed in cases.CPU_SEEDS:
            rng = np.random.default_rng(seed)
            for n in cases.CPU_COUNTS:
                error, scale = checks.m2_bound_terms(stream(rng, n).astype(np.float32))
                if scale > 0:
                    worst[name] = max(worst[name], error / scale)
                assert error <= checks.C * scale, (name, seed, n, error, scale)
    print("worst |M2_32 - M2_64| / (u * bracket):", worst, "C =", checks.C)
    assert max(worst.values()) <= checks.WORST_SEEN * 1.001, worst   # the figure noise_checks.py records is the one measured here


def test_replay_keeps_the_quirk_and_the_mean():
    """Samples 0 and 1 leave (0, 0, 0, 1); a constant stream has M2 exactly 0; the mean with moments is the plain mean to the bit."""
    frames, kinds = cases.sample_frames("40x24", 9)
    zero = np.zeros(frames.shape[1:], np.float32)
    acc, m2, _ = ref.accumulate(frames[:2], zero, zero, 0)
    assert (m2[..., :3] == 0).all() and (m2[..., 3] == 1).all()
    acc, m2, _ = ref.accumulate(frames, zero, zero, 0)
    plain, none, _ = ref.accumulate(frames, zero, None, 0)
    assert none is None
    checks.assert_same_bits(acc, plain, "mean")
    constant = kinds == cases.KINDS.index("constant")
    assert (m2[constant][:, :3] == 0).all() and (m2[constant][:, 3] == 8).all()
    lognormal = kinds == cases.KINDS.index("lognormal")
    mean64, m2_64 = ref.moments64(frames[:, lognormal, :3])
    assert np.allclose(m2[lognormal][:, :3], m2_64, rtol=1e-5) and np.allclose(acc[lognormal][:, :3], mean64, rtol=1e-5)


def test_replay_tree_and_estimate_shapes():
    values = np.random.default_rng(5).uniform(0, 1, 256)
    s = values.copy()
    for stride in (128, 64, 32, 16, 8, 4, 2, 1):
        for t in range(stride):
            s[t] += s[t + stride]
    assert ref.tree_sum(values) == s[0]
    frames, kinds = cases.sample_frames("40x24", 6)
    zero = np.zeros(frames.shape[1:], np.float32)
    acc, m2, _ = ref.accumulate(frames, zero, zero, 0)
    e = ref.estimate(acc, m2, 40, 1e-2)
    assert e["cell_counts"].shape == (2, 3) and e["cell_counts"].sum() + e["cell_nonfinite"].sum() == 40 * 24
    bad = np.isin(kinds, [cases.KINDS.index("huge"), cases.KINDS.index("nan_sample")])
    assert ((e["pixel_map"] == -2) == bad).all() and (e["pixel_map"][:, 40:] == -1).all()
    assert e["cell_counts"][1, 2] == (~bad[16:24, 32:40]).sum()   # the cell clipped on both edges


CONFIG_REFUSALS = [("noise_target", -1.0), ("noise_target", float("nan")), ("noise_target", float("inf")), ("noise_min_samples", 1), ("noise_min_samples", 2.5),
                   ("noise_quantile", 0.0), ("noise_quantile", 1.5), ("noise_quantile", float("nan")), ("noise_floor", 0.0), ("noise_floor", -1.0),
                   ("noise_floor", float("nan")), ("noise_floor", float("inf"))]


def test_config_keys(fresh_config):
    grt = fresh_config
    assert grt.config_get("noise_target") == 0 and grt.config_get("noise_min_samples") == 16
    assert grt.config_get("noise_quantile") == 0.95 and grt.config_get("noise_floor") == float(np.float32(1e-2))
    for key, value in CONFIG_REFUSALS:
        with pytest.raises(KeyError, match=key):
            grt.config_set(**{key: value})
    assert grt.config_get("noise_target") == 0 and grt.config_get("noise_quantile") == 0.95   # a refusal changes nothing
    grt.config_set(noise_target=0.05, noise_min_samples=8, noise_quantile=1.0, noise_floor=0.5)
    assert grt.config_get("noise_target") == float(np.float32(0.05)) and grt.config_get("noise_min_samples") == 8
    assert grt.config_get("noise_quantile") == 1.0 and grt.config_get("noise_floor") == 0.5
    grt.config_reset()
    assert grt.config_get("noise_target") == 0


SUMMARY_CASES = {
    "empty_cells": ([0.0, 3.0, 0.0, 8.0, 1.0], [0, 2, 0, 4, 1], 0.5),
    "one_cell": ([2.5], [5], 0.95),
    "ties": ([1.0, 2.0, 3.0, 1.0, 4.0], [1, 2, 3, 1, 4], 0.5),
    "q_1": ([1.0, 9.0, 4.0, 2.0], [1, 1, 1, 1], 1.0),
    "q_on_a_rank": ([1.0, 2.0, 3.0, 4.0], [1, 1, 1, 1], 0.5),
    "q_just_above_a_rank": ([1.0, 2.0, 3.0, 4.0], [1, 1, 1, 1], 0.5000001),
    "default_quantile_of_20": (list(np.arange(20.0)), [1] * 20, 0.95),
    "tiny_q": ([5.0, 1.0, 3.0], [1, 1, 1], 1e-9),
}


@pytest.mark.parametrize("name", list(SUMMARY_CASES))
def test_noise_summary_against_numpy(grt, name):
    sums, counts, q = SUMMARY_CASES[name]
    status, mean, figure, pixels = grt.noise_summary(sums, counts, q)
    want_mean, want_figure = ref.summary(sums, counts, q)
    assert status == 0 and pixels == sum(counts)
    assert mean == want_mean and figure == want_figure, (mean, want_mean, figure, want_figure)


def test_noise_summary_by_hand_and_refusals(grt):
    assert grt.noise_summary([1.0, 2.0, 3.0, 4.0], [1, 1, 1, 1], 0.5)[2] == 2.0          # rank ceil(0.5 * 4) = 2
    assert grt.noise_summary([1.0, 2.0, 3.0, 4.0], [1, 1, 1, 1], 0.5000001)[2] == 3.0    # just above: the next rank
    assert grt.noise_summary([1.0, 9.0, 4.0, 2.0], [1, 1, 1, 1], 1.0)[2] == 9.0
    assert grt.noise_summary([6.0, 0.0], [3, 0], 0.95)[1:] == (2.0, 2.0, 3)
    assert grt.noise_summary([0.0, 0.0], [0, 0], 0.95) == (1, 0.0, 0.0, 0)               # nothing takes part
    assert grt.noise_summary([], [], 0.95)[0] == 1
    for q in (0.0, -0.1, 1.0001, float("nan")):
        assert grt.noise_summary([1.0], [1], q)[0] == -1
