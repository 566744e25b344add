"""The oracle's SVGF / TAA filter stage against the float64 restatement (tests/svgf_reference.py), on the synthetic frame
sequences of tests/svgf_cases.py fed through Frame.svgf_inputs() / Frame.filter_frame(). No GPU needed.

What has to agree:
* history lengths, exactly -- every decision (previous position, consistency, sky, taps in the image, history counts) is
  formed in float32 by both;
* the images, within F32_BOUND per pixel and channel, relative to max(|float64 value|, 0.1 x the channel's mean over the
  image): what float32 rounding leaves of the stage. Measured on these cases: at most 1.7e-5 (fireflies of 1e4 next to values
  of 1, in sums of up to 49 terms), 2e-6 everywhere else;
* the variances (.w of the two histories), within F32_BOUND of the pixel's E[x^2] (floored at 0.1 x its mean): they are the
  difference E[x^2] - E[x]^2 and carry the rounding of the larger term;
* the TAA history and, with TAA on, the final image, within F32_BOUND after the per-pixel allowance of the YCoCg clamp
  (svgf_reference.Filter.taa_slack at the float32 rounding): the clamp's sigma^2 cancels in a smooth neighbourhood, and only
  there does float32 lose more than a few ulps;
* the history of normals and depths: the octahedral g-buffer texels, bit for bit;
* with TAA on, the TAA history and the final image bit for bit against svgf_reference.taa_resolve32, the resolve replayed in
  float32 from the oracle's own tone-mapped colour and history -- the check of the resolve that needs no allowance.
"""
import numpy as np
import pytest

import svgf_cases
import svgf_reference
from conftest import make_pathtracer

F32_BOUND = 5e-5


def run_case(grt, oracle, case):
    """Yields (frame, oracle state, float64 state, reference) for every frame of the case."""
    scene, pt = make_pathtracer(grt, "cornellbox", case.width, case.height, -1, **svgf_cases.config_kwargs(case))
    try:
        run = svgf_cases.OracleRun(oracle, oracle.SceneView(pt), case)
        ref = svgf_reference.Filter(case.width, case.height, case.pitch, case.config)
        for f, inputs in enumerate(case.frames):
            got = run.step(inputs, f)
            ref.frame(inputs, f)
            yield f, got, svgf_cases.reference_state(ref), ref
    finally:
        pt.close()
        scene.close()


@pytest.mark.parametrize("case", svgf_cases.cases(), ids=repr)
def test_oracle_filter_matches_the_float64_restatement(grt, oracle, case):
    W = case.width
    young = []
    taa_prev = np.zeros((case.height, case.pitch, 4), np.float32)
    for f, got, want, ref in run_case(grt, oracle, case):
        if case.config.enable_taa:   # the oracle's resolve, replayed in float32 from its own inputs: bit for bit
            history, final = svgf_reference.taa_resolve32(got["taa_current"], taa_prev, case.frames[f]["screen_position_prev"], f, W, case.height)
            assert np.array_equal(got["taa_history"][:, :W], history[:, :W]) and np.array_equal(got["final"][:, :W], final[:, :W]), (case, f)
            taa_prev = got["taa_history"]
        assert np.array_equal(got["history_length"][:, :W], want["history_length"][:, :W]), (case, f)
        assert np.array_equal(got["history_normal_and_depth"], want["history_normal_and_depth"]), (case, f)
        errors = svgf_cases.state_errors(got, want, W, ref.taa_slack())
        assert max(errors.values()) <= F32_BOUND, (case, f, errors)
        young.append(int((got["history_length"][:, :W] < 4).sum()))
    # the sequences do what they are for: histories grow past 4, and the cases with events reset some of them
    if case.n_frames >= 5 and case.height > 1:
        assert young[4] < young[0], young
    if "strip" in case.events:
        assert young[5] > young[4], young


def test_the_cases_cover_the_decisions_they_are_named_for(grt, oracle):
    """The depth step sits on the threshold (|12 - 10| == 2.0 is inconsistent), the half-pixel pan makes the right-hand
    bilinear weights exactly zero, the first frame at 256 x 64 has more young pixels than kernel_svgf_variance_listed has
    waves, and the border motion sends previous positions into (-0.5, 0.5), where reprojection's C truncation and floor
    differ, and into (-1.5, -0.5), where TAA finds a single tap in the image."""
    by_name = {c.name: c for c in svgf_cases.cases()}
    case = by_name["exact_64x48"]
    lengths = [got["history_length"][..., 0].copy() for _, got, _, _ in run_case(grt, oracle, case)]
    patch = (slice(case.height - 6, case.height - 3), slice(3, 7))   # the patch (10 -> 12 at frame 3) where no fallback tap leaves it
    assert (lengths[2][patch] == 2).all() and (lengths[3][patch] == 0).all() and (lengths[4][patch] == 1).all()
    half = by_name["half_pixel_64x48_it2"].frames[1]["screen_position_prev"][..., 0]
    s_prev = (np.float32(0.5) + np.float32(0.5) * half[:, :64]) * np.float32(64)
    assert (s_prev - np.floor(s_prev) == 0).all()
    young = [got["history_length"][..., 0] < 4 for _, got, _, _ in run_case(grt, oracle, by_name["zoom_256x64_it1_no_taa"])]
    depth0 = by_name["zoom_256x64_it1_no_taa"].frames[0]["normal_and_depth"][..., 2]
    assert (young[0] & (depth0 != 0)).sum() > 2048 * 4   # more listed pixels than the listed variance pass has waves: its stride loop
    border = by_name["exact_65x33_border"]
    for axis, size in ((0, 65), (1, 33)):
        first = [fr["screen_position_prev"][0, 0, axis] for fr in border.frames[1:]]
        s = [(np.float32(0.5) + np.float32(0.5) * v) * np.float32(size) for v in first]
        assert any(np.trunc(v - np.float32(0.5)) != np.floor(v - np.float32(0.5)) for v in s)   # reprojection
        assert any((v > -1.5) & (v < -0.5) for v in s)   # TAA: left of / above the image, resolved from its one tap in the image
