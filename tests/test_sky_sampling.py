"""Sky importance sampling without a GPU: the float64 restatement (sky_sampling_reference.py) is a density that integrates to 1 and is
non-zero wherever the bilinear sky is, and the host's `sky_sampling` key takes 0 or (0, 1] and nothing else."""
import math

import numpy as np
import pytest

import sky_sampling_reference as ref


def _skies():
    rng = np.random.default_rng(7)
    black_rows = rng.uniform(0.0, 2.0, (16, 24, 4)).astype(np.float32)
    black_rows[3:6] = 0.0; black_rows[-1] = 0.0
    one = np.array([[[0.3, 0.5, 0.7, 1.0]]], np.float32)
    odd = rng.uniform(0.0, 1.0, (19, 37, 4)).astype(np.float32)
    return {"sun": ref.sun_sky(64, 32, (20, 9)), "black_rows": black_rows, "1x1": one, "37x19": odd}


@pytest.mark.parametrize("name", ["sun", "black_rows", "1x1", "37x19"])
def test_reference_pdf_integrates_to_one(name):
    t = ref.Tables(_skies()[name])
    omega = ref.cell_solid_angle(t.h, t.w)
    assert abs(omega.sum() * t.w - 4.0 * math.pi) < 1e-12
    assert abs((t.pdf * omega[:, None]).sum() - 1.0) < 1e-12
    assert abs(t.p_cell.sum() - 1.0) < 1e-12
    if name == "1x1":
        assert abs(t.pdf[0, 0] - 1.0 / (4.0 * math.pi)) < 1e-15
    # the float32 CDFs end at 1 and never decrease
    assert t.marginal[-1] == 1.0 and np.all(np.diff(t.marginal) >= 0)
    assert np.all(t.conditional[:, -1] == 1.0) and np.all(np.diff(t.conditional, axis=1) >= 0)


@pytest.mark.parametrize("name", ["sun", "black_rows", "1x1", "37x19"])
def test_reference_pdf_covers_the_bilinear_sky(name):
    """Wherever sample_sky returns light, the pdf is not 0 -- also beside the sun and at the edges of black rows, where the bilinear
    filter reaches a bright texel that the cell's own texel does not have."""
    sky = _skies()[name]
    rng = np.random.default_rng(11)
    d = rng.normal(size=(200000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = ref.Tables(sky)
    lit = ref.sample_sky(sky, 1.0, d).max(axis=1) > 0
    assert lit.any()
    assert np.all(t.pdf_of(d)[lit] > 0)


def test_reference_inversion_is_the_pdf():
    """Directions from the inversion lie in the cell they were drawn for, and its histogram follows P_cell."""
    sky = _skies()["black_rows"]
    t = ref.Tables(sky)
    n = 256
    g = (np.arange(n, dtype=np.float64) + 0.5) / n
    uv = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    d, row, col, pdf = t.invert(uv)
    r2, c2 = t.cell(d)
    assert np.mean((r2 == row) & (c2 == col)) > 0.999
    assert np.all(pdf > 0)
    hist = np.bincount(row * t.w + col, minlength=t.h * t.w) / len(uv)
    assert np.abs(hist - t.p_cell.ravel()).max() < 2.0 / len(uv) ** 0.5


def test_irradiance_quadrature_of_a_constant_sky_is_pi():
    sky = np.ones((8, 16, 4), np.float32)
    assert np.allclose(ref.upper_hemisphere_irradiance(sky), math.pi, rtol=1e-12)


@pytest.mark.parametrize("value", [0, 0.5, 1])
def test_config_accepts_a_probability(grt, value):
    grt.config_reset()
    try:
        grt.config_set(sky_sampling=value)
        assert grt.config_get("sky_sampling") == pytest.approx(value)
    finally:
        grt.config_reset()
    assert grt.config_get("sky_sampling") == 0.0


@pytest.mark.parametrize("value", [-0.1, 1.5, float("nan")])
def test_config_rejects_anything_else(grt, value):
    grt.config_reset()
    try:
        with pytest.raises(KeyError, match="sky_sampling"):
            grt.config_set(sky_sampling=value)
        assert grt.config_get("sky_sampling") == 0.0
    finally:
        grt.config_reset()
