"""The still-image denoiser without a GPU: the float32 restatement of denoise_reference.py against its float64 text, what the definition
guarantees by construction, the error reduction on the synthetic crease scene, the config keys, the command line's argument refusals and the entry points'
NULL checks.

The float32 / float64 comparison is made STEP BY STEP -- prepare, then every pass on the restatement's own input to that pass -- because a weight is
exp(-x) of differences of its inputs: fed inputs that already differ, two evaluations drift apart by the condition number |l_p - l_q| * denom per pass, which
says nothing about the arithmetic. On equal inputs the distance has a first-order bound in the unit roundoff u = 2^-24, written out term by term in
denoise_reference.one_pass(want_bound=True). The cases (denoise_cases.py) keep v away from 0 so that the bound stays small enough to mean something: its largest
value over the cases below is below 1e-4 of a demodulated colour of order 1 (asserted), and the restatement stays within a third of it."""
import subprocess
from ctypes import byref, c_size_t

import numpy as np
import pytest

import denoise_cases as cases
import denoise_reference as ref

U = ref.EPS32
BOUND_CASES = [("70x37", {}), ("70x37p128", {"sigma_n": 1.0, "sigma_z": 0.25}), ("64x8", {"sigma_l": 1.0, "depth_floor": 1e-3}), ("257x12", {"sigma_n": 0.0}), ("200x150", {"iterations": 6}),
               ("1x1", {})]


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.spacing(np.abs(np.asarray(b, np.float32)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("shape,given", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_restatement_against_float64_step_by_step(shape, given):
    images = cases.general(shape)
    p = ref.params(**given)
    width = images["width"]
    args = [images[k] for k in ("colour", "moments", "albedo", "normal", "position", "fallback", "eye")]
    iv32, g32, s32, v32, a32 = ref.prepare(*args, width, p, np.float32)
    iv64, g64, s64, v64, a64 = ref.prepare(*args, width, p, np.float64)
    assert (s32 == s64).all() and (v32 == v64).all() and iv32.dtype == np.float32 and g32.dtype == np.float32
    if width * cases.SHAPES[shape][1] >= 64:
        assert s32.any() and (~v32).sum() >= 6 and (v32 & ~s32).any()   # surfaces, invalid pixels and sky all occur
    # prepare: I is one division of a float32 by a float32 (u); n three products by 1 / sqrt of a 5-operation sum (5 u); z a 5-operation sum under a sqrt (4 u);
    # v = (luminance of three sqrt of two divisions and a product)^2: 3 + 1 each, 3 for the luminance, 2 for the square: 12 u
    s = s32
    assert (np.abs(iv32[s][:, :3] - iv64[s][:, :3]) <= 1.01 * U * np.abs(iv64[s][:, :3])).all()
    assert (np.abs(g32[s][:, :3] - g64[s][:, :3]) <= 5 * U).all() and (np.abs(g32[s][:, 3] - g64[s][:, 3]) <= 4 * U * g64[s][:, 3]).all()
    assert (np.abs(iv32[s][:, 3] - iv64[s][:, 3]) <= 12 * U * iv64[s][:, 3]).all() and (iv64[s][:, 3] > 0).all()
    assert (iv32[~s] == iv64[~s]).all() and (g32[~s] == 0).all()
    states = []
    out32 = ref.denoise(**images, states=states, **given)
    assert out32.dtype == np.float32 and len(states) == p["iterations"] + 1
    worst = 0.0
    for k, (iv, guide, surface) in enumerate(states[:-1]):
        want, bound_i, bound_v = ref.one_pass(iv.astype(np.float64), guide.astype(np.float64), surface, 1 << k, p, np.float64, want_bound=True)
        got = states[k + 1][0].astype(np.float64)
        err_i, err_v = np.abs(got[..., :3] - want[..., :3]), np.abs(got[..., 3] - want[..., 3])
        assert (err_i <= bound_i).all() and (err_v <= bound_v).all(), (k, float((err_i / np.maximum(bound_i, 1e-300)).max()), float((err_v / np.maximum(bound_v, 1e-300)).max()))
        assert (got[~surface] == iv[~surface]).all()
        worst = max(worst, float(bound_i.max()))
    assert worst < 1e-4   # the bound means something
    # the end-to-end distance is reported, not bounded (see the module text)
    out64 = ref.denoise(**images, dtype=np.float64, **given)
    print("end to end, relative to the image mean:", float(np.abs(out32[s][:, :3] - out64[s][:, :3]).max() / max(1e-30, out64[s][:, :3].mean())) if s.any() else 0.0)


def test_zero_iterations_return_the_mean():
    images = cases.general("70x37")
    for dtype in (np.float32, np.float64):
        out = ref.denoise(**images, dtype=dtype, iterations=0)
        _, _, surface, valid, _ = ref.prepare(*[images[k] for k in ("colour", "moments", "albedo", "normal", "position", "fallback", "eye")], 70, ref.params(), dtype)
        colour = images["colour"][:, :70, :3]
        assert (_ulps(out[surface][:, :3], colour[surface]) <= 2).all()       # C / a * a: two roundings
        assert (out[surface][:, 3] > 0).all()


def test_constant_image_has_the_kernel_weights_exactly():
    """Constant colour, normal and depth: every exponent is 0, every weight 2^-(|i|+|j|); I stays constant and v' is the convolution of v with the squared kernel."""
    images = cases.flat()
    width, height = 40, 24
    for dtype in (np.float32, np.float64):
        states = []
        ref.denoise(**images, dtype=dtype, states=states, iterations=3)
        for k in range(3):
            v = states[k][0][..., 3].astype(np.float64)
            step = 1 << k
            num, den = v.copy(), np.ones((height, width))
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    if i or j:
                        kw = 0.5 ** (abs(i) + abs(j))
                        shifted, inside = ref._shift(v, i * step, j * step)
                        num += kw * kw * shifted; den += kw * inside
            got = states[k + 1][0].astype(np.float64)
            assert np.allclose(got[..., 3], num / den ** 2, rtol=(24 * U if dtype == np.float32 else 1e-14), atol=0)
            assert (_ulps(got[..., :3], states[0][0][..., :3]) <= 2).all()


def test_orthogonal_normals_do_not_exchange_anything():
    """Two regions whose normals are orthogonal: every weight across the crease is exactly 0 (log2(0) = -inf), so no colour and no variance is averaged across it.
    Tripling one side's colours leaves the other side bit-identical after ONE pass at the default parameters, and after all five when sigma_l = 0.
    With sigma_l > 0 and two or more passes the sides do meet, in one place: the 3 x 3 blur of v that scales the luminance weight is not edge-stopped (it is
    svgf_atrous_neighbourhood's), the first pass changes v' on the tripled side (its weights depend on its colours), and the second pass's blur carries that into the
    denom of the column beside the crease. That follows from the definition; its size is printed here and it is a known limit in DESIGN.md 7.9."""
    images, _ = cases.crease()
    changed = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in images.items()}
    changed["colour"][:, 35:70, :3] *= np.float32(3.0)
    for dtype in (np.float32, np.float64):
        for given in ({"iterations": 1}, {"sigma_l": 0.0}):
            a, b = ref.denoise(**images, dtype=dtype, **given), ref.denoise(**changed, dtype=dtype, **given)
            assert (a[:, :35].view(np.uint8) == b[:, :35].view(np.uint8)).all(), given
            assert not (a[:, 35:] == b[:, 35:]).all()
        states_a, states_b = [], []
        a, b = ref.denoise(**images, dtype=dtype, states=states_a), ref.denoise(**changed, dtype=dtype, states=states_b)
        assert (states_a[1][0][:, :35] == states_b[1][0][:, :35]).all() and (states_a[2][0][:, :34] == states_b[2][0][:, :34]).all()   # pass 1 reaches column 34 alone
        print("five passes, sigma_l 4, through the blur of v: largest relative change on the untouched side %.3g" % float(np.abs(a[:, :35, :3] / b[:, :35, :3] - 1).max()))
    assert ref.denoise(**images, sigma_n=0.0, iterations=1).tobytes() != ref.denoise(**images, iterations=1).tobytes()   # (with sigma_n = 0 the crease is no edge)


def test_invalid_and_sky_pixels_come_back_as_defined_and_touch_nothing():
    images = cases.general("70x37")
    out = ref.denoise(**images)
    _, _, surface, valid, _ = ref.prepare(*[images[k] for k in ("colour", "moments", "albedo", "normal", "position", "fallback", "eye")], 70, ref.params(), np.float32)
    sky = valid & ~surface
    assert (out[sky][:, :3] == images["colour"][:, :70][sky][:, :3]).all() and (out[sky][:, 3] == 0).all()
    assert (out[~valid][:, :3] == images["fallback"][:, :70][~valid][:, :3]).all() and (out[~valid][:, 3] == -1).all()
    assert np.isfinite(out).all() and (out[surface][:, 3] > 0).all()
    changed = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in images.items()}
    changed["colour"][:, :70][sky] = np.float32(77.0); changed["fallback"][:, :70][~valid] = np.float32(5.0)
    changed["position"][:, :70][sky] = np.float32(9.0)
    again = ref.denoise(**changed)
    assert (again[surface].view(np.uint8) == out[surface].view(np.uint8)).all()


@pytest.mark.parametrize("samples", [8, 32])
def test_error_falls_by_half_on_the_crease_scene(samples):
    """Relative RMS error against the truth, noisy over denoised, seeds 0..2: at least 2 x each; and out / albedo has no edge at the albedo's cell borders beyond
    what the filtered irradiance has there (the albedo is divided out before the filter and multiplied back after it)."""
    for seed in range(3):
        images, truth = cases.crease(samples=samples, seed=seed)
        noisy = cases.relative_rms(images["colour"][:, :70, :3], truth)
        for dtype in (np.float64, np.float32):
            out = ref.denoise(**images, dtype=dtype)
            ratio = noisy / cases.relative_rms(out[..., :3], truth)
            print("samples %d seed %d %s: %.2f x" % (samples, seed, np.dtype(dtype).name, ratio))
            assert ratio >= 2.0, ratio
        albedo, irradiance, _, _ = cases.crease_truth(70, 37)
        quotient = out[..., :3].astype(np.float64) / albedo
        border = (albedo[:, 1:, 0] != albedo[:, :-1, 0]) & (np.arange(1, 70) != 35)[None, :]    # cell borders in x, but not the crease
        inner = (albedo[:, 1:, 0] == albedo[:, :-1, 0]) & (np.arange(1, 70) != 35)[None, :]
        jump = np.abs(quotient[:, 1:] - quotient[:, :-1]).mean(axis=-1)
        assert jump[border].mean() <= 1.25 * jump[inner].mean(), (jump[border].mean(), jump[inner].mean())


CONFIG_REFUSALS = [("denoise", 2), ("denoise", -1), ("denoise", float("nan")), ("denoise_iterations", 7), ("denoise_iterations", -1), ("denoise_iterations", 2.5),
                   ("denoise_iterations", float("nan")), ("denoise_sigma_l", -1.0), ("denoise_sigma_l", float("inf")), ("denoise_sigma_n", float("nan")), ("denoise_sigma_n", -0.5),
                   ("denoise_sigma_z", -1e-3), ("denoise_sigma_z", float("inf"))]


def test_config_keys(fresh_config):
    grt = fresh_config
    defaults = {"denoise": 0, "denoise_iterations": 5, "denoise_sigma_l": 4.0, "denoise_sigma_n": 128.0, "denoise_sigma_z": 1.0}
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key
    for key, value in CONFIG_REFUSALS:
        with pytest.raises(KeyError, match=key):
            grt.config_set(**{key: value})
    for key, value in defaults.items():
        assert grt.config_get(key) == value, key   # a refusal changes nothing
    grt.config_set(denoise=1, denoise_iterations=0, denoise_sigma_l=0.0, denoise_sigma_n=2.5, denoise_sigma_z=0.5)
    assert [grt.config_get(k) for k in defaults] == [1, 0, 0.0, 2.5, 0.5]
    grt.config_set(denoise_iterations=6)
    assert grt.config_get("denoise_iterations") == 6
    grt.config_reset()
    assert grt.config_get("denoise") == 0 and grt.config_get("denoise_iterations") == 5
    assert {k: ref.DEFAULTS[k] for k in grt.DENOISE_DEFAULTS} == grt.DENOISE_DEFAULTS


def test_command_line_refuses_at_argument_parsing(grt):
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    def refused(*options):
        r = subprocess.run([CLI, "-s", scene_file] + [str(o) for o in options], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Initialization" not in r.stdout, r.stdout + r.stderr
        return r.stderr
    assert "need --denoise" in refused("--denoise-iterations", 3)
    assert "need --denoise" in refused("--denoise-noisy", "noisy.exr")
    assert "--denoise-iterations must be between 0 and 6" in refused("--denoise", "--denoise-iterations", 7)
    assert "--denoise-iterations must be between 0 and 6" in refused("--denoise", "--denoise-iterations", -1)
    assert "invalid integer" in refused("--denoise", "--denoise-iterations", "many")
    assert "names the output file" in refused("--denoise", "-o", "same.exr", "--denoise-noisy", "same.exr")
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(option in r.stdout for option in ("--denoise ", "--denoise-iterations", "--denoise-noisy"))


def test_entry_points_refuse_a_null_context(grt):
    lib = grt.device_lib()
    record = grt.denoise_params()
    image = np.zeros((1, 32, 4), np.float32)
    eye = np.zeros(3, np.float32)
    ms, count = np.zeros(8, np.float32), c_size_t(0)
    calls = {"rt_denoise": lambda: lib.rt_denoise(None, byref(record)),
             "rt_read_denoised": lambda: lib.rt_read_denoised(None, image.ctypes.data),
             "rt_denoise_timed": lambda: lib.rt_denoise_timed(None, byref(record), 1, ms.ctypes.data, 8, byref(count)),
             "rt_denoise_images": lambda: lib.rt_denoise_images(None, 1, 1, 32, *[image.ctypes.data] * 6, eye.ctypes.data, byref(record), 1, image.ctypes.data)}
    for name, call in calls.items():
        assert call() == -1
        assert lib.rt_last_error(None).decode() == name + ": NULL context"
    with pytest.raises(TypeError, match="unknown denoise parameter"):
        grt.denoise_params(sigma=1.0)
    with pytest.raises(ValueError):
        grt.denoise_params(iterations=2.5)
