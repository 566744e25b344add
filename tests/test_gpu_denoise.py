"""The still-image denoiser on the MI355X: the kernels through rt_denoise_images against the float32 restatement of denoise_reference.py,
rt_denoise on a context (Cornell box, 128 x 128), Pathtracer.denoise, save_denoised_image and the command line.

Tolerance. The restatement performs the kernels' float32 operations in their order; what differs is the weight's log2 / exp2 / rcp, which are numpy's on the host
and v_log_f32 / v_exp_f32 / v_rcp_f32 on the device (1 ulp each), under sigma_n = 128. Measured on the MI355X over every case below: the worst per-pixel,
per-channel difference, relative to max(|ref|, 1e-6 x the image mean), is 1.06e-6 on the colour channels and MEASURED_WORST = 7.46e-6 on the variance plane (both at 200 x 150 with 6
iterations) -- below the 1e-5 that tests/test_gpu_svgf_filter.py holds the same weight arithmetic to. TOLERANCE is 4 x the worst of the two, the habit of DESIGN.md 7.5.
Bit-exact: every pixel defined as a copy, the padding's sentinel, and the tiled against the plain pass."""
import subprocess
from ctypes import byref, c_void_p

import numpy as np
import pytest

import denoise_cases as cases
import denoise_reference as ref
from conftest import make_pathtracer

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
MEASURED_WORST = 7.46e-6
TOLERANCE = 4 * MEASURED_WORST

SMALL = ["1x1", "64x8", "70x37", "70x37p128", "257x12"]
PROBE_CASES = [(shape, k) for shape in SMALL for k in range(7)] + [("200x150", 5), ("200x150", 6)]
VARIANTS = {"sigma_n_0": {"sigma_n": 0.0}, "sigma_n_1_z_quarter": {"sigma_n": 1.0, "sigma_z": 0.25}, "sigma_l_0": {"sigma_l": 0.0}, "sigma_z_0": {"sigma_z": 0.0},
            "floors": {"depth_floor": 0.05, "albedo_floor": 0.3}, "constant_w": {}}


@pytest.fixture(scope="module")
def ctx(grt):
    """A bare context: the probe needs no frame, no scene and no estimate."""
    lib = grt.device_lib()
    made = c_void_p()
    assert lib.rt_create(0, byref(made)) == 0, lib.rt_last_error(None)
    yield made
    lib.rt_destroy(made)


_restated = {}


def _restatement(images, key, **given):
    """The float32 restatement and its masks, computed once per case."""
    if key not in _restated:
        p = ref.params(**given)
        _, _, surface, valid, _ = ref.prepare(*[images[k] for k in ("colour", "moments", "albedo", "normal", "position", "fallback", "eye")], images["width"], p, np.float32)
        out = ref.denoise(**images, **given)
        out.setflags(write=False)
        _restated[key] = (out, surface, valid)
    return _restated[key]


def _worst(got, want, surface):
    """The worst relative difference over the surface pixels: (colour channels, variance plane), each relative to max(|want|, 1e-6 x the plane's mean)."""
    if not surface.any():
        return 0.0, 0.0
    g, w = got[surface].astype(np.float64), want[surface].astype(np.float64)
    colour = np.abs(g[:, :3] - w[:, :3]) / np.maximum(np.abs(w[:, :3]), 1e-6 * np.abs(w[:, :3]).mean())
    variance = np.abs(g[:, 3] - w[:, 3]) / np.maximum(np.abs(w[:, 3]), 1e-6 * np.abs(w[:, 3]).mean())
    return float(colour.max()), float(variance.max())


def _check(grt, ctx, images, key, **given):
    width = images["width"]
    want, surface, valid = _restatement(images, key, **given)
    tiled = grt.denoise_images(ctx, **images, tiled=True, sentinel=cases.SENTINEL, **given)
    plain = grt.denoise_images(ctx, **images, tiled=False, sentinel=cases.SENTINEL, **given)
    assert tiled.tobytes() == plain.tobytes(), "the tiled and the plain pass differ"
    assert (tiled.view(np.uint32)[:, width:] == cases.SENTINEL).all(), "the padding columns were written"
    got = tiled[:, :width]
    assert np.isfinite(got).all()
    assert got[~surface].tobytes() == want[~surface].tobytes(), "a pixel defined as a copy differs"
    worst = _worst(got, want, surface)
    print("denoise %s %s: worst relative difference colour %.3g variance %.3g" % (key, given, *worst))
    assert max(worst) <= TOLERANCE, worst
    return got


@pytest.mark.parametrize("shape,iterations", PROBE_CASES, ids=["%s-%d" % c for c in PROBE_CASES])
def test_kernels_against_the_restatement(grt, ctx, shape, iterations):
    """Per-pixel w from 2 to 255, a sky region, a depth discontinuity, mean normals of partly missed pixels, NaN / inf / w < 2 pixels; 0 .. 6 iterations, so that
    every pass is isolated by difference from the run before."""
    images = cases.general(shape)
    got = _check(grt, ctx, images, (shape, iterations), iterations=iterations)
    if iterations == 0:   # prepare and finalize alone: plain IEEE arithmetic, the restatement's bits
        assert got.tobytes() == _restatement(images, (shape, 0), iterations=0)[0].tobytes()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_parameters_reach_the_kernels(grt, ctx, name):
    images = cases.general("70x37", seed=1, constant_w=16 if name == "constant_w" else None)
    got = _check(grt, ctx, images, ("70x37", name), **VARIANTS[name])
    if VARIANTS[name]:
        assert got.tobytes() != grt.denoise_images(ctx, **images)[:, :70].tobytes()


def test_crease_scene_error_falls_on_the_device(grt, ctx):
    images, truth = cases.crease(samples=8, seed=0)
    got = _check(grt, ctx, images, ("crease", 8))
    ratio = cases.relative_rms(images["colour"][:, :70, :3], truth) / cases.relative_rms(got[..., :3], truth)
    print("crease scene, 8 samples: error falls %.2f x" % ratio)
    assert ratio >= 2.0


def test_probe_refusals(grt, ctx):
    images = cases.general("64x8")
    bad = [{"iterations": 7}, {"iterations": -1}, {"sigma_l": -1.0}, {"sigma_n": float("nan")}, {"sigma_z": float("inf")}, {"depth_floor": 0.0}, {"albedo_floor": -1.0},
           {"albedo_floor": float("nan")}]
    for given in bad:
        with pytest.raises(grt.DeviceRefusal, match=list(given)[0]) as refusal:
            grt.denoise_images(ctx, **images, **given)
        assert refusal.value.status == RT_ERROR_INVALID_ARG
    with pytest.raises(grt.DeviceRefusal, match="pitch at least width"):
        grt.denoise_images(ctx, **dict(images, width=65))
    _check(grt, ctx, images, ("64x8", "after refusals"))   # the context is usable


# ---- rt_denoise on a context: cornellbox, 128 x 128, 3 bounces -------------------------------------------------------------------------------------

W, H, SAMPLES = 128, 128, 16
GUIDES = ("AOV_RADIANCE", "AOV_ALBEDO", "AOV_NORMAL", "AOV_POSITION")


def _render(grt, pt, samples, mode="merged"):
    """Samples 0 .. samples - 1 from a fresh progression."""
    grt.set_scheduler(pt.ctx, "slots" if mode == "slots" else "merged")
    pt.invalidate("gpu_config")
    pt.update()
    assert pt.sample_index == 0
    pt.render()
    while pt.sample_index + 1 < samples:
        pt.update()
        pt.render_samples(min(4, samples - pt.sample_index)) if mode == "batches" else pt.render()


def _state(grt, pt):
    """Everything rt_denoise must leave alone: the four accumulators, the moments, the final image."""
    return [pt.read_aov(getattr(grt, name)).copy() for name in GUIDES] + [grt.read_noise_moments(pt.ctx, pt.height, pt.pitch), pt.read_framebuffer().copy()]


def _denoise_own_images(grt, pt, **given):
    colour, albedo, normal, position, moments, final = _state(grt, pt)
    eye = np.array(list(pt.camera().position), np.float32)
    return grt.denoise_images(pt.ctx, colour, moments, albedo, normal, position, final, eye, width=pt.width, sentinel=0, **given)


@pytest.fixture(scope="module")
def cornell(grt):
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, denoise=1)
    yield scene, pt
    grt.set_scheduler(pt.ctx, "merged")
    pt.close(); scene.close(); grt.config_reset()


def test_config_denoise_switches_on_the_estimate_and_the_guides(grt, cornell):
    scene, pt = cornell
    assert grt.get_noise_estimate(pt.ctx)
    mask = pt.device_config().aov_mask
    assert all(mask >> getattr(grt, name) & 1 for name in GUIDES)


@pytest.mark.parametrize("mode", ["merged", "slots"])
def test_rt_denoise_is_the_probe_on_the_contexts_images_and_leaves_the_frame_alone(grt, cornell, mode):
    """(a) the denoised image equals rt_denoise_images fed the context's own read-back images, bit for bit; (b) accumulators, moments and final image are the same
    bits before and after, and a render continued after the call equals the same render without it."""
    scene, pt = cornell
    try:
        _render(grt, pt, SAMPLES, mode)
        before = _state(grt, pt)
        grt.denoise(pt.ctx)
        got = grt.read_denoised(pt.ctx, H, pt.pitch)
        after = _state(grt, pt)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
        assert got[:, :W].tobytes() == _denoise_own_images(grt, pt)[:, :W].tobytes()
        image, variance = pt.denoise()
        assert image.tobytes() == got[:, :W, :3].tobytes() and variance.tobytes() == got[:, :W, 3].tobytes()
        assert (variance > 0).mean() > 0.9 and np.isfinite(image).all()
        for _ in range(4):
            pt.update(); pt.render()
        continued = _state(grt, pt)
        _render(grt, pt, SAMPLES + 4, mode)
        for a, b in zip(continued, _state(grt, pt)):
            assert a.tobytes() == b.tobytes()
    finally:
        grt.set_scheduler(pt.ctx, "merged")


def test_denoised_frame_is_closer_to_a_long_render(grt, cornell):
    """(c) against the same scene at 64 x the samples, the denoised 16-sample frame has the lower relative RMS error."""
    scene, pt = cornell
    _render(grt, pt, SAMPLES * 64, "batches")
    truth = pt.read_framebuffer()[:, :W, :3].astype(np.float64)
    _render(grt, pt, SAMPLES)
    noisy = cases.relative_rms(pt.read_framebuffer()[:, :W, :3], truth)
    denoised = cases.relative_rms(pt.denoise()[0], truth)
    print("cornellbox 128 x 128, 16 samples against 1024: relative RMS error noisy %.4f denoised %.4f (%.2f x)" % (noisy, denoised, noisy / denoised))
    assert denoised < noisy


def test_after_an_adaptive_render(grt, cornell):
    """(d) w is mixed: the sparsely sampled cells enter with their own variance of the mean."""
    scene, pt = cornell
    _render(grt, pt, SAMPLES)
    estimate = pt.noise_estimate()
    means = estimate["cell_sums"] / np.maximum(estimate["cell_counts"], 1)
    chosen = pt.select_adaptive(float(np.quantile(means, 0.9)))   # the noisiest tenth of the cells (and their neighbours) go on
    try:
        assert 0 < chosen["active_cells"] < chosen["cells"]
        for _ in range(2):
            pt.update(); pt.render_samples(4)
    finally:
        pt.adaptive_off()
    w = grt.read_noise_moments(pt.ctx, H, pt.pitch)[:, :W, 3]
    print("adaptive render:", chosen, "w from", w.min(), "to", w.max())
    assert w.min() < w.max()
    grt.denoise(pt.ctx, iterations=4)
    got = grt.read_denoised(pt.ctx, H, pt.pitch)
    assert got[:, :W].tobytes() == _denoise_own_images(grt, pt, iterations=4)[:, :W].tobytes()
    assert np.isfinite(got[:, :W]).all()


def test_refusals_leave_the_previous_image_and_a_usable_context(grt, cornell):
    """(e) one refusal per rule."""
    scene, pt = cornell
    _render(grt, pt, 8)
    grt.denoise(pt.ctx)
    previous = grt.read_denoised(pt.ctx, H, pt.pitch)
    lib = grt.device_lib()

    def refused(status, text, **given):
        with pytest.raises(grt.DeviceRefusal, match=text) as refusal:
            grt.denoise(pt.ctx, **given)
        assert refusal.value.status == status
        assert grt.read_denoised(pt.ctx, H, pt.pitch).tobytes() == previous.tobytes()
    for given, text in (({"iterations": 7}, "iterations"), ({"iterations": -1}, "iterations"), ({"sigma_l": -1.0}, "sigma_l"), ({"sigma_n": float("nan")}, "sigma_n"),
                        ({"sigma_z": float("-inf")}, "sigma_z"), ({"depth_floor": 0.0}, "depth_floor"), ({"albedo_floor": float("inf")}, "albedo_floor")):
        refused(RT_ERROR_INVALID_ARG, text, **given)
    assert lib.rt_denoise(pt.ctx, None) == RT_ERROR_INVALID_ARG and b"NULL params" in lib.rt_last_error(pt.ctx)
    assert lib.rt_read_denoised(pt.ctx, None) == RT_ERROR_INVALID_ARG
    config = pt.device_config()
    for name in ("AOV_ALBEDO", "AOV_NORMAL", "AOV_POSITION"):
        off = type(config).from_buffer_copy(config); off.aov_mask &= ~(1 << getattr(grt, name))
        assert lib.rt_set_config(pt.ctx, byref(off)) == 0
        refused(RT_ERROR_NOT_READY, name[4:])
        assert lib.rt_set_config(pt.ctx, byref(config)) == 0
    svgf = type(config).from_buffer_copy(config); svgf.enable_svgf = 1
    assert lib.rt_set_config(pt.ctx, byref(svgf)) == 0
    refused(RT_ERROR_NOT_READY, "SVGF")
    assert lib.rt_set_config(pt.ctx, byref(config)) == 0
    grt.set_noise_estimate(pt.ctx, False)
    refused(RT_ERROR_NOT_READY, "noise estimate")
    grt.set_noise_estimate(pt.ctx, True)      # the moments start from zeros: w = 0 everywhere
    refused(RT_ERROR_NOT_READY, "no pixel is valid")
    _render(grt, pt, 8)                        # the context is usable: the same render gives the same image
    grt.denoise(pt.ctx)
    assert grt.read_denoised(pt.ctx, H, pt.pitch)[:, :W].tobytes() == previous[:, :W].tobytes()


def test_resize_frees_the_images_and_a_call_after_it_works(grt, cornell):
    """(f)"""
    scene, pt = cornell
    _render(grt, pt, 6)
    grt.denoise(pt.ctx)
    try:
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, 96, 80) == 0
        pt.width, pt.height = 96, 80
        with pytest.raises(grt.DeviceRefusal, match="no denoised image") as refusal:
            grt.read_denoised(pt.ctx, 80, pt.pitch)
        assert refusal.value.status == RT_ERROR_NOT_READY
        _render(grt, pt, 6)
        grt.denoise(pt.ctx, iterations=6)
        got = grt.read_denoised(pt.ctx, 80, pt.pitch)
        assert got.shape == (80, 96, 4) and got.tobytes() == _denoise_own_images(grt, pt, iterations=6).tobytes()
    finally:
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, W, H) == 0
        pt.width, pt.height = W, H


def test_saved_files_decode_to_the_devices_image(grt, cornell, tmp_path):
    scene, pt = cornell
    _render(grt, pt, 8)
    image, _ = pt.denoise(iterations=3)
    for name in ("d.exr", "d.ppm"):
        pt.save_denoised_image(tmp_path / name, iterations=3)
        grt.export_image(tmp_path / ("want_" + name), image)
        assert (tmp_path / name).read_bytes() == (tmp_path / ("want_" + name)).read_bytes()
    pt.save_image(tmp_path / "plain.exr")
    assert (tmp_path / "plain.exr").read_bytes() != (tmp_path / "d.exr").read_bytes()


def test_command_line(grt, tmp_path):
    """pathtracer --denoise: -o receives the denoised image and --denoise-noisy the plain one, both through the exporters, and they decode to what Python writes from
    the same render; with --noise-target --adaptive it runs and filters; with the AO integrator it warns once and writes the plain image.
    (The scene file's film size, 1024 x 1024, wins over -W / -H, as everywhere.)"""
    from test_loaders import CLI
    scene_file = grt.scene_path("cornellbox")
    def run(*options):
        r = subprocess.run([CLI, "-s", scene_file] + [str(o) for o in options], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        return r
    r = run("-N", 8, "--denoise", "--denoise-iterations", 4, "-o", tmp_path / "out.exr", "--denoise-noisy", tmp_path / "noisy.exr")
    assert "Denoised: 4 iterations" in r.stdout and "Wrote %s" % (tmp_path / "noisy.exr") in r.stdout
    grt.config_reset()
    scene = grt.Scene(scene_file)
    w, h = int(grt.config_get("initial_width")), int(grt.config_get("initial_height"))
    grt.config_set(denoise=1, denoise_iterations=4)
    pt = grt.Pathtracer(scene, w, h, device=0)
    try:
        pt.update()
        grt.set_frame_pipelining(pt.ctx, True); grt.set_stream_batch(pt.ctx, 3 * 4 * w * h)   # the burst the command line declares for -N 8
        pt.render()
        while pt.sample_index < 8:
            pt.update(); pt.render_samples(min(4, 8 - pt.sample_index + 1))
        assert pt.sample_index == 8
        pt.save_denoised_image(tmp_path / "want.exr")
        grt.export_image(tmp_path / "want_noisy.exr", pt.read_framebuffer()[:, :w, :3])
    finally:
        pt.close(); scene.close(); grt.config_reset()
    # Two renders in two processes: equal files on all but one of the runs made while this test was written, and on that one a single half-precision value one step
    # apart (the filter itself gives the same bits for the same frame: the tests above). So the decoded images are held to one half-precision step (2^-10
    # relative) in at most one value in 10 000, and their sizes and channels to equality.
    from test_loaders import _parse_exr
    for got_name, want_name in (("out.exr", "want.exr"), ("noisy.exr", "want_noisy.exr")):
        got_channels, got = _parse_exr(tmp_path / got_name)
        want_channels, want = _parse_exr(tmp_path / want_name)
        assert got_channels == want_channels == [("B", 1), ("G", 1), ("R", 1)]
        for name, _ in got_channels:
            assert got[name].shape == want[name].shape == (h, w)
            assert (np.abs(got[name] - want[name]) <= 2.0 ** -10 * np.abs(want[name])).all(), got_name
            assert (got[name] != want[name]).mean() <= 1e-4, got_name
    assert (tmp_path / "out.exr").read_bytes() != (tmp_path / "noisy.exr").read_bytes()
    r = run("-N", 48, "--noise-target", 0.05, "--noise-min-samples", 8, "--adaptive", "--denoise", "-o", tmp_path / "adaptive.exr", "--denoise-noisy", tmp_path / "adaptive_noisy.exr")
    assert "Adaptive:" in r.stdout and "Denoised: 5 iterations" in r.stdout
    assert (tmp_path / "adaptive.exr").read_bytes() != (tmp_path / "adaptive_noisy.exr").read_bytes()
    r = run("-I", "ao", "-N", 3, "--denoise", "-o", tmp_path / "ao.exr")
    assert r.stderr.count("WARNING: --denoise") == 1 and "Denoised" not in r.stdout and "Rendered sample 3" in r.stdout
