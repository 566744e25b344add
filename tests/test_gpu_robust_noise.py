"""The firefly-robust noise estimate on the MI355X: the ROBUST instance of the cells kernel and the selection that takes cell_held, through
rt_estimate_noise_robust_images and rt_select_pixels_robust_images, against the float32 restatement of robust_noise_reference.py; and rt_estimate_noise_robust,
rt_set_noise_robust and the robust rt_select_active_cells on a context (Cornell box, 64 x 64, both schedulers).

Tolerance: none. The restatement performs the kernel's float32 operations in its order and the reduction tree in double; cell sums are compared as doubles, bit for bit."""
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

import adaptive_reference as adaptive
import firefly_cases
import noise_reference as noise
import robust_noise_cases as cases
import robust_noise_reference as ref
from conftest import make_pathtracer

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
FLOOR, TAU = cases.FLOOR, cases.TAU
LIST_SENTINEL = 0xfffffff0


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def contexts(grt):
    """One bare context per probe frame: rt_create + rt_resize, no scene; the pitch is the library's."""
    lib = grt.device_lib()
    lib.rt_resize.argtypes = [c_void_p, c_int, c_int]
    made = {}
    for width, height in cases.SIZES:
        ctx = c_void_p()
        assert lib.rt_create(0, byref(ctx)) == 0, lib.rt_last_error(None)
        assert lib.rt_resize(ctx, width, height) == 0, lib.rt_last_error(ctx)
        made[(width, height)] = (ctx, lib.rt_screen_pitch(ctx))
    yield made
    for ctx, _ in made.values():
        lib.rt_destroy(ctx)


def _assert_estimate(got, want, label):
    assert same_bits(got["cell_sums"], want["cell_sums"]), label + ": cell sums"
    for key in ("cell_counts", "cell_nonfinite", "cell_held"):
        assert np.array_equal(got[key], want[key]), (label, key, got[key], want[key])
    assert same_bits(got["pixel_map"], want["pixel_map"]), label + ": map"
    assert (got["pixels"], got["nonfinite_pixels"], got["held_pixels"]) == (want["pixels"], want["nonfinite_pixels"], want["held_pixels"]), label
    assert got["mean"] == want["mean"], label


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
@pytest.mark.parametrize("size", cases.SIZES, ids=["%dx%d" % s for s in cases.SIZES])
def test_robust_probes_against_the_restatement(grt, contexts, size, tiers):
    """Cells, map, flags and list, bit for bit, with the held fraction at its default and at a value that holds much more; with a resolved image that holds nothing
    back the robust probe gives the plain probe's bits."""
    width, height = size
    ctx, pitch = contexts[size]
    images = cases.probe_case(width, height, pitch, tiers)
    mean, moments, resolved = images["mean"], images["moments"], images["resolved"]
    # the device's own resolve of these images is the restatement's (test_gpu_fireflies.py), the hand-set pixels aside: the probe is handed what a resolve gives
    device = grt.resolve_fireflies_images(ctx, mean, moments, images["tiers"], images["fallback"], width=width, sentinel=firefly_cases.SENTINEL)
    untouched = (np.arange(width * height).reshape(height, width) % 7) != 0
    assert same_bits(device[:, :width][untouched], resolved[:, :width][untouched])
    for tau in (TAU, 0.01):
        want = ref.estimate(mean, moments, resolved, width, FLOOR, tau)
        label = "%dx%d K=%d tau=%g" % (width, height, tiers, tau)
        try:
            got = grt.estimate_noise_robust_images(ctx, height, width, pitch, mean, moments, resolved, floor=FLOOR, held_fraction=tau)
        except grt.DeviceRefusal as refusal:   # (the 1 x 1 frame whose pixel is held or has w < 2: no pixel takes part)
            assert refusal.status == RT_ERROR_NOT_READY and want["pixels"] == 0, label
            continue
        _assert_estimate(got, want, label)
        if width * height >= 256:
            assert want["held_pixels"] > 0 and want["nonfinite_pixels"] > 0 and (want["pixel_map"][:, :width] == -1).any(), label
        counted = want["cell_counts"][want["cell_counts"] > 0]
        means = (want["cell_sums"][want["cell_counts"] > 0] / counted)
        for threshold, dilate in ((float(np.float32(np.median(means))), 0), (float(np.float32(np.median(means))), 1), (0.0, 0), (1e9, 1)):
            hot, active = ref.select(want["cell_sums"], want["cell_counts"], want["cell_nonfinite"], want["cell_held"], width, height, threshold, dilate)
            pixels = adaptive.pixel_list(active, width, height)
            chosen = grt.select_pixels_robust_images(ctx, height, width, pitch, mean, moments, resolved, threshold, floor=FLOOR, held_fraction=tau, dilate=dilate, sentinel=LIST_SENTINEL)
            assert same_bits(chosen["cell_sums"], want["cell_sums"]) and all(np.array_equal(chosen[k], want[k]) for k in ("cell_counts", "cell_nonfinite", "cell_held")), label
            assert np.array_equal(chosen["hot"], hot) and np.array_equal(chosen["active"], active), (label, threshold, dilate)
            assert chosen["hot_cells"] == hot.sum() and chosen["active_cells"] == active.sum() and chosen["list_pixels"] == len(pixels), label
            assert np.array_equal(chosen["list"], pixels) and (chosen["list_tail"] == LIST_SENTINEL).all() and len(chosen["list"]) + len(chosen["list_tail"]) == width * height, label
    nothing = resolved.copy(); nothing[..., 3] = 0.0
    plain = noise.estimate(mean, moments, width, FLOOR)
    if plain["pixels"]:
        got = grt.estimate_noise_robust_images(ctx, height, width, pitch, mean, moments, nothing, floor=FLOOR, held_fraction=TAU)
        device_plain = grt.estimate_noise(ctx, height, width, pitch, floor=FLOOR, mean=mean, moments=moments)
        for key in ("cell_sums", "cell_counts", "cell_nonfinite", "pixel_map"):
            assert same_bits(got[key], device_plain[key]) and same_bits(got[key], plain[key]), key
        assert got["held_pixels"] == 0 and not got["cell_held"].any()


def test_a_cell_of_held_and_nonfinite_pixels_only_is_not_hot(grt, contexts):
    ctx, pitch = contexts[(16, 16)]
    mean = np.ones((16, pitch, 4), np.float32)
    moments = np.ones((16, pitch, 4), np.float32); moments[..., 3] = 4
    resolved = np.zeros((16, pitch, 4), np.float32); resolved[..., 3] = 100.0
    mean[3, :5, 1] = np.nan
    chosen = grt.select_pixels_robust_images(ctx, 16, 16, pitch, mean, moments, resolved, 0.0, floor=FLOOR, held_fraction=TAU, dilate=1, sentinel=LIST_SENTINEL)
    assert chosen["cell_held"].tolist() == [[251]] and chosen["cell_nonfinite"].tolist() == [[5]] and chosen["cell_counts"].tolist() == [[0]]
    assert not chosen["hot"].any() and chosen["list_pixels"] == 0
    moments[7, 7, 3] = 1.0   # a pixel not sampled enough to judge makes it hot
    chosen = grt.select_pixels_robust_images(ctx, 16, 16, pitch, mean, moments, resolved, 1e9, floor=FLOOR, held_fraction=TAU, dilate=0, sentinel=LIST_SENTINEL)
    assert chosen["cell_held"].tolist() == [[250]] and chosen["hot"].all() and chosen["list_pixels"] == 256


def test_probe_refusals(grt, contexts):
    ctx, pitch = contexts[(17, 33)]
    image = np.ones((33, pitch, 4), np.float32)
    for tau in (0.0, 1.0, -0.5, float("nan"), float("inf")):
        for call in (lambda: grt.estimate_noise_robust_images(ctx, 33, 17, pitch, image, image, image, held_fraction=tau),
                     lambda: grt.select_pixels_robust_images(ctx, 33, 17, pitch, image, image, image, 0.1, held_fraction=tau)):
            with pytest.raises(grt.DeviceRefusal, match="held_fraction") as refusal:
                call()
            assert refusal.value.status == RT_ERROR_INVALID_ARG
    with pytest.raises(grt.DeviceRefusal, match="floor"):
        grt.estimate_noise_robust_images(ctx, 33, 17, pitch, image, image, image, floor=0.0)
    with pytest.raises(grt.DeviceRefusal, match="cell_capacity"):
        grt.estimate_noise_robust_images(ctx, 33, 17, pitch, image, image, image, cell_capacity=5)
    with pytest.raises(grt.DeviceRefusal, match="cascade is off") as refusal:   # a bare context has no cascade to resolve
        grt.set_noise_robust(ctx, TAU)
    assert refusal.value.status == RT_ERROR_NOT_READY and grt.get_noise_robust(ctx) == 0.0


# ---- on a context: cornellbox, 64 x 64, 3 bounces; the lowest tier stands for 1 / 64 so that the resolve holds something back ---------------------------------------

W, H, SAMPLES, START = 64, 64, 8, 1.0 / 64.0
LOW = 0.001   # a held fraction at which any tier without full support holds its pixel


def _render(grt, pt, samples, mode="merged"):
    grt.set_scheduler(pt.ctx, "slots" if mode == "slots" else "merged")
    pt.invalidate("gpu_config")
    pt.update()
    assert pt.sample_index == 0
    pt.render()
    while pt.sample_index + 1 < samples:
        pt.update()
        pt.render()


def _state(grt, pt):
    return [pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, H, pt.pitch), grt.read_firefly_cascade(pt.ctx, H, pt.pitch), pt.read_framebuffer().copy()]


@pytest.fixture(scope="module")
def cornell(grt):
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, firefly_filter=1, firefly_start=START)
    yield scene, pt
    grt.set_scheduler(pt.ctx, "merged")
    pt.close(); scene.close(); grt.config_reset()


@pytest.mark.parametrize("mode", ["merged", "slots"])
def test_the_context_calls_are_the_probes_on_its_images_and_leave_the_frame_alone(grt, cornell, mode):
    scene, pt = cornell
    try:
        _render(grt, pt, SAMPLES, mode)
        before = _state(grt, pt)
        mean, moments, tiers, final = before
        plain_off = grt.estimate_noise(pt.ctx, H, W, pt.pitch, floor=FLOOR)
        for tau in (TAU, LOW):
            got = grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch, floor=FLOOR, held_fraction=tau)
            # the resolve it ran counts as a resolve: rt_read_resolved returns it, and it is the resolve of the context's own images
            resolved = grt.read_resolved(pt.ctx, H, pt.pitch)
            assert same_bits(resolved[:, :W], grt.resolve_fireflies_images(pt.ctx, mean, moments, tiers, final, width=W, sentinel=0, start=START)[:, :W])
            for a, b in zip(before, _state(grt, pt)):
                assert a.tobytes() == b.tobytes()
            probe = grt.estimate_noise_robust_images(pt.ctx, H, W, pt.pitch, mean, moments, resolved, floor=FLOOR, held_fraction=tau)
            want = ref.estimate(mean, moments, resolved, W, FLOOR, tau)
            _assert_estimate(got, probe, "context against probe, tau %g (%s)" % (tau, mode))
            _assert_estimate(got, want, "context against restatement, tau %g (%s)" % (tau, mode))
            print("cornellbox %d x %d, %d samples, start 1/64 (%s): tau %g holds %d pixels; mean error plain %.4f, robust %.4f" % (W, H, SAMPLES, mode, tau, got["held_pixels"], plain_off["mean"], got["mean"]))
        assert got["held_pixels"] > 0, "nothing is held even at the low tau: the context test shows nothing"
        # the selection with the mode on: the robust probe's flags and list; off: the plain one's. rt_estimate_noise is the same bits either way.
        threshold = float(np.float32(np.median(want["cell_sums"] / np.maximum(want["cell_counts"], 1))))
        grt.set_noise_robust(pt.ctx, LOW)
        assert grt.get_noise_robust(pt.ctx) == np.float32(LOW)
        plain_on = grt.estimate_noise(pt.ctx, H, W, pt.pitch, floor=FLOOR)
        for key in ("cell_sums", "cell_counts", "cell_nonfinite", "pixel_map"):
            assert same_bits(plain_on[key], plain_off[key]), key
        chosen = grt.select_active_cells(pt.ctx, H, W, threshold, floor=FLOOR, dilate=1)
        listed = grt.read_pixel_list(pt.ctx)
        probe = grt.select_pixels_robust_images(pt.ctx, H, W, pt.pitch, mean, moments, resolved, threshold, floor=FLOOR, held_fraction=LOW, dilate=1)
        hot, active = ref.select(want["cell_sums"], want["cell_counts"], want["cell_nonfinite"], want["cell_held"], W, H, threshold, 1)
        assert np.array_equal(chosen["hot"], probe["hot"]) and np.array_equal(chosen["active"], probe["active"]) and np.array_equal(listed, probe["list"])
        assert np.array_equal(chosen["hot"], hot) and np.array_equal(chosen["active"], active) and 0 < hot.sum() < hot.size
        grt.set_noise_robust(pt.ctx, 0.0)
        assert grt.get_noise_robust(pt.ctx) == 0.0
        chosen = grt.select_active_cells(pt.ctx, H, W, threshold, floor=FLOOR, dilate=1)
        plain_probe = grt.select_pixels_images(pt.ctx, H, W, pt.pitch, mean, moments, threshold, floor=FLOOR, dilate=1)
        assert np.array_equal(chosen["hot"], plain_probe["hot"]) and np.array_equal(grt.read_pixel_list(pt.ctx), plain_probe["list"])
        for a, b in zip(before, _state(grt, pt)):
            assert a.tobytes() == b.tobytes()
        # a render continued after the calls equals the same render without them
        for _ in range(2):
            pt.update(); pt.render()
        continued = _state(grt, pt)
        _render(grt, pt, SAMPLES + 2, mode)
        for a, b in zip(continued, _state(grt, pt)):
            assert a.tobytes() == b.tobytes()
    finally:
        grt.set_noise_robust(pt.ctx, 0.0)
        grt.set_scheduler(pt.ctx, "merged")


def test_refusals_and_what_switches_the_mode_off(grt, cornell):
    scene, pt = cornell
    lib = grt.device_lib()
    _render(grt, pt, 4)

    def refused(call, status, text):
        with pytest.raises(grt.DeviceRefusal, match=text) as refusal:
            call()
        assert refusal.value.status == status
    for tau in (1.0, -0.25, float("nan")):
        refused(lambda: grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch, held_fraction=tau), RT_ERROR_INVALID_ARG, "held_fraction")
        refused(lambda: grt.set_noise_robust(pt.ctx, tau), RT_ERROR_INVALID_ARG, "held_fraction")
    refused(lambda: grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch, floor=float("inf")), RT_ERROR_INVALID_ARG, "floor")
    refused(lambda: grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch, cell_capacity=3), RT_ERROR_INVALID_ARG, "cell_capacity")
    config = pt.device_config()
    svgf = type(config).from_buffer_copy(config); svgf.enable_svgf = 1
    assert lib.rt_set_config(pt.ctx, byref(svgf)) == 0
    refused(lambda: grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch), RT_ERROR_NOT_READY, "SVGF")
    assert lib.rt_set_config(pt.ctx, byref(config)) == 0
    # the mode survives rt_resize as the cascade does
    grt.set_noise_robust(pt.ctx, TAU)
    try:
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, 48, 40) == 0
        assert grt.get_noise_robust(pt.ctx) == np.float32(TAU) and grt.get_firefly_cascade(pt.ctx) is not None
    finally:
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, W, H) == 0
    # zeroed moments: the resolve finds no valid pixel
    grt.set_noise_estimate(pt.ctx, True)
    refused(lambda: grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch), RT_ERROR_NOT_READY, "no pixel is valid")
    refused(lambda: grt.select_active_cells(pt.ctx, H, W, 0.1), RT_ERROR_NOT_READY, "no pixel is valid")
    # switching the cascade off switches the mode off, and it is refused while the cascade is off
    assert grt.get_noise_robust(pt.ctx) == np.float32(TAU)
    grt.set_firefly_cascade(pt.ctx, enable=False)
    assert grt.get_noise_robust(pt.ctx) == 0.0
    refused(lambda: grt.set_noise_robust(pt.ctx, TAU), RT_ERROR_NOT_READY, "cascade is off")
    refused(lambda: grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch), RT_ERROR_NOT_READY, "cascade is off")
    grt.set_firefly_cascade(pt.ctx, start=START)
    grt.set_noise_robust(pt.ctx, TAU)
    grt.set_noise_estimate(pt.ctx, False)   # ... and so does switching the estimate off, which takes the cascade with it
    assert grt.get_noise_robust(pt.ctx) == 0.0 and grt.get_firefly_cascade(pt.ctx) is None
    _render(grt, pt, 4)   # the host puts its configuration back
    assert grt.get_firefly_cascade(pt.ctx) is not None and grt.estimate_noise_robust(pt.ctx, H, W, pt.pitch)["pixels"] > 0


# ---- through the host: the glass / medium scene of scenes.py, 128 x 128 (a rough dielectric holding a medium under two small emitters: caustic paths no light sample reaches) ---

SIZE, GLASS_SAMPLES = 128, 16


def _glass_scene(grt, tmp_path, **config):
    from scenes import write_scene_with_everything
    from test_loaders import _png_bytes
    grt.config_reset()
    scene = grt.Scene(write_scene_with_everything(tmp_path, _png_bytes)); scene.set_sky_scale(0.3)
    grt.config_set(num_bounces=6, **config)
    return scene, grt.Pathtracer(scene, SIZE, SIZE, device=0)


def _render_uniform(grt, pt, samples):
    """Samples 0 .. samples - 1 of a fresh progression, counted from the restart an automatic start makes."""
    pt.invalidate("gpu_config")
    pt.update(); pt.render()
    while True:
        pilot_pending = bool(grt.config_get("firefly_auto_start")) and not pt.firefly_start_measured
        if pt.sample_index + 1 >= samples and not pilot_pending:
            break
        pt.update(); pt.render_samples(min(8, max(samples - pt.sample_index, 1)))   # (after update(): sample_index is the next sample's)
    assert pt.sample_index + 1 == samples


def test_adaptive_render_with_the_robust_estimate(grt, tmp_path):
    """config noise_robust with the automatic start at its default shift: Pathtracer.noise_estimate is the restatement on the read-back images and finds held pixels;
    the selection's flags are numpy's from the robust cell arrays; the passes that follow render the listed pixels and no others."""
    scene, pt = _glass_scene(grt, tmp_path, firefly_filter=1, firefly_auto_start=1, noise_robust=1, noise_target=0.05)
    try:
        _render_uniform(grt, pt, GLASS_SAMPLES)
        assert pt.firefly_start_measured and grt.get_noise_robust(pt.ctx) == np.float32(TAU)
        floor = grt.config_get("noise_floor")
        estimate = pt.noise_estimate()
        mean, moments = pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, SIZE, pt.pitch)
        resolved = grt.read_resolved(pt.ctx, SIZE, pt.pitch)   # the resolve the estimate ran
        want = ref.estimate(mean, moments, resolved, SIZE, floor, TAU)
        plain = noise.estimate(mean, moments, SIZE, floor)
        print("glass / medium scene %d x %d, %d samples, start %g: %d pixels held; mean error plain %.5f, robust %.5f" % (SIZE, SIZE, GLASS_SAMPLES, pt.firefly_start, want["held_pixels"], plain["mean"], want["mean"]))
        assert want["held_pixels"] >= 1, "the scene yields no held pixel at the measured start"
        assert estimate["robust"] and estimate["held_pixels"] == want["held_pixels"] and np.array_equal(estimate["cell_held"], want["cell_held"])
        assert same_bits(estimate["cell_sums"], want["cell_sums"]) and np.array_equal(estimate["cell_counts"], want["cell_counts"]) and estimate["mean"] == want["mean"]
        assert same_bits(pt.noise_map(), want["pixel_map"])
        threshold = float(np.float32(np.quantile(want["cell_sums"] / np.maximum(want["cell_counts"], 1), 0.75)))
        dilate = int(grt.config_get("adaptive_dilate"))
        hot, active = ref.select(want["cell_sums"], want["cell_counts"], want["cell_nonfinite"], want["cell_held"], SIZE, SIZE, threshold, dilate)
        flags = grt.select_active_cells(pt.ctx, SIZE, SIZE, threshold, floor=floor, dilate=dilate)
        assert np.array_equal(flags["hot"], hot) and np.array_equal(flags["active"], active) and 0 < hot.sum() < hot.size
        chosen = pt.select_adaptive(threshold)
        assert (chosen["hot_cells"], chosen["active_cells"]) == (hot.sum(), active.sum())
        listed = grt.read_pixel_list(pt.ctx)
        assert np.array_equal(listed, adaptive.pixel_list(active, SIZE, SIZE)) and chosen["list_pixels"] == len(listed)
        before = moments[:, :SIZE, 3].copy()
        for _ in range(2):
            pt.update(); pt.render_samples(4)
        pt.adaptive_off()
        after = grt.read_noise_moments(pt.ctx, SIZE, pt.pitch)[:, :SIZE, 3]
        in_list = np.zeros(SIZE * SIZE, bool); in_list[listed] = True
        assert np.array_equal(after - before, np.where(in_list.reshape(SIZE, SIZE), 8, 0))   # the sample-count map is consistent with the list
        assert np.allclose(grt.read_firefly_cascade(pt.ctx, SIZE, pt.pitch)[:, :, :SIZE, 3].sum(axis=0), after, atol=1e-3)
        # with the key off the host goes back to the plain estimate
        pt.set_noise_estimate(True, robust=False)
        pt.update()
        assert grt.get_noise_robust(pt.ctx) == 0.0 and not pt.noise_estimate()["robust"]
    finally:
        pt.close(); scene.close(); grt.config_reset()


def test_robust_without_the_filter_warns_and_keeps_the_plain_estimate(grt, capfd):
    scene, pt = make_pathtracer(grt, "cornellbox", 64, 64, 0, num_bounces=3, noise_robust=1, noise_target=0.05)
    try:
        for _ in range(4):
            pt.render(); pt.update()
        estimate = pt.noise_estimate()
        assert not estimate["robust"] and estimate["held_pixels"] == 0 and grt.get_noise_robust(pt.ctx) == 0.0
        assert capfd.readouterr().err.count("WARNING: noise_robust needs the firefly filter") == 1
    finally:
        pt.close(); scene.close(); grt.config_reset()


ERROR_LONG = 1024


def test_the_resolved_image_at_the_automatic_start_is_closer_to_a_long_render_than_the_mean(grt, tmp_path):
    """As test_gpu_fireflies.py's error test, with no scene-specific number: 16 samples against 1 024, the start taken from the frame's own exposure at the default
    shift. The resolved image's relative RMS error is at or below the mean's. The comparison with firefly_start = 1 is printed; it is asserted only where the gap
    exceeds the run-to-run spread DESIGN.md 7.10 measured for this scene at 16 samples (0.008).
    Measured (profiles/fireflies.txt): the automatic start is 1/8 (median exponent -3, shift 0); relative RMS error 0.08333 for the mean, 0.08311 resolved at the
    automatic start (1.003 x), 0.08328 resolved at firefly_start = 1 (1.001 x): a gap of 0.0002, far inside the spread, so the last comparison is printed and not asserted."""
    scene, pt = _glass_scene(grt, tmp_path, firefly_filter=1, firefly_auto_start=1)
    try:
        _render_uniform(grt, pt, ERROR_LONG)
        truth = pt.read_framebuffer()[:, :SIZE, :3].astype(np.float64)
        _render_uniform(grt, pt, GLASS_SAMPLES)
        start = pt.firefly_start
        mean = pt.read_framebuffer()[:, :SIZE, :3].astype(np.float64)
        resolved, _ = pt.resolve_fireflies()
        pt.set_firefly_filter(True, auto_start=False)
        _render_uniform(grt, pt, GLASS_SAMPLES)
        assert pt.firefly_start == 1.0 and np.array_equal(pt.read_framebuffer()[:, :SIZE, :3].astype(np.float64), mean)   # the same frame: the filter changes no sample
        default, _ = pt.resolve_fireflies()
        errors = [firefly_cases.relative_rms(image, truth) for image in (mean, resolved, default)]
        print("glass / medium scene %d x %d, %d samples against %d: relative RMS error mean %.5f, resolved at the automatic start %g %.5f (%.3f x), resolved at firefly_start 1 %.5f (%.3f x)"
              % (SIZE, SIZE, GLASS_SAMPLES, ERROR_LONG, errors[0], start, errors[1], errors[0] / errors[1], errors[2], errors[0] / errors[2]))
        assert start != 1.0
        assert errors[1] <= errors[0]
        if errors[2] - errors[1] > 0.008:
            assert errors[1] < errors[2]
    finally:
        pt.close(); scene.close(); grt.config_reset()


def test_command_line_with_all_four_flags(grt, tmp_path):
    """pathtracer --noise-target --adaptive --firefly-filter --denoise with the automatic start and the robust estimate: it writes its files and prints the start it
    chose, the figure with the name of the estimate, and the held pixels."""
    import re
    import subprocess
    from test_loaders import CLI
    r = subprocess.run([CLI, "-s", grt.scene_path("cornellbox"), "-N", "40", "--noise-target", "0.05", "--noise-min-samples", "8", "--adaptive", "--firefly-filter", "--firefly-start", "4", "--firefly-auto-start",
                        "--noise-robust", "--denoise", "-o", str(tmp_path / "out.exr"), "--noise-map", str(tmp_path / "noise.exr")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    start = re.search(r"Firefly start: (\S+) from the exposure of 4 pilot samples \(median exponent (-?\d+) with shift 0; 4 samples discarded\)", r.stdout)
    assert start and float(start.group(1)) == 2.0 ** int(start.group(2)), r.stdout
    assert "Firefly filter: 6 tiers from %s," % start.group(1) in r.stdout
    assert re.search(r"Noise \(firefly-robust, \d+ pixels held\): figure ", r.stdout) and "Adaptive:" in r.stdout and "Denoised: 5 iterations" in r.stdout, r.stdout
    assert all("Wrote %s" % (tmp_path / n) in r.stdout and (tmp_path / n).stat().st_size > 0 for n in ("out.exr", "noise.exr"))
