"""The firefly filter on the MI355X: the cascade accumulate kernels through rt_accumulate_cascade_frames and the resolve kernels through
rt_resolve_fireflies_images against the float32 restatement of firefly_reference.py, and rt_set_firefly_cascade / rt_resolve_fireflies on a context (Cornell box,
128 x 128).

Tolerance: none. The restatement performs the kernels' float32 operations in their order -- IEEE +, -, *, /, fminf / fmaxf, no contraction --, and the device
gives the same bits over every case below: tiers, resolved image, padding. Mean, moments and final image are compared with what the plain probes
(rt_accumulate_frames, rt_accumulate_list_frames) leave on the same input, bit for bit."""
import subprocess
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

import firefly_cases as cases
import firefly_reference as ref
from conftest import make_pathtracer

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
SENTINEL = cases.SENTINEL


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@pytest.fixture(scope="module")
def contexts(grt):
    """One bare context per probe frame: rt_create + rt_resize, no scene (the accumulate launches need none); the pitch is the library's."""
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


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
@pytest.mark.parametrize("size", cases.SIZES, ids=["%dx%d" % s for s in cases.SIZES])
def test_cascade_accumulate_against_the_restatement_and_the_plain_kernels(grt, contexts, size, tiers):
    """The batch (slots), merged and list forms from fold index 0, 1 and 5, four samples each (the merged forms as two submissions of two): samples on every tier
    boundary, one step below and above it, 0, negative, above the top tier, NaN and inf. What lies outside the set or the list, and the padding, keeps its bits."""
    width, height = size
    ctx, pitch = contexts[size]
    assert pitch >= width
    inside = np.zeros((height, pitch), bool); inside[:, :width] = True
    for first in cases.STARTS:
        frames = cases.sample_frames(width, height, pitch, 4, tiers, seed=first)
        acc, m2, running = cases.running_state(width, height, pitch, tiers, max(first, 2))
        for form in ("batch", "merged", "list"):
            merged = form != "batch"
            # the launch's first fold index: the sample's, or (list) the pixel's own w + 1. At 0 and 1 the tiers are zeroed first: the sentinel must not show through
            resets = first + (form == "list") <= 1
            state = np.tile(cases.sentinel_image((1, height, pitch, 4)), (tiers, 1, 1, 1)) if resets else running
            args = dict(first_sample=[first, first + 2] if merged else first, sample_count=[2, 2] if merged else None, merged=merged, sentinel=SENTINEL)
            if form == "list":
                listed = np.flatnonzero(((np.arange(width * height) * 7 + first) % 3 != 0) | (width * height == 1)).astype(np.uint32)[::-1].copy()   # partial, unordered
                covered = np.zeros((height, pitch), bool); covered[listed // width, listed % width] = True
                m2_in = m2.copy(); m2_in[:, :width, 3] = first   # the list form folds with the pixel's own index w + 1: 1, 2, 6
                acc_in = acc.copy() if first else np.where(inside[..., None], np.float32(0), acc)   # (w = 0: the mean takes the sample; what it held does not matter, NaN aside)
                got = grt.accumulate_cascade_frames(ctx, frames, acc_in, m2_in, state, pixels=listed, **args)
                plain = grt.accumulate_list_frames(ctx, frames, acc_in, m2_in, listed, [2, 2], first_sample=[first, first + 2], sentinel=SENTINEL)
                want = ref.accumulate(frames, state, m2_in[..., 3].astype(np.float64) + 1, 1.0, np.float32, pixels=covered)
            else:
                covered, m2_in, acc_in = inside, m2, acc
                got = grt.accumulate_cascade_frames(ctx, frames, acc_in, m2_in, state, **args)
                plain = grt.accumulate_frames(ctx, frames, acc_in, m2_in, **args)
                want = ref.accumulate(frames, state, first, 1.0, np.float32, pixels=covered)
            got_frames, got_acc, got_m2, got_tiers, got_final = got
            label = "%dx%d K=%d first=%d %s" % (width, height, tiers, first, form)
            assert same_bits(got_frames, plain[0]) and same_bits(got_acc, plain[1]) and same_bits(got_m2, plain[2]) and same_bits(got_final, plain[3]), label
            assert same_bits(got_tiers[:, ~covered], state[:, ~covered]), label + ": a pixel outside the set was written"
            assert np.isfinite(got_tiers[:, covered]).all(), label
            assert same_bits(got_tiers, want), label + ": worst difference %g" % np.nanmax(np.abs(got_tiers[:, covered].astype(np.float64) - want[:, covered]))
            w_sum = got_tiers[:, covered][..., 3].sum(axis=0, dtype=np.float64)
            finite = np.isfinite(frames[..., :3].sum(axis=-1))[:, covered]
            if resets:   # the tiers count the finite samples the mean holds: all four, or (from sample 0, which sample 1 overwrites) the last three
                kept = finite[1:].sum(axis=0) if first == 0 and form != "list" else finite.sum(axis=0)
                assert np.allclose(w_sum, kept, atol=1e-5), label


@pytest.fixture(scope="module")
def ctx(grt):
    """A bare context: the resolve probe needs no frame and no scene."""
    lib = grt.device_lib()
    made = c_void_p()
    assert lib.rt_create(0, byref(made)) == 0, lib.rt_last_error(None)
    yield made
    lib.rt_destroy(made)


@pytest.mark.parametrize("tiers", cases.TIER_COUNTS)
@pytest.mark.parametrize("size", cases.SIZES, ids=["%dx%d" % s for s in cases.SIZES])
def test_resolve_kernels_against_the_restatement(grt, ctx, size, tiers):
    width, height = size
    pitch = (width + 32) // 32 * 32 + (32 if width > 64 else 0)
    assert pitch > width
    images = cases.resolve_case(width, height, pitch, tiers)
    for support in (4.0, 1.5):
        parts = {}
        want = ref.resolve(**images, width=width, support=support, dtype=np.float32, parts=parts)
        tiled = grt.resolve_fireflies_images(ctx, **images, width=width, tiled=True, sentinel=SENTINEL, support=support)
        plain = grt.resolve_fireflies_images(ctx, **images, width=width, tiled=False, sentinel=SENTINEL, support=support)
        assert tiled.tobytes() == plain.tobytes(), "the tiled and the plain kernel differ"
        assert (tiled.view(np.uint32)[:, width:] == SENTINEL).all(), "the padding columns were written"
        got = tiled[:, :width]
        assert np.isfinite(got).all()
        assert same_bits(got, want), "worst difference %g" % np.abs(got.astype(np.float64) - want).max()
        if width * height >= 64:
            assert 1 <= (~parts["valid"]).sum() <= 5 and (got[~parts["valid"]][:, 3] == -1).all()
            assert same_bits(got[~parts["valid"]][:, :3], images["fallback"][:, :width][~parts["valid"]][:, :3])
    # an invalid pixel is not counted by its neighbours: making one invalid changes them exactly as the restatement says (above); here, that it changes them at all
    if width >= 3 and height >= 2:
        y, x = height // 2, width // 2
        moments = images["moments"].copy(); moments[y, x, 3] = 0.0
        tiers_in = images["tiers"].copy(); tiers_in[-1, y, x, :3] = 4.0 * cases.boundaries(tiers)[-1]; tiers_in[-1, y, x, 3] = 1.0   # a bright sample the neighbours could lean on
        with_it = grt.resolve_fireflies_images(ctx, images["mean"], images["moments"], tiers_in, images["fallback"], width=width, support=1.5)
        without = grt.resolve_fireflies_images(ctx, images["mean"], moments, tiers_in, images["fallback"], width=width, support=1.5)
        assert same_bits(without[:, :width], ref.resolve(images["mean"], moments, tiers_in, images["fallback"], width=width, support=1.5))
        assert same_bits(with_it[:, :width], ref.resolve(images["mean"], images["moments"], tiers_in, images["fallback"], width=width, support=1.5))
        assert without[y, x, 3] == -1


def test_probe_refusals(grt, ctx, contexts):
    images = cases.resolve_case(64, 8, 96, 6)
    for given, text in (({"tier_count": 1}, "tiers"), ({"tier_count": 9}, "tiers"), ({"start": 0.0}, "start"), ({"start": float("inf")}, "start"), ({"support": 1.0}, "support"),
                        ({"support": float("nan")}, "support")):
        with pytest.raises(grt.DeviceRefusal, match=text) as refusal:
            grt.resolve_fireflies_images(ctx, **images, **given)
        assert refusal.value.status == RT_ERROR_INVALID_ARG
    with pytest.raises(grt.DeviceRefusal, match="pitch at least width"):
        grt.resolve_fireflies_images(ctx, **images, width=97)
    frame_ctx, pitch = contexts[(3, 2)]
    blank = np.zeros((1, 2, pitch, 4), np.float32)
    state = np.zeros((6, 2, pitch, 4), np.float32)
    for pixels, text in (([6], "outside"), ([1, 1], "second time")):
        with pytest.raises(grt.DeviceRefusal, match=text):
            grt.accumulate_cascade_frames(frame_ctx, blank, blank[0], blank[0], state, first_sample=[3], sample_count=[1], merged=True, pixels=np.array(pixels, np.uint32))
    with pytest.raises(grt.DeviceRefusal, match="merged form"):
        grt.accumulate_cascade_frames(frame_ctx, blank, blank[0], blank[0], state, first_sample=3, pixels=np.array([0], np.uint32))
    with pytest.raises(grt.DeviceRefusal, match="start"):
        grt.accumulate_cascade_frames(frame_ctx, blank, blank[0], blank[0], state, first_sample=3, start=-1.0)


# ---- on a context: cornellbox, 128 x 128, 3 bounces -------------------------------------------------------------------------------------------------

W, H, SAMPLES = 128, 128, 12


def _render(grt, pt, samples, mode="merged"):
    """Samples 0 .. samples - 1 from a fresh progression."""
    grt.set_scheduler(pt.ctx, "slots" if mode == "slots" else "merged")
    pt.invalidate("gpu_config")
    pt.update()
    assert pt.sample_index == 0
    pt.render()
    while pt.sample_index + 1 < samples:
        pt.update()
        pt.render()


def _state(grt, pt):
    """Everything rt_resolve_fireflies must leave alone: accumulator, moments, tiers, final image."""
    return [pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, pt.height, pt.pitch), grt.read_firefly_cascade(pt.ctx, pt.height, pt.pitch), pt.read_framebuffer().copy()]


def _resolve_own_images(grt, pt, **given):
    mean, moments, tiers, final = _state(grt, pt)
    return grt.resolve_fireflies_images(pt.ctx, mean, moments, tiers, final, width=pt.width, sentinel=0, **given)


@pytest.fixture(scope="module")
def cornell(grt):
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, firefly_filter=1)
    yield scene, pt
    grt.set_scheduler(pt.ctx, "merged")
    pt.close(); scene.close(); grt.config_reset()


def test_config_switches_on_the_estimate_and_the_cascade(grt, cornell):
    scene, pt = cornell
    assert grt.get_noise_estimate(pt.ctx)
    assert grt.get_firefly_cascade(pt.ctx) == {"tiers": 6, "start": 1.0, "support": 4.0}


@pytest.mark.parametrize("mode", ["merged", "slots"])
def test_resolve_is_the_probe_on_the_contexts_images_and_leaves_the_frame_alone(grt, cornell, mode):
    """(a) the resolved image equals rt_resolve_fireflies_images fed the context's own read-back images, bit for bit; (b) accumulator, moments, tiers and final image are
    the same bits before and after, and a render continued after the call equals the same render without it; (c) the tiers hold the frame: they sum to w times the mean."""
    scene, pt = cornell
    try:
        _render(grt, pt, SAMPLES, mode)
        before = _state(grt, pt)
        grt.resolve_fireflies(pt.ctx)
        got = grt.read_resolved(pt.ctx, H, pt.pitch)
        for a, b in zip(before, _state(grt, pt)):
            assert a.tobytes() == b.tobytes()
        assert got[:, :W].tobytes() == _resolve_own_images(grt, pt)[:, :W].tobytes()
        image, held = pt.resolve_fireflies()
        assert image.tobytes() == got[:, :W, :3].tobytes() and held.tobytes() == got[:, :W, 3].tobytes()
        assert np.isfinite(image).all() and (held >= -1e-3).all()
        mean, moments, tiers, _ = before
        assert (moments[:, :W, 3] == SAMPLES - 1).all() and np.allclose(tiers[:, :, :W, 3].sum(axis=0), SAMPLES - 1, atol=1e-4)
        total = tiers[:, :, :W, :3].sum(axis=0, dtype=np.float64) / (SAMPLES - 1)
        assert np.allclose(total, mean[:, :W, :3], rtol=1e-4, atol=1e-5)
        kept = got[:, :W, :3].astype(np.float64) @ np.array(ref.LUMA) + got[:, :W, 3]
        assert np.allclose(kept, total @ np.array(ref.LUMA), rtol=1e-4, atol=1e-5)   # kept + held back = the mean
        for _ in range(3):
            pt.update(); pt.render()
        continued = _state(grt, pt)
        _render(grt, pt, SAMPLES + 3, mode)
        for a, b in zip(continued, _state(grt, pt)):
            assert a.tobytes() == b.tobytes()
    finally:
        grt.set_scheduler(pt.ctx, "merged")


def test_the_frame_is_the_same_with_the_cascade_on_and_off(grt, cornell):
    scene, pt = cornell
    _render(grt, pt, 6)
    on = [pt.read_framebuffer().copy(), pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, H, pt.pitch)]
    try:
        grt.config_set(firefly_filter=0, noise_target=1e-30)   # (the estimate stays on)
        _render(grt, pt, 6)
        assert grt.get_firefly_cascade(pt.ctx) is None
        with pytest.raises(grt.DeviceRefusal, match="cascade is off"):
            grt.read_firefly_cascade(pt.ctx, H, pt.pitch)
        off = [pt.read_framebuffer().copy(), pt.read_aov(grt.AOV_RADIANCE).copy(), grt.read_noise_moments(pt.ctx, H, pt.pitch)]
        for a, b in zip(on, off):
            assert a.tobytes() == b.tobytes()
    finally:
        grt.config_set(firefly_filter=1, noise_target=0.0)
        _render(grt, pt, 2)
    assert grt.get_firefly_cascade(pt.ctx) is not None


def test_after_an_adaptive_render(grt, cornell):
    scene, pt = cornell
    _render(grt, pt, SAMPLES)
    estimate = pt.noise_estimate()
    means = estimate["cell_sums"] / np.maximum(estimate["cell_counts"], 1)
    chosen = pt.select_adaptive(float(np.quantile(means, 0.9)))
    try:
        assert 0 < chosen["active_cells"] < chosen["cells"]
        for _ in range(2):
            pt.update(); pt.render_samples(4)
    finally:
        pt.adaptive_off()
    mean, moments, tiers, _ = _state(grt, pt)
    w = moments[:, :W, 3]
    assert w.min() < w.max() and np.allclose(tiers[:, :, :W, 3].sum(axis=0), w, atol=1e-3)   # the list form splats too: W follows w pixel by pixel
    grt.resolve_fireflies(pt.ctx, support=3.0)
    got = grt.read_resolved(pt.ctx, H, pt.pitch)
    assert got[:, :W].tobytes() == _resolve_own_images(grt, pt, support=3.0)[:, :W].tobytes() and np.isfinite(got[:, :W]).all()


@pytest.mark.parametrize("mode", ["merged", "slots", "list"])
def test_all_four_means_are_the_same_with_the_cascade_on_and_off(grt, cornell, mode):
    """The probes take every AOV but RADIANCE away, so this is what holds the cascade kernels' folds of ALBEDO, NORMAL and POSITION: 6 samples with the three
    enabled (list: then two adaptive passes of 4 over the cells above the 0.9 quantile, as test_after_an_adaptive_render), rendered with the cascade on and off.
    The four accumulators, the moments and the final image are the same bytes."""
    scene, pt = cornell
    guides = (grt.AOV_ALBEDO, grt.AOV_NORMAL, grt.AOV_POSITION)

    def frame():
        _render(grt, pt, 6, mode)
        if mode == "list":
            estimate = pt.noise_estimate()
            means = estimate["cell_sums"] / np.maximum(estimate["cell_counts"], 1)
            chosen = pt.select_adaptive(float(np.quantile(means, 0.9)))
            try:
                assert 0 < chosen["active_cells"] < chosen["cells"]
                for _ in range(2):
                    pt.update(); pt.render_samples(4)
            finally:
                pt.adaptive_off()
        return [pt.read_framebuffer().copy(), grt.read_noise_moments(pt.ctx, H, pt.pitch)] + [pt.read_aov(aov).copy() for aov in (grt.AOV_RADIANCE,) + guides]

    try:
        for aov in guides:
            pt.aov_enable(aov)
        on = frame()
        assert grt.get_firefly_cascade(pt.ctx) is not None and grt.read_firefly_cascade(pt.ctx, H, pt.pitch).any()
        grt.config_set(firefly_filter=0, noise_target=1e-30)   # (the estimate stays on)
        off = frame()
        assert grt.get_firefly_cascade(pt.ctx) is None
        assert all(image[:, :W, :3].any() for image in on[2:]), "an AOV was not folded"
        if mode == "list":
            assert on[1][:, :W, 3].min() < on[1][:, :W, 3].max()   # some pixels took the adaptive passes, some did not
        for a, b, what in zip(on, off, ("final image", "moments", "radiance mean", "albedo mean", "normal mean", "position mean")):
            assert a.tobytes() == b.tobytes(), what
    finally:
        grt.config_set(firefly_filter=1, noise_target=0.0)
        for aov in guides:
            pt.aov_enable(aov, False)
        grt.set_scheduler(pt.ctx, "merged")
        _render(grt, pt, 2)
    assert grt.get_firefly_cascade(pt.ctx) is not None


def test_refusals_zeroing_and_resize(grt, cornell):
    scene, pt = cornell
    lib = grt.device_lib()
    _render(grt, pt, 6)
    state = grt.get_firefly_cascade(pt.ctx)

    def refused(call, status, text):
        with pytest.raises(grt.DeviceRefusal, match=text) as refusal:
            call()
        assert refusal.value.status == status
    for given, text in (({"tiers": 1}, "tiers"), ({"tiers": 9}, "tiers"), ({"start": 0.0}, "start"), ({"start": float("nan")}, "start"), ({"support": 1.0}, "support"), ({"support": float("inf")}, "support")):
        refused(lambda: grt.set_firefly_cascade(pt.ctx, **given), RT_ERROR_INVALID_ARG, text)
        assert grt.get_firefly_cascade(pt.ctx) == state   # a refused call leaves the previous state in force
    refused(lambda: grt.resolve_fireflies(pt.ctx, support=1.0), RT_ERROR_INVALID_ARG, "support")
    assert lib.rt_read_firefly_cascade(pt.ctx, None, 0) == RT_ERROR_INVALID_ARG and lib.rt_read_resolved(pt.ctx, None) == RT_ERROR_INVALID_ARG
    assert lib.rt_set_denoise_source(pt.ctx, 2) == RT_ERROR_INVALID_ARG
    small = np.zeros(16, np.float32)
    assert lib.rt_read_firefly_cascade(pt.ctx, small.ctypes.data, small.size) == RT_ERROR_INVALID_ARG and b"capacity" in lib.rt_last_error(pt.ctx)
    config = pt.device_config()
    svgf = type(config).from_buffer_copy(config); svgf.enable_svgf = 1
    assert lib.rt_set_config(pt.ctx, byref(svgf)) == 0
    refused(lambda: grt.resolve_fireflies(pt.ctx), RT_ERROR_NOT_READY, "SVGF")
    assert lib.rt_set_config(pt.ctx, byref(config)) == 0
    # rt_set_noise_estimate zeroes the tiers with the moments; off, it takes the cascade with it
    assert grt.read_firefly_cascade(pt.ctx, H, pt.pitch).any()
    grt.set_noise_estimate(pt.ctx, True)
    assert not grt.read_firefly_cascade(pt.ctx, H, pt.pitch).any() and not grt.read_noise_moments(pt.ctx, H, pt.pitch).any()
    refused(lambda: grt.resolve_fireflies(pt.ctx), RT_ERROR_NOT_READY, "no pixel is valid")
    refused(lambda: grt.read_resolved(pt.ctx, H, pt.pitch), RT_ERROR_NOT_READY, "no resolved image")
    grt.set_noise_estimate(pt.ctx, False)
    assert grt.get_firefly_cascade(pt.ctx) is None
    refused(lambda: grt.resolve_fireflies(pt.ctx), RT_ERROR_NOT_READY, "cascade is off")
    refused(lambda: grt.set_firefly_cascade(pt.ctx), RT_ERROR_NOT_READY, "noise estimate")
    grt.set_noise_estimate(pt.ctx, True)
    grt.set_firefly_cascade(pt.ctx, tiers=3, start=0.5)
    assert grt.read_firefly_cascade(pt.ctx, H, pt.pitch).shape[0] == 3
    grt.set_firefly_cascade(pt.ctx, enable=False)
    assert grt.get_firefly_cascade(pt.ctx) is None
    # the host puts its configuration back at the next update(); rt_resize gives the tiers the new size, zeroed
    _render(grt, pt, 4)
    assert grt.get_firefly_cascade(pt.ctx) == state
    grt.resolve_fireflies(pt.ctx)
    try:
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, 96, 80) == 0
        pt.width, pt.height = 96, 80
        refused(lambda: grt.read_resolved(pt.ctx, 80, pt.pitch), RT_ERROR_NOT_READY, "no resolved image")
        tiers = grt.read_firefly_cascade(pt.ctx, 80, pt.pitch)
        assert tiers.shape == (6, 80, pt.pitch, 4) and not tiers.any()
        _render(grt, pt, 4)
        grt.resolve_fireflies(pt.ctx)
        got = grt.read_resolved(pt.ctx, 80, pt.pitch)
        assert got[:, :96].tobytes() == _resolve_own_images(grt, pt)[:, :96].tobytes()
    finally:
        assert grt.host_lib().grt_pathtracer_resize(pt.handle, W, H) == 0
        pt.width, pt.height = W, H


def test_denoise_from_the_resolved_image(grt, tmp_path):
    """rt_denoise with RT_DENOISE_SOURCE_RESOLVED equals rt_denoise_images fed the resolved image as its colour; it refuses without a resolve and after a fold."""
    scene, pt = make_pathtracer(grt, "cornellbox", W, H, 0, num_bounces=3, firefly_filter=1, denoise=1)
    try:
        _render(grt, pt, 8)
        grt.set_denoise_source(pt.ctx, "resolved")
        with pytest.raises(grt.DeviceRefusal, match="none exists") as refusal:
            grt.denoise(pt.ctx)
        assert refusal.value.status == RT_ERROR_NOT_READY
        grt.resolve_fireflies(pt.ctx)
        resolved = grt.read_resolved(pt.ctx, H, pt.pitch)
        grt.denoise(pt.ctx)
        got = grt.read_denoised(pt.ctx, H, pt.pitch)
        guides = [pt.read_aov(getattr(grt, name)).copy() for name in ("AOV_ALBEDO", "AOV_NORMAL", "AOV_POSITION")]
        eye = np.array(list(pt.camera().position), np.float32)
        want = grt.denoise_images(pt.ctx, resolved, grt.read_noise_moments(pt.ctx, H, pt.pitch), *guides, pt.read_framebuffer(), eye, width=W, sentinel=0)
        assert got[:, :W].tobytes() == want[:, :W].tobytes()
        grt.set_denoise_source(pt.ctx, "mean")
        grt.denoise(pt.ctx)
        assert grt.read_denoised(pt.ctx, H, pt.pitch)[:, :W].tobytes() != got[:, :W].tobytes()
        grt.set_denoise_source(pt.ctx, "resolved")
        pt.update(); pt.render()
        with pytest.raises(grt.DeviceRefusal, match="older than the frame"):
            grt.denoise(pt.ctx)
        image, _ = pt.resolve_fireflies()
        for name in ("r.exr", "r.ppm"):
            pt.save_resolved_image(tmp_path / name)
            grt.export_image(tmp_path / ("want_" + name), image)
            assert (tmp_path / name).read_bytes() == (tmp_path / ("want_" + name)).read_bytes()
    finally:
        pt.close(); scene.close(); grt.config_reset()


def test_the_ao_integrator_keeps_the_cascade_off(grt):
    """Its accumulate keeps no moments and never splats: config firefly_filter = 1 allocates nothing for it, and switches no estimate on."""
    grt.config_reset()
    scene = grt.Scene(grt.scene_path("cornellbox"))
    grt.config_set(firefly_filter=1)
    ao = grt.AO(scene, 64, 64, device=0)
    try:
        ao.update(); ao.render()
        assert grt.get_firefly_cascade(ao.ctx) is None and not grt.get_noise_estimate(ao.ctx)
        with pytest.raises(grt.DeviceRefusal, match="cascade is off") as refusal:
            grt.resolve_fireflies(ao.ctx)
        assert refusal.value.status == RT_ERROR_NOT_READY
        ao.update(); ao.render()
        assert np.isfinite(ao.read_framebuffer()[:, :64, :3]).all() and grt.get_firefly_cascade(ao.ctx) is None
    finally:
        ao.close(); scene.close(); grt.config_reset()


ERROR_SIZE, ERROR_SAMPLES, ERROR_START = 128, 16, 0.0625


def test_the_resolved_image_is_closer_to_a_long_render_than_the_mean(grt, tmp_path):
    """The glass / medium scene of scenes.py (a rough dielectric holding a medium under two small emitters: caustic paths no light sample reaches), 128 x 128, 16
    samples against the plain render of 64 x as many. The scene is dim -- its mean luminance is ~0.2 --, so the lowest tier stands for 1 / 16 (tools/fireflies_sweep.py
    has the rows for every start). The case was picked where the float64 reference, applied to the device's read-back tiers, shows the ordering too: asserted first, so
    that the second assertion tests the kernels and not luck."""
    from scenes import write_scene_with_everything
    from test_loaders import _png_bytes
    grt.config_reset()
    scene = grt.Scene(write_scene_with_everything(tmp_path, _png_bytes)); scene.set_sky_scale(0.3)
    grt.config_set(num_bounces=6, firefly_filter=1, firefly_start=ERROR_START)
    pt = grt.Pathtracer(scene, ERROR_SIZE, ERROR_SIZE, device=0)
    try:
        def render(samples):
            pt.invalidate("gpu_config")
            pt.update(); pt.render()
            while pt.sample_index + 1 < samples:
                pt.update(); pt.render_samples(min(8, samples - pt.sample_index))
            return pt.read_framebuffer()[:, :ERROR_SIZE, :3].astype(np.float64)
        truth = render(64 * ERROR_SAMPLES)
        mean = render(ERROR_SAMPLES)
        resolved, held = pt.resolve_fireflies()
        state = grt.get_firefly_cascade(pt.ctx)
        reference = ref.resolve(pt.read_aov(grt.AOV_RADIANCE), grt.read_noise_moments(pt.ctx, ERROR_SIZE, pt.pitch), grt.read_firefly_cascade(pt.ctx, ERROR_SIZE, pt.pitch),
                                pt.read_framebuffer(), width=ERROR_SIZE, start=state["start"], support=state["support"], dtype=np.float64)
        errors = [cases.relative_rms(image, truth) for image in (mean, reference[..., :3], resolved)]
        print("glass / medium scene %d x %d, %d samples against %d: relative RMS error mean %.5f, float64 reference on the device's tiers %.5f, resolved %.5f (%.3f x); held back %.3f %% of the luminance"
              % (ERROR_SIZE, ERROR_SIZE, ERROR_SAMPLES, 64 * ERROR_SAMPLES, *errors, errors[0] / errors[2], 100 * np.maximum(held, 0).sum() / (mean @ np.array(ref.LUMA)).sum()))
        assert state["start"] == ERROR_START
        assert errors[1] < errors[0]
        assert errors[2] < errors[0]
    finally:
        pt.close(); scene.close(); grt.config_reset()


def test_command_line(grt, tmp_path):
    """pathtracer --firefly-filter: -o receives the resolved image, --firefly-unfiltered the plain one, --firefly-map the held-back plane; with --denoise the
    denoiser runs on the resolved image; it composes with --noise-target --adaptive; with the AO integrator it warns once and writes the plain image."""
    from test_loaders import CLI, _parse_exr
    scene_file = grt.scene_path("cornellbox")
    def run(*options):
        r = subprocess.run([CLI, "-s", scene_file] + [str(o) for o in options], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        return r
    r = run("-N", 8, "--firefly-filter", "--firefly-tiers", 5, "--firefly-support", 3, "-o", tmp_path / "out.exr", "--firefly-unfiltered", tmp_path / "plain.exr", "--firefly-map", tmp_path / "map.exr")
    assert "Firefly filter: 5 tiers from 1, support 3" in r.stdout and all("Wrote %s" % (tmp_path / n) in r.stdout for n in ("out.exr", "plain.exr", "map.exr"))
    _, out = _parse_exr(tmp_path / "out.exr")
    _, plain = _parse_exr(tmp_path / "plain.exr")
    from test_gpu_noise import _read_luminance_exr
    held = _read_luminance_exr(tmp_path / "map.exr")   # (one channel of 32-bit floats, rows as in the images)
    assert out["R"].shape == plain["R"].shape == held.shape
    luma = lambda image: 0.299 * image["R"].astype(np.float64) + 0.587 * image["G"] + 0.114 * image["B"]
    assert (held >= -1e-3).all()
    assert np.allclose(luma(out) + held, luma(plain), rtol=5e-3, atol=5e-3)   # kept + held back = the mean (half-precision files)
    r = run("-N", 8, "--firefly-filter", "--denoise", "-o", tmp_path / "both.exr")
    assert "Firefly filter: 6 tiers" in r.stdout and "Denoised: 5 iterations" in r.stdout
    r = run("-N", 40, "--noise-target", 0.05, "--noise-min-samples", 8, "--adaptive", "--firefly-filter", "-o", tmp_path / "adaptive.exr")
    assert "Adaptive:" in r.stdout and "Firefly filter:" in r.stdout
    r = run("-I", "ao", "-N", 3, "--firefly-filter", "-o", tmp_path / "ao.exr")
    assert r.stderr.count("WARNING: --firefly-filter") == 1 and "Firefly filter:" not in r.stdout and "Rendered sample 3" in r.stdout
