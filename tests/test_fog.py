"""The fog volume without a GPU: the float64 restatement of fog_reference.py against itself -- the white furnace integrates
to 1, the single-scatter Monte Carlo agrees with the quadrature of the integral, the phase function is a density and its sampler draws from
it, the hashed pair's key is one no other draw forms -- and the new entry points' refusal of a NULL context."""
import ctypes
import math
from ctypes import c_int, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

import fog_cases as cases
import fog_reference as ref

RT_ERROR_INVALID_ARG = -1
CAMERA = np.array([0.0, 0.5, -3.0])


def _fan(n, rng, spread=0.17):
    """n rays from the frame tests' camera, within their 20 degree view."""
    d = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), np.ones(n)], axis=1)
    return np.tile(CAMERA, (n, 1)), d / np.linalg.norm(d, axis=1)[:, None]


def test_the_key_is_one_no_other_draw_forms():
    """random_sample's keys (pixel * 7 + dimension) * 128 + bounce stay below 2^31 while the frame has at most 2 396 745 pixels; the fog's has bit 31 set."""
    limit = (1 << 31) // (7 * 128)
    assert limit == 2396745
    assert max(ref.existing_keys(limit - 1, 127)) < 1 << 31 <= max(ref.existing_keys(limit, 127))
    rng = np.random.default_rng(3)
    for pixel in [0, 1, 4095, limit - 1] + [int(v) for v in rng.integers(0, limit, 200)]:
        for bounce in (0, 1, 127):
            key = ref.random_key(pixel, bounce)
            assert key >= 1 << 31 and key not in ref.existing_keys(pixel, bounce)
            assert key == 0x80000000 + pixel * 128 + bounce   # distinct paths: distinct keys
    x, y = ref.random_pair(17, 1, 3)
    assert x.dtype == np.float32 and 0.0 <= x < 1.0 and 0.0 <= y < 1.0
    assert ref.random_pair_integers(17, 1, 3) != ref.random_pair_integers(17, 1, 4)
    # the largest integer still gives a number below 1
    assert np.float32(np.uint32(0xFFFFFFFF)) * ref.ONE_OVER_MAX_UNSIGNED < 1.0


def test_the_pair_is_uniform_and_uncorrelated():
    pairs = np.array([ref.random_pair(p, b, s) for p in range(40) for b in range(4) for s in range(25)], np.float64)
    n = pairs.shape[0]
    assert abs(pairs[:, 0].mean() - 0.5) < 5 * math.sqrt(1 / 12 / n) and abs(pairs[:, 1].mean() - 0.5) < 5 * math.sqrt(1 / 12 / n)
    assert abs(np.corrcoef(pairs[:, 0], pairs[:, 1])[0, 1]) < 5 / math.sqrt(n)


@pytest.mark.parametrize("g", [0.0, 0.3, 0.8, -0.8, 0.95])
def test_the_phase_function_is_a_density_and_the_sampler_draws_from_it(g):
    x, w = np.polynomial.legendre.leggauss(400)
    assert abs(2 * math.pi * (w * ref.hg(x, g)).sum() - 1.0) < 1e-9
    mean_cos = 2 * math.pi * (w * x * ref.hg(x, g)).sum()
    assert abs(mean_cos + g) < 1e-9    # against omega, the way BACK: forward scattering is cos = -1
    rng = np.random.default_rng(5)
    n = 200000
    omega = ref.uniform_sphere(rng.random(n), rng.random(n))
    direction, c = ref.hg_sample(omega, g, rng.random(n), rng.random(n))
    assert np.allclose(np.linalg.norm(direction, axis=1), 1.0, atol=1e-12) and np.allclose(np.einsum("ij,ij->i", direction, omega), c, atol=1e-12)
    assert abs(c.mean() + g) < 5 * c.std() / math.sqrt(n)
    # E[1 / pdf] over the sampler's draws is the measure of the sphere
    assert abs((1.0 / ref.hg(c, g)).mean() - 4 * math.pi) < 5 * (1.0 / ref.hg(c, g)).std() / math.sqrt(n) + 1e-9   # (g = 0: every draw is 4 pi)


def test_the_clip_rules():
    for name, (o, d, t_end) in cases.SEGMENTS.items():
        c = ref.clip(cases.BOX_MIN, cases.BOX_MAX, np.float32(o), np.float32(d), np.float32(t_end))
        empty = any(k in name for k in ("leaving", "miss", "parallel_outside", "graze", "before_entry", "at_entry"))
        assert (c is None) == empty, name
        if c is not None:
            assert math.isfinite(c[0]) and math.isfinite(c[1]) and 0.0 <= c[0] < c[1] <= float(np.float32(t_end)), name
            ok, t0, t1 = ref.clip_many(cases.BOX_MIN.astype(np.float64), cases.BOX_MAX.astype(np.float64), np.float64([np.float32(o)]), np.float64([np.float32(d)]), float(np.float32(t_end)))
            assert ok[0] and t0[0] == c[0] and t1[0] == c[1], name
    assert ref.clip(cases.BOX_MIN, cases.BOX_MAX, (0, 0.5, 2), (0, 0, 1), math.inf)[0] == 0.0   # an origin on a face is inside
    assert np.array_equal(ref.shadow_factor(cases.BOX_MIN, cases.BOX_MAX, (1, 2, 3), (3, 0.5, 0), (0, 0, 1), math.inf), np.ones(3))


def test_the_distance_sample_is_unbiased():
    """E[weight x f] over the pair, for f = 1 on scatter events and for f = 1 on the others, against sigma_s / sigma_t (1 - T) and T per channel."""
    sigma_a, sigma_s, _ = cases.VOLUMES["unequal"]
    sa, ss = np.float32(sigma_a), np.float32(sigma_s)
    st = sa.astype(np.float64) + ss.astype(np.float64)
    L = 1.3
    throughput = np.float32([0.2, 0.9, 0.4])
    rng = np.random.default_rng(11)
    n = 40000
    scattered = np.zeros((n, 3)); passed = np.zeros((n, 3))
    for i in range(n):
        did, _, w = ref.sample_distance(sa, ss, (np.float32(rng.random()), np.float32(rng.random())), L, throughput)
        (scattered if did else passed)[i] = w
    T = np.exp(-st * L)
    for got, want in ((scattered, throughput * ss / st * (1 - T)), (passed, throughput * T)):
        error = got.std(axis=0) / math.sqrt(n)
        assert np.all(np.abs(got.mean(axis=0) - want) < 5 * error), (got.mean(axis=0), want, error)


@pytest.mark.parametrize("g", [0.0, 0.8, -0.8])
def test_the_white_furnace_integrates_to_one(g):
    from fog_cases import FURNACE_BOUNCES, FURNACE_SIGMA
    assert ref.furnace_truncation_bound(cases.BOX_MIN, cases.BOX_MAX, FURNACE_SIGMA, FURNACE_BOUNCES) < 1e-6
    assert ref.furnace_truncation_bound(cases.BOX_MIN, cases.BOX_MAX, FURNACE_SIGMA, FURNACE_BOUNCES - 1) > 1e-6   # the smallest limit that does
    rng = np.random.default_rng(13)
    o, d = _fan(60000, rng)
    plain = ref.furnace(cases.BOX_MIN, cases.BOX_MAX, FURNACE_SIGMA, g, FURNACE_BOUNCES, o, d, rng)
    assert np.all((plain == 1.0) | (plain == 0.0)) and plain.mean() >= 1.0 - 1e-4   # exactly 1 unless truncated
    for mis in (True, False):
        v = ref.furnace(cases.BOX_MIN, cases.BOX_MAX, FURNACE_SIGMA, g, FURNACE_BOUNCES, o, d, rng, nee=True, sky_share=0.5, mis=mis)
        error = v.std() / math.sqrt(v.size)
        print("g = %g, NEE%s: mean %.5f, standard error %.5f" % (g, " + MIS" if mis else "", v.mean(), error))
        assert abs(v.mean() - 1.0) < 5 * error


def test_the_single_scatter_monte_carlo_agrees_with_the_quadrature():
    """The rule of the GPU test, on the CPU, no pixel left out: 16 x 16 pixels, 4 096 samples each, within 5 standard errors of the quadrature."""
    from fog_cases import SHAFT
    a = dict(box_min=cases.BOX_MIN, box_max=cases.BOX_MAX, sigma_a=SHAFT["sigma_a"], sigma_s=SHAFT["sigma_s"], g=SHAFT["g"], light=cases.SHAFT_LIGHT, intensity=cases.SHAFT_INTENSITY)
    # the frame tests' camera: 20 degrees over 16 pixels, looking down +z
    half = math.tan(math.radians(10.0))
    camera = dict(position=CAMERA, bottom_left_corner=np.array([-half, -half, 1.0]), x_axis=np.array([2 * half / 16, 0, 0]), y_axis=np.array([0, 2 * half / 16, 0]))
    w = h = 16
    grid = [0.25, 0.75]
    want = np.zeros(w * h)
    for jx in grid:
        for jy in grid:
            dirs = ref.pixel_rays(camera, w, h, (jx, jy))
            want += np.array([ref.shaft_quadrature(o=CAMERA, d=dirs[k], **a) for k in range(w * h)]) / 4.0
    # the light is at least a box width off every ray: the integrand is bounded
    light = np.array(cases.SHAFT_LIGHT)
    for corner in ((0, 0), (16, 0), (0, 16), (16, 16)):
        d = ref.pixel_rays(camera, 1, 1, corner)[0]
        assert np.linalg.norm(np.cross(light - CAMERA, d)) >= float(cases.BOX_MAX[0] - cases.BOX_MIN[0])
    rng = np.random.default_rng(17)
    n = SHAFT["samples"]
    total = np.zeros(w * h); squares = np.zeros(w * h)
    for _ in range(n // 256):
        dirs = ref.pixel_rays(camera, w, h, rng.random((256 * w * h, 2)), repeat=256)
        v = ref.shaft_monte_carlo(o=np.broadcast_to(CAMERA, dirs.shape), d=dirs, rng=rng, **a).reshape(256, w * h)
        total += v.sum(axis=0); squares += (v * v).sum(axis=0)
    mean = total / n
    error = np.sqrt((squares / n - mean * mean) / (n - 1))
    deviation = np.abs(mean - want) / error
    print("shaft on the CPU: radiance %.4g .. %.4g, worst deviation %.2f standard errors" % (want.min(), want.max(), deviation.max()))
    assert want.min() > 0 and (deviation > 5.0).sum() == 0


def test_config_keys_accept_and_refuse(grt):
    grt.config_reset()
    try:
        grt.config_set(fog="-1,-0.5,2,1,1.5,4", fog_sigma_a=(0.1, 0.2, 0.3), fog_sigma_s=0.5, fog_g=0.3, fog_volumes=1)
        assert grt.config_get("fog") == 1.0 and abs(grt.config_get("fog_g") - 0.3) < 1e-7 and grt.config_get("fog_volumes") == 1.0
        grt.config_set(fog=(-1, -0.5, 2, 1, 1.5, 4), fog_sigma_a="0.25", fog_sigma_s="1, 2, 3", fog_volumes=0)
        for bad in (dict(fog="1,2,3"), dict(fog="0,0,0,0,1,1"), dict(fog="a,b,c,d,e,f"), dict(fog="1,2,3,4,5,6,7"), dict(fog=2), dict(fog_sigma_a="-1"), dict(fog_sigma_a=-0.5),
                    dict(fog_sigma_s=(1, 2)), dict(fog_sigma_s="1,,2"), dict(fog_g=1.0), dict(fog_g=-1.0), dict(fog_g=float("nan")), dict(fog_volumes=2)):
            with pytest.raises(KeyError):
                grt.config_set(**bad)
        assert grt.config_get("fog") == 1.0   # a refused value leaves the one before
        grt.config_set(fog="off")
        assert grt.config_get("fog") == 0.0
    finally:
        grt.config_reset()


def test_the_scene_takes_the_fog_from_the_config_and_round_trips(grt):
    grt.config_reset()
    try:
        plain = grt.Scene(grt.scene_path("cornellbox"))
        described = plain.describe()
        assert plain.fog is None
        grt.config_set(fog="-1,-0.5,2,1,1.5,4", fog_sigma_a=(0.125, 0.25, 0.5), fog_sigma_s=0.75, fog_g=-0.5)
        scene = grt.Scene(grt.scene_path("cornellbox"))
        assert scene.fog == dict(box_min=(-1.0, -0.5, 2.0), box_max=(1.0, 1.5, 4.0), sigma_a=(0.125, 0.25, 0.5), sigma_s=(0.75, 0.75, 0.75), g=-0.5)
        assert scene.describe() == described and scene.mesh_count == plain.mesh_count   # the fog stays out of the description
        scene.clear_fog()
        assert scene.fog is None
        scene.set_fog((0, 0, 0), (1, 2, 3), 0.5, (1, 2, 4), g=0.25)
        assert scene.fog == dict(box_min=(0.0, 0.0, 0.0), box_max=(1.0, 2.0, 3.0), sigma_a=(0.5, 0.5, 0.5), sigma_s=(1.0, 2.0, 4.0), g=0.25)
        for bad in (((0, 0, 0), (0, 1, 1), 0.1, 0.1, 0.0), ((0, 0, 0), (1, 1, 1), -0.1, 0.1, 0.0), ((0, 0, 0), (1, 1, 1), 0.1, float("inf"), 0.0), ((0, 0, 0), (1, 1, 1), 0.1, 0.1, 1.0)):
            with pytest.raises(RuntimeError):
                scene.set_fog(*bad)
        assert scene.fog["g"] == 0.25   # a refused volume leaves the one before
        scene.close(); plain.close()
    finally:
        grt.config_reset()


def test_the_loader_turns_a_null_shape_with_a_medium_into_the_fog(grt, tmp_path, capfd):
    grt.config_reset()
    try:
        bare = grt.Scene(cases.write_fog_shape_scene(tmp_path, "bare", ""))
        path = cases.write_fog_shape_scene(tmp_path, "cube", cases.FOG_CUBE)
        # fog_volumes = 0 (the default): the file loads as it always did -- the complaint about the null BSDF, the default material, the shape in the scene
        before = grt.Scene(path)
        assert "not supported" in capfd.readouterr().err
        assert before.fog is None and before.mesh_count == bare.mesh_count + 1
        described = before.describe()
        grt.config_set(fog_volumes=0)
        again = grt.Scene(path)
        assert again.describe() == described and again.mesh_count == before.mesh_count and again.fog is None
        # fog_volumes = 1: the box, and the shape is gone
        grt.config_set(fog_volumes=1)
        capfd.readouterr()
        scene = grt.Scene(path)
        assert "WARNING" not in capfd.readouterr().err   # the cube is its own bounding box
        assert scene.mesh_count == bare.mesh_count and scene.describe() == bare.describe()
        assert scene.fog == dict(box_min=(2.0, -2.0, -1.5), box_max=(4.0, 2.0, -0.5), sigma_a=(0.0625, 0.125, 0.25), sigma_s=(0.5, 1.0, 2.0), g=0.25)
        # a shape that does not fill its box: one warning, its bounding box
        ball = grt.Scene(cases.write_fog_shape_scene(tmp_path, "ball", cases.FOG_SPHERE))
        assert capfd.readouterr().err.count("does not fill") == 1
        assert ball.mesh_count == bare.mesh_count
        assert np.allclose(ball.fog["box_min"], (-2, -2, -2), atol=1e-5) and np.allclose(ball.fog["box_max"], (2, 2, 2), atol=1e-5)
        # a shape with a surface keeps its medium the old way
        glass = cases.FOG_CUBE.replace('<bsdf type="null"/>', '<bsdf type="dielectric"/>')
        kept = grt.Scene(cases.write_fog_shape_scene(tmp_path, "glass", glass))
        assert kept.fog is None and kept.mesh_count == bare.mesh_count + 1
        # the config key fog beside a file's volume: the key's volume replaces the file's, with a warning (and is no "second volume")
        grt.config_set(fog="0,0,0,1,1,1", fog_sigma_s=0.5)
        capfd.readouterr()
        both = grt.Scene(path)
        assert "replaces the fog volume of the scene file" in capfd.readouterr().err
        assert both.fog["box_max"] == (1.0, 1.0, 1.0) and both.fog["sigma_s"] == (0.5, 0.5, 0.5) and both.mesh_count == bare.mesh_count
        grt.config_set(fog="off")
        # a second volume is refused with its location
        with pytest.raises(RuntimeError) as refused:
            grt.Scene(cases.write_fog_shape_scene(tmp_path, "two", cases.FOG_CUBE + cases.FOG_SPHERE))
        assert "second fog volume" in str(refused.value) and "two.xml" in str(refused.value)
    finally:
        grt.config_reset()


def test_help_lists_the_fog_options(grt):
    import os
    import subprocess
    out = subprocess.run([os.path.join(os.path.dirname(grt.HOST_LIB_PATH), "pathtracer"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    for option in ("--fog ", "--fog-sigma-a", "--fog-sigma-s", "--fog-g", "--fog-volumes"):
        assert option in out, option


P, I, Z, U = c_void_p, c_int, c_size_t, c_uint32
NEW_ENTRY_POINTS = {
    "rt_set_fog_volume":        ([P], [None]),
    "rt_get_fog_volume":        ([P, P], [None, None]),
    "rt_fog_segments":          ([P, Z, P], [None, 0, None]),
    "rt_attenuate_shadow_rays": ([P, Z, P], [None, 0, None]),
    "rt_sort_rays_fog":         ([I, I, I, P, Z, P, Z, P, Z, Z, U] + [P] * 11, [0, 0, 0, None, 0, None, 0, None, 1, 1, 0] + [None] * 11),
}


@pytest.mark.parametrize("name", sorted(NEW_ENTRY_POINTS))
def test_a_null_context_is_refused_with_the_entry_points_own_message(grt, name):
    lib = ctypes.CDLL(grt.DEVICE_LIB_PATH)
    lib.rt_last_error.restype = ctypes.c_char_p; lib.rt_last_error.argtypes = [c_void_p]
    argtypes, values = NEW_ENTRY_POINTS[name]
    entry = getattr(lib, name)
    entry.restype = c_int; entry.argtypes = [c_void_p] + argtypes
    assert entry(None, *values) == RT_ERROR_INVALID_ARG
    assert lib.rt_last_error(None).decode() == "%s: NULL context" % name


def test_the_volume_record_is_64_bytes(grt):
    r = grt.fog_volume_record((0, 1, 2), (3, 4, 5), 0.5, (1, 2, 3), -0.25)
    assert r.nbytes == 64 and list(r) == [0, 1, 2, 3, 4, 5, 0.5, 0.5, 0.5, 1, 2, 3, -0.25, 0, 0, 0]
    with open(grt.REPO_ROOT + "/include/gpu_raytracer_amd.h") as f:
        header = f.read()
    assert "#define RT_ABI_VERSION 17" in header and "rt_fog_volume" in header
