"""Delta emitters on the device -- point, spot and directional lights in next-event estimation -- against the float64
restatement of delta_light_reference.py (the oracle does not know them), on the tables and scenes of delta_light_cases.py.

* tables (rt_upload_delta_lights / rt_read_delta_lights): P_k and the CDF against the float64 sums, the last entry exactly 1; the selection
  exact on every CDF entry, its float neighbours, 0 and 0x1.fffffep-1; a light of zero weight never selected; one refusal per rule, each
  leaving the table before it in force;
* the sample (rt_sample_delta_lights) over a grid of origins: direction, distance, radiance term, the spot falloff, the ok flag;
* the material launch entry by entry (rt_shade_rays) under a delta-only table and under a table split with triangle emitters and the sky;
* the sort launch entry by entry (rt_sort_rays) under q > 0: an emitter hit's MIS weight with the light pdf times 1 - taken, count_light forced
  at taken = 1, a sky miss added whole while s = 0 (null sky tables) and weighed by s alone while s > 0;
* identities, bit for bit: upload-then-clear, sky sampling with the table cleared, a spot that is all beam against the point light;
* a frame against the closed form (point, spot, directional), the share changing the noise and not the mean, the kernel variants.
Every test prints what it measured."""
import ctypes
import math
from ctypes import byref, c_float, c_int, c_void_p

import numpy as np
import pytest

import delta_light_cases as cases
import delta_light_reference as ref
from material_cases import DELTA_LIGHTS, DELTA_WEIGHTS   # the launch tests' delta lights, shared with test_gpu_material_instances.py
from delta_light_reference import POINT, SPOT, DIRECTIONAL, ONE_BELOW_ONE

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
EPS = 2.0 ** -24   # half a float32 ulp of 1: one rounding

# The spot falloff is (cutoff - acosf(c)) / (cutoff - beam) with c = dot(-to_light, axis). Its float32 error has three parts: c itself (the
# direction's error, see test_sample_matches_float64), which acos amplifies by 1 / sqrt(1 - c^2); acosf's own error and the rounding of the
# difference, both a few EPS of pi; the product's rounding. One unit is inv_transition x (direction error / sqrt(1 - c^2) + EPS pi) + EPS.
# (The unit is a bound, generous in each part; what the kernel does is far inside it.) Measured on the MI355X over the probes of
# test_sample_matches_float64 (four tables, 4913 origins each, 876 of them in a transition ring): worst 0.0636 units (table one_spot, light 0, and
# table sixty_five, light 37; table two 0.0493); held to 3 x that.
FALLOFF_MEASURED_UNITS = 0.0636
FALLOFF_BOUND_UNITS = 3.0 * FALLOFF_MEASURED_UNITS


def _lib(grt):
    lib = grt.device_lib()
    lib.rt_set_sky.argtypes = [c_void_p, c_void_p, c_int, c_int, c_float]
    lib.rt_render_samples.argtypes = [c_void_p, c_int, c_int]
    return lib


@pytest.fixture(scope="module")
def bare(grt):
    lib = _lib(grt)
    ctx = c_void_p()
    assert lib.rt_create(0, byref(ctx)) == 0, lib.rt_last_error(None)
    yield lib, ctx
    lib.rt_destroy(ctx)


def _upload(grt, lib, ctx, name, share=1.0):
    lights, weights = cases.TABLES[name]
    assert grt.upload_delta_lights(ctx, grt.delta_light_records(lights, weights), share) == 0, lib.rt_last_error(ctx)
    return ref.Table(lights, weights)


# ---- tables ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(cases.TABLES))
def test_tables_and_selection(grt, bare, name):
    lib, ctx = bare
    table = _upload(grt, lib, ctx, name, share=0.5)
    records, cdf, share = grt.read_delta_lights(ctx)
    assert records.shape == (table.n, 16) and cdf.shape == (table.n,) and share == 0.5
    assert np.array_equal(records.view(np.int32)[:, 3], table.type)
    assert cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all()
    # P_k and the CDF are one rounding of the float64 quotients (2e-7, the bound nee_checks.py holds the emitters' tables to)
    pdf_error = np.abs(records[:, 7] - table.pdf).max(); cdf_error = np.abs(cdf - table.cdf).max()
    print("%s: P_k within %.3g, CDF within %.3g of the float64 sums" % (name, pdf_error, cdf_error))
    assert pdf_error <= 2e-7 and cdf_error <= 2e-7
    assert np.abs(np.linalg.norm(records[:, 4:7].astype(np.float64), axis=1) - 1.0).max() <= 4 * EPS
    spot = table.type == SPOT
    assert np.array_equal(records[spot, 11], table.cos_cutoff[spot].astype(np.float32)) and np.array_equal(records[spot, 12], table.cos_beam[spot].astype(np.float32))
    assert np.abs(records[spot, 14] - table.inv_transition[spot]).max(initial=0) <= 4 * EPS * np.abs(table.inv_transition[spot]).max(initial=0)
    # selection: exact against searchsorted on the device's own CDF
    u = cases.edge_numbers(cdf)
    probes = np.zeros((u.size, 4), np.float32); probes[:, 0] = u; probes[:, 1:] = [0.25, -1.0, 0.5]
    got = grt.sample_delta_lights(ctx, probes)
    picked = got.view(np.int32)[:, 0]
    assert np.array_equal(picked, ref.select(cdf, u)), name
    assert np.array_equal(got[:, 8], records[picked, 7])   # the pdf is the record's, never a difference of CDF entries
    zero = np.nonzero(table.weight == 0)[0]
    assert not np.isin(picked, zero).any(), "%s: a light of zero weight was selected" % name
    inside = cases.inside_numbers(cdf)
    assert np.array_equal(np.isnan(inside), table.weight == 0)
    live = ~np.isnan(inside)
    probes = np.zeros((int(live.sum()), 4), np.float32); probes[:, 0] = inside[live]
    assert np.array_equal(grt.sample_delta_lights(ctx, probes).view(np.int32)[:, 0], np.nonzero(live)[0])


def _refusals(good):
    def changed(light, word, value, share=1.0, as_int=False):
        r = good.copy()
        if as_int:
            r.view(np.int32)[light, word] = value
        else:
            r[light, word] = value
        return r, share
    nan, inf = float("nan"), float("inf")
    return [
        ("unknown type", *changed(0, 0, 3, as_int=True)),
        ("position is not finite", *changed(0, 2, nan)),
        ("position is not finite", *changed(1, 1, inf)),
        ("direction is zero or not finite", (lambda r: (r.__setitem__((1, slice(4, 7)), 0.0), r)[1])(good.copy()), 1.0),
        ("direction is zero or not finite", *changed(2, 5, nan)),
        ("intensity 1 is", *changed(0, 8, -1.0)),
        ("intensity 2 is", *changed(2, 9, inf)),
        ("do not satisfy 0 < beam <= cutoff <= pi", *changed(1, 11, 0.0)),
        ("do not satisfy 0 < beam <= cutoff <= pi", *changed(1, 11, 1.5)),
        ("do not satisfy 0 < beam <= cutoff <= pi", *changed(1, 10, 3.2)),
        ("weight is", *changed(2, 12, -0.5)),
        ("weight is", *changed(0, 12, nan)),
        ("the total weight is", (lambda r: (r.__setitem__((slice(None), 12), 0.0), r)[1])(good.copy()), 1.0),
        ("share is", good.copy(), 0.0),
        ("share is", good.copy(), 1.5),
        ("share is", good.copy(), nan),
    ]


def test_upload_refuses_and_keeps_the_table_before(grt, bare):
    lib, ctx = bare
    _upload(grt, lib, ctx, "two", share=0.25)
    before = grt.read_delta_lights(ctx)
    probes = np.array([[0.1, 0, 0, 0], [0.9, 1, 0, 1]], np.float32)
    sampled = grt.sample_delta_lights(ctx, probes)
    lights = ref.lights_array([(POINT, (0, 3, 0), (0, 0, 1), (5, 5, 5), 0, 0), (SPOT, (1, 4, 0), (0, -1, 0), (9, 9, 9), 1.0, 0.5), (DIRECTIONAL, (0, 0, 0), (0, -1, 1), (1, 1, 1), 0, 0)])
    good = grt.delta_light_records(lights, [1.0, 2.0, 3.0])
    for words, records, share in _refusals(good):
        status = grt.upload_delta_lights(ctx, records, share)
        message = lib.rt_last_error(ctx).decode()
        assert status == RT_ERROR_INVALID_ARG and message.startswith("rt_upload_delta_lights") and words in message, (words, status, message)
        after = grt.read_delta_lights(ctx)
        assert np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32)) and np.array_equal(after[1], before[1]) and after[2] == before[2], words
    too_many = np.tile(good[:1], (grt.MAX_DELTA_LIGHTS + 1, 1))
    assert grt.upload_delta_lights(ctx, too_many, 1.0) == RT_ERROR_INVALID_ARG and "RT_MAX_DELTA_LIGHTS" in lib.rt_last_error(ctx).decode()
    assert np.array_equal(grt.sample_delta_lights(ctx, probes).view(np.uint32), sampled.view(np.uint32))
    # a directional light's position is not looked at; the good table uploads; clearing empties it and the probe says so
    ok = good.copy(); ok[2, 1] = float("nan")
    assert grt.upload_delta_lights(ctx, ok, 1.0) == 0, lib.rt_last_error(ctx)
    assert grt.read_delta_lights(ctx)[0].shape[0] == 3 and np.isfinite(grt.read_delta_lights(ctx)[0]).all()
    assert grt.upload_delta_lights(ctx, None) == 0
    assert grt.read_delta_lights(ctx)[0].shape[0] == 0 and grt.read_delta_lights(ctx)[2] == 0.0
    out = np.zeros((1, grt.DELTA_SAMPLE_OUT), np.float32)
    assert lib.rt_sample_delta_lights(ctx, probes.ctypes.data, 1, out.ctypes.data) == RT_ERROR_NOT_READY and b"no delta lights" in lib.rt_last_error(ctx)


def test_probe_contract(grt, bare):
    """What test_probe_contract.py and test_gpu_probe_contract.py hold for probes in general: a NULL context and NULL arrays are refused with the
    entry point's own message before any HIP work, the output untouched; the empty batch is RT_OK; numbers outside [0, 1) are named."""
    lib, ctx = bare
    _upload(grt, lib, ctx, "two")
    out = np.full((2, grt.DELTA_SAMPLE_OUT), 7.0, np.float32); probes = np.zeros((2, 4), np.float32)
    lib.rt_last_error.restype = ctypes.c_char_p
    assert lib.rt_sample_delta_lights(None, None, 0, None) == RT_ERROR_INVALID_ARG and lib.rt_last_error(None) == b"rt_sample_delta_lights: NULL argument"
    assert lib.rt_sample_delta_lights(ctx, None, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG
    assert lib.rt_sample_delta_lights(ctx, probes.ctypes.data, 1, None) == RT_ERROR_INVALID_ARG
    assert lib.rt_sample_delta_lights(ctx, probes.ctypes.data, (1 << 24) + 1, out.ctypes.data) == RT_ERROR_INVALID_ARG and b"2^24" in lib.rt_last_error(ctx)
    for column, value in ((0, 1.0), (0, -0.25), (0, np.nan), (2, np.inf)):
        bad = probes.copy(); bad[1, column] = value
        assert lib.rt_sample_delta_lights(ctx, bad.ctypes.data, 2, out.ctypes.data) == RT_ERROR_INVALID_ARG and b"probe 1" in lib.rt_last_error(ctx)
    assert lib.rt_sample_delta_lights(ctx, probes.ctypes.data, 0, out.ctypes.data) == 0
    assert (out == 7.0).all()
    assert lib.rt_upload_delta_lights(None, None, 0, 1.0) == RT_ERROR_INVALID_ARG and lib.rt_read_delta_lights(None, None, None, 0, None, None) == RT_ERROR_INVALID_ARG
    assert lib.rt_abi_version() == 17


# ---- the sample -----------------------------------------------------------------------------------------------------------

def _direction_error_bound(table, index, origin, distance):
    """to_light = (position - origin) / d in float32: each difference is one rounding of a number no larger than |origin| + |position|, the
    length three products, two sums and a root, the division one more. Against the exact direction that is, per component, at most
    4 EPS (1 + |origin| + |position|) / d from the differences and 4 EPS from the normalisation."""
    size = 1.0 + np.linalg.norm(origin.astype(np.float64), axis=1) + np.linalg.norm(table.position[index], axis=1)
    return 4 * EPS * size / distance + 4 * EPS, size


@pytest.mark.parametrize("name", list(cases.TABLES))
def test_sample_matches_float64(grt, bare, name):
    lib, ctx = bare
    table = _upload(grt, lib, ctx, name)
    records, cdf, _ = grt.read_delta_lights(ctx)
    origins = cases.origin_grid()
    inside = cases.inside_numbers(cdf)
    live = np.nonzero(~np.isnan(inside))[0]
    light = live[np.arange(origins.shape[0]) % live.size]
    probes = np.concatenate([inside[light][:, None], origins], axis=1).astype(np.float32)
    got = grt.sample_delta_lights(ctx, probes)
    index = got.view(np.int32)[:, 0]
    assert np.array_equal(index, light)
    want = ref.sample(table, index, origins)
    f = got.astype(np.float64)
    kind = table.type[index]
    directional = kind == DIRECTIONAL
    # directional: the staged record's own numbers, exactly
    assert np.array_equal(got[directional, 1:4], -records[index[directional], 4:7]) and np.isposinf(got[directional, 4]).all()
    assert np.array_equal(got[directional, 5:8], records[index[directional], 8:11]) and (got[directional, 9] == 1).all()
    near = ~directional
    with np.errstate(all="ignore"):
        dir_bound, size = _direction_error_bound(table, index, origins, want.distance)
        # ambiguous: c within its own error of one of the two cosines (the error of a dot product of two unit vectors: the direction's, three times, plus its own roundings)
        c_bound = 3 * dir_bound + 4 * EPS
        ambiguous = (kind == SPOT) & (want.margin <= c_bound)
    share = ambiguous.sum() / max(int((kind == SPOT).sum()), 1)
    assert ambiguous.sum() <= 0.05 * origins.shape[0], "%s: %d ambiguous probes" % (name, ambiguous.sum())
    decided = near & ~ambiguous
    assert np.array_equal(got[decided, 9] == 1, want.ok[decided]), "%s: the ok flag of probe %d is not float64's" % (name, np.nonzero(decided & ((got[:, 9] == 1) != want.ok))[0][0])
    ok = decided & want.ok
    assert ok.sum() > 100 or (kind == DIRECTIONAL).all()
    dropped = near & (got[:, 9] == 0)
    assert (got[dropped][:, 1:8] == 0).all()
    direction_error = (np.abs(f[ok, 1:4] - want.to_light[ok]).max(axis=1) / dir_bound[ok]).max(initial=0)
    distance_error = (np.abs(f[ok, 4] - want.distance[ok]) / (4 * EPS * size[ok])).max(initial=0)
    assert direction_error <= 1.0 and distance_error <= 1.0, (name, direction_error, distance_error)
    # point lights: intensity / d^2 -- the distance's relative error twice, the square, the division and (spots) the product: 4 roundings
    plain = ok & ((kind == POINT) | (want.falloff >= 1))
    relative = 2 * (4 * EPS * size / want.distance) + 6 * EPS
    scale = np.maximum(want.radiance, 1e-300)
    radiance_error = (np.abs(f[plain, 5:8] - want.radiance[plain]) / scale[plain] / relative[plain, None]).max(initial=0)
    assert radiance_error <= 1.0, (name, radiance_error)
    # the transition ring: the falloff, recovered from the radiance term (red channel) and the device's own distance
    ring = ok & want.in_transition
    worst_units, worst_light = 0.0, -1
    if ring.any():
        falloff = f[ring, 5] * f[ring, 4] ** 2 / table.intensity[index[ring], 0]
        unit = table.inv_transition[index[ring]] * (c_bound[ring] / np.sqrt(np.maximum(1.0 - want.cos_axis[ring] ** 2, 1e-12)) + EPS * math.pi) + EPS
        units = np.abs(falloff - want.falloff[ring]) / (unit + 8 * EPS * want.falloff[ring])   # (recovering it costs the product's and the square's roundings)
        worst_units = float(units.max()); worst_light = int(index[ring][units.argmax()])
    print("%s: %d probes, %d decided ok, %d in a transition ring, %d ambiguous (%.2f %% of the spot probes); direction %.2f, distance %.2f, radiance %.2f of their bounds; "
          "falloff worst %.4f units (light %d), bound %.4f" % (name, origins.shape[0], ok.sum(), ring.sum(), ambiguous.sum(), 100 * share, direction_error, distance_error,
                                                              radiance_error, worst_units, worst_light, FALLOFF_BOUND_UNITS))
    assert worst_units <= FALLOFF_BOUND_UNITS, (name, worst_units)


def test_ok_flags_at_the_special_origins(grt, bare):
    lib, ctx = bare
    lights = ref.lights_array([(POINT, (1, 2, 3), (0, 0, 1), (5, 6, 7), 0, 0), (SPOT, (0, 4, 0), (0, -1, 0), (9, 8, 7), 0.9, 0.5)])
    assert grt.upload_delta_lights(ctx, grt.delta_light_records(lights, [1.0, 1.0]), 1.0) == 0, lib.rt_last_error(ctx)
    probes = np.array([
        [0.25, 1, 2, 3],         # the point light's own position: d = 0
        [0.75, 0, 4, 0],         # the spot's own position
        [0.75, 0.5, 6, 0.5],     # behind the spot: falloff 0
        [0.75, 3, 3.5, 0],       # beside it, outside the cutoff cone
        [0.25, 1e30, 0, 0],      # the float32 length overflows: the distance is not finite, the sample is dropped
        [0.25, 1e15, 0, 0],      # finite: the radiance term underflows towards 0 and stays finite
        [0.75, 0, -1e15, 0],     # on the spot's axis, as far
        [0.75, 0.1, 1, 0.1],     # inside the beam
    ], np.float32)
    got = grt.sample_delta_lights(ctx, probes)
    assert np.isfinite(got[:, 1:4]).all() and np.isfinite(got[:, 5:]).all() and not np.isnan(got).any()
    assert got[:, 9].tolist() == [0, 0, 0, 0, 0, 1, 1, 1], got[:, 9]
    assert (got[:5, 1:8] == 0).all()
    assert (got[5:7, 5:8] >= 0).all() and (got[5:7, 5:8] < 1e-28).all() and np.allclose(got[5:7, 4], 1e15, rtol=1e-6)
    assert np.allclose(got[7, 5:8], np.array([9, 8, 7]) / (0.1 ** 2 + 9 + 0.1 ** 2), rtol=1e-6)


def test_a_spot_that_is_all_beam_is_the_point_light(grt, bare):
    lib, ctx = bare
    pi32 = float(np.float32(math.pi))   # (the upload's pi: cutoff <= pi holds, and cosf of it is -1)
    origins = cases.origin_grid(seed=41, n=12)
    probes = np.concatenate([np.full((origins.shape[0], 1), 0.5, np.float32), origins], axis=1)
    out = []
    for kind, cutoff in ((SPOT, pi32), (POINT, 0.0)):
        lights = ref.lights_array([(kind, (0.3, 3.0, -0.2), (0.2, -1.0, 0.1), (11, 7, 3), cutoff, cutoff)])
        assert grt.upload_delta_lights(ctx, grt.delta_light_records(lights, [1.0]), 1.0) == 0, lib.rt_last_error(ctx)
        out.append(grt.sample_delta_lights(ctx, probes))
    spot, point = out
    assert np.array_equal(spot[:, 9], point[:, 9]) and (point[:, 9] == 1).all()
    assert np.array_equal(spot[:, 1:5].view(np.uint32), point[:, 1:5].view(np.uint32))
    # the falloff is exactly 1 (c >= cos(beam) = -1), so the product intensity x 1 / d^2 is the point light's to the bit
    assert np.array_equal(spot[:, 5:8].view(np.uint32), point[:, 5:8].view(np.uint32))
    # ... on the back axis too (c == -1 == cos(cutoff) exactly: a cutoff of pi excludes no direction)
    behind = np.array([[0.5, 0, 5, 0], [0.5, 0, 3.5, 0]], np.float32)
    out = []
    for kind, cutoff in ((SPOT, pi32), (POINT, 0.0)):
        lights = ref.lights_array([(kind, (0, 3, 0), (0, -1, 0), (11, 7, 3), cutoff, cutoff)])
        assert grt.upload_delta_lights(ctx, grt.delta_light_records(lights, [1.0]), 1.0) == 0, lib.rt_last_error(ctx)
        out.append(grt.sample_delta_lights(ctx, behind))
    assert (out[0][:, 9] == 1).all() and np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    assert np.array_equal(out[0][:, 1:4], [[0, -1, 0], [0, -1, 0]])


# ---- frames ---------------------------------------------------------------------------------------------------------------

BLACK = np.zeros((1, 1, 4), np.float32)
# Direct light alone: num_bounces = 2 under a black sky. (The path length counts the bounce that only COLLECTS what a ray finds -- sort_rays ends
# every path at bounce num_bounces - 1 before it is shaded, as the reference does --, so a frame of num_bounces = 1 shades nothing: it is black
# but for emitters and sky seen by the camera. With 2 the first hit is shaded, its light sample traced, and its continuation ray finds only
# the black sky or a surface it is ended on -- the floor and the box are diffuse and not emissive, and the scene has no other surface, so the
# continuation contributes exactly 0: each pixel is exactly the one-bounce closed form.) Box filter: a sample lies inside its pixel.
FRAME = dict(num_bounces=2, reconstruction_filter=0, enable_next_event_estimation=1, delta_lights=1)


class Rendering:
    def __init__(self, grt, path, w, h, config, scheduler="merged", black_sky=True):
        self.grt, self.lib, self.w, self.h = grt, _lib(grt), w, h
        grt.config_reset(); grt.config_set(**config)
        self.scene = grt.Scene(path)
        grt.config_set(**config)
        self.pt = grt.Pathtracer(self.scene, w, h, device=0)
        self.pt.update()
        if black_sky:
            assert self.lib.rt_set_sky(self.pt.ctx, BLACK.ctypes.data, 1, 1, 1.0) == 0
        grt.set_scheduler(self.pt.ctx, scheduler)

    def render(self, samples, first=0, batch=16):
        for s in range(first, first + samples, batch):
            assert self.lib.rt_render_samples(self.pt.ctx, s, min(batch, first + samples - s)) == 0, self.lib.rt_last_error(self.pt.ctx)
        return self.pt.read_framebuffer()[:, :self.w].copy()

    def close(self):
        self.pt.close(); self.scene.close(); self.grt.config_reset()


@pytest.mark.parametrize("kind", ["point", "spot", "directional"])
def test_frame_lies_inside_the_closed_form(grt, tmp_path, kind):
    """A diffuse floor and a box under one light, one shaded bounce (FRAME), a pinhole camera, a black sky, 16 samples of 96 x 64 pixels: each pixel's mean lies
    between the minimum and the maximum of albedo / pi x radiance term x cos x visible over a 5 x 5 grid of its footprint, widened by 1e-4
    relative. Left out: pixels whose footprint sees two surfaces, a shadow edge, the edge of a spot's cones or (spot) its transition ring, at
    most 10 % of the frame (each of the two kinds)."""
    w, h = 96, 64
    r = Rendering(grt, cases.write_floor_scene(tmp_path, cases.EMITTERS[kind]), w, h, FRAME)
    try:
        lights = r.scene.delta_lights()
        assert lights.shape[0] == 1
        table = ref.Table(lights, [1.0])
        lo, hi, mixed, ring = cases.picture(r.pt.camera(), w, h, table, 0)
        frame = r.render(16).astype(np.float64)[..., :3]
        again = r.render(16)[..., :3]
        assert np.array_equal(again, frame.astype(np.float32))   # deterministic: the same samples, the same frame
        if kind == "spot":
            assert ring.sum() > 50 and (ring & ~mixed).sum() <= 0.10 * w * h, ring.sum()
            mixed = mixed | ring
        assert mixed.sum() <= 0.10 * w * h, "%d of %d pixels are left out" % (mixed.sum(), w * h)
        keep = ~mixed
        assert (lo[keep].min(axis=1) > 0).sum() > 200 and (hi[keep].max(axis=1) == 0).sum() > 20   # lit and dark pixels are both held
        below = keep[..., None] & (frame < lo * (1 - 1e-4) - 1e-30); above = keep[..., None] & (frame > hi * (1 + 1e-4) + 1e-30)
        bad = below | above
        print("%s: %d pixels held (%d of them dark), %d left out, %d outside" % (kind, keep.sum(), (keep & (hi.max(axis=2) == 0)).sum(), mixed.sum(), bad.any(axis=2).sum()))
        if bad.any():
            y, x, c = [int(v[0]) for v in np.nonzero(bad)]
            raise AssertionError("%s: pixel (%d, %d) channel %d is %.9g, outside [%.9g, %.9g]" % (kind, x, y, c, frame[y, x, c], lo[y, x, c], hi[y, x, c]))
    finally:
        r.close()


def _cornell(grt, scheduler, prepare=None, config=None, samples=(2, 3), size=(64, 64)):
    r = Rendering(grt, grt.scene_path("cornellbox"), size[0], size[1], dict(num_bounces=4, **(config or {})), scheduler, black_sky=False)
    try:
        if prepare:
            prepare(r)
        first, frame = 0, None
        for count in samples:
            frame = r.render(count, first, batch=count); first += count
        return frame, r.pt.counters().shadow[0]
    finally:
        r.close()


POINT_IN_BOX = ((0.0, 1.2, 0.0), (3.0, 2.5, 2.0))   # position and intensity of a point light inside the Cornell box (its room spans about [-1, 1] x [0, 2] x [-1, 1])


def _add_point(r, share=None):
    if share is not None:
        r.grt.config_set(delta_light_share=share)
    r.scene.add_point_light(*POINT_IN_BOX)
    r.pt.invalidate("delta_lights"); r.pt.update()


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_upload_then_clear_is_the_frame_that_never_uploaded(grt, scheduler):
    never, _ = _cornell(grt, scheduler)

    def on_then_off(r):
        _add_point(r)
        lit = r.render(2)
        r.scene.clear_delta_lights()
        r.pt.invalidate("delta_lights"); r.pt.update()
        on_then_off.lit = lit
    again, _ = _cornell(grt, scheduler, on_then_off)
    assert np.array_equal(never, again), scheduler
    assert not np.array_equal(never, on_then_off.lit) and np.isfinite(on_then_off.lit).all()
    assert on_then_off.lit[..., :3].mean() > never[..., :3].mean()   # the light adds light


def test_sky_sampling_with_the_table_cleared_is_untouched(grt):
    sun = np.ones((8, 16, 4), np.float32); sun[2, 5, :3] = 200.0

    def sky(r):
        assert r.lib.rt_set_sky(r.pt.ctx, sun.ctypes.data, 16, 8, 1.0) == 0

    def sky_after_lights(r):
        _add_point(r)
        sky(r)
        r.render(1)
        assert r.grt.upload_delta_lights(r.pt.ctx, None) == 0
    for scheduler in ("merged", "slots"):
        never, shadows = _cornell(grt, scheduler, sky, config=dict(sky_sampling=0.5))   # (the config key: the host class hands it to the device at every update)
        cleared, _ = _cornell(grt, scheduler, sky_after_lights, config=dict(sky_sampling=0.5))
        default, _ = _cornell(grt, scheduler, sky)
        assert np.array_equal(never, cleared), scheduler
        assert not np.array_equal(never, default) and shadows > 0


def test_the_share_changes_the_noise_and_not_the_mean(grt):
    """The Cornell box with its area emitter and a point light, 64 x 64, 64 samples, merged scheduler, with 0.25 and with 0.75 of the light
    samples for the point light: the means of the 8 x 8 pixel blocks agree within 4 standard errors of their difference, the error from the
    per-sample frames of the two renders themselves; fewer than 1 % of the blocks (and channels) may be outside."""
    per_sample = {}
    for share in (0.25, 0.75):
        r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=3, delta_light_share=share), "merged", black_sky=False)
        try:
            _add_point(r)
            records, cdf, staged_share = grt.read_delta_lights(r.pt.ctx)
            assert staged_share == np.float32(share) and records.shape[0] == 1
            # The frame buffer after sample s >= 1 is acc + (x_s - acc) / s (the reference's accumulation, AOV.h: sample 0 is replaced by sample 1),
            # so x_s = acc_before + s (acc_after - acc_before): samples 1 .. 64 are the 64 per-sample frames, and the frame buffer is their mean.
            frames, before = [], None
            for s in range(65):
                assert r.lib.rt_render_samples(r.pt.ctx, s, 1) == 0, r.lib.rt_last_error(r.pt.ctx)
                mean = r.pt.read_framebuffer()[:, :64, :3].astype(np.float64)
                if s >= 1:
                    frames.append(before + s * (mean - before))
                before = mean
            frames = np.stack(frames)
            assert frames.min() >= -1e-3 * np.abs(frames).mean() - 1e-3 * frames.max() / 64 and frames.max() > 0   # (radiance: none negative beyond the rounding of the differences)
            assert np.allclose(frames.mean(axis=0), mean, rtol=1e-3, atol=1e-4)
            per_sample[share] = frames.reshape(64, 8, 8, 8, 8, 3).mean(axis=(2, 4))   # [sample, block row, block column, channel]
        finally:
            r.close()
    a, b = per_sample[0.25], per_sample[0.75]
    difference = a.mean(axis=0) - b.mean(axis=0)
    error = np.sqrt(a.var(axis=0, ddof=1) / 64 + b.var(axis=0, ddof=1) / 64)
    outside = np.abs(difference) > 4.0 * error
    print("share 0.25 against 0.75: %d of %d block means outside 4 standard errors; worst %.2f; noise ratio %.2f" % (
        outside.sum(), outside.size, (np.abs(difference) / np.maximum(error, 1e-30)).max(), a.var(axis=0).mean() / b.var(axis=0).mean()))
    assert outside.sum() < 0.01 * outside.size
    assert not np.array_equal(a, b)


def test_variants_are_finite_and_equal_between_the_schedulers(grt, tmp_path):
    """The instances the launchers take with delta lights: _split_nmap (a normal map on the floor's material), SVGF frames, the slot scheduler."""
    import normal_map_reference
    normal_map_reference.write_tga(str(tmp_path / "n.tga"), normal_map_reference.random_normal_map(5, 16, 16))
    path = cases.write_floor_scene(tmp_path, cases.EMITTERS["point"] + cases.EMITTERS["spot"])
    for label, config, mapped in (("nmap", dict(FRAME, num_bounces=3), True), ("svgf", dict(FRAME, num_bounces=3, enable_svgf=1), False)):
        frames = {}
        for scheduler in ("merged", "slots"):
            r = Rendering(grt, path, 96, 64, config, scheduler, black_sky=False)
            try:
                if mapped:
                    t = r.scene.add_texture(str(tmp_path / "n.tga"), normal_map=True)
                    r.pt.close()
                    r.pt = grt.Pathtracer(r.scene, 96, 64, device=0)   # (textures reach the device when a Pathtracer is created)
                    for i in range(r.scene.material_count):
                        if r.scene.material_type(i) == grt.MATERIAL_DIFFUSE:
                            r.scene.set_material_normal_map(i, t)
                    r.pt.update()
                    grt.set_scheduler(r.pt.ctx, scheduler)
                frames[scheduler] = r.render(3, batch=1)
                assert r.pt.counters().shadow[0] > 0, label
            finally:
                r.close()
        assert np.isfinite(frames["merged"]).all() and frames["merged"][..., :3].max() > 0, label
        assert np.array_equal(frames["merged"], frames["slots"]), label


# ---- the material launch, entry by entry ----------------------------------------------------------------------------------

def _material_world(grt, oracle, tmp_path_factory):
    import material_cases
    return material_cases.World(grt, oracle, tmp_path_factory.mktemp("delta_material"), 0)


@pytest.fixture(scope="module")
def world(grt, oracle, tmp_path_factory):
    w = _material_world(grt, oracle, tmp_path_factory)
    yield w
    w.close()


def _delta_expectation(world, tables, launch, sky_share, share):
    """Per entry of a material launch: where its light sample goes, and its shadow entry in float64 -- material_reference.evaluate with the delta lights
    (the table in float64, the P_k and the CDF read back from the device) and the sky's share in its tables: the one restatement of every instance."""
    import copy
    import material_reference as mref
    import sky_sampling_reference
    with_delta = copy.copy(tables)
    with_delta.sky_share = float(np.float32(sky_share))
    with_delta.sky_tables = sky_sampling_reference.Tables(tables.sky) if sky_share > 0 else None
    records, cdf, _ = world.grt.read_delta_lights(world.ctx)
    with_delta.delta = mref.Delta(ref.Table(DELTA_LIGHTS, DELTA_WEIGHTS), share, records, cdf)
    r = mref.evaluate(world, with_delta, launch, world.bsdf_tables)
    where = np.where(r.route == mref.ROUTE_SKY, 0, np.where(r.route == mref.ROUTE_DELTA, 1, 2))
    return dict(r=r, where=where, u_emitter=r.u_emitter, origin=r.shadow_origin, to_light=r.shadow_direction, distance=r.shadow_distance, illumination=r.illumination,
                has_shadow=r.has_shadow, allowed=r.alive & r.allow_nee, robust=r.robust, textured=r.textured)


def _check_delta_entries(name, launch, got, shadow_at, x, bounds):
    """The shadow entries of the hits whose light sample went to a delta light, against float64, within material_checks.BOUNDS."""
    import material_checks as mc
    mine = x["allowed"] & (x["where"] == 1) & x["robust"]
    emitted = shadow_at >= 0
    wrong = mine & (emitted != x["has_shadow"])
    assert not wrong.any(), "%s: entry %d: a shadow ray %s, float64 says otherwise" % (name, np.nonzero(wrong)[0][0], "is emitted" if emitted[np.nonzero(wrong)[0][0]] else "is missing")
    index = np.nonzero(mine & emitted)[0]
    f = got.shadow_out[shadow_at[index]].view(np.float32).astype(np.float64)
    errors = {
        "shadow_origin": mc._point(f[:, 0:3], x["origin"][index]),
        "shadow_direction": np.abs(f[:, 3:6] - x["to_light"][index]).max(axis=1),
    }
    finite = np.isfinite(x["distance"][index])
    assert np.array_equal(np.isposinf(f[:, 6]), ~finite), "%s: RT_INFINITY exactly for the directional lights' shadow rays" % name
    errors["shadow_distance"] = mc._relative(f[finite, 6], x["distance"][index][finite], 1e-30)
    plain = ~x["textured"][index]
    errors["illumination"] = mc._per_channel(f[plain, 7:10], x["illumination"][index][plain])
    worst = {k: float(v.max(initial=0)) for k, v in errors.items()}
    for k, v in worst.items():
        assert np.isfinite(v) and v <= bounds[k], "%s: %s is %.3g from float64's, the bound is %.3g" % (name, k, v, bounds[k])
    return index.size, int((x["allowed"] & (x["where"] == 1) & ~x["robust"]).sum()), worst


@pytest.mark.parametrize("slot", [0, 1], ids=["diffuse", "plastic"])
def test_material_launch_under_a_delta_only_table(grt, world, slot):
    """Diffuse and plastic hits, per-bounce and merged launches, no triangle emitters: every light sample goes to a delta light (taken = 1)."""
    import material_cases as mcases
    import material_checks as mc
    tables = world.apply(mcases.SETUP["no_lights"])
    try:
        assert grt.upload_delta_lights(world.ctx, grt.delta_light_records(DELTA_LIGHTS, DELTA_WEIGHTS), 0.5) == 0, world.lib.rt_last_error(world.ctx)
        s, q, taken = ref.split(0.0, 0.5, emitters=False)
        launches = [mcases.per_bounce(world, "delta", slot, 1500, b, seed=3100 + 10 * slot + b) for b in (0, 2)] + [mcases.merged(world, "delta", slot, 2500, seed=3150 + slot)]
        for launch in launches:
            name = "delta_only/" + launch.name
            got = mc.device_launch(grt, world.ctx, launch, capacity=launch.entries.n + 37)
            trace_at, shadow_at = mc.match(launch, got, name)
            x = _delta_expectation(world, tables, launch, 0.0, 0.5)
            assert (x["where"] == 1).all()
            count, left_out, worst = _check_delta_entries(name, launch, got, shadow_at, x, mc.BOUNDS)
            assert count > 200 and left_out <= mc.NON_ROBUST_CAP * launch.entries.n, (name, count, left_out)
            print("%-40s %5d entries, %5d shadow entries held, %3d left out; " % (name, launch.entries.n, count, left_out) + " ".join("%s %.2g" % kv for kv in worst.items()))
    finally:
        grt.upload_delta_lights(world.ctx, None)
        world.apply(mcases.SETUP["default"])


@pytest.mark.parametrize("sky_share", [0.0, 0.25])
def test_material_launch_splits_its_light_samples(grt, world, sky_share):
    """Delta lights beside the triangle emitters (share 0.5) and, the second time, the sky (s = 0.25), MIS off: every hit's light sample goes
    where its DIM_NEE_LIGHT number says in float32 -- sky (an infinite shadow ray), delta light (held to float64), emitter (the plain
    launch's sample for the rescaled number, its illumination times 1 / (1 - taken))."""
    import copy
    import material_cases as mcases
    import material_checks as mc
    import material_reference as mref
    # the restatement's own split, first: the shares as float32, every number routed somewhere, the rescaled numbers starting at 0
    s_, q_, t_ = ref.split(0.25, 0.5, True)
    assert (s_, q_, t_) == (np.float32(0.25), np.float32(0.375), np.float32(0.625))
    to, u_d, u_e = ref.route(np.array([0.0, 0.2499, 0.25, 0.6249, 0.625, 0.99], np.float32), s_, q_, t_)
    assert to.tolist() == [0, 0, 1, 1, 2, 2] and u_d[2] == 0 and u_e[4] == 0
    assert ref.split(0.0, 0.5, False) == (np.float32(0), np.float32(1), np.float32(1))
    assert ref.split(0.25, 1.0, True) == (np.float32(0.25), np.float32(0.75), np.float32(1))
    assert ref.split(0.25, float(ONE_BELOW_ONE), True) == (np.float32(0.25), np.float32(0.75), np.float32(1))   # (next to 1 is 1: taken is not the float below it)
    setup = mcases.SETUP["mis_off"]
    tables = world.apply(setup)
    lib = world.lib
    lib.rt_set_sky_sampling.argtypes = [c_void_p, c_float]
    try:
        assert grt.upload_delta_lights(world.ctx, grt.delta_light_records(DELTA_LIGHTS, DELTA_WEIGHTS), 0.5) == 0, lib.rt_last_error(world.ctx)
        assert lib.rt_set_sky_sampling(world.ctx, sky_share) == 0
        s, q, taken = ref.split(sky_share, 0.5, emitters=True)
        launch = mcases.per_bounce(world, "split", 0, 3000, 1, seed=3300)
        name = "split_%g/%s" % (sky_share, launch.name)
        got = mc.device_launch(grt, world.ctx, launch, capacity=launch.entries.n + 37)
        trace_at, shadow_at = mc.match(launch, got, name)
        x = _delta_expectation(world, tables, launch, sky_share, 0.5)
        where = x["where"]
        assert np.array_equal(where, ref.route(tables.random(mref.DIM_NEE_LIGHT, *launch.paths()[1:4])[:, 0], s, q, taken)[0])
        assert all((where == k).sum() > 100 for k in ((0, 1, 2) if sky_share > 0 else (1, 2))), np.bincount(where)
        count, left_out, worst = _check_delta_entries(name, launch, got, shadow_at, x, mc.BOUNDS)
        # the emitters' share: the plain launch's reference on the rescaled number, illumination / (1 - taken)
        slot_, real, bounce, sample, submission = launch.paths()
        rescaled = copy.copy(tables)
        plain_random = tables.random

        def random(dimension, *key):
            v = plain_random(dimension, *key).copy()
            if dimension == mref.DIM_NEE_LIGHT:
                v[:, 0] = x["u_emitter"]
            return v
        rescaled.random = random
        r = mref.evaluate(world, rescaled, launch, world.bsdf_tables)
        mine = (where == 2) & r.robust & x["allowed"]
        assert not (mine & ((shadow_at >= 0) != r.has_shadow)).any(), name
        index = np.nonzero(mine & (shadow_at >= 0) & ~r.textured)[0]
        f = got.shadow_out[shadow_at[index]].view(np.float32).astype(np.float64)
        scaled = r.illumination[index] / (1.0 - float(taken))
        emitter_error = mc._per_channel(f[:, 7:10], scaled).max(initial=0)
        assert index.size > 100 and emitter_error <= mc.BOUNDS["illumination"], (name, index.size, emitter_error)
        assert (mc._relative(f[:, 6], r.shadow_distance[index], 1e-30) <= mc.BOUNDS["shadow_distance"]).all()
        # the sky's share: shadow rays to infinity, and only there and for the directional lights
        to_sky = (where == 0) & (shadow_at >= 0)
        assert np.isposinf(got.shadow_out[shadow_at[to_sky], 6].view(np.float32)).all()
        finite = (where == 2) & (shadow_at >= 0)
        assert np.isfinite(got.shadow_out[shadow_at[finite], 6].view(np.float32)).all()
        print("%-40s sky %d, delta %d (%d shadow entries held, %d left out), emitters %d (%d held, illumination within %.2g); " % (
            name, (where == 0).sum(), (where == 1).sum(), count, left_out, (where == 2).sum(), index.size, emitter_error) + " ".join("%s %.2g" % kv for kv in worst.items()))
    finally:
        lib.rt_set_sky_sampling(world.ctx, 0.0)
        grt.upload_delta_lights(world.ctx, None)
        world.apply(mcases.SETUP["default"])


# ---- the sort launch, entry by entry --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sort_world(grt, oracle, tmp_path_factory):
    import sort_cases
    w = sort_cases.World(grt, oracle, tmp_path_factory.mktemp("delta_sort"), 0)
    yield w
    w.close()


def _tables_with_share(tables, share):
    """The float64 reference's tables with `share` in the place of the sky's: what sort_rays multiplies an emitter hit's light pdf by 1 - of."""
    import copy
    import sky_sampling_reference
    t = copy.copy(tables)
    t.sky_share = float(np.float32(share))
    t.sky_tables = sky_sampling_reference.Tables(tables.sky) if t.sky_share > 0 else None
    return t


def _sub_launch(launch, index, name):
    import sort_reference as sref
    sub = sref.Launch(name, launch.entries.take(index), launch.frame_pixels, launch.frame_slots, bounce=launch.bounce, sample_index=launch.sample_index,
                      iteration=launch.iteration, slot_table=launch.slot_table, submission_birth=launch.submission_birth, aov=launch.aov)
    sub.gnd, sub.gid, sub.gsp = launch.gnd, launch.gid, launch.gsp
    return sub


def _sort_run(world, name, tables, launch, oracle_too):
    """test_gpu_sort.py's run: structure, device against float64 within sort_checks.BOUNDS with robust entries taking float64's outcome, and (for
    entries that are no miss: the oracle reads no sky table for them) device against the oracle under the same share, bit for bit."""
    import sort_cases as scases
    import sort_checks as schecks
    import sort_reference as sref
    e = launch.entries
    result = sref.evaluate(tables, launch, schecks.MARGINS)
    allowed = sref.allowed_outcomes(tables, launch, schecks.MARGINS, result)
    got = schecks.device_launch(world.grt, world.ctx, launch, scases.SENTINEL, capacity=e.n + 37)
    matched = schecks.check_structure(name, tables, launch, got, result, allowed, scases.SENTINEL)
    exact = np.zeros(e.n, bool)
    if oracle_too:
        want = schecks.oracle_launch(tables, launch, scases.SENTINEL)
        exact = ~e.inside & (e.triangle != sref.INVALID)
        schecks.check_identical(name, launch, got, matched, want, schecks.match(launch, want, name + " (oracle)"), exact, "the oracle under 1 - taken")
    errors = schecks.compare_with_reference(name, tables, launch, got, matched, result, schecks.BOUNDS)
    print("%-44s %6d entries, %6d bit for bit with the oracle; " % (name, e.n, exact.sum()) + " ".join("%s %.2g" % (q, v[0]) for q, v in errors.items()))
    return result


def _sort_launches(world, classes, seed):
    """Per-bounce launches at bounces 1 and 2 and the merged launch's entries, restricted to `classes`."""
    import sort_cases as scases
    import sort_reference as sref
    out = []
    for b in (1, 2):
        rng = np.random.default_rng(seed + b)
        px = scases.pixels_for(rng, 4000, world.frame_pixels, 1)
        out.append(scases.per_bounce(world, "bounce%d" % b, scases.make_entries(world, rng, px, b, classes=classes), b, seed=b, slots=1))
    merged = scases.merged_launch(world, scases.NUM_BOUNCES)[0]
    miss = merged.entries.triangle == sref.INVALID
    keep = np.nonzero(miss if classes == (scases.MISS,) else ~miss)[0]
    out.append(_sub_launch(merged, keep, "merged"))
    return out


@pytest.mark.parametrize("setup_name,share", [("default", 0.5), ("sky_share_0.25", 0.5), ("default", 1.0), ("sky_share_0.25", float(ONE_BELOW_ONE))],
                         ids=["s0_q0.5", "s0.25_q0.375", "taken1", "s0.25_next_to_1"])
def test_sort_launch_weighs_emitter_hits_with_one_minus_taken(grt, sort_world, setup_name, share):
    """rt_sort_rays under q > 0 (kernel_sort_split, kernel_sort_stream_split) on emitter and surface hits, MIS on: an emitter hit found by a ray
    that was allowed NEE adds throughput x emission x power_heuristic(brdf_pdf, light_pdf x (1 - taken)) -- taken = s + q, not s --, and with
    taken = 1 (a share of 1) every emitter hit is counted whole. Held to the float64 restatement of the sort launch with taken in the place of
    the sky's share, within sort_checks.BOUNDS, and to the oracle under the same number bit for bit."""
    import sort_cases as scases
    import sort_checks as schecks
    import sort_reference as sref
    world = sort_world
    setup = scases.SETUP[setup_name]
    tables = world.apply(setup)
    try:
        assert grt.upload_delta_lights(world.ctx, grt.delta_light_records(DELTA_LIGHTS, DELTA_WEIGHTS), share) == 0, world.lib.rt_last_error(world.ctx)
        if share == float(ONE_BELOW_ONE):   # s + (1 - s) share is the float below 1: taken is 1 all the same, or a light sample would reach the emitters with a weight of 1.7e7
            assert np.float32(0.25) + np.float32(np.float32(0.75) * ONE_BELOW_ONE) == ONE_BELOW_ONE
        s, q, taken = ref.split(setup.sky_sampling, share, emitters=True)
        assert q > 0 and (taken == 1) == (share > 0.99)
        with_taken = _tables_with_share(tables, taken)
        classes = (scases.EMITTER, scases.EMITTER, scases.DIFFUSE, scases.PLASTIC, scases.DIELECTRIC, scases.CONDUCTOR)
        for launch in _sort_launches(world, classes, 4100):
            name = "%s_share%g/%s" % (setup_name, share, launch.name)
            result = _sort_run(world, name, with_taken, launch, oracle_too=True)
            weighed = np.isfinite(result.light_pdf) & np.isfinite(result.weight)
            if taken == 1:
                assert not weighed.any() and not np.isfinite(result.light_pdf).any(), name   # count_light: no emitter hit is weighed
            else:
                # the check is sharp: with the sky's share in the place of taken the weights are elsewhere, by far more than the bound on the frames
                other = sref.evaluate(tables, launch, schecks.MARGINS)
                apart = np.abs(result.weight[weighed] - other.weight[weighed])
                assert weighed.sum() > 100 and np.nanmedian(apart) > 1e-4 and (apart > 1e-3).sum() > 50, (name, weighed.sum(), np.nanmedian(apart))   # (sort_checks.BOUNDS holds the frames to 9.5e-6)
    finally:
        grt.upload_delta_lights(world.ctx, None)
        world.apply(scases.SETUP["default"])   # (sets the sky's share again too)


@pytest.mark.parametrize("setup_name", ["default", "sky_share_0.25"], ids=["s0", "s0.25"])
def test_sort_launch_adds_a_sky_miss_whole_without_sky_sampling(grt, sort_world, setup_name):
    """Rays that escape under q > 0. With s = 0 (the sky's tables are null: rt_set_sky has just dropped them and no render built them) a miss adds
    throughput x sky whole, allowed NEE or not; with s = 0.25 it is weighed against s x the sky's pdf -- s, not taken. The plain restatement."""
    import sort_cases as scases
    world = sort_world
    setup = scases.SETUP[setup_name]
    tables = world.apply(setup)
    try:
        assert grt.upload_delta_lights(world.ctx, grt.delta_light_records(DELTA_LIGHTS, DELTA_WEIGHTS), 0.5) == 0, world.lib.rt_last_error(world.ctx)
        assert tables.sky_share == setup.sky_sampling
        for launch in _sort_launches(world, (scases.MISS,), 4200):
            e = launch.entries
            assert e.allow_nee.sum() > 100 or launch.name == "merged"
            result = _sort_run(world, "%s_miss/%s" % (setup_name, launch.name), tables, launch, oracle_too=False)
            assert (e.triangle == -1).all() and result.miss.sum() > 0.5 * e.n   # (the rest scatter inside a medium before they escape)
            if setup.sky_sampling == 0:
                assert np.isnan(result.weight).all()
    finally:
        grt.upload_delta_lights(world.ctx, None)
        world.apply(scases.SETUP["default"])
