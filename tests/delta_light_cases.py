"""Tables, probe grids and scenes of the delta-emitter tests (test_delta_lights.py on the CPU, test_gpu_delta_lights.py on the device).

* TABLES: 1, 2, 3 and 65 lights of mixed types; the 3- and the 65-light table have a light of ZERO weight in the middle (never selected),
  the 65-light one is past a wave's width and has weights over four decades.
* origin grids around a light, with the special origins of the ok flag (the light's own position, behind a spot, 1e30 away).
* scene files: one emitter of each type with its defaults; a diffuse floor with a box under one light, and the float64 picture of it --
  a ray caster for a plane and an axis-aligned box, which is all the scene is.
"""
import os

import numpy as np

import delta_light_reference as ref
from delta_light_reference import POINT, SPOT, DIRECTIONAL, ONE_BELOW_ONE


def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        kind = (POINT, SPOT, DIRECTIONAL)[i % 3]
        position = rng.uniform(-4, 4, 3) + [0, 6, 0]
        direction = rng.normal(size=3) * rng.uniform(0.2, 5.0)   # (any length: normalised on upload)
        direction[1] = -abs(direction[1]) - 0.3
        intensity = rng.uniform(0.5, 40.0, 3)
        cutoff = rng.uniform(0.3, 1.4)
        rows.append((kind, position, direction, intensity, cutoff, cutoff * rng.uniform(0.3, 1.0)))
    weights = (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    return ref.lights_array(rows), weights


def _tables():
    out = {}
    out["one_spot"] = (ref.lights_array([(SPOT, (0.5, 4.0, -0.25), (0.1, -1.0, 0.2), (30, 20, 10), 0.7, 0.4)]), np.array([2.5], np.float32))
    l, w = _mixed(2, 21); out["two"] = (l, w)
    l, w = _mixed(3, 22); w[1] = 0.0; out["three_zero_middle"] = (l, w)
    l, w = _mixed(65, 23); w[31] = 0.0; w[32] = 0.0; out["sixty_five"] = (l, w)
    return out


TABLES = _tables()


def _neighbours(values):
    v = np.asarray(values, np.float32)
    out = np.concatenate([v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2)), np.array([0.0, ONE_BELOW_ONE], np.float32)])
    return np.unique(out[(out >= 0) & (out < 1)])


def edge_numbers(cdf32):
    """Every CDF entry, its two float32 neighbours, 0 and 0x1.fffffep-1."""
    return _neighbours(cdf32)


def inside_numbers(cdf32):
    """One random number inside every light's interval of the CDF (None for an empty interval): selects that light."""
    lower = np.concatenate([[0.0], np.asarray(cdf32, np.float64)[:-1]])
    mid = ((lower + np.asarray(cdf32, np.float64)) / 2).astype(np.float32)
    return np.where(np.asarray(cdf32, np.float64) > lower, np.minimum(mid, ONE_BELOW_ONE), np.nan).astype(np.float32)


def origin_grid(seed=31, n=17):
    """n^3 origins in a box of +-8 around (0, 3, 0), jittered: in front of, beside and behind the lights of the tables above."""
    rng = np.random.default_rng(seed)
    g = (np.arange(n) + 0.5) / n * 16.0 - 8.0
    o = np.stack(np.meshgrid(g, g + 3.0, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return (o + rng.uniform(-0.3, 0.3, o.shape)).astype(np.float32)


# ---- scene files ------------------------------------------------------------------------------------------------------

SENSOR = ('<sensor type="perspective"><float name="fov" value="45"/><transform name="toWorld"><lookat origin="0, 7, 5" target="0, 0, 0" up="0, 1, 0"/></transform></sensor>')
ALBEDO = (0.7, 0.5, 0.3)
FLOOR_HALF = 40.0
BOX_MIN, BOX_MAX = np.array([-0.6, 0.0, -0.4]), np.array([0.3, 0.9, 0.5])
BOX_ALBEDO = (0.2, 0.6, 0.4)

EMITTERS = {
    "point": '<emitter type="point"><point name="position" x="1.0" y="3.0" z="0.5"/><rgb name="intensity" value="30, 28, 25"/></emitter>',
    "spot": ('<emitter type="spot"><transform name="toWorld"><lookat origin="1.2, 2.5, 0.8" target="-0.3, 0, -0.3" up="0, 1, 0"/></transform>'
             '<rgb name="intensity" value="60, 50, 40"/><float name="cutoffAngle" value="23"/><float name="beamWidth" value="21"/></emitter>'),
    "directional": '<emitter type="directional"><vector name="direction" x="-0.4" y="-1.0" z="-0.3"/><rgb name="irradiance" value="2.0, 1.8, 1.5"/></emitter>',
}


def write_floor_scene(directory, emitter_xml, name="floor", box=True, extra=""):
    """A diffuse floor (y = 0, albedo ALBEDO), a diffuse box standing on it, a pinhole camera looking down at them, the given emitters."""
    os.makedirs(str(directory), exist_ok=True)
    c, h = (BOX_MIN + BOX_MAX) / 2, (BOX_MAX - BOX_MIN) / 2
    xml = ('<scene version="0.5.0"><integrator type="path"><integer name="maxDepth" value="1"/></integrator>' + SENSOR +
           '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><scale value="%g"/></transform>'
           '<bsdf type="diffuse"><rgb name="reflectance" value="%g, %g, %g"/></bsdf></shape>' % ((FLOOR_HALF,) + ALBEDO))
    if box:
        xml += ('<shape type="cube"><transform name="toWorld"><scale x="%.9g" y="%.9g" z="%.9g"/><translate x="%.9g" y="%.9g" z="%.9g"/></transform>'
                '<bsdf type="diffuse"><rgb name="reflectance" value="%g, %g, %g"/></bsdf></shape>' % (tuple(h) + tuple(c) + BOX_ALBEDO))
    path = os.path.join(str(directory), name + ".xml")
    with open(path, "w") as f:
        f.write(xml + emitter_xml + extra + "</scene>")
    return path


def _box_hit(o, d, lo, hi):
    """Slab test, float64: (t_near, axis of entry, hit) for rays (N, 3); t_near > 0 only."""
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
    tmin, tmax = np.minimum(t0, t1), np.maximum(t0, t1)
    near, far = tmin.max(axis=1), tmax.min(axis=1)
    return near, tmin.argmax(axis=1), (near <= far) & (near > 1e-9)


def picture(camera, width, height, table, light, sub=5, box=True):
    """The float64 picture of the floor scene under light `light` of `table`: for every pixel the minimum and maximum over a sub x sub grid of
    its footprint (corners included) of albedo / pi x radiance term x cos x visible at the first hit, and whether the footprint is `mixed`:
    it sees two surfaces, or a lit and a shadowed point, or (spots) points on both sides of a cone, or a point outside the floor.
    Returns (lo, hi, mixed, transition): (H, W, 3), (H, W, 3), (H, W) bool, (H, W) bool (some point in a spot's transition ring)."""
    pos = np.array(camera.position[:], np.float64); blc = np.array(camera.bottom_left_corner[:], np.float64)
    xa = np.array(camera.x_axis[:], np.float64); ya = np.array(camera.y_axis[:], np.float64)
    f = np.linspace(0.0, 1.0, sub)
    px = (np.arange(width)[None, :, None, None] + f[None, None, None, :]) + np.zeros((height, 1, sub, 1))
    py = (np.arange(height)[:, None, None, None] + f[None, None, :, None]) + np.zeros((1, width, 1, sub))
    d = blc + px[..., None] * xa + py[..., None] * ya
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    o = np.broadcast_to(pos, d.shape)
    with np.errstate(all="ignore"):
        t_floor = np.where(d[:, 1] < 0, -o[:, 1] / d[:, 1], np.inf)
    surface = np.where(np.isfinite(t_floor), 0, -1)
    t = t_floor.copy()
    normal = np.tile([0.0, 1.0, 0.0], (d.shape[0], 1))
    albedo = np.tile(np.array(ALBEDO, np.float64), (d.shape[0], 1))
    if box:
        tb, axis, hit = _box_hit(o, d, BOX_MIN, BOX_MAX)
        closer = hit & (tb < t)
        t = np.where(closer, tb, t)
        n_box = np.zeros_like(d); n_box[np.arange(d.shape[0]), axis] = -np.sign(d[np.arange(d.shape[0]), axis])
        normal = np.where(closer[:, None], n_box, normal)
        albedo = np.where(closer[:, None], np.array(BOX_ALBEDO, np.float64), albedo)
        surface = np.where(closer, 1 + axis * 2 + (n_box[np.arange(d.shape[0]), axis] > 0), surface)
    with np.errstate(all="ignore"):
        point = o + t[:, None] * d
    outside = (surface == 0) & ((np.abs(point[:, 0]) > FLOOR_HALF) | (np.abs(point[:, 2]) > FLOOR_HALF))
    point = np.where(np.isfinite(point), point, 0.0)
    index = np.full(d.shape[0], light, np.int32)
    s = ref.sample(table, index, point)   # (float64 points: the picture is the model's, not a probe's)
    visible = np.ones(d.shape[0], bool)
    if box:
        so = point + 1e-7 * normal
        tb, _, hit = _box_hit(so, s.to_light, BOX_MIN, BOX_MAX)
        visible = ~(hit & (tb < s.distance))
    cos = np.maximum((s.to_light * normal).sum(axis=1), 0.0)
    value = albedo / np.pi * s.radiance * (cos * visible)[:, None]
    value = np.where((s.ok & (surface >= 0))[:, None], value, 0.0)
    shape = (height, width, sub * sub)
    value = value.reshape(shape + (3,))
    surface = surface.reshape(shape); visible = visible.reshape(shape); outside = outside.reshape(shape)
    lit = (s.falloff > 0).reshape(shape); full = (s.falloff >= 1).reshape(shape); ring = s.in_transition.reshape(shape)
    facing = (cos > 0).reshape(shape)
    mixed = ((surface != surface[..., :1]).any(axis=2) | (visible != visible[..., :1]).any(axis=2) | outside.any(axis=2) | (surface < 0).any(axis=2)
             | (lit != lit[..., :1]).any(axis=2) | (full != full[..., :1]).any(axis=2) | (facing != facing[..., :1]).any(axis=2))
    return value.min(axis=2), value.max(axis=2), mixed, ring.any(axis=2)
