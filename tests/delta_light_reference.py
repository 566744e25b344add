"""numpy float64 restatement of the delta emitters -- point, spot and directional lights in next-event estimation -- for
test_delta_lights.py (the host's records against this) and test_gpu_delta_lights.py (the device against this). Written from the model, not
from the kernels: float32 inputs are taken exactly, every operation is float64. The oracle does not know delta lights; this is the pin.

* the table: P_k = w_k / sum(w) and the inclusive, normalised CDF, 1 from the last light of positive weight on;
* the selection: the first entry of the CDF that is >= u (searchsorted, side "left") -- decided on the float32 CDF the device holds;
* the sample a light offers an origin: unit direction, distance, radiance term (intensity x falloff / d^2, or the irradiance), with Mitsuba's
  spot falloff (1 inside the beam, 0 outside the cutoff, linear in the ANGLE between), and the margin by which each deciding comparison
  (c against the two cosines) is taken;
* the selection weights and the automatic share of the host classes;
* the split of a light sample between sky, delta lights and emitters, decided in float32 as the kernel decides it;
* the closed form of a diffuse surface under one light.
"""
import numpy as np

POINT, SPOT, DIRECTIONAL = 0, 1, 2
ONE_BELOW_ONE = np.float32(np.nextafter(np.float32(1), np.float32(0)))   # 0x1.fffffep-1
LUMINANCE = np.array([np.float32(0.299), np.float32(0.587), np.float32(0.114)], np.float64)   # rt_shading.h: luminance


def lights_array(rows):
    """(N, 12) float32 {type, position[3], direction[3], intensity[3], cutoff, beam} from tuples (type, position, direction, intensity, cutoff, beam)."""
    out = np.zeros((len(rows), 12), np.float32)
    for i, (kind, position, direction, intensity, cutoff, beam) in enumerate(rows):
        out[i] = [kind, *position, *direction, *intensity, cutoff, beam]
    return out


class Table:
    """What rt_upload_delta_lights stages, in float64: type, position, unit direction, intensity, the spot constants, P_k and the CDF."""

    def __init__(self, lights, weights):
        l = np.asarray(lights, np.float32).reshape(-1, 12).astype(np.float64)
        w = np.asarray(weights, np.float32).astype(np.float64)
        self.n = l.shape[0]
        self.type = l[:, 0].astype(np.int32)
        self.position = np.where((self.type == DIRECTIONAL)[:, None], 0.0, l[:, 1:4])
        d = l[:, 4:7]
        with np.errstate(all="ignore"):
            self.direction = np.where((self.type == POINT)[:, None], [0.0, 0.0, 1.0], d / np.sqrt((d * d).sum(axis=1))[:, None])
        self.intensity = l[:, 7:10]
        spot = self.type == SPOT
        self.cutoff = np.where(spot, l[:, 10], np.pi)
        self.beam = np.where(spot, l[:, 11], np.pi)
        # the cosines and the reciprocal are float32 constants of the staged record: the kernel compares and multiplies with THOSE
        self.cos_cutoff = np.where(spot, np.cos(l[:, 10]).astype(np.float32), -1.0).astype(np.float64)
        self.cos_beam = np.where(spot, np.cos(l[:, 11]).astype(np.float32), -1.0).astype(np.float64)
        with np.errstate(all="ignore"):
            self.inv_transition = np.where(spot & (l[:, 10] > l[:, 11]), 1.0 / (l[:, 10] - l[:, 11]), 0.0)
        self.weight = w
        total = w.sum()
        self.pdf = w / total
        last_positive = int(np.nonzero(w > 0)[0][-1])
        self.cdf = np.cumsum(w) / total
        self.cdf[last_positive:] = 1.0


def select(cdf32, u):
    """binary_search on the device's own float32 CDF: the first entry >= u."""
    return np.searchsorted(np.asarray(cdf32, np.float32), np.asarray(u, np.float32), side="left").astype(np.int32)


class Sample:
    pass


def sample(table, index, origin):
    """The sample light `index` offers `origin` ((N,) and (N, 3), float32 values taken exactly). to_light, distance (inf: directional),
    radiance (N, 3), falloff, ok; cos_axis (spots: dot(-to_light, axis)) and margin: how far cos_axis is from the nearer of the two cosines
    (inf for other lights)."""
    o = np.asarray(origin).astype(np.float64)   # (float32 probes are taken exactly; float64 points are the model's own)
    kind = table.type[index]
    s = Sample()
    with np.errstate(all="ignore"):
        to_light = table.position[index] - o
        d = np.sqrt((to_light * to_light).sum(axis=1))
        to_light = to_light / d[:, None]
        axis = table.direction[index]
        c = -(to_light * axis).sum(axis=1)
        angle = np.arccos(np.clip(c, -1.0, 1.0))
        outside = (c <= table.cos_cutoff[index]) & (table.cos_cutoff[index] > -1.0)   # (a cutoff of pi excludes no direction, the back axis included)
        falloff = np.where(outside, 0.0, np.where(c >= table.cos_beam[index], 1.0, (table.cutoff[index] - angle) * table.inv_transition[index]))
        falloff = np.where(kind == SPOT, falloff, 1.0)
        radiance = table.intensity[index] * (falloff / (d * d))[:, None]
        directional = kind == DIRECTIONAL
        s.to_light = np.where(directional[:, None], -axis, to_light)
        s.distance = np.where(directional, np.inf, d)
        s.radiance = np.where(directional[:, None], table.intensity[index], radiance)
        s.falloff = falloff
        s.cos_axis = c
        s.margin = np.where(kind == SPOT, np.minimum(np.abs(c - table.cos_cutoff[index]), np.abs(c - table.cos_beam[index])), np.inf)
        s.in_transition = (kind == SPOT) & (c > table.cos_cutoff[index]) & (c < table.cos_beam[index])
        s.ok = np.where(directional, True, (d > 0) & np.isfinite(d) & (falloff > 0)) & np.isfinite(s.radiance).all(axis=1) & (table.pdf[index] > 0)
    return s


def luminance(rgb):
    return (np.asarray(rgb, np.float32).astype(np.float64) * LUMINANCE).sum(axis=-1)


def weights(lights, scene_radius):
    """The host's selection weights: point 4 pi L(I); spot 2 pi L(I) (1 - (cos beam + cos cutoff) / 2); directional pi R^2 L(E)."""
    l = np.asarray(lights, np.float32).reshape(-1, 12).astype(np.float64)
    lum = luminance(l[:, 7:10])
    kind = l[:, 0].astype(np.int32)
    spot = 2.0 * np.pi * lum * (1.0 - 0.5 * (np.cos(l[:, 11]) + np.cos(l[:, 10])))
    return np.where(kind == POINT, 4.0 * np.pi * lum, np.where(kind == SPOT, spot, np.pi * scene_radius ** 2 * lum))


def automatic_share(weights32, lights_total_weight):
    """P_delta / (P_delta + pi x lights_total_weight) inside [0.05, 0.95], from the float32 weights of the records."""
    power = np.asarray(weights32, np.float32).astype(np.float64).sum()
    return float(np.clip(power / (power + np.pi * float(lights_total_weight)), 0.05, 0.95))


def split(sky_share, delta_share_of_rest, emitters):
    """(s, q, taken) as float32, as the device settles them per render: q = (1 - s) share with emitters, all the sky leaves without."""
    s = np.float32(sky_share)
    if emitters and np.float32(delta_share_of_rest) < 1:
        q = np.float32((np.float32(1) - s) * np.float32(delta_share_of_rest))
        taken = np.float32(min(np.float32(s + q), np.float32(1)))
        if taken >= ONE_BELOW_ONE:   # (next to 1 is 1: no light sample reaches the emitters with a weight of 1e7)
            q, taken = np.float32(np.float32(1) - s), np.float32(1)
    else:
        q = np.float32(np.float32(1) - s); taken = np.float32(1)
    return s, q, taken


def route(rand_light_x, s, q, taken):
    """Where a light sample goes (0 sky, 1 delta, 2 emitters) and the rescaled random number, in float32 as next_event_estimation computes them."""
    x = np.asarray(rand_light_x, np.float32)
    where = np.where(x < s, 0, np.where(x < taken, 1, 2))
    with np.errstate(all="ignore"):
        u_delta = np.minimum(((x - s) / q).astype(np.float32), ONE_BELOW_ONE)
        u_emitter = np.minimum(((x - taken) / np.float32(np.float32(1) - taken)).astype(np.float32), ONE_BELOW_ONE)
    return where, u_delta, u_emitter


def diffuse_radiance(albedo, normal, point, table, index, visible=1.0):
    """albedo / pi x radiance term x max(cos, 0) x visible at surface points (N, 3) with unit normals: one light's direct light on a diffuse surface."""
    s = sample(table, np.full(point.shape[0], index, np.int32), point)
    cos = np.maximum((s.to_light * normal).sum(axis=1), 0.0)
    out = np.asarray(albedo, np.float64) / np.pi * s.radiance * (cos * visible)[:, None]
    return np.where(s.ok[:, None], out, 0.0), s
