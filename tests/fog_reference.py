"""The fog volume restated in float64 and exact integers: what csrc/rt_fog.h and the ..._fog sort instances compute, for
test_fog.py (the restatement against itself and against quadrature) and test_gpu_fog.py (the device against the restatement).

* the slab clip of a segment against the box, with the rules for direction components of +-0 and origins on a face;
* the hashed pair of a segment's distance sample, in integers, and its two float32 numbers exactly;
* the channel choice (the device's float32 comparisons, restated in float32), the distance, the weights;
* Henyey-Greenstein eval and sample in the device's convention; the shadow factor;
* a numpy Monte Carlo of the whole estimator on the two closed-form scenes of the frame tests -- the white furnace and the light shaft --
  with the quadrature of the single-scatter integral beside it.
The oracle does not know the fog: this file is the only reference."""
import math

import numpy as np

MAX_BOUNCES = 128
M32 = 0xFFFFFFFF
ONE_OVER_MAX_UNSIGNED = np.array([0x2F7FFFFF], np.uint32).view(np.float32)[0]
FOUR_PI = 4.0 * math.pi


# ---- integers ---------------------------------------------------------------------------------------------------------

def pcg_hash(seed):
    state = (seed * 747796405 + 2891336453) & M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return ((word >> 22) ^ word) & M32


def hash_with(seed, h):
    seed = ((seed ^ 61) ^ h) & M32
    seed = (seed + (seed << 3)) & M32
    seed ^= seed >> 4
    seed = (seed * 0x27D4EB2D) & M32
    return seed


def random_key(pixel, bounce):
    """The path key of the fog's pair: bit 31 over pixel * RT_MAX_BOUNCES + bounce. random_sample's keys are (pixel * 7 + dimension) * 128 + bounce."""
    return 0x80000000 | ((pixel * MAX_BOUNCES + bounce) & M32)


def existing_keys(pixel, bounce):
    return [((pixel * 7 + d) * MAX_BOUNCES + bounce) & M32 for d in range(7)]


def random_pair_integers(pixel, bounce, sample_index):
    h = pcg_hash(random_key(pixel, bounce))
    return hash_with(sample_index & M32, h), hash_with((sample_index + 0xDEADBEEF) & M32, h)


def random_pair(pixel, bounce, sample_index):
    """The two float32 numbers, bit for bit: the integer rounded to float32 (nearest even), times 0x2f7fffff, rounded again."""
    a, b = random_pair_integers(pixel, bounce, sample_index)
    return np.float32(np.uint32(a)) * ONE_OVER_MAX_UNSIGNED, np.float32(np.uint32(b)) * ONE_OVER_MAX_UNSIGNED


# ---- the clip ---------------------------------------------------------------------------------------------------------

def clip(box_min, box_max, o, d, t_end):
    """[t0, t1] of the segment (o, d, [0, t_end]) inside the box, in float64 on the float32 inputs; None when empty or of length 0.
    A direction component of +-0: inside or outside that slab by the origin alone (faces included), no quotient formed."""
    t0, t1 = 0.0, float(t_end)
    for k in range(3):
        ok, dk, lo, hi = float(o[k]), float(d[k]), float(box_min[k]), float(box_max[k])
        if dk == 0.0:
            if not (lo <= ok <= hi):
                return None
            continue
        ta, tb = (lo - ok) / dk, (hi - ok) / dk
        t0 = max(t0, min(ta, tb)); t1 = min(t1, max(ta, tb))
    return (t0, t1) if t1 > t0 else None


def shadow_factor(box_min, box_max, sigma_t, o, d, max_distance):
    c = clip(box_min, box_max, o, d, max_distance)
    if c is None:
        return np.ones(3)
    return np.exp(-np.asarray(sigma_t, np.float64) * (c[1] - c[0]))


# ---- the distance sample ----------------------------------------------------------------------------------------------

def channel(rand_x, throughput):
    """The device's choice, in its own float32 arithmetic: a discrete outcome, so restated exactly."""
    t = np.asarray(throughput, np.float32); u = np.float32(rand_x)
    total = np.float32(np.float32(t[0] + t[1]) + t[2])
    if np.float32(u * total) < t[0]:
        return 0
    if np.float32(u * total) < np.float32(t[0] + t[1]):
        return 1
    return 2


def sample_distance(sigma_a, sigma_s, rand, L, throughput):
    """(scattered, distance, throughput') over a clipped length L, float64 on the float32 inputs (the channel as the device picks it)."""
    sa, ss, t = np.asarray(sigma_a, np.float64), np.asarray(sigma_s, np.float64), np.asarray(throughput, np.float32).astype(np.float64)
    if not ss.sum() > 0.0:
        return False, math.inf, t * np.exp(-sa * L)
    st = sa + ss
    wpdf = t / t.sum()
    y = float(rand[1])
    used = st[channel(rand[0], throughput)]
    distance = math.inf if y == 0.0 or used == 0.0 else -math.log(y) / used   # (the device: -logf(0) and x / 0 are +inf)
    tr = np.exp(-st * min(distance, L))
    if distance < L:
        return True, distance, t * ss * tr / (wpdf * st * tr).sum()
    return False, math.inf, t * tr / (wpdf * tr).sum()


# ---- the phase function -------------------------------------------------------------------------------------------------

def hg(cos_theta, g):
    """value = pdf. cos_theta against omega, the direction BACK along the arriving ray: g > 0 favours cos_theta = -1, straight on."""
    cos_theta = np.asarray(cos_theta, np.float64)
    if abs(g) < 1e-3:
        return np.full(cos_theta.shape, 1.0 / FOUR_PI)
    den = 1.0 + g * g + 2.0 * g * cos_theta
    return (1.0 - g * g) / (FOUR_PI * den * np.sqrt(den))


def hg_cos(g, u1):
    u1 = np.asarray(u1, np.float64)
    if abs(g) < 1e-3:
        return 1.0 - 2.0 * u1
    return -(1.0 + g * g - ((1.0 - g * g) / (1.0 + g - 2.0 * g * u1)) ** 2) / (2.0 * g)


def basis(n):
    """orthonormal_basis of rt_shading.h on (N, 3) unit vectors."""
    sign = np.copysign(1.0, n[:, 2])
    a = -1.0 / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    t = np.stack([1.0 + sign * n[:, 0] * n[:, 0] * a, sign * b, -sign * n[:, 0]], axis=1)
    s = np.stack([b, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
    return t, s


def hg_sample(omega, g, u1, u2):
    """sample_henyey_greenstein(omega, g, u1, u2) on (N, 3) omegas: the directions and their cosines against omega."""
    c = hg_cos(g, u1)
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    phi = 2.0 * math.pi * np.asarray(u2, np.float64)
    t, b = basis(omega)
    return (s * np.sin(phi))[:, None] * t + (s * np.cos(phi))[:, None] * b + c[:, None] * omega, c


# ---- vectorised clip for the Monte Carlo ----------------------------------------------------------------------------------

def clip_many(box_min, box_max, o, d, t_end):
    t0 = np.zeros(o.shape[0]); t1 = np.broadcast_to(np.asarray(t_end, np.float64), (o.shape[0],)).copy()
    inside = np.ones(o.shape[0], bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            par = d[:, k] == 0.0
            ta = (box_min[k] - o[:, k]) / np.where(par, 1.0, d[:, k]); tb = (box_max[k] - o[:, k]) / np.where(par, 1.0, d[:, k])
            t0 = np.where(par, t0, np.maximum(t0, np.minimum(ta, tb))); t1 = np.where(par, t1, np.minimum(t1, np.maximum(ta, tb)))
            inside &= ~par | ((o[:, k] >= box_min[k]) & (o[:, k] <= box_max[k]))
    ok = inside & (t1 > t0)
    return ok, np.where(ok, t0, 0.0), np.where(ok, t1, 0.0)


def uniform_sphere(u1, u2):
    z = 1.0 - 2.0 * u1
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(2 * math.pi * u2), r * np.sin(2 * math.pi * u2), z], axis=1)


# ---- the white furnace ------------------------------------------------------------------------------------------------------
# A sky of radiance 1 in every direction, a grey volume without absorption, nothing else: every path that leaves the box carries exactly 1.

def furnace_truncation_bound(box_min, box_max, sigma_t, num_bounces):
    """An upper bound of the probability that a path is cut by the bounce limit: a path ends at its scatter event of bounce num_bounces - 1,
    i.e. after scattering at every one of num_bounces bounces; no segment inside the box is longer than the diagonal, so each scatters with
    probability at most 1 - exp(-sigma_t * diagonal)."""
    diagonal = float(np.linalg.norm(np.asarray(box_max, np.float64) - np.asarray(box_min, np.float64)))
    return (1.0 - math.exp(-sigma_t * diagonal)) ** num_bounces


def furnace(box_min, box_max, sigma_s, g, num_bounces, o, d, rng, nee=False, sky_share=0.5, mis=True):
    """The estimator on N camera rays (o, d) under the sky of radiance 1 (pdf 1 / 4 pi), float64. nee: light samples at every scatter vertex,
    the sky with probability sky_share (the rest goes to emitters that give nothing), MIS by the power heuristic against the phase pdf; a
    miss after a scatter is weighed the other way round. Returns the N sample values."""
    box_min, box_max = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    n = o.shape[0]
    o, d = o.astype(np.float64).copy(), d.astype(np.float64).copy()
    value = np.zeros(n); alive = np.ones(n, bool); last_pdf = np.zeros(n); weighed = np.zeros(n, bool)
    p_sky = 1.0 / FOUR_PI
    for bounce in range(num_bounces):
        ok, t0, t1 = clip_many(box_min, box_max, o, d, np.inf)
        s = -np.log(1.0 - rng.random(n)) / sigma_s
        scatter = alive & ok & (s < t1 - t0)
        miss = alive & ~scatter
        w = np.where(weighed & nee, (last_pdf ** 2 / (last_pdf ** 2 + (sky_share * p_sky) ** 2)) if mis else 0.0, 1.0)
        value += np.where(miss, w, 0.0)
        alive = scatter
        if bounce == num_bounces - 1 or not alive.any():
            break
        o = o + (t0 + s)[:, None] * d
        if nee:
            pick_sky = rng.random(n) < sky_share
            to_sky = uniform_sphere(rng.random(n), rng.random(n))
            phase = hg(np.einsum("ij,ij->i", -d, to_sky), g)
            light_pdf = sky_share * p_sky
            wl = light_pdf ** 2 / (light_pdf ** 2 + phase ** 2) if mis else 1.0
            _, s0, s1 = clip_many(box_min, box_max, o, to_sky, np.inf)
            value += np.where(alive & pick_sky, phase * wl / light_pdf * np.exp(-sigma_s * (s1 - s0)), 0.0)
        d_new, c = hg_sample(-d, g, rng.random(n), rng.random(n))
        last_pdf = np.where(alive, hg(c, g), last_pdf); weighed = weighed | alive
        d = np.where(alive[:, None], d_new, d)
    return value


# ---- the light shaft ----------------------------------------------------------------------------------------------------------
# One point light of intensity I, a black sky, exactly one scattering event: L(o, d) = integral over the clipped segment of
# sigma_s T(t - t0) p(theta) I / r^2 T(shadow) dt.

def shaft_integrand(box_min, box_max, sigma_a, sigma_s, g, light, intensity, o, d, t, t0):
    """The integrand at distances t (K,) along ONE ray (o, d), scalar channel: sigma_a, sigma_s, intensity floats."""
    st = sigma_a + sigma_s
    x = o[None, :] + t[:, None] * d[None, :]
    to = light[None, :] - x
    r = np.linalg.norm(to, axis=1)
    to = to / r[:, None]
    _, s0, s1 = clip_many(box_min, box_max, x, to, r)
    return sigma_s * np.exp(-st * (t - t0)) * hg(to @ (-d), g) * intensity / (r * r) * np.exp(-st * (s1 - s0))


def shaft_quadrature(box_min, box_max, sigma_a, sigma_s, g, light, intensity, o, d, points=64):
    """Gauss-Legendre over the clipped segment (the integrand is smooth: the light lies outside the box, off the ray)."""
    c = clip(box_min, box_max, o, d, math.inf)
    if c is None:
        return 0.0
    x, w = np.polynomial.legendre.leggauss(points)
    t = 0.5 * (c[1] - c[0]) * (x + 1.0) + c[0]
    f = shaft_integrand(np.asarray(box_min, np.float64), np.asarray(box_max, np.float64), sigma_a, sigma_s, g, np.asarray(light, np.float64), intensity, np.asarray(o, np.float64), np.asarray(d, np.float64), t, c[0])
    return float(0.5 * (c[1] - c[0]) * (w * f).sum())


def shaft_monte_carlo(box_min, box_max, sigma_a, sigma_s, g, light, intensity, o, d, rng):
    """The device's estimator on N rays (o, d), scalar channel: a distance by the exponential of sigma_t, weight sigma_s / sigma_t at a
    scatter event, the light sample phase x I / r^2 x T(shadow) with pdf 1 and MIS weight 1. Returns the N sample values."""
    box_min, box_max, light = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64), np.asarray(light, np.float64)
    st = sigma_a + sigma_s
    n = o.shape[0]
    ok, t0, t1 = clip_many(box_min, box_max, o, d, np.inf)
    s = -np.log(1.0 - rng.random(n)) / st
    scatter = ok & (s < t1 - t0)
    x = o + (t0 + s)[:, None] * d
    to = light[None, :] - x
    r = np.linalg.norm(to, axis=1)
    to = to / r[:, None]
    _, s0, s1 = clip_many(box_min, box_max, x, to, r)
    value = (sigma_s / st) * hg(np.einsum("ij,ij->i", to, -d), g) * intensity / (r * r) * np.exp(-st * (s1 - s0))
    return np.where(scatter, value, 0.0)


def pixel_rays(camera, width, height, jitter, repeat=1):
    """Unit directions of a pinhole camera through (x + jx, y + jy) for all pixels, row-major, `repeat` times over: jitter (repeat * N, 2) per
    ray or (2,). camera: dict with bottom_left_corner, x_axis, y_axis (3,) each."""
    ys, xs = np.mgrid[0:height, 0:width]
    j = np.broadcast_to(np.asarray(jitter, np.float64), (repeat * width * height, 2))
    px = np.tile(xs.reshape(-1), repeat) + j[:, 0]; py = np.tile(ys.reshape(-1), repeat) + j[:, 1]
    v = camera["bottom_left_corner"][None, :] + px[:, None] * camera["x_axis"][None, :] + py[:, None] * camera["y_axis"][None, :]
    return v / np.linalg.norm(v, axis=1)[:, None]
