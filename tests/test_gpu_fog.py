"""The fog volume on the device against the float64 / integer restatement of fog_reference.py (the oracle does not know it),
on the cases of fog_cases.py.

* the segment step (rt_fog_segments): the hashed pair bit for bit; the clip, the distance, the weights and the vertex within bounds derived
  from the float32 roundings of the operations involved (derivations beside the bounds; nothing here is a measured number);
* the attenuation pass (rt_attenuate_shadow_rays) on queues of 0 .. 1 000 rays under both schedulers;
* identities, bit for bit, on the 64 x 64 Cornell box under both schedulers; the never-set frame against the oracle;
* frames against closed forms: absorption only, the white furnace, the light shaft;
* refusals.
Every test prints what it measured."""
import math

import numpy as np
import pytest

import fog_cases as cases
import fog_reference as ref
from fog_cases import FURNACE_BOUNCES, FURNACE_SIGMA, SHAFT

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
EPS = 2.0 ** -24   # half a float32 ulp of 1: one rounding to nearest
# A face distance is (b - o) / d: a difference and a quotient, two roundings, relative 2 EPS (1 + EPS) < 2.5 EPS of the value. t0 and t1 are maxima and
# minima of such values, of 0 and of t_end -- monotone, so they carry at most the largest error among the finite face distances.
FACE = 2.5 * EPS
# logf (at most 1 ulp = 2 EPS relative), the negation exact, the quotient by sigma_t one rounding
DISTANCE = 3.5 * EPS


def _lib(grt):
    lib = grt.device_lib()
    lib.rt_last_error.restype = __import__("ctypes").c_char_p
    return lib


class Rendering:
    def __init__(self, grt, path, w, h, config, scheduler="merged", sky=None):
        self.grt, self.lib, self.w, self.h = grt, _lib(grt), w, h
        grt.config_reset(); grt.config_set(**config)
        self.scene = grt.Scene(path)
        grt.config_set(**config)
        self.pt = grt.Pathtracer(self.scene, w, h, device=0)
        self.pt.update()
        if sky is not None:
            texel = np.array([sky, sky, sky, 1.0], np.float32)
            assert self.lib.rt_set_sky(self.pt.ctx, texel.ctypes.data, 1, 1, 1.0) == 0
        grt.set_scheduler(self.pt.ctx, scheduler)

    def fog(self, box_min, box_max, sigma_a, sigma_s, g=0.0):
        status = self.grt.set_fog_volume(self.pt.ctx, self.grt.fog_volume_record(box_min, box_max, sigma_a, sigma_s, g))
        assert status == 0, self.lib.rt_last_error(self.pt.ctx)

    def render(self, samples, first=0, batch=16):
        for s in range(first, first + samples, batch):
            assert self.lib.rt_render_samples(self.pt.ctx, s, min(batch, first + samples - s)) == 0, self.lib.rt_last_error(self.pt.ctx)
        return self.pt.read_framebuffer()[:, :self.w].copy()

    def camera(self):
        c = self.pt.camera()
        return {k: np.array(list(getattr(c, k)), np.float64) for k in ("position", "bottom_left_corner", "x_axis", "y_axis")}

    def close(self):
        self.pt.close(); self.scene.close(); self.grt.config_reset()


@pytest.fixture(scope="module")
def probing(grt):
    """A 64 x 64 context (the segment step needs the frame size and the RNG tables for its path numbers)."""
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=4))
    yield r
    r.close()


# ---- 1. segments ------------------------------------------------------------------------------------------------------------

def _face_distances(o, d):
    out = []
    for k in range(3):
        if float(d[k]) != 0.0:
            out += [(float(cases.BOX_MIN[k]) - float(o[k])) / float(d[k]), (float(cases.BOX_MAX[k]) - float(o[k])) / float(d[k])]
    return [abs(t) for t in out if math.isfinite(t)]


@pytest.mark.parametrize("volume", list(cases.VOLUMES))
def test_segments_match_float64(grt, probing, volume):
    sigma_a, sigma_s, g = cases.VOLUMES[volume]
    probing.fog(cases.BOX_MIN, cases.BOX_MAX, sigma_a, sigma_s, g)
    names, o, d, t_end, px, b, s = cases.segment_probes()
    n = len(names)
    throughputs = np.array([cases.THROUGHPUTS[i % len(cases.THROUGHPUTS)] for i in range(n)], np.float32)
    flagged = (np.arange(n) % 11 == 10).astype(np.uint32)
    probes = grt.fog_segment_probes(o, d, t_end, px, b, s, throughputs, flagged)
    out = grt.fog_segments(probing.pt.ctx, probes)
    f = out.view(np.float32)
    sa32, ss32 = np.array(sigma_a, np.float32), np.array(sigma_s, np.float32)
    st = sa32.astype(np.float64) + ss32.astype(np.float64)
    worst = dict(t=0.0, distance=0.0, weight=0.0, vertex=0.0)
    ties = clipped = scattered = 0
    for i in range(n):
        what = "%s %s path %s" % (volume, names[i], (int(px[i]), int(b[i]), int(s[i])))
        rx, ry = ref.random_pair(int(px[i]), int(b[i]), int(s[i]))
        assert out[i, 2] == rx.view(np.uint32) and out[i, 3] == ry.view(np.uint32), what   # the pair: bit for bit
        if flagged[i]:   # inside a dielectric's medium: untouched
            assert f[i, 0] == 0.0 and f[i, 1] == 0.0 and out[i, 4] == 0 and np.array_equal(out[i, 6:9], probes[i, 10:13]), what
            continue
        c = ref.clip(cases.BOX_MIN, cases.BOX_MAX, o[i], d[i], t_end[i])
        faces = _face_distances(o[i], d[i])
        t_error = FACE * max(faces) if faces else 0.0
        if c is None or c[1] - c[0] <= 2.0 * t_error:   # empty, or as short as the two ends' errors: the device may see it either way
            if c is not None:
                ties += 1
            if f[i, 1] > f[i, 0]:
                assert c is not None or "graze" in names[i] or "end_at_entry" in names[i], what
                assert f[i, 1] - f[i, 0] <= 2.0 * t_error + EPS * abs(f[i, 1]), what
            else:
                assert f[i, 0] == 0.0 and f[i, 1] == 0.0 and out[i, 4] == 0 and np.array_equal(out[i, 6:9], probes[i, 10:13]), what
            continue
        clipped += 1
        assert abs(f[i, 0] - c[0]) <= t_error + EPS * abs(c[0]) and abs(f[i, 1] - c[1]) <= t_error + EPS * abs(c[1]), (what, f[i, 0:2], c)
        if t_error:
            worst["t"] = max(worst["t"], abs(f[i, 0] - c[0]) / t_error, abs(f[i, 1] - c[1]) / t_error)
        L = c[1] - c[0]
        L_error = 2.0 * t_error + EPS * L   # the two ends, and the rounding of their difference
        did, distance, weight = ref.sample_distance(sa32, ss32, (rx, ry), L, throughputs[i])
        distance_error = DISTANCE * distance if math.isfinite(distance) else 0.0
        if math.isfinite(distance) and abs(distance - L) <= distance_error + L_error:   # the comparison distance < L may fall either way
            ties += 1
            continue
        assert bool(out[i, 4]) == did, (what, distance, L)
        length = distance if did else L
        length_error = distance_error if did else L_error
        # a channel's transmittance exp(-x), x = sigma_t * length: sigma_t is a rounded sum (EPS), the product one more (EPS), so x is off by
        # x (length_error / length + 2 EPS); expf adds 1 ulp (2 EPS). The weight multiplies throughput (exact), sigma_s (exact) and T, and divides by
        # a sum of three non-negative products wpdf * sigma_t * T: wpdf = t / (two additions) is 3 EPS, its two products 2 EPS more, the two
        # additions of the sum 2 EPS, the numerator's two products 2 EPS, the quotient 1: 10 EPS, taken as 16, on top of T's error twice
        # (numerator and denominator).
        x = st * length
        T_error = 2.0 * EPS + x * (length_error / length + 2.0 * EPS)
        weight_bound = 2.0 * T_error.max() + 16.0 * EPS
        got = f[i, 6:9].astype(np.float64)
        assert np.all(np.abs(got - weight) <= weight_bound * np.abs(weight)), (what, got, weight, weight_bound)
        if np.any(weight > 0):
            worst["weight"] = max(worst["weight"], float((np.abs(got - weight)[weight > 0] / (weight_bound * weight[weight > 0])).max()))
        if did:
            scattered += 1
            assert abs(f[i, 5] - distance) <= distance_error, (what, f[i, 5], distance)
            worst["distance"] = max(worst["distance"], abs(f[i, 5] - distance) / distance_error)
            along = c[0] + distance
            vertex = o[i].astype(np.float64) + along * d[i].astype(np.float64)
            # vertex = o + (t0 + s) * d: the sum t0 + s (its parts' errors and EPS), the product and the final sum one rounding each
            bound = np.abs(d[i]) * (t_error + distance_error + EPS * along) + EPS * np.abs(along * d[i]) + EPS * (np.abs(o[i]) + np.abs(along * d[i]))
            assert np.all(np.abs(f[i, 9:12] - vertex) <= bound * 1.0000001), (what, f[i, 9:12], vertex, bound)
            worst["vertex"] = max(worst["vertex"], float((np.abs(f[i, 9:12] - vertex)[bound > 0] / bound[bound > 0]).max()))
        else:
            assert f[i, 5] == np.inf, what
    print("%s: %d probes, %d clipped, %d scattered, %d near ties; worst error as a fraction of its bound: %s" % (volume, n, clipped, scattered, ties, worst))
    assert clipped > n // 3 and ties < n // 10
    if sum(sigma_s) > 0:
        assert scattered > 10


def test_segment_probe_contract(grt, probing):
    lib = _lib(grt)
    ctx = probing.pt.ctx
    assert grt.set_fog_volume(ctx, None) == 0
    one = grt.fog_segment_probes([(0, 0, 0)], [(0, 0, 1)], [np.inf], [0], [0], [0], [(1, 1, 1)])
    out = np.zeros((1, 16), np.uint32)
    assert lib.rt_fog_segments(ctx, one.ctypes.data, 1, out.ctypes.data) == RT_ERROR_NOT_READY
    assert b"no fog volume" in lib.rt_last_error(ctx)
    empty = np.zeros((1, 11), np.uint32)
    assert lib.rt_attenuate_shadow_rays(ctx, empty.ctypes.data, 1, empty.ctypes.data) == RT_ERROR_NOT_READY
    probing.fog(cases.BOX_MIN, cases.BOX_MAX, 0.1, 0.2)
    bad = one.copy(); bad[0, 8] = 128
    assert lib.rt_fog_segments(ctx, bad.ctypes.data, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG
    assert b"bounce" in lib.rt_last_error(ctx)
    assert grt.fog_segments(ctx, np.zeros((0, 16), np.uint32)).shape == (0, 16)


# ---- 2. the sort launch through rt_sort_rays_fog -----------------------------------------------------------------------------

SENTINEL = 0xFFC0DE42
FLAG_ALLOW_NEE, FLAG_INSIDE_MEDIUM, SHADOW_BOUNCE_0 = 1 << 31, 1 << 30, 1 << 30
DIM_BSDF_1 = 6


@pytest.mark.parametrize("count", [256, 1025])
@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_sort_launch_scatters_and_samples_lights(grt, probing, scheduler, count):
    """Missed rays of bounce 0 through the ..._fog sort instance (256 entries and one over a workgroup's 1 024), entry by entry against the segment probe -- the
    same device functions, so vertex and throughput agree bit for bit -- and against float64 for the phase direction and its pdf. Every scattered entry goes on
    from its vertex with RT_FLAG_ALLOW_NEE (the Cornell box has emitters) and the HG pdf; its light sample starts at the vertex itself (no epsilon offset);
    counters, statistics and sentinel words as the launch must leave them. The light samples all go to the box's triangle emitter (taken = 0): their
    direction, length and illumination against float64 (_check_light_samples). Surface hits, later bounces, the other kinds of light and their split: the tests below."""
    sigma_a, sigma_s, g = cases.VOLUMES["unequal"]
    probing.fog(cases.BOX_MIN, cases.BOX_MAX, sigma_a, sigma_s, g)
    ctx = probing.pt.ctx
    sample = 5
    q = cases.shadow_queue(count, seed=300 + count).view(np.float32)
    o, d = q[:, 0:3].copy(), q[:, 3:6].copy()
    pixels = np.arange(count, dtype=np.uint32)
    frame_pixels = probing.pt.pitch * 64
    seg = grt.fog_segments(ctx, grt.fog_segment_probes(o, d, np.full(count, np.inf, np.float32), pixels, 0, sample, np.ones((count, 3), np.float32)))
    scattered = seg[:, 4] == 1
    entries = np.zeros((count, 20), np.uint32); f = entries.view(np.float32)
    f[:, 0:3] = o; f[:, 3:6] = d
    entries[:, 6] = 0; entries[:, 7] = 0xFFFFFFFF; f[:, 8] = np.inf   # a miss
    entries[:, 10] = pixels
    f[:, 11:14] = 0.25   # (bounce 0: the kernel takes 1, not what the queue carries)
    kwargs = dict(capacity=count + 9, sentinel=SENTINEL)
    if scheduler == "merged":
        births = np.zeros(128, np.int32); births[0] = 7
        kwargs.update(iteration=7, slot_table=np.array([[sample, 7, 0, 0]], np.int32), submission_birth=births)
    else:
        kwargs.update(bounce=0, sample_index=sample)
    r = grt.sort_rays_fog(ctx, entries, frame_pixels, 1, **kwargs)
    n = int(scattered.sum())
    assert list(r.counters) == [0, 0, 0, 0, n, count], (list(r.counters), n)
    out = r.trace_out; fo = out.view(np.float32)
    assert np.all(out[n:] == SENTINEL) and np.all(out[:n, 6:10] == SENTINEL) and np.all(out[:n, 15] == SENTINEL) and np.all(out[:n, 18:20] == SENTINEL)   # untouched words
    assert np.all(r.material_out == SENTINEL)
    px = out[:n, 10] & ~np.uint32(FLAG_ALLOW_NEE | FLAG_INSIDE_MEDIUM)
    assert sorted(px.tolist()) == pixels[scattered].tolist()   # every scattered entry once
    assert np.all(out[:n, 10] & FLAG_ALLOW_NEE) and not np.any(out[:n, 10] & FLAG_INSIDE_MEDIUM)
    assert np.array_equal(out[:n, 0:3], seg[px, 9:12]) and np.array_equal(out[:n, 11:14], seg[px, 6:9])   # vertex and throughput: the segment step, bit for bit
    u = grt.random_samples(ctx, DIM_BSDF_1, px, 0, sample).astype(np.float64)
    want, c = ref.hg_sample(-d[px].astype(np.float64), g, u[:, 0], u[:, 1])
    # the direction: cos_theta from u1 (a handful of roundings, amplified by 1 / (1 + g - 2 g u)^2 <= 1 / (1 - |g|)^2 = 6.25), sin_theta = sqrt(1 - cos^2)
    # (absolute EPS / sin_theta), sincosf, the basis and the 3 x 3 product: 64 EPS per component covers it away from sin_theta = 0, taken absolute.
    direction_error = np.abs(fo[:n, 3:6] - want).max()
    assert direction_error <= 64 * EPS / max(1e-3, float(np.sqrt(1 - c * c).min())), direction_error
    # last_pdf = HG(dot(-d, direction_out)): checked against float64 on the device's own direction; the dot product 4 EPS absolute, amplified by
    # 3 g / (1 + g^2 - 2 |g|) <= 11.25 relative for g = 0.6, plus 6 roundings of the formula
    cos_out = np.einsum("ij,ij->i", -d[px].astype(np.float64), fo[:n, 3:6].astype(np.float64))
    pdf = ref.hg(cos_out, g)
    pdf_error = np.abs(fo[:n, 14] - pdf) / pdf
    assert pdf_error.max() <= (4 * 11.25 + 6) * EPS, pdf_error.max()
    # the light samples
    m = r.shadow_count
    sh = r.shadow_out; fs = sh.view(np.float32)
    assert 0 < m <= n and np.all(sh[m:] == SENTINEL)
    word = sh[:m, 10]
    assert np.all((word & SHADOW_BOUNCE_0) != 0) if scheduler == "merged" else np.all((word & SHADOW_BOUNCE_0) == 0)
    spx = word & ~np.uint32(SHADOW_BOUNCE_0)
    assert len(set(spx.tolist())) == m and set(spx.tolist()) <= set(px.tolist())   # at most one per scattered entry
    assert np.array_equal(sh[:m, 0:3], seg[spx, 9:12])   # from the vertex itself: no epsilon offset
    assert np.allclose(np.linalg.norm(fs[:m, 3:6], axis=1), 1.0, atol=1e-5) and np.all(fs[:m, 6] > 0) and np.all(np.isfinite(fs[:m, 7:10])) and np.all(fs[:m, 7:10] >= 0)
    kinds, worst = _check_light_samples(grt, probing.pt, sh[:m], px, seg, d, 0, sample, SplitShares(0.0, 0.0), None)
    assert kinds == (0, 0, m), kinds
    # the frames: a miss that did not scatter wrote its sky radiance, a scattered entry nothing
    assert not r.aov[0][px].any() and np.all(np.isfinite(r.aov[0]))
    if scheduler == "merged":
        assert r.stats[0, 0, 0] == count and r.stats[0, 1, 0] == m and r.stats[0, 2:, 0].sum() == 0
    print("%s, %d entries: %d scattered, %d light samples; direction error %.3g, pdf error %.3g" % (scheduler, count, n, m, direction_error, pdf_error.max()) +
          "; emitter samples' illumination %.3f of its bound" % worst)


# ... the other configurations the launch has to get right, each entry against float64. What every one of them shares:

DIM_RUSSIAN_ROULETTE, DIM_NEE_LIGHT, DIM_NEE_TRIANGLE = 2, 3, 4
SORT_G = 0.6                 # the phase function of these tests
# HG(cos) in float32 against float64 on the same unit vectors: the dot product is off by 4 EPS absolute, which the formula amplifies by at most
# 3 g / (1 - g)^2 = 11.25 (relative, g = 0.6), and the formula itself rounds 6 times
HG_ERROR = (4 * 11.25 + 6) * EPS


class SplitShares:
    """How a render splits its light samples, in the device's float32: s to the sky, q to the delta lights, taken = s + q, the rest to the triangle emitters
    (sky_sampling_prepare; delta_share: the upload's share of what the sky leaves, while triangle emitters exist)."""
    def __init__(self, sky, delta_share):
        self.s = np.float32(sky)
        self.q = np.float32(np.float32(1.0) - self.s) * np.float32(delta_share)
        self.taken = min(np.float32(self.s + self.q), np.float32(1.0))


ONE_BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)
RT_EPSILON = np.float64(np.float32(0.0001))


def _check_light_samples(grt, pt, shadow, scattered_pixels, seg, d_in, bounce, sample, shares, point_light):
    """Every light sample of a launch against float64: `shadow` are the launch's shadow records, seg the segment step of its entries (vertex, throughput'), d_in
    the entries' directions. By DIM_NEE_LIGHT.x (next_event_estimation<2>): below s the sky -- the direction of the sky's tables from the DIM_NEE_TRIANGLE pair, pdf
    s x p_sky, to infinity; below taken the point light (position, intensity) -- pdf q, weight 1; else a triangle emitter, picked by rt_sample_lights from the
    number rescaled to [0, 1) -- offset by RT_EPSILON on ITS side only, pdf luminance x d^2 / (cos x total weight) x (1 - taken), dropped unless that is finite and
    above 1e-4. Sky and emitter samples carry the power heuristic against the phase pdf. Returns the number of samples of each kind and the worst error as a
    fraction of its bound. The bounds: HG in float32 against float64 is HG_ERROR; the point light's term (direction 4 EPS per component, I / r^2 and the
    products and quotients of nee_finish) 24 EPS more; where the heuristic enters, HG counts three times (the value, and twice in the weight) and the light's pdf
    (10 EPS: test_sort_launch_surfaces_and_emitters_behind_the_fog) three times as well (twice in the weight, once as divisor), with 18 roundings of products."""
    ctx = pt.ctx
    f32 = np.float32
    px = shadow[:, 10] & 0x3FFFFFFF
    fs = shadow.view(np.float32)
    vertex = seg[:, 9:12].view(np.float32).astype(np.float64); throughput = seg[:, 6:9].view(np.float32).astype(np.float64)
    every = np.asarray(scattered_pixels, np.uint32)
    u_light = grt.random_samples(ctx, DIM_NEE_LIGHT, every, bounce, sample)
    u_triangle = grt.random_samples(ctx, DIM_NEE_TRIANGLE, every, bounce, sample)
    x = u_light[:, 0]
    to_sky = x < shares.s
    to_point = ~to_sky & (x < shares.taken)
    to_emitter = ~to_sky & ~to_point
    n = len(every)
    direction = np.zeros((n, 3)); length = np.zeros(n); term = np.zeros((n, 3)); valid = np.ones(n, bool); bound = np.zeros(n)
    back = -d_in[every].astype(np.float64)
    if to_sky.any():
        sky = grt.sample_sky_distribution(ctx, u_triangle[to_sky]).astype(np.float64)
        phase = ref.hg(np.einsum("ij,ij->i", back[to_sky], sky[:, 0:3]), SORT_G)
        light_pdf = np.float64(shares.s) * sky[:, 3]
        direction[to_sky] = sky[:, 0:3]; length[to_sky] = np.inf
        term[to_sky] = (phase * (light_pdf ** 2 / (light_pdf ** 2 + phase ** 2)) / light_pdf)[:, None] * grt.sample_sky(ctx, sky[:, 0:3].astype(np.float32)).astype(np.float64)
        bound[to_sky] = 3 * HG_ERROR + 18 * EPS
    if to_point.any():
        position, intensity = point_light
        away = np.asarray(position, np.float64)[None, :] - vertex[every[to_point]]
        r = np.linalg.norm(away, axis=1); away /= r[:, None]
        phase = ref.hg(np.einsum("ij,ij->i", back[to_point], away), SORT_G)
        direction[to_point] = away; length[to_point] = r
        term[to_point] = (phase / r ** 2 / np.float64(shares.q))[:, None] * np.asarray(intensity, np.float64)[None, :]
        bound[to_point] = HG_ERROR + 24 * EPS
    if to_emitter.any():
        rescaled = np.minimum(((x[to_emitter] - shares.taken) / f32(f32(1.0) - shares.taken)).astype(f32), ONE_BELOW_ONE)
        probes = np.stack([rescaled, u_light[to_emitter, 1], u_triangle[to_emitter, 0], u_triangle[to_emitter, 1]], axis=1)
        picked = grt.sample_lights(ctx, probes, use_lds=False).astype(np.float64)
        point, normal, emission = picked[:, 4:7], picked[:, 7:10], picked[:, 10:13]
        v = vertex[every[to_emitter]]
        side = np.copysign(1.0, np.einsum("ij,ij->i", v - point, normal))
        point = point + (side * RT_EPSILON)[:, None] * normal   # the emitter's side; the vertex has no surface to be offset from
        away = point - v
        r = np.linalg.norm(away, axis=1); away /= r[:, None]
        cos_light = np.abs(np.einsum("ij,ij->i", away, normal))
        power = 0.299 * emission[:, 0] + 0.587 * emission[:, 1] + 0.114 * emission[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            light_pdf = power * r ** 2 / (cos_light * pt.lights_total_weight) * np.float64(f32(1.0) - shares.taken)
            phase = ref.hg(np.einsum("ij,ij->i", back[to_emitter], away), SORT_G)
            t = (phase * (light_pdf ** 2 / (light_pdf ** 2 + phase ** 2)) / light_pdf)[:, None] * emission
        ok = np.isfinite(light_pdf) & (light_pdf > 1e-4 * (1 + 16 * EPS))
        unsure = np.isfinite(light_pdf) & (np.abs(light_pdf - 1e-4) <= 1e-4 * 16 * EPS)   # the rule pdf > 1e-4 may fall either way
        assert not unsure.any()
        direction[to_emitter] = away; length[to_emitter] = r; term[to_emitter] = np.where(ok[:, None], t, 0.0)
        valid[to_emitter] = ok
        bound[to_emitter] = 3 * HG_ERROR + 3 * 10 * EPS + 18 * EPS
    # the records: one per vertex with a valid sample, each where float64 puts it
    assert sorted(px.tolist()) == sorted(every[valid].tolist()), (len(px), valid.sum())
    where = {int(p): k for k, p in enumerate(every)}
    k = np.array([where[int(p)] for p in px], int)
    want = throughput[px] * term[k]
    assert np.array_equal(shadow[:, 0:3], seg[px, 9:12])   # from the vertex itself
    assert np.abs(fs[:, 3:6] - direction[k]).max() <= 16 * EPS   # (an emitter's point is itself a float32 product of the probe's; the epsilon offset two more roundings)
    finite = np.isfinite(length[k])
    assert np.all(np.isinf(fs[~finite, 6])) and np.all(np.abs(fs[finite, 6] - length[k][finite]) <= 8 * EPS * length[k][finite])
    error = np.abs(fs[:, 7:10] - want) / np.maximum(want, 1e-300) / bound[k][:, None]
    assert error.max() <= 1.0, (error.max(), np.unravel_index(error.argmax(), error.shape))
    return (int((to_sky & valid).sum()), int((to_point & valid).sum()), int((to_emitter & valid).sum())), float(error.max())


def _sort_entries(o, d, pixels, hits=None, flags=0, throughput=(1.0, 1.0, 1.0), last_pdf=0.0):
    n = len(pixels)
    e = np.zeros((n, 20), np.uint32); f = e.view(np.float32)
    f[:, 0:3] = o; f[:, 3:6] = d
    if hits is None:
        e[:, 7] = 0xFFFFFFFF; f[:, 8] = np.inf   # a miss
    else:
        e[:, 6:10] = hits
    e[:, 10] = np.asarray(pixels, np.uint32) | np.uint32(flags)
    f[:, 11:14] = np.asarray(throughput, np.float32); f[:, 14] = last_pdf
    return e


def _sort_launch(grt, ctx, scheduler, entries, bounce, sample, frame_pixels):
    kwargs = dict(capacity=len(entries) + 9, sentinel=SENTINEL)
    if scheduler == "merged":
        births = np.zeros(128, np.int32); births[0] = 7 - bounce
        kwargs.update(iteration=7, slot_table=np.array([[sample, 7 - bounce, 0, 0]], np.int32), submission_birth=births)
    else:
        kwargs.update(bounce=bounce, sample_index=sample)
    return grt.sort_rays_fog(ctx, entries, frame_pixels, 1, **kwargs)


def _segments(grt, ctx, entries, bounce, sample):
    """The segment step of every entry (the same device functions: bit for bit what the launch computes before Russian roulette)."""
    f = entries.view(np.float32)
    t_end = np.where(entries[:, 7] == 0xFFFFFFFF, np.float32(np.inf), f[:, 8])
    return grt.fog_segments(ctx, grt.fog_segment_probes(f[:, 0:3], f[:, 3:6], t_end, entries[:, 10] & 0x3FFFFFFF, bounce, sample, f[:, 11:14]))


def _rays_at_the_box(count, seed):
    q = cases.shadow_queue(count, seed).view(np.float32)[25:]   # (without the special segments: unit directions)
    return q[:, 0:3].copy(), q[:, 3:6].copy()


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
@pytest.mark.parametrize("sky_share", [0.0, 0.25])
def test_sort_launch_light_samples_delta_only_and_split_with_the_sky(grt, tmp_path, scheduler, sky_share):
    """One point light and no triangle emitter (taken = 1): every scatter vertex has a light sample, whose illumination is compared with float64. sky_share 0:
    the point light alone, pdf 1, weight 1. sky_share 0.25: DIM_NEE_LIGHT.x below the share sends the sample to the sky -- the direction of the sky's tables from
    the DIM_NEE_TRIANGLE pair, pdf share x p_sky, the power heuristic against the phase pdf, a ray to infinity -- and above it to the light with pdf 0.75."""
    I, light = cases.SHAFT_INTENSITY, np.array(cases.SHAFT_LIGHT, np.float64)
    r = Rendering(grt, cases.write_empty_scene(tmp_path, "sort_delta", emitter_xml=cases.shaft_emitter()), 64, 64,
                  dict(num_bounces=4, delta_lights=1, sky_sampling=sky_share), scheduler, sky=1.0)
    try:
        sigma_a, sigma_s, _ = cases.VOLUMES["unequal"]
        r.fog(cases.BOX_MIN, cases.BOX_MAX, sigma_a, sigma_s, SORT_G)
        ctx, sample, frame_pixels = r.pt.ctx, 3, r.pt.pitch * 64
        o, d = _rays_at_the_box(425, 41)
        pixels = np.arange(len(o), dtype=np.uint32)
        entries = _sort_entries(o, d, pixels)
        seg = _segments(grt, ctx, entries, 0, sample)
        got = _sort_launch(grt, ctx, scheduler, entries, 0, sample, frame_pixels)
        n = int((seg[:, 4] == 1).sum())
        assert n > 50 and got.counters[4] == n and got.shadow_count == n   # a light sample at every vertex
        assert np.all(got.trace_out[:n, 10] & FLAG_ALLOW_NEE)
        sh = got.shadow_out[:n]; fs = sh.view(np.float32)
        px = sh[:, 10] & 0x3FFFFFFF
        assert sorted(px.tolist()) == pixels[seg[:, 4] == 1].tolist() and np.array_equal(sh[:, 0:3], seg[px, 9:12])
        vertex = seg[px, 9:12].view(np.float32).astype(np.float64); throughput = seg[px, 6:9].view(np.float32).astype(np.float64)
        u_light = grt.random_samples(ctx, DIM_NEE_LIGHT, px, 0, sample)[:, 0]
        u_sky = grt.random_samples(ctx, DIM_NEE_TRIANGLE, px, 0, sample)
        to_sky = sky_share > 0 and u_light < np.float32(sky_share)
        to_sky = np.broadcast_to(to_sky, (n,))
        sky = grt.sample_sky_distribution(ctx, u_sky).astype(np.float64) if sky_share > 0 else np.zeros((n, 4))
        away = light[None, :] - vertex; distance = np.linalg.norm(away, axis=1); away /= distance[:, None]
        direction = np.where(to_sky[:, None], sky[:, 0:3], away)
        phase = ref.hg(np.einsum("ij,ij->i", -d[px].astype(np.float64), direction), SORT_G)
        light_pdf = np.float64(np.float32(sky_share)) * sky[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            want_sky = phase * 1.0 * (light_pdf ** 2 / (light_pdf ** 2 + phase ** 2)) / light_pdf
        want_light = phase * I / distance ** 2 / np.float64(np.float32(1.0) - np.float32(sky_share))
        want = throughput * np.where(to_sky, want_sky, want_light)[:, None]
        # the direction to the light: a difference, a length and a quotient (4 EPS per component); HG of it (HG_ERROR); I / r^2 and the products and quotients
        # of nee_finish, 10 roundings; the power heuristic 6 more on the sky's side
        bound = HG_ERROR + 24 * EPS
        error = np.abs(fs[:, 7:10] - want) / want
        assert error.max() <= bound, (error.max(), bound)
        assert np.abs(fs[:, 3:6] - direction).max() <= 8 * EPS
        assert np.all(np.isinf(fs[to_sky, 6])) and np.all(np.abs(fs[~to_sky, 6] - distance[~to_sky]) <= 4 * EPS * distance[~to_sky])
        print("%s, sky share %g: %d vertices, %d light samples to the sky; illumination error %.3f of its bound" % (scheduler, sky_share, n, to_sky.sum(), error.max() / bound))
        assert (to_sky.sum() > 10 and (~to_sky).sum() > 10) if sky_share > 0 else not to_sky.any()
    finally:
        r.close()


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_sort_launch_with_nothing_to_sample(grt, tmp_path, scheduler):
    """No emitter, no delta light, no sky sampling: a vertex has no light sample -- no shadow ray, no RT_FLAG_ALLOW_NEE on the ray that goes on (a sky miss after it
    is then added whole) -- and still its vertex, throughput and HG pdf."""
    r = Rendering(grt, cases.write_empty_scene(tmp_path, "sort_nothing"), 64, 64, dict(num_bounces=4), scheduler, sky=1.0)
    try:
        sigma_a, sigma_s, _ = cases.VOLUMES["unequal"]
        r.fog(cases.BOX_MIN, cases.BOX_MAX, sigma_a, sigma_s, SORT_G)
        o, d = _rays_at_the_box(300, 43)
        entries = _sort_entries(o, d, np.arange(len(o)))
        seg = _segments(grt, r.pt.ctx, entries, 0, 2)
        got = _sort_launch(grt, r.pt.ctx, scheduler, entries, 0, 2, r.pt.pitch * 64)
        n = int((seg[:, 4] == 1).sum())
        assert n > 50 and got.counters[4] == n and got.shadow_count == 0 and np.all(got.shadow_out == SENTINEL)
        assert not np.any(got.trace_out[:n, 10] & (FLAG_ALLOW_NEE | FLAG_INSIDE_MEDIUM))
        px = got.trace_out[:n, 10]
        assert np.array_equal(got.trace_out[:n, 0:3], seg[px, 9:12]) and np.array_equal(got.trace_out[:n, 11:14], seg[px, 6:9])
        fo = got.trace_out.view(np.float32)
        pdf = ref.hg(np.einsum("ij,ij->i", -d[px].astype(np.float64), fo[:n, 3:6].astype(np.float64)), SORT_G)
        assert (np.abs(fo[:n, 14] - pdf) / pdf).max() <= HG_ERROR
        # the entries that did not scatter: the sky (radiance 1) through the fog, written at bounce 0
        missed = np.nonzero(seg[:, 4] == 0)[0]
        assert np.array_equal(got.aov[0][missed, 0:3].view(np.uint32), seg[missed, 6:9])   # throughput' x 1, bit for bit
        print("%s: %d vertices without a light sample, %d misses carry their transmittance" % (scheduler, n, len(missed)))
    finally:
        r.close()


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_sort_launch_weighs_a_sky_miss_after_a_scatter(grt, tmp_path, scheduler):
    """Bounce 1, entries as a scatter vertex leaves them (RT_FLAG_ALLOW_NEE, last_pdf = an HG pdf), under a sky share of 0.25 beside a point light: a ray that
    leaves without scattering adds throughput' x sky x power_heuristic(last_pdf, share x p_sky) -- the AOV sums against float64; one that scatters adds nothing."""
    share = 0.25
    r = Rendering(grt, cases.write_empty_scene(tmp_path, "sort_miss", emitter_xml=cases.shaft_emitter()), 64, 64,
                  dict(num_bounces=4, delta_lights=1, sky_sampling=share, enable_russian_roulette=0), scheduler, sky=1.0)
    try:
        sigma_a, sigma_s, _ = cases.VOLUMES["unequal"]
        r.fog(cases.BOX_MIN, cases.BOX_MAX, sigma_a, sigma_s, SORT_G)
        ctx = r.pt.ctx
        o, d = _rays_at_the_box(300, 47)
        n = len(o)
        rng = np.random.default_rng(5)
        last_pdf = ref.hg(rng.uniform(-1, 1, n), SORT_G).astype(np.float32)
        throughput = rng.uniform(0.1, 1.0, (n, 3)).astype(np.float32)
        entries = _sort_entries(o, d, np.arange(n), flags=FLAG_ALLOW_NEE, throughput=throughput, last_pdf=last_pdf)
        seg = _segments(grt, ctx, entries, 1, 4)
        got = _sort_launch(grt, ctx, scheduler, entries, 1, 4, r.pt.pitch * 64)
        missed = seg[:, 4] == 0
        p_sky = np.float64(np.float32(share)) * grt.sky_pdf(ctx, d).astype(np.float64)
        lp = last_pdf.astype(np.float64)
        want = seg[:, 6:9].view(np.float32).astype(np.float64) * (lp ** 2 / (lp ** 2 + p_sky ** 2))[:, None]
        radiance = got.aov[0][:n, 0:3].astype(np.float64)
        assert not radiance[~missed].any()
        error = np.abs(radiance[missed] - want[missed]) / want[missed]
        assert error.max() <= 10 * EPS, error.max()   # share x p_sky, two squares, a sum, a quotient, the sky's texel and two products
        assert got.counters[4] == (~missed).sum()
        print("%s: %d weighed sky misses (weights %.3f .. %.3f), worst error %.2f EPS; %d scattered again" %
              (scheduler, missed.sum(), (lp ** 2 / (lp ** 2 + p_sky ** 2))[missed].min(), (lp ** 2 / (lp ** 2 + p_sky ** 2))[missed].max(), error.max() / EPS, (~missed).sum()))
        assert missed.sum() > 50
    finally:
        r.close()


ROOM_FOG = ((-0.8, 0.2, -0.6), (0.8, 1.8, 0.9), (0.3, 0.2, 0.1), (0.9, 0.7, 0.5), SORT_G)   # inside the Cornell box's room, clear of its walls and its light
CORNELL_EMISSION = np.array([17.0, 12.0, 4.0])


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_sort_launch_surfaces_and_emitters_behind_the_fog(grt, probing, scheduler):
    """Real hits of the Cornell box behind the fog (the rays traced by rt_trace_rays). Bounce 0: a surface hit's material record carries the segment's throughput
    bit for bit (the material kernels read it while the volume is active). Bounce 2, Russian roulette on: every path that goes on -- from a vertex or to a material
    queue -- survived with probability max(throughput') and carries throughput' / it, bit for bit in float32; the others are gone. Bounce 1, rays at the ceiling
    light with RT_FLAG_ALLOW_NEE and an HG last_pdf: throughput' x emission x power_heuristic(last_pdf, light pdf) against float64."""
    ctx, frame_pixels = probing.pt.ctx, probing.pt.pitch * 64
    probing.fog(*ROOM_FOG)
    rng = np.random.default_rng(61)
    n = 600
    o = np.tile(np.array([0.0, 1.0, 3.0], np.float32), (n, 1))
    target = np.stack([rng.uniform(-0.95, 0.95, n), rng.uniform(0.05, 1.9, n), np.full(n, -0.9)], axis=1)
    d = (target - o); d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    hits, _ = grt.trace_rays(ctx, o.T.copy(), d.T.copy())
    assert np.all(hits[:, 1] != 0xFFFFFFFF)
    pixels = np.arange(n, dtype=np.uint32)
    # bounce 0
    entries = _sort_entries(o, d, pixels, hits=hits)
    seg = _segments(grt, ctx, entries, 0, 1)
    got = _sort_launch(grt, ctx, scheduler, entries, 0, 1, frame_pixels)
    records = 0
    for m in range(4):
        q = got.material_out[m][:got.counters[m]]
        px = q[:, 7] & 0x3FFFFFFF
        assert np.all(seg[px, 4] == 0) and np.array_equal(q[:, 8:11], seg[px, 6:9]) and np.array_equal(q[:, 3:7], hits[px])
        assert np.all(np.any(q[:, 8:11].view(np.float32) != 1.0, axis=1))   # every one of these rays crosses the fog (the spectral weight may exceed 1 in the thinnest channel)
        records += len(q)
    assert records > 100 and got.counters[4] == (seg[:, 4] == 1).sum()
    # bounce 2: Russian roulette
    throughput = rng.uniform(0.05, 0.9, (n, 3)).astype(np.float32)
    entries = _sort_entries(o, d, pixels, hits=hits, flags=FLAG_ALLOW_NEE, throughput=throughput, last_pdf=0.1)
    seg = _segments(grt, ctx, entries, 2, 1)
    got = _sort_launch(grt, ctx, scheduler, entries, 2, 1, frame_pixels)
    after = seg[:, 6:9].view(np.float32)
    survival = np.clip(after.max(axis=1), 0.0, 1.0).astype(np.float32)
    u = grt.random_samples(ctx, DIM_RUSSIAN_ROULETTE, pixels, 2, 1)[:, 0]
    lives = ~(u > survival)
    carried = (after / survival[:, None]).astype(np.float32)
    seen = np.zeros(n, bool)
    queues = [got.trace_out[:got.counters[4]][:, [10, 11, 12, 13]]] + [got.material_out[m][:got.counters[m]][:, [7, 8, 9, 10]] for m in range(4)]
    for q in queues:
        px = q[:, 0] & 0x3FFFFFFF
        assert np.all(lives[px]) and np.array_equal(q[:, 1:4], carried[px].view(np.uint32))
        seen[px] = True
    light_hit = ~seen & lives & (seg[:, 4] == 0)   # what lives, did not scatter and is in no queue hit the light (sorted out before the roulette)
    assert (~lives).sum() > 20 and seen.sum() > 100 and light_hit.sum() < n // 10, ((~lives).sum(), seen.sum(), light_hit.sum())
    # bounce 1: the ceiling light, found by a ray that left a scatter vertex
    k = 200
    o1 = np.stack([rng.uniform(-0.6, 0.6, k), rng.uniform(0.3, 1.0, k), rng.uniform(-0.5, 0.7, k)], axis=1).astype(np.float32)
    target = np.stack([rng.uniform(-0.2, 0.2, k), np.full(k, 1.98), rng.uniform(-0.18, 0.12, k)], axis=1)
    d1 = target - o1; d1 = (d1 / np.linalg.norm(d1, axis=1)[:, None]).astype(np.float32)
    hits1, _ = grt.trace_rays(ctx, o1.T.copy(), d1.T.copy())
    last_pdf = ref.hg(rng.uniform(-1, 1, k), SORT_G).astype(np.float32)
    throughput = rng.uniform(0.1, 1.0, (k, 3)).astype(np.float32)
    entries = _sort_entries(o1, d1, np.arange(k), hits=hits1, flags=FLAG_ALLOW_NEE, throughput=throughput, last_pdf=last_pdf)
    seg = _segments(grt, ctx, entries, 1, 1)
    got = _sort_launch(grt, ctx, scheduler, entries, 1, 1, frame_pixels)
    t = hits1[:, 2].view(np.float32).astype(np.float64)
    power = 0.299 * 17.0 + 0.587 * 12.0 + 0.114 * 4.0
    light_pdf = power * t * t / (np.abs(d1[:, 1].astype(np.float64)) * probing.pt.lights_total_weight)
    lp = last_pdf.astype(np.float64)
    want = seg[:, 6:9].view(np.float32).astype(np.float64) * CORNELL_EMISSION[None, :] * (lp ** 2 / (lp ** 2 + light_pdf ** 2))[:, None]
    radiance = got.aov[0][:k, 0:3].astype(np.float64)
    emitter = (seg[:, 4] == 0) & (radiance.sum(axis=1) > 0)
    assert emitter.sum() > 50 and not radiance[seg[:, 4] == 1].any()
    error = np.abs(radiance[emitter] - want[emitter]) / want[emitter]
    # the light's pdf: luminance (3 roundings), t^2 (1), the cosine against the normalised normal (3), a product and a quotient (2): 9, taken as 10 EPS; its
    # square 21, which the heuristic passes on at most whole, with 3 roundings of its own; three products with throughput and emission: 32 EPS
    assert error.max() <= 32 * EPS, error.max()
    print("%s: %d material records behind the fog; roulette: %d ended, %d go on; %d emitter hits weighed, worst error %.1f EPS" %
          (scheduler, records, (~lives).sum(), seen.sum(), emitter.sum(), error.max() / EPS))


ROOM_LIGHT = ((0.3, 1.5, 0.4), (3.0, 2.5, 2.0))   # a point light inside the Cornell box's room: position, intensity


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_sort_launch_splits_its_light_samples_three_ways(grt, scheduler):
    """The Cornell box (a real triangle emitter) with a point light in the room and a sky share of 0.25: 0 < taken < 1. Bounce 0, real hits behind the fog: every
    vertex's light sample -- to the sky, to the point light, or, with DIM_NEE_LIGHT.x rescaled and the pdf times 1 - taken, to the emitter -- against float64.
    Bounce 1: the emitter found by a ray that left a vertex is weighed against the light's pdf times 1 - taken."""
    sky_share = 0.25
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=4, sky_sampling=sky_share), scheduler)
    try:
        r.scene.add_point_light(*ROOM_LIGHT)
        r.pt.invalidate("delta_lights"); r.pt.update()
        texel = np.array([1.0, 1.0, 1.0, 1.0], np.float32)
        assert r.lib.rt_set_sky(r.pt.ctx, texel.ctypes.data, 1, 1, 1.0) == 0
        r.fog(*ROOM_FOG)
        ctx, frame_pixels = r.pt.ctx, r.pt.pitch * 64
        shares = SplitShares(sky_share, r.pt.delta_light_share)
        assert 0.3 < shares.taken < 0.99 and shares.q > 0.04, (shares.s, shares.q, shares.taken)
        rng = np.random.default_rng(67)
        n = 900
        o = np.tile(np.array([0.0, 1.0, 3.0], np.float32), (n, 1))
        target = np.stack([rng.uniform(-0.95, 0.95, n), rng.uniform(0.05, 1.9, n), np.full(n, -0.9)], axis=1)
        d = (target - o); d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
        hits, _ = grt.trace_rays(ctx, o.T.copy(), d.T.copy())
        entries = _sort_entries(o, d, np.arange(n), hits=hits)
        seg = _segments(grt, ctx, entries, 0, 6)
        got = _sort_launch(grt, ctx, scheduler, entries, 0, 6, frame_pixels)
        scattered = np.nonzero(seg[:, 4] == 1)[0]
        assert got.counters[4] == len(scattered) and np.all(got.trace_out[:len(scattered), 10] & FLAG_ALLOW_NEE)
        kinds, worst = _check_light_samples(grt, r.pt, got.shadow_out[:got.shadow_count], scattered, seg, d, 0, 6, shares, ROOM_LIGHT)
        assert min(kinds) > 15, kinds
        # bounce 1: the ceiling light after a scatter
        k = 200
        o1 = np.stack([rng.uniform(-0.6, 0.6, k), rng.uniform(0.3, 1.0, k), rng.uniform(-0.5, 0.7, k)], axis=1).astype(np.float32)
        target = np.stack([rng.uniform(-0.2, 0.2, k), np.full(k, 1.98), rng.uniform(-0.18, 0.12, k)], axis=1)
        d1 = target - o1; d1 = (d1 / np.linalg.norm(d1, axis=1)[:, None]).astype(np.float32)
        hits1, _ = grt.trace_rays(ctx, o1.T.copy(), d1.T.copy())
        last_pdf = ref.hg(rng.uniform(-1, 1, k), SORT_G).astype(np.float32)
        throughput = rng.uniform(0.1, 1.0, (k, 3)).astype(np.float32)
        entries = _sort_entries(o1, d1, np.arange(k), hits=hits1, flags=FLAG_ALLOW_NEE, throughput=throughput, last_pdf=last_pdf)
        seg = _segments(grt, ctx, entries, 1, 6)
        got = _sort_launch(grt, ctx, scheduler, entries, 1, 6, frame_pixels)
        t = hits1[:, 2].view(np.float32).astype(np.float64)
        power = 0.299 * 17.0 + 0.587 * 12.0 + 0.114 * 4.0
        light_pdf = power * t * t / (np.abs(d1[:, 1].astype(np.float64)) * r.pt.lights_total_weight) * np.float64(np.float32(1.0) - shares.taken)
        lp = last_pdf.astype(np.float64)
        want = seg[:, 6:9].view(np.float32).astype(np.float64) * CORNELL_EMISSION[None, :] * (lp ** 2 / (lp ** 2 + light_pdf ** 2))[:, None]
        radiance = got.aov[0][:k, 0:3].astype(np.float64)
        emitter = (seg[:, 4] == 0) & (radiance.sum(axis=1) > 0)
        assert emitter.sum() > 50
        error = np.abs(radiance[emitter] - want[emitter]) / want[emitter]
        assert error.max() <= 34 * EPS, error.max()   # (as with taken = 0, and the factor 1 - taken: two roundings in the pdf's square)
        print("%s: taken %.4f (sky %.2f, point light %.4f); light samples to sky / point light / emitter %s, worst %.3f of its bound; %d emitter hits after a scatter, worst %.1f EPS" %
              (scheduler, shares.taken, shares.s, shares.q, kinds, worst, emitter.sum(), error.max() / EPS))
    finally:
        r.close()


# ---- 3. the attenuation pass ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_attenuation_pass(grt, probing, scheduler):
    sigma_a, sigma_s, g = cases.VOLUMES["unequal"]
    probing.fog(cases.BOX_MIN, cases.BOX_MAX, sigma_a, sigma_s, g)
    grt.set_scheduler(probing.pt.ctx, scheduler)
    try:
        st32 = np.array(sigma_a, np.float32).astype(np.float64) + np.array(sigma_s, np.float32).astype(np.float64)
        for count in (0, 1, 63, 64, 65, 1000):
            q = cases.shadow_queue(count, seed=100 + count)
            out = grt.attenuate_shadow_rays(probing.pt.ctx, q)
            assert out.shape == q.shape
            keep = [0, 1, 2, 3, 4, 5, 6, 10]
            assert np.array_equal(out[:, keep], q[:, keep]), (scheduler, count)   # every other word: bit for bit
            f, fo = q.view(np.float32), out.view(np.float32)
            crossing = infinite = untouched = 0; worst = 0.0
            for i in range(count):
                o, d, md = f[i, 0:3], f[i, 3:6], f[i, 6]
                c = ref.clip(cases.BOX_MIN, cases.BOX_MAX, o, d, md)
                faces = _face_distances(o, d)
                t_error = FACE * max(faces) if faces else 0.0
                L = 0.0 if c is None else c[1] - c[0]
                L_error = 2.0 * t_error + EPS * L
                x = st32 * L
                want = f[i, 7:10].astype(np.float64) * np.exp(-x)
                # exp(-x): x = sigma_t (a rounded sum) * L (its error above), a rounded product; expf 1 ulp; the product with the illumination one rounding
                bound = 3.0 * EPS + st32 * L_error + x * 2.0 * EPS
                assert np.all(np.abs(fo[i, 7:10] - want) <= bound * want), (scheduler, count, i, fo[i, 7:10], want, bound)
                if L > 1e-3:
                    crossing += 1; infinite += int(np.isinf(md))
                    worst = max(worst, float((np.abs(fo[i, 7:10] - want) / (bound * want)).max()))
                    assert np.all(fo[i, 7:10] < f[i, 7:10]), (scheduler, count, i)   # (sigma_t L >= 2.5e-4 in every channel: below 1 in float32)
                elif c is None:
                    untouched += 1
                    assert np.array_equal(out[i], q[i]), (scheduler, count, i)   # a ray outside the box is not stored
            print("%s, %d rays: %d cross the box (%d of them to infinity), %d outside it, worst error %.3f of its bound" % (scheduler, count, crossing, infinite, untouched, worst))
            if count >= 63:
                assert crossing > count // 4 and infinite > 3 and untouched > 3
    finally:
        grt.set_scheduler(probing.pt.ctx, "merged")


# ---- 4. identities ------------------------------------------------------------------------------------------------------------

def _cornell(grt, scheduler, prepare=None, samples=(2, 3)):
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=4), scheduler)
    try:
        if prepare:
            prepare(r)
        first, frame = 0, None
        for count in samples:
            frame = r.render(count, first, batch=count); first += count
        c = r.pt.counters()
        return frame, [list(c.trace[:4]), list(c.shadow[:4]), list(c.diffuse[:4])]
    finally:
        r.close()


FOG_IN_ROOM = ((-0.5, 0.3, -0.5), (0.5, 1.5, 0.5), 0.2, 0.8, 0.3)   # inside the Cornell box's room (about [-1, 1] x [0, 2] x [-1, 1])


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_identities(grt, scheduler):
    never, never_counters = _cornell(grt, scheduler)
    far, far_counters = _cornell(grt, scheduler, lambda r: r.fog((100, 100, 100), (101, 101, 101), 0.5, 0.5, 0.2))
    assert np.array_equal(never, far) and never_counters == far_counters, scheduler   # a box no ray reaches (the ..._fog instances run)
    empty, empty_counters = _cornell(grt, scheduler, lambda r: r.fog(*FOG_IN_ROOM[:2], 0.0, 0.0, 0.5))
    assert np.array_equal(never, empty) and never_counters == empty_counters, scheduler   # zero density: stored, renders as none

    def on_then_off(r):
        r.fog(*FOG_IN_ROOM)
        on_then_off.lit = r.render(2)
        assert r.grt.get_fog_volume(r.pt.ctx) is not None
        assert r.grt.set_fog_volume(r.pt.ctx, None) == 0
        assert r.grt.get_fog_volume(r.pt.ctx) is None
    again, again_counters = _cornell(grt, scheduler, on_then_off)
    assert np.array_equal(never, again) and never_counters == again_counters, scheduler
    assert np.isfinite(on_then_off.lit).all() and not np.array_equal(never, on_then_off.lit)   # ... and the fog does change the picture
    print("%s: far box, zero density and set-then-cleared equal the frame without a volume; with the volume the mean goes %.4f -> %.4f" %
          (scheduler, never[..., :3].mean(), on_then_off.lit[..., :3].mean()))


def test_never_set_is_the_oracle(grt, oracle):
    """With no volume ever set the frame is what it was before the fog existed: the queue sizes of the CPU oracle exactly, its image within 1e-3."""
    grt.config_reset()
    scene = grt.Scene(grt.scene_path("cornellbox"))
    grt.config_set(num_bounces=4)
    pt = grt.Pathtracer(scene, 64, 64, device=0)
    try:
        pt.update()
        assert grt.get_fog_volume(pt.ctx) is None
        frame = oracle.Frame(oracle.SceneView(pt))
        pt.render()
        c = pt.counters()
        oc = frame.render_sample(pt.sample_index)
        assert list(c.trace[:4]) == list(oc.trace[:4]) and list(c.shadow[:4]) == list(oc.shadow[:4])
        got = pt.read_framebuffer()[:, :64, :3]; want = frame.final[:, :64, :3]
        rel = float(np.abs(got - want).sum() / want.sum())
        print("never set: rays per bounce %s, relative L1 against the oracle %.3g" % (list(c.trace[:4]), rel))
        assert rel < 1e-3
    finally:
        pt.close(); scene.close(); grt.config_reset()


# ---- 5. frames against closed forms ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_absorption_only_dims_the_emitter_by_beer_lambert(grt, scheduler):
    """The Cornell box's ceiling light seen through an absorbing box that hangs in the line of sight, one sample of paths one segment long: a pixel that shows
    the emitter shows its radiance times exp(-sigma_a x clipped length), the length from the pixel's own primary ray (rt_generate_rays) clipped in
    float64 -- the POSITION AOV the issue names is not written on an emitter hit. Deterministic."""
    sigma_a = np.array([0.9, 0.4, 0.1], np.float32)
    # the camera stands at (0, 1, 6.8) outside the room, the light hangs at y = 1.98 around x = 0, z = 0: the rays between them enter this box through its front and leave through its top
    box_min, box_max = np.array([-0.5, 1.3, 2.0], np.float32), np.array([0.5, 1.62, 4.0], np.float32)
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=1), scheduler, sky=0.0)
    try:
        o, d, px = grt.generate_rays(r.pt.ctx, 0, 0, 64 * 64)
        clear = r.render(1, 0, 1)[..., :3].astype(np.float64)
        r.fog(box_min, box_max, sigma_a, 0.0)
        dimmed = r.render(1, 0, 1)[..., :3].astype(np.float64)
        lit = clear.sum(axis=2) > 0
        assert lit.sum() > 20, lit.sum()
        # rt_generate_rays gives the rays the render traced: traced on their own, exactly the rays of the lit pixels end on one instance (the light), jitter and all
        hits, _ = grt.trace_rays(r.pt.ctx, o, d)
        lit_rays = lit[px // r.pt.pitch, px % r.pt.pitch]
        light_instance = set(hits[lit_rays, 0].tolist())
        assert len(light_instance) == 1 and not np.any(hits[~lit_rays, 0] == light_instance.pop())
        through = 0; worst = 0.0
        for i in range(64 * 64):
            x, y = int(px[i]) % r.pt.pitch, int(px[i]) // r.pt.pitch
            if not lit[y, x]:
                assert not dimmed[y, x].any()
                continue
            oi, di = o[:, i], d[:, i]
            c = ref.clip(box_min, box_max, oi, di, np.inf)
            faces = [abs((float(b[k]) - float(oi[k])) / float(di[k])) for b in (box_min, box_max) for k in range(3) if di[k] != 0]
            L = 0.0 if c is None else c[1] - c[0]
            L_error = 2.0 * FACE * max(faces) + EPS * L
            xs = sigma_a.astype(np.float64) * L
            want = clear[y, x] * np.exp(-xs)
            bound = 4.0 * EPS + sigma_a * L_error + xs * 2.0 * EPS   # as in the attenuation pass, and one rounding for the frame's fold
            assert np.all(np.abs(dimmed[y, x] - want) <= bound * want), (scheduler, x, y, dimmed[y, x], want)
            if L > 0:
                through += 1; worst = max(worst, float((np.abs(dimmed[y, x] - want) / (bound * want)).max()))
        print("%s: %d pixels show the emitter, %d of them through the box; worst error %.3f of its bound" % (scheduler, lit.sum(), through, worst))
        assert through > 10
    finally:
        r.close()




@pytest.mark.parametrize("g", [0.0, 0.8, -0.8])
def test_white_furnace(grt, tmp_path, g):
    """A sky of radiance 1, a grey volume without absorption, NEE off: every sample is 1 unless the bounce limit cuts its path; the shortfall allowed is the
    truncation probability the restatement bounds, and float32 rounding, derived here for THIS volume (tighter than the general bound of the segment test):
    * a segment's weight. With sigma_a = 0 and a grey throughput (a, a, a) the transmittance T is one float that stands in numerator and denominator alike, so
      its own error cancels. wpdf = a / ((a + a) + a): the first sum is exact, 2 roundings. A channel's pdf wpdf x sigma_t x T: 2 more (sigma_t = 0 + sigma_s is
      exact). Their sum (p + p) + p: 1. Numerator sigma_s x T, the quotient, the product with the throughput: 3. At most 8 EPS, scattered or not;
    * a path has at most FURNACE_BOUNCES + 1 segments: a sample is within 8 EPS x 27 of 1. The mean over the frame's samples is within 8 EPS x the mean number
      of segments per path, which the launch counters give: rays traced / paths;
    * the fold of a sample into the pixel's mean, next = acc + (sample - acc) / n (accumulate_fold). Both lie within 2^-15 of 1, so the difference is exact
      (Sterbenz) and its quotient tiny; what rounds is the sum: at most EPS on a value next to 1. A later fold multiplies what the mean carried by 1 - 1 / n:
      the error of fold j of N reaches the end with weight at most j / N. Together at most EPS (N / 2 + 1)."""
    truncation = ref.furnace_truncation_bound(cases.BOX_MIN, cases.BOX_MAX, FURNACE_SIGMA, FURNACE_BOUNCES)
    assert truncation < 1e-6
    samples = 64
    fold = EPS * (samples / 2 + 1)
    rounding = (FURNACE_BOUNCES + 1) * 8.0 * EPS + fold
    for scheduler in ("merged", "slots"):
        r = Rendering(grt, cases.write_empty_scene(tmp_path), 16, 16, dict(num_bounces=FURNACE_BOUNCES, enable_next_event_estimation=0, enable_russian_roulette=0), scheduler, sky=1.0)
        try:
            r.fog(cases.BOX_MIN, cases.BOX_MAX, 0.0, FURNACE_SIGMA, g)
            rays = paths = scatters = 0
            for first in range(0, samples, 16):
                frame = r.render(16, first)[..., :3].astype(np.float64)
                c = r.pt.counters()   # (of this submission)
                rays += sum(c.trace[:FURNACE_BOUNCES]); paths += c.trace[0]; scatters += c.trace[1]
            assert paths == 16 * 16 * samples
            mean_rounding = 8.0 * EPS * rays / paths + fold
            print("g = %g, %s: pixel means in [%.9f, %.9f], frame mean %.9f; %.3f segments per path; allowed: truncation %.3g, rounding %.3g per pixel and %.3g in the mean" %
                  (g, scheduler, frame.min(), frame.max(), frame.mean(), rays / paths, truncation, rounding, mean_rounding))
            assert frame.max() <= 1.0 + rounding   # (a truncated sample would show as a pixel at 1 - 1/64 and in the mean below)
            assert abs(frame.mean() - 1.0) <= mean_rounding + truncation
            assert scatters > 0   # paths did scatter
        finally:
            r.close()


@pytest.mark.parametrize("g", [0.0, 0.8])
def test_white_furnace_with_light_samples(grt, tmp_path, g):
    """The furnace with NEE, MIS and a sky share of 0.5 (the other half of the light samples goes to an emitter of radiance 1e-6 that subtends 4e-12 sr):
    the light samples of the scatter vertices and the weighed misses after them add up to 1. The frame's mean lies within 5 standard errors of 1, the
    standard error from the variance of the float64 Monte Carlo of the same estimator over the same number of samples."""
    w = h = 16; samples = 256
    r = Rendering(grt, cases.write_empty_scene(tmp_path, "furnace_nee", speck_emits=True), w, h,
                  dict(num_bounces=FURNACE_BOUNCES, enable_russian_roulette=0, reconstruction_filter=0, sky_sampling=0.5), "merged", sky=1.0)
    try:
        r.fog(cases.BOX_MIN, cases.BOX_MAX, 0.0, FURNACE_SIGMA, g)
        frame = r.render(samples)[..., :3].astype(np.float64)
        shadows = r.pt.counters().shadow[0]
        share = __import__("ctypes").c_float()
        camera = r.camera()
        rng = np.random.default_rng(23)
        n = w * h * samples
        dirs = ref.pixel_rays(camera, w, h, rng.random((n, 2)), repeat=samples)
        v = ref.furnace(cases.BOX_MIN, cases.BOX_MAX, FURNACE_SIGMA, g, FURNACE_BOUNCES, np.broadcast_to(camera["position"], dirs.shape), dirs, rng, nee=True, sky_share=0.5)
        error = v.std(ddof=1) / math.sqrt(n)
        print("g = %g: frame mean %.6f (reference Monte Carlo %.6f), standard error %.6f, %d shadow rays at bounce 0" % (g, frame.mean(), v.mean(), error, shadows))
        assert shadows > 0
        assert abs(v.mean() - 1.0) < 5 * error
        assert abs(frame.mean() - 1.0) < 5 * error
    finally:
        r.close()




def test_light_shaft_matches_the_single_scatter_integral(grt, tmp_path):
    """One point light above the box, a black sky, paths of exactly one scattering event (num_bounces 2), a box filter: each pixel's mean lies within 5
    standard errors of the quadrature of sigma_s T p I / r^2 T over its rays (a 2 x 2 grid of its footprint), the standard error from the float64 Monte
    Carlo of the same estimator -- not from the device's moments."""
    w = h = 16
    r = Rendering(grt, cases.write_empty_scene(tmp_path, "shaft", emitter_xml=cases.shaft_emitter()), w, h,
                  dict(num_bounces=2, reconstruction_filter=0, delta_lights=1), "merged", sky=0.0)
    try:
        assert r.scene.delta_lights().shape[0] == 1
        r.fog(cases.BOX_MIN, cases.BOX_MAX, SHAFT["sigma_a"], SHAFT["sigma_s"], SHAFT["g"])
        frame = r.render(SHAFT["samples"])[..., 0].astype(np.float64)
        camera = r.camera()
        want, error = _shaft_reference(camera, w, h)
        deviation = np.abs(frame - want) / error
        print("shaft: radiance %.4g .. %.4g, standard error %.3g .. %.3g, worst deviation %.2f standard errors, mean %.2f" %
              (want.min(), want.max(), error.min(), error.max(), deviation.max(), deviation.mean()))
        assert want.min() > 0
        # The margin is thin and known: on the MI355X the worst pixel lies at 4.04 standard errors and the mean deviation is 1.09 (0.80 for an ideal sequence). The
        # distance numbers are hash_with over consecutive sample indices, as prescribed, and over a pixel's 4 096 samples their mean lies 1.4 standard errors
        # (rms; 4.6 worst of 200 pixels) from 1/2 (known limits). Samples and hash are deterministic, so the figure does not move from run to run;
        # another frame size, sample count or volume draws other hash values and may come closer to 5 with no bug present.
        assert (deviation > 5.0).sum() == 0, np.argwhere(deviation > 5.0)   # (256 pixels at 5 sigma: 1.5e-4 expected failures)
    finally:
        r.close()


def _shaft_reference(camera, w, h, seed=7):
    """Per pixel: the quadrature averaged over a 2 x 2 grid of the footprint, and the standard error of SHAFT['samples'] samples of the estimator."""
    a = dict(box_min=cases.BOX_MIN, box_max=cases.BOX_MAX, sigma_a=SHAFT["sigma_a"], sigma_s=SHAFT["sigma_s"], g=SHAFT["g"], light=cases.SHAFT_LIGHT, intensity=cases.SHAFT_INTENSITY)
    want = np.zeros(w * h)
    grid = [0.25, 0.75]
    for jx in grid:
        for jy in grid:
            dirs = ref.pixel_rays(camera, w, h, (jx, jy))
            want += np.array([ref.shaft_quadrature(o=camera["position"], d=dirs[k], **a) for k in range(w * h)]) / 4.0
    rng = np.random.default_rng(seed)
    n = 1024
    dirs = ref.pixel_rays(camera, w, h, rng.random((n * w * h, 2)), repeat=n)
    values = ref.shaft_monte_carlo(o=np.broadcast_to(camera["position"], dirs.shape), d=dirs, rng=rng, **a).reshape(n, w * h)
    error = values.std(axis=0, ddof=1) / math.sqrt(SHAFT["samples"])
    return want.reshape(h, w), error.reshape(h, w)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals(grt, probing):
    lib, ctx = _lib(grt), probing.pt.ctx
    good = grt.fog_volume_record(cases.BOX_MIN, cases.BOX_MAX, (0.1, 0.2, 0.3), 0.4, 0.5)
    assert grt.set_fog_volume(ctx, good) == 0
    bad = []
    for word, value in [(0, np.nan), (4, np.inf), (3, -1.0), (1, 1.5), (5, 2.0), (6, -0.1), (7, np.nan), (9, np.inf), (11, -1e-9), (12, 1.0), (12, -1.0), (12, np.nan)]:
        v = good.copy(); v[word] = value
        bad.append((word, value, v))
    for word, value, v in bad:
        assert grt.set_fog_volume(ctx, v) == RT_ERROR_INVALID_ARG, (word, value)
        assert b"rt_set_fog_volume" in lib.rt_last_error(ctx)
        assert np.array_equal(grt.get_fog_volume(ctx), good), (word, value)   # the volume before it is still in force
    print("refused: %d invalid volumes, each leaving the one before in force" % len(bad))
    # ... and with SVGF
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=3, enable_svgf=1))
    try:
        r.fog(*FOG_IN_ROOM)
        assert r.lib.rt_render_samples(r.pt.ctx, 0, 1) == RT_ERROR_INVALID_ARG
        assert b"fog volume" in r.lib.rt_last_error(r.pt.ctx)
        assert r.grt.set_fog_volume(r.pt.ctx, None) == 0
        assert r.lib.rt_render_samples(r.pt.ctx, 0, 1) == 0
    finally:
        r.close()
