"""The still-image denoiser in numpy, twice from one text: dtype float64 is the reference -- the definition with pow and exp --, dtype float32 the
restatement -- every operation a float32 one in the order kernels_denoise.hip performs it, the weight as one exp2. numpy's float32 +, -, *, /, sqrt are the IEEE
operations the kernels use; its log2 / exp2 differ from the hardware's v_log_f32 / v_exp_f32 (and 1 / x from v_rcp_f32) by an ulp, which is why the device is held
to the restatement within a measured tolerance and not bit for bit.

Images are (height, pitch, 4) float32; only columns < width are read and produced. The functions are pure: no argument is modified."""
import numpy as np

DEFAULTS = {"iterations": 5, "sigma_l": 4.0, "sigma_n": 128.0, "sigma_z": 1.0, "depth_floor": 1e-2, "albedo_floor": 1e-2}
EPSILON = 1e-8
EPS32 = float(np.finfo(np.float32).eps) / 2   # unit roundoff


def params(**given):
    unknown = set(given) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **given)


def luminance(r, g, b, dt):
    return dt(0.299) * r + dt(0.587) * g + dt(0.114) * b


def _finite3(a):
    return np.isfinite(a[..., :3]).all(axis=-1)


def prepare(colour, moments, albedo, normal, position, fallback, eye, width, p, dt):
    """-> iv (H, W, 4) = (I, v), guide (H, W, 4) = (n, z), surface, valid (H, W) bool, alb (H, W, 3). Pixels that are no surface: iv = (C, 0) when valid,
    (fallback.rgb, 0) when not; guide 0."""
    cut = lambda a: np.asarray(a, np.float32)[:, :width]
    c32, m32, a32, n32, p32, f32 = (cut(a) for a in (colour, moments, albedo, normal, position, fallback))
    valid = (m32[..., 3] >= 2) & np.isfinite(m32[..., 3]) & _finite3(c32) & _finite3(m32) & _finite3(a32) & _finite3(n32) & _finite3(p32)
    with np.errstate(all="ignore"):
        c, m, a, n, ps = (x.astype(dt) for x in (c32, m32, a32, n32, p32))
        nn = n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]
        surface = valid & (nn >= dt(0.25))
        alb = np.maximum(a[..., :3], dt(p["albedo_floor"]))
        w = m[..., 3]
        pairs = (w * (w - dt(1)))[..., None]
        var = m[..., :3] / pairs / (alb * alb)
        root = np.sqrt(np.maximum(dt(0), var))
        sd = luminance(root[..., 0], root[..., 1], root[..., 2], dt)
        inv = dt(1) / np.sqrt(nn)
        e = np.asarray(eye, np.float32).astype(dt)
        d = ps[..., :3] - e
        z = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        iv = np.concatenate([c[..., :3] / alb, (sd * sd)[..., None]], axis=-1)
        guide = np.concatenate([n[..., :3] * inv[..., None], z[..., None]], axis=-1)
    plain = np.concatenate([np.where(valid[..., None], c32[..., :3], f32[..., :3]).astype(dt), np.zeros(valid.shape + (1,), dt)], axis=-1)
    iv = np.where(surface[..., None], iv, plain)
    guide = np.where(surface[..., None], guide, dt(0))
    return iv, guide, surface, valid, alb


def _shift(a, dx, dy):
    """out[y, x] = a[y + dy, x + dx] where that lies inside, else 0; and the inside mask."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
        inside[ys, xs] = True
    return out, inside


def near(iv, guide, surface, dt):
    """The 3 x 3 blur of v (clamped neighbours) and the depth gradient (forward to a surface neighbour inside the image, else backward, else 0)."""
    h, w = surface.shape
    padded = np.pad(iv[..., 3], 1, mode="edge")
    vb = np.zeros((h, w), dt)
    for j in range(3):
        for i in range(3):
            vb = vb + padded[j:j + h, i:i + w] * dt((0.5 if i == 1 else 0.25) * (0.5 if j == 1 else 0.25))
    z = guide[..., 3]
    grads = []
    for dx, dy in ((1, 0), (0, 1)):
        zf, inf = _shift(z, dx, dy); sf, _ = _shift(surface, dx, dy)
        zb, inb = _shift(z, -dx, -dy); sb, _ = _shift(surface, -dx, -dy)
        grads.append(np.where(surface & inf & sf, zf - z, np.where(surface & inb & sb, z - zb, dt(0))))
    return vb, grads[0], grads[1]


def one_pass(iv, guide, surface, step, p, dt, want_bound=False):
    """One a-trous pass of `step`. float64: the definition (pow, exp); float32: the kernel's operations in its order. want_bound (float64): also the first-order
    bound on |I'_32 - I'_64| and |v'_32 - v'_64| per pixel for a float32 evaluation of the SAME inputs (see test_denoise.py)."""
    f32 = dt == np.float32
    with np.errstate(all="ignore"):
        vb, gx, gy = near(iv, guide, surface, dt)
        sl, sn, sz = dt(p["sigma_l"]), dt(p["sigma_n"]), dt(p["sigma_z"])
        denom = dt(1) / np.sqrt(sl * sl * np.maximum(dt(0), vb) + dt(EPSILON))
        lum = luminance(iv[..., 0], iv[..., 1], iv[..., 2], dt)
        z = guide[..., 3]
        z_floor = dt(p["depth_floor"]) * z
        sw = np.ones(surface.shape, dt)
        sc = iv.copy()
        if want_bound:
            sum_dw = np.zeros(surface.shape); sum_dw_i = np.zeros(surface.shape + (3,)); sum_dw_v = np.zeros(surface.shape)
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                if i == 0 and j == 0:
                    continue
                t, inside = _shift(iv, i * step, j * step)
                g, _ = _shift(guide, i * step, j * step)
                s, _ = _shift(surface, i * step, j * step)
                tapped = surface & inside & s
                kw = dt((1.0 if i == 0 else 0.5) * (1.0 if j == 0 else 0.5))
                d = gx * dt(i * step) + gy * dt(j * step)
                m = sz * np.maximum(np.abs(d), z_floor) + dt(EPSILON)
                ln_w_z = np.abs(z - g[..., 3]) * (dt(1) / m) if f32 else np.abs(z - g[..., 3]) / m
                ndn = np.maximum(dt(0), guide[..., 0] * g[..., 0] + guide[..., 1] * g[..., 1] + guide[..., 2] * g[..., 2])
                lq = luminance(t[..., 0], t[..., 1], t[..., 2], dt)
                xl = np.abs(lum - lq) * denom
                if f32:
                    log2_w_n = np.where((ndn > 0) | (sn > 0), sn * np.log2(ndn), dt(0))
                    w = kw * np.exp2(log2_w_n - (xl + ln_w_z) * dt(1.44269504088896340736))
                else:
                    w = kw * np.power(ndn, sn) * np.exp(-xl - ln_w_z)
                w = np.where(tapped, w, dt(0)).astype(dt)
                t = np.where(tapped[..., None], t, dt(0))
                sw = sw + w
                sc = sc + np.concatenate([w[..., None] * t[..., :3], ((w * w) * t[..., 3])[..., None]], axis=-1)
                if want_bound:
                    # the float32 weight's distance from w, to first order in the unit roundoff u: exponent E = sn log2(ndn) - (xl + ln_w_z) log2(e), dw = w ln2 dE + 3 u w.
                    #   ndn: three products and two sums of unit vectors' components, 3 u absolute; log2: 1 ulp; the product with sn: u
                    #   xl: the two luminances (3 roundings each on inputs that are the same numbers), their difference, the product; denom's sqrt, sum, division: 4 u
                    #   ln_w_z: d's two products and sum against cancellation, max, product, sum, reciprocal (1 ulp), product: 6 u and u (|gx i s| + |gy j s|) / max(|d|, z_floor)
                    safe = np.maximum(ndn, 1e-300)
                    d_e = EPS32 * (sn * (3 / (safe * np.log(2)) + 3 * np.abs(np.log2(safe)))
                                   + (6 * xl + 3 * (np.abs(lum) + np.abs(lq)) * denom + ln_w_z * (7 + (np.abs(gx * i * step) + np.abs(gy * j * step)) / np.maximum(np.abs(d), np.maximum(z_floor, 1e-300)))) * 1.4427 + 2)
                    dw = np.where(tapped & (ndn > 0), w * (np.log(2) * d_e + 3 * EPS32), 0.0)
                    sum_dw += dw; sum_dw_i += dw[..., None] * np.abs(t[..., :3]); sum_dw_v += 2 * dw * w * np.abs(t[..., 3])
        inv = dt(1) / sw
        out = sc * inv[..., None]
        out[..., 3] = out[..., 3] * inv
    result = np.where(surface[..., None], out, iv).astype(dt)
    if not want_bound:
        return result
    # I' = sum(w I) / sum(w): the weights' errors in numerator and denominator, and the 8 products, 8 sums, reciprocal and product of the evaluation itself (20 u on sums of
    # non-negative weights times |I|)
    absum = (np.abs(sc[..., :3]) + 0) / sw[..., None]
    bound_i = (sum_dw_i + np.abs(out[..., :3]) * sum_dw[..., None]) / sw[..., None] + 20 * EPS32 * np.maximum(absum, np.abs(out[..., :3]))
    bound_v = (sum_dw_v + 2 * np.abs(out[..., 3]) * sw * sum_dw) / (sw * sw) + 24 * EPS32 * np.abs(out[..., 3])
    return result, np.where(surface[..., None], bound_i, 0.0), np.where(surface, bound_v, 0.0)


def finalize(iv, surface, valid, alb, dt):
    out = iv.copy()
    out[..., :3] = np.where(surface[..., None], iv[..., :3] * alb, iv[..., :3])
    out[..., 3] = np.where(surface, iv[..., 3], np.where(valid, dt(0), dt(-1)))
    return out


def denoise(colour, moments, albedo, normal, position, fallback, eye, width=None, dtype=np.float32, states=None, **given):
    """-> (height, width, 4) of dtype: (r, g, b, v). states: a list that receives (iv, guide, surface) before every pass and the last iv."""
    p = params(**given)
    dt = np.float64 if dtype == np.float64 else np.float32
    width = np.asarray(colour).shape[1] if width is None else width
    iv, guide, surface, valid, alb = prepare(colour, moments, albedo, normal, position, fallback, eye, width, p, dt)
    for k in range(int(p["iterations"])):
        if states is not None:
            states.append((iv, guide, surface))
        iv = one_pass(iv, guide, surface, 1 << k, p, dt)
    if states is not None:
        states.append((iv, guide, surface))
    return finalize(iv, surface, valid, alb, dt)
