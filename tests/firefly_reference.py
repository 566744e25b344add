"""The firefly filter in numpy, twice from one text: dtype float64 is the reference, dtype float32 the restatement -- every operation a float32 one
in the order kernels_fireflies.hip performs it. numpy's float32 +, -, *, / are the IEEE operations the kernels use (no contraction, IEEE division), fmin / fmax are
fminf / fmaxf, so the device is held to the restatement bit for bit.

Images are (height, pitch, 4) float32, tiers (K, height, pitch, 4); the functions are pure: no argument is modified.

The rounding bounds (want_bound, float64 only) are first-order in the unit roundoff u = 2^-24 and written out where they are computed. They hold across the branches of the
definition because the definition is continuous there: at L = lo the weight wl is 1, at L = hi it is 0 and the sample falls whole into the tier above; clamp, min and max are
1-Lipschitz."""
import numpy as np

DEFAULTS = {"tiers": 6, "start": 1.0, "support": 4.0}
BASE = 8
U = float(np.finfo(np.float32).eps) / 2   # unit roundoff
LUMA = tuple(float(np.float32(c)) for c in (0.299, 0.587, 0.114))   # luminance() of rt_shading.h: float constants


def luminance(r, g, b, dt):
    return dt(LUMA[0]) * r + dt(LUMA[1]) * g + dt(LUMA[2]) * b


def boundaries(tiers, start):
    """b_j = start * 8^j as the kernels form them: repeated float32 products (exact until they overflow)."""
    b = [np.float32(start)]
    for _ in range(tiers - 1):
        b.append(np.float32(b[-1] * np.float32(BASE)))
    return b


def splat(tiers, sample, reset, start, dt, bound=None):
    """One sample per pixel into `tiers` (K, ..., 4) of dtype dt, IN PLACE (the one exception to purity: the caller owns the array). sample: (..., 4) float32;
    reset: (...) bool, the pixels whose tiers are zeroed first. bound: None, or an array like tiers that accumulates the first-order bound on |tiers32 - tiers64|."""
    count = tiers.shape[0]
    tiers[:, reset] = 0
    if bound is not None:
        bound[:, reset] = 0
    with np.errstate(all="ignore"):
        v = np.concatenate([sample[..., :3].astype(dt), np.ones(sample.shape[:-1] + (1,), dt)], axis=-1)
        lum = luminance(v[..., 0], v[..., 1], v[..., 2], dt)
        finite = np.isfinite(lum)
        lo = np.full(lum.shape, dt(np.float32(start)))
        j = np.zeros(lum.shape, np.int64)
        for _ in range(count - 1):   # the while loop: once its condition fails it keeps failing (lo does not move)
            step = finite & (lum >= lo * dt(BASE)) & (j < count - 1)
            lo = np.where(step, lo * dt(BASE), lo)
            j = j + step
        whole = (j == count - 1) | (lum <= lo)
        hi = lo * dt(BASE)
        wl = np.fmin(np.fmax((lo / lum - lo / hi) / (dt(1) - lo / hi), dt(0)), dt(1))
        lower = np.where(whole, dt(1), wl).astype(dt)
        upper = (dt(1) - wl).astype(dt)
        if bound is not None:
            # L: three products and two sums, |dL| <= 3 u sum(c |x|). wl = (lo / L - 1/8) / (7/8): 1/8 and 7/8 are exact; the quotient lo / L, the difference and the
            # division round once each, and L's own error enters through d(lo / L) / dL = -lo / L^2:   |dwl| <= (lo / L^2 * |dL| + u lo / L + 2 u |lo / L - 1/8|) / (7/8).
            d_lum = 3 * U * (LUMA[0] * np.abs(v[..., 0]) + LUMA[1] * np.abs(v[..., 1]) + LUMA[2] * np.abs(v[..., 2]))
            safe = np.where(finite & (lum > 0), lum, 1.0)
            d_wl = np.where(finite & (lum > 0) & (j < count - 1), (lo / safe ** 2 * d_lum + U * lo / safe + 2 * U * np.abs(lo / safe - 0.125)) / 0.875, 0.0)
        for t in range(count):
            into = finite & (j == t)
            tiers[t][into] = (tiers[t] + lower[..., None] * v)[into]
            above = finite & ~whole & (j + 1 == t)
            tiers[t][above] = (tiers[t] + upper[..., None] * v)[above]
            if bound is not None:
                # one add: the weight's error times |v|, the product's rounding (and that of 1 - wl), the sum's rounding
                touched = finite & ((j == t) | (j + 1 == t))
                weight = np.where(j == t, lower, upper)
                bound[t][touched] = (bound[t] + (d_wl + 2 * U * np.abs(weight))[..., None] * np.abs(v) + U * np.abs(tiers[t]))[touched]
    return tiers


def accumulate(frames, tiers, fold_index, start, dtype=np.float32, pixels=None, want_bound=False):
    """The splats of one accumulate launch. frames: (samples, H, P, 4) float32 in fold order; tiers: (K, H, P, 4) float32, the state before; fold_index: the fold index
    n of the FIRST sample -- a number (the batch and merged forms: the sample index; a list of (first, count) pairs for several submissions) or an (H, P) array (the
    list form: w + 1 per pixel, counted on from there). pixels: (H, P) bool, the pixels the launch covers (None: all). -> tiers after, dtype; with want_bound also the bound."""
    dt = np.float64 if dtype == np.float64 else np.float32
    out = np.array(tiers, dt)
    bound = np.zeros(out.shape) if want_bound else None
    shape = out.shape[1:3]
    covered = np.ones(shape, bool) if pixels is None else np.asarray(pixels, bool)
    if isinstance(fold_index, (list, tuple)):
        indices = [np.full(shape, float(first + s)) for first, count in fold_index for s in range(count)]
    elif np.ndim(fold_index) == 0:
        indices = [np.full(shape, float(fold_index + s)) for s in range(len(frames))]
    else:
        indices = [np.asarray(fold_index, np.float64) + s for s in range(len(frames))]
    assert len(indices) == len(frames)
    work = out[:, covered]
    work_bound = bound[:, covered] if want_bound else None
    for frame, n in zip(frames, indices):
        splat(work, np.asarray(frame, np.float32)[covered], n[covered] <= 1.0, start, dt, work_bound)
    out[:, covered] = work
    if want_bound:
        bound[:, covered] = work_bound
        return out, bound
    return out


def _shift(a, dx, dy):
    """out[y, x] = a[y + dy, x + dx] where that lies inside, else 0."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def valid_pixels(mean, moments, tiers, width):
    mean, moments, tiers = (np.asarray(a, np.float32) for a in (mean, moments, tiers))
    with np.errstate(invalid="ignore"):
        return (moments[:, :width, 3] >= 1) & np.isfinite(mean[:, :width, :3]).all(axis=-1) & np.isfinite(tiers[:, :, :width]).all(axis=(0, -1))


def resolve(mean, moments, tiers, fallback, width=None, start=1.0, support=4.0, dtype=np.float32, parts=None, want_bound=False):
    """-> (height, width, 4) of dtype: (R / N, luminance(T - R) / N); (fallback.rgb, -1) for a pixel that is not valid. parts: a dict that receives the per-tier
    factors "r" (K, H, W), the support counts "n" and "valid". want_bound (float64): also the first-order bound (H, W, 4) on |out32 - out64|."""
    dt = np.float64 if dtype == np.float64 else np.float32
    tiers32 = np.asarray(tiers, np.float32)
    count = tiers32.shape[0]
    width = tiers32.shape[2] if width is None else width
    valid = valid_pixels(mean, moments, tiers32, width)
    with np.errstate(all="ignore"):
        s = tiers32[:, :, :width].astype(dt)
        n_samples = np.asarray(moments, np.float32)[:, :width, 3].astype(dt)
        area = []
        for j in range(count):
            w = np.where(valid, s[j, ..., 3], dt(0)).astype(dt)
            total = np.zeros(valid.shape, dt)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    total = total + _shift(w, dx, dy)
            area.append(total)
        area.append(np.zeros(valid.shape, dt))   # A_K
        kept = s[0, ..., :3].copy()
        everything = kept.copy()
        b = dt(np.float32(start))
        span = dt(np.float32(support)) - dt(1)
        factors, counts = [np.ones(valid.shape, dt)], [(area[0] + area[1]).astype(dt)]
        if want_bound:
            d_kept = np.zeros(kept.shape); d_all = np.zeros(kept.shape); abs_all = np.abs(kept)
        for j in range(1, count):
            b = b * dt(BASE)
            n = (area[j - 1] + area[j]) + area[j + 1]
            rc = np.fmin(np.fmax((n - dt(1)) / span, dt(0)), dt(1))
            lum_kept = luminance(kept[..., 0], kept[..., 1], kept[..., 2], dt)
            rcol = np.fmin(dt(1), lum_kept / b)
            r = np.fmax(rc, rcol)
            if want_bound:
                # n: up to 27 terms >= 0 summed in 3 x 8 + 2 additions: |dn| <= 10 u n. rc: n - 1, support - 1 and the quotient round once each:
                #   |drc| <= (|dn| + 3 u |n - 1|) / (support - 1).   rcol: |dlum| <= sum(c |dR|) + 3 u sum(c |R|), the quotient rounds once: |drcol| <= (|dlum| + u |lum|) / b.
                # r = max(rc, rcol): |dr| <= max(|drc|, |drcol|).   R' = R + r S: |dR'| <= |dR| + |dr| |S| + u |r S| + u |R'|.
                # A clamp is constant outside its interval: where the argument clears 1 (or 0) by more than its own error, both evaluations give the same 1 (or 0).
                d_rc = (10 * U * np.abs(n) + 3 * U * np.abs(n - 1)) / span
                raw = (n - 1) / span
                d_rc = np.where((raw - d_rc >= 1) | (raw + d_rc <= 0), 0.0, d_rc)
                abs_lum = LUMA[0] * np.abs(kept[..., 0]) + LUMA[1] * np.abs(kept[..., 1]) + LUMA[2] * np.abs(kept[..., 2])
                d_rcol = (LUMA[0] * d_kept[..., 0] + LUMA[1] * d_kept[..., 1] + LUMA[2] * d_kept[..., 2] + 3 * U * abs_lum + U * np.abs(lum_kept)) / b
                d_rcol = np.where(lum_kept / b - d_rcol >= 1, 0.0, d_rcol)
                d_r = np.maximum(d_rc, d_rcol)
            kept = kept + r[..., None] * s[j, ..., :3]
            everything = everything + s[j, ..., :3]
            if want_bound:
                d_kept = d_kept + d_r[..., None] * np.abs(s[j, ..., :3]) + U * np.abs(r[..., None] * s[j, ..., :3]) + U * np.abs(kept)
                abs_all = abs_all + np.abs(s[j, ..., :3])
                d_all = d_all + U * abs_all   # T: one rounding per addition, each at most u times the sum of the magnitudes so far
            factors.append(r); counts.append(n)
        held = everything - kept
        out = np.concatenate([kept / n_samples[..., None], (luminance(held[..., 0], held[..., 1], held[..., 2], dt) / n_samples)[..., None]], axis=-1)
    plain = np.concatenate([np.asarray(fallback, np.float32)[:, :width, :3].astype(dt), np.full(valid.shape + (1,), dt(-1))], axis=-1)
    result = np.where(valid[..., None], out, plain).astype(dt)
    if parts is not None:
        parts.update(r=np.stack(factors), n=np.stack(counts), valid=valid)
    if not want_bound:
        return result
    with np.errstate(all="ignore"):
        # out.rgb = R / N: |d| <= (|dR| + u |R|) / N.   out.w = luminance(T - R) / N: the difference carries |dT| + |dR| + u |T - R|, the luminance 3 u on its magnitudes,
        # the quotient u.
        d_rgb = (d_kept + U * np.abs(kept)) / n_samples[..., None]
        d_held = d_all + d_kept + U * np.abs(held)
        abs_held = LUMA[0] * np.abs(held[..., 0]) + LUMA[1] * np.abs(held[..., 1]) + LUMA[2] * np.abs(held[..., 2])
        d_w = (LUMA[0] * d_held[..., 0] + LUMA[1] * d_held[..., 1] + LUMA[2] * d_held[..., 2] + 4 * U * abs_held) / n_samples
        bound = np.concatenate([d_rgb, d_w[..., None]], axis=-1)
    return result, np.where(valid[..., None], bound, 0.0)
