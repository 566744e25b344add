"""Float64 restatement of alpha-tested opacity masks, and a masked brute force. TEST INFRASTRUCTURE ONLY.

numpy only; the one thing taken from elsewhere is tests/trace_reference.py (its float64 Moeller-Trumbore `intersect_pairs`, its
tolerances and its `BruteForce` record), so that tests/trace_checks.py applies to masked scenes unchanged.

A mask is a bool array [H, W] (True: opaque), row 0 first in texture memory. A candidate with barycentrics (u, v) on a triangle
whose shading record holds uv_0, uv_edge_1, uv_edge_2 (float32 values) looks up the texel that holds
(s, t) = uv_0 + u uv_edge_1 + v uv_edge_2, wrapped: x = floor(s W) mod W, y = floor(t H) mod H.

What float32 may get differently -- the error bound of a texel coordinate, derived here and not tuned against the device:
  * u and v carry the pair's `uv_tol` (trace_reference: TOL.UV x EPS32 x the pair's condition), so s moves by at most
    uv_tol x (|uv_edge_1.s| + |uv_edge_2.s|), in texels times W: the triangle's texture-edge lengths in texels;
  * evaluating uv_0 + u e1 + v e2 and the product with W in float32 is four roundings and one, each half an ulp of an
    intermediate: 4 float32 ulps of |s| W cover them while the intermediates are of the size of s. (They are larger where uv_0
    cancels against the edge terms. The cases of tests/opacity_cases.py keep texture edges of at least one unit against
    |uv_0| <= 2.7, so the first term, >= 8 EPS32 x edge length x W, exceeds an ulp of |uv_0| W there.)
A pair is texel-ambiguous when another texel within that bound of (s W, t H) holds the other bit: float32 may accept or reject it.
"""
import numpy as np

import trace_reference as ref

F32 = np.float32


def cut_of(threshold):
    """The byte a channel must reach: clamp(int(ceilf(threshold * 255.0f)), 0, 255), the product in float32."""
    return int(min(255, max(0, np.ceil(F32(threshold) * F32(255.0)))))


def opaque_of(rgba, channel, threshold):
    """The mask of an RGBA8 image [H, W, 4] (uint8)."""
    return np.asarray(rgba)[:, :, channel] >= cut_of(threshold)


def pack_bits(opaque):
    """Bit y * W + x of texel (x, y) in word (y * W + x) >> 5, bit & 31, no row padding; unused bits of the last word 0."""
    flat = np.asarray(opaque, bool).ravel()
    padded = np.zeros((flat.size + 31) // 32 * 32, np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def texel_of(s, t, width, height):
    """The texel (x, y) that holds the texture coordinate (s, t), wrapped. Float64; exact integers s W belong to the texel they start."""
    x = np.floor(np.asarray(s, np.float64) * width).astype(np.int64) % width
    y = np.floor(np.asarray(t, np.float64) * height).astype(np.int64) % height
    return x, y


def coordinate_of(u, v, uv0, uve1, uve2):
    """(s, t) in float64 from float64 barycentrics and the float32 values of a shading triangle. uv*: (..., 2)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    s = uv0[..., 0] + u * uve1[..., 0] + v * uve2[..., 0]
    t = uv0[..., 1] + u * uve1[..., 1] + v * uve2[..., 1]
    return s, t


def classify(mask, u, v, uv_tol, uv0, uve1, uve2):
    """Per element: (bit of the float64 texel, texel-ambiguous). See the module text for the bound."""
    mask = np.asarray(mask, bool)
    height, width = mask.shape
    s, t = coordinate_of(u, v, uv0, uve1, uve2)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = s * width, t * height
        ex = uv_tol * (np.abs(uve1[..., 0]) + np.abs(uve2[..., 0])) * width + 4.0 * np.spacing(np.abs(fx).astype(F32)).astype(np.float64)
        ey = uv_tol * (np.abs(uve1[..., 1]) + np.abs(uve2[..., 1])) * height + 4.0 * np.spacing(np.abs(fy).astype(F32)).astype(np.float64)
    finite = np.isfinite(fx) & np.isfinite(fy) & np.isfinite(ex) & np.isfinite(ey)
    fx, fy, ex, ey = (np.where(finite, a, 0.0) for a in (fx, fy, ex, ey))
    wide = ~finite | (ex >= 0.5) | (ey >= 0.5)      # the bound spans texels: anything may come out
    ex, ey = np.minimum(ex, 0.5), np.minimum(ey, 0.5)
    x, y = np.floor(fx).astype(np.int64) % width, np.floor(fy).astype(np.int64) % height
    bit = mask[y, x]
    differs = np.zeros(bit.shape, bool)
    for gx in (fx - ex, fx + ex):
        for gy in (fy - ey, fy + ey):
            differs |= mask[np.floor(gy).astype(np.int64) % height, np.floor(gx).astype(np.int64) % width] != bit
    return bit, differs | wide


def masked_brute_force(origin, direction, world, uv0, uve1, uve2, mask_of_triangle, masks, chunk_pairs=1 << 21):
    """trace_reference.brute_force over triangles of which some carry a mask: mask_of_triangle (K,) indexes `masks` (-1: none);
    uv0, uve1, uve2: (K, 2) float32 values of the shading records. A pair whose texel is 0 is dropped before the closest /
    second / clear reductions -- unless it is texel-ambiguous: those enter t_ambiguous (and stay in `t` only where float64's bit is 1).
    Also returns rejected_in_front (N,): candidates float64 rejects in front of each ray's closest hit."""
    TOL, EPS32 = ref.TOL, ref.EPS32
    o = np.ascontiguousarray(np.asarray(origin, np.float64).T)
    d = np.ascontiguousarray(np.asarray(direction, np.float64).T)
    w = np.asarray(world, np.float64)
    p0, e1, e2 = w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]
    uv0, uve1, uve2 = (np.asarray(a, np.float64) for a in (uv0, uve1, uve2))
    mask_of_triangle = np.asarray(mask_of_triangle)
    n, k = o.shape[0], w.shape[0]
    out = {name: np.full(n, np.inf) for name in ("t", "t_second", "t_ambiguous", "t_clear", "t_tiny")}
    for name in ("margin", "grazing", "u", "v", "t_tol", "uv_tol"):
        out[name] = np.zeros(n)
    out["index"] = np.full(n, -1, np.int64)
    rejected_in_front = np.zeros(n, np.int64)
    rows = max(1, chunk_pairs // max(k, 1))
    for a in range(0, n, rows):
        b = min(n, a + rows)
        t, u, v, g, scale, size, nd, det = ref.intersect_pairs(o[a:b], d[a:b], p0, e1, e2)
        with np.errstate(invalid="ignore"):
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_tol = TOL.T * EPS32 * scale / (g * nd)
            uv_tol = TOL.UV * EPS32 * scale / (g * size)
        finite = np.isfinite(t) & (g > 0)
        valid = np.isfinite(t) & (det > 0) & (margin >= 0) & (t > 0)
        with np.errstate(invalid="ignore"):
            tiny = np.isfinite(t) & (det > 0) & ((g == 0) | (np.abs(t) * det < TOL.DET_MIN)) & (margin >= 0) & (t > 0)
            g = np.where(tiny, 0.0, g)
        ambiguous = finite & (margin >= -TOL.MARGIN / TOL.UV * uv_tol) & (t > -TOL.GAP / TOL.T * t_tol) & \
            ((margin < TOL.MARGIN / TOL.UV * uv_tol) | (g < TOL.GRAZING) | (t < TOL.GAP / TOL.T * t_tol))
        # ---- the masks: the float64 bit of every pair of a masked triangle, and whether float32 may see the other one
        opaque = np.ones(t.shape, bool)
        texel_ambiguous = np.zeros(t.shape, bool)
        for m, mask in enumerate(masks):
            cols = np.nonzero(mask_of_triangle == m)[0]
            if cols.size == 0:
                continue
            candidate = (valid | ambiguous | tiny)[:, cols]
            uu, vv, tol = (np.where(candidate, x[:, cols], 0.0) for x in (u, v, uv_tol))
            bit, amb = classify(mask, uu, vv, tol, uv0[cols][None], uve1[cols][None], uve2[cols][None])
            opaque[:, cols] = bit | ~candidate
            texel_ambiguous[:, cols] = amb & candidate
        rejected = ~opaque & ~texel_ambiguous
        rejected_valid = valid & rejected
        valid = valid & opaque                                 # (a texel-ambiguous pair stays a hit only where float64 sees a 1 ...)
        ambiguous = (ambiguous & ~rejected) | (texel_ambiguous & (valid | ambiguous | tiny | rejected_valid))   # ... and is ambiguous either way
        tiny = tiny & ~rejected
        tv = np.where(valid, t, np.inf)
        best = tv.argmin(1)
        r = np.arange(b - a)
        bt = tv[r, best]
        hit = np.isfinite(bt)
        tv2 = tv.copy(); tv2[r, best] = np.inf
        out["t"][a:b] = bt
        out["index"][a:b] = np.where(hit, best, -1)
        out["t_second"][a:b] = tv2.min(1)
        out["t_ambiguous"][a:b] = np.where(ambiguous | tiny, np.maximum(t, 0.0), np.inf).min(1)
        out["t_clear"][a:b] = np.where(valid & ~ambiguous & ~tiny, t, np.inf).min(1)
        out["t_tiny"][a:b] = np.where(tiny, t, np.inf).min(1)
        for name, arr in (("margin", margin), ("grazing", g), ("u", u), ("v", v), ("t_tol", t_tol), ("uv_tol", uv_tol)):
            out[name][a:b] = np.where(hit, arr[r, best], 0.0)
        rejected_in_front[a:b] = (rejected_valid & (t < bt[:, None])).sum(1)
    return ref.BruteForce(**out), rejected_in_front
