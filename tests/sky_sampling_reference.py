"""numpy float64 restatement of sky importance sampling (kernels_sky.hip, rt_shading.h: sky_sample_direction / sky_pdf) and a
quadrature of the bilinear sky, for the CPU and GPU tests of the feature.

A cell is one sky texel in sample_sky's mapping (u = atan2(-z, x) / 2pi + 1/2, v = acos(y) / pi). Its weight is the largest luminance
over the clamped 3 x 3 texel neighbourhood times its solid angle; the pdf of every direction in a cell is P_cell / Omega_cell.
`sky` arguments are (H, W, 4) float arrays as rt_set_sky takes them."""
import numpy as np


def luminance(sky):
    s = np.asarray(sky, np.float64)
    return 0.299 * s[..., 0] + 0.587 * s[..., 1] + 0.114 * s[..., 2]


def footprint_luminance(sky):
    """(H, W): the largest luminance among the texels whose bilinear footprint reaches into each cell (clamped, not wrapped), at least 0."""
    lum = luminance(sky)
    h, w = lum.shape
    out = np.zeros_like(lum)
    for dy in (-1, 0, 1):
        ys = np.clip(np.arange(h) + dy, 0, h - 1)
        for dx in (-1, 0, 1):
            xs = np.clip(np.arange(w) + dx, 0, w - 1)
            out = np.maximum(out, lum[ys][:, xs])
    return out


def row_edges(h):
    return np.pi * np.arange(h + 1) / h


def cell_solid_angle(h, w):
    """(H,): the solid angle of a cell of each row, (cos theta_0 - cos theta_1) 2 pi / W."""
    t = row_edges(h)
    return (np.cos(t[:-1]) - np.cos(t[1:])) * 2.0 * np.pi / w


class Tables:
    """The distribution of one sky: float64 tables, and the float32 CDFs as the device stores them."""

    def __init__(self, sky):
        sky = np.asarray(sky, np.float64)
        self.h, self.w = sky.shape[:2]
        self.lum = footprint_luminance(sky)
        self.weight = self.lum * cell_solid_angle(self.h, self.w)[:, None]
        self.row_total = self.weight.sum(axis=1)
        self.total = float(self.row_total.sum())
        self.p_cell = self.weight / self.total if self.total > 0 else np.zeros_like(self.weight)
        self.pdf = self.lum / self.total if self.total > 0 else np.zeros_like(self.lum)   # = P_cell / Omega_cell
        self.marginal = _cdf32(self.row_total)
        self.conditional = np.stack([_cdf32(r) for r in self.weight])

    def invert(self, uv):
        """(N, 2) float32 points -> (directions (N, 3) float64, row, column, pdf): the device's float32 inversion, the direction in float64."""
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        row, fy = _invert32(self.marginal, uv[:, 1])
        col = np.empty_like(row); fx = np.empty(len(row), np.float32)
        for r in np.unique(row):
            m = row == r
            col[m], fx[m] = _invert32(self.conditional[r], uv[m, 0])
        phi = ((col + fx.astype(np.float64)) / self.w - 0.5) * 2.0 * np.pi
        t = row_edges(self.h)
        c0, c1 = np.cos(t[row]), np.cos(t[row + 1])
        cos_t = c0 + fy.astype(np.float64) * (c1 - c0)
        sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
        d = np.stack([sin_t * np.cos(phi), cos_t, -sin_t * np.sin(phi)], axis=1)
        return d, row, col, self.pdf[row, col]

    def cell(self, directions):
        d = np.asarray(directions, np.float64).reshape(-1, 3)
        u = np.arctan2(-d[:, 2], d[:, 0]) / (2.0 * np.pi) + 0.5
        v = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
        return np.clip((v * self.h).astype(int), 0, self.h - 1), np.clip((u * self.w).astype(int), 0, self.w - 1)

    def pdf_of(self, directions):
        r, c = self.cell(directions)
        return self.pdf[r, c]


def _cdf32(weights):
    """Inclusive, normalised CDF in float32, last entry exactly 1 (uniform for a row without weight), as kernels_sky.hip stores it."""
    weights = np.asarray(weights, np.float64)
    total = weights.sum()
    n = len(weights)
    if not total > 0:
        return ((np.arange(n) + 1) / np.float32(n)).astype(np.float32)
    c = (np.cumsum(weights) / total).astype(np.float32)
    c[-1] = 1.0
    return c


def _invert32(cdf, u):
    """First entry above u and where u lies between it and its predecessor, in float32 operations (rt_shading.h: sky_cdf_invert)."""
    u = np.asarray(u, np.float32)
    i = np.minimum(np.searchsorted(cdf, u, side="right"), len(cdf) - 1)
    c0 = np.where(i > 0, cdf[np.maximum(i - 1, 0)], np.float32(0.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (u - c0).astype(np.float32) / (cdf[i] - c0).astype(np.float32)
    f = np.nan_to_num(f.astype(np.float32), nan=0.0)
    return i, np.clip(f, np.float32(0.0), np.float32(1.0 - 2.0 ** -24)).astype(np.float32)


def sample_sky(sky, scale, directions):
    """sample_sky (rt_shading.h, CUDA/Sky.h) in float64: bilinear, taps clamped at the borders."""
    sky = np.asarray(sky, np.float64)
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    u = np.arctan2(-d[:, 2], d[:, 0]) / (2.0 * np.pi) + 0.5
    v = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
    return scale * _bilinear(sky, u, v)


def _bilinear(sky, u, v):
    h, w = sky.shape[:2]
    def taps(c, n):
        x = c * n - 0.5
        x0 = np.floor(x)
        f = x - x0
        i0 = np.clip(x0.astype(int), 0, n - 1); i1 = np.clip(x0.astype(int) + 1, 0, n - 1)
        return i0, i1, f
    x0, x1, fx = taps(u, w); y0, y1, fy = taps(v, h)
    fx = fx[:, None]; fy = fy[:, None]
    top = sky[y0, x0, :3] * (1 - fx) + sky[y0, x1, :3] * fx
    bottom = sky[y1, x0, :3] * (1 - fx) + sky[y1, x1, :3] * fx
    return top * (1 - fy) + bottom * fy


def _gauss_nodes(breaks, order):
    x, wt = np.polynomial.legendre.leggauss(order)
    a, b = breaks[:-1, None], breaks[1:, None]
    return ((a + b) / 2 + (b - a) / 2 * x).ravel(), ((b - a) / 2 * wt).ravel()


def upper_hemisphere_irradiance(sky, scale=1.0):
    """E = integral over the upper hemisphere (y > 0) of sample_sky(w) cos(theta) dw, RGB, float64. Gauss-Legendre between the kinks of the
    bilinear filter (texel centres) in u and in v, so the piecewise-bilinear sky is integrated to rounding."""
    sky = np.asarray(sky, np.float64)
    h, w = sky.shape[:2]
    ub = np.unique(np.concatenate([[0.0, 1.0], (np.arange(w) + 0.5) / w]))
    vb = np.unique(np.concatenate([[0.0, 0.5], (np.arange(h) + 0.5) / h]))
    vb = vb[vb <= 0.5]
    us, uw = _gauss_nodes(ub, 2)
    vs, vw = _gauss_nodes(vb, 12)
    theta = vs * np.pi
    jac = np.cos(theta) * np.sin(theta) * np.pi * 2.0 * np.pi   # cos(theta) dw = cos sin dtheta dphi, dtheta = pi dv, dphi = 2 pi du
    total = np.zeros(3)
    step = max(1, (1 << 20) // len(us))   # (a slab of v nodes at a time: a 1027 x 515 sky has 6.4 million nodes)
    for first in range(0, len(vs), step):
        uu, vv = np.meshgrid(us, vs[first:first + step])
        L = _bilinear(sky, uu.ravel(), vv.ravel()).reshape(-1, len(us), 3)
        total += np.einsum("vuc,u,v->c", L, uw, (vw * jac)[first:first + step])
    return scale * total


def sun_sky(w=128, h=64, sun=(40, 20), sun_value=20000.0, base=0.5):
    """A dim gradient with a bright 2 x 2-texel sun at texel (x, y) of its top-left corner: the sky of the tests."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sky = np.zeros((h, w, 4), np.float32)
    g = base * (1.0 - yy / h)
    sky[..., 0] = g * 0.8 + 0.05 * xx / w; sky[..., 1] = g * 0.9; sky[..., 2] = g * 1.2
    sky[..., 3] = 1.0
    x, y = sun
    sky[y:y + 2, x:x + 2, :3] = np.array([1.0, 0.95, 0.85], np.float32) * np.float32(sun_value)
    return sky


# ---- the tables entry by entry (tests/sky_cases.py, test_sky_tables.py, test_gpu_sky_tables.py) ---------------------------------------

SKY_BLOCK = 256   # RT_SKY_BLOCK: threads of a scan workgroup; thread t owns the span [t * per_thread, (t + 1) * per_thread) of the n items


def per_thread(n):
    return (n + SKY_BLOCK - 1) // SKY_BLOCK


def luminance32(sky):
    """luminance() of rt_shading.h in float32 operations, unfused (the kernels are built with -ffp-contract=off): (0.299f r + 0.587f g) + 0.114f b."""
    s = np.asarray(sky, np.float32)
    return (np.float32(0.299) * s[..., 0] + np.float32(0.587) * s[..., 1]) + np.float32(0.114) * s[..., 2]


def footprint_luminance32(sky):
    """sky_footprint_luminance of kernels_sky.hip for a sky without NaN: the exact float32 maximum over the clamped 3 x 3 neighbourhood, at least 0."""
    lum = luminance32(sky)
    h, w = lum.shape
    out = np.zeros_like(lum)
    for dy in (-1, 0, 1):
        ys = np.clip(np.arange(h) + dy, 0, h - 1)
        for dx in (-1, 0, 1):
            xs = np.clip(np.arange(w) + dx, 0, w - 1)
            out = np.maximum(out, lum[ys][:, xs])
    return out


def _hillis_steele(v):
    """block_inclusive_scan: the inclusive scan of the last axis (SKY_BLOCK long) in the kernel's order of additions."""
    v = np.array(v, np.float64)
    offset = 1
    while offset < SKY_BLOCK:
        add = np.zeros_like(v)
        add[..., offset:] = v[..., :-offset]
        v = v + add
        offset <<= 1
    return v


def scan_forward(weights):
    """(..., n) float64 -> (inclusive prefix sums, total): the plain order, one running sum from the left."""
    c = np.cumsum(np.asarray(weights, np.float64), axis=-1)
    return c, c[..., -1].copy()


def scan_spans(weights, subtracting=False):
    """(..., n) float64 -> (inclusive prefix sums, total) in the order of kernel_sky_rows / kernel_sky_marginal: each of SKY_BLOCK threads sums its
    span of per_thread(n) items from the left, the span sums are scanned (Hillis-Steele), and every thread walks its span again from the
    scan's entry of the thread before it (0 for thread 0). The total is the scan's last entry. (Padding with 0.0 is exact: x + 0.0 = x.)
    `subtracting=True` starts each walk from `inclusive - sum` instead, as the kernels did before the dynamic-range case showed what that
    difference loses (test_sky_tables.py keeps the demonstration)."""
    weights = np.asarray(weights, np.float64)
    n = weights.shape[-1]
    pt = per_thread(n)
    padded = np.zeros(weights.shape[:-1] + (SKY_BLOCK * pt,), np.float64)
    padded[..., :n] = weights
    spans = padded.reshape(weights.shape[:-1] + (SKY_BLOCK, pt))
    sums = np.zeros(spans.shape[:-1], np.float64)
    for k in range(pt):
        sums = sums + spans[..., k]
    inclusive = _hillis_steele(sums)
    prefix = np.zeros_like(inclusive)
    prefix[..., 1:] = inclusive[..., :-1]
    if subtracting:
        prefix = inclusive - sums
    out = np.empty_like(spans)
    for k in range(pt):
        prefix = prefix + spans[..., k]
        out[..., k] = prefix
    return out.reshape(padded.shape)[..., :n], inclusive[..., -1].copy()


def cdf32_from_scan(prefix, total):
    """The float32 CDF entries kernel_sky_rows / kernel_sky_marginal store for inclusive prefix sums (..., n) and totals (...): float(prefix / total),
    the last entry 1; float(x + 1) / float(n) throughout where the total is not above 0. One rounding from the float64 quotient, as _cdf32."""
    prefix = np.asarray(prefix, np.float64)
    total = np.asarray(total, np.float64)[..., None]
    n = prefix.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (prefix / total).astype(np.float32)
    c[..., -1] = 1.0
    uniform = ((np.arange(n) + 1) / np.float32(n)).astype(np.float32)
    return np.where(total > 0, c, uniform).astype(np.float32)


class DeviceTables:
    """The tables as kernels_sky.hip builds them, restated: luminance and the 3 x 3 maximum exactly in float32, everything after them in float64
    in the given order of additions ("forward": scan_forward, "spans": scan_spans), rounded to float32 once per entry as the kernels round.

    What may differ from the device, and by how much:
    * CDF entries and cell pdfs. The device's float64 quotient differs from this one by its order of additions and by its double cos (relative
      1e-16 .. 1e-11, see below), so the float32 entry differs only where the quotient sits on a float32 rounding boundary: by one ulp, and in
      no more than 1 entry in 10 000 of a table (`CAP`). The two orders here keep that cap against each other on every case of sky_cases.py
      (test_sky_tables.py).
    * Row totals and the total, float64 (`row_total_bound`, `total_bound`). A row total is a sum of W products double(m) * omega. With u = 2^-53:
      each product is rounded once (u), a sum of W terms of one sign in any order is off by at most (W - 1) u of its value, and both sides sum:
      2 W u in all. omega = (cos t0 - cos t1) * 2 pi / W: the arguments are the same IEEE products and quotients on both sides; the device's cos
      is taken as within 2 ulp and numpy's as within 1 ulp, an ulp of a cosine being at most u * 2 (|cos| <= 1: spacing 2^-53 below 1), so the
      difference of the two cosines differs by at most 2 * 3 * 2 u = 12 u absolutely, a share 12 u / (cos t0 - cos t1) of omega -- 3e-10 in the
      polar rows of a 1024-row sky, where the difference cancels to 4.7e-6 -- and the subtraction, the two products and the quotient add 4 u each side.
      bound(row) = row_total * ((2 W + 8) u + 12 u / (cos t0 - cos t1)); bound(total) = sum of the rows' bounds + 2 H u * total."""

    CAP = 10000        # at most 1 entry in CAP of a table may differ between two evaluations, and by one float32 ulp

    def __init__(self, sky, order="forward"):
        scan = {"forward": scan_forward, "spans": scan_spans}[order]
        sky = np.asarray(sky, np.float32)
        self.h, self.w = sky.shape[:2]
        self.lum = footprint_luminance32(sky)
        self.omega = cell_solid_angle(self.h, self.w)
        self.weight = self.lum.astype(np.float64) * self.omega[:, None]
        prefix, self.row_total = scan(self.weight)
        self.conditional = cdf32_from_scan(prefix, self.row_total)
        prefix, total = scan(self.row_total)
        self.total = float(total)
        self.marginal = cdf32_from_scan(prefix, total)
        usable = self.total > 0 and np.isfinite(self.total)
        self.cell_pdf = (self.lum.astype(np.float64) / self.total).astype(np.float32) if usable else np.zeros_like(self.lum)
        u = 2.0 ** -53
        t = row_edges(self.h)
        self.row_total_bound = self.row_total * ((2 * self.w + 8) * u + 12 * u / (np.cos(t[:-1]) - np.cos(t[1:])))
        self.total_bound = float(self.row_total_bound.sum() + 2 * self.h * u * self.total)


def ulp_distance32(a, b):
    """|a - b| in float32 ulps for arrays of finite floats of one sign pattern (the tables are all >= 0)."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def entries_differ(a, b):
    """(entries that differ, the largest difference in ulps) of two float32 tables."""
    d = ulp_distance32(a, b)
    return int((d != 0).sum()), int(d.max()) if d.size else 0


def sampled_cell_probability(marginal, conditional):
    """P32 (H, W) float64: the probability with which the inversion of the float32 CDFs picks each cell, delta marginal x delta conditional."""
    m = np.diff(np.asarray(marginal, np.float64), prepend=0.0)
    c = np.diff(np.asarray(conditional, np.float64), axis=1, prepend=0.0)
    return m[:, None] * c


def sampled_against_claimed(marginal, conditional, p_cell):
    """(sum over cells of |P32 - P_cell|, the bound (W + H) 2^-24 -- every CDF entry is off by at most 2^-25, half an ulp below 1 --, the mass of
    cells with P_cell > 0 that the float32 CDFs never pick)."""
    p32 = sampled_cell_probability(marginal, conditional)
    h, w = p32.shape
    return float(np.abs(p32 - p_cell).sum()), (w + h) * 2.0 ** -24, float(p_cell[(p_cell > 0) & (p32 == 0)].sum())


def invert_tables(marginal, conditional, uv):
    """sky_sample_direction's two searches on given float32 tables: (row, fy, column, fx) for (N, 2) float32 points (u: column, v: row)."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    row, fy = _invert32(np.asarray(marginal, np.float32), uv[:, 1])
    col = np.empty_like(row); fx = np.empty(len(row), np.float32)
    order = np.argsort(row, kind="stable")
    bounds = np.flatnonzero(np.diff(row[order], prepend=-1, append=-1))
    for a, b in zip(bounds[:-1], bounds[1:]):
        idx = order[a:b]
        col[idx], fx[idx] = _invert32(conditional[row[idx[0]]], uv[idx, 0])
    return row, fy, col, fx


def direction_of(h, w, row, fy, col, fx):
    """The float64 direction of a point at fractions (fx, fy) of cell (row, col): phi uniform across the column, cos(theta) across the row."""
    phi = ((col + np.asarray(fx, np.float64)) / w - 0.5) * 2.0 * np.pi
    t = row_edges(h)
    c0, c1 = np.cos(t[row]), np.cos(t[row + 1])
    cos_t = c0 + np.asarray(fy, np.float64) * (c1 - c0)
    sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
    return np.stack([sin_t * np.cos(phi), cos_t, -sin_t * np.sin(phi)], axis=1)
