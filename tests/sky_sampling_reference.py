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
    uu, vv = np.meshgrid(us, vs)
    L = _bilinear(sky, uu.ravel(), vv.ravel()).reshape(len(vs), len(us), 3)
    return scale * np.einsum("vuc,u,v->c", L, uw, vw * jac)


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
