"""Float64 restatement of the SVGF + TAA filter stage: reproject, spatial variance, a-trous, finalize,
TAA resolve + finalize, vectorised over the pixels of a pitch x height frame.

Written from DESIGN.md and the documented semantics of the oracle's `Frame` (oracle/binding.py); it shares no code
with the oracle or the kernels. Every DECISION is formed in float32, exactly as the kernels form it -- the previous
pixel position (C truncation), the reprojection consistency test on normals decoded in float32, sky (depth == 0), whether
a tap lies in the image, history counts and the `history >= 4` switch, which branch of Mitchell-Netravali a distance
takes and whether a TAA resolve has any weight. Everything after the decisions is float64: bilinear weights, edge-stopping
weights with true pow / exp, all sums, E[x^2] - E[x]^2, the 3 x 3 variance blur, the YCoCg clamp and the tone mapping.

Layouts are the oracle Frame's: images are (height, pitch, C); the filter writes columns x < width only, except the
spatial-variance pass, which copies its input to its output in the padding columns; the depth gradient at x = width - 1
reads the neighbour clamped to pitch - 1 (a padding column when pitch > width); the variance blur clamps to width - 1.
The history of normals is kept as the oracle keeps it: the octahedral g-buffer texel (x, y: normal, z: depth).
"""
import numpy as np

F32 = np.float32


def f32c(v):
    """A float32 constant of the kernels, as a float64."""
    return float(F32(v))


EPSILON = f32c(1e-8)
LUMA = (f32c(0.299), f32c(0.587), f32c(0.114))
FEEDBACK_ITERATION = 1
TAA_ROUNDING = 4 * 2.0 ** -24   # relative rounding of the kernels' float32 colours, sums of nine squares and their difference (Filter.taa_slack)


def luminance(c):
    return LUMA[0] * c[..., 0] + LUMA[1] * c[..., 1] + LUMA[2] * c[..., 2]


def oct_decode32(xy):
    """Octahedral normal -> unit normal, in float32 with the kernels' operation order (decisions read it)."""
    xy = np.asarray(xy, F32)
    fx = xy[..., 0] * F32(2) - F32(1)
    fy = xy[..., 1] * F32(2) - F32(1)
    nz = (F32(1) - np.abs(fx)) - np.abs(fy)
    t = np.clip(-nz, F32(0), F32(1))
    nx = fx + np.where(fx >= 0, -t, t)
    ny = fy + np.where(fy >= 0, -t, t)
    inv = F32(1) / np.sqrt((nx * nx + ny * ny) + nz * nz)
    return np.stack([nx * inv, ny * inv, nz * inv], axis=-1).astype(F32)


def dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def rgb_to_ycocg(c):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([0.25 * r + 0.5 * g + 0.25 * b, 0.5 * r - 0.5 * b, -0.25 * r + 0.5 * g - 0.25 * b], axis=-1)


def ycocg_to_rgb(c):
    y, co, cg = c[..., 0], c[..., 1], c[..., 2]
    return np.clip(np.stack([y + co - cg, y + cg, y - co - cg], axis=-1), 0.0, 1.0)


_B = _C = F32(1) / F32(3)
_P1 = ((F32(12) - F32(9) * _B) - F32(6) * _C, (F32(-18) + F32(12) * _B) + F32(6) * _C, F32(6) - F32(2) * _B)
_P2 = (-_B - F32(6) * _C, F32(6) * _B + F32(30) * _C, F32(-12) * _B - F32(48) * _C, F32(8) * _B + F32(24) * _C)
_SIXTH = F32(1) / F32(6)


def mitchell_netravali32(x):
    """The kernels' float32 evaluation (only its sign and zero decide anything)."""
    x = np.abs(np.asarray(x, F32))
    x2 = x * x
    x3 = x2 * x
    near = _SIXTH * ((_P1[0] * x3 + _P1[1] * x2) + _P1[2])
    far = _SIXTH * (((_P2[0] * x3 + _P2[1] * x2) + _P2[2] * x) + _P2[3])
    return np.where(x < 1, near, np.where(x < 2, far, F32(0))).astype(F32)


def mitchell_netravali64(x, x32):
    """Float64 value at the exact distance x, on the branch the float32 distance x32 selects."""
    p1 = [float(v) for v in _P1]
    p2 = [float(v) for v in _P2]
    a, a32 = np.abs(x), np.abs(x32)
    near = (p1[0] * a ** 3 + p1[1] * a ** 2 + p1[2]) / 6.0
    far = (p2[0] * a ** 3 + p2[1] * a ** 2 + p2[2] * a + p2[3]) / 6.0
    return np.where(a32 < 1, near, np.where(a32 < 2, far, 0.0))


def taa_resolve32(curr, prev, screen_position_prev, sample_index, width, height):
    """The TAA resolve and its finalize in float32, operation for operation in the kernels' order: the resolved colour (the next
    frame's history) and the displayed colour for every pixel x < width, given the frame's tone-mapped colour `curr` and the
    history `prev` ((height, pitch, 4) float32). Not a restatement -- a replay: fed the device's own inputs it must give the
    device's outputs bit for bit, which checks the resolve apart from the clamp's ill-conditioning (Filter.taa_slack)."""
    H, P = curr.shape[:2]
    curr, prev = np.asarray(curr, F32), np.asarray(prev, F32)
    y, x = np.mgrid[0:H, 0:P]
    colour = curr.copy()

    def ycocg(c):
        r, g, b = c[..., 0], c[..., 1], c[..., 2]
        return np.stack([(F32(0.25) * r + F32(0.5) * g) + F32(0.25) * b, F32(0.5) * r - F32(0.5) * b,
                         (F32(-0.25) * r + F32(0.5) * g) - F32(0.25) * b], axis=-1)

    if sample_index != 0:
        sp = np.asarray(screen_position_prev, F32)
        s_prev = (F32(0.5) + F32(0.5) * sp[..., 0]) * F32(width)
        t_prev = (F32(0.5) + F32(0.5) * sp[..., 1]) * F32(height)
        x_prev = np.trunc(s_prev + F32(0.5)).astype(np.int64)
        y_prev = np.trunc(t_prev + F32(0.5)).astype(np.int64)
        sum_weight = np.zeros((H, P), F32)
        total = np.zeros((H, P, 4), F32)
        for j in range(-2, 2):
            for i in range(-2, 2):
                tx, ty = x_prev + i, y_prev + j
                ok = (tx >= 0) & (tx < width) & (ty >= 0) & (ty < height)
                w = mitchell_netravali32((tx.astype(F32) + F32(0.5)) - s_prev) * mitchell_netravali32((ty.astype(F32) + F32(0.5)) - t_prev)
                w = np.where(ok, w, F32(0))
                sum_weight = np.where(ok, sum_weight + w, sum_weight)
                tap = prev[np.clip(ty, 0, H - 1), np.clip(tx, 0, P - 1)]
                total = np.where(ok[..., None], total + w[..., None] * tap, total)
        resolve = sum_weight > 0
        c_curr = ycocg(colour)
        c_prev = ycocg(total / np.where(resolve, sum_weight, F32(1))[..., None])
        avg, var = c_curr.copy(), c_curr * c_curr
        for dx, dy in ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)):   # the kernels' tap order
            ok = (x + dx >= 0) & (x + dx < width) & (y + dy >= 0) & (y + dy < height)
            c = ycocg(curr[np.clip(y + dy, 0, H - 1), np.clip(x + dx, 0, P - 1)])
            avg = np.where(ok[..., None], avg + c, avg)
            var = np.where(ok[..., None], var + c * c, var)
        ninth = F32(1) / F32(9)
        avg, var = avg * ninth, var * ninth
        sigma = np.sqrt(np.maximum(F32(0), var - avg * avg))
        c_prev = np.minimum(np.maximum(c_prev, avg - F32(1.25) * sigma), avg + F32(1.25) * sigma)
        t = F32(0.1)
        m = (F32(1) - t) * c_prev + t * c_curr
        rgb = np.clip(np.stack([(m[..., 0] + m[..., 1]) - m[..., 2], m[..., 0] + m[..., 2], (m[..., 0] - m[..., 1]) - m[..., 2]], axis=-1), F32(0), F32(1))
        colour[..., :3] = np.where(resolve[..., None], rgb, colour[..., :3])
    sq = colour * colour
    lum = (F32(0.299) * sq[..., 0] + F32(0.587) * sq[..., 1]) + F32(0.114) * sq[..., 2]
    return colour, sq / (F32(1) - lum)[..., None]


class Config:
    """The filter's switches and parameters (rt_gpu_config), float parameters as the float32 the kernels get."""

    def __init__(self, num_atrous_iterations=6, enable_spatial_variance=1, enable_taa=1, alpha_colour=0.1, alpha_moment=0.1,
                 sigma_z=4.0, sigma_n=16.0, sigma_l=10.0):
        self.num_atrous_iterations = int(num_atrous_iterations)
        self.enable_spatial_variance = int(enable_spatial_variance)
        self.enable_taa = int(enable_taa)
        self.alpha_colour, self.alpha_moment = f32c(alpha_colour), f32c(alpha_moment)
        self.sigma_z, self.sigma_n, self.sigma_l = f32c(sigma_z), f32c(sigma_n), f32c(sigma_l)

    def as_dict(self):
        return dict(num_atrous_iterations=self.num_atrous_iterations, enable_spatial_variance=self.enable_spatial_variance,
                    enable_taa=self.enable_taa, alpha_colour=self.alpha_colour, alpha_moment=self.alpha_moment,
                    sigma_z=self.sigma_z, sigma_n=self.sigma_n, sigma_l=self.sigma_l)


class Filter:
    """The filter's persistent state (zero at the start, as the device and the oracle allocate it) and one frame step."""

    def __init__(self, width, height, pitch, config, rhos=(None,)):
        self.w, self.h, self.p, self.cfg = width, height, pitch, config
        z4 = lambda: np.zeros((height, pitch, 4))
        self.fb_d, self.fb_i, self.acc_d, self.acc_i = z4(), z4(), z4(), z4()   # the per-frame radiance and the accumulators: the ping-pong pair
        self.moment = z4()                                                        # frame_buffer_moment
        self.history_length = np.zeros((height, pitch), np.int64)
        self.history_direct, self.history_indirect, self.history_moment = z4(), z4(), z4()
        self.history_normal_and_depth = np.zeros((height, pitch, 4), F32)         # octahedral, as the oracle keeps it
        self.taa_prev, self.taa_curr, self.final = z4(), z4(), z4()
        self.rhos = tuple(TAA_ROUNDING if r is None else r for r in rhos)
        self._slack = {r: np.zeros((height, pitch)) for r in self.rhos}   # taa_slack: per pixel, for each colour error rho

    # ---- helpers over the frame ------------------------------------------------------------------------------------
    def _grid(self):
        y, x = np.mgrid[0:self.h, 0:self.p]
        return x, y

    def _inside(self, x, y):
        return (x >= 0) & (x < self.w) & (y >= 0) & (y < self.h)

    def _at(self, img, x, y):
        """img[y, x] with the positions clamped into the allocation (the caller masks what is not a real tap)."""
        return img[np.clip(y, 0, self.h - 1), np.clip(x, 0, self.p - 1)]

    def _depth_gradient(self, depth, x, y):
        """(right - centre, below - centre): the right neighbour clamped to the PITCH, the lower one to the height."""
        right = depth[y, np.minimum(x + 1, self.p - 1)]
        below = depth[np.minimum(y + 1, self.h - 1), x]
        return right - depth, below - depth

    def _weights(self, dx, dy, gx, gy, zc, z, nc, n, cl_d, cl_i, l_d, l_i, denom_d, denom_i):
        c = self.cfg
        d = gx * dx + gy * dy
        ln_w_z = np.abs(zc - z) / (c.sigma_z * np.abs(d) + EPSILON)
        w_n = np.power(np.maximum(0.0, np.sum(nc * n, axis=-1)), c.sigma_n)
        return (w_n * np.exp(-np.abs(cl_d - l_d) * denom_d - ln_w_z),
                w_n * np.exp(-np.abs(cl_i - l_i) * denom_i - ln_w_z))

    # ---- the stages ---------------------------------------------------------------------------------------------------
    def _reproject(self, normal32, depth32, depth_prev32, sp):
        c, W, H = self.cfg, self.w, self.h
        x, y = self._grid()
        real = (x < W) & (depth32 != 0)   # sky is left alone (and so are the padding columns)
        d, i = self.fb_d, self.fb_i
        moment = np.stack([luminance(d), luminance(i), luminance(d) ** 2, luminance(i) ** 2], axis=-1)

        s_prev = (F32(0.5) + F32(0.5) * sp[..., 0]) * F32(W)
        t_prev = (F32(0.5) + F32(0.5) * sp[..., 1]) * F32(H)
        x_prev = np.trunc(s_prev - F32(0.5)).astype(np.int64)   # C truncation: -0.5 < s_prev < 0.5 gives 0, not -1
        y_prev = np.trunc(t_prev - F32(0.5)).astype(np.int64)
        fs32, ft32 = s_prev - np.floor(s_prev), t_prev - np.floor(t_prev)
        w32 = [(F32(1) - fs32) * (F32(1) - ft32), fs32 * (F32(1) - ft32), (F32(1) - fs32) * ft32]
        w32.append(((F32(1) - w32[0]) - w32[1]) - w32[2])
        fs, ft = fs32.astype(np.float64), ft32.astype(np.float64)
        w64 = [(1 - fs) * (1 - ft), fs * (1 - ft), (1 - fs) * ft, fs * ft]

        prev_n32 = oct_decode32(self.history_normal_and_depth[..., :2])
        prev_z32 = self.history_normal_and_depth[..., 2]

        def consistent(tx, ty):
            ok = self._inside(tx, ty)
            return ok & (dot32(normal32, self._at(prev_n32, tx, ty)) > F32(0.95)) & (np.abs(depth_prev32 - self._at(prev_z32, tx, ty)) < F32(2))

        hist = (self.history_direct, self.history_indirect, self.history_moment)
        cws32 = np.zeros((H, self.p), F32)
        cws64 = np.zeros((H, self.p))
        bil = [np.zeros((H, self.p, 4)) for _ in range(3)]
        taps = []
        for j in range(2):
            for ii in range(2):
                k = ii + 2 * j
                tx, ty = x_prev + ii, y_prev + j
                ok = consistent(tx, ty)
                cws32 = np.where(ok, cws32 + w32[k], cws32)
                use = ok & (w32[k] != 0)
                taps.append((tx, ty, use, k))
                cws64 += np.where(use, w64[k], 0.0)
        # the bilinear weights in float64; the float32 ones only where every float64 weight is zero and a float32 one is not
        f32_fallback = (cws32 > 0) & (cws64 == 0)
        for tx, ty, use, k in taps:
            wk = np.where(f32_fallback, w32[k].astype(np.float64), w64[k]) * use
            for acc, img in zip(bil, hist):
                acc += wk[..., None] * self._at(img, tx, ty)
        cws_bil = np.where(f32_fallback, sum(np.where(u, w32[k].astype(np.float64), 0.0) for _, _, u, k in taps), cws64)

        box = [np.zeros((H, self.p, 4)) for _ in range(3)]
        count = np.zeros((H, self.p))
        for j in (-1, 0, 1):
            for ii in (-1, 0, 1):
                tx, ty = x_prev + ii, y_prev + j
                ok = consistent(tx, ty)
                count += ok
                for acc, img in zip(box, hist):
                    acc += ok[..., None] * self._at(img, tx, ty)

        use_bil = cws32 > 0
        found = use_bil | (count > 0)
        weight = np.where(use_bil, cws_bil, count)
        safe = np.where(found, weight, 1.0)[..., None]
        prev = [np.where(use_bil[..., None], b, bx) / safe for b, bx in zip(bil, box)]

        length = np.where(real & found, self.history_length + 1, np.where(real, 0, self.history_length))
        inv = 1.0 / np.maximum(length, 1)
        alpha_c = np.maximum(c.alpha_colour, inv)[..., None]
        alpha_m = np.maximum(c.alpha_moment, inv)[..., None]
        d_new = (1 - alpha_c) * prev[0] + alpha_c * d
        i_new = (1 - alpha_c) * prev[1] + alpha_c * i
        m_new = (1 - alpha_m) * prev[2] + alpha_m * moment
        temporal = (length >= 4) | (not c.enable_spatial_variance)
        d_new[..., 3] = np.where(temporal, np.maximum(0.0, m_new[..., 2] - m_new[..., 0] ** 2), d_new[..., 3])
        i_new[..., 3] = np.where(temporal, np.maximum(0.0, m_new[..., 3] - m_new[..., 1] ** 2), i_new[..., 3])
        d_new = np.where(found[..., None], d_new, np.concatenate([d[..., :3], np.ones((H, self.p, 1))], axis=-1))
        i_new = np.where(found[..., None], i_new, np.concatenate([i[..., :3], np.ones((H, self.p, 1))], axis=-1))
        m_new = np.where(found[..., None], m_new, moment)

        r = real[..., None]
        self.fb_d = np.where(r, d_new, d)
        self.fb_i = np.where(r, i_new, i)
        self.moment = np.where(r, m_new, self.moment)
        self.history_length = length

    def _variance(self, normal, depth, d_in, i_in):
        """Spatial variance estimate: a 7 x 7 edge-stopping blur where the history is shorter than 4 frames; a copy elsewhere
        -- the sky, the older pixels and the padding columns (visited: x runs to the pitch)."""
        c, W, H = self.cfg, self.w, self.h
        x, y = self._grid()
        young = (self.history_length < 4) & (depth != 0)   # (padding columns: depth 0)
        denom = 1.0 / c.sigma_l
        cl_d, cl_i = luminance(d_in), luminance(i_in)
        gx, gy = self._depth_gradient(depth, x, y)
        sw_d, sw_i = np.ones((H, self.p)), np.ones((H, self.p))
        sc_d, sc_i = d_in.copy(), i_in.copy()
        sm = np.zeros((H, self.p, 4))
        for j in range(-3, 4):
            for ii in range(-3, 4):
                if ii == 0 and j == 0:
                    continue
                tx, ty = x + ii, y + j
                ok = self._inside(tx, ty)
                td, ti, tm = self._at(d_in, tx, ty), self._at(i_in, tx, ty), self._at(self.moment, tx, ty)
                wd, wi = self._weights(ii, j, gx, gy, depth, self._at(depth, tx, ty), normal, self._at(normal, tx, ty),
                                       cl_d, cl_i, luminance(td), luminance(ti), denom, denom)
                wd, wi = np.where(ok, wd, 0.0), np.where(ok, wi, 0.0)
                sw_d += wd
                sw_i += wi
                sc_d += wd[..., None] * td
                sc_i += wi[..., None] * ti
                sm += tm * np.stack([wd, wi, wd, wi], axis=-1)
        sw_d, sw_i = np.maximum(sw_d, 1e-6), np.maximum(sw_i, 1e-6)
        sc_d /= sw_d[..., None]
        sc_i /= sw_i[..., None]
        sm /= np.stack([sw_d, sw_i, sw_d, sw_i], axis=-1)
        sc_d[..., 3] = np.maximum(0.0, sm[..., 2] - sm[..., 0] ** 2)
        sc_i[..., 3] = np.maximum(0.0, sm[..., 3] - sm[..., 1] ** 2)
        return np.where(young[..., None], sc_d, d_in), np.where(young[..., None], sc_i, i_in)

    def _atrous(self, normal, depth, d_in, i_in, d_out, i_out, step):
        """One pass; sky pixels are not written (the output keeps what it held)."""
        c, W, H = self.cfg, self.w, self.h
        x, y = self._grid()
        real = (x < W) & (depth != 0)
        vb_d, vb_i = np.zeros((H, self.p)), np.zeros((H, self.p))
        for j in (-1, 0, 1):
            for ii in (-1, 0, 1):
                k = (0.5 if ii == 0 else 0.25) * (0.5 if j == 0 else 0.25)   # 1-2-1 x 1-2-1 / 16
                tx, ty = np.clip(x + ii, 0, W - 1), np.clip(y + j, 0, H - 1)
                vb_d += k * d_in[ty, tx, 3]
                vb_i += k * i_in[ty, tx, 3]
        denom_d = 1.0 / np.sqrt(c.sigma_l * c.sigma_l * np.maximum(0.0, vb_d) + EPSILON)
        denom_i = 1.0 / np.sqrt(c.sigma_l * c.sigma_l * np.maximum(0.0, vb_i) + EPSILON)
        cl_d, cl_i = luminance(d_in), luminance(i_in)
        gx, gy = self._depth_gradient(depth, x, y)
        sw_d, sw_i = np.ones((H, self.p)), np.ones((H, self.p))
        sc_d, sc_i = d_in.copy(), i_in.copy()
        for j in (-1, 0, 1):
            for ii in (-1, 0, 1):
                if ii == 0 and j == 0:
                    continue
                tx, ty = x + ii * step, y + j * step
                ok = self._inside(tx, ty)
                td, ti = self._at(d_in, tx, ty), self._at(i_in, tx, ty)
                wd, wi = self._weights(ii * step, j * step, gx, gy, depth, self._at(depth, tx, ty), normal, self._at(normal, tx, ty),
                                       cl_d, cl_i, luminance(td), luminance(ti), denom_d, denom_i)
                wd, wi = np.where(ok, wd, 0.0), np.where(ok, wi, 0.0)
                sw_d += wd
                sw_i += wi
                sc_d += np.stack([wd, wd, wd, wd * wd], axis=-1) * td
                sc_i += np.stack([wi, wi, wi, wi * wi], axis=-1) * ti
        sc_d /= np.stack([sw_d, sw_d, sw_d, sw_d ** 2], axis=-1)
        sc_i /= np.stack([sw_i, sw_i, sw_i, sw_i ** 2], axis=-1)
        r = real[..., None]
        if step == 1 << FEEDBACK_ITERATION:
            self.history_direct = np.where(r, sc_d, self.history_direct)
            self.history_indirect = np.where(r, sc_i, self.history_indirect)
        return np.where(r, sc_d, d_out), np.where(r, sc_i, i_out)

    def _finalize(self, direct, indirect, albedo, normal_and_depth):
        c = self.cfg
        x, _ = self._grid()
        cols = (x < self.w)[..., None]
        colour = (direct + indirect) * albedo
        self.final = np.where(cols, colour, self.final)
        if c.enable_taa:
            t = colour / (1.0 + luminance(colour))[..., None]
            t[..., :3] = np.sqrt(np.maximum(0.0, t[..., :3]))
            self.taa_curr = np.where(cols, t, self.taa_curr)
        if c.num_atrous_iterations <= FEEDBACK_ITERATION:
            self.history_direct = np.where(cols, direct, self.history_direct)
            self.history_indirect = np.where(cols, indirect, self.history_indirect)
        self.history_moment = np.where(cols, self.moment, self.history_moment)
        self.history_normal_and_depth = np.where(cols, normal_and_depth, self.history_normal_and_depth).astype(F32)

    def _taa(self, sp, sample_index):
        W, H, P = self.w, self.h, self.p
        x, y = self._grid()
        cols = x < W
        colour = self.taa_curr.copy()
        if sample_index != 0:
            s_prev = (F32(0.5) + F32(0.5) * sp[..., 0]) * F32(W)
            t_prev = (F32(0.5) + F32(0.5) * sp[..., 1]) * F32(H)
            x_prev = np.trunc(s_prev + F32(0.5)).astype(np.int64)
            y_prev = np.trunc(t_prev + F32(0.5)).astype(np.int64)
            sum32 = np.zeros((H, P), F32)
            sum_w = np.zeros((H, P))
            acc = np.zeros((H, P, 4))
            carried = {r: np.zeros((H, P)) for r in self.rhos}
            for j in range(-2, 2):
                for ii in range(-2, 2):
                    tx, ty = x_prev + ii, y_prev + j
                    ok = self._inside(tx, ty)
                    ax32 = (tx.astype(F32) + F32(0.5)) - s_prev
                    ay32 = (ty.astype(F32) + F32(0.5)) - t_prev
                    w32 = mitchell_netravali32(ax32) * mitchell_netravali32(ay32)
                    sum32 = np.where(ok, sum32 + w32, sum32)
                    w = mitchell_netravali64(tx + 0.5 - s_prev.astype(np.float64), ax32) * mitchell_netravali64(ty + 0.5 - t_prev.astype(np.float64), ay32)
                    w = np.where(ok, w, 0.0)
                    sum_w += w
                    for r in self.rhos:
                        carried[r] += np.abs(w) * self._at(self._slack[r], tx, ty)
                    acc += w[..., None] * self._at(self.taa_prev, tx, ty)
            resolve = sum32 > 0
            curr = rgb_to_ycocg(colour)
            prev = rgb_to_ycocg(acc / np.where(resolve, sum_w, 1.0)[..., None])
            avg, var = np.zeros((H, P, 3)), np.zeros((H, P, 3))
            for j in (-1, 0, 1):
                for ii in (-1, 0, 1):
                    ok = self._inside(x + ii, y + j)
                    cc = rgb_to_ycocg(self._at(self.taa_curr, x + ii, y + j))
                    avg += ok[..., None] * cc
                    var += ok[..., None] * cc * cc
            avg /= 9.0
            var /= 9.0
            sigma = np.sqrt(np.maximum(0.0, var - avg * avg))
            lo, hi = avg - 1.25 * sigma, avg + 1.25 * sigma
            prev_unclamped = prev
            prev = np.clip(prev, lo, hi)
            t = f32c(0.1)
            integrated = ycocg_to_rgb((1 - t) * prev + t * curr)
            colour[..., :3] = np.where(resolve[..., None], integrated, colour[..., :3])
            active = resolve & cols
            for r in self.rhos:
                moved = (1.0 - t) * carried[r] / np.where(resolve, np.abs(sum_w), 1.0)
                self._slack[r] = np.where(active, moved + self._clamp_slack(r, prev_unclamped, avg, var, sigma, lo, hi), 0.0)
        else:
            for r in self.rhos:
                self._slack[r] = np.zeros((H, P))
        self.taa_prev = np.where(cols[..., None], colour, self.taa_prev)
        sq = colour * colour
        self.final = np.where(cols[..., None], sq / (1.0 - luminance(sq))[..., None], self.final)

    @staticmethod
    def _clamp_slack(rho, prev, avg, var, sigma, lo, hi):
        d_sigma2 = 2.0 * rho * (var + avg * avg)
        d_sigma = np.where(sigma * sigma > d_sigma2, d_sigma2 / (2.0 * np.maximum(sigma, 1e-30)), np.sqrt(d_sigma2))
        d_bound = 1.25 * d_sigma + rho * np.abs(avg)
        near = (prev <= lo + d_bound) | (prev >= hi - d_bound)
        return (1.0 - f32c(0.1)) * np.sum(np.where(near, d_bound, 0.0), axis=-1)

    def taa_slack(self, rho=None):
        """How far the TAA outputs of the last frame may move, per pixel, when the colours the resolves of this and the earlier
        frames read carry a relative error rho: (resolved colour, displayed colour), largest over the RGB channels.

        The YCoCg clamp is the one ill-conditioned step of the stage. sigma^2 = E[c^2] - E[c]^2 over nine colours of a filtered,
        smooth neighbourhood cancels: an error of rho in the colours moves it by about 2 rho (E[c^2] + E[c]^2), the bound
        avg +- 1.25 sigma by that over 2 sigma. Where the history lies outside a bound, or that close to it, the move passes into
        the resolved colour (times 0.9, the blend) -- and with the resolved colour into the history of the frames after it
        (0.9 x the Mitchell-Netravali average of the slack of the taps, in |weight|), and through the undone tone mapping
        q / (1 - L(q)), q = colour^2, into the displayed colour. rho = TAA_ROUNDING (None) states the kernels' own float32
        rounding; the rest of the stage agrees with float64 to a few ulps."""
        slack = self._slack[TAA_ROUNDING if rho is None else rho]
        colour = self.taa_prev[..., :3]
        sq = colour * colour
        one_minus_l = 1.0 - luminance(sq)
        dq = 2.0 * np.max(np.abs(colour), axis=-1) * slack
        return slack, dq / one_minus_l + np.max(sq, axis=-1) * dq / one_minus_l ** 2

    def frame(self, inputs, sample_index):
        """One filtered frame. `inputs`: what a frame's path tracing leaves for the filter, (height, pitch, C) float32 arrays
        `direct`, `indirect`, `albedo`, `normal_and_depth` (octahedral normal, depth, previous depth) and `screen_position_prev`."""
        c = self.cfg
        nd = np.asarray(inputs["normal_and_depth"], F32)
        sp = np.asarray(inputs["screen_position_prev"], F32)
        normal32 = oct_decode32(nd[..., :2])
        depth32 = nd[..., 2]
        self.fb_d = np.asarray(inputs["direct"], F32).astype(np.float64)
        self.fb_i = np.asarray(inputs["indirect"], F32).astype(np.float64)
        albedo = np.asarray(inputs["albedo"], F32).astype(np.float64)

        self._reproject(normal32, depth32, nd[..., 3], sp)
        normal, depth = normal32.astype(np.float64), depth32.astype(np.float64)
        d_in, i_in, d_out, i_out = self.fb_d, self.fb_i, self.acc_d, self.acc_i
        names = ["fb", "acc"]
        if c.enable_spatial_variance:
            d_out, i_out = self._variance(normal, depth, d_in, i_in)
            d_in, i_in, d_out, i_out = d_out, i_out, d_in, i_in
            names.reverse()
        for k in range(c.num_atrous_iterations):
            d_out, i_out = self._atrous(normal, depth, d_in, i_in, d_out, i_out, 1 << k)
            d_in, i_in, d_out, i_out = d_out, i_out, d_in, i_in
            names.reverse()
        # where the pair now lives: the accumulators persist into the next frame, the per-frame images are cleared
        pair = {names[0]: (d_in, i_in), names[1]: (d_out, i_out)}
        self.acc_d, self.acc_i = pair["acc"]
        self._finalize(d_in, i_in, albedo, nd)
        if c.enable_taa:
            self._taa(sp, sample_index)
        self.fb_d = np.zeros_like(self.fb_d)
        self.fb_i = np.zeros_like(self.fb_i)
