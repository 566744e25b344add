"""Float64 reference of the four BSDFs of the shade kernels, for the BSDF tests.

Written from the BSDF model the reference renderer defines (its BSDF.h, Material.h, KullaConty.h:12-81 and Sampling.h): it
reads and calls no product or oracle code, so a misreading that the kernel and the oracle share shows up here.

* Fresnel: the dielectric one with total internal reflection when eta^2 (1 - cos^2) >= 1; the conductor one of the
  reference (s and p terms of a^2 + b^2); the average-Fresnel fits of both.
* GGX: D (0 for m.z < 1e-6), Lambda, G1 = 1 / (1 + Lambda), the height-correlated G2 = 1 / (1 + Lambda_o + Lambda_i), 0
  when either direction lies on the back of m. alpha = max(1e-6, roughness^2).
* Warps: the concentric disk (which returns r (sin phi, cos phi)), the cosine hemisphere on it, Heitz's VNDF sampler with
  its blend weight 0.5 + 0.5 v.z and the axis (1, 0, 0) at normal incidence.
* Kulla-Conty: the multiscatter lobe (1 - E_i)(1 - E_o) / max(1e-4, pi (1 - E_avg)), the reciprocity factor, the
  multiscatter Fresnel; IORs remapped from [1.0001, 2.5] to [0, 1] for the dielectric tables.
* The four BSDFs' eval and sample, working from given uniforms (the DIM_BSDF_0 and DIM_BSDF_1 pairs of the probe).

Contract, as in texture_reference.py and svgf_reference.py: every function here is run twice. The first run is a float32
replay (numpy float32 does exactly the IEEE operations of the kernel, which builds with -ffp-contract=off; the LUT lerp is
emulated as the fused multiply-add it is; sin and cos are numpy's, a few ulp from the kernel's). It records every
decision -- the branch comparisons r < F_i, r < E_i, r0.y < F, r0.y > ratio, the hemisphere and back-facing checks,
pdf_is_valid, total internal reflection -- and every LUT coordinate. The second run is float64 and takes those recorded
decisions and coordinates instead of forming its own, so it follows the kernel's branch, and interpolates the same LUT
arrays in float64. The tangent frame of the normal, omega_i and the eval's omega_o are part of the probe and are formed in float32 too.
"""
import numpy as np

F32, F64 = np.float32, np.float64

DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR = 1, 2, 3, 4
ROUGHNESS_CUTOFF = F32(0.05)
LUT_MIN_IOR, LUT_MAX_IOR = F32(1.0001), F32(2.5)
PLASTIC_IOR = 1.5
PMJ_SAMPLES = 4096   # sample indices at or above this take the hashed path of the random numbers
NEAR_RELATIVE = 2e-6   # a threshold comparison closer than this (relative) may go either way between two float32 builds

# the 24-float probe record of rt_bsdf_eval / rt_bsdf_sample
MATERIAL, NORMAL, DIRECTION, ENTERING, TO_LIGHT, COS_O, KEY = slice(0, 8), slice(8, 11), slice(11, 14), 14, slice(15, 18), 18, slice(19, 22)


class Run:
    """One of the two runs: dtype F32 (the replay: records) or F64 (follows the replay's record)."""

    def __init__(self, dtype, record=None):
        self.t = dtype
        self.replay = record is None
        self.record = [] if record is None else record
        self.i = 0
        self.near = None   # per probe: some recorded threshold comparison was within NEAR_RELATIVE (replay only)
        self.PI = F32(3.14159265359) if self.replay else np.pi
        self.INV_PI = F32(0.31830988618) if self.replay else 1.0 / np.pi

    def c(self, x):
        return self.t(x)

    def _take(self, value):
        if self.replay:
            self.record.append(value)
            return value
        v = self.record[self.i]
        self.i += 1
        return v

    def decide(self, cond):
        return self._take(np.asarray(cond, bool))

    def coord(self, x):
        """A value the kernel forms in float32 and looks a table up with: the replay's, in either run."""
        return self._take(np.asarray(x, F32))

    def less(self, a, b):
        """a < b where a or b carries float32 rounding of a direction: records how close the comparison was."""
        if self.replay:
            close = np.abs(a - b) <= NEAR_RELATIVE * np.maximum(np.abs(a), np.abs(b))
            self.near = close if self.near is None else (self.near | close)
        return self.decide(a < b)

    def valid(self, pdf):   # pdf_is_valid (Sampling.h:18-20)
        if self.replay:
            close = np.abs(pdf - F32(1e-4)) <= NEAR_RELATIVE * 1e-4
            self.near = close if self.near is None else (self.near | close)
        return self.decide(np.isfinite(pdf) & (pdf > self.c(1e-4)))


# ---- vectors: tuples of three arrays ----------------------------------------------------------------------------------

def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def scale(s, a):
    return (s * a[0], s * a[1], s * a[2])


def neg(a):
    return (-a[0], -a[1], -a[2])


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def normalize(R, a):
    inv = R.c(1) / np.sqrt(dot(a, a))
    return scale(inv, a)


def where(cond, a, b):
    return tuple(np.where(cond, x, y) for x, y in zip(a, b))


def safe_sqrt(R, x):
    return np.sqrt(np.maximum(R.c(0), x))


def lerp(R, a, b, t):
    return (R.c(1) - t) * a + t * b


def orthonormal_basis(n):
    """The tangent frame of the shading normal, in float32 (part of the probe)."""
    n = [np.asarray(x, F32) for x in n]
    sign = np.copysign(F32(1), n[2])
    a = F32(-1) / (sign + n[2])
    b = n[0] * n[1] * a
    tangent = (F32(1) + sign * n[0] * n[0] * a, sign * b, -sign * n[0])
    bitangent = (b, sign + n[1] * n[1] * a, -n[1])
    return tangent, bitangent, tuple(n)


def world_to_local(v, t, b, n):
    return (dot(t, v), dot(b, v), dot(n, v))


def local_to_world(v, t, b, n):
    return tuple(t[k] * v[0] + b[k] * v[1] + n[k] * v[2] for k in range(3))


def reflect(R, d, n):
    return add(scale(R.c(2) * dot(d, n), n), neg(d))


def refract(R, d, n, eta):
    cos_theta = dot(d, n)
    k = R.c(1) - eta * eta * (R.c(1) - cos_theta * cos_theta)
    return add(scale(eta * cos_theta - safe_sqrt(R, k), n), neg(scale(eta, d)))


# ---- Fresnel, GGX -----------------------------------------------------------------------------------------------------

def fresnel_dielectric(R, cos_i, eta):
    sin2 = eta * eta * (R.c(1) - cos_i * cos_i)
    tir = R.decide(sin2 >= R.c(1))
    cos_o = safe_sqrt(R, R.c(1) - sin2)
    p = (eta * cos_i - cos_o) / (eta * cos_i + cos_o)
    s = (cos_i - eta * cos_o) / (cos_i + eta * cos_o)
    return np.where(tir, R.c(1), R.c(0.5) * (p * p + s * s))


def fresnel_conductor(R, cos_i, eta, k):
    c2 = cos_i * cos_i
    s2i = R.c(1) - c2
    out = []
    for e, kk in zip(eta, k):
        inner = e * e - kk * kk - s2i
        a2b2 = safe_sqrt(R, inner * inner + R.c(4) * kk * kk * e * e)
        a = safe_sqrt(R, R.c(0.5) * (a2b2 + inner))
        s2 = (a2b2 + c2 - R.c(2) * a * cos_i) / (a2b2 + c2 + R.c(2) * a * cos_i)
        x, y = a2b2 * c2 + s2i * s2i, R.c(2) * a * cos_i * s2i
        p2 = (x - y) / (x + y) * s2
        out.append(R.c(0.5) * (p2 + s2))
    return tuple(out)


def average_fresnel_dielectric(R, ior):
    return (ior - R.c(1)) / (R.c(4.08567) + R.c(1.00071) * ior)


def average_fresnel_conductor(R, eta, k):
    c = R.c
    out = []
    for e, kk in zip(eta, k):
        num = e * (c(133.736) - c(98.9833) * e) + kk * (e * (c(59.5617) - c(3.98288) * e) - c(182.37)) + ((c(0.30818) * e - c(13.1093)) * e - c(62.5919)) * kk * kk - c(8.21474)
        den = kk * (e * (c(94.6517) - c(15.8558) * e) - c(187.166)) + (c(-78.476) * e - c(395.268)) * e + (e * (e - c(15.4387)) - c(62.0752)) * kk * kk
        out.append(num / den)
    return tuple(out)


def roughness_to_alpha(R, r):
    return np.maximum(R.c(1e-6), r * r)


def ggx_D(R, m, a):
    flat = R.decide(m[2] < R.c(1e-6))
    sx, sy = -m[0] / (m[2] * a), -m[1] / (m[2] * a)
    sl = R.c(1) + sx * sx + sy * sy
    c2 = m[2] * m[2]
    return np.where(flat, R.c(0), R.c(1) / (sl * sl * R.PI * a * a * (c2 * c2)))


def ggx_lambda(R, w, a):
    return R.c(0.5) * (np.sqrt(R.c(1) + ((a * w[0]) ** 2 + (a * w[1]) ** 2) / (w[2] * w[2])) - R.c(1))


def ggx_G1(R, w, a):
    return R.c(1) / (R.c(1) + ggx_lambda(R, w, a))


def ggx_G2(R, wo, wi, wm, a):
    i_back = R.decide(dot(wi, wm) * wi[2] <= R.c(0))
    o_back = R.decide(dot(wo, wm) * wo[2] <= R.c(0))
    return np.where(i_back | o_back, R.c(0), R.c(1) / (R.c(1) + ggx_lambda(R, wo, a) + ggx_lambda(R, wi, a)))


# ---- warps --------------------------------------------------------------------------------------------------------------

def sample_disk(R, u1, u2):
    a = R.c(2) * u1 - R.c(1)
    b = R.c(2) * u2 - R.c(1)
    first = R.decide(a * a > b * b)
    r = np.where(first, a, b)
    phi = np.where(first, R.c(0.25) * R.PI * (b / a), R.c(0.5) * R.PI - R.c(0.25) * R.PI * (a / b))
    return r * np.sin(phi), r * np.cos(phi)


def sample_cosine(R, u1, u2):
    x, y = sample_disk(R, u1, u2)
    return (x, y, safe_sqrt(R, R.c(1) - (x * x + y * y)))


def sample_vndf(R, omega, a, u1, u2):
    v = normalize(R, (a * omega[0], a * omega[1], omega[2]))
    ls = v[0] * v[0] + v[1] * v[1]
    tilted = R.decide(ls > R.c(0))
    inv = np.where(tilted, R.c(1) / np.sqrt(np.where(tilted, ls, R.c(1))), R.c(0))
    axis_1 = where(tilted, (-v[1] * inv, v[0] * inv, R.c(0) * inv), (R.c(1) + 0 * inv, 0 * inv, 0 * inv))
    axis_2 = cross(v, axis_1)
    t1, d_y = sample_disk(R, u1, u2)
    t2 = lerp(R, safe_sqrt(R, R.c(1) - t1 * t1), d_y, R.c(0.5) + R.c(0.5) * v[2])
    n_h = add(add(scale(t1, axis_1), scale(t2, axis_2)), scale(safe_sqrt(R, R.c(1) - t1 * t1 - t2 * t2), v))
    return normalize(R, (a * n_h[0], a * n_h[1], n_h[2]))


def sample_pdf_cosine(R, omega_o):
    return omega_o[2] * R.INV_PI


# ---- Kulla-Conty tables ------------------------------------------------------------------------------------------------

def _taps(coord, n):
    """Clamp-addressed texel positions, formed in float32: x = s n - 0.5."""
    x = np.asarray(coord, F32) * F32(n) - F32(0.5)
    x0 = np.floor(x)
    f = x - x0
    i0 = np.clip(x0.astype(np.int64), 0, n - 1)
    i1 = np.clip(x0.astype(np.int64) + 1, 0, n - 1)
    return i0, i1, f


def _lerp_table(R, a, b, f):
    if R.replay:   # lerpf = fmaf(t, b - a, a): one rounding (a float32 product is exact in float64)
        return (f.astype(F64) * (b - a).astype(F64) + a.astype(F64)).astype(F32)
    return a.astype(F64) + f.astype(F64) * (b.astype(F64) - a.astype(F64))


def lut_2d(R, table, nx, ny, s, t):
    x0, x1, fx = _taps(s, nx)
    y0, y1, fy = _taps(t, ny)
    table = np.asarray(table, F32).reshape(-1)
    r0 = _lerp_table(R, table[x0 + y0 * nx], table[x1 + y0 * nx], fx)
    r1 = _lerp_table(R, table[x0 + y1 * nx], table[x1 + y1 * nx], fx)
    return _lerp_table(R, r0, r1, fy)


def lut_3d(R, table, s, t, r):
    z0, z1, fz = _taps(r, 16)
    table = np.asarray(table, F32).reshape(16, 256)
    lo = _lut_2d_rows(R, table[z0], s, t)
    hi = _lut_2d_rows(R, table[z1], s, t)
    return _lerp_table(R, lo, hi, fz)


def _lut_2d_rows(R, rows, s, t):
    x0, x1, fx = _taps(s, 16)
    y0, y1, fy = _taps(t, 16)
    g = lambda x, y: np.take_along_axis(rows, (x + 16 * y)[:, None], axis=1)[:, 0]
    r0 = _lerp_table(R, g(x0, y0), g(x1, y0), fx)
    r1 = _lerp_table(R, g(x0, y1), g(x1, y1), fx)
    return _lerp_table(R, r0, r1, fy)


def remap_ior(ior):
    ior = np.asarray(ior, F32)
    return F32(0) + (ior - LUT_MIN_IOR) / (LUT_MAX_IOR - LUT_MIN_IOR) * F32(1)


class Tables:
    """The six Kulla-Conty tables (the device's or the oracle's): directional enter / leave 16^3, average enter / leave 16^2,
    conductor directional 32^2, conductor average 32."""

    def __init__(self, luts):
        self.dir_enter, self.dir_leave, self.avg_enter, self.avg_leave, self.cond_dir, self.cond_avg = [np.asarray(l, F32).reshape(-1) for l in luts]

    def dielectric_directional(self, R, ior, rough, cos, entering):
        ior_c, rough_c, cos_c = R.coord(remap_ior(ior)), R.coord(rough), R.coord(np.abs(np.asarray(cos, F32)))
        enter = lut_3d(R, self.dir_enter, ior_c, rough_c, cos_c)
        leave = lut_3d(R, self.dir_leave, ior_c, rough_c, cos_c)
        return np.where(entering, enter, leave)

    def dielectric_average(self, R, ior, rough, entering):
        ior_c, rough_c = R.coord(remap_ior(ior)), R.coord(rough)
        return lut_2d(R, self.avg_enter if entering else self.avg_leave, 16, 16, ior_c, rough_c)

    def conductor_directional(self, R, rough, cos):
        return lut_2d(R, self.cond_dir, 32, 32, R.coord(rough), R.coord(np.abs(np.asarray(cos, F32))))

    def conductor_average(self, R, rough):
        x0, x1, f = _taps(R.coord(rough), 32)
        return _lerp_table(R, self.cond_avg[x0], self.cond_avg[x1], f)


def multiscatter_lobe(R, E_i, E_o, E_avg):
    return (R.c(1) - E_i) * (R.c(1) - E_o) / np.maximum(R.c(1e-4), R.PI * (R.c(1) - E_avg))


def reciprocity_factor(R, E_avg_enter, E_avg_leave):
    return (R.c(1) - E_avg_leave) / np.maximum(R.c(1e-4), R.c(2) - E_avg_enter - E_avg_leave)


def fresnel_multiscatter(R, F_avg, E_avg):
    return tuple(F * F * E_avg / (R.c(1) - F * (R.c(1) - E_avg)) for F in F_avg)


# ---- the four BSDFs -----------------------------------------------------------------------------------------------------

class Result:
    """ok: 1, 0, or -1 (refused: omega_i.z <= 0); pdf; value: the bsdf (eval) or the throughput factor (sample), (N, 3);
    direction (N, 3); medium; allow_nee; omega_i_z; near: a threshold comparison of the replay lay within NEAR_RELATIVE."""


def _setup(R, probes):
    p = np.asarray(probes, F32)
    t, b, n = orthonormal_basis((p[:, 8], p[:, 9], p[:, 10]))
    d = (p[:, 11], p[:, 12], p[:, 13])
    if not R.replay:
        t, b, n = [tuple(x.astype(F64) for x in v) for v in (t, b, n)]
        d = tuple(x.astype(F64) for x in d)
    omega_i = _local(R, neg(d), (t, b, n))
    m = p[:, MATERIAL] if R.replay else p[:, MATERIAL].astype(F64)
    return p, m, (t, b, n), omega_i


def _local(R, v, frame):
    """omega_i and the eval's omega_o, formed in float32 as the kernel forms them: at normal incidence the VNDF sampler's
    azimuth follows the rounding residue of omega_i.xy, which a float64 frame would not reproduce."""
    w = tuple(R.coord(x) for x in world_to_local(v, *frame))
    return w if R.replay else tuple(x.astype(F64) for x in w)


def _vec(R, p, sl):
    return tuple(p[:, k] if R.replay else p[:, k].astype(F64) for k in range(sl.start, sl.stop))


def _diffuse(R, p, m, frame, omega_i, eval, U):
    albedo = (m[:, 0], m[:, 1], m[:, 2])
    n = p.shape[0]
    if eval:
        cos_o = p[:, COS_O] if R.replay else p[:, COS_O].astype(F64)
        up = ~R.decide(p[:, COS_O] <= 0)
        pdf = cos_o * R.INV_PI
        value = (cos_o * R.INV_PI,) * 3
        ok = up & R.valid(pdf)
        return ok, np.where(up, pdf, 0), tuple(np.where(up, v, 0) for v in value), _vec(R, p, TO_LIGHT), np.full(n, -1), np.ones(n, bool)
    r = U[0]
    omega_o = sample_cosine(R, r[:, 0], r[:, 1])
    pdf = omega_o[2] * R.INV_PI
    return R.valid(pdf), pdf, albedo, local_to_world(omega_o, *frame), np.full(n, -1), np.ones(n, bool)


def _plastic_parts(R, m, omega_i, omega_o, omega_m, F_i, G1_i, a):
    eta = R.c(1) / R.c(PLASTIC_IOR)
    albedo = (m[:, 0], m[:, 1], m[:, 2])
    F = fresnel_dielectric(R, dot(omega_i, omega_m), eta)
    D = ggx_D(R, omega_m, a)
    G2 = ggx_G2(R, omega_o, omega_i, omega_m, a)
    spec = F * G2 * D / (R.c(4) * omega_i[2])
    F_o = fresnel_dielectric(R, omega_o[2], eta)
    F_avg = average_fresnel_dielectric(R, R.c(PLASTIC_IOR))
    isf = R.c(1) - (R.c(1) - F_avg) * (eta * eta)
    diff = tuple(eta * eta * (R.c(1) - F_i) * (R.c(1) - F_o) * al * R.INV_PI / (R.c(1) - al * isf) * omega_o[2] for al in albedo)
    pdf_spec = G1_i * D / (R.c(4) * omega_i[2])
    pdf_diff = omega_o[2] * R.INV_PI
    pdf = lerp(R, pdf_diff, pdf_spec, F_i)
    return tuple(spec + d for d in diff), pdf


def _plastic(R, p, m, frame, omega_i, eval, U):
    n = p.shape[0]
    a = roughness_to_alpha(R, m[:, 4])
    eta = R.c(1) / R.c(PLASTIC_IOR)
    F_i = fresnel_dielectric(R, omega_i[2], eta)
    G1_i = ggx_G1(R, omega_i, a)
    if eval:
        up = ~R.decide(p[:, COS_O] <= 0)
        to_light = _vec(R, p, TO_LIGHT)
        omega_o = _local(R, to_light, frame)
        omega_m = normalize(R, add(omega_i, omega_o))
        bsdf, pdf = _plastic_parts(R, m, omega_i, omega_o, omega_m, F_i, G1_i, a)
        ok = up & R.valid(pdf)
        return ok, np.where(up, pdf, 0), tuple(np.where(up, v, 0) for v in bsdf), to_light, np.full(n, -1), np.ones(n, bool)
    r_fresnel, r_brdf = U[0][:, 0], U[1]
    specular = R.less(r_fresnel, F_i)
    m_vndf = sample_vndf(R, omega_i, a, r_brdf[:, 0], r_brdf[:, 1])
    o_vndf = reflect(R, omega_i, m_vndf)
    o_cos = sample_cosine(R, r_brdf[:, 0], r_brdf[:, 1])
    m_cos = normalize(R, add(omega_i, o_cos))
    omega_m, omega_o = where(specular, m_vndf, m_cos), where(specular, o_vndf, o_cos)
    below = R.decide(omega_m[2] < 0)
    bsdf, pdf = _plastic_parts(R, m, omega_i, omega_o, omega_m, F_i, G1_i, a)
    ok = ~below & R.valid(pdf)
    return ok, np.where(below, 0, pdf), tuple(np.where(below, 1, v / pdf) for v in bsdf), local_to_world(omega_o, *frame), np.full(n, -1), np.ones(n, bool)


def _dielectric_common(R, T, ior, rough, eta, omega_i):
    entering = R.decide(eta < R.c(1))
    E_i = T.dielectric_directional(R, ior, rough, omega_i[2], entering)
    F_avg = average_fresnel_dielectric(R, ior)
    F_avg = np.where(entering, F_avg, R.c(1) - (R.c(1) - F_avg) / (ior * ior))
    E_enter = T.dielectric_average(R, ior, rough, True)
    E_leave = T.dielectric_average(R, ior, rough, False)
    x = reciprocity_factor(R, E_enter, E_leave)
    ratio = np.where(entering, x, R.c(1) - x) * (R.c(1) - F_avg)
    return entering, E_i, ratio, E_enter, E_leave


def _dielectric_lobes(R, T, ior, rough, eta, reflected, entering, omega_i, omega_o, omega_m, F, E_i, ratio, E_enter, E_leave):
    a = roughness_to_alpha(R, rough)
    D = ggx_D(R, omega_m, a)
    G1 = ggx_G1(R, omega_i, a)
    G2 = ggx_G2(R, omega_o, omega_i, omega_m, a)
    i_m, o_m = np.abs(dot(omega_i, omega_m)), np.abs(dot(omega_o, omega_m))
    # reflection
    E_o_r = T.dielectric_directional(R, ior, rough, omega_o[2], entering)
    single_r = F * G2 * D / (R.c(4) * omega_i[2])
    pdf_single_r = F * G1 * D / (R.c(4) * omega_i[2])
    multi_r = (R.c(1) - ratio) * np.abs(omega_o[2]) * multiscatter_lobe(R, E_i, E_o_r, np.where(entering, E_enter, E_leave))
    pdf_multi_r = (R.c(1) - ratio) * np.abs(omega_o[2]) * R.INV_PI
    # transmission: E_avg of the other side on purpose (BSDF.h:281)
    E_o_t = T.dielectric_directional(R, ior, rough, omega_o[2], ~entering)
    denom = (eta * i_m + o_m) ** 2
    single_t = (R.c(1) - F) * G2 * D * i_m * o_m / (omega_i[2] * denom * (eta * eta))
    pdf_single_t = (R.c(1) - F) * G1 * D * i_m * o_m / (omega_i[2] * denom)
    multi_t = ratio * np.abs(omega_o[2]) * multiscatter_lobe(R, E_i, E_o_t, np.where(entering, E_leave, E_enter))
    pdf_multi_t = ratio * np.abs(omega_o[2]) * R.INV_PI
    single, multi = np.where(reflected, single_r, single_t), np.where(reflected, multi_r, multi_t)
    pdf = lerp(R, np.where(reflected, pdf_multi_r, pdf_multi_t), np.where(reflected, pdf_single_r, pdf_single_t), E_i)
    return single + multi, pdf


def _flip_up(R, m):
    down = R.decide(np.signbit(m[2]))
    return where(down, neg(m), m)


def _dielectric(R, T, p, m, frame, omega_i, eval, U):
    n = p.shape[0]
    medium_material = p[:, 0].view(np.int32)
    ior, rough = m[:, 1], m[:, 2]
    eta = np.where(p[:, ENTERING] != 0, R.c(1) / ior, ior)
    allow = R.decide(p[:, 2] >= ROUGHNESS_CUTOFF)
    if eval:
        to_light = _vec(R, p, TO_LIGHT)
        omega_o = _local(R, to_light, frame)
        reflected = R.decide(omega_o[2] >= 0)
        omega_m = where(reflected, normalize(R, add(omega_i, omega_o)), normalize(R, add(scale(eta, omega_i), omega_o)))
        omega_m = _flip_up(R, omega_m)
        F = fresnel_dielectric(R, np.abs(dot(omega_i, omega_m)), eta)
        entering, E_i, ratio, E_enter, E_leave = _dielectric_common(R, T, ior, rough, eta, omega_i)
        bsdf, pdf = _dielectric_lobes(R, T, ior, rough, eta, reflected, entering, omega_i, omega_o, omega_m, F, E_i, ratio, E_enter, E_leave)
        return R.valid(pdf), pdf, (bsdf,) * 3, to_light, np.full(n, -1), allow
    r0, r1 = U[0], U[1]
    a = roughness_to_alpha(R, rough)
    entering, E_i, ratio, E_enter, E_leave = _dielectric_common(R, T, ior, rough, eta, omega_i)
    single = R.less(r0[:, 0], E_i)
    # the single-scattering lobe: a visible normal, reflected with probability F
    m_v = sample_vndf(R, omega_i, a, r1[:, 0], r1[:, 1])
    F_v = fresnel_dielectric(R, np.abs(dot(omega_i, m_v)), eta)
    refl_v = R.less(r0[:, 1], F_v)
    o_v = where(refl_v, reflect(R, omega_i, m_v), refract(R, omega_i, m_v, eta))
    # the multiple-scattering lobe: a cosine direction, transmitted with probability ratio
    o_c = sample_cosine(R, r1[:, 0], r1[:, 1])
    refl_c = R.less(ratio, r0[:, 1])
    o_c = where(refl_c, o_c, neg(o_c))
    m_c = where(refl_c, normalize(R, add(omega_i, o_c)), normalize(R, add(scale(eta, omega_i), o_c)))
    m_c = _flip_up(R, m_c)
    F_c = fresnel_dielectric(R, np.abs(dot(omega_i, m_c)), eta)
    reflected = np.where(single, refl_v, refl_c)
    omega_o, omega_m, F = where(single, o_v, o_c), where(single, m_v, m_c), np.where(single, F_v, F_c)
    wrong_side = reflected ^ R.decide(omega_o[2] >= 0)
    bsdf, pdf = _dielectric_lobes(R, T, ior, rough, eta, reflected, entering, omega_i, omega_o, omega_m, F, E_i, ratio, E_enter, E_leave)
    medium = np.where(~reflected & entering, medium_material, -1)
    ok = ~wrong_side & R.valid(pdf)
    return ok, np.where(wrong_side, 0, pdf), (np.where(wrong_side, 1, bsdf / pdf),) * 3, local_to_world(omega_o, *frame), np.where(wrong_side, -1, medium), allow


def _conductor_lobes(R, T, eta, k, rough, omega_i, omega_o, omega_m, o_dot_m, E_i):
    a = roughness_to_alpha(R, rough)
    F = fresnel_conductor(R, o_dot_m, eta, k)
    D = ggx_D(R, omega_m, a)
    G1 = ggx_G1(R, omega_i, a)
    G2 = ggx_G2(R, omega_o, omega_i, omega_m, a)
    E_o = T.conductor_directional(R, rough, omega_o[2])
    E_avg = T.conductor_average(R, rough)
    F_ms = fresnel_multiscatter(R, average_fresnel_conductor(R, eta, k), E_avg)
    lobe = multiscatter_lobe(R, E_i, E_o, E_avg)
    brdf = tuple(Fc * G2 * D / (R.c(4) * omega_i[2]) + Fm * lobe * omega_o[2] for Fc, Fm in zip(F, F_ms))
    pdf = lerp(R, omega_o[2] * R.INV_PI, G1 * D / (R.c(4) * omega_i[2]), E_i)
    return brdf, pdf


def _conductor(R, T, p, m, frame, omega_i, eval, U):
    n = p.shape[0]
    eta, rough, k = (m[:, 0], m[:, 1], m[:, 2]), m[:, 3], (m[:, 4], m[:, 5], m[:, 6])
    allow = R.decide(p[:, 3] >= ROUGHNESS_CUTOFF)
    E_i = T.conductor_directional(R, rough, omega_i[2])
    if eval:
        up = ~R.decide(p[:, COS_O] <= 0)
        to_light = _vec(R, p, TO_LIGHT)
        omega_o = _local(R, to_light, frame)
        omega_m = normalize(R, add(omega_o, omega_i))
        o_dot_m = dot(omega_o, omega_m)
        front = up & ~R.decide(o_dot_m <= 0)
        brdf, pdf = _conductor_lobes(R, T, eta, k, rough, omega_i, omega_o, omega_m, o_dot_m, E_i)
        ok = front & R.valid(pdf)
        return ok, np.where(front, pdf, 0), tuple(np.where(front, v, 0) for v in brdf), to_light, np.full(n, -1), allow
    r0, r1 = U[0], U[1]
    a = roughness_to_alpha(R, rough)
    single = R.less(r0[:, 0], E_i)
    m_v = sample_vndf(R, omega_i, a, r1[:, 0], r1[:, 1])
    o_v = reflect(R, omega_i, m_v)
    o_c = sample_cosine(R, r1[:, 0], r1[:, 1])
    m_c = normalize(R, add(omega_i, o_c))
    omega_m, omega_o = where(single, m_v, m_c), where(single, o_v, o_c)
    o_dot_m = dot(omega_o, omega_m)
    fail = R.decide((o_dot_m <= 0) | (omega_o[2] < 0))
    brdf, pdf = _conductor_lobes(R, T, eta, k, rough, omega_i, omega_o, omega_m, o_dot_m, E_i)
    ok = ~fail & R.valid(pdf)
    return ok, np.where(fail, 0, pdf), tuple(np.where(fail, 1, v / pdf) for v in brdf), local_to_world(omega_o, *frame), np.full(n, -1), allow


def _run(R, material_type, probes, eval, U, T):
    p, m, frame, omega_i = _setup(R, probes)
    refused = R.decide(omega_i[2] <= 0)
    if material_type == DIFFUSE:
        out = _diffuse(R, p, m, frame, omega_i, eval, U)
    elif material_type == PLASTIC:
        out = _plastic(R, p, m, frame, omega_i, eval, U)
    elif material_type == DIELECTRIC:
        out = _dielectric(R, T, p, m, frame, omega_i, eval, U)
    elif material_type == CONDUCTOR:
        out = _conductor(R, T, p, m, frame, omega_i, eval, U)
    else:
        raise ValueError(material_type)
    ok, pdf, value, direction, medium, allow = out
    r = Result()
    r.ok = np.where(refused, -1, np.where(ok, 1, 0))
    r.pdf = np.where(refused, 0, np.asarray(pdf, F64))
    r.value = np.where(refused[:, None], 0, np.stack([np.broadcast_to(np.asarray(v, F64), pdf.shape) for v in value], axis=1))
    r.direction = np.where(refused[:, None], 0, np.stack([np.asarray(d, F64) for d in direction], axis=1))
    r.medium = np.where(refused, -1, medium)
    r.allow_nee = np.asarray(allow, bool)
    r.omega_i_z = np.asarray(omega_i[2], F64)
    return r


def evaluate(material_type, probes, tables=None, eval=True, uniforms=None):
    """The float64 result of rt_bsdf_eval (eval=True) or rt_bsdf_sample (eval=False) on (N, 24) probe records. uniforms: the
    DIM_BSDF_0 and DIM_BSDF_1 pairs of each probe's key, two (N, 2) float32 arrays (sample only). tables: Tables of the
    LUTs (dielectric and conductor). Returns (float64 Result, float32 replay Result); the float64 one carries `near`."""
    U = None if uniforms is None else [np.asarray(u, F32) for u in uniforms]
    with np.errstate(all="ignore"):
        replay = Run(F32)
        r32 = _run(replay, material_type, probes, eval, U, tables)
        n = np.asarray(probes).shape[0]
        U64 = None if U is None else [u.astype(F64) for u in U]
        r64 = _run(Run(F64, replay.record), material_type, probes, eval, U64, tables)
    r64.near = replay.near if replay.near is not None else np.zeros(n, bool)
    return r64, r32


# ---- the pdf over solid-angle bins, for the goodness-of-fit tests ---------------------------------------------------------

def bin_index(directions, n_z=16, n_phi=32):
    """Bin of each unit direction (local frame): n_z bands uniform in z per hemisphere (upper first), n_phi in phi."""
    d = np.asarray(directions, F64)
    z = np.clip(d[:, 2], -1.0, 1.0)
    phi = np.mod(np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi)
    upper = z >= 0
    band = np.where(upper, np.minimum((z * n_z).astype(np.int64), n_z - 1), n_z + np.minimum((-z * n_z).astype(np.int64), n_z - 1))
    return band * n_phi + np.minimum((phi / (2 * np.pi) * n_phi).astype(np.int64), n_phi - 1)


def pdf_quadrature(material_type, probe, tables, hemispheres=(True, False), n_z=16, n_phi=32, sub=8):
    """Expected fraction of samples per bin of bin_index: the float64 eval pdf integrated over each bin with sub x sub
    midpoints (dz dphi is the solid angle), 0 where the eval refuses the direction. probe: one 24-float record whose normal
    is +z, so the local frame is the world frame."""
    z_edges = (np.arange(n_z * sub) + 0.5) / (n_z * sub)
    phi_c = (np.arange(n_phi * sub) + 0.5) / (n_phi * sub) * 2 * np.pi
    out = np.zeros(2 * n_z * n_phi)
    for h, upper in enumerate((True, False)):
        if upper not in hemispheres:
            continue
        zz, pp = np.meshgrid(z_edges if upper else -z_edges, phi_c, indexing="ij")
        s = np.sqrt(np.maximum(0.0, 1 - zz * zz))
        dirs = np.stack([s * np.cos(pp), s * np.sin(pp), zz], axis=-1).reshape(-1, 3)
        probes = np.repeat(np.asarray(probe, F32)[None], dirs.shape[0], axis=0)
        probes[:, TO_LIGHT] = dirs
        probes[:, COS_O] = dirs[:, 2]
        r, _ = evaluate(material_type, probes, tables, eval=True)
        pdf = np.where(r.ok == 1, r.pdf, 0.0).reshape(n_z * sub, n_phi * sub)
        w = (1.0 / (n_z * sub)) * (2 * np.pi / (n_phi * sub))
        cells = (pdf * w).reshape(n_z, sub, n_phi, sub).sum(axis=(1, 3))
        out[h * n_z * n_phi:(h + 1) * n_z * n_phi] = cells.reshape(-1)
    return out


def chi2_test(observed_bins, other_count, expected_fraction, n, min_expected=5.0):
    """Pearson chi^2 of sample counts against n times the quadrature. Bins expecting fewer than min_expected samples are merged
    (by increasing expectation) into one; `other_count` (failed samples, invalid pdfs, directions outside the hemispheres the
    eval covers) is one more bin, expecting n (1 - sum). Returns (p-value, chi^2, degrees of freedom)."""
    from math import erf, sqrt
    exp = np.asarray(expected_fraction, F64) * n
    obs = np.asarray(observed_bins, F64)
    order = np.argsort(exp)
    small = exp[order] < min_expected
    e_list, o_list = list(exp[order][~small]), list(obs[order][~small])
    if small.any():
        e_list.append(exp[order][small].sum()); o_list.append(obs[order][small].sum())
    e_list.append(max(n - exp.sum(), 0.0)); o_list.append(float(other_count))
    e, o = np.array(e_list), np.array(o_list)
    keep = e > 0
    if (o[~keep] > 0).any():
        return 0.0, np.inf, int(keep.sum()) - 1
    chi2 = float(((o[keep] - e[keep]) ** 2 / e[keep]).sum())
    dof = int(keep.sum()) - 1
    # Wilson-Hilferty: chi^2 / dof is close to normal for the dof here (hundreds)
    z = ((chi2 / dof) ** (1 / 3) - (1 - 2 / (9 * dof))) / sqrt(2 / (9 * dof))
    return 0.5 * (1 - erf(z / sqrt(2))), chi2, dof
