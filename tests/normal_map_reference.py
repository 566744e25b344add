"""Float64 restatement of the tangent-space normal maps of DESIGN.md 7.2 (normal_map_perturb, rt_shading.h), probe by probe, in the
record layout of rt_perturb_normals (include/gpu_raytracer_amd.h), and the helpers the normal-map tests share: probe packing, an
uncompressed-TGA writer, and the decoded world normal of a constant map on an axis-aligned quad."""
import numpy as np

import texture_reference as tref

F32 = np.float32
PROBE_IN = 48
EPS = 1e-2   # RT_NORMAL_MAP_VIEW_EPSILON

# Tolerance against this file, per component of the unit result (test_gpu_normal_maps.py). The device's texel is within
# TEX_TOL of the float64 one (test_gpu_texture_unit.py: the fp32 lerp chain on RGBA8 inputs); t = 2c - 1 doubles it, and
# normalising a vector of length |t| divides it by |t|: 2 * TEX_TOL * sqrt(3) / |t|. The frame is a chain of about 40
# roundings (the barycentric normal, two 3 x 3 products, dp/du, one projection, two normalisations, a cross product), each
# 2^-24 relative, amplified by 1 / sin(dp/du, n) in the projection: FRAME_ULPS * 2^-24 / sin. Both grow by at most 1 / EPS
# where the view guard moves m (its correction divides by a length of at least EPS).
TEX_TOL = 1e-5
FRAME_ULPS = 64


def bound(t_length, sin_tn, guarded):
    b = 2.0 * TEX_TOL * np.sqrt(3.0) / t_length + FRAME_ULPS * 2.0 ** -24 / sin_tn
    return np.where(guarded, b / EPS, b)


def pack(p0, e1, e2, n0, ne1, ne2, uv0, uve1, uve2, u, v, world, direction, filter, lod=0.0, g1=(0.0, 0.0), g2=(0.0, 0.0)):
    r = np.zeros(PROBE_IN, F32)
    r[0:3], r[3:6], r[6:9], r[9:12], r[12:15], r[15:18] = p0, e1, e2, n0, ne1, ne2
    r[18:20], r[20:22], r[22:24] = uv0, uve1, uve2
    r[24], r[25] = u, v
    r[26:38] = np.asarray(world, F32).reshape(12)
    r[38:41] = direction
    r[41], r[42] = filter, lod
    r[43:45], r[45:47] = g1, g2
    return r


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def frame(rec):
    """Tangent frame of (N, 48) records in float64: n (interpolated world normal, before the side flip), T, B, det, sin(dp/du, n),
    entering, and whether the frame falls back (det 0 / not finite, dp/du along n)."""
    r = np.asarray(rec, np.float64).reshape(-1, PROBE_IN)
    e1, e2, n0, ne1, ne2 = r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12:15], r[:, 15:18]
    duv1, duv2, u, v = r[:, 20:22], r[:, 22:24], r[:, 24:25], r[:, 25:26]
    W = r[:, 26:38].reshape(-1, 3, 4)[:, :, :3]
    n = _normalize(np.einsum("nij,nj->ni", W, n0 + u * ne1 + v * ne2))
    det = duv1[:, 0] * duv2[:, 1] - duv2[:, 0] * duv1[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        dpdu = np.einsum("nij,nj->ni", W, (duv2[:, 1:2] * e1 - duv1[:, 1:2] * e2) / det[:, None])
        t = dpdu - n * np.sum(n * dpdu, axis=1, keepdims=True)
        sin_tn = np.linalg.norm(t, axis=1) / np.linalg.norm(dpdu, axis=1)
        T = _normalize(t)
    ng = _normalize(np.cross(np.einsum("nij,nj->ni", W, e1), np.einsum("nij,nj->ni", W, e2)))
    B = np.cross(n, T) * (np.sign(det) * np.where(np.sum(ng * n, axis=1) < 0.0, -1.0, 1.0))[:, None]
    entering = np.sum(r[:, 38:41] * ng, axis=1) < 0.0
    fallback = ~(np.isfinite(det) & (det != 0.0)) | ~(sin_tn ** 2 > 1e-8) | ~np.isfinite(sin_tn)
    return dict(n=n, T=T, B=B, det=det, sin_tn=sin_tn, entering=entering, fallback=fallback, ng=ng)


def tex_coords(rec):
    """The texture coordinate of the hit as the device forms it, uv0 + u uve1 + v uve2 in float32: on a map with uncorrelated
    neighbouring texels a coordinate one float32 rounding away reads a visibly different value, which is the texture unit's
    input, not its error (the texture tests, too, hand the float64 reference the device's float32 coordinates)."""
    r = np.asarray(rec, F32).reshape(-1, PROBE_IN)
    return (r[:, 18:20] + r[:, 24:25] * r[:, 20:22]).astype(F32) + (r[:, 25:26] * r[:, 22:24]).astype(F32)


def fetch(levels, width, height, rec):
    """The map's texel at every record, float64 (texture_reference), with the filter and footprint of the record."""
    r = np.asarray(rec, F32).reshape(-1, PROBE_IN)
    st = tex_coords(r).astype(F32)
    lod_bias = F32(0.5 * np.log2(float(width * height)))
    out = np.zeros((r.shape[0], 4))
    for f in (0, 1, 2):
        k = r[:, 41] == f
        if not k.any():
            continue
        args = np.zeros((int(k.sum()), 8), F32)
        args[:, 0:2] = st[k]
        args[:, 2] = r[k, 42] + lod_bias
        args[:, 3:7] = r[k, 43:47]
        out[k] = tref.sample(levels, width, height, f, args)
    return out


def perturb(rec, texel):
    """normal_map_perturb in float64: (N, 3) final world shading normal, (N,) fell back, and the guard's state
    (fired, |t|, the cosine with the viewer before the guard)."""
    r = np.asarray(rec, np.float64).reshape(-1, PROBE_IN)
    fr = frame(r)
    tv = 2.0 * np.asarray(texel, np.float64)[:, :3] - 1.0
    t_length = np.linalg.norm(tv, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = _normalize(tv[:, 0:1] * fr["T"] + tv[:, 1:2] * fr["B"] + tv[:, 2:3] * fr["n"])
    fallback = fr["fallback"] | ~(t_length > 0.0)
    side = np.where(fr["entering"], 1.0, -1.0)[:, None]
    m = m * side
    w = -_normalize(r[:, 38:41])
    cos_view = np.sum(m * w, axis=1)
    fired = cos_view < EPS
    guarded = _normalize(m + (EPS - cos_view)[:, None] * w)
    m = np.where(fired[:, None], guarded, m)
    plain = fr["n"] * side
    m = np.where(fallback[:, None], plain, m)
    return m, fallback, dict(fired=fired & ~fallback, t_length=t_length, cos_view=cos_view, sin_tn=fr["sin_tn"], frame=fr)


def write_tga(path, rgb):
    """Uncompressed 24-bit true-colour TGA, top-left origin: rgb is (h, w, 3) uint8, row 0 at the top."""
    rgb = np.asarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    header = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, w & 255, w >> 8, h & 255, h >> 8, 24, 0x20])
    with open(path, "wb") as f:
        f.write(header + np.ascontiguousarray(rgb[:, :, ::-1]).tobytes())


def random_normal_map(seed, w, h):
    """A smooth random tangent-space map: unit vectors with z >= 0.35, encoded 0.5 + 0.5 t, as uint8 (h, w, 3)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w] / np.array([h, w]).reshape(2, 1, 1)
    tx = 0.6 * np.sin(2 * np.pi * (xx * rng.integers(1, 5) + rng.random())) * np.cos(2 * np.pi * yy * rng.integers(1, 4))
    ty = 0.6 * np.cos(2 * np.pi * (yy * rng.integers(1, 5) + rng.random()))
    t = np.stack([tx, ty, np.ones_like(tx)], axis=-1)
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    return np.clip(np.round((0.5 + 0.5 * t) * 255.0), 0, 255).astype(np.uint8)


def constant_map_normal(c):
    """The float32 world normal the device decodes constant texel c (RGB bytes) to on a quad in the y = 0 plane whose vertex
    normals are +y and whose file coordinates run u along +x, v along +z. The OBJ loader stores v as 1 - v, so on the device v runs
    along -z: T = +x, B (which follows dp/dv) = -z = cross(n, T), an unmirrored frame. m = normalize(t.x T + t.y B + t.z n) with
    t = 2 c / 255 - 1, in the device's float32 operations."""
    c = np.asarray(c, F32) * F32(1.0 / 255.0)
    t = F32(2.0) * c - F32(1.0)
    m = np.array([t[0], t[2], -t[1]], F32)
    length = np.sqrt(F32(m[0] * m[0]) + F32(m[1] * m[1]) + F32(m[2] * m[2]), dtype=F32)
    return (m / length).astype(F32)
