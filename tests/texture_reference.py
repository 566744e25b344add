"""Float64 reference of the software texture unit, for the texture-unit tests.

Written from DESIGN.md section 5 and the `rt_texture_desc` comment of include/gpu_raytracer_amd.h alone: it reads and
calls no product or oracle code, so a misreading that the kernel and the oracle share shows up here.

* Mip chain: level l is max(w >> l, 1) x max(h >> l, 1); levels lie back to back, level 0 first.
* BC1 (D3D rules): 8 bytes per 4 x 4 texels, ((w + 3) / 4) x ((h + 3) / 4) blocks per level in row-major order. End points
  expand from 5:6:5 by bit replication; c0 > c1: four colours, the two thirds rounded to nearest; otherwise three colours (the
  half rounded down) and index 3 transparent black. Texel (x, y) of a block takes index bits 2 (4 y + x).
* Bilinear: texel centres at x = s W - 0.5, wrap addressing for material textures (clamp for the sky and the LUTs).
* Trilinear: lod clamped to [0, levels - 1]; floor(lod) and the next level blended by the fraction; one level when the
  fraction is 0 or there is no next level.
* Anisotropic (tex2DGrad): with p = |gradient| in texels, N = min(ceil(p_max / p_min), 16) probes (at least 1) at offsets
  (i + 0.5) / N - 0.5 along the major gradient, trilinear at lod = log2(max(p_max / N, 1e-12)), averaged.
* Sky: u = atan2(-z, x) / 2 pi + 0.5, v = acos(y) / pi, clamp-addressed bilinear, times the sky scale.

Contract: the texel-space POSITION is part of the definition and is formed in float32, as the kernel forms it (the product
builds with -ffp-contract=off, so no multiply-add is fused): x = f32(f32(s W) - 0.5); the probe coordinates s + major.x o with
o = (i + 0.5) / N - 0.5; and p_max, p_min, N and lod. numpy float32 does exactly these IEEE operations. Everything after the
position is float64: floor, wrap, the texel fetch, the weights, the blends and the sums. Without this rule the rounding of
s W at |s| = 1000 moves a sample by 1/64 texel and a comparison would measure float32, not the filter. The sky is the
exception: atan2f / acosf place its sample only to a few ulp, so its position is formed in float64 and compared with a
tolerance instead.
"""
import numpy as np

F32 = np.float32


def level_sizes(width, height, mip_levels):
    return [(max(width >> l, 1), max(height >> l, 1)) for l in range(mip_levels)]


def full_chain_levels(width, height):
    return int(max(width, height)).bit_length()


def rgba8_levels(texels, width, height, mip_levels):
    """Slices an RGBA8 chain (uint8, levels back to back) into one (h, w, 4) array per level."""
    texels = np.asarray(texels, np.uint8).reshape(-1)
    out, offset = [], 0
    for w, h in level_sizes(width, height, mip_levels):
        out.append(texels[offset:offset + w * h * 4].reshape(h, w, 4))
        offset += w * h * 4
    if offset != texels.size:
        raise ValueError("chain holds %d bytes, %d x %d x %d levels need %d" % (texels.size, width, height, mip_levels, offset))
    return out


def bc1_block_count(width, height, mip_levels):
    return sum(((w + 3) // 4) * ((h + 3) // 4) for w, h in level_sizes(width, height, mip_levels))


def _expand_565(c):
    r, g, b = c >> 11, (c >> 5) & 63, c & 31
    return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)], axis=-1)


def bc1_decode_blocks(blocks):
    """(n, 8) uint8 BC1 blocks -> (n, 16, 4) uint8 RGBA, texel y * 4 + x of each block."""
    b = np.asarray(blocks, np.uint8).reshape(-1, 8).astype(np.uint32)
    n = b.shape[0]
    c0 = b[:, 0] | (b[:, 1] << 8)
    c1 = b[:, 2] | (b[:, 3] << 8)
    indices = b[:, 4] | (b[:, 5] << 8) | (b[:, 6] << 16) | (b[:, 7] << 24)
    e0, e1 = _expand_565(c0), _expand_565(c1)
    four = (c0 > c1)[:, None]
    palette = np.zeros((n, 4, 4), np.uint32)
    palette[:, 0, :3], palette[:, 1, :3] = e0, e1
    palette[:, 0:3, 3] = 255
    palette[:, 2, :3] = np.where(four, (2 * e0 + e1 + 1) // 3, (e0 + e1) // 2)
    palette[:, 3, :3] = np.where(four, (e0 + 2 * e1 + 1) // 3, 0)
    palette[:, 3, 3] = np.where(four[:, 0], 255, 0)
    select = (indices[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3
    return palette[np.arange(n)[:, None], select].astype(np.uint8)


def bc1_levels(blocks, width, height, mip_levels):
    """Decodes a BC1 chain (8-byte blocks, levels back to back) into one (h, w, 4) uint8 array per level; levels
    smaller than a block keep the top-left texels of theirs."""
    decoded = bc1_decode_blocks(blocks)
    if decoded.shape[0] != bc1_block_count(width, height, mip_levels):
        raise ValueError("chain holds %d blocks, %d x %d x %d levels need %d" % (decoded.shape[0], width, height, mip_levels, bc1_block_count(width, height, mip_levels)))
    out, offset = [], 0
    for w, h in level_sizes(width, height, mip_levels):
        bw, bh = (w + 3) // 4, (h + 3) // 4
        d = decoded[offset:offset + bw * bh].reshape(bh, bw, 4, 4, 4)   # block row, block column, y, x, channel
        out.append(np.ascontiguousarray(d.transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)[:h, :w]))
        offset += bw * bh
    return out


def chain_bytes(levels):
    """One (h, w, 4) uint8 array per level -> the RGBA8 chain as rt_texture_desc holds it."""
    return np.concatenate([np.ascontiguousarray(l, np.uint8).reshape(-1) for l in levels])


def texel_position(coord, n):
    """x = f32(f32(coord n) - 0.5): the float32 part of the contract."""
    return ((np.asarray(coord, F32) * F32(n)).astype(F32) - F32(0.5)).astype(F32)


def bilinear_wrap(level, s, t):
    """Wrap-addressed bilinear fetch of one (h, w, 4) uint8 level at float32 (s, t); float64 RGBA in [0, 1]."""
    h, w = level.shape[:2]
    x = texel_position(s, w).astype(np.float64)
    y = texel_position(t, h).astype(np.float64)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = xi % w, (xi + 1) % w, yi % h, (yi + 1) % h
    c = level.astype(np.float64) / 255.0
    top = c[ya, xa] * (1.0 - fx) + c[ya, xb] * fx
    bottom = c[yb, xa] * (1.0 - fx) + c[yb, xb] * fx
    return top * (1.0 - fy) + bottom * fy


def tex2d(levels, s, t):
    """tex2D: level 0."""
    return bilinear_wrap(levels[0], np.asarray(s, F32), np.asarray(t, F32))


def tex2d_lod(levels, s, t, lod):
    """tex2DLod: trilinear between floor(lod) and the next level, lod clamped to [0, levels - 1]."""
    s, t = np.asarray(s, F32), np.asarray(t, F32)
    lod = np.minimum(np.maximum(np.asarray(lod, F32), F32(0)), F32(len(levels) - 1)).astype(np.float64)
    l0 = np.floor(lod).astype(np.int64)
    fl = (lod - l0)[:, None]
    single = (fl[:, 0] == 0.0) | (l0 + 1 >= len(levels))
    out = np.zeros((s.size, 4))
    for l in np.unique(l0):
        m = l0 == l
        a = bilinear_wrap(levels[l], s[m], t[m])
        both = ~single[m]
        if both.any():
            idx = np.flatnonzero(m)[both]
            b = bilinear_wrap(levels[l + 1], s[idx], t[idx])
            a[both] = a[both] * (1.0 - fl[idx]) + b * fl[idx]
        out[m] = a
    return out


def anisotropic_footprint(width, height, dx, dy):
    """(N as float32, lod as float32, major gradient (n, 2) float32), formed in float32 as the kernel forms them."""
    dx, dy = np.asarray(dx, F32).reshape(-1, 2), np.asarray(dy, F32).reshape(-1, 2)
    w, h = F32(width), F32(height)

    def length(g):
        a, b = (g[:, 0] * w).astype(F32), (g[:, 1] * h).astype(F32)
        return np.sqrt((a * a).astype(F32) + (b * b).astype(F32)).astype(F32)
    px, py = length(dx), length(dy)
    p_max, p_min = np.maximum(px, py), np.minimum(px, py)
    major = np.where((px >= py)[:, None], dx, dy)
    n_f = np.minimum(np.ceil((p_max / np.maximum(p_min, F32(1e-12))).astype(F32)), F32(16)).astype(F32)
    n_f = np.where(n_f >= F32(1), n_f, F32(1)).astype(F32)
    lod = np.log2(np.maximum((p_max / n_f).astype(F32), F32(1e-12))).astype(F32)
    return n_f, lod, major


def tex2d_grad(levels, width, height, s, t, dx, dy):
    """tex2DGrad: N trilinear probes along the major gradient, averaged."""
    s, t = np.asarray(s, F32), np.asarray(t, F32)
    n_f, lod, major = anisotropic_footprint(width, height, dx, dy)
    n = n_f.astype(np.int64)
    total = np.zeros((s.size, 4))
    for i in range(int(n.max(initial=1))):
        m = n > i
        o = ((F32(i) + F32(0.5)) / n_f[m]).astype(F32) - F32(0.5)
        ps = (s[m] + (major[m, 0] * o).astype(F32)).astype(F32)
        pt = (t[m] + (major[m, 1] * o).astype(F32)).astype(F32)
        total[m] += tex2d_lod(levels, ps, pt, lod[m])
    return total / n[:, None]


def sample(levels, width, height, filter, args):
    """Filter 0 / 1 / 2 on (n, 8) float32 args {s, t, lod, dx.x, dx.y, dy.x, dy.y, pad} (rt_sample_texture's layout)."""
    a = np.asarray(args, F32).reshape(-1, 8)
    if filter == 0:
        return tex2d(levels, a[:, 0], a[:, 1])
    if filter == 1:
        return tex2d_lod(levels, a[:, 0], a[:, 1], a[:, 2])
    return tex2d_grad(levels, width, height, a[:, 0], a[:, 1], a[:, 3:5], a[:, 5:7])


def clamp_taps(x, n):
    """Clamp addressing around a texel-space position x (float64): (i0, i1, fraction)."""
    x0 = np.floor(x)
    i = x0.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), x - x0


def lut(table, coords):
    """Clamp-addressed linear fetch of a 1-, 2- or 3-d float table indexed [z][y][x] at (n, dims) float32 coordinates."""
    table = np.asarray(table, np.float64)
    c = np.asarray(coords, F32).reshape(-1, table.ndim)
    taps = [clamp_taps(texel_position(c[:, k], table.shape[table.ndim - 1 - k]).astype(np.float64), table.shape[table.ndim - 1 - k]) for k in range(table.ndim)]
    out = np.zeros(c.shape[0])
    for corner in range(1 << table.ndim):
        weight = np.ones(c.shape[0])
        index = []
        for k in range(table.ndim):
            i0, i1, f = taps[k]
            upper = (corner >> k) & 1
            weight *= f if upper else 1.0 - f
            index.append(i1 if upper else i0)
        out += weight * table[tuple(index[::-1])]
    return out


def sky(image, scale, directions):
    """sample_sky on an equirect (h, w, 4) float image for (n, 3) unit directions: float64 RGB."""
    img = np.asarray(image, np.float64)
    h, w = img.shape[:2]
    d = np.asarray(directions, F32).reshape(-1, 3).astype(np.float64)
    u = np.arctan2(-d[:, 2], d[:, 0]) / (2.0 * np.pi) + 0.5
    v = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
    x0, x1, fx = clamp_taps(u * w - 0.5, w)
    y0, y1, fy = clamp_taps(v * h - 0.5, h)
    fx, fy = fx[:, None], fy[:, None]
    top = img[y0, x0] * (1.0 - fx) + img[y0, x1] * fx
    bottom = img[y1, x0] * (1.0 - fx) + img[y1, x1] * fx
    return scale * (top * (1.0 - fy) + bottom * fy)[:, :3]
