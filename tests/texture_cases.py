"""Textures and coordinates of the texture-unit tests (test_texture_unit.py on the CPU, test_gpu_texture_unit.py on the device).

Every level of every texture has its own random content (no box filter), so a wrong level offset cannot pass."""
import numpy as np

from texture_reference import bc1_block_count, bc1_levels, full_chain_levels, level_sizes, rgba8_levels

F32 = np.float32

# (w, h): full mip chains. 37 x 23 mixes power-of-two and other sides level by level (37x23, 18x11, 9x5, 4x2, 2x1, 1x1);
# 256 x 16 reaches N x 1 while the width keeps halving; 64 x 256 is Sponza's shape.
RGBA8_SIZES = [(1, 1), (1, 7), (3, 1), (5, 3), (37, 23), (1000, 750), (64, 64), (256, 16), (64, 256)]
# full chains down to 1 x 1 (levels of 2 x 2 and 1 x 1 use part of a block); 12 x 20 and 6 x 10 are not powers of two
BC1_SIZES = [(4, 4), (8, 8), (64, 64), (64, 8), (12, 20), (6, 10)]


class Texture:
    def __init__(self, name, width, height, levels, data, fmt):
        self.name, self.width, self.height, self.mip_levels = name, width, height, levels
        self.data = data            # what rt_texture_desc::texels points at: RGBA8 chain or BC1 blocks
        self.format = fmt           # 0 RGBA8, 1 BC1
        self.power_of_two = (width & (width - 1)) == 0 and (height & (height - 1)) == 0

    def levels(self):
        if self.format == 0:
            return rgba8_levels(self.data, self.width, self.height, self.mip_levels)
        return bc1_levels(self.data, self.width, self.height, self.mip_levels)

    def __repr__(self):
        return self.name


def rgba8_texture(w, h, seed):
    rng = np.random.default_rng(seed)
    levels = full_chain_levels(w, h)
    count = sum(lw * lh for lw, lh in level_sizes(w, h, levels))
    return Texture("rgba8_%dx%d" % (w, h), w, h, levels, rng.integers(0, 256, count * 4, dtype=np.uint8), 0)


def bc1_blocks(count, rng):
    """Random blocks: c0 > c1 and c0 < c1 about equally often, and about one in eight with c0 == c1."""
    blocks = rng.integers(0, 256, (count, 8), dtype=np.uint8)
    equal = rng.random(count) < 0.125
    blocks[equal, 2:4] = blocks[equal, 0:2]
    return blocks


def bc1_texture(w, h, seed):
    rng = np.random.default_rng(seed)
    levels = full_chain_levels(w, h)
    return Texture("bc1_%dx%d" % (w, h), w, h, levels, bc1_blocks(bc1_block_count(w, h, levels), rng).reshape(-1), 1)


def bc1_texture_above(w, h, seed, floor):
    """bc1_texture whose every decoded texel is opaque and at least `floor` (a byte) in every channel: both endpoints of a block lie at or above it and
    c0 > c1 (the four-colour mode, whose two other colours lie between the endpoints; no transparent black)."""
    rng = np.random.default_rng(seed)
    levels = full_chain_levels(w, h)
    count = bc1_block_count(w, h, levels)
    lo5, lo6 = (floor + 7) // 8, (floor + 3) // 4   # (a 5-bit r expands to at least 8 r, a 6-bit g to at least 4 g)
    r1 = rng.integers(lo5, 31, count); r0 = rng.integers(r1 + 1, 32)   # c0's red above c1's: c0 > c1 as 16-bit numbers
    g, b = rng.integers(lo6, 64, (2, count)), rng.integers(lo5, 32, (2, count))
    c0, c1 = (r0 << 11) | (g[0] << 5) | b[0], (r1 << 11) | (g[1] << 5) | b[1]
    blocks = rng.integers(0, 256, (count, 8), dtype=np.uint8)   # (the indices: any)
    blocks[:, 0], blocks[:, 1], blocks[:, 2], blocks[:, 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    return Texture("bc1_above_%dx%d" % (w, h), w, h, levels, blocks.reshape(-1), 1)


def rgba8_textures():
    return [rgba8_texture(w, h, 100 + i) for i, (w, h) in enumerate(RGBA8_SIZES)]


def bc1_textures():
    return [bc1_texture(w, h, 200 + i) for i, (w, h) in enumerate(BC1_SIZES)]


SPECIAL_COORDS = [0.0, -0.0, 1.0, float(np.nextafter(F32(1), F32(0))), -0.3, -3.7, 5.25, 1000.3, -1000.3]
RATIOS = [1.0, 1.5, 2.9, 4.0, 16.0, 40.0]


def _pack(s, t, lod=None, dx=None, dy=None):
    a = np.zeros((len(s), 8), F32)
    a[:, 0], a[:, 1] = s, t
    if lod is not None:
        a[:, 2] = lod
    if dx is not None:
        a[:, 3:5], a[:, 5:7] = dx, dy
    return a


def _positions(tex, rng, uniform):
    """s, t: uniform in [0, 1), exact texel centres and edges k / W of every level, and the special values in every pairing."""
    s = [rng.random(uniform)]
    t = [rng.random(uniform)]
    for w, h in level_sizes(tex.width, tex.height, tex.mip_levels):
        for n, own, other in ((w, s, t), (h, t, s)):
            k = rng.integers(-2 * n, 3 * n + 1, 200)
            own.append(np.concatenate([(k + 0.5) / n, k / n]))
            other.append(rng.random(400))
    sp = np.array(SPECIAL_COORDS)
    s.append(np.repeat(sp, sp.size)); t.append(np.tile(sp, sp.size))
    s.append(sp); t.append(rng.random(sp.size))
    s.append(rng.random(sp.size)); t.append(sp)
    return np.concatenate(s).astype(F32), np.concatenate(t).astype(F32)


def args_level0(tex, seed=1, uniform=8000):
    s, t = _positions(tex, np.random.default_rng(seed), uniform)
    return _pack(s, t)


def args_lod(tex, seed=2, uniform=8000):
    rng = np.random.default_rng(seed)
    s, t = _positions(tex, rng, uniform)
    top = tex.mip_levels - 1
    choices = np.concatenate([[-2.5, -1.0, -0.0, 0.0, top + 0.5, top + 1.0, top + 7.25], np.arange(tex.mip_levels, dtype=np.float64),
                              np.arange(tex.mip_levels) + 0.25, np.arange(tex.mip_levels) + 0.5, np.arange(tex.mip_levels) + 0.875])
    lod = np.where(rng.random(s.size) < 0.5, rng.choice(choices, s.size), rng.uniform(-1.0, top + 1.5, s.size))
    return _pack(s, t, lod=lod)


def args_grad(tex, seed=3, count=10000):
    """Gradients of every ratio (1, 1.5, 2.9, exactly 4, 16 and 40, the last capped at 16 probes), major along x and along y,
    as dx or as dy; one gradient zero; both zero (N = 1); and power-of-two footprints (minor and major 2^k texels along the
    axes, ratio 1, 2, 4 or 16) whose lod is an exact integer."""
    rng = np.random.default_rng(seed)
    W, H = tex.width, tex.height
    s, t = rng.random(count), rng.random(count)
    special = rng.random(count) < 0.2
    s[special] = rng.choice(SPECIAL_COORDS, special.sum())
    t[special] = rng.choice(SPECIAL_COORDS, special.sum())
    minor_texels = np.exp2(rng.uniform(-3, np.log2(max(W, H)) + 1, count))
    ratio = rng.choice(RATIOS, count)
    along_y = rng.random(count) < 0.5
    angle = rng.uniform(0, 2 * np.pi, count) * (rng.random(count) < 0.5)   # half exactly along an axis
    axis_major = np.where(along_y, np.pi / 2, 0.0) + angle
    major = np.stack([np.cos(axis_major) * minor_texels * ratio / W, np.sin(axis_major) * minor_texels * ratio / H], axis=1)
    minor = np.stack([-np.sin(axis_major) * minor_texels / W, np.cos(axis_major) * minor_texels / H], axis=1)
    swap = rng.random(count) < 0.5
    dx = np.where(swap[:, None], minor, major)
    dy = np.where(swap[:, None], major, minor)
    kind = rng.random(count)
    dx[kind < 0.05] = 0.0                               # one gradient zero
    dy[(kind >= 0.05) & (kind < 0.1)] = 0.0
    both = (kind >= 0.1) & (kind < 0.13)                # both zero: N = 1, lod clamps to 0
    dx[both] = 0.0; dy[both] = 0.0
    exact = (kind >= 0.13) & (kind < 0.4)               # power-of-two footprints along the axes
    k = rng.integers(-2, int(np.log2(max(W, H))) + 2, exact.sum())
    r = rng.choice([1, 2, 4, 16], exact.sum())
    minor_len = np.exp2(k.astype(np.float64))
    ex_major_x = rng.random(exact.sum()) < 0.5
    mx = np.where(ex_major_x, minor_len * r / W, 0.0); my = np.where(ex_major_x, 0.0, minor_len * r / H)
    nx = np.where(ex_major_x, 0.0, minor_len / W); ny = np.where(ex_major_x, minor_len / H, 0.0)
    dx[exact] = np.stack([mx, my], 1); dy[exact] = np.stack([nx, ny], 1)
    return _pack(s, t, dx=dx.astype(F32), dy=dy.astype(F32))


def all_args(tex):
    return {0: args_level0(tex), 1: args_lod(tex), 2: args_grad(tex)}


def lod_is_exact(tex, args):
    """Probes whose anisotropic lod is an exact integer in float32 (p_max / N a power of two): log2 of it is exact in any library."""
    from texture_reference import anisotropic_footprint
    n_f, _, major = anisotropic_footprint(tex.width, tex.height, args[:, 3:5], args[:, 5:7])
    dx, dy = args[:, 3:5], args[:, 5:7]
    w, h = F32(tex.width), F32(tex.height)

    def length(g):
        a, b = (g[:, 0] * w).astype(F32), (g[:, 1] * h).astype(F32)
        return np.sqrt((a * a).astype(F32) + (b * b).astype(F32)).astype(F32)
    q = np.maximum((np.maximum(length(dx), length(dy)) / n_f).astype(F32), F32(1e-12))
    mantissa, _ = np.frexp(q)
    return mantissa == 0.5


def table_cases(seed=5):
    """Random tables with sides 1, 2 and 7 in every dimension count, plus the shapes of the Kulla-Conty tables."""
    rng = np.random.default_rng(seed)
    shapes = [(1,), (2,), (7,), (32,), (1, 1), (2, 7), (7, 2), (1, 7), (32, 32), (16, 16), (1, 1, 1), (2, 2, 2), (7, 2, 1), (1, 7, 2), (16, 16, 16)]
    return [rng.random(shape).astype(F32) for shape in shapes]


def table_coords(dims, seed=6, count=3000, sides=None):
    """Below 0, above 1, texel centres, 0, 1 and uniform in [0, 1)."""
    rng = np.random.default_rng(seed)
    c = rng.random((count, dims))
    c[: count // 6] = rng.uniform(-0.5, 0.0, (count // 6, dims))
    c[count // 6: count // 3] = rng.uniform(1.0, 1.5, (count // 6, dims))
    if sides is not None:
        for k, n in enumerate(sides):
            c[count // 3: count // 2, k] = (rng.integers(0, n, count // 2 - count // 3) + 0.5) / n
    ends = np.array([0.0, 1.0, -0.0, float(np.nextafter(F32(1), F32(0)))])
    c[-ends.size:] = ends[:, None]
    c[-2 * ends.size:-ends.size] = np.tile(ends, dims).reshape(dims, -1).T[::-1]
    return c.astype(F32)


def sky_image(seed=7, w=64, h=32):
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 4)).astype(F32) * 4.0
    return img


def sky_directions(seed=8, count=20000):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d.astype(F32)


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
