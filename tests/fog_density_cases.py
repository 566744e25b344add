"""Shared cases of the density-grid tests (test_fog_density.py, test_gpu_fog_density.py): the grids, the segments added to those of fog_cases.py, the
bounds of the voxel march derived from its float32 roundings, and the rendering helper of the GPU file."""
import math

import numpy as np

import fog_cases as cases

EPS = 2.0 ** -24   # half a float32 ulp of 1: one rounding to nearest
BOX_MIN, BOX_MAX = cases.BOX_MIN, cases.BOX_MAX   # 2 x 2 x 2
R3 = cases.R3

GRID_NAMES = ["1x1x1", "2x1x1", "1x1x7", "5x4x3", "8x8x8", "9x8x8", "8x8x9", "17x5x9", "64x64x64"]   # nx x ny x nz
ONE_BRICK = (4, 4, 2)   # the brick (bx, by, bz) of 64 x 64 x 64 that holds density


def dims(name):
    return tuple(int(v) for v in name.split("x"))


def grid(name):
    """The seeded grid of a name, as (nz, ny, nx) float32. Values include 0, 1e-30 and 1e6; wherever nz > 1 the slab k = 0 is empty (a ray can cross density 0 only)."""
    nx, ny, nz = dims(name)
    rng = np.random.default_rng(1000 + nx * 10000 + ny * 100 + nz)
    if name == "1x1x1":
        return np.full((1, 1, 1), 0.75, np.float32)
    if name == "2x1x1":
        return np.array([[[0.0, 1e6]]], np.float32)
    if name == "1x1x7":
        return np.array([0.0, 1e-30, 1.0, 2.5, 0.0, 1e6, 0.25], np.float32).reshape(7, 1, 1)
    if name == "64x64x64":
        g = np.zeros((64, 64, 64), np.float32)
        bx, by, bz = ONE_BRICK
        g[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = rng.uniform(0.5, 2.0, (8, 8, 8))
        return g
    g = rng.uniform(0.0, 3.0, (nz, ny, nx)).astype(np.float32)
    g[rng.random((nz, ny, nx)) < 0.35] = 0.0
    flat = g.reshape(-1)
    g[0] = 0.0
    flat[rng.integers(nx * ny, flat.size)] = 1e-30; flat[rng.integers(nx * ny, flat.size)] = 1e6
    if name == "9x8x8":
        g[:, :, :8] = 0.0; g[1:, :, 8] = np.maximum(g[1:, :, 8], 0.5)   # the whole brick empty, the partial one (one voxel wide) not
    if name == "8x8x9":
        g[8] = 0.0                                                         # the partial brick (one slab) empty
    return g


SHAFT_HALVES = (0.25, 2.0)   # the 2 x 1 x 1 grid of the light-shaft tests: thin for x below the box's middle, dense above it


def tame(grid_):
    """The grid without its 1e6 outlier (for the tests whose bound a value of 1e6 would make empty)."""
    return np.minimum(grid_, np.float32(3.0))


def cell(name):
    nx, ny, nz = dims(name)
    return (BOX_MAX - BOX_MIN).astype(np.float64) / np.array([nx, ny, nz], np.float64)


def extra_segments(name):
    """name -> (origin, direction, t_end): rays along a cell plane, through cell corners on the diagonal, inside one voxel, through density 0 only."""
    nx, ny, nz = dims(name)
    c = cell(name)
    lo = BOX_MIN.astype(np.float64)
    plane_x = float(np.float32(lo[0] + np.float32(nx // 2) * np.float32(c[0]))) if nx > 1 else 0.0
    plane_y = float(np.float32(lo[1] + np.float32(ny // 2) * np.float32(c[1]))) if ny > 1 else 0.5
    inside = lo + 0.5 * c
    out = {
        "along_x_plane":       ((plane_x, 0.5, 0.0), (0.0, 0.0, 1.0), math.inf),
        "along_y_plane_back":  ((3.0, plane_y, 3.1), (-1.0, 0.0, 0.0), math.inf),
        "in_plane_diagonal":   ((plane_x, -2.5, 0.0), (0.0, cases.R2, cases.R2), math.inf),
        "corner_diagonal":     ((-2.0, -1.5, 1.0), (R3, R3, R3), math.inf),
        "corner_diagonal_back": ((2.0, 2.5, 5.0), (-R3, -R3, -R3), math.inf),
        "corner_diagonal_end": ((-2.0, -1.5, 1.0), (R3, R3, R3), 3.0),
        "inside_one_voxel":    (tuple(inside - 0.05 * c), (R3, R3, R3), 0.1 * float(c.min())),
        "inside_one_voxel_back": (tuple(lo + (np.array([nx, ny, nz]) - 0.5) * c), (-R3, R3, -R3), 0.2 * float(c.min())),
        "skew":                ((-2.7, -0.9, 1.1), (0.55708601, 0.37139068, 0.74278135), math.inf),
        "skew_back":           ((1.9, 2.2, 4.6), (-0.59628479, -0.66666667, -0.4472136), math.inf),
    }
    if nz > 1:
        out["density_0_only"] = ((-3.0, 0.5, float(lo[2] + 0.5 * c[2])), (1.0, 0.0, 0.0), math.inf)
    if name == "2x1x1":
        out["density_0_only"] = ((-0.5, 0.5, 0.0), (0.0, 0.0, 1.0), math.inf)
    return out


def segments(name):
    s = dict(cases.SEGMENTS)
    s.update(extra_segments(name))
    return s


PATHS = cases.PATHS[:5]


def segment_probes(name):
    names, o, d, t, px, b, s = [], [], [], [], [], [], []
    for seg_name, (origin, direction, t_end) in segments(name).items():
        for pixel, bounce, sample in PATHS:
            names.append(seg_name); o.append(origin); d.append(direction); t.append(t_end); px.append(pixel); b.append(bounce); s.append(sample)
    return names, np.array(o, np.float32), np.array(d, np.float32), np.array(t, np.float32), np.array(px, np.uint32), np.array(b, np.uint32), np.array(s, np.uint32)


# ---- the bounds of the march ----------------------------------------------------------------------------------------------------
# Derived from the roundings of rt_fog_grid.h, with B = the largest |coordinate| of the box and O = the largest |coordinate| of the origin.
# * A plane: cell = (hi - lo) / n is two roundings (2 EPS relative), float(i) * cell one more: 3 EPS x extent <= 6 EPS B; the sum with lo: EPS x |plane| <= EPS B.
#   The difference plane - o: EPS (B + O). The quotient by d_k: EPS |t|. So a crossing is computed within (8 B + O) EPS / |d_k| + EPS |t| of where float64 has it.
# * An index taken from the position (the entry voxel, and behind an empty brick): floor((o + t d - lo) / cell). t d and the two sums: EPS (|t d| + |p| + |p - lo|)
#   <= EPS (O + 4 B) for a point p of the box; t itself carries the crossing's error; the index is wrong only where p lies that close to a plane, that is for a
#   time of at most (O + 4 B) EPS / |d_k| around the crossing, on top of it.
#   Together: a crossing's allowance a_c = (12 B + 2 O) EPS / |d_k| + 2 EPS |t_c|. While the march is within a_c of crossing c it may be in a voxel that is not the
#   true one: a neighbour across that plane or, where crossings of several axes fall together, across an edge or a corner. The density it uses there is at most
#   rho_c, the largest value among the 3 x 3 x 3 voxels around the crossing point, so D is off by at most the sum of rho_c a_c over the crossings that can
#   matter -- those within a_c of [t0, t1] (a plane just outside the interval can still be stepped over by the march).
# * The sums: seg = t_exit - t rounds once (EPS seg), rho x seg once, D + ... once per step: (pieces + 3) EPS D.
# * Where the interval's ends are not the device's own (a test that clips in float64): each end is off by clip_error, in density at most the grid's maximum.
def crossing_allowances(box_min, box_max, grid_, o, d, t0, t1):
    """[(a_c, rho_c)] of the crossings within their allowance of [t0, t1]."""
    nz, ny, nx = grid_.shape
    n = (nx, ny, nz)
    B = float(max(np.abs(box_min).max(), np.abs(box_max).max())); O = float(np.abs(o).max())
    o = [float(v) for v in o]; d = [float(v) for v in d]
    lo = [float(v) for v in box_min]; hi = [float(v) for v in box_max]
    out = []
    for k in range(3):
        if d[k] == 0.0:
            continue
        for i in range(n[k] + 1):
            t = (lo[k] + i * (hi[k] - lo[k]) / n[k] - o[k]) / d[k]
            a = (12.0 * B + 2.0 * O) * EPS / abs(d[k]) + 2.0 * EPS * abs(t)
            if not (t0 - a <= t <= t1 + a):
                continue
            at = min(max(t, t0), t1)
            index = [min(max(int(math.floor((o[j] + at * d[j] - lo[j]) / ((hi[j] - lo[j]) / n[j]))), 0), n[j] - 1) for j in range(3)]
            index[k] = min(max(i, 0), n[k] - 1)
            around = grid_[max(index[2] - 1, 0):index[2] + 2, max(index[1] - 1, 0):index[1] + 2, max(index[0] - 1, 0):index[0] + 2]
            out.append((a, float(around.max())))
    return out


def density_length_bound(box_min, box_max, grid_, o, d, t0, t1, D, pieces, clip_error=0.0):
    """(the bound of |D32 - D64|, the largest crossing allowance)."""
    allowances = crossing_allowances(box_min, box_max, grid_, o, d, t0, t1)
    bound = sum(a * rho for a, rho in allowances) + (pieces + 3) * EPS * D + 2.0 * clip_error * float(grid_.max())
    return bound, (max(a for a, _ in allowances) if allowances else 0.0)


class Rendering:
    """A scene file rendered through the C ABI on device 0 (the helper of test_gpu_fog.py, with the grid)."""
    def __init__(self, grt, path, w, h, config, scheduler="merged", sky=None):
        import ctypes
        self.grt, self.lib, self.w, self.h = grt, grt.device_lib(), w, h
        self.lib.rt_last_error.restype = ctypes.c_char_p
        grt.config_reset(); grt.config_set(**config)
        self.scene = grt.Scene(path)
        grt.config_set(**config)
        self.pt = grt.Pathtracer(self.scene, w, h, device=0)
        self.pt.update()
        if sky is not None:
            texel = np.array([sky, sky, sky, 1.0], np.float32)
            assert self.lib.rt_set_sky(self.pt.ctx, texel.ctypes.data, 1, 1, 1.0) == 0
        grt.set_scheduler(self.pt.ctx, scheduler)

    def fog(self, box_min, box_max, sigma_a, sigma_s, g=0.0):
        status = self.grt.set_fog_volume(self.pt.ctx, self.grt.fog_volume_record(box_min, box_max, sigma_a, sigma_s, g))
        assert status == 0, self.lib.rt_last_error(self.pt.ctx)

    def density(self, grid_):
        status = self.grt.set_fog_density(self.pt.ctx, grid_)
        assert status == 0, self.lib.rt_last_error(self.pt.ctx)

    def render(self, samples, first=0, batch=16):
        for s in range(first, first + samples, batch):
            assert self.lib.rt_render_samples(self.pt.ctx, s, min(batch, first + samples - s)) == 0, self.lib.rt_last_error(self.pt.ctx)
        return self.pt.read_framebuffer()[:, :self.w].copy()

    def close(self):
        self.pt.close(); self.scene.close(); self.grt.config_reset()
