"""The density grid of the fog volume restated in float64, by a method independent of the device's voxel march (csrc/rt_fog_grid.h):
all plane crossings of a segment are collected and SORTED, and the voxel of each interval between two of them is taken from the interval's
MIDPOINT -- no stepping, no index carried from one interval to the next. On top of that the density length D(t) = integral of rho ds, its
inversion, and the estimator of fog_reference.py with length replaced by density length."""
import math

import numpy as np

import fog_reference as ref


def planes(lo, hi, n):
    """The n + 1 cell planes of one axis in float64 on the float32 box: lo + i (hi - lo) / n, the outermost the faces themselves."""
    lo, hi = float(lo), float(hi)
    p = [lo + i * (hi - lo) / n for i in range(n + 1)]
    p[0], p[n] = lo, hi
    return p


def intervals(box_min, box_max, grid, o, d, t0, t1):
    """The segment (o, d, [t0, t1]) cut at every cell plane it crosses: [(t_a, t_b, rho, [(axis, plane, t_cross)] of the cut at t_a)], t0 <= t_a < t_b <= t1,
    in order. grid: (nz, ny, nx). The voxel of an interval is the one its midpoint lies in (clamped: a midpoint on a face belongs to the box)."""
    nz, ny, nx = grid.shape
    n = (nx, ny, nz)
    o = [float(v) for v in o]; d = [float(v) for v in d]
    t0, t1 = float(t0), float(t1)
    cuts = []
    for k in range(3):
        if d[k] == 0.0:
            continue
        for p in planes(box_min[k], box_max[k], n[k])[1:-1]:
            t = (p - o[k]) / d[k]
            if t0 < t < t1:
                cuts.append((t, k, p))
    cuts.sort()
    out = []
    edges = [(t0, None, None)] + cuts + [(t1, None, None)]
    for a, b in zip(edges[:-1], edges[1:]):
        if not b[0] > a[0]:
            continue
        mid = 0.5 * (a[0] + b[0]) if math.isfinite(b[0]) else a[0] + 1.0
        index = []
        for k in range(3):
            lo, hi = float(box_min[k]), float(box_max[k])
            i = int(math.floor((o[k] + mid * d[k] - lo) / ((hi - lo) / n[k])))
            index.append(min(max(i, 0), n[k] - 1))
        out.append((a[0], b[0], float(grid[index[2], index[1], index[0]]), a[1], a[2]))
    return out


def density_length(box_min, box_max, grid, o, d, t0, t1):
    return sum(rho * (b - a) for a, b, rho, _, _ in intervals(box_min, box_max, grid, o, d, t0, t1) if rho > 0.0)


def invert(pieces, target):
    """Where D(t) passes `target` over the intervals of a segment: (t, D before the interval, the interval) or None when D(t1) <= target."""
    D = 0.0
    for piece in pieces:
        a, b, rho = piece[:3]
        if rho > 0.0:
            if D + rho * (b - a) > target:
                return a + (target - D) / rho, D, piece
            D += rho * (b - a)
    return None


def sample_target(sigma_a, sigma_s, rand, throughput):
    """The homogeneous distance sample d* (the channel as the device picks it); inf without scattering."""
    return ref.sample_distance(sigma_a, sigma_s, rand, math.inf, throughput)[1] if np.asarray(sigma_s, np.float64).sum() > 0.0 else math.inf


def sample_distance(box_min, box_max, grid, sigma_a, sigma_s, rand, o, d, t0, t1, throughput):
    """(scattered, t of the vertex or inf, density length up to the vertex or over the whole interval, throughput')."""
    pieces = intervals(box_min, box_max, grid, o, d, t0, t1)
    D = sum(rho * (b - a) for a, b, rho, _, _ in pieces if rho > 0.0)
    if not D > 0.0:
        return False, math.inf, 0.0, np.asarray(throughput, np.float32).astype(np.float64)
    did, distance, weight = ref.sample_distance(sigma_a, sigma_s, rand, D, throughput)
    if not did:
        return False, math.inf, D, weight
    t, _, _ = invert(pieces, distance)
    return True, t, distance, weight


def shadow_factor(box_min, box_max, grid, sigma_t, o, d, max_distance):
    c = ref.clip(box_min, box_max, o, d, max_distance)
    if c is None:
        return np.ones(3), 0.0
    D = density_length(box_min, box_max, grid, o, d, c[0], c[1])
    return np.exp(-np.asarray(sigma_t, np.float64) * D), D


# ---- the light shaft through a grid dense in one half ------------------------------------------------------------------------------
# A 2 x 1 x 1 grid (rho_left for x below the box's middle, rho_right above it), one point light, a black sky, exactly one scattering event. The density
# length of a straight piece has a closed form here -- the piece is cut once, where it crosses the middle plane -- so neither the march nor the sorted
# crossings above are involved.

def halves_length(middle, rho, p0, p1):
    """Density length of the straight pieces p0 -> p1 ((N, 3) each, inside the box) through the two halves."""
    x0, x1 = p0[:, 0] - middle, p1[:, 0] - middle
    length = np.linalg.norm(p1 - p0, axis=1)
    r0 = np.where(x0 < 0, rho[0], rho[1]); r1 = np.where(x1 < 0, rho[0], rho[1])
    cut = (x0 < 0) != (x1 < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(cut, np.abs(x0) / (np.abs(x0) + np.abs(x1)), 1.0)
    return length * (r0 * f + r1 * (1.0 - f))


def _shaft_term(box_min, box_max, middle, rho, sigma_a, sigma_s, g, light, intensity, x, d):
    """phase x I / r^2 x T(shadow) at the points x (N, 3) of rays with directions d (N, 3) or (3,)."""
    to = light[None, :] - x
    r = np.linalg.norm(to, axis=1)
    to = to / r[:, None]
    _, s0, s1 = ref.clip_many(box_min, box_max, x, to, r)
    shadow = halves_length(middle, rho, x + s0[:, None] * to, x + s1[:, None] * to)
    return ref.hg(np.einsum("ij,ij->i", to, -np.broadcast_to(d, x.shape)), g) * intensity / (r * r) * np.exp(-(sigma_a + sigma_s) * shadow)


def shaft_quadrature_halves(box_min, box_max, rho, sigma_a, sigma_s, g, light, intensity, o, d, points=64):
    """The single-scatter radiance along ONE ray: Gauss-Legendre over each side of the middle plane (the integrand is smooth on either)."""
    box_min, box_max, light = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64), np.asarray(light, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    c = ref.clip(box_min, box_max, o, d, math.inf)
    if c is None:
        return 0.0
    middle = 0.5 * (box_min[0] + box_max[0])
    cuts = [c[0], c[1]]
    if d[0] != 0.0 and c[0] < (middle - o[0]) / d[0] < c[1]:
        cuts.insert(1, (middle - o[0]) / d[0])
    x, w = np.polynomial.legendre.leggauss(points)
    total = 0.0
    start = o + c[0] * d
    for a, b in zip(cuts[:-1], cuts[1:]):
        t = 0.5 * (b - a) * (x + 1.0) + a
        p = o[None, :] + t[:, None] * d[None, :]
        D = halves_length(middle, rho, np.broadcast_to(start, p.shape), p)
        here = np.where(p[:, 0] < middle, rho[0], rho[1])
        f = sigma_s * here * np.exp(-(sigma_a + sigma_s) * D) * _shaft_term(box_min, box_max, middle, rho, sigma_a, sigma_s, g, light, intensity, p, d)
        total += 0.5 * (b - a) * float((w * f).sum())
    return total


def shaft_monte_carlo_halves(box_min, box_max, rho, sigma_a, sigma_s, g, light, intensity, o, d, rng):
    """The device's estimator on N rays (o, d), scalar channel: d* by the exponential of sigma_t, a scatter event where the density length passes it, weight
    sigma_s / sigma_t, the light sample phase x I / r^2 x T(shadow). Returns the N sample values."""
    box_min, box_max, light = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64), np.asarray(light, np.float64)
    middle = 0.5 * (box_min[0] + box_max[0])
    st = sigma_a + sigma_s
    n = o.shape[0]
    ok, t0, t1 = ref.clip_many(box_min, box_max, o, d, np.inf)
    p0, p1 = o + t0[:, None] * d, o + t1[:, None] * d
    with np.errstate(divide="ignore", invalid="ignore"):
        tm = np.where(d[:, 0] != 0.0, (middle - o[:, 0]) / np.where(d[:, 0] != 0.0, d[:, 0], 1.0), np.inf)
    tm = np.where((tm > t0) & (tm < t1), tm, t1)   # the end of the first piece
    first = np.where(0.5 * (p0[:, 0] + (o + tm[:, None] * d)[:, 0]) < middle, rho[0], rho[1])
    second = np.where(first == rho[0], rho[1], rho[0])
    D1 = first * (tm - t0); D = D1 + second * (t1 - tm)
    s = -np.log(1.0 - rng.random(n)) / st
    scatter = ok & (s < D)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(s < D1, t0 + s / first, tm + (s - D1) / second)
    x = o + np.where(scatter, t, t0)[:, None] * d
    value = (sigma_s / st) * _shaft_term(box_min, box_max, middle, rho, sigma_a, sigma_s, g, light, intensity, x, d)
    return np.where(scatter, value, 0.0)


# ---- the march itself, restated operation by operation in float32 ------------------------------------------------------------------
# Not the reference (that is the sorted-crossings method above): the device's rules in numpy float32, so that the rules and the derived bounds can be
# checked against the reference without a GPU (test_fog_density.py).

F = np.float32


def _plane_distance(o, d, lo, hi, cell, n, i):
    if d == 0.0:
        return F(np.inf)
    plane = lo if i <= 0 else hi if i >= n else F(lo + F(F(i) * cell))
    with np.errstate(all="ignore"):
        return F(F(plane - o) / d)


def _cell_index(o, d, t, lo, cell, first, last):
    with np.errstate(all="ignore"):
        f = np.floor(F(F(F(o + F(t * d)) - lo) / cell))
    return last if f >= F(last) else int(f) if f > F(first) else first


def clip32(box_min, box_max, o, d, t_end):
    """fog_clip in float32: (t0, t1) or None."""
    t0, t1 = F(0.0), F(t_end)
    for k in range(3):
        ok, dk, lo, hi = F(o[k]), F(d[k]), F(box_min[k]), F(box_max[k])
        if dk == 0.0:
            if not (lo <= ok <= hi):
                return None
            continue
        with np.errstate(all="ignore"):
            ta, tb = F(F(lo - ok) / dk), F(F(hi - ok) / dk)
        t0 = F(np.fmax(t0, np.fmin(ta, tb))); t1 = F(np.fmin(t1, np.fmax(ta, tb)))
    return (t0, t1) if t1 > t0 else None


def march32(box_min, box_max, grid, o, d, t0, t1, target=math.inf, skip=True):
    """(scattered, t_scatter, density length, voxel steps, brick steps) of the float32 march; skip=False: no brick is taken as empty."""
    nz, ny, nx = grid.shape
    n = (nx, ny, nz)
    lo = [F(v) for v in box_min]; hi = [F(v) for v in box_max]
    o = [F(v) for v in o]; d = [F(v) for v in d]
    t0, t1, target = F(t0), F(t1), F(target)
    cell = [F(F(hi[k] - lo[k]) / F(n[k])) for k in range(3)]
    i = [_cell_index(o[k], d[k], t0, lo[k], cell[k], 0, n[k] - 1) for k in range(3)]
    t, D = t0, F(0.0)
    steps = [0, 0]
    for _ in range(nx + ny + nz + 3):
        b = [i[k] // 8 for k in range(3)]
        empty = skip and not (grid[b[2] * 8:b[2] * 8 + 8, b[1] * 8:b[1] * 8 + 8, b[0] * 8:b[0] * 8 + 8] > 0).any()
        p = [(min((b[k] + 1) * 8, n[k]) if empty else i[k] + 1) if d[k] > 0 else (b[k] * 8 if empty else i[k]) for k in range(3)]
        tk = [_plane_distance(o[k], d[k], lo[k], hi[k], cell[k], n[k], p[k]) for k in range(3)]
        t_exit = F(np.fmin(np.fmin(tk[0], tk[1]), np.fmin(tk[2], t1)))
        rho = F(0.0) if empty else F(grid[i[2], i[1], i[0]])
        steps[1 if empty else 0] += 1
        with np.errstate(all="ignore"):
            seg = F(np.fmax(F(t_exit - t), F(0.0)))
            D_next = F(D + F(rho * seg)) if rho > 0 else D
        if D_next > target:
            t_s = F(np.fmin(F(t + F(F(target - D) / rho)), t_exit))
            return True, float(t_s), float(F(D + F(rho * F(np.fmax(F(t_s - t), F(0.0)))))), steps[0], steps[1]
        D, t = D_next, t_exit
        if not t_exit < t1:
            break
        k = 0 if tk[0] == t_exit else 1 if tk[1] == t_exit else 2
        if empty:
            i[k] = p[k] if d[k] > 0 else p[k] - 1
            for j in range(3):
                if j != k:
                    i[j] = _cell_index(o[j], d[j], t, lo[j], cell[j], b[j] * 8, min(b[j] * 8 + 7, n[j] - 1))
        else:
            i[k] += 1 if d[k] > 0 else -1
        if i[k] < 0 or i[k] >= n[k]:
            break
    return False, math.inf, float(D), steps[0], steps[1]


def bricks(grid):
    """(number of 8 x 8 x 8 bricks, how many hold no density) of a (nz, ny, nx) grid, edge bricks partial."""
    nz, ny, nx = grid.shape
    total = empty = 0
    for z in range(0, nz, 8):
        for y in range(0, ny, 8):
            for x in range(0, nx, 8):
                total += 1
                empty += int(not (grid[z:z + 8, y:y + 8, x:x + 8] > 0).any())
    return total, empty
