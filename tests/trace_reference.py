"""Float64 brute-force ray casting, and which rays float32 traversal must get exactly right. TEST INFRASTRUCTURE ONLY.

Shares nothing with the oracle or the kernels: Moeller-Trumbore in float64 over every triangle of a scene given as world-space
vertices, vectorised over (ray, triangle) pairs in chunks. For each ray it returns the closest hit and its triangle, the
closest hit of any other triangle, the barycentric margin and a grazing measure of the hit, and the nearest intersection that
float32 arithmetic could get wrong either way (see `Tolerances`).

Robust rays (`robust_closest`, `robust_shadow`) are those whose answer no float32 implementation of the same operation may
change: their hit is clear of every triangle edge, not grazing, clear of the runner-up, not at t ~ 0 and (shadow rays) not at
the maximum distance. Every tolerance is a multiple of the float32 unit roundoff times the condition of the quantity, named in
`Tolerances` with the worst case measured over tests/trace_cases.py (tests/test_trace_reference.py prints them).
"""
from dataclasses import dataclass

import numpy as np

EPS32 = 2.0 ** -24


@dataclass(frozen=True)
class Tolerances:
    # All in units of EPS32 x (the condition of the quantity). The coordinate scale S of a ray / triangle pair is
    # max(|origin|, |vertex 0|, |t * direction|) (infinity norms): the float32 operands of Moeller-Trumbore are of that size.
    #  t:       |t32 - t64| <= T x EPS32 x S / (g |d|), g the grazing measure |det| / (|e1| |e2| |d|).
    #           Measured worst case over the cases (robust rays): 6.4 (the nested shells of `deep`; 3.6 elsewhere).
    T: float = 8.0
    #  u, v:    |u32 - u64| <= UV x EPS32 x S / (g L), L = sqrt(|e1| |e2|); the stored 16-bit u, v add 1 / 65535.
    #           Measured worst case beyond the 1 / 65535: 1.4 (instanced_many).
    UV: float = 8.0
    # A hit is robust when its barycentric margin is at least MARGIN x the u, v bound, its grazing measure at least
    # GRAZING, the next other intersection (and the nearest ambiguous one) further than GAP x the t bound, and its t
    # at least GAP x the t bound. A shadow ray is robust when no ambiguous intersection lies before its limit and the
    # nearest hit is not within GAP x the t bound of the limit.
    MARGIN: float = 4.0 * 8.0
    GRAZING: float = 1e-4
    # Moeller-Trumbore's determinant and t's numerator (t x det) are products of three float32 lengths: below 2^-126 they are
    # subnormal or zero and the triangle is lost or its t imprecise (triangles of ~1e-13 and below). A hit where either is below
    # DET_MIN is ambiguous, and a traversal's t for it is only checked to name a real intersection.
    DET_MIN: float = 2.0 ** -100
    # A shadow ray is not robust when an ambiguous intersection lies before its limit times (1 + LIMIT_REL): the t of an
    # ambiguous pair has no bound of its own (a ray through a vertex of a closed mesh: float64 may miss every triangle there).
    LIMIT_REL: float = 1e-4
    GAP: float = 4.0 * 8.0


TOL = Tolerances()


@dataclass
class BruteForce:
    t: np.ndarray          # float64 (N,): closest hit (inf: none)
    index: np.ndarray      # int64 (N,): its triangle (-1: none)
    t_second: np.ndarray   # float64 (N,): closest hit of any other triangle (inf: none)
    margin: np.ndarray     # float64 (N,): min(u, v, 1 - u - v) of the hit
    grazing: np.ndarray    # float64 (N,): |det| / (|e1| |e2| |d|) of the hit
    u: np.ndarray
    v: np.ndarray
    t_tol: np.ndarray      # float64 (N,): the t bound of the hit (TOL.T)
    uv_tol: np.ndarray     # float64 (N,): the u, v bound of the hit (TOL.UV)
    t_ambiguous: np.ndarray  # float64 (N,): nearest intersection float32 may accept or reject either way (inf: none)
    t_clear: np.ndarray    # float64 (N,): nearest hit that is not ambiguous (inf: none): no float32 traversal may go past it
    t_tiny: np.ndarray     # float64 (N,): nearest hit on which float32 underflows (TOL.DET_MIN; inf: none): its float32 t is arbitrary


def intersect_pairs(o, d, p0, e1, e2):
    """Moeller-Trumbore in float64 for every (ray, triangle) pair. o, d: (N, 3); p0, e1, e2: (K, 3).
    Returns t, u, v, grazing, scale, size (each (N, K)); t is NaN where det == 0."""
    h = np.cross(d[:, None, :], e2[None, :, :])
    det = np.einsum("kj,nkj->nk", e1, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / det
        s = o[:, None, :] - p0[None, :, :]
        u = f * np.einsum("nkj,nkj->nk", s, h)
        q = np.cross(s, e1[None, :, :])
        v = f * np.einsum("nj,nkj->nk", d, q)
        t = f * np.einsum("kj,nkj->nk", e2, q)
    n1, n2, nd = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1), np.linalg.norm(d, axis=1)
    denom = n1[None, :] * n2[None, :] * nd[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        grazing = np.where(denom > 0, np.abs(det) / denom, 0.0)
    scale = np.maximum(np.abs(o).max(1)[:, None], np.abs(p0).max(1)[None, :])
    with np.errstate(invalid="ignore"):
        scale = np.maximum(scale, np.nan_to_num(np.abs(t), posinf=0.0) * np.abs(d).max(1)[:, None])
    size = np.sqrt(n1 * n2)[None, :]
    grazing = np.where(np.abs(det) >= TOL.DET_MIN, grazing, 0.0)   # (lost to float32 underflow: treated as degenerate -- ambiguous below)
    return t, u, v, grazing, scale, size, nd[:, None], np.abs(det)


def brute_force(origin, direction, world, chunk_pairs=1 << 21):
    """origin, direction: (3, N) (any float type); world: (K, 3, 3) triangle vertices. Returns a BruteForce."""
    o = np.ascontiguousarray(np.asarray(origin, np.float64).T)
    d = np.ascontiguousarray(np.asarray(direction, np.float64).T)
    w = np.asarray(world, np.float64)
    p0, e1, e2 = w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]
    n, k = o.shape[0], w.shape[0]
    out = {name: np.full(n, np.inf) for name in ("t", "t_second", "t_ambiguous", "t_clear", "t_tiny")}
    for name in ("margin", "grazing", "u", "v", "t_tol", "uv_tol"):
        out[name] = np.zeros(n)
    out["index"] = np.full(n, -1, np.int64)
    rows = max(1, chunk_pairs // max(k, 1))
    for a in range(0, n, rows):
        b = min(n, a + rows)
        t, u, v, g, scale, size, nd, det = intersect_pairs(o[a:b], d[a:b], p0, e1, e2)
        with np.errstate(invalid="ignore"):
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_tol = TOL.T * EPS32 * scale / (g * nd)
            uv_tol = TOL.UV * EPS32 * scale / (g * size)
        finite = np.isfinite(t) & (g > 0)
        valid = np.isfinite(t) & (det > 0) & (margin >= 0) & (t > 0)
        with np.errstate(invalid="ignore"):
            tiny = np.isfinite(t) & (det > 0) & ((g == 0) | (np.abs(t) * det < TOL.DET_MIN)) & (margin >= 0) & (t > 0)   # a hit float32 may lose to underflow
            g = np.where(tiny, 0.0, g)
        # could float32 flip this pair's test? near an edge, grazing, or at t ~ 0
        ambiguous = finite & (margin >= -TOL.MARGIN / TOL.UV * uv_tol) & (t > -TOL.GAP / TOL.T * t_tol) & \
            ((margin < TOL.MARGIN / TOL.UV * uv_tol) | (g < TOL.GRAZING) | (t < TOL.GAP / TOL.T * t_tol))
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
    return BruteForce(**out)


def robust_closest(bf):
    """Rays whose closest hit (or miss) every float32 Moeller-Trumbore over the same triangles must reproduce."""
    hit = np.isfinite(bf.t)
    clear = (bf.margin >= TOL.MARGIN / TOL.UV * bf.uv_tol) & (bf.grazing >= TOL.GRAZING) & (bf.t >= TOL.GAP / TOL.T * bf.t_tol)
    gap = TOL.GAP / TOL.T * bf.t_tol
    with np.errstate(invalid="ignore"):   # (inf - inf: a miss, decided below)
        alone = (bf.t_second - bf.t > gap) & (bf.t_ambiguous - bf.t > gap)
    return np.where(hit, clear & alone, ~np.isfinite(bf.t_ambiguous))


def occluded(bf, max_distance):
    """Float64 occlusion: some hit with 0 < t < max_distance."""
    return bf.t < np.asarray(max_distance, np.float64)


def robust_shadow(bf, max_distance):
    m = np.asarray(max_distance, np.float64)
    gap = np.where(np.isfinite(bf.t), TOL.GAP / TOL.T * bf.t_tol, 0.0)
    with np.errstate(invalid="ignore"):   # (inf - inf)
        near_limit = np.isfinite(bf.t) & (np.abs(bf.t - m) <= gap)
    return ~near_limit & ~(bf.t_ambiguous < m * (1 + TOL.LIMIT_REL) + gap) & (robust_closest(bf) | ~(bf.t < m + gap)) & ~np.isfinite(bf.t_tiny)


def evaluate_named(origin, direction, hits_world):
    """Float64 Moeller-Trumbore of each ray against ONE triangle each (the one a traversal named): t, margin, grazing,
    t bound, u, v, u, v bound, and whether float32 underflows on it (TOL.DET_MIN). hits_world: (N, 3, 3)."""
    o = np.asarray(origin, np.float64).T
    d = np.asarray(direction, np.float64).T
    w = np.asarray(hits_world, np.float64)
    p0, e1, e2 = w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]
    h = np.cross(d, e2)
    det = (e1 * h).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / det
        s = o - p0
        u = f * (s * h).sum(1)
        q = np.cross(s, e1)
        v = f * (d * q).sum(1)
        t = f * (e2 * q).sum(1)
        nd = np.linalg.norm(d, axis=1)
        g = np.abs(det) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * nd)
        scale = np.maximum(np.maximum(np.abs(o).max(1), np.abs(p0).max(1)), np.abs(t) * np.abs(d).max(1))
        t_tol = TOL.T * EPS32 * scale / (g * nd)
        uv_tol = TOL.UV * EPS32 * scale / (g * np.sqrt(np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)))
        margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
        tiny = (np.abs(det) < TOL.DET_MIN) | (np.abs(t * det) < TOL.DET_MIN)
    return t, margin, g, t_tol, u, v, uv_tol, tiny


def world_triangles_of_hits(triangles, transforms, mesh_id, triangle_id):
    """World-space vertices (N, 3, 3) of the triangles hit records name: the product's own staging arrays (triangles: (T, 24)
    position_0, edge_1, edge_2, ...; transforms: (M, 12) object -> world rows), evaluated in float64."""
    tri = np.asarray(triangles, np.float64).reshape(-1, 24)[triangle_id]
    v = np.stack([tri[:, 0:3], tri[:, 0:3] + tri[:, 3:6], tri[:, 0:3] + tri[:, 6:9]], 1)
    m = np.asarray(transforms, np.float64).reshape(-1, 3, 4)[mesh_id]
    return np.einsum("nij,nkj->nki", m[:, :, :3], v) + m[:, None, :, 3]
