"""The light tree of next-event estimation restated: the build in float32, bit for bit (leaves, Morton order, nodes), and in float64; the
importance, the descent and its pmf in float32 (the device's operations in the device's order: gpu-raytracer_amd/csrc/rt_light_tree.h, kernels_light_tree.hip)
and in float64; the pdfs of the two estimators of direct light (selection by power, selection by the tree) and their variance at a point.

A scene here is a `Scene`: what the device holds when it builds -- triangles (T, 24) float32 (position_0, edge_1, edge_2 in the first nine words), transforms
(I, 3, 4) float32 in the order of the instance tables, material_ids (I,), material_types (K,) uint8, materials (K, 8) float32 (emission in the first three words), the
light tables of rt_upload_lights (triangle_indices, spans (E, 2) inclusive, transform_indices (E,)) and position (None, or scene index -> row for a device-built TLAS).

Derived bounds (eps = 2^-24, one float32 rounding is eps / 2 relative):
  * leaf area. S: sum of |m_ij| |v_j| + |m_i3| over a row, the largest over the triangle's vertices and rows; L: the longest world edge. A world coordinate carries the
    rounding of the object-space sum v_0 + e (eps / 2 |v|, through the matrix: eps / 2 S) and of three products and three sums (at most 2.5 eps S): <= 3 eps S. An edge
    component: two of those and its own rounding: d_e = 6 eps S + eps L. A cross-product component: two products of two factors each off by d_e (4 L d_e) and three
    roundings (1.5 eps L^2). The norm of three of them and its own roundings (2 eps L^2), halved: |A32 - A64| <= 3.5 L d_e + 2.3 eps L^2 <= AREA_BOUND = 4 L d_e + 3 eps L^2.
  * leaf power: the luminance is three products and two sums of non-negative terms (2 eps relative), times A (eps / 2): |Phi32 - Phi64| <= AREA_BOUND * Y + 3 eps Phi64.
  * sum of the pmfs over all leaves at one point: at every inner node the two factors are P and fl(1 - P) = (1 - P)(1 + d), |d| <= eps / 2, so they sum to within
    eps / 2 of 1; every product along a path of `depth` factors rounds `depth` times. |sum - 1| <= 1.01 * depth * eps, plus what underflows (N * 2^-125).
  * device pmf against float64 on the same tree with the same branches: see pmf_bound.
"""
import numpy as np

F = np.float32
EPS = 2.0 ** -24
FLT_MIN, FLT_MAX = np.float32(np.finfo(np.float32).tiny), np.float32(np.finfo(np.float32).max)
FRESH_BELOW = F(2.0 ** -16)            # RT_LIGHT_TREE_FRESH_BELOW
ONE_BELOW_ONE = np.nextafter(F(1), F(0))
MATERIAL_LIGHT = 0
EMPTY_LO, EMPTY_HI = F(3.0e38), F(-3.0e38)


class Scene:
    def __init__(self, triangles, transforms, material_ids, material_types, materials, triangle_indices, spans, transform_indices, position=None):
        self.triangles = np.ascontiguousarray(triangles, F).reshape(-1, 24)
        self.transforms = np.ascontiguousarray(transforms, F).reshape(-1, 3, 4)
        self.material_ids = np.ascontiguousarray(material_ids, np.int32)
        self.material_types = np.ascontiguousarray(material_types, np.uint8)
        self.materials = np.ascontiguousarray(materials, F).reshape(-1, 8)
        self.triangle_indices = np.ascontiguousarray(triangle_indices, np.int32)
        self.spans = np.ascontiguousarray(spans, np.int32).reshape(-1, 2)
        self.transform_indices = np.ascontiguousarray(transform_indices, np.int32)
        self.position = None if position is None else np.ascontiguousarray(position, np.int32)

    def leaf_table(self):
        """entry, place in triangle_indices, triangle, instance row of every leaf id; leaf_base."""
        counts = self.spans[:, 1] - self.spans[:, 0] + 1
        base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        entry = np.repeat(np.arange(self.spans.shape[0]), counts)
        place = self.spans[entry, 0] + (np.arange(base[-1]) - base[entry])
        rows = self.transform_indices[entry]
        if self.position is not None:
            rows = self.position[rows]
        return entry.astype(np.int32), place.astype(np.int32), self.triangle_indices[place], rows.astype(np.int32), base


def _world(scene, dtype):
    """World-space vertices (N, 3 vertices, 3) of every leaf in `dtype` with the device's operation order, and the per-leaf luminance."""
    entry, place, tri, rows, base = scene.leaf_table()
    t = scene.triangles[tri].astype(dtype)
    v0 = t[:, 0:3]; v = np.stack([v0, v0 + t[:, 3:6], v0 + t[:, 6:9]], 1)
    m = scene.transforms[rows].astype(dtype)
    w = np.empty_like(v)
    for c in range(3):
        for d in range(3):
            w[:, c, d] = ((m[:, d, 0] * v[:, c, 0] + m[:, d, 1] * v[:, c, 1]) + m[:, d, 2] * v[:, c, 2]) + m[:, d, 3]
    mat = scene.material_ids[rows]
    e = scene.materials[mat, 0:3].astype(dtype)
    lum = (dtype(0.299) * e[:, 0] + dtype(0.587) * e[:, 1]) + dtype(0.114) * e[:, 2] if dtype is not np.float64 else (np.float64(F(0.299)) * e[:, 0] + np.float64(F(0.587)) * e[:, 1]) + np.float64(F(0.114)) * e[:, 2]
    lum = np.where(scene.material_types[mat] == MATERIAL_LIGHT, lum, dtype(0))
    return v, m, w, lum


def _area(w, dtype):
    e1 = w[:, 1] - w[:, 0]; e2 = w[:, 2] - w[:, 0]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]; ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]; nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return dtype(0.5) * np.sqrt((nx * nx + ny * ny) + nz * nz)


class Leaves:
    pass


def leaves32(scene):
    """The leaf records as the device computes them: box_lo, box_hi (N, 3), area, power (N,) float32, plus entry and triangle."""
    with np.errstate(all="ignore"):
        v, m, w, lum = _world(scene, F)
        out = Leaves()
        out.entry, _, out.triangle, out.rows, out.base = scene.leaf_table()
        out.lo = w.min(1); out.hi = w.max(1)
        area = _area(w, F)
        power = area * lum
        ok = (area > 0) & (area <= FLT_MAX) & (power > 0) & (power <= FLT_MAX)
        out.power = np.where(ok, power, F(0)).astype(F)
        out.area = np.where(area <= FLT_MAX, area, F(0)).astype(F)
    return out


def leaves64(scene):
    """area, power in float64 from the same float32 inputs, and the two bounds of the module docstring."""
    v, m, w, lum = _world(scene, np.float64)
    area = _area(w, np.float64)
    S = (np.abs(m[:, None, :, :3]) * np.abs(v[:, :, None, :])).sum(-1).max((1, 2)) + np.abs(m[:, :, 3]).max(1)
    L = np.max([np.linalg.norm(w[:, a] - w[:, b], axis=1) for a, b in ((1, 0), (2, 0), (2, 1))], 0)
    d_e = 6 * EPS * S + EPS * L
    area_bound = 4 * L * d_e + 3 * EPS * L * L
    power = area * lum
    return area, power, area_bound, area_bound * lum + 3 * EPS * power


def _expand_bits(v):
    v = v.astype(np.uint64)
    v = (v * np.uint64(0x00010001)) & np.uint64(0xFF0000FF)
    v = (v * np.uint64(0x00000101)) & np.uint64(0x0F00F00F)
    v = (v * np.uint64(0x00000011)) & np.uint64(0xC30C30C3)
    v = (v * np.uint64(0x00000005)) & np.uint64(0x49249249)
    return v


def morton_keys(lo, hi):
    """(30-bit Morton code of the box centre inside the box of all leaves) << 32 | leaf id, the float32 arithmetic of tlas_morton."""
    smin = lo.min(0); smax = hi.max(0)
    code = np.zeros(lo.shape[0], np.uint64)
    with np.errstate(all="ignore"):
        for d in range(3):
            extent = F(smax[d] - smin[d])
            centre = F(0.5) * (lo[:, d] + hi[:, d])
            t = (centre - smin[d]) / extent if extent > 0 else np.full(lo.shape[0], F(0.5))
            t = np.minimum(np.maximum(t * F(1024.0), F(0)), F(1023.0))
            code |= _expand_bits(t.astype(np.uint32)) << np.uint64(2 - d)
    return (code << np.uint64(32)) | np.arange(lo.shape[0], dtype=np.uint64)


class Tree:
    """leaf_count N, padded M, depth log2 M; nodes (2M - 1, 8) float32; order[s] = leaf id at sorted place s; slot_of_leaf[id] = M - 1 + s."""


def padded_size(n):
    m = 1
    while m < n:
        m *= 2
    return m


def build32(scene, leaves=None):
    """The tree bit for bit: the float32 restatement of kernels_light_tree.hip."""
    lv = leaves if leaves is not None else leaves32(scene)
    n = lv.area.size; m = padded_size(n)
    t = Tree(); t.leaf_count = n; t.padded = m; t.depth = m.bit_length() - 1; t.leaves = lv
    t.keys = morton_keys(lv.lo, lv.hi)
    t.order = np.argsort(t.keys, kind="stable").astype(np.int32)
    t.slot_of_leaf = np.empty(n, np.int32); t.slot_of_leaf[t.order] = m - 1 + np.arange(n, dtype=np.int32)
    nodes = np.zeros((2 * m - 1, 8), F)
    nodes[m - 1:, 0:3] = EMPTY_LO; nodes[m - 1:, 4:7] = EMPTY_HI
    nodes[m - 1:m - 1 + n, 0:3] = lv.lo[t.order]; nodes[m - 1:m - 1 + n, 3] = lv.power[t.order]; nodes[m - 1:m - 1 + n, 4:7] = lv.hi[t.order]
    count = m // 2
    while count >= 1:
        first = count - 1
        i = first + np.arange(count); l = 2 * i + 1; r = 2 * i + 2
        with np.errstate(all="ignore"):
            nodes[i, 3] = nodes[l, 3] + nodes[r, 3]
        lo = np.full((count, 3), EMPTY_LO, F); hi = np.full((count, 3), EMPTY_HI, F)
        for child in (l, r):
            live = (nodes[child, 3] > 0)[:, None]
            lo = np.where(live, np.minimum(lo, nodes[child, 0:3]), lo); hi = np.where(live, np.maximum(hi, nodes[child, 4:7]), hi)
        nodes[i, 0:3] = lo; nodes[i, 4:7] = hi
        count //= 2
    t.nodes = nodes
    return t


def tree_from_nodes(nodes, leaf_count, slot_of_leaf):
    """A Tree around nodes read back from the device (rt_read_light_tree), for the pmf functions below."""
    t = Tree(); t.nodes = np.ascontiguousarray(nodes, F).reshape(-1, 8); t.padded = (t.nodes.shape[0] + 1) // 2; t.leaf_count = leaf_count
    t.depth = t.padded.bit_length() - 1; t.slot_of_leaf = np.asarray(slot_of_leaf, np.int32)
    return t


# ---- importance, descent, pmf ----------------------------------------------------------------------------------------------------

def _importance(nodes, index, p, dtype):
    """Importance of nodes `index` (K,) seen from points p (K, 3), and their Phi, in dtype with the device's operation order."""
    nd = nodes[index].astype(dtype); p = p.astype(dtype)
    phi = nd[:, 3]
    with np.errstate(all="ignore"):
        c = dtype(0.5) * (nd[:, 0:3] + nd[:, 4:7]); h = dtype(0.5) * (nd[:, 4:7] - nd[:, 0:3]); d = p - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r2 = (h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) + h[:, 2] * h[:, 2]
        denominator = np.maximum(np.maximum(d2, r2), dtype(FLT_MIN))
        value = np.where(phi > 0, phi / denominator, dtype(0))
    return value, phi, d, c, d2, r2, denominator


def left32(tree, node, p):
    """P_left at inner nodes `node` (K,) from p (K, 3) in float32: (probability, or -1 where nothing below has power; whether the Phi ratio was used)."""
    with np.errstate(all="ignore"):
        il, pl = _importance(tree.nodes, 2 * node + 1, p, F)[:2]
        ir, pr = _importance(tree.nodes, 2 * node + 2, p, F)[:2]
        s = il + ir
        fallback = ~((s > 0) & (s <= FLT_MAX))
        s2 = pl + pr
        dead = fallback & ~((s2 > 0) & (s2 <= FLT_MAX))
        left = np.where(fallback, pl / s2, il / s)
    return np.where(dead, F(-1), left).astype(F), fallback


def sample32(tree, p, u, u2):
    """light_tree_sample on K probes: (slot, pmf) float32 restatement."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3); k = p.shape[0]
    u = np.broadcast_to(np.asarray(u, F), (k,)).copy(); u2 = np.broadcast_to(np.asarray(u2, F), (k,))
    node = np.zeros(k, np.int64); pmf = np.ones(k, F); first = np.ones(k, bool); alive = np.full(k, bool(tree.nodes[0, 3] > 0))
    for _ in range(tree.depth):
        left, _ = left32(tree, node, p)
        alive &= left >= 0
        with np.errstate(all="ignore"):
            go_left = u < left
            right = F(1) - left
            u = np.where(go_left, u / left, (u - left) / right).astype(F)
            pmf = (pmf * np.where(go_left, left, right)).astype(F)
        node = 2 * node + np.where(go_left, 1, 2)
        u = np.minimum(u, ONE_BELOW_ONE)
        switch = first & (pmf < FRESH_BELOW)
        u = np.where(switch, u2, u); first &= ~switch
    return np.where(alive, node, -1), np.where(alive, pmf, F(0))


def _path(tree, slot):
    """The nodes from the root down to the parents of `slot` (K,), and whether each step goes right: (depth, K) each."""
    path = np.asarray(slot, np.int64) + 1
    nodes = np.zeros((tree.depth, path.size), np.int64); rights = np.zeros((tree.depth, path.size), bool)
    node = np.zeros(path.size, np.int64)
    for level in range(tree.depth):
        right = ((path >> (tree.depth - 1 - level)) & 1).astype(bool)
        nodes[level] = node; rights[level] = right
        node = 2 * node + 1 + right
    return nodes, rights


def pmf32(tree, p, slot):
    """light_tree_pmf, float32 restatement: the same factors in the same order as sample32."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    nodes, rights = _path(tree, np.broadcast_to(slot, (p.shape[0],)))
    pmf = np.ones(p.shape[0], F); alive = np.full(p.shape[0], bool(tree.nodes[0, 3] > 0))
    for level in range(tree.depth):
        left, _ = left32(tree, nodes[level], p)
        alive &= left >= 0
        pmf = (pmf * np.where(rights[level], F(1) - left, left)).astype(F)
    return np.where(alive, pmf, F(0))


def pmf64(tree, p, slot):
    """The pmf in float64 on the float32 nodes, taking at every node the branch (importance or Phi ratio) the float32 walk takes, and the first-order bound of
    the float32 walk's difference from it.

    pmf_bound. A node's denominator D = max(d^2, r^2, FLT_MIN): the centre rounds once (eps / 2 |c|), the difference p - c once more (eps / 2 |d|), so a component of d
    is off by dd = eps / 2 (|c| + |d|); d^2 by 2 |d| . dd + |dd|^2 and three roundings (1.5 eps d^2); r^2 by 2.5 eps r^2 (exact halves, differences rounded once).
    rho = dD / D + eps bounds the relative error of an importance (the quotient rounds once). P = I_l / (I_l + I_r) is off by at most P (1 - P)(rho_l + rho_r) + 1.5 eps
    absolutely (the sum, the quotient and 1 - P each round once, all below 1); with the Phi ratio rho = 0. The product of `depth` factors adds their relative errors
    and depth * eps / 2 of its own roundings; the bound returned is 1.5 x that first-order sum (second-order terms: the tests keep rho below 1/4) times the float64 pmf.
    Returns (pmf, bound, largest rho met)."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    nodes, rights = _path(tree, np.broadcast_to(slot, (p.shape[0],)))
    pmf = np.ones(p.shape[0]); relative = np.zeros(p.shape[0]); worst_rho = 0.0
    alive = np.full(p.shape[0], bool(tree.nodes[0, 3] > 0))
    for level in range(tree.depth):
        left32_, fallback = left32(tree, nodes[level], p)
        alive &= left32_ >= 0
        rho = []
        vals = []
        for child in (2 * nodes[level] + 1, 2 * nodes[level] + 2):
            value, phi, d, c, d2, r2, den = _importance(tree.nodes, child, p, np.float64)
            dd = EPS / 2 * (np.abs(c) + np.abs(d))
            err_d2 = (2 * np.abs(d) * dd + dd * dd).sum(1) + 1.5 * EPS * d2
            err = np.where(d2 >= r2, err_d2, np.maximum(2.5 * EPS * r2, np.where(d2 + err_d2 > r2, err_d2, 0.0)))
            r = np.where(phi > 0, err / den + EPS, 0.0)
            rho.append(np.where(fallback, 0.0, r)); vals.append(np.where(fallback, phi, value))
        with np.errstate(all="ignore"):
            total = vals[0] + vals[1]
            left = np.where(total > 0, vals[0] / total, 0.0)
        factor = np.where(rights[level], 1.0 - left, left)
        absolute = left * (1.0 - left) * (rho[0] + rho[1]) + 1.5 * EPS
        with np.errstate(all="ignore"):
            relative += np.where(factor > 0, absolute / factor, 0.0) + EPS / 2
        pmf *= factor
        worst_rho = max(worst_rho, float(np.max(rho[0], initial=0.0)), float(np.max(rho[1], initial=0.0)))
    pmf = np.where(alive, pmf, 0.0)
    return pmf, 1.5 * relative * pmf + 2.0 ** -140, worst_rho


def all_pmfs(tree, point, fn=pmf32):
    """The pmf of every leaf id at one point."""
    return fn(tree, np.broadcast_to(np.asarray(point, F), (tree.leaf_count, 3)), tree.slot_of_leaf)


def sum_bound(tree):
    return 1.01 * tree.depth * EPS + tree.leaf_count * 2.0 ** -125


def selection_tolerance(tree):
    """Counts of one leaf over 2^16 equally spaced u against 2^16 pmf: an interval of width w holds between 2^16 w - 1 and 2^16 w + 1 grid points; each of its ends
    drifts by at most 1.5 eps per level in u (the rescale's three roundings, below 1 in absolute terms, mapped back through intervals no wider than 1), and the
    float32 pmf differs from the interval's width by depth * eps relative. (Below a node reached with probability < 2^-16 the descent goes on with u2: at most one
    grid point reaches it, and lands on one leaf.) In counts: 2 + 2^16 (3 eps depth + eps depth)."""
    return 2.0 + 2.0 ** 16 * 4 * EPS * tree.depth


# ---- the two estimators of direct light at a point ---------------------------------------------------------------------------------

def power_pmf(scene, leaves):
    """Selection by power alone, as the cumulative tables of rt_upload_lights make it: Y area scale^2 per mesh entry, area within it. Here: proportional to the float64 power."""
    _, power, _, _ = leaves64(scene)
    return power / power.sum()


def emitter_pdfs(scene, tree, point, normal=None):
    """For a diffuse receiver at `point` (normal up by default) and every leaf, with the triangle's centroid standing for its points: the unoccluded contribution
    c_k = f L cos cos A / d^2 of the whole leaf, and the two selection pmfs. Returns (c, pmf_power, pmf_tree)."""
    v, m, w, lum = _world(scene, np.float64)
    area = _area(w, np.float64)
    centroid = w.mean(1)
    e1 = w[:, 1] - w[:, 0]; e2 = w[:, 2] - w[:, 0]
    n = np.cross(e1, e2); length = np.linalg.norm(n, axis=1); n = n / np.where(length > 0, length, 1.0)[:, None]
    normal = np.array([0.0, 1.0, 0.0]) if normal is None else np.asarray(normal, np.float64)
    to = centroid - np.asarray(point, np.float64); d2 = (to * to).sum(1); to = to / np.sqrt(d2)[:, None]
    cos_hit = np.maximum(to @ normal, 0.0); cos_light = np.abs((to * n).sum(1))
    c = lum * cos_hit * cos_light * area / d2 / np.pi
    power = area * lum
    return c, power / power.sum(), all_pmfs(tree, point, lambda t, p, s: pmf64(t, p, s)[0])


def estimator_moments(scene, tree, points, power_selection, normal=None, q=4):
    """First and second moment of ONE light sample c(p, x) / (pmf_k(p) / A_k) for a diffuse receiver: p uniform over `points` (the pixel's footprint on the receiver),
    leaf k by the tree's pmf at p (or, power_selection, by power), x uniform on the triangle (a q x q stratified grid of the unit square folded onto it), c = f L cos cos / d^2,
    unoccluded. The variance within a triangle and within the footprint is in it, divided by each selection's own pmf: E[X^2] = mean_p sum_k A_k^2 mean_x c^2 / pmf_k(p)."""
    import nee_reference
    v, m, w, lum = _world(scene, np.float64)
    area = _area(w, np.float64)
    n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]); n = n / np.where(area > 0, 2 * area, 1.0)[:, None]
    normal = np.array([0.0, 1.0, 0.0]) if normal is None else np.asarray(normal, np.float64)
    g = (np.arange(q) + 0.5) / q
    a, b = nee_reference.sample_triangle(np.repeat(g, q), np.tile(g, q))
    x = w[:, None, 0] + a[None, :, None] * (w[:, None, 1] - w[:, None, 0]) + b[None, :, None] * (w[:, None, 2] - w[:, None, 0])   # (N, q^2, 3)
    power = area * lum
    first = second = 0.0
    for point in np.asarray(points, np.float64).reshape(-1, 3):
        to = x - point; d2 = (to * to).sum(-1); to = to / np.sqrt(d2)[..., None]
        c = lum[:, None] * np.maximum(to @ normal, 0.0) * np.abs((to * n[:, None]).sum(-1)) / d2 / np.pi * area[:, None]   # the integrand times A: what / pmf makes the sample
        pmf = power / power.sum() if power_selection else all_pmfs(tree, point, lambda t, p, s_: pmf64(t, p, s_)[0])
        live = (c > 0).any(1)
        assert (pmf[live] > 0).all()
        first += c.mean(1).sum(); second += ((c[live] ** 2).mean(1) / pmf[live]).sum()
    k = np.asarray(points).reshape(-1, 3).shape[0]
    return first / k, second / k


def selection_variance(c, pmf):
    """Variance of the one-sample estimator c_k / pmf_k of sum c_k when leaf k is drawn with probability pmf_k (the part of the direct-light variance that the
    selection makes; the point on the triangle adds the same to both selections to first order)."""
    live = c > 0
    assert (pmf[live] > 0).all()
    return float((c[live] ** 2 / pmf[live]).sum() - c.sum() ** 2)


# ---- the launches, entry by entry: what stands in for the power tables in the float64 restatements of the material and sort launches ----

class PerEntry(float):
    """A `lights_total_weight` per entry. The restatements of the material and sort launches (material_reference.py, sort_reference.py) compute an emitter's pdf as
    Y d^2 / (cos x lights_total_weight); with W_i = Y_i A_i / pmf_i in its place that is pmf_i d^2 / (A_i cos), the tree's. Compares as a positive number, multiplies
    as the array (numpy defers to __rmul__ / __mul__ because __array_ufunc__ is None)."""
    __array_ufunc__ = None

    def __new__(cls, values):
        self = float.__new__(cls, 1.0)
        self.values = np.asarray(values, np.float64)
        return self

    def __mul__(self, other):
        return self.values * other

    __rmul__ = __mul__


def leaf_of_slot(tree):
    out = np.full(2 * tree.padded - 1, -1, np.int64); out[tree.slot_of_leaf] = np.arange(tree.leaf_count)
    return out


def pick_leaves(tree, positions, u, u2, ulps=64):
    """The leaf light_tree_sample picks for each entry from float32(positions), its float64 pmf there, and whether the pick is robust: the same leaf for u moved by
    `ulps` float32 spacings of 1 either way (the device's hit point differs from float64's by a few ulps, which moves every P_left by less than that)."""
    p = np.ascontiguousarray(positions, F).reshape(-1, 3)
    u = np.asarray(u, F); u2 = np.asarray(u2, F)
    slot, _ = sample32(tree, p, u, u2)
    step = F(ulps * 2.0 ** -24)
    lower, _ = sample32(tree, p, np.maximum(u - step, F(0)), u2); upper, _ = sample32(tree, p, np.minimum(u + step, ONE_BELOW_ONE), u2)
    lower2, _ = sample32(tree, p, u, np.maximum(u2 - step, F(0))); upper2, _ = sample32(tree, p, u, np.minimum(u2 + step, ONE_BELOW_ONE))
    robust = (slot == lower) & (slot == upper) & (slot == lower2) & (slot == upper2) & (slot >= 0)
    pmf = pmf64(tree, p, np.maximum(slot, 0))[0]
    return leaf_of_slot(tree)[np.maximum(slot, 0)], np.where(slot >= 0, pmf, 0.0), robust


def lights_on_leaves(scene, leaf, rand_triangle):
    """nee_reference.sample_lights' result (point, normal, emission in float64) for given leaves: the point from the DIM_NEE_TRIANGLE pair as nee_pick_light takes it."""
    import nee_reference
    entry, place, tri_id, rows, base = scene.leaf_table()
    r = nee_reference.Picked()
    r.triangle = tri_id[leaf]; r.transform_id = rows[leaf]
    uv = np.asarray(rand_triangle, F).astype(np.float64)
    a, b = nee_reference.sample_triangle(uv[:, 0], uv[:, 1])
    tri = scene.triangles[r.triangle].astype(np.float64)
    p0, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    m = scene.transforms[r.transform_id].astype(np.float64)
    r.point = np.einsum("nij,nj->ni", m[:, :, :3], p0 + a[:, None] * e1 + b[:, None] * e2) + m[:, :, 3]
    normal = np.einsum("nij,nj->ni", m[:, :, :3], np.cross(e1, e2))
    with np.errstate(invalid="ignore", divide="ignore"):
        r.normal = normal / np.linalg.norm(normal, axis=1)[:, None]
    r.emission = scene.materials[scene.material_ids[r.transform_id], :3].astype(np.float64)
    return r


def leaf_of_hit(scene, mesh, triangle):
    """The leaf id of a hit (instance row, triangle id), -1 where it is no leaf: the inverse tables' job."""
    entry, place, tri_id, rows, base = scene.leaf_table()
    table = {(int(r), int(t)): k for k, (r, t) in reversed(list(enumerate(zip(rows, tri_id))))}
    return np.array([table.get((int(m), int(t)), -1) for m, t in zip(mesh, triangle)], np.int64)
