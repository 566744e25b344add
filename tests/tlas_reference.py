"""What a TLAS of the device build has to be, checked in float64 from the 80-byte nodes alone. TEST INFRASTRUCTURE ONLY.

Nothing of the product or of its restatement (oracle/oracle_tlas.cpp) is used: the nodes are decoded here, the instances' world
boxes come from the eight corners in float64, and the only float32 arithmetic restated is what DEFINES a node's grid -- the
corner sums ((r0 x + r1 y) + r2 z) + r3 and the exponent rule.

  structure     `order` is a permutation; inner children sit in consecutive node slots from base_child in slot order, leaves at
                consecutive positions from base_leaf in slot order; meta bytes as the traversal reads them; every node used.
  containment   a decoded child box contains the float64 world box of every instance below it within SLACK: per coordinate
                4 * 2^-24 * (|r0 x| + |r1 y| + |r2 z| + |r3|), the bound of a four-term float32 sum (worst corner).
  thickness     every filled slot has q_hi > q_lo in all three axes: the traversal's node test is `tmin < tmax`, a child box of
                zero thickness is never entered.
  tightness     a child box sticks out of the float64 box of what is below it by less than one grid step of its node per
                side plus the slack; by one step more only on the side the thickness rule widened (q_hi - q_lo == 1).
  exponents     exactly: per axis the smallest power of two >= float32(extent * float32(1 / 255)), biased exponent clamped to
                1 .. 254, the extent float32(max - min) of the float32 union of the world boxes below the node, floored at 2^-11 of
                the largest coordinate of the scene box (and at 1e-30). The floor is what keeps the thickness rule meaningful: a
                node of coplanar children has extent 0, a grid over 1e-30 has steps of 1e-32, and a child box one such step thick
                is as lost to a float32 node test as a flat one (6 of the 200 tiles of `flat_tiles_200` were, under such nodes).
"""
import numpy as np

U32 = 2.0 ** -24


def corner_terms(transforms, local_boxes):
    """(n, 8, 3, 4): the four terms r0 x, r1 y, r2 z, r3 of every world coordinate of every box corner, in the dtype given."""
    t = np.asarray(transforms).reshape(-1, 3, 4); b = np.asarray(local_boxes).reshape(-1, 2, 3)
    corners = np.stack([np.stack([b[:, (c >> d) & 1, d] for d in range(3)], axis=1) for c in range(8)], axis=1)   # (n, 8, 3)
    products = t[:, None, :, :3] * corners[:, :, None, :]
    return np.concatenate([products, np.broadcast_to(t[:, None, :, 3:], products.shape[:3] + (1,))], axis=3)


def world_boxes64(transforms, local_boxes):
    """((n, 2, 3) float64 world boxes, (n, 3) slack)."""
    terms = corner_terms(np.asarray(transforms, np.float64), np.asarray(local_boxes, np.float64))
    world = terms.sum(axis=3)
    slack = 4 * U32 * np.abs(terms).sum(axis=3).max(axis=1)
    return np.stack([world.min(axis=1), world.max(axis=1)], axis=1), slack


def world_boxes32(transforms, local_boxes):
    """(n, 2, 3) float32 world boxes as the build defines them: each coordinate summed left to right in float32. (Which of two
    equal zeros a bound keeps is not restated: the sign of a zero changes no extent.)"""
    terms = corner_terms(np.asarray(transforms, np.float32), np.asarray(local_boxes, np.float32))
    with np.errstate(over="ignore", under="ignore"):
        world = ((terms[..., 0] + terms[..., 1]) + terms[..., 2]) + terms[..., 3]
    return np.stack([world.min(axis=1), world.max(axis=1)], axis=1)


def decode(nodes):
    """(count, 80) uint8 -> origin (count, 3) f32, biased exponents (count, 3), imask, base_child, base_leaf, meta (count, 8),
    q (count, 3 axes, 2 (lo, hi), 8 slots)."""
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 80)
    words = nodes.view(np.uint32).reshape(-1, 20)
    origin = words[:, 0:3].copy().view(np.float32)
    exponents = np.stack([(words[:, 3] >> (8 * d)) & 0xff for d in range(3)], axis=1).astype(np.int64)
    return origin, exponents, (words[:, 3] >> 24) & 0xff, words[:, 4].astype(np.int64), words[:, 5].astype(np.int64), nodes[:, 24:32], nodes[:, 32:80].reshape(-1, 3, 2, 8)


def structure(nodes, order):
    """Asserts the structural rules and returns per node the list of (slot, child node or -1, instances below as an int array),
    and the nodes level by level."""
    n = len(order)
    order = np.asarray(order)
    assert sorted(order.tolist()) == list(range(n)), "order is not a permutation"
    _, _, imask, base_child, base_leaf, meta, _ = decode(nodes)
    count = len(imask)
    assert count >= 1
    children = [None] * count
    seen_leaves = np.zeros(n, bool)
    levels = [[0]]
    used = 1
    while levels[-1]:
        below = []
        for k in levels[-1]:
            entry = []; inner_rank = 0; leaf_rank = 0
            for s in range(8):
                m = int(meta[k, s])
                if m == 0:
                    assert not (imask[k] >> s) & 1, "an imask bit names an empty slot"
                    continue
                if (imask[k] >> s) & 1:
                    assert m == (0x20 | (24 + s)), (k, s, m)
                    child = int(base_child[k]) + inner_rank; inner_rank += 1
                    assert child == used and child < count, "inner children are not consecutive in level and slot order"   # (breadth-first numbering)
                    used += 1
                    below.append(child); entry.append((s, child, None))
                else:
                    assert (m >> 5) == 1 and (m & 31) == leaf_rank and leaf_rank < 24, (k, s, m)
                    position = int(base_leaf[k]) + leaf_rank; leaf_rank += 1
                    assert position < n and not seen_leaves[position], (k, s, position)
                    seen_leaves[position] = True
                    entry.append((s, -1, np.array([order[position]], np.int64)))
            assert entry, "a node without children"
            children[k] = entry
        levels.append(below)
    levels.pop()
    assert used == count and seen_leaves.all(), "nodes or instances left over"
    for level in reversed(levels):     # the instances below every inner child
        for k in level:
            children[k] = [(s, c, inst if c < 0 else np.concatenate([i for _, _, i in children[c]])) for s, c, inst in children[k]]
    return children, levels


def level_widths(nodes):
    """Nodes per level, breadth-first over imask and base_child alone."""
    _, _, imask, base_child, _, _, _ = decode(nodes)
    widths = []; level = [0]
    while level:
        widths.append(len(level))
        level = [int(base_child[k]) + r for k in level for r in range(bin(int(imask[k])).count("1"))]
    return widths


def extent_floor(boxes32):
    """The least extent a node's grid is laid over: 2^-11 of the largest coordinate of the scene box, at least 1e-30."""
    with np.errstate(under="ignore"):
        return np.maximum(np.float32(np.abs(boxes32).max()) * np.float32(2.0 ** -11), np.float32(1.0e-30))


def expected_exponents(lo32, hi32, floor):
    """The exponent rule on the float32 union (lo32, hi32: (3,) float32) of what is below a node."""
    with np.errstate(over="ignore", under="ignore"):
        extent = np.maximum((hi32 - lo32).astype(np.float32), floor)
        scaled = (extent * (np.float32(1.0) / np.float32(255.0))).astype(np.float32)
    bits = scaled.view(np.uint32).astype(np.int64)
    exponent = (bits >> 23) + ((bits & 0x7fffff) != 0)
    return np.clip(exponent, 1, 254)


class Findings:
    """What a run measured: the largest containment error in units of the slack, and the child boxes the thickness rule widened."""
    def __init__(self):
        self.containment_in_slacks = 0.0; self.flat = 0; self.widened = 0; self.children = 0


def check(nodes, order, transforms, local_boxes, require_thickness=True):
    """All of the above on one TLAS. Returns Findings; with require_thickness=False flat child boxes are counted, not refused."""
    children, levels = structure(nodes, order)
    origin, exponents, _, _, _, _, q = decode(nodes)
    boxes64, slack = world_boxes64(transforms, local_boxes)
    boxes32 = world_boxes32(transforms, local_boxes)
    step = np.ldexp(1.0, (exponents - 127).astype(np.int64))           # (count, 3) float64, exact
    p = origin.astype(np.float64)
    found = Findings()
    floor = extent_floor(boxes32)
    for k, entry in enumerate(children):
        everything = np.concatenate([inst for _, _, inst in entry])
        want = expected_exponents(boxes32[everything, 0].min(axis=0), boxes32[everything, 1].max(axis=0), floor)
        assert np.array_equal(exponents[k], want), "node %d: exponents %r, the rule gives %r" % (k, exponents[k].tolist(), want.tolist())
        for s, _, inst in entry:
            q_lo, q_hi = q[k, :, 0, s].astype(np.int64), q[k, :, 1, s].astype(np.int64)
            lo, hi = p[k] + q_lo * step[k], p[k] + q_hi * step[k]
            below_lo, below_hi = boxes64[inst, 0], boxes64[inst, 1]
            # containment
            short = np.maximum(lo - below_lo, below_hi - hi)                       # (instances, 3): > 0 where the child box falls short
            with np.errstate(divide="ignore", invalid="ignore"):
                in_slacks = np.where(short > 0, short / slack[inst], 0.0)
            found.containment_in_slacks = max(found.containment_in_slacks, float(in_slacks.max()))
            assert (short <= slack[inst]).all(), "node %d slot %d: an instance sticks out of its child box by %.3g slacks" % (k, s, in_slacks.max())
            # thickness
            found.children += 1
            if (q_hi <= q_lo).any():
                found.flat += 1
                assert not require_thickness, "node %d slot %d: a child box of zero thickness, q_lo %r q_hi %r" % (k, s, q_lo.tolist(), q_hi.tolist())
            # tightness
            group_slack = slack[inst].max(axis=0)
            with np.errstate(over="ignore"):   # widened: one step thick, and the float64 box (give or take the slack) lies on one grid line
                line_lo = np.clip(np.floor((below_lo.min(axis=0) - p[k] + group_slack) / step[k]), 0, 255)
                line_hi = np.clip(np.ceil((below_hi.max(axis=0) - p[k] - group_slack) / step[k]), 0, 255)
            widened = (q_hi - q_lo == 1) & (line_hi <= line_lo)
            found.widened += int(widened.any())
            room_lo = step[k] * np.where(widened & (q_hi == 255), 2.0, 1.0) + group_slack
            room_hi = step[k] * np.where(widened & (q_hi < 255), 2.0, 1.0) + group_slack
            assert (below_lo.min(axis=0) - lo < room_lo).all() and (hi - below_hi.max(axis=0) < room_hi).all(), \
                "node %d slot %d: the child box is more than a grid step larger than what is below it" % (k, s)
    return found


# ---- rays -----------------------------------------------------------------------------------------------------------------

def world_triangles(transforms, mesh, mesh_triangles):
    """(total, 3, 3) float64 world-space triangles of all instances in scene order, and the instance of each."""
    out, owner = [], []
    t = np.asarray(transforms, np.float64).reshape(-1, 3, 4)
    for kind, triangles in enumerate(mesh_triangles):
        which = np.nonzero(np.asarray(mesh) == kind)[0]
        if which.size == 0:
            continue
        v = np.asarray(triangles, np.float64)                                                            # (K, 3, 3)
        world = np.einsum("nij,kvj->nkvi", t[which][:, :, :3], v) + t[which][:, None, None, :, 3]
        out.append(world.reshape(-1, 3, 3)); owner.append(np.repeat(which, v.shape[0]))
    return np.concatenate(out), np.concatenate(owner)


def miss(rays):
    """The brute force's answer for rays with nothing near them."""
    import trace_reference as ref
    fields = {f: np.zeros(rays) for f in ref.BruteForce.__dataclass_fields__}
    for f in ("t", "t_second", "t_ambiguous", "t_clear", "t_tiny"):
        fields[f] = np.full(rays, np.inf)
    fields["index"] = np.full(rays, -1, np.int64)
    return ref.BruteForce(**fields)


SCREEN = 0.005     # grazing measure below which a (ray, triangle) pair is kept whatever its box says


def brute_force(origin, direction, world, owner, boxes64, chunk=8):
    """trace_reference.brute_force, field for field, without most of its (ray, triangle) pairs. A pair can only matter -- be a hit,
    or an intersection float32 might accept either way -- where the ray meets the triangle's plane within the triangle's margins,
    and trace_reference's margins are MARGIN * 2^-24 * S / g long (S the largest coordinate involved, g the grazing measure
    |n . d|). So per chunk of rays only the triangles are kept (a) of instances whose float64 world box, grown by that length at
    g = SCREEN (rounded up to 1e-3 S), a ray of the chunk passes through, and (b) that some ray of the chunk grazes with g < SCREEN."""
    import trace_reference as ref
    o = np.asarray(origin, np.float64).T; d = np.asarray(direction, np.float64).T
    largest = 2.0 * max(np.abs(o).max(), np.abs(boxes64).max())                    # |t d| <= |o| + |p|
    assert 1.5 * ref.TOL.MARGIN * ref.EPS32 / SCREEN < 1e-3 and ref.TOL.GAP * ref.EPS32 / SCREEN < 1e-3 and SCREEN > ref.TOL.GRAZING
    lo, hi = boxes64[:, 0] - 1e-3 * largest, boxes64[:, 1] + 1e-3 * largest
    e1, e2 = world[:, 1] - world[:, 0], world[:, 2] - world[:, 0]
    normal = np.cross(e1, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        normal = normal / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))[:, None]      # |normal . d| / |d| is trace_reference's grazing measure
    unit = d / np.linalg.norm(d, axis=1, keepdims=True)
    parts = []
    for a in range(0, o.shape[0], chunk):
        oo, dd = o[a:a + chunk, None, :], d[a:a + chunk, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo[None] - oo) / dd, (hi[None] - oo) / dd
        near = np.fmax.reduce(np.fmin(t1, t2), axis=2); far = np.fmin.reduce(np.fmax(t1, t2), axis=2)
        inside = ((oo >= lo[None]) & (oo <= hi[None]) | (dd != 0)).all(axis=2)        # an axis the ray runs along: its origin must lie in the slab
        member = (inside & ~(near > far) & ~(far < 0)).any(axis=0)
        with np.errstate(invalid="ignore"):
            grazed = ~(np.abs(unit[a:a + chunk] @ normal.T) >= SCREEN).all(axis=0)      # (NaN normals of degenerate triangles: kept)
        chosen = np.nonzero(member[owner] | grazed)[0]
        bf = ref.brute_force(o[a:a + chunk].T, d[a:a + chunk].T, world[chosen]) if chosen.size else miss(len(oo))
        if chosen.size:
            bf.index = np.where(bf.index >= 0, chosen[np.maximum(bf.index, 0)], -1)
        parts.append(bf)
    fields = [f for f in ref.BruteForce.__dataclass_fields__]
    return ref.BruteForce(**{f: np.concatenate([getattr(p, f) for p in parts]) for f in fields})
