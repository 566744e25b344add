"""Inputs of the device BLAS build that the CPU test (tests/test_blas.py) and the GPU test (tests/test_gpu_blas_cases.py) share.
TEST INFRASTRUCTURE ONLY: numpy, seeded, nothing of the product.

A case is what rt_build_geometry takes: `records` (T, 24) float32 (position_0, edge_1, edge_2 and fifteen numbers that tell the
records apart), `mesh_first` (M + 1,) int32, and `given`: None or (first triangle, (n, 6) float32 piece boxes) for
rt_set_build_boxes. `traced` says what its rays are held to: "floor" -- at least 30 % of the rays hit and 30 % are robust, and
the float64 rules of tests/trace_checks.py hold; "real" -- only those rules (every hit a real float64 intersection, robust rays
exact), for geometry whose rays cannot reach the floor (said in `why`); None -- not traced (the brute force would not be cheap).

What the cases are for (each premise is asserted on the restatement's output by `assert_premise` before anything is launched):
  leaves        1, 2, 3 triangles: one leaf; 4, 5: the first cut; 24: eight full leaves; 25: the first inner child; 33;
  sizes         63 .. 2 049: waves, workgroups and the levels of the run-box table, which change between 2^k - 1 and 2^k;
  wide          20 000 triangles: levels wider than one workgroup of kernel_blas_runs (256) and of kernel_blas_nodes (32);
  meshes        300 meshes of 0 .. 9 triangles, empty ones first, last and adjacent, one triangle between two meshes of 500: waves
                of kernel_blas_triangle_boxes with three and more meshes and waves inside one mesh; 2, 3, 256, 257 and 1 025
                meshes of one triangle: mesh_bits and the radix digits;
  equal codes   4 097 copies of one triangle (the halving alone); 200 triangles around one centre (the area rule alone);
  degenerate    points and needles, a grid in one plane, sizes 1e-4 and 1e4, an offset of 1e5 (the padding loop doubles), and
                `far_grid_line`: a floor whose padded box lies on one grid line of a node 131 072 wide;
  given boxes   a floor triangle as 16 copies with a 4 x 4 grid of boxes, a box that misses its triangle, a range past the input.
"""
from collections import namedtuple

import numpy as np

F = np.float32
RAYS = 1500                    # per traced case, half aimed at triangle centres from outside, half at random
TRACED_UP_TO = 2400            # triangles: beyond, the float64 brute force is not cheap

Case = namedtuple("Case", "name records mesh_first given traced why down")


def records_of(vertices):
    """(T, 24) float32 records of (T, 3, 3) vertices: position_0, edge_1, edge_2, then numbers no two records share."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3, 3)
    r = np.zeros((len(v), 24), F)
    r[:, 0:3] = v[:, 0]; r[:, 3:6] = v[:, 1] - v[:, 0]; r[:, 6:9] = v[:, 2] - v[:, 0]
    r[:, 9:24] = (np.arange(len(v))[:, None] * 16 + np.arange(15)[None, :]) % 8191 + 0.5
    return r


def vertices_of(records):
    """(T, 3, 3) float64: the vertices the traversal's test sees, p0, p0 + e1, p0 + e2 of the float32 records."""
    r = np.asarray(records, np.float64).reshape(-1, 24)
    return np.stack([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9]], axis=1)


def make(name, vertices, mesh_first=None, given=None, traced="auto", why="", down=None):
    records = records_of(vertices)
    first = np.array([0, len(records)] if mesh_first is None else mesh_first, np.int32)
    if traced == "auto":
        traced = "floor" if len(records) <= TRACED_UP_TO else None
    return Case(name, records, first, given, traced, why, down)


def soup(seed, n, size=0.3, extent=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * size) * extent + offset


LEAF_SIZES = [1, 2, 3, 4, 5, 24, 25, 33]


def octants(n):
    """n >= 24 small triangles, three around each corner of a cube and the rest around the first: the cuts at the three highest
    Morton bits part the corners, so 24 triangles are eight full leaves and the 25th makes the first inner child."""
    rng = np.random.default_rng(n)
    corner = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)], np.float64) * 2 - 1
    which = np.concatenate([np.repeat(np.arange(8), 3), np.zeros(n - 24, np.int64)])
    return corner[which][:, None, :] + rng.normal(size=(n, 3, 3)) * 0.08


TABLE_SIZES = [63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
MESH_COUNTS = [2, 3, 256, 257, 1025]


def many_meshes():
    """300 meshes: counts 0 .. 9 at random, but empty meshes first and last, three adjacent empty ones in the middle, and one mesh
    of one triangle between two of 500."""
    rng = np.random.default_rng(300)
    counts = rng.integers(0, 10, 300)
    counts[0] = counts[1] = 0; counts[-1] = 0; counts[100:103] = 0
    counts[200], counts[201], counts[202] = 500, 1, 500
    first = np.concatenate([[0], np.cumsum(counts)])
    centres = rng.uniform(-8, 8, (300, 3))
    vertices = np.concatenate([centres[m] + rng.uniform(-1, 1, (c, 1, 3)) * 0.6 + rng.normal(size=(c, 3, 3)) * 0.25 for m, c in enumerate(counts)])
    return make("meshes_300", vertices, first)


def one_triangle_meshes(count):
    rng = np.random.default_rng(count)
    vertices = rng.uniform(-6, 6, (count, 1, 3)) + rng.normal(size=(count, 3, 3)) * 0.5
    return make("meshes_of_one_%d" % count, vertices, np.arange(count + 1))


def copies():
    one = soup(4097, 1, 0.5)
    return make("copies_4097", np.repeat(one, 4097, axis=0), traced="real", why="every hit is tied between 4 097 triangles: no hit is robust")


def concentric():
    """200 triangles of sizes 0.01 .. 2 in random planes, each moved so that the centre of its box is (0.5, -0.25, 1): equal
    Morton cells, different boxes."""
    rng = np.random.default_rng(200)
    v = rng.normal(size=(200, 3, 3)) * np.geomspace(0.01, 2.0, 200)[:, None, None]
    v += (np.array([0.5, -0.25, 1.0]) - 0.5 * (v.min(axis=1) + v.max(axis=1)))[:, None, :]
    return make("concentric_200", v)


def points_and_needles():
    rng = np.random.default_rng(90)
    at = rng.uniform(-2, 2, (60, 1, 3))
    points = np.repeat(at[:30], 3, axis=1)
    along = rng.normal(size=(30, 1, 3))
    needles = at[30:] + along * np.array([0.0, 0.5, 1.0])[None, :, None]           # three collinear vertices
    return make("points_and_needles_60", np.concatenate([points, needles]), traced="real", why="no triangle has an area: nothing can be hit")


def plane_grid():
    """A 12 x 12 grid of squares in the plane y = 0.75, two triangles each: every box of the tree is flat in y."""
    g = np.arange(12.0) / 6 - 1
    x, z = [a.ravel() for a in np.meshgrid(g, g)]
    s = 1 / 6
    v = np.zeros((288, 3, 3)); v[:, :, 1] = 0.75
    v[0::2, :, 0] = np.stack([x, x + s, x + s], 1); v[0::2, :, 2] = np.stack([z, z, z + s], 1)
    v[1::2, :, 0] = np.stack([x, x + s, x], 1); v[1::2, :, 2] = np.stack([z, z + s, z + s], 1)
    return make("plane_grid_288", v)


def far_grid_line():
    """Two floor triangles at y = 0 spanning +-65 536 in x and z, two wall triangles in the plane x = -65 536 spanning +-65 536 in y
    and z. The walls' Morton codes have the top bit clear, the floors' have it set: the root has a child of the two floor triangles,
    whose padded box [-0.001, 0.001] vanishes in float32 beside the root's origin -65 536 -- both bounds fall on grid line 64 of a
    grid of 1 024-unit steps. `down`: one ray per floor triangle from y = 1 straight down, well inside it."""
    s = 65536.0
    floor = [[[-s, 0, -s], [s, 0, -s], [s, 0, s]], [[-s, 0, -s], [s, 0, s], [-s, 0, s]]]
    wall = [[[-s, -s, -s], [-s, s, -s], [-s, s, s]], [[-s, -s, -s], [-s, s, s], [-s, -s, s]]]
    down = (np.array([0, 1]), np.array([[30000.0, 1.0, -30000.0], [-30000.0, 1.0, 30000.0]]))
    return make("far_grid_line", np.array(wall + floor, np.float64), down=down)


def floor_pieces():
    """A floor triangle 8 units wide given as 16 copies with the 4 x 4 grid of boxes over its square (the cells beyond the diagonal
    miss it), under 24 small triangles."""
    floor = np.array([[[-4.0, 0, -4], [4, 0, -4], [4, 0, 4]]])
    above = soup(16, 24, 0.25, extent=3.0) + np.array([0, 3.5, 0])
    cells = np.array([[-4 + 2 * i, -1, -4 + 2 * j, -2 + 2 * i, 1, -2 + 2 * j] for i in range(4) for j in range(4)], F)
    return make("floor_pieces_16", np.concatenate([above[:10], np.repeat(floor, 16, axis=0), above[10:]]), given=(10, cells))


def piece_misses():
    """Seven records of six triangles: records 2 and 3 are copies of one triangle, the first with a box around all of it, the second
    with a box beside it, which the intersection collapses to a point. (A triangle is found through its pieces' boxes: the copies of
    one triangle have to cover it between them, as these two do.)"""
    v = soup(6, 6, 0.5)
    v = np.concatenate([v[:3], v[2:]])
    lo, hi = v.min(axis=1), v.max(axis=1)
    boxes = np.array([np.concatenate([lo[2] - 0.5, hi[2] + 0.5]), np.concatenate([hi[3] + 1.0, hi[3] + 2.0])], F)
    return make("piece_misses_7", v, given=(2, boxes))


def given_past_input():
    v = soup(40, 40, 0.3)
    boxes = np.tile(np.array([[-0.1, -0.1, -0.1, 0.1, 0.1, 0.1]], F), (8, 1))
    return make("given_past_input_40", v, given=(33, boxes))      # 33 + 8 > 40: ignored as a whole


def all_cases():
    cases = [make("leaf_%d" % n, octants(n) if n in (24, 25) else soup(n, n, 0.4)) for n in LEAF_SIZES]
    cases += [make("soup_%d" % n, soup(n, n, 0.12)) for n in TABLE_SIZES]
    cases += [make("soup_20000", soup(20000, 20000, 0.03))]
    cases += [many_meshes()] + [one_triangle_meshes(m) for m in MESH_COUNTS]
    cases += [copies(), concentric(), points_and_needles(), plane_grid(),
              make("tiny_1e-4_300", soup(301, 300, 0.2, extent=1e-4)),
              make("huge_1e4_300", soup(302, 300, 0.2, extent=1e4)),
              make("offset_1e5_300", soup(303, 300, 0.2, offset=1e5), traced="real", why="a unit mesh at 1e5: float32 resolves 0.008 there, rays and vertices alike"),
              far_grid_line(), floor_pieces(), piece_misses(), given_past_input()]
    return cases


_cache = {}


def cases():
    if "all" not in _cache:
        _cache["all"] = all_cases()
    return _cache["all"]


def names():
    return [c.name for c in cases()]


def by_name(name):
    return next(c for c in cases() if c.name == name)


def assert_premise(case, built, rebuild):
    """What a case is for is true of it. built: blas_reference.build of the case; rebuild(case, **changes): the same with changes."""
    import blas_reference
    T, M = len(case.records), len(case.mesh_first) - 1
    widths = built.level_widths
    if case.name == "leaf_24":
        assert widths == [1] and (np.asarray(built.nodes)[-1, 24:32] >> 5 == 7).all()
    if case.name == "leaf_25":
        root = np.asarray(built.nodes)[-2]
        assert widths == [1, 1] and bin(int(root[15])).count("1") == 1 and (root[24:32] != 0).all()
    if case.name.startswith("soup_") and T in TABLE_SIZES and (T & (T - 1)) == 0:
        assert blas_reference.table_levels(T - 1) + 1 == blas_reference.table_levels(T) == blas_reference.table_levels(T + 1)
    if case.name == "soup_20000":
        assert max(widths) > 256 and any(w % 32 for w in widths), widths
    if case.name == "meshes_300":
        counts = np.diff(case.mesh_first)
        assert counts[0] == 0 and counts[-1] == 0 and (counts[100:103] == 0).all() and list(counts[200:203]) == [500, 1, 500]
        per_wave = [len(set(built.mesh_of[w:w + 64].tolist())) for w in range(0, T, 64)]
        assert max(per_wave) >= 3 and any(n == 1 and w * 64 + 64 <= T for w, n in enumerate(per_wave)), per_wave
    if case.name.startswith("meshes_of_one_"):
        bits = 1
        while (1 << bits) < M:
            bits += 1
        assert (M in (3, 257, 1025)) == (M > 2 and (1 << (bits - 1)) + 1 == M)           # the counts just past a power of two need one bit more
        assert not np.array_equal(rebuild(case, mesh_bits=bits - 1).position, built.position)   # ... and one bit fewer is another build
    if case.name in ("copies_4097", "concentric_200"):
        assert len(set(built.codes.tolist())) == 1
        lo, hi = blas_reference.padded_boxes(case.records)
        assert (len(np.unique(np.concatenate([lo, hi], axis=1), axis=0)) == 1) == (case.name == "copies_4097")
    if case.name == "offset_1e5_300":
        lo, hi = blas_reference.padded_boxes(case.records)
        assert (hi - lo >= F(0.001)).all() and np.abs(lo).min() > 9e4
    if case.name == "plane_grid_288":
        lo, hi = blas_reference.padded_boxes(case.records)
        assert (vertices_of(case.records)[:, :, 1] == 0.75).all() and (lo[:, 1] < F(0.75)).all() and (hi[:, 1] > F(0.75)).all() and (hi[:, 1] - lo[:, 1] < F(0.01)).all()
    if case.name == "far_grid_line":
        before = rebuild(case, keep_thickness=False)
        assert before.flat_children >= 1 and built.flat_children == before.flat_children     # the floor's child has q_lo == q_hi until it is widened
        root = np.asarray(before.nodes)[-1]
        flat_slots = np.nonzero((root[48:56] == root[56:64]) & (root[24:32] != 0))[0]
        assert len(flat_slots) == 1 and root[48 + flat_slots[0]] == 64, root[48:64]
        which, origin = case.down
        v = vertices_of(case.records)[2 + which]                                             # inside, in float64
        e1, e2, s = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], origin - v[:, 0]
        det = e1[:, 0] * e2[:, 2] - e1[:, 2] * e2[:, 0]
        a, b = (s[:, 0] * e2[:, 2] - s[:, 2] * e2[:, 0]) / det, (e1[:, 0] * s[:, 2] - e1[:, 2] * s[:, 0]) / det
        assert (np.minimum(np.minimum(a, b), 1 - a - b) > 0.05).all() and (origin[:, 1] == 1).all()
    if case.given is not None:
        first, boxes = case.given                                   # between them the pieces of a triangle cover it: its rays can find it
        if first + len(boxes) <= T:
            v = vertices_of(case.records)
            for i in range(T):
                same = [j for j in range(T) if np.array_equal(v[i], v[j])]
                inside = [boxes[j - first] for j in same if first <= j < first + len(boxes)]
                assert len(inside) == len(same) or len(inside) == 0
                for corner in v[i] if inside else []:
                    assert any((b[:3] <= corner).all() and (corner <= b[3:]).all() for b in inside), (case.name, i)
        without = rebuild(case, given=None)
        assert np.array_equal(without.nodes, built.nodes) == (case.name == "given_past_input_40")
    if case.name == "piece_misses_7":
        pieces, has = blas_reference.pieces_of(T, case.given)
        lo, hi = blas_reference.padded_boxes(case.records, pieces, has)
        assert has.sum() == 2 and (hi[3] - lo[3] < F(0.01)).all()                       # the piece beside the triangle collapsed to a padded point


def rays_of(case):
    """(3, N) float32 origins and directions: half from outside the scene box at points well inside triangles (barycentric
    coordinates of at least 0.15; triangles drawn with replacement, so that a mesh of one triangle gets its share too), half from
    random places in random directions; `down` rays first."""
    v = vertices_of(case.records)
    rng = np.random.default_rng(7919 * len(v) + 13)
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    diagonal = max(float(np.linalg.norm(hi - lo)), 1e-3 * float(np.abs(v).max()))
    aimed = rng.integers(0, len(v), RAYS // 2)
    away = rng.normal(size=(len(aimed), 3)); away /= np.linalg.norm(away, axis=1, keepdims=True)
    weights = 0.15 + 0.55 * rng.dirichlet(np.ones(3), len(aimed))
    target = (v[aimed] * weights[:, :, None]).sum(axis=1)
    loose = RAYS - len(aimed)
    anywhere = 0.5 * (lo + hi) + rng.uniform(-0.75, 0.75, (loose, 3)) * diagonal
    heading = rng.normal(size=(loose, 3)); heading /= np.linalg.norm(heading, axis=1, keepdims=True)
    origin = np.concatenate([target + 1.5 * diagonal * away, anywhere]); direction = np.concatenate([-away, heading]) + 0.0
    if case.down is not None:
        origin = np.concatenate([case.down[1], origin]); direction = np.concatenate([np.tile([0.0, -1.0, 0.0], (len(case.down[1]), 1)), direction])
    return np.ascontiguousarray(origin.T, F), np.ascontiguousarray(direction.T, F)


_brute = {}


def brute_force(case):
    """The float64 brute force over a traced case's rays, computed once and left unchanged: (origin, direction, BruteForce)."""
    import tlas_reference
    if case.name not in _brute:
        origin, direction = rays_of(case)
        v = vertices_of(case.records)
        boxes = np.stack([v.min(axis=1), v.max(axis=1)], axis=1)
        _brute[case.name] = (origin, direction, tlas_reference.brute_force(origin, direction, v, np.arange(len(v)), boxes))
    return _brute[case.name]
