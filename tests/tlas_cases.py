"""Inputs of the device TLAS build that the CPU test (tests/test_tlas.py) and the GPU test (tests/test_gpu_tlas.py) share.
TEST INFRASTRUCTURE ONLY: numpy, seeded, nothing of the product.

A case is what rt_build_tlas takes, in scene order: `transforms` and `transforms_inv` (n, 3, 4) float32, `local_boxes`
(n, 6) float32 (object-space min xyz, max xyz) and `mesh` (n,), the mesh each instance shows. There are two meshes: a unit
cube (12 triangles) and a unit square in the xz-plane (2 triangles, zero height). Every case is shuffled into a random scene
order, so that scene index and Morton order have nothing to do with each other.

What the cases are for:
  sizes         the launch-shape boundaries: 1 024 / 1 025 (256 against 1 024 threads, sorted boxes in LDS against global
                memory), the powers of two and their neighbours (bitonic padding), 4 096 (the most one launch takes);
  wide levels   levels of more nodes than the workgroup has threads, so that the numbering scan of step 3b runs a second chunk
                and carries its totals over: `wide` names the thread count the widest level has to exceed, and the tests
                assert that it does before anything is launched;
  degenerate    coincident instances, point boxes, a line, a plane, scales over ten decades, magnitudes up to the exponent
                clamps of the node format;
  flat          child boxes whose lower and upper bound meet on one grid line of their node: `aim` lists, for instances with
                such a box, a point of the instance and the unit normal there -- a ray down the normal has to hit it;
  signed zeros  box bounds of both -0.0 and +0.0.
"""
from collections import namedtuple

import numpy as np

CUBE, SQUARE = 0, 1
MESH_BOXES = np.array([[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], [-0.5, 0.0, -0.5, 0.5, 0.0, 0.5]], np.float32)
TRACED_UP_TO = 1100            # cases of at most this many instances are also traced (and those that say so themselves)

Case = namedtuple("Case", "name transforms transforms_inv local_boxes mesh wide aim traced magnitude")


def mesh_triangles(mesh):
    """(K, 3, 3) float32 vertices of a mesh's triangles."""
    if mesh == SQUARE:   # split along the diagonal x == z
        v = np.array([[-0.5, 0, -0.5], [0.5, 0, -0.5], [0.5, 0, 0.5], [-0.5, 0, 0.5]], np.float32)
        return v[np.array([[0, 1, 2], [0, 2, 3]])]
    v = np.array([[(c & 1) - 0.5, ((c >> 1) & 1) - 0.5, ((c >> 2) & 1) - 0.5] for c in range(8)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v[np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])]


def rotations(rng, n):
    """(n, 3, 3) float64 rotation matrices of uniformly random unit quaternions."""
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def compose(position, rotation, scale):
    """Object -> world matrices T R S and their inverses, (n, 3, 4) float32 each; the inverse is formed in float64."""
    position = np.asarray(position, np.float64); n = position.shape[0]
    rotation = np.broadcast_to(np.eye(3), (n, 3, 3)) if rotation is None else np.asarray(rotation, np.float64)
    scale = np.broadcast_to(np.asarray(scale, np.float64), (n,))
    m = np.concatenate([rotation * scale[:, None, None], position[:, :, None]], axis=2)
    inv_r = np.swapaxes(rotation, 1, 2) / scale[:, None, None]
    inv = np.concatenate([inv_r, -np.einsum("nij,nj->ni", inv_r, position)[:, :, None]], axis=2)
    return m.astype(np.float32), inv.astype(np.float32)


def make(name, rng, transforms, transforms_inv, mesh, local_boxes=None, wide=None, aim=None, traced=None, magnitude=1.0):
    """Shuffles a case into a random scene order. aim: (instances, object-space points (k, 3)) -> world points and normals."""
    n = transforms.shape[0]
    mesh = np.broadcast_to(np.asarray(mesh, np.int32), (n,)).copy()
    boxes = MESH_BOXES[mesh].copy() if local_boxes is None else np.asarray(local_boxes, np.float32).reshape(n, 6).copy()
    shuffle = rng.permutation(n)
    transforms, transforms_inv, boxes, mesh = transforms[shuffle], transforms_inv[shuffle], boxes[shuffle], mesh[shuffle]
    aimed = None
    if aim is not None:
        where = np.empty(n, np.int64); where[shuffle] = np.arange(n)
        instances = where[np.asarray(aim[0], np.int64)]
        m = transforms[instances].astype(np.float64)
        point = np.einsum("nij,nj->ni", m[:, :, :3], np.asarray(aim[1], np.float64)) + m[:, :, 3]
        normal = m[:, :, 1] / np.linalg.norm(m[:, :, 1], axis=1, keepdims=True)     # the square's normal is its object-space y axis
        aimed = (instances, point, normal)
    return Case(name, np.ascontiguousarray(transforms), np.ascontiguousarray(transforms_inv), np.ascontiguousarray(boxes), mesh, wide, aimed,
                n <= TRACED_UP_TO if traced is None else traced, float(magnitude))


def uniform(name, seed, n, extent=20.0, magnitude=1.0, **more):
    """n instances of both meshes at uniformly random places, randomly rotated, scaled by 0.3 .. 1.5 (times `magnitude`)."""
    rng = np.random.default_rng(seed)
    m, inv = compose(rng.uniform(-extent, extent, (n, 3)) * magnitude, rotations(rng, n), rng.uniform(0.3, 1.5, n) * magnitude)
    return make(name, rng, m, inv, rng.integers(0, 2, n), magnitude=magnitude, **more)


SIZES = [1, 2, 8, 9, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]


def comb():
    """A level of 1 792 nodes under 1 024 threads. The builder cuts the widest run first, so its trees are near-complete 8-ary
    ones and uniform placement never gets a level past ~500 nodes at 4 096 instances. Unit cubes on the integer points of a
    16^3 grid: the scene box is exactly 16 wide and a point's Morton cell is 64 g + 32, so four octant digits (o1, o2, o3, o4)
    (x is bit 2 of a digit, the highest digit first) name a point and the tree's first four levels. For o1 in 0..6 and o2 in
    0..7: an even o2 holds ONE instance, at (o1, o2, 0, 0); an odd o2 holds TWO coincident instances at every (o1, o2, o3, o4).
    One more instance sits at (7, 7, 7, 7). 3 613 instances; level widths 1, 7, 28, 224, 1 792."""
    def point(digits):
        g = np.zeros(3, np.int64)
        for o in digits:
            g = 2 * g + np.array([(o >> 2) & 1, (o >> 1) & 1, o & 1])
        return g
    points = []
    for o1 in range(7):
        for o2 in range(8):
            if o2 % 2 == 0:
                points.append(point((o1, o2, 0, 0)))
            else:
                points += [point((o1, o2, o3, o4)) for o3 in range(8) for o4 in range(8) for _ in range(2)]
    points.append(point((7, 7, 7, 7)))
    rng = np.random.default_rng(3613)
    m, inv = compose(np.array(points, np.float64), None, 1.0)
    return make("comb_3613", rng, m, inv, CUBE, wide=1024, traced=True)


def coincident(name, seed, n, **more):
    rng = np.random.default_rng(seed)
    m, inv = compose(np.tile([[1.5, -2.0, 0.75]], (n, 1)), np.tile(rotations(rng, 1), (n, 1, 1)), 1.25)
    return make(name, rng, m, inv, CUBE, **more)


def points_at_one_point():
    """300 instances whose world boxes are one point: squares scaled by 2^-100 at (3, 4, 5). The products vanish beside the
    translation in float32, the inverse (2^100) is finite."""
    rng = np.random.default_rng(300)
    m, inv = compose(np.tile([[3.0, 4.0, 5.0]], (300, 1)), rotations(rng, 300), 2.0 ** -100)
    return make("points_300", rng, m, inv, SQUARE)


def line():
    rng = np.random.default_rng(1025)
    position = np.zeros((1025, 3)); position[:, 0] = rng.uniform(-300, 300, 1025)
    m, inv = compose(position, rotations(rng, 1025), rng.uniform(0.3, 1.5, 1025))
    return make("line_1025", rng, m, inv, rng.integers(0, 2, 1025))


def plane():
    """2 049 squares lying in the plane y = 0: every box of the tree is flat in y."""
    rng = np.random.default_rng(2049)
    position = rng.uniform(-60, 60, (2049, 3)); position[:, 1] = 0.0
    m, inv = compose(position, None, rng.uniform(0.3, 1.5, 2049))
    return make("plane_2049", rng, m, inv, SQUARE)


def scales():
    rng = np.random.default_rng(900)
    m, inv = compose(rng.uniform(-100, 100, (900, 3)), rotations(rng, 900), 10.0 ** rng.uniform(-6, 4, 900))
    return make("scales_900", rng, m, inv, rng.integers(0, 2, 900))


AIM_POINT = [0.25, 0.0, -0.125]     # inside the square's first triangle, an eighth of its side away from the diagonal and the edges


def flat_tiles():
    """200 unit tiles with exactly flat boxes on integer heights: lower and upper bound of a tile are the same number, and on
    a node grid of a power-of-two step that starts at an integer they land on one grid line."""
    rng = np.random.default_rng(200)
    n = 200
    position = np.stack([rng.integers(0, 160, n) * 0.25, rng.integers(0, 20, n).astype(np.float64), rng.integers(0, 160, n) * 0.25], 1)
    m, inv = compose(position, None, 1.0)
    return make("flat_tiles_200", rng, m, inv, SQUARE, aim=(np.arange(n), np.tile(AIM_POINT, (n, 1))))


def flat_small_instances():
    """The shape a scene file gives: object-space boxes padded by 0.001 (what a flat triangle's box is widened to before it reaches
    the builder), instances scaled by 1e-3, on distinct multiples of 128 in a scene about 2 000 units wide. A box is 2e-6 thick
    at a coordinate whose float32 spacing is up to 1.2e-4: flat or one ulp thick, far below a grid step."""
    rng = np.random.default_rng(266)
    n = 200
    cells = rng.choice(16 ** 3, n, replace=False)
    position = np.stack([cells // 256, (cells // 16) % 16, cells % 16], 1) * 128.0
    m, inv = compose(position, None, 1e-3)
    boxes = np.tile(MESH_BOXES[SQUARE], (n, 1)); boxes[:, 1] -= 0.001; boxes[:, 4] += 0.001
    return make("flat_small_200", rng, m, inv, SQUARE, local_boxes=boxes, aim=(np.arange(n), np.tile(AIM_POINT, (n, 1))))


def flat_in_the_bounding_planes():
    """One tile in the minimum plane and one in the maximum plane of the root, whose height is 255 grid steps of 1 / 16: the
    lower tile quantises to 0 = 0 and is widened upwards, the upper one to 255 = 255 and is widened downwards. Six cubes
    strictly between them keep the node's other axes ordinary."""
    rng = np.random.default_rng(255)
    height = 255.0 / 16.0
    position = np.array([[2.0, 0.0, 3.0], [9.0, height, 7.0]] + [[rng.uniform(0, 12), rng.uniform(2, 12), rng.uniform(0, 12)] for _ in range(6)])
    m, inv = compose(position, None, 1.0)
    return make("flat_planes_8", rng, m, inv, [SQUARE, SQUARE] + [CUBE] * 6, aim=(np.arange(2), np.tile(AIM_POINT, (2, 1))))


def signed_zeros():
    """64 squares in the plane y = 0 whose boxes reach 0.25 above them (a box may be larger than its mesh). The lower bound in y
    is a sum of zeros, ((a * x + 1 * y) + b * z) + t with a = b = t = y = +-0: the builder keeps the last of equal corners, the one
    at (max x, min y, max z), and there every term is -0.0 for the instances written with negative zeros -- their bound is -0.0,
    that of the others +0.0."""
    rng = np.random.default_rng(64)
    n = 64
    position = np.stack([rng.integers(-40, 40, n) * 0.5, np.zeros(n), rng.integers(-40, 40, n) * 0.5], 1)
    m, inv = compose(position, None, 1.0)
    boxes = np.tile(MESH_BOXES[SQUARE], (n, 1)); boxes[:, 4] = 0.25
    negative = np.arange(n) % 2 == 1
    for a in (m, inv):
        a[negative, 1, 0] = -0.0; a[negative, 1, 2] = -0.0; a[negative, 1, 3] = -0.0
    boxes[negative, 1] = -0.0
    return make("signed_zeros_64", rng, m, inv, SQUARE, local_boxes=boxes)


def all_cases():
    cases = [uniform("uniform_%d" % n, 1000 + n, n) for n in SIZES]
    cases += [coincident("coincident_1024", 1024, 1024, wide=256),
              uniform("ragged_1000", 1000, 1000, extent=14.0, wide=256),
              comb(),
              coincident("coincident_4096", 4096, 4096),
              points_at_one_point(), line(), plane(), scales()]
    cases += [uniform("magnitude_%g" % mag, 500 + k, 500, magnitude=mag) for k, mag in enumerate((1e-30, 1e-20, 1e-10, 1e10, 1e18, 1e30))]
    cases += [flat_tiles(), flat_small_instances(), flat_in_the_bounding_planes(), signed_zeros()]
    return cases


_cache = {}


def cases():
    """The cases, built once per process."""
    if "all" not in _cache:
        _cache["all"] = all_cases()
    return _cache["all"]


def names():
    return [c.name for c in cases()]


def by_name(name):
    return next(c for c in cases() if c.name == name)
