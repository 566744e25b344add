"""Small adversarial scenes for the traversal tests, and their rays. TEST INFRASTRUCTURE ONLY.

Each case writes its scene (OBJ + Mitsuba XML) under a directory the test gives it and returns the world-space triangles in
float64 (what tests/trace_reference.py casts against) and closest-hit rays in float32. Vertices are float32 values, so the
loader reads exactly what the float64 side holds; instances are placed by translate / rotate / uniform scale (the loader keeps an
instance as position, rotation and one scale factor, as the reference does, so a non-uniform scale cannot be an instance's).
Shadow rays are derived from the closest-hit rays by the tests (`shadow_limits`).
"""
import os
from dataclasses import dataclass, field

import numpy as np

SENSOR = ('<sensor type="perspective"><float name="fov" value="60"/><transform name="toWorld">'
          '<lookat origin="%s" target="%s" up="0, 1, 0"/></transform></sensor>')


@dataclass
class Case:
    name: str
    scene: str                      # the XML file
    world: np.ndarray               # (K, 3, 3) float64 world-space vertices of every triangle
    origin: np.ndarray              # (3, N) float32
    direction: np.ndarray           # (3, N) float32
    config: dict = field(default_factory=dict)   # config_set() values the case needs (merge_static = 0: instanced)
    closed: bool = False            # every ray starts inside or aims at a closed mesh: a miss is a leak


def f32(a):
    return np.asarray(np.asarray(a, np.float64).astype(np.float32), np.float64)


def write_obj(path, vertices, faces):
    with open(path, "w") as f:
        for v in np.asarray(vertices, np.float32):
            f.write("v %r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in faces:
            f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))


def write_scene(directory, name, shapes, eye="0, 0, 10", target="0, 0, 0"):
    path = os.path.join(directory, name + ".xml")
    with open(path, "w") as f:
        f.write('<scene version="0.5.0">%s%s</scene>' % (SENSOR % (eye, target), "".join(shapes)))
    return path


def obj_shape(filename, transform=""):
    return '<shape type="obj"><string name="filename" value="%s"/>%s<bsdf type="diffuse"/></shape>' % (
        filename, '<transform name="toWorld">%s</transform>' % transform if transform else "")


def one_mesh(directory, name, vertices, faces, **kw):
    """The faces as two meshes with the identity transform (two, so that the default config flattens them into one tree)."""
    half = (len(faces) + 1) // 2
    for k, part in enumerate((faces[:half], faces[half:])):
        write_obj(os.path.join(directory, "%s_%d.obj" % (name, k)), vertices, part)
    v = f32(vertices)
    return write_scene(directory, name, [obj_shape("%s_%d.obj" % (name, k)) for k in range(2)], **kw), v[np.asarray(faces)]


def normalised(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=0, keepdims=True)).astype(np.float32)


def aim(origins, targets):
    """(3, N) rays from origins to targets (float32 directions, not renormalised in float32)."""
    return np.asarray(origins, np.float32), normalised(np.asarray(targets, np.float64) - np.asarray(origins, np.float64))


def box(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[lo[0] if i & 1 == 0 else hi[0], lo[1] if i & 2 == 0 else hi[1], lo[2] if i & 4 == 0 else hi[2]] for i in range(8)])
    f = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)]
    return v, f


def merge(parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(np.asarray(v, np.float64)); fs += [(a + base, b + base, c + base) for a, b, c in f]; base += len(v)
    return np.concatenate(vs), fs


def icosphere(level):
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]; v.append(m / np.linalg.norm(m)); cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), f


def blob(n):
    """A closed lumpy sphere (the GPU parity tests' blob) as triangles."""
    v, f = [], []
    for i in range(n + 1):
        th = np.pi * i / n
        for j in range(2 * n):
            ph = np.pi * j / n
            r = 1.0 + 0.15 * np.sin(3 * th) * np.cos(2 * ph)
            v.append((r * np.sin(th) * np.cos(ph), r * np.cos(th), r * np.sin(th) * np.sin(ph)))
    for i in range(n):
        for j in range(2 * n):
            a = i * 2 * n + j; b = i * 2 * n + (j + 1) % (2 * n); c = (i + 1) * 2 * n + (j + 1) % (2 * n); e = (i + 1) * 2 * n + j
            f += [(a, b, c), (a, c, e)]
    return np.array(v), f


def random_rays(rng, n, centre, radius, target_radius):
    o = centre[:, None] + rng.normal(size=(3, n)) * radius
    t = centre[:, None] + rng.normal(size=(3, n)) * target_radius
    return aim(o, t)


# ---- the cases ----------------------------------------------------------------------------------------------------

def case_boxes(directory):
    """Axis-aligned boxes with integer corners; rays with components of exactly +0 and -0, origins on box planes."""
    v, f = merge([box((0, 0, 0), (1, 1, 1)), box((2, 0, 0), (3, 1, 1)), box((0.5, 2, -1), (1.5, 3, 0)), box((-2, -2, -2), (-1, 4, -1.5))])
    scene, world = one_mesh(directory, "boxes", v, f)
    dirs = np.array([(1, 0, 0), (-1, -0.0, 0), (0, -0.0, 1), (-0.0, 1, -0.0), (0, -1, -0.0), (0.0, 0.0, -1), (1, 1, 0), (-1, -0.0, 1),
                     (0, 1, -1), (1, 1, 1), (-1, 0.5, -0.0)], np.float64).T
    dirs = np.where(dirs == 0, dirs, dirs / np.linalg.norm(dirs, axis=0, keepdims=True)).astype(np.float32)   # (signed zeros kept)
    g = np.arange(-1.0, 4.01, 0.5)
    o = np.stack(np.meshgrid(g, g, g - 1.5, indexing="ij")).reshape(3, -1).astype(np.float32)
    O = np.repeat(o, dirs.shape[1], axis=1); D = np.tile(dirs, (1, o.shape[1]))
    return Case("boxes", scene, world, O, D)


def case_slivers(directory):
    """Needle triangles, zero-area triangles (exact float32 zero determinant: must never be hit) and a wall behind them."""
    needles = [((0, 0, z), (10, 0, z), (10, 1e-3 * (1 + z), z)) for z in range(4)]
    needles += [((-5, -5, 5), (5, 5, 5 + 1e-4), (5, 5.0001, 5))]
    zero = [((0, 0, 2), (1, 1, 3), (2, 2, 4)), ((1, 1, 1), (1, 1, 1), (2, 3, 1)), ((-3, 0, 1), (3, 0, 1), (0, 0, 1))]
    wall = [((-20, -20, 8), (20, -20, 8), (20, 20, 8)), ((-20, -20, 8), (20, 20, 8), (-20, 20, 8))]
    tris = np.array(needles + zero + wall, np.float64)
    scene, world = one_mesh(directory, "slivers", tris.reshape(-1, 3), [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(len(tris))])
    rng = np.random.default_rng(11)
    n = 3000
    o = np.stack([rng.uniform(-2, 12, n), rng.uniform(-1, 3, n), np.full(n, -3.0)])
    targets = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2], tris.mean(1)])   # vertices and centroids, jittered
    t = targets[rng.integers(0, len(targets), n)].T + rng.normal(size=(3, n)) * np.array([[1e-3], [1e-3], [0]])
    O, D = aim(o, t)
    return Case("slivers", scene, world, O, D)


def case_layers(directory):
    """Parallel quads 10 * 2^-9 apart at t ~ 10 (below 2^-7 of t: the 16-bit skip bound cannot tell them apart), with coplanar
    duplicates: the same quad twice, and the same plane under the other diagonal."""
    parts = []
    for k in range(8):
        z = 10.0 + k * 10.0 * 2.0 ** -9
        v = [(-4, -4, z), (4, -4, z), (4, 4, z), (-4, 4, z)]
        parts.append((v, [(0, 1, 2), (0, 2, 3)] if k % 2 == 0 else [(0, 1, 3), (1, 2, 3)]))
        if k in (2, 5):
            parts.append((v, [(0, 1, 2), (0, 2, 3)]))          # exact duplicate
            parts.append((v, [(0, 1, 3), (1, 2, 3)]))          # same plane, other diagonal
    v, f = merge(parts)
    scene, world = one_mesh(directory, "layers", v, f)
    rng = np.random.default_rng(12)
    n = 4000
    o = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), np.zeros(n)])
    t = np.stack([rng.uniform(-3.5, 3.5, n), rng.uniform(-3.5, 3.5, n), np.full(n, 10.0)])
    O, D = aim(o, t)
    return Case("layers", scene, world, O, D)


SHRINK = 0.75   # radius of a shell over the one outside it (0.75^120 ~ 1e-15: every determinant stays a normal float32)


def case_deep(directory, shells=120, per_shell=16, seed=13, name="deep", config=None):
    """Shells of small triangles around the ray origins, each SHRINK times the radius of the one outside it: the tree
    nests the shells level after level, and a ray from the centre crosses a box at every level with siblings left on its stack.
    The oracle's max_stack is 16 for the flattened tree (beyond the 10 entries the device keeps in LDS: its spill to HBM runs, and
    well within its 32) and 10 under the TLAS (merge_static = 0)."""
    rng = np.random.default_rng(seed)
    tris = []
    for k in range(shells):
        r = SHRINK ** k
        c = rng.normal(size=(per_shell, 3)); c /= np.linalg.norm(c, axis=1, keepdims=True)
        c *= r * rng.uniform(1.0, 1.5, (per_shell, 1))
        tris.append(c[:, None, :] + rng.normal(size=(per_shell, 3, 3)) * 0.3 * r)
    tris = np.concatenate(tris)
    count = len(tris)
    scene, world = one_mesh(directory, name, tris.reshape(-1, 3), [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(count)])
    n = 3000
    o = rng.normal(size=(3, n)) * (SHRINK ** rng.integers(0, shells, n))[None, :] * 0.1
    o[:, :500] = 0.0
    d = normalised(rng.normal(size=(3, n)))
    return Case(name, scene, world, o.astype(np.float32), d, config=config or {})


def case_scaled(directory, name, scale, offset):
    """The blob mesh at `scale`, moved by `offset`: the CWBVH's exponent bytes and the origin's precision at extremes."""
    v, f = blob(12)
    v = f32(v * scale + offset)
    scene, world = one_mesh(directory, name, v, f, eye="%r, %r, %r" % (offset, offset, offset + 5 * scale), target="%r, %r, %r" % (offset, offset, offset))
    rng = np.random.default_rng(14)
    n = 3000
    centre = np.full(3, float(offset))
    o = centre[:, None] + normalised(rng.normal(size=(3, n))).astype(np.float64) * 4 * scale
    t = centre[:, None] + rng.normal(size=(3, n)) * 0.6 * scale
    O, D = aim(o, t)
    return Case(name, scene, world, O, D)


def case_flat(directory):
    """Every triangle at z = 0 (zero extent on one axis): rays in the plane and across it."""
    rng = np.random.default_rng(15)
    g = np.arange(-4, 5, dtype=np.float64)
    X, Y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([X.ravel() + rng.uniform(-0.3, 0.3, X.size) * (np.abs(X.ravel()) < 4), Y.ravel() + rng.uniform(-0.3, 0.3, X.size) * (np.abs(Y.ravel()) < 4), np.zeros(X.size)], 1)
    f = []
    for i in range(8):
        for j in range(8):
            a, b, c, e = i * 9 + j, (i + 1) * 9 + j, (i + 1) * 9 + j + 1, i * 9 + j + 1
            f += [(a, b, c), (a, c, e)]
    scene, world = one_mesh(directory, "flat", v, f)
    n = 1500
    o_in = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), np.zeros(n)])
    d_in = rng.normal(size=(3, n)); d_in[2] = 0.0
    o_x = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.choice([-3.0, 3.0], n)])
    t_x = np.stack([rng.uniform(-4.5, 4.5, n), rng.uniform(-4.5, 4.5, n), np.zeros(n)])
    O1, D1 = o_in.astype(np.float32), normalised(d_in)
    O2, D2 = aim(o_x, t_x)
    return Case("flat", scene, world, np.concatenate([O1, O2], 1), np.concatenate([D1, D2], 1))


def case_icosphere(directory):
    """A closed icosphere; rays aimed exactly at its vertices and edge midpoints, from inside and outside. A miss is a leak."""
    v, f = icosphere(2)
    v = f32(v * 2.0)
    scene, world = one_mesh(directory, "icosphere", v, f)
    mids = np.array([(v[a] + v[b]) / 2 for a, b, c in f for a, b in ((a, b), (b, c), (c, a))])
    targets = np.concatenate([v, mids])
    rng = np.random.default_rng(16)
    inside = rng.normal(size=(3, len(targets))) * 0.4
    outside = normalised(rng.normal(size=(3, len(targets)))).astype(np.float64) * 6.0
    O1, D1 = aim(inside, targets.T)
    O2, D2 = aim(outside, targets.T)
    return Case("icosphere", scene, world, np.concatenate([O1, O2], 1), np.concatenate([D1, D2], 1), closed=True)


def rotation(axis, degrees):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(degrees); x, y, z = axis; c, s = np.cos(a), np.sin(a)
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def case_instanced(directory, name, count, seed, rays=3000):
    """`count` instances of the blob and a box, rotated, uniformly scaled and moved, one BLAS each under the TLAS (merge_static = 0)."""
    rng = np.random.default_rng(seed)
    bv, bf = blob(6)
    xv, xf = box((-1, -0.5, -0.25), (1, 0.5, 0.25))
    write_obj(os.path.join(directory, name + "_blob.obj"), bv, bf)
    write_obj(os.path.join(directory, name + "_box.obj"), xv, xf)
    shapes, world = [], []
    extent = 3.0 * count ** (1 / 3)
    for i in range(count):
        s = float(np.float32(rng.uniform(0.3, 1.2)))
        ax = float(np.float32(rng.uniform(0, 360))); ay = float(np.float32(rng.uniform(0, 360)))
        p = f32(rng.uniform(-extent, extent, 3))
        v, f, obj = (bv, bf, "_blob.obj") if i % 3 else (xv, xf, "_box.obj")
        shapes.append(obj_shape(name + obj, '<scale value="%r"/><rotate x="1" angle="%r"/><rotate y="1" angle="%r"/><translate x="%r" y="%r" z="%r"/>' % (s, ax, ay, float(p[0]), float(p[1]), float(p[2]))))
        m = rotation((0, 1, 0), ay) @ rotation((1, 0, 0), ax) * s
        world.append((f32(v) @ m.T + p)[np.asarray(f)])
    scene = write_scene(directory, name, shapes, eye="0, 0, %r" % (3 * extent))
    O, D = random_rays(rng, rays, np.zeros(3), extent, extent)
    return Case(name, scene, np.concatenate(world), O, D, config={"merge_static": 0})


def all_cases(directory):
    os.makedirs(directory, exist_ok=True)
    return [case_boxes(directory), case_slivers(directory), case_layers(directory), case_deep(directory),
            case_deep(directory, name="deep_instanced", config={"merge_static": 0}),
            case_scaled(directory, "scale_small", 1e-4, 0.0), case_scaled(directory, "scale_large", 1e4, 0.0),
            case_scaled(directory, "offset", 1.0, 1e5), case_flat(directory), case_icosphere(directory),
            case_instanced(directory, "instanced", 40, 17), case_instanced(directory, "instanced_many", 1100, 18, rays=600)]


def shadow_limits(t32, rng):
    """Shadow-ray limits for rays whose float32 closest hit is t32 (inf: miss): 0, +inf, exactly t32, its float32 neighbours on
    either side, and a random fraction / multiple of it -- six limits per ray, in that order."""
    t = np.asarray(t32, np.float32)
    finite = np.isfinite(t)
    base = np.where(finite, t, np.float32(1.0))
    lim = [np.zeros_like(t), np.full_like(t, np.inf), base, np.nextafter(base, np.float32(0)), np.nextafter(base, np.float32(np.inf)),
           (base * rng.uniform(0.25, 2.0, t.size)).astype(np.float32)]
    return np.stack(lim, 1).ravel()
