"""Scenes of the light-tree tests (test_light_tree.py on the CPU, test_gpu_light_tree.py on the device): small on purpose -- the shapes at which the build or the walk
can go wrong. Each case is a light_tree_reference.Scene made from explicit triangles, instance matrices and light tables; `upload` puts one on a bare device context
through the C ABI (no BVH is traversed by anything these tests call, so the node array is a placeholder).

  n1 n2 n3 n64 n65 n257 n1000   random triangles in a cube, over one to three light-mesh entries with different matrices and emissions; 1000 leaves need more than
                                one workgroup, and a level of 512 nodes a launch of its own
  equal_centres                 37 copies of one triangle: every Morton code equal, the id breaks every tie
  line, plane                   box centres on a line (the box of all leaves has zero extent in two axes) and in a plane (in one)
  point                         copies of one axis-aligned triangle and, at its centre, triangles whose three vertices coincide: zero-extent boxes, no power
  scales                        coordinates from 1e-3 to 1e4 in one scene, triangles a tenth of their distance from the origin in size
  zero_area                     a triangle whose vertices lie on a line, among live ones
  instanced                     one mesh of 8 triangles three times: as it is, scaled 2 x, and scaled (1, 3, 0.5) and rotated -- A must be the true world area
  device_tlas                   the instances of `instanced` and 40 more triangles, the TLAS built on the device: the tables name instances by scene index
"""
from ctypes import byref, c_void_p

import numpy as np

import light_tree_reference as ref

F = np.float32


def _triangles(p0, e1, e2):
    t = np.zeros((len(p0), 24), F)
    t[:, 0:3] = p0; t[:, 3:6] = e1; t[:, 6:9] = e2
    t[:, 9:12] = (0, 1, 0)
    return t


def _matrix(scale=(1, 1, 1), axis=None, angle=0.0, translate=(0, 0, 0)):
    m = np.diag(np.asarray(scale, np.float64))
    if axis is not None:
        a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
        k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        m = (np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * k @ k) @ m
    return np.concatenate([m, np.asarray(translate, np.float64)[:, None]], 1).astype(F)


def _scene(groups, emissions, matrices, position=None, extra_dark_material=True):
    """groups: one (n_i, 24) triangle array per mesh data; entry i is instance i with matrix i and light material i, over the triangles of group data[i]."""
    datas = groups["datas"]; use = groups["use"]
    first = np.concatenate([[0], np.cumsum([d.shape[0] for d in datas])]).astype(int)
    triangles = np.concatenate(datas)
    spans = np.array([[first[u], first[u + 1] - 1] for u in use], np.int32)
    entries = len(use)
    materials = np.zeros((entries + 1, 8), F); types = np.zeros(entries + 1, np.uint8)
    materials[:entries, 0:3] = emissions; types[entries] = 1   # the last material: diffuse (no instance of these scenes uses it as an emitter)
    return ref.Scene(triangles, np.stack(matrices), np.arange(entries), types, materials, np.arange(triangles.shape[0]), spans, np.arange(entries), position)


def _random(n, seed, entries):
    rng = np.random.default_rng(seed)
    cuts = sorted(rng.choice(np.arange(1, n), size=min(entries, n) - 1, replace=False)) if n > 1 and entries > 1 else []
    bounds = [0] + [int(c) for c in cuts] + [n]
    datas = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        k = b - a
        datas.append(_triangles(rng.uniform(-5, 5, (k, 3)), rng.normal(0, 0.3, (k, 3)), rng.normal(0, 0.3, (k, 3))))
    mats = [_matrix(), _matrix((1.5, 1.5, 1.5), (0, 1, 0), 0.7, (3, 1, -2)), _matrix((0.5, 2.0, 1.0), (1, 1, 0), 2.1, (-4, 0, 6))][:len(datas)]
    emis = [(10, 10, 10), (2, 30, 4), (0.5, 0.25, 7)][:len(datas)]
    return _scene({"datas": datas, "use": list(range(len(datas)))}, emis, mats)


def _copies(n, zero_extent=0):
    tri = _triangles(np.tile([[1.0, 2.0, -1.0]], (n, 1)), np.tile([[0.5, 0, 0]], (n, 1)), np.tile([[0, 0, 0.75]], (n, 1)))
    if zero_extent:
        dot = _triangles(np.tile([[1.25, 2.0, -0.625]], (zero_extent, 1)), np.zeros((zero_extent, 3)), np.zeros((zero_extent, 3)))
        tri = np.concatenate([tri[:n // 2], dot, tri[n // 2:]])
    half = tri.shape[0] // 2
    return _scene({"datas": [tri[:half], tri[half:]], "use": [0, 1]}, [(5, 5, 5), (1, 9, 1)], [_matrix(), _matrix()])


def _line():
    n = 29; rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(-20, 20, n))
    tri = _triangles(np.stack([x, np.full(n, 1.0), np.zeros(n)], 1), np.stack([rng.uniform(0.1, 0.4, n), np.zeros(n), np.zeros(n)], 1), np.stack([np.zeros(n), rng.uniform(0.1, 0.4, n), np.zeros(n)], 1))
    tri[:, 1] = 1.0 - tri[:, 7] / 2   # centres of the boxes on the line y = 1, z = 0 up to rounding; all triangles in the plane z = 0
    return _scene({"datas": [tri], "use": [0]}, [(3, 4, 5)], [_matrix()])


def _plane():
    n = 45; rng = np.random.default_rng(4)
    p0 = np.stack([rng.uniform(-8, 8, n), np.full(n, 2.0), rng.uniform(-8, 8, n)], 1)
    tri = _triangles(p0, np.stack([rng.uniform(0.2, 1, n), np.zeros(n), rng.uniform(-0.3, 0.3, n)], 1), np.stack([rng.uniform(-0.3, 0.3, n), np.zeros(n), rng.uniform(0.2, 1, n)], 1))
    return _scene({"datas": [tri], "use": [0]}, [(6, 6, 2)], [_matrix()])


def _scales():
    n = 48; rng = np.random.default_rng(5)
    r = 10.0 ** rng.uniform(-3, 4, n)
    direction = rng.normal(size=(n, 3)); direction /= np.linalg.norm(direction, axis=1)[:, None]
    tri = _triangles(direction * r[:, None], rng.normal(0, 0.1, (n, 3)) * r[:, None], rng.normal(0, 0.1, (n, 3)) * r[:, None])
    return _scene({"datas": [tri[:20], tri[20:]], "use": [0, 1]}, [(1, 1, 1), (40, 40, 40)], [_matrix(), _matrix()])


def _zero_area():
    s = _random(20, 21, 2)
    s.triangles[0, 0:9] = (1, 2, -1, 0.25, 0.125, -0.5, 0.5, 0.25, -1.0)   # entry 0 (the identity): edge_2 = 2 edge_1 in exact floats, the vertices lie on a line
    return s


def _mesh8():
    rng = np.random.default_rng(31)
    return _triangles(rng.uniform(-1, 1, (8, 3)), rng.normal(0, 0.5, (8, 3)), rng.normal(0, 0.5, (8, 3)))


def _instanced():
    mesh = _mesh8()
    mats = [_matrix(translate=(-4, 3, 0)), _matrix((2, 2, 2), translate=(0, 3, 0)), _matrix((1, 3, 0.5), (1, 2, 3), 0.9, (5, 3, 1))]
    return _scene({"datas": [mesh], "use": [0, 0, 0]}, [(8, 8, 8), (8, 8, 8), (1, 2, 12)], mats)


def _device_tlas():
    mesh = _mesh8(); rng = np.random.default_rng(32)
    more = _triangles(rng.uniform(-6, 6, (40, 3)), rng.normal(0, 0.4, (40, 3)), rng.normal(0, 0.4, (40, 3)))
    mats = [_matrix(translate=(-4, 3, 0)), _matrix((2, 2, 2), translate=(0, 3, 0)), _matrix((1, 3, 0.5), (1, 2, 3), 0.9, (5, 3, 1)), _matrix(translate=(0, 6, 0)), _matrix((0.7, 0.7, 0.7), (0, 0, 1), 1.3, (7, -2, -5))]
    return _scene({"datas": [mesh, more], "use": [0, 0, 0, 1, 1]}, [(8, 8, 8), (8, 8, 8), (1, 2, 12), (3, 3, 3), (9, 1, 1)], mats)


CASES = {
    "n1": lambda: _random(1, 11, 1), "n2": lambda: _random(2, 12, 2), "n3": lambda: _random(3, 13, 2), "n64": lambda: _random(64, 14, 3), "n65": lambda: _random(65, 15, 3),
    "n257": lambda: _random(257, 16, 3), "n1000": lambda: _random(1000, 17, 3), "equal_centres": lambda: _copies(37), "line": _line, "plane": _plane,
    "point": lambda: _copies(16, zero_extent=5), "scales": _scales, "zero_area": _zero_area, "instanced": _instanced, "device_tlas": _device_tlas,
}
DEVICE_TLAS = {"device_tlas"}
NAMES = list(CASES)


def scene(name):
    return CASES[name]()


def grid(tree, lv):
    """The points the pmf is checked at: inside the box of the lights, on a leaf's box centre (as the device computes it), far away (1e6), at a corner of the box."""
    root_lo, root_hi = tree.nodes[0, 0:3].astype(np.float64), tree.nodes[0, 4:7].astype(np.float64)
    live = np.nonzero(lv.power > 0)[0]
    k = live[len(live) // 2]
    centre = F(0.5) * (lv.lo[k] + lv.hi[k])
    rng = np.random.default_rng(7)
    inside = root_lo + rng.random((3, 3)) * (root_hi - root_lo)
    return np.concatenate([inside, centre[None], [[1e6, -1e6, 1e6]], [[3e5, 1e6, 7e5]], root_lo[None], root_hi[None], [[root_lo[0], root_hi[1], root_lo[2]]]]).astype(F)


# ---- a bare device context holding a scene -----------------------------------------------------------------------------------------

def light_tables(s):
    """Valid cumulative tables for rt_upload_lights over the scene's spans (the tree does not read them; the power selection does)."""
    lv64 = ref.leaves64(s)
    power = np.maximum(lv64[1], 0.0) + 1e-30
    entry, place, _, _, base = s.leaf_table()
    triangle_cdf = np.ones(s.triangle_indices.size, F)
    mesh_weight = np.zeros(s.spans.shape[0])
    for m in range(s.spans.shape[0]):
        w = power[base[m]:base[m + 1]]; mesh_weight[m] = w.sum()
        c = (np.cumsum(w) / w.sum()).astype(F); c[-1] = 1.0
        triangle_cdf[s.spans[m, 0]:s.spans[m, 1] + 1] = c
    mesh_cdf = (np.cumsum(mesh_weight) / mesh_weight.sum()).astype(F); mesh_cdf[-1] = 1.0
    return triangle_cdf, mesh_cdf, float(mesh_weight.sum())


def upload(grt, s, device_tlas=False, device=0):
    """A context holding scene `s` (geometry, instances, materials, light tables). Returns (ctx, scene as the device holds it): with device_tlas the instance
    tables are gathered into TLAS order by rt_build_tlas and the returned scene carries that order and the position map. Destroy with lib.rt_destroy(ctx)."""
    lib = grt.device_lib()
    ctx = c_void_p()
    assert lib.rt_create(device, byref(ctx)) == 0, lib.rt_last_error(None)
    n = s.transforms.shape[0]
    nodes = np.zeros((2 * n + 2, 20), np.uint32)
    assert lib.rt_upload_geometry(ctx, s.triangles.ctypes.data, s.triangles.shape[0], nodes.ctypes.data, nodes.shape[0]) == 0, lib.rt_last_error(ctx)
    roots = np.full(n, 2 * n, np.int32)
    forward = np.ascontiguousarray(s.transforms.reshape(n, 12))
    inverse = np.zeros((n, 12), F)
    for i in range(n):
        m4 = np.eye(4); m4[:3] = s.transforms[i]
        inverse[i] = np.linalg.inv(m4)[:3].reshape(12)
    ids = np.ascontiguousarray(s.material_ids, np.int32)
    out = s
    if device_tlas:
        boxes = np.tile(np.array([-1, -1, -1, 1, 1, 1], F), (n, 1))
        assert lib.rt_build_tlas(ctx, roots.ctypes.data, ids.ctypes.data, forward.ctypes.data, inverse.ctypes.data, forward.ctypes.data, boxes.ctypes.data, n) == 0, lib.rt_last_error(ctx)
    else:
        assert lib.rt_upload_instances(ctx, roots.ctypes.data, ids.ctypes.data, forward.ctypes.data, inverse.ctypes.data, forward.ctypes.data, n) == 0, lib.rt_last_error(ctx)
    assert lib.rt_upload_materials(ctx, s.material_types.ctypes.data, s.materials.ctypes.data, s.material_types.size) == 0, lib.rt_last_error(ctx)
    triangle_cdf, mesh_cdf, weight = light_tables(s)
    assert grt.upload_lights(ctx, s.triangle_indices, triangle_cdf, mesh_cdf, s.spans, s.transform_indices, weight) == 0, lib.rt_last_error(ctx)
    if device_tlas:
        t = np.zeros((n, 12), F); mat = np.zeros(n, np.int32); position = np.zeros(n, np.int32)
        assert lib.rt_read_instances(ctx, None, mat.ctypes.data, t.ctypes.data, None, None, position.ctypes.data) == 0, lib.rt_last_error(ctx)
        out = ref.Scene(s.triangles, t, mat, s.material_types, s.materials, s.triangle_indices, s.spans, s.transform_indices, position)
    return ctx, out


# ---- scenes loaded through the host library (frames) ---------------------------------------------------------------------------------

def scene_from_pathtracer(pt):
    """The reference Scene of what a Pathtracer stages (with or without a device): the tree the device builds from it is build32 of this, bit for bit."""
    return ref.Scene(pt.array("triangles").reshape(-1, 24), pt.array("mesh_transforms").reshape(-1, 3, 4), pt.array("mesh_material_ids"), pt.array("material_types"),
                     pt.array("materials").reshape(-1, 8), pt.array("light_triangle_indices"), pt.array("light_mesh_triangle_span").reshape(-1, 2),
                     pt.array("light_mesh_transform_indices"))


WORLD = dict(grid=16, spacing=2.0, height=1.5, half=0.15, radiance=60.0, floor_half=40.0, albedo=0.7)
WORLD_SENSOR = '<sensor type="perspective"><float name="fov" value="50"/><transform name="toWorld"><lookat origin="0, 16, 26" target="0, 0, 2" up="0, 1, 0"/></transform></sensor>'


def write_many_lights(directory, grid=None, name="many_lights", sensor=WORLD_SENSOR, **changes):
    """The small many-light world: grid x grid small quads (each a shape of its own: a light-mesh entry of two triangles) facing down over a wide diffuse floor."""
    import os
    w = dict(WORLD, **changes)
    g = grid or w["grid"]
    os.makedirs(str(directory), exist_ok=True)
    xml = ('<scene version="0.5.0"><integrator type="path"><integer name="maxDepth" value="2"/></integrator>' + sensor +
           '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><scale value="%g"/></transform>'
           '<bsdf type="diffuse"><rgb name="reflectance" value="%g, %g, %g"/></bsdf></shape>' % (w["floor_half"], w["albedo"], w["albedo"], w["albedo"]))
    for i in range(g):
        for j in range(g):
            x = (i - (g - 1) / 2) * w["spacing"]; z = (j - (g - 1) / 2) * w["spacing"]
            xml += ('<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="90"/><scale value="%g"/><translate x="%g" y="%g" z="%g"/></transform>'
                    '<emitter type="area"><rgb name="radiance" value="%g, %g, %g"/></emitter></shape>' % (w["half"], x, w["height"], z, w["radiance"], w["radiance"], w["radiance"]))
    path = os.path.join(str(directory), name + ".xml")
    with open(path, "w") as f:
        f.write(xml + "</scene>")
    return path


def footprints(camera, xs, ys, sub=2):
    """Where sub x sub stratified rays through each pixel (xs, ys) meet the floor y = 0: (K, sub^2, 3). The pixels are floor_points' (they see the floor)."""
    o = np.array(camera.position[:3], np.float64)
    offsets = (np.arange(sub) + 0.5) / sub
    out = np.empty((len(xs), sub * sub, 3))
    for j, (ox, oy) in enumerate((a, b) for a in offsets for b in offsets):
        d = (np.array(camera.bottom_left_corner[:3], np.float64)[None] + (xs + ox)[:, None] * np.array(camera.x_axis[:3], np.float64)[None]
             + (ys + oy)[:, None] * np.array(camera.y_axis[:3], np.float64)[None])
        out[:, j] = o[None] + (-o[1] / d[:, 1])[:, None] * d
    return out


def floor_points(camera, width, height, step, world=WORLD, grid=None):
    """Where the centre rays of every `step`-th pixel meet the floor y = 0, for the pixels that see the floor and no lamp: (pixel x, pixel y, points (K, 3))."""
    g = grid or world["grid"]
    xs, ys = np.meshgrid(np.arange(step // 2, width, step), np.arange(step // 2, height, step))
    xs, ys = xs.ravel(), ys.ravel()
    o = np.array(camera.position[:3], np.float64)
    d = (np.array(camera.bottom_left_corner[:3], np.float64)[None] + (xs + 0.5)[:, None] * np.array(camera.x_axis[:3], np.float64)[None]
         + (ys + 0.5)[:, None] * np.array(camera.y_axis[:3], np.float64)[None])
    keep = d[:, 1] < 0
    t = np.where(keep, -o[1] / np.where(keep, d[:, 1], -1.0), 0.0)
    p = o[None] + t[:, None] * d
    keep &= (np.abs(p[:, 0]) < world["floor_half"]) & (np.abs(p[:, 2]) < world["floor_half"])
    at_lamps = o[None] + ((world["height"] - o[1]) / np.where(d[:, 1] < 0, d[:, 1], -1.0))[:, None] * d   # where the ray crosses the lamps' plane
    extent = (g - 1) / 2 * world["spacing"]
    fx = (at_lamps[:, 0] + extent) / world["spacing"]; fz = (at_lamps[:, 2] + extent) / world["spacing"]
    near = (np.abs(fx - np.round(fx)) * world["spacing"] < 2 * world["half"]) & (np.abs(fz - np.round(fz)) * world["spacing"] < 2 * world["half"]) & (np.abs(at_lamps[:, 0]) < extent + 1) & (np.abs(at_lamps[:, 2]) < extent + 1)
    keep &= ~near
    return xs[keep], ys[keep], p[keep]


def simulate_selection(c, pmf, samples, rng):
    """`samples` draws of the one-sample estimator c_k / pmf_k of a point's direct light: their mean and the Welford standard error of that mean."""
    live = pmf > 0
    k = rng.choice(np.nonzero(live)[0], size=samples, p=pmf[live] / pmf[live].sum())
    x = c[k] / pmf[k]
    return x.mean(), np.sqrt(x.var(ddof=1) / samples)
