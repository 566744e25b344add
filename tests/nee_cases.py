"""Scenes and probe grids of the light-sampling tests (test_nee.py on the CPU, test_gpu_nee.py on the device).

The scenes are written into a temporary directory and loaded through the host library, so the light tables under test are the
ones `Pathtracer` stages for a frame:

* few       -- four light-mesh entries over three mesh datas: a rectangle; an irregular quad as a scaled and rotated instance; two
               instances of one strip mesh with different emission, one of them scaled and rotated too. The strip's FIRST triangle
               has zero area (two equal consecutive table entries at the head of its span).
* limit     -- 64 instances of one mesh data of exactly 2048 triangles of unequal area, with different scales: both LDS limits met.
* meshes65  -- 65 such instances: one light mesh past RT_LIGHT_MESHES_IN_LDS.
* tris2049  -- three instances of a mesh data of 2049 triangles: one triangle past RT_LIGHT_TRIANGLES_IN_LDS.
"""
import os

import numpy as np

LIGHT_MESHES_IN_LDS, LIGHT_TRIANGLES_IN_LDS = 64, 2048   # RT_LIGHT_MESHES_IN_LDS, RT_LIGHT_TRIANGLES_IN_LDS (rt_lights.h)
ONE_BELOW_ONE = np.float32(np.nextafter(np.float32(1), np.float32(0)))   # 0x1.fffffep-1

HEAD = ('<scene version="0.5.0"><integrator type="path"><integer name="maxDepth" value="4"/></integrator>'
        '<sensor type="perspective"><float name="fov" value="50"/><transform name="toWorld"><lookat origin="0, 3, 12" target="0, 2, 0" up="0, 1, 0"/></transform></sensor>'
        '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><scale value="20"/></transform><bsdf type="diffuse"><rgb name="reflectance" value="0.6, 0.6, 0.6"/></bsdf></shape>')


def _emitter(filename, radiance, scale, axis, angle, translate):
    return ('<shape type="obj"><string name="filename" value="%s"/><transform name="toWorld"><scale value="%.6f"/><rotate %s="1" angle="%.4f"/>'
            '<translate x="%.5f" y="%.5f" z="%.5f"/></transform><emitter type="area"><rgb name="radiance" value="%g, %g, %g"/></emitter></shape>'
            % ((filename, scale, axis, angle) + tuple(translate) + tuple(radiance)))


def ribbon_obj(triangles, seed):
    """A ribbon in the plane y = 0 with exactly `triangles` triangles of unequal area, facing -y."""
    rng = np.random.default_rng(seed)
    quads = (triangles + 1) // 2
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.2, 1.8, quads))]) * (4.0 / quads)
    z = rng.uniform(0.3, 1.0, quads + 1)
    lines = []
    for i in range(quads + 1):
        lines.append("v %.7f 0 %.7f" % (x[i] - 2.0, -z[i]))
        lines.append("v %.7f 0 %.7f" % (x[i] - 2.0, z[i]))
    faces = []
    for i in range(quads):
        a, b, c, d = 2 * i + 1, 2 * i + 2, 2 * i + 3, 2 * i + 4
        faces.append("f %d %d %d" % (a, c, b)); faces.append("f %d %d %d" % (b, c, d))
    return "\n".join(lines + faces[:triangles]) + "\n"


def write_few(directory):
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "quad.obj"), "w") as f:   # two triangles of areas 1.5 and 0.7
        f.write("v -1 0 -1\nv 1 0 -1\nv 0.4 0 0.4\nv -1 0 0.5\nf 1 2 3\nf 1 3 4\n")
    with open(os.path.join(directory, "strip.obj"), "w") as f:  # the first triangle is a line: zero area
        f.write("v 0 0 0\nv 1 0 0\nv 2 0 0\nv 0 0 1\nv 1 0 1.5\nv 2.5 0 1\nv 3 0 0\n"
                "f 1 2 3\nf 1 2 4\nf 2 5 4\nf 2 3 5\nf 3 6 5\nf 3 7 6\n")
    xml = HEAD
    xml += ('<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="90"/><scale value="0.75"/><translate x="-3" y="5" z="0.5"/></transform>'
            '<emitter type="area"><rgb name="radiance" value="10, 10, 10"/></emitter></shape>')
    xml += _emitter("quad.obj", (20, 5, 5), 0.5, "z", 160.0, (2.5, 4.0, -1.0))
    xml += _emitter("strip.obj", (4, 6, 12), 1.0, "x", 180.0, (-1.5, 6.0, 2.0))
    xml += _emitter("strip.obj", (12, 6, 2), 1.7, "z", 205.0, (3.0, 3.0, 3.0))
    path = os.path.join(directory, "few.xml")
    with open(path, "w") as f:
        f.write(xml + "</scene>")
    return path


def write_instances(directory, name, triangles, instances, seed):
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, name + ".obj"), "w") as f:
        f.write(ribbon_obj(triangles, seed))
    rng = np.random.default_rng(seed + 100)
    xml = HEAD
    for i in range(instances):
        xml += _emitter(name + ".obj", (6, 7, 8), rng.uniform(0.3, 1.5), "xz"[i % 2], 180.0 + rng.uniform(-35, 35),
                        (rng.uniform(-8, 8), rng.uniform(3, 9), rng.uniform(-8, 8)))
    path = os.path.join(directory, name + ".xml")
    with open(path, "w") as f:
        f.write(xml + "</scene>")
    return path


class Case:
    def __init__(self, name, write, config, lds, meshes, triangles):
        self.name, self.write, self.config, self.lds, self.meshes, self.triangles = name, write, config, lds, meshes, triangles


def _cases(device_tlas):
    out = []
    for tlas in ((0, 1) if device_tlas else (0,)):
        t = {"device_tlas": tlas}
        tag = "_device_tlas" if tlas else ""
        for merge in (0, 1):
            out.append(Case("few_merge%d%s" % (merge, tag), write_few, dict(t, merge_static=merge), True, 4, 10))
        out.append(Case("limit" + tag, lambda d: write_instances(d, "limit", 2048, 64, 11), dict(t), True, 64, 2048))
        out.append(Case("meshes65" + tag, lambda d: write_instances(d, "meshes65", 2048, 65, 12), dict(t), False, 65, 2048))
        out.append(Case("tris2049" + tag, lambda d: write_instances(d, "tris2049", 2049, 3, 13), dict(t), False, 3, 2049))
    return out


CPU_CASES = _cases(False)   # device_tlas needs a device: the host-only integrator builds its TLAS on the host
GPU_CASES = _cases(True)


def load(grt, case, directory, device, width=32, height=32):
    """(scene, pathtracer) of a case, updated once, so the light tables are staged (and uploaded, with a device)."""
    path = case.write(str(directory))
    grt.config_reset(); grt.config_set(**case.config)
    scene = grt.Scene(path)
    grt.config_set(**case.config)
    pt = grt.Pathtracer(scene, width, height, device=device)
    pt.update()
    return scene, pt


def _neighbours(values):
    """Every value, the float32 below it and the float32 above it, kept to [0, 1)."""
    v = np.asarray(values, np.float32)
    v = v[np.isfinite(v)]
    out = np.concatenate([v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2)), np.array([0.0, ONE_BELOW_ONE], np.float32)])
    return np.unique(out[(out >= 0) & (out < 1)])


def _fill(u_mesh, u_triangle, seed):
    n = u_mesh.size
    rng = np.random.default_rng(seed)
    p = np.empty((n, 4), np.float32)
    p[:, 0] = u_mesh; p[:, 1] = u_triangle
    p[:, 2:] = rng.random((n, 2), np.float32)
    p[:, 2:] = np.minimum(p[:, 2:], ONE_BELOW_ONE)
    return p


def edge_probes(tables):
    """u on every table entry, its two float neighbours, 0 and 0x1.fffffep-1: every mesh-table edge value with a few u_triangle, and
    for every light-mesh entry (selected by a u_mesh inside its interval) every edge value of its span of the triangle table."""
    mesh_cdf = tables.mesh_cdf
    mesh_edges = _neighbours(mesh_cdf)
    tri_few = np.array([0.0, 0.25, 0.5, ONE_BELOW_ONE], np.float32)
    um = [np.repeat(mesh_edges, tri_few.size)]; ut = [np.tile(tri_few, mesh_edges.size)]
    lower = np.concatenate([[np.float32(0)], mesh_cdf[:-1]])
    inside = ((lower.astype(np.float64) + mesh_cdf) / 2).astype(np.float32)
    for m in range(mesh_cdf.size):
        first, last = tables.spans[m]
        edges = _neighbours(tables.triangle_cdf[first:last + 1])
        um.append(np.full(edges.size, inside[m], np.float32)); ut.append(edges)
    return _fill(np.concatenate(um), np.concatenate(ut), 5)


def stratified_probes(n=256, seed=6):
    """An n x n stratified grid of (u_mesh, u_triangle), jittered, with random (u_1, u_2)."""
    rng = np.random.default_rng(seed)
    j = rng.random((n, n, 2))
    um = ((np.arange(n)[:, None] + j[:, :, 0]) / n).astype(np.float32).reshape(-1)
    ut = ((np.arange(n)[None, :] + j[:, :, 1]) / n).astype(np.float32).reshape(-1)
    return _fill(np.minimum(um, ONE_BELOW_ONE), np.minimum(ut, ONE_BELOW_ONE), seed + 1)


def uniform_probes(count=1 << 20, seed=7):
    """`count` independent uniform probes (fixed seed) for the goodness-of-fit tests."""
    rng = np.random.default_rng(seed)
    return np.minimum(rng.random((count, 4), np.float32), ONE_BELOW_ONE)
