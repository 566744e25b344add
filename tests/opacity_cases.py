"""Masked scenes for the opacity-mask tests, and their rays. TEST INFRASTRUCTURE ONLY.

Built with the helpers of tests/trace_cases.py. Every masked shape is an OBJ with texture coordinates under a
<bsdf type="mask"> whose opacity is a 32-bit TGA written here (top-down, so that row 0 of the array is row 0 of the texture; the
mask is its alpha channel at threshold 0.5). A case carries what tests/opacity_reference.py needs: per world-space triangle the
float32 values of its shading record's uv_0, uv_edge_1, uv_edge_2 -- the OBJ loader's `1 - v` and the edge subtraction are
restated here in float32, and the GPU tests compare them with the arrays the product staged -- and the index of its mask.
"""
import os
from dataclasses import dataclass, field

import numpy as np

import trace_cases as cases

F32 = np.float32


@dataclass
class MaskedCase(cases.Case):
    uv0: np.ndarray = None               # (K, 2) float32
    uve1: np.ndarray = None
    uve2: np.ndarray = None
    mask_of_triangle: np.ndarray = None  # (K,) index into masks, -1: none
    instance_of_triangle: np.ndarray = None   # (K,) the shape (scene order) a triangle belongs to
    masks: list = field(default_factory=list)      # bool [H, W] each, True: opaque
    mask_of_instance: list = field(default_factory=list)
    more_origin: np.ndarray = None       # a second, larger ray set (beyond RT_NARROW_MAX_RAYS), or None
    more_direction: np.ndarray = None


def write_tga(path, rgba):
    """Uncompressed true-colour TGA, top-down: 32 bits per pixel for [H, W, 4], 24 for [H, W, 3]."""
    rgba = np.asarray(rgba, np.uint8)
    h, w, c = rgba.shape
    header = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, w & 255, w >> 8, h & 255, h >> 8, 8 * c, 0x20 | (8 if c == 4 else 0)])
    order = [2, 1, 0, 3][:c]
    with open(path, "wb") as f:
        f.write(header + rgba[:, :, order].tobytes())


def mask_image(opaque, rng=None):
    """An RGBA image whose alpha is 255 where `opaque` and 0 elsewhere; colours random (they must not matter)."""
    opaque = np.asarray(opaque, bool)
    rgba = np.zeros(opaque.shape + (4,), np.uint8)
    rgba[:, :, :3] = 200 if rng is None else rng.integers(0, 256, opaque.shape + (3,))
    rgba[:, :, 3] = np.where(opaque, 255, 0)
    return rgba


def write_obj_uv(path, vertices, uvs, faces):
    """v / vt / f a/a b/b c/c: one texture coordinate per vertex."""
    with open(path, "w") as f:
        for v in np.asarray(vertices, F32):
            f.write("v %r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in np.asarray(uvs, F32):
            f.write("vt %r %r\n" % (float(t[0]), float(t[1])))
        for a, b, c in faces:
            f.write("f %d/%d %d/%d %d/%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1))


def shading_uv(uvs, faces):
    """uv_0, uv_edge_1, uv_edge_2 (float32) of every face as the loader stores them: v is flipped (1 - v), edges are differences."""
    t = np.asarray(uvs, F32).copy()
    t[:, 1] = F32(1.0) - t[:, 1]
    f = np.asarray(faces)
    return t[f[:, 0]], (t[f[:, 1]] - t[f[:, 0]]).astype(F32), (t[f[:, 2]] - t[f[:, 0]]).astype(F32)


def masked_shape(obj, tga, transform=""):
    bsdf = '<bsdf type="diffuse"/>' if tga is None else \
        '<bsdf type="mask"><texture name="opacity" type="bitmap"><string name="filename" value="%s"/></texture><bsdf type="diffuse"/></bsdf>' % tga
    return '<shape type="obj"><string name="filename" value="%s"/>%s%s</shape>' % (
        obj, '<transform name="toWorld">%s</transform>' % transform if transform else "", bsdf)


def assemble(name, scene, parts, masks, origin, direction, config=None, **more):
    """parts: (world (k, 3, 3), uv0, uve1, uve2, mask index) per shape, in scene order."""
    world = np.concatenate([p[0] for p in parts])
    counts = [len(p[0]) for p in parts]
    return MaskedCase(name, scene, world, origin, direction, config=config or {},
                      uv0=np.concatenate([p[1] for p in parts]), uve1=np.concatenate([p[2] for p in parts]), uve2=np.concatenate([p[3] for p in parts]),
                      mask_of_triangle=np.concatenate([np.full(c, p[4]) for c, p in zip(counts, parts)]),
                      instance_of_triangle=np.concatenate([np.full(c, i) for i, c in enumerate(counts)]),
                      masks=masks, mask_of_instance=[p[4] for p in parts], **more)


def case_layers(directory, name="layers", config=None, seed=21, rays=4000, more_rays=24000, solid=False):
    """Six parallel quads 0.5 apart in front of an opaque wall, all under one 33 x 70 random mask (not a power of two, W x H not a
    multiple of 32, half the bits set); texture coordinates span [-1.3, 2.7] (wrap, negative values), two quads are mirrored.
    A closest-hit ray passes up to six rejected candidates. Three shapes with the identity transform: flattened into one tree
    by default (aliases), one BLAS each under the TLAS with merge_static = 0."""
    rng = np.random.default_rng(seed)
    opaque = rng.random((70, 33)) < 0.5
    if solid:   # (the identity tests: every bit 1, the rays unchanged)
        opaque = np.ones_like(opaque)
    write_tga(os.path.join(directory, name + "_mask.tga"), mask_image(opaque, rng))
    lo, hi = -1.3, 2.7
    parts, shapes = [], []
    for half in range(2):
        vs, ts, fs = [], [], []
        for k in range(3 * half, 3 * half + 3):
            z = 10.0 + 0.5 * k
            mirrored = k in (1, 4)
            base = len(vs)
            vs += [(-4, -4, z), (4, -4, z), (4, 4, z), (-4, 4, z)]
            ts += [(hi, lo), (lo, lo), (lo, hi), (hi, hi)] if mirrored else [(lo, lo), (hi, lo), (hi, hi), (lo, hi)]
            fs += [(base, base + 1, base + 2), (base, base + 2, base + 3)] if k % 2 == 0 else [(base, base + 1, base + 3), (base + 1, base + 2, base + 3)]
        obj = "%s_%d.obj" % (name, half)
        write_obj_uv(os.path.join(directory, obj), vs, ts, fs)
        shapes.append(masked_shape(obj, name + "_mask.tga"))
        parts.append((cases.f32(vs)[np.asarray(fs)], *shading_uv(ts, fs), 0))
    wall_v = [(-20, -20, 14), (20, -20, 14), (20, 20, 14), (-20, 20, 14)]
    wall_f = [(0, 1, 2), (0, 2, 3)]
    write_obj_uv(os.path.join(directory, name + "_wall.obj"), wall_v, [(0, 0), (1, 0), (1, 1), (0, 1)], wall_f)
    shapes.append(masked_shape(name + "_wall.obj", None))
    parts.append((cases.f32(wall_v)[np.asarray(wall_f)], *shading_uv([(0, 0), (1, 0), (1, 1), (0, 1)], wall_f), -1))
    scene = cases.write_scene(directory, name, shapes)

    def rays_of(n):
        o = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), np.zeros(n)])
        t = np.stack([rng.uniform(-3.5, 3.5, n), rng.uniform(-3.5, 3.5, n), np.full(n, 10.0)])
        return cases.aim(o, t)
    O, D = rays_of(rays)
    MO, MD = rays_of(more_rays) if more_rays else (None, None)
    return assemble(name, scene, parts, [opaque], O, D, config=config, more_origin=MO, more_direction=MD)


def case_instanced(directory, name="instanced", seed=22, rays=3000, drop_instance=None, masks_override=None):
    """One 8-triangle mesh (a 2 x 2 grid of quads) instanced three times, rotated, scaled and moved: instance 0 under a 64 x 64
    mask, instance 1 unmasked, instance 2 under a 5 x 3 mask. A mask looked up per triangle instead of per instance fails here.
    drop_instance: the same scene without that shape (its rays unchanged). masks_override: other bits for the two masks."""
    rng = np.random.default_rng(seed)
    masks = [rng.random((64, 64)) < 0.5, rng.random((3, 5)) < 0.5]
    if masks_override is not None:
        masks = [np.asarray(m, bool) for m in masks_override]
    for k, m in enumerate(masks):
        write_tga(os.path.join(directory, "%s_mask%d.tga" % (name, k)), mask_image(m, rng))
    g = [-1.0, 0.0, 1.0]
    vs = [(x, y, 0.0) for y in g for x in g]
    ts = [(0.75 * (x + 1), 0.75 * (y + 1) - 0.25) for y in g for x in g]     # [0, 1.5] x [-0.25, 1.25]
    fs = []
    for j in range(2):
        for i in range(2):
            a, b, c, e = j * 3 + i, j * 3 + i + 1, (j + 1) * 3 + i + 1, (j + 1) * 3 + i
            fs += [(a, b, c), (a, c, e)]
    write_obj_uv(os.path.join(directory, name + "_mesh.obj"), vs, ts, fs)
    placements = [(1.5, 20.0, 35.0, (0.0, 0.0, 0.0), 0), (1.25, -30.0, 10.0, (0.5, -0.25, 1.5), -1), (2.0, 15.0, -25.0, (-0.25, 0.5, 3.0), 1)]
    parts, shapes = [], []
    for i, (s, ax, ay, p, mask) in enumerate(placements):
        if i == drop_instance:
            continue
        tga = None if mask < 0 else "%s_mask%d.tga" % (name, mask)
        shapes.append(masked_shape(name + "_mesh.obj", tga, '<scale value="%r"/><rotate x="1" angle="%r"/><rotate y="1" angle="%r"/><translate x="%r" y="%r" z="%r"/>' % (s, ax, ay, *p)))
        m = cases.rotation((0, 1, 0), ay) @ cases.rotation((1, 0, 0), ax) * s
        parts.append(((cases.f32(vs) @ m.T + np.asarray(p))[np.asarray(fs)], *shading_uv(ts, fs), mask))
    scene = cases.write_scene(directory, name if drop_instance is None else "%s_without_%d" % (name, drop_instance), shapes)
    o = np.stack([rng.uniform(-2, 2, rays), rng.uniform(-2, 2, rays), np.full(rays, -6.0)])
    t = np.stack([rng.uniform(-2.5, 2.5, rays), rng.uniform(-2.5, 2.5, rays), rng.uniform(0.0, 3.0, rays)])
    O, D = cases.aim(o, t)
    return assemble(name, scene, parts, masks, O, D, config={"merge_static": 0})


def case_tiny(directory, name, opaque, seed=23, rays=1500):
    """A single masked quad (texture coordinates [-1, 2]: three periods) in front of an opaque wall; `opaque` is the whole mask:
    1 x 1 (bit 0, bit 1), 31 x 1, 32 x 1."""
    rng = np.random.default_rng(seed)
    opaque = np.asarray(opaque, bool)
    write_tga(os.path.join(directory, name + "_mask.tga"), mask_image(opaque, rng))
    quad_v = [(-4, -4, 10), (4, -4, 10), (4, 4, 10), (-4, 4, 10)]
    quad_t = [(-1, -1), (2, -1), (2, 2), (-1, 2)]
    f = [(0, 1, 2), (0, 2, 3)]
    wall_v = [(-20, -20, 12), (20, -20, 12), (20, 20, 12), (-20, 20, 12)]
    wall_t = [(0, 0), (1, 0), (1, 1), (0, 1)]
    write_obj_uv(os.path.join(directory, name + "_quad.obj"), quad_v, quad_t, f)
    write_obj_uv(os.path.join(directory, name + "_wall.obj"), wall_v, wall_t, f)
    scene = cases.write_scene(directory, name, [masked_shape(name + "_quad.obj", name + "_mask.tga"), masked_shape(name + "_wall.obj", None)])
    parts = [(cases.f32(quad_v)[np.asarray(f)], *shading_uv(quad_t, f), 0), (cases.f32(wall_v)[np.asarray(f)], *shading_uv(wall_t, f), -1)]
    o = np.stack([rng.uniform(-3, 3, rays), rng.uniform(-3, 3, rays), np.zeros(rays)])
    t = np.stack([rng.uniform(-3.5, 3.5, rays), rng.uniform(-3.5, 3.5, rays), np.full(rays, 10.0)])
    O, D = cases.aim(o, t)
    return assemble(name, scene, parts, [opaque], O, D)


def tiny_masks(seed=24):
    rng = np.random.default_rng(seed)
    return [("tiny_1x1_clear", np.zeros((1, 1), bool)), ("tiny_1x1_opaque", np.ones((1, 1), bool)),
            ("tiny_31x1", rng.random((1, 31)) < 0.5), ("tiny_32x1", rng.random((1, 32)) < 0.5)]


def all_cases(directory):
    """layers (flattened: `flat` with the skipping walk on and off is a matter of config), layers under the TLAS, instanced, tiny."""
    os.makedirs(directory, exist_ok=True)
    return [case_layers(directory), case_layers(directory, name="layers_tlas", config={"merge_static": 0}, more_rays=0), case_instanced(directory)] + \
        [case_tiny(directory, name, opaque) for name, opaque in tiny_masks()]


def shadow_rays(case, bf, seed=7, origin=None, direction=None):
    """Six shadow rays per closest-hit ray (trace_cases.shadow_limits) around the float32 value of the reference's closest hit."""
    origin = case.origin if origin is None else origin
    direction = case.direction if direction is None else direction
    limits = cases.shadow_limits(bf.t.astype(F32), np.random.default_rng(seed))
    return np.repeat(origin, 6, 1), np.repeat(direction, 6, 1), limits
