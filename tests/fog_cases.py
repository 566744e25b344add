"""Shared cases of the fog tests (test_fog.py, test_gpu_fog.py): the box, the volumes, the segments of the clip, the shadow queues of the
attenuation pass, and the scene files of the frame tests."""
import math
import os

import numpy as np

BOX_MIN = np.array([-1.0, -0.5, 2.0], np.float32)
BOX_MAX = np.array([1.0, 1.5, 4.0], np.float32)

# name -> (sigma_a, sigma_s, g)
VOLUMES = {
    "grey":       ((0.0, 0.0, 0.0), (0.7, 0.7, 0.7), 0.0),
    "absorbing":  ((0.9, 0.4, 0.1), (0.0, 0.0, 0.0), 0.0),
    "unequal":    ((0.1, 0.2, 0.05), (1.5, 0.6, 0.2), 0.6),
    "one_channel": ((0.0, 0.3, 0.0), (0.0, 0.0, 2.0), -0.4),
}
THROUGHPUTS = [(1.0, 1.0, 1.0), (0.5, 0.0, 0.25), (0.0, 0.0, 0.7), (0.2, 0.9, 0.4)]

R2 = math.sqrt(0.5)
R3 = math.sqrt(1.0 / 3.0)
INF = math.inf
# name -> (origin, direction, t_end); what the clip must make of it stands in the name
SEGMENTS = {
    "outside_through":       ((0.0, 0.5, 0.0), (0.0, 0.0, 1.0), INF),
    "inside":                ((0.2, 0.3, 3.0), (R3, R3, R3), INF),
    "inside_backwards":      ((0.2, 0.3, 3.0), (-R3, -R3, -R3), INF),
    "on_face_entering":      ((0.0, 0.5, 2.0), (0.0, 0.0, 1.0), INF),
    "on_face_leaving":       ((0.0, 0.5, 2.0), (0.0, 0.0, -1.0), INF),
    "on_face_parallel":      ((0.0, 0.5, 2.0), (1.0, 0.0, 0.0), INF),
    "on_face_parallel_neg0": ((0.0, 0.5, 4.0), (-1.0, -0.0, -0.0), INF),
    "on_corner_entering":    ((-1.0, -0.5, 2.0), (R3, R3, R3), INF),
    "on_corner_leaving":     ((-1.0, -0.5, 2.0), (-R3, R3, R3), INF),
    "miss":                  ((3.0, 0.5, 0.0), (0.0, 0.0, 1.0), INF),
    "miss_behind":           ((0.0, 0.5, 5.0), (0.0, 0.0, 1.0), INF),
    "edge_through":          ((-2.0, 0.5, 1.0), (R2, 0.0, R2), INF),
    "edge_graze":            ((-2.0, 0.5, 3.0), (R2, 0.0, -R2), INF),
    "parallel_outside_pos0": ((0.0, 2.0, 0.0), (0.0, 0.0, 1.0), INF),
    "parallel_outside_neg0": ((0.0, 2.0, 0.0), (-0.0, -0.0, 1.0), INF),
    "parallel_inside_neg0":  ((0.3, 0.5, 0.0), (-0.0, 0.0, 1.0), INF),
    "parallel_two_axes":     ((0.3, -0.5, 0.0), (0.0, -0.0, 1.0), INF),
    "subnormal_component":   ((-1.0, 0.5, 0.0), (1e-42, 0.0, 1.0), INF),
    "end_before_entry":      ((0.0, 0.5, 0.0), (0.0, 0.0, 1.0), 1.5),
    "end_at_entry":          ((0.0, 0.5, 0.0), (0.0, 0.0, 1.0), 2.0),
    "end_inside":            ((0.0, 0.5, 0.0), (0.0, 0.0, 1.0), 3.0),
    "end_inside_from_inside": ((0.2, 0.3, 3.0), (R3, R3, R3), 0.25),
    "end_beyond":            ((0.0, 0.5, 0.0), (0.0, 0.0, 1.0), 7.0),
    "diagonal":              ((-3.0, -2.0, 0.5), (0.5883484, 0.39223227, 0.70710677), INF),
    "long_way":              ((0.0, 0.5, -1000.0), (0.0, 0.0, 1.0), INF),
}
# (pixel, bounce, sample) of the paths every segment is probed with; pixels stay below the 64 x 64 frame of the probing context
PATHS = [(0, 0, 0), (1, 0, 0), (17, 1, 3), (4095, 2, 4095), (2048, 0, 4096), (333, 5, 70000), (63, 127, 1), (1000, 3, 12)]


def segment_probes():
    """Every segment on every path: (names, origins (N, 3), directions (N, 3), t_end (N,), pixel, bounce, sample (N,) each)."""
    names, o, d, t, px, b, s = [], [], [], [], [], [], []
    for name, (origin, direction, t_end) in SEGMENTS.items():
        for pixel, bounce, sample in PATHS:
            names.append(name); o.append(origin); d.append(direction); t.append(t_end); px.append(pixel); b.append(bounce); s.append(sample)
    return names, np.array(o, np.float32), np.array(d, np.float32), np.array(t, np.float32), np.array(px, np.uint32), np.array(b, np.uint32), np.array(s, np.uint32)


def shadow_queue(count, seed):
    """A shadow queue of `count` rays around the box, (count, 11) uint32 {origin, direction, max_distance, illumination, pixel word}: rays that
    cross the box, miss it, start inside it, end inside it, run to infinity; the segments above among them."""
    rng = np.random.default_rng(seed)
    q = np.zeros((count, 11), np.uint32); f = q.view(np.float32)
    centre, half = (BOX_MIN + BOX_MAX) / 2, (BOX_MAX - BOX_MIN) / 2
    o = centre + rng.uniform(-2.5, 2.5, (count, 3)) * half
    target = centre + rng.uniform(-1.5, 1.5, (count, 3)) * half
    d = target - o; length = np.linalg.norm(d, axis=1); d /= length[:, None]
    md = np.where(rng.random(count) < 0.4, np.inf, length * rng.uniform(0.2, 2.0, count))
    segments = list(SEGMENTS.values())
    for i in range(min(count, len(segments))):
        o[i], d[i], md[i] = segments[i]
    f[:, 0:3] = o; f[:, 3:6] = d; f[:, 6] = md
    f[:, 7:10] = rng.uniform(0.0, 4.0, (count, 3))
    q[:, 10] = rng.integers(0, 1 << 30, count, dtype=np.uint32) | (rng.integers(0, 2, count, dtype=np.uint32) << 30)
    return q


# ---- scene files --------------------------------------------------------------------------------------------------------
# The frame tests need a scene with geometry and (for light samples split with emitters) an emitter, neither of which a path may reach: a
# rectangle of side 2e-3 at a distance of 1e3 behind the camera subtends 4e-12 sr.

def _write(directory, name, xml):
    os.makedirs(str(directory), exist_ok=True)
    path = os.path.join(str(directory), name + ".xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def sensor(fov):
    return ('<sensor type="perspective"><float name="fov" value="%g"/><transform name="toWorld"><lookat origin="0, 0.5, -3" target="0, 0.5, 3" up="0, 1, 0"/></transform></sensor>' % fov)


FAR_SPECK = ('<shape type="rectangle"><transform name="toWorld"><scale value="0.001"/><translate x="0" y="0.5" z="-1000"/></transform>%s</shape>')


def write_empty_scene(directory, name="empty", fov=20.0, emitter_xml="", speck_emits=False):
    """The camera at (0, 0.5, -3) looking down +z at the box of this file, and a speck far behind it: diffuse, or an emitter of radiance 1e-6."""
    inner = ('<emitter type="area"><rgb name="radiance" value="1e-6, 1e-6, 1e-6"/></emitter>' if speck_emits
             else '<bsdf type="diffuse"><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>')
    return _write(directory, name, '<scene version="0.5.0"><integrator type="path"/>' + sensor(fov) + (FAR_SPECK % inner) + emitter_xml + "</scene>")


# the frame tests' constants, shared by the CPU and the GPU file
FURNACE_SIGMA = 0.25    # optical depth 0.5 across the 2 wide box
FURNACE_BOUNCES = 26    # the smallest bounce limit whose truncation bound is below 1e-6 (test_fog.py)
SHAFT = dict(sigma_a=0.05, sigma_s=0.3, g=0.5, samples=4096)


def write_fog_shape_scene(directory, name, shapes):
    """The empty scene plus the given shape elements (the loader tests)."""
    return _write(directory, name, '<scene version="0.5.0"><integrator type="path"/>' + sensor(20.0) + (FAR_SPECK % '<bsdf type="diffuse"/>') + shapes + "</scene>")


FOG_MEDIUM = ('<medium type="homogeneous" name="interior"><rgb name="sigmaA" value="0.125, 0.25, 0.5"/><rgb name="sigmaS" value="1, 2, 4"/><float name="scale" value="0.5"/>'
              '<phase type="hg"><float name="g" value="0.25"/></phase></medium>')
FOG_CUBE = ('<shape type="cube"><transform name="toWorld"><scale x="1" y="2" z="0.5"/><translate x="3" y="0" z="-1"/></transform><bsdf type="null"/>' + FOG_MEDIUM + '</shape>')
FOG_SPHERE = ('<shape type="sphere"><float name="radius" value="2"/><bsdf type="null"/>' + FOG_MEDIUM + '</shape>')

SHAFT_LIGHT = (0.0, 4.6, 3.0)        # above the box: 3.1 from its top face, at least 2.9 from every camera ray of a 20 degree view (the box is 2 wide)
SHAFT_INTENSITY = 40.0


def shaft_emitter():
    return '<emitter type="point"><point name="position" x="%g" y="%g" z="%g"/><rgb name="intensity" value="%g, %g, %g"/></emitter>' % (SHAFT_LIGHT + (SHAFT_INTENSITY,) * 3)
