"""The shapes of tests/test_generate.py and tests/test_gpu_generate.py: frames, queue orders, submissions, sample batches, cameras and filters for the
three generate launches, each named for what it can break. Not a cross product: order x frame x submission, samples x kernel, filter x camera."""
import os
from collections import namedtuple

import numpy as np

import generate_reference as ref

# ---- frames (width, height) ---------------------------------------------------------------------------------------
FRAMES = [
    (1, 1),      # pitch 32, frame_pixels 32
    (5, 3),      # narrower than a block, lower than a band
    (8, 8),      # exactly one patch: all fast path
    (9, 9),      # one column and one row beyond a patch
    (33, 17),    # pitch 64 != width, one clipped column block, one clipped band
    (64, 8),     # one band of whole patches
    (40, 20),    # clipped tiles
    (136, 24),   # x and y beyond the 128-texel blue-noise tile
]
RAY_FRAME = (33, 17)          # the frame of the filter x camera families and of the sample batches
WRAP_FRAME = (136, 24)
STRIDE_FRAME = (256, 136)     # x 16 samples: 557 056 rays, more than the 2 048 x 256 threads of the stream kernels' grid
GRID_THREADS = 2048 * 256

# ---- queue orders (block_width, band_rows); None: the scheduler's choice -----------------------------------------
ORDERS = [(0, 0), (8, 8), (16, 4), None]   # (16, 4): not shipped -- the generic path on whole blocks

# ---- sample batches (first sample, count, slot_base) ---------------------------------------------------------------
SAMPLES = [
    (0, 1, 0),
    (0, 4, 3),
    (0, 1, 511),       # sample 0 in the highest slot: sample_index + s - slot is negative and wraps as unsigned
    (4094, 4, 508),    # crosses sample 4096: PMJ table to hash fallback
    (5, 16, 0),
]
SVGF_SAMPLES = [(first, count, slot_base) for first in (1, 2, 3) for count, slot_base in ((1, 2), (4, 7))]   # every TAA residue first of a batch at some slot
SPLITS = [[(5, 16)], [(5 + k, 1) for k in range(16)], [(5 + 4 * k, 4) for k in range(4)], [(5, 5), (10, 11)]]   # 16 = 16 x 1 = 4 x 4 = 5 + 11

# ---- queue placement -----------------------------------------------------------------------------------------------
PLACEMENTS = [(before, offset, parity) for before in (0, 1, 63, 64) for offset in (0, 7) for parity in (0, 1)]
GUARD = 5                     # entries behind the last ray that must keep their sentinel
SENTINEL = 0xA5C3F00D

# ---- cameras and filters ---------------------------------------------------------------------------------------
Camera = namedtuple("Camera", "name sensor origin target")
PINHOLE = Camera("pinhole", '<sensor type="perspective"><float name="fov" value="45"/>', "0.25, 2.5, 7", "0, 0.5, 0")
THIN = Camera("thin lens", '<sensor type="thinlens"><float name="fov" value="45"/><float name="apertureRadius" value="0.15"/><float name="focusDistance" value="4"/>', "0.25, 2.5, 7", "0, 0.5, 0")
FAR = Camera("thin lens far from the origin", THIN.sensor, "1000.25, 2.5, -700.5", "1000, 0.5, -707.5")   # the origin's ulp is 6e-5
NARROW = Camera("narrow field of view", '<sensor type="perspective"><float name="fov" value="2"/>', "0.25, 2.5, 7", "0, 0.5, 0")   # neighbouring directions differ in the last bits

Family = namedtuple("Family", "name camera filter svgf direction_angle origin_ulps")
# direction_angle (radians) and origin_ulps (ulps of the origin's largest coordinate): the oracle's largest distance to the float64 reference over the
# family's rays, measured by test_generate.py::test_the_oracle_stays_within_the_measured_distance_of_float64 on the CPU (glibc's logf, sinf, cosf) and
# rounded up to two digits; that test holds the oracle to them. The device is allowed DEVICE_FACTOR times as much: ocml's logf and sincosf differ
# from glibc's by a few ulp in either direction and the rest of the chain is the same float32 arithmetic. Device against oracle: the same bound.
DEVICE_FACTOR = 2.0
FAMILIES = [
    Family("box pinhole",        PINHOLE, ref.FILTER_BOX,      0, 1.4e-7, 0.0),   # measured 1.312e-7, 0
    Family("tent pinhole",       PINHOLE, ref.FILTER_TENT,     0, 1.2e-7, 0.0),   # measured 1.157e-7, 0
    Family("gaussian pinhole",   PINHOLE, ref.FILTER_GAUSSIAN, 0, 1.4e-7, 0.0),   # measured 1.309e-7, 0 (with the 136 x 24 frame)
    Family("box thin lens",      THIN,    ref.FILTER_BOX,      0, 1.1e-7, 0.51),   # measured 1.005e-7, 0.5087
    Family("tent thin lens",     THIN,    ref.FILTER_TENT,     0, 1.2e-7, 0.51),   # measured 1.112e-7, 0.5087
    Family("gaussian thin lens", THIN,    ref.FILTER_GAUSSIAN, 0, 1.2e-7, 0.51),   # measured 1.164e-7, 0.5087
    Family("svgf pinhole",       PINHOLE, ref.FILTER_GAUSSIAN, 1, 1.1e-7, 0.0),   # measured 1.073e-7, 0
    Family("gaussian far",       FAR,     ref.FILTER_GAUSSIAN, 0, 1.2e-7, 0.5),   # measured 1.164e-7, 0.4999
    Family("gaussian narrow",    NARROW,  ref.FILTER_GAUSSIAN, 0, 7.6e-8, 0.0),   # measured 7.599e-8, 0
]
DEFAULT_FAMILY = FAMILIES[2]


def family_samples(family):
    return SVGF_SAMPLES if family.svgf else [SAMPLES[1], SAMPLES[3]]


def write_scene(directory, camera):
    """One diffuse rectangle under `camera`; no emitters (nothing here traces a ray)."""
    path = os.path.join(str(directory), "generate_%s.xml" % camera.name.replace(" ", "_"))
    with open(path, "w") as f:
        f.write('<scene version="0.5.0"><integrator type="path"><integer name="maxDepth" value="2"/></integrator>%s'
                '<transform name="toWorld"><lookat origin="%s" target="%s" up="0, 1, 0"/></transform></sensor>'
                '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><scale value="6"/></transform>'
                '<bsdf type="diffuse"><rgb name="reflectance" value="0.7, 0.6, 0.5"/></bsdf></shape></scene>' % (camera.sensor, camera.origin, camera.target))
    return path


def load(grt, directory, family, width, height, device):
    """(scene, pathtracer) of `family` at width x height; device -1 stages the scene without a GPU."""
    settings = dict(reconstruction_filter=family.filter, enable_svgf=family.svgf)
    grt.config_reset(); grt.config_set(**settings)
    scene = grt.Scene(write_scene(directory, family.camera))
    grt.config_set(**settings)
    pt = grt.Pathtracer(scene, width, height, device=device)
    pt.update()
    return scene, pt


def reference_camera(pt):
    c = pt.camera()
    return ref.Camera(list(c.position), list(c.bottom_left_corner), list(c.x_axis), list(c.y_axis), c.aperture_radius, c.focal_distance)


class Expectation:
    """The whole frame of one family, per sample: the oracle's float32 rays and the float64 rays from the oracle's random pairs, by scan-line index.
    Computed once per sample and kept."""
    def __init__(self, oracle, pt, family, width, height):
        self.view, self.family, self.width, self.height = oracle.SceneView(pt), family, width, height
        self.camera = reference_camera(pt)
        self.pitch = pt.pitch
        self.samples = {}

    def sample(self, index):
        if index not in self.samples:
            w, h, n = self.width, self.height, self.width * self.height
            o, d, px = self.view.generate(index, 0, n)
            scan = np.arange(n)
            x, y = scan % w, scan // w
            assert np.array_equal(px, x + y * self.pitch)
            u_filter, u_aperture = self.view.random(ref.DIM_FILTER, px, 0, index), self.view.random(ref.DIM_APERTURE, px, 0, index)
            ro, rd = ref.rays(x, y, u_filter, u_aperture, self.camera, self.family.filter, self.family.svgf, np.full(n, index))
            self.samples[index] = dict(oracle_origin=o.T.copy(), oracle_direction=d.T.copy(), origin=ro, direction=rd, u_filter=u_filter, u_aperture=u_aperture)
        return self.samples[index]

    def gather(self, name, scan, sample_index):
        """`name` for queue entries given as (scan-line index, sample index) arrays."""
        if scan.size == 0:
            return np.zeros((0, 3))
        tables = {int(s): self.sample(int(s))[name] for s in np.unique(sample_index)}
        first = next(iter(tables.values()))
        out = np.empty((scan.size, first.shape[1]), first.dtype)
        for s, table in tables.items():
            rows = sample_index == s
            out[rows] = table[scan[rows]]
        return out


# ---- submissions ---------------------------------------------------------------------------------------------------
Submission = namedtuple("Submission", "name kernel args orders")   # args: keyword arguments of ref.layout / grt.generate_primary_rays


def tile_submissions(width, height):
    """Band tiles (8 scan lines: the scheduler walks them in patches) and 3-line tiles (it does not) over 2 and 3 ranks, every rank."""
    out = []
    for rows, orders in ((8, [(8, 8), (16, 4), None]), (3, [(0, 0), None])):
        tile_pixels = rows * width
        if tile_pixels > width * height:
            continue
        for ranks in (2, 3):
            for rank in range(ranks):
                tiles = (tile_pixels, rank, ranks)
                count = ref.tile_count(width, height, *tiles)
                out.append(Submission("%d-line tiles, rank %d of %d" % (rows, rank, ranks), ref.KERNEL_STREAM, dict(pixel_count=count, tiles=tiles), orders))
    return out


def list_submissions(width, height):
    if width < 9 or height < 9:
        return []
    last_cell = ((width - 1) // ref.NOISE_CELL, (height - 1) // ref.NOISE_CELL)   # clipped by the frame unless both sides are multiples of 16
    cells = ref.cell_list(width, height, [last_cell] + ([(0, 0)] if last_cell != (0, 0) else []))
    frame = width * height
    return [Submission("list: a cell clipped by the frame", ref.KERNEL_STREAM_LIST, dict(pixel_list=cells), [None]),
            Submission("list: one pixel", ref.KERNEL_STREAM_LIST, dict(pixel_list=np.array([frame - 1], np.uint32)), [None]),
            Submission("list: descending", ref.KERNEL_STREAM_LIST, dict(pixel_list=np.arange(frame - 1, -1, -3, dtype=np.uint32)), [None]),
            Submission("list: empty", ref.KERNEL_STREAM_LIST, dict(pixel_list=np.zeros(0, np.uint32)), [None])]


def submissions(width, height):
    frame = width * height
    out = [Submission("whole frame, kernel_generate", ref.KERNEL_GENERATE, dict(pixel_count=frame), [(0, 0)]),
           Submission("whole frame", ref.KERNEL_STREAM, dict(pixel_count=frame), ORDERS),
           Submission("empty range", ref.KERNEL_STREAM, dict(pixel_offset=min(3, frame), pixel_count=0), [(0, 0), None]),
           Submission("empty range, kernel_generate", ref.KERNEL_GENERATE, dict(pixel_offset=0, pixel_count=0), [(0, 0)])]
    if 3 * width + 8 <= frame:
        for kernel in (ref.KERNEL_GENERATE, ref.KERNEL_STREAM):
            out.append(Submission("range, kernel %d" % kernel, kernel, dict(pixel_offset=width + 3, pixel_count=2 * width + 5), [(0, 0), None]))
    return out + tile_submissions(width, height) + list_submissions(width, height)


def submission_set(width, height, sub):
    """The scan-line indices the submission must cover, whatever the order."""
    return np.sort(ref.submission_pixels(width, height, **sub.args))
