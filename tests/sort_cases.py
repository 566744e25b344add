"""Scene, settings and trace queues of the sort-launch tests (test_sort.py on the CPU, test_gpu_sort.py on the device).

The scene is scenes.write_scene_with_everything (textured plastic floor, two emitters of which one is a rotated and scaled file mesh, a
rough dielectric holding a scattering medium, a conductor) plus a diffuse sphere, loaded through the host library with one BLAS per
mesh. The media table is replaced (rt_upload_media on the device, the view's array for the oracle) by six media: the scene's own, a
purely absorbing one (sigma_s = 0), one whose sigma_t differs by three orders of magnitude between the channels, and three that differ
from the first in g alone (0, +0.999, -0.999). Skies: an HDR one (sky_sampling_reference.sun_sky, 64 x 32) and a 1 x 1 one.

Hits are synthetic: (instance, triangle, t, u, v) come from the scene's tables (an emitter's triangles from the light tables); no
traversal runs. Only states the renderer can reach are built: bounce-0 entries carry no flags; ALLOW_NEE comes with a valid last_pdf
(what an entry without the flag holds there is NaN: nothing may read it); fields the kernel must not read hold garbage."""
import ctypes

import numpy as np

import sky_sampling_reference as sky_ref
import sort_reference as ref
from sort_reference import Entries, Launch, LIGHT, DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR, INVALID

NUM_BOUNCES = 8
MAX_BOUNCES = 128            # RT_MAX_BOUNCES
WIDTH = HEIGHT = 128
GRID = 512 * 1024            # threads of the sort launch: 512 workgroups of 1024 (rt_launch_sort, rt_launch_sort_stream)
BLOCK = 1024
SENTINEL = 0xFFC0DE42        # as a float a NaN, as an int negative, as a pixel word beyond every frame
SUBMISSIONS = 128            # RT_STREAM_SUBMISSIONS
MISS, EMITTER = "miss", "emitter"
CLASSES = (MISS, EMITTER, DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR)


def media_table(scene_medium):
    m = np.zeros((6, 8), np.float32)
    m[0] = scene_medium
    m[1] = [0.3, 0.6, 1.2, 0.0, 0.0, 0.0, 0.0, 0.0]
    m[2] = [0.01, 0.5, 5.0, 0.9, 0.05, 3.0, 40.0, 0.0]
    for k, g in ((3, 0.0), (4, 0.999), (5, -0.999)):
        m[k] = scene_medium; m[k, 3] = g
    return m


def one_by_one_sky():
    return np.array([[[0.7, 0.8, 1.1, 1.0]]], np.float32)


class Setup:
    """Settings of a group of launches: rt_gpu_config fields that differ from the default, the sky, the sky's share of the light
    samples (rt_set_sky_sampling), the pixel of the pixel query, whether the light tables are there."""

    def __init__(self, name, config=None, sky="hdr", sky_sampling=0.0, pixel_query=-1, lights=True, black_emitter=False):
        self.name, self.config, self.sky, self.sky_sampling, self.pixel_query, self.lights = name, dict(config or {}), sky, sky_sampling, pixel_query, lights
        self.black_emitter = black_emitter   # the second emitter's material emits nothing (its row of the materials table is zeroed)


QUERY_PIXEL = 5 + 7 * WIDTH
SETUPS = [
    Setup("default", pixel_query=QUERY_PIXEL),
    Setup("nee_off", {"enable_next_event_estimation": 0}),
    Setup("mis_off", {"enable_multiple_importance_sampling": 0}),
    Setup("roulette_off", {"enable_russian_roulette": 0}),
    Setup("mipmapping_off", {"enable_mipmapping": 0}),
    Setup("svgf_on", {"enable_svgf": 1}, pixel_query=QUERY_PIXEL),
    Setup("sky_1x1", sky="one"),
    Setup("sky_share_0.25", sky_sampling=0.25),
    Setup("sky_share_0.5", sky_sampling=0.5),
    Setup("sky_share_1", sky_sampling=1.0),
    Setup("sky_share_0.5_mis_off", {"enable_multiple_importance_sampling": 0}, sky_sampling=0.5),
    Setup("sky_share_0.5_no_emitters", sky_sampling=0.5, lights=False),
    Setup("sky_share_0.5_1x1", sky="one", sky_sampling=0.5),
    Setup("black_emitter", black_emitter=True, pixel_query=QUERY_PIXEL),
    Setup("black_emitter_svgf", {"enable_svgf": 1}, black_emitter=True),
    Setup("bounces_128", {"num_bounces": MAX_BOUNCES}, pixel_query=QUERY_PIXEL),   # the longest path the queues' counters allow
]
SETUP = {s.name: s for s in SETUPS}


class World:
    """The loaded scene: host pathtracer (device < 0: host only), oracle view, and the tables the queues are drawn from."""

    # what a test module with another frame or more shapes overrides (material_cases.py)
    FRAME = (WIDTH, HEIGHT)
    EXTRA_SHAPES = ('<shape type="sphere"><float name="radius" value="0.3"/><transform name="toWorld"><translate x="1.2" y="0.3" z="1.5"/></transform>'
                    '<bsdf type="diffuse"><rgb name="reflectance" value="0.5, 0.7, 0.3"/></bsdf></shape>')

    def __init__(self, grt, oracle, directory, device):
        from scenes import write_scene_with_everything
        from test_loaders import _png_bytes
        path = write_scene_with_everything(directory, _png_bytes)
        xml = open(path).read().replace("</scene>", self.EXTRA_SHAPES + "</scene>")
        open(path, "w").write(xml)
        self.prepare(directory)
        self.grt, self.oracle, self.device = grt, oracle, device
        settings = dict(merge_static=0, num_bounces=NUM_BOUNCES)
        grt.config_reset(); grt.config_set(**settings)
        self.scene = grt.Scene(path)
        grt.config_set(**settings)
        self.pt = grt.Pathtracer(self.scene, self.FRAME[0], self.FRAME[1], device=device)
        self.pt.update()
        self.view = oracle.SceneView(self.pt)
        self.ctx = self.pt.ctx if device >= 0 else None
        self.lib = grt.device_lib() if device >= 0 else None
        s, k = self.view.scene, self.view.keep
        self.pitch, self.frame_pixels = s.screen_pitch, s.screen_pitch * s.screen_height
        assert self.pitch == self.FRAME[0]
        self.base_config = oracle.GPUConfig()
        ctypes.memmove(ctypes.byref(self.base_config), ctypes.byref(s.config), ctypes.sizeof(s.config))
        assert self.base_config.num_bounces == NUM_BOUNCES
        self.media = media_table(np.asarray(k["media"], np.float32).reshape(-1, 8)[0])
        self.skies = {"hdr": (np.ascontiguousarray(sky_ref.sun_sky(64, 32, sun=(40, 9), sun_value=300.0)), 1.0), "one": (one_by_one_sky(), 1.0)}
        # SVGF matrices of the test's own (row-major; w stays positive over the scene), the previous frame's a little different
        self.view_projection = np.array([1.2, 0.0, 0.1, 0.3, 0.0, 1.5, 0.2, -0.4, 0.05, 0.1, -1.01, 5.8, 0.02, 0.03, -1.0, 9.0], np.float32)
        self.view_projection_prev = (self.view_projection * np.float32(1.03125) + np.float32(0.015625)).astype(np.float32)
        self.light_tables = tuple(np.array(k[n]) for n in ("light_triangle_indices", "light_triangle_cumulative_probability", "light_mesh_cumulative_probability",
                                                            "light_mesh_triangle_span", "light_mesh_transform_indices")) + (float(s.lights_total_weight),)
        types = np.asarray(k["material_types"], np.uint8)[np.asarray(k["mesh_material_ids"], np.int32)]
        self.instances = {t: np.nonzero(types == t)[0].astype(np.int32) for t in (LIGHT, DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR)}
        for t, meshes in self.instances.items():
            assert meshes.size > 0, "the scene has no instance of material type %d" % t
        assert self.instances[LIGHT].size == 2
        spans = self.light_tables[3].reshape(-1, 2)
        self.light_triangles = {int(mesh): self.light_tables[0][first:last + 1] for mesh, (first, last) in zip(self.light_tables[4], spans)}
        self.triangle_count = np.asarray(k["triangles"]).size // 24
        self.mesh_count = types.size
        self.material_types = np.array(k["material_types"], np.uint8)
        self.materials = np.array(k["materials"], np.float32).reshape(-1, 8)
        self.black_materials = self.materials.copy()
        self.black_instance = int(self.instances[LIGHT][1])
        self.black_materials[np.asarray(k["mesh_material_ids"], np.int32)[self.black_instance], :3] = 0.0
        # previous transforms that differ from the current ones (a still scene stages them equal): the g-buffers of an emitter seen at bounce 0 must read the right table
        prev = np.array(k["mesh_transforms"], np.float32)
        prev.reshape(-1, 12)[:, 3] += np.float32(0.125); prev.reshape(-1, 12)[:, 5] *= np.float32(1.0625)
        k["mesh_transforms_prev"] = prev; s.mesh_transforms_prev = prev.ctypes.data
        assert not np.array_equal(prev.reshape(-1, 12)[self.instances[LIGHT]], np.asarray(k["mesh_transforms"], np.float32).reshape(-1, 12)[self.instances[LIGHT]])
        if self.ctx is not None:
            status = self.lib.rt_upload_instances(self.ctx, k["mesh_bvh_root_indices"].ctypes.data, k["mesh_material_ids"].ctypes.data, k["mesh_transforms"].ctypes.data,
                                                  k["mesh_transforms_inv"].ctypes.data, prev.ctypes.data, self.mesh_count)
            assert status == 0, self.lib.rt_last_error(self.ctx)
        self.applied = None

    def prepare(self, directory):
        """Hook: the scene's files are written, nothing is loaded yet."""

    def close(self):
        self.pt.close(); self.scene.close(); self.grt.config_reset()

    def effective_share(self, setup, config):
        """RtParams::sky_nee_share as a render settles it (rt_scene.hip: sky_sampling_prepare)."""
        if setup.sky_sampling <= 0 or not config.enable_next_event_estimation:
            return 0.0
        return setup.sky_sampling if setup.lights else 1.0

    def apply(self, setup):
        """Puts a setup in force: in the oracle's view and, with a device, in the context (through the C ABI's own setters).
        Returns the float64 reference's tables for it."""
        v, s, k = self.view, self.view.scene, self.view.keep
        cfg = self.oracle.GPUConfig()
        ctypes.memmove(ctypes.byref(cfg), ctypes.byref(self.base_config), ctypes.sizeof(cfg))
        for field, value in setup.config.items():
            assert hasattr(cfg, field)
            setattr(cfg, field, value)
        ctypes.memmove(ctypes.byref(s.config), ctypes.byref(cfg), ctypes.sizeof(cfg))
        s.config.aov_mask |= 1
        sky, scale = self.skies[setup.sky]
        k["sky"] = sky; s.sky = sky.ctypes.data; s.sky_height, s.sky_width = sky.shape[:2]; s.sky_scale = scale
        k["media"] = self.media; s.media = self.media.ctypes.data; s.medium_count = self.media.shape[0]
        s.lights_total_weight = self.light_tables[5] if setup.lights else 0.0
        materials = self.black_materials if setup.black_emitter else self.materials
        k["materials"] = materials; s.materials = materials.ctypes.data
        for i in range(16):
            s.view_projection[i] = float(self.view_projection[i]); s.view_projection_prev[i] = float(self.view_projection_prev[i])
        if self.ctx is not None:
            lib, ctx, grt = self.lib, self.ctx, self.grt
            def ok(status):
                assert status == 0, lib.rt_last_error(ctx)
            device_cfg = grt.GPUConfig()
            ctypes.memmove(ctypes.byref(device_cfg), ctypes.byref(cfg), ctypes.sizeof(cfg))
            ok(lib.rt_set_config(ctx, ctypes.byref(device_cfg)))
            ok(lib.rt_set_sky(ctx, sky.ctypes.data, sky.shape[1], sky.shape[0], scale))
            ok(lib.rt_upload_media(ctx, self.media.ctypes.data, self.media.shape[0]))
            ok(lib.rt_upload_materials(ctx, self.material_types.ctypes.data, materials.ctypes.data, self.material_types.size))
            ok(lib.rt_set_svgf_matrices(ctx, self.view_projection.ctypes.data, self.view_projection_prev.ctypes.data))
            ok(lib.rt_set_pixel_query(ctx, setup.pixel_query))
            ok(lib.rt_set_sky_sampling(ctx, setup.sky_sampling))
            if setup.lights:
                ok(grt.upload_lights(ctx, *self.light_tables))
            else:
                ok(lib.rt_upload_lights(ctx, None, None, 0, None, None, None, 0, 0.0))
        self.applied = setup
        return ref.Tables(v, sky_share=self.effective_share(setup, cfg), pixel_query=setup.pixel_query)


# ---- queues -------------------------------------------------------------------------------------------------------------------------

def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def pixels_for(rng, n, frame_pixels, frame_slots, keep=()):
    """n distinct virtual pixels in random order; those of `keep` come first."""
    p = rng.permutation(frame_pixels * frame_slots).astype(np.uint32)
    if len(keep):
        keep = np.asarray(keep, np.uint32)
        p = np.concatenate([keep, p[~np.isin(p, keep)]])
    return p[:n]


def slots_needed(n, frame_pixels):
    return max(1, -(-int(n * 1.05 + 16) // frame_pixels))


def make_entries(world, rng, pixels, bounce, classes=CLASSES, inside_share=0.35, media=(0, 1, 2), first_bounce_inside=False):
    """Random entries, one per pixel, at the given bounce (an int or one per entry)."""
    n = len(pixels)
    bounce = np.broadcast_to(np.asarray(bounce, np.int64), (n,))
    e = Entries(n)
    e.pixel[:] = pixels
    e.origin[:] = rng.uniform(-3, 3, (n, 3)); e.direction[:] = unit_vectors(rng, n)
    cls = rng.integers(0, len(classes), n)
    e.mesh[:] = 0x55aa; e.triangle[:] = INVALID; e.t[:] = np.inf        # a miss: the mesh word is never read
    for c, kind in enumerate(classes):
        m = np.nonzero(cls == c)[0]
        if kind == MISS or m.size == 0:
            continue
        e.t[m] = np.exp(rng.uniform(-3.0, 2.0, m.size))
        u = rng.integers(0, 65536, m.size); v = rng.integers(0, 65536, m.size)
        over = u + v > 65535
        u[over] = 65535 - u[over]; v[over] = 65535 - v[over]
        e.u16[m] = u; e.v16[m] = v
        if kind == EMITTER:
            mesh = rng.choice(world.instances[LIGHT], m.size)
            e.mesh[m] = mesh
            for light in world.instances[LIGHT]:
                mm = m[mesh == light]
                e.triangle[mm] = rng.choice(world.light_triangles[int(light)], mm.size)
        else:
            e.mesh[m] = rng.choice(world.instances[kind], m.size)
            e.triangle[m] = rng.integers(0, world.triangle_count, m.size)
    later = bounce > 0
    e.throughput[:] = np.where(later[:, None], rng.uniform(0.0, 1.5, (n, 3)) * rng.uniform(0.05, 1.0, (n, 1)), np.nan)   # bounce 0 ignores it
    e.allow_nee[:] = later & (rng.random(n) < 0.5)
    e.last_pdf[:] = np.where(e.allow_nee, np.exp(rng.uniform(np.log(2e-4), np.log(50.0), n)), np.nan)
    e.inside[:] = (later | first_bounce_inside) & (rng.random(n) < inside_share)
    e.medium[:] = np.where(e.inside, rng.choice(np.asarray(media), n), 0x7ead)   # outside a medium the word is never read
    e.cone_angle[:] = rng.uniform(1e-4, 1e-2, n); e.cone_width[:] = rng.uniform(1e-4, 1.0, n)
    return e


def per_bounce(world, name, entries, bounce, sample_index=3, seed=0, slots=None):
    return Launch(name, entries, world.frame_pixels, slots or slots_needed(entries.n, world.frame_pixels), bounce=bounce, sample_index=sample_index, seed=seed)


def mixed_launches(world, bounces=(0, 1, 2, NUM_BOUNCES - 2, NUM_BOUNCES - 1), n=6000, keep=()):
    """Every class in random order -- misses, emitters, the four surface types, inside each of the three media -- one launch per bounce."""
    out = []
    for b in bounces:
        rng = np.random.default_rng(100 + b)
        px = pixels_for(rng, n, world.frame_pixels, 1, keep)
        out.append(per_bounce(world, "mixed_bounce%d" % b, make_entries(world, rng, px, b), b, seed=b, slots=1))
    return out


LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, GRID, GRID + 1, 5 * GRID // 2)


def single_submission_table(slots, birth, first_sample=40):
    """Slot table of one submission whose samples fill slots 0 .. slots-1 in order."""
    table = np.zeros((slots, 4), np.int32)
    table[:, 0] = first_sample + np.arange(slots); table[:, 1] = birth; table[:, 2] = 0; table[:, 3] = np.arange(slots)
    births = np.zeros(SUBMISSIONS, np.int32); births[0] = birth
    return table, births


def length_launches(world, lengths=LENGTHS, merged=False):
    out = []
    for n in lengths:
        rng = np.random.default_rng(200 + n % 1000)
        slots = slots_needed(n, world.frame_pixels)
        e = make_entries(world, rng, pixels_for(rng, n, world.frame_pixels, slots), 1)
        if merged:
            table, births = single_submission_table(slots, 6)
            out.append(Launch("length_%d_merged" % n, e, world.frame_pixels, slots, iteration=7, slot_table=table, submission_birth=births, seed=n % 97))
        else:
            out.append(per_bounce(world, "length_%d" % n, e, 1, seed=n % 97, slots=slots))
    return out


def uniform_launches(world):
    """All entries to one material queue; all terminated; exactly one survivor, in the last lane of the last wave of a workgroup; one
    survivor per wave -- each with whole rounds only and with a partial last round."""
    out = []
    for tag, n in (("whole", 2 * BLOCK), ("partial", GRID + BLOCK + 500)):
        rng = np.random.default_rng(300 + n % 1000)
        slots = slots_needed(n, world.frame_pixels)
        px = pixels_for(rng, n, world.frame_pixels, slots)

        def surfaces(kind):
            e = make_entries(world, rng, px, 1, classes=(kind,), inside_share=0.0)
            e.throughput[:] = rng.uniform(1.0, 2.0, (n, 3))       # survival probability saturates at 1: nothing is culled
            return e
        out.append(per_bounce(world, "all_to_conductor_%s" % tag, surfaces(CONDUCTOR), 1, seed=1, slots=slots))
        misses = make_entries(world, rng, px, 1, classes=(MISS,), inside_share=0.0)
        out.append(per_bounce(world, "all_terminated_%s" % tag, misses, 1, seed=2, slots=slots))
        for what, survivors in (("one_survivor_last_lane", np.array([(n // BLOCK) * BLOCK - 1])),
                                ("one_survivor_per_wave", np.arange(17, n, 64))):
            e = misses.take(np.arange(n))
            hit = surfaces(PLASTIC)
            for name, _, _ in Entries.FIELDS:
                getattr(e, name)[survivors] = getattr(hit, name)[survivors]
            out.append(per_bounce(world, "%s_%s" % (what, tag), e, 1, seed=3, slots=slots))
    return out


def emitter_edge_launches(world, tables, bounces=(0, 1, 2)):
    """Emitter hits on the edges of the light pdf, at bounce 0 (seen directly: the g-buffers under SVGF, the pixel query), 1 (DIRECT) and 2 (INDIRECT)."""
    out = []
    for b in bounces:
        rng = np.random.default_rng(400 + b)
        n = 64
        px = pixels_for(rng, n, world.frame_pixels, 2, keep=(QUERY_PIXEL, QUERY_PIXEL + world.frame_pixels))
        e = make_entries(world, rng, px, b, classes=(EMITTER,), inside_share=0.0)
        if b > 0:
            e.allow_nee[:] = True; e.last_pdf[:] = np.exp(rng.uniform(np.log(2e-4), np.log(50.0), n))
            # geometric normal of each entry's emitter, to place directions at chosen angles to it
            tri = tables.triangles[e.triangle].astype(np.float64)
            normal = np.einsum("nij,nj->ni", tables.transforms[e.mesh].astype(np.float64)[:, :, :3], np.cross(tri[:, 3:6], tri[:, 6:9]))
            normal /= np.linalg.norm(normal, axis=1)[:, None]
            tangent = np.cross(normal, np.roll(normal, 1, axis=1) + 0.5); tangent /= np.linalg.norm(tangent, axis=1)[:, None]
            for i, cos in enumerate((0.0, 1e-42, 1e-30, 1e-7, 1e-3)):      # grazing: exactly 0 is not reachable in float32, the dot product decides
                v = tangent[i] * np.sqrt(max(1.0 - cos * cos, 0.0)) + normal[i] * cos
                e.direction[i] = v.astype(np.float32)
            e.t[5] = np.float32(1e-30); e.t[6] = np.float32(1e-12); e.t[7] = np.float32(1e18); e.t[8] = np.float32(3e38)   # t * t underflows, overflows
            e.last_pdf[9] = np.nextafter(np.float32(1e-4), np.float32(1)); e.last_pdf[10] = np.float32(1e-4 * 1.5)
            # light_pdf just below / just above 1e-4: t chosen in float64 for a head-on hit, a few parts in 1e-7 .. 1e-6 to either side
            for i, delta in zip(range(11, 19), (-3e-6, -1e-6, -3e-7, -6e-8, 6e-8, 3e-7, 1e-6, 3e-6)):
                e.direction[i] = (-normal[i]).astype(np.float32)
                emission = tables.materials[tables.material_ids[e.mesh[i]]][:3].astype(np.float64)
                power = 0.299 * emission[0] + 0.587 * emission[1] + 0.114 * emission[2]
                if power > 0:   # (a black emitter has no such distance: its light_pdf is 0 everywhere)
                    e.t[i] = np.float32(np.sqrt(1e-4 * tables.lights_total_weight / power) * (1.0 + delta))
            e.allow_nee[19:24] = False; e.last_pdf[19:24] = np.nan                                   # counted in full
        out.append(per_bounce(world, "emitter_edges_bounce%d" % b, e, b, sample_index=0, seed=b, slots=2))
    return out


def roulette_edge_launches(world, tables):
    """Surface hits whose survival probability sits on the roulette's edges: maximum exactly 1, above 1 (saturate), equal to the entry's
    own random number (r > p is false: it survives), its float neighbours, zero throughput. (With SVGF on the frame's albedo multiplies in:
    the launches' ALBEDO frame holds 0, 0.5 and 1 in turn, see plan.)"""
    rng = np.random.default_rng(500)
    b, sample_index, n = 2, 5, 256
    px = pixels_for(rng, n, world.frame_pixels, 1)
    e = make_entries(world, rng, px, b, classes=(DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR), inside_share=0.0)
    r = tables.view.random(ref.DIM_RUSSIAN_ROULETTE, px, b, sample_index)[:, 0]
    k = np.arange(n) % 8
    top = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5, k == 6], [np.float32(1.0), np.float32(1.75), r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(2)), np.float32(0.0), np.float32(1e-40)],
                    rng.uniform(0, 1, n).astype(np.float32)).astype(np.float32)
    e.throughput[:] = top[:, None] * rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    e.throughput[np.arange(n), rng.integers(0, 3, n)] = top
    return [per_bounce(world, "roulette_edges", e, b, sample_index=sample_index, seed=4, slots=1)]


def medium_edge_launches(world, tables):
    """Entries inside media on the edges of the walk: the free-flight distance equal to t in float32 and its neighbours, a miss inside a
    medium (t infinite), a throughput with one zero channel, with all channels zero (NaN pdf), g = 0 and near +-1, the absorbing medium."""
    rng = np.random.default_rng(600)
    b, sample_index, n = 3, 2, 512
    px = pixels_for(rng, n, world.frame_pixels, 1)
    e = make_entries(world, rng, px, b, classes=(MISS, DIFFUSE, PLASTIC, CONDUCTOR, EMITTER), inside_share=1.0, media=(0, 1, 2, 3, 4, 5))
    k = np.arange(n) % 8
    # the distance the entry draws if its first channel is chosen, as float64 sees it, rounded to float32
    rs = tables.view.random(ref.DIM_BSDF_0, px, b, sample_index).astype(np.float64)
    sigma_t = (tables.media[e.medium][:, 0:3].astype(np.float64) + tables.media[e.medium][:, 4:7].astype(np.float64))
    on_edge = (k < 3) & (e.triangle != INVALID) & (e.medium != 1)
    e.throughput[on_edge] = [1.0, 0.0, 0.0]                                      # the first channel is chosen whatever the random number
    with np.errstate(divide="ignore"):
        d32 = (-np.log(rs[:, 1]) / sigma_t[:, 0]).astype(np.float32)
    edge_t = np.where(k == 0, d32, np.where(k == 1, np.nextafter(d32, np.float32(0)), np.nextafter(d32, np.float32(np.inf))))
    e.t[on_edge] = edge_t[on_edge]
    e.throughput[k == 3, 1] = 0.0                                                # one zero channel
    e.throughput[k == 4] = 0.0                                                   # all zero: the wavelength pdf is 0 / 0
    return [per_bounce(world, "medium_edges", e, b, sample_index=sample_index, seed=5, slots=1)]


def first_bounce_inside_launch(world):
    """The one state the code handles that ray generation never produces: inside a medium at bounce 0 (the cone starts from pixel_spread_angle)."""
    rng = np.random.default_rng(700)
    n = 2000
    px = pixels_for(rng, n, world.frame_pixels, 1)
    e = make_entries(world, rng, px, 0, inside_share=1.0, media=(0, 2, 3), first_bounce_inside=True)
    return [per_bounce(world, "inside_medium_at_bounce0", e, 0, sample_index=1, seed=6, slots=1)]


def sky_direction_launches(world, tables, bounce=1):
    """Misses whose directions lie on the poles, on the seam (x < 0, z = +-0), on the cell borders of the sky table and next to them."""
    rng = np.random.default_rng(800)
    h, w = tables.sky.shape[:2]
    dirs = [[0, 1, 0], [0, -1, 0], [-1, 0, 0.0], [-1, 0, -0.0], [-0.6, 0.8, 0.0], [-0.6, 0.8, -0.0], [1, 0, 0], [0, 0, 1], [0, 0, -1]]
    us = np.arange(w + 1) / w; vs = np.arange(h + 1) / h
    for u in us[::max(1, w // 16)]:
        for v in vs[1:-1:max(1, h // 8)]:
            phi, theta = (u - 0.5) * 2 * np.pi, v * np.pi
            dirs.append([np.sin(theta) * np.cos(phi), np.cos(theta), -np.sin(theta) * np.sin(phi)])
    d = np.array(dirs, np.float64)
    d = np.concatenate([d, d + rng.normal(scale=2e-7, size=d.shape)])
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    d[2] = [-1, 0, 0.0]; d[3] = [-1, 0, -0.0]
    n = d.shape[0] * 2
    px = pixels_for(rng, n, world.frame_pixels, 1)
    e = make_entries(world, rng, px, bounce, classes=(MISS,), inside_share=0.0)
    e.direction[:] = np.concatenate([d, d])
    e.allow_nee[:d.shape[0]] = True; e.last_pdf[:d.shape[0]] = np.exp(rng.uniform(np.log(2e-4), np.log(50.0), d.shape[0]))
    e.allow_nee[d.shape[0]:] = False; e.last_pdf[d.shape[0]:] = np.nan
    return [per_bounce(world, "sky_directions", e, bounce, seed=7, slots=1)]


def merged_launch(world, num_bounces=MAX_BOUNCES, n=9000):
    """One launch of the merged wavefront under a path length of num_bounces: seven sample slots of four submissions at bounces 0, 1, one in the
    middle (7; 2 for a short path) and num_bounces - 1 (the last bounce: every entry of it ends), slots not in submission order, a slot whose
    index_in_submission is not 0 (it must not answer the pixel query), entries of all submissions interleaved within every wave."""
    rng = np.random.default_rng(900)
    iteration, middle = num_bounces + 1, 7 if num_bounces > 8 else 2
    #          sample, birth,                          submission, index_in_submission
    table = [(11,     iteration - 1,                   9,          1),
             (70,     iteration,                       3,          0),
             (10,     iteration - 1,                   9,          0),
             (71,     iteration,                       3,          1),
             (5,      iteration - middle,              127,        0),
             (200,    iteration - (num_bounces - 1),   64,         0),
             (72,     iteration,                       3,          2)]
    table = np.array(table, np.int32)
    births = np.full(SUBMISSIONS, iteration + 1000, np.int32)   # rows of submissions that are not in flight: any bounce they implied would be out of range
    for row in table:
        births[row[2]] = row[1]
    slots = table.shape[0]
    # the query pixel in slot 1 (index 0 of its submission: answers) and in slot 3 (index 1: must not)
    px = pixels_for(rng, n, world.frame_pixels, slots, keep=(QUERY_PIXEL + world.frame_pixels, QUERY_PIXEL + 3 * world.frame_pixels))
    bounce = iteration - table[px // world.frame_pixels, 1]
    e = make_entries(world, rng, px, bounce)
    hit = np.nonzero((e.triangle != INVALID) & ((px == px[0]) | (px == px[1])))[0]
    for i in (0, 1):   # both query entries are surface hits
        if i not in hit:
            src = np.nonzero((e.triangle != INVALID) & (bounce == 0))[0][i]
            for name in ("mesh", "triangle", "t", "u16", "v16"):
                getattr(e, name)[i] = getattr(e, name)[src]
    return [Launch("merged_mixed", e, world.frame_pixels, slots, iteration=iteration, slot_table=table, submission_birth=births, seed=8)]


def plan(world, tables, setup):
    """The launches of a setup."""
    name = setup.name
    if name == "default":
        return (mixed_launches(world, keep=(QUERY_PIXEL,)) + length_launches(world) + length_launches(world, merged=True) + uniform_launches(world)
                + emitter_edge_launches(world, tables) + roulette_edge_launches(world, tables) + medium_edge_launches(world, tables)
                + first_bounce_inside_launch(world) + sky_direction_launches(world, tables))
    if name == "svgf_on":
        out = mixed_launches(world, keep=(QUERY_PIXEL,)) + emitter_edge_launches(world, tables, bounces=(0, 1))
        for value in (0.0, 0.5, 1.0):   # what the roulette reads back from the ALBEDO frame
            launch = roulette_edge_launches(world, tables)[0]
            launch.name += "_albedo%g" % value
            launch.aov[ref.ALBEDO][:, :3] = value
            out.append(launch)
        return out
    if name == "sky_1x1":
        return mixed_launches(world, bounces=(0, 1)) + sky_direction_launches(world, tables)
    if name == "bounces_128":
        return merged_launch(world) + mixed_launches(world, bounces=(MAX_BOUNCES - 2, MAX_BOUNCES - 1))
    if name.startswith("black_emitter"):
        return emitter_edge_launches(world, tables) + mixed_launches(world, bounces=(0, 1, 2))
    if name.startswith("sky_share"):
        out = mixed_launches(world, bounces=(0, 1, 2)) + sky_direction_launches(world, tables) + emitter_edge_launches(world, tables, bounces=(1, 2))
        if name == "sky_share_0.5":   # the merged wavefront's _sky instance
            out += merged_launch(world, NUM_BOUNCES) + length_launches(world, lengths=(1025, GRID + 1), merged=True)
        return out
    return mixed_launches(world) + emitter_edge_launches(world, tables, bounces=(1, 2))
