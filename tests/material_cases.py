"""Scene, settings and material queues of the material-launch tests (test_material.py on the CPU, test_gpu_material.py on the device).

The world is sort_cases.World -- textured rough-plastic floor under a scale of 5, two emitters of which one is a rotated, scaled and
translated file mesh, a rough dielectric sphere holding a medium, a conductor sphere, a diffuse sphere -- in a 64 x 64 frame, plus a
textured diffuse quad under a rotation, a scale of 0.7 and a translation, and an untextured rough-plastic sphere (so that both textured
material types also have an instance whose albedo is a constant). Every instance's previous transform differs from its
current one (World stages them so), so screen_position_prev is not the current position. Spheres interpolate their normals: the
shading normal is not the geometric one, and the curvature is not zero.

Hits are synthetic, as in sort_cases: (instance, triangle, t, u, v) from the scene's tables, directions uniform over the sphere (so
about half the entries arrive at the back face). Entries are built in the state the sort leaves them: at bounce 0 the throughput and
cone words hold the sentinel, outside a medium the medium word holds it, the padding holds it.

The variants of the launch (test_gpu_material_variants.py on the device, their reference-only checks in test_material.py) have setups of their
own (SKY_SETUPS: the sky takes a share of the light samples), a world of their own (VariantWorld, at the end of this file) and their launches
(sky_launches, sky_length_launches, sky_lights_launch, map_launches, sky_map_launches). PLAIN_SETUPS are the setups the oracle can be asked about."""
import ctypes

import numpy as np

import sort_cases
from sort_cases import SENTINEL, NUM_BOUNCES, SUBMISSIONS, pixels_for, slots_needed, unit_vectors, single_submission_table   # noqa: F401 (the tests' vocabulary)
from sort_reference import Entries, DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR

WIDTH = HEIGHT = 64
BLOCK = 256                   # RT_SHADE_BLOCK
GRID, STREAM_GRID = 2048, 8192   # workgroups of rt_launch_material and rt_launch_material_stream
SLOT_NAMES = ("diffuse", "plastic", "dielectric", "conductor")
SLOT_TYPES = (DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR)
MATERIAL_WORDS, TRACE_WORDS, SHADOW_WORDS = 16, 20, 11
AOV_MASK = 1 | (1 << 3) | (1 << 4) | (1 << 5)    # RADIANCE (always on), ALBEDO, NORMAL, POSITION
ROUGHNESS_WORD = {PLASTIC: 4, DIELECTRIC: 2, CONDUCTOR: 3}   # of the 8-float material record (bsdf_checks.roughness_of)
MAX_VALUE_ENTRIES = 4096
ALBEDO_FLOOR = 60.0 / 255.0   # every texel of the world's texture is 64 / 255 or more; a mip level is an average, rounded to 8 bits at most once per level


class Setup(sort_cases.Setup):
    """sort_cases.Setup with the three frames of the launch enabled, and
    `smooth`: the dielectric and the conductor get a roughness below the cutoff, so that their BSDFs do not allow next-event estimation
    (no shadow ray, no ALLOW_NEE, no last_pdf);
    `bc1`: the device holds one more texture, of BC1 blocks decoded per fetch (rt_set_texture_expansion(ctx, 0)), which no material names:
    the launchers then take the diffuse and plastic instances that can decode (not the _texels ones) for the scene's own RGBA8 texture."""

    def __init__(self, name, config=None, smooth=False, bc1=False, aov_mask=AOV_MASK, **rest):
        config = dict(config or {}); config.setdefault("aov_mask", aov_mask)
        super().__init__(name, config, **rest)
        self.smooth, self.bc1 = smooth, bc1


SETUPS = [
    Setup("default"),
    Setup("nee_off", {"enable_next_event_estimation": 0}),
    Setup("mis_off", {"enable_multiple_importance_sampling": 0}),
    Setup("mipmapping_off", {"enable_mipmapping": 0}),
    Setup("svgf_on", {"enable_svgf": 1}),
    Setup("no_lights", lights=False),
    Setup("smooth", smooth=True),
    Setup("frames_off", aov_mask=1),
    Setup("bc1_present", bc1=True),
    # the _sky instances (test_gpu_material_variants.py): the sky takes a share of the light samples
    Setup("sky_share_0.25", sky_sampling=0.25),
    Setup("sky_share_0.5", sky_sampling=0.5),
    Setup("sky_share_1", sky_sampling=1.0),
    Setup("sky_share_0.5_mis_off", {"enable_multiple_importance_sampling": 0}, sky_sampling=0.5),
    Setup("sky_share_0.5_no_emitters", sky_sampling=0.5, lights=False),
    Setup("sky_share_0.5_1x1", sky="one", sky_sampling=0.5),
    Setup("sky_share_0.5_svgf", {"enable_svgf": 1}, sky_sampling=0.5),
    Setup("sky_share_0.5_bc1", bc1=True, sky_sampling=0.5),
]
SETUP = {s.name: s for s in SETUPS}
SKY_SETUPS = tuple(s for s in SETUPS if s.sky_sampling > 0)
PLAIN_SETUPS = tuple(s for s in SETUPS if not s.sky_sampling > 0)   # what the oracle, which samples no sky, can be asked about


class World(sort_cases.World):
    FRAME = (WIDTH, HEIGHT)
    EXTRA_SHAPES = sort_cases.World.EXTRA_SHAPES + (
        '<shape type="obj"><string name="filename" value="quad.obj"/><transform name="toWorld"><scale value="0.7"/><rotate y="1" angle="30"/><rotate x="1" angle="-60"/>'
        '<translate x="2.2" y="1.0" z="-1.0"/></transform><bsdf type="diffuse"><texture type="bitmap" name="reflectance"><string name="filename" value="t.png"/></texture></bsdf></shape>'
        '<shape type="sphere"><float name="radius" value="0.35"/><transform name="toWorld"><translate x="-0.4" y="0.35" z="2.2"/></transform>'
        '<bsdf type="roughplastic"><rgb name="diffuseReflectance" value="0.3, 0.55, 0.8"/><float name="alpha" value="0.16"/></bsdf></shape>')

    def prepare(self, directory):
        """The texture both textured materials use: random texels of 64 / 255 or more in every channel (material_checks.TEXTURED_RELATIVE needs the floor)."""
        from test_loaders import _png_bytes
        (directory / "t.png").write_bytes(_png_bytes(np.random.default_rng(3).integers(64, 256, (32, 32, 3)), 2, 8))

    def roughness_of_instance(self, tables):
        """Linear roughness per instance under the applied setup (1 for diffuse, whose sample is the cosine lobe)."""
        r = np.ones(tables.materials.shape[0])
        for kind, word in ROUGHNESS_WORD.items():
            r[tables.material_types == kind] = tables.materials[tables.material_types == kind, word]
        return r[tables.material_ids]

    def __init__(self, grt, oracle, directory, device):
        super().__init__(grt, oracle, directory, device)
        k = self.view.keep
        ids = np.asarray(k["mesh_material_ids"], np.int32)
        textured = self.materials[:, 3].view(np.int32) >= 0     # word 3 of a diffuse or plastic record: its texture
        for kind in (DIFFUSE, PLASTIC):
            mine = self.material_types[ids[self.instances[kind]]] == kind
            assert (mine & textured[ids[self.instances[kind]]]).any(), "no textured material of type %d" % kind
        for kind in (DIFFUSE, PLASTIC):
            assert (~textured[ids[self.instances[kind]]]).any(), "no untextured material of type %d" % kind
        self.textured_instance = textured[ids] & np.isin(self.material_types[ids], (DIFFUSE, PLASTIC))
        assert (self.materials[textured & np.isin(self.material_types, (DIFFUSE, PLASTIC)), :3] == 1.0).all(), "a textured material scales its texture"
        rows = np.asarray(k["mesh_transforms"], np.float32).reshape(-1, 3, 4)
        scale = np.linalg.norm(rows[:, 0, :3].astype(np.float64), axis=1)
        assert (np.abs(scale - 1.0) > 0.1).sum() >= 3, "fewer than three instances under a non-unit scale"
        # the Kulla-Conty tables of the dielectric and the conductor: the device's own, or the oracle's integration at 1500 samples a cell (as
        # test_bsdf.py; both sides of a comparison read the same numbers, but how ill-conditioned 1 - E is depends on them: the bounds measured
        # on the CPU have to see tables like the device's)
        if device >= 0:
            luts = grt.read_luts(self.ctx)
        else:
            v = self.view
            luts = [v.integrate_dielectric_cells(True, 0, 4096, 1500), v.integrate_dielectric_cells(False, 0, 4096, 1500)]
            luts += [oracle.average_dielectric(luts[0]), oracle.average_dielectric(luts[1])]
            luts.append(v.integrate_conductor_cells(0, 1024, 1500))
            luts.append(oracle.average_conductor(luts[4]))
        k["luts"] = [np.ascontiguousarray(l, dtype=np.float32) for l in luts]
        s = self.view.scene
        (s.lut_dielectric_directional_albedo_enter, s.lut_dielectric_directional_albedo_leave, s.lut_dielectric_albedo_enter,
         s.lut_dielectric_albedo_leave, s.lut_conductor_directional_albedo, s.lut_conductor_albedo) = [l.ctypes.data for l in k["luts"]]
        import bsdf_reference
        self.bsdf_tables = bsdf_reference.Tables(k["luts"])
        self.textures_compressed = False   # the scene's one texture is decoded to texels at upload: the launchers take the _texels instances of the diffuse and plastic kernels
        self.rough_materials = self.materials
        self.smooth_materials = self.materials.copy()
        for kind in (DIELECTRIC, CONDUCTOR):
            self.smooth_materials[self.material_types == kind, ROUGHNESS_WORD[kind]] = 0.02

    def apply(self, setup):
        self.materials = self.smooth_materials if getattr(setup, "smooth", False) else self.rough_materials
        try:
            tables = super().apply(setup)
        finally:
            self.materials = self.rough_materials
        if self.ctx is not None and bool(getattr(setup, "bc1", False)) != self.textures_compressed:
            self.upload_textures(bool(setup.bc1))
        return tables

    def upload_textures(self, with_bc1):
        """The scene's textures again (rt_upload_textures), with or without a BC1 texture behind them that is decoded per fetch."""
        from texture_cases import bc1_texture
        from test_gpu_texture_unit import TextureDesc   # (the texture tests' mirror of rt_texture_desc: one copy)
        scene_textures = self.pt.textures()
        extra = bc1_texture(8, 8, 7) if with_bc1 else None
        descs = (TextureDesc * (len(scene_textures) + 1))()
        for i, (texels, w, h, levels) in enumerate(scene_textures):
            descs[i].texels, descs[i].width, descs[i].height, descs[i].mip_levels, descs[i].format = texels.ctypes.data, w, h, levels, 0
            descs[i].lod_width, descs[i].lod_height = self.pt.texture_lod_size(i)
        if extra is not None:
            d = descs[len(scene_textures)]
            d.texels, d.width, d.height, d.mip_levels, d.format = extra.data.ctypes.data, extra.width, extra.height, extra.mip_levels, extra.format
        lib = self.lib
        lib.rt_set_texture_expansion.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.rt_upload_textures.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        assert lib.rt_set_texture_expansion(self.ctx, 0 if with_bc1 else 1) == 0, lib.rt_last_error(self.ctx)
        assert lib.rt_upload_textures(self.ctx, descs, len(scene_textures) + (1 if with_bc1 else 0)) == 0, lib.rt_last_error(self.ctx)
        self.textures_compressed = with_bc1


class Launch:
    """One material launch: the queue of slot `slot`, how its entries' bounce and sample are found (per-bounce form: bounce,
    sample_index; merged form: iteration, slot_table (S, 4) int32, submission_birth int32[128]), the frames' size."""

    def __init__(self, name, slot, entries, frame_pixels, frame_slots, bounce=None, sample_index=0, iteration=None, slot_table=None, submission_birth=None, first_throughput=False):
        self.name, self.slot, self.entries, self.frame_pixels, self.frame_slots = name, int(slot), entries, int(frame_pixels), int(frame_slots)
        self.first_throughput = bool(first_throughput)   # the queue holds bounce 0's throughput too, as the ..._fog sort instance stores it
        self.bounce, self.sample_index, self.iteration = bounce, sample_index, iteration
        self.slot_table = None if slot_table is None else np.ascontiguousarray(slot_table, np.int32).reshape(-1, 4)
        self.submission_birth = None if submission_birth is None else np.ascontiguousarray(submission_birth, np.int32)
        self.merged = iteration is not None

    def paths(self):
        """Per entry: sample slot, real pixel, bounce, sample index (the RNG's), submission."""
        e = self.entries
        slot = (e.pixel // self.frame_pixels).astype(np.int64)
        real = (e.pixel % self.frame_pixels).astype(np.uint32)
        if self.merged:
            row = self.slot_table[slot]
            return slot, real, self.iteration - row[:, 1].astype(np.int64), row[:, 0].astype(np.int64), row[:, 2].astype(np.int64)
        zero = np.zeros(e.n, np.int64)
        return slot, real, zero + self.bounce, self.sample_index + slot, zero

    def sub(self, index, name=None):
        """The launch on the entries `index` alone."""
        return Launch(name or self.name + "_sample", self.slot, self.entries.take(index), self.frame_pixels, self.frame_slots, bounce=self.bounce, sample_index=self.sample_index,
                      iteration=self.iteration, slot_table=self.slot_table, submission_birth=self.submission_birth, first_throughput=self.first_throughput)

    def pack(self, garbage=None):
        """(N, 16) uint32 records as the sort writes them; `garbage` (a float32) replaces the sentinel in the words the sort leaves
        unwritten at bounce 0 (throughput, cone) -- the launch must not read them."""
        e = self.entries
        bounce = self.paths()[2]
        r = np.full((e.n, MATERIAL_WORDS), SENTINEL, np.uint32)
        r[:, 0:3] = e.direction.view(np.uint32)
        r[:, 3] = e.mesh.view(np.uint32); r[:, 4] = e.triangle.view(np.uint32); r[:, 5] = e.t.view(np.uint32); r[:, 6] = (e.u16 & 0xffff) | (e.v16 << 16)
        r[:, 7] = e.pixel | (e.inside.astype(np.uint32) << 30)
        later = bounce > 0
        carried = later | self.first_throughput
        r[carried, 8:11] = e.throughput.view(np.uint32)[carried]
        r[e.inside, 11] = e.medium.view(np.uint32)[e.inside]
        r[later, 12] = e.cone_angle.view(np.uint32)[later]; r[later, 13] = e.cone_width.view(np.uint32)[later]
        if garbage is not None:
            first = ~later
            r[first, 8:11] = np.float32(garbage).view(np.uint32); r[first, 12:14] = np.float32(garbage).view(np.uint32)
        return r


def make_entries(world, rng, pixels, slot, bounce, inside_share=None):
    """Random hits on the instances of slot `slot`'s material type, one per pixel, at the given bounce (an int or one per entry).
    Inside a medium: a third of the dielectric's entries beyond bounce 0, a tenth of the others' (the medium passes through them)."""
    e = sort_cases.make_entries(world, rng, pixels, bounce, classes=(SLOT_TYPES[slot],),
                                inside_share=(0.33 if slot == 2 else 0.1) if inside_share is None else inside_share)
    e.allow_nee[:] = False   # (a material entry carries no such flag)
    return e


def per_bounce(world, name, slot, n, bounce, seed, sample_index=3, slots=None, **kw):
    rng = np.random.default_rng(seed)
    slots = slots or slots_needed(n, world.frame_pixels)
    e = make_entries(world, rng, pixels_for(rng, n, world.frame_pixels, slots), slot, bounce, **kw)
    return Launch("%s_%s_bounce%d_%d" % (name, SLOT_NAMES[slot], bounce, n), slot, e, world.frame_pixels, slots, bounce=bounce, sample_index=sample_index)


def merged(world, name, slot, n, seed, num_bounces=NUM_BOUNCES, **kw):
    """One launch of the merged wavefront: five sample slots of three submissions at bounces 0, 1 and num_bounces - 1, slots not in
    submission order, entries of all submissions interleaved."""
    rng = np.random.default_rng(seed)
    iteration = num_bounces + 3
    #          sample, birth,                        submission, index_in_submission
    table = np.array([(11, iteration - 1,                 9,   1),
                      (70, iteration,                     3,   0),
                      (10, iteration - 1,                 9,   0),
                      (200, iteration - (num_bounces - 1), 64, 0),
                      (71, iteration,                     3,   1)], np.int32)
    births = np.full(SUBMISSIONS, iteration + 1000, np.int32)
    for row in table:
        births[row[2]] = row[1]
    slots = table.shape[0]
    assert n <= slots * world.frame_pixels
    px = pixels_for(rng, n, world.frame_pixels, slots)
    bounce = iteration - table[px // world.frame_pixels, 1]
    e = make_entries(world, rng, px, slot, bounce, **kw)
    return Launch("%s_%s_merged_%d" % (name, SLOT_NAMES[slot], n), slot, e, world.frame_pixels, slots, iteration=iteration, slot_table=table, submission_birth=births)


LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 4 * 256 + 3)
SECOND_ROUND = GRID * BLOCK + 1          # per-bounce: one entry in a second grid-stride round
BOUNCES = (0, 1, NUM_BOUNCES - 1)


def value_launches(world):
    """The plain and the merged instance of all four slots: per-bounce launches at bounce 0, 1 and the last, one merged launch."""
    out = []
    for slot in range(4):
        for b in BOUNCES:
            out.append(per_bounce(world, "mixed", slot, 3000, b, seed=1000 + 10 * slot + b))
        out.append(merged(world, "mixed", slot, 4000, seed=1100 + slot))
    return out


def length_launches(world):
    """Queue lengths around a wave and a workgroup, per-bounce (bounce 1) and merged, over the slots in turn."""
    out = []
    for k, n in enumerate(LENGTHS):
        out.append(per_bounce(world, "length", k % 4, n, 1, seed=1200 + k, slots=1))
        out.append(merged(world, "length", (k + 1) % 4, n, seed=1300 + k))
    return out


def small_launches(world):
    """One small launch per slot and form, for the setups that change one setting."""
    out = []
    for slot in range(4):
        out.append(per_bounce(world, "small", slot, 700, 0, seed=1400 + slot))
        out.append(per_bounce(world, "small", slot, 700, 2, seed=1410 + slot))
    out.append(merged(world, "small", 0, 1500, seed=1420))
    out.append(merged(world, "small", 2, 1500, seed=1421))
    return out


def second_round_launch(world):
    """2048 x 256 + 1 diffuse entries at bounce 1: the last entry is alone in the second grid-stride round."""
    return per_bounce(world, "second_round", 0, SECOND_ROUND, 1, seed=1500)


def plan(world, setup, tables=None):
    if setup.name == "default":
        return value_launches(world) + length_launches(world) + (threshold_launches(world, tables) if tables is not None else [])
    if setup.name == "svgf_on" and tables is not None:
        return small_launches(world) + threshold_launches(world, tables)
    return small_launches(world)


def from_records(world, name, slot, records, bounce, sample_index):
    """A per-bounce launch on (N, 16) material records of a sort launch (rt_sort_rays / oracle_sort), one sample slot."""
    r = np.ascontiguousarray(records, np.uint32).reshape(-1, MATERIAL_WORDS)
    e = Entries(r.shape[0])
    e.direction[:] = r[:, 0:3].view(np.float32)
    e.mesh[:] = r[:, 3].view(np.int32); e.triangle[:] = r[:, 4].view(np.int32); e.t[:] = r[:, 5].view(np.float32)
    e.u16[:] = r[:, 6] & 0xffff; e.v16[:] = r[:, 6] >> 16
    e.pixel[:] = r[:, 7] & 0x3fffffff; e.inside[:] = (r[:, 7] >> 30) & 1
    e.throughput[:] = r[:, 8:11].view(np.float32); e.medium[:] = r[:, 11].view(np.int32)
    e.cone_angle[:] = r[:, 12].view(np.float32); e.cone_width[:] = r[:, 13].view(np.float32)
    return Launch("%s_%s_bounce%d_%d" % (name, SLOT_NAMES[slot], bounce, e.n), slot, e, world.frame_pixels, 1, bounce=bounce, sample_index=sample_index)


def threshold_launches(world, tables):
    """Launches that sit on the set-up's thresholds on purpose, one per slot at bounce 0 (the frames) and at bounce 1, 96 entries each, in
    groups of eight: a direction in the geometric plane (dot(direction, geometric normal) = 0 as float64 sees it, rounded to float32) and
    its float neighbours in each component; a direction perpendicular to the shading normal (omega_i.z = 0) and its neighbours; a
    head-on hit of the back face; a hit at t = 0; a hit on the edge u + v = 1; the rest random. Exempt from the cap on non-robust
    entries; an entry next to a threshold may go either way, every other entry takes float64's."""
    import material_reference as ref
    out = []
    for slot in range(4):
        for bounce in (0, 1):
            launch = per_bounce(world, "threshold", slot, 96, bounce, seed=2000 + 10 * slot + bounce, slots=1, inside_share=0.0)
            e = launch.entries
            r = ref.evaluate(world, tables, launch, world.bsdf_tables)
            k = np.arange(e.n) % 8
            for group, axis in ((0, r.geometric_normal), (1, r.normal)):
                for i in np.nonzero(k == group)[0]:
                    a = axis[i]
                    tangent = np.cross(a, np.roll(a, 1) + 0.5); tangent /= np.linalg.norm(tangent)
                    d = tangent.astype(np.float32)
                    step = (i // 8) % 7   # 0: as rounded; 1..6: one component one float up or down
                    if step:
                        c = (step - 1) // 2
                        d[c] = np.nextafter(d[c], np.float32(2.0 if step % 2 else -2.0))
                    e.direction[i] = d
            back = np.nonzero(k == 2)[0]
            e.direction[back] = r.geometric_normal[back].astype(np.float32)
            e.t[k == 3] = 0.0
            edge = np.nonzero(k == 4)[0]
            e.v16[edge] = 65535 - e.u16[edge]
            out.append(launch)
    return out


THRESHOLD_LAUNCHES = ("threshold_",)


class LightsWorld:
    """A scene of nee_cases.py -- a diffuse floor under many emitters -- as the material tests need it: the light tables fit the shade
    kernels' LDS copy (at most 64 mesh entries and 2048 triangle entries) or go beyond it, which decides where nee_pick_light searches.
    Only the diffuse queue has instances here."""

    def __init__(self, grt, oracle, case, directory, device):
        import nee_cases
        import sort_reference
        self.grt, self.device, self.case = grt, device, case
        self.scene, self.pt = nee_cases.load(grt, case, directory, device, WIDTH, HEIGHT)
        self.view = oracle.SceneView(self.pt)
        self.ctx = self.pt.ctx if device >= 0 else None
        self.lib = grt.device_lib() if device >= 0 else None
        s, k = self.view.scene, self.view.keep
        self.frame_pixels = s.screen_pitch * s.screen_height
        s.config.aov_mask = AOV_MASK
        if self.ctx is not None:
            cfg = grt.GPUConfig()
            ctypes.memmove(ctypes.byref(cfg), ctypes.byref(s.config), ctypes.sizeof(cfg))
            assert self.lib.rt_set_config(self.ctx, ctypes.byref(cfg)) == 0, self.lib.rt_last_error(self.ctx)
        types = np.asarray(k["material_types"], np.uint8)[np.asarray(k["mesh_material_ids"], np.int32)]
        self.instances = {t: np.nonzero(types == t)[0].astype(np.int32) for t in range(5)}
        self.triangle_count = np.asarray(k["triangles"]).size // 24
        self.textured_instance = np.zeros(types.size, bool)
        self.textures_compressed = False
        self.bsdf_tables = None
        self.tables = sort_reference.Tables(self.view)

    def roughness_of_instance(self, tables):
        return np.ones(tables.material_ids.size)

    def close(self):
        self.pt.close(); self.scene.close(); self.grt.config_reset()


def light_table_launches(world):
    """Hits on the floor under the emitters, on the floor's own triangles (by far the largest of the scene; the emitters' ribbons are made
    of slivers, whose geometric normal float32 cannot resolve), at bounce 0 and 2 and in the merged form."""
    out = [per_bounce(world, "lights", 0, 700, 0, seed=2100, inside_share=0.0), per_bounce(world, "lights", 0, 700, 2, seed=2101, inside_share=0.0),
           merged(world, "lights", 0, 1500, seed=2102, num_bounces=3, inside_share=0.0)]
    tri = np.asarray(world.view.keep["triangles"], np.float32).reshape(-1, 24).astype(np.float64)
    e1, e2 = tri[:, 3:6], tri[:, 6:9]
    with np.errstate(all="ignore"):
        area = np.linalg.norm(np.cross(e1, e2), axis=1)
        good = np.nonzero(area > 0.5 * area.max())[0].astype(np.int32)
    assert 2 <= good.size <= 4, good
    for k, launch in enumerate(out):
        launch.entries.triangle[:] = np.random.default_rng(2110 + k).choice(good, launch.entries.n)
    return out


# ---- the variants of the launch: _sky, _nmap, _sky_nmap (test_gpu_material_variants.py; their left-out caps in test_material.py) -------

TILT, FLAT, INWARD = (200, 90, 180), (128, 128, 255), (128, 128, 0)   # the constant normal maps: a strong tilt; the unperturbed normal within 8 bits; t.z = -1 (the view guard fires)
MAP_TEXELS = (FLAT, TILT, INWARD)   # in upload order, behind the scene's own textures (and the BC1 one of a bc1 setup)


class VariantWorld(World):
    """World plus what the variants' launches need and World lacks (its dielectric and conductor are untransformed spheres, every triangle of
    it has texture coordinates with a determinant): a rough dielectric and a rough conductor quad under a rotation and a non-unit scale, whose
    triangles (quad.obj) carry non-degenerate texture coordinates, and a conductor mesh without texture coordinates (uv_det == 0: the mapped
    normal falls back). Mirrored coordinates (uv_det < 0) World has already: the loader stores v as 1 - v, so every quad.obj triangle has
    them, next to the spheres' uv_det > 0. Hits are synthetic, so any instance goes with any triangle: a launch picks its triangles by
    determinant (triangles_where). Three constant RGBA8 textures lie behind the scene's own: MAP_TEXELS."""
    EXTRA_SHAPES = World.EXTRA_SHAPES + (
        '<shape type="obj"><string name="filename" value="quad.obj"/><transform name="toWorld"><scale value="0.6"/><rotate y="1" angle="40"/><rotate x="1" angle="-50"/>'
        '<translate x="-2.4" y="1.4" z="-1.5"/></transform><bsdf type="roughdielectric"><float name="intIOR" value="1.5"/><float name="alpha" value="0.3"/></bsdf></shape>'
        '<shape type="obj"><string name="filename" value="quad.obj"/><transform name="toWorld"><scale value="1.7"/><rotate z="1" angle="25"/><rotate x="1" angle="70"/>'
        '<translate x="0.5" y="1.8" z="-3.0"/></transform><bsdf type="roughconductor"><string name="material" value="Cu"/><float name="alpha" value="0.2"/></bsdf></shape>'
        '<shape type="obj"><string name="filename" value="bare.obj"/><transform name="toWorld"><scale value="0.8"/><rotate y="1" angle="-35"/>'
        '<translate x="3.0" y="0.6" z="1.0"/></transform><bsdf type="roughconductor"><string name="material" value="Au"/><float name="alpha" value="0.25"/></bsdf></shape>')

    def prepare(self, directory):
        super().prepare(directory)
        (directory / "bare.obj").write_text("v -1 0 -1\nv 1 0 -1\nv 1 0 1\nv -1 0.3 1\nf 1 3 2\nf 1 4 3\n")   # no vt: the loader leaves the coordinates 0; the first triangle is level and faces +y

    def __init__(self, grt, oracle, directory, device):
        super().__init__(grt, oracle, directory, device)
        tri = np.asarray(self.view.keep["triangles"], np.float32).reshape(-1, 24).astype(np.float64)
        self.uv_det = tri[:, 20] * tri[:, 23] - tri[:, 22] * tri[:, 21]
        e1, e2 = tri[:, 3:6], tri[:, 6:9]
        with np.errstate(all="ignore"):
            self.squareness = np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
        assert (self.uv_det > 0).sum() > 100 and (self.uv_det < 0).sum() >= 4 and (self.uv_det == 0).sum() >= 2, "the scene lacks a sign of uv_det"
        ids = np.asarray(self.view.keep["mesh_material_ids"], np.int32)
        rows = np.asarray(self.view.keep["mesh_transforms"], np.float32).reshape(-1, 3, 4).astype(np.float64)
        scale = np.linalg.norm(rows[:, 0, :3], axis=1)
        rotated = np.array([not np.allclose(m[:, :3], np.diag(np.diag(m[:, :3])), atol=1e-6) for m in rows])
        self.transformed_instance = rotated & (np.abs(scale - 1.0) > 0.1)
        for kind in (DIELECTRIC, CONDUCTOR):
            mine = self.instances[kind]
            assert self.transformed_instance[mine].any() and (~self.transformed_instance[mine]).any(), "type %d: no instance under a rotation and a scale, or none without" % kind
        self.instance_material = ids
        self.map_base = None
        from texture_cases import bc1_texture_above
        self.bc1 = bc1_texture_above(16, 16, 7, 64)   # blocks decoded per fetch; 64 / 255 >= ALBEDO_FLOOR in every channel of every texel and level
        self.bc1_index = len(self.pt.textures())
        self._oracle_textures = (self.view.keep["tex_table"], self.view.scene.textures, self.view.scene.texture_count)
        if self.ctx is not None:
            self.upload_textures(False)

    def upload_textures(self, with_bc1):
        """World's, with the three constant maps behind: 4 x 4 RGBA8 images with their whole mip chain, every texel the same. The BC1 texture of a bc1
        setup is self.bc1 (every texel at or above ALBEDO_FLOOR), at index self.bc1_index."""
        from test_gpu_texture_unit import TextureDesc
        scene_textures = self.pt.textures()
        extra = [self.bc1] if with_bc1 else []
        self._maps = [np.ascontiguousarray(np.tile(np.array(list(c) + [255], np.uint8), 16 + 4 + 1)) for c in MAP_TEXELS]
        count = len(scene_textures) + len(extra) + len(self._maps)
        descs = (TextureDesc * count)()
        for i, (texels, w, h, levels) in enumerate(scene_textures):
            descs[i].texels, descs[i].width, descs[i].height, descs[i].mip_levels, descs[i].format = texels.ctypes.data, w, h, levels, 0
            descs[i].lod_width, descs[i].lod_height = self.pt.texture_lod_size(i)
        k = len(scene_textures)
        for t in extra:
            d = descs[k]; k += 1
            d.texels, d.width, d.height, d.mip_levels, d.format = t.data.ctypes.data, t.width, t.height, t.mip_levels, t.format
        self.map_base = k
        for texels in self._maps:
            d = descs[k]; k += 1
            d.texels, d.width, d.height, d.mip_levels, d.format = texels.ctypes.data, 4, 4, 3, 0
        lib = self.lib
        lib.rt_set_texture_expansion.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.rt_upload_textures.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        assert lib.rt_set_texture_expansion(self.ctx, 0 if with_bc1 else 1) == 0, lib.rt_last_error(self.ctx)
        assert lib.rt_upload_textures(self.ctx, descs, count) == 0, lib.rt_last_error(self.ctx)
        self.textures_compressed = with_bc1

    def with_bc1_albedo(self, materials):
        """The materials table with the textured diffuse and plastic materials' albedo texture replaced by the BC1 texture."""
        out = materials.copy()
        textured = (materials[:, 3].view(np.int32) >= 0) & np.isin(self.material_types, (DIFFUSE, PLASTIC))
        assert {int(t) for t in self.material_types[textured]} == {DIFFUSE, PLASTIC}
        out[:, 3].view(np.int32)[textured] = self.bc1_index
        return out

    def oracle_textures(self, with_bc1):
        """The oracle's texture table: the scene's, and (with_bc1) the BC1 texture behind them as the RGBA8 chain its blocks decode to -- the oracle's
        unit reads texels, the device's decodes the blocks at every fetch (test_gpu_texture_unit.py holds the two to each other)."""
        from oracle.binding import OracleTexture
        from texture_reference import chain_bytes
        k, s = self.view.keep, self.view.scene
        table, pointer, count = self._oracle_textures
        if with_bc1:
            assert count == self.bc1_index
            chain = np.ascontiguousarray(chain_bytes(self.bc1.levels()))
            bigger = (OracleTexture * (count + 1))()
            for i in range(count):
                ctypes.memmove(ctypes.byref(bigger[i]), ctypes.byref(table[i]), ctypes.sizeof(OracleTexture))
            t = bigger[count]
            t.texels, t.width, t.height, t.mip_levels, t.lod_width, t.lod_height = chain.ctypes.data, self.bc1.width, self.bc1.height, self.bc1.mip_levels, 0, 0
            k["tex_table_bc1"], k["tex_chain_bc1"] = bigger, chain
            s.textures, s.texture_count = ctypes.cast(bigger, ctypes.c_void_p), count + 1
        else:
            s.textures, s.texture_count = pointer, count

    def triangles_where(self, what):
        """Triangle ids by their texture coordinates: "regular" (uv_det > 0), "mirrored" (uv_det < 0), "degenerate" (uv_det == 0); none a sliver."""
        sign = {"regular": self.uv_det > 0, "mirrored": self.uv_det < 0, "degenerate": self.uv_det == 0}[what]
        return np.nonzero(sign & (self.squareness > 0.2))[0].astype(np.int32)

    def set_maps(self, tables, which):
        """Puts normal maps in force: `which` maps a material type to one of MAP_TEXELS, for that type's materials that can take it -- the
        untextured ones of the diffuse and plastic slots (texel known, albedo constant), the transformed instances' of the dielectric and conductor
        slots (the spheres stay unmapped: every launch holds both kinds of hit). On the device and in `tables` (map_ids, map_texels) for
        material_reference.evaluate. An empty `which` clears them."""
        base = self.map_base if self.map_base is not None else len(self.pt.textures())
        ids = np.full(self.materials.shape[0], -1, np.int32)
        textured = self.materials[:, 3].view(np.int32) >= 0
        for kind, texel in which.items():
            for material in np.unique(self.instance_material[self.instances[kind]]):
                if kind in (DIFFUSE, PLASTIC):
                    takes = not textured[material]
                else:
                    takes = self.transformed_instance[(self.instance_material == material)].all()
                if takes:
                    ids[material] = base + MAP_TEXELS.index(texel)
        if self.ctx is not None:
            assert self.grt.upload_material_normal_maps(self.ctx, ids) == 0, self.lib.rt_last_error(self.ctx)
        tables.map_ids = ids if which else None
        tables.map_texels = {base + k: c for k, c in enumerate(MAP_TEXELS)}
        for k in range(base):
            tables.map_texels[k] = "varied"
        return ids


    def apply(self, setup):
        """World's, plus what an InstanceSetup asks for beyond a sky share -- delta lights (tables.delta), the light tree (tables.tree), a fog
        volume (tables.fog_active) -- on the device and in the tables of material_reference.evaluate; any other setup clears all three."""
        import delta_light_reference
        import light_tree_cases
        import light_tree_reference
        import material_reference
        grt, ctx = self.grt, self.ctx
        delta, tree, fog = getattr(setup, "delta", None), getattr(setup, "tree", False), getattr(setup, "fog", False)
        albedo = bool(getattr(setup, "bc1_albedo", False))
        assert not albedo or setup.bc1
        if ctx is not None:   # (the tree off before the light tables change: it is built again, from the tables in force, when it is enabled below)
            assert grt.set_light_tree(ctx, False) == 0 and grt.upload_delta_lights(ctx, None) == 0 and grt.set_fog_volume(ctx, None) == 0, self.lib.rt_last_error(ctx)
            if albedo and not self.textures_compressed:
                self.upload_textures(True)   # (before the materials that name the texture)
        scene_materials = self.rough_materials, self.smooth_materials
        if albedo:
            self.rough_materials, self.smooth_materials = (self.with_bc1_albedo(m) for m in scene_materials)
        try:
            tables = super().apply(setup)
        finally:
            self.rough_materials, self.smooth_materials = scene_materials
            self.materials = self.rough_materials
        self.oracle_textures(albedo)
        tables.delta = tables.tree = None
        tables.fog_active = bool(fog)
        if delta is not None:
            table = delta_light_reference.Table(DELTA_LIGHTS, DELTA_WEIGHTS)
            records = cdf = None
            if ctx is not None:
                assert grt.upload_delta_lights(ctx, grt.delta_light_records(DELTA_LIGHTS, DELTA_WEIGHTS), delta) == 0, self.lib.rt_last_error(ctx)
                records, cdf, share = grt.read_delta_lights(ctx)
                assert share == np.float32(delta)
            tables.delta = material_reference.Delta(table, delta, records, cdf)
        if tree:
            scene = light_tree_cases.scene_from_pathtracer(self.pt)
            want = light_tree_reference.build32(scene)
            nodes, slot_of_leaf, area = want.nodes, want.slot_of_leaf, want.leaves.area
            if ctx is not None:
                assert grt.set_light_tree(ctx, True) == 0, self.lib.rt_last_error(ctx)
                got = grt.read_light_tree(ctx)
                assert got.leaf_count == want.leaf_count > 0 and np.array_equal(got.nodes.view(np.uint32), want.nodes.view(np.uint32)), "the device's tree is not its restatement"
                nodes, slot_of_leaf, area = got.nodes, got.slot_of_leaf, got.leaf_area
            tables.tree = material_reference.TreeTables(scene, light_tree_reference.tree_from_nodes(nodes, want.leaf_count, slot_of_leaf), area)
        if fog and ctx is not None:
            assert grt.set_fog_volume(ctx, grt.fog_volume_record(*FOG)) == 0, self.lib.rt_last_error(ctx)
        return tables


# ---- every instance of the material launch (test_gpu_material_instances.py; the conditions on its launches in test_material.py) ----------

# The delta lights of the launch tests: a point light, a spot whose cones cross the scene, a directional light, a second point light
DELTA_LIGHTS = np.array([[0, 0.5, 3.0, 0.5, 0, 0, 1, 30, 25, 20, 0, 0],
                         [1, -1.5, 4.0, 1.0, 0.3, -1.0, -0.2, 80, 90, 100, 0.9, 0.5],
                         [2, 0, 0, 0, -0.3, -1.0, 0.2, 2.0, 2.5, 3.0, 0, 0],
                         [0, 2.0, 1.5, -1.0, 0, 0, 1, 4, 8, 12, 0, 0]], np.float32)   # delta_light_reference.lights_array rows
DELTA_WEIGHTS = np.array([3.0, 2.0, 4.0, 1.0], np.float32)
FOG = ((-6.0, 0.0, -6.0), (6.0, 3.0, 6.0), 0.02, 0.05, 0.3)   # fog_volume_record's arguments: a box around the scene, absorbing and scattering
LIGHT_SUFFIXES = ("", "_sky", "_split", "_tree")   # by rt_light_split


class InstanceSetup(Setup):
    """Setup plus `delta`: the share rt_upload_delta_lights gives DELTA_LIGHTS (None: no delta lights); `tree`: the light tree on; `fog`: the
    volume FOG in force; `bc1_albedo` (with bc1): the textured diffuse and plastic materials take the BC1 texture as their albedo, so that the blocks
    are decoded inside the material kernel."""

    def __init__(self, name, config=None, delta=None, tree=False, fog=False, bc1_albedo=False, **rest):
        super().__init__(name, config, **rest)
        self.delta, self.tree, self.fog, self.bc1_albedo = delta, tree, fog, bc1_albedo


def light_split(tables):
    """rt_light_split for the tables of a setup in force: tree > delta share > sky share."""
    import material_reference
    nee_on, share, lit, delta, tree, fog = material_reference.settings_in_force(tables)
    return 3 if tree is not None else 2 if delta is not None else 1 if share > 0 else 0


def instance(world, tables, launch):
    """The __global__ entry point material_kernels_for picks for the launch (kernels_material.hip): the slot's row (the _texels one of the diffuse and
    plastic slots while no texture holds compressed blocks), the form, the split in force, the slot's bit of normal_map_slots."""
    map_ids = getattr(tables, "map_ids", None)
    mapped = map_ids is not None and bool((map_ids[tables.material_types == SLOT_TYPES[launch.slot]] >= 0).any())
    return instance_name(launch.slot, launch.merged, launch.slot < 2 and not world.textures_compressed, light_split(tables), mapped)


def instance_name(slot, merged, texels, split, mapped):
    return "kernel_material_" + SLOT_NAMES[slot] + ("_stream" if merged else "") + ("_texels" if texels else "") + LIGHT_SUFFIXES[split] + ("_nmap" if mapped else "")


def all_instances():
    """The 96 names by the rule: 6 rows (four slots, the _texels forms of the first two) x 4 splits x _nmap x 2 forms."""
    return {instance_name(slot, merged, texels, split, mapped) for slot in range(4) for texels in ((False, True) if slot < 2 else (False,))
            for split in range(4) for mapped in (False, True) for merged in (False, True)}


def listed_instances(path):
    """The same set read from rt_material.h as text: the rows of RT_MATERIAL_KERNEL_LIST, the suffixes of RT_MATERIAL_KERNEL_VARIANTS, and
    RT_DEFINE_MATERIAL_KERNELS' two names per pair."""
    import re
    text = open(path).read()
    rows = re.findall(r"^\tX\((\w+),\s*(\w*),\s*\w+(?:<\w+>)?,\s*(\d),", text, re.M)
    variants = text[text.index("#define RT_MATERIAL_KERNEL_VARIANTS(X)"):text.index("#define RT_DEFINE_MATERIAL_KERNELS")]
    suffixes = re.findall(r"RT_MATERIAL_KERNEL_LIST\(X, (\w*), (\d), (true|false)\)", variants)
    assert len(rows) == 6 and len(suffixes) == 8, (rows, suffixes)
    for suffix, split, mapped in suffixes:   # (a suffix says what its template arguments say)
        assert suffix == LIGHT_SUFFIXES[int(split)] + ("_nmap" if mapped == "true" else ""), (suffix, split, mapped)
    for material, texels, slot in rows:
        assert SLOT_NAMES[int(slot)] == material, (material, slot)
    return {"kernel_material_%s%s%s%s" % (material, stream, texels, suffix) for material, texels, _ in rows for suffix, _, _ in suffixes for stream in ("", "_stream")}


LIGHT_VARIANTS = {   # light variant -> what puts it in force: all three routes under _split and _tree
    "": dict(),
    "_sky": dict(sky_sampling=0.25),
    "_split": dict(sky_sampling=0.25, delta=0.5),
    "_tree": dict(sky_sampling=0.25, delta=0.5, tree=True),
}
# per-bounce, merged: the shortest rung of a ladder of LENGTH_STEP entries a step at which every route in force holds more than 100 robust shadow entries in every
# launch of INSTANCE_CASES -- found on the CPU from the reference alone (test_material.py: test_instance_launches_are_the_shortest_that_hold_every_route)
INSTANCE_LENGTHS, LENGTH_STEP = (1250, 1500), 250


def instance_setup(variant, compressed=False, **changes):
    name = "instances%s%s" % (variant or "_plain", "_bc1" if compressed else "") + "".join("_%s" % k for k in sorted(changes) if changes[k])
    settings = dict(LIGHT_VARIANTS[variant], bc1=compressed, bc1_albedo=compressed)
    config = {}
    if changes.pop("mis_off", False):
        config["enable_multiple_importance_sampling"] = 0
    if changes.pop("taken0", False):
        settings.update(sky_sampling=0.0, delta=None)
    settings.update(changes)
    return InstanceSetup(name, config, **settings)


INSTANCE_ROWS = tuple((slot, compressed) for compressed in (False, True) for slot in ((0, 1, 2, 3) if not compressed else (0, 1)))   # the six rows of RT_MATERIAL_KERNEL_LIST


# every (light variant, mapped, slot, compressed) whose two launches make up the 96: the rows that can decode compressed blocks last (the textures are
# uploaded again when a setup changes that)
INSTANCE_CASES = [(light, mapped, slot, compressed) for compressed in (False, True) for mapped in (False, True) for light in LIGHT_VARIANTS
                  for slot, c in INSTANCE_ROWS if c == compressed]


def instance_case_id(case):
    light, mapped, slot, compressed = case
    return "%s%s-%s%s" % (light.lstrip("_") or "plain", "_nmap" if mapped else "", SLOT_NAMES[slot], "" if compressed or slot >= 2 else "_texels")


def instance_launches(world, variant, mapped, slot, compressed, lengths=INSTANCE_LENGTHS, tag="instances"):
    """One per-bounce launch (bounce 0 and 2 alternate across the rows) and one merged launch of a row: (maps, launch) pairs. A mapped launch draws
    from the regular and the mirrored triangles, as map_launches does."""
    row = INSTANCE_ROWS.index((slot, compressed))
    k = 100 * tuple(LIGHT_VARIANTS).index(variant) + 50 * mapped + 4 * row
    maps = {SLOT_TYPES[slot]: TILT} if mapped else {}
    out = [per_bounce(world, tag, slot, lengths[0], (0, 2)[row % 2], seed=6000 + k), merged(world, tag, slot, lengths[1], seed=6001 + k)]
    if mapped:
        both = np.concatenate([world.triangles_where("regular"), world.triangles_where("mirrored")])
        for launch in out:
            launch.entries.triangle[:] = np.random.default_rng(6002 + k).choice(both, launch.entries.n)
    return [(maps, launch) for launch in out]


def instance_length_launches(world, variant_index):
    """Order and structure of one light variant: one entry, one wave, a workgroup and one entry; per bounce and merged, over the slots in turn."""
    out = []
    for k, n in enumerate(SKY_LENGTHS):
        out.append(per_bounce(world, "instances_length", (2 * k + variant_index) % 4, n, 1, seed=6500 + 10 * variant_index + k, slots=1))
        out.append(merged(world, "instances_length", (2 * k + 1 + variant_index) % 4, n, seed=6550 + 10 * variant_index + k))
    return out


def fog_launches(world):
    """The material launch while a fog volume is in force: bounce 0 per bounce and the merged form, the diffuse and the conductor slot. Every entry
    carries a throughput of its own, bounce 0 included (the ..._fog sort instance stores it: the first segment may have crossed the fog)."""
    out = []
    for slot in (0, 3):
        for launch in (per_bounce(world, "fog", slot, 1500, 0, seed=6600 + slot), merged(world, "fog", slot, 2500, seed=6610 + slot)):
            e = launch.entries
            rng = np.random.default_rng(6620 + slot)
            first = launch.paths()[2] == 0
            e.throughput[first] = (rng.uniform(0.2, 0.9, (int(first.sum()), 3)) * rng.uniform(0.3, 1.0, (int(first.sum()), 1))).astype(np.float32)
            launch.first_throughput = True   # (per_bounce and merged build the plain queue; this one is the fog's)
            out.append(launch)
    return out


class WideWorld(VariantWorld):
    """VariantWorld in a frame of 128 x 64 pixels: 8192 x 256 + 1 distinct (slot, pixel) entries fit the slot table's 512 sample slots (257 of them)."""
    FRAME = (2 * WIDTH, HEIGHT)


STREAM_SECOND_ROUND = STREAM_GRID * BLOCK + 1   # merged form: one entry in a second grid-stride round


def second_round_merged(world, slot, seed):
    """8192 x 256 + 1 entries of the merged form: the last one is alone in the second grid-stride round. Every sample slot the entries need has a row in the
    table, over three submissions at bounces 0, 1 and the last."""
    rng = np.random.default_rng(seed)
    n, iteration = STREAM_SECOND_ROUND, NUM_BOUNCES + 3
    slots = slots_needed(n, world.frame_pixels)
    assert slots <= 512
    k = np.arange(slots)
    submission = np.array([3, 9, 64])[k % 3]
    birth = np.array([iteration, iteration - 1, iteration - (NUM_BOUNCES - 1)])[k % 3]
    table = np.stack([1000 + k, birth, submission, k // 3], axis=1).astype(np.int32)
    births = np.full(SUBMISSIONS, iteration + 1000, np.int32)
    births[[3, 9, 64]] = [iteration, iteration - 1, iteration - (NUM_BOUNCES - 1)]
    px = pixels_for(rng, n, world.frame_pixels, slots)
    bounce = iteration - table[px // world.frame_pixels, 1]
    e = make_entries(world, rng, px, slot, bounce)
    return Launch("second_round_%s_merged_%d" % (SLOT_NAMES[slot], n), slot, e, world.frame_pixels, slots, iteration=iteration, slot_table=table, submission_birth=births)


def value_sample(n, seed):
    """At most MAX_VALUE_ENTRIES of n entries: the last 257 and a seeded random sample of the rest."""
    rest = np.random.default_rng(seed).choice(n - 257, MAX_VALUE_ENTRIES - 257, replace=False)
    return np.unique(np.concatenate([rest, np.arange(n - 257, n)]))


def _restrict(world, launch, what, seed, meshes=None):
    """The launch with its triangles drawn from triangles_where(what) (and its instances from `meshes`)."""
    rng = np.random.default_rng(seed)
    launch.entries.triangle[:] = rng.choice(world.triangles_where(what), launch.entries.n)
    if meshes is not None:
        launch.entries.mesh[:] = rng.choice(np.asarray(meshes, np.int32), launch.entries.n)
    return launch


def sky_launches(world, setup):
    """The _sky instances under a setup with a sky share: under sky_share_0.5 all four slots at bounce 0 and 2 (1500 entries) and merged (2500);
    under the others bounce 1 of the diffuse and the conductor slot and the merged plastic one."""
    tag = "sky"
    if setup.name == "sky_share_0.5":
        out = []
        for slot in range(4):
            out += [per_bounce(world, tag, slot, 1500, b, seed=4000 + 10 * slot + b) for b in (0, 2)]
            out.append(merged(world, tag, slot, 2500, seed=4050 + slot))
        return out
    k = [s.name for s in SKY_SETUPS].index(setup.name)
    return [per_bounce(world, tag, 0, 1500, 1, seed=4100 + 10 * k), per_bounce(world, tag, 3, 1500, 1, seed=4101 + 10 * k), merged(world, tag, 1, 2500, seed=4102 + 10 * k)]


SKY_LENGTHS = (1, 64, 257)


def sky_length_launches(world):
    """Order and structure of the _sky instances (sky_share_0.5): one entry, one wave, a workgroup and one entry; per bounce and merged."""
    out = []
    for k, n in enumerate(SKY_LENGTHS):
        out.append(per_bounce(world, "sky_length", (2 * k) % 4, n, 1, seed=4200 + k, slots=1))
        out.append(merged(world, "sky_length", (2 * k + 1) % 4, n, seed=4210 + k))
    return out


def sky_lights_launch(world):
    """A LightsWorld launch (meshes65: the light tables in global memory) for a _sky instance."""
    return light_table_launches(world)[1]


def lights_world_sky(world, share, sky):
    """Gives a LightsWorld the sky `sky` ((H, W, 4) float32) and a sky share: in the oracle's view, on the device, and in world.tables."""
    import sky_sampling_reference as sky_ref
    s, k = world.view.scene, world.view.keep
    k["sky"] = sky; s.sky = sky.ctypes.data; s.sky_height, s.sky_width = sky.shape[:2]; s.sky_scale = 1.0
    if world.ctx is not None:
        lib = world.lib
        lib.rt_set_sky_sampling.argtypes = [ctypes.c_void_p, ctypes.c_float]
        assert lib.rt_set_sky(world.ctx, sky.ctypes.data, sky.shape[1], sky.shape[0], ctypes.c_float(1.0)) == 0, lib.rt_last_error(world.ctx)
        assert lib.rt_set_sky_sampling(world.ctx, share) == 0, lib.rt_last_error(world.ctx)
    t = world.tables
    t.sky = np.asarray(sky, np.float32); t.sky_scale = 1.0
    t.sky_share = float(np.float32(share)); t.sky_tables = sky_ref.Tables(t.sky)
    return t


def map_launches(world):
    """The _nmap instances (SKY == 0, under svgf_on): (maps, launch) pairs, `maps` what set_maps takes. The tilt map on the dielectric and the
    conductor slot (bounce 0, 2, merged) and on the untextured diffuse and plastic materials; the two other constant maps on the conductor
    slot; the conductor slot on mirrored triangles only and on triangles without texture coordinates only. The general launches draw from
    the regular and the mirrored triangles alike."""
    out = []
    both = np.concatenate([world.triangles_where("regular"), world.triangles_where("mirrored")])
    for slot in (2, 3, 0, 1):
        maps = {SLOT_TYPES[slot]: TILT}
        for launch in [per_bounce(world, "nmap", slot, 1500, b, seed=4300 + 10 * slot + b) for b in (0, 2)] + [merged(world, "nmap", slot, 1500, seed=4350 + slot)]:
            launch.entries.triangle[:] = np.random.default_rng(4360 + slot).choice(both, launch.entries.n)
            out.append((maps, launch))
    for k, (texel, label) in enumerate(((FLAT, "flat"), (INWARD, "inward"))):
        launch = per_bounce(world, "nmap_" + label, 3, 1500, 0, seed=4400 + k)
        launch.entries.triangle[:] = np.random.default_rng(4410 + k).choice(both, launch.entries.n)
        out.append(({CONDUCTOR: texel}, launch))
    mapped_conductors = [i for i in world.instances[CONDUCTOR] if world.transformed_instance[i]]
    out.append(({CONDUCTOR: TILT}, _restrict(world, per_bounce(world, "nmap_mirrored", 3, 1500, 0, seed=4420), "mirrored", 4421, mapped_conductors)))
    out.append(({CONDUCTOR: TILT}, _restrict(world, per_bounce(world, "nmap_degenerate", 3, 1500, 0, seed=4430), "degenerate", 4431, mapped_conductors)))
    return out


def sky_map_launches(world):
    """The _sky_nmap instances (sky_share_0.5, the tilt map): the diffuse and the conductor slot, bounce 1 per bounce and merged."""
    out = []
    both = np.concatenate([world.triangles_where("regular"), world.triangles_where("mirrored")])
    for slot in (0, 3):
        for launch in (per_bounce(world, "sky_nmap", slot, 1500, 1, seed=4500 + slot), merged(world, "sky_nmap", slot, 1500, seed=4510 + slot)):
            launch.entries.triangle[:] = np.random.default_rng(4520 + slot).choice(both, launch.entries.n)
            out.append(({SLOT_TYPES[slot]: TILT}, launch))
    return out
