"""Alpha-tested opacity masks on the device: the bits rt_upload_material_opacity builds, its errors, the CWBVH
kernels' _mask instances on explicit rays and through the frame's launch against the masked float64 brute force
(tests/opacity_reference.py), exact identities (an all-ones mask, an all-zeros mask, no mask), frames, and Sponza's cut-outs.

The oracle knows nothing of masks: masked scenes are pinned by float64 here. What the oracle still gives is the deepest walk of
the same scene without masks, which bounds the masked walk (a rejected candidate pushes nothing), checked against RT_STACK_SIZE
before any launch.
"""
import ctypes
import os
from ctypes import byref, c_int, c_int32, c_size_t, c_void_p

import numpy as np
import pytest

import opacity_cases as ocases
import opacity_reference as oref
import texture_cases
import trace_cases as cases
import trace_checks as checks
import trace_reference as ref

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG = -1
REL_L1_TOL = 1e-4                       # the suite's frame tolerance (tests/test_gpu_full_size.py)
SENTINEL = np.uint32(0xA5A5A5A5)
KERNEL_GENERAL_MASK, KERNEL_FLAT_MASK, KERNEL_FLAT_SKIP_MASK, KERNEL_COUNTING_MASK = 4, 5, 6, 7
SIZES = [(1, 1), (5, 3), (31, 1), (32, 1), (33, 70), (64, 64), (256, 16)]   # (W, H)


class TextureDesc(ctypes.Structure):   # rt_texture_desc
    _fields_ = [("texels", c_void_p), ("width", c_int32), ("height", c_int32), ("mip_levels", c_int32),
                ("lod_width", c_int32), ("lod_height", c_int32), ("format", c_int32), ("reserved", c_int32)]


def record(line):
    """The measured numbers (profiles/opacity_masks.txt holds a run's): printed, `pytest -s` shows them."""
    print(line)


# ---- a bare context with textures and materials -----------------------------------------------------------------

def random_images(seed):
    """RGBA8 images of SIZES whose bytes cover 0..255 and sit on the cuts (0, 1, 127, 128, 254, 255) often."""
    rng = np.random.default_rng(seed)
    out = []
    for w, h in SIZES:
        img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        edge = rng.random((h, w, 4)) < 0.4
        img[edge] = rng.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), int(edge.sum()))
        out.append(img)
    return out


def upload_textures(lib, ctx, images, extra=()):
    lib.rt_upload_textures.argtypes = [c_void_p, c_void_p, c_size_t]
    descs = (TextureDesc * (len(images) + len(extra)))()
    keep = [np.ascontiguousarray(i) for i in images]
    for d, img in zip(descs, keep):
        d.texels = img.ctypes.data; d.width = img.shape[1]; d.height = img.shape[0]; d.mip_levels = 1; d.format = 0
    for d, t in zip(descs[len(images):], extra):
        d.texels = t.data.ctypes.data; d.width = t.width; d.height = t.height; d.mip_levels = t.mip_levels; d.format = t.format
    assert lib.rt_upload_textures(ctx, descs, len(descs)) == 0, lib.rt_last_error(ctx)


def upload_diffuse_materials(lib, ctx, count, light_at=None):
    types = np.full(count, 1, np.uint8)          # RT_MATERIAL_DIFFUSE
    if light_at is not None:
        types[light_at] = 0
    records = np.zeros((count, 8), np.float32); records[:, :3] = 0.5
    assert lib.rt_upload_materials(ctx, types.ctypes.data, records.ctypes.data, count) == 0, lib.rt_last_error(ctx)


def read_words(lib, ctx, material, width, height, slack=0):
    n = (width * height + 31) // 32
    words = np.full(n + slack, 0xDEADBEEF, np.uint32)
    w, h = c_int(), c_int()
    status = lib.rt_read_material_opacity(ctx, material, words.ctypes.data, n + slack, byref(w), byref(h))
    return status, words, (w.value, h.value)


@pytest.fixture()
def bare(grt):
    lib = grt.device_lib()
    lib.rt_set_texture_expansion.argtypes = [c_void_p, c_int]
    ctx = c_void_p()
    assert lib.rt_create(0, byref(ctx)) == 0
    yield lib, ctx
    lib.rt_destroy(ctx)


# ---- 1. bits ----------------------------------------------------------------------------------------------------

def test_bits_equal_the_reference(grt, bare):
    """rt_read_material_opacity equals pack_bits of the chosen channel >= ceil(threshold * 255), bit for bit, for every size, channels
    0 and 3 and thresholds 1 / 255, 0.5 and 1; the unused bits of the last word are 0; a second build gives the same words."""
    lib, ctx = bare
    images = random_images(41)
    upload_textures(lib, ctx, images)
    upload_diffuse_materials(lib, ctx, len(images))
    ids = np.arange(len(images))
    for channel in (0, 3):
        for threshold in (1 / 255, 0.5, 1.0):
            builds = []
            for _ in range(2):
                assert grt.upload_material_opacity(ctx, ids, [channel] * len(images), [threshold] * len(images)) == 0, lib.rt_last_error(ctx)
                got = []
                for m, img in enumerate(images):
                    h, w = img.shape[:2]
                    status, words, size = read_words(lib, ctx, m, w, h, slack=1)
                    assert status == 0 and size == (w, h)
                    assert words[-1] == 0xDEADBEEF                       # nothing written past the mask's words
                    want = oref.pack_bits(oref.opaque_of(img, channel, threshold))
                    assert np.array_equal(words[:-1], want), (w, h, channel, threshold)
                    if (w * h) % 32:
                        assert words[-2] >> ((w * h) % 32) == 0, (w, h)   # the tail
                    assert np.array_equal(grt.read_material_opacity(ctx, m), oref.opaque_of(img, channel, threshold))
                    got.append(words[:-1].copy())
                builds.append(got)
            assert all(np.array_equal(a, b) for a, b in zip(*builds))


# ---- 2. errors --------------------------------------------------------------------------------------------------

def test_upload_errors_leave_the_tables_as_they_were(grt, bare):
    lib, ctx = bare
    images = random_images(42)[:3]
    assert lib.rt_set_texture_expansion(ctx, 0) == 0
    bc1 = texture_cases.bc1_texture(8, 8, 5)
    upload_textures(lib, ctx, images, extra=[bc1])           # texture 3 is not RT_TEXTURE_RGBA8
    n = 4
    upload_diffuse_materials(lib, ctx, n, light_at=3)
    good = ([0, 1, -1, 2], [3, 0, 0, 1], [0.5, 0.25, 0.5, 1.0])
    assert grt.upload_material_opacity(ctx, *good) == 0, lib.rt_last_error(ctx)

    def table():
        out = []
        for m in range(n):
            status, words, size = read_words(lib, ctx, m, 70, 70)
            out.append((status, size, words[:(size[0] * size[1] + 31) // 32].tolist() if status == 0 else None))
        return out
    before = table()
    assert [s for s, _, _ in before] == [0, 0, RT_ERROR_INVALID_ARG, RT_ERROR_INVALID_ARG]     # none; a mask on a light is ignored
    assert before[0][2] == oref.pack_bits(oref.opaque_of(images[0], 3, 0.5)).tolist() and before[1][2] == oref.pack_bits(oref.opaque_of(images[1], 0, 0.25)).tolist()
    nan = float("nan")
    bad = [(([0, 1, -1], [3, 0, 0], [0.5] * 3), b"materials"),                                  # count differs from rt_upload_materials
           (([0, 1, -1, 2, 0], [0] * 5, [0.5] * 5), b"materials"),
           (([0, 4, -1, 2], [0] * 4, [0.5] * 4), b"names texture"),                             # id out of range
           (([0, -2, -1, 2], [0] * 4, [0.5] * 4), b"names texture"),
           (([0, 3, -1, 2], [0] * 4, [0.5] * 4), b"RT_TEXTURE_RGBA8"),                          # a BC1 texture
           (([0, 1, -1, 2], [0, 4, 0, 0], [0.5] * 4), b"channel"),
           (([0, 1, -1, 2], [0, -1, 0, 0], [0.5] * 4), b"channel"),
           (([0, 1, -1, 2], [0] * 4, [0.5, 0.0, 0.5, 0.5]), b"threshold"),
           (([0, 1, -1, 2], [0] * 4, [0.5, -0.25, 0.5, 0.5]), b"threshold"),
           (([0, 1, -1, 2], [0] * 4, [0.5, 1.0000001, 0.5, 0.5]), b"threshold"),
           (([0, 1, -1, 2], [0] * 4, [0.5, nan, 0.5, 0.5]), b"threshold")]
    for args, message in bad:
        assert grt.upload_material_opacity(ctx, *args) == RT_ERROR_INVALID_ARG, args
        assert message in lib.rt_last_error(ctx), (args, lib.rt_last_error(ctx))
        assert table() == before, args
    # capacity too small; a material out of range
    small = np.zeros(1, np.uint32)
    assert lib.rt_read_material_opacity(ctx, 1, small.ctypes.data, 0, None, None) == RT_ERROR_INVALID_ARG
    assert lib.rt_read_material_opacity(ctx, 7, small.ctypes.data, 1, None, None) == RT_ERROR_INVALID_ARG
    # NULL clears; rt_upload_materials and rt_upload_textures reset
    assert grt.upload_material_opacity(ctx, None, None, None) == 0
    assert [s for s, _, _ in table()] == [RT_ERROR_INVALID_ARG] * n
    assert grt.upload_material_opacity(ctx, *good) == 0 and table() == before
    upload_diffuse_materials(lib, ctx, n)
    assert [s for s, _, _ in table()] == [RT_ERROR_INVALID_ARG] * n
    assert grt.upload_material_opacity(ctx, *good) == 0
    upload_textures(lib, ctx, images)
    assert [s for s, _, _ in table()] == [RT_ERROR_INVALID_ARG] * n


def test_masks_with_another_bvh_type_are_refused(grt, tmp_path):
    """With a mask uploaded, rt_set_bvh_type(ctx, 4) or 2 makes rt_trace_rays and the render entry points return RT_ERROR_INVALID_ARG
    before any launch; back at 8, or with the masks cleared, they run."""
    case = ocases.case_tiny(str(tmp_path), "tiny_bvh", np.array([[True, False]]), rays=64)
    scene, pt = checks.load(grt, case, 0)
    lib = grt.device_lib()
    try:
        hits, _ = grt.trace_rays(pt.ctx, case.origin, case.direction)
        for width in (4, 2):
            assert lib.rt_set_bvh_type(pt.ctx, width) == 0
            with pytest.raises(RuntimeError, match="opacity masks"):
                grt.trace_rays(pt.ctx, case.origin, case.direction)
            with pytest.raises(RuntimeError, match="opacity masks"):
                grt.trace_shadow_rays(pt.ctx, case.origin, case.direction, np.ones(64, np.float32))
            assert lib.rt_render_sample(pt.ctx, 0) == RT_ERROR_INVALID_ARG
        assert lib.rt_set_bvh_type(pt.ctx, 8) == 0
        again, _ = grt.trace_rays(pt.ctx, case.origin, case.direction)
        assert np.array_equal(hits, again)
    finally:
        pt.close(); scene.close()


# ---- what the float64 side needs from a loaded case ---------------------------------------------------------------

class Loaded:
    """A case on the device, its masked brute force (shared by the tests of a module run) and the product's own tables."""
    _brute = {}

    def __init__(self, grt, case, **config):
        self.grt, self.case = grt, case
        self.scene, self.pt = checks.load(grt, case, 0, **config)
        tri = self.pt.array("triangles").reshape(-1, 24)
        self.uv = tri[:, 18:24].astype(np.float64)
        # the case's restatement of the loader's texture coordinates is what the device holds (every case row appears among the staged triangles)
        staged = {tuple(row) for row in tri[:, 18:24].tolist()}
        mine = np.concatenate([case.uv0, case.uve1, case.uve2], 1).astype(np.float32)
        assert all(tuple(row) in staged for row in mine.tolist()), case.name
        # the mask of every instance row, through its material: the device's bits must be one of the case's masks
        self.material_of_mesh = self.pt.array("mesh_material_ids")
        self.mask_of_material = {}
        for material in sorted(set(self.material_of_mesh.tolist())):
            if material < 0:
                continue
            try:
                bits = grt.read_material_opacity(self.pt.ctx, material)
            except RuntimeError:
                continue
            match = [k for k, m in enumerate(case.masks) if m.shape == bits.shape and np.array_equal(m, bits)]
            assert match, (case.name, material)
            self.mask_of_material[material] = match[0]

    def brute(self, which="origin"):
        key = (self.case.name, which)
        if key not in Loaded._brute:
            c = self.case
            o, d = (c.origin, c.direction) if which == "origin" else (c.more_origin, c.more_direction)
            Loaded._brute[key] = oref.masked_brute_force(o, d, c.world, c.uv0, c.uve1, c.uve2, c.mask_of_triangle, c.masks)[0]
        return Loaded._brute[key]

    def check_named_texels(self, label, origin, direction, hits, bf, only_robust=True):
        """No (robust) ray may name an (instance, triangle, u, v) whose float64 texel is 0 and not texel-ambiguous. Returns the share of
        hits on masked materials that were left out as texel-ambiguous."""
        mesh, tri, _, _, _ = checks.unpack(hits)
        idx = np.nonzero(tri >= 0)[0]
        if only_robust:
            idx = idx[ref.robust_closest(bf)[idx]]
        masked = np.array([self.material_of_mesh[m] in self.mask_of_material for m in mesh[idx]], bool)
        idx = idx[masked]
        if idx.size == 0:
            return 0.0
        world = ref.world_triangles_of_hits(self.pt.array("triangles"), self.pt.array("mesh_transforms"), mesh[idx], tri[idx])
        _, _, _, _, un, vn, uv_tol, _ = ref.evaluate_named(origin[:, idx], direction[:, idx], world)
        uv = self.uv[tri[idx]]
        left_out = 0
        for material, k in self.mask_of_material.items():
            rows = np.nonzero(self.material_of_mesh[mesh[idx]] == material)[0]
            if rows.size == 0:
                continue
            bit, ambiguous = oref.classify(self.case.masks[k], un[rows], vn[rows], uv_tol[rows], uv[rows, 0:2], uv[rows, 2:4], uv[rows, 4:6])
            bad = rows[~bit & ~ambiguous]
            assert bad.size == 0, "%s: %d hits lie on a clear texel, first ray %d" % (label, bad.size, idx[bad[0]])
            left_out += int(ambiguous.sum())
        return left_out / idx.size

    def close(self):
        self.pt.close(); self.scene.close()


@pytest.fixture(scope="module")
def masked_cases(tmp_path_factory):
    return ocases.all_cases(str(tmp_path_factory.mktemp("opacity_cases_gpu")))


def configurations(case):
    """A case's contexts: the flattened tree with the skipping walk on and off, or the TLAS engines (merge_static = 0)."""
    if case.config.get("merge_static", 1) == 0:
        return [({}, KERNEL_GENERAL_MASK)]
    return [({}, KERNEL_FLAT_SKIP_MASK), ({"skip_behind_hit": 0}, KERNEL_FLAT_MASK)]


def six(bf):
    return ref.BruteForce(**{k: np.repeat(v, 6) for k, v in bf.__dict__.items()})


# ---- 3. explicit rays -------------------------------------------------------------------------------------------

def test_explicit_rays_against_the_masked_brute_force(grt, masked_cases):
    """Every case through rt_trace_rays and rt_trace_shadow_rays (the 8-lanes-per-ray path; `layers` also with 24 000 rays, the
    lane-per-ray path): trace_checks' float64 rules against the masked brute force, and no robust ray names a clear texel."""
    for case in masked_cases:
        for config, _ in configurations(case):
            loaded = Loaded(grt, case, **config)
            try:
                label = "%s / %s" % (case.name, config)
                bf = loaded.brute()
                hits, _ = grt.trace_rays(loaded.pt.ctx, case.origin, case.direction)
                checks.check_closest(label, case, loaded.pt, case.origin, case.direction, hits, bf)
                loaded.check_named_texels(label, case.origin, case.direction, hits, bf)
                so, sd, md = ocases.shadow_rays(case, bf)
                occluded, _ = grt.trace_shadow_rays(loaded.pt.ctx, so, sd, md)
                checks.check_shadow(label, occluded, six(bf), md)
                if case.more_origin is not None:
                    more = loaded.brute("more")
                    hits, _ = grt.trace_rays(loaded.pt.ctx, case.more_origin, case.more_direction)
                    checks.check_closest(label + " (wide)", case, loaded.pt, case.more_origin, case.more_direction, hits, more)
                    loaded.check_named_texels(label + " (wide)", case.more_origin, case.more_direction, hits, more)
                    so, sd, md = ocases.shadow_rays(case, more, origin=case.more_origin, direction=case.more_direction)
                    occluded, _ = grt.trace_shadow_rays(loaded.pt.ctx, so, sd, md)
                    checks.check_shadow(label + " (wide)", occluded, six(more), md)
            finally:
                loaded.close()


# ---- 4. the frame's launch --------------------------------------------------------------------------------------

def probe(grt, pt, iteration, o, d, so, sd, md, counting=False):
    hits = np.full((o.shape[1], 4), SENTINEL, np.uint32)
    return grt.trace_stream_rays(pt.ctx, iteration, o, d, hits, so, sd, md, counting=counting)


def test_stream_launch_against_the_masked_brute_force(grt, oracle, masked_cases):
    """layers (flattened, skipping walk on and off), layers under the TLAS and instanced through rt_trace_stream_rays: both
    parities, a narrow batch (<= 6 000 + 10 000 rays) and a full one, and the counting kernel. info[0] names the masked instance
    of the expected engine, no record stays at the sentinel, shadow_light is 0 or 1, the float64 rules hold, and the narrow and
    the wide batch agree bit for bit on the rays they share."""
    for case in masked_cases:
        if case.name.startswith("tiny"):
            continue
        for config, kernel in configurations(case):
            loaded = Loaded(grt, case, **config)
            try:
                pt, label = loaded.pt, "%s / %s" % (case.name, config)
                if case.more_origin is not None:   # more than RT_NARROW_MAX_RAYS in the full batch: the lane-per-ray engine
                    o, d = np.concatenate([case.origin, case.more_origin], 1), np.concatenate([case.direction, case.more_direction], 1)
                    bf = ref.BruteForce(**{k: np.concatenate([v, getattr(loaded.brute("more"), k)]) for k, v in loaded.brute().__dict__.items()})
                else:
                    o, d, bf = case.origin, case.direction, loaded.brute()
                so, sd, md = ocases.shadow_rays(case, bf, origin=o, direction=d)
                view = oracle.SceneView(pt)                                    # the unmasked walk of the same scene bounds the masked one's stack
                _, cstats = view.trace(o, d)
                _, sstats = view.trace_shadow(so, sd, md)
                assert cstats.max_stack <= checks.STACK_LIMIT and sstats.max_stack <= checks.STACK_LIMIT, label   # (before any launch)
                n, m = o.shape[1], so.shape[1]
                results = {}
                for iteration, nc, ns in ((0, min(n, 6000), min(m, 10000)), (1, n, m), (2, n, m), (3, min(n, 6000), min(m, 10000))):
                    hits, light, _, info = probe(grt, pt, iteration, o[:, :nc], d[:, :nc], so[:, :ns], sd[:, :ns], md[:ns])
                    assert info[0] == kernel, (label, info)
                    assert nc + ns <= info[3] and (iteration not in (0, 3) or nc + ns <= info[2]), (label, info)
                    if case.more_origin is not None and iteration in (1, 2):
                        assert nc + ns > info[2], (label, info)               # the full batch is beyond the narrow engine
                    assert not (hits == SENTINEL).all(1).any(), "%s: %d closest-hit rays never dealt" % (label, (hits == SENTINEL).all(1).sum())
                    assert np.isin(light, (0.0, 1.0)).all(), "%s: shadow rays dealt %s times" % (label, sorted(set(light.tolist())))
                    results[iteration] = (hits, light)
                    sub = ref.BruteForce(**{k: v[:nc] for k, v in bf.__dict__.items()})
                    checks.check_closest("%s, iteration %d" % (label, iteration), case, pt, o[:, :nc], d[:, :nc], hits, sub)
                    loaded.check_named_texels(label, o[:, :nc], d[:, :nc], hits, sub)
                    checks.check_shadow(label, 1.0 - light, ref.BruteForce(**{k: v[:ns] for k, v in six(bf).__dict__.items()}), md[:ns])
                nc, ns = results[0][0].shape[0], results[0][1].size
                assert np.array_equal(results[0][0], results[1][0][:nc]) and np.array_equal(results[0][1], results[1][1][:ns]), label   # narrow == wide
                assert np.array_equal(results[1][0], results[2][0]) and np.array_equal(results[0][0], results[3][0]), label              # the parities
                if not config:
                    hits, light, stats, info = probe(grt, pt, 1, o, d, so, sd, md, counting=True)
                    assert info[0] == KERNEL_COUNTING_MASK
                    assert np.array_equal(hits, results[1][0]) and np.array_equal(light, results[1][1]), label
                    assert stats["closest"]["rays"] == n and stats["shadow"]["rays"] == m
            finally:
                loaded.close()


# ---- 5. identities ----------------------------------------------------------------------------------------------

def test_an_all_ones_mask_changes_nothing(grt, tmp_path):
    """layers and instanced with every bit 1: hit records and shadow results, explicit and through the frame's launch, are
    bit-identical to the same context after its masks are cleared (the plain instances)."""
    solid = [ocases.case_layers(str(tmp_path), name="layers_solid", solid=True),
             ocases.case_instanced(str(tmp_path), name="instanced_solid", masks_override=[np.ones((64, 64), bool), np.ones((3, 5), bool)])]
    for case in solid:
        scene, pt = checks.load(grt, case, 0)
        try:
            masked_materials = [m for m in range(scene.material_count) if scene.material_opacity_map(m) is not None]
            assert masked_materials and all(grt.read_material_opacity(pt.ctx, m).all() for m in masked_materials)
            o, d = (case.origin, case.direction) if case.more_origin is None else (np.concatenate([case.origin, case.more_origin], 1), np.concatenate([case.direction, case.more_direction], 1))
            so, sd = np.repeat(case.origin, 2, 1), np.repeat(case.direction, 2, 1)
            md = np.tile(np.float32([11.2, np.inf]), case.origin.shape[1])

            def run():
                hits, _ = grt.trace_rays(pt.ctx, o, d)
                few, _ = grt.trace_rays(pt.ctx, case.origin, case.direction)
                occluded, _ = grt.trace_shadow_rays(pt.ctx, so, sd, md)
                stream_hits, light, _, info = probe(grt, pt, 1, o, d, so, sd, md)
                return (hits, few, occluded, stream_hits, light), int(info[0])
            masked, kernel = run()
            assert kernel >= KERNEL_GENERAL_MASK
            assert grt.upload_material_opacity(pt.ctx, None, None, None) == 0
            plain, kernel = run()
            assert kernel < KERNEL_GENERAL_MASK
            for a, b in zip(masked, plain):
                assert np.array_equal(a, b), case.name
            assert (checks.unpack(plain[0])[1] >= 0).mean() > 0.3
        finally:
            pt.close(); scene.close()


def test_an_all_zeros_mask_removes_the_instance(grt, tmp_path):
    """instanced with instance 0 under an all-zeros mask against the scene loaded without that instance: t bits, u, v and hit /
    miss of every ray are equal; mesh ids are compared through the instance order."""
    rng_mask = np.random.default_rng(22).random((64, 64))   # (shapes only: the override keeps the case's rays)
    clear = ocases.case_instanced(str(tmp_path), name="instanced_clear", masks_override=[np.zeros(rng_mask.shape, bool), np.random.default_rng(3).random((3, 5)) < 0.5])
    without = ocases.case_instanced(str(tmp_path), name="instanced_clear", masks_override=clear.masks, drop_instance=0)
    assert np.array_equal(clear.origin, without.origin) and np.array_equal(clear.direction, without.direction)
    results = []
    for case in (clear, without):
        scene, pt = checks.load(grt, case, 0)
        try:
            hits, _ = grt.trace_rays(pt.ctx, case.origin, case.direction)
            stream, _, _, _ = probe(grt, pt, 0, case.origin, case.direction, *(np.zeros((3, 0), np.float32),) * 2, np.zeros(0, np.float32))
            assert np.array_equal(hits, stream)
            mesh, tri, _, _, _ = checks.unpack(hits)
            scene_index = np.where(tri >= 0, pt.array("tlas_indices")[np.where(tri >= 0, mesh, 0)], -1)
            results.append((hits, scene_index))
        finally:
            pt.close(); scene.close()
    (a, ia), (b, ib) = results
    assert np.array_equal(a[:, 1:], b[:, 1:])                                  # triangle, t bits, u | v
    hit = checks.unpack(a)[1] >= 0
    assert hit.mean() > 0.1 and (ia[hit] != 0).all() and np.array_equal(ia[hit], ib[hit] + 1)


def test_clearing_the_masks_restores_the_frame(grt, tmp_path):
    """A 32 x 32 cornellbox frame after rt_upload_material_opacity(ctx, NULL, ...) is bit-identical to one rendered before any mask was
    set; with the masks in force it is another frame."""
    rng = np.random.default_rng(8)
    ocases.write_tga(str(tmp_path / "holes.tga"), ocases.mask_image(rng.random((8, 8)) < 0.5, rng))
    grt.config_reset()
    scene = grt.Scene(grt.scene_path("cornellbox"))
    texture = scene.add_texture(str(tmp_path / "holes.tga"), normal_map=True)
    pt = grt.Pathtracer(scene, 32, 32, device=0)
    pt.update()
    lib = grt.device_lib()
    try:
        n = scene.material_count
        assert lib.rt_render_samples(pt.ctx, 0, 2) == 0
        before = pt.read_framebuffer().copy()
        assert grt.upload_material_opacity(pt.ctx, [texture] * n, [3] * n, [0.5] * n) == 0, lib.rt_last_error(pt.ctx)
        assert lib.rt_render_samples(pt.ctx, 0, 2) == 0
        masked = pt.read_framebuffer().copy()
        assert np.isfinite(masked).all() and not np.array_equal(masked, before)
        assert grt.upload_material_opacity(pt.ctx, None, None, None) == 0
        assert lib.rt_render_samples(pt.ctx, 0, 2) == 0
        assert np.array_equal(pt.read_framebuffer(), before)
    finally:
        pt.close(); scene.close()


# ---- 6. frames --------------------------------------------------------------------------------------------------

CHECKER = np.array([[(x + y) % 2 == 0 for x in range(4)] for y in range(4)])


def chamber_scene(directory, name, divider):
    """A closed box cut in two by a horizontal divider at y = 0.5: the emitter above it, the camera and the floor it looks at below.
    divider: "masked" (one quad over the whole cross-section under the 4 x 4 checker mask), "quads" (eight small quads over the
    opaque texels), "quads_split" (the same, every quad split along its other diagonal)."""
    bv, bf = cases.box((-2, -2, -2), (2, 2, 2))
    ocases.write_obj_uv(os.path.join(directory, "box.obj"), bv, np.zeros((8, 2)), bf)
    ocases.write_obj_uv(os.path.join(directory, "lamp.obj"), [(-0.5, 1.9, -0.5), (0.5, 1.9, -0.5), (0.5, 1.9, 0.5), (-0.5, 1.9, 0.5)], np.zeros((4, 2)), [(0, 1, 2), (0, 2, 3)])
    grey = '<bsdf type="diffuse"><rgb name="reflectance" value="0.6, 0.6, 0.6"/></bsdf>'
    shapes = ['<shape type="obj"><string name="filename" value="box.obj"/>%s</shape>' % grey,
              '<shape type="obj"><string name="filename" value="lamp.obj"/><emitter type="area"><rgb name="radiance" value="40, 40, 40"/></emitter></shape>']
    lo, size = -2.5, 1.25                                                     # the divider overlaps the walls; a texel is 1.25 x 1.25
    if divider == "masked":
        ocases.write_tga(os.path.join(directory, "checker.tga"), ocases.mask_image(CHECKER))
        v = [(lo, 0.5, lo), (lo + 4 * size, 0.5, lo), (lo + 4 * size, 0.5, lo + 4 * size), (lo, 0.5, lo + 4 * size)]
        t = [(0, 1), (1, 1), (1, 0), (0, 0)]                                  # the loader's 1 - v: s = (x + 2.5) / 5, t = (z + 2.5) / 5 on the device
        ocases.write_obj_uv(os.path.join(directory, "divider.obj"), v, t, [(0, 1, 2), (0, 2, 3)])
        shapes.append('<shape type="obj"><string name="filename" value="divider.obj"/><bsdf type="mask"><texture name="opacity" type="bitmap">'
                      '<string name="filename" value="checker.tga"/></texture>%s</bsdf></shape>' % grey)
    else:
        v, f = [], []
        for j in range(4):
            for i in range(4):
                if not CHECKER[j, i]:
                    continue
                b = len(v)
                x0, z0 = lo + size * i, lo + size * j
                v += [(x0, 0.5, z0), (x0 + size, 0.5, z0), (x0 + size, 0.5, z0 + size), (x0, 0.5, z0 + size)]
                f += [(b, b + 1, b + 2), (b, b + 2, b + 3)] if divider == "quads" else [(b, b + 1, b + 3), (b + 1, b + 2, b + 3)]
        ocases.write_obj_uv(os.path.join(directory, divider + ".obj"), v, np.zeros((len(v), 2)), f)
        shapes.append('<shape type="obj"><string name="filename" value="%s.obj"/>%s</shape>' % (divider, grey))
    return cases.write_scene(directory, name, shapes, eye="0, -0.25, 1.75", target="0, -2, -0.25")


def test_a_masked_quad_renders_like_its_cut_out_geometry(grt, tmp_path):
    """64 x 64, 16 samples, NEE + MIS: the masked divider against eight small quads over its opaque texels, by the suite's relative
    L1. The bound is what re-tessellation alone costs -- the cut-out scene against itself with every quad split along its other
    diagonal, rendered here -- times two (the mask adds one more source of rounding, at the texel borders), never below
    REL_L1_TOL. The lower chamber is lit only through the holes: every pixel is exactly 0 when the mask is not uploaded, and
    the mean radiance with it is positive."""
    frames = {}
    for name, divider, clear in (("masked", "masked", False), ("unmasked", "masked", True), ("quads", "quads", False), ("quads_split", "quads_split", False)):
        grt.config_reset()
        grt.config_set(num_bounces=4)
        scene = grt.Scene(chamber_scene(str(tmp_path), name, divider))
        scene.set_sky_scale(0.0)   # (a closed box: no ray should see the sky, and none that slips through an edge may bring light)
        grt.config_set(num_bounces=4)
        pt = grt.Pathtracer(scene, 64, 64, device=0)
        pt.update()
        try:
            if clear:
                assert grt.upload_material_opacity(pt.ctx, None, None, None) == 0
            pt.render_samples(16)
            frames[name] = pt.read_framebuffer()[:, :64, :3].astype(np.float64)
        finally:
            pt.close(); scene.close()
    assert all(np.isfinite(f).all() for f in frames.values())
    assert (frames["unmasked"] == 0).all()                                    # no light reaches the lower chamber through a solid divider
    assert frames["masked"].mean() > 0 and (frames["masked"].sum(2) > 0).mean() > 0.5
    rel = lambda got, want: float(np.abs(got - want).sum() / want.sum())
    retessellation = rel(frames["quads_split"], frames["quads"])
    mask = rel(frames["masked"], frames["quads"])
    bound = max(2.0 * retessellation, REL_L1_TOL)
    print("relative L1: masked against cut-out geometry %.3g, cut-out geometry re-tessellated %.3g, bound %.3g" % (mask, retessellation, bound))
    record("frames 64x64x16spp: relative L1 masked vs cut-out geometry %.3g; cut-out geometry vs itself re-tessellated %.3g; bound %.3g; mean radiance below the divider %.4g" % (
        mask, retessellation, bound, frames["masked"].mean()))
    assert mask <= bound, (mask, retessellation, bound)


# ---- 7. Sponza --------------------------------------------------------------------------------------------------

def test_sponza_cut_outs(grt):
    """alpha_masks = 1, 160 x 90, 1 sample, the default flattened layout: the masked materials are exactly those whose albedo file
    is chain_texture.tga or sponza_thorn_diff.tga; the frame is finite; of 5 000 camera-like rays aimed at where the masked
    materials' triangles are, some that hit them without masks now hit something behind; no reported hit on a masked material lies on a
    clear texel (texel-ambiguous hits, at most 2 %, left out). With alpha_masks = 0 no mask is uploaded."""
    from conftest import make_pathtracer
    import re
    scene, pt = make_pathtracer(grt, "sponza", 160, 90, 0)
    try:
        _, _, _, info = probe(grt, pt, 0, *(np.zeros((3, 0), np.float32),) * 4, np.zeros(0, np.float32))
        assert info[0] < KERNEL_GENERAL_MASK
        assert all(scene.material_opacity_map(i) is None for i in range(scene.material_count))
    finally:
        pt.close(); scene.close()

    scene, pt = make_pathtracer(grt, "sponza", 160, 90, 0, alpha_masks=1)
    try:
        text = scene.describe()
        names = {int(l.split()[1]): re.search(r'name="([^"]*)"', l).group(1) for l in text.splitlines() if l.startswith("texture ")}
        albedo = {int(l.split()[1]): int(re.search(r"texture=(-?\d+)", l).group(1)) for l in text.splitlines() if l.startswith("material ")}
        want = {m for m, t in albedo.items() if t >= 0 and os.path.basename(names[t]) in ("chain_texture.tga", "sponza_thorn_diff.tga")}
        got = {m for m in range(scene.material_count) if scene.material_opacity_map(m) is not None}
        assert want and got == want, (sorted(got), sorted(want))
        for m in got:
            assert scene.material_opacity_map(m)[1:] == (3, 0.5)
        pt.render()
        assert np.isfinite(pt.read_framebuffer()).all()
        _, _, _, info = probe(grt, pt, 0, *(np.zeros((3, 0), np.float32),) * 4, np.zeros(0, np.float32))
        assert info[0] == KERNEL_FLAT_SKIP_MASK

        # where the masked materials are: in the flattened layout their triangles are world-space copies that name their instance
        material_of_mesh = pt.array("mesh_material_ids")
        masks = {m: grt.read_material_opacity(pt.ctx, m) for m in got}
        assert all(0.05 < 1.0 - bits.mean() < 0.95 for bits in masks.values())
        staged = pt.array("triangles").reshape(-1, 24)
        alias_mesh = pt.array("alias_mesh_ids")
        copies = np.nonzero((alias_mesh >= 0) & np.isin(material_of_mesh[np.maximum(alias_mesh, 0)], sorted(got)))[0]
        assert copies.size > 1000
        p0, e1, e2 = (staged[copies, k:k + 3].astype(np.float64) for k in (0, 3, 6))
        # 5 000 camera-like rays: from the scene's camera to random points of those triangles
        rng = np.random.default_rng(31)
        eye = np.array(scene.get_camera()[0], np.float64)
        pick = rng.integers(0, copies.size, 5000)
        b = rng.random((2, 5000)); outside = b.sum(0) > 1; b[:, outside] = 1 - b[:, outside]
        targets = (p0[pick] + b[0][:, None] * e1[pick] + b[1][:, None] * e2[pick]).T
        o, d = cases.aim(np.repeat(eye[:, None], 5000, 1).astype(np.float32), targets)
        assert grt.upload_material_opacity(pt.ctx, None, None, None) == 0
        plain, _ = grt.trace_rays(pt.ctx, o, d)
        # ... with the masks back in force (the host's own upload)
        pt.invalidate("materials"); pt.update()
        hits, _ = grt.trace_rays(pt.ctx, o, d)
        pmesh, ptri, pt_t, _, _ = checks.unpack(plain)
        hmesh, htri, ht, _, _ = checks.unpack(hits)
        was_masked = (ptri >= 0) & np.isin(material_of_mesh[np.where(ptri >= 0, pmesh, 0)], sorted(got))
        behind = was_masked & ((htri < 0) | (ht > pt_t))
        assert was_masked.sum() > 1000 and behind.sum() >= 1, (int(was_masked.sum()), int(behind.sum()))
        assert not ((ptri >= 0) & (htri >= 0) & (ht < pt_t)).any()             # a mask only ever lets a ray go further
        # no hit on a clear texel
        idx = np.nonzero((htri >= 0) & np.isin(material_of_mesh[np.where(htri >= 0, hmesh, 0)], sorted(got)))[0]
        assert idx.size > 300
        world = ref.world_triangles_of_hits(staged, pt.array("mesh_transforms"), hmesh[idx], htri[idx])
        _, _, _, _, un, vn, uv_tol, _ = ref.evaluate_named(o[:, idx], d[:, idx], world)
        uv = staged[htri[idx], 18:24].astype(np.float64)
        left_out = 0
        for m, bits in masks.items():
            rows = np.nonzero(material_of_mesh[hmesh[idx]] == m)[0]
            if rows.size == 0:
                continue
            bit, ambiguous = oref.classify(bits, un[rows], vn[rows], uv_tol[rows], uv[rows, 0:2], uv[rows, 2:4], uv[rows, 4:6])
            assert not (~bit & ~ambiguous).any(), (m, int((~bit & ~ambiguous).sum()))
            left_out += int(ambiguous.sum())
        assert left_out <= 0.02 * idx.size, (left_out, idx.size)
        record("sponza 5000 rays at the masked materials: %d hit them without masks, %d of those go on behind with masks; %d hits on masked materials checked, %d left out as texel-ambiguous" % (
            int(was_masked.sum()), int(behind.sum()), idx.size, left_out))
    finally:
        pt.close(); scene.close()
