"""Tangent-space normal maps on the device: normal_map_perturb through rt_perturb_normals against the float64
restatement in normal_map_reference.py, a constant map against the same surface with tilted vertex normals (the oracle-pinned
path), bit-identity of everything a map does not touch, Sponza fully mapped, and the errors of rt_upload_material_normal_maps."""
import ctypes
from ctypes import byref, c_int, c_int32, c_size_t, c_void_p

import numpy as np
import pytest

import normal_map_reference as ref
import texture_cases as cases

pytestmark = pytest.mark.gpu

F32 = np.float32
RT_ERROR_INVALID_ARG = -1
REL_L1_TOL, REL_L2_TOL = 1e-4, 2e-3   # the suite's frame tolerances (tests/test_gpu_full_size.py)


class TextureDesc(ctypes.Structure):   # rt_texture_desc
    _fields_ = [("texels", c_void_p), ("width", c_int32), ("height", c_int32), ("mip_levels", c_int32),
                ("lod_width", c_int32), ("lod_height", c_int32), ("format", c_int32), ("reserved", c_int32)]


MAPS = [cases.rgba8_texture(w, h, 30 + i) for i, (w, h) in enumerate([(1, 1), (16, 8), (37, 23), (64, 64), (256, 16)])]


@pytest.fixture(scope="module", params=["texels", "compressed"])
def probe_ctx(grt, request):
    """A bare context holding the maps: with a BC1 texture kept as blocks beside them (textures_compressed == 1, the COMPRESSED
    instantiation) or without (the _texels one)."""
    lib = grt.device_lib()
    lib.rt_set_texture_expansion.argtypes = [c_void_p, c_int]
    lib.rt_upload_textures.argtypes = [c_void_p, c_void_p, c_size_t]
    ctx = c_void_p()
    assert lib.rt_create(0, byref(ctx)) == 0
    textures = MAPS + ([cases.bc1_texture(8, 8, 5)] if request.param == "compressed" else [])
    assert lib.rt_set_texture_expansion(ctx, 0) == 0
    descs = (TextureDesc * len(textures))()
    for d, t in zip(descs, textures):
        d.texels = t.data.ctypes.data; d.width = t.width; d.height = t.height; d.mip_levels = t.mip_levels; d.format = t.format
    assert lib.rt_upload_textures(ctx, descs, len(textures)) == 0, lib.rt_last_error(ctx)
    yield ctx
    lib.rt_destroy(ctx)


def _records(seed, count, tex):
    """Random hits: triangles (some with mirrored and some with degenerate texture coordinates), instance transforms (rotation,
    uniform scale, translation), rays from both sides and at grazing angles, every filter."""
    rng = np.random.default_rng(seed)
    r = np.zeros((count, ref.PROBE_IN), F32)
    r[:, 0:3] = rng.normal(size=(count, 3))
    r[:, 3:9] = rng.normal(size=(count, 6))
    r[:, 9:12] = rng.normal(size=(count, 3)); r[:, 12:18] = 0.3 * rng.normal(size=(count, 6))
    r[:, 18:20] = rng.random((count, 2)); r[:, 20:24] = rng.normal(size=(count, 4))
    mirrored = rng.random(count) < 0.3
    r[mirrored, 20] *= -1; r[mirrored, 22] *= -1
    degenerate = rng.random(count) < 0.05
    r[degenerate, 22:24] = 2 * r[degenerate, 20:22]
    uv = rng.random((count, 2)); flip = uv.sum(axis=1) > 1; uv[flip] = 1 - uv[flip]
    r[:, 24:26] = uv
    for i in range(count):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        m = np.eye(3, 4) if rng.random() < 0.3 else np.concatenate([rng.uniform(0.2, 3.0) * q, rng.normal(size=(3, 1))], axis=1)
        r[i, 26:38] = m.reshape(12)
    d = rng.normal(size=(count, 3))
    grazing = rng.random(count) < 0.3   # nearly in the triangle's plane: the view guard fires for many of them
    ng = np.cross(np.einsum("nij,nj->ni", r[:, 26:38].reshape(-1, 3, 4)[:, :, :3], r[:, 3:6]),
                  np.einsum("nij,nj->ni", r[:, 26:38].reshape(-1, 3, 4)[:, :, :3], r[:, 6:9]))
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    d[grazing] -= 0.97 * ng[grazing] * np.sum(d[grazing] * ng[grazing], axis=1, keepdims=True)
    r[:, 38:41] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 41] = rng.integers(0, 3, count)
    r[:, 42] = rng.uniform(-8, 2, count)
    scale = rng.uniform(0.2, 4.0, (count, 1)) / np.array([tex.width, tex.height])
    r[:, 43:47] = rng.normal(size=(count, 4)) * np.concatenate([scale, scale], axis=1)
    return r


@pytest.mark.parametrize("tex", MAPS, ids=lambda t: t.name)
def test_probe_matches_the_float64_reference(grt, probe_ctx, tex):
    index = MAPS.index(tex)
    recs = _records(100 + index, 6000, tex)
    got = grt.perturb_normals(probe_ctx, index, recs)
    want, fallback, st = ref.perturb(recs, ref.fetch(tex.levels(), tex.width, tex.height, recs))
    fr = st["frame"]
    length = np.linalg.norm(got[:, :3].astype(np.float64), axis=1)
    assert np.isfinite(got).all() and np.allclose(length, 1.0, atol=1e-5)
    w = -recs[:, 38:41].astype(np.float64)
    cos = np.sum(got[:, :3] * w, axis=1)
    mapped = got[:, 3] == 0.0
    assert (cos[mapped] >= ref.EPS / 2).all()
    # boundaries: the side of the triangle, the frame's fallback rules, the view guard's threshold, short map vectors
    det_rel = np.abs(fr["det"]) / (np.linalg.norm(recs[:, 20:22], axis=1) * np.linalg.norm(recs[:, 22:24], axis=1) + 1e-30)
    side = np.abs(np.sum(w * fr["ng"], axis=1))
    interior = ((fallback & (det_rel == 0)) | (~fallback & (det_rel > 1e-3) & (fr["sin_tn"] > 0.05) & (np.abs(st["cos_view"] - ref.EPS) > 2e-3)
                                               & (st["t_length"] > 0.25))) & (side > 1e-3)
    assert interior.mean() > 0.5 and (interior & st["fired"]).sum() > 20 and (interior & fallback).sum() > 20
    assert (mapped[interior] == ~fallback[interior]).all()
    tol = ref.bound(np.maximum(st["t_length"], 1e-3), np.maximum(np.nan_to_num(fr["sin_tn"], nan=1.0), 1e-3), st["fired"])[interior]
    err = np.abs(got[interior, :3] - want[interior]).max(axis=1)
    assert (err <= tol).all(), (err.max(), np.argmax(err / tol))


def test_probe_refuses_bad_arguments(grt, probe_ctx):
    lib = grt.device_lib()
    rec = _records(1, 1, MAPS[0])
    out = np.zeros(4, F32)
    assert lib.rt_perturb_normals(probe_ctx, len(MAPS) + 5, rec.ctypes.data, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG
    bad = rec.copy(); bad[0, 41] = 3
    assert lib.rt_perturb_normals(probe_ctx, 0, bad.ctypes.data, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG
    assert lib.rt_perturb_normals(probe_ctx, 0, None, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG


# ---- frames -------------------------------------------------------------------------------------------------------------------

C = (160, 110, 230)   # the constant texel: a normal tilted by ~40 degrees
QUAD_OBJ = "v -2 0 -2\nv 2 0 -2\nv 2 0 2\nv -2 0 2\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn %s\nf 1/1/1 3/3/1 2/2/1\nf 1/1/1 4/4/1 3/3/1\n"
MODELS = {
    "diffuse": '<bsdf type="diffuse"><rgb name="reflectance" value="0.7, 0.5, 0.3"/></bsdf>',
    "plastic": '<bsdf type="roughplastic"><rgb name="diffuseReflectance" value="0.3, 0.5, 0.7"/><float name="alpha" value="0.3"/></bsdf>',
    "dielectric": '<bsdf type="roughdielectric"><float name="intIOR" value="1.5"/><float name="alpha" value="0.3"/></bsdf>',
    "conductor": '<bsdf type="roughconductor"><rgb name="eta" value="0.2, 0.9, 1.1"/><rgb name="k" value="3.9, 2.4, 2.1"/><float name="alpha" value="0.3"/></bsdf>',
}
LIGHT = ('<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="90"/><scale value="0.8"/><translate x="-1" y="3" z="1"/></transform>'
         '<emitter type="area"><rgb name="radiance" value="12, 11, 10"/></emitter></shape>')
CAMERA = ('<sensor type="perspective"><float name="fov" value="40"/><transform name="toWorld"><lookat origin="0.5, 6, 1.5" target="0, 0, 0" up="0, 0, -1"/>'
          '</transform></sensor>')


def _quad_scene(tmp_path, tag, bsdf, normal, extra=""):
    (tmp_path / (tag + ".obj")).write_text(QUAD_OBJ % " ".join(repr(float(x)) for x in normal))
    xml = ('<scene version="0.5.0"><integrator type="path"><integer name="maxDepth" value="5"/></integrator>' + CAMERA + LIGHT +
           '<shape type="obj"><string name="filename" value="%s.obj"/>%s</shape>%s</scene>' % (tag, bsdf, extra))
    (tmp_path / (tag + ".xml")).write_text(xml)
    return str(tmp_path / (tag + ".xml"))


def _render(grt, path, scheduler, samples=4, w=96, h=64, prepare=None):
    grt.config_reset()
    scene = grt.Scene(path)
    grt.config_set(enable_next_event_estimation=1, enable_multiple_importance_sampling=1)
    if prepare:
        prepare(scene)
    pt = grt.Pathtracer(scene, w, h, device=0)
    try:
        pt.update()
        grt.set_scheduler(pt.ctx, scheduler)
        lib = grt.device_lib()
        lib.rt_render_samples.argtypes = [c_void_p, c_int, c_int]
        assert lib.rt_render_samples(pt.ctx, 0, samples) == 0, lib.rt_last_error(pt.ctx)
        return pt.read_framebuffer()[:, :w, :3].copy()
    finally:
        pt.close(); scene.close()


def _pixel_l2(got, want):
    d2 = ((got.astype(np.float64) - want) ** 2).sum(axis=2)
    return float(np.sqrt(d2.mean()) / np.sqrt((want.astype(np.float64) ** 2).sum(axis=2).mean()))


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
@pytest.mark.parametrize("model", list(MODELS))
def test_constant_map_equals_tilted_vertex_normals(grt, tmp_path, model, scheduler):
    """A quad with a constant map renders as the same quad whose vertex normals are the vector the texel decodes to. Only camera
    rays reach the quad, and from this camera its mapped normal faces every one of them (the guard does not fire)."""
    ref.write_tga(str(tmp_path / "c.tga"), np.tile(np.array(C, np.uint8), (4, 4, 1)))
    m = ref.constant_map_normal(C)
    nmap = '<bsdf type="normalmap"><texture name="normalmap" type="bitmap"><string name="filename" value="c.tga"/></texture>%s</bsdf>' % MODELS[model]
    mapped = _render(grt, _quad_scene(tmp_path, "mapped", nmap, (0.0, 1.0, 0.0)), scheduler)
    tilted = _render(grt, _quad_scene(tmp_path, "tilted", MODELS[model], m), scheduler)
    assert np.isfinite(mapped).all() and tilted.sum() > 0
    rel = float(np.abs(mapped - tilted).sum() / tilted.sum())
    assert rel < REL_L1_TOL and _pixel_l2(mapped, tilted) < REL_L2_TOL, (rel, _pixel_l2(mapped, tilted))
    plain = _render(grt, _quad_scene(tmp_path, "plain", MODELS[model], (0.0, 1.0, 0.0)), scheduler)
    assert float(np.abs(plain - tilted).sum() / tilted.sum()) > 10 * REL_L1_TOL   # the map does change the picture


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
@pytest.mark.parametrize("model", list(MODELS))
def test_unreached_mapped_material_changes_nothing(grt, tmp_path, model, scheduler):
    """A mapped material of the same slot on a speck no path reaches: the slot runs its _nmap instance, and the frame is bit-identical
    to the one without the map (an unmapped hit inside an _nmap instance runs the plain arithmetic)."""
    ref.write_tga(str(tmp_path / "n.tga"), ref.random_normal_map(3, 16, 16))
    nmap = '<bsdf type="normalmap"><texture name="normalmap" type="bitmap"><string name="filename" value="n.tga"/></texture>%s</bsdf>' % MODELS[model]
    speck = ('<shape type="obj"><string name="filename" value="speck.obj"/><transform name="toWorld"><scale value="0.0001"/><translate x="5000" y="-9000" z="7000"/>'
             '</transform>%s</shape>')
    (tmp_path / "speck.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n")
    with_map = _render(grt, _quad_scene(tmp_path, "a", MODELS[model], (0.3, 1.0, 0.1), speck % nmap), scheduler)
    without = _render(grt, _quad_scene(tmp_path, "b", MODELS[model], (0.3, 1.0, 0.1), speck % MODELS[model]), scheduler)
    assert with_map.sum() > 0 and np.array_equal(with_map, without)


def test_removing_every_map_restores_the_plain_frame(grt, tmp_path):
    """Uploading -1 for every material after maps: bit-identical to a context that never had one."""
    ref.write_tga(str(tmp_path / "n.tga"), ref.random_normal_map(4, 16, 16))
    path = _quad_scene(tmp_path, "q", MODELS["plastic"], (0.0, 1.0, 0.0))
    plain = _render(grt, path, "merged")
    grt.config_reset()
    scene = grt.Scene(path)
    grt.config_set(enable_next_event_estimation=1, enable_multiple_importance_sampling=1)
    t = scene.add_texture(str(tmp_path / "n.tga"), normal_map=True)
    pt = grt.Pathtracer(scene, 96, 64, device=0)
    try:
        lib = grt.device_lib()
        lib.rt_render_samples.argtypes = [c_void_p, c_int, c_int]
        for i in range(scene.material_count):
            scene.set_material_normal_map(i, t)
        pt.update()
        grt.set_scheduler(pt.ctx, "merged")
        assert lib.rt_render_samples(pt.ctx, 0, 4) == 0
        mapped = pt.read_framebuffer()[:, :96, :3].copy()
        assert not np.array_equal(mapped, plain)
        for i in range(scene.material_count):
            scene.set_material_normal_map(i, -1)
        pt.invalidate("materials"); pt.update()
        assert lib.rt_render_samples(pt.ctx, 0, 4) == 0
        assert np.array_equal(pt.read_framebuffer()[:, :96, :3], plain)
    finally:
        pt.close(); scene.close()


def test_upload_errors_leave_the_frame_unchanged(grt, tmp_path):
    ref.write_tga(str(tmp_path / "n.tga"), ref.random_normal_map(5, 16, 16))
    path = _quad_scene(tmp_path, "q", MODELS["diffuse"], (0.0, 1.0, 0.0))
    grt.config_reset()
    scene = grt.Scene(path)
    t = scene.add_texture(str(tmp_path / "n.tga"), normal_map=True)
    for i in range(scene.material_count):
        scene.set_material_normal_map(i, t)
    pt = grt.Pathtracer(scene, 96, 64, device=0)
    try:
        pt.update()
        lib = grt.device_lib()
        lib.rt_render_samples.argtypes = [c_void_p, c_int, c_int]
        assert lib.rt_render_samples(pt.ctx, 0, 2) == 0
        before = pt.read_framebuffer().copy()
        n = scene.material_count
        assert grt.upload_material_normal_maps(pt.ctx, [t] * (n + 1)) == RT_ERROR_INVALID_ARG            # count mismatch
        assert grt.upload_material_normal_maps(pt.ctx, [t + 1000] * n) == RT_ERROR_INVALID_ARG           # no such texture
        assert grt.upload_material_normal_maps(pt.ctx, [-2] * n) == RT_ERROR_INVALID_ARG
        assert lib.rt_upload_material_normal_maps(pt.ctx, None, n) == RT_ERROR_INVALID_ARG              # NULL
        assert lib.rt_render_samples(pt.ctx, 0, 2) == 0
        assert np.array_equal(pt.read_framebuffer(), before)
    finally:
        pt.close(); scene.close()


@pytest.mark.parametrize("svgf", [0, 1])
def test_sponza_fully_mapped_stays_finite(grt, tmp_path, svgf):
    """Sponza at the benchmark's size with a generated map on every material: finite frames, a unit NORMAL AOV."""
    ref.write_tga(str(tmp_path / "n.tga"), ref.random_normal_map(7, 256, 256))
    def prepare(scene):
        t = scene.add_texture(str(tmp_path / "n.tga"), normal_map=True)
        for i in range(scene.material_count):
            scene.set_material_normal_map(i, t)
    grt.config_reset()
    grt.config_set(num_bounces=5)
    scene = grt.Scene(grt.scene_path("sponza"))
    grt.config_set(num_bounces=5, enable_svgf=svgf, enable_taa=svgf)
    prepare(scene)
    pt = grt.Pathtracer(scene, 1920, 1080, device=0)
    try:
        pt.aov_enable(grt.AOV_NORMAL)
        pt.update()
        lib = grt.device_lib()
        for s in range(3):
            assert lib.rt_render_sample(pt.ctx, s) == 0, lib.rt_last_error(pt.ctx)
        frame = pt.read_framebuffer()[:, :1920, :3]
        assert np.isfinite(frame).all() and frame.max() > 0
        lib.rt_render_samples.argtypes = [c_void_p, c_int, c_int]
        assert lib.rt_render_samples(pt.ctx, 0, 1) == 0   # one sample from the start: the accumulated AOV is that sample's
        normal = pt.read_aov(grt.AOV_NORMAL)[:, :1920, :3]
        length = np.linalg.norm(normal.astype(np.float64), axis=2)
        hit = length > 0
        assert np.allclose(length[hit], 1.0, atol=1e-4)
        assert hit.mean() > 0.5 or svgf   # (with SVGF the filter owns the frame's AOVs: only what it leaves is checked)
    finally:
        pt.close(); scene.close()
