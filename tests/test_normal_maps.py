"""Tangent-space normal maps on the CPU: the Mitsuba loader's `normalmap` wrapper and its data textures, and
self-checks of the float64 restatement in normal_map_reference.py that the GPU tests hold the device to."""
import re

import numpy as np
import pytest

import normal_map_reference as ref

F32 = np.float32
RNG_MAP = ref.random_normal_map(11, 16, 8)


def _materials(scene):
    """name -> (index, type, diffuse bits, linear_roughness bits, eta bits, ior bits, texture) from describe()"""
    out = {}
    for line in scene.describe().splitlines():
        if not line.startswith("material "):
            continue
        f = dict(re.findall(r'(\w+)=("[^"]*"|\S+)', line))
        out[f["name"].strip('"')] = dict(index=int(line.split()[1]), type=int(f["type"]), diffuse=f["diffuse"], roughness=f["linear_roughness"],
                                        eta=f["eta"], k=f["k"], ior=f["ior"], texture=int(f["texture"]))
    return out


def _write_scene(tmp_path, bsdfs, shapes):
    (tmp_path / "tri.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n")
    ref.write_tga(str(tmp_path / "n.tga"), RNG_MAP)
    xml = '<scene version="0.5.0">' + "".join(bsdfs)
    for s in shapes:
        xml += '<shape type="obj"><string name="filename" value="tri.obj"/>%s</shape>' % s
    (tmp_path / "s.xml").write_text(xml + "</scene>")
    return str(tmp_path / "s.xml")


NMAP = '<texture name="normalmap" type="bitmap"><boolean name="raw" value="true"/><string name="filename" value="n.tga"/></texture>'
MODELS = {
    "diffuse": '<bsdf type="diffuse"><rgb name="reflectance" value="0.2, 0.4, 0.6"/></bsdf>',
    "plastic": '<bsdf type="roughplastic"><rgb name="diffuseReflectance" value="0.7, 0.1, 0.3"/><float name="alpha" value="0.3"/></bsdf>',
    "conductor": '<bsdf type="roughconductor"><rgb name="eta" value="0.2, 0.9, 1.1"/><rgb name="k" value="3.9, 2.4, 2.1"/><float name="alpha" value="0.15"/></bsdf>',
    "dielectric": '<bsdf type="roughdielectric"><float name="intIOR" value="1.7"/><float name="alpha" value="0.2"/></bsdf>',
}


def _with_id(bsdf, id_):
    return bsdf.replace("<bsdf ", '<bsdf id="%s" ' % id_, 1)


@pytest.mark.parametrize("wrap", ["plain", "inside_twosided", "outside_twosided"])
def test_normalmap_wrapper_keeps_the_wrapped_material(grt, fresh_config, tmp_path, wrap):
    """normalmap(x), twosided(normalmap(x)) and normalmap(twosided(x)) around all four models: each keeps its type, colour and
    parameters (the plain model is loaded beside it for comparison) and gets the map, an RGBA8 data texture whose level 0 is the
    file's bytes even with block compression on."""
    grt.config_set(enable_block_compression=1)
    bsdfs = []
    for name, model in MODELS.items():
        bsdfs.append(_with_id(model, "plain_" + name))
        if wrap == "plain":
            bsdfs.append('<bsdf type="normalmap" id="mapped_%s">%s%s</bsdf>' % (name, NMAP, model))
        elif wrap == "inside_twosided":
            bsdfs.append('<bsdf type="twosided" id="mapped_%s"><bsdf type="normalmap">%s%s</bsdf></bsdf>' % (name, NMAP, model))
        else:
            bsdfs.append('<bsdf type="normalmap" id="mapped_%s">%s<bsdf type="twosided">%s</bsdf></bsdf>' % (name, NMAP, model))
    shapes = ['<ref id="mapped_%s"/>' % n for n in MODELS]
    scene = grt.Scene(_write_scene(tmp_path, bsdfs, shapes))
    try:
        scene.wait_until_loaded()
        mats = _materials(scene)
        maps = set()
        for name in MODELS:
            plain, mapped = mats["plain_" + name], mats["mapped_" + name]
            for key in ("type", "diffuse", "roughness", "eta", "k", "ior"):
                assert plain[key] == mapped[key], (name, key, plain, mapped)
            assert scene.material_normal_map(plain["index"]) == -1
            maps.add(scene.material_normal_map(mapped["index"]))
        assert len(maps) == 1 and -1 not in maps          # one file, one kind: one texture
        t = maps.pop()
        tex = scene.texture(t)
        assert not scene.texture_compressed(t)
        assert (tex["width"], tex["height"]) == (16, 8)
        level0 = tex["texels"][:16 * 8, :3].reshape(8, 16, 3)
        assert np.array_equal(level0, RNG_MAP)
    finally:
        scene.close()


def test_normalmap_around_a_ref_copies_the_material(grt, fresh_config, tmp_path):
    """normalmap(<ref>): a copy of the referenced material carries the map; the original, still used by another shape, does not."""
    bsdfs = [_with_id(MODELS["plastic"], "base"), '<bsdf type="normalmap" id="bumpy">%s<ref id="base"/></bsdf>' % NMAP]
    scene = grt.Scene(_write_scene(tmp_path, bsdfs, ['<ref id="base"/>', '<ref id="bumpy"/>']))
    try:
        scene.wait_until_loaded()
        mats = _materials(scene)
        base, bumpy = mats["base"], mats["bumpy"]
        assert base["index"] != bumpy["index"]
        for key in ("type", "diffuse", "roughness"):
            assert base[key] == bumpy[key]
        assert scene.material_normal_map(base["index"]) == -1
        assert scene.material_normal_map(bumpy["index"]) >= 0
    finally:
        scene.close()


def test_one_file_as_colour_and_normal_map_is_two_textures(grt, fresh_config, tmp_path):
    """The texture cache is keyed on (file, kind): the colour texture is sRGB-decoded, the normal map holds the bytes."""
    colour = '<bsdf type="diffuse"><texture name="reflectance" type="bitmap"><string name="filename" value="n.tga"/></texture></bsdf>'
    bsdfs = ['<bsdf type="normalmap" id="both">%s%s</bsdf>' % (NMAP, colour)]
    scene = grt.Scene(_write_scene(tmp_path, bsdfs, ['<ref id="both"/>']))
    try:
        scene.wait_until_loaded()
        m = _materials(scene)["both"]
        t_colour, t_map = m["texture"], scene.material_normal_map(m["index"])
        assert t_colour >= 0 and t_map >= 0 and t_colour != t_map
        raw = scene.texture(t_map)["texels"][:128, :3].reshape(8, 16, 3)
        decoded = scene.texture(t_colour)["texels"][:128, :3].reshape(8, 16, 3)
        assert np.array_equal(raw, RNG_MAP) and not np.array_equal(decoded, RNG_MAP)
    finally:
        scene.close()


def test_normalmap_without_a_bitmap_loads_the_wrapped_bsdf(grt, fresh_config, tmp_path):
    bsdfs = [_with_id(MODELS["conductor"], "plain"), '<bsdf type="normalmap" id="bare">%s</bsdf>' % MODELS["conductor"]]
    scene = grt.Scene(_write_scene(tmp_path, bsdfs, ['<ref id="bare"/>']))
    try:
        mats = _materials(scene)
        for key in ("type", "eta", "k", "roughness"):
            assert mats["plain"][key] == mats["bare"][key]
        assert scene.material_normal_map(mats["bare"]["index"]) == -1
    finally:
        scene.close()


def test_set_material_normal_map_checks_its_arguments(grt, fresh_config, tmp_path):
    scene = grt.Scene(_write_scene(tmp_path, [_with_id(MODELS["diffuse"], "d")], ['<ref id="d"/>']))
    try:
        t = scene.add_texture(str(tmp_path / "n.tga"), normal_map=True)
        i = _materials(scene)["d"]["index"]
        scene.set_material_normal_map(i, t)
        assert scene.material_normal_map(i) == t
        scene.set_material_normal_map(i, -1)
        assert scene.material_normal_map(i) == -1
        with pytest.raises(RuntimeError):
            scene.set_material_normal_map(i, t + 1)
        with pytest.raises(RuntimeError):
            scene.set_material_normal_map(1000, t)
    finally:
        scene.close()


# ---- the float64 restatement ---------------------------------------------------------------------------------------

def _random_records(seed, count=4000, mirrored=False):
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(count):
        e1, e2 = rng.normal(size=3), rng.normal(size=3)
        n0 = rng.normal(size=3); ne1 = 0.2 * rng.normal(size=3); ne2 = 0.2 * rng.normal(size=3)
        uve1, uve2 = rng.normal(size=2), rng.normal(size=2)
        if mirrored:
            uve1[0], uve2[0] = -uve1[0], -uve2[0]
        u, v = rng.random(), rng.random()
        if u + v > 1:
            u, v = 1 - u, 1 - v
        recs.append(ref.pack(rng.normal(size=3), e1, e2, n0, ne1, ne2, rng.random(2), uve1, uve2, u, v, np.eye(3, 4), rng.normal(size=3), 0))
    return np.array(recs)


def test_reference_returns_unit_normals_in_front_of_the_viewer():
    recs = _random_records(1)
    texel = np.random.default_rng(2).random((len(recs), 4))
    m, fallback, st = ref.perturb(recs, texel)
    assert np.allclose(np.linalg.norm(m, axis=1), 1.0, atol=1e-12)
    w = -recs[:, 38:41] / np.linalg.norm(recs[:, 38:41], axis=1, keepdims=True)
    cos = np.sum(m * w, axis=1)
    assert st["fired"].any() and (cos[~fallback] >= ref.EPS / 2).all()


def test_reference_mirrored_uvs_flip_the_bitangent():
    a, b = _random_records(3, 500), _random_records(3, 500, mirrored=True)
    fa, fb = ref.frame(a), ref.frame(b)
    assert (np.sign(fa["det"]) == -np.sign(fb["det"])).all()
    # mirroring u negates dp/du: T flips, and B = sign(det) cross(n, T) stays -- the handedness of (T, B, n) flips with the uv layout
    assert np.allclose(fa["T"], -fb["T"]) and np.allclose(fa["B"], fb["B"])
    winding = np.where(np.sum(fa["ng"] * fa["n"], axis=1) < 0.0, -1.0, 1.0)
    assert np.allclose(np.sum(np.cross(fa["T"], fa["B"]) * fa["n"], axis=1), np.sign(fa["det"]) * winding)


def test_reference_degenerate_uvs_keep_the_interpolated_normal():
    recs = _random_records(4, 200)
    recs[:100, 22:24] = 2.0 * recs[:100, 20:22]   # uve2 parallel to uve1: det = 0
    recs[100:, 20:24] = 0.0                       # all uvs equal
    texel = np.random.default_rng(5).random((len(recs), 4))
    m, fallback, st = ref.perturb(recs, texel)
    assert fallback.all()
    side = np.where(st["frame"]["entering"], 1.0, -1.0)[:, None]
    assert np.allclose(m, st["frame"]["n"] * side)


def test_reference_instanced_hit_equals_the_transformed_one():
    """A hit on an instance (rotation and uniform scale) equals the hit on the triangle moved to world space."""
    rng = np.random.default_rng(6)
    recs = _random_records(7, 300)
    texel = rng.random((len(recs), 4))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    M = np.zeros((3, 4)); M[:, :3] = 1.7 * q; M[:, 3] = rng.normal(size=3)
    inst = recs.copy(); inst[:, 26:38] = M.reshape(12)
    moved = recs.copy()
    R = M[:, :3]
    for a, b in ((0, 3), (3, 6), (6, 9), (9, 12), (12, 15), (15, 18)):
        moved[:, a:b] = recs[:, a:b] @ R.T
    moved[:, 0:3] += M[:, 3]
    m1, f1, _ = ref.perturb(inst, texel)
    m2, f2, _ = ref.perturb(moved, texel)
    assert (f1 == f2).all() and np.allclose(m1, m2, atol=1e-9)


def test_constant_map_normal_decodes_the_texel():
    c = (150, 90, 230)
    m = ref.constant_map_normal(c)
    t = 2.0 * np.array(c) / 255.0 - 1.0
    want = np.array([t[0], t[2], -t[1]]) / np.linalg.norm(t)
    assert m.dtype == F32 and np.allclose(m, want, atol=1e-6)
