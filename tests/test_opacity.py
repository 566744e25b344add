"""Alpha-tested opacity masks on the CPU: self-checks of the float64 restatement (opacity_reference.py), the
conditions the masked cases (opacity_cases.py) must meet to test anything, the Mitsuba loader's `mask` wrapper, the `alpha_masks`
switch, and the library's ABI."""
import ctypes
import re

import numpy as np
import pytest

import opacity_cases as ocases
import opacity_reference as oref
import trace_reference as ref


@pytest.fixture(scope="module")
def all_cases(tmp_path_factory):
    return ocases.all_cases(str(tmp_path_factory.mktemp("opacity_cases")))


# ---- the reference against hand-computed values -------------------------------------------------------------------

def test_texel_of_wraps_floors_and_keeps_integral_coordinates():
    """W = 4, H = 2: s W = -1.04 -> floor -2 -> texel 2; exactly integral s W starts its texel (1.0 -> 0, 0.25 -> 1, -1.0 -> 0,
    -0.25 -> 3); t H likewise."""
    s = np.array([-0.26, 0.25, 1.0, -1.0, -0.25, 0.999, 2.5, -0.01])
    x, _ = oref.texel_of(s, np.zeros_like(s), 4, 2)
    assert x.tolist() == [2, 1, 0, 0, 3, 3, 2, 3]
    t = np.array([0.0, 0.5, -0.5, 0.49, 1.0, -0.001, 7.75])
    _, y = oref.texel_of(np.zeros_like(t), t, 4, 2)
    assert y.tolist() == [0, 1, 1, 0, 0, 1, 1]
    x, y = oref.texel_of(0.3, 0.9, 1, 1)
    assert (int(x), int(y)) == (0, 0)
    x, y = oref.texel_of(np.array([-1.3, 2.7]), np.array([-1.3, 2.7]), 33, 70)   # -42.9 -> -43 -> 23; 89.1 -> 89 -> 23; -91 -> 49; 189 -> 49
    assert x.tolist() == [23, 23] and y.tolist() == [49, 49]


def test_pack_bits_and_the_cut():
    assert oref.pack_bits(np.ones((3, 5), bool)).tolist() == [0x7fff]          # 15 bits, the tail of the word 0
    m = np.zeros((2, 33), bool); m[0, 0] = m[0, 32] = m[1, 0] = m[1, 32] = True       # bits 0, 32, 33, 65
    assert oref.pack_bits(m).tolist() == [1, 3, 2]
    assert oref.pack_bits(np.ones((1, 32), bool)).tolist() == [0xffffffff] and oref.pack_bits(np.zeros((1, 1), bool)).tolist() == [0]
    assert [oref.cut_of(t) for t in (1 / 255, 0.5, 1.0, 0.25, 1e-9)] == [1, 128, 255, 64, 1]
    rgba = np.zeros((1, 4, 4), np.uint8); rgba[0, :, 3] = [0, 127, 128, 255]; rgba[0, :, 0] = [255, 1, 0, 254]
    assert oref.opaque_of(rgba, 3, 0.5).tolist() == [[False, False, True, True]]
    assert oref.opaque_of(rgba, 0, 1.0).tolist() == [[True, False, False, False]]
    assert oref.opaque_of(rgba, 0, 1 / 255).tolist() == [[True, True, False, True]]


def test_classify_flags_borders_where_the_bit_changes_only():
    """A 4 x 1 mask 1 1 0 0 under uv_0 = 0, edges (1, 0) and (0, 1): u is s. u = 0.125 (mid texel 0) and 0.25 (the border between
    two 1s) are clear; 0.5 + 1e-9 (the border 1 | 0) is ambiguous whichever side; 0.99999999 borders the wrap 0 | 1."""
    mask = np.array([[True, True, False, False]])
    z = np.zeros((5, 2)); e1 = np.tile([1.0, 0.0], (5, 1)); e2 = np.tile([0.0, 1.0], (5, 1))
    u = np.array([0.125, 0.25, 0.5 + 1e-9, 0.5 - 1e-9, 0.99999999])
    bit, amb = oref.classify(mask, u, np.full(5, 0.3), np.full(5, 1e-6), z, e1, e2)
    assert bit.tolist() == [True, True, False, True, False] and amb.tolist() == [False, False, True, True, True]
    # a bound of half a texel or more: anything may come out
    _, amb = oref.classify(mask, u[:1], np.array([0.3]), np.array([0.2]), z[:1], e1[:1], e2[:1])
    assert amb.tolist() == [True]


def test_masked_brute_force_drops_rejected_pairs():
    """Two quads' worth of triangles one behind the other; the front one under an all-zero mask is invisible, under an all-one mask
    it is the hit, and without masks the result is trace_reference.brute_force's."""
    tri = np.array([[(-1, -1, 1), (3, -1, 1), (-1, 3, 1)], [(-1, -1, 2), (3, -1, 2), (-1, 3, 2)]], np.float64)
    o = np.zeros((3, 2), np.float32); d = np.array([[0.0, 0.1], [0.0, 0.05], [1.0, 1.0]], np.float32).T.copy().T
    uv0 = np.zeros((2, 2), np.float32); e1 = np.tile(np.float32([1, 0]), (2, 1)); e2 = np.tile(np.float32([0, 1]), (2, 1))
    which = np.array([0, -1])
    clear, rej = oref.masked_brute_force(o, d, tri, uv0, e1, e2, which, [np.zeros((2, 2), bool)])
    assert clear.index.tolist() == [1, 1] and rej.tolist() == [1, 1] and np.isinf(clear.t_second).all()
    solid, rej = oref.masked_brute_force(o, d, tri, uv0, e1, e2, which, [np.ones((2, 2), bool)])
    plain = ref.brute_force(o, d, tri)
    assert rej.tolist() == [0, 0]
    for name, value in plain.__dict__.items():
        assert np.array_equal(getattr(solid, name), value), name


# ---- conditions on the cases --------------------------------------------------------------------------------------

def test_the_cases_test_something(all_cases):
    """Under the float64 reference alone: at least 95 % of each case's closest-hit rays are robust, and at least 95 % of its shadow
    rays -- of the three of trace_cases.shadow_limits' six per ray that can be: the limits at the float32 hit distance and its two
    neighbours lie within the t bound of the hit BY CONSTRUCTION (they probe the `t < limit` comparison itself and no float64
    rule decides them), so for a ray that hits at most half of the six are robust whatever the seed. In `layers` at least 30 %
    of the robust rays have one or more rejected candidates in front of their hit."""
    for case in all_cases:
        bf, rejected = oref.masked_brute_force(case.origin, case.direction, case.world, case.uv0, case.uve1, case.uve2, case.mask_of_triangle, case.masks)
        robust = ref.robust_closest(bf)
        assert robust.mean() >= 0.95, (case.name, robust.mean())
        _, _, limits = ocases.shadow_rays(case, bf)
        sbf = ref.BruteForce(**{k: np.repeat(v, 6) for k, v in bf.__dict__.items()})
        robust_shadow = ref.robust_shadow(sbf, limits).reshape(-1, 6)
        print("%s: robust closest %.3f, robust shadow by limit %s, rays with rejected candidates in front %.3f" % (
            case.name, robust.mean(), robust_shadow.mean(0).round(3).tolist(), (rejected[robust] > 0).mean()))
        assert robust_shadow[:, [0, 1, 5]].mean() >= 0.95, (case.name, robust_shadow.mean(0))
        if case.name.startswith("layers"):
            assert (rejected[robust] > 0).mean() >= 0.30 and rejected.max() == 6, (case.name, (rejected[robust] > 0).mean(), rejected.max())
        if case.more_origin is not None:
            more, _ = oref.masked_brute_force(case.more_origin, case.more_direction, case.world, case.uv0, case.uve1, case.uve2, case.mask_of_triangle, case.masks)
            assert ref.robust_closest(more).mean() >= 0.95


# ---- the loader ---------------------------------------------------------------------------------------------------

DIFFUSE = '<bsdf type="diffuse"><rgb name="reflectance" value="0.2, 0.4, 0.6"/></bsdf>'
CONDUCTOR = '<bsdf type="roughconductor"><rgb name="eta" value="0.2, 0.9, 1.1"/><rgb name="k" value="3.9, 2.4, 2.1"/><float name="alpha" value="0.15"/></bsdf>'
OPACITY = '<texture name="opacity" type="bitmap"><string name="filename" value="%s"/></texture>'


def _with_id(bsdf, id_):
    return bsdf.replace("<bsdf ", '<bsdf id="%s" ' % id_, 1)


def _material_lines(scene):
    return {re.search(r'name="([^"]*)"', line).group(1): re.sub(r"^material \d+", "", line) for line in scene.describe().splitlines() if line.startswith("material ")}


def _index_of(scene, name):
    for line in scene.describe().splitlines():
        if line.startswith("material ") and 'name="%s"' % name in line:
            return int(line.split()[1])
    raise KeyError(name)


def _write_scene(tmp_path, bsdfs, shapes):
    rng = np.random.default_rng(5)
    (tmp_path / "tri.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n")
    holes = rng.random((6, 9)) < 0.5
    ocases.write_tga(str(tmp_path / "rgba.tga"), ocases.mask_image(holes, rng))
    ocases.write_tga(str(tmp_path / "rgb.tga"), ocases.mask_image(holes, rng)[:, :, :3])
    solid = ocases.mask_image(np.ones((6, 9), bool), rng)
    ocases.write_tga(str(tmp_path / "solid.tga"), solid)                    # four channels, alpha constant
    xml = '<scene version="0.5.0">' + "".join(bsdfs)
    for s in shapes:
        xml += '<shape type="obj"><string name="filename" value="tri.obj"/>%s</shape>' % s
    (tmp_path / "s.xml").write_text(xml + "</scene>")
    return str(tmp_path / "s.xml")


def test_mask_wrapper_records_the_bitmap(grt, fresh_config, tmp_path):
    """mask(x), twosided(mask(x)), mask(twosided(x)) and mask(<ref>): the wrapped material keeps every parameter describe() lists and
    gets the opacity map -- a data texture, channel a for the 4-channel file and r for the 3-channel one, threshold 0.5. Around
    a <ref> a copy carries it; the original does not. describe() never mentions it."""
    bsdfs = [_with_id(DIFFUSE, "plain"),
             '<bsdf type="mask" id="cut">%s%s</bsdf>' % (OPACITY % "rgba.tga", DIFFUSE),
             '<bsdf type="twosided" id="outer"><bsdf type="mask">%s%s</bsdf></bsdf>' % (OPACITY % "rgb.tga", DIFFUSE),
             '<bsdf type="mask" id="inner">%s<bsdf type="twosided">%s</bsdf></bsdf>' % (OPACITY % "rgba.tga", DIFFUSE),
             '<bsdf type="mask" id="copy">%s<ref id="plain"/></bsdf>' % (OPACITY % "rgba.tga")]
    scene = grt.Scene(_write_scene(tmp_path, bsdfs, ['<ref id="%s"/>' % n for n in ("plain", "cut", "outer", "inner", "copy")]))
    try:
        lines = _material_lines(scene)
        text = scene.describe()
        assert "opacity" not in text and "mask" not in text.replace("rgba.tga", "").replace("rgb.tga", "")
        strip = lambda l: re.sub(r'name="[^"]*"', "", l)
        for name in ("cut", "outer", "inner", "copy"):
            assert strip(lines[name]) == strip(lines["plain"]), name
        assert scene.material_opacity_map(_index_of(scene, "plain")) is None
        for name, channel in (("cut", 3), ("outer", 0), ("inner", 3), ("copy", 3)):
            texture, got_channel, threshold = scene.material_opacity_map(_index_of(scene, name))
            assert texture >= 0 and got_channel == channel and threshold == 0.5, name
            assert not scene.texture_compressed(texture)
        assert scene.material_opacity_map(_index_of(scene, "cut"))[0] == scene.material_opacity_map(_index_of(scene, "inner"))[0]   # cached per (file, kind)
    finally:
        scene.close()


def test_mask_without_a_bitmap_is_as_before(grt, fresh_config, tmp_path):
    """A float / rgb opacity, or none: the wrapped BSDF, no map, no extra texture."""
    bsdfs = [_with_id(CONDUCTOR, "plain"),
             '<bsdf type="mask" id="half"><float name="opacity" value="0.5"/>%s</bsdf>' % CONDUCTOR,
             '<bsdf type="mask" id="tint"><rgb name="opacity" value="0.5, 0.5, 0.5"/>%s</bsdf>' % CONDUCTOR,
             '<bsdf type="mask" id="bare">%s</bsdf>' % CONDUCTOR]
    scene = grt.Scene(_write_scene(tmp_path, bsdfs, ['<ref id="%s"/>' % n for n in ("plain", "half", "tint", "bare")]))
    try:
        lines = _material_lines(scene)
        strip = lambda l: re.sub(r'name="[^"]*"', "", l)
        for name in ("half", "tint", "bare"):
            assert strip(lines[name]) == strip(lines["plain"]) and scene.material_opacity_map(_index_of(scene, name)) is None, name
        assert not any(line.startswith("texture ") for line in scene.describe().splitlines())
    finally:
        scene.close()


def _textured(file, id_):
    return '<bsdf type="diffuse" id="%s"><texture name="reflectance" type="bitmap"><string name="filename" value="%s"/></texture></bsdf>' % (id_, file)


def test_alpha_masks_masks_the_materials_whose_file_has_a_varying_alpha(grt, fresh_config, tmp_path):
    """alpha_masks = 1: the material textured with the 4-channel file whose alpha varies gets a mask from it (the file a second
    time, as data; channel 3, threshold 0.5); the 3-channel file and the constant alpha do not; an explicit mask wins; with 0
    (the default) nobody does."""
    bsdfs = [_textured("rgba.tga", "holes"), _textured("rgb.tga", "opaque"), _textured("solid.tga", "constant"),
             '<bsdf type="mask" id="explicit">%s%s</bsdf>' % (OPACITY % "rgb.tga", _textured("rgba.tga", "x").replace(' id="x"', ""))]
    shapes = ['<ref id="%s"/>' % n for n in ("holes", "opaque", "constant", "explicit")]
    path = _write_scene(tmp_path, bsdfs, shapes)
    scene = grt.Scene(path)
    try:
        assert [scene.material_opacity_map(_index_of(scene, n)) is None for n in ("holes", "opaque", "constant", "explicit")] == [True, True, True, False]
    finally:
        scene.close()
    grt.config_set(alpha_masks=1)
    scene = grt.Scene(path)
    try:
        got = {n: scene.material_opacity_map(_index_of(scene, n)) for n in ("holes", "opaque", "constant", "explicit")}
        assert got["opaque"] is None and got["constant"] is None
        texture, channel, threshold = got["holes"]
        assert channel == 3 and threshold == 0.5 and texture != int(re.search(r"texture=(-?\d+)", _material_lines(scene)["holes"]).group(1))
        assert not scene.texture_compressed(texture)
        assert got["explicit"][1] == 0 and got["explicit"][0] != texture      # rgb.tga's red channel, not the albedo's alpha
    finally:
        scene.close()


def test_scene_set_material_opacity_map_checks_its_arguments(grt, fresh_config, tmp_path):
    scene = grt.Scene(_write_scene(tmp_path, [_with_id(DIFFUSE, "d")], ['<ref id="d"/>']))
    try:
        t = scene.add_texture(str(tmp_path / "rgba.tga"), normal_map=True)
        d = _index_of(scene, "d")
        scene.set_material_opacity_map(d, t, channel=1, threshold=0.25)
        assert scene.material_opacity_map(d) == (t, 1, 0.25)
        for bad in (dict(texture=t + 1), dict(texture=-2), dict(texture=t, channel=4), dict(texture=t, threshold=0.0), dict(texture=t, threshold=float("nan"))):
            with pytest.raises(RuntimeError):
                scene.set_material_opacity_map(d, **bad)
        assert scene.material_opacity_map(d) == (t, 1, 0.25)
        scene.set_material_opacity_map(d, -1)
        assert scene.material_opacity_map(d) is None
    finally:
        scene.close()


# ---- the library --------------------------------------------------------------------------------------------------

def test_the_library_exports_the_opacity_entry_points(grt):
    lib = ctypes.CDLL(grt.DEVICE_LIB_PATH)
    assert lib.rt_abi_version() == 17
    assert hasattr(lib, "rt_upload_material_opacity") and hasattr(lib, "rt_read_material_opacity")
    assert callable(grt.upload_material_opacity) and callable(grt.read_material_opacity)
