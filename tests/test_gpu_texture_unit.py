"""The device's software texture unit (rt_shading.h, through rt_sample_texture / rt_sample_table / rt_sample_sky) against the
oracle and against the float64 restatement of DESIGN.md section 5 in texture_reference.py, probe by probe.

Filters 0 and 1 and the LUTs are IEEE fp32 with written-out fmaf and no transcendental function: device and oracle agree to
the bit. Filter 2 forms its lod with log2f, whose device and glibc versions may differ by an ulp: bit-identical where the lod
is exact (power-of-two footprints), within 2e-6 elsewhere. Against the float64 reference: 1e-5 (the fp32 lerp chain on RGBA8
inputs); the sky 2e-4 of its range, as atan2f / acosf place the sample to a few ulp only, and 1e-5 on the six axes."""
import ctypes
from ctypes import byref, c_int, c_int32, c_size_t, c_void_p

import numpy as np
import pytest

import texture_cases as cases
import texture_reference as ref
from texture_reference import F32

pytestmark = pytest.mark.gpu

TOL = 1e-5
GRAD_TOL = 2e-6

RGBA8 = cases.rgba8_textures()
BC1 = cases.bc1_textures()


class TextureDesc(ctypes.Structure):   # rt_texture_desc
    _fields_ = [("texels", c_void_p), ("width", c_int32), ("height", c_int32), ("mip_levels", c_int32),
                ("lod_width", c_int32), ("lod_height", c_int32), ("format", c_int32), ("reserved", c_int32)]


class Context:
    """A bare device context holding `textures` (rt_upload_textures), BC1 decoded at upload or per fetch."""

    def __init__(self, grt, textures, expand=1):
        self.lib = lib = grt.device_lib()
        lib.rt_set_texture_expansion.argtypes = [c_void_p, c_int]
        lib.rt_upload_textures.argtypes = [c_void_p, c_void_p, c_size_t]
        lib.rt_set_sky.argtypes = [c_void_p, c_void_p, c_int, c_int, ctypes.c_float]
        self.ctx = c_void_p()
        assert lib.rt_create(0, byref(self.ctx)) == 0, lib.rt_last_error(None)
        self.textures = list(textures)
        assert lib.rt_set_texture_expansion(self.ctx, expand) == 0
        self.status = self.upload(self.textures)

    def upload(self, textures):
        descs = (TextureDesc * max(len(textures), 1))()
        for d, t in zip(descs, textures):
            d.texels = t.data.ctypes.data; d.width = t.width; d.height = t.height; d.mip_levels = t.mip_levels; d.format = t.format
        return self.lib.rt_upload_textures(self.ctx, descs, len(textures))

    def index(self, tex):
        return next(i for i, t in enumerate(self.textures) if t is tex)

    def close(self):
        self.lib.rt_destroy(self.ctx)


@pytest.fixture(scope="module")
def expanded(grt):
    """RGBA8 textures and BC1 decoded at upload: RtParams::textures_compressed == 0, the `_texels` instantiation."""
    c = Context(grt, RGBA8 + BC1, expand=1)
    assert c.status == 0, c.lib.rt_last_error(c.ctx)
    yield c
    c.close()


@pytest.fixture(scope="module")
def per_fetch(grt):
    """The same textures with the BC1 blocks kept (decoded per fetch): textures_compressed == 1, the other instantiation."""
    c = Context(grt, RGBA8 + BC1, expand=0)
    assert c.status == 0, c.lib.rt_last_error(c.ctx)
    yield c
    c.close()


def _oracle_chain(tex):
    return tex.data if tex.format == 0 else ref.chain_bytes(tex.levels())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare(grt, oracle, context, tex, filter):
    args = cases.all_args(tex)[filter]
    got = grt.sample_texture(context.ctx, context.index(tex), filter, args)
    assert np.isfinite(got).all()
    want_oracle = oracle.tex2d(_oracle_chain(tex), tex.width, tex.height, tex.mip_levels, filter, args)
    same = (_bits(got) == _bits(want_oracle)).all(axis=1)
    if filter in (0, 1):
        bad = np.flatnonzero(~same)
        assert bad.size == 0, "%d of %d probes differ from the oracle, first args %s: device %s oracle %s" % (
            bad.size, same.size, args[bad[0]].tolist(), got[bad[0]].tolist(), want_oracle[bad[0]].tolist())
    else:
        exact = cases.lod_is_exact(tex, args)
        message = "bit-identical to the oracle: %.4f of %d probes (%d with an exact lod)" % (same.mean(), same.size, exact.sum())
        assert exact.sum() > 100, message
        assert same[exact].all(), message + "; an exact-lod probe differs: args %s" % args[exact & ~same][0].tolist()
        assert np.abs(got - want_oracle).max() <= GRAD_TOL, message + "; max |device - oracle| %.3g" % np.abs(got - want_oracle).max()
    want = ref.sample(tex.levels(), tex.width, tex.height, filter, args)
    err = np.abs(got - want).max(axis=1)
    assert err.max() <= TOL, "max |device - float64| %.3g at args %s" % (err.max(), args[err.argmax()].tolist())
    return got


@pytest.mark.parametrize("filter", [0, 1, 2], ids=["level0", "lod", "grad"])
@pytest.mark.parametrize("tex", RGBA8 + BC1, ids=repr)
def test_device_filter_matches_oracle_and_float64_reference(grt, oracle, expanded, tex, filter):
    _compare(grt, oracle, expanded, tex, filter)


@pytest.mark.parametrize("filter", [0, 1, 2], ids=["level0", "lod", "grad"])
@pytest.mark.parametrize("tex", BC1, ids=repr)
def test_per_fetch_bc1_decode_matches_oracle_and_float64_reference(grt, oracle, per_fetch, tex, filter):
    _compare(grt, oracle, per_fetch, tex, filter)


@pytest.mark.parametrize("filter", [0, 1, 2], ids=["level0", "lod", "grad"])
def test_rgba8_gives_the_same_bits_in_both_instantiations(grt, expanded, per_fetch, filter):
    """texture_bilinear<false> (no BC1 block on the device) and <true> (a raw BC1 texture present) on the same RGBA8 texels."""
    for tex in RGBA8:
        args = cases.all_args(tex)[filter]
        a = grt.sample_texture(expanded.ctx, expanded.index(tex), filter, args)
        b = grt.sample_texture(per_fetch.ctx, per_fetch.index(tex), filter, args)
        assert np.array_equal(_bits(a), _bits(b)), tex


@pytest.mark.parametrize("mode", ["expanded", "per_fetch"])
def test_bc1_texel_centres_return_the_numpy_decode(grt, request, mode):
    """Every texel centre of every level of the power-of-two BC1 textures, at lod = the level: kernel_expand_bc1 and the expanded
    addressing (decoded at upload), or bc1_texel per fetch, return exactly the D3D decode of texture_reference."""
    context = request.getfixturevalue(mode)
    for tex in (t for t in BC1 if t.power_of_two):
        levels = tex.levels()
        args, want = [], []
        for l, level in enumerate(levels):
            h, w = level.shape[:2]
            y, x = np.mgrid[0:h, 0:w]
            a = np.zeros((w * h, 8), F32)
            a[:, 0] = (x.reshape(-1) + 0.5) / w; a[:, 1] = (y.reshape(-1) + 0.5) / h; a[:, 2] = l
            args.append(a)
            want.append(level.reshape(-1, 4).astype(F32) * F32(1.0 / 255.0))
        args, want = np.concatenate(args), np.concatenate(want)
        got = grt.sample_texture(context.ctx, context.index(tex), 1, args)
        assert np.array_equal(_bits(got), _bits(want)), (tex, int((_bits(got) != _bits(want)).any(axis=1).sum()))
        assert np.array_equal(np.rint(got * 255).astype(np.uint8), np.concatenate([l.reshape(-1, 4) for l in levels]))


def test_lut_probes_match_oracle_and_float64_reference(grt, oracle, expanded):
    """lut_get_1d / _2d / _3d on the device's own Kulla-Conty tables (rt_read_luts) and on random tables with sides 1, 2 and 7."""
    from conftest import make_pathtracer
    scene, pt = make_pathtracer(grt, "cornellbox", 64, 64, 0)
    try:
        luts = grt.read_luts(pt.ctx)
    finally:
        pt.close(); scene.close(); grt.config_reset()
    real = [luts[0].reshape(16, 16, 16), luts[1].reshape(16, 16, 16), luts[2].reshape(16, 16), luts[3].reshape(16, 16), luts[4].reshape(32, 32), luts[5]]
    assert all(np.abs(t).max() > 0 for t in real)
    for table in real + cases.table_cases():
        coords = cases.table_coords(table.ndim, sides=table.shape[::-1])
        got = grt.sample_table(expanded.ctx, table, coords)
        want_oracle = oracle.lut(table, coords)
        assert np.array_equal(_bits(got), _bits(want_oracle)), (table.shape, int((_bits(got) != _bits(want_oracle)).sum()))
        err = np.abs(got - ref.lut(table, coords))
        assert err.max() <= TOL * max(1.0, float(np.abs(table).max())), (table.shape, err.max(), coords[err.argmax()].tolist())


def test_sky_probes_match_float64_reference(grt, oracle, expanded):
    img = cases.sky_image()
    scale = 1.5
    span = scale * float(img[..., :3].max() - img[..., :3].min())
    assert expanded.lib.rt_set_sky(expanded.ctx, img.ctypes.data, img.shape[1], img.shape[0], scale) == 0
    d = cases.sky_directions()
    got = grt.sample_sky(expanded.ctx, d)
    err = np.abs(got - ref.sky(img, scale, d)).max()
    assert err <= 2e-4 * span, err / span
    assert np.abs(got - oracle.sample_sky(img, scale, d)).max() <= 2e-4 * span
    axes = grt.sample_sky(expanded.ctx, cases.AXES)
    assert np.abs(axes - ref.sky(img, scale, cases.AXES)).max() <= 1e-5 * span, axes


def test_probes_refuse_bad_arguments(grt, expanded):
    with pytest.raises(RuntimeError, match="texture index out of range"):
        grt.sample_texture(expanded.ctx, len(expanded.textures), 0, np.zeros((1, 8)))
    with pytest.raises(RuntimeError, match="texture index out of range"):
        grt.sample_texture(expanded.ctx, -1, 0, np.zeros((1, 8)))
    with pytest.raises(RuntimeError, match="filter must be"):
        grt.sample_texture(expanded.ctx, 0, 3, np.zeros((1, 8)))
    lib = grt.device_lib()
    table, coords, out = np.zeros(4, F32), np.zeros(3, F32), np.zeros(1, F32)
    for dims in (0, 4):
        assert lib.rt_sample_table(expanded.ctx, table.ctypes.data, 2, 2, 1, dims, coords.ctypes.data, 1, out.ctypes.data) != 0
        assert b"dims must be" in lib.rt_last_error(expanded.ctx)
    assert lib.rt_sample_table(expanded.ctx, table.ctypes.data, 0, 2, 1, 2, coords.ctypes.data, 1, out.ctypes.data) != 0
    assert b"table side" in lib.rt_last_error(expanded.ctx)
    fresh = Context(grt, [])
    try:
        assert fresh.status == 0
        with pytest.raises(RuntimeError, match="no sky uploaded"):
            grt.sample_sky(fresh.ctx, cases.AXES)
        with pytest.raises(RuntimeError, match="texture index out of range"):
            grt.sample_texture(fresh.ctx, 0, 0, np.zeros((1, 8)))
    finally:
        fresh.close()
