"""The oracle's software texture unit (oracle/oracle_texture_api.cpp) against the float64 restatement of DESIGN.md section 5 in
texture_reference.py, probe by probe (no GPU). The device side of the same comparison is test_gpu_texture_unit.py."""
import struct

import numpy as np
import pytest

import texture_cases as cases
import texture_reference as ref
from texture_reference import F32

TOL = 1e-5   # RGBA8 inputs: the fp32 lerp chain is a few ulp of 1.0

RGBA8 = cases.rgba8_textures()
BC1 = cases.bc1_textures()


def _oracle_chain(tex):
    """The RGBA8 chain the oracle filters: the texels themselves, or the decoded BC1 levels."""
    return tex.data if tex.format == 0 else ref.chain_bytes(tex.levels())


def _describe(got, want, args):
    err = np.abs(got.astype(np.float64) - want).max(axis=1)
    i = int(err.argmax())
    return "max |err| %.3g at probe %d args %s: got %s want %s" % (err[i], i, args[i].tolist(), got[i].tolist(), want[i].tolist())


@pytest.mark.parametrize("filter", [0, 1, 2], ids=["level0", "lod", "grad"])
@pytest.mark.parametrize("tex", RGBA8 + BC1, ids=repr)
def test_oracle_filter_matches_float64_reference(oracle, tex, filter):
    args = cases.all_args(tex)[filter]
    got = oracle.tex2d(_oracle_chain(tex), tex.width, tex.height, tex.mip_levels, filter, args)
    want = ref.sample(tex.levels(), tex.width, tex.height, filter, args)
    assert np.abs(got - want).max() <= TOL, _describe(got, want, args)


def test_unbatched_oracle_entry_points_agree_with_the_batch(oracle):
    tex = RGBA8[4]   # 37 x 23
    chain = _oracle_chain(tex)
    for filter in (0, 1, 2):
        args = cases.all_args(tex)[filter][::97]
        batch = oracle.tex2d(chain, tex.width, tex.height, tex.mip_levels, filter, args)
        for a, b in zip(args, batch):
            one = oracle.tex2d_one(chain, tex.width, tex.height, tex.mip_levels, filter, a[0], a[1], a[2], a[3:5], a[5:7])
            assert np.array_equal(one.view(np.uint32), b.view(np.uint32))
    table = cases.table_cases()[-1]
    coords = cases.table_coords(3, count=60)
    batch = oracle.lut(table, coords)
    assert [oracle.lut_one(table, *c) for c in coords] == batch.tolist()


def test_reference_by_hand():
    """A few values worked out on paper, so the reference is pinned by more than its own text."""
    level = np.array([[[0, 0, 0, 0], [255, 51, 0, 255]]], np.uint8)   # 2 x 1: black, then (1, 0.2, 0, 1)
    # s = 0: x = -0.5 -> texels -1 (wraps to 1) and 0, half each; s = 0.25: the centre of texel 0; s = 0.5: between 0 and 1
    got = ref.bilinear_wrap(level, np.array([0.0, 0.25, 0.5, 0.75, 1.0], F32), np.zeros(5, F32))
    half = np.array([0.5, 0.1, 0.0, 0.5])
    assert np.allclose(got, [half, [0, 0, 0, 0], half, [1, 0.2, 0, 1], half], atol=1e-15)
    # one BC1 block, c0 = white > c1 = black: indices 0, 1, 2, 3 -> 255, 0, 170, 85; c0 < c1: 0, 255, 127, transparent black
    block = struct.pack("<HHI", 0xffff, 0x0000, 0b11100100)
    dec = ref.bc1_decode_blocks(np.frombuffer(block, np.uint8))[0]
    assert dec[:4, 0].tolist() == [255, 0, 170, 85] and dec[:4, 3].tolist() == [255, 255, 255, 255]
    dec = ref.bc1_decode_blocks(np.frombuffer(struct.pack("<HHI", 0x0000, 0xffff, 0b11100100), np.uint8))[0]
    assert dec[:4].tolist() == [[0, 0, 0, 255], [255, 255, 255, 255], [127, 127, 127, 255], [0, 0, 0, 0]]
    # 5:6:5 bit replication: r = 0b10000 -> 0b10000100 = 132, g = 0b100000 -> 0b10000010 = 130
    dec = ref.bc1_decode_blocks(np.frombuffer(struct.pack("<HHI", (16 << 11) | (32 << 5) | 1, 0, 0), np.uint8))[0]
    assert dec[0].tolist() == [132, 130, 8, 255]
    # anisotropic footprint: 8 x 2 texels -> 4 probes at lod 1; 40 x 1 -> capped at 16 probes, lod log2(40 / 16)
    n, lod, _ = ref.anisotropic_footprint(64, 64, [[8 / 64, 0]], [[0, 2 / 64]])
    assert (n[0], lod[0]) == (4, 1)
    n, lod, _ = ref.anisotropic_footprint(64, 64, [[0, 1 / 64]], [[40 / 64, 0]])
    assert n[0] == 16 and abs(lod[0] - np.log2(2.5)) < 1e-6


@pytest.mark.parametrize("table", cases.table_cases(), ids=lambda t: "x".join(map(str, t.shape[::-1])))
def test_oracle_luts_match_float64_reference(oracle, table):
    coords = cases.table_coords(table.ndim, sides=table.shape[::-1])
    got = oracle.lut(table, coords)
    want = ref.lut(table, coords)
    err = np.abs(got - want)
    assert err.max() <= TOL, (err.max(), coords[err.argmax()].tolist())


def test_oracle_sky_matches_float64_reference(oracle):
    img = cases.sky_image()
    span = float(img[..., :3].max() - img[..., :3].min())
    d = cases.sky_directions()
    got = oracle.sample_sky(img, 1.5, d)
    want = ref.sky(img, 1.5, d)
    assert np.abs(got - want).max() <= 2e-4 * 1.5 * span
    axes = oracle.sample_sky(img, 1.5, cases.AXES)
    assert np.abs(axes - ref.sky(img, 1.5, cases.AXES)).max() <= 1e-5 * 1.5 * span
    # oracle_image_bilinear_clamp is the fetch of sample_sky
    for (x, y, z), c in zip(d[:50], got[:50]):
        u = np.arctan2(-z, x) / (2 * np.pi) + 0.5
        v = np.arccos(np.clip(y, -1, 1)) / np.pi
        assert np.abs(1.5 * oracle.image_bilinear_clamp(img, u, v)[:3] - c).max() <= 2e-4 * 1.5 * span


def _dds(width, height, levels, blocks):
    header = b"DDS " + struct.pack("<IIIIIII", 124, 0x1007 | 0x20000, height, width, 0, 0, levels) + b"\0" * 44 \
        + struct.pack("<II4sIIIII", 32, 4, b"DXT1", 0, 0, 0, 0, 0) + struct.pack("<IIIII", 0x1000, 0, 0, 0, 0)
    return header + blocks.tobytes()


def test_numpy_bc1_decoder_matches_the_hosts(grt, tmp_path):
    """texture_reference.bc1_decode_blocks against BlockCompression::decode_bc1_block (the host's D3D decode), reached through
    Pathtracer.textures() of a scene whose DXT1 .dds textures hold random blocks of all three kinds (c0 > c1, c0 < c1, c0 == c1)."""
    rng = np.random.default_rng(11)
    sizes = [(64, 32), (16, 16), (8, 8), (4, 4)]
    blocks = {}
    for i, (w, h) in enumerate(sizes):
        levels = ref.full_chain_levels(w, h)
        blocks[i] = cases.bc1_blocks(ref.bc1_block_count(w, h, levels), rng)
        (tmp_path / ("t%d.dds" % i)).write_bytes(_dds(w, h, levels, blocks[i]))
    kinds = np.concatenate([(b[:, 1].astype(int) << 8 | b[:, 0]) - (b[:, 3].astype(int) << 8 | b[:, 2]) for b in blocks.values()])
    assert (kinds > 0).sum() > 50 and (kinds < 0).sum() > 50 and (kinds == 0).sum() > 10
    (tmp_path / "s.xml").write_text('<scene version="0.5.0">' + "".join(
        '<shape type="rectangle"><transform name="toWorld"><translate x="%d"/></transform><bsdf type="diffuse"><texture name="reflectance" type="bitmap">'
        '<string name="filename" value="t%d.dds"/></texture></bsdf></shape>' % (3 * i, i) for i in range(len(sizes))) + '</scene>')
    grt.config_reset()
    scene = grt.Scene(str(tmp_path / "s.xml"))
    pt = grt.Pathtracer(scene, 16, 16, device=-1)
    try:
        found = [t for t in pt.textures() if t[1] > 1]
        assert [(w, h) for _, w, h, _ in found] == sizes
        compared = 0
        for i, (texels, w, h, levels) in enumerate(found):
            assert levels >= 1
            mine = ref.bc1_levels(blocks[i][: ref.bc1_block_count(w, h, levels)], w, h, levels)
            host = ref.rgba8_levels(texels, w, h, levels)
            for l in range(levels):
                assert np.array_equal(mine[l], host[l]), (sizes[i], l)
                compared += mine[l].size // 4
        assert compared > 2000
    finally:
        pt.close(); scene.close(); grt.config_reset()
