"""The density grid of the fog volume without a GPU: the float64 reference of fog_density_reference.py (sorted plane crossings, voxels
from midpoints) against closed forms; the voxel march's rules, restated in float32, against that reference inside the bounds derived in
fog_density_cases.py; the gridvolume file; the config key, the command line, the scene and the loader; the new entry points' refusal of a NULL context."""
import ctypes
import math
import os
import struct
import subprocess
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest

import fog_cases as cases
import fog_density_cases as dcases
import fog_density_reference as dref

RT_ERROR_INVALID_ARG = -1
BOX_MIN, BOX_MAX = cases.BOX_MIN, cases.BOX_MAX


def test_a_constant_grid_is_the_homogeneous_length_times_its_value():
    grid = np.full((3, 4, 5), 1.75, np.float32)
    for name, (o, d, t_end) in cases.SEGMENTS.items():
        c = cases_clip(o, d, t_end)
        if c is None:
            continue
        D = dref.density_length(BOX_MIN, BOX_MAX, grid, np.float32(o), np.float32(d), *c)
        assert abs(D - 1.75 * (c[1] - c[0])) <= 1e-12 * (1.0 + abs(c[1])), name


def cases_clip(o, d, t_end):
    import fog_reference as ref
    return ref.clip(BOX_MIN, BOX_MAX, np.float32(o), np.float32(d), np.float32(t_end))


def test_a_slab_stack_sums_its_slabs():
    rho = np.array([0.0, 1e-30, 1.0, 2.5, 0.0, 1e6, 0.25], np.float64)
    grid = rho.astype(np.float32).reshape(7, 1, 1)
    dz = 2.0 / 7.0
    exact = float((grid.reshape(-1).astype(np.float64) * dz).sum())
    # along z, through the whole stack
    assert abs(dref.density_length(BOX_MIN, BOX_MAX, grid, (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 2.0, 4.0) - exact) <= 1e-12 * exact
    # oblique: every slab is crossed over dz / d_z
    d = np.array([0.3, 0.1, 1.0]); d /= np.linalg.norm(d)
    o = np.array([-0.5, 0.0, 0.0])
    c = cases_clip(o, d, math.inf)
    assert abs(dref.density_length(BOX_MIN, BOX_MAX, grid, np.float32(o), np.float32(d), *c) - exact / float(np.float32(d[2]))) <= 1e-6 * exact
    # half way: the first three slabs and half of the fourth
    half = float((rho[:3] * dz).sum() + rho[3] * (1.0 - 3 * dz))
    assert abs(dref.density_length(BOX_MIN, BOX_MAX, grid, (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 2.0, 3.0) - half) <= 1e-12
    # the inversion: where D passes `half`
    pieces = dref.intervals(BOX_MIN, BOX_MAX, grid, (0.1, 0.2, 0.0), (0.0, 0.0, 1.0), 2.0, 4.0)
    t, before, piece = dref.invert(pieces, half)
    assert abs(t - 3.0) <= 1e-12 and piece[2] == 2.5 and abs(before - float((rho[:3] * dz).sum())) <= 1e-12
    assert dref.invert(pieces, 2.0 * exact) is None


def test_a_ray_along_an_axis_sums_its_row():
    grid = dcases.grid("5x4x3")
    c = dcases.cell("5x4x3")
    for j in range(4):
        for k in range(3):
            o = (-3.0, float(BOX_MIN[1] + (j + 0.5) * c[1]), float(BOX_MIN[2] + (k + 0.5) * c[2]))
            D = dref.density_length(BOX_MIN, BOX_MAX, grid, np.float32(o), (1.0, 0.0, 0.0), 2.0, 4.0)
            assert abs(D - float(grid[k, j, :].astype(np.float64).sum() * c[0])) <= 1e-9


@pytest.mark.parametrize("name", dcases.GRID_NAMES)
def test_the_march_rules_in_float32_stay_inside_the_derived_bound(name):
    """The device's rules (fog_density_reference.march32) on every segment, with and without empty-brick skipping: it terminates, and its density length lies
    within the bound of fog_density_cases.py of the float64 reference; skipping reads no voxel of an empty brick."""
    grid = dcases.grid(name)
    worst = 0.0; crossed = 0
    for seg, (o, d, t_end) in dcases.segments(name).items():
        o32, d32 = np.float32(o), np.float32(d)
        c = dref.clip32(BOX_MIN, BOX_MAX, o32, d32, t_end)
        if c is None:
            continue
        pieces = dref.intervals(BOX_MIN, BOX_MAX, grid, o32, d32, c[0], c[1])
        D = sum(rho * (b - a) for a, b, rho, _, _ in pieces if rho > 0)
        bound, _ = dcases.density_length_bound(BOX_MIN, BOX_MAX, grid, o32, d32, float(c[0]), float(c[1]), D, len(pieces))
        for skip in (True, False):
            did, _, got, voxels, bricks_ = dref.march32(BOX_MIN, BOX_MAX, grid, o32, d32, c[0], c[1], skip=skip)
            assert not did and voxels + bricks_ <= sum(grid.shape) + 3
            assert abs(got - D) <= bound + 1e-45, (name, seg, skip, got, D, bound)
            if bound > 0:
                worst = max(worst, abs(got - D) / bound)
            if not skip:
                assert bricks_ == 0
        crossed += 1
    print("%s: %d segments cross the box; worst |D32 - D64| is %.3f of its bound" % (name, crossed, worst))
    assert crossed >= 20


def test_the_shaft_reference_agrees_with_itself_and_with_the_sorted_crossings():
    """The light shaft through a grid dense in one half: the closed-form density length of the two halves against the sorted-crossings reference, and the
    Monte Carlo of the estimator against the quadrature of the single-scatter integral (8 x 8 pixels, 2 048 samples each, 5 standard errors)."""
    import fog_reference as ref
    rho = dcases.SHAFT_HALVES
    grid = np.array(rho, np.float32).reshape(1, 1, 2)
    rng = np.random.default_rng(29)
    for _ in range(50):
        p0, p1 = rng.uniform(BOX_MIN, BOX_MAX), rng.uniform(BOX_MIN, BOX_MAX)
        length = float(np.linalg.norm(p1 - p0))
        want = dref.density_length(BOX_MIN, BOX_MAX, grid, p0, (p1 - p0) / length, 0.0, length)
        assert abs(float(dref.halves_length(0.0, rho, p0[None, :], p1[None, :])[0]) - want) <= 1e-9
    camera_position = np.array([0.0, 0.5, -3.0])
    a = dict(box_min=BOX_MIN, box_max=BOX_MAX, rho=rho, sigma_a=cases.SHAFT["sigma_a"], sigma_s=cases.SHAFT["sigma_s"], g=cases.SHAFT["g"], light=cases.SHAFT_LIGHT, intensity=cases.SHAFT_INTENSITY)
    half = math.tan(math.radians(10.0))
    w = h = 8
    camera = dict(position=camera_position, bottom_left_corner=np.array([-half, -half, 1.0]), x_axis=np.array([2 * half / w, 0, 0]), y_axis=np.array([0, 2 * half / h, 0]))
    want = np.zeros(w * h)
    for jx in (0.25, 0.75):
        for jy in (0.25, 0.75):
            dirs = ref.pixel_rays(camera, w, h, (jx, jy))
            want += np.array([dref.shaft_quadrature_halves(o=camera_position, d=dirs[k], **a) for k in range(w * h)]) / 4.0
    n = 2048
    dirs = ref.pixel_rays(camera, w, h, rng.random((n * w * h, 2)), repeat=n)
    v = dref.shaft_monte_carlo_halves(o=np.broadcast_to(camera_position, dirs.shape), d=dirs, rng=rng, **a).reshape(n, w * h)
    mean, error = v.mean(axis=0), v.std(axis=0, ddof=1) / math.sqrt(n)
    deviation = np.abs(mean - want) / error
    left, right = want.reshape(h, w)[:, :w // 2].mean(), want.reshape(h, w)[:, w // 2:].mean()
    print("shaft through halves %s on the CPU: radiance %.4g .. %.4g (left half %.4g, right half %.4g), worst deviation %.2f standard errors" % (rho, want.min(), want.max(), left, right, deviation.max()))
    assert want.min() > 0 and (deviation > 5.0).sum() == 0 and right > 1.5 * left   # the dense half shines


def test_bricks_are_counted(grt):
    for name in dcases.GRID_NAMES:
        nx, ny, nz = dcases.dims(name)
        total, empty = dref.bricks(dcases.grid(name))
        assert total == -(-nx // 8) * -(-ny // 8) * -(-nz // 8)
        assert 0 <= empty <= total
    assert dref.bricks(dcases.grid("64x64x64")) == (512, 511)
    assert dref.bricks(dcases.grid("9x8x8")) == (2, 1) and dref.bricks(dcases.grid("8x8x9")) == (2, 1)


# ---- the gridvolume file ---------------------------------------------------------------------------------------------------------

def test_the_vol_file_round_trips_and_refuses(grt, tmp_path):
    grid = dcases.grid("17x5x9")
    path = str(tmp_path / "plume.vol")
    grt.write_vol(path, grid, (-1, -0.5, 2, 1, 1.5, 4))
    raw = open(path, "rb").read()
    assert raw[:4] == b"VOL\x03" and struct.unpack("<5i", raw[4:24]) == (1, 17, 5, 9, 1) and struct.unpack("<6f", raw[24:48]) == (-1, -0.5, 2, 1, 1.5, 4)
    assert len(raw) == 48 + 4 * grid.size and np.array_equal(np.frombuffer(raw[48:], np.float32).reshape(9, 5, 17), grid)   # x fastest
    back, box = grt.read_vol(path)
    assert back.shape == (9, 5, 17) and np.array_equal(back, grid) and list(box) == [-1, -0.5, 2, 1, 1.5, 4]

    def refused(name, data, word):
        bad = str(tmp_path / name)
        with open(bad, "wb") as f:
            f.write(data)
        with pytest.raises(RuntimeError) as e:
            grt.read_vol(bad)
        assert name in str(e.value) and word in str(e.value), str(e.value)
    refused("magic.vol", b"VOX" + raw[3:], "VOL")
    refused("version.vol", b"VOL\x02" + raw[4:], "version")
    refused("short_header.vol", raw[:40], "header")
    refused("short.vol", raw[:-4], "shorter")
    refused("encoding.vol", raw[:4] + struct.pack("<i", 2) + raw[8:], "encoding")
    refused("channels.vol", raw[:20] + struct.pack("<i", 3) + raw[24:], "channels")
    refused("dims.vol", raw[:8] + struct.pack("<i", 0) + raw[12:], "dims")
    nan = bytearray(raw); nan[48 + 4 * (17 * 5 + 3):48 + 4 * (17 * 5 + 3) + 4] = struct.pack("<f", math.nan)
    refused("nan.vol", bytes(nan), "cell (3, 0, 1)")
    negative = bytearray(raw); negative[48:52] = struct.pack("<f", -1.0)
    refused("negative.vol", bytes(negative), "cell (0, 0, 0)")
    with pytest.raises(RuntimeError) as e:
        grt.read_vol(str(tmp_path / "missing.vol"))
    assert "missing.vol" in str(e.value)
    with pytest.raises(RuntimeError):
        grt.write_vol(str(tmp_path / "bad.vol"), np.full((1, 1, 1), np.inf, np.float32))


# ---- config, command line, scene ---------------------------------------------------------------------------------------------------

def test_the_config_key_and_the_scene(grt, tmp_path):
    grid = dcases.grid("5x4x3")
    path = str(tmp_path / "grid.vol")
    grt.write_vol(path, grid)
    grt.config_reset()
    try:
        assert grt.config_get("fog_density") == 0.0
        plain = grt.Scene(grt.scene_path("cornellbox"))
        assert plain.fog_density is None and plain.fog is None
        described = plain.describe()
        grt.config_set(fog_density=path)
        assert grt.config_get("fog_density") == 1.0
        with pytest.raises(KeyError):
            grt.config_set(fog_density="")
        assert grt.config_get("fog_density") == 1.0   # a refused value leaves the one before
        scene = grt.Scene(grt.scene_path("cornellbox"))
        assert np.array_equal(scene.fog_density, grid) and scene.fog is None   # a grid without a volume: stored, inert
        assert scene.describe() == described   # the grid stays out of the description
        scene.set_fog((0, 0, 0), (1, 2, 3), 0.5, (1, 2, 4), g=0.25)
        fog = dict(box_min=(0.0, 0.0, 0.0), box_max=(1.0, 2.0, 3.0), sigma_a=(0.5, 0.5, 0.5), sigma_s=(1.0, 2.0, 4.0), g=0.25)
        assert scene.fog == fog   # exactly its five keys, with a grid too
        other = dcases.grid("1x1x7")
        scene.set_fog_density(other)
        assert scene.fog_density.shape == (7, 1, 1) and np.array_equal(scene.fog_density, other) and scene.fog == fog
        for bad in (np.full((1, 1, 1), np.nan), np.full((2, 2, 2), -1.0), np.zeros((1, 1, 1025)), np.full((1, 2, 1), np.inf)):
            with pytest.raises(RuntimeError):
                scene.set_fog_density(bad)
        with pytest.raises(ValueError):
            scene.set_fog_density(np.zeros((2, 2)))
        assert np.array_equal(scene.fog_density, other)   # a refused grid leaves the one before
        scene.clear_fog()
        assert scene.fog is None and np.array_equal(scene.fog_density, other)   # state of its own
        scene.clear_fog_density()
        assert scene.fog_density is None
        grt.config_set(fog_density="off")
        assert grt.config_get("fog_density") == 0.0
        assert grt.Scene(grt.scene_path("cornellbox")).fog_density is None
        grt.config_set(fog_density=str(tmp_path / "nowhere.vol"))
        with pytest.raises(RuntimeError) as e:
            grt.Scene(grt.scene_path("cornellbox"))
        assert "nowhere.vol" in str(e.value)
        scene.close(); plain.close()
    finally:
        grt.config_reset()


def test_help_lists_the_option(grt):
    out = subprocess.run([os.path.join(os.path.dirname(grt.HOST_LIB_PATH), "pathtracer"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    assert "--fog-density" in out


# ---- the loader ------------------------------------------------------------------------------------------------------------------

def _heterogeneous(vol, albedo="0.8", scale="2.5", extra=""):
    return ('<shape type="cube"><transform name="toWorld"><scale x="1" y="2" z="0.5"/><translate x="3" y="0" z="-1"/></transform><bsdf type="null"/>'
            '<medium type="heterogeneous" name="interior"><volume name="density" type="gridvolume"><string name="filename" value="%s"/></volume>'
            '<volume name="albedo" type="constvolume"><spectrum name="value" value="%s"/></volume><float name="scale" value="%s"/>%s'
            '<phase type="hg"><float name="g" value="0.25"/></phase></medium></shape>' % (vol, albedo, scale, extra))


def test_the_loader_turns_a_heterogeneous_null_shape_into_the_fog_with_its_grid(grt, tmp_path, capfd):
    grid = dcases.grid("5x4x3")
    grt.write_vol(str(tmp_path / "smoke.vol"), grid, (2, -2, -1.5, 4, 2, -0.5))
    grt.write_vol(str(tmp_path / "elsewhere.vol"), grid, (0, 0, 0, 1, 1, 1))
    grt.config_reset()
    try:
        bare = grt.Scene(cases.write_fog_shape_scene(tmp_path, "bare", ""))
        path = cases.write_fog_shape_scene(tmp_path, "smoke", _heterogeneous("smoke.vol"))
        # fog_volumes = 0 (the default): the file loads as it always did
        before = grt.Scene(path)
        assert before.fog is None and before.fog_density is None and before.mesh_count == bare.mesh_count + 1
        described = before.describe()
        grt.config_set(fog_volumes=0)
        again = grt.Scene(path)
        assert again.describe() == described and again.fog is None and again.fog_density is None
        # fog_volumes = 1: the box with the grid, and the shape is gone
        grt.config_set(fog_volumes=1)
        capfd.readouterr()
        scene = grt.Scene(path)
        assert "WARNING" not in capfd.readouterr().err   # the file's box is the shape's
        assert scene.mesh_count == bare.mesh_count and scene.describe() == bare.describe()
        fog = scene.fog
        assert fog["box_min"] == (2.0, -2.0, -1.5) and fog["box_max"] == (4.0, 2.0, -0.5) and fog["g"] == 0.25
        assert np.allclose(fog["sigma_s"], (2.0, 2.0, 2.0)) and np.allclose(fog["sigma_a"], (0.5, 0.5, 0.5), atol=1e-6)   # albedo x scale, (1 - albedo) x scale
        assert np.array_equal(scene.fog_density, grid)
        # the file's own box is ignored, with one warning if it differs
        moved = grt.Scene(cases.write_fog_shape_scene(tmp_path, "moved", _heterogeneous("elsewhere.vol")))
        assert capfd.readouterr().err.count("bounding box of the gridvolume file") == 1
        assert moved.fog["box_min"] == (2.0, -2.0, -1.5) and np.array_equal(moved.fog_density, grid)
        # a second volume is refused with its location
        with pytest.raises(RuntimeError) as refused:
            grt.Scene(cases.write_fog_shape_scene(tmp_path, "two", _heterogeneous("smoke.vol") + cases.FOG_SPHERE))
        assert "second fog volume" in str(refused.value) and "two.xml" in str(refused.value)
        # what the medium must have
        for name, xml, word in (("textured", _heterogeneous("smoke.vol").replace('type="constvolume"', 'type="gridvolume"'), "albedo"),
                                ("missing", _heterogeneous("not_there.vol"), "not_there.vol")):
            with pytest.raises(RuntimeError) as e:
                grt.Scene(cases.write_fog_shape_scene(tmp_path, name, xml))
            assert word in str(e.value), str(e.value)
    finally:
        grt.config_reset()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

P, I, Z = c_void_p, c_int, c_size_t
NEW_ENTRY_POINTS = {
    "rt_set_fog_density":      ([P, I, I, I], [None, 1, 1, 1]),
    "rt_get_fog_density_info": ([P, P, P, P, P], [None] * 5),
    "rt_fog_density_segments": ([P, Z, P], [None, 0, None]),
}


@pytest.mark.parametrize("name", sorted(NEW_ENTRY_POINTS))
def test_a_null_context_is_refused_with_the_entry_points_own_message(grt, name):
    lib = ctypes.CDLL(grt.DEVICE_LIB_PATH)
    lib.rt_last_error.restype = ctypes.c_char_p; lib.rt_last_error.argtypes = [c_void_p]
    argtypes, values = NEW_ENTRY_POINTS[name]
    entry = getattr(lib, name)
    entry.restype = c_int; entry.argtypes = [c_void_p] + argtypes
    assert entry(None, *values) == RT_ERROR_INVALID_ARG
    assert lib.rt_last_error(None).decode() == "%s: NULL context" % name


def test_the_header_still_says_17(grt):
    with open(grt.REPO_ROOT + "/include/gpu_raytracer_amd.h") as f:
        header = f.read()
    assert "#define RT_ABI_VERSION 17" in header
    for name in NEW_ENTRY_POINTS:
        assert name + "(" in header
    assert "rt_fog_segments stays the homogeneous step" in header
    assert [n for n in ("set_fog_density", "get_fog_density_info", "fog_density_segments", "read_vol", "write_vol") if not hasattr(grt, n)] == []
