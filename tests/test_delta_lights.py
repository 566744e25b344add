"""Delta emitters on the host, no device: what the scene loader makes of <emitter type="point" / "spot" / "directional">, the
Python scene interface, and the records, selection weights and share the path tracer stages for rt_upload_delta_lights, against the float64
restatement of delta_light_reference.py. (rt_upload_delta_lights' own refusals need a context: test_gpu_delta_lights.py.)"""
import math

import numpy as np
import pytest

import delta_light_cases as cases
import delta_light_reference as ref
from delta_light_reference import POINT, SPOT, DIRECTIONAL


def _load(grt, path, **config):
    grt.config_reset(); grt.config_set(**config)
    return grt.Scene(path)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


@pytest.fixture(autouse=True)
def _reset(grt):
    yield
    grt.config_reset()


def test_each_emitter_type_loads_with_its_defaults(grt, tmp_path):
    xml = ('<emitter type="spot"/>'
           '<emitter type="directional"/>'
           '<emitter type="point"/>'
           '<emitter type="spot"><float name="cutoffAngle" value="40"/></emitter>'
           '<emitter type="directional"><vector name="direction" value="0, -2, 0"/><rgb name="irradiance" value="3, 2, 1"/></emitter>')
    scene = _load(grt, cases.write_floor_scene(tmp_path, xml), delta_lights=1)
    try:
        l = scene.delta_lights()
        assert l.shape == (5, 12)
        assert l[:, 0].tolist() == [SPOT, DIRECTIONAL, POINT, SPOT, DIRECTIONAL]
        # spot: at the origin, along +z, intensity 1, cutoff 20 degrees, beam 3/4 of it
        assert np.array_equal(l[0, 1:4], [0, 0, 0]) and np.array_equal(l[0, 4:7], [0, 0, 1]) and np.array_equal(l[0, 7:10], [1, 1, 1])
        assert l[0, 10] == np.float32(np.float32(20.0) / np.float32(180.0) * np.float32(math.pi)) and abs(l[0, 11] - math.radians(15.0)) < 1e-7
        # directional: travels along +z, irradiance 1; point: at the origin, intensity 1
        assert np.array_equal(l[1, 4:7], [0, 0, 1]) and np.array_equal(l[1, 7:10], [1, 1, 1])
        assert np.array_equal(l[2, 1:4], [0, 0, 0]) and np.array_equal(l[2, 7:10], [1, 1, 1])
        # degrees become radians; the beam follows a given cutoff
        assert abs(l[3, 10] - math.radians(40.0)) < 1e-6 and abs(l[3, 11] - math.radians(30.0)) < 1e-6
        assert np.allclose(l[4, 4:7], [0, -1, 0], atol=1e-7) and np.array_equal(l[4, 7:10], [3, 2, 1])
    finally:
        scene.close()


def test_to_world_lookat_gives_position_and_direction(grt, tmp_path):
    xml = cases.EMITTERS["spot"] + ('<emitter type="directional"><transform name="toWorld"><lookat origin="3, 5, 1" target="1, 0, 2" up="0, 1, 0"/></transform></emitter>'
                                     '<emitter type="point"><transform name="toWorld"><translate x="1.5" y="2.5" z="-3.5"/></transform><rgb name="intensity" value="4, 5, 6"/></emitter>')
    scene = _load(grt, cases.write_floor_scene(tmp_path, xml), delta_lights=1)
    try:
        l = scene.delta_lights().astype(np.float64)
        assert np.allclose(l[0, 1:4], [1.2, 2.5, 0.8], atol=1e-6)
        assert np.allclose(l[0, 4:7], _unit(np.array([-0.3, 0, -0.3]) - [1.2, 2.5, 0.8]), atol=1e-6)
        assert abs(l[0, 10] - math.radians(23.0)) < 1e-6 and abs(l[0, 11] - math.radians(21.0)) < 1e-6
        assert np.allclose(l[1, 4:7], _unit(np.array([1, 0, 2]) - [3, 5, 1]), atol=1e-6)
        assert np.allclose(l[2, 1:4], [1.5, 2.5, -3.5], atol=1e-6) and np.array_equal(l[2, 7:10], [4, 5, 6])
        assert np.allclose(np.linalg.norm(l[:2, 4:7], axis=1), 1.0, atol=1e-6)
    finally:
        scene.close()


def test_point_emitters_stay_icosahedra_unless_asked(grt, tmp_path):
    path = cases.write_floor_scene(tmp_path, cases.EMITTERS["point"])
    as_today = _load(grt, path)
    flagged_off = _load(grt, path, delta_lights=0)
    as_light = _load(grt, path, delta_lights=1)
    try:
        assert grt.config_get("delta_lights") == 1
        assert "PointLight" in as_today.describe() and as_today.describe() == flagged_off.describe()
        assert as_today.delta_lights().shape[0] == 0 and flagged_off.delta_lights().shape[0] == 0
        assert as_today.mesh_count == as_light.mesh_count + 1 and "PointLight" not in as_light.describe()
        l = as_light.delta_lights()
        assert l.shape[0] == 1 and l[0, 0] == POINT and np.array_equal(l[0, 1:4], [1.0, 3.0, 0.5]) and np.array_equal(l[0, 7:10], [30, 28, 25])
    finally:
        as_today.close(); flagged_off.close(); as_light.close()


def test_scenes_without_such_emitters_keep_their_description(grt, tmp_path):
    plain = cases.write_floor_scene(tmp_path, "", name="plain")
    with_lights = cases.write_floor_scene(tmp_path, cases.EMITTERS["spot"] + cases.EMITTERS["directional"], name="lit")
    a, b, c = _load(grt, plain), _load(grt, plain, delta_lights=1), _load(grt, with_lights)
    try:
        assert a.describe() == b.describe() == c.describe()   # (delta lights are kept out of describe(), like normal maps)
        assert a.delta_lights().shape[0] == 0 and c.delta_lights().shape[0] == 2
    finally:
        a.close(); b.close(); c.close()


def test_a_bad_spot_is_ignored_with_a_warning(grt, tmp_path, capfd):
    xml = '<emitter type="spot"><float name="cutoffAngle" value="20"/><float name="beamWidth" value="30"/></emitter>'
    scene = _load(grt, cases.write_floor_scene(tmp_path, xml))
    try:
        assert scene.delta_lights().shape[0] == 0
        assert "beamWidth" in capfd.readouterr().err
    finally:
        scene.close()


def test_scene_interface_adds_and_refuses(grt, tmp_path):
    scene = _load(grt, cases.write_floor_scene(tmp_path, ""))
    try:
        assert scene.add_point_light((1, 2, 3), (4, 5, 6)) == 0
        assert scene.add_spot_light((0, 4, 0), (0, -2, 0), (10, 10, 10), 0.8) == 1
        assert scene.add_directional_light((1, -1, 0), (2, 2, 2)) == 2
        l = scene.delta_lights()
        assert l[:, 0].tolist() == [POINT, SPOT, DIRECTIONAL] and l[1, 10] == np.float32(0.8) and l[1, 11] == np.float32(0.75 * 0.8)
        for call, words in ((lambda: scene.add_spot_light((0, 0, 0), (0, 0, 0), (1, 1, 1), 0.5), "needs a direction"),
                            (lambda: scene.add_spot_light((0, 0, 0), (0, 0, 1), (1, 1, 1), 0.5, 0.6), "0 < beam <= cutoff <= pi"),
                            (lambda: scene.add_spot_light((0, 0, 0), (0, 0, 1), (1, 1, 1), 3.5), "0 < beam <= cutoff <= pi"),
                            (lambda: scene.add_point_light((0, float("nan"), 0), (1, 1, 1)), "not finite"),
                            (lambda: scene.add_directional_light((0, 0, 0), (1, 1, 1)), "needs a direction"),
                            (lambda: scene.add_point_light((0, 0, 0), (1, -1, 1)), "must not be negative")):
            with pytest.raises(ValueError, match=words):
                call()
        assert scene.delta_lights().shape[0] == 3
        scene.clear_delta_lights()
        assert scene.delta_lights().shape[0] == 0
    finally:
        scene.close()


def _scene_radius(pt):
    """Half the diagonal of the box around the scene's instances, from the staged triangles (the floor scene's transforms are baked)."""
    tri = pt.array("triangles").reshape(-1, 24).astype(np.float64)
    p0, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    points = np.concatenate([p0, p0 + e1, p0 + e2])
    return 0.5 * np.linalg.norm(points.max(axis=0) - points.min(axis=0))


@pytest.mark.parametrize("area_light", [False, True], ids=["delta_only", "with_area_light"])
def test_weights_and_share_of_the_staged_records(grt, tmp_path, area_light):
    extra = ('<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="90"/><scale value="0.5"/><translate x="-1" y="4" z="0"/></transform>'
             '<emitter type="area"><rgb name="radiance" value="9, 8, 7"/></emitter></shape>') if area_light else ""
    path = cases.write_floor_scene(tmp_path, "".join(cases.EMITTERS.values()), extra=extra)
    scene = _load(grt, path, delta_lights=1, merge_static=0)
    pt = grt.Pathtracer(scene, 32, 32, device=-1)
    try:
        pt.update()
        records = pt.array("delta_light_records").reshape(-1, grt.DELTA_LIGHT_WORDS)
        lights = scene.delta_lights()
        assert records.shape[0] == 3
        assert np.array_equal(records.view(np.int32)[:, 0], lights[:, 0].astype(np.int32))
        assert np.array_equal(records[:, 1:12], lights[:, 1:12])
        want = ref.weights(lights, _scene_radius(pt))
        # the weights are computed in double and rounded once; the scene's radius comes from float32 boxes (a few ulp of it, squared)
        assert np.allclose(records[:, 12], want, rtol=4e-6, atol=0), (records[:, 12], want)
        assert (records[:, 12] > 0).all()
        total = pt.lights_total_weight
        assert (total > 0) == area_light
        share = ref.automatic_share(records[:, 12], total)
        assert abs(pt.delta_light_share - share) <= 1e-6, (pt.delta_light_share, share)
        if not area_light:
            assert pt.delta_light_share == np.float32(0.95)   # all the power is theirs: the clamp
        grt.config_set(delta_light_share=0.3)
        pt.invalidate("delta_lights"); pt.update()
        assert pt.delta_light_share == np.float32(0.3)
        scene.clear_delta_lights()
        pt.invalidate("delta_lights"); pt.update()
        assert pt.array("delta_light_records").size == 0 and pt.delta_light_share == 0.0
    finally:
        pt.close(); scene.close()


def test_config_keys_are_checked(grt):
    grt.config_reset()
    assert grt.config_get("delta_lights") == 0 and grt.config_get("delta_light_share") == 0
    for bad in (-0.1, 1.5):
        with pytest.raises(KeyError, match="delta_light_share"):
            grt.config_set(delta_light_share=bad)
    grt.config_set(delta_light_share=1.0, delta_lights=1)
    assert grt.config_get("delta_light_share") == 1.0 and grt.config_get("delta_lights") == 1
