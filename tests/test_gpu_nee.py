"""Light selection of next-event estimation on the device (rt_sample_lights: the shade kernels' nee_pick_light, sample_light and
sample_triangle on the context's own light tables) against the oracle and the float64 reference of nee_reference.py, on the scenes of
nee_cases.py with the host's TLAS and the device-built one; and rt_upload_lights's refusal of tables the search would not end on.

* Selection is exact: entry, transform id (after the mesh_position remap) and triangle equal the oracle's and searchsorted's on
  every probe -- every table entry, its float neighbours, 0, 0x1.fffffep-1, a stratified 256 x 256 grid.
* The launch that copies the tables into LDS as the shade kernels do and the launch that searches global memory return the same
  bits in every field; the path flag says LDS for `few` and `limit` (64 meshes, 2048 triangles: both limits met) and global for
  `meshes65` and `tris2049`.
* Device against oracle: bit-identical in every field, NaN equal to NaN (nee_checks.py says why). Device against float64: the bounds
  of nee_checks.py, measured on the oracle.
* 2^20 uniform selections fit the exact probabilities of the geometry (one launch per scene).
* rt_upload_lights refuses one table per rule with RT_ERROR_INVALID_ARG and a message, and the tables uploaded before stay in force:
  the frame and the selections after the refusals equal those before. No kernel is ever launched on a refused table.
"""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

import nee_cases as cases
import nee_checks as checks
import nee_reference as ref

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
FIELDS = [0, 1, 2] + list(range(4, 13))   # everything but the path flag and the padding


@pytest.fixture(scope="module")
def loaded(grt, oracle, tmp_path_factory):
    """case name -> (pathtracer, view, tables), each scene loaded once on device 0."""
    cache, open_handles = {}, []

    def get(case):
        if case.name not in cache:
            scene, pt = cases.load(grt, case, tmp_path_factory.mktemp(case.name), 0)
            open_handles.append((scene, pt))
            view = oracle.SceneView(pt)
            cache[case.name] = (pt, view, ref.Tables(view))
        return cache[case.name]
    yield get
    for scene, pt in open_handles:
        pt.close(); scene.close()
    grt.config_reset()


BY_NAME = {c.name: c for c in cases.GPU_CASES}


@pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c.name for c in cases.GPU_CASES])
def test_device_selection_matches_oracle_and_float64(grt, loaded, case):
    pt, view, tables = loaded(case)
    assert tables.mesh_cdf.size == case.meshes and tables.triangle_cdf.size == case.triangles, (tables.mesh_cdf.size, tables.triangle_cdf.size)
    for what, probes in (("edges", cases.edge_probes(tables)), ("stratified", cases.stratified_probes())):
        name = "%s %s" % (case.name, what)
        as_shaded = grt.sample_lights(pt.ctx, probes, use_lds=True)
        from_global = grt.sample_lights(pt.ctx, probes, use_lds=False)
        flag = checks.ids_of(as_shaded)[:, 3]
        assert (flag == (1 if case.lds else 0)).all(), "%s: the launch read %s" % (name, "global memory" if case.lds else "LDS")
        assert (checks.ids_of(from_global)[:, 3] == 0).all(), name
        checks.check_identical(name, as_shaded, from_global, "the global-memory launch", FIELDS)
        want = view.sample_lights(probes)
        checks.check_identical(name, as_shaded, want, "the oracle", FIELDS)
        checks.check_identical(name, from_global, want, "the oracle", FIELDS)
        checks.compare_with_reference(name, as_shaded, ref.sample_lights(tables, probes))


@pytest.mark.parametrize("name,joint", [("few_merge0", True), ("limit", False), ("limit_device_tlas", False)])
def test_device_selection_fits_the_distribution(grt, loaded, name, joint):
    pt, view, tables = loaded(BY_NAME[name])
    probes = cases.uniform_probes()
    got = grt.sample_lights(pt.ctx, probes, use_lds=True)
    checks.check_selection_distribution(name, got, tables, joint)
    if joint:
        checks.check_barycentrics(name, got, probes, tables, int(np.argmax(np.diff(np.concatenate([[0], tables.mesh_cdf])))))


def _frame(grt, pt):
    lib = grt.device_lib()
    assert lib.rt_render_sample(pt.ctx, 0) == 0, lib.rt_last_error(pt.ctx)
    return pt.read_framebuffer().copy()


def test_upload_refuses_tables_the_search_cannot_finish_on(grt, loaded):
    pt, view, tables = loaded(BY_NAME["few_merge0"])
    lib = grt.device_lib()
    probes = cases.stratified_probes(64)
    before = _frame(grt, pt)
    picked = grt.sample_lights(pt.ctx, probes)
    assert before[..., :3].max() > 0
    for rule, words, triangle_indices, triangle_cdf, mesh_cdf, spans, transform_indices, weight in checks.refused_tables(tables):
        status = grt.upload_lights(pt.ctx, triangle_indices, triangle_cdf, mesh_cdf, spans, transform_indices, weight)
        message = lib.rt_last_error(pt.ctx).decode()
        assert status == RT_ERROR_INVALID_ARG and "rt_upload_lights" in message and words in message, (rule, status, message)
    # the tables uploaded before are still in force
    assert np.array_equal(_frame(grt, pt), before)
    assert np.array_equal(grt.sample_lights(pt.ctx, probes).view(np.uint32), picked.view(np.uint32))
    # what the host stages uploads, also with a stretch of the triangle table that no mesh entry names and that holds NaN
    good = (tables.triangle_indices, tables.triangle_cdf, tables.mesh_cdf, tables.spans, tables.transform_indices, tables.total_weight)
    extra = (np.concatenate([good[0], np.zeros(3, np.int32)]), np.concatenate([good[1], np.array([np.nan, 0.5, 0.25], np.float32)])) + good[2:]
    for t in (extra, good):
        assert grt.upload_lights(pt.ctx, *t) == 0, lib.rt_last_error(pt.ctx)
        assert np.array_equal(grt.sample_lights(pt.ctx, probes).view(np.uint32), picked.view(np.uint32))
    assert np.array_equal(_frame(grt, pt), before)


def test_empty_tables_stay_valid_and_probes_refuse_bad_arguments(grt, loaded):
    pt, view, tables = loaded(BY_NAME["few_merge0"])
    lib = grt.device_lib()
    good = np.array([[0.5, 0.5, 0.5, 0.5]], np.float32)
    out = np.zeros((1, grt.LIGHT_SAMPLE_OUT), np.float32)
    assert lib.rt_sample_lights(pt.ctx, None, 1, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG
    assert lib.rt_sample_lights(pt.ctx, good.ctypes.data, 1, 1, None) == RT_ERROR_INVALID_ARG
    assert lib.rt_sample_lights(pt.ctx, good.ctypes.data, (1 << 24) + 1, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG and b"2^24" in lib.rt_last_error(pt.ctx)
    assert lib.rt_sample_lights(pt.ctx, good.ctypes.data, 1, 2, out.ctypes.data) == RT_ERROR_INVALID_ARG
    for column, value in ((0, 1.0), (1, 1.0), (1, -0.25), (0, np.nan), (3, 1.5)):   # the searches end only for numbers below the tables' last entry
        bad = good.copy(); bad[0, column] = value
        with pytest.raises(RuntimeError, match=r"outside \[0, 1\)"):
            grt.sample_lights(pt.ctx, bad)
    assert grt.sample_lights(pt.ctx, np.zeros((0, 4), np.float32)).shape == (0, grt.LIGHT_SAMPLE_OUT)

    ctx = c_void_p()   # a context without emitters: empty tables upload, and the probe says so instead of searching them
    assert lib.rt_create(0, byref(ctx)) == 0, lib.rt_last_error(None)
    try:
        assert lib.rt_sample_lights(ctx, good.ctypes.data, 1, 1, out.ctypes.data) == RT_ERROR_NOT_READY and b"no lights" in lib.rt_last_error(ctx)
        assert lib.rt_upload_lights(ctx, None, None, 0, None, None, None, 0, 0.0) == 0, lib.rt_last_error(ctx)
        assert lib.rt_sample_lights(ctx, good.ctypes.data, 1, 1, out.ctypes.data) == RT_ERROR_NOT_READY and b"no lights" in lib.rt_last_error(ctx)
    finally:
        lib.rt_destroy(ctx)
