"""Light selection of next-event estimation without a GPU: the oracle's pick_light (oracle_sample_lights: sample_light,
sample_triangle, the emitter's point, normal and emission) against the float64 restatement of nee_reference.py, on the light tables
the host stages for the scenes of nee_cases.py; the exact selection probabilities against the staged tables and against 2^20
uniform selections; the rules of rt_upload_lights as the oracle's scene view applies them. The device side is test_gpu_nee.py; the
bounds and what is exact are in nee_checks.py.

Each case prints its worst error against float64; those are the figures in nee_checks.py."""
import numpy as np
import pytest

import nee_cases as cases
import nee_checks as checks
import nee_reference as ref


@pytest.fixture(scope="module")
def loaded(grt, oracle, tmp_path_factory):
    """case name -> (view, tables), each scene loaded once (host only)."""
    cache, open_handles = {}, []

    def get(case):
        if case.name not in cache:
            scene, pt = cases.load(grt, case, tmp_path_factory.mktemp(case.name), -1)
            open_handles.append((scene, pt))
            view = oracle.SceneView(pt)
            cache[case.name] = (view, ref.Tables(view))
        return cache[case.name]
    yield get
    for scene, pt in open_handles:
        pt.close(); scene.close()
    grt.config_reset()


BY_NAME = {c.name: c for c in cases.CPU_CASES}


@pytest.mark.parametrize("case", cases.CPU_CASES, ids=[c.name for c in cases.CPU_CASES])
def test_oracle_selection_matches_float64(loaded, case):
    view, tables = loaded(case)
    assert tables.mesh_cdf.size == case.meshes and tables.triangle_cdf.size == case.triangles, (tables.mesh_cdf.size, tables.triangle_cdf.size)
    assert (tables.mesh_cdf.size <= cases.LIGHT_MESHES_IN_LDS and tables.triangle_cdf.size <= cases.LIGHT_TRIANGLES_IN_LDS) == case.lds
    for what, probes in (("edges", cases.edge_probes(tables)), ("stratified", cases.stratified_probes())):
        got = view.sample_lights(probes)
        checks.compare_with_reference("%s %s" % (case.name, what), got, ref.sample_lights(tables, probes))


def test_the_zero_area_triangle_is_selected_only_at_zero(loaded):
    """few: the strip's first triangle has zero area, so its table entry equals its successor's lower edge, 0. It is the answer only
    to u_triangle = 0, as the span's first entry, and the sample is then refused further on through its NaN normal."""
    view, tables = loaded(BY_NAME["few_merge0"])
    strips = [m for m in range(4) if tables.spans[m, 1] - tables.spans[m, 0] == 5]
    assert len(strips) == 2 and all(tables.triangle_cdf[tables.spans[m, 0]] == 0 for m in strips)
    lower = np.concatenate([[0], tables.mesh_cdf[:-1]]).astype(np.float64)
    for m in strips:
        u_mesh = np.float32((lower[m] + tables.mesh_cdf[m]) / 2)
        tiny = np.float32(np.nextafter(np.float32(0), np.float32(1)))
        got = view.sample_lights(np.array([[u_mesh, 0, 0.3, 0.3], [u_mesh, tiny, 0.3, 0.3]], np.float32))
        ids = checks.ids_of(got)
        degenerate = tables.triangle_indices[tables.spans[m, 0]]
        assert ids[0, 0] == m and ids[0, 2] == degenerate and np.isnan(got[0, 7:10]).all()
        assert ids[1, 0] == m and ids[1, 2] == tables.triangle_indices[tables.spans[m, 0] + 1] and np.isfinite(got[1, 7:10]).all()


@pytest.mark.parametrize("case", cases.CPU_CASES, ids=[c.name for c in cases.CPU_CASES])
def test_staged_tables_hold_the_exact_probabilities(loaded, case):
    """The tables the host stages against luminance * area * scale^2 / W and area_triangle / area_mesh computed from the triangles,
    transforms and materials: float32 entries of a float64 running sum, so 2e-7 absolute (3 float32 half-ulps at 1); the tables end
    in exactly 1 and never decrease; the total weight to 1e-6 relative."""
    view, tables = loaded(case)
    mesh_p, slot_p, weight = ref.exact_probabilities(tables)
    assert abs(tables.total_weight - weight) <= 1e-6 * weight
    assert tables.mesh_cdf[-1] == 1 and (np.diff(tables.mesh_cdf) >= 0).all()
    assert np.abs(np.cumsum(mesh_p) - tables.mesh_cdf).max() <= 2e-7
    for m in range(tables.mesh_cdf.size):
        first, last = tables.spans[m]
        span = tables.triangle_cdf[first:last + 1]
        assert span[-1] == 1 and (np.diff(span) >= 0).all()
        assert np.abs(np.cumsum(slot_p[m]) - span).max() <= 2e-7, m


@pytest.mark.parametrize("name,joint", [("few_merge0", True), ("limit", False)])
def test_oracle_selection_fits_the_distribution(loaded, name, joint):
    view, tables = loaded(BY_NAME[name])
    probes = cases.uniform_probes()
    got = view.sample_lights(probes)
    checks.check_selection_distribution(name, got, tables, joint)
    if name == "few_merge0":
        checks.check_barycentrics(name, got, probes, tables, int(np.argmax(np.diff(np.concatenate([[0], tables.mesh_cdf])))))


def test_scene_view_refuses_tables_the_search_cannot_finish_on(oracle, loaded):
    """The rules of rt_upload_lights in the oracle's scene view (binding.check_light_tables), one table per rule; entries no mesh
    names may hold anything; empty tables are valid."""
    view, tables = loaded(BY_NAME["few_merge0"])
    oracle.check_light_tables(tables.triangle_cdf, tables.mesh_cdf, tables.spans, tables.total_weight)
    for rule, words, _, triangle_cdf, mesh_cdf, spans, _, weight in checks.refused_tables(tables):
        with pytest.raises(ValueError, match=words):
            oracle.check_light_tables(triangle_cdf, mesh_cdf, spans, weight)
    unnamed = np.concatenate([tables.triangle_cdf, np.array([np.nan, 0.5, 0.25], np.float32)])   # a stretch no mesh entry refers to
    oracle.check_light_tables(unnamed, tables.mesh_cdf, tables.spans, tables.total_weight)
    oracle.check_light_tables(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros((0, 2), np.int32), 0.0)
    with pytest.raises(ValueError, match="outside"):
        view.sample_lights(np.array([[0.5, 1.0, 0.5, 0.5]], np.float32))


def test_reference_by_hand():
    """The float64 reference on tables worked out on paper."""
    cdf = np.array([0.0, 0.25, 0.25, 1.0], np.float32)
    u = np.array([0.0, 0.25, np.nextafter(np.float32(0.25), np.float32(1)), 0.1, cases.ONE_BELOW_ONE], np.float32)
    z = np.zeros(u.size, np.int64)
    assert ref.search(cdf, z, z + 3, u).tolist() == [0, 1, 3, 1, 3]         # the first entry >= u; of two equal entries the first
    assert ref.search(cdf, z + 2, z + 3, u).tolist() == [2, 2, 3, 2, 3]     # a span is searched from its own first entry
    a, b = ref.sample_triangle(np.array([0.2, 0.8, 0.5]), np.array([0.6, 0.2, 0.5]))
    assert np.allclose(a, [0.1, 0.7, 0.25]) and np.allclose(b, [0.5, 0.1, 0.25]) and (a + b <= 1).all()
    assert abs(ref.luminance([1, 1, 1]) - 1) < 1e-12
