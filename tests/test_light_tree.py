"""The light tree without a device: the restatements of light_tree_reference.py against themselves on the scenes of light_tree_cases.py, and the
plumbing -- config key, command line, Python, the loader's entry points and their refusal of a NULL context.

The restatement against itself, for every case: the float32 tree holds every leaf once, its root's Phi is the sum of the leaves' within depth roundings, an inner node's
box holds the boxes of its children of positive Phi and nothing of the others; leaf A and Phi lie within the derived bounds of float64; on the grid the pmfs of all leaves
sum to 1 within the bound derived from depth, the float32 pmf lies within pmf_bound of float64 (and the grid keeps rho, the relative error of an importance, below 1/4,
where the first-order bound means something), what the descent reports is the pmf of the leaf it arrives at, bit for bit, and it never arrives at a leaf without power;
2^16 equally spaced u select every leaf 2^16 pmf times within selection_tolerance. A wrong rescale or comparison in the restatement would fail the last; the device
is then held to the restatement bit for bit (test_gpu_light_tree.py).
"""
import ctypes
import os
import subprocess
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest

import light_tree_cases as cases
import light_tree_reference as ref

RT_ERROR_INVALID_ARG = -1
F = np.float32


@pytest.fixture(scope="module")
def trees():
    cache = {}

    def get(name):
        if name not in cache:
            s = cases.scene(name)
            cache[name] = (s, ref.build32(s))
        return cache[name]
    return get


@pytest.mark.parametrize("name", cases.NAMES)
def test_restated_tree_is_a_tree_over_every_leaf(trees, name):
    s, t = trees(name)
    n, m, lv = t.leaf_count, t.padded, t.leaves
    assert m >= n and m & (m - 1) == 0 and (m == 1 or m // 2 < n)
    assert np.array_equal(np.sort(t.order), np.arange(n)) and np.array_equal(t.slot_of_leaf[t.order], m - 1 + np.arange(n))
    assert (np.diff(t.keys[t.order].astype(object)) > 0).all(), "the keys are not strictly increasing along the order"
    total = lv.power.astype(np.float64).sum()
    assert abs(float(t.nodes[0, 3]) - total) <= t.depth * ref.EPS * total + 1e-300
    for i in range(m - 1):
        lo, hi = t.nodes[i, 0:3], t.nodes[i, 4:7]
        for c in (2 * i + 1, 2 * i + 2):
            if t.nodes[c, 3] > 0:
                assert (lo <= t.nodes[c, 0:3]).all() and (hi >= t.nodes[c, 4:7]).all()
        live = [c for c in (2 * i + 1, 2 * i + 2) if t.nodes[c, 3] > 0]
        if live:
            assert np.array_equal(lo, np.min([t.nodes[c, 0:3] for c in live], 0)) and np.array_equal(hi, np.max([t.nodes[c, 4:7] for c in live], 0))
        else:
            assert t.nodes[i, 3] == 0 and (lo > hi).all()
    area, power, area_bound, power_bound = ref.leaves64(s)
    assert (np.abs(lv.area - area) <= area_bound).all() and (np.abs(lv.power - power) <= power_bound).all()


def test_world_area_is_the_true_area_under_a_non_uniform_scale(trees):
    s, t = trees("instanced")
    area = t.leaves.area.astype(np.float64)
    assert np.allclose(area[8:16], 4.0 * area[0:8], rtol=1e-5)                       # scaled 2 x: area x 4
    assert not np.allclose(area[16:24], 3.0 * area[0:8], rtol=1e-2)                   # (1, 3, 0.5): no single factor ...
    m = s.transforms[2, :, :3].astype(np.float64)
    tri = s.triangles[:8].astype(np.float64)
    true = 0.5 * np.linalg.norm(np.cross(tri[:, 3:6] @ m.T, tri[:, 6:9] @ m.T), axis=1)   # ... but half the cross product of the transformed edges
    assert np.allclose(area[16:24], true, rtol=1e-5)


@pytest.mark.parametrize("name", cases.NAMES)
def test_restated_pmf_sums_to_one_and_agrees_with_float64(trees, name):
    s, t = trees(name)
    for point in cases.grid(t, t.leaves):
        pts = np.broadcast_to(point, (t.leaf_count, 3))
        pmf = ref.pmf32(t, pts, t.slot_of_leaf)
        assert abs(float(pmf.astype(np.float64).sum()) - 1.0) <= ref.sum_bound(t), (name, point.tolist())
        p64, bound, rho = ref.pmf64(t, pts, t.slot_of_leaf)
        assert rho < 0.25 and abs(p64.sum() - 1.0) < 1e-12
        assert (np.abs(pmf - p64) <= bound).all(), (name, point.tolist(), float(np.max(np.abs(pmf - p64) / bound)))
        assert (pmf[t.leaves.power == 0] == 0).all()


@pytest.mark.parametrize("name", cases.NAMES)
def test_restated_descent_reports_the_pmf_of_its_leaf(trees, name):
    s, t = trees(name)
    rng = np.random.default_rng(9)
    edge = np.array([0.0, ref.ONE_BELOW_ONE, 0.5, 2.0 ** -24], F)
    u = np.concatenate([np.repeat(edge, edge.size), np.minimum(rng.random(500, F), ref.ONE_BELOW_ONE)])
    u2 = np.concatenate([np.tile(edge, edge.size), np.minimum(rng.random(500, F), ref.ONE_BELOW_ONE)])
    leaf_of_slot = np.full(2 * t.padded - 1, -1); leaf_of_slot[t.slot_of_leaf] = np.arange(t.leaf_count)
    for point in cases.grid(t, t.leaves):
        pts = np.broadcast_to(point, (u.size, 3))
        slot, pmf = ref.sample32(t, pts, u, u2)
        leaf = leaf_of_slot[slot]
        assert (leaf >= 0).all() and (t.leaves.power[leaf] > 0).all() and (pmf > 0).all()
        assert np.array_equal(pmf.view(np.uint32), ref.pmf32(t, pts, slot).view(np.uint32))


@pytest.mark.parametrize("name", ["n65", "n257"])
def test_restated_selection_counts_follow_the_pmf(trees, name):
    s, t = trees(name)
    u = (np.arange(1 << 16) / 65536.0).astype(F)
    leaf_of_slot = np.full(2 * t.padded - 1, -1); leaf_of_slot[t.slot_of_leaf] = np.arange(t.leaf_count)
    for point in cases.grid(t, t.leaves)[[0, 3, 4, 6]]:
        slot, _ = ref.sample32(t, np.broadcast_to(point, (u.size, 3)), u, F(0.5))
        counts = np.bincount(leaf_of_slot[slot], minlength=t.leaf_count)
        pmf = ref.all_pmfs(t, point).astype(np.float64)
        assert np.max(np.abs(counts - 65536.0 * pmf)) <= ref.selection_tolerance(t), (name, point.tolist())


def test_the_tree_beats_power_selection_where_lights_are_many_and_far_apart(trees):
    """What the frame test on the device predicts its noise ratio from: the variance the selection adds to direct light under a row of equal lamps."""
    n = 32
    tri = cases._triangles(np.stack([np.arange(n) * 4.0, np.full(n, 2.0), np.zeros(n)], 1), np.tile([[0.5, 0, 0]], (n, 1)), np.tile([[0, 0, 0.5]], (n, 1)))
    s = cases._scene({"datas": [tri], "use": [0]}, [(10, 10, 10)], [cases._matrix()])
    t = ref.build32(s)
    c, by_power, by_tree = ref.emitter_pdfs(s, t, (0.25, 0.0, 0.25))
    assert abs(by_power.sum() - 1) < 1e-12 and abs(by_tree.sum() - 1) < 1e-6
    assert ref.selection_variance(c, by_tree) < 0.1 * ref.selection_variance(c, by_power)


def test_restated_estimators_agree_within_the_share_the_frame_test_allows(grt, tmp_path):
    """What test_gpu_light_tree.py's tree-on-against-off frame test allows -- at most 5 % of the pixels with means more than 4 standard errors of their difference apart,
    at 48 samples -- holds for the float64 restatement of the two estimators alone (selection by power, selection by the tree, the triangle's centroid for its points)
    at the floor points of that frame; and the tree's predicted variance is the lower one."""
    path = cases.write_many_lights(tmp_path)
    grt.config_reset(); grt.config_set(num_bounces=2)
    scene = grt.Scene(path); pt = grt.Pathtracer(scene, 64, 64, device=-1); pt.update()
    try:
        s = cases.scene_from_pathtracer(pt); t = ref.build32(s)
        assert t.leaf_count == 512
        xs, ys, points = cases.floor_points(pt.camera(), 64, 64, 4)
        assert len(points) > 150
        rng = np.random.default_rng(2)
        outside = 0; by = [0.0, 0.0]
        for point in points:
            c, by_power, by_tree = ref.emitter_pdfs(s, t, point)
            by[0] += ref.selection_variance(c, by_power); by[1] += ref.selection_variance(c, by_tree)
            m0, e0 = cases.simulate_selection(c, by_power, 48, rng); m1, e1 = cases.simulate_selection(c, by_tree, 48, rng)
            outside += abs(m1 - m0) > 4.0 * np.sqrt(e0 * e0 + e1 * e1)
        assert outside <= 0.05 * len(points), (outside, len(points))
        assert by[1] < 0.5 * by[0], by
    finally:
        pt.close(); scene.close(); grt.config_reset()


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------

def test_config_key_round_trips_and_rejects_other_values(fresh_config):
    grt = fresh_config
    assert grt.config_get("light_tree") == 0
    grt.config_set(light_tree=1)
    assert grt.config_get("light_tree") == 1
    with pytest.raises(KeyError, match="light_tree must be 0 or 1"):
        grt.config_set(light_tree=2)
    assert grt.config_get("light_tree") == 1
    grt.config_reset()
    assert grt.config_get("light_tree") == 0


def test_pathtracer_switch_sets_the_key_and_a_host_only_update_accepts_it(fresh_config):
    grt = fresh_config
    scene = grt.Scene(grt.scene_path("cornellbox"))
    pt = grt.Pathtracer(scene, 16, 16, device=-1)
    try:
        pt.set_light_tree(True)
        assert grt.config_get("light_tree") == 1
        pt.update()
        pt.set_light_tree(False)
        assert grt.config_get("light_tree") == 0
    finally:
        pt.close(); scene.close()


def test_help_lists_the_option(grt):
    out = subprocess.run([os.path.join(os.path.dirname(grt.HOST_LIB_PATH), "pathtracer"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    assert "--light-tree" in out


def test_python_names_and_the_header(grt):
    for name in ("set_light_tree", "read_light_tree", "sample_light_tree", "light_tree_pmf"):
        assert callable(getattr(grt, name))
    assert callable(grt.Pathtracer.set_light_tree) and grt.MAX_LIGHT_TREE_LEAVES == 1 << 22
    with open(grt.REPO_ROOT + "/include/gpu_raytracer_amd.h") as f:
        header = f.read()
    assert "#define RT_ABI_VERSION 17" in header and "#define RT_MAX_LIGHT_TREE_LEAVES (1 << 22)" in header
    for name in ("rt_set_light_tree", "rt_get_light_tree", "rt_read_light_tree", "rt_sample_light_tree", "rt_light_tree_pmf"):
        assert "int %s(" % name in header


P, I, Z = c_void_p, c_int, c_size_t
ENTRY_POINTS = {
    "rt_set_light_tree":    ([I], [1], "rt_set_light_tree: NULL context"),
    "rt_read_light_tree":   ([P, P, P, Z, P, P, Z, P, Z, P, Z], [None, None, None, 0, None, None, 0, None, 0, None, 0], "rt_read_light_tree: NULL context"),
    "rt_sample_light_tree": ([P, Z, P], [None, 0, None], "rt_sample_light_tree: NULL argument"),
    "rt_light_tree_pmf":    ([P, Z, P], [None, 0, None], "rt_light_tree_pmf: NULL argument"),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_a_null_context_is_refused_without_a_device(grt, name):
    lib = ctypes.CDLL(grt.DEVICE_LIB_PATH)
    lib.rt_last_error.restype = ctypes.c_char_p; lib.rt_last_error.argtypes = [c_void_p]
    argtypes, values, message = ENTRY_POINTS[name]
    entry = getattr(lib, name)
    entry.restype = c_int; entry.argtypes = [c_void_p] + argtypes
    assert entry(None, *values) == RT_ERROR_INVALID_ARG
    assert lib.rt_last_error(None).decode() == message
    lib.rt_get_light_tree.argtypes = [c_void_p]
    assert lib.rt_get_light_tree(None) == 0
