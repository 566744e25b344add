"""The oracle's traversal against a float64 brute force on small adversarial scenes (tests/trace_cases.py), for the CWBVH with
the skipping walk on and off, the TLAS layout, the binary and the 4-wide BVH. CPU only; the GPU half is test_gpu_trace_stream.py.

Prints, per case and walk, the robust fraction of the rays and the worst t and u, v errors against float64 (in units of the
bounds of tests/trace_reference.py, and t in float32 ulps).
"""
import numpy as np
import pytest

import trace_cases as cases
import trace_checks as checks
import trace_reference as ref


def test_reference_self_check():
    """Hand-computed rays: the unit quad at z = 1 seen from the origin (t = 1 exactly), an edge hit, a miss, a zero-area triangle."""
    quad = np.array([[(-1, -1, 1), (1, -1, 1), (1, 1, 1)], [(-1, -1, 1), (1, 1, 1), (-1, 1, 1)], [(0, 0, 2), (1, 1, 3), (2, 2, 4)]], np.float64)
    o = np.zeros((3, 4))
    d = np.array([[0, 0, 1], [0.5, -0.5, 1], [0, 3, 1], [1, 1, 2]], np.float64).T
    bf = ref.brute_force(o, d, quad)
    assert bf.t[0] == 1.0 and bf.index[0] in (0, 1) and bf.t_second[0] == 1.0      # the diagonal: both halves, a tie
    assert not ref.robust_closest(bf)[0]                                             # ... so not robust
    assert bf.t[1] == 1.0 and bf.index[1] == 0 and abs(bf.margin[1] - 0.25) < 1e-15 and ref.robust_closest(bf)[1]
    assert not np.isfinite(bf.t[2]) and bf.index[2] == -1 and ref.robust_closest(bf)[2]
    assert (bf.index != 2).all() and bf.t[3] == 0.5                                  # det = 0 (triangle 2, on the ray): never hit
    assert ref.occluded(bf, np.array([2.0, 1.0, np.inf, 0.5])).tolist() == [True, False, False, False]
    assert not ref.robust_shadow(bf, np.array([2.0, 1.0, np.inf, 0.5]))[1]          # the limit at the hit


@pytest.fixture(scope="module")
def all_cases(tmp_path_factory):
    return cases.all_cases(str(tmp_path_factory.mktemp("trace_cases")))


WALKS = [("cwbvh", {}), ("cwbvh plain walk", {"skip_behind_hit": 0}), ("bvh2", {"bvh_type": 2}), ("bvh4", {"bvh_type": 4})]


def test_oracle_matches_float64_on_adversarial_scenes(grt, oracle, all_cases):
    report = checks.Report()
    rng = np.random.default_rng(5)
    for case in all_cases:
        bf = ref.brute_force(case.origin, case.direction, case.world)
        t_bits = {}
        for walk, config in WALKS:
            scene, pt = checks.load(grt, case, -1, **config)
            width = config.get("bvh_type", 8)
            view = oracle.SceneView(pt, bvh_type=width)
            hits, stats = view.trace(case.origin, case.direction)
            label = "%s / %s" % (case.name, walk)
            if width == 8:
                assert stats.max_stack <= checks.STACK_LIMIT, label
                assert pt.static_geometry_whole_scene == (case.config.get("merge_static", 1) != 0), label   # the flattened tree or the TLAS layout, as meant
                assert pt.skip_behind_hit == (pt.static_geometry_whole_scene and config.get("skip_behind_hit", 1) != 0), label
            checks.check_closest(label, case, pt, case.origin, case.direction, hits, bf, report)
            t_bits[walk] = hits[:, 2].copy()
            if walk == "cwbvh plain walk":   # the skipping walk drops only groups behind the hit: the same records, bit for bit
                assert np.array_equal(hits, first_hits), label
            if walk == "cwbvh":
                first_hits = hits
                t32 = checks.unpack(hits)[2]
                limits = cases.shadow_limits(np.where(checks.unpack(hits)[1] >= 0, t32, np.inf), rng)
                so, sd = np.repeat(case.origin, 6, 1), np.repeat(case.direction, 6, 1)
                occ, _ = view.trace_shadow(so, sd, limits)
                sbf = ref.BruteForce(**{k: np.repeat(v, 6) for k, v in bf.__dict__.items()})
                checks.check_shadow(label, occ, sbf, limits)
                # against the oracle's own closest hit: never occluded at a limit of exactly its t (t < max_distance is strict) or 0. One ulp
                # beyond it need not be occluded: a node's box may be entered after the triangle it holds (a face in the plane of the box), and
                # the shadow walk tests the box against the limit
                hit = checks.unpack(hits)[1] >= 0
                assert (occ.reshape(-1, 6)[hit, 2] == 0).all(), label
                assert (occ.reshape(-1, 6)[:, 0] == 0).all(), label
            pt.close(); scene.close()
        # on robust rays every walk finds the same closest distance, bit for bit (elsewhere the walks may differ: BVH2 / BVH4 order the
        # triangles their own way and test unquantised boxes, so at a shared vertex or edge another triangle's float32 t may win)
        robust = ref.robust_closest(bf)
        for walk in t_bits:
            assert np.array_equal(t_bits[walk][robust], t_bits["cwbvh"][robust]), "%s: %s t bits differ from the CWBVH walk's" % (case.name, walk)
    print("\n" + "\n".join(report.lines()))
