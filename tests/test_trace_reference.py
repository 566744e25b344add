"""The oracle's traversal against a float64 brute force on small adversarial scenes (tests/trace_cases.py), for the CWBVH with
the skipping walk on and off, the TLAS layout, the binary and the 4-wide BVH. CPU only; the GPU half is test_gpu_trace_stream.py (the merged
wavefront's launch) and test_gpu_trace_queue.py (the per-bounce launches, all three widths), which launch these cases only because every walk's
deepest stack is shown here to stay within the device's.

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
    deepest = {}   # walk -> (max_stack, case), closest-hit and shadow rays together
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
            # every width's deepest stack, closest-hit and shadow rays (the six limits per ray the device tests use): the device walkers keep
            # RT_STACK_SIZE entries per lane and do not check their spill index, so a case beyond it must never be launched
            tri_w, t_w = checks.unpack(hits)[1], checks.unpack(hits)[2]
            limits_w = cases.shadow_limits(np.where(tri_w >= 0, t_w, np.inf), np.random.default_rng(7))
            _, shadow_stats = view.trace_shadow(np.repeat(case.origin, 6, 1), np.repeat(case.direction, 6, 1), limits_w)
            depth = max(int(stats.max_stack), int(shadow_stats.max_stack))
            assert depth <= checks.STACK_LIMIT, "%s: max_stack %d beyond RT_STACK_SIZE" % (label, depth)
            if depth > deepest.get(walk, (0, ""))[0]:
                deepest[walk] = (depth, case.name)
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
    print("deepest traversal stack per walk (RT_STACK_SIZE %d, RT_LDS_STACK %d): %s" % (
        checks.STACK_LIMIT, checks.LDS_STACK, ", ".join("%s %d (%s)" % (walk, deepest[walk][0], deepest[walk][1]) for walk, _ in WALKS)))
    # each width goes beyond the LDS part of the device's stack on some case, so the device tests on these cases run its spill to HBM: a later
    # change of the cases cannot silently stop exercising it
    for walk, _ in WALKS:
        assert deepest[walk][0] > checks.LDS_STACK, "%s: no case takes the stack beyond the %d entries kept in LDS (deepest %d)" % (walk, checks.LDS_STACK, deepest[walk][0])


def test_expected_frames_on_a_hand_written_queue():
    """trace_checks.expected_frames, which the device tests compare frames with: set against add, the flag's mask, occluded rays, null frames, AO."""
    F = checks.FLAG_BOUNCE_0
    prefill = [np.arange(24, dtype=np.float32).reshape(6, 4) + np.float32(100 * (k + 1)) for k in range(3)]
    light = np.array([[1, 2, 3], [0.5, 0.25, 0.125], [7, 8, 9], [10, 20, 30]], np.float32)
    occluded = np.array([0, 0, 1, 0], np.uint8)
    # per-bounce, bounce 0: rays 0, 1, 3 reach pixels 4, 0, 2; ray 2 (pixel 5) is occluded; pixels 1 and 3 are unnamed
    words = np.array([4, 0, 5, 2], np.uint32)
    r, d, i = checks.expected_frames(prefill, light, words, occluded, bounce=0)
    assert r[4].tolist() == [117.0, 119.0, 121.0, 119.0] and r[0].tolist() == [100.5, 101.25, 102.125, 103.0] and r[2].tolist() == [118.0, 129.0, 140.0, 111.0]
    assert d[4].tolist() == [1.0, 2.0, 3.0, 0.0] and d[0].tolist() == [0.5, 0.25, 0.125, 0.0] and d[2].tolist() == [10.0, 20.0, 30.0, 0.0]   # set: the prefill and its w are gone
    assert np.array_equal(i, prefill[2])
    for frame, before in zip((r, d, i), prefill):
        assert np.array_equal(frame[[1, 3, 5]], before[[1, 3, 5]])   # unnamed and occluded pixels
    # ... a later bounce: DIRECT untouched, INDIRECT added to
    r1, d1, i1 = checks.expected_frames(prefill, light, words, occluded, bounce=3)
    assert np.array_equal(r1, r) and np.array_equal(d1, prefill[1])
    assert i1[4].tolist() == [317.0, 319.0, 321.0, 319.0] and np.array_equal(i1[[1, 3, 5]], prefill[2][[1, 3, 5]])
    # merged: the flag picks the frame per ray and is no part of the pixel
    flagged = words | np.array([F, 0, F, 0], np.uint32)
    rm, dm, im = checks.expected_frames(prefill, light, flagged, occluded)
    assert np.array_equal(rm, r)
    assert dm[4].tolist() == [1.0, 2.0, 3.0, 0.0] and np.array_equal(dm[[0, 1, 2, 3, 5]], prefill[1][[0, 1, 2, 3, 5]])
    assert np.array_equal(im[4], prefill[2][4]) and im[0].tolist() == [300.5, 301.25, 302.125, 303.0] and im[2].tolist() == [318.0, 329.0, 340.0, 311.0]
    with pytest.raises(AssertionError):
        checks.expected_frames(prefill, light, flagged, occluded, bounce=0)             # a flag in a per-bounce word
    with pytest.raises(AssertionError):
        checks.expected_frames(prefill, light, np.array([4, 0, 4 | F, 2], np.uint32), occluded)   # one pixel twice (the flag does not tell them apart)
    # null frames: the others are what they were with all three
    for missing in ([0], [1], [2], [0, 1, 2]):
        some = [None if k in missing else prefill[k] for k in range(3)]
        out = checks.expected_frames(some, light, flagged, occluded)
        for k, want in enumerate((rm, dm, im)):
            assert out[k] is None if k in missing else np.array_equal(out[k], want)
    # AO: RADIANCE set to ones whatever the illumination, nothing else touched
    ra, da, ia = checks.expected_frames(prefill, light, words, occluded, bounce=0, ao=True)
    assert (ra[[4, 0, 2]] == 1.0).all() and np.array_equal(ra[[1, 3, 5]], prefill[0][[1, 3, 5]]) and np.array_equal(da, prefill[1]) and np.array_equal(ia, prefill[2])
    # the inputs are left alone, and check_frames tells a lost contribution from a doubled one
    assert prefill[0][4].tolist() == [116.0, 117.0, 118.0, 119.0]
    assert checks.check_frames("hand", [rm, dm, im], [rm, dm, im], prefill, light, flagged) == [6, 6, 6]
    lost = rm.copy(); lost[4] = prefill[0][4]
    with pytest.raises(AssertionError, match="LOST"):
        checks.check_frames("hand", [lost, dm, im], [rm, dm, im], prefill, light, flagged)
    twice = rm.copy(); twice[4] = prefill[0][4] + np.float32(2) * np.array([1, 2, 3, 0], np.float32)
    with pytest.raises(AssertionError, match="TWICE"):
        checks.check_frames("hand", [twice, dm, im], [rm, dm, im], prefill, light, flagged)
