"""The merged wavefront's traversal launch, ray by ray, through rt_trace_stream_rays (the frame's own kernel choice and engines)
against the oracle (bit for bit) and the float64 brute force (tests/trace_reference.py), on the adversarial scenes of
tests/trace_cases.py and on Sponza.

Covered: the three frame kernels (flat skipping, flat, general) and the counting kernel, both queue parities, the narrow
(<= RT_NARROW_MAX_RAYS rays), mixed-with-endgame and split engines, the dealing boundaries of fetch_ray's blocks and regions,
and that the probe leaves the next frame unchanged. Every batch's oracle max_stack is checked against RT_STACK_SIZE on the CPU
before the launch: the device does not check its spill index.
"""
import numpy as np
import pytest

import trace_cases as cases
import trace_checks as checks
import trace_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xA5A5A5A5)   # what every hit record holds before a launch: a record left so was never dealt
KERNEL_GENERAL, KERNEL_FLAT, KERNEL_FLAT_SKIP, KERNEL_COUNTING = 0, 1, 2, 3


def probe(grt, pt, iteration, o, d, so, sd, md, counting=False):
    hits = np.full((o.shape[1], 4), SENTINEL, np.uint32)
    return grt.trace_stream_rays(pt.ctx, iteration, o, d, hits, so, sd, md, counting=counting)


def shadow_rays(case, oracle_hits, seed):
    _, tri, t, _, _ = checks.unpack(oracle_hits)
    limits = cases.shadow_limits(np.where(tri >= 0, t, np.inf), np.random.default_rng(seed))
    return np.repeat(case.origin, 6, 1), np.repeat(case.direction, 6, 1), limits


@pytest.fixture(scope="module")
def all_cases(tmp_path_factory):
    return cases.all_cases(str(tmp_path_factory.mktemp("trace_cases_gpu")))


def test_stream_launch_matches_the_oracle_and_float64(grt, oracle, all_cases):
    """Every case under each kernel, both parities, the narrow and the mixed engine: hits bit-identical to the oracle (mesh,
    triangle, t bits, quantised u, v), shadow_light exactly 1 - the oracle's occlusion, no record left undealt, and the float64
    rules on top. The counting kernel's counters equal the oracle's exactly."""
    for case in all_cases:
        bf = ref.brute_force(case.origin, case.direction, case.world)
        flat = case.config.get("merge_static", 1) != 0
        for config, kernel in (({}, KERNEL_FLAT_SKIP if flat else KERNEL_GENERAL), ({"skip_behind_hit": 0}, KERNEL_FLAT if flat else KERNEL_GENERAL)):
            scene, pt = checks.load(grt, case, 0, **config)
            view = oracle.SceneView(pt)
            want_hits, cstats = view.trace(case.origin, case.direction)
            so, sd, md = shadow_rays(case, want_hits, 7)
            want_occ, sstats = view.trace_shadow(so, sd, md)
            assert cstats.max_stack <= checks.STACK_LIMIT and sstats.max_stack <= checks.STACK_LIMIT, case.name   # (before any launch)
            n, m = case.origin.shape[1], so.shape[1]
            label = "%s / %s" % (case.name, config)
            # narrow: both queues within RT_NARROW_MAX_RAYS; mixed with the endgame: all of them
            for iteration, nc, ns in ((0, min(n, 6000), min(m, 10000)), (1, n, m), (2, n, m), (3, min(n, 6000), min(m, 10000))):
                hits, light, _, info = probe(grt, pt, iteration, case.origin[:, :nc], case.direction[:, :nc], so[:, :ns], sd[:, :ns], md[:ns])
                assert info[0] == kernel, (label, info)
                assert nc + ns <= info[3] and (iteration not in (0, 3) or nc + ns <= info[2]), (label, info)   # (the subsets: the narrow engine)
                assert not (hits == SENTINEL).all(1).any(), "%s: %d closest-hit rays never dealt" % (label, (hits == SENTINEL).all(1).sum())
                bad = np.nonzero((hits != want_hits[:nc]).any(1))[0]
                assert bad.size == 0, "%s, iteration %d: %d hits differ from the oracle, first ray %d: %s against %s" % (label, iteration, bad.size, bad[0], hits[bad[0]].tolist(), want_hits[bad[0]].tolist())
                assert np.isin(light, (0.0, 1.0)).all(), "%s: shadow rays dealt %s times" % (label, sorted(set(light.tolist())))
                bad = np.nonzero(light != 1.0 - want_occ[:ns])[0]
                assert bad.size == 0, "%s, iteration %d: %d shadow rays differ from the oracle's occlusion, first %d" % (label, iteration, bad.size, bad[0])
                if nc == n and ns == m:
                    all_hits, all_light = hits, light
            checks.check_closest(label, case, pt, case.origin, case.direction, all_hits, bf)
            checks.check_shadow(label, 1.0 - all_light, ref.BruteForce(**{k: np.repeat(v, 6) for k, v in bf.__dict__.items()}), md)
            if not config:
                # the counting kernel (what rt_set_trace_statistics launches) on the same rays: the oracle's counters, exactly -- the walk of a ray is
                # the oracle's step for step, and a ray's counts do not depend on which lane or wave deals it
                hits, light, stats, info = probe(grt, pt, 1, case.origin, case.direction, so, sd, md, counting=True)
                assert info[0] == KERNEL_COUNTING
                assert np.array_equal(hits, want_hits) and np.array_equal(light, 1.0 - want_occ), label
                for kind, st in (("closest", cstats), ("shadow", sstats)):
                    got = stats[kind]
                    want = dict(nodes=st.nodes, triangles=st.triangles, instances_transformed=st.instances_transformed, instances_identity=st.instances_identity, rays=st.rays)
                    assert got == want, (label, kind, got, want)
            pt.close(); scene.close()


def test_every_ray_is_dealt_once_at_the_dealing_boundaries(grt, oracle, all_cases):
    """Queue lengths at the edges of fetch_ray's blocks (64), of the narrow engine (16384) and of the endgame's regions (W x 64,
    W x 256 for a grid of W waves), odd closest / shadow splits and empty queues, both parities. Rays that miss everything, so
    that every shadow ray must add exactly 1: a ray left undealt shows as 0, a ray dealt twice as 2, a closest-hit record
    left undealt keeps the sentinel."""
    case = all_cases[0]   # the boxes
    scene, pt = checks.load(grt, case, 0)
    _, _, _, info = probe(grt, pt, 0, *(np.zeros((3, 0), np.float32),) * 4, np.zeros(0, np.float32))
    assert info[0] == KERNEL_FLAT_SKIP
    W = int(info[1])
    assert W >= 64 and info[2] == 16384 and info[3] == 10 * 1024 * 1024
    totals = [0, 1, 63, 64, 65, 16384, 16385, W * 64 - 1, W * 64 + 1, W * 256 - 1, W * 256 + 1, W * 256 + W * 64 + 7]
    splits = []
    for k, total in enumerate(totals):
        closest = total // 3 if k % 2 else total - total // 5
        splits.append((k & 1, closest, total - closest))
    splits += [(0, 16384, 0), (1, 0, 16384), (0, 16385, 0), (1, 0, W * 256 + 1), (0, W * 256 + W * 64 + 7, 0)]
    biggest = max(c for _, c, _ in splits) + max(s for _, _, s in splits)
    rng = np.random.default_rng(3)
    o = (np.float32(50.0) + rng.uniform(0, 1, (3, biggest))).astype(np.float32)   # beyond the boxes, looking away from them
    d = cases.normalised(np.abs(rng.normal(size=(3, biggest))) + 0.1)
    md = np.full(biggest, np.inf, np.float32)
    miss = np.array([0, 0xFFFFFFFF, 0x7F800000, 0], np.uint32)   # mesh 0, RT_INVALID, t = inf, u = v = 0
    _, stats = oracle.SceneView(pt).trace(o[:, :1000], d[:, :1000])
    assert stats.max_stack <= checks.STACK_LIMIT
    for iteration, nc, ns in splits:
        hits, light, _, info = probe(grt, pt, iteration, o[:, :nc], d[:, :nc], o[:, nc:nc + ns], d[:, nc:nc + ns], md[nc:nc + ns])
        undealt = int((hits == SENTINEL).all(1).sum())
        assert undealt == 0, "%d + %d rays (iteration %d): %d closest-hit rays never dealt" % (nc, ns, iteration, undealt)
        assert (hits == miss).all(), (nc, ns, iteration)
        assert (light == 1.0).all(), "%d + %d rays (iteration %d): shadow rays dealt %s times" % (nc, ns, iteration, sorted(set(light.tolist())))
    pt.close(); scene.close()


def test_the_split_engine_on_sponza(grt, oracle):
    """Above RT_MIXED_MAX_RAYS the launch runs closest-hit and shadow rays one after the other: 10.5 M incoherent closest-hit rays
    (and 4096 shadow rays) through the frame's launch, all of them equal to rt_trace_rays, a 1 / 64 subset to the oracle; and
    Sponza's camera rays through the narrow and the mixed engine against the oracle."""
    from conftest import make_pathtracer
    scene, pt = make_pathtracer(grt, "sponza", 160, 90, 0)
    view = oracle.SceneView(pt)
    o, d, _ = view.generate(0, 0, 160 * 90)
    want, st = view.trace(o, d)
    assert st.max_stack <= checks.STACK_LIMIT
    for iteration, n in ((0, 8000), (1, 160 * 90)):
        hits, _, _, info = probe(grt, pt, iteration, o[:, :n], d[:, :n], *(np.zeros((3, 0), np.float32),) * 2, np.zeros(0, np.float32))
        assert info[0] == KERNEL_FLAT_SKIP and np.array_equal(hits, want[:n]), iteration
    n = 10 * 1024 * 1024 + 512 * 1024
    rng = np.random.default_rng(9)
    lo, hi = np.array([-1800, 20, -700], np.float32), np.array([1700, 1200, 650], np.float32)   # inside the atrium
    O = (lo[:, None] + (hi - lo)[:, None] * rng.random((3, n), np.float32)).astype(np.float32)
    D = rng.normal(size=(3, n)).astype(np.float32); D /= np.linalg.norm(D, axis=0)
    so, sd, md = O[:, :4096], D[:, ::-1][:, :4096].copy(), np.full(4096, 300.0, np.float32)
    sub = slice(0, n, 64)
    want_sub, st = view.trace(O[:, sub], D[:, sub])
    want_occ, st2 = view.trace_shadow(so, sd, md)
    assert st.max_stack <= checks.STACK_LIMIT and st2.max_stack <= checks.STACK_LIMIT
    hits, light, _, info = probe(grt, pt, 1, O, D, so, sd, md)
    assert n + 4096 > info[3] and info[0] == KERNEL_FLAT_SKIP
    assert not (hits == SENTINEL).all(1).any()
    assert np.array_equal(hits[sub], want_sub)
    assert np.array_equal(light, 1.0 - want_occ)
    explicit, _ = grt.trace_rays(pt.ctx, O, D)
    assert np.array_equal(hits, explicit)
    pt.close(); scene.close()


def test_the_probe_leaves_the_next_frame_unchanged(grt):
    """A frame rendered after the probe is bit-identical to one rendered without it."""
    from conftest import make_pathtracer
    images = []
    for with_probe in (False, True):
        scene, pt = make_pathtracer(grt, "cornellbox", 96, 64, 0, num_bounces=4)
        pt.render()
        if with_probe:
            rng = np.random.default_rng(1)
            o = np.zeros((3, 5000), np.float32) + np.array([[0.0], [1.0], [0.0]], np.float32)
            d = cases.normalised(rng.normal(size=(3, 5000)))
            for iteration in (0, 1, 6, 7):
                probe(grt, pt, iteration, o, d, o, d, np.full(5000, 0.5, np.float32))
        pt.update(); pt.render()
        images.append(pt.read_framebuffer().copy())
        pt.close(); scene.close()
    assert np.array_equal(images[0], images[1])


def test_the_probe_refuses_bad_arguments(grt):
    from conftest import make_pathtracer
    scene, pt = make_pathtracer(grt, "cornellbox", 32, 32, 0)
    lib = grt.device_lib()
    info = np.zeros(4, np.int32)
    assert lib.rt_trace_stream_rays(pt.ctx, -1, *[None] * 6, 0, None, *[None] * 7, 0, None, None, info.ctypes.data) != 0
    assert b"negative iteration" in lib.rt_last_error(pt.ctx)
    assert lib.rt_trace_stream_rays(pt.ctx, 0, *[None] * 6, 5, None, *[None] * 7, 0, None, None, info.ctypes.data) != 0
    assert b"NULL closest-hit" in lib.rt_last_error(pt.ctx)
    assert lib.rt_trace_stream_rays(pt.ctx, 0, *[None] * 6, 0, None, *[None] * 7, 3, None, None, info.ctypes.data) != 0
    assert b"NULL shadow" in lib.rt_last_error(pt.ctx)
    assert lib.rt_trace_stream_rays(pt.ctx, 0, *[None] * 6, 0, None, *[None] * 7, 0, None, None, None) != 0
    assert lib.rt_trace_stream_rays(pt.ctx, 0, *[None] * 6, 0, None, *[None] * 7, 0, None, None, info.ctypes.data) == 0
    pt.close(); scene.close()
