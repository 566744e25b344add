"""The frame's per-bounce traversal launches and the BVH2 / BVH4 walker, ray by ray, through rt_trace_queue_rays (the launchers a frame of the
slots scheduler calls: rt_launch_trace, then rt_launch_trace_shadow; their _counting forms; rt_launch_trace_shadow_ao; and, merged, the merged
wavefront's one launch with the caller's illumination, pixel words and frames) against the oracle (bit for bit) and the float64 brute force
(tests/trace_reference.py), on the adversarial scenes of tests/trace_cases.py.

What fails if a piece is wrong:
* bvh_trace_persistent's fetch_ray (BVH2 / BVH4): test_every_ray_is_dealt_once_at_the_walkers_boundaries -- a record that keeps its sentinel, a pixel
  that keeps its prefill (lost) or holds prefill + 2 x value (dealt twice), at every step of ray_block and at the early return of a wave;
* its spill: `deep` under width 4 (oracle max_stack 25) and `instanced_many` under width 2 (15) in test_hits_and_occlusion_match_the_oracle_and_float64
  -- a wrong spilled entry changes a hit record, which must equal the oracle's bits;
* its TLAS leave: the instanced cases there (rotated, scaled instances: a ray not restored to world space hits the wrong triangle or t);
* the non-UNIFIED CWBVH engine's narrow / wide choice: the same test's three launches per case (bounce 0: coherent, wide at any count; bounce 1 at
  <= 16384 rays: narrow; bounce 1 above: wide), and 16384 / 16385 / 1000-at-bounce-0 in the dealing test;
* the two shadow sources' three writes (ShadowQueueSource::finish, ShadowStreamSource::contribute): test_where_a_contribution_goes_* compare RADIANCE,
  RADIANCE_DIRECT and RADIANCE_INDIRECT as bits with trace_checks.expected_frames (set against add, the flag's mask, w = 0, the null-frame guards);
* ShadowAOSource: test_the_ao_launch_sets_radiance_to_one.

Every batch's oracle max_stack OF THE WIDTH IT RUNS UNDER is checked against RT_STACK_SIZE on the CPU before any launch (Walk.__init__): the device does
not check its spill index. A batch that failed would not be launched; with the present cases none does (tests/test_trace_reference.py prints the maxima).
"""
import numpy as np
import pytest

import trace_cases as cases
import trace_checks as checks
import trace_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xA5A5A5A5)   # what every hit record holds before a launch: a record left so was never dealt
MISS = np.array([0, 0xFFFFFFFF, 0x7F800000, 0], np.uint32)   # mesh 0, RT_INVALID, t = inf, u = v = 0
NARROW_MAX, FETCH_BLOCK_MAX, MAX_BOUNCES = 16384, 256, 128
COUNTERS = ("nodes", "triangles", "instances_transformed", "instances_identity", "rays")
CASE_NAMES = ("boxes", "slivers", "layers", "deep", "deep_instanced", "scale_small", "scale_large", "offset", "flat", "icosphere", "instanced", "instanced_many")
INSTANCED = ("deep_instanced", "instanced", "instanced_many")   # merge_static = 0 is the case's own: the `tlas` walk would repeat `cwbvh`
WALKS = {"cwbvh": (8, {}), "cwbvh plain walk": (8, {"skip_behind_hit": 0}), "cwbvh tlas": (8, {"merge_static": 0}), "bvh2": (2, {"bvh_type": 2}), "bvh4": (4, {"bvh_type": 4})}
WIDTH_WALK = {8: "cwbvh", 2: "bvh2", 4: "bvh4"}


@pytest.fixture(scope="module")
def all_cases(tmp_path_factory):
    found = cases.all_cases(str(tmp_path_factory.mktemp("trace_queue_gpu")))
    assert tuple(c.name for c in found) == CASE_NAMES
    return {c.name: c for c in found}


@pytest.fixture(scope="module")
def brute():
    """The float64 brute force of a case's rays, computed once per case and shared by its walks (never changed)."""
    cache = {}

    def of(case):
        if case.name not in cache:
            cache[case.name] = ref.brute_force(case.origin, case.direction, case.world)
        return cache[case.name]
    return of


def empty3():
    return np.zeros((3, 0), np.float32)


class Walk:
    """A case under one walk: its rays and six shadow rays per ray with the oracle's answers OF THAT WIDTH; queues of any length repeat them in
    order (a ray's result does not depend on where in a queue it stands). The oracle's deepest stack is checked before anything is launched."""

    def __init__(self, grt, oracle, case, walk):
        self.grt, self.case, self.walk = grt, case, walk
        self.width, config = WALKS[walk]
        self.scene, self.pt = checks.load(grt, case, 0, **config)
        self.view = oracle.SceneView(self.pt, bvh_type=self.width)
        self.o, self.d = case.origin, case.direction
        self.hits, self.stats = self.view.trace(self.o, self.d)
        _, tri, t, _, _ = checks.unpack(self.hits)
        self.md = cases.shadow_limits(np.where(tri >= 0, t, np.inf), np.random.default_rng(7))
        self.so, self.sd = np.repeat(self.o, 6, 1), np.repeat(self.d, 6, 1)
        self.occluded, self.shadow_stats = self.view.trace_shadow(self.so, self.sd, self.md)
        self.n, self.m = self.o.shape[1], self.so.shape[1]
        self.label = "%s / %s" % (case.name, walk)
        # before any launch: the device does not check its spill index
        self.safe = self.stats.max_stack <= checks.STACK_LIMIT and self.shadow_stats.max_stack <= checks.STACK_LIMIT
        assert self.safe, "%s: oracle max_stack %d / %d beyond RT_STACK_SIZE -- not launched" % (self.label, self.stats.max_stack, self.shadow_stats.max_stack)

    def close(self):
        self.pt.close(); self.scene.close()

    def launch(self, bounce, nc, ns, form=0, merged=False):
        """nc closest-hit and ns shadow rays (ray j is base ray j mod n / m); shadow ray j carries (1, 0.5, 0.25) for pixel j of three zeroed frames.
        Every record against the oracle's bits, every pixel against expected_frames. Returns (hits, occluded as the frames tell it, stats, info)."""
        assert self.safe
        ci, si = np.arange(nc) % self.n, np.arange(ns) % self.m
        light = np.tile(np.array([1.0, 0.5, 0.25], np.float32), (ns, 1))
        words = np.arange(ns, dtype=np.uint32)
        prefill = [np.zeros((ns, 4), np.float32) for _ in range(3)]
        hits, frames, stats, info = self.grt.trace_queue_rays(self.pt.ctx, bounce, self.o[:, ci], self.d[:, ci], np.full((nc, 4), SENTINEL, np.uint32),
                                                              self.so[:, si], self.sd[:, si], self.md[si], light, words, prefill, ns, merged=merged, form=form)
        label = "%s: %d + %d rays, %s %d, form %d" % (self.label, nc, ns, "iteration" if merged else "bounce", bounce, form)
        assert info[0] == self.width and info[3] == NARROW_MAX and (merged or info[4] == FETCH_BLOCK_MAX), (label, info)
        undealt = int((hits == SENTINEL).all(1).sum())
        assert undealt == 0, "%s: %d closest-hit rays never dealt (their records keep the sentinel)" % (label, undealt)
        bad = np.nonzero((hits != self.hits[ci]).any(1))[0]
        assert bad.size == 0, "%s: %d hits differ from the oracle, first ray %d: %s against %s" % (label, bad.size, bad[0], hits[bad[0]].tolist(), self.hits[ci][bad[0]].tolist())
        want = checks.expected_frames(prefill, light, words, self.occluded[si], bounce=None if merged else bounce)
        self.contributions = checks.check_frames(label, frames, want, prefill, light, words)
        return hits, frames[0][:, 0] == 0.0, stats, info

    def counters(self, shadow):
        st = self.shadow_stats if shadow else self.stats
        return {name: int(getattr(st, name)) for name in COUNTERS}


def over(base, least):
    """The smallest whole number of repeats of a queue of `base` rays that holds more than `least`."""
    return base * (least // base + 1)


# (merge_static = 0 is an instanced case's own config: there the `cwbvh tlas` walk would repeat `cwbvh`)
CASE_WALKS = [(c, w) for c in CASE_NAMES for w in WALKS if not (w == "cwbvh tlas" and c in INSTANCED)]


@pytest.mark.parametrize("case_name,walk", CASE_WALKS)
def test_hits_and_occlusion_match_the_oracle_and_float64(grt, oracle, all_cases, brute, case_name, walk):
    """Every case under every walk through the per-bounce launches at bounce 0 (closest hit coherent: one ray per lane at any count), bounce 1 within
    RT_NARROW_MAX_RAYS (width 8: the narrow engine) and bounce 1 just beyond it (the wide engine); through the counting launches (width 8); and
    through the explicit kernels (rt_trace_rays, rt_trace_shadow_rays). Hit records equal the oracle's of the same width bit for bit with no sentinel
    left, shadow rays deliver exactly where the oracle says unoccluded, the float64 rules hold, the counters equal the oracle's."""
    case = all_cases[case_name]
    rays = Walk(grt, oracle, case, walk)
    try:
        n, m = rays.n, rays.m
        assert n <= NARROW_MAX
        launched = []
        hits, occluded, _, info = rays.launch(0, n, m)
        launched.append((0, n, m))
        contributions = list(rays.contributions)
        for nc, ns in ((n, min(m, NARROW_MAX)), (over(n, NARROW_MAX), over(m, NARROW_MAX))):
            rays.launch(1, nc, ns)
            launched.append((1, nc, ns))
        report = checks.Report()
        bf = brute(case)
        checks.check_closest(rays.label, case, rays.pt, case.origin, case.direction, hits, bf, report)
        robust_shadow = checks.check_shadow(rays.label, occluded, ref.BruteForce(**{k: np.repeat(v, 6) for k, v in bf.__dict__.items()}), rays.md)
        if rays.width == 8:
            # the walk of a ray is the oracle's step for step, and a ray's counts do not depend on which lane or wave deals it
            _, _, stats, _ = rays.launch(1, n, m, form=grt.TRACE_QUEUE_COUNTING)
            launched.append(("counting", n, m))
            for kind, shadow in (("closest", False), ("shadow", True)):
                assert stats[kind] == rays.counters(shadow), (rays.label, kind, stats[kind], rays.counters(shadow))
        # the explicit kernels: the same engine instances on caller-given arrays
        explicit, _ = grt.trace_rays(rays.pt.ctx, case.origin, case.direction)
        bad = np.nonzero((explicit != rays.hits).any(1))[0]
        assert bad.size == 0, "%s: rt_trace_rays: %d hits differ from the oracle, first ray %d" % (rays.label, bad.size, bad[0])
        explicit_occluded, _ = grt.trace_shadow_rays(rays.pt.ctx, rays.so, rays.sd, rays.md)
        bad = np.nonzero(explicit_occluded != rays.occluded)[0]
        assert bad.size == 0, "%s: rt_trace_shadow_rays: %d rays differ from the oracle's occlusion, first %d" % (rays.label, bad.size, bad[0])
        print("\n%s\n  %d + %d rays, robust shadow share %.1f %%, oracle max_stack %d / %d, grid waves %d / %d, launches %s, contributions checked per frame %s" % (
            report.lines()[0], n, m, 100 * robust_shadow, rays.stats.max_stack, rays.shadow_stats.max_stack, info[1], info[2], launched, contributions))
    finally:
        rays.close()


# ---- where a contribution goes -------------------------------------------------------------------------------------

class Contributions:
    """Shadow queues on the boxes under one width: rays that miss everything (as the dealing tests build them) mixed with rays of unlimited reach aimed
    from outside at a point well inside one of the closed boxes, which the oracle says are occluded. Ray j of a queue is base ray j mod 4000, carries a
    triple of its own and names pixel perm[j] of P = M + M // 4 + 5, so some pixels are named by no ray; the three frames hold distinct finite values
    per pixel and channel."""

    def __init__(self, grt, oracle, case, width):
        self.grt, self.width = grt, width
        self.scene, self.pt = checks.load(grt, case, 0, **WALKS[WIDTH_WALK[width]][1])
        view = oracle.SceneView(self.pt, bvh_type=width)
        rng = np.random.default_rng(21)
        centres = np.array([(0.5, 0.5, 0.5), (2.5, 0.5, 0.5), (1.0, 2.5, -0.5), (-1.5, 1.0, -1.75)])   # of case_boxes' four boxes
        targets = centres[rng.integers(0, 4, 2000)].T + rng.uniform(-0.1, 0.1, (3, 2000))
        blocked_o, blocked_d = cases.aim(targets + cases.normalised(rng.normal(size=(3, 2000))).astype(np.float64) * 12.0, targets)
        o = np.concatenate([blocked_o, (np.float32(50.0) + rng.uniform(0, 1, (3, 2000))).astype(np.float32)], 1)
        d = np.concatenate([blocked_d, cases.normalised(np.abs(rng.normal(size=(3, 2000))) + 0.1)], 1)
        order = rng.permutation(4000)
        self.o, self.d = np.ascontiguousarray(o[:, order]), np.ascontiguousarray(d[:, order])
        self.md = np.full(4000, np.inf, np.float32)
        self.occluded, stats = view.trace_shadow(self.o, self.d, self.md)
        _, cstats = view.trace(self.o, self.d)
        assert stats.max_stack <= checks.STACK_LIMIT and cstats.max_stack <= checks.STACK_LIMIT   # (before any launch)
        assert self.occluded[order < 2000].all() and not self.occluded[order >= 2000].any()   # half blocked by a box, half beyond the boxes
        self.label = "boxes / width %d" % width

    def close(self):
        self.pt.close(); self.scene.close()

    def queue(self, count, flags=False, seed=0):
        rng = np.random.default_rng(100 + seed)
        index = np.arange(count) % 4000
        pixels = count + count // 4 + 5
        words = rng.permutation(pixels)[:count].astype(np.uint32)
        if flags:
            words |= np.where(rng.random(count) < 0.5, checks.FLAG_BOUNCE_0, np.uint32(0)).astype(np.uint32)
        j = np.arange(count, dtype=np.int64)
        light = np.stack([((j % 1021) + 1) / 8.0, ((j % 509) + 1) / 16.0, (j + 1) / 1024.0], 1).astype(np.float32)
        assert count < 1 << 24   # (the third component, (j + 1) / 1024, is exact and so distinct per ray)
        flat = np.arange(pixels * 4, dtype=np.float64).reshape(pixels, 4) * 0.125
        prefill = [(flat + 1000.0 * (k + 1)).astype(np.float32) for k in range(3)]   # (exact in float32: below 2^20 with three fraction bits)
        return index, words, light, prefill, pixels

    def launch(self, step, count, present=(0, 1, 2), merged=False, form=0, closest=0, flags=False, seed=0):
        index, words, light, prefill, pixels = self.queue(count, flags, seed)
        given = [prefill[k] if k in present else None for k in range(3)]
        ci = np.arange(closest) % 4000
        hits, frames, _, info = self.grt.trace_queue_rays(self.pt.ctx, step, self.o[:, ci], self.d[:, ci], np.full((closest, 4), SENTINEL, np.uint32),
                                                          self.o[:, index], self.d[:, index], self.md[index], light, words, given, pixels, merged=merged, form=form)
        label = "%s: %d shadow rays, %s %d, form %d, frames %s" % (self.label, count, "iteration" if merged else "bounce", step, form, list(present))
        assert not (hits == SENTINEL).all(1).any(), label
        want = checks.expected_frames(given, light, words, self.occluded[index], bounce=None if merged else step, ao=form == self.grt.TRACE_QUEUE_AO)
        checked = checks.check_frames(label, frames, want, given, light, words)
        live = ~self.occluded[index].astype(bool)
        first = (words & checks.FLAG_BOUNCE_0) != 0 if merged else np.full(count, step == 0)
        return info, checked, (int(live.sum()), int((live & first).sum()), int((live & ~first).sum()))


@pytest.fixture(scope="module")
def contributions(grt, oracle, all_cases):
    made = {}

    def of(width):
        if width not in made:
            for c in made.values():   # one context at a time
                c.close()
            made.clear()
            made[width] = Contributions(grt, oracle, all_cases["boxes"], width)
        return made[width]
    yield of
    for c in made.values():
        c.close()


@pytest.mark.parametrize("bounce", [0, 1, MAX_BOUNCES - 1])
@pytest.mark.parametrize("width", [8, 2, 4])
def test_where_a_contribution_goes_per_bounce(contributions, width, bounce):
    """ShadowQueueSource::finish through rt_launch_trace_shadow: RADIANCE += (value, 0) in all four channels; RADIANCE_DIRECT = (value, 0) at bounce 0;
    RADIANCE_INDIRECT += (value, 0) later; unnamed pixels and those of occluded rays keep the prefill bits; a frame passed as NULL is not there and
    the others are still right (each alone, and all three). 3000 rays (width 8: the narrow engine) and 20001 (the wide one)."""
    c = contributions(width)
    lines = []
    for count, present in ((3000, (0, 1, 2)), (3000, (1, 2)), (3000, (0, 2)), (3000, (0, 1)), (3000, ()), (20001, (0, 1, 2))):
        info, checked, live = c.launch(bounce, count, present, seed=bounce)
        assert info[0] == width
        assert live[0] > count // 8 and live[0] < count - count // 8
        lines.append("%d rays, frames %s: pixels compared %s, unoccluded %d (bounce 0: %d, later: %d)" % (count, list(present), checked, *live))
    print("\n%s, bounce %d:\n  %s" % (c.label, bounce, "\n  ".join(lines)))


def test_where_a_contribution_goes_in_the_merged_launch(contributions):
    """ShadowStreamSource::contribute through rt_launch_trace_stream, the flag set on about half of the rays so that ONE launch feeds RADIANCE_DIRECT
    (set) and RADIANCE_INDIRECT (added to), the flag stripped from the pixel index: the narrow engine (<= 16384 rays), and the mixed engine with
    five times 64 rays per wave of the grid, more than half of them unoccluded, so that the waves' deferred lists (contribution_flush, 128 entries)
    run full and are flushed partial at the end; both parities; with closest-hit rays in the same launch; each frame NULL in turn."""
    c = contributions(8)
    info, _, _ = c.launch(0, 0, merged=True)
    W = int(info[1])
    assert W >= 64 and info[5] in (1, 2)   # (a flat kernel: the boxes are one tree)
    lines = []
    for iteration, count, closest, present in ((0, 5000, 1000, (0, 1, 2)), (1, 5000, 1000, (0, 1, 2)), (2, 16384, 0, (0, 1, 2)), (3, 5000, 7, (1, 2)), (4, 5000, 7, (0, 2)), (5, 5000, 7, (0, 1)),
                                               (6, 5000, 0, ()), (7, 5 * 64 * W + 77, 1000, (0, 1, 2)), (8, 5 * 64 * W + 13, 0, (0, 1, 2))):
        info, checked, live = c.launch(iteration, count, present, merged=True, closest=closest, flags=True, seed=iteration)
        assert (count + closest <= NARROW_MAX) or live[0] > 64 * W
        assert live[1] > live[0] // 4 and live[2] > live[0] // 4   # one launch feeds both frames
        lines.append("iteration %d, %d + %d rays, frames %s: pixels compared %s, unoccluded %d (flagged: %d, not: %d)" % (iteration, closest, count, list(present), checked, *live))
    print("\n%s, merged launch, %d waves:\n  %s" % (c.label, W, "\n  ".join(lines)))


@pytest.mark.parametrize("width", [8, 2, 4])
def test_the_ao_launch_sets_radiance_to_one(grt, contributions, width):
    """ShadowAOSource::finish through rt_launch_trace_shadow_ao: an unoccluded ray sets its RADIANCE pixel to (1, 1, 1, 1) whatever its illumination,
    an occluded one leaves the prefill; RADIANCE_DIRECT and RADIANCE_INDIRECT, though given, are not touched; without RADIANCE nothing is written."""
    c = contributions(width)
    lines = []
    for count, present in ((3000, (0, 1, 2)), (20001, (0, 1, 2)), (3000, (1, 2))):
        info, checked, live = c.launch(0, count, present, form=grt.TRACE_QUEUE_AO, seed=9)
        assert info[0] == width
        lines.append("%d rays, frames %s: pixels compared %s, unoccluded %d" % (count, list(present), checked, live[0]))
    print("\n%s, AO launch:\n  %s" % (c.label, "\n  ".join(lines)))


# ---- dealing -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def miss_rays():
    """Rays beyond the boxes, looking away from them: every one misses everything."""
    rng = np.random.default_rng(3)
    count = 5 * 1024 * 1024   # (576 x W rays for the longest queue: W is at most 256 CUs x 8 workgroups x 4 waves)
    o = (np.float32(50.0) + rng.random((3, count), np.float32)).astype(np.float32)
    d = rng.random((3, count), np.float32) + np.float32(0.1)
    d /= np.sqrt((d.astype(np.float64) ** 2).sum(0)).astype(np.float32)
    return o, d


@pytest.mark.parametrize("kind", ["closest", "shadow", "both"])
@pytest.mark.parametrize("width", [2, 4, 8])
def test_every_ray_is_dealt_once_at_the_walkers_boundaries(grt, oracle, all_cases, miss_rays, width, kind):
    """Queue lengths at the edges of fetch_ray's blocks for a grid of W waves: 64, W x 64 (below it some waves return at once: their first block lies
    beyond the queue), and every step of ray_block = max(64, min(256, (n / 2W) & ~63)) -- 2W x 128, 2W x 192, 2W x 256; width 8 also at
    RT_NARROW_MAX_RAYS, and at bounce 0, where the closest-hit launch stays wide below it. Closest-hit only, shadow only and both, at bounces 0, 1
    and RT_MAX_BOUNCES - 1 (each has its own pair of cursors). All rays miss: every hit record must be the miss record, and every shadow ray must add
    its value exactly once -- check_frames says whether a contribution was lost (the prefill is left) or made twice (prefill + 2 x value)."""
    O, D = miss_rays
    scene, pt = checks.load(grt, all_cases["boxes"], 0, **WALKS[WIDTH_WALK[width]][1])
    try:
        view = oracle.SceneView(pt, bvh_type=width)
        sample = slice(0, O.shape[1], O.shape[1] // 4096)
        want, stats = view.trace(O[:, sample], D[:, sample])
        occluded, shadow_stats = view.trace_shadow(O[:, sample], D[:, sample], np.full(want.shape[0], np.inf, np.float32))
        assert stats.max_stack <= checks.STACK_LIMIT and shadow_stats.max_stack <= checks.STACK_LIMIT   # (before any launch)
        assert (want == MISS).all() and not occluded.any()

        def launch(bounce, nc, ns):
            light = np.tile(np.array([1.0, 2.0, 4.0], np.float32), (ns, 1))
            words = np.arange(ns, dtype=np.uint32)
            prefill = [(np.arange(ns * 4, dtype=np.int64).reshape(ns, 4) % 251).astype(np.float32), None, None]
            hits, frames, _, info = grt.trace_queue_rays(pt.ctx, bounce, O[:, :nc], D[:, :nc], np.full((nc, 4), SENTINEL, np.uint32),
                                                         O[:, :ns], D[:, :ns], np.full(ns, np.inf, np.float32), light, words, prefill, ns)
            label = "width %d, bounce %d, %d + %d rays" % (width, bounce, nc, ns)
            undealt = int((hits == SENTINEL).all(1).sum())
            assert undealt == 0, "%s: %d closest-hit rays never dealt (their records keep the sentinel), first %d" % (label, undealt, np.nonzero((hits == SENTINEL).all(1))[0][0])
            assert (hits == MISS).all(), "%s: a ray that misses everything has a hit record other than the miss record" % label
            want_frames = checks.expected_frames(prefill, light, words, np.zeros(ns, np.uint8), bounce=bounce)
            checks.check_frames(label, frames, want_frames, prefill, light, words)
            return info

        info = launch(0, 0, 0)
        assert info[0] == width and info[3] == NARROW_MAX and info[4] == FETCH_BLOCK_MAX
        Wc, Ws = int(info[1]), int(info[2])
        assert Wc >= 64 and Ws >= 64

        def lengths(W):
            return [0, 1, 63, 64, 65, W * 64 - 1, W * 64 + 1, 2 * W * 128 - 1, 2 * W * 128 + 1, 2 * W * 192 + 1, 2 * W * 256 - 1, 2 * W * 256 + 1, 2 * W * 256 + W * 64 + 7]
        plan = []   # (bounce, closest-hit rays, shadow rays)
        for k, (lc, ls) in enumerate(zip(lengths(Wc), lengths(Ws))):
            bounce = 1 if width == 8 else (0, 1, MAX_BOUNCES - 1)[k % 3]   # (width 8: bounce 1, so that the count alone picks the engine)
            plan.append((bounce, lc if kind != "shadow" else 0, ls if kind != "closest" else 0))
        if width == 8:
            for bounce, length in ((1, NARROW_MAX), (1, NARROW_MAX + 1), (0, NARROW_MAX + 1), (0, 1000), (MAX_BOUNCES - 1, 65)):
                plan.append((bounce, length if kind != "shadow" else 0, length if kind != "closest" else 0))
        assert max(max(nc, ns) for _, nc, ns in plan) <= O.shape[1]
        for bounce, nc, ns in plan:
            launch(bounce, nc, ns)
        print("\nwidth %d, %s: grid waves %d / %d, queue lengths dealt (bounce, closest, shadow): %s" % (width, kind, Wc, Ws, plan))
    finally:
        pt.close(); scene.close()


# ---- the probe and the context ---------------------------------------------------------------------------------------

def assert_safe(oracle, pt, o, d, md, width=8):
    """Before any launch: the oracle's deepest stack on these rays, closest hit and shadow (the device does not check its spill index)."""
    view = oracle.SceneView(pt, bvh_type=width)
    _, stats = view.trace(o, d)
    _, shadow_stats = view.trace_shadow(o, d, md)
    assert stats.max_stack <= checks.STACK_LIMIT and shadow_stats.max_stack <= checks.STACK_LIMIT


def probe_series(grt, oracle, pt):
    """Every form of the probe once, on rays inside the Cornell box."""
    ctx, width = pt.ctx, 8
    rng = np.random.default_rng(1)
    n = 5000
    o = np.zeros((3, n), np.float32) + np.array([[0.0], [1.0], [0.0]], np.float32)
    d = cases.normalised(rng.normal(size=(3, n)))
    md = np.full(n, 0.5, np.float32)
    assert_safe(oracle, pt, o, d, md)
    light = rng.random((n, 3)).astype(np.float32)
    words = rng.permutation(n + 100)[:n].astype(np.uint32)
    frames = [rng.random((n + 100, 4)).astype(np.float32) for _ in range(3)]
    hits = np.full((n, 4), SENTINEL, np.uint32)
    for bounce in (0, 1, 3):
        grt.trace_queue_rays(ctx, bounce, o, d, hits, o, d, md, light, words, frames, n + 100)
    grt.trace_queue_rays(ctx, 0, empty3(), empty3(), hits[:0], o, d, md, light, words, frames, n + 100, form=grt.TRACE_QUEUE_AO)
    if width == 8:
        grt.trace_queue_rays(ctx, 1, o, d, hits, o, d, md, light, words, frames, n + 100, form=grt.TRACE_QUEUE_COUNTING)
        for iteration in (0, 1, 6, 7):
            grt.trace_queue_rays(ctx, iteration, o, d, hits, o, d, md, light, words | np.where(np.arange(n) % 2 == 0, checks.FLAG_BOUNCE_0, np.uint32(0)).astype(np.uint32),
                                 frames, n + 100, merged=True)


@pytest.mark.parametrize("integrator,scheduler", [("path", "slots"), ("path", "merged"), ("ao", "slots")])
def test_the_probe_leaves_the_next_frame_unchanged(grt, oracle, integrator, scheduler):
    """A Cornell 96 x 64 frame rendered after a series of probe calls (every form) equals the frame rendered without them, bit for bit: under the
    slots scheduler, under the merged one, and in the AO integrator's context."""
    images = []
    for with_probe in (False, True):
        grt.config_reset()
        grt.config_set(num_bounces=4)
        scene = grt.Scene(grt.scene_path("cornellbox"))
        grt.config_set(num_bounces=4)
        pt = grt.AO(scene, 96, 64, device=0, radius=0.5) if integrator == "ao" else grt.Pathtracer(scene, 96, 64, device=0)
        if integrator == "path":
            grt.set_scheduler(pt.ctx, scheduler)
        pt.update()
        pt.render()
        if with_probe:
            probe_series(grt, oracle, pt)
        pt.update(); pt.render()
        images.append(pt.read_framebuffer().copy())
        pt.close(); scene.close()
    assert images[0].any()
    assert np.array_equal(images[0].view(np.uint32), images[1].view(np.uint32))


class RawCall:
    """rt_trace_queue_rays through ctypes on a small valid call, one argument changed per refusal."""

    def __init__(self, grt, oracle, pt, width=8):
        self.lib, self.ctx = grt.device_lib(), pt.ctx
        rng = np.random.default_rng(2)
        self.o = np.zeros((3, 4), np.float32) + np.array([[0.0], [1.0], [0.0]], np.float32)
        self.d = cases.normalised(rng.normal(size=(3, 4)))
        self.md = np.full(4, 0.5, np.float32)
        assert_safe(oracle, pt, self.o, self.d, self.md, width)
        self.light = np.ones((4, 3), np.float32)
        self.hits = np.zeros((4, 4), np.uint32)
        self.frames = [np.zeros((8, 4), np.float32) for _ in range(3)]
        self.stats = np.zeros(10, np.uint64)
        self.info = np.zeros(6, np.int32)

    def __call__(self, merged=0, step=1, form=0, closest=4, shadow=4, words=(0, 5, 2, 7), frame_pixels=8, null=(), stats=False):
        self.words = np.array(words, np.uint32)

        def ptr(name, a):
            return None if name in null else a.ctypes.data
        rays = [ptr("closest", a) for a in (self.o[0], self.o[1], self.o[2], self.d[0], self.d[1], self.d[2])]
        shadow_rays = [ptr("shadow", a) for a in (self.o[0], self.o[1], self.o[2], self.d[0], self.d[1], self.d[2])]
        status = self.lib.rt_trace_queue_rays(self.ctx, merged, step, form, *rays, closest, ptr("hits", self.hits), *shadow_rays, ptr("max_distance", self.md),
                                              ptr("illumination", self.light), ptr("words", self.words), shadow, *[ptr("frame%d" % k, f) for k, f in enumerate(self.frames)],
                                              frame_pixels, self.stats.ctypes.data if stats else None, ptr("info", self.info))
        return status, self.lib.rt_last_error(self.ctx).decode()


F = int(checks.FLAG_BOUNCE_0)
REFUSALS = [
    ("NULL closest-hit rays", "NULL closest-hit", dict(null=("closest",))),
    ("NULL hit array", "NULL closest-hit", dict(null=("hits",))),
    ("NULL shadow rays", "NULL shadow", dict(null=("shadow",))),
    ("NULL max_distance", "NULL shadow", dict(null=("max_distance",))),
    ("NULL illumination", "NULL shadow", dict(null=("illumination",))),
    ("NULL pixel words", "NULL shadow", dict(null=("words",))),
    ("NULL info", "NULL info", dict(null=("info",))),
    ("negative bounce", "bounce outside", dict(step=-1)),
    ("bounce RT_MAX_BOUNCES", "bounce outside", dict(step=MAX_BOUNCES)),
    ("negative iteration", "negative iteration", dict(merged=1, step=-1)),
    ("pixel at frame_pixels", "beyond the 8 pixels", dict(words=(0, 8, 2, 7))),
    ("pixel beyond frame_pixels, merged, flag stripped", "beyond the 8 pixels", dict(merged=1, words=(0, 9 | F, 2, 7))),
    ("bit 31 of a pixel word", "beyond the 8 pixels", dict(words=(0, 5 | (1 << 31), 2, 7))),
    ("one pixel twice", "appears twice", dict(words=(0, 5, 2, 5))),
    ("one pixel twice, merged, told apart only by the flag", "appears twice", dict(merged=1, words=(0, 5, 2, 5 | F))),
    ("flag in a per-bounce word", "flag", dict(words=(0, 5 | F, 2, 7))),
    ("more than 2^28 closest-hit rays", "2^28 rays", dict(closest=(1 << 28) + 1)),
    ("more than 2^28 shadow rays", "2^28 rays", dict(shadow=(1 << 28) + 1)),
    ("more than 2^28 rays together", "2^28 rays", dict(closest=1 << 27, shadow=(1 << 27) + 1)),
    ("more than 2^28 pixels", "2^28 pixels", dict(frame_pixels=(1 << 28) + 1)),
    ("merged neither 0 nor 1", "merged must be", dict(merged=2)),
    ("unknown form", "form must be", dict(form=3)),
    ("the AO form merged", "form must be", dict(merged=1, form=2)),
    ("the AO form at a later bounce", "AO form", dict(form=2, step=1, closest=0)),
    ("the AO form with closest-hit rays", "AO form", dict(form=2, step=0)),
    ("counting without stats10", "stats10", dict(form=1)),
    ("stats10 without counting", "stats10", dict(stats=True)),
]


@pytest.fixture(scope="module")
def cornell(grt):
    from conftest import make_pathtracer
    scene, pt = make_pathtracer(grt, "cornellbox", 32, 32, 0)
    yield pt
    pt.close(); scene.close()


@pytest.mark.parametrize("rule,words,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_probe_refuses(grt, oracle, cornell, rule, words, change):
    """One argument per rule: RT_ERROR_INVALID_ARG with a message that names the entry point and the rule, nothing written, before any launch -- and
    the context usable afterwards: the valid call goes through and delivers."""
    call = RawCall(grt, oracle, cornell)
    status, message = call(**change)
    assert status == -1 and "rt_trace_queue_rays" in message and words in message, (rule, status, message)
    assert not call.hits.any() and not any(f.any() for f in call.frames), "%s: the refused call wrote" % rule
    status, message = call()
    assert status == 0, message
    assert call.info[0] == 8 and call.hits.any()
    status, message = call(merged=1, step=3, words=(0, 5 | F, 2, 7))
    assert status == 0, message


@pytest.mark.parametrize("bvh_type", [2, 4])
def test_the_probe_refuses_counting_and_the_merged_form_on_other_widths(grt, oracle, bvh_type):
    """The counting kernels and the merged wavefront's launch walk the CWBVH only: refused under BVH2 / BVH4 before any launch; the plain per-bounce
    form and the AO form run there."""
    from conftest import make_pathtracer
    scene, pt = make_pathtracer(grt, "cornellbox", 32, 32, 0, bvh_type=bvh_type)
    try:
        call = RawCall(grt, oracle, pt, bvh_type)
        status, message = call(form=1, stats=True)
        assert status == -1 and "rt_trace_queue_rays: the counting kernels walk the CWBVH" in message, message
        status, message = call(merged=1, step=2)
        assert status == -1 and "rt_trace_queue_rays: the merged wavefront's launch walks the CWBVH" in message, message
        assert not call.hits.any() and not any(f.any() for f in call.frames)
        status, message = call()
        assert status == 0 and call.info[0] == bvh_type and call.hits.any(), message
        status, message = call(form=2, step=0, closest=0)
        assert status == 0, message
    finally:
        pt.close(); scene.close()
