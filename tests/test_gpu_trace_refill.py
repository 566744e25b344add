"""The refill path of the merged wavefront's traversal launch (kernels_trace.hip, bvh8_trace_engine): how rays are dealt at the ends
of blocks, region pieces and queues, and the per-wave list of shadow rays whose contribution to the frame is added later, by all
lanes of the wave together (contribution_flush) -- through rt_trace_stream_rays, where shadow ray i adds (1, 0, 0) to pixel i of a
zeroed frame: float32(0) + float32(1) = 1 for a ray that reached its light, 0 for an occluded one; a lost flush shows as 0 where
1 is due, a doubled one as 2. Whole frames are compared with digests recorded before the list existed (tests/refill_frames.py).

The oracle is asked once per scene, for the base rays; a queue of any length repeats them (a ray's result and its node and
triangle counts do not depend on where in a queue it stands), so the counting kernel's counters are sums of the oracle's.
"""
import json
import os

import numpy as np
import pytest

import refill_frames
import trace_cases as cases
import trace_checks as checks

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xA5A5A5A5)
KERNEL_GENERAL, KERNEL_FLAT, KERNEL_FLAT_SKIP, KERNEL_COUNTING = 0, 1, 2, 3
NARROW_MAX, MIXED_MAX = 16384, 10 * 1024 * 1024
COUNTERS = ("nodes", "triangles", "instances_transformed", "instances_identity", "rays")


class Rays:
    """A case's rays and six shadow rays per ray, with the oracle's answers; queues of any length repeat them in order."""

    def __init__(self, grt, oracle, case, **config):
        self.case, self.grt = case, grt
        self.scene, self.pt = checks.load(grt, case, 0, **config)
        self.view = oracle.SceneView(self.pt)
        self.o, self.d = case.origin, case.direction
        self.hits, stats = self.view.trace(self.o, self.d)
        _, tri, t, _, _ = checks.unpack(self.hits)
        self.md = cases.shadow_limits(np.where(tri >= 0, t, np.inf), np.random.default_rng(7))
        self.so, self.sd = np.repeat(self.o, 6, 1), np.repeat(self.d, 6, 1)
        self.occluded, shadow_stats = self.view.trace_shadow(self.so, self.sd, self.md)
        assert stats.max_stack <= checks.STACK_LIMIT and shadow_stats.max_stack <= checks.STACK_LIMIT   # (before any launch: the device does not check its spill index)
        self.light = (np.float32(0.0) + (np.float32(1.0) - self.occluded.astype(np.float32))).astype(np.float32)   # what the launch leaves in pixel i, in float32
        self.n, self.m = self.o.shape[1], self.so.shape[1]
        self._sums = {}

    def close(self):
        self.pt.close(); self.scene.close()

    def counters(self, shadow, count):
        """The oracle's counters of the first `count` rays of the repeated queue: whole repeats of the base plus the rest."""
        base = self.m if shadow else self.n

        def of(k):
            if (shadow, k) not in self._sums:
                if k == 0:
                    self._sums[shadow, k] = np.zeros(len(COUNTERS), np.int64)
                else:
                    _, st = self.view.trace_shadow(self.so[:, :k], self.sd[:, :k], self.md[:k]) if shadow else self.view.trace(self.o[:, :k], self.d[:, :k])
                    self._sums[shadow, k] = np.array([getattr(st, name) for name in COUNTERS], np.int64)
            return self._sums[shadow, k]
        return (count // base) * of(base) + of(count % base)

    def launch(self, iteration, nc, ns, counting=False, shadow_index=None):
        """One launch of nc closest-hit and ns shadow rays (shadow ray j is base ray shadow_index[j], default j mod m); checks every
        record and every pixel and returns info."""
        ci = np.arange(nc) % self.n
        si = np.arange(ns) % self.m if shadow_index is None else shadow_index
        hits = np.full((nc, 4), SENTINEL, np.uint32)
        hits, light, stats, info = self.grt.trace_stream_rays(self.pt.ctx, iteration, self.o[:, ci], self.d[:, ci], hits, self.so[:, si], self.sd[:, si], self.md[si], counting=counting)
        label = "%s: %d + %d rays, iteration %d%s" % (self.case.name, nc, ns, iteration, ", counting" if counting else "")
        undealt = int((hits == SENTINEL).all(1).sum())
        assert undealt == 0, "%s: %d closest-hit rays never dealt" % (label, undealt)
        bad = np.nonzero((hits != self.hits[ci]).any(1))[0]
        assert bad.size == 0, "%s: %d hits differ from the oracle, first ray %d: %s against %s" % (label, bad.size, bad[0], hits[bad[0]].tolist(), self.hits[ci][bad[0]].tolist())
        want = self.light[si]
        bad = np.nonzero(light.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, ("%s: %d pixels differ, first shadow ray %d holds %r where %r is due (0 for 1: never dealt or its contribution lost, 2: added twice); values %s"
                               % (label, bad.size, bad[0], float(light[bad[0]]), float(want[bad[0]]), sorted(set(light[bad].tolist()))[:8]))
        if counting:
            assert info[0] == KERNEL_COUNTING, (label, info)
            for kind, shadow, count in (("closest", False, nc), ("shadow", True, ns)):
                if shadow_index is None or not shadow:
                    want_counters = dict(zip(COUNTERS, (int(x) for x in self.counters(shadow, count))))
                    assert stats[kind] == want_counters, (label, kind, stats[kind], want_counters)
        return info


@pytest.fixture(scope="module")
def case_directory(tmp_path_factory):
    return str(tmp_path_factory.mktemp("trace_refill_gpu"))


@pytest.fixture(scope="module")
def boxes(grt, oracle, case_directory):
    rays = Rays(grt, oracle, cases.case_boxes(case_directory))
    yield rays
    rays.close()


def grid_waves(rays):
    info = rays.launch(0, 0, 0)
    assert info[0] == KERNEL_FLAT_SKIP and info[2] == NARROW_MAX and info[3] == MIXED_MAX, info
    assert info[1] >= 64
    return int(info[1])


def splits_of(total, k):
    """Odd closest-hit / shadow splits of a queue length, and the queue of either kind alone."""
    a = total // 3 if k % 2 else total - total // 5
    return [(a, total - a), (total, 0), (0, total)]


SMALL = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 256 + 63, 256 + 64, 256 + 65)


def test_dealing_at_the_ends_of_blocks_pieces_and_queues(boxes):
    """Queue lengths at which a 64-ray piece, a 256-ray block or a queue ends, both parities, odd splits and either queue empty.
    Up to RT_NARROW_MAX_RAYS rays the plain launch runs the narrow engine and the counting launch the wide mixed one; beyond, both
    run the mixed engine with the endgame's regions (W x 64 and W x 256: where the region size changes). Every hit equals the
    oracle's, every pixel holds what its shadow ray owes, no record keeps its sentinel, the counters equal the oracle's."""
    W = grid_waves(boxes)
    k = 0
    for total in SMALL:
        for nc, ns in splits_of(total, k):
            for counting in (False, True):
                boxes.launch((k >> 1) & 1, nc, ns, counting)   # (either parity with either kernel)
                k += 1
    for total in (W * 64 - 1, W * 64 + 1, W * 256 - 1, W * 256 + 1):
        for nc, ns in splits_of(total, k):
            info = boxes.launch(k & 1, nc, ns, counting=total == W * 64 + 1)
            assert NARROW_MAX < nc + ns <= info[3]
            k += 1
    # the kind changes inside a piece: a short queue in front of a long one and behind it
    for nc, ns in ((1, W * 64 + 63), (65, W * 64), (257, W * 64 + 1), (W * 64 + 63, 1), (W * 64, 65), (W * 64 + 1, 257)):
        boxes.launch(k & 1, nc, ns)
        k += 1


def test_dealing_in_the_flat_and_the_general_kernel(grt, oracle, case_directory):
    """The same on the flat kernel without the skipping walk and on an instanced scene's general kernel (40 instances under the
    TLAS), at fewer lengths."""
    for case, config, kernel in ((cases.case_boxes(case_directory), {"skip_behind_hit": 0}, KERNEL_FLAT), (cases.case_instanced(case_directory, "instanced", 40, 17), {}, KERNEL_GENERAL)):
        rays = Rays(grt, oracle, case, **config)
        info = rays.launch(0, 0, 0)
        W = int(info[1])
        assert info[0] == kernel, (case.name, info)
        k = 0
        for total in (65, 257, 256 + 65, W * 64 + 1):
            for nc, ns in splits_of(total, k):
                rays.launch(k & 1, nc, ns, counting=total == 257)
                k += 1
        rays.close()


def test_the_split_engines_hand_over_at_short_queues(boxes):
    """Above RT_MIXED_MAX_RAYS the closest-hit engine runs first and the shadow engine after it, each on its own queue: shadow
    queues that end inside the first piece, the first block and past a region, behind 10 M closest-hit rays."""
    W = grid_waves(boxes)
    for k, ns in enumerate((65, 257, W * 64 + 129)):
        info = boxes.launch(k & 1, MIXED_MAX + 1 - (k & 1) * 64, ns)
        assert MIXED_MAX < MIXED_MAX + 1 - (k & 1) * 64 + ns and info[0] == KERNEL_FLAT_SKIP


def test_the_contribution_list_at_its_thresholds(boxes):
    """W x 256 shadow rays are dealt as one 256-ray region per wave. Of region r the first K[r mod 8] rays reach their light (the
    lane appends to its wave's list) and the rest are occluded (nothing to append), K = 63, 64, 65, 127, 128, 129, 0, 256: waves
    that collect one entry less than, exactly and one more than the 64 entries at which the list is flushed before a refill, and
    than its 128 slots -- and waves that leave with 63, 64, 1, ... entries still listed, which the lanes that leave must flush.
    Then queues whose rays all append, never append and alternate, ending inside a piece; once behind a closest-hit queue that
    moves every region by an odd offset, once through the counting kernel."""
    W = grid_waves(boxes)
    lit, dark = np.nonzero(boxes.occluded == 0)[0], np.nonzero(boxes.occluded != 0)[0]
    assert lit.size > 256 and dark.size > 256

    def pick(reaches):   # shadow ray j: a base ray that reaches its light where reaches[j], else an occluded one (both cycled through)
        j = np.arange(reaches.size)
        return np.where(reaches, lit[j % lit.size], dark[j % dark.size])

    K = np.array((63, 64, 65, 127, 128, 129, 0, 256))
    position = np.arange(W * 256)
    by_region = (position % 256) < K[(position // 256) % 8]
    boxes.launch(1, 0, W * 256, shadow_index=pick(by_region))
    boxes.launch(0, 0, W * 256, counting=True, shadow_index=pick(by_region))
    nc = 1000 * 256 + 37   # (the regions are cut from both queues as one: shadow ray j stands at nc + j)
    shifted = ((position + nc) % 256) < K[((position + nc) // 256) % 8]
    boxes.launch(1, nc, W * 256 - nc, shadow_index=pick(shifted[:W * 256 - nc]))
    tail = W * 64 + 129
    for reaches in (np.ones(tail, bool), np.zeros(tail, bool), np.arange(tail) % 2 == 0, np.arange(tail) % 3 != 0):
        boxes.launch(0, 0, tail, shadow_index=pick(reaches))
    # the narrow engine (a ray per 8-lane group: the group's first lane appends): 2048 groups' worth and an odd rest
    for ns in (63, 64 * 8 + 1, 129 * 8, NARROW_MAX):
        boxes.launch(1, 0, ns, shadow_index=pick(np.ones(ns, bool)))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refill_frames.json")


@pytest.mark.parametrize("scene_name", refill_frames.SCENES)
def test_frames_are_what_they_were(grt, scene_name):
    """Two 4-sample frames at 64 x 64 with 10 bounces through the merged wavefront, as a declared burst and one submission per
    iteration: every float of the framebuffer as the commit before the contribution list rendered it (radiance, and through it
    the direct and indirect frames' arithmetic: `=` for bounce 0, `+=` after it)."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert (golden["width"], golden["height"], golden["spp"], golden["bounces"], golden["frames"]) == (refill_frames.W, refill_frames.H, refill_frames.SPP, refill_frames.BOUNCES, refill_frames.FRAMES)
    images = {}
    for burst in (True, False):
        image, counts = refill_frames.render(grt, scene_name, burst)
        assert sum(counts[1]) == golden["shadow_rays"][refill_frames.key(scene_name, burst)]
        assert refill_frames.digest(image) == golden["sha256"][refill_frames.key(scene_name, burst)], (scene_name, burst)
        images[burst] = image
    assert np.array_equal(images[True], images[False])
