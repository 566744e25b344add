"""The three generate launches -- kernel_generate, kernel_generate_stream, kernel_generate_stream_list -- entry by entry through
rt_generate_primary_rays, on the cases of tests/generate_cases.py: which (pixel, sample) every queue entry holds (tests/generate_reference.py,
exact), what the launch leaves alone (sentinels, the count word), each ray against the oracle and against float64 (the distances
tests/test_generate.py measures, times DEVICE_FACTOR), and that a (pixel, sample) pair's six floats are the same bits from every kernel, order, slot,
queue place, batch split, tile split and list."""
import ctypes

import numpy as np
import pytest

import generate_cases as cases
import generate_reference as ref

pytestmark = pytest.mark.gpu

RT_OK, RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY, RT_ERROR_OUT_OF_RANGE = 0, -1, -4, -5


class Rig:
    """One family at one frame size on the device, its expectation, and every ray the device has produced for it so far: ray[sample] is
    (pixels, 6) uint32 by scan-line index, seen[sample] says which rows are filled. A second launch must reproduce the bits."""
    def __init__(self, grt, oracle, directory, family, frame):
        self.family, self.frame = family, frame
        self.scene, self.pt = cases.load(grt, directory, family, *frame, 0)
        assert self.pt.pitch == ref.pitch_of(frame[0])
        self.expect = cases.Expectation(oracle, self.pt, family, *frame)
        self.ray, self.seen = {}, {}
        self.equal_directions = self.equal_origins = self.rays = 0
        self.worst_angle = self.worst_ulps = self.worst_oracle_angle = self.worst_oracle_ulps = 0.0

    def remember(self, label, scan, sample, six):
        for s in np.unique(sample):
            rows = sample == s
            if int(s) not in self.ray:
                self.ray[int(s)] = np.zeros((self.frame[0] * self.frame[1], 6), np.uint32)
                self.seen[int(s)] = np.zeros(self.frame[0] * self.frame[1], bool)
            table, seen = self.ray[int(s)], self.seen[int(s)]
            old = seen[scan[rows]]
            differ = (table[scan[rows]][old] != six[rows][old]).any(1)
            assert not differ.any(), "%s: sample %d: %d rays differ in their bits from an earlier launch, first pixel %d" % (label, s, differ.sum(), scan[rows][old][differ][0])
            table[scan[rows]] = six[rows]
            seen[scan[rows]] = True


@pytest.fixture(scope="module")
def rigs(grt, oracle, tmp_path_factory):
    directory = tmp_path_factory.mktemp("generate_cases_gpu")
    made = {}

    def rig(family, frame):
        if (family.name, frame) not in made:
            made[family.name, frame] = Rig(grt, oracle, directory, family, frame)
        return made[family.name, frame]
    yield rig
    for r in made.values():
        r.pt.close(); r.scene.close()
    grt.config_reset()


def launch(grt, rig, label, kernel, args, order=None, first=0, count=1, slot_base=0, before=0, offset=0, parity=0, rays_checked=True):
    """One launch, checked: layout, sentinels, count word, the order `info` reports, every ray against the oracle and float64, and the bits
    against every earlier launch of the rig. Returns (scan-line index, sample index, six floats as uint32) per entry."""
    w, h = rig.frame
    if kernel == ref.KERNEL_GENERATE:
        slot_base = before = offset = 0
    want_order = (0, 0) if kernel != ref.KERNEL_STREAM else ref.scheduler_order(w, h, **args) if order is None else tuple(order)
    words, scan, sample = ref.layout(kernel, w, h, want_order, first, count, slot_base, **args)
    rays, base = words.size, before + offset
    queue = np.full((7, base + rays + cases.GUARD), cases.SENTINEL, np.uint32)
    out, info = grt.generate_primary_rays(rig.pt.ctx, kernel, queue, first_sample=first, sample_count=count, slot_base=slot_base, iteration=4 + parity,
                                          queue_before=before, queue_offset=offset, order=None if order is None else want_order, **args)
    # 1. layout, exact
    assert tuple(info[:2]) == want_order, (label, info)
    pixels = rays // count
    assert info[2] == min(max(-(-(pixels if kernel == ref.KERNEL_GENERATE else rays) // 256), 1), 2048), (label, info)
    bad = np.nonzero(out[6, base:base + rays] != words)[0]
    assert bad.size == 0, "%s: %d of %d pixel words differ, first entry %d: %#x, want %#x" % (label, bad.size, rays, bad[0], out[6, base + bad[0]], words[bad[0]])
    assert (out[:, :base] == cases.SENTINEL).all(), "%s: the launch wrote in front of entry %d" % (label, base)
    assert (out[:, base + rays:] == cases.SENTINEL).all(), "%s: the launch wrote behind its %d rays" % (label, rays)
    assert info[3] == (rays if kernel == ref.KERNEL_GENERATE else before), (label, info)
    six = out[:6, base:base + rays].T.copy()
    floats = six.view(np.float32)
    assert np.isfinite(floats).all(), label
    rig.remember(label, scan, sample, six)
    if rays_checked and rays:
        family, e = rig.family, rig.expect
        # 2. and 3. against the oracle and against float64, matched by (pixel, sample)
        for name, want_o, want_d in (("oracle", e.gather("oracle_origin", scan, sample), e.gather("oracle_direction", scan, sample)),
                                     ("float64", e.gather("origin", scan, sample), e.gather("direction", scan, sample))):
            angle, ulps = ref.angle(floats[:, 3:], want_d), ref.origin_ulps(floats[:, :3], want_o)
            if name == "oracle":
                rig.worst_oracle_angle, rig.worst_oracle_ulps = max(rig.worst_oracle_angle, angle.max()), max(rig.worst_oracle_ulps, ulps.max())
                rig.equal_directions += int((floats[:, 3:] == want_d).all(1).sum()); rig.equal_origins += int((floats[:, :3] == want_o).all(1).sum()); rig.rays += rays
            else:
                rig.worst_angle, rig.worst_ulps = max(rig.worst_angle, angle.max()), max(rig.worst_ulps, ulps.max())
            assert angle.max() <= cases.DEVICE_FACTOR * family.direction_angle, "%s: direction %.3g rad from %s at entry %d (allowed %.3g)" % (label, angle.max(), name, angle.argmax(), cases.DEVICE_FACTOR * family.direction_angle)
            assert ulps.max() <= cases.DEVICE_FACTOR * family.origin_ulps, "%s: origin %.3g ulp from %s at entry %d (allowed %.3g)" % (label, ulps.max(), name, ulps.argmax(), cases.DEVICE_FACTOR * family.origin_ulps)
    return scan, sample, six


def test_layout_of_every_frame_submission_and_order(grt, rigs):
    """order x frame x submission, 4 samples into slots 3..6 (kernel_generate strides its grid: it is sized from the pixels): exact layout,
    sentinels, count word, reported order, every ray against the oracle and float64, the same bits whatever the order, submission or kernel."""
    launches = 0
    for frame in cases.FRAMES:
        rig = rigs(cases.DEFAULT_FAMILY, frame)
        for sub in cases.submissions(*frame):
            for order in sub.orders:
                launch(grt, rig, "%d x %d, %s, order %s" % (*frame, sub.name, order), sub.kernel, sub.args, order, 0, 4, 3)
                launches += 1
        assert all(rig.seen[s].all() for s in range(4)), frame
    assert launches > 150


def test_sample_batches_by_kernel(grt, rigs):
    """samples x kernel: slot 511 with sample 0 (the shifted sample index wraps), a batch across sample 4096, 16 samples, and the splits
    16 = 16 x 1 = 4 x 4 = 5 + 11 at other slots: the same bits."""
    frame = cases.RAY_FRAME
    rig = rigs(cases.DEFAULT_FAMILY, frame)
    n = frame[0] * frame[1]
    cells = ref.cell_list(*frame, [(cx, cy) for cy in range(-(-frame[1] // 16)) for cx in range(-(-frame[0] // 16))])
    assert np.array_equal(np.sort(cells), np.arange(n))
    submissions = ((ref.KERNEL_GENERATE, dict(pixel_count=n)), (ref.KERNEL_STREAM, dict(pixel_count=n)), (ref.KERNEL_STREAM_LIST, dict(pixel_list=cells)))
    for first, count, slot_base in cases.SAMPLES:
        for kernel, args in submissions:
            launch(grt, rig, "kernel %d, samples %d + %d at slot %d" % (kernel, first, count, slot_base), kernel, args, None, first, count, slot_base)
    for split in cases.SPLITS:
        for kernel, args in submissions:
            for k, (first, count) in enumerate(split):
                launch(grt, rig, "kernel %d, split %s" % (kernel, split), kernel, args, None, first, count, (37 * k + 11 * len(split)) % 400)
    assert all(rig.seen[s].all() for s in list(range(5, 21)) + [0, 1, 2, 3, 4094, 4095, 4096, 4097])


def test_queue_placement(grt, rigs):
    """Entries already in the queue (the count word) and queue_offset, on both parities: the rays land behind before + queue_offset, nothing else is
    written, the count word stays (kernel_stream_advance does the counting), the bits are the same."""
    frame = (9, 9)
    rig = rigs(cases.DEFAULT_FAMILY, frame)
    lists = cases.list_submissions(*frame)
    for before, offset, parity in cases.PLACEMENTS:
        launch(grt, rig, "before %d, offset %d, parity %d" % (before, offset, parity), ref.KERNEL_STREAM, dict(pixel_count=81), None, 0, 2, 5, before, offset, parity)
        launch(grt, rig, "list, before %d, offset %d, parity %d" % (before, offset, parity), ref.KERNEL_STREAM_LIST, lists[0].args, None, 0, 2, 9, before, offset, parity)


@pytest.mark.parametrize("family", cases.FAMILIES, ids=[f.name for f in cases.FAMILIES])
def test_filter_and_camera_families(grt, rigs, family):
    """filter x camera, all three kernels, batches at slots: rays against the oracle and float64 within the family's measured bounds, the same
    bits from every kernel, and the facts that need no tolerance. Prints the share of rays bit-equal to the oracle's (run with -s)."""
    frames = [cases.RAY_FRAME] + ([cases.WRAP_FRAME] if family is cases.DEFAULT_FAMILY else [])
    for frame in frames:
        rig = rigs(family, frame)
        w, h = frame
        n = w * h
        camera = rig.expect.camera
        position = camera.position.astype(np.float32).view(np.uint32)
        for first, count, slot_base in cases.family_samples(family):
            for kernel, args in ((ref.KERNEL_GENERATE, dict(pixel_count=n)), (ref.KERNEL_STREAM, dict(pixel_count=n)),
                                 (ref.KERNEL_STREAM_LIST, dict(pixel_list=np.arange(n - 1, -1, -1, dtype=np.uint32)))):
                label = "%s, %d x %d, kernel %d, samples %d + %d at slot %d" % (family.name, w, h, kernel, first, count, slot_base)
                scan, sample, six = launch(grt, rig, label, kernel, args, None, first, count, slot_base)
                if camera.aperture_radius == 0.0:
                    assert (six[:, :3] == position).all(), label   # pinhole origins: the camera position's bits
                    x, y = scan % w, scan // w
                    jitter = ref.recovered_jitter(x, y, six.view(np.float32)[:, 3:], camera)
                    margin = ref.recovery_margin(x, y, camera)
                    if family.svgf:   # every pixel of a sample: the table entry of (first + s) & 3, whatever the slot
                        want = ref.TAA_JITTER[:, sample & 3].T.astype(np.float64)
                        assert np.abs(jitter - want).max() <= margin, (label, np.abs(jitter - want).max(), margin)
                    elif family.filter == ref.FILTER_BOX:
                        assert jitter.min() >= -margin and jitter.max() < 1.0 + margin, (label, jitter.min(), jitter.max())
                    elif family.filter == ref.FILTER_TENT:
                        assert jitter.min() >= -1.0 - margin and jitter.max() <= 1.0 + margin, (label, jitter.min(), jitter.max())
        print("%-20s %3d x %-3d %6d rays: bit-equal to the oracle: directions %.3f, origins %.3f; worst against float64 %.3g rad, %.3g ulp; against the oracle %.3g rad, %.3g ulp"
              % (family.name, w, h, rig.rays, rig.equal_directions / rig.rays, rig.equal_origins / rig.rays, rig.worst_angle, rig.worst_ulps, rig.worst_oracle_angle, rig.worst_oracle_ulps))


def test_the_stream_kernels_second_grid_stride_round(grt, rigs):
    """256 x 136 x 16 samples: 557 056 rays for the 2 048 x 256 threads of the stream kernels' grid. Layout, and kernel against kernel."""
    frame = cases.STRIDE_FRAME
    rig = rigs(cases.DEFAULT_FAMILY, frame)
    n = frame[0] * frame[1]
    assert n * 16 > cases.GRID_THREADS
    cells = ref.cell_list(*frame, [(cx, cy) for cy in range(-(-frame[1] // 16)) for cx in range(frame[0] // 16)])
    launch(grt, rig, "stride, kernel_generate_stream", ref.KERNEL_STREAM, dict(pixel_count=n), None, 5, 16, 100, 64, 7, 1, rays_checked=False)
    launch(grt, rig, "stride, kernel_generate_stream_list", ref.KERNEL_STREAM_LIST, dict(pixel_list=cells), None, 5, 16, 300, 1, 0, 0, rays_checked=False)


def test_refusals_and_the_next_frame(grt):
    """Every refusal with its code and message and nothing written; and a frame rendered after probe calls equals the frame rendered without."""
    from conftest import make_pathtracer
    lib = grt.device_lib()
    images = []
    for with_probe in (False, True):
        scene, pt = make_pathtracer(grt, "cornellbox", 96, 64, 0, num_bounces=4)
        pt.render()
        if with_probe:
            ctx = pt.ctx
            frame_pixels = pt.pitch * 64
            out = np.full(64, cases.SENTINEL, np.uint32)
            info = np.full(4, 77, np.int32)
            seven, i = [out.ctypes.data] * 7, info.ctypes.data
            listed = np.array([5, 96 * 64], np.uint32)

            def call(kernel=1, iteration=0, first=0, count=1, offset=0, pixels=8, tiles=(0, 0, 0), slot=0, before=0, queue_offset=0, order=(-1, -1), plist=None, capacity=64, arrays=seven, info_pointer=i):
                return lib.rt_generate_primary_rays(ctx, kernel, iteration, first, count, offset, pixels, *tiles, slot, before, queue_offset, *order, plist, capacity, *arrays, info_pointer)
            name = "rt_generate_primary_rays: "
            refusals = [
                (lambda: call(arrays=seven[:3] + [None] + seven[4:]), RT_ERROR_INVALID_ARG, "NULL array"),
                (lambda: call(info_pointer=None), RT_ERROR_INVALID_ARG, "NULL array"),
                (lambda: call(kernel=3), RT_ERROR_INVALID_ARG, "kernel must be 0 (kernel_generate), 1 (kernel_generate_stream) or 2 (kernel_generate_stream_list)"),
                (lambda: call(pixels=-1), RT_ERROR_INVALID_ARG, "a count below zero"),
                (lambda: call(before=-1), RT_ERROR_INVALID_ARG, "a count below zero"),
                (lambda: call(queue_offset=-1), RT_ERROR_INVALID_ARG, "a count below zero"),
                (lambda: call(first=-1), RT_ERROR_INVALID_ARG, "a count below zero"),
                (lambda: call(count=0), RT_ERROR_INVALID_ARG, "sample_count must be 1..16"),
                (lambda: call(count=17, pixels=1), RT_ERROR_INVALID_ARG, "sample_count must be 1..16"),
                (lambda: call(slot=509, count=4), RT_ERROR_INVALID_ARG, "slot_base + sample_count beyond the 512 sample slots"),
                (lambda: call(kernel=0, slot=1), RT_ERROR_INVALID_ARG, "kernel_generate has no slot_base, queue count or queue_offset"),
                (lambda: call(kernel=2, offset=1, plist=listed.ctypes.data, pixels=1), RT_ERROR_INVALID_ARG, "kernel_generate_stream_list has no pixel_offset and no tiles"),
                (lambda: call(kernel=2, pixels=2), RT_ERROR_INVALID_ARG, "NULL pixel list"),
                (lambda: call(tiles=(96, 0, 0)), RT_ERROR_INVALID_ARG, "tile_stride must be at least 1 with tiles"),
                (lambda: call(order=(8, 0)), RT_ERROR_INVALID_ARG, "block_width and band_rows must both be -1 (the scheduler's choice), both 0 (scan lines) or, for kernel_generate_stream, both positive"),
                (lambda: call(capacity=0), RT_ERROR_INVALID_ARG, "capacity must be in [1, 2^28]"),
                (lambda: call(pixels=16, count=4, capacity=63), RT_ERROR_INVALID_ARG, "capacity below queue count + queue_offset + rays"),
                (lambda: call(pixels=50, before=10, queue_offset=5), RT_ERROR_INVALID_ARG, "capacity below queue count + queue_offset + rays"),
                (lambda: call(kernel=2, plist=listed.ctypes.data, pixels=2), RT_ERROR_INVALID_ARG, "list entry 1: pixel 6144 beyond the 6144 pixels of the frame"),
                (lambda: call(offset=96 * 64 - 7), RT_ERROR_OUT_OF_RANGE, "the last pixel of the range, 6144, lies beyond the 6144 pixel frame"),
                (lambda: call(tiles=(96 * 8, 7, 8), offset=96 * 8), RT_ERROR_OUT_OF_RANGE, "the last pixel of the range, 11527, lies beyond the 6144 pixel frame"),   # a second tile of rank 7 of 8
            ]
            assert (512 * frame_pixels) < 1 << 30   # (the 2^30 refusal needs a larger frame: below)
            for refusal, status, message in refusals:
                assert refusal() == status, message
                assert lib.rt_last_error(ctx).decode() == name + message
                assert (out == cases.SENTINEL).all() and (info == 77).all(), message
            # ... and launches that run, at both parities and through all three kernels
            queue = np.full((7, 96 * 64 * 2 + 9), cases.SENTINEL, np.uint32)
            for kernel, parity in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
                args = dict(pixel_list=np.arange(96 * 64, dtype=np.uint32)) if kernel == 2 else dict(pixel_count=96 * 64)
                grt.generate_primary_rays(ctx, kernel, queue, first_sample=3, sample_count=2, slot_base=0 if kernel == 0 else 100, iteration=6 + parity, queue_before=0 if kernel == 0 else 4, **args)
        pt.update(); pt.render()
        images.append(pt.read_framebuffer().copy())
        pt.close(); scene.close()
    assert np.array_equal(images[0], images[1])

    # (slot_base + sample_count) * frame_pixels >= 2^30: 512 slots of a 2048 x 1024 frame
    scene, pt = make_pathtracer(grt, "cornellbox", 2048, 1024, 0, num_bounces=2)
    out, info = np.full(64, cases.SENTINEL, np.uint32), np.zeros(4, np.int32)
    assert lib.rt_generate_primary_rays(pt.ctx, 1, 0, 0, 1, 0, 8, 0, 0, 0, 511, 0, 0, -1, -1, None, 64, *[out.ctypes.data] * 7, info.ctypes.data) == RT_ERROR_INVALID_ARG
    assert lib.rt_last_error(pt.ctx).decode() == "rt_generate_primary_rays: (slot_base + sample_count) * frame_pixels must be below 2^30"
    assert lib.rt_generate_primary_rays(pt.ctx, 1, 0, 0, 1, 0, 8, 0, 0, 0, 510, 0, 0, -1, -1, None, 64, *[out.ctypes.data] * 7, info.ctypes.data) == RT_OK
    assert (out[:8] != cases.SENTINEL).all() and (out[8:] == cases.SENTINEL).all()
    pt.close(); scene.close()

    # no RNG tables and no rt_resize: a bare context
    lib.rt_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    bare = ctypes.c_void_p()
    assert lib.rt_create(0, ctypes.byref(bare)) == RT_OK
    out = np.full(64, cases.SENTINEL, np.uint32)
    assert lib.rt_generate_primary_rays(bare, 1, 0, 0, 1, 0, 8, 0, 0, 0, 0, 0, 0, -1, -1, None, 64, *[out.ctypes.data] * 7, info.ctypes.data) == RT_ERROR_NOT_READY
    assert lib.rt_last_error(bare).decode() == "rt_generate_primary_rays: RNG tables not uploaded or rt_resize not called"
    assert (out == cases.SENTINEL).all()
    lib.rt_destroy(bare)
    grt.config_reset()
