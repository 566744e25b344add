"""The restatement of the generate stage (tests/generate_reference.py) on the cases of tests/generate_cases.py, without a device: the queue layout is a
permutation of every submission's pixels, the band walk keeps 8 x 8 patches together, tiles partition the frame, scan-line order is the oracle's,
and the float64 ray agrees with the oracle's float32 ray for every ray of every family -- by the distances this module measures and
generate_cases.FAMILIES records, which bound the device in tests/test_gpu_generate.py."""
import numpy as np
import pytest

import generate_cases as cases
import generate_reference as ref


def resolved(width, height, sub, order):
    return ref.scheduler_order(width, height, **sub.args) if order is None else order


def test_the_layout_is_a_permutation_of_the_submissions_pixels():
    checked = 0
    for w, h in cases.FRAMES + [cases.STRIDE_FRAME]:
        assert ref.pitch_of(w) % 32 == 0 and 0 <= ref.pitch_of(w) - w < 32
        for sub in cases.submissions(w, h):
            want = cases.submission_set(w, h, sub)
            assert np.unique(want).size == want.size and (want.size == 0 or (want[0] >= 0 and want[-1] < w * h)), (w, h, sub.name)
            for order in sub.orders:
                for first, count, slot_base in ((0, 1, 0), (0, 4, 3)):
                    words, scan, sample = ref.layout(sub.kernel, w, h, resolved(w, h, sub, order), first, count, slot_base, **sub.args)
                    assert words.size == want.size * count and np.unique(words).size == words.size, (w, h, sub.name, order)
                    for s in range(count):
                        rows = slice(s * want.size, (s + 1) * want.size)
                        assert np.array_equal(np.sort(scan[rows]), want), (w, h, sub.name, order, s)
                        assert (sample[rows] == first + s).all()
                        slot = s + (0 if sub.kernel == ref.KERNEL_GENERATE else slot_base)
                        x, y = scan[rows] % w, scan[rows] // w
                        assert np.array_equal(words[rows], slot * ref.pitch_of(w) * h + x + y * ref.pitch_of(w))
                    checked += 1
    assert checked > 300


def test_sixty_four_consecutive_entries_of_an_unclipped_band_cover_one_patch():
    for w, h in ((8, 8), (64, 8), (40, 20), (33, 17), (136, 24)):
        _, scan, _ = ref.layout(ref.KERNEL_STREAM, w, h, (8, 8), pixel_count=w * h)
        patches = 0
        for band in range(h // 8):             # the whole bands ...
            for block in range(w // 8):        # ... and in them the whole blocks
                k = band * 8 * w + block * 64
                x, y = scan[k:k + 64] % w, scan[k:k + 64] // w
                assert np.array_equal(x, np.tile(np.arange(block * 8, block * 8 + 8), 8)) and np.array_equal(y, np.repeat(np.arange(band * 8, band * 8 + 8), 8)), (w, h, band, block)
                patches += 1
        assert patches == (h // 8) * (w // 8) >= 1
    # the cells of a pixel list are in the same order
    cell = ref.cell_list(40, 20, [(0, 0)])
    _, scan, _ = ref.layout(ref.KERNEL_STREAM, 40, 20, (8, 8), pixel_count=800)
    assert np.array_equal(cell[:128], np.concatenate([scan[0:64], scan[64:128]]))


def test_the_tiles_of_all_ranks_partition_the_frame():
    for w, h in cases.FRAMES:
        by_split = {}
        for sub in cases.tile_submissions(w, h):
            tile_pixels, rank, ranks = sub.args["tiles"]
            by_split.setdefault((tile_pixels, ranks), []).append(cases.submission_set(w, h, sub))
        for key, sets in by_split.items():
            assert len(sets) == key[1]
            assert np.array_equal(np.sort(np.concatenate(sets)), np.arange(w * h)), (w, h, key)
    assert sum(1 for w, h in cases.FRAMES if cases.tile_submissions(w, h)) >= 5
    # the rank that owns the clipped last tile has fewer pixels than whole tiles
    assert ref.tile_count(40, 20, 320, 2, 3) == 160 and ref.tile_count(40, 20, 320, 0, 2) == 480 and ref.tile_count(33, 17, 264, 0, 2) == 264 + 33


def test_the_schedulers_choice_is_patches_for_whole_bands_only():
    assert ref.scheduler_order(40, 20, pixel_count=800) == (8, 8)
    assert ref.scheduler_order(40, 20, pixel_count=ref.tile_count(40, 20, 320, 1, 2), tiles=(320, 1, 2)) == (8, 8)
    assert ref.scheduler_order(40, 20, pixel_offset=43, pixel_count=85) == (0, 0)
    assert ref.scheduler_order(40, 20, pixel_offset=0, pixel_count=799) == (0, 0)
    assert ref.scheduler_order(40, 20, pixel_count=ref.tile_count(40, 20, 120, 0, 2), tiles=(120, 0, 2)) == (0, 0)
    assert ref.scheduler_order(40, 20, pixel_list=np.arange(5)) == (0, 0)


@pytest.fixture(scope="module")
def expectations(grt, oracle, tmp_path_factory):
    """(family name, frame) -> Expectation on a scene staged without a device."""
    directory = tmp_path_factory.mktemp("generate_cases")
    out, keep = {}, []
    for family in cases.FAMILIES:
        for frame in [cases.RAY_FRAME] + ([cases.WRAP_FRAME] if family is cases.DEFAULT_FAMILY else []):
            scene, pt = cases.load(grt, directory, family, *frame, -1)
            assert pt.pitch == ref.pitch_of(frame[0])
            cam, cfg = pt.camera(), pt.device_config()
            assert cfg.reconstruction_filter == family.filter and cfg.enable_svgf == family.svgf
            assert (cam.aperture_radius > 0.1) == ("thin" in family.camera.name)
            out[family.name, frame] = cases.Expectation(oracle, pt, family, *frame)
            keep.append((scene, pt))
    yield out
    for scene, pt in keep:
        pt.close(); scene.close()
    grt.config_reset()


def family_sample_indices(family):
    return sorted({first + s for first, count, _ in cases.family_samples(family) for s in range(count)})


def test_scan_line_order_reproduces_the_oracles_pixel_words(expectations):
    for (name, (w, h)), e in expectations.items():
        for offset, count in ((0, w * h), (w + 3, 2 * w + 5)):
            _, _, px = e.view.generate(0, offset, count)
            for kernel in (ref.KERNEL_GENERATE, ref.KERNEL_STREAM):
                words, _, _ = ref.layout(kernel, w, h, (0, 0), pixel_offset=offset, pixel_count=count)
                assert np.array_equal(words, px), (name, w, h, kernel)


def test_no_draw_is_degenerate_and_the_reference_is_finite(expectations):
    """No filter draw is exactly 0 (logf(0)) and no aperture draw exactly (0.5, 0.5) (0 / 0 in the disk map): no ray is excluded anywhere."""
    rays = 0
    for (name, frame), e in expectations.items():
        for index in family_sample_indices(e.family):
            s = e.sample(index)
            assert (s["u_filter"] > 0).all() and (s["u_filter"] < 1).all() and not (s["u_aperture"] == 0.5).all(1).any(), (name, index)
            for key in ("origin", "direction", "oracle_origin", "oracle_direction"):
                assert np.isfinite(s[key]).all(), (name, index, key)
            rays += s["origin"].shape[0]
    assert rays > 30000


def test_the_oracle_stays_within_the_measured_distance_of_float64(expectations):
    """Measures, per family, the oracle's largest angle to the float64 direction and its largest origin difference in ulps of the origin's largest
    coordinate (printed: run with -s), and holds them to the constants of generate_cases.FAMILIES, which are these figures rounded up."""
    for family in cases.FAMILIES:
        angle, ulps = 0.0, 0.0
        for (name, frame), e in expectations.items():
            if name != family.name:
                continue
            for index in family_sample_indices(family):
                s = e.sample(index)
                angle = max(angle, float(ref.angle(s["oracle_direction"], s["direction"]).max()))
                ulps = max(ulps, float(ref.origin_ulps(s["oracle_origin"], s["origin"]).max()))
        print("%-20s oracle against float64: direction %.3g rad, origin %.3g ulp" % (family.name, angle, ulps))
        assert angle <= family.direction_angle and ulps <= family.origin_ulps, (family.name, angle, ulps)
        assert family.direction_angle <= 2.0 * max(angle, 2.0 ** -24) and family.origin_ulps <= max(2.0 * ulps, 0.5), (family.name, angle, ulps)   # rounded up, not padded
    # The bounds the suite already uses for kernel_generate at one sample, absolute per component: directions 3e-7 (pinhole Gaussian), 5e-7 and
    # origins 1e-6 (thin lens at |position| 7: 2.1 ulp). Twice the measured figures stay below them.
    by_name = {f.name: f for f in cases.FAMILIES}
    assert cases.DEVICE_FACTOR * by_name["gaussian pinhole"].direction_angle < 3e-7
    assert cases.DEVICE_FACTOR * by_name["gaussian thin lens"].direction_angle < 5e-7
    assert cases.DEVICE_FACTOR * by_name["gaussian thin lens"].origin_ulps * 2.0 ** -21 < 1e-6


def test_pinhole_and_svgf_facts_of_the_reference(expectations):
    """What the GPU test asserts without a tolerance holds for the restatement: pinhole origins are the camera position, the jitter recovered from a
    float64 direction is the jitter that made it, box jitter lies in [0, 1), tent jitter in [-1, 1], the SVGF jitter is the table entry."""
    for (name, (w, h)), e in expectations.items():
        family = e.family
        if "thin" in family.camera.name:
            continue
        scan = np.arange(w * h)
        x, y = scan % w, scan // w
        for index in family_sample_indices(family):
            s = e.sample(index)
            assert (s["origin"] == e.camera.position).all()
            assert (s["oracle_origin"] == e.camera.position.astype(np.float32)).all()
            j = ref.recovered_jitter(x, y, s["direction"], e.camera)
            want = ref.jitter(s["u_filter"], family.filter, family.svgf, np.full(scan.size, index))
            assert np.abs(j - want).max() < 1e-9 * max(w, h), name
            if family.svgf:
                assert (want == ref.TAA_JITTER[:, index & 3].astype(np.float64)).all()
            elif family.filter == ref.FILTER_BOX:
                assert (want >= 0).all() and (want < 1).all()
            elif family.filter == ref.FILTER_TENT:
                assert (want >= -1).all() and (want <= 1).all()
            assert ref.recovery_margin(x, y, e.camera) < 1e-3, name
