"""Comparisons shared by test_sort.py (oracle against float64, CPU) and test_gpu_sort.py (device against oracle and float64).

Queue order is unspecified: entries are matched by their virtual pixel, which is unique within a launch.

Structure (exact, every launch; check_structure): the counters; positions [0, count) of every queue hold one entry each, no pixel twice, no
input entry in two queues; every word at or beyond `count`, and every field the kernel must not write (the medium of an entry outside a
medium, the cone fields at bounce 0 or with mip-mapping off, the throughput at bounce 0, the hit and last_pdf of a continuation ray, the
padding), still holds the sentinel; frame and g-buffer pixels that no entry names, and frames float64 says an entry leaves alone, are
untouched; every entry ends in an outcome float64 allows it; merged: the statistics rows equal the counts recomputed from the matched
entries, every other row is zero.

Device against oracle, bit for bit (check_identical; NaN equal to NaN): the entries outside every medium that are no misses. Read side by
side, that path of sort_rays and of the oracle's kernel_sort is + - * /, sqrtf (normalize of the emitter's normal), fabsf, fmaxf / fminf
(saturate, the roulette's maximum) and comparisons, on both sides without contraction. What is NOT on it, and is therefore compared with
float64 under measured bounds instead: expf (beer_lambert: every entry inside a medium, the purely absorbing one included -- not only the
scattering media), logf (sample_exp), sincosf (the phase function), atan2f and acosf (sample_sky, sky_pdf: every miss).

Device against float64 (compare_with_reference), for the robust entries: the errors below were measured on the ORACLE against
sort_reference.py over every launch of test_sort.py (which prints them and asserts the oracle stays within the bound); the bound is 3 x the
worst case, and the device is held to the same number.

    quantity     worst oracle error   launch                                 bound
    throughput   5.76e-07             default/length_1310720                 1.75e-06  max |a - b| / max |b| over the channels of a stored throughput
    origin       1.91e-07             default/length_524289                  5.8e-07   scattered origin, relative to max |origin| + distance
    direction    2.16e-06             default/length_1310720_merged          6.5e-06   scattered direction, max |a - b| / (1 + 1 / sin(theta)): the sine of the
                                                                                       scattering angle is sqrt(1 - cos^2), which magnifies the cosine's rounding near the poles
    cone_width   1.27e-07             default/inside_medium_at_bounce0       3.9e-07   pixel_spread_angle * distance at bounce 0, relative
    aov          3.15e-06             default/length_524288                  9.5e-06   a frame's rgb after the launch, relative to max(|b|, |before|) and, for a miss, to
                                                                                       throughput x the sky's largest texel (the lookup's error is a position error times
                                                                                       the difference of neighbouring texels)
    gbuffer      8.55e-08             svgf_on/mixed_bounce0                  2.6e-07   g-buffer floats, relative to max(1, |b|)

    comparison                      quantity      worst oracle error                      launch                           margin
    scatter_distance < t            distance      1.43e-07 relative                       default/length_1310720           4.35e-07
    three-way wavelength choice     r * sum       1.53e-07 of the throughput's sum        default/length_1310720_merged    4.65e-07
    r > survival_probability        survival      4.72e-07 relative                       svgf_on/mixed_bounce1            1.45e-06
    pdf_is_valid(light_pdf)         light_pdf     1.11e-07 x (1 + 1 / cos_theta_light)    default/length_524288            3.4e-07 x (1 + 1 / cos)
    sky cell of a direction         u, v          1.16e-07 absolute                       sky_share_0.5/length_524289_merged  3.5e-07
    (the margins' errors are taken over the robust entries, on which both sides take the same branches; non-robust entries measured in the
    launches of random entries: at most 1 per launch)

Decisions next to a threshold. An entry is robust when every comparison it takes clears its threshold, in float64, by more than the margin;
the margin is 3 x the worst error of the compared quantity, measured in the same run from the float32 intermediates oracle_sort reports
(light_pdf: the cosine is a dot product of unit vectors, its error is absolute; relative to the pdf it grows as 1 / cos, so error and margin
are stated as multiples of 1 + 1 / cos_theta_light. An entry is also non-robust where the float32 denominator cos * total_weight is denormal,
where light_pdf is within a factor 2 of the largest float, where t is infinite, and where a NaN is met: float64 cannot say which float32
operation overflows first.)

Robust entries take float64's outcome exactly, on the oracle and on the device. The others are excused from that and from the value bounds,
not from the structure rules. At most 0.5 % of the entries of a launch that reach such a comparison may be non-robust (asserted in
test_sort.py). Launches that sit on a threshold on purpose are exempt from the cap, by name:
    emitter_edges_*   light_pdf just below / above 1e-4, grazing and denormal cosines, t * t under- and overflowing -- outside every medium: bit for bit with the oracle
    roulette_edges    survival probability equal to the random number and its float neighbours -- outside every medium: bit for bit with the oracle
    medium_edges      free-flight distance equal to t and its float neighbours, all-zero throughput (NaN): through logf / expf, so not bit for bit;
                      the threshold entries obey the structure rules; the NaN entries must also show the oracle's outcome and NaN in the same fields (check_nan_pattern)
    sky_directions    directions on cell borders of the sky table (the _sky instances): through atan2f / acosf; the structure rules alone
"""
import numpy as np

import sort_reference as ref
from sort_reference import TRACE_WORDS, MATERIAL_WORDS, SCATTERED, TERMINATED, OUTCOME_NAMES

BOUNDS = {"throughput": 1.75e-06, "origin": 5.8e-07, "direction": 6.5e-06, "cone_width": 3.9e-07, "aov": 9.5e-06, "gbuffer": 2.6e-07}
MARGINS = {"distance": 4.35e-07, "wavelength": 4.65e-07, "survival": 1.45e-06, "light_pdf": 3.4e-07, "sky_uv": 3.5e-07}
THRESHOLD_LAUNCHES = ("emitter_edges_", "roulette_edges", "medium_edges", "sky_directions")
NON_ROBUST_CAP = 0.005
PIXEL_MASK = np.uint32(0x3fffffff)
STAT_TRACE, STAT_SHADOW, STAT_DIFFUSE = 0, 1, 2


class Outputs:
    """What a launch left behind, from the device (rt_sort_rays) or the oracle (oracle_sort per sample slot, joined)."""


def device_launch(grt, ctx, launch, sentinel, capacity=None):
    r = grt.sort_rays(ctx, launch.entries.pack(), launch.frame_pixels, launch.frame_slots, bounce=launch.bounce, sample_index=launch.sample_index,
                      iteration=launch.iteration, slot_table=launch.slot_table, submission_birth=launch.submission_birth, capacity=capacity, sentinel=sentinel,
                      aov=launch.aov, gbuffer_normal_and_depth=launch.gnd, gbuffer_ids=launch.gid, gbuffer_screen_prev=launch.gsp)
    o = Outputs()
    o.trace_out, o.material_out, o.counters, o.aov, o.gnd, o.gid, o.gsp, o.stats = r.trace_out, r.material_out, r.counters, r.aov, r.gbuffer_normal_and_depth, r.gbuffer_ids, r.gbuffer_screen_prev, r.stats
    o.pixel_query = r.pixel_query.copy()
    return o


def oracle_launch(tables, launch, sentinel):
    """The launch through oracle_sort: one call per sample slot (the oracle knows pixels and samples, not virtual pixels), queues joined in slot order."""
    e = launch.entries
    slot, real, bounce, sample, submission, first = launch.paths()
    capacity = max(e.n, 1)
    o = Outputs()
    o.trace_out = np.full((capacity, TRACE_WORDS), sentinel, np.uint32); o.material_out = np.full((4, capacity, MATERIAL_WORDS), sentinel, np.uint32)
    o.counters = np.zeros(6, np.int32); o.counters[5] = e.n
    o.aov, o.gnd, o.gid, o.gsp = launch.aov.copy(), launch.gnd.copy(), launch.gid.copy(), launch.gsp.copy()
    o.pixel_query = np.full(2, sentinel, np.uint32).view(np.int32)
    o.internals = np.full((e.n, 8), np.nan, np.float32)
    o.stats = None
    fp = launch.frame_pixels
    table = None if tables.sky_share <= 0 else tables.sky_tables.pdf.astype(np.float32)
    for s in np.unique(slot):
        index = np.nonzero(slot == s)[0]
        part = e.take(index)
        base = int(s) * fp
        answers = bool(first[index[0]]) if launch.merged else s == 0
        trace, material, counts, internals = tables.view.sort(
            part.pack(pixel=real[index]), int(bounce[index[0]]), int(sample[index[0]]), [o.aov[k, base:base + fp] for k in range(4)],
            o.gnd[base:base + fp], o.gid[base:base + fp], o.gsp[base:base + fp], sentinel=sentinel, aov_enabled=tables.aov_enabled,
            pixel_query_pixel=tables.pixel_query if answers else -1, pixel_query=o.pixel_query if answers else None, sky_share=tables.sky_share, sky_cell_pdf=table)
        o.internals[index] = internals
        n = counts[4]
        rows = trace[:n].copy(); rows[:, 10] += np.uint32(base)
        o.trace_out[o.counters[4]:o.counters[4] + n] = rows; o.counters[4] += n
        for m in range(4):
            n = counts[m]
            rows = material[m, :n].copy(); rows[:, 7] += np.uint32(base)
            o.material_out[m, o.counters[m]:o.counters[m] + n] = rows; o.counters[m] += n
    return o


def match(launch, out, name):
    """Per input entry: its outcome (0..3 material queue, SCATTERED, TERMINATED) and the record it became (N, 20; material records fill 16 words)."""
    e = launch.entries
    order = np.argsort(e.pixel, kind="stable")
    sorted_pixels = e.pixel[order]
    outcome = np.full(e.n, TERMINATED)
    records = np.zeros((e.n, TRACE_WORDS), np.uint32)
    seen = np.zeros(e.n, bool)
    capacity = out.trace_out.shape[0]
    for queue in range(5):
        count = int(out.counters[queue])
        label = OUTCOME_NAMES[queue]
        assert 0 <= count <= min(capacity, e.n), "%s: %s counter %d with %d entries in (capacity %d)" % (name, label, count, e.n, capacity)
        if count == 0:
            continue
        rows = out.trace_out[:count] if queue == 4 else out.material_out[queue, :count]
        pixel = rows[:, 10 if queue == 4 else 7] & PIXEL_MASK
        at = np.minimum(np.searchsorted(sorted_pixels, pixel), e.n - 1)
        known = sorted_pixels[at] == pixel
        if not known.all():
            raise AssertionError("%s: %s queue position %d holds pixel %d (word 0x%08x), which no input entry has" % (name, label, _first(~known), pixel[~known][0], rows[_first(~known), 10 if queue == 4 else 7]))
        index = order[at]
        twice = np.nonzero(np.bincount(index, minlength=e.n) > 1)[0]
        if twice.size:
            raise AssertionError("%s: entry %d (pixel %d) is in the %s queue twice" % (name, twice[0], e.pixel[twice[0]], label))
        again = seen[index]
        if again.any():
            i = index[again][0]
            raise AssertionError("%s: entry %d (pixel %d) is in the %s queue and in the %s queue" % (name, i, e.pixel[i], OUTCOME_NAMES[outcome[i]], label))
        seen[index] = True
        outcome[index] = queue
        records[index, :rows.shape[1]] = rows
    return outcome, records


def _first(mask):
    return int(np.nonzero(mask)[0][0])


def check_structure(name, tables, launch, out, result, allowed, sentinel):
    e = launch.entries
    slot, real, bounce, sample, submission, first = launch.paths()
    assert out.counters[5] == e.n, "%s: the input queue's counter changed: %d, %d entries" % (name, out.counters[5], e.n)
    outcome, records = match(launch, out, name)
    # every entry ends in an outcome float64 allows it
    bad = ~allowed[np.arange(e.n), outcome]
    if bad.any():
        i = _first(bad)
        raise AssertionError("%s: entry %d (pixel %d, bounce %d, %s): outcome %s, float64 allows %s" % (
            name, i, e.pixel[i], bounce[i], "robust" if result.robust[i] else "next to a threshold", OUTCOME_NAMES[outcome[i]], [OUTCOME_NAMES[k] for k in np.nonzero(allowed[i])[0]]))
    for queue in range(5):
        sure = int((result.robust & (result.outcome == queue)).sum()); maybe = int((~result.robust & allowed[:, queue]).sum())
        assert sure <= out.counters[queue] <= sure + maybe, "%s: %s counter %d, float64 puts %d there (and %d more within the margins)" % (name, OUTCOME_NAMES[queue], out.counters[queue], sure, maybe)
    # beyond the count: the sentinel
    for queue in range(5):
        rows = out.trace_out if queue == 4 else out.material_out[queue]
        wrong = rows[int(out.counters[queue]):] != np.uint32(sentinel)
        if wrong.any():
            raise AssertionError("%s: %s queue, position %d (count %d), word %d was written" % (name, OUTCOME_NAMES[queue], out.counters[queue] + np.nonzero(wrong)[0][0], out.counters[queue], np.nonzero(wrong)[1][0]))
    # conditional fields
    mip = tables.config["enable_mipmapping"] != 0
    is_material, is_trace = outcome < 4, outcome == SCATTERED
    held = records != np.uint32(sentinel)

    def must_hold_sentinel(rows, words, what):
        wrong = rows[:, None] & held[:, words]
        if wrong.any():
            i = _first(wrong.any(axis=1))
            raise AssertionError("%s: entry %d (pixel %d, bounce %d, %s queue): %s was written (0x%08x)" % (name, i, e.pixel[i], bounce[i], OUTCOME_NAMES[outcome[i]], what, records[i, words][wrong[i]][0]))

    def must_be_written(rows, words, what):
        wrong = rows[:, None] & ~held[:, words]
        if wrong.any():
            i = _first(wrong.any(axis=1))
            raise AssertionError("%s: entry %d (pixel %d, bounce %d, %s queue): %s was not written" % (name, i, e.pixel[i], bounce[i], OUTCOME_NAMES[outcome[i]], what))

    must_hold_sentinel(is_material & ~e.inside, [11], "the medium of an entry outside a medium")
    must_be_written(is_material & e.inside, [11], "the medium of an entry inside a medium")
    must_hold_sentinel(is_material & ~((bounce > 0) & mip), [12, 13], "a cone field at bounce 0 or without mip-mapping")
    must_be_written(is_material & (bounce > 0) & mip, [12, 13], "a cone field")
    must_hold_sentinel(is_material & (bounce == 0), [8, 9, 10], "the throughput at bounce 0")
    must_hold_sentinel(is_material, [14, 15], "padding")
    must_hold_sentinel(is_trace, [6, 7, 8, 9, 14, 18, 19], "the hit, last_pdf or padding of a continuation ray")
    must_hold_sentinel(is_trace & ~mip, [16, 17], "a cone field without mip-mapping")
    must_be_written(is_trace & mip, [16, 17], "a cone field of a continuation ray")
    # exact copies and flags
    d = e.direction.view(np.uint32)
    want = np.stack([d[:, 0], d[:, 1], d[:, 2], e.mesh.view(np.uint32), e.triangle.view(np.uint32), e.t.view(np.uint32), (e.u16 & 0xffff) | (e.v16 << 16),
                     e.pixel | (e.inside.astype(np.uint32) << 30)], axis=1)
    wrong = is_material[:, None] & (records[:, 0:8] != want)
    if wrong.any():
        i = _first(wrong.any(axis=1))
        raise AssertionError("%s: entry %d (pixel %d): material record words %s differ from the input's direction / hit / pixel and flags" % (name, i, e.pixel[i], np.nonzero(wrong[i])[0].tolist()))
    wrong = is_material & e.inside & (records[:, 11] != e.medium.view(np.uint32))
    if wrong.any():
        raise AssertionError("%s: entry %d: medium %d stored for medium %d" % (name, _first(wrong), records[_first(wrong), 11], e.medium[_first(wrong)]))
    wrong = is_material & (bounce > 0) & mip & ((records[:, 12] != e.cone_angle.view(np.uint32)) | (records[:, 13] != e.cone_width.view(np.uint32)))
    if wrong.any():
        raise AssertionError("%s: entry %d: the cone of a material entry is not the input's" % (name, _first(wrong)))
    wrong = is_trace & ((records[:, 10] != (e.pixel | np.uint32(1 << 30))) | (records[:, 15] != e.medium.view(np.uint32)))
    if wrong.any():
        raise AssertionError("%s: entry %d: pixel word / medium of a continuation ray: 0x%08x, %d" % (name, _first(wrong), records[_first(wrong), 10], records[_first(wrong), 15]))
    # the cone of a continuation ray: the input's at bounce > 0; at bounce 0 the angle is the camera's pixel_spread_angle (the width has a measured bound)
    wrong = is_trace & (bounce > 0) & mip & ((records[:, 16] != e.cone_angle.view(np.uint32)) | (records[:, 17] != e.cone_width.view(np.uint32)))
    if wrong.any():
        i = _first(wrong)
        raise AssertionError("%s: entry %d (pixel %d, bounce %d): the cone of a continuation ray is (0x%08x, 0x%08x), the input's is (0x%08x, 0x%08x)" % (
            name, i, e.pixel[i], bounce[i], records[i, 16], records[i, 17], e.cone_angle.view(np.uint32)[i], e.cone_width.view(np.uint32)[i]))
    spread = np.array([tables.pixel_spread_angle], np.float32).view(np.uint32)[0]
    wrong = is_trace & (bounce == 0) & mip & (records[:, 16] != spread)
    if wrong.any():
        raise AssertionError("%s: entry %d (pixel %d): the cone angle of a ray scattered at bounce 0 is 0x%08x, pixel_spread_angle is 0x%08x" % (name, _first(wrong), e.pixel[_first(wrong)], records[_first(wrong), 16], spread))
    # frames: pixels no entry names, and frames an entry leaves alone
    named = np.zeros(launch.aov.shape[1], bool); named[e.pixel] = True
    sure_pixels = np.zeros_like(named); sure_pixels[e.pixel[result.robust]] = True
    for k, label in enumerate(("RADIANCE", "RADIANCE_DIRECT", "RADIANCE_INDIRECT", "ALBEDO")):
        changed = (out.aov[k].view(np.uint32) != launch.aov[k].view(np.uint32)).any(axis=1)
        wrong = changed & ~named
        if wrong.any():
            raise AssertionError("%s: %s frame: pixel %d, which no entry names, changed" % (name, label, _first(wrong)))
        wrong = changed & sure_pixels & ~result.touched[k]
        if wrong.any():
            raise AssertionError("%s: %s frame: pixel %d changed, float64 leaves it alone" % (name, label, _first(wrong)))
    for label, got, before in (("normal and depth", out.gnd, launch.gnd), ("mesh and triangle id", out.gid, launch.gid), ("previous screen position", out.gsp, launch.gsp)):
        changed = (got.view(np.uint32) != before.view(np.uint32)).any(axis=1)
        wrong = changed & ~result.gbuffer_touched
        if wrong.any():
            raise AssertionError("%s: g-buffer %s: pixel %d changed, float64 leaves it alone" % (name, label, _first(wrong)))
    wrong = result.gbuffer_touched & (out.gid != result.gid).any(axis=1)
    if wrong.any():
        raise AssertionError("%s: g-buffer ids of pixel %d: %s, expected %s" % (name, _first(wrong), out.gid[_first(wrong)], result.gid[_first(wrong)]))
    want_query = np.full(2, sentinel, np.uint32).view(np.int32) if result.pixel_query is None else np.array(result.pixel_query, np.int32)
    assert np.array_equal(out.pixel_query, want_query), "%s: the pixel query answers %s, expected %s" % (name, out.pixel_query, want_query)
    # statistics of the merged wavefront
    if out.stats is not None:
        want = np.zeros_like(out.stats)
        np.add.at(want, (submission, STAT_TRACE, bounce), 1)
        mq = outcome < 4
        np.add.at(want, (submission[mq], STAT_DIFFUSE + outcome[mq], bounce[mq]), 1)
        wrong = out.stats != want
        if wrong.any():
            s, kind, b = [int(v[0]) for v in np.nonzero(wrong)]
            raise AssertionError("%s: statistics of submission %d, kind %d, bounce %d: %d, the matched entries give %d" % (name, s, kind, b, out.stats[s, kind, b], want[s, kind, b]))
    return outcome, records


def _same(a, b):
    """Bitwise equal, or both NaN (a NaN's payload is not part of the contract)."""
    au, bu = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    nan_a = ((au & 0x7f800000) == 0x7f800000) & ((au & 0x007fffff) != 0)
    nan_b = ((bu & 0x7f800000) == 0x7f800000) & ((bu & 0x007fffff) != 0)
    return (au == bu) | (nan_a & nan_b)


def check_identical(name, launch, got, got_matched, want, want_matched, entries, other):
    """Every output of the entries of `entries` (bool mask): outcome, record, the four frames' pixels, the g-buffer pixels. (Integer words whose
    bits look like a NaN are the sentinel, on both sides.)"""
    e = launch.entries
    (outcome_a, records_a), (outcome_b, records_b) = got_matched, want_matched
    wrong = entries & (outcome_a != outcome_b)
    if wrong.any():
        i = _first(wrong)
        raise AssertionError("%s: entry %d (pixel %d): outcome %s, %s has %s" % (name, i, e.pixel[i], OUTCOME_NAMES[outcome_a[i]], other, OUTCOME_NAMES[outcome_b[i]]))
    wrong = entries[:, None] & ~_same(records_a, records_b)
    if wrong.any():
        i = _first(wrong.any(axis=1)); w = _first(wrong[i])
        raise AssertionError("%s: entry %d (pixel %d, %s queue): record word %d is 0x%08x (%r), %s has 0x%08x (%r)" % (
            name, i, e.pixel[i], OUTCOME_NAMES[outcome_a[i]], w, records_a[i, w], records_a[i, w:w + 1].view(np.float32)[0], other, records_b[i, w], records_b[i, w:w + 1].view(np.float32)[0]))
    px = e.pixel
    for label, a, b in (("RADIANCE", got.aov[0], want.aov[0]), ("RADIANCE_DIRECT", got.aov[1], want.aov[1]), ("RADIANCE_INDIRECT", got.aov[2], want.aov[2]), ("ALBEDO", got.aov[3], want.aov[3]),
                        ("g-buffer normal and depth", got.gnd, want.gnd), ("g-buffer ids", got.gid, want.gid), ("g-buffer previous screen position", got.gsp, want.gsp)):
        wrong = entries[:, None] & ~_same(a[px], b[px])
        if wrong.any():
            i = _first(wrong.any(axis=1))
            raise AssertionError("%s: entry %d (pixel %d): %s is %s, %s has %s" % (name, i, px[i], label, a[px[i]], other, b[px[i]]))


def check_nan_pattern(name, launch, got, got_matched, want, want_matched, entries, other):
    """The entries that meet a NaN on their way (a black throughput inside a scattering medium: the wavelength pdf is 0 / 0): the same outcome, and NaN in
    the same words of the record (every word read as a float: the sentinel is a NaN on both sides, integers of these records are none) and in the same
    components of the frames' and g-buffers' pixels."""
    e = launch.entries
    (outcome_a, records_a), (outcome_b, records_b) = got_matched, want_matched
    wrong = entries & (outcome_a != outcome_b)
    if wrong.any():
        i = _first(wrong)
        raise AssertionError("%s: entry %d (pixel %d) meets a NaN: outcome %s, %s has %s" % (name, i, e.pixel[i], OUTCOME_NAMES[outcome_a[i]], other, OUTCOME_NAMES[outcome_b[i]]))
    wrong = entries[:, None] & (np.isnan(records_a.view(np.float32)) != np.isnan(records_b.view(np.float32)))
    if wrong.any():
        i = _first(wrong.any(axis=1)); w = _first(wrong[i])
        raise AssertionError("%s: entry %d (pixel %d, %s queue) meets a NaN: record word %d is 0x%08x, %s has 0x%08x" % (name, i, e.pixel[i], OUTCOME_NAMES[outcome_a[i]], w, records_a[i, w], other, records_b[i, w]))
    px = e.pixel
    for label, a, b in (("RADIANCE", got.aov[0], want.aov[0]), ("RADIANCE_DIRECT", got.aov[1], want.aov[1]), ("RADIANCE_INDIRECT", got.aov[2], want.aov[2]), ("ALBEDO", got.aov[3], want.aov[3]),
                        ("g-buffer normal and depth", got.gnd, want.gnd), ("g-buffer previous screen position", got.gsp, want.gsp)):
        wrong = entries[:, None] & (np.isnan(a[px]) != np.isnan(b[px]))
        if wrong.any():
            i = _first(wrong.any(axis=1))
            raise AssertionError("%s: entry %d (pixel %d) meets a NaN: %s is %s, %s has %s" % (name, i, px[i], label, a[px[i]], other, b[px[i]]))


def compare_with_reference(name, tables, launch, out, matched, result, bounds=None):
    """The robust entries against float64. Returns {quantity: (worst error, entry)}; with `bounds`, asserts each within its bound."""
    e = launch.entries
    outcome, records = matched
    slot, real, bounce, sample, submission, first = launch.paths()
    robust = result.robust
    wrong = robust & (outcome != result.outcome)
    if wrong.any():
        i = _first(wrong)
        raise AssertionError("%s: entry %d (pixel %d, bounce %d) is robust: outcome %s, float64 has %s" % (name, i, e.pixel[i], bounce[i], OUTCOME_NAMES[outcome[i]], OUTCOME_NAMES[result.outcome[i]]))
    worst = {}

    def note(quantity, mask, error):
        bad = mask & ~np.isfinite(error)
        if bad.any():
            raise AssertionError("%s: entry %d (pixel %d, bounce %d): %s is not finite where float64 is" % (name, _first(bad), e.pixel[_first(bad)], bounce[_first(bad)], quantity))
        error = np.where(mask, error, 0.0)
        i = int(np.argmax(error)) if error.size else 0
        worst[quantity] = (float(error[i]) if error.size else 0.0, i)
        if bounds is not None and error.size and error[i] > bounds[quantity]:
            raise AssertionError("%s: entry %d (pixel %d, bounce %d, %s): %s differs from float64 by %.3g, bound %.3g" % (name, i, e.pixel[i], bounce[i], OUTCOME_NAMES[outcome[i]], quantity, error[i], bounds[quantity]))

    with np.errstate(all="ignore"):
        def f(words):
            return np.ascontiguousarray(records[:, words]).view(np.float32).astype(np.float64)
        is_material, is_trace = robust & (outcome < 4) & (bounce > 0), robust & (outcome == SCATTERED)
        stored = np.where(is_trace[:, None], f([11, 12, 13]), f([8, 9, 10]))
        scale = np.maximum(np.abs(result.throughput_out).max(axis=1), ref.FLT_MIN)
        note("throughput", is_material | is_trace, np.abs(stored - result.throughput_out).max(axis=1) / scale)
        note("origin", is_trace, np.abs(f([0, 1, 2]) - result.origin_out).max(axis=1) / (np.abs(e.origin).max(axis=1) + result.distance))
        note("direction", is_trace, np.abs(f([3, 4, 5]) - result.direction_out).max(axis=1) / (1.0 + 1.0 / result.sin_theta))
        mip = tables.config["enable_mipmapping"] != 0
        note("cone_width", is_trace & (bounce == 0) & mip, np.abs(f([17])[:, 0] - result.cone_width_out) / result.cone_width_out)
        error = np.zeros(e.n)
        for k in range(4):
            a, b, before = out.aov[k][e.pixel][:, :3].astype(np.float64), result.aov[k][e.pixel][:, :3], launch.aov[k][e.pixel][:, :3].astype(np.float64)
            error = np.maximum(error, (np.abs(a - b) / np.maximum(np.maximum(np.maximum(np.abs(b), np.abs(before)), result.aov_scale[:, None]), ref.FLT_MIN)).max(axis=1))
        aov_defined = robust & np.isfinite(result.aov[:, e.pixel, :3]).all(axis=(0, 2))
        note("aov", aov_defined, error)
        gb = robust & result.gbuffer_touched[e.pixel]
        a = np.concatenate([out.gnd[e.pixel], out.gsp[e.pixel]], axis=1).astype(np.float64); b = np.concatenate([result.gnd[e.pixel], result.gsp[e.pixel]], axis=1)
        note("gbuffer", gb, (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max(axis=1))
    return worst


def measure_margins(out, result):
    """The oracle's float32 intermediates against float64's: {margin name: worst error} over the entries that compute them on both sides."""
    with np.errstate(all="ignore"):
        i = out.internals.astype(np.float64)

        def worst(a, b, scale):
            ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(scale) & (scale > 0) & result.robust   # (robust: both sides took the same branches)
            return float((np.abs(a - b)[ok] / scale[ok]).max()) if ok.any() else 0.0
        one = np.ones(i.shape[0])
        return {"distance": worst(i[:, 0], result.distance, result.distance),
                "wavelength": worst(i[:, 1], result.wavelength_x, result.throughput_sum),
                "survival": worst(i[:, 2], result.survival, result.survival),
                "light_pdf": worst(np.where(result.pdf_in_range, i[:, 3], np.nan), result.light_pdf, result.light_pdf * (1.0 + 1.0 / result.cos_light)),
                "sky_uv": max(worst(i[:, 5], result.sky_u, one), worst(i[:, 6], result.sky_v, one))}


def non_robust_share(result):
    """(non-robust entries, entries that reach a comparison next to which one can be non-robust)."""
    reach = result.reaches_comparison
    return int((reach & ~result.robust).sum()), int(reach.sum())
