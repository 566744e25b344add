"""Comparisons shared by test_material.py (the oracle's shade_material under the structure rules, CPU) and test_gpu_material.py (the device's
material launch, rt_shade_rays, against the rules and against the oracle).

Entries are matched by their virtual pixel, which is unique within a launch.

Structure (exact, every launch; check_structure):
* the input queue's counter is unchanged; positions [0, count) of the next trace queue and of the shadow queue hold one entry each, every
  one an input entry, none twice (so an entry continues at most once and emits at most one shadow ray); every word at or beyond `count`
  holds the sentinel;
* a continuation record: origin, direction, pixel word and throughput written; the hit words and the padding hold the sentinel; ALLOW_NEE
  set exactly where last_pdf was written; INSIDE_MEDIUM set exactly where the medium word was written, which then names a medium of the
  table; the cone words written exactly with mip-mapping;
* a shadow record is written whole; its pixel word carries RT_SHADOW_FLAG_BOUNCE_0 exactly in the merged form at bounce 0;
* without next-event estimation (off, or neither lights nor a sky share) there is no shadow ray;
* frames and g-buffers: a pixel holds the sentinel unless a bounce-0 entry names it; a frame the context has disabled, and the g-buffers
  without SVGF, hold it everywhere; a pixel is written whole (four, two, two words) and in NORMAL, POSITION and the g-buffers together;
* merged form: the statistics rows equal the shadow rays counted per (submission, bounce) from the matched records, every other cell is 0.

Order (exact, launches of at most RT_SHADE_BLOCK entries; check_order): one workgroup makes one round, so both output queues hold their
entries by direction octant (x < 0: 4, y < 0: 2, z < 0: 1) and, within an octant, in input order (block_bucketed_append2).

Against the oracle (check_against_oracle), NaN equal to NaN:
* bit for bit, over the WHOLE arrays (both sides start from the sentinel): the NORMAL and POSITION frames and the three g-buffers; the
  ALBEDO frame at the pixels of untextured hits;
* per entry, bit for bit: whether it emits a shadow ray, and the shadow record's origin, direction, max_distance and pixel word; its
  illumination where the hit's material has no texture (selection, the epsilon offsets, the light pdf, eval and the MIS weight are IEEE
  operations only); cone_angle and cone_width of a continuation record (the curvature term included);
* per entry, the same outcome (continues or not), flags and medium; direction, last_pdf and throughput within the bounds test_gpu_bsdf.py
  holds rt_bsdf_sample to (passed in by the caller, not restated here); the origin within the direction's bound times the size of the
  epsilon offset's operands (the offset follows the direction's sign against the geometric normal, and adds to the hit point);
* textured hits: the fetch is not IEEE-only -- the anisotropic filter of bounce 0 forms its level of detail with log2f inside the texture unit
  (rt_shading.h: texture_get_grad), the launch forms it with log2f beyond bounce 0 -- so the albedo is held to the bound
  test_gpu_texture_unit.py measured for such a fetch (its GRAD_TOL, imported); the throughput to the BSDF's bounds like every other hit's,
  with nothing added; the illumination, which the issue's bit-for-bit rule cannot cover here, to TEXTURED_RELATIVE (derived below).
  The tests print how many textured records are bit-identical all the same.
An entry may take another outcome than the oracle's only where a deciding comparison is next to its threshold. The two of the set-up are
reported by the oracle as float32 numbers (dot(direction, geometric normal) < 0, omega_i.z <= 0: both dot products of unit vectors, IEEE
only, so bit-identical on the device -- these can never differ); the BSDF's own branches compare a random number with a Fresnel term or
a table value that carries the sin / cos difference, and are replayed by bsdf_reference.py (`near`, within NEAR_RELATIVE). Such entries
are left out of the value comparisons and counted, at most sort_checks.NON_ROBUST_CAP of a launch's entries (no floor: a launch too small for one such entry has none).
"""
import numpy as np

from material_cases import ALBEDO_FLOOR, BLOCK, SENTINEL, SHADOW_WORDS, TRACE_WORDS
from sort_checks import NON_ROBUST_CAP   # noqa: F401 (the cap the tests assert)

PIXEL_MASK = np.uint32(0x3fffffff)
FLAG_ALLOW_NEE, FLAG_INSIDE_MEDIUM, SHADOW_FLAG_BOUNCE_0 = np.uint32(1 << 31), np.uint32(1 << 30), np.uint32(1 << 30)
STAT_SHADOW = 1
ALBEDO, NORMAL, POSITION = range(3)
from test_gpu_texture_unit import GRAD_TOL as TEXTURE_TOL   # device against oracle, measured there: a filtered fetch whose level of detail went through log2f
# What that does to a throughput or an illumination, per channel and relative: the diffuse BSDF is linear in the albedo a, the plastic's
# diffuse lobe goes as a / (1 - a k) with k = 1 - (1 - F_avg) / 1.5^2 < 0.6, whose logarithmic derivative 1 / (1 - a k) is below 2.5 (the
# specular lobe it is added to is positive and has no albedo), and every texel of the world's textures is at least ALBEDO_FLOOR.
TEXTURED_RELATIVE = 2.5 * TEXTURE_TOL / ALBEDO_FLOOR


class Outputs:
    """What a launch left behind, from the device (rt_shade_rays) or the oracle (oracle_shade per sample slot, joined): trace_out (C, 20),
    shadow_out (C, 11), counters int32[3] {next trace, shadow, input}, aov (3, P, 4), gnd (P, 4), gid (P, 2), gsp (P, 2) uint32 words,
    stats (128, 6, 128) or None."""


def enabled_frames(tables):
    mask = tables.config["aov_mask"] | ((1 << 3) if tables.config["enable_svgf"] else 0)   # rt_set_config: SVGF turns ALBEDO on
    return tuple(bool((mask >> a) & 1) for a in (3, 4, 5))


def device_launch(grt, ctx, launch, capacity=None, garbage=None):
    r = grt.shade_rays(ctx, launch.slot, launch.pack(garbage), launch.frame_pixels, launch.frame_slots, bounce=launch.bounce, sample_index=launch.sample_index,
                       iteration=launch.iteration, slot_table=launch.slot_table, submission_birth=launch.submission_birth, capacity=capacity, sentinel=SENTINEL)
    o = Outputs()
    o.trace_out, o.shadow_out, o.counters, o.aov, o.gnd, o.gid, o.gsp, o.stats = r.trace_out, r.shadow_out, r.counters, r.aov, r.gbuffer_normal_and_depth, r.gbuffer_ids, r.gbuffer_screen_prev, r.stats
    return o


def oracle_launch(tables, launch, garbage=None):
    """The launch through oracle_shade: one call per sample slot (the oracle knows pixels and samples, not virtual pixels), queues joined in
    slot order (a launch of one slot keeps input order). internals (N, 2): dot(direction, geometric normal), omega_i.z."""
    e = launch.entries
    slot, real, bounce, sample, submission = launch.paths()
    records = launch.pack(garbage)
    capacity, pixels, fp = max(e.n, 1), launch.frame_pixels * launch.frame_slots, launch.frame_pixels
    o = Outputs()
    o.trace_out = np.full((capacity, TRACE_WORDS), SENTINEL, np.uint32); o.shadow_out = np.full((capacity, SHADOW_WORDS), SENTINEL, np.uint32)
    o.counters = np.array([0, 0, e.n], np.int32)
    o.aov = np.full((3, pixels, 4), SENTINEL, np.uint32)
    o.gnd, o.gid, o.gsp = np.full((pixels, 4), SENTINEL, np.uint32), np.full((pixels, 2), SENTINEL, np.uint32), np.full((pixels, 2), SENTINEL, np.uint32)
    o.internals = np.full((e.n, 2), np.nan, np.float32)
    o.stats = None
    for s in np.unique(slot):
        index = np.nonzero(slot == s)[0]
        base = int(s) * fp
        part = records[index].copy(); part[:, 7] = (part[:, 7] & ~PIXEL_MASK) | real[index]
        b = int(bounce[index[0]])
        trace, shadow, counts, internals = tables.view.shade(launch.slot, part, b, int(sample[index[0]]), [o.aov[k, base:base + fp] for k in range(3)],
                                                             o.gnd[base:base + fp], o.gid[base:base + fp], o.gsp[base:base + fp], sentinel=SENTINEL, aov_enabled=enabled_frames(tables))
        o.internals[index] = internals
        n = counts[0]
        rows = trace[:n].copy(); rows[:, 10] += np.uint32(base)
        o.trace_out[o.counters[0]:o.counters[0] + n] = rows; o.counters[0] += n
        n = counts[1]
        rows = shadow[:n].copy(); rows[:, 10] += np.uint32(base)
        if launch.merged and b == 0:
            rows[:, 10] |= SHADOW_FLAG_BOUNCE_0
        o.shadow_out[o.counters[1]:o.counters[1] + n] = rows; o.counters[1] += n
    return o


def _first(mask):
    return int(np.nonzero(mask)[0][0])


def match(launch, out, name):
    """Per input entry: its position in the next trace queue and in the shadow queue (-1: none)."""
    e = launch.entries
    order = np.argsort(e.pixel, kind="stable")
    sorted_pixels = e.pixel[order]
    capacity = out.trace_out.shape[0]
    positions = []
    for queue, label, rows_all, word in ((0, "next trace", out.trace_out, 10), (1, "shadow", out.shadow_out, 10)):
        count = int(out.counters[queue])
        assert 0 <= count <= min(capacity, e.n), "%s: %s counter %d with %d entries in (capacity %d)" % (name, label, count, e.n, capacity)
        position = np.full(e.n, -1, np.int64)
        if count:
            rows = rows_all[:count]
            pixel = rows[:, word] & PIXEL_MASK
            at = np.minimum(np.searchsorted(sorted_pixels, pixel), e.n - 1)
            known = sorted_pixels[at] == pixel
            if not known.all():
                raise AssertionError("%s: %s queue position %d holds pixel %d (word 0x%08x), which no input entry has" % (name, label, _first(~known), pixel[~known][0], rows[_first(~known), word]))
            index = order[at]
            twice = np.nonzero(np.bincount(index, minlength=e.n) > 1)[0]
            if twice.size:
                raise AssertionError("%s: entry %d (pixel %d) is in the %s queue twice" % (name, twice[0], e.pixel[twice[0]], label))
            position[index] = np.arange(count)
        positions.append(position)
    return positions[0], positions[1]


def check_structure(name, tables, launch, out):
    e, cfg = launch.entries, tables.config
    slot, real, bounce, sample, submission = launch.paths()
    sentinel = np.uint32(SENTINEL)
    assert out.counters[2] == e.n, "%s: the input queue's counter changed: %d, %d entries" % (name, out.counters[2], e.n)
    trace_at, shadow_at = match(launch, out, name)
    for label, rows, count in (("next trace", out.trace_out, out.counters[0]), ("shadow", out.shadow_out, out.counters[1])):
        wrong = rows[int(count):] != sentinel
        if wrong.any():
            raise AssertionError("%s: %s queue, position %d (count %d), word %d was written" % (name, label, count + np.nonzero(wrong)[0][0], count, np.nonzero(wrong)[1][0]))

    # continuation records
    index = np.nonzero(trace_at >= 0)[0]
    rec = out.trace_out[trace_at[index]]
    held = rec != sentinel

    def fail(mask, what):
        if mask.any():
            i = index[_first(mask)]
            raise AssertionError("%s: entry %d (pixel %d, bounce %d): %s (record %s)" % (name, i, e.pixel[i], bounce[i], what, ["%08x" % w for w in out.trace_out[trace_at[i]]]))

    fail(~held[:, [0, 1, 2, 3, 4, 5, 10, 11, 12, 13]].all(axis=1), "origin, direction, pixel word or throughput was not written")
    fail(held[:, [6, 7, 8, 9]].any(axis=1), "a hit word of a continuation ray was written")
    fail(held[:, [18, 19]].any(axis=1), "padding was written")
    allow = (rec[:, 10] & FLAG_ALLOW_NEE) != 0
    inside = (rec[:, 10] & FLAG_INSIDE_MEDIUM) != 0
    fail(held[:, 14] & ~allow, "last_pdf was written though the BSDF does not allow NEE")
    fail(~held[:, 14] & allow, "last_pdf was not written though ALLOW_NEE is set")
    fail(held[:, 15] & ~inside, "the medium was written outside a medium")
    fail(~held[:, 15] & inside, "the medium was not written inside a medium")
    fail(inside & (rec[:, 15].view(np.int32) < 0) | inside & (rec[:, 15].view(np.int32) >= tables.media.shape[0]), "the medium id is beyond the media table")
    mip = cfg["enable_mipmapping"] != 0
    fail(held[:, [16, 17]].any(axis=1) if not mip else ~held[:, [16, 17]].all(axis=1), "the cone words were written without mip-mapping" if not mip else "a cone word was not written")

    # shadow records
    s_index = np.nonzero(shadow_at >= 0)[0]
    s_rec = out.shadow_out[shadow_at[s_index]]
    whole = (s_rec != sentinel).all(axis=1)
    if not whole.all():
        i = s_index[_first(~whole)]
        raise AssertionError("%s: entry %d (pixel %d): a word of its shadow record was not written" % (name, i, e.pixel[i]))
    flagged = (s_rec[:, 10] & SHADOW_FLAG_BOUNCE_0) != 0
    expected = (bounce[s_index] == 0) if launch.merged else np.zeros(s_index.size, bool)
    if (flagged != expected).any():
        i = s_index[_first(flagged != expected)]
        raise AssertionError("%s: entry %d (pixel %d, bounce %d, %s form): RT_SHADOW_FLAG_BOUNCE_0 is %s" % (
            name, i, e.pixel[i], bounce[i], "merged" if launch.merged else "per-bounce", "set" if flagged[_first(flagged != expected)] else "clear"))
    nee = cfg["enable_next_event_estimation"] != 0 and (tables.lights_total_weight > 0.0 or tables.sky_share > 0.0)   # (a sky share: light samples without emitters)
    if not nee:
        assert out.counters[1] == 0, "%s: %d shadow rays without next-event estimation" % (name, out.counters[1])

    # frames and g-buffers
    named = np.zeros(launch.frame_pixels * launch.frame_slots, bool)
    named[e.pixel[bounce == 0]] = True
    frames = enabled_frames(tables)
    svgf = cfg["enable_svgf"] != 0
    written = {}
    for label, array, on in (("ALBEDO", out.aov[ALBEDO], frames[0]), ("NORMAL", out.aov[NORMAL], frames[1]), ("POSITION", out.aov[POSITION], frames[2]),
                             ("g-buffer normal and depth", out.gnd, svgf), ("g-buffer ids", out.gid, svgf), ("g-buffer previous position", out.gsp, svgf)):
        touched = array != sentinel
        stray = touched.any(axis=1) & ~(named & on)
        if stray.any():
            raise AssertionError("%s: %s pixel %d was written (%s)" % (name, label, _first(stray), "the frame is off" if not on else "no bounce-0 entry names it"))
        partial = touched.any(axis=1) & ~touched.all(axis=1)
        if partial.any() and label != "g-buffer ids":   # (an id may equal the sentinel's low bits never; a float word may: not in these scenes)
            raise AssertionError("%s: %s pixel %d was written in part" % (name, label, _first(partial)))
        written[label] = touched.any(axis=1)
    for a, b in (("NORMAL", "POSITION"), ("g-buffer normal and depth", "g-buffer ids"), ("g-buffer normal and depth", "g-buffer previous position")):
        if (frames[1] and frames[2]) if a == "NORMAL" else svgf:
            assert np.array_equal(written[a], written[b]), "%s: %s and %s were written at different pixels (first %d)" % (name, a, b, _first(written[a] != written[b]))
    if svgf and frames[1]:
        assert np.array_equal(written["NORMAL"], written["g-buffer ids"]), "%s: the NORMAL frame and the g-buffers were written at different pixels" % name
    # every entry that goes on, or connects to a light, at bounce 0 has left its surface in the frames
    if frames[1]:
        lost = ((trace_at >= 0) | (shadow_at >= 0)) & (bounce == 0) & ~written["NORMAL"][e.pixel]
        assert not lost.any(), "%s: entry %d (pixel %d) continues at bounce 0 but its NORMAL pixel holds the sentinel" % (name, _first(lost) if lost.any() else -1, e.pixel[_first(lost)] if lost.any() else -1)

    # the merged form's statistics
    if launch.merged and out.stats is not None:   # (the oracle keeps none)
        want = np.zeros_like(out.stats)
        np.add.at(want, (submission[s_index], STAT_SHADOW, bounce[s_index]), 1)
        if not np.array_equal(out.stats, want):
            sub, kind, b = [int(x[0]) for x in np.nonzero(out.stats != want)]
            raise AssertionError("%s: statistics of submission %d, kind %d, bounce %d: %d, the queues hold %d" % (name, sub, kind, b, out.stats[sub, kind, b], want[sub, kind, b]))
    return trace_at, shadow_at


def octant(direction_words):
    d = direction_words.view(np.float32)
    return (d[:, 0] < 0) * 4 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 1


def check_order(name, launch, out, trace_at, shadow_at):
    """One workgroup, one round: both queues by direction octant and, within an octant, in input order."""
    assert launch.entries.n <= BLOCK
    for label, rows, at in (("next trace", out.trace_out, trace_at), ("shadow", out.shadow_out, shadow_at)):
        index = np.nonzero(at >= 0)[0]                       # input order
        bucket = octant(rows[at[index], 3:6])
        want = index[np.argsort(bucket, kind="stable")]      # by octant, input order within
        got = index[np.argsort(at[index])]                   # by position in the queue
        if not np.array_equal(got, want):
            k = _first(got != want)
            raise AssertionError("%s: %s queue position %d holds input entry %d, octant order puts entry %d there" % (name, label, k, got[k], want[k]))


def _same(a, b):
    """Bit for bit, NaN equal to NaN (whatever its payload)."""
    fa, fb = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


def check_against_oracle(name, world, tables, launch, got, got_at, want, want_at, reference, sample_bounds):
    """got / want: Outputs of the device and the oracle with their matches; reference: material_reference.evaluate's Result (its `near`:
    entries with a deciding comparison next to its threshold); sample_bounds: test_gpu_bsdf.SAMPLE_BOUNDS. Returns the counts printed by
    the tests: entries compared bit for bit, entries left out (of this comparison or of the one with float64)."""
    e = launch.entries
    # (the set-up's own two comparisons are IEEE dot products, bit-identical on both sides: they excuse nothing here)
    near = reference.near_sample | reference.near_light
    slot, real, bounce, sample, submission = launch.paths()
    textured = world.textured_instance[e.mesh]

    # frames, whole arrays
    for label, a, b in (("NORMAL", got.aov[NORMAL], want.aov[NORMAL]), ("POSITION", got.aov[POSITION], want.aov[POSITION]), ("g-buffer normal and depth", got.gnd, want.gnd),
                        ("g-buffer ids", got.gid, want.gid), ("g-buffer previous position", got.gsp, want.gsp)):
        bad = ~_same(a, b).all(axis=1)
        if bad.any():
            p = _first(bad); i = np.nonzero(e.pixel == p)[0]
            raise AssertionError("%s: %s pixel %d (entry %s): device %s, oracle %s" % (name, label, p, i.tolist(), a[p].view(np.float32).tolist(), b[p].view(np.float32).tolist()))
    plain_pixels = np.ones(got.aov.shape[1], bool); plain_pixels[e.pixel[textured]] = False
    bad = ~_same(got.aov[ALBEDO], want.aov[ALBEDO]).all(axis=1) & plain_pixels
    assert not bad.any(), "%s: ALBEDO pixel %d (untextured): device %s, oracle %s" % (name, _first(bad) if bad.any() else -1, got.aov[ALBEDO][bad][:1].view(np.float32).tolist(), want.aov[ALBEDO][bad][:1].view(np.float32).tolist())
    tex_pixels = e.pixel[textured & (bounce == 0)]
    a, b = got.aov[ALBEDO][tex_pixels], want.aov[ALBEDO][tex_pixels]
    assert np.array_equal(a == np.uint32(SENTINEL), b == np.uint32(SENTINEL)), "%s: textured ALBEDO pixels written on one side only" % name
    live = (a != np.uint32(SENTINEL)).all(axis=1)
    worst_albedo = float(np.abs(a[live].view(np.float32)[:, :3].astype(np.float64) - b[live].view(np.float32)[:, :3]).max()) if live.any() else 0.0
    assert worst_albedo <= TEXTURE_TOL, "%s: a textured ALBEDO pixel is %.3g from the oracle's (bound %.3g)" % (name, worst_albedo, TEXTURE_TOL)

    # shadow rays
    differ = (got_at[1] >= 0) != (want_at[1] >= 0)
    assert not (differ & ~near).any(), "%s: entry %d (pixel %d, bounce %d) emits a shadow ray on one side only (device %s)" % (
        name, _first(differ & ~near) if (differ & ~near).any() else -1, e.pixel[_first(differ & ~near)] if (differ & ~near).any() else -1,
        bounce[_first(differ & ~near)] if (differ & ~near).any() else -1, (got_at[1] >= 0)[_first(differ & ~near)] if (differ & ~near).any() else None)
    both = np.nonzero((got_at[1] >= 0) & (want_at[1] >= 0))[0]
    a, b = got.shadow_out[got_at[1][both]], want.shadow_out[want_at[1][both]]
    same = _same(a, b)
    geometry = same[:, [0, 1, 2, 3, 4, 5, 6, 10]].all(axis=1)
    if not geometry.all():
        k = _first(~geometry); i = both[k]
        raise AssertionError("%s: entry %d (pixel %d, bounce %d): shadow ray origin, direction, max_distance or pixel word differ: device %s, oracle %s" % (
            name, i, e.pixel[i], bounce[i], a[k].view(np.float32).tolist(), b[k].view(np.float32).tolist()))
    light = same[:, 7:10].all(axis=1) | textured[both]
    if not light.all():
        k = _first(~light); i = both[k]
        raise AssertionError("%s: entry %d (pixel %d, bounce %d): illumination differs: device %s, oracle %s" % (name, i, e.pixel[i], bounce[i], a[k, 7:10].view(np.float32).tolist(), b[k, 7:10].view(np.float32).tolist()))
    t = textured[both]
    if t.any():
        ia, ib = a[t, 7:10].view(np.float32).astype(np.float64), b[t, 7:10].view(np.float32).astype(np.float64)
        err = np.abs(ia - ib) / np.maximum(np.abs(ib), 1e-30)
        assert (err <= TEXTURED_RELATIVE).all(), "%s: a textured hit's illumination is %.3g (relative, per channel) from the oracle's (bound %.3g)" % (name, err.max(), TEXTURED_RELATIVE)

    # continuation rays
    differ = (got_at[0] >= 0) != (want_at[0] >= 0)
    if (differ & ~near).any():
        i = _first(differ & ~near)
        raise AssertionError("%s: entry %d (pixel %d, bounce %d, set-up %s): %s on the device, %s in the oracle, away from every threshold" % (
            name, i, e.pixel[i], bounce[i], want.internals[i].tolist(), "continues" if got_at[0][i] >= 0 else "ends", "continues" if want_at[0][i] >= 0 else "ends"))
    left_out = near | differ
    both = np.nonzero((got_at[0] >= 0) & (want_at[0] >= 0) & ~left_out)[0]
    a, b = got.trace_out[got_at[0][both]], want.trace_out[want_at[0][both]]
    same = _same(a, b)
    for words, what in (([10], "the pixel word and flags"), ([15], "the medium"), ([16], "cone_angle"), ([17], "cone_width")):
        bad = ~same[:, words].all(axis=1)
        if bad.any():
            k = _first(bad); i = both[k]
            raise AssertionError("%s: entry %d (pixel %d, bounce %d): %s differs: device 0x%08x (%r), oracle 0x%08x (%r)" % (
                name, i, e.pixel[i], bounce[i], what, a[k, words[0]], float(a[k, words[0]:words[0] + 1].view(np.float32)[0]), b[k, words[0]], float(b[k, words[0]:words[0] + 1].view(np.float32)[0])))
    roughness = world.roughness_of_instance(tables)[e.mesh[both]]
    dir_tol = np.where(roughness < 0.3, sample_bounds["smooth"][0], sample_bounds["rough"][0])
    rel_tol = np.where(roughness < 0.3, sample_bounds["smooth"][1], sample_bounds["rough"][1])
    fa, fb = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
    errors = {}
    errors["direction"] = np.abs(fa[:, 3:6] - fb[:, 3:6]).max(axis=1)
    with np.errstate(invalid="ignore"):
        has_pdf = (b[:, 10] & FLAG_ALLOW_NEE) != 0
        errors["pdf"] = np.where(has_pdf, np.abs(fa[:, 14] - fb[:, 14]) / np.maximum(np.abs(fb[:, 14]), 1e-30), 0.0)
        # the throughput: the BSDF's factor relative per channel (as rt_bsdf_sample's is held), times the incoming throughput and the albedo
        errors["throughput"] = (np.abs(fa[:, 11:14] - fb[:, 11:14]) / np.maximum(np.abs(fb[:, 11:14]), 1e-30)).max(axis=1)
    # the origin is the hit point (bit-identical) plus EPSILON x the geometric normal on the side the direction leaves on: bit-identical too,
    # unless the direction lies in the surface's plane to within its own bound, where the side may differ (then 2 EPSILON at most)
    flat = reference.near_origin[both]
    moved = ~same[:, [0, 1, 2]].all(axis=1)
    if (moved & ~flat).any():
        k = _first(moved & ~flat); i = both[k]
        raise AssertionError("%s: entry %d (pixel %d, bounce %d): the origin differs from the oracle's: device %s, oracle %s" % (name, i, e.pixel[i], bounce[i], fa[k, 0:3].tolist(), fb[k, 0:3].tolist()))
    errors["origin"] = np.where(flat, np.abs(fa[:, 0:3] - fb[:, 0:3]).max(axis=1), 0.0)
    worst = {}
    for q, tol in (("direction", dir_tol), ("pdf", rel_tol), ("throughput", rel_tol), ("origin", 2.0001e-4)):
        err = np.nan_to_num(errors[q], nan=0.0)
        nan_differs = np.isnan(errors[q]) & ~same[:, {"direction": [3, 4, 5], "pdf": [14], "throughput": [11, 12, 13], "origin": [0, 1, 2]}[q]].all(axis=1)
        over = (err > tol) | nan_differs
        if over.any():
            k = int(np.argmax(np.where(over, err + 1.0, 0.0))); i = both[k]
            raise AssertionError("%s: entry %d (pixel %d, bounce %d, roughness %.3g): %s is %.3g from the oracle's (bound %.3g): device %s, oracle %s" % (
                name, i, e.pixel[i], bounce[i], roughness[k], q, err[k], np.broadcast_to(tol, err.shape)[k], fa[k].tolist(), fb[k].tolist()))
        worst[q] = float(err.max()) if err.size else 0.0
    worst["albedo"] = worst_albedo
    bitwise = int(same[:, [10, 15, 16, 17]].all(axis=1).sum())
    return dict(entries=e.n, bit_for_bit=bitwise, shadow_bit_for_bit=int(geometry.sum()), left_out=int((left_out | reference.near).sum()), worst=worst)



# ---- against the float64 reference (material_reference.py) ----------------------------------------------------------------------------
# Measured on the oracle over every launch of test_material.py (which prints the table and asserts it); the bound is 4 x the worst case,
# and the device is held to the same number. Errors: `normal`, `direction`, `shadow_direction` absolute (unit vectors); `position`,
# `origin`, `shadow_origin`, `gbuffer` relative to max(1, |value|); `cone_width`, `pdf`, `shadow_distance` relative; `cone_angle` relative
# to |angle| + |curvature term| (1 + 1 / |normal . direction|) (the term divides by that dot product); `throughput`, `illumination`
# relative per channel, floored at 1e-3 of the largest channel (bsdf_checks.py's rule). Textured hits are left out of the last two.
#   quantity          worst oracle error   launch
MEASURED = {
    "normal":           (1.46e-07, "default/length_diffuse_merged_257"),
    "position":         (7.84e-07, "limit/lights_diffuse_merged_1500"),
    "gbuffer":          (3.09e-06, "svgf_on/small_plastic_bounce0_700"),
    "cone_width":       (9.17e-08, "default/mixed_plastic_merged_4000"),
    "cone_angle":       (1.82e-07, "default/mixed_diffuse_bounce1_3000"),
    "direction":        (9.25e-05, "default/mixed_conductor_merged_4000"),
    "pdf":              (0.000971, "default/mixed_conductor_merged_4000"),
    "throughput":       (0.000493, "default/mixed_dielectric_bounce1_3000"),
    "origin":           (9.7e-07, "limit/lights_diffuse_merged_1500"),
    "shadow_origin":    (9.7e-07, "limit/lights_diffuse_merged_1500"),
    "shadow_direction": (6.92e-07, "default/mixed_diffuse_bounce0_3000"),
    "shadow_distance":  (4.22e-07, "mis_off/small_diffuse_bounce0_700"),
    "illumination":     (0.00453, "default/mixed_conductor_merged_4000"),
    # the throughput on the launches of material_cases.VariantWorld (test_material.py: test_variant_world_bound_is_four_times_the_worst_case)
    "variant_throughput": (0.00242, "svgf_on/nmap_flat_conductor_bounce0_1500"),
    # the NORMAL frame of a mapped hit: material_reference.mapped_normal32, the float32 restatement of normal_map_perturb, against float64
    # (test_material.py: test_mapped_normal_bound_is_four_times_the_float32_restatement); absolute, per component
    "mapped_normal":    (2.02e-06, "svgf_on/nmap_inward_conductor_bounce0_1500"),
    # the throughput on the unmapped conductor launches of test_gpu_material_instances.py (test_material.py: test_instance_throughput_bound_is_four_times_the_worst_case)
    "instance_throughput": (0.0007, "instances_plain/instances_conductor_bounce2_1250"),
}
BOUNDS = {q: 4.0 * v[0] for q, v in MEASURED.items()}


def _relative(a, b, floor=1.0):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def _point(a, b):
    """A point's error, relative to its largest coordinate (or 1): float32 resolves the small coordinates of a far point no better."""
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


def _per_channel(a, b):
    floor = 1e-3 * np.abs(b).max(axis=1, keepdims=True) + 1e-30
    return (np.abs(a - b) / np.maximum(np.abs(b), floor)).max(axis=1)


def compare_with_reference(name, tables, launch, out, at, r, bounds):
    """out / at: a launch's Outputs and match; r: material_reference.evaluate's Result. Robust entries take float64's outcome exactly
    (alive, continues, emits a shadow ray, ALLOW_NEE, medium); their values are compared. Returns {quantity: (worst error, entry)};
    asserts against `bounds` where it is given (None: measure only)."""
    e, cfg = launch.entries, tables.config
    slot, real, bounce, sample, submission = launch.paths()
    trace_at, shadow_at = at
    robust = r.robust
    sentinel = np.uint32(SENTINEL)
    frames = enabled_frames(tables)

    def outcome(mask, what):
        if mask.any():
            i = _first(mask)
            raise AssertionError("%s: entry %d (pixel %d, bounce %d), away from every threshold: %s" % (name, i, e.pixel[i], bounce[i], what))

    outcome(robust & (trace_at >= 0) & ~r.continues, "it continues, float64 says it ends")
    outcome(robust & (trace_at < 0) & r.continues, "it ends, float64 says it continues")
    outcome(robust & (shadow_at >= 0) & ~r.has_shadow, "it emits a shadow ray, float64 says it emits none")
    outcome(robust & (shadow_at < 0) & r.has_shadow, "it emits no shadow ray, float64 says it emits one")
    first = bounce == 0
    if frames[1]:
        wrote = (out.aov[NORMAL][e.pixel] != sentinel).any(axis=1)
        outcome(robust & first & (wrote != r.alive), "the NORMAL frame was written though float64 drops the entry in the set-up, or the other way round")

    errors = {}

    def measure(quantity, error, index):
        error = np.asarray(error, np.float64)
        if error.size == 0:
            return
        bad = ~np.isfinite(error)
        if bad.any():
            i = index[_first(bad)]
            raise AssertionError("%s: entry %d (pixel %d, bounce %d): %s is not comparable (NaN or infinite on one side)" % (name, i, e.pixel[i], bounce[i], quantity))
        k = int(error.argmax())
        if error[k] > errors.get(quantity, (-1.0, -1))[0]:
            errors[quantity] = (float(error[k]), int(index[k]))

    # frames and g-buffers at bounce 0
    index = np.nonzero(robust & first & r.alive)[0]
    if frames[1]:
        measure("normal", np.abs(out.aov[NORMAL][e.pixel[index], :3].view(np.float32) - r.normal[index]).max(axis=1), index)
    if frames[2]:
        measure("position", _point(out.aov[POSITION][e.pixel[index], :3].view(np.float32), r.position[index]), index)
    if cfg["enable_svgf"]:
        px = e.pixel[index]
        assert np.array_equal(out.gid[px].view(np.int32), r.gid[index]), "%s: a g-buffer's mesh and triangle ids are not the entry's" % name
        measure("gbuffer", np.maximum(_relative(out.gnd[px].view(np.float32), r.gnd[index]).max(axis=1), _relative(out.gsp[px].view(np.float32), r.gsp[index]).max(axis=1)), index)

    # continuation rays
    index = np.nonzero(robust & (trace_at >= 0) & r.continues)[0]
    rec = out.trace_out[trace_at[index]]
    f = rec.view(np.float32).astype(np.float64)
    allow = (rec[:, 10] & FLAG_ALLOW_NEE) != 0
    inside = (rec[:, 10] & FLAG_INSIDE_MEDIUM) != 0
    bad = allow != r.allow_nee[index]
    outcome(np.isin(np.arange(e.n), index[bad]), "ALLOW_NEE is not what the BSDF's roughness says")
    medium = np.where(inside, rec[:, 15].view(np.int32), -1)
    bad = medium != r.medium[index]
    outcome(np.isin(np.arange(e.n), index[bad]), "the medium of the continuation ray is not float64's")
    if cfg["enable_mipmapping"]:
        measure("cone_width", _relative(f[:, 17], r.cone_width[index], 1e-30), index)
        measure("cone_angle", np.abs(f[:, 16] - r.cone_angle[index]) / r.cone_angle_scale[index], index)
    measure("direction", np.abs(f[:, 3:6] - r.direction[index]).max(axis=1), index)
    measure("pdf", _relative(f[allow, 14], r.pdf[index][allow], 1e-30), index[allow])
    plain = ~r.textured[index]
    measure("throughput", _per_channel(f[plain, 11:14], r.throughput[index][plain]), index[plain])
    level = ~r.near_origin[index]
    measure("origin", _point(f[level, 0:3], r.origin[index][level]), index[level])

    # shadow rays
    index = np.nonzero(robust & (shadow_at >= 0) & r.has_shadow)[0]
    f = out.shadow_out[shadow_at[index]].view(np.float32).astype(np.float64)
    measure("shadow_origin", _point(f[:, 0:3], r.shadow_origin[index]), index)
    measure("shadow_direction", np.abs(f[:, 3:6] - r.shadow_direction[index]).max(axis=1), index)
    # (a sky entry's ray runs to infinity: RT_INFINITY exactly, and a finite length for every emitter entry)
    to_sky = np.isposinf(r.shadow_distance[index])
    outcome(np.isin(np.arange(e.n), index[np.isposinf(f[:, 6]) != to_sky]), "max_distance is +inf for a shadow ray to an emitter, or finite for one to the sky")
    measure("shadow_distance", _relative(f[~to_sky, 6], r.shadow_distance[index][~to_sky], 1e-30), index[~to_sky])
    plain = ~r.textured[index]
    measure("illumination", _per_channel(f[plain, 7:10], r.illumination[index][plain]), index[plain])

    if bounds is not None:
        for quantity, (error, i) in errors.items():
            assert error <= bounds[quantity], "%s: entry %d (pixel %d, bounce %d): %s is %.3g from float64's, the bound is %.3g" % (name, i, e.pixel[i], bounce[i], quantity, error, bounds[quantity])
    return errors
