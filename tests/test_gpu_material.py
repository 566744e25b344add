"""The material launch on the device, entry by entry: rt_shade_rays (the production launchers rt_launch_material / rt_launch_material_stream, so
the shipped grid and the launcher's own choice of instance) on the launches of material_cases.py, under the rules of material_checks.py:

* structure, exact, every launch: counters, one record per position, the sentinel wherever the kernel must not write (last_pdf without
  ALLOW_NEE, the medium outside a medium, the cone words without mip-mapping, every frame and g-buffer pixel no bounce-0 entry names), the
  flag bits, RT_SHADOW_FLAG_BOUNCE_0, the merged wavefront's statistics rows;
* order, exact, for launches of one workgroup: both output queues by direction octant and, within one, in input order;
* device against oracle (oracle_shade): bit for bit where only IEEE operations lie between input and output, the continuation ray within
  the bounds of test_gpu_bsdf.py (imported, not restated);
* queue lengths around a wave and a workgroup, and one entry in a second grid-stride round;
* between instances, bit for bit: a merged launch against per-bounce launches of the same entries; a sort launch's material queues fed in
  unchanged (rt_sort_rays -> rt_shade_rays against oracle_sort -> oracle_shade);
* what the sort leaves unwritten at bounce 0 is not read;
* the _nmap instances of the diffuse and plastic slots: unmapped hits equal the plain instance, a mapped hit's g-buffer normal is its shading normal;
* the refusals of rt_shade_rays, one per rule, and that a frame rendered after a series of probe calls equals the one before.
No launch is made on refused input. Every test prints, per launch, the instance launched, the entries, those compared bit for bit and those
left out, and its own time."""
import time

import numpy as np
import pytest

import material_cases as cases
import material_checks as checks
import material_reference as ref
import sort_cases
import sort_checks
from test_gpu_bsdf import SAMPLE_BOUNDS

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def world(grt, oracle, tmp_path_factory):
    w = cases.World(grt, oracle, tmp_path_factory.mktemp("material"), 0)
    yield w
    w.close()


@pytest.fixture(autouse=True)
def timed(request):
    start = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - start))


def instance(world, tables, launch):
    """The __global__ entry point rt_launch_material / rt_launch_material_stream picks for the launch (kernels_material.hip)."""
    name = "kernel_material_" + cases.SLOT_NAMES[launch.slot] + ("_stream" if launch.merged else "")
    if launch.slot < 2 and not world.textures_compressed:
        name += "_texels"
    return name + ("_sky" if tables.sky_share > 0 else "")


def run(world, setup_name, tables, launch, capacity=None):
    name = "%s/%s" % (setup_name, launch.name)
    got = checks.device_launch(world.grt, world.ctx, launch, capacity=capacity or launch.entries.n + 37)
    got_at = checks.check_structure(name, tables, launch, got)
    if launch.entries.n <= cases.BLOCK:
        checks.check_order(name, launch, got, *got_at)
    want = checks.oracle_launch(tables, launch)
    want_at = checks.match(launch, want, name + " (oracle)")
    reference = ref.reference_of(world, tables, launch)
    counts = checks.check_against_oracle(name, world, tables, launch, got, got_at, want, want_at, reference, SAMPLE_BOUNDS)
    checks.compare_with_reference(name, tables, launch, got, got_at, reference, checks.BOUNDS)
    if not launch.name.startswith(cases.THRESHOLD_LAUNCHES):
        assert counts["left_out"] <= checks.NON_ROBUST_CAP * launch.entries.n, "%s: %d of %d entries left out" % (name, counts["left_out"], launch.entries.n)
    print("%-44s %-40s %6d entries, %6d continue (%6d bit for bit), %6d shadow rays (%6d bit for bit), %3d left out; " % (
        name, instance(world, tables, launch), launch.entries.n, got.counters[0], counts["bit_for_bit"], got.counters[1], counts["shadow_bit_for_bit"], counts["left_out"])
        + " ".join("%s %.2g" % kv for kv in counts["worst"].items()))
    return got, got_at


@pytest.mark.parametrize("setup", cases.PLAIN_SETUPS, ids=[s.name for s in cases.PLAIN_SETUPS])
def test_device_obeys_the_rules_and_matches_the_oracle(world, setup):
    tables = world.apply(setup)
    for launch in cases.plan(world, setup, tables):
        run(world, setup.name, tables, launch)


@pytest.mark.parametrize("case", [c for c in __import__("nee_cases").GPU_CASES if c.name in ("limit", "meshes65", "tris2049")], ids=lambda c: c.name)
def test_light_tables_within_and_beyond_the_lds_limits(grt, oracle, tmp_path, case):
    """The light tables in the workgroup's LDS copy (64 mesh entries and 2048 triangle entries: the limit) and in global memory (one entry
    more of either kind): the shadow records bit for bit against the oracle, which searches one table either way."""
    w = cases.LightsWorld(grt, oracle, case, tmp_path, 0)
    try:
        for launch in cases.light_table_launches(w):
            got, got_at = run(w, case.name, w.tables, launch)
            assert got.counters[1] > 100
    finally:
        w.close()


def test_a_second_grid_stride_round(world):
    """2048 x 256 + 1 diffuse entries at bounce 1, per-bounce form: structure on all of them, values on a strided sample of 4096 and on the
    entry that is alone in the second round. (The merged form's 8192 x 256 + 1 entries need 513 sample slots of this frame: the slot table
    has 512.)"""
    tables = world.apply(cases.SETUP["default"])
    launch = cases.second_round_launch(world)
    name = "default/" + launch.name
    got = checks.device_launch(world.grt, world.ctx, launch)
    got_at = checks.check_structure(name, tables, launch, got)
    n = launch.entries.n
    sample = np.unique(np.concatenate([np.arange(0, n, n // (cases.MAX_VALUE_ENTRIES - 2)), [n - 2, n - 1]]))
    sub = cases.Launch(launch.name + "_sample", launch.slot, launch.entries.take(sample), launch.frame_pixels, launch.frame_slots, bounce=launch.bounce, sample_index=launch.sample_index)
    want = checks.oracle_launch(tables, sub)
    want_at = checks.match(sub, want, name + " (oracle)")
    picked = checks.Outputs()
    picked.trace_out, picked.shadow_out, picked.counters = got.trace_out, got.shadow_out, got.counters
    picked.aov, picked.gnd, picked.gid, picked.gsp = got.aov, got.gnd, got.gid, got.gsp
    counts = checks.check_against_oracle(name, world, tables, sub, picked, (got_at[0][sample], got_at[1][sample]), want, want_at, ref.reference_of(world, tables, sub), SAMPLE_BOUNDS)
    checks.compare_with_reference(name, tables, sub, picked, (got_at[0][sample], got_at[1][sample]), ref.reference_of(world, tables, sub), checks.BOUNDS)
    assert counts["left_out"] <= checks.NON_ROBUST_CAP * sample.size, "%s: %d of %d sampled entries left out" % (name, counts["left_out"], sample.size)
    print("%-44s %-40s %6d entries, %6d sampled, %6d bit for bit, %3d left out" % (name, instance(world, tables, launch), n, sample.size, counts["bit_for_bit"], counts["left_out"]))


def test_merged_launch_equals_per_bounce_launches(world):
    """Each entry of a merged launch against the per-bounce instance given the same bounce, virtual pixel and the sample index the slot table
    implies: the same float operations in another instantiation, so every output bit -- but RT_SHADOW_FLAG_BOUNCE_0, which only the merged form sets."""
    tables = world.apply(cases.SETUP["svgf_on"])
    for slot in range(4):
        merged = cases.merged(world, "instances", slot, 2500, seed=1800 + slot)
        name = merged.name
        got = checks.device_launch(world.grt, world.ctx, merged)
        got_at = checks.check_structure(name, tables, merged, got)
        sample_slot, real, bounce, sample, submission = merged.paths()
        for s in np.unique(sample_slot):
            index = np.nonzero(sample_slot == s)[0]
            single = cases.Launch("%s_slot%d_per_bounce" % (name, s), slot, merged.entries.take(index), merged.frame_pixels, merged.frame_slots,
                                  bounce=int(bounce[index[0]]), sample_index=int(sample[index[0]]) - int(s))
            want = checks.device_launch(world.grt, world.ctx, single)
            want_at = checks.check_structure(single.name, tables, single, want)
            for queue, rows_got, rows_want in ((0, got.trace_out, want.trace_out), (1, got.shadow_out, want.shadow_out)):
                a_at, b_at = got_at[queue][index], want_at[queue]
                assert np.array_equal(a_at >= 0, b_at >= 0), "%s: queue %d: an entry is in one launch's queue only" % (single.name, queue)
                live = a_at >= 0
                a, b = rows_got[a_at[live]].copy(), rows_want[b_at[live]]
                if queue == 1:
                    a[:, 10] &= ~checks.SHADOW_FLAG_BOUNCE_0
                assert np.array_equal(a, b), "%s: queue %d: entry %d differs between the merged and the per-bounce launch" % (single.name, queue, index[live][np.nonzero((a != b).any(axis=1))[0][0]])
            px = merged.entries.pixel[index]
            for label, a, b in (("aov", got.aov.transpose(1, 0, 2), want.aov.transpose(1, 0, 2)), ("gnd", got.gnd, want.gnd), ("gid", got.gid, want.gid), ("gsp", got.gsp, want.gsp)):
                assert np.array_equal(a[px], b[px]), "%s: %s differs between the merged and the per-bounce launch" % (single.name, label)
        print("%-44s %-40s %6d entries, all bit for bit against the per-bounce instance" % (name, instance(world, tables, merged), merged.entries.n))


def test_normal_mapped_instances(world):
    """The _nmap instances of the diffuse and the plastic slot (a normal map on the two textured materials makes the launchers take them),
    per bounce and merged, under SVGF: a hit whose material has no map equals the plain instance in every output bit; a mapped hit at
    bounce 0 leaves ONE normal behind -- the g-buffer's octahedral normal encodes the NORMAL frame's, which is no longer the interpolated
    normal the plain instance wrote there."""
    from sort_reference import _oct_encode
    tables = world.apply(cases.SETUP["svgf_on"])
    world.upload_textures(False)   # a map must be an RT_TEXTURE_RGBA8 texture: the scene's one again, as plain texels (the same texels either way)
    launches = [cases.per_bounce(world, "nmap", slot, 700, b, seed=2200 + 10 * slot + b) for slot in (0, 1) for b in (0, 2)] + [cases.merged(world, "nmap", slot, 1500, seed=2250 + slot) for slot in (0, 1)]
    plain = [checks.device_launch(world.grt, world.ctx, launch) for launch in launches]
    textured_material = (tables.materials[:, 3].view(np.int32) >= 0) & np.isin(tables.material_types, (cases.DIFFUSE, cases.PLASTIC))
    maps = np.where(textured_material, tables.materials[:, 3].view(np.int32), -1).astype(np.int32)   # each textured material's own texture as its map
    assert (maps >= 0).sum() == 2
    assert world.grt.upload_material_normal_maps(world.ctx, maps) == 0, world.lib.rt_last_error(world.ctx)
    try:
        for launch, before in zip(launches, plain):
            name = "svgf_on/" + launch.name
            got = checks.device_launch(world.grt, world.ctx, launch)
            got_at = checks.check_structure(name, tables, launch, got)
            before_at = checks.match(launch, before, name + " (plain)")
            e = launch.entries
            bounce = launch.paths()[2]
            mapped = world.textured_instance[e.mesh]
            assert mapped.sum() > 100 and (~mapped).sum() > 100, name
            for queue, rows_a, rows_b in ((0, got.trace_out, before.trace_out), (1, got.shadow_out, before.shadow_out)):
                a_at, b_at = got_at[queue][~mapped], before_at[queue][~mapped]
                assert np.array_equal(a_at >= 0, b_at >= 0), "%s: an unmapped hit is in one instance's queue only" % name
                live = a_at >= 0
                assert np.array_equal(rows_a[a_at[live]], rows_b[b_at[live]]), "%s: queue %d: an unmapped hit differs from the plain instance" % (name, queue)
            px = e.pixel[~mapped]
            for label, a, b in (("aov", got.aov.transpose(1, 0, 2), before.aov.transpose(1, 0, 2)), ("gnd", got.gnd, before.gnd), ("gid", got.gid, before.gid), ("gsp", got.gsp, before.gsp)):
                assert np.array_equal(a[px], b[px]), "%s: %s of an unmapped hit differs from the plain instance" % (name, label)
            first = np.nonzero(mapped & (bounce == 0) & (got.aov[checks.NORMAL][e.pixel] != np.uint32(cases.SENTINEL)).all(axis=1))[0]
            if (bounce == 0).any():
                px = e.pixel[first]
                shading = got.aov[checks.NORMAL][px, :3].view(np.float32).astype(np.float64)
                interpolated = before.aov[checks.NORMAL][px, :3].view(np.float32).astype(np.float64)
                moved = np.abs(shading - interpolated).max(axis=1) > 1e-3
                assert moved.sum() > 0.5 * first.size > 20, "%s: the map moves %d of %d normals" % (name, moved.sum(), first.size)
                encoded = got.gnd[px, :2].view(np.float32).astype(np.float64)
                ox, oy = _oct_encode(shading)
                error = np.maximum(np.abs(encoded[:, 0] - ox), np.abs(encoded[:, 1] - oy))
                # (the encoding is a handful of float32 operations on numbers below 1: 1e-6 is several ulp of them, the map moves the normals by 1e-3 and more)
                assert (error <= 1e-6).all(), "%s: entry %d: the g-buffer's normal is not the NORMAL frame's (%.3g apart in the octahedral square)" % (name, first[int(error.argmax())], error.max())
                ox, oy = _oct_encode(interpolated[moved])
                assert (np.maximum(np.abs(encoded[moved, 0] - ox), np.abs(encoded[moved, 1] - oy)) > 1e-5).all(), "%s: a g-buffer normal still encodes the interpolated normal" % name
            print("%-44s kernel_material_%s%s_texels_nmap %6d entries, %6d unmapped all bit for bit with the plain instance, %6d mapped at bounce 0" % (
                name, cases.SLOT_NAMES[launch.slot], "_stream" if launch.merged else "", e.n, (~mapped).sum(), first.size))
    finally:
        assert world.grt.upload_material_normal_maps(world.ctx, np.full(maps.size, -1, np.int32)) == 0


def test_sort_output_feeds_the_material_launch(world):
    """One chain: the material_out of an rt_sort_rays call fed unchanged to rt_shade_rays, against the oracle's sort followed by its shade."""
    tables = world.apply(cases.SETUP["default"])
    rng = np.random.default_rng(1700)
    for bounce in (0, 2):
        e = sort_cases.make_entries(world, rng, sort_cases.pixels_for(rng, 3000, world.frame_pixels, 1), bounce)
        launch = sort_cases.per_bounce(world, "chain_bounce%d" % bounce, e, bounce, slots=1)
        device_sorted = sort_checks.device_launch(world.grt, world.ctx, launch, cases.SENTINEL)
        oracle_sorted = sort_checks.oracle_launch(tables, launch, cases.SENTINEL)
        for slot in range(4):
            n = int(device_sorted.counters[slot])
            assert n > 50 and n == oracle_sorted.counters[slot]
            fed = cases.from_records(world, "chain", slot, device_sorted.material_out[slot, :n], bounce, launch.sample_index)
            r = world.grt.shade_rays(world.ctx, slot, device_sorted.material_out[slot, :n], world.frame_pixels, 1, bounce=bounce, sample_index=launch.sample_index, capacity=n + 5, sentinel=cases.SENTINEL)
            got = checks.Outputs()
            got.trace_out, got.shadow_out, got.counters, got.aov, got.gnd, got.gid, got.gsp, got.stats = r.trace_out, r.shadow_out, r.counters, r.aov, r.gbuffer_normal_and_depth, r.gbuffer_ids, r.gbuffer_screen_prev, r.stats
            name = "chain/" + fed.name
            got_at = checks.check_structure(name, tables, fed, got)
            fed_oracle = cases.from_records(world, "chain", slot, oracle_sorted.material_out[slot, :n], bounce, launch.sample_index)
            want = checks.oracle_launch(tables, fed_oracle)
            want_at = checks.match(fed_oracle, want, name + " (oracle)")
            # the two sorts queue the same entries in their own orders: the oracle's results, entry by entry, in the device's order
            order = np.argsort(fed_oracle.entries.pixel)[np.searchsorted(np.sort(fed_oracle.entries.pixel), fed.entries.pixel)]
            assert np.array_equal(fed_oracle.entries.pixel[order], fed.entries.pixel)
            # ... on the entries both sorts hand over bit for bit (all but those whose throughput went through a medium's expf: test_gpu_sort.py)
            same = (fed.pack() == fed_oracle.pack()[order]).all(axis=1)
            assert same.all() if bounce == 0 else same.sum() > 0.5 * n, "%s: %d of %d records differ between the two sorts" % (name, (~same).sum(), n)
            keep = np.nonzero(same)[0]
            sub = cases.from_records(world, "chain", slot, fed.pack()[keep], bounce, launch.sample_index)
            reference = ref.reference_of(world, tables, sub)
            want.internals = want.internals[order][keep]
            if not same.all():   # the frames are compared whole: a bounce above 0 writes none
                assert bounce > 0
            counts = checks.check_against_oracle(name, world, tables, sub, got, (got_at[0][keep], got_at[1][keep]), want, (want_at[0][order][keep], want_at[1][order][keep]), reference, SAMPLE_BOUNDS)
            checks.compare_with_reference(name, tables, sub, got, (got_at[0][keep], got_at[1][keep]), reference, checks.BOUNDS)
            assert counts["left_out"] <= checks.NON_ROBUST_CAP * keep.size, "%s: %d of %d entries left out" % (name, counts["left_out"], keep.size)
            print("%-44s %-40s %6d entries, %6d handed over bit for bit by both sorts, %6d of those bit for bit, %3d left out" % (
                name, instance(world, tables, fed), n, keep.size, counts["bit_for_bit"], counts["left_out"]))


def test_unwritten_words_of_bounce_0_are_not_read(world):
    """At bounce 0 the sort stores neither throughput nor cone words: a launch whose input carries the sentinel (a NaN) there equals, bit for
    bit, the same launch with finite garbage there. Per-bounce and merged."""
    tables = world.apply(cases.SETUP["default"])
    for launch in [cases.per_bounce(world, "unwritten", slot, 600, 0, seed=1600 + slot) for slot in range(4)] + [cases.merged(world, "unwritten", slot, 1500, seed=1610 + slot) for slot in (0, 1, 2, 3)]:
        assert (launch.paths()[2] == 0).sum() > 100
        a, b = checks.device_launch(world.grt, world.ctx, launch), checks.device_launch(world.grt, world.ctx, launch, garbage=0.37)
        for field in ("counters", "aov", "gnd", "gid", "gsp"):
            assert np.array_equal(getattr(a, field), getattr(b, field)), "%s: %s depends on words the sort leaves unwritten" % (launch.name, field)
        for field in ("trace_out", "shadow_out"):   # (workgroups append in the order their atomics land: the queues are compared entry by entry)
            rows_a, rows_b = getattr(a, field), getattr(b, field)
            assert np.array_equal(rows_a[np.argsort(rows_a[:, 10], kind="stable")], rows_b[np.argsort(rows_b[:, 10], kind="stable")]), "%s: %s depends on words the sort leaves unwritten" % (launch.name, field)
        print("%-44s %-40s %6d entries, all bit for bit with garbage in the unwritten words" % (launch.name, instance(world, tables, launch), launch.entries.n))


def _frame(world):
    assert world.lib.rt_render_sample(world.ctx, 0) == 0, world.lib.rt_last_error(world.ctx)
    return world.pt.read_framebuffer().copy()


def test_refusals_and_that_probe_calls_leave_no_trace(world):
    tables = world.apply(cases.SETUP["default"])
    lib, ctx, fp = world.lib, world.ctx, world.frame_pixels
    before = _frame(world)
    assert np.isfinite(before).all() and before[..., :3].max() > 0

    n, slots, capacity = 8, 2, 16
    good_launch = cases.per_bounce(world, "refusals", 0, n, 1, seed=1900, slots=1)
    good_launch.entries.inside[0] = True; good_launch.entries.medium[0] = 2
    good = good_launch.pack()
    table, births = cases.single_submission_table(slots, 6)
    pixels = slots * fp
    out = dict(trace_out=np.zeros((capacity, 20), np.uint32), shadow_out=np.zeros((capacity, 11), np.uint32), counters=np.zeros(3, np.int32), aov=np.zeros((3, pixels, 4), np.uint32),
               gnd=np.zeros((pixels, 4), np.uint32), gid=np.zeros((pixels, 2), np.uint32), gsp=np.zeros((pixels, 2), np.uint32), stats=np.zeros((128, 6, 128), np.int32))

    def call(records, merged=0, step=1, slot=0, count=n, capacity=capacity, frame_slots=slots, table=table, slot_count=slots, births=births, **null):
        p = {k: (None if k in null else v.ctypes.data) for k, v in out.items()}
        return lib.rt_shade_rays(ctx, merged, step, 0, slot, None if records is None else records.ctypes.data, count, None if table is None else table.ctypes.data, slot_count,
                                 None if births is None else births.ctypes.data, capacity, frame_slots, cases.SENTINEL, p["trace_out"], p["shadow_out"], p["counters"], p["aov"], p["gnd"],
                                 p["gid"], p["gsp"], p["stats"])

    def changed(word, entry, value):
        r = good.copy(); r[entry, word] = np.uint32(value & 0xffffffff)
        return r

    late_table = table.copy(); late_table[:, 1] = 9           # born after the iteration: a negative bounce
    late_births = births.copy(); late_births[0] = 9
    far_table = table.copy(); far_table[0, 2] = 128
    odd_table = table.copy(); odd_table[1, 1] = 5             # not its submission's birth
    second_slot = changed(7, 3, fp + 17)                      # an entry of slot 1
    plastic_instance = int(world.instances[cases.PLASTIC][0])
    refused = [
        ("NULL material queue", "NULL array", dict(records=None)),
        ("NULL output queue", "NULL array", dict(records=good, trace_out=None)),
        ("NULL shadow queue", "NULL array", dict(records=good, shadow_out=None)),
        ("NULL frames", "NULL array", dict(records=good, aov=None)),
        ("NULL slot table", "NULL slot table", dict(records=good, merged=1, step=7, table=None)),
        ("NULL statistics", "NULL slot table", dict(records=good, merged=1, step=7, stats=None)),
        ("material slot 4", "material_slot", dict(records=good, slot=4)),
        ("negative material slot", "material_slot", dict(records=good, slot=-1)),
        ("more entries than capacity", "capacity", dict(records=good, capacity=n - 1)),
        ("negative bounce", "bounce outside", dict(records=good, step=-1)),
        ("bounce RT_MAX_BOUNCES - 1", "bounce outside", dict(records=good, step=127)),
        ("bounce beyond the path length", "num_bounces", dict(records=good, step=cases.NUM_BOUNCES)),
        ("negative iteration", "negative iteration", dict(records=good, merged=1, step=-1)),
        ("no frame slots", "frame_slots", dict(records=good, frame_slots=0)),
        ("pixel beyond the frames", "beyond the", dict(records=changed(7, 2, pixels))),
        ("pixel beyond the frames, medium flag set", "beyond the", dict(records=changed(7, 2, pixels | (1 << 30)))),
        ("one pixel twice", "appears twice", dict(records=changed(7, 5, int(good[1, 7] & 0x3fffffff)))),
        ("mesh id beyond the instances", "mesh id", dict(records=changed(3, 4, world.mesh_count))),
        ("negative mesh id", "mesh id", dict(records=changed(3, 4, -1))),
        ("triangle id beyond the triangles", "triangle id", dict(records=changed(4, 4, world.triangle_count))),
        ("RT_INVALID as triangle id", "triangle id", dict(records=changed(4, 4, -1))),
        ("an instance of another material", "does not belong to queue", dict(records=changed(3, 4, plastic_instance))),
        ("the right instances in the wrong queue", "does not belong to queue", dict(records=good, slot=1)),
        ("medium id beyond the media", "medium id", dict(records=changed(11, 0, world.media.shape[0]))),
        ("negative medium id", "medium id", dict(records=changed(11, 0, -1))),
        ("slot beyond the table", "beyond the", dict(records=second_slot, merged=1, step=7, slot_count=1)),
        ("submission beyond the ring", "submission", dict(records=good, merged=1, step=7, table=far_table)),
        ("bounce of an entry negative", "bounce", dict(records=good, merged=1, step=7, table=late_table, births=late_births)),
        ("bounce of an entry beyond RT_MAX_BOUNCES", "bounce", dict(records=good, merged=1, step=6 + 128)),
        ("slot born apart from its submission", "birth", dict(records=good, merged=1, step=7, table=odd_table)),
    ]
    untouched = {k: v.copy() for k, v in out.items()}
    for rule, words, arguments in refused:
        status = call(**arguments)
        message = lib.rt_last_error(ctx).decode()
        assert status == RT_ERROR_INVALID_ARG and "rt_shade_rays" in message and words in message, (rule, status, message)
        for k, v in out.items():
            assert np.array_equal(v, untouched[k]), "%s: the refused call wrote %s" % (rule, k)
    assert call(records=good) == 0, lib.rt_last_error(ctx)
    assert out["counters"][2] == n
    assert call(records=second_slot, merged=1, step=7) == 0, lib.rt_last_error(ctx)
    assert out["counters"][2] == n
    # what an entry outside a medium holds in its medium word is never looked at
    assert call(records=changed(11, 3, -7)) == 0, lib.rt_last_error(ctx)

    for launch in cases.small_launches(world):
        checks.device_launch(world.grt, world.ctx, launch)
    assert np.array_equal(_frame(world), before), "a frame rendered after the probe calls differs from the one before"
