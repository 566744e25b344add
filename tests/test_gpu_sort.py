"""The sort launch on the device, entry by entry: rt_sort_rays (the production launchers rt_launch_sort / rt_launch_sort_stream, so the four
instances kernel_sort, kernel_sort_stream, kernel_sort_sky, kernel_sort_stream_sky and the shipped grid) on the launches of sort_cases.py,
against the oracle (oracle_sort) and the float64 reference (sort_reference.py) under the rules of sort_checks.py:

* structure, exact, every launch: counters, one entry per position, the sentinel wherever the kernel must not write, untouched pixels, the
  merged wavefront's statistics rows;
* device against oracle, bit for bit, for every entry outside every medium that is no miss;
* device against float64 within the bounds measured on the oracle (test_sort.py), robust entries taking float64's outcome exactly;
* between instances, bit for bit: a merged launch against per-bounce launches of the same entries; a _sky launch against the plain one for
  the entries the sky's share cannot reach (material-queue entries and medium scatters);
* the refusals of rt_sort_rays, one argument per rule, and that a frame rendered after a series of probe calls equals the one before.
No launch is made on refused input."""
import numpy as np
import pytest

import sort_cases as cases
import sort_checks as checks
import sort_reference as ref

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def world(grt, oracle, tmp_path_factory):
    w = cases.World(grt, oracle, tmp_path_factory.mktemp("sort"), 0)
    yield w
    w.close()


def run(world, setup_name, tables, launch):
    name = "%s/%s" % (setup_name, launch.name)
    e = launch.entries
    result = ref.evaluate(tables, launch, checks.MARGINS)
    allowed = ref.allowed_outcomes(tables, launch, checks.MARGINS, result)
    got = checks.device_launch(world.grt, world.ctx, launch, cases.SENTINEL, capacity=e.n + 37)
    matched = checks.check_structure(name, tables, launch, got, result, allowed, cases.SENTINEL)
    want = checks.oracle_launch(tables, launch, cases.SENTINEL)
    exact = ~e.inside & (e.triangle != ref.INVALID)
    want_matched = checks.match(launch, want, name + " (oracle)")
    checks.check_identical(name, launch, got, matched, want, want_matched, exact, "the oracle")
    checks.check_nan_pattern(name, launch, got, matched, want, want_matched, ~result.finite, "the oracle")
    if launch.name == "medium_edges":
        assert (~result.finite).sum() >= 20, "%s: the launch holds no entry that meets a NaN" % name
    errors = checks.compare_with_reference(name, tables, launch, got, matched, result, checks.BOUNDS)
    print("%-48s %8d entries, %7d bit for bit; " % (name, e.n, exact.sum()) + " ".join("%s %.2g" % (q, v[0]) for q, v in errors.items()))
    return got, matched


@pytest.mark.parametrize("setup", cases.SETUPS, ids=[s.name for s in cases.SETUPS])
def test_device_matches_oracle_and_float64(world, setup):
    tables = world.apply(setup)
    for launch in cases.plan(world, tables, setup):
        run(world, setup.name, tables, launch)


@pytest.mark.parametrize("setup_name,num_bounces", [("bounces_128", cases.MAX_BOUNCES), ("sky_share_0.5", cases.NUM_BOUNCES)], ids=["kernel_sort_stream", "kernel_sort_stream_sky"])
def test_merged_launch_equals_per_bounce_launches(world, setup_name, num_bounces):
    """Each entry of a merged launch against the per-bounce instance given the same bounce, virtual pixel, frames and the sample index the slot
    table implies: the same float operations in another instantiation, so every output bit."""
    world.apply(cases.SETUP[setup_name])
    merged = cases.merged_launch(world, num_bounces)[0]
    got = checks.device_launch(world.grt, world.ctx, merged, cases.SENTINEL)
    outcome, records = checks.match(merged, got, merged.name)
    slot, real, bounce, sample, submission, first = merged.paths()
    for s in np.unique(slot):
        index = np.nonzero(slot == s)[0]
        single = ref.Launch("slot%d_per_bounce" % s, merged.entries.take(index), merged.frame_pixels, merged.frame_slots, bounce=int(bounce[index[0]]),
                            sample_index=int(sample[index[0]]) - int(s), aov=merged.aov)
        single.gnd, single.gid, single.gsp = merged.gnd, merged.gid, merged.gsp
        want = checks.device_launch(world.grt, world.ctx, single, cases.SENTINEL)
        checks.check_identical("%s, slot %d" % (merged.name, s), single, got, (outcome[index], records[index]), want, checks.match(single, want, single.name),
                               np.ones(index.size, bool), "the per-bounce launch")


def test_sky_instance_equals_plain_instance_where_the_share_cannot_reach(world):
    """Material-queue entries and medium scatters do not depend on the sky's share: kernel_sort_sky against kernel_sort and, for the merged launch,
    kernel_sort_stream_sky against kernel_sort_stream, every output bit."""
    outs = {}
    for name in ("default", "sky_share_0.5"):
        world.apply(cases.SETUP[name])
        outs[name] = []
        for launch in cases.mixed_launches(world, bounces=(0, 1, 2, cases.NUM_BOUNCES - 2)) + cases.merged_launch(world, cases.NUM_BOUNCES):
            got = checks.device_launch(world.grt, world.ctx, launch, cases.SENTINEL)
            outs[name].append((launch, got, checks.match(launch, got, "%s/%s" % (name, launch.name))))
    for (launch, plain, plain_matched), (_, sky, sky_matched) in zip(outs["default"], outs["sky_share_0.5"]):
        checks.check_identical("sky_share_0.5/" + launch.name, launch, sky, sky_matched, plain, plain_matched, plain_matched[0] <= ref.SCATTERED, "the plain instance")


def _frame(world):
    assert world.lib.rt_render_sample(world.ctx, 0) == 0, world.lib.rt_last_error(world.ctx)
    return world.pt.read_framebuffer().copy()


def test_refusals_and_that_probe_calls_leave_no_trace(world):
    tables = world.apply(cases.SETUP["default"])
    lib, ctx, fp = world.lib, world.ctx, world.frame_pixels
    before = _frame(world)
    assert np.isfinite(before).all() and before[..., :3].max() > 0

    rng = np.random.default_rng(1)
    n, slots, capacity = 8, 2, 16
    e = cases.make_entries(world, rng, np.arange(n, dtype=np.uint32) * 3 + 1, 1, classes=(ref.DIFFUSE, cases.EMITTER), inside_share=0.0)
    e.inside[0] = True; e.medium[0] = 2
    table, births = cases.single_submission_table(slots, 6)
    pixels = slots * fp
    out = dict(trace_out=np.zeros((capacity, 20), np.uint32), material_out=np.zeros((4, capacity, 16), np.uint32), counters=np.zeros(6, np.int32), aov=np.zeros((4, pixels, 4), np.float32),
               gnd=np.zeros((pixels, 4), np.float32), gid=np.zeros((pixels, 2), np.int32), gsp=np.zeros((pixels, 2), np.float32), query=np.zeros(2, np.int32), stats=np.zeros((128, 6, 128), np.int32))

    def call(records, merged=0, step=1, count=n, capacity=capacity, frame_slots=slots, table=table, slot_count=slots, births=births, **null):
        p = {k: (None if k in null else v.ctypes.data) for k, v in out.items()}
        return lib.rt_sort_rays(ctx, merged, step, 0, None if records is None else records.ctypes.data, count, None if table is None else table.ctypes.data, slot_count,
                                None if births is None else births.ctypes.data, capacity, frame_slots, cases.SENTINEL, p["trace_out"], p["material_out"], p["counters"], p["aov"], p["gnd"],
                                p["gid"], p["gsp"], p["query"], p["stats"])

    good = e.pack()

    def changed(word, entry, value):
        r = good.copy(); r[entry, word] = np.uint32(value & 0xffffffff)
        return r

    late_table = table.copy(); late_table[:, 1] = 9           # born after the iteration: a negative bounce
    late_births = births.copy(); late_births[0] = 9
    far_table = table.copy(); far_table[0, 2] = 128
    odd_table = table.copy(); odd_table[1, 1] = 5             # not its submission's birth
    second_slot = changed(10, 3, fp + 17)                     # an entry of slot 1
    refused = [
        ("NULL trace queue", "NULL array", dict(records=None)),
        ("NULL output queue", "NULL array", dict(records=good, trace_out=None)),
        ("NULL frames", "NULL array", dict(records=good, aov=None)),
        ("NULL slot table", "NULL slot table", dict(records=good, merged=1, step=7, table=None)),
        ("NULL statistics", "NULL slot table", dict(records=good, merged=1, step=7, stats=None)),
        ("more entries than capacity", "capacity", dict(records=good, capacity=n - 1)),
        ("negative bounce", "bounce outside", dict(records=good, step=-1)),
        ("bounce RT_MAX_BOUNCES", "bounce outside", dict(records=good, step=128)),
        ("bounce beyond the path length", "num_bounces", dict(records=good, step=cases.NUM_BOUNCES)),
        ("negative iteration", "negative iteration", dict(records=good, merged=1, step=-1)),
        ("no frame slots", "frame_slots", dict(records=good, frame_slots=0)),
        ("pixel beyond the frames", "beyond the", dict(records=changed(10, 2, pixels))),
        ("pixel beyond the frames, flags set", "beyond the", dict(records=changed(10, 2, pixels | (1 << 31)))),
        ("one pixel twice", "appears twice", dict(records=changed(10, 5, int(good[1, 10] & 0x3fffffff)))),
        ("mesh id beyond the instances", "mesh id", dict(records=changed(6, 4, world.mesh_count))),
        ("negative mesh id", "mesh id", dict(records=changed(6, 4, -1))),
        ("triangle id beyond the triangles", "triangle id", dict(records=changed(7, 4, world.triangle_count))),
        ("negative triangle id that is not RT_INVALID", "triangle id", dict(records=changed(7, 4, -2))),
        ("medium id beyond the media", "medium id", dict(records=changed(15, 0, world.media.shape[0]))),
        ("negative medium id", "medium id", dict(records=changed(15, 0, -1))),
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
        assert status == RT_ERROR_INVALID_ARG and "rt_sort_rays" in message and words in message, (rule, status, message)
        for k, v in out.items():
            assert np.array_equal(v, untouched[k]), "%s: the refused call wrote %s" % (rule, k)
    assert call(records=good) == 0, lib.rt_last_error(ctx)
    assert call(records=second_slot, merged=1, step=7) == 0, lib.rt_last_error(ctx)
    assert out["counters"][5] == n and out["stats"][0, 0, 1] == n
    # what an entry outside a medium holds in its medium word is never looked at
    assert call(records=changed(15, 3, -7)) == 0, lib.rt_last_error(ctx)

    for launch in cases.mixed_launches(world, bounces=(0, 2)) + cases.length_launches(world, lengths=(1025,), merged=True):
        checks.device_launch(world.grt, world.ctx, launch, cases.SENTINEL)
    assert np.array_equal(_frame(world), before), "a frame rendered after the probe calls differs from the one before"
