"""Every instance of the material launch on the device, entry by entry: the 96 entry points the kernels_material_*.hip units compile from shade_material (rt_material.h) -- 6 rows
(diffuse, plastic, dielectric, conductor, and the _texels forms of the first two) x 8 variants (the light split: plain, _sky, _split, _tree; with and
without _nmap) x 2 forms (per-bounce, _stream) -- each picked by material_kernels_for ([(NMAP * 4 + SKY) * rows + row]) from the context's settings,
run by rt_shade_rays on the launches of material_cases.py (VariantWorld) and held to the float64 composition of material_reference.py with the runner
of test_gpu_material_variants.py: check_structure, check_order up to one workgroup, compare_with_reference on every quantity under
material_checks.BOUNDS (the throughput of the mapped rows under VARIANT_BOUNDS and of the unmapped conductor rows under CONDUCTOR_BOUNDS, both measured
on the oracle in test_material.py; a guarded mapped normal under BOUNDS["mapped_normal"]; a sky direction within INVERSION_BOUND), robust entries taking float64's outcomes exactly, at most NON_ROBUST_CAP of a launch left out, and more than 100 robust shadow
entries on every route in force (sky, delta light, emitter by power or by tree). The conditions on the inputs are shown on the CPU, from the reference
alone, in test_material.py.

Which test reaches which instances (each name per-bounce and _stream; rows: diffuse and plastic with and without _texels, dielectric, conductor):
* all 6 rows x {plain, _sky, _split, _tree} x {-, _nmap}: test_every_instance[<variant>-<row>] -- one per-bounce launch (bounce 0 and 2 alternate across the
  rows) and one merged launch each; _sky: a sky share of 0.25; _split: the delta lights of material_cases.DELTA_LIGHTS at share 0.5 beside it, so that
  all three routes are in force; _tree: the light tree on with the same two shares; _nmap: the tilt map on the slot's type, on regular and mirrored
  triangles; the rows without _texels under the bc1 setup with the textured diffuse and plastic materials' albedo in the BC1 texture itself, so that
  the blocks are decoded inside the material kernel: on the plain instances those hits are held to the oracle (which reads the decoded chain) in
  albedo, throughput and illumination as RGBA8-textured hits are, on every other variant their ALBEDO pixel and continuation entry equal the plain
  compressed instance's bit for bit;
* the same instances with MIS off: test_one_row_per_light_variant_without_mis; _tree with both shares 0 (taken == 0): test_tree_row_with_nothing_taken;
* kernel_material_{dielectric,conductor}{_split,_tree} on smooth materials (no shadow entry, no ALLOW_NEE, every output bit the plain instance's):
  test_smooth_rows_equal_the_plain_instance;
* the queue lengths 1, 64 and 257 (structure and order) of every light variant: test_queue_lengths_of_every_light_variant;
* the merged form's second grid-stride round, 8192 x 256 + 1 entries in a 128 x 64 frame, kernel_material_diffuse_stream_texels and
  kernel_material_conductor_stream_tree: test_second_round_of_the_merged_form;
* a fog volume around the launch (bounce 0's throughput read from the queue; the tree displaced): test_launch_under_a_fog_volume;
* the count: test_every_instance_was_launched.
Every launch prints its instance, the entries held per route, those left out and the worst error per quantity; every test prints its wall time."""
import time

import numpy as np
import pytest

import material_cases as cases
import material_checks as checks
import material_reference as ref
import test_gpu_material_variants as variants
from test_gpu_bsdf import SAMPLE_BOUNDS
from test_gpu_material_variants import VARIANT_BOUNDS, _matched_rows, instance

pytestmark = pytest.mark.gpu

# The throughput of the unmapped conductor rows: the oracle's error on these very queues under the plain setup (test_material.py), 4 x that
CONDUCTOR_BOUNDS = dict(checks.BOUNDS, throughput=checks.BOUNDS["instance_throughput"])
RAN = {}      # instance -> the launches this module held it on
CASES_DONE = set()
EVERY_CASE = cases.INSTANCE_CASES


@pytest.fixture(scope="module")
def world(grt, oracle, tmp_path_factory):
    w = cases.VariantWorld(grt, oracle, tmp_path_factory.mktemp("instances"), 0)
    yield w
    w.apply(cases.SETUP["default"])
    w.close()


@pytest.fixture(autouse=True)
def timed(request):
    start = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - start))


def run(world, setup_name, tables, launch, **how):
    out = variants.run(world, setup_name, tables, launch, **how)
    RAN.setdefault(instance(world, tables, launch), []).append("%s/%s" % (setup_name, launch.name))
    return out


def _row(world, setup, light, mapped, slot, compressed, sides=True, **launches):
    """The two launches of one row under `setup`; asserts the instance each one takes."""
    tables = world.apply(setup)
    assert world.textures_compressed == compressed
    out = []
    try:
        for maps, launch in cases.instance_launches(world, light, mapped, slot, compressed, **launches):
            world.set_maps(tables, maps)
            want = cases.instance_name(slot, launch.merged, slot < 2 and not compressed, tuple(cases.LIGHT_VARIANTS).index(light), mapped)
            assert instance(world, tables, launch) == want, (instance(world, tables, launch), want)
            got, got_at, r = run(world, setup.name, tables, launch, sides=sides, bounds=VARIANT_BOUNDS if mapped else CONDUCTOR_BOUNDS if slot == 3 else checks.BOUNDS)
            assert not mapped or ((r.mapped & r.robust).sum() > 100 and (~r.mapped & r.robust).sum() > 100), launch.name
            out.append((launch, got, got_at, r))
    finally:
        world.set_maps(tables, {})
    return tables, out


@pytest.mark.parametrize("case", EVERY_CASE, ids=cases.instance_case_id)
def test_every_instance(world, case):
    light, mapped, slot, compressed = case
    setup = cases.instance_setup(light, compressed)
    tables, out = _row(world, setup, light, mapped, slot, compressed)
    if compressed:
        _bc1_albedo_checks(world, setup, tables, out, plain=light == "" and not mapped)
    CASES_DONE.add(case)


def _bc1_albedo_checks(world, setup, tables, out, plain):
    """The hits whose albedo is the BC1 texture, decoded per fetch inside the kernel. The plain instance: the whole launch against the oracle as
    test_gpu_material.py holds a launch (the oracle fetches from the decoded chain) -- a textured hit's albedo within TEXTURE_TOL, its throughput within
    the BSDF's bounds, its illumination within TEXTURED_RELATIVE. Every other variant: the variant touches neither the albedo nor the continuation ray, and
    nothing is fused under -ffp-contract=off, so a textured hit's ALBEDO pixel and continuation entry (throughput included) are the plain compressed
    instance's on the same entries, bit for bit."""
    bc1 = tables.materials[:, 3].view(np.int32) == world.bc1_index
    assert bc1.sum() == 2 and world.textures_compressed
    plain_tables = tables if plain else world.apply(cases.instance_setup("", True))
    world.set_maps(plain_tables, {})
    for launch, got, got_at, r in out:
        name = "%s/%s" % (setup.name, launch.name)
        e, bounce = launch.entries, launch.paths()[2]
        textured = r.textured & bc1[tables.material_ids[e.mesh]]
        assert textured.sum() > 100 and np.array_equal(textured, r.textured), name
        if plain:
            want = checks.oracle_launch(plain_tables, launch)
            counts = checks.check_against_oracle(name, world, plain_tables, launch, got, got_at, want, checks.match(launch, want, name + " (oracle)"), r, SAMPLE_BOUNDS)
            print("%-50s %4d hits on the BC1 albedo against the oracle: " % (name, textured.sum()) + " ".join("%s %.2g" % kv for kv in counts["worst"].items()))
            continue
        before = checks.device_launch(world.grt, world.ctx, launch, capacity=e.n + 37)
        assert instance(world, plain_tables, launch) == cases.instance_name(launch.slot, launch.merged, False, 0, False)
        a, b = _matched_rows(launch, got, name)[0][textured], _matched_rows(launch, before, name + " (plain)")[0][textured]
        differ = (a != b).any(axis=1)
        assert not differ.any(), "%s: entry %d: the continuation entry of a hit on the BC1 albedo differs from the plain compressed instance's" % (name, np.nonzero(textured)[0][np.nonzero(differ)[0][0]])
        px = e.pixel[textured & (bounce == 0)]
        assert np.array_equal(got.aov[checks.ALBEDO][px], before.aov[checks.ALBEDO][px]), "%s: the ALBEDO pixel of a hit on the BC1 albedo differs from the plain compressed instance's" % name
        continuing = int((a[:, 0] != np.uint32(cases.SENTINEL)).sum())
        assert continuing > 50 and (px.size > 50 or not (bounce == 0).any()), name
        print("%-50s %4d hits on the BC1 albedo, %4d continue, %4d ALBEDO pixels: bit for bit the plain compressed instance's" % (name, textured.sum(), continuing, px.size))


@pytest.mark.parametrize("light", list(cases.LIGHT_VARIANTS), ids=lambda l: l.lstrip("_") or "plain")
def test_one_row_per_light_variant_without_mis(world, light):
    """MIS off: an emitter's and the sky's sample carry no weight (a delta light's never does)."""
    slot = tuple(cases.LIGHT_VARIANTS).index(light)
    _row(world, cases.instance_setup(light, mis_off=True), light, False, slot, False, tag="instances_mis_off")


def test_tree_row_with_nothing_taken(world):
    """The tree alone, neither sky nor delta lights taking a share: next_event_estimation<3> with taken == 0 sends every light sample to the tree."""
    tables, out = _row(world, cases.instance_setup("_tree", taken0=True), "_tree", False, 0, False, tag="instances_taken0")
    for launch, got, got_at, r in out:
        assert (r.route == ref.ROUTE_TREE).all() and np.isfinite(got.shadow_out[:got.counters[1], 6].view(np.float32)).all(), launch.name


@pytest.mark.parametrize("light", ["_split", "_tree"])
def test_smooth_rows_equal_the_plain_instance(world, light):
    """Dielectric and conductor below the roughness cutoff: their BSDFs allow no NEE, so a _split or _tree instance emits no shadow entry, sets no
    ALLOW_NEE, and equals the plain instance on the same entries in every output bit."""
    for slot in (2, 3):
        tables, out = _row(world, cases.instance_setup(light, smooth=True), light, False, slot, False, sides=False, tag="instances_smooth")
        plain = world.apply(cases.instance_setup("", smooth=True))
        for launch, got, got_at, r in out:
            assert got.counters[1] == 0 and got.counters[0] > 100, launch.name
            rec = got.trace_out[:got.counters[0]]
            assert ((rec[:, 10] & checks.FLAG_ALLOW_NEE) == 0).all() and (rec[:, 14] == np.uint32(cases.SENTINEL)).all(), launch.name
            assert instance(world, plain, launch) == cases.instance_name(slot, launch.merged, False, 0, False)
            before = checks.device_launch(world.grt, world.ctx, launch, capacity=launch.entries.n + 37)
            assert np.array_equal(got.counters, before.counters), launch.name
            for a, b, what in zip(_matched_rows(launch, got, launch.name), _matched_rows(launch, before, launch.name + " (plain)"), ("continuation", "shadow")):
                assert np.array_equal(a, b), "%s: a %s record differs from the plain instance's" % (launch.name, what)
            for field in ("aov", "gnd", "gid", "gsp"):
                assert np.array_equal(getattr(got, field), getattr(before, field)), "%s: %s differs from the plain instance's" % (launch.name, field)


@pytest.mark.parametrize("light", list(cases.LIGHT_VARIANTS), ids=lambda l: l.lstrip("_") or "plain")
def test_queue_lengths_of_every_light_variant(world, light):
    """One entry, one wave, a workgroup and one entry: structure and order."""
    setup = cases.instance_setup(light)
    tables = world.apply(setup)
    world.set_maps(tables, {})
    for launch in cases.instance_length_launches(world, tuple(cases.LIGHT_VARIANTS).index(light)):
        run(world, setup.name, tables, launch, sides=False)


@pytest.fixture(scope="module")
def wide_world(grt, oracle, tmp_path_factory):
    w = cases.WideWorld(grt, oracle, tmp_path_factory.mktemp("instances_wide"), 0)
    yield w
    w.apply(cases.SETUP["default"])
    w.close()


@pytest.mark.parametrize("light,slot", [("", 0), ("_tree", 3)], ids=["plain_diffuse", "tree_conductor"])
def test_second_round_of_the_merged_form(wide_world, light, slot):
    """8192 x 256 + 1 entries of the merged form (the suite's one large queue): structure on all of them, values on the last 257 and a seeded
    sample, MAX_VALUE_ENTRIES in all. The last entry is alone in the second grid-stride round of its workgroup."""
    world = wide_world
    setup = cases.instance_setup(light)
    tables = world.apply(setup)
    world.set_maps(tables, {})
    launch = cases.second_round_merged(world, slot, seed=6700 + slot)
    n = launch.entries.n
    assert n == cases.STREAM_GRID * cases.BLOCK + 1 and n > cases.STREAM_GRID * cases.BLOCK
    sample = cases.value_sample(n, 6710 + slot)
    assert sample.size <= cases.MAX_VALUE_ENTRIES and (sample[-257:] == np.arange(n - 257, n)).all()
    start = time.perf_counter()
    got, got_at, r = run(world, setup.name, tables, launch, sample=sample)
    assert got.counters[2] == n and got_at[0].size == sample.size
    print("%s: %d entries, %d continue, %d shadow rays, %.2f s" % (launch.name, n, got.counters[0], got.counters[1], time.perf_counter() - start))


@pytest.mark.parametrize("shares", [True, False], ids=["all_routes", "tree_alone"])
def test_launch_under_a_fog_volume(world, shares):
    """rt_set_fog_volume in force around rt_shade_rays: shade_material reads bounce 0's throughput from the queue (the ..._fog sort instance stores it), and
    the light tree is displaced -- the launch takes the _split instance where delta lights take a share, the plain one where the tree stood alone."""
    setup = cases.instance_setup("_tree", fog=True, taken0=not shares)
    expected = "_split" if shares else ""
    tables = world.apply(setup)
    world.set_maps(tables, {})
    assert tables.fog_active and tables.tree is not None
    for launch in cases.fog_launches(world):
        assert instance(world, tables, launch) == cases.instance_name(launch.slot, launch.merged, launch.slot < 2, cases.LIGHT_SUFFIXES.index(expected), False)
        first = launch.paths()[2] == 0
        assert first.sum() > 100 and (np.abs(launch.entries.throughput[first] - 1.0) > 0.05).all()
        got, got_at, r = run(world, setup.name, tables, launch)
        assert not (r.route == ref.ROUTE_TREE).any()
        # the check is sharp: with 1 in the place of the carried throughput the first hits' values are elsewhere by far more than the bound
        carried = r.robust & first & (got_at[0] >= 0) & ~r.textured
        written = got.trace_out[got_at[0][carried], 11:14].view(np.float32).astype(np.float64)
        assert carried.sum() > 50 and (np.abs(written - r.throughput[carried]).max(axis=1) < np.abs(written - r.throughput[carried] / launch.entries.throughput[carried]).max(axis=1)).all(), launch.name


def test_every_instance_was_launched():
    """The union of instance() over the launches this module ran is the list of rt_material.h, all 96 (test_material.py holds that list to the text)."""
    if len(CASES_DONE) < len(EVERY_CASE):
        pytest.skip("counts the launches of test_every_instance: run the whole module (%d of %d cases ran)" % (len(CASES_DONE), len(EVERY_CASE)))
    every = cases.all_instances()
    missing = sorted(every - set(RAN))
    print("%d of %d instances launched" % (len(every & set(RAN)), len(every)))
    assert len(every) == 96 and not missing and set(RAN) <= every, missing
