"""The material launch on the CPU: the oracle's shade_material (oracle_shade) on the launches of material_cases.py, against the float64
restatement of material_reference.py and under the structure rules of material_checks.py -- the same rules, and the same code, the
device's launch is held to in test_gpu_material.py. This is where the bounds of material_checks.MEASURED are measured: every launch prints
its share of non-robust entries and its worst errors, the last test measures all launches afresh, prints the worst of each quantity and
holds the recorded constants to them. The cap on non-robust entries (0.5 % of a launch's entries, no floor) is asserted here on the
reference alone, for every launch that is not built on a threshold."""
import numpy as np
import pytest

import material_cases as cases
import material_checks as checks
import material_reference as ref
import sort_cases
import sort_checks

WORST = {}   # quantity -> (error, "setup/launch"), over the whole module

# |dot(direction, geometric normal)| or |omega_i.z| below this counts as next to the threshold: both are dot products of float32 unit
# vectors, three products and two sums, so eight rounding errors of 2^-24 at most
SETUP_MARGIN = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def world(grt, oracle, tmp_path_factory):
    w = cases.World(grt, oracle, tmp_path_factory.mktemp("material"), -1)
    yield w
    w.close()


def run(world, setup_name, tables, launch):
    name = "%s/%s" % (setup_name, launch.name)
    out = checks.oracle_launch(tables, launch)
    trace_at, shadow_at = checks.check_structure(name, tables, launch, out)
    r = ref.reference_of(world, tables, launch)
    # the oracle's own float32 numbers for the set-up's two comparisons: float64 must have flagged every one of them that is next to zero
    close = (np.abs(out.internals) <= SETUP_MARGIN).any(axis=1)
    assert not (close & ~(r.near_entering | r.near_alive)).any(), "%s: float64 calls an entry robust whose float32 set-up sits on a threshold" % name
    errors = checks.compare_with_reference(name, tables, launch, out, (trace_at, shadow_at), r, checks.BOUNDS)
    loose = int(r.near.sum())
    print("%-44s %6d entries, %6d continue, %6d shadow rays, %3d next to a threshold; " % (name, launch.entries.n, out.counters[0], out.counters[1], loose)
          + " ".join("%s %.2g" % (q, v[0]) for q, v in errors.items()))
    for quantity, (error, _) in errors.items():
        if error > WORST.get(quantity, (0.0, ""))[0]:
            WORST[quantity] = (error, name)
    if launch.name.startswith(cases.THRESHOLD_LAUNCHES):
        assert r.near_entering.sum() >= 8 and r.near_alive.sum() >= 8, "%s: the launch sits on no threshold (%d, %d)" % (name, r.near_entering.sum(), r.near_alive.sum())
    else:
        assert loose <= checks.NON_ROBUST_CAP * launch.entries.n, "%s: %d of %d entries are next to a threshold" % (name, loose, launch.entries.n)
    return out, trace_at, shadow_at


@pytest.mark.parametrize("setup", cases.SETUPS, ids=[s.name for s in cases.SETUPS])
def test_oracle_obeys_the_structure_rules(world, setup):
    tables = world.apply(setup)
    for launch in cases.plan(world, setup, tables):
        run(world, setup.name, tables, launch)


def test_the_launches_reach_every_branch(world):
    """Both faces of every material, dead entries (omega_i.z <= 0), entries that end in the BSDF, shadow rays, media through the dielectric."""
    tables = world.apply(cases.SETUP["default"])
    for launch in cases.value_launches(world):
        out, trace_at, shadow_at = run(world, "default", tables, launch)
        e = launch.entries
        bounce = launch.paths()[2]
        entering = out.internals[:, 0] < 0
        assert entering.sum() > 500 and (~entering).sum() > 500, launch.name
        assert (trace_at >= 0).sum() > 500 and (shadow_at >= 0).sum() > 100, launch.name
        assert ((trace_at < 0) & ~(out.internals[:, 1] > 0)).sum() >= 10, "%s: no entry ends in the set-up" % launch.name
        if launch.slot == 2:
            assert ((trace_at < 0) & (out.internals[:, 1] > 0)).sum() >= 1, "%s: no entry ends in the BSDF's sample" % launch.name
        if (bounce > 0).any():
            assert e.inside.sum() > 50
            rec = out.trace_out[trace_at[(trace_at >= 0) & e.inside]]
            assert ((rec[:, 10] & checks.FLAG_INSIDE_MEDIUM) != 0).sum() > 10, "%s: no entry stays inside its medium" % launch.name
        if launch.slot == 2:
            # the dielectric is the one surface a path crosses: some leave their medium, some enter the sphere's own
            went_in = out.trace_out[trace_at[(trace_at >= 0) & ~e.inside], 10] & checks.FLAG_INSIDE_MEDIUM
            came_out = out.trace_out[trace_at[(trace_at >= 0) & e.inside], 10] & checks.FLAG_INSIDE_MEDIUM
            assert (went_in != 0).sum() > 20 and ((came_out == 0).sum() > 5 or not (bounce > 0).any()), launch.name


def test_smooth_materials_write_no_last_pdf(world):
    """Below the roughness cutoff the dielectric and the conductor do not allow NEE: no shadow ray, no flag, last_pdf left alone."""
    tables = world.apply(cases.SETUP["smooth"])
    for launch in cases.small_launches(world):
        if launch.slot < 2:
            continue
        out, trace_at, _ = run(world, "smooth", tables, launch)
        rec = out.trace_out[:out.counters[0]]
        assert out.counters[0] > 100 and out.counters[1] == 0
        assert ((rec[:, 10] & checks.FLAG_ALLOW_NEE) == 0).all() and (rec[:, 14] == np.uint32(cases.SENTINEL)).all()


def test_unwritten_words_of_bounce_0_are_not_read(world):
    """At bounce 0 the sort stores neither throughput nor cone words: a launch whose input carries the sentinel there equals, bit for bit, the
    same launch with finite garbage there."""
    tables = world.apply(cases.SETUP["default"])
    for launch in [cases.per_bounce(world, "unwritten", slot, 600, 0, seed=1600 + slot) for slot in range(4)] + [cases.merged(world, "unwritten", 1, 1500, seed=1610)]:
        a, b = checks.oracle_launch(tables, launch), checks.oracle_launch(tables, launch, garbage=0.37)
        bounce = launch.paths()[2]
        assert (bounce == 0).sum() > 100
        for field in ("trace_out", "shadow_out", "counters", "aov", "gnd", "gid", "gsp"):
            assert np.array_equal(getattr(a, field), getattr(b, field)), "%s: %s depends on words the sort leaves unwritten" % (launch.name, field)


def test_sort_output_feeds_the_material_launch(world):
    """The chain's CPU half: a material queue of oracle_sort goes into oracle_shade unchanged (and counts among the launches the bounds are
    measured on)."""
    tables = world.apply(sort_cases.SETUP["default"])
    tables.config["aov_mask"] = cases.AOV_MASK
    world.view.scene.config.aov_mask = cases.AOV_MASK
    rng = np.random.default_rng(1700)
    for bounce in (0, 2):
        e = sort_cases.make_entries(world, rng, sort_cases.pixels_for(rng, 3000, world.frame_pixels, 1), bounce)
        launch = sort_cases.per_bounce(world, "chain_bounce%d" % bounce, e, bounce, slots=1)
        sorted_ = sort_checks.oracle_launch(tables, launch, cases.SENTINEL)
        for slot in range(4):
            n = int(sorted_.counters[slot])
            assert n > 50
            records = sorted_.material_out[slot, :n]
            fed = cases.from_records(world, "chain", slot, records, bounce, launch.sample_index)
            assert np.array_equal(fed.pack(), records), "the tests' material records are not the sort's"
            run(world, "chain", tables, fed)


LIGHT_CASES = [c for c in __import__("nee_cases").CPU_CASES if c.name in ("limit", "meshes65", "tris2049")]


@pytest.mark.parametrize("case", LIGHT_CASES, ids=lambda c: c.name)
def test_light_tables_within_and_beyond_the_lds_limits(grt, oracle, tmp_path, case):
    """The tail of next-event estimation on scenes whose light tables fit the shade kernels' LDS copy exactly (64 meshes, 2048 triangles) and
    exceed it by one (the oracle searches one table either way: what this pins is the launches and the float64 side)."""
    w = cases.LightsWorld(grt, oracle, case, tmp_path, -1)
    try:
        for launch in cases.light_table_launches(w):
            out, _, shadow_at = run(w, case.name, w.tables, launch)
            assert (shadow_at >= 0).sum() > 100
    finally:
        w.close()


def test_measured_bounds_are_four_times_the_worst_case(world, grt, oracle, tmp_path):
    """Prints the table of material_checks.MEASURED from this run and holds the constants there to it: a measured value is the worst oracle
    error over every launch of every setup and of the light-table scenes (to the three digits it is written with), and a bound is 4 x that.
    (Measured afresh here, whatever ran before.)"""
    WORST.clear()
    for case in LIGHT_CASES:
        w = cases.LightsWorld(grt, oracle, case, tmp_path / case.name, -1)
        try:
            for launch in cases.light_table_launches(w):
                run(w, case.name, w.tables, launch)
        finally:
            w.close()
    for setup in cases.SETUPS:
        tables = world.apply(setup)
        for launch in cases.plan(world, setup, tables):
            run(world, setup.name, tables, launch)
    test_sort_output_feeds_the_material_launch(world)
    for quantity, (error, name) in sorted(WORST.items()):
        print("%-18s worst %.3g  (%s)  recorded %.3g  bound %.3g" % (quantity, error, name, checks.MEASURED[quantity][0], checks.BOUNDS[quantity]))
    for quantity, (error, name) in sorted(WORST.items()):
        recorded = checks.MEASURED[quantity][0]
        assert error <= recorded * 1.0000001 and recorded <= error * 1.06, "%s: recorded %.3g, the worst case is %.3g (%s)" % (quantity, recorded, error, name)
        assert checks.BOUNDS[quantity] == 4.0 * recorded
