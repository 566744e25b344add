"""The sort launch on the CPU: the oracle's kernel_sort (oracle_sort) against the float64 reference of sort_reference.py, on the launches
of sort_cases.py. This is where the bounds and margins of sort_checks.py are measured -- every launch prints its share of non-robust
entries and its worst errors, the last test prints the worst of each over all launches next to 3 x that -- and where the cap on
non-robust entries is asserted, on the reference alone. The device is held to the same numbers in test_gpu_sort.py."""
import numpy as np
import pytest

import sort_cases as cases
import sort_checks as checks
import sort_reference as ref

WORST = {}   # quantity -> (error, "setup/launch"), over the whole module
DONE = set()


@pytest.fixture(scope="module")
def world(grt, oracle, tmp_path_factory):
    w = cases.World(grt, oracle, tmp_path_factory.mktemp("sort"), -1)
    yield w
    w.close()


def run(setup_name, tables, launch):
    name = "%s/%s" % (setup_name, launch.name)
    result = ref.evaluate(tables, launch, checks.MARGINS)
    allowed = ref.allowed_outcomes(tables, launch, checks.MARGINS, result)
    out = checks.oracle_launch(tables, launch, cases.SENTINEL)
    matched = checks.check_structure(name, tables, launch, out, result, allowed, cases.SENTINEL)
    errors = checks.compare_with_reference(name, tables, launch, out, matched, result, checks.BOUNDS)
    margins = checks.measure_margins(out, result)
    loose, reach = checks.non_robust_share(result)
    print("%-48s %8d entries, %6d of %8d next to a threshold; " % (name, launch.entries.n, loose, reach)
          + " ".join("%s %.2g" % (q, v[0]) for q, v in errors.items()) + " | " + " ".join("%s %.2g" % kv for kv in margins.items()))
    for quantity, (error, _) in errors.items():
        if error > WORST.get(quantity, (0.0, ""))[0]:
            WORST[quantity] = (error, name)
    for quantity, error in margins.items():
        assert error * 3.0 <= checks.MARGINS[quantity] * 1.0000001, "%s: the oracle's %s is %.3g from float64's: 3 x that is beyond the margin %.3g" % (name, quantity, error, checks.MARGINS[quantity])
        if error > WORST.get("margin " + quantity, (0.0, ""))[0]:
            WORST["margin " + quantity] = (error, name)
    if launch.name == "medium_edges":
        assert (~result.finite).sum() >= 20, "%s: the launch holds no entry that meets a NaN" % name
    if setup_name == "black_emitter" and launch.name.startswith("emitter_edges"):
        assert (result.light_pdf == 0).sum() >= 5 or launch.bounce == 0, "%s: no MIS-weighed hit on the black emitter" % name
    if not launch.name.startswith(checks.THRESHOLD_LAUNCHES):
        assert loose <= checks.NON_ROBUST_CAP * reach, "%s: %d of %d entries are next to a threshold" % (name, loose, reach)
    return result


def run_setup(world, setup):
    tables = world.apply(setup)
    seen = set()
    for launch in cases.plan(world, tables, setup):
        seen.update(np.unique(run(setup.name, tables, launch).outcome).tolist())
    DONE.add(setup.name)
    return seen


@pytest.mark.parametrize("setup", cases.SETUPS, ids=[s.name for s in cases.SETUPS])
def test_oracle_matches_float64(world, setup):
    seen = run_setup(world, setup)
    if setup.name == "default":
        assert seen == set(range(6)), "the launches of the default setup never reach outcome(s) %s" % sorted(set(range(6)) - seen)


def test_the_launches_reach_every_branch(world):
    """The mixed queue is worth its name: every class at every bounce, every medium, both kinds of emitter hit, both roulette outcomes."""
    tables = world.apply(cases.SETUP["default"])
    for launch in cases.mixed_launches(world):
        e, r = launch.entries, ref.evaluate(tables, launch, checks.MARGINS)
        types = tables.material_types[tables.material_ids[np.where(e.triangle >= 0, e.mesh, 0)]]
        assert (e.triangle < 0).sum() > 100
        for t in range(5):
            assert ((e.triangle >= 0) & (types == t)).sum() > 100, (launch.name, t)
        if launch.bounce > 0:
            for medium in (0, 1, 2):
                assert (e.inside & (e.medium == medium)).sum() > 100
            assert (r.outcome == ref.SCATTERED).sum() > 50 or launch.bounce == cases.NUM_BOUNCES - 1
            assert np.isfinite(r.light_pdf).sum() > 50 and np.isfinite(r.weight).sum() > 20
        if 0 < launch.bounce < cases.NUM_BOUNCES - 1:
            survived = (r.outcome < 4).sum(); culled = (np.isfinite(r.survival) & (r.outcome == ref.TERMINATED)).sum()
            assert survived > 100 and culled > 100, (launch.name, survived, culled)


def test_measured_bounds_are_three_times_the_worst_case(world):
    """Prints the table of sort_checks.py's docstring from this run, and holds the constants there to it: a bound is 3 x the worst oracle error
    over every launch (to the two digits it is written with), no more. (Runs the setups the session has not run yet.)"""
    for setup in cases.SETUPS:
        if setup.name not in DONE:
            run_setup(world, setup)
    rows = []
    for quantity, (error, name) in sorted(WORST.items()):
        key = quantity.replace("margin ", "")
        constant = checks.MARGINS[key] if quantity.startswith("margin") else checks.BOUNDS[key]
        rows.append((quantity, error, name, constant))
        print("%-20s worst %.3g  (%s)  3 x = %.3g  constant %.3g" % (quantity, error, name, 3 * error, constant))
    for quantity, error, name, constant in rows:
        assert 3 * error <= constant * 1.0000001 and constant <= 3 * error * 1.06, "%s: constant %.3g, 3 x the worst case (%.3g, %s) is %.3g" % (quantity, constant, error, name, 3 * error)
