"""The material launch on the CPU: the oracle's shade_material (oracle_shade) on the launches of material_cases.py, against the float64
restatement of material_reference.py and under the structure rules of material_checks.py -- the same rules, and the same code, the
device's launch is held to in test_gpu_material.py. This is where the bounds of material_checks.MEASURED are measured: every launch prints
its share of non-robust entries and its worst errors, the last test measures all launches afresh, prints the worst of each quantity and
holds the recorded constants to them. The cap on non-robust entries (0.5 % of a launch's entries, no floor) is asserted here on the
reference alone, for every launch that is not built on a threshold.

The _sky, _nmap and _sky_nmap variants of the launch have no oracle side. For them this module holds the float64 composition itself
(material_reference.py with a sky share and normal maps) to facts it does not share with the kernel -- the estimator's closed-form mean, the
route's edges and probabilities, the mapped frame's handedness, the view guard's floor, the fallbacks --, asserts the cap on left-out entries
of every launch of test_gpu_material_variants.py, and measures the two bounds those launches need beyond MEASURED's: the oracle's throughput
error on VariantWorld's launches and the float32 restatement of the mapped normal."""
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


@pytest.mark.parametrize("setup", cases.PLAIN_SETUPS, ids=[s.name for s in cases.PLAIN_SETUPS])
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
    for setup in cases.PLAIN_SETUPS:
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


# ---- the variants of the launch (_sky, _nmap, _sky_nmap): the float64 side alone -- the oracle samples no sky and knows no normal map ----

@pytest.fixture(scope="module")
def variant_world(grt, oracle, tmp_path_factory):
    w = cases.VariantWorld(grt, oracle, tmp_path_factory.mktemp("variants"), -1)
    yield w
    w.close()


def count_left_out(world, setup_name, tables, launch, sides=True):
    """The near flags are the reference's alone: the cap on left-out entries can be asserted here, without a device."""
    name = "%s/%s" % (setup_name, launch.name)
    r = ref.reference_of(world, tables, launch)
    n = launch.entries.n
    sky, emitter = r.to_sky & r.has_shadow & r.robust, ~r.to_sky & r.has_shadow & r.robust
    print("%-52s %5d entries, %4d sky and %4d emitter shadow entries held, %4d mapped (%4d fell back), %3d next to a threshold" % (
        name, n, sky.sum(), emitter.sum(), r.mapped.sum(), r.map_fallback.sum(), r.near.sum()))
    assert r.near.sum() <= checks.NON_ROBUST_CAP * n, "%s: %d of %d entries are next to a threshold" % (name, r.near.sum(), n)
    if sides:
        share, lit = tables.sky_share, tables.lights_total_weight > 0
        assert sky.sum() > 100 or not share > 0, "%s: %d robust sky entries" % (name, sky.sum())
        assert emitter.sum() > 100 or not (lit and share < 1), "%s: %d robust emitter entries" % (name, emitter.sum())
        if tables.map_ids is not None:
            assert (r.mapped & r.robust).sum() > 100 and (~r.mapped & r.robust).sum() > 100 or launch.name.startswith(("nmap_mirrored", "nmap_degenerate")), name
    return r


@pytest.mark.parametrize("setup", cases.SKY_SETUPS, ids=[s.name for s in cases.SKY_SETUPS])
def test_sky_launches_keep_the_cap(variant_world, setup):
    world = variant_world
    tables = world.apply(setup)
    tables.map_ids = None
    for launch in cases.sky_launches(world, setup):
        count_left_out(world, setup.name, tables, launch)
    if setup.name == "sky_share_0.5":
        for launch in cases.sky_length_launches(world):
            count_left_out(world, setup.name, tables, launch, sides=False)
        for maps, launch in cases.sky_map_launches(world):
            world.set_maps(tables, maps)
            count_left_out(world, setup.name, tables, launch)


def test_mapped_launches_keep_the_cap(variant_world):
    world = variant_world
    tables = world.apply(cases.SETUP["svgf_on"])
    for maps, launch in cases.map_launches(world):
        world.set_maps(tables, maps)
        launch._reference = None   # (one tables object, another set of maps)
        r = count_left_out(world, "svgf_on", tables, launch)
        if launch.name.startswith("nmap_degenerate"):
            assert r.mapped.all() and r.map_fallback.all()
        if launch.name.startswith("nmap_mirrored"):
            assert r.mapped.all() and not r.map_fallback.any() and (world.uv_det[launch.entries.triangle] < 0).all()


def test_sky_launch_on_global_light_tables_keeps_the_cap(grt, oracle, tmp_path):
    case = [c for c in LIGHT_CASES if c.name == "meshes65"][0]
    w = cases.LightsWorld(grt, oracle, case, tmp_path, -1)
    try:
        w.map_ids = None
        tables = cases.lights_world_sky(w, 0.5, np.ascontiguousarray(__import__("sky_sampling_reference").sun_sky(64, 32, sun=(40, 9), sun_value=300.0)))
        tables.map_ids = None
        count_left_out(w, "meshes65_sky_share_0.5", tables, cases.sky_lights_launch(w))
    finally:
        w.close()


def _up_facing_hits(world, n, bounce=0):
    """n copies of one hit of the untextured diffuse sphere's instance (a translation) on the level triangle of bare.obj: the shading and the
    geometric normal are +y exactly, the ray arrives straight down."""
    tri = np.asarray(world.view.keep["triangles"], np.float32).reshape(-1, 24).astype(np.float64)
    level = np.nonzero((world.uv_det == 0) & (tri[:, 10] == 1.0) & (np.abs(tri[:, 12:18]).sum(axis=1) == 0) & (np.cross(tri[:, 3:6], tri[:, 6:9])[:, 1] > 0))[0]
    assert level.size == 1, level
    mesh = [i for i in world.instances[cases.DIFFUSE] if not world.textured_instance[i] and not world.transformed_instance[i]][0]
    slots = n // world.frame_pixels
    launch = cases.per_bounce(world, "up", 0, n, bounce, seed=1, slots=slots, inside_share=0.0)
    e = launch.entries
    e.pixel[:] = np.arange(n)
    e.mesh[:] = mesh; e.triangle[:] = level[0]; e.u16[:] = 20000; e.v16[:] = 30000; e.t[:] = 1.0
    e.direction[:] = [0.0, -1.0, 0.0]
    return launch


def _with_random(tables, light_x, pair):
    """`tables` with DIM_NEE_LIGHT.x and the DIM_NEE_TRIANGLE pair replaced: a stratified grid instead of the generator's numbers."""
    import copy
    out = copy.copy(tables)
    plain = tables.random

    def random(dimension, *key):
        v = plain(dimension, *key).copy()
        if dimension == ref.DIM_NEE_LIGHT:
            v[:, 0] = light_x
        if dimension == ref.DIM_NEE_TRIANGLE:
            v[:] = pair
        return v
    out.random = random
    return out


GRID = 256   # the stratified grid of the estimator's mean: GRID x GRID points, jittered by a fixed generator


def _grid():
    rng = np.random.default_rng(77)
    i, j = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
    return ((np.stack([i.ravel(), j.ravel()], axis=1) + rng.random((GRID * GRID, 2))) / GRID).astype(np.float32)


@pytest.mark.parametrize("sky", ["hdr", "one"])
def test_sky_estimator_has_the_closed_form_mean(variant_world, sky):
    """A diffuse hit with its normal up. MIS off: the reference's sky entries -- every light sample sent there, times the share s with which one
    goes there -- average to albedo / pi x the upper hemisphere's irradiance under the bilinear sky (a quadrature, sky_sampling_reference.py).
    MIS on, shares 0.25 and 0.5: that half plus the BSDF-sampled half, a cosine-distributed ray that misses and is weighed by the sort launch's
    restatement (sort_reference.py: power_heuristic(last_pdf, s x sky_pdf)), has the same mean. Tolerance: five standard errors of the mean,
    from the samples themselves (an upper estimate for a stratified grid). A wrong factor s, 1 - s, pdf or weight in either half shows."""
    import sky_sampling_reference as sky_ref
    import sort_reference
    world = variant_world
    pair = _grid()
    n = pair.shape[0]
    launch = _up_facing_hits(world, n)
    albedo = None
    for mis, shares in ((0, (0.5,)), (1, (0.25, 0.5))):
        for share in shares:
            setup = cases.Setup("mean", {"enable_multiple_importance_sampling": mis}, sky=sky, sky_sampling=share)
            tables = world.apply(setup)
            tables.map_ids = None
            r = ref.evaluate(world, _with_random(tables, 0.0, pair), launch, world.bsdf_tables)
            assert r.alive.all() and r.to_sky.all() and np.allclose(r.normal, [0.0, 1.0, 0.0], atol=1e-12) and not r.textured.any()
            albedo = tables.materials[tables.material_ids[launch.entries.mesh[0]], :3].astype(np.float64)
            want = albedo / np.pi * sky_ref.upper_hemisphere_irradiance(tables.sky, tables.sky_scale)
            samples = share * np.where(r.has_shadow[:, None], r.illumination, 0.0)
            if mis:
                # the other half: cosine-distributed directions about +y from the same grid, as misses of the sort launch at the next bounce
                phi, cos_t = 2.0 * np.pi * pair[:, 0].astype(np.float64), np.sqrt(1.0 - pair[:, 1].astype(np.float64))
                sin_t = np.sqrt(1.0 - cos_t * cos_t)
                e = sort_reference.Entries(n)
                e.pixel[:] = np.arange(n); e.direction[:] = np.stack([sin_t * np.cos(phi), cos_t, sin_t * np.sin(phi)], axis=1)
                e.triangle[:] = sort_reference.INVALID; e.t[:] = np.inf
                e.throughput[:] = albedo; e.allow_nee[:] = True; e.last_pdf[:] = e.direction[:, 1] / np.float32(np.pi)
                miss = sort_cases.per_bounce(world, "mean_miss", e, 1, slots=n // world.frame_pixels)
                s = sort_reference.evaluate(tables, miss, sort_checks.MARGINS)
                assert np.isfinite(s.weight).all()
                samples = samples + e.throughput.astype(np.float64) * s.sky * s.weight[:, None]
            mean, error = samples.mean(axis=0), samples.std(axis=0, ddof=1) / np.sqrt(n)
            print("sky %s, share %g, MIS %d: mean %s, closed form %s, standard error %s" % (sky, share, mis, mean, want, error))
            assert (np.abs(mean - want) <= 5.0 * error).all(), (sky, share, mis, mean.tolist(), want.tolist(), error.tolist())
            assert (error <= 0.05 * want).all(), "the tolerance says nothing: standard error %s of %s" % (error, want)


@pytest.mark.parametrize("share", [0.25, 0.5, 0.3])
def test_routing_of_the_light_samples(variant_world, share):
    """u < s goes to the sky, decided in float32; the emitters' number starts at 0 where u = s and never reaches 1; over a fine grid of u the
    sky gets s and every emitter mesh (1 - s) x its table probability, so the probabilities sum to 1."""
    s = np.float32(share)
    edge = np.array([0.0, np.nextafter(s, np.float32(0)), s, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    to_sky, rescaled = ref.route(edge, s)
    assert to_sky.tolist() == [True, True, False, False]
    assert rescaled[2] == 0.0 and rescaled[3] < 1.0 and rescaled[3] <= ref.ONE_BELOW_ONE and rescaled.dtype == np.float32
    n = 1 << 20
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    to_sky, rescaled = ref.route(u, s)
    assert ((rescaled[~to_sky] >= 0.0) & (rescaled[~to_sky] < 1.0)).all() and (np.diff(rescaled[~to_sky]) >= 0).all()
    assert abs(to_sky.mean() - float(s)) <= 2.0 / n
    mesh_cdf = np.asarray(variant_world.light_tables[2], np.float32)
    p_mesh = np.diff(mesh_cdf.astype(np.float64), prepend=0.0)
    picked = np.minimum(np.searchsorted(mesh_cdf, rescaled[~to_sky], side="left"), mesh_cdf.size - 1)   # (either side: a grid point on an entry is one in a million)
    got = np.bincount(picked, minlength=mesh_cdf.size) / n
    assert np.allclose(got, (1.0 - float(s)) * p_mesh, atol=4.0 / n), (got, p_mesh)
    assert abs(to_sky.mean() + got.sum() - 1.0) <= 1e-12 and abs(float(s) + ((1.0 - float(s)) * p_mesh).sum() - 1.0) <= 1e-6


def test_mapped_normals_of_the_reference(variant_world):
    """The composition of normal_map_reference.py with the launch's set-up, on the mapped launches: the (128, 128, 255) map moves no normal
    further than 8 bits leave it; the frame follows dp/du and dp/dv on regular and on mirrored triangles (so a mirrored one is left-handed
    about the normal, and the mapped normal still right); under the (128, 128, 0) map the view guard leaves cos_view >= eps / sqrt(1 + eps^2), eps less a rounding of the guard's own formula; every fallback
    condition returns the flipped interpolated normal."""
    import normal_map_reference as nm
    world = variant_world
    tables = world.apply(cases.SETUP["svgf_on"])
    launches = {launch.name: (maps, launch) for maps, launch in cases.map_launches(world)}

    def evaluated(name):
        maps, launch = launches[name]
        world.set_maps(tables, maps)
        return launch, ref.evaluate(world, tables, launch, world.bsdf_tables)

    # the unperturbed normal within 8 bits: t = (1, 1, 255) / 255 in the frame, the angle constant_map_normal's vector makes with its quad's +y
    launch, r = evaluated("nmap_flat_conductor_bounce0_1500")
    decoded = nm.constant_map_normal(cases.FLAT).astype(np.float64)
    bound = np.arccos(decoded[1] / np.linalg.norm(decoded))
    angle = np.arccos(np.clip((r.normal * r.interpolated_normal).sum(axis=1), -1.0, 1.0))
    unguarded = r.mapped & ((-launch.entries.direction.astype(np.float64) * r.interpolated_normal).sum(axis=1) > 0.05)
    assert unguarded.sum() > 100 and 0.9 * bound <= angle[unguarded].max() <= bound * (1.0 + 1e-5), (angle[unguarded].max(), bound)
    assert np.array_equal(r.normal[~r.mapped], r.interpolated_normal[~r.mapped])

    # the frame: T along dp/du, B along dp/dv, whatever the sign of uv_det
    for name, sign in (("nmap_mirrored_conductor_bounce0_1500", -1.0), ("nmap_conductor_bounce0_1500", 0.0)):
        launch, r = evaluated(name)
        e = launch.entries
        m = r.mapped
        tri = tables.triangles[e.triangle[m]].astype(np.float64)
        u = (e.u16[m].astype(np.float32) / np.float32(65535.0)).astype(np.float64); v = (e.v16[m].astype(np.float32) / np.float32(65535.0)).astype(np.float64)
        fr = nm.frame(ref.map_records(tri, u, v, tables.transforms[e.mesh[m]].astype(np.float64), e.direction[m].astype(np.float64)))
        det = fr["det"]
        assert (np.sign(det) == sign).all() if sign else ((det > 0).sum() > 100 and (det < 0).sum() > 10)
        W = tables.transforms[e.mesh[m]].astype(np.float64)[:, :, :3]
        e1, e2, duv1, duv2 = tri[:, 3:6], tri[:, 6:9], tri[:, 20:22], tri[:, 22:24]
        dpdu = np.einsum("nij,nj->ni", W, (duv2[:, 1:2] * e1 - duv1[:, 1:2] * e2) / det[:, None])
        dpdv = np.einsum("nij,nj->ni", W, (-duv2[:, 0:1] * e1 + duv1[:, 0:1] * e2) / det[:, None])
        assert ((fr["T"] * dpdu).sum(axis=1) > 0).all() and ((fr["B"] * dpdv).sum(axis=1) > 0).all(), name
        handed = (np.cross(fr["T"], fr["B"]) * fr["n"]).sum(axis=1)
        assert np.allclose(np.abs(handed), 1.0, atol=1e-9)
        assert (np.sign(handed) == np.sign(det) * np.sign((fr["ng"] * fr["n"]).sum(axis=1))).all(), name
        # ... and the tilt map leans the normal towards +T (t.x > 0) and -B (t.y < 0) on both
        lean = np.where(r.entering[m][:, None], r.normal[m], -r.normal[m])
        free = (-e.direction[m].astype(np.float64) * r.normal[m]).sum(axis=1) > 0.05   # (the view guard has not moved it)
        assert ((lean * fr["T"]).sum(axis=1)[free] > 0).all() and ((lean * fr["B"]).sum(axis=1)[free] < 0).all(), name

    # the view guard
    launch, r = evaluated("nmap_inward_conductor_bounce0_1500")
    cos_view = (-launch.entries.direction.astype(np.float64) * r.normal).sum(axis=1)
    # (t.z = -1 points away from every viewer: the guard fires on each. It adds (eps - cos) w BEFORE normalising, and the sum is
    # sqrt(1 - cos^2 + eps^2) long: the cosine it leaves is eps over that, at least eps / sqrt(1 + eps^2) = eps (1 - 5e-5), and eps or more unless |cos| < eps)
    floor = nm.EPS / np.sqrt(1.0 + nm.EPS ** 2)
    assert r.mapped.sum() > 100 and (cos_view[r.mapped] >= floor - 1e-12).all() and (cos_view[r.mapped] > 0.9999 * nm.EPS).all()
    assert r.alive[r.mapped].all()

    # the fallbacks, one by one
    launch, r = evaluated("nmap_degenerate_conductor_bounce0_1500")
    assert r.map_fallback.all() and np.array_equal(r.normal, r.interpolated_normal)
    maps, launch = launches["nmap_conductor_bounce0_1500"]
    e = launch.entries
    tri = tables.triangles[e.triangle].astype(np.float64)
    u = np.full(e.n, 0.25); v = np.full(e.n, 0.25)
    W = tables.transforms[e.mesh].astype(np.float64)
    rec = ref.map_records(tri, u, v, W, e.direction.astype(np.float64))
    tilt = np.repeat(np.array([cases.TILT], np.float64) / 255.0, e.n, axis=0)
    plain = nm.frame(rec)
    flipped = plain["n"] * np.where(plain["entering"], 1.0, -1.0)[:, None]
    for what, change in (("det is not finite", lambda a: a.__setitem__((slice(None), 20), np.inf)),
                         ("det is 0", lambda a: a.__setitem__((slice(None), slice(20, 24)), 0.0))):
        broken = rec.copy(); change(broken)
        with np.errstate(all="ignore"):
            got, fallback, _ = nm.perturb(broken, tilt)
        assert fallback.all() and np.array_equal(got, flipped), what
    # dp/du along the normal: the vertex normals all point along dp/du
    along = rec.copy()
    det = plain["det"][:, None]
    dpdu_local = (along[:, 23:24] * along[:, 3:6] - along[:, 21:22] * along[:, 6:9]) / det
    along[:, 9:12] = dpdu_local; along[:, 12:18] = 0.0
    rigid = np.abs(np.linalg.norm(W[:, 0, :3], axis=1) - 1.0) < 1e-3   # (under a rigid transform the world normal is then along the world dp/du)
    got, fallback, info = nm.perturb(along[rigid], tilt[rigid])
    f = nm.frame(along[rigid])
    assert rigid.sum() > 100 and fallback.all() and np.array_equal(got, f["n"] * np.where(f["entering"], 1.0, -1.0)[:, None]), "|t|^2 <= 1e-8 |dpdu|^2"
    got, fallback, _ = nm.perturb(rec, np.full((e.n, 3), 0.5))
    assert fallback.all() and np.array_equal(got, flipped), "m == 0"
    got, fallback, _ = nm.perturb(rec, tilt)
    assert not fallback.any() and (np.abs(got - flipped).max(axis=1) > 1e-2).all()


def _oracle_on_variant_launches(world):
    """The oracle's plain shade_material (no maps) on the mapped launches of VariantWorld against float64: {quantity: (worst error, launch)}."""
    tables = world.apply(cases.SETUP["svgf_on"])
    tables.map_ids = None
    worst = {}
    for maps, launch in cases.map_launches(world):
        launch._reference = None
        name = "svgf_on/" + launch.name
        out = checks.oracle_launch(tables, launch)
        at = checks.check_structure(name, tables, launch, out)
        errors = checks.compare_with_reference(name, tables, launch, out, at, ref.reference_of(world, tables, launch), None)
        launch._reference = None
        for quantity, (error, _) in errors.items():
            if error > worst.get(quantity, (0.0, ""))[0]:
                worst[quantity] = (error, name)
    return worst


def test_variant_world_bound_is_four_times_the_worst_case(variant_world):
    """VariantWorld's launches draw other hits than World's, and one quantity's float32 error on them exceeds what World's launches showed: the
    throughput of the rough dielectric's and conductor's sample (1 - E of the Kulla-Conty tables is ill-conditioned). Its bound is measured as the others are: the
    oracle -- the float32 restatement of the plain instance, which every unmapped hit runs -- against float64 on the same launches with no map
    in force; material_checks.MEASURED["variant_throughput"] is this run's maximum, the device is held to 4 x it. Every other quantity stays
    within its recorded worst case times 4 here too."""
    worst = _oracle_on_variant_launches(variant_world)
    for quantity, (error, name) in sorted(worst.items()):
        print("%-18s worst %.3g  (%s)  bound %.3g" % (quantity, error, name, checks.BOUNDS[quantity]))
    error, name = worst["throughput"]
    recorded, launch = checks.MEASURED["variant_throughput"]
    assert error <= recorded * 1.0000001 and recorded <= error * 1.06 and launch == name, "variant_throughput: recorded %.3g (%s), the worst case is %.3g (%s)" % (recorded, launch, error, name)
    assert checks.BOUNDS["variant_throughput"] == 4.0 * recorded
    for quantity, (error, name) in worst.items():
        if quantity != "throughput":
            assert error <= checks.BOUNDS[quantity], "%s: the oracle is %.3g from float64 on %s" % (quantity, error, name)


def test_mapped_normal_bound_is_four_times_the_float32_restatement(variant_world):
    """A mapped normal the view guard has moved does not hold under BOUNDS["normal"] on the device (2.0e-6 against 5.8e-7 on
    nmap_inward_conductor_bounce0_1500): the guard's sum m + (eps - cos) w is sqrt(1 - cos^2 + eps^2) long, down to eps = 1e-2 where the map
    points straight away from the viewer, and normalising it divides the frame's float32 error by that length. The bound is therefore that of
    a float32 restatement of the set-up and normal_map_perturb (material_reference.mapped_normal32, operation by operation as rt_shading.h and
    shade_material have them), measured against float64 on the mapped hits at bounce 0 of the same launches, away from the thresholds:
    material_checks.MEASURED["mapped_normal"] is this run's maximum, and the device is held to 4 x it."""
    world = variant_world
    tables = world.apply(cases.SETUP["svgf_on"])
    worst = (0.0, "")
    for maps, launch in cases.map_launches(world):
        world.set_maps(tables, maps)
        r = ref.evaluate(world, tables, launch, world.bsdf_tables)
        e, bounce = launch.entries, launch.paths()[2]
        texel = list(maps.values())[0]
        got, fallback = ref.mapped_normal32(tables.triangles[e.triangle], e.u16, e.v16, tables.transforms[e.mesh], e.direction, texel)
        held = r.mapped & r.robust & r.alive & (bounce == 0)
        assert np.array_equal(fallback[held], r.map_fallback[held]), launch.name
        error = np.abs(got[held].astype(np.float64) - r.normal[held]).max(axis=1)
        print("%-48s %5d mapped hits at bounce 0, float32 within %.3g of float64" % (launch.name, held.sum(), error.max(initial=0.0)))
        if error.max(initial=0.0) > worst[0]:
            worst = (float(error.max()), "svgf_on/" + launch.name)
    recorded, name = checks.MEASURED["mapped_normal"]
    print("mapped_normal      worst %.3g  (%s)  recorded %.3g  bound %.3g" % (worst[0], worst[1], recorded, checks.BOUNDS["mapped_normal"]))
    assert worst[0] <= recorded * 1.0000001 and recorded <= worst[0] * 1.06 and name == worst[1], "mapped_normal: recorded %.3g (%s), the worst case is %.3g (%s)" % (recorded, name, worst[0], worst[1])
    assert checks.BOUNDS["mapped_normal"] == 4.0 * recorded


# ---- every instance of the launch (test_gpu_material_instances.py): the conditions on its launches, from the reference alone ----------

def test_instance_names_are_the_list_of_rt_material():
    """The 96 names material_cases.instance() can form, by the rule, are the entry points the slots' units define from rt_material.h: the rows of
    RT_MATERIAL_KERNEL_LIST times the suffixes of RT_MATERIAL_KERNEL_VARIANTS times the two forms, read as text. The selector is kernels_material.hip's."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-raytracer_amd", "csrc")
    by_rule, listed = cases.all_instances(), cases.listed_instances(os.path.join(csrc, "rt_material.h"))
    assert len(by_rule) == 96 and by_rule == listed, sorted(by_rule ^ listed)
    text = open(os.path.join(csrc, "kernels_material.hip")).read()
    assert "const int variant = (p.normal_map_slots >> material_slot & 1) * 4 + rt_light_split(p);" in text   # (the index the docstrings quote)


def routes_held(world, setup_name, tables, launch, sides=True):
    """The conditions test_gpu_material_variants.run asserts, as far as the reference alone decides them: the left-out share within NON_ROBUST_CAP, the
    routes a partition of the entries, every route in force holding more than 100 robust shadow entries. Returns the Result and the counts."""
    name = "%s/%s" % (setup_name, launch.name)
    r = ref.evaluate(world, tables, launch, world.bsdf_tables)
    n = launch.entries.n
    held = r.robust & r.has_shadow
    routes = [int((held & (r.route == k)).sum()) for k in range(4)]
    print("%-58s %-46s %5d entries, held: %4d sky, %4d delta, %4d by power, %4d by tree; %4d mapped; %3d next to a threshold" % (
        name, cases.instance(world, tables, launch), n, *routes, (r.mapped & r.robust).sum(), r.near.sum()))
    assert r.near.sum() <= checks.NON_ROBUST_CAP * n, "%s: %d of %d entries are next to a threshold" % (name, r.near.sum(), n)
    in_force = [ref.route_in_force(tables, k) for k in range(4)]
    assert sum(int((r.route == k).sum()) for k in range(4)) == n and all(in_force[k] or not (r.route == k).any() for k in range(4)), "%s: the routes do not partition the entries" % name
    assert np.array_equal(r.route == ref.ROUTE_SKY, r.to_sky) and np.array_equal(r.route == ref.ROUTE_DELTA, r.to_delta), name
    assert not (r.has_shadow & ~np.array(in_force)[r.route]).any(), name
    # the route says what the shadow ray looks like: to infinity for the sky and for a directional light, finite otherwise
    endless = np.isposinf(r.shadow_distance[r.has_shadow])
    directional = np.zeros(n, bool)
    if r.to_delta.any():
        directional = r.to_delta & (tables.delta.table.type[np.maximum(r.delta_light, 0)] == 2)
    assert np.array_equal(endless, (r.to_sky | directional)[r.has_shadow]), name
    if sides:
        for k in range(4):
            assert routes[k] > 100 or not in_force[k], "%s: %d robust %s entries" % (name, routes[k], ref.ROUTE_NAMES[k])
    return r, routes


@pytest.mark.parametrize("case", cases.INSTANCE_CASES, ids=cases.instance_case_id)
def test_instance_launches_keep_the_conditions(variant_world, case):
    world = variant_world
    light, mapped, slot, compressed = case
    setup = cases.instance_setup(light, compressed)
    tables = world.apply(setup)
    assert ref.route_in_force(tables, ref.ROUTE_SKY) == (light != "") and ref.route_in_force(tables, ref.ROUTE_DELTA) == (light in ("_split", "_tree"))
    assert ref.route_in_force(tables, ref.ROUTE_TREE) == (light == "_tree") and ref.route_in_force(tables, ref.ROUTE_POWER) == (light != "_tree")
    for maps, launch in cases.instance_launches(world, light, mapped, slot, compressed):
        world.set_maps(tables, maps)
        world.textures_compressed = compressed   # (without a device no texture is uploaded: what instance() reads)
        try:
            assert cases.instance(world, tables, launch) == cases.instance_name(slot, launch.merged, slot < 2 and not compressed, tuple(cases.LIGHT_VARIANTS).index(light), mapped)
        finally:
            world.textures_compressed = False
        r, routes = routes_held(world, setup.name, tables, launch)
        assert not mapped or ((r.mapped & r.robust).sum() > 100 and (~r.mapped & r.robust).sum() > 100), launch.name
        if compressed:
            # the textured materials' albedo is the BC1 texture; the oracle fetches it from the decoded chain, and no fetch falls below the floor
            bc1 = tables.materials[:, 3].view(np.int32) == world.bc1_index
            on_bc1 = bc1[tables.material_ids[launch.entries.mesh]]
            assert bc1.sum() == 2 and np.array_equal(on_bc1, r.textured) and on_bc1.sum() > 100, launch.name
            assert min(int(level.min()) for level in world.bc1.levels()) >= 64 and 64 / 255 >= cases.ALBEDO_FLOOR
            if light == "" and not mapped:
                out = checks.oracle_launch(tables, launch)
                checks.check_structure(setup.name + "/" + launch.name, tables, launch, out)
                px = launch.entries.pixel[on_bc1 & (launch.paths()[2] == 0) & r.alive]
                albedo = out.aov[checks.ALBEDO][px, :3].view(np.float32)
                first = (launch.paths()[2] == 0).any()   # (the ALBEDO frame is written at bounce 0)
                assert (px.size > 50 and np.unique(albedo).size > 50 if first else px.size == 0) and (albedo >= cases.ALBEDO_FLOOR).all() and (albedo <= 1.0).all(), launch.name


def test_instance_launches_are_the_shortest_that_hold_every_route(variant_world):
    """INSTANCE_LENGTHS is the shortest rung, not the shortest queue: the first rung of the ladder (steps of LENGTH_STEP) at which every launch of INSTANCE_CASES holds more than 100 robust entries on every
    route in force: one rung lower, some launch of each form holds 100 or fewer on some route. (The case above asserts the rung itself.)"""
    world = variant_world
    short = [False, False]
    lower = tuple(n - cases.LENGTH_STEP for n in cases.INSTANCE_LENGTHS)
    for light, mapped, slot, compressed in cases.INSTANCE_CASES:
        if all(short):
            break
        setup = cases.instance_setup(light, compressed)
        tables = world.apply(setup)
        for form, (maps, launch) in enumerate(cases.instance_launches(world, light, mapped, slot, compressed, lengths=lower)):
            world.set_maps(tables, maps)
            r = ref.evaluate(world, tables, launch, world.bsdf_tables)
            held = r.robust & r.has_shadow
            if any(ref.route_in_force(tables, k) and (held & (r.route == k)).sum() <= 100 for k in range(4)):
                print("%s/%s: a route holds 100 entries or fewer at %d" % (setup.name, launch.name, launch.entries.n))
                short[form] = True
    assert all(short) and cases.INSTANCE_LENGTHS[0] <= 1500 and cases.INSTANCE_LENGTHS[1] <= 2500, short


def test_further_instance_launches_keep_the_conditions(variant_world, grt, oracle, tmp_path):
    """MIS off, the tree with nothing taken, the smooth rows, the queue lengths, the fog launches, and the sampled entries of the merged form's second round."""
    world = variant_world
    for light in cases.LIGHT_VARIANTS:
        index = tuple(cases.LIGHT_VARIANTS).index(light)
        setup = cases.instance_setup(light, mis_off=True)
        tables = world.apply(setup); world.set_maps(tables, {})
        for maps, launch in cases.instance_launches(world, light, False, index, False, tag="instances_mis_off"):
            routes_held(world, setup.name, tables, launch)
        setup = cases.instance_setup(light)
        tables = world.apply(setup); world.set_maps(tables, {})
        for launch in cases.instance_length_launches(world, index):
            routes_held(world, setup.name, tables, launch, sides=False)
    setup = cases.instance_setup("_tree", taken0=True)
    tables = world.apply(setup); world.set_maps(tables, {})
    for maps, launch in cases.instance_launches(world, "_tree", False, 0, False, tag="instances_taken0"):
        r, routes = routes_held(world, setup.name, tables, launch)
        assert (r.route == ref.ROUTE_TREE).all() and cases.light_split(tables) == 3
    for light in ("_split", "_tree"):
        setup = cases.instance_setup(light, smooth=True)
        tables = world.apply(setup); world.set_maps(tables, {})
        for slot in (2, 3):
            for maps, launch in cases.instance_launches(world, light, False, slot, False, tag="instances_smooth"):
                r, routes = routes_held(world, setup.name, tables, launch, sides=False)
                assert not r.has_shadow.any() and not r.allow_nee.any() and r.continues.sum() > 100
    for changes, split in ((dict(), 2), (dict(taken0=True), 0)):
        setup = cases.instance_setup("_tree", fog=True, **changes)
        tables = world.apply(setup); world.set_maps(tables, {})
        assert tables.tree is not None and cases.light_split(tables) == split
        for launch in cases.fog_launches(world):
            r, routes = routes_held(world, setup.name, tables, launch)
            first = launch.paths()[2] == 0
            assert not (r.route == ref.ROUTE_TREE).any() and first.sum() > 100 and np.isfinite(r.throughput[first & r.continues & ~r.textured]).all()
    wide = cases.WideWorld(grt, oracle, tmp_path, -1)
    try:
        for light, slot in (("", 0), ("_tree", 3)):
            setup = cases.instance_setup(light)
            tables = wide.apply(setup); wide.set_maps(tables, {})
            launch = cases.second_round_merged(wide, slot, seed=6700 + slot)
            sample = cases.value_sample(launch.entries.n, 6710 + slot)
            assert launch.entries.n == 8192 * 256 + 1 and np.unique(launch.entries.pixel).size == launch.entries.n and launch.frame_slots <= 512
            routes_held(wide, setup.name, tables, launch.sub(sample))
    finally:
        wide.close()


@pytest.mark.parametrize("sky_share", [0.0, 0.5])
def test_a_delta_share_no_number_reaches_is_the_launch_without_delta_lights(variant_world, sky_share):
    """The three-way routing of the _split instances against the restatement as it stood before them: with a delta-light share of 1e-30, q = (1 - s) 1e-30
    is positive and taken = s + q rounds to s, so no random number lies in [s, taken) -- every field of the Result equals, bit for bit, that of the
    same launch without delta lights (the plain restatement with s = 0, the _sky one with s = 0.5). With `delta` and `tree` None the Result is that of
    tables which never had the attributes."""
    import copy
    import delta_light_reference
    world = variant_world
    setup = cases.SETUP["sky_share_0.5" if sky_share else "default"]
    tables = world.apply(setup); world.set_maps(tables, {})
    never = copy.copy(tables)
    for name in ("delta", "tree", "fog_active"):
        delattr(never, name)
    unreached = copy.copy(tables)
    unreached.delta = ref.Delta(delta_light_reference.Table(cases.DELTA_LIGHTS, cases.DELTA_WEIGHTS), 1e-30)
    for launch in (cases.sky_launches(world, setup) if sky_share else cases.small_launches(world)):
        a = ref.evaluate(world, never, launch, world.bsdf_tables)
        for label, other in (("delta and tree None", tables), ("a share no number reaches", unreached)):
            b = ref.evaluate(world, other, launch, world.bsdf_tables)
            assert cases.light_split(other) == (2 if other is unreached else 1 if sky_share else 0)
            for field, value in vars(a).items():
                if other is unreached and (field == "route" or (field == "u_emitter" and not sky_share)):   # (the plain restatement rescales no number: NaN there, u itself here)
                    assert field == "route" or np.array_equal(b.u_emitter, tables.random(ref.DIM_NEE_LIGHT, *launch.paths()[1:4])[:, 0])
                    continue
                x, y = np.asarray(value), np.asarray(getattr(b, field))
                assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s (%s): %s differs" % (launch.name, label, field)
            assert not b.to_delta.any()


# kernel_material_conductor_stream on the MI355X, instances_plain/instances_conductor_merged_1500: the entry furthest from float64's throughput, how far, and
# the launch's worst direction error (printed by test_gpu_material_instances.py)
DEVICE_WORST_ENTRY, DEVICE_WORST_THROUGHPUT, DEVICE_DIRECTION_ERROR = 199, 2.32e-3, 9.3e-6


def _oracle_on_instance_launches(world, mapped_too=False):
    """The oracle's plain shade_material on the entries of the unmapped conductor launches of INSTANCE_CASES, under the plain setup (the continuation ray of a hit does not depend on
    the light variant) against float64: {quantity: (worst error, launch)}."""
    worst = {}
    for compressed in (False, True):
        setup = cases.instance_setup("", compressed)
        tables = world.apply(setup)
        tables.map_ids = None
        for light, mapped, slot, c in cases.INSTANCE_CASES:
            if c != compressed or slot != 3 or (mapped and not mapped_too):
                continue
            for maps, launch in cases.instance_launches(world, light, mapped, slot, compressed):
                name = "%s/%s" % (cases.instance_setup(light, compressed).name, launch.name)
                out = checks.oracle_launch(tables, launch)
                at = checks.check_structure(name, tables, launch, out)
                errors = checks.compare_with_reference(name, tables, launch, out, at, ref.evaluate(world, tables, launch, world.bsdf_tables), None)
                for quantity, (error, _) in errors.items():
                    if error > worst.get(quantity, (0.0, ""))[0]:
                        worst[quantity] = (error, name)
    return worst


def test_instance_throughput_bound_is_four_times_the_worst_case(variant_world):
    """The unmapped conductor rows of the instance launches are further queues of VariantWorld's hits, and on one of them the device's throughput leaves
    BOUNDS["throughput"], which World's launches set: 2.32e-3 against 1.97e-3, kernel_material_conductor_stream, entry 199 of
    instances_plain/instances_conductor_merged_1500 -- a rough conductor's sample 2.3e-3 above the shading plane (omega_o.z), where G2 / G1 and the
    Kulla-Conty term change by about 1 / omega_o.z of every change of the direction. That is asserted here, in float64: the BSDF's value / pdf at the
    sampled direction is the sample's factor (within 1e-4), and moving that direction by DEVICE_DIRECTION_ERROR along the normal -- the device's worst
    direction error in that launch, 9.3e-6, a fortieth of BOUNDS["direction"] -- moves the factor of that entry by more than the 2.32e-3 seen, while the
    launch's median entry moves by less than a hundredth of that. So the reference's throughput is ill-conditioned in the direction there, whoever
    computes it, and the kernel's direction is within its bound. The bound is measured as "variant_throughput" was: the oracle against float64 on the
    entries of every unmapped conductor launch of INSTANCE_CASES under the plain setup (a hit's continuation ray does not depend on the light variant);
    material_checks.MEASURED["instance_throughput"] is this run's maximum, and the device's unmapped conductor rows are held to 4 x it (2.8e-3); every
    other unmapped row keeps BOUNDS, the mapped ones VARIANT_BOUNDS. Every other quantity stays within its bound here too."""
    import bsdf_reference
    world = variant_world
    tables = world.apply(cases.instance_setup(""))
    world.set_maps(tables, {})
    launch = cases.instance_launches(world, "", False, 3, False)[1][1]
    assert launch.name == "instances_conductor_merged_1500"
    r = ref.evaluate(world, tables, launch, world.bsdf_tables)
    e = launch.entries
    slot, real, bounce, sample, submission = launch.paths()
    materials = tables.materials[tables.material_ids[e.mesh]]

    def factor(direction):   # value / pdf of the BSDF's eval towards `direction`: what its sample multiplies the throughput by
        probes = ref._probes(materials, r.normal, e.direction.astype(np.float64), r.entering, real, sample, bounce, to_light=direction, cos_o=(direction * r.normal).sum(axis=1))
        with np.errstate(all="ignore"):
            x, _ = bsdf_reference.evaluate(bsdf_reference.CONDUCTOR, probes, world.bsdf_tables, eval=True)
            return x.value / x.pdf[:, None]
    held = r.continues & r.robust
    at = factor(r.direction)
    assert held[DEVICE_WORST_ENTRY] and np.abs(at[held] / r.sample_factor[held] - 1.0).max() <= 1e-4
    moved = r.direction + DEVICE_DIRECTION_ERROR * r.normal
    moved /= np.linalg.norm(moved, axis=1)[:, None]
    change = np.abs(factor(moved)[held] / at[held] - 1.0).max(axis=1)
    mine = change[np.nonzero(held)[0] == DEVICE_WORST_ENTRY][0]
    height = (r.direction[DEVICE_WORST_ENTRY] * r.normal[DEVICE_WORST_ENTRY]).sum()
    print("entry %d: omega_o.z %.3g; a direction error of %.2g moves its throughput by %.3g (the device is %.3g from float64), the launch's median entry by %.3g" % (
        DEVICE_WORST_ENTRY, height, DEVICE_DIRECTION_ERROR, mine, DEVICE_WORST_THROUGHPUT, np.median(change)))
    assert 1e-3 < height < 3e-3 and mine > DEVICE_WORST_THROUGHPUT and np.median(change) < 0.01 * DEVICE_WORST_THROUGHPUT
    assert DEVICE_DIRECTION_ERROR < checks.BOUNDS["direction"] / 30 and checks.BOUNDS["throughput"] < DEVICE_WORST_THROUGHPUT <= checks.BOUNDS["instance_throughput"]
    worst = _oracle_on_instance_launches(variant_world)
    for quantity, (error, name) in sorted(worst.items()):
        print("%-18s worst %.3g  (%s)  bound %.3g" % (quantity, error, name, checks.BOUNDS[quantity]))
    error, name = worst["throughput"]
    recorded, launch = checks.MEASURED["instance_throughput"]
    assert error <= recorded * 1.0000001 and recorded <= error * 1.06 and launch == name, "instance_throughput: recorded %.3g (%s), the worst case is %.3g (%s)" % (recorded, launch, error, name)
    assert checks.BOUNDS["instance_throughput"] == 4.0 * recorded
    for quantity, (error, name) in worst.items():
        if quantity != "throughput":
            assert error <= checks.BOUNDS[quantity], "%s: the oracle is %.3g from float64 on %s" % (quantity, error, name)
