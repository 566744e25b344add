"""The variants of the material launch on the device, entry by entry: the _sky, _nmap and _sky_nmap instances that rt_launch_material and
rt_launch_material_stream pick through material_kernels_for ([(NMAP * 4 + SKY) * rows + row]) when the sky takes a share of the light samples
(rt_set_sky_sampling) or a material of the slot has a normal map (rt_upload_material_normal_maps), run by rt_shade_rays on the launches of
material_cases.py (VariantWorld) and held to the float64 composition of material_reference.py. The oracle samples no sky and knows no normal
map: float64 is the only reference here, as for the delta lights.

Every launch: check_structure and, up to one workgroup, check_order as they are; compare_with_reference under material_checks.BOUNDS, robust
entries taking float64's outcomes exactly (alive, continues, emits a shadow ray, ALLOW_NEE, medium; a ray to the sky has max_distance +inf
exactly, one to an emitter a finite one, so the route is float64's float32 comparison). A sky entry's written direction is, bit for bit, what
rt_sample_sky_distribution returns for its DIM_NEE_TRIANGLE pair (rt_random_samples), and within test_gpu_sky_sampling.INVERSION_BOUND of the
numpy inversion of the tables read back (rt_read_sky_tables); its origin and illumination are held from that written direction. Entries next
to a threshold, and sky entries further from the inversion (cell borders), are left out and counted: at most NON_ROBUST_CAP of a launch.

Which launch reaches which group of instances (each name with and without _stream):
* kernel_material_{diffuse,plastic}_texels_sky, kernel_material_{dielectric,conductor}_sky: test_sky_instances[sky_share_0.5], bounce 0 and 2
  and merged, every slot; the other shares and settings (0.25, 1, MIS off, no emitters, a 1 x 1 sky, SVGF) on diffuse, conductor and merged plastic;
* kernel_material_{diffuse,plastic}_sky (the rows that can decode compressed blocks): test_sky_instances[sky_share_0.5_bc1];
* the light tables in global memory inside a _sky instance: test_sky_instance_on_global_light_tables;
* kernel_material_{diffuse,plastic}_texels_nmap, kernel_material_{dielectric,conductor}_nmap: test_mapped_instances;
* kernel_material_diffuse_texels_sky_nmap, kernel_material_conductor_sky_nmap: test_sky_mapped_instances.
Bounds: material_checks.BOUNDS throughout, with two numbers of their own that test_material.py measures on the CPU and asserts: the
throughput on the mapped launches (the oracle's error on the same launches with no map in force, "variant_throughput") and the NORMAL frame
of a mapped hit the view guard has moved (a float32 restatement of normal_map_perturb, "mapped_normal"), each x 4.
Identities on one small launch each: the emitters' half under MIS off is the plain reference on the rescaled number over 1 - s; a _sky launch
equals, bit for bit, a _split launch whose delta lights take a share no random number reaches; a merged _sky launch equals per-bounce ones.
Every test prints, per launch, the instance, the sky, emitter and mapped entries held, those left out, and the worst error per quantity."""
import copy
import time

import numpy as np
import pytest

import material_cases as cases
import material_checks as checks
import material_reference as ref
import sky_sampling_reference as sky_ref
from test_gpu_sky_sampling import INVERSION_BOUND, _angle

pytestmark = pytest.mark.gpu

# The mapped launches' throughput: measured on the oracle for these very launches with no map in force (test_material.py), 4 x that.
# (The NORMAL frame of a mapped hit the view guard has moved is held to BOUNDS["mapped_normal"], the float32 restatement's error x 4: run.)
VARIANT_BOUNDS = dict(checks.BOUNDS, throughput=checks.BOUNDS["variant_throughput"])
HDR_SKY = dict(sun=(40, 9), sun_value=300.0)   # sort_cases.World's sky, for the LightsWorld launch


@pytest.fixture(scope="module")
def world(grt, oracle, tmp_path_factory):
    w = cases.VariantWorld(grt, oracle, tmp_path_factory.mktemp("variants"), 0)
    yield w
    w.close()


@pytest.fixture(autouse=True)
def timed(request):
    start = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - start))


instance = cases.instance   # the __global__ entry point material_kernels_for picks for a launch: any of the 96 (material_cases.py)


def device_random(world, dimension, launch):
    """rt_random_samples for every entry of the launch (the generator's numbers as the kernel draws them)."""
    slot, real, bounce, sample, submission = launch.paths()
    out = np.zeros((launch.entries.n, 2), np.float32)
    key = bounce.astype(np.int64) * (1 << 32) + sample.astype(np.int64)
    for k in np.unique(key):
        m = key == k
        out[m] = world.grt.random_samples(world.ctx, dimension, real[m], int(k >> 32), int(k & 0xffffffff))
    return out


def sky_directions(world, name, tables, launch, got, shadow_at, r):
    """The written direction of every shadow entry float64 routes to the sky: bit for bit rt_sample_sky_distribution's for the entry's pair,
    within INVERSION_BOUND of the numpy inversion of the device's own tables (further: a cell-border case, left out). Returns the directions
    (N, 3; NaN elsewhere), rt_sky_pdf's values for them, and the mask of the entries left out."""
    grt, ctx, n = world.grt, world.ctx, launch.entries.n
    slot, real, bounce, sample, submission = launch.paths()
    pair = device_random(world, ref.DIM_NEE_TRIANGLE, launch)
    assert np.array_equal(pair, tables.random(ref.DIM_NEE_TRIANGLE, real, bounce, sample)), "%s: the device draws other numbers than the reference" % name
    mine = r.to_sky & r.alive & r.allow_nee & (shadow_at >= 0)
    index = np.nonzero(mine)[0]
    written = got.shadow_out[shadow_at[index], 3:6].view(np.float32)
    probe = grt.sample_sky_distribution(ctx, pair[index])
    same = (written.view(np.uint32) == probe[:, :3].view(np.uint32)).all(axis=1)
    assert same.all(), "%s: entry %d: the shadow ray's direction %s is not rt_sample_sky_distribution's %s for its pair %s" % (
        name, index[np.nonzero(~same)[0][0]] if (~same).any() else -1, written[~same][:1].tolist(), probe[~same][:1, :3].tolist(), pair[index][~same][:1].tolist())
    t = grt.read_sky_tables(ctx)
    row, fy, col, fx = sky_ref.invert_tables(t["marginal"], t["conditional"], pair[index])
    want = sky_ref.direction_of(t["height"], t["width"], row, fy, col, fx)
    apart = _angle(written.astype(np.float64), want)
    directions = np.full((n, 3), np.nan); directions[index] = written
    pdfs = np.full(n, np.nan); pdfs[index] = grt.sky_pdf(ctx, written)
    far = np.zeros(n, bool); far[index] = apart > INVERSION_BOUND
    return directions, pdfs, far, float(apart[apart <= INVERSION_BOUND].max(initial=0.0))


def run(world, setup_name, tables, launch, sides=True, bounds=checks.BOUNDS, sample=None):
    """One launch of any instance: check_structure, check_order up to one workgroup, compare_with_reference on every quantity with robust entries taking
    float64's outcomes exactly, the values under `bounds`. sides: every route in force holds more than 100 robust shadow entries. sample: the entries
    whose values are compared (a large queue: structure on all of it)."""
    name = "%s/%s" % (setup_name, launch.name)
    kernel = instance(world, tables, launch)
    n = launch.entries.n
    got = checks.device_launch(world.grt, world.ctx, launch, capacity=n + 37)
    got_at = checks.check_structure(name, tables, launch, got)
    if n <= cases.BLOCK:
        checks.check_order(name, launch, got, *got_at)
    if sample is not None:
        launch = launch.sub(sample)
        got_at = (got_at[0][sample], got_at[1][sample])
        n = launch.entries.n
    r = ref.evaluate(world, tables, launch, world.bsdf_tables)   # the reference's own inversion: the routes
    far, inversion = np.zeros(n, bool), 0.0
    if r.to_sky.any():
        directions, pdfs, far, inversion = sky_directions(world, name, tables, launch, got, got_at[1], r)
        r = ref.evaluate(world, tables, launch, world.bsdf_tables, sky_directions=directions, sky_pdfs=pdfs)
    errors = checks.compare_with_reference(name, tables, launch, got, got_at, r, None)   # (outcomes asserted; the values measured, printed, then held)
    left_out = int((r.near | far).sum())
    held = r.robust & ~far & (got_at[1] >= 0)
    routes = [int((held & (r.route == k)).sum()) for k in range(4)]
    sky, emitter, mapped = routes[ref.ROUTE_SKY], routes[ref.ROUTE_POWER] + routes[ref.ROUTE_TREE], int((r.mapped & r.robust).sum())
    print("%-50s %-46s %5d entries, held: %4d sky, %4d delta, %4d emitter (%s) shadow entries, %4d mapped hits; %3d left out; inversion %.2g " % (
        name, kernel, n, sky, routes[ref.ROUTE_DELTA], emitter, "tree" if routes[ref.ROUTE_TREE] else "power", mapped, left_out, inversion) + " ".join("%s %.2g" % (q, v[0]) for q, v in errors.items()))
    e, bounce = launch.entries, launch.paths()[2]
    if r.mapped.any() and "normal" in errors:
        # the NORMAL frame by kind of hit: under the existing bound, but for a mapped normal the view guard has moved -- normalising the guard's
        # sum divides the frame's error by its length, down to eps: that one under the float32 restatement's error x 4 (MEASURED["mapped_normal"])
        del errors["normal"]
        index = np.nonzero(r.robust & (bounce == 0) & r.alive)[0]
        apart = np.abs(got.aov[checks.NORMAL][e.pixel[index], :3].view(np.float32) - r.normal[index]).max(axis=1)
        moved = r.mapped[index] & r.map_guarded[index]
        for label, pick, bound in (("an unmapped", ~r.mapped[index], checks.BOUNDS["normal"]), ("a mapped", r.mapped[index] & ~moved, checks.BOUNDS["normal"]),
                                   ("a mapped and guarded", moved, checks.BOUNDS["mapped_normal"])):
            worst = float(apart[pick].max(initial=0.0))
            print("%-50s   NORMAL frame of %s hit: %.3g from float64's (bound %.3g, %d hits)" % (name, label, worst, bound, pick.sum()))
            assert worst <= bound, "%s: the NORMAL frame of %s hit is %.3g from float64's, the bound is %.3g" % (name, label, worst, bound)
    for quantity, (error, i) in errors.items():
        assert error <= bounds[quantity], "%s: entry %d (pixel %d, bounce %d, to %s%s): %s is %.3g from float64's, the bound is %.3g" % (
            name, i, e.pixel[i], bounce[i], ref.ROUTE_NAMES[r.route[i]], ", mapped" if r.mapped[i] else "", quantity, error, bounds[quantity])
    assert left_out <= checks.NON_ROBUST_CAP * n, "%s: %d of %d entries left out" % (name, left_out, n)
    if sides:
        for route, count in enumerate(routes):
            assert count > 100 or not ref.route_in_force(tables, route), "%s: %d %s entries held" % (name, count, ref.ROUTE_NAMES[route])
    return got, got_at, r


@pytest.mark.parametrize("setup", cases.SKY_SETUPS, ids=[s.name for s in cases.SKY_SETUPS])
def test_sky_instances(world, setup):
    """The _sky instances under every setup with a sky share; under sky_share_0.5 all four slots at bounce 0 and 2 and merged, and the queue
    lengths 1, 64 and 257 for order and structure."""
    tables = world.apply(setup)
    for launch in cases.sky_launches(world, setup):
        got, got_at, r = run(world, setup.name, tables, launch)
        if tables.sky_share >= 1.0:
            assert np.isposinf(got.shadow_out[:got.counters[1], 6].view(np.float32)).all(), "%s: a share of 1 (or no emitters) sends every light sample to the sky" % launch.name
    if setup.name == "sky_share_0.5":
        for launch in cases.sky_length_launches(world):
            run(world, setup.name, tables, launch, sides=False)


def test_sky_instance_on_global_light_tables(grt, oracle, tmp_path):
    """meshes65 (one light mesh more than the shade kernels' LDS copy holds) with half the light samples to the sky: nee_pick_light searches
    global memory inside a _sky instance."""
    case = [c for c in __import__("nee_cases").GPU_CASES if c.name == "meshes65"][0]
    w = cases.LightsWorld(grt, oracle, case, tmp_path, 0)
    try:
        tables = cases.lights_world_sky(w, 0.5, np.ascontiguousarray(sky_ref.sun_sky(64, 32, **HDR_SKY)))
        run(w, "meshes65_sky_share_0.5", tables, cases.sky_lights_launch(w))
    finally:
        w.lib.rt_set_sky_sampling(w.ctx, 0.0)
        w.close()


def test_emitter_half_without_mis_is_the_plain_sample_rescaled(world):
    """sky_share_0.5_mis_off: an entry that goes to the emitters carries the plain launch's illumination for the rescaled number
    u' = (u - s) / (1 - s), times 1 / (1 - s) -- the reference of the plain instance (no share) on u', not the sky-aware one."""
    setup = cases.SETUP["sky_share_0.5_mis_off"]
    tables = world.apply(setup)
    launch = cases.per_bounce(world, "rescaled", 0, 1500, 1, seed=4600)
    name = setup.name + "/" + launch.name
    got = checks.device_launch(world.grt, world.ctx, launch, capacity=launch.entries.n + 37)
    trace_at, shadow_at = checks.check_structure(name, tables, launch, got)
    routed = ref.evaluate(world, tables, launch, world.bsdf_tables)
    plain = copy.copy(tables)
    plain.sky_share, plain.sky_tables = 0.0, None
    draw = tables.random

    def random(dimension, *key):
        v = draw(dimension, *key).copy()
        if dimension == ref.DIM_NEE_LIGHT:
            v[:, 0] = routed.u_emitter
        return v
    plain.random = random
    r = ref.evaluate(world, plain, launch, world.bsdf_tables)
    mine = ~routed.to_sky & r.robust & routed.robust & r.alive & r.allow_nee
    assert not (mine & ((shadow_at >= 0) != r.has_shadow)).any(), name
    index = np.nonzero(mine & (shadow_at >= 0) & ~r.textured)[0]
    f = got.shadow_out[shadow_at[index]].view(np.float32).astype(np.float64)
    s = float(np.float32(tables.sky_share))
    error = checks._per_channel(f[:, 7:10], r.illumination[index] / (1.0 - s)).max(initial=0)
    distance = checks._relative(f[:, 6], r.shadow_distance[index], 1e-30).max(initial=0)
    print("%-50s %-46s %5d entries, %4d emitter entries held: illumination within %.2g of the plain sample / (1 - s), distance %.2g" % (
        name, instance(world, tables, launch), launch.entries.n, index.size, error, distance))
    assert index.size > 100 and error <= checks.BOUNDS["illumination"] and distance <= checks.BOUNDS["shadow_distance"], (name, index.size, error, distance)


def _matched_rows(launch, out, name):
    """Per input entry its two records (NaN-free uint32 words; a row of the sentinel where it has none)."""
    trace_at, shadow_at = checks.match(launch, out, name)
    trace = np.where((trace_at >= 0)[:, None], out.trace_out[np.maximum(trace_at, 0)], np.uint32(cases.SENTINEL))
    shadow = np.where((shadow_at >= 0)[:, None], out.shadow_out[np.maximum(shadow_at, 0)], np.uint32(cases.SENTINEL))
    return trace, shadow


def test_sky_instance_equals_the_split_instance_no_sample_reaches(world):
    """rt_upload_delta_lights accepts any share in (0, 1]: with 1e-30 the delta lights' share q = (1 - s) x 1e-30 is positive -- the launchers
    take the _split instances -- and taken = s + q rounds to s, so no random number lies in [s, taken): every entry goes where the _sky
    instance sends it, through next_event_estimation<2>'s own copy of the two branches. All records and frames agree bit for bit."""
    tables = world.apply(cases.SETUP["sky_share_0.5"])
    grt, ctx = world.grt, world.ctx
    lights = np.zeros((1, 12), np.float32); lights[0, 2] = 5.0; lights[0, 7:10] = 10.0   # a point light no entry samples
    for slot in (1, 3):
        launch = cases.merged(world, "unreached", slot, 1500, seed=4610 + slot) if slot == 1 else cases.per_bounce(world, "unreached", slot, 1500, 1, seed=4610 + slot)
        sky = checks.device_launch(grt, ctx, launch, capacity=launch.entries.n + 37)
        try:
            assert grt.upload_delta_lights(ctx, grt.delta_light_records(lights, np.ones(1, np.float32)), 1e-30) == 0, world.lib.rt_last_error(ctx)
            split = checks.device_launch(grt, ctx, launch, capacity=launch.entries.n + 37)
        finally:
            assert grt.upload_delta_lights(ctx, None) == 0
        assert np.array_equal(sky.counters, split.counters), launch.name
        for a, b, what in zip(_matched_rows(launch, sky, launch.name), _matched_rows(launch, split, launch.name + " (_split)"), ("continuation", "shadow")):
            differ = (a != b).any(axis=1)
            assert not differ.any(), "%s: entry %d: the %s record differs between the _sky and the _split instance" % (launch.name, np.nonzero(differ)[0][0], what)
        for field in ("aov", "gnd", "gid", "gsp"):
            assert np.array_equal(getattr(sky, field), getattr(split, field)), "%s: %s differs between the _sky and the _split instance" % (launch.name, field)
        to_sky = int(np.isposinf(sky.shadow_out[:sky.counters[1], 6].view(np.float32)).sum())
        assert to_sky > 100 and sky.counters[1] - to_sky > 100
        print("%-50s %-46s %5d entries, %4d sky and %4d emitter shadow entries, all bit for bit with the _split instance" % (
            "sky_share_0.5/" + launch.name, instance(world, tables, launch), launch.entries.n, to_sky, sky.counters[1] - to_sky))


def test_merged_sky_launch_equals_per_bounce_launches(world):
    """test_gpu_material.py's identity for the _sky instances: each entry of a merged launch against the per-bounce instance given the same
    bounce, virtual pixel and sample index -- every output bit but RT_SHADOW_FLAG_BOUNCE_0."""
    tables = world.apply(cases.SETUP["sky_share_0.5_svgf"])
    for slot in (0, 2):
        merged = cases.merged(world, "sky_instances", slot, 2500, seed=4620 + slot)
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
        to_sky = int(np.isposinf(got.shadow_out[:got.counters[1], 6].view(np.float32)).sum())
        assert to_sky > 100 and got.counters[1] - to_sky > 100
        print("%-50s %-46s %5d entries, %4d sky and %4d emitter shadow entries, all bit for bit against the per-bounce instance" % (
            "sky_share_0.5_svgf/" + name, instance(world, tables, merged), merged.entries.n, to_sky, got.counters[1] - to_sky))


def _unmapped_equal_plain(name, launch, got, got_at, before, pick, what):
    """The entries of `pick` in every output bit against the plain instance's launch `before`."""
    before_at = checks.match(launch, before, name + " (plain)")
    e = launch.entries
    for queue, rows_a, rows_b in ((0, got.trace_out, before.trace_out), (1, got.shadow_out, before.shadow_out)):
        a_at, b_at = got_at[queue][pick], before_at[queue][pick]
        assert np.array_equal(a_at >= 0, b_at >= 0), "%s: %s is in one instance's queue only" % (name, what)
        live = a_at >= 0
        assert np.array_equal(rows_a[a_at[live]], rows_b[b_at[live]]), "%s: queue %d: %s differs from the plain instance" % (name, queue, what)
    px = e.pixel[pick]
    for label, a, b in (("aov", got.aov.transpose(1, 0, 2), before.aov.transpose(1, 0, 2)), ("gnd", got.gnd, before.gnd), ("gid", got.gid, before.gid), ("gsp", got.gsp, before.gsp)):
        assert np.array_equal(a[px], b[px]), "%s: %s of %s differs from the plain instance" % (name, label, what)
    return before_at


def _mapped_checks(world, setup_name, tables, maps, launch, bounds=checks.BOUNDS):
    """One launch with `maps` in force against the same launch without (the plain, or the _sky, instance) and against float64."""
    import normal_map_reference as nm
    from sort_reference import _oct_encode
    name = "%s/%s" % (setup_name, launch.name)
    e, bounce = launch.entries, launch.paths()[2]
    world.set_maps(tables, {})
    before = checks.device_launch(world.grt, world.ctx, launch, capacity=e.n + 37)
    world.set_maps(tables, maps)
    degenerate = launch.name.startswith("nmap_degenerate")
    got, got_at, r = run(world, setup_name, tables, launch, sides=False, bounds=bounds)
    assert degenerate or launch.name.startswith("nmap_mirrored") or ((r.mapped & r.robust).sum() > 100 and (~r.mapped & r.robust).sum() > 100), name
    # a hit whose material has no map, and a mapped hit whose triangle has no texture coordinates, run the plain instance's arithmetic
    before_at = _unmapped_equal_plain(name, launch, got, got_at, before, ~r.mapped | r.map_fallback, "an unmapped hit (or one that fell back)")
    if degenerate:
        assert r.mapped.all() and r.map_fallback.all()
    # the ray cone never sees the map: cone words equal the plain instance's wherever both continue
    both = (got_at[0] >= 0) & (before_at[0] >= 0)
    assert both.sum() > 100 and np.array_equal(got.trace_out[got_at[0][both], 16:18], before.trace_out[before_at[0][both], 16:18]), "%s: a cone word of a mapped hit differs from the plain instance's" % name
    moved_count = 0
    if (bounce == 0).any() and tables.config["enable_svgf"] and not degenerate:   # (a hit that fell back has the plain instance's normal, held above)
        sentinel = np.uint32(cases.SENTINEL)
        first = np.nonzero(r.mapped & ~r.map_fallback & r.robust & (bounce == 0) & (got.aov[checks.NORMAL][e.pixel] != sentinel).all(axis=1) & (before.aov[checks.NORMAL][e.pixel] != sentinel).all(axis=1))[0]
        px = e.pixel[first]
        shading = got.aov[checks.NORMAL][px, :3].view(np.float32).astype(np.float64)
        interpolated = before.aov[checks.NORMAL][px, :3].view(np.float32).astype(np.float64)
        # ONE normal: the g-buffer's octahedral normal encodes the NORMAL frame's (a handful of float32 operations on numbers below 1)
        ox, oy = _oct_encode(shading)
        encoded = got.gnd[px, :2].view(np.float32).astype(np.float64)
        assert first.size > 100 and (np.maximum(np.abs(encoded[:, 0] - ox), np.abs(encoded[:, 1] - oy)) <= 1e-6).all(), "%s: the g-buffer's normal is not the NORMAL frame's" % name
        angle = _angle(shading, interpolated)
        texel = [c for c in maps.values()][0]
        if texel == cases.FLAT:
            # what 8 bits leave of "unperturbed": the angle constant_map_normal's decoded vector makes with its quad's normal, and float32's share
            decoded = nm.constant_map_normal(texel).astype(np.float64)
            unguarded = (-e.direction[first].astype(np.float64) * interpolated).sum(axis=1) > 0.05
            bound = np.arccos(decoded[1]) + 4 * checks.BOUNDS["normal"]
            assert unguarded.sum() > 100 and (angle[unguarded] <= bound).all(), "%s: the (128, 128, 255) map moves a normal by %.3g rad, 8 bits leave %.3g" % (name, angle[unguarded].max(), bound)
        else:
            assert (angle > 1e-2).sum() > 0.9 * first.size, "%s: the map moves %d of %d normals" % (name, (angle > 1e-2).sum(), first.size)
        moved_count = first.size
    return moved_count


def test_mapped_instances(world):
    """The _nmap instances of all four slots under SVGF (SKY == 0): the tilt map (200, 90, 180) on the transformed dielectric and conductor
    instances' materials and on the untextured diffuse and plastic materials (bounce 0, 2, merged), the maps (128, 128, 255) and (128, 128, 0)
    on the conductor slot, mirrored triangles (uv_det < 0) and triangles without texture coordinates (uv_det == 0) on the conductor slot.
    Mapped hits are held to float64 with the mapped normal in the BSDF frame, next-event estimation, the NORMAL frame and the g-buffer, and the
    interpolated one in the ray cone; unmapped hits and fallen-back ones equal the plain instance in every bit."""
    tables = world.apply(cases.SETUP["svgf_on"])
    try:
        for maps, launch in cases.map_launches(world):
            launch._reference = None
            _mapped_checks(world, "svgf_on", tables, maps, launch, bounds=VARIANT_BOUNDS)
    finally:
        world.set_maps(tables, {})


def test_sky_mapped_instances(world):
    """The _sky_nmap instances of the diffuse and the conductor slot (sky_share_0.5, the tilt map), bounce 1 per bounce and merged: the sky's and
    the emitters' shadow entries of mapped hits shade with the mapped normal; unmapped hits equal the _sky instance in every bit."""
    tables = world.apply(cases.SETUP["sky_share_0.5"])
    try:
        for maps, launch in cases.sky_map_launches(world):
            _mapped_checks(world, "sky_share_0.5", tables, maps, launch)
            r = ref.evaluate(world, tables, launch, world.bsdf_tables)
            both_sides = r.mapped & r.robust & r.has_shadow
            assert (both_sides & r.to_sky).sum() > 50 and (both_sides & ~r.to_sky).sum() > 50, launch.name
    finally:
        world.set_maps(tables, {})
