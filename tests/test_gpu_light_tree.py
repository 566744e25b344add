"""The light tree on the device against its restatements (light_tree_reference.py), on the scenes of light_tree_cases.py.

Tree, through rt_read_light_tree, for every case: each leaf id occurs once and padding leaves are empty; the sorted order equals the restatement's; every node's box and
Phi equal the float32 restatement bit for bit; leaf A and Phi lie within the derived bounds of the float64 values; the inverse tables invert.
Pmf, for every case on the grid of light_tree_cases.grid: the pmfs of all leaves sum to 1 within 1.01 * depth * 2^-24 (+ N * 2^-125); the device pmf equals the float32
restatement bit for bit and lies within pmf_bound of float64; what rt_sample_light_tree reports equals rt_light_tree_pmf of the same leaf bit for bit; leaves without
power are never returned, not at u = 0 and not at the float below 1.
Selection, on the 65- and 257-leaf cases: 2^16 equally spaced u; each leaf's count equals 2^16 pmf within selection_tolerance (2 + the derived drift of the interval's ends).
Refusals: RT_ERROR_INVALID_ARG, a message that names the cause, the state untouched.
Frames (further down, each with its own docstring): the polygon form factor with the tree; tree on against off on the many-light world (means, noise ratio against the
reference's prediction); enable, render, disable under both schedulers; scheduler identity and the _tree_nmap / SVGF / sky variants; a fog volume displaces the tree.
Launches, entry by entry, through rt_shade_rays and rt_sort_rays with the helpers of material_checks.py and sort_checks.py, at their tolerances.
"""
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

import light_tree_cases as cases
import light_tree_reference as ref

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG = -1
F = np.float32


@pytest.fixture(scope="module")
def built(grt):
    """case name -> (ctx, scene as the device holds it, tree read back, float32 restatement), each built once."""
    lib = grt.device_lib()
    cache = {}

    def get(name):
        if name not in cache:
            ctx, s = cases.upload(grt, cases.scene(name), device_tlas=name in cases.DEVICE_TLAS)
            assert grt.set_light_tree(ctx, True) == 0, lib.rt_last_error(ctx)
            assert lib.rt_get_light_tree(ctx) == 1
            got = grt.read_light_tree(ctx, s.transforms.shape[0], s.triangles.shape[0])
            cache[name] = (ctx, s, got, ref.build32(s))
        return cache[name]
    yield get
    for ctx, _, _, _ in cache.values():
        lib.rt_destroy(ctx)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", cases.NAMES)
def test_tree_equals_the_float32_restatement_bit_for_bit(grt, built, name):
    ctx, s, got, want = built(name)
    n, m = want.leaf_count, want.padded
    assert (got.leaf_count, got.padded) == (n, m) and got.nodes.shape == (2 * m - 1, 8)
    # each leaf id occurs exactly once, in the restatement's order; padding leaves are empty
    slots = got.slot_of_leaf
    assert np.array_equal(np.sort(slots), m - 1 + np.arange(n)), "a leaf id is missing or doubled"
    order = np.empty(n, np.int32); order[slots - (m - 1)] = np.arange(n)
    assert np.array_equal(order, want.order), "the sorted order differs from the restatement's"
    padding = got.nodes[m - 1 + n:]
    assert (padding[:, 3] == 0).all() and (padding[:, 0:3] > padding[:, 4:7]).all()
    assert (got.nodes[:, 7] == 0).all(), "the pad word is not free"
    # every node: box and Phi bit for bit
    bad = np.nonzero((bits(got.nodes) != bits(want.nodes)).any(1))[0]
    assert bad.size == 0, "%d nodes differ, first %d: %s vs %s" % (bad.size, bad[0], got.nodes[bad[0]].tolist(), want.nodes[bad[0]].tolist())
    # leaf records: ids exact, A and Phi bit for bit against float32 and within the derived bounds of float64
    lv = want.leaves
    assert np.array_equal(got.leaf_entry, lv.entry) and np.array_equal(got.leaf_triangle, lv.triangle)
    assert np.array_equal(bits(got.leaf_area), bits(lv.area)) and np.array_equal(bits(got.leaf_power), bits(lv.power))
    area, power, area_bound, power_bound = ref.leaves64(s)
    print("%s: N %d M %d, worst |A - A64| / bound %.3g, |Phi - Phi64| / bound %.3g" % (name, n, m, np.max(np.abs(got.leaf_area - area) / np.maximum(area_bound, 1e-300)), np.max(np.abs(got.leaf_power - power) / np.maximum(power_bound, 1e-300))))
    assert (np.abs(got.leaf_area - area) <= area_bound).all() and (np.abs(got.leaf_power - power) <= power_bound).all()
    # the inverse tables invert: (row, triangle) of every leaf leads back to its id (the lowest id where one triangle of one instance is named twice)
    entry_of_mesh, place_of_triangle = got.entry_of_mesh, got.place_of_triangle
    entry, place, tri, rows, base = s.leaf_table()
    for k in range(n):
        e = entry_of_mesh[rows[k]]; pl = place_of_triangle[tri[k]]
        assert e >= 0 and s.spans[e, 0] <= pl <= s.spans[e, 1]
        assert (rows[base[e]], s.triangle_indices[pl]) == (rows[k], tri[k])
        if e == entry[k] and pl == place[k]:
            assert base[e] + (pl - s.spans[e, 0]) == k
    lit = np.zeros(s.transforms.shape[0], bool); lit[rows] = True
    assert (entry_of_mesh[~lit] == -1).all()


@pytest.mark.parametrize("name", cases.NAMES)
def test_pmf_sums_to_one_and_matches_both_restatements(grt, built, name):
    ctx, s, got, want = built(name)
    n = want.leaf_count
    ids = np.arange(n, dtype=np.int32)
    tree = ref.tree_from_nodes(got.nodes, n, got.slot_of_leaf)
    worst_sum = worst_64 = worst_rho = 0.0
    for point in cases.grid(want, want.leaves):
        pts = np.broadcast_to(point, (n, 3))
        pmf = grt.light_tree_pmf(ctx, ids, pts)
        worst_sum = max(worst_sum, abs(float(pmf.astype(np.float64).sum()) - 1.0))
        assert abs(float(pmf.astype(np.float64).sum()) - 1.0) <= ref.sum_bound(want), (name, point.tolist(), float(pmf.astype(np.float64).sum()))
        assert np.array_equal(bits(pmf), bits(ref.pmf32(tree, pts, got.slot_of_leaf))), (name, point.tolist())
        p64, bound, rho = ref.pmf64(tree, pts, got.slot_of_leaf)
        assert rho < 0.25, "the grid point makes the first-order bound meaningless"
        worst_64 = max(worst_64, float(np.max(np.abs(pmf - p64) / bound))); worst_rho = max(worst_rho, rho)
        assert (np.abs(pmf - p64) <= bound).all(), (name, point.tolist())
        assert (pmf[want.leaves.power == 0] == 0).all()
    print("%s: worst |sum - 1| %.3g (bound %.3g), |pmf - pmf64| / bound %.3g, rho %.3g" % (name, worst_sum, ref.sum_bound(want), worst_64, worst_rho))


@pytest.mark.parametrize("name", cases.NAMES)
def test_sample_reports_the_pmf_of_its_leaf_and_never_a_leaf_without_power(grt, built, name):
    ctx, s, got, want = built(name)
    rng = np.random.default_rng(9)
    grid = cases.grid(want, want.leaves)
    edge = np.array([0.0, ref.ONE_BELOW_ONE, 0.5, 2.0 ** -24], F)
    u = np.concatenate([np.repeat(edge, edge.size), np.minimum(rng.random(2000, F), ref.ONE_BELOW_ONE)])
    u2 = np.concatenate([np.tile(edge, edge.size), np.minimum(rng.random(2000, F), ref.ONE_BELOW_ONE)])
    tree = ref.tree_from_nodes(got.nodes, want.leaf_count, got.slot_of_leaf)
    for point in grid:
        pts = np.broadcast_to(point, (u.size, 3))
        leaf, slot, pmf = grt.sample_light_tree(ctx, u, u2, pts)
        assert (leaf >= 0).all() and (leaf < want.leaf_count).all() and np.array_equal(got.slot_of_leaf[leaf], slot)
        assert (want.leaves.power[leaf] > 0).all(), "a leaf without power was returned"
        assert (pmf > 0).all()
        assert np.array_equal(bits(pmf), bits(grt.light_tree_pmf(ctx, leaf, pts))), "the sample's pmf is not rt_light_tree_pmf's of the same leaf"
        slot32, pmf32 = ref.sample32(tree, pts, u, u2)
        assert np.array_equal(slot32, slot) and np.array_equal(bits(pmf32), bits(pmf)), "the descent differs from its float32 restatement"


@pytest.mark.parametrize("name", ["n65", "n257"])
def test_selection_counts_follow_the_pmf(grt, built, name):
    ctx, s, got, want = built(name)
    n = want.leaf_count
    u = (np.arange(1 << 16) / 65536.0).astype(F)
    tolerance = ref.selection_tolerance(want)
    for point in cases.grid(want, want.leaves)[[0, 3, 4, 6]]:
        leaf, _, _ = grt.sample_light_tree(ctx, u, F(0.5), np.broadcast_to(point, (u.size, 3)))
        counts = np.bincount(leaf, minlength=n)
        pmf = grt.light_tree_pmf(ctx, np.arange(n, dtype=np.int32), np.broadcast_to(point, (n, 3))).astype(np.float64)
        worst = float(np.max(np.abs(counts - 65536.0 * pmf)))
        print("%s at %s: worst |count - 2^16 pmf| %.3f (tolerance %.3f)" % (name, point.tolist(), worst, tolerance))
        assert worst <= tolerance


def test_refusals_leave_the_state_untouched(grt, built):
    lib = grt.device_lib()
    ctx, s, got, want = built("n64")
    n, m = c_int(), c_int()
    nodes = np.zeros((2 * want.padded - 1, 8), F); leaves = np.zeros((want.leaf_count, 4), np.uint32); slots = np.zeros(want.leaf_count, np.int32)

    def refused(status, word):
        message = lib.rt_last_error(ctx).decode()
        assert status == RT_ERROR_INVALID_ARG and word in message, (status, message)

    refused(lib.rt_read_light_tree(ctx, None, byref(m), None, 0, None, None, 0, None, 0, None, 0), "NULL")
    refused(lib.rt_read_light_tree(ctx, byref(n), None, None, 0, None, None, 0, None, 0, None, 0), "NULL")
    refused(lib.rt_read_light_tree(ctx, byref(n), byref(m), nodes.ctypes.data, nodes.shape[0] - 1, None, None, 0, None, 0, None, 0), "nodes")
    refused(lib.rt_read_light_tree(ctx, byref(n), byref(m), None, 0, leaves.ctypes.data, None, want.leaf_count - 1, None, 0, None, 0), "leaves")
    refused(lib.rt_read_light_tree(ctx, byref(n), byref(m), None, 0, None, slots.ctypes.data, 0, None, 0, None, 0), "leaves")
    refused(lib.rt_read_light_tree(ctx, byref(n), byref(m), None, 0, None, None, 0, slots.ctypes.data, 1, None, 0), "instances")
    refused(lib.rt_read_light_tree(ctx, byref(n), byref(m), None, 0, None, None, 0, None, 0, slots.ctypes.data, 1), "triangles")
    refused(lib.rt_set_light_tree(ctx, 2), "0 or 1")
    out = np.zeros(4, F); probe = np.array([0.5, 0.5, 0, 0, 0], F)
    refused(lib.rt_sample_light_tree(ctx, None, 1, out.ctypes.data), "NULL")
    refused(lib.rt_light_tree_pmf(ctx, probe.ctypes.data, 1, None), "NULL")
    for bad, word in ((np.array([1.0, 0.5, 0, 0, 0], F), "outside [0, 1)"), (np.array([0.5, -0.1, 0, 0, 0], F), "outside [0, 1)"), (np.array([0.5, 0.5, np.inf, 0, 0], F), "not finite")):
        refused(lib.rt_sample_light_tree(ctx, bad.ctypes.data, 1, out.ctypes.data), word)
    bad = np.zeros(4, F); bad.view(np.int32)[0] = want.leaf_count
    refused(lib.rt_light_tree_pmf(ctx, bad.ctypes.data, 1, out.ctypes.data), "outside [0, %d)" % want.leaf_count)
    # tables that would make more leaves than the tree may hold: refused by the upload while the tree is on, and the tables before stay in force
    entries, span = 2048, 2049   # 2048 entries over one span of 2049 triangles: 2^22 + 2048 leaves from small tables
    assert entries * span > grt.MAX_LIGHT_TREE_LEAVES
    big = (np.zeros(span, np.int32), np.ones(span, F), np.ones(entries, F), np.tile(np.array([[0, span - 1]], np.int32), (entries, 1)), np.zeros(entries, np.int32), 1.0)
    refused(grt.upload_lights(ctx, *big), "RT_MAX_LIGHT_TREE_LEAVES")
    again = grt.read_light_tree(ctx)
    assert (again.leaf_count, again.padded) == (want.leaf_count, want.padded) and np.array_equal(bits(again.nodes), bits(got.nodes)) and lib.rt_get_light_tree(ctx) == 1

    # a context of its own: probes before a tree exists; enabling over such tables
    other = c_void_p()
    assert lib.rt_create(0, byref(other)) == 0
    try:
        for call in (lambda: lib.rt_sample_light_tree(other, probe.ctypes.data, 1, out.ctypes.data), lambda: lib.rt_light_tree_pmf(other, np.zeros(4, F).ctypes.data, 1, out.ctypes.data)):
            status = call(); message = lib.rt_last_error(other).decode()
            assert status == RT_ERROR_INVALID_ARG and "no light tree exists" in message, (status, message)
        assert lib.rt_read_light_tree(other, byref(n), byref(m), None, 0, None, None, 0, None, 0, None, 0) == 0 and (n.value, m.value) == (0, 0)
        assert grt.upload_lights(other, *big) == 0, lib.rt_last_error(other)   # (the tree is off: the tables themselves are valid)
        status = grt.set_light_tree(other, True); message = lib.rt_last_error(other).decode()
        assert status == RT_ERROR_INVALID_ARG and "RT_MAX_LIGHT_TREE_LEAVES" in message and lib.rt_get_light_tree(other) == 0, (status, message)
        # no emitters: enabled, nothing built, the probes still refuse
        assert lib.rt_upload_lights(other, None, None, 0, None, None, None, 0, 0.0) == 0
        assert grt.set_light_tree(other, True) == 0 and lib.rt_get_light_tree(other) == 1
        assert grt.read_light_tree(other).padded == 0
        assert lib.rt_sample_light_tree(other, probe.ctypes.data, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG
    finally:
        lib.rt_destroy(other)


# ---- frames ----------------------------------------------------------------------------------------------------------------------------

BLACK = np.zeros((1, 1, 4), F)


class Rendering:
    """A scene file on device 0 through the host classes; the frames through rt_render_samples."""

    def __init__(self, grt, path, w, h, config, scheduler="merged", black_sky=True):
        self.grt, self.lib, self.w, self.h = grt, grt.device_lib(), w, h
        grt.config_reset(); grt.config_set(**config)
        self.scene = grt.Scene(path)
        grt.config_set(**config)
        self.pt = grt.Pathtracer(self.scene, w, h, device=0)
        self.pt.update()
        if black_sky:
            assert self.lib.rt_set_sky(self.pt.ctx, BLACK.ctypes.data, 1, 1, 1.0) == 0
        grt.set_scheduler(self.pt.ctx, scheduler)

    def render(self, samples, first=0, batch=16):
        for s in range(first, first + samples, batch):
            assert self.lib.rt_render_samples(self.pt.ctx, s, min(batch, first + samples - s)) == 0, self.lib.rt_last_error(self.pt.ctx)
        return self.pt.read_framebuffer()[:, :self.w].copy()

    def close(self):
        self.pt.close(); self.scene.close(); self.grt.config_reset()


def _rectangle_form_factor(x0, x1, z0, z1, h):
    """Form factor from a horizontal rectangle [x0, x1] x [z0, z1] at height h to the point below the origin (tests/test_oracle.py)."""
    def corner(x, z):
        a, b = np.sqrt(h * h + x * x), np.sqrt(h * h + z * z)
        return (x / a * np.arctan(z / a) + z / b * np.arctan(x / b)) / (2.0 * np.pi)
    return corner(x1, z1) - corner(x0, z1) - corner(x1, z0) + corner(x0, z0)


def test_frame_with_the_tree_lies_inside_the_closed_form(grt, tmp_path):
    """A white diffuse floor seen from straight above through a 2-degree lens, three unoccluded emissive quads of unequal radiance at unequal distances, direct light
    only (num_bounces = 2, a black sky): the mean of the 12 x 12 pixels is sum L_i F_i, F the form factor of a rectangle. Margin: 4 standard errors of the frame's mean,
    from the per-pixel Welford moments of rt_set_noise_estimate (the pixels are independent), plus 2e-3 relative for the footprint (the 12 x 12 pixels cover a square of
    0.017 on the floor, over which the irradiance of lights at least 0.8 away varies by less than 0.017 / 0.8 x 10 %)."""
    (tmp_path / "quad.obj").write_text("v -1 0 -1\nv 1 0 -1\nv 1 0 1\nv -1 0 1\nf 1 2 3\nf 1 3 4\n")
    (tmp_path / "s.xml").write_text(
        '<scene version="0.5.0"><integrator type="path"><integer name="maxDepth" value="2"/></integrator>'
        '<sensor type="perspective"><float name="fov" value="2"/><transform name="toWorld"><lookat origin="0.001, 0.5, 0" target="0, 0, 0" up="0, 0, 1"/></transform></sensor>'
        '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><scale value="20"/></transform><bsdf type="diffuse"><rgb name="reflectance" value="1, 1, 1"/></bsdf></shape>'
        '<shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="90"/><scale value="0.5"/><translate y="1"/></transform><emitter type="area"><rgb name="radiance" value="1, 1, 1"/></emitter></shape>'
        '<shape type="obj"><string name="filename" value="quad.obj"/><transform name="toWorld"><scale value="0.5"/><translate x="1.5" y="0.8" z="0.25"/></transform>'
        '<emitter type="area"><rgb name="radiance" value="3, 3, 3"/></emitter></shape>'
        '<shape type="obj"><string name="filename" value="quad.obj"/><transform name="toWorld"><scale value="0.5"/><translate x="-4.5" y="3" z="-2.75"/></transform>'
        '<emitter type="area"><rgb name="radiance" value="40, 40, 40"/></emitter></shape></scene>')
    analytic = (1.0 * _rectangle_form_factor(-0.5, 0.5, -0.5, 0.5, 1.0) + 3.0 * _rectangle_form_factor(1.0, 2.0, -0.25, 0.75, 0.8)
                + 40.0 * _rectangle_form_factor(-5.0, -4.0, -3.25, -2.25, 3.0))
    r = Rendering(grt, str(tmp_path / "s.xml"), 12, 12, dict(num_bounces=2, enable_russian_roulette=0, reconstruction_filter=0, light_tree=1))
    try:
        assert r.lib.rt_get_light_tree(r.pt.ctx) == 1 and grt.read_light_tree(r.pt.ctx).leaf_count == 6
        grt.set_noise_estimate(r.pt.ctx, True)
        samples = 256
        frame = r.render(samples + 1).astype(np.float64)[..., 0]
        moments = grt.read_noise_moments(r.pt.ctx, 12, r.pt.pitch)[:, :12].astype(np.float64)
        w = moments[..., 3]
        assert (w >= samples - 1).all()
        error = np.sqrt((moments[..., 0] / (w * (w - 1))).sum()) / frame.size
        mean = frame.mean()
        print("closed form %.6f, mean with the tree %.6f, standard error %.2e: %.2f standard errors" % (analytic, mean, error, (mean - analytic) / error))
        assert abs(mean - analytic) <= 4.0 * error + 2e-3 * analytic
    finally:
        r.close()


def _cornell(grt, scheduler, prepare=None, config=None, samples=(2, 3), size=(64, 64)):
    r = Rendering(grt, grt.scene_path("cornellbox"), size[0], size[1], dict(num_bounces=4, **(config or {})), scheduler, black_sky=False)
    try:
        if prepare:
            prepare(r)
        first, frame = 0, None
        for count in samples:
            frame = r.render(count, first, batch=count); first += count
        return frame
    finally:
        r.close()


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_enable_render_disable_is_the_frame_that_never_enabled(grt, scheduler):
    never = _cornell(grt, scheduler)

    def on_then_off(r):
        assert grt.set_light_tree(r.pt.ctx, True) == 0 and grt.read_light_tree(r.pt.ctx).leaf_count > 0
        on_then_off.lit = r.render(2)
        assert grt.set_light_tree(r.pt.ctx, False) == 0 and grt.read_light_tree(r.pt.ctx).padded == 0
    again = _cornell(grt, scheduler, on_then_off)
    assert np.array_equal(never, again), scheduler
    assert np.isfinite(on_then_off.lit).all() and not np.array_equal(on_then_off.lit, _cornell(grt, scheduler, samples=(2,)))   # (the tree was in force: other samples)


def test_schedulers_agree_with_the_tree_and_its_variants_are_finite(grt, tmp_path):
    """With the tree on, the merged wavefront and the slot scheduler give identical frames: the plain _tree instances, _tree_nmap (a normal map on the diffuse
    materials), SVGF frames, and the tree beside sky sampling (taken > 0)."""
    import normal_map_reference
    normal_map_reference.write_tga(str(tmp_path / "n.tga"), normal_map_reference.random_normal_map(5, 16, 16))
    path = cases.write_many_lights(tmp_path, grid=4)
    for label, config, mapped, sky in (("tree", dict(num_bounces=3), False, False), ("nmap", dict(num_bounces=3), True, False), ("svgf", dict(num_bounces=3, enable_svgf=1), False, False),
                                       ("sky", dict(num_bounces=3, sky_sampling=0.25), False, True)):
        frames = {}
        for scheduler in ("merged", "slots"):
            r = Rendering(grt, path, 48, 32, dict(config, light_tree=1), scheduler, black_sky=not sky)
            try:
                if mapped:
                    t = r.scene.add_texture(str(tmp_path / "n.tga"), normal_map=True)
                    r.pt.close()
                    r.pt = grt.Pathtracer(r.scene, 48, 32, device=0)   # (textures reach the device when a Pathtracer is created)
                    for i in range(r.scene.material_count):
                        if r.scene.material_type(i) == grt.MATERIAL_DIFFUSE:
                            r.scene.set_material_normal_map(i, t)
                    r.pt.update()
                    assert r.lib.rt_set_sky(r.pt.ctx, BLACK.ctypes.data, 1, 1, 1.0) == 0
                    grt.set_scheduler(r.pt.ctx, scheduler)
                assert r.lib.rt_get_light_tree(r.pt.ctx) == 1 and grt.read_light_tree(r.pt.ctx).leaf_count == 32
                frames[scheduler] = r.render(3, batch=1)
                assert r.pt.counters().shadow[0] > 0, label
            finally:
                r.close()
        assert np.isfinite(frames["merged"]).all() and frames["merged"][..., :3].max() > 0, label
        assert np.array_equal(frames["merged"], frames["slots"]), label


def test_a_fog_volume_displaces_the_tree_with_one_warning(grt, tmp_path, capfd):
    path = cases.write_many_lights(tmp_path, grid=4)
    fog = dict(fog="-6,0,-6,6,3,6", fog_sigma_s=0.05)
    frames = {}
    for tree in (0, 1):
        capfd.readouterr()
        r = Rendering(grt, path, 48, 32, dict(num_bounces=3, light_tree=tree, **fog))
        try:
            assert r.lib.rt_get_light_tree(r.pt.ctx) == tree
            frames[tree] = r.render(2, batch=1)
            again = r.render(2, first=2, batch=1)
            assert np.isfinite(again).all()
        finally:
            r.close()
        assert capfd.readouterr().err.count("the light tree is not used") == tree
    assert np.array_equal(frames[0], frames[1]) and frames[0][..., :3].max() > 0


WORLD_SAMPLES, WORLD_K, WORLD_SHARE = 48, 4.0, 0.05


def test_tree_on_against_off_same_mean_less_noise(grt, tmp_path):
    """The many-light world (16 x 16 small quads over a wide floor), 64 x 64 pixels, 48 samples, direct light without MIS (every sample is the light sample c / pdf alone:
    what light_tree_reference.emitter_pdfs describes). Means: per pixel |mean_on - mean_off| <= 4 standard errors of the difference (Welford moments of both renders); at
    most 5 % of the pixels outside (heavy tails under selection by power: test_light_tree.py checks that the float64 restatement of the two estimators stays within that
    share at this sample count). Noise: the sum over the sampled floor pixels of the per-pixel sample variance with the tree, over the same sum without, against the
    ratio the reference predicts from the two selection pmfs at those pixels' floor points. Margin 3, set before the first run on a device: the variance estimates come
    from 48 samples of a heavy-tailed estimator (the reference's own 48-sample estimates of this ratio reach 1.7 x the prediction at their 99.9th percentile) and the
    prediction takes a triangle's centroid for its points and a pixel's centre for its footprint (light_tree_reference.estimator_moments, which integrates over both,
    moves it by 1 %). The device's 0.30 is inside the margin but above what those two explain; DESIGN.md 7.11, known limit (8). The tree's noise must also simply be lower."""
    path = cases.write_many_lights(tmp_path)
    config = dict(num_bounces=2, reconstruction_filter=0, enable_multiple_importance_sampling=0, enable_russian_roulette=0)
    mean, variance, error2 = {}, {}, {}
    for tree in (0, 1):
        r = Rendering(grt, path, 64, 64, dict(config, light_tree=tree))
        try:
            if tree:
                s = cases.scene_from_pathtracer(r.pt); want = ref.build32(s)
                got = grt.read_light_tree(r.pt.ctx)
                assert got.leaf_count == 512 and np.array_equal(bits(got.nodes), bits(want.nodes)), "the tree of a loaded scene differs from its restatement"
                xs, ys, points = cases.floor_points(r.pt.camera(), 64, 64, 4)
                predicted_tree = predicted_power = 0.0
                for point in points:
                    c, by_power, by_tree = ref.emitter_pdfs(s, want, point)
                    predicted_power += ref.selection_variance(c, by_power); predicted_tree += ref.selection_variance(c, by_tree)
            grt.set_noise_estimate(r.pt.ctx, True)
            mean[tree] = r.render(WORLD_SAMPLES + 1).astype(np.float64)[..., 0]
            m = grt.read_noise_moments(r.pt.ctx, 64, r.pt.pitch)[:, :64].astype(np.float64)
            variance[tree] = m[..., 0] / (m[..., 3] - 1); error2[tree] = variance[tree] / m[..., 3]
        finally:
            r.close()
    t = np.abs(mean[1] - mean[0]); bound = WORLD_K * np.sqrt(error2[0] + error2[1])
    outside = t > bound + 1e-12
    measured = variance[1][ys, xs].sum() / variance[0][ys, xs].sum(); predicted = predicted_tree / predicted_power
    print("tree on against off: %d of %d pixels outside %g standard errors (allowed %d); noise ratio measured %.4f, predicted %.4f (margin 3: %.4f), over %d floor pixels" % (
        outside.sum(), outside.size, WORLD_K, int(WORLD_SHARE * outside.size), measured, predicted, 3 * predicted, len(xs)))
    albedo2 = cases.WORLD["albedo"] ** 2   # (the reference's c leaves the floor's albedo out)
    print("summed per-pixel variance, measured / predicted: by power %.4g / %.4g, by the tree %.4g / %.4g" % (
        variance[0][ys, xs].sum(), albedo2 * predicted_power, variance[1][ys, xs].sum(), albedo2 * predicted_tree))
    assert mean[0].max() > 0 and outside.sum() <= WORLD_SHARE * outside.size
    assert measured < 1.0 and measured <= 3.0 * predicted


# ---- the launches, entry by entry ----------------------------------------------------------------------------------------------------------
# rt_shade_rays and rt_sort_rays with the tree in force take the _tree instances. The material launch's float64 restatement is material_reference.evaluate with the
# tree in its tables (tables.tree: the leaf the descent picks from the hit point, pdf = pmf d^2 / (A cos) (1 - taken)). The sort launch's is the plain one
# (sort_reference.py) with lights_total_weight, per entry, Y A / pmf -- so that Y d^2 / (cos W) is pmf d^2 / (A cos). The tolerances are material_checks.BOUNDS and sort_checks.BOUNDS.

WORLD_DELTA = [(0, (0.5, 3.0, 0.5), (0, 0, 1), (30, 25, 20), 0, 0), (0, (2.0, 1.5, -1.0), (0, 0, 1), (4, 8, 12), 0, 0)]   # two point lights (delta_light_reference.lights_array rows)
WORLD_DELTA_WEIGHTS = np.array([1.0, 2.0], F)


def _tree_of(grt, world):
    s = cases.scene_from_pathtracer(world.pt)
    got = grt.read_light_tree(world.ctx)
    want = ref.build32(s)
    assert got.leaf_count == want.leaf_count > 0 and np.array_equal(bits(got.nodes), bits(want.nodes))
    return s, ref.tree_from_nodes(got.nodes, got.leaf_count, got.slot_of_leaf), got


def _shares(grt, world, sky_share, delta):
    """Puts the sky's share and (delta: True for 0.5, or the share itself) two point lights in force; returns (s, q, taken) as the device will settle them."""
    import delta_light_reference as dref
    from ctypes import c_float
    world.lib.rt_set_sky_sampling.argtypes = [c_void_p, c_float]
    assert world.lib.rt_set_sky_sampling(world.ctx, sky_share) == 0
    if delta:
        lights = dref.lights_array(WORLD_DELTA)
        share = 0.5 if delta is True else float(delta)
        assert grt.upload_delta_lights(world.ctx, grt.delta_light_records(lights, WORLD_DELTA_WEIGHTS), share) == 0, world.lib.rt_last_error(world.ctx)
        return dref.split(sky_share, share, emitters=True)
    return F(sky_share), F(0), F(sky_share)


def _with_share(tables, share):
    import copy
    import sky_sampling_reference
    t = copy.copy(tables)
    t.sky_share = float(F(share))
    t.sky_tables = sky_sampling_reference.Tables(tables.sky) if t.sky_share > 0 else None
    return t


@pytest.fixture(scope="module")
def material_world(grt, oracle, tmp_path_factory):
    import material_cases
    w = material_cases.World(grt, oracle, tmp_path_factory.mktemp("tree_material"), 0)
    yield w
    w.close()


@pytest.mark.parametrize("sky_share,delta,mis", [(0.0, False, True), (0.0, False, False), (0.25, False, True), (0.0, True, True), (0.25, True, False)],
                         ids=["taken0", "taken0_mis_off", "sky", "delta", "sky_delta_mis_off"])
def test_material_launch_with_the_tree_carries_the_restated_shadow_rays(grt, material_world, sky_share, delta, mis):
    """A _tree material launch (diffuse hits, per-bounce at bounces 0 and 2 and merged): the shadow ray of every hit whose light sample goes to the emitters carries
    throughput f L w / pdf of the float64 restatement with pdf = pmf d^2 / (A cos)(1 - taken), from the restated origin in the restated direction. Entries whose pick is
    not robust (u within 64 ulps of a node's boundary) or that the plain restatement flags are left out, at most material_checks.NON_ROBUST_CAP of a launch."""
    import delta_light_reference as dref
    import material_cases as mcases
    import material_checks as mc
    import material_reference as mref
    world = material_world
    tables = world.apply(mcases.SETUP["default" if mis else "mis_off"])
    try:
        s_, q_, taken = _shares(grt, world, sky_share, delta)
        assert grt.set_light_tree(world.ctx, True) == 0, world.lib.rt_last_error(world.ctx)
        s, tree, got_tree = _tree_of(grt, world)
        launches = [mcases.per_bounce(world, "tree", 0, 1500, b, seed=5100 + b) for b in (0, 2)] + [mcases.merged(world, "tree", 0, 2500, seed=5150)]
        for launch in launches:
            name = "tree_%s/%s" % ("mis" if mis else "nomis", launch.name)
            got = mc.device_launch(grt, world.ctx, launch, capacity=launch.entries.n + 37)
            trace_at, shadow_at = mc.match(launch, got, name)
            under_tree = _with_share(tables, s_)   # the one restatement of every instance: the sky's share, the delta lights and the tree in its tables
            under_tree.delta = mref.Delta(dref.Table(dref.lights_array(WORLD_DELTA), WORLD_DELTA_WEIGHTS), 0.5 if delta is True else float(delta), *grt.read_delta_lights(world.ctx)[:2]) if delta else None
            under_tree.tree = mref.TreeTables(s, tree, got_tree.leaf_area)
            r = mref.evaluate(world, under_tree, launch, world.bsdf_tables)
            to_emitters = r.route == mref.ROUTE_TREE
            slot_, real, bounce, sample, submission = launch.paths()
            assert np.array_equal(to_emitters, ~(tables.random(mref.DIM_NEE_LIGHT, real, bounce, sample)[:, 0] < taken))   # (u below taken goes to the sky or a delta light)
            leaf = r.tree_leaf
            mine = to_emitters & r.alive & r.allow_nee & r.robust
            left_out = int((to_emitters & r.alive & r.allow_nee & ~r.robust).sum())
            emitted = shadow_at >= 0
            wrong = mine & (emitted != r.has_shadow)
            assert not wrong.any(), "%s: entry %d: a shadow ray %s, float64 says otherwise" % (name, np.nonzero(wrong)[0][0], "is emitted" if emitted[np.nonzero(wrong)[0][0]] else "is missing")
            index = np.nonzero(mine & emitted)[0]
            f = got.shadow_out[shadow_at[index]].view(F).astype(np.float64)
            plain_rows = ~r.textured[index]
            errors = {"shadow_origin": mc._point(f[:, 0:3], r.shadow_origin[index]), "shadow_direction": np.abs(f[:, 3:6] - r.shadow_direction[index]).max(axis=1),
                      "shadow_distance": mc._relative(f[:, 6], r.shadow_distance[index], 1e-30), "illumination": mc._per_channel(f[plain_rows, 7:10], r.illumination[index][plain_rows])}
            worst = {k: float(v.max(initial=0)) for k, v in errors.items()}
            print("%-36s %5d entries, %5d shadow entries held, %3d left out, leaves picked %d; " % (name, launch.entries.n, index.size, left_out, np.unique(leaf[index]).size) + " ".join("%s %.2g" % kv for kv in worst.items()))
            assert index.size > 200 and left_out <= mc.NON_ROBUST_CAP * launch.entries.n, (name, index.size, left_out)
            for k, v in worst.items():
                assert np.isfinite(v) and v <= mc.BOUNDS[k], "%s: %s is %.3g from float64's, the bound is %.3g" % (name, k, v, mc.BOUNDS[k])
    finally:
        grt.set_light_tree(world.ctx, False)
        grt.upload_delta_lights(world.ctx, None)
        world.lib.rt_set_sky_sampling(world.ctx, 0.0)
        world.apply(mcases.SETUP["default"])


def test_material_launch_at_taken_one_sends_no_light_sample_to_the_emitters(grt, material_world):
    """The tree in force and a delta-light share of 1 (taken == 1): next_event_estimation<3> never reaches the tree. Every shadow ray a _tree material launch emits ends
    on one of the two point lights (origin + direction x distance within 1e-4 relative of a light's position); and the launch does emit shadow rays."""
    import material_cases as mcases
    import material_checks as mc
    world = material_world
    world.apply(mcases.SETUP["default"])
    try:
        s_, q_, taken = _shares(grt, world, 0.0, 1.0)
        assert float(taken) == 1.0
        assert grt.set_light_tree(world.ctx, True) == 0, world.lib.rt_last_error(world.ctx)
        assert grt.read_light_tree(world.ctx).leaf_count > 0
        positions = np.array([row[1] for row in WORLD_DELTA], np.float64)
        for launch in [mcases.per_bounce(world, "taken1", 0, 1500, 1, seed=5300), mcases.merged(world, "taken1", 0, 2500, seed=5350)]:
            got = mc.device_launch(grt, world.ctx, launch, capacity=launch.entries.n + 37)
            trace_at, shadow_at = mc.match(launch, got, "taken1/" + launch.name)
            f = got.shadow_out[shadow_at[shadow_at >= 0]].view(F).astype(np.float64)
            assert f.shape[0] > 200, f.shape
            end = f[:, 0:3] + f[:, 3:6] * f[:, 6:7]
            miss = np.linalg.norm(end[:, None] - positions[None], axis=2).min(axis=1) / (1.0 + f[:, 6])
            print("taken1/%-30s %5d shadow rays, all to a point light: worst end-point miss %.2g" % (launch.name, f.shape[0], miss.max()))
            assert np.isfinite(f[:, 6]).all() and miss.max() <= 1e-4
    finally:
        grt.set_light_tree(world.ctx, False)
        grt.upload_delta_lights(world.ctx, None)
        world.apply(mcases.SETUP["default"])


@pytest.fixture(scope="module")
def sort_world(grt, oracle, tmp_path_factory):
    import sort_cases
    w = sort_cases.World(grt, oracle, tmp_path_factory.mktemp("tree_sort"), 0)
    yield w
    w.close()


@pytest.mark.parametrize("sky_share,delta", [(0.0, False), (0.25, False), (0.0, True), (0.25, True), (0.0, 1.0)], ids=["taken0", "sky", "delta", "sky_delta", "taken1"])
def test_sort_launch_with_the_tree_weighs_emitter_hits_by_the_trees_pmf(grt, sort_world, sky_share, delta):
    """rt_sort_rays with the tree in force (kernel_sort_tree, kernel_sort_stream_tree), MIS on: an emitter hit found by a ray that was allowed NEE adds throughput x
    emission x power_heuristic(brdf_pdf, pmf(origin) t^2 / (A cos) (1 - taken)), the pmf of the hit triangle's leaf seen from the ray's origin in the queue. The float64
    restatement of the sort launch with W_i = Y A / pmf_i per entry, within sort_checks.BOUNDS; and the weights are far from the power tables' (the check is sharp).
    taken1 (the delta lights' share is 1, so taken == 1): count_light is forced -- every emitter hit adds throughput x emission whole (the restatement's frames, to
    sort_checks.BOUNDS) and none is weighed."""
    import copy
    import sort_cases as scases
    import sort_checks as schecks
    import sort_reference as sref
    world = sort_world
    tables = world.apply(scases.SETUP["default" if sky_share == 0 else "sky_share_0.25"])
    try:
        s_, q_, taken = _shares(grt, world, sky_share, delta)
        assert grt.set_light_tree(world.ctx, True) == 0, world.lib.rt_last_error(world.ctx)
        s, tree, got_tree = _tree_of(grt, world)
        classes = (scases.EMITTER, scases.EMITTER, scases.DIFFUSE, scases.PLASTIC, scases.DIELECTRIC, scases.CONDUCTOR)
        launches = []
        for b in (1, 2):
            rng = np.random.default_rng(5200 + b)
            px = scases.pixels_for(rng, 4000, world.frame_pixels, 1)
            launches.append(scases.per_bounce(world, "bounce%d" % b, scases.make_entries(world, rng, px, b, classes=classes), b, seed=b, slots=1))
        merged = scases.merged_launch(world, scases.NUM_BOUNCES)[0]
        keep = np.nonzero(merged.entries.triangle != sref.INVALID)[0]
        sub = sref.Launch("merged", merged.entries.take(keep), merged.frame_pixels, merged.frame_slots, bounce=merged.bounce, sample_index=merged.sample_index,
                          iteration=merged.iteration, slot_table=merged.slot_table, submission_birth=merged.submission_birth, aov=merged.aov)
        sub.gnd, sub.gid, sub.gsp = merged.gnd, merged.gid, merged.gsp
        launches.append(sub)
        for launch in launches:
            e = launch.entries
            name = "tree_s%g_%s/%s" % (sky_share, "delta" if delta else "nodelta", launch.name)
            hit = e.triangle != sref.INVALID
            leaf = ref.leaf_of_hit(s, np.where(hit, e.mesh, -1), e.triangle)
            on_leaf = leaf >= 0
            pmf = ref.pmf64(tree, e.origin, tree.slot_of_leaf[np.maximum(leaf, 0)])[0]
            rows = s.leaf_table()[3][np.maximum(leaf, 0)]
            emission = s.materials[s.material_ids[rows], :3].astype(np.float64)
            y = np.float64(F(0.299)) * emission[:, 0] + np.float64(F(0.587)) * emission[:, 1] + np.float64(F(0.114)) * emission[:, 2]
            with np.errstate(all="ignore"):
                w = np.where(on_leaf & (pmf > 0), y * got_tree.leaf_area[np.maximum(leaf, 0)].astype(np.float64) / pmf, np.inf)
            under_tree = _with_share(tables, taken); under_tree.lights_total_weight = ref.PerEntry(w)
            result = sref.evaluate(under_tree, launch, schecks.MARGINS)
            allowed = sref.allowed_outcomes(under_tree, launch, schecks.MARGINS, result)
            got = schecks.device_launch(world.grt, world.ctx, launch, scases.SENTINEL, capacity=e.n + 37)
            matched = schecks.check_structure(name, under_tree, launch, got, result, allowed, scases.SENTINEL)
            errors = schecks.compare_with_reference(name, under_tree, launch, got, matched, result, schecks.BOUNDS)
            weighed = np.isfinite(result.light_pdf) & np.isfinite(result.weight)
            assert (pmf[on_leaf & (e.t > 0)] > 0).any()
            if float(taken) == 1.0:
                assert not weighed.any() and not np.isfinite(result.light_pdf).any() and on_leaf.sum() > 100, name
                print("%-40s %6d entries, %5d emitter hits, taken = 1: all counted whole, none weighed; " % (name, e.n, on_leaf.sum()) + " ".join("%s %.2g" % (k, v[0]) for k, v in errors.items()))
                continue
            other = sref.evaluate(_with_share(tables, taken), launch, schecks.MARGINS)
            apart = np.abs(result.weight[weighed] - other.weight[weighed])
            print("%-40s %6d entries, %5d emitter hits weighed; " % (name, e.n, weighed.sum()) + " ".join("%s %.2g" % (k, v[0]) for k, v in errors.items()) + "; median |w - w_power| %.3g" % np.nanmedian(apart))
            assert weighed.sum() > 100 and np.nanmedian(apart) > 1e-4 and (apart > 1e-3).sum() > 50, (name, weighed.sum(), np.nanmedian(apart))
    finally:
        grt.set_light_tree(world.ctx, False)
        grt.upload_delta_lights(world.ctx, None)
        world.apply(scases.SETUP["default"])
