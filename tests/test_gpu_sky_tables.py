"""The sky sampling tables on the MI355X, entry by entry (kernel_sky_rows, kernel_sky_marginal, kernel_sky_cell_pdf of kernels_sky.hip, read
back through rt_read_sky_tables), at the sizes of environment maps: the cases of sky_cases.py against the float64 restatement of
sky_sampling_reference.py under the conditions of sky_table_checks.py, the inversion (rt_sample_sky_distribution) against numpy's on the device's
own tables, and chi-square, the closed-form frame and the evaluation probe at size. test_sky_tables.py shows that the reference alone keeps every
condition used here."""
import math
from ctypes import byref, c_double, c_int, c_size_t, c_void_p, POINTER
from types import SimpleNamespace

import numpy as np
import pytest

import sky_sampling_reference as ref
import sky_table_checks as checks
from sky_cases import BY_NAME, CASES
from test_gpu_sky_sampling import _angle, _check_sun_lit_plane, _lib, _set_sky

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG = -1
_current = {}


@pytest.fixture(scope="module")
def bare(grt):
    lib = _lib(grt)
    ctx = c_void_p()
    assert lib.rt_create(0, byref(ctx)) == 0, lib.rt_last_error(None)
    yield lib, ctx
    _current.clear()
    lib.rt_destroy(ctx)


def _load(grt, bare, name):
    """The case's sky on the module's context, its tables read back and its reference: kept until another case is asked for (the tests run
    case by case, and the tests behind the parametrised ones begin with the last case, the 2048 x 1024 sky: one upload of it per module)."""
    if _current.get("name") != name:
        _current.clear()
        lib, ctx = bare
        case = BY_NAME[name]
        sky = case.build()
        _set_sky(lib, ctx, sky)
        _current.update(name=name, state=SimpleNamespace(case=case, sky=sky, ctx=ctx, got=grt.read_sky_tables(ctx), want=ref.DeviceTables(sky), plain=None))
    return _current["state"]


def _plain(state):
    if state.plain is None:
        state.plain = ref.Tables(state.sky)
    return state.plain


@pytest.fixture(scope="module", params=CASES, ids=lambda c: c.name)
def loaded(request, grt, bare):
    return _load(grt, bare, request.param.name)


def test_read_back_refusals_and_partial_reads(grt, bare):
    lib, ctx = bare
    lib.rt_read_sky_tables.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double), c_size_t]
    assert lib.rt_read_sky_tables(None, None, None, None, None, None, None, None, 0) == RT_ERROR_INVALID_ARG
    assert lib.rt_last_error(None) == b"rt_read_sky_tables: NULL context"
    fresh = c_void_p()
    assert lib.rt_create(0, byref(fresh)) == 0
    try:
        assert lib.rt_read_sky_tables(fresh, None, None, None, None, None, None, None, 0) == RT_ERROR_INVALID_ARG
        assert lib.rt_last_error(fresh) == b"rt_read_sky_tables: no sky uploaded (rt_set_sky)"
        sky = ref.sun_sky(37, 19, (5, 5))
        _set_sky(lib, fresh, sky)
        w, h, total = c_int(), c_int(), c_double()
        assert lib.rt_read_sky_tables(fresh, byref(w), byref(h), None, None, None, None, byref(total), 0) == 0 and (w.value, h.value) == (37, 19) and total.value > 0
        marginal = np.full(20, -1.0, np.float32)
        assert lib.rt_read_sky_tables(fresh, None, None, marginal.ctypes.data, None, None, None, None, 37 * 19 - 1) == RT_ERROR_INVALID_ARG
        assert lib.rt_last_error(fresh) == b"rt_read_sky_tables: room for 702 cells, the 37x19 sky has 703" and np.all(marginal == -1.0)
        assert lib.rt_read_sky_tables(fresh, None, None, marginal.ctypes.data, None, None, None, None, 37 * 19) == 0
        assert marginal[18] == 1.0 and marginal[19] == -1.0
        whole = grt.read_sky_tables(fresh)
        assert np.array_equal(whole["marginal"], marginal[:19]) and whole["total"] == total.value
        # the context is as a render with sampling on leaves it: the probes and a second read see the same tables
        d = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]], np.float32)
        assert np.array_equal(grt.sky_pdf(fresh, d), [whole["cell_pdf"][0, 18], whole["cell_pdf"][9, 18]])
        again = grt.read_sky_tables(fresh)
        assert all(np.array_equal(whole[k], again[k]) for k in whole)
        sky[3, 3, 0] = np.nan
        _set_sky(lib, fresh, sky)
        assert lib.rt_read_sky_tables(fresh, byref(w), byref(h), None, None, None, None, None, 0) == RT_ERROR_INVALID_ARG
        assert lib.rt_last_error(fresh).startswith(b"rt_read_sky_tables: sky sampling needs a finite sky")
    finally:
        lib.rt_destroy(fresh)


def test_structure(loaded):
    checks.check_structure(loaded.got, loaded.want, loaded.case.underflows)
    if loaded.case.name.startswith("constant"):
        checks.check_constant_sky(loaded.got)


def test_row_totals_and_total(loaded):
    share = checks.check_totals(loaded.got, loaded.want)
    print("%s: row totals and total at %.3g of their bound" % (loaded.case.name, share))


def test_entries_bit_for_bit(loaded):
    figures = checks.check_entries(loaded.got, loaded.want)
    print("%s: entries differing (count, ulps) %s" % (loaded.case.name, figures))


def test_marginal_is_the_span_scan_of_the_row_totals(loaded):
    checks.check_marginal_is_the_span_scan(loaded.got)


def test_what_is_sampled_is_what_is_claimed(loaded):
    share, unreachable = checks.check_sampled_is_claimed(loaded.got, _plain(loaded).p_cell)
    print("%s: sum |P32 - P_cell| at %.3g of (W + H) 2^-24, unreachable mass %.3g" % (loaded.case.name, share, unreachable))


ONE_BELOW = np.float32(1.0 - 2.0 ** -24)
GRID = 256


def _grid():
    g = (np.arange(GRID, dtype=np.float32) + np.float32(0.5)) / np.float32(GRID)
    return np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2).astype(np.float32)


def _around(entries):
    e = np.asarray(entries, np.float32)
    v = np.concatenate([e, np.nextafter(e, np.float32(-1.0)), np.nextafter(e, np.float32(2.0))])
    return v[(v >= 0) & (v <= ONE_BELOW)]


def _pick(n, count, rng):
    if n <= count:
        return np.arange(n)
    return np.unique(np.concatenate([[0, 1, n - 2, n - 1], rng.choice(n, count, replace=False)]))


def _edge_points(got):
    """0, 2^-24, 1 - 2^-24, and table entries with their two float32 neighbours: some 300 of the marginal (at three values of u) and a
    hundred each of four lit rows' CDFs (v in the middle of the row's interval of the marginal)."""
    rng = np.random.default_rng(17)
    basics = np.array([0.0, 2.0 ** -24, ONE_BELOW], np.float32)
    m, c = got["marginal"], got["conditional"]
    v_edges = np.unique(np.concatenate([basics, _around(m[_pick(len(m), 300, rng)])]))
    points = [np.stack([np.full(len(v_edges), u, np.float32), v_edges], axis=1) for u in (0.0, 0.5, ONE_BELOW)]
    below = np.concatenate([[np.float32(0.0)], m[:-1]])
    lit = np.flatnonzero(m > below)
    for r in np.unique(lit[[0, len(lit) // 3, len(lit) // 2, len(lit) - 1]]):
        middle = np.float32(0.5) * (below[r] + m[r])
        v = middle if below[r] < middle < m[r] else below[r]
        u_edges = np.unique(np.concatenate([basics, _around(c[r, _pick(c.shape[1], 100, rng)])]))
        points.append(np.stack([u_edges, np.full(len(u_edges), v, np.float32)], axis=1))
    return np.concatenate(points).astype(np.float32)


def _inversion(grt, state):
    """rt_sample_sky_distribution on the grid and the edge points, and numpy's searches on the tables the device returned; once per case."""
    if "inversion" not in _current:
        got = state.got
        uv = np.concatenate([_grid(), _edge_points(got)])
        out = grt.sample_sky_distribution(state.ctx, uv)
        row, fy, col, fx = ref.invert_tables(got["marginal"], got["conditional"], uv)
        _current["inversion"] = SimpleNamespace(uv=uv, d=out[:, :3], pdf=out[:, 3], row=row, fy=fy, col=col, fx=fx)
    return _current["inversion"]


def test_inversion_on_the_devices_own_tables(grt, loaded):
    """rt_sample_sky_distribution against numpy's searches on the tables the device returned: every point in the cell numpy finds -- the direction
    within the existing test's 1e-5 rad of that cell's point at the same fractions, no stray allowed (the search is comparisons only) --, the
    returned pdf rt_sky_pdf's of the returned direction bit for bit, and the inversion monotone along both axes of the grid."""
    got, ctx = loaded.got, loaded.ctx
    h, w = got["height"], got["width"]
    p = _inversion(grt, loaded)
    assert np.allclose(np.linalg.norm(p.d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    apart = _angle(p.d.astype(np.float64), ref.direction_of(h, w, p.row, p.fy, p.col, p.fx))
    far = apart > 1e-5
    other_lookup = p.pdf != grt.sky_pdf(ctx, p.d)
    print("%s: largest angle to numpy's point %.3g rad, %d apart; pdf not rt_sky_pdf's of the direction at %d points" % (loaded.case.name, apart.max(), far.sum(), other_lookup.sum()))
    assert far.sum() == 0, (int(far.sum()), p.uv[far][:4], p.row[far][:4], p.col[far][:4])
    assert other_lookup.sum() == 0, (int(other_lookup.sum()), p.uv[other_lookup][:4], p.row[other_lookup][:4], p.col[other_lookup][:4], p.fx[other_lookup][:4], p.fy[other_lookup][:4])
    # monotone: along a grid line of constant v (one row) the azimuth never steps back, along one of constant u the height never rises
    grid = p.d[:GRID * GRID].astype(np.float64).reshape(GRID, GRID, 3)
    azimuth = np.arctan2(-grid[..., 2], grid[..., 0]) / (2.0 * np.pi) + 0.5
    assert np.all(np.diff(azimuth, axis=1) >= -1e-6), float(np.diff(azimuth, axis=1).min())
    assert np.all(np.diff(grid[..., 1], axis=0) <= 2.0 ** -22), float(np.diff(grid[..., 1], axis=0).max())
    columns = p.col[:GRID * GRID].reshape(GRID, GRID); rows = p.row[:GRID * GRID].reshape(GRID, GRID)
    assert np.all(np.diff(columns, axis=1) >= 0) and np.all(np.diff(rows, axis=0) >= 0)


def test_sampled_pdf_is_the_picked_cells_entry_and_positive(grt, loaded):
    """The pdf rt_sample_sky_distribution returns is the read-back entry of the cell the searches picked, bit for bit; every returned pdf is
    positive and sample_sky(direction) / pdf finite, at u = 0 and on the 1e+-30 sky as well.

    sky_sample_direction returns the picked cell's entry and keeps the direction inside that cell as sky_cell finds it, so the first condition and
    the test before this one together say that sampling and evaluation read one number. Before it did, the pdf was read through
    sky_pdf(direction), and a direction at fraction 0 of its cell -- u equal to a CDF entry, or u = 0 -- went through atan2f / acosf into the cell
    before it about every other time: 16 of 318 up to 2 065 of 3 936 edge points per case returned a neighbour's entry (never one of the 65 536
    grid points), and 0 where the neighbour was weightless (3, 2, 13 and 47 points of the black-row, black-column, single-texel and 1e+-30 skies)."""
    got = loaded.got
    p = _inversion(grt, loaded)
    other_cell = p.pdf != got["cell_pdf"][p.row, p.col]
    radiance = grt.sample_sky(loaded.ctx, p.d).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = radiance / p.pdf[:, None].astype(np.float64)
    dark = ~(p.pdf > 0) | ~np.isfinite(ratio).all(axis=1)
    print("%s: %d points (%d at edges); pdf not the picked cell's entry %d (%d of them grid points), pdf not positive or ratio not finite %d (%d grid points)"
          % (loaded.case.name, len(p.uv), len(p.uv) - GRID * GRID, other_cell.sum(), other_cell[:GRID * GRID].sum(), dark.sum(), dark[:GRID * GRID].sum()))
    assert other_cell.sum() == 0, (int(other_cell.sum()), p.uv[other_cell][:4], p.row[other_cell][:4], p.col[other_cell][:4], p.fx[other_cell][:4], p.fy[other_cell][:4])
    assert dark.sum() == 0, (int(dark.sum()), p.uv[dark][:4])


# ---- at size: chi-square, the evaluation probe, frames (the parametrised tests above end on the 2048 x 1024 sky: it is still loaded) --------

def _chi_square(grt, state):
    """test_gpu_sky_sampling.test_chi_square_of_the_cells' method: 2^20 random points binned by the cell of their direction against N P_cell."""
    uv = np.random.default_rng(5).random((1 << 20, 2), dtype=np.float32)
    out = grt.sample_sky_distribution(state.ctx, uv)
    t = _plain(state)
    r, c = t.cell(out[:, :3])
    counts = np.bincount(r * t.w + c, minlength=t.h * t.w).astype(np.float64)
    expected = len(uv) * t.p_cell.ravel()
    big = expected >= 5
    assert counts[expected == 0].sum() == 0
    obs = np.append(counts[big], counts[~big].sum()); exp = np.append(expected[big], expected[~big].sum())
    keep = exp > 0
    chi2 = float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum())
    dof = int(keep.sum()) - 1
    print("%s: chi-square %.1f on %d degrees of freedom" % (state.case.name, chi2, dof))
    assert dof >= 8 and (chi2 - dof) / math.sqrt(2 * dof) < 5.0, (state.case.name, chi2, dof)


def test_chi_square_at_real_size(grt, bare):
    _chi_square(grt, _load(grt, bare, "real_size_2048x1024"))


def _clamped_max(a, reach):
    h, w = a.shape
    out = a.copy()
    for dy in range(-reach, reach + 1):
        ys = np.clip(np.arange(h) + dy, 0, h - 1)
        for dx in range(-reach, reach + 1):
            xs = np.clip(np.arange(w) + dx, 0, w - 1)
            out = np.maximum(out, a[ys][:, xs])
    return out


def test_evaluation_probe_at_real_size(grt, bare):
    """rt_sample_sky against sample_sky in float64 on the 2048 x 1024 sky. The tolerance is the float32 tap position times the sky's slope there:
    u = atan2f(..) * (1 / 2pi) + 0.5 carries the atan2f's error (taken as 3 ulp of a value below pi, 3 * 2^-22, over 2 pi), the rounding of the
    constant, of the product and of the sum (2^-25 each); u * W - 0.5 adds two half ulps of a value below 2048 (2^-14 each): 5.4e-4 texel in x.
    v = acosf(..) * (1 / pi) likewise: 3 * 2^-22 / pi + 2 * 2^-25, times H, plus two half ulps below 1024 (2^-15): 3.6e-4 texel in y. A bilinear
    surface moves by at most its largest neighbouring-texel difference per texel of displacement (taken over the 5 x 5 texels around the point:
    the taps and whatever the displaced taps reach); the three lerps add 8 * 2^-24 of the largest texel there."""
    state = _load(grt, bare, "real_size_2048x1024")
    sky, h, w = state.sky, state.case.height, state.case.width
    rng = np.random.default_rng(23)
    d = rng.normal(size=(200000, 3))
    sun = ref.direction_of(h, w, np.full(20000, 299), rng.uniform(-1.0, 3.0, 20000), np.full(20000, 687), rng.uniform(-1.0, 3.0, 20000))   # around the 2 x 2 sun
    d = np.concatenate([d / np.linalg.norm(d, axis=1, keepdims=True), sun, [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]]).astype(np.float32)
    got = grt.sample_sky(state.ctx, d).astype(np.float64)
    want = ref.sample_sky(sky, 1.0, d)
    position_x = w * (3 * 2.0 ** -22 / (2 * np.pi) + 3 * 2.0 ** -25) + 2 * 2.0 ** -14
    position_y = h * (3 * 2.0 ** -22 / np.pi + 2 * 2.0 ** -25) + 2 * 2.0 ** -15
    rgb = sky[..., :3].astype(np.float64)
    right = np.abs(rgb[:, np.clip(np.arange(w) + 1, 0, w - 1)] - rgb).max(axis=2)
    down = np.abs(rgb[np.clip(np.arange(h) + 1, 0, h - 1)] - rgb).max(axis=2)
    slope = _clamped_max(np.maximum(right, down), 2)
    largest = _clamped_max(rgb.max(axis=2), 2)
    r, c = _plain(state).cell(d)
    tolerance = (position_x + position_y) * slope[r, c] + 8 * 2.0 ** -24 * largest[r, c]
    share = np.abs(got - want).max(axis=1) / tolerance
    print("rt_sample_sky at 2048 x 1024: worst share of the tolerance %.3g (tap position %.2e / %.2e texel)" % (share.max(), position_x, position_y))
    assert np.all(share <= 1.0), (float(share.max()), d[np.argmax(share)])


def test_chi_square_under_a_sun_across_a_span_border(grt, bare):
    _chi_square(grt, _load(grt, bare, "sun_border_x_1027x515"))


def test_sun_lit_plane_under_the_sky_whose_sun_straddles_a_span_border(grt, tmp_path):
    """test_gpu_sky_sampling's closed-form frame (every pixel ALBEDO / pi * E, the image mean within five standard errors with the option on, with
    and without MIS, and off) under the 1027 x 515 sky of sky_cases.py, at that test's sample counts."""
    _check_sun_lit_plane(grt, tmp_path, BY_NAME["sun_border_x_1027x515"].build())
