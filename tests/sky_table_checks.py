"""What a set of sky sampling tables must keep against the float64 reference (sky_sampling_reference.DeviceTables, forward order), whoever built
them: the device (test_gpu_sky_tables.py, through rt_read_sky_tables) or the reference in the kernels' own order of additions
(test_sky_tables.py). `got` is the dict read_sky_tables returns; every check returns the figures it measured."""
import numpy as np

import sky_sampling_reference as ref


def as_read_back(t):
    """A DeviceTables in the form of read_sky_tables' dict."""
    return dict(width=t.w, height=t.h, marginal=t.marginal, conditional=t.conditional, cell_pdf=t.cell_pdf, row_totals=t.row_total, total=t.total)


def check_structure(got, want, underflows=False):
    h, w = want.h, want.w
    assert (got["width"], got["height"]) == (w, h)
    assert got["marginal"].shape == (h,) and got["conditional"].shape == (h, w) and got["cell_pdf"].shape == (h, w) and got["row_totals"].shape == (h,)
    assert got["marginal"].dtype == np.float32 and got["conditional"].dtype == np.float32 and got["cell_pdf"].dtype == np.float32
    assert np.all(np.diff(got["marginal"]) >= 0) and got["marginal"][0] >= 0 and got["marginal"][-1] == np.float32(1.0)
    assert np.all(np.diff(got["conditional"], axis=1) >= 0) and np.all(got["conditional"][:, 0] >= 0) and np.all(got["conditional"][:, -1] == np.float32(1.0))
    weightless = want.row_total == 0
    assert np.array_equal(got["row_totals"] == 0, weightless)
    uniform = ((np.arange(w) + 1) / np.float32(w)).astype(np.float32)
    assert np.array_equal(got["conditional"][weightless], np.broadcast_to(uniform, (int(weightless.sum()), w)))
    previous = np.concatenate([[np.float32(0.0)], got["marginal"][:-1]])
    inner = weightless.copy(); inner[-1] = False   # (the last entry is the forced 1.0)
    assert np.array_equal(got["marginal"][inner], previous[inner])
    # pdf 0 exactly where the footprint luminance is 0 -- and, in a sky whose range exceeds float32's, where the quotient rounds to 0
    quiet = (want.lum > 0) & (want.lum.astype(np.float64) / want.total < 2.0 ** -150)
    assert underflows or not quiet.any()
    assert np.array_equal(got["cell_pdf"] == 0, (want.lum == 0) | quiet)
    assert np.all(got["cell_pdf"] >= 0) and np.isfinite(got["cell_pdf"]).all()


def check_totals(got, want):
    """Row totals and the total within the bounds derived in DeviceTables' docstring. Returns the worst share of a bound taken."""
    row_error = np.abs(got["row_totals"] - want.row_total)
    assert np.all(row_error <= want.row_total_bound), float(np.max(row_error / np.where(want.row_total_bound > 0, want.row_total_bound, 1.0)))
    total_error = abs(got["total"] - want.total)
    assert total_error <= want.total_bound, total_error / want.total_bound
    lit = want.row_total_bound > 0
    return max(float((row_error[lit] / want.row_total_bound[lit]).max()) if lit.any() else 0.0, total_error / want.total_bound)


def check_entries(got, want):
    """CDF entries and cell pdfs as float32 bits: at most one ulp apart, at most 1 entry in 10 000 of a table apart at all. Returns {table: (differing, worst ulps)}."""
    figures = {}
    for name, a, b in (("marginal", got["marginal"], want.marginal), ("conditional", got["conditional"], want.conditional), ("cell_pdf", got["cell_pdf"], want.cell_pdf)):
        differing, worst = ref.entries_differ(a, b)
        assert worst <= 1, (name, differing, worst)
        assert differing * ref.DeviceTables.CAP <= a.size, (name, differing, a.size)
        figures[name] = (differing, worst)
    return figures


def check_marginal_is_the_span_scan(got):
    """kernel_sky_marginal's arithmetic is IEEE double additions in a fixed order and one division per entry: on the row totals the read-back itself
    returns, the total and every marginal entry are reproduced bit for bit."""
    prefix, total = ref.scan_spans(got["row_totals"])
    assert float(total) == got["total"], (float(total), got["total"])
    assert np.array_equal(ref.cdf32_from_scan(prefix, total), got["marginal"])


def check_sampled_is_claimed(got, p_cell):
    """sum |P32 - P_cell| within (W + H) 2^-24, P_cell the plain float64 table. Returns (share of the bound, mass the float32 CDFs never pick)."""
    distance, bound, unreachable = ref.sampled_against_claimed(got["marginal"], got["conditional"], p_cell)
    assert distance <= bound, (distance, bound)
    return distance / bound, unreachable


def check_constant_sky(got):
    """A constant sky in closed form. A float32 rounding boundary in [2^-e-1, 2^-e) is a multiple of 2^-(e+25), so k / 257 (no such multiple: 257 is odd)
    lies at least 1 / (257 2^(e+25)) from it, a relative 2^-25 / 257 = 1.2e-10 or more; the double sums and the quotient are off by a relative
    2 W 2^-53 = 6e-14. So the conditional entries are (x + 1) / W rounded once, exactly; the marginal keeps the cap of check_entries."""
    h, w = got["height"], got["width"]
    assert w == 257
    closed = ((np.arange(w) + 1.0) / w).astype(np.float32); closed[-1] = 1.0
    assert np.array_equal(got["conditional"], np.broadcast_to(closed, (h, w)))
    marginal = ((1.0 - np.cos(np.pi * (np.arange(h) + 1.0) / h)) / 2.0).astype(np.float32); marginal[-1] = 1.0
    differing, worst = ref.entries_differ(got["marginal"], marginal)
    assert worst <= 1 and differing * ref.DeviceTables.CAP <= h, (differing, worst)
