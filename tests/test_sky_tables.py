"""The float64 reference of the sky sampling tables against itself (no GPU): every case of sky_cases.py is what its premise says, and the
reference evaluated in the kernels' own order of additions (spans of per_thread items, a Hillis-Steele scan of the span sums) keeps every
condition test_gpu_sky_tables.py puts to the device against the reference in the plain order -- so a device failure is the device's."""
import numpy as np
import pytest

import sky_sampling_reference as ref
import sky_table_checks as checks
from sky_cases import CASES

_cache = {}


def _tables(case):
    """(sky, forward-order tables, span-order tables, the plain float64 Tables) of a case, one case kept at a time (the tests run case by case)."""
    if case.name not in _cache:
        _cache.clear()
        sky = case.build()
        _cache[case.name] = (sky, ref.DeviceTables(sky, "forward"), ref.DeviceTables(sky, "spans"), ref.Tables(sky))
    return _cache[case.name]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_case_is_what_its_premise_says(case):
    sky, forward, spans, plain = _tables(case)
    assert sky.shape == (case.height, case.width, 4) and sky.dtype == np.float32 and case.premise
    case.check(sky, forward)
    # building it again gives the same sky: the GPU test sees these texels
    assert np.array_equal(case.build(), sky)
    # the float32 luminance is the float64 one to rounding, and the float32 maximum picks among the same texels
    assert np.allclose(forward.lum, plain.lum, rtol=3e-7, atol=0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_two_orders_of_additions_keep_the_cap(case):
    """Forward cumsum against spans + Hillis-Steele: structure exact, totals within the derived bounds, entries within 1 ulp and 1 in 10 000."""
    _, forward, spans, _ = _tables(case)
    got = checks.as_read_back(spans)
    checks.check_structure(got, forward, case.underflows)
    checks.check_structure(checks.as_read_back(forward), forward, case.underflows)
    share = checks.check_totals(got, forward)
    figures = checks.check_entries(got, forward)
    checks.check_marginal_is_the_span_scan(got)
    if case.name.startswith("constant"):
        checks.check_constant_sky(got); checks.check_constant_sky(checks.as_read_back(forward))
    print("%s: totals at %.3g of their bound, entries differing %s" % (case.name, share, figures))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_float32_cdfs_sample_what_the_pdf_claims(case):
    """sum |P32 - P_cell| <= (W + H) 2^-24 for the reference's own float32 CDFs, in both orders."""
    _, forward, spans, plain = _tables(case)
    for t in (forward, spans):
        share, unreachable = checks.check_sampled_is_claimed(checks.as_read_back(t), plain.p_cell)
        print("%s: sampled against claimed at %.3g of the bound, unreachable mass %.3g" % (case.name, share, unreachable))


def test_walking_from_inclusive_minus_sum_loses_the_prefix():
    """Why the kernels take a span's starting prefix from the scan's entry of the thread before, not from `inclusive - sum`: in the dynamic-range
    sky a span's own sum can be 2^53 times what lies in front of it, the difference keeps no correct digit, and the float32 CDF of such a row
    steps back at the span's first entry. The scan as it is now is monotone on the same rows."""
    from sky_cases import BY_NAME
    _, forward, _, _ = _tables(BY_NAME["dynamic_range_513x300"])
    old_prefix, old_total = ref.scan_spans(forward.weight, subtracting=True)
    old = ref.cdf32_from_scan(old_prefix, old_total)
    new_prefix, new_total = ref.scan_spans(forward.weight)
    assert np.array_equal(old_total, new_total)
    assert (np.diff(old, axis=1) < 0).sum() > 100
    assert (np.diff(ref.cdf32_from_scan(new_prefix, new_total), axis=1) < 0).sum() == 0


def test_span_scan_is_a_scan():
    """scan_spans against exact integer sums at every size class (integers below 2^53 add exactly in any order)."""
    rng = np.random.default_rng(1)
    for n in (1, 2, 255, 256, 257, 511, 512, 513, 1027, 2048):
        w = rng.integers(0, 1000, (3, n)).astype(np.float64)
        prefix, total = ref.scan_spans(w)
        assert np.array_equal(prefix, np.cumsum(w, axis=1)) and np.array_equal(total, w.sum(axis=1))
        assert ref.per_thread(n) == -(-n // 256)


def test_luminance32_is_unfused_float32():
    rng = np.random.default_rng(2)
    s = rng.uniform(0, 10, (1000, 3)).astype(np.float32)
    want = ((np.float32(0.299) * s[:, 0]).astype(np.float32) + (np.float32(0.587) * s[:, 1]).astype(np.float32)).astype(np.float32) + (np.float32(0.114) * s[:, 2]).astype(np.float32)
    got = ref.luminance32(s)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    # and it is not the float64 expression rounded once
    assert not np.array_equal(got, ref.luminance(s).astype(np.float32))


def test_invert_tables_matches_the_existing_inversion():
    sky = ref.sun_sky(64, 32, (20, 9))
    t = ref.Tables(sky)
    rng = np.random.default_rng(3)
    uv = rng.random((5000, 2), dtype=np.float32)
    want, row, col, _ = t.invert(uv)
    r, fy, c, fx = ref.invert_tables(t.marginal, t.conditional, uv)
    assert np.array_equal(r, row) and np.array_equal(c, col)
    assert np.array_equal(ref.direction_of(t.h, t.w, r, fy, c, fx), want)
