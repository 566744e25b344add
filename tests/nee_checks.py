"""The comparisons test_nee.py (oracle, CPU) and test_gpu_nee.py (device) share for light selection (rt_sample_lights /
oracle_sample_lights against nee_reference.py).

What is exact, and why
    * entry, transform id, triangle index: comparisons of float32 numbers only -- no tolerance, no exception list.
    * device against oracle, every field: bit-identical, NaN equal to NaN. The path uses +, -, *, /, sqrtf and comparisons, both
      sides build with -ffp-contract=off. Derived, not measured.
    * LDS launch against global launch: the same floats read from another memory -- bit-identical.

Bounds against float64 (measured on the ORACLE against nee_reference.py on the CPU, over every case of nee_cases.CPU_CASES, edge and
stratified probes; bound = 3 x the worst case; the device is held to the same numbers, and being bit-identical to the oracle it
measures the same):
    * point:    |error|_inf / (1 + |point|_2)   measured 8.0e-8 (few, stratified probes)           bound POINT_TOL  = 2.4e-7
      (two multiply-adds of the barycentric sum and three of the transform: a few float32 ulp, 6e-8 each, of the largest term)
    * normal:   |error|_inf                     measured 1.46e-7 (limit, a rotated ribbon)         bound NORMAL_TOL = 4.4e-7
      (cross product of two edges, a 3 x 3 product and a normalisation)
    * emission: copied from the material table: exact.
    A zero-area triangle has a NaN normal on both sides (0 / 0 in normalize); it must be NaN in exactly the same probes.

Goodness of fit: (chi2 - dof) / sqrt(2 dof) < 5 with cells expected below 5 pooled into one, as test_gpu_sky_sampling.py does; a cell
of probability 0 (the zero-area triangle) must stay empty.
"""
import math

import numpy as np

import nee_reference as ref

POINT_TOL, NORMAL_TOL = 2.4e-7, 4.4e-7


def ids_of(out):
    """entry, transform id, triangle, path flag of (N, 16) float32 records."""
    return np.ascontiguousarray(out[:, :4]).view(np.int32)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check_identical(name, got, want, what, columns=slice(0, 13)):
    """Every field of `columns` bit-identical (NaN equal to NaN) on every probe."""
    same = same_bits(got[:, columns], want[:, columns]).all(1)
    bad = np.nonzero(~same)[0]
    assert bad.size == 0, "%s: %d of %d probes differ from %s, first %d: %s vs %s" % (
        name, bad.size, got.shape[0], what, bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


def check_selection(name, got, want):
    """Entry, transform id and triangle equal the float64 reference's (searchsorted) on every probe."""
    ids = ids_of(got)
    for k, field in enumerate(("entry", "transform_id", "triangle")):
        bad = np.nonzero(ids[:, k] != getattr(want, field))[0]
        assert bad.size == 0, "%s: %s differs from searchsorted on %d of %d probes, first %d: %d vs %d" % (
            name, field, bad.size, ids.shape[0], bad[0], ids[bad[0], k], getattr(want, field)[bad[0]])


def compare_with_reference(name, got, want):
    """Point, normal and emission against float64 at the bounds of the docstring. Returns the worst errors."""
    check_selection(name, got, want)
    point = np.abs(got[:, 4:7] - want.point).max(1) / (1.0 + np.linalg.norm(want.point, axis=1))
    nan_ref = np.isnan(want.normal).any(1); nan_got = np.isnan(got[:, 7:10]).any(1)
    assert np.array_equal(nan_ref, nan_got), "%s: NaN normals in %d probes, the reference has %d" % (name, nan_got.sum(), nan_ref.sum())
    normal = np.abs(got[~nan_ref, 7:10] - want.normal[~nan_ref]).max(1) if (~nan_ref).any() else np.zeros(1)
    assert np.array_equal(got[:, 10:13].astype(np.float64), want.emission), "%s: emission differs from the material table" % name
    worst = {"point": float(point.max()), "normal": float(normal.max()), "nan_normals": int(nan_ref.sum())}
    print("%s: %d probes, worst point %.3g (bound %.3g), normal %.3g (bound %.3g), %d NaN normals (zero-area triangle)" % (
        name, got.shape[0], worst["point"], POINT_TOL, worst["normal"], NORMAL_TOL, worst["nan_normals"]))
    assert worst["point"] <= POINT_TOL and worst["normal"] <= NORMAL_TOL, (name, worst)
    return worst


def chi2_score(counts, expected):
    """(chi2 - dof) / sqrt(2 dof) of observed counts against expected ones, cells expected below 5 pooled; cells expected 0 must be empty."""
    counts = np.asarray(counts, np.float64); expected = np.asarray(expected, np.float64)
    assert counts[expected == 0].sum() == 0, "samples in a cell of probability 0"
    big = expected >= 5
    obs = np.append(counts[big], counts[~big].sum()); exp = np.append(expected[big], expected[~big].sum())
    keep = exp > 0
    chi2 = float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum())
    dof = int(keep.sum()) - 1
    return (chi2 - dof) / math.sqrt(2 * dof), chi2, dof


def check_selection_distribution(name, got, tables, joint):
    """Uniform probes' selections against the exact probabilities of the geometry: binned by (entry, slot) if `joint`, else by
    entry and by triangle slot (summed over entries of one span) separately."""
    ids = ids_of(got)
    n = ids.shape[0]
    mesh_p, slot_p, _ = ref.exact_probabilities(tables)
    entry = ids[:, 0].astype(np.int64)
    first = tables.spans[entry, 0].astype(np.int64)
    lookup = np.full(int(tables.triangle_indices.max()) + 1, -1, np.int64)
    slot = np.empty(n, np.int64)
    for f in np.unique(first):
        last = int(tables.spans[tables.spans[:, 0] == f][0, 1])
        lookup[:] = -1
        lookup[tables.triangle_indices[f:last + 1]] = np.arange(last + 1 - f)
        sel = first == f
        slot[sel] = lookup[ids[sel, 2]]
    assert (slot >= 0).all(), "%s: a triangle outside the selected entry's span" % name
    scores = {}
    if joint:
        offsets = np.concatenate([[0], np.cumsum([p.size for p in slot_p])])
        counts = np.bincount(offsets[entry] + slot, minlength=offsets[-1])
        expected = n * np.concatenate([mesh_p[m] * slot_p[m] for m in range(mesh_p.size)])
        scores["entry x triangle"] = chi2_score(counts, expected)
    else:
        scores["entry"] = chi2_score(np.bincount(entry, minlength=mesh_p.size), n * mesh_p)
        spans = np.unique(tables.spans, axis=0)
        assert spans.shape[0] == 1, "separate binning expects the instances of one mesh data"
        scores["triangle"] = chi2_score(np.bincount(slot, minlength=slot_p[0].size), n * slot_p[0])
    for what, (score, chi2, dof) in scores.items():
        print("%s: chi2 by %s: %.1f at %d degrees of freedom, score %.2f" % (name, what, chi2, dof, score))
        assert score < 5.0, (name, what, chi2, dof)
    return scores


def check_barycentrics(name, got, probes, tables, entry):
    """The points selected on light-mesh entry `entry`'s largest triangle, taken back to barycentrics in float64 and binned 4 x 4:
    cells wholly inside the triangle hold 1/8 of them, the four cut by the hypotenuse 1/16, the rest nothing."""
    ids = ids_of(got)
    first, last = tables.spans[entry]
    tri = tables.triangles[tables.triangle_indices[first:last + 1]].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 3:6], tri[:, 6:9]), axis=1)
    triangle = int(tables.triangle_indices[first + int(area.argmax())])
    sel = (ids[:, 0] == entry) & (ids[:, 2] == triangle)
    t = tables.triangles[triangle].astype(np.float64)
    m = tables.transforms[tables.transform_indices[entry]].astype(np.float64)
    basis = np.stack([m[:, :3] @ t[3:6], m[:, :3] @ t[6:9]], 1)                      # world-space edges
    origin = m[:, :3] @ t[0:3] + m[:, 3]
    uv = np.linalg.lstsq(basis, (got[sel, 4:7].astype(np.float64) - origin).T, rcond=None)[0].T
    want = np.stack(ref.sample_triangle(probes[sel, 2].astype(np.float64), probes[sel, 3].astype(np.float64)), 1)
    assert np.abs(uv - want).max() < 1e-5, (name, float(np.abs(uv - want).max()))      # the fold itself, per probe
    i = np.clip(np.floor(4 * uv[:, 0]).astype(int), 0, 3); j = np.clip(np.floor(4 * uv[:, 1]).astype(int), 0, 3)
    counts = np.bincount(4 * i + j, minlength=16)
    expected = np.array([[1 / 8 if a + b <= 2 else 1 / 16 if a + b == 3 else 0 for b in range(4)] for a in range(4)]).ravel() * sel.sum()
    score, chi2, dof = chi2_score(counts, expected)
    print("%s: %d points on triangle %d, chi2 of the 4 x 4 barycentric cells %.1f at %d degrees of freedom, score %.2f" % (name, sel.sum(), triangle, chi2, dof, score))
    assert sel.sum() > 10000 and score < 5.0, (name, int(sel.sum()), chi2, dof)


def refused_tables(tables):
    """One set of light tables per rule of rt_upload_lights, each a copy of the valid `tables` with one thing wrong:
    (rule, words the message must hold, triangle_indices, triangle_cdf, mesh_cdf, spans, transform_indices, total_weight)."""
    good = (tables.triangle_indices.copy(), tables.triangle_cdf.copy(), tables.mesh_cdf.copy(), tables.spans.copy(), tables.transform_indices.copy(), tables.total_weight)
    first, last = (int(v) for v in tables.spans[0])
    assert last > first and tables.mesh_cdf.size >= 2
    out = []

    def case(rule, words, change):
        t = [a.copy() if isinstance(a, np.ndarray) else a for a in good]
        change(t)
        out.append((rule, words) + tuple(t))

    def put(index, position, value):
        def change(t):
            t[index][position] = value
        return change

    def weight(value):
        def change(t):
            t[5] = value
        return change

    below_one = np.float32(0.9999)
    case("NaN in the mesh table", "NaN", put(2, 0, np.nan))
    case("the mesh table decreases", "below entry", put(2, 1, tables.mesh_cdf[0] / 2))
    case("the mesh table ends below 1", "below 1", put(2, -1, below_one))
    case("NaN in a named span", "NaN", put(1, first, np.nan))
    case("a named span decreases", "below entry", put(1, last - 1, np.float32(2.0)))
    case("a named span ends below 1", "below 1", put(1, last, below_one))
    case("a span starts below 0", "span", put(3, (0, 0), -1))
    case("a span ends past the triangle table", "span", put(3, (0, 1), tables.triangle_cdf.size))
    case("a span with first > last", "span", put(3, (0, 0), last + 1))
    case("a total weight of NaN", "lights_total_weight", weight(float("nan")))
    case("an infinite total weight", "lights_total_weight", weight(float("inf")))
    case("a negative total weight", "lights_total_weight", weight(-1.0))
    case("a total weight of 0 with light meshes", "lights_total_weight", weight(0.0))
    return out
