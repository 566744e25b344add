"""The device BLAS build (gpu-raytracer_amd/csrc/kernels_blas.hip), CPU part: the float32 restatement of the build
(tests/blas_reference.py) on every case of tests/blas_cases.py keeps the float64 rules a BLAS has to keep (structure, containment
within a derived slack, thickness, tightness, exponents exactly), the premises of the cases hold, the rays of the traced cases are
worth tracing (at least 30 % hit and 30 % robust against the float64 brute force), and vertices that are not finite end the build
within its level limit with every triangle in one leaf. The GPU part (tests/test_gpu_blas_cases.py) holds the kernels to the
restatement's bytes and to the same rules.

Measured on the restatement (the device's bytes are the same): containment at most 0.993 of the slack (soup_20000; 0.87 - 0.99 for
the soups of 63 and more triangles and the one-triangle meshes, 0.15 for the copies); the largest overhang 0.9999 of a grid step;
child boxes the thickness rule widened: far_grid_line 1 of 2 (before the rule went into kernel_blas_nodes that box had
q_lo == q_hi == 64 in y and both rays straight down at the floor missed on the device), elsewhere none."""
import numpy as np
import pytest

import blas_cases
import blas_reference
import trace_reference

_built = {}


def rebuild(case, **changes):
    arguments = dict(given=case.given); arguments.update(changes)
    return blas_reference.build(case.records, case.mesh_first, reserved_of(case), **arguments)


def reserved_of(case):
    """Node slots kept free in front: room for the TLAS of one instance per mesh."""
    return 2 * (len(case.mesh_first) - 1)


def restated(case):
    """The restatement's build of a case, computed once, premise asserted, left unchanged."""
    if case.name not in _built:
        built = rebuild(case)
        blas_cases.assert_premise(case, built, rebuild)
        _built[case.name] = built
    return _built[case.name]


def leaf_order(case, position):
    """(records, pieces, has_piece) in leaf order: what rt_read_geometry returns for a build that placed input i at position[i]."""
    T = len(case.records)
    order = np.empty(T, np.int64); order[np.asarray(position, np.int64)] = np.arange(T)
    pieces, has = blas_reference.pieces_of(T, case.given)
    return case.records[order], pieces[order], has[order]


@pytest.mark.parametrize("name", blas_cases.names())
def test_restatement_keeps_the_float64_rules_on_every_case(name):
    case = blas_cases.by_name(name)
    built = restated(case)
    M = len(case.mesh_first) - 1
    assert sorted(built.position.tolist()) == list(range(len(case.records)))
    triangles, pieces, has = leaf_order(case, built.position)
    found = blas_reference.check(built.nodes, reserved_of(case), M, triangles, pieces, has)
    assert blas_reference.level_widths(built.nodes, reserved_of(case), M) == built.level_widths
    print("%s: %d nodes, level widths %r, containment %.3f of the slack, overhang %.4f grid steps, %d of %d child boxes widened" % (
        name, len(built.nodes) - reserved_of(case), built.level_widths, found.containment_in_slacks, found.overhang_in_steps, found.widened, found.children))
    assert (found.widened > 0) == (name == "far_grid_line")


@pytest.mark.parametrize("name", blas_cases.names())
def test_thickness_rule_changes_only_child_boxes_whose_bounds_coincide(name):
    """The node kernel before and after tlas_keep_thickness went into it, restated: the same node count and positions, and bytes that
    differ only in the quantised bounds of (node, slot, axis) triples that had q_lo == q_hi -- none but far_grid_line's floor."""
    case = blas_cases.by_name(name)
    after, before = restated(case), rebuild(case, keep_thickness=False)
    assert len(after.nodes) == len(before.nodes) and np.array_equal(after.position, before.position)
    a, b = np.asarray(after.nodes), np.asarray(before.nodes)
    assert np.array_equal(a[:, :32], b[:, :32])
    qa, qb = a[:, 32:].reshape(-1, 3, 2, 8), b[:, 32:].reshape(-1, 3, 2, 8)
    changed = (qa != qb).any(axis=2)                               # (node, axis, slot)
    flat = (qb[:, :, 0] == qb[:, :, 1]) & (b[:, None, 24:32] != 0)
    assert np.array_equal(changed, flat) and bool(flat.any()) == (name == "far_grid_line")
    assert ((qa[:, :, 1].astype(int) - qa[:, :, 0].astype(int))[flat] == 1).all()


def test_case_list_covers_the_launch_shapes():
    """Over all cases: a level wider than a workgroup of kernel_blas_runs, and level widths that are no multiple of the 32 nodes
    a workgroup of kernel_blas_nodes holds -- below 32, between 32 and 256, and above."""
    widths = sorted({w for c in blas_cases.cases() for w in restated(c).level_widths})
    ragged = [w for w in widths if w % 32]
    print("level widths over all cases: %r" % widths)
    assert max(widths) > 256 and any(w < 32 for w in ragged) and any(32 < w < 256 for w in ragged) and any(w > 256 for w in ragged)


@pytest.mark.parametrize("name", [c.name for c in blas_cases.cases() if c.traced])
def test_rays_of_the_traced_cases_are_worth_tracing(name):
    case = blas_cases.by_name(name)
    origin, direction, bf = blas_cases.brute_force(case)
    hit, robust = np.isfinite(bf.t).mean(), trace_reference.robust_closest(bf).mean()
    print("%s: %d rays, %.1f %% hit, %.1f %% robust (%s)" % (name, origin.shape[1], 100 * hit, 100 * robust, case.traced))
    if case.traced == "floor":
        assert hit >= 0.3 and robust >= 0.3, (name, hit, robust)
    else:
        assert case.why
    if case.down is not None:
        which, _ = case.down
        assert np.array_equal(bf.index[:len(which)], 2 + which) and trace_reference.robust_closest(bf)[:len(which)].all()


NOT_FINITE = [("nan_vertex", np.nan, 1), ("inf_vertex", np.inf, 1), ("minus_inf_vertices", -np.inf, 7), ("all_nan", np.nan, 0)]


@pytest.mark.parametrize("name,value,every", NOT_FINITE)
def test_vertices_that_are_not_finite_end_the_build(name, value, every):
    """CPU only (a test on a shared GPU must not depend on a loop ending): 300 triangles of which one, every seventh or all have a
    vertex coordinate that is NaN or infinite. The restated build ends within the level limit, numbers every node and puts every
    triangle into exactly one leaf."""
    records = blas_cases.records_of(blas_cases.soup(77, 300, 0.2))
    if every == 0:
        records[:, 0:9] = value
    elif every == 1:
        records[123, 1] = value
    else:
        records[::every, 4] = value
    built = blas_reference.build(records, np.array([0, 300]), 2)
    assert built.levels <= blas_reference.LEVEL_LIMIT
    blas_reference.structure(built.nodes, 2, 1, 300)
    assert sorted(built.position.tolist()) == list(range(300))
