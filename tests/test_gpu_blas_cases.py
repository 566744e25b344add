"""GPU part of the device BLAS build's own tests (see tests/test_blas.py for the CPU part): the eleven kernels, the library sort and
the scans of gpu-raytracer_amd/csrc/kernels_blas.hip on the cases of tests/blas_cases.py, through the C ABI alone
(rt_set_build_boxes, rt_build_geometry, rt_read_geometry, rt_build_tlas, rt_trace_rays) on one raw context.

Per case: node count, node bytes and out_triangle_positions are those of the float32 restatement (tests/blas_reference.py), byte for
byte but for the sign of a zero node origin; the triangles read back are the input records gathered by the inverse of the positions;
the float64 rules hold on the device's own bytes; rays through the built trees (one identity instance per mesh that has
triangles) keep the float64 rules of tests/trace_checks.py against the brute force over the case's triangles.

What the MI355X showed: all 35 cases byte-identical to the restatement (zero signs of origins apart); containment at most 0.993 of
the slack (soup_20000), overhang at most 0.9999 of a grid step; far_grid_line before kernel_blas_nodes kept a thickness: bytes equal to
the restatement without the rule, the floor's child on grid lines 64 / 64 in y, both rays down at the floor missed -- with the rule both
hit; the whole file takes 4.4 s, the longest case (20 000 triangles) 0.7 s."""
import ctypes

import numpy as np
import pytest

import blas_cases
import blas_reference
import trace_checks
from test_blas import leaf_order, reserved_of, restated

pytestmark = pytest.mark.gpu


class BareContext:
    """One raw context; what it holds is the last case built."""

    def __init__(self, grt):
        P, Z = ctypes.c_void_p, ctypes.c_size_t
        self.grt = grt
        self.lib = lib = grt.device_lib()
        lib.rt_build_geometry.argtypes = [P, P, Z, P, Z, Z, P, P, P, P]
        lib.rt_set_build_boxes.argtypes = [P, P, Z, Z]
        lib.rt_read_geometry.argtypes = [P, P, P]
        lib.rt_build_tlas.argtypes = [P, P, P, P, P, P, P, Z]
        self.ctx = P()
        assert lib.rt_create(0, ctypes.byref(self.ctx)) == 0, lib.rt_last_error(None)

    def error(self):
        return self.lib.rt_last_error(self.ctx)

    def set_boxes(self, given):
        first, boxes = given
        boxes = np.ascontiguousarray(boxes, np.float32)
        assert self.lib.rt_set_build_boxes(self.ctx, boxes.ctypes.data, first, len(boxes)) == 0, self.error()

    def build_raw(self, records, mesh_first, mesh_count, triangle_count, reserved):
        """rt_build_geometry as given; returns (status, roots, positions, node count)."""
        records = np.ascontiguousarray(records, np.float32); mesh_first = np.ascontiguousarray(mesh_first, np.int32)
        roots = np.full(max(mesh_count, 1), -1, np.int32); position = np.full(max(triangle_count, 1), -1, np.int32); count = ctypes.c_size_t(0)
        status = self.lib.rt_build_geometry(self.ctx, records.ctypes.data, triangle_count, mesh_first.ctypes.data, mesh_count, reserved, roots.ctypes.data,
                                            position.ctypes.data, ctypes.byref(count), None)
        return status, roots, position, count.value

    def build(self, case, with_boxes=True):
        """Builds a case; returns (nodes, triangles in leaf order, positions)."""
        T, M = len(case.records), len(case.mesh_first) - 1
        if with_boxes and case.given is not None:
            self.set_boxes(case.given)
        status, roots, position, count = self.build_raw(case.records, case.mesh_first, M, T, reserved_of(case))
        assert status == 0, self.error()
        assert np.array_equal(roots, reserved_of(case) + np.arange(M))
        return self.read(count, T) + (position,)

    def read(self, node_count, triangle_count):
        nodes = np.zeros((node_count, 80), np.uint8); triangles = np.zeros((triangle_count, 24), np.float32)
        assert self.lib.rt_read_geometry(self.ctx, triangles.ctypes.data, nodes.ctypes.data) == 0, self.error()
        return nodes, triangles

    def instance_the_meshes(self, case, built, triangles):
        """One identity instance per mesh that has triangles, its box the mesh's."""
        meshes = np.nonzero(np.diff(case.mesh_first) > 0)[0]
        n = len(meshes)
        roots = (reserved_of(case) + meshes).astype(np.int32); materials = np.zeros(n, np.int32)
        identity = np.ascontiguousarray(np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (n, 1)))
        boxes = np.ascontiguousarray(np.concatenate([built.mesh_lo[meshes], built.mesh_hi[meshes]], axis=1), np.float32)
        assert self.lib.rt_build_tlas(self.ctx, roots.ctypes.data, materials.ctypes.data, identity.ctypes.data, identity.ctypes.data, identity.ctypes.data,
                                      boxes.ctypes.data, n) == 0, self.error()
        self.arrays = {"triangles": triangles, "mesh_transforms": identity}

    def array(self, name):            # what trace_checks.check_closest asks a path tracer for
        return self.arrays[name]

    def trace(self, origin, direction):
        return self.grt.trace_rays(self.ctx, origin, direction)[0]


@pytest.fixture(scope="module")
def bare(grt):
    context = BareContext(grt)
    yield context
    context.lib.rt_destroy(context.ctx)


def assert_same_build(case, built, nodes, position, triangles):
    blas_reference.same_bytes(case.name, nodes, built.nodes)
    assert np.array_equal(position, built.position), "%s: out_triangle_positions differ from the restatement, first at triangle %d" % (
        case.name, int(np.argmax(position != built.position)))
    assert triangles[position].tobytes() == case.records.tobytes(), "%s: the triangles read back are not the input gathered by the inverse of the positions" % case.name


@pytest.mark.parametrize("name", blas_cases.names())
def test_kernels_on_the_boundary_wide_level_many_mesh_and_degenerate_cases(grt, bare, name):
    case = blas_cases.by_name(name)
    built = restated(case)                                  # (premise asserted before anything is launched)
    M = len(case.mesh_first) - 1
    nodes, triangles, position = bare.build(case)
    assert_same_build(case, built, nodes, position, triangles)
    _, pieces, has = leaf_order(case, position)
    found = blas_reference.check(nodes, reserved_of(case), M, triangles, pieces, has)
    print("%s: %d nodes, widest level %d, containment %.3f of the slack, overhang %.4f grid steps, %d of %d child boxes widened" % (
        name, len(nodes) - reserved_of(case), max(built.level_widths), found.containment_in_slacks, found.overhang_in_steps, found.widened, found.children))
    if not case.traced:
        return
    origin, direction, bf = blas_cases.brute_force(case)
    bare.instance_the_meshes(case, built, triangles)
    hits = bare.trace(origin, direction)
    # a hit names its triangle by leaf-order place; the brute force went over the input order
    trace_checks.check_closest(name, case, bare, origin, direction, hits, bf)
    hit = hits[:, 1] != 0xffffffff
    print("%s: %d rays, %.1f %% hit, %.1f %% robust" % (name, len(hit), 100 * hit.mean(), 100 * trace_checks.ref.robust_closest(bf).mean()))
    if case.down is not None:
        which, _ = case.down
        assert hit[:len(which)].all(), "%s: %d of %d rays straight down miss the floor" % (name, int((~hit[:len(which)]).sum()), len(which))
        assert np.array_equal(hits[:len(which), 1].astype(np.int64), position[2 + which])


def test_refused_builds_change_nothing_and_a_later_build_owes_nothing_to_an_earlier_one(grt, bare):
    """Once for the file. (a) rt_build_geometry refuses a mesh_first_triangle that does not run from 0 to the triangle count or that
    decreases, no meshes and no triangles: non-zero, a message that names the rule, and what rt_read_geometry and a set of rays give
    afterwards is what they gave before. (b) Boxes set before a refused build are gone with it: the plain build that follows is
    that of no boxes. (c) 33 triangles built after 20 000 on the same context give the 33-triangle case's bytes."""
    small, large = blas_cases.by_name("leaf_33"), blas_cases.by_name("soup_20000")
    built = restated(small)
    nodes, triangles, position = bare.build(small)
    assert_same_build(small, built, nodes, position, triangles)
    origin, direction, _ = blas_cases.brute_force(small)
    bare.instance_the_meshes(small, built, triangles)
    hits = bare.trace(origin, direction)
    assert (hits[:, 1] != 0xffffffff).mean() > 0.3
    before = bare.read(len(nodes), 33)                      # (the TLAS has moved into the reserved slots by now)
    records, T = small.records, 33
    boxes = np.tile(np.array([[-0.05, -0.05, -0.05, 0.05, 0.05, 0.05]], np.float32), (8, 1))
    assert not np.array_equal(blas_reference.build(records, small.mesh_first, reserved_of(small), given=(4, boxes)).nodes, built.nodes)   # boxes that would show
    refusals = [(np.array([0, 32]), 1, T, b"from 0 to triangle_count"), (np.array([1, 33]), 1, T, b"from 0 to triangle_count"),
                (np.array([0, 20, 10, 33]), 3, T, b"must not decrease"), (np.array([0, 33]), 0, T, b"at least one"), (np.array([0, 0]), 1, 0, b"at least one")]
    for mesh_first, mesh_count, triangle_count, rule in refusals:
        bare.set_boxes((4, boxes))
        status, _, _, _ = bare.build_raw(records, mesh_first, mesh_count, triangle_count, reserved_of(small))
        assert status != 0 and rule in bare.error(), (mesh_first.tolist(), status, bare.error())
        after = bare.read(len(nodes), 33)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(bare.trace(origin, direction), hits)
    nodes, triangles, position = bare.build(small)          # (b): the boxes set before the last refusal are not pending
    assert_same_build(small, built, nodes, position, triangles)
    nodes, triangles, position = bare.build(large)          # (c)
    assert_same_build(large, restated(large), nodes, position, triangles)
    nodes, triangles, position = bare.build(small)
    assert_same_build(small, built, nodes, position, triangles)
