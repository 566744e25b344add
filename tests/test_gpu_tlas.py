"""GPU part of the device TLAS build (see tests/test_tlas.py for the CPU part): the kernel reproduces the bytes of its
one-thread restatement; rays traced through the device-built TLAS hit what they hit through the host-built one; frames
rendered with it match the oracle, also while instances move and several frames are in flight.

The cases of tests/tlas_cases.py (launch-shape boundaries 1 .. 4 096, levels wider than the workgroup, degenerate placement, flat
child boxes, signed zeros) go through rt_build_tlas on one raw context and come back through rt_read_tlas and rt_read_instances:
bytes against the restatement, the float64 rules of tests/tlas_reference.py on the device's bytes, the gathered tables exactly, and
rays against the float64 brute force under the rules of tests/trace_checks.py. What the MI355X showed:
  * byte-identical to the restatement on all 35 cases, the wide levels included: 512 nodes (coincident_1024) and 333 (ragged_1000)
    under 256 threads, 1 792 (comb_3613) under 1 024 -- the chunked numbering scan of step 3b with full and ragged later chunks;
  * signed zeros: before node origins were canonicalised, signed_zeros_64 differed from the restatement in 7 words, all of them
    the sign bit of a zero origin (the lanes of the shuffle union and the serial union keep different zeros); both now write +0.0
    and the comparison is as strict as for every other case;
  * the largest containment error is 0.46 of the derived slack (uniform_2049); no case exceeds 0.5;
  * child boxes the thickness rule widened: points_300 372 of 372, plane_2049 2 619 of 2 619, scales_900 29 of 1 195, flat_tiles_200
    202 of 264, flat_small_200 183 of 266, flat_planes_8 2 of 8; elsewhere none. Every flat instance of the three flat cases is hit
    by the ray down its normal (200, 200 and 2 rays). With the widening alone 6 and 10 of the 200 were still lost (node test of
    kernels_trace.hip restated in float32 on the restatement's nodes): their nodes hold coplanar children, had no extent and
    therefore a grid of 1e-32 steps, which is why a node's grid now has a least extent (rt_tlas_build.h)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import tlas_cases
import tlas_reference
import trace_checks
from conftest import make_pathtracer
from test_tlas import assert_premise, check_tlas, instanced_scene_file, world_boxes_of

pytestmark = pytest.mark.gpu

REL_L1_TOL = 1e-4


def read_tlas(grt, pt, n):
    lib = grt.device_lib()
    lib.rt_read_tlas.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    order = np.zeros(n, np.int32); nodes = np.zeros((2 * n, 80), np.uint8); count = ctypes.c_int32(0)
    assert lib.rt_read_tlas(pt.ctx, order.ctypes.data, nodes.ctypes.data, 2 * n, ctypes.byref(count)) == 0, lib.rt_last_error(pt.ctx)
    return nodes[:count.value], order


@pytest.mark.reference_layout
@pytest.mark.parametrize("count", [1, 5, 60, 1500])
def test_device_tlas_equals_its_restatement_and_traces_like_the_host_tlas(grt, oracle, tmp_path, count):
    path = instanced_scene_file(str(tmp_path / "s"), count=count)
    w, h = 160, 100
    hits, orders = {}, {}
    for device_tlas in (1, 0):
        grt.config_reset(); grt.config_set(device_tlas=device_tlas, num_bounces=3)
        scene = grt.Scene(path)
        pt = grt.Pathtracer(scene, w, h, device=0); pt.update()
        n = scene.mesh_count
        if device_tlas:
            nodes, order = read_tlas(grt, pt, n)
            transforms = pt.array("scene_order_transforms").reshape(-1, 12).copy(); boxes = pt.array("scene_order_boxes").reshape(-1, 6).copy()
            want_nodes, want_order = oracle.tlas_build(transforms, boxes)
            assert np.array_equal(order, want_order) and np.array_equal(nodes, want_nodes)       # byte for byte
            check_tlas(nodes, order, world_boxes_of(transforms, boxes))
            orders[1] = order
        else:
            orders[0] = pt.array("tlas_indices").copy()
        view = oracle.SceneView(pt)
        o, d, _ = view.generate(0, 0, w * h)
        rng = np.random.default_rng(7)
        extra_o = rng.uniform(-14, 14, (3, 20000)).astype(np.float32); extra_d = rng.normal(size=(3, 20000)).astype(np.float32); extra_d /= np.linalg.norm(extra_d, axis=0)
        o = np.concatenate([o, extra_o], axis=1); d = np.concatenate([d, extra_d], axis=1)
        hits[device_tlas], _ = grt.trace_rays(pt.ctx, o, d)
        if device_tlas:   # the oracle walks the very nodes the device built (host view of the device TLAS): bit-exact, instance ids included
            want, _ = view.trace(o, d)
            assert np.array_equal(hits[1], want)
        pt.close(); scene.close()
    hit = hits[0][:, 1] != 0xffffffff
    assert hit.mean() > 0.3 and np.array_equal(hits[0][:, 1:], hits[1][:, 1:])
    assert np.array_equal(orders[0][hits[0][hit, 0].astype(np.int64)], orders[1][hits[1][hit, 0].astype(np.int64)])
    grt.config_reset()


def test_frames_with_a_device_tlas_match_the_oracle_while_instances_move(grt, oracle, tmp_path):
    """enable_scene_update: every frame the instances move and Integrator::build_tlas runs -- on the device (device_tlas = 1;
    the default -1 picks it for such scenes from 1024 instances on). (a) each frame against the oracle, which reads the device-built TLAS back; the light tables
    name instances by scene index and the device maps them; (b) six frames accumulated with 1 and with 3 frames in flight
    (slot scheduler: every chain reads the TLAS version it was submitted with) are bit-identical."""
    path = instanced_scene_file(str(tmp_path / "s"), count=40)
    w, h = 200, 120
    lib = grt.device_lib()

    def move(scene, base, frame):
        for m in range(3, scene.mesh_count):
            pos, _, scale = base[m]
            a = 0.35 * frame + 0.2 * m
            scene.set_mesh_transform(m, [pos[0] + 0.6 * np.sin(a), pos[1], pos[2] + 0.6 * np.cos(a)], [0.0, float(np.sin(a / 2)), 0.0, float(np.cos(a / 2))], scale)

    grt.config_reset(); grt.config_set(num_bounces=3, enable_scene_update=1, device_tlas=1)
    scene = grt.Scene(path)
    base = [scene.mesh_transform(m) for m in range(scene.mesh_count)]
    pt = grt.Pathtracer(scene, w, h, device=0); pt.update()
    for frame in range(3):
        move(scene, base, frame); pt.update()
        lib.rt_render_sample.argtypes = [ctypes.c_void_p, ctypes.c_int]
        assert lib.rt_render_sample(pt.ctx, 0) == 0
        nodes, order = read_tlas(grt, pt, scene.mesh_count)                # built on the device: rt_read_tlas has something to read
        view = oracle.SceneView(pt); ref = oracle.Frame(view)
        oc = ref.render_sample(0); c = pt.counters()
        assert all(abs(a - b) <= 2 + 0.002 * b for a, b in zip(list(c.trace[:3]), list(oc.trace[:3]))), (list(c.trace[:3]), list(oc.trace[:3]))
        assert all(abs(a - b) <= 2 + 0.002 * b for a, b in zip(list(c.shadow[:3]), list(oc.shadow[:3])))
        got, want = pt.read_framebuffer()[:, :w, :3], ref.final[:, :w, :3]
        assert np.abs(got - want).sum() / want.sum() < REL_L1_TOL, frame
    pt.close(); scene.close()

    images = []
    for in_flight in (1, 3):
        grt.config_reset(); grt.config_set(num_bounces=3, enable_scene_update=1, device_tlas=1)
        scene = grt.Scene(path)
        pt = grt.Pathtracer(scene, w, h, device=0); pt.update()
        grt.set_samples_in_flight(pt.ctx, in_flight)
        for frame in range(40):      # more frames than the scene ring has versions (12)
            move(scene, base, frame); pt.update()
            assert lib.rt_render_sample(pt.ctx, frame) == 0
        images.append(pt.read_framebuffer().copy())
        pt.close(); scene.close()
    assert np.array_equal(images[0], images[1]) and images[0][..., :3].max() > 0.0
    grt.config_reset()


def test_merged_wavefront_on_a_scene_with_more_instances_than_its_lds_root_table(grt, tmp_path):
    """The fused traversal launch keeps the BLAS roots of up to 1 024 instances in LDS and fetches every node -- TLAS nodes
    included -- from the BLAS node array, into whose reserved slots the TLAS is copied. Beyond 1 024 instances the roots
    come from global memory: frames of a 1 203-instance scene (host TLAS and device TLAS) are bit-identical under the
    merged wavefront and under the per-submission chains, whose kernels read the TLAS from its own buffer."""
    import ctypes
    path = instanced_scene_file(str(tmp_path / "s"), count=1200)
    lib = grt.device_lib()
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    for device_tlas in (0, 1):
        images = []
        for scheduler in ("merged", "slots"):
            grt.config_reset(); grt.config_set(device_tlas=device_tlas, num_bounces=4)
            scene = grt.Scene(path)
            pt = grt.Pathtracer(scene, 160, 100, device=0); pt.update()
            assert scene.mesh_count > 1024
            grt.set_scheduler(pt.ctx, scheduler)
            for first in (0, 2, 4):
                assert lib.rt_render_samples(pt.ctx, first, 2) == 0
            images.append(pt.read_framebuffer().copy())
            pt.close(); scene.close()
        assert np.array_equal(images[0], images[1]) and images[0][..., :3].max() > 0, device_tlas
    grt.config_reset()


def test_device_tlas_switched_on_after_the_scene_was_flattened(grt, oracle, tmp_path):
    """A scene is staged with its static instances flattened (the default; here the whole scene: rays start inside node 0). Then
    device_tlas is switched on at run time: the TLAS the device builds has a leaf per scene instance and node 0 becomes its
    root -- the integrator has to stage the reference's layout again and rt_build_tlas has to move the ray entry back above the
    instances, or every ray would read TLAS leaves as triangles. Frames before and after against the oracle."""
    from test_gpu_parity import compare_frames
    path = instanced_scene_file(str(tmp_path / "s"), count=2)     # floor + two emitters + 2 blobs of one mesh: all five stand still, all are flattened
    grt.config_reset(); grt.config_set(num_bounces=4)
    scene = grt.Scene(path); grt.config_set(num_bounces=4)
    pt = grt.Pathtracer(scene, 160, 100, device=0); pt.update()
    assert pt.static_geometry_whole_scene and pt.static_geometry_members == scene.mesh_count
    compare_frames(grt, oracle, pt, 2, 160, 100)
    grt.config_set(device_tlas=1)
    pt.invalidate("scene"); pt.update()
    assert pt.static_geometry_members == 0 and not pt.static_geometry_whole_scene
    compare_frames(grt, oracle, pt, 2, 160, 100)
    position, rotation, scale = scene.mesh_transform(4)
    scene.set_mesh_transform(4, (position[0] + 1.0, position[1], position[2]), rotation, scale)
    pt.invalidate("scene"); pt.update()
    compare_frames(grt, oracle, pt, 2, 160, 100)
    pt.close(); scene.close(); grt.config_reset()


# ---- the kernel on the cases of tests/tlas_cases.py, through the C ABI alone ---------------------------------------------------

RESERVED_TLAS_NODES = 8192            # 2 x 4096: room for the largest TLAS one launch builds
RAYS = 1500                           # per traced case; half aimed at instances, half at random


class BareScene:
    """One raw context holding the two meshes of tlas_cases, each with a BLAS the device built."""

    def __init__(self, grt):
        P, Z = ctypes.c_void_p, ctypes.c_size_t
        self.lib = lib = grt.device_lib()
        lib.rt_build_geometry.argtypes = [P, P, Z, P, Z, Z, P, P, P, P]
        lib.rt_read_geometry.argtypes = [P, P, P]
        lib.rt_build_tlas.argtypes = [P, P, P, P, P, P, P, Z]
        lib.rt_read_tlas.argtypes = [P, P, P, Z, P]
        lib.rt_read_instances.argtypes = [P, P, P, P, P, P, P]
        lib.rt_read_instances.restype = ctypes.c_int
        self.ctx = P()
        assert lib.rt_create(0, ctypes.byref(self.ctx)) == 0, lib.rt_last_error(None)
        self.mesh_triangles = [tlas_cases.mesh_triangles(m) for m in (tlas_cases.CUBE, tlas_cases.SQUARE)]
        records, first = [], [0]
        for vertices in self.mesh_triangles:
            r = np.zeros((len(vertices), 24), np.float32)                       # position_0, edge_1, edge_2, normal_0, its edges, uv
            r[:, 0:3] = vertices[:, 0]; r[:, 3:6] = vertices[:, 1] - vertices[:, 0]; r[:, 6:9] = vertices[:, 2] - vertices[:, 0]
            normal = np.cross(r[:, 3:6], r[:, 6:9]); r[:, 9:12] = normal / np.linalg.norm(normal, axis=1, keepdims=True)
            records.append(r); first.append(first[-1] + len(vertices))
        records = np.ascontiguousarray(np.concatenate(records)); first = np.array(first, np.int32)
        self.roots = np.zeros(2, np.int32)
        node_count = ctypes.c_size_t(0)
        assert lib.rt_build_geometry(self.ctx, records.ctypes.data, len(records), first.ctypes.data, 2, RESERVED_TLAS_NODES, self.roots.ctypes.data, None,
                                     ctypes.byref(node_count), None) == 0, lib.rt_last_error(self.ctx)
        assert node_count.value >= RESERVED_TLAS_NODES + 2
        self.triangles = np.zeros((len(records), 24), np.float32)                # in the order the build stored them: what a hit's triangle id names
        assert lib.rt_read_geometry(self.ctx, self.triangles.ctypes.data, None) == 0, lib.rt_last_error(self.ctx)

    def tables(self, case):
        """The scene-order tables of a case: distinct numbers everywhere, so that a gather that takes a wrong row shows."""
        n = len(case.mesh)
        return (np.ascontiguousarray(self.roots[case.mesh]), (np.arange(n, dtype=np.int32) * 3 + 1), case.transforms.reshape(n, 12),
                case.transforms_inv.reshape(n, 12), np.ascontiguousarray(case.transforms.reshape(n, 12) + np.float32(1.0)))

    def build(self, case, count=None):
        roots, materials, transforms, inverse, previous = self.tables(case)
        n = len(case.mesh) if count is None else count
        return self.lib.rt_build_tlas(self.ctx, roots.ctypes.data, materials.ctypes.data, transforms.ctypes.data, inverse.ctypes.data, previous.ctypes.data,
                                      case.local_boxes.ctypes.data, n)

    def read(self, n):
        order = np.zeros(n, np.int32); nodes = np.zeros((2 * n, 80), np.uint8); count = ctypes.c_int32(0)
        assert self.lib.rt_read_tlas(self.ctx, order.ctypes.data, nodes.ctypes.data, 2 * n, ctypes.byref(count)) == 0, self.lib.rt_last_error(self.ctx)
        tables = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32), np.zeros(n, np.int32)]
        assert self.lib.rt_read_instances(self.ctx, *[t.ctypes.data for t in tables]) == 0, self.lib.rt_last_error(self.ctx)
        assert 1 <= count.value <= 2 * n
        return nodes[:count.value].copy(), order, tables

    def array(self, name):            # what trace_checks.check_closest asks a path tracer for
        return {"triangles": self.triangles, "mesh_transforms": self.tlas_order_transforms}[name]


@pytest.fixture(scope="module")
def bare_scene(grt):
    scene = BareScene(grt)
    yield scene
    scene.lib.rt_destroy(scene.ctx)


_restated = {}


def restated(oracle, case):
    """The restatement's nodes and order of a case, computed once and left unchanged."""
    if case.name not in _restated:
        nodes, order = oracle.tlas_build(case.transforms.reshape(-1, 12), case.local_boxes)
        assert_premise(case, nodes)                    # before anything is launched
        nodes.setflags(write=False); order.setflags(write=False)
        _restated[case.name] = (nodes, order)
    return _restated[case.name]


def assert_same_bytes(name, nodes, order, want_nodes, want_order):
    if len(nodes) == len(want_nodes) and not np.array_equal(nodes, want_nodes):     # say what differs before failing
        words, want_words = nodes.view(np.uint32).reshape(-1, 20), want_nodes.view(np.uint32).reshape(-1, 20)
        differ = np.argwhere(words != want_words)
        only_zero_signs = bool((differ[:, 1] < 3).all() and ((words ^ want_words)[words != want_words] == 0x80000000).all())
        print("%s: %d words differ from the restatement, first (node, word) %r, only signs of zero origins: %s" % (name, len(differ), differ[0].tolist(), only_zero_signs))
    assert len(nodes) == len(want_nodes) and np.array_equal(nodes, want_nodes) and np.array_equal(order, want_order), name


def rays_of(case, boxes64):
    """(3, RAYS) float32 origins and directions: rays from outside the scene box at the centres of instances, and random ones."""
    rng = np.random.default_rng(7919 * len(case.mesh) + 13)
    lo, hi = boxes64[:, 0].min(axis=0), boxes64[:, 1].max(axis=0)
    diagonal = max(float(np.linalg.norm(hi - lo)), 1e-3 * float(np.abs(boxes64).max()))
    n = len(case.mesh)
    rays = RAYS // 3 if case.name.startswith("coincident") else RAYS      # (every aimed ray meets every instance there: the brute force has no pair to leave out)
    aimed = rng.choice(n, min(n, rays // 2), replace=False)
    away = rng.normal(size=(len(aimed), 3)); away /= np.linalg.norm(away, axis=1, keepdims=True)
    target = 0.5 * (boxes64[aimed, 0] + boxes64[aimed, 1])
    loose = rays - len(aimed)
    anywhere = 0.5 * (lo + hi) + rng.uniform(-0.75, 0.75, (loose, 3)) * diagonal
    heading = rng.normal(size=(loose, 3)); heading /= np.linalg.norm(heading, axis=1, keepdims=True)
    origin = np.concatenate([target + 1.5 * diagonal * away, anywhere]); direction = np.concatenate([-away, heading]) + 0.0
    return np.ascontiguousarray(origin.T, np.float32), np.ascontiguousarray(direction.T, np.float32)


def rays_down_the_normals(case):
    """Per instance of case.aim a ray from half the instance's size above the aimed point, down the normal. Checked here in float64 on the
    float32 rays: each starts above its instance and meets it well inside the square's first triangle, at the distance returned with the rays."""
    instances, point, normal = case.aim
    size = np.linalg.norm(case.transforms[instances][:, :, 1].astype(np.float64), axis=1)
    origin = (point + 0.5 * size[:, None] * normal).astype(np.float32); direction = (-normal + 0.0).astype(np.float32)
    m = np.zeros((len(instances), 4, 4)); m[:, :3] = case.transforms[instances]; m[:, 3, 3] = 1.0
    inverse = np.linalg.inv(m)
    o = np.einsum("nij,nj->ni", inverse[:, :3, :3], origin.astype(np.float64)) + inverse[:, :3, 3]
    d = np.einsum("nij,nj->ni", inverse[:, :3, :3], direction.astype(np.float64))
    t = -o[:, 1] / d[:, 1]
    x, z = o[:, 0] + t * d[:, 0], o[:, 2] + t * d[:, 2]
    assert (o[:, 1] > 0.1).all() and (d[:, 1] < 0).all() and (np.minimum(np.minimum(0.5 - x, z + 0.5), x - z) >= 0.05).all()
    return np.ascontiguousarray(origin.T), np.ascontiguousarray(direction.T), t


@pytest.mark.parametrize("name", tlas_cases.names())
def test_kernel_on_the_boundary_wide_level_and_degenerate_cases(grt, oracle, bare_scene, name):
    """rt_build_tlas on one case of tests/tlas_cases.py, read back with rt_read_tlas and rt_read_instances:
      * nodes, node count and order are the restatement's, byte for byte -- for the cases whose widest level exceeds the workgroup
        this is the check of step 3b's chunked scan, which has no CPU twin;
      * the float64 rules of tests/tlas_reference.py hold on the device's own bytes;
      * the five tables are the scene-order inputs gathered by `order`, and position[order[p]] == p, exactly;
      * cases of at most 1 100 instances, and the comb: rays aimed at instances from outside the scene box and random rays, through
        rt_trace_rays, keep the float64 rules of tests/trace_checks.py against the brute force over every instance's triangles;
      * flat cases: the ray down the normal of every flat instance hits that instance."""
    case = tlas_cases.by_name(name)
    n = len(case.mesh)
    want_nodes, want_order = restated(oracle, case)
    assert bare_scene.build(case) == 0, bare_scene.lib.rt_last_error(bare_scene.ctx)
    nodes, order, (roots, materials, transforms, inverse, previous, position) = bare_scene.read(n)
    assert_same_bytes(name, nodes, order, want_nodes, want_order)
    found = tlas_reference.check(nodes, order, case.transforms, case.local_boxes)
    print("%s: %d nodes, widest level %d, containment %.3f of the slack, %d of %d child boxes widened" % (
        name, len(nodes), max(tlas_reference.level_widths(nodes)), found.containment_in_slacks, found.widened, found.children))
    for got, given in zip((roots, materials, transforms, inverse, previous), bare_scene.tables(case)):
        assert got.tobytes() == np.ascontiguousarray(given[order]).tobytes()
    assert np.array_equal(position[order], np.arange(n))
    if not case.traced:
        return
    boxes64, _ = tlas_reference.world_boxes64(case.transforms, case.local_boxes)
    world, owner = tlas_reference.world_triangles(case.transforms, case.mesh, bare_scene.mesh_triangles)
    origin, direction = rays_of(case, boxes64)
    if case.aim is not None:
        down_o, down_d, down_t = rays_down_the_normals(case)
        origin = np.concatenate([down_o, origin], axis=1); direction = np.concatenate([down_d, direction], axis=1)
    hits, _ = grt.trace_rays(bare_scene.ctx, origin, direction)
    bf = tlas_reference.brute_force(origin, direction, world, owner, boxes64)
    bare_scene.tlas_order_transforms = transforms
    trace_checks.check_closest(name, case, bare_scene, origin, direction, hits, bf)
    hit = hits[:, 1] != 0xffffffff
    print("%s: %d rays, %.1f %% hit, %.1f %% robust" % (name, len(hit), 100 * hit.mean(), 100 * trace_checks.ref.robust_closest(bf).mean()))
    if case.aim is not None:
        aimed = len(case.aim[0])
        assert hit[:aimed].all(), "%s: %d of %d flat instances are not hit down their normal" % (name, int((~hit[:aimed]).sum()), aimed)
        named = order[hits[:aimed, 0].astype(np.int64)]
        # the instance itself -- or another one at the same distance (tiles of one height overlap): check_closest has shown that hit to be real
        same = (named == case.aim[0]) | (np.abs(hits[:aimed, 2].view(np.float32).astype(np.float64) - down_t) <= bf.t_tol[:aimed])
        assert same.all(), "%s: %d rays down a normal hit something else than their instance" % (name, int((~same).sum()))


def test_build_refuses_sizes_outside_its_range_and_a_smaller_build_leaves_nothing_of_a_larger_one(grt, oracle, bare_scene):
    """Once for the whole file. (a) rt_build_tlas with 0 and with 4 097 instances is refused and launches nothing: the TLAS and the tables
    read back afterwards are those of the build before. (b) A build of 65 instances after one of 2 049 on the same context (the same
    ring entries, the same scratch area) gives the 65-instance case's bytes."""
    large, small = tlas_cases.by_name("uniform_2049"), tlas_cases.by_name("uniform_65")
    assert bare_scene.build(large) == 0, bare_scene.lib.rt_last_error(bare_scene.ctx)
    before = bare_scene.read(2049)
    assert_same_bytes(large.name, before[0], before[1], *restated(oracle, large))
    beyond = tlas_cases.uniform("uniform_4097", 4097, 4097)          # real arrays of 4 097 rows: a launch would have something to read
    for case, count in ((large, 0), (beyond, 4097)):
        assert bare_scene.build(case, count) != 0 and b"1 .. 4096" in bare_scene.lib.rt_last_error(bare_scene.ctx)
        after = bare_scene.read(2049)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and all(np.array_equal(a, b) for a, b in zip(before[2], after[2]))
    assert bare_scene.build(small) == 0, bare_scene.lib.rt_last_error(bare_scene.ctx)
    nodes, order, tables = bare_scene.read(65)
    assert_same_bytes(small.name, nodes, order, *restated(oracle, small))
    assert np.array_equal(tables[5][order], np.arange(65)) and tables[2].tobytes() == small.transforms.reshape(65, 12)[order].tobytes()
