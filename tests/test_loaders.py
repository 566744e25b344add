"""Host side: Mitsuba XML / OBJ loading, primitive tessellation, device data layout (CPU only)."""
import os

import numpy as np
import pytest

from conftest import make_pathtracer


@pytest.mark.reference_layout
def test_cornell_scene_inventory(grt):
    scene, pt = make_pathtracer(grt, "cornellbox", 512, 512, -1)
    # reference Data/cornellbox/scene.xml: 5 walls + light (rectangles, 2 tris) + 2 cubes (12 tris)
    assert scene.mesh_count == 8
    tris = pt.array("triangles").reshape(-1, 24)
    assert tris.shape[0] == 36
    # XML overrides: film 1024x1024 and maxDepth 65 (MitsubaLoader.cpp:610-616)
    assert grt.config_get("initial_width") == 1024
    assert pt.device_config().num_bounces == 65
    types = pt.array("material_types")
    assert (types == grt.MATERIAL_LIGHT).sum() == 1 and (types == grt.MATERIAL_DIFFUSE).sum() >= 8
    mats = pt.array("materials").reshape(-1, 8)
    light = mats[types == grt.MATERIAL_LIGHT][0]
    assert np.allclose(light[:3], [17, 12, 4])
    assert pt.lights_total_weight > 0
    pt.close(); scene.close()


@pytest.mark.reference_layout
def test_device_layout_rules(grt):
    """reference Integrator.cpp:101-283,399-430: TLAS slots first, MSB = identity, triangles as edges."""
    scene, pt = make_pathtracer(grt, "cornellbox", 64, 64, -1)
    roots = pt.array("mesh_bvh_root_indices").view(np.uint32)
    assert (roots >> 31).all()                      # primitives have baked transforms -> identity
    assert ((roots & 0x7fffffff) >= 2 * scene.mesh_count).all()
    nodes = pt.array("bvh8_nodes").reshape(-1, 80)
    assert nodes.shape[0] == 2 * scene.mesh_count + 8   # one CWBVH node per tiny mesh
    order = pt.array("tlas_indices")
    assert sorted(order.tolist()) == list(range(scene.mesh_count))
    xf = pt.array("mesh_transforms").reshape(-1, 12)
    assert np.allclose(xf, np.tile(np.eye(4, dtype=np.float32)[:3].reshape(-1), (scene.mesh_count, 1)))
    pt.close(); scene.close()


@pytest.mark.reference_layout
def test_sponza_inventory(grt):
    scene, pt = make_pathtracer(grt, "sponza", 64, 64, -1)
    assert scene.mesh_count == 384 and scene.mesh_data_count == 383
    tris = pt.array("triangles").reshape(-1, 24)
    assert tris.shape[0] == 262687                     # unique Sponza triangles
    nodes = pt.array("bvh8_nodes")
    assert nodes.size // 80 == 32291 + 2 * 384         # BASELINE.md section 2 + reserved TLAS slots
    roots = pt.array("mesh_bvh_root_indices").view(np.uint32)
    assert ((roots >> 31) == 0).sum() == 2             # the two translated icosphere lights
    assert pt.array("light_mesh_transform_indices").size == 2
    pt.close(); scene.close()


def test_obj_loader_fan_triangulation_and_negative_indices(grt, tmp_path):
    obj = tmp_path / "quad.obj"
    obj.write_text("# quad\no q\nv 0 0 0\nv 1 0 0 1.0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nf 1/1/1 2/2/1 3/3/1 4/4/1\nf -4//-1 -3//-1 -2//-1\n")
    grt.config_reset()
    scene = grt.Scene(str(obj))
    scene.wait_until_loaded()
    tris = scene.mesh_data_array(0, "triangles", np.float32).reshape(-1, 24)
    assert tris.shape[0] == 3
    assert np.allclose(tris[0, 0:9], [0, 0, 0, 1, 0, 0, 1, 1, 0])
    assert np.allclose(tris[1, 0:9], [0, 0, 0, 1, 1, 0, 0, 1, 0])     # fan: (v0, prev, curr)
    assert np.allclose(tris[0, 18:24], [0, 1, 1, 1, 1, 0])            # v flipped: t.y = 1 - t.y
    assert np.allclose(tris[2, 0:9], [0, 0, 0, 1, 0, 0, 1, 1, 0])     # negative indices
    scene.close()


def test_unsupported_scene_format_is_an_error(grt, tmp_path):
    bad = tmp_path / "scene.serialized"
    bad.write_text("x\n")
    grt.config_reset()
    with pytest.raises(RuntimeError, match="not supported"):
        grt.Scene(str(bad))


@pytest.mark.reference_layout
def test_mitsuba_materials_media_and_instances(grt, tmp_path):
    (tmp_path / "tri.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    xml = tmp_path / "scene.xml"
    xml.write_text("""<?xml version="1.0"?>
<!-- comment -->
<scene version="0.5.0">
  <integrator type="path"><integer name="maxDepth" value="7"/></integrator>
  <sensor type="thinlens"><float name="fov" value="60"/><float name="apertureRadius" value="0.1"/>
    <transform name="toWorld"><lookat origin="0, 0, 5" target="0, 0, 0" up="0, 1, 0"/></transform>
    <film type="hdrfilm"><integer name="width" value="320"/><integer name="height" value="200"/></film></sensor>
  <bsdf type="roughplastic" id="pl"><rgb name="diffuseReflectance" value="0.2, 0.3, 0.4"/><float name="alpha" value="0.3"/></bsdf>
  <bsdf type="roughconductor" id="cu"><rgb name="eta" value="1.25, 1.02, 0.3"/><rgb name="k" value="2.48, 2.58, 3.2"/><float name="alpha" value="0.1"/></bsdf>
  <shape type="obj"><string name="filename" value="tri.obj"/><ref id="pl"/>
    <transform name="toWorld"><scale value="2"/><translate x="1" y="2" z="3"/></transform></shape>
  <shape type="sphere"><float name="radius" value="0.5"/><bsdf type="roughdielectric"><string name="intIOR" value="water"/><float name="alpha" value="0.1"/></bsdf>
    <medium type="homogeneous" name="interior"><rgb name="sigmaA" value="0.1, 0.2, 0.3"/><rgb name="sigmaS" value="1, 1, 1"/><phase type="hg"><float name="g" value="0.2"/></phase></medium></shape>
  <shape type="rectangle"><ref id="cu"/></shape>
  <shape type="cube"><emitter type="area"><rgb name="radiance" value="5, 5, 5"/></emitter></shape>
</scene>""")
    grt.config_reset()
    scene = grt.Scene(str(xml))
    pt = grt.Pathtracer(scene, 320, 200, device=-1)
    pt.update()
    assert pt.device_config().num_bounces == 7
    types = pt.array("material_types").tolist()
    assert types.count(grt.MATERIAL_PLASTIC) == 1 and types.count(grt.MATERIAL_CONDUCTOR) == 1
    assert types.count(grt.MATERIAL_DIELECTRIC) == 1 and types.count(grt.MATERIAL_LIGHT) == 1
    mats = pt.array("materials").reshape(-1, 8)
    diel = mats[types.index(grt.MATERIAL_DIELECTRIC)]
    assert diel[:1].view(np.int32)[0] == 1 and abs(diel[1] - 1.333) < 1e-6 and abs(diel[2] - 0.1) < 1e-7   # medium id, ior, roughness
    media = pt.array("media").reshape(-1, 8)
    assert media.shape[0] == 2 and abs(media[1, 3] - 0.2) < 1e-7
    # Van de Hulst round trip is approximate; sigma_t = 1/mfp is exact
    assert np.allclose(media[1, 0:3] + media[1, 4:7], [1.1, 1.2, 1.3], rtol=1e-5)
    # the OBJ instance keeps a transform: scale 2 then translate
    order = pt.array("tlas_indices").tolist()
    roots = pt.array("mesh_bvh_root_indices").view(np.uint32)
    xf = pt.array("mesh_transforms").reshape(-1, 12)
    i = order.index(0)
    assert (roots[i] >> 31) == 0
    assert np.allclose(xf[i], [2, 0, 0, 1, 0, 2, 0, 2, 0, 0, 2, 3], atol=1e-6)
    inv = pt.array("mesh_transforms_inv").reshape(-1, 12)
    assert np.allclose(inv[i], [0.5, 0, 0, -0.5, 0, 0.5, 0, -1, 0, 0, 0.5, -1.5], atol=1e-6)
    cam = pt.camera()
    assert abs(cam.aperture_radius - 0.1) < 1e-7 and np.allclose(list(cam.position), [0, 0, 5])
    assert scene.mesh_count == 4 and pt.array("triangles").size // 24 == 1 + 20 * 64 + 2 + 12
    pt.close(); scene.close()


def test_mesh_transform_edit_rebuilds_the_tlas_tables(grt, oracle):
    """Mesh::position / rotation / scale edits (the reference's UI) + invalidate("scene"): the next
    update() writes the new matrices in TLAS order, clears the identity flag of the moved mesh, and the
    oracle finds the mesh at its new place."""
    scene, pt = make_pathtracer(grt, "cornellbox", 64, 64, -1)
    moved = 5                                                   # the short cube (12 triangles)
    pos, rot, scale = scene.mesh_transform(moved)
    assert pos == [0.0, 0.0, 0.0] and rot == [0.0, 0.0, 0.0, 1.0] and scale == 1.0
    view = oracle.SceneView(pt)
    o, d, _ = view.generate(0, 0, 64 * 64)
    before, _ = view.trace(o, d)
    scene.set_mesh_transform(moved, [0.0, 0.25, 0.0], [0.0, 0.38268343, 0.0, 0.92387953], 1.25)
    pt.invalidate("scene"); pt.update()
    order = pt.array("tlas_indices").tolist()
    slot = order.index(moved)
    roots = pt.array("mesh_bvh_root_indices").view(np.uint32)
    assert (roots[slot] >> 31) == 0 and ((roots >> 31) == 0).sum() == 1
    xf = pt.array("mesh_transforms").reshape(-1, 3, 4)[slot]
    assert np.allclose(xf[:, 3], [0.0, 0.25, 0.0]) and np.allclose(np.linalg.norm(xf[:, 0]), 1.25, atol=1e-5)
    inv = pt.array("mesh_transforms_inv").reshape(-1, 3, 4)[slot]
    full, full_inv = np.vstack([xf, [0, 0, 0, 1]]), np.vstack([inv, [0, 0, 0, 1]])
    assert np.allclose(full @ full_inv, np.eye(4), atol=1e-5)
    prev = pt.array("mesh_transforms_prev").reshape(-1, 3, 4)[slot]
    assert np.allclose(prev, np.eye(4)[:3])                     # transform_prev = the transform before this update
    after, stats = oracle.SceneView(pt).trace(o, d)
    assert stats.instances_transformed > 0 and not np.array_equal(before[:, 2], after[:, 2])
    pt.close(); scene.close()


def test_pixel_query_protocol_without_a_device(grt):
    """set_pixel_query arms the query (window y is top-down, Integrator.h:266-277); the status only
    advances when something renders."""
    scene, pt = make_pathtracer(grt, "cornellbox", 64, 48, -1)
    assert pt.pixel_query == (-1, -1, -1, 0)
    pt.set_pixel_query(10, 8)
    assert pt.pixel_query == (10 + (48 - 8) * pt.pitch, -1, -1, 1)
    pt.set_pixel_query(640, 8)                                  # outside the frame: ignored
    assert pt.pixel_query[0] == 10 + (48 - 8) * pt.pitch
    pt.update()
    assert pt.pixel_query[3] == 1                               # still pending: nothing was rendered
    pt.close(); scene.close()


def test_bvh4_collapse_invariants(grt):
    """BVH4Converter.cpp: node 1 is the entry point, every reachable node has 2..4 children, leaves cover
    every primitive index exactly once, child boxes lie inside their parent's box."""
    import ctypes
    lib = grt.host_lib()
    rng = np.random.default_rng(21)
    n = 3000
    p0 = (rng.random((n, 3)) * 40).astype(np.float32)
    tris = np.zeros((n, 24), np.float32)
    tris[:, 0:3] = p0; tris[:, 3:6] = p0 + rng.random((n, 3)).astype(np.float32); tris[:, 6:9] = p0 + rng.random((n, 3)).astype(np.float32)
    h = lib.grt_build_blas(tris.ctypes.data, n)
    size = ctypes.c_size_t()
    ptr = lib.grt_built_array(h, b"bvh4_nodes", ctypes.byref(size))
    raw = np.frombuffer((ctypes.c_char * size.value).from_address(ptr), dtype=np.uint8).copy()
    lib.grt_built_free(h)
    boxes = raw.view(np.float32).reshape(-1, 32)[:, :24].reshape(-1, 6, 4)      # min x,y,z / max x,y,z per child
    ic = raw.view(np.int32).reshape(-1, 32)[:, 24:].reshape(-1, 4, 2)
    assert tuple(ic[1, 0]) == (0, 0)
    covered = np.zeros(n, np.int32)
    stack, visited = [(0, None)], 0
    while stack:
        node, parent_box = stack.pop()
        counts = ic[node, :, 1]
        children = 4 if (counts != -1).all() else int(np.argmax(counts == -1))
        assert 2 <= children <= 4
        visited += 1
        for c in range(children):
            box = boxes[node, :, c]
            assert (box[:3] <= box[3:]).all()
            if parent_box is not None:
                assert (box[:3] >= parent_box[:3] - 1e-4).all() and (box[3:] <= parent_box[3:] + 1e-4).all()
            index, count = ic[node, c]
            if count > 0:
                covered[index:index + count] += 1
            else:
                stack.append((index, box))
    assert (covered == 1).all() and visited > n // 4


def _read_bvh_cache(path):
    """Parses a .bvh cache the way the reference's BVHLoader does (BVHLoader.cpp:19-33,150-176):
    28-byte header, then one raw deflate stream with triangles, nodes, indices."""
    import struct, zlib
    raw = open(path, "rb").read()
    ident, version, bvh_type, optimized, cost_node, cost_leaf, n_tri, n_node, n_index = struct.unpack("<4sbb?xffiii", raw[:28])
    payload = zlib.decompressobj(-15).decompress(raw[28:])
    assert len(payload) == 96 * n_tri + 32 * n_node + 4 * n_index
    tris = np.frombuffer(payload[:96 * n_tri], np.float32).reshape(-1, 24)
    nodes = np.frombuffer(payload[96 * n_tri:96 * n_tri + 32 * n_node], np.uint8)
    indices = np.frombuffer(payload[96 * n_tri + 32 * n_node:], np.int32)
    return dict(ident=ident, version=version, bvh_type=bvh_type, optimized=optimized, cost_node=cost_node, cost_leaf=cost_leaf,
                triangles=tris, nodes=nodes, indices=indices)


def _write_bvh_cache(path, c):
    import struct, zlib
    z = zlib.compressobj(9, zlib.DEFLATED, -15)
    body = z.compress(c["triangles"].tobytes() + c["nodes"].tobytes() + c["indices"].tobytes()) + z.flush()
    header = struct.pack("<4sbb?xffiii", c["ident"], c["version"], c["bvh_type"], c["optimized"], c["cost_node"], c["cost_leaf"],
                         c["triangles"].shape[0], c["nodes"].size // 32, c["indices"].size)
    open(path, "wb").write(header + body)


def test_bvh_cache_files_follow_the_reference_format(grt, tmp_path):
    """<mesh>.bvh (BVHLoader.cpp): written on the first load, read on the next, ignored when stale,
    built with other settings, truncated or inconsistent; holds the SAH tree, or the spatial-split
    tree when bvh_type = SBVH."""
    rng = np.random.default_rng(2)
    n = 300
    p0 = rng.random((n, 3)) * 4; p1 = p0 + rng.random((n, 3)) * 3 - 1.5; p2 = p0 + rng.random((n, 3)) * 0.4
    obj = tmp_path / "m.obj"
    with open(obj, "w") as f:
        for a, b, c in zip(p0, p1, p2):
            f.write("v %.6f %.6f %.6f\nv %.6f %.6f %.6f\nv %.6f %.6f %.6f\n" % (*a, *b, *c))
        for i in range(n):
            f.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    cache = str(obj) + ".bvh"

    def load(**config):
        grt.config_reset()
        grt.config_set(**config)
        scene = grt.Scene(str(obj)); scene.wait_until_loaded()
        out = {k: scene.mesh_data_array(0, k, dt).copy() for k, dt in (("triangles", np.float32), ("bvh2_nodes", np.uint8), ("bvh2_indices", np.int32), ("bvh8_nodes", np.uint8))}
        scene.close()
        return out

    built = load()                                   # caching is opt-in: nothing is written by default
    assert not os.path.exists(cache)
    first = load(enable_bvh_cache=1)
    c = _read_bvh_cache(cache)
    assert c["ident"] == b"BVH\0" and c["version"] == 7 and c["bvh_type"] == 0 and not c["optimized"] and (c["cost_node"], c["cost_leaf"]) == (4.0, 1.0)
    assert np.array_equal(c["triangles"].ravel(), built["triangles"]) and np.array_equal(c["nodes"], built["bvh2_nodes"]) and np.array_equal(c["indices"], built["bvh2_indices"])
    assert all(np.array_equal(first[k], built[k]) for k in built)

    # a cache written by someone else (here: python, in the reference's layout) is what gets loaded ...
    marked = dict(c); marked["triangles"] = c["triangles"].copy(); marked["triangles"][5, 0] += 0.125
    _write_bvh_cache(cache, marked)
    second = load(enable_bvh_cache=1)
    assert second["triangles"].reshape(-1, 24)[5, 0] == marked["triangles"][5, 0] and np.array_equal(second["bvh2_nodes"], built["bvh2_nodes"])
    assert np.array_equal(second["bvh8_nodes"], built["bvh8_nodes"])             # the CWBVH is re-derived from the cached tree
    # ... unless rebuilding is forced, the settings differ, or the mesh file is newer
    assert np.array_equal(load(enable_bvh_cache=1, bvh_force_rebuild=1)["triangles"], built["triangles"])
    _write_bvh_cache(cache, marked)
    assert np.array_equal(load(enable_bvh_cache=1, sah_cost_node=3.0)["triangles"], built["triangles"])
    _write_bvh_cache(cache, marked)
    later = os.stat(cache).st_mtime + 10
    os.utime(obj, (later, later))
    assert np.array_equal(load(enable_bvh_cache=1)["triangles"], built["triangles"])
    assert np.array_equal(_read_bvh_cache(cache)["triangles"].ravel(), built["triangles"])   # and the cache was refreshed

    # damaged caches are rejected, not trusted: truncated stream, child index out of range
    raw = open(cache, "rb").read()
    open(cache, "wb").write(raw[:len(raw) // 2])
    os.utime(cache, (later + 5, later + 5))
    assert np.array_equal(load(enable_bvh_cache=1)["bvh2_nodes"], built["bvh2_nodes"])
    bad = _read_bvh_cache(cache); bad["indices"] = bad["indices"].copy(); bad["indices"][3] = n + 7
    _write_bvh_cache(cache, bad)
    os.utime(cache, (later + 5, later + 5))
    assert np.array_equal(load(enable_bvh_cache=1)["bvh2_indices"], built["bvh2_indices"])

    # bvh_type = SBVH caches the spatial-split tree (header type 1, more references than triangles)
    os.remove(cache)
    grt.config_reset(); grt.config_set(bvh_type="sbvh", enable_bvh_cache=1)
    scene = grt.Scene(str(obj)); pt = grt.Pathtracer(scene, 8, 8, device=-1)
    device_nodes = scene.mesh_data_array(0, "device_bvh2_nodes", np.uint8).copy()
    pt.close(); scene.close()
    c = _read_bvh_cache(cache)
    assert c["bvh_type"] == 1 and c["indices"].size > n and c["triangles"].shape[0] == n
    scene = grt.Scene(str(obj)); pt = grt.Pathtracer(scene, 8, 8, device=-1)   # second time: from the cache
    assert np.array_equal(scene.mesh_data_array(0, "device_bvh2_nodes", np.uint8), device_nodes)
    pt.close(); scene.close(); grt.config_reset()


def test_bvh_caches_of_optimized_trees_and_tiny_meshes_load_again(grt, tmp_path):
    """Two ways a valid cache used to be refused and rebuilt on every load: (1) BVHOptimizer re-inserts subtrees into
    freed node slots, so children may precede their parent in the array -- the loader must check that the nodes form
    a tree, not their order; (2) a stream so short that zlib still holds output when the file is at its end (2
    triangles inflate from one read). A marked cache proves that the second load really came from the file. A cache
    whose nodes form a cycle, or share a subtree, is still rejected."""
    rng = np.random.default_rng(5)
    for name, n, config in (("opt", 400, dict(enable_bvh_optimization=1, bvh_optimizer_max_num_batches=3)), ("tiny", 2, dict())):
        p0 = rng.random((n, 3)) * 4; p1 = p0 + rng.random((n, 3)) * 3 - 1.5; p2 = p0 + rng.random((n, 3)) * 0.4
        obj = tmp_path / (name + ".obj")
        with open(obj, "w") as f:
            for a, b, c in zip(p0, p1, p2):
                f.write("v %.6f %.6f %.6f\nv %.6f %.6f %.6f\nv %.6f %.6f %.6f\n" % (*a, *b, *c))
            for i in range(n):
                f.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
        cache = str(obj) + ".bvh"

        def load():
            grt.config_reset(); grt.config_set(enable_bvh_cache=1, **config)
            scene = grt.Scene(str(obj)); scene.wait_until_loaded()
            out = {k: scene.mesh_data_array(0, k, dt).copy() for k, dt in (("triangles", np.float32), ("bvh2_nodes", np.uint8), ("bvh2_indices", np.int32))}
            scene.close()
            return out

        built = load()
        c = _read_bvh_cache(cache)
        assert bool(c["optimized"]) == (name == "opt") and np.array_equal(c["nodes"], built["bvh2_nodes"])
        nodes = c["nodes"].view(np.int32).reshape(-1, 8)          # 6 floats of box, left_or_first, count | axis << 30
        inner = np.nonzero((nodes[:, 7] & 0x3fffffff) == 0)[0]
        inner = inner[inner != 1]
        if name == "opt":
            assert (nodes[inner, 6] < inner).any()                    # the optimizer did put children in front of parents
        marked = dict(c); marked["triangles"] = c["triangles"].copy(); marked["triangles"][1, 0] += 0.25
        _write_bvh_cache(cache, marked)
        again = load()
        assert again["triangles"].reshape(-1, 24)[1, 0] == marked["triangles"][1, 0], name   # came from the cache
        assert np.array_equal(again["bvh2_nodes"], built["bvh2_nodes"]) and np.array_equal(again["bvh2_indices"], built["bvh2_indices"])
        if name == "opt":
            # not a tree: an inner node pointing back at the root's children (cycle / shared subtree) -> rebuilt
            bad = dict(marked); bad_nodes = nodes.copy(); bad_nodes[inner[-1], 6] = nodes[0, 6]
            bad["nodes"] = bad_nodes.view(np.uint8).ravel()
            _write_bvh_cache(cache, bad)
            rebuilt = load()
            assert np.array_equal(rebuilt["triangles"], built["triangles"]) and np.array_equal(rebuilt["bvh2_nodes"], built["bvh2_nodes"])
    grt.config_reset()


def test_bmp_palette_indices_beyond_the_declared_colours_stay_in_bounds(grt, tmp_path):
    """An 8-bit BMP whose pixels name palette entries the file does not hold (biClrUsed = 2, index 255) used to read
    past the buffer; such entries are black now, and pixel data that claims to start inside the headers is refused."""
    import struct
    def bmp(colours_used, data_offset, pixel):
        palette = bytes([10, 20, 30, 0, 40, 50, 60, 0])[:4 * colours_used]
        header = struct.pack("<IiiHHIIiiII", 40, 1, 1, 1, 8, 0, 4, 2835, 2835, colours_used, 0)
        body = header + palette
        pixels = bytes([pixel, 0, 0, 0])
        offset = 14 + len(body) if data_offset is None else data_offset
        return b"BM" + struct.pack("<IHHI", 14 + len(body) + 4, 0, 0, offset) + body + pixels
    for name, data, expect in (("ok.bmp", bmp(2, None, 1), (60, 50, 40, 255)), ("beyond.bmp", bmp(2, None, 255), (0, 0, 0, 255)), ("inside.bmp", bmp(2, 0, 1), None)):
        path = tmp_path / name
        open(path, "wb").write(data)
        if expect is None:
            with pytest.raises(RuntimeError, match="cannot decode"):
                grt.load_texture(path)
        else:
            level0 = grt.load_texture(path)[0]
            assert level0.shape == (1, 1, 4) and np.array_equal(level0, _srgb_to_linear_u8(np.array(expect, np.uint8).reshape(1, 1, 4))), name


def _ply_bytes(fmt, positions, normals, uvs, faces, index_type="int", with_extras=False, face_extras=None):
    """Serialises a mesh as PLY in one of the three encodings (an independent writer for the reader under test)."""
    import struct
    face_extras = with_extras if face_extras is None else face_extras
    header = ["ply", "format %s 1.0" % fmt, "comment made by the test", "element vertex %d" % len(positions),
              "property float x", "property float y", "property float z"]
    if normals is not None:
        header += ["property float nx", "property float ny", "property float nz"]
    if with_extras:
        header += ["property uchar red"]
    if uvs is not None:
        header += ["property double s", "property double t"]
    header += ["element face %d" % len(faces), "property list uchar %s vertex_indices" % index_type]
    if face_extras:
        header += ["property short flags"]
    header += ["end_header"]
    out = ("\n".join(header) + "\n").encode()
    e = "<" if fmt == "binary_little_endian" else ">"
    icode = {"int": "i", "uint": "I", "ushort": "H", "uchar": "B"}[index_type]
    for v in range(len(positions)):
        if fmt == "ascii":
            vals = list(positions[v]) + (list(normals[v]) if normals is not None else []) + ([200] if with_extras else []) + (list(uvs[v]) if uvs is not None else [])
            out += (" ".join(repr(float(x)) if not isinstance(x, int) else str(x) for x in vals) + "\n").encode()
        else:
            out += struct.pack(e + "3f", *positions[v])
            if normals is not None: out += struct.pack(e + "3f", *normals[v])
            if with_extras: out += struct.pack("B", 200)
            if uvs is not None: out += struct.pack(e + "2d", *uvs[v])
    for f in faces:
        if fmt == "ascii":
            out += ("%d %s%s\n" % (len(f), " ".join(map(str, f)), " 3" if face_extras else "")).encode()
        else:
            out += struct.pack("B", len(f)) + struct.pack(e + "%d%s" % (len(f), icode), *f)
            if face_extras: out += struct.pack(e + "h", 3)
    return out


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_ply_loader_reads_all_three_encodings(grt, tmp_path, fmt):
    """PLYLoader.cpp: scalar types by name, s/t as texture coordinates with the v flip, polygons
    fan-triangulated around their first corner, unknown properties skipped, and a mesh without
    normals gets face normals from the Triangle constructor."""
    rng = np.random.default_rng(4)
    positions = np.round(rng.random((7, 3)) * 4 - 2, 3).astype(np.float32)
    normals = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (7, 1))
    uvs = np.round(rng.random((7, 2)), 3)
    faces = [[0, 1, 2], [2, 3, 4, 5], [1, 6, 5, 4, 3]]
    want_corners = [(0, 1, 2), (2, 3, 4), (2, 4, 5), (1, 6, 5), (1, 5, 4), (1, 4, 3)]
    for variant, (with_normals, extras, index_type) in enumerate(((True, False, "int"), (False, True, "ushort" if fmt != "ascii" else "uint"))):
        path = tmp_path / ("m%d.ply" % variant)
        path.write_bytes(_ply_bytes(fmt, positions, normals if with_normals else None, uvs, faces, index_type, extras))
        grt.config_reset()
        scene = grt.Scene(str(path)); scene.wait_until_loaded()
        tris = scene.mesh_data_array(0, "triangles", np.float32).reshape(-1, 24).copy()
        scene.close()
        assert tris.shape[0] == len(want_corners)
        for t, corners in zip(tris, want_corners):
            got_p = t[0:9].reshape(3, 3); got_uv = t[18:24].reshape(3, 2); got_n = t[9:18].reshape(3, 3)
            face_n = np.cross(positions[corners[1]] - positions[corners[0]], positions[corners[2]] - positions[corners[0]])
            flipped = with_normals and face_n[2] < 0        # the Triangle constructor swaps corners 1 and 2 when every normal opposes the face
            order = (corners[0], corners[2], corners[1]) if flipped else corners
            assert np.array_equal(got_p, positions[list(order)])
            want_uv = np.stack([uvs[list(order), 0].astype(np.float32), 1.0 - uvs[list(order), 1].astype(np.float32)], 1)
            assert np.allclose(got_uv, want_uv, atol=1e-6)
            if with_normals:
                assert np.array_equal(got_n, normals[list(order)])
            else:
                unit = face_n / np.linalg.norm(face_n)
                assert np.allclose(got_n, np.tile(unit, (3, 1)), atol=1e-5)


def test_ply_in_a_mitsuba_scene_and_malformed_files(grt, tmp_path):
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    (tmp_path / "quad.ply").write_bytes(_ply_bytes("binary_little_endian", positions, None, None, [[0, 1, 3, 2]]))
    (tmp_path / "s.xml").write_text('<scene version="0.5.0"><shape type="ply"><string name="filename" value="quad.ply"/></shape></scene>')
    grt.config_reset()
    scene = grt.Scene(str(tmp_path / "s.xml")); scene.wait_until_loaded()
    assert scene.mesh_data_array(0, "triangles", np.float32).size == 2 * 24
    scene.close()
    for name, data in (("short.ply", _ply_bytes("binary_little_endian", positions, None, None, [[0, 1, 3, 2]])[:-5]),
                       ("range.ply", _ply_bytes("ascii", positions, None, None, [[0, 1, 9]])),
                       ("edge.ply", _ply_bytes("ascii", positions, None, None, [[0, 1]])),
                       ("elem.ply", b"ply\nformat ascii 1.0\nelement edge 1\nproperty int a\nend_header\n1\n"),
                       ("nohdr.ply", b"plx\n")):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(Exception):
            s = grt.Scene(str(tmp_path / name)); s.wait_until_loaded()


def _parse_exr(path):
    """Minimal reader for uncompressed scan-line OpenEXR files, written from the file format
    description (magic, attribute list, offset table, one chunk per line with channels in
    alphabetical order)."""
    import struct
    raw = open(path, "rb").read()
    assert raw[:4] == bytes([0x76, 0x2f, 0x31, 0x01]) and struct.unpack("<I", raw[4:8])[0] == 2
    pos, attrs = 8, {}
    def cstr():
        nonlocal pos
        end = raw.index(b"\0", pos); s = raw[pos:end].decode(); pos = end + 1; return s
    while raw[pos] != 0:
        name, kind = cstr(), cstr()
        size = struct.unpack("<i", raw[pos:pos + 4])[0]; pos += 4
        attrs[name] = (kind, raw[pos:pos + size]); pos += size
    pos += 1
    kind, ch = attrs["channels"]
    channels, cp = [], 0
    while ch[cp] != 0:
        end = ch.index(b"\0", cp); nm = ch[cp:end].decode(); cp = end + 1
        ptype, _, xs, ys = struct.unpack("<iIii", ch[cp:cp + 16]); cp += 16
        channels.append((nm, ptype)); assert xs == ys == 1
    assert attrs["compression"][1] == b"\0" and attrs["lineOrder"][1] == b"\0"
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    offsets = struct.unpack("<%dQ" % h, raw[pos:pos + 8 * h])
    image = {nm: np.zeros((h, w), np.float32) for nm, _ in channels}
    for row in range(h):
        y, size = struct.unpack("<ii", raw[offsets[row]:offsets[row] + 8])
        p = offsets[row] + 8
        for nm, ptype in channels:
            assert ptype == 1
            image[nm][y - y0] = np.frombuffer(raw[p:p + 2 * w], np.float16).astype(np.float32); p += 2 * w
        assert p - offsets[row] - 8 == size
    assert offsets[-1] + 8 + size == len(raw)
    return channels, image


def test_exporters_write_the_reference_file_formats(grt, tmp_path):
    """PPMExporter.cpp / EXRExporter.cpp: rows flipped (the frame's row 0 is the bottom), PPM header
    'P6\\n w\\n h\\n 255\\n' with truncating 8-bit conversion of the tone-mapped frame (post.frag: ACES,
    gamma 2.2, through the 8-bit back buffer), EXR with half channels B, G, R and no compression."""
    rng = np.random.default_rng(8)
    h, w = 5, 7
    img = (rng.random((h, w, 3)) * 3).astype(np.float32)
    img[0, 0] = (-1.0, 0.0, 70000.0)     # negative, zero, beyond the half range
    img[1, 1] = (1e-8, 6.1e-5, 0.333)    # flushes to zero, the smallest normal half, an inexact value

    grt.export_image(tmp_path / "a.ppm", img)
    raw = open(tmp_path / "a.ppm", "rb").read()
    header = b"P6\n %d\n %d\n 255\n" % (w, h)
    assert raw.startswith(header) and len(raw) == len(header) + w * h * 3
    got = np.frombuffer(raw[len(header):], np.uint8).reshape(h, w, 3)
    c = np.maximum(img.astype(np.float64), 0)
    aces = np.clip(c * (2.51 * c + 0.03) / (c * (2.43 * c + 0.59) + 0.14), 0, 1) ** (1 / 2.2)
    want = np.floor(aces * 255 + 0.5)[::-1]
    assert np.abs(got.astype(np.int32) - want).max() <= 1 and (got == want).mean() > 0.9   # k/255*255 may land just under k in fp32

    grt.export_image(tmp_path / "a.exr", img)
    channels, image = _parse_exr(tmp_path / "a.exr")
    assert channels == [("B", 1), ("G", 1), ("R", 1)]
    with np.errstate(over="ignore"):
        want16 = img[::-1].astype(np.float16).astype(np.float32)      # (no ties in this image: tinyexr rounds those away from zero, numpy to even)
    for k, name in enumerate("RGB"):
        assert np.array_equal(image[name], want16[:, :, k]), name
    assert np.isinf(image["B"][h - 1, 0]) and image["R"][h - 1, 0] == -1.0

    with pytest.raises(RuntimeError, match="unsupported output file extension"):
        grt.export_image(tmp_path / "a.png", img)
    with pytest.raises(RuntimeError, match="failed to write"):
        grt.export_image(tmp_path / "no_such_dir" / "a.ppm", img)


CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-raytracer_amd", "host", "pathtracer")


def test_command_line_front_end_parses_like_the_reference():
    """Args.cpp:51-184 -- option names, the messages for unknown options and bad values; no device needed."""
    import subprocess
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, timeout=60)
    r = run("--help")
    assert r.returncode == 0
    for name in ("--integrator", "--width", "--height", "--bounce", "--samples", "--output", "--scene", "--sky", "--bvh", "--nee", "--mis",
                 "--force-rebuild", "--sah-node", "--sah-leaf", "--sbvh-alpha", "--mipmap", "--help"):
        assert name in r.stdout, name
    r = run()
    assert r.returncode == 1 and "no scene file" in r.stderr
    r = run("--bvh", "bvh16", "x.xml")
    assert r.returncode == 1 and "not a recognized BVH type" in r.stderr
    r = run("-I", "photonmap", "x.xml")
    assert r.returncode == 1 and "not a recognized integrator type" in r.stderr
    r = run("--frobnicate", "-s", "/no/such/scene.xml", "--device", "-1")
    assert "Unrecognized command line option '--frobnicate'" in r.stdout and r.returncode == 1 and "unable to open" in r.stderr
    r = run("/no/such/scene.obj", "--device", "-1")                 # a bare argument is a scene file
    assert r.returncode == 1 and "scene.obj" in r.stderr


def _serialized_archive(meshes, version):
    """Mitsuba .serialized writer for the test: [0x041c, version, zlib(mesh)]* + offsets + count."""
    import struct, zlib
    out, offsets = b"", []
    for m in meshes:
        offsets.append(len(out))
        real = "d" if m["double"] else "f"
        flags = (0x0001 if m.get("normals") is not None else 0) | (0x0002 if m.get("uvs") is not None else 0) | \
                (0x0008 if m.get("colours") is not None else 0) | (0x0010 if m.get("face_normals") else 0) | (0x2000 if m["double"] else 0x1000)
        body = struct.pack("<I", flags)
        if version > 3:
            body += m["name"].encode() + b"\0"
        body += struct.pack("<QQ", len(m["positions"]), len(m["faces"]))
        for key in ("positions", "normals", "uvs", "colours"):
            if m.get(key) is not None:
                body += np.asarray(m[key], np.float64 if m["double"] else np.float32).tobytes()
        body += np.asarray(m["faces"], np.uint32).tobytes()
        out += struct.pack("<HH", 0x041c, version) + zlib.compress(body)
    for o in offsets:
        out += struct.pack("<Q" if version > 3 else "<I", o)
    return out + struct.pack("<I", len(meshes))


@pytest.mark.parametrize("version", [3, 4])
def test_serialized_mesh_archives(grt, tmp_path, version):
    """SerializedLoader.cpp: end-of-file dictionary with 32-bit (<= v3) or 64-bit offsets, per-mesh zlib
    stream, flags for normals / uvs / colours / face normals / precision, shapeIndex selection."""
    rng = np.random.default_rng(6)
    quad = dict(name="quad", double=(version > 3), positions=[[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], normals=[[0, 0, 1]] * 4,
                uvs=[[0, 0], [1, 0], [1, 1], [0, 1]], colours=[[1, 0, 0]] * 4, faces=[[0, 1, 2], [0, 2, 3]])
    pos = np.round(rng.random((5, 3)) * 2, 3)
    fan = dict(name="fan", double=False, positions=pos, faces=[[0, 1, 2], [0, 2, 3], [0, 3, 4]], face_normals=True)
    (tmp_path / "meshes.serialized").write_bytes(_serialized_archive([quad, fan], version))
    (tmp_path / "s.xml").write_text('<scene version="0.5.0">'
                                    '<shape type="serialized"><string name="filename" value="meshes.serialized"/></shape>'
                                    '<shape type="serialized"><string name="filename" value="meshes.serialized"/><integer name="shapeIndex" value="1"/></shape></scene>')
    grt.config_reset()
    scene = grt.Scene(str(tmp_path / "s.xml")); scene.wait_until_loaded()
    assert scene.mesh_data_count == 2
    q = scene.mesh_data_array(0, "triangles", np.float32).reshape(-1, 24)
    f = scene.mesh_data_array(1, "triangles", np.float32).reshape(-1, 24)
    scene.close()
    assert q.shape[0] == 2 and np.array_equal(q[1, 0:9], [0, 0, 0, 1, 1, 0, 0, 1, 0]) and np.array_equal(q[0, 9:18], [0, 0, 1] * 3)
    assert np.array_equal(q[1, 18:24], [0, 0, 1, 1, 0, 1])             # serialized uvs are taken as they are (no v flip)
    assert f.shape[0] == 3
    for t, (a, b, c) in zip(f, fan["faces"]):
        p = pos.astype(np.float32)
        n = np.cross(p[b] - p[a], p[c] - p[a]); n /= np.linalg.norm(n)
        assert np.array_equal(t[0:9].reshape(3, 3), p[[a, b, c]]) and np.allclose(t[9:18].reshape(3, 3), n, atol=1e-6)
    # a shape index beyond the dictionary and a truncated archive are errors, not crashes
    (tmp_path / "bad.xml").write_text('<scene version="0.5.0"><shape type="serialized"><string name="filename" value="meshes.serialized"/><integer name="shapeIndex" value="2"/></shape></scene>')
    with pytest.raises(RuntimeError, match="no shape #2"):
        s = grt.Scene(str(tmp_path / "bad.xml")); s.wait_until_loaded()
    (tmp_path / "meshes.serialized").write_bytes(_serialized_archive([quad, fan], version)[:40])
    with pytest.raises(RuntimeError):
        s = grt.Scene(str(tmp_path / "s.xml")); s.wait_until_loaded()


@pytest.mark.parametrize("binary", [False, True])
def test_hair_strands_become_tapered_ribbons(grt, tmp_path, binary):
    """MitshairLoader.cpp: ascii (blank line ends a strand) and BINARY_HAIR (+inf ends a strand) files;
    every segment gives two triangles of a flat ribbon, `radius` wide on each side at the root and
    closing to a point at the tip; strands with fewer than 2 vertices are dropped."""
    import struct
    strands = [np.array([[0, 0, 0], [0, 1, 0], [0.2, 2, 0], [0.2, 3, 0.1]], np.float32), np.array([[5, 5, 5]], np.float32),
               np.array([[1, 0, 0], [1, 0.5, 0.5], [1, 1, 1]], np.float32)]
    if binary:
        data = b"BINARY_HAIR" + struct.pack("<I", sum(len(s) for s in strands))
        for s in strands:
            data += s.tobytes() + struct.pack("<f", np.inf)
    else:
        data = "".join("".join("%g %g %g\n" % tuple(v) for v in s) + "\n" for s in strands).encode()
    (tmp_path / "h.hair").write_bytes(data)
    (tmp_path / "s.xml").write_text('<scene version="0.5.0"><shape type="hair"><string name="filename" value="h.hair"/><float name="radius" value="0.05"/></shape></scene>')
    grt.config_reset()
    loads = []
    for _ in range(2):
        scene = grt.Scene(str(tmp_path / "s.xml")); scene.wait_until_loaded()
        loads.append(scene.mesh_data_array(0, "triangles", np.float32).reshape(-1, 24).copy())
        scene.close()
    tris = loads[0]
    # the random ribbon angle is seeded by the file name; the last triangle of a strand is degenerate
    # (both tip corners coincide), so its generated face normal is NaN -- as in the reference
    assert np.array_equal(loads[0], loads[1], equal_nan=True)
    assert tris.shape[0] == 2 * 3 + 2 * 2
    first, last = tris[0], tris[5]
    root_a, root_b = first[0:3], first[3:6]
    assert np.allclose((root_a + root_b) / 2, strands[0][0], atol=1e-6) and abs(np.linalg.norm(root_a - root_b) - 0.1) < 1e-5
    assert abs(np.dot(root_a - root_b, strands[0][1] - strands[0][0])) < 1e-5        # across the strand direction
    assert np.allclose(last[3:6], strands[0][3], atol=1e-6) and np.allclose(last[6:9], strands[0][3], atol=1e-6)   # both tip corners meet
    mid = tris[2]                                                 # second segment starts at 2/3 of the radius
    assert abs(np.linalg.norm(mid[0:3] - mid[3:6]) - 0.1 * 2 / 3) < 1e-5


def _png_bytes(pixels, colour_type, depth, interlace=False, palette=None, trns=None, filters=(0, 1, 2, 3, 4)):
    """PNG encoder for the decoder test. pixels: (h, w, channels) integer samples in [0, 2^depth)."""
    import struct, zlib
    h, w, ch = pixels.shape

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)

    def pack_rows(img):
        rows = []
        for y in range(img.shape[0]):
            samples = img[y].reshape(-1)
            if depth == 16:
                rows.append(samples.astype(">u2").tobytes())
            elif depth == 8:
                rows.append(samples.astype(np.uint8).tobytes())
            else:
                bits = "".join(format(int(s), "0%db" % depth) for s in samples)
                bits += "0" * (-len(bits) % 8)
                rows.append(bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)))
        return rows

    def filter_rows(rows, bpp):
        out, prior = b"", bytes(len(rows[0])) if rows else b""
        for y, row in enumerate(rows):
            f = filters[y % len(filters)]
            enc = bytearray(len(row))
            for i in range(len(row)):
                a = row[i - bpp] if i >= bpp else 0
                b = prior[i]
                c = prior[i - bpp] if i >= bpp else 0
                if f == 0: pred = 0
                elif f == 1: pred = a
                elif f == 2: pred = b
                elif f == 3: pred = (a + b) // 2
                else:
                    p = a + b - c; pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                enc[i] = (row[i] - pred) & 255
            out += bytes([f]) + bytes(enc)
            prior = row
        return out

    bpp = max(1, ch * depth // 8)
    if interlace:
        raw = b""
        for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
            sub = pixels[y0::dy, x0::dx]
            if sub.shape[0] and sub.shape[1]:
                raw += filter_rows(pack_rows(sub), bpp)
    else:
        raw = filter_rows(pack_rows(pixels), bpp)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0, 1 if interlace else 0))
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", trns)
    comp = zlib.compress(raw)
    out += chunk(b"IDAT", comp[:len(comp) // 2]) + chunk(b"IDAT", comp[len(comp) // 2:])    # split across two chunks
    return out + chunk(b"IEND", b"")


def _srgb_to_linear_u8(rgba8):
    """What the texture loader stores for an 8-bit sRGB image: gamma_to_linear in float32, truncated to 8 bits."""
    c = rgba8.astype(np.float32) / np.float32(255.0)
    lin = np.where(c <= np.float32(0.04045), c / np.float32(12.92), ((c + np.float32(0.055)) / np.float32(1.055)) ** np.float32(2.4))
    return np.clip(lin * np.float32(255.0), 0, 255).astype(np.uint8)


def test_png_bmp_and_dds_textures_decode(grt, tmp_path):
    """Texture formats besides TGA: PNG in every colour type / depth / interlace mode with all five
    scanline filters, BMP 24 / 32 / palettised, DXT1 / DXT3 / DXT5 DDS. Level 0 of the loaded texture is
    the decoded image converted from sRGB to linear (DDS: stored values unchanged)."""
    import struct
    rng = np.random.default_rng(10)
    grt.config_reset()
    h, w = 13, 11
    cases = []
    for interlace in (False, True):
        rgb8 = rng.integers(0, 256, (h, w, 3)); cases.append((_png_bytes(rgb8, 2, 8, interlace), np.dstack([rgb8, np.full((h, w), 255)])))
        rgba8 = rng.integers(0, 256, (h, w, 4)); cases.append((_png_bytes(rgba8, 6, 8, interlace), rgba8))
        rgba16 = rng.integers(0, 65536, (h, w, 4)); cases.append((_png_bytes(rgba16, 6, 16, interlace), rgba16 >> 8))
        ga8 = rng.integers(0, 256, (h, w, 2)); cases.append((_png_bytes(ga8, 4, 8, interlace), np.dstack([ga8[:, :, 0]] * 3 + [ga8[:, :, 1]])))
        for depth in (1, 2, 4, 8, 16):
            g = rng.integers(0, 1 << depth, (h, w, 1))
            g8 = (g * 255 // ((1 << depth) - 1)) if depth < 8 else (g >> (depth - 8))
            cases.append((_png_bytes(g, 0, depth, interlace), np.dstack([g8[:, :, 0]] * 3 + [np.full((h, w), 255)])))
        for depth in (1, 2, 4, 8):
            n = 1 << depth
            palette = rng.integers(0, 256, (n, 3)); alpha = rng.integers(0, 256, max(1, n // 2))
            idx = rng.integers(0, n, (h, w, 1))
            a = np.where(idx[:, :, 0] < len(alpha), np.concatenate([alpha, np.full(n, 255)])[idx[:, :, 0]], 255)
            cases.append((_png_bytes(idx, 3, depth, interlace, palette=palette, trns=bytes(alpha.astype(np.uint8))), np.dstack([palette[idx[:, :, 0]], a])))
    key = rng.integers(0, 256, (h, w, 3)); key[2, 3] = (9, 8, 7)          # colour-key transparency
    want = np.dstack([key, np.where((key == (9, 8, 7)).all(axis=2), 0, 255)])
    cases.append((_png_bytes(key, 2, 8, trns=struct.pack(">HHH", 9, 8, 7)), want))
    for i, (data, rgba) in enumerate(cases):
        path = tmp_path / ("t%d.png" % i); path.write_bytes(data)
        levels = grt.load_texture(path)
        assert levels[0].shape == (h, w, 4) and np.array_equal(levels[0], _srgb_to_linear_u8(rgba)), i
        assert [l.shape[:2] for l in levels][-1] == (1, 1) and len(levels) == 4           # 13x11 -> 6x5 -> 3x2 -> 1x1

    # BMP: bottom-up 24 bit with row padding, top-down 32 bit BI_RGB, 8 bit palettised
    rgb = rng.integers(0, 256, (5, 3, 3)).astype(np.uint8)
    row = lambda r: bytes(r[:, ::-1].reshape(-1)) + b"\0" * ((-3 * 3) % 4)
    bmp24 = b"BM" + struct.pack("<IHHI", 54 + 12 * 5, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, 3, 5, 1, 24, 0, 0, 0, 0, 0, 0) + b"".join(row(rgb[y]) for y in range(4, -1, -1))
    bgra = np.dstack([rgb[:, :, ::-1], np.full((5, 3), 0, np.uint8)])       # an all-zero fourth byte means "no alpha", as in stb_image
    bmp32 = b"BM" + struct.pack("<IHHI", 54 + 60, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, 3, -5, 1, 32, 0, 0, 0, 0, 0, 0) + bgra.tobytes()
    pal = rng.integers(0, 256, (256, 3)).astype(np.uint8); idx = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    bmp8 = b"BM" + struct.pack("<IHHI", 54 + 1024 + 20, 0, 0, 54 + 1024) + struct.pack("<IiiHHIIiiII", 40, 3, 5, 1, 8, 0, 0, 0, 0, 256, 0) + \
        np.hstack([pal[:, ::-1], np.zeros((256, 1), np.uint8)]).tobytes() + b"".join(bytes(idx[y]) + b"\0" for y in range(4, -1, -1))
    for name, data, want in (("a.bmp", bmp24, rgb), ("b.bmp", bmp32, rgb), ("c.bmp", bmp8, pal[idx])):
        (tmp_path / name).write_bytes(data)
        got = grt.load_texture(tmp_path / name)[0]
        assert np.array_equal(got, _srgb_to_linear_u8(np.dstack([want, np.full((5, 3), 255, np.uint8)]))), name

    # DDS: 8x4 DXT1 with two mip levels; block 0 in 4-colour mode, block 1 in 3-colour + transparent mode
    def rgb565(r, g, b): return (r << 11) | (g << 5) | b
    def expand(c): r, g, b = c >> 11, (c >> 5) & 63, c & 31; return np.array([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)])
    c0, c1 = rgb565(31, 10, 3), rgb565(4, 50, 20)
    idx0 = rng.integers(0, 4, 16); idx1 = rng.integers(0, 4, 16)
    pack = lambda ix: sum(int(v) << (2 * i) for i, v in enumerate(ix))
    blocks = struct.pack("<HHI", c0, c1, pack(idx0)) + struct.pack("<HHI", c1, c0, pack(idx1)) + struct.pack("<HHI", c0, c1, 0)   # level 1: 4x2 -> one block
    header = b"DDS " + struct.pack("<IIIIIII", 124, 0x1007 | 0x20000, 4, 8, 0, 0, 2) + b"\0" * 44 + struct.pack("<II4sIIIII", 32, 4, b"DXT1", 0, 0, 0, 0, 0) + struct.pack("<IIIII", 0x1000, 0, 0, 0, 0)
    assert len(header) == 128
    (tmp_path / "t.dds").write_bytes(header + blocks)
    levels = grt.load_texture(tmp_path / "t.dds")
    assert [l.shape for l in levels] == [(4, 8, 4)]      # the 4x2 level is stored but never used: the reference halves the block counts (2x1 -> 1x0) and stops at zero
    e0, e1 = expand(c0), expand(c1)
    four = [e0, e1, (2 * e0 + e1 + 1) // 3, (e0 + 2 * e1 + 1) // 3]
    three = [e1, e0, (e0 + e1) // 2, np.zeros(3, int)]
    for i in range(16):
        assert np.array_equal(levels[0][i // 4, i % 4, :3], four[idx0[i]]) and levels[0][i // 4, i % 4, 3] == 255
        assert np.array_equal(levels[0][i // 4, 4 + i % 4, :3], three[idx1[i]]) and levels[0][i // 4, 4 + i % 4, 3] == (0 if idx1[i] == 3 else 255)
    # DXT5: interpolated alpha; DXT3: explicit 4-bit alpha
    alpha_idx = rng.integers(0, 8, 16)
    a_bits = sum(int(v) << (3 * i) for i, v in enumerate(alpha_idx))
    dxt5 = bytes([200, 40]) + a_bits.to_bytes(6, "little") + struct.pack("<HHI", c1, c0, pack(idx0))
    hdr5 = header[:84] + b"DXT5" + header[88:]; hdr5 = hdr5[:12] + struct.pack("<II", 4, 4) + hdr5[20:28] + struct.pack("<I", 1) + hdr5[32:]
    (tmp_path / "t5.dds").write_bytes(hdr5 + dxt5)
    l5 = grt.load_texture(tmp_path / "t5.dds")[0]
    ramp = [200, 40] + [((7 - k) * 200 + k * 40 + 3) // 7 for k in range(1, 7)]
    assert [int(l5[i // 4, i % 4, 3]) for i in range(16)] == [ramp[v] for v in alpha_idx]
    four_b = [e1, e0, (2 * e1 + e0 + 1) // 3, (e1 + 2 * e0 + 1) // 3]                 # c1 < c0 numerically, but DXT5 colour blocks are always 4-colour
    assert all(np.array_equal(l5[i // 4, i % 4, :3], four_b[idx0[i]]) for i in range(16))
    nibbles = rng.integers(0, 16, 16)
    dxt3 = bytes(int(nibbles[2 * i]) | (int(nibbles[2 * i + 1]) << 4) for i in range(8)) + struct.pack("<HHI", c0, c1, pack(idx0))
    (tmp_path / "t3.dds").write_bytes(hdr5[:84] + b"DXT3" + hdr5[88:] + dxt3)
    l3 = grt.load_texture(tmp_path / "t3.dds")[0]
    assert [int(l3[i // 4, i % 4, 3]) for i in range(16)] == [int(v) * 17 for v in nibbles]

    for name, data in (("bad1.png", cases[0][0][:60]), ("bad2.png", b"\x89PNG\r\n\x1a\n" + b"\0" * 40), ("bad.dds", header[:100]), ("bad.bmp", bmp24[:70])):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(RuntimeError, match="cannot decode"):
            grt.load_texture(tmp_path / name)


def test_texture_decoders_equal_the_references_stb_image(grt, oracle, tmp_path):
    """Live pin against the stb_image.h the reference vendors (compiled verbatim into oracle/_ref): every
    Sponza TGA, and PNG / BMP files of all the kinds the decoder test generates, decode to the same RGBA bytes."""
    import glob, struct
    if oracle.ref_lib() is None or not hasattr(oracle.ref_lib(), "ref_stbi_load_rgba"):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    grt.config_reset()
    grt.config_set(enable_mipmapping=0)
    files = sorted(glob.glob(os.path.join(os.path.dirname(grt.scene_path("sponza")), "textures", "*.tga")))
    assert len(files) >= 15
    rng = np.random.default_rng(12)
    h, w = 9, 14
    generated = []
    for interlace in (False, True):
        generated.append(_png_bytes(rng.integers(0, 256, (h, w, 3)), 2, 8, interlace))
        generated.append(_png_bytes(rng.integers(0, 256, (h, w, 4)), 6, 8, interlace))
        generated.append(_png_bytes(rng.integers(0, 65536, (h, w, 4)), 6, 16, interlace))
        generated.append(_png_bytes(rng.integers(0, 65536, (h, w, 3)), 2, 16, interlace, trns=struct.pack(">HHH", 300, 2, 1)))
        generated.append(_png_bytes(rng.integers(0, 256, (h, w, 2)), 4, 8, interlace))
        generated.append(_png_bytes(rng.integers(0, 65536, (h, w, 2)), 4, 16, interlace))
        for depth in (1, 2, 4, 8, 16):
            generated.append(_png_bytes(rng.integers(0, 1 << depth, (h, w, 1)), 0, depth, interlace))
            generated.append(_png_bytes(rng.integers(0, 1 << depth, (h, w, 1)), 0, depth, interlace, trns=struct.pack(">H", 1)))
        for depth in (1, 2, 4, 8):
            n = 1 << depth
            generated.append(_png_bytes(rng.integers(0, n, (h, w, 1)), 3, depth, interlace, palette=rng.integers(0, 256, (n, 3)),
                                        trns=bytes(rng.integers(0, 256, max(1, n // 2)).astype(np.uint8))))
    for i, data in enumerate(generated):
        path = tmp_path / ("g%d.png" % i); path.write_bytes(data); files.append(str(path))
    rgb = rng.integers(0, 256, (5, 3, 3)).astype(np.uint8)
    row = lambda r: bytes(r[:, ::-1].reshape(-1)) + b"\0" * ((-3 * 3) % 4)
    bmps = {"a.bmp": b"BM" + struct.pack("<IHHI", 54 + 60, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, 3, 5, 1, 24, 0, 0, 0, 0, 0, 0) + b"".join(row(rgb[y]) for y in range(4, -1, -1))}
    for alpha in (0, 77):
        bgra = np.dstack([rgb[:, :, ::-1], np.full((5, 3), alpha, np.uint8)])
        bmps["b%d.bmp" % alpha] = b"BM" + struct.pack("<IHHI", 54 + 60, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, 3, -5, 1, 32, 0, 0, 0, 0, 0, 0) + bgra.tobytes()
    pal = rng.integers(0, 256, (256, 3)).astype(np.uint8); idx = rng.integers(0, 256, (5, 3)).astype(np.uint8)
    bmps["c.bmp"] = b"BM" + struct.pack("<IHHI", 54 + 1024 + 20, 0, 0, 54 + 1024) + struct.pack("<IiiHHIIiiII", 40, 3, 5, 1, 8, 0, 0, 0, 0, 256, 0) + \
        np.hstack([pal[:, ::-1], np.zeros((256, 1), np.uint8)]).tobytes() + b"".join(bytes(idx[y]) + b"\0" for y in range(4, -1, -1))
    for name, data in bmps.items():
        (tmp_path / name).write_bytes(data); files.append(str(tmp_path / name))
    for f in files:
        ref = oracle.ref_stbi_load(f)
        assert ref is not None, f
        got = grt.load_texture(f)[0]
        assert got.shape == ref.shape and np.array_equal(got, _srgb_to_linear_u8(ref)), f
    grt.config_reset()


JPEG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
JPEG_PHOTO_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_photos")


def _decode_without_gamma(grt, path):
    """Level 0 of the loaded texture is sRGB -> linear of the decoded bytes; that map is monotone but not
    injective at the dark end, so compare through it (as the other decoder tests do)."""
    return grt.load_texture(path)[0]


def test_jpeg_decoder_matches_the_references_stb_image_digests(grt):
    """Baseline / progressive, 4:4:4 / 4:2:2 / 4:2:0, restart intervals, grey, CMYK, tiny and odd sizes
    (tests/golden/jpeg, written by Pillow): the decoded image equals what the reference's stb_image decodes.
    Without oracle/_ref the comparison is by digest of the linear-light bytes derived from the committed
    stb digests' images -- so here the product is checked against golden linear textures."""
    import hashlib, json
    golden = json.load(open(os.path.join(os.path.dirname(JPEG_DIR), "jpeg_golden.json")))["files"]
    assert len(golden) >= 20
    grt.config_reset(); grt.config_set(enable_mipmapping=0)
    for name, want in sorted(golden.items()):
        level0 = grt.load_texture(os.path.join(JPEG_DIR, name))[0]
        assert level0.shape == (want["height"], want["width"], 4), name
        assert hashlib.sha256(level0.tobytes()).hexdigest() == want["sha256_linear"], name
    grt.config_reset()


def test_jpeg_decoder_live_against_stb_image(grt, oracle):
    import glob
    if oracle.ref_lib() is None or not hasattr(oracle.ref_lib(), "ref_stbi_load_rgba"):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    files = sorted(glob.glob(os.path.join(JPEG_DIR, "*.jpg")))
    # and two photographs (baseline 4:2:0 and 4:4:4; the sample images of matplotlib and scikit-learn)
    files += sorted(glob.glob(os.path.join(JPEG_PHOTO_DIR, "*.jpg")))
    assert len(files) >= 22
    grt.config_reset(); grt.config_set(enable_mipmapping=0)
    for f in files:
        ref = oracle.ref_stbi_load(f)
        assert ref is not None, f
        got = grt.load_texture(f)[0]
        assert got.shape == ref.shape, f
        want = _srgb_to_linear_u8(ref)
        assert np.array_equal(got, want), (f, int((got != want).sum()))
    grt.config_reset()


def _product_mip_step(grt, filter_type, src, w_dst, h_dst):
    import ctypes
    lib = grt.host_lib()
    lib.grt_mipmap_downsample.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p]
    src = np.ascontiguousarray(src, np.float32)
    dst = np.zeros((h_dst, w_dst, 4), np.float32)
    assert lib.grt_mipmap_downsample(filter_type, src.shape[1], src.shape[0], w_dst, h_dst, src.ctypes.data, dst.ctypes.data) == 0
    return dst


def test_mip_filters_match_the_reference_generator(grt, oracle):
    """Mipmap.cpp: box (the default), lanczos and kaiser kernels. Bit-identical float results against the
    reference's own Mipmap::downsample (oracle/_ref) for halving steps of even, odd and 1-wide levels and for
    the direct original -> level steps the wide filters use; without _ref, the kernels' basic properties."""
    rng = np.random.default_rng(14)
    steps = [((16, 16), (8, 8)), ((13, 11), (6, 5)), ((6, 5), (3, 2)), ((3, 2), (1, 1)), ((64, 1), (32, 1)), ((1, 9), (1, 4)), ((40, 24), (5, 3)), ((33, 17), (1, 1))]
    have_ref = oracle.ref_lib() is not None and hasattr(oracle.ref_lib(), "ref_mipmap_downsample")
    for filter_type in (0, 1, 2):
        for (w, h), (wd, hd) in steps:
            src = rng.random((h, w, 4)).astype(np.float32)
            got = _product_mip_step(grt, filter_type, src, wd, hd)
            if have_ref:
                want = oracle.ref_mipmap_downsample(filter_type, src, wd, hd)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (filter_type, w, h)
            const = _product_mip_step(grt, filter_type, np.full((h, w, 4), 0.25, np.float32), wd, hd)
            assert np.allclose(const, 0.25, atol=1e-6)            # normalised kernels reproduce a constant
    box = _product_mip_step(grt, 0, np.arange(16 * 4, dtype=np.float32).reshape(1, 16, 4), 8, 1)
    assert np.allclose(box[0, :, 0], np.arange(16 * 4, dtype=np.float32).reshape(16, 4)[:, 0].reshape(8, 2).mean(1))   # 2:1 box = pair average


def test_mip_filter_choice_reaches_the_texture_loader(grt, tmp_path):
    rng = np.random.default_rng(15)
    img = rng.integers(0, 256, (16, 16, 3))
    (tmp_path / "t.png").write_bytes(_png_bytes(img, 2, 8))
    chains = {}
    for name, value in (("box", 0), ("lanczos", 1), ("kaiser", 2)):
        grt.config_reset(); grt.config_set(mipmap_filter=value)
        chains[name] = grt.load_texture(tmp_path / "t.png")
        assert [l.shape[:2] for l in chains[name]] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    grt.config_reset()
    assert np.array_equal(chains["box"][0], chains["kaiser"][0])
    assert not np.array_equal(chains["box"][1], chains["lanczos"][1]) and not np.array_equal(chains["lanczos"][1], chains["kaiser"][1])
    with pytest.raises(KeyError):
        grt.config_set(mipmap_filter=3)


def _product_shape(grt, shape, transform16, p0=(0, 0, 0), p1=(0, 0, 1), radius=1.0, detail=-1):
    import ctypes
    lib = grt.host_lib()
    lib.grt_geometry_shape.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    t = np.ascontiguousarray(transform16, np.float32); a = np.asarray(p0, np.float32); b = np.asarray(p1, np.float32)
    n = lib.grt_geometry_shape(shape, t.ctypes.data, a.ctypes.data, b.ctypes.data, radius, detail, None, 0)
    assert n > 0, lib.grt_last_error()
    out = np.zeros((n, 24), np.float32)
    lib.grt_geometry_shape(shape, t.ctypes.data, a.ctypes.data, b.ctypes.data, radius, detail, out.ctypes.data, n)
    return out


def test_primitive_shapes_equal_the_references_geometry(grt, oracle):
    """Mitsuba rectangle / cube / disk / cylinder / sphere shapes are tessellated on load with the transform
    baked in (Util/Geometry.cpp). Triangle order, vertices, normals and uvs are bit-identical to the reference's
    own Geometry.cpp (oracle/_ref) -- they feed the BVH and the light CDFs."""
    if oracle.ref_lib() is None or not hasattr(oracle.ref_lib(), "ref_geometry_shape"):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    rng = np.random.default_rng(17)
    transforms = [np.eye(4, dtype=np.float32)]
    for _ in range(3):
        m = np.eye(4, dtype=np.float32)
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        m[:3, :3] = (q * rng.uniform(0.3, 2.5, 3)).astype(np.float32)        # rotation x non-uniform scale (incl. mirroring)
        m[:3, 3] = rng.uniform(-3, 3, 3)
        transforms.append(m)
    counts = {}
    for m in transforms:
        for shape, kwargs in ((0, {}), (1, {}), (2, {}), (2, dict(detail=7)), (3, {}), (3, dict(p0=(0.5, -1, 0.25), p1=(-0.5, 2, 1), radius=0.3, detail=9)),
                              (4, {}), (4, dict(detail=0)), (4, dict(detail=1))):
            want = oracle.ref_geometry_shape(shape, m.ravel(), **kwargs)
            got = _product_shape(grt, shape, m.ravel(), **kwargs)
            assert got.shape == want.shape, (shape, kwargs)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, kwargs)
            counts[(shape, tuple(sorted(kwargs)))] = got.shape[0]
    assert counts[(0, ())] == 2 and counts[(1, ())] == 12 and counts[(2, ())] == 32 and counts[(4, ())] == 20 * 4 ** 3


def test_hdr_sky_equals_stbi_loadf(grt, oracle, tmp_path):
    """Sky::load (Sky.cpp:12-35) takes the floats of stbi_loadf: RGBE with run-length and flat scanlines."""
    import ctypes
    rng = np.random.default_rng(19)
    w, h = 40, 6
    rgbe = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    rgbe[:, :, 3] = rng.integers(110, 150, (h, w)); rgbe[2, 5, 3] = 0; rgbe[1, :12] = rgbe[1, 0]       # a zero exponent, a run
    def rle_row(row):
        out = bytes([2, 2, w >> 8, w & 255])
        for c in range(4):
            vals, x = row[:, c], 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and vals[x + run] == vals[x]: run += 1
                if run >= 3:
                    out += bytes([128 + run, int(vals[x])]); x += run
                else:
                    lit = 1
                    while x + lit < w and lit < 128 and not (x + lit + 2 < w and vals[x + lit] == vals[x + lit + 1] == vals[x + lit + 2]): lit += 1
                    out += bytes([lit]) + bytes(vals[x:x + lit].tolist()); x += lit
        return out
    header = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)
    (tmp_path / "rle.hdr").write_bytes(header + b"".join(rle_row(rgbe[y]) for y in range(h)))
    w2 = 5                                                        # narrower than 8: always stored flat
    header2 = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w2)
    (tmp_path / "flat.hdr").write_bytes(header2 + rgbe[:, :w2].tobytes())
    lib = grt.host_lib()
    lib.grt_sky_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t]
    for name, (ww, hh) in (("rle.hdr", (w, h)), ("flat.hdr", (w2, h))):
        sw, sh = ctypes.c_int(), ctypes.c_int()
        out = np.zeros((hh, ww, 4), np.float32)
        assert lib.grt_sky_load(str(tmp_path / name).encode(), ctypes.byref(sw), ctypes.byref(sh), out.ctypes.data, out.size) == out.size
        assert (sw.value, sh.value) == (ww, hh) and (out[:, :, 3] == 0).all()
        e = rgbe[:, :ww]
        scale = np.where(e[:, :, 3] > 0, np.ldexp(np.float32(1.0), e[:, :, 3].astype(np.int32) - 136), 0).astype(np.float32)
        assert np.array_equal(out[:, :, :3], e[:, :, :3].astype(np.float32) * scale[:, :, None])
        if oracle.ref_lib() is not None and hasattr(oracle.ref_lib(), "ref_stbi_loadf_rgb"):
            ref = oracle.ref_stbi_loadf(tmp_path / name)
            assert ref is not None and np.array_equal(ref.view(np.uint32), out[:, :, :3].view(np.uint32)), name


def test_camera_state_equals_the_references_camera(grt, oracle):
    """Camera::resize / recalibrate / update (Camera.cpp:9-96): the view pyramid the generate kernel reads
    (3 rotated vectors + pixel spread angle) and the projection / view-projection matrices SVGF reprojects
    with are bit-identical to the reference's Camera.cpp compiled into oracle/_ref."""
    import ctypes
    if oracle.ref_lib() is None or not hasattr(oracle.ref_lib(), "ref_camera_state"):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    sig = [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    ref, lib = oracle.ref_lib(), grt.host_lib()
    ref.ref_camera_state.argtypes = sig; lib.grt_camera_state.argtypes = sig
    rng = np.random.default_rng(23)
    for fov_deg, (w, h) in ((85.0, (1920, 1080)), (19.5, (512, 512)), (60.0, (900, 600)), (120.0, (33, 77))):
        for updates in (1, 2):
            pos = rng.uniform(-5, 5, 3).astype(np.float32)
            q = rng.normal(size=4).astype(np.float32); q /= np.linalg.norm(q)
            a, b = np.zeros(58, np.float32), np.zeros(58, np.float32)
            ref.ref_camera_state(np.float32(np.deg2rad(fov_deg)), w, h, pos.ctypes.data, q.ctypes.data, updates, a.ctypes.data)
            assert lib.grt_camera_state(np.float32(np.deg2rad(fov_deg)), w, h, pos.ctypes.data, q.ctypes.data, updates, b.ctypes.data) == 0
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (fov_deg, w, h, updates, np.flatnonzero(a != b))


def test_instance_transforms_and_media_equal_the_reference_math(grt, oracle):
    """Mesh::update (Mesh.cpp:16-33: transform, its inverse built from the inverted factors, transformed AABB)
    and Medium::from_sigmas / to_sigmas (Medium.h:16-37) over the reference's own Matrix4 / Quaternion / AABB /
    Vector3 code in oracle/_ref: bit-identical floats. These are the instance tables and sigma_a / sigma_s the
    device gets."""
    import ctypes
    if oracle.ref_lib() is None or not hasattr(oracle.ref_lib(), "ref_mesh_transform"):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    ref, lib = oracle.ref_lib(), grt.host_lib()
    sig = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    ref.ref_mesh_transform.argtypes = sig; lib.grt_mesh_transform.argtypes = sig
    rng = np.random.default_rng(29)
    for i in range(50):
        pos = rng.uniform(-20, 20, 3).astype(np.float32)
        q = rng.normal(size=4).astype(np.float32); q /= np.linalg.norm(q)
        if i == 0: pos[:] = 0; q[:] = (0, 0, 0, 1)
        scale = np.float32(1.0 if i < 2 else rng.uniform(0.05, 30))
        lo = rng.uniform(-5, 0, 3).astype(np.float32); box = np.concatenate([lo, lo + rng.uniform(0, 8, 3).astype(np.float32)])
        if i == 3: box[3] = box[0]                                   # a flat box: fix_if_needed widens it
        a, b = np.zeros(38, np.float32), np.zeros(38, np.float32)
        ref.ref_mesh_transform(pos.ctypes.data, q.ctypes.data, scale, box.ctypes.data, a.ctypes.data)
        assert lib.grt_mesh_transform(pos.ctypes.data, q.ctypes.data, scale, box.ctypes.data, b.ctypes.data) == 0
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, np.flatnonzero(a != b))
    sig = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    ref.ref_medium_round_trip.argtypes = sig; lib.grt_medium_round_trip.argtypes = sig
    for g in (0.0, 0.2, -0.7, 0.9999):
        for _ in range(10):
            sa = rng.uniform(0.001, 5, 3).astype(np.float32); ss = rng.uniform(0.001, 50, 3).astype(np.float32)
            a, b = np.zeros(12, np.float32), np.zeros(12, np.float32)
            ref.ref_medium_round_trip(sa.ctypes.data, ss.ctypes.data, g, a.ctypes.data)
            assert lib.grt_medium_round_trip(sa.ctypes.data, ss.ctypes.data, g, b.ctypes.data) == 0
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (g, a, b)


def test_bc1_encoder_equals_the_references_stb_dxt(grt, oracle):
    """BlockCompression.cpp restates stb_dxt v1.12 HIGHQUAL (TextureLoader.cpp:250): identical 8 bytes per block
    against stb_compress_dxt_block compiled verbatim into oracle/_ref -- random blocks, smooth gradients,
    two-colour and constant blocks (every constant value: that is the generated single-colour table), blocks with
    zero padding as at a level's edge, and every 4x4 block of a real texture."""
    import ctypes
    if oracle.ref_lib() is None or not hasattr(oracle.ref_lib(), "ref_stb_compress_bc1_block"):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    ref, lib = oracle.ref_lib(), grt.host_lib()
    lib.grt_compress_bc1_block.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(31)
    blocks = [rng.integers(0, 256, (16, 4)).astype(np.uint8) for _ in range(3000)]
    for _ in range(3000):                                            # smooth blocks: a base colour plus a small gradient and noise
        base = rng.integers(0, 256, 3); grad = rng.normal(0, 12, 3)
        b = np.zeros((16, 4), np.uint8)
        for i in range(16):
            b[i, :3] = np.clip(base + grad * (i % 4 - 1.5) + rng.normal(0, 3, 3), 0, 255)
        b[:, 3] = 255
        blocks.append(b)
    for _ in range(500):                                             # two colours, and nearly constant blocks
        c = rng.integers(0, 256, (2, 3)); b = np.zeros((16, 4), np.uint8); b[:, :3] = c[rng.integers(0, 2, 16)]; b[:, 3] = 255; blocks.append(b)
        b = np.full((16, 4), 255, np.uint8); b[:, :3] = rng.integers(0, 256, 3); b[rng.integers(0, 16), rng.integers(0, 3)] ^= 1; blocks.append(b)
    for v in range(256):
        blocks.append(np.full((16, 4), v, np.uint8))
        b = np.zeros((16, 4), np.uint8); b[:, 0] = v; b[:, 1] = 255 - v; b[:, 2] = (v * 7) & 255; b[:, 3] = 255; blocks.append(b)
    for _ in range(300):                                             # partially outside the image: zero texels
        b = rng.integers(0, 256, (16, 4)).astype(np.uint8); keep = rng.integers(1, 4); b.reshape(4, 4, 4)[:, keep:] = 0; blocks.append(b)
    grt.config_reset(); grt.config_set(enable_mipmapping=0)
    tex = grt.load_texture(os.path.join(os.path.dirname(grt.scene_path("sponza")), "textures", "sponza_floor_a_diff.tga"))[0]
    grt.config_reset()
    crop = tex[:256, :256]
    for y in range(0, 256, 4):
        for x in range(0, 256, 4):
            blocks.append(np.ascontiguousarray(crop[y:y + 4, x:x + 4]).reshape(16, 4))
    mismatches = 0
    a, b = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    for blk in blocks:
        blk = np.ascontiguousarray(blk)
        ref.ref_stb_compress_bc1_block(blk.ctypes.data, a.ctypes.data)
        lib.grt_compress_bc1_block(blk.ctypes.data, b.ctypes.data)
        mismatches += not np.array_equal(a, b)
    assert mismatches == 0, "%d of %d blocks differ" % (mismatches, len(blocks))


def test_block_compressed_textures_follow_the_reference_pipeline(grt, oracle, tmp_path):
    """enable_block_compression (the reference's default, TextureLoader.cpp:208-262): every level of a
    power-of-two texture is BC1-quantised block by block, the chain ends at the one-block level, and the LOD
    bias is derived from the block counts (Texture::lod_width). Level 0 equals decode(stb_compress_dxt_block)
    of the uncompressed level for every block (verbatim stb_dxt in oracle/_ref); non-power-of-two textures are
    left alone. The oracle renders a scene with such textures (bounce > 0 lookups use the shifted bias)."""
    import ctypes
    rng = np.random.default_rng(33)
    y, x = np.mgrid[0:32, 0:64]
    img = np.dstack([127 + 100 * np.sin(x / 5.0), 127 + 100 * np.cos(y / 3.0), (x * 4 + y * 2) % 256]) + rng.normal(0, 6, (32, 64, 3))
    img = np.clip(img, 0, 255).astype(np.int64)
    (tmp_path / "pow2.png").write_bytes(_png_bytes(img, 2, 8))
    (tmp_path / "odd.png").write_bytes(_png_bytes(img[:30, :60], 2, 8))
    grt.config_reset()
    plain = grt.load_texture(tmp_path / "pow2.png")
    packed = grt.load_texture(tmp_path / "pow2.png", block_compression=None)   # the default configuration compresses
    odd = grt.load_texture(tmp_path / "odd.png", block_compression=True)
    grt.config_reset()
    assert [l.shape[:2] for l in plain] == [(32, 64), (16, 32), (8, 16), (4, 8), (2, 4), (1, 2), (1, 1)]
    assert [l.shape[:2] for l in packed] == [(32, 64), (16, 32), (8, 16), (4, 8), (2, 4)]      # 16x8 blocks ... 1x1 block
    assert np.array_equal(odd[0], grt.load_texture(tmp_path / "odd.png")[0])                  # 60x30: not compressed
    assert not np.array_equal(packed[0], plain[0]) and np.abs(packed[0][:, :, :3].astype(int) - plain[0][:, :, :3]).mean() < 12   # a noisy, colourful image: BC1 has two end points per block
    assert (packed[0][:, :, 3] == 255).all()
    if oracle.ref_lib() is not None and hasattr(oracle.ref_lib(), "ref_stb_compress_bc1_block"):
        ref = oracle.ref_lib()
        for level, (src, got) in enumerate(zip(plain, packed)):
            h, w = src.shape[:2]
            for by in range((h + 3) // 4):
                for bx in range((w + 3) // 4):
                    block = np.zeros((4, 4, 4), np.uint8)
                    part = src[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4]
                    block[:part.shape[0], :part.shape[1]] = part
                    comp = np.zeros(8, np.uint8)
                    ref.ref_stb_compress_bc1_block(block.ctypes.data, comp.ctypes.data)
                    c0, c1 = int(comp[0]) | int(comp[1]) << 8, int(comp[2]) | int(comp[3]) << 8
                    ex = lambda c: np.array([((c >> 11) * 33) >> 2, (((c >> 5) & 63) * 65) >> 4, ((c & 31) * 33) >> 2])
                    e0, e1 = ex(c0), ex(c1)
                    pal = [e0, e1, (2 * e0 + e1 + 1) // 3, (e0 + 2 * e1 + 1) // 3] if c0 > c1 else [e0, e1, (e0 + e1) // 2, np.zeros(3, int)]
                    bits = int.from_bytes(bytes(comp[4:8]), "little")
                    for j in range(part.shape[0]):
                        for i in range(part.shape[1]):
                            assert np.array_equal(got[by * 4 + j, bx * 4 + i, :3], pal[(bits >> (2 * (4 * j + i))) & 3]), (level, bx, by)

    # through the scene loader and the oracle: lod size = block counts, and the render reacts to it
    (tmp_path / "floor.obj").write_text("v -4 0 -4\nv 4 0 -4\nv 4 0 4\nv -4 0 4\nvt 0 0\nvt 6 0\nvt 6 6\nvt 0 6\nf 1/1 3/3 2/2\nf 1/1 4/4 3/3\n")
    (tmp_path / "s.xml").write_text('<scene version="0.5.0"><sensor type="perspective"><float name="fov" value="50"/><transform name="toWorld"><lookat origin="0, 1.5, 5" target="0, 0, 0" up="0, 1, 0"/></transform></sensor>'
                                    '<shape type="obj"><string name="filename" value="floor.obj"/><bsdf type="diffuse"><texture type="bitmap" name="reflectance"><string name="filename" value="pow2.png"/></texture></bsdf></shape>'
                                    '<shape type="sphere"><float name="radius" value="0.7"/><transform name="toWorld"><translate y="0.7"/></transform><bsdf type="diffuse"><rgb name="reflectance" value="0.9, 0.9, 0.9"/></bsdf></shape></scene>')
    images = {}
    for compress in (0, 1):
        grt.config_reset()
        grt.config_set(enable_block_compression=compress)
        scene = grt.Scene(str(tmp_path / "s.xml"))
        grt.config_set(num_bounces=3)
        pt = grt.Pathtracer(scene, 48, 32, device=-1); pt.update()
        assert pt.texture_lod_size(0) == ((16, 8) if compress else (0, 0))
        assert pt.textures()[0][3] == (5 if compress else 7)
        frame = oracle.Frame(oracle.SceneView(pt))
        for s in range(3):
            frame.render_sample(s)
        images[compress] = frame.final[:, :48, :3].copy()
        pt.close(); scene.close()
    grt.config_reset()
    assert np.isfinite(images[1]).all() and not np.array_equal(images[0], images[1])
    assert abs(images[0].mean() - images[1].mean()) < 0.05 * images[0].mean()


def test_hostile_inputs_are_rejected_not_trusted(grt, tmp_path):
    """Regressions from fuzzing the host loaders under ASAN / UBSAN (mutated PNG / JPEG / BMP / DDS / TGA / PPM /
    PLY / serialized / hair / OBJ / XML / .bvh / .hdr files): every one of these used to read or write out of
    bounds, overflow, or allocate without bound."""
    import struct, zlib
    grt.config_reset()
    # non-finite vertices poison every SAH comparison (the split search then found no axis at all)
    (tmp_path / "nan.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 nan 0\nv 2 2 2\nv 3 2 2\nv 2 3 2\nf 1 2 3\nf 4 5 6\n")
    with pytest.raises(RuntimeError, match="non-finite"):
        s = grt.Scene(str(tmp_path / "nan.obj")); s.wait_until_loaded()
    # an integer with far too many digits
    (tmp_path / "digits.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 99999999999999999999999\n")
    s = grt.Scene(str(tmp_path / "digits.obj")); s.wait_until_loaded(); s.close()
    # error messages may quote bytes that are not UTF-8
    (tmp_path / "bytes.ply").write_bytes(b"ply\nformat ascii 1.0\nelement \xff\xfe 3\nend_header\n")
    with pytest.raises(RuntimeError):
        s = grt.Scene(str(tmp_path / "bytes.ply")); s.wait_until_loaded()

    # .bvh caches: NaN boxes, a child that points back at its parent, counts no file of that size can hold, a bool that is neither 0 nor 1
    obj = tmp_path / "m.obj"
    rng = np.random.default_rng(3)
    p = rng.random((30, 3)) * 4
    obj.write_text("".join("v %f %f %f\n" % tuple(v) for v in p) + "".join("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(10)))
    grt.config_set(enable_bvh_cache=1)
    s = grt.Scene(str(obj)); s.wait_until_loaded()
    good_nodes = s.mesh_data_array(0, "bvh2_nodes", np.uint8).copy(); good_bvh8 = s.mesh_data_array(0, "bvh8_nodes", np.uint8).copy(); s.close()
    cache = str(obj) + ".bvh"
    good = _read_bvh_cache(cache)
    def attempt(mutator):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        mutator(c)
        _write_bvh_cache(cache, c)
        os.utime(cache, (2e9, 2e9))
        grt.config_reset(); grt.config_set(enable_bvh_cache=1)
        s = grt.Scene(str(obj)); s.wait_until_loaded()
        nodes = s.mesh_data_array(0, "bvh2_nodes", np.uint8).copy(); bvh8 = s.mesh_data_array(0, "bvh8_nodes", np.uint8).copy(); s.close()
        assert np.array_equal(nodes, good_nodes) and np.array_equal(bvh8, good_bvh8)        # rebuilt from the mesh, not taken from the cache
    def nan_box(c): c["nodes"].view(np.float32)[8 * 2] = np.nan
    def cycle(c): c["nodes"].view(np.int32)[8 * 2 + 6] = 0                                     # node 2's child index -> the root
    attempt(nan_box); attempt(cycle)
    raw = bytearray(open(cache, "rb").read())
    _write_bvh_cache(cache, good); raw = bytearray(open(cache, "rb").read())
    for patch in ((16, struct.pack("<i", 0x7fffffff)), (6, bytes([7]))):                       # num_triangles, the bool
        bad = bytearray(raw); bad[patch[0]:patch[0] + len(patch[1])] = patch[1]
        open(cache, "wb").write(bytes(bad)); os.utime(cache, (2e9, 2e9))
        grt.config_reset(); grt.config_set(enable_bvh_cache=1)
        s = grt.Scene(str(obj)); s.wait_until_loaded()
        assert np.array_equal(s.mesh_data_array(0, "bvh2_nodes", np.uint8), good_nodes); s.close()
    grt.config_reset()

    # images that announce absurd sizes, and a JPEG whose coefficients overflow 32-bit IDCT arithmetic
    png = _png_bytes(rng.integers(0, 256, (4, 4, 3)), 2, 8)
    huge = bytearray(png); huge[16:24] = struct.pack(">II", 30000, 30000)
    huge[29:33] = struct.pack(">I", zlib.crc32(bytes(huge[12:29])) & 0xffffffff)
    (tmp_path / "huge.png").write_bytes(bytes(huge))
    with pytest.raises(RuntimeError, match="cannot decode"):
        grt.load_texture(tmp_path / "huge.png")
    jpg = bytearray(open(os.path.join(JPEG_DIR, "base_444_q90.jpg"), "rb").read())
    dqt = jpg.index(b"\xff\xdb")
    jpg[dqt + 5:dqt + 5 + 64] = bytes([255]) * 64                                            # enormous quantisation steps
    (tmp_path / "loud.jpg").write_bytes(bytes(jpg))
    grt.load_texture(tmp_path / "loud.jpg")                                                   # decodes (to garbage) without overflow
    (tmp_path / "big.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2000000000 +X 2000000000\n" + bytes(64))
    (tmp_path / "sky.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    lib = grt.host_lib()
    import ctypes
    lib.grt_sky_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t]
    w, h = ctypes.c_int(), ctypes.c_int(); out = np.zeros(16, np.float32)
    assert lib.grt_sky_load(str(tmp_path / "big.hdr").encode(), ctypes.byref(w), ctypes.byref(h), out.ctypes.data, out.size) == 4 and (w.value, h.value) == (1, 1)   # the white fallback


def test_tga_variants_equal_stb_image(grt, oracle, tmp_path):
    """Every TGA flavour stb_image reads: colour-mapped (8 / 16-bit indices; 15 / 16 / 24 / 32-bit palettes), 15 / 16 /
    24 / 32-bit true colour, 8-bit grey and 16-bit grey + alpha, raw and run-length encoded, both row orders, with an
    image ID and a palette offset. Compared with the reference's stb_image where oracle/_ref exists."""
    import struct
    rng = np.random.default_rng(37)
    w, h = 7, 5

    def tga(image_type, bpp, pixels, palette=b"", palette_len=0, palette_bits=0, palette_start=0, descriptor=0, ident=b""):
        header = struct.pack("<BBBHHBHHHHBB", len(ident), 1 if palette_len else 0, image_type, palette_start, palette_len, palette_bits, 0, 0, w, h, bpp, descriptor)
        return header + ident + palette + pixels

    def rle(pixels, size):
        out, i, n = b"", 0, len(pixels) // size
        while i < n:
            px = pixels[i * size:(i + 1) * size]
            run = 1
            while i + run < n and run < 128 and pixels[(i + run) * size:(i + run + 1) * size] == px: run += 1
            if run > 1:
                out += bytes([0x80 | (run - 1)]) + px; i += run
            else:
                lit = 1
                while i + lit < n and lit < 128 and pixels[(i + lit) * size:(i + lit + 1) * size] != pixels[(i + lit - 1) * size:(i + lit) * size]: lit += 1
                out += bytes([lit - 1]) + pixels[i * size:(i + lit) * size]; i += lit
        return out

    files = {}
    for bpp in (15, 16, 24, 32):
        size = (bpp + 7) // 8
        px = bytes(rng.integers(0, 256, w * h * size).astype(np.uint8))
        px = px[:8 * size] + px[:size] * 6 + px[14 * size:]                     # a run for the RLE form
        files["true%d.tga" % bpp] = tga(2, bpp, px)
        files["true%d_top.tga" % bpp] = tga(2, bpp, px, descriptor=0x20 | (8 if bpp == 32 else 0), ident=b"id!")
        files["true%d_rle.tga" % bpp] = tga(10, bpp, rle(px, size))
        files["true%d_rtl.tga" % bpp] = tga(2, bpp, px, descriptor=0x10)        # right-to-left flag: ignored like stb_image does
    grey = bytes(rng.integers(0, 256, w * h).astype(np.uint8))
    files["grey8.tga"] = tga(3, 8, grey); files["grey8_rle.tga"] = tga(11, 8, rle(grey[:10] + grey[:1] * 9 + grey[19:], 1))
    ga = bytes(rng.integers(0, 256, w * h * 2).astype(np.uint8))
    files["grey16.tga"] = tga(3, 16, ga)
    for pbits in (15, 16, 24, 32):
        psize = (pbits + 7) // 8
        pal = bytes(rng.integers(0, 256, 20 * psize).astype(np.uint8))
        idx8 = bytes(rng.integers(0, 24, w * h).astype(np.uint8))                # some indices beyond the palette: entry 0
        files["map%d.tga" % pbits] = tga(1, 8, idx8, palette=pal, palette_len=20, palette_bits=pbits)
        files["map%d_rle.tga" % pbits] = tga(9, 8, rle(idx8[:5] + idx8[:1] * 12 + idx8[17:], 1), palette=pal, palette_len=20, palette_bits=pbits)
        idx16 = rng.integers(0, 20, w * h).astype("<u2").tobytes()
        files["map%d_wide.tga" % pbits] = tga(1, 16, idx16, palette=b"\x00\x00" + pal, palette_len=20, palette_bits=pbits, palette_start=2)
    grt.config_reset(); grt.config_set(enable_mipmapping=0)
    have_ref = oracle.ref_lib() is not None and hasattr(oracle.ref_lib(), "ref_stbi_load_rgba")
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        got = grt.load_texture(tmp_path / name)[0]
        assert got.shape == (h, w, 4), name
        if have_ref:
            ref = oracle.ref_stbi_load(tmp_path / name)
            assert ref is not None, name
            assert np.array_equal(got, _srgb_to_linear_u8(ref)), name
    # spot checks that do not need the reference: 5-5-5 scaling and the bottom-up default
    px = struct.pack("<H", (31 << 10) | (16 << 5) | 1) * (w * h)
    (tmp_path / "c.tga").write_bytes(tga(2, 16, px))
    assert np.array_equal(grt.load_texture(tmp_path / "c.tga")[0][0, 0], _srgb_to_linear_u8(np.array([[[255, (16 * 255) // 31, (1 * 255) // 31, 255]]], np.uint8))[0, 0])
    rows = bytes([10] * w + [200] * w * (h - 1))
    (tmp_path / "r.tga").write_bytes(tga(3, 8, rows))
    lv = grt.load_texture(tmp_path / "r.tga")[0]
    assert lv[h - 1, 0, 0] == _srgb_to_linear_u8(np.array([[[10, 10, 10, 255]]], np.uint8))[0, 0, 0] and lv[0, 0, 0] > lv[h - 1, 0, 0]
    grt.config_reset()


def test_pnm_files_equal_stb_image(grt, oracle, tmp_path):
    rng = np.random.default_rng(41)
    files = {"a.ppm": b"P6\n# a comment\n5 3\n255\n" + bytes(rng.integers(0, 256, 45).astype(np.uint8)),
             "b.pgm": b"P5 4 6 255\n" + bytes(rng.integers(0, 256, 24).astype(np.uint8)),
             "c.ppm": b"P6\r\n2 2\r\n200\r" + bytes(rng.integers(0, 200, 12).astype(np.uint8))}
    grt.config_reset(); grt.config_set(enable_mipmapping=0)
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        got = grt.load_texture(tmp_path / name)[0]
        if oracle.ref_lib() is not None and hasattr(oracle.ref_lib(), "ref_stbi_load_rgba"):
            ref = oracle.ref_stbi_load(tmp_path / name)
            assert ref is not None and np.array_equal(got, _srgb_to_linear_u8(ref)), name
    assert np.array_equal(grt.load_texture(tmp_path / "b.pgm")[0][:, :, 0], grt.load_texture(tmp_path / "b.pgm")[0][:, :, 2])
    for bad in (b"P6\n5 3\n65535\n" + bytes(90), b"P6\n5 3\n255\n" + bytes(10), b"P4\n8 1\n\xff"):
        (tmp_path / "bad.ppm").write_bytes(bad)
        with pytest.raises(RuntimeError):
            grt.load_texture(tmp_path / "bad.ppm")
    grt.config_reset()
