"""numpy float64 restatement of the material launch (rt_material.h: shade_material, and rt_lights.h: the tail of next-event estimation; the reference's
shade_material and next_event_estimation, Pathtracer.cu:465-757 as oracle_pathtrace.cpp cites them) on the records of rt_shade_rays, for
test_material.py (oracle against this) and test_gpu_material.py (device against this). Vectorised over the entries of one launch; float32
inputs are taken exactly, every operation is float64.

New here, written from the model: the surface set-up (interpolation, world transform, inverse scale, geometric normal, the entering
flip), ray-cone propagation (width, angle, the curvature term and its flip), the tail of next-event estimation (both epsilon offsets, the
light pdf, the MIS weight, the illumination), the g-buffer projection, and which words of a record are written. Composed from the modules
that already restate them: the BSDFs' sample and eval (bsdf_reference.py, on a probe built from this set-up), the light selection
(nee_reference.py), the octahedral encoding and the frames' layout (sort_reference.py). The random numbers are the oracle's
(test_random_samples_are_bit_exact holds them equal to the device's).

Not restated: the albedo fetch of a textured material and its footprint. texture_reference.py defines a fetch on float32 positions that
the caller hands it (its contract), and the float32 position of a float64 footprint is not the kernel's; textured hits are therefore held
to this reference in everything but their albedo, throughput and illumination, and to the oracle in those (material_checks.py).

`evaluate` also says how close every deciding comparison of an entry comes to its threshold: entering_material (dot(direction, geometric
normal) < 0), omega_i.z <= 0, cos_theta_hit <= 0 and pdf_is_valid(light_pdf) of the light sample, and the BSDF's own branches and
pdf_is_valid (bsdf_reference.py's replay: `near`). An entry is non-robust when one of them is within its margin.

The variants of the launch (rt_material.h: the _sky and _nmap instances), composed from the modules that restate their parts:
* a sky share s = tables.sky_share > 0 (next_event_estimation<1>): each allowed entry is routed in float32 as the kernel routes it -- to the
  sky where DIM_NEE_LIGHT.x < s, else to the emitters on the rescaled number min((u - s) / (1 - s), 0x1.fffffep-1), whose light pdf carries
  the factor 1 - s into pdf_is_valid and into the MIS weight. A sky entry takes its direction and cell pdf from the DIM_NEE_TRIANGLE pair
  through the sky's tables (sky_sampling_reference.py), its radiance from sample_sky, light_pdf = s x pdf, valid when positive and finite,
  and an infinite max_distance. With s >= 1 (a share of 1, or no emitters) every entry goes to the sky and no light table is read;
* normal maps (the NMAP branch of shade_material): `map_ids`, one map per material (-1: none), and `map_texels`, per map its constant texel
  (three bytes) or "varied". A mapped hit of a constant map shades with normal_map_reference.perturb on that texel -- every filter and level
  of a constant 8-bit image returns it, so no fetch is restated -- in the BSDF frame, omega_i.z <= 0, next-event estimation, the NORMAL
  frame and the g-buffer; the ray cone's curvature term and its dot(normal, direction) keep the interpolated normal. A hit of a varied map
  has no reference value here (`varied`; rt_perturb_normals holds those) and counts as left out.
* delta lights (the _split instances, next_event_estimation<2>): `tables.delta`, a Delta -- the table of delta_light_reference.py, the P_k and the CDF
  as the device holds them, and the upload's share. The shares settle as delta_light_reference.split settles them and every allowed entry is
  routed by delta_light_reference.route, in float32: to the sky below s, to a delta light below taken = s + q, else to the emitters on
  (u - taken) / (1 - taken), whose pdf carries 1 - taken. A delta entry: the light from the CDF on (u - s) / q, one epsilon offset towards it
  (against its direction for a directional light), the sample of delta_light_reference.sample from that origin, pdf q P_k, no MIS weight, and
  a max_distance of +inf exactly for a directional light;
* the light tree (the _tree instances, next_event_estimation<3>): `tables.tree`, a TreeTables -- the scene, the tree and the leaves' areas as
  the device holds them (light_tree_reference.py). The routing is the _split instances' (taken may be 0); an emitter entry takes the leaf the
  descent picks from the hit point on (u', DIM_NEE_LIGHT.y), the point on it from the DIM_NEE_TRIANGLE pair, and
  pdf = pmf d^2 / (A cos) (1 - taken). The tree is not in force without emitters, with NEE off or under a fog volume.
`route` says per entry where its light sample goes (ROUTE_SKY, ROUTE_DELTA, ROUTE_POWER, ROUTE_TREE).
* a fog volume (`tables.fog_active`): shade_material takes bounce 0's throughput from the queue, as every other bounce's.
Their deciding comparisons carry near flags of their own (near_sky, near_map; near_light takes in the routes' edges, a spot's two cosines, the
sliver margin of the offset towards a delta light, and a descent of the tree that a few ulps of u would turn), counted like the others."""
import numpy as np

import bsdf_reference
import delta_light_reference
import light_tree_reference
import nee_reference
import normal_map_reference
import sky_sampling_reference
from sort_reference import DIFFUSE, DIELECTRIC, _normalize, _oct_encode

DIM_BSDF_0, DIM_BSDF_1, DIM_NEE_LIGHT, DIM_NEE_TRIANGLE = 5, 6, 3, 4   # Sampling.h:30-42
EPSILON = float(np.float32(1e-4))
INVALID = -1
# A dot product of two float32 unit vectors is three products and two sums: at most eight roundings of 2^-24 each on terms of size <= 1,
# on top of the unit vectors' own (each component within 2^-24 relative of its float64 value after a normalisation of three roundings).
DOT_MARGIN = 16 * 2.0 ** -24
PDF_MARGIN = 1e-5   # relative, around pdf_is_valid's 1e-4: the light pdf is distance^2 / cosine, some twenty float32 operations
ONE_BELOW_ONE = np.float32(np.nextafter(np.float32(1), np.float32(0)))   # 0x1.fffffep-1
# How close to a border of its sky cell (in cells) a direction may lie before the float32 atan2f / acosf of sky_cell may find the neighbour:
# their error is a few 2^-24 of a turn, times the 64 to 1024 cells of a row.
SKY_CELL_MARGIN = 1e-4
T_LENGTH_MARGIN = 1e-3   # relative, around normal_map_perturb's |t|^2 > 1e-8 |dpdu|^2
# A sampled direction that grazes the shading plane: G2's `o_back` decides on the sign of omega_o.z, the diffuse lobe and the pdf are proportional
# to it, so its float32 error of about 2^-23 is DOT_MARGIN / |omega_o.z| of the throughput. bsdf_checks.py calls |omega_o.z| < 1e-3 grazing and holds
# the value there to 1 only. A mapped normal leans against the surface, and the view guard pins omega_i.z at 1e-2 for every hit it moves: such
# samples, rare in an unmapped launch, are a few per thousand mapped hits. They are flagged (mapped hits only) and left out.
GRAZING = 1e-3
ROUTE_SKY, ROUTE_DELTA, ROUTE_POWER, ROUTE_TREE = range(4)
ROUTE_NAMES = ("sky", "delta light", "emitter by power", "emitter by tree")
# A spot's c = dot(-to_light, axis) against its two cosines: the direction's float32 error grows with 1 / distance (test_gpu_delta_lights.py)
SPOT_MARGIN = 64 * 2.0 ** -24
# The epsilon offset towards a delta light follows the sign of dot(toward, geometric normal), `toward` not normalised
DELTA_SIDE_MARGIN = 64 * DOT_MARGIN


class Delta:
    """`tables.delta`: the delta lights in force. table: delta_light_reference.Table; share: rt_upload_delta_lights' (of what the sky leaves);
    records, cdf: rt_read_delta_lights' (without a device: the table's own numbers rounded to float32)."""

    def __init__(self, table, share, records=None, cdf=None):
        self.table, self.share = table, float(share)
        self.pdf32 = np.asarray(table.pdf if records is None else records[:, 7], np.float32)
        self.cdf32 = np.asarray(table.cdf if cdf is None else cdf, np.float32)


class TreeTables:
    """`tables.tree`: the light tree in force. scene: light_tree_reference.Scene; tree: the nodes as the device holds them (tree_from_nodes of
    rt_read_light_tree, or build32's without a device: bit-identical); leaf_area: float32 per leaf id."""

    def __init__(self, scene, tree, leaf_area):
        self.scene, self.tree, self.leaf_area = scene, tree, np.asarray(leaf_area, np.float32)


class Result:
    pass


def _rows(m, v):
    return np.einsum("nij,nj->ni", m[:, :, :3], v)


def _dot(a, b):
    return (a * b).sum(axis=1)


def _offset(origin, direction, geometric_normal):
    """ray_origin_epsilon_offset: along the geometric normal, to the side the direction leaves on."""
    side = np.sign(_dot(direction, geometric_normal))
    side = np.where(side == 0, 1.0, side)
    return origin + (side * EPSILON)[:, None] * geometric_normal


def _probes(materials, normal, direction, entering, pixel, sample, bounce, to_light=None, cos_o=None):
    """The 24-float records of bsdf_reference.py: the set-up as the kernel hands it to its BSDF."""
    n = normal.shape[0]
    p = np.zeros((n, 24), np.float32)
    p[:, bsdf_reference.MATERIAL] = materials
    p[:, bsdf_reference.NORMAL] = normal
    p[:, bsdf_reference.DIRECTION] = direction
    p[:, bsdf_reference.ENTERING] = entering
    if to_light is not None:
        p[:, bsdf_reference.TO_LIGHT] = np.nan_to_num(to_light)
        p[:, bsdf_reference.COS_O] = np.nan_to_num(cos_o)
    p[:, bsdf_reference.KEY].view(np.uint32)[:] = np.stack([pixel, sample, bounce], axis=1).astype(np.uint32)
    return p


def route(u, share):
    """Where next_event_estimation<1> sends a light sample, in float32 as the kernel computes it: (to the sky, the rescaled number of the
    emitters' half)."""
    u = np.asarray(u, np.float32); s = np.float32(share)
    with np.errstate(all="ignore"):
        rescaled = np.minimum(((u - s) / (np.float32(1) - s)).astype(np.float32), ONE_BELOW_ONE)
    return u < s, rescaled


def map_records(tri, u, v, world_m, direction):
    """The (N, 48) float64 records of normal_map_reference.frame / perturb for hits on (N, 24) triangles."""
    rec = np.zeros((tri.shape[0], normal_map_reference.PROBE_IN))
    rec[:, 0:24] = tri
    rec[:, 24], rec[:, 25] = u, v
    rec[:, 26:38] = world_m.reshape(-1, 12)
    rec[:, 38:41] = direction
    return rec


def settings_in_force(tables):
    """What decides the light variant of a launch, as sky_sampling_prepare and rt_light_tree_in_force settle it: (NEE on, the sky's share, emitters
    exist, tables.delta or None, tables.tree or None, a fog volume is in force). No delta lights with NEE off; no tree without NEE, without emitters, or under fog."""
    nee_on = tables.config["enable_next_event_estimation"] != 0
    share = np.float64(np.float32(tables.sky_share)) if nee_on else 0.0   # the _sky instances: RtParams::sky_nee_share
    lit = tables.lights_total_weight > 0.0
    fog = bool(getattr(tables, "fog_active", False))
    delta = getattr(tables, "delta", None) if nee_on else None
    tree = getattr(tables, "tree", None) if nee_on and lit and not fog else None
    return nee_on, share, lit, delta, tree, fog


def route_in_force(tables, route):
    """Whether light samples of a launch under `tables` can take `route`."""
    nee_on, share, lit, delta, tree, fog = settings_in_force(tables)
    taken = share
    if delta is not None or tree is not None:
        taken = np.float64(delta_light_reference.split(np.float32(share), delta.share if delta is not None else 0.0, lit)[2])
    return bool(nee_on and {ROUTE_SKY: share > 0.0, ROUTE_DELTA: delta is not None and taken > share, ROUTE_POWER: lit and taken < 1.0 and tree is None,
                            ROUTE_TREE: lit and taken < 1.0 and tree is not None}[route])


def evaluate(world, tables, launch, bsdf_tables, sky_directions=None, sky_pdfs=None, map_ids=None, map_texels=None):
    """The launch in float64. sky_directions (N, 3), sky_pdfs (N,): what to use in place of the reference's own inversion of the sky's
    tables for the tail of a sky entry, where finite (the device test hands over the direction a launch wrote, which it holds to the
    inversion separately, and rt_sky_pdf's value for it; an entry whose float64 cell has another pdf is flagged). map_ids, map_texels:
    the normal maps (default: tables.map_ids, tables.map_texels where a test has set them). Further fields with a sky share: to_sky (the
    route), u_emitter, sky_direction, sky_pdf, near_sky; with maps: mapped, varied, map_fallback, map_guarded, interpolated_normal, near_map.
     Per entry (N): alive (the set-up keeps it), continues, has_shadow, robust and the near_* masks; normal,
    position (what the NORMAL and POSITION frames get at bounce 0), gnd (N, 4), gid (N, 2), gsp (N, 2) (the g-buffer rows under SVGF);
    cone_width, cone_angle and cone_angle_scale (what the angle's error is relative to); direction, origin, pdf, throughput (NaN rows
    for a textured hit), medium, allow_nee of the continuation ray; shadow_origin, shadow_direction, shadow_distance, illumination
    (NaN rows for a textured hit); geometric_normal."""
    e, cfg, n = launch.entries, tables.config, launch.entries.n
    slot, real, bounce, sample, submission = launch.paths()
    kind = DIFFUSE + launch.slot
    f64 = np.float64
    r = Result()
    with np.errstate(all="ignore"):
        d = e.direction.astype(f64); t = e.t.astype(f64)
        tri = tables.triangles[e.triangle].astype(f64)
        p0, e1, e2, n0, ne1, ne2 = (tri[:, 3 * k:3 * k + 3] for k in range(6))
        u = (e.u16.astype(np.float32) / np.float32(65535.0)).astype(f64)[:, None]; v = (e.v16.astype(np.float32) / np.float32(65535.0)).astype(f64)[:, None]
        local = p0 + u * e1 + v * e2
        world_m = tables.transforms[e.mesh].astype(f64)
        position = _rows(world_m, local) + world_m[:, :, 3]
        normal = _normalize(_rows(world_m, n0 + u * ne1 + v * ne2))
        scale_inv = 1.0 / np.sqrt((world_m[:, 0, :3] ** 2).sum(axis=1))

        # ray cone (RayCone.h): the width grows by angle x t, the angle changes with the surface's curvature
        mip = cfg["enable_mipmapping"] != 0
        first = bounce == 0
        angle_in = np.where(first, tables.pixel_spread_angle, e.cone_angle.astype(f64))
        width = np.where(first, angle_in * t, e.cone_width.astype(f64) + angle_in * t)
        pe0, ne0 = e1 - e2, ne1 - ne2
        curvature = (_dot(ne1, e1) / _dot(e1, e1) + _dot(ne2, e2) / _dot(e2, e2) + _dot(ne0, pe0) / _dot(pe0, pe0)) / 3.0 * scale_inv

        we1, we2 = _rows(world_m, e1), _rows(world_m, e2)
        gn = np.cross(we1, we2)
        area = np.sqrt((gn * gn).sum(axis=1))
        gn = gn / area[:, None]
        # the cross product of two nearly parallel edges cancels: its float32 direction is off by the rounding error times this factor (1 for a right angle)
        sliver = np.sqrt((we1 * we1).sum(axis=1) * (we2 * we2).sum(axis=1)) / area
        facing = _dot(d, gn)
        entering = facing < 0
        interpolated = np.where(entering[:, None], normal, -normal); curvature = np.where(entering, curvature, -curvature)
        material_id = tables.material_ids[e.mesh]

        # the NMAP branch: the shading normal of a mapped hit; `interpolated` stays what the ray cone reads
        normal = interpolated
        map_ids = getattr(tables, "map_ids", None) if map_ids is None else map_ids
        map_texels = getattr(tables, "map_texels", None) if map_texels is None else map_texels
        r.mapped = np.zeros(n, bool); r.varied = np.zeros(n, bool); r.near_map = np.zeros(n, bool); r.map_fallback = np.zeros(n, bool); r.map_guarded = np.zeros(n, bool)
        if map_ids is not None and n:
            entry_map = np.asarray(map_ids, np.int32)[material_id]
            r.mapped = entry_map >= 0
            normal = interpolated.copy()
            for m in np.unique(entry_map[r.mapped]):
                at = np.nonzero(entry_map == m)[0]
                texel = map_texels[int(m)]
                if isinstance(texel, str):   # "varied": the fetch is not restated
                    r.varied[at] = True
                    continue
                rec = map_records(tri[at], u[at, 0], v[at, 0], world_m[at], d[at])
                c = np.asarray(texel, np.float64)[None, :3] / 255.0   # (the byte over 255, as texel_to_float has it within float32 rounding)
                shading, fallback, info = normal_map_reference.perturb(rec, np.repeat(c, at.size, axis=0))
                normal[at] = shading
                r.map_fallback[at] = fallback
                r.map_guarded[at] = info["fired"]   # the view guard moved the mapped normal
                fr = info["frame"]
                close_guard = np.abs(info["cos_view"] - normal_map_reference.EPS) <= DOT_MARGIN
                close_tangent = np.abs(fr["sin_tn"] ** 2 - 1e-8) <= T_LENGTH_MARGIN * 1e-8
                close_side = ~(np.abs(_dot(fr["ng"], fr["n"])) > DOT_MARGIN * sliver[at])
                degenerate = ~(np.isfinite(fr["det"]) & (fr["det"] != 0.0))
                r.near_map[at] = ~degenerate & (close_tangent | (~fallback & (close_guard | close_side)))
        r.interpolated_normal = interpolated
        omega_i_z = _dot(-d, normal)
        alive = omega_i_z > 0
        r.near_entering = ~(np.abs(facing) > DOT_MARGIN * sliver)
        r.near_alive = np.abs(omega_i_z) <= DOT_MARGIN
        r.alive, r.entering, r.normal, r.position, r.geometric_normal = alive, entering, normal, position, gn
        term = 2.0 * curvature * np.abs(width) / _dot(interpolated, d)
        r.cone_width, r.cone_angle = width, angle_in - term
        r.cone_angle_scale = np.abs(angle_in) + np.abs(term) * (1.0 + 1.0 / np.abs(_dot(interpolated, d)))

        # g-buffers (SVGF.cu as rt_surface.h: svgf_set_gbuffers)
        prev_m = tables.transforms_prev[e.mesh].astype(f64)
        position_prev = _rows(prev_m, local) + prev_m[:, :, 3]
        one = np.ones((n, 1))
        u_curr = np.concatenate([position, one], axis=1) @ tables.view_projection.astype(f64).T
        u_prev = np.concatenate([position_prev, one], axis=1) @ tables.view_projection_prev.astype(f64).T
        ox, oy = _oct_encode(normal)
        r.gnd = np.stack([ox, oy, u_curr[:, 2], u_prev[:, 2]], axis=1)
        r.gid = np.stack([e.mesh, e.triangle], axis=1)
        r.gsp = u_prev[:, :2] / u_prev[:, 3:4]

        # the BSDF, on the probe the set-up amounts to
        material_id = tables.material_ids[e.mesh]
        materials = tables.materials[material_id].copy()
        textured = world.textured_instance[e.mesh]
        if kind in (bsdf_reference.DIFFUSE, bsdf_reference.PLASTIC):
            materials[:, 3] = np.array([INVALID], np.int32).view(np.float32)[0]
        fog = settings_in_force(tables)[5]   # (the ..._fog sort instance has stored bounce 0's throughput too)
        throughput_in = e.throughput.astype(f64) if fog else np.where(first[:, None], 1.0, e.throughput.astype(f64))
        svgf_first = (cfg["enable_svgf"] != 0) & first
        albedo = materials[:, :3].astype(f64)
        if kind == bsdf_reference.DIFFUSE:   # calc_albedo: the diffuse BSDF's albedo goes into the throughput at once, unless SVGF demodulates the first hit
            throughput = np.where(svgf_first[:, None], throughput_in, throughput_in * albedo)
        else:
            throughput = throughput_in
        uniforms = [tables.random(DIM_BSDF_0, real, bounce, sample), tables.random(DIM_BSDF_1, real, bounce, sample)]
        probes = _probes(materials, normal, d, entering, real, sample, bounce)
        s64, _ = bsdf_reference.evaluate(kind, probes, bsdf_tables, eval=False, uniforms=uniforms)
        r.sample_probes, r.sample_factor = probes, s64.value   # (what a float32 restatement of the BSDF's sample is handed, and float64's answer)
        r.near_sample = alive & s64.near
        r.near_map |= r.mapped & ~r.map_fallback & alive & (s64.ok == 1) & (np.abs(_dot(s64.direction, normal)) < GRAZING)
        r.continues = alive & (s64.ok == 1)
        r.allow_nee = s64.allow_nee
        r.direction = s64.direction
        r.pdf = s64.pdf
        factor = np.ones((n, 3)) if kind == bsdf_reference.DIFFUSE else s64.value
        r.throughput = np.where(textured[:, None], np.nan, throughput * factor)
        r.origin = _offset(position, s64.direction, gn)
        r.near_origin = ~(np.abs(_dot(s64.direction, gn)) > 64 * DOT_MARGIN * sliver)   # the offset's side follows the sign of this dot product
        inside_in = np.where(e.inside, e.medium, INVALID)
        if kind == DIELECTRIC:   # a transmitted path enters the sphere's medium or leaves the one it was in; a reflected one keeps it
            reflected = _dot(s64.direction, normal) >= 0
            material_medium = materials[:, 0].view(np.int32)
            r.medium = np.where(reflected, inside_in, np.where(entering, material_medium, INVALID))
        else:
            r.medium = inside_in

        # next-event estimation (Pathtracer.cu:465-555): the light the random numbers select, then the tail
        nee_on, share, lit, delta, tree, fog = settings_in_force(tables)
        split = delta is not None or tree is not None   # the _split and _tree instances: three routes
        taken = share
        if split:
            s32, q32, taken32 = delta_light_reference.split(np.float32(share), delta.share if delta is not None else 0.0, lit)
            taken = f64(taken32)
        emitters = lit and taken < 1.0
        nee = nee_on and (lit or share > 0.0 or delta is not None)
        r.has_shadow = np.zeros(n, bool); r.near_light = np.zeros(n, bool); r.near_sky = np.zeros(n, bool); r.to_sky = np.zeros(n, bool)
        r.shadow_origin = np.full((n, 3), np.nan); r.shadow_direction = np.full((n, 3), np.nan); r.shadow_distance = np.full(n, np.nan); r.illumination = np.full((n, 3), np.nan)
        r.u_emitter = np.full(n, np.nan, np.float32); r.sky_direction = np.full((n, 3), np.nan); r.sky_pdf = np.full(n, np.nan); r.light_pdf = np.full(n, np.nan)
        r.route = np.full(n, ROUTE_TREE if tree is not None else ROUTE_POWER, np.int8); r.to_delta = np.zeros(n, bool)
        if nee and n:
            rl, rt = tables.random(DIM_NEE_LIGHT, real, bounce, sample), tables.random(DIM_NEE_TRIANGLE, real, bounce, sample)
            allowed = alive & s64.allow_nee
            to_sky = np.zeros(n, bool); to_delta = np.zeros(n, bool); near_route = np.zeros(n, bool)
            u_light = rl[:, 0].astype(f64)
            if split:
                where, u_delta, r.u_emitter = delta_light_reference.route(rl[:, 0], s32, q32, taken32)
                to_sky, to_delta = where == 0, where == 1
                rl = rl.copy(); rl[:, 0] = np.where(where == 2, r.u_emitter, 0.0)
                selection = f64(np.float32(1) - taken32)
                if q32 > 0:
                    near_route |= np.abs(u_light - taken) <= f64(np.spacing(taken32))
            elif share > 0.0:
                to_sky, r.u_emitter = route(rl[:, 0], share)
                if not emitters:
                    to_sky = np.ones(n, bool)
                rl = rl.copy(); rl[:, 0] = np.where(to_sky, 0.0, r.u_emitter)
            if not split:
                selection = f64(np.float32(1) - np.float32(share))   # `selection` of nee_connect<true>: 1.0f - share
            r.to_sky, r.to_delta = to_sky, to_delta
            r.route = np.where(to_sky, ROUTE_SKY, np.where(to_delta, ROUTE_DELTA, r.route)).astype(np.int8)

            # the emitters' half: the light the (rescaled) random numbers select, then both epsilon offsets
            origin = np.full((n, 3), np.nan); to_light = np.full((n, 3), np.nan); distance = np.full(n, np.nan); light_pdf = np.full(n, np.nan)
            radiance = np.full((n, 3), np.nan); near_half = np.zeros(n, bool)
            if emitters:
                if tree is not None:   # the leaf the descent picks from the un-offset hit point, the point on it as nee_pick_light takes it
                    leaf, pmf, robust_pick = light_tree_reference.pick_leaves(tree.tree, position, rl[:, 0], rl[:, 1])
                    light = light_tree_reference.lights_on_leaves(tree.scene, leaf, rt)
                else:
                    light = nee_reference.sample_lights(nee_reference.Tables(tables.view), np.concatenate([rl, rt], axis=1))
                hit = _offset(position, light.point - position, gn)
                light_point = _offset(light.point, hit - light.point, light.normal)
                to_light = light_point - hit
                distance = np.sqrt((to_light * to_light).sum(axis=1))
                to_light = to_light / distance[:, None]
                cos_light = np.abs(_dot(to_light, light.normal))
                power = f64(np.float32(0.299)) * light.emission[:, 0] + f64(np.float32(0.587)) * light.emission[:, 1] + f64(np.float32(0.114)) * light.emission[:, 2]
                if tree is not None:
                    light_pdf = pmf * distance * distance / (tree.leaf_area[leaf].astype(f64) * cos_light)
                else:
                    light_pdf = power * distance * distance / (cos_light * tables.lights_total_weight)
                if share > 0.0 or split:
                    light_pdf = light_pdf * selection
                valid = np.isfinite(light_pdf) & (light_pdf > 1e-4)
                origin, radiance = hit, light.emission
                # (the sides of the two epsilon offsets follow two more dot products)
                near_half = ((np.abs(light_pdf - 1e-4) <= PDF_MARGIN * 1e-4 * (1.0 + 1.0 / cos_light))
                             | ~(np.abs(_dot(light.point - position, gn)) > DOT_MARGIN * sliver * distance)
                             | ~(np.abs(_dot(hit - light.point, light.normal)) > DOT_MARGIN * distance))
                if tree is not None:
                    near_half |= ~robust_pick
                    r.tree_leaf = leaf
            else:
                valid = np.zeros(n, bool)

            # the delta lights' share: the light from the CDF, one offset on the hit's side, the sample the light offers that origin; no MIS weight
            if delta is not None:
                table = delta.table
                picked = delta_light_reference.select(delta.cdf32, np.where(to_delta, u_delta, 0.0))
                toward = np.where((table.type[picked] == delta_light_reference.DIRECTIONAL)[:, None], -table.direction[picked], table.position[picked] - position)
                delta_origin = _offset(position, toward, gn)
                smp = delta_light_reference.sample(table, picked, delta_origin)
                delta_pdf = f64(q32) * delta.pdf32[picked].astype(f64)
                near_delta = (((table.type[picked] == delta_light_reference.SPOT) & (smp.margin <= SPOT_MARGIN * (1.0 + 1.0 / np.maximum(smp.distance, 1e-3))))
                              | ~(np.abs(_dot(toward, gn)) > DELTA_SIDE_MARGIN * np.sqrt(_dot(toward, toward))))
                k = to_delta[:, None]
                origin = np.where(k, delta_origin, origin); to_light = np.where(k, smp.to_light, to_light); distance = np.where(to_delta, smp.distance, distance)
                light_pdf = np.where(to_delta, delta_pdf, light_pdf); valid = np.where(to_delta, smp.ok & np.isfinite(delta_pdf) & (delta_pdf > 0.0), valid)
                radiance = np.where(k, smp.radiance, radiance); near_half = np.where(to_delta, near_delta, near_half)
                r.delta_light = np.where(to_delta, picked, -1)

            # the sky's half: the direction and its cell's pdf from the DIM_NEE_TRIANGLE pair, one offset, a ray to infinity
            if share > 0.0:
                sky = tables.sky_tables
                own_direction, _, _, own_pdf = sky.invert(rt)
                r.sky_direction, r.sky_pdf = own_direction, own_pdf
                to_sky_direction, pdf_sky = own_direction, sky.pdf_of(own_direction)
                if sky_directions is not None:
                    given = np.isfinite(np.asarray(sky_directions, f64)).all(axis=1)
                    to_sky_direction = np.where(given[:, None], np.asarray(sky_directions, f64), own_direction)
                    pdf_sky = sky.pdf_of(to_sky_direction)
                sky_origin = _offset(position, to_sky_direction, gn)
                sky_light_pdf = share * pdf_sky
                sky_valid = np.isfinite(sky_light_pdf) & (sky_light_pdf > 0.0)
                uu = np.arctan2(-to_sky_direction[:, 2], to_sky_direction[:, 0]) / (2.0 * np.pi) + 0.5
                vv = np.arccos(np.clip(to_sky_direction[:, 1], -1.0, 1.0)) / np.pi
                on_border = np.zeros(n, bool)
                for c, cells in ((uu, sky.w), (vv, sky.h)):
                    x = c * cells
                    on_border |= np.abs(x - np.round(x)) <= SKY_CELL_MARGIN
                if sky_pdfs is not None:   # the cell rt_sky_pdf found for the written direction is not float64's
                    seen = np.asarray(sky_pdfs, f64)
                    on_border |= np.isfinite(seen) & ~(np.abs(seen - pdf_sky) <= 1e-5 * pdf_sky)
                one_ulp = f64(np.spacing(np.float32(share)))
                near_route |= (emitters | (delta is not None)) & (np.abs(u_light - share) <= one_ulp)
                near_sky_half = (on_border | ~(np.abs(_dot(to_sky_direction, gn)) > DOT_MARGIN * sliver))
                k = to_sky[:, None]
                origin = np.where(k, sky_origin, origin); to_light = np.where(k, to_sky_direction, to_light); distance = np.where(to_sky, np.inf, distance)
                light_pdf = np.where(to_sky, sky_light_pdf, light_pdf); valid = np.where(to_sky, sky_valid, valid)
                radiance = np.where(k, sky_sampling_reference.sample_sky(tables.sky, tables.sky_scale, to_sky_direction), radiance)
                near_half = np.where(to_sky, near_sky_half, near_half)
            near_half = near_half | near_route
            cos_margin = np.where(to_sky | to_delta, 4 * DOT_MARGIN, DOT_MARGIN)

            # the tail (nee_finish): the BSDF towards the sample, the MIS weight, the illumination
            cos_hit = _dot(to_light, normal)
            e_probes = _probes(materials, normal, d, entering, real, sample, bounce, to_light=to_light, cos_o=cos_hit)
            e64, _ = bsdf_reference.evaluate(kind, e_probes, bsdf_tables, eval=True)
            r.has_shadow = allowed & (e64.ok == 1) & valid
            r.near_light = allowed & (e64.near | (np.abs(cos_hit) <= cos_margin) | near_half)
            r.near_sky = r.near_light & to_sky
            weight = light_pdf ** 2 / (light_pdf ** 2 + e64.pdf ** 2) if cfg["enable_multiple_importance_sampling"] else 1.0
            if delta is not None:   # (no BSDF-sampled ray finds a delta light)
                weight = np.where(to_delta, 1.0, weight)
            illumination = throughput * e64.value * radiance * np.asarray(weight)[..., None] / light_pdf[:, None]
            r.shadow_origin, r.shadow_direction, r.shadow_distance = origin, to_light, distance
            r.illumination = np.where(textured[:, None], np.nan, illumination)
            r.light_pdf = light_pdf
            r.bsdf_pdf_to_light = e64.pdf
    r.textured = textured
    r.near = r.near_entering | r.near_alive | r.near_sample | r.near_light | r.near_map | r.varied
    r.robust = ~r.near
    return r



def reference_of(world, tables, launch):
    """evaluate, once per launch and setup (the tests share it)."""
    cached = getattr(launch, "_reference", None)
    if cached is None or cached[0] is not tables:   # (the tables object itself is kept: an id could be reused)
        launch._reference = (tables, evaluate(world, tables, launch, world.bsdf_tables))
    return launch._reference[1]



# ---- float32 restatement of the mapped normal (normal_map_perturb and the set-up that feeds it), operation by operation ---------------
# numpy float32 arithmetic is IEEE and unfused, as the kernels are built (-ffp-contract=off); sums run left to right as rt_math.h writes them.
# test_material.py measures this against float64 (material_checks.MEASURED["mapped_normal"]); the device is held to 4 x that.

_F = np.float32


def _dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross32(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _normalize32(a):
    inv = _F(1.0) / np.sqrt(_dot32(a, a))
    return a * inv[:, None]


def _m_direction32(m, v):
    return np.stack([(m[:, i, 0] * v[:, 0] + m[:, i, 1] * v[:, 1]) + m[:, i, 2] * v[:, 2] for i in range(3)], axis=1)


def mapped_normal32(triangles, u16, v16, transforms, direction, texel):
    """The shading normal shade_material<.., NMAP> hands its BSDF for hits of a constant map `texel` (three bytes), in float32: (N, 3)
    float32 and whether normal_map_perturb fell back. triangles (N, 24), transforms (N, 3, 4), direction (N, 3) float32."""
    tri = np.ascontiguousarray(triangles, _F); world = np.ascontiguousarray(transforms, _F); d = np.ascontiguousarray(direction, _F)
    with np.errstate(all="ignore"):
        u = (u16.astype(_F) / _F(65535.0))[:, None]; v = (v16.astype(_F) / _F(65535.0))[:, None]
        e1, e2, n0, ne1, ne2 = tri[:, 3:6], tri[:, 6:9], tri[:, 9:12], tri[:, 12:15], tri[:, 15:18]
        duv1, duv2 = tri[:, 20:22], tri[:, 22:24]
        n = _normalize32(_m_direction32(world, (n0 + u * ne1) + v * ne2))
        det = duv1[:, 0] * duv2[:, 1] - duv2[:, 0] * duv1[:, 1]
        dpdu = _m_direction32(world, (duv2[:, 1:2] * e1 - duv1[:, 1:2] * e2) / det[:, None])
        gn = _cross32(_m_direction32(world, e1), _m_direction32(world, e2))
        gn = gn * (_F(1.0) / np.sqrt(_dot32(gn, gn)))[:, None]
        entering = _dot32(d, gn) < 0
        t = dpdu - n * _dot32(n, dpdu)[:, None]
        t2 = _dot32(t, t)
        fallback = ~((det != 0) & np.isfinite(det)) | ~((t2 > _F(1e-8) * _dot32(dpdu, dpdu)) & np.isfinite(t2))
        t = t / np.sqrt(t2)[:, None]
        b = _cross32(n, t)
        b = np.where(((det < 0) != (_dot32(gn, n) < 0))[:, None], -b, b)
        c = np.asarray(texel, np.uint8).astype(_F)[:3] * (_F(1.0) / _F(255.0))   # texel_to_float
        x = _F(2.0) * c - _F(1.0)
        m = (x[0] * t + x[1] * b) + x[2] * n
        m2 = _dot32(m, m)
        fallback |= ~(m2 > 0)
        m = m / np.sqrt(m2)[:, None]
        m = np.where(entering[:, None], m, -m)
        w = -d
        cos_view = _dot32(m, w)
        eps = _F(normal_map_reference.EPS)
        guarded = _normalize32(m + (eps - cos_view)[:, None] * w)
        m = np.where((cos_view < eps)[:, None], guarded, m)
        plain = np.where(entering[:, None], n, -n)
    return np.where(fallback[:, None], plain, m).astype(_F), fallback
