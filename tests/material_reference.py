"""numpy float64 restatement of the material launch (kernels_shade.hip: shade_material and the tail of next-event estimation; the reference's
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
pdf_is_valid (bsdf_reference.py's replay: `near`). An entry is non-robust when one of them is within its margin."""
import numpy as np

import bsdf_reference
import nee_reference
from sort_reference import DIFFUSE, DIELECTRIC, _normalize, _oct_encode

DIM_BSDF_0, DIM_BSDF_1, DIM_NEE_LIGHT, DIM_NEE_TRIANGLE = 5, 6, 3, 4   # Sampling.h:30-42
EPSILON = float(np.float32(1e-4))
INVALID = -1
# A dot product of two float32 unit vectors is three products and two sums: at most eight roundings of 2^-24 each on terms of size <= 1,
# on top of the unit vectors' own (each component within 2^-24 relative of its float64 value after a normalisation of three roundings).
DOT_MARGIN = 16 * 2.0 ** -24
PDF_MARGIN = 1e-5   # relative, around pdf_is_valid's 1e-4: the light pdf is distance^2 / cosine, some twenty float32 operations


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


def evaluate(world, tables, launch, bsdf_tables):
    """The launch in float64. Per entry (N): alive (the set-up keeps it), continues, has_shadow, robust and the near_* masks; normal,
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
        normal = np.where(entering[:, None], normal, -normal); curvature = np.where(entering, curvature, -curvature)
        omega_i_z = _dot(-d, normal)
        alive = omega_i_z > 0
        r.near_entering = ~(np.abs(facing) > DOT_MARGIN * sliver)
        r.near_alive = np.abs(omega_i_z) <= DOT_MARGIN
        r.alive, r.entering, r.normal, r.position, r.geometric_normal = alive, entering, normal, position, gn
        term = 2.0 * curvature * np.abs(width) / _dot(normal, d)
        r.cone_width, r.cone_angle = width, angle_in - term
        r.cone_angle_scale = np.abs(angle_in) + np.abs(term) * (1.0 + 1.0 / np.abs(_dot(normal, d)))

        # g-buffers (SVGF.cu as kernels_shade.hip: svgf_set_gbuffers)
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
        throughput_in = np.where(first[:, None], 1.0, e.throughput.astype(f64))
        svgf_first = (cfg["enable_svgf"] != 0) & first
        albedo = materials[:, :3].astype(f64)
        if kind == bsdf_reference.DIFFUSE:   # calc_albedo: the diffuse BSDF's albedo goes into the throughput at once, unless SVGF demodulates the first hit
            throughput = np.where(svgf_first[:, None], throughput_in, throughput_in * albedo)
        else:
            throughput = throughput_in
        uniforms = [tables.random(DIM_BSDF_0, real, bounce, sample), tables.random(DIM_BSDF_1, real, bounce, sample)]
        probes = _probes(materials, normal, d, entering, real, sample, bounce)
        s64, _ = bsdf_reference.evaluate(kind, probes, bsdf_tables, eval=False, uniforms=uniforms)
        r.near_sample = alive & s64.near
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
        nee = (cfg["enable_next_event_estimation"] != 0) and tables.lights_total_weight > 0.0
        r.has_shadow = np.zeros(n, bool); r.near_light = np.zeros(n, bool)
        r.shadow_origin = np.full((n, 3), np.nan); r.shadow_direction = np.full((n, 3), np.nan); r.shadow_distance = np.full(n, np.nan); r.illumination = np.full((n, 3), np.nan)
        if nee and n:
            rl, rt = tables.random(DIM_NEE_LIGHT, real, bounce, sample), tables.random(DIM_NEE_TRIANGLE, real, bounce, sample)
            light = nee_reference.sample_lights(nee_reference.Tables(tables.view), np.concatenate([rl, rt], axis=1))
            hit = _offset(position, light.point - position, gn)
            light_point = _offset(light.point, hit - light.point, light.normal)
            to_light = light_point - hit
            distance = np.sqrt((to_light * to_light).sum(axis=1))
            to_light = to_light / distance[:, None]
            cos_light = np.abs(_dot(to_light, light.normal))
            cos_hit = _dot(to_light, normal)
            power = f64(np.float32(0.299)) * light.emission[:, 0] + f64(np.float32(0.587)) * light.emission[:, 1] + f64(np.float32(0.114)) * light.emission[:, 2]
            light_pdf = power * distance * distance / (cos_light * tables.lights_total_weight)
            e_probes = _probes(materials, normal, d, entering, real, sample, bounce, to_light=to_light, cos_o=cos_hit)
            e64, _ = bsdf_reference.evaluate(kind, e_probes, bsdf_tables, eval=True)
            valid = np.isfinite(light_pdf) & (light_pdf > 1e-4)
            allowed = alive & s64.allow_nee
            r.has_shadow = allowed & (e64.ok == 1) & valid
            # (the sides of the two epsilon offsets follow two more dot products)
            r.near_light = allowed & (e64.near | (np.abs(cos_hit) <= DOT_MARGIN) | (np.abs(light_pdf - 1e-4) <= PDF_MARGIN * 1e-4 * (1.0 + 1.0 / cos_light))
                                      | ~(np.abs(_dot(light.point - position, gn)) > DOT_MARGIN * sliver * distance)
                                      | ~(np.abs(_dot(hit - light.point, light.normal)) > DOT_MARGIN * distance))
            weight = light_pdf ** 2 / (light_pdf ** 2 + e64.pdf ** 2) if cfg["enable_multiple_importance_sampling"] else 1.0
            illumination = throughput * e64.value * light.emission * np.asarray(weight)[..., None] / light_pdf[:, None]
            r.shadow_origin, r.shadow_direction, r.shadow_distance = hit, to_light, distance
            r.illumination = np.where(textured[:, None], np.nan, illumination)
            r.light_pdf = light_pdf
    r.textured = textured
    r.near = r.near_entering | r.near_alive | r.near_sample | r.near_light
    r.robust = ~r.near
    return r


def reference_of(world, tables, launch):
    """evaluate, once per launch and setup (the tests share it)."""
    cached = getattr(launch, "_reference", None)
    if cached is None or cached[0] is not tables:   # (the tables object itself is kept: an id could be reused)
        launch._reference = (tables, evaluate(world, tables, launch, world.bsdf_tables))
    return launch._reference[1]

