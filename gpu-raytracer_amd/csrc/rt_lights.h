// rt_lights.h -- next event estimation (Pathtracer.cu:465-555): the light sample of a hit or of a fog scatter vertex, by the power tables, the sky's
// tables, the delta lights' table or the light tree. For the material kernels (rt_material.h), the ..._fog sort instances (kernels_sort.hip: fog_vertex_light_sample),
// the AO integrator's shadow ray record (kernels_generate.hip) and the probes (kernels_probes.hip).
#pragma once
#include "rt_surface.h"
#include "rt_fog.h"   // henyey_greenstein (PhaseHG)

// The two cumulative tables of light sampling, copied into LDS by the workgroup when they fit (Sponza: 2 meshes, 480 triangles):
// the two binary searches are chains of ~2 + ~9 dependent loads per hit, each a round trip to L2 from a kernel that runs 3-4 waves
// per SIMD; from LDS a step costs a twentieth of that. Same floats, same comparisons.
#ifndef RT_LIGHT_TABLES_LDS
#define RT_LIGHT_TABLES_LDS 1
#endif
#define RT_LIGHT_MESHES_IN_LDS    64
#define RT_LIGHT_TRIANGLES_IN_LDS 2048
struct LightTablesLDS { float mesh_cdf[RT_LIGHT_MESHES_IN_LDS]; float triangle_cdf[RT_LIGHT_TRIANGLES_IN_LDS]; };
RT_DEV bool light_tables_fit_lds(const RtParams & p) { return p.light_mesh_count <= RT_LIGHT_MESHES_IN_LDS && p.light_triangle_count <= RT_LIGHT_TRIANGLES_IN_LDS; }
RT_DEV void light_tables_to_lds(const RtParams & p, LightTablesLDS & lds) {   // whole workgroup; the caller's next barrier publishes the copy
	if (!light_tables_fit_lds(p)) return;
	for (int i = threadIdx.x; i < p.light_mesh_count;     i += blockDim.x) lds.mesh_cdf[i]     = p.light_mesh_cumulative_probability[i];
	for (int i = threadIdx.x; i < p.light_triangle_count; i += blockDim.x) lds.triangle_cdf[i] = p.light_triangle_cumulative_probability[i];
}
typedef const __attribute__((address_space(3))) float * LdsFloatTable;   // (typed: ds_read_b32, not a FLAT load)

RT_DEV int sample_light(const RtParams & p, const LightTablesLDS * lds, float u1, float u2, int & transform_id) { // Sampling.h:180-190
	const bool from_lds = lds != nullptr && light_tables_fit_lds(p);   // uniform
	int light_mesh_id = from_lds ? binary_search((LdsFloatTable)lds->mesh_cdf, 0, p.light_mesh_count - 1, u1)
	                             : binary_search(p.light_mesh_cumulative_probability, 0, p.light_mesh_count - 1, u1);
	transform_id = p.light_mesh_transform_indices[light_mesh_id];
	if (p.mesh_position) transform_id = p.mesh_position[transform_id]; // device-built TLAS: the host only knows scene indices
	int2 span = p.light_mesh_triangle_span[light_mesh_id];
	int light_triangle_id = from_lds ? binary_search((LdsFloatTable)lds->triangle_cdf, span.x, span.y, u2)
	                                 : binary_search(p.light_triangle_cumulative_probability, span.x, span.y, u2);
	return p.light_triangle_indices[light_triangle_id];
}

struct ShadowRay { f3 origin, direction; float max_distance; f3 illumination; };

// The light sample of a hit: a point on an emitter chosen by the two cumulative tables, in world space, with the emitter's normal and emission.
// It depends on the path's random numbers alone, not on the surface. (Measured, profiles/r04_shade_stage.txt 5.: taking it BEFORE the surface
// set-up, so that its loads run beside the hit's own chain, changes nothing -- the material kernels are not waiting on that chain.)
struct LightSample { f3 point, geometric_normal, emission; };
RT_DEV LightSample nee_pick_light(const RtParams & p, const LightTablesLDS * light_lds, f2 rand_light, f2 rand_triangle) {
	int light_mesh_id;
	int light_triangle_id = sample_light(p, light_lds, rand_light.x, rand_light.y, light_mesh_id);
	f2 light_uv = sample_triangle(rand_triangle.x, rand_triangle.y);

	f3 p0, e1, e2;
	triangle_get_positions(p, light_triangle_id, p0, e1, e2);
	LightSample light;
	light.point = barycentric(light_uv.x, light_uv.y, p0, e1, e2);
	light.geometric_normal = cross(e1, e2);

	const float4 * light_world = p.mesh_transforms + size_t(light_mesh_id) * 3;
	light.point = m_position(light_world, light.point);
	light.geometric_normal = normalize(m_direction(light_world, light.geometric_normal));

	int light_material_id = p.mesh_material_ids[light_mesh_id];
	light.emission = mk3(p.materials[2 * light_material_id]);
	return light;
}

// The tail of every light sample: the BSDF towards it, the MIS weight, the shadow ray. `light_pdf` is the sample's pdf in solid angle; an emitter's
// has to pass pdf_is_valid (the reference's rule), the sky's only has to be positive and finite (the BSDF-miss side weighs every sky direction).
// DELTA: a delta light -- `light_pdf` is the probability of having picked it, and no BSDF-sampled ray can find it: the MIS weight is 1.
template<bool EMITTER, bool DELTA = false, typename BSDF>
RT_DEV bool nee_finish(const RtParams & p, const BSDF & bsdf, f3 origin, f3 to_light, float max_distance, float cos_theta_hit, f3 radiance, float light_pdf, f3 throughput, ShadowRay & shadow) {
	f3 bsdf_value; float bsdf_pdf;
	if (!bsdf.eval(p, to_light, cos_theta_hit, bsdf_value, bsdf_pdf)) return false;
	if (EMITTER ? !pdf_is_valid(light_pdf) : !(light_pdf > 0.0f && isfinite(light_pdf))) return false;

	float mis_weight = !DELTA && p.config.enable_multiple_importance_sampling ? power_heuristic(light_pdf, bsdf_pdf) : 1.0f;
	shadow.illumination = throughput * bsdf_value * radiance * mis_weight / light_pdf;
	shadow.origin = origin;
	shadow.direction = to_light;
	shadow.max_distance = max_distance;
	return true;
}

// Connects a hit with its light sample. Returns true and fills `shadow` when the sample has to be traced (the caller appends it).
// `selection`: the probability that the light sample went to the emitters (1 - the sky's share; 1 without sky sampling).
template<bool SKY, typename BSDF>
RT_DEV bool nee_connect(const RtParams & p, const LightSample & light, const BSDF & bsdf, f3 hit_point, f3 normal, f3 geometric_normal, f3 throughput, float selection, ShadowRay & shadow) {
	f3 light_point = light.point, light_geometric_normal = light.geometric_normal;
	hit_point   = ray_origin_epsilon_offset(hit_point,   light_point - hit_point, geometric_normal);
	light_point = ray_origin_epsilon_offset(light_point, hit_point - light_point, light_geometric_normal);

	f3 to_light = light_point - hit_point;
	float distance_to_light = length(to_light);
	to_light /= distance_to_light;

	float cos_theta_light = abs_dot(to_light, light_geometric_normal);
	float cos_theta_hit = dot(to_light, normal);

	f3 emission = light.emission;
	float light_power = luminance(emission.x, emission.y, emission.z);
	float light_pdf   = light_power * square(distance_to_light) / (cos_theta_light * p.lights_total_weight);
	if (SKY) light_pdf *= selection;
	return nee_finish<true>(p, bsdf, hit_point, to_light, distance_to_light, cos_theta_hit, emission, light_pdf, throughput, shadow);
}
// The light tree's light sample: the triangle by a descent of the tree from the un-offset hit point (u, and u2 once u is used up), the point on it from
// rand_triangle as nee_pick_light takes it; pdf = pmf d^2 / (A cos) x selection, A the triangle's world area. False without a leaf of positive power.
template<typename BSDF>
RT_DEV bool nee_connect_tree(const RtParams & p, const BSDF & bsdf, f3 hit_point, f3 normal, f3 geometric_normal, f3 throughput, float selection, float u, float u2, f2 rand_triangle, ShadowRay & shadow) {
	const LightTreePick pick = light_tree_sample(p.light_tree, hit_point.x, hit_point.y, hit_point.z, u, u2);
	if (pick.slot < 0) return false;
	const float4 leaf = p.light_tree.leaves[p.light_tree.leaf_of_slot[pick.slot - (p.light_tree.padded - 1)]];
	int light_mesh_id = p.light_mesh_transform_indices[__float_as_int(leaf.x)];
	if (p.mesh_position) light_mesh_id = p.mesh_position[light_mesh_id];
	f2 light_uv = sample_triangle(rand_triangle.x, rand_triangle.y);
	f3 p0, e1, e2;
	triangle_get_positions(p, __float_as_int(leaf.y), p0, e1, e2);
	const float4 * light_world = p.mesh_transforms + size_t(light_mesh_id) * 3;
	f3 light_point = m_position(light_world, barycentric(light_uv.x, light_uv.y, p0, e1, e2));
	f3 light_geometric_normal = normalize(m_direction(light_world, cross(e1, e2)));
	f3 emission = mk3(p.materials[2 * p.mesh_material_ids[light_mesh_id]]);

	hit_point   = ray_origin_epsilon_offset(hit_point,   light_point - hit_point, geometric_normal);
	light_point = ray_origin_epsilon_offset(light_point, hit_point - light_point, light_geometric_normal);
	f3 to_light = light_point - hit_point;
	float distance_to_light = length(to_light);
	to_light /= distance_to_light;
	float cos_theta_light = abs_dot(to_light, light_geometric_normal);
	float cos_theta_hit = dot(to_light, normal);
	float light_pdf = pick.pmf * square(distance_to_light) / (leaf.z * cos_theta_light) * selection;
	return nee_finish<true>(p, bsdf, hit_point, to_light, distance_to_light, cos_theta_hit, emission, light_pdf, throughput, shadow);
}
// The sky as the light sample (sky importance sampling): a direction from the sky's tables, traced to infinity.
template<typename BSDF>
RT_DEV bool nee_connect_sky(const RtParams & p, const BSDF & bsdf, f3 hit_point, f3 normal, f3 geometric_normal, f3 throughput, f2 rand_direction, ShadowRay & shadow) {
	float sky_pdf_value;
	f3 to_sky = sky_sample_direction(p, rand_direction.x, rand_direction.y, sky_pdf_value);
	f3 origin = ray_origin_epsilon_offset(hit_point, to_sky, geometric_normal);
	return nee_finish<false>(p, bsdf, origin, to_sky, RT_INFINITY, dot(to_sky, normal), sample_sky(p, to_sky), p.sky_nee_share * sky_pdf_value, throughput, shadow);
}
// ---- delta emitters ----
RT_DEV int nee_pick_delta(const RtParams & p, float u) { return binary_search(p.delta_light_cdf, 0, p.delta_light_count - 1, u); }
// Where the light lies as seen from `point` (not normalised): what the hit's epsilon offset is decided by.
RT_DEV f3 delta_light_toward(const RtDeltaLight & light, f3 point) {
	return __float_as_int(light.position_type.w) == RT_DELTA_LIGHT_DIRECTIONAL ? -mk3(light.direction_pdf) : mk3(light.position_type) - point;
}
// The sample a delta light offers `origin`: unit direction, the shadow ray's length, and the radiance term (intensity x falloff / d^2, or the
// irradiance). False -- drop the sample -- when the distance is 0 or not finite, the falloff is 0 or the term is not finite.
struct DeltaSample { f3 to_light; float max_distance; f3 radiance; };
RT_DEV bool delta_light_sample(const RtDeltaLight & light, f3 origin, DeltaSample & sample) {
	const int type = __float_as_int(light.position_type.w);
	f3 intensity = mk3(light.intensity_cos_cutoff);
	if (type == RT_DELTA_LIGHT_DIRECTIONAL) {
		sample.to_light = -mk3(light.direction_pdf);
		sample.max_distance = RT_INFINITY;
		sample.radiance = intensity;
	} else {
		f3 to_light = mk3(light.position_type) - origin;
		float d = length(to_light);
		if (!(d > 0.0f && isfinite(d))) return false;
		to_light /= d;
		float falloff = 1.0f;
		if (type == RT_DELTA_LIGHT_SPOT) {   // Mitsuba's: full inside the beam, none outside the cutoff, linear in the ANGLE between
			float c = dot(-to_light, mk3(light.direction_pdf));
			if (c <= light.intensity_cos_cutoff.w && light.intensity_cos_cutoff.w > -1.0f) return false;   // (a cutoff of pi, cosine -1, excludes no direction: not the back axis either)
			if (c < light.spot.x) falloff = (light.spot.y - acosf(c)) * light.spot.z;
			if (!(falloff > 0.0f)) return false;
		}
		sample.to_light = to_light;
		sample.max_distance = d;
		sample.radiance = intensity * falloff / square(d);
	}
	return isfinite(sample.radiance.x) && isfinite(sample.radiance.y) && isfinite(sample.radiance.z);
}
// A delta light as the light sample: the light from the table's CDF, a shadow ray to it (to infinity for a directional light) from the hit,
// offset on the hit's side only -- the light has no surface. pdf: the probability of this light, the delta lights' share times the record's P_k.
template<typename BSDF>
RT_DEV bool nee_connect_delta(const RtParams & p, const BSDF & bsdf, f3 hit_point, f3 normal, f3 geometric_normal, f3 throughput, float u, ShadowRay & shadow) {
	const RtDeltaLight light = p.delta_lights[nee_pick_delta(p, u)];
	f3 origin = ray_origin_epsilon_offset(hit_point, delta_light_toward(light, hit_point), geometric_normal);
	DeltaSample sample;
	if (!delta_light_sample(light, origin, sample)) return false;
	return nee_finish<false, true>(p, bsdf, origin, sample.to_light, sample.max_distance, dot(sample.to_light, normal), sample.radiance, p.delta_nee_share * light.direction_pdf.w, throughput, shadow);
}
// SKY 1: the light sample goes to the sky with probability p.sky_nee_share (DIM_NEE_LIGHT.x below it; its direction from the DIM_NEE_TRIANGLE
// pair), else to the emitters, with DIM_NEE_LIGHT.x rescaled to [0, 1) -- the same random dimensions either way.
// SKY 2: ... and to a delta light with probability p.delta_nee_share (DIM_NEE_LIGHT.x below p.nee_taken, rescaled to [0, 1) for the table's search).
// SKY 3: as 2 (taken in [0, 1]: with 0 every light sample goes to the emitters), the emitter picked by the light tree (nee_connect_tree).
template<int SKY, typename BSDF>
RT_DEV bool next_event_estimation(const RtParams & p, const LightTablesLDS * light_lds, int pixel_index, int bounce, int sample_index, const BSDF & bsdf, f3 hit_point, f3 normal, f3 geometric_normal, f3 throughput, ShadowRay & shadow) {
	f2 rand_light    = random_sample(p, bsdf.rng, DIM_NEE_LIGHT,    unsigned(bounce));
	f2 rand_triangle = random_sample(p, bsdf.rng, DIM_NEE_TRIANGLE, unsigned(bounce));
	if (!SKY) return nee_connect<false>(p, nee_pick_light(p, light_lds, rand_light, rand_triangle), bsdf, hit_point, normal, geometric_normal, throughput, 1.0f, shadow);
	if (SKY == 1) {
		const float share = p.sky_nee_share;   // (0, 1]: the _sky kernels run only while sampling is active
		if (rand_light.x < share) return nee_connect_sky(p, bsdf, hit_point, normal, geometric_normal, throughput, rand_triangle, shadow);
		rand_light.x = fminf((rand_light.x - share) / (1.0f - share), 0x1.fffffep-1f);   // (share < 1 here)
		return nee_connect<true>(p, nee_pick_light(p, light_lds, rand_light, rand_triangle), bsdf, hit_point, normal, geometric_normal, throughput, 1.0f - share, shadow);
	}
	const float share = p.sky_nee_share, taken = p.nee_taken;   // taken in (0, 1]: the _split kernels run only while the delta lights take a share
	if (rand_light.x < share) return nee_connect_sky(p, bsdf, hit_point, normal, geometric_normal, throughput, rand_triangle, shadow);
	if (rand_light.x < taken) return nee_connect_delta(p, bsdf, hit_point, normal, geometric_normal, throughput, fminf((rand_light.x - share) / p.delta_nee_share, 0x1.fffffep-1f), shadow);
	rand_light.x = fminf((rand_light.x - taken) / (1.0f - taken), 0x1.fffffep-1f);   // (taken < 1 here)
	if constexpr (SKY == 3) return nee_connect_tree(p, bsdf, hit_point, normal, geometric_normal, throughput, 1.0f - taken, rand_light.x, rand_light.y, rand_triangle, shadow);
	else return nee_connect<true>(p, nee_pick_light(p, light_lds, rand_light, rand_triangle), bsdf, hit_point, normal, geometric_normal, throughput, 1.0f - taken, shadow);
}

// The light sample of a fog scatter vertex (sort_rays<.., FOG>): next_event_estimation<2> with a phase "BSDF" -- eval gives value = pdf = HG(cos), no cosine
// factor -- and a geometric normal of zero, which makes every ray_origin_epsilon_offset on the vertex's side the identity: there is no surface. DIM_NEE_LIGHT
// and DIM_NEE_TRIANGLE of the bounce are free: no surface draws them at a bounce that ended in the air. The tables come from global memory.
struct PhaseHG {
	RandomPath rng; f3 omega; float g;   // omega: back along the arriving ray
	RT_DEV bool eval(const RtParams &, f3 to_light, float, f3 & bsdf, float & pdf) const {
		pdf = henyey_greenstein(dot(omega, to_light), g);
		bsdf = mk3(pdf);
		return pdf > 0.0f && isfinite(pdf);
	}
};
struct FogLightSample { f3 origin, direction; float max_distance; f3 illumination; };
RT_DEV bool fog_vertex_light_sample(const RtParams & p, int pixel_index, int bounce, int sample_index, f3 ray_direction, f3 vertex, f3 throughput, FogLightSample & out) {
	PhaseHG phase;
	phase.rng = random_path(p, unsigned(pixel_index), unsigned(sample_index)); phase.omega = -ray_direction; phase.g = p.fog_g;
	ShadowRay shadow;
	if (!next_event_estimation<2>(p, nullptr, pixel_index, bounce, sample_index, phase, vertex, mk3(0.0f), mk3(0.0f), throughput, shadow)) return false;
	out.origin = shadow.origin; out.direction = shadow.direction; out.max_distance = shadow.max_distance; out.illumination = shadow.illumination;
	return true;
}
