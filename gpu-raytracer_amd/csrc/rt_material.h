// rt_material.h -- the material launch: shade_material<BSDF> with next-event estimation, the one list of its 96 kernel instances, and what a row's unit
// (kernels_material_<material><_texels>.hip) compiles of that list. The selector and the two launchers are in kernels_material.hip.
//
// Replaces kernel_material_{diffuse,plastic,dielectric,conductor} of the reference (CUDA/Pathtracer.cu:465-773, CUDA/BSDF.h).
#pragma once
#include "rt_bsdf.h"
#include "rt_lights.h"

// ---- shade_material<BSDF> (Pathtracer.cu:557-757) -------------------------------------------------------------

RT_DEV float triangle_get_lod(float double_area_world_inv, f2 te1, f2 te2) {
	float area_texel = fabsf(te1.x * te2.y - te2.x * te1.y);
	return sqrtf(area_texel * double_area_world_inv);
}
RT_DEV float triangle_get_curvature(f3 pe1, f3 pe2, f3 ne1, f3 ne2) {
	f3 ne0 = ne1 - ne2;
	f3 pe0 = pe1 - pe2;
	float k_01 = dot(ne1, pe1) / dot(pe1, pe1);
	float k_02 = dot(ne2, pe2) / dot(pe2, pe2);
	float k_12 = dot(ne0, pe0) / dot(pe0, pe0);
	return (k_01 + k_02 + k_12) * (1.0f / 3.0f);
}
RT_DEV void ray_cone_get_ellipse_axes(f3 ray_direction, f3 geometric_normal, float cone_width, f3 & axis_1, f3 & axis_2) {
	f3 h_1 = ray_direction - dot(geometric_normal, ray_direction) * geometric_normal;
	f3 h_2 = cross(geometric_normal, h_1);
	axis_1 = cone_width / fmaxf(0.0001f, length(h_1 - dot(ray_direction, h_1) * ray_direction)) * h_1;
	axis_2 = cone_width / fmaxf(0.0001f, length(h_2 - dot(ray_direction, h_2) * ray_direction)) * h_2;
}
RT_DEV f2 ray_cone_ellipse_axis_to_gradient(const TriangleFull & tri, float double_area_inv, f3 geometric_normal, f3 hit_point, f2 hit_tex_coord, f3 ellipse_axis) {
	f3 e_p = hit_point + ellipse_axis - tri.position_0;
	float u = dot(geometric_normal, cross(e_p, tri.position_edge_2)) * double_area_inv;
	float v = dot(geometric_normal, cross(tri.position_edge_1, e_p)) * double_area_inv;
	return barycentric(u, v, tri.tex_coord_0, tri.tex_coord_edge_1, tri.tex_coord_edge_2) - hit_tex_coord;
}
RT_DEV float ray_cone_get_lod(f3 ray_direction, f3 geometric_normal, float cone_width) { return fabsf(cone_width / dot(ray_direction, geometric_normal)); }

// MERGED: the queue holds the surface hits of every submission in flight (see sort_rays); bounce and sample come
// from the slot table, the launch arguments are ignored.
// SKY: how the light samples are split (rt_light_split): 1 between the sky and the emitters, 2 with the delta lights as well, see next_event_estimation.
// NMAP: some material of this slot has a normal map (RtParams::normal_map_slots): a hit whose material has one shades with the mapped
// normal (normal_map_perturb); a hit whose material has none runs the arithmetic of the plain instance.
template<typename BSDF, int SLOT, bool MERGED, int SKY = 0, bool NMAP = false>
RT_DEV void shade_material(const RtParams & p, int launch_bounce, int launch_sample_index) {
	const RtMaterialBuffer & q = p.material[SLOT];
	const int iq = MERGED ? (p.stream_iteration & 1) : (launch_bounce & 1);
	const RtTraceBuffer & out = p.trace[iq ^ 1];
	const int buffer_size = MERGED ? p.stream->material_count[SLOT]
	                               : (SLOT == 0 ? p.sizes->diffuse[launch_bounce] : SLOT == 1 ? p.sizes->plastic[launch_bounce] : SLOT == 2 ? p.sizes->dielectric[launch_bounce] : p.sizes->conductor[launch_bounce]);

	__shared__ BlockBucketLDS<RT_SHADE_BLOCK / RT_WAVE_SIZE> append_lds;
#if RT_SHADE_ONE_APPEND
	__shared__ BlockBucket2LDS<RT_SHADE_BLOCK / RT_WAVE_SIZE> append2_lds;
#endif
	__shared__ StreamStatsLDS stats_lds;
	int * const shadow_counter = MERGED ? &p.stream->shadow_count[iq]    : &p.sizes->shadow[launch_bounce];
	int * const trace_counter  = MERGED ? &p.stream->trace_count[iq ^ 1] : &p.sizes->trace[launch_bounce + 1];
	const bool nee_enabled = SKY || (p.config.enable_next_event_estimation && p.lights_total_weight > 0.0f); // uniform
#if RT_LIGHT_TABLES_LDS
	__shared__ LightTablesLDS light_lds;
	if (SKY != 3 && nee_enabled && (!SKY || p.lights_total_weight > 0.0f) && blockIdx.x * blockDim.x < unsigned(buffer_size)) light_tables_to_lds(p, light_lds);   // (the ..._tree instances search no table)
	const LightTablesLDS * const light_tables = &light_lds;
#else
	const LightTablesLDS * const light_tables = nullptr;
#endif
	if (MERGED) stream_stats_clear(stats_lds); else __syncthreads();   // (either way a barrier: the tables are in place)

	// every thread of the workgroup makes the same number of rounds (block_aggregated_append has barriers)
	for (int first = blockIdx.x * blockDim.x; first < buffer_size; first += gridDim.x * blockDim.x) {
		const int index = first + int(threadIdx.x);
		// what survives from the surface set-up to the two queue appends
		BSDF bsdf;
		int pixel_index = 0, medium_id = RT_INVALID;
		f3 throughput = mk3(1.0f), hit_point = mk3(0.0f), geometric_normal = mk3(0.0f);
		float cone_angle = 0.0f, cone_width = 0.0f;
		ShadowRay shadow; bool has_shadow_ray = false;
		int bounce = launch_bounce, sample_index = launch_sample_index, submission = 0;

		auto set_up_surface = [&]() -> bool { // false: the path ends here
		if (index >= buffer_size) return false;
		unsigned pixel_index_and_flags = q.pixel_index_and_flags[index];
		pixel_index = int(pixel_index_and_flags & ~RT_FLAGS_ALL);
		if (MERGED) {
			RtPathInfo info = rt_stream_path_info(p, unsigned(pixel_index));
			bounce = info.bounce; sample_index = int(info.sample_index_for_rng); submission = info.submission;
		}
		f3 ray_direction = load3(q.direction, index);
		HitInfo hit = unpack_hit(q.hits[index]);

		bool inside_medium = pixel_index_and_flags & RT_FLAG_INSIDE_MEDIUM;
		medium_id = inside_medium ? q.medium[index] : RT_INVALID;

		// (fog_active: the ..._fog sort instance has stored the throughput of bounce 0 too -- the first segment may have crossed the fog)
		if (MERGED) { f3 carried = load3(q.throughput, index); throughput = bounce == 0 && !p.fog_active ? mk3(1.0f) : carried; }   // (beside the slot-table lookup, see sort_rays)
		else throughput = bounce == 0 && !p.fog_active ? mk3(1.0f) : load3(q.throughput, index);

		TriangleFull tri = triangle_get_full(p, hit.triangle_id);
		hit_point = barycentric(hit.u, hit.v, tri.position_0, tri.position_edge_1, tri.position_edge_2);
		f3 normal    = barycentric(hit.u, hit.v, tri.normal_0,   tri.normal_edge_1,   tri.normal_edge_2);
		f2 tex_coord = barycentric(hit.u, hit.v, tri.tex_coord_0, tri.tex_coord_edge_1, tri.tex_coord_edge_2);
		f3 hit_point_local = hit_point;

		const float4 * world = p.mesh_transforms + size_t(hit.mesh_id) * 3;
		hit_point = m_position(world, hit_point);
		normal = normalize(m_direction(world, normal));

		float4 world_row_0 = world[0];
		float mesh_scale_inv = 1.0f / length(mk3(world_row_0.x, world_row_0.y, world_row_0.z));

		float curvature = 0.0f;
		if (p.config.enable_mipmapping) {
			float carried_angle = 0.0f, carried_width = 0.0f;
			if (MERGED || bounce > 0) { carried_angle = q.cone_angle[index]; carried_width = q.cone_width[index]; }
			if (bounce == 0) { cone_angle = p.camera.pixel_spread_angle; cone_width = cone_angle * hit.t; }
			else             { cone_angle = carried_angle; cone_width = carried_width + cone_angle * hit.t; }
			curvature = triangle_get_curvature(tri.position_edge_1, tri.position_edge_2, tri.normal_edge_1, tri.normal_edge_2) * mesh_scale_inv;
		}

		// the normal map of the hit's material, and its tangent from the object-space triangle (before the edges go to world space)
		int normal_map_id = RT_INVALID; f3 dpdu = mk3(0.0f); float uv_det = 0.0f;
		if (NMAP) {
			normal_map_id = p.material_normal_maps[p.mesh_material_ids[hit.mesh_id]];
			if (normal_map_id != RT_INVALID) dpdu = m_direction(world, normal_map_dpdu(tri.position_edge_1, tri.position_edge_2, tri.tex_coord_edge_1, tri.tex_coord_edge_2, uv_det));
		}

		tri.position_edge_1 = m_direction(world, tri.position_edge_1);
		tri.position_edge_2 = m_direction(world, tri.position_edge_2);

		geometric_normal = cross(tri.position_edge_1, tri.position_edge_2);
		float triangle_double_area_inv = 1.0f / length(geometric_normal);
		geometric_normal *= triangle_double_area_inv;

		bool entering_material = dot(ray_direction, geometric_normal) < 0.0f;
		if (!entering_material) { normal = -normal; curvature = -curvature; }

		// The texture footprint of the hit (ray cones): gradients at bounce 0, a level of detail after that. Computed once, for the
		// albedo and the normal map alike.
		TextureLOD lod = { mk2(0.0f, 0.0f), mk2(0.0f, 0.0f), 0.0f };
		bool have_footprint = false;
		auto footprint = [&]() {
			if (bounce == 0) {
				f3 axis_1, axis_2;
				ray_cone_get_ellipse_axes(ray_direction, geometric_normal, cone_width, axis_1, axis_2);
				lod.gradient_1 = ray_cone_ellipse_axis_to_gradient(tri, triangle_double_area_inv, geometric_normal, hit_point, tex_coord, axis_1);
				lod.gradient_2 = ray_cone_ellipse_axis_to_gradient(tri, triangle_double_area_inv, geometric_normal, hit_point, tex_coord, axis_2);
			} else {
				float lod_triangle = triangle_get_lod(triangle_double_area_inv, tri.tex_coord_edge_1, tri.tex_coord_edge_2);
				float lod_ray_cone = ray_cone_get_lod(ray_direction, geometric_normal, cone_width);
				lod.lod = log2f(lod_triangle * lod_ray_cone);
			}
		};

		// What the BSDF frame, next-event estimation, the NORMAL AOV and the SVGF g-buffer see; `normal` stays the interpolated
		// normal, which the ray cone's curvature term keeps.
		f3 shading_normal = normal;
		if (NMAP && normal_map_id != RT_INVALID) {
			if (p.config.enable_mipmapping) { footprint(); have_footprint = true; }
			const int filter = !p.config.enable_mipmapping ? 0 : bounce == 0 ? 2 : 1;
			normal_map_perturb<BSDF::MAP_COMPRESSED>(p.textures[normal_map_id], filter, tex_coord, lod.lod, lod.gradient_1, lod.gradient_2, dpdu, uv_det,
			                                         entering_material ? normal : -normal, geometric_normal, entering_material, ray_direction, shading_normal);
		}

		f3 tangent, bitangent;
		orthonormal_basis(shading_normal, tangent, bitangent);
		f3 omega_i = world_to_local(-ray_direction, tangent, bitangent, shading_normal);
		if (omega_i.z <= 0.0f) return false;

		int material_id = p.mesh_material_ids[hit.mesh_id];

		bsdf.pixel_index = pixel_index; bsdf.bounce = bounce; bsdf.sample_index = sample_index; bsdf.rng = random_path(p, unsigned(pixel_index), unsigned(sample_index));
		bsdf.tangent = tangent; bsdf.bitangent = bitangent; bsdf.normal = shading_normal; bsdf.omega_i = omega_i;
		bsdf.init(p, entering_material, material_id);

		if (BSDF::HAS_ALBEDO) {
			if (p.config.enable_mipmapping && bsdf.has_texture() && !have_footprint) footprint();
			bsdf.calc_albedo(p, throughput, tex_coord, lod);
		} else if (bounce == 0) {
			aov_set(p, RT_AOV_ALBEDO, pixel_index, mk4(1.0f));
		}

		if (bounce == 0) {
			aov_set(p, RT_AOV_NORMAL,   pixel_index, mk4(shading_normal));
			aov_set(p, RT_AOV_POSITION, pixel_index, mk4(hit_point));
		}

		if (p.config.enable_mipmapping) cone_angle -= 2.0f * curvature * fabsf(cone_width) / dot(normal, ray_direction);

		if (bounce == 0 && p.config.enable_svgf) {
			f3 hit_point_prev = m_position(p.mesh_transforms_prev + size_t(hit.mesh_id) * 3, hit_point_local);
			int x = pixel_index % p.screen_pitch, y = pixel_index / p.screen_pitch;
			svgf_set_gbuffers(p, x, y, hit, hit_point, shading_normal, hit_point_prev);
		}

		if (nee_enabled && bsdf.allow_nee()) {
			has_shadow_ray = next_event_estimation<SKY>(p, light_tables, pixel_index, bounce, sample_index, bsdf, hit_point, shading_normal, geometric_normal, throughput, shadow);
		}
		return true;
		};

		bool alive = set_up_surface();

		auto store_shadow_ray = [&](int shadow_ray_index) {
			store3(p.shadow.origin,    shadow_ray_index, shadow.origin);
			store3(p.shadow.direction, shadow_ray_index, shadow.direction);
			p.shadow.max_distance[shadow_ray_index] = shadow.max_distance;
			// merged wavefront: the trace launch that consumes the ray cannot know its bounce from a launch argument
			unsigned pixel_word = unsigned(pixel_index) | (MERGED && bounce == 0 ? RT_SHADOW_FLAG_BOUNCE_0 : 0u);
			p.shadow.illumination_and_pixel_index[shadow_ray_index] = make_float4(shadow.illumination.x, shadow.illumination.y, shadow.illumination.z, __uint_as_float(pixel_word));
		};
		if (nee_enabled && MERGED) stream_stats_add(stats_lds, has_shadow_ray, submission, RT_STAT_SHADOW);
#if !RT_SHADE_ONE_APPEND
		if (nee_enabled) {
			// (both ray queues: the workgroup's rays ordered by direction octant, see block_bucketed_append)
			int shadow_ray_index = block_bucketed_append(has_shadow_ray, RT_RAY_BUCKET(shadow.direction), shadow_counter, append_lds);
			if (has_shadow_ray) store_shadow_ray(shadow_ray_index);
		}
#endif

		f3 direction_out = mk3(0.0f); float pdf = 0.0f;
		bool continues = alive && bsdf.sample(p, throughput, medium_id, direction_out, pdf);

		int index_out;
#if RT_SHADE_ONE_APPEND
		// the round's two appends (shadow ray, continuation ray) in one: two workgroup barriers and one atomic latency instead of four and two
		if (nee_enabled) {
			int shadow_ray_index;
			block_bucketed_append2(has_shadow_ray, RT_RAY_BUCKET(shadow.direction), shadow_counter, continues, RT_RAY_BUCKET(direction_out), trace_counter, append2_lds, shadow_ray_index, index_out);
			if (has_shadow_ray) store_shadow_ray(shadow_ray_index);
		} else
#endif
		index_out = block_bucketed_append(continues, RT_RAY_BUCKET(direction_out), trace_counter, append_lds);
		if (!continues) continue;

		f3 origin_out = ray_origin_epsilon_offset(hit_point, direction_out, geometric_normal);
		store3(out.origin,    index_out, origin_out);
		store3(out.direction, index_out, direction_out);
		if (medium_id != RT_INVALID) out.medium[index_out] = medium_id;
		if (p.config.enable_mipmapping) { out.cone_angle[index_out] = cone_angle; out.cone_width[index_out] = cone_width; }

		bool allow_nee = bsdf.allow_nee();
		unsigned flags = 0;
		if (allow_nee)               flags |= RT_FLAG_ALLOW_NEE;
		if (medium_id != RT_INVALID) flags |= RT_FLAG_INSIDE_MEDIUM;
		out.pixel_index_and_flags[index_out] = unsigned(pixel_index) | flags;
		store3(out.throughput, index_out, throughput);
		if (allow_nee) out.last_pdf[index_out] = pdf;
	}
	if (MERGED) stream_stats_flush(p, stats_lds);
}

// ---- the material kernels: one list, expanded for the eight (SKY, NMAP) combinations ----------------------------------
// A row: X(material, _texels or nothing, BSDF type, slot, waves per SIMD of the merged instance, ...). Each row yields, per combination,
// the per-bounce kernel_material_<material><_texels><suffix> and the merged kernel_material_<material>_stream<_texels><suffix>.
//   ..._texels: no texture on the device holds compressed blocks (RtParams::textures_compressed == 0)
//   ..._sky:    sky importance sampling is active (RtParams::sky_nee_share > 0) and no delta light takes a share, launched only then
//   ..._split:  delta lights take a share of the light samples (RtParams::delta_nee_share > 0), with or without the sky, launched only then
//   ..._tree:   a light tree is in force (rt_light_tree_in_force), with or without the sky and delta lights, launched only then
//   ..._nmap:   some material of the slot has a normal map (RtParams::normal_map_slots), launched only then
// The rows' order is material_kernels_for's index: the four slots, then the _texels forms of slots 0 and 1.
#ifndef RT_SHADE_WAVES_DIFFUSE
#define RT_SHADE_WAVES_DIFFUSE RT_SHADE_WAVES
#endif
#define RT_MATERIAL_KERNEL_LIST(X, ...) \
	X(diffuse,    ,        BSDFDiffuse,         0, RT_SHADE_WAVES,         __VA_ARGS__) \
	X(plastic,    ,        BSDFPlastic,         1, RT_SHADE_WAVES,         __VA_ARGS__) \
	X(dielectric, ,        BSDFDielectric,      2, RT_SHADE_WAVES,         __VA_ARGS__) \
	X(conductor,  ,        BSDFConductor,       3, RT_SHADE_WAVES,         __VA_ARGS__) \
	X(diffuse,    _texels, BSDFDiffuseT<false>, 0, RT_SHADE_WAVES_DIFFUSE, __VA_ARGS__) \
	X(plastic,    _texels, BSDFPlasticT<false>, 1, RT_SHADE_WAVES,         __VA_ARGS__)
#define RT_MATERIAL_KERNEL_VARIANTS(X) RT_MATERIAL_KERNEL_LIST(X, , 0, false) RT_MATERIAL_KERNEL_LIST(X, _sky, 1, false) RT_MATERIAL_KERNEL_LIST(X, _split, 2, false) RT_MATERIAL_KERNEL_LIST(X, _tree, 3, false) \
	RT_MATERIAL_KERNEL_LIST(X, _nmap, 0, true) RT_MATERIAL_KERNEL_LIST(X, _sky_nmap, 1, true) RT_MATERIAL_KERNEL_LIST(X, _split_nmap, 2, true) RT_MATERIAL_KERNEL_LIST(X, _tree_nmap, 3, true)

// ---- one unit per row: the material kernels are where the compile time goes ---------------------------------------------------
// RT_MATERIAL_ROW_<material><_texels>(...) keeps or drops what that row expands to. kernels_material_<material><_texels>.hip defines its own row's as
// `__VA_ARGS__` before it includes this header; the other five are nothing, so the unit compiles, from the one list, the 16 instances of its row alone.
#ifndef RT_MATERIAL_ROW_diffuse
#define RT_MATERIAL_ROW_diffuse(...)
#endif
#ifndef RT_MATERIAL_ROW_plastic
#define RT_MATERIAL_ROW_plastic(...)
#endif
#ifndef RT_MATERIAL_ROW_dielectric
#define RT_MATERIAL_ROW_dielectric(...)
#endif
#ifndef RT_MATERIAL_ROW_conductor
#define RT_MATERIAL_ROW_conductor(...)
#endif
#ifndef RT_MATERIAL_ROW_diffuse_texels
#define RT_MATERIAL_ROW_diffuse_texels(...)
#endif
#ifndef RT_MATERIAL_ROW_plastic_texels
#define RT_MATERIAL_ROW_plastic_texels(...)
#endif
#define RT_DEFINE_MATERIAL_KERNELS(MATERIAL, TEXELS, BSDF, SLOT, STREAM_WAVES, SUFFIX, SKY, NMAP) RT_MATERIAL_ROW_##MATERIAL##TEXELS( \
__global__ void __launch_bounds__(RT_SHADE_BLOCK, RT_SHADE_WAVES) kernel_material_##MATERIAL##TEXELS##SUFFIX(RtParams p, int bounce, int sample_index) { shade_material<BSDF, SLOT, false, SKY, NMAP>(p, bounce, sample_index); } \
__global__ void __launch_bounds__(RT_SHADE_BLOCK, STREAM_WAVES) kernel_material_##MATERIAL##_stream##TEXELS##SUFFIX(RtParams p) { shade_material<BSDF, SLOT, true, SKY, NMAP>(p, 0, 0); })
// The entry points of a row, from the same list: [NMAP * 4 + SKY]
struct MaterialKernels { void (*bounce)(RtParams, int, int); void (*merged)(RtParams); };
#define RT_MATERIAL_KERNEL_ENTRY(MATERIAL, TEXELS, BSDF, SLOT, STREAM_WAVES, SUFFIX, SKY, NMAP) RT_MATERIAL_ROW_##MATERIAL##TEXELS({ kernel_material_##MATERIAL##TEXELS##SUFFIX, kernel_material_##MATERIAL##_stream##TEXELS##SUFFIX },)
// What a row's unit hands to the host (no device symbol crosses a unit): its eight pairs of entry points, in the order of RT_MATERIAL_KERNEL_VARIANTS
#define RT_DECLARE_MATERIAL_ROW(MATERIAL, TEXELS, ...) const MaterialKernels * rt_material_kernels_##MATERIAL##TEXELS();
RT_MATERIAL_KERNEL_LIST(RT_DECLARE_MATERIAL_ROW, )
#undef RT_DECLARE_MATERIAL_ROW
// The whole of a row's unit: its kernels, the table of their entry points, and the function that returns it
#define RT_MATERIAL_UNIT(ROW) \
RT_MATERIAL_KERNEL_VARIANTS(RT_DEFINE_MATERIAL_KERNELS) \
const MaterialKernels * rt_material_kernels_##ROW() { \
	static const MaterialKernels kernels[8] = { RT_MATERIAL_KERNEL_VARIANTS(RT_MATERIAL_KERNEL_ENTRY) }; \
	return kernels; \
}
