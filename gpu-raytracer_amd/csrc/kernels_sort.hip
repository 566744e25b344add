// kernels_sort.hip -- the per-bounce "sort" dispatch kernel: what a traced ray found (the sky, an emitter, a medium, the fog, a surface)
// and the material queue it continues in. 12 instances and their two launchers.
//
// Replaces kernel_sort of the reference (CUDA/Pathtracer.cu:199-463).
#include "rt_lights.h"   // fog_vertex_light_sample (the ..._fog instances); rt_surface.h with it
#include "rt_fog_grid.h"

// ---- kernel_sort -----------------------------------------------------------------------------------

// Returns true if the path terminates (Pathtracer.cu:199-218)
RT_DEV bool russian_roulette(const RtParams & p, int pixel_index, int bounce, int sample_index, f3 & throughput) {
	if (bounce == p.config.num_bounces - 1) return true;
	if (p.config.enable_russian_roulette && bounce > 0) {
		f3 t = throughput;
		if (p.config.enable_svgf) t *= mk3(aov_get(p, RT_AOV_ALBEDO, pixel_index));
		float survival_probability = saturate(fmaxf(fmaxf(t.x, t.y), t.z));
		float r = random_sample(p, DIM_RUSSIAN_ROULETTE, unsigned(pixel_index), unsigned(bounce), unsigned(sample_index)).x;
		if (r > survival_probability) return true;
		throughput /= survival_probability;
	}
	return false;
}

RT_DEV void add_radiance(const RtParams & p, int bounce, int pixel_index, f3 illumination, f3 bounce0_value) {
	if (bounce == 0) {
		aov_set(p, RT_AOV_ALBEDO,          pixel_index, mk4(1.0f));
		aov_set(p, RT_AOV_RADIANCE,        pixel_index, mk4(bounce0_value));
		aov_set(p, RT_AOV_RADIANCE_DIRECT, pixel_index, mk4(bounce0_value));
	} else if (bounce == 1) {
		aov_add(p, RT_AOV_RADIANCE,        pixel_index, mk4(illumination));
		aov_add(p, RT_AOV_RADIANCE_DIRECT, pixel_index, mk4(illumination));
	} else {
		aov_add(p, RT_AOV_RADIANCE,          pixel_index, mk4(illumination));
		aov_add(p, RT_AOV_RADIANCE_INDIRECT, pixel_index, mk4(illumination));
	}
}

// MERGED: the launch processes the trace queue of iteration p.stream_iteration, whose entries are at different
// bounces and belong to different samples (rt_stream_path_info); the launch arguments are ignored.
// SKY: how the light samples are split (rt_light_split). 1 (the ..._sky instances): sky importance sampling is active (RtParams::sky_nee_share > 0) --
// what a BSDF-sampled ray finds of the sky and of the emitters is weighed against the light samples' pdfs, which now include the sky's share.
// 2 (the ..._split instances): delta lights take a share (RtParams::delta_nee_share > 0), with or without the sky -- the pdfs include what both
// take (RtParams::nee_taken; a delta light itself is never found by a BSDF-sampled ray).
// 3 (the ..._tree instances): a light tree is in force (rt_light_tree_in_force) -- everything 2 does, also with nee_taken == 0, and an emitter that
// a BSDF-sampled ray hits is weighed with the tree's pmf of its triangle instead of the power tables'.
// FOG (the ..._fog instances, on the SKY = 2 flavour, which covers the other two: with nee_taken == 0 it is the plain estimator to the bit): a fog volume
// is in force (RtParams::fog_active). A segment outside a dielectric's medium is clipped against the box; inside, the path scatters or
// loses throughput, and a scatter vertex samples the lights -- its shadow ray joins the shadow queue from here (fog_vertex_light_sample, rt_lights.h, below
// next_event_estimation) -- and goes on in a Henyey-Greenstein direction. FOG = 2 (the ..._fog_grid instances): a density grid lies over the box
// (RtParams::fog_grid) -- the segment step is the voxel march of rt_fog_grid.h, everything around it the same statements.
template<bool MERGED, int SKY = 0, int FOG = 0>
RT_DEV void sort_rays(const RtParams & p, int launch_bounce, int launch_sample_index) {
	const int q = MERGED ? (p.stream_iteration & 1) : (launch_bounce & 1);
	const int ray_count = MERGED ? p.stream->trace_count[q] : p.sizes->trace[launch_bounce];
	const RtTraceBuffer & in  = p.trace[q];
	const RtTraceBuffer & out = p.trace[q ^ 1];
	__shared__ BlockAppendLDS<4, RT_SORT_BLOCK / RT_WAVE_SIZE> append_lds;
	__shared__ StreamStatsLDS stats_lds;
	int * const material_counters[4] = {
		MERGED ? &p.stream->material_count[0] : &p.sizes->diffuse[launch_bounce],    MERGED ? &p.stream->material_count[1] : &p.sizes->plastic[launch_bounce],
		MERGED ? &p.stream->material_count[2] : &p.sizes->dielectric[launch_bounce], MERGED ? &p.stream->material_count[3] : &p.sizes->conductor[launch_bounce] };
	int * const next_trace_counter = MERGED ? &p.stream->trace_count[q ^ 1] : &p.sizes->trace[launch_bounce + 1];
	// (`if constexpr`: the other instances are compiled from the statements they always had)
	FogVolume fog; bool fog_nee = false; int * shadow_counter = nullptr;
	[[maybe_unused]] FogGrid grid;
	if constexpr (FOG == 2) grid = fog_grid(p, fog_volume(p));
	if constexpr (FOG) {
		fog = fog_volume(p);
		fog_nee = p.config.enable_next_event_estimation && (p.lights_total_weight > 0.0f || p.nee_taken > 0.0f);   // uniform: a light sample is possible at a scatter vertex
		shadow_counter = MERGED ? &p.stream->shadow_count[q] : &p.sizes->shadow[launch_bounce];   // where the material kernels of this bounce / iteration append too
	}
	if (MERGED) stream_stats_clear(stats_lds);

	// every thread of the workgroup makes the same number of rounds (block_aggregated_append has barriers)
	for (int first = blockIdx.x * blockDim.x; first < ray_count; first += gridDim.x * blockDim.x) {
		const int index = first + int(threadIdx.x);
		f3 ray_direction = mk3(0.0f); uint4 packed_hit = make_uint4(0, 0, 0, 0);
		float ray_cone_angle = 0.0f, ray_cone_width = 0.0f;
		int pixel_index = 0, medium_id = RT_INVALID;
		f3 throughput = mk3(1.0f);
		int bounce = launch_bounce, sample_index = launch_sample_index, submission = 0;
		// FOG: what a scatter vertex hands to the two appends below the classification (slot 4: the path goes on from the vertex)
		[[maybe_unused]] bool fog_shadow_ray = false;
		[[maybe_unused]] FogLightSample fog_shadow;
		[[maybe_unused]] f3 fog_vertex = mk3(0.0f), fog_direction_out = mk3(0.0f);

		// classify one ray: the material queue it continues in, or -1 (missed, hit a light, scattered, terminated)
		auto classify = [&]() -> int {
		if (index >= ray_count) return -1;
		unsigned pixel_index_and_flags = in.pixel_index_and_flags[index];
		pixel_index = int(pixel_index_and_flags & ~RT_FLAGS_ALL);
		bool first_of_submission = true;
		if (MERGED) {
			RtPathInfo info = rt_stream_path_info(p, unsigned(pixel_index));
			bounce = info.bounce; sample_index = int(info.sample_index_for_rng); submission = info.submission; first_of_submission = info.first_of_submission;
		}
		ray_direction = load3(in.direction, index);
		packed_hit = in.hits[index];
		HitInfo hit = unpack_hit(packed_hit);

		// Merged wavefront: the bounce of an entry comes out of the slot table, i.e. behind two dependent loads; the entry's other fields
		// are fetched beside them, not after them (every queue array has a slot for every entry; what bounce 0 never wrote is not used).
		if (MERGED ? p.config.enable_mipmapping : (bounce > 0 && p.config.enable_mipmapping)) {
			float angle = in.cone_angle[index], width = in.cone_width[index];
			if (bounce > 0) { ray_cone_angle = angle; ray_cone_width = width; }
		}

		int x = pixel_index % p.screen_pitch;
		int y = pixel_index / p.screen_pitch;

		bool allow_nee     = pixel_index_and_flags & RT_FLAG_ALLOW_NEE;
		bool inside_medium = pixel_index_and_flags & RT_FLAG_INSIDE_MEDIUM;

		if (MERGED) { f3 carried = load3(in.throughput, index); throughput = bounce == 0 ? mk3(1.0f) : carried; }
		else throughput = bounce == 0 ? mk3(1.0f) : load3(in.throughput, index);

		if (inside_medium) {
			medium_id = in.medium[index];
			HomogeneousMedium medium = medium_as_homogeneous(p, medium_id);
			bool medium_can_scatter = (medium.sigma_s.x + medium.sigma_s.y + medium.sigma_s.z) > 0.0f;
			if (medium_can_scatter) {
				f2 rand_scatter = random_sample(p, DIM_BSDF_0, unsigned(pixel_index), unsigned(bounce), unsigned(sample_index));
				f2 rand_phase   = random_sample(p, DIM_BSDF_1, unsigned(pixel_index), unsigned(bounce), unsigned(sample_index));
				f3 sigma_t = medium.sigma_a + medium.sigma_s;

				float throughput_sum = throughput.x + throughput.y + throughput.z;
				f3 wavelength_pdf = throughput / throughput_sum;

				float sigma_t_used;
				if      (rand_scatter.x * throughput_sum < throughput.x)                sigma_t_used = sigma_t.x;
				else if (rand_scatter.x * throughput_sum < throughput.x + throughput.y) sigma_t_used = sigma_t.y;
				else                                                                   sigma_t_used = sigma_t.z;

				float scatter_distance = sample_exp(sigma_t_used, rand_scatter.y);
				f3 transmittance = beer_lambert(sigma_t, fminf(scatter_distance, hit.t));

				if (scatter_distance < hit.t) {
					f3 pdf = wavelength_pdf * sigma_t * transmittance;
					throughput *= medium.sigma_s * transmittance / (pdf.x + pdf.y + pdf.z);
					if (russian_roulette(p, pixel_index, bounce, sample_index, throughput)) return -1;

					f3 direction_out = sample_henyey_greenstein(-ray_direction, medium.g, rand_phase.x, rand_phase.y);
					f3 origin_out = load3(in.origin, index) + scatter_distance * ray_direction;

					int index_out = wave_aggregated_append(next_trace_counter);
					store3(out.origin,    index_out, origin_out);
					store3(out.direction, index_out, direction_out);
					out.medium[index_out] = medium_id;
					if (p.config.enable_mipmapping) {
						if (bounce == 0) { ray_cone_angle = p.camera.pixel_spread_angle; ray_cone_width = p.camera.pixel_spread_angle * scatter_distance; }
						out.cone_angle[index_out] = ray_cone_angle;
						out.cone_width[index_out] = ray_cone_width;
					}
					out.pixel_index_and_flags[index_out] = unsigned(pixel_index) | RT_FLAG_INSIDE_MEDIUM;
					store3(out.throughput, index_out, throughput);
					return -1;
				} else {
					f3 pdf = wavelength_pdf * transmittance;
					throughput *= transmittance / (pdf.x + pdf.y + pdf.z);
				}
			} else {
				throughput *= beer_lambert(medium.sigma_a, hit.t);
			}
		}

		if constexpr (FOG) if (!inside_medium) {   // (a dielectric's own medium displaces the fog)
			const f3 origin = load3(in.origin, index);
			float t0, t1;
			if (fog_clip(fog, origin, ray_direction, hit.triangle_id == RT_INVALID ? RT_INFINITY : hit.t, t0, t1)) {
				const RandomPath rng = random_path(p, unsigned(pixel_index), unsigned(sample_index));
				float scatter_distance;
				[[maybe_unused]] float grid_along, grid_density_length;
				bool scattered;
				if constexpr (FOG == 2) scattered = fog_grid_sample_distance(fog, grid, fog_random_pair(rng, unsigned(bounce)), origin, ray_direction, t0, t1, throughput, scatter_distance, grid_along, grid_density_length);
				else scattered = fog_sample_distance(fog, fog_random_pair(rng, unsigned(bounce)), t1 - t0, throughput, scatter_distance);
				if (scattered) {
					if (russian_roulette(p, pixel_index, bounce, sample_index, throughput)) return -1;
					float along = t0 + scatter_distance;
					if constexpr (FOG == 2) along = grid_along;
					const f3 vertex = origin + along * ray_direction;
					if (fog_nee) fog_shadow_ray = fog_vertex_light_sample(p, pixel_index, bounce, sample_index, ray_direction, vertex, throughput, fog_shadow);
					f2 rand_phase = random_sample(p, rng, DIM_BSDF_1, unsigned(bounce));
					fog_direction_out = sample_henyey_greenstein(-ray_direction, fog.g, rand_phase.x, rand_phase.y);   // value / pdf = 1: the throughput stays
					fog_vertex = vertex;
					if (p.config.enable_mipmapping) {
						if (bounce == 0) { ray_cone_angle = p.camera.pixel_spread_angle; ray_cone_width = ray_cone_angle * along; }
						else ray_cone_width += ray_cone_angle * along;
					}
					return 4;
				}
			}
		}

		if (hit.triangle_id == RT_INVALID) { // miss: sky
			f3 illumination = throughput * sample_sky(p, ray_direction);
			if (SKY && allow_nee && (SKY == 1 || p.sky_nee_share > 0.0f)) {   // the light samples reach the sky too: MIS against them, or (MIS off) leave the sky to them (delta lights alone: the sky whole, its tables unread)
				if (!p.config.enable_multiple_importance_sampling) return -1;
				illumination *= power_heuristic(in.last_pdf[index], p.sky_nee_share * sky_pdf(p, ray_direction));
			}
			add_radiance(p, bounce, pixel_index, illumination, illumination);
			return -1;
		}

		if (bounce == 0 && first_of_submission && p.pixel_query_pixel == (MERGED ? int(unsigned(pixel_index) % p.frame_pixels) : pixel_index)) { // Pathtracer.cu:345-348 (sample 0 of a batch: virtual == real index)
			p.pixel_query_out[0] = hit.mesh_id;
			p.pixel_query_out[1] = hit.triangle_id;
		}

		int material_id = p.mesh_material_ids[hit.mesh_id];
		int material_type = p.material_types[material_id];

		if (material_type == RT_MATERIAL_LIGHT) {
			f3 p0, e1, e2;
			triangle_get_positions(p, hit.triangle_id, p0, e1, e2);
			f3 light_point = barycentric(hit.u, hit.v, p0, e1, e2);
			f3 light_point_prev = light_point;
			f3 light_geometric_normal = cross(e1, e2);

			const float4 * world = p.mesh_transforms + size_t(hit.mesh_id) * 3;
			light_point = m_position(world, light_point);
			light_geometric_normal = normalize(m_direction(world, light_geometric_normal));

			if (bounce == 0 && p.config.enable_svgf) {
				light_point_prev = m_position(p.mesh_transforms_prev + size_t(hit.mesh_id) * 3, light_point_prev);
				svgf_set_gbuffers(p, x, y, hit, light_point, light_geometric_normal, light_point_prev);
			}

			f3 emission = mk3(p.materials[2 * material_id]);

			bool count_light = p.config.enable_next_event_estimation ? !allow_nee : true;
			if (SKY && (SKY == 1 ? p.sky_nee_share : p.nee_taken) >= 1.0f) count_light = true;   // every light sample goes to the sky or a delta light: emitters are found by BSDF sampling alone
			if (count_light) {
				if constexpr (FOG) add_radiance(p, bounce, pixel_index, throughput * emission, throughput * emission);   // (the camera may look through the box)
				else add_radiance(p, bounce, pixel_index, throughput * emission, emission);
				return -1;
			}
			if (p.config.enable_multiple_importance_sampling) {
				float cos_theta_light = abs_dot(ray_direction, light_geometric_normal);
				float distance_to_light_squared = hit.t * hit.t;
				float brdf_pdf = in.last_pdf[index];
				float light_power = luminance(emission.x, emission.y, emission.z);
				float light_pdf = light_power * distance_to_light_squared / (cos_theta_light * p.lights_total_weight);
				if constexpr (SKY == 3) {   // the tree's pmf of this triangle as seen from the ray's origin (what the light sample there weighed it with, one epsilon offset apart)
					float area = 0.0f;
					const int slot = light_tree_slot_of_hit(p.light_tree, p.light_mesh_triangle_span, hit.mesh_id, hit.triangle_id, area);
					const f3 origin = load3(in.origin, index);
					const float pmf = slot >= 0 ? light_tree_pmf(p.light_tree, origin.x, origin.y, origin.z, slot) : 0.0f;
					if (!(pmf > 0.0f)) {   // no light sample from there can reach this triangle (a probability rounded to 0, a triangle the tables do not name): this ray is its only estimator
						add_radiance(p, bounce, pixel_index, throughput * emission, emission);
						return -1;
					}
					light_pdf = pmf * distance_to_light_squared / (area * cos_theta_light);
				}
				if (SKY) light_pdf *= 1.0f - (SKY == 1 ? p.sky_nee_share : p.nee_taken);
				if (!pdf_is_valid(light_pdf)) return -1;
				float mis_weight = power_heuristic(brdf_pdf, light_pdf);
				f3 illumination = throughput * emission * mis_weight;
				aov_add(p, RT_AOV_RADIANCE, pixel_index, mk4(illumination));
				if (bounce == 1) aov_add(p, RT_AOV_RADIANCE_DIRECT,   pixel_index, mk4(illumination));
				else             aov_add(p, RT_AOV_RADIANCE_INDIRECT, pixel_index, mk4(illumination));
			}
			return -1;
		}

		if (russian_roulette(p, pixel_index, bounce, sample_index, throughput)) return -1;

		switch (material_type) {
			case RT_MATERIAL_DIFFUSE:    return 0;
			case RT_MATERIAL_PLASTIC:    return 1;
			case RT_MATERIAL_DIELECTRIC: return 2;
			case RT_MATERIAL_CONDUCTOR:  return 3;
		}
		return -1;
		};

		int slot = classify();
		if (MERGED) {
			stream_stats_add(stats_lds, index < ray_count, submission, RT_STAT_TRACE);
			#pragma unroll
			for (int m = 0; m < 4; m++) stream_stats_add(stats_lds, slot == m, submission, RT_STAT_DIFFUSE + m);
			if constexpr (FOG) stream_stats_add(stats_lds, fog_shadow_ray, submission, RT_STAT_SHADOW);
		}
		if constexpr (FOG) {
			// One returning atomic per workgroup and queue here too: with wave-level appends (the inside_medium branch's way) the benchmark scene in fog spent 6.2 ms
			// of a 12.4 ms step in this launch, at the L2's rate of returning atomics on one word (profiles/fog_volume.txt). A path continues in a material queue
			// or (slot 4) from its scatter vertex, never both: one append for the five; the vertices' light samples take a second.
			// Every thread of the workgroup gets here in every round: the bounce limit, Russian roulette and every other end of a path are `return`s INSIDE classify
			// (slot -1), never a `continue` or `return` of this loop, whose bound is the same for the whole workgroup -- so no lane can skip the barriers of an append.
			__shared__ BlockAppendLDS<5, RT_SORT_BLOCK / RT_WAVE_SIZE> fog_append_lds;
			__shared__ BlockAppendLDS<1, RT_SORT_BLOCK / RT_WAVE_SIZE> fog_shadow_lds;
			int * const fog_counters[5] = { material_counters[0], material_counters[1], material_counters[2], material_counters[3], next_trace_counter };
			int * const fog_shadow_counters[1] = { shadow_counter };
			const int index_out = block_aggregated_append(slot, fog_counters, fog_append_lds);
			const int shadow_ray_index = block_aggregated_append(fog_shadow_ray ? 0 : -1, fog_shadow_counters, fog_shadow_lds);
			if (fog_shadow_ray) {
				store3(p.shadow.origin,    shadow_ray_index, fog_shadow.origin);
				store3(p.shadow.direction, shadow_ray_index, fog_shadow.direction);
				p.shadow.max_distance[shadow_ray_index] = fog_shadow.max_distance;
				unsigned pixel_word = unsigned(pixel_index) | (MERGED && bounce == 0 ? RT_SHADOW_FLAG_BOUNCE_0 : 0u);   // (as shade_material: store_shadow_ray)
				p.shadow.illumination_and_pixel_index[shadow_ray_index] = make_float4(fog_shadow.illumination.x, fog_shadow.illumination.y, fog_shadow.illumination.z, __uint_as_float(pixel_word));
			}
			if (slot == 4) {
				store3(out.origin,    index_out, fog_vertex);
				store3(out.direction, index_out, fog_direction_out);
				if (p.config.enable_mipmapping) { out.cone_angle[index_out] = ray_cone_angle; out.cone_width[index_out] = ray_cone_width; }
				// what the ray finds of the emitters and the sky is weighed against the vertex's light sample by the next sort launch, as after a surface
				out.pixel_index_and_flags[index_out] = unsigned(pixel_index) | (fog_nee ? RT_FLAG_ALLOW_NEE : 0u);
				store3(out.throughput, index_out, throughput);
				out.last_pdf[index_out] = henyey_greenstein(dot(-ray_direction, fog_direction_out), fog.g);
			} else if (slot >= 0) material_queue_store<true>(p, slot, index_out, bounce, ray_direction, medium_id, ray_cone_angle, ray_cone_width, packed_hit, pixel_index, throughput);
			continue;
		}
		int index_out = block_aggregated_append(slot, material_counters, append_lds);
		if (slot >= 0) material_queue_store(p, slot, index_out, bounce, ray_direction, medium_id, ray_cone_angle, ray_cone_width, packed_hit, pixel_index, throughput);
	}
	if (MERGED) stream_stats_flush(p, stats_lds);
}

__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort(RtParams p, int bounce, int sample_index) { sort_rays<false>(p, bounce, sample_index); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort_stream(RtParams p) { sort_rays<true>(p, 0, 0); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort_sky(RtParams p, int bounce, int sample_index) { sort_rays<false, 1>(p, bounce, sample_index); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort_stream_sky(RtParams p) { sort_rays<true, 1>(p, 0, 0); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort_split(RtParams p, int bounce, int sample_index) { sort_rays<false, 2>(p, bounce, sample_index); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort_stream_split(RtParams p) { sort_rays<true, 2>(p, 0, 0); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort_tree(RtParams p, int bounce, int sample_index) { sort_rays<false, 3>(p, bounce, sample_index); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_WAVES) kernel_sort_stream_tree(RtParams p) { sort_rays<true, 3>(p, 0, 0); }
// The ..._fog instances, launched only while a fog volume is in force. A scatter vertex carries a whole light sample (two table searches, a delta light or a
// sky direction, the phase function) on top of the sort: at the 64 registers of RT_SORT_WAVES that spills, so these ask for RT_SORT_FOG_WAVES = 4 waves per
// SIMD (128 registers; one 1024-thread workgroup per CU, whose 16 waves are those 4 per SIMD). LDS: the statistics block of the other instances and two append blocks of their own.
#ifndef RT_SORT_FOG_WAVES
#define RT_SORT_FOG_WAVES 4
#endif
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_FOG_WAVES) kernel_sort_fog(RtParams p, int bounce, int sample_index) { sort_rays<false, 2, 1>(p, bounce, sample_index); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_FOG_WAVES) kernel_sort_stream_fog(RtParams p) { sort_rays<true, 2, 1>(p, 0, 0); }
// The ..._fog_grid instances, launched only while a density grid is in force (RtParams::fog_grid): the same kernels with the voxel march as their segment step.
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_FOG_WAVES) kernel_sort_fog_grid(RtParams p, int bounce, int sample_index) { sort_rays<false, 2, 2>(p, bounce, sample_index); }
__global__ void __launch_bounds__(RT_SORT_BLOCK, RT_SORT_FOG_WAVES) kernel_sort_stream_fog_grid(RtParams p) { sort_rays<true, 2, 2>(p, 0, 0); }

// ---- launchers ---------------------------------------------------------------------------------------------------

// (the ..._sky instance while sky importance sampling is active, the ..._split one while delta lights take a share, the ..._tree one while a light tree is in force, as for the material kernels)
void rt_launch_sort(const RtParams & p, int bounce, int sample_index, hipStream_t stream) {
	const int split = rt_light_split(p);
	hipLaunchKernelGGL(p.fog_active ? (p.fog_grid ? kernel_sort_fog_grid : kernel_sort_fog) : split == 3 ? kernel_sort_tree : split == 2 ? kernel_sort_split : split == 1 ? kernel_sort_sky : kernel_sort, dim3(2048 * RT_SHADE_BLOCK / RT_SORT_BLOCK), dim3(RT_SORT_BLOCK), 0, stream, p, bounce, sample_index);
}
void rt_launch_sort_stream(const RtParams & p, hipStream_t stream) {
	const int split = rt_light_split(p);
	hipLaunchKernelGGL(p.fog_active ? (p.fog_grid ? kernel_sort_stream_fog_grid : kernel_sort_stream_fog) : split == 3 ? kernel_sort_stream_tree : split == 2 ? kernel_sort_stream_split : split == 1 ? kernel_sort_stream_sky : kernel_sort_stream, dim3(RT_STREAM_SORT_GRID * RT_SHADE_BLOCK / RT_SORT_BLOCK), dim3(RT_SORT_BLOCK), 0, stream, p);
}
