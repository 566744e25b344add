#include "Pathtracer.h"
#include "Exporters.h"
#include <algorithm>
#include <cmath>
#include <stdexcept>

#include <cmath>
#include <cstring>
#include <map>

void Pathtracer::gpu_init(int width, int height) {
	Integrator::gpu_init(width, height);
	lights_total_weight = 0.0f;
}

void Pathtracer::gpu_free() {
	Integrator::gpu_free();
}

// reference: Pathtracer::resize_init (Pathtracer.cpp:255-301)
void Pathtracer::resize_init(int width, int height) {
	screen_width  = width;
	screen_height = height;
	screen_pitch  = Math::round_up(width, 32);
	pixel_count   = width * height;

	if (ctx) check(rt_resize(ctx, width, height));
	aov_enable(AOVType::RADIANCE);

	scene.camera.resize(width, height);
	invalidated_camera = true;
	sample_index = 0;

	if (gpu_config.enable_svgf) { // SVGF needs these inputs (Pathtracer.cpp:331-334)
		aov_enable(AOVType::RADIANCE_DIRECT);
		aov_enable(AOVType::RADIANCE_INDIRECT);
		aov_enable(AOVType::ALBEDO);
	}
}

void Pathtracer::resize_free() { }

// Per light-emitting MeshData: triangle areas -> per-mesh CDF over triangles; per Mesh:
// weight = luminance(emission) * total area (reference: Pathtracer.cpp:384-500).
void Pathtracer::calc_light_power() {
	std::map<int, std::vector<Mesh *>> light_users; // mesh_data handle -> meshes, ascending handle order
	for (Mesh & mesh : scene.meshes) {
		const Material & material = scene.asset_manager.get_material(mesh.material_handle);
		if (material.is_light()) light_users[mesh.mesh_data_handle.handle].push_back(&mesh);
		else mesh.light.weight = 0.0f;
	}

	light_triangle_indices.clear();
	light_triangle_cumulative_probability.clear();
	std::vector<double> triangle_area;

	for (auto & [mesh_data_handle, meshes] : light_users) {
		const MeshData & mesh_data = scene.asset_manager.mesh_datas[mesh_data_handle];

		size_t first = light_triangle_indices.size();
		size_t count = mesh_data.triangles.size();
		double total_area = 0.0;
		for (size_t t = 0; t < count; t++) {
			const Triangle & tri = mesh_data.triangles[t];
			float area = 0.5f * Vector3::length(Vector3::cross(tri.position_1 - tri.position_0, tri.position_2 - tri.position_0));
			light_triangle_indices.push_back(reverse_indices[mesh_data_triangle_offsets[mesh_data_handle] + int(t)]);
			triangle_area.push_back(area);
			total_area += area;
		}

		for (Mesh * mesh : meshes) {
			const Material & material = scene.asset_manager.get_material(mesh->material_handle);
			mesh->light.weight               = Math::luminance(material.emission) * float(total_area);
			mesh->light.first_triangle_index = int(first);
			mesh->light.triangle_count       = int(count);
		}

		light_triangle_cumulative_probability.resize(first + count);
		double cumulative = 0.0;
		for (size_t i = first; i < first + count; i++) {
			cumulative += triangle_area[i] / total_area;
			light_triangle_cumulative_probability[i] = float(cumulative);
		}
		for (size_t i = first; i < first + count; i++) light_triangle_cumulative_probability[i] /= float(cumulative);
	}

	if (!light_triangle_indices.empty()) invalidated_scene = true; // mesh tables are filled once the TLAS exists
}

// Second CDF level, over light meshes in TLAS order, weight scaled by scale^2
// (reference: Pathtracer.cpp:503-534).
void Pathtracer::calc_light_mesh_weights() {
	light_mesh_cumulative_probability.clear();
	light_mesh_triangle_span.clear();
	light_mesh_transform_indices.clear();

	// Order of the light meshes in the CDF: TLAS order, as in the reference -- unless the TLAS is built on the device, whose
	// order the host does not know; then scene order, with scene indices as transform indices (the device maps them)
	// Flattened static geometry: the instance tables' rows are in another order (TLAS leaves, then the flattened members), but the
	// light meshes keep the ORDER the reference gives them -- that of its own top-level tree's leaves (reference_tlas_order) --:
	// the position of a light in the distribution decides which light a random number selects, i.e. it enters the image
	double total = 0.0;
	size_t rows = tlas_on_device ? scene.meshes.size() : tlas.indices.size();   // the instance tables' rows
	std::vector<int> row_of_mesh;
	const bool reference_order = !tlas_on_device && !reference_tlas_order.empty();
	if (reference_order) {
		row_of_mesh.assign(scene.meshes.size(), -1);
		for (size_t i = 0; i < rows; i++) if (tlas.indices[i] >= 0) row_of_mesh[size_t(tlas.indices[i])] = int(i);
	}
	size_t entries = reference_order ? reference_tlas_order.size() : rows;
	for (size_t k = 0; k < entries; k++) {
		size_t i = reference_order ? size_t(row_of_mesh[size_t(reference_tlas_order[k])]) : k;
		if (!tlas_on_device && tlas.indices[i] < 0) continue;   // the row of the flattened static geometry: its members have rows of their own
		const Mesh & mesh = scene.meshes[tlas_on_device ? int(i) : tlas.indices[i]];
		if (mesh.light.weight > 0.0f) {
			total += double(mesh.light.weight * mesh.scale * mesh.scale);
			light_mesh_cumulative_probability.push_back(float(total));
			light_mesh_triangle_span.push_back(mesh.light.first_triangle_index);
			light_mesh_triangle_span.push_back(mesh.light.first_triangle_index + mesh.light.triangle_count - 1);
			light_mesh_transform_indices.push_back(int(i));
		}
	}
	for (float & p : light_mesh_cumulative_probability) p /= float(total);
	lights_total_weight = float(total);

	if (ctx) check(rt_upload_lights(ctx,
		light_triangle_indices.data(), light_triangle_cumulative_probability.data(), light_triangle_indices.size(),
		light_mesh_cumulative_probability.data(), light_mesh_triangle_span.data(), light_mesh_transform_indices.data(), light_mesh_transform_indices.size(),
		lights_total_weight));
}

// scene.delta_lights -> records with their selection weights, an estimate of the power each sends into the scene: point 4 pi luminance(I); spot
// 2 pi luminance(I) (1 - (cos beam + cos cutoff) / 2), the cone of the mean of its two angles' cosines; directional pi R^2 luminance(E), what the scene's
// bounding sphere intercepts. The share against the triangle emitters (whose lights_total_weight is luminance x area: pi times that is their power) is
// by power, kept inside [0.05, 0.95], unless cpu_config.delta_light_share names one.
void Pathtracer::calc_delta_lights() {
	delta_light_records.clear();
	delta_light_share = 0.0f;
	if (scene.delta_lights.empty()) {
		if (ctx && delta_lights_uploaded) { check(rt_upload_delta_lights(ctx, nullptr, 0, 0.0f)); delta_lights_uploaded = false; delta_lights_on_device.clear(); sample_index = 0; }
		return;
	}
	AABB bounds = AABB::create_empty();
	for (const Mesh & mesh : scene.meshes) bounds.expand(mesh.aabb);
	const double radius = scene.meshes.empty() ? 0.0 : 0.5 * double(Vector3::length(bounds.max - bounds.min));
	const double pi = 3.14159265358979323846;
	double power = 0.0;
	for (const DeltaLight & light : scene.delta_lights) {
		rt_delta_light r = { };
		r.type = int32_t(light.type);
		r.position[0] = light.position.x; r.position[1] = light.position.y; r.position[2] = light.position.z;
		r.direction[0] = light.direction.x; r.direction[1] = light.direction.y; r.direction[2] = light.direction.z;
		r.intensity[0] = light.intensity.x; r.intensity[1] = light.intensity.y; r.intensity[2] = light.intensity.z;
		r.cutoff = light.cutoff; r.beam = light.beam;
		const double luminance = double(Math::luminance(light.intensity));
		double weight = 0.0;
		switch (light.type) {
			case DeltaLight::Type::POINT:       weight = 4.0 * pi * luminance; break;
			case DeltaLight::Type::SPOT:        weight = 2.0 * pi * luminance * (1.0 - 0.5 * (cos(double(light.beam)) + cos(double(light.cutoff)))); break;
			case DeltaLight::Type::DIRECTIONAL: weight = pi * radius * radius * luminance; break;
		}
		r.weight = float(weight);
		power += double(r.weight);
		delta_light_records.push_back(r);
	}
	if (cpu_config.delta_light_share > 0.0f) delta_light_share = cpu_config.delta_light_share;
	else {
		double by_power = power / (power + pi * double(lights_total_weight));
		delta_light_share = float(by_power < 0.05 ? 0.05 : by_power > 0.95 ? 0.95 : by_power);
		if (!(power > 0.0)) delta_light_share = 0.05f;   // (black lights: the upload refuses them with its own message)
	}
	if (!gpu_config.enable_next_event_estimation && !warned_delta_lights_without_nee) {
		fprintf(stderr, "WARNING: the scene's point, spot and directional emitters are found by next-event estimation alone: without it they light nothing\n");
		warned_delta_lights_without_nee = true;
	}
	const bool same = delta_lights_uploaded && delta_light_share == delta_light_share_on_device && delta_light_records.size() == delta_lights_on_device.size()
	                  && memcmp(delta_light_records.data(), delta_lights_on_device.data(), delta_light_records.size() * sizeof(rt_delta_light)) == 0;
	if (ctx && !same) {
		check(rt_upload_delta_lights(ctx, delta_light_records.data(), delta_light_records.size(), delta_light_share));
		delta_lights_uploaded = true; delta_lights_on_device = delta_light_records; delta_light_share_on_device = delta_light_share;
		sample_index = 0;
	}
}

// reference: Pathtracer::update (Pathtracer.cpp:536-736)
void Pathtracer::update(float delta) {
	{   // automatic start: a resize, a change of the scene or of a firefly key drops the measured start -- Integrator::update then puts firefly_start back
		const FireflyStartKey key = { screen_width, screen_height, cpu_config.firefly_filter, cpu_config.firefly_auto_start, cpu_config.firefly_tiers, cpu_config.firefly_start_shift,
		                              cpu_config.firefly_pilot_samples, cpu_config.firefly_start };
		const bool scene_changed = invalidated_sky || invalidated_materials || invalidated_mediums || (invalidated_scene && !cpu_config.enable_scene_update);
		if (scene_changed || memcmp(&key, &firefly_start_key, sizeof(key)) != 0) { firefly_start_key = key; firefly_start_measured = false; firefly_start_in_force = 0.0f; }
	}
	if (invalidated_sky) {
		invalidated_sky = false;
		if (ctx) check(rt_set_sky(ctx, &scene.sky.data[0].x, scene.sky.width, scene.sky.height, scene.sky.scale));
		sample_index = 0;
	}

	if (invalidated_materials) {
		const std::vector<Material> & scene_materials = scene.asset_manager.materials;
		material_types.assign(scene_materials.size(), 0);
		materials.assign(scene_materials.size(), DeviceMaterial());

		for (size_t i = 0; i < scene_materials.size(); i++) {
			const Material & m = scene_materials[i];
			material_types[i] = (unsigned char)m.type;
			switch (m.type) {
				case Material::Type::LIGHT:
					materials[i].light.emission = m.emission;
					break;
				case Material::Type::DIFFUSE:
					materials[i].diffuse.diffuse    = m.diffuse;
					materials[i].diffuse.texture_id = m.texture_handle.handle;
					break;
				case Material::Type::PLASTIC:
					materials[i].plastic.diffuse          = m.diffuse;
					materials[i].plastic.texture_id       = m.texture_handle.handle;
					materials[i].plastic.linear_roughness = m.linear_roughness;
					break;
				case Material::Type::DIELECTRIC:
					materials[i].dielectric.medium_id        = m.medium_handle.handle;
					materials[i].dielectric.ior              = Math::max(m.index_of_refraction, 1.0001f);
					materials[i].dielectric.linear_roughness = m.linear_roughness;
					break;
				case Material::Type::CONDUCTOR:
					materials[i].conductor.eta              = m.eta;
					materials[i].conductor.linear_roughness = m.linear_roughness;
					materials[i].conductor.k                = m.k;
					break;
			}
		}
		if (ctx) check(rt_upload_materials(ctx, material_types.data(), materials.data(), materials.size()));
		// tangent-space normal maps: their own table beside the 32-byte records (rt_upload_materials has reset it to none)
		std::vector<int32_t> normal_maps(scene_materials.size(), INVALID);
		for (size_t i = 0; i < scene_materials.size(); i++) normal_maps[i] = scene_materials[i].normal_map_handle.handle;
		if (ctx) check(rt_upload_material_normal_maps(ctx, normal_maps.data(), normal_maps.size()));
		// opacity masks: built on the device from level 0 of the named data textures (rt_upload_materials has reset them to none).
		// Only the CWBVH kernels test them: under another BVH type the scene renders without its cut-outs.
		std::vector<int32_t> opacity_textures(scene_materials.size(), INVALID), opacity_channels(scene_materials.size(), 0);
		std::vector<float> opacity_thresholds(scene_materials.size(), 0.5f);
		bool any_opacity = false;
		for (size_t i = 0; i < scene_materials.size(); i++) {
			const Material & m = scene_materials[i];
			if (m.opacity_handle.handle == INVALID || m.type == Material::Type::LIGHT) continue;
			const Texture & t = scene.asset_manager.textures[m.opacity_handle.handle];
			if (!t.bc1_blocks.empty()) continue;   // (a colour texture named through the API: not a mask the device can build)
			opacity_textures[i] = m.opacity_handle.handle;
			opacity_channels[i] = m.opacity_channel >= 0 ? m.opacity_channel : (t.file_alpha ? 3 : 0);
			opacity_thresholds[i] = m.opacity_threshold;
			any_opacity = true;
		}
		if (any_opacity && cpu_config.bvh_type != BVHType::BVH8) {
			fprintf(stderr, "WARNING: opacity masks are only tested by the CWBVH kernels (bvh_type 8): rendering without them\n");
			any_opacity = false;
		}
		if (ctx && any_opacity) check(rt_upload_material_opacity(ctx, opacity_textures.data(), opacity_channels.data(), opacity_thresholds.data(), opacity_textures.size()));

		bool had_lights = scene.has_lights;
		scene.check_materials();
		if (had_lights != scene.has_lights) {
			if (scene.has_lights) {
				invalidated_scene = true;
			} else {
				lights_total_weight = 0.0f;
				for (Mesh & mesh : scene.meshes) mesh.light.weight = 0.0f;
				if (ctx) check(rt_upload_lights(ctx, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0.0f));
			}
		}
		if (scene.has_lights) calc_light_power();

		sample_index = 0;
		invalidated_materials = false;
	}

	if (invalidated_mediums) {
		const std::vector<Medium> & scene_media = scene.asset_manager.media;
		media.assign(scene_media.size(), DeviceMedium());
		for (size_t i = 0; i < scene_media.size(); i++) {
			scene_media[i].to_sigmas(media[i].sigma_a, media[i].sigma_s);
			media[i].g = scene_media[i].g;
		}
		if (ctx && !media.empty()) check(rt_upload_media(ctx, media.data(), media.size()));
		sample_index = 0;
		invalidated_mediums = false;
	}

	// The per-mesh light tables (CDF, transform indices) are in TLAS order. With enable_scene_update the TLAS is
	// rebuilt every frame (Integrator::update sets invalidated_scene only after this point), so the tables follow
	// it every frame too. The reference captures the flag here as well but without this term (Pathtracer.cpp:694),
	// i.e. after a TLAS reorder its NEE samples stale instance transforms: a reference flaw, not reproduced.
	bool invalidated_light_mesh_weights = invalidated_scene || cpu_config.enable_scene_update;

	if (gpu_config.enable_svgf) {
		memcpy(&svgf_matrices[0],  scene.camera.view_projection.cells,      64);
		memcpy(&svgf_matrices[16], scene.camera.view_projection_prev.cells, 64);
		if (ctx) check(rt_set_svgf_matrices(ctx, &svgf_matrices[0], &svgf_matrices[16]));
		if (invalidated_aovs && !aov_is_enabled(AOVType::ALBEDO)) aov_enable(AOVType::ALBEDO);
	}

	if (cpu_config.denoise && !gpu_config.enable_svgf) {   // the denoiser's guides (the estimate itself: Integrator::update)
		for (AOVType guide : { AOVType::ALBEDO, AOVType::NORMAL, AOVType::POSITION }) if (!aov_is_enabled(guide)) aov_enable(guide);
	}

	Integrator::update(delta);

	if (gpu_config.enable_svgf && ctx) {
		// the matrices of THIS frame are only known after camera.update(); the reference uploads
		// the pre-update pair (Pathtracer.cpp:707-717), which lags by one frame for a moving camera
		// and is identical for a static one.
	}

	if (invalidated_light_mesh_weights) {
		calc_light_mesh_weights();
		if (!gpu_config.enable_svgf) sample_index = 0;
	}
	if (invalidated_fog) {
		rt_fog_volume v = { };
		if (scene.has_fog) {
			const FogVolume & f = scene.fog;
			const float values[13] = { f.box_min.x, f.box_min.y, f.box_min.z, f.box_max.x, f.box_max.y, f.box_max.z, f.sigma_a.x, f.sigma_a.y, f.sigma_a.z, f.sigma_s.x, f.sigma_s.y, f.sigma_s.z, f.g };
			memcpy(&v, values, sizeof(values));
		}
		if (ctx && (scene.has_fog != fog_on_device || memcmp(&v, &fog_record_on_device, sizeof(v)) != 0)) {
			check(rt_set_fog_volume(ctx, scene.has_fog ? &v : nullptr));
			fog_on_device = scene.has_fog; fog_record_on_device = v;
			sample_index = 0;
		}
		// the density grid: state of its own on the device; uploaded when its values or dims have changed
		const FogDensity & grid = scene.fog_density;
		if (ctx && (scene.has_fog_density != fog_density_on_device || (scene.has_fog_density && (grid.values != fog_density_values_on_device || grid.nx != fog_density_dims_on_device[0] || grid.ny != fog_density_dims_on_device[1] || grid.nz != fog_density_dims_on_device[2])))) {
			check(rt_set_fog_density(ctx, scene.has_fog_density ? grid.values.data() : nullptr, grid.nx, grid.ny, grid.nz));
			fog_density_on_device = scene.has_fog_density;
			fog_density_values_on_device = scene.has_fog_density ? grid.values : std::vector<float>();
			fog_density_dims_on_device[0] = grid.nx; fog_density_dims_on_device[1] = grid.ny; fog_density_dims_on_device[2] = grid.nz;
			sample_index = 0;
		}
		invalidated_fog = false;
	}
	if (ctx) {   // the firefly-robust estimate follows the cascade
		const bool cascade = rt_get_firefly_cascade(ctx, nullptr) != 0;
		if (cpu_config.noise_robust && !cascade && noise_robust_allowed && !warned_noise_robust) {
			fprintf(stderr, "WARNING: noise_robust needs the firefly filter (firefly_filter = 1, plain path tracing): keeping the plain noise estimate\n");
			warned_noise_robust = true;
		}
		const float wanted = cpu_config.noise_robust && cascade && noise_robust_allowed ? cpu_config.noise_held_fraction : 0.0f;
		if (rt_get_noise_robust(ctx) != wanted) check(rt_set_noise_robust(ctx, wanted));
	}
	if (invalidated_light_mesh_weights || invalidated_delta_lights) {   // (after the emitters: the share weighs against their total; after the TLAS: the scene's bounds)
		if (!scene.delta_lights.empty() || !delta_light_records.empty() || delta_lights_uploaded) calc_delta_lights();
		invalidated_delta_lights = false;
	}
}

// A progression that starts over renders the whole frame: the list was selected from the moments of the progression before.
static void restart_drops_pixel_list(rt_context * ctx, int sample_index) {
	if (sample_index < 2 && rt_get_pixel_list(ctx)) rt_set_pixel_list(ctx, 0);
}

float Pathtracer::firefly_start() const {
	rt_firefly_params have = { };
	return ctx && rt_get_firefly_cascade(ctx, &have) ? have.start : cpu_config.firefly_start;
}

bool Pathtracer::firefly_pilot_pending() const {
	return cpu_config.firefly_filter && cpu_config.firefly_auto_start && !firefly_start_measured && !gpu_config.enable_svgf && rt_get_firefly_cascade(ctx, nullptr) != 0;
}

// Automatic start, called before sample `sample_index` is rendered: once the pilot samples 0 .. firefly_pilot_samples - 1 are in the frame, the
// exposure is measured and the start computed; a start other than the one in force is set -- which zeroes the tiers -- and the progression starts over at sample 0.
void Pathtracer::measure_firefly_start() {
	if (!firefly_pilot_pending() || sample_index < cpu_config.firefly_pilot_samples) return;
	rt_exposure exposure = { }; uint64_t histogram[256];
	check(rt_measure_exposure(ctx, &exposure, histogram));
	firefly_start_measured = true;
	float start = 0.0f;
	if (grt_exposure_start(histogram, cpu_config.firefly_start_shift, &start, &firefly_median_exponent) != 0) {
		if (!warned_firefly_start_empty) fprintf(stderr, "WARNING: firefly_auto_start: no pixel of the pilot has a positive finite luminance; keeping firefly_start %g\n", cpu_config.firefly_start);
		warned_firefly_start_empty = true;
		return;
	}
	rt_firefly_params cascade = { };
	rt_get_firefly_cascade(ctx, &cascade);
	firefly_start_in_force = start;
	if (cascade.start == start) return;
	cascade.start = start;
	check(rt_set_firefly_cascade(ctx, &cascade));
	firefly_pilot_samples_discarded += sample_index;
	sample_index = 0;
}

void Pathtracer::render() {
	require_device();
	measure_firefly_start();
	restart_drops_pixel_list(ctx, sample_index);
	check(rt_render_sample(ctx, sample_index));
	if (pixel_query_status == PixelQueryStatus::PENDING) pixel_query_status = PixelQueryStatus::OUTPUT_READY; // Pathtracer.cpp:852-854
}

void Pathtracer::render_samples(int count) {
	require_device();
	if (count < 1) return;
	measure_firefly_start();
	restart_drops_pixel_list(ctx, sample_index);
	if (pixel_query_status == PixelQueryStatus::PENDING) pixel_query_status = PixelQueryStatus::OUTPUT_READY;
	if (gpu_config.enable_svgf) { // SVGF frames feed each other's history: one at a time
		for (int i = 0; i < count; i++) { if (i) sample_index++; check(rt_render_sample(ctx, sample_index)); }
		return;
	}
	while (count > 0) {
		int n = count < 16 ? count : 16;
		if (firefly_pilot_pending() && sample_index < cpu_config.firefly_pilot_samples && n > cpu_config.firefly_pilot_samples - sample_index) n = cpu_config.firefly_pilot_samples - sample_index;   // the pilot ends a burst
		check(rt_render_samples(ctx, sample_index, n));
		sample_index += n - 1;
		count -= n;
		if (count > 0) { sample_index++; measure_firefly_start(); restart_drops_pixel_list(ctx, sample_index); }
	}
}

int grt_noise_summary(const double * cell_sums, const int32_t * cell_counts, size_t cells, double quantile, double * out_mean, double * out_figure, long long * out_pixels) {
	if (out_mean) *out_mean = 0.0;
	if (out_figure) *out_figure = 0.0;
	if (out_pixels) *out_pixels = 0;
	if (!(quantile > 0.0 && quantile <= 1.0)) return -1;
	double sum = 0.0; long long pixels = 0;
	std::vector<double> means;
	for (size_t c = 0; c < cells; c++) {
		if (cell_counts[c] <= 0) continue;
		sum += cell_sums[c]; pixels += cell_counts[c];
		means.push_back(cell_sums[c] / double(cell_counts[c]));
	}
	if (out_pixels) *out_pixels = pixels;
	if (means.empty()) return 1;
	std::sort(means.begin(), means.end());
	size_t rank = size_t(std::ceil(quantile * double(means.size())));
	rank = rank < 1 ? 1 : rank > means.size() ? means.size() : rank;
	if (out_mean) *out_mean = sum / double(pixels);
	if (out_figure) *out_figure = means[rank - 1];
	return 0;
}

// The cascade's start from the exposure histogram of rt_measure_exposure: two to the median exponent plus `shift`. The median bin is the
// smallest bin whose cumulative count reaches rank (pixels + 1) / 2; the exponent is clamped to -96 .. 96, which keeps start * 8^7 finite. 1, with nothing
// written, for an empty histogram.
int grt_exposure_start(const uint64_t * histogram256, int shift, float * out_start, int * out_median_exponent) {
	uint64_t pixels = 0;
	for (int b = 0; b < 256; b++) pixels += histogram256[b];
	if (pixels == 0) return 1;
	const uint64_t rank = pixels / 2 + pixels % 2;   // (pixels + 1) / 2 without the overflow
	uint64_t reached = 0; int bin = 0;
	for (; bin < 256; bin++) { reached += histogram256[bin]; if (reached >= rank) break; }
	int exponent = bin - 127 + shift;
	exponent = exponent < -96 ? -96 : exponent > 96 ? 96 : exponent;
	if (out_start) *out_start = std::ldexp(1.0f, exponent);
	if (out_median_exponent) *out_median_exponent = exponent;
	return 0;
}

NoiseEstimate Pathtracer::noise(std::vector<float> * pixel_map, bool allow_empty) {
	require_device();
	if (!rt_get_noise_estimate(ctx)) throw std::runtime_error("Pathtracer::noise: the noise estimate is off (set noise_estimate_wanted or cpu_config.noise_target before update())");
	NoiseEstimate e;
	e.cells_x = (screen_width + 15) / 16; e.cells_y = (screen_height + 15) / 16;
	const size_t cells = size_t(e.cells_x) * e.cells_y;
	e.cell_sums.assign(cells, 0.0); e.cell_counts.assign(cells, 0); e.cell_nonfinite.assign(cells, 0);
	if (pixel_map) pixel_map->assign(size_t(screen_pitch) * screen_height, -1.0f);
	rt_noise_estimate out = { };
	const float held_fraction = rt_get_noise_robust(ctx);   // (update() keeps it at cpu_config.noise_held_fraction while noise_robust is in force)
	e.robust = held_fraction > 0.0f;
	int status;
	if (e.robust) {
		e.cell_held.assign(cells, 0);
		int64_t held = 0;
		status = rt_estimate_noise_robust(ctx, cpu_config.noise_floor, held_fraction, &out, e.cell_sums.data(), e.cell_counts.data(), e.cell_nonfinite.data(), e.cell_held.data(), cells,
		                                  pixel_map ? pixel_map->data() : nullptr, &held);
		e.held_pixels = held;
	} else status = rt_estimate_noise(ctx, cpu_config.noise_floor, &out, e.cell_sums.data(), e.cell_counts.data(), e.cell_nonfinite.data(), cells, pixel_map ? pixel_map->data() : nullptr);
	if (!(status == RT_ERROR_NOT_READY && allow_empty && out.cells_x == e.cells_x)) check(status);   // (an empty frame's arrays and counters are filled before the refusal)
	e.nonfinite_pixels = out.nonfinite_pixels;
	grt_noise_summary(e.cell_sums.data(), e.cell_counts.data(), cells, cpu_config.noise_quantile, &e.mean, &e.figure, &e.pixels);
	last_noise_robust = e.robust; last_noise_held_pixels = e.held_pixels; last_noise_cell_held = e.cell_held;
	return e;
}

AdaptiveSelection Pathtracer::select_adaptive(float threshold) {
	require_device();
	if (!rt_get_noise_estimate(ctx)) throw std::runtime_error("Pathtracer::select_adaptive: the noise estimate is off (set noise_estimate_wanted or cpu_config.noise_target before update())");
	rt_cell_selection out = { };
	check(rt_select_active_cells(ctx, cpu_config.noise_floor, threshold, cpu_config.adaptive_dilate ? 1 : 0, &out, nullptr, 0));
	check(rt_set_pixel_list(ctx, out.list_pixels > 0 ? 1 : 0));
	AdaptiveSelection a;
	a.cells = (long long)out.cells_x * out.cells_y; a.hot_cells = out.hot_cells; a.active_cells = out.active_cells; a.list_pixels = out.list_pixels;
	return a;
}

void Pathtracer::adaptive_off() {
	require_device();
	check(rt_set_pixel_list(ctx, 0));
}

rt_denoise_params Pathtracer::denoise_defaults() {
	rt_denoise_params p = { cpu_config.denoise_iterations, cpu_config.denoise_sigma_l, cpu_config.denoise_sigma_n, cpu_config.denoise_sigma_z, cpu_config.denoise_depth_floor, cpu_config.denoise_albedo_floor };
	return p;
}

std::vector<float> Pathtracer::denoise(const rt_denoise_params * params) {
	require_device();
	const rt_denoise_params p = params ? *params : denoise_defaults();
	check(rt_denoise(ctx, &p));
	std::vector<float> image(size_t(screen_pitch) * screen_height * 4);
	check(rt_read_denoised(ctx, image.data()));
	return image;
}

void Pathtracer::save_denoised_image(const std::string & filename, const rt_denoise_params * params) {
	const std::vector<float> rgba = denoise(params);
	std::vector<Vector3> rgb(rgba.size() / 4);
	for (size_t i = 0; i < rgb.size(); i++) rgb[i] = Vector3(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
	std::string error;
	if (!Exporters::save(filename, screen_pitch, screen_width, screen_height, rgb, &error)) throw std::runtime_error(error);
}

std::vector<float> Pathtracer::resolve_fireflies(float support) {
	require_device();
	check(rt_resolve_fireflies(ctx, support > 0.0f ? support : cpu_config.firefly_support));
	std::vector<float> image(size_t(screen_pitch) * screen_height * 4);
	check(rt_read_resolved(ctx, image.data()));
	return image;
}

void Pathtracer::save_resolved_image(const std::string & filename, float support) {
	const std::vector<float> rgba = resolve_fireflies(support);
	std::vector<Vector3> rgb(rgba.size() / 4);
	for (size_t i = 0; i < rgb.size(); i++) rgb[i] = Vector3(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
	std::string error;
	if (!Exporters::save(filename, screen_pitch, screen_width, screen_height, rgb, &error)) throw std::runtime_error(error);
}

double Pathtracer::sample_counts(std::vector<float> * counts) {
	require_device();
	std::vector<float> moments(size_t(screen_pitch) * screen_height * 4);
	check(rt_read_noise_moments(ctx, moments.data()));
	if (counts) counts->assign(size_t(screen_pitch) * screen_height, 0.0f);
	double sum = 0.0;
	for (int y = 0; y < screen_height; y++) for (int x = 0; x < screen_width; x++) {
		const float w = moments[(size_t(x) + size_t(y) * screen_pitch) * 4 + 3];
		if (counts) (*counts)[size_t(x) + size_t(y) * screen_pitch] = w;
		sum += double(w);
	}
	return sum / (double(screen_width) * double(screen_height));
}
