// rt_bsdf.h -- the four BSDFs (CUDA/BSDF.h) and the albedo fetch they share: what shade_material (rt_material.h) shades a hit with and what
// kernel_bsdf_probe (kernels_probes.hip) runs on its own.
#pragma once
#include "rt_shading.h"

struct TextureLOD { f2 gradient_1, gradient_2; float lod; };

template<bool COMPRESSED>
RT_DEV f3 sample_albedo(const RtParams & p, int bounce, f3 diffuse, int texture_id, const RtTexture & tex, f2 tex_coord, const TextureLOD & lod) { // RayCone.h:19-29
	if (texture_id == RT_INVALID) return diffuse;
	if (p.config.enable_mipmapping) {
		if (bounce == 0) return diffuse * mk3(texture_get_grad<COMPRESSED>(tex, tex_coord.x, tex_coord.y, lod.gradient_1, lod.gradient_2));
		return diffuse * mk3(texture_get_lod<COMPRESSED>(tex, tex_coord.x, tex_coord.y, lod.lod + tex.lod_bias));
	}
	return diffuse * mk3(texture_get<COMPRESSED>(tex, tex_coord.x, tex_coord.y));
}
template<bool COMPRESSED>
RT_DEV f3 sample_albedo(const RtParams & p, int bounce, f3 diffuse, int texture_id, f2 tex_coord, const TextureLOD & lod) {
	if (texture_id == RT_INVALID) return diffuse;
	const RtTexture tex = p.textures[texture_id];
	return sample_albedo<COMPRESSED>(p, bounce, diffuse, texture_id, tex, tex_coord, lod);
}

struct BSDFCommon {
	int pixel_index, bounce, sample_index;
	RandomPath rng;   // random_path(pixel_index, sample_index): what every random_sample of this hit shares
	f3 tangent, bitangent, normal, omega_i;
};

// COMPRESSED: whether a texture may hold BC1 blocks to be decoded per fetch (see texture_bilinear)
template<bool COMPRESSED>
struct BSDFDiffuseT : BSDFCommon {
	static constexpr bool HAS_ALBEDO = true;
	static constexpr bool MAP_COMPRESSED = COMPRESSED;   // the texture instantiation a normal map is read with (the _nmap instances)
	f3 diffuse; int texture_id; f3 albedo;
	RT_DEV void init(const RtParams & p, bool, int material_id) { float4 m = p.materials[2 * material_id]; diffuse = mk3(m.x, m.y, m.z); texture_id = __float_as_int(m.w); }
	RT_DEV void calc_albedo(const RtParams & p, f3 & throughput, f2 tex_coord, const TextureLOD & lod) {
		albedo = sample_albedo<COMPRESSED>(p, bounce, diffuse, texture_id, tex_coord, lod);
		if (bounce == 0) aov_set(p, RT_AOV_ALBEDO, pixel_index, mk4(albedo));
		if (!(p.config.enable_svgf && bounce == 0)) throughput *= albedo;
	}
	RT_DEV bool eval(const RtParams &, f3, float cos_theta_o, f3 & bsdf, float & pdf) const {
		if (cos_theta_o <= 0.0f) return false;
		bsdf = mk3(cos_theta_o * RT_ONE_OVER_PI);
		pdf  = cos_theta_o * RT_ONE_OVER_PI;
		return pdf_is_valid(pdf);
	}
	RT_DEV bool sample(const RtParams & p, f3 &, int &, f3 & direction_out, float & pdf) const {
		f2 r = random_sample(p, rng, DIM_BSDF_0, unsigned(bounce));
		f3 omega_o = sample_cosine_weighted_direction(r.x, r.y);
		direction_out = local_to_world(omega_o, tangent, bitangent, normal);
		pdf = omega_o.z * RT_ONE_OVER_PI;
		return pdf_is_valid(pdf);
	}
	RT_DEV bool has_texture() const { return texture_id != RT_INVALID; }
	RT_DEV bool allow_nee() const { return true; }
};

typedef BSDFDiffuseT<true> BSDFDiffuse;

template<bool COMPRESSED>
struct BSDFPlasticT : BSDFCommon {
	static constexpr bool HAS_ALBEDO = true;
	static constexpr bool MAP_COMPRESSED = COMPRESSED;
	static constexpr float IOR = 1.5f;
	static constexpr float ETA = 1.0f / IOR;
	f3 diffuse; int texture_id; float linear_roughness; f3 albedo;
	float F_i, lambda_i, G1_i;
	RT_DEV void init(const RtParams & p, bool, int material_id) {
		float4 m = p.materials[2 * material_id]; diffuse = mk3(m.x, m.y, m.z); texture_id = __float_as_int(m.w);
		linear_roughness = p.materials[2 * material_id + 1].x;
		// what the light sample's evaluation (eval) and the bounce (sample) both need of the incoming direction, computed once per hit
		float ax = roughness_to_alpha(linear_roughness);
		F_i = fresnel_dielectric(omega_i.z, ETA);
		lambda_i = ggx_lambda(omega_i, ax, ax);
		G1_i = 1.0f / (1.0f + lambda_i);   // ggx_G1(omega_i, ax, ay)
	}
	// ggx_G2(omega_o, omega_i, omega_m, ax, ay) with the cached lambda of omega_i (the sum in the function's order)
	RT_DEV float G2_with(f3 omega_o, f3 omega_m, float ax, float ay) const {
		bool i_back = dot(omega_i, omega_m) * omega_i.z <= 0.0f;
		bool o_back = dot(omega_o, omega_m) * omega_o.z <= 0.0f;
		if (i_back || o_back) return 0.0f;
		return 1.0f / (1.0f + ggx_lambda(omega_o, ax, ay) + lambda_i);
	}
	RT_DEV void calc_albedo(const RtParams & p, f3 &, f2 tex_coord, const TextureLOD & lod) {
		albedo = sample_albedo<COMPRESSED>(p, bounce, diffuse, texture_id, tex_coord, lod);
		if (bounce == 0) aov_set(p, RT_AOV_ALBEDO, pixel_index, mk4(albedo));
	}
	RT_DEV f3 diffuse_lobe(float F_i, float F_o, float cos_o) const {
		float F_avg = average_fresnel(IOR);
		float internal_scattering_factor = 1.0f - (1.0f - F_avg) * square(ETA);
		return ETA * ETA * (1.0f - F_i) * (1.0f - F_o) * albedo * RT_ONE_OVER_PI / (1.0f - albedo * internal_scattering_factor) * cos_o;
	}
	RT_DEV bool eval(const RtParams &, f3 to_light, float cos_theta_o, f3 & bsdf, float & pdf) const {
		if (cos_theta_o <= 0.0f) return false;
		f3 omega_o = world_to_local(to_light, tangent, bitangent, normal);
		f3 omega_m = normalize(omega_i + omega_o);
		float ax = roughness_to_alpha(linear_roughness), ay = ax;
		float F  = fresnel_dielectric(dot(omega_i, omega_m), ETA);
		float D  = ggx_D(omega_m, ax, ay);
		float G1 = G1_i;
		float G2 = G2_with(omega_o, omega_m, ax, ay);
		f3 brdf_specular = mk3(F * G2 * D / (4.0f * omega_i.z));
		float F_o = fresnel_dielectric(omega_o.z, ETA);
		f3 brdf_diffuse = diffuse_lobe(F_i, F_o, omega_o.z);
		float pdf_specular = G1 * D / (4.0f * omega_i.z);
		float pdf_diffuse  = omega_o.z * RT_ONE_OVER_PI;
		pdf  = lerp_ref(pdf_diffuse, pdf_specular, F_i);
		bsdf = brdf_specular + brdf_diffuse;
		return pdf_is_valid(pdf);
	}
	RT_DEV bool sample(const RtParams & p, f3 & throughput, int &, f3 & direction_out, float & pdf) const {
		float rand_fresnel = random_sample(p, rng, DIM_BSDF_0, unsigned(bounce)).x;
		f2    rand_brdf    = random_sample(p, rng, DIM_BSDF_1, unsigned(bounce));
		float ax = roughness_to_alpha(linear_roughness), ay = ax;
		f3 omega_m, omega_o;
		if (rand_fresnel < F_i) {
			omega_m = sample_visible_normals_ggx(omega_i, ax, ay, rand_brdf.x, rand_brdf.y);
			omega_o = reflect_direction(omega_i, omega_m);
		} else {
			omega_o = sample_cosine_weighted_direction(rand_brdf.x, rand_brdf.y);
			omega_m = normalize(omega_i + omega_o);
		}
		if (omega_m.z < 0.0f) return false;
		float F  = fresnel_dielectric(dot(omega_i, omega_m), ETA);
		float D  = ggx_D(omega_m, ax, ay);
		float G1 = G1_i;
		float G2 = G2_with(omega_o, omega_m, ax, ay);
		f3 brdf_specular = mk3(F * G2 * D / (4.0f * omega_i.z));
		float F_o = fresnel_dielectric(omega_o.z, ETA);
		f3 brdf_diffuse = diffuse_lobe(F_i, F_o, omega_o.z);
		float pdf_specular = G1 * D / (4.0f * omega_i.z);
		float pdf_diffuse  = omega_o.z * RT_ONE_OVER_PI;
		pdf = lerp_ref(pdf_diffuse, pdf_specular, F_i);
		throughput *= (brdf_specular + brdf_diffuse) / pdf;
		direction_out = local_to_world(omega_o, tangent, bitangent, normal);
		return pdf_is_valid(pdf);
	}
	RT_DEV bool has_texture() const { return texture_id != RT_INVALID; }
	RT_DEV bool allow_nee() const { return true; }
};

typedef BSDFPlasticT<true> BSDFPlastic;

struct BSDFDielectric : BSDFCommon {
	static constexpr bool HAS_ALBEDO = false;
	static constexpr bool MAP_COMPRESSED = false;   // (normal maps are RGBA8: rt_upload_material_normal_maps)
	int medium_id_material; float ior, linear_roughness, eta;
	RT_DEV void init(const RtParams & p, bool entering_material, int material_id) {
		float4 m = p.materials[2 * material_id];
		medium_id_material = __float_as_int(m.x); ior = m.y; linear_roughness = m.z;
		eta = entering_material ? 1.0f / ior : ior;
	}
	RT_DEV void calc_albedo(const RtParams &, f3 &, f2, const TextureLOD &) { }

	struct Lobes { float bsdf_single, bsdf_multi, pdf_single, pdf_multi; };
	RT_DEV Lobes lobes(const RtParams & p, bool reflected, bool entering_material, f3 omega_o, f3 omega_m, float F, float E_i, float ratio, float E_avg_enter, float E_avg_leave) const {
		float ax = roughness_to_alpha(linear_roughness), ay = ax;
		float D  = ggx_D(omega_m, ax, ay);
		float G1 = ggx_G1(omega_i, ax, ay);
		float G2 = ggx_G2(omega_o, omega_i, omega_m, ax, ay);
		float i_dot_m = abs_dot(omega_i, omega_m);
		float o_dot_m = abs_dot(omega_o, omega_m);
		Lobes l;
		if (reflected) {
			l.bsdf_single = F * G2 * D / (4.0f * omega_i.z);
			l.pdf_single  = F * G1 * D / (4.0f * omega_i.z);
			float E_o   = dielectric_directional_albedo(p, ior, linear_roughness, omega_o.z, entering_material);
			float E_avg = entering_material ? E_avg_enter : E_avg_leave;
			l.bsdf_multi = (1.0f - ratio) * fabsf(omega_o.z) * kulla_conty_multiscatter_lobe(E_i, E_o, E_avg);
			l.pdf_multi  = (1.0f - ratio) * fabsf(omega_o.z) * RT_ONE_OVER_PI;
		} else {
			l.bsdf_single = (1.0f - F) * G2 * D * i_dot_m * o_dot_m / (omega_i.z * square(eta * i_dot_m + o_dot_m) * square(eta));
			l.pdf_single  = (1.0f - F) * G1 * D * i_dot_m * o_dot_m / (omega_i.z * square(eta * i_dot_m + o_dot_m));
			float E_o   = dielectric_directional_albedo(p, ior, linear_roughness, omega_o.z, !entering_material);
			float E_avg = entering_material ? E_avg_leave : E_avg_enter; // inverted on purpose (BSDF.h:281)
			l.bsdf_multi = ratio * fabsf(omega_o.z) * kulla_conty_multiscatter_lobe(E_i, E_o, E_avg);
			l.pdf_multi  = ratio * fabsf(omega_o.z) * RT_ONE_OVER_PI;
		}
		return l;
	}
	RT_DEV void common(const RtParams & p, bool & entering_material, float & E_i, float & ratio, float & E_avg_enter, float & E_avg_leave) const {
		entering_material = eta < 1.0f;
		E_i = dielectric_directional_albedo(p, ior, linear_roughness, omega_i.z, entering_material);
		float F_avg = average_fresnel(ior);
		if (!entering_material) F_avg = 1.0f - (1.0f - F_avg) / square(ior);
		E_avg_enter = dielectric_albedo(p, ior, linear_roughness, true);
		E_avg_leave = dielectric_albedo(p, ior, linear_roughness, false);
		float x = kulla_conty_dielectric_reciprocity_factor(E_avg_enter, E_avg_leave);
		ratio = (entering_material ? x : (1.0f - x)) * (1.0f - F_avg);
	}
	RT_DEV bool eval(const RtParams & p, f3 to_light, float, f3 & bsdf, float & pdf) const {
		f3 omega_o = world_to_local(to_light, tangent, bitangent, normal);
		bool reflected = omega_o.z >= 0.0f;
		f3 omega_m = reflected ? normalize(omega_i + omega_o) : normalize(eta * omega_i + omega_o);
		omega_m *= sign_of(omega_m.z);
		float F = fresnel_dielectric(abs_dot(omega_i, omega_m), eta);
		bool entering_material; float E_i, ratio, E_avg_enter, E_avg_leave;
		common(p, entering_material, E_i, ratio, E_avg_enter, E_avg_leave);
		Lobes l = lobes(p, reflected, entering_material, omega_o, omega_m, F, E_i, ratio, E_avg_enter, E_avg_leave);
		bsdf = mk3(l.bsdf_single + l.bsdf_multi);
		pdf = lerp_ref(l.pdf_multi, l.pdf_single, E_i);
		return pdf_is_valid(pdf);
	}
	RT_DEV bool sample(const RtParams & p, f3 & throughput, int & medium_id, f3 & direction_out, float & pdf) const {
		f2 r0 = random_sample(p, rng, DIM_BSDF_0, unsigned(bounce));
		f2 r1 = random_sample(p, rng, DIM_BSDF_1, unsigned(bounce));
		float ax = roughness_to_alpha(linear_roughness), ay = ax;
		bool entering_material; float E_i, ratio, E_avg_enter, E_avg_leave;
		common(p, entering_material, E_i, ratio, E_avg_enter, E_avg_leave);

		float F; bool reflected; f3 omega_m, omega_o;
		if (r0.x < E_i) {
			omega_m = sample_visible_normals_ggx(omega_i, ax, ay, r1.x, r1.y);
			F = fresnel_dielectric(abs_dot(omega_i, omega_m), eta);
			reflected = r0.y < F;
			omega_o = reflected ? reflect_direction(omega_i, omega_m) : refract_direction(omega_i, omega_m, eta);
		} else {
			omega_o = sample_cosine_weighted_direction(r1.x, r1.y);
			reflected = r0.y > ratio;
			if (reflected) {
				omega_m = normalize(omega_i + omega_o);
			} else {
				omega_o = -omega_o;
				omega_m = normalize(eta * omega_i + omega_o);
			}
			omega_m *= sign_of(omega_m.z);
			F = fresnel_dielectric(abs_dot(omega_i, omega_m), eta);
		}
		if (reflected ^ (omega_o.z >= 0.0f)) return false;

		Lobes l = lobes(p, reflected, entering_material, omega_o, omega_m, F, E_i, ratio, E_avg_enter, E_avg_leave);
		if (!reflected) medium_id = entering_material ? medium_id_material : RT_INVALID;
		pdf = lerp_ref(l.pdf_multi, l.pdf_single, E_i);
		throughput *= (l.bsdf_single + l.bsdf_multi) / pdf;
		direction_out = local_to_world(omega_o, tangent, bitangent, normal);
		return pdf_is_valid(pdf);
	}
	RT_DEV bool has_texture() const { return false; }
	RT_DEV bool allow_nee() const { return linear_roughness >= RT_ROUGHNESS_CUTOFF; }
};

struct BSDFConductor : BSDFCommon {
	static constexpr bool HAS_ALBEDO = false;
	static constexpr bool MAP_COMPRESSED = false;
	f3 eta3, k3; float linear_roughness;
	RT_DEV void init(const RtParams & p, bool, int material_id) {
		float4 a = p.materials[2 * material_id], b = p.materials[2 * material_id + 1];
		eta3 = mk3(a.x, a.y, a.z); linear_roughness = a.w; k3 = mk3(b.x, b.y, b.z);
	}
	RT_DEV void calc_albedo(const RtParams &, f3 &, f2, const TextureLOD &) { }
	RT_DEV void lobes(const RtParams & p, f3 omega_o, f3 omega_m, float o_dot_m, float E_i, f3 & brdf, float & pdf) const {
		float ax = roughness_to_alpha(linear_roughness), ay = ax;
		f3    F  = fresnel_conductor(o_dot_m, eta3, k3);
		float D  = ggx_D(omega_m, ax, ay);
		float G1 = ggx_G1(omega_i, ax, ay);
		float G2 = ggx_G2(omega_o, omega_i, omega_m, ax, ay);
		f3    brdf_single = F * G2 * D / (4.0f * omega_i.z);
		float pdf_single  =     G1 * D / (4.0f * omega_i.z);
		float E_o   = conductor_directional_albedo(p, linear_roughness, omega_o.z);
		float E_avg = conductor_albedo(p, linear_roughness);
		f3 F_avg = average_fresnel(eta3, k3);
		f3 F_ms  = fresnel_multiscatter(F_avg, E_avg);
		f3    brdf_multi = F_ms * kulla_conty_multiscatter_lobe(E_i, E_o, E_avg) * omega_o.z;
		float pdf_multi  = omega_o.z * RT_ONE_OVER_PI;
		brdf = brdf_single + brdf_multi;
		pdf = lerp_ref(pdf_multi, pdf_single, E_i);
	}
	RT_DEV bool eval(const RtParams & p, f3 to_light, float cos_theta_o, f3 & bsdf, float & pdf) const {
		if (cos_theta_o <= 0.0f) return false;
		f3 omega_o = world_to_local(to_light, tangent, bitangent, normal);
		f3 omega_m = normalize(omega_o + omega_i);
		float o_dot_m = dot(omega_o, omega_m);
		if (o_dot_m <= 0.0f) return false;
		float E_i = conductor_directional_albedo(p, linear_roughness, omega_i.z);
		lobes(p, omega_o, omega_m, o_dot_m, E_i, bsdf, pdf);
		return pdf_is_valid(pdf);
	}
	RT_DEV bool sample(const RtParams & p, f3 & throughput, int &, f3 & direction_out, float & pdf) const {
		f2 r0 = random_sample(p, rng, DIM_BSDF_0, unsigned(bounce));
		f2 r1 = random_sample(p, rng, DIM_BSDF_1, unsigned(bounce));
		float ax = roughness_to_alpha(linear_roughness), ay = ax;
		float E_i = conductor_directional_albedo(p, linear_roughness, omega_i.z);
		f3 omega_m, omega_o;
		if (r0.x < E_i) {
			omega_m = sample_visible_normals_ggx(omega_i, ax, ay, r1.x, r1.y);
			omega_o = reflect_direction(omega_i, omega_m);
		} else {
			omega_o = sample_cosine_weighted_direction(r1.x, r1.y);
			omega_m = normalize(omega_i + omega_o);
		}
		float o_dot_m = dot(omega_o, omega_m);
		if (o_dot_m <= 0.0f || omega_o.z < 0.0f) return false;
		f3 brdf;
		lobes(p, omega_o, omega_m, o_dot_m, E_i, brdf, pdf);
		throughput *= brdf / pdf;
		direction_out = local_to_world(omega_o, tangent, bitangent, normal);
		return pdf_is_valid(pdf);
	}
	RT_DEV bool has_texture() const { return false; }
	RT_DEV bool allow_nee() const { return linear_roughness >= RT_ROUGHNESS_CUTOFF; }
};
