// Scene-level material / medium / texture descriptions
// (reference: Src/Renderer/Material.h, Medium.h, Texture.h).
#pragma once
#include <string>
#include <vector>

#include "Handle.h"

struct Texture {
	std::string name;
	int width = 0, height = 0;
	// Linear-light RGBA8 texels for every mip level, level 0 first.
	std::vector<unsigned char> texels;
	std::vector<size_t> mip_offsets; // in texels (4 bytes each)
	// Size that enters the LOD bias; 0 = width / height. Block counts for a BC1-compressed texture, as in
	// the reference (TextureLoader.cpp:256-258 overwrite width / height, Integrator.cpp:95 reads them).
	int lod_width = 0, lod_height = 0;
	// BC1 blocks (8 bytes per 4x4 texels, rows of blocks, all kept levels back to back) of a block-compressed
	// texture: what the device stores and decodes in its texel fetch. `texels` then holds the decoded levels --
	// the same values, for the host-side consumers (exporters, the parity checker).
	std::vector<unsigned char> bc1_blocks;
	// A data texture (a tangent-space normal map): texels are the file's bytes as stored -- no sRGB decode, mips filtered on
	// the raw values, never block-compressed.
	bool data = false;
	// The file it was decoded from, and whether that file stores an alpha (fourth) channel -- what an opacity mask reads (Material::opacity_handle)
	std::string filename;
	bool file_alpha = false;

	int mip_levels() const { return int(mip_offsets.size()); }
};

struct Medium {
	std::string name;

	Vector3 C   = 1.0f; // multi-scatter albedo
	Vector3 mfp = 1.0f; // mean free path
	float   g   = 0.0f; // Henyey-Greenstein mean cosine

	// Van de Hulst albedo inversion, both directions (reference: Renderer/Medium.h:18-37)
	void from_sigmas(const Vector3 & sigma_a, const Vector3 & sigma_s) {
		Vector3 sigma_t = sigma_a + sigma_s;
		Vector3 alpha = sigma_s / sigma_t;
		Vector3 s = Vector3::apply((1.0f - alpha) / (1.0f - alpha * g), sqrtf);
		C   = (1.0f - s) * (1.0f - 0.139f * s) / (1.0f + 1.17f * s);
		mfp = 1.0f / sigma_t;
	}
	void to_sigmas(Vector3 & sigma_a, Vector3 & sigma_s) const {
		Vector3 s = 4.09712f + 4.20863f * C - Vector3::apply(9.59217f + 41.6808f * C + 17.7126f * C * C, sqrtf);
		Vector3 alpha = (1.0f - s * s) / (1.0f - Math::clamp(g, -0.999f, 0.999f) * s * s);
		Vector3 sigma_t = 1.0f / Vector3::max(mfp, 1e-6f);
		sigma_s = alpha * sigma_t;
		sigma_a = sigma_t - sigma_s;
	}
};

struct Material {
	std::string name;

	enum struct Type : char { LIGHT, DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR };
	Type type = Type::DIFFUSE;

	Vector3 emission;

	Vector3         diffuse = Vector3(1.0f, 1.0f, 1.0f);
	Handle<Texture> texture_handle;
	Handle<Texture> normal_map_handle;   // tangent-space normal map (a data texture), INVALID: none
	// Opacity mask: a data texture whose level 0 cuts holes into the surface -- texels whose `opacity_channel` byte is below
	// ceil(opacity_threshold * 255) let rays through. INVALID: none. Channel -1: alpha when the file has four channels, red otherwise
	// (known once the file is decoded: resolved_opacity_channel). opacity_from_albedo: set by cpu_config.alpha_masks, kept only if the file's alpha
	// turns out to vary (AssetManager::wait_until_loaded drops it otherwise).
	Handle<Texture> opacity_handle;
	int   opacity_channel = -1;
	float opacity_threshold = 0.5f;
	bool  opacity_from_albedo = false;

	Handle<Medium> medium_handle;
	float          index_of_refraction = 1.33f;

	Vector3 eta = Vector3(1.33f);
	Vector3 k   = Vector3(1.0f);

	float linear_roughness = 0.5f;

	bool is_light() const { return type == Type::LIGHT && Vector3::length_squared(emission) > 0.0f; }
};
