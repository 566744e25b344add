// Scene = asset tables + placed meshes + camera + sky, with the reference's member
// names (Src/Renderer/Scene.h, Src/Assets/AssetManager.h) so that code written
// against `scene.asset_manager.materials` / `scene.meshes` / `scene.camera` ports over.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "Camera.h"
#include "Config.h"
#include "Mesh.h"

struct Sky {
	std::vector<Vector4> data;
	int   width  = 0;
	int   height = 0;
	float scale  = 1.0f;

	// Radiance .hdr (RGBE) loader; an empty file name gives a 1x1 white sky, the
	// stand-in for the HDR files missing from the reference mount.
	void load(const std::string & filename);
};

struct AssetManager {
	std::vector<MeshData> mesh_datas;
	std::vector<Material> materials;
	std::vector<Medium>   media;
	std::vector<Texture>  textures;

	AssetManager();

	using FallbackLoader = std::function<std::vector<Triangle>(const std::string & filename)>;

	Handle<MeshData> add_mesh_data(const std::string & filename, FallbackLoader loader);
	// `filename` keys the mesh (and is what the loader receives); `bvh_filename` names its cache file
	Handle<MeshData> add_mesh_data(const std::string & filename, const std::string & bvh_filename, FallbackLoader loader);
	Handle<MeshData> add_mesh_data(std::vector<Triangle> triangles);
	Handle<Material> add_material(Material material);
	Handle<Medium>   add_medium(Medium medium);
	// kind DATA: the texels are values, not colours (normal maps), see Texture::data; a file is cached once per kind.
	// Once the assets are loaded a new texture is decoded right away.
	enum struct TextureKind { COLOUR, DATA };
	Handle<Texture>  add_texture(const std::string & filename, const std::string & name, TextureKind kind = TextureKind::COLOUR);

	// Builds every pending BLAS (one job per mesh file on a thread pool) and decodes textures.
	void wait_until_loaded();
	void add_alpha_masks();   // cpu_config.alpha_masks: masks from the albedo files' alpha channels (before the assets are loaded)
	void prepare_device_bvhs(BVHType type); // builds MeshData::device_bvh* for a non-BVH8 type, in parallel

	MeshData & get_mesh_data(Handle<MeshData> h) { return mesh_datas[h.handle]; }
	Material & get_material (Handle<Material> h) { return materials [h.handle]; }
	Medium   & get_medium   (Handle<Medium>   h) { return media     [h.handle]; }
	Texture  & get_texture  (Handle<Texture>  h) { return textures  [h.handle]; }
	const MeshData & get_mesh_data(Handle<MeshData> h) const { return mesh_datas[h.handle]; }
	const Material & get_material (Handle<Material> h) const { return materials [h.handle]; }

	double bvh_build_ms = 0.0; // wall time of the parallel BLAS build

private:
	std::map<std::string, Handle<MeshData>> mesh_data_cache;
	std::map<std::pair<std::string, TextureKind>, Handle<Texture>> texture_cache;

	struct PendingMesh    { int handle; std::string filename; FallbackLoader loader; std::string bvh_filename; };
	struct PendingTexture { int handle; std::string filename; };
	static void load_texture(Texture & texture, const std::string & filename);
	void resolve_alpha_masks();
	std::vector<PendingMesh>    pending_meshes;
	std::vector<PendingTexture> pending_textures;
	bool assets_loaded = false;
};

// A light without area: only next-event estimation finds it. intensity: W/sr (point, spot) or irradiance in W/m^2 (directional);
// direction: a spot's axis, or the way a directional light's light travels; cutoff and beam: a spot's angles in radians.
struct DeltaLight {
	enum struct Type { POINT = 0, SPOT = 1, DIRECTIONAL = 2 } type = Type::POINT;
	Vector3 position, direction = Vector3(0.0f, 0.0f, 1.0f), intensity = Vector3(1.0f);
	float cutoff = 0.0f, beam = 0.0f;
};

// The scene-wide fog volume: a homogeneous medium inside an axis-aligned box. Not part of a scene's description (grt_scene_describe).
struct FogVolume {
	Vector3 box_min, box_max = Vector3(1.0f), sigma_a, sigma_s;
	float g = 0.0f;
	// what rt_set_fog_volume will ask too, with its reason (empty: fine)
	std::string complaint() const;
};

// The density grid of the fog volume: nx * ny * nz values >= 0, x fastest, laid over the volume's box. Not part of a scene's description either.
// read_vol / write_vol: Mitsuba 0.6's gridvolume file -- "VOL", version 3, encoding 1 (float32), the dims, 1 channel, the bounding box {min[3], max[3]},
// the data x fastest. A refusal (ParseError) carries the file name.
struct FogDensity {
	std::vector<float> values;
	int nx = 0, ny = 0, nz = 0;
	// what rt_set_fog_density will ask too, with its reason (empty: fine)
	std::string complaint() const;
	static FogDensity read_vol(const std::string & filename, float box[6]);
	void write_vol(const std::string & filename, const float box[6]) const;
};

struct Scene {
	AssetManager asset_manager;
	bool      has_fog = false;   // (after a change of either: Pathtracer::invalidated_fog)
	FogVolume fog;
	bool       has_fog_density = false;   // (state of its own beside the volume; after a change: Pathtracer::invalidated_fog too)
	FogDensity fog_density;
	std::vector<DeltaLight> delta_lights;   // (after a change: Pathtracer::invalidated_delta_lights)

	Camera            camera;
	std::vector<Mesh> meshes;
	Sky               sky;

	bool has_diffuse    = false;
	bool has_plastic    = false;
	bool has_dielectric = false;
	bool has_conductor  = false;
	bool has_lights     = false;

	// Loads everything named in cpu_config.scene_filenames (.xml / .obj) and the sky.
	Scene();

	Mesh & add_mesh(std::string name, Handle<MeshData> mesh_data_handle, Handle<Material> material_handle = Handle<Material>::get_default());

	void check_materials();
	void update(float delta);
};

namespace OBJLoader     { std::vector<Triangle> load(const std::string & filename); }
namespace PLYLoader     { std::vector<Triangle> load(const std::string & filename); }
namespace SerializedLoader { std::vector<Triangle> load(const std::string & filename, int shape_index); }
namespace MitshairLoader   { std::vector<Triangle> load(const std::string & filename, float radius); }
namespace MitsubaLoader { void load(const std::string & filename, Scene & scene); }
namespace TextureLoader {
	// texture->data on entry: load as a data texture (no sRGB decode, no block compression; DDS files are refused)
	bool load(const std::string & filename, Texture * texture);
	// Whether the image file stores an alpha channel, by its header: PNG colour types 4 and 6, 32-bit BMP, TGA with 32-bit pixels or palette entries or
	// 16-bit grey + alpha; JPEG, PNM and DDS never. False for a file that cannot be read.
	bool file_has_alpha(const std::string & filename);
	// One mip step with the box / lanczos / kaiser kernel of the reference (Src/Math/Mipmap.cpp)
	void downsample(MipmapFilterType filter, int w_src, int h_src, int w_dst, int h_dst, const Vector4 * src, Vector4 * dst, std::vector<Vector4> & temp);
}

namespace Geometry {
	std::vector<Triangle> rectangle(const Matrix4 & transform);
	std::vector<Triangle> cube     (const Matrix4 & transform);
	std::vector<Triangle> disk     (const Matrix4 & transform, int num_segments = 32);
	std::vector<Triangle> cylinder (const Matrix4 & transform, const Vector3 & p0, const Vector3 & p1, float radius, int num_segments = 32);
	std::vector<Triangle> sphere   (const Matrix4 & transform, int num_subdivisions = 3);
}
