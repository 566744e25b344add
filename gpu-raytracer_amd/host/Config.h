// Global render settings, same field names as the reference so callers that
// poke `gpu_config.num_bounces` / `cpu_config.bvh_type` keep working
// (reference: Src/Config.h:7-64, Src/CUDA/Common.h:18-67).
#pragma once
#include <string>
#include <vector>

#include "../../include/gpu_raytracer_amd.h"

enum struct ReconstructionFilter : int { BOX = RT_FILTER_BOX, TENT = RT_FILTER_TENT, GAUSSIAN = RT_FILTER_GAUSSIAN };

enum struct AOVType : int {
	RADIANCE = RT_AOV_RADIANCE,
	RADIANCE_DIRECT = RT_AOV_RADIANCE_DIRECT,
	RADIANCE_INDIRECT = RT_AOV_RADIANCE_INDIRECT,
	ALBEDO = RT_AOV_ALBEDO,
	NORMAL = RT_AOV_NORMAL,
	POSITION = RT_AOV_POSITION,
	COUNT = RT_AOV_COUNT
};

// Mirrors the reference GPUConfig field for field; converted to the C-ABI's
// rt_gpu_config by Integrator::update.
struct GPUConfig {
	ReconstructionFilter reconstruction_filter = ReconstructionFilter::GAUSSIAN;
	unsigned aov_mask = 0;

	int num_bounces = 10;

	bool enable_mipmapping                   = true;
	bool enable_next_event_estimation        = true;
	bool enable_multiple_importance_sampling = true;
	bool enable_russian_roulette             = true;
	bool enable_svgf                         = false;
	bool enable_spatial_variance             = true;
	bool enable_taa                          = true;

	float alpha_colour = 0.1f;
	float alpha_moment = 0.1f;
	int   num_atrous_iterations = 6;
	float sigma_z =  4.0f;
	float sigma_n = 16.0f;
	float sigma_l = 10.0f;
};

enum struct BVHType { BVH, SBVH, BVH4, BVH8 };
enum struct IntegratorType { PATHTRACER, AO };
enum struct MipmapFilterType { BOX, LANCZOS, KAISER };

struct CPUConfig {
	int initial_width  = 900;
	int initial_height = 600;

	std::vector<std::string> scene_filenames;
	std::string              sky_filename;

	int         output_sample_index = INVALID_SAMPLE;
	std::string output_filename     = "render.ppm";

	bool enable_scene_update = false;
	// Where the TLAS is built: 0 = on the host (SAH + CWBVH conversion, byte-identical to the reference's), 1 = on the device
	// (rt_build_tlas: one kernel launch, CWBVH only, up to 4096 instances), -1 = on the device when the scene is rebuilt
	// every frame (enable_scene_update) and has at least 1024 instances: there the host build is the CPU work inside the frame loop
	int  device_tlas = -1;
	// Where the bottom-level trees of a CWBVH scene are built: 0 = on the host (SAH / SBVH builder + BVH8Converter, byte-identical
	// to the reference's), 1 = on the device (rt_build_geometry: a linear BVH over all meshes at once; fast to build, dearer to traverse)
	int  device_blas = 0;
	// ... and, for the flattened tree of such a build, early split clipping in front of it: a triangle longer than this fraction of the flattened
	// geometry's longest side is cut into pieces, each piece a reference with its own box (StaticBVHBuilder::presplit, rt_set_build_boxes) -- the
	// Morton-order builder has no spatial splits of its own. 0: off.
	float device_presplit = 0.08f;   // (Sponza, flattened, ms per step of the benchmark: 0 1.72, 0.3 1.67, 0.15 1.61, 0.1 1.56, 0.075 1.55, 0.05 1.62, 0.025 1.62; host tree 1.43: profiles/r05_device_blas_presplit.txt)
	// Static geometry: 1 = every instance that has not been seen moving and whose mesh is not instanced more than twice (two or
	// more such instances) is flattened into ONE bottom-level tree -- a ray then walks one well-built tree (StaticBVHBuilder:
	// SAH object and spatial splits) instead of entering a dozen overlapping per-mesh trees; hits still name the scene's
	// instances and triangles (rt_upload_triangle_aliases), and with nothing left outside the tree rays start inside it
	// (rt_set_static_geometry). CWBVH with the TLAS built on the host only; an instance that starts to move is taken out
	// again (one rebuild). 2 = the same with the per-mesh SAH builder (no spatial splits). 3 = only instances with the
	// identity transform (their copies are their triangles bit for bit; a transformed instance's copies are its triangles
	// taken to world space, which the reference's layout never does: it takes the ray to object space). 0 = one BLAS per
	// mesh under the TLAS, exactly the reference's structure (Integrator.cpp:101-283).
	int  merge_static = 1;
	// The flattening policy, as memory (a copy costs ~176 bytes per triangle: 96 B shading triangle, 48 B traversal positions, the
	// names of the original, its share of the tree's nodes): a mesh that is instanced N times joins only if the N - 1 copies BEYOND
	// the first stay under static_mesh_copy_limit_mb -- copying an instanced mesh per instance is the opposite of what instancing
	// is for (441 instances of a 102 400-triangle mesh: 7.9 GB and a 45 M-triangle tree to build) --, and meshes join in scene order
	// until all copies together reach static_copy_budget_mb. What does not join keeps its TLAS leaf.
	int  static_mesh_copy_limit_mb = 64;
	int  static_copy_budget_mb = 2048;
	// ... and what a triangle test costs relative to a node step when that tree's binary form is collapsed into 8-wide nodes
	// (BVH8Converter: 1 in the reference; here a triangle test runs with a quarter of a wave's lanes, a node step with most)
	float static_primitive_cost = 1.0f;
	// ... and how that collapse deals a node's children to the eight octant slots (BVH8Converter::slot_assignment): 0 = the reference's greedy rule by centres
	// (BVH8Converter.cpp:146-205), 5 = inner children to the slots of least total cost by the corner a ray enters them at, leaves take what is left.
	// The flattened tree is this renderer's own layout: its slot order is free.
	int   static_slot_assignment = 5;
	// ... and then re-seated by what this many sample rays over the flattened geometry say (bvh8_learn_slot_order, SlotOrder.cpp: a seeded, pure function of the
	// geometry). 0: off.
	int   static_slot_learning_rays = 1000000;
	// The seating is trained for the camera as it stood (static_slot_learning_viewpoint): when the camera has travelled further than this fraction of the flattened
	// geometry's diagonal from there, the tree is seated again for the new viewpoint BESIDE the frame loop (a worker thread, 0.3 s for Sponza) and its nodes are
	// swapped in between two frames (rt_update_nodes). 0: never. Trees the DEVICE built (device_blas) get their first seating the same way.
	float static_reseat_distance = 0.1f;
	// Closest-hit rays of a one-tree scene drop stacked groups of children that lie behind the hit they already hold (rt_set_skip_behind_hit): same hits,
	// 12 % fewer node visits on Sponza. false: the reference's walk, node for node.
	bool  skip_behind_hit = true;
	// Sky importance sampling for next-event estimation (rt_set_sky_sampling): 0 = off, the reference's estimator; (0, 1] = the sky's share
	// of the light samples when the scene has emitters (all of them when it has none). Same expectation, less noise under a sky with a sun.
	float sky_sampling = 0.0f;
	// Light tree (rt_set_light_tree): 1 = next-event estimation picks a triangle emitter by a descent of a tree over all of them from the shading
	// point, instead of by power alone. Same expectation, less noise with many lights; off by default. The path tracer switches it after the light tables
	// are uploaded; the AO integrator ignores it.
	int   light_tree = 0;
	// Noise estimate. noise_target: 0 = off; > 0 = the device keeps second moments beside the radiance mean (rt_set_noise_estimate) and the
	// command-line renderer and Pathtracer.render_until stop once the figure -- the noise_quantile quantile of the cells' mean relative standard error -- is at or
	// below it, never before noise_min_samples samples. noise_floor: the floor of the luminance the error is taken relative to.
	float noise_target = 0.0f;
	int   noise_min_samples = 16;
	double noise_quantile = 0.95;
	float noise_floor = 1e-2f;
	// Adaptive sampling (needs noise_target > 0). adaptive_sampling 1: after noise_min_samples uniform samples, every noise check that goes on selects
	// the cells whose mean error is above the target and the next passes render their pixels only. adaptive_dilate 1: the neighbours of such a cell stay active too.
	// adaptive_sampling is read by the command-line renderer's loop alone (--adaptive sets it): Pathtracer::render never selects by itself, Python's render_until
	// takes its own `adaptive` argument, and FrameSplit has no pixel lists (the command line warns and renders uniformly). adaptive_dilate is read by
	// Pathtracer::select_adaptive, whoever calls it.
	int   adaptive_sampling = 0;
	int   adaptive_dilate = 1;
	// Denoised stills. denoise 1: the first Pathtracer::update() switches on the noise estimate and the ALBEDO, NORMAL and POSITION AOVs, which
	// Pathtracer::denoise() filters the accumulated frame by; the command-line renderer (--denoise) then writes the filtered image. The frame itself is rendered
	// as with 0. denoise_iterations: a-trous passes of step 1, 2, 4, ... (0..6); denoise_sigma_l / _n / _z: the edge-stopping weights' luminance, normal and depth terms.
	int   denoise = 0;
	int   denoise_iterations = 5;
	float denoise_sigma_l = 4.0f, denoise_sigma_n = 128.0f, denoise_sigma_z = 1.0f;
	float denoise_depth_floor = 1e-2f, denoise_albedo_floor = 1e-2f;
	// Firefly filter. firefly_filter 1: the first Pathtracer::update() switches on the noise estimate and the tier cascade beside it, which
	// Pathtracer::resolve_fireflies() reweights into an image; the command-line renderer (--firefly-filter) then writes that image. The frame itself is rendered as
	// with 0. firefly_tiers: K, 2..8; firefly_start: b_0 > 0, the luminance tier 0 stands for (tier j: b_0 * 8^j); firefly_support: kappa > 1, the number of
	// neighbouring samples that keep a tier whole.
	int   firefly_filter = 0;
	int   firefly_tiers = 6;
	float firefly_start = 1.0f, firefly_support = 4.0f;
	// A start taken from the frame's own exposure. firefly_auto_start 1: the progression begins with firefly_start, as above; after
	// firefly_pilot_samples uniform samples (>= 2: sample 1 overwrites sample 0) Pathtracer measures the exponent histogram of the mean's luminance
	// (rt_measure_exposure), takes start = 2^(median exponent + firefly_start_shift) (grt_exposure_start) and, where that differs from the start in force, sets
	// it and starts over at sample 0. firefly_start_shift, -16 .. 16: 0, the measured default (tools/fireflies_sweep.py --auto-start), makes the median brightness
	// class the lowest tier's boundary; tiers are a factor 8 apart, so shifts three apart resolve alike while the tiers cover the frame's range.
	int   firefly_auto_start = 0;
	int   firefly_start_shift = 0;
	int   firefly_pilot_samples = 4;
	// The firefly-robust noise estimate (needs firefly_filter = 1, else one warning and the plain estimate). noise_robust 1: Pathtracer::noise and
	// select_adaptive leave out the pixels of which the resolve holds back more than noise_held_fraction (in (0, 1)) of their brightness.
	int   noise_robust = 0;
	float noise_held_fraction = 0.25f;
	// Alpha-tested cut-outs from the albedo textures: 1 = every surface material whose albedo FILE has an alpha channel that is not constant gets an
	// opacity mask from it (channel a, threshold 0.5; an explicit <bsdf type="mask"> wins). Read when a scene is loaded. 0: off, as the reference renders them.
	int   alpha_masks = 0;
	// Delta emitters. delta_lights: 1 = a Mitsuba <emitter type="point"> loads as a true point light (intensity in W/sr); 0 = as the reference's
	// tiny emissive icosahedron. Read when a scene is loaded; spot and directional emitters are delta lights either way. delta_light_share: the probability
	// that a light sample the sky did not take goes to a delta light while the scene has triangle emitters too; 0 = by power (Pathtracer::calc_delta_lights).
	int   delta_lights = 0;
	float delta_light_share = 0.0f;
	// Fog volume: one homogeneous medium inside an axis-aligned box, handed to a scene when it is loaded. fog: off, or the box {min[3], max[3]};
	// fog_sigma_a / fog_sigma_s: absorption and scattering per unit length, RGB; fog_g: Henyey-Greenstein asymmetry. fog_volumes: 1 = a Mitsuba shape
	// with <bsdf type="null"/> and an interior homogeneous medium becomes the fog over its world bounding box and is not added to the scene; 0: loaded as before.
	// With both, the key `fog` wins: its volume replaces the file's, with a warning.
	bool  fog = false;
	float fog_box[6] = { 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f };
	float fog_sigma_a[3] = { 0.0f, 0.0f, 0.0f }, fog_sigma_s[3] = { 0.1f, 0.1f, 0.1f };
	float fog_g = 0.0f;
	int   fog_volumes = 0;
	// Density grid of the fog volume: empty (off), or the path of a Mitsuba gridvolume file (.vol) laid over the volume's box
	std::string fog_density;
	int   static_slot_learning_viewpoint = 1;   // a quarter of those rays are paths from the camera as it stands when the tree is built (0: none are; half come from points of the free space, the rest from the surface, either way)
	// ... and early split clipping (StaticBVHBuilder::presplit, as in front of the device build) in front of that builder's own SAH + spatial splits: fraction of
	// the geometry's longest side above which a triangle is cut blindly first. 0: off.
	float static_presplit = 0.0f;

	IntegratorType integrator = IntegratorType::PATHTRACER; // read by the command-line front end

	MipmapFilterType mipmap_filter = MipmapFilterType::BOX;
	// BC1-quantise power-of-two textures like the reference does by default (BlockCompression.cpp). Off by
	// default here until the textured GPU parity tests have been re-run with it.
	bool enable_block_compression = true;  // the reference's default (Config.h:55): every power-of-two texture is stored as BC1
	// Block-compressed textures are decoded ONCE, when they are uploaded (rt_set_texture_expansion): the device keeps 64 bytes per
	// 4x4 block instead of 8 and the shade kernels fetch texels instead of decoding a block per fetch -- the same texel values.
	// false: the 8-byte blocks stay compressed on the device (an eighth of the memory, a third more shade time).
	bool expand_block_compressed_textures = true;
	// The SVGF filter's a-trous passes stage a workgroup's taps in LDS (rt_set_svgf_tiles); false: every tap is a global load, as in the
	// reference's kernel_svgf_atrous. Bit-identical images either way.
	bool svgf_lds_tiles = true;
	BVHType bvh_type = BVHType::BVH8;

	// "<mesh file>.bvh" caches (BVHCache.h). The reference always reads and writes them; a library
	// that may sit on a read-only asset tree only does so when asked to.
	bool enable_bvh_cache        = false;
	bool bvh_force_rebuild       = false; // ignore existing caches (they are still rewritten)
	bool enable_bvh_optimization = false; // BVHOptimizer::optimize on every binary tree after it is built (-O)
	int  bvh_optimizer_max_time        = 60000; // milliseconds
	int  bvh_optimizer_max_num_batches = 1000;

	float sah_cost_node = 4.0f;   // BVH8 conversion and leaf collapse
	float sah_cost_leaf = 1.0f;
	float sbvh_alpha    = 10e-5f; // 1: never split spatially, 0: always consider it

	static constexpr int INVALID_SAMPLE = -1;
};

extern GPUConfig gpu_config;
extern CPUConfig cpu_config;
