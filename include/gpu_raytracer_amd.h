/*
 * gpu_raytracer_amd.h -- C ABI of the MI355X-native wavefront path tracer device layer.
 *
 * This is the drop-in boundary for the hot path of jan-van-bergen/GPU-Raytracer
 * (ray-generate -> BVH8/CWBVH trace -> sort -> shade/NEE -> shadow trace ->
 * accumulate | SVGF/TAA).  The reference has no FFI: its host class `Integrator`
 * talks to the device code by *name* -- 23 `extern "C" __global__` kernels found
 * with cuModuleGetFunction (Src/Renderer/Integrators/Pathtracer.cpp:79-101) and
 * ~55 `__device__` globals found with cuModuleGetGlobal (`get_global("...")`,
 * Integrator.cpp / Pathtracer.cpp).  Every entry point below replaces one group of
 * those by-name bindings; the comment on each one cites what it replaces.
 *
 * Conventions: plain pointers and sizes only (no C++/torch types); one opaque
 * context per GPU; every function returns RT_OK (0) or a negative rt_status and
 * records a message retrievable with rt_last_error(); host pointers unless the
 * name says `_device`; all work is enqueued on the context's HIP stream and is
 * complete when the call returns only where stated ("synchronous").
 */
#ifndef GPU_RAYTRACER_AMD_H
#define GPU_RAYTRACER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants shared with the reference (Src/CUDA/Common.h) -------------------- */
#define RT_MAX_BOUNCES                  128   /* Common.h:75  MAX_BOUNCES            */
#define RT_BATCH_SIZE                   (1080 * 720) /* Common.h:71 BATCH_SIZE       */
#define RT_PMJ_NUM_SEQUENCES            64    /* Common.h:79                         */
#define RT_PMJ_NUM_SAMPLES_PER_SEQUENCE 4096  /* Common.h:80                         */
#define RT_BLUE_NOISE_NUM_TEXTURES      16    /* Common.h:82                         */
#define RT_BLUE_NOISE_TEXTURE_DIM       128   /* Common.h:83                         */
#define RT_MAX_ATROUS_ITERATIONS        10    /* Common.h:99                         */
#define RT_LUT_DIELECTRIC_DIM           16    /* Common.h:87-89 (ior, roughness, cos)*/
#define RT_LUT_CONDUCTOR_DIM            32    /* Common.h:94-95                      */
#define RT_INVALID                      (-1)

typedef enum rt_status {
	RT_OK                 =  0,
	RT_ERROR_INVALID_ARG  = -1,
	RT_ERROR_NO_DEVICE    = -2,   /* no HIP device / hipSetDevice failed               */
	RT_ERROR_HIP          = -3,   /* a HIP runtime call failed (message has the detail)*/
	RT_ERROR_NOT_READY    = -4,   /* render before the scene/tables were uploaded      */
	RT_ERROR_OUT_OF_RANGE = -5
} rt_status;

/* AOVType, Common.h:28-37 */
typedef enum rt_aov_type {
	RT_AOV_RADIANCE = 0, RT_AOV_RADIANCE_DIRECT, RT_AOV_RADIANCE_INDIRECT,
	RT_AOV_ALBEDO, RT_AOV_NORMAL, RT_AOV_POSITION, RT_AOV_COUNT
} rt_aov_type;

/* ReconstructionFilter, Common.h:21-25 */
typedef enum rt_filter { RT_FILTER_BOX = 0, RT_FILTER_TENT, RT_FILTER_GAUSSIAN } rt_filter;

/* MaterialType, CUDA/Material.h:13-19 (one byte per material on the device) */
typedef enum rt_material_type {
	RT_MATERIAL_LIGHT = 0, RT_MATERIAL_DIFFUSE, RT_MATERIAL_PLASTIC, RT_MATERIAL_DIELECTRIC, RT_MATERIAL_CONDUCTOR
} rt_material_type;

/* GPUConfig, Common.h:39-67 -- replaces the `config` device constant (Integrator.cpp:521). */
typedef struct rt_gpu_config {
	int32_t  reconstruction_filter;            /* rt_filter                               */
	uint32_t aov_mask;                         /* bit i = AOV i enabled                   */
	int32_t  num_bounces;
	int32_t  enable_mipmapping;
	int32_t  enable_next_event_estimation;
	int32_t  enable_multiple_importance_sampling;
	int32_t  enable_russian_roulette;
	int32_t  enable_svgf;
	int32_t  enable_spatial_variance;
	int32_t  enable_taa;
	float    alpha_colour;
	float    alpha_moment;
	int32_t  num_atrous_iterations;
	float    sigma_z;
	float    sigma_n;
	float    sigma_l;
} rt_gpu_config;

/* Camera, CUDA/Camera.h:10-18 -- replaces the `camera` constant (Integrator.cpp:454-481). */
typedef struct rt_camera {
	float position[3];
	float bottom_left_corner[3];
	float x_axis[3];
	float y_axis[3];
	float pixel_spread_angle;
	float aperture_radius;
	float focal_distance;
} rt_camera;

enum { RT_TEXTURE_RGBA8 = 0, RT_TEXTURE_BC1 = 1 };

/* One mip-mapped RGBA8 texture in LINEAR light, i.e. what the reference hands to
 * cuMipmappedArray before optional BC1 compression (Assets/TextureLoader.cpp:145-206).
 * CDNA compute parts have no texture units, so wrap addressing and bi/tri-linear
 * filtering are done in the shade kernel on these texels.                             */
typedef struct rt_texture_desc {
	const uint8_t * texels;      /* all mip levels back to back, level 0 first, 4 B/texel */
	int32_t         width, height; /* level 0 size; level l is max(w>>l,1) x max(h>>l,1)  */
	int32_t         mip_levels;
	/* Size that enters lod_bias = 0.5 * log2(w * h) (Integrator.cpp:95); 0 = width / height. The reference
	 * overwrites Texture::width/height with the BLOCK counts when it BC1-compresses a texture
	 * (TextureLoader.cpp:256-258), so compressed textures carry a bias that is 2 lower.                  */
	int32_t         lod_width, lod_height;
	/* RT_TEXTURE_RGBA8: `texels` as described above. RT_TEXTURE_BC1: `texels` points at the BC1 blocks the reference
	 * hands to its texture unit (TextureLoader.cpp:208-262): 8 bytes per 4x4 texels, ((w+3)/4) x ((h+3)/4) blocks per
	 * level in row-major order, levels back to back; the shade kernels decode a block per texel fetch (D3D rules:
	 * bit-replicated end points, thirds rounded to nearest, 3-colour + transparent mode when c0 <= c1).            */
	int32_t         format;
	int32_t         reserved;
} rt_texture_desc;

/* Per-stage counters of the last rt_render_sample, replaces the read-back of
 * `buffer_sizes` (Pathtracer.cpp:845-847) and the CUDAEventPool timings.              */
typedef struct rt_counters {
	int32_t trace     [RT_MAX_BOUNCES];        /* rays traced per bounce (closest hit)    */
	int32_t shadow    [RT_MAX_BOUNCES];        /* shadow rays traced per bounce           */
	int32_t diffuse   [RT_MAX_BOUNCES];
	int32_t plastic   [RT_MAX_BOUNCES];
	int32_t dielectric[RT_MAX_BOUNCES];
	int32_t conductor [RT_MAX_BOUNCES];
	float   ms_generate, ms_trace, ms_sort, ms_shade, ms_shadow, ms_post; /* HIP-event sums */
	float   ms_total;
} rt_counters;

typedef struct rt_context rt_context;

/* ---- lifetime: replaces CUDAContext::init / Integrator::cuda_init / cuda_free --------
 * (Device/CUDAContext.cpp:21, Pathtracer.cpp:9-41, Integrator.h:203-229)                */
int          rt_create (int device_ordinal, rt_context ** out_ctx);
void         rt_destroy(rt_context * ctx);
const char * rt_last_error(const rt_context * ctx);      /* ctx may be NULL: last global error */
const char * rt_version(void);
/* Layout version of the structs that cross this boundary. Bumped whenever one changes size or meaning, so that a client
 * built against an older header fails its start-up check instead of passing arrays with the wrong stride:
 *   1  round 1
 *   2  rt_texture_desc grew `format`, `lod_width`, `lod_height` (32 -> 40 bytes; rt_upload_textures rejects unknown formats)
 *   3  RT_TIMING_* kinds of rt_get_launch_timings, rt_comm_* / rt_all_gather_* entry points (additions only)
 *   4  rt_upload_triangle_aliases, rt_set_static_geometry (additions only)
 *   5  rt_set_texture_expansion, rt_texture_bytes (additions only; BC1 textures are decoded at upload unless asked otherwise)
 *   6  rt_set_svgf_tiles, rt_set_stream_batch (additions only; 5 and 6 also carried rt_set_node_format / rt_set_node_cache)
 *   7  rt_set_node_format (a 96-byte decoded copy of the node array) and rt_set_node_cache (the top of the flattened tree in LDS) REMOVED:
 *      both measured slower than the 80-byte walk on MI355X (profiles/r04_traversal_experiments.txt items 2 and 4) and were off by default;
 *      rt_set_build_boxes added
 *   8  rt_set_skip_behind_hit, rt_get_skip_behind_hit, rt_geometry_fits_flat_engine, rt_update_nodes (additions only)
 *   9  rt_sample_texture, rt_sample_table, rt_sample_sky (additions only)
 *  10  rt_read_svgf_state and the RT_SVGF_STATE_* images it reads (additions only)
 *  11  rt_set_sky_sampling, rt_get_sky_sampling, rt_sample_sky_distribution, rt_sky_pdf (additions only; sky importance sampling, off by default)
 *  12  rt_bsdf_eval, rt_bsdf_sample (additions only)
 *  13  rt_trace_stream_rays (additions only)
 *  14  rt_upload_material_normal_maps, rt_perturb_normals (additions only; tangent-space normal maps)
 *  15  rt_sample_lights (addition); rt_upload_lights refuses tables on which the light search would not end (see there)
 *  16  rt_sort_rays (addition)
 *  17  rt_upload_material_opacity, rt_read_material_opacity (additions only; alpha-tested opacity masks, off until a mask is uploaded)
 *      (still 17: rt_upload_delta_lights, rt_read_delta_lights, rt_sample_delta_lights -- new entry points and a record of their own, no
 *      existing struct or call changed; point, spot and directional emitters, off until a table is uploaded)
 *      (still 17: rt_set_noise_estimate, rt_get_noise_estimate, rt_read_noise_moments, rt_estimate_noise, rt_accumulate_frames -- new entry points and a
 *      result struct of their own; the per-pixel noise estimate, off by default)
 *      (still 17: rt_select_active_cells, rt_set_pixel_list, rt_get_pixel_list, rt_read_pixel_list, rt_select_pixels_images, rt_accumulate_list_frames
 *      -- new entry points and a result struct of their own; adaptive sampling, off by default)
 *      (still 17: rt_set_fog_volume, rt_get_fog_volume, rt_fog_segments, rt_attenuate_shadow_rays, rt_sort_rays_fog -- new entry points and a
 *      struct of their own; the fog volume, off until one is set)
 *      (still 17: rt_set_fog_density, rt_get_fog_density_info, rt_fog_density_segments -- new entry points; the volume's density grid)
 *      (still 17: rt_read_sky_tables -- a new entry point; the read-back of the sky's sampling tables)
 *      (still 17: rt_denoise, rt_read_denoised, rt_denoise_timed, rt_denoise_images -- new entry points and a parameter struct of their own; the
 *      still-image denoiser, which runs only when called)
 *      (still 17: rt_set_firefly_cascade, rt_get_firefly_cascade, rt_read_firefly_cascade, rt_resolve_fireflies, rt_read_resolved, rt_resolve_fireflies_timed,
 *      rt_set_denoise_source, rt_get_denoise_source, rt_accumulate_cascade_frames, rt_resolve_fireflies_images -- new entry points and a parameter struct of their
 *      own; the firefly filter, off until it is set)
 *      (still 17: rt_trace_queue_rays -- a new entry point; the frame's per-bounce traversal launches on explicit queues, for tests)
 *      (still 17: rt_measure_exposure, rt_measure_exposure_images, rt_estimate_noise_robust, rt_set_noise_robust, rt_get_noise_robust,
 *      rt_estimate_noise_robust_images, rt_select_pixels_robust_images -- new entry points and a result struct of their own; the frame's exposure and the
 *      firefly-robust noise estimate, both off until they are called or set)
 *      (still 17: rt_set_light_tree, rt_get_light_tree, rt_read_light_tree, rt_sample_light_tree, rt_light_tree_pmf -- new entry points; the light tree of
 *      next-event estimation, off until it is set)
 * Check `rt_abi_version() == RT_ABI_VERSION` once after loading the library.                                          */
#define RT_ABI_VERSION 17
int rt_abi_version(void);

/* ---- scene upload ------------------------------------------------------------------- */
/* Replaces globals `triangles` and `bvh8_nodes` (Integrator.cpp:153-154,268-269).
 * triangles: triangle_count x 96 B in the device layout CUDA/Raytracing/Triangle.h:4-11
 * (position_0, edge_1, edge_2, normal_0, n_edge_1, n_edge_2, uv_0, uv_edge_1, uv_edge_2),
 * already permuted by the BLAS indices.  bvh8_nodes: node_count x 80 B CWBVH nodes
 * (BVH/BVH.h:61-80); slots [0, 2*mesh_count) are reserved for the TLAS.                 */
int rt_upload_geometry(rt_context * ctx, const void * triangles, size_t triangle_count,
                       const void * bvh8_nodes, size_t node_count);
/* 1 when a one-tree scene of this size (rt_set_static_geometry(ctx, 1)) is walked by the flattened scene's engine, whose node offsets are a 24-bit multiply and
 * whose triangle offsets are 32 bits wide: fewer than 2^24 nodes and less than 4 GiB of 48-byte triangle records. Larger scenes are walked by the general
 * engine (64-bit addresses), the reference's way. A pure function: no context, no device.                                                             */
int rt_geometry_fits_flat_engine(size_t node_count, size_t triangle_count);
/* Static geometry flattened into ONE bottom-level tree (no counterpart in the reference, which traverses one BLAS per mesh
 * under the TLAS whether the meshes move or not -- Integrator.cpp:101-283,399-430): the caller adds COPIES of the triangles
 * of its static instances to the triangle array, builds (or lets rt_build_geometry build) one more CWBVH over the copies and
 * gives that tree one TLAS leaf. mesh_ids / triangle_ids have one entry per triangle of the uploaded array: mesh_ids[i] < 0
 * for an ordinary triangle; for a copy, a closest hit on it is reported as instance mesh_ids[i] (a row of the
 * rt_upload_instances tables, which may lie behind the rows the TLAS references) and triangle triangle_ids[i] (an ordinary
 * triangle of the array), so that everything behind traversal -- materials, transforms, light tables, the SVGF ids -- sees
 * the instances the scene names. Call after rt_upload_geometry / rt_build_geometry, which forget the aliases; NULL arrays
 * clear them. CWBVH traversal only.                                                                                  */
int rt_upload_triangle_aliases(rt_context * ctx, const int32_t * mesh_ids, const int32_t * triangle_ids);
/* ... and when NOTHING is left outside that tree (no instance moves), the TLAS has nothing to decide: with whole_scene = 1 the
 * caller uploads the ROOT NODE OF THE FLATTENED TREE as the one "TLAS" node (rt_upload_tlas, node slot 0; its child and
 * triangle indices are absolute, so the copy works from there) and row 0 of rt_upload_instances describes the tree (identity
 * transform); every ray then starts INSIDE the tree -- one node step and one instance entry less per ray. whole_scene = 0
 * (the state after every geometry upload): node 0 is a TLAS root, as in the reference (BVH8.h:161-165), and a flattened tree
 * is one of its leaves. Drains the context when the value changes. CWBVH traversal only.                              */
int rt_set_static_geometry(rt_context * ctx, int32_t whole_scene);
/* Replaces nodes [first_node, first_node + node_count) of the uploaded CWBVH node array (80 bytes each) in place, between frames: for a tree whose children were
 * given other octant slots beside the frame loop (the host re-seats the flattened tree when the camera has travelled: Integrator.cpp, reseat worker). The
 * caller keeps node count, boxes, leaves and every index as they were; the context is drained first (a ray's stack entries are only valid within one launch). */
int rt_update_nodes(rt_context * ctx, const void * nodes, size_t first_node, size_t node_count);
/* The walk of closest-hit rays through a one-tree scene (rt_set_static_geometry(ctx, 1)). The reference keeps the children of a node that a ray
 * enters but does not visit at once as ONE stack entry without a distance (BVH8.h:166-199) and therefore still walks into every one of them after a
 * hit in front of them has been found; it makes up for that with 32-lane warps and triangle postponing (BVH8.h:200,234-240). enable = 1 (the
 * default): a stack entry also carries a 16-bit lower bound of the distance at which the ray enters any child left in it (the mask word's unused
 * bits 8..23) and is dropped at its pop when that bound is not in front of the hit held -- a visit that could enter no child. Closest hits are the
 * reference walk's (ties in t between coplanar triangles aside: the walk's order decides those, as it does in the reference); the number of nodes a
 * ray fetches falls (Sponza: 13.1 -> 11.5 per ray). enable = 0: the reference's walk, node for node. Scenes that keep a TLAS always walk the
 * reference's way. Drains the context when the value changes. rt_get_skip_behind_hit: 1 while the walk is in effect (wish AND one-tree scene).  */
int rt_set_skip_behind_hit(rt_context * ctx, int32_t enable);
int rt_get_skip_behind_hit(const rt_context * ctx);
/* Sky importance sampling for next-event estimation (DESIGN.md "Sky importance sampling"). probability 0: off, the default -- the
 * reference's estimator, every frame as before. (0, 1]: light samples also go to the sky, drawn from a distribution over its texels
 * (tables built on the device at the first render after rt_set_sky that wants them); with triangle emitters the sky gets this share
 * of the light samples, without them all. Same expectation, less noise under skies with a sun. Needs NEE on; a black sky leaves it
 * inactive; a sky with NaN / infinite texels makes the render return RT_ERROR_INVALID_ARG. Anything outside {0} u (0, 1], NaN
 * included: RT_ERROR_INVALID_ARG. Takes effect at the next render.                                                                */
int rt_set_sky_sampling(rt_context * ctx, float probability);
int rt_get_sky_sampling(const rt_context * ctx, float * out_probability);
/* Replaces the per-frame TLAS memcpy into the front of `bvh8_nodes` (Integrator.cpp:404-409). The
 * TLAS, the instance tables (rt_upload_instances) and the light tables (rt_upload_lights) are
 * versioned on the device: the call copies the host data into pinned staging and returns (the
 * caller's buffers are free again), the device copy is asynchronous, samples already in flight keep
 * the version they were submitted with and later rt_render_sample calls see the new one. The GPU is
 * only drained when a table outgrows its ring.                                                   */
/* Builds the CWBVH of every mesh ON THE DEVICE instead of uploading host-built nodes (replaces rt_upload_geometry; reference:
 * SAHBuilder.cpp:13-104 + BVH8Converter.cpp:7-335 run per mesh on host threads at load time). `triangles` are the 96-byte
 * device triangles of all meshes back to back in any order, mesh m owning [mesh_first_triangle[m], mesh_first_triangle[m + 1]).
 * The device sorts each mesh's triangles along a Morton curve, builds 8-wide compressed nodes over the sorted order (<= 3
 * triangles per leaf) and stores the triangles in leaf order: out_triangle_positions[i] is where input triangle i went (the
 * caller remaps whatever names triangles by index: light tables), out_root_indices[m] the root node of mesh m (node slots
 * [0, reserved_tlas_nodes) stay free for the TLAS). A linear BVH: built in a fraction of the host build's time, dearer to
 * traverse than the SAH tree; closest hits are the same. rt_read_geometry returns what was built (host views, checker).
 * A mesh may have no triangles (its root is a node without children); an input of no triangles or no meshes is refused with
 * RT_ERROR_INVALID_ARG, like a mesh_first_triangle that decreases or does not run from 0 to triangle_count, and leaves the
 * context's geometry as it was.                                                                                            */
int rt_build_geometry(rt_context * ctx, const void * triangles, size_t triangle_count, const int32_t * mesh_first_triangle, size_t mesh_count,
                      size_t reserved_tlas_nodes, int32_t * out_root_indices, int32_t * out_triangle_positions, size_t * out_node_count, float * out_build_ms);
/* Spatial splits for the build above, decided by the caller (early split clipping): triangles [first_triangle, first_triangle + count) of the NEXT
 * rt_build_geometry are references -- copies of triangles that were cut into pieces, one copy per piece -- and `boxes` (6 floats each: min xyz,
 * max xyz) are the pieces' boxes. The tree is built over those boxes (intersected with the triangle's own), a leaf still tests the whole
 * triangle, so hits do not change; what changes is how many nodes a ray walks past a floor or wall triangle that spans half the scene
 * (the reference gets this from SBVHBuilder.cpp's spatial splits). Consumed by one build; the flattened static geometry uses it
 * (host/Integrator.cpp, cpu_config.device_presplit), whose copies carry the names of their originals (rt_upload_triangle_aliases).        */
int rt_set_build_boxes(rt_context * ctx, const float * boxes, size_t first_triangle, size_t count);
int rt_read_geometry(rt_context * ctx, void * out_triangles, void * out_bvh8_nodes);
int rt_upload_tlas(rt_context * ctx, const void * tlas_nodes, size_t tlas_node_count);
/* Replaces `bvh2_nodes` (Integrator.cpp:205-206): binary SAH BVH, 32 B nodes, for
 * rt_set_bvh_type(ctx, 2) (BASELINE config #1).  TLAS occupies the first slots likewise. */
int rt_upload_geometry_bvh2(rt_context * ctx, const void * triangles, size_t triangle_count,
                            const void * bvh2_nodes, size_t node_count);
int rt_upload_tlas_bvh2(rt_context * ctx, const void * tlas_nodes, size_t tlas_node_count);
/* Replaces `bvh4_nodes` (Integrator.cpp:216-251): 4-wide BVH, 128 B nodes (BVH/BVH.h:25-57), node 1
 * of the TLAS and of every BLAS is the entry point; for rt_set_bvh_type(ctx, 4).            */
int rt_upload_geometry_bvh4(rt_context * ctx, const void * triangles, size_t triangle_count,
                            const void * bvh4_nodes, size_t node_count);
int rt_upload_tlas_bvh4(rt_context * ctx, const void * tlas_nodes, size_t tlas_node_count);
/* Selects the trace kernels (kernel_trace_bvh2 / bvh4 / bvh8 of the reference, Pathtracer.cpp:115-135). */
int rt_set_bvh_type(rt_context * ctx, int bvh_width /* 2, 4 or 8 */);

/* Per-frame TLAS build ON THE DEVICE: replaces, for scenes whose instances move, the host work of Integrator::build_tlas
 * (Integrator.cpp:399-430: SAH build over the instance boxes, CWBVH conversion, re-ordering of the per-instance tables)
 * and rt_upload_tlas + rt_upload_instances. Everything is given in SCENE order (one entry per instance, any order the
 * host likes, the same every frame): root_indices / material_ids / transforms / transforms_inv / transforms_prev as for
 * rt_upload_instances, local_boxes = 6 floats per instance, the object-space min and max of its BLAS. One kernel launch
 * (asynchronous, a new version of the scene ring like the uploads) sorts the instances along a Morton curve, builds the
 * 8-wide compressed TLAS over them in node slots [0, 2 * mesh_count) and gathers the tables into TLAS order. CWBVH
 * kernels only; 1 <= mesh_count <= 4096. With a device-built TLAS rt_upload_lights takes SCENE indices in
 * light_mesh_transform_indices. rt_read_tlas copies the result back (tests, pixel-query translation):
 * order[position] = scene index, the nodes actually used (80 bytes each) and their count; any pointer may be NULL. */
int rt_build_tlas(rt_context * ctx, const int32_t * root_indices, const int32_t * material_ids,
                  const float * transforms, const float * transforms_inv, const float * transforms_prev,
                  const float * local_boxes, size_t mesh_count);
int rt_read_tlas(rt_context * ctx, int32_t * order, void * nodes, size_t node_capacity, int32_t * node_count);
/* The instance tables the kernels read, in TLAS order (tests): mesh_count entries each as rt_upload_instances takes them -- what was
 * uploaded, or what rt_build_tlas gathered -- and position[scene index] = TLAS position, which exists only while the current TLAS
 * is the device's (else RT_ERROR_NOT_READY when asked for). Waits for the work in flight; any pointer may be NULL.
 * (An addition that changes no struct: RT_ABI_VERSION stays.)                                                                     */
int rt_read_instances(rt_context * ctx, int32_t * root_indices, int32_t * material_ids,
                      float * transforms, float * transforms_inv, float * transforms_prev, int32_t * position);
/* Replaces mesh_bvh_root_indices / mesh_material_ids / mesh_transforms{,_inv,_prev}
 * (Integrator.cpp:412-429). Index = TLAS-order mesh id. Matrices are 12 floats, row-major
 * 3x4.  MSB of root_indices[i] = "identity transform" (Integrator.cpp:415).              */
int rt_upload_instances(rt_context * ctx, const int32_t * root_indices, const int32_t * material_ids,
                        const float * transforms, const float * transforms_inv, const float * transforms_prev,
                        size_t mesh_count);
/* Replaces material_types / materials (Pathtracer.cpp:545-589): types = 1 B each,
 * materials = 32 B each in the union layout of CUDA/Material.h:21-39.                    */
int rt_upload_materials(rt_context * ctx, const uint8_t * types, const void * materials, size_t count);
/* Tangent-space normal maps, beside the 32-byte records: texture_ids[i] is the map of material i of the last
 * rt_upload_materials, or -1 (none). count must equal that upload's material count and every id must name an RT_TEXTURE_RGBA8
 * texture of the last rt_upload_textures; otherwise RT_ERROR_INVALID_ARG and the table stays as it was. rt_upload_materials
 * and rt_upload_textures reset the table to none. Only materials of the four surface types use their map.                                       */
int rt_upload_material_normal_maps(rt_context * ctx, const int32_t * texture_ids, size_t count);
/* Alpha-tested opacity masks: binary cut-outs tested inside the CWBVH traversal, for closest-hit and shadow rays alike.
 * texture_ids[i] is the texture whose level 0 masks material i of the last rt_upload_materials, or -1 (none); channels[i] in 0..3
 * (r, g, b, a) and thresholds[i] in (0, 1] say which texels are opaque: those whose byte of that channel is >= ceil(threshold * 255).
 * The bits (one per texel) are built on the device by this call, which drains the context first. RT_ERROR_INVALID_ARG, with the
 * tables left as they were, when count differs from that upload's material count, an id is out of range or names a texture that is
 * not RT_TEXTURE_RGBA8, a channel is outside 0..3 or a threshold is NaN or outside (0, 1]. NULL texture_ids clears the masks;
 * rt_upload_materials and rt_upload_textures reset them to none. A mask on a light material is ignored. A ray / triangle candidate
 * is accepted only where the mask of its instance's material is 1 at the texel that holds (s, t) = uv_0 + u uv_edge_1 + v uv_edge_2,
 * wrapped; shading and light sampling never look at masks. CWBVH kernels only: with rt_set_bvh_type 2 or 4 and a mask uploaded every
 * render / trace entry point returns RT_ERROR_INVALID_ARG before any launch.                                                         */
int rt_upload_material_opacity(rt_context * ctx, const int32_t * texture_ids, const int32_t * channels, const float * thresholds, size_t count);
/* The packed bits of material `material`'s mask: bit y * width + x of the texel (x, y) in word (y * width + x) >> 5, bit & 31, no row
 * padding, unused bits of the last word 0. out_width / out_height (optional) are set whenever the material has a mask.
 * RT_ERROR_INVALID_ARG for a material without a mask or when capacity_words < ceil(width * height / 32).                             */
int rt_read_material_opacity(rt_context * ctx, int material, uint32_t * words, size_t capacity_words, int32_t * out_width, int32_t * out_height);
/* Replaces `media` (Pathtracer.cpp:681-697): 32 B each {sigma_a.xyz, g, sigma_s.xyz, pad}. */
int rt_upload_media(rt_context * ctx, const void * media, size_t count);
/* Replaces `textures` (Integrator.cpp:33-98). */
int rt_upload_textures(rt_context * ctx, const rt_texture_desc * descs, size_t count);
/* Where RT_TEXTURE_BC1 textures are decoded. enable = 1 (the default): once, by rt_upload_textures -- the device keeps 16 RGBA8
 * texels (64 bytes) per block, blocks and mip levels in the order of the compressed chain, and a filtered fetch reads texels.
 * enable = 0: the device keeps the 8-byte blocks and the shade kernels decode a block per texel fetch. The reference hands
 * the blocks to NVIDIA's texture unit (Assets/TextureLoader.cpp:208-262, CUDA/Material.h:60-75), which decodes for free; CDNA
 * compute has no such unit and the per-fetch decode was a third of a shade kernel's instructions, while 8 x the bytes of the
 * compressed chain is nothing next to 288 GB. Both settings produce the same texel values (one decode routine), hence the same
 * images. Takes effect at the next rt_upload_textures. rt_texture_bytes: device bytes the uploaded textures occupy.          */
int rt_set_texture_expansion(rt_context * ctx, int enable);
size_t rt_texture_bytes(rt_context * ctx);
/* Replaces light_* globals and lights_total_weight (Pathtracer.cpp:455-534).
 * The kernels' search of a cumulative table (binary_search) ends inside its span only if the span's last entry is >= the number
 * searched for, so the tables are checked on the host before anything is staged: the mesh table, and every span of the triangle
 * table that a mesh entry names (entries no mesh refers to are not looked at), must hold no NaN, must never decrease and must
 * end in an entry >= 1.0f; every span must satisfy 0 <= first <= last < light_triangle_count; lights_total_weight must be finite
 * and >= 0, and > 0 when there are mesh entries. Otherwise RT_ERROR_INVALID_ARG with a message that names the entry, and the
 * tables uploaded before stay in force. Empty tables (no emitters) are valid.                                                  */
int rt_upload_lights(rt_context * ctx,
                     const int32_t * light_triangle_indices, const float * light_triangle_cumulative_probability, size_t light_triangle_count,
                     const float * light_mesh_cumulative_probability, const int32_t * light_mesh_triangle_span /* 2 per mesh */,
                     const int32_t * light_mesh_transform_indices, size_t light_mesh_count,
                     float lights_total_weight);
/* Delta emitters: point, spot and directional lights, which only next-event estimation can find. One rt_delta_light each:
 * type; position (point, spot); direction (spot: its axis; directional: the direction the light TRAVELS; any non-zero length, normalised on
 * upload); intensity (point, spot: W/sr; directional: irradiance, W/m^2); cutoff and beam (spot, radians: full intensity inside `beam`, none
 * outside `cutoff`, linear in the angle between); weight (>= 0: the light is selected with probability weight / sum of weights).
 * share in (0, 1]: the probability that a light sample the sky did not take goes to a delta light while triangle emitters exist too
 * (q = (1 - sky share) * share); without triangle emitters the delta lights take all of them. Checked on the host before anything is
 * staged: count <= RT_MAX_DELTA_LIGHTS, a known type, finite positions, finite non-zero directions, finite intensities >= 0,
 * 0 < beam <= cutoff <= pi (spot), finite weights >= 0 with a finite sum > 0, share in (0, 1]. Otherwise RT_ERROR_INVALID_ARG with a message
 * that names the light, and the table uploaded before stays in force. records == NULL or count == 0 clears the table: the context then
 * launches exactly the kernels it launched before any upload (the lights are sampled by the ..._split instances of the sort and material kernels, taken only while
 * a table is in force and next-event estimation is on). Drains the context (not a per-frame upload). With next-event estimation
 * disabled the lights contribute nothing.                                                                                      */
#define RT_DELTA_LIGHT_POINT       0
#define RT_DELTA_LIGHT_SPOT        1
#define RT_DELTA_LIGHT_DIRECTIONAL 2
#define RT_MAX_DELTA_LIGHTS        65536
typedef struct rt_delta_light {
	int32_t type;
	float position[3];
	float direction[3];
	float intensity[3];
	float cutoff, beam;
	float weight;
	float reserved[3];
} rt_delta_light; /* 64 bytes */
int rt_upload_delta_lights(rt_context * ctx, const rt_delta_light * records, size_t count, float share);
/* The light tree: position-aware selection of the triangle emitters in next-event estimation. Off by default; while it is off nothing
 * changes: the same kernels are launched and the frames are the same to the bit. enable = 1: a tree over all triangle emitters in world space is built on the
 * device -- one leaf per (light-mesh entry m of rt_upload_lights, triangle j of its span), id leaf_base[m] + j in table order, at most
 * RT_MAX_LIGHT_TREE_LEAVES of them, else RT_ERROR_INVALID_ARG and the state before stays in force -- as soon as geometry, instances, materials and light tables
 * are all there, and again after any rt_upload_lights, rt_upload_instances, rt_build_tlas, rt_upload_materials or geometry upload: those calls mark the tree, and it is
 * rebuilt once before the next render, launch probe or read-back that uses it; a build drains the context. While a
 * tree exists, next-event estimation is on and no fog volume is active, a light sample that goes to the emitters picks its triangle by a descent of the tree
 * from the shading point, and the matching probability enters the MIS weight of an emitter that a BSDF-sampled ray hits (the ..._tree kernel instances).
 * Without triangle emitters nothing is built and the plain kernels run. The AO integrator ignores it.                                                        */
#define RT_MAX_LIGHT_TREE_LEAVES (1 << 22)
int rt_set_light_tree(rt_context * ctx, int enable);
int rt_get_light_tree(rt_context * ctx);
/* The tree as built (waits for the work in flight). *out_leaf_count = N, *out_padded = M = 2^ceil(log2 N) (both 0 while no tree exists; both pointers are
 * required). nodes: 2 M - 1 nodes of 8 floats {box_min[3], Phi, box_max[3], pad} in heap numbering (children of i: 2i + 1, 2i + 2; the leaf at sorted place s:
 * M - 1 + s; padding leaves: Phi 0, an inverted box). leaves: N records of 4 words, by id {light-mesh entry (int32), triangle id (int32), world area A
 * (float), power Phi (float)}. slot_of_leaf: N node indices. entry_of_mesh: per row of the instance tables its light-mesh entry or -1; place_of_triangle: per
 * triangle its place in light_triangle_indices or -1. Any array may be NULL; an array given with less room than it needs is RT_ERROR_INVALID_ARG.           */
int rt_read_light_tree(rt_context * ctx, int32_t * out_leaf_count, int32_t * out_padded, float * nodes, size_t node_capacity,
                       uint32_t * leaves, int32_t * slot_of_leaf, size_t leaf_capacity,
                       int32_t * entry_of_mesh, size_t mesh_capacity, int32_t * place_of_triangle, size_t triangle_capacity);
/* The kernels' selection and its pmf on explicit probes (synchronous; RT_ERROR_INVALID_ARG while no tree exists). rt_sample_light_tree: probes count x 5 floats
 * {u, u2 in [0, 1), p[3] finite}; out count x 4 words {leaf id (int32; -1: the tree holds no power), node (int32), pmf (float), pad}.
 * rt_light_tree_pmf: probes count x 4 words {leaf id (int32), p[3]}; out count floats, the bits rt_sample_light_tree reports when it picks that leaf from p.  */
int rt_sample_light_tree(rt_context * ctx, const float * probes, size_t count, float * out);
int rt_light_tree_pmf(rt_context * ctx, const float * probes, size_t count, float * out);
/* The table as staged for the kernels. records: count x RT_DELTA_LIGHT_RECORD floats {position[3], type (int32 bits), unit direction[3],
 * P_k (the light's selection probability, computed in double from its weight), intensity[3], cos(cutoff), cos(beam), cutoff,
 * 1 / (cutoff - beam) (0 when they are equal), pad}; cdf: count floats, inclusive and normalised, the last entry exactly 1. Either array
 * may be NULL; capacity: lights the arrays have room for (RT_ERROR_INVALID_ARG when fewer than the table holds and an array is given).
 * *out_count: lights in the table; *out_share: the share of the upload (0 without a table).                                       */
#define RT_DELTA_LIGHT_RECORD 16
int rt_read_delta_lights(rt_context * ctx, float * records, float * cdf, size_t capacity, size_t * out_count, float * out_share);
/* Replaces pmj_samples / blue_noise_textures (Integrator.cpp:298-304):
 * pmj = 64*4096 float2, blue_noise = 16*128*128 uchar2.                                   */
int rt_upload_rng(rt_context * ctx, const float * pmj_samples, const uint8_t * blue_noise);
/* Replaces sky_texture / sky_scale (Integrator.cpp:285-296): equirect float4 image.       */
int rt_set_sky(rt_context * ctx, const float * rgba, int width, int height, float scale);

/* ---- per-frame state ------------------------------------------------------------------ */
/* Replaces resize_init/resize_free: screen_width/pitch/height, AOV buffers, SVGF buffers
 * (Pathtracer.cpp:255-301,316-357). pitch = round_up(width, 32).                          */
int rt_resize(rt_context * ctx, int width, int height);
int rt_set_camera(rt_context * ctx, const rt_camera * camera);
/* Replaces `svgf_data` (Pathtracer.cpp:707-717): two row-major 4x4 matrices.              */
int rt_set_svgf_matrices(rt_context * ctx, const float * view_projection, const float * view_projection_prev);
int rt_set_config(rt_context * ctx, const rt_gpu_config * config);
/* How the a-trous passes of the SVGF filter (CUDA/SVGF/SVGF.h:416-554: kernel_svgf_atrous, one thread per pixel, nine taps of three images
 * through the texture cache) fetch their taps. enable = 1 (the default): a workgroup stages the (direct, indirect, normal + depth) values
 * its pixels tap -- rows `step` apart, 64 adjacent columns plus `step` on either side -- in LDS once and taps from there; enable = 0: every
 * tap is a global load, as in the reference. The arithmetic of a pixel is one function for both: images are bit-identical. Passes with a
 * step above 32 (more than six iterations) always use the untiled form.                                                        */
int rt_set_svgf_tiles(rt_context * ctx, int enable);
/* Multi-GPU tile split: this context only renders pixels [offset, offset+count) of the
 * scan-order frame (the reference's kernel_generate(sample, pixel_offset, pixel_count),
 * Pathtracer.cu:122-131). Default = whole frame.                                          */
int rt_set_pixel_range(rt_context * ctx, int pixel_offset, int pixel_count);

/* Interleaved variant for load balance: this context owns tiles first_tile, first_tile +
 * tile_stride, ... of `tile_pixels` consecutive scan-order pixels each (whole rows).
 * rt_set_pixel_range switches back to one contiguous range.                                */
int rt_set_pixel_tiles(rt_context * ctx, int tile_pixels, int first_tile, int tile_stride);
/* Frame exchange for the tile split (both asynchronous on the context's stream, DEVICE pointers):
 * pack   copies this context's `tiles` tiles of the final image into dst (tiles*tile_pixels
 *        float4, zero padded) -- the send buffer of one all-gather over RCCL;
 * unpack scatters the all-gathered buffer [world][tiles_per_rank*tile_pixels] float4 back into
 *        the final image in scan order.                                                       */
int rt_pack_pixels(rt_context * ctx, void * dst_device, int tile_pixels, int first_tile, int tile_stride, int tiles);
int rt_unpack_pixels(rt_context * ctx, const void * src_device, int tile_pixels, int world, int tiles_per_rank);

/* The same exchange WITHOUT a Python / torch.distributed layer: the tile split of a C++ host (host/FrameSplit.h,
 * `pathtracer --devices 0,1,...`). One communicator per context, over RCCL (librccl.so is bound at run time, so the library
 * has no link-time dependency on it):
 *   several processes, one GPU each:  rank 0 calls rt_comm_unique_id and hands the 128 bytes to the others (any side channel:
 *                                     a file, a socket, MPI), every rank calls rt_comm_init_rank (= ncclCommInitRank);
 *   one process, several GPUs:        rt_comm_init_all over its contexts (= ncclCommInitAll). Contexts that SHARE a GPU --
 *                                     which RCCL refuses -- are joined by stream-ordered peer copies instead (tests).
 * A context renders the tiles rt_set_pixel_tiles(ctx, tile_pixels, rank, world) names; rt_all_gather_framebuffer packs them,
 * all-gathers (ncclAllGather on the context's stream) and scatters the result into every context's final image, asynchronously.
 * Contexts of one process are exchanged by ONE call (grouped: ncclGroupStart / End). rt_all_gather_svgf_inputs moves what the
 * SVGF filter stage reads of a frame instead (DIRECT, INDIRECT, ALBEDO, the g-buffers: 80 B per pixel; see rt_pack_svgf_inputs).
 * Environment GRT_COLLECTIVE_LIBRARY names another library with RCCL's entry points (ncclGetUniqueId, ncclCommInitRank, ncclCommInitAll, ncclCommDestroy,
 * ncclAllGather, ncclGroupStart / End, ncclGetErrorString) to bind instead of librccl.so: a site's own build -- or the loopback stand-in of the test suite
 * (tests/support/loopback_ccl.cpp), which lets two PROCESSES that share one GPU run this exchange with world = 2 (tests/test_gpu_rccl.py).               */
int rt_comm_unique_id(void * out_id_128_bytes);
int rt_comm_init_rank(rt_context * ctx, const void * unique_id_128_bytes, int rank, int world);
int rt_comm_init_all(rt_context ** contexts, int count);
int rt_comm_destroy(rt_context * ctx);
int rt_all_gather_framebuffer(rt_context * ctx);
int rt_all_gather_framebuffers(rt_context ** contexts, int count);
int rt_all_gather_svgf_inputs(rt_context ** contexts, int count);
/* Stream-ordered hand-over of device buffers between the context and a consumer's HIP stream
 * (e.g. the stream RCCL runs on), so that the host never has to block between frames:
 *   rt_stream_wait_for_context: `stream` (a hipStream_t) waits for everything the context has
 *       enqueued on its transfer stream so far (rt_pack_pixels, rt_unpack_pixels);
 *   rt_context_wait_for_stream: the context's transfer stream waits for everything enqueued on
 *       `stream` so far (e.g. the collective that still reads the buffer the next pack writes). */
/* SVGF / TAA frames under the tile split (config 3 on N GPUs). The filter stage needs neighbourhoods of +-(3 + 2^5) pixels
 * and reprojects from anywhere in the previous frame, so every rank filters the WHOLE frame, redundantly: a rank path-traces
 * its own tiles (rt_render_sample_unfiltered: like rt_render_sample, stopping before the filter stage), the ranks exchange
 * what the filter reads of this frame -- the per-frame DIRECT / INDIRECT / ALBEDO buffers and the three g-buffers, packed
 * as 5 float4 per pixel by rt_pack_svgf_inputs (same tile arguments as rt_pack_pixels), one all-gather,
 * rt_unpack_svgf_inputs -- and rt_filter_frame runs reproject / variance / a-trous / finalize / TAA on every rank
 * (Pathtracer.cpp:798-838). Bit-identical to one context rendering the whole frame (tests/test_gpu_materials_svgf.py). */
int rt_render_sample_unfiltered(rt_context * ctx, int sample_index);
int rt_pack_svgf_inputs(rt_context * ctx, void * dst_device, int tile_pixels, int first_tile, int tile_stride, int tiles);
int rt_unpack_svgf_inputs(rt_context * ctx, const void * src_device, int tile_pixels, int world, int tiles_per_rank);
int rt_filter_frame(rt_context * ctx, int sample_index);
/* Copies one of the SVGF / TAA filter's persistent images, pitch*height elements, to dst (host). Synchronous: waits for the
 * filter work already enqueued (slot 0 included). `which` is one of RT_SVGF_STATE_*; element types:
 *   HISTORY_LENGTH           int32   frames of history per pixel after the last filtered frame
 *   HISTORY_DIRECT/INDIRECT  float4  what the next frame reprojects from (after the feedback a-trous iteration)
 *   HISTORY_MOMENT           float4  luminance moments (l_d, l_i, l_d^2, l_i^2) the next frame reprojects from
 *   HISTORY_NORMAL_AND_DEPTH float4  the last frame's DECODED normal in .xyz and depth in .w
 *   FRAME_MOMENT             float4  the last frame's temporally integrated moments
 *   TAA_HISTORY              float4  the resolved colour the next frame's TAA reads (tone-mapped)
 *   TAA_CURRENT              float4  the last frame's filtered colour, tone-mapped, as its TAA resolve read it
 * Refused: a NULL context or dst, an unknown `which`, SVGF not allocated. */
#define RT_SVGF_STATE_HISTORY_LENGTH           0
#define RT_SVGF_STATE_HISTORY_DIRECT           1
#define RT_SVGF_STATE_HISTORY_INDIRECT         2
#define RT_SVGF_STATE_HISTORY_MOMENT           3
#define RT_SVGF_STATE_HISTORY_NORMAL_AND_DEPTH 4
#define RT_SVGF_STATE_FRAME_MOMENT             5
#define RT_SVGF_STATE_TAA_HISTORY              6
#define RT_SVGF_STATE_TAA_CURRENT              7
#define RT_SVGF_STATE_COUNT                    8
int rt_read_svgf_state(rt_context * ctx, int which, void * dst);
int rt_stream_wait_for_context(rt_context * ctx, void * stream);
int rt_context_wait_for_stream(rt_context * ctx, void * stream);

/* Pixels per wavefront batch. The reference hard-codes BATCH_SIZE = 1080*720 to bound VRAM
 * (Common.h:69-71) and loops over batches; results do not depend on it. Default 0 = the whole
 * frame in one batch (MI355X has 288 GB of HBM; bigger launches hide traversal latency better). */
int rt_set_batch_size(rt_context * ctx, int batch_size);

/* Samples per pixel rendered concurrently (1..8, default 3). The reference submits the ~40
 * launches of one sample strictly one after the other on one stream (Pathtracer.cpp:738-855);
 * here consecutive rt_render_sample calls alternate between `count` sets of queues / streams and
 * only the accumulate step is ordered between them, so a sample's small deep-bounce launches
 * run in the shadow of its neighbour's. Results are identical for every count (SVGF frames
 * included: only their filter stage is ordered). Profiled / statistics passes run one at a time. Memory: one set of wavefront
 * queues + per-sample frame buffers per sample in flight (~1 GB each at 1920x1080).        */
int rt_set_samples_in_flight(rt_context * ctx, int count);

/* ---- render: replaces Pathtracer::render (Pathtracer.cpp:738-855) ---------------------- */
/* One sample for this context's pixel range: generate, (trace, sort, shade*, shadow) x
 * bounces, then accumulate or SVGF/TAA.  Asynchronous; rt_synchronize or a read waits.    */
int rt_render_sample(rt_context * ctx, int sample_index);
/* sample_count (1..16) consecutive samples per pixel, sample_index .. sample_index+count-1, as
 * ONE wavefront: every launch carries count x as many paths, so the deep bounces (and the small
 * pixel share of one rank of a multi-GPU job) fill the GPU, and the launch-latency floor of a
 * bounce is paid once per batch. Each path is keyed on (pixel, its own sample index) and the
 * per-sample frame buffers are folded into the accumulators in sample order, so the result is
 * bit-identical to count calls of rt_render_sample (tests/test_gpu_parity.py). Not for SVGF.
 * rt_get_counters reports the batch totals.                                               */
int rt_render_samples(rt_context * ctx, int sample_index, int sample_count);

/* How consecutive rt_render_sample(s) calls are scheduled on the device.
 * RT_SCHEDULER_MERGED (default): the calls feed ONE wavefront. Each call ("submission") adds its primary rays to the
 *   wavefront and advances it by one iteration (trace, sort, shade of every submission in flight: the new one is at
 *   bounce 0, the one before at bounce 1, ...), so every launch has the size of a whole sample and a submission is
 *   complete num_bounces - 1 calls later; reads and rt_synchronize run the remaining iterations. Same arithmetic per
 *   path, per-sample frame buffers folded in submission order: images are bit-identical to RT_SCHEDULER_SLOTS.
 *   (The reference runs the chain of one sample at a time, Pathtracer.cpp:738-855: its deep bounces are launches of a
 *   few thousand rays.) SVGF frames go through it as well: every sample slot has its own g-buffer set, a frame is
 *   filtered when it has passed its last bounce, frames in submission order. The binary / 4-wide BVH kernels,
 *   num_bounces = 0, explicit pixel batches and the SVGF tile split always use the slot scheduler.
 * RT_SCHEDULER_SLOTS: one launch chain per submission, up to rt_set_samples_in_flight chains concurrently on their own
 *   streams, each reading the scene version (TLAS, instances, lights) that was current when it was submitted: the
 *   choice for scenes that upload a new TLAS every frame.                                                           */
enum { RT_SCHEDULER_MERGED = 0, RT_SCHEDULER_SLOTS = 1 };
int rt_set_scheduler(rt_context * ctx, int scheduler);
/* Merged scheduler: one more iteration of the wavefront without new samples (no-op when nothing is in flight), and the
 * number of submissions whose accumulate step has been enqueued so far -- a frame loop that hands every completed
 * frame to a collective calls rt_advance / rt_render_samples and packs the frame when the count moves
 * (bench.py); rt_pack_pixels and the reads on their own complete everything first.                       */
int rt_advance(rt_context * ctx);
/* enable = 1: the application keeps several frames in flight.
 *  - rt_pack_pixels / rt_unpack_pixels are ordered after the submissions COMPLETED so far instead of first completing
 *    everything in flight, so that later frames keep filling the wavefront while an earlier one is exchanged;
 *  - small submissions share iterations: a submission generates its primary rays at once, but the iteration that traces
 *    them is only enqueued when 1920 x 1080 x 4 paths are waiting for it (or 8 submissions), so that the launches of one
 *    rank of an N-GPU tile split are as large as those of a whole frame. Whatever needs progress enqueues the iteration
 *    with the submissions that are there: rt_advance, a camera change, every call that completes the work in flight
 *    (reads, uploads, rt_synchronize). rt_submissions_completed only reports.                                          */
int rt_set_frame_pipelining(rt_context * ctx, int enable);
/* How many paths the submissions of ONE iteration may bring (frame pipelining on; default 1920 x 1080 x 4, 0 restores it; at most 8
 * submissions share an iteration whatever the number). An application that knows its burst -- a batch job of N samples that asks for
 * the image only at the end -- gives the burst's paths: its frames then enter the wavefront together and walk their bounces side by
 * side, N_bounces iterations in all, instead of one after the other through N_submissions + N_bounces - 1 iterations of which the
 * first and the last N_bounces - 1 are only partly filled (20 samples at 1080p as five 4-sample submissions: 10 iterations instead
 * of 14, 1.49 -> 1.43 ms per sample). Queues and sample frames grow with the number (412 bytes per path, one frame per sample and
 * bounce in flight). A long-running frame loop keeps the default: its steady state already fills every iteration.                 */
int rt_set_stream_batch(rt_context * ctx, long long paths);
int rt_submissions_completed(rt_context * ctx, uint64_t * out_count);
/* Replaces the `pixel_query` global (Integrator.h:266-277, Integrator.cpp:483-495, Pathtracer.cu:345-348):
 * the mesh (TLAS-order id) and triangle that the primary ray of pixel `pixel_index` = x + y * pitch hits
 * in the next sample rendered (-1 disarms it). rt_get_pixel_query waits and returns -1, -1 for a miss. */
int rt_set_pixel_query(rt_context * ctx, int pixel_index);
int rt_get_pixel_query(rt_context * ctx, int * mesh_id, int * triangle_id);
/* The reference's second integrator, AO::render (Integrators/AO.cpp:148-200, CUDA/AO.cu):
 * primary hit -> one cosine-weighted occlusion ray of length ao_radius -> RADIANCE = 1 where it
 * escapes, NORMAL / POSITION AOVs; needs geometry, instances, RNG tables, rt_resize, rt_set_camera
 * (materials, lights and sky are not used). One sample per call for the context's pixel range. */
int rt_render_ao_sample(rt_context * ctx, int sample_index, float ao_radius);
int rt_synchronize(rt_context * ctx);
/* Per-stage HIP-event timing (ms_generate..ms_post of rt_counters) costs ~2 events per
 * kernel launch, so it is opt-in; ms_total is always measured. Replaces the CUDAEventPool
 * instrumentation of the reference (Pathtracer.cpp:751-843, Device/CUDAEvent.h:31-53).
 * enable = 1: events around every stage; samples are rendered one at a time with the shadow rays
 *             on the main chain, so the stage times are those of each kernel running alone.
 * enable = 2: events around EVERY traversal launch, on the stream each is launched on; concurrency
 *             (merged wavefront, or side stream and samples in flight) stays as in production.
 *             rt_get_counters then returns in ms_trace / ms_shadow the SUM over those launches
 *             since the mode was enabled or counters were last read, rt_get_launch_timings each.
 * enable = 3: as 2, plus events around every OTHER launch of the merged wavefront (generate, sort, one per
 *             material queue, accumulate, each SVGF / TAA kernel): the per-stage rooflines of bench.py. */
int rt_set_profiling(rt_context * ctx, int enable);
/* What a timed launch was (rt_set_profiling 2 / 3). */
enum {
	RT_TIMING_TRACE = 0,        /* closest-hit launches; the fused traversal launch of the merged wavefront */
	RT_TIMING_SHADOW = 1,       /* separate shadow launches (slot scheduler) */
	RT_TIMING_SORT = 2, RT_TIMING_GENERATE = 3, RT_TIMING_ACCUMULATE = 4,
	RT_TIMING_MATERIAL_0 = 5,   /* + material slot: diffuse, plastic, dielectric, conductor */
	RT_TIMING_SVGF_REPROJECT = 9, RT_TIMING_SVGF_VARIANCE = 10, RT_TIMING_SVGF_ATROUS = 11, RT_TIMING_SVGF_FINALIZE = 12,
	RT_TIMING_TAA = 13, RT_TIMING_TAA_FINALIZE = 14,
	RT_TIMING_KINDS = 15
};
/* Durations in milliseconds of the launches of one kind since the mode was enabled (or since the last call for
 * that kind), in submission order; each event pair sits on the stream the launch runs on.                    */
int rt_get_launch_timings(rt_context * ctx, int kind, float * out_ms, int capacity, int * out_count);
/* Work statistics of the trace kernels: when enabled, rt_render_sample runs counting variants
 * of kernel_trace(_shadow)_bvh8 (slower: per-ray atomics) and rt_get_trace_statistics returns,
 * for the last sample, 10 x u64 {closest-hit: BVH8 nodes fetched, triangles tested, transformed
 * instance entries, identity instance entries, rays; then the same five for shadow rays}.
 * These are the N_node / N_tri / N_inst of the algorithmic-bytes roofline.     */
int rt_set_trace_statistics(rt_context * ctx, int enable);
/* Merged scheduler with statistics on: the ten counters after each iteration (cumulative), oldest first; per-launch
 * work = difference of consecutive rows.                                                                  */
int rt_get_trace_statistics_history(rt_context * ctx, uint64_t * out_rows10, int capacity_rows, int * out_rows);
int rt_get_trace_statistics(rt_context * ctx, uint64_t * out10);
/* Counters of the most recent completed rt_render_sample (synchronous).                    */
int rt_get_counters(rt_context * ctx, rt_counters * out);

/* ---- results ----------------------------------------------------------------------------*/
/* Replaces get_aov(type).accumulator read-back (Main.cpp:226-249). Copies pitch*height
 * float4 to dst (host). accumulated=0 reads the per-frame framebuffer instead.             */
int rt_read_aov(rt_context * ctx, int aov_type, float * dst, int accumulated);
/* The final image (`accumulator` surface, Pathtracer.cu:24): pitch*height float4.          */
int rt_read_framebuffer(rt_context * ctx, float * dst);
/* Device pointer of the final image for zero-copy consumers (RCCL gather).                 */
int rt_framebuffer_device_ptr(rt_context * ctx, void ** out_ptr, size_t * out_bytes);
int rt_screen_pitch(rt_context * ctx);

/* ---- noise estimate ------------------------------------------------------*/
/* enable = 1: the accumulate step of every path-traced sample also keeps, per pixel and for RADIANCE only, Welford's second moment beside
 * the running mean: one float4 (M2_r, M2_g, M2_b, w), w the number of samples it stands for. The mean, every accumulator and the final
 * image stay what they are with the estimate off, to the bit. The moments follow AOV.h:35-46's quirk, by which sample 1 overwrites sample
 * 0: samples 0 and 1 leave (0, 0, 0, 1), sample n >= 2 adds d * (fb - mean_new) with d = fb - mean_old and sets w = n. A restart at sample
 * 0 therefore resets a pixel by itself; rt_resize frees the image with the other frame buffers and a CHANGE of the pixel set
 * (rt_set_pixel_range, rt_set_pixel_tiles) zeroes it (w == 0: no sample ever reached the pixel -- another rank's tile is such a pixel).
 * SVGF frames and the AO integrator keep no moments. Off by default; both values drain the context, and the image starts from zeros.    */
int rt_set_noise_estimate(rt_context * ctx, int enable);
int rt_get_noise_estimate(const rt_context * ctx);
/* The moments image: pitch*height float4. RT_ERROR_NOT_READY while the estimate is off. Waits for the work in flight.                   */
int rt_read_noise_moments(rt_context * ctx, float * dst);
/* The estimate over cells of 16 x 16 pixels laid over width x height (edge cells clipped), cells_x = ceil(width / 16), row-major.
 * A pixel takes part when w >= 2 and its mean and M2 are finite; with w >= 2 and anything not finite it is counted as non-finite and
 * left out of the sums. Per pixel, in float32 and in this shape, with luminance(r, g, b) = 0.299 r + 0.587 g + 0.114 b (`luminance` of
 * csrc/rt_shading.h, the Y of the shade and filter kernels):
 *   v = (M2_r + M2_g) + M2_b;   e_p = sqrtf(v / (w * (w - 1.0f))) / fmaxf(luminance(mean), floor)
 * -- the standard error of the mean over its brightness. cell_sums / cell_counts / cell_nonfinite (cell_capacity entries each, at least
 * cells_x * cells_y): per cell the sum of e_p in double over its participating pixels (a fixed reduction tree: the same bits on every
 * run), their number, and the number of non-finite pixels. pixel_map: NULL, or pitch*height floats: e_p, -1 where the pixel takes no
 * part (the padding columns too), -2 where it is non-finite. out->mean: the cell sums added in cell order, in double, over out->pixels.
 * Completes the work in flight. RT_ERROR_NOT_READY while the estimate is off or when no pixel takes part (the cell arrays are filled
 * all the same); RT_ERROR_INVALID_ARG for a floor that is not finite and positive or a capacity that is too small.                      */
typedef struct rt_noise_estimate {
	int32_t cells_x, cells_y;
	int64_t pixels;             /* participating */
	int64_t nonfinite_pixels;
	double  mean;               /* of e_p over the participating pixels */
} rt_noise_estimate;
int rt_estimate_noise(rt_context * ctx, float floor, rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite,
                      size_t cell_capacity, float * pixel_map);

/* ---- adaptive sampling ---------------------------------------------------*/
/* Which cells of the noise estimate still need samples, and their pixels as a list render calls can cover instead of the frame.
 * rt_select_active_cells completes the work in flight, runs the noise kernel on the context's accumulator and moments, then selects:
 * a cell c is HOT when  cell_counts[c] > 0 && cell_sums[c] > (double)threshold * (double)cell_counts[c]  (in double, in this shape), or
 * when  cell_counts[c] + cell_nonfinite[c] <  its in-frame pixel count (it has pixels with w < 2, not sampled enough to judge). A cell
 * whose pixels are all non-finite is not hot. A cell is ACTIVE when it is hot or, with dilate = 1, when one of its up to 8 neighbours
 * inside the cell grid is hot. The list: one uint32 x + y * width per in-frame pixel of the active cells; the cells by ascending index,
 * inside a cell the 8 x 8 patches (0,0), (8,0), (0,8), (8,8), a patch row by row, pixels outside the frame skipped (the list is dense).
 * No atomics decide anything: the same bits on every run. The list stays with the context (pitch*height uint32, allocated at the first
 * selection) until the next selection, rt_resize, rt_set_noise_estimate or a change of the pixel set, each of which also switches
 * rt_set_pixel_list off; a uniform rt_render_samples of sample 0 or 1 -- a progression that starts over -- drops the selection too. cell_flags: NULL, or cell_capacity >= cells_x * cells_y bytes: bit 0 hot, bit 1 active.
 * RT_ERROR_NOT_READY while the estimate is off; RT_ERROR_INVALID_ARG for a floor that is not finite and positive, a threshold that is
 * not finite and >= 0, a dilate outside {0, 1}, a capacity that is too small, under a tile split or a pixel range, and while SVGF is on. */
typedef struct rt_cell_selection {
	int32_t cells_x, cells_y;
	int64_t hot_cells, active_cells;
	int64_t list_pixels;        /* the length of the list */
} rt_cell_selection;
int rt_select_active_cells(rt_context * ctx, float floor, float threshold, int dilate, rt_cell_selection * out, uint8_t * cell_flags, size_t cell_capacity);
/* enable = 1: rt_render_samples covers the selected list instead of the frame. Every pixel folds with its OWN sample count: n = w + 1,
 * w from the moments image, then n + 1 for each further sample of the call; sample_index is the random-number index only, and a pixel's
 * primary ray and random numbers are the ones a uniform call with that sample_index gives it. Refused (RT_ERROR_INVALID_ARG) when no
 * selection exists (under a pixel range other than the whole frame or a tile split none can: setting either drops it, and
 * rt_select_active_cells is refused there), the list is empty, or SVGF is on. While on,
 * rt_render_samples is refused -- never rendered uniformly -- under RT_SCHEDULER_SLOTS or wherever the merged wavefront would not be
 * taken, for sample_index < 2, and so is rt_render_ao_sample. Both values complete the work in flight.                              */
int rt_set_pixel_list(rt_context * ctx, int enable);
int rt_get_pixel_list(const rt_context * ctx);
/* The selected list: *out_count entries (also with dst == NULL); RT_ERROR_INVALID_ARG when capacity is below it, RT_ERROR_NOT_READY
 * without a selection.                                                                                                                */
int rt_read_pixel_list(rt_context * ctx, uint32_t * dst, size_t capacity, size_t * out_count);

/* ---- denoised stills -----------------------------------------------------*/
/* A variance-guided a-trous filter on the accumulated frame, for stills: the RADIANCE mean, its measured variance (the moments of the noise
 * estimate) and the accumulated ALBEDO, NORMAL and POSITION means as guides. Per pixel, all in float32 and in the shapes DESIGN.md 7.9 gives:
 *   valid    w >= 2 and r, g, b / x, y, z of the mean, the moments, albedo, normal and position (and w) finite
 *   surface  valid and |N|^2 >= 0.25                         a = max(A, albedo_floor)          I = C / a
 *   v = luminance(sqrt(var_r), sqrt(var_g), sqrt(var_b))^2,  var_c = M2_c / (w (w - 1)) / a_c^2   (the variance of the mean's luminance for fully correlated channels)
 *   guide (n, z) = (N / |N|, |P - camera position|); the depth gradient g per axis: forward difference of z to a surface neighbour inside the image, else backward, else 0
 * Pass k = 0 .. iterations - 1, step s = 2^k, for every surface pixel p over its surface taps q = p + s (i, j) inside the image, centre weight 1:
 *   w_q = 2^-(|i|+|j|) * exp2(sigma_n * log2(max(0, n_p . n_q)) - (|l_p - l_q| * denom + |z_p - z_q| / (sigma_z * max(|g . (s i, s j)|, depth_floor * z_p) + 1e-8)) * log2(e))
 *   denom = 1 / sqrt(sigma_l^2 * max(0, blur3x3(v)) + 1e-8),   I' = sum(w I) / sum(w),   v' = sum(w^2 v) / sum(w)^2
 * The result, pitch*height float4: (I * a, v) for surface pixels, (C, 0) for valid pixels that are no surface (sky), and for invalid pixels the final
 * image's pixel with .w = -1; invalid pixels are never tapped. The padding columns are not written.
 * rt_denoise completes the work in flight and filters the context's frame (camera position: the last rt_set_camera's) into an image of the context's; its
 * working images (48 B per pixel, and the 16 B of the result) are allocated at the first call and freed by rt_resize. It writes no accumulator, no moments and
 * not the final image: rendering goes on afterwards as if it had not been called. RT_ERROR_NOT_READY, each with its own message, while the noise estimate is
 * off, while ALBEDO, NORMAL or POSITION is not enabled, while SVGF is on, and when no pixel is valid; RT_ERROR_INVALID_ARG for a NULL pointer, iterations
 * outside 0..6, sigmas that are negative or not finite, floors that are not finite and positive. A refused call leaves the previous result in place.
 * rt_read_denoised: the result of the last successful rt_denoise; RT_ERROR_NOT_READY without one (rt_resize drops it).
 * (Additions that change no struct and no call: RT_ABI_VERSION stays.)                                                                              */
typedef struct rt_denoise_params {
	int32_t iterations;          /* 0..6; the host's default: 5 */
	float   sigma_l, sigma_n, sigma_z;   /* the host's defaults: 4, 128, 1 */
	float   depth_floor;         /* the host's default: 1e-2 */
	float   albedo_floor;        /* the host's default: 1e-2 */
} rt_denoise_params;
int rt_denoise(rt_context * ctx, const rt_denoise_params * params);
int rt_read_denoised(rt_context * ctx, float * dst);
/* rt_denoise with a HIP event pair around each of its kernels: kernel_ms[0] prepare, then one entry per pass (or the finalize kernel with 0 iterations);
 * *out_count entries are written, capacity must be at least iterations + 1 (or 2). tiled: as rt_denoise_images. For measurements (tools/denoise_cost.py). */
int rt_denoise_timed(rt_context * ctx, const rt_denoise_params * params, int tiled, float * kernel_ms, size_t capacity, size_t * out_count);

/* ---- firefly filter ------------------------------------------------------*/
/* Tiered accumulation with a reweighted resolve, after Zirr, Hanika and Dachsbacher 2018, "Re-weighting firefly samples". Off until rt_set_firefly_cascade; while
 * it is off a context launches exactly the kernels it launched before these calls existed and allocates nothing for them.
 * While it is on, every RADIANCE sample an accumulate kernel folds into the mean is also splatted into `tiers` (K) images beside the moments image, per pixel
 * S_j = (sum w r, sum w g, sum w b, sum w), tier j standing for the luminance b_j = start * 8^j. All float32, IEEE division, no contraction:
 *   L = luminance(sample.rgb); a sample whose L is not finite is not splatted
 *   lo = start; j = 0; while (L >= lo * 8 && j < K - 1) { lo *= 8; j++; }
 *   j == K - 1 or L <= lo:  S_j += (rgb, 1)
 *   otherwise, hi = lo * 8: wl = clamp((lo / L - lo / hi) / (1 - lo / hi), 0, 1);  S_j += wl * (rgb, 1);  S_j+1 += (1 - wl) * (rgb, 1)
 * so the tiers of a pixel sum to the sum of its samples (nothing is clamped away), sum_j W_j is its sample count, and one splat puts at most b_j of luminance into
 * a tier below the top one. The tiers follow the mean and the moments: a fold with index <= 1 (sample 0 sets the mean, sample 1 overwrites it) zeroes the pixel's
 * tiers before its splat, and whatever zeroes the moments image (rt_set_noise_estimate, a change of the pixel set) zeroes the tiers; rt_resize gives them the new
 * size, zeroed. Mean, moments and final image are the same bits with the cascade on and off. SVGF frames and the AO integrator never splat.
 * rt_set_firefly_cascade: params NULL switches it off and frees the tiers. Completes the work in flight; the tiers are allocated and zeroed on switching on and
 * on every change of `tiers` or `start` (the samples folded before are not in them: restart the progression). tiers * 16 B per pixel of the pitched frame: about
 * 200 MB at 1920 x 1080 with 6 tiers. RT_ERROR_NOT_READY while the noise estimate is off (switching the estimate off switches the cascade off as NULL does: tiers and resolved image are freed);
 * RT_ERROR_INVALID_ARG for tiers outside 2..8, start not finite and positive, support not finite and above 1. A refused call leaves the previous state in force.
 * rt_get_firefly_cascade: 1 and *out (may be NULL) while it is on, else 0. rt_read_firefly_cascade: the tiers, `tiers` images of pitch*height float4 one behind
 * the other (capacity: floats), after the work in flight.
 *
 * rt_resolve_fireflies, on the whole frame, float32, sums in the stated order:
 *   valid(q)  w(q) >= 1 (the moments image), the mean's r, g, b finite, all tiers finite
 *   for a valid p, N = w(p):  A_j = sum of W_j(q) over the valid q of the 3 x 3 neighbourhood inside the image, in row order
 *     n_j = (A_j-1 + A_j) + A_j+1, A_-1 = A_K = 0;   R = S_0.rgb (r_0 = 1);   for j = 1 .. K - 1 in order, b_j = start * 8^j:
 *     rc = clamp((n_j - 1) / (support - 1), 0, 1);  rcol = min(1, luminance(R) / b_j);  r_j = max(rc, rcol);  R += r_j * S_j.rgb
 *   out(p) = (R / N, luminance(T - R) / N), T = sum_j S_j.rgb in tier order: .w is the luminance that was held back
 *   an invalid p gets the final image's pixel with .w = -1, and is never counted in a neighbourhood
 * The estimator is consistent, not unbiased: for a tier of positive probability n_j grows with N, so r_j -> 1.
 * It completes the work in flight and writes one result image of the context's (allocated at the first call, freed by rt_resize): no accumulator, no moments, no
 * tiers and not the final image; rendering goes on afterwards as if it had not been called. support: the kappa above (> 1, finite; the host's default 4).
 * RT_ERROR_NOT_READY, each with its own message, while the cascade is off, while SVGF is on, and when no pixel is valid.
 * rt_read_resolved: the last successful resolve, pitch*height float4; RT_ERROR_NOT_READY without one.
 * rt_resolve_fireflies_timed: the resolve with a HIP event pair around its kernel, *kernel_ms its time; tiled as rt_resolve_fireflies_images.
 * rt_set_denoise_source: RT_DENOISE_SOURCE_RESOLVED makes rt_denoise take its colour image from the last resolve instead of the RADIANCE mean (the moments stay the
 * measured ones: a firefly's pixel carries a large variance and accepts its neighbours); rt_denoise then answers RT_ERROR_NOT_READY when there is no resolve or
 * the frame has been folded into or zeroed since. No denoise kernel differs.
 * (Additions that change no struct and no call: RT_ABI_VERSION stays.)                                                                              */
typedef struct rt_firefly_params {
	int32_t tiers;     /* 2..8; the host's default: 6 */
	float   start;     /* b_0 > 0; the host's default: 1 */
	float   support;   /* kappa > 1, what rt_resolve_fireflies_images and the host take as default; the host's default: 4 */
} rt_firefly_params;
enum { RT_DENOISE_SOURCE_MEAN = 0, RT_DENOISE_SOURCE_RESOLVED = 1 };
int rt_set_firefly_cascade(rt_context * ctx, const rt_firefly_params * params);
int rt_get_firefly_cascade(const rt_context * ctx, rt_firefly_params * out);
int rt_read_firefly_cascade(rt_context * ctx, float * dst, size_t capacity);
int rt_resolve_fireflies(rt_context * ctx, float support);
int rt_read_resolved(rt_context * ctx, float * dst);
int rt_resolve_fireflies_timed(rt_context * ctx, float support, int tiled, float * kernel_ms);
int rt_set_denoise_source(rt_context * ctx, int source);
int rt_get_denoise_source(const rt_context * ctx);

/* The frame's exposure: which power of two its pixels are bright as, for a cascade start relative to the frame (grt_exposure_start of the
 * host library turns the histogram into one). Over the width x height pixels of the RADIANCE mean and the moments image, the padding columns never read:
 * a pixel with w < 1 (or a w that is NaN) takes no part; with w >= 1 and r, g, b or luminance(mean) not finite it counts in nonfinite_pixels; Y =
 * luminance(mean), float32 in the shape of rt_estimate_noise; Y <= 0 counts in dark_pixels; else histogram256[(bits(Y) >> 23) & 255] gets one count -- the
 * biased exponent, denormals in bin 0. pixels: the total of the 256 bins. Integer counts: the same on every run.
 * rt_measure_exposure completes the work in flight and writes nothing a render reads; RT_ERROR_NOT_READY while the noise estimate is off (no w), while SVGF is on
 * (its frames keep no moments) and before rt_resize. (Additions that change no struct and no call: RT_ABI_VERSION stays.)                              */
typedef struct rt_exposure { int64_t pixels, dark_pixels, nonfinite_pixels; } rt_exposure;
int rt_measure_exposure(rt_context * ctx, rt_exposure * out, uint64_t * histogram256);

/* The firefly-robust noise estimate: rt_estimate_noise that follows the resolve's judgement. held_fraction tau in (0, 1) (the host's default
 * 0.25: a quarter of the pixel's light is unsupported) is part of the definition, as floor is. A pixel that takes part by rt_estimate_noise's rule is HELD when
 * the resolve found it valid (resolved.w >= 0) and, in float32,  resolved.w > tau * fmaxf(luminance(mean), floor).  A held pixel is left out of its cell's sum
 * and count, counted in cell_held, and -3 in the map; everything else is rt_estimate_noise to the letter, and a cell without a held pixel has its bits.
 * *out_held_pixels (may be NULL): the total of cell_held.
 * rt_estimate_noise_robust completes the work in flight, runs rt_resolve_fireflies with the cascade's support -- a resolve like any other: rt_read_resolved returns
 * it, rt_set_denoise_source takes it as fresh -- and then the robust cells kernel. Errors as rt_estimate_noise, and RT_ERROR_NOT_READY while the cascade is off or
 * when the resolve finds no valid pixel, RT_ERROR_INVALID_ARG for a tau outside (0, 1).
 * rt_set_noise_robust: while held_fraction is in (0, 1), rt_select_active_cells selects from the robust cells (resolve included), with a second clause that
 * counts held pixels as judged:  cell_counts[c] + cell_nonfinite[c] + cell_held[c] < its in-frame pixel count;  out and cell_flags keep their meaning. 0 switches
 * it off. Refused (RT_ERROR_NOT_READY) while the cascade is off; switching the cascade off switches it off; rt_resize keeps it as it keeps the cascade.
 * rt_estimate_noise itself never changes. (Additions that change no struct and no call: RT_ABI_VERSION stays.)                                          */
int rt_estimate_noise_robust(rt_context * ctx, float floor, float held_fraction, rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts,
                             int32_t * cell_nonfinite, int32_t * cell_held, size_t cell_capacity, float * pixel_map, int64_t * out_held_pixels);
int rt_set_noise_robust(rt_context * ctx, float held_fraction);   /* 0: off */
float rt_get_noise_robust(const rt_context * ctx);

/* Kulla-Conty LUTs as computed on the device at first use (kernel_integrate_* /
 * kernel_average_*, CUDA/KullaConty.h:83-240): 16^3, 16^3, 16^2, 16^2, 32^2, 32 floats.
 * Any pointer may be NULL. Synchronous.                                                     */
int rt_read_luts(rt_context * ctx, float * dielectric_directional_enter, float * dielectric_directional_leave,
                 float * dielectric_enter, float * dielectric_leave, float * conductor_directional, float * conductor);
/* The tables of sky importance sampling as the device built them for the last rt_set_sky (kernels_sky.hip; built here if nothing has
 * wanted them yet, which leaves the context as a render with sampling on leaves it). *out_width, *out_height: the sky's size (W, H);
 * marginal_cdf: H floats; conditional_cdf and cell_pdf: H x W floats, x fastest; row_totals: H doubles (the rows' weights before
 * normalisation); *out_total: their sum. Any pointer may be NULL. capacity: the room of every array given, in cells; below W x H with an
 * array given: RT_ERROR_INVALID_ARG (the sizes are still written, so a first call with no array asks for them). RT_ERROR_INVALID_ARG
 * also without a sky and for a sky with NaN or infinite texels. Synchronous. (An addition that changes no struct: RT_ABI_VERSION stays.) */
int rt_read_sky_tables(rt_context * ctx, int * out_width, int * out_height, float * marginal_cdf, float * conditional_cdf, float * cell_pdf,
                       double * row_totals, double * out_total, size_t capacity);

/* ---- kernel-level entry points (parity tests and micro-benchmarks) ----------------------*/
/* kernel_trace_bvh8 / kernel_trace_shadow_bvh8 on caller-supplied rays (SoA host arrays).
 * hits: ray_count x uint4 {mesh_id, triangle_id, t bits, u16|v16<<16} (Buffers.h:25-32).
 * Synchronous. `repeat` > 1 re-runs the kernel for timing; out_ms = mean kernel ms.        */
int rt_trace_rays(rt_context * ctx, const float * ox, const float * oy, const float * oz,
                  const float * dx, const float * dy, const float * dz, size_t ray_count,
                  uint32_t * hits, int repeat, float * out_ms);
int rt_trace_shadow_rays(rt_context * ctx, const float * ox, const float * oy, const float * oz,
                         const float * dx, const float * dy, const float * dz, const float * max_distance,
                         size_t ray_count, uint8_t * occluded, int repeat, float * out_ms);
/* The merged wavefront's traversal launch (the frame's own kernel and engine choice) on explicit rays (synchronous; CWBVH only).
 * `iteration`: its parity picks the queue and cursor halves. closest_count rays (ox..dz) write hits (uint32[4] each as
 * rt_trace_rays; the array is uploaded first, so a value the launch never overwrites stays). shadow_count rays (sox..sdz,
 * max_distance) each carry illumination (1, 0, 0) for pixel i: shadow_light[i] is what the launch added, 0 occluded, 1 not
 * (2 or more: the ray was dealt twice). stats10: NULL for the frame's kernel, else the counting kernel runs and its 10 counters
 * ({nodes, triangles, transformed, identity instance entries, rays} x {closest, shadow}) are returned. info: 4 ints {kernel (0 general,
 * 1 flat, 2 flat skipping, 3 counting; with opacity masks uploaded 4 general, 5 flat, 6 flat skipping, 7 counting: their _mask instances), waves of its persistent grid, RT_NARROW_MAX_RAYS, RT_MIXED_MAX_RAYS}. Leaves no state a frame reads. */
int rt_trace_stream_rays(rt_context * ctx, int iteration,
                         const float * ox, const float * oy, const float * oz, const float * dx, const float * dy, const float * dz,
                         size_t closest_count, uint32_t * hits,
                         const float * sox, const float * soy, const float * soz, const float * sdx, const float * sdy, const float * sdz,
                         const float * max_distance, size_t shadow_count, float * shadow_light,
                         uint64_t * stats10, int32_t * info);
/* The frame's traversal launches on explicit queues whose shadow rays carry the caller's illumination and pixel words into the caller's frames
 * (synchronous). merged 0, step = bounce in [0, RT_MAX_BOUNCES): what the slots scheduler launches for one bounce -- the closest-hit launch, then the
 * shadow launch on the slot's second spill area -- by the launchers a frame calls, so the BVH width (2, 4, 8) and the opacity-mask instances are the
 * context's. form RT_TRACE_QUEUE_PLAIN: the frame's kernels; RT_TRACE_QUEUE_COUNTING: the counting kernels (CWBVH only), their ten counters in stats10
 * as rt_trace_stream_rays returns them (stats10 is NULL for every other form); RT_TRACE_QUEUE_AO: the AO integrator's shadow launch alone (step 0, no
 * closest-hit rays). merged 1, step = iteration: the merged wavefront's one launch, as rt_trace_stream_rays runs it (CWBVH only; form PLAIN or COUNTING).
 * closest_count rays (ox..dz) write hits as there (uploaded first: a value the launch never overwrites stays). shadow_count rays (sox..sdz,
 * max_distance) carry illumination[3 * i .. 3 * i + 2] for the pixel pixel_words[i]; in the merged form bit RT_TRACE_QUEUE_FLAG_BOUNCE_0 of the word
 * marks a ray of bounce 0 (refused in the per-bounce form, where the bounce is `step`). radiance, radiance_direct, radiance_indirect: frame_pixels x 4
 * floats each, uploaded first and read back whole; NULL: the launch has no such frame. An unoccluded shadow ray adds (illumination, 0) to RADIANCE,
 * and sets RADIANCE_DIRECT to it (bounce 0) or adds it to RADIANCE_INDIRECT (later bounces); the AO form sets RADIANCE to (1, 1, 1, 1). Refused
 * before any launch: a pixel at or beyond frame_pixels, two shadow rays that name the same pixel (the contribution is a plain read-modify-write), more
 * than 2^28 rays or pixels. info: RT_TRACE_QUEUE_INFO ints {BVH width, waves of the closest-hit launch's persistent grid, waves of the shadow launch's
 * (merged: the one launch's, twice), RT_NARROW_MAX_RAYS, RT_FETCH_BLOCK_MAX (-1 merged), the merged launch's kernel as rt_trace_stream_rays numbers
 * them (-1 per-bounce)}. Leaves no state a frame reads. (An addition that changes no struct: RT_ABI_VERSION stays.) */
#define RT_TRACE_QUEUE_PLAIN    0
#define RT_TRACE_QUEUE_COUNTING 1
#define RT_TRACE_QUEUE_AO       2
#define RT_TRACE_QUEUE_INFO     6
#define RT_TRACE_QUEUE_FLAG_BOUNCE_0 (1u << 30)
int rt_trace_queue_rays(rt_context * ctx, int merged, int step, int form,
                        const float * ox, const float * oy, const float * oz, const float * dx, const float * dy, const float * dz,
                        size_t closest_count, uint32_t * hits,
                        const float * sox, const float * soy, const float * soz, const float * sdx, const float * sdy, const float * sdz,
                        const float * max_distance, const float * illumination, const uint32_t * pixel_words, size_t shadow_count,
                        float * radiance, float * radiance_direct, float * radiance_indirect, size_t frame_pixels,
                        uint64_t * stats10, int32_t * info);
/* kernel_generate only: writes the primary rays of pixels [offset, offset+count).          */
int rt_generate_rays(rt_context * ctx, int sample_index, int pixel_offset, int pixel_count,
                     float * ox, float * oy, float * oz, float * dx, float * dy, float * dz,
                     uint32_t * pixel_index_and_flags);
/* One of the three generate launches on a caller-given submission (synchronous). kernel: 0 kernel_generate (per-bounce schedulers), 1
 * kernel_generate_stream, 2 kernel_generate_stream_list (merged wavefront), each through the launcher the schedulers call. Camera, filter, SVGF flag
 * and RNG tables are the context's; the submission is the call's: samples first_sample .. first_sample + sample_count - 1 (1..16: batch_samples) of
 * local pixels [pixel_offset, pixel_offset + pixel_count), which tile_pixels / tile_first / tile_stride map to the frame as rt_set_tile_split does
 * (tile_pixels 0: no tiles), or -- kernel 2 -- of the pixel_count entries (x + y * width) of pixel_list. Kernels 1 and 2: sample s goes to sample
 * slot slot_base + s, `iteration`'s parity picks the queue half, the queue holds queue_before entries already (the control block's count word) and the
 * rays land behind queue_before + queue_offset. Kernel 0 takes 0 for these three. block_width / band_rows (kernel 1): the queue order, both 0 for scan
 * lines, both -1 for what the scheduler chooses for such a submission. The seven queue arrays hold `capacity` entries each: they are uploaded first
 * and read back whole, so a value the launch never overwrites stays. info: 4 ints {block_width, band_rows as launched, workgroups of the grid, the
 * count word after the launch: RtBufferSizes::trace[0] for kernel 0, else trace_count[iteration & 1], which the stream kernels leave alone}.
 * Refused: NULL arrays, counts below zero, sample_count outside [1, 16], slot_base + sample_count > 512, (slot_base + sample_count) * frame_pixels
 * >= 2^30, capacity < queue_before + queue_offset + pixel_count * sample_count, a pixel beyond width * height; RT_ERROR_NOT_READY without RNG tables
 * or rt_resize. Leaves no state a frame reads. (An addition that changes no struct: RT_ABI_VERSION stays.)                                          */
int rt_generate_primary_rays(rt_context * ctx, int kernel, int iteration, int first_sample, int sample_count, int pixel_offset, int pixel_count,
                             int tile_pixels, int tile_first, int tile_stride, int slot_base, int queue_before, int queue_offset,
                             int block_width, int band_rows, const uint32_t * pixel_list, size_t capacity,
                             float * ox, float * oy, float * oz, float * dx, float * dy, float * dz, uint32_t * pixel_index_and_flags, int32_t * info);
/* random<Dim>() (CUDA/Sampling.h:44-84) for `count` (pixel_index) values: out = float2 each. */
int rt_random_samples(rt_context * ctx, int dimension, const uint32_t * pixel_indices, size_t count,
                      uint32_t bounce, uint32_t sample_index, float * out_xy);
/* The software texture unit (rt_shading.h) on explicit coordinates; synchronous.
 * rt_sample_texture: texture `texture_index` of the last rt_upload_textures. filter 0 = texture_get (level 0),
 * 1 = texture_get_lod, 2 = texture_get_grad. args: count x 8 floats {s, t, lod, dx.x, dx.y, dy.x, dy.y, pad}
 * (filter 0 reads s, t; 1 also lod; 2 the gradients, not lod). out_rgba: count x 4 floats.
 * rt_sample_table: lut_get_1d / _2d / _3d (dims 1, 2, 3) on a caller-supplied nx [x ny [x nz]] float table,
 * x fastest. coords: count x 3 floats {s, t, r}, the unused ones ignored. out: count floats.
 * rt_sample_sky: sample_sky on what rt_set_sky uploaded. directions: count x 3 floats (unit length); out_rgb: count x 3. */
int rt_sample_texture(rt_context * ctx, int texture_index, int filter, const float * args, size_t count, float * out_rgba);
int rt_sample_table(rt_context * ctx, const float * table, int nx, int ny, int nz, int dims, const float * coords, size_t count, float * out);
int rt_sample_sky(rt_context * ctx, const float * directions, size_t count, float * out_rgb);
/* Sky importance sampling on explicit arguments (builds the tables if needed; synchronous).
 * rt_sample_sky_distribution: uv: count x 2 floats in [0, 1) (u picks the column, v the row); out_xyz_pdf: count x 4 floats
 * {direction, pdf in solid angle}. RT_ERROR_INVALID_ARG for a sky without weight.
 * rt_sky_pdf: the pdf (solid angle) the distribution gives each of `count` unit directions (count x 3 floats); out_pdf: count. */
int rt_sample_sky_distribution(rt_context * ctx, const float * uv, size_t count, float * out_xyz_pdf);
int rt_sky_pdf(rt_context * ctx, const float * directions, size_t count, float * out_pdf);
/* One BSDF of the shade kernels on explicit probes (synchronous): set up as a material kernel sets up a hit (tangent frame of the normal,
 * omega_i, the path's random numbers, init, albedo on a throughput of 1), then its own eval (rt_bsdf_eval) or sample (rt_bsdf_sample).
 * material_type: RT_MATERIAL_DIFFUSE .. RT_MATERIAL_CONDUCTOR; the Kulla-Conty tables are the context's (integrated if need be).
 * probes: count x 24 floats {material (the 32-byte record of rt_upload_materials; texture id RT_INVALID only), shading normal[3]
 * (flipped to the side the ray arrives from), ray direction[3], entering_material (0 / 1), to_light[3], cos_theta_o (eval only),
 * pixel index, sample index, bounce (uint32 bits; sample only), pad[2]}.
 * out: count x 12 floats {ok (1 / 0; -1: refused, omega_i.z <= 0, as the shade kernels refuse it), pdf, bsdf (eval) or throughput
 * factor (sample)[3], direction (to_light, or the sampled one)[3], medium id, allow_nee, omega_i.z, pad}. Writes no frame buffer. */
int rt_bsdf_eval(rt_context * ctx, int material_type, const float * probes, size_t count, float * out);
int rt_bsdf_sample(rt_context * ctx, int material_type, const float * probes, size_t count, float * out);
/* The shade kernels' light selection on explicit random numbers (synchronous): nee_pick_light -- sample_light's two table searches,
 * sample_triangle, the point, normal and emission of the emitter -- on the light tables, triangles, transforms and materials the context
 * holds. probes: count x 4 floats {u_mesh, u_triangle, u_1, u_2}, each in [0, 1). use_lds = 1: the tables are chosen as the shade
 * kernels choose them (a workgroup copies them into LDS when there are at most 64 mesh entries and 2048 triangle entries, else global
 * memory); 0: global memory. out: count x RT_LIGHT_SAMPLE_OUT floats {light-mesh entry, transform id (row of the instance tables, after
 * the device-built TLAS's remapping), triangle index, 1 if the searches read LDS else 0 (these four int32 bits), point[3], geometric
 * normal[3], emission[3], pad[3]}. RT_ERROR_NOT_READY without emitters. Writes no frame buffer.                                      */
#define RT_LIGHT_SAMPLE_OUT 16
int rt_sample_lights(rt_context * ctx, const float * probes, size_t count, int use_lds, float * out);
/* The shade kernels' delta-light sample on explicit probes (synchronous): nee_pick_delta -- the search of the table's CDF -- and
 * delta_light_sample -- direction, distance, radiance term -- on the table of rt_upload_delta_lights. probes: count x 4 floats
 * {u in [0, 1), origin[3] (finite; the shadow ray's origin, taken as it is)}. out: count x RT_DELTA_SAMPLE_OUT floats {light index (int32
 * bits), to_light[3] (unit), max_distance (RT_INFINITY for a directional light), radiance term[3] (intensity x falloff / d^2, or the
 * irradiance), pdf (P_k of the light's record: the probability of this light among the delta lights), ok (1 / 0: 0 when the distance is 0
 * or not finite, the falloff is 0, the radiance term is not finite or P_k is 0), pad[2]}. RT_ERROR_NOT_READY without a table. Writes no
 * frame buffer.                                                                                                                  */
#define RT_DELTA_SAMPLE_OUT 12
int rt_sample_delta_lights(rt_context * ctx, const float * probes, size_t count, float * out);
/* The shade kernels' normal-map perturbation (normal_map_perturb, rt_shading.h) on explicit hits (synchronous), with texture
 * `texture_index` (RT_TEXTURE_RGBA8) of the last rt_upload_textures as the map. probes: count x RT_NORMAL_PROBE_IN floats
 * {p0[3], e1[3], e2[3] (object-space triangle: vertex 0 and the two edges), n0[3], ne1[3], ne2[3] (vertex normal 0 and its
 * edges), uv0[2], uve1[2], uve2[2], u, v (barycentrics), world[12] (3x4 row-major: rotation and uniform scale), ray direction[3],
 * filter (0: level 0, 1: lod, 2: gradients), lod (filter 1; the texture's lod bias is added as in the shade kernels),
 * gradient_1[2], gradient_2[2] (filter 2), pad}. out: count x 4 floats {world shading normal[3] (on the side the ray arrives
 * from, after the view guard), 1 if the hit fell back to the interpolated normal else 0}.                                 */
#define RT_NORMAL_PROBE_IN 48
int rt_perturb_normals(rt_context * ctx, int texture_index, const float * probes, size_t count, float * out);
/* The sort launch on an explicit trace queue (synchronous): the production launcher -- the per-bounce one (merged = 0: `step` is the
 * bounce, sample_index the launch's) or the merged wavefront's (merged = 1: `step` is the iteration; bounce and sample of an entry come
 * out of slot_table / submission_birth) -- so the instance (plain or _sky) and the grid are the shipped ones, on the context's own
 * parameter block with the queues, the counters / control block, the slot table, the four AOV frames the launch touches, the g-buffers
 * and the pixel-query word replaced by buffers of this call. Nothing of the context changes but what a render would settle (the sky
 * tables when sky sampling is wanted).
 * Records are 32-bit words. trace_in: count x RT_SORT_TRACE_WORDS {origin[3], direction[3], hit[4] (as rt_trace_rays), pixel_index_and_flags,
 * throughput[3], last_pdf, medium, cone_angle, cone_width, pad[2]}. The pixel is a VIRTUAL pixel v = slot * frame_pixels + pixel
 * (frame_pixels = rt_screen_pitch x height) with slot < frame_slots <= 512; the frames below hold frame_slots * frame_pixels pixels.
 * slot_table (merged): slot_count x 4 ints {sample_index, birth_iteration, submission, index_in_submission}; submission_birth: 128 ints.
 * trace_out: capacity x RT_SORT_TRACE_WORDS (the next trace queue) and material_out: 4 x capacity x RT_SORT_MATERIAL_WORDS {direction[3],
 * hit[4], pixel_index_and_flags, throughput[3], medium, cone_angle, cone_width, pad[2]} (diffuse, plastic, dielectric, conductor): every
 * device array is filled with `sentinel` first and read back to its capacity, so a word the launch did not write holds the sentinel.
 * counters6: {diffuse, plastic, dielectric, conductor, next trace queue, this trace queue} after the launch. aov_frames (in / out):
 * 4 x frame_slots * frame_pixels x 4 floats, RT_AOV_RADIANCE, _DIRECT, _INDIRECT, _ALBEDO; a frame the context has disabled is not
 * given to the kernel. gbuffer_* (in / out): 4 floats, 2 ints, 2 floats per pixel. pixel_query2 (in / out): what the launch answers
 * for the pixel of rt_set_pixel_query. stats (merged; out): 128 x 6 x RT_MAX_BOUNCES ints, rays per (submission, queue kind, bounce).
 * RT_ERROR_INVALID_ARG with a message, before anything is launched, for whatever could make the kernel read or write outside these
 * buffers or the context's tables: NULL arrays, count > capacity, a bounce outside [0, RT_MAX_BOUNCES) or not below num_bounces, a virtual pixel beyond the frames,
 * two entries with one virtual pixel (the AOV updates are plain read-modify-writes: one path per pixel and launch), a mesh id beyond
 * the instance table, a triangle id beyond the triangle array (other than RT_INVALID), a medium id beyond rt_upload_media's table on
 * an entry flagged inside a medium, a slot beyond the table, a submission beyond 128, an entry's bounce outside [0, min(RT_MAX_BOUNCES, num_bounces))
 * or a slot whose birth is not its submission's.                                                                              */
#define RT_SORT_TRACE_WORDS    20
#define RT_SORT_MATERIAL_WORDS 16
int rt_sort_rays(rt_context * ctx, int merged, int step, int sample_index, const uint32_t * trace_in, size_t count,
                 const int32_t * slot_table, size_t slot_count, const int32_t * submission_birth,
                 size_t capacity, size_t frame_slots, uint32_t sentinel,
                 uint32_t * trace_out, uint32_t * material_out, int32_t * counters6,
                 float * aov_frames, float * gbuffer_normal_and_depth, int32_t * gbuffer_mesh_id_and_triangle_id, float * gbuffer_screen_position_prev,
                 int32_t * pixel_query2, int32_t * stats);
/* The material launch on an explicit material queue (synchronous): the production launcher -- rt_launch_material (merged = 0: `step` is
 * the bounce, sample_index the launch's) or rt_launch_material_stream (merged = 1: `step` is the iteration; bounce and sample of an entry
 * come out of slot_table / submission_birth) -- for queue `material_slot` (0 diffuse, 1 plastic, 2 dielectric, 3 conductor), so the
 * instance (plain, _texels, _sky, _nmap and their combinations) and the grid are the shipped ones, on the context's own parameter block
 * with that material queue, the next trace queue, the shadow queue, the counters / control block, the slot table, the three AOV frames
 * the launch writes and the g-buffers replaced by buffers of this call. Nothing of the context changes but what a render would settle
 * (the Kulla-Conty tables for slots 2 and 3, the sky tables when sky sampling is wanted).
 * material_in: count x RT_SORT_MATERIAL_WORDS, exactly one of the four queues rt_sort_rays returns in material_out (virtual pixels, slot
 * table and frame_slots as there). trace_out: capacity x RT_SORT_TRACE_WORDS, the next trace queue in rt_sort_rays's trace_in layout.
 * shadow_out: capacity x RT_SHADE_SHADOW_WORDS {origin[3], direction[3], max_distance, illumination[3], pixel word (the virtual pixel;
 * merged form: | 1 << 30 on a ray emitted at bounce 0)}. counters3: {next trace queue, shadow queue, this material queue} after the
 * launch. aov_frames: 3 x frame_slots * frame_pixels x 4 words, RT_AOV_ALBEDO, _NORMAL, _POSITION (a frame the context has disabled is
 * not given to the kernel); gbuffer_*: 4, 2, 2 words per pixel. All of these are OUTPUTS: every device array is filled with `sentinel`
 * first and read back whole, so a word the launch did not write holds the sentinel. stats (merged; out): 128 x 6 x RT_MAX_BOUNCES ints.
 * RT_ERROR_INVALID_ARG with a message, before anything is launched, for whatever could make the kernel read or write outside these
 * buffers or the context's tables: NULL arrays, count > capacity, a bounce outside [0, RT_MAX_BOUNCES - 1) or not below num_bounces, a
 * virtual pixel beyond the frames, two entries with one virtual pixel, a mesh id beyond the instance table, a triangle id beyond the
 * triangle array, an instance whose material is not of the queue's type, a medium id beyond rt_upload_media's table on an entry flagged
 * inside a medium, a slot beyond the table, a submission beyond 128, an entry's bounce outside [0, min(RT_MAX_BOUNCES, num_bounces)) or
 * a slot whose birth is not its submission's. (An addition that changes no struct: RT_ABI_VERSION stays.)
 * While a fog volume of positive density is in force (rt_set_fog_volume) an entry of bounce 0 is shaded with the throughput its record carries, as the
 * ..._fog sort instances store it (the camera's segment may have crossed the fog); without one, bounce 0 takes a throughput of 1 whatever the record holds. */
#define RT_SHADE_SHADOW_WORDS 11
int rt_shade_rays(rt_context * ctx, int merged, int step, int sample_index, int material_slot, const uint32_t * material_in, size_t count,
                  const int32_t * slot_table, size_t slot_count, const int32_t * submission_birth,
                  size_t capacity, size_t frame_slots, uint32_t sentinel,
                  uint32_t * trace_out, uint32_t * shadow_out, int32_t * counters3,
                  uint32_t * aov_frames, uint32_t * gbuffer_normal_and_depth, uint32_t * gbuffer_mesh_id_and_triangle_id, uint32_t * gbuffer_screen_position_prev,
                  int32_t * stats);
/* The accumulate launch on explicit images (synchronous): ONE launch of the production launcher -- rt_launch_accumulate (merged = 0: one
 * submission, first_sample[0] the sample index the fold starts at, sample_count[0] <= 16 the samples of the batch) or
 * rt_launch_accumulate_group (merged = 1: 1 .. 8 submissions folded in order, as the merged wavefront completes them) -- over the
 * context's own pixel set (rt_set_pixel_range / rt_set_pixel_tiles). frames (in / out): the samples of all submissions, one after the
 * other, pitch*height float4 each (at most 512, below 2^30 pixels together; the merged form clears what it folds). accumulator (in / out):
 * the RADIANCE mean, pitch*height float4; no other AOV is given to the kernel. moments (in / out): NULL -- the plain kernel runs -- or the
 * (M2_r, M2_g, M2_b, w) image, and the ..._moments kernel runs. final_image (out): pitch*height float4, filled with `sentinel` first; the
 * caller fills the in / out images, so a pixel outside the set keeps what it was given everywhere. Sample indices are >= 0 and stay below
 * 2^24. Leaves no state a frame reads. RT_ERROR_INVALID_ARG with a message for anything else, a NULL context first -- and while the
 * context covers a pixel list (rt_set_pixel_list): rt_accumulate_list_frames is the probe of that launch.                               */
int rt_accumulate_frames(rt_context * ctx, int merged, const int32_t * first_sample, const int32_t * sample_count, size_t submissions,
                         float * frames, float * accumulator, float * moments, uint32_t sentinel, float * final_image);
/* rt_estimate_noise's kernel on explicit images of the context's frame size (synchronous): mean and moments are pitch*height float4 from
 * the caller; everything else as rt_estimate_noise, which need not be enabled.                                                          */
int rt_estimate_noise_images(rt_context * ctx, const float * mean, const float * moments, float floor, rt_noise_estimate * out, double * cell_sums,
                             int32_t * cell_counts, int32_t * cell_nonfinite, size_t cell_capacity, float * pixel_map);
/* Selection and compaction (rt_select_active_cells' kernels) on explicit images of the context's frame size (synchronous): mean and
 * moments are pitch*height float4. The cell arrays (cell_capacity >= cells_x * cells_y entries each; cell_flags bytes) and the list
 * (list_capacity >= width * height entries; out->list_pixels are written) come back. Leaves the context's own list alone.            */
int rt_select_pixels_images(rt_context * ctx, const float * mean, const float * moments, float floor, float threshold, int dilate, rt_cell_selection * out,
                            double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, uint8_t * cell_flags, size_t cell_capacity,
                            uint32_t * list, size_t list_capacity);
/* ONE launch of the list accumulate launcher (what the merged wavefront runs for list submissions) on explicit images (synchronous):
 * 1 .. 8 submissions of sample_count[k] samples; first_sample is passed on and does not enter the fold. frames, accumulator, moments
 * (required), final_image and sentinel as in rt_accumulate_frames. list: list_count entries x + y * width. Refused before any launch
 * (RT_ERROR_INVALID_ARG): an entry outside the frame and a pixel listed twice -- the fold is a plain read-modify-write.                */
int rt_accumulate_list_frames(rt_context * ctx, const int32_t * first_sample, const int32_t * sample_count, size_t submissions,
                              float * frames, float * accumulator, float * moments, const uint32_t * list, size_t list_count, uint32_t sentinel, float * final_image);
/* rt_denoise's launchers on explicit images of a size of the caller's (synchronous; the context needs no frame, no scene and no estimate): colour, moments,
 * albedo, normal, position and fallback (what rt_denoise takes from the final image) are pitch*height float4, pitch >= width, width * height and pitch * height
 * below 2^26; eye: the camera position. out: pitch*height float4, read first: what the kernels do not write -- the padding columns -- comes back as the caller
 * gave it. tiled = 1: the passes stage their taps in LDS (what rt_denoise runs), 0: the plain pass kernel; the two agree bit for bit. Parameters are refused as
 * by rt_denoise. Leaves the context's own images untouched.                                                                                              */
int rt_denoise_images(rt_context * ctx, int width, int height, int pitch, const float * colour, const float * moments, const float * albedo, const float * normal,
                      const float * position, const float * fallback, const float * eye, const rt_denoise_params * params, int tiled, float * out);
/* rt_accumulate_frames and rt_accumulate_list_frames in one, with the cascade: ONE launch of the production launcher (rt_set_firefly_cascade's kernels) on
 * explicit images. merged = 0: the batch form (one submission, <= 16 samples, frames not cleared); merged = 1: the merged group; list != NULL (merged must be 1):
 * the group over a pixel list, checked as by rt_accumulate_list_frames. tiers: params->tiers images of pitch*height float4 one behind the other, in and out.
 * moments is required. Everything else as in those two probes; params->support is checked and not used.                                            */
int rt_accumulate_cascade_frames(rt_context * ctx, int merged, const int32_t * first_sample, const int32_t * sample_count, size_t submissions, float * frames,
                                 float * accumulator, float * moments, const uint32_t * list, size_t list_count, const rt_firefly_params * params, float * tiers,
                                 uint32_t sentinel, float * final_image);
/* rt_resolve_fireflies' kernel on explicit images of a size of the caller's (synchronous; the context needs no frame and no scene): mean, moments and fallback are
 * pitch*height float4, tiers params->tiers such images one behind the other, pitch >= width, pitch * height below 2^26. out: pitch*height float4, read first: what
 * the kernel does not write -- the padding columns -- comes back as the caller gave it. tiled = 1: the W of a tile's halo staged in LDS (what rt_resolve_fireflies
 * runs), 0: the plain kernel; the two agree bit for bit.                                                                                            */
int rt_resolve_fireflies_images(rt_context * ctx, int width, int height, int pitch, const float * mean, const float * moments, const float * tiers, const float * fallback,
                                const rt_firefly_params * params, int tiled, float * out);
/* rt_measure_exposure's kernel on explicit images of a size of the caller's (synchronous; the context needs no frame, no scene and no estimate): mean and
 * moments are pitch*height float4, pitch >= width, pitch * height below 2^26.                                                                          */
int rt_measure_exposure_images(rt_context * ctx, int width, int height, int pitch, const float * mean, const float * moments, rt_exposure * out, uint64_t * histogram256);
/* rt_estimate_noise_robust's cells kernel and the robust selection on explicit images of the context's frame size (synchronous): as rt_estimate_noise_images and
 * rt_select_pixels_images, with `resolved` -- pitch*height float4 as rt_read_resolved gives them -- from the caller instead of a resolve, and cell_held beside
 * the other cell arrays. Neither needs the estimate or the cascade.                                                                                     */
int rt_estimate_noise_robust_images(rt_context * ctx, const float * mean, const float * moments, const float * resolved, float floor, float held_fraction,
                                    rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, int32_t * cell_held, size_t cell_capacity,
                                    float * pixel_map, int64_t * out_held_pixels);
int rt_select_pixels_robust_images(rt_context * ctx, const float * mean, const float * moments, const float * resolved, float floor, float held_fraction, float threshold,
                                   int dilate, rt_cell_selection * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, int32_t * cell_held,
                                   uint8_t * cell_flags, size_t cell_capacity, uint32_t * list, size_t list_capacity);
/* ---- fog volume ---------------------------------------------------------------------------------------------------
 * One scene-wide homogeneous medium inside an axis-aligned box, with multiple scattering and light sampling at every scatter vertex. Off
 * until a volume is set; while it is off a context launches exactly the kernels it launched before these calls existed. (Additions that
 * change no struct and no call: RT_ABI_VERSION stays.)
 * rt_set_fog_volume: NULL clears the volume. Checked on the host before anything is staged -- a finite box with min < max on every axis,
 * finite sigmas >= 0, |g| < 1 -- and a refused call (RT_ERROR_INVALID_ARG with a message) leaves the volume before it in force. A change
 * completes what the context has in flight first. A volume whose sigma_a + sigma_s is 0 in all three channels is stored (rt_get_fog_volume
 * returns it) but renders as no volume. Rendering with a volume in force and enable_svgf is refused (a scatter vertex has no g-buffer);
 * the AO integrator ignores the volume.                                                                                            */
typedef struct rt_fog_volume {
	float box_min[3], box_max[3];
	float sigma_a[3], sigma_s[3];   /* absorption and scattering coefficients per unit length, RGB */
	float g;                        /* Henyey-Greenstein asymmetry, |g| < 1 */
	uint32_t reserved[3];           /* ignored on input, 0 on output */
} rt_fog_volume;                    /* 64 bytes */
int rt_set_fog_volume(rt_context * ctx, const rt_fog_volume * volume);
int rt_get_fog_volume(rt_context * ctx, rt_fog_volume * out, int * out_set);
/* The fog's segment step on explicit segments (synchronous), through the device functions the sort kernels call, on the volume in force
 * (RT_ERROR_NOT_READY without one; a volume of zero density is taken as it is). probes: count x RT_FOG_SEGMENT_IN 32-bit words {o[3],
 * d[3], t_end (RT_INFINITY: a miss), pixel, bounce, sample (uint32), throughput[3], inside_medium (uint32: 0 / 1), pad[2]}. out: count x
 * RT_FOG_SEGMENT_OUT words {t0, t1 (the clipped interval; both 0 when it is empty), the two random numbers, scattered (uint32), distance
 * (along the clipped interval; RT_INFINITY beyond its end), throughput'[3], vertex[3], pad[4]}. An entry flagged inside a medium comes back
 * with t0 = t1 = 0, its throughput untouched. Needs the RNG tables and rt_resize (the pixel's random numbers).                       */
#define RT_FOG_SEGMENT_IN  16
#define RT_FOG_SEGMENT_OUT 16
int rt_fog_segments(rt_context * ctx, const uint32_t * probes, size_t count, uint32_t * out);
/* kernel_fog_attenuate_shadows on an explicit shadow queue (synchronous): shadow_in / shadow_out: count x RT_SHADE_SHADOW_WORDS in
 * rt_shade_rays' layout. The launch is the one of the context's scheduler (rt_set_scheduler): the per-bounce loop's reads the count from
 * RtBufferSizes::shadow[0], the merged wavefront's from the control block's shadow_count[0]. The volume in force applies (RT_ERROR_NOT_READY
 * without one; a volume of zero density is taken as it is).                                                                          */
int rt_attenuate_shadow_rays(rt_context * ctx, const uint32_t * shadow_in, size_t count, uint32_t * shadow_out);
/* rt_sort_rays with the fog volume in force: the ..._fog instance of the sort launch, which appends the light samples of its scatter
 * vertices to the shadow queue. Arguments as rt_sort_rays, plus shadow_out: capacity x RT_SHADE_SHADOW_WORDS (rt_shade_rays' layout; filled
 * with the sentinel first) and shadow_count: the shadow queue's counter after the launch. RT_ERROR_NOT_READY without a volume of positive
 * density.                                                                                                                          */
int rt_sort_rays_fog(rt_context * ctx, int merged, int step, int sample_index, const uint32_t * trace_in, size_t count,
                     const int32_t * slot_table, size_t slot_count, const int32_t * submission_birth,
                     size_t capacity, size_t frame_slots, uint32_t sentinel,
                     uint32_t * trace_out, uint32_t * material_out, int32_t * counters6,
                     float * aov_frames, float * gbuffer_normal_and_depth, int32_t * gbuffer_mesh_id_and_triangle_id, float * gbuffer_screen_position_prev,
                     int32_t * pixel_query2, int32_t * stats, uint32_t * shadow_out, int32_t * shadow_count);
/* ---- density grid of the fog volume -----------------------------------------------------------------------------------
 * rho[z][y][x], nx x ny x nz float32 values laid over the box of the fog volume in force (x fastest; voxel (i, j, k) spans [min + i * cell,
 * min + (i + 1) * cell) per axis, cell = (max - min) / n; no interpolation): inside a voxel the coefficients are rho * sigma_a and rho *
 * sigma_s, g is unchanged. Paths scatter by the homogeneous scheme over DENSITY LENGTH (the integral of rho along the ray, by a voxel march
 * that crosses bricks of 8 x 8 x 8 voxels without density in one step); shadow rays are multiplied by exp(-sigma_t * density length).
 * (Additions that change no struct and no call: RT_ABI_VERSION stays.)
 * rt_set_fog_density: `density` is a host pointer; NULL clears the grid. Checked on the host before anything is staged -- dims in 1 .. 1024,
 * nx * ny * nz <= 2^27, every value finite and >= 0 -- and a refused call (RT_ERROR_INVALID_ARG, the message names the first bad cell)
 * leaves the grid before it in force. A change completes what the context has in flight first. The grid is state of its own: it survives
 * rt_set_fog_volume calls and maps onto whatever box is in force; without a volume it is stored and inert. A grid of zeros renders as no
 * volume (exactly the kernels of a context without one). rt_fog_segments stays the homogeneous step and ignores the grid;
 * rt_attenuate_shadow_rays and rt_sort_rays_fog launch what the context would launch: the ..._grid instances while a grid is in force.
 * rt_get_fog_density_info: the dims of the grid in force, its bricks (ceil(n / 8) per axis), how many hold no density, the largest value.
 * rt_fog_density_segments: rt_fog_segments' records through the grid's segment step, with pad words filled: word 12 the density length (over
 * the whole clipped interval when the path did not scatter, over [t0, vertex] when it did), word 13 the voxels read, word 14 the empty
 * bricks crossed. RT_ERROR_NOT_READY without a volume or without a grid.                                                             */
int rt_set_fog_density(rt_context * ctx, const float * density, int nx, int ny, int nz);
int rt_get_fog_density_info(rt_context * ctx, int dims[3], int * bricks, int * empty_bricks, float * max_density, int * out_set);
int rt_fog_density_segments(rt_context * ctx, const uint32_t * probes, size_t count, uint32_t * out);
/* Streaming-read bandwidth probe used as the measured HBM roofline (GB/s).                 */
int rt_measure_stream_bandwidth(rt_context * ctx, size_t bytes, int repeat, float * out_gbps);

#ifdef __cplusplus
}
#endif
#endif /* GPU_RAYTRACER_AMD_H */
