// rt_types.h -- device-side data layout shared by the C ABI implementation and the kernels.
//
// HBM layout (all buffers are plain hipMalloc'd linear memory, 16-byte aligned):
//   triangles      float4[6 * T]   device triangle = 96 B (reference CUDA/Raytracing/Triangle.h:4-11)
//   bvh8_nodes     float4[5 * N]   CWBVH node = 80 B        (reference CUDA/Raytracing/BVH8.h:19-25)
//   per-instance   int[M], float4[3 * M] x3                 (reference CUDA/Raytracing/Mesh.h:29-36)
//   ray queues     SoA, one float/uint array per component, RT_BATCH_SIZE entries each
//                  (reference Pathtracer.cu:32-66) -- every queue access by consecutive lanes
//                  is a fully coalesced 256 B transaction per 64-lane wave.
//   AOVs           float4[pitch * height] framebuffer + accumulator per enabled AOV
// Material queues: the reference packs two material types into one allocation growing from
// both ends to save VRAM (Pathtracer.cu:73-90); with 288 GB of HBM3E each type simply gets
// its own queue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpu_raytracer_amd.h"
#include "rt_light_tree.h"

#define RT_WAVE_SIZE 64
#define RT_INFINITY __builtin_huge_valf()

struct RtVec3SoA { float * x, * y, * z; };

struct RtTraceBuffer { // Pathtracer.cu:33-46
	RtVec3SoA origin, direction;
	uint4   * hits;
	float   * cone_angle, * cone_width;
	int     * medium;
	unsigned * pixel_index_and_flags;
	RtVec3SoA throughput;
	float   * last_pdf;
};

struct RtMaterialBuffer { // Pathtracer.cu:49-61
	RtVec3SoA direction;
	uint4   * hits;
	float   * cone_angle, * cone_width;
	int     * medium;
	unsigned * pixel_index_and_flags;
	RtVec3SoA throughput;
};

struct RtShadowBuffer { // Pathtracer.cu:64-68, BVH.h:16-21
	RtVec3SoA origin, direction;
	float  * max_distance;
	float4 * illumination_and_pixel_index;
};

struct RtBufferSizes { // Pathtracer.cu:103-114
	int trace     [RT_MAX_BOUNCES];
	int diffuse   [RT_MAX_BOUNCES];
	int plastic   [RT_MAX_BOUNCES];
	int dielectric[RT_MAX_BOUNCES];
	int conductor [RT_MAX_BOUNCES];
	int shadow    [RT_MAX_BOUNCES];
	int rays_retired       [RT_MAX_BOUNCES];
	int rays_retired_shadow[RT_MAX_BOUNCES];
};

// ---- merged wavefront (rt_context.h, "PathStream") ---------------------------------------------------------
// Instead of one launch chain per submission (generate -> (trace, sort, shade, shadow) x bounces), whose launches
// shrink bounce by bounce until they no longer fill the GPU, consecutive submissions feed ONE wavefront: iteration
// i traces / sorts / shades the rays of every submission in flight -- the primary rays of the newest next to bounce
// 1 of the one before, bounce 2 of the one before that ... -- so every launch has the size of a whole sample and
// there are no per-submission tails. A queue entry does not store its bounce: its virtual pixel index names a SAMPLE
// SLOT (v = slot * frame_pixels + pixel; the slot's per-sample AOV frame lives at the same offset), and the slot table
// says which sample that is and in which iteration it was generated; bounce = iteration - birth.
#define RT_STREAM_SAMPLE_SLOTS 512    // samples in flight (each owns one frame of the per-sample AOV buffers)
#define RT_STREAM_SUBMISSIONS  128    // ring of submissions whose per-bounce statistics are kept
enum { RT_STAT_TRACE = 0, RT_STAT_SHADOW, RT_STAT_DIFFUSE, RT_STAT_PLASTIC, RT_STAT_DIELECTRIC, RT_STAT_CONDUCTOR, RT_STAT_KINDS };

struct RtStreamSlot { int sample_index, birth_iteration, submission, index_in_submission; }; // one int4 per sample slot

struct RtStreamTable {                 // written by the host per submission (asynchronous copy in stream order)
	RtStreamSlot slots[RT_STREAM_SAMPLE_SLOTS];
	int submission_birth[RT_STREAM_SUBMISSIONS];
};

#define RT_ENDGAME_MAX_WAVES 16384     // waves of the persistent traversal grid that can own a region of a queue's end (256 CUs x 16 workgroups x 4)
struct RtStreamControl {               // queue sizes and ray-claim cursors; [iteration & 1] where two launches overlap in time
	int trace_count[2];                // rays in trace queue [i & 1]: appended by sort / shade of i - 1 and generate of i
	int material_count[4];
	int shadow_count[2];               // shadow rays emitted by the shade kernels of iteration i, traced by the launch of i + 1
	int cursor[2][2];                  // [i & 1][closest, shadow] cursors of the fused trace launch
	int pad[4];
	int stats[RT_STREAM_SUBMISSIONS][RT_STAT_KINDS][RT_MAX_BOUNCES]; // rays per submission, queue kind and bounce
	int endgame[2][2][RT_ENDGAME_MAX_WAVES];   // [i & 1][closest (or the mixed launch's one queue), shadow][region]: the end of a queue is dealt in regions, one per wave, that other waves help to finish (kernels_trace.hip: fetch_ray)
};

struct RtTexture {
	const uchar4 * texels;   // linear RGBA8, mip levels back to back; or BC1 blocks (uint2 each); or expanded blocks (16 texels each), see `format`
	int   width, height, mip_levels;
	float lod_bias;          // 0.5 * log2(width * height)   (Integrator.cpp:95)
	int   format;            // RT_TEXTURE_RGBA8 / RT_TEXTURE_BC1 / RT_TEXTURE_BC1_EXPANDED
	int   pad;
};
// Device-only format (rt_set_texture_expansion, on by default): a BC1 texture whose blocks rt_upload_textures has decoded ONCE,
// with the shade kernels' own bc1_texel, into 16 RGBA8 texels each -- 64 bytes per block, row-major inside the block, blocks and
// levels in the order of the compressed chain. The reference leaves the decode to NVIDIA's texture unit; this chip has none, and
// decoding a block per texel fetch was ~55 vector instructions x 8 texels x up to 16 probes per lookup: a third of a shade
// kernel's instructions. 8 x the bytes of BC1 (Sponza: 13 -> 105 MB of 288 GB), the same texel values to the bit, and a bilinear
// footprint still lies in one or two 64-byte blocks (a linear RGBA8 image would spread it over two rows).
#define RT_TEXTURE_BC1_EXPANDED 2

struct RtAOV { float4 * framebuffer, * accumulator; };

// Opacity mask of a material (rt_upload_material_opacity): one bit per texel of level 0 of a texture, bit y * width + x
// in word (y * width + x) >> 5, no row padding; 1: opaque. Built once on the device; the traversal kernels read nothing else of the texture.
struct RtOpacityMask { const unsigned * bits; int width, height; };

// One delta emitter as staged by rt_upload_delta_lights (RT_DELTA_LIGHT_RECORD floats, read back by rt_read_delta_lights).
struct RtDeltaLight {
	float4 position_type;        // position, type (int bits: RT_DELTA_LIGHT_*)
	float4 direction_pdf;        // unit direction (spot: axis; directional: the way the light travels), P_k: the light's selection probability
	float4 intensity_cos_cutoff; // intensity (W/sr; directional: irradiance), cos(cutoff)
	float4 spot;                 // cos(beam), cutoff (radians), 1 / (cutoff - beam), pad
};

// Everything a kernel needs, passed BY VALUE as kernel argument (lives in the kernarg
// segment and is read with scalar loads; no __constant__ symbols, so several contexts
// can coexist in one process).
struct RtParams {
	// geometry
	const float4 * triangles;            // 6 float4: full shading triangle
	const float4 * triangle_positions;   // 3 float4: position_0, edge_1, edge_2 (traversal copy)
	const float4 * bvh8_nodes;
	const float4 * bvh2_nodes;  // 2 float4 per node
	const float4 * bvh4_nodes;  // 8 float4 per node
	// The TLAS (node indices [0, tlas_node_count) of whichever BVH type is selected) is versioned per
	// frame and lives outside the static node arrays, see rt_context.h (SceneRing).
	const float4 * tlas_nodes;
	int tlas_node_count;
	int bvh_width;              // 8: CWBVH kernels (default), 4: 4-wide BVH kernels, 2: binary-BVH kernels
	const int    * mesh_bvh_root_indices;
	int mesh_count;                   // instances (the fused traversal launch keeps the root table of a small scene in LDS)
	int geometry_below_4gib;          // bvh8_nodes and triangle_positions are both shorter than 4 GiB: the flattened scene's engine addresses them with 32-bit offsets
	int entry_tlas_stack_size;        // RT_INVALID: rays start at the TLAS root; 0: node 0 is the root of the one world-space tree that holds the
	                                  // whole scene and rays start inside it, as instance row 0 (rt_set_static_geometry)
	int skip_behind_hit;              // rt_set_skip_behind_hit's wish (default 1); what the kernels do is rt_skip_walk(p) below
	int has_triangle_aliases;         // some triangles are copies that report the (instance, triangle) named in the padding of their
	                                  // position record instead of themselves (rt_upload_triangle_aliases)
	const int    * mesh_material_ids;
	const float4 * mesh_transforms, * mesh_transforms_inv, * mesh_transforms_prev;
	// TLAS built on the device (rt_build_tlas): scene index of an instance -> its position in TLAS order, for tables that
	// name instances by scene index (light_mesh_transform_indices); null when the host supplied everything in TLAS order
	const int    * mesh_position;
	// materials
	const uint8_t * material_types;
	const float4  * materials;  // 2 float4 per material
	const float4  * media;      // 2 float4 per medium
	const RtTexture * textures;
	int svgf_tiles;                   // 1 (default): the a-trous passes stage a workgroup's taps in LDS (rt_set_svgf_tiles; kernels_post.hip: kernel_svgf_atrous_tiled)
	int textures_compressed;          // 1: at least one texture holds BC1 blocks that a fetch has to decode (rt_set_texture_expansion(ctx, 0)); picks the material kernels' instantiation
	// lights
	const int   * light_triangle_indices;
	const float * light_triangle_cumulative_probability;
	const float * light_mesh_cumulative_probability;
	const int2  * light_mesh_triangle_span;
	const int   * light_mesh_transform_indices;
	int   light_mesh_count, light_triangle_count;
	float lights_total_weight;
	// rng
	const float2 * pmj_samples;
	const uchar2 * blue_noise;
	// sky
	const float4 * sky;
	int sky_width, sky_height;
	float sky_scale;
	// Kulla-Conty LUTs
	const float * lut_dielectric_directional_albedo_enter, * lut_dielectric_directional_albedo_leave;
	const float * lut_dielectric_albedo_enter, * lut_dielectric_albedo_leave;
	const float * lut_conductor_directional_albedo, * lut_conductor_albedo;
	// frame
	rt_camera     camera;
	rt_gpu_config config;
	float view_projection[16], view_projection_prev[16];
	int screen_width, screen_height, screen_pitch;
	// Sample batching: rt_render_samples renders `batch_samples` consecutive samples of every pixel as
	// ONE wavefront. The queues and the per-sample AOV frame buffers are addressed with a "virtual"
	// pixel index v = s * frame_pixels + pixel (s = sample within the batch, frame_pixels = pitch *
	// height); only the RNG needs (pixel, first_sample + s) back, see rt_split_virtual_pixel.
	unsigned frame_pixels, frame_pixels_magic; // magic = floor(2^32 / frame_pixels) + 1
	int batch_samples;
	// pixel query (PixelQuery of the reference, CUDA/Pathtracer.cu:345-348): the bounce-0 hit of this pixel
	// index (x + y * pitch, -1 = none) is written to pixel_query_out[0..1] = { mesh_id, triangle_id }
	int   pixel_query_pixel;
	int * pixel_query_out;
	// multi-GPU tile split: local pixel i -> scan-order pixel (tile_pixels == 0: identity)
	int tile_pixels, tile_first, tile_stride;
	// queues
	RtTraceBuffer    trace[2];
	RtMaterialBuffer material[4];   // diffuse, plastic, dielectric, conductor
	RtShadowBuffer   shadow;
	RtBufferSizes  * sizes;
	// merged wavefront only (null / 0 otherwise)
	RtStreamControl     * stream;
	const RtStreamTable * stream_table;
	int stream_iteration;
	int * ray_cursors;                // [RT_MAX_BOUNCES][2 (closest, shadow)] ray-fetch cursors
	uint2 * stack_spill;                // traversal stack entries beyond the LDS part, [entry][grid lane]
	// outputs
	RtAOV    aovs[RT_AOV_COUNT];
	float4 * final_image;           // the reference's `accumulator` surface
	// SVGF / TAA
	float4 * gbuffer_normal_and_depth;
	int2   * gbuffer_mesh_id_and_triangle_id;
	float2 * gbuffer_screen_position_prev;
	float4 * frame_buffer_moment;
	int    * history_length;
	float4 * history_direct, * history_indirect, * history_moment, * history_normal_and_depth;
	float4 * taa_frame_prev, * taa_frame_curr, * taa_frame_next;   // next: where kernel_taa writes the history of the following frame (swapped with prev after every filtered frame)
	int * svgf_young_pixels;          // [0]: how many pixels this frame's kernel_svgf_reproject left with fewer than 4 frames of history, [RT_SVGF_YOUNG_HEADER ...]: their indices (kernel_svgf_variance_listed); emptied by kernel_svgf_finalize
	float2 * svgf_variance[2];        // (direct.w, indirect.w) of the radiance framebuffers [0] and accumulators [1], kept in step by the filter kernels
	float4 * svgf_normal_and_depth;   // (normal, depth) of the frame being filtered: decoded once by kernel_svgf_reproject for the variance / a-trous taps
	// Sky importance sampling (rt_set_sky_sampling; tables built by kernels_sky.hip, one cell per sky texel, row-major). Opt-in: while
	// sky_nee_share is 0 the tables may be null and every kernel takes the reference's estimator (the ..._sky kernel instances are not launched).
	const float * sky_marginal_cdf;     // [sky_height]: inclusive, normalised CDF over rows; last entry 1
	const float * sky_conditional_cdf;  // [sky_height][sky_width]: inclusive, normalised CDF of each row; last entry 1
	const float * sky_cell_pdf;         // [sky_height][sky_width]: pdf (solid angle) of every direction in the cell
	float sky_nee_share;                // probability that a light sample goes to the sky: 0 off / inactive; rt_set_sky_sampling's value with triangle emitters, 1 without
	// Tangent-space normal maps (rt_upload_material_normal_maps): the map of each material (RT_INVALID: none), and bit s set
	// when some material of slot s (diffuse, plastic, dielectric, conductor) has one -- only then does the launcher take that slot's _nmap instance.
	const int * material_normal_maps;
	int normal_map_slots;
	// Alpha-tested opacity masks (rt_upload_material_opacity): the mask of each material as an index into opacity_masks (RT_INVALID: none).
	// opacity_active: some material has one -- only then do the launchers take the CWBVH kernels' _mask instances, the only code that reads these fields.
	const int * material_opacity;
	const RtOpacityMask * opacity_masks;
	int opacity_active;
	// Delta emitters (rt_upload_delta_lights): the records and their inclusive, normalised CDF (last entry 1). delta_nee_share (q) is the
	// probability that a light sample goes to a delta light, settled per render beside sky_nee_share (s); nee_taken = s + q is what the sky and the delta
	// lights take together (with q == 0 it is s to the bit). While q is 0 the tables may be null; only the ..._split kernel instances read these.
	const RtDeltaLight * delta_lights;
	const float * delta_light_cdf;
	int   delta_light_count;
	float delta_nee_share, nee_taken;
	// Fog volume (rt_set_fog_volume): one homogeneous medium inside an axis-aligned box. fog_active: a volume of positive density is in
	// force -- only then do the launchers take the ..._fog instances of the sort kernels and the attenuation pass of the shadow queue, the only kernels
	// that read the other fog fields; a material kernel reads fog_active alone (a path's first segment may then have lost throughput, see shade_material).
	int   fog_active;
	float fog_box_min[3], fog_box_max[3];
	float fog_sigma_a[3], fog_sigma_s[3];
	float fog_g;
	// Density grid of the fog volume (rt_set_fog_density): rho[z][y][x] over the box above, x fastest, and one byte per brick of 8 x 8 x 8
	// voxels (0: the brick holds no density). fog_grid: a grid with a positive maximum is in force -- only then do the launchers take the ..._fog_grid sort
	// instances and the ..._grid attenuation kernels, the only kernels that read these fields. (A grid of zeros clears fog_active instead.)
	int   fog_grid;
	int   fog_grid_dims[3];
	const float * fog_density;
	const unsigned char * fog_bricks;
	// Light tree (rt_set_light_tree, DESIGN.md 7.11, rt_light_tree.h): position-aware selection of the triangle emitters. light_tree.padded > 0: a tree is
	// built -- only then, with next-event estimation on and no fog volume in force, do the launchers take the ..._tree instances of the sort and material
	// kernels, the only kernels that read these fields.
	RtLightTree light_tree;
};
// Which instances of the sort and material kernels a launcher takes: 0 the plain ones, 1 the ..._sky ones (sky importance sampling alone), 2 the ..._split
// ones (delta lights take a share, with or without the sky), 3 the ..._tree ones (a light tree is in force: everything 2 does, nee_taken may be 0, the emitters
// picked by the tree). Shadow rays are traced without triangle emitters whenever it is not 0.
static inline __host__ __device__ bool rt_light_tree_in_force(const RtParams & p) {
	return p.light_tree.padded > 0 && p.config.enable_next_event_estimation && !p.fog_active && p.lights_total_weight > 0.0f;
}
static inline __host__ __device__ int rt_light_split(const RtParams & p) { return rt_light_tree_in_force(p) ? 3 : p.delta_nee_share > 0.0f ? 2 : p.sky_nee_share > 0.0f ? 1 : 0; }
static inline __host__ __device__ bool rt_light_samples_split(const RtParams & p) { return rt_light_split(p) != 0; }
// "Skip behind the hit" (kernels_trace.hip): closest-hit rays drop stacked groups of children that lie behind the hit they hold. Taken when the context wants it
// (rt_set_skip_behind_hit) AND the scene is ONE tree the flattened scene's engine walks (rt_set_static_geometry(ctx, 1), arrays below 4 GiB): every CWBVH
// closest-hit kernel -- the merged wavefront's launch, its counting variant, the per-bounce and the explicit kernels -- decides by this one rule.
static inline __host__ __device__ bool rt_skip_walk(const RtParams & p) { return p.skip_behind_hit != 0 && p.entry_tlas_stack_size == 0 && p.geometry_below_4gib != 0; }


// Scan-order index of local pixel i of this context: its tiles are tile_first, tile_first +
// tile_stride, ... each tile_pixels long (whole rows), see gpu-raytracer_amd/parallel.py.
__device__ __forceinline__ int rt_map_pixel(const RtParams & p, int i) {
	if (p.tile_pixels == 0) return i;
	return ((i / p.tile_pixels) * p.tile_stride + p.tile_first) * p.tile_pixels + i % p.tile_pixels;
}

// v -> pixel, and the sample within the batch (v < 2^30, at most 16 samples per batch)
__device__ __forceinline__ unsigned rt_split_virtual_pixel(const RtParams & p, unsigned v, unsigned & sample_in_batch) {
	unsigned s = __umulhi(v, p.frame_pixels_magic);   // floor(v / frame_pixels) or one too many
	if (s * p.frame_pixels > v) s--;
	sample_in_batch = s;
	return v - s * p.frame_pixels;
}

// merged wavefront: slot, sample and bounce of a queue entry (see RtStreamSlot). `sample_index_for_rng` is what
// random_sample() expects from its callers: it adds the slot number it splits off the virtual index itself.
struct RtPathInfo { int bounce, submission; unsigned sample_index_for_rng; bool first_of_submission; };
__device__ __forceinline__ RtPathInfo rt_stream_path_info(const RtParams & p, unsigned virtual_pixel) {
	unsigned slot;
	rt_split_virtual_pixel(p, virtual_pixel, slot);
	RtStreamSlot e = p.stream_table->slots[slot];
	RtPathInfo info;
	info.bounce = p.stream_iteration - e.birth_iteration;
	info.submission = e.submission;
	info.sample_index_for_rng = unsigned(e.sample_index) - slot;
	info.first_of_submission = e.index_in_submission == 0;
	return info;
}

#define RT_FLAG_ALLOW_NEE     (1u << 31)
#define RT_FLAG_INSIDE_MEDIUM (1u << 30)
#define RT_FLAGS_ALL          (RT_FLAG_ALLOW_NEE | RT_FLAG_INSIDE_MEDIUM)
#define RT_SHADOW_FLAG_BOUNCE_0 (1u << 30)   // merged wavefront: pixel word of a shadow ray emitted at bounce 0

// Launch helpers implemented in the kernel translation units
void rt_launch_generate(const RtParams & p, int sample_index, int pixel_offset, int pixel_count, hipStream_t stream);
void rt_launch_expand_bc1(const uint2 * blocks, uchar4 * texels, size_t block_count, hipStream_t stream);
void rt_launch_trace(const RtParams & p, int bounce, hipStream_t stream);
// merged wavefront (the iteration is p.stream_iteration); stats: null, or 10 x u64 as for the counting variants below
void rt_launch_generate_stream(const RtParams & p, int sample_index, int pixel_offset, int pixel_count, int slot_base, int queue_offset, int block_width, int band_rows, hipStream_t stream);
void rt_launch_stream_advance(RtStreamControl * control, int iteration, int generated, int * progress, int reset_ring_first, int reset_ring_count, hipStream_t stream);
void rt_launch_trace_stream(const RtParams & p, unsigned long long * stats, hipStream_t stream);
enum { RT_STREAM_KERNEL_GENERAL = 0, RT_STREAM_KERNEL_FLAT = 1, RT_STREAM_KERNEL_FLAT_SKIP = 2, RT_STREAM_KERNEL_COUNTING = 3,
       RT_STREAM_KERNEL_GENERAL_MASK = 4, RT_STREAM_KERNEL_FLAT_MASK = 5, RT_STREAM_KERNEL_FLAT_SKIP_MASK = 6, RT_STREAM_KERNEL_COUNTING_MASK = 7 };   // (_MASK: p.opacity_active)
void rt_trace_stream_launch_info(const RtParams & p, bool stats, int32_t * info);   // the kernel rt_launch_trace_stream picks, its grid in waves, the two engine limits
void rt_trace_queue_launch_info(const RtParams & p, bool counting, bool ao, int32_t * info);   // the per-bounce launchers' choice: BVH width, waves of the closest-hit and of the shadow grid, RT_NARROW_MAX_RAYS, RT_FETCH_BLOCK_MAX
void rt_launch_sort_stream(const RtParams & p, hipStream_t stream);
void rt_launch_material_stream(const RtParams & p, int material_slot, hipStream_t stream);
void rt_launch_trace_shadow(const RtParams & p, int bounce, hipStream_t stream);
void rt_launch_ambient_occlusion(const RtParams & p, int sample_index, float ao_radius, hipStream_t stream);
void rt_launch_trace_shadow_ao(const RtParams & p, hipStream_t stream);
void rt_launch_sort(const RtParams & p, int bounce, int sample_index, hipStream_t stream);
void rt_launch_material(const RtParams & p, int material_slot, int bounce, int sample_index, hipStream_t stream);
#define RT_SVGF_YOUNG_HEADER 16
// The accumulate step (kernels_accumulate.hip): ONE launch folds the submissions of `group`, in order, into the accumulators.
//   group    count submissions; submission k holds sample_count[k] samples from first_sample[k] on, its sample frames slot_base[k] frames into the AOVs' framebuffers
//   clear    true: the frames are cleared on the way (the merged wavefront). false: a batch -- count 1, slot_base 0 -- whose frames the caller clears
//   list     null: pixels [pixel_offset, pixel_offset + pixel_count) of the context's pixel set. Else pixel_count entries x + y * width, every pixel folded
//            with its own sample count: needs clear, and moments (w is read from it)
//   moments  null, or the (M2_r, M2_g, M2_b, w) image of rt_set_noise_estimate, kept beside the RADIANCE mean
//   tiers    tiers.tiers null, or the firefly filter's tier images: `count` (2..8) pitched float4 images (sum w r, sum w g, sum w b, sum w), `plane`
//            pixels apart in one allocation; tier j takes the samples whose luminance lies around start * 8^j. Needs moments; mean, moments and final image come
//            out as without the tiers
// A kernel argument of its own: RtParams keeps its size.
#define RT_ACCUMULATE_GROUP 8
#define RT_FIREFLY_MAX_TIERS 8
#define RT_FIREFLY_BASE 8.0f
struct RtAccumulateGroup { int count; int first_sample[RT_ACCUMULATE_GROUP], sample_count[RT_ACCUMULATE_GROUP], slot_base[RT_ACCUMULATE_GROUP]; };
struct RtFireflyTiers { float4 * tiers; size_t plane; int count; float start; };
struct RtAccumulate { RtAccumulateGroup group; bool clear; const unsigned * list; int pixel_offset, pixel_count; float4 * moments; RtFireflyTiers tiers; };
void rt_launch_accumulate(const RtParams & p, const RtAccumulate & accumulate, hipStream_t stream);
// The noise estimate (kernel_noise_cells): one workgroup per RT_NOISE_CELL^2 pixels of width x height; mean and moments are pitched float4 images, pixel_map
// (pitched floats) may be null, the three cell arrays hold ceil(width / 16) * ceil(height / 16) entries, row-major.
#define RT_NOISE_CELL 16
void rt_launch_noise_cells(const float4 * mean, const float4 * moments, int width, int height, int pitch, float floor, float * pixel_map,
                           double * cell_sums, int * cell_counts, int * cell_nonfinite, hipStream_t stream);
// The firefly-robust estimate: the same kernel text beside the resolved image of the firefly filter. A participating pixel whose resolved .w >= 0
// and .w > held_fraction * fmaxf(luminance(mean), floor) is held: left out of sum and count, counted in cell_held, -3 in the map.
void rt_launch_noise_cells_robust(const float4 * mean, const float4 * moments, const float4 * resolved, int width, int height, int pitch, float floor, float held_fraction,
                                  float * pixel_map, double * cell_sums, int * cell_counts, int * cell_nonfinite, int * cell_held, hipStream_t stream);
// Adaptive sampling. select: kernel_select_cells, kernel_scan_cells and kernel_compact_cells on the cell arrays of rt_launch_noise_cells: flags
// (one byte per cell: bit 0 hot, bit 1 active), active_pixels and offsets (one int per cell), totals (3 ints: list length, hot cells, active cells), list (room for
// width * height entries, x + y * width each). rt_launch_generate_stream_list is the generate step of a submission over such a list.
// cell_held (the robust cells; null: the plain selection): held pixels count as judged, as non-finite ones do.
void rt_launch_select_cells(const double * cell_sums, const int * cell_counts, const int * cell_nonfinite, int width, int height, float threshold, int dilate,
                            unsigned char * flags, int * active_pixels, int * offsets, int * totals, unsigned * list, hipStream_t stream, const int * cell_held = nullptr);
void rt_launch_generate_stream_list(const RtParams & p, int sample_index, const unsigned * list, int pixel_count, int slot_base, int queue_offset, hipStream_t stream);
// The still-image denoiser (kernels_denoise.hip): prepare, `iterations` a-trous passes (0..6) of step 1, 2, 4, ..., the last of which finalizes;
// with 0 iterations prepare and a finalize kernel. any_valid: null, or one int the prepare kernel sets to 1 when a pixel is valid. All images are pitched float4; iv[0], iv[1] and guide are the filter's own (iv[1] is not touched below 2
// iterations), `out` receives the result, the rest is read only. Arguments of the kernels' own: RtParams keeps its size. tiled: the passes stage their taps in LDS.
// mark(user, k, stream), if given, is called before kernel k = 0 and after every kernel (k = 1 ...).
struct RtDenoiseArgs { int width, height, pitch, iterations; float sigma_l, sigma_n, sigma_z, depth_floor, albedo_floor; float eye[3]; };
struct RtDenoiseImages { const float4 * colour, * moments, * albedo, * normal, * position, * fallback; float4 * iv[2], * guide, * out; int * any_valid; };
void rt_launch_denoise(const RtDenoiseArgs & args, const RtDenoiseImages & images, bool tiled, hipStream_t stream,
                       void (*mark)(void * user, int kernel, hipStream_t stream) = nullptr, void * user = nullptr);
// The firefly filter (kernels_fireflies.hip): the tiers are filled by the accumulate step (RtAccumulate).
// The resolve: (mean, moments, tiers) -> out = (R / N, luminance(T - R) / N), and (fallback.rgb, -1) for a pixel that is not valid. All images are pitched float4;
// any_valid: null, or one int the kernel sets to 1 when a pixel is valid. tiled: the W of the tile's halo are staged in LDS; the plain kernel gives the same bits.
struct RtFireflyResolveArgs { int width, height, pitch, tiers; float start, support; };
struct RtFireflyResolveImages { const float4 * mean, * moments, * fallback, * tiers; size_t plane; float4 * out; int * any_valid; };
void rt_launch_fireflies_resolve(const RtFireflyResolveArgs & args, const RtFireflyResolveImages & images, bool tiled, hipStream_t stream);
// The exposure histogram (kernel_exposure_histogram): over the width x height pixels with w >= 1, the float32 exponent of luminance(mean) counted
// into histogram[0 .. 255], the pixels with luminance <= 0 into [RT_EXPOSURE_DARK], those with a mean that is not finite into [RT_EXPOSURE_NONFINITE]. The
// caller zeroes the RT_EXPOSURE_WORDS words; the kernel adds to them.
#define RT_EXPOSURE_BINS 256
#define RT_EXPOSURE_DARK 256
#define RT_EXPOSURE_NONFINITE 257
#define RT_EXPOSURE_WORDS 258
void rt_launch_exposure_histogram(const float4 * mean, const float4 * moments, int width, int height, int pitch, unsigned long long * histogram, hipStream_t stream);
// mark(user, k, stream), if given, is called before and after kernel k = 0 reproject, 1 variance, 2 a-trous (each pass), 3 finalize, 4 TAA, 5 TAA finalize
void rt_launch_svgf_taa(const RtParams & p, int sample_index, hipStream_t stream, void (*mark)(void * user, int svgf_kernel, hipStream_t stream) = nullptr, void * user = nullptr);
void rt_launch_random(const RtParams & p, int dimension, const unsigned * pixel_indices, int count, unsigned bounce, unsigned sample_index, float2 * out, hipStream_t stream);
// Test support: the software texture unit on explicit coordinates (rt_sample_texture / rt_sample_table / rt_sample_sky)
void rt_launch_sample_texture(const RtParams & p, int texture_index, int filter, const float * args, int count, float4 * out, hipStream_t stream);
void rt_launch_sample_table(const float * table, int nx, int ny, int nz, int dims, const float * coords, int count, float * out, hipStream_t stream);
void rt_launch_sample_sky(const RtParams & p, const float * directions, int count, float * out, hipStream_t stream);
// Test support: one BSDF's eval or sample on explicit probes (rt_bsdf_eval / rt_bsdf_sample); probe i uses material i of p.materials
#define RT_BSDF_PROBE_IN  24
#define RT_BSDF_PROBE_OUT 12
void rt_launch_bsdf_probe(const RtParams & p, int material_type, bool eval, const float * probes, int count, float * out, hipStream_t stream);
// Test support: nee_pick_light on explicit random numbers (rt_sample_lights); 4 floats in, RT_LIGHT_SAMPLE_OUT out per probe
void rt_launch_sample_lights(const RtParams & p, const float * probes, int count, bool use_lds, float * out, hipStream_t stream);
// Test support: nee_pick_delta and delta_light_sample on explicit probes (rt_sample_delta_lights); 4 floats in, RT_DELTA_SAMPLE_OUT out per probe
void rt_launch_sample_delta_lights(const RtParams & p, const float * probes, int count, float * out, hipStream_t stream);
// Fog volume: the shadow queue's attenuation pass -- the per-bounce loop's (the queue of `bounce`) and the merged wavefront's (the queue the
// material kernels of p.stream_iteration appended to) -- and the probe of the segment step (rt_fog_segments).
void rt_launch_fog_attenuate_shadows(const RtParams & p, int bounce, hipStream_t stream);
void rt_launch_fog_attenuate_shadows_stream(const RtParams & p, hipStream_t stream);
void rt_launch_fog_segments(const RtParams & p, const uint32_t * probes, int count, uint32_t * out, hipStream_t stream);
// Density grid. The two attenuation launchers above take their ..._grid kernels while p.fog_grid; rt_launch_fog_density_segments is the
// grid's segment step on rt_fog_segments' records; rt_launch_fog_mark_bricks fills the brick table of an uploaded grid (one workgroup per brick) and
// adds the number of empty bricks to *empty_count.
void rt_launch_fog_density_segments(const RtParams & p, const uint32_t * probes, int count, uint32_t * out, hipStream_t stream);
void rt_launch_fog_mark_bricks(const float * density, int nx, int ny, int nz, unsigned char * bricks, int * empty_count, hipStream_t stream);
// Test support: normal_map_perturb on explicit hits (rt_perturb_normals); RT_NORMAL_PROBE_IN floats in, 4 out per probe
void rt_launch_perturb_normals(const RtParams & p, int texture_index, const float * probes, int count, float * out, hipStream_t stream);
// Sky importance sampling (kernels_sky.hip). build: the three tables of RtParams from the sky; row_total: sky_height doubles, total: one double (the
// sum of all cell weights, read back by the host). sample / pdf: the device functions of rt_shading.h on explicit arguments (test support).
void rt_launch_sky_build(const float4 * sky, int width, int height, float * marginal_cdf, float * conditional_cdf, float * cell_pdf, double * row_total, double * total, hipStream_t stream);
void rt_launch_sample_sky_distribution(const RtParams & p, const float * uv, int count, float * out_xyz_pdf, hipStream_t stream);
void rt_launch_sky_pdf(const RtParams & p, const float * directions, int count, float * out_pdf, hipStream_t stream);
void rt_launch_integrate_luts(const RtParams & p, float * dielectric_dir_enter, float * dielectric_dir_leave, float * dielectric_enter, float * dielectric_leave,
                              float * conductor_dir, float * conductor, hipStream_t stream);
void rt_launch_pack_pixels(const RtParams & p, float4 * dst, int tile_pixels, int tile_first, int tile_stride, int tiles, hipStream_t stream);
void rt_launch_unpack_pixels(const RtParams & p, const float4 * src, int tile_pixels, int world, int tiles_per_rank, hipStream_t stream);
void rt_launch_pack_svgf(const RtParams & p, float4 * dst, int tile_pixels, int tile_first, int tile_stride, int tiles, hipStream_t stream);
void rt_launch_unpack_svgf(const RtParams & p, const float4 * src, int tile_pixels, int world, int tiles_per_rank, hipStream_t stream);
void rt_launch_stream_read(const float4 * src, size_t count, float * sink, hipStream_t stream);
// Counting variants: stats = 10 x u64 {closest: nodes, triangles, inst_xform, inst_ident, rays; shadow: same}
void rt_launch_trace_counting(const RtParams & p, int bounce, unsigned long long * stats, hipStream_t stream);
void rt_launch_trace_shadow_counting(const RtParams & p, int bounce, unsigned long long * stats, hipStream_t stream);
// Stand-alone trace on explicit ray arrays (rt_trace_rays / rt_trace_shadow_rays)
void rt_launch_trace_explicit(const RtParams & p, RtVec3SoA origin, RtVec3SoA direction, uint4 * hits, int ray_count, int * retired_counter, hipStream_t stream);
void rt_launch_trace_shadow_explicit(const RtParams & p, RtVec3SoA origin, RtVec3SoA direction, const float * max_distance, uint8_t * occluded, int ray_count, int * retired_counter, hipStream_t stream);
