// rt_context.h -- what the units of the C ABI share: the context and the structs it is made of, error handling, and the internal functions that
// cross a unit boundary. The units: rt_api.hip (context, frame state, results), rt_scene.hip (scene uploads and device builds), rt_render.hip (the slot
// scheduler and the render entry points), rt_stream.hip (the merged wavefront's host side), rt_noise.hip (noise estimate, adaptive sampling), rt_denoise.hip (denoised stills), rt_fireflies.hip (firefly filter),
// rt_exchange.hip (frame exchange of the tile split), rt_light_tree.hip (the light tree of next-event estimation), rt_probes.hip (kernel-level entry points). Private to csrc/.
#pragma once
#include "rt_types.h"

#include <cstddef>
#include <deque>
#include <string>
#include <vector>

// Everything one sample per pixel owns while it is in flight. Up to RT_MAX_SAMPLE_SLOTS samples
// are rendered concurrently (rt_set_samples_in_flight): consecutive rt_render_sample calls take the
// slots round-robin, each on its own stream, and only the accumulate step is ordered between them.
// Why: a wavefront pass is a chain of ~40 launches whose deep bounces are too small to fill 256 CUs
// and whose persistent trace launches each end in a tail; a second sample's kernels fill those holes.
#define RT_MAX_SAMPLE_SLOTS 8
#define RT_MAX_BATCH_SAMPLES 16

// The queues of one wavefront, `capacity` entries each: two trace queues (this bounce's and the next), one per material,
// one of shadow rays. Each scheduler owns one set (SampleSlot, PathStream); queues_allocate / queues_free handle a set.
struct WavefrontQueues {
	RtTraceBuffer trace[2] = { }; RtMaterialBuffer material[4] = { }; RtShadowBuffer shadow = { };
	size_t capacity = 0;
	bool allocated = false;
};

struct SampleSlot {
	bool created = false;
	hipStream_t stream = nullptr;      // the sample's launch chain
	hipStream_t side   = nullptr;      // shadow rays of bounce b, concurrent with the closest-hit trace of bounce b+1
	hipEvent_t ev_shaded = nullptr, ev_shadowed = nullptr, ev_done = nullptr, ev_frame_start = nullptr, ev_frame_end = nullptr;
	WavefrontQueues queues;
	RtBufferSizes * sizes = nullptr;
	int * ray_cursors = nullptr;
	void * spill[2] = { nullptr, nullptr };  // traversal stack spill of the closest-hit / shadow launch
	int * counter_totals = nullptr;          // 6 x RT_MAX_BOUNCES ints accumulated over batches
	RtBufferSizes * pinned_counters = nullptr;
	void * aov_framebuffer[RT_AOV_COUNT] = { };  // slots 1..: per-sample frame buffers (slot 0 uses ctx->aov_buffers[i][0])
	int aov_samples = 1;                         // samples per batch the frame buffers of this slot are sized for
	// SVGF g-buffers (normal+depth, mesh+triangle id, previous screen position) are written by the
	// bounce-0 kernels of a frame and read by its filter stage: one set per slot lets frame n+1 be
	// traced while frame n is filtered. Pixels that miss all geometry keep the value of the last
	// frame that hit something (the reference never clears them), so a frame starts from a copy of
	// its predecessor's set, taken as soon as that frame's bounce-0 shading is done (ev_gbuffers).
	void * gbuffers[3] = { };                    // slots 1..; slot 0 uses ctx->svgf_buffers[0..2]
	hipEvent_t ev_gbuffers = nullptr;
};

// Per-frame scene data (the TLAS and the five per-instance tables, rebuilt by Integrator::build_tlas for
// every frame of an animated scene) lives in a ring of versions: an upload fills the next version
// through pinned staging with an asynchronous copy, the kernels of later samples get its address (the
// parameter block is passed by value), samples already in flight keep reading theirs. No upload of this
// kind drains the pipeline; a version is only waited for when the ring wraps around onto a sample
// that still uses it.
#define RT_SCENE_VERSIONS 12
struct SceneRing {
	void * device[RT_SCENE_VERSIONS] = { };
	void * pinned[RT_SCENE_VERSIONS] = { };
	hipEvent_t copied[RT_SCENE_VERSIONS] = { };
	size_t capacity = 0;   // bytes allocated per version (grows only)
	size_t bytes = 0;      // bytes of the current version
	int current = -1;
	// Sample slots that have submitted work reading a version since it was last written. (A slot used to remember only the
	// version of its LAST submission: with the host several frames ahead of the device, an older submission still queued
	// on the same slot lost its claim and the ring wrapped around onto the version it was about to read -- found with 1 500
	// moving instances and 48 frames, tools/animation_bench.py: a TLAS overwritten under a running traversal.)
	unsigned users[RT_SCENE_VERSIONS] = { };
	hipEvent_t last_use[RT_SCENE_VERSIONS][RT_MAX_SAMPLE_SLOTS] = { }; // end of the slot's latest submission that reads the version
};

// ---- merged wavefront (RT_SCHEDULER_MERGED; the idea is described at RtStreamSlot in rt_types.h) -------------------
// Host side: ONE stream, one set of queues sized for `capacity` rays. A submission (one rt_render_samples call) gets a
// run of sample slots, generates its primary rays into the current trace queue and advances the wavefront by one
// iteration; it is complete -- accumulated into the shared accumulators, in submission order -- after the iteration in
// which it reaches its last bounce. What bounds the queues: every path in flight occupies at most one entry of a
// queue, paths only die, so (wavefront size reported by an earlier iteration) + (rays generated since) bounds the
// entries any queue can receive; the host stays RT_STREAM_RUN_AHEAD iterations ahead of the device at most, reads the
// reported sizes from pinned memory without blocking, and runs iterations without new samples while a new
// submission would not fit.
// Small submissions (the tiles of one rank of a multi-GPU split: 1/8 of a frame) would make small iterations again --
// launches that do not fill the machine, fixed costs per iteration that no longer disappear behind the rays. When the
// application pipelines frames (rt_set_frame_pipelining) a submission therefore generates its rays at once but the
// iteration is only enqueued when RT_STREAM_BATCH_PATHS paths have been generated for it (or RT_STREAM_MAX_BATCH
// submissions), so the iterations of a 1/8 split carry 8 frames and are as large as those of a whole frame. Anything that
// needs progress -- rt_advance, every call that flushes, a change of camera -- enqueues the iteration with what is there.
#define RT_STREAM_BATCH_PATHS     (1920 * 1080 * 4)
#define RT_STREAM_MAX_BATCH       8
#define RT_STREAM_PROGRESS_RING   64
#define RT_STREAM_RUN_AHEAD       4
#define RT_STREAM_TABLE_SNAPSHOTS 8
#define RT_STREAM_HISTORY_ROWS    4096
#define RT_STREAM_STATS_ROW       (RT_STAT_KINDS * RT_MAX_BOUNCES)   // ints per submission

struct StreamSubmission {
	int first_sample, sample_count, slot_base, ring, birth, last, paths;
	int range_offset, range_count, tile_pixels, tile_first, tile_stride;
	bool list = false;   // over the context's pixel list (rt_set_pixel_list): range_offset 0, range_count the list's length
};

struct PathStream {
	bool created = false;
	hipStream_t stream = nullptr;
	hipEvent_t ev_idle = nullptr;         // after the last completion enqueued so far: what main-stream consumers wait for
	WavefrontQueues queues;
	RtStreamControl * control = nullptr;
	RtStreamTable * table_device = nullptr;
	RtStreamTable table_host;             // what the device table will hold once the copies enqueued so far have run
	RtStreamTable * table_staging = nullptr; hipEvent_t table_copied[RT_STREAM_TABLE_SNAPSHOTS] = { }; int table_next = 0;
	void * spill = nullptr;
	void * aov_framebuffer[RT_AOV_COUNT] = { }; int frame_slots = 0;   // per-sample frames, one per sample slot
	void * gbuffers[3] = { };             // SVGF: one g-buffer set (float4, int2, float2 per pixel) per sample slot
	int last_gbuffer_slot = -1;           // the set of the frame submitted last, if that was a frame of this wavefront
	bool slot_used[RT_STREAM_SAMPLE_SLOTS] = { };
	int next_slot = 0, next_ring = 0;
	int iteration = 0;                    // the next iteration to enqueue
	int base_iteration = 0;               // nothing generated before it is still in flight
	std::deque<StreamSubmission> in_flight;
	int pending = 0; long long pending_paths = 0;   // the newest submissions: rays generated, iteration not enqueued yet
	// ... their slot-table entries and statistics rows reach the device ONCE, with the iteration that first needs them (one copy and the advance launch instead
	// of a copy and a fill per submission: a rank of an 8-GPU split spent 0.1 ms of its 5.4 ms burst on five such pairs, profiles/r05_rank_timeline.txt)
	bool table_dirty = false; int reset_ring_first = 0, reset_ring_count = 0;
	int * progress = nullptr;             // pinned [RING][2] = { iteration, wavefront size }, written by kernel_stream_advance
	hipEvent_t iteration_done[RT_STREAM_PROGRESS_RING] = { };
	int generated[RT_STREAM_PROGRESS_RING] = { };
	int known_iteration = -1; long long known_size = 0;
	unsigned long long submissions_completed = 0;
	int * stats_host = nullptr;           // pinned [RT_STREAM_SUBMISSIONS][RT_STREAM_STATS_ROW]
	hipEvent_t ev_begin[RT_STREAM_SUBMISSIONS] = { }, ev_end[RT_STREAM_SUBMISSIONS] = { };
	int last_completed_ring = -1;
};

struct rt_context {
	int device = 0;
	hipStream_t stream = nullptr;      // "main": uploads, read-backs, pack/unpack, kernel-level entry points
	hipEvent_t ev_main = nullptr, ev_interop = nullptr;
	std::string error;

	SampleSlot slots[RT_MAX_SAMPLE_SLOTS];
	// (Two such wavefronts taking the submissions in turns, their traversal launches serialised by an event chain so that
	// one pipeline's sort / shade kernels would run beside the other's traversal, were built and measured: 3.23 ms per step
	// against 3.02 ms with one -- the persistent traversal launch holds every wave slot of the machine until its queue is
	// drained, nothing can start beside it. Removed; profiles/r02_two_pipelines_*.)
	PathStream path_stream;
	unsigned long long * stream_history = nullptr; int stream_history_rows = 0;   // pinned [ROWS][10]: trace statistics after each traversal launch
	int scheduler = RT_SCHEDULER_MERGED;
	bool last_render_merged = false;
	bool defer_filter = false;         // rt_render_sample_unfiltered: an SVGF frame stops before its filter stage (tile split)
	bool frame_pipelining = false;     // rt_pack_pixels / rt_unpack_pixels follow the completed submissions only (rt_set_frame_pipelining)
	long long stream_batch_paths = 0;  // paths the submissions of one iteration may bring (rt_set_stream_batch); 0: RT_STREAM_BATCH_PATHS
	int samples_in_flight = 3;
	unsigned render_counter = 0;
	int last_slot = -1;

	RtParams params;               // zero-initialised in rt_create
	std::vector<void *> owned;     // every hipMalloc'd pointer, freed in rt_destroy

	// named allocations that get replaced on re-upload
	void * triangles = nullptr, * triangle_positions = nullptr, * bvh8_nodes = nullptr, * bvh2_nodes = nullptr, * bvh4_nodes = nullptr;
	size_t tlas_node_bytes = 80;        // what the current TLAS version was uploaded as (80 CWBVH, 32 binary, 128 4-wide)
	int lowest_blas_root = 0x7fffffff;  // over the instances uploaded last: the node slots below it are free for the TLAS copy of the merged wavefront
	unsigned long long tlas_version = 0, tlas_version_in_nodes = ~0ull;   // the merged wavefront traces a copy of the TLAS inside the BLAS node array (stream_sync_tlas)
	bool expand_bc1 = true;   // rt_set_texture_expansion: BC1 textures are decoded once, at upload (rt_types.h: RT_TEXTURE_BC1_EXPANDED)
	size_t texture_bytes = 0; // what rt_upload_textures holds on the device
	std::vector<float> build_boxes; size_t build_boxes_first = 0;   // rt_set_build_boxes: consumed by the next rt_build_geometry
	size_t bvh4_node_count = 0;
	size_t bvh8_node_count = 0, bvh2_node_count = 0, triangle_count = 0;
	size_t mesh_count = 0;
	SceneRing tlas_ring, instance_ring, light_ring;
	int * device_tlas_order = nullptr, * device_tlas_node_count = nullptr; // current TLAS built by rt_build_tlas (else null)
	hipEvent_t ev_scene = nullptr;  // the last asynchronous scene upload on the main stream
	void * material_types = nullptr, * materials = nullptr, * media = nullptr;
	size_t medium_count = 0;                   // entries of rt_upload_media's table (rt_sort_rays checks medium ids against it)
	bool has_material[4] = { false, false, false, false };
	std::vector<uint8_t> material_type_list;   // what rt_upload_materials uploaded (rt_upload_material_normal_maps checks against it)
	void * material_normal_maps = nullptr;     // int per material (rt_upload_material_normal_maps)
	std::vector<int> texture_formats;          // the device format of every texture of rt_upload_textures
	std::vector<RtTexture> texture_records;    // ... and its record (device pointer, size), as uploaded
	// opacity masks (rt_upload_material_opacity): the two device tables and the bits of all masks in one allocation; host copies for rt_read_material_opacity
	void * material_opacity = nullptr, * opacity_masks = nullptr, * opacity_bits = nullptr;
	std::vector<int> material_opacity_list; std::vector<RtOpacityMask> opacity_mask_list;
	bool has_lights = false;
	void * texture_table = nullptr; std::vector<void *> texture_data;
	void * pmj = nullptr, * blue_noise = nullptr;
	void * sky = nullptr;
	// sky importance sampling (rt_set_sky_sampling; kernels_sky.hip): the tables are built at the first render that wants them after rt_set_sky
	float sky_sampling = 0.0f;               // 0: off (the reference's estimator); (0, 1]: the sky's share of the light samples when emitters exist
	void * sky_tables = nullptr;             // floats: marginal CDF [H], conditional CDFs [H * W], cell pdfs [H * W]
	void * sky_table_sums = nullptr;         // doubles: row totals [H], total [1]
	bool sky_tables_ready = false;
	double sky_total = 0.0;                  // the sum of the cell weights (0: a black sky, sampling stays inactive; not finite: an error)
	// delta emitters (rt_upload_delta_lights): one device allocation (the records, then their CDF) and the host's copy of both
	// (rt_read_delta_lights); the share of the upload. What a render makes of it (RtParams::delta_nee_share) is settled by sky_sampling_prepare.
	void * delta_lights = nullptr;
	std::vector<float> delta_light_records, delta_light_cdf;
	float delta_light_share = 0.0f;
	// fog volume (rt_set_fog_volume): what the caller set, as rt_get_fog_volume returns it; RtParams::fog_* hold what the kernels read
	bool fog_set = false;
	rt_fog_volume fog = { };
	// its density grid (rt_set_fog_density), state of its own beside the volume: the device copy, the brick table, what
	// rt_get_fog_density_info reports. fog_refresh_active (rt_api.hip) settles RtParams::fog_active and fog_grid from both.
	bool fog_grid_set = false;
	int fog_grid_dims[3] = { 0, 0, 0 }, fog_grid_bricks = 0, fog_grid_empty_bricks = 0;
	float fog_grid_max = 0.0f;
	void * fog_density = nullptr, * fog_bricks = nullptr;
	// light tree (rt_set_light_tree): the wish; the spans of the light tables uploaded last (the leaves are counted from them); the one allocation
	// behind RtParams::light_tree, which says whether a tree is built
	bool light_tree_on = false, light_tree_fog_warned = false;
	bool light_tree_dirty = false;   // an upload the tree depends on has come since it was built (geometry, instances, TLAS build, materials, light tables): light_tree_refresh rebuilds
	std::vector<int32_t> light_spans;
	void * light_tree_memory = nullptr;
	void * luts[6] = { }; bool luts_ready = false;
	int bvh_width = 8;

	// frame resources
	void * aov_buffers[RT_AOV_COUNT][2] = { };
	void * final_image = nullptr;
	void * svgf_buffers[16] = { }; bool svgf_allocated = false;   // [15]: RtParams::svgf_young_pixels
	size_t frame_pixels = 0; // pitch * height
	// noise estimate (rt_set_noise_estimate): (M2_r, M2_g, M2_b, w) per pixel beside the RADIANCE accumulator, kept by the ..._moments
	// accumulate kernels while the estimate is on and SVGF is off; null while it is off (or before rt_resize)
	bool noise_estimate = false;
	void * noise_moments = nullptr;
	// adaptive sampling (rt_select_active_cells): the pixels of the active cells, x + y * screen_width each, pixel_list_count of them in a buffer of
	// frame_pixels entries -- allocated at the first selection, freed by rt_resize and with the estimate, dropped whenever the moments image is zeroed.
	// pixel_list_on (rt_set_pixel_list): render calls cover the list.
	void * pixel_list = nullptr;
	int pixel_list_count = 0;
	bool pixel_list_selected = false, pixel_list_on = false;

	// still-image denoiser (rt_denoise): three (I, v) images -- two of them a run's ping-pong pair, the third the result of the last successful
	// run (denoise_result, -1: none), a run's last kernel writing into the pair's free image -- and the guide image; a flag the prepare kernel raises when a pixel is valid. Allocated at
	// the first rt_denoise, freed by rt_resize.
	void * denoise_images[3] = { }, * denoise_guide = nullptr; int * denoise_any_valid = nullptr;
	int denoise_result = -1;
	int denoise_source = RT_DENOISE_SOURCE_MEAN;   // rt_set_denoise_source

	// firefly filter (rt_set_firefly_cascade): firefly.tiers images of (sum w rgb, sum w), frame_pixels apart in one allocation, kept by the ..._cascade
	// accumulate kernels beside the moments image and zeroed whenever that image is; they exist exactly while the cascade is on, the moments image exists and the
	// frame has a size. firefly_resolved: the result image of rt_resolve_fireflies (allocated at the first call, freed by rt_resize); it is current while
	// firefly_resolved_at == folds, the number of accumulate launches and zeroings the frame has seen.
	bool firefly_on = false;
	rt_firefly_params firefly = { };
	void * firefly_tiers = nullptr, * firefly_resolved = nullptr; int * firefly_any_valid = nullptr;
	unsigned long long folds = 1, firefly_resolved_at = 0;
	// firefly-robust noise estimate (rt_set_noise_robust): the held fraction while rt_select_active_cells selects from the robust cells, else 0.
	// On only while the cascade is.
	float noise_robust = 0.0f;

	// frame exchange of the tile split (rt_comm_*): this context's rank in a group of `world` contexts, each on its own GPU
	// (RCCL communicator) or, for tests on one GPU, several in one process (peer copies)
	struct FrameExchange {
		int rank = 0, world = 1;
		void * comm = nullptr;                       // ncclComm_t
		std::vector<rt_context *> peers;             // in-process transport: all contexts of the group, by rank
		float4 * packed = nullptr, * gathered = nullptr; size_t packed_pixels = 0;   // per pixel `channels` float4
		hipEvent_t ev_packed = nullptr, ev_copied = nullptr;
	} exchange;

	int * explicit_retired = nullptr;
	int * pixel_query_out = nullptr;   // device { mesh_id, triangle_id }
	int batch_size_request = 0;              // 0 = whole frame (288 GB of HBM: no reason to cut a frame into pieces)
	int pixel_offset = 0, pixel_count = -1;  // -1 = whole frame

	rt_counters last_counters;
	bool profiling = false;          // mode 1: per-stage events, one sample at a time
	bool launch_timing = false;      // mode 2: events around every traversal launch, concurrency untouched
	bool launch_timing_all = false;  // mode 3: ... and around every other launch of the merged wavefront
	bool time_this_sample = false;
	std::vector<hipEvent_t> span_events; std::vector<int> span_kinds; size_t span_used = 0; // mode 2: [begin, end] pairs
	bool trace_statistics = false;
	unsigned long long * trace_stats = nullptr;    // device, 10 x u64
	unsigned long long host_trace_stats[10] = { };
	std::vector<hipEvent_t> stage_events; std::vector<int> stage_kinds; size_t stage_used = 0;
};

// SVGF g-buffers: a set is three images, bytes per pixel: normal + depth (float4), mesh + triangle id (int2), previous screen position (float2).
// gbuffer_bytes: member i of one set at the current frame size. stream_gbuffer: member i of the set of the merged wavefront's sample slot `slot`
// (PathStream::gbuffers[i] holds frame_slots sets, one behind the other).
static const size_t gbuffer_pixel_bytes[3] = { 16, 8, 8 };
inline size_t gbuffer_bytes(const rt_context * ctx, int i) { return ctx->frame_pixels * gbuffer_pixel_bytes[i]; }
inline void * stream_gbuffer(const rt_context * ctx, int i, int slot) { return (char *)ctx->path_stream.gbuffers[i] + gbuffer_bytes(ctx, i) * size_t(slot); }

// Internal functions that cross a unit boundary, by the unit that defines them (where each is described). Hidden: the library exports the C ABI only.
#pragma GCC visibility push(hidden)
// rt_api.hip
int fail(rt_context * ctx, int status, const char * fmt, ...);
int device_alloc(rt_context * ctx, void ** out, size_t bytes);
void device_free(rt_context * ctx, void * p);
hipError_t quiesce(rt_context * ctx);
hipError_t main_waits_for_samples(rt_context * ctx);
int check_ready(rt_context * ctx, const char * caller, int needs);
int resolve_pixel_range(rt_context * ctx, const char * caller, int * out_offset, int * out_count);
// rt_scene.hip
int mark_scene_versions_in_use(rt_context * ctx, int slot_index, hipStream_t st);
int sky_tables_build(rt_context * ctx, const char * caller);
int sky_sampling_prepare(rt_context * ctx, const char * caller);
int ensure_luts(rt_context * ctx);
// rt_light_tree.hip
int light_tree_leaves_allowed(rt_context * ctx, const char * caller, const int32_t * spans, size_t entries);
int light_tree_refresh(rt_context * ctx, const char * caller);
void light_tree_fog_warning(rt_context * ctx);
// rt_render.hip
void use_queues(RtParams & p, const WavefrontQueues & q);
int queues_allocate(rt_context * ctx, WavefrontQueues & q, size_t entries);
void queues_free(rt_context * ctx, WavefrontQueues & q);
int ensure_slot(rt_context * ctx, int index);
RtParams slot_params(const rt_context * ctx, const SampleSlot & slot, int index);
int ensure_queues(rt_context * ctx, int slot_index = 0, size_t pixels = 0);
void stage_mark(rt_context * ctx, int kind, hipStream_t stream);
void span_mark(rt_context * ctx, int kind, hipStream_t stream);
// rt_stream.hip
int stream_create(rt_context * ctx);
void stream_destroy(rt_context * ctx);
void stream_save_gbuffers(rt_context * ctx);
void stream_release_frames(rt_context * ctx);
RtParams stream_params(const rt_context * ctx, int iteration);
int stream_sync_tlas(rt_context * ctx);
void stream_launch_generate(const RtParams & pg, int first_sample, const unsigned * list, int range_offset, int range_count, int slot_base, int queue_offset, hipStream_t st, int * order2);
int stream_enqueue_iteration(rt_context * ctx);
int stream_launch_pending(rt_context * ctx);
hipError_t stream_flush(rt_context * ctx);
int stream_submit(rt_context * ctx, int sample_index, int sample_count, int range_offset, int range_count);
// rt_noise.hip
void pixel_list_drop(rt_context * ctx);
void pixel_list_free(rt_context * ctx);
int sync_noise_moments(rt_context * ctx);
int noise_moments_reset(rt_context * ctx);
float4 * noise_moments_for(const rt_context * ctx, const RtParams & p);
struct NoiseRobust { const float4 * resolved; float held_fraction; int32_t * cell_held; int64_t * held_pixels; };   // the robust forms of the two sequences below
int noise_estimate_images(rt_context * ctx, const char * caller, const float4 * mean, const float4 * moments, float floor, rt_noise_estimate * out,
                          double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, size_t cell_capacity, float * pixel_map, const NoiseRobust * robust = nullptr);
int selection_arguments(rt_context * ctx, const char * caller, float floor, float threshold, int dilate);
int held_fraction_argument(rt_context * ctx, const char * caller, float held_fraction);
int select_cells_images(rt_context * ctx, const char * caller, const float4 * mean, const float4 * moments, float floor, float threshold, int dilate, unsigned * list,
                        rt_cell_selection * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, uint8_t * cell_flags, size_t cell_capacity,
                        const NoiseRobust * robust = nullptr);
// rt_denoise.hip
void denoise_free(rt_context * ctx);
int denoise_arguments(rt_context * ctx, const char * caller, const rt_denoise_params * params);
// rt_fireflies.hip
int sync_firefly_tiers(rt_context * ctx);
int firefly_tiers_zero(rt_context * ctx);
void firefly_free(rt_context * ctx);
RtFireflyTiers firefly_tiers_for(rt_context * ctx, const RtParams & p);
int firefly_arguments(rt_context * ctx, const char * caller, int tiers, float start, float support);
int firefly_resolve_frame(rt_context * ctx, const char * caller, float support, bool tiled, float * kernel_ms);
int exposure_measure_images(rt_context * ctx, const char * caller, const float4 * mean, const float4 * moments, int width, int height, int pitch, rt_exposure * out, uint64_t * histogram256);
#pragma GCC visibility pop

#define RT_HIP(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(ctx, RT_ERROR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)
#define RT_REQUIRE(ctx, cond, msg) do { if (!(cond)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s", msg); } while (0)

// What a render or trace entry point needs uploaded before it launches anything. NEED_SCENE reports missing geometry
// and missing instances apart; NEED_SCENE_JOINT (the explicit-ray entry points) reports them as one.
enum { NEED_SCENE = 1, NEED_SCENE_JOINT = 2, NEED_MATERIALS = 4, NEED_RNG = 8, NEED_SKY = 16, NEED_FRAME = 32 };

// the `kind` of stage_mark (rt_set_profiling(ctx, 1))
enum { STAGE_GENERATE = 0, STAGE_TRACE, STAGE_SORT, STAGE_SHADE, STAGE_SHADOW, STAGE_POST, STAGE_END };
// what a [begin, end] event pair of rt_set_profiling(ctx, 2 / 3) brackets (the `kind` of rt_get_launch_timings)
enum { SPAN_TRACE = RT_TIMING_TRACE, SPAN_SHADOW = RT_TIMING_SHADOW, SPAN_SORT = RT_TIMING_SORT, SPAN_GENERATE = RT_TIMING_GENERATE, SPAN_ACCUMULATE = RT_TIMING_ACCUMULATE,
       SPAN_MATERIAL = RT_TIMING_MATERIAL_0, SPAN_SVGF = RT_TIMING_SVGF_REPROJECT };

// The queue records of the launch probes (include/gpu_raytracer_amd.h: RT_SORT_TRACE_WORDS, RT_SORT_MATERIAL_WORDS, RT_SHADE_SHADOW_WORDS), described ONCE: which
// array of the queue -- the pointer `member` bytes into the buffer struct -- holds words [word, word + words) of an entry's record. Host side only; the probes'
// staging and read-back (rt_probes.hip: Probe::queue, Probe::queue_back) and their entry checks go by these tables, so a new queue member is one line here.
struct RecordField { size_t member; int word, words; };
#define RT_RECORD_FIELD(B, m, word, words) { offsetof(B, m), word, words }
#define RT_RECORD_VEC3(B, m, word) RT_RECORD_FIELD(B, m.x, word, 1), RT_RECORD_FIELD(B, m.y, (word) + 1, 1), RT_RECORD_FIELD(B, m.z, (word) + 2, 1)
template<typename B> struct RecordLayout;
template<> struct RecordLayout<RtTraceBuffer> {   // words 18 and 19 are padding
	static constexpr int words = RT_SORT_TRACE_WORDS;
	static constexpr RecordField fields[] = { RT_RECORD_VEC3(RtTraceBuffer, origin, 0), RT_RECORD_VEC3(RtTraceBuffer, direction, 3), RT_RECORD_FIELD(RtTraceBuffer, hits, 6, 4),
		RT_RECORD_FIELD(RtTraceBuffer, pixel_index_and_flags, 10, 1), RT_RECORD_VEC3(RtTraceBuffer, throughput, 11), RT_RECORD_FIELD(RtTraceBuffer, last_pdf, 14, 1),
		RT_RECORD_FIELD(RtTraceBuffer, medium, 15, 1), RT_RECORD_FIELD(RtTraceBuffer, cone_angle, 16, 1), RT_RECORD_FIELD(RtTraceBuffer, cone_width, 17, 1) };
};
template<> struct RecordLayout<RtMaterialBuffer> {   // words 14 and 15 are padding
	static constexpr int words = RT_SORT_MATERIAL_WORDS;
	static constexpr RecordField fields[] = { RT_RECORD_VEC3(RtMaterialBuffer, direction, 0), RT_RECORD_FIELD(RtMaterialBuffer, hits, 3, 4), RT_RECORD_FIELD(RtMaterialBuffer, pixel_index_and_flags, 7, 1),
		RT_RECORD_VEC3(RtMaterialBuffer, throughput, 8), RT_RECORD_FIELD(RtMaterialBuffer, medium, 11, 1), RT_RECORD_FIELD(RtMaterialBuffer, cone_angle, 12, 1),
		RT_RECORD_FIELD(RtMaterialBuffer, cone_width, 13, 1) };
};
template<> struct RecordLayout<RtShadowBuffer> {
	static constexpr int words = RT_SHADE_SHADOW_WORDS;
	static constexpr RecordField fields[] = { RT_RECORD_VEC3(RtShadowBuffer, origin, 0), RT_RECORD_VEC3(RtShadowBuffer, direction, 3), RT_RECORD_FIELD(RtShadowBuffer, max_distance, 6, 1),
		RT_RECORD_FIELD(RtShadowBuffer, illumination_and_pixel_index, 7, 4) };
};
// the first word of the array `member` (an offsetof into B) in B's record
template<typename B> constexpr int record_word(size_t member) {
	for (const RecordField & f : RecordLayout<B>::fields) if (f.member == member) return f.word;
	return -1;
}
// every array of the buffer is described exactly once, inside the record, and no word belongs to two arrays
template<typename B> constexpr bool record_layout_sound() {
	unsigned long long words = 0, members = 0; size_t count = 0;
	for (const RecordField & f : RecordLayout<B>::fields) {
		const unsigned long long member = 1ull << (f.member / sizeof(void *));
		if (f.member % sizeof(void *) || f.member >= sizeof(B) || (members & member) || f.words < 1) return false;
		members |= member; count++;
		for (int w = f.word; w < f.word + f.words; w++) {
			if (w < 0 || w >= RecordLayout<B>::words || (words >> w & 1)) return false;
			words |= 1ull << w;
		}
	}
	return count * sizeof(void *) == sizeof(B);
}
static_assert(record_layout_sound<RtTraceBuffer>() && record_layout_sound<RtMaterialBuffer>() && record_layout_sound<RtShadowBuffer>(), "a queue record's table does not match its buffer");
