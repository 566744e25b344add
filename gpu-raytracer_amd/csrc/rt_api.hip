// rt_api.hip -- the C ABI of include/gpu_raytracer_amd.h: the context itself (create, destroy, errors, allocation, what waits for what), the frame
// state (size, camera, config, pixel range, the setters and getters) and the read-backs. The rest of the ABI: scene uploads and device builds in
// rt_scene.hip, the render entry points and the slot scheduler in rt_render.hip, the merged wavefront's host side in rt_stream.hip, the noise
// estimate and adaptive sampling in rt_noise.hip, the kernel-level entry points in rt_probes.hip, the frame exchange of the tile split in
// rt_exchange.hip; rt_context.h is what they share.
// One rt_context owns one HIP device: a stream, every device buffer, and the RtParams block
// handed to the kernels by value. It plays the role of the reference's Device/ layer plus the
// device half of Integrator/Pathtracer (buffer ownership, `buffer_sizes` handling, the
// wavefront launch loop of Pathtracer::render, Pathtracer.cpp:738-855).
#include "rt_context.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>

static thread_local std::string g_global_error;

int fail(rt_context * ctx, int status, const char * fmt, ...) {
	char buffer[512];
	va_list args; va_start(args, fmt); vsnprintf(buffer, sizeof(buffer), fmt, args); va_end(args);
	if (ctx) ctx->error = buffer;
	g_global_error = buffer;
	return status;
}

int device_alloc(rt_context * ctx, void ** out, size_t bytes) {
	if (bytes == 0) bytes = 16;
	RT_HIP(ctx, hipMalloc(out, bytes));
	ctx->owned.push_back(*out);
	return RT_OK;
}
void device_free(rt_context * ctx, void * p) {
	if (!p) return;
	for (size_t i = 0; i < ctx->owned.size(); i++) if (ctx->owned[i] == p) { ctx->owned[i] = ctx->owned.back(); ctx->owned.pop_back(); break; }
	(void)hipFree(p);
}

// Wait for everything the context has in flight: the merged wavefront (run to completion first), every sample
// slot (and its side stream), then main.
hipError_t quiesce(rt_context * ctx) {
	if (ctx->path_stream.created) {
		hipError_t e = stream_flush(ctx);                            if (e != hipSuccess) return e;
		e = hipStreamSynchronize(ctx->path_stream.stream);           if (e != hipSuccess) return e;
	}
	for (SampleSlot & slot : ctx->slots) if (slot.created) {
		hipError_t e = hipStreamSynchronize(slot.side);   if (e != hipSuccess) return e;
		e = hipStreamSynchronize(slot.stream);            if (e != hipSuccess) return e;
	}
	return hipStreamSynchronize(ctx->stream);
}

// Main-stream work that reads or writes frame results is ordered after every sample already submitted.
hipError_t main_waits_for_samples(rt_context * ctx) {
	if (ctx->path_stream.created) {
		if (!ctx->frame_pipelining) { hipError_t e = stream_flush(ctx); if (e != hipSuccess) return e; }
		hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->path_stream.ev_idle, 0); if (e != hipSuccess) return e;
	}
	for (SampleSlot & slot : ctx->slots) if (slot.created) {
		hipError_t e = hipStreamWaitEvent(ctx->stream, slot.ev_done, 0); if (e != hipSuccess) return e;
	}
	return hipSuccess;
}

// the node array of the selected BVH type has been uploaded
static bool bvh_nodes_present(const rt_context * ctx) {
	const RtParams & p = ctx->params;
	return ctx->bvh_width == 8 ? p.bvh8_nodes != nullptr : (ctx->bvh_width == 4 ? p.bvh4_nodes != nullptr : p.bvh2_nodes != nullptr);
}

int check_ready(rt_context * ctx, const char * caller, int needs) {
	const RtParams & p = ctx->params;
	if ((needs & (NEED_SCENE | NEED_SCENE_JOINT)) && p.opacity_active && ctx->bvh_width != 8)
		return fail(ctx, RT_ERROR_INVALID_ARG, "%s: opacity masks are uploaded (rt_upload_material_opacity) and only the CWBVH kernels test them; rt_set_bvh_type is %d", caller, ctx->bvh_width);
	const bool geometry = p.triangles && bvh_nodes_present(ctx), instances = p.mesh_bvh_root_indices != nullptr;
	const struct { int need; bool missing; const char * what; } checks[] = {
		{ NEED_SCENE,       !geometry,                        "geometry not uploaded" },
		{ NEED_SCENE,       !instances,                       "instances not uploaded" },
		{ NEED_SCENE_JOINT, !geometry || !instances,          "geometry / instances not uploaded" },
		{ NEED_MATERIALS,   !p.materials,                     "materials not uploaded" },
		{ NEED_RNG,         !p.pmj_samples || !p.blue_noise,  "RNG tables not uploaded" },
		{ NEED_SKY,         !p.sky,                           "sky not set" },
		{ NEED_FRAME,       ctx->frame_pixels == 0,           "rt_resize was not called" },
	};
	for (const auto & c : checks) if ((needs & c.need) && c.missing) return fail(ctx, RT_ERROR_NOT_READY, "%s: %s", caller, c.what);
	return RT_OK;
}

// The pixels a render call covers: rt_set_pixel_range's (offset, count) -- the rest of the frame for a negative count --
// or, in tile mode, local pixels 0 .. count-1, which rt_map_pixel maps to this context's tiles.
int resolve_pixel_range(rt_context * ctx, const char * caller, int * out_offset, int * out_count) {
	const RtParams & p = ctx->params;
	const int frame = p.screen_width * p.screen_height;
	int offset = ctx->pixel_offset, count = ctx->pixel_count < 0 ? frame - offset : ctx->pixel_count;
	if (ctx->pixel_list_on) { offset = 0; count = ctx->pixel_list_count; }   // entries 0 .. count-1 of the selected list (rt_set_pixel_list)
	else if (p.tile_pixels > 0) {
		int tiles_total = (frame + p.tile_pixels - 1) / p.tile_pixels;
		int owned = p.tile_first < tiles_total ? (tiles_total - p.tile_first + p.tile_stride - 1) / p.tile_stride : 0;
		offset = 0; count = owned * p.tile_pixels;
		int last_tile = p.tile_first + (owned - 1) * p.tile_stride;
		if (owned > 0 && last_tile == tiles_total - 1) count -= tiles_total * p.tile_pixels - frame; // clipped last tile
	} else if (offset + count > frame) return fail(ctx, RT_ERROR_OUT_OF_RANGE, "%s: pixel range [%d,%d) exceeds the %d pixel frame", caller, offset, offset + count, frame);
	*out_offset = offset; *out_count = count;
	return RT_OK;
}

// ---- frame state ---------------------------------------------------------------------------------------

static int sync_aovs(rt_context * ctx) {
	size_t bytes = ctx->frame_pixels * 16;
	for (int i = 0; i < RT_AOV_COUNT; i++) {
		bool enabled = (ctx->params.config.aov_mask >> i) & 1u;
		bool allocated = ctx->aov_buffers[i][0] != nullptr;
		if (enabled && !allocated && bytes) {
			RT_HIP(ctx, quiesce(ctx));
			stream_release_frames(ctx);
			for (int k = 0; k < 2; k++) { // [0]: slot 0's per-sample frame buffer(s), [1]: the accumulator
				size_t n = k == 0 ? bytes * ctx->slots[0].aov_samples : bytes;
				int s = device_alloc(ctx, &ctx->aov_buffers[i][k], n); if (s) return s;
				RT_HIP(ctx, hipMemset(ctx->aov_buffers[i][k], 0, n));
			}
			// (the filter's mirror of the radiance accumulators' variances starts from the same zeros)
			if ((i == RT_AOV_RADIANCE_DIRECT || i == RT_AOV_RADIANCE_INDIRECT) && ctx->svgf_buffers[13]) RT_HIP(ctx, hipMemset(ctx->svgf_buffers[13], 0, ctx->frame_pixels * 8));
			for (int k = 1; k < RT_MAX_SAMPLE_SLOTS; k++) if (ctx->slots[k].created) { // per-sample frame buffers of the other slots
				int s = device_alloc(ctx, &ctx->slots[k].aov_framebuffer[i], bytes * ctx->slots[k].aov_samples); if (s) return s;
				RT_HIP(ctx, hipMemset(ctx->slots[k].aov_framebuffer[i], 0, bytes * ctx->slots[k].aov_samples));
			}
		} else if (!enabled && allocated) {
			RT_HIP(ctx, quiesce(ctx));
			stream_release_frames(ctx);
			for (int k = 0; k < 2; k++) { device_free(ctx, ctx->aov_buffers[i][k]); ctx->aov_buffers[i][k] = nullptr; }
			for (int k = 1; k < RT_MAX_SAMPLE_SLOTS; k++) { device_free(ctx, ctx->slots[k].aov_framebuffer[i]); ctx->slots[k].aov_framebuffer[i] = nullptr; }
		}
		ctx->params.aovs[i].framebuffer = (float4 *)ctx->aov_buffers[i][0];
		ctx->params.aovs[i].accumulator = (float4 *)ctx->aov_buffers[i][1];
	}
	return RT_OK;
}

static int sync_svgf(rt_context * ctx) {
	bool want = ctx->params.config.enable_svgf != 0;
	if (want == ctx->svgf_allocated || ctx->frame_pixels == 0) return RT_OK;
	if (want) {
		// gbuffers (float4, int2, float2), moment, history x5 (length is int), taa x2, decoded normal + depth, variance pairs x2
		const size_t elem[15] = { gbuffer_pixel_bytes[0], gbuffer_pixel_bytes[1], gbuffer_pixel_bytes[2], 16, 4, 16, 16, 16, 16, 16, 16, 16, 8, 8, 16 };
		for (int i = 0; i < 15; i++) {
			int s = device_alloc(ctx, &ctx->svgf_buffers[i], ctx->frame_pixels * elem[i]); if (s) return s;
			RT_HIP(ctx, hipMemsetAsync(ctx->svgf_buffers[i], 0, ctx->frame_pixels * elem[i], ctx->stream));
		}
		{ int s = device_alloc(ctx, &ctx->svgf_buffers[15], (RT_SVGF_YOUNG_HEADER + ctx->frame_pixels) * 4); if (s) return s; RT_HIP(ctx, hipMemsetAsync(ctx->svgf_buffers[15], 0, RT_SVGF_YOUNG_HEADER * 4, ctx->stream)); }
		for (int k = 1; k < RT_MAX_SAMPLE_SLOTS; k++) if (ctx->slots[k].created) for (int i = 0; i < 3; i++) {
			int s = device_alloc(ctx, &ctx->slots[k].gbuffers[i], gbuffer_bytes(ctx, i)); if (s) return s;
			RT_HIP(ctx, hipMemsetAsync(ctx->slots[k].gbuffers[i], 0, gbuffer_bytes(ctx, i), ctx->stream));
		}
		// The filter keeps (direct.w, indirect.w) of the radiance accumulators mirrored in svgf_variance[1] and writes both only where it
		// filters (not at sky pixels). The mirror starts at zero, so the accumulators' .w have to: radiance accumulated WITHOUT the filter
		// before it was switched on would leave stale .w at the sky pixels the variance blur taps across a silhouette. With SVGF on the
		// two accumulators are the filter's ping-pong images (SVGF.h:416-554) and the sample count restarts, so nothing is lost.
		RT_HIP(ctx, quiesce(ctx));
		for (int aov : { RT_AOV_RADIANCE_DIRECT, RT_AOV_RADIANCE_INDIRECT })
			if (ctx->aov_buffers[aov][1]) RT_HIP(ctx, hipMemsetAsync(ctx->aov_buffers[aov][1], 0, ctx->frame_pixels * 16, ctx->stream));
	} else {
		RT_HIP(ctx, quiesce(ctx));
		for (int i = 0; i < 16; i++) { device_free(ctx, ctx->svgf_buffers[i]); ctx->svgf_buffers[i] = nullptr; }
		for (SampleSlot & slot : ctx->slots) for (int i = 0; i < 3; i++) { device_free(ctx, slot.gbuffers[i]); slot.gbuffers[i] = nullptr; }
		ctx->path_stream.last_gbuffer_slot = -1;
		for (void * & g : ctx->path_stream.gbuffers) { device_free(ctx, g); g = nullptr; }
	}
	ctx->svgf_allocated = want;
	RtParams & p = ctx->params;
	p.gbuffer_normal_and_depth        = (float4 *)ctx->svgf_buffers[0];
	p.gbuffer_mesh_id_and_triangle_id = (int2   *)ctx->svgf_buffers[1];
	p.gbuffer_screen_position_prev    = (float2 *)ctx->svgf_buffers[2];
	p.frame_buffer_moment             = (float4 *)ctx->svgf_buffers[3];
	p.history_length                  = (int    *)ctx->svgf_buffers[4];
	p.history_direct                  = (float4 *)ctx->svgf_buffers[5];
	p.history_indirect                = (float4 *)ctx->svgf_buffers[6];
	p.history_moment                  = (float4 *)ctx->svgf_buffers[7];
	p.history_normal_and_depth        = (float4 *)ctx->svgf_buffers[8];
	p.taa_frame_prev                  = (float4 *)ctx->svgf_buffers[9];
	p.taa_frame_curr                  = (float4 *)ctx->svgf_buffers[10];
	p.svgf_normal_and_depth           = (float4 *)ctx->svgf_buffers[11];
	p.svgf_variance[0]                = (float2 *)ctx->svgf_buffers[12];
	p.svgf_variance[1]                = (float2 *)ctx->svgf_buffers[13];
	p.taa_frame_next                  = (float4 *)ctx->svgf_buffers[14];   // (prev and next trade places after every filtered frame: kernel_taa)
	p.svgf_young_pixels               = (int    *)ctx->svgf_buffers[15];
	return RT_OK;
}

extern "C" {

const char * rt_version(void) { return "gpu-raytracer_amd 0.3 (gfx950, HIP; ABI 4)"; }
int rt_abi_version(void) { return RT_ABI_VERSION; }

const char * rt_last_error(const rt_context * ctx) { return ctx ? ctx->error.c_str() : g_global_error.c_str(); }

int rt_create(int device_ordinal, rt_context ** out_ctx) {
	if (!out_ctx) return fail(nullptr, RT_ERROR_INVALID_ARG, "rt_create: out_ctx is NULL");
	*out_ctx = nullptr;
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count == 0) return fail(nullptr, RT_ERROR_NO_DEVICE, "rt_create: no HIP device available (%s)", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
	if (device_ordinal < 0 || device_ordinal >= count) return fail(nullptr, RT_ERROR_NO_DEVICE, "rt_create: device ordinal %d out of range [0,%d)", device_ordinal, count);
	if (hipSetDevice(device_ordinal) != hipSuccess) return fail(nullptr, RT_ERROR_NO_DEVICE, "rt_create: hipSetDevice(%d) failed", device_ordinal);

	rt_context * ctx = new rt_context();
	ctx->device = device_ordinal;
	memset(&ctx->params, 0, sizeof(ctx->params));
	ctx->params.entry_tlas_stack_size = RT_INVALID;
	ctx->params.svgf_tiles = 1;
	ctx->params.skip_behind_hit = 1;
	memset(&ctx->last_counters, 0, sizeof(ctx->last_counters));
	RT_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
	RT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_main, hipEventDisableTiming));
	RT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_interop, hipEventDisableTiming));
	RT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_scene, hipEventDisableTiming));
	RT_HIP(ctx, hipEventRecord(ctx->ev_scene, ctx->stream));

	int s = ensure_slot(ctx, 0); if (s) return s;
	s = device_alloc(ctx, (void **)&ctx->explicit_retired, 8 * sizeof(int)); if (s) return s;
	s = device_alloc(ctx, (void **)&ctx->pixel_query_out, 2 * sizeof(int)); if (s) return s;
	RT_HIP(ctx, hipMemset(ctx->pixel_query_out, 0xff, 2 * sizeof(int)));
	ctx->params.pixel_query_out = ctx->pixel_query_out;
	ctx->params.pixel_query_pixel = -1;
	// the kernel-level entry points run on the main stream with slot 0's buffers (after quiesce())
	ctx->params.sizes        = ctx->slots[0].sizes;
	ctx->params.ray_cursors  = ctx->slots[0].ray_cursors;
	ctx->params.stack_spill  = (uint2 *)ctx->slots[0].spill[0];

	ctx->params.frame_pixels = 1u << 30; ctx->params.frame_pixels_magic = 5; ctx->params.batch_samples = 1; // until rt_resize
	ctx->params.bvh_width = 8;
	// default config = reference defaults (Common.h:39-67)
	rt_gpu_config c = { RT_FILTER_GAUSSIAN, 1u << RT_AOV_RADIANCE, 10, 1, 1, 1, 1, 0, 1, 1, 0.1f, 0.1f, 6, 4.0f, 16.0f, 10.0f };
	ctx->params.config = c;
	*out_ctx = ctx;
	return RT_OK;
}

void rt_destroy(rt_context * ctx) {
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	(void)quiesce(ctx);
	stream_destroy(ctx);
	(void)rt_comm_destroy(ctx);
	for (void * p : ctx->owned) (void)hipFree(p);
	for (hipEvent_t e : ctx->stage_events) (void)hipEventDestroy(e);
	for (hipEvent_t e : ctx->span_events) (void)hipEventDestroy(e);
	for (SampleSlot & slot : ctx->slots) if (slot.stream) {
		if (slot.pinned_counters) (void)hipHostFree(slot.pinned_counters);
		for (hipEvent_t e : { slot.ev_shaded, slot.ev_shadowed, slot.ev_done, slot.ev_gbuffers, slot.ev_frame_start, slot.ev_frame_end }) if (e) (void)hipEventDestroy(e);
		(void)hipStreamDestroy(slot.side);
		(void)hipStreamDestroy(slot.stream);
	}
	(void)hipEventDestroy(ctx->ev_main);
	(void)hipEventDestroy(ctx->ev_interop);
	(void)hipEventDestroy(ctx->ev_scene);
	for (SceneRing * ring : { &ctx->tlas_ring, &ctx->instance_ring, &ctx->light_ring }) for (int v = 0; v < RT_SCENE_VERSIONS; v++) {
		if (ring->pinned[v]) (void)hipHostFree(ring->pinned[v]);
		if (ring->copied[v]) (void)hipEventDestroy(ring->copied[v]);
		for (hipEvent_t e : ring->last_use[v]) if (e) (void)hipEventDestroy(e);
	}
	(void)hipStreamDestroy(ctx->stream);
	delete ctx;
}

int rt_resize(rt_context * ctx, int width, int height) {
	RT_REQUIRE(ctx, ctx && width > 0 && height > 0, "rt_resize: invalid size");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	int pitch = (width + 31) / 32 * 32; // Math::round_up(width, WARP_SIZE), Pathtracer.cpp:258
	ctx->params.screen_width = width; ctx->params.screen_height = height; ctx->params.screen_pitch = pitch;
	ctx->frame_pixels = size_t(pitch) * height;
	ctx->path_stream.last_gbuffer_slot = -1; // the filter's histories start over with the new size
	stream_release_frames(ctx);

	for (int i = 0; i < RT_AOV_COUNT; i++) for (int k = 0; k < 2; k++) { device_free(ctx, ctx->aov_buffers[i][k]); ctx->aov_buffers[i][k] = nullptr; }
	for (int i = 0; i < RT_AOV_COUNT; i++) for (int k = 1; k < RT_MAX_SAMPLE_SLOTS; k++) { device_free(ctx, ctx->slots[k].aov_framebuffer[i]); ctx->slots[k].aov_framebuffer[i] = nullptr; }
	for (SampleSlot & slot : ctx->slots) slot.aov_samples = 1;
	ctx->params.frame_pixels = unsigned(ctx->frame_pixels);
	ctx->params.frame_pixels_magic = unsigned((1ull << 32) / ctx->frame_pixels) + 1u;
	for (size_t i = 0; i < sizeof(ctx->svgf_buffers) / sizeof(*ctx->svgf_buffers); i++) { device_free(ctx, ctx->svgf_buffers[i]); ctx->svgf_buffers[i] = nullptr; }   // (all 16: the third TAA image [14] and the young-pixel list [15] used to stay behind, 20 B per pixel per resize)
	for (SampleSlot & slot : ctx->slots) for (int i = 0; i < 3; i++) { device_free(ctx, slot.gbuffers[i]); slot.gbuffers[i] = nullptr; }
	ctx->svgf_allocated = false;
	device_free(ctx, ctx->final_image); ctx->final_image = nullptr;
	int s = device_alloc(ctx, &ctx->final_image, ctx->frame_pixels * 16); if (s) return s;
	RT_HIP(ctx, hipMemsetAsync(ctx->final_image, 0, ctx->frame_pixels * 16, ctx->stream));
	ctx->params.final_image = (float4 *)ctx->final_image;
	device_free(ctx, ctx->noise_moments); ctx->noise_moments = nullptr;
	pixel_list_free(ctx);
	denoise_free(ctx);
	firefly_free(ctx);
	if ((s = sync_aovs(ctx))) return s;
	if ((s = sync_svgf(ctx))) return s;
	return sync_noise_moments(ctx);
}

int rt_set_camera(rt_context * ctx, const rt_camera * camera) {
	RT_REQUIRE(ctx, ctx && camera, "rt_set_camera: NULL argument");
	if (memcmp(&ctx->params.camera, camera, sizeof(*camera)) != 0) { int status = stream_launch_pending(ctx); if (status) return status; } // bounce 0 is shaded with the camera
	ctx->params.camera = *camera;
	return RT_OK;
}

int rt_set_svgf_matrices(rt_context * ctx, const float * view_projection, const float * view_projection_prev) {
	RT_REQUIRE(ctx, ctx && view_projection && view_projection_prev, "rt_set_svgf_matrices: NULL argument");
	memcpy(ctx->params.view_projection,      view_projection,      64);
	memcpy(ctx->params.view_projection_prev, view_projection_prev, 64);
	return RT_OK;
}

int rt_set_svgf_tiles(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_svgf_tiles: NULL context");
	ctx->params.svgf_tiles = enable != 0;   // (read at launch time: the filter launches of frames already enqueued keep what they were enqueued with)
	return RT_OK;
}

int rt_set_config(rt_context * ctx, const rt_gpu_config * config) {
	RT_REQUIRE(ctx, ctx && config, "rt_set_config: NULL argument");
	RT_REQUIRE(ctx, config->num_bounces >= 0 && config->num_bounces <= RT_MAX_BOUNCES, "rt_set_config: num_bounces out of range");
	RT_REQUIRE(ctx, config->num_atrous_iterations >= 0 && config->num_atrous_iterations <= RT_MAX_ATROUS_ITERATIONS, "rt_set_config: num_atrous_iterations out of range");
	(void)hipSetDevice(ctx->device);
	if (ctx->path_stream.created && memcmp(&ctx->params.config, config, sizeof(*config)) != 0) RT_HIP(ctx, stream_flush(ctx)); // the submissions in flight were made under the old settings
	ctx->params.config = *config;
	ctx->params.config.aov_mask |= 1u << RT_AOV_RADIANCE;
	if (config->enable_svgf) ctx->params.config.aov_mask |= (1u << RT_AOV_RADIANCE_DIRECT) | (1u << RT_AOV_RADIANCE_INDIRECT) | (1u << RT_AOV_ALBEDO);
	int s = sync_aovs(ctx); if (s) return s;
	return sync_svgf(ctx);
}

// The fog volume. Everything is checked before anything changes; a change completes what is in flight first (paths in flight were
// sorted under the other estimator), as a change of the sky's share does.
// fog_active: a volume is set, some sigma is positive, and there is no density grid or one with a positive maximum -- a volume of zero density, and a grid of
// zeros over any volume, are stored and render as no volume. fog_grid: the ..._grid kernels are the ones to launch. A grid without a volume is inert.
static void fog_refresh_active(rt_context * ctx) {
	RtParams & p = ctx->params;
	float density = 0.0f;
	for (int k = 0; k < 3; k++) density = fmaxf(density, ctx->fog.sigma_a[k] + ctx->fog.sigma_s[k]);
	const bool grid = ctx->fog_grid_set;
	p.fog_active = ctx->fog_set && density > 0.0f && (!grid || ctx->fog_grid_max > 0.0f);
	p.fog_grid = p.fog_active && grid;
	for (int k = 0; k < 3; k++) p.fog_grid_dims[k] = ctx->fog_grid_dims[k];
	p.fog_density = (const float *)ctx->fog_density; p.fog_bricks = (const unsigned char *)ctx->fog_bricks;
}
int rt_set_fog_volume(rt_context * ctx, const rt_fog_volume * volume) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_set_fog_volume: NULL context");
	rt_fog_volume v = { };
	if (volume) {
		v = *volume;
		memset(v.reserved, 0, sizeof(v.reserved));
		for (int k = 0; k < 3; k++) {
			if (!(std::isfinite(v.box_min[k]) && std::isfinite(v.box_max[k]))) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_volume: the box is not finite on axis %d (%.9g .. %.9g)", k, double(v.box_min[k]), double(v.box_max[k]));
			if (!(v.box_min[k] < v.box_max[k])) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_volume: the box needs min < max on axis %d (%.9g .. %.9g)", k, double(v.box_min[k]), double(v.box_max[k]));
			if (!(std::isfinite(v.sigma_a[k]) && v.sigma_a[k] >= 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_volume: sigma_a[%d] = %.9g must be finite and >= 0", k, double(v.sigma_a[k]));
			if (!(std::isfinite(v.sigma_s[k]) && v.sigma_s[k] >= 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_volume: sigma_s[%d] = %.9g must be finite and >= 0", k, double(v.sigma_s[k]));
		}
		if (!(std::fabs(v.g) < 1.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_volume: g = %.9g must lie in (-1, 1)", double(v.g));
	}
	const bool set = volume != nullptr;
	if (set == ctx->fog_set && memcmp(&v, &ctx->fog, sizeof(v)) == 0) return RT_OK;
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	ctx->fog_set = set; ctx->fog = v;
	RtParams & p = ctx->params;
	for (int k = 0; k < 3; k++) { p.fog_box_min[k] = v.box_min[k]; p.fog_box_max[k] = v.box_max[k]; p.fog_sigma_a[k] = v.sigma_a[k]; p.fog_sigma_s[k] = v.sigma_s[k]; }
	p.fog_g = v.g;
	fog_refresh_active(ctx);
	return RT_OK;
}

// The density grid: state of its own beside the volume, mapped onto whatever box is in force. Checked on the host before anything is
// staged; the new grid is allocated, copied and its brick table marked before the one before it is let go, so a refused or failed call leaves that in force.
int rt_set_fog_density(rt_context * ctx, const float * density, int nx, int ny, int nz) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_set_fog_density: NULL context");
	if (!density) {
		if (!ctx->fog_grid_set) return RT_OK;
		(void)hipSetDevice(ctx->device);
		RT_HIP(ctx, quiesce(ctx));
		device_free(ctx, ctx->fog_density); device_free(ctx, ctx->fog_bricks);
		ctx->fog_density = ctx->fog_bricks = nullptr;
		ctx->fog_grid_set = false; ctx->fog_grid_dims[0] = ctx->fog_grid_dims[1] = ctx->fog_grid_dims[2] = 0;
		ctx->fog_grid_bricks = ctx->fog_grid_empty_bricks = 0; ctx->fog_grid_max = 0.0f;
		fog_refresh_active(ctx);
		return RT_OK;
	}
	const int dims[3] = { nx, ny, nz };
	for (int k = 0; k < 3; k++) if (dims[k] < 1 || dims[k] > 1024) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_density: n%c = %d outside 1 .. 1024", "xyz"[k], dims[k]);
	const size_t cells = size_t(nx) * size_t(ny) * size_t(nz);
	if (cells > size_t(1) << 27) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_density: %d x %d x %d = %zu cells, more than 2^27", nx, ny, nz, cells);
	float max_density = 0.0f;
	for (size_t i = 0; i < cells; i++) {
		const float v = density[i];
		if (!(std::isfinite(v) && v >= 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_fog_density: cell (%zu, %zu, %zu) = %.9g must be finite and >= 0", i % size_t(nx), i / size_t(nx) % size_t(ny), i / (size_t(nx) * size_t(ny)), double(v));
		max_density = fmaxf(max_density, v);
	}
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	const int bricks = ((nx + 7) / 8) * ((ny + 7) / 8) * ((nz + 7) / 8);
	void * dev_density = nullptr, * dev_bricks = nullptr, * dev_empty = nullptr;
	int s = device_alloc(ctx, &dev_density, cells * sizeof(float));
	if (!s) s = device_alloc(ctx, &dev_bricks, size_t(bricks));
	if (!s) s = device_alloc(ctx, &dev_empty, sizeof(int));
	int empty = 0;
	hipError_t e = hipSuccess;
	if (!s) {
		e = hipMemcpyAsync(dev_density, density, cells * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess) e = hipMemsetAsync(dev_empty, 0, sizeof(int), ctx->stream);
		if (e == hipSuccess) { rt_launch_fog_mark_bricks((const float *)dev_density, nx, ny, nz, (unsigned char *)dev_bricks, (int *)dev_empty, ctx->stream); e = hipGetLastError(); }
		if (e == hipSuccess) e = hipMemcpyAsync(&empty, dev_empty, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	}
	device_free(ctx, dev_empty);
	if (s || e != hipSuccess) {
		device_free(ctx, dev_density); device_free(ctx, dev_bricks);
		return s ? s : fail(ctx, RT_ERROR_HIP, "rt_set_fog_density: %s", hipGetErrorString(e));
	}
	device_free(ctx, ctx->fog_density); device_free(ctx, ctx->fog_bricks);
	ctx->fog_density = dev_density; ctx->fog_bricks = dev_bricks;
	ctx->fog_grid_set = true; ctx->fog_grid_dims[0] = nx; ctx->fog_grid_dims[1] = ny; ctx->fog_grid_dims[2] = nz;
	ctx->fog_grid_bricks = bricks; ctx->fog_grid_empty_bricks = empty; ctx->fog_grid_max = max_density;
	fog_refresh_active(ctx);
	return RT_OK;
}

int rt_get_fog_density_info(rt_context * ctx, int dims[3], int * bricks, int * empty_bricks, float * max_density, int * out_set) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_get_fog_density_info: NULL context");
	RT_REQUIRE(ctx, dims && bricks && empty_bricks && max_density && out_set, "rt_get_fog_density_info: NULL argument");
	for (int k = 0; k < 3; k++) dims[k] = ctx->fog_grid_dims[k];
	*bricks = ctx->fog_grid_bricks; *empty_bricks = ctx->fog_grid_empty_bricks; *max_density = ctx->fog_grid_max; *out_set = ctx->fog_grid_set ? 1 : 0;
	return RT_OK;
}

int rt_get_fog_volume(rt_context * ctx, rt_fog_volume * out, int * out_set) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_get_fog_volume: NULL context");
	RT_REQUIRE(ctx, out && out_set, "rt_get_fog_volume: NULL argument");
	*out = ctx->fog; *out_set = ctx->fog_set ? 1 : 0;
	return RT_OK;
}

int rt_set_pixel_range(rt_context * ctx, int pixel_offset, int pixel_count) {
	RT_REQUIRE(ctx, ctx && pixel_offset >= 0, "rt_set_pixel_range: invalid argument");
	if (ctx->pixel_offset != pixel_offset || ctx->pixel_count != pixel_count || ctx->params.tile_pixels != 0) { int s = noise_moments_reset(ctx); if (s) return s; }
	ctx->pixel_offset = pixel_offset;
	ctx->pixel_count  = pixel_count;
	ctx->params.tile_pixels = 0;
	return RT_OK;
}

int rt_set_pixel_tiles(rt_context * ctx, int tile_pixels, int first_tile, int tile_stride) {
	RT_REQUIRE(ctx, ctx && tile_pixels > 0 && first_tile >= 0 && tile_stride > 0 && first_tile < tile_stride, "rt_set_pixel_tiles: invalid argument");
	if (ctx->params.tile_pixels != tile_pixels || ctx->params.tile_first != first_tile || ctx->params.tile_stride != tile_stride) { int s = noise_moments_reset(ctx); if (s) return s; }
	ctx->params.tile_pixels = tile_pixels;
	ctx->params.tile_first  = first_tile;
	ctx->params.tile_stride = tile_stride;
	return RT_OK;
}

int rt_pack_pixels(rt_context * ctx, void * dst_device, int tile_pixels, int first_tile, int tile_stride, int tiles) {
	RT_REQUIRE(ctx, ctx && dst_device && tile_pixels > 0 && tile_stride > 0 && tiles >= 0, "rt_pack_pixels: invalid argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->final_image) return fail(ctx, RT_ERROR_NOT_READY, "rt_pack_pixels: rt_resize was not called");
	RT_HIP(ctx, main_waits_for_samples(ctx));
	rt_launch_pack_pixels(ctx->params, (float4 *)dst_device, tile_pixels, first_tile, tile_stride, tiles, ctx->stream);
	RT_HIP(ctx, hipGetLastError());
	return RT_OK;
}

int rt_unpack_pixels(rt_context * ctx, const void * src_device, int tile_pixels, int world, int tiles_per_rank) {
	RT_REQUIRE(ctx, ctx && src_device && tile_pixels > 0 && world > 0 && tiles_per_rank > 0, "rt_unpack_pixels: invalid argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->final_image) return fail(ctx, RT_ERROR_NOT_READY, "rt_unpack_pixels: rt_resize was not called");
	RT_HIP(ctx, main_waits_for_samples(ctx));
	rt_launch_unpack_pixels(ctx->params, (const float4 *)src_device, tile_pixels, world, tiles_per_rank, ctx->stream);
	RT_HIP(ctx, hipGetLastError());
	return RT_OK;
}

// ---- SVGF frames under the tile split ---------------------------------------------------------------
int rt_render_sample_unfiltered(rt_context * ctx, int sample_index) {
	RT_REQUIRE(ctx, ctx, "rt_render_sample_unfiltered: NULL context");
	if (!ctx->params.config.enable_svgf) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_sample_unfiltered: SVGF is not enabled");
	ctx->defer_filter = true;
	int status = rt_render_samples(ctx, sample_index, 1);
	ctx->defer_filter = false;
	return status;
}

int rt_pack_svgf_inputs(rt_context * ctx, void * dst_device, int tile_pixels, int first_tile, int tile_stride, int tiles) {
	RT_REQUIRE(ctx, ctx && dst_device && tile_pixels > 0 && tile_stride > 0 && tiles >= 0, "rt_pack_svgf_inputs: invalid argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->svgf_allocated) return fail(ctx, RT_ERROR_NOT_READY, "rt_pack_svgf_inputs: SVGF is not enabled");
	RT_HIP(ctx, main_waits_for_samples(ctx));
	rt_launch_pack_svgf(slot_params(ctx, ctx->slots[0], 0), (float4 *)dst_device, tile_pixels, first_tile, tile_stride, tiles, ctx->stream);
	RT_HIP(ctx, hipGetLastError());
	return RT_OK;
}

int rt_unpack_svgf_inputs(rt_context * ctx, const void * src_device, int tile_pixels, int world, int tiles_per_rank) {
	RT_REQUIRE(ctx, ctx && src_device && tile_pixels > 0 && world > 0 && tiles_per_rank > 0, "rt_unpack_svgf_inputs: invalid argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->svgf_allocated) return fail(ctx, RT_ERROR_NOT_READY, "rt_unpack_svgf_inputs: SVGF is not enabled");
	RT_HIP(ctx, main_waits_for_samples(ctx));
	rt_launch_unpack_svgf(slot_params(ctx, ctx->slots[0], 0), (const float4 *)src_device, tile_pixels, world, tiles_per_rank, ctx->stream);
	RT_HIP(ctx, hipGetLastError());
	return RT_OK;
}

int rt_filter_frame(rt_context * ctx, int sample_index) {
	RT_REQUIRE(ctx, ctx, "rt_filter_frame: NULL context");
	(void)hipSetDevice(ctx->device);
	if (!ctx->params.config.enable_svgf || !ctx->svgf_allocated) return fail(ctx, RT_ERROR_NOT_READY, "rt_filter_frame: SVGF is not enabled");
	SampleSlot & slot = ctx->slots[0];
	RtParams p = slot_params(ctx, slot, 0);
	p.batch_samples = 1;
	hipStream_t st = slot.stream;
	RT_HIP(ctx, hipEventRecord(ctx->ev_main, ctx->stream));      // after the scatter of the gathered tiles (main stream)
	RT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_main, 0));
	rt_launch_svgf_taa(p, sample_index, st);
	if (p.config.enable_taa) std::swap(ctx->params.taa_frame_prev, ctx->params.taa_frame_next);   // (the snapshot that launched kernel_taa decides, not a config set meanwhile)
	for (int i = 0; i < RT_AOV_COUNT; i++) if (p.aovs[i].framebuffer) RT_HIP(ctx, hipMemsetAsync(p.aovs[i].framebuffer, 0, ctx->frame_pixels * 16, st)); // aovs_clear_to_zero
	RT_HIP(ctx, hipEventRecord(slot.ev_done, st));
	RT_HIP(ctx, hipGetLastError());
	return RT_OK;
}

int rt_read_svgf_state(rt_context * ctx, int which, void * dst) {
	RT_REQUIRE(ctx, ctx && dst, "rt_read_svgf_state: NULL argument");
	RT_REQUIRE(ctx, which >= 0 && which < RT_SVGF_STATE_COUNT, "rt_read_svgf_state: unknown image (which is not one of RT_SVGF_STATE_*)");
	(void)hipSetDevice(ctx->device);
	if (!ctx->svgf_allocated) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_svgf_state: SVGF is not allocated");
	const RtParams & p = ctx->params;
	const void * src = nullptr;
	size_t bytes = 16;
	switch (which) {
		case RT_SVGF_STATE_HISTORY_LENGTH:           src = p.history_length; bytes = 4; break;
		case RT_SVGF_STATE_HISTORY_DIRECT:           src = p.history_direct; break;
		case RT_SVGF_STATE_HISTORY_INDIRECT:         src = p.history_indirect; break;
		case RT_SVGF_STATE_HISTORY_MOMENT:           src = p.history_moment; break;
		case RT_SVGF_STATE_HISTORY_NORMAL_AND_DEPTH: src = p.history_normal_and_depth; break;
		case RT_SVGF_STATE_FRAME_MOMENT:             src = p.frame_buffer_moment; break;
		case RT_SVGF_STATE_TAA_HISTORY:              src = p.taa_frame_prev; break;   // (swapped with taa_frame_next after every filtered frame)
		case RT_SVGF_STATE_TAA_CURRENT:              src = p.taa_frame_curr; break;
	}
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(dst, src, ctx->frame_pixels * bytes, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_stream_wait_for_context(rt_context * ctx, void * stream) {
	RT_REQUIRE(ctx, ctx, "rt_stream_wait_for_context: NULL context");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, hipEventRecord(ctx->ev_interop, ctx->stream));
	RT_HIP(ctx, hipStreamWaitEvent((hipStream_t)stream, ctx->ev_interop, 0));
	return RT_OK;
}

int rt_context_wait_for_stream(rt_context * ctx, void * stream) {
	RT_REQUIRE(ctx, ctx, "rt_context_wait_for_stream: NULL context");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, hipEventRecord(ctx->ev_interop, (hipStream_t)stream));
	RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_interop, 0));
	return RT_OK;
}

int rt_set_trace_statistics(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_trace_statistics: NULL context");
	(void)hipSetDevice(ctx->device);
	if (enable && !ctx->trace_stats) { int s = device_alloc(ctx, (void **)&ctx->trace_stats, 10 * sizeof(unsigned long long)); if (s) return s; }
	{ int s = stream_launch_pending(ctx); if (s) return s; }
	ctx->trace_statistics = enable != 0;
	return RT_OK;
}

int rt_get_trace_statistics(rt_context * ctx, uint64_t * out10) {
	RT_REQUIRE(ctx, ctx && out10, "rt_get_trace_statistics: NULL argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->trace_stats) return fail(ctx, RT_ERROR_NOT_READY, "rt_get_trace_statistics: statistics were never enabled");
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(out10, ctx->trace_stats, 10 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_set_batch_size(rt_context * ctx, int batch_size) {
	RT_REQUIRE(ctx, ctx && batch_size >= 0, "rt_set_batch_size: invalid argument");
	ctx->batch_size_request = batch_size;
	return RT_OK;
}

int rt_set_profiling(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_profiling: NULL context");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	ctx->profiling = enable == 1;
	ctx->launch_timing = enable == 2 || enable == 3;
	ctx->launch_timing_all = enable == 3;
	ctx->span_used = 0;
	ctx->stage_used = 0;
	return RT_OK;
}

int rt_get_launch_timings(rt_context * ctx, int kind, float * out_ms, int capacity, int * out_count) {
	RT_REQUIRE(ctx, ctx && out_count && (out_ms || capacity == 0) && kind >= 0 && kind < RT_TIMING_KINDS, "rt_get_launch_timings: invalid argument");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	int n = 0;
	for (size_t i = 0; i + 1 < ctx->span_used; i += 2) {
		if (ctx->span_kinds[i] != kind) continue;
		float d = 0.0f;
		if (hipEventElapsedTime(&d, ctx->span_events[i], ctx->span_events[i + 1]) != hipSuccess) continue;
		if (n < capacity) out_ms[n] = d;
		n++;
	}
	*out_count = n;
	if (n <= capacity) { // everything delivered: start over (a call with too small a buffer only reports the count)
		size_t kept = 0;
		for (size_t i = 0; i + 1 < ctx->span_used; i += 2) if (ctx->span_kinds[i] != kind) {
			std::swap(ctx->span_events[kept], ctx->span_events[i]); std::swap(ctx->span_events[kept + 1], ctx->span_events[i + 1]);
			ctx->span_kinds[kept] = ctx->span_kinds[i]; ctx->span_kinds[kept + 1] = ctx->span_kinds[i + 1];
			kept += 2;
		}
		ctx->span_used = kept;
	}
	return RT_OK;
}

int rt_set_scheduler(rt_context * ctx, int scheduler) {
	RT_REQUIRE(ctx, ctx && (scheduler == RT_SCHEDULER_MERGED || scheduler == RT_SCHEDULER_SLOTS), "rt_set_scheduler: unknown scheduler");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	ctx->scheduler = scheduler;
	return RT_OK;
}

int rt_set_texture_expansion(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_texture_expansion: NULL context");
	ctx->expand_bc1 = enable != 0;   // takes effect at the next rt_upload_textures
	return RT_OK;
}
size_t rt_texture_bytes(rt_context * ctx) { return ctx ? ctx->texture_bytes : 0; }

int rt_set_frame_pipelining(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_frame_pipelining: NULL context");
	ctx->frame_pipelining = enable != 0;
	return RT_OK;
}

int rt_set_stream_batch(rt_context * ctx, long long paths) {
	RT_REQUIRE(ctx, ctx && paths >= 0, "rt_set_stream_batch: invalid argument");
	ctx->stream_batch_paths = paths;   // (read by the next submission; what already waits for company is enqueued by whatever needs progress, as always)
	return RT_OK;
}

int rt_get_trace_statistics_history(rt_context * ctx, uint64_t * out_rows10, int capacity_rows, int * out_rows) {
	RT_REQUIRE(ctx, ctx && out_rows && (out_rows10 || capacity_rows == 0), "rt_get_trace_statistics_history: invalid argument");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	int rows = ctx->stream_history ? ctx->stream_history_rows : 0;
	*out_rows = rows;
	if (rows > capacity_rows) rows = capacity_rows;
	if (rows > 0) memcpy(out_rows10, ctx->stream_history, size_t(rows) * 10 * sizeof(uint64_t));
	return RT_OK;
}

// ---- results ---------------------------------------------------------------------------------------------------

int rt_read_aov(rt_context * ctx, int aov_type, float * dst, int accumulated) {
	RT_REQUIRE(ctx, ctx && dst && aov_type >= 0 && aov_type < RT_AOV_COUNT, "rt_read_aov: invalid argument");
	(void)hipSetDevice(ctx->device);
	void * src = ctx->aov_buffers[aov_type][accumulated ? 1 : 0];
	if (!src) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_aov: AOV %d is not enabled", aov_type);
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(dst, src, ctx->frame_pixels * 16, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_read_framebuffer(rt_context * ctx, float * dst) {
	RT_REQUIRE(ctx, ctx && dst, "rt_read_framebuffer: NULL argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->final_image) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_framebuffer: rt_resize was not called");
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(dst, ctx->final_image, ctx->frame_pixels * 16, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_framebuffer_device_ptr(rt_context * ctx, void ** out_ptr, size_t * out_bytes) {
	RT_REQUIRE(ctx, ctx && out_ptr && out_bytes, "rt_framebuffer_device_ptr: NULL argument");
	if (!ctx->final_image) return fail(ctx, RT_ERROR_NOT_READY, "rt_framebuffer_device_ptr: rt_resize was not called");
	*out_ptr = ctx->final_image;
	*out_bytes = ctx->frame_pixels * 16;
	return RT_OK;
}

int rt_screen_pitch(rt_context * ctx) { return ctx ? ctx->params.screen_pitch : 0; }

int rt_read_luts(rt_context * ctx, float * dielectric_dir_enter, float * dielectric_dir_leave, float * dielectric_enter, float * dielectric_leave, float * conductor_dir, float * conductor) {
	RT_REQUIRE(ctx, ctx, "rt_read_luts: NULL context");
	(void)hipSetDevice(ctx->device);
	if (!ctx->params.pmj_samples) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_luts: RNG tables not uploaded");
	int s = ensure_luts(ctx); if (s) return s;
	RT_HIP(ctx, quiesce(ctx));
	float * dst[6] = { dielectric_dir_enter, dielectric_dir_leave, dielectric_enter, dielectric_leave, conductor_dir, conductor };
	const size_t bytes[6] = { 4096 * 4, 4096 * 4, 256 * 4, 256 * 4, 1024 * 4, 32 * 4 };
	for (int i = 0; i < 6; i++) if (dst[i]) RT_HIP(ctx, hipMemcpy(dst[i], ctx->luts[i], bytes[i], hipMemcpyDeviceToHost));
	return RT_OK;
}

} // extern "C"
