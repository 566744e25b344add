// rt_stream.hip -- the merged wavefront's host side (RT_SCHEDULER_MERGED; PathStream in rt_context.h describes the idea): what rt_render_samples
// (rt_render.hip) hands a submission to, and what every call that needs its progress or its end drives. Internal: no entry point is defined here.
#include "rt_context.h"

#include <algorithm>
#include <cstring>

// rt_launch_svgf_taa calls this before and after each of its kernels (mode 3)
static void svgf_span_mark(void * user, int svgf_kernel, hipStream_t stream) { span_mark((rt_context *)user, SPAN_SVGF + svgf_kernel, stream); }

int stream_create(rt_context * ctx) {
	PathStream & s = ctx->path_stream;
	if (s.created) return RT_OK;
	if (!ctx->stream_history) RT_HIP(ctx, hipHostMalloc((void **)&ctx->stream_history, sizeof(unsigned long long) * 10 * RT_STREAM_HISTORY_ROWS));
	RT_HIP(ctx, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
	RT_HIP(ctx, hipEventCreateWithFlags(&s.ev_idle, hipEventDisableTiming));
	RT_HIP(ctx, hipEventRecord(s.ev_idle, s.stream));
	int status = device_alloc(ctx, (void **)&s.control, sizeof(RtStreamControl)); if (status) return status;
	RT_HIP(ctx, hipMemset(s.control, 0, sizeof(RtStreamControl)));
	status = device_alloc(ctx, (void **)&s.table_device, sizeof(RtStreamTable)); if (status) return status;
	RT_HIP(ctx, hipMemset(s.table_device, 0, sizeof(RtStreamTable)));
	memset(&s.table_host, 0, sizeof(s.table_host));
	RT_HIP(ctx, hipHostMalloc((void **)&s.table_staging, sizeof(RtStreamTable) * RT_STREAM_TABLE_SNAPSHOTS));
	for (hipEvent_t & e : s.table_copied) { RT_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming)); RT_HIP(ctx, hipEventRecord(e, s.stream)); }
	// one spill area: the closest-hit and the shadow part of the fused launch run one after the other in the same waves
	status = device_alloc(ctx, &s.spill, size_t(24) * 8 * 256 * 8 * 256); if (status) return status;
	RT_HIP(ctx, hipHostMalloc((void **)&s.progress, sizeof(int) * 2 * RT_STREAM_PROGRESS_RING));
	for (int i = 0; i < 2 * RT_STREAM_PROGRESS_RING; i++) s.progress[i] = -1;
	for (hipEvent_t & e : s.iteration_done) { RT_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming)); RT_HIP(ctx, hipEventRecord(e, s.stream)); }
	RT_HIP(ctx, hipHostMalloc((void **)&s.stats_host, sizeof(int) * RT_STREAM_SUBMISSIONS * RT_STREAM_STATS_ROW));
	memset(s.stats_host, 0, sizeof(int) * RT_STREAM_SUBMISSIONS * RT_STREAM_STATS_ROW);
	for (int i = 0; i < RT_STREAM_SUBMISSIONS; i++) { RT_HIP(ctx, hipEventCreate(&s.ev_begin[i])); RT_HIP(ctx, hipEventCreate(&s.ev_end[i])); }
	s.created = true;
	return RT_OK;
}

void stream_destroy(rt_context * ctx) {
	PathStream & s = ctx->path_stream;
	if (ctx->stream_history) { (void)hipHostFree(ctx->stream_history); ctx->stream_history = nullptr; }
	if (!s.stream) return;
	if (s.table_staging) (void)hipHostFree(s.table_staging);
	if (s.progress)      (void)hipHostFree(s.progress);
	if (s.stats_host)    (void)hipHostFree(s.stats_host);
	for (hipEvent_t e : s.table_copied)   if (e) (void)hipEventDestroy(e);
	for (hipEvent_t e : s.iteration_done) if (e) (void)hipEventDestroy(e);
	for (hipEvent_t e : s.ev_begin)       if (e) (void)hipEventDestroy(e);
	for (hipEvent_t e : s.ev_end)         if (e) (void)hipEventDestroy(e);
	if (s.ev_idle) (void)hipEventDestroy(s.ev_idle);
	(void)hipStreamDestroy(s.stream);
	s.stream = nullptr; s.created = false;
}

// SVGF: a frame starts from a copy of the g-buffers of the frame before it (the reference has ONE set that every frame
// overwrites where its primary rays hit something). Before the sets of the sample slots are freed or re-allocated the
// latest one moves to the set of slot 0 of the slot scheduler, where the next frame of either scheduler finds it.
void stream_save_gbuffers(rt_context * ctx) {
	PathStream & s = ctx->path_stream;
	if (s.last_gbuffer_slot >= 0 && s.gbuffers[0] && ctx->svgf_buffers[0]) {
		(void)hipDeviceSynchronize();
		for (int i = 0; i < 3; i++) (void)hipMemcpy(ctx->svgf_buffers[i], stream_gbuffer(ctx, i, s.last_gbuffer_slot), gbuffer_bytes(ctx, i), hipMemcpyDeviceToDevice);
		ctx->last_slot = 0;
	}
	s.last_gbuffer_slot = -1;
}

// The per-sample frames of the sample slots (they are freed with the frame resources: rt_resize, AOV changes).
void stream_release_frames(rt_context * ctx) {
	PathStream & s = ctx->path_stream;
	for (void * & fb : s.aov_framebuffer) { device_free(ctx, fb); fb = nullptr; }
	stream_save_gbuffers(ctx);
	for (void * & g : s.gbuffers) { device_free(ctx, g); g = nullptr; }
	s.frame_slots = 0;
}

static int stream_ensure_frames(rt_context * ctx, int wanted_slots) {
	PathStream & s = ctx->path_stream;
	int limit = int(std::min<size_t>(RT_STREAM_SAMPLE_SLOTS, ((size_t(1) << 30) - 1) / ctx->frame_pixels));
	int slots = std::min(limit, std::max(wanted_slots, 8));
	bool complete = s.frame_slots >= slots;
	for (int i = 0; i < RT_AOV_COUNT; i++) if ((ctx->aov_buffers[i][0] != nullptr) != (s.aov_framebuffer[i] != nullptr)) complete = false;
	if (ctx->svgf_allocated != (s.gbuffers[0] != nullptr)) complete = false;
	if (complete) return RT_OK;
	RT_HIP(ctx, quiesce(ctx));
	slots = std::max(slots, s.frame_slots);
	stream_save_gbuffers(ctx);
	for (void * & g : s.gbuffers) { device_free(ctx, g); g = nullptr; }
	for (void * & fb : s.aov_framebuffer) { device_free(ctx, fb); fb = nullptr; }
	size_t bytes = ctx->frame_pixels * 16 * size_t(slots);
	for (int i = 0; i < RT_AOV_COUNT; i++) if (ctx->aov_buffers[i][0]) {
		int status = device_alloc(ctx, &s.aov_framebuffer[i], bytes); if (status) return status;
		RT_HIP(ctx, hipMemset(s.aov_framebuffer[i], 0, bytes));
	}
	if (ctx->svgf_allocated) for (int i = 0; i < 3; i++) {
		int status = device_alloc(ctx, &s.gbuffers[i], gbuffer_bytes(ctx, i) * size_t(slots)); if (status) return status;
		RT_HIP(ctx, hipMemset(s.gbuffers[i], 0, gbuffer_bytes(ctx, i) * size_t(slots)));
	}
	s.frame_slots = slots;
	for (bool & used : s.slot_used) used = false;
	s.next_slot = 0;
	return RT_OK;
}

static int stream_ensure_queues(rt_context * ctx, size_t entries) {
	PathStream & s = ctx->path_stream;
	if (s.queues.allocated && s.queues.capacity >= entries) return RT_OK;
	RT_HIP(ctx, quiesce(ctx));
	if (s.queues.allocated) queues_free(ctx, s.queues);
	return queues_allocate(ctx, s.queues, entries);
}

// The parameter block of iteration `iteration`: the context's block with the stream's queues, control block and
// per-sample frames patched in.
RtParams stream_params(const rt_context * ctx, int iteration) {
	const PathStream & s = ctx->path_stream;
	RtParams p = ctx->params;
	use_queues(p, s.queues);
	p.sizes = nullptr; p.ray_cursors = nullptr; p.stack_spill = (uint2 *)s.spill;
	p.stream = s.control; p.stream_table = s.table_device; p.stream_iteration = iteration;
	for (int i = 0; i < RT_AOV_COUNT; i++) p.aovs[i].framebuffer = (float4 *)s.aov_framebuffer[i];
	if (s.gbuffers[0]) { // x + y * pitch of a VIRTUAL pixel is the virtual pixel: the shade kernels write the set of the path's slot
		p.gbuffer_normal_and_depth = (float4 *)s.gbuffers[0]; p.gbuffer_mesh_id_and_triangle_id = (int2 *)s.gbuffers[1]; p.gbuffer_screen_position_prev = (float2 *)s.gbuffers[2];
	}
	p.batch_samples = 1;
	return p;
}

// Reads the wavefront sizes the device has reported so far (pinned memory, no synchronisation).
static void stream_update_known(PathStream & s) {
	for (int k = std::max(s.known_iteration + 1, s.iteration - RT_STREAM_PROGRESS_RING + 1); k < s.iteration; k++) {
		volatile int * entry = s.progress + 2 * (k % RT_STREAM_PROGRESS_RING);
		if (entry[0] != k) break;
		s.known_iteration = k; s.known_size = entry[1];
	}
}

// Upper bound of the paths in flight when the next iteration starts (before anything it generates).
static long long stream_bound(PathStream & s) {
	stream_update_known(s);
	int from = s.base_iteration; long long bound = 0;
	if (s.known_iteration >= s.base_iteration) { from = s.known_iteration + 1; bound = s.known_size; }
	for (int k = from; k < s.iteration; k++) bound += s.generated[k % RT_STREAM_PROGRESS_RING];
	return bound;
}

// The submissions that have passed their last bounce with iteration i (consecutive, in submission order; with batched
// admission up to RT_STREAM_MAX_BATCH of them): folded into the accumulators, their sample slots cleared and released.
static int stream_complete(rt_context * ctx, const StreamSubmission * subs, int count, const RtParams & p) {
	PathStream & s = ctx->path_stream;
	hipStream_t st = s.stream;
	// the accumulate step follows the main-stream work submitted so far (rt_pack_pixels of an earlier frame reads,
	// rt_unpack_pixels writes the image)
	RT_HIP(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
	RT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_main, 0));
	stage_mark(ctx, STAGE_POST, st);
	if (p.config.enable_svgf) { // one filtered frame per submission: reproject / variance / a-trous / finalize / TAA on its own sample frames and g-buffers
		for (int k = 0; k < count; k++) {
			const StreamSubmission & sub = subs[k];
			RtParams pf = p;
			pf.taa_frame_prev = ctx->params.taa_frame_prev; pf.taa_frame_next = ctx->params.taa_frame_next;   // (they trade places after every filtered frame)
			for (int i = 0; i < RT_AOV_COUNT; i++) if (pf.aovs[i].framebuffer) pf.aovs[i].framebuffer += size_t(sub.slot_base) * ctx->frame_pixels;
			pf.gbuffer_normal_and_depth += size_t(sub.slot_base) * ctx->frame_pixels; pf.gbuffer_mesh_id_and_triangle_id += size_t(sub.slot_base) * ctx->frame_pixels; pf.gbuffer_screen_position_prev += size_t(sub.slot_base) * ctx->frame_pixels;
			rt_launch_svgf_taa(pf, sub.first_sample, st, ctx->launch_timing_all && ctx->time_this_sample ? svgf_span_mark : nullptr, ctx);
			if (pf.config.enable_taa) std::swap(ctx->params.taa_frame_prev, ctx->params.taa_frame_next);   // (the submission's own config snapshot launched kernel_taa: the same one decides the swap)
			for (int i = 0; i < RT_AOV_COUNT; i++) if (pf.aovs[i].framebuffer) RT_HIP(ctx, hipMemsetAsync(pf.aovs[i].framebuffer, 0, ctx->frame_pixels * 16 * size_t(sub.sample_count), st)); // aovs_clear_to_zero
		}
	} else
	for (int first = 0; first < count; ) {
		// one launch for a run of submissions over the same pixels
		const StreamSubmission & head = subs[first];
		RtAccumulate a = { };
		RtAccumulateGroup & group = a.group;
		int k = first;
		for (; k < count && group.count < RT_ACCUMULATE_GROUP; k++) {
			const StreamSubmission & sub = subs[k];
			if (sub.range_offset != head.range_offset || sub.range_count != head.range_count || sub.tile_pixels != head.tile_pixels || sub.tile_first != head.tile_first || sub.tile_stride != head.tile_stride || sub.list != head.list) break;
			group.first_sample[group.count] = sub.first_sample; group.sample_count[group.count] = sub.sample_count; group.slot_base[group.count] = sub.slot_base;
			group.count++;
		}
		RtParams pa = p;
		pa.tile_pixels = head.tile_pixels; pa.tile_first = head.tile_first; pa.tile_stride = head.tile_stride;
		span_mark(ctx, SPAN_ACCUMULATE, st);
		a.clear = true; a.pixel_offset = head.range_offset; a.pixel_count = head.range_count;
		a.list = head.list ? (const unsigned *)ctx->pixel_list : nullptr;   // (the list does not change while a submission is in flight)
		a.moments = noise_moments_for(ctx, pa);
		a.tiers = firefly_tiers_for(ctx, pa);   // (the cascade forms of the same kernels while rt_set_firefly_cascade is on)
		rt_launch_accumulate(pa, a, st);
		span_mark(ctx, SPAN_ACCUMULATE, st);
		first = k;
	}
	stage_mark(ctx, STAGE_END, st);
	if (!p.config.enable_svgf) for (int k = 0; k < count; k++) {
		const StreamSubmission & sub = subs[k];
		// the AOVs the accumulate kernel does not fold (DIRECT / INDIRECT exist for the filter only) are cleared the plain way
		for (int i : { RT_AOV_RADIANCE_DIRECT, RT_AOV_RADIANCE_INDIRECT }) if (p.aovs[i].framebuffer)
			RT_HIP(ctx, hipMemsetAsync(p.aovs[i].framebuffer + size_t(sub.slot_base) * ctx->frame_pixels, 0, ctx->frame_pixels * 16 * size_t(sub.sample_count), st)); // aovs_clear_to_zero
	}
	for (int k = 0; k < count; ) { // statistics rows: consecutive ring entries travel in one copy
		int run = 1;
		while (k + run < count && subs[k + run].ring == subs[k].ring + run) run++;
		RT_HIP(ctx, hipMemcpyAsync(s.stats_host + size_t(subs[k].ring) * RT_STREAM_STATS_ROW, &s.control->stats[subs[k].ring][0][0], sizeof(int) * RT_STREAM_STATS_ROW * size_t(run), hipMemcpyDeviceToHost, st));
		k += run;
	}
	for (int k = 0; k < count; k++) {
		const StreamSubmission & sub = subs[k];
		RT_HIP(ctx, hipEventRecord(s.ev_end[sub.ring], st));
		for (int j = 0; j < sub.sample_count; j++) s.slot_used[sub.slot_base + j] = false;
		s.last_completed_ring = sub.ring;
		s.submissions_completed++;
	}
	RT_HIP(ctx, hipEventRecord(s.ev_idle, st));
	return RT_OK;
}

// The fused traversal launch fetches every node from ONE array: the TLAS (which lives in a ring of versions, for the
// per-submission chains that keep frames of different scene versions in flight) is copied into the slots [0, node count)
// that the BLAS node array reserves for it -- node indices below the TLAS size never name BLAS nodes. Nothing of the merged
// wavefront is in flight when the TLAS changes (every upload completes it first), and the other kernels never read those slots.
int stream_sync_tlas(rt_context * ctx) {
	if (ctx->tlas_version_in_nodes == ctx->tlas_version) return RT_OK;
	if (!ctx->params.tlas_nodes || ctx->params.tlas_node_count <= 0) {   // one BVH, no TLAS: node 0 is its root
		ctx->tlas_version_in_nodes = ctx->tlas_version; return RT_OK;
	}
	if (!ctx->bvh8_nodes || size_t(ctx->params.tlas_node_count) > ctx->bvh8_node_count) return fail(ctx, RT_ERROR_NOT_READY, "rt_render_samples: the TLAS does not fit the node slots the geometry reserves for it");
	// the copy below overwrites node slots [0, tlas_node_count): they must be CWBVH nodes and must not hold BLAS nodes (the host
	// classes reserve 2 x meshes slots in front of the first BLAS; a C-API caller with another layout gets an error, not a
	// silently corrupted BVH -- the per-submission scheduler, which reads the TLAS from its own buffer, renders such layouts)
	if (ctx->tlas_node_bytes != 80) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: the merged wavefront needs the TLAS as 80-byte CWBVH nodes (rt_upload_tlas); select RT_SCHEDULER_SLOTS for other BVH types");
	if (ctx->params.tlas_node_count > ctx->lowest_blas_root) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: a BLAS root (node %d) lies inside the %d node slots the merged wavefront copies the TLAS into; reserve them in front of the BLAS nodes or select RT_SCHEDULER_SLOTS", ctx->lowest_blas_root, ctx->params.tlas_node_count);
	hipStream_t st = ctx->path_stream.stream;
	RT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_scene, 0));
	RT_HIP(ctx, hipMemcpyAsync(ctx->bvh8_nodes, ctx->params.tlas_nodes, size_t(ctx->params.tlas_node_count) * 80, hipMemcpyDeviceToDevice, st));
	ctx->tlas_version_in_nodes = ctx->tlas_version;
	return RT_OK;
}

// The generate launch of a submission, as the scheduler chooses it (stream_generate below, and rt_generate_primary_rays, which reports the choice
// to the tests). `pg`: the parameters of the iteration with the submission's batch_samples and tiles; `list`: its pixel list, or null.
// Queue order of the primary rays: 8 x 8 pixel patches along bands of 8 scan lines when the submission's pixel list is made of whole bands
// (the whole frame, or tiles of whole bands: rt_map_pixel keeps a band together); scan lines otherwise. order2, if given: { block_width, band_rows }.
void stream_launch_generate(const RtParams & pg, int first_sample, const unsigned * list, int range_offset, int range_count, int slot_base, int queue_offset, hipStream_t st, int * order2) {
	const int order = 8;
	const int frame = pg.screen_width * pg.screen_height;
	const bool whole_bands = pg.tile_pixels > 0 ? pg.tile_pixels % (order * pg.screen_width) == 0 : (range_offset == 0 && range_count == frame);
	if (order2) order2[0] = order2[1] = list ? 0 : whole_bands ? order : 0;   // (a list is in patch order already: the kernel walks it as it is)
	if (list) rt_launch_generate_stream_list(pg, first_sample, list, range_count, slot_base, queue_offset, st);
	else rt_launch_generate_stream(pg, first_sample, range_offset, range_count, slot_base, queue_offset, whole_bands ? order : 0, whole_bands ? order : 0, st);
}

// The primary rays of a new submission: appended to the trace queue of the iteration that is enqueued next, behind the
// rays of the submissions already waiting for it.
static int stream_generate(rt_context * ctx, const StreamSubmission & sub) {
	PathStream & s = ctx->path_stream;
	hipStream_t st = s.stream;
	RT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_scene, 0));  // asynchronous scene uploads (they flush the wavefront first)
	RtParams pg = stream_params(ctx, s.iteration);
	pg.batch_samples = sub.sample_count;
	pg.tile_pixels = sub.tile_pixels; pg.tile_first = sub.tile_first; pg.tile_stride = sub.tile_stride;
	RT_HIP(ctx, hipEventRecord(s.ev_begin[sub.ring], st));
	stage_mark(ctx, STAGE_GENERATE, st);
	span_mark(ctx, SPAN_GENERATE, st);
	stream_launch_generate(pg, sub.first_sample, sub.list ? (const unsigned *)ctx->pixel_list : nullptr, sub.range_offset, sub.range_count, sub.slot_base, int(s.pending_paths), st, nullptr);
	span_mark(ctx, SPAN_GENERATE, st);
	s.pending++; s.pending_paths += sub.paths;
	return RT_OK;
}

// One iteration of the wavefront: advance (counts the rays generated since the last one in) -> fused trace -> sort ->
// shade, then the accumulate step of every submission that has just passed its last bounce.
int stream_enqueue_iteration(rt_context * ctx) {
	PathStream & s = ctx->path_stream;
	const int i = s.iteration;
	hipStream_t st = s.stream;
	if (i - RT_STREAM_RUN_AHEAD >= 0) RT_HIP(ctx, hipEventSynchronize(s.iteration_done[(i - RT_STREAM_RUN_AHEAD) % RT_STREAM_PROGRESS_RING]));
	RtParams p = stream_params(ctx, i);
	const int generated = int(s.pending_paths);
	s.pending = 0; s.pending_paths = 0;
	if (s.table_dirty) {
		// the table travels in stream order: the kernels of earlier iterations have run when it lands, and they never look at the entries of free slots
		int snapshot = s.table_next; s.table_next = (s.table_next + 1) % RT_STREAM_TABLE_SNAPSHOTS;
		RT_HIP(ctx, hipEventSynchronize(s.table_copied[snapshot]));
		s.table_staging[snapshot] = s.table_host;
		RT_HIP(ctx, hipMemcpyAsync(s.table_device, &s.table_staging[snapshot], sizeof(RtStreamTable), hipMemcpyHostToDevice, st));
		RT_HIP(ctx, hipEventRecord(s.table_copied[snapshot], st));
		s.table_dirty = false;
	}
	rt_launch_stream_advance(s.control, i, generated, s.progress + 2 * (i % RT_STREAM_PROGRESS_RING), s.reset_ring_first, s.reset_ring_count, st);
	s.reset_ring_count = 0;
	s.generated[i % RT_STREAM_PROGRESS_RING] = generated;
	RT_HIP(ctx, hipEventRecord(s.iteration_done[i % RT_STREAM_PROGRESS_RING], st));
	stage_mark(ctx, STAGE_TRACE, st);
	span_mark(ctx, SPAN_TRACE, st);
	rt_launch_trace_stream(p, ctx->trace_statistics ? ctx->trace_stats : nullptr, st);
	span_mark(ctx, SPAN_TRACE, st);
	if (ctx->trace_statistics && ctx->stream_history_rows < RT_STREAM_HISTORY_ROWS)
		RT_HIP(ctx, hipMemcpyAsync(ctx->stream_history + size_t(10) * ctx->stream_history_rows++, ctx->trace_stats, 10 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	stage_mark(ctx, STAGE_SORT, st);
	span_mark(ctx, SPAN_SORT, st);
	rt_launch_sort_stream(p, st);
	span_mark(ctx, SPAN_SORT, st);
	stage_mark(ctx, STAGE_SHADE, st);
	for (int m = 0; m < 4; m++) if (ctx->has_material[m]) { span_mark(ctx, SPAN_MATERIAL + m, st); rt_launch_material_stream(p, m, st); span_mark(ctx, SPAN_MATERIAL + m, st); }
	if (p.fog_active && p.config.enable_next_event_estimation) { stage_mark(ctx, STAGE_SHADOW, st); rt_launch_fog_attenuate_shadows_stream(p, st); }   // the shadow rays of this iteration (sort's scatter vertices, the material kernels' hits), before the next iteration traces them
	stage_mark(ctx, STAGE_END, st);
	s.iteration = i + 1;
	StreamSubmission done[RT_STREAM_MAX_BATCH]; int done_count = 0;
	while (!s.in_flight.empty() && s.in_flight.front().last <= i) {
		done[done_count++] = s.in_flight.front();
		s.in_flight.pop_front();
		if (done_count == RT_STREAM_MAX_BATCH || s.in_flight.empty() || s.in_flight.front().last > i) {
			int status = stream_complete(ctx, done, done_count, p); if (status) return status;
			done_count = 0;
		}
	}
	if (s.in_flight.empty()) s.base_iteration = s.iteration;
	RT_HIP(ctx, hipGetLastError());
	return RT_OK;
}

// Submissions that wait for company get their iteration now (before a setting they were made under changes).
int stream_launch_pending(rt_context * ctx) {
	if (!ctx->path_stream.created || ctx->path_stream.pending == 0) return RT_OK;
	(void)hipSetDevice(ctx->device);
	return stream_enqueue_iteration(ctx);
}

// Runs the wavefront until nothing is in flight (the calls that read results or change state need that).
hipError_t stream_flush(rt_context * ctx) {
	PathStream & s = ctx->path_stream;
	while (s.created && !s.in_flight.empty()) if (stream_enqueue_iteration(ctx) != RT_OK) return hipErrorUnknown;
	return hipSuccess;
}

// rt_render_samples under RT_SCHEDULER_MERGED
int stream_submit(rt_context * ctx, int sample_index, int sample_count, int range_offset, int range_count) {
	int status = stream_create(ctx); if (status) return status;
	PathStream & s = ctx->path_stream;
	const int num_bounces = ctx->params.config.num_bounces;
	const long long paths = (long long)range_count * sample_count;
	if (paths <= 0) return RT_OK;
	// submissions per iteration: one, unless the application pipelines frames and they are small
	// (SVGF frames: never, a frame inherits the g-buffers its predecessor's bounce 0 has written)
	const long long batch_paths = ctx->stream_batch_paths > 0 ? ctx->stream_batch_paths : (long long)RT_STREAM_BATCH_PATHS;
	const int batch = (ctx->frame_pipelining && !ctx->params.config.enable_svgf) ? int(std::min<long long>(RT_STREAM_MAX_BATCH, (batch_paths + paths - 1) / paths)) : 1;
	status = stream_ensure_frames(ctx, sample_count * (num_bounces + 1) * batch); if (status) return status;
	if (sample_count > s.frame_slots) return fail(ctx, RT_ERROR_OUT_OF_RANGE, "rt_render_samples: %d samples of a %zu pixel frame exceed the %d sample slots of the merged wavefront", sample_count, ctx->frame_pixels, s.frame_slots);
	// room for four iterations' worth of new paths -- or, for a declared burst of whole frames (rt_set_stream_batch), for the burst and a quarter: its frames
	// enter together and only die from then on (412 bytes per path: 21 GB for five 4-sample frames at 1080p instead of 68)
	const double room = batch_paths > (long long)RT_STREAM_BATCH_PATHS && paths * batch > (long long)RT_STREAM_BATCH_PATHS ? 1.25 : 4.0;
	if (size_t(paths * batch) > s.queues.capacity || !s.queues.allocated) { status = stream_ensure_queues(ctx, size_t(double(paths * batch) * room) + 1024); if (status) return status; }

	// admission: sample slots, a statistics ring entry, and room in the queues
	int slot_base = -1;
	for (;;) {
		bool ring_free = s.in_flight.size() < RT_STREAM_SUBMISSIONS - 1;
		slot_base = -1;
		const int legal_bases = s.frame_slots - sample_count + 1;   // every base 0 .. frame_slots - sample_count is tried, starting at next_slot (round robin)
		for (int start = 0; start < legal_bases && slot_base < 0; start++) {
			int candidate = ((s.next_slot < legal_bases ? s.next_slot : 0) + start) % legal_bases;
			bool free_run = true;
			for (int k = 0; k < sample_count; k++) if (s.slot_used[candidate + k]) { free_run = false; break; }
			if (free_run) slot_base = candidate;
		}
		bool fits = stream_bound(s) + s.pending_paths + paths <= (long long)s.queues.capacity;   // (with the submissions already waiting for the next iteration)
		if (ring_free && slot_base >= 0 && fits) break;
		if (!fits && s.known_iteration < s.iteration - 1 && s.iteration > s.base_iteration) { // the bound is stale: let the device catch up
			RT_HIP(ctx, hipEventSynchronize(s.iteration_done[(s.iteration - 1) % RT_STREAM_PROGRESS_RING]));
			continue;
		}
		if (s.in_flight.empty()) return fail(ctx, RT_ERROR_OUT_OF_RANGE, "rt_render_samples: the merged wavefront cannot take %lld paths (capacity %zu, %d sample slots)", paths, s.queues.capacity, s.frame_slots);
		status = stream_enqueue_iteration(ctx); if (status) return status;   // advance (with the submissions waiting, if any): paths die, submissions complete
	}

	StreamSubmission sub;
	sub.first_sample = sample_index; sub.sample_count = sample_count; sub.slot_base = slot_base;
	sub.ring = s.next_ring; s.next_ring = (s.next_ring + 1) % RT_STREAM_SUBMISSIONS;
	sub.birth = s.iteration; sub.last = s.iteration + num_bounces - 1; sub.paths = int(paths);
	sub.range_offset = range_offset; sub.range_count = range_count;
	sub.tile_pixels = ctx->params.tile_pixels; sub.tile_first = ctx->params.tile_first; sub.tile_stride = ctx->params.tile_stride;
	sub.list = ctx->pixel_list_on;
	for (int k = 0; k < sample_count; k++) {
		s.slot_used[slot_base + k] = true;
		s.table_host.slots[slot_base + k] = { sample_index + k, sub.birth, sub.ring, k };
	}
	s.next_slot = (slot_base + sample_count) % s.frame_slots;
	s.table_host.submission_birth[sub.ring] = sub.birth;
	// the table and the submission's (zeroed) statistics row travel with the iteration it joins (stream_enqueue_iteration): generate, the only kernel that runs
	// before that, reads neither
	if (s.reset_ring_count == 0) s.reset_ring_first = sub.ring;
	s.reset_ring_count++; s.table_dirty = true;
	if (ctx->trace_statistics && s.in_flight.empty()) { // statistics are per run of the wavefront
		RT_HIP(ctx, hipMemsetAsync(ctx->trace_stats, 0, 10 * sizeof(unsigned long long), s.stream));
		ctx->stream_history_rows = 0;
	}
	s.in_flight.push_back(sub);
	if (ctx->params.config.enable_svgf && s.gbuffers[0]) { // the frame starts from the g-buffers of the frame before it
		const void * from[3];
		for (int i = 0; i < 3; i++) {
			if (s.last_gbuffer_slot >= 0) from[i] = stream_gbuffer(ctx, i, s.last_gbuffer_slot);
			else from[i] = (ctx->last_slot > 0 && ctx->slots[ctx->last_slot].gbuffers[i]) ? ctx->slots[ctx->last_slot].gbuffers[i] : ctx->svgf_buffers[i]; // (the slot scheduler is drained)
			void * to = stream_gbuffer(ctx, i, slot_base);
			if (from[i] && from[i] != to) RT_HIP(ctx, hipMemcpyAsync(to, from[i], gbuffer_bytes(ctx, i), hipMemcpyDeviceToDevice, s.stream));
		}
		s.last_gbuffer_slot = slot_base;
	}
	status = stream_sync_tlas(ctx); if (status) return status;
	status = stream_generate(ctx, sub); if (status) return status;
	if (s.pending < batch && s.pending_paths < batch_paths) return RT_OK;   // wait for more of the same size
	return stream_enqueue_iteration(ctx);
}
