// rt_render.hip -- the part of the C ABI (include/gpu_raytracer_amd.h) that renders: the render entry points, and the per-submission ("slot") scheduler they run when the
// merged wavefront (rt_stream.hip) does not take the submission -- sample slots, the queue sets both schedulers allocate, the profiling marks, the
// wavefront launch loops of the path tracer and the AO integrator -- with the calls that drive or drain either scheduler and read its counters.
#include "rt_context.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// HIP multiplexes its streams onto 4 hardware queues unless GPU_MAX_HW_QUEUES says otherwise, and the variable is read when
// the HIP runtime initialises, i.e. at the first HIP call of the PROCESS. The per-submission scheduler keeps up to 2 x
// (submissions in flight) streams busy and loses their overlap silently when they share queues
// (profiles/r01_small_range_concurrency.txt). A library has no business editing its host's environment (and cannot know
// whether HIP is already up -- PyTorch imported first, say), and neither do the applications that ship with it: the queue
// slots of a GPU are shared by every process on it. The merged wavefront (the default scheduler) needs two streams; a
// context says so once when it is asked for more concurrent streams than the process has queues for.
static void warn_if_streams_share_queues(int streams_needed) {
	static bool warned = false;
	if (warned) return;
	const char * value = getenv("GPU_MAX_HW_QUEUES");
	const int queues = value ? atoi(value) : 4;
	if (queues >= streams_needed) return;
	warned = true;
	fprintf(stderr, "[grt] %d streams in flight but GPU_MAX_HW_QUEUES=%s: HIP will multiplex them onto %d hardware queues and serialise their kernels; "
	                "the merged scheduler (the default) needs two streams\n", streams_needed, value ? value : "(unset, 4)", queues);
}

#define RT_RAY_CURSOR_BYTES (RT_MAX_BOUNCES * 2 * sizeof(int))   // RtParams::ray_cursors of a slot: [RT_MAX_BOUNCES][2 (closest hit, shadow)] ints

// Every device array of a queue set as (pointer, bytes per entry), in declaration order, which is the allocation order.
template<typename Visit> static void for_each_queue_array(WavefrontQueues & q, Visit && visit) {
	auto vec3 = [&](RtVec3SoA & v) { visit((void **)&v.x, 4); visit((void **)&v.y, 4); visit((void **)&v.z, 4); };
	for (RtTraceBuffer & t : q.trace) {
		vec3(t.origin); vec3(t.direction); visit((void **)&t.hits, 16); visit((void **)&t.cone_angle, 4); visit((void **)&t.cone_width, 4);
		visit((void **)&t.medium, 4); visit((void **)&t.pixel_index_and_flags, 4); vec3(t.throughput); visit((void **)&t.last_pdf, 4);
	}
	for (RtMaterialBuffer & m : q.material) {
		vec3(m.direction); visit((void **)&m.hits, 16); visit((void **)&m.cone_angle, 4); visit((void **)&m.cone_width, 4);
		visit((void **)&m.medium, 4); visit((void **)&m.pixel_index_and_flags, 4); vec3(m.throughput);
	}
	vec3(q.shadow.origin); vec3(q.shadow.direction); visit((void **)&q.shadow.max_distance, 4); visit((void **)&q.shadow.illumination_and_pixel_index, 16);
}

// The kernels see a queue set through the parameter block.
void use_queues(RtParams & p, const WavefrontQueues & q) {
	memcpy(p.trace, q.trace, sizeof(p.trace)); memcpy(p.material, q.material, sizeof(p.material)); p.shadow = q.shadow;
}

int queues_allocate(rt_context * ctx, WavefrontQueues & q, size_t entries) {
	int status = RT_OK;
	for_each_queue_array(q, [&](void ** p, size_t bytes) { if (status == RT_OK) status = device_alloc(ctx, p, entries * bytes); });
	if (status) return status;
	q.capacity = entries;
	q.allocated = true;
	return RT_OK;
}
void queues_free(rt_context * ctx, WavefrontQueues & q) {
	for_each_queue_array(q, [&](void ** p, size_t) { device_free(ctx, *p); *p = nullptr; });
	q.allocated = false;
}

int ensure_slot(rt_context * ctx, int index) {
	SampleSlot & slot = ctx->slots[index];
	if (slot.created) return RT_OK;
	if (index > 0) warn_if_streams_share_queues(2 * (index + 1) + 2);   // two streams per slot, the main stream, the merged wavefront's
	RT_HIP(ctx, hipStreamCreateWithFlags(&slot.stream, hipStreamNonBlocking));
	RT_HIP(ctx, hipStreamCreateWithFlags(&slot.side,   hipStreamNonBlocking));
	RT_HIP(ctx, hipEventCreateWithFlags(&slot.ev_shaded,   hipEventDisableTiming));
	RT_HIP(ctx, hipEventCreateWithFlags(&slot.ev_shadowed, hipEventDisableTiming));
	RT_HIP(ctx, hipEventCreateWithFlags(&slot.ev_done,     hipEventDisableTiming));
	RT_HIP(ctx, hipEventCreate(&slot.ev_frame_start));
	RT_HIP(ctx, hipEventCreate(&slot.ev_frame_end));
	RT_HIP(ctx, hipEventCreateWithFlags(&slot.ev_gbuffers, hipEventDisableTiming));
	RT_HIP(ctx, hipEventRecord(slot.ev_done, slot.stream)); // so that waiting on a never-used slot is a no-op
	RT_HIP(ctx, hipEventRecord(slot.ev_gbuffers, slot.stream));
	int s = device_alloc(ctx, (void **)&slot.sizes, sizeof(RtBufferSizes)); if (s) return s;
	s = device_alloc(ctx, (void **)&slot.counter_totals, 6 * RT_MAX_BOUNCES * sizeof(int)); if (s) return s;
	s = device_alloc(ctx, (void **)&slot.ray_cursors, RT_RAY_CURSOR_BYTES); if (s) return s;
	// spill area for traversal stacks deeper than the LDS part: 24 entries x 8 B x (256 CUs x 8 workgroups x 256 lanes),
	// one per launch that can be resident at the same time
	for (int k = 0; k < 2; k++) { s = device_alloc(ctx, &slot.spill[k], size_t(24) * 8 * 256 * 8 * 256); if (s) return s; }
	RT_HIP(ctx, hipHostMalloc((void **)&slot.pinned_counters, sizeof(RtBufferSizes)));
	memset(slot.pinned_counters, 0, sizeof(RtBufferSizes));
	size_t bytes = ctx->frame_pixels * 16;
	if (index > 0 && bytes) for (int i = 0; i < RT_AOV_COUNT; i++) if (ctx->aov_buffers[i][0]) {
		s = device_alloc(ctx, &slot.aov_framebuffer[i], bytes); if (s) return s;
		RT_HIP(ctx, hipMemset(slot.aov_framebuffer[i], 0, bytes));
	}
	if (index > 0 && ctx->svgf_allocated) for (int i = 0; i < 3; i++) {
		s = device_alloc(ctx, &slot.gbuffers[i], gbuffer_bytes(ctx, i)); if (s) return s;
		RT_HIP(ctx, hipMemset(slot.gbuffers[i], 0, gbuffer_bytes(ctx, i)));
	}
	slot.created = true;
	return RT_OK;
}

// The kernels get RtParams by value: the context's block with one slot's per-sample pointers patched in.
RtParams slot_params(const rt_context * ctx, const SampleSlot & slot, int index) {
	RtParams p = ctx->params;
	use_queues(p, slot.queues);
	p.sizes = slot.sizes; p.ray_cursors = slot.ray_cursors; p.stack_spill = (uint2 *)slot.spill[0];
	if (index > 0) for (int i = 0; i < RT_AOV_COUNT; i++) p.aovs[i].framebuffer = (float4 *)slot.aov_framebuffer[i];
	if (index > 0 && slot.gbuffers[0]) {
		p.gbuffer_normal_and_depth        = (float4 *)slot.gbuffers[0];
		p.gbuffer_mesh_id_and_triangle_id = (int2   *)slot.gbuffers[1];
		p.gbuffer_screen_position_prev    = (float2 *)slot.gbuffers[2];
	}
	return p;
}

static size_t wanted_batch_size(const rt_context * ctx) {
	size_t frame = size_t(ctx->params.screen_width) * ctx->params.screen_height;
	size_t n = ctx->batch_size_request > 0 ? size_t(ctx->batch_size_request) : frame;
	if (n < 1) n = 1;
	return n;
}

int ensure_queues(rt_context * ctx, int slot_index, size_t pixels) {
	SampleSlot & slot = ctx->slots[slot_index];
	size_t n = pixels > 0 ? pixels : wanted_batch_size(ctx); // entries: pixels of a batch x samples per batch
	if (slot.queues.allocated && slot.queues.capacity >= n) return RT_OK;
	if (slot.queues.allocated) { // grow: release the old queues
		RT_HIP(ctx, quiesce(ctx));
		queues_free(ctx, slot.queues);
	}
	int s = queues_allocate(ctx, slot.queues, n); if (s) return s;
	if (slot_index == 0) use_queues(ctx->params, slot.queues);
	return RT_OK;
}

// Frame buffers of one slot for `samples` samples per batch (they only ever grow).
static int ensure_aov_batch(rt_context * ctx, int slot_index, int samples) {
	SampleSlot & slot = ctx->slots[slot_index];
	if (slot.aov_samples >= samples) return RT_OK;
	RT_HIP(ctx, quiesce(ctx));
	size_t bytes = ctx->frame_pixels * 16 * size_t(samples);
	for (int i = 0; i < RT_AOV_COUNT; i++) {
		void ** fb = slot_index == 0 ? &ctx->aov_buffers[i][0] : &slot.aov_framebuffer[i];
		if (!*fb) continue;
		device_free(ctx, *fb); *fb = nullptr;
		int s = device_alloc(ctx, fb, bytes); if (s) return s;
		RT_HIP(ctx, hipMemset(*fb, 0, bytes));
		if (slot_index == 0) ctx->params.aovs[i].framebuffer = (float4 *)*fb;
	}
	slot.aov_samples = samples;
	return RT_OK;
}

void stage_mark(rt_context * ctx, int kind, hipStream_t stream) {
	if (!ctx->profiling) return;
	if (ctx->stage_used == ctx->stage_events.size()) { hipEvent_t e; (void)hipEventCreate(&e); ctx->stage_events.push_back(e); ctx->stage_kinds.push_back(0); }
	ctx->stage_kinds[ctx->stage_used] = kind;
	(void)hipEventRecord(ctx->stage_events[ctx->stage_used++], stream);
}

// mode 2: an event on the launch's own stream before and after it (does not order other streams)
void span_mark(rt_context * ctx, int kind, hipStream_t stream) {
	if (!ctx->time_this_sample) return;
	if (kind != SPAN_TRACE && kind != SPAN_SHADOW && !ctx->launch_timing_all) return;
	if (ctx->span_used == ctx->span_events.size()) { hipEvent_t e; (void)hipEventCreate(&e); ctx->span_events.push_back(e); ctx->span_kinds.push_back(0); }
	ctx->span_kinds[ctx->span_used] = kind;
	(void)hipEventRecord(ctx->span_events[ctx->span_used++], stream);
}

// One batch's queue sizes, added to the submission's totals. (C linkage: the code object and the kernel traces under profiles/ name it plainly.)
extern "C" __global__ void kernel_accumulate_counters(const RtBufferSizes * sizes, int * totals) {
	int b = threadIdx.x;
	if (b >= RT_MAX_BOUNCES) return;
	totals[0 * RT_MAX_BOUNCES + b] += sizes->trace[b];
	totals[1 * RT_MAX_BOUNCES + b] += sizes->shadow[b];
	totals[2 * RT_MAX_BOUNCES + b] += sizes->diffuse[b];
	totals[3 * RT_MAX_BOUNCES + b] += sizes->plastic[b];
	totals[4 * RT_MAX_BOUNCES + b] += sizes->dielectric[b];
	totals[5 * RT_MAX_BOUNCES + b] += sizes->conductor[b];
}

// The end of a slot-scheduler submission on slot `slot_index`: its counters travel to pinned memory, its end is recorded,
// and the scene versions it read stay in use until it is done.
static int finish_slot_submission(rt_context * ctx, int slot_index) {
	SampleSlot & slot = ctx->slots[slot_index];
	hipStream_t st = slot.stream;
	RT_HIP(ctx, hipMemcpyAsync(slot.pinned_counters, slot.counter_totals, 6 * RT_MAX_BOUNCES * sizeof(int), hipMemcpyDeviceToHost, st));
	RT_HIP(ctx, hipEventRecord(slot.ev_frame_end, st));
	RT_HIP(ctx, hipEventRecord(slot.ev_done, st));
	int status = mark_scene_versions_in_use(ctx, slot_index, st); if (status) return status;
	ctx->last_slot = slot_index;
	RT_HIP(ctx, hipGetLastError());
	return RT_OK;
}

extern "C" {

int rt_render_sample(rt_context * ctx, int sample_index) { return rt_render_samples(ctx, sample_index, 1); }

// The accumulate step of a batch: one submission, its frames at slot 0, cleared by the caller after the launch.
static RtAccumulate batch_accumulate(int sample_index, int sample_count, int range_offset, int range_count, float4 * moments, const RtFireflyTiers & tiers) {
	RtAccumulate a = { };
	a.group.count = 1; a.group.first_sample[0] = sample_index; a.group.sample_count[0] = sample_count;
	a.pixel_offset = range_offset; a.pixel_count = range_count; a.moments = moments; a.tiers = tiers;
	return a;
}

int rt_render_samples(rt_context * ctx, int sample_index, int sample_count) {
	RT_REQUIRE(ctx, ctx, "rt_render_sample: NULL context");
	RT_REQUIRE(ctx, sample_count >= 1 && sample_count <= RT_MAX_BATCH_SAMPLES, "rt_render_samples: sample_count must be 1..16");
	(void)hipSetDevice(ctx->device);
	int s = check_ready(ctx, "rt_render_sample", NEED_SCENE | NEED_MATERIALS | NEED_RNG | NEED_SKY | NEED_FRAME); if (s) return s;
	if (ctx->bvh_width != 8 && ctx->trace_statistics) return fail(ctx, RT_ERROR_NOT_READY, "rt_render_sample: trace statistics exist for the CWBVH kernels only");
	// Slot choice: round-robin over the samples in flight. Profiling / statistics passes use one slot,
	// serialised. SVGF frames pipeline like plain samples under either scheduler: only their filter stage is ordered.
	// Scheduler (see rt_set_scheduler): the merged wavefront where its kernels exist
	const bool merged = ctx->scheduler == RT_SCHEDULER_MERGED && ctx->params.config.num_bounces > 0 && ctx->bvh_width == 8
	                    && !(ctx->params.config.enable_svgf && ctx->defer_filter) // the tile split of SVGF frames exchanges the filter's inputs per frame
	                    && !(ctx->batch_size_request > 0); // explicit pixel batches (a VRAM bound of the reference) are a slot-scheduler feature
	if (ctx->params.config.enable_svgf && ctx->params.fog_active) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: a fog volume (rt_set_fog_volume) cannot be rendered with enable_svgf: a scatter vertex has no g-buffer");
	if (ctx->params.config.enable_svgf && sample_count != 1) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: SVGF frames are rendered one sample at a time");
	if (ctx->pixel_list_on) {   // a refusal, never a silent uniform render: the list kernels exist for the merged wavefront's plain frames, and a pixel's own count starts at w >= 1
		if (ctx->scheduler != RT_SCHEDULER_MERGED) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: a pixel list (rt_set_pixel_list) needs RT_SCHEDULER_MERGED");
		if (!merged) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: a pixel list (rt_set_pixel_list) needs the merged wavefront, which this context does not take (num_bounces 0, a BVH other than CWBVH, or an explicit pixel batch size)");
		if (ctx->params.config.enable_svgf) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: SVGF frames cannot cover a pixel list (rt_set_pixel_list)");
		if (sample_index < 2) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_samples: a pixel list (rt_set_pixel_list) continues a progression, sample_index %d is below 2", sample_index);
	}
	else if (sample_index < 2 && ctx->pixel_list_selected) pixel_list_drop(ctx);   // a uniform sample 0 or 1 starts the pixels' moments over: a selection made from the ones before says nothing about them
	if (merged != ctx->last_render_merged) { RT_HIP(ctx, quiesce(ctx)); ctx->last_render_merged = merged; }
	if (ctx->has_material[2] || ctx->has_material[3]) { s = ensure_luts(ctx); if (s) return s; }
	s = sky_sampling_prepare(ctx, "rt_render_sample"); if (s) return s;
	if (size_t(sample_count) * ctx->frame_pixels >= (1u << 30)) return fail(ctx, RT_ERROR_OUT_OF_RANGE, "rt_render_samples: %d samples of a %zu pixel frame exceed the 30-bit path index", sample_count, ctx->frame_pixels);
	int range_offset = 0, range_count = 0;
	s = resolve_pixel_range(ctx, "rt_render_sample", &range_offset, &range_count); if (s) return s;
	if (merged) {
		ctx->time_this_sample = ctx->launch_timing;
		return stream_submit(ctx, sample_index, sample_count, range_offset, range_count);
	}
	bool exclusive = ctx->profiling || ctx->trace_statistics || ctx->defer_filter;
	int slot_index = exclusive ? 0 : int(ctx->render_counter++ % unsigned(ctx->samples_in_flight));
	s = ensure_slot(ctx, slot_index); if (s) return s;
	SampleSlot & slot = ctx->slots[slot_index];
	s = ensure_aov_batch(ctx, slot_index, sample_count); if (s) return s;
	int batch_limit = int(wanted_batch_size(ctx));
	int batch_size  = range_count < batch_limit ? range_count : batch_limit; // pixels per wavefront batch; each carries sample_count paths
	s = ensure_queues(ctx, slot_index, size_t(batch_size > 0 ? batch_size : 1) * sample_count); if (s) return s;
	RtParams p = slot_params(ctx, slot, slot_index);
	p.batch_samples = sample_count;
	RtParams p_shadow = p; p_shadow.stack_spill = (uint2 *)slot.spill[1]; // the shadow launch may be resident together with the next closest-hit launch

	ctx->time_this_sample = ctx->launch_timing;
	hipStream_t st = slot.stream;
	// The wavefront part depends on nothing the main stream does asynchronously (uploads and the LUT
	// integration synchronise); only the accumulate step below has to follow the main-stream work
	// submitted so far (rt_pack_pixels of the previous frame reads, rt_unpack_pixels writes the image).
	RT_HIP(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
	// ... and it reads the scene version that is current now (asynchronous TLAS / instance uploads)
	RT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_scene, 0));

	if (exclusive) for (int k = 1; k < RT_MAX_SAMPLE_SLOTS; k++) if (ctx->slots[k].created) RT_HIP(ctx, hipStreamWaitEvent(st, ctx->slots[k].ev_done, 0));

	ctx->stage_used = 0;
	RT_HIP(ctx, hipEventRecord(slot.ev_frame_start, st));
	const bool svgf = p.config.enable_svgf != 0;
	if (svgf && ctx->path_stream.last_gbuffer_slot >= 0) { // the previous frame went through the merged wavefront (which is drained by now)
		stream_save_gbuffers(ctx);                            // ... into the set of slot 0 (a blocking copy)
	}
	if (svgf && ctx->last_slot >= 0 && ctx->last_slot != slot_index) { // inherit the g-buffers of the previous frame
		SampleSlot & prev = ctx->slots[ctx->last_slot];
		void * from[3] = { ctx->last_slot == 0 ? ctx->svgf_buffers[0] : prev.gbuffers[0], ctx->last_slot == 0 ? ctx->svgf_buffers[1] : prev.gbuffers[1], ctx->last_slot == 0 ? ctx->svgf_buffers[2] : prev.gbuffers[2] };
		void * to[3]   = { p.gbuffer_normal_and_depth, p.gbuffer_mesh_id_and_triangle_id, p.gbuffer_screen_position_prev };
		if (prev.created) RT_HIP(ctx, hipStreamWaitEvent(st, prev.ev_gbuffers, 0));
		for (int i = 0; i < 3; i++) if (from[i] && to[i] && from[i] != to[i]) RT_HIP(ctx, hipMemcpyAsync(to[i], from[i], gbuffer_bytes(ctx, i), hipMemcpyDeviceToDevice, st));
	}

	bool trace_shadows = p.config.enable_next_event_estimation && ((ctx->has_lights && p.lights_total_weight > 0.0f) || rt_light_samples_split(p) || p.fog_active);   // (sky importance sampling, delta lights: shadow rays without emitters; a fog volume: whenever NEE is on)
	const bool fog_shadows = trace_shadows && p.fog_active;   // the queue passes through the fog's attenuation pass on the stream that traces it
	// Shadow rays of bounce b only feed the frame buffers, so they run on the side stream while the
	// main chain traces bounce b+1; they are joined before the next kernel that touches the frame
	// buffers (sort: sky / emissive hits), which keeps the order of the float additions per pixel.
	bool overlap = trace_shadows && !ctx->profiling && !ctx->trace_statistics;

	// generate -> (trace, sort, shade, shadow) x bounces for every batch of the range, on st (+ side)
	RT_HIP(ctx, hipMemsetAsync(slot.counter_totals, 0, 6 * RT_MAX_BOUNCES * sizeof(int), st));
	if (ctx->trace_statistics) RT_HIP(ctx, hipMemsetAsync(ctx->trace_stats, 0, 10 * sizeof(unsigned long long), st));
	int pixels_left = range_count;
	bool shadow_pending = false;
	while (pixels_left > 0) {
		int pixel_offset = range_offset + (range_count - pixels_left);
		int pixel_count  = batch_size < pixels_left ? batch_size : pixels_left;

		if (shadow_pending) { RT_HIP(ctx, hipStreamWaitEvent(st, slot.ev_shadowed, 0)); shadow_pending = false; } // the previous batch's queues are reused
		RT_HIP(ctx, hipMemsetAsync(slot.sizes, 0, sizeof(RtBufferSizes), st));
		RT_HIP(ctx, hipMemsetAsync(slot.ray_cursors, 0, RT_RAY_CURSOR_BYTES, st));
		stage_mark(ctx, STAGE_GENERATE, st);
		rt_launch_generate(p, sample_index, pixel_offset, pixel_count, st);

		for (int bounce = 0; bounce < p.config.num_bounces; bounce++) {
			stage_mark(ctx, STAGE_TRACE, st);
			if (ctx->trace_statistics) rt_launch_trace_counting(p, bounce, ctx->trace_stats, st);
			else { span_mark(ctx, SPAN_TRACE, st); rt_launch_trace(p, bounce, st); span_mark(ctx, SPAN_TRACE, st); }
			if (shadow_pending) { RT_HIP(ctx, hipStreamWaitEvent(st, slot.ev_shadowed, 0)); shadow_pending = false; }
			stage_mark(ctx, STAGE_SORT, st);
			rt_launch_sort(p, bounce, sample_index, st);
			stage_mark(ctx, STAGE_SHADE, st);
			for (int m = 0; m < 4; m++) if (ctx->has_material[m]) rt_launch_material(p, m, bounce, sample_index, st);
			if (svgf && bounce == 0 && pixels_left <= batch_size) RT_HIP(ctx, hipEventRecord(slot.ev_gbuffers, st)); // last pixel batch: the g-buffers of this frame are complete
			if (trace_shadows) {
				stage_mark(ctx, STAGE_SHADOW, st);
				if (fog_shadows && !overlap) rt_launch_fog_attenuate_shadows(p, bounce, st);
				if (ctx->trace_statistics) rt_launch_trace_shadow_counting(p, bounce, ctx->trace_stats, st);
				else if (!overlap) rt_launch_trace_shadow(p, bounce, st);
				else {
					RT_HIP(ctx, hipEventRecord(slot.ev_shaded, st));
					RT_HIP(ctx, hipStreamWaitEvent(slot.side, slot.ev_shaded, 0));
					if (fog_shadows) rt_launch_fog_attenuate_shadows(p_shadow, bounce, slot.side);
					span_mark(ctx, SPAN_SHADOW, slot.side);
					rt_launch_trace_shadow(p_shadow, bounce, slot.side);
					span_mark(ctx, SPAN_SHADOW, slot.side);
					RT_HIP(ctx, hipEventRecord(slot.ev_shadowed, slot.side));
					shadow_pending = true;
				}
			}
		}
		hipLaunchKernelGGL(kernel_accumulate_counters, dim3(1), dim3(RT_MAX_BOUNCES), 0, st, slot.sizes, slot.counter_totals);
		pixels_left -= batch_size;
	}
	if (shadow_pending) RT_HIP(ctx, hipStreamWaitEvent(st, slot.ev_shadowed, 0));

	// The accumulate step folds this sample into the shared accumulators: strictly in sample order.
	RT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_main, 0));
	if (ctx->last_slot >= 0 && ctx->last_slot != slot_index && ctx->slots[ctx->last_slot].created) RT_HIP(ctx, hipStreamWaitEvent(st, ctx->slots[ctx->last_slot].ev_done, 0));
	stage_mark(ctx, STAGE_POST, st);
	const bool deferred = p.config.enable_svgf && ctx->defer_filter; // rt_filter_frame does the rest once the ranks have exchanged their tiles
	if (deferred) { }
	else if (p.config.enable_svgf) { p.taa_frame_prev = ctx->params.taa_frame_prev; p.taa_frame_next = ctx->params.taa_frame_next; rt_launch_svgf_taa(p, sample_index, st); if (p.config.enable_taa) std::swap(ctx->params.taa_frame_prev, ctx->params.taa_frame_next); }
	else rt_launch_accumulate(p, batch_accumulate(sample_index, sample_count, range_offset, range_count, noise_moments_for(ctx, p), firefly_tiers_for(ctx, p)), st);
	stage_mark(ctx, STAGE_END, st);

	// aovs_clear_to_zero (Integrator.cpp:379-385)
	if (!deferred) for (int i = 0; i < RT_AOV_COUNT; i++) if (p.aovs[i].framebuffer) RT_HIP(ctx, hipMemsetAsync(p.aovs[i].framebuffer, 0, ctx->frame_pixels * 16 * sample_count, st));
	return finish_slot_submission(ctx, slot_index);
}

// Ambient-occlusion integrator (AO::render, Integrators/AO.cpp:148-200): generate -> trace ->
// kernel_ambient_occlusion -> shadow trace (sets RADIANCE) per batch, then accumulate. One sample at
// a time on slot 0; it shares the queues, the trace kernels and the accumulate kernel of the path tracer.
int rt_render_ao_sample(rt_context * ctx, int sample_index, float ao_radius) {
	RT_REQUIRE(ctx, ctx, "rt_render_ao_sample: NULL context");
	RT_REQUIRE(ctx, ao_radius > 0.0f, "rt_render_ao_sample: ao_radius must be positive");
	(void)hipSetDevice(ctx->device);
	int s = check_ready(ctx, "rt_render_ao_sample", NEED_SCENE | NEED_RNG | NEED_FRAME); if (s) return s;
	if (ctx->params.tile_pixels > 0) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_ao_sample: tile mode is not supported, use rt_set_pixel_range");
	if (ctx->pixel_list_on) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_render_ao_sample: the AO integrator cannot cover a pixel list (rt_set_pixel_list)");
	int range_offset = 0, range_count = 0;
	s = resolve_pixel_range(ctx, "rt_render_ao_sample", &range_offset, &range_count); if (s) return s;

	if (ctx->last_render_merged) { RT_HIP(ctx, quiesce(ctx)); ctx->last_render_merged = false; } // this integrator runs on slot 0
	s = ensure_slot(ctx, 0); if (s) return s;
	int batch_limit = int(wanted_batch_size(ctx));
	int batch_size  = range_count < batch_limit ? range_count : batch_limit;
	s = ensure_queues(ctx, 0, size_t(batch_size > 0 ? batch_size : 1)); if (s) return s;
	SampleSlot & slot = ctx->slots[0];
	RtParams p = slot_params(ctx, slot, 0);
	p.batch_samples = 1;
	p.config.enable_svgf = 0; // the AO integrator has no SVGF path; the TAA jitter of kernel_generate stays off

	hipStream_t st = slot.stream;
	RT_HIP(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
	RT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_main, 0));

	for (int k = 1; k < RT_MAX_SAMPLE_SLOTS; k++) if (ctx->slots[k].created) RT_HIP(ctx, hipStreamWaitEvent(st, ctx->slots[k].ev_done, 0));

	RT_HIP(ctx, hipEventRecord(slot.ev_frame_start, st));
	RT_HIP(ctx, hipMemsetAsync(slot.counter_totals, 0, 6 * RT_MAX_BOUNCES * sizeof(int), st));
	int pixels_left = range_count;
	while (pixels_left > 0) {
		int pixel_offset = range_offset + (range_count - pixels_left);
		int pixel_count  = batch_size < pixels_left ? batch_size : pixels_left;
		RT_HIP(ctx, hipMemsetAsync(slot.sizes, 0, sizeof(RtBufferSizes), st));
		RT_HIP(ctx, hipMemsetAsync(slot.ray_cursors, 0, RT_RAY_CURSOR_BYTES, st));
		rt_launch_generate(p, sample_index, pixel_offset, pixel_count, st);
		rt_launch_trace(p, 0, st);
		rt_launch_ambient_occlusion(p, sample_index, ao_radius, st);
		rt_launch_trace_shadow_ao(p, st);
		hipLaunchKernelGGL(kernel_accumulate_counters, dim3(1), dim3(RT_MAX_BOUNCES), 0, st, slot.sizes, slot.counter_totals);
		pixels_left -= batch_size;
	}
	RtParams p_acc = p; // kernel_accumulate of AO.cu:161-183 folds RADIANCE, NORMAL and POSITION only
	p_acc.aovs[RT_AOV_ALBEDO].framebuffer = nullptr;
	ctx->folds++;   // (the mean moves: a resolved image is older than the frame from here on)
	rt_launch_accumulate(p_acc, batch_accumulate(sample_index, 1, range_offset, range_count, nullptr, { }), st);
	for (int i = 0; i < RT_AOV_COUNT; i++) if (p.aovs[i].framebuffer) RT_HIP(ctx, hipMemsetAsync(p.aovs[i].framebuffer, 0, ctx->frame_pixels * 16, st));
	return finish_slot_submission(ctx, 0);
}

int rt_set_pixel_query(rt_context * ctx, int pixel_index) {
	RT_REQUIRE(ctx, ctx, "rt_set_pixel_query: NULL context");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemset(ctx->pixel_query_out, 0xff, 2 * sizeof(int))); // { INVALID, INVALID }
	ctx->params.pixel_query_pixel = pixel_index;
	return RT_OK;
}

int rt_get_pixel_query(rt_context * ctx, int * mesh_id, int * triangle_id) {
	RT_REQUIRE(ctx, ctx && mesh_id && triangle_id, "rt_get_pixel_query: NULL argument");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	int out[2] = { -1, -1 };
	RT_HIP(ctx, hipMemcpy(out, ctx->pixel_query_out, sizeof(out), hipMemcpyDeviceToHost));
	*mesh_id = out[0]; *triangle_id = out[1];
	return RT_OK;
}

int rt_set_samples_in_flight(rt_context * ctx, int count) {
	RT_REQUIRE(ctx, ctx && count >= 1 && count <= RT_MAX_SAMPLE_SLOTS, "rt_set_samples_in_flight: count must be 1..8");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	ctx->samples_in_flight = count;
	return RT_OK;
}

int rt_advance(rt_context * ctx) {
	RT_REQUIRE(ctx, ctx, "rt_advance: NULL context");
	(void)hipSetDevice(ctx->device);
	if (!ctx->path_stream.created || ctx->path_stream.in_flight.empty()) return RT_OK;
	ctx->time_this_sample = ctx->launch_timing;
	return stream_enqueue_iteration(ctx);
}

int rt_submissions_completed(rt_context * ctx, uint64_t * out_count) {
	RT_REQUIRE(ctx, ctx && out_count, "rt_submissions_completed: NULL argument");
	*out_count = ctx->path_stream.submissions_completed;
	return RT_OK;
}

int rt_synchronize(rt_context * ctx) {
	RT_REQUIRE(ctx, ctx, "rt_synchronize: NULL context");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	return RT_OK;
}

int rt_get_counters(rt_context * ctx, rt_counters * out) {
	RT_REQUIRE(ctx, ctx && out, "rt_get_counters: NULL argument");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	rt_counters c; memset(&c, 0, sizeof(c));
	float ms = 0.0f;
	if (ctx->last_render_merged && ctx->path_stream.last_completed_ring >= 0) { // the last submission the merged wavefront completed
		const PathStream & s = ctx->path_stream;
		const int * row = s.stats_host + size_t(s.last_completed_ring) * RT_STREAM_STATS_ROW;
		memcpy(c.trace,      row + RT_STAT_TRACE      * RT_MAX_BOUNCES, sizeof(c.trace));
		memcpy(c.shadow,     row + RT_STAT_SHADOW     * RT_MAX_BOUNCES, sizeof(c.shadow));
		memcpy(c.diffuse,    row + RT_STAT_DIFFUSE    * RT_MAX_BOUNCES, sizeof(c.diffuse));
		memcpy(c.plastic,    row + RT_STAT_PLASTIC    * RT_MAX_BOUNCES, sizeof(c.plastic));
		memcpy(c.dielectric, row + RT_STAT_DIELECTRIC * RT_MAX_BOUNCES, sizeof(c.dielectric));
		memcpy(c.conductor,  row + RT_STAT_CONDUCTOR  * RT_MAX_BOUNCES, sizeof(c.conductor));
		if (hipEventElapsedTime(&ms, s.ev_begin[s.last_completed_ring], s.ev_end[s.last_completed_ring]) == hipSuccess) c.ms_total = ms;
	} else {
		const SampleSlot & slot = ctx->slots[ctx->last_slot < 0 ? 0 : ctx->last_slot];
		const int * totals = (const int *)slot.pinned_counters;
		memcpy(c.trace,      totals + 0 * RT_MAX_BOUNCES, sizeof(c.trace));
		memcpy(c.shadow,     totals + 1 * RT_MAX_BOUNCES, sizeof(c.shadow));
		memcpy(c.diffuse,    totals + 2 * RT_MAX_BOUNCES, sizeof(c.diffuse));
		memcpy(c.plastic,    totals + 3 * RT_MAX_BOUNCES, sizeof(c.plastic));
		memcpy(c.dielectric, totals + 4 * RT_MAX_BOUNCES, sizeof(c.dielectric));
		memcpy(c.conductor,  totals + 5 * RT_MAX_BOUNCES, sizeof(c.conductor));
		if (hipEventElapsedTime(&ms, slot.ev_frame_start, slot.ev_frame_end) == hipSuccess) c.ms_total = ms;
	}
	if (ctx->launch_timing) { // sums over every launch since the mode was enabled (rt_get_launch_timings returns each and starts over)
		for (size_t i = 0; i + 1 < ctx->span_used; i += 2) {
			float d = 0.0f;
			if (hipEventElapsedTime(&d, ctx->span_events[i], ctx->span_events[i + 1]) == hipSuccess) { if (ctx->span_kinds[i] == SPAN_TRACE) c.ms_trace += d; else if (ctx->span_kinds[i] == SPAN_SHADOW) c.ms_shadow += d; }
		}
	}
	if (ctx->profiling) {
		float * bucket[STAGE_END] = { &c.ms_generate, &c.ms_trace, &c.ms_sort, &c.ms_shade, &c.ms_shadow, &c.ms_post };
		static const bool print_stages = getenv("GRT_STAGE_TRACE") != nullptr; // one line per launch group, in submission order
		static const char * stage_names[STAGE_END] = { "generate", "trace", "sort", "shade", "shadow", "post" };
		for (size_t i = 0; i + 1 < ctx->stage_used; i++) {
			float d = 0.0f;
			if (hipEventElapsedTime(&d, ctx->stage_events[i], ctx->stage_events[i + 1]) == hipSuccess && ctx->stage_kinds[i] < STAGE_END) {
				*bucket[ctx->stage_kinds[i]] += d;
				if (print_stages) fprintf(stderr, "[grt] stage %-8s %8.4f ms\n", stage_names[ctx->stage_kinds[i]], d);
			}
		}
		if (ctx->last_render_merged) ctx->stage_used = 0; // the merged wavefront's stage events add up over its iterations until they are read
	}
	ctx->last_counters = c;
	*out = c;
	return RT_OK;
}

} // extern "C"
