// rt_probes.hip -- the kernel-level entry points of include/gpu_raytracer_amd.h ("probes"): one kernel, or one launch of a frame, on explicit
// arguments, for the tests and for bench.py. All are synchronous. In order: the scaffold every probe stands on (Probe, with the codec of the queue
// records rt_context.h describes; PixelsOnce), the trace and generate probes, the one-array-in, one-array-out probes, the sort, fog and material launch
// probes on their shared front and back (QueueLaunch, LaunchCounters, LaunchFrames), and the image probes (accumulate, noise, selection, denoise, fireflies).
#include "rt_context.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

// What every probe does around its launch, written once: device copies of the caller's arrays and device arrays for the results, ONE check that
// they all exist, the end of the launch, the read-backs, and a pair of timing events. Everything is released on every path.
namespace {
struct Probe {
	rt_context * ctx; const char * name;   // the entry point's, for its messages
	std::vector<void *> arrays; bool failed = false;
	hipEvent_t begin = nullptr, end = nullptr;
	Probe(rt_context * c, const char * n) : ctx(c), name(n) { }
	~Probe() { for (void * p : arrays) (void)hipFree(p); for (hipEvent_t e : { begin, end }) if (e) (void)hipEventDestroy(e); }
	// `count` elements on the device: a copy of the caller's `src`, or room for a result (src == nullptr)
	template<typename T> T * array(size_t count, const void * src = nullptr) {
		void * p = nullptr; const size_t bytes = count * sizeof(T);
		if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { failed = true; return nullptr; }
		arrays.push_back(p);
		if (src && bytes && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) failed = true;
		return (T *)p;
	}
	RtVec3SoA vec3(size_t count, const float * x, const float * y, const float * z) { return { array<float>(count, x), array<float>(count, y), array<float>(count, z) }; }
	// the one check after the last array()
	int allocated() { return failed ? fail(ctx, RT_ERROR_HIP, "%s: device allocation failed", name) : RT_OK; }
	// after the launch: its error, then the wait -- for everything the context has in flight (the probes on the main stream), or for `own` alone
	int finish(hipStream_t own = nullptr) {
		RT_HIP(ctx, hipGetLastError());
		if (own) RT_HIP(ctx, hipStreamSynchronize(own)); else RT_HIP(ctx, quiesce(ctx));
		return RT_OK;
	}
	int read(void * dst, const void * src, size_t bytes) { RT_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return RT_OK; }
	int finish_and_read(void * dst, const void * src, size_t bytes) { int s = finish(); return s ? s : read(dst, src, bytes); }   // (main stream, one result)
	// `count` 32-bit words: a copy of the caller's `src`, or (src == nullptr) all `sentinel`
	void * words(size_t count, const void * src, uint32_t sentinel) {
		if (!src) staging.assign(count, sentinel);
		return array<uint32_t>(count, src ? src : staging.data());
	}
	// A queue of `capacity` entries (the launch probes; B: RtTraceBuffer, RtMaterialBuffer or RtShadowBuffer, its record in rt_context.h's RecordLayout<B>) from `n`
	// records; every word of the arrays beyond them holds `sentinel` ...
	template<typename B> B queue(const uint32_t * records, size_t n, size_t capacity, uint32_t sentinel) {
		B b = { };
		for (const RecordField & f : RecordLayout<B>::fields) {
			staging.assign(std::max(capacity, size_t(1)) * f.words, sentinel);
			for (size_t i = 0; i < n; i++) for (int w = 0; w < f.words; w++) staging[i * f.words + w] = records[i * RecordLayout<B>::words + f.word + w];
			void * p = array<uint32_t>(capacity * f.words, staging.data());
			memcpy((char *)&b + f.member, &p, sizeof p);
		}
		return b;
	}
	// ... an output queue, all sentinel ...
	template<typename B> B queue(size_t capacity, uint32_t sentinel) { return queue<B>(nullptr, 0, capacity, sentinel); }
	// ... and back: the whole arrays into `capacity` records, whose padding words get `sentinel`
	template<typename B> bool queue_back(const B & b, uint32_t * records, size_t capacity, uint32_t sentinel) {
		const size_t stride = RecordLayout<B>::words;
		std::fill(records, records + capacity * stride, sentinel);
		for (const RecordField & f : RecordLayout<B>::fields) {
			void * p; memcpy(&p, (const char *)&b + f.member, sizeof p);
			staging.resize(std::max(capacity, size_t(1)) * f.words);
			if (read(staging.data(), p, capacity * f.words * 4)) return false;
			for (size_t i = 0; i < capacity; i++) for (int w = 0; w < f.words; w++) records[i * stride + f.word + w] = staging[i * f.words + w];
		}
		return true;
	}
	std::vector<uint32_t> staging;
	// *ms: the time of `launch` (main stream), waited for
	template<typename Launch> int time(float * ms, Launch && launch) {
		if (!begin) RT_HIP(ctx, hipEventCreate(&begin));
		if (!end) RT_HIP(ctx, hipEventCreate(&end));
		RT_HIP(ctx, hipEventRecord(begin, ctx->stream));
		launch();
		RT_HIP(ctx, hipEventRecord(end, ctx->stream));
		RT_HIP(ctx, quiesce(ctx));
		RT_HIP(ctx, hipEventElapsedTime(ms, begin, end));
		return RT_OK;
	}
};

// "Every pixel in range and named once", for the probes whose launch writes a pixel per entry without an atomic: name() says what an entry's pixel is, and
// the caller words its own refusal.
struct PixelsOnce {
	enum Named { FRESH, BEYOND, TWICE };
	std::vector<uint8_t> seen; size_t pixels;
	explicit PixelsOnce(size_t n) : seen((n + 7) / 8, 0), pixels(n) { }
	Named name(size_t pixel) {
		if (pixel >= pixels) return BEYOND;
		const uint8_t bit = uint8_t(1u << (pixel & 7));
		if (seen[pixel >> 3] & bit) return TWICE;
		seen[pixel >> 3] |= bit;
		return FRESH;
	}
};
} // namespace

// The repeat / timing loop of the explicit-ray entry points around `launch` (one traversal on the main stream):
// *out_ms gets the mean time of `repeat` launches.
template<typename Launch> static int time_explicit_launches(Probe & probe, int repeat, float * out_ms, Launch && launch) {
	rt_context * ctx = probe.ctx;
	if (repeat < 1) repeat = 1;
	float total = 0.0f;
	for (int r = 0; r < repeat; r++) {
		RT_HIP(ctx, hipMemsetAsync(ctx->explicit_retired, 0, 8 * sizeof(int), ctx->stream));
		float ms = 0.0f; int s = probe.time(&ms, launch); if (s) return s;
		total += ms;
	}
	RT_HIP(ctx, hipGetLastError());
	if (out_ms) *out_ms = total / float(repeat);
	return RT_OK;
}

// The queues and frames of the two trace-launch probes (rt_trace_stream_rays, rt_trace_queue_rays) as the caller gave them ...
namespace {
struct TraceQueueArgs {
	const float * origin[3], * direction[3]; size_t closest_count; uint32_t * hits;
	const float * shadow_origin[3], * shadow_direction[3], * max_distance; size_t shadow_count;
	const float4 * light;        // per shadow ray: illumination and pixel word, as the shade kernels queue them
	float * frames[3];           // RADIANCE, RADIANCE_DIRECT, RADIANCE_INDIRECT: frame_pixels float4 each; NULL: the launch has no such frame
	size_t frame_pixels;
	uint64_t * stats10;          // NULL, or the counting kernels' ten words
};
const int trace_queue_frame_aov[3] = { RT_AOV_RADIANCE, RT_AOV_RADIANCE_DIRECT, RT_AOV_RADIANCE_INDIRECT };
static_assert(RT_TRACE_QUEUE_FLAG_BOUNCE_0 == RT_SHADOW_FLAG_BOUNCE_0, "the public header names the kernels' flag");
// ... and on the device: every array is the caller's before the launch (a hit record or a pixel the launch never writes keeps its value) and read back whole after it
struct TraceQueueBuffers {
	RtTraceBuffer trace = { }; RtShadowBuffer shadow = { }; float4 * frames[3] = { nullptr, nullptr, nullptr }; unsigned long long * stats = nullptr;
	void upload(Probe & probe, const TraceQueueArgs & a) {
		trace.origin = probe.vec3(a.closest_count, a.origin[0], a.origin[1], a.origin[2]); trace.direction = probe.vec3(a.closest_count, a.direction[0], a.direction[1], a.direction[2]);
		trace.hits = probe.array<uint4>(a.closest_count, a.hits);
		shadow.origin = probe.vec3(a.shadow_count, a.shadow_origin[0], a.shadow_origin[1], a.shadow_origin[2]);
		shadow.direction = probe.vec3(a.shadow_count, a.shadow_direction[0], a.shadow_direction[1], a.shadow_direction[2]);
		shadow.max_distance = probe.array<float>(a.shadow_count, a.max_distance);
		shadow.illumination_and_pixel_index = probe.array<float4>(a.shadow_count, a.light);
		for (int k = 0; k < 3; k++) if (a.frames[k]) frames[k] = probe.array<float4>(a.frame_pixels, a.frames[k]);
		const unsigned long long zeros[10] = { };
		if (a.stats10) stats = probe.array<unsigned long long>(10, zeros);
	}
	// the launch's frames: these three where given, no other AOV
	void patch_frames(RtParams & p) const {
		for (int i = 0; i < RT_AOV_COUNT; i++) p.aovs[i].framebuffer = nullptr;
		for (int k = 0; k < 3; k++) p.aovs[trace_queue_frame_aov[k]].framebuffer = frames[k];
	}
	int read(Probe & probe, const TraceQueueArgs & a) const {
		int s = RT_OK;
		if (a.closest_count && (s = probe.read(a.hits, trace.hits, a.closest_count * 16))) return s;
		for (int k = 0; k < 3; k++) if (frames[k] && a.frame_pixels && (s = probe.read(a.frames[k], frames[k], a.frame_pixels * 16))) return s;
		return stats ? probe.read(a.stats10, stats, 10 * sizeof(unsigned long long)) : RT_OK;
	}
};
} // namespace

// The merged wavefront's traversal launch (rt_launch_trace_stream, as stream_enqueue_iteration calls it) on the queues of `a`, for both probes. The
// parameter block is stream_params(ctx, iteration) with the closest-hit queue of parity iteration & 1, the shadow queue, the control block and the
// three radiance frames replaced by buffers of this call. Runs on the wavefront's own stream with its own spill area, after quiesce(); nothing of the
// context changes but what the scheduler would set up itself (stream_create, stream_sync_tlas). info4: rt_trace_stream_launch_info's.
static int trace_stream_probe(rt_context * ctx, const char * name, int iteration, const TraceQueueArgs & a, int32_t * info4) {
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx)); // the wavefront's stream and spill area are borrowed
	int s = check_ready(ctx, name, NEED_SCENE_JOINT); if (s) return s;
	if (ctx->params.bvh_width != 8) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: the merged wavefront's launch walks the CWBVH (bvh_width %d)", name, ctx->params.bvh_width);
	s = stream_create(ctx); if (s) return s;
	s = stream_sync_tlas(ctx); if (s) return s;
	PathStream & ps = ctx->path_stream;
	const int q = iteration & 1;

	Probe probe(ctx, name);
	TraceQueueBuffers b; b.upload(probe, a);
	std::unique_ptr<RtStreamControl> control_host(new RtStreamControl());   // (value-initialised: zero cursors and region words)
	control_host->trace_count[q] = int(a.closest_count);
	control_host->shadow_count[q ^ 1] = int(a.shadow_count);
	RtStreamControl * control = probe.array<RtStreamControl>(1, control_host.get());
	if ((s = probe.allocated())) return s;

	RtParams p = stream_params(ctx, iteration);
	p.trace[q] = b.trace;
	p.shadow = b.shadow;
	p.stream = control;
	b.patch_frames(p);
	rt_trace_stream_launch_info(p, b.stats != nullptr, info4);
	rt_launch_trace_stream(p, b.stats, ps.stream);
	if ((s = probe.finish(ps.stream))) return s;
	return b.read(probe, a);
}

// One bounce of the slots scheduler's traversal (rt_render_samples: rt_launch_trace, then rt_launch_trace_shadow with the slot's second spill area;
// their _counting forms; or rt_launch_trace_shadow_ao alone, as rt_render_ao_sample launches it) on the queues of `a`. The parameter block is slot 0's
// with the closest-hit queue of parity bounce & 1, the shadow queue, the counters, the cursors and the three radiance frames replaced by buffers of
// this call. Runs on the main stream after quiesce(). info5: rt_trace_queue_launch_info's.
static int trace_bounce_probe(rt_context * ctx, const char * name, int bounce, int form, const TraceQueueArgs & a, int32_t * info5) {
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx)); // slot 0's spill areas are borrowed
	int s = check_ready(ctx, name, NEED_SCENE_JOINT); if (s) return s;
	const bool counting = form == RT_TRACE_QUEUE_COUNTING, ao = form == RT_TRACE_QUEUE_AO;
	if (counting && ctx->params.bvh_width != 8) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: the counting kernels walk the CWBVH (bvh_width %d)", name, ctx->params.bvh_width);

	Probe probe(ctx, name);
	TraceQueueBuffers b; b.upload(probe, a);
	RtBufferSizes sizes_host = { };
	sizes_host.trace[bounce] = int(a.closest_count); sizes_host.shadow[bounce] = int(a.shadow_count);
	RtBufferSizes * sizes = probe.array<RtBufferSizes>(1, &sizes_host);
	const std::vector<int> zero_cursors(RT_MAX_BOUNCES * 2, 0);
	int * cursors = probe.array<int>(zero_cursors.size(), zero_cursors.data());
	if ((s = probe.allocated())) return s;

	RtParams p = ctx->params;
	p.trace[bounce & 1] = b.trace;
	p.shadow = b.shadow;
	p.sizes = sizes; p.ray_cursors = cursors;
	b.patch_frames(p);
	RtParams p_shadow = p; p_shadow.stack_spill = (uint2 *)ctx->slots[0].spill[1];   // (as the render loop: the shadow launch may be resident with the next closest-hit launch)
	rt_trace_queue_launch_info(p, counting, ao, info5);
	if (ao) rt_launch_trace_shadow_ao(p, ctx->stream);
	else if (counting) { rt_launch_trace_counting(p, bounce, b.stats, ctx->stream); rt_launch_trace_shadow_counting(p, bounce, b.stats, ctx->stream); }
	else { rt_launch_trace(p, bounce, ctx->stream); rt_launch_trace_shadow(p_shadow, bounce, ctx->stream); }
	if ((s = probe.finish())) return s;
	return b.read(probe, a);
}

extern "C" {

int rt_trace_rays(rt_context * ctx, const float * ox, const float * oy, const float * oz,
                  const float * dx, const float * dy, const float * dz, size_t ray_count,
                  uint32_t * hits, int repeat, float * out_ms) {
	RT_REQUIRE(ctx, ctx && ox && oy && oz && dx && dy && dz && hits, "rt_trace_rays: NULL argument");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx)); // slot 0's spill area and cursors are borrowed
	int s = check_ready(ctx, "rt_trace_rays", NEED_SCENE_JOINT); if (s) return s;
	Probe probe(ctx, "rt_trace_rays");
	RtVec3SoA o = probe.vec3(ray_count, ox, oy, oz), d = probe.vec3(ray_count, dx, dy, dz);
	uint4 * dev_hits = probe.array<uint4>(ray_count);
	if ((s = probe.allocated())) return s;
	s = time_explicit_launches(probe, repeat, out_ms, [&] { rt_launch_trace_explicit(ctx->params, o, d, dev_hits, int(ray_count), ctx->explicit_retired, ctx->stream); }); if (s) return s;
	return probe.read(hits, dev_hits, ray_count * 16);
}

int rt_trace_shadow_rays(rt_context * ctx, const float * ox, const float * oy, const float * oz,
                         const float * dx, const float * dy, const float * dz, const float * max_distance,
                         size_t ray_count, uint8_t * occluded, int repeat, float * out_ms) {
	RT_REQUIRE(ctx, ctx && ox && oy && oz && dx && dy && dz && max_distance && occluded, "rt_trace_shadow_rays: NULL argument");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx)); // slot 0's spill area and cursors are borrowed
	int s = check_ready(ctx, "rt_trace_shadow_rays", NEED_SCENE_JOINT); if (s) return s;
	Probe probe(ctx, "rt_trace_shadow_rays");
	RtVec3SoA o = probe.vec3(ray_count, ox, oy, oz), d = probe.vec3(ray_count, dx, dy, dz);
	float * dev_max = probe.array<float>(ray_count, max_distance);
	uint8_t * dev_occ = probe.array<uint8_t>(ray_count);
	if ((s = probe.allocated())) return s;
	s = time_explicit_launches(probe, repeat, out_ms, [&] { rt_launch_trace_shadow_explicit(ctx->params, o, d, dev_max, dev_occ, int(ray_count), ctx->explicit_retired, ctx->stream); }); if (s) return s;
	return probe.read(occluded, dev_occ, ray_count);
}

// rt_trace_stream_rays: trace_stream_probe on explicit rays, with a radiance frame of one pixel per shadow ray and no other: every shadow ray i
// carries illumination (1, 0, 0) for pixel i, so what the launch adds to pixel i tells how often ray i reached its light unoccluded.
int rt_trace_stream_rays(rt_context * ctx, int iteration,
                         const float * ox, const float * oy, const float * oz, const float * dx, const float * dy, const float * dz,
                         size_t closest_count, uint32_t * hits,
                         const float * sox, const float * soy, const float * soz, const float * sdx, const float * sdy, const float * sdz,
                         const float * max_distance, size_t shadow_count, float * shadow_light,
                         uint64_t * stats10, int32_t * info) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_trace_stream_rays: NULL context");
	RT_REQUIRE(ctx, info != nullptr, "rt_trace_stream_rays: NULL info");
	RT_REQUIRE(ctx, iteration >= 0, "rt_trace_stream_rays: negative iteration");
	RT_REQUIRE(ctx, closest_count == 0 || (ox && oy && oz && dx && dy && dz && hits), "rt_trace_stream_rays: NULL closest-hit ray or hit array");
	RT_REQUIRE(ctx, shadow_count == 0 || (sox && soy && soz && sdx && sdy && sdz && max_distance && shadow_light), "rt_trace_stream_rays: NULL shadow ray, max_distance or shadow_light array");
	RT_REQUIRE(ctx, closest_count + shadow_count <= size_t(1) << 28, "rt_trace_stream_rays: more than 2^28 rays in one launch");
	std::vector<float4> light(shadow_count), radiance(shadow_count, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
	for (size_t i = 0; i < shadow_count; i++) {   // (i < 2^28: RT_SHADOW_FLAG_BOUNCE_0 clear)
		uint32_t pixel_word = uint32_t(i); float w; memcpy(&w, &pixel_word, 4);
		light[i] = make_float4(1.0f, 0.0f, 0.0f, w);
	}
	const TraceQueueArgs a = { { ox, oy, oz }, { dx, dy, dz }, closest_count, hits, { sox, soy, soz }, { sdx, sdy, sdz }, max_distance, shadow_count, light.data(),
	                           { shadow_count ? &radiance[0].x : nullptr, nullptr, nullptr }, shadow_count, stats10 };
	int s = trace_stream_probe(ctx, "rt_trace_stream_rays", iteration, a, info); if (s) return s;
	for (size_t i = 0; i < shadow_count; i++) shadow_light[i] = radiance[i].x;
	return RT_OK;
}

// rt_trace_queue_rays: one bounce's traversal launches of the slots scheduler (trace_bounce_probe), or the merged wavefront's launch
// (trace_stream_probe), on explicit queues whose shadow rays carry the caller's illumination and pixel words into the caller's three frames.
int rt_trace_queue_rays(rt_context * ctx, int merged, int step, int form,
                        const float * ox, const float * oy, const float * oz, const float * dx, const float * dy, const float * dz,
                        size_t closest_count, uint32_t * hits,
                        const float * sox, const float * soy, const float * soz, const float * sdx, const float * sdy, const float * sdz,
                        const float * max_distance, const float * illumination, const uint32_t * pixel_words, size_t shadow_count,
                        float * radiance, float * radiance_direct, float * radiance_indirect, size_t frame_pixels,
                        uint64_t * stats10, int32_t * info) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_trace_queue_rays: NULL context");
	RT_REQUIRE(ctx, info != nullptr, "rt_trace_queue_rays: NULL info");
	RT_REQUIRE(ctx, merged == 0 || merged == 1, "rt_trace_queue_rays: merged must be 0 (per-bounce launches) or 1 (merged wavefront)");
	RT_REQUIRE(ctx, form == RT_TRACE_QUEUE_PLAIN || form == RT_TRACE_QUEUE_COUNTING || (form == RT_TRACE_QUEUE_AO && !merged),
	           "rt_trace_queue_rays: form must be 0 (the frame's kernels), 1 (the counting kernels) or, per-bounce only, 2 (the AO integrator's shadow launch)");
	RT_REQUIRE(ctx, step >= 0 && (merged || step < RT_MAX_BOUNCES), merged ? "rt_trace_queue_rays: negative iteration" : "rt_trace_queue_rays: bounce outside [0, RT_MAX_BOUNCES)");
	RT_REQUIRE(ctx, form != RT_TRACE_QUEUE_AO || (step == 0 && closest_count == 0), "rt_trace_queue_rays: the AO form launches the shadow queue of bounce 0 alone (step and closest_count must be 0)");
	RT_REQUIRE(ctx, (form == RT_TRACE_QUEUE_COUNTING) == (stats10 != nullptr), "rt_trace_queue_rays: stats10 must be given for the counting kernels and NULL otherwise");
	RT_REQUIRE(ctx, closest_count == 0 || (ox && oy && oz && dx && dy && dz && hits), "rt_trace_queue_rays: NULL closest-hit ray or hit array");
	RT_REQUIRE(ctx, shadow_count == 0 || (sox && soy && soz && sdx && sdy && sdz && max_distance && illumination && pixel_words),
	           "rt_trace_queue_rays: NULL shadow ray, max_distance, illumination or pixel word array");
	RT_REQUIRE(ctx, closest_count <= size_t(1) << 28 && shadow_count <= size_t(1) << 28 && closest_count + shadow_count <= size_t(1) << 28, "rt_trace_queue_rays: more than 2^28 rays in one launch");
	RT_REQUIRE(ctx, frame_pixels <= size_t(1) << 28, "rt_trace_queue_rays: more than 2^28 pixels in a frame");
	std::vector<float4> light(shadow_count);
	{	// every pixel a shadow ray names lies inside the frames, and no two rays name the same one: the contribution is a plain read-modify-write,
		// and a frame never queues two shadow rays per pixel and bounce
		PixelsOnce once(frame_pixels);
		for (size_t i = 0; i < shadow_count; i++) {
			const uint32_t word = pixel_words[i];
			if (!merged && (word & RT_SHADOW_FLAG_BOUNCE_0)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_trace_queue_rays: shadow ray %zu: the bounce-0 flag is set in the pixel word of a per-bounce launch", i);
			const uint32_t pixel = word & ~RT_SHADOW_FLAG_BOUNCE_0;
			const PixelsOnce::Named named = once.name(pixel);
			if (named == PixelsOnce::BEYOND) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_trace_queue_rays: shadow ray %zu: pixel %u beyond the %zu pixels of the frames", i, pixel, frame_pixels);
			if (named == PixelsOnce::TWICE) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_trace_queue_rays: shadow ray %zu: pixel %u appears twice", i, pixel);
			float w; memcpy(&w, &word, 4);
			light[i] = make_float4(illumination[3 * i], illumination[3 * i + 1], illumination[3 * i + 2], w);
		}
	}
	const TraceQueueArgs a = { { ox, oy, oz }, { dx, dy, dz }, closest_count, hits, { sox, soy, soz }, { sdx, sdy, sdz }, max_distance, shadow_count, light.data(),
	                           { radiance, radiance_direct, radiance_indirect }, frame_pixels, stats10 };
	for (int i = 0; i < RT_TRACE_QUEUE_INFO; i++) info[i] = -1;
	if (!merged) return trace_bounce_probe(ctx, "rt_trace_queue_rays", step, form, a, info);
	int32_t stream_info[4];
	int s = trace_stream_probe(ctx, "rt_trace_queue_rays", step, a, stream_info); if (s) return s;
	info[0] = 8; info[1] = info[2] = stream_info[1]; info[3] = stream_info[2]; info[5] = stream_info[0];   // (one launch: one grid; no ray_block of this kind)
	return RT_OK;
}


int rt_generate_rays(rt_context * ctx, int sample_index, int pixel_offset, int pixel_count,
                     float * ox, float * oy, float * oz, float * dx, float * dy, float * dz, uint32_t * pixel_index_and_flags) {
	RT_REQUIRE(ctx, ctx && ox && oy && oz && dx && dy && dz && pixel_index_and_flags, "rt_generate_rays: NULL argument");
	RT_REQUIRE(ctx, pixel_count >= 0, "rt_generate_rays: negative pixel_count");
	(void)hipSetDevice(ctx->device);
	if (!ctx->params.pmj_samples || ctx->frame_pixels == 0) return fail(ctx, RT_ERROR_NOT_READY, "rt_generate_rays: RNG tables not uploaded or rt_resize not called");
	RT_HIP(ctx, quiesce(ctx)); // slot 0's queues are borrowed
	int s = ensure_queues(ctx); if (s) return s;
	if (size_t(pixel_count) > ctx->slots[0].queues.capacity) return fail(ctx, RT_ERROR_OUT_OF_RANGE, "rt_generate_rays: pixel_count %d exceeds the queue capacity %zu", pixel_count, ctx->slots[0].queues.capacity);
	Probe probe(ctx, "rt_generate_rays");   // (no array of its own: the rays are read from slot 0's queue)
	rt_launch_generate(ctx->params, sample_index, pixel_offset, pixel_count, ctx->stream);
	if ((s = probe.finish())) return s;
	const RtTraceBuffer & t = ctx->params.trace[0];
	void * const dst[7] = { ox, oy, oz, dx, dy, dz, pixel_index_and_flags };
	const void * const src[7] = { t.origin.x, t.origin.y, t.origin.z, t.direction.x, t.direction.y, t.direction.z, t.pixel_index_and_flags };
	for (int i = 0; i < 7 && s == RT_OK; i++) s = probe.read(dst[i], src[i], size_t(pixel_count) * 4);
	return s;
}

// rt_generate_primary_rays: one of the three generate launches (rt_launch_generate, rt_launch_generate_stream, rt_launch_generate_stream_list, as the
// per-bounce loop and stream_generate call them) on a caller-given submission. The parameter block is the context's (ctx->params, or
// stream_params(ctx, iteration)) with the submission's batch_samples and tiles, and with the trace queue (of parity iteration & 1 for the stream
// kernels) and the counters (RtBufferSizes) or the control block replaced by buffers of this call. Camera, filter, SVGF flag and RNG tables are
// the context's. Runs on the main stream after quiesce(); nothing of the context changes but what the scheduler would set up itself (stream_create).
int rt_generate_primary_rays(rt_context * ctx, int kernel, int iteration, int first_sample, int sample_count, int pixel_offset, int pixel_count,
                             int tile_pixels, int tile_first, int tile_stride, int slot_base, int queue_before, int queue_offset,
                             int block_width, int band_rows, const uint32_t * pixel_list, size_t capacity,
                             float * ox, float * oy, float * oz, float * dx, float * dy, float * dz, uint32_t * pixel_index_and_flags, int32_t * info) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_generate_primary_rays: NULL context");
	RT_REQUIRE(ctx, ox && oy && oz && dx && dy && dz && pixel_index_and_flags && info, "rt_generate_primary_rays: NULL array");
	RT_REQUIRE(ctx, kernel >= 0 && kernel <= 2, "rt_generate_primary_rays: kernel must be 0 (kernel_generate), 1 (kernel_generate_stream) or 2 (kernel_generate_stream_list)");
	RT_REQUIRE(ctx, iteration >= 0 && first_sample >= 0 && pixel_offset >= 0 && pixel_count >= 0 && tile_pixels >= 0 && tile_first >= 0 && tile_stride >= 0 &&
	                slot_base >= 0 && queue_before >= 0 && queue_offset >= 0, "rt_generate_primary_rays: a count below zero");
	RT_REQUIRE(ctx, sample_count >= 1 && sample_count <= RT_MAX_BATCH_SAMPLES, "rt_generate_primary_rays: sample_count must be 1..16");
	RT_REQUIRE(ctx, slot_base + sample_count <= RT_STREAM_SAMPLE_SLOTS, "rt_generate_primary_rays: slot_base + sample_count beyond the 512 sample slots");
	RT_REQUIRE(ctx, kernel != 0 || (slot_base == 0 && queue_before == 0 && queue_offset == 0), "rt_generate_primary_rays: kernel_generate has no slot_base, queue count or queue_offset");
	RT_REQUIRE(ctx, kernel != 2 || (pixel_offset == 0 && tile_pixels == 0), "rt_generate_primary_rays: kernel_generate_stream_list has no pixel_offset and no tiles");
	RT_REQUIRE(ctx, kernel != 2 || pixel_list || pixel_count == 0, "rt_generate_primary_rays: NULL pixel list");
	RT_REQUIRE(ctx, tile_pixels == 0 || tile_stride >= 1, "rt_generate_primary_rays: tile_stride must be at least 1 with tiles");
	RT_REQUIRE(ctx, (block_width == -1 && band_rows == -1) || (block_width == 0 && band_rows == 0) || (kernel == 1 && block_width > 0 && band_rows > 0),
	           "rt_generate_primary_rays: block_width and band_rows must both be -1 (the scheduler's choice), both 0 (scan lines) or, for kernel_generate_stream, both positive");
	RT_REQUIRE(ctx, capacity >= 1 && capacity <= size_t(1) << 28, "rt_generate_primary_rays: capacity must be in [1, 2^28]");
	(void)hipSetDevice(ctx->device);
	if (!ctx->params.pmj_samples || !ctx->params.blue_noise || ctx->frame_pixels == 0) return fail(ctx, RT_ERROR_NOT_READY, "rt_generate_primary_rays: RNG tables not uploaded or rt_resize not called");
	const size_t frame_pixels = ctx->frame_pixels;
	const size_t frame = size_t(ctx->params.screen_width) * size_t(ctx->params.screen_height);
	RT_REQUIRE(ctx, size_t(slot_base + sample_count) * frame_pixels < size_t(1) << 30, "rt_generate_primary_rays: (slot_base + sample_count) * frame_pixels must be below 2^30");
	const size_t rays = size_t(pixel_count) * size_t(sample_count);
	RT_REQUIRE(ctx, size_t(queue_before) + size_t(queue_offset) + rays <= capacity, "rt_generate_primary_rays: capacity below queue count + queue_offset + rays");
	if (kernel == 2) {
		for (int i = 0; i < pixel_count; i++)
			if (pixel_list[i] >= frame) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_generate_primary_rays: list entry %d: pixel %u beyond the %zu pixels of the frame", i, pixel_list[i], frame);
	} else if (pixel_count > 0) {   // rt_map_pixel grows with the local index: the last pixel decides
		const size_t i = size_t(pixel_offset) + size_t(pixel_count) - 1;
		const size_t last = tile_pixels == 0 ? i : ((i / size_t(tile_pixels)) * size_t(tile_stride) + size_t(tile_first)) * size_t(tile_pixels) + i % size_t(tile_pixels);
		if (last >= frame) return fail(ctx, RT_ERROR_OUT_OF_RANGE, "rt_generate_primary_rays: the last pixel of the range, %zu, lies beyond the %zu pixel frame", last, frame);
	}
	RT_HIP(ctx, quiesce(ctx));
	int s = stream_create(ctx); if (s) return s;
	const int q = kernel == 0 ? 0 : iteration & 1;

	Probe probe(ctx, "rt_generate_primary_rays");
	RtTraceBuffer trace = { };
	trace.origin = probe.vec3(capacity, ox, oy, oz); trace.direction = probe.vec3(capacity, dx, dy, dz);   // the caller's values: a sentinel shows an entry the launch never wrote
	trace.pixel_index_and_flags = probe.array<unsigned>(capacity, pixel_index_and_flags);
	const unsigned * list = kernel == 2 ? probe.array<unsigned>(size_t(pixel_count), pixel_list) : nullptr;
	RtBufferSizes * sizes = nullptr; RtStreamControl * control = nullptr;
	if (kernel == 0) {
		RtBufferSizes sizes_host = { };
		sizes = probe.array<RtBufferSizes>(1, &sizes_host);
	} else {
		std::unique_ptr<RtStreamControl> control_host(new RtStreamControl());   // (value-initialised: zero cursors and region words)
		control_host->trace_count[q] = queue_before;
		control = probe.array<RtStreamControl>(1, control_host.get());
	}
	if ((s = probe.allocated())) return s;

	RtParams p = kernel == 0 ? ctx->params : stream_params(ctx, iteration);
	p.batch_samples = sample_count;
	p.tile_pixels = tile_pixels; p.tile_first = tile_first; p.tile_stride = tile_stride;
	p.trace[q] = trace;
	p.sizes = sizes; p.stream = control;
	int order[2] = { block_width, band_rows };
	if (kernel == 0) { order[0] = order[1] = 0; rt_launch_generate(p, first_sample, pixel_offset, pixel_count, ctx->stream); }
	else if (kernel == 2 || block_width < 0) stream_launch_generate(p, first_sample, list, pixel_offset, pixel_count, slot_base, queue_offset, ctx->stream, order);   // (a list has one order)
	else rt_launch_generate_stream(p, first_sample, pixel_offset, pixel_count, slot_base, queue_offset, block_width, band_rows, ctx->stream);
	if ((s = probe.finish())) return s;

	void * const dst[7] = { ox, oy, oz, dx, dy, dz, pixel_index_and_flags };
	const void * const src[7] = { trace.origin.x, trace.origin.y, trace.origin.z, trace.direction.x, trace.direction.y, trace.direction.z, trace.pixel_index_and_flags };
	for (int i = 0; i < 7; i++) if ((s = probe.read(dst[i], src[i], capacity * 4))) return s;
	// the grid of the three launchers: one thread per pixel (kernel_generate) or per ray, at most 2 048 workgroups of 256, the rest grid-strided
	const size_t blocks = ((kernel == 0 ? size_t(pixel_count) : rays) + 255) / 256;
	info[0] = order[0]; info[1] = order[1]; info[2] = int(std::min(std::max(blocks, size_t(1)), size_t(2048)));
	if (kernel == 0) {
		RtBufferSizes sizes_host;
		if ((s = probe.read(&sizes_host, sizes, sizeof(RtBufferSizes)))) return s;
		info[3] = sizes_host.trace[0];
	} else {
		if ((s = probe.read(&info[3], &control->trace_count[q], sizeof(int)))) return s;
	}
	return RT_OK;
}

int rt_random_samples(rt_context * ctx, int dimension, const uint32_t * pixel_indices, size_t count, uint32_t bounce, uint32_t sample_index, float * out_xy) {
	RT_REQUIRE(ctx, ctx && pixel_indices && out_xy && dimension >= 0 && dimension < 7, "rt_random_samples: invalid argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->params.pmj_samples || ctx->params.screen_pitch == 0) return fail(ctx, RT_ERROR_NOT_READY, "rt_random_samples: RNG tables not uploaded or rt_resize not called");
	Probe probe(ctx, "rt_random_samples");
	unsigned * dev_px = probe.array<unsigned>(count, pixel_indices);
	float2 * dev_out = probe.array<float2>(count);
	int s = probe.allocated(); if (s) return s;
	rt_launch_random(ctx->params, dimension, dev_px, int(count), bounce, sample_index, dev_out, ctx->stream);
	return probe.finish_and_read(out_xy, dev_out, count * 8);
}

int rt_sample_texture(rt_context * ctx, int texture_index, int filter, const float * args, size_t count, float * out_rgba) {
	RT_REQUIRE(ctx, ctx && args && out_rgba, "rt_sample_texture: NULL argument");
	RT_REQUIRE(ctx, texture_index >= 0 && size_t(texture_index) < ctx->texture_data.size(), "rt_sample_texture: texture index out of range");
	RT_REQUIRE(ctx, filter >= 0 && filter <= 2, "rt_sample_texture: filter must be 0 (level 0), 1 (lod) or 2 (gradients)");
	RT_REQUIRE(ctx, count <= size_t(1) << 28, "rt_sample_texture: more than 2^28 probes");
	(void)hipSetDevice(ctx->device);
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_sample_texture");
	float * dev_args = probe.array<float>(count * 8, args);
	float4 * dev_out = probe.array<float4>(count);
	int s = probe.allocated(); if (s) return s;
	rt_launch_sample_texture(ctx->params, texture_index, filter, dev_args, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out_rgba, dev_out, count * 16);
}

int rt_sample_table(rt_context * ctx, const float * table, int nx, int ny, int nz, int dims, const float * coords, size_t count, float * out) {
	RT_REQUIRE(ctx, ctx && table && coords && out, "rt_sample_table: NULL argument");
	RT_REQUIRE(ctx, dims >= 1 && dims <= 3, "rt_sample_table: dims must be 1, 2 or 3");
	RT_REQUIRE(ctx, nx >= 1 && nx <= 65536 && (dims < 2 || (ny >= 1 && ny <= 65536)) && (dims < 3 || (nz >= 1 && nz <= 65536)), "rt_sample_table: a table side is outside [1, 65536]");
	RT_REQUIRE(ctx, count <= size_t(1) << 28, "rt_sample_table: more than 2^28 probes");
	size_t entries = size_t(nx) * (dims >= 2 ? size_t(ny) : 1) * (dims >= 3 ? size_t(nz) : 1);
	RT_REQUIRE(ctx, entries <= size_t(1) << 28, "rt_sample_table: more than 2^28 table entries");
	(void)hipSetDevice(ctx->device);
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_sample_table");
	float * dev_table = probe.array<float>(entries, table);
	float * dev_coords = probe.array<float>(count * 3, coords);
	float * dev_out = probe.array<float>(count);
	int s = probe.allocated(); if (s) return s;
	rt_launch_sample_table(dev_table, nx, dims >= 2 ? ny : 1, dims >= 3 ? nz : 1, dims, dev_coords, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out, dev_out, count * 4);
}

int rt_sample_sky(rt_context * ctx, const float * directions, size_t count, float * out_rgb) {
	RT_REQUIRE(ctx, ctx && directions && out_rgb, "rt_sample_sky: NULL argument");
	RT_REQUIRE(ctx, ctx->params.sky, "rt_sample_sky: no sky uploaded (rt_set_sky)");
	RT_REQUIRE(ctx, count <= size_t(1) << 28, "rt_sample_sky: more than 2^28 probes");
	(void)hipSetDevice(ctx->device);
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_sample_sky");
	float * dev_dirs = probe.array<float>(count * 3, directions);
	float * dev_out = probe.array<float>(count * 3);
	int s = probe.allocated(); if (s) return s;
	rt_launch_sample_sky(ctx->params, dev_dirs, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out_rgb, dev_out, count * 12);
}

int rt_sample_sky_distribution(rt_context * ctx, const float * uv, size_t count, float * out_xyz_pdf) {
	RT_REQUIRE(ctx, ctx && uv && out_xyz_pdf, "rt_sample_sky_distribution: NULL argument");
	RT_REQUIRE(ctx, ctx->params.sky, "rt_sample_sky_distribution: no sky uploaded (rt_set_sky)");
	RT_REQUIRE(ctx, count <= size_t(1) << 28, "rt_sample_sky_distribution: more than 2^28 probes");
	(void)hipSetDevice(ctx->device);
	int s = sky_tables_build(ctx, "rt_sample_sky_distribution"); if (s) return s;
	RT_REQUIRE(ctx, ctx->sky_total > 0.0, "rt_sample_sky_distribution: the sky has no weight to sample");
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_sample_sky_distribution");
	float * dev_uv = probe.array<float>(count * 2, uv);
	float * dev_out = probe.array<float>(count * 4);
	if ((s = probe.allocated())) return s;
	rt_launch_sample_sky_distribution(ctx->params, dev_uv, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out_xyz_pdf, dev_out, count * 16);
}

int rt_sky_pdf(rt_context * ctx, const float * directions, size_t count, float * out_pdf) {
	RT_REQUIRE(ctx, ctx && directions && out_pdf, "rt_sky_pdf: NULL argument");
	RT_REQUIRE(ctx, ctx->params.sky, "rt_sky_pdf: no sky uploaded (rt_set_sky)");
	RT_REQUIRE(ctx, count <= size_t(1) << 28, "rt_sky_pdf: more than 2^28 probes");
	(void)hipSetDevice(ctx->device);
	int s = sky_tables_build(ctx, "rt_sky_pdf"); if (s) return s;
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_sky_pdf");
	float * dev_dirs = probe.array<float>(count * 3, directions);
	float * dev_out = probe.array<float>(count);
	if ((s = probe.allocated())) return s;
	rt_launch_sky_pdf(ctx->params, dev_dirs, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out_pdf, dev_out, count * 4);
}

// rt_bsdf_eval / rt_bsdf_sample: a copy of the parameters whose material table is the probes' own materials (probe i: material i),
// with the Kulla-Conty tables of the context, no AOV and SVGF off, so that nothing of a frame is read or written.
static int bsdf_probe(rt_context * ctx, const char * name, bool eval, int material_type, const float * probes, size_t count, float * out) {
	if (!ctx || !probes || !out) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: NULL argument", name);
	if (material_type < RT_MATERIAL_DIFFUSE || material_type > RT_MATERIAL_CONDUCTOR)
		return fail(ctx, RT_ERROR_INVALID_ARG, "%s: material_type must be diffuse (1), plastic (2), dielectric (3) or conductor (4)", name);
	if (count > size_t(1) << 24) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: more than 2^24 probes", name);
	if (material_type == RT_MATERIAL_DIFFUSE || material_type == RT_MATERIAL_PLASTIC) {
		for (size_t i = 0; i < count; i++) {
			int32_t texture_id; memcpy(&texture_id, probes + i * RT_BSDF_PROBE_IN + 3, 4);
			if (texture_id != RT_INVALID) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: probe %zu names texture %d (only RT_INVALID is probed)", name, i, texture_id);
		}
	}
	(void)hipSetDevice(ctx->device);
	if (!ctx->params.pmj_samples || ctx->params.screen_pitch == 0) return fail(ctx, RT_ERROR_NOT_READY, "%s: RNG tables not uploaded or rt_resize not called", name);
	int s = ensure_luts(ctx); if (s) return s;
	if (count == 0) return RT_OK;
	std::vector<float> materials(count * 8);
	for (size_t i = 0; i < count; i++) memcpy(&materials[i * 8], probes + i * RT_BSDF_PROBE_IN, 32);
	Probe probe(ctx, name);
	float * dev_materials = probe.array<float>(count * 8, materials.data());
	float * dev_probes = probe.array<float>(count * RT_BSDF_PROBE_IN, probes);
	float * dev_out = probe.array<float>(count * RT_BSDF_PROBE_OUT);
	if ((s = probe.allocated())) return s;
	RtParams p = ctx->params;
	p.materials = (const float4 *)dev_materials;
	p.textures = nullptr;
	for (int a = 0; a < RT_AOV_COUNT; a++) p.aovs[a].framebuffer = p.aovs[a].accumulator = nullptr;
	p.config.enable_svgf = 0;
	rt_launch_bsdf_probe(p, material_type, eval, dev_probes, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out, dev_out, count * RT_BSDF_PROBE_OUT * 4);
}

int rt_bsdf_eval(rt_context * ctx, int material_type, const float * probes, size_t count, float * out) {
	return bsdf_probe(ctx, "rt_bsdf_eval", true, material_type, probes, count, out);
}
int rt_bsdf_sample(rt_context * ctx, int material_type, const float * probes, size_t count, float * out) {
	return bsdf_probe(ctx, "rt_bsdf_sample", false, material_type, probes, count, out);
}

int rt_sample_lights(rt_context * ctx, const float * probes, size_t count, int use_lds, float * out) {
	RT_REQUIRE(ctx, ctx && probes && out, "rt_sample_lights: NULL argument");
	RT_REQUIRE(ctx, count <= size_t(1) << 24, "rt_sample_lights: more than 2^24 probes");
	RT_REQUIRE(ctx, use_lds == 0 || use_lds == 1, "rt_sample_lights: use_lds must be 0 (global memory) or 1 (as the shade kernels choose)");
	const RtParams & p = ctx->params;
	if (p.light_mesh_count <= 0 || p.light_triangle_count <= 0 || !(p.lights_total_weight > 0.0f))
		return fail(ctx, RT_ERROR_NOT_READY, "rt_sample_lights: no lights uploaded (rt_upload_lights with at least one light mesh entry)");
	if (!p.triangles || !p.mesh_transforms || !p.mesh_material_ids || !p.materials)
		return fail(ctx, RT_ERROR_NOT_READY, "rt_sample_lights: geometry, instance tables or materials not uploaded");
	for (size_t i = 0; i < count * 4; i++)   // (the searches end only for numbers up to the tables' last entry, 1)
		if (!(probes[i] >= 0.0f && probes[i] < 1.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_sample_lights: probe %zu: random number %zu is %.9g, outside [0, 1)", i / 4, i % 4, double(probes[i]));
	(void)hipSetDevice(ctx->device);
	int s = sky_sampling_prepare(ctx, "rt_sample_lights"); if (s) return s;   // (as a render settles it; the selection does not read it)
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_sample_lights");
	float * dev_probes = probe.array<float>(count * 4, probes);
	float * dev_out = probe.array<float>(count * RT_LIGHT_SAMPLE_OUT);
	if ((s = probe.allocated())) return s;
	rt_launch_sample_lights(p, dev_probes, int(count), use_lds != 0, dev_out, ctx->stream);
	return probe.finish_and_read(out, dev_out, count * RT_LIGHT_SAMPLE_OUT * 4);
}

int rt_sample_delta_lights(rt_context * ctx, const float * probes, size_t count, float * out) {
	RT_REQUIRE(ctx, ctx && probes && out, "rt_sample_delta_lights: NULL argument");
	RT_REQUIRE(ctx, count <= size_t(1) << 24, "rt_sample_delta_lights: more than 2^24 probes");
	const RtParams & p = ctx->params;
	if (p.delta_light_count <= 0 || !p.delta_lights || !p.delta_light_cdf)
		return fail(ctx, RT_ERROR_NOT_READY, "rt_sample_delta_lights: no delta lights uploaded (rt_upload_delta_lights)");
	for (size_t i = 0; i < count; i++) {   // (the search ends only for numbers up to the table's last entry, 1)
		const float * a = probes + i * 4;
		if (!(a[0] >= 0.0f && a[0] < 1.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_sample_delta_lights: probe %zu: random number is %.9g, outside [0, 1)", i, double(a[0]));
		if (!(std::isfinite(a[1]) && std::isfinite(a[2]) && std::isfinite(a[3]))) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_sample_delta_lights: probe %zu: origin is not finite", i);
	}
	(void)hipSetDevice(ctx->device);
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_sample_delta_lights");
	float * dev_probes = probe.array<float>(count * 4, probes);
	float * dev_out = probe.array<float>(count * RT_DELTA_SAMPLE_OUT);
	int s = probe.allocated(); if (s) return s;
	rt_launch_sample_delta_lights(p, dev_probes, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out, dev_out, count * RT_DELTA_SAMPLE_OUT * 4);
}

int rt_perturb_normals(rt_context * ctx, int texture_index, const float * probes, size_t count, float * out) {
	RT_REQUIRE(ctx, ctx && probes && out, "rt_perturb_normals: NULL argument");
	RT_REQUIRE(ctx, texture_index >= 0 && size_t(texture_index) < ctx->texture_formats.size(), "rt_perturb_normals: texture index out of range");
	RT_REQUIRE(ctx, ctx->texture_formats[texture_index] == RT_TEXTURE_RGBA8, "rt_perturb_normals: the map must be an RT_TEXTURE_RGBA8 texture");
	RT_REQUIRE(ctx, count <= size_t(1) << 24, "rt_perturb_normals: more than 2^24 probes");
	for (size_t i = 0; i < count; i++) {
		float filter = probes[i * RT_NORMAL_PROBE_IN + 41];
		RT_REQUIRE(ctx, filter == 0.0f || filter == 1.0f || filter == 2.0f, "rt_perturb_normals: filter must be 0 (level 0), 1 (lod) or 2 (gradients)");
	}
	(void)hipSetDevice(ctx->device);
	if (count == 0) return RT_OK;
	Probe probe(ctx, "rt_perturb_normals");
	float * dev_probes = probe.array<float>(count * RT_NORMAL_PROBE_IN, probes);
	float * dev_out = probe.array<float>(count * 4);
	int s = probe.allocated(); if (s) return s;
	rt_launch_perturb_normals(ctx->params, texture_index, dev_probes, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out, dev_out, count * 16);
}

} // extern "C"

// ---- the sort and material launch probes: what rt_sort_rays (with its fog form) and rt_shade_rays do around their launch, written once ----
namespace {
// The arguments the two share. `name` is the entry point's, for every message.
struct QueueLaunch {
	rt_context * ctx; const char * name;
	int merged, step; size_t count;   // merged: `step` is the iteration, else the bounce; `count` entries in the queue the launch reads
	const int32_t * slot_table; size_t slot_count; const int32_t * submission_birth;   // (merged form)
	size_t capacity, frame_slots;
	size_t pixels() const { return frame_slots * ctx->frame_pixels; }
};

// The argument checks in the order the refusals are decided: `merged`, the entry point's own refusal (`own`: its text, or null), then what the two share, down to the
// slot table. tables_given: slot table, births and statistics (merged form). bounce_limit: RT_MAX_BOUNCES, or one less for a launch that appends to the NEXT
// bounce's trace queue, whose per-bounce counter RtBufferSizes::trace[bounce + 1] would else be the next array's first word.
int queue_launch_arguments(const QueueLaunch & a, const char * own, bool tables_given, int bounce_limit) {
	rt_context * ctx = a.ctx; const char * name = a.name;
	if (a.merged != 0 && a.merged != 1) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: merged must be 0 (per-bounce launch) or 1 (merged wavefront)", name);
	if (own) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: %s", name, own);
	if (a.merged && !tables_given) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: NULL slot table, submission births or statistics (merged form)", name);
	if (a.step < 0 || (!a.merged && a.step >= bounce_limit))
		return fail(ctx, RT_ERROR_INVALID_ARG, a.merged ? "%s: negative iteration" : bounce_limit == RT_MAX_BOUNCES ? "%s: bounce outside [0, RT_MAX_BOUNCES)" : "%s: bounce outside [0, RT_MAX_BOUNCES - 1)", name);
	if (a.capacity < 1 || a.capacity > size_t(1) << 28) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: capacity must be in [1, 2^28]", name);
	if (a.count > a.capacity) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: more entries than the queue capacity", name);
	// a bounce the path length does not reach is refused too: beyond it the per-bounce counter of the next trace queue runs into the next array of RtBufferSizes
	if (!a.merged && a.step >= ctx->params.config.num_bounces) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: bounce outside [0, num_bounces)", name);
	(void)hipSetDevice(ctx->device);
	int s = check_ready(ctx, name, NEED_SCENE_JOINT | NEED_MATERIALS | NEED_RNG | NEED_SKY | NEED_FRAME); if (s) return s;
	if (a.frame_slots < 1 || a.frame_slots > size_t(RT_STREAM_SAMPLE_SLOTS) || a.frame_slots * ctx->frame_pixels >= size_t(1) << 30)
		return fail(ctx, RT_ERROR_INVALID_ARG, "%s: frame_slots must be in [1, 512] and frame_slots * frame_pixels below 2^30", name);
	if (!a.merged) return RT_OK;
	if (a.slot_count < 1 || a.slot_count > size_t(RT_STREAM_SAMPLE_SLOTS)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: slot_count must be in [1, 512]", name);
	for (size_t k = 0; k < a.slot_count; k++) {
		const int32_t * e = a.slot_table + 4 * k;
		if (e[2] < 0 || e[2] >= RT_STREAM_SUBMISSIONS) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: slot %zu: submission %d outside [0, %d)", name, k, e[2], RT_STREAM_SUBMISSIONS);
		if (e[1] != a.submission_birth[e[2]]) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: slot %zu: birth iteration %d is not its submission's (%d)", name, k, e[1], a.submission_birth[e[2]]);
	}
	return RT_OK;
}

// Every index the kernel forms from an entry of the queue it reads (B: RtTraceBuffer or RtMaterialBuffer) stays inside the call's buffers and the context's tables.
// miss_allowed: a triangle id of RT_INVALID names no triangle and no instance. also(i, mesh_id): the entry point's own test of a hit entry, after these.
template<typename B, typename Also> int queue_launch_entries(const QueueLaunch & a, const uint32_t * records, bool miss_allowed, Also && also) {
	constexpr int PIXEL = record_word<B>(offsetof(B, pixel_index_and_flags)), HIT = record_word<B>(offsetof(B, hits)), MEDIUM = record_word<B>(offsetof(B, medium));
	static_assert(PIXEL >= 0 && HIT >= 0 && MEDIUM >= 0, "the record has a pixel word, a hit and a medium");
	rt_context * ctx = a.ctx; const char * name = a.name;
	const size_t pixels = a.pixels(), frame_pixels = ctx->frame_pixels;
	PixelsOnce once(pixels);
	for (size_t i = 0; i < a.count; i++) {
		const uint32_t * r = records + i * RecordLayout<B>::words;
		const uint32_t v = r[PIXEL] & ~RT_FLAGS_ALL;
		const PixelsOnce::Named named = once.name(v);
		if (named == PixelsOnce::BEYOND) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: entry %zu: virtual pixel %u beyond the %zu pixels of the frames", name, i, v, pixels);
		if (named == PixelsOnce::TWICE) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: entry %zu: virtual pixel %u appears twice", name, i, v);
		const int32_t mesh_id = int32_t(r[HIT]), triangle_id = int32_t(r[HIT + 1]);
		if (!miss_allowed || triangle_id != RT_INVALID) {
			if (triangle_id < 0 || size_t(triangle_id) >= ctx->triangle_count) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: entry %zu: triangle id %d beyond the %zu triangles", name, i, triangle_id, ctx->triangle_count);
			if (mesh_id < 0 || size_t(mesh_id) >= ctx->mesh_count) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: entry %zu: mesh id %d beyond the %zu instances", name, i, mesh_id, ctx->mesh_count);
			if (int s = also(i, mesh_id)) return s;
		}
		if (r[PIXEL] & RT_FLAG_INSIDE_MEDIUM) {
			const int32_t medium = int32_t(r[MEDIUM]);
			if (medium < 0 || size_t(medium) >= ctx->medium_count) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: entry %zu: medium id %d beyond the %zu media", name, i, medium, ctx->medium_count);
		}
		if (a.merged) {
			const size_t slot = v / frame_pixels;
			if (slot >= a.slot_count) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: entry %zu: slot %zu beyond the %zu slots of the table", name, i, slot, a.slot_count);
			const int bounce = a.step - a.slot_table[4 * slot + 1];
			if (bounce < 0 || bounce >= RT_MAX_BOUNCES || bounce >= ctx->params.config.num_bounces)
				return fail(ctx, RT_ERROR_INVALID_ARG, "%s: entry %zu: bounce %d outside [0, min(RT_MAX_BOUNCES, num_bounces))", name, i, bounce);
		}
	}
	return RT_OK;
}

// The counters a launch reads and writes, as its scheduler keeps them: the control block (merged; with the slot table where one is given) or RtBufferSizes, all
// zero but for what `set_control` / `set_sizes` write -- the count of the queue the launch reads. After read() the host copies are what the launch left.
struct LaunchCounters {
	RtBufferSizes * sizes = nullptr; RtStreamControl * control = nullptr; RtStreamTable * table = nullptr;
	std::unique_ptr<RtStreamControl> control_host; RtBufferSizes sizes_host = { };
	template<typename SetControl, typename SetSizes>
	void stage(Probe & probe, bool merged, SetControl && set_control, SetSizes && set_sizes, const int32_t * slot_table = nullptr, size_t slot_count = 0, const int32_t * submission_birth = nullptr) {
		if (!merged) { set_sizes(sizes_host); sizes = probe.array<RtBufferSizes>(1, &sizes_host); return; }
		control_host.reset(new RtStreamControl());   // (value-initialised: zero cursors and region words)
		set_control(*control_host);
		control = probe.array<RtStreamControl>(1, control_host.get());
		if (!slot_table) return;
		std::unique_ptr<RtStreamTable> table_host(new RtStreamTable());
		memcpy(table_host->slots, slot_table, slot_count * sizeof(RtStreamSlot));
		memcpy(table_host->submission_birth, submission_birth, sizeof(table_host->submission_birth));
		table = probe.array<RtStreamTable>(1, table_host.get());
	}
	void patch(RtParams & p) const { p.sizes = sizes; p.stream = control; p.stream_table = table; }
	// (stats: the merged form's statistics, the control block's)
	int read(Probe & probe, int32_t * stats) {
		if (!control) return probe.read(&sizes_host, sizes, sizeof(RtBufferSizes));
		int s = probe.read(control_host.get(), control, sizeof(RtStreamControl)); if (s) return s;
		memcpy(stats, control_host->stats, sizeof(control_host->stats));
		return RT_OK;
	}
};
int * material_sizes(RtBufferSizes & z, int material_slot) { return material_slot == 0 ? z.diffuse : material_slot == 1 ? z.plastic : material_slot == 2 ? z.dielectric : z.conductor; }

// The AOV frames of a launch (`count` of them, at most four, of the kinds `aov`; one after the other in the caller's `frames`) and the three g-buffers, `pixels`
// pixels each: before the launch the caller's values, or (stage(..., false, ...)) the sentinel in every word; read back whole after it.
struct LaunchFrames {
	const int * aov; int count; void * frames, * normal_and_depth, * mesh_id_and_triangle_id, * screen_position_prev;   // the caller's: 4, 4, 2 and 2 words a pixel
	float4 * dev_frames[4] = { }; float4 * g_nd = nullptr; int2 * g_id = nullptr; float2 * g_sp = nullptr;
	void stage(Probe & probe, size_t pixels, bool callers_values, uint32_t sentinel) {
		auto image = [&](const void * host, size_t words) { return probe.words(pixels * words, callers_values ? host : nullptr, sentinel); };
		for (int k = 0; k < count; k++) dev_frames[k] = (float4 *)image((const uint32_t *)frames + size_t(k) * pixels * 4, 4);
		g_nd = (float4 *)image(normal_and_depth, 4); g_id = (int2 *)image(mesh_id_and_triangle_id, 2); g_sp = (float2 *)image(screen_position_prev, 2);
	}
	// the launch has these frames where the context has the AOV, and no other
	void patch(const rt_context * ctx, RtParams & p) const {
		for (int a = 0; a < RT_AOV_COUNT; a++) p.aovs[a].framebuffer = nullptr;
		for (int k = 0; k < count; k++) if (ctx->aov_buffers[aov[k]][0]) p.aovs[aov[k]].framebuffer = dev_frames[k];
		p.gbuffer_normal_and_depth = g_nd; p.gbuffer_mesh_id_and_triangle_id = g_id; p.gbuffer_screen_position_prev = g_sp;
	}
	int read(Probe & probe, size_t pixels) const {
		int s = RT_OK;
		for (int k = 0; k < count && s == RT_OK; k++) s = probe.read((uint32_t *)frames + size_t(k) * pixels * 4, dev_frames[k], pixels * 16);
		if (s || (s = probe.read(normal_and_depth, g_nd, pixels * 16)) || (s = probe.read(mesh_id_and_triangle_id, g_id, pixels * 8))) return s;
		return probe.read(screen_position_prev, g_sp, pixels * 8);
	}
};
} // namespace

// rt_sort_rays: the sort launch (rt_launch_sort or rt_launch_sort_stream, as the per-bounce loop and stream_enqueue_iteration call them) on an
// explicit trace queue. The parameter block is the context's (ctx->params, or stream_params(ctx, iteration)) with both trace queues, the four
// material queues, the counters (RtBufferSizes) or the control block and slot table, the AOV frames, the g-buffers and the pixel-query word
// replaced by buffers of this call, every output array filled with the caller's sentinel. Runs on the main stream after quiesce().
// rt_sort_rays_fog is the same call with a shadow queue (shadow_out / shadow_count, both null for rt_sort_rays): the ..._fog instance appends the light
// samples of its scatter vertices to it. The messages name rt_sort_rays either way.
static int sort_rays_probe(rt_context * ctx, int merged, int step, int sample_index, const uint32_t * trace_in, size_t count,
                           const int32_t * slot_table, size_t slot_count, const int32_t * submission_birth,
                           size_t capacity, size_t frame_slots, uint32_t sentinel,
                           uint32_t * trace_out, uint32_t * material_out, int32_t * counters6,
                           float * aov_frames, float * gbuffer_normal_and_depth, int32_t * gbuffer_mesh_id_and_triangle_id, float * gbuffer_screen_position_prev,
                           int32_t * pixel_query2, int32_t * stats, uint32_t * shadow_out, int32_t * shadow_count) {
	const QueueLaunch a = { ctx, "rt_sort_rays", merged, step, count, slot_table, slot_count, submission_birth, capacity, frame_slots };
	const bool arrays = (trace_in || count == 0) && trace_out && material_out && counters6 && aov_frames && gbuffer_normal_and_depth &&
	                    gbuffer_mesh_id_and_triangle_id && gbuffer_screen_position_prev && pixel_query2;
	int s = queue_launch_arguments(a, arrays ? nullptr : "NULL array", slot_table && submission_birth && stats, RT_MAX_BOUNCES); if (s) return s;
	if ((s = queue_launch_entries<RtTraceBuffer>(a, trace_in, true, [](size_t, int32_t) { return int(RT_OK); }))) return s;
	RT_HIP(ctx, quiesce(ctx));
	s = sky_sampling_prepare(ctx, a.name); if (s) return s;   // (as a render settles it: it decides the instance)

	Probe probe(ctx, a.name);
	const int q = step & 1; const size_t pixels = a.pixels();
	const RtTraceBuffer in = probe.queue<RtTraceBuffer>(trace_in, count, capacity, sentinel), out = probe.queue<RtTraceBuffer>(capacity, sentinel);
	RtMaterialBuffer material[4];
	for (RtMaterialBuffer & m : material) m = probe.queue<RtMaterialBuffer>(capacity, sentinel);
	const RtShadowBuffer shadow = shadow_out ? probe.queue<RtShadowBuffer>(capacity, sentinel) : RtShadowBuffer { };
	static const int frame_aov[4] = { RT_AOV_RADIANCE, RT_AOV_RADIANCE_DIRECT, RT_AOV_RADIANCE_INDIRECT, RT_AOV_ALBEDO };
	LaunchFrames frames = { frame_aov, 4, aov_frames, gbuffer_normal_and_depth, gbuffer_mesh_id_and_triangle_id, gbuffer_screen_position_prev };
	frames.stage(probe, pixels, true, sentinel);
	int * query = probe.array<int>(2, pixel_query2);
	LaunchCounters counters;
	counters.stage(probe, merged != 0, [&](RtStreamControl & c) { c.trace_count[q] = int(count); }, [&](RtBufferSizes & z) { z.trace[step] = int(count); }, slot_table, slot_count, submission_birth);
	if ((s = probe.allocated())) return s;

	RtParams p = merged ? stream_params(ctx, step) : ctx->params;
	p.trace[q] = in; p.trace[q ^ 1] = out;
	if (shadow_out) p.shadow = shadow; else p.fog_active = 0;   // (rt_sort_rays: the instances it always launched; the ..._fog ones need this call's shadow queue)
	for (int m = 0; m < 4; m++) p.material[m] = material[m];
	counters.patch(p); frames.patch(ctx, p);
	p.pixel_query_out = query;
	if (merged) rt_launch_sort_stream(p, ctx->stream); else rt_launch_sort(p, step, sample_index, ctx->stream);
	if ((s = probe.finish(ctx->stream))) return s;

	bool read = probe.queue_back(out, trace_out, capacity, sentinel);
	for (int m = 0; m < 4; m++) read = read && probe.queue_back(material[m], material_out + size_t(m) * capacity * RT_SORT_MATERIAL_WORDS, capacity, sentinel);
	if (shadow_out) read = read && probe.queue_back(shadow, shadow_out, capacity, sentinel);
	if (!read) return fail(ctx, RT_ERROR_HIP, "%s: reading the queues back failed", a.name);
	if ((s = counters.read(probe, stats))) return s;
	if (merged) {
		const RtStreamControl & c = *counters.control_host;
		if (shadow_count) *shadow_count = c.shadow_count[q];
		for (int m = 0; m < 4; m++) counters6[m] = c.material_count[m];
		counters6[4] = c.trace_count[q ^ 1]; counters6[5] = c.trace_count[q];
	} else {
		RtBufferSizes & z = counters.sizes_host;
		if (shadow_count) *shadow_count = z.shadow[step];
		for (int m = 0; m < 4; m++) counters6[m] = material_sizes(z, m)[step];
		counters6[4] = step + 1 < RT_MAX_BOUNCES ? z.trace[step + 1] : 0; counters6[5] = z.trace[step];
	}
	if ((s = frames.read(probe, pixels))) return s;
	return probe.read(pixel_query2, query, 8);
}

// rt_fog_segments and rt_fog_density_segments after their NULL checks: the fog's segment step on explicit segments, on the volume (density: and the grid) in force.
static int fog_segments_probe(rt_context * ctx, const char * name, bool density, const uint32_t * probes, size_t count, uint32_t * out) {
	if (count > size_t(1) << 24) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: more than 2^24 probes", name);
	if (!ctx->fog_set) return fail(ctx, RT_ERROR_NOT_READY, "%s: no fog volume set (rt_set_fog_volume)", name);
	if (density && !ctx->fog_grid_set) return fail(ctx, RT_ERROR_NOT_READY, "%s: no density grid set (rt_set_fog_density)", name);
	(void)hipSetDevice(ctx->device);
	int s = check_ready(ctx, name, NEED_RNG | NEED_FRAME); if (s) return s;
	for (size_t i = 0; i < count; i++) {
		const uint32_t * a = probes + i * RT_FOG_SEGMENT_IN;
		if (a[7] >= 1u << 30) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: probe %zu: pixel %u beyond the 30-bit path index", name, i, a[7]);
		if (a[8] >= unsigned(RT_MAX_BOUNCES)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: probe %zu: bounce %u outside [0, RT_MAX_BOUNCES)", name, i, a[8]);
	}
	if (count == 0) return RT_OK;
	Probe probe(ctx, name);
	uint32_t * dev_probes = probe.array<uint32_t>(count * RT_FOG_SEGMENT_IN, probes);
	uint32_t * dev_out = probe.array<uint32_t>(count * RT_FOG_SEGMENT_OUT);
	if ((s = probe.allocated())) return s;
	// (a grid of zeros, or a volume without density, is marched as it is: the device fields are set whenever a grid is)
	(density ? rt_launch_fog_density_segments : rt_launch_fog_segments)(ctx->params, dev_probes, int(count), dev_out, ctx->stream);
	return probe.finish_and_read(out, dev_out, count * RT_FOG_SEGMENT_OUT * 4);
}

extern "C" {

int rt_sort_rays(rt_context * ctx, int merged, int step, int sample_index, const uint32_t * trace_in, size_t count,
                 const int32_t * slot_table, size_t slot_count, const int32_t * submission_birth,
                 size_t capacity, size_t frame_slots, uint32_t sentinel,
                 uint32_t * trace_out, uint32_t * material_out, int32_t * counters6,
                 float * aov_frames, float * gbuffer_normal_and_depth, int32_t * gbuffer_mesh_id_and_triangle_id, float * gbuffer_screen_position_prev,
                 int32_t * pixel_query2, int32_t * stats) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_sort_rays: NULL context");
	return sort_rays_probe(ctx, merged, step, sample_index, trace_in, count, slot_table, slot_count, submission_birth, capacity, frame_slots, sentinel, trace_out, material_out, counters6,
	                       aov_frames, gbuffer_normal_and_depth, gbuffer_mesh_id_and_triangle_id, gbuffer_screen_position_prev, pixel_query2, stats, nullptr, nullptr);
}

int rt_sort_rays_fog(rt_context * ctx, int merged, int step, int sample_index, const uint32_t * trace_in, size_t count,
                     const int32_t * slot_table, size_t slot_count, const int32_t * submission_birth,
                     size_t capacity, size_t frame_slots, uint32_t sentinel,
                     uint32_t * trace_out, uint32_t * material_out, int32_t * counters6,
                     float * aov_frames, float * gbuffer_normal_and_depth, int32_t * gbuffer_mesh_id_and_triangle_id, float * gbuffer_screen_position_prev,
                     int32_t * pixel_query2, int32_t * stats, uint32_t * shadow_out, int32_t * shadow_count) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_sort_rays_fog: NULL context");
	RT_REQUIRE(ctx, shadow_out && shadow_count, "rt_sort_rays_fog: NULL shadow queue or counter");
	if (!ctx->params.fog_active) return fail(ctx, RT_ERROR_NOT_READY, "rt_sort_rays_fog: no fog volume of positive density is in force (rt_set_fog_volume)");
	RT_REQUIRE(ctx, !ctx->params.config.enable_svgf, "rt_sort_rays_fog: a fog volume cannot be rendered with enable_svgf");
	return sort_rays_probe(ctx, merged, step, sample_index, trace_in, count, slot_table, slot_count, submission_birth, capacity, frame_slots, sentinel, trace_out, material_out, counters6,
	                       aov_frames, gbuffer_normal_and_depth, gbuffer_mesh_id_and_triangle_id, gbuffer_screen_position_prev, pixel_query2, stats, shadow_out, shadow_count);
}

// rt_fog_segments: the fog's segment step (rt_fog.h: clip, hashed pair, distance sample) on explicit segments, on the volume in force.
int rt_fog_segments(rt_context * ctx, const uint32_t * probes, size_t count, uint32_t * out) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_fog_segments: NULL context");
	RT_REQUIRE(ctx, (probes && out) || count == 0, "rt_fog_segments: NULL argument");
	return fog_segments_probe(ctx, "rt_fog_segments", false, probes, count, out);
}

// rt_fog_density_segments: the segment step over the density grid in force (rt_fog_grid.h: the voxel march under the same clip, pair and weights), on
// rt_fog_segments' records.
int rt_fog_density_segments(rt_context * ctx, const uint32_t * probes, size_t count, uint32_t * out) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_fog_density_segments: NULL context");
	RT_REQUIRE(ctx, (probes && out) || count == 0, "rt_fog_density_segments: NULL argument");
	return fog_segments_probe(ctx, "rt_fog_density_segments", true, probes, count, out);
}

// rt_attenuate_shadow_rays: the fog's attenuation pass, as the context's scheduler launches it, on an explicit shadow queue. The parameter block is the
// context's with the shadow queue and the word the launch reads its count from replaced by buffers of this call.
int rt_attenuate_shadow_rays(rt_context * ctx, const uint32_t * shadow_in, size_t count, uint32_t * shadow_out) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_attenuate_shadow_rays: NULL context");
	RT_REQUIRE(ctx, (shadow_in && shadow_out) || count == 0, "rt_attenuate_shadow_rays: NULL argument");
	RT_REQUIRE(ctx, count <= size_t(1) << 28, "rt_attenuate_shadow_rays: more than 2^28 rays");
	if (!ctx->fog_set) return fail(ctx, RT_ERROR_NOT_READY, "rt_attenuate_shadow_rays: no fog volume set (rt_set_fog_volume)");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	const bool merged = ctx->scheduler == RT_SCHEDULER_MERGED;
	Probe probe(ctx, "rt_attenuate_shadow_rays");
	const RtShadowBuffer shadow = probe.queue<RtShadowBuffer>(shadow_in, count, count, 0u);   // (a queue of exactly `count` entries: nothing to fill)
	LaunchCounters counters;
	counters.stage(probe, merged, [&](RtStreamControl & c) { c.shadow_count[0] = int(count); }, [&](RtBufferSizes & z) { z.shadow[0] = int(count); });
	int s = probe.allocated(); if (s) return s;
	RtParams p = ctx->params;
	p.shadow = shadow; p.sizes = counters.sizes; p.stream = counters.control; p.stream_iteration = 0;
	if (merged) rt_launch_fog_attenuate_shadows_stream(p, ctx->stream); else rt_launch_fog_attenuate_shadows(p, 0, ctx->stream);
	if ((s = probe.finish(ctx->stream))) return s;
	if (count == 0) return RT_OK;
	if (!probe.queue_back(shadow, shadow_out, count, 0u)) return fail(ctx, RT_ERROR_HIP, "rt_attenuate_shadow_rays: reading the queue back failed");
	return RT_OK;
}

// rt_shade_rays: the material launch (rt_launch_material or rt_launch_material_stream, as the per-bounce loop and stream_enqueue_iteration call them) on an
// explicit material queue. The parameter block is the context's (ctx->params, or stream_params(ctx, iteration)) with the material queue of `material_slot`,
// the next trace queue, the shadow queue, the counters (RtBufferSizes) or the control block and slot table, the ALBEDO / NORMAL / POSITION frames and the
// g-buffers replaced by buffers of this call, every one filled with the caller's sentinel. Runs on the main stream after quiesce().
int rt_shade_rays(rt_context * ctx, int merged, int step, int sample_index, int material_slot, const uint32_t * material_in, size_t count,
                  const int32_t * slot_table, size_t slot_count, const int32_t * submission_birth,
                  size_t capacity, size_t frame_slots, uint32_t sentinel,
                  uint32_t * trace_out, uint32_t * shadow_out, int32_t * counters3,
                  uint32_t * aov_frames, uint32_t * gbuffer_normal_and_depth, uint32_t * gbuffer_mesh_id_and_triangle_id, uint32_t * gbuffer_screen_position_prev,
                  int32_t * stats) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_shade_rays: NULL context");
	const QueueLaunch a = { ctx, "rt_shade_rays", merged, step, count, slot_table, slot_count, submission_birth, capacity, frame_slots };
	const bool arrays = (material_in || count == 0) && trace_out && shadow_out && counters3 && aov_frames && gbuffer_normal_and_depth &&
	                    gbuffer_mesh_id_and_triangle_id && gbuffer_screen_position_prev;
	const char * own = material_slot < 0 || material_slot >= 4 ? "material_slot must be 0 (diffuse), 1 (plastic), 2 (dielectric) or 3 (conductor)" : arrays ? nullptr : "NULL array";
	int s = queue_launch_arguments(a, own, slot_table && submission_birth && stats, RT_MAX_BOUNCES - 1); if (s) return s;
	RT_HIP(ctx, quiesce(ctx));
	std::vector<int32_t> mesh_material(ctx->mesh_count);
	if (count) RT_HIP(ctx, hipMemcpy(mesh_material.data(), ctx->params.mesh_material_ids, ctx->mesh_count * 4, hipMemcpyDeviceToHost));
	s = queue_launch_entries<RtMaterialBuffer>(a, material_in, false, [&](size_t i, int32_t mesh_id) -> int {   // ... and the entry sits in its material's queue
		const int32_t material_id = mesh_material[mesh_id];
		if (material_id < 0 || size_t(material_id) >= ctx->material_type_list.size() || int(ctx->material_type_list[material_id]) != RT_MATERIAL_DIFFUSE + material_slot)
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_shade_rays: entry %zu: the material of instance %d (material %d) does not belong to queue %d", i, mesh_id, material_id, material_slot);
		return RT_OK;
	});
	if (s) return s;
	if (material_slot >= 2) { s = ensure_luts(ctx); if (s) return s; }   // (as a render settles them)
	s = sky_sampling_prepare(ctx, a.name); if (s) return s;   // (... and this: it decides the instance)

	Probe probe(ctx, a.name);
	const int q = step & 1; const size_t pixels = a.pixels();
	const RtMaterialBuffer in = probe.queue<RtMaterialBuffer>(material_in, count, capacity, sentinel);
	const RtTraceBuffer out = probe.queue<RtTraceBuffer>(capacity, sentinel);
	const RtShadowBuffer shadow = probe.queue<RtShadowBuffer>(capacity, sentinel);
	static const int frame_aov[3] = { RT_AOV_ALBEDO, RT_AOV_NORMAL, RT_AOV_POSITION };
	LaunchFrames frames = { frame_aov, 3, aov_frames, gbuffer_normal_and_depth, gbuffer_mesh_id_and_triangle_id, gbuffer_screen_position_prev };
	frames.stage(probe, pixels, false, sentinel);
	LaunchCounters counters;
	counters.stage(probe, merged != 0, [&](RtStreamControl & c) { c.material_count[material_slot] = int(count); }, [&](RtBufferSizes & z) { material_sizes(z, material_slot)[step] = int(count); },
	               slot_table, slot_count, submission_birth);
	if ((s = probe.allocated())) return s;

	RtParams p = merged ? stream_params(ctx, step) : ctx->params;
	p.trace[q] = RtTraceBuffer { }; p.trace[q ^ 1] = out;   // (the launch appends to the next trace queue and never looks at this bounce's)
	for (int m = 0; m < 4; m++) p.material[m] = RtMaterialBuffer { };
	p.material[material_slot] = in;
	p.shadow = shadow;
	counters.patch(p); frames.patch(ctx, p);
	p.pixel_query_out = nullptr;
	if (merged) rt_launch_material_stream(p, material_slot, ctx->stream); else rt_launch_material(p, material_slot, step, sample_index, ctx->stream);
	if ((s = probe.finish(ctx->stream))) return s;

	if (!probe.queue_back(out, trace_out, capacity, sentinel) || !probe.queue_back(shadow, shadow_out, capacity, sentinel)) return fail(ctx, RT_ERROR_HIP, "%s: reading the queues back failed", a.name);
	if ((s = counters.read(probe, stats))) return s;
	if (merged) {
		const RtStreamControl & c = *counters.control_host;
		counters3[0] = c.trace_count[q ^ 1]; counters3[1] = c.shadow_count[q]; counters3[2] = c.material_count[material_slot];
	} else {
		RtBufferSizes & z = counters.sizes_host;
		counters3[0] = z.trace[step + 1]; counters3[1] = z.shadow[step]; counters3[2] = material_sizes(z, material_slot)[step];
	}
	return frames.read(probe, pixels);
}

// The three accumulate probes -- rt_accumulate_frames, rt_accumulate_list_frames, rt_accumulate_cascade_frames -- after their own NULL and mode checks: ONE
// launch of rt_launch_accumulate, as rt_render_samples (merged false: a batch) and stream_complete (merged: a group) make it, on explicit images. The parameter
// block is the context's with every AOV but RADIANCE taken away, RADIANCE's frames and accumulator and the final image replaced by buffers of this call. list
// null: the pixel set is the context's, which must not cover a list (without_list: where to go then). indices_enter: first_sample reaches the fold, so it is
// held below 2^24. moments, and cascade with tiers, may be null. Runs on the main stream after quiesce().
static int accumulate_probe(rt_context * ctx, const char * name, bool merged, bool indices_enter, const char * without_list, const int32_t * first_sample, const int32_t * sample_count,
                            size_t submissions, float * frames, float * accumulator, float * moments, const uint32_t * list, size_t list_count, const rt_firefly_params * cascade,
                            float * tiers, uint32_t sentinel, float * final_image) {
	if (submissions < 1 || submissions > size_t(merged ? RT_ACCUMULATE_GROUP : 1))
		return fail(ctx, RT_ERROR_INVALID_ARG, merged ? "%s: 1 to RT_ACCUMULATE_GROUP submissions" : "%s: the batch form takes one submission", name);
	RtAccumulate a = { };
	size_t total = 0;
	for (size_t k = 0; k < submissions; k++) {
		if (first_sample[k] < 0 || sample_count[k] < 1 || sample_count[k] > RT_STREAM_SAMPLE_SLOTS) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: a first sample below 0 or a sample count outside [1, 512]", name);
		if (!merged && sample_count[k] > RT_MAX_BATCH_SAMPLES) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: a batch holds at most 16 samples", name);
		if (indices_enter && size_t(first_sample[k]) + size_t(sample_count[k]) > size_t(1) << 24) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: sample indices must stay below 2^24", name);
		a.group.first_sample[k] = first_sample[k]; a.group.sample_count[k] = sample_count[k]; a.group.slot_base[k] = int(total);
		total += size_t(sample_count[k]);
	}
	a.group.count = int(submissions); a.clear = merged;
	(void)hipSetDevice(ctx->device);
	const size_t frame_pixels = ctx->frame_pixels;
	if (frame_pixels == 0) return fail(ctx, RT_ERROR_NOT_READY, "%s: rt_resize was not called", name);
	if (total > size_t(RT_STREAM_SAMPLE_SLOTS) || total * frame_pixels >= size_t(1) << 30) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: at most 512 samples and fewer than 2^30 pixels in all", name);
	int s;
	if (list) {   // before any launch: every entry inside the frame, no pixel twice (two threads folding one pixel would race)
		const size_t frame = size_t(ctx->params.screen_width) * size_t(ctx->params.screen_height);
		if (list_count < 1 || list_count > frame) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: the list holds 1 to width * height entries", name);
		PixelsOnce once(frame);
		for (size_t i = 0; i < list_count; i++) {
			const PixelsOnce::Named named = once.name(list[i]);
			if (named == PixelsOnce::BEYOND) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: list entry %zu (%u) lies outside the %zu pixel frame", name, i, list[i], frame);
			if (named == PixelsOnce::TWICE) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: list entry %zu names pixel %u a second time", name, i, list[i]);
		}
		a.pixel_count = int(list_count);
	} else {
		if (ctx->pixel_list_on) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: the context covers a pixel list (rt_set_pixel_list); %s", name, without_list);
		if ((s = resolve_pixel_range(ctx, name, &a.pixel_offset, &a.pixel_count))) return s;
	}
	RT_HIP(ctx, quiesce(ctx));

	Probe probe(ctx, name);
	const size_t tier_pixels = cascade ? frame_pixels * size_t(cascade->tiers) : 0;
	float4 * dev_frames = probe.array<float4>(total * frame_pixels, frames);
	float4 * dev_accumulator = probe.array<float4>(frame_pixels, accumulator);
	if (moments) a.moments = probe.array<float4>(frame_pixels, moments);
	if (cascade) a.tiers = { probe.array<float4>(tier_pixels, tiers), frame_pixels, cascade->tiers, cascade->start };
	if (list) a.list = probe.array<unsigned>(list_count, list);
	float4 * dev_final = (float4 *)probe.words(frame_pixels * 4, nullptr, sentinel);
	if ((s = probe.allocated())) return s;

	RtParams p = ctx->params;
	for (int v = 0; v < RT_AOV_COUNT; v++) p.aovs[v].framebuffer = p.aovs[v].accumulator = nullptr;
	p.aovs[RT_AOV_RADIANCE].framebuffer = dev_frames; p.aovs[RT_AOV_RADIANCE].accumulator = dev_accumulator;
	p.final_image = dev_final;
	rt_launch_accumulate(p, a, ctx->stream);
	if ((s = probe.finish())) return s;
	if ((s = probe.read(frames, dev_frames, total * frame_pixels * 16)) || (s = probe.read(accumulator, dev_accumulator, frame_pixels * 16))) return s;
	if (moments && (s = probe.read(moments, a.moments, frame_pixels * 16))) return s;
	if (cascade && (s = probe.read(tiers, a.tiers.tiers, tier_pixels * 16))) return s;
	return probe.read(final_image, dev_final, frame_pixels * 16);
}

int rt_accumulate_frames(rt_context * ctx, int merged, const int32_t * first_sample, const int32_t * sample_count, size_t submissions,
                         float * frames, float * accumulator, float * moments, uint32_t sentinel, float * final_image) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_accumulate_frames: NULL context");
	RT_REQUIRE(ctx, merged == 0 || merged == 1, "rt_accumulate_frames: merged must be 0 (one batch) or 1 (a group of submissions)");
	RT_REQUIRE(ctx, first_sample && sample_count && frames && accumulator && final_image, "rt_accumulate_frames: NULL array");
	return accumulate_probe(ctx, "rt_accumulate_frames", merged != 0, true, "rt_accumulate_list_frames is the probe of that launch", first_sample, sample_count, submissions, frames, accumulator,
	                        moments, nullptr, 0, nullptr, nullptr, sentinel, final_image);
}

} // extern "C"

// The estimate and the selection on the caller's images, after the entry points' NULL checks; each plain (resolved null: no held_fraction, cell_held or held
// count) or firefly-robust.
static int estimate_noise_images_probe(rt_context * ctx, const char * name, const float * mean, const float * moments, const float * resolved, float floor, float held_fraction,
                                       rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, int32_t * cell_held, size_t cell_capacity,
                                       float * pixel_map, int64_t * out_held_pixels) {
	if (!(floor > 0.0f && floor < __builtin_huge_valf())) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: floor must be finite and positive", name);
	int s = resolved ? held_fraction_argument(ctx, name, held_fraction) : RT_OK; if (s) return s;
	(void)hipSetDevice(ctx->device);
	if (ctx->frame_pixels == 0) return fail(ctx, RT_ERROR_NOT_READY, "%s: rt_resize was not called", name);
	RT_HIP(ctx, quiesce(ctx));
	Probe probe(ctx, name);
	const float4 * dev_mean = probe.array<float4>(ctx->frame_pixels, mean), * dev_moments = probe.array<float4>(ctx->frame_pixels, moments);
	const NoiseRobust robust = { resolved ? probe.array<float4>(ctx->frame_pixels, resolved) : nullptr, held_fraction, cell_held, out_held_pixels };
	if ((s = probe.allocated())) return s;
	return noise_estimate_images(ctx, name, dev_mean, dev_moments, floor, out, cell_sums, cell_counts, cell_nonfinite, cell_capacity, pixel_map, resolved ? &robust : nullptr);
}

static int select_pixels_images_probe(rt_context * ctx, const char * name, const float * mean, const float * moments, const float * resolved, float floor, float held_fraction,
                                      float threshold, int dilate, rt_cell_selection * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, int32_t * cell_held,
                                      uint8_t * cell_flags, size_t cell_capacity, uint32_t * list, size_t list_capacity) {
	int s = selection_arguments(ctx, name, floor, threshold, dilate); if (s) return s;
	if (resolved && (s = held_fraction_argument(ctx, name, held_fraction))) return s;
	(void)hipSetDevice(ctx->device);
	if (ctx->frame_pixels == 0) return fail(ctx, RT_ERROR_NOT_READY, "%s: rt_resize was not called", name);
	const size_t frame = size_t(ctx->params.screen_width) * size_t(ctx->params.screen_height);
	if (list_capacity < frame) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: list_capacity is below width * height", name);
	RT_HIP(ctx, quiesce(ctx));
	Probe probe(ctx, name);
	const float4 * dev_mean = probe.array<float4>(ctx->frame_pixels, mean), * dev_moments = probe.array<float4>(ctx->frame_pixels, moments);
	const NoiseRobust robust = { resolved ? probe.array<float4>(ctx->frame_pixels, resolved) : nullptr, held_fraction, cell_held, nullptr };
	unsigned * dev_list = probe.array<unsigned>(frame, list);   // (what the kernels do not write comes back as the caller gave it)
	if ((s = probe.allocated())) return s;
	if ((s = select_cells_images(ctx, name, dev_mean, dev_moments, floor, threshold, dilate, dev_list, out, cell_sums, cell_counts, cell_nonfinite, cell_flags, cell_capacity,
	                             resolved ? &robust : nullptr))) return s;
	return probe.read(list, dev_list, frame * 4);
}

extern "C" {

int rt_estimate_noise_images(rt_context * ctx, const float * mean, const float * moments, float floor, rt_noise_estimate * out, double * cell_sums,
                             int32_t * cell_counts, int32_t * cell_nonfinite, size_t cell_capacity, float * pixel_map) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_estimate_noise_images: NULL context");
	RT_REQUIRE(ctx, mean && moments && out && cell_sums && cell_counts && cell_nonfinite, "rt_estimate_noise_images: NULL argument");
	return estimate_noise_images_probe(ctx, "rt_estimate_noise_images", mean, moments, nullptr, floor, 0.0f, out, cell_sums, cell_counts, cell_nonfinite, nullptr, cell_capacity, pixel_map, nullptr);
}

int rt_select_pixels_images(rt_context * ctx, const float * mean, const float * moments, float floor, float threshold, int dilate, rt_cell_selection * out,
                            double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, uint8_t * cell_flags, size_t cell_capacity, uint32_t * list, size_t list_capacity) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_select_pixels_images: NULL context");
	RT_REQUIRE(ctx, mean && moments && out && cell_sums && cell_counts && cell_nonfinite && cell_flags && list, "rt_select_pixels_images: NULL argument");
	return select_pixels_images_probe(ctx, "rt_select_pixels_images", mean, moments, nullptr, floor, 0.0f, threshold, dilate, out, cell_sums, cell_counts, cell_nonfinite, nullptr, cell_flags,
	                                  cell_capacity, list, list_capacity);
}

int rt_denoise_images(rt_context * ctx, int width, int height, int pitch, const float * colour, const float * moments, const float * albedo, const float * normal,
                      const float * position, const float * fallback, const float * eye, const rt_denoise_params * params, int tiled, float * out) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_denoise_images: NULL context");
	RT_REQUIRE(ctx, colour && moments && albedo && normal && position && fallback && eye && out, "rt_denoise_images: NULL argument");
	int s = denoise_arguments(ctx, "rt_denoise_images", params); if (s) return s;
	RT_REQUIRE(ctx, tiled == 0 || tiled == 1, "rt_denoise_images: tiled must be 0 or 1");
	RT_REQUIRE(ctx, width > 0 && height > 0 && pitch >= width, "rt_denoise_images: width and height must be positive and pitch at least width");
	RT_REQUIRE(ctx, (long long)pitch * height < (1ll << 26), "rt_denoise_images: pitch * height must stay below 2^26");
	RT_REQUIRE(ctx, std::isfinite(eye[0]) && std::isfinite(eye[1]) && std::isfinite(eye[2]), "rt_denoise_images: eye is not finite");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	Probe probe(ctx, "rt_denoise_images");
	const size_t pixels = size_t(pitch) * size_t(height);
	RtDenoiseImages images = { probe.array<float4>(pixels, colour), probe.array<float4>(pixels, moments), probe.array<float4>(pixels, albedo), probe.array<float4>(pixels, normal),
	                           probe.array<float4>(pixels, position), probe.array<float4>(pixels, fallback), { probe.array<float4>(pixels), probe.array<float4>(pixels) },
	                           probe.array<float4>(pixels), probe.array<float4>(pixels, out), nullptr };
	if ((s = probe.allocated())) return s;
	const RtDenoiseArgs args = { width, height, pitch, params->iterations, params->sigma_l, params->sigma_n, params->sigma_z, params->depth_floor, params->albedo_floor, { eye[0], eye[1], eye[2] } };
	rt_launch_denoise(args, images, tiled != 0, ctx->stream);
	return probe.finish_and_read(out, images.out, pixels * 16);
}

int rt_accumulate_list_frames(rt_context * ctx, const int32_t * first_sample, const int32_t * sample_count, size_t submissions,
                              float * frames, float * accumulator, float * moments, const uint32_t * list, size_t list_count, uint32_t sentinel, float * final_image) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_accumulate_list_frames: NULL context");
	RT_REQUIRE(ctx, first_sample && sample_count && frames && accumulator && moments && list && final_image, "rt_accumulate_list_frames: NULL array");
	return accumulate_probe(ctx, "rt_accumulate_list_frames", true, false, nullptr, first_sample, sample_count, submissions, frames, accumulator, moments, list, list_count, nullptr, nullptr,
	                        sentinel, final_image);
}

int rt_accumulate_cascade_frames(rt_context * ctx, int merged, const int32_t * first_sample, const int32_t * sample_count, size_t submissions, float * frames,
                                 float * accumulator, float * moments, const uint32_t * list, size_t list_count, const rt_firefly_params * params, float * tiers,
                                 uint32_t sentinel, float * final_image) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_accumulate_cascade_frames: NULL context");
	RT_REQUIRE(ctx, merged == 0 || merged == 1, "rt_accumulate_cascade_frames: merged must be 0 (one batch) or 1 (a group of submissions)");
	RT_REQUIRE(ctx, first_sample && sample_count && frames && accumulator && moments && params && tiers && final_image, "rt_accumulate_cascade_frames: NULL array");
	RT_REQUIRE(ctx, !list || merged, "rt_accumulate_cascade_frames: a pixel list takes the merged form");
	int s = firefly_arguments(ctx, "rt_accumulate_cascade_frames", params->tiers, params->start, params->support); if (s) return s;
	return accumulate_probe(ctx, "rt_accumulate_cascade_frames", merged != 0, true, "pass a list", first_sample, sample_count, submissions, frames, accumulator, moments, list, list_count, params, tiers,
	                        sentinel, final_image);
}

int rt_resolve_fireflies_images(rt_context * ctx, int width, int height, int pitch, const float * mean, const float * moments, const float * tiers, const float * fallback,
                                const rt_firefly_params * params, int tiled, float * out) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_resolve_fireflies_images: NULL context");
	RT_REQUIRE(ctx, mean && moments && tiers && fallback && params && out, "rt_resolve_fireflies_images: NULL argument");
	int s = firefly_arguments(ctx, "rt_resolve_fireflies_images", params->tiers, params->start, params->support); if (s) return s;
	RT_REQUIRE(ctx, tiled == 0 || tiled == 1, "rt_resolve_fireflies_images: tiled must be 0 or 1");
	RT_REQUIRE(ctx, width > 0 && height > 0 && pitch >= width, "rt_resolve_fireflies_images: width and height must be positive and pitch at least width");
	RT_REQUIRE(ctx, (long long)pitch * height < (1ll << 26), "rt_resolve_fireflies_images: pitch * height must stay below 2^26");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	Probe probe(ctx, "rt_resolve_fireflies_images");
	const size_t pixels = size_t(pitch) * size_t(height);
	const RtFireflyResolveImages images = { probe.array<float4>(pixels, mean), probe.array<float4>(pixels, moments), probe.array<float4>(pixels, fallback),
	                                        probe.array<float4>(pixels * size_t(params->tiers), tiers), pixels, probe.array<float4>(pixels, out), nullptr };
	if ((s = probe.allocated())) return s;
	const RtFireflyResolveArgs args = { width, height, pitch, params->tiers, params->start, params->support };
	rt_launch_fireflies_resolve(args, images, tiled != 0, ctx->stream);
	return probe.finish_and_read(out, images.out, pixels * 16);
}

int rt_measure_exposure_images(rt_context * ctx, int width, int height, int pitch, const float * mean, const float * moments, rt_exposure * out, uint64_t * histogram256) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_measure_exposure_images: NULL context");
	RT_REQUIRE(ctx, mean && moments && out && histogram256, "rt_measure_exposure_images: NULL argument");
	RT_REQUIRE(ctx, width > 0 && height > 0 && pitch >= width, "rt_measure_exposure_images: width and height must be positive and pitch at least width");
	RT_REQUIRE(ctx, (long long)pitch * height < (1ll << 26), "rt_measure_exposure_images: pitch * height must stay below 2^26");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	Probe probe(ctx, "rt_measure_exposure_images");
	const size_t pixels = size_t(pitch) * size_t(height);
	const float4 * dev_mean = probe.array<float4>(pixels, mean), * dev_moments = probe.array<float4>(pixels, moments);
	int s = probe.allocated(); if (s) return s;
	return exposure_measure_images(ctx, "rt_measure_exposure_images", dev_mean, dev_moments, width, height, pitch, out, histogram256);
}

int rt_estimate_noise_robust_images(rt_context * ctx, const float * mean, const float * moments, const float * resolved, float floor, float held_fraction,
                                    rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, int32_t * cell_held, size_t cell_capacity,
                                    float * pixel_map, int64_t * out_held_pixels) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_estimate_noise_robust_images: NULL context");
	RT_REQUIRE(ctx, mean && moments && resolved && out && cell_sums && cell_counts && cell_nonfinite && cell_held, "rt_estimate_noise_robust_images: NULL argument");
	return estimate_noise_images_probe(ctx, "rt_estimate_noise_robust_images", mean, moments, resolved, floor, held_fraction, out, cell_sums, cell_counts, cell_nonfinite, cell_held, cell_capacity,
	                                   pixel_map, out_held_pixels);
}

int rt_select_pixels_robust_images(rt_context * ctx, const float * mean, const float * moments, const float * resolved, float floor, float held_fraction, float threshold,
                                   int dilate, rt_cell_selection * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, int32_t * cell_held,
                                   uint8_t * cell_flags, size_t cell_capacity, uint32_t * list, size_t list_capacity) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_select_pixels_robust_images: NULL context");
	RT_REQUIRE(ctx, mean && moments && resolved && out && cell_sums && cell_counts && cell_nonfinite && cell_held && cell_flags && list, "rt_select_pixels_robust_images: NULL argument");
	return select_pixels_images_probe(ctx, "rt_select_pixels_robust_images", mean, moments, resolved, floor, held_fraction, threshold, dilate, out, cell_sums, cell_counts, cell_nonfinite, cell_held,
	                                  cell_flags, cell_capacity, list, list_capacity);
}

int rt_measure_stream_bandwidth(rt_context * ctx, size_t bytes, int repeat, float * out_gbps) {
	RT_REQUIRE(ctx, ctx && out_gbps && bytes >= 1024, "rt_measure_stream_bandwidth: invalid argument");
	(void)hipSetDevice(ctx->device);
	Probe probe(ctx, "rt_measure_stream_bandwidth");
	size_t count = bytes / 16;
	float4 * src = probe.array<float4>(count);
	float * sink = probe.array<float>(4);
	int s = probe.allocated(); if (s) return s;
	RT_HIP(ctx, hipMemsetAsync(src, 0x3c, count * 16, ctx->stream));
	if (repeat < 1) repeat = 1;
	rt_launch_stream_read(src, count, sink, ctx->stream); // warm-up
	float best = 1e30f;
	for (int r = 0; r < repeat; r++) {
		float ms = 0.0f;
		s = probe.time(&ms, [&] { rt_launch_stream_read(src, count, sink, ctx->stream); }); if (s) return s;
		if (ms < best) best = ms;
	}
	*out_gbps = float(double(count * 16) / (double(best) * 1e-3) / 1e9);
	return RT_OK;
}

} // extern "C"
