// rt_fireflies.hip -- the part of the C ABI (include/gpu_raytracer_amd.h) that is the firefly filter: the tier images as the context keeps them beside
// the moments image, and the entry points on the context's frame, the exposure measurement (7.10.1) among them. The probes on explicit images,
// rt_accumulate_cascade_frames, rt_resolve_fireflies_images and rt_measure_exposure_images, are in rt_probes.hip; they run the same launchers.
#include "rt_context.h"

#include <cmath>

int firefly_arguments(rt_context * ctx, const char * caller, int tiers, float start, float support) {
	if (tiers < 2 || tiers > RT_FIREFLY_MAX_TIERS) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: tiers must be 2..8, not %d", caller, tiers);
	if (!(std::isfinite(start) && start > 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: start must be finite and above 0", caller);
	if (!(std::isfinite(support) && support > 1.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: support must be finite and above 1", caller);
	return RT_OK;
}

// The caller has quiesced the context.
void firefly_free(rt_context * ctx) {
	for (void ** image : { &ctx->firefly_tiers, &ctx->firefly_resolved, (void **)&ctx->firefly_any_valid }) if (*image) { device_free(ctx, *image); *image = nullptr; }
	ctx->firefly_resolved_at = 0;
}

// The tiers exist exactly while the cascade is on, the moments image exists and the frame has a size; they start from zeros, as the moments do. Without the
// estimate the cascade goes off. The caller has quiesced the context and calls this after sync_noise_moments.
int sync_firefly_tiers(rt_context * ctx) {
	if (!ctx->noise_estimate && ctx->firefly_on) { ctx->firefly_on = false; ctx->noise_robust = 0.0f; firefly_free(ctx); }   // (as rt_set_firefly_cascade(ctx, NULL): the resolved image goes too)
	const bool want = ctx->firefly_on && ctx->noise_moments && ctx->frame_pixels > 0;
	if (want && !ctx->firefly_tiers) {
		const size_t bytes = ctx->frame_pixels * 16 * size_t(ctx->firefly.tiers);
		int s = device_alloc(ctx, &ctx->firefly_tiers, bytes); if (s) return s;
		RT_HIP(ctx, hipMemset(ctx->firefly_tiers, 0, bytes));
	} else if (!want && ctx->firefly_tiers) { device_free(ctx, ctx->firefly_tiers); ctx->firefly_tiers = nullptr; }
	ctx->folds++;
	return RT_OK;
}
// With the moments image: whatever zeroes it zeroes the tiers. The caller has quiesced the context.
int firefly_tiers_zero(rt_context * ctx) {
	ctx->folds++;
	if (!ctx->firefly_tiers) return RT_OK;
	RT_HIP(ctx, hipMemset(ctx->firefly_tiers, 0, ctx->frame_pixels * 16 * size_t(ctx->firefly.tiers)));
	return RT_OK;
}
// What an accumulate launch under parameter block p with a moments image splats into: none (tiers null: the plain kernels) while the cascade is off or the
// launch is an SVGF frame's. Counts the launch as a fold either way it goes.
RtFireflyTiers firefly_tiers_for(rt_context * ctx, const RtParams & p) {
	ctx->folds++;
	if (!ctx->firefly_tiers || !ctx->noise_moments || p.config.enable_svgf) return { };
	return { (float4 *)ctx->firefly_tiers, ctx->frame_pixels, ctx->firefly.tiers, ctx->firefly.start };
}

// rt_resolve_fireflies, rt_resolve_fireflies_timed (kernel_ms != nullptr) and the resolve of rt_estimate_noise_robust / the robust rt_select_active_cells (rt_noise.hip)
int firefly_resolve_frame(rt_context * ctx, const char * caller, float support, bool tiled, float * kernel_ms) {
	(void)hipSetDevice(ctx->device);
	if (!ctx->firefly_on) return fail(ctx, RT_ERROR_NOT_READY, "%s: the firefly cascade is off (rt_set_firefly_cascade)", caller);
	int s = firefly_arguments(ctx, caller, ctx->firefly.tiers, ctx->firefly.start, support); if (s) return s;
	const RtParams & p = ctx->params;
	if (p.config.enable_svgf) return fail(ctx, RT_ERROR_NOT_READY, "%s: SVGF is on: its frames are not splatted into the tiers", caller);
	if (!ctx->firefly_tiers || !ctx->noise_moments || !ctx->aov_buffers[RT_AOV_RADIANCE][1]) return fail(ctx, RT_ERROR_NOT_READY, "%s: rt_resize was not called", caller);
	RT_HIP(ctx, quiesce(ctx));
	if (!ctx->firefly_resolved) { s = device_alloc(ctx, &ctx->firefly_resolved, ctx->frame_pixels * 16); if (s) return s; RT_HIP(ctx, hipMemset(ctx->firefly_resolved, 0, ctx->frame_pixels * 16)); ctx->firefly_resolved_at = 0; }
	if (!ctx->firefly_any_valid) { s = device_alloc(ctx, (void **)&ctx->firefly_any_valid, 16); if (s) return s; }
	// (whether a pixel is valid is known only after the kernel: a run that finds none has written fallback pixels alone, and the image counts as absent)
	const RtFireflyResolveArgs args = { p.screen_width, p.screen_height, p.screen_pitch, ctx->firefly.tiers, ctx->firefly.start, support };
	const RtFireflyResolveImages images = { (const float4 *)ctx->aov_buffers[RT_AOV_RADIANCE][1], (const float4 *)ctx->noise_moments, (const float4 *)ctx->final_image,
	                                        (const float4 *)ctx->firefly_tiers, ctx->frame_pixels, (float4 *)ctx->firefly_resolved, ctx->firefly_any_valid };
	hipEvent_t begin = nullptr, end = nullptr;
	hipError_t e = hipMemsetAsync(ctx->firefly_any_valid, 0, 4, ctx->stream);
	if (e == hipSuccess && kernel_ms) { e = hipEventCreate(&begin); if (e == hipSuccess) e = hipEventCreate(&end); if (e == hipSuccess) e = hipEventRecord(begin, ctx->stream); }
	if (e == hipSuccess) { rt_launch_fireflies_resolve(args, images, tiled, ctx->stream); e = hipGetLastError(); }
	if (e == hipSuccess && kernel_ms) e = hipEventRecord(end, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	int valid = 0;
	if (e == hipSuccess) e = hipMemcpy(&valid, ctx->firefly_any_valid, 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && kernel_ms) e = hipEventElapsedTime(kernel_ms, begin, end);
	for (hipEvent_t ev : { begin, end }) if (ev) (void)hipEventDestroy(ev);
	if (e != hipSuccess) return fail(ctx, RT_ERROR_HIP, "%s: the resolve kernel or its copies failed: %s", caller, hipGetErrorString(e));
	if (valid == 0) { ctx->firefly_resolved_at = 0; return fail(ctx, RT_ERROR_NOT_READY, "%s: no pixel is valid yet (a sample past sample 0 is needed: w >= 1)", caller); }
	ctx->firefly_resolved_at = ctx->folds;
	return RT_OK;
}

// kernel_exposure_histogram on two pitched float4 images already on the device (rt_measure_exposure: the RADIANCE accumulator and the moments image;
// rt_probes.hip: the caller's), on the main stream, which the caller has drained. Shared so that the probe and the entry point cannot differ.
int exposure_measure_images(rt_context * ctx, const char * caller, const float4 * mean, const float4 * moments, int width, int height, int pitch, rt_exposure * out, uint64_t * histogram256) {
	void * dev = nullptr;
	int s = device_alloc(ctx, &dev, RT_EXPOSURE_WORDS * 8); if (s) return s;
	unsigned long long words[RT_EXPOSURE_WORDS] = { };
	hipError_t e = hipMemsetAsync(dev, 0, RT_EXPOSURE_WORDS * 8, ctx->stream);
	if (e == hipSuccess) { rt_launch_exposure_histogram(mean, moments, width, height, pitch, (unsigned long long *)dev, ctx->stream); e = hipGetLastError(); }
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess) e = hipMemcpy(words, dev, sizeof(words), hipMemcpyDeviceToHost);
	device_free(ctx, dev);
	if (e != hipSuccess) return fail(ctx, RT_ERROR_HIP, "%s: the histogram kernel or its copies failed: %s", caller, hipGetErrorString(e));
	out->pixels = 0; out->dark_pixels = int64_t(words[RT_EXPOSURE_DARK]); out->nonfinite_pixels = int64_t(words[RT_EXPOSURE_NONFINITE]);
	for (int b = 0; b < RT_EXPOSURE_BINS; b++) { histogram256[b] = uint64_t(words[b]); out->pixels += int64_t(words[b]); }
	return RT_OK;
}

extern "C" {

int rt_measure_exposure(rt_context * ctx, rt_exposure * out, uint64_t * histogram256) {
	RT_REQUIRE(ctx, ctx, "rt_measure_exposure: NULL context");
	RT_REQUIRE(ctx, out && histogram256, "rt_measure_exposure: NULL argument");
	(void)hipSetDevice(ctx->device);
	const RtParams & p = ctx->params;
	if (!ctx->noise_estimate) return fail(ctx, RT_ERROR_NOT_READY, "rt_measure_exposure: the noise estimate is off (rt_set_noise_estimate): its moments image says which pixels hold a sample");
	if (p.config.enable_svgf) return fail(ctx, RT_ERROR_NOT_READY, "rt_measure_exposure: SVGF is on: its frames keep no moments");
	if (!ctx->noise_moments || !ctx->aov_buffers[RT_AOV_RADIANCE][1]) return fail(ctx, RT_ERROR_NOT_READY, "rt_measure_exposure: rt_resize was not called");
	RT_HIP(ctx, quiesce(ctx));
	return exposure_measure_images(ctx, "rt_measure_exposure", (const float4 *)ctx->aov_buffers[RT_AOV_RADIANCE][1], (const float4 *)ctx->noise_moments, p.screen_width, p.screen_height,
	                               p.screen_pitch, out, histogram256);
}

int rt_set_firefly_cascade(rt_context * ctx, const rt_firefly_params * params) {
	RT_REQUIRE(ctx, ctx, "rt_set_firefly_cascade: NULL context");
	(void)hipSetDevice(ctx->device);
	if (params) {
		int s = firefly_arguments(ctx, "rt_set_firefly_cascade", params->tiers, params->start, params->support); if (s) return s;
		if (!ctx->noise_estimate) return fail(ctx, RT_ERROR_NOT_READY, "rt_set_firefly_cascade: the noise estimate is off (rt_set_noise_estimate): the tiers live beside its moments image");
	}
	RT_HIP(ctx, quiesce(ctx));   // the accumulate launches in flight were enqueued with or without the tiers
	if (!params) { ctx->firefly_on = false; ctx->noise_robust = 0.0f; firefly_free(ctx); ctx->folds++; return RT_OK; }   // (the robust estimate follows the resolve: off with it)
	const bool same = ctx->firefly_on && ctx->firefly.tiers == params->tiers && ctx->firefly.start == params->start;
	if (same) { ctx->firefly = *params; return RT_OK; }   // (support alone: a value the host reads back)
	// The new tiers first, the old ones freed once they exist: a call that fails to allocate leaves the previous state in force.
	const rt_firefly_params previous = ctx->firefly; const bool was_on = ctx->firefly_on;
	void * old = ctx->firefly_tiers;
	ctx->firefly_tiers = nullptr; ctx->firefly = *params; ctx->firefly_on = true;
	int s = sync_firefly_tiers(ctx);
	if (s) {
		if (ctx->firefly_tiers) device_free(ctx, ctx->firefly_tiers);
		ctx->firefly_tiers = old; ctx->firefly = previous; ctx->firefly_on = was_on;
		return s;
	}
	if (old) device_free(ctx, old);
	ctx->firefly_resolved_at = 0;
	return RT_OK;
}

int rt_get_firefly_cascade(const rt_context * ctx, rt_firefly_params * out) {
	if (!ctx || !ctx->firefly_on) return 0;
	if (out) *out = ctx->firefly;
	return 1;
}

int rt_read_firefly_cascade(rt_context * ctx, float * dst, size_t capacity) {
	RT_REQUIRE(ctx, ctx, "rt_read_firefly_cascade: NULL context");
	RT_REQUIRE(ctx, dst, "rt_read_firefly_cascade: NULL argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->firefly_tiers) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_firefly_cascade: the firefly cascade is off (rt_set_firefly_cascade) or rt_resize was not called");
	const size_t floats = ctx->frame_pixels * 4 * size_t(ctx->firefly.tiers);
	if (capacity < floats) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_firefly_cascade: capacity %zu is below the %zu floats of %d tiers", capacity, floats, ctx->firefly.tiers);
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(dst, ctx->firefly_tiers, floats * 4, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_resolve_fireflies(rt_context * ctx, float support) {
	RT_REQUIRE(ctx, ctx, "rt_resolve_fireflies: NULL context");
	return firefly_resolve_frame(ctx, "rt_resolve_fireflies", support, true, nullptr);
}

int rt_resolve_fireflies_timed(rt_context * ctx, float support, int tiled, float * kernel_ms) {
	RT_REQUIRE(ctx, ctx, "rt_resolve_fireflies_timed: NULL context");
	RT_REQUIRE(ctx, kernel_ms, "rt_resolve_fireflies_timed: NULL argument");
	RT_REQUIRE(ctx, tiled == 0 || tiled == 1, "rt_resolve_fireflies_timed: tiled must be 0 or 1");
	return firefly_resolve_frame(ctx, "rt_resolve_fireflies_timed", support, tiled != 0, kernel_ms);
}

int rt_read_resolved(rt_context * ctx, float * dst) {
	RT_REQUIRE(ctx, ctx, "rt_read_resolved: NULL context");
	RT_REQUIRE(ctx, dst, "rt_read_resolved: NULL argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->firefly_resolved || ctx->firefly_resolved_at == 0) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_resolved: no resolved image exists (rt_resolve_fireflies)");
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(dst, ctx->firefly_resolved, ctx->frame_pixels * 16, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_set_denoise_source(rt_context * ctx, int source) {
	RT_REQUIRE(ctx, ctx, "rt_set_denoise_source: NULL context");
	RT_REQUIRE(ctx, source == RT_DENOISE_SOURCE_MEAN || source == RT_DENOISE_SOURCE_RESOLVED, "rt_set_denoise_source: source must be RT_DENOISE_SOURCE_MEAN or RT_DENOISE_SOURCE_RESOLVED");
	ctx->denoise_source = source;
	return RT_OK;
}
int rt_get_denoise_source(const rt_context * ctx) { return ctx ? ctx->denoise_source : RT_DENOISE_SOURCE_MEAN; }

} // extern "C"
