// rt_denoise.hip -- the part of the C ABI (include/gpu_raytracer_amd.h) that is the still-image denoiser: the filter's images as the context keeps
// them and the entry points on the context's frame. The probe on explicit images, rt_denoise_images, is in rt_probes.hip; both run rt_launch_denoise.
#include "rt_context.h"

#include <cmath>

// The caller has quiesced the context.
void denoise_free(rt_context * ctx) {
	for (void *& image : ctx->denoise_images) { if (image) device_free(ctx, image); image = nullptr; }
	if (ctx->denoise_guide) { device_free(ctx, ctx->denoise_guide); ctx->denoise_guide = nullptr; }
	if (ctx->denoise_any_valid) { device_free(ctx, ctx->denoise_any_valid); ctx->denoise_any_valid = nullptr; }
	ctx->denoise_result = -1;
}

int denoise_arguments(rt_context * ctx, const char * caller, const rt_denoise_params * params) {
	if (!params) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: NULL params", caller);
	if (params->iterations < 0 || params->iterations > 6) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: iterations must be 0..6, not %d", caller, params->iterations);
	const struct { float value; const char * name; bool positive; } checks[] = {
		{ params->sigma_l, "sigma_l", false }, { params->sigma_n, "sigma_n", false }, { params->sigma_z, "sigma_z", false },
		{ params->depth_floor, "depth_floor", true }, { params->albedo_floor, "albedo_floor", true } };
	for (const auto & c : checks) {
		if (!std::isfinite(c.value)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: %s is not finite", caller, c.name);
		if (c.positive ? !(c.value > 0.0f) : !(c.value >= 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: %s must be %s", caller, c.name, c.positive ? "above 0" : "at least 0");
	}
	return RT_OK;
}

namespace {
struct KernelTimes { rt_context * ctx; std::vector<hipEvent_t> events; };
void record_kernel(void * user, int, hipStream_t stream) {
	KernelTimes * t = (KernelTimes *)user;
	hipEvent_t e = nullptr;
	if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, stream); t->events.push_back(e); }
}
}

// rt_denoise and rt_denoise_timed (kernel_ms != nullptr)
static int denoise_frame(rt_context * ctx, const char * caller, const rt_denoise_params * params, bool tiled, float * kernel_ms, size_t capacity, size_t * out_count) {
	int s = denoise_arguments(ctx, caller, params); if (s) return s;
	(void)hipSetDevice(ctx->device);
	const RtParams & p = ctx->params;
	if (!ctx->noise_moments || !ctx->aov_buffers[RT_AOV_RADIANCE][1])
		return fail(ctx, RT_ERROR_NOT_READY, "%s: the noise estimate is off (rt_set_noise_estimate) or rt_resize was not called: the filter needs the measured variance", caller);
	static const struct { int aov; const char * name; } guides[] = { { RT_AOV_ALBEDO, "ALBEDO" }, { RT_AOV_NORMAL, "NORMAL" }, { RT_AOV_POSITION, "POSITION" } };
	for (const auto & g : guides) if (!((p.config.aov_mask >> g.aov) & 1u) || !ctx->aov_buffers[g.aov][1])
		return fail(ctx, RT_ERROR_NOT_READY, "%s: the %s AOV is not enabled (rt_set_config, aov_mask): the filter needs it as a guide", caller, g.name);
	if (p.config.enable_svgf) return fail(ctx, RT_ERROR_NOT_READY, "%s: SVGF is on: its frames keep no moments and are filtered already", caller);
	const size_t kernels = params->iterations == 0 ? 2 : size_t(params->iterations) + 1;
	if (kernel_ms && capacity < kernels) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: capacity %zu is below the %zu kernels of the run", caller, capacity, kernels);
	RT_HIP(ctx, quiesce(ctx));
	const float4 * colour = (const float4 *)ctx->aov_buffers[RT_AOV_RADIANCE][1];
	if (ctx->denoise_source == RT_DENOISE_SOURCE_RESOLVED) {   // (after quiesce: the folds in flight are counted)
		if (!ctx->firefly_resolved || ctx->firefly_resolved_at == 0) return fail(ctx, RT_ERROR_NOT_READY, "%s: the source is the resolved image (rt_set_denoise_source) and none exists (rt_resolve_fireflies)", caller);
		if (ctx->firefly_resolved_at != ctx->folds) return fail(ctx, RT_ERROR_NOT_READY, "%s: the resolved image is older than the frame: samples were folded in since (rt_resolve_fireflies)", caller);
		colour = (const float4 *)ctx->firefly_resolved;
	}
	for (void *& image : ctx->denoise_images) if (!image) { s = device_alloc(ctx, &image, ctx->frame_pixels * 16); if (s) return s; RT_HIP(ctx, hipMemset(image, 0, ctx->frame_pixels * 16)); }
	if (!ctx->denoise_guide) { s = device_alloc(ctx, &ctx->denoise_guide, ctx->frame_pixels * 16); if (s) return s; }
	if (!ctx->denoise_any_valid) { s = device_alloc(ctx, (void **)&ctx->denoise_any_valid, 16); if (s) return s; }

	// the pair: the two images that do not hold the last result; the run's last kernel writes into the one its input is not
	int pair[2], n = 0;
	for (int i = 0; i < 3 && n < 2; i++) if (i != ctx->denoise_result) pair[n++] = i;
	const int last_input = params->iterations == 0 ? 0 : (params->iterations - 1) & 1;
	RtDenoiseArgs args = { p.screen_width, p.screen_height, p.screen_pitch, params->iterations, params->sigma_l, params->sigma_n, params->sigma_z, params->depth_floor, params->albedo_floor,
	                       { p.camera.position[0], p.camera.position[1], p.camera.position[2] } };
	RtDenoiseImages images = { colour, (const float4 *)ctx->noise_moments, (const float4 *)ctx->aov_buffers[RT_AOV_ALBEDO][1],
	                           (const float4 *)ctx->aov_buffers[RT_AOV_NORMAL][1], (const float4 *)ctx->aov_buffers[RT_AOV_POSITION][1], (const float4 *)ctx->final_image,
	                           { (float4 *)ctx->denoise_images[pair[0]], (float4 *)ctx->denoise_images[pair[1]] }, (float4 *)ctx->denoise_guide,
	                           (float4 *)ctx->denoise_images[pair[last_input ^ 1]], ctx->denoise_any_valid };
	KernelTimes times = { ctx, { } };
	hipError_t e = hipMemsetAsync(ctx->denoise_any_valid, 0, 4, ctx->stream);
	if (e == hipSuccess) {
		rt_launch_denoise(args, images, tiled, ctx->stream, kernel_ms ? record_kernel : nullptr, &times);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	int valid = 0;
	if (e == hipSuccess) e = hipMemcpy(&valid, ctx->denoise_any_valid, 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && kernel_ms && times.events.size() == kernels + 1) {
		for (size_t k = 0; k < kernels && e == hipSuccess; k++) e = hipEventElapsedTime(&kernel_ms[k], times.events[k], times.events[k + 1]);
		if (out_count) *out_count = kernels;
	} else if (kernel_ms && e == hipSuccess) e = hipErrorUnknown;
	for (hipEvent_t ev : times.events) (void)hipEventDestroy(ev);
	if (e != hipSuccess) return fail(ctx, RT_ERROR_HIP, "%s: the filter's kernels or their copies failed: %s", caller, hipGetErrorString(e));
	if (valid == 0) return fail(ctx, RT_ERROR_NOT_READY, "%s: no pixel is valid yet (two samples past sample 0 are needed: w >= 2)", caller);
	ctx->denoise_result = pair[last_input ^ 1];
	return RT_OK;
}

extern "C" {

int rt_denoise(rt_context * ctx, const rt_denoise_params * params) {
	RT_REQUIRE(ctx, ctx, "rt_denoise: NULL context");
	return denoise_frame(ctx, "rt_denoise", params, true, nullptr, 0, nullptr);
}

int rt_denoise_timed(rt_context * ctx, const rt_denoise_params * params, int tiled, float * kernel_ms, size_t capacity, size_t * out_count) {
	RT_REQUIRE(ctx, ctx, "rt_denoise_timed: NULL context");
	RT_REQUIRE(ctx, kernel_ms && out_count, "rt_denoise_timed: NULL argument");
	RT_REQUIRE(ctx, tiled == 0 || tiled == 1, "rt_denoise_timed: tiled must be 0 or 1");
	return denoise_frame(ctx, "rt_denoise_timed", params, tiled != 0, kernel_ms, capacity, out_count);
}

int rt_read_denoised(rt_context * ctx, float * dst) {
	RT_REQUIRE(ctx, ctx, "rt_read_denoised: NULL context");
	RT_REQUIRE(ctx, dst, "rt_read_denoised: NULL argument");
	(void)hipSetDevice(ctx->device);
	if (ctx->denoise_result < 0) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_denoised: no denoised image exists (rt_denoise)");
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(dst, ctx->denoise_images[ctx->denoise_result], ctx->frame_pixels * 16, hipMemcpyDeviceToHost));
	return RT_OK;
}

} // extern "C"
