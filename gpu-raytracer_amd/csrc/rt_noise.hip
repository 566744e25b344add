// rt_noise.hip -- the part of the C ABI (include/gpu_raytracer_amd.h) that is the per-pixel noise estimate, its firefly-robust form
// and adaptive sampling: the second-moment image and the pixel list as the context keeps them, the two kernel sequences the probes share -- each
// plain or robust --, and the entry points on top.
#include "rt_context.h"

// The pixel list of adaptive sampling is a selection from one state of the moments image: dropped whenever that image is zeroed, freed with it.
// The caller has quiesced the context -- no submission in flight reads the list.
void pixel_list_drop(rt_context * ctx) { ctx->pixel_list_on = false; ctx->pixel_list_selected = false; ctx->pixel_list_count = 0; }
void pixel_list_free(rt_context * ctx) { pixel_list_drop(ctx); if (ctx->pixel_list) { device_free(ctx, ctx->pixel_list); ctx->pixel_list = nullptr; } }

// The second-moment image exists exactly while the estimate is on and the frame has a size; it starts from zeros (w == 0: no sample has reached the pixel).
// The caller has quiesced the context.
int sync_noise_moments(rt_context * ctx) {
	const bool want = ctx->noise_estimate && ctx->frame_pixels > 0;
	if (want && !ctx->noise_moments) {
		int s = device_alloc(ctx, &ctx->noise_moments, ctx->frame_pixels * 16); if (s) return s;
		RT_HIP(ctx, hipMemset(ctx->noise_moments, 0, ctx->frame_pixels * 16));
	} else if (!want && ctx->noise_moments) { device_free(ctx, ctx->noise_moments); ctx->noise_moments = nullptr; }
	if (!want) pixel_list_free(ctx);
	return sync_firefly_tiers(ctx);   // (beside the moments image, or not at all)
}
// A change of the pixel set: the moments of pixels the context no longer renders would go stale beside means that another rank's image replaces.
int noise_moments_reset(rt_context * ctx) {
	if (!ctx->noise_moments) return RT_OK;
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemset(ctx->noise_moments, 0, ctx->frame_pixels * 16));
	pixel_list_drop(ctx);
	return firefly_tiers_zero(ctx);
}
// What the accumulate launchers get as `moments` for a launch under parameter block p: the image while the estimate is on and the launch is not an SVGF frame's
// (whose accumulators are the filter's ping-pong images), else null -- the plain kernels, as before.
float4 * noise_moments_for(const rt_context * ctx, const RtParams & p) { return p.config.enable_svgf ? nullptr : (float4 *)ctx->noise_moments; }

// kernel_noise_cells on two pitched float4 images of the context's frame size, already on the device (rt_estimate_noise: the RADIANCE accumulator and the moments
// image; rt_probes.hip: the caller's), on the main stream, which the caller has drained. Shared so that the probe and the entry point cannot differ.
int noise_estimate_images(rt_context * ctx, const char * caller, const float4 * mean, const float4 * moments, float floor, rt_noise_estimate * out,
                          double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, size_t cell_capacity, float * pixel_map, const NoiseRobust * robust) {
	const RtParams & p = ctx->params;
	const int cells_x = (p.screen_width + RT_NOISE_CELL - 1) / RT_NOISE_CELL, cells_y = (p.screen_height + RT_NOISE_CELL - 1) / RT_NOISE_CELL;
	const size_t cells = size_t(cells_x) * cells_y;
	if (cell_capacity < cells) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: cell_capacity %zu is below the %d x %d cells of the frame", caller, cell_capacity, cells_x, cells_y);
	void * dev_sums = nullptr, * dev_counts = nullptr, * dev_map = nullptr;
	auto release = [&] { device_free(ctx, dev_sums); device_free(ctx, dev_counts); device_free(ctx, dev_map); };
	int s = device_alloc(ctx, &dev_sums, cells * 8);
	if (!s) s = device_alloc(ctx, &dev_counts, cells * 12);   // counts, then non-finite counts, then (robust) held counts
	if (!s && pixel_map) s = device_alloc(ctx, &dev_map, ctx->frame_pixels * 4);
	if (s) { release(); return s; }
	std::vector<float> map_host;
	hipError_t e = hipSuccess;
	if (dev_map) {   // the padding columns, which the kernel leaves alone, read as pixels that take no part
		map_host.assign(ctx->frame_pixels, -1.0f);
		e = hipMemcpyAsync(dev_map, map_host.data(), ctx->frame_pixels * 4, hipMemcpyHostToDevice, ctx->stream);
	}
	if (e == hipSuccess) {
		if (robust) rt_launch_noise_cells_robust(mean, moments, robust->resolved, p.screen_width, p.screen_height, p.screen_pitch, floor, robust->held_fraction, (float *)dev_map, (double *)dev_sums,
		                                         (int *)dev_counts, (int *)dev_counts + cells, (int *)dev_counts + 2 * cells, ctx->stream);
		else rt_launch_noise_cells(mean, moments, p.screen_width, p.screen_height, p.screen_pitch, floor, (float *)dev_map, (double *)dev_sums, (int *)dev_counts, (int *)dev_counts + cells, ctx->stream);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess) e = hipMemcpy(cell_sums, dev_sums, cells * 8, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(cell_counts, dev_counts, cells * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(cell_nonfinite, (int *)dev_counts + cells, cells * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && robust) e = hipMemcpy(robust->cell_held, (int *)dev_counts + 2 * cells, cells * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && dev_map) e = hipMemcpy(pixel_map, dev_map, ctx->frame_pixels * 4, hipMemcpyDeviceToHost);
	release();
	if (e != hipSuccess) return fail(ctx, RT_ERROR_HIP, "%s: the noise kernel or its copies failed: %s", caller, hipGetErrorString(e));
	out->cells_x = cells_x; out->cells_y = cells_y; out->pixels = 0; out->nonfinite_pixels = 0; out->mean = 0.0;
	double sum = 0.0;   // in cell order, in double: the one order every caller sees
	for (size_t c = 0; c < cells; c++) { sum += cell_sums[c]; out->pixels += cell_counts[c]; out->nonfinite_pixels += cell_nonfinite[c]; }
	if (robust && robust->held_pixels) { *robust->held_pixels = 0; for (size_t c = 0; c < cells; c++) *robust->held_pixels += robust->cell_held[c]; }
	if (out->pixels == 0) return fail(ctx, RT_ERROR_NOT_READY, "%s: no pixel takes part yet (two samples past sample 0 are needed: w >= 2)", caller);
	out->mean = sum / double(out->pixels);
	return RT_OK;
}

// The noise kernel, the selection and the compaction on two pitched float4 images of the context's frame size, already on the device, into `list` (room for
// width * height entries), on the main stream, which the caller has drained. cell_sums / cell_counts / cell_nonfinite / cell_flags may each be null.
// Shared by rt_select_active_cells and the probe so that they cannot differ.
int select_cells_images(rt_context * ctx, const char * caller, const float4 * mean, const float4 * moments, float floor, float threshold, int dilate, unsigned * list,
                        rt_cell_selection * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, uint8_t * cell_flags, size_t cell_capacity,
                        const NoiseRobust * robust) {
	const RtParams & p = ctx->params;
	const int cells_x = (p.screen_width + RT_NOISE_CELL - 1) / RT_NOISE_CELL, cells_y = (p.screen_height + RT_NOISE_CELL - 1) / RT_NOISE_CELL;
	const size_t cells = size_t(cells_x) * cells_y;
	if ((cell_sums || cell_counts || cell_nonfinite || cell_flags || (robust && robust->cell_held)) && cell_capacity < cells)
		return fail(ctx, RT_ERROR_INVALID_ARG, "%s: cell_capacity %zu is below the %d x %d cells of the frame", caller, cell_capacity, cells_x, cells_y);
	// one allocation: sums (double), then counts, non-finite counts, held counts (robust), active pixels, offsets (int each), totals (3 ints, padded to 4), flags (bytes)
	void * dev = nullptr;
	int s = device_alloc(ctx, &dev, cells * 8 + cells * 20 + 16 + cells); if (s) return s;
	double * dev_sums = (double *)dev;
	int * dev_counts = (int *)(dev_sums + cells), * dev_nonfinite = dev_counts + cells, * dev_held = dev_nonfinite + cells, * dev_active = dev_held + cells, * dev_offsets = dev_active + cells, * dev_totals = dev_offsets + cells;
	unsigned char * dev_flags = (unsigned char *)(dev_totals + 4);
	if (robust) rt_launch_noise_cells_robust(mean, moments, robust->resolved, p.screen_width, p.screen_height, p.screen_pitch, floor, robust->held_fraction, nullptr, dev_sums, dev_counts, dev_nonfinite, dev_held, ctx->stream);
	else rt_launch_noise_cells(mean, moments, p.screen_width, p.screen_height, p.screen_pitch, floor, nullptr, dev_sums, dev_counts, dev_nonfinite, ctx->stream);
	rt_launch_select_cells(dev_sums, dev_counts, dev_nonfinite, p.screen_width, p.screen_height, threshold, dilate, dev_flags, dev_active, dev_offsets, dev_totals, list, ctx->stream, robust ? dev_held : nullptr);
	int totals[3] = { 0, 0, 0 };
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess) e = hipMemcpy(totals, dev_totals, sizeof(totals), hipMemcpyDeviceToHost);
	if (e == hipSuccess && cell_sums) e = hipMemcpy(cell_sums, dev_sums, cells * 8, hipMemcpyDeviceToHost);
	if (e == hipSuccess && cell_counts) e = hipMemcpy(cell_counts, dev_counts, cells * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && cell_nonfinite) e = hipMemcpy(cell_nonfinite, dev_nonfinite, cells * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && robust && robust->cell_held) e = hipMemcpy(robust->cell_held, dev_held, cells * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && cell_flags) e = hipMemcpy(cell_flags, dev_flags, cells, hipMemcpyDeviceToHost);
	device_free(ctx, dev);
	if (e != hipSuccess) return fail(ctx, RT_ERROR_HIP, "%s: the selection kernels or their copies failed: %s", caller, hipGetErrorString(e));
	out->cells_x = cells_x; out->cells_y = cells_y; out->list_pixels = totals[0]; out->hot_cells = totals[1]; out->active_cells = totals[2];
	return RT_OK;
}

int selection_arguments(rt_context * ctx, const char * caller, float floor, float threshold, int dilate) {
	if (!(floor > 0.0f && floor < __builtin_huge_valf())) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: floor must be finite and positive", caller);
	if (!(threshold >= 0.0f && threshold < __builtin_huge_valf())) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: threshold must be finite and at least 0", caller);
	if (dilate != 0 && dilate != 1) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: dilate must be 0 or 1", caller);
	return RT_OK;
}

int held_fraction_argument(rt_context * ctx, const char * caller, float held_fraction) {
	if (!(held_fraction > 0.0f && held_fraction < 1.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: held_fraction must lie inside (0, 1)", caller);
	return RT_OK;
}

// Why a list cannot stand for this context's pixel set (null: it can): the list names pixels of the whole frame, and SVGF frames keep no moments.
static const char * pixel_list_obstacle(const rt_context * ctx) {
	const RtParams & p = ctx->params;
	if (p.tile_pixels > 0) return "a tile split is set (rt_set_pixel_tiles)";
	if (ctx->pixel_offset != 0 || (ctx->pixel_count >= 0 && ctx->pixel_count != p.screen_width * p.screen_height)) return "a pixel range other than the whole frame is set (rt_set_pixel_range)";
	if (p.config.enable_svgf) return "SVGF is on";
	return nullptr;
}

extern "C" {

// ---- noise estimate ---------------------------------------------------------------------------------

int rt_set_noise_estimate(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_noise_estimate: NULL context");
	RT_REQUIRE(ctx, enable == 0 || enable == 1, "rt_set_noise_estimate: enable must be 0 or 1");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));   // the accumulate launches in flight were enqueued with or without the image
	ctx->noise_estimate = enable != 0;
	int s = sync_noise_moments(ctx); if (s) return s;
	if (ctx->noise_moments) RT_HIP(ctx, hipMemset(ctx->noise_moments, 0, ctx->frame_pixels * 16));
	pixel_list_drop(ctx);
	return firefly_tiers_zero(ctx);
}
int rt_get_noise_estimate(const rt_context * ctx) { return ctx && ctx->noise_estimate ? 1 : 0; }

int rt_read_noise_moments(rt_context * ctx, float * dst) {
	RT_REQUIRE(ctx, ctx && dst, "rt_read_noise_moments: NULL argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->noise_moments) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_noise_moments: the noise estimate is off (rt_set_noise_estimate) or rt_resize was not called");
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy(dst, ctx->noise_moments, ctx->frame_pixels * 16, hipMemcpyDeviceToHost));
	return RT_OK;
}

// rt_estimate_noise and rt_estimate_noise_robust after their NULL checks. robust: null, or the robust form's held_fraction, cell_held and held count; its image
// is the context's, after a resolve of its own (which drains the context, and refuses while the cascade is off).
static int estimate_noise_frame(rt_context * ctx, const char * name, float floor, rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite,
                                size_t cell_capacity, float * pixel_map, NoiseRobust * robust) {
	if (!(floor > 0.0f && floor < __builtin_huge_valf())) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: floor must be finite and positive", name);
	int s = robust ? held_fraction_argument(ctx, name, robust->held_fraction) : RT_OK; if (s) return s;
	(void)hipSetDevice(ctx->device);
	if (!ctx->noise_moments || !ctx->aov_buffers[RT_AOV_RADIANCE][1]) return fail(ctx, RT_ERROR_NOT_READY, "%s: the noise estimate is off (rt_set_noise_estimate) or rt_resize was not called", name);
	if (!robust) RT_HIP(ctx, quiesce(ctx));
	else if ((s = firefly_resolve_frame(ctx, name, ctx->firefly.support, true, nullptr))) return s;
	else robust->resolved = (const float4 *)ctx->firefly_resolved;
	return noise_estimate_images(ctx, name, (const float4 *)ctx->aov_buffers[RT_AOV_RADIANCE][1], (const float4 *)ctx->noise_moments, floor, out, cell_sums, cell_counts, cell_nonfinite,
	                             cell_capacity, pixel_map, robust);
}

int rt_estimate_noise(rt_context * ctx, float floor, rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite, size_t cell_capacity, float * pixel_map) {
	RT_REQUIRE(ctx, ctx, "rt_estimate_noise: NULL context");
	RT_REQUIRE(ctx, out && cell_sums && cell_counts && cell_nonfinite, "rt_estimate_noise: NULL argument");
	return estimate_noise_frame(ctx, "rt_estimate_noise", floor, out, cell_sums, cell_counts, cell_nonfinite, cell_capacity, pixel_map, nullptr);
}

// ---- firefly-robust estimate -----------------------------------------------------------------------

int rt_estimate_noise_robust(rt_context * ctx, float floor, float held_fraction, rt_noise_estimate * out, double * cell_sums, int32_t * cell_counts, int32_t * cell_nonfinite,
                             int32_t * cell_held, size_t cell_capacity, float * pixel_map, int64_t * out_held_pixels) {
	RT_REQUIRE(ctx, ctx, "rt_estimate_noise_robust: NULL context");
	RT_REQUIRE(ctx, out && cell_sums && cell_counts && cell_nonfinite && cell_held, "rt_estimate_noise_robust: NULL argument");
	NoiseRobust robust = { nullptr, held_fraction, cell_held, out_held_pixels };
	return estimate_noise_frame(ctx, "rt_estimate_noise_robust", floor, out, cell_sums, cell_counts, cell_nonfinite, cell_capacity, pixel_map, &robust);
}

int rt_set_noise_robust(rt_context * ctx, float held_fraction) {
	RT_REQUIRE(ctx, ctx, "rt_set_noise_robust: NULL context");
	if (held_fraction == 0.0f) { ctx->noise_robust = 0.0f; return RT_OK; }
	int s = held_fraction_argument(ctx, "rt_set_noise_robust", held_fraction); if (s) return s;
	if (!ctx->firefly_on) return fail(ctx, RT_ERROR_NOT_READY, "rt_set_noise_robust: the firefly cascade is off (rt_set_firefly_cascade): the robust estimate follows its resolve");
	ctx->noise_robust = held_fraction;
	return RT_OK;
}
float rt_get_noise_robust(const rt_context * ctx) { return ctx ? ctx->noise_robust : 0.0f; }

// ---- adaptive sampling ------------------------------------------------------------------------------

int rt_select_active_cells(rt_context * ctx, float floor, float threshold, int dilate, rt_cell_selection * out, uint8_t * cell_flags, size_t cell_capacity) {
	RT_REQUIRE(ctx, ctx, "rt_select_active_cells: NULL context");
	RT_REQUIRE(ctx, out, "rt_select_active_cells: NULL argument");
	int s = selection_arguments(ctx, "rt_select_active_cells", floor, threshold, dilate); if (s) return s;
	(void)hipSetDevice(ctx->device);
	if (!ctx->noise_moments || !ctx->aov_buffers[RT_AOV_RADIANCE][1]) return fail(ctx, RT_ERROR_NOT_READY, "rt_select_active_cells: the noise estimate is off (rt_set_noise_estimate) or rt_resize was not called");
	if (const char * why = pixel_list_obstacle(ctx)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_select_active_cells: %s", why);
	RT_HIP(ctx, quiesce(ctx));   // from here on no submission reads the list: the new one may replace it
	const bool robust_on = ctx->noise_robust > 0.0f;   // (rt_set_noise_robust: the cells of rt_estimate_noise_robust, after a resolve of their own)
	if (robust_on && (s = firefly_resolve_frame(ctx, "rt_select_active_cells", ctx->firefly.support, true, nullptr))) return s;
	const NoiseRobust robust = { (const float4 *)ctx->firefly_resolved, ctx->noise_robust, nullptr, nullptr };
	if (!ctx->pixel_list) { s = device_alloc(ctx, &ctx->pixel_list, ctx->frame_pixels * 4); if (s) return s; }
	const bool was_on = ctx->pixel_list_on;
	pixel_list_drop(ctx);
	s = select_cells_images(ctx, "rt_select_active_cells", (const float4 *)ctx->aov_buffers[RT_AOV_RADIANCE][1], (const float4 *)ctx->noise_moments, floor, threshold, dilate,
	                        (unsigned *)ctx->pixel_list, out, nullptr, nullptr, nullptr, cell_flags, cell_capacity, robust_on ? &robust : nullptr);
	if (s) return s;
	ctx->pixel_list_selected = true; ctx->pixel_list_count = int(out->list_pixels);
	ctx->pixel_list_on = was_on && ctx->pixel_list_count > 0;   // (render calls that were covering the list go on with the new one; an empty list covers nothing and switches it off)
	return RT_OK;
}

int rt_set_pixel_list(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_pixel_list: NULL context");
	RT_REQUIRE(ctx, enable == 0 || enable == 1, "rt_set_pixel_list: enable must be 0 or 1");
	(void)hipSetDevice(ctx->device);
	if (enable) {
		if (!ctx->pixel_list_selected || !ctx->pixel_list) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_pixel_list: no selection exists (rt_select_active_cells)");
		if (ctx->pixel_list_count <= 0) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_pixel_list: the selected list is empty");
		// (a pixel range or a tile split needs no check of its own: setting either zeroes the moments, which drops the selection, and none can be made under them)
		if (ctx->params.config.enable_svgf) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_pixel_list: SVGF is on");
	}
	if ((enable != 0) != ctx->pixel_list_on) RT_HIP(ctx, quiesce(ctx));
	ctx->pixel_list_on = enable != 0;
	return RT_OK;
}
int rt_get_pixel_list(const rt_context * ctx) { return ctx && ctx->pixel_list_on ? 1 : 0; }

int rt_read_pixel_list(rt_context * ctx, uint32_t * dst, size_t capacity, size_t * out_count) {
	RT_REQUIRE(ctx, ctx, "rt_read_pixel_list: NULL context");
	RT_REQUIRE(ctx, out_count, "rt_read_pixel_list: NULL argument");
	(void)hipSetDevice(ctx->device);
	if (!ctx->pixel_list_selected || !ctx->pixel_list) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_pixel_list: no selection exists (rt_select_active_cells)");
	*out_count = size_t(ctx->pixel_list_count);
	if (!dst) return RT_OK;
	if (capacity < size_t(ctx->pixel_list_count)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_pixel_list: capacity %zu is below the %d entries of the list", capacity, ctx->pixel_list_count);
	RT_HIP(ctx, quiesce(ctx));
	if (ctx->pixel_list_count > 0) RT_HIP(ctx, hipMemcpy(dst, ctx->pixel_list, size_t(ctx->pixel_list_count) * 4, hipMemcpyDeviceToHost));
	return RT_OK;
}

} // extern "C"
