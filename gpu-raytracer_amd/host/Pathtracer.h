// Wavefront path tracing integrator, host side (reference: Src/Renderer/Integrators/
// Pathtracer.h:146-267, Pathtracer.cpp). The launch loop itself lives behind
// rt_render_sample(); this class packs materials/media, builds the light CDFs and keeps
// the reference's update()/render() protocol.
#pragma once
#include "Integrator.h"

// The noise estimate of a frame: per cell of 16 x 16 pixels the sum of the pixels' relative standard error e_p, their number and the number of
// non-finite pixels, as rt_estimate_noise returns them; `mean` is e_p's mean over the frame and `figure` the cpu_config.noise_quantile quantile of the cells'
// means (cells with a count above 0, nearest rank) -- what a noise target is compared with.
struct NoiseEstimate {
	int cells_x = 0, cells_y = 0;
	std::vector<double> cell_sums; std::vector<int32_t> cell_counts, cell_nonfinite;
	long long pixels = 0, nonfinite_pixels = 0;
	double mean = 0.0, figure = 0.0;
	// The firefly-robust estimate (cpu_config.noise_robust): the pixels the resolve holds back are left out of sums and counts and counted here
	bool robust = false;
	std::vector<int32_t> cell_held; long long held_pixels = 0;
};
// mean and figure from cell arrays, for C++ and Python alike. The mean: the sums added in cell order over the counts' total. The figure: the means sum / count of
// the cells with count > 0, sorted; entry ceil(quantile * m) of the m (1-based, at least 1). 0: fine; 1: no cell has a count (both 0); -1: quantile outside (0, 1].
extern "C" int grt_noise_summary(const double * cell_sums, const int32_t * cell_counts, size_t cells, double quantile, double * out_mean, double * out_figure, long long * out_pixels);
// The firefly cascade's start from the exposure histogram of rt_measure_exposure: 2^(median exponent + shift), the exponent clamped to
// -96 .. 96. 0: fine; 1: the histogram is empty, nothing is written. Either result may be NULL.
extern "C" int grt_exposure_start(const uint64_t * histogram256, int shift, float * out_start, int * out_median_exponent);

// What Pathtracer::select_adaptive chose: of `cells` cells, the hot ones (mean error above the threshold, or pixels not judged yet), the active
// ones (hot, or beside a hot one under cpu_config.adaptive_dilate) and the pixels of the active cells -- what the next render calls cover.
struct AdaptiveSelection { long long cells = 0, hot_cells = 0, active_cells = 0, list_pixels = 0; };

struct Pathtracer final : Integrator {
	// Light sampling tables (reference: Pathtracer.cpp:384-534)
	std::vector<int>   light_triangle_indices;
	std::vector<float> light_triangle_cumulative_probability;
	std::vector<float> light_mesh_cumulative_probability;
	std::vector<int>   light_mesh_triangle_span;      // {first, last} per light mesh
	std::vector<int>   light_mesh_transform_indices;  // TLAS-order mesh id per light mesh
	float              lights_total_weight = 0.0f;
	// Delta emitters: scene.delta_lights as rt_upload_delta_lights takes them, and the share that goes with them
	std::vector<rt_delta_light> delta_light_records;
	float              delta_light_share = 0.0f;
	// Fog volume: scene.fog reaches the device at update() when it has changed (the call drains what is in flight)
	bool               invalidated_fog = true;
	bool               fog_on_device = false; rt_fog_volume fog_record_on_device = { };
	bool               fog_density_on_device = false; std::vector<float> fog_density_values_on_device; int fog_density_dims_on_device[3] = { 0, 0, 0 };   // 
	bool               invalidated_delta_lights = true;   // scene.delta_lights or cpu_config.delta_light_share changed
	bool               delta_lights_uploaded = false, warned_delta_lights_without_nee = false;
	std::vector<rt_delta_light> delta_lights_on_device; float delta_light_share_on_device = 0.0f;   // what the device holds (an unchanged table is not uploaded again: the upload drains)

	// The SVGFData pair last handed to the device (reference: Pathtracer.cpp:707-717)
	std::vector<float> svgf_matrices = std::vector<float>(32, 0.0f);

	Pathtracer(int width, int height, Scene & scene, int device_ordinal = 0) : Integrator(scene, device_ordinal) {
		gpu_init(width, height);
	}
	// Source compatibility with `Pathtracer(frame_buffer_handle, width, height, scene)` (Main.cpp:68)
	Pathtracer(unsigned /*frame_buffer_handle*/, int width, int height, Scene & scene) : Pathtracer(width, height, scene, 0) { }

	void gpu_init(int width, int height) override;
	void gpu_free() override;

	void resize_init(int width, int height) override;
	void resize_free() override;

	void update(float delta) override;
	void render() override;
	// `count` samples per pixel in one wavefront (rt_render_samples): the same image as calling
	// update(); render(); `count` times. sample_index ends on the last sample rendered, so the next
	// update() continues the progression where the reference's loop would be.
	void render_samples(int count);
	// The estimate of what has been accumulated so far (completes the work in flight). Needs the device estimate on: noise_estimate_wanted or
	// cpu_config.noise_target > 0 before the update() of sample 0. pixel_map: e_p per pixel at x + y * pitch, -1 where the pixel takes no part, -2 non-finite.
	// While cpu_config.noise_robust is in force (update() sets rt_set_noise_robust) this is rt_estimate_noise_robust -- a resolve, then the cells without the held
	// pixels, -3 in the map --, and select_adaptive selects from the same cells.
	// Throws when the estimate is off; a frame without a participating pixel (allow_empty) returns pixels == 0 instead of throwing.
	NoiseEstimate noise(std::vector<float> * pixel_map = nullptr, bool allow_empty = false);
	// Adaptive sampling: selects the cells whose mean error is above `threshold` (rt_select_active_cells with cpu_config.noise_floor and
	// adaptive_dilate) and switches the render calls over to their pixels (rt_set_pixel_list); an empty selection switches back to the whole frame. The pass
	// index goes on as before -- it is the random-number index; every pixel folds with its own count. Needs the estimate on and at least two samples past
	// sample 0. A restart of the progression (sample_index 0 at render time: camera, scene, config, resize) switches the list off by itself.
	AdaptiveSelection select_adaptive(float threshold);
	void adaptive_off();
	// Denoised stills: the accumulated frame through rt_denoise, pitch * height float4 (r, g, b, variance of the filtered luminance over albedo).
	// Needs the noise estimate and the ALBEDO, NORMAL and POSITION AOVs on -- cpu_config.denoise = 1 before the update() of sample 0 does all four -- and no SVGF.
	// params: null for the configuration's (denoise_defaults). Completes the work in flight and changes nothing a later render reads.
	static rt_denoise_params denoise_defaults();
	std::vector<float> denoise(const rt_denoise_params * params = nullptr);
	// The denoised image through the exporters save_image uses (ppm, exr by the file's extension); the AOV files save_image writes beside its image are not written
	void save_denoised_image(const std::string & filename, const rt_denoise_params * params = nullptr);
	// Firefly filter: the tier cascade through rt_resolve_fireflies, pitch * height float4 (r, g, b, luminance held back). Needs
	// cpu_config.firefly_filter = 1 before the update() of sample 0 (which switches on the noise estimate and the cascade) and no SVGF. support: kappa, 0 for the
	// configuration's. Completes the work in flight and changes nothing a later render reads.
	std::vector<float> resolve_fireflies(float support = 0.0f);
	// The start of the cascade in force: cpu_config.firefly_start, or under cpu_config.firefly_auto_start what was measured after the pilot samples
	// (DESIGN.md 7.10.1). The measured start survives restarts of the progression; a resize, a change of the scene or of a firefly key measures again.
	float firefly_start() const;
	bool noise_robust_allowed = true;               // false: a rank of a FrameSplit, whose tiers are not gathered -- update() keeps the plain estimate
	bool last_noise_robust = false; long long last_noise_held_pixels = 0; std::vector<int32_t> last_noise_cell_held;   // of the last noise()
	bool firefly_start_measured = false;            // the pilot of the current configuration has been rendered and measured
	int  firefly_median_exponent = 0;               // what it found (with the shift, clamped), when a start could be computed
	long long firefly_pilot_samples_discarded = 0;  // samples rendered and dropped by restarts after a measurement ("extra")
	// The resolved image through the exporters save_image uses (ppm, exr by the file's extension)
	void save_resolved_image(const std::string & filename, float support = 0.0f);
	// w per pixel (x + y * pitch; 0 in the padding) -- the number of samples the pixel's mean stands for -- and, returned, the mean of w over the frame's pixels.
	// w is one below the samples rendered for the pixel: sample 1 overwrites sample 0 (AOV.h:35-46). Reports of "samples per pixel" add the 1.
	double sample_counts(std::vector<float> * counts = nullptr);

	void calc_light_power();
	void geometry_was_rebuilt() override { if (scene.has_lights) calc_light_power(); }   // light_triangle_indices name device triangles
	void calc_light_mesh_weights();
	void calc_delta_lights();

private:
	void measure_firefly_start();   // before a sample is rendered
	bool firefly_pilot_pending() const;
	struct FireflyStartKey { int width, height, filter, automatic, tiers, shift, pilot; float start; } firefly_start_key = { };
	bool warned_firefly_start_empty = false, warned_noise_robust = false;

};
