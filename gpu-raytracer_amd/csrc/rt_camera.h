// rt_camera.h -- the primary ray of a pixel and sample (CUDA/Camera.h:20-62), for the generate kernels of kernels_generate.hip and kernels_list.hip.
#pragma once
#include "rt_shading.h"

// `taa_index`: the sample index that picks the TAA jitter (the merged wavefront passes a sample index shifted by the slot,
// which random_sample undoes).
RT_DEV void camera_generate_ray(const RtParams & p, int pixel_index, int sample_index, int x, int y, f3 & origin, f3 & direction, int taa_index) {
	f2 rand_filter   = random_sample(p, DIM_FILTER,   unsigned(pixel_index), 0, unsigned(sample_index));
	// (a pinhole camera -- aperture radius 0, uniform over the launch -- multiplies its lens sample by zero: the draw and the disk mapping are skipped, the ray is the same)
	const bool thin_lens = p.camera.aperture_radius != 0.0f;
	f2 rand_aperture = thin_lens ? random_sample(p, DIM_APERTURE, unsigned(pixel_index), 0, unsigned(sample_index)) : mk2(0.0f, 0.0f);

	f2 jitter;
	if (p.config.enable_svgf) {
		const float taa_halton_x[4] = { 0.3f, 0.7f, 0.2f, 0.8f };
		const float taa_halton_y[4] = { 0.2f, 0.8f, 0.7f, 0.3f };
		jitter.x = taa_halton_x[taa_index & 3];
		jitter.y = taa_halton_y[taa_index & 3];
	} else if (p.config.reconstruction_filter == RT_FILTER_BOX) {
		jitter = rand_filter;
	} else if (p.config.reconstruction_filter == RT_FILTER_TENT) {
		jitter.x = sample_tent(rand_filter.x);
		jitter.y = sample_tent(rand_filter.y);
	} else {
		f2 g = sample_gaussian(rand_filter.x, rand_filter.y);
		jitter.x = 0.5f + 0.5f * g.x;
		jitter.y = 0.5f + 0.5f * g.y;
	}
	float x_jittered = float(x) + jitter.x;
	float y_jittered = float(y) + jitter.y;

	f3 blc = mk3(p.camera.bottom_left_corner[0], p.camera.bottom_left_corner[1], p.camera.bottom_left_corner[2]);
	f3 xa  = mk3(p.camera.x_axis[0], p.camera.x_axis[1], p.camera.x_axis[2]);
	f3 ya  = mk3(p.camera.y_axis[0], p.camera.y_axis[1], p.camera.y_axis[2]);

	f3 focal_point = p.camera.focal_distance * normalize(blc + x_jittered * xa + y_jittered * ya);
	f2 lens_point  = thin_lens ? p.camera.aperture_radius * sample_disk(rand_aperture.x, rand_aperture.y) : mk2(0.0f, 0.0f);

	f3 offset = xa * lens_point.x + ya * lens_point.y;
	direction = normalize(focal_point - offset);
	origin = mk3(p.camera.position[0], p.camera.position[1], p.camera.position[2]) + offset;
}
