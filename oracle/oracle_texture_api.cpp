// oracle/oracle_texture_api.cpp -- TEST INFRASTRUCTURE ONLY.
// C entry points to the software texture unit of the oracle (oracle_shading.h), so that the
// reference's device code running on the CPU (oracle/ref/ref_cuda_harness.cpp) filters textures by the same rules
// as the oracle and the HIP kernels: the NVIDIA texture unit is the one part of the reference's device path that
// has no definition to restate.
#include "oracle_shading.h"
#include <cstring>

extern "C" {

void oracle_tex2d(const oracle_texture * tex, float s, float t, float out[4]) {
	float4 c = texture_get(*tex, s, t);
	out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
}
void oracle_tex2d_lod(const oracle_texture * tex, float s, float t, float lod, float out[4]) {
	float4 c = texture_get_lod(*tex, s, t, lod);
	out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
}
void oracle_tex2d_grad(const oracle_texture * tex, float s, float t, const float dx[2], const float dy[2], float out[4]) {
	float4 c = texture_get_grad(*tex, s, t, make_float2(dx[0], dx[1]), make_float2(dy[0], dy[1]));
	out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
}
float oracle_lut_1d(const float * lut, int nx, float s) { return lut_get_1d(lut, nx, s); }
float oracle_lut_2d(const float * lut, int nx, int ny, float s, float t) { return lut_get_2d(lut, nx, ny, s, t); }
float oracle_lut_3d(const float * lut, int nx, int ny, int nz, float s, float t, float r) { return lut_get_3d(lut, nx, ny, nz, s, t, r); }

// Clamp-addressed bilinear fetch of a float4 image at normalised coordinates (the sky: Sky.h:15)
void oracle_image_bilinear_clamp(const float * rgba, int width, int height, float u, float v, float out[4]) {
	int x0, x1, y0, y1; float fx, fy;
	clamp_taps(u, width, x0, x1, fx); clamp_taps(v, height, y0, y1, fy);
	auto texel = [&](int x, int y) { const float * p = rgba + (size_t(x) + size_t(y) * width) * 4; return make_float4(p[0], p[1], p[2], p[3]); };
	float4 c = lerp4(lerp4(texel(x0, y0), texel(x1, y0), fx), lerp4(texel(x0, y1), texel(x1, y1), fx), fy);
	out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
}

// Batches of the above for the tests (one call per array instead of one per probe). args: 8 floats per probe
// {s, t, lod, dx.x, dx.y, dy.x, dy.y, pad}; filter 0 = oracle_tex2d, 1 = oracle_tex2d_lod, 2 = oracle_tex2d_grad.
void oracle_tex2d_batch(const oracle_texture * tex, int filter, const float * args, size_t count, float * out_rgba) {
	for (size_t i = 0; i < count; i++) {
		const float * a = args + 8 * i;
		if (filter == 0) oracle_tex2d(tex, a[0], a[1], out_rgba + 4 * i);
		else if (filter == 1) oracle_tex2d_lod(tex, a[0], a[1], a[2], out_rgba + 4 * i);
		else oracle_tex2d_grad(tex, a[0], a[1], a + 3, a + 5, out_rgba + 4 * i);
	}
}
// coords: 3 floats per probe {s, t, r}; dims 1, 2, 3 = oracle_lut_1d / _2d / _3d
void oracle_lut_batch(const float * lut, int nx, int ny, int nz, int dims, const float * coords, size_t count, float * out) {
	for (size_t i = 0; i < count; i++) {
		const float * c = coords + 3 * i;
		out[i] = dims == 1 ? oracle_lut_1d(lut, nx, c[0]) : dims == 2 ? oracle_lut_2d(lut, nx, ny, c[0], c[1]) : oracle_lut_3d(lut, nx, ny, nz, c[0], c[1], c[2]);
	}
}

// sample_sky (Sky.h:7-16) on an equirect float4 image, through the oracle's own function: a scene holding only the sky
void oracle_sample_sky(const float * rgba, int width, int height, float scale, const float direction[3], float out[3]) {
	oracle_scene scene;
	memset(&scene, 0, sizeof(scene));
	scene.sky = rgba; scene.sky_width = width; scene.sky_height = height; scene.sky_scale = scale;
	float3 c = sample_sky(scene, make_float3(direction[0], direction[1], direction[2]));
	out[0] = c.x; out[1] = c.y; out[2] = c.z;
}

void oracle_sample_sky_batch(const float * rgba, int width, int height, float scale, const float * directions, size_t count, float * out_rgb) {
	for (size_t i = 0; i < count; i++) oracle_sample_sky(rgba, width, height, scale, directions + 3 * i, out_rgb + 3 * i);
}

} // extern "C"
