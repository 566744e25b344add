// kernels_fireflies.hip -- the resolve of the firefly filter and its exposure measurement (tiered accumulation with a reweighted resolve, after Zirr, Hanika and Dachsbacher
// 2018; the accumulate step of kernels_accumulate.hip splats every RADIANCE sample into the pixel's K tier images).
//   kernel_fireflies_resolve(_tiled)   (mean, moments, tiers) -> (R / N, luminance held back / N): every tier scaled by how well its 3 x 3 neighbourhood
//                                      supports it; tiled in LDS, or plain (the probe's cross-check)
//   kernel_exposure_histogram          (mean, moments) -> the histogram of the float32 exponents of the mean's luminance (the cascade's start
//                                      taken from the frame's own exposure); integer counts
// Same contract as the other image kernels: -ffp-contract=off, every operation a plain IEEE float32 one in the order written (the divisions are IEEE
// divisions), so the float32 restatement of tests/firefly_reference.py gives the same bits.
#include "rt_shading.h"

#ifndef RT_FIREFLY_ROWS
#define RT_FIREFLY_ROWS 8   // rows of pixels per workgroup (one wave each) of the tiled resolve
#endif

// A pixel's tiers into registers (tier j >= K reads as zeros) and whether it is valid: w >= 1, the mean finite, every tier finite. *n: its w.
RT_DEV bool fireflies_load(const RtFireflyResolveArgs & a, const RtFireflyResolveImages & im, int pixel_index, float4 (&s)[RT_FIREFLY_MAX_TIERS], float & n) {
	const float4 c = im.mean[pixel_index], m = im.moments[pixel_index];
	bool valid = m.w >= 1.0f && finite3(c);
	#pragma unroll
	for (int j = 0; j < RT_FIREFLY_MAX_TIERS; j++) {
		s[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (j < a.tiers) { s[j] = im.tiers[size_t(j) * im.plane + pixel_index]; valid = valid && finite4(s[j]); }
	}
	n = m.w;
	return valid;
}

// The resolve of one pixel, shared by the two kernels below. support(j, i, k): W_j of the pixel at (x + i, y + k), i, k in {-1, 0, 1}, and 0 where that pixel
// lies outside the image or is not valid (adding 0 leaves a sum's bits alone) -- from the images in one kernel, from the workgroup's LDS tile in the other.
template<typename Support>
RT_DEV void fireflies_resolve_pixel(const RtFireflyResolveArgs & a, const RtFireflyResolveImages & im, int pixel_index, bool valid, const float4 (&s)[RT_FIREFLY_MAX_TIERS], float n, Support support) {
	if (!valid) { const float4 fb = im.fallback[pixel_index]; im.out[pixel_index] = make_float4(fb.x, fb.y, fb.z, -1.0f); return; }
	float area[RT_FIREFLY_MAX_TIERS];
	#pragma unroll
	for (int j = 0; j < RT_FIREFLY_MAX_TIERS; j++) {
		area[j] = 0.0f;
		if (j < a.tiers) {
			#pragma unroll
			for (int k = -1; k <= 1; k++) {
				#pragma unroll
				for (int i = -1; i <= 1; i++) area[j] += support(j, i, k);
			}
		}
	}
	f3 kept = mk3(s[0].x, s[0].y, s[0].z), total = kept;   // r_0 = 1
	float b = a.start;
	const float span = a.support - 1.0f;
	#pragma unroll
	for (int j = 1; j < RT_FIREFLY_MAX_TIERS; j++) {
		if (j < a.tiers) {
			b *= RT_FIREFLY_BASE;
			const float count = (area[j - 1] + area[j]) + (j + 1 < RT_FIREFLY_MAX_TIERS ? area[j + 1] : 0.0f);   // (area[K] is 0)
			const float rc = fminf(fmaxf((count - 1.0f) / span, 0.0f), 1.0f);
			const float rcol = fminf(1.0f, luminance(kept.x, kept.y, kept.z) / b);
			const float r = fmaxf(rc, rcol);
			kept = mk3(kept.x + r * s[j].x, kept.y + r * s[j].y, kept.z + r * s[j].z);
			total = mk3(total.x + s[j].x, total.y + s[j].y, total.z + s[j].z);
		}
	}
	im.out[pixel_index] = make_float4(kept.x / n, kept.y / n, kept.z / n, luminance(total.x - kept.x, total.y - kept.y, total.z - kept.z) / n);
}

// Plain: tiles of 64 x 4 pixels in XCD bands (xcd_tile of rt_shading.h); every tap loads its pixel's mean, moments and tiers again.
__global__ void __launch_bounds__(256) kernel_fireflies_resolve(RtFireflyResolveArgs a, RtFireflyResolveImages im) {
	const unsigned tiles_x = (unsigned(a.width) + 63u) / 64u, tiles_y = (unsigned(a.height) + 3u) / 4u;
	const unsigned tiles = tiles_x * tiles_y, tile = xcd_tile();
	if (tile >= tiles) return;
	const int x = int(tile % tiles_x) * 64 + int(threadIdx.x), y = int(tile / tiles_x) * 4 + int(threadIdx.y);
	const bool has_pixel = x < a.width && y < a.height;
	float4 s[RT_FIREFLY_MAX_TIERS]; float n = 0.0f;
	const int pixel_index = x + y * a.pitch;
	const bool valid = has_pixel && fireflies_load(a, im, pixel_index, s, n);
	raise_any_valid(im.any_valid, valid);
	if (!has_pixel) return;
	float near[9][RT_FIREFLY_MAX_TIERS];
	#pragma unroll
	for (int t = 0; t < 9; t++) {
		const int qx = x + t % 3 - 1, qy = y + t / 3 - 1;
		float4 q[RT_FIREFLY_MAX_TIERS]; float qn;
		const bool q_valid = valid && qx >= 0 && qy >= 0 && qx < a.width && qy < a.height && fireflies_load(a, im, qx + qy * a.pitch, q, qn);   // (an invalid pixel resolves nothing)
		#pragma unroll
		for (int j = 0; j < RT_FIREFLY_MAX_TIERS; j++) near[t][j] = q_valid ? q[j].w : 0.0f;
	}
	fireflies_resolve_pixel(a, im, pixel_index, valid, s, n, [&](int j, int i, int k) { return near[(k + 1) * 3 + i + 1][j]; });
}

// Tiled: a workgroup resolves 64 x TY pixels, one wave per row. The W of every tier over the (64 + 2) x (TY + 2) halo is staged in LDS, tier-major (consecutive lanes
// on consecutive banks), at most 8 floats per position: 21.1 KB with TY = 8. A thread loads its own pixel's mean, moments and tiers with 16-byte loads, keeps the
// colours in registers and stages its W (0 when the pixel is not valid); the first 2 * 66 + 2 TY threads load one position of the ring around the tile each -- the only
// bytes read twice. Tiles are numbered row-major and XCD k takes the k-th eighth of the sequence (xcd_tile of rt_shading.h has the reasons). Same arithmetic
// per pixel (fireflies_resolve_pixel) on the same W: bit-identical to the plain kernel.
template<int TY>
__global__ void __launch_bounds__(64 * TY) kernel_fireflies_resolve_tiled(RtFireflyResolveArgs a, RtFireflyResolveImages im) {
	constexpr int W = 64 + 2, ROWS = TY + 2, N = W * ROWS, RING = 2 * W + 2 * TY;
	static_assert(RING <= 64 * TY, "one ring position per thread");
	__shared__ float tile_w[RT_FIREFLY_MAX_TIERS][N];
	const unsigned tiles_x = (unsigned(a.width) + 63u) / 64u, tiles_y = (unsigned(a.height) + unsigned(TY) - 1u) / unsigned(TY);
	const unsigned tiles = tiles_x * tiles_y, tile = xcd_tile();
	if (tile >= tiles) return;   // (the whole workgroup: no barrier is left waiting)
	const int x0 = int(tile % tiles_x) * 64, y0 = int(tile / tiles_x) * TY;
	const int tx = int(threadIdx.x) & 63, ty = int(threadIdx.x) >> 6;
	const int x = x0 + tx, y = y0 + ty;
	const bool has_pixel = x < a.width && y < a.height;
	const int pixel_index = x + y * a.pitch, centre = (ty + 1) * W + tx + 1;

	float4 s[RT_FIREFLY_MAX_TIERS]; float n = 0.0f;
	const bool valid = has_pixel && fireflies_load(a, im, pixel_index, s, n);
	raise_any_valid(im.any_valid, valid);
	#pragma unroll
	for (int j = 0; j < RT_FIREFLY_MAX_TIERS; j++) if (j < a.tiers) tile_w[j][centre] = valid ? s[j].w : 0.0f;
	if (int(threadIdx.x) < RING) {   // the ring: top row, bottom row, then the two columns row by row
		const int h = int(threadIdx.x);
		const int c = h < W ? h : h < 2 * W ? h - W : ((h - 2 * W) & 1) * (W - 1);
		const int r = h < W ? 0 : h < 2 * W ? ROWS - 1 : 1 + ((h - 2 * W) >> 1);
		const int qx = x0 - 1 + c, qy = y0 - 1 + r;
		float4 q[RT_FIREFLY_MAX_TIERS]; float qn;
		const bool q_valid = qx >= 0 && qy >= 0 && qx < a.width && qy < a.height && fireflies_load(a, im, qx + qy * a.pitch, q, qn);
		#pragma unroll
		for (int j = 0; j < RT_FIREFLY_MAX_TIERS; j++) if (j < a.tiers) tile_w[j][r * W + c] = q_valid ? q[j].w : 0.0f;
	}
	__syncthreads();

	if (!has_pixel) return;
	fireflies_resolve_pixel(a, im, pixel_index, valid, s, n, [&](int j, int i, int k) { return tile_w[j][centre + i + k * W]; });
}

// The exposure histogram (rt_measure_exposure): which power of two the frame's pixels are bright as, so that the cascade's start can follow the
// median class. A pixel with w >= 1 is non-finite when r, g, b or the luminance of its mean is not finite, dark when Y = luminance(mean) <= 0, and else counts in
// bin (bits(Y) >> 23) & 255, its biased exponent (denormals: bin 0). The padding columns are never read. Counts are integers, so the atomics decide nothing: a
// workgroup counts its pixels -- index i of the width x height frame, a stride of the whole grid apart -- in LDS and adds the bins it filled to the global words.
__global__ void __launch_bounds__(256) kernel_exposure_histogram(const float4 * __restrict__ mean, const float4 * __restrict__ moments, int width, int height, int pitch,
                                                                 unsigned long long * __restrict__ histogram) {
	__shared__ unsigned bins[RT_EXPOSURE_WORDS];
	for (int t = threadIdx.x; t < RT_EXPOSURE_WORDS; t += 256) bins[t] = 0u;
	__syncthreads();
	const unsigned pixels = unsigned(width) * unsigned(height);
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < pixels; i += gridDim.x * 256u) {
		const size_t pixel_index = size_t(i % unsigned(width)) + size_t(i / unsigned(width)) * size_t(pitch);
		if (!(moments[pixel_index].w >= 1.0f)) continue;
		const float4 c = mean[pixel_index];
		const float lum = luminance(c.x, c.y, c.z);
		int bin = RT_EXPOSURE_NONFINITE;
		if (finite3(c) && fabsf(lum) < __builtin_huge_valf()) bin = lum <= 0.0f ? RT_EXPOSURE_DARK : int((__float_as_uint(lum) >> 23) & 255u);
		atomicAdd(&bins[bin], 1u);
	}
	__syncthreads();
	for (int t = threadIdx.x; t < RT_EXPOSURE_WORDS; t += 256) if (bins[t]) atomicAdd(&histogram[t], (unsigned long long)bins[t]);
}

// At most 1024 workgroups (four to a compute unit): every one ends with an atomic per bin it filled, and atomics on one word retire one after the other.
void rt_launch_exposure_histogram(const float4 * mean, const float4 * moments, int width, int height, int pitch, unsigned long long * histogram, hipStream_t stream) {
	const unsigned pixels = unsigned(width) * unsigned(height);
	unsigned blocks = (pixels + 255u) / 256u;
	blocks = blocks > 1024u ? 1024u : blocks < 1u ? 1u : blocks;
	hipLaunchKernelGGL(kernel_exposure_histogram, dim3(blocks), dim3(256), 0, stream, mean, moments, width, height, pitch, histogram);
}

void rt_launch_fireflies_resolve(const RtFireflyResolveArgs & a, const RtFireflyResolveImages & im, bool tiled, hipStream_t stream) {
	const unsigned tiles_x = (unsigned(a.width) + 63u) / 64u;
	if (tiled) {
		const unsigned tiles = tiles_x * ((unsigned(a.height) + unsigned(RT_FIREFLY_ROWS) - 1u) / unsigned(RT_FIREFLY_ROWS));
		hipLaunchKernelGGL(kernel_fireflies_resolve_tiled<RT_FIREFLY_ROWS>, dim3(xcd_tile_grid(tiles)), dim3(64 * RT_FIREFLY_ROWS), 0, stream, a, im);
	} else {
		const unsigned tiles = tiles_x * ((unsigned(a.height) + 3u) / 4u);
		hipLaunchKernelGGL(kernel_fireflies_resolve, dim3(xcd_tile_grid(tiles)), dim3(64, 4), 0, stream, a, im);
	}
}
