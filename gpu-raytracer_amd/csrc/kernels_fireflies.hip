// kernels_fireflies.hip -- the firefly filter: tiered accumulation with a reweighted resolve, after Zirr, Hanika and Dachsbacher 2018. Two families:
//   kernel_accumulate_cascade<CLEAR, LIST>   the three moments accumulate kernels of kernels_post.hip (batch, merged group, group over a pixel list) with the
//                                            splat of every RADIANCE sample into the pixel's K tier images beside the fold
//   kernel_fireflies_resolve(_tiled)         (mean, moments, tiers) -> (R / N, luminance held back / N): every tier scaled by how well its 3 x 3 neighbourhood
//                                            supports it; tiled in LDS, or plain (the probe's cross-check)
// A unit of its own: no existing unit's code object moves. Same contract as the other image kernels: -ffp-contract=off, every operation a plain IEEE float32
// one in the order written (the divisions are IEEE divisions), so the float32 restatement of tests/firefly_reference.py gives the same bits.
#include "rt_shading.h"

#define RT_FIREFLY_BASE 8.0f
#ifndef RT_FIREFLY_ROWS
#define RT_FIREFLY_ROWS 8   // rows of pixels per workgroup (one wave each) of the tiled resolve
#endif

RT_DEV bool fireflies_finite3(float4 v) { return fabsf(v.x) < __builtin_huge_valf() && fabsf(v.y) < __builtin_huge_valf() && fabsf(v.z) < __builtin_huge_valf(); }
RT_DEV bool fireflies_finite4(float4 v) { return fireflies_finite3(v) && fabsf(v.w) < __builtin_huge_valf(); }

// ---- accumulate with the cascade ---------------------------------------------------------------------------------------

// accumulate_fold<true> of kernels_post.hip, restated (shared through a header it would have to be visible to that unit: see the note there): the same
// operations in the same order, so mean and moments are the plain kernels' bits.
RT_DEV f4 cascade_fold(f4 acc, f4 & m2, f4 fb, float n) {   // n > 0
	f4 d = fb - acc;
	f4 next = acc + d / n;
	if (n >= 2.0f) { f4 t = d * (fb - next); m2 = mk4(m2.x + t.x, m2.y + t.y, m2.z + t.z, n); }
	else m2 = mk4(0.0f, 0.0f, 0.0f, 1.0f);
	return next;
}
RT_DEV f4 cascade_fold_plain(f4 acc, f4 fb, float n) { f4 d = fb - acc; return acc + d / n; }   // accumulate_fold<false>

RT_DEV void cascade_add(float4 * tier, float weight, f4 fb) {
	const float4 s = *tier;
	*tier = make_float4(s.x + weight * fb.x, s.y + weight * fb.y, s.z + weight * fb.z, s.w + weight);
}
// One RADIANCE sample into the pixel's tiers: a read-modify-write of at most two of them. One thread owns the pixel for the whole launch, so no atomics.
// reset: the fold index is <= 1 -- the mean is about to hold this sample alone (where the moments become (0, 0, 0, 1)) --, and so are the tiers.
RT_DEV void cascade_splat(const RtFireflyTiers & t, int pixel_index, f4 fb, bool reset) {
	float4 * tiers = t.tiers + pixel_index;
	if (reset) for (int j = 0; j < t.count; j++) tiers[size_t(j) * t.plane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	const float l = luminance(fb.x, fb.y, fb.z);
	if (!(fabsf(l) < __builtin_huge_valf())) return;   // (a finite luminance has finite channels)
	float lo = t.start; int j = 0;
	while (l >= lo * RT_FIREFLY_BASE && j < t.count - 1) { lo *= RT_FIREFLY_BASE; j++; }
	if (j == t.count - 1 || l <= lo) { cascade_add(tiers + size_t(j) * t.plane, 1.0f, fb); return; }
	const float hi = lo * RT_FIREFLY_BASE;
	const float wl = fminf(fmaxf((lo / l - lo / hi) / (1.0f - lo / hi), 0.0f), 1.0f);
	cascade_add(tiers + size_t(j) * t.plane, wl, fb);
	cascade_add(tiers + size_t(j + 1) * t.plane, 1.0f - wl, fb);
}

// One AOV of one pixel over the launch's samples: aov_accumulate / aov_accumulate_group (LIST false: the fold index is the sample's, the accumulator is loaded
// at the first sample past sample 0) and aov_accumulate_list (LIST true: the fold index is the pixel's own, n at load) of kernels_post.hip in one text. CLEAR:
// the sample frames are cleared on the way (the merged forms). RADIANCE: moments and splat beside the mean.
template<bool RADIANCE, bool CLEAR, bool LIST>
RT_DEV f4 cascade_aov(const RtParams & p, const RtAccumulateGroup & g, int aov, int pixel_index, float n_list, float4 * moments, const RtFireflyTiers & tiers) {
	const RtAOV & a = p.aovs[aov];
	if (!a.framebuffer) return mk4(0.0f);
	f4 acc = mk4(0.0f), m2 = mk4(0.0f);
	bool loaded = false;
	if (LIST) { acc = mk4(a.accumulator[pixel_index]); if (RADIANCE) m2 = mk4(moments[pixel_index]); loaded = true; }
	float n = n_list;
	for (int k = 0; k < g.count; k++) {
		if (!LIST) n = float(g.first_sample[k]);
		float4 * frames = a.framebuffer + size_t(g.slot_base[k]) * p.frame_pixels;
		for (int s = 0; s < g.sample_count[k]; s++, n += 1.0f) {
			float4 * sample = frames + size_t(s) * p.frame_pixels + pixel_index;
			f4 fb = mk4(*sample);
			if (CLEAR) *sample = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			if (RADIANCE) cascade_splat(tiers, pixel_index, fb, n <= 1.0f);
			if (LIST || n > 0.0f) {
				if (!loaded) { acc = mk4(a.accumulator[pixel_index]); if (RADIANCE) m2 = mk4(moments[pixel_index]); }
				acc = RADIANCE ? cascade_fold(acc, m2, fb, n) : cascade_fold_plain(acc, fb, n);
			} else { acc = fb; if (RADIANCE) m2 = mk4(0.0f, 0.0f, 0.0f, 1.0f); }
			loaded = true;
		}
	}
	a.accumulator[pixel_index] = to_float4(acc);
	if (RADIANCE) moments[pixel_index] = to_float4(m2);
	return acc;
}

template<bool CLEAR, bool LIST>
__global__ void __launch_bounds__(256) kernel_accumulate_cascade(RtParams p, RtAccumulateGroup g, const unsigned * __restrict__ list, int pixel_offset, int pixel_count, float4 * moments,
                                                                 RtFireflyTiers tiers) {
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pixel_count; i += gridDim.x * blockDim.x) {
		int idx = LIST ? int(list[i]) : rt_map_pixel(p, i + pixel_offset);
		int x = idx % p.screen_width, y = idx / p.screen_width;
		int pixel_index = x + y * p.screen_pitch;
		float n = LIST ? moments[pixel_index].w + 1.0f : 0.0f;

		f4 colour = cascade_aov<true, CLEAR, LIST>(p, g, RT_AOV_RADIANCE, pixel_index, n, moments, tiers);
		cascade_aov<false, CLEAR, LIST>(p, g, RT_AOV_ALBEDO,   pixel_index, n, nullptr, tiers);
		cascade_aov<false, CLEAR, LIST>(p, g, RT_AOV_NORMAL,   pixel_index, n, nullptr, tiers);
		cascade_aov<false, CLEAR, LIST>(p, g, RT_AOV_POSITION, pixel_index, n, nullptr, tiers);

		if (!isfinite(colour.x + colour.y + colour.z)) colour = mk4(1000.0f, 0.0f, 1000.0f, 1.0f); // NaN guard, Pathtracer.cu:790-793
		p.final_image[pixel_index] = to_float4(colour);
	}
}

static int cascade_blocks(int pixel_count) {
	int blocks = (pixel_count + 255) / 256;
	return blocks > 4096 ? 4096 : blocks < 1 ? 1 : blocks;
}
void rt_launch_accumulate_cascade(const RtParams & p, float frames_accumulated, int pixel_offset, int pixel_count, hipStream_t stream, float4 * moments, const RtFireflyTiers & tiers) {
	RtAccumulateGroup one = { };   // the batch is one submission whose frames the caller clears
	one.count = 1; one.first_sample[0] = int(frames_accumulated); one.sample_count[0] = p.batch_samples;
	hipLaunchKernelGGL((kernel_accumulate_cascade<false, false>), dim3(cascade_blocks(pixel_count)), dim3(256), 0, stream, p, one, (const unsigned *)nullptr, pixel_offset, pixel_count, moments, tiers);
}
void rt_launch_accumulate_group_cascade(const RtParams & p, const RtAccumulateGroup & group, int pixel_offset, int pixel_count, hipStream_t stream, float4 * moments, const RtFireflyTiers & tiers) {
	hipLaunchKernelGGL((kernel_accumulate_cascade<true, false>), dim3(cascade_blocks(pixel_count)), dim3(256), 0, stream, p, group, (const unsigned *)nullptr, pixel_offset, pixel_count, moments, tiers);
}
void rt_launch_accumulate_group_list_cascade(const RtParams & p, const RtAccumulateGroup & group, const unsigned * list, int pixel_count, hipStream_t stream, float4 * moments, const RtFireflyTiers & tiers) {
	hipLaunchKernelGGL((kernel_accumulate_cascade<true, true>), dim3(cascade_blocks(pixel_count)), dim3(256), 0, stream, p, group, list, 0, pixel_count, moments, tiers);
}

// ---- resolve -------------------------------------------------------------------------------------------------------------

// A pixel's tiers into registers (tier j >= K reads as zeros) and whether it is valid: w >= 1, the mean finite, every tier finite. *n: its w.
RT_DEV bool fireflies_load(const RtFireflyResolveArgs & a, const RtFireflyResolveImages & im, int pixel_index, float4 (&s)[RT_FIREFLY_MAX_TIERS], float & n) {
	const float4 c = im.mean[pixel_index], m = im.moments[pixel_index];
	bool valid = m.w >= 1.0f && fireflies_finite3(c);
	#pragma unroll
	for (int j = 0; j < RT_FIREFLY_MAX_TIERS; j++) {
		s[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (j < a.tiers) { s[j] = im.tiers[size_t(j) * im.plane + pixel_index]; valid = valid && fireflies_finite4(s[j]); }
	}
	n = m.w;
	return valid;
}

RT_DEV void fireflies_flag(const RtFireflyResolveImages & im, bool valid) {   // (kernel_denoise_prepare's: one lane of a wave, and only while the flag reads 0)
	if (!im.any_valid) return;
	const unsigned long long mask = __ballot(valid);
	if (valid && int(lane_id()) == __ffsll((long long)mask) - 1 && __hip_atomic_load(im.any_valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
		__hip_atomic_store(im.any_valid, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// Plain: tiles of 64 x 4 pixels in XCD bands (denoise_tile_pixel of kernels_denoise.hip); every tap loads its pixel's mean, moments and tiers again.
__global__ void __launch_bounds__(256) kernel_fireflies_resolve(RtFireflyResolveArgs a, RtFireflyResolveImages im) {
	const unsigned tiles_x = (unsigned(a.width) + 63u) / 64u, tiles_y = (unsigned(a.height) + 3u) / 4u;
	const unsigned tiles = tiles_x * tiles_y, per_xcd = gridDim.x / 8u;
	const unsigned tile = (blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u;
	if (tile >= tiles) return;
	const int x = int(tile % tiles_x) * 64 + int(threadIdx.x), y = int(tile / tiles_x) * 4 + int(threadIdx.y);
	const bool has_pixel = x < a.width && y < a.height;
	float4 s[RT_FIREFLY_MAX_TIERS]; float n = 0.0f;
	const int pixel_index = x + y * a.pitch;
	const bool valid = has_pixel && fireflies_load(a, im, pixel_index, s, n);
	fireflies_flag(im, valid);
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
// bytes read twice. Tiles are numbered row-major and XCD k takes the k-th eighth of the sequence (post_tile_pixel of kernels_post.hip has the reasons). Same arithmetic
// per pixel (fireflies_resolve_pixel) on the same W: bit-identical to the plain kernel.
template<int TY>
__global__ void __launch_bounds__(64 * TY) kernel_fireflies_resolve_tiled(RtFireflyResolveArgs a, RtFireflyResolveImages im) {
	constexpr int W = 64 + 2, ROWS = TY + 2, N = W * ROWS, RING = 2 * W + 2 * TY;
	static_assert(RING <= 64 * TY, "one ring position per thread");
	__shared__ float tile_w[RT_FIREFLY_MAX_TIERS][N];
	const unsigned tiles_x = (unsigned(a.width) + 63u) / 64u, tiles_y = (unsigned(a.height) + unsigned(TY) - 1u) / unsigned(TY);
	const unsigned tiles = tiles_x * tiles_y, per_xcd = gridDim.x / 8u;
	const unsigned tile = (blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u;
	if (tile >= tiles) return;   // (the whole workgroup: no barrier is left waiting)
	const int x0 = int(tile % tiles_x) * 64, y0 = int(tile / tiles_x) * TY;
	const int tx = int(threadIdx.x) & 63, ty = int(threadIdx.x) >> 6;
	const int x = x0 + tx, y = y0 + ty;
	const bool has_pixel = x < a.width && y < a.height;
	const int pixel_index = x + y * a.pitch, centre = (ty + 1) * W + tx + 1;

	float4 s[RT_FIREFLY_MAX_TIERS]; float n = 0.0f;
	const bool valid = has_pixel && fireflies_load(a, im, pixel_index, s, n);
	fireflies_flag(im, valid);
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

void rt_launch_fireflies_resolve(const RtFireflyResolveArgs & a, const RtFireflyResolveImages & im, bool tiled, hipStream_t stream) {
	const unsigned tiles_x = (unsigned(a.width) + 63u) / 64u;
	if (tiled) {
		const unsigned tiles = tiles_x * ((unsigned(a.height) + unsigned(RT_FIREFLY_ROWS) - 1u) / unsigned(RT_FIREFLY_ROWS));
		hipLaunchKernelGGL(kernel_fireflies_resolve_tiled<RT_FIREFLY_ROWS>, dim3((tiles + 7) / 8 * 8), dim3(64 * RT_FIREFLY_ROWS), 0, stream, a, im);
	} else {
		const unsigned tiles = tiles_x * ((unsigned(a.height) + 3u) / 4u);
		hipLaunchKernelGGL(kernel_fireflies_resolve, dim3((tiles + 7) / 8 * 8), dim3(64, 4), 0, stream, a, im);
	}
}
