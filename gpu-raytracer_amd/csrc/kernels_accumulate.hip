// kernels_accumulate.hip -- the accumulate step: the frames of finished samples folded into the running mean of RADIANCE, ALBEDO, NORMAL and POSITION, with or
// without RADIANCE's second moments and its firefly tiers (7.10), over a pixel range or a pixel list (7.6). Replaces kernel_accumulate
// (CUDA/Pathtracer.cu:775-796). ONE text -- fold, splat, per-AOV loop, pixel loop -- and one kernel per combination somebody launches.
// Plain streams of 48 B per pixel and AOV: one thread per pixel, 16-byte loads and stores. -ffp-contract=off: every operation is a plain IEEE float32 one in the
// order written (the divisions are IEEE divisions), so tests/noise_reference.py and tests/firefly_reference.py give the same bits.
#include "rt_shading.h"

// One sample folded into the running mean, AOV.h:35-46: sample 0 sets the mean and sample 1 overwrites it (fb - acc over n = 1), the quirk every
// comparison with the reference rests on. MOMENTS: Welford's second moment beside it, from the values the mean's own fold has just
// computed -- d = fb - acc_old and acc_new -- in plain float32 -, /, *, +: m2 = (M2_r, M2_g, M2_b, w), w the number of samples the moment stands for.
// Samples 0 and 1 leave (0, 0, 0, 1): after either the mean holds one sample alone.
template<bool MOMENTS> RT_DEV f4 accumulate_fold(f4 acc, f4 & m2, f4 fb, float n) {   // n > 0
	f4 d = fb - acc;
	f4 next = acc + d / n;
	if (MOMENTS) {
		if (n >= 2.0f) { f4 t = d * (fb - next); m2 = mk4(m2.x + t.x, m2.y + t.y, m2.z + t.z, n); }
		else m2 = mk4(0.0f, 0.0f, 0.0f, 1.0f);
	}
	return next;
}

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

// One AOV of one pixel over the launch's samples: the submissions of the group one after the other, a submission's samples one after the other, exactly as
// separate launches would fold them, with the accumulator kept in registers in between.
//   LIST false  the fold index is the sample's (first_sample of its submission, counted on); the accumulator is loaded at the first sample past sample 0
//   LIST true   the fold index is the PIXEL'S OWN (rt_set_pixel_list): n_list = w + 1 at load, w the number of samples its moments stand for, then n + 1 for every
//               further sample; first_sample does not enter. w = 0 (never sampled) gives n = 1: the mean takes the sample, the moments become (0, 0, 0, 1)
//   CLEAR       the sample frames are cleared on the way (aovs_clear_to_zero: only the pixels this context renders were ever written, a memset of the whole
//               frames moved 8x the bytes on a 1/8 split). Without it the launch is a batch: ONE submission at slot 0 whose frames the caller clears
//   MOMENTS / CASCADE   second moments / splat into the tiers beside the mean (RADIANCE only)
template<bool MOMENTS, bool CASCADE, bool CLEAR, bool LIST>
RT_DEV f4 accumulate_aov(const RtParams & p, const RtAccumulate & a, int aov, int pixel_index, float n_list) {
	const RtAOV & v = p.aovs[aov];
	if (!v.framebuffer) return mk4(0.0f);
	f4 acc = mk4(0.0f), m2 = mk4(0.0f);
	bool loaded = false;
	if (LIST) { acc = mk4(v.accumulator[pixel_index]); if (MOMENTS) m2 = mk4(a.moments[pixel_index]); loaded = true; }
	float n = n_list;
	const int submissions = CLEAR ? a.group.count : 1;
	for (int k = 0; k < submissions; k++) {
		if (!LIST) n = float(a.group.first_sample[k]);
		float4 * frames = v.framebuffer + size_t(CLEAR ? a.group.slot_base[k] : 0) * p.frame_pixels;
		const int samples = a.group.sample_count[k];
		for (int s = 0; s < samples; s++, n += 1.0f) {
			float4 * sample = frames + size_t(s) * p.frame_pixels + pixel_index;
			f4 fb = mk4(*sample);
			if (CLEAR) *sample = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			if (CASCADE) cascade_splat(a.tiers, pixel_index, fb, n <= 1.0f);
			if (LIST || n > 0.0f) {
				if (!loaded) { acc = mk4(v.accumulator[pixel_index]); if (MOMENTS) m2 = mk4(a.moments[pixel_index]); }
				acc = accumulate_fold<MOMENTS>(acc, m2, fb, n);
			} else { acc = fb; if (MOMENTS) m2 = mk4(0.0f, 0.0f, 0.0f, 1.0f); }
			loaded = true;
		}
	}
	v.accumulator[pixel_index] = to_float4(acc);
	if (MOMENTS) a.moments[pixel_index] = to_float4(m2);
	return acc;
}

// The pixel loop; `first` and `stride` are the thread's index in the grid and the grid's size. (The kernels form them themselves: read in this function, blockDim
// compiled without the kernel's promise of uniform workgroups -- a select between two implicit arguments and a vector load at the top of every wave, where the
// kernel's own read is one scalar load -- and every launch took 0.4 .. 0.8 us longer.)
template<bool MOMENTS, bool CASCADE, bool CLEAR, bool LIST>
RT_DEV void accumulate_pixels(const RtParams & p, const RtAccumulate & a, int first, int stride) {
	for (int i = first; i < a.pixel_count; i += stride) {
		int idx = LIST ? int(a.list[i]) : rt_map_pixel(p, i + a.pixel_offset);
		int x = idx % p.screen_width, y = idx / p.screen_width;
		int pixel_index = x + y * p.screen_pitch;
		float n = LIST ? a.moments[pixel_index].w + 1.0f : 0.0f;

		f4 colour = accumulate_aov<MOMENTS, CASCADE, CLEAR, LIST>(p, a, RT_AOV_RADIANCE, pixel_index, n);
		accumulate_aov<false, false, CLEAR, LIST>(p, a, RT_AOV_ALBEDO,   pixel_index, n);
		accumulate_aov<false, false, CLEAR, LIST>(p, a, RT_AOV_NORMAL,   pixel_index, n);
		accumulate_aov<false, false, CLEAR, LIST>(p, a, RT_AOV_POSITION, pixel_index, n);

		if (!isfinite(colour.x + colour.y + colour.z)) colour = mk4(1000.0f, 0.0f, 1000.0f, 1.0f); // NaN guard, Pathtracer.cu:790-793
		p.final_image[pixel_index] = to_float4(colour);
	}
}

// The combinations somebody launches, in accumulate_kernel_for's order: the slots scheduler's batch and the merged wavefront's group, each without and with the
// moments; the group over a pixel list (its fold index is read from the moments); the three moments forms with the cascade.
#define RT_ACCUMULATE_KERNEL_LIST(X) \
	X(kernel_accumulate,                    false, false, false, false) \
	X(kernel_accumulate_moments,            true,  false, false, false) \
	X(kernel_accumulate_group,              false, false, true,  false) \
	X(kernel_accumulate_group_moments,      true,  false, true,  false) \
	X(kernel_accumulate_group_list_moments, true,  false, true,  true ) \
	X(kernel_accumulate_cascade,            true,  true,  false, false) \
	X(kernel_accumulate_group_cascade,      true,  true,  true,  false) \
	X(kernel_accumulate_group_list_cascade, true,  true,  true,  true )
#define RT_DEFINE_ACCUMULATE_KERNEL(NAME, MOMENTS, CASCADE, CLEAR, LIST) \
__global__ void __launch_bounds__(256) NAME(RtParams p, RtAccumulate a) { accumulate_pixels<MOMENTS, CASCADE, CLEAR, LIST>(p, a, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x); }
RT_ACCUMULATE_KERNEL_LIST(RT_DEFINE_ACCUMULATE_KERNEL)
#undef RT_DEFINE_ACCUMULATE_KERNEL

#define RT_ACCUMULATE_KERNEL_ENTRY(NAME, MOMENTS, CASCADE, CLEAR, LIST) NAME,
static void (* const accumulate_kernels[])(RtParams, RtAccumulate) = { RT_ACCUMULATE_KERNEL_LIST(RT_ACCUMULATE_KERNEL_ENTRY) };
#undef RT_ACCUMULATE_KERNEL_ENTRY
#undef RT_ACCUMULATE_KERNEL_LIST
// What rt_launch_accumulate launches. A list and the tiers each come with the moments, a list with a group (RtAccumulate).
static void (*accumulate_kernel_for(const RtAccumulate & a))(RtParams, RtAccumulate) {
	const int clear = a.clear ? 1 : 0, list = a.list ? 1 : 0;
	return accumulate_kernels[a.tiers.tiers ? 5 + clear + list : list ? 4 : clear * 2 + (a.moments ? 1 : 0)];
}
void rt_launch_accumulate(const RtParams & p, const RtAccumulate & a, hipStream_t stream) {
	int blocks = (a.pixel_count + 255) / 256;
	blocks = blocks > 4096 ? 4096 : blocks < 1 ? 1 : blocks;
	hipLaunchKernelGGL(accumulate_kernel_for(a), dim3(blocks), dim3(256), 0, stream, p, a);
}
