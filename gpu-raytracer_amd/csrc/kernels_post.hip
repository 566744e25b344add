// kernels_post.hip -- image-space kernels: the noise estimate, the adaptive-sampling cell selection, SVGF (reproject / variance / a-trous /
// finalize), TAA, plus the Kulla-Conty LUT integration kernels and a bandwidth probe. (The accumulate step is kernels_accumulate.hip.)
//
// Replaces the six kernels of CUDA/SVGF/{SVGF,TAA}.h and the four LUT kernels of CUDA/KullaConty.h:83-240.
// All of these stream pitch x height float4 images: HBM-bandwidth bound, so each thread
// handles one pixel with 16-byte loads/stores and consecutive lanes touch consecutive
// pixels (256 B per wave per access). CUDA surfaces become plain pitched arrays; reads the
// reference does with cudaBoundaryModeClamp are clamped index computations.
#include "rt_shading.h"

#define RT_POST_BLOCK_X 64
#define RT_POST_BLOCK_Y 4

// Pixel of this thread in the image-space kernels below (SVGF, TAA): tiles of 64 x 4 pixels, row-major, in XCD bands (xcd_tile of rt_shading.h has the
// reasons). Returns false for a padding workgroup.
RT_DEV bool post_tile_pixel(const RtParams & p, int & x, int & y) {
	const unsigned tiles_x = (unsigned(p.screen_pitch) + RT_POST_BLOCK_X - 1) / RT_POST_BLOCK_X;
	const unsigned tiles_y = (unsigned(p.screen_height) + RT_POST_BLOCK_Y - 1) / RT_POST_BLOCK_Y;
	const unsigned tiles = tiles_x * tiles_y, tile = xcd_tile();
	if (tile >= tiles) return false;
	x = int(tile % tiles_x) * RT_POST_BLOCK_X + int(threadIdx.x);
	y = int(tile / tiles_x) * RT_POST_BLOCK_Y + int(threadIdx.y);
	return true;
}

RT_DEV f4 ld4(const float4 * p, int i) { return mk4(p[i]); }
RT_DEV void st4(float4 * p, int i, f4 v) { p[i] = to_float4(v); }

// ---- noise estimate (rt_estimate_noise) ----------------------------------------------------------------
// One workgroup per cell of RT_NOISE_CELL x RT_NOISE_CELL pixels of the screen (not of the pitch: the padding columns are never read), edge cells
// clipped; thread t owns pixel (t % 16, t / 16) of the cell. A pixel takes part when w >= 2 and its mean and M2 are finite; with w >= 2 and anything
// not finite it is counted as non-finite and left out. Its error is the standard error of the mean's three channels over the mean's luminance
// (`luminance` of rt_shading.h, floored), in float32 in exactly this shape:
//   v = (M2_r + M2_g) + M2_b;  e_p = sqrtf(v / (w * (w - 1.0f))) / fmaxf(luminance(mean), floor)
// The cell's sum of e_p (double), its participating and its non-finite pixels are reduced by a fixed tree in LDS -- s[t] += s[t + stride], stride
// 128 .. 1 -- without atomics: the same bits on every run and every rank, as the sky tables' scans are.
//
// ROBUST (rt_estimate_noise_robust) is the same text beside the resolved image of the firefly filter: a pixel that takes part by the rule above is
// HELD when the resolve found it valid (resolved.w >= 0) and held back more than held_fraction of its brightness, in float32
//   resolved.w > held_fraction * fmaxf(luminance(mean), floor)
// A held pixel is left out of sum and count, counted in cell_held, and -3 in the map. With no held pixel in a cell its three results are the plain kernel's bits.
template<bool ROBUST>
RT_DEV void noise_cells(const float4 * __restrict__ mean, const float4 * __restrict__ moments, const float4 * __restrict__ resolved, int width, int height, int pitch,
                        int cells_x, float floor, float held_fraction, float * __restrict__ pixel_map,
                        double * __restrict__ cell_sums, int * __restrict__ cell_counts, int * __restrict__ cell_nonfinite, int * __restrict__ cell_held) {
	__shared__ double sums[RT_NOISE_CELL * RT_NOISE_CELL];
	__shared__ int counts[RT_NOISE_CELL * RT_NOISE_CELL], nonfinite[RT_NOISE_CELL * RT_NOISE_CELL], held[ROBUST ? RT_NOISE_CELL * RT_NOISE_CELL : 1];
	const int t = threadIdx.x;
	const int x = int(blockIdx.x % unsigned(cells_x)) * RT_NOISE_CELL + t % RT_NOISE_CELL;
	const int y = int(blockIdx.x / unsigned(cells_x)) * RT_NOISE_CELL + t / RT_NOISE_CELL;
	double sum = 0.0; int count = 0, bad = 0, back = 0;
	if (x < width && y < height) {
		const size_t pixel_index = size_t(x) + size_t(y) * pitch;
		const float4 m = moments[pixel_index];
		float e = -1.0f;
		if (m.w >= 2.0f) {
			const float4 c = mean[pixel_index];
			if (isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(m.x) && isfinite(m.y) && isfinite(m.z)) {
				float v = (m.x + m.y) + m.z;
				e = sqrtf(v / (m.w * (m.w - 1.0f))) / fmaxf(luminance(c.x, c.y, c.z), floor);
				sum = double(e); count = 1;
				if (ROBUST) {
					const float r = resolved[pixel_index].w;
					if (r >= 0.0f && r > held_fraction * fmaxf(luminance(c.x, c.y, c.z), floor)) { e = -3.0f; sum = 0.0; count = 0; back = 1; }
				}
			} else { e = -2.0f; bad = 1; }
		}
		if (pixel_map) pixel_map[pixel_index] = e;
	}
	sums[t] = sum; counts[t] = count; nonfinite[t] = bad;
	if (ROBUST) held[t] = back;
	__syncthreads();
	for (int stride = RT_NOISE_CELL * RT_NOISE_CELL / 2; stride >= 1; stride >>= 1) {
		if (t < stride) { sums[t] += sums[t + stride]; counts[t] += counts[t + stride]; nonfinite[t] += nonfinite[t + stride]; if (ROBUST) held[t] += held[t + stride]; }
		__syncthreads();
	}
	if (t == 0) { cell_sums[blockIdx.x] = sums[0]; cell_counts[blockIdx.x] = counts[0]; cell_nonfinite[blockIdx.x] = nonfinite[0]; if (ROBUST) cell_held[blockIdx.x] = held[0]; }
}
__global__ void __launch_bounds__(RT_NOISE_CELL * RT_NOISE_CELL) kernel_noise_cells(const float4 * __restrict__ mean, const float4 * __restrict__ moments, int width, int height, int pitch,
                                                                                    int cells_x, float floor, float * __restrict__ pixel_map,
                                                                                    double * __restrict__ cell_sums, int * __restrict__ cell_counts, int * __restrict__ cell_nonfinite) {
	noise_cells<false>(mean, moments, nullptr, width, height, pitch, cells_x, floor, 0.0f, pixel_map, cell_sums, cell_counts, cell_nonfinite, nullptr);
}
__global__ void __launch_bounds__(RT_NOISE_CELL * RT_NOISE_CELL) kernel_noise_cells_robust(const float4 * __restrict__ mean, const float4 * __restrict__ moments, const float4 * __restrict__ resolved,
                                                                                           int width, int height, int pitch, int cells_x, float floor, float held_fraction, float * __restrict__ pixel_map,
                                                                                           double * __restrict__ cell_sums, int * __restrict__ cell_counts, int * __restrict__ cell_nonfinite, int * __restrict__ cell_held) {
	noise_cells<true>(mean, moments, resolved, width, height, pitch, cells_x, floor, held_fraction, pixel_map, cell_sums, cell_counts, cell_nonfinite, cell_held);
}

void rt_launch_noise_cells(const float4 * mean, const float4 * moments, int width, int height, int pitch, float floor, float * pixel_map,
                           double * cell_sums, int * cell_counts, int * cell_nonfinite, hipStream_t stream) {
	const int cells_x = (width + RT_NOISE_CELL - 1) / RT_NOISE_CELL, cells_y = (height + RT_NOISE_CELL - 1) / RT_NOISE_CELL;
	hipLaunchKernelGGL(kernel_noise_cells, dim3(unsigned(cells_x) * unsigned(cells_y)), dim3(RT_NOISE_CELL * RT_NOISE_CELL), 0, stream,
	                   mean, moments, width, height, pitch, cells_x, floor, pixel_map, cell_sums, cell_counts, cell_nonfinite);
}
void rt_launch_noise_cells_robust(const float4 * mean, const float4 * moments, const float4 * resolved, int width, int height, int pitch, float floor, float held_fraction,
                                  float * pixel_map, double * cell_sums, int * cell_counts, int * cell_nonfinite, int * cell_held, hipStream_t stream) {
	const int cells_x = (width + RT_NOISE_CELL - 1) / RT_NOISE_CELL, cells_y = (height + RT_NOISE_CELL - 1) / RT_NOISE_CELL;
	hipLaunchKernelGGL(kernel_noise_cells_robust, dim3(unsigned(cells_x) * unsigned(cells_y)), dim3(RT_NOISE_CELL * RT_NOISE_CELL), 0, stream,
	                   mean, moments, resolved, width, height, pitch, cells_x, floor, held_fraction, pixel_map, cell_sums, cell_counts, cell_nonfinite, cell_held);
}

// ---- adaptive sampling: the cells still above the noise target, and their pixels as a list (rt_select_active_cells) ----------
// The in-frame pixels of cell (cx, cy): edge cells are clipped.
RT_DEV int cell_frame_pixels(int cx, int cy, int width, int height) {
	return min(RT_NOISE_CELL, width - cx * RT_NOISE_CELL) * min(RT_NOISE_CELL, height - cy * RT_NOISE_CELL);
}
// A cell is hot when its mean error is above the threshold -- compared in double, as sum > threshold * count, so that the host reproduces it from the
// cell arrays -- or when it has in-frame pixels that took no part without being non-finite (w < 2: not sampled enough to judge). A cell of non-finite
// pixels only is not hot: more samples do not repair a NaN mean.
// HELD (the robust cells): the pixels the firefly filter holds back count as judged too -- a cell of held and non-finite pixels only is not hot.
template<bool HELD>
RT_DEV bool cell_is_hot(const double * __restrict__ cell_sums, const int * __restrict__ cell_counts, const int * __restrict__ cell_nonfinite, const int * __restrict__ cell_held, int c, int frame_pixels, float threshold) {
	const int count = cell_counts[c];
	if (count > 0 && cell_sums[c] > double(threshold) * double(count)) return true;
	return count + cell_nonfinite[c] + (HELD ? cell_held[c] : 0) < frame_pixels;
}
// One thread per cell. flags: bit 0 hot, bit 1 active (hot, or with dilate = 1 one of the up to 8 neighbours inside the grid hot); active_pixels: the
// cell's in-frame pixels when it is active, else 0 -- what the scan below turns into list offsets.
template<bool HELD>
RT_DEV void select_cells(const double * __restrict__ cell_sums, const int * __restrict__ cell_counts, const int * __restrict__ cell_nonfinite, const int * __restrict__ cell_held,
                         int width, int height, int cells_x, int cells_y, float threshold, int dilate,
                         unsigned char * __restrict__ flags, int * __restrict__ active_pixels) {
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= cells_x * cells_y) return;
	const int cx = c % cells_x, cy = c / cells_x;
	const bool hot = cell_is_hot<HELD>(cell_sums, cell_counts, cell_nonfinite, cell_held, c, cell_frame_pixels(cx, cy, width, height), threshold);
	bool active = hot;
	if (dilate && !hot)
		for (int ny = max(cy - 1, 0); ny <= min(cy + 1, cells_y - 1); ny++) for (int nx = max(cx - 1, 0); nx <= min(cx + 1, cells_x - 1); nx++)
			if (cell_is_hot<HELD>(cell_sums, cell_counts, cell_nonfinite, cell_held, nx + ny * cells_x, cell_frame_pixels(nx, ny, width, height), threshold)) active = true;
	flags[c] = (unsigned char)((hot ? 1 : 0) | (active ? 2 : 0));
	active_pixels[c] = active ? cell_frame_pixels(cx, cy, width, height) : 0;
}
__global__ void __launch_bounds__(256) kernel_select_cells(const double * __restrict__ cell_sums, const int * __restrict__ cell_counts, const int * __restrict__ cell_nonfinite,
                                                           int width, int height, int cells_x, int cells_y, float threshold, int dilate,
                                                           unsigned char * __restrict__ flags, int * __restrict__ active_pixels) {
	select_cells<false>(cell_sums, cell_counts, cell_nonfinite, nullptr, width, height, cells_x, cells_y, threshold, dilate, flags, active_pixels);
}
__global__ void __launch_bounds__(256) kernel_select_cells_robust(const double * __restrict__ cell_sums, const int * __restrict__ cell_counts, const int * __restrict__ cell_nonfinite,
                                                                  const int * __restrict__ cell_held, int width, int height, int cells_x, int cells_y, float threshold, int dilate,
                                                                  unsigned char * __restrict__ flags, int * __restrict__ active_pixels) {
	select_cells<true>(cell_sums, cell_counts, cell_nonfinite, cell_held, width, height, cells_x, cells_y, threshold, dilate, flags, active_pixels);
}
// Exclusive prefix sum of active_pixels over the cells in ascending cell index, one workgroup: thread t adds up its run of consecutive cells, the 256 run
// totals are scanned in LDS (Hillis-Steele, integers), the run is walked again. totals: { list length, hot cells, active cells }. No atomics: the
// offsets, and with them the list, are the same on every run.
__global__ void __launch_bounds__(256) kernel_scan_cells(const int * __restrict__ active_pixels, const unsigned char * __restrict__ flags, int cells, int * __restrict__ offsets, int * __restrict__ totals) {
	__shared__ int pixels[256], hot[256], active[256];
	const int t = threadIdx.x;
	const int run = (cells + 255) / 256, begin = min(t * run, cells), end = min(begin + run, cells);
	int sum = 0, h = 0, a = 0;
	for (int c = begin; c < end; c++) { sum += active_pixels[c]; h += flags[c] & 1; a += (flags[c] >> 1) & 1; }
	pixels[t] = sum; hot[t] = h; active[t] = a;
	__syncthreads();
	for (int stride = 1; stride < 256; stride <<= 1) {
		int add = t >= stride ? pixels[t - stride] : 0;
		__syncthreads();
		pixels[t] += add;
		__syncthreads();
	}
	int at = pixels[t] - sum;   // exclusive
	for (int c = begin; c < end; c++) { offsets[c] = at; at += active_pixels[c]; }
	for (int stride = 128; stride >= 1; stride >>= 1) {
		if (t < stride) { hot[t] += hot[t + stride]; active[t] += active[t + stride]; }
		__syncthreads();
	}
	if (t == 0) { totals[0] = pixels[255]; totals[1] = hot[0]; totals[2] = active[0]; }
}
// One workgroup per cell; an active cell writes its in-frame pixels, x + y * width each, from offsets[cell] on. Thread t stands for the pixel that comes t-th in
// the cell's order: the four 8 x 8 patches (0,0), (8,0), (0,8), (8,8), a patch row by row -- 64 consecutive entries of an unclipped cell cover one patch, the
// queue order kernel_generate_stream uses for whole bands. In a clipped cell the pixels outside the frame are skipped and the list stays dense: a pixel's
// place is its rank among the in-frame threads, an inclusive scan of the 256 flags in LDS.
__global__ void __launch_bounds__(RT_NOISE_CELL * RT_NOISE_CELL) kernel_compact_cells(const unsigned char * __restrict__ flags, const int * __restrict__ offsets, int width, int height, int cells_x,
                                                                                      unsigned * __restrict__ list) {
	__shared__ int rank[RT_NOISE_CELL * RT_NOISE_CELL];
	const int cell = blockIdx.x;
	if (!(flags[cell] & 2)) return;   // (the whole workgroup)
	const int t = threadIdx.x;
	const int patch = t >> 6, in_patch = t & 63;
	const int x = (cell % cells_x) * RT_NOISE_CELL + (patch & 1) * 8 + (in_patch & 7);
	const int y = (cell / cells_x) * RT_NOISE_CELL + (patch >> 1) * 8 + (in_patch >> 3);
	const int inside = x < width && y < height ? 1 : 0;
	rank[t] = inside;
	__syncthreads();
	for (int stride = 1; stride < RT_NOISE_CELL * RT_NOISE_CELL; stride <<= 1) {
		int add = t >= stride ? rank[t - stride] : 0;
		__syncthreads();
		rank[t] += add;
		__syncthreads();
	}
	if (inside) list[offsets[cell] + rank[t] - 1] = unsigned(x) + unsigned(y) * unsigned(width);
}

void rt_launch_select_cells(const double * cell_sums, const int * cell_counts, const int * cell_nonfinite, int width, int height, float threshold, int dilate,
                            unsigned char * flags, int * active_pixels, int * offsets, int * totals, unsigned * list, hipStream_t stream, const int * cell_held) {
	const int cells_x = (width + RT_NOISE_CELL - 1) / RT_NOISE_CELL, cells_y = (height + RT_NOISE_CELL - 1) / RT_NOISE_CELL, cells = cells_x * cells_y;
	if (cell_held) hipLaunchKernelGGL(kernel_select_cells_robust, dim3((cells + 255) / 256), dim3(256), 0, stream, cell_sums, cell_counts, cell_nonfinite, cell_held, width, height, cells_x, cells_y, threshold, dilate, flags, active_pixels);
	else hipLaunchKernelGGL(kernel_select_cells, dim3((cells + 255) / 256), dim3(256), 0, stream, cell_sums, cell_counts, cell_nonfinite, width, height, cells_x, cells_y, threshold, dilate, flags, active_pixels);
	hipLaunchKernelGGL(kernel_scan_cells, dim3(1), dim3(256), 0, stream, active_pixels, flags, cells, offsets, totals);
	hipLaunchKernelGGL(kernel_compact_cells, dim3(cells), dim3(RT_NOISE_CELL * RT_NOISE_CELL), 0, stream, flags, offsets, width, height, cells_x, list);
}

// ---- SVGF ----------------------------------------------------------------------------------------

#define RT_SVGF_EPSILON 1e-8f
#define RT_FEEDBACK_ITERATION 1

RT_DEV f3 oct_decode_normal(f2 f) {
	f = mk2(f.x * 2.0f - 1.0f, f.y * 2.0f - 1.0f);
	f3 n = mk3(f.x, f.y, 1.0f - fabsf(f.x) - fabsf(f.y));
	float t = saturate(-n.z);
	n.x += n.x >= 0.0f ? -t : t;
	n.y += n.y >= 0.0f ? -t : t;
	return normalize(n);
}
RT_DEV f3 rgb_to_ycocg(f3 c) { return mk3(0.25f * c.x + 0.5f * c.y + 0.25f * c.z, 0.5f * c.x - 0.5f * c.z, -0.25f * c.x + 0.5f * c.y - 0.25f * c.z); }
RT_DEV f3 ycocg_to_rgb(f3 c) { return mk3(saturate(c.x + c.y - c.z), saturate(c.x + c.z), saturate(c.x - c.y - c.z)); }
RT_DEV float mitchell_netravali(float x) {
	const float B = 1.0f / 3.0f, C = 1.0f / 3.0f;
	x = fabsf(x);
	float x2 = x * x, x3 = x2 * x;
	if (x < 1.0f) return (1.0f / 6.0f) * ((12.0f - 9.0f * B - 6.0f * C) * x3 + (-18.0f + 12.0f * B + 6.0f * C) * x2 + (6.0f - 2.0f * B));
	if (x < 2.0f) return (1.0f / 6.0f) * ((-B - 6.0f * C) * x3 + (6.0f * B + 30.0f * C) * x2 + (-12.0f * B - 48.0f * C) * x + (8.0f * B + 24.0f * C));
	return 0.0f;
}

// history_normal_and_depth holds the previous frame's (normal, depth) DECODED (kernel_svgf_finalize copies the frame's decoded
// image, see kernel_svgf_reproject): up to 4 + 9 of these tests per pixel no longer decode an octahedral normal each.
RT_DEV bool is_tap_consistent(const RtParams & p, int x, int y, f3 normal, float depth) {
	if (x < 0 || x >= p.screen_width)  return false;
	if (y < 0 || y >= p.screen_height) return false;
	float4 prev = p.history_normal_and_depth[x + y * p.screen_pitch];
	return dot(normal, mk3(prev.x, prev.y, prev.z)) > 0.95f && fabsf(depth - prev.w) < 2.0f;
}

// The edge-stopping weights of the variance and a-trous filters (SVGF.h:268-282):
//     w = max(0, n . n')^sigma_n * exp(-|l - l'| * denom - |z - z'| / (sigma_z |grad z . delta| + eps))
// 8 resp. 48 taps per pixel, two weights (direct, indirect) per tap. Written with powf / expf of the device library (full
// range, correctly-rounded-ish: ~200 + 2 x 30 VALU instructions per tap) the six a-trous passes of a 1080p frame cost 0.7 ms
// of VALU time for 0.2 ms of memory traffic. Both weights are ONE power of two each:
//     w = exp2(sigma_n * log2(n . n') - (|l - l'| * denom + ln_w_z) * log2(e))
// on the hardware's v_log_f32 / v_exp_f32 / v_rcp_f32 (1 ulp each). Fed the same inputs as the oracle (powf / expf of
// libm), the filtered histories, variances and the tone-mapped colour TAA reads differ from its by at most 8.3e-7 relative
// per pixel and channel (measured on MI355X; tests/test_gpu_svgf_filter.py holds them to 1e-5, the listed variance's tree
// sums included). TAA's YCoCg clamp amplifies such differences: its history and the displayed image differ from the oracle's
// by up to 9e-4 and 3e-3 where a clamp bound is ill-conditioned; the test checks the resolve itself bit for bit from the
// device's own inputs. Nothing that decides a threshold (reprojection consistency, history lengths) goes through here: the
// history lengths, and every image of a frame with no a-trous pass and no spatial variance, are bit-identical to the oracle's.
RT_DEV float fast_log2(float x) { return __builtin_amdgcn_logf(x); }
RT_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
RT_DEV float fast_rcp(float x)  { return __builtin_amdgcn_rcpf(x); }

RT_DEV f2 edge_stopping_weights(const RtParams & p, int delta_x, int delta_y, f2 center_depth_gradient, float center_depth, float depth,
		f3 center_normal, f3 normal, float cl_direct, float cl_indirect, float l_direct, float l_indirect, float denom_direct, float denom_indirect) {
	const float log2_e = 1.44269504088896340736f;
	float d = center_depth_gradient.x * float(delta_x) + center_depth_gradient.y * float(delta_y);
	float ln_w_z = fabsf(center_depth - depth) * fast_rcp(p.config.sigma_z * fabsf(d) + RT_SVGF_EPSILON);
	float n_dot_n = fmaxf(0.0f, dot(center_normal, normal));
	// pow(0, sigma_n) = 0 for sigma_n > 0 and 1 for sigma_n = 0; log2(0) = -inf does the first, the second needs the select
	float log2_w_n = (n_dot_n > 0.0f || p.config.sigma_n > 0.0f) ? p.config.sigma_n * fast_log2(n_dot_n) : 0.0f;
	float w_l_direct   = fast_exp2(log2_w_n - (fabsf(cl_direct   - l_direct)   * denom_direct   + ln_w_z) * log2_e);
	float w_l_indirect = fast_exp2(log2_w_n - (fabsf(cl_indirect - l_indirect) * denom_indirect + ln_w_z) * log2_e);
	return mk2(w_l_direct, w_l_indirect);
}

// `direct_out` / `indirect_out` / `variance_out` (null without the spatial variance estimate): where kernel_svgf_variance writes.
// That kernel only has work for pixels whose history is shorter than 4 frames; for all others -- and the sky -- its output is
// a copy of this kernel's, which this kernel therefore writes itself (the copy used to cost a second pass over 64 B per pixel).
__global__ void __launch_bounds__(256) kernel_svgf_reproject(RtParams p, float4 * direct_out, float4 * indirect_out, float2 * variance_out) {
	int x, y;
	if (!post_tile_pixel(p, x, y)) return;
	if (x >= p.screen_width || y >= p.screen_height) return;
	int pixel_index = x + y * p.screen_pitch;

	float4 * fb_direct = p.aovs[RT_AOV_RADIANCE_DIRECT].framebuffer, * fb_indirect = p.aovs[RT_AOV_RADIANCE_INDIRECT].framebuffer;
	f4 direct = ld4(fb_direct, pixel_index), indirect = ld4(fb_indirect, pixel_index);

	f4 moment;
	moment.x = luminance(direct.x, direct.y, direct.z);
	moment.y = luminance(indirect.x, indirect.y, indirect.z);
	moment.z = moment.x * moment.x;
	moment.w = moment.y * moment.y;

	float4 normal_and_depth = p.gbuffer_normal_and_depth[pixel_index];
	float2 screen_position_prev = p.gbuffer_screen_position_prev[pixel_index];

	f3 normal = oct_decode_normal(mk2(normal_and_depth.x, normal_and_depth.y));
	float depth = normal_and_depth.z, depth_prev = normal_and_depth.w;
	// the variance and a-trous passes read every pixel's normal up to 9 + 6 x 9 times per frame: decoded once, here, into a
	// float4 of its own (normal, depth) -- the same 16 bytes per tap as the octahedral g-buffer texel, without the decode
	p.svgf_normal_and_depth[pixel_index] = make_float4(normal.x, normal.y, normal.z, depth);
	// ... and the variance pair (direct.w, indirect.w) of every pixel once more in a float2 image of its own: the a-trous passes
	// blur it over 3 x 3 neighbours, and a .w picked out of two float4 images costs the cache as much as the float4s
	if (depth == 0.0f) { // sky
		p.svgf_variance[0][pixel_index] = make_float2(direct.w, indirect.w);
		if (direct_out) { st4(direct_out, pixel_index, direct); st4(indirect_out, pixel_index, indirect); variance_out[pixel_index] = make_float2(direct.w, indirect.w); }
		return;
	}

	float s_prev = (0.5f + 0.5f * screen_position_prev.x) * float(p.screen_width);
	float t_prev = (0.5f + 0.5f * screen_position_prev.y) * float(p.screen_height);
	int x_prev = int(s_prev - 0.5f);
	int y_prev = int(t_prev - 0.5f);

	float fs = s_prev - floorf(s_prev), ft = t_prev - floorf(t_prev);
	float w0 = (1.0f - fs) * (1.0f - ft), w1 = fs * (1.0f - ft), w2 = (1.0f - fs) * ft;
	float w3 = 1.0f - w0 - w1 - w2;
	float weights[4] = { w0, w1, w2, w3 };
	float consistent_weights_sum = 0.0f;

	#pragma unroll
	for (int j = 0; j < 2; j++) {
		#pragma unroll
		for (int i = 0; i < 2; i++) {
			int tap = i + j * 2;
			if (is_tap_consistent(p, x_prev + i, y_prev + j, normal, depth_prev)) consistent_weights_sum += weights[tap];
			else weights[tap] = 0.0f;
		}
	}

	f4 prev_direct = mk4(0.0f), prev_indirect = mk4(0.0f), prev_moment = mk4(0.0f);
	if (consistent_weights_sum > 0.0f) {
		#pragma unroll
		for (int j = 0; j < 2; j++) {
			#pragma unroll
			for (int i = 0; i < 2; i++) {
				int tap = i + j * 2;
				if (weights[tap] != 0.0f) {
					int tap_index = (x_prev + i) + (y_prev + j) * p.screen_pitch;
					prev_direct   += weights[tap] * ld4(p.history_direct,   tap_index);
					prev_indirect += weights[tap] * ld4(p.history_indirect, tap_index);
					prev_moment   += weights[tap] * ld4(p.history_moment,   tap_index);
				}
			}
		}
	} else {
		for (int j = -1; j <= 1; j++) for (int i = -1; i <= 1; i++) {
			int tap_x = x_prev + i, tap_y = y_prev + j;
			if (is_tap_consistent(p, tap_x, tap_y, normal, depth_prev)) {
				int tap_index = tap_x + tap_y * p.screen_pitch;
				prev_direct   += ld4(p.history_direct,   tap_index);
				prev_indirect += ld4(p.history_indirect, tap_index);
				prev_moment   += ld4(p.history_moment,   tap_index);
				consistent_weights_sum += 1.0f;
			}
		}
	}

	int history_now = 0;   // the pixel's history length after this frame
	if (consistent_weights_sum > 0.0f) {
		prev_direct   = prev_direct   / consistent_weights_sum;
		prev_indirect = prev_indirect / consistent_weights_sum;
		prev_moment   = prev_moment   / consistent_weights_sum;

		int history = ++p.history_length[pixel_index];
		history_now = history;
		float inv_history = 1.0f / float(history);
		float alpha_colour = fmaxf(p.config.alpha_colour, inv_history);
		float alpha_moment = fmaxf(p.config.alpha_moment, inv_history);

		direct   = lerp_ref(prev_direct,   direct,   alpha_colour);
		indirect = lerp_ref(prev_indirect, indirect, alpha_colour);
		moment   = lerp_ref(prev_moment,   moment,   alpha_moment);

		if (history >= 4 || !p.config.enable_spatial_variance) {
			direct.w   = fmaxf(0.0f, moment.z - moment.x * moment.x);
			indirect.w = fmaxf(0.0f, moment.w - moment.y * moment.y);
		}
	} else {
		p.history_length[pixel_index] = 0;
		direct.w = 1.0f;
		indirect.w = 1.0f;
	}
	st4(fb_direct, pixel_index, direct);
	st4(fb_indirect, pixel_index, indirect);
	st4(p.frame_buffer_moment, pixel_index, moment);
	p.svgf_variance[0][pixel_index] = make_float2(direct.w, indirect.w);
	if (direct_out && history_now >= 4) { st4(direct_out, pixel_index, direct); st4(indirect_out, pixel_index, indirect); variance_out[pixel_index] = make_float2(direct.w, indirect.w); }
	// a pixel the spatial variance estimate has to visit: listed for kernel_svgf_variance_listed (one atomic per wave)
	if (direct_out && history_now < 4) { int slot = wave_aggregated_append(p.svgf_young_pixels); p.svgf_young_pixels[RT_SVGF_YOUNG_HEADER + slot] = pixel_index; }
}

// The spatial variance estimate of ONE pixel (SVGF.h:286-414): a 7 x 7 edge-stopping blur for pixels with fewer than 4 frames of history, nothing
// (or, in the padding columns, a copy) for the others.
RT_DEV void svgf_variance_pixel(const RtParams & p, int x, int y, const float4 * d_in, const float4 * i_in, float4 * d_out, float4 * i_out, float2 * variance_out) {
	int pixel_index = x + y * p.screen_pitch;

	int history = p.history_length[pixel_index];
	if (history >= 4 && x < p.screen_width) return;   // copied by kernel_svgf_reproject (which does not visit the padding columns: they keep the copy below)
	if (history >= 4) { float4 d = d_in[pixel_index], i = i_in[pixel_index]; d_out[pixel_index] = d; i_out[pixel_index] = i; variance_out[pixel_index] = make_float2(d.w, i.w); return; }

	const float4 * __restrict__ normal_and_depth = p.svgf_normal_and_depth;   // (normal, depth), decoded by kernel_svgf_reproject
	float luminance_denom = 1.0f / p.config.sigma_l;
	f4 cd = ld4(d_in, pixel_index), ci = ld4(i_in, pixel_index);
	float cl_d = luminance(cd.x, cd.y, cd.z), cl_i = luminance(ci.x, ci.y, ci.z);

	float4 cnd = normal_and_depth[pixel_index];
	f3 center_normal = mk3(cnd.x, cnd.y, cnd.z);
	float center_depth = cnd.w;
	int xr = min(x + 1, p.screen_pitch - 1), yd = min(y + 1, p.screen_height - 1);
	f2 grad = mk2(normal_and_depth[xr + y * p.screen_pitch].w - center_depth,
	              normal_and_depth[x + yd * p.screen_pitch].w - center_depth);

	if (center_depth == 0.0f) { if (x < p.screen_width) return; st4(d_out, pixel_index, cd); st4(i_out, pixel_index, ci); variance_out[pixel_index] = make_float2(cd.w, ci.w); return; }   // sky: copied by kernel_svgf_reproject

	float sw_d = 1.0f, sw_i = 1.0f;
	f4 sc_d = cd, sc_i = ci;
	f4 sum_moment = mk4(0.0f);
	const int radius = 3;
	for (int j = -radius; j <= radius; j++) {
		int tap_y = y + j;
		if (tap_y < 0 || tap_y >= p.screen_height) continue;
		for (int i = -radius; i <= radius; i++) {
			int tap_x = x + i;
			if (tap_x < 0 || tap_x >= p.screen_width) continue;
			if (i == 0 && j == 0) continue;
			int tap_index = tap_x + tap_y * p.screen_pitch;
			f4 td = ld4(d_in, tap_index), ti = ld4(i_in, tap_index), moment = ld4(p.frame_buffer_moment, tap_index);
			float l_d = luminance(td.x, td.y, td.z), l_i = luminance(ti.x, ti.y, ti.z);
			float4 nd = normal_and_depth[tap_index];
			f2 w = edge_stopping_weights(p, i, j, grad, center_depth, nd.w, center_normal, mk3(nd.x, nd.y, nd.z), cl_d, cl_i, l_d, l_i, luminance_denom, luminance_denom);
			sw_d += w.x; sw_i += w.y;
			sc_d += w.x * td;
			sc_i += w.y * ti;
			sum_moment += moment * mk4(w.x, w.y, w.x, w.y);
		}
	}
	sw_d = fmaxf(sw_d, 1e-6f); sw_i = fmaxf(sw_i, 1e-6f);
	sc_d = sc_d / sw_d; sc_i = sc_i / sw_i;
	sum_moment = mk4(sum_moment.x / sw_d, sum_moment.y / sw_i, sum_moment.z / sw_d, sum_moment.w / sw_i);
	sc_d.w = fmaxf(0.0f, sum_moment.z - sum_moment.x * sum_moment.x);
	sc_i.w = fmaxf(0.0f, sum_moment.w - sum_moment.y * sum_moment.y);
	st4(d_out, pixel_index, sc_d);
	st4(i_out, pixel_index, sc_i);
	variance_out[pixel_index] = make_float2(sc_d.w, sc_i.w);
}

// Every pixel of the frame (and its padding columns, as the reference: SVGF.h:293) ...
__global__ void __launch_bounds__(256) kernel_svgf_variance(RtParams p, const float4 * d_in, const float4 * i_in, float4 * d_out, float4 * i_out, float2 * variance_out) {
	int x, y;
	if (!post_tile_pixel(p, x, y)) return;
	if (x >= p.screen_pitch || y >= p.screen_height) return;
	svgf_variance_pixel(p, x, y, d_in, i_in, d_out, i_out, variance_out);
}
// ... or only the pixels kernel_svgf_reproject has listed (svgf_young_pixels: those it left with fewer than 4 frames of history; everything else
// it has copied itself), ONE WAVE per listed pixel, one of the 48 taps per lane. From the fourth frame of a view on the young pixels are the
// disoccluded ones along silhouettes, a per cent of the frame -- and the pass over all pixels took 0.034 ms all the same: not for the launch, but
// because a young pixel's lane walked its 48 taps one after the other (four dependent-latency loads each) while the rest of the machine had left.
// A lane per tap makes that one load latency and a wave reduction. The sums are formed in a tree instead of in tap order: the last bits differ from
// kernel_svgf_variance (and the oracle) as any re-association does, far inside the filter's tolerance; results do not depend on the launch shape.
// Used when the image has no padding columns (those are only ever copied, by the kernel above).
RT_DEV float wave_sum(float v) {
	#pragma unroll
	for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_xor(v, offset);
	return v;
}
__global__ void __launch_bounds__(256) kernel_svgf_variance_listed(RtParams p, const float4 * d_in, const float4 * i_in, float4 * d_out, float4 * i_out, float2 * variance_out) {
	const int count = p.svgf_young_pixels[0];
	const int lane = int(threadIdx.x) & 63, waves = int(gridDim.x * blockDim.x) >> 6;
	const int tap_j = lane / 7 - 3, tap_i = lane % 7 - 3;   // lanes 0..48: the 7 x 7 window (lane 24 is the centre), 49..63: idle
	const float4 * __restrict__ normal_and_depth = p.svgf_normal_and_depth;
	const float luminance_denom = 1.0f / p.config.sigma_l;
	for (int k = int(blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < count; k += waves) {
		const int pixel_index = p.svgf_young_pixels[RT_SVGF_YOUNG_HEADER + k];
		const int x = pixel_index % p.screen_pitch, y = pixel_index / p.screen_pitch;
		f4 cd = ld4(d_in, pixel_index), ci = ld4(i_in, pixel_index);
		float cl_d = luminance(cd.x, cd.y, cd.z), cl_i = luminance(ci.x, ci.y, ci.z);
		float4 cnd = normal_and_depth[pixel_index];
		f3 center_normal = mk3(cnd.x, cnd.y, cnd.z);
		float center_depth = cnd.w;
		if (center_depth == 0.0f) continue;   // (sky is never listed; uniform over the wave)
		int xr = min(x + 1, p.screen_pitch - 1), yd = min(y + 1, p.screen_height - 1);
		f2 grad = mk2(normal_and_depth[xr + y * p.screen_pitch].w - center_depth, normal_and_depth[x + yd * p.screen_pitch].w - center_depth);

		const int tap_x = x + tap_i, tap_y = y + tap_j;
		const bool tap = lane < 49 && lane != 24 && tap_x >= 0 && tap_x < p.screen_width && tap_y >= 0 && tap_y < p.screen_height;
		float w_d = 0.0f, w_i = 0.0f;
		f4 td = mk4(0.0f), ti = mk4(0.0f), moment = mk4(0.0f);
		if (tap) {
			const int tap_index = tap_x + tap_y * p.screen_pitch;
			td = ld4(d_in, tap_index); ti = ld4(i_in, tap_index); moment = ld4(p.frame_buffer_moment, tap_index);
			float l_d = luminance(td.x, td.y, td.z), l_i = luminance(ti.x, ti.y, ti.z);
			float4 nd = normal_and_depth[tap_index];
			f2 w = edge_stopping_weights(p, tap_i, tap_j, grad, center_depth, nd.w, center_normal, mk3(nd.x, nd.y, nd.z), cl_d, cl_i, l_d, l_i, luminance_denom, luminance_denom);
			w_d = w.x; w_i = w.y;
		}
		float sw_d = 1.0f + wave_sum(w_d), sw_i = 1.0f + wave_sum(w_i);
		f4 sc_d = cd + mk4(wave_sum(w_d * td.x), wave_sum(w_d * td.y), wave_sum(w_d * td.z), wave_sum(w_d * td.w));
		f4 sc_i = ci + mk4(wave_sum(w_i * ti.x), wave_sum(w_i * ti.y), wave_sum(w_i * ti.z), wave_sum(w_i * ti.w));
		f4 sum_moment = mk4(wave_sum(moment.x * w_d), wave_sum(moment.y * w_i), wave_sum(moment.z * w_d), wave_sum(moment.w * w_i));
		if (lane != 0) continue;
		sw_d = fmaxf(sw_d, 1e-6f); sw_i = fmaxf(sw_i, 1e-6f);
		sc_d = sc_d / sw_d; sc_i = sc_i / sw_i;
		sum_moment = mk4(sum_moment.x / sw_d, sum_moment.y / sw_i, sum_moment.z / sw_d, sum_moment.w / sw_i);
		sc_d.w = fmaxf(0.0f, sum_moment.z - sum_moment.x * sum_moment.x);
		sc_i.w = fmaxf(0.0f, sum_moment.w - sum_moment.y * sum_moment.y);
		st4(d_out, pixel_index, sc_d);
		st4(i_out, pixel_index, sc_i);
		variance_out[pixel_index] = make_float2(sc_d.w, sc_i.w);
	}
}

// One a-trous pass (SVGF.h:416-554). Per pixel: the 3x3 Gaussian blur of the variance (9 taps, .w only), then 8 taps at
// +-step_size of (direct, indirect, normal + depth) = 48 B each. The tap loops are fully unrolled (the offsets are
// -step, 0, +step: the bounds tests become four comparisons per pixel), the normals come decoded, both weights of a tap are one
// v_exp_f32 each (edge_stopping_weights): ~600 vector instructions per pixel where the literal form ran ~3 000 -- the pass
// moves 80 B of compulsory traffic per pixel and was bound by the vector ALUs at a third of the stream bandwidth
// (BENCH config3 kernels; profiles/r03_svgf.txt).
// The arithmetic of a pixel, shared by the two kernels below: `tap_d / tap_i / tap_nd (i, j)` return (direct, indirect, normal + depth) of the
// pixel at (x + i * step_size, y + j * step_size), i, j in {-1, 0, 1} -- read from the images by one kernel, from the workgroup's LDS tile by the other.
// What a pixel of an a-trous pass reads of its IMMEDIATE neighbours, whatever the step size: the 3 x 3 blur of the variance pair and the depths
// to the right and below (the depth gradient). Loaded first -- in the tiled kernel before the barrier, beside the staging loads.
struct AtrousNeighbourhood { float vb_d, vb_i, depth_right, depth_below; };
RT_DEV AtrousNeighbourhood svgf_atrous_neighbourhood(const RtParams & p, int x, int y, const float2 * __restrict__ variance_in) {
	const int pitch = p.screen_pitch;
	const float4 * __restrict__ normal_and_depth = p.svgf_normal_and_depth;   // (normal, depth), decoded by kernel_svgf_reproject
	// clamped neighbours for the variance blur
	const int xl = max(x - 1, 0), xr1 = min(x + 1, p.screen_width - 1), yu = max(y - 1, 0), yd1 = min(y + 1, p.screen_height - 1);
	const int col[3] = { xl, x, xr1 }, row[3] = { yu * pitch, y * pitch, yd1 * pitch };
	AtrousNeighbourhood n;
	n.vb_d = 0.0f; n.vb_i = 0.0f;
	#pragma unroll
	for (int j = 0; j < 3; j++) {
		#pragma unroll
		for (int i = 0; i < 3; i++) {
			const float kernel_weight = (i == 1 ? 0.5f : 0.25f) * (j == 1 ? 0.5f : 0.25f) * 1.0f;   // 0.25 * 2^-(|i| + |j|), |i| = distance from the centre
			const float2 variance = variance_in[col[i] + row[j]];   // (d_in[..].w, i_in[..].w), see kernel_svgf_reproject
			n.vb_d += variance.x * kernel_weight;
			n.vb_i += variance.y * kernel_weight;
		}
	}
	int xr = min(x + 1, pitch - 1), yd = min(y + 1, p.screen_height - 1);
	n.depth_right = normal_and_depth[xr + y * pitch].w;
	n.depth_below = normal_and_depth[x + yd * pitch].w;
	return n;
}

// What kernel_svgf_finalize does with a pixel's filtered (direct, indirect) pair (SVGF.h:556-609) -- shared by that kernel and by the LAST a-trous pass when it runs
// tiled (round 6): the pass then hands its result over in registers instead of writing the pair (and its variance mirror, which nothing reads after the last pass) for a
// kernel that reads it back: 88 bytes per pixel and a launch less. `normal_and_depth`: the frame's decoded (normal, depth) of the pixel.
RT_DEV void svgf_finalize_pixel(const RtParams & p, int pixel_index, f4 direct, f4 indirect, float4 normal_and_depth) {
	if (pixel_index == 0) p.svgf_young_pixels[0] = 0;   // (this frame's variance pass is behind us: the next frame's reproject fills the list again)
	f4 colour = (direct + indirect) * aov_get(p, RT_AOV_ALBEDO, pixel_index);
	st4(p.final_image, pixel_index, colour);

	if (p.config.enable_taa) {
		colour = colour / (1.0f + luminance(colour.x, colour.y, colour.z));
		colour.x = safe_sqrt(colour.x); colour.y = safe_sqrt(colour.y); colour.z = safe_sqrt(colour.z);
		st4(p.taa_frame_curr, pixel_index, colour);
	}
	float4 moment = p.frame_buffer_moment[pixel_index];
	if (p.config.num_atrous_iterations <= RT_FEEDBACK_ITERATION) { st4(p.history_direct, pixel_index, direct); st4(p.history_indirect, pixel_index, indirect); }
	p.history_moment[pixel_index] = moment;
	p.history_normal_and_depth[pixel_index] = normal_and_depth;   // decoded (normal, depth) of this frame

	p.gbuffer_normal_and_depth[pixel_index] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	p.gbuffer_mesh_id_and_triangle_id[pixel_index] = make_int2(0, 0);
	if (!p.config.enable_taa) p.gbuffer_screen_position_prev[pixel_index] = make_float2(0.0f, 0.0f);
}

// FINAL: the frame's last pass; the result goes to svgf_finalize_pixel instead of the images (a sky pixel, which no pass writes, finalizes what the pair's images hold for it:
// exactly what kernel_svgf_finalize would have read).
template<bool FINAL = false, typename TapD, typename TapI, typename TapND>
RT_DEV void svgf_atrous_pixel(const RtParams & p, int x, int y, int step_size, const AtrousNeighbourhood & near, float4 * __restrict__ d_out, float4 * __restrict__ i_out,
                              float2 * __restrict__ variance_out, TapD tap_d, TapI tap_i, TapND tap_nd) {
	const int pitch = p.screen_pitch;
	int pixel_index = x + y * pitch;
	float denom_d = 1.0f / sqrtf(p.config.sigma_l * p.config.sigma_l * fmaxf(0.0f, near.vb_d) + RT_SVGF_EPSILON);
	float denom_i = 1.0f / sqrtf(p.config.sigma_l * p.config.sigma_l * fmaxf(0.0f, near.vb_i) + RT_SVGF_EPSILON);

	f4 cd = mk4(tap_d(0, 0)), ci = mk4(tap_i(0, 0));
	float cl_d = luminance(cd.x, cd.y, cd.z), cl_i = luminance(ci.x, ci.y, ci.z);

	float4 cnd = tap_nd(0, 0);
	f3 center_normal = mk3(cnd.x, cnd.y, cnd.z);
	float center_depth = cnd.w;
	if (center_depth == 0.0f) { // sky: outputs intentionally not written (SVGF.h:462)
		if (FINAL) svgf_finalize_pixel(p, pixel_index, ld4(d_out, pixel_index), ld4(i_out, pixel_index), cnd);
		return;
	}

	f2 grad = mk2(near.depth_right - center_depth, near.depth_below - center_depth);

	const bool in_x[3] = { x - step_size >= 0, true, x + step_size < p.screen_width };
	const bool in_y[3] = { y - step_size >= 0, true, y + step_size < p.screen_height };
	float sw_d = 1.0f, sw_i = 1.0f;
	f4 sc_d = cd, sc_i = ci;
	#pragma unroll
	for (int j = -1; j <= 1; j++) {
		#pragma unroll
		for (int i = -1; i <= 1; i++) {
			if (i == 0 && j == 0) continue;
			if (in_x[i + 1] && in_y[j + 1]) {
				f4 td = mk4(tap_d(i, j)), ti = mk4(tap_i(i, j));
				float4 nd = tap_nd(i, j);
				float l_d = luminance(td.x, td.y, td.z), l_i = luminance(ti.x, ti.y, ti.z);
				f2 w = edge_stopping_weights(p, i * step_size, j * step_size, grad, center_depth, nd.w, center_normal, mk3(nd.x, nd.y, nd.z), cl_d, cl_i, l_d, l_i, denom_d, denom_i);
				sw_d += w.x; sw_i += w.y;
				sc_d += mk4(w.x, w.x, w.x, w.x * w.x) * td;
				sc_i += mk4(w.y, w.y, w.y, w.y * w.y) * ti;
			}
		}
	}
	float inv_d = 1.0f / sw_d, inv_i = 1.0f / sw_i;
	sc_d *= inv_d; sc_i *= inv_i;
	sc_d.w *= inv_d; sc_i.w *= inv_i;
	if (step_size == (1 << RT_FEEDBACK_ITERATION)) { st4(p.history_direct, pixel_index, sc_d); st4(p.history_indirect, pixel_index, sc_i); }
	if (FINAL) { svgf_finalize_pixel(p, pixel_index, sc_d, sc_i, cnd); return; }
	st4(d_out, pixel_index, sc_d);
	st4(i_out, pixel_index, sc_i);
	variance_out[pixel_index] = make_float2(sc_d.w, sc_i.w);
}

__global__ void __launch_bounds__(256) kernel_svgf_atrous(RtParams p, const float4 * __restrict__ d_in, const float4 * __restrict__ i_in, float4 * __restrict__ d_out, float4 * __restrict__ i_out, const float2 * __restrict__ variance_in, float2 * __restrict__ variance_out, int step_size) {
	int x, y;
	if (!post_tile_pixel(p, x, y)) return;
	if (x >= p.screen_width || y >= p.screen_height) return;
	const int pitch = p.screen_pitch, pixel_index = x + y * pitch;
	const float4 * __restrict__ normal_and_depth = p.svgf_normal_and_depth;
	svgf_atrous_pixel(p, x, y, step_size, svgf_atrous_neighbourhood(p, x, y, variance_in), d_out, i_out, variance_out,
		[&](int i, int j) { return d_in[pixel_index + i * step_size + j * step_size * pitch]; },
		[&](int i, int j) { return i_in[pixel_index + i * step_size + j * step_size * pitch]; },
		[&](int i, int j) { return normal_and_depth[pixel_index + i * step_size + j * step_size * pitch]; });
}

// The same pass with the three tapped images of a workgroup staged in LDS (rt_set_svgf_tiles, on by default).
// The pass above asks for 9 x 48 B of taps per pixel of which 48 B are compulsory; its 64 x 4 tiles share the taps of a row among their
// lanes but not the three rows a tap pattern spans (for a step of 4 and more they are twelve different rows for four rows of pixels), and what
// L1 does not hold comes over the L2 -> L1 path again: ~560 B per pixel and pass, 17 TB/s at 0.063 ms per 1080p pass -- the pass is bound
// by THAT, at half the stream rate of its compulsory bytes (BENCH config3: frac_unique 0.51). Two things make a tile's taps mostly its own:
//   * a workgroup's TY rows of pixels are STEP rows apart (y = y_base + STEP * k): the row above the first and the row below the last are
//     all it needs beside its own -- (TY + 2) / TY rows per row of pixels at every step size, where adjacent rows need 3 from step 4 on;
//   * the columns are 64 adjacent pixels plus STEP on either side, loaded once into LDS ([row][column], float4 per image) and tapped
//     from there with ds_read_b128: the L1 / L2 path sees (64 + 2 STEP) / 64 x (TY + 2) / TY of the compulsory bytes (1.3 x at step 1,
//     2.5 x at step 32) instead of 9 x.
// The 3 x 3 variance blur and the depth gradient look at a pixel's immediate neighbours, which are not in the tile unless STEP is 1: they
// stay global loads (8 and 16 bytes, rows shared by the lanes of a wave). Same arithmetic per pixel (svgf_atrous_pixel): images are
// bit-identical to the untiled pass (tests/test_gpu_materials_svgf.py::test_svgf_lds_tiles_do_not_change_a_frame).
// Tiles are numbered column-fastest within one residue class of rows, XCD k takes the k-th eighth of the sequence (as post_tile_pixel):
// neighbours in x, which share their STEP halo columns, run back to back on one L2.
#ifndef RT_SVGF_FUSED_FINALIZE
#define RT_SVGF_FUSED_FINALIZE 1   // the last tiled a-trous pass finalizes its pixels itself (svgf_finalize_pixel); 0: kernel_svgf_finalize after it, as the reference does
#endif
#ifndef RT_ATROUS_ROWS
#define RT_ATROUS_ROWS 8   // rows of pixels per workgroup (one wave each) of the tiled passes up to step 16
#endif
template<int STEP, int TY, bool FINAL>
__global__ void __launch_bounds__(64 * TY) kernel_svgf_atrous_tiled(RtParams p, const float4 * __restrict__ d_in, const float4 * __restrict__ i_in, float4 * __restrict__ d_out, float4 * __restrict__ i_out, const float2 * __restrict__ variance_in, float2 * __restrict__ variance_out) {
	constexpr int W = 64 + 2 * STEP, ROWS = TY + 2, N = W * ROWS, THREADS = 64 * TY;
	__shared__ float4 tile_d[N], tile_i[N], tile_nd[N];
	const unsigned tiles_x = (unsigned(p.screen_width) + 63u) / 64u;
	const unsigned blocks_y = (unsigned(p.screen_height) + unsigned(TY * STEP) - 1u) / unsigned(TY * STEP);
	const unsigned tiles = tiles_x * unsigned(STEP) * blocks_y, tile = xcd_tile();
	if (tile >= tiles) return;   // (the whole workgroup: no barrier is left waiting)
	const int x0 = int(tile % tiles_x) * 64;
	const unsigned above = tile / tiles_x;
	const int y_base = int(above / unsigned(STEP)) * (TY * STEP) + int(above % unsigned(STEP));
	const int pitch = p.screen_pitch;
	const float4 * __restrict__ normal_and_depth = p.svgf_normal_and_depth;

	// this thread's pixel, and what it needs of its immediate neighbours (global loads: issued before the staging loop, they land with it)
	const int tx = int(threadIdx.x) & 63, ty = int(threadIdx.x) >> 6;
	const int x = x0 + tx, y = y_base + STEP * ty;
	const bool has_pixel = x < p.screen_width && y < p.screen_height;
	AtrousNeighbourhood near = { 0.0f, 0.0f, 0.0f, 0.0f };
	if (has_pixel) near = svgf_atrous_neighbourhood(p, x, y, variance_in);

	// stage: row r of the tile is image row y_base + STEP * (r - 1), column c is image column x0 - STEP + c. Positions outside the image are never
	// tapped (in_x / in_y of svgf_atrous_pixel); they are filled from the clamped position so that every load is inside the images.
	for (int pos = int(threadIdx.x); pos < N; pos += THREADS) {
		const int c = pos % W, r = pos / W;
		const int gx = min(max(x0 - STEP + c, 0), p.screen_width - 1), gy = min(max(y_base + STEP * (r - 1), 0), p.screen_height - 1);
		const int source = gx + gy * pitch;
		tile_d[pos] = d_in[source]; tile_i[pos] = i_in[source]; tile_nd[pos] = normal_and_depth[source];
	}
	__syncthreads();

	if (!has_pixel) return;
	const int centre = (ty + 1) * W + tx + STEP;
	svgf_atrous_pixel<FINAL>(p, x, y, STEP, near, d_out, i_out, variance_out,
		[&](int i, int j) { return tile_d [centre + i * STEP + j * W]; },
		[&](int i, int j) { return tile_i [centre + i * STEP + j * W]; },
		[&](int i, int j) { return tile_nd[centre + i * STEP + j * W]; });
}
template<int STEP, int TY>
static void launch_atrous_tiled(const RtParams & p, bool final_pass, const float4 * d_in, const float4 * i_in, float4 * d_out, float4 * i_out, const float2 * variance_in, float2 * variance_out, hipStream_t stream) {
	const unsigned tiles = ((unsigned(p.screen_width) + 63u) / 64u) * unsigned(STEP) * ((unsigned(p.screen_height) + unsigned(TY * STEP) - 1u) / unsigned(TY * STEP));
	if (final_pass) hipLaunchKernelGGL((kernel_svgf_atrous_tiled<STEP, TY, true>), dim3(xcd_tile_grid(tiles)), dim3(64 * TY), 0, stream, p, d_in, i_in, d_out, i_out, variance_in, variance_out);
	else hipLaunchKernelGGL((kernel_svgf_atrous_tiled<STEP, TY, false>), dim3(xcd_tile_grid(tiles)), dim3(64 * TY), 0, stream, p, d_in, i_in, d_out, i_out, variance_in, variance_out);
}
// false: no tiled form for this step size (more than six iterations): the caller launches kernel_svgf_atrous
static bool launch_atrous_tiled_step(const RtParams & p, int step_size, bool final_pass, const float4 * d_in, const float4 * i_in, float4 * d_out, float4 * i_out, const float2 * variance_in, float2 * variance_out, hipStream_t stream) {
	switch (step_size) {   // LDS per workgroup: (64 + 2 STEP) x (TY + 2) x 48 B = 31.7 / 32.6 / 34.6 / 38.4 / 46.1 / 36.9 KB with 8 rows (4 at step 32)
		case 1:  launch_atrous_tiled<1,  RT_ATROUS_ROWS>(p, final_pass, d_in, i_in, d_out, i_out, variance_in, variance_out, stream); return true;
		case 2:  launch_atrous_tiled<2,  RT_ATROUS_ROWS>(p, final_pass, d_in, i_in, d_out, i_out, variance_in, variance_out, stream); return true;
		case 4:  launch_atrous_tiled<4,  RT_ATROUS_ROWS>(p, final_pass, d_in, i_in, d_out, i_out, variance_in, variance_out, stream); return true;
		case 8:  launch_atrous_tiled<8,  RT_ATROUS_ROWS>(p, final_pass, d_in, i_in, d_out, i_out, variance_in, variance_out, stream); return true;
		case 16: launch_atrous_tiled<16, RT_ATROUS_ROWS>(p, final_pass, d_in, i_in, d_out, i_out, variance_in, variance_out, stream); return true;
		case 32: launch_atrous_tiled<32, 4>(p, final_pass, d_in, i_in, d_out, i_out, variance_in, variance_out, stream); return true;
	}
	return false;
}

__global__ void __launch_bounds__(256) kernel_svgf_finalize(RtParams p, const float4 * colour_direct, const float4 * colour_indirect) {
	int x, y;
	if (!post_tile_pixel(p, x, y)) return;
	if (x >= p.screen_width || y >= p.screen_height) return;
	int pixel_index = x + y * p.screen_pitch;
	svgf_finalize_pixel(p, pixel_index, ld4(colour_direct, pixel_index), ld4(colour_indirect, pixel_index), p.svgf_normal_and_depth[pixel_index]);
}

RT_DEV f3 clamp3(f3 v, f3 lo, f3 hi) { return mk3(clampf(v.x, lo.x, hi.x), clampf(v.y, lo.y, hi.y), clampf(v.z, lo.z, hi.z)); }

// Reads taa_frame_curr (3 x 3 around the pixel) and taa_frame_prev (4 x 4 around where the pixel was), and writes what the reference's
// kernel_taa and kernel_taa_finalize write between them (TAA.h:10-172): the resolved colour as the NEXT frame's history, the displayed image
// (the tone mapping undone), the cleared motion vector. The history goes to a third image, taa_frame_next -- other threads are still reading
// taa_frame_prev --, and the host swaps the two pointers after the launch (rt_api.hip, rt_render.hip, rt_stream.hip: after every rt_launch_svgf_taa). The reference needs
// the second kernel because it resolves in place; here that pass (read 16, write 40 bytes per pixel) is gone.
__global__ void __launch_bounds__(256) kernel_taa(RtParams p, int sample_index) {
	int x, y;
	if (!post_tile_pixel(p, x, y)) return;
	if (x >= p.screen_width || y >= p.screen_height) return;
	int pixel_index = x + y * p.screen_pitch;

	f4 colour = ld4(p.taa_frame_curr, pixel_index);
	auto finish = [&](f4 resolved) {   // kernel_taa_finalize (TAA.h:150-172)
		st4(p.taa_frame_next, pixel_index, resolved);
		resolved = resolved * resolved;
		resolved = resolved / (1.0f - luminance(resolved.x, resolved.y, resolved.z));
		st4(p.final_image, pixel_index, resolved);
		p.gbuffer_screen_position_prev[pixel_index] = make_float2(0.0f, 0.0f);
	};
	if (sample_index == 0) { finish(colour); return; }

	float2 sp = p.gbuffer_screen_position_prev[pixel_index];
	float s_prev = (0.5f + 0.5f * sp.x) * float(p.screen_width);
	float t_prev = (0.5f + 0.5f * sp.y) * float(p.screen_height);
	int x_prev = int(s_prev + 0.5f), y_prev = int(t_prev + 0.5f);

	float sum_weight = 0.0f;
	f4 sum = mk4(0.0f);
	for (int j = y_prev - 2; j < y_prev + 2; j++) {
		if (j < 0 || j >= p.screen_height) continue;
		for (int i = x_prev - 2; i < x_prev + 2; i++) {
			if (i < 0 || i >= p.screen_width) continue;
			float weight = mitchell_netravali(float(i) + 0.5f - s_prev) * mitchell_netravali(float(j) + 0.5f - t_prev);
			sum_weight += weight;
			sum += weight * ld4(p.taa_frame_prev, i + j * p.screen_pitch);
		}
	}
	if (sum_weight > 0.0f) {
		f3 colour_curr = rgb_to_ycocg(mk3(colour));
		f3 colour_prev = rgb_to_ycocg(mk3(sum / sum_weight));
		f3 avg = colour_curr, var = colour_curr * colour_curr;
		int pitch = p.screen_pitch;
		#define RT_TAA_TAP(offset) { f3 c = rgb_to_ycocg(mk3(ld4(p.taa_frame_curr, pixel_index + (offset)))); avg += c; var += c * c; }
		if (x >= 1) {
			if (y >= 1) RT_TAA_TAP(-pitch - 1)
			RT_TAA_TAP(-1)
			if (y < p.screen_height - 1) RT_TAA_TAP(pitch - 1)
		}
		if (y >= 1) RT_TAA_TAP(-pitch)
		if (y < p.screen_height - 1) RT_TAA_TAP(pitch)
		if (x < p.screen_width - 1) {
			if (y >= 1) RT_TAA_TAP(1 - pitch)
			RT_TAA_TAP(1)
			if (y < p.screen_height - 1) RT_TAA_TAP(1 + pitch)
		}
		#undef RT_TAA_TAP
		avg *= 1.0f / 9.0f; var *= 1.0f / 9.0f;
		f3 sigma2 = var - avg * avg;
		f3 sigma = mk3(safe_sqrt(sigma2.x), safe_sqrt(sigma2.y), safe_sqrt(sigma2.z));
		colour_prev = clamp3(colour_prev, avg - 1.25f * sigma, avg + 1.25f * sigma);
		f3 integrated = ycocg_to_rgb(lerp_ref(colour_prev, colour_curr, 0.1f));
		colour.x = integrated.x; colour.y = integrated.y; colour.z = integrated.z;
	}
	finish(colour);
}

// Launch order of Pathtracer::render (Pathtracer.cpp:798-838)
void rt_launch_svgf_taa(const RtParams & p, int sample_index, hipStream_t stream, void (*mark)(void * user, int svgf_kernel, hipStream_t stream), void * user) {
	dim3 block(RT_POST_BLOCK_X, RT_POST_BLOCK_Y);
	const unsigned tiles = ((p.screen_pitch + block.x - 1) / block.x) * ((p.screen_height + block.y - 1) / block.y);
	dim3 grid(xcd_tile_grid(tiles));
	#define RT_TIMED(k, launch) { if (mark) mark(user, k, stream); launch; if (mark) mark(user, k, stream); }

	float4 * direct_in    = p.aovs[RT_AOV_RADIANCE_DIRECT].framebuffer;
	float4 * indirect_in  = p.aovs[RT_AOV_RADIANCE_INDIRECT].framebuffer;
	float4 * direct_out   = p.aovs[RT_AOV_RADIANCE_DIRECT].accumulator;
	float4 * indirect_out = p.aovs[RT_AOV_RADIANCE_INDIRECT].accumulator;
	const bool estimate = p.config.enable_spatial_variance != 0;
	RT_TIMED(0, hipLaunchKernelGGL(kernel_svgf_reproject, grid, block, 0, stream, p, estimate ? direct_out : nullptr, estimate ? indirect_out : nullptr, estimate ? p.svgf_variance[1] : nullptr));

	// svgf_variance[0] mirrors the .w of the two framebuffers, [1] that of the two accumulators -- pixel for pixel, the ones a pass
	// leaves unwritten (sky) included: every kernel that writes a (direct, indirect) pair writes the pair's variances as well
	float2 * variance_in = p.svgf_variance[0], * variance_out = p.svgf_variance[1];
	if (p.config.enable_spatial_variance) {
		if (p.screen_pitch == p.screen_width) { RT_TIMED(1, hipLaunchKernelGGL(kernel_svgf_variance_listed, dim3(2048), dim3(256), 0, stream, p, direct_in, indirect_in, direct_out, indirect_out, variance_out)); }
		else { RT_TIMED(1, hipLaunchKernelGGL(kernel_svgf_variance, grid, block, 0, stream, p, direct_in, indirect_in, direct_out, indirect_out, variance_out)); }
		float4 * t = direct_in; direct_in = direct_out; direct_out = t;
		t = indirect_in; indirect_in = indirect_out; indirect_out = t;
		float2 * v = variance_in; variance_in = variance_out; variance_out = v;
	}
	bool finalized = false;   // the last pass has run tiled and has done kernel_svgf_finalize's work on its way out
	for (int i = 0; i < p.config.num_atrous_iterations; i++) {
		const bool last = i == p.config.num_atrous_iterations - 1;
		auto atrous_pass = [&](int step_size) {
			if (p.svgf_tiles && launch_atrous_tiled_step(p, step_size, last && RT_SVGF_FUSED_FINALIZE, direct_in, indirect_in, direct_out, indirect_out, variance_in, variance_out, stream)) { finalized = last && RT_SVGF_FUSED_FINALIZE; return; }
			hipLaunchKernelGGL(kernel_svgf_atrous, grid, block, 0, stream, p, direct_in, indirect_in, direct_out, indirect_out, variance_in, variance_out, step_size);
		};
		RT_TIMED(2, atrous_pass(1 << i));
		float4 * t = direct_in; direct_in = direct_out; direct_out = t;
		t = indirect_in; indirect_in = indirect_out; indirect_out = t;
		float2 * v = variance_in; variance_in = variance_out; variance_out = v;
	}
	if (!finalized) RT_TIMED(3, hipLaunchKernelGGL(kernel_svgf_finalize, grid, block, 0, stream, p, direct_in, indirect_in));

	if (p.config.enable_taa) {
		RT_TIMED(4, hipLaunchKernelGGL(kernel_taa, grid, block, 0, stream, p, sample_index));   // (the caller swaps taa_frame_prev / taa_frame_next)
	}
	#undef RT_TIMED
}

// ---- Kulla-Conty LUT integration (KullaConty.h:83-240) -------------------------------------------------------
// One thread per LUT cell, NUM_SAMPLES Monte-Carlo samples each, online average.

#define RT_LUT_NUM_SAMPLES 100000

__global__ void kernel_integrate_dielectric(RtParams p, int entering_material, float * lut_directional_albedo) {
	int thread_index = blockIdx.x * blockDim.x + threadIdx.x;
	if (thread_index >= 16 * 16 * 16) return;
	int i = thread_index % 16, r = (thread_index / 16) % 16, c = (thread_index / 256) % 16;

	float ior = remap((float(i) + 0.5f) / 16.0f, 0.0f, 1.0f, RT_LUT_DIELECTRIC_MIN_IOR, RT_LUT_DIELECTRIC_MAX_IOR);
	float eta = entering_material ? 1.0f / ior : ior;
	float linear_roughness = (float(r) + 0.5f) / 16.0f;
	float cos_theta = (float(c) + 0.5f) / 16.0f;
	float sin_theta = safe_sqrt(1.0f - square(cos_theta));
	f3 omega_i = mk3(sin_theta, 0.0f, cos_theta);

	float ax = roughness_to_alpha(linear_roughness), ay = ax;
	float avg = 0.0f;
	for (int s = 0; s < RT_LUT_NUM_SAMPLES; s++) {
		float rand_fresnel = random_sample(p, DIM_BSDF_0, unsigned(thread_index), 0, unsigned(s)).y;
		f2    rand_brdf    = random_sample(p, DIM_BSDF_1, unsigned(thread_index), 0, unsigned(s));

		f3 omega_m = sample_visible_normals_ggx(omega_i, ax, ay, rand_brdf.x, rand_brdf.y);
		float F = fresnel_dielectric(abs_dot(omega_i, omega_m), eta);
		bool reflected = rand_fresnel < F;
		f3 omega_o = reflected ? reflect_direction(omega_i, omega_m) : refract_direction(omega_i, omega_m, eta);

		float weight = 0.0f;
		if (!(reflected ^ (omega_o.z >= 0.0f))) {
			float D  = ggx_D(omega_m, ax, ay);
			float G1 = ggx_G1(omega_i, ax, ay);
			float G2 = ggx_G2(omega_o, omega_i, omega_m, ax, ay);
			float i_dot_m = abs_dot(omega_i, omega_m);
			float o_dot_m = abs_dot(omega_o, omega_m);
			float pdf = reflected ? F * G1 * D / (4.0f * omega_i.z)
			                      : (1.0f - F) * G1 * D * i_dot_m * o_dot_m / (omega_i.z * square(eta * i_dot_m + o_dot_m));
			weight = pdf_is_valid(pdf) ? G2 / G1 : 0.0f;
		}
		avg = avg + (weight - avg) / float(s + 1);
	}
	lut_directional_albedo[thread_index] = avg;
}

__global__ void kernel_average_dielectric(const float * lut_directional_albedo, float * lut_albedo) {
	int thread_index = blockIdx.x * blockDim.x + threadIdx.x;
	if (thread_index >= 16 * 16) return;
	int i = thread_index % 16, r = (thread_index / 16) % 16;
	float avg = 0.0f;
	for (int c = 0; c < 16; c++) {
		float cos_theta = (float(c) + 0.5f) / 16.0f;
		float sample = lut_directional_albedo[i + r * 16 + c * 256] * cos_theta;
		avg = avg + (sample - avg) / float(c + 1);
	}
	lut_albedo[thread_index] = 2.0f * avg;
}

__global__ void kernel_integrate_conductor(RtParams p, float * lut_directional_albedo) {
	int thread_index = blockIdx.x * blockDim.x + threadIdx.x;
	if (thread_index >= 32 * 32) return;
	int r = thread_index % 32, c = (thread_index / 32) % 32;
	float linear_roughness = (float(r) + 0.5f) / 32.0f;
	float cos_theta = (float(c) + 0.5f) / 32.0f;
	float sin_theta = safe_sqrt(1.0f - square(cos_theta));
	f3 omega_i = mk3(sin_theta, 0.0f, cos_theta);
	float ax = roughness_to_alpha(linear_roughness), ay = ax;

	float avg = 0.0f;
	for (int s = 0; s < RT_LUT_NUM_SAMPLES; s++) {
		f2 rand_brdf = random_sample(p, DIM_BSDF_0, unsigned(thread_index), 0, unsigned(s));
		f3 omega_m = sample_visible_normals_ggx(omega_i, ax, ay, rand_brdf.x, rand_brdf.y);
		f3 omega_o = reflect_direction(omega_i, omega_m);
		float weight = 0.0f;
		if (!(dot(omega_o, omega_m) <= 0.0f || omega_o.z <= 0.0f)) {
			float D  = ggx_D(omega_m, ax, ay);
			float G1 = ggx_G1(omega_i, ax, ay);
			float G2 = ggx_G2(omega_o, omega_i, omega_m, ax, ay);
			float pdf = G1 * D / (4.0f * omega_i.z);
			weight = pdf_is_valid(pdf) ? G2 / G1 : 0.0f;
		}
		avg = avg + (weight - avg) / float(s + 1);
	}
	lut_directional_albedo[thread_index] = avg;
}

__global__ void kernel_average_conductor(const float * lut_directional_albedo, float * lut_albedo) {
	int thread_index = blockIdx.x * blockDim.x + threadIdx.x;
	if (thread_index >= 32) return;
	int r = thread_index;
	float avg = 0.0f;
	for (int c = 0; c < 32; c++) {
		float cos_theta = (float(c) + 0.5f) / 32.0f;
		float sample = lut_directional_albedo[r + c * 32] * cos_theta;
		avg = avg + (sample - avg) / float(c + 1);
	}
	lut_albedo[thread_index] = 2.0f * avg;
}

void rt_launch_integrate_luts(const RtParams & p, float * dielectric_dir_enter, float * dielectric_dir_leave, float * dielectric_enter, float * dielectric_leave,
                              float * conductor_dir, float * conductor, hipStream_t stream) {
	// The cells draw their samples with random_sample(thread_index, ...), whose first step splits a *virtual* pixel
	// index by the frame size (sample batches, rt_types.h). A cell index is not a path index: give the kernels the
	// pre-resize split (one 2^30-pixel frame) so that cells never fold onto each other and the tables do not
	// depend on the render resolution -- as in the reference, whose random<>() knows no such split.
	RtParams q = p;
	q.frame_pixels = 1u << 30; q.frame_pixels_magic = 5;
	// 64-thread blocks: 4096 cells -> 64 workgroups, so the long sample loops spread over many CUs
	hipLaunchKernelGGL(kernel_integrate_dielectric, dim3(4096 / 64), dim3(64), 0, stream, q, 1, dielectric_dir_enter);
	hipLaunchKernelGGL(kernel_integrate_dielectric, dim3(4096 / 64), dim3(64), 0, stream, q, 0, dielectric_dir_leave);
	hipLaunchKernelGGL(kernel_average_dielectric, dim3(1), dim3(256), 0, stream, dielectric_dir_enter, dielectric_enter);
	hipLaunchKernelGGL(kernel_average_dielectric, dim3(1), dim3(256), 0, stream, dielectric_dir_leave, dielectric_leave);
	hipLaunchKernelGGL(kernel_integrate_conductor, dim3(1024 / 64), dim3(64), 0, stream, q, conductor_dir);
	hipLaunchKernelGGL(kernel_average_conductor, dim3(1), dim3(64), 0, stream, conductor_dir, conductor);
}

// ---- multi-GPU frame exchange: pack this rank's tiles / scatter the all-gathered tiles -------------------------

__global__ void __launch_bounds__(256) kernel_pack_pixels(RtParams p, float4 * dst, int tile_pixels, int tile_first, int tile_stride, int count) {
	int frame_pixels = p.screen_width * p.screen_height;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		int g = ((i / tile_pixels) * tile_stride + tile_first) * tile_pixels + i % tile_pixels;
		float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (g < frame_pixels) v = p.final_image[g % p.screen_width + (g / p.screen_width) * p.screen_pitch];
		dst[i] = v;
	}
}

__global__ void __launch_bounds__(256) kernel_unpack_pixels(RtParams p, const float4 * src, int tile_pixels, int world, int tiles_per_rank) {
	int frame_pixels = p.screen_width * p.screen_height;
	for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < frame_pixels; g += gridDim.x * blockDim.x) {
		int tile = g / tile_pixels;
		int owner = tile % world, slot = tile / world;
		p.final_image[g % p.screen_width + (g / p.screen_width) * p.screen_pitch] = src[size_t(owner * tiles_per_rank + slot) * tile_pixels + g % tile_pixels];
	}
}

// SVGF under the tile split: what the filter stage of a frame reads of THIS frame's path tracing -- the
// per-frame DIRECT / INDIRECT / ALBEDO buffers and the three g-buffers -- travels as 5 float4 per pixel (80 B): every rank
// packs its tiles, one all-gather, every rank scatters all tiles and then filters the whole frame (its histories are
// complete: it filtered every earlier frame too).
__global__ void __launch_bounds__(256) kernel_pack_svgf(RtParams p, float4 * dst, int tile_pixels, int tile_first, int tile_stride, int count) {
	int frame_pixels = p.screen_width * p.screen_height;
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		int g = ((i / tile_pixels) * tile_stride + tile_first) * tile_pixels + i % tile_pixels;
		float4 v[5];
		for (int k = 0; k < 5; k++) v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (g < frame_pixels) {
			int idx = g % p.screen_width + (g / p.screen_width) * p.screen_pitch;
			v[0] = p.aovs[RT_AOV_RADIANCE_DIRECT].framebuffer[idx];
			v[1] = p.aovs[RT_AOV_RADIANCE_INDIRECT].framebuffer[idx];
			v[2] = p.aovs[RT_AOV_ALBEDO].framebuffer[idx];
			v[3] = p.gbuffer_normal_and_depth[idx];
			int2 ids = p.gbuffer_mesh_id_and_triangle_id[idx]; float2 prev = p.gbuffer_screen_position_prev[idx];
			v[4] = make_float4(__int_as_float(ids.x), __int_as_float(ids.y), prev.x, prev.y);
		}
		for (int k = 0; k < 5; k++) dst[size_t(5) * i + k] = v[k];
	}
}
__global__ void __launch_bounds__(256) kernel_unpack_svgf(RtParams p, const float4 * src, int tile_pixels, int world, int tiles_per_rank) {
	int frame_pixels = p.screen_width * p.screen_height;
	for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < frame_pixels; g += gridDim.x * blockDim.x) {
		int tile = g / tile_pixels;
		int owner = tile % world, slot = tile / world;
		const float4 * v = src + size_t(5) * (size_t(owner * tiles_per_rank + slot) * tile_pixels + g % tile_pixels);
		int idx = g % p.screen_width + (g / p.screen_width) * p.screen_pitch;
		p.aovs[RT_AOV_RADIANCE_DIRECT].framebuffer[idx]   = v[0];
		p.aovs[RT_AOV_RADIANCE_INDIRECT].framebuffer[idx] = v[1];
		p.aovs[RT_AOV_ALBEDO].framebuffer[idx]            = v[2];
		p.gbuffer_normal_and_depth[idx] = v[3];
		float4 w = v[4];
		p.gbuffer_mesh_id_and_triangle_id[idx] = make_int2(__float_as_int(w.x), __float_as_int(w.y));
		p.gbuffer_screen_position_prev[idx]    = make_float2(w.z, w.w);
	}
}
void rt_launch_pack_svgf(const RtParams & p, float4 * dst, int tile_pixels, int tile_first, int tile_stride, int tiles, hipStream_t stream) {
	int count = tiles * tile_pixels;
	int blocks = (count + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
	hipLaunchKernelGGL(kernel_pack_svgf, dim3(blocks), dim3(256), 0, stream, p, dst, tile_pixels, tile_first, tile_stride, count);
}
void rt_launch_unpack_svgf(const RtParams & p, const float4 * src, int tile_pixels, int world, int tiles_per_rank, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_unpack_svgf, dim3(4096), dim3(256), 0, stream, p, src, tile_pixels, world, tiles_per_rank);
}

void rt_launch_pack_pixels(const RtParams & p, float4 * dst, int tile_pixels, int tile_first, int tile_stride, int tiles, hipStream_t stream) {
	int count = tiles * tile_pixels;
	int blocks = (count + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
	hipLaunchKernelGGL(kernel_pack_pixels, dim3(blocks), dim3(256), 0, stream, p, dst, tile_pixels, tile_first, tile_stride, count);
}
void rt_launch_unpack_pixels(const RtParams & p, const float4 * src, int tile_pixels, int world, int tiles_per_rank, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_unpack_pixels, dim3(4096), dim3(256), 0, stream, p, src, tile_pixels, world, tiles_per_rank);
}

// ---- streaming-read probe: the measured HBM roofline the trace kernel is priced against --------------------

__global__ void __launch_bounds__(256) kernel_stream_read(const float4 * __restrict__ src, size_t count, float * sink) {
	float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	size_t stride = size_t(gridDim.x) * blockDim.x;
	for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
		float4 v = src[i];
		acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
	}
	if (acc.x + acc.y + acc.z + acc.w == 123456.789f) *sink = acc.x; // never true: keeps the loads alive
}

void rt_launch_stream_read(const float4 * src, size_t count, float * sink, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_stream_read, dim3(256 * 8), dim3(256), 0, stream, src, count, sink);
}
