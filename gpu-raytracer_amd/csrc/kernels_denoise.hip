// kernels_denoise.hip -- the still-image denoiser: a variance-guided a-trous filter on the accumulated frame. Three kernels:
//   prepare   (C, moments, A, N, P) -> (I, v) = (demodulated colour, variance of the mean's luminance) and the guide (n, z)
//   pass k    one a-trous pass of step 2^k on (I, v) under the guide, tiled in LDS (kernel_denoise_pass_tiled) or plain (kernel_denoise_pass)
//   finalize  (I, v) -> (I * a, v); the LAST pass does this in registers, the kernel of its own runs with 0 iterations only
// Same contract as the other image kernels: -ffp-contract=off, every operation a plain IEEE
// float32 one in the order written, except the weight's log2 / exp2 / rcp, which are the hardware's (1 ulp each), as in edge_stopping_weights
// of kernels_post.hip, whose form the weight below has.
#include "rt_shading.h"

#define RT_DENOISE_BLOCK_X 64
#define RT_DENOISE_BLOCK_Y 4
#define RT_DENOISE_EPSILON 1e-8f
#ifndef RT_DENOISE_ROWS
#define RT_DENOISE_ROWS 8   // rows of pixels per workgroup (one wave each) of the tiled passes up to step 16; 4 at step 32
#endif

// Pixel of this thread in the untiled kernels: tiles of 64 x 4 pixels, row-major, in XCD bands (xcd_tile of rt_shading.h has the reasons); false for a
// padding workgroup and outside the image.
RT_DEV bool denoise_tile_pixel(const RtDenoiseArgs & a, int & x, int & y) {
	const unsigned tiles_x = (unsigned(a.pitch) + RT_DENOISE_BLOCK_X - 1) / RT_DENOISE_BLOCK_X;
	const unsigned tiles_y = (unsigned(a.height) + RT_DENOISE_BLOCK_Y - 1) / RT_DENOISE_BLOCK_Y;
	const unsigned tiles = tiles_x * tiles_y, tile = xcd_tile();
	if (tile >= tiles) return false;
	x = int(tile % tiles_x) * RT_DENOISE_BLOCK_X + int(threadIdx.x);
	y = int(tile / tiles_x) * RT_DENOISE_BLOCK_Y + int(threadIdx.y);
	return x < a.width && y < a.height;
}
static unsigned denoise_grid(const RtDenoiseArgs & a) {
	const unsigned tiles = ((unsigned(a.pitch) + RT_DENOISE_BLOCK_X - 1) / RT_DENOISE_BLOCK_X) * ((unsigned(a.height) + RT_DENOISE_BLOCK_Y - 1) / RT_DENOISE_BLOCK_Y);
	return xcd_tile_grid(tiles);
}

// A guide is a surface's exactly when its normal is not the zero vector (a surface's is a unit vector).
RT_DEV bool guide_is_surface(float4 g) { return g.x != 0.0f || g.y != 0.0f || g.z != 0.0f; }

// ---- prepare --------------------------------------------------------------------------------------------------------
// What the images hold for a pixel that is not a surface: iv = (C, 0) and guide (0, 0, 0, 0) when it is valid, iv = (fallback.rgb, 0) and guide
// (0, 0, 0, -1) when it is not. No pass taps such a pixel or reads its z (both ask guide_is_surface first); its v = 0 enters its neighbours' variance blur
// as the definition says; the -1 is how the finalize step, which copies iv, tells the two apart.
__global__ void __launch_bounds__(256) kernel_denoise_prepare(RtDenoiseArgs a, RtDenoiseImages im) {
	int x, y;
	if (!denoise_tile_pixel(a, x, y)) return;
	const int pixel_index = x + y * a.pitch;
	const float4 c = im.colour[pixel_index], m = im.moments[pixel_index], al = im.albedo[pixel_index], nr = im.normal[pixel_index], ps = im.position[pixel_index];
	const bool valid = m.w >= 2.0f && fabsf(m.w) < __builtin_huge_valf() && finite3(c) && finite3(m) && finite3(al) && finite3(nr) && finite3(ps);
	raise_any_valid(im.any_valid, valid);
	const float nn = nr.x * nr.x + nr.y * nr.y + nr.z * nr.z;
	if (!(valid && nn >= 0.25f)) {
		if (valid) { im.iv[0][pixel_index] = make_float4(c.x, c.y, c.z, 0.0f); im.guide[pixel_index] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
		else { const float4 fb = im.fallback[pixel_index]; im.iv[0][pixel_index] = make_float4(fb.x, fb.y, fb.z, 0.0f); im.guide[pixel_index] = make_float4(0.0f, 0.0f, 0.0f, -1.0f); }
		return;
	}
	const f3 alb = mk3(fmaxf(al.x, a.albedo_floor), fmaxf(al.y, a.albedo_floor), fmaxf(al.z, a.albedo_floor));
	const float pairs = m.w * (m.w - 1.0f);
	const f3 var = mk3(m.x / pairs / (alb.x * alb.x), m.y / pairs / (alb.y * alb.y), m.z / pairs / (alb.z * alb.z));
	const float sd = luminance(safe_sqrt(var.x), safe_sqrt(var.y), safe_sqrt(var.z));   // (an M2 that rounding left below 0 counts as 0)
	const float inv = 1.0f / sqrtf(nn);
	const f3 d = mk3(ps.x - a.eye[0], ps.y - a.eye[1], ps.z - a.eye[2]);
	im.iv[0][pixel_index] = make_float4(c.x / alb.x, c.y / alb.y, c.z / alb.z, sd * sd);
	im.guide[pixel_index] = make_float4(nr.x * inv, nr.y * inv, nr.z * inv, length(d));
}

// ---- the pass -------------------------------------------------------------------------------------------------------
// What a pixel reads of its IMMEDIATE neighbours, whatever the step: the 3 x 3 blur of v (neighbours clamped to the image, as svgf_atrous_neighbourhood)
// and the depth gradient -- per axis the forward difference of z where that neighbour is inside the image and a surface, else the backward one, else 0.
// Global loads, issued by the tiled kernel before its barrier.
struct DenoiseNear { float vb, grad_x, grad_y; float4 guide; };
RT_DEV float denoise_gradient(const float4 * __restrict__ guide, float z, int forward, bool forward_inside, int backward, bool backward_inside) {
	if (forward_inside) { const float4 g = guide[forward]; if (guide_is_surface(g)) return g.w - z; }
	if (backward_inside) { const float4 g = guide[backward]; if (guide_is_surface(g)) return z - g.w; }
	return 0.0f;
}
RT_DEV DenoiseNear denoise_near(const RtDenoiseArgs & a, int x, int y, const float4 * __restrict__ iv_in, const float4 * __restrict__ guide) {
	const int pitch = a.pitch;
	const int xl = max(x - 1, 0), xr = min(x + 1, a.width - 1), yu = max(y - 1, 0), yd = min(y + 1, a.height - 1);
	const int col[3] = { xl, x, xr }, row[3] = { yu * pitch, y * pitch, yd * pitch };
	DenoiseNear n;
	n.vb = 0.0f;
	#pragma unroll
	for (int j = 0; j < 3; j++) {
		#pragma unroll
		for (int i = 0; i < 3; i++) {
			const float kernel_weight = (i == 1 ? 0.5f : 0.25f) * (j == 1 ? 0.5f : 0.25f);
			n.vb += iv_in[col[i] + row[j]].w * kernel_weight;
		}
	}
	const int pixel_index = x + y * pitch;
	n.guide = guide[pixel_index];
	n.grad_x = 0.0f; n.grad_y = 0.0f;
	if (guide_is_surface(n.guide)) {
		n.grad_x = denoise_gradient(guide, n.guide.w, pixel_index + 1, x + 1 < a.width, pixel_index - 1, x >= 1);
		n.grad_y = denoise_gradient(guide, n.guide.w, pixel_index + pitch, y + 1 < a.height, pixel_index - pitch, y >= 1);
	}
	return n;
}

RT_DEV float denoise_log2(float x) { return __builtin_amdgcn_logf(x); }
RT_DEV float denoise_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
RT_DEV float denoise_rcp(float x)  { return __builtin_amdgcn_rcpf(x); }

// The pass's arithmetic for one pixel, shared by the two kernels below: `tap_iv / tap_g (i, j)` return (I, v) and the guide of the pixel at
// (x + i * step, y + j * step), i, j in {-1, 0, 1} -- read from the images by one kernel, from the workgroup's LDS tiles by the other; the centre's guide comes
// with `near`. FINAL: the filter's last pass; the result goes to `out` as (I * a, v), a the floored albedo, instead of to iv_out.
template<bool FINAL, typename TapIV, typename TapG>
RT_DEV void denoise_pass_pixel(const RtDenoiseArgs & a, int x, int y, int step, const DenoiseNear & near, float4 * __restrict__ target, const float4 * __restrict__ albedo,
                               TapIV tap_iv, TapG tap_g) {
	const int pixel_index = x + y * a.pitch;
	const f4 c = mk4(tap_iv(0, 0));
	if (!guide_is_surface(near.guide)) {   // copied; an invalid pixel leaves the filter with .w = -1
		target[pixel_index] = make_float4(c.x, c.y, c.z, FINAL && near.guide.w < 0.0f ? -1.0f : c.w);
		return;
	}
	const float log2_e = 1.44269504088896340736f;
	const float denom = 1.0f / sqrtf(a.sigma_l * a.sigma_l * fmaxf(0.0f, near.vb) + RT_DENOISE_EPSILON);
	const float cl = luminance(c.x, c.y, c.z);
	const f3 cn = mk3(near.guide.x, near.guide.y, near.guide.z);
	const float cz = near.guide.w, z_floor = a.depth_floor * cz;
	const bool in_x[3] = { x - step >= 0, true, x + step < a.width };
	const bool in_y[3] = { y - step >= 0, true, y + step < a.height };
	float sw = 1.0f;
	f4 sc = c;
	#pragma unroll
	for (int j = -1; j <= 1; j++) {
		#pragma unroll
		for (int i = -1; i <= 1; i++) {
			if (i == 0 && j == 0) continue;
			if (in_x[i + 1] && in_y[j + 1]) {
				const float4 g = tap_g(i, j);
				if (guide_is_surface(g)) {
					const f4 t = mk4(tap_iv(i, j));
					const float kernel_weight = (i == 0 ? 1.0f : 0.5f) * (j == 0 ? 1.0f : 0.5f);
					const float d = near.grad_x * float(i * step) + near.grad_y * float(j * step);
					const float ln_w_z = fabsf(cz - g.w) * denoise_rcp(a.sigma_z * fmaxf(fabsf(d), z_floor) + RT_DENOISE_EPSILON);
					const float n_dot_n = fmaxf(0.0f, dot(cn, mk3(g.x, g.y, g.z)));
					// pow(0, sigma_n) = 0 for sigma_n > 0 and 1 for sigma_n = 0; log2(0) = -inf does the first, the second needs the select
					const float log2_w_n = (n_dot_n > 0.0f || a.sigma_n > 0.0f) ? a.sigma_n * denoise_log2(n_dot_n) : 0.0f;
					const float w = kernel_weight * denoise_exp2(log2_w_n - (fabsf(cl - luminance(t.x, t.y, t.z)) * denom + ln_w_z) * log2_e);
					sw += w;
					sc += mk4(w, w, w, w * w) * t;
				}
			}
		}
	}
	const float inv = 1.0f / sw;
	sc *= inv;
	sc.w *= inv;
	if (FINAL) {
		const float4 al = albedo[pixel_index];
		sc = mk4(sc.x * fmaxf(al.x, a.albedo_floor), sc.y * fmaxf(al.y, a.albedo_floor), sc.z * fmaxf(al.z, a.albedo_floor), sc.w);
	}
	target[pixel_index] = to_float4(sc);
}

template<bool FINAL>
__global__ void __launch_bounds__(256) kernel_denoise_pass(RtDenoiseArgs a, const float4 * __restrict__ iv_in, const float4 * __restrict__ guide, float4 * __restrict__ target,
                                                           const float4 * __restrict__ albedo, int step) {
	int x, y;
	if (!denoise_tile_pixel(a, x, y)) return;
	const int pitch = a.pitch, pixel_index = x + y * pitch;
	denoise_pass_pixel<FINAL>(a, x, y, step, denoise_near(a, x, y, iv_in, guide), target, albedo,
		[&](int i, int j) { return iv_in[pixel_index + i * step + j * step * pitch]; },
		[&](int i, int j) { return guide[pixel_index + i * step + j * step * pitch]; });
}

// The same pass with the two tapped images of a workgroup staged in LDS, on the pattern of kernel_svgf_atrous_tiled (kernels_post.hip, where the reasons are
// written down): a workgroup's TY rows of pixels are STEP rows apart, its columns are 64 adjacent pixels plus STEP on either side, so a tile of
// (64 + 2 STEP) x (TY + 2) positions of 32 B holds every tap; tiles are numbered column-fastest within one residue class of rows and XCD k takes the k-th
// eighth of the sequence. Same arithmetic per pixel (denoise_pass_pixel): bit-identical to the plain pass.
template<int STEP, int TY, bool FINAL>
__global__ void __launch_bounds__(64 * TY) kernel_denoise_pass_tiled(RtDenoiseArgs a, const float4 * __restrict__ iv_in, const float4 * __restrict__ guide, float4 * __restrict__ target,
                                                                     const float4 * __restrict__ albedo) {
	constexpr int W = 64 + 2 * STEP, ROWS = TY + 2, N = W * ROWS, THREADS = 64 * TY;
	__shared__ float4 tile_iv[N], tile_g[N];
	const unsigned tiles_x = (unsigned(a.width) + 63u) / 64u;
	const unsigned blocks_y = (unsigned(a.height) + unsigned(TY * STEP) - 1u) / unsigned(TY * STEP);
	const unsigned tiles = tiles_x * unsigned(STEP) * blocks_y, tile = xcd_tile();
	if (tile >= tiles) return;   // (the whole workgroup: no barrier is left waiting)
	const int x0 = int(tile % tiles_x) * 64;
	const unsigned above = tile / tiles_x;
	const int y_base = int(above / unsigned(STEP)) * (TY * STEP) + int(above % unsigned(STEP));
	const int pitch = a.pitch;

	// this thread's pixel, and what it needs of its immediate neighbours (global loads: issued before the staging loop, they land with it)
	const int tx = int(threadIdx.x) & 63, ty = int(threadIdx.x) >> 6;
	const int x = x0 + tx, y = y_base + STEP * ty;
	const bool has_pixel = x < a.width && y < a.height;
	DenoiseNear near = { 0.0f, 0.0f, 0.0f, make_float4(0.0f, 0.0f, 0.0f, 0.0f) };
	if (has_pixel) near = denoise_near(a, x, y, iv_in, guide);

	// stage: row r of the tile is image row y_base + STEP * (r - 1), column c is image column x0 - STEP + c. Positions outside the image are never
	// tapped (in_x / in_y of denoise_pass_pixel); they are filled from the clamped position so that every load is inside the images.
	for (int pos = int(threadIdx.x); pos < N; pos += THREADS) {
		const int c = pos % W, r = pos / W;
		const int gx = min(max(x0 - STEP + c, 0), a.width - 1), gy = min(max(y_base + STEP * (r - 1), 0), a.height - 1);
		const int source = gx + gy * pitch;
		tile_iv[pos] = iv_in[source]; tile_g[pos] = guide[source];
	}
	__syncthreads();

	if (!has_pixel) return;
	const int centre = (ty + 1) * W + tx + STEP;
	denoise_pass_pixel<FINAL>(a, x, y, STEP, near, target, albedo,
		[&](int i, int j) { return tile_iv[centre + i * STEP + j * W]; },
		[&](int i, int j) { return tile_g [centre + i * STEP + j * W]; });
}

// ---- finalize (0 iterations) ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) kernel_denoise_finalize(RtDenoiseArgs a, const float4 * __restrict__ iv_in, const float4 * __restrict__ guide, float4 * __restrict__ out,
                                                               const float4 * __restrict__ albedo) {
	int x, y;
	if (!denoise_tile_pixel(a, x, y)) return;
	const int pixel_index = x + y * a.pitch;
	const float4 c = iv_in[pixel_index], g = guide[pixel_index];
	if (!guide_is_surface(g)) { out[pixel_index] = make_float4(c.x, c.y, c.z, g.w < 0.0f ? -1.0f : c.w); return; }
	const float4 al = albedo[pixel_index];
	out[pixel_index] = make_float4(c.x * fmaxf(al.x, a.albedo_floor), c.y * fmaxf(al.y, a.albedo_floor), c.z * fmaxf(al.z, a.albedo_floor), c.w);
}

// ---- launchers ------------------------------------------------------------------------------------------------------
template<int STEP, int TY>
static void launch_denoise_tiled(const RtDenoiseArgs & a, bool final_pass, const float4 * iv_in, const float4 * guide, float4 * target, const float4 * albedo, hipStream_t stream) {
	const unsigned tiles = ((unsigned(a.width) + 63u) / 64u) * unsigned(STEP) * ((unsigned(a.height) + unsigned(TY * STEP) - 1u) / unsigned(TY * STEP));
	if (final_pass) hipLaunchKernelGGL((kernel_denoise_pass_tiled<STEP, TY, true>), dim3(xcd_tile_grid(tiles)), dim3(64 * TY), 0, stream, a, iv_in, guide, target, albedo);
	else hipLaunchKernelGGL((kernel_denoise_pass_tiled<STEP, TY, false>), dim3(xcd_tile_grid(tiles)), dim3(64 * TY), 0, stream, a, iv_in, guide, target, albedo);
}
static void launch_denoise_tiled_step(const RtDenoiseArgs & a, int step, bool final_pass, const float4 * iv_in, const float4 * guide, float4 * target, const float4 * albedo, hipStream_t stream) {
	switch (step) {   // LDS per workgroup: (64 + 2 STEP) x (TY + 2) x 32 B = 21.1 / 21.8 / 23.0 / 25.6 / 30.7 / 24.6 KB with 8 rows (4 at step 32)
		case 1:  launch_denoise_tiled<1,  RT_DENOISE_ROWS>(a, final_pass, iv_in, guide, target, albedo, stream); return;
		case 2:  launch_denoise_tiled<2,  RT_DENOISE_ROWS>(a, final_pass, iv_in, guide, target, albedo, stream); return;
		case 4:  launch_denoise_tiled<4,  RT_DENOISE_ROWS>(a, final_pass, iv_in, guide, target, albedo, stream); return;
		case 8:  launch_denoise_tiled<8,  RT_DENOISE_ROWS>(a, final_pass, iv_in, guide, target, albedo, stream); return;
		case 16: launch_denoise_tiled<16, RT_DENOISE_ROWS>(a, final_pass, iv_in, guide, target, albedo, stream); return;
		default: launch_denoise_tiled<32, 4>(a, final_pass, iv_in, guide, target, albedo, stream); return;
	}
}

void rt_launch_denoise(const RtDenoiseArgs & a, const RtDenoiseImages & im, bool tiled, hipStream_t stream, void (*mark)(void * user, int kernel, hipStream_t stream), void * user) {
	const dim3 block(RT_DENOISE_BLOCK_X, RT_DENOISE_BLOCK_Y);
	const unsigned grid = denoise_grid(a);
	int kernel = 0;
	if (mark) mark(user, kernel, stream);
	hipLaunchKernelGGL(kernel_denoise_prepare, dim3(grid), block, 0, stream, a, im);
	if (mark) mark(user, ++kernel, stream);
	if (a.iterations == 0) {
		hipLaunchKernelGGL(kernel_denoise_finalize, dim3(grid), block, 0, stream, a, (const float4 *)im.iv[0], (const float4 *)im.guide, im.out, im.albedo);
		if (mark) mark(user, ++kernel, stream);
		return;
	}
	for (int k = 0; k < a.iterations; k++) {
		const bool final_pass = k == a.iterations - 1;
		const float4 * iv_in = im.iv[k & 1];
		float4 * target = final_pass ? im.out : im.iv[(k & 1) ^ 1];
		if (tiled) launch_denoise_tiled_step(a, 1 << k, final_pass, iv_in, im.guide, target, im.albedo, stream);
		else if (final_pass) hipLaunchKernelGGL(kernel_denoise_pass<true>, dim3(grid), block, 0, stream, a, iv_in, (const float4 *)im.guide, target, im.albedo, 1 << k);
		else hipLaunchKernelGGL(kernel_denoise_pass<false>, dim3(grid), block, 0, stream, a, iv_in, (const float4 *)im.guide, target, im.albedo, 1 << k);
		if (mark) mark(user, ++kernel, stream);
	}
}
