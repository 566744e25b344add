// kernels_sky.hip -- the tables of sky importance sampling (rt_set_sky_sampling) and its test entry points.
//
// One cell per sky texel, in sample_sky's mapping (u = atan2(-z, x) / 2pi + 1/2, v = acos(y) / pi). The weight of a cell is the largest
// luminance among the texels whose bilinear footprint reaches into it -- the 3 x 3 neighbourhood, clamped as clamp_taps clamps -- times
// the cell's solid angle (cos theta_0 - cos theta_1) 2pi / W. sample_sky filters bilinearly, so a black texel beside the sun still returns
// light: the maximum keeps the pdf non-zero wherever the radiance is.
//
// Three launches, no float atomics (the tables are the same to the bit on every run and on every rank of a tile split):
//   kernel_sky_rows      one workgroup per row: cell weights, a block scan in double, the row's normalised CDF; the row total in double
//   kernel_sky_marginal  one workgroup: a block scan of the row totals, the marginal CDF, the total
//   kernel_sky_cell_pdf  every cell: pdf = P_cell / Omega_cell = largest luminance / total
#include "rt_shading.h"

#define RT_SKY_BLOCK 256

// Inclusive scan of one double per thread over the workgroup (Hillis-Steele in LDS: a fixed order of additions).
RT_DEV double block_inclusive_scan(double v, double * lds) {
	lds[threadIdx.x] = v;
	__syncthreads();
	for (int offset = 1; offset < RT_SKY_BLOCK; offset <<= 1) {
		double add = threadIdx.x >= unsigned(offset) ? lds[threadIdx.x - offset] : 0.0;
		__syncthreads();
		v += add;
		lds[threadIdx.x] = v;
		__syncthreads();
	}
	return v;
}
// What lies in front of this thread's span, after block_inclusive_scan: the scan's entry of the thread before. Not `inclusive - sum`: where the span's
// own sum is 2^53 times what lies in front of it (a sun beside a dim texel, both in one span), that difference has no correct digit left and the row's
// CDF steps back at the span's first entry.
RT_DEV double sky_exclusive_prefix(const double * lds) { return threadIdx.x > 0 ? lds[threadIdx.x - 1] : 0.0; }

// Largest luminance over the clamped 3 x 3 neighbourhood of texel (x, y); a NaN anywhere in it makes the result NaN.
RT_DEV float sky_footprint_luminance(const float4 * __restrict__ sky, int width, int height, int x, int y) {
	float m = 0.0f;
	for (int dy = -1; dy <= 1; dy++) {
		int yy = min(max(y + dy, 0), height - 1);
		for (int dx = -1; dx <= 1; dx++) {
			int xx = min(max(x + dx, 0), width - 1);
			float4 t = sky[xx + size_t(yy) * width];
			float l = luminance(t.x, t.y, t.z);
			if (l > m || l != l) m = l;
			if (m != m) return m;
		}
	}
	return m;
}

// Thread t of the workgroup owns the contiguous span [t * per_thread, (t + 1) * per_thread) of the n items.
__global__ void __launch_bounds__(RT_SKY_BLOCK) kernel_sky_rows(const float4 * __restrict__ sky, int width, int height, float * __restrict__ conditional_cdf,
                                                                float * __restrict__ cell_luminance, double * __restrict__ row_total) {
	__shared__ double lds[RT_SKY_BLOCK];
	const int row = blockIdx.x;
	const double pi = 3.14159265358979323846;
	const double omega = (cos(pi * row / height) - cos(pi * (row + 1) / height)) * 2.0 * pi / width;
	const int per_thread = (width + RT_SKY_BLOCK - 1) / RT_SKY_BLOCK;
	const int first = min(int(threadIdx.x) * per_thread, width), last = min(first + per_thread, width);
	float * cdf = conditional_cdf + size_t(row) * width;
	float * lum = cell_luminance + size_t(row) * width;

	double sum = 0.0;
	for (int x = first; x < last; x++) {
		float m = sky_footprint_luminance(sky, width, height, x, row);
		lum[x] = m;
		sum += double(m) * omega;
	}
	block_inclusive_scan(sum, lds);
	const double total = lds[RT_SKY_BLOCK - 1];
	double prefix = sky_exclusive_prefix(lds);
	for (int x = first; x < last; x++) {
		prefix += double(lum[x]) * omega;
		cdf[x] = !(total > 0.0) ? float(x + 1) / float(width) : x == width - 1 ? 1.0f : float(prefix / total);   // (a row without weight is never picked)
	}
	if (threadIdx.x == 0) row_total[row] = total;
}

__global__ void __launch_bounds__(RT_SKY_BLOCK) kernel_sky_marginal(const double * __restrict__ row_total, int height, float * __restrict__ marginal_cdf, double * __restrict__ total_out) {
	__shared__ double lds[RT_SKY_BLOCK];
	const int per_thread = (height + RT_SKY_BLOCK - 1) / RT_SKY_BLOCK;
	const int first = min(int(threadIdx.x) * per_thread, height), last = min(first + per_thread, height);
	double sum = 0.0;
	for (int y = first; y < last; y++) sum += row_total[y];
	block_inclusive_scan(sum, lds);
	const double total = lds[RT_SKY_BLOCK - 1];
	double prefix = sky_exclusive_prefix(lds);
	for (int y = first; y < last; y++) {
		prefix += row_total[y];
		marginal_cdf[y] = !(total > 0.0) ? float(y + 1) / float(height) : y == height - 1 ? 1.0f : float(prefix / total);
	}
	if (threadIdx.x == 0) total_out[0] = total;
}

// in: the largest footprint luminance of every cell; out: its pdf (0 throughout when the total is 0 or not finite: sampling stays off)
__global__ void __launch_bounds__(RT_SKY_BLOCK) kernel_sky_cell_pdf(float * __restrict__ cell, size_t count, const double * __restrict__ total_in) {
	const double total = total_in[0];
	const bool usable = total > 0.0 && total < __builtin_huge_val();
	for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += size_t(gridDim.x) * blockDim.x)
		cell[i] = usable ? float(double(cell[i]) / total) : 0.0f;
}

void rt_launch_sky_build(const float4 * sky, int width, int height, float * marginal_cdf, float * conditional_cdf, float * cell_pdf, double * row_total, double * total, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_sky_rows, dim3(height), dim3(RT_SKY_BLOCK), 0, stream, sky, width, height, conditional_cdf, cell_pdf, row_total);
	hipLaunchKernelGGL(kernel_sky_marginal, dim3(1), dim3(RT_SKY_BLOCK), 0, stream, (const double *)row_total, height, marginal_cdf, total);
	size_t count = size_t(width) * height;
	size_t groups = (count + RT_SKY_BLOCK - 1) / RT_SKY_BLOCK;
	hipLaunchKernelGGL(kernel_sky_cell_pdf, dim3(unsigned(groups < 4096 ? groups : 4096)), dim3(RT_SKY_BLOCK), 0, stream, cell_pdf, count, (const double *)total);
}

// rt_sample_sky_distribution / rt_sky_pdf: the shade kernels' sky_sample_direction and sky_pdf on caller-supplied arguments
__global__ void kernel_sample_sky_distribution(RtParams p, const float * uv, int count, float * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	float pdf;
	f3 d = sky_sample_direction(p, uv[2 * size_t(i)], uv[2 * size_t(i) + 1], pdf);
	float * o = out + 4 * size_t(i);
	o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = pdf;
}
__global__ void kernel_sky_pdf(RtParams p, const float * directions, int count, float * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * d = directions + 3 * size_t(i);
	out[i] = sky_pdf(p, mk3(d[0], d[1], d[2]));
}
void rt_launch_sample_sky_distribution(const RtParams & p, const float * uv, int count, float * out_xyz_pdf, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_sample_sky_distribution, dim3((count + 255) / 256), dim3(256), 0, stream, p, uv, count, out_xyz_pdf);
}
void rt_launch_sky_pdf(const RtParams & p, const float * directions, int count, float * out_pdf, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_sky_pdf, dim3((count + 255) / 256), dim3(256), 0, stream, p, directions, count, out_pdf);
}
