// kernels_fog.hip -- the fog volume's own launches: the attenuation pass of the shadow queue, the probes of the segment step, and the
// brick table of a density grid. (The scatter events themselves live in the ..._fog and ..._fog_grid instances of the sort kernels, kernels_sort.hip.)
#include "rt_fog_grid.h"

#define RT_FOG_BLOCK 256

// Every shadow ray of a queue is multiplied by exp(-sigma_t * clipped length): rays from a surface and from a scatter vertex alike, rays to infinity
// (the sky, directional lights) over their finite part inside the box. Runs after the material launches of a bounce or iteration and before the queue is
// traced. Grid-stride; the count is read from device memory (no host round trip in the merged wavefront); the only stores are to `illumination`,
// and a ray that does not cross the box is not stored at all. The pixel word travels in the same float4 and is written back as loaded.
// GRID (the ..._grid kernels, while a density grid is in force): exp(-sigma_t * D) with the density length D of the voxel march (rt_fog_grid.h); a ray that
// meets no density is not stored.
template<bool GRID = false>
RT_DEV void fog_attenuate_shadows(const RtParams & p, const int * count_word) {
	const int count = *count_word;
	const FogVolume fog = fog_volume(p);
	if constexpr (GRID) {
		const FogGrid grid = fog_grid(p, fog);
		for (int index = blockIdx.x * blockDim.x + threadIdx.x; index < count; index += gridDim.x * blockDim.x) {
			f3 origin = load3(p.shadow.origin, index), direction = load3(p.shadow.direction, index);
			f3 transmittance;
			if (!fog_grid_transmittance(fog, grid, origin, direction, p.shadow.max_distance[index], transmittance)) continue;
			float4 v = p.shadow.illumination_and_pixel_index[index];
			v.x *= transmittance.x; v.y *= transmittance.y; v.z *= transmittance.z;
			p.shadow.illumination_and_pixel_index[index] = v;
		}
		return;
	}
	for (int index = blockIdx.x * blockDim.x + threadIdx.x; index < count; index += gridDim.x * blockDim.x) {
		f3 origin = load3(p.shadow.origin, index), direction = load3(p.shadow.direction, index);
		float t0, t1;
		if (!fog_clip(fog, origin, direction, p.shadow.max_distance[index], t0, t1)) continue;
		f3 transmittance = beer_lambert(fog.sigma_a + fog.sigma_s, t1 - t0);
		float4 v = p.shadow.illumination_and_pixel_index[index];
		v.x *= transmittance.x; v.y *= transmittance.y; v.z *= transmittance.z;
		p.shadow.illumination_and_pixel_index[index] = v;
	}
}
__global__ void __launch_bounds__(RT_FOG_BLOCK) kernel_fog_attenuate_shadows(RtParams p, int bounce) { fog_attenuate_shadows(p, &p.sizes->shadow[bounce]); }
__global__ void __launch_bounds__(RT_FOG_BLOCK) kernel_fog_attenuate_shadows_stream(RtParams p) { fog_attenuate_shadows(p, &p.stream->shadow_count[p.stream_iteration & 1]); }
__global__ void __launch_bounds__(RT_FOG_BLOCK) kernel_fog_attenuate_shadows_grid(RtParams p, int bounce) { fog_attenuate_shadows<true>(p, &p.sizes->shadow[bounce]); }
__global__ void __launch_bounds__(RT_FOG_BLOCK) kernel_fog_attenuate_shadows_stream_grid(RtParams p) { fog_attenuate_shadows<true>(p, &p.stream->shadow_count[p.stream_iteration & 1]); }

// rt_fog_segments: the segment step of the ..._fog sort instances on explicit segments, through the same device functions. Records: gpu_raytracer_amd.h.
__global__ void kernel_fog_segments(RtParams p, const uint32_t * probes, int count, uint32_t * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const uint32_t * a = probes + size_t(i) * RT_FOG_SEGMENT_IN;
	uint32_t * o = out + size_t(i) * RT_FOG_SEGMENT_OUT;
	auto f = [&](int k) { return __uint_as_float(a[k]); };
	f3 origin = mk3(f(0), f(1), f(2)), direction = mk3(f(3), f(4), f(5));
	float t_end = f(6);
	f3 throughput = mk3(f(10), f(11), f(12));
	const bool inside_medium = a[13] != 0;
	const FogVolume fog = fog_volume(p);
	f2 rand = fog_random_pair(random_path(p, a[7], a[9]), a[8]);
	float t0 = 0.0f, t1 = 0.0f, distance = RT_INFINITY; bool scattered = false;
	f3 vertex = mk3(0.0f);
	if (!inside_medium && fog_clip(fog, origin, direction, t_end, t0, t1)) {
		scattered = fog_sample_distance(fog, rand, t1 - t0, throughput, distance);
		if (scattered) vertex = origin + (t0 + distance) * direction;
	} else { t0 = 0.0f; t1 = 0.0f; }
	o[0] = __float_as_uint(t0); o[1] = __float_as_uint(t1); o[2] = __float_as_uint(rand.x); o[3] = __float_as_uint(rand.y);
	o[4] = scattered ? 1u : 0u; o[5] = __float_as_uint(distance);
	o[6] = __float_as_uint(throughput.x); o[7] = __float_as_uint(throughput.y); o[8] = __float_as_uint(throughput.z);
	o[9] = __float_as_uint(vertex.x); o[10] = __float_as_uint(vertex.y); o[11] = __float_as_uint(vertex.z);
	o[12] = o[13] = o[14] = o[15] = 0u;
}

// rt_fog_density_segments: the segment step of the ..._fog_grid sort instances on rt_fog_segments' records; words 12..14: the density length (over the
// whole clipped interval, or up to the vertex of a path that scattered), the voxels read, the empty bricks crossed.
__global__ void kernel_fog_density_segments(RtParams p, const uint32_t * probes, int count, uint32_t * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const uint32_t * a = probes + size_t(i) * RT_FOG_SEGMENT_IN;
	uint32_t * o = out + size_t(i) * RT_FOG_SEGMENT_OUT;
	auto f = [&](int k) { return __uint_as_float(a[k]); };
	f3 origin = mk3(f(0), f(1), f(2)), direction = mk3(f(3), f(4), f(5));
	float t_end = f(6);
	f3 throughput = mk3(f(10), f(11), f(12));
	const bool inside_medium = a[13] != 0;
	const FogVolume fog = fog_volume(p);
	const FogGrid grid = fog_grid(p, fog);
	f2 rand = fog_random_pair(random_path(p, a[7], a[9]), a[8]);
	float t0 = 0.0f, t1 = 0.0f, distance = RT_INFINITY, t_scatter = RT_INFINITY, density_length = 0.0f; bool scattered = false;
	int steps[2] = { 0, 0 };
	f3 vertex = mk3(0.0f);
	if (!inside_medium && fog_clip(fog, origin, direction, t_end, t0, t1)) {
		scattered = fog_grid_sample_distance<true>(fog, grid, rand, origin, direction, t0, t1, throughput, distance, t_scatter, density_length, steps);
		if (scattered) vertex = origin + t_scatter * direction;
	} else { t0 = 0.0f; t1 = 0.0f; }
	o[0] = __float_as_uint(t0); o[1] = __float_as_uint(t1); o[2] = __float_as_uint(rand.x); o[3] = __float_as_uint(rand.y);
	o[4] = scattered ? 1u : 0u; o[5] = __float_as_uint(distance);
	o[6] = __float_as_uint(throughput.x); o[7] = __float_as_uint(throughput.y); o[8] = __float_as_uint(throughput.z);
	o[9] = __float_as_uint(vertex.x); o[10] = __float_as_uint(vertex.y); o[11] = __float_as_uint(vertex.z);
	o[12] = __float_as_uint(density_length); o[13] = uint32_t(steps[0]); o[14] = uint32_t(steps[1]); o[15] = 0u;
}

// The brick table of a grid: one workgroup per brick of RT_FOG_BRICK^3 voxels (edge bricks are partial), 256 threads over its 512 voxels; byte 1 where any
// voxel holds density. The empty bricks are counted for rt_get_fog_density_info.
__global__ void __launch_bounds__(256) kernel_fog_mark_bricks(const float * density, int nx, int ny, int nz, int nbx, int nby, unsigned char * bricks, int * empty_count) {
	const int brick = blockIdx.x, bx = brick % nbx, by = (brick / nbx) % nby, bz = brick / (nbx * nby);
	bool any = false;
	for (int v = threadIdx.x; v < RT_FOG_BRICK * RT_FOG_BRICK * RT_FOG_BRICK; v += blockDim.x) {
		const int x = bx * RT_FOG_BRICK + (v & 7), y = by * RT_FOG_BRICK + ((v >> 3) & 7), z = bz * RT_FOG_BRICK + (v >> 6);
		if (x < nx && y < ny && z < nz) any = any || density[(size_t(z) * ny + y) * nx + x] > 0.0f;
	}
	const int some = __syncthreads_or(any ? 1 : 0);
	if (threadIdx.x == 0) { bricks[brick] = some ? 1 : 0; if (!some) atomicAdd(empty_count, 1); }
}

// (the grids: what the queue can hold is not known on the host in the merged wavefront; 1024 workgroups stride over whatever the count word says)
void rt_launch_fog_attenuate_shadows(const RtParams & p, int bounce, hipStream_t stream) {
	hipLaunchKernelGGL(p.fog_grid ? kernel_fog_attenuate_shadows_grid : kernel_fog_attenuate_shadows, dim3(1024), dim3(RT_FOG_BLOCK), 0, stream, p, bounce);
}
void rt_launch_fog_attenuate_shadows_stream(const RtParams & p, hipStream_t stream) {
	hipLaunchKernelGGL(p.fog_grid ? kernel_fog_attenuate_shadows_stream_grid : kernel_fog_attenuate_shadows_stream, dim3(1024), dim3(RT_FOG_BLOCK), 0, stream, p);
}
void rt_launch_fog_segments(const RtParams & p, const uint32_t * probes, int count, uint32_t * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_fog_segments, dim3((count + 255) / 256), dim3(256), 0, stream, p, probes, count, out);
}
void rt_launch_fog_density_segments(const RtParams & p, const uint32_t * probes, int count, uint32_t * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_fog_density_segments, dim3((count + 255) / 256), dim3(256), 0, stream, p, probes, count, out);
}
void rt_launch_fog_mark_bricks(const float * density, int nx, int ny, int nz, unsigned char * bricks, int * empty_count, hipStream_t stream) {
	const int nbx = (nx + RT_FOG_BRICK - 1) / RT_FOG_BRICK, nby = (ny + RT_FOG_BRICK - 1) / RT_FOG_BRICK, nbz = (nz + RT_FOG_BRICK - 1) / RT_FOG_BRICK;
	hipLaunchKernelGGL(kernel_fog_mark_bricks, dim3(nbx * nby * nbz), dim3(256), 0, stream, density, nx, ny, nz, nbx, nby, bricks, empty_count);
}
