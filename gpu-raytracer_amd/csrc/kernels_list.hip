// kernels_list.hip -- the generate step of submissions over a pixel list (rt_set_pixel_list). A unit of its own so that the units of the
// kernels that existed before it keep their code objects to the byte of every instruction (profiles/adaptive_sampling_resources.txt).
#include "rt_surface.h"   // RT_SHADE_BLOCK
#include "rt_camera.h"

// kernel_generate_stream of kernels_generate.hip over a pixel list (rt_set_pixel_list): queue entry i of sample s takes pixel list[i] = x + y * screen_width, the third mapping of the domain
// rt_map_pixel maps. The list is in patch order already (64 consecutive entries of an unclipped cell cover an 8 x 8 patch). camera_generate_ray gets what a
// uniform submission of the same first sample passes for the pixel: its primary ray and all its random numbers are those of uniform rendering.
__global__ void __launch_bounds__(RT_SHADE_BLOCK) kernel_generate_stream_list(RtParams p, int sample_index, const unsigned * __restrict__ list, int pixel_count, int slot_base, int queue_offset) {
	const int ray_count = pixel_count * p.batch_samples;
	const RtTraceBuffer & out = p.trace[p.stream_iteration & 1];
	const int base = p.stream->trace_count[p.stream_iteration & 1] + queue_offset;
	for (int index = blockIdx.x * blockDim.x + threadIdx.x; index < ray_count; index += gridDim.x * blockDim.x) {
		int sample_in_batch = index / pixel_count;
		int index_offset = int(list[index - sample_in_batch * pixel_count]);
		int x = index_offset % p.screen_width;
		int y = index_offset / p.screen_width;
		int pixel_index = x + y * p.screen_pitch;
		unsigned slot = unsigned(slot_base + sample_in_batch);
		unsigned virtual_pixel = slot * p.frame_pixels + unsigned(pixel_index);

		f3 origin, direction;
		camera_generate_ray(p, int(virtual_pixel), sample_index + sample_in_batch - int(slot), x, y, origin, direction, sample_index + sample_in_batch); // random_sample adds the slot back

		store3(out.origin,    base + index, origin);
		store3(out.direction, base + index, direction);
		out.pixel_index_and_flags[base + index] = virtual_pixel;
	}
}

void rt_launch_generate_stream_list(const RtParams & p, int sample_index, const unsigned * list, int pixel_count, int slot_base, int queue_offset, hipStream_t stream) {
	int blocks = (pixel_count * p.batch_samples + RT_SHADE_BLOCK - 1) / RT_SHADE_BLOCK;   // capped and grid-strided, as the other streaming launches
	if (blocks < 1) blocks = 1;
	if (blocks > 2048) blocks = 2048;
	hipLaunchKernelGGL(kernel_generate_stream_list, dim3(blocks), dim3(RT_SHADE_BLOCK), 0, stream, p, sample_index, list, pixel_count, slot_base, queue_offset);
}
