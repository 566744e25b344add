// kernels_material.hip -- the selector and the two launchers of the material launch. The kernels are compiled row by row
// (kernels_material_{diffuse,plastic,dielectric,conductor,diffuse_texels,plastic_texels}.hip) from the one list in rt_material.h; this unit holds none.
#include "rt_material.h"

// What the material launchers launch for a slot (0 .. 3)
static const MaterialKernels & material_kernels_for(const RtParams & p, int material_slot) {
	#define RT_MATERIAL_ROW_TABLE(MATERIAL, TEXELS, ...) rt_material_kernels_##MATERIAL##TEXELS,
	static const MaterialKernels * (* const rows[])() = { RT_MATERIAL_KERNEL_LIST(RT_MATERIAL_ROW_TABLE, ) };
	#undef RT_MATERIAL_ROW_TABLE
	const int variant = (p.normal_map_slots >> material_slot & 1) * 4 + rt_light_split(p);
	const int row = material_slot < 2 && !p.textures_compressed ? 4 + material_slot : material_slot;
	return rows[row]()[variant];
}
void rt_launch_material(const RtParams & p, int material_slot, int bounce, int sample_index, hipStream_t stream) {
	hipLaunchKernelGGL(material_kernels_for(p, material_slot).bounce, dim3(2048), dim3(RT_SHADE_BLOCK), 0, stream, p, bounce, sample_index);
}
void rt_launch_material_stream(const RtParams & p, int material_slot, hipStream_t stream) {
	hipLaunchKernelGGL(material_kernels_for(p, material_slot).merged, dim3(RT_STREAM_SHADE_GRID), dim3(RT_SHADE_BLOCK), 0, stream, p);
}
