// kernels_material_diffuse_texels.hip -- the material kernels of the row `diffuse _texels` of RT_MATERIAL_KERNEL_LIST (rt_material.h): eight variants,
// two forms. The diffuse kernels while no texture on the device holds compressed blocks.
#define RT_MATERIAL_ROW_diffuse_texels(...) __VA_ARGS__
#include "rt_material.h"
RT_MATERIAL_UNIT(diffuse_texels)
