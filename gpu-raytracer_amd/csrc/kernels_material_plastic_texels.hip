// kernels_material_plastic_texels.hip -- the material kernels of the row `plastic _texels` of RT_MATERIAL_KERNEL_LIST (rt_material.h): eight variants,
// two forms. The plastic kernels while no texture on the device holds compressed blocks.
#define RT_MATERIAL_ROW_plastic_texels(...) __VA_ARGS__
#include "rt_material.h"
RT_MATERIAL_UNIT(plastic_texels)
