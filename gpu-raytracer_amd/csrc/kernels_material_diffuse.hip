// kernels_material_diffuse.hip -- the material kernels of the row `diffuse` of RT_MATERIAL_KERNEL_LIST (rt_material.h): eight variants, two forms.
// Replaces kernel_material_diffuse of the reference (CUDA/Pathtracer.cu:557-757).
#define RT_MATERIAL_ROW_diffuse(...) __VA_ARGS__
#include "rt_material.h"
RT_MATERIAL_UNIT(diffuse)
