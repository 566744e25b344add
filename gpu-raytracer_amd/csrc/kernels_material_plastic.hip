// kernels_material_plastic.hip -- the material kernels of the row `plastic` of RT_MATERIAL_KERNEL_LIST (rt_material.h): eight variants, two forms.
// Replaces kernel_material_plastic of the reference (CUDA/Pathtracer.cu:557-757).
#define RT_MATERIAL_ROW_plastic(...) __VA_ARGS__
#include "rt_material.h"
RT_MATERIAL_UNIT(plastic)
