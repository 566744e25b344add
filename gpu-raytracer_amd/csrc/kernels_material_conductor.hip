// kernels_material_conductor.hip -- the material kernels of the row `conductor` of RT_MATERIAL_KERNEL_LIST (rt_material.h): eight variants, two forms.
// Replaces kernel_material_conductor of the reference (CUDA/Pathtracer.cu:557-757).
#define RT_MATERIAL_ROW_conductor(...) __VA_ARGS__
#include "rt_material.h"
RT_MATERIAL_UNIT(conductor)
