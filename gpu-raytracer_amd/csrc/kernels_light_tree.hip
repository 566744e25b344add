// kernels_light_tree.hip -- the light tree of next-event estimation built ON THE DEVICE (the data structure: rt_light_tree.h).
//   1  leaves   one thread per leaf k = leaf_base[m] + j: the triangle's three vertices through the instance's matrix, their box, the true world area
//               (half the length of the cross product of the transformed edges), the power; the box of all leaves (integer atomics on order-preserving
//               keys, one set per wave, as kernels_blas.hip does); the inverse tables entry_of_mesh and place_of_triangle
//   2  keys     30-bit Morton code of the box centre inside the box of all leaves << 32 | leaf id; ONE radix sort (rocPRIM)
//   3  place    sorted place s -> node M - 1 + s, padding leaves behind them; slot_of_leaf, leaf_of_slot
//   4  levels   bottom up, one launch per level while a level is wider than one workgroup, then ONE workgroup for the levels of 256 nodes and fewer, which
//               it keeps in LDS between its barriers. No workgroup reads, in the launch that wrote it, what another workgroup wrote: stream order is the only
//               hand-off between workgroups (the XCDs' L2s are not coherent with each other inside a launch).
// Every float operation is a single rounded float32 operation in the order written: tests/light_tree_reference.py restates leaves, order and nodes bit for bit.
#include "rt_math.h"
#include "rt_types.h"
#include "rt_tlas_build.h"
#include "rt_light_tree.h"

#include <algorithm>
#include <cstring>   // (rocPRIM's texture iterator calls memset from host code without including it)
#include <rocprim/rocprim.hpp>

#define RT_LIGHT_TREE_BLOCK 256

RT_DEV int light_tree_ordered(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
RT_DEV float light_tree_unordered(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void __launch_bounds__(RT_LIGHT_TREE_BLOCK) kernel_light_tree_begin(LightTreeBuildArgs a) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < a.mesh_count) a.entry_of_mesh[i] = -1;
	if (i < a.triangle_count) a.place_of_triangle[i] = -1;
	if (i < 3) { a.scene_box[i] = light_tree_ordered(3.0e38f); a.scene_box[3 + i] = light_tree_ordered(-3.0e38f); }
}

__global__ void __launch_bounds__(RT_LIGHT_TREE_BLOCK) kernel_light_tree_leaves(LightTreeBuildArgs a) {
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	const bool valid = k < a.leaf_count;
	TlasBox box; tlas_box_empty(box);
	if (valid) {
		int lo = 0, hi = a.light_mesh_count;   // the entry whose range [leaf_base[m], leaf_base[m + 1]) holds leaf k
		while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (a.leaf_base[mid] <= k) lo = mid; else hi = mid; }
		const int entry = lo;
		const int place = a.light_mesh_triangle_span[entry].x + (k - a.leaf_base[entry]);
		const int triangle = a.light_triangle_indices[place];
		int mesh = a.light_mesh_transform_indices[entry];
		if (a.mesh_position) mesh = a.mesh_position[mesh];   // device-built TLAS: the tables name instances by scene index
		float area = 0.0f, power = 0.0f;
		if (triangle >= 0 && triangle < a.triangle_count && mesh >= 0 && mesh < a.mesh_count) {
			const float4 * t = a.triangles + size_t(triangle) * 6;
			const float4 t0 = t[0], t1 = t[1], t2 = t[2];
			const float v[3][3] = { { t0.x, t0.y, t0.z }, { t0.x + t0.w, t0.y + t1.x, t0.z + t1.y }, { t0.x + t1.z, t0.y + t1.w, t0.z + t2.x } };
			const float4 * m = a.mesh_transforms + size_t(mesh) * 3;
			float w[3][3];
			for (int c = 0; c < 3; c++) for (int d = 0; d < 3; d++) {
				const float4 row = m[d];
				w[c][d] = ((row.x * v[c][0] + row.y * v[c][1]) + row.z * v[c][2]) + row.w;
				box.min[d] = fminf(box.min[d], w[c][d]); box.max[d] = fmaxf(box.max[d], w[c][d]);
			}
			const float e1[3] = { w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2] }, e2[3] = { w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2] };
			const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
			area = 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
			const int material = a.mesh_material_ids[mesh];
			if (material >= 0 && material < a.material_count && a.material_types[material] == RT_MATERIAL_LIGHT) {
				const float4 emission = a.materials[2 * size_t(material)];
				power = area * ((0.299f * emission.x + 0.587f * emission.y) + 0.114f * emission.z);
			}
			if (!(area > 0.0f && area <= FLT_MAX && power > 0.0f && power <= FLT_MAX)) power = 0.0f;   // never chosen
			if (!(area <= FLT_MAX)) area = 0.0f;
			atomicMin((unsigned *)&a.entry_of_mesh[mesh], unsigned(entry));          // (-1 is the largest unsigned; two entries on one instance: the lower)
			atomicMin((unsigned *)&a.place_of_triangle[triangle], unsigned(place));
		} else {
			for (int d = 0; d < 3; d++) box.min[d] = box.max[d] = 0.0f;
		}
		a.leaf_nodes[2 * size_t(k)]     = make_float4(box.min[0], box.min[1], box.min[2], power);
		a.leaf_nodes[2 * size_t(k) + 1] = make_float4(box.max[0], box.max[1], box.max[2], 0.0f);
		a.leaves[k] = make_float4(__int_as_float(entry), __int_as_float(triangle), area, power);
	}
	// the box of all leaves: every lane of the wave stays in the reduction, the ones beyond the input hold the empty box
	#pragma unroll
	for (int d = 0; d < 3; d++) {
		float lo = box.min[d], hi = box.max[d];
		for (int offset = 32; offset > 0; offset >>= 1) { lo = fminf(lo, __shfl_xor(lo, offset)); hi = fmaxf(hi, __shfl_xor(hi, offset)); }
		if ((threadIdx.x & 63) == 0 && lo <= hi) { atomicMin(&a.scene_box[d], light_tree_ordered(lo)); atomicMax(&a.scene_box[3 + d], light_tree_ordered(hi)); }
	}
}

__global__ void __launch_bounds__(RT_LIGHT_TREE_BLOCK) kernel_light_tree_keys(LightTreeBuildArgs a) {
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= a.leaf_count) return;
	TlasBox scene, box;
	for (int d = 0; d < 3; d++) { scene.min[d] = light_tree_unordered(a.scene_box[d]); scene.max[d] = light_tree_unordered(a.scene_box[3 + d]); }
	const float4 lo = a.leaf_nodes[2 * size_t(k)], hi = a.leaf_nodes[2 * size_t(k) + 1];
	box.min[0] = lo.x; box.min[1] = lo.y; box.min[2] = lo.z; box.max[0] = hi.x; box.max[1] = hi.y; box.max[2] = hi.z;
	a.keys[k] = (uint64_t(tlas_morton(box, scene)) << 32) | uint64_t(uint32_t(k));
	a.ids[k] = k;
}

__global__ void __launch_bounds__(RT_LIGHT_TREE_BLOCK) kernel_light_tree_place(LightTreeBuildArgs a) {
	const int s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= a.padded) return;
	const size_t node = size_t(a.padded) - 1 + s;
	if (s < a.leaf_count) {
		const int id = a.sorted_ids[s];
		a.nodes[2 * node] = a.leaf_nodes[2 * size_t(id)]; a.nodes[2 * node + 1] = a.leaf_nodes[2 * size_t(id) + 1];
		a.slot_of_leaf[id] = int(node); a.leaf_of_slot[s] = id;
	} else {   // padding: no power, an inverted box
		a.nodes[2 * node] = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.0f); a.nodes[2 * node + 1] = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f);
		a.leaf_of_slot[s] = -1;
	}
}

// An inner node from its children: Phi_left + Phi_right; the union of the boxes of the children of positive Phi (none: the inverted box).
RT_DEV void light_tree_join(float4 l_lo, float4 l_hi, float4 r_lo, float4 r_hi, float4 & lo, float4 & hi) {
	lo = make_float4(3.0e38f, 3.0e38f, 3.0e38f, l_lo.w + r_lo.w); hi = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, 0.0f);
	if (l_lo.w > 0.0f) { lo.x = fminf(lo.x, l_lo.x); lo.y = fminf(lo.y, l_lo.y); lo.z = fminf(lo.z, l_lo.z); hi.x = fmaxf(hi.x, l_hi.x); hi.y = fmaxf(hi.y, l_hi.y); hi.z = fmaxf(hi.z, l_hi.z); }
	if (r_lo.w > 0.0f) { lo.x = fminf(lo.x, r_lo.x); lo.y = fminf(lo.y, r_lo.y); lo.z = fminf(lo.z, r_lo.z); hi.x = fmaxf(hi.x, r_hi.x); hi.y = fmaxf(hi.y, r_hi.y); hi.z = fmaxf(hi.z, r_hi.z); }
}

// one level of `count` nodes from `first` on; its children were written by an earlier launch
__global__ void __launch_bounds__(RT_LIGHT_TREE_BLOCK) kernel_light_tree_level(float4 * nodes, int first, int count) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const size_t node = size_t(first) + i, left = 2 * node + 1, right = 2 * node + 2;
	float4 lo, hi;
	light_tree_join(nodes[2 * left], nodes[2 * left + 1], nodes[2 * right], nodes[2 * right + 1], lo, hi);
	nodes[2 * node] = lo; nodes[2 * node + 1] = hi;
}

// ONE workgroup: the levels of `top_count` (a power of two, at most RT_LIGHT_TREE_BLOCK) nodes and fewer. The first of them reads its children from memory
// (an earlier launch wrote them), the ones above read this workgroup's own LDS copy after a barrier.
__global__ void __launch_bounds__(RT_LIGHT_TREE_BLOCK) kernel_light_tree_top(float4 * nodes, int top_count) {
	__shared__ float4 lds_lo[2 * RT_LIGHT_TREE_BLOCK], lds_hi[2 * RT_LIGHT_TREE_BLOCK];   // heap numbering, nodes [0, 2 top_count - 1)
	const int i = threadIdx.x;
	if (i < top_count) {
		const size_t node = size_t(top_count) - 1 + i, left = 2 * node + 1, right = 2 * node + 2;
		light_tree_join(nodes[2 * left], nodes[2 * left + 1], nodes[2 * right], nodes[2 * right + 1], lds_lo[node], lds_hi[node]);
		nodes[2 * node] = lds_lo[node]; nodes[2 * node + 1] = lds_hi[node];
	}
	for (int count = top_count / 2; count >= 1; count /= 2) {
		__syncthreads();
		if (i < count) {
			const int node = count - 1 + i, left = 2 * node + 1, right = 2 * node + 2;
			light_tree_join(lds_lo[left], lds_hi[left], lds_lo[right], lds_hi[right], lds_lo[node], lds_hi[node]);
			nodes[2 * size_t(node)] = lds_lo[node]; nodes[2 * size_t(node) + 1] = lds_hi[node];
		}
	}
}

size_t rt_light_tree_sort_scratch_bytes(size_t leaves) {
	size_t bytes = 0;
	(void)rocprim::radix_sort_pairs(nullptr, bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (int *)nullptr, (int *)nullptr, leaves, 0, 62);
	return bytes + 256;
}

hipError_t rt_light_tree_build(const LightTreeBuildArgs & a, hipStream_t stream) {
	const int N = a.leaf_count, M = a.padded, B = RT_LIGHT_TREE_BLOCK;
	if (N < 1 || M < N || (M & (M - 1)) != 0) return hipErrorInvalidValue;
	const int widest = std::max(std::max(a.mesh_count, a.triangle_count), 3);
	hipLaunchKernelGGL(kernel_light_tree_begin, dim3((widest + B - 1) / B), dim3(B), 0, stream, a);
	hipLaunchKernelGGL(kernel_light_tree_leaves, dim3((N + B - 1) / B), dim3(B), 0, stream, a);
	hipLaunchKernelGGL(kernel_light_tree_keys, dim3((N + B - 1) / B), dim3(B), 0, stream, a);
	size_t bytes = a.sort_scratch_bytes;
	hipError_t e = rocprim::radix_sort_pairs(a.sort_scratch, bytes, a.keys, a.sorted_keys, a.ids, a.sorted_ids, size_t(N), 0, 62, stream);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(kernel_light_tree_place, dim3((M + B - 1) / B), dim3(B), 0, stream, a);
	int count = M / 2;   // nodes of the level above the leaves, first node count - 1
	for (; count > B; count /= 2) hipLaunchKernelGGL(kernel_light_tree_level, dim3(count / B), dim3(B), 0, stream, a.nodes, count - 1, count);
	if (count >= 1) hipLaunchKernelGGL(kernel_light_tree_top, dim3(1), dim3(B), 0, stream, a.nodes, count);
	return hipGetLastError();
}

// ---- probes ----
__global__ void kernel_light_tree_sample(RtLightTree t, const float * probes, int count, float * out) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * a = probes + size_t(i) * 5;
	const LightTreePick pick = light_tree_sample(t, a[2], a[3], a[4], a[0], a[1]);
	float * o = out + size_t(i) * 4;
	o[0] = __int_as_float(pick.slot >= 0 ? t.leaf_of_slot[pick.slot - (t.padded - 1)] : -1);
	o[1] = __int_as_float(pick.slot); o[2] = pick.pmf; o[3] = 0.0f;
}
__global__ void kernel_light_tree_pmf(RtLightTree t, const float * probes, int count, float * out) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * a = probes + size_t(i) * 4;
	out[i] = light_tree_pmf(t, a[1], a[2], a[3], t.slot_of_leaf[__float_as_int(a[0])]);
}
void rt_launch_light_tree_sample(const RtLightTree & t, const float * probes, int count, float * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_light_tree_sample, dim3((count + 255) / 256), dim3(256), 0, stream, t, probes, count, out);
}
void rt_launch_light_tree_pmf(const RtLightTree & t, const float * probes, int count, float * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_light_tree_pmf, dim3((count + 255) / 256), dim3(256), 0, stream, t, probes, count, out);
}
