// rt_light_tree.h -- the light tree: what the kernels read of it, and the selection and its pmf as device functions shared by the
// material and sort kernels (rt_lights.h and kernels_sort.hip, the ..._tree instances) and the probes (kernels_light_tree.hip: rt_sample_light_tree, rt_light_tree_pmf).
//
// The tree: one leaf per (light-mesh entry m, triangle j of its span), id k = leaf_base[m] + j; the leaves sorted along a Morton curve of their box
// centres (ties by id); an implicit complete binary tree over the sorted order, padded to M = 2^ceil(log2 N) leaves, in heap numbering -- the children of
// node i are 2i + 1 and 2i + 2, the leaf of sorted place s is node M - 1 + s, no pointers. A node is two float4: {box_min, Phi}, {box_max, pad}. Phi of a
// leaf is its power (world area x luminance of the emission), Phi of an inner node Phi_left + Phi_right in float32, in that order; an inner node's box is
// the union of the boxes of its children of positive Phi. A node of Phi == 0 (a padding leaf, a triangle without area or emission, a subtree of such) is
// never entered and its box is never read.
//
// Every float operation below is a single rounded float32 operation in the order written (the units build with -ffp-contract=off; nothing is fused), so that
// tests/light_tree_reference.py restates it bit for bit.
#pragma once
#include <float.h>
#include <stdint.h>

// The descent's rule for its random number: u is rescaled at every level, which spends -log2(P) of its 24 bits. Once the product of the probabilities so
// far has fallen below 2^-16 -- fewer than 8 bits are left -- the descent continues, ONCE, with the second number (DIM_NEE_LIGHT.y, which the tree otherwise
// leaves free). The rule looks at the product alone, never at u: the pmf of a leaf does not depend on it.
#define RT_LIGHT_TREE_FRESH_BELOW 0x1p-16f

struct RtLightTree {
	const float4 * nodes;             // [2 * (2 M - 1)]
	const float4 * leaves;            // [N], by id: {light-mesh entry (int bits), triangle id (int bits), world area A, Phi}
	const int * leaf_of_slot;         // [M]: id of the leaf at sorted place s (node M - 1 + s), -1 for padding
	const int * slot_of_leaf;         // [N]: node of leaf id
	const int * leaf_base;            // [light_mesh_count + 1]
	const int * entry_of_mesh;        // [mesh_count]: light-mesh entry of an instance (row of the instance tables), or -1
	const int * place_of_triangle;    // [triangle_count]: place of a triangle in light_triangle_indices, or -1
	int leaf_count, padded;           // N, M; padded == 0: no tree
};

#if defined(__HIPCC__)
// Importance of `node` seen from p: Phi / max(d^2, r^2, FLT_MIN), d^2 the squared distance from p to the box centre, r^2 the squared half diagonal.
__device__ __forceinline__ float light_tree_importance(const RtLightTree & t, int node, float px, float py, float pz, float & phi) {
	const float4 lo = t.nodes[2 * size_t(node)];
	phi = lo.w;
	if (!(phi > 0.0f)) return 0.0f;
	const float4 hi = t.nodes[2 * size_t(node) + 1];
	const float cx = 0.5f * (lo.x + hi.x), cy = 0.5f * (lo.y + hi.y), cz = 0.5f * (lo.z + hi.z);
	const float hx = 0.5f * (hi.x - lo.x), hy = 0.5f * (hi.y - lo.y), hz = 0.5f * (hi.z - lo.z);
	const float dx = px - cx, dy = py - cy, dz = pz - cz;
	const float d2 = (dx * dx + dy * dy) + dz * dz;
	const float r2 = (hx * hx + hy * hy) + hz * hz;
	return phi / fmaxf(fmaxf(d2, r2), FLT_MIN);
}
// Probability of the left child at inner node `node`: I_l / (I_l + I_r); Phi_l / (Phi_l + Phi_r) when that sum is not finite or not positive; -1 when
// neither is (a subtree without power, or one whose power has overflowed): nothing below can be chosen.
__device__ __forceinline__ float light_tree_left(const RtLightTree & t, int node, float px, float py, float pz) {
	float phi_l, phi_r;
	float left = light_tree_importance(t, 2 * node + 1, px, py, pz, phi_l);
	const float right = light_tree_importance(t, 2 * node + 2, px, py, pz, phi_r);
	float sum = left + right;
	if (!(sum > 0.0f && sum <= FLT_MAX)) {
		left = phi_l; sum = phi_l + phi_r;
		if (!(sum > 0.0f && sum <= FLT_MAX)) return -1.0f;
	}
	return left / sum;
}
// The descent from the root. slot: the node of the chosen leaf, -1 when the tree holds no power; pmf: the product of the probabilities along its path.
struct LightTreePick { int slot; float pmf; };
__device__ __forceinline__ LightTreePick light_tree_sample(const RtLightTree & t, float px, float py, float pz, float u, float u2) {
	LightTreePick pick = { -1, 0.0f };
	if (t.padded <= 0 || !(t.nodes[0].w > 0.0f)) return pick;
	int node = 0; float pmf = 1.0f; bool first_number = true;
	while (node < t.padded - 1) {
		const float left = light_tree_left(t, node, px, py, pz);
		if (left < 0.0f) return pick;
		if (u < left) { node = 2 * node + 1; u = u / left; pmf = pmf * left; }
		else { const float right = 1.0f - left; node = 2 * node + 2; u = (u - left) / right; pmf = pmf * right; }
		u = fminf(u, 0x1.fffffep-1f);
		if (first_number && pmf < RT_LIGHT_TREE_FRESH_BELOW) { u = u2; first_number = false; }
	}
	pick.slot = node; pick.pmf = pmf;
	return pick;
}
// The pmf of the leaf at node `slot`: the same factors in the same order -- the path from the root is the binary expansion of slot + 1 below its leading
// one -- hence the bits light_tree_sample reports when it arrives there.
__device__ __forceinline__ float light_tree_pmf(const RtLightTree & t, float px, float py, float pz, int slot) {
	if (t.padded <= 0 || !(t.nodes[0].w > 0.0f)) return 0.0f;
	const unsigned path = unsigned(slot) + 1u;
	int node = 0; float pmf = 1.0f;
	for (int bit = 30 - __clz(int(path)); bit >= 0; bit--) {
		const float left = light_tree_left(t, node, px, py, pz);
		if (left < 0.0f) return 0.0f;
		const bool right = (path >> bit) & 1u;
		pmf = pmf * (right ? 1.0f - left : left);
		node = 2 * node + 1 + (right ? 1 : 0);
	}
	return pmf;   // (a leaf of Phi == 0 below the root has importance 0: its last factor is 0, or the walk ended at -1)
}
// The node of the leaf a hit (instance row, triangle) lies on, or -1 when it is no leaf of the tree.
__device__ __forceinline__ int light_tree_slot_of_hit(const RtLightTree & t, const int2 * spans, int mesh_id, int triangle_id, float & area) {
	const int entry = t.entry_of_mesh[mesh_id], place = t.place_of_triangle[triangle_id];
	if (entry < 0 || place < 0) return -1;
	const int2 span = spans[entry];
	if (place < span.x || place > span.y) return -1;
	const int leaf = t.leaf_base[entry] + (place - span.x);
	area = t.leaves[leaf].z;
	return t.slot_of_leaf[leaf];
}
#endif

// The build (kernels_light_tree.hip): everything on `stream`, nothing waited for. sort_scratch: rt_light_tree_sort_scratch_bytes(N) bytes.
struct LightTreeBuildArgs {
	// in: the scene as the kernels hold it
	const float4 * triangles; const float4 * mesh_transforms; const int * mesh_position; const int * mesh_material_ids;
	const uint8_t * material_types; const float4 * materials;
	const int * light_triangle_indices; const int2 * light_mesh_triangle_span; const int * light_mesh_transform_indices;
	int light_mesh_count, mesh_count, triangle_count, material_count;
	// out: RtLightTree's arrays
	float4 * nodes, * leaves; int * leaf_of_slot, * slot_of_leaf, * entry_of_mesh, * place_of_triangle;
	const int * leaf_base;
	int leaf_count, padded;
	// scratch
	float4 * leaf_nodes; int * scene_box; uint64_t * keys, * sorted_keys; int * ids, * sorted_ids; void * sort_scratch; size_t sort_scratch_bytes;
};
size_t rt_light_tree_sort_scratch_bytes(size_t leaves);
hipError_t rt_light_tree_build(const LightTreeBuildArgs & a, hipStream_t stream);
// probes: {u, u2, p[3]} -> {leaf id, slot (int bits), pmf, pad}; {leaf id (int bits), p[3]} -> pmf
void rt_launch_light_tree_sample(const RtLightTree & t, const float * probes, int count, float * out, hipStream_t stream);
void rt_launch_light_tree_pmf(const RtLightTree & t, const float * probes, int count, float * out, hipStream_t stream);
