// rt_build_args.h -- the argument blocks of the device BLAS build (kernels_blas.hip) and the device TLAS build (kernels_build.hip), which their kernels
// take BY VALUE, and the host functions that launch them: ONE definition for the kernels and for the caller that fills them (rt_scene.hip). Private to csrc/.
#pragma once
#include "rt_tlas_build.h"

#include <hip/hip_runtime.h>

struct BlasBuildArgs {
	int triangle_count, mesh_count, first_node;     // first_node: index of mesh 0's root (node slots below it are reserved for the TLAS)
	const float4 * triangles;                        // input, 6 float4 each, meshes back to back
	const int * mesh_first;                          // [mesh_count + 1]
	float4 * triangles_out, * positions_out;         // leaf order: 6 resp. 3 float4 per triangle
	uint32_t * nodes;                                // 20 words per node
	int * order, * position;                         // leaf position -> input triangle, and back
	// scratch
	TlasBox * triangle_boxes, * sorted_boxes, * mesh_boxes, * child_boxes;
	TlasBox * box_table;                             // [table_levels][triangle_count]: entry (j, i) = box of sorted triangles [i, i + 2^(j+1)), clamped at the end (level 0 of the idea is sorted_boxes)
	int table_levels, split_widest;                  // split_widest: the round-3 rule (the piece with the most triangles first), for comparison
	int * triangle_mesh;
	uint64_t * keys; int * ids;                      // unsorted
	uint64_t * sorted_keys; int * sorted_ids;
	int2 * range;                                    // per node: its run [lo, hi) of the sorted order
	int * runs;                                      // per node of the level: begin[9], children, inner children, leaf triangles
	int * inner_count, * leaf_count, * inner_base, * leaf_base;   // per node of the level
	int * level_state;                               // { nodes used, triangles placed, nodes of the next level }
	const float * given_boxes; int given_first, given_count;   // rt_set_build_boxes: triangles [given_first, given_first + given_count) come with boxes of their own (6 floats: min, max), null / 0: none
};

struct TlasBuildArgs {
	int count;                       // instances
	// scene order inputs
	const int    * root_indices;     // BLAS root | identity flag << 31
	const int    * material_ids;
	const float4 * transforms, * transforms_inv, * transforms_prev; // 3 float4 per instance
	const float  * local_boxes;      // 6 floats per instance: object-space min, max of its BLAS
	// TLAS order outputs
	uint32_t * nodes;                // 20 words per node, capacity 2 * count nodes
	int      * out_root_indices, * out_material_ids;
	float4   * out_transforms, * out_transforms_inv, * out_transforms_prev;
	int      * order;                // position -> scene index
	int      * position;             // scene index -> position
	int      * node_count;
	// scratch (global): boxes[count], queues 2 x count x {node, lo, hi}, per level-node records
	TlasBox  * boxes, * sorted_boxes;
	int      * queue;                // [2][count][3]
	int      * runs;                 // [count][12]: begin[9], children, inner children, leaf children
	int      * bases;                // [count][2]: first child node index, first leaf position
	TlasBox  * child_boxes;          // (unused since the lane-per-child build; kept for the layout of the scratch area)
};

// kernels_blas.hip
size_t rt_blas_build_scratch_bytes(size_t triangles, size_t meshes);
hipError_t rt_blas_build(BlasBuildArgs a, void * library_scratch, size_t library_scratch_bytes, int * pinned_state, hipStream_t stream, int * out_node_count, size_t node_capacity);
// kernels_build.hip
void rt_launch_build_tlas(const TlasBuildArgs & args, hipStream_t stream);
