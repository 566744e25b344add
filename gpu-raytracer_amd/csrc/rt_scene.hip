// rt_scene.hip -- the part of the C ABI (include/gpu_raytracer_amd.h) that is a scene upload: the scene rings, geometry / TLAS / instances for the three BVH widths, the
// device BLAS and TLAS builds and their read-backs, materials with their normal maps and opacity masks, media, textures, lights and delta lights, the
// RNG tables, the sky with its sampling tables, and the BSDF look-up tables integrated from the RNG tables.
#include "rt_build_args.h"
#include "rt_context.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// (re)allocate + synchronous upload
static int upload(rt_context * ctx, void ** slot, const void * src, size_t bytes) {
	RT_HIP(ctx, quiesce(ctx)); // samples in flight may still read the old buffer
	device_free(ctx, *slot);
	*slot = nullptr;
	int s = device_alloc(ctx, slot, bytes);
	if (s != RT_OK) return s;
	if (bytes && src) RT_HIP(ctx, hipMemcpy(*slot, src, bytes, hipMemcpyHostToDevice));
	return RT_OK;
}

// Next version of a scene ring, sized `bytes`: returns its pinned staging buffer for the caller to fill;
// ring_commit() then starts the copy. `which` selects the slot field that remembers the version in use.
static int ring_begin(rt_context * ctx, SceneRing & ring, size_t bytes, void ** staging) {
	if (bytes == 0) bytes = 16;
	// a launch of the merged wavefront traces the rays of every submission in flight against ONE scene version
	if (ctx->path_stream.created) {
		RT_HIP(ctx, stream_flush(ctx));
		// ... and the copy into the next version (main stream) runs after everything the wavefront has enqueued: its kernels read
		// ring versions too, and nothing else orders the two streams (the flush only ENQUEUES the remaining iterations). Without
		// this wait a version was safe from being overwritten under a running iteration only because RT_SCENE_VERSIONS (12)
		// exceeds what RT_STREAM_RUN_AHEAD (4) lets the host get ahead.
		RT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->path_stream.ev_idle, 0));
	}
	if (bytes > ring.capacity) { // first use, or the scene outgrew the ring: start over (the only case that drains)
		RT_HIP(ctx, quiesce(ctx));
		size_t capacity = bytes + bytes / 2 + 256; // a TLAS changes its node count a little from frame to frame
		for (int v = 0; v < RT_SCENE_VERSIONS; v++) {
			device_free(ctx, ring.device[v]); ring.device[v] = nullptr;
			if (ring.pinned[v]) { (void)hipHostFree(ring.pinned[v]); ring.pinned[v] = nullptr; }
			int s = device_alloc(ctx, &ring.device[v], capacity); if (s) return s;
			RT_HIP(ctx, hipHostMalloc(&ring.pinned[v], capacity));
			if (!ring.copied[v]) RT_HIP(ctx, hipEventCreateWithFlags(&ring.copied[v], hipEventDisableTiming));
		}
		ring.capacity = capacity;
		ring.current = -1;
		for (unsigned & users : ring.users) users = 0;
	}
	ring.bytes = bytes;
	int v = (ring.current + 1) % RT_SCENE_VERSIONS;
	// wait for the submissions that read version v -- for them only: a slot's ev_done is re-recorded by every later
	// submission, waiting on it would stall the host behind the frame it has just submitted
	for (int k = 0; k < RT_MAX_SAMPLE_SLOTS; k++) if ((ring.users[v] >> k) & 1u) RT_HIP(ctx, hipEventSynchronize(ring.last_use[v][k]));
	ring.users[v] = 0;
	if (ring.current >= 0) RT_HIP(ctx, hipEventSynchronize(ring.copied[v])); // its previous staging copy (recorded when it was last filled)
	*staging = ring.pinned[v];
	ring.current = v;
	return RT_OK;
}

static int ring_commit(rt_context * ctx, SceneRing & ring) {
	int v = ring.current;
	RT_HIP(ctx, hipMemcpyAsync(ring.device[v], ring.pinned[v], ring.bytes, hipMemcpyHostToDevice, ctx->stream));
	RT_HIP(ctx, hipEventRecord(ring.copied[v], ctx->stream));
	RT_HIP(ctx, hipEventRecord(ctx->ev_scene, ctx->stream));
	return RT_OK;
}

// A submission on sample slot `slot_index` (stream `st`, everything enqueued) read the current version of every scene ring
int mark_scene_versions_in_use(rt_context * ctx, int slot_index, hipStream_t st) {
	for (SceneRing * ring : { &ctx->tlas_ring, &ctx->instance_ring, &ctx->light_ring }) {
		if (ring->current < 0) continue;
		hipEvent_t & e = ring->last_use[ring->current][slot_index];
		if (!e) RT_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
		RT_HIP(ctx, hipEventRecord(e, st));
		ring->users[ring->current] |= 1u << slot_index;
	}
	return RT_OK;
}

// traversal copy of the triangles: positions only, 48 B stride (first 36 B of each 96 B triangle + 12 B pad)
static int upload_triangle_positions(rt_context * ctx, const void * triangles, size_t triangle_count) {
	std::vector<float> positions(triangle_count * 12, 0.0f);
	const float * src = (const float *)triangles;
	for (size_t t = 0; t < triangle_count; t++) memcpy(&positions[t * 12], src + t * 24, 36);
	int s = upload(ctx, &ctx->triangle_positions, positions.data(), triangle_count * 48); if (s) return s;
	ctx->params.triangle_positions = (const float4 *)ctx->triangle_positions;
	ctx->params.has_triangle_aliases = 0; ctx->params.entry_tlas_stack_size = RT_INVALID;
	return RT_OK;
}

// The node array of one BVH width as the context holds it: 80-byte CWBVH nodes (8), 32-byte binary (2) or 128-byte 4-wide (4) nodes.
struct NodeArray { void * & device; size_t & count; const float4 * & param; size_t node_bytes; };
static NodeArray node_array(rt_context * ctx, int width) {
	if (width == 2) return { ctx->bvh2_nodes, ctx->bvh2_node_count, ctx->params.bvh2_nodes, 32 };
	if (width == 4) return { ctx->bvh4_nodes, ctx->bvh4_node_count, ctx->params.bvh4_nodes, 128 };
	return { ctx->bvh8_nodes, ctx->bvh8_node_count, ctx->params.bvh8_nodes, 80 };
}

static int upload_geometry(rt_context * ctx, const char * caller, int width, const void * triangles, size_t triangle_count, const void * nodes, size_t node_count) {
	if (!ctx || !triangles || !nodes) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: NULL argument", caller);
	NodeArray a = node_array(ctx, width);
	if (width == 8) { ctx->build_boxes.clear(); ctx->build_boxes_first = 0; }   // (boxes set for a build that never came do not wait for another geometry's)
	(void)hipSetDevice(ctx->device);
	int s = upload(ctx, &ctx->triangles, triangles, triangle_count * 96); if (s) return s;
	s = upload(ctx, &a.device, nodes, node_count * a.node_bytes); if (s) return s;
	s = upload_triangle_positions(ctx, triangles, triangle_count); if (s) return s;
	ctx->triangle_count = triangle_count; a.count = node_count;
	ctx->light_tree_dirty = true;   // (place_of_triangle is sized by the triangle count)
	ctx->params.triangles = (const float4 *)ctx->triangles;
	a.param = (const float4 *)a.device;
	if (width == 8) {   // what only the CWBVH has: the merged wavefront's TLAS copy in its node array, the flattened scene's engine
		ctx->tlas_version_in_nodes = ~0ull;
		ctx->params.geometry_below_4gib = rt_geometry_fits_flat_engine(node_count, triangle_count);
	}
	return RT_OK;
}

// A new version of the TLAS, in the node format of `width`
static int upload_tlas(rt_context * ctx, const char * caller, int width, const void * tlas_nodes, size_t tlas_node_count) {
	if (!ctx || !tlas_nodes) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: NULL argument", caller);
	NodeArray a = node_array(ctx, width);
	if (!a.device || tlas_node_count > a.count) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: geometry not uploaded or TLAS larger than the node array", caller);
	(void)hipSetDevice(ctx->device);
	void * staging = nullptr;
	int s = ring_begin(ctx, ctx->tlas_ring, tlas_node_count * a.node_bytes, &staging); if (s) return s;
	memcpy(staging, tlas_nodes, tlas_node_count * a.node_bytes);
	s = ring_commit(ctx, ctx->tlas_ring); if (s) return s;
	ctx->params.tlas_nodes = (const float4 *)ctx->tlas_ring.device[ctx->tlas_ring.current];
	ctx->params.tlas_node_count = int(tlas_node_count);
	ctx->tlas_node_bytes = a.node_bytes;
	ctx->tlas_version++;
	return RT_OK;
}

// Opacity masks: word w of a mask holds texels [32 w, 32 w + 32) of level 0, bit k set iff byte `channel` of texel 32 w + k is >= cut.
// One thread per word, a plain store, no atomics: the bits are the same on every run. The tail word's bits past the last texel stay 0
// (texel_count is below 2^30, see rt_upload_material_opacity: every comparison is between non-negative ints).
__global__ void kernel_build_opacity_bits(const unsigned * texels, unsigned * words, int texel_count, int word_count, int channel, int cut) {
	int w = blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= word_count) return;
	int first = w * 32;
	unsigned bits = 0;
	for (int k = 0; k < 32; k++) {
		if (first + k < texel_count && int((texels[first + k] >> (8 * channel)) & 0xffu) >= cut) bits |= 1u << k;
	}
	words[w] = bits;
}
// Drops the masks (drains first: rays in flight read them). The next launches take the plain instances again.
static int opacity_clear(rt_context * ctx) {
	if (!ctx->material_opacity && !ctx->opacity_masks && !ctx->opacity_bits) return RT_OK;
	RT_HIP(ctx, quiesce(ctx));
	device_free(ctx, ctx->material_opacity); device_free(ctx, ctx->opacity_masks); device_free(ctx, ctx->opacity_bits);
	ctx->material_opacity = ctx->opacity_masks = ctx->opacity_bits = nullptr;
	ctx->material_opacity_list.clear(); ctx->opacity_mask_list.clear();
	ctx->params.material_opacity = nullptr; ctx->params.opacity_masks = nullptr; ctx->params.opacity_active = 0;
	return RT_OK;
}
// rt_upload_triangle_aliases: the two names of every triangle go into the padding of its position record
__global__ void kernel_name_triangles(float4 * positions, const int2 * names, int count) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	float4 last = positions[size_t(i) * 3 + 2];
	last.z = __int_as_float(names[i].x); last.w = __int_as_float(names[i].y);
	positions[size_t(i) * 3 + 2] = last;
}

// binary_search (rt_shading.h) ends inside its span only if the span's last entry is >= the searched value, and it is searched with numbers
// below 1: a table that ends lower sends every lane that draws a larger number past its end, for good. So the mesh table and every span a mesh
// entry names are checked here, on the host, before anything is staged. Triangle entries no mesh refers to are left alone: an emitter of zero
// emission or zero area has no mesh entry, and its stretch of the triangle table may hold NaN (0 / 0).
static int check_cumulative_table(rt_context * ctx, const char * what, const float * cdf, size_t first, size_t last) {
	for (size_t i = first; i <= last; i++) {
		if (std::isnan(cdf[i])) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: %s: entry %zu is NaN", what, i);
		if (i > first && cdf[i] < cdf[i - 1]) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: %s: entry %zu (%.9g) is below entry %zu (%.9g)", what, i, double(cdf[i]), i - 1, double(cdf[i - 1]));
	}
	if (cdf[last] < 1.0f) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: %s: its last entry, %zu, is %.9g, below 1: a search for a larger number would not end", what, last, double(cdf[last]));
	return RT_OK;
}
static int check_light_tables(rt_context * ctx, const int32_t * triangle_indices, const float * triangle_cdf, size_t triangle_count,
                              const float * mesh_cdf, const int32_t * mesh_span, const int32_t * mesh_transform_indices, size_t mesh_count, float total_weight) {
	if (triangle_count > size_t(INT32_MAX) || mesh_count > size_t(INT32_MAX)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: more than 2^31 - 1 table entries");
	if (!std::isfinite(total_weight) || total_weight < 0.0f) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: lights_total_weight is %.9g (it must be finite and not negative)", double(total_weight));
	if (triangle_count > 0 && (!triangle_indices || !triangle_cdf)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: NULL triangle table with light_triangle_count = %zu", triangle_count);
	if (mesh_count == 0) return RT_OK;
	if (!mesh_cdf || !mesh_span || !mesh_transform_indices) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: NULL mesh table with light_mesh_count = %zu", mesh_count);
	if (!(total_weight > 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: lights_total_weight is 0 with %zu light mesh entries", mesh_count);
	int s = check_cumulative_table(ctx, "the light mesh table", mesh_cdf, 0, mesh_count - 1); if (s) return s;
	for (size_t m = 0; m < mesh_count; m++) {
		long long first = mesh_span[2 * m], last = mesh_span[2 * m + 1];
		if (first < 0 || last >= (long long)triangle_count || first > last)
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_lights: light mesh entry %zu: its triangle span [%lld, %lld] is not inside [0, %zu) with first <= last", m, first, last, triangle_count);
		if (m > 0 && mesh_span[2 * m] == mesh_span[2 * m - 2] && mesh_span[2 * m + 1] == mesh_span[2 * m - 1]) continue;   // (instances of one mesh data: the span just checked)
		char what[96]; snprintf(what, sizeof(what), "the triangle table in the span [%lld, %lld] of light mesh entry %zu", first, last, m);
		s = check_cumulative_table(ctx, what, triangle_cdf, size_t(first), size_t(last)); if (s) return s;
	}
	return RT_OK;
}

extern "C" {

// What the flattened scene's engine (kernel_trace_stream_bvh8_flat*) can address: a node's byte offset is v_mul_u32_u24(index, 80) -- a 24-bit multiply, exact for
// fewer than 2^24 nodes (1.34 GB of them: the 4 GiB of the 32-bit offset is never the limit for nodes) -- and a triangle's a 32-bit index * 48. Beyond either limit
// the general engine walks the scene (64-bit addresses). (Round 5 checked the 4 GiB only: advisor finding.)
int rt_geometry_fits_flat_engine(size_t node_count, size_t triangle_count) {
	return node_count < (size_t(1) << 24) && triangle_count * 48 < (1ull << 32) ? 1 : 0;
}

int rt_upload_geometry(rt_context * ctx, const void * triangles, size_t triangle_count, const void * bvh8_nodes, size_t node_count) {
	return upload_geometry(ctx, "rt_upload_geometry", 8, triangles, triangle_count, bvh8_nodes, node_count);
}
int rt_upload_geometry_bvh2(rt_context * ctx, const void * triangles, size_t triangle_count, const void * bvh2_nodes, size_t node_count) {
	return upload_geometry(ctx, "rt_upload_geometry_bvh2", 2, triangles, triangle_count, bvh2_nodes, node_count);
}
int rt_upload_geometry_bvh4(rt_context * ctx, const void * triangles, size_t triangle_count, const void * bvh4_nodes, size_t node_count) {
	return upload_geometry(ctx, "rt_upload_geometry_bvh4", 4, triangles, triangle_count, bvh4_nodes, node_count);
}
int rt_upload_tlas(rt_context * ctx, const void * tlas_nodes, size_t tlas_node_count) { return upload_tlas(ctx, "rt_upload_tlas", 8, tlas_nodes, tlas_node_count); }
int rt_upload_tlas_bvh2(rt_context * ctx, const void * tlas_nodes, size_t tlas_node_count) { return upload_tlas(ctx, "rt_upload_tlas_bvh2", 2, tlas_nodes, tlas_node_count); }
int rt_upload_tlas_bvh4(rt_context * ctx, const void * tlas_nodes, size_t tlas_node_count) { return upload_tlas(ctx, "rt_upload_tlas_bvh4", 4, tlas_nodes, tlas_node_count); }

// Static geometry flattened into one BLAS: its triangles are COPIES of triangles that other BLASes own, and a hit on a copy is
// reported as the instance and the triangle it was copied from (kernels_trace.hip translates once per ray, when the ray is done).
// The two names are the last 8 bytes of the 48-byte position record (36 B of positions + 12 B of padding), so the translation
// costs one load from a line the triangle test has touched.
int rt_upload_triangle_aliases(rt_context * ctx, const int32_t * mesh_ids, const int32_t * triangle_ids) {
	RT_REQUIRE(ctx, ctx && ctx->triangle_positions, "rt_upload_triangle_aliases: no geometry uploaded");
	(void)hipSetDevice(ctx->device);
	if (!mesh_ids || !triangle_ids) { RT_HIP(ctx, quiesce(ctx)); ctx->params.has_triangle_aliases = 0; return RT_OK; }
	size_t count = ctx->triangle_count;
	std::vector<int32_t> names(2 * count);
	bool any = false;
	for (size_t i = 0; i < count; i++) {
		bool copy = mesh_ids[i] >= 0;
		RT_REQUIRE(ctx, !copy || (triangle_ids[i] >= 0 && size_t(triangle_ids[i]) < count && mesh_ids[triangle_ids[i]] < 0), "rt_upload_triangle_aliases: a copy must name a triangle of the array that is not itself a copy");
		names[2 * i] = copy ? mesh_ids[i] : -1; names[2 * i + 1] = copy ? triangle_ids[i] : -1;
		any = any || copy;
	}
	RT_HIP(ctx, quiesce(ctx));
	void * device_names = nullptr;
	int s = device_alloc(ctx, &device_names, names.size() * 4); if (s) return s;
	hipError_t e = hipMemcpy(device_names, names.data(), names.size() * 4, hipMemcpyHostToDevice);
	if (e == hipSuccess && count) {
		kernel_name_triangles<<<unsigned((count + 255) / 256), 256, 0, ctx->stream>>>((float4 *)ctx->triangle_positions, (const int2 *)device_names, int(count));
		e = hipGetLastError();
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	}
	device_free(ctx, device_names);
	if (e != hipSuccess) return fail(ctx, RT_ERROR_HIP, "rt_upload_triangle_aliases: %s", hipGetErrorString(e));
	ctx->params.has_triangle_aliases = any ? 1 : 0;
	return RT_OK;
}

// Replaces nodes [first_node, first_node + node_count) of the uploaded CWBVH node array in place: a tree whose children have been re-seated beside the frame
// loop (host/Integrator.cpp: reseat worker). A ray holds stack entries (child base, mask) only INSIDE one traversal launch, so the swap is safe between launches:
// the context is drained first. Boxes, leaves and triangles must be what they were (the caller's contract: the node count and every index stay).
int rt_update_nodes(rt_context * ctx, const void * nodes, size_t first_node, size_t node_count) {
	RT_REQUIRE(ctx, ctx && (nodes || node_count == 0), "rt_update_nodes: NULL argument");
	RT_REQUIRE(ctx, ctx->bvh8_nodes && first_node <= ctx->bvh8_node_count && node_count <= ctx->bvh8_node_count - first_node, "rt_update_nodes: range outside the uploaded CWBVH node array");
	if (node_count == 0) return RT_OK;
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	RT_HIP(ctx, hipMemcpy((char *)ctx->bvh8_nodes + first_node * 80, nodes, node_count * 80, hipMemcpyHostToDevice));
	return RT_OK;
}

// Where rays start: 0 = at the TLAS root in node slot 0; 1 = the whole scene is ONE world-space bottom-level tree whose root node
// the caller has put into node slot 0 (through rt_upload_tlas), rays are inside it from the start, as instance row 0. A change
// drains the context first: samples in flight were submitted against the old entry.
int rt_set_static_geometry(rt_context * ctx, int32_t whole_scene) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_set_static_geometry: NULL context");
	int entry = whole_scene ? 0 : RT_INVALID;
	if (ctx->params.entry_tlas_stack_size == entry) return RT_OK;
	RT_REQUIRE(ctx, !whole_scene || ctx->bvh8_nodes, "rt_set_static_geometry: CWBVH geometry only");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	ctx->params.entry_tlas_stack_size = entry;
	return RT_OK;
}

// "Skip behind the hit": see kernels_trace.hip. The wish is stored; the kernels take the walk when the scene is also one tree below 4 GiB (rt_skip_walk).
int rt_set_skip_behind_hit(rt_context * ctx, int32_t enable) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_set_skip_behind_hit: NULL context");
	if ((ctx->params.skip_behind_hit != 0) == (enable != 0)) return RT_OK;
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));   // (samples in flight were submitted under the other walk; the counters of a statistics pass must belong to one)
	ctx->params.skip_behind_hit = enable != 0;
	return RT_OK;
}
int rt_get_skip_behind_hit(const rt_context * ctx) { return ctx && rt_skip_walk(ctx->params) ? 1 : 0; }

// ---- BLAS build on the device (kernels_blas.hip) ---------------------------------------------------------------------

int rt_set_build_boxes(rt_context * ctx, const float * boxes, size_t first_triangle, size_t count) {
	RT_REQUIRE(ctx, ctx && (boxes || count == 0), "rt_set_build_boxes: NULL argument");
	RT_REQUIRE(ctx, first_triangle < (size_t(1) << 30) && count < (size_t(1) << 30), "rt_set_build_boxes: range out of bounds");
	ctx->build_boxes.assign(boxes, boxes + 6 * count);
	ctx->build_boxes_first = first_triangle;
	return RT_OK;
}

int rt_build_geometry(rt_context * ctx, const void * triangles, size_t triangle_count, const int32_t * mesh_first_triangle, size_t mesh_count,
                      size_t reserved_tlas_nodes, int32_t * out_root_indices, int32_t * out_triangle_positions, size_t * out_node_count, float * out_build_ms) {
	// rt_set_build_boxes: boxes that come with some of the triangles -- taken by THIS call whatever becomes of it (an early error exit used to leave them pending
	// for the next build, of possibly unrelated geometry: advisor finding, round 5); whatever does not fit the input is ignored
	std::vector<float> given_boxes; size_t given_first = 0;
	if (ctx) { given_boxes.swap(ctx->build_boxes); given_first = ctx->build_boxes_first; ctx->build_boxes_first = 0; }
	RT_REQUIRE(ctx, ctx && triangles && mesh_first_triangle, "rt_build_geometry: NULL argument");
	RT_REQUIRE(ctx, triangle_count >= 1 && mesh_count >= 1, "rt_build_geometry: at least one triangle and one mesh (a mesh may be empty, the input may not)");
	RT_REQUIRE(ctx, triangle_count < (size_t(1) << 30) && mesh_count < (size_t(1) << 24), "rt_build_geometry: too many triangles / meshes");
	RT_REQUIRE(ctx, mesh_first_triangle[0] == 0 && size_t(mesh_first_triangle[mesh_count]) == triangle_count, "rt_build_geometry: mesh_first_triangle must run from 0 to triangle_count");
	for (size_t m = 0; m < mesh_count; m++) RT_REQUIRE(ctx, mesh_first_triangle[m] <= mesh_first_triangle[m + 1], "rt_build_geometry: mesh_first_triangle must not decrease");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	const size_t T = triangle_count, M = mesh_count;
	const size_t node_capacity = reserved_tlas_nodes + M + T;          // every inner node has at least two children
	const size_t level_capacity = std::max(M, T / (4) + 1) + 1;        // an inner node holds more than 3 triangles
	// outputs (kept): triangles and positions in leaf order, nodes; everything else is scratch of this call
	void * out_triangles = nullptr, * out_positions = nullptr, * out_nodes = nullptr, * scratch = nullptr;
	int * pinned = nullptr; hipEvent_t t0 = nullptr, t1 = nullptr;
	// ONE way out on failure: whatever of the outputs, the scratch area, the pinned word and the timing events exists is released
	// (a scratch allocation that does not fit is a recoverable error: it must not strand the hundreds of MB allocated before it)
	auto give_up = [&](int status) {
		device_free(ctx, scratch); device_free(ctx, out_triangles); device_free(ctx, out_positions); device_free(ctx, out_nodes);
		if (pinned) (void)hipHostFree(pinned);
		if (t0) (void)hipEventDestroy(t0);
		if (t1) (void)hipEventDestroy(t1);
		return status;
	};
	#define RT_BUILD_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return give_up(fail(ctx, RT_ERROR_HIP, "rt_build_geometry: %s failed: %s", #call, hipGetErrorString(e_))); } while (0)
	int s;
	if ((s = device_alloc(ctx, &out_triangles, T * 96))) return give_up(s);
	if ((s = device_alloc(ctx, &out_positions, T * 48))) return give_up(s);
	if ((s = device_alloc(ctx, &out_nodes, node_capacity * 80))) return give_up(s);
	size_t at = 0;
	auto region = [&](size_t bytes) { size_t begin = at; at += (bytes + 255) / 256 * 256; return begin; };
	const size_t o_in = region(T * 96), o_first = region((M + 1) * 4), o_order = region(T * 4), o_position = region(T * 4),
	             o_tbox = region(T * 24), o_sbox = region(T * 24), o_mbox = region(M * 24), o_cbox = region(level_capacity * 8 * 24), o_tmesh = region(T * 4),
	             o_keys = region(T * 8), o_ids = region(T * 4), o_skeys = region(T * 8), o_sids = region(T * 4), o_range = region(node_capacity * 8),
	             o_runs = region(level_capacity * 48), o_ic = region(level_capacity * 4), o_lc = region(level_capacity * 4), o_ib = region(level_capacity * 4), o_lb = region(level_capacity * 4),
	             o_state = region(16);
	// boxes of all power-of-two runs of the sorted order (kernel_blas_box_table: the area of any run is two look-ups): levels 1 .. floor(log2 T)
	int table_levels = 0; while ((size_t(2) << table_levels) <= T) table_levels++;
	static const bool split_widest = getenv("GRT_BLAS_SPLIT_WIDEST") != nullptr;   // round 3's rule (most triangles first), for tools/blas_bench.py
	const size_t o_table = region(split_widest ? 0 : size_t(table_levels) * T * 24);
	const size_t library_bytes = rt_blas_build_scratch_bytes(T, M + level_capacity);
	const size_t o_library = region(library_bytes);
	const size_t given_count = given_first + given_boxes.size() / 6 <= T ? given_boxes.size() / 6 : 0;
	const size_t o_given = region(given_count * 24);
	if ((s = device_alloc(ctx, &scratch, at))) return give_up(s);
	char * base = (char *)scratch;
	RT_BUILD_HIP(hipMemcpyAsync(base + o_in, triangles, T * 96, hipMemcpyHostToDevice, ctx->stream));
	RT_BUILD_HIP(hipMemcpyAsync(base + o_first, mesh_first_triangle, (M + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	if (given_count) RT_BUILD_HIP(hipMemcpyAsync(base + o_given, given_boxes.data(), given_count * 24, hipMemcpyHostToDevice, ctx->stream));
	RT_BUILD_HIP(hipMemsetAsync(out_nodes, 0, node_capacity * 80, ctx->stream));
	BlasBuildArgs a;
	a.triangle_count = int(T); a.mesh_count = int(M); a.first_node = int(reserved_tlas_nodes);
	a.triangles = (const float4 *)(base + o_in); a.mesh_first = (const int *)(base + o_first);
	a.triangles_out = (float4 *)out_triangles; a.positions_out = (float4 *)out_positions; a.nodes = (uint32_t *)out_nodes;
	a.order = (int *)(base + o_order); a.position = (int *)(base + o_position);
	a.triangle_boxes = (TlasBox *)(base + o_tbox); a.sorted_boxes = (TlasBox *)(base + o_sbox); a.mesh_boxes = (TlasBox *)(base + o_mbox); a.child_boxes = (TlasBox *)(base + o_cbox);
	a.triangle_mesh = (int *)(base + o_tmesh);
	a.box_table = (TlasBox *)(base + o_table); a.table_levels = table_levels; a.split_widest = split_widest ? 1 : 0;
	a.keys = (uint64_t *)(base + o_keys); a.ids = (int *)(base + o_ids); a.sorted_keys = (uint64_t *)(base + o_skeys); a.sorted_ids = (int *)(base + o_sids);
	a.range = (int2 *)(base + o_range); a.runs = (int *)(base + o_runs);
	a.inner_count = (int *)(base + o_ic); a.leaf_count = (int *)(base + o_lc); a.inner_base = (int *)(base + o_ib); a.leaf_base = (int *)(base + o_lb);
	a.level_state = (int *)(base + o_state);
	a.given_boxes = given_count ? (const float *)(base + o_given) : nullptr; a.given_first = int(given_first); a.given_count = int(given_count);
	RT_BUILD_HIP(hipHostMalloc((void **)&pinned, 16));
	RT_BUILD_HIP(hipEventCreate(&t0)); RT_BUILD_HIP(hipEventCreate(&t1));
	RT_BUILD_HIP(hipEventRecord(t0, ctx->stream));
	int node_count = 0;
	hipError_t e = rt_blas_build(a, base + o_library, library_bytes, pinned, ctx->stream, &node_count, node_capacity);
	if (e == hipSuccess) e = hipEventRecord(t1, ctx->stream);
	if (e == hipSuccess && out_triangle_positions) e = hipMemcpyAsync(out_triangle_positions, a.position, T * 4, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	float ms = 0.0f;
	if (e == hipSuccess) (void)hipEventElapsedTime(&ms, t0, t1);
	if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return give_up(fail(ctx, RT_ERROR_HIP, "rt_build_geometry: %s", hipGetErrorString(e))); }
	(void)hipEventDestroy(t0); (void)hipEventDestroy(t1); (void)hipHostFree(pinned);
	device_free(ctx, scratch);
	#undef RT_BUILD_HIP
	// the context's geometry is what was built
	device_free(ctx, ctx->triangles); device_free(ctx, ctx->triangle_positions); device_free(ctx, ctx->bvh8_nodes);
	ctx->triangles = out_triangles; ctx->triangle_positions = out_positions; ctx->bvh8_nodes = out_nodes;
	ctx->triangle_count = T; ctx->bvh8_node_count = size_t(node_count);
	ctx->light_tree_dirty = true;
	ctx->tlas_version_in_nodes = ~0ull;
	ctx->params.triangles = (const float4 *)out_triangles; ctx->params.triangle_positions = (const float4 *)out_positions; ctx->params.bvh8_nodes = (const float4 *)out_nodes;
	ctx->params.geometry_below_4gib = rt_geometry_fits_flat_engine(size_t(node_count), size_t(T));
	ctx->params.has_triangle_aliases = 0; ctx->params.entry_tlas_stack_size = RT_INVALID;
	if (out_root_indices) for (size_t m = 0; m < M; m++) out_root_indices[m] = int32_t(reserved_tlas_nodes + m);
	if (out_node_count) *out_node_count = size_t(node_count);
	if (out_build_ms) *out_build_ms = ms;
	return RT_OK;
}

int rt_read_geometry(rt_context * ctx, void * out_triangles, void * out_bvh8_nodes) {
	RT_REQUIRE(ctx, ctx && ctx->triangles && ctx->bvh8_nodes, "rt_read_geometry: no CWBVH geometry on the device");
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	if (out_triangles)  RT_HIP(ctx, hipMemcpy(out_triangles,  ctx->triangles,  ctx->triangle_count * 96, hipMemcpyDeviceToHost));
	if (out_bvh8_nodes) RT_HIP(ctx, hipMemcpy(out_bvh8_nodes, ctx->bvh8_nodes, ctx->bvh8_node_count * 80, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_set_bvh_type(rt_context * ctx, int bvh_width) {
	RT_REQUIRE(ctx, ctx, "rt_set_bvh_type: NULL context");
	if (bvh_width != 8 && bvh_width != 4 && bvh_width != 2) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_set_bvh_type: the device has kernels for the binary BVH (2), the 4-wide BVH (4) and the 8-wide CWBVH (8), got %d", bvh_width);
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	ctx->bvh_width = bvh_width;
	ctx->params.bvh_width = bvh_width;
	return RT_OK;
}

int rt_upload_instances(rt_context * ctx, const int32_t * root_indices, const int32_t * material_ids,
                        const float * transforms, const float * transforms_inv, const float * transforms_prev, size_t mesh_count) {
	RT_REQUIRE(ctx, ctx && root_indices && material_ids && transforms && transforms_inv && transforms_prev, "rt_upload_instances: NULL argument");
	(void)hipSetDevice(ctx->device);
	// one allocation per version: roots | material ids | transforms | inverse | previous (48-byte rows are 16-byte aligned)
	size_t padded = (mesh_count + 3) / 4 * 4;
	size_t offset[6] = { 0, padded * 4, padded * 8, padded * 8 + mesh_count * 48, padded * 8 + mesh_count * 96, padded * 8 + mesh_count * 144 };
	const void * src[5] = { root_indices, material_ids, transforms, transforms_inv, transforms_prev };
	size_t bytes[5] = { mesh_count * 4, mesh_count * 4, mesh_count * 48, mesh_count * 48, mesh_count * 48 };
	void * staging = nullptr;
	int s = ring_begin(ctx, ctx->instance_ring, offset[5], &staging); if (s) return s;
	for (int i = 0; i < 5; i++) memcpy((char *)staging + offset[i], src[i], bytes[i]);
	s = ring_commit(ctx, ctx->instance_ring); if (s) return s;
	ctx->lowest_blas_root = 0x7fffffff;
	for (size_t i = 0; i < mesh_count; i++) ctx->lowest_blas_root = std::min(ctx->lowest_blas_root, int(root_indices[i] & 0x7fffffff));
	const char * base = (const char *)ctx->instance_ring.device[ctx->instance_ring.current];
	ctx->mesh_count = mesh_count; ctx->params.mesh_count = int(mesh_count);
	ctx->params.mesh_bvh_root_indices = (const int *)(base + offset[0]);
	ctx->params.mesh_material_ids     = (const int *)(base + offset[1]);
	ctx->params.mesh_transforms       = (const float4 *)(base + offset[2]);
	ctx->params.mesh_transforms_inv   = (const float4 *)(base + offset[3]);
	ctx->params.mesh_transforms_prev  = (const float4 *)(base + offset[4]);
	ctx->params.mesh_position = nullptr;   // the host supplies everything in TLAS order
	ctx->device_tlas_order = nullptr; ctx->device_tlas_node_count = nullptr;
	ctx->light_tree_dirty = true;   // (rebuilt once, before the next launch that reads it: light_tree_refresh)
	return RT_OK;
}

// ---- TLAS build on the device (kernels_build.hip) ---------------------------------------------------------------

int rt_build_tlas(rt_context * ctx, const int32_t * root_indices, const int32_t * material_ids,
                  const float * transforms, const float * transforms_inv, const float * transforms_prev,
                  const float * local_boxes, size_t mesh_count) {
	RT_REQUIRE(ctx, ctx && root_indices && material_ids && transforms && transforms_inv && transforms_prev && local_boxes, "rt_build_tlas: NULL argument");
	RT_REQUIRE(ctx, mesh_count >= 1 && mesh_count <= RT_TLAS_BUILD_MAX, "rt_build_tlas: 1 .. 4096 instances (larger scenes build the TLAS on the host: rt_upload_tlas)");
	RT_REQUIRE(ctx, ctx->bvh_width == 8 && ctx->bvh8_nodes && 2 * mesh_count <= ctx->bvh8_node_count, "rt_build_tlas: CWBVH geometry with 2 * mesh_count reserved node slots must be uploaded first");
	(void)hipSetDevice(ctx->device);
	const size_t n = mesh_count, padded = (n + 3) / 4 * 4;
	// one allocation per version: outputs | inputs | scratch (every region 16-byte aligned)
	size_t offset[24]; size_t at = 0; int regions = 0;
	auto region = [&](size_t bytes) { offset[regions++] = at; at += (bytes + 15) / 16 * 16; };
	region(padded * 4); region(padded * 4); region(n * 48); region(n * 48); region(n * 48);   // 0..4 out: roots, materials, transforms, inverse, previous
	region(padded * 4); region(padded * 4); region(16);                                      // 5..7 out: position, order, node count
	const size_t inputs_begin = at;
	region(padded * 4); region(padded * 4); region(n * 48); region(n * 48); region(n * 48); region(n * 24); // 8..13 in
	const size_t inputs_end = at;
	region(n * 24); region(n * 24); region(n * 48); region(n * 8); region(n * 192); region(n * 24); // 14..19 scratch: boxes, queues, runs, bases, child boxes, boxes in sorted order
	void * staging = nullptr;
	int s = ring_begin(ctx, ctx->instance_ring, at, &staging); if (s) return s;
	const void * src[6] = { root_indices, material_ids, transforms, transforms_inv, transforms_prev, local_boxes };
	const size_t bytes[6] = { n * 4, n * 4, n * 48, n * 48, n * 48, n * 24 };
	for (int i = 0; i < 6; i++) memcpy((char *)staging + offset[8 + i], src[i], bytes[i]);
	char * base = (char *)ctx->instance_ring.device[ctx->instance_ring.current];
	RT_HIP(ctx, hipMemcpyAsync(base + inputs_begin, (char *)staging + inputs_begin, inputs_end - inputs_begin, hipMemcpyHostToDevice, ctx->stream));
	void * tlas_staging = nullptr;
	s = ring_begin(ctx, ctx->tlas_ring, 2 * n * 80, &tlas_staging); if (s) return s;
	void * tlas_device = ctx->tlas_ring.device[ctx->tlas_ring.current];

	TlasBuildArgs a;
	a.count = int(n);
	a.root_indices = (const int *)(base + offset[8]); a.material_ids = (const int *)(base + offset[9]);
	a.transforms = (const float4 *)(base + offset[10]); a.transforms_inv = (const float4 *)(base + offset[11]); a.transforms_prev = (const float4 *)(base + offset[12]);
	a.local_boxes = (const float *)(base + offset[13]);
	a.nodes = (uint32_t *)tlas_device;
	a.out_root_indices = (int *)(base + offset[0]); a.out_material_ids = (int *)(base + offset[1]);
	a.out_transforms = (float4 *)(base + offset[2]); a.out_transforms_inv = (float4 *)(base + offset[3]); a.out_transforms_prev = (float4 *)(base + offset[4]);
	a.position = (int *)(base + offset[5]); a.order = (int *)(base + offset[6]); a.node_count = (int *)(base + offset[7]);
	a.boxes = (TlasBox *)(base + offset[14]); a.queue = (int *)(base + offset[15]); a.runs = (int *)(base + offset[16]); a.bases = (int *)(base + offset[17]); a.child_boxes = (TlasBox *)(base + offset[18]); a.sorted_boxes = (TlasBox *)(base + offset[19]);
	rt_launch_build_tlas(a, ctx->stream);
	RT_HIP(ctx, hipGetLastError());
	RT_HIP(ctx, hipEventRecord(ctx->instance_ring.copied[ctx->instance_ring.current], ctx->stream));
	RT_HIP(ctx, hipEventRecord(ctx->tlas_ring.copied[ctx->tlas_ring.current], ctx->stream));
	RT_HIP(ctx, hipEventRecord(ctx->ev_scene, ctx->stream));

	ctx->mesh_count = n; ctx->params.mesh_count = int(n);
	ctx->params.tlas_nodes = (const float4 *)tlas_device;
	ctx->params.tlas_node_count = int(2 * n);     // the node slots reserved for the TLAS; BLAS nodes start behind them
	ctx->params.entry_tlas_stack_size = RT_INVALID;   // node 0 is a TLAS root from now on: rays start above the instances (rt_set_static_geometry(ctx, 1) does not survive a TLAS build)
	ctx->tlas_version++;
	ctx->params.mesh_bvh_root_indices = a.out_root_indices;
	ctx->params.mesh_material_ids     = a.out_material_ids;
	ctx->params.mesh_transforms       = a.out_transforms;
	ctx->params.mesh_transforms_inv   = a.out_transforms_inv;
	ctx->params.mesh_transforms_prev  = a.out_transforms_prev;
	ctx->params.mesh_position         = a.position;
	ctx->device_tlas_order = a.order; ctx->device_tlas_node_count = a.node_count;
	ctx->light_tree_dirty = true;
	return RT_OK;
}

int rt_read_tlas(rt_context * ctx, int32_t * order, void * nodes, size_t node_capacity, int32_t * node_count) {
	RT_REQUIRE(ctx, ctx, "rt_read_tlas: NULL context");
	(void)hipSetDevice(ctx->device);
	if (!ctx->device_tlas_order) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_tlas: the current TLAS was not built on the device (rt_build_tlas)");
	RT_HIP(ctx, quiesce(ctx));
	int count = 0;
	RT_HIP(ctx, hipMemcpy(&count, ctx->device_tlas_node_count, sizeof(int), hipMemcpyDeviceToHost));
	if (node_count) *node_count = count;
	if (order) RT_HIP(ctx, hipMemcpy(order, ctx->device_tlas_order, ctx->mesh_count * sizeof(int), hipMemcpyDeviceToHost));
	if (nodes) RT_HIP(ctx, hipMemcpy(nodes, ctx->params.tlas_nodes, std::min(node_capacity, size_t(count)) * 80, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_read_instances(rt_context * ctx, int32_t * root_indices, int32_t * material_ids, float * transforms, float * transforms_inv, float * transforms_prev, int32_t * position) {
	RT_REQUIRE(ctx, ctx, "rt_read_instances: NULL context");
	(void)hipSetDevice(ctx->device);
	const RtParams & p = ctx->params;
	if (!p.mesh_bvh_root_indices) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_instances: no instance tables on the device (rt_upload_instances, rt_build_tlas)");
	if (position && !p.mesh_position) return fail(ctx, RT_ERROR_NOT_READY, "rt_read_instances: position[] exists only when the current TLAS was built on the device (rt_build_tlas)");
	RT_HIP(ctx, quiesce(ctx));
	const size_t n = ctx->mesh_count;
	if (root_indices)    RT_HIP(ctx, hipMemcpy(root_indices,    p.mesh_bvh_root_indices, n * 4,  hipMemcpyDeviceToHost));
	if (material_ids)    RT_HIP(ctx, hipMemcpy(material_ids,    p.mesh_material_ids,     n * 4,  hipMemcpyDeviceToHost));
	if (transforms)      RT_HIP(ctx, hipMemcpy(transforms,      p.mesh_transforms,       n * 48, hipMemcpyDeviceToHost));
	if (transforms_inv)  RT_HIP(ctx, hipMemcpy(transforms_inv,  p.mesh_transforms_inv,   n * 48, hipMemcpyDeviceToHost));
	if (transforms_prev) RT_HIP(ctx, hipMemcpy(transforms_prev, p.mesh_transforms_prev,  n * 48, hipMemcpyDeviceToHost));
	if (position)        RT_HIP(ctx, hipMemcpy(position,        p.mesh_position,         n * 4,  hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_upload_materials(rt_context * ctx, const uint8_t * types, const void * materials, size_t count) {
	RT_REQUIRE(ctx, ctx && types && materials, "rt_upload_materials: NULL argument");
	(void)hipSetDevice(ctx->device);
	int s = upload(ctx, &ctx->material_types, types, count); if (s) return s;
	s = upload(ctx, &ctx->materials, materials, count * 32); if (s) return s;
	ctx->params.material_types = (const uint8_t *)ctx->material_types;
	ctx->params.materials      = (const float4 *)ctx->materials;
	ctx->material_type_list.assign(types, types + count);
	ctx->params.material_normal_maps = nullptr;   // new materials: no normal maps until rt_upload_material_normal_maps
	ctx->params.normal_map_slots = 0;
	s = opacity_clear(ctx); if (s) return s;      // ... and no opacity masks until rt_upload_material_opacity

	// Scene::check_materials (Scene.cpp:50-70): which material kernels have to run at all
	for (bool & h : ctx->has_material) h = false;
	ctx->has_lights = false;
	const float * m = (const float *)materials;
	for (size_t i = 0; i < count; i++) {
		switch (types[i]) {
			case RT_MATERIAL_DIFFUSE:    ctx->has_material[0] = true; break;
			case RT_MATERIAL_PLASTIC:    ctx->has_material[1] = true; break;
			case RT_MATERIAL_DIELECTRIC: ctx->has_material[2] = true; break;
			case RT_MATERIAL_CONDUCTOR:  ctx->has_material[3] = true; break;
			case RT_MATERIAL_LIGHT:      ctx->has_lights |= (m[8 * i] * m[8 * i] + m[8 * i + 1] * m[8 * i + 1] + m[8 * i + 2] * m[8 * i + 2]) > 0.0f; break;
			default: return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_materials: unknown material type %d at index %zu", int(types[i]), i);
		}
	}
	ctx->light_tree_dirty = true;   // (emission may have changed)
	return RT_OK;
}

int rt_upload_material_normal_maps(rt_context * ctx, const int32_t * texture_ids, size_t count) {
	RT_REQUIRE(ctx, ctx && (texture_ids || count == 0), "rt_upload_material_normal_maps: NULL argument");
	RT_REQUIRE(ctx, ctx->params.materials, "rt_upload_material_normal_maps: no materials uploaded");
	if (count != ctx->material_type_list.size())
		return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_normal_maps: %zu ids for %zu materials", count, ctx->material_type_list.size());
	int slots = 0;
	for (size_t i = 0; i < count; i++) {
		int id = texture_ids[i];
		if (id == RT_INVALID) continue;
		if (id < 0 || size_t(id) >= ctx->texture_formats.size())
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_normal_maps: material %zu names texture %d of %zu", i, id, ctx->texture_formats.size());
		if (ctx->texture_formats[id] != RT_TEXTURE_RGBA8)
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_normal_maps: material %zu names texture %d, which is not RT_TEXTURE_RGBA8", i, id);
		int type = ctx->material_type_list[i];
		if (type >= RT_MATERIAL_DIFFUSE && type <= RT_MATERIAL_CONDUCTOR) slots |= 1 << (type - RT_MATERIAL_DIFFUSE);
	}
	(void)hipSetDevice(ctx->device);
	if (slots == 0) {   // none (or only on lights): every launch keeps its plain instance
		RT_HIP(ctx, quiesce(ctx));
		ctx->params.material_normal_maps = nullptr;
		ctx->params.normal_map_slots = 0;
		return RT_OK;
	}
	int s = upload(ctx, &ctx->material_normal_maps, texture_ids, count * sizeof(int32_t)); if (s) return s;
	ctx->params.material_normal_maps = (const int *)ctx->material_normal_maps;
	ctx->params.normal_map_slots = slots;
	return RT_OK;
}

// Opacity masks. Everything is checked before anything changes; then the context is drained (rays in flight hold no mask
// state, but the launches that carry them read the tables), the old masks are freed and one mask per distinct (texture, channel, cut) is
// built on the device. A mask on a light material is ignored: masks act in traversal, and emitters are sampled whole.
int rt_upload_material_opacity(rt_context * ctx, const int32_t * texture_ids, const int32_t * channels, const float * thresholds, size_t count) {
	RT_REQUIRE(ctx, ctx, "rt_upload_material_opacity: NULL context");
	(void)hipSetDevice(ctx->device);
	if (!texture_ids) return opacity_clear(ctx);
	RT_REQUIRE(ctx, channels && thresholds, "rt_upload_material_opacity: NULL channels or thresholds");
	RT_REQUIRE(ctx, ctx->params.materials, "rt_upload_material_opacity: no materials uploaded");
	if (count != ctx->material_type_list.size())
		return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_opacity: %zu entries for %zu materials", count, ctx->material_type_list.size());
	struct Key { int texture, channel, cut; size_t first_word; };
	std::vector<Key> keys; std::vector<int> mask_of_material(count, RT_INVALID);
	size_t total_words = 0;
	for (size_t i = 0; i < count; i++) {
		int id = texture_ids[i];
		if (id == RT_INVALID) continue;
		if (id < 0 || size_t(id) >= ctx->texture_records.size())
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_opacity: material %zu names texture %d of %zu", i, id, ctx->texture_records.size());
		if (ctx->texture_formats[id] != RT_TEXTURE_RGBA8)
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_opacity: material %zu names texture %d, which is not RT_TEXTURE_RGBA8", i, id);
		if (channels[i] < 0 || channels[i] > 3)
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_opacity: material %zu: channel %d is not in 0..3", i, channels[i]);
		if (!(thresholds[i] > 0.0f && thresholds[i] <= 1.0f))   // (false for NaN)
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_opacity: material %zu: threshold %.9g is not in (0, 1]", i, double(thresholds[i]));
		const RtTexture & t = ctx->texture_records[id];
		if ((long long)t.width * t.height >= (1ll << 30))
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_material_opacity: material %zu: texture %d has 2^30 texels or more", i, id);
		if (ctx->material_type_list[i] == RT_MATERIAL_LIGHT) continue;
		int cut = int(ceilf(thresholds[i] * 255.0f)); cut = cut < 0 ? 0 : (cut > 255 ? 255 : cut);
		size_t k = 0;
		while (k < keys.size() && !(keys[k].texture == id && keys[k].channel == channels[i] && keys[k].cut == cut)) k++;
		if (k == keys.size()) { keys.push_back({ id, channels[i], cut, total_words }); total_words += (size_t(t.width) * t.height + 31) / 32; }
		mask_of_material[i] = int(k);
	}
	int s = opacity_clear(ctx); if (s) return s;
	if (keys.empty()) { RT_HIP(ctx, quiesce(ctx)); return RT_OK; }
	RT_HIP(ctx, quiesce(ctx));
	s = device_alloc(ctx, &ctx->opacity_bits, total_words * 4); if (s) return s;
	std::vector<RtOpacityMask> masks(keys.size());
	for (size_t k = 0; k < keys.size(); k++) {
		const RtTexture & t = ctx->texture_records[keys[k].texture];
		int texel_count = t.width * t.height, word_count = (texel_count + 31) / 32;
		unsigned * words = (unsigned *)ctx->opacity_bits + keys[k].first_word;
		kernel_build_opacity_bits<<<unsigned((word_count + 255) / 256), 256, 0, ctx->stream>>>((const unsigned *)t.texels, words, texel_count, word_count, keys[k].channel, keys[k].cut);
		hipError_t e = hipGetLastError();
		if (e != hipSuccess) { (void)opacity_clear(ctx); return fail(ctx, RT_ERROR_HIP, "rt_upload_material_opacity: building the bits failed: %s", hipGetErrorString(e)); }
		masks[k] = { words, t.width, t.height };
	}
	hipError_t e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) { (void)opacity_clear(ctx); return fail(ctx, RT_ERROR_HIP, "rt_upload_material_opacity: building the bits failed: %s", hipGetErrorString(e)); }
	s = upload(ctx, &ctx->opacity_masks, masks.data(), masks.size() * sizeof(RtOpacityMask)); if (s) { (void)opacity_clear(ctx); return s; }
	s = upload(ctx, &ctx->material_opacity, mask_of_material.data(), count * sizeof(int)); if (s) { (void)opacity_clear(ctx); return s; }
	ctx->material_opacity_list = mask_of_material; ctx->opacity_mask_list = masks;
	ctx->params.material_opacity = (const int *)ctx->material_opacity;
	ctx->params.opacity_masks = (const RtOpacityMask *)ctx->opacity_masks;
	ctx->params.opacity_active = 1;
	return RT_OK;
}
int rt_read_material_opacity(rt_context * ctx, int material, uint32_t * words, size_t capacity_words, int32_t * out_width, int32_t * out_height) {
	RT_REQUIRE(ctx, ctx, "rt_read_material_opacity: NULL context");
	if (material < 0 || size_t(material) >= ctx->material_opacity_list.size() || ctx->material_opacity_list[material] == RT_INVALID)
		return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_material_opacity: material %d has no opacity mask", material);
	const RtOpacityMask & m = ctx->opacity_mask_list[ctx->material_opacity_list[material]];
	size_t word_count = (size_t(m.width) * m.height + 31) / 32;
	if (out_width) *out_width = m.width;
	if (out_height) *out_height = m.height;
	if (!words || capacity_words < word_count)
		return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_material_opacity: the %d x %d mask of material %d takes %zu words, capacity %zu", m.width, m.height, material, word_count, capacity_words);
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, hipMemcpy(words, m.bits, word_count * 4, hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_upload_media(rt_context * ctx, const void * media, size_t count) {
	RT_REQUIRE(ctx, ctx && (media || count == 0), "rt_upload_media: NULL argument");
	(void)hipSetDevice(ctx->device);
	int s = upload(ctx, &ctx->media, media, count * 32); if (s) return s;
	ctx->params.media = (const float4 *)ctx->media;
	ctx->medium_count = count;
	return RT_OK;
}

int rt_upload_textures(rt_context * ctx, const rt_texture_desc * descs, size_t count) {
	RT_REQUIRE(ctx, ctx && (descs || count == 0), "rt_upload_textures: NULL argument");
	(void)hipSetDevice(ctx->device);
	for (void * p : ctx->texture_data) device_free(ctx, p);
	ctx->texture_data.clear(); ctx->texture_bytes = 0; ctx->texture_formats.clear(); ctx->texture_records.clear();
	{ int cleared = opacity_clear(ctx); if (cleared) return cleared; }   // the masks were built from textures of the old table
	std::vector<RtTexture> table(count);
	for (size_t i = 0; i < count; i++) {
		const rt_texture_desc & d = descs[i];
		RT_REQUIRE(ctx, d.texels && d.width > 0 && d.height > 0 && d.mip_levels > 0, "rt_upload_textures: invalid texture descriptor");
		RT_REQUIRE(ctx, d.format == RT_TEXTURE_RGBA8 || d.format == RT_TEXTURE_BC1, "rt_upload_textures: unknown texture format");
		size_t bytes = 0;
		for (int l = 0; l < d.mip_levels; l++) {
			int w = d.width >> l; if (w < 1) w = 1; int h = d.height >> l; if (h < 1) h = 1;
			bytes += d.format == RT_TEXTURE_BC1 ? size_t((w + 3) / 4) * ((h + 3) / 4) * 8 : size_t(w) * h * 4;
		}
		void * dev = nullptr;
		int s = upload(ctx, &dev, d.texels, bytes); if (s) return s;
		int device_format = d.format;
		if (d.format == RT_TEXTURE_BC1 && ctx->expand_bc1) {   // decode every block once, here, instead of once per texel fetch
			void * expanded = nullptr;
			s = device_alloc(ctx, &expanded, bytes * 8); if (s) { device_free(ctx, dev); return s; }
			rt_launch_expand_bc1((const uint2 *)dev, (uchar4 *)expanded, bytes / 8, ctx->stream);
			hipError_t e = hipGetLastError(); if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
			device_free(ctx, dev);
			if (e != hipSuccess) { device_free(ctx, expanded); return fail(ctx, RT_ERROR_HIP, "rt_upload_textures: expanding BC1 blocks failed: %s", hipGetErrorString(e)); }
			dev = expanded; bytes *= 8; device_format = RT_TEXTURE_BC1_EXPANDED;
		}
		ctx->texture_data.push_back(dev);
		ctx->texture_bytes += bytes;
		table[i].texels = (const uchar4 *)dev;
		table[i].width = d.width; table[i].height = d.height; table[i].mip_levels = d.mip_levels;
		table[i].format = device_format; table[i].pad = 0;
		ctx->texture_formats.push_back(device_format);
		int lod_width  = d.lod_width  > 0 ? d.lod_width  : d.width;
		int lod_height = d.lod_height > 0 ? d.lod_height : d.height;
		table[i].lod_bias = 0.5f * log2f(float(lod_width * lod_height)); // Integrator.cpp:95
	}
	int s = upload(ctx, &ctx->texture_table, table.data(), count * sizeof(RtTexture)); if (s) return s;
	ctx->params.textures = (const RtTexture *)ctx->texture_table;
	ctx->texture_records = table;
	ctx->params.material_normal_maps = nullptr;   // the maps named textures of the old table
	ctx->params.normal_map_slots = 0;
	ctx->params.textures_compressed = 0;
	for (const RtTexture & t : table) if (t.format == RT_TEXTURE_BC1) ctx->params.textures_compressed = 1;
	return RT_OK;
}

int rt_upload_lights(rt_context * ctx,
                     const int32_t * light_triangle_indices, const float * light_triangle_cumulative_probability, size_t light_triangle_count,
                     const float * light_mesh_cumulative_probability, const int32_t * light_mesh_triangle_span,
                     const int32_t * light_mesh_transform_indices, size_t light_mesh_count, float lights_total_weight) {
	RT_REQUIRE(ctx, ctx, "rt_upload_lights: NULL context");
	int s = check_light_tables(ctx, light_triangle_indices, light_triangle_cumulative_probability, light_triangle_count,
	                           light_mesh_cumulative_probability, light_mesh_triangle_span, light_mesh_transform_indices, light_mesh_count, lights_total_weight);
	if (s) return s;   // (nothing staged: the tables uploaded before stay in force)
	if (ctx->light_tree_on && (s = light_tree_leaves_allowed(ctx, "rt_upload_lights", light_mesh_triangle_span, light_mesh_count))) return s;
	(void)hipSetDevice(ctx->device);
	// the per-mesh tables change with every TLAS rebuild (they are in TLAS order): versioned like the TLAS itself
	const void * src[5] = { light_triangle_indices, light_triangle_cumulative_probability, light_mesh_cumulative_probability, light_mesh_triangle_span, light_mesh_transform_indices };
	size_t bytes[5] = { light_triangle_count * 4, light_triangle_count * 4, light_mesh_count * 4, light_mesh_count * 8, light_mesh_count * 4 };
	size_t offset[6] = { 0 };
	for (int i = 0; i < 5; i++) offset[i + 1] = offset[i] + ((src[i] ? bytes[i] : 0) + 15) / 16 * 16;
	void * staging = nullptr;
	s = ring_begin(ctx, ctx->light_ring, offset[5], &staging); if (s) return s;
	for (int i = 0; i < 5; i++) if (src[i] && bytes[i]) memcpy((char *)staging + offset[i], src[i], bytes[i]);
	s = ring_commit(ctx, ctx->light_ring); if (s) return s;
	const char * base = (const char *)ctx->light_ring.device[ctx->light_ring.current];
	ctx->params.light_triangle_indices                = (const int *)(base + offset[0]);
	ctx->params.light_triangle_cumulative_probability = (const float *)(base + offset[1]);
	ctx->params.light_mesh_cumulative_probability     = (const float *)(base + offset[2]);
	ctx->params.light_mesh_triangle_span              = (const int2 *)(base + offset[3]);
	ctx->params.light_mesh_transform_indices          = (const int *)(base + offset[4]);
	ctx->params.light_mesh_count    = int(light_mesh_count);
	ctx->params.light_triangle_count = int(light_triangle_count);
	ctx->params.lights_total_weight = lights_total_weight;
	ctx->light_spans.assign(light_mesh_triangle_span, light_mesh_triangle_span + 2 * light_mesh_count);
	ctx->light_tree_dirty = true;
	return RT_OK;
}

// Delta emitters. Everything is checked before anything is staged: a refused table leaves the one before in force. The staged record
// carries what the kernels would otherwise compute per sample (the cosines, 1 / (cutoff - beam)) and the light's own selection probability, from the
// weights in double; the CDF is inclusive and normalised and ends in exactly 1 from the last light of positive weight on, so that binary_search ends
// for every number below 1 and never selects a light of zero weight that follows a positive one.
int rt_upload_delta_lights(rt_context * ctx, const rt_delta_light * records, size_t count, float share) {
	RT_REQUIRE(ctx, ctx, "rt_upload_delta_lights: NULL context");
	(void)hipSetDevice(ctx->device);
	if (!records || count == 0) {   // clear
		if (!ctx->delta_lights) return RT_OK;
		RT_HIP(ctx, quiesce(ctx));
		device_free(ctx, ctx->delta_lights); ctx->delta_lights = nullptr;
		ctx->delta_light_records.clear(); ctx->delta_light_cdf.clear(); ctx->delta_light_share = 0.0f;
		ctx->params.delta_lights = nullptr; ctx->params.delta_light_cdf = nullptr; ctx->params.delta_light_count = 0;
		ctx->params.delta_nee_share = 0.0f; ctx->params.nee_taken = ctx->params.sky_nee_share;   // (nothing is in flight; the next render settles the sky's share again)
		return RT_OK;
	}
	if (count > size_t(RT_MAX_DELTA_LIGHTS)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: %zu lights, more than RT_MAX_DELTA_LIGHTS (%d)", count, RT_MAX_DELTA_LIGHTS);
	if (!(share > 0.0f && share <= 1.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: share is %.9g, outside (0, 1]", double(share));
	const float pi = 3.14159265358979323846f;
	double total = 0.0;
	for (size_t i = 0; i < count; i++) {
		const rt_delta_light & l = records[i];
		if (l.type != RT_DELTA_LIGHT_POINT && l.type != RT_DELTA_LIGHT_SPOT && l.type != RT_DELTA_LIGHT_DIRECTIONAL)
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: light %zu: unknown type %d", i, l.type);
		for (int k = 0; k < 3; k++) {
			if (l.type != RT_DELTA_LIGHT_DIRECTIONAL && !std::isfinite(l.position[k])) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: light %zu: position is not finite", i);
			if (!(std::isfinite(l.intensity[k]) && l.intensity[k] >= 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: light %zu: intensity %d is %.9g (it must be finite and not negative)", i, k, double(l.intensity[k]));
		}
		if (l.type != RT_DELTA_LIGHT_POINT) {
			double n = double(l.direction[0]) * l.direction[0] + double(l.direction[1]) * l.direction[1] + double(l.direction[2]) * l.direction[2];
			if (!(std::isfinite(n) && n > 0.0)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: light %zu: direction is zero or not finite", i);
		}
		if (l.type == RT_DELTA_LIGHT_SPOT && !(l.beam > 0.0f && l.beam <= l.cutoff && l.cutoff <= pi))
			return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: light %zu: beam %.9g and cutoff %.9g do not satisfy 0 < beam <= cutoff <= pi", i, double(l.beam), double(l.cutoff));
		if (!(std::isfinite(l.weight) && l.weight >= 0.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: light %zu: weight is %.9g (it must be finite and not negative)", i, double(l.weight));
		total += double(l.weight);
	}
	if (!(std::isfinite(total) && total > 0.0)) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_upload_delta_lights: the total weight is %.9g (it must be finite and positive)", total);

	std::vector<float> staged(count * RT_DELTA_LIGHT_RECORD, 0.0f), cdf(count);
	size_t last_positive = 0;
	for (size_t i = 0; i < count; i++) if (records[i].weight > 0.0f) last_positive = i;
	double running = 0.0;
	for (size_t i = 0; i < count; i++) {
		const rt_delta_light & l = records[i];
		float * r = &staged[i * RT_DELTA_LIGHT_RECORD];
		const bool has_position = l.type != RT_DELTA_LIGHT_DIRECTIONAL, has_direction = l.type != RT_DELTA_LIGHT_POINT;
		for (int k = 0; k < 3; k++) r[k] = has_position ? l.position[k] : 0.0f;
		memcpy(&r[3], &l.type, 4);
		if (has_direction) {
			double n = sqrt(double(l.direction[0]) * l.direction[0] + double(l.direction[1]) * l.direction[1] + double(l.direction[2]) * l.direction[2]);
			for (int k = 0; k < 3; k++) r[4 + k] = float(double(l.direction[k]) / n);
		} else r[6] = 1.0f;
		r[7] = float(double(l.weight) / total);
		for (int k = 0; k < 3; k++) r[8 + k] = l.intensity[k];
		const bool spot = l.type == RT_DELTA_LIGHT_SPOT;
		r[11] = spot ? float(cos(double(l.cutoff))) : -1.0f;   // (in double, rounded once: the float64 restatement's own constants)
		r[12] = spot ? float(cos(double(l.beam))) : -1.0f;
		r[13] = spot ? l.cutoff : pi;
		r[14] = spot && l.cutoff > l.beam ? 1.0f / (l.cutoff - l.beam) : 0.0f;
		running += double(l.weight);
		cdf[i] = i >= last_positive ? 1.0f : float(running / total);
	}
	const size_t record_bytes = staged.size() * sizeof(float);
	std::vector<char> image(record_bytes + count * sizeof(float));
	memcpy(image.data(), staged.data(), record_bytes);
	memcpy(image.data() + record_bytes, cdf.data(), count * sizeof(float));
	int s = upload(ctx, &ctx->delta_lights, image.data(), image.size()); if (s) return s;   // (drains the context)
	ctx->params.delta_lights = (const RtDeltaLight *)ctx->delta_lights;
	ctx->params.delta_light_cdf = (const float *)((const char *)ctx->delta_lights + record_bytes);
	ctx->params.delta_light_count = int(count);
	ctx->delta_light_records.swap(staged); ctx->delta_light_cdf.swap(cdf); ctx->delta_light_share = share;
	return RT_OK;
}

int rt_read_delta_lights(rt_context * ctx, float * records, float * cdf, size_t capacity, size_t * out_count, float * out_share) {
	RT_REQUIRE(ctx, ctx, "rt_read_delta_lights: NULL context");
	const size_t count = ctx->delta_light_cdf.size();
	if (out_count) *out_count = count;
	if (out_share) *out_share = ctx->delta_light_share;
	if ((records || cdf) && capacity < count) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_delta_lights: room for %zu lights, the table holds %zu", capacity, count);
	if (records && count) memcpy(records, ctx->delta_light_records.data(), count * RT_DELTA_LIGHT_RECORD * sizeof(float));
	if (cdf && count) memcpy(cdf, ctx->delta_light_cdf.data(), count * sizeof(float));
	return RT_OK;
}

int rt_upload_rng(rt_context * ctx, const float * pmj_samples, const uint8_t * blue_noise) {
	RT_REQUIRE(ctx, ctx && pmj_samples && blue_noise, "rt_upload_rng: NULL argument");
	(void)hipSetDevice(ctx->device);
	int s = upload(ctx, &ctx->pmj, pmj_samples, size_t(RT_PMJ_NUM_SEQUENCES) * RT_PMJ_NUM_SAMPLES_PER_SEQUENCE * 8); if (s) return s;
	s = upload(ctx, &ctx->blue_noise, blue_noise, size_t(RT_BLUE_NOISE_NUM_TEXTURES) * RT_BLUE_NOISE_TEXTURE_DIM * RT_BLUE_NOISE_TEXTURE_DIM * 2); if (s) return s;
	ctx->params.pmj_samples = (const float2 *)ctx->pmj;
	ctx->params.blue_noise  = (const uchar2 *)ctx->blue_noise;
	ctx->luts_ready = false;
	return RT_OK;
}

int rt_set_sky(rt_context * ctx, const float * rgba, int width, int height, float scale) {
	RT_REQUIRE(ctx, ctx && rgba && width > 0 && height > 0, "rt_set_sky: invalid argument");
	(void)hipSetDevice(ctx->device);
	int s = upload(ctx, &ctx->sky, rgba, size_t(width) * height * 16); if (s) return s;
	ctx->params.sky = (const float4 *)ctx->sky;
	ctx->params.sky_width = width; ctx->params.sky_height = height; ctx->params.sky_scale = scale;
	// (upload drained the context) the sampling tables belong to the old sky
	device_free(ctx, ctx->sky_tables); device_free(ctx, ctx->sky_table_sums);
	ctx->sky_tables = ctx->sky_table_sums = nullptr;
	ctx->sky_tables_ready = false;
	ctx->params.sky_marginal_cdf = ctx->params.sky_conditional_cdf = ctx->params.sky_cell_pdf = nullptr;
	ctx->params.sky_nee_share = 0.0f;
	return RT_OK;
}

int rt_set_sky_sampling(rt_context * ctx, float probability) {
	RT_REQUIRE(ctx, ctx != nullptr, "rt_set_sky_sampling: NULL context");
	RT_REQUIRE(ctx, probability == 0.0f || (probability > 0.0f && probability <= 1.0f), "rt_set_sky_sampling: the probability must be 0 (off) or in (0, 1]");
	ctx->sky_sampling = probability;   // (takes effect at the next render, see sky_sampling_prepare)
	return RT_OK;
}
int rt_get_sky_sampling(const rt_context * ctx, float * out_probability) {
	if (!ctx || !out_probability) return fail(nullptr, RT_ERROR_INVALID_ARG, "rt_get_sky_sampling: NULL argument");
	*out_probability = ctx->sky_sampling;
	return RT_OK;
}

// The sky's sampling tables as the device built them (built here if no render or probe has wanted them yet: the state a render with sampling on leaves).
int rt_read_sky_tables(rt_context * ctx, int * out_width, int * out_height, float * marginal_cdf, float * conditional_cdf, float * cell_pdf,
                       double * row_totals, double * out_total, size_t capacity) {
	RT_REQUIRE(ctx, ctx, "rt_read_sky_tables: NULL context");
	RT_REQUIRE(ctx, ctx->params.sky, "rt_read_sky_tables: no sky uploaded (rt_set_sky)");
	const size_t w = size_t(ctx->params.sky_width), h = size_t(ctx->params.sky_height);
	if (out_width) *out_width = int(w);
	if (out_height) *out_height = int(h);
	if ((marginal_cdf || conditional_cdf || cell_pdf || row_totals) && capacity < w * h)
		return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_sky_tables: room for %zu cells, the %zux%zu sky has %zu", capacity, w, h, w * h);
	(void)hipSetDevice(ctx->device);
	int s = sky_tables_build(ctx, "rt_read_sky_tables"); if (s) return s;
	const float * tables = (const float *)ctx->sky_tables;
	const double * sums = (const double *)ctx->sky_table_sums;
	if (marginal_cdf)    RT_HIP(ctx, hipMemcpyAsync(marginal_cdf, tables, h * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	if (conditional_cdf) RT_HIP(ctx, hipMemcpyAsync(conditional_cdf, tables + h, w * h * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	if (cell_pdf)        RT_HIP(ctx, hipMemcpyAsync(cell_pdf, tables + h + w * h, w * h * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	if (row_totals)      RT_HIP(ctx, hipMemcpyAsync(row_totals, sums, h * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (out_total)       RT_HIP(ctx, hipMemcpyAsync(out_total, sums + h, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return RT_OK;
}

} // extern "C"

// The sky's sampling tables (kernels_sky.hip), built once per rt_set_sky; synchronous (it reads the total back).
int sky_tables_build(rt_context * ctx, const char * caller) {
	RtParams & p = ctx->params;
	if (!ctx->sky_tables_ready) {
		const size_t w = size_t(p.sky_width), h = size_t(p.sky_height);
		int s = device_alloc(ctx, &ctx->sky_tables, (h + 2 * w * h) * sizeof(float)); if (s) return s;
		s = device_alloc(ctx, &ctx->sky_table_sums, (h + 1) * sizeof(double)); if (s) return s;
		float * tables = (float *)ctx->sky_tables;
		double * sums = (double *)ctx->sky_table_sums;
		rt_launch_sky_build(p.sky, p.sky_width, p.sky_height, tables, tables + h, tables + h + w * h, sums, sums + h, ctx->stream);
		RT_HIP(ctx, hipGetLastError());
		RT_HIP(ctx, hipMemcpyAsync(&ctx->sky_total, sums + h, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
		RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
		p.sky_marginal_cdf = tables; p.sky_conditional_cdf = tables + h; p.sky_cell_pdf = tables + h + w * h;
		ctx->sky_tables_ready = true;
	}
	if (!std::isfinite(ctx->sky_total) || !std::isfinite(p.sky_scale))
		return fail(ctx, RT_ERROR_INVALID_ARG, "%s: sky sampling needs a finite sky (the %dx%d sky has NaN or infinite texels, or its scale is not finite)", caller, p.sky_width, p.sky_height);
	return RT_OK;
}

// Before a render: how this render splits its light samples. The sky's share (RtParams::sky_nee_share), building the tables if sampling is wanted:
// 0 -- sampling off, NEE off, or a sky without weight; all of them only when there is nothing else to sample, neither triangle emitters nor delta
// lights. The delta lights' share (RtParams::delta_nee_share): 0 without a table or with NEE off; the upload's share of what the sky
// leaves while triangle emitters exist; all the sky leaves without them. Both 0 keeps every kernel on the reference's estimator.
int sky_sampling_prepare(rt_context * ctx, const char * caller) {
	RtParams & p = ctx->params;
	{ int s = light_tree_refresh(ctx, caller); if (s) return s; }   // (the light tree follows the uploads since the last launch: one drain and one build, however many they were)
	light_tree_fog_warning(ctx);   // (a fog volume displaces the light tree: said once)
	const bool emitters = p.lights_total_weight > 0.0f;
	const bool delta = p.delta_light_count > 0 && p.config.enable_next_event_estimation;
	float share = 0.0f;
	if (ctx->sky_sampling > 0.0f && p.config.enable_next_event_estimation) {
		int s = sky_tables_build(ctx, caller); if (s) return s;
		if (ctx->sky_total > 0.0 && p.sky_scale != 0.0f) share = emitters || delta ? ctx->sky_sampling : 1.0f;
	}
	float delta_share = 0.0f, taken = share;
	if (delta) {
		delta_share = emitters ? (1.0f - share) * ctx->delta_light_share : 1.0f - share;
		taken = emitters ? fminf(share + delta_share, 1.0f) : 1.0f;
		// A share of 1 (or next to it) leaves the emitters nothing: s + (1 - s) may round to the float below 1, and a light sample that reached the emitters
		// with probability 6e-8 would carry a weight of 1.7e7. Then taken IS 1: the emitters are found by BSDF sampling alone (sort_rays: count_light).
		if (ctx->delta_light_share >= 1.0f || taken >= 0x1.fffffep-1f) { taken = 1.0f; delta_share = 1.0f - share; }
	}
	if (share != p.sky_nee_share || delta_share != p.delta_nee_share || taken != p.nee_taken) {
		RT_HIP(ctx, quiesce(ctx));   // (paths in flight were shaded under the other estimator)
		p.sky_nee_share = share; p.delta_nee_share = delta_share; p.nee_taken = taken;
	}
	return RT_OK;
}

int ensure_luts(rt_context * ctx) {
	if (ctx->luts_ready) return RT_OK;
	const size_t bytes[6] = { 4096 * 4, 4096 * 4, 256 * 4, 256 * 4, 1024 * 4, 32 * 4 };
	for (int i = 0; i < 6; i++) if (!ctx->luts[i]) { int s = device_alloc(ctx, &ctx->luts[i], bytes[i]); if (s) return s; }
	RtParams & p = ctx->params;
	rt_launch_integrate_luts(p, (float *)ctx->luts[0], (float *)ctx->luts[1], (float *)ctx->luts[2], (float *)ctx->luts[3], (float *)ctx->luts[4], (float *)ctx->luts[5], ctx->stream);
	RT_HIP(ctx, hipGetLastError());
	p.lut_dielectric_directional_albedo_enter = (const float *)ctx->luts[0];
	p.lut_dielectric_directional_albedo_leave = (const float *)ctx->luts[1];
	p.lut_dielectric_albedo_enter             = (const float *)ctx->luts[2];
	p.lut_dielectric_albedo_leave             = (const float *)ctx->luts[3];
	p.lut_conductor_directional_albedo        = (const float *)ctx->luts[4];
	p.lut_conductor_albedo                    = (const float *)ctx->luts[5];
	ctx->luts_ready = true;
	RT_HIP(ctx, quiesce(ctx)); // once per context: the sample streams read the tables without further ordering
	return RT_OK;
}
