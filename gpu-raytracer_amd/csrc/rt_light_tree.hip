// rt_light_tree.hip -- the part of the C ABI (include/gpu_raytracer_amd.h) that is the light tree of next-event estimation: the switch, the
// rebuild behind every upload the tree depends on, the read-back and the two probes. The build itself: kernels_light_tree.hip; what the kernels read: rt_light_tree.h.
#include "rt_context.h"

#include <cmath>
#include <cstdio>
#include <cstring>

// The leaves the spans of a set of light tables make: one per (entry, triangle of its span). Refused above RT_MAX_LIGHT_TREE_LEAVES.
static size_t light_tree_count(const int32_t * spans, size_t entries) {
	size_t n = 0;
	for (size_t m = 0; m < entries; m++) n += size_t(spans[2 * m + 1] - spans[2 * m] + 1);   // (rt_upload_lights has checked first <= last)
	return n;
}
int light_tree_leaves_allowed(rt_context * ctx, const char * caller, const int32_t * spans, size_t entries) {
	const size_t n = light_tree_count(spans, entries);
	if (n > size_t(RT_MAX_LIGHT_TREE_LEAVES))
		return fail(ctx, RT_ERROR_INVALID_ARG, "%s: the light tables make %zu leaves of the light tree, more than RT_MAX_LIGHT_TREE_LEAVES (%d)", caller, n, RT_MAX_LIGHT_TREE_LEAVES);
	return RT_OK;
}

static void light_tree_drop(rt_context * ctx) {
	device_free(ctx, ctx->light_tree_memory); ctx->light_tree_memory = nullptr;
	ctx->params.light_tree = RtLightTree{ };
}

// Called before every launch or read-back that uses the tree (the render preamble, the launch probes, rt_read_light_tree, the two tree probes, rt_set_light_tree). If
// an upload the tree depends on has come since it was built: builds the tree the context's scene makes, if the tree is wanted and everything it reads is there;
// otherwise no tree is in force (the plain kernels run). The uploads themselves only mark the tree: a scene update of several uploads costs one drain and one build,
// the build never sees one upload's tables beside another's stale ones, and no upload fails after it has taken effect. Drains the context first: paths in flight
// were shaded under the tree before, or under none -- and they read the scene versions that tree was built from.
int light_tree_refresh(rt_context * ctx, const char * caller) {
	if (!ctx->light_tree_dirty) return RT_OK;
	ctx->light_tree_dirty = false;
	if (!ctx->light_tree_on && !ctx->light_tree_memory) return RT_OK;
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	light_tree_drop(ctx);
	if (!ctx->light_tree_on) return RT_OK;
	const RtParams & p = ctx->params;
	const size_t entries = ctx->light_spans.size() / 2, N = light_tree_count(ctx->light_spans.data(), entries);
	if (N == 0 || N > size_t(RT_MAX_LIGHT_TREE_LEAVES) || int(entries) != p.light_mesh_count) return RT_OK;
	if (!p.triangles || !p.mesh_transforms || !p.mesh_material_ids || !p.materials || !p.material_types || ctx->mesh_count == 0 || ctx->triangle_count == 0) return RT_OK;
	size_t M = 1; while (M < N) M *= 2;

	size_t at = 0;
	auto region = [&](size_t bytes) { const size_t begin = at; at += (bytes + 255) / 256 * 256; return begin; };
	const size_t o_nodes = region((2 * M - 1) * 32), o_leaves = region(N * 16), o_leaf_of_slot = region(M * 4), o_slot_of_leaf = region(N * 4), o_leaf_base = region((entries + 1) * 4),
	             o_entry_of_mesh = region(ctx->mesh_count * 4), o_place_of_triangle = region(ctx->triangle_count * 4);
	const size_t tree_bytes = at;
	const size_t sort_bytes = rt_light_tree_sort_scratch_bytes(N);
	at = 0;
	const size_t s_leaf_nodes = region(N * 32), s_scene_box = region(32), s_keys = region(N * 8), s_sorted_keys = region(N * 8), s_ids = region(N * 4), s_sorted_ids = region(N * 4), s_sort = region(sort_bytes);
	const size_t scratch_bytes = at;

	void * memory = nullptr, * scratch = nullptr;
	int s = device_alloc(ctx, &memory, tree_bytes); if (s) return s;
	if (hipMalloc(&scratch, scratch_bytes) != hipSuccess) { device_free(ctx, memory); return fail(ctx, RT_ERROR_HIP, "%s: the light tree's build scratch (%zu bytes) could not be allocated", caller, scratch_bytes); }
	std::vector<int32_t> leaf_base(entries + 1, 0);
	for (size_t m = 0; m < entries; m++) leaf_base[m + 1] = leaf_base[m] + (ctx->light_spans[2 * m + 1] - ctx->light_spans[2 * m] + 1);
	char * base = (char *)memory, * tmp = (char *)scratch;

	LightTreeBuildArgs a = { };
	a.triangles = p.triangles; a.mesh_transforms = p.mesh_transforms; a.mesh_position = p.mesh_position; a.mesh_material_ids = p.mesh_material_ids;
	a.material_types = p.material_types; a.materials = p.materials;
	a.light_triangle_indices = p.light_triangle_indices; a.light_mesh_triangle_span = p.light_mesh_triangle_span; a.light_mesh_transform_indices = p.light_mesh_transform_indices;
	a.light_mesh_count = int(entries); a.mesh_count = int(ctx->mesh_count); a.triangle_count = int(ctx->triangle_count); a.material_count = int(ctx->material_type_list.size());
	a.nodes = (float4 *)(base + o_nodes); a.leaves = (float4 *)(base + o_leaves); a.leaf_of_slot = (int *)(base + o_leaf_of_slot); a.slot_of_leaf = (int *)(base + o_slot_of_leaf);
	a.entry_of_mesh = (int *)(base + o_entry_of_mesh); a.place_of_triangle = (int *)(base + o_place_of_triangle); a.leaf_base = (const int *)(base + o_leaf_base);
	a.leaf_count = int(N); a.padded = int(M);
	a.leaf_nodes = (float4 *)(tmp + s_leaf_nodes); a.scene_box = (int *)(tmp + s_scene_box); a.keys = (uint64_t *)(tmp + s_keys); a.sorted_keys = (uint64_t *)(tmp + s_sorted_keys);
	a.ids = (int *)(tmp + s_ids); a.sorted_ids = (int *)(tmp + s_sorted_ids); a.sort_scratch = tmp + s_sort; a.sort_scratch_bytes = sort_bytes;

	hipError_t e = hipMemcpyAsync(base + o_leaf_base, leaf_base.data(), (entries + 1) * 4, hipMemcpyHostToDevice, ctx->stream);   // (main stream: behind the uploads the build reads)
	if (e == hipSuccess) e = rt_light_tree_build(a, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	(void)hipFree(scratch);
	if (e != hipSuccess) { device_free(ctx, memory); return fail(ctx, RT_ERROR_HIP, "%s: building the light tree failed: %s", caller, hipGetErrorString(e)); }

	ctx->light_tree_memory = memory;
	RtLightTree & t = ctx->params.light_tree;
	t.nodes = a.nodes; t.leaves = a.leaves; t.leaf_of_slot = a.leaf_of_slot; t.slot_of_leaf = a.slot_of_leaf; t.leaf_base = a.leaf_base;
	t.entry_of_mesh = a.entry_of_mesh; t.place_of_triangle = a.place_of_triangle; t.leaf_count = int(N); t.padded = int(M);
	return RT_OK;
}

// A fog volume displaces the tree (known limits): said once per context, at the first render that meets both.
void light_tree_fog_warning(rt_context * ctx) {
	if (ctx->light_tree_fog_warned || !(ctx->params.light_tree.padded > 0 && ctx->params.fog_active)) return;
	ctx->light_tree_fog_warned = true;
	fprintf(stderr, "gpu_raytracer_amd: a fog volume is active: the light tree is not used (the emitters are selected by power, as without rt_set_light_tree)\n");
}

int rt_set_light_tree(rt_context * ctx, int enable) {
	RT_REQUIRE(ctx, ctx, "rt_set_light_tree: NULL context");
	RT_REQUIRE(ctx, enable == 0 || enable == 1, "rt_set_light_tree: enable must be 0 or 1");
	if ((enable != 0) == ctx->light_tree_on) return RT_OK;
	if (enable) {
		int s = light_tree_leaves_allowed(ctx, "rt_set_light_tree", ctx->light_spans.data(), ctx->light_spans.size() / 2); if (s) return s;
	}
	ctx->light_tree_on = enable != 0;
	ctx->light_tree_dirty = true;
	int s = light_tree_refresh(ctx, "rt_set_light_tree");
	if (s) { ctx->light_tree_on = false; ctx->light_tree_dirty = true; (void)light_tree_refresh(ctx, "rt_set_light_tree"); }
	return s;
}

int rt_get_light_tree(rt_context * ctx) { return ctx && ctx->light_tree_on ? 1 : 0; }

int rt_read_light_tree(rt_context * ctx, int32_t * out_leaf_count, int32_t * out_padded, float * nodes, size_t node_capacity, uint32_t * leaves, int32_t * slot_of_leaf, size_t leaf_capacity,
                       int32_t * entry_of_mesh, size_t mesh_capacity, int32_t * place_of_triangle, size_t triangle_capacity) {
	RT_REQUIRE(ctx, ctx, "rt_read_light_tree: NULL context");
	RT_REQUIRE(ctx, out_leaf_count && out_padded, "rt_read_light_tree: NULL out_leaf_count or out_padded");
	{ int s = light_tree_refresh(ctx, "rt_read_light_tree"); if (s) return s; }
	const RtLightTree & t = ctx->params.light_tree;
	const size_t N = size_t(t.leaf_count), M = size_t(t.padded), node_count = M ? 2 * M - 1 : 0;
	if (nodes && node_capacity < node_count) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_light_tree: room for %zu nodes, the tree holds %zu", node_capacity, node_count);
	if ((leaves || slot_of_leaf) && leaf_capacity < N) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_light_tree: room for %zu leaves, the tree holds %zu", leaf_capacity, N);
	if (M && entry_of_mesh && mesh_capacity < ctx->mesh_count) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_light_tree: room for %zu instances, the scene holds %zu", mesh_capacity, ctx->mesh_count);
	if (M && place_of_triangle && triangle_capacity < ctx->triangle_count) return fail(ctx, RT_ERROR_INVALID_ARG, "rt_read_light_tree: room for %zu triangles, the scene holds %zu", triangle_capacity, ctx->triangle_count);
	*out_leaf_count = int32_t(N); *out_padded = int32_t(M);
	if (M == 0) return RT_OK;
	(void)hipSetDevice(ctx->device);
	RT_HIP(ctx, quiesce(ctx));
	if (nodes)             RT_HIP(ctx, hipMemcpy(nodes, t.nodes, node_count * 32, hipMemcpyDeviceToHost));
	if (leaves)            RT_HIP(ctx, hipMemcpy(leaves, t.leaves, N * 16, hipMemcpyDeviceToHost));
	if (slot_of_leaf)      RT_HIP(ctx, hipMemcpy(slot_of_leaf, t.slot_of_leaf, N * 4, hipMemcpyDeviceToHost));
	if (entry_of_mesh)     RT_HIP(ctx, hipMemcpy(entry_of_mesh, t.entry_of_mesh, ctx->mesh_count * 4, hipMemcpyDeviceToHost));
	if (place_of_triangle) RT_HIP(ctx, hipMemcpy(place_of_triangle, t.place_of_triangle, ctx->triangle_count * 4, hipMemcpyDeviceToHost));
	return RT_OK;
}

// The two probes share their checks: a tree must exist, every number of a probe must be what the device functions expect.
static int light_tree_probe(rt_context * ctx, const char * name, bool sample, const float * probes, size_t count, float * out) {
	if (!ctx || !probes || !out) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: NULL argument", name);
	if (count > size_t(1) << 24) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: more than 2^24 probes", name);
	{ int s = light_tree_refresh(ctx, name); if (s) return s; }
	const RtLightTree & t = ctx->params.light_tree;
	if (t.padded <= 0) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: no light tree exists (rt_set_light_tree(ctx, 1) on a scene with triangle emitters)", name);
	const size_t in = sample ? 5 : 4, out_words = sample ? 4 : 1;
	for (size_t i = 0; i < count; i++) {
		const float * a = probes + i * in;
		if (sample) {
			for (int k = 0; k < 2; k++) if (!(a[k] >= 0.0f && a[k] < 1.0f)) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: probe %zu: random number %d is %.9g, outside [0, 1)", name, i, k, double(a[k]));
		} else {
			int32_t leaf; memcpy(&leaf, a, 4);
			if (leaf < 0 || leaf >= t.leaf_count) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: probe %zu: leaf %d outside [0, %d)", name, i, leaf, t.leaf_count);
		}
		const float * point = a + (sample ? 2 : 1);
		if (!(std::isfinite(point[0]) && std::isfinite(point[1]) && std::isfinite(point[2]))) return fail(ctx, RT_ERROR_INVALID_ARG, "%s: probe %zu: the point is not finite", name, i);
	}
	if (count == 0) return RT_OK;
	(void)hipSetDevice(ctx->device);
	void * dev_probes = nullptr, * dev_out = nullptr;
	hipError_t e = hipMalloc(&dev_probes, count * in * 4);
	if (e == hipSuccess) e = hipMalloc(&dev_out, count * out_words * 4);
	if (e == hipSuccess) e = hipMemcpy(dev_probes, probes, count * in * 4, hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		if (sample) rt_launch_light_tree_sample(t, (const float *)dev_probes, int(count), (float *)dev_out, ctx->stream);
		else rt_launch_light_tree_pmf(t, (const float *)dev_probes, int(count), (float *)dev_out, ctx->stream);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = quiesce(ctx);
	if (e == hipSuccess) e = hipMemcpy(out, dev_out, count * out_words * 4, hipMemcpyDeviceToHost);
	(void)hipFree(dev_probes); (void)hipFree(dev_out);
	if (e != hipSuccess) return fail(ctx, RT_ERROR_HIP, "%s failed: %s", name, hipGetErrorString(e));
	return RT_OK;
}
int rt_sample_light_tree(rt_context * ctx, const float * probes, size_t count, float * out) { return light_tree_probe(ctx, "rt_sample_light_tree", true, probes, count, out); }
int rt_light_tree_pmf(rt_context * ctx, const float * probes, size_t count, float * out) { return light_tree_probe(ctx, "rt_light_tree_pmf", false, probes, count, out); }
