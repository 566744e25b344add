// rt_surface.h -- what the kernel families that came out of one shade unit share of a hit and of the queues: the launch-shape knobs, the packed hit,
// the triangle getters, the SVGF g-buffer store, the material queue's store and the per-submission statistics of the merged wavefront.
// Included by kernels_generate.hip, kernels_sort.hip, kernels_material_*.hip, kernels_probes.hip and kernels_list.hip.
//
// Differences from the reference's kernels (CUDA/Pathtracer.cu) that are design, not behaviour:
//   * every queue append (next ray, shadow ray, material queue) is ONE returning atomic per
//     64-lane wave (wave_aggregated_append) instead of one per thread;
//   * kernels are grid-stride loops over a fixed grid sized to the machine, so that the deep,
//     nearly empty bounces do not launch ~3000 idle workgroups;
//   * albedo / sky / LUT fetches go through the software texture unit in rt_shading.h.
#pragma once
#include "rt_shading.h"

#ifndef RT_SHADE_BLOCK
#define RT_SHADE_BLOCK 256
#endif
#ifndef RT_SHADE_WAVES
// The material kernels wait on scattered triangle / texture / light-table reads; left alone the compiler uses 129-140 VGPRs
// (3 waves per SIMD). Asking for 4 waves caps them at 128 registers: one more wave to hide the latency behind.
#define RT_SHADE_WAVES 4
#endif
#ifndef RT_SHADE_ONE_APPEND
#define RT_SHADE_ONE_APPEND 1   // 1: the shadow-ray and the continuation-ray append of a shade round share barriers and atomic latency (block_bucketed_append2)
#endif
#ifndef RT_OCTANT_BUCKETS
#define RT_OCTANT_BUCKETS 1   // a shade workgroup appends its rays ordered by direction octant (rt_math.h: block_bucketed_append)
#endif
#if RT_OCTANT_BUCKETS
#define RT_RAY_BUCKET(d) direction_octant(d)
#else
#define RT_RAY_BUCKET(d) 0u
#endif
#ifndef RT_SORT_BLOCK
#define RT_SORT_BLOCK 1024  // kernel_sort: 16 waves share one atomic per material queue (256: 0.230 ms per step, 512: 0.143, 1024: 0.138; profiles/r04_shade_stage.txt)
#endif
#ifndef RT_SORT_WAVES
// Waves per SIMD asked of the sort kernels' register allocation. The kernel is a chain of dependent gathers (queue entry -> slot table -> sample
// tables of the roulette; hit -> instance material -> material type) at a fifth of the vector ALUs: what it needs is rays in flight. 8 = 64
// registers (the general form takes 100: one 1024-thread workgroup per CU, 4 waves per SIMD), two workgroups per CU; the 128 bytes of scratch
// that costs sit in the branches Sponza never takes (media, emitters seen by a BSDF ray). Measured, one box: sort 0.135 -> 0.103 ms per step
// (profiles/r04_shade_stage.txt, 5.); 512-thread workgroups at 6 waves (80 registers): 0.165.
#define RT_SORT_WAVES 8
#endif
#ifndef RT_STREAM_SHADE_GRID
#define RT_STREAM_SHADE_GRID 8192   // workgroups of the grid-stride shade launches of the merged wavefront: 2 048 (two rounds of
                                    // resident workgroups) left 2.7 of 4 waves per SIMD resident on average; 8 192: shade stage -9 %, step -2.4 %
#endif
#ifndef RT_STREAM_SORT_GRID
#define RT_STREAM_SORT_GRID 2048    // ... and of its sort launch (in units of RT_SHADE_BLOCK threads)
#endif

struct HitInfo { float t, u, v; int mesh_id, triangle_id; };

RT_DEV HitInfo unpack_hit(uint4 h) { // Buffers.h:34-48
	HitInfo r;
	r.mesh_id = int(h.x); r.triangle_id = int(h.y);
	r.t = __uint_as_float(h.z);
	r.u = float(h.w & 0xffffu) / 65535.0f;
	r.v = float(h.w >> 16)     / 65535.0f;
	return r;
}

struct TriangleFull {
	f3 position_0, position_edge_1, position_edge_2;
	f3 normal_0, normal_edge_1, normal_edge_2;
	f2 tex_coord_0, tex_coord_edge_1, tex_coord_edge_2;
};
RT_DEV void triangle_get_positions(const RtParams & p, int index, f3 & p0, f3 & e1, f3 & e2) {
	const float4 * t = p.triangles + size_t(index) * 6;
	float4 a = t[0], b = t[1], c = t[2];
	p0 = mk3(a.x, a.y, a.z); e1 = mk3(a.w, b.x, b.y); e2 = mk3(b.z, b.w, c.x);
}
RT_DEV TriangleFull triangle_get_full(const RtParams & p, int index) {
	const float4 * t = p.triangles + size_t(index) * 6;
	float4 a = t[0], b = t[1], c = t[2], d = t[3], e = t[4], f = t[5];
	TriangleFull r;
	r.position_0 = mk3(a.x, a.y, a.z); r.position_edge_1 = mk3(a.w, b.x, b.y); r.position_edge_2 = mk3(b.z, b.w, c.x);
	r.normal_0 = mk3(c.y, c.z, c.w); r.normal_edge_1 = mk3(d.x, d.y, d.z); r.normal_edge_2 = mk3(d.w, e.x, e.y);
	r.tex_coord_0 = mk2(e.z, e.w); r.tex_coord_edge_1 = mk2(f.x, f.y); r.tex_coord_edge_2 = mk2(f.z, f.w);
	return r;
}
RT_DEV f3 barycentric(float u, float v, f3 base, f3 e1, f3 e2) { return base + u * e1 + v * e2; }
RT_DEV f2 barycentric(float u, float v, f2 base, f2 e1, f2 e2) { return base + u * e1 + v * e2; }

RT_DEV f3 m_position(const float4 * m, f3 v) {
	float4 r0 = m[0], r1 = m[1], r2 = m[2];
	return mk3(r0.x * v.x + r0.y * v.y + r0.z * v.z + r0.w, r1.x * v.x + r1.y * v.y + r1.z * v.z + r1.w, r2.x * v.x + r2.y * v.y + r2.z * v.z + r2.w);
}
RT_DEV f3 m_direction(const float4 * m, f3 v) {
	float4 r0 = m[0], r1 = m[1], r2 = m[2];
	return mk3(r0.x * v.x + r0.y * v.y + r0.z * v.z, r1.x * v.x + r1.y * v.y + r1.z * v.z, r2.x * v.x + r2.y * v.y + r2.z * v.z);
}

// SVGF g-buffers (CUDA/SVGF/SVGF.h:61-84)
RT_DEV f2 oct_encode_normal(f3 n) {
	n /= (fabsf(n.x) + fabsf(n.y) + fabsf(n.z));
	if (n.z < 0.0f) {
		n.x = (1.0f - fabsf(n.y)) * (n.x >= 0.0f ? +1.0f : -1.0f);
		n.y = (1.0f - fabsf(n.x)) * (n.y >= 0.0f ? +1.0f : -1.0f);
	}
	return mk2(0.5f + 0.5f * n.x, 0.5f + 0.5f * n.y);
}
RT_DEV f4 mat4_mul(const float * m, f4 v) {
	return mk4(
		m[ 0] * v.x + m[ 1] * v.y + m[ 2] * v.z + m[ 3] * v.w,
		m[ 4] * v.x + m[ 5] * v.y + m[ 6] * v.z + m[ 7] * v.w,
		m[ 8] * v.x + m[ 9] * v.y + m[10] * v.z + m[11] * v.w,
		m[12] * v.x + m[13] * v.y + m[14] * v.z + m[15] * v.w);
}
RT_DEV void svgf_set_gbuffers(const RtParams & p, int x, int y, const HitInfo & hit, f3 hit_point, f3 normal, f3 hit_point_prev) {
	f4 u_curr = mat4_mul(p.view_projection,      mk4(hit_point.x, hit_point.y, hit_point.z, 1.0f));
	f4 u_prev = mat4_mul(p.view_projection_prev, mk4(hit_point_prev.x, hit_point_prev.y, hit_point_prev.z, 1.0f));
	f2 oct = oct_encode_normal(normal);
	int idx = x + y * p.screen_pitch;
	p.gbuffer_normal_and_depth[idx] = make_float4(oct.x, oct.y, u_curr.z, u_prev.z);
	p.gbuffer_mesh_id_and_triangle_id[idx] = make_int2(hit.mesh_id, hit.triangle_id);
	p.gbuffer_screen_position_prev[idx] = make_float2(u_prev.x / u_prev.w, u_prev.y / u_prev.w);
}

// first_throughput (the ..._fog sort instances): the throughput of bounce 0 is stored too -- the first segment may have lost some in the fog, and shade_material reads it while fog_active
template<bool FIRST_THROUGHPUT = false>
RT_DEV void material_queue_store(const RtParams & p, int slot, int index_out, int bounce, f3 ray_direction, int medium_id, float cone_angle, float cone_width, uint4 hit, int pixel_index, f3 throughput) {
	const RtMaterialBuffer & q = p.material[slot];
	store3(q.direction, index_out, ray_direction);
	if (medium_id != RT_INVALID) q.medium[index_out] = medium_id;
	if (bounce > 0 && p.config.enable_mipmapping) { q.cone_angle[index_out] = cone_angle; q.cone_width[index_out] = cone_width; }
	q.hits[index_out] = hit;
	unsigned flags = unsigned(medium_id != RT_INVALID) << 30;
	q.pixel_index_and_flags[index_out] = unsigned(pixel_index) | flags;
	if (FIRST_THROUGHPUT || bounce > 0) store3(q.throughput, index_out, throughput);
}

// ---- per-submission statistics of the merged wavefront ------------------------------------------------------
// Rays per (submission, queue kind, bounce), what rt_get_counters reports. A workgroup tallies in LDS -- per wave one
// LDS add for every distinct submission among its lanes (queues are mostly sorted by submission, so usually one) --
// and flushes its non-zero cells with one global add each when it is done.
struct StreamStatsLDS { int count[RT_STREAM_SUBMISSIONS][RT_STAT_KINDS]; };

RT_DEV void stream_stats_clear(StreamStatsLDS & lds) {
	for (int i = threadIdx.x; i < RT_STREAM_SUBMISSIONS * RT_STAT_KINDS; i += blockDim.x) (&lds.count[0][0])[i] = 0;
	__syncthreads();
}
// called in converged or diverged flow by any subset of lanes: lanes with `counted` add one to (submission, kind)
RT_DEV void stream_stats_add(StreamStatsLDS & lds, bool counted, int submission, int kind) {
	unsigned long long remaining = __ballot(counted);
	while (remaining) {
		int leader = __ffsll((long long)remaining) - 1;
		int s = __shfl(submission, leader);
		unsigned long long same = __ballot(counted && submission == s) & remaining;
		if (int(lane_id()) == leader) atomicAdd(&lds.count[s][kind], __popcll(same));
		remaining &= ~same;
	}
}
RT_DEV void stream_stats_flush(const RtParams & p, StreamStatsLDS & lds) {
	__syncthreads();
	for (int i = threadIdx.x; i < RT_STREAM_SUBMISSIONS * RT_STAT_KINDS; i += blockDim.x) {
		int n = (&lds.count[0][0])[i];
		if (n == 0) continue;
		int submission = i / RT_STAT_KINDS, kind = i % RT_STAT_KINDS;
		int bounce = p.stream_iteration - p.stream_table->submission_birth[submission];
		if (bounce >= 0 && bounce < RT_MAX_BOUNCES) atomicAdd(&p.stream->stats[submission][kind][bounce], n);
	}
}
