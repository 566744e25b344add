// kernels_probes.hip -- the test probes of the shading code: the software texture unit, the BSDFs, light and delta-light sampling and normal maps,
// each on caller-supplied records through the very functions the sort and material kernels call (rt_probes.hip is their C ABI). The probe of
// the random numbers, kernel_random, is in kernels_generate.hip.
#include "rt_bsdf.h"
#include "rt_lights.h"

// rt_sample_texture / rt_sample_table / rt_sample_sky: the software texture unit on caller-supplied coordinates, through the very
// functions the shade kernels call. args: 8 floats per probe {s, t, lod, dx.x, dx.y, dy.x, dy.y, pad}; filter 0 texture_get,
// 1 texture_get_lod, 2 texture_get_grad. COMPRESSED is picked from p.textures_compressed as rt_launch_material does.
template<bool COMPRESSED>
__global__ void kernel_sample_texture(RtParams p, int texture_index, int filter, const float * args, int count, float4 * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const RtTexture tex = p.textures[texture_index];
	const float * a = args + size_t(i) * 8;
	f4 c = filter == 0 ? texture_get<COMPRESSED>(tex, a[0], a[1])
	     : filter == 1 ? texture_get_lod<COMPRESSED>(tex, a[0], a[1], a[2])
	     :               texture_get_grad<COMPRESSED>(tex, a[0], a[1], mk2(a[3], a[4]), mk2(a[5], a[6]));
	out[i] = make_float4(c.x, c.y, c.z, c.w);
}
// dims 1..3: lut_get_1d / _2d / _3d; coords: 3 floats per probe {s, t, r}
__global__ void kernel_sample_table(const float * table, int nx, int ny, int nz, int dims, const float * coords, int count, float * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * c = coords + size_t(i) * 3;
	out[i] = dims == 1 ? lut_get_1d(table, nx, c[0]) : dims == 2 ? lut_get_2d(table, nx, ny, c[0], c[1]) : lut_get_3d(table, nx, ny, nz, c[0], c[1], c[2]);
}
__global__ void kernel_sample_sky(RtParams p, const float * directions, int count, float * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * d = directions + size_t(i) * 3;
	f3 c = sample_sky(p, mk3(d[0], d[1], d[2]));
	out[3 * size_t(i)] = c.x; out[3 * size_t(i) + 1] = c.y; out[3 * size_t(i) + 2] = c.z;
}

// rt_bsdf_eval / rt_bsdf_sample: one BSDF set up as set_up_surface sets it up, then its own eval or sample. Probe i reads material i
// of p.materials (the per-call table rt_probes.hip uploads). Record in: RT_BSDF_PROBE_IN floats {material[8], normal[3], direction[3],
// entering, to_light[3], cos_theta_o, pixel, sample, bounce (uint32 bits), pad[2]}; out: RT_BSDF_PROBE_OUT floats {ok (1, 0, or -1:
// omega_i.z <= 0), pdf, bsdf or throughput[3], direction out[3], medium id, allow_nee, omega_i.z, pad}.
template<typename BSDF, bool EVAL>
__global__ void kernel_bsdf_probe(RtParams p, const float * probes, int count, float * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * a = probes + size_t(i) * RT_BSDF_PROBE_IN;
	float * o = out + size_t(i) * RT_BSDF_PROBE_OUT;
	for (int k = 0; k < RT_BSDF_PROBE_OUT; k++) o[k] = 0.0f;
	f3 normal = mk3(a[8], a[9], a[10]), ray_direction = mk3(a[11], a[12], a[13]);
	bool entering_material = a[14] != 0.0f;
	f3 tangent, bitangent;
	orthonormal_basis(normal, tangent, bitangent);
	f3 omega_i = world_to_local(-ray_direction, tangent, bitangent, normal);
	o[10] = omega_i.z;
	if (omega_i.z <= 0.0f) { o[0] = -1.0f; return; }

	unsigned pixel_index = __float_as_uint(a[19]), sample_index = __float_as_uint(a[20]), bounce = __float_as_uint(a[21]);
	BSDF bsdf;
	bsdf.pixel_index = int(pixel_index); bsdf.bounce = int(bounce); bsdf.sample_index = int(sample_index); bsdf.rng = random_path(p, pixel_index, sample_index);
	bsdf.tangent = tangent; bsdf.bitangent = bitangent; bsdf.normal = normal; bsdf.omega_i = omega_i;
	bsdf.init(p, entering_material, i);
	f3 throughput = mk3(1.0f);
	if (BSDF::HAS_ALBEDO) {
		TextureLOD lod = { mk2(0.0f, 0.0f), mk2(0.0f, 0.0f), 0.0f };
		bsdf.calc_albedo(p, throughput, mk2(0.0f, 0.0f), lod);
	}

	bool ok; float pdf = 0.0f; f3 value, direction_out; int medium_id = RT_INVALID;
	if (EVAL) {
		value = mk3(0.0f);
		direction_out = mk3(a[15], a[16], a[17]);
		ok = bsdf.eval(p, direction_out, a[18], value, pdf);
	} else {
		direction_out = mk3(0.0f);
		ok = bsdf.sample(p, throughput, medium_id, direction_out, pdf);
		value = throughput;
	}
	o[0] = ok ? 1.0f : 0.0f;
	o[1] = pdf;
	o[2] = value.x; o[3] = value.y; o[4] = value.z;
	o[5] = direction_out.x; o[6] = direction_out.y; o[7] = direction_out.z;
	o[8] = float(medium_id);
	o[9] = bsdf.allow_nee() ? 1.0f : 0.0f;
}

// rt_sample_lights: nee_pick_light on explicit random numbers, with the tables chosen as shade_material chooses them (use_lds: the
// workgroup of RT_SHADE_BLOCK threads copies them with light_tables_to_lds and passes the copy) or from global memory (nullptr).
// Record in: {u_mesh, u_triangle, u_1, u_2}; out: RT_LIGHT_SAMPLE_OUT floats {light-mesh entry, transform id (after the mesh_position
// remap), triangle index, 1 if the searches read LDS else 0 (int32 bits), point[3], geometric normal[3], emission[3], pad[3]}.
// The transform id and the triangle are sample_light's own; the entry is the first of its two searches made again on the same table.
__global__ void kernel_sample_lights(RtParams p, const float * probes, int count, int use_lds, float * out) {
	__shared__ LightTablesLDS light_lds;
	if (use_lds) light_tables_to_lds(p, light_lds);
	__syncthreads();
	const LightTablesLDS * const light_tables = use_lds ? &light_lds : nullptr;
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * a = probes + size_t(i) * 4;
	float * o = out + size_t(i) * RT_LIGHT_SAMPLE_OUT;
	const bool from_lds = light_tables != nullptr && light_tables_fit_lds(p);
	int entry = from_lds ? binary_search((LdsFloatTable)light_tables->mesh_cdf, 0, p.light_mesh_count - 1, a[0])
	                     : binary_search(p.light_mesh_cumulative_probability, 0, p.light_mesh_count - 1, a[0]);
	int transform_id;
	int triangle_id = sample_light(p, light_tables, a[0], a[1], transform_id);
	LightSample light = nee_pick_light(p, light_tables, mk2(a[0], a[1]), mk2(a[2], a[3]));
	o[0] = __int_as_float(entry); o[1] = __int_as_float(transform_id); o[2] = __int_as_float(triangle_id); o[3] = __int_as_float(from_lds ? 1 : 0);
	o[4] = light.point.x; o[5] = light.point.y; o[6] = light.point.z;
	o[7] = light.geometric_normal.x; o[8] = light.geometric_normal.y; o[9] = light.geometric_normal.z;
	o[10] = light.emission.x; o[11] = light.emission.y; o[12] = light.emission.z;
	o[13] = o[14] = o[15] = 0.0f;
}

// rt_sample_delta_lights: nee_pick_delta and delta_light_sample on explicit probes. Record in: {u, origin[3]}; out: RT_DELTA_SAMPLE_OUT floats
// {light index (int32 bits), to_light[3], max_distance, radiance term[3], P_k, ok, pad[2]}; a dropped sample reports zeros for direction, distance and term.
__global__ void kernel_sample_delta_lights(RtParams p, const float * probes, int count, float * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * a = probes + size_t(i) * 4;
	float * o = out + size_t(i) * RT_DELTA_SAMPLE_OUT;
	const int index = nee_pick_delta(p, a[0]);
	const RtDeltaLight light = p.delta_lights[index];
	DeltaSample sample;
	bool ok = delta_light_sample(light, mk3(a[1], a[2], a[3]), sample) && light.direction_pdf.w > 0.0f;
	if (!ok) { sample.to_light = mk3(0.0f); sample.max_distance = 0.0f; sample.radiance = mk3(0.0f); }
	o[0] = __int_as_float(index);
	o[1] = sample.to_light.x; o[2] = sample.to_light.y; o[3] = sample.to_light.z;
	o[4] = sample.max_distance;
	o[5] = sample.radiance.x; o[6] = sample.radiance.y; o[7] = sample.radiance.z;
	o[8] = light.direction_pdf.w;
	o[9] = ok ? 1.0f : 0.0f;
	o[10] = o[11] = 0.0f;
}

// rt_perturb_normals: normal_map_perturb on explicit hits, the surface set up as set_up_surface sets it up (RT_NORMAL_PROBE_IN floats per
// probe, layout in gpu_raytracer_amd.h; out: 4 floats {normal[3], fell back}). COMPRESSED is picked as for the material kernels.
template<bool COMPRESSED>
__global__ void kernel_perturb_normals(RtParams p, int texture_index, const float * probes, int count, float * out) {
	int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const float * a = probes + size_t(i) * RT_NORMAL_PROBE_IN;
	TriangleFull tri;
	tri.position_0 = mk3(a[0], a[1], a[2]); tri.position_edge_1 = mk3(a[3], a[4], a[5]); tri.position_edge_2 = mk3(a[6], a[7], a[8]);
	tri.normal_0 = mk3(a[9], a[10], a[11]); tri.normal_edge_1 = mk3(a[12], a[13], a[14]); tri.normal_edge_2 = mk3(a[15], a[16], a[17]);
	tri.tex_coord_0 = mk2(a[18], a[19]); tri.tex_coord_edge_1 = mk2(a[20], a[21]); tri.tex_coord_edge_2 = mk2(a[22], a[23]);
	const float u = a[24], v = a[25];
	const float4 world[3] = { make_float4(a[26], a[27], a[28], a[29]), make_float4(a[30], a[31], a[32], a[33]), make_float4(a[34], a[35], a[36], a[37]) };
	const f3 ray_direction = mk3(a[38], a[39], a[40]);
	const int filter = int(a[41]);

	f3 normal    = barycentric(u, v, tri.normal_0,    tri.normal_edge_1,    tri.normal_edge_2);
	f2 tex_coord = barycentric(u, v, tri.tex_coord_0, tri.tex_coord_edge_1, tri.tex_coord_edge_2);
	normal = normalize(m_direction(world, normal));
	float uv_det;
	f3 dpdu = m_direction(world, normal_map_dpdu(tri.position_edge_1, tri.position_edge_2, tri.tex_coord_edge_1, tri.tex_coord_edge_2, uv_det));
	f3 geometric_normal = cross(m_direction(world, tri.position_edge_1), m_direction(world, tri.position_edge_2));
	geometric_normal *= 1.0f / length(geometric_normal);
	bool entering_material = dot(ray_direction, geometric_normal) < 0.0f;

	f3 shading_normal = entering_material ? normal : -normal;
	bool mapped = normal_map_perturb<COMPRESSED>(p.textures[texture_index], filter, tex_coord, a[42], mk2(a[43], a[44]), mk2(a[45], a[46]), dpdu, uv_det,
	                                             normal, geometric_normal, entering_material, ray_direction, shading_normal);
	float * o = out + size_t(i) * 4;
	o[0] = shading_normal.x; o[1] = shading_normal.y; o[2] = shading_normal.z; o[3] = mapped ? 0.0f : 1.0f;
}

// ---- launchers ---------------------------------------------------------------------------------------------------

void rt_launch_sample_texture(const RtParams & p, int texture_index, int filter, const float * args, int count, float4 * out, hipStream_t stream) {
	hipLaunchKernelGGL(p.textures_compressed ? kernel_sample_texture<true> : kernel_sample_texture<false>, dim3((count + 255) / 256), dim3(256), 0, stream, p, texture_index, filter, args, count, out);
}
void rt_launch_sample_table(const float * table, int nx, int ny, int nz, int dims, const float * coords, int count, float * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_sample_table, dim3((count + 255) / 256), dim3(256), 0, stream, table, nx, ny, nz, dims, coords, count, out);
}
void rt_launch_sample_sky(const RtParams & p, const float * directions, int count, float * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_sample_sky, dim3((count + 255) / 256), dim3(256), 0, stream, p, directions, count, out);
}
void rt_launch_perturb_normals(const RtParams & p, int texture_index, const float * probes, int count, float * out, hipStream_t stream) {
	hipLaunchKernelGGL(p.textures_compressed ? kernel_perturb_normals<true> : kernel_perturb_normals<false>, dim3((count + 255) / 256), dim3(256), 0, stream, p, texture_index, probes, count, out);
}
// diffuse and plastic: the COMPRESSED instantiations the textureless material kernels launch (no texture is read either way)
template<bool EVAL>
static void launch_bsdf_probe(const RtParams & p, int material_type, const float * probes, int count, float * out, hipStream_t stream) {
	dim3 grid((count + 255) / 256), block(256);
	switch (material_type) {
		case RT_MATERIAL_DIFFUSE:    hipLaunchKernelGGL((kernel_bsdf_probe<BSDFDiffuse,    EVAL>), grid, block, 0, stream, p, probes, count, out); break;
		case RT_MATERIAL_PLASTIC:    hipLaunchKernelGGL((kernel_bsdf_probe<BSDFPlastic,    EVAL>), grid, block, 0, stream, p, probes, count, out); break;
		case RT_MATERIAL_DIELECTRIC: hipLaunchKernelGGL((kernel_bsdf_probe<BSDFDielectric, EVAL>), grid, block, 0, stream, p, probes, count, out); break;
		case RT_MATERIAL_CONDUCTOR:  hipLaunchKernelGGL((kernel_bsdf_probe<BSDFConductor,  EVAL>), grid, block, 0, stream, p, probes, count, out); break;
	}
}
void rt_launch_sample_lights(const RtParams & p, const float * probes, int count, bool use_lds, float * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_sample_lights, dim3((count + RT_SHADE_BLOCK - 1) / RT_SHADE_BLOCK), dim3(RT_SHADE_BLOCK), 0, stream, p, probes, count, use_lds ? 1 : 0, out);
}
void rt_launch_sample_delta_lights(const RtParams & p, const float * probes, int count, float * out, hipStream_t stream) {
	hipLaunchKernelGGL(kernel_sample_delta_lights, dim3((count + 255) / 256), dim3(256), 0, stream, p, probes, count, out);
}
void rt_launch_bsdf_probe(const RtParams & p, int material_type, bool eval,const float * probes, int count, float * out, hipStream_t stream) {
	if (eval) launch_bsdf_probe<true>(p, material_type, probes, count, out, stream);
	else      launch_bsdf_probe<false>(p, material_type, probes, count, out, stream);
}
