// rt_fog_grid.h -- the density grid of the fog volume: rho[z][y][x], nx x ny x nz float32 values >= 0 laid over the box of the fog volume in
// force, constant within a voxel; inside voxel v the coefficients are rho_v * sigma_a and rho_v * sigma_s. The homogeneous estimator of rt_fog.h holds
// unchanged with length replaced by DENSITY LENGTH D(t) = integral of rho ds: the same hashed pair, the same channel choice, the same weights (rho
// scales sigma_a and sigma_s alike and cancels from the scatter weight). This file is the voxel march that gives D and inverts it, shared by the
// ..._fog_grid instances of the sort kernels (kernels_sort.hip), the ..._grid attenuation kernels and the probe (kernels_fog.hip).
// tests/fog_density_reference.py restates D and its inversion in float64 by another method (sorted plane crossings, voxels from interval midpoints).
#pragma once
#include "rt_fog.h"

#define RT_FOG_BRICK 8   // voxels per brick edge: a brick table marks the bricks that hold no density, and a ray crosses such a brick in one step

struct FogGrid { const float * density; const unsigned char * bricks; int nx, ny, nz; f3 cell; };
RT_DEV FogGrid fog_grid(const RtParams & p, const FogVolume & fog) {
	FogGrid g;
	g.density = p.fog_density; g.bricks = p.fog_bricks;
	g.nx = p.fog_grid_dims[0]; g.ny = p.fog_grid_dims[1]; g.nz = p.fog_grid_dims[2];
	g.cell = mk3((fog.box_max.x - fog.box_min.x) / float(g.nx), (fog.box_max.y - fog.box_min.y) / float(g.ny), (fog.box_max.z - fog.box_min.z) / float(g.nz));
	return g;
}

// Plane i of an axis with n cells: lo + float(i) * cell, from the INDEX at every step (never by adding increments), and the outermost planes are the box
// faces themselves, exact -- so a 1 x 1 x 1 grid of 1.0 has the planes fog_clip clipped against and gives the homogeneous result to the bit.
// The distance to it is the division (plane - o) / d; a direction component of +0 or -0 never crosses a plane of its axis: infinity.
RT_DEV float fog_plane_distance(float o, float d, float lo, float hi, float cell, int n, int i) {
	if (d == 0.0f) return RT_INFINITY;
	float plane = i <= 0 ? lo : i >= n ? hi : lo + float(i) * cell;
	return (plane - o) / d;
}
// floor((o + t d - lo) / cell) clamped to [first, last] (a NaN gives first)
RT_DEV int fog_cell_index(float o, float d, float t, float lo, float cell, int first, int last) {
	float f = floorf((o + t * d - lo) / cell);
	return f >= float(last) ? last : f > float(first) ? int(f) : first;
}

// The march over a clipped segment (o, d, [t0, t1]) (fog_clip). Accumulates D += rho * seg voxel by voxel until the end t1, until an index leaves the
// grid, or until D would pass `target` (the homogeneous distance sample d*, RT_INFINITY for a shadow ray) inside a voxel of rho > 0: then the
// path scatters at t_scatter = min(t + (target - D) / rho, t_exit) and the function returns true. `density_length` is D(t1) when it returns false and
// D up to the vertex when it returns true.
// The scatter test is D + rho * seg > target, strictly, with the very sum that becomes the next D: the sums only grow, so "the march scattered" and
// fog_sample_distance's `distance < L` with L = D(t1) are the same statement, and with L = (t1 - t0) * 1 (one cell of 1.0) it is the homogeneous test.
// An empty brick (RT_FOG_BRICK^3 voxels without density, edge bricks partial) is crossed in one step against the brick's own planes, none of its voxels
// read; behind it the index on the crossed axis is the plane's (an integer), the other two are taken from the position, clamped to the brick's range.
// At most nx + ny + nz + 3 steps whatever the input (NaN included: every comparison that continues the loop is false for one).
// COUNT (the probe): steps[0] voxels read, steps[1] empty bricks crossed.
template<bool COUNT = false>
RT_DEV bool fog_grid_march(const FogVolume & fog, const FogGrid & grid, f3 o, f3 d, float t0, float t1, float target, float & density_length, float & t_scatter, int * steps = nullptr) {
	const int nx = grid.nx, ny = grid.ny, nz = grid.nz;
	const int nbx = (nx + RT_FOG_BRICK - 1) / RT_FOG_BRICK, nby = (ny + RT_FOG_BRICK - 1) / RT_FOG_BRICK;
	int ix = fog_cell_index(o.x, d.x, t0, fog.box_min.x, grid.cell.x, 0, nx - 1);
	int iy = fog_cell_index(o.y, d.y, t0, fog.box_min.y, grid.cell.y, 0, ny - 1);
	int iz = fog_cell_index(o.z, d.z, t0, fog.box_min.z, grid.cell.z, 0, nz - 1);
	float t = t0, D = 0.0f;
	t_scatter = RT_INFINITY;
	const int cap = nx + ny + nz + 3;
	for (int step = 0; step < cap; step++) {
		const int bx = ix / RT_FOG_BRICK, by = iy / RT_FOG_BRICK, bz = iz / RT_FOG_BRICK;
		const bool empty = grid.bricks[(bz * nby + by) * nbx + bx] == 0;
		// the planes through which the ray leaves this voxel or, in an empty brick, the whole brick
		const int px = d.x > 0.0f ? (empty ? min((bx + 1) * RT_FOG_BRICK, nx) : ix + 1) : (empty ? bx * RT_FOG_BRICK : ix);
		const int py = d.y > 0.0f ? (empty ? min((by + 1) * RT_FOG_BRICK, ny) : iy + 1) : (empty ? by * RT_FOG_BRICK : iy);
		const int pz = d.z > 0.0f ? (empty ? min((bz + 1) * RT_FOG_BRICK, nz) : iz + 1) : (empty ? bz * RT_FOG_BRICK : iz);
		const float tx = fog_plane_distance(o.x, d.x, fog.box_min.x, fog.box_max.x, grid.cell.x, nx, px);
		const float ty = fog_plane_distance(o.y, d.y, fog.box_min.y, fog.box_max.y, grid.cell.y, ny, py);
		const float tz = fog_plane_distance(o.z, d.z, fog.box_min.z, fog.box_max.z, grid.cell.z, nz, pz);
		const float t_exit = fminf(fminf(tx, ty), fminf(tz, t1));
		const float rho = empty ? 0.0f : grid.density[(iz * ny + iy) * nx + ix];
		if (COUNT) steps[empty ? 1 : 0]++;
		const float seg = fmaxf(t_exit - t, 0.0f);
		const float D_next = rho > 0.0f ? D + rho * seg : D;   // (a voxel without density adds exactly 0, over an infinite segment too)
		if (D_next > target) {
			t_scatter = fminf(t + (target - D) / rho, t_exit);
			density_length = D + rho * fmaxf(t_scatter - t, 0.0f);
			return true;
		}
		D = D_next; t = t_exit;
		if (!(t_exit < t1)) break;
		if (tx == t_exit) {
			ix = empty ? (d.x > 0.0f ? px : px - 1) : (d.x > 0.0f ? ix + 1 : ix - 1);
			if (empty) {
				iy = fog_cell_index(o.y, d.y, t, fog.box_min.y, grid.cell.y, by * RT_FOG_BRICK, min(by * RT_FOG_BRICK + RT_FOG_BRICK - 1, ny - 1));
				iz = fog_cell_index(o.z, d.z, t, fog.box_min.z, grid.cell.z, bz * RT_FOG_BRICK, min(bz * RT_FOG_BRICK + RT_FOG_BRICK - 1, nz - 1));
			}
			if (ix < 0 || ix >= nx) break;
		} else if (ty == t_exit) {
			iy = empty ? (d.y > 0.0f ? py : py - 1) : (d.y > 0.0f ? iy + 1 : iy - 1);
			if (empty) {
				ix = fog_cell_index(o.x, d.x, t, fog.box_min.x, grid.cell.x, bx * RT_FOG_BRICK, min(bx * RT_FOG_BRICK + RT_FOG_BRICK - 1, nx - 1));
				iz = fog_cell_index(o.z, d.z, t, fog.box_min.z, grid.cell.z, bz * RT_FOG_BRICK, min(bz * RT_FOG_BRICK + RT_FOG_BRICK - 1, nz - 1));
			}
			if (iy < 0 || iy >= ny) break;
		} else {
			iz = empty ? (d.z > 0.0f ? pz : pz - 1) : (d.z > 0.0f ? iz + 1 : iz - 1);
			if (empty) {
				ix = fog_cell_index(o.x, d.x, t, fog.box_min.x, grid.cell.x, bx * RT_FOG_BRICK, min(bx * RT_FOG_BRICK + RT_FOG_BRICK - 1, nx - 1));
				iy = fog_cell_index(o.y, d.y, t, fog.box_min.y, grid.cell.y, by * RT_FOG_BRICK, min(by * RT_FOG_BRICK + RT_FOG_BRICK - 1, ny - 1));
			}
			if (iz < 0 || iz >= nz) break;
		}
	}
	density_length = D;
	return false;
}

// The homogeneous distance sample d* of fog_sample_distance -- the channel by throughput, the exponential distance in it -- without its weights:
// what the march inverts D against. RT_INFINITY without scattering (absorption only: the march gives the whole density length).
RT_DEV float fog_sample_target(const FogVolume & fog, f2 rand, f3 throughput) {
	if (!(fog.sigma_s.x + fog.sigma_s.y + fog.sigma_s.z > 0.0f)) return RT_INFINITY;
	f3 sigma_t = fog.sigma_a + fog.sigma_s;
	float throughput_sum = throughput.x + throughput.y + throughput.z;
	float sigma_t_used;
	if      (rand.x * throughput_sum < throughput.x)                sigma_t_used = sigma_t.x;
	else if (rand.x * throughput_sum < throughput.x + throughput.y) sigma_t_used = sigma_t.y;
	else                                                            sigma_t_used = sigma_t.z;
	return sample_exp(sigma_t_used, rand.y);
}

// The segment step over the grid: whether the path scatters, at t_scatter along the ray; either way `throughput` takes exactly what fog_sample_distance
// gives over the density length (`distance` is d* as there: RT_INFINITY when the path does not scatter). A segment without density leaves the path untouched.
template<bool COUNT = false>
RT_DEV bool fog_grid_sample_distance(const FogVolume & fog, const FogGrid & grid, f2 rand, f3 o, f3 d, float t0, float t1, f3 & throughput, float & distance, float & t_scatter, float & density_length, int * steps = nullptr) {
	const float target = fog_sample_target(fog, rand, throughput);
	const bool scattered = fog_grid_march<COUNT>(fog, grid, o, d, t0, t1, target, density_length, t_scatter, steps);
	distance = RT_INFINITY;
	if (!scattered && !(density_length > 0.0f)) return false;
	// (a march that scattered passed d* for good: any length beyond d* gives the weights of the scatter event)
	fog_sample_distance(fog, rand, scattered ? RT_INFINITY : density_length, throughput, distance);
	return scattered;
}

// exp(-sigma_t * D) of a ray (o, d, [0, max_distance]) over its clipped interval; false (nothing to multiply) where it does not cross the box or meets no density
RT_DEV bool fog_grid_transmittance(const FogVolume & fog, const FogGrid & grid, f3 o, f3 d, float max_distance, f3 & transmittance) {
	float t0, t1, D, t_scatter;
	if (!fog_clip(fog, o, d, max_distance, t0, t1)) return false;
	fog_grid_march(fog, grid, o, d, t0, t1, RT_INFINITY, D, t_scatter);
	if (!(D > 0.0f)) return false;
	transmittance = beer_lambert(fog.sigma_a + fog.sigma_s, D);
	return true;
}
