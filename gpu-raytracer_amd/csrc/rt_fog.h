// rt_fog.h -- the fog volume: one homogeneous medium inside an axis-aligned box. The device functions of a path segment -- the clip
// against the box, the hashed pair of random numbers, the distance sample with its weights -- and of the phase function, shared by the ..._fog
// instances of the sort kernels (kernels_sort.hip), the attenuation pass of the shadow queue and the probe of the segment step (kernels_fog.hip).
// tests/fog_reference.py restates every function of this file in float64 / integers.
#pragma once
#include "rt_shading.h"

#define RT_ONE_OVER_FOUR_PI 0.07957747154594767f

struct FogVolume { f3 box_min, box_max, sigma_a, sigma_s; float g; };
RT_DEV FogVolume fog_volume(const RtParams & p) {
	FogVolume v;
	v.box_min = mk3(p.fog_box_min[0], p.fog_box_min[1], p.fog_box_min[2]); v.box_max = mk3(p.fog_box_max[0], p.fog_box_max[1], p.fog_box_max[2]);
	v.sigma_a = mk3(p.fog_sigma_a[0], p.fog_sigma_a[1], p.fog_sigma_a[2]); v.sigma_s = mk3(p.fog_sigma_s[0], p.fog_sigma_s[1], p.fog_sigma_s[2]);
	v.g = p.fog_g;
	return v;
}

// One slab of the clip. A direction component of +0 or -0: the ray runs parallel to the slab and is inside it or outside it by its origin alone (the faces
// belong to the box); no quotient is formed, so no NaN. Otherwise the two face distances are DIVISIONS (b - o) / d, not products with 1 / d: the
// reciprocal of a subnormal component is infinite and 0 * inf would be a NaN for an origin on a face. False: the ray never is between the faces.
RT_DEV bool fog_slab(float o, float d, float lo, float hi, float & t_near, float & t_far) {
	if (d == 0.0f) return o >= lo && o <= hi;
	float ta = (lo - o) / d, tb = (hi - o) / d;
	t_near = fmaxf(t_near, fminf(ta, tb));
	t_far  = fminf(t_far,  fmaxf(ta, tb));
	return true;
}
// The part of the segment (o, d, [0, t_end]) inside the box: [t0, t1]. False -- the segment is left as it is -- when that is empty or of length 0.
// An origin on a face is inside (t0 = 0) when the ray enters, and the interval is empty when it leaves.
RT_DEV bool fog_clip(const FogVolume & fog, f3 o, f3 d, float t_end, float & t0, float & t1) {
	t0 = 0.0f; t1 = t_end;
	bool inside = fog_slab(o.x, d.x, fog.box_min.x, fog.box_max.x, t0, t1);
	inside = fog_slab(o.y, d.y, fog.box_min.y, fog.box_max.y, t0, t1) && inside;
	inside = fog_slab(o.z, d.z, fog.box_min.z, fog.box_max.z, t0, t1) && inside;
	return inside && t1 > t0;
}

// The two numbers of a segment's distance sample (channel choice, distance): a hashed pair in the form random_sample takes beyond the PMJ tables,
// under a key of its own: bit 31 set over pixel * RT_MAX_BOUNCES + bounce. random_sample's keys, (pixel * 7 + dimension) * RT_MAX_BOUNCES + bounce, stay
// below 2^31 for frames of up to 2 396 745 pixels, so no draw of such a frame shares the key. Not DIM_BSDF_0: the surface at the end
// of an unscattered segment draws that pair, and "did not scatter" is a condition on the distance number.
RT_DEV unsigned fog_random_key(unsigned pixel, unsigned bounce) { return 0x80000000u | (pixel * unsigned(RT_MAX_BOUNCES) + bounce); }
RT_DEV f2 fog_random_pair(const RandomPath & path, unsigned bounce) {
	unsigned hash = pcg_hash(fog_random_key(path.pixel, bounce));
	const float one_over_max_unsigned = __uint_as_float(0x2f7fffffu);
	float x = float(hash_with(path.sample_index,               hash)) * one_over_max_unsigned;
	float y = float(hash_with(path.sample_index + 0xdeadbeefu, hash)) * one_over_max_unsigned;
	return mk2(x, y);
}

// The distance sample over a clipped length L, the spectral scheme of sort_rays' inside_medium branch: the channel by throughput, an exponential
// distance in it, the channel-averaged pdf. Returns whether the path scatters, at `distance` < L; either way `throughput` takes its weight.
// Absorption only (sigma_s = 0): no sample, the plain transmittance.
RT_DEV bool fog_sample_distance(const FogVolume & fog, f2 rand, float L, f3 & throughput, float & distance) {
	distance = RT_INFINITY;
	if (!(fog.sigma_s.x + fog.sigma_s.y + fog.sigma_s.z > 0.0f)) { throughput *= beer_lambert(fog.sigma_a, L); return false; }
	f3 sigma_t = fog.sigma_a + fog.sigma_s;
	float throughput_sum = throughput.x + throughput.y + throughput.z;
	f3 wavelength_pdf = throughput / throughput_sum;
	float sigma_t_used;
	if      (rand.x * throughput_sum < throughput.x)                sigma_t_used = sigma_t.x;
	else if (rand.x * throughput_sum < throughput.x + throughput.y) sigma_t_used = sigma_t.y;
	else                                                            sigma_t_used = sigma_t.z;
	distance = sample_exp(sigma_t_used, rand.y);
	f3 transmittance = beer_lambert(sigma_t, fminf(distance, L));
	if (distance < L) {
		f3 pdf = wavelength_pdf * sigma_t * transmittance;
		throughput *= fog.sigma_s * transmittance / (pdf.x + pdf.y + pdf.z);
		return true;
	}
	f3 pdf = wavelength_pdf * transmittance;
	throughput *= transmittance / (pdf.x + pdf.y + pdf.z);
	distance = RT_INFINITY;
	return false;
}

// exp(-sigma_t * clipped length) of a ray (o, d, [0, max_distance]); 1 where it does not cross the box
RT_DEV f3 fog_transmittance(const FogVolume & fog, f3 o, f3 d, float max_distance) {
	float t0, t1;
	if (!fog_clip(fog, o, d, max_distance, t0, t1)) return mk3(1.0f);
	return beer_lambert(fog.sigma_a + fog.sigma_s, t1 - t0);
}

// Henyey-Greenstein, value = pdf, in the convention of sample_henyey_greenstein(omega, ...): cos_theta is measured against omega, the direction BACK
// along the arriving ray, so g > 0 favours cos_theta = -1 (straight on). Below |g| = 1e-3 the sampler is isotropic and so is this: exactly 1 / 4 pi.
RT_DEV float henyey_greenstein(float cos_theta, float g) {
	if (fabsf(g) < 1e-3f) return RT_ONE_OVER_FOUR_PI;
	float denominator = 1.0f + g * g + 2.0f * g * cos_theta;
	return RT_ONE_OVER_FOUR_PI * (1.0f - g * g) / (denominator * sqrtf(denominator));
}
