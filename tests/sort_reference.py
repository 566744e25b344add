"""numpy float64 restatement of the sort launch (kernels_sort.hip: sort_rays; the reference's kernel_sort, Pathtracer.cu:199-463 as
oracle_pathtrace.cpp cites it) on the records of rt_sort_rays, for test_sort.py (oracle against this) and test_gpu_sort.py (device
against this). Vectorised over the entries of one launch; float32 inputs are taken exactly, every operation is float64.

The random numbers are oracle_random's (pinned bit-exact elsewhere); the sky pdf is sky_sampling_reference.Tables'. What the _sky
instances (sort_rays<*, true>) add is restated from the device code: a miss flagged ALLOW_NEE is dropped without MIS and weighed by
power_heuristic(last_pdf, share * sky_pdf) with it; an emitter's light_pdf carries (1 - share); share 1 counts every emitter hit.

`evaluate` also says how far every comparison an entry takes is from its threshold (the `near_*` masks, against the margins of
sort_checks.MARGINS), and can be asked to take a comparison the other way (`flip`) so that the outcomes float64 allows for an entry
within the margin can be listed (`allowed_outcomes`)."""
import numpy as np

import sky_sampling_reference as sky_ref

DIM_RUSSIAN_ROULETTE, DIM_BSDF_0, DIM_BSDF_1 = 2, 5, 6            # Sampling.h:30-42
FLAG_ALLOW_NEE, FLAG_INSIDE_MEDIUM = 1 << 31, 1 << 30            # Pathtracer.cu:27-30
LIGHT, DIFFUSE, PLASTIC, DIELECTRIC, CONDUCTOR = range(5)
SCATTERED, TERMINATED = 4, 5                                     # outcomes 0..3: the material queues
OUTCOME_NAMES = ("diffuse", "plastic", "dielectric", "conductor", "scattered", "terminated")
TRACE_WORDS, MATERIAL_WORDS = 20, 16
INVALID = -1
RADIANCE, DIRECT, INDIRECT, ALBEDO = range(4)                    # the four frames of rt_sort_rays, in its order
FLT_MAX, FLT_MIN = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)
OUTCOME_FLIPS = ("scatter", "roulette", "wavelength0", "wavelength1")


class Entries:
    """A trace queue, one numpy array per field (N entries)."""
    FIELDS = (("origin", np.float32, 3), ("direction", np.float32, 3), ("mesh", np.int32, 0), ("triangle", np.int32, 0), ("t", np.float32, 0),
              ("u16", np.uint32, 0), ("v16", np.uint32, 0), ("pixel", np.uint32, 0), ("allow_nee", bool, 0), ("inside", bool, 0),
              ("throughput", np.float32, 3), ("last_pdf", np.float32, 0), ("medium", np.int32, 0), ("cone_angle", np.float32, 0), ("cone_width", np.float32, 0))

    def __init__(self, n):
        self.n = n
        for name, dtype, width in self.FIELDS:
            setattr(self, name, np.zeros((n, width) if width else n, dtype))
        self.medium[:] = INVALID

    def take(self, index):
        out = Entries(0)
        for name, _, _ in self.FIELDS:
            setattr(out, name, getattr(self, name)[index].copy())
        out.n = out.pixel.size
        return out

    @staticmethod
    def concatenate(parts):
        out = Entries(0)
        for name, _, _ in Entries.FIELDS:
            setattr(out, name, np.concatenate([getattr(p, name) for p in parts]))
        out.n = out.pixel.size
        return out

    def pack(self, pixel=None):
        """(N, 20) uint32 records of rt_sort_rays / oracle_sort; `pixel` replaces the virtual pixels (the oracle takes real ones)."""
        r = np.zeros((self.n, TRACE_WORDS), np.uint32)
        r[:, 0:3] = self.origin.view(np.uint32); r[:, 3:6] = self.direction.view(np.uint32)
        r[:, 6] = self.mesh.view(np.uint32); r[:, 7] = self.triangle.view(np.uint32); r[:, 8] = self.t.view(np.uint32)
        r[:, 9] = (self.u16 & 0xffff) | (self.v16 << 16)
        r[:, 10] = (self.pixel if pixel is None else pixel.astype(np.uint32)) | (self.allow_nee.astype(np.uint32) << 31) | (self.inside.astype(np.uint32) << 30)
        r[:, 11:14] = self.throughput.view(np.uint32); r[:, 14] = self.last_pdf.view(np.uint32); r[:, 15] = self.medium.view(np.uint32)
        r[:, 16] = self.cone_angle.view(np.uint32); r[:, 17] = self.cone_width.view(np.uint32)
        return r


class Launch:
    """One sort launch: the queue, how its entries' bounce and sample are found, and what the frames hold before it.
    Per-bounce form: bounce, sample_index. Merged form: iteration, slot_table (S, 4) int32 {sample_index, birth_iteration, submission,
    index_in_submission}, submission_birth int32[128]. aov (4, P, 4) float32, gnd (P, 4) float32, gid (P, 2) int32, gsp (P, 2) float32
    with P = frame_slots * frame_pixels."""

    def __init__(self, name, entries, frame_pixels, frame_slots, bounce=None, sample_index=0, iteration=None, slot_table=None, submission_birth=None,
                 aov=None, seed=0):
        self.name, self.entries, self.frame_pixels, self.frame_slots = name, entries, int(frame_pixels), int(frame_slots)
        self.bounce, self.sample_index, self.iteration = bounce, sample_index, iteration
        self.slot_table = None if slot_table is None else np.ascontiguousarray(slot_table, np.int32).reshape(-1, 4)
        self.submission_birth = None if submission_birth is None else np.ascontiguousarray(submission_birth, np.int32)
        self.merged = iteration is not None
        p = self.frame_pixels * self.frame_slots
        rng = np.random.default_rng(1000 + seed)
        # frames that hold something everywhere: an update of the wrong pixel, or a set where an add is meant, shows
        self.aov = rng.uniform(0.0, 1.0, (4, p, 4)).astype(np.float32) if aov is None else np.ascontiguousarray(aov, np.float32).reshape(4, p, 4)
        self.gnd = rng.uniform(-1.0, 1.0, (p, 4)).astype(np.float32)
        self.gid = rng.integers(100, 200, (p, 2)).astype(np.int32)
        self.gsp = rng.uniform(-1.0, 1.0, (p, 2)).astype(np.float32)

    def paths(self):
        """Per entry: slot, real pixel, bounce, sample index (the RNG's), submission, first sample of its submission."""
        e = self.entries
        slot = (e.pixel // self.frame_pixels).astype(np.int64)
        real = (e.pixel % self.frame_pixels).astype(np.uint32)
        if self.merged:
            row = self.slot_table[slot]
            return slot, real, self.iteration - row[:, 1].astype(np.int64), row[:, 0].astype(np.int64), row[:, 2].astype(np.int64), row[:, 3] == 0
        zero = np.zeros(e.n, np.int64)
        return slot, real, zero + self.bounce, self.sample_index + slot, zero, np.ones(e.n, bool)


class Tables:
    """What the sort launch reads of a scene, from an oracle SceneView (whose arrays and settings the test may have replaced)."""

    def __init__(self, view, sky_share=0.0, pixel_query=-1):
        self.view = view
        self.pixel_query = int(pixel_query)   # rt_set_pixel_query's pixel (x + y * pitch), -1: none
        s = view.scene
        k = view.keep
        self.material_ids = np.asarray(k["mesh_material_ids"], np.int32)
        self.material_types = np.asarray(k["material_types"], np.uint8)
        self.materials = np.asarray(k["materials"], np.float32).reshape(-1, 8)
        self.triangles = np.asarray(k["triangles"], np.float32).reshape(-1, 24)
        self.transforms = np.asarray(k["mesh_transforms"], np.float32).reshape(-1, 3, 4)
        self.transforms_prev = np.asarray(k["mesh_transforms_prev"], np.float32).reshape(-1, 3, 4)
        self.media = np.asarray(k["media"], np.float32).reshape(-1, 8)
        self.sky = np.asarray(k["sky"], np.float32).reshape(s.sky_height, s.sky_width, 4)
        self.sky_scale = float(np.float32(s.sky_scale))
        self.lights_total_weight = float(np.float32(s.lights_total_weight))
        self.pixel_spread_angle = float(np.float32(s.camera.pixel_spread_angle))
        self.view_projection = np.array(list(s.view_projection), np.float32).reshape(4, 4)
        self.view_projection_prev = np.array(list(s.view_projection_prev), np.float32).reshape(4, 4)
        self.pitch, self.frame_pixels = s.screen_pitch, s.screen_pitch * s.screen_height
        self.config = {f: getattr(s.config, f) for f in ("num_bounces", "enable_mipmapping", "enable_next_event_estimation", "enable_multiple_importance_sampling",
                                                         "enable_russian_roulette", "enable_svgf", "aov_mask")}
        svgf = self.config["enable_svgf"] != 0
        mask = self.config["aov_mask"] | 1 | (0b1110 if svgf else 0)   # rt_set_config: RADIANCE always, the other three with SVGF
        self.aov_enabled = tuple(bool((mask >> a) & 1) for a in range(4))
        self.sky_share = float(np.float32(sky_share))
        self.sky_tables = sky_ref.Tables(self.sky) if self.sky_share > 0 else None

    def random(self, dimension, real, bounce, sample):
        out = np.zeros((real.size, 2), np.float32)
        key = bounce.astype(np.int64) * (1 << 32) + sample.astype(np.int64)
        for k in np.unique(key):
            m = key == k
            out[m] = self.view.random(dimension, real[m], int(k >> 32), int(k & 0xffffffff))
        return out


def _normalize(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _henyey_greenstein(omega, g, u1, u2):
    """sample_henyey_greenstein (Sampling.h / rt_shading.h), float64."""
    with np.errstate(all="ignore"):
        iso = np.abs(g) < np.float64(np.float32(1e-3))
        gg = np.where(iso, 1.0, g)
        cos_t = np.where(iso, 1.0 - 2.0 * u1, -(1.0 + gg * gg - ((1.0 - gg * gg) / (1.0 + gg - 2.0 * gg * u1)) ** 2) / (2.0 * gg))
        sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
        phi = 2.0 * np.pi * u2
        local = np.stack([sin_t * np.sin(phi), sin_t * np.cos(phi), cos_t], axis=1)   # sincos_pair returns (sin, cos): x = sin, y = cos
        sign = np.copysign(1.0, omega[:, 2])
        a = -1.0 / (sign + omega[:, 2])
        b = omega[:, 0] * omega[:, 1] * a
        tangent = np.stack([1.0 + sign * omega[:, 0] * omega[:, 0] * a, sign * b, -sign * omega[:, 0]], axis=1)
        binormal = np.stack([b, sign + omega[:, 1] * omega[:, 1] * a, -omega[:, 1]], axis=1)
        return tangent * local[:, 0:1] + binormal * local[:, 1:2] + omega * local[:, 2:3], sin_t


def _oct_encode(n):
    with np.errstate(all="ignore"):
        n = n / np.abs(n).sum(axis=1)[:, None]
        x, y = n[:, 0].copy(), n[:, 1].copy()
        low = n[:, 2] < 0
        fx = (1.0 - np.abs(y)) * np.where(x >= 0, 1.0, -1.0)
        x = np.where(low, fx, x)
        fy = (1.0 - np.abs(x)) * np.where(y >= 0, 1.0, -1.0)   # (the reference folds y with the x it has just folded)
        y = np.where(low, fy, y)
        return 0.5 + 0.5 * x, 0.5 + 0.5 * y


class Result:
    pass


def evaluate(tables, launch, margins, flip=frozenset()):
    """The launch in float64. Returns a Result with, per entry: outcome; robust; throughput_out, origin_out, direction_out, cone_angle_out,
    cone_width_out (float64; what a material or continuation entry stores); finite (no NaN / infinity met); the near_* masks; and the
    decision quantities of oracle_sort's internals (distance, wavelength_x, survival, light_pdf, weight, sky_u, sky_v, cos_light;
    NaN where the entry computes none). Per launch: aov (4, P, 4) float64, the expected frames; touched (4, P) bool; gnd (P, 4) float64,
    gid (P, 2), gsp (P, 2) float64 and gbuffer_touched (P,); pixel_query (2,) or None when nothing answers."""
    e, cfg, n = launch.entries, tables.config, launch.entries.n
    slot, real, bounce, sample, submission, first = launch.paths()
    f64 = np.float64
    nan = np.full(n, np.nan)
    r = Result()
    r.bounce, r.submission, r.slot = bounce, submission, slot
    with np.errstate(all="ignore"):
        d = e.direction.astype(f64); t = e.t.astype(f64)
        tp = np.where((bounce == 0)[:, None], 1.0, e.throughput.astype(f64))
        outcome = np.full(n, -1)
        mip = cfg["enable_mipmapping"] != 0
        cone_angle = np.where((bounce > 0) & mip, e.cone_angle.astype(f64), 0.0)
        cone_width = np.where((bounce > 0) & mip, e.cone_width.astype(f64), 0.0)
        albedo = launch.aov[ALBEDO][e.pixel][:, :3].astype(f64)
        r_rr = tables.random(DIM_RUSSIAN_ROULETTE, real, bounce, sample)[:, 0].astype(f64)
        r.survival = nan.copy(); r.near_roulette = np.zeros(n, bool)

        def roulette(active, tp):
            """russian_roulette for the entries of `active`: (terminated, throughput afterwards)."""
            last = bounce == cfg["num_bounces"] - 1
            use = active & ~last & (cfg["enable_russian_roulette"] != 0) & (bounce > 0)
            tt = tp * albedo if cfg["enable_svgf"] else tp
            p = np.fmin(np.fmax(np.fmax.reduce(tt, axis=1), 0.0), 1.0)   # saturate(fmaxf(fmaxf(x, y), z)) = fminf(fmaxf(., 0), 1): a NaN maximum becomes 0
            r.survival = np.where(use, p, r.survival)
            r.near_roulette |= use & ~(np.abs(r_rr - p) > margins["survival"] * p)
            die = r_rr > p
            if "roulette" in flip:
                die = ~die
            return active & (last | (use & die)), np.where((use & ~die)[:, None], tp / p[:, None], tp)

        # ---- participating medium
        inside = e.inside
        med = tables.media[np.where(inside, e.medium, 0)]
        sigma_a, g, sigma_s = med[:, 0:3].astype(f64), med[:, 3].astype(f64), med[:, 4:7].astype(f64)
        can = inside & ((med[:, 4] + med[:, 5] + med[:, 6]) > 0)
        absorb = inside & ~can
        tp = np.where(absorb[:, None], tp * np.exp(-sigma_a * t[:, None]), tp)
        rs = tables.random(DIM_BSDF_0, real, bounce, sample).astype(f64)
        rp = tables.random(DIM_BSDF_1, real, bounce, sample).astype(f64)
        sigma_t = sigma_a + sigma_s
        tsum = tp.sum(axis=1)
        wpdf = tp / tsum[:, None]
        x = rs[:, 0] * tsum
        c0, c1 = x < tp[:, 0], x < tp[:, 0] + tp[:, 1]
        r.near_wavelength0 = can & ~(np.abs(x - tp[:, 0]) > margins["wavelength"] * tsum)
        r.near_wavelength1 = can & ~c0 & ~(np.abs(x - (tp[:, 0] + tp[:, 1])) > margins["wavelength"] * tsum)
        if "wavelength0" in flip:
            c0 = ~c0
        if "wavelength1" in flip:
            c1 = ~c1
        used = np.where(c0, sigma_t[:, 0], np.where(c1, sigma_t[:, 1], sigma_t[:, 2]))
        dist = -np.log(rs[:, 1]) / used
        trans = np.exp(-sigma_t * np.minimum(dist, t)[:, None])
        scatter = dist < t
        r.near_scatter = can & ~(np.abs(dist - t) > margins["distance"] * np.maximum(dist, t)) & ~(np.isinf(t) & np.isfinite(dist))   # (a miss: every finite distance scatters)
        if "scatter" in flip:
            scatter = ~scatter
        scatter &= can
        pdf_s = (wpdf * sigma_t * trans).sum(axis=1)
        pdf_n = (wpdf * trans).sum(axis=1)
        tp = np.where(scatter[:, None], tp * sigma_s * trans / pdf_s[:, None], np.where(can[:, None], tp * trans / pdf_n[:, None], tp))
        r.distance = np.where(can, dist, nan); r.wavelength_x = np.where(can, x, nan); r.throughput_sum = np.where(can, tsum, nan)
        died, tp_after = roulette(scatter, tp)
        tp = np.where(scatter[:, None], tp_after, tp)
        outcome[scatter & died] = TERMINATED
        outcome[scatter & ~died] = SCATTERED
        r.direction_out, r.sin_theta = _henyey_greenstein(-d, g, rp[:, 0], rp[:, 1])
        r.origin_out = e.origin.astype(f64) + dist[:, None] * d
        first_cone = scatter & (bounce == 0) & mip
        cone_angle = np.where(first_cone, tables.pixel_spread_angle, cone_angle)
        cone_width = np.where(first_cone, tables.pixel_spread_angle * dist, cone_width)
        r.cone_angle_out, r.cone_width_out = cone_angle, cone_width

        # ---- frames
        aov = launch.aov.astype(f64)
        touched = np.zeros((4, aov.shape[1]), bool)
        enabled = tables.aov_enabled

        def aov_set(which, mask, value):
            if enabled[which]:
                aov[which, e.pixel[mask], :3] = value[mask] if np.ndim(value) == 2 else value
                touched[which, e.pixel[mask]] = True

        def aov_add(which, mask, value):
            if enabled[which]:
                aov[which, e.pixel[mask], :3] += value[mask]
                touched[which, e.pixel[mask]] = True

        def add_radiance(mask, illumination, bounce0_value):
            b0, b1, b2 = mask & (bounce == 0), mask & (bounce == 1), mask & (bounce > 1)
            aov_set(ALBEDO, b0, 1.0); aov_set(RADIANCE, b0, bounce0_value); aov_set(DIRECT, b0, bounce0_value)
            aov_add(RADIANCE, b1, illumination); aov_add(DIRECT, b1, illumination)
            aov_add(RADIANCE, b2, illumination); aov_add(INDIRECT, b2, illumination)

        # ---- miss: the sky
        live = outcome < 0
        miss = live & (e.triangle == INVALID)
        sky = sky_ref.sample_sky(tables.sky, tables.sky_scale, d)
        illumination = tp * sky
        r.sky = np.where(miss[:, None], sky, np.nan)
        r.aov_scale = np.where(miss, tp.max(axis=1) * np.abs(tables.sky[..., :3]).max() * abs(tables.sky_scale), 0.0)   # the most the lookup's taps can differ by, times the throughput
        r.weight = nan.copy(); r.sky_u = nan.copy(); r.sky_v = nan.copy(); r.near_cell = np.zeros(n, bool)
        weighed = miss & e.allow_nee & (tables.sky_share > 0)
        dropped = weighed & (cfg["enable_multiple_importance_sampling"] == 0)
        weighed &= ~dropped
        if tables.sky_share > 0:
            u = np.arctan2(-d[:, 2], d[:, 0]) / (2.0 * np.pi) + 0.5
            v = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
            h, w = tables.sky.shape[:2]
            uw, vh = u * w, v * h
            inner_u = (uw > 0.5) & (uw < w - 0.5); inner_v = (vh > 0.5) & (vh < h - 0.5)   # beyond the last border the cell is clamped: no decision
            r.near_cell = weighed & ((inner_u & (np.abs(uw - np.round(uw)) <= margins["sky_uv"] * w)) | (inner_v & (np.abs(vh - np.round(vh)) <= margins["sky_uv"] * h)))
            sky_pdf = tables.sky_share * tables.sky_tables.pdf_of(d)
            b2 = e.last_pdf.astype(f64) ** 2
            weight = b2 / (b2 + sky_pdf * sky_pdf)
            illumination = np.where(weighed[:, None], illumination * weight[:, None], illumination)
            r.weight = np.where(weighed, weight, r.weight); r.sky_u = np.where(weighed, u, nan); r.sky_v = np.where(weighed, v, nan)
        add_radiance(miss & ~dropped, illumination, illumination)
        outcome[miss] = TERMINATED

        # ---- pixel query (Pathtracer.cu:345-348)
        live = outcome < 0
        asked = live & (bounce == 0) & first & ((real if launch.merged else e.pixel).astype(np.int64) == tables.pixel_query)
        r.pixel_query = (int(e.mesh[asked][-1]), int(e.triangle[asked][-1])) if asked.any() else None

        # ---- emitters
        mesh = np.where(live, e.mesh, 0); triangle = np.where(live, e.triangle, 0)
        material = tables.material_ids[mesh]
        mtype = tables.material_types[material].astype(np.int64)
        light = live & (mtype == LIGHT)
        tri = tables.triangles[triangle].astype(f64)
        p0, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
        bu = (e.u16.astype(np.float32) / np.float32(65535.0)).astype(f64); bv = (e.v16.astype(np.float32) / np.float32(65535.0)).astype(f64)
        local = p0 + bu[:, None] * e1 + bv[:, None] * e2
        world = tables.transforms[mesh].astype(f64)
        point = np.einsum("nij,nj->ni", world[:, :, :3], local) + world[:, :, 3]
        normal = _normalize(np.einsum("nij,nj->ni", world[:, :, :3], np.cross(e1, e2)))
        gb = light & (bounce == 0) & (cfg["enable_svgf"] != 0)
        r.gnd, r.gid, r.gsp = launch.gnd.astype(f64), launch.gid.copy(), launch.gsp.astype(f64)
        r.gbuffer_touched = np.zeros(r.gnd.shape[0], bool)
        if gb.any():
            prev = tables.transforms_prev[mesh].astype(f64)
            point_prev = np.einsum("nij,nj->ni", prev[:, :, :3], local) + prev[:, :, 3]
            one = np.ones((n, 1))
            u_curr = np.concatenate([point, one], axis=1) @ tables.view_projection.astype(f64).T
            u_prev = np.concatenate([point_prev, one], axis=1) @ tables.view_projection_prev.astype(f64).T
            ox, oy = _oct_encode(normal)
            px = e.pixel[gb]
            r.gnd[px] = np.stack([ox, oy, u_curr[:, 2], u_prev[:, 2]], axis=1)[gb]
            r.gid[px] = np.stack([e.mesh, e.triangle], axis=1)[gb]
            r.gsp[px] = (u_prev[:, :2] / u_prev[:, 3:4])[gb]
            r.gbuffer_touched[px] = True
        emission = tables.materials[material][:, :3].astype(f64)
        count_light = light & (~e.allow_nee if cfg["enable_next_event_estimation"] else True)
        if tables.sky_share >= 1.0:
            count_light = light
        add_radiance(count_light, tp * emission, emission)
        mis = light & ~count_light & (cfg["enable_multiple_importance_sampling"] != 0)
        cos_light = np.abs((d * normal).sum(axis=1))
        power = f64(np.float32(0.299)) * emission[:, 0] + f64(np.float32(0.587)) * emission[:, 1] + f64(np.float32(0.114)) * emission[:, 2]
        denominator = cos_light * tables.lights_total_weight
        light_pdf = power * t * t / denominator
        if tables.sky_share > 0:
            light_pdf = light_pdf * f64(np.float32(1.0) - np.float32(tables.sky_share))
        threshold = f64(np.float32(1e-4))
        valid = np.isfinite(light_pdf) & (light_pdf > threshold) & (light_pdf <= FLT_MAX) & (denominator >= FLT_MIN)
        # near: around 1e-4, around the largest float, and where the float32 denominator is denormal or underflows
        r.near_pdf = mis & (~(np.abs(light_pdf - threshold) > margins["light_pdf"] * (1.0 + 1.0 / cos_light) * threshold)
                            | ((light_pdf > 0.5 * FLT_MAX) & np.isfinite(light_pdf)) | ((denominator < 4.0 * FLT_MIN) & (denominator > 0)) | ~np.isfinite(t))
        if "pdf" in flip:
            valid = ~valid
        b2 = e.last_pdf.astype(f64) ** 2
        weight = b2 / (b2 + light_pdf * light_pdf)
        contribution = tp * emission * weight[:, None]
        add = mis & valid
        aov_add(RADIANCE, add, contribution)
        aov_add(DIRECT, add & (bounce == 1), contribution); aov_add(INDIRECT, add & (bounce != 1), contribution)
        r.light_pdf = np.where(mis, light_pdf, nan); r.cos_light = np.where(mis, cos_light, nan)
        # where float32 neither underflows nor overflows on the way to light_pdf: the entries its error can be measured on
        r.pdf_in_range = mis & (denominator >= 4.0 * FLT_MIN) & (light_pdf < 0.5 * FLT_MAX) & (t * t > 4.0 * FLT_MIN) & (light_pdf > 4.0 * FLT_MIN)
        r.weight = np.where(add, weight, r.weight)
        outcome[light] = TERMINATED

        # ---- surfaces
        live = outcome < 0
        died, tp_after = roulette(live, tp)
        tp = np.where(live[:, None], tp_after, tp)
        outcome[live & died] = TERMINATED
        survive = live & ~died
        outcome[survive] = mtype[survive] - 1
    r.outcome = outcome
    r.throughput_out = tp
    r.finite = np.isfinite(tp).all(axis=1)
    r.near = r.near_roulette | r.near_wavelength0 | r.near_wavelength1 | r.near_scatter | r.near_pdf | r.near_cell
    r.robust = ~r.near & r.finite
    r.reaches_comparison = can | ~np.isnan(r.survival) | mis | weighed
    r.aov, r.touched = aov, touched
    r.scattering = can
    r.inside = inside
    r.miss = miss
    return r


def allowed_outcomes(tables, launch, margins, result):
    """(N, 6) bool: the outcomes float64 allows each entry -- its own, and for an entry next to a threshold those it reaches with that
    comparison taken the other way."""
    allowed = np.zeros((launch.entries.n, 6), bool)
    allowed[np.arange(launch.entries.n), result.outcome] = True
    near = {"scatter": result.near_scatter, "roulette": result.near_roulette, "wavelength0": result.near_wavelength0, "wavelength1": result.near_wavelength1}
    for name in OUTCOME_FLIPS:
        if near[name].any():
            other = evaluate(tables, launch, margins, flip=frozenset([name])).outcome
            allowed[np.nonzero(near[name])[0], other[near[name]]] = True
    loose = ~result.finite   # a NaN met on the way: comparisons with it are false on every side, but float64 cannot say which float32 operation made it first
    allowed[loose] = True
    return allowed
