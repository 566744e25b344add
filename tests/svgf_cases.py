"""Synthetic frame sequences for the SVGF / TAA filter tests (tests/test_svgf_filter.py, tests/test_gpu_svgf_filter.py).

A case is a frame size, a filter configuration and a list of frames; a frame is what the path tracing of one frame
leaves for the filter -- direct, indirect, albedo, octahedral normal + depth + previous depth, mesh / triangle ids and
the previous screen position -- as (height, pitch, C) float32 arrays, zero in the padding columns (as the device and the
oracle leave them). Geometry is a few analytic surfaces in screen space, with dyadic depths and slopes, so that depths and
depth gradients are exact in float32 and no decision depends on rounding:

* a background plane, depth 10 + x / 64 (slanted in x up to the right border: the depth gradient at x = width - 1 reads the
  padding column where pitch > width), normal facing the camera;
* sky (depth 0) over the top rows, and a foreground block (depth 5, tilted normal) whose edges are silhouettes against both;
* on request: a flat patch whose depth steps from exactly 10.0 to 12.0 (and whose previous depth says 12.0) -- the
  reprojection's |depth - previous| < 2 sits on its threshold --, a patch whose normal turns by 23 degrees (fails the 0.95
  test) next to one that turns by 6 degrees (passes), and a thin strip that is disoccluded at a given frame.

The motion is a screen-space map from a pixel's centre to where it was in the previous frame.
"""
import numpy as np

from svgf_reference import Config

F32 = np.float32
NORMAL_FRONT = (0.5, 0.5)        # octahedral (0, 0, 1)
NORMAL_TILTED = (0.62, 0.44)     # the foreground block
NORMAL_TURN_FAIL = (0.65, 0.5)   # (0.3, 0, 0.7) normalised: n . front = 0.92
NORMAL_TURN_PASS = (0.55, 0.5)   # n . front = 0.995


def pitch_of(width):
    return (width + 31) // 32 * 32


class Case:
    def __init__(self, name, width, height, frames, motion="static", radiance="noisy", config=None, events=(), seed=1):
        self.name, self.width, self.height, self.pitch = name, width, height, pitch_of(width)
        self.config = Config(**(config or {}))
        self.motion, self.radiance, self.events, self.seed = motion, radiance, set(events), seed
        self.n_frames = frames
        self._frames = None

    def __repr__(self):
        return self.name

    @property
    def frames(self):
        if self._frames is None:
            rng = np.random.default_rng(self.seed)
            self._frames = [self._frame(f, rng) for f in range(self.n_frames)]
        return self._frames

    # ---- geometry ---------------------------------------------------------------------------------------------------
    def _geometry(self, f):
        W, H = self.width, self.height
        y, x = np.mgrid[0:H, 0:W]
        depth = (10.0 + x / 64.0).astype(F32)
        depth_prev = depth.copy()
        oct_n = np.empty((H, W, 2), F32)
        oct_n[...] = NORMAL_FRONT
        ids = np.zeros((H, W, 2), np.int32)
        ids[..., 1] = (x // 8 + 16 * (y // 8)).astype(np.int32)
        if H >= 8:   # sky over the top eighth, and where x is a multiple of 23 on the second row (single-pixel holes)
            sky = (y < H // 8) | ((y == H // 8 + 1) & (x % 23 == 5))
        elif W >= 8:
            sky = x < W // 8
        else:
            sky = np.zeros((H, W), bool)
        if W >= 8 and H >= 8:   # the foreground block
            block = (x >= W // 3) & (x < W // 3 + max(2, W // 5)) & (y >= H // 8 - 1) & (y < H // 2)
            depth[block] = 5.0
            depth_prev[block] = 5.0
            oct_n[block] = NORMAL_TILTED
            ids[block, 0] = 1
        if "depth_step" in self.events and W >= 16 and H >= 16:   # frames >= 3: a flat patch steps from 10 to exactly 12
            patch = (x >= 2) & (x < 8) & (y >= H - 8) & (y < H - 2)
            depth[patch] = 12.0 if f >= 3 else 10.0
            depth_prev[patch] = 12.0 if f >= 3 else 10.0
            ids[patch, 0] = 2
        if "normal_turn" in self.events and W >= 32 and H >= 16 and f >= 2:
            turn = (y >= H - 8) & (y < H - 2)
            oct_n[turn & (x >= W - 16) & (x < W - 10)] = NORMAL_TURN_FAIL
            oct_n[turn & (x >= W - 9) & (x < W - 3)] = NORMAL_TURN_PASS
        if "strip" in self.events and f >= 5:   # a two-pixel strip is disoccluded at frame 5: young pixels among old ones
            strip = (x >= W // 2) & (x < W // 2 + 2) & (y >= H // 2) if W >= 4 else (y >= H // 2) & (y < H // 2 + 2)
            depth[strip] += F32(3.0)
            depth_prev[strip] = depth[strip]
        depth[sky] = 0.0
        depth_prev[sky] = 0.0
        oct_n[sky] = 0.0
        ids[sky] = 0
        return depth, depth_prev, oct_n, ids

    # ---- motion: where the centre of a pixel was in the previous frame, in pixels --------------------------------------
    def _previous_position(self, f):
        W, H = self.width, self.height
        y, x = np.mgrid[0:H, 0:W]
        cx, cy = x + 0.5, y + 0.5
        m = self.motion
        if m == "static" or f == 0:
            return cx, cy
        if m == "pan":          # fractional, different each frame
            return cx + 0.37 + 0.11 * f, cy - 0.23
        if m == "half_pixel":   # s_prev = x + 1 exactly: the bilinear weights of the right-hand taps are exactly zero
            return cx + 0.5, cy
        if m == "zoom":
            return W / 2 + (cx - W / 2) * 0.9375, H / 2 + (cy - H / 2) * 0.9375
        if m == "border":       # the left / top borders pushed in and out. At the first column / row the previous positions fall
            # in (-0.5, 0.5), where reprojection's int(s - 0.5) and floor differ, and (frame 2) in (-1.5, -0.5), where TAA's 4 x 4 window
            # holds one tap inside the image (int(s + 0.5) and floor differ there too, but both windows hold that tap and no other)
            dx, dy = ((-0.8, -0.6), (0.9, 0.675), (-1.2, -1.1), (1.3, 0.975), (-0.9, -0.675), (0.55, 0.4125), (-0.75, -0.5625))[f % 7]
            return cx + dx, cy + dy
        raise ValueError(m)

    # ---- radiance -----------------------------------------------------------------------------------------------------
    def _radiance(self, f, rng, depth):
        W, H = self.width, self.height
        y, x = np.mgrid[0:H, 0:W]
        smooth = 1.0 + 0.3 * np.sin(0.21 * x + 0.13 * y)[..., None] * np.array([1.0, 0.8, 0.6])
        direct = smooth * np.array([0.9, 0.7, 0.5])
        indirect = (1.0 + 0.2 * np.cos(0.17 * x - 0.11 * y))[..., None] * np.array([0.3, 0.35, 0.4])
        if self.radiance in ("noisy", "fireflies"):
            direct = direct * (1.0 + 0.6 * (rng.random((H, W, 1)) - 0.5))
            indirect = indirect * (1.0 + 0.8 * (rng.random((H, W, 3)) - 0.5))
        if self.radiance == "fireflies":   # fireflies of 1e4 (their weights underflow) and exact zeros
            hot = rng.random((H, W)) < 0.01
            direct[hot] = 1.0e4
            indirect[(rng.random((H, W)) < 0.005)] = 1.0e4
            direct[(x >= 3) & (x < 9)] = 0.0
            indirect[(y >= H - 3)] = 0.0
        direct[depth == 0] *= 0.5   # the sky's own radiance
        indirect[depth == 0] = 0.0
        albedo = (0.5 + 0.3 * np.sin(0.05 * x + 0.07 * y))[..., None] * np.array([1.0, 0.9, 0.8])
        albedo[depth == 0] = 1.0
        return direct, indirect, albedo

    def _frame(self, f, rng):
        W, H, P = self.width, self.height, self.pitch
        depth, depth_prev, oct_n, ids = self._geometry(f)
        direct, indirect, albedo = self._radiance(f, rng, depth)
        sx, sy = self._previous_position(f)
        out = {k: np.zeros((H, P, c), F32) for k, c in (("direct", 4), ("indirect", 4), ("albedo", 4), ("normal_and_depth", 4), ("screen_position_prev", 2))}
        out["mesh_and_triangle"] = np.zeros((H, P, 2), np.int32)
        out["direct"][:, :W, :3] = direct
        out["indirect"][:, :W, :3] = indirect
        out["albedo"][:, :W, :3] = albedo
        out["normal_and_depth"][:, :W] = np.concatenate([oct_n, depth[..., None], depth_prev[..., None]], axis=-1)
        out["screen_position_prev"][:, :W, 0] = (2.0 * sx / W - 1.0).astype(F32)
        out["screen_position_prev"][:, :W, 1] = (2.0 * sy / H - 1.0).astype(F32)
        out["mesh_and_triangle"][:, :W] = ids
        return out


def cases():
    """Small on purpose: the GPU file runs every case twice (SVGF tiles on and off)."""
    return [
        # pitch == width: the listed variance pass
        Case("pan_64x48_it6", 64, 48, 7, motion="pan", events=("depth_step", "normal_turn", "strip")),
        Case("half_pixel_64x48_it2", 64, 48, 5, motion="half_pixel", config=dict(num_atrous_iterations=2)),
        Case("zoom_256x64_it1_no_taa", 256, 64, 3, motion="zoom", config=dict(num_atrous_iterations=1, enable_taa=0)),   # frame 0: 14 000 young pixels, the stride loop
        Case("sigma_n0_64x48_it2", 64, 48, 4, motion="pan", radiance="smooth",
             config=dict(num_atrous_iterations=2, sigma_n=0.0, sigma_l=3.0, alpha_colour=0.2, alpha_moment=0.3, enable_taa=0)),
        Case("fireflies_64x48_it6_no_taa", 64, 48, 5, motion="static", radiance="fireflies", config=dict(enable_taa=0)),
        # pitch != width: the full-frame variance pass, its padding-column copies, the depth gradient at the last column
        Case("zoom_333x77_it6", 333, 77, 5, motion="zoom", events=("normal_turn",)),
        Case("border_65x33_it7", 65, 33, 7, motion="border", events=("depth_step", "strip"), config=dict(num_atrous_iterations=7)),
        Case("column_1x70_it10", 1, 70, 5, motion="pan", config=dict(num_atrous_iterations=10)),
        Case("row_97x1_it10_no_variance", 97, 1, 5, motion="border", config=dict(num_atrous_iterations=10, enable_spatial_variance=0)),
        Case("sigma_n0_65x33_it6", 65, 33, 4, motion="zoom", config=dict(sigma_n=0.0)),
        # the last pass at steps 4, 8 and 16 (the fused finalize of those tiled instantiations)
        Case("static_48x40_it3", 48, 40, 3, config=dict(num_atrous_iterations=3)),
        Case("pan_40x24_it4", 40, 24, 3, motion="pan", config=dict(num_atrous_iterations=4)),
        Case("zoom_70x20_it5", 70, 20, 3, motion="zoom", config=dict(num_atrous_iterations=5)),
        # no pass uses the fast weights: bit-identical to the oracle
        Case("exact_64x48", 64, 48, 7, motion="pan", events=("depth_step", "normal_turn", "strip"), config=dict(num_atrous_iterations=0, enable_spatial_variance=0)),
        Case("exact_65x33_border", 65, 33, 7, motion="border", events=("depth_step", "strip"), config=dict(num_atrous_iterations=0, enable_spatial_variance=0)),
    ]


def exact(case):
    """No pass of this case goes through edge_stopping_weights: everything it computes is IEEE float32 in a fixed order."""
    return case.config.num_atrous_iterations == 0 and not case.config.enable_spatial_variance


# ---- running a case through the oracle, and comparing images -------------------------------------------------------------
def config_kwargs(case):
    """grt.config_set keywords of a case (SVGF on)."""
    c = case.config
    return dict(enable_svgf=1, enable_spatial_variance=c.enable_spatial_variance, enable_taa=c.enable_taa, num_atrous_iterations=c.num_atrous_iterations,
                alpha_colour=c.alpha_colour, alpha_moment=c.alpha_moment, sigma_z=c.sigma_z, sigma_n=c.sigma_n, sigma_l=c.sigma_l)


class OracleRun:
    """The oracle's Frame fed a case's frames through Frame.svgf_inputs() / Frame.filter_frame()."""

    def __init__(self, oracle, view, case):
        s = view.scene
        assert (s.screen_width, s.screen_height, s.screen_pitch) == (case.width, case.height, case.pitch)
        assert s.config.enable_svgf and s.config.num_atrous_iterations == case.config.num_atrous_iterations
        self.case, self.frame = case, oracle.Frame(view)

    def step(self, inputs, sample_index):
        arrays = self.frame.svgf_inputs()
        for name, a in arrays.items():
            a[...] = inputs[name].reshape(a.shape)
        self.frame.filter_frame(sample_index)
        return self.state()

    def state(self):
        """name -> (height, pitch, C) image, the names of read_svgf_state plus `final`. `taa_current`: the frame's tone-mapped
        colour the TAA resolve reads."""
        H, P = self.case.height, self.case.pitch
        b = self.frame.buffers
        img = lambda a: a.reshape(H, P, -1).copy()
        return {"history_length": img(b["hl"]), "history_direct": img(b["hd"]), "history_indirect": img(b["hi"]), "history_moment": img(b["hm"]),
                "history_normal_and_depth": img(b["hnd"]), "frame_moment": img(b["mom"]), "taa_history": img(b["tp"]), "taa_current": img(b["tc"]),
                "final": self.frame.final.copy()}


def reference_state(ref):
    """The same names for a svgf_reference.Filter."""
    return {"history_length": ref.history_length[..., None], "history_direct": ref.history_direct, "history_indirect": ref.history_indirect,
            "history_moment": ref.history_moment, "history_normal_and_depth": ref.history_normal_and_depth, "frame_moment": ref.moment,
            "taa_history": ref.taa_prev, "taa_current": ref.taa_curr, "final": ref.final}


# images compared value for value: (name, channels); the variances (.w of the two histories) go by `variance_errors`.
# `taa_current`, the colour TAA resolves, is upstream of the clamp: no allowance ever applies to it.
VALUE_IMAGES = (("final", slice(0, 3)), ("history_direct", slice(0, 3)), ("history_indirect", slice(0, 3)), ("history_moment", slice(0, 4)),
                ("frame_moment", slice(0, 4)), ("taa_history", slice(0, 3)), ("taa_current", slice(0, 4)))
FLOOR = 0.1   # the relative error's floor, as a fraction of the image channel's mean magnitude


def value_errors(got, want, width, channels, slack=None):
    """Per pixel and channel: (|got - want| - slack) / max(|want|, FLOOR x the channel's mean |want| over the image); the
    maximum. `slack` (height, pitch): what the TAA clamp's conditioning allows a pixel beyond that (Filter.taa_slack)."""
    g = got[:, :width, channels].astype(np.float64)
    w = want[:, :width, channels].astype(np.float64)
    floor = FLOOR * np.abs(w).reshape(-1, w.shape[-1]).mean(axis=0)
    scale = np.maximum(np.abs(w), np.maximum(floor, 1e-30))
    d = np.abs(g - w)
    if slack is not None:
        d = np.maximum(0.0, d - slack[:, :width, None])
    return float(np.max(d / scale)) if g.size else 0.0


def variance_errors(got, want, second_moment, width):
    """A variance next to E[x^2] (that of the pixel, floored at FLOOR x its mean): the difference of E[x^2] and E[x]^2 is
    compared at the scale of what it was formed from."""
    g = got[:, :width].astype(np.float64)
    w = want[:, :width].astype(np.float64)
    m = np.abs(second_moment[:, :width].astype(np.float64))
    scale = np.maximum(m, np.maximum(FLOOR * m.mean(), 1e-30))
    return float(np.max(np.abs(g - w) / scale)) if g.size else 0.0


def state_errors(got, want, width, taa_slack=None):
    """name -> worst relative error of `got` against `want` (both state dicts); `taa_slack`: (resolved, displayed) per-pixel
    allowances of the TAA clamp (Filter.taa_slack), for the TAA history and, with TAA on, the final image."""
    slack = dict(zip(("taa_history", "final"), taa_slack)) if taa_slack is not None else {}
    out = {name: value_errors(got[name], want[name], width, ch, slack.get(name)) for name, ch in VALUE_IMAGES}
    out["variance_direct"] = variance_errors(got["history_direct"][..., 3], want["history_direct"][..., 3], want["history_moment"][..., 2], width)
    out["variance_indirect"] = variance_errors(got["history_indirect"][..., 3], want["history_indirect"][..., 3], want["history_moment"][..., 3], width)
    return out
