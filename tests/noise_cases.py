"""The inputs of the noise tests: sample streams per pixel, laid over the two probe frames (40 x 24 at pitch 64: 3 x 2 cells, clipped on both edges; 16 x 16)."""
import numpy as np

F = np.float32
FRAMES = {"40x24": (40, 24, 64), "16x16": (16, 16, 32)}   # width, height, pitch = round_up(width, 32)
SENTINEL = 0x7fc0dead                                      # a NaN pattern no fold produces
KINDS = ("constant", "lognormal", "firefly_at_0", "firefly_at_1", "firefly_at_last", "zeros", "denormals", "huge", "nan_sample", "tight", "uniform")


def kind_map(width, height, pitch):
    """Which stream a pixel carries: kind index by scan position, so every cell holds every kind; -1 in the padding columns."""
    k = np.full((height, pitch), -1, np.int32)
    k[:, :width] = (np.arange(width)[None, :] + 3 * np.arange(height)[:, None]) % len(KINDS)
    return k


def streams(kind, samples, count, rng):
    """(samples, count, 3) float32 for `count` pixels of one kind."""
    shape = (samples, count, 3)
    if kind == "constant":
        x = np.broadcast_to(rng.uniform(0.1, 4.0, (1, count, 3)), shape).copy()
    elif kind == "lognormal":
        x = rng.lognormal(0.0, 1.0, shape)
    elif kind.startswith("firefly_at_"):
        x = rng.uniform(0.5, 1.5, shape)
        x[{"0": 0, "1": 1, "last": samples - 1}[kind[11:]]] = 1e4
    elif kind == "zeros":
        x = np.zeros(shape)
    elif kind == "denormals":
        x = rng.uniform(1.0, 200.0, shape) * 1e-41
    elif kind == "huge":
        x = rng.uniform(0.5, 1.0, shape) * 1e30
    elif kind == "nan_sample":
        x = rng.uniform(0.5, 1.5, shape)
        x[min(2, samples - 1), :, 1] = np.nan
    elif kind == "tight":
        x = 1000.0 + rng.normal(0.0, 1e-2, shape)
    elif kind == "uniform":
        x = rng.uniform(0.0, 1.0, shape)
    else:
        raise KeyError(kind)
    return x.astype(F)


def sample_frames(frame, samples, seed=7):
    """(samples, height, pitch, 4) float32 sample frames of FRAMES[frame] with every kind in every cell (w channel: the alpha the shade kernels write, 1);
    the padding columns hold the sentinel. Returns (frames, kind_map)."""
    width, height, pitch = FRAMES[frame]
    rng = np.random.default_rng(seed)
    kinds = kind_map(width, height, pitch)
    frames = np.empty((samples, height, pitch, 4), F)
    frames.view(np.uint32)[...] = SENTINEL
    for i, kind in enumerate(KINDS):
        at = kinds == i
        frames[:, at, :3] = streams(kind, samples, int(at.sum()), rng)
        frames[:, at, 3] = 1
    return frames, kinds


def sentinel_image(frame):
    width, height, pitch = FRAMES[frame]
    image = np.empty((height, pitch, 4), F)
    image.view(np.uint32)[...] = SENTINEL
    return image


def pixel_set_mask(frame, offset=0, count=-1, tiles=None):
    """(height, pitch) bool: the pixels rt_set_pixel_range(offset, count) or rt_set_pixel_tiles(*tiles) = (tile_pixels, first, stride) names."""
    width, height, pitch = FRAMES[frame]
    total = width * height
    scan = np.zeros(total, bool)
    if tiles is None:
        scan[offset:total if count < 0 else offset + count] = True
    else:
        tile_pixels, first, stride = tiles
        tile = np.arange(total) // tile_pixels
        scan[(tile % stride) == first] = True
    mask = np.zeros((height, pitch), bool)
    mask[:, :width] = scan.reshape(height, width)
    return mask


# streams for the float64 comparison on the CPU: (name, function of (rng, n) -> (n + 1,) float32, sample 0 included)
CPU_STREAMS = {
    "lognormal": lambda rng, n: rng.lognormal(0.0, 1.0, n + 1),
    "tight": lambda rng, n: 1000.0 + rng.normal(0.0, 1e-2, n + 1),
    "firefly": lambda rng, n: np.where(rng.uniform(size=n + 1) < 0.02, 1e4, 1e-2),
    "uniform": lambda rng, n: rng.uniform(0.0, 1.0, n + 1),
}
CPU_COUNTS = tuple(range(2, 256))
CPU_SEEDS = (1, 2, 3)
