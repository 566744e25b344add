"""Inputs of the firefly filter's tests, shared by test_fireflies.py (no GPU) and test_gpu_fireflies.py. Everything is float32 and seeded: the
same bits on every machine."""
import numpy as np

SENTINEL = 0x7fc0dead
SIZES = [(1, 1), (3, 2), (63, 5), (64, 8), (65, 9), (130, 17)]   # width, height: below, at and above the 64-pixel tile row; no multiple of the 8 (4) tile rows
TIER_COUNTS = [2, 6, 8]
STARTS = [0, 1, 5]   # the first fold index of a launch: sample 0 (sets the mean), sample 1 (overwrites it), a running mean
LUMA = np.array([0.299, 0.587, 0.114], np.float32)


def sentinel_image(shape):
    return np.full(shape, SENTINEL, np.uint32).view(np.float32)


def boundaries(tiers, start=1.0):
    b = [np.float32(start)]
    for _ in range(tiers - 1):
        b.append(np.float32(b[-1] * np.float32(8)))
    return np.array(b, np.float32)


def palette(tiers, start=1.0):
    """Grey levels (their luminance is the level to within an ulp: the weights sum to 1) on every tier boundary, one float32 step below and above it, 0, negative,
    far above the top tier, and NaN / inf."""
    b = boundaries(tiers, start)
    levels = [0.0, -2.5, np.nan, np.inf, float(b[-1]) * 100.0, float(b[0]) * 0.25]
    for x in b:
        levels += [float(x), float(np.nextafter(x, np.float32(0))), float(np.nextafter(x, np.float32(np.inf))), float(x) * 3.0]
    return np.array(levels, np.float32)


def sample_frames(width, height, pitch, samples, tiers, start=1.0, seed=0):
    """(samples, height, pitch, 4) float32: coloured samples whose luminance is log-uniform from a quarter of the lowest boundary to four times the top one, every
    third (pixel, sample) a grey palette level instead; .w = 1; the sentinel in the padding columns."""
    rng = np.random.default_rng(seed + 131 * tiers + width)
    b = boundaries(tiers, start)
    lum = np.exp(rng.uniform(np.log(float(b[0]) * 0.25), np.log(float(b[-1]) * 4.0), (samples, height, width)))
    tint = rng.uniform(0.2, 1.0, (samples, height, width, 3))
    tint /= (tint * LUMA.astype(np.float64)).sum(axis=-1, keepdims=True)
    rgb = (tint * lum[..., None]).astype(np.float32)
    levels = palette(tiers, start)
    s, y, x = np.mgrid[0:samples, 0:height, 0:width]
    linear = x + y * width + s * (width * height + 1) + seed
    grey = linear % 3 == 0
    rgb[grey] = levels[(linear[grey] // 3) % len(levels)][:, None]
    frames = np.tile(sentinel_image((1, height, pitch, 4)), (samples, 1, 1, 1))
    frames[:, :, :width, :3] = rgb
    frames[:, :, :width, 3] = 1.0
    return frames


def running_state(width, height, pitch, tiers, w, seed=0):
    """A plausible state after w >= 2 samples: accumulator, moments (w in .w) and tiers (their W summing to w), finite inside the frame, the sentinel in the padding."""
    rng = np.random.default_rng(seed + 17)
    acc, m2 = sentinel_image((height, pitch, 4)).copy(), sentinel_image((height, pitch, 4)).copy()
    acc[:, :width, :3] = rng.uniform(0.0, 4.0, (height, width, 3)); acc[:, :width, 3] = 1.0
    m2[:, :width, :3] = rng.uniform(0.0, 9.0, (height, width, 3)); m2[:, :width, 3] = float(w)
    state = np.tile(sentinel_image((1, height, pitch, 4)), (tiers, 1, 1, 1))
    share = rng.dirichlet(np.ones(tiers), (height, width)).astype(np.float32)
    for j in range(tiers):
        state[j, :, :width, 3] = share[..., j] * np.float32(w)
        state[j, :, :width, :3] = rng.uniform(0.0, 2.0, (height, width, 3)) * (share[..., j] * np.float32(w) * boundaries(tiers)[j])[..., None]
    return acc, m2, state


def splat_samples(samples, tiers, start, ref, dtype=np.float64):
    """The tiers of pixels that received `samples` ((N, H, W, 3) or (N, H, W, 4)) from fold index 1 on. -> (K, H, W, 4)."""
    samples = np.asarray(samples, np.float32)
    if samples.shape[-1] == 3:
        samples = np.concatenate([samples, np.ones(samples.shape[:-1] + (1,), np.float32)], axis=-1)
    zero = np.zeros((tiers,) + samples.shape[1:], np.float32)
    return ref.accumulate(samples, zero, 1, start, dtype)


def field(samples):
    """mean, moments (w = N) and fallback images for pixels that received `samples` (N, H, W, 3): what the accumulate kernels would hold, to the rounding that
    does not matter here (the resolve reads w and the mean's finiteness only)."""
    samples = np.asarray(samples, np.float64)
    n, h, w = samples.shape[:3]
    mean = np.zeros((h, w, 4), np.float32); mean[..., :3] = samples[..., :3].mean(axis=0); mean[..., 3] = 1.0
    moments = np.zeros((h, w, 4), np.float32); moments[..., 3] = n
    fallback = np.full((h, w, 4), 7.0, np.float32)
    return mean, moments, fallback


def resolve_case(width, height, pitch, tiers, seed=0):
    """Images for the resolve probe: per-pixel sample counts 1 .. 40, tiers splatted from seeded samples (bright ones rare), pitch > width with the sentinel in the
    padding, and -- where there is room -- invalid pixels one rule each: w = 0, w = NaN, a NaN mean, an inf tier colour, a NaN tier W."""
    rng = np.random.default_rng(seed + 1009 * tiers + width)
    b = boundaries(tiers)
    counts = rng.integers(1, 41, (height, width))
    total = int(counts.max())
    bright = rng.uniform(0, 1, (total, height, width)) < 0.06
    lum = np.where(bright, np.exp(rng.uniform(np.log(4.0), np.log(float(b[-1]) * 4.0), bright.shape)), rng.uniform(0.05, 1.5, bright.shape))
    tint = rng.uniform(0.2, 1.0, bright.shape + (3,))
    tint /= (tint * LUMA.astype(np.float64)).sum(axis=-1, keepdims=True)
    samples = np.concatenate([(tint * lum[..., None]), np.ones(bright.shape + (1,))], axis=-1).astype(np.float32)
    taken = np.arange(total)[:, None, None] < counts[None]
    samples[~taken] = np.nan   # a sample that is not finite is not splatted: the pixel has `counts` samples
    import firefly_reference as ref
    state = ref.accumulate(samples, np.zeros((tiers, height, width, 4), np.float32), 1, 1.0, np.float32)
    mean = np.zeros((height, width, 4), np.float32)
    mean[..., :3] = np.where(taken[..., None], samples[..., :3], 0).sum(axis=0) / counts[..., None]; mean[..., 3] = 1.0
    moments = np.zeros((height, width, 4), np.float32); moments[..., :3] = rng.uniform(0, 3, (height, width, 3)); moments[..., 3] = counts
    if width * height >= 64:
        spots = [(int(rng.integers(0, height)), int(rng.integers(0, width))) for _ in range(5)]
        moments[spots[0]][3] = 0.0
        moments[spots[1]][3] = np.nan
        mean[spots[2]][1] = np.nan
        state[tiers - 1][spots[3]][0] = np.inf
        state[0][spots[4]][3] = np.nan
    def padded(image):
        out = np.tile(sentinel_image((1,) * (image.ndim - 3) + (height, pitch, 4)), image.shape[:-3] + (1, 1, 1))
        out[..., :width, :] = image
        return out
    fallback = np.zeros((height, width, 4), np.float32); fallback[..., :3] = rng.uniform(0, 1000, (height, width, 3)); fallback[..., 3] = 1.0
    images = {"mean": padded(mean), "moments": padded(moments), "tiers": padded(state), "fallback": padded(fallback)}
    for image in images.values():
        image.setflags(write=False)
    return images


def relative_rms(image, truth):
    truth = np.asarray(truth, np.float64)
    return float(np.sqrt(np.mean((np.asarray(image, np.float64) - truth) ** 2) / np.mean(truth ** 2)))
