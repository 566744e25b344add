"""Inputs of the firefly-robust noise estimate's tests, shared by test_robust_noise.py (no GPU) and test_gpu_robust_noise.py. Everything is
float32 and seeded: the same bits on every machine."""
import numpy as np

import firefly_cases
import firefly_reference as fireflies
import noise_reference as noise

F = np.float32
FLOOR = 1e-2
TAU = 0.25
SIZES = [(1, 1), (16, 16), (17, 33), (130, 17)]   # width, height: a lone pixel, a lone whole cell, cells clipped both ways, three resolve tiles in a row and a clipped one
TIER_COUNTS = [2, 6, 8]

PLANTED_SIZE, PLANTED_SAMPLES, PLANTED_VALUE = 32, 16, 50.0
LONE = [(2, 3), (5, 9), (8, 12), (11, 5), (13, 14)]   # (y, x) in cell 0, no two within each other's 3 x 3 neighbourhood
BLOCK = [(6, 6), (6, 7), (7, 6), (7, 7)]


def planted_frame(kind, start=1.0, tiers=6, support=4.0):
    """The frame of the issue: 32 x 32, 16 grey lognormal samples around 0.05 per pixel (relative deviation 0.25), and one sample of 50 in each of the five LONE
    pixels (kind "lone"), in each pixel of the 2 x 2 BLOCK (kind "block"), or nowhere (kind "none"). Folded from sample index 1, so w = 16. Returns mean, moments,
    tiers and the float32 resolve."""
    rng = np.random.default_rng(20181204)
    n = PLANTED_SIZE
    level = (0.05 * np.exp(rng.normal(-0.25 ** 2 / 2, 0.25, (PLANTED_SAMPLES, n, n)))).astype(F)
    for y, x in {"none": [], "lone": LONE, "block": BLOCK}[kind]:
        level[5, y, x] = PLANTED_VALUE
    frames = np.ones((PLANTED_SAMPLES, n, n, 4), F); frames[..., :3] = level[..., None]
    zero = np.zeros((n, n, 4), F)
    mean, moments, final = noise.accumulate(frames, zero, zero, 1)
    state = fireflies.accumulate(frames, np.zeros((tiers, n, n, 4), F), 1, start, np.float32)
    resolved = fireflies.resolve(mean, moments, state, final, start=start, support=support, dtype=np.float32)
    return {"mean": mean, "moments": moments, "tiers": state, "resolved": resolved, "fallback": final}


def padded(image, pitch, sentinel=firefly_cases.SENTINEL):
    """(height, width, 4) -> (height, pitch, 4) with the sentinel in the padding columns."""
    height, width = image.shape[:2]
    out = np.full((height, pitch, 4), sentinel, np.uint32).view(F).copy()
    out[:, :width] = image
    return out


def probe_case(width, height, pitch, tiers, seed=0):
    """Images for the robust probes: firefly_cases.resolve_case (sample counts 1 .. 40, rare bright samples, an invalid pixel of every kind, the sentinel in the
    padding) with its float32 resolve beside it, and -- where there is room -- a pixel with M2 not finite and one the resolve calls invalid that takes part."""
    images = dict(firefly_cases.resolve_case(width, height, pitch, tiers, seed))
    moments = images["moments"].copy()
    if width * height >= 64:
        moments[height // 2, width // 3, 1] = np.inf
    images["moments"] = moments
    resolved = fireflies.resolve(images["mean"], moments, images["tiers"], images["fallback"], width=width, dtype=np.float32)
    # every seventh pixel's held-back luminance is set by hand, in turn: the pixel's own bound tau * max(Y, floor), one float32 step above it, four times it, the
    # resolve's "not valid", NaN, nothing -- so that every frame, the 1 x 1 one too, meets the comparison on both sides (with few tiers a resolve holds little back)
    mean = images["mean"][:, :width]
    with np.errstate(all="ignore"):
        lum = (noise.LUMINANCE[0] * mean[..., 0] + noise.LUMINANCE[1] * mean[..., 1]) + noise.LUMINANCE[2] * mean[..., 2]
        bound = (F(TAU) * np.fmax(lum, F(FLOOR))).astype(F)
        above = np.nextafter(bound, F(np.inf))
    y, x = np.mgrid[0:height, 0:width]
    linear = x + y * width
    turn = np.where(linear % 7 == 0, (linear // 7 + seed + tiers) % 6, -1)
    for k, value in enumerate((bound, above, bound * F(4), np.full_like(bound, -1), np.full_like(bound, np.nan), np.zeros_like(bound))):
        resolved[..., 3] = np.where(turn == k, value, resolved[..., 3])
    images["resolved"] = padded(resolved, pitch)
    for image in images.values():
        image.setflags(write=False)
    return images
