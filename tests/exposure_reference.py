"""References for the exposure measurement: a numpy restatement of the exponent histogram -- the luminance in float32 in the kernel's shape, the
bin read from the float's own bits, so no logarithm enters and device and numpy agree count for count -- and of grt_exposure_start. Nothing here imports the product."""
import numpy as np

import noise_reference as noise

F = np.float32
CLAMP = 96


def luminance(mean):
    mean = np.asarray(mean, F)
    with np.errstate(all="ignore"):
        return ((noise.LUMINANCE[0] * mean[..., 0] + noise.LUMINANCE[1] * mean[..., 1]) + noise.LUMINANCE[2] * mean[..., 2]).astype(F)


def classify(mean, moments, width=None):
    """(bins, dark, nonfinite) over pixels (height, width): bins int64, -1 where the pixel has no bin; dark / nonfinite bool. A pixel with w < 1 (or w NaN) takes no part."""
    mean, moments = np.asarray(mean, F), np.asarray(moments, F)
    width = mean.shape[1] if width is None else width
    mean, moments = mean[:, :width], moments[:, :width]
    with np.errstate(all="ignore"):
        part = moments[..., 3] >= 1
        lum = luminance(mean)
        finite = np.isfinite(mean[..., :3]).all(-1) & np.isfinite(lum)
        nonfinite = part & ~finite
        dark = part & finite & (lum <= 0)
        binned = part & finite & (lum > 0)
    exponent = ((np.ascontiguousarray(lum).view(np.uint32) >> 23) & 255).astype(np.int64)
    return np.where(binned, exponent, -1), dark, nonfinite


def histogram(mean, moments, width=None):
    """rt_measure_exposure: dict with histogram ((256,) uint64), pixels, dark_pixels, nonfinite_pixels."""
    bins, dark, nonfinite = classify(mean, moments, width)
    counts = np.bincount(bins[bins >= 0], minlength=256).astype(np.uint64)
    return {"histogram": counts, "pixels": int(counts.sum()), "dark_pixels": int(dark.sum()), "nonfinite_pixels": int(nonfinite.sum())}


def start(counts, shift=0):
    """grt_exposure_start: (start, exponent) or None for an empty histogram. rank = (pixels + 1) // 2; the median bin is the smallest bin whose cumulative count reaches it."""
    counts = [int(c) for c in np.asarray(counts).ravel()]
    assert len(counts) == 256
    pixels = sum(counts)
    if pixels == 0:
        return None
    rank, reached = (pixels + 1) // 2, 0
    for median, c in enumerate(counts):
        reached += c
        if reached >= rank:
            break
    exponent = min(max(median - 127 + shift, -CLAMP), CLAMP)
    return float(F(2.0) ** F(exponent)), exponent
