"""References for the firefly-robust noise estimate: the float32 restatement of the robust cells -- noise_reference's per-pixel error and
reduction tree with the held pixels taken out -- and of the selection's second clause. Nothing here imports the product."""
import numpy as np

import adaptive_reference as adaptive
import noise_reference as noise

F = np.float32
CELL = noise.CELL
TAU = 0.25   # the host's default held_fraction


def held_pixels(mean, m2, resolved, floor, tau):
    """(height, pitch) bool: the pixels that take part by the plain rule and that the resolve holds back: resolved.w >= 0 and, in float32,
    resolved.w > tau * fmaxf(luminance(mean), floor)."""
    mean, resolved = np.asarray(mean, F), np.asarray(resolved, F)
    _, part, _ = noise.pixel_error(mean, m2, floor)
    with np.errstate(all="ignore"):
        lum = (noise.LUMINANCE[0] * mean[..., 0] + noise.LUMINANCE[1] * mean[..., 1]) + noise.LUMINANCE[2] * mean[..., 2]
        r = resolved[..., 3]
        return part & (r >= 0) & (r > F(tau) * np.fmax(lum, F(floor)))


def estimate(mean, m2, resolved, width, floor, tau=TAU):
    """rt_estimate_noise_robust_images on pitched images (height, pitch, 4): noise_reference.estimate's dict with the held pixels left out of sums and counts,
    -3 in the map, counted in cell_held (cells_y, cells_x) and held_pixels."""
    height, pitch = mean.shape[:2]
    e, part, bad = noise.pixel_error(mean, m2, floor)
    inside = np.zeros((height, pitch), bool); inside[:, :width] = True
    held = held_pixels(mean, m2, resolved, floor, tau) & inside
    part, bad = part & inside & ~held, bad & inside
    pixel_map = np.full((height, pitch), -1, F)
    pixel_map[part] = e[part]; pixel_map[bad] = -2; pixel_map[held] = -3
    cells_x, cells_y = (width + CELL - 1) // CELL, (height + CELL - 1) // CELL
    sums = np.zeros((cells_y, cells_x))
    counts, nonfinite, back = (np.zeros((cells_y, cells_x), np.int32) for _ in range(3))
    for cy in range(cells_y):
        for cx in range(cells_x):
            block = np.zeros((CELL, CELL))
            ys, xs = slice(cy * CELL, min((cy + 1) * CELL, height)), slice(cx * CELL, min((cx + 1) * CELL, width))
            sub = np.where(part[ys, xs], e[ys, xs].astype(np.float64), 0.0)
            block[:sub.shape[0], :sub.shape[1]] = sub
            sums[cy, cx] = noise.tree_sum(block.ravel())
            counts[cy, cx] = part[ys, xs].sum(); nonfinite[cy, cx] = bad[ys, xs].sum(); back[cy, cx] = held[ys, xs].sum()
    total = 0.0
    with np.errstate(all="ignore"):
        for v in sums.ravel():
            total = total + v
    pixels = int(counts.sum())
    return {"pixel_map": pixel_map, "cell_sums": sums, "cell_counts": counts, "cell_nonfinite": nonfinite, "cell_held": back, "pixels": pixels,
            "nonfinite_pixels": int(nonfinite.sum()), "held_pixels": int(back.sum()), "mean": total / pixels if pixels else 0.0}


def select(cell_sums, cell_counts, cell_nonfinite, cell_held, width, height, threshold, dilate):
    """(hot, active): adaptive_reference.select with the held pixels counted as judged, as the non-finite ones are."""
    return adaptive.select(cell_sums, cell_counts, np.asarray(cell_nonfinite, np.int64) + np.asarray(cell_held, np.int64), width, height, threshold, dilate)
