"""References for the noise estimate: a numpy float32 REPLAY of the accumulate fold with second moments and of the per-pixel error, in the
expression shapes the kernels are written in (every operation a single float32 operation, no contraction), a replay of the cells' double reduction tree,
and a float64 restatement (two passes over samples 1..n) the replay is measured against. Nothing here imports the product."""
import numpy as np

F = np.float32
U = 2.0 ** -24           # unit roundoff of float32
CELL = 16
LUMINANCE = (F(0.299), F(0.587), F(0.114))   # `luminance` of csrc/rt_shading.h


def fold(acc, m2, fb, n):
    """One sample `fb` folded at sample index n (AOV.h:35-46 with its quirk: sample 1 overwrites sample 0). acc, m2, fb: (..., 4) float32. Returns new (acc, m2).
    m2 = (M2_r, M2_g, M2_b, w); m2 None: the plain fold."""
    n = F(n)
    with np.errstate(all="ignore"):
        if not n > 0:
            new_acc = fb.copy()
            new_m2 = None if m2 is None else np.broadcast_to(np.array([0, 0, 0, 1], F), m2.shape).copy()
            return new_acc, new_m2
        d = fb - acc
        new_acc = acc + d / n
        if m2 is None:
            return new_acc, None
        if n >= 2:
            new_m2 = m2.copy()
            new_m2[..., :3] = m2[..., :3] + (d * (fb - new_acc))[..., :3]
            new_m2[..., 3] = n
        else:
            new_m2 = np.broadcast_to(np.array([0, 0, 0, 1], F), m2.shape).copy()
    return new_acc, new_m2


def accumulate(frames, accumulator, moments, first_sample, mask=None):
    """frames (S, ..., 4) folded in order from sample index first_sample into copies of accumulator / moments (moments None: plain). mask (...): the pixels
    of the set; the others keep what they had. Returns (accumulator, moments, final_image-as-the-kernel-writes-it)."""
    acc, m2 = accumulator.astype(F).copy(), None if moments is None else moments.astype(F).copy()
    for s in range(frames.shape[0]):
        acc, m2 = fold(acc, m2, frames[s].astype(F), first_sample + s)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite((acc[..., 0] + acc[..., 1]) + acc[..., 2])
    final = acc.copy()
    final[bad] = np.array([1000, 0, 1000, 1], F)   # the NaN guard of kernel_accumulate
    if mask is not None:
        acc = np.where(mask[..., None], acc, accumulator)
        if m2 is not None:
            m2 = np.where(mask[..., None], m2, moments)
    return acc, m2, final


def accumulate_group(frames, accumulator, moments, first_samples, sample_counts, mask=None):
    """The submissions of a group, one after the other: the same folds in the same order."""
    acc, m2, final, at = accumulator, moments, None, 0
    for first, count in zip(first_samples, sample_counts):
        acc, m2, final = accumulate(frames[at:at + count], acc, m2, first, mask)
        at += count
    return acc, m2, final


def pixel_error(mean, m2, floor):
    """(e_p, participates, nonfinite) for images (..., 4) float32: e_p = sqrtf(v / (w * (w - 1))) / fmaxf(luminance(mean), floor), v = (M2_r + M2_g) + M2_b."""
    mean, m2, floor = mean.astype(F), m2.astype(F), F(floor)
    w = m2[..., 3]
    with np.errstate(all="ignore"):
        enough = w >= 2
        finite = np.isfinite(mean[..., :3]).all(-1) & np.isfinite(m2[..., :3]).all(-1)
        v = (m2[..., 0] + m2[..., 1]) + m2[..., 2]
        lum = (LUMINANCE[0] * mean[..., 0] + LUMINANCE[1] * mean[..., 1]) + LUMINANCE[2] * mean[..., 2]
        e = np.sqrt(v / (w * (w - F(1)))) / np.fmax(lum, floor)
    return e.astype(F), enough & finite, enough & ~finite


def tree_sum(values256):
    """The cell's reduction: s[t] += s[t + stride] for stride 128, 64, ..., 1 on 256 doubles."""
    s = np.array(values256, np.float64).copy()
    assert s.shape == (256,)
    stride = 128
    with np.errstate(all="ignore"):
        while stride >= 1:
            s[:stride] = s[:stride] + s[stride:2 * stride]
            stride //= 2
    return s[0]


def estimate(mean, m2, width, floor):
    """rt_estimate_noise on pitched images (height, pitch, 4): dict with pixel_map (height, pitch; -1 no part -- padding too --, -2 non-finite), cell_sums,
    cell_counts, cell_nonfinite (cells_y, cells_x), pixels, nonfinite_pixels, mean (cell sums added in cell order over the count)."""
    height, pitch = mean.shape[:2]
    e, part, bad = pixel_error(mean, m2, floor)
    inside = np.zeros((height, pitch), bool); inside[:, :width] = True
    part, bad = part & inside, bad & inside
    pixel_map = np.full((height, pitch), -1, F)
    pixel_map[part] = e[part]; pixel_map[bad] = -2
    cells_x, cells_y = (width + CELL - 1) // CELL, (height + CELL - 1) // CELL
    sums, counts, nonfinite = np.zeros((cells_y, cells_x)), np.zeros((cells_y, cells_x), np.int32), np.zeros((cells_y, cells_x), np.int32)
    for cy in range(cells_y):
        for cx in range(cells_x):
            block = np.zeros((CELL, CELL))
            ys, xs = slice(cy * CELL, min((cy + 1) * CELL, height)), slice(cx * CELL, min((cx + 1) * CELL, width))
            sub = np.where(part[ys, xs], e[ys, xs].astype(np.float64), 0.0)
            block[:sub.shape[0], :sub.shape[1]] = sub
            sums[cy, cx] = tree_sum(block.ravel())          # thread t = ly * 16 + lx
            counts[cy, cx] = part[ys, xs].sum(); nonfinite[cy, cx] = bad[ys, xs].sum()
    total = 0.0
    with np.errstate(all="ignore"):
        for v in sums.ravel():
            total = total + v
    pixels = int(counts.sum())
    return {"pixel_map": pixel_map, "cell_sums": sums, "cell_counts": counts, "cell_nonfinite": nonfinite, "pixels": pixels,
            "nonfinite_pixels": int(nonfinite.sum()), "mean": total / pixels if pixels else 0.0}


def moments64(samples):
    """float64 restatement for samples (S, ...) float32, S >= 2: mean and M2 over samples 1 .. S-1 (sample 0 is overwritten), two passes."""
    x = samples[1:].astype(np.float64)
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).sum(0)


def summary(cell_sums, cell_counts, quantile):
    """grt_noise_summary: (mean, figure) -- the quantile of the cell means over cells with a count, nearest rank on the sorted means."""
    sums, counts = np.asarray(cell_sums, np.float64).ravel(), np.asarray(cell_counts).ravel()
    keep = counts > 0
    if not keep.any():
        return 0.0, 0.0
    total = 0.0
    for v in sums[keep]:
        total += v
    means = np.sort(sums[keep] / counts[keep])
    rank = min(max(int(np.ceil(quantile * len(means))), 1), len(means))
    return total / counts[keep].sum(), means[rank - 1]
