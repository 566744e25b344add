"""References for adaptive sampling: a numpy restatement of the cell selection (hot and active flags from the cell arrays of the noise
estimate) and of the pixel list (order and density), and a float32 replay of the list accumulate step -- every pixel folded with its own sample count --
that reuses the fold of noise_reference.py. Nothing here imports the product."""
import numpy as np

import noise_reference as noise

F = np.float32
CELL = noise.CELL
PATCH = 8
PATCH_ORDER = ((0, 0), (8, 0), (0, 8), (8, 8))   # (x, y) of the four patches of a cell, in list order


def cell_grid(width, height):
    return (width + CELL - 1) // CELL, (height + CELL - 1) // CELL


def frame_pixels(width, height):
    """(cells_y, cells_x) int: the in-frame pixels of every cell (edge cells are clipped)."""
    cells_x, cells_y = cell_grid(width, height)
    w = np.minimum(CELL, width - CELL * np.arange(cells_x))
    h = np.minimum(CELL, height - CELL * np.arange(cells_y))
    return h[:, None] * w[None, :]


def select(cell_sums, cell_counts, cell_nonfinite, width, height, threshold, dilate):
    """(hot, active), (cells_y, cells_x) bool each. Hot: count > 0 and sum > double(threshold) * double(count), or count + nonfinite < the cell's in-frame
    pixels. Active: hot, or with dilate = 1 one of the up to 8 neighbours inside the grid hot."""
    sums, counts, nonfinite = np.asarray(cell_sums, np.float64), np.asarray(cell_counts, np.int64), np.asarray(cell_nonfinite, np.int64)
    with np.errstate(all="ignore"):
        above = (counts > 0) & (sums > np.float64(F(threshold)) * counts.astype(np.float64))
    hot = above | (counts + nonfinite < frame_pixels(width, height))
    active = hot.copy()
    if dilate:
        padded = np.zeros((hot.shape[0] + 2, hot.shape[1] + 2), bool)
        padded[1:-1, 1:-1] = hot
        for dy in range(3):
            for dx in range(3):
                active |= padded[dy:dy + hot.shape[0], dx:dx + hot.shape[1]]
    return hot, active


def pixel_list(active, width, height):
    """The list: uint32 x + y * width of the in-frame pixels of the active cells; cells by ascending index, inside a cell the patches in PATCH_ORDER,
    a patch row by row. Vectorised: the 256 offsets of a cell in list order, added to every active cell's corner, then clipped to the frame."""
    t = np.arange(CELL * CELL)
    patch, inside = t // (PATCH * PATCH), t % (PATCH * PATCH)
    dx = np.array([p[0] for p in PATCH_ORDER])[patch] + inside % PATCH
    dy = np.array([p[1] for p in PATCH_ORDER])[patch] + inside // PATCH
    cells_y, cells_x = active.shape
    cells = np.flatnonzero(np.asarray(active).ravel())
    x = (cells % cells_x)[:, None] * CELL + dx[None, :]
    y = (cells // cells_x)[:, None] * CELL + dy[None, :]
    keep = (x < width) & (y < height)
    return (x[keep] + y[keep] * width).astype(np.uint32)   # (boolean indexing walks row-major: cell by cell, t ascending)


def accumulate_list(frames, accumulator, moments, pixels, width, sample_counts):
    """The list accumulate launch. frames (S, height, pitch, 4), accumulator and moments (height, pitch, 4) float32; pixels: the list. Every listed pixel folds all S
    samples in order with n = w + 1, w + 2, ... (w its moments' fourth channel); the submissions' boundaries (sample_counts) do not enter. Returns (frames,
    accumulator, moments, written, final): the frames with the listed pixels cleared, `written` the (height, pitch) mask of listed pixels, `final` the final-image
    values (NaN guard applied) to be looked at under `written` only."""
    assert frames.shape[0] == int(np.sum(sample_counts))
    height, pitch = accumulator.shape[:2]
    pixels = np.asarray(pixels, np.int64)
    written = np.zeros((height, pitch), bool)
    written[pixels // width, pixels % width] = True
    assert written.sum() == len(pixels), "a pixel is listed twice"
    acc, m2 = accumulator.astype(F).copy(), moments.astype(F).copy()
    start = m2[..., 3].copy()
    for w in np.unique(start[written]):                        # pixels that share a count share the scalar n of noise_reference.fold
        at = written & (start == w)
        a, m = acc[at], m2[at]
        for s in range(frames.shape[0]):
            a, m = noise.fold(a, m, frames[s][at].astype(F), F(F(w) + F(1)) + F(s))
        acc[at], m2[at] = a, m
    with np.errstate(all="ignore"):
        bad = ~np.isfinite((acc[..., 0] + acc[..., 1]) + acc[..., 2])
    final = acc.copy()
    final[bad] = np.array([1000, 0, 1000, 1], F)
    cleared = frames.copy()
    cleared[:, written] = 0
    return cleared, acc, m2, written, final
