"""The inputs of the adaptive-sampling tests: probe frames and, per frame, mean and moments images whose per-pixel errors are exact binary fractions, so that a
threshold can sit exactly on a cell's mean."""
import numpy as np

F = np.float32
CELL = 16
# width, height, pitch = round_up(width, 32). 40 x 24: 3 x 2 cells clipped in both directions, the corner cell 8 x 8, a padded pitch.
FRAMES = {"40x24": (40, 24, 64), "16x16": (16, 16, 32), "17x1": (17, 1, 32), "1x1": (1, 1, 32), "130x70": (130, 70, 160)}
FLOOR = 2.0          # above every luminance used here: e_p = sqrtf(v / (w * (w - 1))) / 2
SELECTION_CASES = ("on_threshold", "threshold_one_ulp_below", "just_above", "every_cell_hot", "nonfinite_cell", "unsampled_pixels", "hot_corner_dilate_0", "hot_corner_dilate_1", "threshold_0")


def images(frame, error=0.5):
    """mean (1, 1, 1) and moments with w = 2 and M2 = (8 * error^2, 0, 0): e_p = sqrt(8 e^2 / 2) / 2 = error exactly. The padding columns hold pixels that would
    count as non-finite if they were read."""
    width, height, pitch = FRAMES[frame]
    mean = np.ones((height, pitch, 4), F)
    moments = np.zeros((height, pitch, 4), F)
    moments[..., 0] = 8 * error * error; moments[..., 3] = 2
    mean[:, width:] = np.nan; moments[:, width:] = np.array([1, 1, 1, 5], F)
    return mean, moments


def cell_slices(frame, cell):
    width, height, pitch = FRAMES[frame]
    cells_x = (width + CELL - 1) // CELL
    cx, cy = cell % cells_x, cell // cells_x
    return slice(cy * CELL, min((cy + 1) * CELL, height)), slice(cx * CELL, min((cx + 1) * CELL, width))


def cell_count(frame):
    width, height, pitch = FRAMES[frame]
    return ((width + CELL - 1) // CELL) * ((height + CELL - 1) // CELL)


def selection_case(frame, name):
    """(mean, moments, threshold, dilate) of one case; every pixel's error is 0.5 unless the case says otherwise."""
    mean, moments = images(frame)
    last = cell_count(frame) - 1
    threshold, dilate = 0.5, 0
    if name == "on_threshold":            # sum == threshold * count in every cell: nothing is hot, the list is empty
        pass
    elif name == "threshold_one_ulp_below":   # the float32 below 0.5: threshold * count (exact in double) lies one float32 ulp per pixel below the sums, every cell is hot
        threshold = float(np.nextafter(F(0.5), F(0)))
    elif name == "just_above":            # one pixel of the last cell a little noisier (a few float32 ulps): that cell's sum alone lies above threshold * count
        ys, xs = cell_slices(frame, last)
        moments[ys.start, xs.start, 0] = F(2.000001)
    elif name == "every_cell_hot":
        threshold = 0.25
    elif name == "nonfinite_cell":        # cell 0 holds non-finite pixels only: not hot, whatever the threshold; the others are
        ys, xs = cell_slices(frame, 0)
        mean[ys, xs, 1] = np.nan
        threshold = 0.25
    elif name == "unsampled_pixels":      # the last cell has a pixel with w = 1 and one with w = 0: hot without a sum above the threshold
        ys, xs = cell_slices(frame, last)
        moments[ys.start, xs.start] = np.array([0, 0, 0, 1], F)
        moments[ys.stop - 1, xs.stop - 1] = 0
    elif name.startswith("hot_corner_dilate_"):   # cell 0 alone is hot; with dilate = 1 its neighbours inside the grid are active too
        ys, xs = cell_slices(frame, 0)
        moments[ys, xs, 0] = 8.0          # e_p = 1
        dilate = int(name[-1])
    elif name == "threshold_0":           # every cell with a positive sum is hot; the first cell's pixels have no noise at all
        ys, xs = cell_slices(frame, 0)
        moments[ys, xs, 0] = 0
        threshold = 0.0
    else:
        raise KeyError(name)
    return mean, moments, threshold, dilate


def brute_force_list(active, width, height):
    """The list order written out a second time, as plain loops."""
    out = []
    cells_y, cells_x = active.shape
    for cell in range(cells_x * cells_y):
        if not active[cell // cells_x, cell % cells_x]:
            continue
        x0, y0 = (cell % cells_x) * CELL, (cell // cells_x) * CELL
        for px, py in ((0, 0), (8, 0), (0, 8), (8, 8)):
            for row in range(8):
                for column in range(8):
                    x, y = x0 + px + column, y0 + py + row
                    if x < width and y < height:
                        out.append(x + y * width)
    return np.array(out, np.uint32)
