"""The first stage of the wavefront restated: which (pixel, sample) every queue entry of a generate launch holds, and that entry's ray in float64.
numpy only; reads nothing of the product. The layout follows the comments above kernel_generate_stream (kernels_generate.hip) and rt_map_pixel
(rt_types.h), the ray follows camera_generate_ray (rt_camera.h; CUDA/Camera.h:20-62 of the reference)."""
import numpy as np

SAMPLE_SLOTS = 512                 # RT_STREAM_SAMPLE_SLOTS
MAX_BATCH_SAMPLES = 16             # RT_MAX_BATCH_SAMPLES
PMJ_SAMPLES = 4096                 # RT_PMJ_NUM_SAMPLES_PER_SEQUENCE: beyond it random_sample falls back to a hash
BLUE_NOISE_DIM = 128               # RT_BLUE_NOISE_TEXTURE_DIM
DIM_FILTER, DIM_APERTURE = 0, 1
FILTER_BOX, FILTER_TENT, FILTER_GAUSSIAN = 0, 1, 2
KERNEL_GENERATE, KERNEL_STREAM, KERNEL_STREAM_LIST = 0, 1, 2
TAA_JITTER = np.array([[0.3, 0.7, 0.2, 0.8], [0.2, 0.8, 0.7, 0.3]], np.float32)   # the four-entry table, as the float32 values the kernels hold
NOISE_CELL = 16                    # the cells of a pixel list (kernels_post.hip: four 8 x 8 patches each)


def pitch_of(width):
    """A frame's rows start every 32 pixels."""
    return (width + 31) // 32 * 32


# ---- the queue layout ----------------------------------------------------------------------------------------------

def tile_count(width, height, tile_pixels, tile_first, tile_stride):
    """The local pixels of a rank whose tiles are tile_first, tile_first + tile_stride, ... of tile_pixels each; the frame's last tile may be
    clipped (resolve_pixel_range)."""
    frame = width * height
    tiles_total = (frame + tile_pixels - 1) // tile_pixels
    owned = (tiles_total - tile_first + tile_stride - 1) // tile_stride if tile_first < tiles_total else 0
    count = owned * tile_pixels
    if owned > 0 and tile_first + (owned - 1) * tile_stride == tiles_total - 1:
        count -= tiles_total * tile_pixels - frame
    return count


def map_pixel(local, tiles):
    """rt_map_pixel: local pixel -> scan-line index of the frame. tiles = (tile_pixels, tile_first, tile_stride), tile_pixels 0 for none."""
    local = np.asarray(local, np.int64)
    tile_pixels, tile_first, tile_stride = tiles
    if tile_pixels == 0:
        return local
    return ((local // tile_pixels) * tile_stride + tile_first) * tile_pixels + local % tile_pixels


def band_walk(width, height, block_width, band_rows):
    """The frame in bands of band_rows scan lines, a band in blocks of block_width columns, a block row by row; the last band may be lower and the
    last block narrower. Entry k: the scan-line index (x + y * width) of the k-th pixel of the walk. A band holds the same scan-line indices as walk
    positions, so a submission made of whole bands visits its own pixels."""
    out = []
    for y0 in range(0, height, band_rows):
        for x0 in range(0, width, block_width):
            for y in range(y0, min(y0 + band_rows, height)):
                for x in range(x0, min(x0 + block_width, width)):
                    out.append(x + y * width)
    return np.array(out, np.int64)


def cell_list(width, height, cells):
    """The pixel list of the 16 x 16 cells `cells` ((cx, cy) each), in the order the selection writes it: a cell's four 8 x 8 patches (0,0), (8,0),
    (0,8), (8,8), a patch row by row, pixels outside the frame skipped. Entries are x + y * width."""
    out = []
    for cx, cy in cells:
        for py, px in ((0, 0), (0, 8), (8, 0), (8, 8)):
            for y in range(cy * NOISE_CELL + py, cy * NOISE_CELL + py + 8):
                for x in range(cx * NOISE_CELL + px, cx * NOISE_CELL + px + 8):
                    if x < width and y < height:
                        out.append(x + y * width)
    return np.array(out, np.uint32)


def submission_pixels(width, height, pixel_offset=0, pixel_count=0, tiles=(0, 0, 0), pixel_list=None):
    """The scan-line indices a submission covers, in local order (before any band walk)."""
    if pixel_list is not None:
        return np.asarray(pixel_list, np.int64)
    return map_pixel(np.arange(pixel_count, dtype=np.int64) + pixel_offset, tiles)


def layout(kernel, width, height, order=(0, 0), first_sample=0, sample_count=1, slot_base=0, **submission):
    """The virtual pixel word of every queue entry the launch writes, in queue order (entry 0 is the first one behind what the queue held):
    sample s of the batch fills entries [s * pixels, (s + 1) * pixels); the word is slot * frame_pixels + x + y * pitch with slot = slot_base + s
    (kernel_generate: s). Returns (words uint32, scan-line index int64, sample index int64) per entry."""
    scan = submission_pixels(width, height, **submission)
    if kernel == KERNEL_STREAM and tuple(order) != (0, 0):
        scan = band_walk(width, height, *order)[scan]
    pitch = pitch_of(width)
    frame_pixels = pitch * height
    pixel = scan % width + (scan // width) * pitch
    s = np.repeat(np.arange(sample_count, dtype=np.int64), scan.size)
    slot = s + (0 if kernel == KERNEL_GENERATE else slot_base)
    words = slot * frame_pixels + np.tile(pixel, sample_count)
    assert words.size == 0 or words.max() < 1 << 30
    return words.astype(np.uint32), np.tile(scan, sample_count), first_sample + s


def scheduler_order(width, height, pixel_offset=0, pixel_count=0, tiles=(0, 0, 0), pixel_list=None):
    """What the merged wavefront launches for such a submission: patches of 8 x 8 along bands of 8 scan lines when the pixels are whole bands."""
    if pixel_list is not None:
        return (0, 0)
    whole = tiles[0] % (8 * width) == 0 if tiles[0] > 0 else (pixel_offset == 0 and pixel_count == width * height)
    return (8, 8) if whole else (0, 0)


# ---- the ray in float64 ------------------------------------------------------------------------------------------------

def normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def tent(u):
    with np.errstate(invalid="ignore"):
        return np.where(u < 0.5, np.sqrt(2.0 * u) - 1.0, 1.0 - np.sqrt(np.maximum(2.0 - 2.0 * u, 0.0)))


def jitter(u_filter, reconstruction_filter, svgf, taa_index):
    """(N, 2) offsets inside the pixel from the (N, 2) filter draws."""
    u = np.asarray(u_filter, np.float64)
    if svgf:
        return TAA_JITTER.astype(np.float64)[:, np.asarray(taa_index) & 3].T * np.ones((u.shape[0], 1))
    if reconstruction_filter == FILTER_BOX:
        return u
    if reconstruction_filter == FILTER_TENT:
        return tent(u)
    f = np.sqrt(-2.0 * np.log(u[:, 0]))
    a = 2.0 * np.pi * u[:, 1]
    return 0.5 + 0.5 * np.stack([f * np.sin(a), f * np.cos(a)], 1)


def disk(u):
    """The concentric map of (N, 2) draws; (sin, cos) of the angle, as the kernels pair them."""
    a, b = 2.0 * u[:, 0] - 1.0, 2.0 * u[:, 1] - 1.0
    first = a * a > b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, a, b)
        phi = np.where(first, 0.25 * np.pi * (b / a), 0.5 * np.pi - 0.25 * np.pi * (a / b))
    return np.stack([r * np.sin(phi), r * np.cos(phi)], 1)


class Camera:
    """The device camera's fields as float64 (their float32 values, exactly)."""
    def __init__(self, position, bottom_left_corner, x_axis, y_axis, aperture_radius, focal_distance):
        self.position, self.blc, self.xa, self.ya = (np.array([float(np.float32(c)) for c in v]) for v in (position, bottom_left_corner, x_axis, y_axis))
        self.aperture_radius, self.focal_distance = float(np.float32(aperture_radius)), float(np.float32(focal_distance))


def rays(x, y, u_filter, u_aperture, camera, reconstruction_filter, svgf, taa_index):
    """Origins and directions (N, 3) float64 of pixels (x, y) with the float32 draws u_filter, u_aperture (N, 2) and the TAA index (N,)."""
    j = jitter(u_filter, reconstruction_filter, svgf, taa_index)
    xj, yj = np.asarray(x, np.float64) + j[:, 0], np.asarray(y, np.float64) + j[:, 1]
    focal = camera.focal_distance * normalize(camera.blc + xj[:, None] * camera.xa + yj[:, None] * camera.ya)
    if camera.aperture_radius != 0.0:
        lens = camera.aperture_radius * disk(np.asarray(u_aperture, np.float64))
    else:
        lens = np.zeros((xj.size, 2))
    offset = lens[:, :1] * camera.xa + lens[:, 1:] * camera.ya
    return camera.position + offset, normalize(focal - offset)


def recovered_jitter(x, y, direction, camera):
    """The pinhole projection inverted: where the ray position + t * direction meets the image plane blc + xj * xa + yj * ya, minus the pixel."""
    d = np.asarray(direction, np.float64)
    a = np.empty((d.shape[0], 3, 3))
    a[:, :, 0], a[:, :, 1], a[:, :, 2] = camera.xa, camera.ya, -d
    solution = np.linalg.solve(a, np.broadcast_to(-camera.blc, d.shape)[:, :, None])[:, :, 0]
    return solution[:, :2] - np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], 1)


def recovery_margin(x, y, camera):
    """How far recovered_jitter may lie from the jitter of a float32 direction, in pixels. The direction's components are rounded to float32 after a
    normalisation of a handful of float32 operations: 8 units of 2^-24 of angle. An angle e moves the intersection with the image plane by
    e * |v|^2 / D, v the vector to the point and D the plane's distance; a pixel is |xa| wide."""
    n = normalize(np.cross(camera.xa, camera.ya))
    distance = abs(float((camera.blc * n).sum()))
    v = camera.blc + (np.asarray(x, np.float64)[:, None] + 1.0) * camera.xa + (np.asarray(y, np.float64)[:, None] + 1.0) * camera.ya
    return 8.0 * 2.0 ** -24 * float((v * v).sum(1).max()) / (distance * float(np.sqrt((camera.xa ** 2).sum())))


def angle(a, b):
    """The angle between (N, 3) directions, in float64 (atan2 of cross and dot: exact down to zero)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.sqrt((np.cross(a, b) ** 2).sum(-1)), (a * b).sum(-1))


def origin_ulps(a, b):
    """The largest difference of (N, 3) origins per ray, in units of the float32 ulp of the ray's largest coordinate."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    largest = np.maximum(np.abs(a).max(-1), np.abs(b).max(-1))
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(largest, 2.0 ** -126))) - 23)
    return np.abs(a - b).max(-1) / ulp
