"""Inputs of the denoiser's tests, shared by test_denoise.py (no GPU) and test_gpu_denoise.py. Every image is (height, pitch, 4) float32 and
seeded: the same bits on every machine.

What the cases guarantee (test_denoise.py relies on it):
  * every surface pixel has v > 0 by a margin: the relative standard error of a sample is SIGMA_REL = 0.8 and w <= 255, so sqrt(v) >= 0.05 x the demodulated
    luminance -- |l_p - l_q| * denom, the condition number of the luminance exponent, stays below ~25 instead of reaching 1e4 (denom's 1e-8 floor);
  * |N|^2 is 1, 0.36, 0.16 or 0 -- never near the 0.25 that decides what a surface is --, and w is a whole number, so float32 and float64 classify alike;
  * depths are >= 2 and the camera is the origin, so z has no cancellation.
"""
import numpy as np

SENTINEL = 0x7fc0dead
SIGMA_REL = 0.8
EYE = np.zeros(3, np.float32)

# name: (width, height, pitch)
SHAPES = {"1x1": (1, 1, 32), "64x8": (64, 8, 64), "70x37": (70, 37, 72), "70x37p128": (70, 37, 128), "200x150": (200, 150, 224), "257x12": (257, 12, 288)}


def crease_truth(width, height):
    """Two planes meeting at x = width / 2 with orthogonal normals, a checkerboard albedo of 5 x 3 pixel cells, a smooth irradiance.
    -> albedo, irradiance (H, W, 3), normal, position (H, W, 3), all float64."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    left = x < width / 2
    check = ((x // 5 + y // 3) % 2).astype(bool)
    albedo = np.where(check[..., None], np.array([0.8, 0.7, 0.6]), np.array([0.2, 0.25, 0.3]))
    irradiance = (1.0 + 0.5 * np.sin(x / 9.0) * np.cos(y / 7.0))[..., None] * np.array([1.0, 0.9, 0.8]) * np.where(left, 1.0, 0.6)[..., None]
    r = np.sqrt(0.5)
    normal = np.where(left[..., None], np.array([r, 0.0, -r]), np.array([-r, 0.0, -r]))
    depth = 5.0 + 0.05 * np.abs(x - width / 2)
    position = np.stack([(x - width / 2) * 0.05, (y - height / 2) * 0.05, depth], axis=-1)
    return albedo, irradiance, normal, position


def _images(width, height, pitch, colour, m2, w, albedo, normal, position, seed):
    """(H, W, 3) float64 arrays -> the six (H, pitch, 4) float32 images, the sentinel in the padding columns, a fallback of seeded colours."""
    def image(rgb, fourth):
        out = np.full((height, pitch, 4), SENTINEL, np.uint32).view(np.float32).copy()
        out[:, :width, :3] = rgb
        out[:, :width, 3] = fourth
        return out
    rng = np.random.default_rng(seed + 977)
    fallback = image(rng.uniform(0.0, 1000.0, (height, width, 3)), 1.0)
    return {"colour": image(colour, 1.0), "moments": image(m2, w), "albedo": image(albedo, 1.0), "normal": image(normal, 0.0), "position": image(position, 0.0),
            "fallback": fallback, "eye": EYE, "width": width}


def crease(width=70, height=37, pitch=72, samples=8, seed=0):
    """The crease scene from `samples` samples per pixel, each truth x lognormal(sigma = 1, mean 1), one factor for the three channels. -> images, truth (H, W, 3)."""
    albedo, irradiance, normal, position = crease_truth(width, height)
    truth = albedo * irradiance
    rng = np.random.default_rng(seed)
    factors = np.exp(rng.normal(-0.5, 1.0, (samples, height, width)))
    mean = factors.mean(axis=0)
    m2 = ((factors - mean) ** 2).sum(axis=0)
    images = _images(width, height, pitch, truth * mean[..., None], truth ** 2 * m2[..., None], float(samples), albedo, normal, position, seed)
    return images, truth


def general(shape, seed=0, constant_w=None):
    """The crease scene with everything the filter must cope with: per-pixel w from 2 to 255 (an adaptive render's), a sky region, a foreground box two units from the
    camera (a depth discontinuity), mean normals of partly missed pixels (|N|^2 0.36: still a surface; 0.16: not), and invalid pixels: w < 2, NaN and inf in each input."""
    width, height, pitch = SHAPES[shape]
    albedo, irradiance, normal, position = crease_truth(width, height)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    w = rng.integers(2, 256, (height, width)).astype(np.float64) if constant_w is None else np.full((height, width), float(constant_w))
    box = (x >= width // 4) & (x < width // 4 + max(1, width // 6)) & (y >= height // 3) & (y < height // 3 + max(1, height // 4)) & (width > 8)
    normal = np.where(box[..., None], np.array([0.0, 0.0, -1.0]), normal)
    position = np.where(box[..., None], np.stack([(x - width / 2) * 0.02, (y - height / 2) * 0.02, np.full(x.shape, 2.0)], axis=-1), position)
    truth = albedo * irradiance
    mean = truth * np.maximum(0.05, 1.0 + SIGMA_REL / np.sqrt(w) * rng.normal(0.0, 1.0, (height, width)))[..., None]
    m2 = (truth * SIGMA_REL) ** 2 * ((w - 1.0) * rng.uniform(0.6, 1.6, (height, width)))[..., None]
    sky = (y >= height - max(1, height // 5)) & (width > 1)
    normal = np.where(sky[..., None], 0.0, normal); position = np.where(sky[..., None], 0.0, position); albedo = np.where(sky[..., None], 0.0, albedo)
    mean = np.where(sky[..., None], np.array([0.3, 0.5, 0.9]), mean)
    scale = rng.choice([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.6, 0.4], (height, width))
    normal = normal * scale[..., None]
    images = _images(width, height, pitch, mean, m2, w, albedo, normal, position, seed)
    if width * height >= 64:   # invalid pixels, one rule each, away from each other
        spots = [(name, (int(rng.integers(0, height)), int(rng.integers(0, width)))) for name in ("w1", "w0", "nan_colour", "inf_moment", "nan_albedo", "inf_normal", "nan_position", "nan_w")]
        for name, (py, px) in spots:
            if name == "w1": images["moments"][py, px, 3] = 1.0
            if name == "w0": images["moments"][py, px] = 0.0
            if name == "nan_colour": images["colour"][py, px, 1] = np.nan
            if name == "inf_moment": images["moments"][py, px, 0] = np.inf
            if name == "nan_albedo": images["albedo"][py, px, 2] = np.nan
            if name == "inf_normal": images["normal"][py, px, 0] = -np.inf
            if name == "nan_position": images["position"][py, px, 1] = np.nan
            if name == "nan_w": images["moments"][py, px, 3] = np.nan
    for image in images.values():
        if isinstance(image, np.ndarray):
            image.setflags(write=False)
    return images


def flat(width=40, height=24, pitch=64, seed=3):
    """Constant colour, normal and depth; v varies from pixel to pixel."""
    rng = np.random.default_rng(seed)
    ones = np.ones((height, width, 3))
    colour = ones * np.array([0.5, 0.25, 0.125])
    w = 16.0
    m2 = (rng.uniform(0.5, 2.0, (height, width)) * w * (w - 1.0))[..., None] * ones * 0.01
    position = ones * np.array([0.0, 0.0, 4.0])
    return _images(width, height, pitch, colour, m2, w, ones * 0.5, ones * np.array([0.0, 0.0, -1.0]), position, seed)


def relative_rms(image, truth):
    return float(np.sqrt(np.mean((np.asarray(image, np.float64) - truth) ** 2) / np.mean(truth ** 2)))
