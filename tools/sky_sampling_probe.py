"""Sky importance sampling on Sponza at 1920 x 1080 under a generated sun sky: milliseconds per sample with the option on and off,
and the MSE of each against a high-sample reference of the default estimator at equal time.

    python tools/sky_sampling_probe.py [--reference-samples 1024] [--share 0.5] [--out profiles/r07_sky_sampling.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_raytracer_amd as grt   # noqa: E402
import sky_sampling_reference as ref   # noqa: E402

W, H = 1920, 1080


def open_sponza(config, sky):
    grt.config_reset()
    grt.config_set(**config)
    scene = grt.Scene(grt.scene_path("sponza"))
    grt.config_set(**config)
    pt = grt.Pathtracer(scene, W, H, device=0)
    pt.update()
    lib = grt.device_lib()
    lib.rt_set_sky.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.rt_set_sky(pt.ctx, sky.ctypes.data, sky.shape[1], sky.shape[0], 1.0) == 0
    return scene, pt, lib


def render(pt, lib, samples, batch=8):
    """Returns (image, seconds): `samples` samples in batches, timed from the first submission to the read-back."""
    assert lib.rt_render_samples(pt.ctx, 0, 1) == 0, lib.rt_last_error(pt.ctx)   # warm-up (tables, queues)
    pt.read_framebuffer()
    t0 = time.perf_counter()
    for first in range(0, samples, batch):
        assert lib.rt_render_samples(pt.ctx, first, min(batch, samples - first)) == 0, lib.rt_last_error(pt.ctx)
    img = pt.read_framebuffer()[:, :W, :3].astype(np.float64)
    return img, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-samples", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sky = np.ascontiguousarray(ref.sun_sky(1024, 512, (300, 120), sun_value=20000.0))
    base = dict(num_bounces=5)
    lines = ["Sponza %dx%d, generated sun sky 1024 x 512 (2 x 2-texel sun of 20000 over a dim gradient), %d bounces" % (W, H, base["num_bounces"])]

    scene, pt, lib = open_sponza(base, sky)
    reference, t_ref = render(pt, lib, a.reference_samples)
    pt.close(); scene.close()
    lines.append("reference: default estimator, %d samples, %.1f s" % (a.reference_samples, t_ref))

    results = {}
    for label, share in (("off", 0.0), ("on p=%g" % a.share, a.share)):
        scene, pt, lib = open_sponza(dict(base, sky_sampling=share), sky)
        img, seconds = render(pt, lib, a.samples)
        pt.close(); scene.close()
        ms = seconds * 1e3 / a.samples
        results[label] = (ms, img)
        lines.append("%-8s %.3f ms per sample (%d samples), MSE vs reference at %d samples %.4g" % (label, ms, a.samples, a.samples, float(((img - reference) ** 2).mean())))
    (ms_off, img_off), (ms_on, img_on) = results.values()
    mse_off = float(((img_off - reference) ** 2).mean()); mse_on = float(((img_on - reference) ** 2).mean())
    # equal time: MSE falls as 1 / samples, so a per-sample cost ratio converts one into the other
    lines.append("equal time: MSE(off) / MSE(on) = %.2f (the MSE of `on` scaled by its cost per sample, %.3f / %.3f ms)" % (mse_off / (mse_on * ms_on / ms_off), ms_on, ms_off))
    lines.append("note: the reference has its own noise; its MSE against the truth is about MSE(off at %d samples) x %d / %d" % (a.samples, a.samples, a.reference_samples))
    lines.append("note: the reference renders samples 0 .. %d with the default estimator, so `off` shares its first %d samples with it: its MSE is"
                 " biased low and the equal-time ratio favours `off`" % (a.reference_samples - 1, a.samples))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    grt.config_reset()


if __name__ == "__main__":
    main()
