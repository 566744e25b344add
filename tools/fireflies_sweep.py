#!/usr/bin/env python3
"""The firefly filter's parameters, one at a time: relative RMS error of the mean, the resolved image and the resolved image through the denoiser
against a 2 048-sample plain render, at 16 and 64 samples, on the firefly scene of tests/scenes.py (rough dielectric with a medium under two small emitters) and on the
benchmark's Sponza at 480 x 270 with sky sampling off and on. The sampler has no seed: the run-to-run spread of a mean of N samples is measured between two DISJOINT
sample sets of one progression -- samples 1 .. N - 1 (what the frame holds after N samples; sample 1 overwrites sample 0) and samples N .. 2N - 1, recovered as
((2N - 1) M_2N - (N - 1) M_N) / N -- "seed A" and "seed B" below. Prints a table and one JSON line.

    python tools/fireflies_sweep.py [--scenes firefly,sponza,sponza_sky] [--reference 2048] [--size 256]
"""
import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEFAULT = {"tiers": 6, "start": 1.0, "support": 4.0}
ROWS = [dict(DEFAULT)] + [dict(DEFAULT, tiers=k) for k in (3, 4, 8)] + [dict(DEFAULT, start=b) for b in (0.015625, 0.0625, 0.25, 4.0)] + [dict(DEFAULT, support=s) for s in (2.0, 8.0)]


def relative_rms(image, truth):
    truth = np.asarray(truth, np.float64)
    return float(np.sqrt(np.mean((np.asarray(image, np.float64) - truth) ** 2) / np.mean(truth ** 2)))


def render_to(pt, samples, restart=True):
    if restart:
        pt.invalidate("gpu_config")
        pt.update(); pt.render()
    while pt.sample_index + 1 < samples:
        pt.update(); pt.render_samples(min(8, samples - pt.sample_index))
    return pt.read_framebuffer()[:, :pt.width, :3].astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="firefly,sponza,sponza_sky")
    ap.add_argument("--reference", type=int, default=2048)
    ap.add_argument("--size", type=int, default=256, help="the firefly scene's width and height")
    args = ap.parse_args()
    import gpu_raytracer_amd as grt
    report = []
    for name in args.scenes.split(","):
        if name == "firefly":
            from scenes import write_scene_with_everything
            from test_loaders import _png_bytes
            grt.config_reset()
            tmp = tempfile.TemporaryDirectory()
            scene = grt.Scene(write_scene_with_everything(Path(tmp.name), _png_bytes)); scene.set_sky_scale(0.3)
            width = height = args.size
            grt.config_set(num_bounces=6)
        else:
            import bench
            scene = bench.build_scene(grt)
            width, height = 480, 270
            grt.config_set(sky_sampling=0.5 if name == "sponza_sky" else 0.0)
        grt.config_set(firefly_filter=1, denoise=1)
        pt = grt.Pathtracer(scene, width, height, device=0)
        truth = render_to(pt, args.reference)
        print("%s, %d x %d, against %d samples" % (name, width, height, args.reference))
        print("  %-34s %8s %8s %8s %8s %10s %10s" % ("tiers / start / support", "samples", "mean", "resolved", "ratio", "res+den", "mean+den"))
        for samples in (16, 64):
            mean_a = render_to(pt, samples)
            mean_2n = render_to(pt, 2 * samples, restart=False)
            mean_b = ((2 * samples - 1) * mean_2n - (samples - 1) * mean_a) / samples
            err_a, err_b = relative_rms(mean_a, truth), relative_rms(mean_b, truth)
            print("  spread of the mean at %d samples: seed A %.4f, seed B %.4f, |A - B| = %.4f" % (samples, err_a, err_b, abs(err_a - err_b)))
            report.append({"scene": name, "samples": samples, "mean_seed_a": err_a, "mean_seed_b": err_b})
            for row in ROWS:
                grt.config_set(firefly_tiers=row["tiers"], firefly_start=row["start"], firefly_support=row["support"])
                mean = render_to(pt, samples)
                resolved, held = pt.resolve_fireflies()
                grt.set_denoise_source(pt.ctx, "resolved")
                resolved_denoised = pt.denoise()[0]
                grt.set_denoise_source(pt.ctx, "mean")
                mean_denoised = pt.denoise()[0]
                e = [relative_rms(x, truth) for x in (mean, resolved, resolved_denoised, mean_denoised)]
                share = float(np.maximum(held, 0).sum() / max(1e-30, (mean @ np.array([0.299, 0.587, 0.114])).sum()))
                print("  %-34s %8d %8.4f %8.4f %8.3f %10.4f %10.4f   held back %.3f %%" % ("%d / %g / %g" % (row["tiers"], row["start"], row["support"]), samples, e[0], e[1], e[0] / e[1], e[2], e[3], 100 * share))
                report.append(dict(row, scene=name, samples=samples, mean=e[0], resolved=e[1], resolved_denoised=e[2], mean_denoised=e[3], held_back_share=share))
        pt.close(); scene.close(); grt.config_reset()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
