#!/usr/bin/env python3
"""The firefly filter's parameters, one at a time: relative RMS error of the mean, the resolved image and the resolved image through the denoiser
against a 2 048-sample plain render, at 16 and 64 samples, on the firefly scene of tests/scenes.py (rough dielectric with a medium under two small emitters) and on the
benchmark's Sponza at 480 x 270 with sky sampling off and on. The sampler has no seed: the run-to-run spread of a mean of N samples is measured between two DISJOINT
sample sets of one progression -- samples 1 .. N - 1 (what the frame holds after N samples; sample 1 overwrites sample 0) and samples N .. 2N - 1, recovered as
((2N - 1) M_2N - (N - 1) M_N) / N -- "seed A" and "seed B" below. Prints a table and one JSON line.

    python tools/fireflies_sweep.py [--scenes firefly,sponza,sponza_sky] [--reference 2048] [--size 256] [--auto-start]

--auto-start: instead of the parameter rows, the start taken from the frame's own exposure (config firefly_auto_start) with firefly_start_shift
-2 .. +4 on the same scenes and sample counts -- the rows the default shift is chosen by: the lowest summed relative RMS error of the resolved image among the shifts
whose resolved error is at or below the mean's in every row, or the shift that misses that by least.
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


SHIFTS = range(-2, 5)


def choose_shift(report):
    """7.10's own condition: the resolved error at or below the mean's in every row. Among the shifts that meet it the lowest summed resolved error; if none does, the
    one whose worst row misses by least."""
    total = {s: sum(r["resolved"] for r in report if r["shift"] == s) for s in SHIFTS}
    miss = {s: max(r["resolved"] - r["mean"] for r in report if r["shift"] == s) for s in SHIFTS}
    print("shift: summed resolved error, worst resolved - mean over the rows")
    for s in SHIFTS:
        print("  %-+4d %8.4f %+9.4f%s" % (s, total[s], miss[s], "" if miss[s] <= 0 else "   (above the mean's in a row)"))
    meeting = [s for s in SHIFTS if miss[s] <= 0]
    chosen = min(meeting, key=lambda s: total[s]) if meeting else min(SHIFTS, key=lambda s: miss[s])
    print("chosen shift: %+d%s" % (chosen, "" if meeting else " (no shift meets the condition in every row: the one that misses by least)"))
    return chosen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="firefly,sponza,sponza_sky")
    ap.add_argument("--reference", type=int, default=2048)
    ap.add_argument("--size", type=int, default=256, help="the firefly scene's width and height")
    ap.add_argument("--auto-start", action="store_true", help="sweep firefly_start_shift -2 .. +4 under firefly_auto_start instead of the parameter rows")
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
        grt.config_set(firefly_filter=1, denoise=0 if args.auto_start else 1)
        pt = grt.Pathtracer(scene, width, height, device=0)
        truth = render_to(pt, args.reference)
        print("%s, %d x %d, against %d samples" % (name, width, height, args.reference))
        if args.auto_start:
            print("  %-8s %8s %10s %8s %8s %8s" % ("shift", "samples", "start", "mean", "resolved", "ratio"))
            for samples in (16, 64):
                for shift in SHIFTS:
                    grt.config_set(firefly_auto_start=1, firefly_start_shift=shift)
                    mean = render_to(pt, samples)   # (the progression starts over after the pilot: the samples count from there)
                    assert pt.firefly_start_measured
                    resolved, held = pt.resolve_fireflies()
                    e = [relative_rms(x, truth) for x in (mean, resolved)]
                    print("  %-+8d %8d %10g %8.4f %8.4f %8.3f" % (shift, samples, pt.firefly_start, e[0], e[1], e[0] / e[1]))
                    report.append({"scene": name, "samples": samples, "shift": shift, "start": pt.firefly_start, "mean": e[0], "resolved": e[1]})
            pt.close(); scene.close(); grt.config_reset()
            continue
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
    if args.auto_start:
        choose_shift(report)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
