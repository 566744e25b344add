#!/usr/bin/env python3
"""What the exposure measurement and the firefly-robust noise estimate cost: one rt_measure_exposure, and one rt_estimate_noise_robust
against one rt_estimate_noise, at 1920 x 1080 on an idle context that holds a rendered frame -- whole calls on the host's clock (allocation, launch, wait and
read-back of the cell arrays included; no pixel map), the three in alternating repeats, in the manner of tools/fireflies_cost.py. The robust call is expected to cost
the resolve on top of the plain one (rt_resolve_fireflies_timed, printed beside it). Prints a report and one JSON line.

    python tools/robust_noise_cost.py [--repeats 9] [--samples 8] [--scene sponza|cornellbox] [--width 1920 --height 1080]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import gpu_raytracer_amd as grt
    if args.scene == "sponza":
        import bench
        scene = bench.build_scene(grt)
    else:
        grt.config_reset()
        scene = grt.Scene(grt.scene_path(args.scene))
    grt.config_set(firefly_filter=1)
    pt = grt.Pathtracer(scene, args.width, args.height, device=0)
    pt.update(); pt.render()
    while pt.sample_index + 1 < args.samples:
        pt.update(); pt.render_samples(min(4, args.samples - pt.sample_index))
    pt.read_framebuffer()
    calls = {"measure_exposure": lambda: grt.measure_exposure(pt.ctx),
             "estimate_noise": lambda: grt.estimate_noise(pt.ctx, args.height, args.width, pt.pitch, want_map=False),
             "estimate_noise_robust": lambda: grt.estimate_noise_robust(pt.ctx, args.height, args.width, pt.pitch, want_map=False)}
    times = {name: [] for name in calls}
    resolve = []
    for repeat in range(args.repeats + 1):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            if repeat:   # (the first round warms up: allocation, code load)
                times[name].append((time.perf_counter() - t0) * 1e3)
        resolve.append(grt.resolve_fireflies_timed(pt.ctx, tiled=True))
    held = grt.estimate_noise_robust(pt.ctx, args.height, args.width, pt.pitch, want_map=False)["held_pixels"]
    report = {"scene": args.scene, "width": args.width, "height": args.height, "samples": args.samples, "repeats": args.repeats, "held_pixels": held,
              "resolve_kernel_ms": float(np.median(resolve[1:]))}
    for name, values in times.items():
        report[name + "_ms"] = float(np.median(values))
        print("%-24s median of %d alternating calls %.4f ms (%.4f .. %.4f)" % (name, args.repeats, report[name + "_ms"], min(values), max(values)))
    print("robust - plain %.4f ms; the resolve kernel alone %.4f ms; %d pixels held" % (report["estimate_noise_robust_ms"] - report["estimate_noise_ms"], report["resolve_kernel_ms"], held))
    pt.close(); scene.close(); grt.config_reset()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
