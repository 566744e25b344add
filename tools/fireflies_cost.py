#!/usr/bin/env python3
"""What the firefly filter costs: the benchmark's Sponza frame at 1920 x 1080. The accumulate launch with the cascade against the plain
_moments launch (set_profiling(ctx, 3) / launch_timings, alternating renders), and the resolve kernel, tiled and plain in alternating repeats
(rt_resolve_fireflies_timed: a HIP event pair around the kernel), beside what the bytes predict. Prints a report and one JSON line.

    python tools/fireflies_cost.py [--repeats 9] [--samples 16] [--tiers 6] [--scene sponza|cornellbox] [--width 1920 --height 1080]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--tiers", type=int, default=6)
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
    pixels = args.width * args.height
    report = {"scene": args.scene, "width": args.width, "height": args.height, "samples": args.samples, "tiers": args.tiers, "repeats": args.repeats}

    def render(pt):
        pt.invalidate("gpu_config")
        pt.update(); pt.render()
        while pt.sample_index + 1 < args.samples:
            pt.update(); pt.render_samples(min(4, args.samples - pt.sample_index))
        pt.read_framebuffer()

    # the accumulate launches of a render of `samples` samples in submissions of 4, cascade on and off in alternating renders (the estimate on in both)
    grt.config_set(noise_target=1e-30, firefly_tiers=args.tiers)
    pt = grt.Pathtracer(scene, args.width, args.height, device=0)
    grt.set_profiling(pt.ctx, 3)
    launches = {0: [], 1: []}
    for repeat in range(args.repeats + 1):
        for on in (0, 1):
            grt.config_set(firefly_filter=on)
            render(pt)
            times = grt.launch_timings(pt.ctx, "accumulate")
            if repeat:   # (the first pair warms up: allocation, code load)
                launches[on].append(float(np.sum(times)))
    report["accumulate_ms_per_render"] = {"moments": float(np.median(launches[0])), "cascade": float(np.median(launches[1]))}
    print("accumulate launches of a %d-sample render at %d x %d, median of %d alternating renders: _moments %.4f ms, cascade (%d tiers) %.4f ms (%.2f x)"
          % (args.samples, args.width, args.height, args.repeats, report["accumulate_ms_per_render"]["moments"], args.tiers, report["accumulate_ms_per_render"]["cascade"],
             report["accumulate_ms_per_render"]["cascade"] / report["accumulate_ms_per_render"]["moments"]))
    grt.set_profiling(pt.ctx, 0)

    gbps = float(grt.measure_stream_bandwidth(pt.ctx))
    grt.resolve_fireflies_timed(pt.ctx, tiled=True); grt.resolve_fireflies_timed(pt.ctx, tiled=False)   # warm
    runs = {True: [], False: []}
    for _ in range(args.repeats):
        for tiled in (True, False):
            runs[tiled].append(grt.resolve_fireflies_timed(pt.ctx, tiled=tiled))
    bytes_per_pixel = 16 * (args.tiers + 4)   # mean, moments, K tiers read, the result written (the fallback is read for invalid pixels only)
    predicted = bytes_per_pixel * pixels / (gbps * 1e9) * 1e3
    tiled_ms, plain_ms = float(np.median(runs[True])), float(np.median(runs[False]))
    print("resolve, %d tiers: tiled %.4f ms (%.4f .. %.4f), plain %.4f ms; the bytes (%d B per pixel at %.0f GB/s) predict %.4f ms: %.2f x"
          % (args.tiers, tiled_ms, min(runs[True]), max(runs[True]), plain_ms, bytes_per_pixel, gbps, predicted, tiled_ms / predicted))
    report.update(stream_gbps=gbps, resolve_tiled_ms=tiled_ms, resolve_plain_ms=plain_ms, resolve_bytes_ms=predicted)

    # What the rest is: the tiled resolve over the tier count (fresh, zeroed tiers: w >= 1 and zeros are valid pixels, and the kernel's work does not depend on the values).
    # A line through the medians, ms = fixed + per_tier * K, against the bytes' 64 B + 16 B * K per pixel: the slope prices the tier loads, the intercept everything
    # that does not scale with them (launch, the mean / moments loads, the barrier, the ring's second round of loads, the write).
    by_tiers = {}
    for _ in range(args.repeats):
        for k in (2, 4, 6, 8):
            grt.set_firefly_cascade(pt.ctx, tiers=k)
            grt.resolve_fireflies_timed(pt.ctx, tiled=True)
            by_tiers.setdefault(k, []).append(grt.resolve_fireflies_timed(pt.ctx, tiled=True))
    ks = sorted(by_tiers)
    medians = [float(np.median(by_tiers[k])) for k in ks]
    per_tier, fixed = np.polyfit(ks, medians, 1)
    per_tier_bytes, fixed_bytes = 16 * pixels / (gbps * 1e9) * 1e3, 64 * pixels / (gbps * 1e9) * 1e3
    print("tiled resolve over K = %s: %s ms; fit %.4f + %.4f K ms against the bytes' %.4f + %.4f K" % (ks, ["%.4f" % m for m in medians], fixed, per_tier, fixed_bytes, per_tier_bytes))
    report.update(resolve_by_tiers=dict(zip(ks, medians)), resolve_fixed_ms=float(fixed), resolve_per_tier_ms=float(per_tier), bytes_fixed_ms=fixed_bytes, bytes_per_tier_ms=per_tier_bytes)
    pt.close(); scene.close(); grt.config_reset()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
