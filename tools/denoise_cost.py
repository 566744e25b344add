#!/usr/bin/env python3
"""What rt_denoise costs: the benchmark's Sponza frame at 1920 x 1080, 5 iterations, per kernel, tiled and plain in alternating
repeats (rt_denoise_timed: a HIP event pair around every kernel), beside what the bytes predict; then the SVGF a-trous stage's per-pass time on the
same frame size and machine (set_profiling(ctx, 3) / launch_timings). Prints a report and one JSON line.

    python tools/denoise_cost.py [--repeats 9] [--samples 16] [--scene sponza|cornellbox] [--width 1920 --height 1080]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(times):
    t = np.sort(np.asarray(times, np.float64), axis=0)
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stream-gbps", type=float, default=0.0, help="the stream bandwidth to predict with; 0: measured here (rt_measure_stream_bandwidth)")
    args = ap.parse_args()
    import gpu_raytracer_amd as grt
    if args.scene == "sponza":
        import bench
        scene = bench.build_scene(grt)
    else:
        grt.config_reset()
        scene = grt.Scene(grt.scene_path(args.scene))
    grt.config_set(denoise=1, denoise_iterations=args.iterations)
    pt = grt.Pathtracer(scene, args.width, args.height, device=0)
    pt.update(); pt.render()
    while pt.sample_index + 1 < args.samples:
        pt.update(); pt.render_samples(min(4, args.samples - pt.sample_index))
    pixels = args.width * args.height
    gbps = args.stream_gbps or float(grt.measure_stream_bandwidth(pt.ctx))
    grt.denoise_timed(pt.ctx, True, iterations=args.iterations); grt.denoise_timed(pt.ctx, False, iterations=args.iterations)   # warm: allocation, code load
    runs = {True: [], False: []}
    for _ in range(args.repeats):   # alternating, so that drift of the machine reaches both forms alike
        for tiled in (True, False):
            runs[tiled].append(grt.denoise_timed(pt.ctx, tiled, iterations=args.iterations))
    # compulsory bytes per pixel: prepare reads 5 images and writes 2; a pass reads (I, v) and the guide once (32 B; the blur's and the gradient's neighbours are
    # its own taps' lines) and writes 16 B; the last pass also reads the albedo
    kernels = ["prepare"] + ["pass step %d" % (1 << k) for k in range(args.iterations)] if args.iterations else ["prepare", "finalize"]
    bytes_per_pixel = [7 * 16] + [48] * (args.iterations - 1) + [64] if args.iterations else [7 * 16, 64]
    report = {"scene": args.scene, "width": args.width, "height": args.height, "samples": args.samples, "iterations": args.iterations, "repeats": args.repeats,
              "stream_gbps": gbps, "kernels": []}
    print("rt_denoise at %d x %d, %d iterations, %d alternating repeats; stream bandwidth %.0f GB/s" % (args.width, args.height, args.iterations, args.repeats, gbps))
    print("%-14s %28s %28s %10s" % ("kernel", "tiled ms median (min .. max)", "plain ms median (min .. max)", "bytes ms"))
    tiled_ms, plain_ms = summary(runs[True]), summary(runs[False])
    for k, name in enumerate(kernels):
        predicted = bytes_per_pixel[k] * pixels / (gbps * 1e9) * 1e3
        print("%-14s %12.4f (%.4f .. %.4f) %12.4f (%.4f .. %.4f) %10.4f" % (name, tiled_ms[0][k], tiled_ms[1][k], tiled_ms[2][k], plain_ms[0][k], plain_ms[1][k], plain_ms[2][k], predicted))
        report["kernels"].append({"name": name, "tiled_ms": float(tiled_ms[0][k]), "plain_ms": float(plain_ms[0][k]), "bytes_ms": predicted})
    totals = [float(np.median([r.sum() for r in runs[t]])) for t in (True, False)]
    print("%-14s %12.4f %28.4f %27.4f" % ("sum", totals[0], totals[1], sum(bytes_per_pixel) * pixels / (gbps * 1e9) * 1e3))
    report["tiled_total_ms"], report["plain_total_ms"] = totals
    pt.close()

    # the SVGF a-trous stage on the same frame size: per-pass launch times of a few frames
    grt.config_set(denoise=0, enable_svgf=1)
    pt = grt.Pathtracer(scene, args.width, args.height, device=0)
    grt.set_profiling(pt.ctx, 3)
    for _ in range(6):
        pt.update(); pt.render()
    pt.read_framebuffer()
    atrous = grt.launch_timings(pt.ctx, "svgf_atrous")
    if len(atrous):
        print("SVGF a-trous passes on the same frame size: %d launches, median %.4f ms (min %.4f, max %.4f)" % (len(atrous), float(np.median(atrous)), float(atrous.min()), float(atrous.max())))
        report["svgf_atrous_pass_ms"] = float(np.median(atrous))
    pt.close(); scene.close(); grt.config_reset()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
