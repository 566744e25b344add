"""What adaptive sampling costs and gains on the benchmark's scene, camera, size, bounce count and burst (bench.py). No pass mark.

1. Mechanism: every cell active (threshold 0, dilate 1), so the list holds the same rays in cell order instead of band order. Milliseconds per step (4 samples
   per pixel, wall clock) and the generate / traversal / accumulate stage times (rt_get_launch_timings) through the list against uniform submissions, in
   alternating pairs on one context; medians, beside the spread of the uniform runs themselves.
2. Selection: one rt_select_active_cells call on an idle context (wall clock).
3. The point of it: render_until to one noise target -- the figure a uniform pilot run has after --pilot samples -- uniformly and adaptively: wall time, total
   paths, and the share of cells active at each check (every 32 samples, the burst the command line declares).

    python tools/adaptive_sampling_cost.py [--rounds 4] [--steps 16] [--pilot 128] [--cap 1024] [--out profiles/adaptive_sampling.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from delta_light_cost import H, NUM_BOUNCES, SPP, W, open_bench_scene   # bench.py's scene and shape, stated once

STAGES = ("generate", "trace", "sort", "accumulate")


def measure(grt, lib, ctx, steps, first):
    def run(n, at):
        for s in range(n):
            if lib.rt_render_samples(ctx, at + s * SPP, SPP) != 0:
                raise RuntimeError(lib.rt_last_error(ctx).decode())
        lib.rt_synchronize(ctx)
        return at + n * SPP
    at = run(4, first)   # warm-up
    grt.set_profiling(ctx, 0)
    t0 = time.perf_counter()
    at = run(steps, at)
    step_ms = (time.perf_counter() - t0) / steps * 1e3
    grt.set_profiling(ctx, 3)
    for kind in STAGES:
        grt.launch_timings(ctx, kind)   # (drop what the warm-up left)
    at = run(steps, at)
    stages = [float(grt.launch_timings(ctx, kind).sum()) / steps for kind in STAGES]
    grt.set_profiling(ctx, 0)
    return [step_ms] + stages, at


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--pilot", type=int, default=128)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gpu_raytracer_amd as grt
    scene = open_bench_scene(grt)
    pt = grt.Pathtracer(scene, W, H, device=0)
    pt.set_noise_estimate(True)
    pt.update()
    lib, ctx = grt.device_lib(), pt.ctx
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    grt.set_frame_pipelining(ctx, True); grt.set_stream_batch(ctx, 8 * SPP * W * H)   # bench.py's declared burst
    floor = grt.config_get("noise_floor")
    lines = ["adaptive_sampling_cost: Sponza %dx%d, %d bounces, %d spp per step, burst of 8 submissions" % (W, H, NUM_BOUNCES, SPP)]

    # 1. the mechanism, every cell active
    for first in (0, 4, 8, 12):
        if lib.rt_render_samples(ctx, first, SPP) != 0:
            raise RuntimeError(lib.rt_last_error(ctx).decode())
    chosen = grt.select_active_cells(ctx, H, W, 0.0, floor=floor, dilate=1)
    lines.append("1. mechanism: threshold 0, dilate 1 after 16 uniform samples: %d of %d cells active, the list holds %d of %d pixels; %d rounds of %d steps, list and uniform alternating"
                 % (chosen["active_cells"], chosen["cells_x"] * chosen["cells_y"], chosen["list_pixels"], W * H, args.rounds, args.steps))
    rows = {True: [], False: []}
    at = 16
    for r in range(args.rounds):
        for on in (True, False) if r % 2 == 0 else (False, True):
            grt.set_pixel_list(ctx, on)
            row, at = measure(grt, lib, ctx, args.steps, at)
            rows[on].append(row)
    grt.set_pixel_list(ctx, False)
    names = ("step",) + STAGES
    for on in (True, False):
        lines.append("%-8s %s" % ("list" if on else "uniform", "   ".join(" ".join("%s %.4f" % (n, v) for n, v in zip(names, row)) for row in rows[on])))
    m, u = np.median(np.array(rows[True]), axis=0), np.median(np.array(rows[False]), axis=0)
    spread = np.array(rows[False]).max(axis=0) - np.array(rows[False]).min(axis=0)
    lines.append("median ms per step, uniform -> list (the uniform runs' own max - min): " + "; ".join(
        "%s %.4f -> %.4f (%+.1f %%, spread %.4f)" % (n, u[i], m[i], 100 * (m[i] / u[i] - 1) if u[i] else 0.0, spread[i]) for i, n in enumerate(names)))

    # 2. one selection on an idle context
    select_ms = []
    for _ in range(12):
        lib.rt_synchronize(ctx)
        t0 = time.perf_counter()
        grt.select_active_cells(ctx, H, W, 0.05, floor=floor, dilate=1)
        select_ms.append((time.perf_counter() - t0) * 1e3)
    lines.append("2. one rt_select_active_cells call on an idle context (noise kernel, selection, scan, compaction, copies of %d flags; wall clock): median %.3f ms, min %.3f ms over %d calls"
                 % (chosen["cells_x"] * chosen["cells_y"], float(np.median(select_ms)), min(select_ms), len(select_ms)))

    # 3. to one noise target, uniformly and adaptively
    def restart():
        pt.set_noise_estimate(True); pt.invalidate("gpu_config")
    restart()
    pilot = pt.render_until(0.0, args.pilot, check_every=32)
    target = float(np.float32(pilot["figure"]))
    lines.append("3. target %.6g: the figure of a uniform run after %d samples; render_until(check_every=32, cap %d), wall clock of the whole call" % (target, args.pilot, args.cap))
    for adaptive in (False, True, False, True):
        restart()
        lib.rt_synchronize(ctx)
        t0 = time.perf_counter()
        result = pt.render_until(target, args.cap, check_every=32, adaptive=adaptive)
        lib.rt_synchronize(ctx)
        seconds = time.perf_counter() - t0
        counts, mean = pt.sample_counts()
        paths = (mean + 1.0) * W * H     # w counts the samples past sample 0
        lines.append("%-8s %4d passes, figure %.6g%s, %.3f s, %.4g paths (%.2f samples per pixel on average)%s"
                     % ("adaptive" if adaptive else "uniform", result["samples"], result["figure"], " (capped)" if result["capped"] else "", seconds, paths, mean + 1.0,
                        "; active cells per check: " + " ".join("%.3f" % s for s in result["active_share"]) if adaptive else ""))
    pt.close(); scene.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
