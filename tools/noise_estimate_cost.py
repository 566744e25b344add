"""What the noise estimate costs on the benchmark's scene, camera, size, bounce count and burst (bench.py): the accumulate stage
(rt_get_launch_timings, kind "accumulate") and the whole step (4 samples per pixel, wall clock) in milliseconds per step, with the estimate on and
off in alternating pairs on one context, against the off runs of the same process; and the time of one rt_estimate_noise call. No pass mark.

    python tools/noise_estimate_cost.py [--rounds 4] [--steps 16] [--out profiles/noise_estimate.txt]
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


def measure(grt, lib, ctx, steps):
    def run(n):
        for s in range(n):   # sample indices advance, as in a progression: the moments need n >= 2 to do their work
            if lib.rt_render_samples(ctx, 2 + s * SPP, SPP) != 0:
                raise RuntimeError(lib.rt_last_error(ctx).decode())
        lib.rt_synchronize(ctx)
    run(4)   # warm-up
    grt.set_profiling(ctx, 0)
    t0 = time.perf_counter()
    run(steps)
    step_ms = (time.perf_counter() - t0) / steps * 1e3
    grt.set_profiling(ctx, 3)
    grt.launch_timings(ctx, "accumulate")   # (drop what the warm-up left)
    run(steps)
    accumulate_ms = float(grt.launch_timings(ctx, "accumulate").sum()) / steps
    grt.set_profiling(ctx, 0)
    return step_ms, accumulate_ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gpu_raytracer_amd as grt
    scene = open_bench_scene(grt)
    pt = grt.Pathtracer(scene, W, H, device=0)
    pt.update()
    lib, ctx = grt.device_lib(), pt.ctx
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    grt.set_frame_pipelining(ctx, True); grt.set_stream_batch(ctx, 8 * SPP * W * H)   # bench.py's declared burst
    rows = {True: [], False: []}
    estimate_ms = []
    for r in range(args.rounds):
        for on in (True, False) if r % 2 == 0 else (False, True):
            grt.set_noise_estimate(ctx, on)
            rows[on].append(measure(grt, lib, ctx, args.steps))
            if on:
                for _ in range(3):
                    t0 = time.perf_counter()
                    grt.estimate_noise(ctx, H, W, pt.pitch, want_map=False)
                    estimate_ms.append((time.perf_counter() - t0) * 1e3)
    pt.close(); scene.close()
    lines = ["noise_estimate_cost: Sponza %dx%d, %d bounces, %d spp per step, burst of 8 submissions; %d rounds of %d steps, estimate on and off alternating on one context"
             % (W, H, NUM_BOUNCES, SPP, args.rounds, args.steps),
             "%-4s %s" % ("on", "  ".join("step %6.3f accumulate %6.4f" % row for row in rows[True])),
             "%-4s %s" % ("off", "  ".join("step %6.3f accumulate %6.4f" % row for row in rows[False]))]
    m, u = np.median(np.array(rows[True]), axis=0), np.median(np.array(rows[False]), axis=0)
    lines.append("median ms per step: step %.3f -> %.3f (%+.1f %%), accumulate stage %.4f -> %.4f (%+.1f %%)"
                 % (u[0], m[0], 100 * (m[0] / u[0] - 1), u[1], m[1], 100 * (m[1] / u[1] - 1)))
    lines.append("one rt_estimate_noise call on an idle context (kernel, copies of %d cells, wall clock): median %.3f ms, min %.3f ms over %d calls"
                 % (((W + 15) // 16) * ((H + 15) // 16), float(np.median(estimate_ms)), min(estimate_ms), len(estimate_ms)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
