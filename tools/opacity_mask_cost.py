"""What alpha-tested opacity masks cost: the benchmark's scene, camera, size and bounce count (bench.py) loaded with
alpha_masks = 1, and the traversal stage (the merged wavefront's trace launches, rt_get_launch_timings) and the whole step (4 samples
per pixel, wall clock) in milliseconds per step, with the masks uploaded and cleared in alternating pairs on one context. Cleared,
the context launches the plain kernels; the scene, its tree and its textures are the same in both.

    python tools/opacity_mask_cost.py [--rounds 4] [--steps 16] [--out profiles/opacity_mask_cost.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_raytracer_amd as grt   # noqa: E402

W, H, NUM_BOUNCES, SPP = 1920, 1080, 10, 4   # bench.py
KERNEL_NAMES = {0: "general", 1: "flat", 2: "flat skipping", 3: "counting", 4: "general, masked", 5: "flat, masked", 6: "flat skipping, masked", 7: "counting, masked"}


def open_bench_scene():
    """bench.py's scene (open_scene): Sponza, every other diffuse material rough plastic; loaded with alpha_masks = 1."""
    grt.config_reset()
    grt.config_set(alpha_masks=1)
    scene = grt.Scene(grt.scene_path("sponza_reference_maps" if grt.reference_sponza_textures_installed() else "sponza"))
    for i in range(1, scene.material_count, 2):
        if scene.material_type(i) == grt.MATERIAL_DIFFUSE:
            scene.set_material(i, grt.MATERIAL_PLASTIC, None, 0.3)
    grt.config_set(num_bounces=NUM_BOUNCES, alpha_masks=1)
    return scene


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=4, help="masked / unmasked pairs")
    ap.add_argument("--steps", type=int, default=16, help="steps per run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    scene = open_bench_scene()
    pt = grt.Pathtracer(scene, W, H, device=0)
    lib, ctx = grt.device_lib(), pt.ctx
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    material_count = scene.material_count
    masked_materials = [i for i in range(material_count) if scene.material_opacity_map(i) is not None]

    def attach(masked):
        pt.invalidate("materials")
        pt.update()                                               # (uploads the scene's masks)
        if not masked and grt.upload_material_opacity(ctx, None, None, None) != 0:
            raise RuntimeError(lib.rt_last_error(ctx).decode())
        empty = np.zeros((3, 0), np.float32)
        return int(grt.trace_stream_rays(ctx, 0, empty, empty, np.zeros((0, 4), np.uint32), empty, empty, np.zeros(0, np.float32))[3][0])

    def steps(n):
        for s in range(n):
            if lib.rt_render_samples(ctx, 0, SPP) != 0:
                raise RuntimeError(lib.rt_last_error(ctx).decode())
        lib.rt_synchronize(ctx)

    rows = {True: [], False: []}
    kernels = {}
    for r in range(args.rounds):
        for masked in (True, False) if r % 2 == 0 else (False, True):
            kernels[masked] = attach(masked)
            steps(4)   # warm-up
            grt.set_profiling(ctx, 0)
            t0 = time.perf_counter()
            steps(args.steps)
            step_ms = (time.perf_counter() - t0) / args.steps * 1e3
            grt.set_profiling(ctx, 2)
            grt.launch_timings(ctx, "trace")   # (drop what the warm-up left)
            steps(args.steps)
            trace_ms = float(grt.launch_timings(ctx, "trace").sum()) / args.steps
            grt.set_profiling(ctx, 0)
            rows[masked].append((step_ms, trace_ms))
    pt.close(); scene.close()

    lines = ["opacity_mask_cost: Sponza %dx%d, %d bounces, %d spp per step, alpha_masks = 1 (%d of %d materials masked); %d rounds of %d steps, "
             "masks uploaded and cleared alternating; traversal kernel: %s / %s" % (W, H, NUM_BOUNCES, SPP, len(masked_materials), material_count, args.rounds, args.steps,
                                                                              KERNEL_NAMES.get(kernels[True], kernels[True]), KERNEL_NAMES.get(kernels[False], kernels[False])),
             "%-9s %s" % ("masked", "  ".join("step %6.3f traversal %6.3f" % row for row in rows[True])),
             "%-9s %s" % ("unmasked", "  ".join("step %6.3f traversal %6.3f" % row for row in rows[False]))]
    m, u = np.median(np.array(rows[True]), axis=0), np.median(np.array(rows[False]), axis=0)
    lines.append("median ms per step: step %.3f -> %.3f (%+.1f %%), traversal stage %.3f -> %.3f (%+.1f %%)"
                 % (u[0], m[0], 100 * (m[0] / u[0] - 1), u[1], m[1], 100 * (m[1] / u[1] - 1)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
