"""What a tangent-space normal map on every material costs: the benchmark's scene, camera, size and bounce count (bench.py), a
normal map generated from a seed attached to every material, and the shade stage (the four material launches, rt_get_launch_timings)
and the whole step (4 samples per pixel, wall clock) in milliseconds per step, mapped and unmapped runs alternating on one context.

    python tools/normal_map_cost.py [--seed 7] [--size 1024] [--rounds 4] [--steps 16] [--out profiles/normal_map_cost.txt]
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_raytracer_amd as grt   # noqa: E402
import normal_map_reference as ref   # noqa: E402

W, H, NUM_BOUNCES, SPP = 1920, 1080, 10, 4   # bench.py
MATERIAL_KINDS = ("material_diffuse", "material_plastic", "material_dielectric", "material_conductor")


def open_bench_scene(map_file):
    """bench.py's scene (open_scene): Sponza, every other diffuse material rough plastic; plus the map as a texture."""
    grt.config_reset()
    scene = grt.Scene(grt.scene_path("sponza_reference_maps" if grt.reference_sponza_textures_installed() else "sponza"))
    for i in range(1, scene.material_count, 2):
        if scene.material_type(i) == grt.MATERIAL_DIFFUSE:
            scene.set_material(i, grt.MATERIAL_PLASTIC, None, 0.3)
    grt.config_set(num_bounces=NUM_BOUNCES)
    texture = scene.add_texture(map_file, normal_map=True)
    return scene, texture


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024, help="side of the generated map")
    ap.add_argument("--rounds", type=int, default=4, help="mapped / unmapped pairs")
    ap.add_argument("--steps", type=int, default=16, help="steps per run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        map_file = os.path.join(tmp, "normal_map.tga")
        ref.write_tga(map_file, ref.random_normal_map(args.seed, args.size, args.size))
        scene, texture = open_bench_scene(map_file)
        pt = grt.Pathtracer(scene, W, H, device=0)   # (loads the map)
    lib, ctx = grt.device_lib(), pt.ctx
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]

    def attach(mapped):
        for i in range(scene.material_count):
            scene.set_material_normal_map(i, texture if mapped else -1)
        pt.invalidate("materials")
        pt.update()

    def steps(n):
        for s in range(n):
            if lib.rt_render_samples(ctx, 0, SPP) != 0:
                raise RuntimeError(lib.rt_last_error(ctx).decode())
        lib.rt_synchronize(ctx)

    rows = {True: [], False: []}
    for r in range(args.rounds):
        for mapped in (True, False) if r % 2 == 0 else (False, True):
            attach(mapped)
            steps(4)   # warm-up
            grt.set_profiling(ctx, 0)
            t0 = time.perf_counter()
            steps(args.steps)
            step_ms = (time.perf_counter() - t0) / args.steps * 1e3
            grt.set_profiling(ctx, 3)
            for kind in MATERIAL_KINDS:
                grt.launch_timings(ctx, kind)   # (drop what the warm-up left)
            steps(args.steps)
            shade_ms = sum(float(grt.launch_timings(ctx, kind).sum()) for kind in MATERIAL_KINDS) / args.steps
            grt.set_profiling(ctx, 0)
            rows[mapped].append((step_ms, shade_ms))
    pt.close(); scene.close()

    lines = ["normal_map_cost: Sponza %dx%d, %d bounces, %d spp per step, a %dx%d generated map (seed %d) on every material; "
             "%d rounds of %d steps, mapped and unmapped alternating" % (W, H, NUM_BOUNCES, SPP, args.size, args.size, args.seed, args.rounds, args.steps),
             "%-9s %s" % ("mapped", "  ".join("step %6.3f shade %6.3f" % row for row in rows[True])),
             "%-9s %s" % ("unmapped", "  ".join("step %6.3f shade %6.3f" % row for row in rows[False]))]
    m, u = np.median(np.array(rows[True]), axis=0), np.median(np.array(rows[False]), axis=0)
    lines.append("median ms per step: step %.3f -> %.3f (%+.1f %%), shade stage %.3f -> %.3f (%+.1f %%)"
                 % (u[0], m[0], 100 * (m[0] / u[0] - 1), u[1], m[1], 100 * (m[1] / u[1] - 1)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
