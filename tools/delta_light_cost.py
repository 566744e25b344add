"""What the delta emitters cost on the benchmark's scene, camera, size and bounce count (bench.py): the shade stage (the four
material launches, rt_get_launch_timings) and the whole step (4 samples per pixel, wall clock) in milliseconds per step.

    python tools/delta_light_cost.py --mode sky [--package DIR]   # one run with sky sampling 0.5 (the _sky instances): one JSON line. --package names the
                                                                  # package directory of ANOTHER build (the parent commit's), so that a shell loop can
                                                                  # alternate the two builds, one process each, in one session
    python tools/delta_light_cost.py --mode plain [--package DIR] # the same without sky sampling (the plain instances)
    python tools/delta_light_cost.py --mode sun [--rounds 4] [--out profiles/...]   # with and without one directional sun (automatic share), alternating on one context
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NUM_BOUNCES, SPP = 1920, 1080, 10, 4   # bench.py
MATERIAL_KINDS = ("material_diffuse", "material_plastic", "material_dielectric", "material_conductor")


def load_package(directory):
    """The package in `directory` (a build's gpu-raytracer_amd), with this tree's assets."""
    spec = importlib.util.spec_from_file_location("gpu_raytracer_amd", os.path.join(directory, "__init__.py"), submodule_search_locations=[directory])
    module = importlib.util.module_from_spec(spec)
    sys.modules["gpu_raytracer_amd"] = module
    spec.loader.exec_module(module)
    module.ASSET_DIR = os.path.join(ROOT, "assets")
    os.environ["GRT_ASSET_DIR"] = module.ASSET_DIR
    return module


def open_bench_scene(grt, **config):
    """bench.py's scene (open_scene): Sponza, every other diffuse material rough plastic."""
    grt.config_reset()
    scene = grt.Scene(grt.scene_path("sponza_reference_maps" if grt.reference_sponza_textures_installed() else "sponza"))
    for i in range(1, scene.material_count, 2):
        if scene.material_type(i) == grt.MATERIAL_DIFFUSE:
            scene.set_material(i, grt.MATERIAL_PLASTIC, None, 0.3)
    grt.config_set(num_bounces=NUM_BOUNCES, **config)
    return scene


def measure(grt, lib, ctx, steps):
    def run(n):
        for s in range(n):
            if lib.rt_render_samples(ctx, 0, SPP) != 0:
                raise RuntimeError(lib.rt_last_error(ctx).decode())
        lib.rt_synchronize(ctx)
    run(4)   # warm-up
    grt.set_profiling(ctx, 0)
    t0 = time.perf_counter()
    run(steps)
    step_ms = (time.perf_counter() - t0) / steps * 1e3
    grt.set_profiling(ctx, 3)
    for kind in MATERIAL_KINDS:
        grt.launch_timings(ctx, kind)   # (drop what the warm-up left)
    run(steps)
    shade_ms = sum(float(grt.launch_timings(ctx, kind).sum()) for kind in MATERIAL_KINDS) / steps
    grt.set_profiling(ctx, 0)
    return step_ms, shade_ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=["sky", "plain", "sun"], required=True)
    ap.add_argument("--package", default=os.path.join(ROOT, "gpu-raytracer_amd"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    grt = load_package(os.path.abspath(args.package))
    scene = open_bench_scene(grt, **({"sky_sampling": 0.5} if args.mode == "sky" else {}))
    pt = grt.Pathtracer(scene, W, H, device=0)
    pt.update()
    lib, ctx = grt.device_lib(), pt.ctx
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    if args.mode in ("sky", "plain"):
        step_ms, shade_ms = measure(grt, lib, ctx, args.steps)
        print(json.dumps({"mode": args.mode, "package": os.path.relpath(os.path.abspath(args.package), ROOT), "step_ms": round(step_ms, 4), "shade_ms": round(shade_ms, 4)}))
        pt.close(); scene.close()
        return
    rows = {True: [], False: []}
    for r in range(args.rounds):
        for sun in (True, False) if r % 2 == 0 else (False, True):
            scene.clear_delta_lights()
            if sun:
                scene.add_directional_light((-0.3, -1.0, 0.2), (20.0, 18.0, 15.0))
            pt.invalidate("delta_lights"); pt.update()
            rows[sun].append(measure(grt, lib, ctx, args.steps))
    share = pt.delta_light_share
    pt.close(); scene.close()
    lines = ["delta_light_cost: Sponza %dx%d, %d bounces, %d spp per step, one directional sun (automatic share; the last staged share %.3f); "
             "%d rounds of %d steps, with and without the sun alternating on one context" % (W, H, NUM_BOUNCES, SPP, share, args.rounds, args.steps),
             "%-9s %s" % ("sun", "  ".join("step %6.3f shade %6.3f" % row for row in rows[True])),
             "%-9s %s" % ("no sun", "  ".join("step %6.3f shade %6.3f" % row for row in rows[False]))]
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
