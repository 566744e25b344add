"""What the light tree costs and buys, on one GPU:

  build    rt_set_light_tree(ctx, 1) on bare contexts of 10^3, 10^4, 10^5 and 10^6 random emissive triangles: milliseconds of the whole call on the host's clock
           (allocation, the launches, the wait), median of 5 off / on pairs
  stages   the many-light world of the tests at a larger size (32 x 32 lamps, 1280 x 720, 4 bounces, 4 samples per step): sort and shade stage and the whole step
           with the tree on against off, on one context in alternating pairs
  noise    the same world: the noise figure (rt_estimate_noise, the mean of the cells) at equal samples, and with the tree's sample count scaled to equal time

    python tools/light_tree_cost.py [--rounds 4] [--steps 12] [--samples 64] [--out profiles/light_tree.txt]
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, NUM_BOUNCES, SPP, GRID = 1280, 720, 4, 4, 32
STAGES = {"sort": ("sort",), "shade": ("material_diffuse", "material_plastic", "material_dielectric", "material_conductor")}


def build_times(grt, cases, ref, lines):
    lib = grt.device_lib()
    for n in (1000, 10000, 100000, 1000000):
        rng = np.random.default_rng(n)
        tri = cases._triangles(rng.uniform(-50, 50, (n, 3)), rng.normal(0, 0.3, (n, 3)), rng.normal(0, 0.3, (n, 3)))
        s = cases._scene({"datas": [tri], "use": [0]}, [(5, 5, 5)], [cases._matrix()])
        ctx, _ = cases.upload(grt, s)
        times = []
        for _ in range(5):
            assert grt.set_light_tree(ctx, False) == 0
            t0 = time.perf_counter()
            assert grt.set_light_tree(ctx, True) == 0, lib.rt_last_error(ctx)
            times.append((time.perf_counter() - t0) * 1e3)
        tree = grt.read_light_tree(ctx)
        lines.append("build   N %8d  M %8d  rt_set_light_tree(1): median %.3f ms (min %.3f, max %.3f)" % (tree.leaf_count, tree.padded, np.median(times), min(times), max(times)))
        lib.rt_destroy(ctx)


def measure(grt, lib, ctx, steps):
    def run(n):
        for _ in range(n):
            if lib.rt_render_samples(ctx, 0, SPP) != 0:
                raise RuntimeError(lib.rt_last_error(ctx).decode())
        lib.rt_synchronize(ctx)
    run(3)
    grt.set_profiling(ctx, 0)
    t0 = time.perf_counter()
    run(steps)
    step_ms = (time.perf_counter() - t0) / steps * 1e3
    grt.set_profiling(ctx, 3)
    for kinds in STAGES.values():
        for kind in kinds:
            grt.launch_timings(ctx, kind)
    run(steps)
    stage = {name: sum(float(grt.launch_timings(ctx, kind).sum()) for kind in kinds) / steps for name, kinds in STAGES.items()}
    grt.set_profiling(ctx, 0)
    return step_ms, stage["sort"], stage["shade"]


def noise_at(grt, lib, pt, samples):
    grt.set_noise_estimate(pt.ctx, False); grt.set_noise_estimate(pt.ctx, True)   # (the moments start over)
    t0 = time.perf_counter()
    for s in range(0, samples + 1, 16):
        assert lib.rt_render_samples(pt.ctx, s, min(16, samples + 1 - s)) == 0, lib.rt_last_error(pt.ctx)
    lib.rt_synchronize(pt.ctx)
    seconds = time.perf_counter() - t0
    return grt.estimate_noise(pt.ctx, H, W, pt.pitch, want_map=False)["mean"], seconds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gpu_raytracer_amd as grt
    import light_tree_cases as cases
    import light_tree_reference as ref
    lib = grt.device_lib()
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lines = ["light_tree_cost: build on bare contexts; stages and noise on the many-light world, %d x %d lamps, %d x %d, %d bounces, %d spp per step" % (GRID, GRID, W, H, NUM_BOUNCES, SPP)]
    build_times(grt, cases, ref, lines)

    path = cases.write_many_lights(tempfile.mkdtemp(), grid=GRID, floor_half=80.0)
    grt.config_reset(); grt.config_set(num_bounces=NUM_BOUNCES)
    scene = grt.Scene(path); grt.config_set(num_bounces=NUM_BOUNCES)
    pt = grt.Pathtracer(scene, W, H, device=0); pt.update()
    ctx = pt.ctx
    rows = {True: [], False: []}
    for r in range(args.rounds):
        for tree in (True, False) if r % 2 == 0 else (False, True):
            assert grt.set_light_tree(ctx, tree) == 0, lib.rt_last_error(ctx)
            rows[tree].append(measure(grt, lib, ctx, args.steps))
    for tree in (False, True):
        lines.append("%-8s %s" % ("tree on" if tree else "tree off", "  ".join("step %6.3f sort %6.3f shade %6.3f" % row for row in rows[tree])))
    on, off = np.median(np.array(rows[True]), axis=0), np.median(np.array(rows[False]), axis=0)
    lines.append("median ms per step, off -> on: step %.3f -> %.3f (%+.1f %%), sort stage %.3f -> %.3f (%+.1f %%), shade stage %.3f -> %.3f (%+.1f %%); leaves %d"
                 % (off[0], on[0], 100 * (on[0] / off[0] - 1), off[1], on[1], 100 * (on[1] / off[1] - 1), off[2], on[2], 100 * (on[2] / off[2] - 1), grt.read_light_tree(ctx).leaf_count or 2 * GRID * GRID))
    assert grt.set_light_tree(ctx, False) == 0
    noise_off, seconds_off = noise_at(grt, lib, pt, args.samples)
    assert grt.set_light_tree(ctx, True) == 0
    noise_on, seconds_on = noise_at(grt, lib, pt, args.samples)
    equal_time = max(2, int(round(args.samples * seconds_off / seconds_on)))
    noise_on_time, seconds_on_time = noise_at(grt, lib, pt, equal_time)
    lines.append("noise figure (rt_estimate_noise, mean of the cells): tree off %d samples %.4f in %.3f s; tree on %d samples %.4f in %.3f s (equal samples: x %.3f); "
                 "tree on %d samples %.4f in %.3f s (equal time: x %.3f)" % (args.samples, noise_off, seconds_off, args.samples, noise_on, seconds_on, noise_on / noise_off,
                                                                         equal_time, noise_on_time, seconds_on_time, noise_on_time / noise_off))
    pt.close(); scene.close(); grt.config_reset()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
