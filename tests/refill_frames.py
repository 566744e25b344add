"""Frames for tests/test_gpu_trace_refill.py: two 4-sample frames of a bundled scene at 64 x 64 with 10 bounces through the merged
wavefront, as one declared burst or one submission per iteration, and the digest of what rt_read_framebuffer returns.

Run as a program (on a GPU, with the build whose frames are to be recorded) it writes the digests of all four frames as JSON:
    python tests/refill_frames.py tests/golden/refill_frames.json
tests/golden/refill_frames.json was recorded this way from the commit BEFORE the traversal launch batched its shadow rays'
contributions, twice, with equal results."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

W, H, SPP, BOUNCES, FRAMES = 64, 64, 4, 10, 2
SCENES = ("cornellbox", "sponza")


def render(grt, scene_name, burst):
    """(framebuffer float32 copy, per-bounce closest-hit and shadow ray counts)"""
    grt.config_reset()
    grt.config_set(num_bounces=BOUNCES)
    scene = grt.Scene(grt.scene_path(scene_name))
    grt.config_set(num_bounces=BOUNCES)
    pt = grt.Pathtracer(scene, W, H, device=0)
    pt.update()
    lib = grt.device_lib()
    lib.rt_render_samples.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    grt.set_scheduler(pt.ctx, "merged")
    if burst:
        grt.set_frame_pipelining(pt.ctx, True)
        grt.set_stream_batch(pt.ctx, FRAMES * SPP * W * H)
    for f in range(FRAMES):
        assert lib.rt_render_samples(pt.ctx, SPP * f, SPP) == 0, lib.rt_last_error(pt.ctx)
    for _ in range(BOUNCES + FRAMES + 2):   # (no-ops once nothing is in flight)
        grt.advance(pt.ctx)
    assert grt.submissions_completed(pt.ctx) == FRAMES
    counters = pt.counters()
    image = pt.read_framebuffer().copy()
    counts = [int(c) for c in counters.trace[:BOUNCES]], [int(c) for c in counters.shadow[:BOUNCES]]
    pt.close(); scene.close()
    grt.config_reset()
    return image, counts


def digest(image):
    return hashlib.sha256(np.ascontiguousarray(image, np.float32).tobytes()).hexdigest()


def key(scene_name, burst):
    return "%s/%s" % (scene_name, "burst" if burst else "one_by_one")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gpu_raytracer_amd as grt
    out = {"width": W, "height": H, "spp": SPP, "bounces": BOUNCES, "frames": FRAMES, "sha256": {}, "shadow_rays": {}}
    for scene_name in SCENES:
        for burst in (True, False):
            image, counts = render(grt, scene_name, burst)
            assert np.isfinite(image).all() and image[..., :3].max() > 0.0
            out["sha256"][key(scene_name, burst)] = digest(image)
            out["shadow_rays"][key(scene_name, burst)] = int(sum(counts[1]))
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
