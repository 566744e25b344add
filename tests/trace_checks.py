"""What the CPU and the GPU traversal tests share: loading a case, the float64 rules a traversal's results must keep, and the
report line per case. TEST INFRASTRUCTURE ONLY.

Rules (tests/trace_reference.py names the tolerances):
* robust closest-hit rays: the named triangle is hit at float64's closest t (so it is float64's, or coplanar with it over the
  hit point), t within the t bound, the stored
  16-bit u, v within 1 / 65535 of float64's plus the u, v bound; robust misses stay misses;
* every hit: the named triangle is a real float64 intersection -- margin >= -(u, v bound), t >= -(t bound) -- at a t within its
  t bound of the float64 t of that triangle, and not behind float64's nearest unambiguous hit (t_clear);
* a miss only where no float64 hit is robust: float64's closest hit must be ambiguous;
* robust shadow rays: occlusion equals float64's.
"""
import numpy as np

import trace_reference as ref

TOL_GAP = ref.TOL.GAP / ref.TOL.T
STACK_LIMIT = 32   # RT_STACK_SIZE (kernels_trace.hip): entries per lane; the device does not check its spill index
LDS_STACK = 10     # RT_LDS_STACK: the entries of them kept in LDS; a deeper stack spills to HBM


def load(grt, case, device, **config):
    grt.config_reset()
    grt.config_set(**case.config, **config)
    scene = grt.Scene(case.scene)
    grt.config_set(**case.config, **config)
    pt = grt.Pathtracer(scene, 32, 32, device=device)
    pt.update()
    return scene, pt


def unpack(hits):
    return hits[:, 0].view(np.int32), hits[:, 1].view(np.int32), hits[:, 2].view(np.float32), hits[:, 3] & 0xffff, hits[:, 3] >> 16


class Report:
    """Worst cases against float64 over a run, in units of the tolerances (1.0 = at the bound)."""

    def __init__(self):
        self.rows = []

    def add(self, label, robust_fraction, t_units, t_ulps, uv_units, leaks=None):
        self.rows.append((label, robust_fraction, t_units, t_ulps, uv_units, leaks))

    def lines(self):
        out = []
        for label, rf, tu, tl, uvu, leaks in self.rows:
            out.append("%-28s robust %5.1f %%  worst t %6.3f of bound (%6.1f ulp)  worst u,v %6.3f of bound%s" % (
                label, 100 * rf, tu, tl, uvu, "" if leaks is None else "  leaks %d" % leaks))
        return out


def check_closest(label, case, pt, origin, direction, hits, bf, report=None):
    """The float64 rules on closest-hit records `hits` of rays (origin, direction) against the brute force `bf`."""
    mesh, tri, t, u16, v16 = unpack(hits)
    hit = tri >= 0
    robust = ref.robust_closest(bf)
    f64_hit = np.isfinite(bf.t)
    # robust misses stay misses, robust hits stay hits
    bad = np.nonzero(robust & (hit != f64_hit))[0]
    assert bad.size == 0, "%s: %d robust rays hit / miss against float64, first %d: t %r, float64 t %r" % (label, bad.size, bad[0], t[bad[0]], bf.t[bad[0]])
    # a miss only where float64's closest hit is not robust
    bad = np.nonzero(~hit & f64_hit & robust)[0]
    assert bad.size == 0
    idx = np.nonzero(hit)[0]
    report_t = report_ulp = report_uv = 0.0
    if idx.size:
        world = ref.world_triangles_of_hits(pt.array("triangles"), pt.array("mesh_transforms"), mesh[idx], tri[idx])
        tn, margin, g, t_tol, un, vn, uv_tol, tiny = ref.evaluate_named(origin[:, idx], direction[:, idx], world)
        with np.errstate(invalid="ignore"):
            real = (margin >= -uv_tol) & (tn >= -t_tol) & (np.abs(t[idx] - tn) <= t_tol) & (tn <= bf.t_clear[idx] + np.where(np.isfinite(bf.t_clear[idx]), TOL_GAP * bf.t_tol[idx], 0) + t_tol)
        real |= tiny & (tn > 0)   # (float32 underflows on this triangle: its t and u, v are not checked, only that it lies ahead)
        bad = idx[~real]
        assert bad.size == 0, "%s: %d hits are not float64 intersections of the triangle they name, first ray %d: t %r named-t %r margin %r float64 t %r" % (
            label, bad.size, bad[0], t[bad[0]], tn[~real][0], margin[~real][0], bf.t[bad[0]])
        r = robust[idx]
        if r.any():
            ri = idx[r]
            # float64's triangle: the named one is a real intersection (above) at float64's closest t. On a robust ray no other
            # triangle's intersection lies within GAP t bounds of it, so only float64's triangle -- or a coplanar one that covers the
            # same point, as a quad split along its other diagonal does -- can be there.
            bad = ri[~(np.abs(tn[r] - bf.t[ri]) <= bf.t_tol[ri] + t_tol[r])]
            assert bad.size == 0, "%s: %d robust rays name a triangle that float64 does not hit at its closest t, first ray %d (t %r, float64 t %r)" % (label, bad.size, bad[0], t[bad[0]], bf.t[bad[0]])
            err_t = np.abs(t[ri].astype(np.float64) - bf.t[ri])
            assert (err_t <= bf.t_tol[ri]).all(), "%s: t off float64 beyond its bound" % label
            err_u = np.abs(u16[ri] / 65535.0 - un[r]); err_v = np.abs(v16[ri] / 65535.0 - vn[r])   # (u, v of the named triangle)
            err_uv = np.maximum(err_u, err_v)
            assert (err_uv <= 1 / 65535.0 + uv_tol[r]).all(), "%s: u, v off float64 beyond 1/65535 and their bound" % label
            report_t = float((err_t / bf.t_tol[ri]).max())
            report_ulp = float((err_t / np.spacing(np.abs(bf.t[ri]).astype(np.float32)).astype(np.float64)).max())
            report_uv = float((np.maximum(err_uv - 1 / 65535.0, 0) / uv_tol[r]).max())
    if report is not None:
        leaks = int((~hit).sum()) if case.closed else None
        report.add(label, float(robust.mean()), report_t, report_ulp, report_uv, leaks)


FLAG_BOUNCE_0 = np.uint32(1 << 30)   # RT_SHADOW_FLAG_BOUNCE_0: merged wavefront, the pixel word of a shadow ray emitted at bounce 0
RADIANCE, DIRECT, INDIRECT = range(3)   # the three frames of rt_trace_queue_rays, in its order


def expected_frames(frames, illumination, pixel_words, occluded, bounce=None, ao=False):
    """What a shadow launch leaves in the frames [RADIANCE, DIRECT, INDIRECT] ((P, 4) float32 each, None: the launch has no such frame), in float32
    as the kernels add (ShadowQueueSource::finish, ShadowStreamSource::contribute, ShadowAOSource::finish in kernels_trace.hip): an unoccluded ray
    of illumination (M, 3) adds value = (illumination, 0) to its RADIANCE pixel in all four channels, SETS its DIRECT pixel to value when it is of
    bounce 0 and adds value to its INDIRECT pixel otherwise; an occluded ray writes nothing. `bounce`: the per-bounce launch's (the pixel word is
    the pixel); None: the merged launch, where FLAG_BOUNCE_0 of the word says bounce 0 and the rest is the pixel. ao: the AO integrator's launch,
    which sets RADIANCE to (1, 1, 1, 1) and touches nothing else. No two rays may name one pixel. Returns new arrays (None where None)."""
    words = np.asarray(pixel_words, np.uint32)
    light = np.asarray(illumination, np.float32).reshape(-1, 3)
    live = ~np.asarray(occluded).astype(bool)
    if bounce is None:
        pixel, first = (words & ~FLAG_BOUNCE_0).astype(np.int64), (words & FLAG_BOUNCE_0) != 0
    else:
        assert not (words & FLAG_BOUNCE_0).any(), "a per-bounce launch has no flag in its pixel words"
        pixel, first = words.astype(np.int64), np.full(words.size, bounce == 0)
    assert np.unique(pixel).size == pixel.size, "two shadow rays name one pixel"
    value = np.concatenate([light, np.zeros((light.shape[0], 1), np.float32)], 1)
    out = [None if f is None else np.array(f, np.float32, copy=True) for f in frames]
    if ao:
        if out[RADIANCE] is not None:
            out[RADIANCE][pixel[live]] = np.float32(1.0)
        return out
    if out[RADIANCE] is not None:
        out[RADIANCE][pixel[live]] = out[RADIANCE][pixel[live]] + value[live]
    if out[DIRECT] is not None:
        out[DIRECT][pixel[live & first]] = value[live & first]
    if out[INDIRECT] is not None:
        out[INDIRECT][pixel[live & ~first]] = out[INDIRECT][pixel[live & ~first]] + value[live & ~first]
    return out


def check_frames(label, got, want, prefill, illumination, pixel_words):
    """The frames a launch left, against expected_frames, AS BITS; a pixel that differs is named with what happened to it where that can be told: a
    contribution lost (the prefill is still there) or made twice (prefill + 2 x value). Returns the pixels compared per frame."""
    words = np.asarray(pixel_words, np.uint32)
    pixel = (words & ~FLAG_BOUNCE_0).astype(np.int64)
    value = np.concatenate([np.asarray(illumination, np.float32).reshape(-1, 3), np.zeros((words.size, 1), np.float32)], 1)
    counts = []
    for name, g, w, before in zip(("RADIANCE", "RADIANCE_DIRECT", "RADIANCE_INDIRECT"), got, want, prefill):
        assert (g is None) == (w is None), "%s: %s is %s" % (label, name, "missing" if g is None else "unexpected")
        if g is None:
            counts.append(0)
            continue
        bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).any(1))[0]
        if bad.size:
            p = int(bad[0])
            ray = np.nonzero(pixel == p)[0]
            what = "no ray names it"
            if ray.size:
                r = int(ray[0])
                twice = np.asarray(before, np.float32)[p] + value[r] + value[r]
                what = "ray %d names it (word 0x%08x, value %s): %s" % (r, int(words[r]), value[r].tolist(),
                       "its contribution was LOST (the prefill is unchanged)" if np.array_equal(g[p].view(np.uint32), np.asarray(before, np.float32)[p].view(np.uint32))
                       else "its contribution was made TWICE" if np.array_equal(g[p].view(np.uint32), twice.view(np.uint32)) else "neither lost nor doubled")
            raise AssertionError("%s: %d pixels of %s differ from the expected frame, first pixel %d: got %s, want %s, prefill %s; %s" % (
                label, bad.size, name, p, g[p].tolist(), w[p].tolist(), np.asarray(before, np.float32)[p].tolist(), what))
        counts.append(int(g.shape[0]))
    return counts


def check_shadow(label, occluded, bf, max_distance):
    robust = ref.robust_shadow(bf, max_distance)
    want = ref.occluded(bf, max_distance)
    bad = np.nonzero(robust & (np.asarray(occluded).astype(bool) != want))[0]
    assert bad.size == 0, "%s: %d robust shadow rays disagree with float64 occlusion, first %d (limit %r, float64 t %r)" % (
        label, bad.size, bad[0], max_distance[bad[0]], bf.t[bad[0]])
    return float(robust.mean())
