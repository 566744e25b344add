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


def check_shadow(label, occluded, bf, max_distance):
    robust = ref.robust_shadow(bf, max_distance)
    want = ref.occluded(bf, max_distance)
    bad = np.nonzero(robust & (np.asarray(occluded).astype(bool) != want))[0]
    assert bad.size == 0, "%s: %d robust shadow rays disagree with float64 occlusion, first %d (limit %r, float64 t %r)" % (
        label, bad.size, bad[0], max_distance[bad[0]], bf.t[bad[0]])
    return float(robust.mean())
