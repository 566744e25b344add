"""What the CPU and the GPU BSDF tests share: the tolerance regions, the sample-eval consistency check and the goodness of fit.

Tolerances against the float64 reference (bsdf_reference.py), measured on the oracle (the device's eval is bit-identical to
it; its samples differ from it by the sin / cos ulps of the warps). pdf: relative error; value: relative error per channel,
floored at 1e-3 of the probe's largest channel; direction: absolute. Regions, with the worst case measured on the oracle:

* diffuse: 2e-4 (measured 4e-5; the pdf of a sample is omega_o.z / pi of a float32 direction).
* roughness >= 0.3, |omega_i.z| and |omega_o.z| >= 1e-3: plastic and conductor pdf 1e-4 (3e-5), value 3e-3 (7.4e-4: the
  conductor's Fresnel at k >> eta); dielectric pdf 4e-3 (1.4e-3), value 4e-2 (8e-3: ior 1.0001 and ior 3 outside the
  LUT range, where 1 - F_avg and the reciprocity factor cancel).
* the cutoff <= roughness < 0.3: pdf 2e-2 (9.6e-3), value 6e-2 (2.8e-2). D of a float32 half-vector at alpha = 0.0025 is
  conditioned like tan(theta) / alpha^2.
* roughness below the cutoff, or omega_i.z or omega_o.z below 1e-3: pdf 2e-2 (7.3e-3); the value only to 1 (0.44: a
  dielectric at grazing exit).
* the index-matched dielectric (ior = 1): ok flags only. eval's half-vector eta omega_i + omega_o of the straight-through
  direction degenerates (relative pdf errors of 1e16 are measured), so only which probes succeed is pinned.
Directions of successful samples: 1e-3 everywhere (measured 2.3e-4 at the cutoff).
"""
import numpy as np

import bsdf_cases as cases
import bsdf_reference as ref

DIRECTION_TOL = 1e-3


def roughness_of(material_type, m):
    return {ref.DIFFUSE: 1.0, ref.PLASTIC: m[4], ref.DIELECTRIC: m[2], ref.CONDUCTOR: m[3]}[material_type]


def bounds(material_type, material, grazing):
    """(pdf tolerance, value tolerance) per probe, or None: ok flags only."""
    r = roughness_of(material_type, material)
    if material_type == ref.DIELECTRIC and material[1] == 1.0:
        return None
    if material_type == ref.DIFFUSE:
        return np.full(grazing.shape, 2e-4), np.full(grazing.shape, 2e-4)
    if r < cases.CUTOFF:
        return np.full(grazing.shape, 2e-2), np.full(grazing.shape, 1.0)
    if r < 0.3:
        p, v = 2e-2, 6e-2
    elif material_type == ref.DIELECTRIC:
        p, v = 4e-3, 4e-2
    else:
        p, v = 1e-4, 3e-3
    return np.where(grazing, 2e-2, p), np.where(grazing, 1.0, v)


def compare_with_reference(label, material_type, probes, got, want, skip=None):
    """got: (N, 12) output records; want: the float64 Result. skip: probes left out of the value comparison (named by the caller)."""
    skip = np.zeros(len(probes), bool) if skip is None else skip
    bad = np.nonzero((got[:, 0] != want.ok) & ~skip)[0]
    assert bad.size == 0, "%s: ok flags differ at %d probes, first %d: got %s want %d" % (label, bad.size, bad[0], got[bad[0]].tolist(), want.ok[bad[0]])
    b = bounds(material_type, probes[0, :8], np.zeros(1, bool))
    if b is None:
        return
    n = probes[:, 8:11].astype(np.float64)
    oz = np.abs((got[:, 5:8] * n).sum(1))
    grazing = np.minimum(oz, np.abs(got[:, 10])) < 1e-3
    pdf_tol, val_tol = bounds(material_type, probes[0, :8], grazing)
    sel = (got[:, 0] == 1) & (want.ok == 1) & ~skip
    e_pdf = np.abs(got[:, 1] - want.pdf) / np.maximum(np.abs(want.pdf), 1e-30)
    floor = 1e-3 * np.abs(want.value).max(1, keepdims=True) + 1e-30
    e_val = (np.abs(got[:, 2:5] - want.value) / np.maximum(np.abs(want.value), floor)).max(1)
    e_dir = np.abs(got[:, 5:8] - want.direction).max(1)
    for name, e, tol in (("pdf", e_pdf, pdf_tol), ("value", e_val, val_tol), ("direction", e_dir, DIRECTION_TOL)):
        over = np.nonzero(sel & (e > tol))[0]
        assert over.size == 0, "%s: %s off at %d probes, worst %.3g at %d: got %s want pdf %r value %s dir %s" % (
            label, name, over.size, e[over].max(), over[e[over].argmax()], got[over[e[over].argmax()]].tolist(), want.pdf[over[e[over].argmax()]],
            want.value[over[e[over].argmax()]].tolist(), want.direction[over[e[over].argmax()]].tolist())


def uniforms(random, probes):
    """The DIM_BSDF_0 and DIM_BSDF_1 pairs of every probe's key. random(dimension, pixels, bounce, sample) -> (N, 2)."""
    key = probes[:, 19:22].view(np.uint32)
    out = [np.zeros((len(probes), 2), np.float32) for _ in range(2)]
    for bounce in np.unique(key[:, 2]):
        for sample in np.unique(key[key[:, 2] == bounce, 1]):
            sel = (key[:, 2] == bounce) & (key[:, 1] == sample)
            for k, dim in enumerate((5, 6)):   # DIM_BSDF_0, DIM_BSDF_1
                out[k][sel] = random(dim, key[sel, 0], int(bounce), int(sample))
    return out


def eval_at_samples(probes, sampled):
    """Eval probes at the directions the samples returned."""
    e = probes.copy()
    e[:, 15:18] = sampled[:, 5:8]
    e[:, 18] = (sampled[:, 5:8] * probes[:, 8:11]).sum(1, dtype=np.float32)
    return e


def check_consistency(label, material_type, probes, sampled, evaluated):
    """For every successful sample whose direction eval covers: eval's pdf equals the sample's, and the throughput factor is
    bsdf / pdf (times the albedo for diffuse). Plastic's reflections below the horizon (pinned elsewhere) are left out."""
    r = roughness_of(material_type, probes[0, :8])
    if material_type != ref.DIFFUSE and r < 0.1:
        return 0
    if material_type == ref.DIELECTRIC and probes[0, 1] < 1.33:   # ior 1 (pinned: ok flags only) and 1.0001 (pdf ill-conditioned)
        return 0
    cos_o = (sampled[:, 5:8] * probes[:, 8:11]).sum(1)
    sel = (sampled[:, 0] == 1) & (np.minimum(np.abs(cos_o), np.abs(sampled[:, 10])) >= 1e-3)
    if material_type != ref.DIELECTRIC:
        sel &= cos_o > 0
    assert (evaluated[sel, 0] == 1).all(), "%s: eval refuses %d sampled directions" % (label, (evaluated[sel, 0] != 1).sum())
    tol = 2e-3 if r >= 0.3 else 1e-2   # eval re-derives omega_o from the world direction: at alpha = 0.01 that moves D by 4e-3
    rel = np.abs(evaluated[sel, 1] - sampled[sel, 1]) / sampled[sel, 1]
    assert rel.size == 0 or rel.max() < tol, "%s: eval pdf differs from the sample's by %.3g" % (label, rel.max())
    factor = evaluated[sel, 2:5] / evaluated[sel, 1:2]
    if material_type == ref.DIFFUSE:
        factor = factor * probes[sel, 0:3]
    rel = np.abs(factor - sampled[sel, 2:5]) / np.maximum(np.abs(sampled[sel, 2:5]), 1e-3)
    assert rel.size == 0 or rel.max() < tol, "%s: throughput differs from bsdf / pdf by %.3g" % (label, rel.max())
    return int(sel.sum())


def chi2_p_value(material_type, probe, sampled, tables):
    """Goodness of fit of sampled directions (normal +z) against the float64 quadrature of the eval pdf over the upper
    hemisphere. Transmitted samples go to the "other" bin: the reference's transmission pdf takes |omega_o . m| in the
    refraction Jacobian's denominator (eta |i.m| + |o.m|)^2, where the signed o.m belongs, so its lower hemisphere does not
    integrate to the sampled density; the reflected part is held to the fit."""
    expected = ref.pdf_quadrature(material_type, probe, tables, hemispheres=(True,))
    n = len(sampled)
    ok = sampled[:, 0] == 1
    covered = ok & (np.isfinite(sampled[:, 5:8]).all(1)) & (sampled[:, 7] >= 0)
    counts = np.bincount(ref.bin_index(sampled[covered, 5:8]), minlength=expected.size)
    p, chi2, dof = ref.chi2_test(counts, n - covered.sum(), expected, n)
    return p, chi2, dof, int(n - covered.sum())
