"""The shade kernels' four BSDFs on the device (rt_bsdf_eval / rt_bsdf_sample) against the oracle and the float64 reference.

* eval, device against oracle: bit-identical (ok flag, pdf, rgb; NaN equal to NaN) on every probe, given the device's LUTs.
  Both build with -ffp-contract=off and eval uses only IEEE operations.
* sample, device against oracle: ok flag and medium id identical. The warps' sinf / cosf differ from the oracle's libm by
  about 3e-7; the VNDF sampler's normalisations, the reflection and the refraction carry that into the direction, and D into
  the pdf. Bounds: roughness >= 0.3 (and diffuse) direction 1e-5, pdf and throughput 1e-3 relative (measured 4.8e-6 and
  4.5e-4); below 0.3 direction 3e-4, pdf and throughput 1e-2 (measured 1.1e-4 and 3.7e-3, the latter at ior = 1). A probe may take the other branch -- and change its ok flag, direction and medium --
  only where the float32 replay of bsdf_reference.py finds a deciding comparison (r < F_i, r0.x < E_i, r0.y < F,
  r0.y > ratio, pdf_is_valid) within 2e-6 relative of its threshold; those probes are counted and left out of the value
  comparisons.
* Device against the float64 reference: the tolerance regions of bsdf_checks.py (measured on the oracle; the device's eval is
  the oracle's bit for bit), with the same near-threshold probes left out. The index-matched dielectric is held to its ok
  flags only.
* Sample-eval consistency and the chi^2 fit, as in test_bsdf.py, on the device's samples.
* Kulla-Conty LUT coverage: cells in which every index of every axis of each directional table appears, first and last
  included, against the oracle's integration at 1e5 samples (2e-4); the averages against average_* of the device's own
  directional tables.
"""
import numpy as np
import pytest

import bsdf_cases as cases
import bsdf_checks as checks
import bsdf_reference as ref
from conftest import make_pathtracer

pytestmark = pytest.mark.gpu

GRIDS = cases.grids(every=3)
# rt_bsdf_sample against the oracle: (direction absolute, pdf and throughput relative), for roughness >= 0.3 (and diffuse) and below it
# (see the docstring; test_gpu_material.py holds the material launch's continuation rays to the same two pairs)
SAMPLE_BOUNDS = {"rough": (1e-5, 1e-3), "smooth": (3e-4, 1e-2)}


@pytest.fixture(scope="module")
def dev(grt, oracle):
    scene, pt = make_pathtracer(grt, "cornellbox", 64, 64, 0)
    luts = grt.read_luts(pt.ctx)
    view = oracle.SceneView(pt, luts=luts)
    view.tables = ref.Tables(luts)
    view.luts = luts
    view.ctx = pt.ctx
    yield view
    pt.close(); scene.close()


def _same(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name,material_type,probes", GRIDS, ids=[g[0] for g in GRIDS])
def test_device_matches_oracle_and_reference(grt, dev, name, material_type, probes):
    got = grt.bsdf_eval(dev.ctx, material_type, probes)
    want = dev.bsdf_eval(material_type, probes)
    same = _same(got[:, :5], want[:, :5]).all(1) & (got[:, 9] == want[:, 9]) & _same(got[:, 10], want[:, 10])
    bad = np.nonzero(~same)[0]
    assert bad.size == 0, "%s eval: %d probes differ from the oracle, first %d: %s vs %s" % (name, bad.size, bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())
    r_eval, _ = ref.evaluate(material_type, probes, dev.tables, eval=True)
    checks.compare_with_reference(name + " eval", material_type, probes, got, r_eval)

    U = checks.uniforms(dev.random, probes)   # the oracle's random numbers, which the RNG tests hold equal to the device's
    got = grt.bsdf_sample(dev.ctx, material_type, probes)
    want = dev.bsdf_sample(material_type, probes)
    r, _ = ref.evaluate(material_type, probes, dev.tables, eval=False, uniforms=U)
    differ = (got[:, 0] != want[:, 0]) | (got[:, 8] != want[:, 8])
    flipped = differ | ((got[:, 0] == 1) & (np.abs(got[:, 5:8] - want[:, 5:8]).max(1) > 1e-6) & r.near)
    assert not (differ & ~r.near).any(), "%s sample: ok flag or medium differ from the oracle away from any threshold at probes %s" % (
        name, np.nonzero(differ & ~r.near)[0][:8].tolist())
    both = (got[:, 0] == 1) & ~flipped
    smooth = material_type != ref.DIFFUSE and checks.roughness_of(material_type, probes[0, :8]) < 0.3
    dir_tol, rel_tol = SAMPLE_BOUNDS["smooth" if smooth else "rough"]
    errors = {"direction": np.abs(got[both, 5:8] - want[both, 5:8]).max(1) if both.any() else np.zeros(1)}
    for k, label in ((1, "pdf"), (2, "r"), (3, "g"), (4, "b")):
        errors[label] = np.abs(got[both, k] - want[both, k]) / np.maximum(np.abs(want[both, k]), 1e-30) if both.any() else np.zeros(1)
    worst = {k: float(v.max()) for k, v in errors.items()}
    assert worst["direction"] <= dir_tol and max(worst["pdf"], worst["r"], worst["g"], worst["b"]) <= rel_tol, (
        "%s: direction %.3g pdf %.3g rgb %.3g %.3g %.3g, %d probes on the other branch" % (
            name, worst["direction"], worst["pdf"], worst["r"], worst["g"], worst["b"], int(flipped.sum())))
    checks.compare_with_reference(name + " sample", material_type, probes, got, r, skip=flipped)
    checks.check_consistency(name, material_type, probes, got, grt.bsdf_eval(dev.ctx, material_type, checks.eval_at_samples(probes, got)))


@pytest.mark.parametrize("name,material_type,material,entering,cos_i", cases.CHI2, ids=[c[0] for c in cases.CHI2])
def test_device_sampled_directions_fit_the_pdf(grt, dev, name, material_type, material, entering, cos_i):
    probes = cases.chi2_probes(material, entering, cos_i)
    sampled = grt.bsdf_sample(dev.ctx, material_type, probes)
    p, chi2, dof, other = checks.chi2_p_value(material_type, probes[0], sampled, dev.tables)
    assert p > 1e-6, (name, p, chi2, dof, other)


def test_probes_refuse_bad_arguments(grt, dev):
    p = cases.grid(0, cases.material_record(ref.DIFFUSE), True)[:4].copy()
    for bad_type in (0, 5, -1):
        with pytest.raises(RuntimeError, match="material_type"):
            grt.bsdf_eval(dev.ctx, bad_type, p)
    p[1, 3] = np.array([0], np.int32).view(np.float32)[0]   # texture 0
    with pytest.raises(RuntimeError, match="texture"):
        grt.bsdf_sample(dev.ctx, ref.DIFFUSE, p)


def _covering_cells(n, dims):
    """Cells of an n^dims table in which every index of every axis appears, the first and last included."""
    cells = set()
    for k in range(n):
        idx = [k] + [(k * (2 * a + 5) + 3 * a) % n for a in range(1, dims)]
        cells.add(sum(i * n ** a for a, i in enumerate(idx)))
    cells.add(0); cells.add(n ** dims - 1)
    return sorted(cells)


def test_kulla_conty_lut_coverage(dev, oracle):
    luts = dev.luts
    for entering, lut in ((True, luts[0]), (False, luts[1])):
        for cell in _covering_cells(16, 3):
            want = dev.integrate_dielectric_cells(entering, cell, 1)
            assert abs(lut[cell] - want[0]) <= 2e-4, (entering, cell, lut[cell], want[0])
    for cell in _covering_cells(32, 2):
        want = dev.integrate_conductor_cells(cell, 1)
        assert abs(luts[4][cell] - want[0]) <= 2e-4, (cell, luts[4][cell], want[0])
    assert np.allclose(luts[2], oracle.average_dielectric(luts[0]), rtol=0, atol=1e-6)
    assert np.allclose(luts[3], oracle.average_dielectric(luts[1]), rtol=0, atol=1e-6)
    assert np.allclose(luts[5], oracle.average_conductor(luts[4]), rtol=0, atol=1e-6)
