"""The oracle's four BSDFs (oracle_bsdf_eval / oracle_bsdf_sample) against the float64 restatement of bsdf_reference.py,
probe by probe, with no GPU; sample-eval consistency and a chi^2 goodness of fit of the sampled directions. The Kulla-Conty
tables are the oracle's own cell integration at a reduced sample count. The device side is test_gpu_bsdf.py; the
tolerance regions are in bsdf_checks.py."""
import numpy as np
import pytest

import bsdf_cases as cases
import bsdf_checks as checks
import bsdf_reference as ref

LUT_SAMPLES = 1500


@pytest.fixture(scope="module")
def view(grt, oracle):
    grt.config_reset()
    scene = grt.Scene(grt.scene_path("cornellbox"))
    pt = grt.Pathtracer(scene, 16, 16, device=-1); pt.update()
    plain = oracle.SceneView(pt)
    luts = [plain.integrate_dielectric_cells(True, 0, 4096, LUT_SAMPLES), plain.integrate_dielectric_cells(False, 0, 4096, LUT_SAMPLES)]
    luts += [oracle.average_dielectric(luts[0]), oracle.average_dielectric(luts[1])]
    luts.append(plain.integrate_conductor_cells(0, 1024, LUT_SAMPLES))
    luts.append(oracle.average_conductor(luts[4]))
    v = oracle.SceneView(pt, luts=luts)
    v.tables = ref.Tables(luts)
    yield v
    pt.close(); scene.close()


GRIDS = cases.grids(every=3)


@pytest.mark.parametrize("name,material_type,probes", GRIDS, ids=[g[0] for g in GRIDS])
def test_oracle_matches_float64_reference(view, name, material_type, probes):
    got = view.bsdf_eval(material_type, probes)
    want, _ = ref.evaluate(material_type, probes, view.tables, eval=True)
    checks.compare_with_reference(name + " eval", material_type, probes, got, want)
    got = view.bsdf_sample(material_type, probes)
    want, _ = ref.evaluate(material_type, probes, view.tables, eval=False, uniforms=checks.uniforms(view.random, probes))
    checks.compare_with_reference(name + " sample", material_type, probes, got, want)
    assert (got[:, 9] == want.allow_nee).all()
    checks.check_consistency(name, material_type, probes, got, view.bsdf_eval(material_type, checks.eval_at_samples(probes, got)))


def test_refused_and_pinned_cases(view):
    """omega_i.z <= 0 is refused (-1). Plastic continues below the horizon with a valid pdf (BSDF.h:154 rejects only
    omega_m.z < 0; G2 is 0 there, and the diffuse term stays positive because 1 - F_o changes sign with cos_o), and the
    float64 reference agrees on exactly which probes do. (ior = 1: the ok flags agree, in the grids.)"""
    p = cases.grid(0, cases.material_record(ref.PLASTIC, roughness=0.6), True, hashed=True)
    p[:, 11:14] *= -1   # every ray now leaves the surface
    assert (view.bsdf_sample(ref.PLASTIC, p)[:, 0] == -1).all() and (view.bsdf_eval(ref.PLASTIC, p)[:, 0] == -1).all()
    p = cases.chi2_probes(cases.material_record(ref.PLASTIC, roughness=0.6), True, 0.15, count=1 << 15)
    got = view.bsdf_sample(ref.PLASTIC, p)
    want, _ = ref.evaluate(ref.PLASTIC, p, view.tables, eval=False, uniforms=checks.uniforms(view.random, p))
    below = (got[:, 0] == 1) & (got[:, 7] < 0)
    assert below.sum() > 0 and np.isfinite(got[below, 1:5]).all()
    assert np.array_equal(below, (want.ok == 1) & (want.direction[:, 2] < 0))


@pytest.mark.parametrize("name,material_type,material,entering,cos_i", cases.CHI2, ids=[c[0] for c in cases.CHI2])
def test_sampled_directions_fit_the_pdf(view, name, material_type, material, entering, cos_i):
    probes = cases.chi2_probes(material, entering, cos_i)
    sampled = view.bsdf_sample(material_type, probes)
    p, chi2, dof, other = checks.chi2_p_value(material_type, probes[0], sampled, view.tables)
    assert p > 1e-6, (name, p, chi2, dof, other)


def test_reference_by_hand():
    """A few values worked out on paper, so the reference is pinned by more than its own text."""
    R = ref.Run(ref.F64)   # a float64 run that records its own decisions, with the true pi
    R.PI, R.INV_PI = np.pi, 1 / np.pi
    one = np.ones(1)
    # normal incidence on glass: ((1 - 1.5) / (1 + 1.5))^2 = 0.04
    assert abs(ref.fresnel_dielectric(R, one, 1 / 1.5)[0] - 0.04) < 1e-12
    assert ref.fresnel_dielectric(R, 0.1 * one, 1.5)[0] == 1.0   # total internal reflection leaving glass at 84 degrees
    # a conductor with k = 0 is a dielectric of that eta at normal incidence
    assert abs(ref.fresnel_conductor(R, one, (1.5 * one,) * 3, (0 * one,) * 3)[0][0] - 0.04) < 1e-12
    # GGX D integrates the projected area to 1: sum D(m) m.z dm over the hemisphere
    z = (np.arange(4000) + 0.5) / 4000
    D = ref.ggx_D(R, (np.sqrt(1 - z * z), 0 * z, z), 0.3 * np.ones_like(z))
    assert abs((D * z).sum() * 2 * np.pi / 4000 - 1) < 1e-3
    # Lambda(0, 0, 1) = 0; the concentric disk maps the centre and the corner (1, 1) -> r = 1 on phi = pi / 4
    assert ref.ggx_lambda(R, (0 * one, 0 * one, one), one)[0] == 0
    x, y = ref.sample_disk(R, one, one)
    assert abs(x[0] - np.sin(np.pi / 4)) < 1e-12 and abs(y[0] - np.cos(np.pi / 4)) < 1e-12
