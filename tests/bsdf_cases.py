"""Probe sets of the BSDF tests: 24-float records of rt_bsdf_eval / rt_bsdf_sample (include/gpu_raytracer_amd.h).

The grids reach the edges the whole-frame tests rarely or never hit: omega_i.z of exactly 1 (the VNDF sampler's axis at
normal incidence) and down to 1e-4; omega_o in both hemispheres; roughness 0, 1e-3, either side of the cutoff, 1; IORs at
and outside the ends of the dielectric LUT, the index-matched ior = 1, both sides of the surface with total internal
reflection; conductors with k = 0 and the furnace material. Keys of two kinds: sample indices below the PMJ table size
(the PMJ + blue-noise path the frames use) and above it (the hashed path, which the goodness-of-fit tests need: across
pixels at one sample index the PMJ path takes only 256 distinct values per axis).
"""
import numpy as np

from bsdf_reference import CONDUCTOR, DIELECTRIC, DIFFUSE, PLASTIC, PMJ_SAMPLES

F32 = np.float32
CUTOFF = F32(0.05)
ROUGHNESS = [F32(0), F32(1e-3), np.nextafter(CUTOFF, F32(0)), CUTOFF, np.nextafter(CUTOFF, F32(1)), F32(0.1), F32(0.3), F32(0.6), F32(1)]
IORS = [1.0, 1.0001, 1.33, 1.5, 2.5, 3.0]
CONDUCTORS = {   # (eta, k)
    "k0": ((1.5, 1.2, 0.8), (0.0, 0.0, 0.0)),
    "gold": ((0.143, 0.374, 1.442), (3.983, 2.385, 1.603)),
    "copper": ((0.200, 0.924, 1.102), (3.912, 2.452, 2.142)),
    "furnace": ((0.2, 0.2, 0.2), (8.0, 8.0, 8.0)),
}
COS_I = [1.0, 0.999, 0.9, 0.7, 0.5, 0.3, 0.1, 0.03, 1e-2, 1e-3, 1e-4]
PHI_O = [0.0, 0.9, 2.2, np.pi, 4.4]


def material_record(material_type, roughness=0.3, ior=1.5, eta=(1, 1, 1), k=(0, 0, 0), albedo=(0.8, 0.5, 0.2), medium=3):
    """The 32-byte record of rt_upload_materials (CUDA/Material.h:21-39) as 8 float32."""
    m = np.zeros(8, F32)
    if material_type in (DIFFUSE, PLASTIC):
        m[:3] = albedo
        m[3:4] = np.array([-1], np.int32).view(F32)   # texture id RT_INVALID
        m[4] = roughness
    elif material_type == DIELECTRIC:
        m[0:1] = np.array([medium], np.int32).view(F32)
        m[1], m[2] = ior, roughness
    else:
        m[:3] = eta; m[3] = roughness; m[4:7] = k
    return m


def _tilted_normal(i):
    """A few shading normals, +z first (the frame where local = world)."""
    normals = [(0, 0, 1), (0.3, -0.2, 0.93), (-0.6, 0.7, -0.3), (0, 0, -1), (0.8, 0.6, 0.0)]
    n = np.array(normals[i % len(normals)], np.float64)
    return (n / np.linalg.norm(n)).astype(F32)


def _local_dir(cos_theta, phi):
    s = np.sqrt(max(0.0, 1 - cos_theta * cos_theta))
    return np.array([s * np.cos(phi), s * np.sin(phi), cos_theta])


def probes(material, entering, normal_index, pairs, keys):
    """One record per (omega_i, omega_o) pair in the frame of normal `normal_index`, with the given keys (pixel, sample, bounce)."""
    n = _tilted_normal(normal_index).astype(np.float64)
    sign = np.copysign(1.0, n[2]); a = -1.0 / (sign + n[2]); b = n[0] * n[1] * a
    t = np.array([1 + sign * n[0] * n[0] * a, sign * b, -sign * n[0]]); bt = np.array([b, sign + n[1] * n[1] * a, -n[1]])
    out = np.zeros((len(pairs), 24), F32)
    for r, ((wi, wo), key) in enumerate(zip(pairs, keys)):
        d = -(wi[0] * t + wi[1] * bt + wi[2] * n)
        l = wo[0] * t + wo[1] * bt + wo[2] * n
        out[r, :8] = material
        out[r, 8:11] = n
        out[r, 11:14] = d / np.linalg.norm(d)
        out[r, 14] = 1.0 if entering else 0.0
        out[r, 15:18] = l / np.linalg.norm(l)
        out[r, 18] = F32(out[r, 15:18].astype(np.float64) @ n)
        out[r, 19:22] = np.array(key, np.uint32).view(F32)
    return out


def direction_pairs(lower=True):
    """omega_i over COS_I x 2 azimuths, omega_o over COS_I (both hemispheres) x PHI_O."""
    pairs = []
    for ci in COS_I:
        for phi_i in (0.0, 2.5):
            wi = _local_dir(ci, phi_i)
            for co in COS_I:
                for phi_o in PHI_O:
                    for s in ((1, -1) if lower else (1,)):
                        pairs.append((wi, _local_dir(s * co, phi_o)))
    return pairs


def configurations():
    """(name, material_type, material record, entering) of every configuration the grids run."""
    out = [("diffuse", DIFFUSE, material_record(DIFFUSE), True)]
    for r in ROUGHNESS:
        out.append(("plastic_r%.9g" % r, PLASTIC, material_record(PLASTIC, roughness=r), True))
        for name, (eta, k) in CONDUCTORS.items():
            out.append(("conductor_%s_r%.9g" % (name, r), CONDUCTOR, material_record(CONDUCTOR, roughness=r, eta=eta, k=k), True))
        for ior in IORS:
            for entering in (True, False):
                out.append(("dielectric_ior%g_r%.9g_%s" % (ior, r, "in" if entering else "out"), DIELECTRIC,
                            material_record(DIELECTRIC, roughness=r, ior=ior), entering))
    return out


def grid(config_index, material, entering, hashed=False, every=1):
    """The direction grid of one configuration, under one of the normals, each pair with its own key."""
    pairs = direction_pairs()[::every]
    count = len(pairs)
    pixels = (np.arange(count) * 37 + config_index * 101) % 4093
    samples = (np.arange(count) * 7 + config_index) % PMJ_SAMPLES + (PMJ_SAMPLES if hashed else 0)
    bounces = np.arange(count) % 3
    keys = list(zip(pixels, samples, bounces))
    return probes(material, entering, config_index, pairs, keys)


def grids(every=1):
    """Every configuration's grid with PMJ keys and with hashed keys: [(name, material_type, probes)]."""
    out = []
    for i, (name, material_type, material, entering) in enumerate(configurations()):
        out.append((name + "_pmj", material_type, grid(i, material, entering, False, every)))
        out.append((name + "_hashed", material_type, grid(i, material, entering, True, every)))
    return out


# goodness of fit: normal +z, hashed keys, 2^20 samples per configuration
CHI2_SAMPLES = 1 << 20
CHI2 = [
    ("diffuse", DIFFUSE, material_record(DIFFUSE), True, 0.6),
    ("plastic_r0.3", PLASTIC, material_record(PLASTIC, roughness=0.3), True, 0.8),
    ("plastic_r0.6_grazing", PLASTIC, material_record(PLASTIC, roughness=0.6), True, 0.15),
    ("conductor_gold_r0.3", CONDUCTOR, material_record(CONDUCTOR, 0.3, 1.5, *CONDUCTORS["gold"]), True, 0.5),
    ("conductor_furnace_r1", CONDUCTOR, material_record(CONDUCTOR, 1.0, 1.5, *CONDUCTORS["furnace"]), True, 0.9),
    ("dielectric_ior1.5_r0.3_in", DIELECTRIC, material_record(DIELECTRIC, roughness=0.3, ior=1.5), True, 0.7),
    ("dielectric_ior1.5_r0.3_out", DIELECTRIC, material_record(DIELECTRIC, roughness=0.3, ior=1.5), False, 0.8),
    ("dielectric_ior1.33_r0.6_in", DIELECTRIC, material_record(DIELECTRIC, roughness=0.6, ior=1.33), True, 0.4),
]


def chi2_probes(material, entering, cos_i, count=CHI2_SAMPLES, seed=0):
    """count copies of one incoming direction under the +z normal, keys on the hashed path (sample >= the PMJ table)."""
    wi = _local_dir(cos_i, 0.7)
    p = np.zeros((count, 24), F32)
    p[:, :8] = material
    p[:, 10] = 1.0
    p[:, 11:14] = -wi
    p[:, 14] = 1.0 if entering else 0.0
    i = np.arange(count, dtype=np.uint64)
    p[:, 19] = ((i % 1024) + 1024 * seed).astype(np.uint32).view(F32)
    p[:, 20] = (PMJ_SAMPLES + i // 1024).astype(np.uint32).view(F32)
    p[:, 21] = np.zeros(count, np.uint32).view(F32)
    return p
