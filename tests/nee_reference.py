"""Float64 numpy restatement of the shade kernels' light selection (sample_light, sample_triangle, nee_pick_light of
rt_lights.h; Sampling.h:180-190 and Pathtracer.cu:472-493 of the reference), and the exact selection probabilities.

The table search is `searchsorted(..., side="left")` within the span: the first entry >= u, which is what `binary_search`
returns whenever it returns (it returns `middle` only if u <= cdf[middle] and, unless middle is the span's first entry,
u > cdf[middle - 1]; in a table that never decreases that index is unique). Comparisons of a float32 u with float32 entries are
exact in float64, so the selection is not a matter of precision.
"""
import numpy as np


def luminance(rgb):
    rgb = np.asarray(rgb, np.float64)
    return 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]


class Tables:
    """The arrays light selection reads, as the oracle's scene view holds them (what the device is given)."""

    def __init__(self, view):
        k = view.keep
        self.triangle_indices = np.asarray(k["light_triangle_indices"], np.int32).reshape(-1)
        self.triangle_cdf = np.asarray(k["light_triangle_cumulative_probability"], np.float32).reshape(-1)
        self.mesh_cdf = np.asarray(k["light_mesh_cumulative_probability"], np.float32).reshape(-1)
        self.spans = np.asarray(k["light_mesh_triangle_span"], np.int32).reshape(-1, 2)
        self.transform_indices = np.asarray(k["light_mesh_transform_indices"], np.int32).reshape(-1)
        self.triangles = np.asarray(k["triangles"], np.float32).reshape(-1, 24)
        self.transforms = np.asarray(k["mesh_transforms"], np.float32).reshape(-1, 3, 4)
        self.material_ids = np.asarray(k["mesh_material_ids"], np.int32).reshape(-1)
        self.materials = np.asarray(k["materials"], np.float32).reshape(-1, 8)
        self.total_weight = float(view.scene.lights_total_weight)

    def emission(self, transform_id):
        return self.materials[self.material_ids[transform_id], :3].astype(np.float64)


def search(cdf, first, last, u):
    """The first index in [first, last] whose entry is >= u, per probe (first, last, u arrays)."""
    out = np.empty(u.size, np.int64)
    keys = first.astype(np.int64) * (1 << 32) + last.astype(np.int64)
    for key in np.unique(keys):
        sel = keys == key
        f, l = int(key >> 32), int(key & 0xffffffff)
        out[sel] = f + np.searchsorted(cdf[f:l + 1].astype(np.float64), u[sel].astype(np.float64), side="left")
        assert (out[sel] <= l).all(), "a search past the span's last entry: the table does not end in an entry >= u"
    return out


def sample_triangle(u1, u2):
    """Sampling.h: the unit square folded onto the triangle."""
    above = u2 > u1
    a = np.where(above, u1 * 0.5, u1 - u2 * 0.5)
    b = np.where(above, u2 - u1 * 0.5, u2 * 0.5)
    return a, b


class Picked:
    pass


def sample_lights(tables, probes):
    """The float64 result of rt_sample_lights on (N, 4) probes: entry, transform_id, triangle (exact), point, normal, emission."""
    p = np.asarray(probes, np.float32).reshape(-1, 4)
    u = p.astype(np.float64)
    n = p.shape[0]
    r = Picked()
    r.entry = search(tables.mesh_cdf, np.zeros(n, np.int64), np.full(n, tables.mesh_cdf.size - 1, np.int64), p[:, 0])
    r.transform_id = tables.transform_indices[r.entry].astype(np.int64)
    span = tables.spans[r.entry]
    r.slot = search(tables.triangle_cdf, span[:, 0], span[:, 1], p[:, 1])
    r.triangle = tables.triangle_indices[r.slot].astype(np.int64)
    a, b = sample_triangle(u[:, 2], u[:, 3])
    r.uv = np.stack([a, b], 1)
    tri = tables.triangles[r.triangle].astype(np.float64)
    p0, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    local = p0 + a[:, None] * e1 + b[:, None] * e2
    m = tables.transforms[r.transform_id].astype(np.float64)
    r.point = np.einsum("nij,nj->ni", m[:, :, :3], local) + m[:, :, 3]
    normal = np.einsum("nij,nj->ni", m[:, :, :3], np.cross(e1, e2))
    with np.errstate(invalid="ignore", divide="ignore"):
        r.normal = normal / np.linalg.norm(normal, axis=1)[:, None]   # NaN for a zero-area triangle, as on the device
    r.emission = np.stack([tables.emission(t) for t in r.transform_id]) if n else np.zeros((0, 3))
    return r


def exact_probabilities(tables):
    """From the geometry alone, not from the tables: P(entry) = luminance(emission) * area * scale^2 / W over the light-mesh entries
    (area: the object-space area of the entry's mesh data, scale: its instance's uniform scale), and per entry
    P(slot | entry) = area of the triangle / area of the mesh over its span of the triangle table. Returns (mesh_p, [slot_p per entry], W)."""
    slot_p, weight = [], []
    for m in range(tables.mesh_cdf.size):
        first, last = tables.spans[m]
        tri = tables.triangles[tables.triangle_indices[first:last + 1]].astype(np.float64)
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 3:6], tri[:, 6:9]), axis=1)
        t = tables.transform_indices[m]
        scale = np.linalg.norm(tables.transforms[t].astype(np.float64)[0, :3])
        slot_p.append(area / area.sum())
        weight.append(luminance(tables.emission(t)) * area.sum() * scale * scale)
    weight = np.array(weight)
    return weight / weight.sum(), slot_p, weight.sum()
