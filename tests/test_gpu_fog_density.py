"""The density grid of the fog volume on the device against the float64 reference of fog_density_reference.py (sorted plane crossings,
voxels from midpoints), on the cases of fog_density_cases.py.

* the voxel march (rt_fog_density_segments): clip and hashed pair bit for bit with rt_fog_segments; density length, distance, weights and vertex within
  bounds derived from the float32 roundings (fog_density_cases.py and beside the bounds here; nothing is a measured number); step counts on unambiguous rays;
  the brick table against numpy;
* the ..._grid attenuation pass and the ..._fog_grid sort launch under both schedulers;
* identities, bit for bit, on the 64 x 64 Cornell box under both schedulers;
* frames against closed forms: an absorbing slab stack, the white furnace over a sparse grid, a light shaft through a grid dense in one half;
* refusals.
Every test prints what it measured."""
import math

import numpy as np
import pytest

import fog_cases as cases
import fog_density_cases as dcases
import fog_density_reference as dref
import fog_reference as ref
from fog_cases import FURNACE_BOUNCES, FURNACE_SIGMA
from fog_density_cases import EPS, Rendering

pytestmark = pytest.mark.gpu

RT_ERROR_INVALID_ARG, RT_ERROR_NOT_READY = -1, -4
BOX_MIN, BOX_MAX = cases.BOX_MIN, cases.BOX_MAX
FACE = 2.5 * EPS       # a face distance (b - o) / d: a difference and a quotient (test_gpu_fog.py)
DISTANCE = 3.5 * EPS   # logf (1 ulp), the quotient by sigma_t


@pytest.fixture(scope="module")
def probing(grt):
    """A 64 x 64 Cornell context (the segment step needs the frame size and the RNG tables for its path numbers)."""
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=4))
    yield r
    r.grt.set_fog_density(r.pt.ctx, None)
    r.close()


# ---- 1. the march ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dcases.GRID_NAMES)
def test_the_march_matches_float64(grt, probing, name):
    """Every segment on every volume. A grid with a voxel of 1e6 is marched twice: as it is -- every assertion holds, but beside such a voxel the bound of D is of
    the order of d* itself and most comparisons count as ties -- and without the outlier (fog_density_cases.tame), where the ties must be few."""
    grid = dcases.grid(name)
    counts, worst = _march_against_float64(grt, probing, name, grid)
    print("%s: %s; worst error as a fraction of its bound: %s" % (name, counts, worst))
    if grid.max() > 3.0:
        counts, worst = _march_against_float64(grt, probing, name, dcases.tame(grid))
        print("%s without its outlier: %s; worst error as a fraction of its bound: %s" % (name, counts, worst))
    assert counts["clipped"] > 400 and counts["ties"] < counts["clipped"] // 8
    if name != "64x64x64":
        assert counts["scattered"] > 10
    else:
        assert counts["scattered"] > 0   # (segments along x = 0, y = 0.5 cross the one brick)
    if name not in ("1x1x1",):
        assert counts["empty"] > 0   # rays through density 0 only


def _march_against_float64(grt, probing, name, grid):
    probing.density(grid)
    ctx = probing.pt.ctx
    names, o, d, t_end, px, b, s = dcases.segment_probes(name)
    n = len(names)
    throughputs = np.array([cases.THROUGHPUTS[i % len(cases.THROUGHPUTS)] for i in range(n)], np.float32)
    flagged = (np.arange(n) % 11 == 10).astype(np.uint32)
    probes = grt.fog_segment_probes(o, d, t_end, px, b, s, throughputs, flagged)
    worst = dict(D=0.0, distance=0.0, weight=0.0, vertex=0.0)
    counts = dict(clipped=0, scattered=0, ties=0, empty=0)
    for volume, (sigma_a, sigma_s, g) in cases.VOLUMES.items():
        probing.fog(BOX_MIN, BOX_MAX, sigma_a, sigma_s, g)
        homogeneous = grt.fog_segments(ctx, probes)
        out = grt.fog_density_segments(ctx, probes)
        f = out.view(np.float32)
        assert np.array_equal(out[:, 0:4], homogeneous[:, 0:4]), (name, volume)   # the clip and the pair: bit for bit with the homogeneous step
        sa32, ss32 = np.array(sigma_a, np.float32), np.array(sigma_s, np.float32)
        st = sa32.astype(np.float64) + ss32.astype(np.float64)
        for i in range(n):
            what = "%s %s %s path %s" % (name, volume, names[i], (int(px[i]), int(b[i]), int(s[i])))
            t0, t1 = float(f[i, 0]), float(f[i, 1])
            if flagged[i] or not t1 > t0:   # inside a dielectric's medium, or outside the box: untouched
                assert t0 == 0.0 and t1 == 0.0 and out[i, 4] == 0 and np.array_equal(out[i, 6:9], probes[i, 10:13]) and not out[i, 12:15].any(), what
                continue
            counts["clipped"] += 1
            rand = (f[i, 2], f[i, 3])
            pieces = dref.intervals(BOX_MIN, BOX_MAX, grid, o[i], d[i], t0, t1)   # (over the device's own interval: the clip is rt_fog_segments', tested there)
            D = sum(rho * (bb - aa) for aa, bb, rho, _, _ in pieces if rho > 0)
            bound, a_max = dcases.density_length_bound(BOX_MIN, BOX_MAX, grid, o[i], d[i], t0, t1, D, len(pieces))
            assert out[i, 13] + out[i, 14] <= sum(grid.shape) + 3 and out[i, 13] + out[i, 14] >= 1, what
            target = dref.sample_target(sa32, ss32, rand, throughputs[i])
            target_error = DISTANCE * target if math.isfinite(target) else 0.0
            if math.isfinite(target) and abs(target - D) <= bound + target_error:   # the comparison D > d* may fall either way
                counts["ties"] += 1
                continue
            did = target < D
            assert bool(out[i, 4]) == did, (what, target, D, bound)
            got = f[i, 6:9].astype(np.float64)
            if not did:
                got_D = float(f[i, 12])
                assert abs(got_D - D) <= bound + 1e-45, (what, got_D, D, bound)
                assert f[i, 5] == np.inf and not out[i, 9:12].any(), what
                if bound > 0:
                    worst["D"] = max(worst["D"], abs(got_D - D) / bound)
                if D == 0.0 and got_D == 0.0:   # no density met: the path is left untouched
                    counts["empty"] += 1
                    assert np.array_equal(out[i, 6:9], probes[i, 10:13]), what
                    continue
            length, length_error = (target, target_error) if did else (D, bound)
            _, _, weight = ref.sample_distance(sa32, ss32, rand, D, throughputs[i])
            # the weights: test_gpu_fog.py's derivation with the density length for the length -- a channel's transmittance exp(-x), x = sigma_t * length, is off by
            # 2 EPS + sigma_t * length_error + 2 EPS x, twice (numerator and denominator), and 16 EPS for the products and quotients around it. A transmittance below
            # float32's normal range (1.2e-38) is rounded absolutely, not relatively; the factor beside it is below 1e8 for these volumes: 1e-30 absolute.
            T_error = 2.0 * EPS + st * length_error + st * length * 2.0 * EPS
            weight_bound = 2.0 * T_error.max() + 16.0 * EPS
            assert np.all(np.abs(got - weight) <= weight_bound * np.abs(weight) + 1e-30), (what, got, weight, weight_bound)
            if np.any(weight > 1e-20):
                worst["weight"] = max(worst["weight"], float((np.abs(got - weight)[weight > 1e-20] / (weight_bound * weight[weight > 1e-20])).max()))
            if not did:
                continue
            counts["scattered"] += 1
            assert abs(f[i, 5] - target) <= target_error, (what, f[i, 5], target)
            worst["distance"] = max(worst["distance"], abs(f[i, 5] - target) / target_error)
            assert abs(float(f[i, 12]) - target) <= bound + target_error + 2.0 * EPS * target, (what, f[i, 12], target)   # the density length up to the vertex is d*
            t, before, piece = dref.invert(pieces, target)
            aa, bb, rho = piece[:3]
            if min(abs(target - before), abs(before + rho * (bb - aa) - target)) <= bound + target_error:   # d* at a voxel's end: the vertex may lie in either voxel
                counts["ties"] += 1
                continue
            # the vertex. t_s = t_v + (d* - D_v) / rho: the voxel's entry t_v is a crossing (a_max), D_v carries the bound, d* its own error, the quotient and the sum
            # one rounding each; t_s and the reference's t both lie in the voxel's interval, the device's within a_max of [a, b] at either end.
            t_error = min(a_max + (bound + target_error) / rho + 2.0 * EPS * abs(t), (bb - aa) + 2.0 * a_max)
            vertex = o[i].astype(np.float64) + t * d[i].astype(np.float64)
            vertex_bound = np.abs(d[i]) * t_error + EPS * np.abs(t * d[i]) + EPS * (np.abs(o[i]) + np.abs(t * d[i]))
            assert np.all(np.abs(f[i, 9:12] - vertex) <= vertex_bound * 1.0000001), (what, f[i, 9:12], vertex, vertex_bound)
            if np.any(vertex_bound > 0):
                worst["vertex"] = max(worst["vertex"], float((np.abs(f[i, 9:12] - vertex)[vertex_bound > 0] / vertex_bound[vertex_bound > 0]).max()))
    return counts, worst


def _row_steps(grid, axis, j, k):
    """(voxel steps, brick steps, sum of the row) of an axis-parallel ray through the cell centres of row (j, k): x rows are (y, z) = (j, k), z rows (x, y) = (j, k)."""
    nz, ny, nx = grid.shape
    row = grid[k, j, :] if axis == 0 else grid[:, k, j]
    voxels = bricks = 0
    for first in range(0, row.size, 8):
        if axis == 0:
            brick = grid[k // 8 * 8:k // 8 * 8 + 8, j // 8 * 8:j // 8 * 8 + 8, first:first + 8]
        else:
            brick = grid[first:first + 8, k // 8 * 8:k // 8 * 8 + 8, j // 8 * 8:j // 8 * 8 + 8]
        if (brick > 0).any():
            voxels += min(8, row.size - first)
        else:
            bricks += 1
    return voxels, bricks, float(row.astype(np.float64).sum())


@pytest.mark.parametrize("name", ["5x4x3", "8x8x8", "9x8x8", "8x8x9", "17x5x9", "64x64x64"])
def test_step_counts_on_axis_parallel_rays_and_the_brick_table(grt, probing, name):
    """Rays along +x and along -z through cell centres, under the absorbing volume (no scatter event ends the march): the steps are unambiguous -- every voxel of a
    brick with density, one step per brick without -- and the density length is the row's sum times the cell. The brick table's counts are numpy's."""
    grid = dcases.grid(name)
    nx, ny, nz = dcases.dims(name)
    c = dcases.cell(name)
    sigma_a, sigma_s, g = cases.VOLUMES["absorbing"]
    probing.fog(BOX_MIN, BOX_MAX, sigma_a, sigma_s, g)
    probing.density(grid)
    info = grt.get_fog_density_info(probing.pt.ctx)
    total, empty = dref.bricks(grid)
    assert info == dict(dims=(nx, ny, nz), bricks=total, empty_bricks=empty, max_density=float(grid.max())), info
    rows = []
    rng = np.random.default_rng(7)
    for _ in range(24):
        j, k = int(rng.integers(0, ny)), int(rng.integers(0, nz))
        rows.append((0, j, k, (-3.0, BOX_MIN[1] + (j + 0.5) * c[1], BOX_MIN[2] + (k + 0.5) * c[2]), (1.0, 0.0, 0.0)))
        j, k = int(rng.integers(0, nx)), int(rng.integers(0, ny))
        rows.append((2, j, k, (BOX_MIN[0] + (j + 0.5) * c[0], BOX_MIN[1] + (k + 0.5) * c[1], 7.0), (0.0, 0.0, -1.0)))
    if name == "64x64x64":   # through the one brick with density, and past it
        bx, by, bz = dcases.ONE_BRICK
        rows.append((0, by * 8 + 3, bz * 8 + 5, (-3.0, BOX_MIN[1] + (by * 8 + 3.5) * c[1], BOX_MIN[2] + (bz * 8 + 5.5) * c[2]), (1.0, 0.0, 0.0)))
        rows.append((0, 1, 1, (-3.0, BOX_MIN[1] + 1.5 * c[1], BOX_MIN[2] + 1.5 * c[2]), (1.0, 0.0, 0.0)))
    o = np.array([r[3] for r in rows], np.float32); d = np.array([r[4] for r in rows], np.float32)
    out = grt.fog_density_segments(probing.pt.ctx, grt.fog_segment_probes(o, d, np.inf, 0, 0, 0, (1.0, 1.0, 1.0)))
    f = out.view(np.float32)
    seen = set()
    for i, (axis, j, k, _, _) in enumerate(rows):
        voxels, bricks_, total_density = _row_steps(grid, axis, j, k)
        assert (int(out[i, 13]), int(out[i, 14])) == (voxels, bricks_), (name, rows[i], out[i, 13:15], voxels, bricks_)
        D = total_density * c[axis]
        pieces = (nx, ny, nz)[axis]
        bound, _ = dcases.density_length_bound(BOX_MIN, BOX_MAX, grid, o[i], d[i], float(f[i, 0]), float(f[i, 1]), D, pieces)
        assert abs(f[i, 12] - D) <= bound, (name, rows[i], f[i, 12], D, bound)
        seen.add((voxels > 0, bricks_ > 0))
    print("%s: %d bricks, %d empty; %d axis-parallel rays, steps as counted by numpy" % (name, total, empty, len(rows)))
    if name == "64x64x64":
        assert (int(out[-1, 13]), int(out[-1, 14])) == (0, 8) and (int(out[-2, 13]), int(out[-2, 14])) == (8, 7)   # a ray that misses the one brick reads no voxel
        assert f[-1, 12] == 0.0 and f[-2, 12] > 0.0


def test_probe_contract(grt, probing):
    lib, ctx = probing.lib, probing.pt.ctx
    one = grt.fog_segment_probes([(0, 0.5, 0)], [(0, 0, 1)], [np.inf], [0], [0], [0], [(1, 1, 1)])
    out = np.zeros((1, 16), np.uint32)
    probing.fog(BOX_MIN, BOX_MAX, 0.1, 0.2)
    assert grt.set_fog_density(ctx, None) == 0 and grt.get_fog_density_info(ctx) is None
    assert lib.rt_fog_density_segments(ctx, one.ctypes.data, 1, out.ctypes.data) == RT_ERROR_NOT_READY
    assert b"no density grid" in lib.rt_last_error(ctx)
    probing.density(dcases.grid("5x4x3"))
    assert grt.set_fog_volume(ctx, None) == 0
    assert grt.get_fog_density_info(ctx)["dims"] == (5, 4, 3)   # state of its own: it survives the volume
    assert lib.rt_fog_density_segments(ctx, one.ctypes.data, 1, out.ctypes.data) == RT_ERROR_NOT_READY
    assert b"no fog volume" in lib.rt_last_error(ctx)
    probing.fog(BOX_MIN, BOX_MAX, 0.1, 0.2)
    bad = one.copy(); bad[0, 8] = 128
    assert lib.rt_fog_density_segments(ctx, bad.ctypes.data, 1, out.ctypes.data) == RT_ERROR_INVALID_ARG
    assert b"bounce" in lib.rt_last_error(ctx)
    assert grt.fog_density_segments(ctx, np.zeros((0, 16), np.uint32)).shape == (0, 16)
    # rt_fog_segments stays the homogeneous step: the same records with and without the grid
    with_grid = grt.fog_segments(ctx, one)
    assert grt.set_fog_density(ctx, None) == 0
    assert np.array_equal(grt.fog_segments(ctx, one), with_grid)


# ---- 2. the attenuation pass -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_attenuation_pass(grt, probing, scheduler):
    """The ..._grid attenuation kernels on queues of 0 .. 1 000 rays: illumination x exp(-sigma_t D) against float64, every other word bit for bit. The grid is
    17 x 5 x 9 without its 1e6 outlier (beside a value of 1e6 the bound of D says nothing). The ends of the interval are the float64 clip's here: each is off by
    FACE x the largest face distance (test_gpu_fog.py), which density_length_bound takes as clip_error."""
    sigma_a, sigma_s, g = cases.VOLUMES["unequal"]
    grid = dcases.tame(dcases.grid("17x5x9"))
    probing.fog(BOX_MIN, BOX_MAX, sigma_a, sigma_s, g)
    probing.density(grid)
    grt.set_scheduler(probing.pt.ctx, scheduler)
    try:
        st32 = np.array(sigma_a, np.float32).astype(np.float64) + np.array(sigma_s, np.float32).astype(np.float64)
        for count in (0, 1, 63, 64, 65, 1000):
            q = cases.shadow_queue(count, seed=100 + count)
            out = grt.attenuate_shadow_rays(probing.pt.ctx, q)
            assert out.shape == q.shape
            keep = [0, 1, 2, 3, 4, 5, 6, 10]
            assert np.array_equal(out[:, keep], q[:, keep]), (scheduler, count)   # every other word: bit for bit
            f, fo = q.view(np.float32), out.view(np.float32)
            dimmed = untouched = 0; worst = 0.0
            for i in range(count):
                o, d, md = f[i, 0:3], f[i, 3:6], f[i, 6]
                c = ref.clip(BOX_MIN, BOX_MAX, o, d, md)
                faces = [abs((float(bd[k]) - float(o[k])) / float(d[k])) for bd in (BOX_MIN, BOX_MAX) for k in range(3) if d[k] != 0]
                faces = [t for t in faces if math.isfinite(t)]
                t_error = FACE * max(faces) if faces else 0.0
                if c is None:   # outside the box in float64: the device may still see a graze as long as the two ends' errors
                    D, D_error = 0.0, 2.0 * t_error * float(grid.max())
                    untouched += int(np.array_equal(out[i], q[i]))   # (a ray outside the box is not stored)
                else:
                    pieces = dref.intervals(BOX_MIN, BOX_MAX, grid, o, d, c[0], c[1])
                    D = sum(rho * (bb - aa) for aa, bb, rho, _, _ in pieces if rho > 0)
                    D_error, _ = dcases.density_length_bound(BOX_MIN, BOX_MAX, grid, o, d, c[0], c[1], D, len(pieces), clip_error=t_error)
                x = st32 * D
                want = f[i, 7:10].astype(np.float64) * np.exp(-x)
                # exp(-x): x = sigma_t (a rounded sum) * D (its error above), a rounded product; expf 1 ulp; the product with the illumination one rounding
                bound = 3.0 * EPS + st32 * D_error + x * 2.0 * EPS
                assert np.all(np.abs(fo[i, 7:10] - want) <= bound * want), (scheduler, count, i, fo[i, 7:10], want, bound)
                if D > 1e-3:
                    dimmed += 1
                    worst = max(worst, float((np.abs(fo[i, 7:10] - want) / (bound * want)).max()))
                    assert np.all(fo[i, 7:10] < f[i, 7:10]), (scheduler, count, i)
            print("%s, %d rays: %d dimmed, %d outside the box, worst error %.3f of its bound" % (scheduler, count, dimmed, untouched, worst))
            if count >= 63:
                assert dimmed > count // 5 and untouched > 3
    finally:
        grt.set_scheduler(probing.pt.ctx, "merged")


# ---- 3. the sort launch ------------------------------------------------------------------------------------------------------------

SENTINEL = 0xFFC0DE42
FLAG_ALLOW_NEE, FLAG_INSIDE_MEDIUM, SHADOW_BOUNCE_0 = 1 << 31, 1 << 30, 1 << 30


@pytest.mark.parametrize("count", [256, 1025])
@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_sort_launch_marches_the_grid(grt, probing, scheduler, count):
    """Missed rays of bounce 0 through the ..._fog_grid sort instance, entry by entry against the segment probe -- the same device functions, so vertex and
    throughput agree bit for bit; every scattered entry goes on from its vertex, its light sample starts at that vertex; counters, statistics and sentinel
    words as the launch must leave them (the homogeneous launch's test, test_gpu_fog.py, checks the light samples themselves)."""
    sigma_a, sigma_s, g = cases.VOLUMES["unequal"]
    probing.fog(BOX_MIN, BOX_MAX, sigma_a, sigma_s, g)
    probing.density(dcases.tame(dcases.grid("17x5x9")))
    ctx = probing.pt.ctx
    sample = 5
    q = cases.shadow_queue(count, seed=300 + count).view(np.float32)
    o, d = q[:, 0:3].copy(), q[:, 3:6].copy()
    pixels = np.arange(count, dtype=np.uint32)
    frame_pixels = probing.pt.pitch * 64
    probes = grt.fog_segment_probes(o, d, np.full(count, np.inf, np.float32), pixels, 0, sample, np.ones((count, 3), np.float32))
    seg = grt.fog_density_segments(ctx, probes)
    homogeneous = grt.fog_segments(ctx, probes)
    scattered = seg[:, 4] == 1
    assert not np.array_equal(seg[:, 4:12], homogeneous[:, 4:12])   # the grid does change the outcome
    entries = np.zeros((count, 20), np.uint32); f = entries.view(np.float32)
    f[:, 0:3] = o; f[:, 3:6] = d
    entries[:, 6] = 0; entries[:, 7] = 0xFFFFFFFF; f[:, 8] = np.inf   # a miss
    entries[:, 10] = pixels
    f[:, 11:14] = 0.25   # (bounce 0: the kernel takes 1, not what the queue carries)
    kwargs = dict(capacity=count + 9, sentinel=SENTINEL)
    if scheduler == "merged":
        births = np.zeros(128, np.int32); births[0] = 7
        kwargs.update(iteration=7, slot_table=np.array([[sample, 7, 0, 0]], np.int32), submission_birth=births)
    else:
        kwargs.update(bounce=0, sample_index=sample)
    r = grt.sort_rays_fog(ctx, entries, frame_pixels, 1, **kwargs)
    n = int(scattered.sum())
    assert n > count // 10
    assert list(r.counters) == [0, 0, 0, 0, n, count], (list(r.counters), n)
    out = r.trace_out
    assert np.all(out[n:] == SENTINEL) and np.all(out[:n, 6:10] == SENTINEL) and np.all(out[:n, 15] == SENTINEL) and np.all(out[:n, 18:20] == SENTINEL)   # untouched words
    assert np.all(r.material_out == SENTINEL)
    px = out[:n, 10] & ~np.uint32(FLAG_ALLOW_NEE | FLAG_INSIDE_MEDIUM)
    assert sorted(px.tolist()) == pixels[scattered].tolist()   # every scattered entry once
    assert np.all(out[:n, 10] & FLAG_ALLOW_NEE) and not np.any(out[:n, 10] & FLAG_INSIDE_MEDIUM)
    assert np.array_equal(out[:n, 0:3], seg[px, 9:12]) and np.array_equal(out[:n, 11:14], seg[px, 6:9])   # vertex and throughput: the segment step, bit for bit
    m = r.shadow_count
    sh = r.shadow_out; fs = sh.view(np.float32)
    assert 0 < m <= n and np.all(sh[m:] == SENTINEL)
    word = sh[:m, 10]
    assert np.all((word & SHADOW_BOUNCE_0) != 0) if scheduler == "merged" else np.all((word & SHADOW_BOUNCE_0) == 0)
    spx = word & ~np.uint32(SHADOW_BOUNCE_0)
    assert len(set(spx.tolist())) == m and set(spx.tolist()) <= set(px.tolist())   # at most one per scattered entry
    assert np.array_equal(sh[:m, 0:3], seg[spx, 9:12])   # from the vertex itself
    assert np.allclose(np.linalg.norm(fs[:m, 3:6], axis=1), 1.0, atol=1e-5) and np.all(fs[:m, 6] > 0) and np.all(np.isfinite(fs[:m, 7:10])) and np.all(fs[:m, 7:10] >= 0)
    assert not r.aov[0][px].any() and np.all(np.isfinite(r.aov[0]))
    if scheduler == "merged":
        assert r.stats[0, 0, 0] == count and r.stats[0, 1, 0] == m and r.stats[0, 2:, 0].sum() == 0
    print("%s, %d entries: %d scattered (%d under the homogeneous step), %d light samples" % (scheduler, count, n, int((homogeneous[:, 4] == 1).sum()), m))


# ---- 4. identities ---------------------------------------------------------------------------------------------------------------

FOG_IN_ROOM = ((-0.5, 0.3, -0.5), (0.5, 1.5, 0.5), 0.2, 0.8, 0.3)   # inside the Cornell box's room


def _cornell(grt, scheduler, prepare=None, samples=(2, 3)):
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=4), scheduler)
    try:
        if prepare:
            prepare(r)
        first, frame = 0, None
        for count in samples:
            frame = r.render(count, first, batch=count); first += count
        c = r.pt.counters()
        return frame, [list(c.trace[:4]), list(c.shadow[:4]), list(c.diffuse[:4])]
    finally:
        r.close()


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_identities(grt, scheduler):
    never, never_counters = _cornell(grt, scheduler)
    homogeneous, homogeneous_counters = _cornell(grt, scheduler, lambda r: r.fog(*FOG_IN_ROOM))
    assert not np.array_equal(never, homogeneous)

    def one_cell(r):
        r.fog(*FOG_IN_ROOM); r.density(np.ones((1, 1, 1), np.float32))
    ones, ones_counters = _cornell(grt, scheduler, one_cell)
    assert np.array_equal(ones, homogeneous) and ones_counters == homogeneous_counters, scheduler   # the outer planes are the box faces: 1 x 1 x 1 of 1.0 is no grid

    grid = dcases.grid("5x4x3")
    box_min, box_max, sigma_a, sigma_s, g = FOG_IN_ROOM

    def plain(r):
        r.fog(box_min, box_max, sigma_a, sigma_s, g); r.density(grid)

    def doubled(r):
        r.fog(box_min, box_max, np.float32(sigma_a) / np.float32(2), np.float32(sigma_s) / np.float32(2), g); r.density(grid * np.float32(2))
    a, a_counters = _cornell(grt, scheduler, plain)
    b, b_counters = _cornell(grt, scheduler, doubled)
    assert np.array_equal(a, b) and a_counters == b_counters, scheduler   # rho scales sigma: twice the grid under half the sigmas
    assert not np.array_equal(a, homogeneous) and not np.array_equal(a, never)

    def zeros(r):
        r.fog(*FOG_IN_ROOM); r.density(np.zeros((3, 4, 5), np.float32))
        assert r.pt.ctx and r.grt.get_fog_density_info(r.pt.ctx)["empty_bricks"] == 1
    empty, empty_counters = _cornell(grt, scheduler, zeros)
    assert np.array_equal(empty, never) and empty_counters == never_counters, scheduler   # a grid of zeros renders as no volume

    def set_then_cleared(r):
        r.fog(*FOG_IN_ROOM); r.density(grid)
        set_then_cleared.lit = r.render(2)
        assert r.grt.set_fog_density(r.pt.ctx, None) == 0 and r.grt.get_fog_density_info(r.pt.ctx) is None
    again, again_counters = _cornell(grt, scheduler, set_then_cleared)
    assert np.array_equal(again, homogeneous) and again_counters == homogeneous_counters, scheduler   # clearing the grid gives back the homogeneous frame
    assert np.isfinite(set_then_cleared.lit).all()
    print("%s: 1x1x1 of 1.0 = no grid; 2 x grid under sigma / 2 = grid; zeros = no volume; cleared = homogeneous. Means: none %.4f, homogeneous %.4f, 5x4x3 %.4f" %
          (scheduler, never[..., :3].mean(), homogeneous[..., :3].mean(), a[..., :3].mean()))


# ---- 5. frames against closed forms ---------------------------------------------------------------------------------------------

STACK = np.array([0.0, 1e-30, 1.0, 2.5, 0.0, 0.6, 0.25], np.float32)


@pytest.mark.parametrize("scheduler", ["merged", "slots"])
def test_an_absorbing_slab_stack_dims_the_emitter(grt, scheduler):
    """test_gpu_fog.py's absorption test through a 1 x 1 x 7 stack: a pixel that shows the Cornell box's light through the box shows its radiance times
    exp(-sigma_a x sum of rho_i x the length inside slab i), the lengths from the pixel's own primary ray (rt_generate_rays) cut at the slabs in float64. Deterministic."""
    sigma_a = np.array([0.9, 0.4, 0.1], np.float32)
    box_min, box_max = np.array([-0.5, 1.3, 2.0], np.float32), np.array([0.5, 1.62, 4.0], np.float32)
    grid = STACK.reshape(7, 1, 1)
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=1), scheduler, sky=0.0)
    try:
        o, d, px = grt.generate_rays(r.pt.ctx, 0, 0, 64 * 64)
        clear = r.render(1, 0, 1)[..., :3].astype(np.float64)
        r.fog(box_min, box_max, sigma_a, 0.0); r.density(grid)
        dimmed = r.render(1, 0, 1)[..., :3].astype(np.float64)
        lit = clear.sum(axis=2) > 0
        assert lit.sum() > 20, lit.sum()
        through = 0; worst = 0.0
        for i in range(64 * 64):
            x, y = int(px[i]) % r.pt.pitch, int(px[i]) // r.pt.pitch
            if not lit[y, x]:
                assert not dimmed[y, x].any()
                continue
            oi, di = o[:, i], d[:, i]
            c = ref.clip(box_min, box_max, oi, di, np.inf)
            D = D_error = 0.0
            if c is not None:
                faces = [abs((float(bd[k]) - float(oi[k])) / float(di[k])) for bd in (box_min, box_max) for k in range(3) if di[k] != 0]
                pieces = dref.intervals(box_min, box_max, grid, oi, di, c[0], c[1])
                D = sum(rho * (bb - aa) for aa, bb, rho, _, _ in pieces if rho > 0)
                D_error, _ = dcases.density_length_bound(box_min, box_max, grid, oi, di, c[0], c[1], D, len(pieces), clip_error=FACE * max(faces))
            xs = sigma_a.astype(np.float64) * D
            want = clear[y, x] * np.exp(-xs)
            bound = 4.0 * EPS + sigma_a * D_error + xs * 2.0 * EPS   # as in the attenuation pass, and one rounding for the frame's fold
            assert np.all(np.abs(dimmed[y, x] - want) <= bound * want), (scheduler, x, y, dimmed[y, x], want, bound)
            if D > 0:
                through += 1; worst = max(worst, float((np.abs(dimmed[y, x] - want) / (bound * want)).max()))
        print("%s: %d pixels show the emitter, %d of them through the stack; worst error %.3f of its bound" % (scheduler, lit.sum(), through, worst))
        assert through > 10
    finally:
        r.close()


def _sparse_grid():
    rng = np.random.default_rng(41)
    g = rng.uniform(0.25, 1.0, (12, 10, 9)).astype(np.float32)   # values <= 1: no voxel denser than the homogeneous furnace
    g[rng.random(g.shape) < 0.6] = 0.0
    g[:, :, 0:2] = 0.0
    return g


@pytest.mark.parametrize("g", [0.0, 0.8])
def test_white_furnace_over_a_sparse_grid(grt, tmp_path, g):
    """test_gpu_fog.py's furnace over a seeded sparse grid (9 x 10 x 12, 60 % of it empty, values <= 1): a sky of radiance 1, no absorption, NEE off -- every
    sample is 1 unless the bounce limit cuts its path. The allowances, derived as there:
    * truncation: no segment's density length exceeds the diagonal x 1, so a segment scatters with probability at most 1 - exp(-sigma x diagonal): the
      homogeneous bound holds;
    * a segment's weight: the march's steps add nothing to it. The density length enters a weight only through the transmittance T = exp(-sigma_t D), one float
      that stands in numerator and denominator alike (sigma_a = 0, a grey throughput), so whatever error the march left in D cancels with T itself: 8 EPS
      per segment as in the homogeneous furnace, and exactly 0 for a segment that met no density (the path is left untouched);
    * the fold into the pixel's mean: EPS (N / 2 + 1)."""
    truncation = ref.furnace_truncation_bound(BOX_MIN, BOX_MAX, FURNACE_SIGMA, FURNACE_BOUNCES)
    assert truncation < 1e-6
    grid = _sparse_grid()
    assert grid.max() <= 1.0
    samples = 64
    fold = EPS * (samples / 2 + 1)
    rounding = (FURNACE_BOUNCES + 1) * 8.0 * EPS + fold
    for scheduler in ("merged", "slots"):
        r = Rendering(grt, cases.write_empty_scene(tmp_path), 16, 16, dict(num_bounces=FURNACE_BOUNCES, enable_next_event_estimation=0, enable_russian_roulette=0), scheduler, sky=1.0)
        try:
            r.fog(BOX_MIN, BOX_MAX, 0.0, FURNACE_SIGMA * 4.0, g); r.density(grid * np.float32(0.25))   # (rho sigma <= FURNACE_SIGMA everywhere)
            rays = paths = scatters = 0
            for first in range(0, samples, 16):
                frame = r.render(16, first)[..., :3].astype(np.float64)
                c = r.pt.counters()
                rays += sum(c.trace[:FURNACE_BOUNCES]); paths += c.trace[0]; scatters += c.trace[1]
            assert paths == 16 * 16 * samples
            mean_rounding = 8.0 * EPS * rays / paths + fold
            print("g = %g, %s: pixel means in [%.9f, %.9f], frame mean %.9f; %.3f segments per path; allowed: truncation %.3g, rounding %.3g per pixel and %.3g in the mean" %
                  (g, scheduler, frame.min(), frame.max(), frame.mean(), rays / paths, truncation, rounding, mean_rounding))
            assert frame.max() <= 1.0 + rounding
            assert abs(frame.mean() - 1.0) <= mean_rounding + truncation
            assert scatters > 0
        finally:
            r.close()


def test_light_shaft_through_a_grid_dense_in_one_half(grt, tmp_path):
    """test_gpu_fog.py's light shaft with a 2 x 1 x 1 grid over the box (thin for x < 0, dense for x > 0): one point light above the box, a black sky, paths of
    exactly one scattering event, a box filter. Each pixel's mean lies within 5 standard errors of the quadrature of the single-scatter integral over its rays
    (a 2 x 2 grid of its footprint; fog_density_reference.shaft_quadrature_halves), the standard error from the float64 Monte Carlo of the same estimator."""
    w = h = 16
    samples = cases.SHAFT["samples"]
    rho = dcases.SHAFT_HALVES
    r = Rendering(grt, cases.write_empty_scene(tmp_path, "shaft", emitter_xml=cases.shaft_emitter()), w, h,
                  dict(num_bounces=2, reconstruction_filter=0, delta_lights=1), "merged", sky=0.0)
    try:
        assert r.scene.delta_lights().shape[0] == 1
        r.fog(BOX_MIN, BOX_MAX, cases.SHAFT["sigma_a"], cases.SHAFT["sigma_s"], cases.SHAFT["g"])
        r.density(np.array(rho, np.float32).reshape(1, 1, 2))
        frame = r.render(samples)[..., 0].astype(np.float64)
        c = r.pt.camera()
        camera = {k: np.array(list(getattr(c, k)), np.float64) for k in ("position", "bottom_left_corner", "x_axis", "y_axis")}
        a = dict(box_min=BOX_MIN, box_max=BOX_MAX, rho=rho, sigma_a=cases.SHAFT["sigma_a"], sigma_s=cases.SHAFT["sigma_s"], g=cases.SHAFT["g"], light=cases.SHAFT_LIGHT, intensity=cases.SHAFT_INTENSITY)
        want = np.zeros(w * h)
        for jx in (0.25, 0.75):
            for jy in (0.25, 0.75):
                dirs = ref.pixel_rays(camera, w, h, (jx, jy))
                want += np.array([dref.shaft_quadrature_halves(o=camera["position"], d=dirs[k], **a) for k in range(w * h)]) / 4.0
        rng = np.random.default_rng(7)
        n = 1024
        dirs = ref.pixel_rays(camera, w, h, rng.random((n * w * h, 2)), repeat=n)
        values = dref.shaft_monte_carlo_halves(o=np.broadcast_to(camera["position"], dirs.shape), d=dirs, rng=rng, **a).reshape(n, w * h)
        error = (values.std(axis=0, ddof=1) / math.sqrt(samples)).reshape(h, w)
        want = want.reshape(h, w)
        deviation = np.abs(frame - want) / error
        print("shaft through halves %s: radiance %.4g .. %.4g (left half %.4g, right half %.4g on the device), standard error %.3g .. %.3g, worst deviation %.2f standard errors, mean %.2f" %
              (rho, want.min(), want.max(), frame[:, :w // 2].mean(), frame[:, w // 2:].mean(), error.min(), error.max(), deviation.max(), deviation.mean()))
        halves = sorted([frame[:, :w // 2].mean(), frame[:, w // 2:].mean()])
        assert want.min() > 0 and halves[1] > 1.5 * halves[0]   # the dense half shines
        assert (deviation > 5.0).sum() == 0, np.argwhere(deviation > 5.0)   # (256 pixels at 5 sigma: 1.5e-4 expected failures)
    finally:
        r.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(grt, probing):
    lib, ctx = probing.lib, probing.pt.ctx
    good = dcases.grid("5x4x3")
    probing.fog(BOX_MIN, BOX_MAX, 0.1, 0.2)
    probing.density(good)
    before = grt.get_fog_density_info(ctx)
    probe = grt.fog_segment_probes([(0, 0.5, 0)], [(0.1, 0.05, 1)], [np.inf], [3], [0], [0], [(1, 1, 1)])
    record = grt.fog_density_segments(ctx, probe)
    bad = []
    for value in (np.nan, np.inf, -np.inf, -1e-30, -1.0):
        v = good.copy(); v[2, 1, 3] = value
        bad.append((v, b"cell (3, 1, 2)"))
    bad.append((np.zeros((1, 1, 1025), np.float32), b"nx"))
    bad.append((np.zeros((1025, 1, 1), np.float32), b"nz"))
    for v, word in bad:
        assert grt.set_fog_density(ctx, v) == RT_ERROR_INVALID_ARG
        message = lib.rt_last_error(ctx)
        assert b"rt_set_fog_density" in message and word in message, message
        assert grt.get_fog_density_info(ctx) == before and np.array_equal(grt.fog_density_segments(ctx, probe), record)   # the grid before it is still in force
    v = np.zeros(1, np.float32)
    for dims_ in ((0, 1, 1), (1, -1, 1), (1, 1, 0)):
        assert lib.rt_set_fog_density(ctx, v.ctypes.data, *dims_) == RT_ERROR_INVALID_ARG
        assert grt.get_fog_density_info(ctx) == before
    print("refused: %d invalid grids, each leaving the one before in force" % (len(bad) + 3))
    # ... and with SVGF
    r = Rendering(grt, grt.scene_path("cornellbox"), 64, 64, dict(num_bounces=3, enable_svgf=1))
    try:
        r.fog(*FOG_IN_ROOM); r.density(good)
        assert r.lib.rt_render_samples(r.pt.ctx, 0, 1) == RT_ERROR_INVALID_ARG
        assert b"fog volume" in r.lib.rt_last_error(r.pt.ctx)
        r.density(np.zeros((1, 1, 1), np.float32))   # a grid of zeros: no volume is in force
        assert r.lib.rt_render_samples(r.pt.ctx, 0, 1) == 0
    finally:
        r.close()


def test_the_scene_uploads_its_grid_at_update(grt):
    """Scene.set_fog_density reaches the device at update() after invalidate("fog"), and leaves when it is cleared."""
    grt.config_reset()
    scene = grt.Scene(grt.scene_path("cornellbox"))
    pt = grt.Pathtracer(scene, 64, 64, device=0)
    try:
        pt.update()
        assert grt.get_fog_density_info(pt.ctx) is None
        scene.set_fog(*FOG_IN_ROOM); scene.set_fog_density(dcases.grid("9x8x8"))
        pt.invalidate("fog"); pt.update()
        info = grt.get_fog_density_info(pt.ctx)
        assert info["dims"] == (9, 8, 8) and (info["bricks"], info["empty_bricks"]) == (2, 1) and grt.get_fog_volume(pt.ctx) is not None
        pt.render()
        assert np.isfinite(pt.read_framebuffer()).all()
        scene.clear_fog_density()
        pt.invalidate("fog"); pt.update()
        assert grt.get_fog_density_info(pt.ctx) is None and grt.get_fog_volume(pt.ctx) is not None
    finally:
        pt.close(); scene.close(); grt.config_reset()
