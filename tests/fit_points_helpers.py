"""References for ndt_fit_points_batch{,_dev} (tests only): tests/test_fit_points_host.py and tests/test_gpu_fit_points.py.

ref_stats       ndt_fit_stats restated in numpy: math.fsum over the selected distances, one division, `<=` on the widened
                value.  Where the selected distances have an exact fp64 sum (fitness_workloads.sum_is_exact) this IS what
                the device must give, bit for bit, whatever its order of summation; elsewhere it is within n 2^-53.
narrow_pool     queries over a map whose non-zero distances lie in a window of binades narrow enough for an exact sum of n.
half_scene      the relocalisation scene of a map that covers only part of the scan.
ranged_best     the re-ranking rule of Map.relocalize(max_d2=...), restated.
"""
import math

import numpy as np

import fitness_workloads as W

F = np.float32
DBL_MAX = W.DBL_MAX
STATS_FIELDS = ("fitness", "fitness_all", "n_in", "n_dist", "n_points")
IDENT = (F(1.0), F(0.0), F(0.0), F(0.0))


def ref_stats(d, max_d2):
    """(fitness, fitness_all, n_in, n_dist, n_points) of one match whose float32 distances are d (inf or NaN: no distance)."""
    d = np.asarray(d, dtype=F).ravel()
    d64 = d.astype(np.float64)                              # widened BEFORE the comparison
    has = np.isfinite(d64)
    with np.errstate(invalid="ignore"):
        inn = has & (d64 <= float(max_d2))
    n_in, n_dist = int(inn.sum()), int(has.sum())
    fit = math.fsum(d64[inn].tolist()) / n_in if n_in else DBL_MAX
    fit_all = math.fsum(d64[has].tolist()) / n_dist if n_dist else DBL_MAX
    return fit, fit_all, n_in, n_dist, len(d)


def stats_tuple(s):
    """A FIT_STATS_DTYPE record as ref_stats' tuple (reserved must be 0)."""
    assert int(s["reserved"]) == 0
    return float(s["fitness"]), float(s["fitness_all"]), int(s["n_in"]), int(s["n_dist"]), int(s["n_points"])


def tf_of_pose(pose):
    """The four float32 (c, s, tx, ty) a test passes as `tf` for a pose (x, y, yaw)."""
    return (F(math.cos(pose[2])), F(math.sin(pose[2])), F(pose[0]), F(pose[1]))


def describe(w, q, want, got, what=""):
    """The first query whose device distance differs from brute force, with its voxel: what fitness_workloads.localise
    prints, without the bisection (every query is at hand)."""
    want, got = np.asarray(want, dtype=F), np.asarray(got, dtype=F)
    fin = np.isfinite(want)
    bad = np.flatnonzero(np.where(fin, want.view(np.uint32) != got.view(np.uint32), got != np.inf))
    if len(bad) == 0:
        return None
    i = int(bad[0])
    G = W.grid_of(w.map, w.leaf)
    v = np.nan_to_num(W.voxel_of(G, q[i:i + 1])[0], nan=-1.0, posinf=2.0 ** 31, neginf=-2.0 ** 31)
    return ("%s: %d of %d queries differ; first: point %d, query (%r, %r), voxel (%d, %d) of a %d x %d grid, cx & 7 = %d, cy & 7 = %d, "
            "leaf %r: brute force %r, device %r" % (what, len(bad), len(q), i, float(q[i, 0]), float(q[i, 1]), int(v[0]), int(v[1]),
                                                    G.div_x, G.div_y, int(np.clip(v[0], 0, G.div_x - 1)) & 7,
                                                    int(np.clip(v[1], 0, G.div_y - 1)) & 7, float(G.leaf), float(want[i]), float(got[i])))


def narrow_pool(w, n_each, seed=5):
    """One scan per entry of n_each over the map of workload w (disjoint slices of one pool of random queries in the grid's
    box, input order kept), every non-zero distance inside ONE window of max_binades(max(n_each)) binades that ends at
    64 leaf^2 -- as fitness_workloads.wave_scan draws them -- so that every scan's sum, and every subset's, is exact.
    -> (list of scans, list of their brute-force distances)."""
    rng = np.random.Generator(np.random.Philox(seed))
    G = W.grid_of(w.map, w.leaf)
    L = float(G.leaf)
    lo = np.array([G.min_bx, G.min_by]) * L
    hi = lo + np.array([G.div_x, G.div_y]) * L
    total = int(sum(n_each))
    pool = rng.uniform(lo - 2 * L, hi + 2 * L, size=(3 * total + 4096, 2)).astype(F)
    pool[::97] = w.map[(np.arange(len(pool[::97])) * 7) % len(w.map)]        # exact hits among them
    d = W.brute_sq(w.map, pool)
    room = W.max_binades(max(n_each))
    eL = int(np.frexp(L * L)[1])
    e = np.frexp(d.astype(np.float64))[1]
    ok = np.flatnonzero(np.isfinite(d) & ((d == 0) | ((e >= eL + 7 - room) & (e <= eL + 6))))
    assert len(ok) >= total, (len(ok), total)
    scans, ds, s = [], [], 0
    for n in n_each:
        sel = ok[s:s + n]; s += n
        scans.append(pool[sel]); ds.append(d[sel])
        assert W.sum_is_exact(ds[-1])
    return scans, ds


# ------------------------------------------------------------------------------------------ relocalisation in half a map
# (scan index, axis, side): the C1 map cut at the median of the scan's world coordinate `axis` at the true pose, keeping the
# side below (-1) or above (+1) it -- about half of the scan's points have no map near them at the truth.  Chosen on the CPU
# oracle (tests/test_fit_points_host.py asserts it): the unbounded mean ranks a wrong candidate first, the ranged one the truth.
HALF_SCENES = ((0, 0, -1), (5, 0, 1))


def half_scene(m, sf, k, axis, side):
    """-> (the cut map float32, scan, truth)."""
    scan, truth, _ = sf.make(k)
    c, s = math.cos(truth[2]), math.sin(truth[2])
    wx = c * scan[:, 0].astype(np.float64) - s * scan[:, 1] + truth[0]
    wy = s * scan[:, 0].astype(np.float64) + c * scan[:, 1] + truth[1]
    med = float(np.median((wx, wy)[axis]))
    keep = (m[:, axis] <= med) if side < 0 else (m[:, axis] >= med)
    return np.ascontiguousarray(m[keep]), scan, truth


def ranged_best(records, fitness, n_in):
    """Lowest `converged ? ranged fitness : 1e7`, ties to the higher n_in, then the lower index; -1 for no records."""
    keys = [((float(fitness[c]) if records[c]["converged"] else 1e7), -int(n_in[c]), c) for c in range(len(records))]
    return min(keys)[2] if keys else -1


def ranged_of_records(map_xy, scan, records, max_d2, sse):
    """(fitness, n_in) per record by brute force on the queries the record's own matrix gives."""
    fit, n_in = [], []
    for r in records:
        d = W.brute_sq(map_xy, W.queries_of(scan, (r["T00"], r["T10"], r["T03"], r["T13"]), sse))
        st = ref_stats(d, max_d2)
        fit.append(st[0]); n_in.append(st[2])
    return np.array(fit), np.array(n_in)
