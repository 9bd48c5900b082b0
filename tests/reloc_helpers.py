"""References for relocalisation (ndt_score_*, ndt_lattice_select_dev, ndt_relocalize; tests only).

lattice_poses   the definition of a lattice's poses in numpy: x0 + i * step, one rounded multiply, one rounded add.
ref_select      the candidate pick as include/ndt_mi355x.h defines it, by sorting.
ref_best        the cost rule: converged ? fitness : 1e7, lowest first, ties to the lower index.
oracle_scores   score and pairs of a pose list on the CPU oracle (one eval_at per pose).
"""
import ctypes as C
import math

import numpy as np

# the lattice of the issue's prototype: the whole +-24 m world of configs[0] at 0.6 m, every yaw at 10 degrees
LAT = dict(x0=-24.0, y0=-24.0, yaw0=-math.pi, step_x=0.6, step_y=0.6, step_yaw=2.0 * math.pi / 36, nx=81, ny=81, nyaw=36)
NOT_CONVERGED_COST = 1e7           # src/PoseEstimator.cpp:43-46


def lattice_size(lat):
    return lat["nx"] * lat["ny"] * lat["nyaw"]


def lattice_ijk(lat, idx):
    idx = np.asarray(idx, dtype=np.int64)
    i = idx % lat["nx"]
    j = (idx // lat["nx"]) % lat["ny"]
    k = idx // (lat["nx"] * lat["ny"])
    return i, j, k


def lattice_poses(lat, idx=None):
    """[len, 3] float64: numpy's float64 product and sum round once each, as the library's definition does."""
    if idx is None:
        idx = np.arange(lattice_size(lat), dtype=np.int64)
    i, j, k = lattice_ijk(lat, idx)
    out = np.empty((len(i), 3), dtype=np.float64)
    out[:, 0] = np.float64(lat["x0"]) + i.astype(np.float64) * np.float64(lat["step_x"])
    out[:, 1] = np.float64(lat["y0"]) + j.astype(np.float64) * np.float64(lat["step_y"])
    out[:, 2] = np.float64(lat["yaw0"]) + k.astype(np.float64) * np.float64(lat["step_yaw"])
    return out


def capi_lattice(capi, lat):
    return capi.PoseLattice(lat["x0"], lat["y0"], lat["yaw0"], lat["step_x"], lat["step_y"], lat["step_yaw"],
                            lat["nx"], lat["ny"], lat["nyaw"])


def ref_eligible(score, pairs, dims, local_max):
    """dims = (nx, ny, nyaw).  pairs > 0 and, with local_max, score > every lattice neighbour of lower index and >= every
    one of higher index; neighbours outside the lattice do not exist, no yaw wrap."""
    nx, ny, nk = dims
    s = np.asarray(score, dtype=np.float64).reshape(nk, ny, nx)
    ok = np.asarray(pairs).reshape(nk, ny, nx) > 0
    if not local_max:
        return ok.ravel()
    ok = ok.copy()

    def cut(d, n):            # (centre slice, neighbour slice) along an axis of length n for offset d
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))

    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if dk == dj == di == 0:
                    continue
                (ck, nk_), (cj, nj_), (ci, ni_) = cut(dk, nk), cut(dj, ny), cut(di, nx)
                c, nb = s[ck, cj, ci], s[nk_, nj_, ni_]
                lower = (dk * ny + dj) * nx + di < 0
                ok[ck, cj, ci] &= (c > nb) if lower else (c >= nb)
    return ok.ravel()


def ref_select(score, pairs, dims, top_k, local_max):
    """The min(top_k, eligible) eligible indices of largest score, descending, ties to the lower index (uint64)."""
    score = np.asarray(score, dtype=np.float64).ravel()
    idx = np.flatnonzero(ref_eligible(score, pairs, dims, local_max))
    order = np.lexsort((idx, -score[idx]))
    return idx[order][:top_k].astype(np.uint64)


def ref_cost(records):
    return np.where(records["converged"] != 0, records["fitness"], NOT_CONVERGED_COST)


def ref_best(records):
    """arg-min of the cost, ties to the lower index; -1 for no records."""
    return int(np.argmin(ref_cost(records))) if len(records) else -1


def oracle_scores(oracle, om, scan, poses):
    """(score [P] float64, pairs [P] uint32) of oracle.Map `om` at every pose, through ndt_oracle_eval_at."""
    L = oracle.lib()
    scan = np.ascontiguousarray(scan, dtype=np.float32).reshape(-1, 2)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    P = len(poses)
    score = np.zeros(P, dtype=np.float64)
    pairs = np.zeros(P, dtype=np.uint32)
    g = (C.c_double * 3)(); H = (C.c_double * 9)(); pr = C.c_double(); p = (C.c_double * 3)()
    sp, n, prr = scan.ctypes.data, len(scan), C.byref(pr)
    f = L.ndt_oracle_eval_at
    for q in range(P):
        p[0], p[1], p[2] = poses[q]
        score[q] = f(om.h, sp, n, 8, p, g, H, prr)
        pairs[q] = int(pr.value)
    return score, pairs


def relocalize_ref(oracle, om, scan, lat, top_k, local_max=True):
    """The prototype on the oracle: sweep, pick, refine with align_batch(shared_scan) -> dict like capi.Map.relocalize."""
    poses = lattice_poses(lat)
    score, pairs = oracle_scores(oracle, om, scan, poses)
    cand = ref_select(score, pairs, (lat["nx"], lat["ny"], lat["nyaw"]), top_k, local_max)
    scan = np.ascontiguousarray(scan, dtype=np.float32).reshape(-1, 2)
    rec = om.align_batch(scan, [0, len(scan)], poses[cand.astype(np.int64)], shared_scan=True) if len(cand) else \
        np.zeros(0, dtype=oracle.RESULT_DTYPE)
    return dict(cand_index=cand, cand_score=score[cand.astype(np.int64)], records=rec, best=ref_best(rec), scores=score)


def wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def pose_error(pose, truth):
    """(metres, radians) between a record's pose and the truth."""
    return math.hypot(pose[0] - truth[0], pose[1] - truth[1]), abs(wrap(pose[2] - truth[2]))


def eval_poses(sf, k, n_random=200, half=24.0, seed=77):
    """The pose list of the score tests for scan k: the four poses of test_single_evaluation_matches_oracle (init, truth,
    near-zero yaw, (30, 30) beyond the map's rim -- where a 30 m scan may still reach a voxel), one pose far off the map, and
    n_random poses drawn uniformly over the world and all yaws."""
    scan, truth, init = sf.make(k)
    rng = np.random.default_rng(seed + k)
    rnd = np.stack([rng.uniform(-half, half, n_random), rng.uniform(-half, half, n_random),
                    rng.uniform(-math.pi, math.pi, n_random)], axis=1)
    fixed = np.array([init, truth, [truth[0], truth[1], 5e-5], [30.0, 30.0, 0.3], [300.0, -300.0, 0.3]], dtype=np.float64)
    return scan, truth, np.concatenate([fixed, rnd])


def edge_poses(truth):
    """Poses of the edge tests: on the map, at its rim, far off it (float32 overflow included) -- finite ones only."""
    return np.array([truth, [truth[0], truth[1], truth[2] + 100.0], [24.0, 24.0, 0.0], [-24.3, 23.9, 3.0], [30.0, 30.0, 0.3],
                     [1e6, -1e6, 1.0], [1e30, 0.0, 0.0], [0.0, -1e39, 0.5], [0.0, 0.0, 1e5], [0.0, 0.0, -1e20]], dtype=np.float64)


def crafted_volumes():
    """(name, dims (nx, ny, nyaw), score, pairs) -- the pick's corner cases."""
    out = []
    rng = np.random.default_rng(3)
    dims = (7, 5, 3)
    n = 7 * 5 * 3
    out.append(("all_equal", dims, np.full(n, 2.5), np.ones(n, np.uint32)))
    s = np.zeros(n); s[40] = s[41] = 9.0                                  # two cells, x neighbours
    out.append(("plateau2", dims, s, np.ones(n, np.uint32)))
    s = rng.uniform(0.0, 1.0, n)
    for c in (0, 6, 28, 34, 70, 76, 98, 104, 3, 52, 14):                  # the eight corners, two edge cells, an interior cell
        s[c] = 5.0 + c
    out.append(("faces_corners", dims, s, np.ones(n, np.uint32)))
    s = rng.uniform(0.0, 1.0, n); p = np.ones(n, np.uint32)
    best = np.argsort(-s)[:6]
    p[best[::2]] = 0                                                      # the best, third and fifth: no pairs
    out.append(("pairs_zero", dims, s, p))
    out.append(("none_eligible", dims, rng.uniform(0.0, 1.0, n), np.zeros(n, np.uint32)))
    out.append(("one", (1, 1, 1), np.array([0.25]), np.ones(1, np.uint32)))
    out.append(("one_empty", (1, 1, 1), np.array([0.25]), np.zeros(1, np.uint32)))
    s = rng.uniform(0.0, 1.0, 40); s[[0, 13, 14, 39]] = [3.0, 4.0, 4.0, 2.0]
    out.append(("line_y", (1, 40, 1), s.copy(), np.ones(40, np.uint32)))
    out.append(("line_x", (40, 1, 1), s.copy(), np.ones(40, np.uint32)))
    out.append(("line_yaw", (1, 1, 40), s.copy(), np.ones(40, np.uint32)))
    # more than one run of 1024 poses, ties across runs, signed zeros
    dims = (33, 17, 5)
    n = 33 * 17 * 5
    s = np.round(rng.uniform(0.0, 4.0, n), 1); s[s == 0.0] = -0.0
    p = (rng.uniform(0, 1, n) > 0.2).astype(np.uint32)
    out.append(("ties_across_runs", dims, s, p))
    return out
