"""References for the loop search over several submaps (ndt_loop_gate_multi, ndt_sessions_loop_candidates_multi,
ndt_sessions_find_loops_multi) and for ndt_fit_points_multi; tests only.

gate_multi_ref  the k nearest eligible submaps in (dist, submap) order by loops_helpers.gate_ref's own arithmetic: gate_ref is
                asked again with the closed cloud of every submap it has already given made empty -- an empty cloud is not
                eligible, and nothing else of the rule looks at a cloud's size.
decide_ref      the decision of ndt_sessions_find_loops_multi restated: cand_cost per slot, best, found.
fit_multi_case  three small maps of fitness_workloads (two leaves, two world offsets) and twelve matches dealt over them.
"""
import numpy as np

import fitness_workloads as W
from fit_points_helpers import IDENT, tf_of_pose
from loops_helpers import gate_ref

F = np.float32
NOT_USABLE_COST = 1e7
MULTI = dict(radius=4.0, max_submaps=2, max_d2=0.09, min_overlap=0.5)         # the issue's parameters on the lap


def gate_multi_ref(poses, sub_first, sub_anchor, sub_offsets, max_submaps, **loop):
    """-> list of gate_ref's dicts, nearest first (possibly empty); `loop`: gate_ref's keywords (loops_helpers.loop_params_dict)."""
    sizes = np.diff(np.asarray(sub_offsets, np.uint64).astype(np.int64))
    out = []
    for _ in range(max_submaps):
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        ref = gate_ref(poses, sub_first, sub_anchor, off, **loop)
        if ref is None:
            break
        out.append(ref)
        sizes[ref["submap"]] = 0
    return out


def decide_ref(converged, fit, min_overlap, max_cost):
    """converged [n], fit = FIT_STATS-like records or (fitness, n_in, n_points) triples [n] -> (cand_cost [n], best, found)."""
    cost, keys = [], []
    for c in range(len(converged)):
        fitness, n_in, n_points = (float(fit[c]["fitness"]), int(fit[c]["n_in"]), int(fit[c]["n_points"])) if hasattr(fit[c], "dtype") \
            else (float(fit[c][0]), int(fit[c][1]), int(fit[c][2]))
        usable = bool(converged[c]) and n_in >= 1 and float(n_in) >= np.float64(min_overlap) * np.float64(n_points)
        k = fitness if usable else NOT_USABLE_COST
        ok = k <= max_cost
        cost.append(k)
        keys.append((not ok, -(n_in if usable else 0), k, c))
    if not keys:
        return np.zeros(0), -1, 0
    best = min(keys)[3]
    return np.array(cost, np.float64), best, int(cost[best] <= max_cost)


# ------------------------------------------------------------------------------------------ ndt_fit_points_multi
FIT_MAPS = (("one", 0.3, W.OFFSETS[0]), ("narrow7", 0.3, W.OFFSETS[0]), ("islands", 1.0, W.OFFSETS[1]))
FIT_LENGTHS = (0, 1, 63, 64, 65, 129, 300, 64, 65, 1, 300, 129)              # twelve matches
FIT_MAP_OF = (0, 1, 2, 0, 1, 2, 0, 2, 0, 2, 2, 0)                            # every map shared by several matches (the tests pass a fourth entry that none names)
STILL = dict(max_iter=0, min_pts=1 << 30)


def fit_multi_case():
    """-> (workloads [3], matches: list of (map index, scan [n, 2] float32, tf of four float32)).  Match b's scan is a slice of
    its map's query set, seen from a pose of its own (the identity for every third match), so that its transform lands it on
    the map again."""
    ws = [W.make(f, leaf, off) for f, leaf, off in FIT_MAPS]
    matches = []
    for b, (n, mi) in enumerate(zip(FIT_LENGTHS, FIT_MAP_OF)):
        w = ws[mi]
        q = w.queries[(37 * b) % 500:][:n]
        if b % 3 == 0:
            scan, tf = q, IDENT
        else:
            base, L = W.lattice_base(w.leaf, w.offset)
            pose = (base[0] + (1.5 + b) * L, base[1] - (0.7 * b) * L, 0.35 * b - 1.0)
            scan, tf = W.scan_for(q, pose), tf_of_pose(pose)
        matches.append((mi, np.ascontiguousarray(scan, F).reshape(-1, 2), tf))
    return ws, matches
