"""Workloads that walk ndt_sessions_find_loops_multi and ndt_sessions_find_cross_loops through what they added to the search (LpSearch)
(ndt_slam_amd/csrc/ndt_loops.hip.h; tests only): several candidates of a session in a row behind one newest scan (rank, scan_of),
a resident map slot per rank, another session's closed cloud, trajectory and anchor pose (owner_of), the ranged verification
and the host decision behind it.  tests/loop_shape_workloads.py's machinery and settings: 181 beams, score_thre -1, sepThre 1,
LP; a call carries kind ("multi", "cross", or none of it: the single search), mp (max_submaps, max_d2, min_overlap) and, for
a cross call, against.  tests/test_loop_multi_shapes_host.py checks every certificate that needs no device;
tests/test_gpu_loop_multi_shapes.py holds the device byte for byte to the composed chain on every family.

With sepThre 1 a session splits at its own steps 2, 4, 6, ...: behind its step k it has k // 2 closed submaps, the multi search
may meet all but the newest of them (nearest first: on these drives the newest eligible one is rank 0), the cross search every
closed submap of the OTHER sessions.

What was found while the table was made:
  cross_owners  the issue's searcher without a closed submap has 2 frames, not 3: a session's step 2 closes its first submap.
  refused_ranks the set with the outlier in the newest eligible submap carries it in that submap's LAST scan (scan 7 of 12): in
                its first scan (6) the triple (5, 6, 7) drops the lone point at step 7, before the submap closes.  And it is
                another point than session_workloads.GRID_OUTLIER: the build refuses a BOX of more than 2^28 cells, and at
                scan 7's heading (8000, 8000) lies 3.5 degrees off the map's x axis -- 37600 x 2300 cells, a map that builds.
                AHEAD_OUTLIER lies on the box's diagonal there.
  decisions     the issue's grid has no candidate with usable and unusable slots together: the eight picks of a 0.1 m lattice
                end in one basin and share their overlap.  WIDE adds calls on a lattice of 0.5 m and 5 degrees.  No record fails
                to converge, with MaximumIterations = 1 either (tried on this set: 120 records, 120 converged).
"""
import math

import numpy as np

import loop_shape_workloads as L
import session_workloads as W
from loop_shape_workloads import INF, LP, _call, _family, _logs, cut_scan, gate_of, lp  # noqa: F401
from session_helpers import lockstep

MP = dict(max_submaps=4, max_d2=0.09, min_overlap=0.5)
DBL_MAX = float(np.finfo(np.float64).max)


def mp(**kw):
    return dict(MP, **kw)


def multi(k, which, tag="", lp_=None, **mp_kw):
    return _call(k, lp_ or lp(), which, tag, kind="multi", mp=mp(**mp_kw))


def cross(k, which, against=None, tag="", lp_=None, **mp_kw):
    return _call(k, lp_ or lp(), which, tag, kind="cross", mp=mp(**mp_kw), against=None if against is None else list(against))


def multi_params(capi, call):
    """ndt_loop_multi_params of a multi or cross call."""
    q = call["lp"]
    hx, hy, hk = q["half"]
    return capi.default_loop_multi_params(min_path=q["min_path"], radius=q["radius"], step_xy=q["step_xy"], step_yaw=q["step_yaw"],
                                          half_x=hx, half_y=hy, half_yaw=hk, top_k=q["top_k"], local_max=q["local_max"],
                                          max_cost=q["max_cost"], **call["mp"])


# ---------------------------------------------------------------------------------------------- the families
RANK_FRAMES = (6, 8, 10, 12)                        # behind step 11: 1, 2, 3 and 4 eligible submaps
RANK_CUTS = (1, 63, 65, 257)                        # raw points of the last scans


def _ragged_ranks():
    logs = _logs([(33 + i, n) for i, n in enumerate(RANK_FRAMES)])
    for i, n in enumerate(RANK_CUTS):
        logs[i][0][-1] = cut_scan(logs[i][0][-1], n)
    return _family("ragged_ranks", logs, [multi(11, [1] * 4)], per_session=[1, 2, 3, 4], submaps=[[0], [1, 0], [2, 1, 0], [3, 2, 1, 0]])


MANY_S = 65
MANY_CLASSES = tuple((33 + c, 12) for c in range(5))


def _many_ranks():
    cls = [(7 * i + 3) % len(MANY_CLASSES) for i in range(MANY_S)]
    return _family("many_ranks", _logs(MANY_CLASSES), [multi(11, [1] * MANY_S)], cls=cls, per_class=4)


REFUSED = ((33, 12), (34, 12), (35, 12))


AHEAD_OUTLIER = (11000.0, 0.0)                      # straight ahead: at scan 7's heading (138 deg) it spans 27000 x 24000 cells


def _refused_ranks(name, bad, scan, rank, outlier=W.GRID_OUTLIER):
    """Session `bad` carries the outlier in scan `scan`: the closed cloud of its candidate of rank `rank`."""
    logs = _logs(REFUSED)
    logs[bad][0][scan] = np.concatenate([logs[bad][0][scan], np.array([outlier], np.float64)])
    others = [0 if i == bad else 1 for i in range(3)]
    calls = [multi(11, [1, 1, 1], "all"), multi(11, others, "without the bad session")]
    if rank == 0:
        calls.append(multi(11, [1 - o for o in others], "the bad session alone, one submap", max_submaps=1))
    return _family(name, logs, calls, tolerant=True, bad=bad, bad_scan=scan, bad_rank=rank, outlier=tuple(outlier))


OWNER_FRAMES = (6, 2, 12, 4)                        # A: 2 closed submaps, B: none (not a track), C: 5, D: 1
OWNERS_PAIR = [1, 0, 0, 1]                          # `against` of the first call: A and D, three closed submaps between them
OWNER_SHIFT = ((0.03, 0.0), (0.0, 0.0), (0.0, -0.04), (-0.02, 0.02))    # metres added to a whole odometry: no two sessions share a pose


def _cross_owners():
    """The drives share one odometry path; shifted by a few centimetres each, an owner's pose at a scan is not the searcher's
    pose at the scan of the same number (the anchor pose of the edge is then told apart from the searcher's own)."""
    logs = _logs([(33 + i, n) for i, n in enumerate(OWNER_FRAMES)])
    for (scans, odo), (dx, dy) in zip(logs, OWNER_SHIFT):
        odo[:, 0] += dx
        odo[:, 1] += dy
    return _family("cross_owners", logs, [cross(11, [1, 1, 1, 1], OWNERS_PAIR, "against A and D"),
                                          cross(11, [1, 1, 0, 1], None, "C is searched and does not search")],
                   closed=[2, 0, 5, 1], silent_track=2, not_a_track=1)


CRE_BAD = 0                                         # the outlier in its scan 0 AND an empty newest scan: it searches, too


def _cross_refused_empty():
    logs = _logs(((33, 6), (34, 6), (35, 6)))
    logs[CRE_BAD][0][0] = np.concatenate([logs[CRE_BAD][0][0], np.array([W.GRID_OUTLIER], np.float64)])
    logs[CRE_BAD][0][5] = W.EMPTY
    return _family("cross_refused_empty", logs, [cross(5, [1, 1, 1], None, "all"), cross(5, [1, 1, 1], [0, 1, 1], "without the bad track"),
                                                 cross(5, [1, 0, 0], None, "only the empty searcher")],
                   tolerant=True, bad=CRE_BAD, bad_submap=0, empty=CRE_BAD)


def _cross_zero_pose():
    """zero_pose's drive, and beside it the same line under another drive's scans: both maps are in the line's frame."""
    (scans, odo), _ = L.family("zero_pose")["logs"]
    beside = _logs(((34, len(L.ZERO_X)),))[0][0]
    logs = [([x.copy() for x in scans], odo.copy()), (beside, odo.copy())]
    return _family("cross_zero_pose", logs, [cross(len(L.ZERO_X) - 1, [1, 1], None)], zero=0)


DECISION_GRID = [(o, d, c, k) for o in (0.0, 0.5, 1.0) for d in (0.0, 0.09, DBL_MAX) for c in (-INF, 0.02, INF) for k in (1, 8)]


WIDE = dict(step_xy=0.5, step_yaw=math.radians(5.0))           # picks in different basins
WIDE_OVERLAPS = (0.5, 0.75, 0.9)


def _decisions():
    logs = _logs(((33, 8), (34, 10)))
    calls = [multi(9, [1, 1], "min_overlap %s max_d2 %s max_cost %s top_k %d" % (o, d, c, k), lp(max_cost=c, top_k=k), min_overlap=o, max_d2=d)
             for o, d, c, k in DECISION_GRID]
    calls += [multi(9, [1, 1], "wide, min_overlap %s" % o, lp(**WIDE), min_overlap=o) for o in WIDE_OVERLAPS]
    return _family("decisions", logs, calls)


HISTORY_FRAMES = (15, 12, 13)
HISTORY_THIN = ((0, 4), (0, 5))                     # (class, scan) cut to every second beam: submap 2 of class 0 is a small cloud


def _slot_history():
    logs = _logs([(33 + i, n) for i, n in enumerate(HISTORY_FRAMES)])
    for c, k in HISTORY_THIN:
        logs[c][0][k] = logs[c][0][k][::2].copy()
    every = [1, 1, 1]
    calls = [_call(7, lp(), every, "single 7"), multi(7, every, "multi 4 at 7"), multi(7, every, "multi 2 at 7", max_submaps=2),
             cross(7, every, None, "cross at 7"),
             multi(9, every, "multi 4 at 9"), cross(9, every, None, "cross at 9"), _call(9, lp(), every, "single 9"),
             multi(9, every, "multi 4 at 9 again"),
             multi(12, every, "multi 2 at 12", max_submaps=2), cross(12, every, None, "cross at 12"), multi(12, every, "multi 4 at 12")]
    return _family("slot_history", logs, calls, twin=True)


FAMILIES = {
    "ragged_ranks": _ragged_ranks, "many_ranks": _many_ranks,
    "refused_rank3": lambda: _refused_ranks("refused_rank3", 1, 0, 3),
    "refused_rank0_first": lambda: _refused_ranks("refused_rank0_first", 0, 7, 0, AHEAD_OUTLIER),
    "slot_history": _slot_history, "cross_owners": _cross_owners, "cross_refused_empty": _cross_refused_empty,
    "cross_zero_pose": _cross_zero_pose, "decisions": _decisions,
}
_MADE = {}


def family(name):
    if name not in _MADE:
        _MADE[name] = FAMILIES[name]()
    return _MADE[name]


def kind_of(call):
    return call.get("kind", "single")


# ---------------------------------------------------------------------------------------------- the host model
def host_track(pm):
    """A model's (poses, sub_first, sub_anchor, sub_offsets) as the gates take them (session_schedules.host_gate's rule: every
    closed submap that held a scan counts as a cloud with points)."""
    import session_schedules as SS
    firsts, anchors, _ = SS.layout(pm)
    sizes = [1 if len(s.scans) else 0 for s in pm.submaps[:-1]]
    off = np.concatenate([[0], np.cumsum(sizes), [sum(sizes)]]).astype(np.uint64) if sizes else np.zeros(2, np.uint64)
    return SS.host_poses(pm), np.asarray(firsts, np.int32), np.asarray(anchors, np.int32), off


def host_candidates(capi, fam, call, pms):
    """The candidates of one call on the host models, in the call's order: [(session, rank, owner session, submap, anchor_scan,
    newest_scan)].  The single and the multi search by gate_multi_ref (loops_multi_helpers), the cross search by cross_gate_ref
    (cross_loops_helpers) with the tracks in ascending session order."""
    from cross_loops_helpers import cross_gate_ref
    from loops_multi_helpers import gate_multi_ref
    cls, kind, out = fam["cls"], kind_of(call), []
    named = [i for i, w in enumerate(call["which"]) if w]
    if kind != "cross":
        k = call["mp"]["max_submaps"] if kind == "multi" else 1
        for i in named:
            pm = pms[cls[i]]
            if not pm.poses:
                continue
            for r, c in enumerate(gate_multi_ref(*host_track(pm), k, **gate_of(call["lp"]))):
                out.append((i, r, i, c["submap"], c["anchor_scan"], c["newest_scan"]))
        return out
    p = multi_params(capi, call)
    who = [i for i in range(len(cls)) if (call["against"] is None or call["against"][i]) and pms[cls[i]].poses and len(pms[cls[i]].submaps) >= 2]
    tracks = [host_track(pms[cls[i]]) for i in who]
    for i in named:
        pm = pms[cls[i]]
        if not pm.poses or not tracks:
            continue
        poses = host_track(pm)[0]
        for c in cross_gate_ref(capi, poses[-1], len(poses) - 1, who.index(i) if i in who else -1, tracks, p, session=i):
            out.append((i, int(c["rank"]), who[int(c["map_session"])], int(c["cand"]["submap"]), int(c["cand"]["anchor_scan"]),
                        int(c["cand"]["newest_scan"])))
    return out


def host_run(capi, fam):
    """The family on replay.PointCloudMap's bookkeeping alone (loop_shape_workloads.host_run's model) -> (per call
    host_candidates' list, the models behind the last step)."""
    import session_schedules as SS
    logs = fam["logs"]
    C = len(logs)
    pms, prev, out = [SS.host_map(fam["p"]["sepThre"]) for _ in range(C)], [None] * C, []
    for k, scans, odo, act in lockstep(logs, fam["starts"]):
        for c in range(C):
            if act[c]:
                SS.host_add(pms[c], odo[c], prev[c], k)
                prev[c] = odo[c].copy()
        out += [host_candidates(capi, fam, call, pms) for call in fam["calls"] if call["k"] == k]
    return out, pms
