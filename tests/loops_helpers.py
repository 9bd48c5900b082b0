"""References for the loop search (ndt_loop_gate, ndt_sessions_loop_candidates, ndt_sessions_find_loops; tests only).

gate_ref        the gating of include/ndt_mi355x.h restated in numpy float64 scalars: one rounding per product, sum and root.
robot_frame     a map-frame scan at a pose back in the robot frame, ndt_repose_points' arithmetic in numpy.
loop_workload   the issue's workload: the 5 m circle of synth.replay_records, 0.6 m per frame, 181 beams, sepThre 5.
expected_pose   where the newest scan truly is in the drifted map: traj[anchor] (+) truth[anchor]^-1 (+) truth[newest].
chain_layout    what ndt_sessions_trajectory and ndt_sessions_global_map give for a session, from a comparison chain.
compose_loop    one candidate's search made of public single-job calls on a chain's own data (a refused map: its code and
                nothing else; an empty filtered scan: nothing scored, nothing picked); assert_loop_is holds an ndt_loop and its
                records to such a result, assert_composed composes and holds, loop_bytes is a candidate's whole result as bytes.
"""
import math
import re

import numpy as np

from ndt_slam_amd import replay, synth
from gpu_support import sync, to_dev
from reloc_helpers import ref_best, ref_cost
from session_correct_helpers import layout
from session_helpers import session_logs
from test_gpu_sessions_correct import chain_poses

FULL_LAP, HALF_LAP = 56, 28


def loop_params_dict(p):
    return dict(min_path=p.min_path, radius=p.radius, step_xy=p.step_xy, step_yaw=p.step_yaw, half=(p.half_x, p.half_y, p.half_yaw))


def gate_ref(poses, sub_first, sub_anchor, sub_offsets, min_path, radius, step_xy, step_yaw, half):
    """-> dict(submap, anchor_scan, newest_scan, nearest_scan, dist, path, lattice = dict like reloc_helpers.LAT) or None."""
    T = np.asarray(poses, np.float64).reshape(-1, 3)
    n, n_closed = len(T), len(sub_first) - 1
    if n < 1 or n_closed < 2:
        return None

    def dist(a, b):
        dx, dy = T[a, 0] - T[b, 0], T[a, 1] - T[b, 1]
        return np.sqrt(dx * dx + dy * dy)

    best = None
    for m in range(n_closed - 1):
        first, last = int(sub_first[m]), int(sub_first[m + 1]) - 1
        if last < first or sub_offsets[m + 1] == sub_offsets[m]:
            continue
        path = np.float64(0.0)
        for k in range(last, n - 1):
            path = path + dist(k + 1, k)
        if not path >= min_path:
            continue
        d, near = dist(n - 1, first), first
        for k in range(first + 1, last + 1):
            dk = dist(n - 1, k)
            if dk < d:
                d, near = dk, k
        if not d <= radius or (best is not None and not d < best["dist"]):
            continue
        best = dict(submap=m, anchor_scan=int(sub_anchor[m]), newest_scan=n - 1, nearest_scan=near, dist=float(d), path=float(path))
    if best is None:
        return None
    tx, ty, yaw = T[n - 1, 0], T[n - 1, 1], T[n - 1, 2] * np.float64(math.pi) / np.float64(180)
    hx, hy, hk = half
    best["lattice"] = dict(x0=float(tx - np.float64(hx) * np.float64(step_xy)), y0=float(ty - np.float64(hy) * np.float64(step_xy)),
                           yaw0=float(yaw - np.float64(hk) * np.float64(step_yaw)), step_x=step_xy, step_y=step_xy, step_yaw=step_yaw,
                           nx=2 * hx + 1, ny=2 * hy + 1, nyaw=2 * hk + 1)
    return best


def same_candidate(rec, ref):
    """A LOOP_CANDIDATE_DTYPE record against gate_ref's dict, the doubles to the bit."""
    L, R = rec["lattice"], ref["lattice"]
    return (all(int(rec[f]) == ref[f] for f in ("submap", "anchor_scan", "newest_scan", "nearest_scan")) and
            all(np.float64(rec[f]).tobytes() == np.float64(ref[f]).tobytes() for f in ("dist", "path")) and
            all(np.float64(L[f]).tobytes() == np.float64(R[f]).tobytes() for f in ("x0", "y0", "yaw0", "step_x", "step_y", "step_yaw")) and
            all(int(L[f]) == R[f] for f in ("nx", "ny", "nyaw")))


def robot_frame(xy, pose):
    """ndt_repose_points with old pose = `pose` (tx, ty, th[deg]) and new pose = (0, 0, 0): fp64, rounded once to float32."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    if tuple(np.float64(v).tobytes() for v in pose) == (np.float64(0.0).tobytes(),) * 3:
        return xy.copy()
    a = np.float64(pose[2]) * np.float64(math.pi) / np.float64(180)
    c, s = np.cos(a), np.sin(a)
    dx, dy = xy[:, 0].astype(np.float64) - np.float64(pose[0]), xy[:, 1].astype(np.float64) - np.float64(pose[1])
    lx = dx * c + dy * s
    ly = dx * (-s) + dy * c
    gx = np.float64(1.0) * lx + np.float64(-0.0) * ly + np.float64(0.0)
    gy = np.float64(0.0) * lx + np.float64(1.0) * ly + np.float64(0.0)
    return np.stack([gx, gy], axis=1).astype(np.float32)


def loop_workload(seed=33, n_frames=FULL_LAP, **params):
    """((scans, odometry), true poses [n, 3], launch parameters) of one session of the workload."""
    (log,) = session_logs(((seed, n_frames),), n_beams=181)
    _, truth = synth.replay_records(n_frames=n_frames, n_beams=181, step=0.6, seed=seed)
    return log, np.asarray(truth, np.float64).reshape(-1, 3), dict(replay.LAUNCH_PARAMS, sepThre=5.0, **params)


def compose(a, b):
    """Pose a (+) pose b (tx, ty, th[deg])."""
    r = math.radians(a[2])
    return np.array([a[0] + math.cos(r) * b[0] - math.sin(r) * b[1], a[1] + math.sin(r) * b[0] + math.cos(r) * b[1], a[2] + b[2]])


def between(a, b):
    """a^-1 (+) b."""
    r = math.radians(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([math.cos(r) * dx + math.sin(r) * dy, -math.sin(r) * dx + math.cos(r) * dy, b[2] - a[2]])


def expected_pose(traj, truth, anchor, newest):
    return compose(np.asarray(traj, np.float64).reshape(-1, 3)[anchor], between(truth[anchor], truth[newest]))


def pose_gap(p, q):
    """(metres, degrees) between two (tx, ty, th[deg]) poses."""
    return math.hypot(p[0] - q[0], p[1] - q[1]), abs((p[2] - q[2] + 180.0) % 360.0 - 180.0)


# ---- the search composed of public single-job calls on a comparison chain (needs the device) ----

def chain_layout(chain, i):
    """What ndt_sessions_trajectory and ndt_sessions_global_map give for session i, from the chain's bookkeeping."""
    pm = chain.pcmaps[i]
    first, anchor, _ = layout(pm)
    sizes = [len(s.p_cloud) for s in pm.submaps[:-1]]
    off = np.concatenate([[0], np.cumsum(sizes), [sum(sizes)]]).astype(np.uint64) if sizes else np.zeros(2, np.uint64)
    return chain_poses(chain, i), first, anchor, off


def _zero_loop(status, n_src=0):
    return dict(status=status, n_src=n_src, n_cand=0, best=-1, cand_index=np.zeros(0, np.uint64), cand_score=np.zeros(0), cand_cost=np.zeros(0),
                pose=np.zeros(3), rel=np.zeros(3), found=0)


def compose_loop(sc, i, cand, lp):
    """One candidate's search made of public single-job calls on the chain's own data -> (fields of its ndt_loop, records).
    A candidate cloud whose map the single build refuses gives that code as the status and nothing else; a newest scan that
    filters to no point scores nothing and picks nothing."""
    import torch
    capi, ctx, chain = sc["capi"], sc["ctx"], sc["chain"]
    pm, traj = chain.pcmaps[i], chain_poses(chain, i)
    none = np.zeros(0, capi.RESULT_DTYPE)
    cloud = np.ascontiguousarray(pm.submaps[int(cand["submap"])].p_cloud, np.float32).reshape(-1, 2)
    try:
        gm = capi.Map(ctx, cloud, chain.params)
    except capi.NdtError as e:
        return _zero_loop(int(re.search(r"-> (-?\d+):", str(e)).group(1))), none
    newest = np.ascontiguousarray(pm.submaps[-1].scans[-1], np.float32).reshape(-1, 2)
    src = newest
    if len(newest):
        robot = capi.repose_points(ctx, newest, [0, len(newest)], traj[-1:], np.zeros((1, 3)))
        src = ctx.prefilter(robot, sc["p"]["LeafSize"])
    if not len(src):
        gm.close()
        return _zero_loop(0), none
    L = capi.PoseLattice.from_buffer_copy(cand["lattice"].tobytes())
    d_src = to_dev(src)
    d_s = torch.zeros(L.size, dtype=torch.float64, device=d_src.device)
    d_p = torch.zeros(L.size, dtype=torch.int32, device=d_src.device)
    d_c = torch.zeros(lp.top_k, dtype=torch.int64, device=d_src.device)
    d_n = torch.zeros(1, dtype=torch.int32, device=d_src.device)
    sync()
    gm.score_lattice(d_src.data_ptr(), len(src), L, d_s.data_ptr(), d_p.data_ptr())
    gm.lattice_select(L, d_s.data_ptr(), d_p.data_ptr(), lp.top_k, lp.local_max, d_c.data_ptr(), d_n.data_ptr())
    sync()
    n = int(d_n.cpu()[0])
    idx, score = d_c.cpu().numpy()[:n].astype(np.uint64), d_s.cpu().numpy()
    recs = np.concatenate([gm.align_batch(src, [0, len(src)], L.pose(int(q)).reshape(1, 3)) for q in idx]) if n else none
    gm.close()
    best = ref_best(recs)
    out = dict(status=0, n_src=len(src), n_cand=n, best=best, cand_index=idx, cand_score=score[idx.astype(np.int64)], cand_cost=ref_cost(recs))
    if best >= 0:
        w = recs[best]["pose"]
        out["pose"] = np.array([w[0], w[1], w[2] * np.float64(180) / np.float64(np.pi)])
        out["rel"] = capi.pg_edge_between(traj[int(cand["anchor_scan"])], out["pose"])
        out["found"] = int(out["cand_cost"][best] <= lp.max_cost)
    else:
        out["pose"], out["rel"], out["found"] = np.zeros(3), np.zeros(3), 0
    return out, recs


def loop_bytes(loop, rec):
    """A candidate's whole ndt_loop and its written records as bytes."""
    return loop.tobytes() + rec[:int(loop["n_cand"])].tobytes()


def assert_loop_is(loop, rec, ref, recs, lp):
    """An ndt_loop and its records against compose_loop's result, byte for byte."""
    n = ref["n_cand"]
    assert loop["status"] == ref["status"] and loop["n_cand"] == n and loop["best"] == ref["best"] and loop["found"] == ref["found"]
    for f in ("cand_index", "cand_score", "cand_cost"):
        assert loop[f][:n].tobytes() == ref[f].tobytes(), f
        assert not loop[f][n:].any(), f
    assert rec[:n].tobytes() == recs.tobytes()                              # every record, byte for byte
    assert loop["pose"].tobytes() == ref["pose"].tobytes()
    e = loop["edge"]
    assert (e["from_"], e["to"]) == (loop["cand"]["anchor_scan"], loop["cand"]["newest_scan"])
    assert e["rel"].tobytes() == ref["rel"].tobytes() and e["info"].tobytes() == np.array(lp.info[:]).tobytes()


def assert_composed(sc, loop, rec, lp):
    """A search that ran (status NDT_OK) against the composition on the chain's session of the same index."""
    ref, recs = compose_loop(sc, int(loop["cand"]["session"]), loop["cand"], lp)
    assert loop["status"] == 0
    assert_loop_is(loop, rec, ref, recs, lp)
