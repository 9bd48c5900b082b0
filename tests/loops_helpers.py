"""References for the loop search (ndt_loop_gate, ndt_sessions_loop_candidates, ndt_sessions_find_loops; tests only).

gate_ref        the gating of include/ndt_mi355x.h restated in numpy float64 scalars: one rounding per product, sum and root.
robot_frame     a map-frame scan at a pose back in the robot frame, ndt_repose_points' arithmetic in numpy.
loop_workload   the issue's workload: the 5 m circle of synth.replay_records, 0.6 m per frame, 181 beams, sepThre 5.
expected_pose   where the newest scan truly is in the drifted map: traj[anchor] (+) truth[anchor]^-1 (+) truth[newest].
"""
import math

import numpy as np

from ndt_slam_amd import replay, synth
from session_helpers import session_logs

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
