"""Workloads that walk ndt_sessions_find_loops (ndt_slam_amd/csrc/ndt_loops.hip.h) through its own layout arithmetic (tests
only): named families of small session sets, the searches made on them, and per family a certificate that says which branch
of LpSearch / loop_scan_kernel / loop_guess_kernel it reaches.  tests/test_loop_shapes_host.py checks every certificate
that needs no device; tests/test_gpu_loop_shapes.py holds the device byte for byte to the composed chain on every family and
checks the certificates that are statements about picks (n_cand), on the composed reference.

The logs are synth.replay_records drives (session_helpers.session_logs) of 181 beams: the candidate maps then have voxels with
a covariance and the sweep picks poses (at 61 beams it picks none, see tests/session_workloads.py).  Every family runs with
score_thre = -1 -- the fused pose is the odometry prediction, so the host knows poses, splits and candidates (host_run) -- and
sepThre 1.0: with 0.609 m per step a session splits at its own steps 2, 4, 6, ..., has two closed submaps from step 4 on, and
with LP (min_path 0, radius 10: the whole circle) its candidate behind step k is submap (k // 2) - 2, the newest eligible one.

A family is a dict: name, logs [(scans, odo)] and starts per CLASS, cls (the class of every session of the set; the chain
runs one session per class), p (launch parameters), tolerant (the chain runs with allow_item_failures), calls [dict(k, lp,
which, tag)] -- the searches behind step k, lp a dict of ndt_loop_params fields, which a flag per session of the set -- and
the keys its certificate needs.

What was found while the table was made:
  empty_newest  ndt_sessions_step stores a step whose scan has no points as a zero-length newest scan (SsStep::book pushes
                scan_off.back() + 0), so the candidate of such a session IS searched with an empty scan: it scores nothing and
                picks nothing (status NDT_OK, n_cand 0, best -1), beside others that pick.  A call whose candidates all have an
                empty newest scan returns before anything is queued (N == 0).
  map_reuse     the issue's third search ("submap 0 again") would meet the first search's cloud again, point for point, while
                its certificate wants three different counts; the certificate is kept: the third search meets a later submap
                that is larger than the second's and differs from the first's.
  zero_pose     IN.  An out-and-back drive along x with heading 0 in steps of 0.5 m: every product of the reference's
                prediction (oracle.predict: the motion in the previous frame, then last (+) motion) is by cos 0 = 1 or
                sin 0 = 0 and every sum is of multiples of 0.5, so the poses are exact and the last one is bit-equal to
                (+0, +0, +0); tests/test_loop_shapes_host.py shows it with session_helpers.OracleSessions.
"""
import math

import numpy as np

import session_workloads as W
from loops_helpers import robot_frame
from session_helpers import lockstep, session_logs, to_map_frame

BEAMS = 181
LP = dict(min_path=0.0, radius=10.0, step_xy=0.1, step_yaw=math.radians(1.0), half=(2, 2, 1), top_k=8, local_max=0, max_cost=0.02)
GATE_KEYS = ("min_path", "radius", "step_xy", "step_yaw", "half")
INF = float("inf")


def lp(**kw):
    return dict(LP, **kw)


def gate_of(lp_):
    return {k: lp_[k] for k in GATE_KEYS}


def loop_params(capi, lp_):
    hx, hy, hk = lp_["half"]
    return capi.default_loop_params(min_path=lp_["min_path"], radius=lp_["radius"], step_xy=lp_["step_xy"], step_yaw=lp_["step_yaw"],
                                    half_x=hx, half_y=hy, half_yaw=hk, top_k=lp_["top_k"], local_max=lp_["local_max"],
                                    max_cost=lp_["max_cost"])


def launch(**kw):
    return W.launch_params(sepThre=1.0, score_thre=-1.0, **kw)


_DRIVES = {}


def _logs(specs, n_beams=BEAMS):
    """Copies of the drives (a drive is made once however many families take it)."""
    for spec in specs:
        if (spec, n_beams) not in _DRIVES:
            _DRIVES[(spec, n_beams)] = session_logs((spec,), n_beams=n_beams)[0]
    return [([x.copy() for x in _DRIVES[(spec, n_beams)][0]], _DRIVES[(spec, n_beams)][1].copy()) for spec in specs]


def _call(k, lp_, which, tag="", **more):
    """more (tests/loop_multi_shape_workloads.py): kind "multi" or "cross", mp (the ndt_loop_multi_params fields beside `loop`),
    against (a flag per session of the set, cross only); a call without them is a single search."""
    return dict(k=k, lp=lp_, which=list(which), tag=tag, **more)


def _family(name, logs, calls, cls=None, starts=None, tolerant=False, **more):
    return dict(name=name, logs=logs, starts=starts or [0] * len(logs), cls=list(cls) if cls is not None else list(range(len(logs))),
                p=launch(), tolerant=tolerant, calls=calls, **more)


# ---------------------------------------------------------------------------------------------- the families
RAGGED = (1, 63, 64, 65, 181, 257)                 # raw points of the last scans


def cut_scan(scan, n):
    """The first n points of a scan; beyond its length the scan tiled with 1 cm of jitter (tests/test_gpu_reloc.py)."""
    scan = np.asarray(scan, np.float64).reshape(-1, 2)
    if n <= len(scan):
        return scan[:n].copy()
    rng = np.random.default_rng(n)
    return np.tile(scan, (-(-n // len(scan)), 1))[:n] + rng.normal(0.0, 0.01, (n, 2))


def _ragged():
    logs = _logs([(33 + i, 6) for i in range(len(RAGGED))])
    for i, n in enumerate(RAGGED):
        logs[i][0][5] = cut_scan(logs[i][0][5], n)
    return _family("ragged", logs, [_call(5, lp(), [1] * len(RAGGED))])


def _dead_slots():
    logs = _logs(((33, 6), (34, 6)))
    return _family("dead_slots", logs, [_call(5, lp(half=(1, 1, 0), local_max=1), [1, 1], "nine"),
                                        _call(5, lp(half=(0, 0, 0), local_max=1), [1, 1], "one")])


FAR, FAR_SESSION = 500.0, 1


def _nothing_picked():
    logs = _logs(((33, 6), (34, 6), (35, 6)))
    logs[FAR_SESSION][0][5] = logs[FAR_SESSION][0][5] + np.array([FAR, 0.0])
    return _family("nothing_picked", logs, [_call(5, lp(), [1, 1, 1], "all"), _call(5, lp(), [1, 0, 1], "neighbours")], tolerant=True,
                   far=FAR_SESSION)


EMPTY_SESSIONS = (1, 2)


def _empty_newest():
    logs = _logs(((33, 6), (34, 6), (35, 6), (36, 6)))
    for i in EMPTY_SESSIONS:
        logs[i][0][5] = W.EMPTY
    return _family("empty_newest", logs, [_call(5, lp(), [1, 1, 1, 1], "mixed"), _call(5, lp(), [0, 1, 1, 0], "only_empty")],
                   empty=list(EMPTY_SESSIONS))


LATER_FRAMES = (6, 8, 10, 12)                       # behind step 11: 2, 3, 4 and 5 closed submaps -> the submaps 0, 1, 2, 3


def _later_submap():
    logs = _logs([(33 + i, n) for i, n in enumerate(LATER_FRAMES)])
    return _family("later_submap", logs, [_call(11, lp(), [1, 1, 1, 1])], submaps=[0, 1, 2, 3])


def _refused(name, bad):
    logs = _logs(((33, 6), (34, 6), (35, 6)))
    logs[bad][0][0] = np.concatenate([logs[bad][0][0], np.array([W.GRID_OUTLIER], np.float64)])
    return _family(name, logs, [_call(5, lp(), [1, 1, 1])], tolerant=True, bad=bad)


REUSE_THIN = (2, 3, 4, 5)                           # the scans that submap 2's cloud is made of, cut to every second beam
REUSE_STEPS = ((5, 0), (9, 2), (13, 4))             # (the step a search comes behind, the submap it meets)


def _map_reuse():
    logs = _logs(((33, 15),))
    for k in REUSE_THIN:
        logs[0][0][k] = logs[0][0][k][::2].copy()
    return _family("map_reuse", logs, [_call(k, lp(), [1], "search %d" % j) for j, (k, _) in enumerate(REUSE_STEPS)],
                   submaps=[m for _, m in REUSE_STEPS], twin=True)


def _picks_and_costs():
    logs = _logs(((33, 6), (34, 6)))
    calls = [_call(5, lp(top_k=k, local_max=m, max_cost=c), [1, 1], "top_k %d local_max %d max_cost %s" % (k, m, c))
             for k in (1, 8) for m in (0, 1) for c in (-INF, INF)]
    return _family("picks_and_costs", logs, calls)


MANY_S = 65
MANY_CLASSES = ((33, 6), (34, 8), (35, 10), (36, 6), (37, 8))           # behind step 9: the submaps 0, 1, 2, 0, 1


def _many():
    cls = [(7 * i + 3) % len(MANY_CLASSES) for i in range(MANY_S)]
    return _family("many", _logs(MANY_CLASSES), [_call(9, lp(), [1] * MANY_S)], cls=cls, submaps=[0, 1, 2, 0, 1])


ZERO_X = (0.0, 0.5, 1.0, 1.5, 2.0, 1.5, 1.0, 0.5, 0.0)                  # out and back along x, heading 0: reversing home


def _zero_pose():
    (scans, _), beside = _logs(((33, len(ZERO_X)),))[0], _logs(((34, len(ZERO_X)),))[0]      # (the circle's scans at the line's poses)
    odo = np.array([(x, 0.0, 0.0) for x in ZERO_X], np.float64)
    return _family("zero_pose", [(scans, odo), beside], [_call(len(ZERO_X) - 1, lp(), [1, 1])], zero=0)


FAMILIES = {
    "ragged": _ragged, "dead_slots": _dead_slots, "nothing_picked": _nothing_picked, "empty_newest": _empty_newest,
    "later_submap": _later_submap, "refused_first": lambda: _refused("refused_first", 0),
    "refused_middle": lambda: _refused("refused_middle", 1), "map_reuse": _map_reuse, "picks_and_costs": _picks_and_costs,
    "many": _many, "zero_pose": _zero_pose,
}
_MADE = {}


def family(name):
    if name not in _MADE:
        _MADE[name] = FAMILIES[name]()
    return _MADE[name]


# ---------------------------------------------------------------------------------------------- the host model
def host_run(fam):
    """The family on replay.PointCloudMap's bookkeeping alone, the odometry's prediction as the poses (session_schedules'
    model) -> per call {class: gate_ref's dict or None}, and the models behind the last step."""
    import session_schedules as SS          # (here: the device module takes the table alone)
    logs = fam["logs"]
    C = len(logs)
    pms, prev, out = [SS.host_map(fam["p"]["sepThre"]) for _ in range(C)], [None] * C, []
    for k, scans, odo, act in lockstep(logs, fam["starts"]):
        for c in range(C):
            if act[c]:
                SS.host_add(pms[c], odo[c], prev[c], k)
                prev[c] = odo[c].copy()
        for call in fam["calls"]:
            if call["k"] == k:
                named = sorted({fam["cls"][i] for i, w in enumerate(call["which"]) if w})
                out.append({c: SS.host_gate(pms[c], gate_of(call["lp"])) if len(pms[c].submaps) >= 3 else None for c in named})
    return out, pms


def stored_and_filtered(fam, c, pose):
    """Class c's last scan as the set stores it at `pose` (resampled, map frame, float32) and as a search filters it (robot
    frame, the pre-filter's host model): (stored points, filtered points)."""
    import prefilter_workloads as PW
    from ndt_slam_amd import replay
    p = fam["p"]
    raw = np.asarray(fam["logs"][c][0][-1], np.float64).reshape(-1, 2)
    if not len(raw):
        return 0, 0
    stored = to_map_frame(replay.resample_points(raw, p["space"], p["space_thre"]), pose).astype(np.float32)
    return len(stored), len(PW.model(robot_frame(stored, pose), p["LeafSize"]))
