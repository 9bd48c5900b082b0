"""Time of one ndt_sessions_occ_rebuild over S sessions that have driven the lap of tests/loops_helpers.loop_workload (the 5 m
circle, 56 frames of 181 beams, sepThre 5; 8 seeds in turn), every session into a 500 x 500 grid of 0.1 m, against
  (a) what a caller can do without the archive, per session: the host form ndt_occ_integrate of all its scans (already
      resampled and in the map frame: the caller's own resampling and transform are not in the time), and
  (b) the unfused device composition over all sessions: ndt_scan_to_map_batch_dev of the archived points into a map-frame
      scratch, then one ndt_occ_integrate_dev;
and the same call on sessions that stand still (56 times their first scan at one pose: every beam of a session starts in one
cell and scans repeat their cells), the worst case for contention (LOG.md R35.1).  The three forms' grids are compared
counter for counter before anything is timed.  Host clock around calls that end in a device synchronise, every call behind
the clears of its grids; two warm rounds, the forms alternated, median and range of the repeats.
python tools/occ_rebuild_bench.py [--sessions 256] [--reps 9] [--json PATH]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ndt_slam_amd import capi, replay, synth  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


S, REPS, FRAMES, N_LOGS = arg("--sessions", 256), arg("--reps", 9), 56, 8
GEOM = capi.OccGeometry(-25.0, -25.0, 0.1, 500, 500)
ctx = capi.Context(0)
dev = torch.device("cuda", 0)

logs = []
for seed in range(33, 33 + N_LOGS):
    recs, _ = synth.replay_records(n_frames=FRAMES, n_beams=181, step=0.6, seed=seed)
    logs.append(([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs],
                 np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64)))


def drive(still):
    """A set with the archive behind FRAMES steps: the lap, or every session's first scan again and again at its first pose."""
    p = dict(replay.LAUNCH_PARAMS, sepThre=5.0, **({"score_thre": -1.0} if still else {}))
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p), archive=True)
    for k in range(FRAMES):
        f = 0 if still else k
        recs = ses.step([logs[i % N_LOGS][0][f] for i in range(S)], np.array([logs[i % N_LOGS][1][f] for i in range(S)]))
        assert recs["stepped"].all() and not recs["status"].any()
    return ses


def summary(x):
    return dict(median=float(np.median(x)), min=float(min(x)), max=float(max(x)))


def timed(fn, grids):
    for g in grids:
        g.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(still):
    ses = drive(still)
    grids = [capi.OccGrid(ctx, GEOM) for _ in range(S)]
    # the other forms' inputs: the archive and the trajectories as the set holds them
    arch = [ses.archive_scans(i) for i in range(S)]
    traj = [ses.trajectory(i)[0] for i in range(S)]
    n_scans = sum(len(a) for a in arch)
    robot, off = capi.pack_scans([x for a in arch for x in a], dtype=np.float64)
    poses = np.concatenate(traj)
    grid_of = np.repeat(np.arange(S, dtype=np.int32), [len(a) for a in arch])
    d_robot, d_off = torch.from_numpy(robot).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev)
    d_poses, d_gof = torch.from_numpy(poses).to(dev), torch.from_numpy(grid_of).to(dev)
    d_map = torch.zeros((len(robot), 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def rebuild():
        return ses.occ_rebuild(grids, clear=False)

    def unfused():
        ctx.scan_to_map_batch_dev(d_robot.data_ptr(), 16, d_off.data_ptr(), n_scans, len(robot), d_poses.data_ptr(), d_map.data_ptr())
        capi.integrate_occ_dev(ctx, grids, d_gof.data_ptr(), d_map.data_ptr(), d_off.data_ptr(), n_scans, len(robot), d_poses.data_ptr(), 24)

    # the map-frame scans on the host, for (a): the device's own float32 points
    unfused()
    torch.cuda.synchronize()
    h_map = d_map.cpu().numpy()
    first = np.concatenate([[0], np.cumsum([len(a) for a in arch])])
    per = [(np.ascontiguousarray(h_map[int(off[first[i]]):int(off[first[i + 1]])]),
            (off[first[i]:first[i + 1] + 1] - off[first[i]]).astype(np.uint64), np.ascontiguousarray(traj[i])) for i in range(S)]

    def per_session_host():
        for i, (xy, o, org) in enumerate(per):
            capi.integrate_occ(ctx, [grids[i]], xy, o, org)

    # the same counters from all three forms
    sample = range(0, S, max(S // 16, 1))
    want = {i: grids[i].counts() for i in sample}
    for fn in (rebuild, per_session_host):
        for g in grids:
            g.clear()
        fn()
        for i in sample:
            c = grids[i].counts()
            assert np.array_equal(c[0], want[i][0]) and np.array_equal(c[1], want[i][1]) and c[1].sum() > 1000, i
    for g in grids:
        g.clear()
    st = rebuild()
    forms = (("rebuild_ms", rebuild), ("unfused_dev_ms", unfused), ("per_session_host_ms", per_session_host))
    for _ in range(2):
        for _, fn in forms:
            timed(fn, grids)
    t = {name: [] for name, _ in forms}
    for _ in range(REPS):
        for name, fn in forms:
            t[name].append(timed(fn, grids))
    out = {name: summary(v) for name, v in t.items()}
    # NDT_OPT_WORKGROUPS: fewer workgroups in flight, fewer adders per cell
    for wg in (64, 128, 256):
        ctx.set_option(capi.OPT_WORKGROUPS, wg)
        timed(rebuild, grids)
        out["rebuild_wg%d_ms" % wg] = summary([timed(rebuild, grids) for _ in range(REPS)])
    ctx.set_option(capi.OPT_WORKGROUPS, 0)
    out.update(scans=n_scans, points=int(len(robot)), runs=int(sum((len(x) + 255) // 256 for a in arch for x in a)),
               stats={k: int(st[k]) for k in st.dtype.names}, table_bytes=64 * S + 32 * (n_scans + 1),
               archive_bytes=16 * int(len(robot)))
    for g in grids:
        g.close()
    ses.close()
    return out


out = dict(sessions=S, reps=REPS, frames=FRAMES, lib=os.path.basename(capi.LIB_PATH), lap=measure(False), still=measure(True))
print(json.dumps(out), flush=True)
if "--json" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
