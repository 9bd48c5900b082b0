"""Device-resident lockstep sessions (ndt_sessions_step) against the host path (replay.run_sessions) on the same logs:
S SLAM sessions replay synthetic drives (synth.replay_records, about 1200 points per scan, 40 steps, sepThre giving submaps
of about 12 scans), both paths stepped side by side in one process and ALTERNATING step by step (which goes first flips
every step).  The time of a step is the host clock around the synchronous step of each path:
  (a) one Sessions.step: raw scans and odometry up, the step records down;
  (b) one step of replay.run_sessions' loop (restated below, statement for statement): matchScanBegin per session, one
      estimate_poses, matchScanEnd per session, one ops.local_maps, FrontEnd.processEnd.
The first 3 steps warm up; the result is the median of the next --reps steps with min / max, every step's time is kept.
Done = at every S the slowest (a) repeat is faster than the fastest (b) repeat.  The two paths' poses are compared at the
end (1e-4 m / 1e-4 rad, the project's parity bound).  --only a: (a) alone (for a kernel trace of it).
Usage: python tools/prof_sessions.py [--sessions 16,64,256] [--steps 40] [--reps 20] [--only a] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, replay, synth      # noqa: E402
from ndt_slam_amd.pose_estimator import Scan2D, Pose2D, estimate_poses      # noqa: E402

N_BEAMS, STEP_M, SEP_THRE, N_DISTINCT = 1200, 0.3, 3.6, 8


def make_logs(S, steps):
    """S logs of `steps` scans; N_DISTINCT different drives, repeated over the sessions."""
    base = []
    for s in range(min(S, N_DISTINCT)):
        recs, _ = synth.replay_records(n_frames=steps, n_beams=N_BEAMS, step=STEP_M, seed=33 + s)
        base.append([(np.asarray(r["front"], np.float64).reshape(-1, 2), (r["x"], r["y"], r["th"]), r["stamp"]) for r in recs])
    return [base[s % len(base)] for s in range(S)]


def host_step(launchers, scans, ops):
    """One iteration of replay.run_sessions' loop over sessions that all have a scan (the batched path)."""
    need = []
    for L, scan in zip(launchers, scans):
        pred = L.frontEnd.smat.matchScanBegin(scan)
        if pred is not None:
            need.append((L, pred))
    if need:
        res = estimate_poses([L.smat.estim for L, _ in need], [q for _, q in need])
        for (L, _), (cost, est, cov) in zip(need, res):
            L.smat.matchScanEnd(cost, est, cov)
    leaf = launchers[0].pcmap.submaps[-1].LeafSize
    out = ops.local_maps([L.pcmap.localMapItem() for L in launchers], leaf)
    for L, (p_cloud, target, n_prev) in zip(launchers, out):
        L.pcmap.setLocalMap(p_cloud, target, n_prev)
    for L in launchers:
        L.frontEnd.processEnd()


def run(S, steps, reps, only, warmup=3):
    ctx = capi.Context(0)
    p = dict(replay.LAUNCH_PARAMS, sepThre=SEP_THRE, end_frame=steps)
    logs = make_logs(S, steps)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    launchers = None
    if only != "a":
        launchers = [replay.SlamLauncher(ctx, **p) for _ in range(S)]
        for L in launchers:
            L.pcmap.deferred = True
    t = {"a_resident": [], "b_run_sessions": []}
    stats, pts = [], []
    res_poses = [[] for _ in range(S)]
    for k in range(steps):
        scans = [logs[i][k][0] for i in range(S)]
        odo = np.array([logs[i][k][1] for i in range(S)])
        pts.append(float(np.mean([len(x) for x in scans])))

        def a():
            t0 = time.perf_counter()
            recs = ses.step(scans, odo)
            t["a_resident"].append((time.perf_counter() - t0) * 1e3)
            for i in range(S):
                res_poses[i].append(tuple(recs[i]["pose"]))
            st = ses.stats()
            stats.append(dict(h2d_bytes=int(st.h2d_bytes), d2h_bytes=int(st.d2h_bytes), host_waits=st.host_waits,
                              triples_run=st.triples_run, sessions_stepped=st.sessions_stepped))

        def b():
            host_scans = [Scan2D(logs[i][k][0].copy(), sid=logs[i][k][2], pose=Pose2D(*logs[i][k][1])) for i in range(S)]
            t0 = time.perf_counter()
            host_step(launchers, host_scans, ctx)
            t["b_run_sessions"].append((time.perf_counter() - t0) * 1e3)

        order = [a] if only == "a" else ([a, b] if k % 2 == 0 else [b, a])
        for fn in order:
            fn()
    res = dict(sessions=S, steps=steps, points_per_raw_scan=float(np.mean(pts)), sep_thre=SEP_THRE, warmup=warmup, reps=reps,
               stats_last_step=stats[-1], host_waits=sorted({s["host_waits"] for s in stats}))
    for name, ts in t.items():
        if not ts:
            continue
        rep = ts[warmup:warmup + reps]
        res[name] = dict(ms_per_step=float(np.median(rep)), spread_ms=[float(min(rep)), float(max(rep))],
                         repeats_ms=[round(x, 4) for x in rep], all_steps_ms=[round(x, 4) for x in ts])
    if only != "a":
        worst = [0.0, 0.0]
        for i, L in enumerate(launchers):
            for q, r in zip(L.frontEnd.get_poses(), res_poses[i]):
                worst[0] = max(worst[0], abs(q.tx - r[0]), abs(q.ty - r[1]))
                worst[1] = max(worst[1], abs(np.radians((q.th - r[2] + 180.0) % 360.0 - 180.0)))
        res["max_pose_difference"] = dict(m=worst[0], rad=worst[1])
        ra, rb = res["a_resident"], res["b_run_sessions"]
        res["speedup_a_over_b"] = rb["ms_per_step"] / ra["ms_per_step"]
        res["a_slowest_beats_b_fastest"] = bool(ra["spread_ms"][1] < rb["spread_ms"][0])
    ses.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="16,64,256")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = []
    for S in a.sessions.split(","):
        out.append(run(int(S), a.steps, a.reps, a.only))
        print(json.dumps({k: v for k, v in out[-1].items()}), flush=True)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
