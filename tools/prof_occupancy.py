"""ndt_occ_integrate_dev / ndt_occ_render_dev / ndt_sessions_occ_integrate on a scan set of the workload's shape.

Workload: --scans (256) scans of --beams (1081) beams over 270 degrees, ranges 0.5 .. 30 m (a room-like profile: most beams
long), res 0.05 m, 2048 x 2048 grids centred on the origins.  Three arrangements:
  per_scan   one grid per scan (grid_of = identity)
  shared     one grid for all scans (grid_of = NULL): every run's origin cell and the cells near it are contended
  sessions   --sessions (256) resident sessions (tools/prof_sessions.py's logs), ndt_sessions_occ_integrate behind every step
Figures: HIP events recorded on a stream of the tool's own around the call (so the table upload and occ_jobs_kernel are
inside), median of --reps after one warm-up; for `sessions` the host clock around the synchronous call with its stats
read-back, beside the host clock around that ndt_sessions_step.
  integrate_ms, updates (n_hit + n_pass of the call's stats), updates_per_s, atomic_bytes_per_s (4 bytes per update)
  render_ms and its share of 9 bytes per cell at --hbm-tbs (8.0)
Usage: python tools/prof_occupancy.py [--scans 256] [--beams 1081] [--reps 5] [--sessions 256] [--steps 8] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, replay      # noqa: E402

RES, N = 0.05, 2048
FLOAT_ATOMIC_TBS = 1.3      # chip-wide rate of no-return FLOAT atomic adds on the MI355X (public micro-architecture notes); the
                            # integer rate is not given there


def med(x):
    return float(np.median(np.asarray(x, dtype=np.float64)))


def make_scans(B, beams, seed=19):
    """B scans in the map frame around B origins near (0, 0): ranges 0.5 .. 30 m, piecewise smooth."""
    rng = np.random.default_rng(seed)
    origins = np.concatenate([rng.uniform(-2.0, 2.0, size=(B, 2)), rng.uniform(-180.0, 180.0, size=(B, 1))], axis=1)
    a = np.radians(np.linspace(-135.0, 135.0, beams))
    scans = []
    for b in range(B):
        knots = rng.uniform(0.5, 30.0, size=12)
        r = np.clip(np.interp(np.linspace(0, 11, beams), np.arange(12), knots) + rng.normal(0.0, 0.02, size=beams), 0.5, 30.0)
        th = a + np.radians(origins[b, 2])
        scans.append(np.stack([origins[b, 0] + r * np.cos(th), origins[b, 1] + r * np.sin(th)], axis=1).astype(np.float32))
    return scans, origins


def timed(torch, stream, fn, reps):
    out = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(stream.cuda_stream); e1.record(stream)
        e1.synchronize()
        if k:
            out.append(e0.elapsed_time(e1))
    return out


def batch_forms(args, torch, ctx, out):
    dev = torch.device("cuda", 0)
    B = args.scans
    scans, origins = make_scans(B, args.beams)
    xy = np.concatenate(scans)
    off = np.arange(B + 1, dtype=np.int64) * args.beams
    d_xy, d_off, d_org = torch.from_numpy(xy).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(origins).to(dev)
    d_gof = torch.arange(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(4, dtype=torch.int64, device=dev)
    geom = capi.OccGeometry(-N * RES / 2, -N * RES / 2, RES, N, N)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for name, n_grids in (("per_scan", B), ("shared", 1)):
        grids = [capi.OccGrid(ctx, geom) for _ in range(n_grids)]

        def call(st):
            capi.integrate_occ_dev(ctx, grids, d_gof.data_ptr() if n_grids > 1 else None, d_xy.data_ptr(), d_off.data_ptr(), B, len(xy),
                                   d_org.data_ptr(), 24, capi.DBL_MAX, d_st.data_ptr(), st)
        ms = timed(torch, stream, call, args.reps)
        st = d_st.cpu().numpy()
        upd = int(st[1] + st[2])
        m = med(ms)
        out[name] = dict(grids=n_grids, integrate_ms=m, integrate_ms_all=ms, n_beams=int(st[0]), n_skipped=int(st[3]), updates=upd,
                         updates_per_s=upd / (m * 1e-3), atomic_bytes_per_s=4.0 * upd / (m * 1e-3),
                         share_of_float_atomic_rate=4.0 * upd / (m * 1e-3) / (FLOAT_ATOMIC_TBS * 1e12))
        if name == "shared":
            d_img = torch.zeros(N * N, dtype=torch.int8, device=dev)
            torch.cuda.synchronize()
            rs = timed(torch, stream, lambda st: grids[0].render_dev(d_img.data_ptr(), 1, st), args.reps)
            floor_ms = 9.0 * N * N / (args.hbm_tbs * 1e12) * 1e3
            out["render"] = dict(render_ms=med(rs), render_ms_all=rs, bytes=9 * N * N, floor_ms_at_hbm=floor_ms,
                                 known_share=float((d_img.cpu().numpy() >= 0).mean()))
        for g in grids:
            g.close()


def sessions_form(args, torch, ctx, out):
    from prof_sessions import SEP_THRE, make_logs
    S, steps = args.sessions, args.steps
    p = dict(replay.LAUNCH_PARAMS, sepThre=SEP_THRE, end_frame=steps)
    logs = make_logs(S, steps)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    geom = capi.OccGeometry(-N * RES / 2, -N * RES / 2, RES, N, N)
    grids = [capi.OccGrid(ctx, geom) for _ in range(S)]
    t_step, t_occ, upd = [], [], []
    for k in range(steps):
        scans = [logs[i][k][0] for i in range(S)]
        odo = np.array([logs[i][k][1] for i in range(S)])
        t0 = time.perf_counter()
        recs = ses.step(scans, odo)
        t1 = time.perf_counter()
        st = ses.occ_integrate(grids, np.ascontiguousarray(recs["stepped"], np.uint8))
        t2 = time.perf_counter()
        t_step.append((t1 - t0) * 1e3); t_occ.append((t2 - t1) * 1e3); upd.append(int(st["n_hit"]) + int(st["n_pass"]))
    w = 3
    out["sessions"] = dict(sessions=S, steps=steps, warmup=w, step_ms=med(t_step[w:]), occ_integrate_ms=med(t_occ[w:]),
                           occ_share_of_step=med(t_occ[w:]) / med(t_step[w:]), updates=med(upd[w:]), step_ms_all=t_step,
                           occ_integrate_ms_all=t_occ)
    for g in grids:
        g.close()
    ses.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--beams", type=int, default=1081)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sessions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    ctx = capi.Context(0)
    out = dict(tool="tools/prof_occupancy.py", scans=args.scans, beams=args.beams, res=RES, grid=[N, N], reps=args.reps,
               origin_cell_aggregation="built in (one atomic per run); not measured without",
               float_atomic_rate_tbs=FLOAT_ATOMIC_TBS, integer_atomic_rate="not given in the notes")
    batch_forms(args, torch, ctx, out)
    if args.sessions > 0:
        sessions_form(args, torch, ctx, out)
    print(json.dumps({k: ({a: b for a, b in v.items() if not a.endswith("_all")} if isinstance(v, dict) else v) for k, v in out.items()}))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
