"""Time of one ndt_sessions_correct over S sessions whose current submaps hold 12 scans, against the same work done session
by session with the single-submap entry points (ndt_repose_points_dev, ndt_make_map_dev, ndt_prefilter_batch_dev with one
scan, ndt_map_build_dev) on device copies of the same scans (LOG.md R33.1).  Host clock around calls that end in a device
synchronise; warm runs first, the two forms alternated, the median of the repeats.
python tools/sessions_correct_bench.py [--sessions 256] [--beams 541] [--reps 9] [--json PATH]"""
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


S, BEAMS, REPS, N_SCANS, N_LOGS = arg("--sessions", 256), arg("--beams", 541), arg("--reps", 9), 12, 8
p = dict(replay.LAUNCH_PARAMS, sepThre=1e9)
ctx = capi.Context(0)
dev = torch.device("cuda", 0)

logs = []
for seed in range(33, 33 + N_LOGS):
    recs, _ = synth.replay_records(n_frames=N_SCANS, n_beams=BEAMS, step=0.3, seed=seed)
    logs.append(([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs],
                 np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64)))
ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
for k in range(N_SCANS):
    recs = ses.step([logs[i % N_LOGS][0][k] for i in range(S)], np.array([logs[i % N_LOGS][1][k] for i in range(S)]))
    assert recs["stepped"].all() and not recs["status"].any()
traj = [ses.trajectory(i) for i in range(S)]
assert all(len(t[0]) == N_SCANS and t[3] == 0 for t in traj)


def adjusted(poses, sign):
    out = poses.copy()
    g = np.arange(1, len(out) + 1)[:, None] * sign
    return out + g * np.array([0.015, -0.010, 0.12])


# the per-session form's inputs: each session's 12 scans in the map frame (resampled, at the poses of its records), on the device
def map_frame(lps, pose):
    a = np.radians(pose[2])
    c, s = np.cos(a), np.sin(a)
    return np.stack([c * lps[:, 0] - s * lps[:, 1] + pose[0], s * lps[:, 0] + c * lps[:, 1] + pose[1]], axis=1).astype(np.float32)


rs = [[replay.resample_points(x, p["space"], p["space_thre"]) for x in logs[j][0]] for j in range(N_LOGS)]
per = []
params = capi.default_params(resolution=p["Resolution"], step_size=p["StepSize"], trans_eps=p["TransformationEpsilon"],
                             max_iter=p["MaximumIterations"], grid_margin=8)
for i in range(S):
    scans = [map_frame(rs[i % N_LOGS][k], traj[i][0][k]) for k in range(N_SCANS)]
    allp, off = capi.pack_scans(scans)
    n = len(allp)
    d = dict(xy=torch.from_numpy(allp).to(dev), off=off, d_off=torch.from_numpy(off.astype(np.int64)).to(dev), n=n,
             cloud=torch.zeros((n + 1, 2), dtype=torch.float32, device=dev), cnt=torch.zeros(1, dtype=torch.int64, device=dev),
             filt=torch.zeros((n + 1, 2), dtype=torch.float32, device=dev), foff=torch.zeros(2, dtype=torch.int64, device=dev),
             old=torch.from_numpy(traj[i][0].copy()).to(dev), new=[torch.from_numpy(adjusted(traj[i][0], sg)).to(dev) for sg in (1, -1)])
    per.append(d)
torch.cuda.synchronize()
for d in per:                                           # every session's map, to rebuild in place
    d["map"] = capi.Map(ctx, params=params, dev_ptr=d["xy"].data_ptr(), n=d["n"])
torch.cuda.synchronize()


def per_session(which):
    """repose -> make_map -> prefilter -> map build, one session after the other; the counts come down between the calls."""
    for d in per:
        capi.repose_points_dev(ctx, d["xy"].data_ptr(), 8, d["d_off"].data_ptr(), N_SCANS, d["old"].data_ptr(), d["new"][which].data_ptr(),
                               d["xy"].data_ptr(), 8)
        ctx.make_map_dev(d["xy"].data_ptr(), 8, d["off"], True, True, True, p["resol"], p["thre_neighbor"], d["cloud"].data_ptr(),
                         d["cnt"].data_ptr())
        torch.cuda.synchronize()
        nc = int(d["cnt"].item())
        coff = torch.tensor([0, nc], dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.prefilter_batch_dev(d["cloud"].data_ptr(), 8, coff.data_ptr(), 1, max(nc, 1), p["LeafSize"], d["filt"].data_ptr(), d["foff"].data_ptr())
        torch.cuda.synchronize()
        nf = int(d["foff"][1].item())
        d["map"].rebuild(dev_ptr=d["filt"].data_ptr(), n=nf)
        d["old"], d["new"][which] = d["new"][which], d["old"]          # (the next run moves them back)
    torch.cuda.synchronize()


state = {"sign": 1}


def one_call():
    new = {i: adjusted(ses.trajectory(i)[0], state["sign"]) for i in range(S)}
    t0 = time.perf_counter()
    st = ses.correct(new)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert not any(st.values())
    state["sign"] = -state["sign"]
    return dt * 1e3


def looped(which):
    t0 = time.perf_counter()
    per_session(which)
    return (time.perf_counter() - t0) * 1e3


for w in range(2):                                       # warm: both forms, both directions
    one_call()
    looped(w)
a, b = [], []
for r in range(REPS):
    a.append(one_call())
    b.append(looped(r % 2))
stats = ses.stats()
out = dict(sessions=S, beams=BEAMS, scans_per_submap=N_SCANS, points_per_session=int(np.mean([d["n"] for d in per])), reps=REPS,
           correct_ms=dict(median=float(np.median(a)), min=float(min(a)), max=float(max(a))),
           per_session_ms=dict(median=float(np.median(b)), min=float(min(b)), max=float(max(b))),
           host_waits=stats.host_waits, triples_run=stats.triples_run, h2d_bytes=int(stats.h2d_bytes), d2h_bytes=int(stats.d2h_bytes))
print(json.dumps(out), flush=True)
if "--json" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
ses.close()
