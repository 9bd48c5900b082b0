"""Times of the cross-session loop search (LOG.md R41.1) over S sessions that drive the lap of tests/loops_helpers.loop_workload
in one map frame (8 seeds of the 56-frame lap, 181 beams, sepThre 5):
  * the cross gate: ndt_cross_gate_batch (one upload, two launches, one read-back) against ndt_cross_gate looped over the
    searchers on the host, on the set's own read-outs and on tracks of --scans poses each (the lap's poses repeated with a
    little noise, cut into submaps of 9 scans) -- the product the gate is on the device for;
  * the whole call: ndt_sessions_find_cross_loops against what a caller composes without it -- the host gate per searcher, per
    searcher the newest scan into the robot frame and the pre-filter, per candidate a map rebuild, ndt_relocalize_dev and one
    ndt_fit_points_batch_dev with its records uploaded and its statistics read back.
Host clock around calls that end in a device synchronise; two warm rounds, the forms alternated, median and range of the repeats.
python tools/cross_loops_bench.py [--sessions 256] [--scans 1000] [--reps 9] [--json PATH]"""
import ctypes as C
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


S, SCANS, REPS, FRAMES, N_LOGS = arg("--sessions", 256), arg("--scans", 1000), arg("--reps", 9), 56, 8
p = dict(replay.LAUNCH_PARAMS, sepThre=5.0)
ctx = capi.Context(0)
dev = torch.device("cuda", 0)
lib = capi.lib()
mp = capi.default_loop_multi_params(radius=4.0, max_submaps=2, max_d2=0.09, min_overlap=0.5)
K = mp.max_submaps


def summary(x):
    return dict(median=float(np.median(x)), min=float(min(x)), max=float(max(x)))


def alternate(forms, reps=REPS):
    """{name: fn() -> ms}: two warm rounds, then `reps` rounds with the forms one after the other."""
    for _ in range(2):
        for fn in forms.values():
            fn()
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            t[k].append(fn())
    return {k: summary(v) for k, v in t.items()}


# ---- the gate on arrays: both forms through the library's own entry points, the marshalling done once
def gate_forms(tracks, last, newest, own):
    arr, keep = capi._cross_tracks(tracks)
    n, T = len(last), len(tracks)
    out_d, n_d = np.zeros((n, K), capi.CROSS_CANDIDATE_DTYPE), np.zeros(n, np.int32)
    out_h, n_h = np.zeros((n, K), capi.CROSS_CANDIDATE_DTYPE), np.zeros(n, np.int32)
    one = C.c_int()

    def device():
        t0 = time.perf_counter()
        ctx.check(lib.ndt_cross_gate_batch(ctx.h, last.ctypes.data, newest.ctypes.data, own.ctypes.data, n, C.addressof(arr), T, C.byref(mp),
                                           out_d.ctypes.data, n_d.ctypes.data), "ndt_cross_gate_batch")
        return (time.perf_counter() - t0) * 1e3

    def host():
        t0 = time.perf_counter()
        for i in range(n):
            rc = lib.ndt_cross_gate(last[i].ctypes.data, int(newest[i]), int(own[i]), C.addressof(arr), T, C.byref(mp),
                                    out_h[i].ctypes.data, C.byref(one))
            assert rc == 0
            n_h[i] = one.value
        return (time.perf_counter() - t0) * 1e3

    t = alternate(dict(device=device, host=host))
    out_h["cand"]["session"] = np.where(np.arange(K)[None, :] < n_h[:, None], np.arange(n)[:, None], 0)
    assert n_d.tobytes() == n_h.tobytes() and out_d.tobytes() == out_h.tobytes(), "the device gate is the host gate, to the byte"
    rows = sum(len(t_[1]) - 1 for t_ in tracks)
    poses = sum(int(t_[1][-1]) for t_ in tracks)
    return dict(searchers=n, tracks=T, rows=rows, pairs=n * rows, distance_evaluations=n * poses, candidates=int(n_d.sum()),
                device_ms=t["device"], host_ms=t["host"], keep=len(keep))


logs = []
for seed in range(33, 33 + N_LOGS):
    recs, _ = synth.replay_records(n_frames=FRAMES, n_beams=181, step=0.6, seed=seed)
    logs.append(([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs],
                 np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64)))
ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
for k in range(FRAMES):
    recs = ses.step([logs[i % N_LOGS][0][k] for i in range(S)], np.array([logs[i % N_LOGS][1][k] for i in range(S)]))
    assert recs["stepped"].all() and not recs["status"].any()

# (a) the gate on the set's own read-outs
trajs = [ses.trajectory(i) for i in range(S)]
parts = [ses.global_map(i)[1] for i in range(S)]
set_tracks = [(t[0], t[1], t[2], np.concatenate([[0], np.cumsum([len(c) for c in parts[i]])]).astype(np.uint64)) for i, t in enumerate(trajs)]
last = np.ascontiguousarray(np.stack([t[0][-1] for t in trajs]))
newest = np.array([len(t[0]) - 1 for t in trajs], np.int32)
own = np.arange(S, dtype=np.int32)
gate_set = gate_forms(set_tracks, last, newest, own)

# (b) the gate at the issue's scale: S tracks of SCANS poses
rng = np.random.default_rng(41)
long_tracks = []
for i in range(S):
    base = np.tile(trajs[i % N_LOGS][0], (SCANS // FRAMES + 1, 1))[:SCANS] + np.append(rng.normal(0.0, 0.05, 2), 0.0)
    first = np.arange(0, SCANS, 9, dtype=np.int32)
    ends = np.append(first[1:] - 1, SCANS - 1)
    long_tracks.append((np.ascontiguousarray(base), first, (first + (ends - first) // 2).astype(np.int32),
                        (np.arange(len(first) + 1) * 800).astype(np.uint64)))
last_long = np.ascontiguousarray(np.stack([t[0][-1] for t in long_tracks]))
gate_long = gate_forms(long_tracks, last_long, np.full(S, SCANS - 1, np.int32), own)

# (c) the whole call against the composition
cands = ses.cross_candidates(mp)
J = len(cands)
assert J == K * S, "every session stands in two closed submaps of other sessions"
params = capi.default_params(resolution=p["Resolution"], step_size=p["StepSize"], trans_eps=p["TransformationEpsilon"],
                             max_iter=p["MaximumIterations"], grid_margin=8)
zero = torch.zeros((1, 3), dtype=torch.float64, device=dev)


def map_frame(lps, pose):
    a = np.radians(pose[2])
    c, s = np.cos(a), np.sin(a)
    return np.stack([c * lps[:, 0] - s * lps[:, 1] + pose[0], s * lps[:, 0] + c * lps[:, 1] + pose[1]], axis=1).astype(np.float32)


per = []
for i in range(S):
    pose = trajs[i][0][-1]
    scan = map_frame(replay.resample_points(logs[i % N_LOGS][0][FRAMES - 1], p["space"], p["space_thre"]), pose)
    n = len(scan)
    per.append(dict(scan=torch.from_numpy(scan).to(dev), n=n, off=torch.tensor([0, n], dtype=torch.int64, device=dev),
                    pose=torch.from_numpy(pose.reshape(1, 3).copy()).to(dev), robot=torch.zeros((n, 2), dtype=torch.float32, device=dev),
                    filt=torch.zeros((n, 2), dtype=torch.float32, device=dev), foff=torch.zeros(2, dtype=torch.int64, device=dev)))
jobs = []
for c in cands:
    cloud = np.ascontiguousarray(parts[int(c["map_session"])][int(c["cand"]["submap"])])
    jobs.append(dict(base=per[int(c["cand"]["session"])], cloud=torch.from_numpy(cloud).to(dev), n_cloud=len(cloud),
                     lattice=capi.PoseLattice.from_buffer_copy(c["cand"]["lattice"].tobytes()),
                     stats=torch.zeros(capi.NDT_LOOP_MAX_CAND * 32, dtype=torch.uint8, device=dev)))
torch.cuda.synchronize()
for e in jobs:
    e["map"] = capi.Map(ctx, params=params, dev_ptr=e["cloud"].data_ptr(), n=e["n_cloud"])
torch.cuda.synchronize()
TF_AT = capi.RESULT_DTYPE.fields["T00"][1]
arr_set, keep_set = capi._cross_tracks(set_tracks)
lp = mp.loop


def composed():
    t0 = time.perf_counter()
    out, one = np.zeros(K, capi.CROSS_CANDIDATE_DTYPE), C.c_int()
    for i in range(S):
        assert lib.ndt_cross_gate(last[i].ctypes.data, int(newest[i]), i, C.addressof(arr_set), S, C.byref(mp), out.ctypes.data, C.byref(one)) == 0
    for d in per:
        capi.repose_points_dev(ctx, d["scan"].data_ptr(), 8, d["off"].data_ptr(), 1, d["pose"].data_ptr(), zero.data_ptr(), d["robot"].data_ptr(), 8)
        ctx.prefilter_batch_dev(d["robot"].data_ptr(), 8, d["off"].data_ptr(), 1, d["n"], p["LeafSize"], d["filt"].data_ptr(), d["foff"].data_ptr())
        torch.cuda.synchronize()
        d["nf"] = int(d["foff"][1].item())
    for e in jobs:
        d = e["base"]
        e["map"].rebuild(dev_ptr=e["cloud"].data_ptr(), n=e["n_cloud"])
        rec = e["map"].relocalize(None, e["lattice"], top_k=lp.top_k, local_max=bool(lp.local_max), dev_ptr=d["filt"].data_ptr(), n=d["nf"],
                                  stride=8)["records"]
        if len(rec):
            d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8)).to(dev)
            e["map"].fit_points_dev(d["filt"].data_ptr(), d["foff"].data_ptr(), len(rec), d["nf"], d_rec.data_ptr() + TF_AT, capi.RESULT_BYTES,
                                    mp.max_d2, None, e["stats"].data_ptr(), shared_scan=True)
            e["st"] = e["stats"].cpu()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


found = [0]


def one_call():
    t0 = time.perf_counter()
    loops = ses.find_cross_loops(mp)
    torch.cuda.synchronize()
    found[0] = int(loops["m"]["loop"]["found"].sum())
    return (time.perf_counter() - t0) * 1e3


def candidates_only():
    t0 = time.perf_counter()
    ses.cross_candidates(mp)
    return (time.perf_counter() - t0) * 1e3


whole = alternate(dict(find_cross_loops=one_call, cross_candidates=candidates_only, composed=composed))
ses.find_cross_loops(mp)
q = ses.stats()
out = dict(sessions=S, reps=REPS, gate_on_the_set=gate_set, gate_long_tracks=dict(gate_long, scans_per_track=SCANS),
           search=dict(candidates=J, found=found[0], find_cross_loops_ms=whole["find_cross_loops"], cross_candidates_ms=whole["cross_candidates"],
                       composed_ms=whole["composed"], host_waits=q.host_waits, h2d_bytes=int(q.h2d_bytes), d2h_bytes=int(q.d2h_bytes)))
print(json.dumps(out), flush=True)
if "--json" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
for e in jobs:
    e["map"].close()
ses.close()
