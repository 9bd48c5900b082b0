"""Time of one ndt_sessions_remake_closed over S sessions that have driven the lap of tests/loops_helpers.loop_workload (the 5 m
circle, 56 frames of 181 beams, sepThre 5; 8 seeds in turn: the workload of tools/occ_rebuild_bench.py), all named, behind a
correction of every session, against the composed chain of public calls a caller would use for the same clouds, per session:
ndt_sessions_archive_scans (to the host), the upload, ndt_scan_to_map_batch_dev, ndt_local_map_batch_dev over the session's
closed submaps, the offsets read back.  The chain's clouds are compared with the set's closed parts byte for byte on a sample
of the sessions before anything is timed.  The remake is idempotent, so every repeat does the same work.  Host clock around
calls that end in a device synchronise; two warm rounds, the forms alternated, median and range of the repeats.  Device
memory taken by the first call (its scratch and the context's, all grow-only) is read from the runtime's free-memory count.
python tools/remake_closed_bench.py [--sessions 256] [--reps 9] [--json PATH]"""
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
ctx = capi.Context(0)
dev = torch.device("cuda", 0)
P = dict(replay.LAUNCH_PARAMS, sepThre=5.0)

logs = []
for seed in range(33, 33 + N_LOGS):
    recs, _ = synth.replay_records(n_frames=FRAMES, n_beams=181, step=0.6, seed=seed)
    logs.append(([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs],
                 np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64)))

ses = capi.Sessions(ctx, S, capi.session_params_from_launch(P), archive=True)
for k in range(FRAMES):
    recs = ses.step([logs[i % N_LOGS][0][k] for i in range(S)], np.array([logs[i % N_LOGS][1][k] for i in range(S)]))
    assert recs["stepped"].all() and not recs["status"].any()
new = {}
for i in range(S):                                         # a loop's correction: the drift spread over every pose
    t = ses.trajectory(i)[0].copy()
    t += np.arange(1, len(t) + 1)[:, None] * np.array([0.0015, -0.0010, 0.012])
    new[i] = t
assert set(ses.correct(new).values()) == {capi.NDT_OK}
torch.cuda.synchronize()
free0 = torch.cuda.mem_get_info()[0]
assert set(ses.remake_closed(range(S)).values()) == {capi.NDT_OK}
torch.cuda.synchronize()
first_call_bytes = free0 - torch.cuda.mem_get_info()[0]
st = ses.stats()


def chain(i, keep=False):
    """Session i's closed clouds by the public calls -> the clouds (keep) or nothing."""
    traj, sub_first, _, _ = ses.trajectory(i)
    ranges = replay.closed_scan_ranges(sub_first, len(sub_first) - 1)
    last = ranges[-1][1]
    scans = ses.archive_scans(i, 0, last + 1)
    xy, off = capi.pack_scans(scans, dtype=np.float64)
    d_in, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev)
    d_pose = torch.from_numpy(np.ascontiguousarray(traj[:last + 1])).to(dev)
    d_map = torch.empty((len(xy), 2), dtype=torch.float32, device=dev)
    descs, cap = [], 0
    for m, (a, b) in enumerate(ranges):
        assert b >= a
        descs.append(capi.SubmapDesc(d_map.data_ptr(), off[a:].ctypes.data, b - a + 1, int(sub_first[m] == 0), 1,
                                     int(P["removeMoving"]), float(P["resol"]), float(P["thre_neighbor"]), None, 0))
        cap += int(off[b + 1] - off[a]) * (2 if b == a else 1)
    n = len(descs)
    d_cloud = torch.empty((cap + 1, 2), dtype=torch.float32, device=dev)
    d_target = torch.empty((cap + 1, 2), dtype=torch.float32, device=dev)
    d_coff, d_toff = (torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
    d_status = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                              # (the context works on a stream of its own)
    ctx.scan_to_map_batch_dev(d_in.data_ptr(), 16, d_off.data_ptr(), last + 1, len(xy), d_pose.data_ptr(), d_map.data_ptr())
    ctx.local_maps_dev(descs, P["LeafSize"], d_cloud.data_ptr(), d_coff.data_ptr(), d_target.data_ptr(), d_toff.data_ptr(),
                       d_status.data_ptr())
    torch.cuda.synchronize()
    toff = d_toff.cpu().numpy()
    assert not d_status.cpu().numpy().any()
    if keep:
        t = d_target.cpu().numpy()
        return [t[int(toff[m]):int(toff[m + 1])].copy() for m in range(n)]


sample = range(0, S, max(S // 16, 1))
for i in sample:
    got, want = ses.global_map(i)[1][:-1], chain(i, keep=True)
    assert len(got) == len(want) >= 2 and all(x.tobytes() == y.tobytes() and len(x) for x, y in zip(got, want)), i


def remake():
    ses.remake_closed(range(S))


def composed():
    for i in range(S):
        chain(i)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(x):
    return dict(median=float(np.median(x)), min=float(min(x)), max=float(max(x)))


forms = (("remake_closed_ms", remake), ("composed_chain_ms", composed))
for _ in range(2):
    for _, fn in forms:
        timed(fn)
t = {name: [] for name, _ in forms}
for _ in range(REPS):
    for name, fn in forms:
        t[name].append(timed(fn))
out = {name: summary(v) for name, v in t.items()}
n_closed = [len(ses.trajectory(i)[1]) - 1 for i in range(S)]
out.update(sessions=S, reps=REPS, frames=FRAMES, closed_submaps=int(sum(n_closed)), triples=int(st.triples_run),
           host_waits=int(st.host_waits), h2d_bytes=int(st.h2d_bytes), d2h_bytes=int(st.d2h_bytes),
           first_call_device_bytes=int(first_call_bytes), ratio=out["composed_chain_ms"]["median"] / out["remake_closed_ms"]["median"])
print(json.dumps(out), flush=True)
if "--json" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
ses.close()
