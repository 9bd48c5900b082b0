"""Every session's local map in one call (ndt_local_map_batch_dev): S SLAM sessions, each with a submap of 12 scans in the
map frame and the cloud of the submap before it, inputs resident on the device, timed two ways on one stream:
  (a) one ndt_local_map_batch_dev call over the S submaps;
  (b) the per-session path for the same work: per submap ndt_make_map_dev, a read-back of its count,
      ndt_prefilter_batch_dev with B = 1; then one read-back of the filtered counts and the device-to-device copies that
      put each previous cloud and filtered cloud together.
Host clock around a synchronise, after 3 warm-up calls each; the two paths ALTERNATE in one process, repeat by repeat;
median of --reps repeats with the spread (min, max) and every repeat's time, ms per step.  Before a time is printed (a)'s
three outputs -- clouds, targets and both offset arrays -- are checked against (b)'s byte for byte (behind the timed repeats:
the check's read-backs leave the device idle, and the first call after that ran 9-23 ms on the MI355X, LOG.md R11.1).  --only a: (a) alone (for a kernel trace of it).
Usage: python tools/prof_local_map_batch.py [--shapes 64x1200,256x1200,64x10000] [--reps N] [--only a] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, synth      # noqa: E402
from ndt_slam_amd.replay import LAUNCH_PARAMS      # noqa: E402

N_SCANS, N_PREV = 12, 5000
RESOL, THRE, LEAF = LAUNCH_PARAMS["resol"], LAUNCH_PARAMS["thre_neighbor"], LAUNCH_PARAMS["LeafSize"]


def run(S, n_points, reps, only, warmup=3):
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    st = torch.cuda.ExternalStream(ctx.stream)
    subs = []
    for s in range(S):
        scans = synth.submap_scans(N_SCANS, n_points, seed=21 + s)
        off = np.zeros(N_SCANS + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in scans])
        prev = synth.make_map(N_PREV, 8.0, seed=500 + s)
        subs.append(dict(d_all=torch.from_numpy(np.ascontiguousarray(np.concatenate(scans))).to(dev), off=off,
                         d_prev=torch.from_numpy(np.ascontiguousarray(prev)).to(dev)))
    descs = (capi.SubmapDesc * S)(*[
        capi.SubmapDesc(u["d_all"].data_ptr(), u["off"].ctypes.data, N_SCANS, 0, 1, 1, RESOL, THRE, u["d_prev"].data_ptr(),
                        len(u["d_prev"])) for u in subs])
    cap_cloud = sum(int(u["off"][-1]) for u in subs)
    cap_target = cap_cloud + sum(len(u["d_prev"]) for u in subs)

    def outputs():
        return dict(cloud=torch.zeros((cap_cloud + 1, 2), dtype=torch.float32, device=dev),
                    target=torch.zeros((cap_target + 1, 2), dtype=torch.float32, device=dev),
                    coff=torch.zeros(S + 1, dtype=torch.int64, device=dev), toff=torch.zeros(S + 1, dtype=torch.int64, device=dev),
                    status=torch.zeros(S, dtype=torch.int32, device=dev))

    A, B = outputs(), outputs()
    # (b)'s own scratch: every submap's filtered cloud at the place its capacity gives it, its offsets pair, the counts
    b_tmp = torch.zeros((cap_cloud + 1, 2), dtype=torch.float32, device=dev)
    b_raw = torch.zeros((S, 2), dtype=torch.int64, device=dev)            # {0, count of the cloud}: the filter's raw offsets
    b_flt = torch.zeros((S, 2), dtype=torch.int64, device=dev)            # {0, count of the filtered cloud}
    cap_at = np.concatenate([[0], np.cumsum([int(u["off"][-1]) for u in subs])])
    torch.cuda.synchronize()

    def a():
        ctx.local_maps_dev(descs, LEAF, A["cloud"].data_ptr(), A["coff"].data_ptr(), A["target"].data_ptr(),
                           A["toff"].data_ptr(), A["status"].data_ptr())

    def b():
        with torch.cuda.stream(st):
            coff = [0]
            for s, u in enumerate(subs):
                ctx.make_map_dev(u["d_all"].data_ptr(), 8, u["off"], False, True, True, RESOL, THRE,
                                 B["cloud"].data_ptr() + 8 * coff[-1], b_raw[s, 1:].data_ptr())
                n = int(b_raw[s, 1].item())                               # the count read-back (a host wait)
                coff.append(coff[-1] + n)
                ctx.prefilter_batch_dev(B["cloud"].data_ptr() + 8 * coff[-2], 8, b_raw[s].data_ptr(), 1, n, LEAF,
                                        b_tmp.data_ptr() + 8 * int(cap_at[s]), b_flt[s].data_ptr())
            cnt = b_flt[:, 1].cpu().numpy()                               # one read-back of the filtered counts
            toff = [0]
            for s, u in enumerate(subs):
                t0, np_, m = toff[-1], len(u["d_prev"]), int(cnt[s])
                B["target"][t0:t0 + np_].copy_(u["d_prev"], non_blocking=True)
                B["target"][t0 + np_:t0 + np_ + m].copy_(b_tmp[int(cap_at[s]):int(cap_at[s]) + m], non_blocking=True)
                toff.append(t0 + np_ + m)
            B["coff"].copy_(torch.from_numpy(np.array(coff, np.int64)), non_blocking=False)
            B["toff"].copy_(torch.from_numpy(np.array(toff, np.int64)), non_blocking=False)

    res = dict(sessions=S, scans_per_submap=N_SCANS, points_per_scan=n_points, prev_points=N_PREV, input_points=cap_cloud)
    paths = [("a_one_call", a)] if only == "a" else [("a_one_call", a), ("b_per_session", b)]
    for _ in range(warmup):
        for _, fn in paths:
            fn(); st.synchronize()
    ts, queued = {name: [] for name, _ in paths}, {name: [] for name, _ in paths}
    for _ in range(reps):
        for name, fn in paths:
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()                                      # the call has returned: everything is queued
            st.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
            queued[name].append((t1 - t0) * 1e3)
    for name, _ in paths:
        res[name] = dict(ms_per_step=float(np.median(ts[name])), reps=reps, spread_ms=[float(min(ts[name])), float(max(ts[name]))],
                         times_ms=[round(t, 4) for t in ts[name]], host_queue_ms=[round(t, 4) for t in queued[name]])
    # the check, behind the timed repeats (its read-backs leave the device idle for a while) and in front of every print
    if only != "a":
        same = all(A[k].cpu().numpy().tobytes() == B[k].cpu().numpy().tobytes() for k in ("coff", "toff", "status"))
        nc, nt = int(A["coff"][-1].item()), int(A["toff"][-1].item())
        same = same and A["cloud"][:nc].cpu().numpy().tobytes() == B["cloud"][:nc].cpu().numpy().tobytes()
        same = same and A["target"][:nt].cpu().numpy().tobytes() == B["target"][:nt].cpu().numpy().tobytes()
        res["a_equals_b"] = bool(same)
        res["cloud_points"], res["target_points"] = nc, nt
        if not same:
            raise SystemExit("prof_local_map_batch: (a) and (b) differ at S = %d, %d points per scan" % (S, n_points))
        res["speedup_a_over_b"] = res["b_per_session"]["ms_per_step"] / res["a_one_call"]["ms_per_step"]
        res["a_slowest_beats_b_fastest"] = bool(max(ts["a_one_call"]) < min(ts["b_per_session"]))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x1200,256x1200,64x10000", help="SESSIONSxPOINTS_PER_SCAN, comma separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = []
    for shape in a.shapes.split(","):
        S, n = shape.split("x")
        out.append(run(int(S), int(n), a.reps, a.only))
        print(json.dumps(out[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
