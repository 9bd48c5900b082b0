"""Many maps in one set of launches (ndt_map_build_batch_dev): S SLAM sessions in the C1 shape -- a 5k-point local map and
a 360-point scan per session, maps resident on one context, rebuilt from two alternating clouds per session (the local map
refilled every step, src/PointCloudMap.cpp:119-131) -- timed three ways:
  (a) one ndt_map_build_batch_dev call over the S maps;
  (b) S ndt_map_build_dev calls, back to back on the context's stream;
  (c) a full lockstep match step: (a) plus one ndt_align_batch_multi_dev launch over the S maps, against (b) plus the same
      launch.
Host clock around a synchronise, after 3 warm-up calls; median of --reps repeats with the spread (min, max), ms per step.
The exports and the multi-map records of (a)'s maps are checked against (b)'s byte for byte.  --only a: (a) alone (for a
kernel trace of it).
Usage: python tools/prof_batch_build.py [--sessions 64,256] [--reps N] [--only a] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, synth      # noqa: E402

CFG = synth.CONFIGS["C1"]


def timed(fn, sync, reps, warmup=3):
    for _ in range(warmup):
        fn(); sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(); sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def run(S, reps, only):
    dev = torch.device("cuda", 0)
    prm = capi.default_params(resolution=CFG["resolution"])
    clouds, scans, inits = [], [], []
    for s in range(S):
        m = synth.make_map(CFG["n_map"], CFG["half"], seed=10_000 + s)
        scan, truth, init = synth.ScanFactory(m, CFG["half"], CFG["n_scan"]).make(s)
        clouds.append((m, m + np.float32([0.05, -0.04])))          # the two clouds a session's map alternates between
        scans.append(scan); inits.append(init)
    d_cl = [[torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for c in clouds] for k in (0, 1)]
    ptrs = [[t.data_ptr() for t in d_cl[k]] for k in (0, 1)]
    ns = [CFG["n_map"]] * S
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    d_sc = torch.from_numpy(np.concatenate(scans)).to(dev)
    d_of = torch.from_numpy(off).to(dev)
    d_in = torch.from_numpy(np.array(inits)).to(dev)
    out = torch.zeros(S * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)

    def contexts():
        ctx = capi.Context(0)
        return ctx, torch.cuda.ExternalStream(ctx.stream)

    ctx_a, st_a = contexts()
    maps_a = ctx_a.build_maps_dev(ptrs[0], ns, prm)
    turn = {"a": 0, "b": 0}
    torch.cuda.synchronize()

    sync_a = st_a.synchronize                                      # (the launches below do not defer their fitness kernels)

    def a():
        turn["a"] ^= 1
        ctx_a.build_maps_dev(ptrs[turn["a"]], ns, prm, maps_a)

    def launch(ctx, maps):
        ctx.align_batch_multi_dev(maps, None, d_sc.data_ptr(), d_of.data_ptr(), S, len(d_sc), d_in.data_ptr(), out.data_ptr())

    res = dict(sessions=S, map_points=CFG["n_map"], points_per_scan=CFG["n_scan"])
    ms, ts = timed(a, sync_a, reps)
    res["a_batch_build"] = dict(ms_per_step=ms, reps=reps, spread_ms=[float(min(ts)), float(max(ts))])
    a(); sync_a()
    res["a_build_ms_device"] = ctx_a.last_timing()[0]
    if only == "a":
        return res

    ctx_b, st_b = contexts()
    maps_b = [capi.Map(ctx_b, dev_ptr=ptrs[0][s], n=ns[s], params=prm) for s in range(S)]
    sync_b = st_b.synchronize

    def b():
        turn["b"] ^= 1
        for s in range(S):
            maps_b[s].rebuild(dev_ptr=ptrs[turn["b"]][s], n=ns[s])

    ms, ts = timed(b, sync_b, reps)
    res["b_build_each"] = dict(ms_per_step=ms, reps=reps, spread_ms=[float(min(ts)), float(max(ts))])
    res["speedup_a_over_b"] = res["b_build_each"]["ms_per_step"] / res["a_batch_build"]["ms_per_step"]

    ms, ts = timed(lambda: (a(), launch(ctx_a, maps_a)), sync_a, reps)
    res["c_step_batch_build"] = dict(ms_per_step=ms, reps=reps, spread_ms=[float(min(ts)), float(max(ts))])
    ms, ts = timed(lambda: (b(), launch(ctx_b, maps_b)), sync_b, reps)
    res["c_step_build_each"] = dict(ms_per_step=ms, reps=reps, spread_ms=[float(min(ts)), float(max(ts))])
    res["speedup_step"] = res["c_step_build_each"]["ms_per_step"] / res["c_step_batch_build"]["ms_per_step"]
    ms, ts = timed(lambda: launch(ctx_a, maps_a), sync_a, reps)
    res["launch_alone"] = dict(ms_per_step=ms, reps=reps, spread_ms=[float(min(ts)), float(max(ts))])

    # both sets built from the same clouds (their last turn), then the check
    if turn["a"] != turn["b"]:
        a(); sync_a()
    ok = True
    for s in range(S):
        ea, eb = maps_a[s].export(), maps_b[s].export()
        ok = ok and bytes(maps_a[s].info()) == bytes(maps_b[s].info()) and all(ea[k].tobytes() == eb[k].tobytes() for k in ea)
    launch(ctx_a, maps_a); sync_a()
    ra = out.cpu().numpy().tobytes()
    launch(ctx_b, maps_b); sync_b()
    rb = out.cpu().numpy().tobytes()
    res["a_equals_b"] = bool(ok and ra == rb)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = [run(int(s), a.reps, a.only) for s in a.sessions.split(",")]
    for r in out:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
