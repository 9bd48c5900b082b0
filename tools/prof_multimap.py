"""Many SLAM sessions in one launch (ndt_align_batch_multi_dev): S sessions in the C1 shape -- a 360-point scan against a
5k-point local map, every session with its own map from its own seed, maps resident on one context -- timed three ways:
  (a) one ndt_align_batch_multi_dev call over the S maps;
  (b) S ndt_align_batch_dev calls with B = 1, back to back on one stream;
  (c) S ndt_align calls (host pointers, synchronous: the reference's one scan at a time).
Host clock around a synchronise, after 3 warm-up calls; median of --reps repeats for (a) and (b), of max(3, reps // 4) for
(c) (each entry records its count), ms per step and matches/s.  The records of
(a) are checked against (b)'s byte for byte.  --only a: (a) alone (for a kernel trace of it).
Usage: python tools/prof_multimap.py [--sessions 64,256] [--reps N] [--only a] [--json PATH]"""
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


def sessions(S):
    clouds, scans, inits = [], [], []
    for s in range(S):
        m = synth.make_map(CFG["n_map"], CFG["half"], seed=10_000 + s)
        scan, truth, init = synth.ScanFactory(m, CFG["half"], CFG["n_scan"]).make(s)
        clouds.append(m); scans.append(scan); inits.append(init)
    return clouds, scans, np.array(inits)


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
    ctx = capi.Context(0)
    prm = capi.default_params(resolution=CFG["resolution"])
    clouds, scans, inits = sessions(S)
    maps = [capi.Map(ctx, c, prm) for c in clouds]
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    d_sc = torch.from_numpy(np.concatenate(scans)).to(dev)
    d_of = torch.from_numpy(off).to(dev)
    d_in = torch.from_numpy(inits).to(dev)
    out_a = torch.zeros(S * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    out_b = torch.zeros(S * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    stream = torch.cuda.ExternalStream(ctx.stream)
    torch.cuda.synchronize()

    def sync():
        ctx.wait_launch(0, None)
        stream.synchronize()

    def a():
        ctx.align_batch_multi_dev(maps, None, d_sc.data_ptr(), d_of.data_ptr(), S, len(d_sc), d_in.data_ptr(),
                                  out_a.data_ptr())

    def b():
        for s in range(S):
            maps[s].align_batch_dev(d_sc.data_ptr(), d_of.data_ptr() + 8 * s, 1, len(d_sc), d_in.data_ptr() + 24 * s,
                                    out_b.data_ptr() + capi.RESULT_BYTES * s)

    def c():
        for s in range(S):
            maps[s].align(scans[s], inits[s])

    res = dict(sessions=S, points_per_scan=CFG["n_scan"], map_points=CFG["n_map"])
    forms = [("a_multi", a)] if only == "a" else [("a_multi", a), ("b_batch_dev_each", b), ("c_align_each", c)]
    for name, fn in forms:
        n = reps if name != "c_align_each" else max(3, reps // 4)      # (c): S synchronous calls per repeat, fewer repeats
        ms, ts = timed(fn, sync, n)
        res[name] = dict(ms_per_step=ms, matches_per_s=S / ms * 1e3, reps=n, spread_ms=[float(min(ts)), float(max(ts))])
    if only != "a":
        ra = out_a.cpu().numpy().tobytes()
        rb = out_b.cpu().numpy().tobytes()
        res["a_equals_b"] = ra == rb
        rec = np.frombuffer(ra, dtype=capi.RESULT_DTYPE)
        res["converged"] = int(rec["converged"].sum())
        res["speedup_a_over_b"] = res["b_batch_dev_each"]["ms_per_step"] / res["a_multi"]["ms_per_step"]
        res["speedup_a_over_c"] = res["c_align_each"]["ms_per_step"] / res["a_multi"]["ms_per_step"]
        a(); sync()
        mk, fk = ctx.kernel_timing(0)
        res["a_kernels_last_launch_ms"] = dict(match=mk, fitness=fk)
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
