"""The device resampler (ndt_resample_batch_dev) alone: device time per call with HIP events (warm-up, median of
--reps repeats) for 256 synthetic 1081-beam scans at the launch-file parameters and for one long scan with no resync
point, next to the host mirror replay.resample_points on the same scans.  Every device result is checked against the
mirror, bit for bit.  Also prints what bounds the walk: the longest piece of each input in output points.
Usage: python tools/prof_resample.py [--reps N] [--long N] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, replay, synth      # noqa: E402

SPACE, SPACE_THRE = replay.LAUNCH_PARAMS["space"], replay.LAUNCH_PARAMS["space_thre"]


def longest_piece(scans):
    """Output points of the longest piece (the walk of one lane): pieces start at the first point of a scan and at
    every point whose step from its predecessor is at least max(space, space_thre)."""
    best = 0
    for s in scans:
        step = np.hypot(*np.diff(s, axis=0).T)
        starts = np.concatenate([[0], 1 + np.nonzero(step >= max(SPACE, SPACE_THRE))[0], [len(s)]])
        for a, b in zip(starts[:-1], starts[1:]):
            best = max(best, len(replay.resample_points(s[a:b], SPACE, SPACE_THRE)))
    return best


def measure(ctx, scans, reps, warmup=3):
    dev = torch.device("cuda", 0)
    B = len(scans)
    raw = np.concatenate(scans)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    cap = capi.resample_capacity(len(raw), SPACE, SPACE_THRE)
    d_raw, d_off = torch.from_numpy(raw).to(dev), torch.from_numpy(off).to(dev)
    d64 = torch.zeros((cap, 2), dtype=torch.float64, device=dev)
    d32 = torch.zeros((cap, 2), dtype=torch.float32, device=dev)
    d_oo = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    ctx.set_stream(st.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    torch.cuda.synchronize()
    for it in range(warmup + reps):
        e0.record(st)
        ctx.resample_batch_dev(d_raw.data_ptr(), 16, d_off.data_ptr(), B, len(raw), SPACE, SPACE_THRE, d64.data_ptr(),
                               d32.data_ptr(), d_oo.data_ptr(), d_st.data_ptr(), stream=st.cuda_stream)
        e1.record(st)
        torch.cuda.synchronize()
        if it >= warmup:
            ts.append(e0.elapsed_time(e1))
    ctx.set_stream(None)
    oo, o64, status = d_oo.cpu().numpy(), d64.cpu().numpy(), d_st.cpu().numpy()
    t = time.perf_counter()
    refs = [replay.resample_points(s, SPACE, SPACE_THRE) for s in scans]
    host_s = time.perf_counter() - t
    same = bool(np.all(status == 0)) and all(np.array_equal(o64[oo[b]:oo[b + 1]], refs[b]) for b in range(B))
    return dict(scans=B, raw_points=int(len(raw)), out_points=int(oo[-1]), device_ms_median=float(np.median(ts)),
                device_ms_min=float(np.min(ts)), device_ms_max=float(np.max(ts)), reps=len(ts),
                host_mirror_ms_per_scan=1e3 * host_s / B, host_mirror_ms_total=1e3 * host_s,
                longest_piece_outputs=longest_piece(scans), bit_equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--long", type=int, default=120000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    recs, _ = synth.replay_records(n_frames=256, n_beams=1081)
    batch = [np.ascontiguousarray(r["front"], dtype=np.float64) for r in recs]
    rng = np.random.default_rng(3)
    steps = rng.normal(0, 0.02, (a.long, 2))
    steps *= np.minimum(1.0, 0.2 / np.maximum(np.hypot(steps[:, 0], steps[:, 1]), 1e-12))[:, None]
    long_scan = steps.cumsum(0)                       # every step below max(space, space_thre): one piece
    torch.cuda.init()                                 # torch's runtime first, then the library's context (as the tests do)
    ctx = capi.Context(0)
    out = {"batch_256x1081": measure(ctx, batch, a.reps), "one_long_scan": measure(ctx, [long_scan], a.reps)}
    for k, r in out.items():
        per_out_us = 1e3 * r["device_ms_median"] / max(1, r["longest_piece_outputs"])
        r["device_us_per_output_of_longest_piece"] = per_out_us
        print("%-15s %4d scans %7d -> %7d points: device %.4f ms (median of %d; min %.4f, max %.4f) | host mirror %.3f ms "
              "per scan, %.1f ms in all | longest piece %d outputs (%.3f us each at the median) | bit-equal %s" % (
                  k, r["scans"], r["raw_points"], r["out_points"], r["device_ms_median"], r["reps"], r["device_ms_min"],
                  r["device_ms_max"], r["host_mirror_ms_per_scan"], r["host_mirror_ms_total"], r["longest_piece_outputs"],
                  per_out_us, r["bit_equal"]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if not all(r["bit_equal"] for r in out.values()):
        sys.exit("device result differs from replay.resample_points")


if __name__ == "__main__":
    main()
